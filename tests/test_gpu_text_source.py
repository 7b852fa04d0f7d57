"""The four text sources of the training step on the MI355X (trainers/text_source.py): for every source, on the single-person
trainer and on the two-person trainer in PIT mode, the captured step is the fused step bit for bit -- loss, flat parameters,
both Adam moments, gradient norm and step counter -- over two steps with different text inputs of the same shape, out of ONE
graph.  The shapes are the smallest reference configurations (oracle/fill.py: config1, config1x2)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hig_amd  # noqa: E402
import class_head_worker as W  # noqa: E402
from oracle import fill  # noqa: E402
from test_gpu_caption_bank import CAPS, bits, build, pit_trainer, trainer  # noqa: E402

DEV = "cuda"
SOURCES = ("embeddings", "clip", "bank", "class_ids")


def twin_trainers(source, pit):
    """Two identical trainers (fused, captured) of the model this source trains, and the case's shapes."""
    if source == "class_ids":
        c = fill.ICASES["config1x2"]
        return c, [W.pit_trainer(c) for _ in range(2)]
    c = fill.ICASES["config1x2"] if pit else fill.CASES["config1"]
    kw = dict(caption_bank=16) if source == "bank" else {}
    if pit:
        models = [build(cls=hig_amd.MotionInteractionTransformer, c=c, **kw).train() for _ in range(2)]
        return c, [(pit_trainer(m), m) for m in models]
    models = [build(c=c, **kw).train() for _ in range(2)]
    return c, [(trainer(m), m) for m in models]


def motion_inputs(c, pit, k):
    """x0, noise, t, length of step k: the model batch is B rows, or the 2 B rows [motion1 | motion2] of B pairs."""
    shape = ((2 if pit else 1) * c["B"], c["T"], c["F"])
    x0 = (fill.tensor_for("src.x0.%d" % k, shape) * 10).to(DEV)
    noise = (fill.tensor_for("src.noise.%d" % k, shape) * 10).to(DEV)
    t = torch.tensor([(v + 123 * k) % 1000 for v in c["t"]], device=DEV)
    return x0, noise, t, torch.tensor(c["lengths"], device=DEV)


def captions(rows, k):
    """Step k's captions of the model batch's text rows; in PIT mode the rows are c1, c2, c2, c1."""
    if rows == 2:
        return [CAPS[2 * k], CAPS[2 * k + 1]]
    c1, c2 = [CAPS[4 * k], CAPS[4 * k + 1]], [CAPS[4 * k + 2], CAPS[4 * k]]
    return c1 + c2 + c2 + c1


def text_inputs(source, c, pit, k, tr, m):
    """The step's text keywords for this trainer (a bank request belongs to the model whose bank made it)."""
    rows = (4 if pit else 1) * c["B"]
    if source == "embeddings":
        return dict(xf_proj=(fill.tensor_for("src.xp.%d" % k, (rows, 4 * c["d"])) * 10).to(DEV),
                    xf_out=(fill.tensor_for("src.xo.%d" % k, (rows, c["N"], c["Lt"])) * 10).to(DEV))
    if source == "clip":
        clip_out, eot = tr.clip_inputs(captions(rows, k))
        return dict(clip_out=clip_out, eot=eot)
    if source == "bank":
        return dict(caption_batch=m.caption_bank.batch(captions(rows, k), DEV))
    return dict(class_ids=torch.tensor(W.PIT_IDS[k], dtype=torch.int32, device=DEV))


def assert_same_step(tf, mf, tc, mc, lf, lc, steps, what):
    torch.cuda.synchronize()
    sf, sc = tf.fused_state(), tc.fused_state()
    assert torch.equal(bits(lf), bits(lc)) and torch.isfinite(lf).all(), what
    assert torch.equal(bits(mf.flat_params().flat), bits(mc.flat_params().flat)), what
    assert torch.equal(bits(sf["m"]), bits(sc["m"])) and torch.equal(bits(sf["v"]), bits(sc["v"])), what
    assert torch.equal(bits(sf["gnorm"]), bits(sc["gnorm"])), what
    assert sf["step"].item() == sc["step"].item() == steps, what


CASES = [(s, pit) for s in SOURCES for pit in (False, True) if pit or s != "class_ids"]     # (class ids: the cap_id PIT model)


@pytest.mark.parametrize("source,pit", CASES, ids=["%s-%s" % (s, "pit" if p else "single") for s, p in CASES])
def test_captured_step_equals_the_fused_step_bit_for_bit_for_every_text_source(source, pit):
    c, ((tf, mf), (tc, mc)) = twin_trainers(source, pit)
    for k in range(2):
        x0, noise, t, length = motion_inputs(c, pit, k)
        lf = tf.train_step_fused(x0, t, length, noise=noise, **text_inputs(source, c, pit, k, tf, mf)).clone()
        lc = tc.train_step_captured(x0, t, length, noise=noise, **text_inputs(source, c, pit, k, tc, mc)).clone()
        assert_same_step(tf, mf, tc, mc, lf, lc, k + 1, (source, pit, k))
    graphs = tc.fused_state()["graphs"]
    assert len(graphs) == 1 and not tf.fused_state()["graphs"]              # one graph served both steps
    assert next(iter(graphs))[1] == source                                  # (the sources' kinds are their names here)


def test_one_trainer_fed_embeddings_and_then_clip_features_keeps_one_graph_for_each():
    """Same model, same shapes of the motion: the source is part of the key, and each graph's second replay (with other text
    inputs, behind a step of the other source) still equals the fused twin."""
    pit = False
    c, ((tf, mf), (tc, mc)) = twin_trainers("clip", pit)
    steps = 0
    for k in range(2):
        for source in ("embeddings", "clip"):
            x0, noise, t, length = motion_inputs(c, pit, k)
            lf = tf.train_step_fused(x0, t, length, noise=noise, **text_inputs(source, c, pit, k, tf, mf)).clone()
            lc = tc.train_step_captured(x0, t, length, noise=noise, **text_inputs(source, c, pit, k, tc, mc)).clone()
            steps += 1
            assert_same_step(tf, mf, tc, mc, lf, lc, steps, (source, k))
            assert len(tc.fused_state()["graphs"]) == (1 if (k, source) == (0, "embeddings") else 2)
    assert sorted(key[1] for key in tc.fused_state()["graphs"]) == ["clip", "embeddings"]
