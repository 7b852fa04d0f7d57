"""Training the evaluation classifiers on the GPU: hig_softmax_xent, the `trainable=True` classes' gradients against the fp64
oracle under autograd (and against the reference's own gradients of tests/golden/g18_eval_train.npz), five Adam steps through
both routes against the reference's, and EvalModelTrainer.train end to end.

Bounds.  Gradients: ||got - ref|| <= 2e-4 ||ref|| + 1e-6 per parameter, the project's bound for this same layer backward
(tests/test_gpu_text_head.py).  Five steps: losses within 1e-5 relative of the reference's (the forward tolerance of these
models), the total update p_5 - p_0 within 10x the fp32 reference's own stored distance from the reference run in fp64, over
the concatenation of the trained parameters WITHOUT the key thirds [d:2d] of every in_proj_bias (gradient = rounding noise around
an exact zero, which Adam divides by itself).  hig_softmax_xent: `xent_bounds` below, from its operation count.
"""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hig_amd  # noqa: E402
from hig_amd.models.evaluation_models import softmax_xent  # noqa: E402
from oracle import fill  # noqa: E402
from oracle import eval_models_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
GOLD = os.path.join(ROOT, "tests", "golden")
UNUSED = {"init_pos_embedding", "time_embed.0.weight", "time_embed.0.bias", "time_embed.2.weight", "time_embed.2.bias"}
CLS = {"enc": hig_amd.MotionEncoder, "con": hig_amd.MotionConsistencyEvalModel}
CASES = {
    "tiny": R.EVAL_CASES["tiny"],                                                                         # head dim 8: VALU attention
    "mfma": dict(B=4, T=33, F=15, d=128, H=2, ff=128, L=2, num_frames=40, length=[33, 32, 1, 17]),       # head dim 64; S = 66 / 67
    "hd128": dict(B=2, T=20, F=15, d=256, H=2, ff=256, L=1, num_frames=24, length=[20, 3]),              # head dim 128
    "shortest": dict(B=1, T=2, F=15, d=64, H=8, ff=128, L=2, num_frames=16, length=[1]),
}


@functools.lru_cache(maxsize=None)
def golden(name="g18_eval_train.npz"):
    return np.load(os.path.join(GOLD, name))


def labels_for(B, C):
    return torch.tensor([(7 * b + 3) % C for b in range(B)], dtype=torch.int64)


def case_inputs(cname):
    c = CASES[cname]
    if cname == "tiny":
        return R.eval_inputs("tiny", c)
    x1 = fill.tensor_for("g18.x1." + cname, (c["B"], c["T"], c["F"]))
    x2 = fill.tensor_for("g18.x2." + cname, (c["B"], c["T"], c["F"]))
    return x1, x2, torch.tensor(c["length"], dtype=torch.int64)


def build(kind, cname, **kw):
    c = CASES[cname]
    m = CLS[kind](input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"], num_layers=c["L"],
                  num_heads=c["H"], **kw)
    m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def oracle(kind, cname, feat_weight):
    """fp64 oracle under autograd, computed once per (model, case, loss): (loss, {name: grad or None})."""
    c = CASES[cname]
    shapes = R.param_shapes(kind, c["F"], c["d"], c["ff"], c["L"], c["num_frames"])
    p = {k: fill.tensor_for(k, s).double().requires_grad_(True) for k, s in shapes.items()}
    x1, x2, length = case_inputs(cname)
    if kind == "enc":
        logits, feat = R.motion_encoder_forward(p, x1.double(), x2.double(), length, c["H"])
    else:
        logits, feat = R.consistency_forward(p, x1.double(), x2.double(), length, c["H"]), None
    loss = F.cross_entropy(logits, labels_for(c["B"], logits.shape[1]))
    if feat_weight:
        loss = loss + feat_weight * feat.square().sum()
    loss.backward()
    return loss.item(), {k: (None if v.grad is None else v.grad.detach()) for k, v in p.items()}


def run_model(m, kind, cname, feat_weight=0.0, inputs=None):
    """One forward + backward of the product through autograd -> (loss tensor, {name: grad or None})."""
    x1, x2, length = inputs if inputs is not None else case_inputs(cname)
    for p in m.parameters():
        p.grad = None
    out = m(x1.to(DEV), x2.to(DEV), length=length)
    logits, feat = out if kind == "enc" else (out, None)
    loss = F.cross_entropy(logits, labels_for(logits.shape[0], logits.shape[1]).to(DEV))
    if feat_weight:
        loss = loss + feat_weight * feat.square().sum()
    loss.backward()
    return loss.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def check_grads(got, ref, what):
    worst = (-1.0, "")
    for k, r in ref.items():
        if r is None:
            assert got[k] is None, "%s: %s has a gradient, the reference has none" % (what, k)
            continue
        err, scale = (got[k].double().cpu() - r.double()).norm().item(), r.double().norm().item()
        worst = max(worst, (err / (2e-4 * scale + 1e-6), k))
        assert err <= 2e-4 * scale + 1e-6, "%s: %s off by %.3e (|ref| %.3e)" % (what, k, err, scale)
    return worst


# ---- hig_softmax_xent -----------------------------------------------------------------------------------------------------
def xent_bounds(x, labels):
    """fp64 reference and per-element bounds of the kernel's arithmetic (u = 2^-24), row by row:
      e_c = expf(x_c - m): the difference carries u |x_c - m| into the argument, the exponential 2 u:  a_c = |x_c - m| + 2
      se = sum_c e_c over C terms: relative (abar + C) u, abar = sum_c p_c a_c
      row = m + logf(se) - x_label: (abar + C) u from se, 2 u |log se| for logf, u |lse| and u |row| for the two sums
      loss = mean of the rows: each wave adds ceil(B / 4) rows, three more sums and the product with fl(1 / B): (B / 4 + 6) u |loss|
      p_c = e_c / se: relative (a_c + abar + C + 1) u;  dlogits_c = (p_c - onehot) / B: u |p_c - onehot| for the difference, 2 u for / B
    plus 2e-38 absolute where expf underflows (x_c - m < -87)."""
    B, C = x.shape
    xd = x.double()
    m = xd.amax(1, keepdim=True)
    e = torch.exp(xd - m)
    se = e.sum(1, keepdim=True)
    p = e / se
    a = (xd - m).abs() + 2
    abar = (p * a).sum(1, keepdim=True)
    lse = (m + se.log()).squeeze(1)
    onehot = F.one_hot(labels, C).double()
    rows = lse - (xd * onehot).sum(1)
    row_err = U * ((abar.squeeze(1) + C) + 2 * se.log().abs().squeeze(1) + lse.abs() + rows.abs())
    loss = rows.mean()
    loss_err = row_err.mean() + (B / 4 + 6) * U * loss.abs()
    dl = (p - onehot) / B
    dl_err = U / B * (p * (a + abar + C + 1) + 3 * (p - onehot).abs()) + 2e-38
    return loss, loss_err, dl, dl_err


@pytest.mark.parametrize("B,C", [(1, 2), (3, 26), (70, 26), (5, 64)])
def test_softmax_xent(B, C):
    g = torch.Generator().manual_seed(100 * B + C)
    x = torch.randn(B, C, generator=g) * 2
    x[::2] = (torch.rand(B, C, generator=g)[::2] * 2 - 1) * 80           # every other row spread over +-80
    x[0, 0], x[0, C - 1] = 80.0, -80.0
    if B > 2:
        x[2, 1] = x[2, C - 1] = x[2].max() + 1                           # a tie: the first maximum is the prediction
    labels = labels_for(B, C)
    loss_ref, loss_err, dl_ref, dl_err = xent_bounds(x, labels)
    outs = [softmax_xent(x.to(DEV), labels) for _ in range(2)]
    loss, dl, pred = outs[0]
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])), "two calls differ"
    assert abs(loss.item() - loss_ref.item()) <= loss_err.item(), (loss.item(), loss_ref.item(), loss_err.item())
    err = (dl.double().cpu() - dl_ref).abs()
    print("xent B=%d C=%d: loss err / bound %.3f, dlogits err / bound %.3f" % (B, C, abs(loss.item() - loss_ref.item()) / loss_err.item(), (err / dl_err).max().item()))
    assert (err <= dl_err).all()
    assert torch.equal(pred.cpu(), x.argmax(1)) and (B <= 2 or pred[2].item() == 1)
    assert (dl.double().cpu().sum(1).abs() <= dl_err.sum(1)).all(), "rows of dlogits sum to 0"
    ref = F.cross_entropy(x.double(), labels)                             # the definition: nn.CrossEntropyLoss(), mean
    assert abs(ref.item() - loss_ref.item()) <= 1e-12 * (1 + abs(ref.item()))
    only_loss = softmax_xent(x.to(DEV), labels, want_dlogits=False)
    assert only_loss[1] is None and torch.equal(only_loss[0], loss) and torch.equal(only_loss[2], pred)


# ---- gradients of the two classes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", list(CASES))
@pytest.mark.parametrize("kind", ["enc", "con"])
def test_model_gradients_against_the_fp64_oracle(kind, cname):
    m = build(kind, cname, trainable=True).train()
    loss, got = run_model(m, kind, cname)
    ref_loss, ref = oracle(kind, cname, 0.0)
    assert abs(loss.item() - ref_loss) <= 1e-5 * abs(ref_loss)
    worst = check_grads(got, ref, "%s %s" % (kind, cname))
    assert {k for k, v in got.items() if v is None} == UNUSED
    c = CASES[cname]
    assert (got["sequence_embedding"][c["T"] - 1:] == 0).all(), "rows of sequence_embedding the forward never read"
    print("%s %s: loss rel %.1e, worst gradient at %.3f of its bound (%s)" % (kind, cname, abs(loss.item() - ref_loss) / abs(ref_loss), *worst))
    # padded tokens are never keys and reach no output: what they hold changes no bit of the loss or of any gradient
    x1, x2, length = case_inputs(cname)
    x1, x2 = x1.clone(), x2.clone()
    for b, n in enumerate(length.tolist()):
        x1[b, n:], x2[b, n:] = 3.25, -1.5
    loss2, got2 = run_model(m, kind, cname, inputs=(x1, x2, length))
    if any(n < c["T"] for n in length.tolist()):
        assert torch.equal(loss, loss2)
        for k, v in got.items():
            assert (v is None and got2[k] is None) or torch.equal(v, got2[k]), "%s changed with the padded tokens' features" % k


@pytest.mark.parametrize("kind", ["enc", "con"])
def test_tiny_gradients_against_the_reference_and_through_the_feature(kind):
    g, c = golden(), CASES["tiny"]
    m = build(kind, "tiny", trainable=True).train()
    loss, got = run_model(m, kind, "tiny")
    assert abs(loss.item() - float(g[kind + ".loss"])) <= 1e-5 * float(g[kind + ".loss"])
    ref = {k: (None if k in UNUSED else torch.from_numpy(g["%s.grad.%s" % (kind, k)])) for k in got}
    check_grads(got, ref, kind + " tiny vs the reference's own gradients")
    _, ref64 = oracle(kind, "tiny", 0.0)
    mults = []
    for k in got:   # each parameter's distance from the fp64 oracle as a multiple of the fp32 reference's own (its floor)
        if got[k] is not None:
            dist, floor = ((got[k].double().cpu() - ref64[k]).norm() / ref64[k].norm()).item(), float(g["%s.floor.%s" % (kind, k)])
            mults.append((dist / floor, k))
            print("%s tiny %-55s %.2e = %5.2f x floor %.2e" % (kind, k, dist, dist / floor, floor))
    print("%s tiny: worst distance from the fp64 oracle, in units of the fp32 reference's own (floor): %.2f (%s)" % (kind, *max(mults)))
    # softmax shift invariance: the key third of every in_proj_bias gradient is mathematically zero
    d = c["d"]
    for k in got:
        if k.endswith("in_proj_bias"):
            mine, theirs = got[k][d:2 * d].double().norm().item(), np.linalg.norm(g["%s.grad.%s" % (kind, k)][d:2 * d].astype(np.float64))
            print("%s %s key third: |got| %.2e, |reference| %.2e" % (kind, k, mine, theirs))
            assert mine <= 10 * theirs
    if kind == "enc":   # both outputs carry gradient
        loss_f, got_f = run_model(m, kind, "tiny", feat_weight=0.5)
        ref_loss, ref_f = oracle(kind, "tiny", 0.5)
        assert abs(loss_f.item() - ref_loss) <= 1e-5 * abs(ref_loss)
        check_grads(got_f, ref_f, "enc tiny, CE + 0.5 |feature|^2")
    for prec in ("bf16x3", "bf16"):
        mp = build(kind, "tiny", trainable=True, precision=prec).train()
        with pytest.raises(NotImplementedError):
            run_model(mp, kind, "tiny")
    # one backward per forward: the activations go back to the pool with the first
    x1, x2, length = case_inputs("tiny")
    out = m(x1.to(DEV), x2.to(DEV), length=length)
    loss = (out[0] if kind == "enc" else out).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="a second time"):
        loss.backward()
    out = m(x1.to(DEV), x2.to(DEV), length=length)
    with torch.no_grad():
        m.sequence_embedding.add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        (out[0] if kind == "enc" else out).sum().backward()


# ---- five Adam steps -----------------------------------------------------------------------------------------------------
def update_distance(upd, ref, d):
    """rel-L2 over the concatenation of the trained parameters, the key thirds of every in_proj_bias left out."""
    a, b = [], []
    for k, r in ref.items():
        u, r = upd[k].double().cpu().reshape(r.shape), r.double()
        if k.endswith("in_proj_bias"):
            u, r = torch.cat([u[:d], u[2 * d:]]), torch.cat([r[:d], r[2 * d:]])
        a.append(u.reshape(-1)), b.append(r.reshape(-1))
    a, b = torch.cat(a), torch.cat(b)
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("kind", ["enc", "con"])
def test_five_adam_steps_both_routes(kind):
    g, gu, c = golden(), golden("g18_eval_train_update.npz"), CASES["tiny"]
    x1, x2, length = case_inputs("tiny")
    x1, x2 = x1.to(DEV), x2.to(DEV)
    labels = labels_for(c["B"], 26 if kind == "enc" else 2)
    opt = types.SimpleNamespace(lr=2e-4, num_epochs=2, log_every=1, dim_pose=c["F"], model_dir="unused")
    ref_upd = {k[len(kind) + 7:]: torch.from_numpy(gu[k]) for k in gu.files if k.startswith(kind + ".upd64.")}
    floor = float(g[kind + ".upd_floor"])
    upds = {}
    for route in ("fused", "autograd"):
        m = build(kind, "tiny", trainable=True).train()
        p0 = {k: p.detach().clone() for k, p in m.named_parameters()}
        tr = hig_amd.EvalModelTrainer(opt, m, kind="encoder" if kind == "enc" else "consistency")
        step = tr.train_step_fused if route == "fused" else tr.train_step
        losses = [step(x1, x2, length, labels)[0] for _ in range(5)]
        losses = torch.stack(losses).double().cpu().numpy()
        rel = np.abs(losses - g[kind + ".losses"]) / g[kind + ".losses"]
        upd = upds[route] = {k: p.detach() - p0[k] for k, p in m.named_parameters()}
        dist = update_distance(upd, ref_upd, c["d"])
        print("%s %s: losses within %.1e of the reference's, update %.2e from the fp64 reference's = %.2f x the fp32 reference's own %.2e"
              % (kind, route, rel.max(), dist, dist / floor, floor))
        assert (rel <= 1e-5).all()
        assert dist <= 10 * floor
        assert set(ref_upd) == {k for k in p0 if k not in UNUSED}
        for k in UNUSED:
            assert torch.equal(dict(m.named_parameters())[k].detach(), p0[k]), "%s moved" % k
    between = update_distance(upds["fused"], {k: upds["autograd"][k].cpu() for k in ref_upd}, c["d"])
    print("%s: the two routes are %.2e apart (%.2f x the floor)" % (kind, between, between / floor))
    assert between <= 10 * floor


@pytest.mark.parametrize("kind", ["enc", "con"])
def test_fused_steps_with_a_shorter_batch_after_a_longer_one(kind):
    """T = 12, then T = 6 on the same flat gradient buffer: the backward writes rows [0, T - 1) of sequence_embedding's gradient,
    so the rows the longer batch wrote must be cleared: they are exact zeros, and the second step's gradient is what the autograd
    route computes from the same parameters, within the gradient bound of this file (the same kernels behind both; the routes
    differ in the rounding of d(loss) / d(logits): hig_softmax_xent against torch's cross_entropy backward)."""
    c = CASES["tiny"]
    x1, x2, length = case_inputs("tiny")
    labels = labels_for(c["B"], 26 if kind == "enc" else 2)
    opt = types.SimpleNamespace(lr=2e-4, num_epochs=2, log_every=1, dim_pose=c["F"], model_dir="unused")
    m = build(kind, "tiny", trainable=True).train()
    tr = hig_amd.EvalModelTrainer(opt, m, kind="encoder" if kind == "enc" else "consistency")
    tr.train_step_fused(x1.to(DEV), x2.to(DEV), length, labels)
    st = tr.fused_state()
    assert (st["gviews"][0][c["T"] - 1:] == 0).all() and (st["gviews"][0][:c["T"] - 1] != 0).any()
    after_one = {k: v.detach().clone() for k, v in m.state_dict().items()}
    short = (x1[:, :6].contiguous(), x2[:, :6].contiguous(), torch.tensor([6, 3, 1]))
    tr.train_step_fused(short[0].to(DEV), short[1].to(DEV), short[2], labels)
    names = {id(p): k for k, p in m.named_parameters()}
    fused = {names[id(p)]: gv.clone() for p, gv in zip(m.trained_parameters(), st["gviews"])}
    assert (fused["sequence_embedding"][5:] == 0).all(), "rows of sequence_embedding the T = 6 forward never read"
    m2 = build(kind, "tiny", trainable=True).train()
    m2.load_state_dict(after_one, strict=True)
    _, auto = run_model(m2, kind, "tiny", inputs=short)
    worst = check_grads(fused, {k: auto[k].cpu() for k in fused}, "%s fused vs autograd after a shorter batch" % kind)
    print("%s: fused vs autograd gradients of the T = 6 step, worst at %.4f of the bound (%s)" % (kind, *worst))


# ---- the loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["encoder", "consistency"])
def test_trainer_trains_saves_and_the_evaluator_reads_it(kind, tmp_path):
    short = "enc" if kind == "encoder" else "con"
    c = CASES["tiny"]
    m = build(short, "tiny", trainable=True)
    g = torch.Generator().manual_seed(5)
    motion1, motion2 = torch.randn(12, c["T"], c["F"] + 4, generator=g) * 0.1, torch.randn(12, c["T"], c["F"] + 4, generator=g) * 0.1
    lens = torch.tensor([12, 7, 1, 5] * 3)
    with torch.no_grad():   # labels the untrained model already gets right: the validation accuracy starts above zero
        out = m.eval()(motion1[:, :, :-4].to(DEV), motion2[:, :, :-4].to(DEV), length=lens)
        labels = (out[0] if kind == "encoder" else out).max(dim=1).indices.cpu()
    if kind == "encoder":
        batches = [(labels[i:i + 4], motion1[i:i + 4], motion2[i:i + 4], lens[i:i + 4], None) for i in (0, 4, 8)]
    else:
        batches = [(None, motion1[i:i + 4], motion2[i:i + 4], lens[i:i + 4], None, labels[i:i + 4]) for i in (0, 4, 8)]
    opt = types.SimpleNamespace(lr=2e-4, num_epochs=3, log_every=2, dim_pose=c["F"], model_dir=str(tmp_path / "model"))
    tr = hig_amd.EvalModelTrainer(opt, m, kind=kind)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x1d, x2d = motion1[:, :, :-4].to(DEV), motion2[:, :, :-4].to(DEV)
    saved, save = [], tr.save

    def save_and_remember(path):   # what the model computes, in .eval(), with the parameters that go into the file
        save(path)
        with torch.no_grad():
            saved.append(m.eval()(x1d, x2d, length=lens))

    tr.save = save_and_remember
    train_acc, val_acc = tr.train(batches, batches)
    assert len(train_acc) == len(val_acc) == 2 and tr.best_acc > 0 and saved
    assert any(not torch.equal(v, before[k]) for k, v in m.state_dict().items()), "nothing was trained"
    path = os.path.join(opt.model_dir, "best_eval_model.pth")
    fresh = build(short, "tiny")                                          # default-built: inference only
    fresh.load_state_dict(torch.load(path, map_location="cpu"), strict=True)
    other = build("con" if short == "enc" else "enc", "tiny")
    from hig_amd.datasets.evaluator import EvaluatorModelWrapper
    models = (fresh, other) if short == "enc" else (other, fresh)
    w = EvaluatorModelWrapper(types.SimpleNamespace(dataset_name="ntu_mul", device=DEV), models=models)
    fin, feat, cons = w.get_motion_embeddings(motion1, motion2, lens)
    if short == "enc":
        assert torch.equal(saved[-1][0], fin) and torch.equal(saved[-1][1], feat)
    else:
        assert torch.equal(saved[-1], cons)
