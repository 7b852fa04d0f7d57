"""The EMA of the weights on the MI355X (include/hig.h, 'EMA weights'): hig_clip_adam_ema / hig_ema_update / hig_swap_f32
against tests/ema_bounds.py, then the trainer: the three training routes, bf16 storage, the `ema_weights()` scope, sampling
with `set_sampler(weights="ema")`, checkpoints and the two-person trainer.  References and bounds are evaluated in fp64 on
the device (plain torch): 4194307 elements per case would otherwise spend the test's time on the host.

Largest |error| / bound measured on an MI355X (the RATIO lines of `pytest -s`):
    hig_clip_adam_ema.ema                 1.000 (n4194307), 0.959 (n1027), 0.406 (n3): the blend is one fma, so the error is the
                                          rounding of e' alone and reaches the bound's u |e'| term at the foot of a binade
    train_step_fused.ema, update.ema      0.297 over five steps (errors of successive steps do not line up)
    resume.ema 0.596, ema-less checkpoint.first update 0.999, DDPMMulTrainer.train_step_fused.ema 0.997"""
import ctypes as C
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import hig_amd  # noqa: E402
from hig_amd import _lib  # noqa: E402
from oracle import fill  # noqa: E402
import ema_bounds as eb  # noqa: E402
from test_gpu_rowops_contract import Buf, P, S, held, ok, lib  # noqa: E402
from test_gpu_trainer_state import build, trainer, step_inputs, run_steps  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
ADAM = dict(lr=2e-4, b1=0.9, b2=0.999, eps=1e-8)
DECAY = 0.999
C1 = fill.CASES["config1"]


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ----------------------------------------------------------------------------------------------------------------------
# kernel contract
# ----------------------------------------------------------------------------------------------------------------------
class Off:
    """n floats that start `off` floats behind a 16-byte boundary, NaN around them."""

    def __init__(self, src, off):
        n = src.numel()
        self.n, self.off = n, off
        self.buf = torch.full((n + 16,), float("nan"), device=DEV)
        self.out = self.buf[4 + off:4 + off + n]
        self.out.copy_(src)
        assert self.out.data_ptr() % 16 == 4 * off

    def p(self):
        return C.c_void_p(self.out.data_ptr())

    def around(self, what):
        assert torch.isnan(self.buf[:4 + self.off]).all() and torch.isnan(self.buf[4 + self.off + self.n:]).all(), \
            "%s: a store landed outside the %d elements" % (what, self.n)
        assert not torch.isnan(self.out).any(), "%s: NaN inside" % what


def adam_state(n):
    g = torch.Generator(device=DEV).manual_seed(n)
    p = torch.randn(n, generator=g, device=DEV)
    return dict(p=p, m=0.1 * torch.randn(n, generator=g, device=DEV), v=0.01 * torch.rand(n, generator=g, device=DEV),
                g=0.3 * torch.randn(n, generator=g, device=DEV), e=p + 1e-3 * torch.randn(n, generator=g, device=DEV))


def run_update(host, n, step, with_shadow, ema=None):
    """hig_sumsq_partial + hig_clip_adam_shadow (ema None) or hig_clip_adam_ema on guarded copies of `host`, the device counter
    preset to `step`; -> the guarded buffers."""
    bufs = {k: Buf.flat(n) for k in ("p", "m", "v")}
    for k in bufs:
        bufs[k].out.copy_(host[k].view(1, -1))
    state = Buf.flat(2)       # {float gnorm; int32 step}
    state.out.zero_()
    state.out.view(torch.int32)[0, 1] = step
    scratch = Buf.flat(_lib.NORM_BLOCKS)
    ok(lib().hig_sumsq_partial(P(host["g"]), n, 1.0, scratch.p(), S()))
    shadow_n = n // 4 * 4 if with_shadow else 0
    shadow = Buf.flat(max(shadow_n, 4), BF16)
    lr_dev = torch.tensor([ADAM["lr"]], device=DEV)
    args = (bufs["p"].p(), P(host["g"]), bufs["m"].p(), bufs["v"].p(), n, 1.0, P(lr_dev), ADAM["b1"], ADAM["b2"], ADAM["eps"],
            0.5, 1.0, scratch.p(), state.p(), state.p(1), shadow.p() if with_shadow else None, shadow_n)
    if ema is None:
        ok(lib().hig_clip_adam_shadow(*args, S()))
    else:
        decay, warmup, origin = ema
        bufs["e"] = Buf.flat(n)
        bufs["e"].out.copy_(host["e"].view(1, -1))
        ok(lib().hig_clip_adam_ema(*args, bufs["e"].p(), decay, warmup, origin, S()))
    bufs.update(state=state, shadow=shadow, shadow_n=shadow_n)
    return bufs


@pytest.mark.parametrize("with_shadow", (False, True))
@pytest.mark.parametrize("n", eb.SIZES)
def test_fused_update_keeps_adam_bits_and_holds_the_ema(n, with_shadow):
    """Steps 0, 1, 2 x ema_origin 0, 1 x warm-up on / off.  p, m, v, shadow and gnorm: the bits of hig_clip_adam_shadow; ema
    within the bound; the guard bands (NaN patterns behind n, in every buffer) intact and never blended in; hig_ema_update on
    the same p' at the same update number (device counter, and host count), aligned or one float off: the same bits."""
    host = adam_state(n)
    for step in (0, 1, 2):
        want = run_update(host, n, step, with_shadow)
        p_new = want["p"].written("hig_clip_adam_shadow p")[0].to(DEV)
        for origin in (0, 1):
            for warmup in (0, 1):
                what = "hig_clip_adam_ema n%d_step%d_origin%d_warmup%d%s" % (n, step, origin, warmup, "_shadow" if with_shadow else "")
                got = run_update(host, n, step, with_shadow, ema=(DECAY, warmup, origin))
                for k in ("p", "m", "v"):
                    assert same_bits(got[k].written(what + " " + k), want[k].out.cpu()), "%s: %s differs from hig_clip_adam_shadow" % (what, k)
                got["state"].guards(what)
                assert same_bits(got["state"].out, want["state"].out), what + ": gnorm / step differ"
                assert got["state"].out.view(torch.int32)[0, 1].item() == step + 1
                if got["shadow_n"]:
                    assert same_bits(got["shadow"].written(what + " shadow"), want["shadow"].out.cpu())
                else:
                    got["shadow"].untouched(what + " shadow")
                e_new = got["e"].written(what + " ema")[0].to(DEV)       # (guards intact, no NaN leaked in)
                ref, bound = eb.ema_step_bound(host["e"], p_new, step, origin, DECAY, warmup)
                held(what.replace(" ", ".ema ", 1), e_new, ref, bound)
                # the stand-alone pass: the counter has been incremented by now; and the host count
                n_upd = eb.update_number(step, origin)
                for off in (0, 1):
                    for dev_count in (True, False):
                        e2, p2 = Off(host["e"], off), Off(p_new, off)
                        ok(lib().hig_ema_update(e2.p(), p2.p(), n, DECAY, warmup, got["state"].p(1) if dev_count else None, origin,
                                                n_upd if not dev_count else -7, S()))
                        e2.around(what + " hig_ema_update")
                        p2.around(what + " hig_ema_update p")
                        assert same_bits(e2.out, e_new), "%s: hig_ema_update (offset %d, %s count) differs from the fused ema" % (
                            what, off, "device" if dev_count else "host")
                        assert same_bits(p2.out, p_new)


@pytest.mark.parametrize("n", eb.SIZES)
def test_swap_is_exact_and_its_own_inverse(n):
    g = torch.Generator(device=DEV).manual_seed(n)
    a0, b0 = torch.randn(n, generator=g, device=DEV), torch.randn(n, generator=g, device=DEV)
    a0[0], b0[n - 1] = -0.0, float("inf")
    for oa, ob in ((0, 0), (1, 0), (0, 1), (1, 1)):
        a, b = Off(a0, oa), Off(b0, ob)
        ok(lib().hig_swap_f32(a.p(), b.p(), n, S()))
        for x in (a, b):
            x.around("hig_swap_f32 n%d offsets %d %d" % (n, oa, ob))
        assert same_bits(a.out, b0) and same_bits(b.out, a0)
        ok(lib().hig_swap_f32(a.p(), b.p(), n, S()))
        assert same_bits(a.out, a0) and same_bits(b.out, b0)
    a = Off(a0, 0)
    assert lib().hig_swap_f32(a.p(), C.c_void_p(a.out.data_ptr() + 4 * (n - 1)), n, S()) != 0      # overlapping: refused, untouched
    torch.cuda.synchronize()
    assert same_bits(a.out, a0)


# ----------------------------------------------------------------------------------------------------------------------
# training routes
# ----------------------------------------------------------------------------------------------------------------------
EMA_OPT = dict(ema_decay=DECAY, ema_warmup=True)


def flat_of(tr):
    return tr.encoder.flat_params().flat


def fused_steps(tr, steps, captured=False):
    """run_steps, keeping (parameters, loss) after every step."""
    snaps, losses = [], []
    for i in steps:
        run_steps(tr, [i], captured)
        snaps.append(flat_of(tr).clone())
        losses.append(tr.fused_state()["loss"].clone())
    return snaps, losses


@pytest.fixture(scope="module")
def trained():
    """Five fused steps on config1 without and with the EMA, and the captured route with it.  Read-only for the tests."""
    off, on, cap = (trainer(build().train(), **o) for o in ({}, EMA_OPT, EMA_OPT))
    e0 = flat_of(on).clone()
    r = dict(off=off, on=on, cap=cap, e0=e0)
    r["off_snaps"], r["off_loss"] = fused_steps(off, range(5))
    r["on_snaps"], r["on_loss"] = fused_steps(on, range(5))
    r["cap_snaps"], r["cap_loss"] = fused_steps(cap, range(5), captured=True)
    return r


def test_ema_leaves_the_fused_step_alone_and_follows_the_recurrence(trained):
    off, on = trained["off"], trained["on"]
    for a, b in zip(trained["off_snaps"] + trained["off_loss"], trained["on_snaps"] + trained["on_loss"]):
        assert same_bits(a, b)
    for k in ("m", "v", "step", "gnorm"):
        assert torch.equal(off.fused_state()[k], on.fused_state()[k]), k
    assert off.ema_state() is None and off._ema is None
    st = on.ema_state()
    assert (st["origin"], st["num_updates"], st["decay"], st["warmup"]) == (0, 5, DECAY, True)
    ref, bound = eb.ema_recurrence(trained["e0"], trained["on_snaps"], 0, 0, DECAY, 1)
    held("train_step_fused.ema", st["flat"], ref, bound)
    assert not same_bits(st["flat"], flat_of(on)) and not same_bits(st["flat"], trained["e0"])


def test_captured_step_equals_the_fused_step_with_the_ema(trained):
    """Fails when the capture warm-up's step leaks into the EMA or its count."""
    on, cap = trained["on"], trained["cap"]
    for a, b in zip(trained["on_snaps"] + trained["on_loss"], trained["cap_snaps"] + trained["cap_loss"]):
        assert same_bits(a, b)
    assert same_bits(on.ema_state()["flat"], cap.ema_state()["flat"])
    assert cap.ema_state()["num_updates"] == 5 and cap.ema_state()["origin"] == 0
    assert cap.fused_state()["step"].item() == 5
    for k in ("m", "v"):
        assert torch.equal(on.fused_state()[k], cap.fused_state()[k])


def test_update_route_follows_the_recurrence():
    """forward-side autograd + torch.optim.Adam + hig_ema_update with the host count."""
    m = build().train()
    tr = trainer(m, **EMA_OPT)
    tr.opt_encoder = torch.optim.Adam(m.parameters(), lr=2e-4)
    e0 = flat_of(tr).clone()
    snaps = []
    for i in range(5):
        x0, t, ln, xp, xo, nz = step_inputs(i)
        out = tr.diffusion.training_losses(m, x0, t, model_kwargs={"xf_proj": xp, "xf_out": xo, "length": ln}, noise=nz)
        tr.real_noise, tr.fake_noise = out["target"], out["pred"]
        tr.src_mask = m.generate_src_mask(C1["T"], ln).to(DEV)
        tr.update()
        snaps.append(flat_of(tr).clone())
    st = tr.ema_state()
    assert st["num_updates"] == 5 and not same_bits(snaps[0], e0)
    ref, bound = eb.ema_recurrence(e0, snaps, 0, 0, DECAY, 1)
    held("update.ema", st["flat"], ref, bound)


# ----------------------------------------------------------------------------------------------------------------------
# bf16 storage
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("captured", (False, True))
def test_bf16_storage_shadow_and_a_step_after_the_scope(captured):
    from test_gpu_bf16_training import make_trainer
    c = fill.CASES["width"]
    gi = {k: v.to(DEV) for k, v in fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"]).items()}
    g = torch.Generator().manual_seed(5)
    noises = [torch.randn(gi["x"].shape, generator=g).to(DEV) for _ in range(3)]
    a, b = make_trainer(c, "bf16"), make_trainer(c, "bf16")
    b.opt.ema_decay = DECAY

    def step(tr, k):
        f = tr.train_step_captured if captured else tr.train_step_fused
        f(gi["x"], gi["t"], gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"], noise=noises[k])

    for k in range(2):
        step(a, k)
        step(b, k)
        fa, fb = a.encoder.flat_params(), b.encoder.flat_params()
        assert same_bits(fa.flat, fb.flat)
        assert same_bits(fa.shadow16_buffer(), fb.shadow16_buffer())
        assert same_bits(fb.shadow16_buffer(), fb.flat[:fb.core_numel].to(BF16))
    assert not same_bits(b.ema_state()["flat"], fb.flat)
    b.encoder.eval()
    with b.ema_weights():
        with torch.no_grad():      # a forward inside: the shadow is re-derived from the averaged weights
            b.encoder(gi["x"], gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"])
        assert same_bits(fb.shadow16_buffer(), fb.flat[:fb.core_numel].to(BF16)) and not same_bits(fa.flat, fb.flat)
    b.encoder.train()
    assert same_bits(fa.flat, fb.flat)
    step(a, 2)
    step(b, 2)
    assert same_bits(fa.flat, fb.flat) and same_bits(fa.shadow16_buffer(), fb.shadow16_buffer())
    assert same_bits(a.fused_state()["loss"], b.fused_state()["loss"])


# ----------------------------------------------------------------------------------------------------------------------
# scope, sampling
# ----------------------------------------------------------------------------------------------------------------------
def forward(m):
    c = C1
    gi = {k: v.to(DEV) for k, v in fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"]).items()}
    was = m.training
    m.eval()
    with torch.no_grad():
        out = m(gi["x"], gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"])
    m.train(was)
    return out


def model_from_ema(tr, tmp_path):
    """A fresh model with the averaged weights, through the checkpoint's 'encoder_ema'."""
    f = str(tmp_path / "ema.tar")
    tr.save(f, 0, 5)
    ck = torch.load(f)
    fresh = build()
    res = fresh.load_state_dict(ck["encoder_ema"], strict=False)
    assert list(res.unexpected_keys) == []
    assert all(k.startswith("clip.") for k in res.missing_keys)          # only the frozen tower is not duplicated
    fresh.params_changed()
    return fresh, ck


def test_scope_exchanges_in_place_and_restores_bit_for_bit(trained, tmp_path):
    on = trained["on"]
    m = on.encoder
    fresh, ck = model_from_ema(on, tmp_path)
    assert set(ck) == {"opt_encoder", "ep", "total_it", "encoder", "encoder_ema", "ema"}
    assert ck["ema"] == dict(decay=DECAY, warmup=True, origin=0, num_updates=5)
    before, ema_before = flat_of(on).clone(), on.ema_state()["flat"].clone()
    ptr = flat_of(on).data_ptr()
    out_before = forward(m)
    with on.ema_weights() as same:
        assert same is on and flat_of(on).data_ptr() == ptr
        assert same_bits(flat_of(on), ema_before) and same_bits(on.ema_state()["flat"], before)
        inside = forward(m)
        assert same_bits(inside, forward(fresh)) and not same_bits(inside, out_before)
        x0, t, ln, xp, xo, nz = step_inputs(9)
        for call in (lambda: on.train_step_fused(x0, t, ln, xp, xo, noise=nz), lambda: on.train_step_captured(x0, t, ln, xp, xo, noise=nz),
                     on.update, lambda: on.save(str(tmp_path / "no.tar"), 0, 0)):
            with pytest.raises(RuntimeError, match="ema_weights"):
                call()
        with pytest.raises(RuntimeError, match="nest"):
            with on.ema_weights():
                pass
        assert same_bits(flat_of(on), ema_before)          # the refused calls and the refused entry changed nothing
    assert same_bits(flat_of(on), before) and same_bits(on.ema_state()["flat"], ema_before)
    assert same_bits(forward(m), out_before)               # no stale text context or shadow
    with pytest.raises(ZeroDivisionError):                 # an exception inside still restores
        with on.ema_weights():
            1 / 0
    assert same_bits(flat_of(on), before) and not on._ema_scope


CAPS = ["a person waves", "two people hug"]


def sample(tr, **kw):
    tr.set_sampler(steps=3, method="ddim", **kw)
    torch.manual_seed(3)
    return torch.stack(tr.generate(CAPS, torch.tensor([C1["T"], 41]), C1["F"]))


def test_sampling_from_the_ema(trained, tmp_path):
    on, off = trained["on"], trained["off"]
    fresh, _ = model_from_ema(on, tmp_path)
    before = flat_of(on).clone()
    want = sample(trainer(fresh))
    got = sample(on, weights="ema")
    assert same_bits(got, want) and torch.isfinite(got).all()
    assert same_bits(flat_of(on), before)
    today = sample(off)                                     # no EMA anywhere: the parent's path
    assert same_bits(sample(on, weights="model"), today) and same_bits(sample(on), today)
    assert not same_bits(got, today)
    off.set_sampler(steps=3, method="ddim", weights="ema")
    with pytest.raises(RuntimeError, match="ema_decay"):
        off.generate(CAPS, torch.tensor([C1["T"], 41]), C1["F"])
    off.set_sampler()
    on.set_sampler()
    with pytest.raises(ValueError, match="weights"):
        on.set_sampler(weights="average")


# ----------------------------------------------------------------------------------------------------------------------
# checkpoints
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("captured", (False, True))
def test_resume_continues_the_ema_and_its_warm_up(tmp_path, captured):
    f = str(tmp_path / "latest.tar")
    t1 = trainer(build().train(), fused_step=True, **EMA_OPT)
    run_steps(t1, range(3), captured)
    t1.save(f, 0, 3)
    run_steps(t1, range(3, 5), captured)
    t2 = trainer(build().train(), fused_step=True, **EMA_OPT)
    assert t2.load(f) == (0, 3)
    s2 = t2.ema_state()
    assert (s2["origin"], s2["num_updates"]) == (0, 3) and t2.fused_state()["step"].item() == 3
    run_steps(t2, range(3, 5), captured)
    s1 = t1.ema_state()
    assert same_bits(flat_of(t1), flat_of(t2)) and same_bits(s1["flat"], s2["flat"])
    assert s1["num_updates"] == s2["num_updates"] == 5
    # the warm-up went on at n = 4, 5: one more blend from the saved EMA with those weights, not with n = 1, 2
    ck = torch.load(f)
    name, p = next((k, q) for k, q in t1.encoder.named_parameters() if k.endswith("out.weight"))
    saved = ck["encoder_ema"][name].to(DEV)
    fp = t1.encoder.flat_params()
    o = next(o for q, o in zip(fp.params, fp.offsets) if q is p)
    snaps = []
    t3 = trainer(build().train(), fused_step=True, **EMA_OPT)
    t3.load(f)
    for i in (3, 4):
        run_steps(t3, [i])
        snaps.append(t3.encoder.flat_params().flat[o:o + p.numel()].clone())
    ref, bound = eb.ema_recurrence(saved.reshape(-1), snaps, 3, 0, DECAY, 1)
    held("resume.ema", s1["flat"][o:o + p.numel()], ref, bound)
    wrong, _ = eb.ema_recurrence(saved.reshape(-1), snaps, 0, 0, DECAY, 1)
    assert eb.ratio(wrong, ref, bound) > 1.0


def test_checkpoint_keys_and_an_ema_less_checkpoint(tmp_path):
    f = str(tmp_path / "plain.tar")
    t0 = trainer(build().train(), fused_step=True)
    run_steps(t0, range(2))
    t0.save(f, 0, 2)
    assert set(torch.load(f)) == {"opt_encoder", "ep", "total_it", "encoder"}
    t1 = trainer(build().train(), fused_step=True, **EMA_OPT)
    t1.load(f)
    st = t1.ema_state()
    assert same_bits(st["flat"], flat_of(t1)) and same_bits(flat_of(t1), flat_of(t0))
    assert (st["origin"], st["num_updates"]) == (2, 0)
    before = st["flat"].clone()
    run_steps(t1, [2])
    ref, bound = eb.ema_step_bound(before, flat_of(t1), 2, 2, DECAY, 1)         # its first update: n = 1
    held("ema-less checkpoint.first update", st["flat"], ref, bound)
    assert st["num_updates"] == 1


def test_inference_trainer_loads_and_samples_from_the_ema(trained, tmp_path):
    on = trained["on"]
    f = str(tmp_path / "ema.tar")
    on.save(f, 0, 5)
    args = types.SimpleNamespace(device=torch.device(DEV), diffusion_steps=1000, is_train=False)
    inf = hig_amd.DDPMTrainer(args, build().eval())
    inf.load(f)
    st = inf.ema_state()
    assert same_bits(st["flat"], on.ema_state()["flat"]) and same_bits(flat_of(inf), flat_of(on))
    assert (st["decay"], st["warmup"], st["origin"], st["num_updates"]) == (DECAY, True, 0, 5)
    assert same_bits(sample(inf, weights="ema"), sample(on, weights="ema"))
    on.set_sampler()


# ----------------------------------------------------------------------------------------------------------------------
# two-person trainer
# ----------------------------------------------------------------------------------------------------------------------
def test_two_person_fused_pit_step_and_generate():
    from test_gpu_interaction import build as build_pair, _trainer as pair_trainer, CAP1, CAP2
    c = fill.ICASES["tiny2"]
    B, T, Fd = c["B"], c["T"], c["F"]
    x0 = (fill.tensor_for("ema2.x0", (2 * B, T, Fd)) * 10).to(DEV)
    noise = (fill.tensor_for("ema2.noise", x0.shape) * 10).to(DEV)
    tt, length = torch.tensor(c["t"], device=DEV), torch.tensor(c["lengths"], device=DEV)
    xf_proj = (fill.tensor_for("ema2.xp", (4 * B, 4 * c["d"])) * 10).to(DEV)
    xf_out = (fill.tensor_for("ema2.xo", (4 * B, c["N"], c["Lt"])) * 10).to(DEV)
    off, on = pair_trainer(c, build_pair(c).train()), pair_trainer(c, build_pair(c).train())
    on.opt.ema_decay, on.opt.ema_warmup = DECAY, False
    e0 = flat_of(on).clone()
    for tr in (off, on):
        tr.train_step_fused(x0, tt, length, xf_proj, xf_out, noise=noise)
    assert same_bits(flat_of(off), flat_of(on)) and not same_bits(flat_of(on), e0)
    ref, bound = eb.ema_step_bound(e0, flat_of(on), 0, 0, DECAY, 0)
    held("DDPMMulTrainer.train_step_fused.ema", on.ema_state()["flat"], ref, bound)
    assert not same_bits(on.ema_state()["flat"], e0)
    on.set_sampler(steps=3, method="ddim", weights="ema")
    before = flat_of(on).clone()
    outs = on.generate(CAP1, CAP2, torch.tensor([T, 9]), Fd)
    assert len(outs) == B and all(o[0].shape == (T, Fd) and torch.isfinite(o[0]).all() and torch.isfinite(o[1]).all() for o in outs)
    assert same_bits(flat_of(on), before)


# ----------------------------------------------------------------------------------------------------------------------
# re-homed parameters; trainable tensors outside the flat buffer
# ----------------------------------------------------------------------------------------------------------------------
def test_ema_moves_along_when_the_model_is_rehomed():
    """`.to()` / `.float()` drop the flat parameter buffer: the EMA stays tied to the live one, the captured step re-captures."""
    t1, t2 = trainer(build().train(), **EMA_OPT), trainer(build().train(), **EMA_OPT)
    run_steps(t1, [0], captured=True)
    run_steps(t2, [0])
    old = flat_of(t1).data_ptr()
    t1.to(torch.device(DEV))
    t1.encoder.float()
    run_steps(t1, [1, 2], captured=True)
    run_steps(t2, [1, 2])
    assert flat_of(t1).data_ptr() != old and t1.ema_state()["ptr"] == flat_of(t1).data_ptr()
    assert same_bits(flat_of(t1), flat_of(t2)) and same_bits(t1.ema_state()["flat"], t2.ema_state()["flat"])
    assert t1.ema_state()["num_updates"] == 3


def test_trainable_tensors_outside_the_flat_buffer_have_twins():
    """cap_id model: the class embeddings (and its torch text projection) train outside the flat buffer.  update() blends them
    with hig_ema_update, the scope exchanges them with hig_swap_f32, the checkpoint names them."""
    from test_gpu_interaction import build as build_pair, case_inputs
    c = fill.ICASES["tiny2"]
    m = build_pair(c, cap_id=True).train()
    args = types.SimpleNamespace(device=torch.device(DEV), diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=c["B"],
                                 multi=True, label_path="labels/", cap_id=True, ema_decay=DECAY, ema_warmup=False)
    tr = hig_amd.DDPMMulTrainer(args, m)
    tr.opt_encoder = torch.optim.Adam(m.parameters(), lr=2e-4)
    _, gi = case_inputs(c)
    ids = [torch.tensor([3, 41], device=DEV), torch.tensor([4, 40], device=DEV)]
    tr.fake_noise = m(gi["x"], gi["t"], length=gi["length"], text=ids)
    tr.real_noise = (fill.tensor_for("ema.capid.target", tr.fake_noise.shape) * 10.0).to(DEV)
    tr.src_mask = m.generate_src_mask(c["T"], gi["length"]).to(DEV)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    e0 = flat_of(tr).clone()
    tr.update()
    st = tr.ema_state()
    assert "cap_embedding" in st["outside"] and st["num_updates"] == 1
    now = dict(m.named_parameters())
    for k, e in st["outside"].items():
        assert not same_bits(now[k], before[k]), k                                   # it trained
        ref, bound = eb.ema_step_bound(before[k].reshape(-1), now[k].detach().reshape(-1), 0, 0, DECAY, 0)
        held("update.outside." + k, e.reshape(-1), ref, bound)
    ref, bound = eb.ema_step_bound(e0, flat_of(tr), 0, 0, DECAY, 0)
    held("update.flat (cap_id)", st["flat"], ref, bound)
    after = {k: p.detach().clone() for k, p in m.named_parameters()}
    twins = {k: e.clone() for k, e in st["outside"].items()}
    with tr.ema_weights():
        for k in twins:
            assert same_bits(now[k], twins[k]) and same_bits(st["outside"][k], after[k])
    for k, p in m.named_parameters():
        assert same_bits(p, after[k]), k
    sd = tr._ema_state_dict(st)
    assert set(st["outside"]) <= set(sd) and set(sd) == {k for k, p in m.named_parameters() if p.requires_grad}
