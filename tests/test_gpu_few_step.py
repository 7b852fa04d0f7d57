"""Few-step sampling on the MI355X: the contract of hig_ddim_step and hig_advance_timesteps (every element within the bound of
tests/ddim_bounds.py, every output written, nothing around it touched, every refusal silent), SpacedDiffusion's fused steps
and loops against what the reference computes on the same strided schedule (golden G16), captured loops against eager ones,
and the trainers' set_sampler.

Measured on an MI355X (largest |error| / bound over all cases; `pytest -s` prints the RATIO lines this was collected from):
    output                       bound                    ratio  at
    hig_ddim_step.x_prev         ddim_bound               0.590  3 x 180001, eta 0.5, clip 1
    hig_ddim_step.pred_xstart    2 u (|a x| + |b eps|)    0.995  1 x 2200003, eta 1, clip 0
pred_xstart is three roundings under a bound that counts exactly those, over 2.2 million elements (hig_p_sample_step.pred_xstart:
0.944 over 540003); x_prev has a dozen roundings that do not all fall the same way.
Fused class path against G16, per-sample rel-L2 / max(1e-6, 4 floor) (`GATE` lines), largest over the four samples:
    ddim, eta 0 / 0.5 / 1 x clip 0 / 1, sample and pred_xstart    0.000  (all twelve rows: bit for bit the reference's output)
    p_sample.clip0 sample / pred_xstart                           0.059 / 0.059
"""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import ddim_bounds as db  # noqa: E402
import hig_amd  # noqa: E402
from hig_amd import _lib  # noqa: E402
from hig_amd.models import gaussian_diffusion as gdm  # noqa: E402
from hig_amd.models import spaced_diffusion as sdm  # noqa: E402
from oracle import fill  # noqa: E402
from test_gpu_bf16_storage import CASES16  # noqa: E402
from test_gpu_bf16_storage import build as build16  # noqa: E402
from test_gpu_denoiser import _NoiseFeed, _trainer, build, case_inputs, rel  # noqa: E402
from test_gpu_interaction import CAP1, CAP2  # noqa: E402
from test_gpu_interaction import _trainer as _mul_trainer  # noqa: E402
from test_gpu_interaction import build as build_pair  # noqa: E402
from test_gpu_rowops_contract import DEV, Buf, P, S, held, lib, ok, refused  # noqa: E402

N, K = 1000, 10
ETAS, CLIPS = (0.0, 0.5, 1.0), (False, True)
EINVAL = -1


def spaced(k=K, n=N):
    return hig_amd.SpacedDiffusion(hig_amd.space_timesteps(n, k), betas=gdm.get_named_beta_schedule("linear", n),
                                   model_mean_type=gdm.ModelMeanType.EPSILON, model_var_type=gdm.ModelVarType.FIXED_SMALL,
                                   loss_type=gdm.LossType.MSE)


def patch_randn(randn=None, randn_like=None):
    """Replaces th.randn / th.randn_like in both diffusion modules until the returned undo() runs."""
    proxy = types.SimpleNamespace(**{k: getattr(torch, k) for k in dir(torch) if not k.startswith("__")})
    if randn is not None:
        proxy.randn = randn
    if randn_like is not None:
        proxy.randn_like = randn_like
    old = gdm.th, sdm.th
    gdm.th = sdm.th = proxy

    def undo():
        gdm.th, sdm.th = old
    return undo


# ----------------------------------------------------------------------------------------------------------------------
# 6. hig_ddim_step
# ----------------------------------------------------------------------------------------------------------------------
def ddim_call(xp_, ep, zp, tp, tabp, nsteps, B, per, eta, clip, outp, predp):
    return lib().hig_ddim_step(xp_, ep, zp, tp, tabp, nsteps, B, per, eta, clip, outp, predp, S())


def run_ddim_case(tag, B, per, shifted=False, etas=ETAS, clips=(0, 1)):
    x, eps, z, t, tab = db.ddim_case(B, per, seed=per, shifted=shifted)
    nsteps = tab.shape[1]
    xd, ed, zd, td, tabd = (v.contiguous().to(DEV) for v in (x, eps, z, t, tab))
    for eta in etas:
        for clip in clips:
            zz, zp = (None, None) if eta == 0 else (z, P(zd))
            (xp, b), (x0, b0) = db.ddim_bound(x, eps, zz, t, tab, eta, clip)
            what = "%s eta%g clip%d" % (tag, eta, clip)
            o1, o0 = Buf.flat(B * per), Buf.flat(B * per)
            ok(ddim_call(P(xd), P(ed), zp, P(td), P(tabd), nsteps, B, per, eta, clip, o1.p(), o0.p()))
            held("hig_ddim_step.x_prev " + what, o1.written("x_prev").view(B, per), xp, b)
            held("hig_ddim_step.pred_xstart " + what, o0.written("pred_xstart").view(B, per), x0, b0)
            # pred_xstart NULL, out of place: the same x_prev
            o2 = Buf.flat(B * per)
            ok(ddim_call(P(xd), P(ed), zp, P(td), P(tabd), nsteps, B, per, eta, clip, o2.p(), None))
            assert torch.equal(o2.written("x_prev, pred NULL"), o1.out.cpu()), what + ": pred_xstart NULL changes x_prev"
            # in place (x_prev == x), with and without pred_xstart
            for with_pred in (True, False):
                inplace, pr = Buf.flat(B * per), Buf.flat(B * per)
                inplace.out.copy_(xd.view(1, -1))
                ok(ddim_call(inplace.p(), P(ed), zp, P(td), P(tabd), nsteps, B, per, eta, clip, inplace.p(),
                             pr.p() if with_pred else None))
                assert torch.equal(inplace.written("in place"), o1.out.cpu()), what + ": the in-place step differs"
                if with_pred:
                    assert torch.equal(pr.written("pred in place"), o0.out.cpu()), what + ": in-place pred_xstart differs"
                else:
                    pr.untouched("pred_xstart NULL")
    return xd, ed, zd, td, tabd, nsteps


@pytest.mark.parametrize("per", db.PER_SAMPLE)
def test_ddim_step_contract(per):
    """B = 4 at t = (0, 1, K // 2, K - 1), K = 10 of 1000; per_sample 1 / 5 / 4099: one element, a float4 and a rest, samples that
    start inside a float4 and a rest after many vectors.  eta 0 (z NULL) / 0.5 / 1 x clip 0 / 1, out of place and in place,
    pred_xstart given and NULL."""
    run_ddim_case("B4_per%d" % per, 4, per)


def test_ddim_step_masks_the_noise_at_t0_where_sigma_is_not_zero():
    """The table without its first column: row t = 0 has sigma > 0, so a kernel that drops the t != 0 mask shows
    (tests/ddim_bounds.py, `noise_at_t0`)."""
    run_ddim_case("shifted_B4_per5", 4, 5, shifted=True, etas=(0.5, 1.0))


def test_ddim_step_large_extents():
    """3 x 180001 (rowops_bounds.DDPM_SHAPE: sample boundaries inside a workgroup, a scalar rest) and 1 x 2200003 (550000
    float4 groups: a second trip of the grid-stride loop of 2048 x 256 threads)."""
    run_ddim_case("3x180001", *db.WRAP_SHAPE, etas=(0.5,), clips=(1,))
    run_ddim_case("1x2200003", *db.BIG_SHAPE, etas=(1.0,), clips=(0,))


def test_ddim_step_unaligned_pointers_take_the_scalar_path():
    """Operands that start 4 bytes past a 16-byte boundary: no float4 access is possible, the result is the same."""
    B, per = 4, 37
    x, eps, z, t, tab = db.ddim_case(B, per, seed=37)
    n = B * per
    pad = lambda v: torch.cat([torch.zeros(1), v.flatten()]).to(DEV)  # noqa: E731
    xd, ed, zd = pad(x), pad(eps), pad(z)
    td, tabd = t.to(DEV), tab.to(DEV)
    (xp, b), (x0, b0) = db.ddim_bound(x, eps, z, t, tab, 0.5, 1)
    o1, o0 = Buf.flat(n + 1), Buf.flat(n + 1)
    o1.out.zero_(), o0.out.zero_()
    ok(ddim_call(P(xd, 1), P(ed, 1), P(zd, 1), P(td), P(tabd), tab.shape[1], B, per, 0.5, 1, o1.p(1), o0.p(1)))
    held("hig_ddim_step.x_prev unaligned", o1.written("x_prev")[0, 1:].view(B, per), xp, b)
    held("hig_ddim_step.pred_xstart unaligned", o0.written("pred_xstart")[0, 1:].view(B, per), x0, b0)
    assert o1.out[0, 0].item() == 0 and o0.out[0, 0].item() == 0


def test_ddim_step_refusals():
    B, per = 4, 5
    x, eps, z, t, tab = db.ddim_case(B, per, seed=5)
    xd, ed, zd, td, tabd = (v.contiguous().to(DEV) for v in (x, eps, z, t, tab))
    o1, o0 = Buf.flat(B * per), Buf.flat(B * per)
    good = dict(x=P(xd), eps=P(ed), z=P(zd), t=P(td), tab=P(tabd), nsteps=K, B=B, per=per, eta=0.5, clip=1, out=o1.p(), pred=o0.p())
    bad = (("x NULL", dict(x=None)), ("eps NULL", dict(eps=None)), ("t NULL", dict(t=None)), ("tab NULL", dict(tab=None)),
           ("x_prev NULL", dict(out=None)), ("z NULL with eta > 0", dict(z=None)), ("eta < 0", dict(eta=-0.5)),
           ("eta NaN", dict(eta=float("nan"))), ("eta inf", dict(eta=float("inf"))), ("B = 0", dict(B=0)), ("B < 0", dict(B=-4)), ("per_sample = 0", dict(per=0)),
           ("per_sample < 0", dict(per=-5)), ("nsteps = 0", dict(nsteps=0)), ("nsteps < 0", dict(nsteps=-10)))
    for what, change in bad:
        a = dict(good, **change)
        rc = ddim_call(a["x"], a["eps"], a["z"], a["t"], a["tab"], a["nsteps"], a["B"], a["per"], a["eta"], a["clip"], a["out"],
                       a["pred"])
        assert rc == EINVAL, "%s: returned %d" % (what, rc)
        refused(rc, (o1, o0), "hig_ddim_step, " + what)
    # and the accepted forms next to them: z NULL at eta == 0, z given at eta == 0 (never read: it holds NaN)
    nan_z = torch.full_like(zd, float("nan"))
    ok(ddim_call(P(xd), P(ed), P(nan_z), P(td), P(tabd), K, B, per, 0.0, 1, o1.p(), o0.p()))
    a = o1.written("eta 0, z given").clone()
    ok(ddim_call(P(xd), P(ed), None, P(td), P(tabd), K, B, per, 0.0, 1, o1.p(), None))
    assert torch.equal(o1.written("eta 0, z NULL"), a)


# ----------------------------------------------------------------------------------------------------------------------
# 7. hig_advance_timesteps
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 63, 64, 65, 1000))
def test_advance_timesteps(B):
    tmap = torch.tensor(hig_amd.space_timesteps(N, K), dtype=torch.int64)
    t = (torch.arange(B, dtype=torch.int64) * 7) % K          # 0 first: -> -1, t_model = map[0]
    assert t[0] == 0
    tb, tm = Buf.flat(2 * B), Buf.flat(2 * B)                  # (B int64 values in a guarded run of 8 B bytes)
    tb.out.view(torch.int64).copy_(t.to(DEV).view(1, -1))
    mapd = tmap.to(DEV)
    ok(lib().hig_advance_timesteps(tb.p(), P(mapd), K, B, tm.p(), S()))
    tb.guards("hig_advance_timesteps.t")
    tm.guards("hig_advance_timesteps.t_model")
    assert torch.equal(tb.out.view(torch.int64).cpu()[0], t - 1)
    assert torch.equal(tm.out.view(torch.int64).cpu()[0], tmap[(t - 1).clamp_min(0)])
    # a second step from there: -1 -> -2 still reads map[0]
    ok(lib().hig_advance_timesteps(tb.p(), P(mapd), K, B, tm.p(), S()))
    assert torch.equal(tm.out.view(torch.int64).cpu()[0], tmap[(t - 2).clamp_min(0)])
    fresh_t, fresh_m = Buf.flat(2 * B), Buf.flat(2 * B)
    for what, args in (("t NULL", (None, P(mapd), K, B, fresh_m.p())), ("map NULL", (fresh_t.p(), None, K, B, fresh_m.p())),
                       ("t_model NULL", (fresh_t.p(), P(mapd), K, B, None)), ("B = 0", (fresh_t.p(), P(mapd), K, 0, fresh_m.p())),
                       ("nsteps = 0", (fresh_t.p(), P(mapd), 0, B, fresh_m.p()))):
        rc = lib().hig_advance_timesteps(*args, S())
        assert rc == EINVAL, what
        refused(rc, (fresh_t, fresh_m), "hig_advance_timesteps, " + what)


# ----------------------------------------------------------------------------------------------------------------------
# 8. the fused class path against the reference
# ----------------------------------------------------------------------------------------------------------------------
def test_fused_steps_match_reference_golden(gold):
    """SpacedDiffusion.ddim_sample (every eta and clip row) and p_sample on ROCm tensors against the reference's outputs: per
    sample rel-L2 <= max(1e-6, 4 x the reference's own distance from fp64), and never above 1e-3."""
    g = gold("g16_few_step.npz")
    sd = spaced()
    x, eps, z, t = (torch.tensor(g[k]).to(DEV) for k in ("x", "eps", "z", "t"))
    stub = lambda *_a, **_k: eps  # noqa: E731
    launches = []
    real = _lib.lib

    class Spy:
        def __getattr__(self, name):
            launches.append(name)
            return getattr(real(), name)

    undo = patch_randn(randn_like=lambda v, **_: z)
    _lib.lib = lambda: Spy()
    try:
        rows = {}
        for clip in CLIPS:
            for eta in ETAS:
                rows["ddim.eta%g.clip%d" % (eta, clip)] = sd.ddim_sample(stub, x, t, clip_denoised=clip, eta=eta)
        assert launches == ["hig_ddim_step"] * 6, launches          # the fused kernel really ran, for both clip values
        rows["p_sample.clip0"] = sd.p_sample(stub, x, t, clip_denoised=False)
        assert launches[6:] == ["hig_p_sample_step"], launches
    finally:
        _lib.lib = real
        undo()
    for tag, r in rows.items():
        floor = torch.tensor(g[tag + ".floor"])
        gate = torch.maximum(torch.full_like(floor, 1e-6), 4 * floor).clamp_max(1e-3)
        for key in ("sample", "pred_xstart"):
            a, b = r[key].double().cpu().flatten(1), torch.tensor(g["%s.%s" % (tag, key)]).double().flatten(1)
            e = (a - b).norm(dim=1) / b.norm(dim=1)
            print("GATE %s.%s %s" % (tag, key, " ".join("%.3f" % v for v in (e / gate).tolist())))
            assert (e <= gate).all(), (tag, key, e.tolist(), gate.tolist())


# ----------------------------------------------------------------------------------------------------------------------
# 9. loops against the reference
# ----------------------------------------------------------------------------------------------------------------------
def loop_setup():
    c = fill.CASES["tiny"]
    m = build(c).eval()
    _, gi = case_inputs(c)
    kw = {"xf_proj": gi["xf_proj"], "xf_out": gi["xf_out"], "length": gi["length"]}
    shape = (c["B"], c["T"], c["F"])
    x0 = (fill.tensor_for("g16.x0", shape) * 10.0).to(DEV)
    return m, kw, shape, x0


def test_captured_ddim_loop_matches_reference_golden(gold):
    g = gold("g16_few_step.npz")
    m, kw, shape, x0 = loop_setup()
    sd = spaced()
    replays = []
    real = torch.cuda.CUDAGraph.replay
    torch.cuda.CUDAGraph.replay = lambda self: (replays.append(1), real(self))[1]
    try:
        final = sd.ddim_sample_loop(m, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, eta=0.0)
    finally:
        torch.cuda.CUDAGraph.replay = real
    assert len(replays) == K                                          # the captured path, one replay per kept step
    assert rel(final, g["loop.ddim.eta0"]) < 2e-4


@pytest.mark.parametrize("tag,prefix", (("loop.ddim.eta1", "g16.z"), ("loop.ddpm", "g16.p")))
def test_eager_loops_with_injected_noise_match_reference_golden(gold, tag, prefix):
    g = gold("g16_few_step.npz")
    m, kw, shape, x0 = loop_setup()
    sd = spaced()
    sd.use_hip_graph = False   # injected noise sequence: the eager loop, step for step
    feed = _NoiseFeed(prefix, DEV)
    undo = patch_randn(randn=feed.randn, randn_like=feed.randn_like)
    try:
        if tag == "loop.ddpm":
            final = sd.p_sample_loop(m, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw)
        else:
            final = sd.ddim_sample_loop(m, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, eta=1.0)
    finally:
        undo()
    assert feed.i == K
    assert rel(final, g[tag]) < 2e-4


# ----------------------------------------------------------------------------------------------------------------------
# 10. captured equals eager
# ----------------------------------------------------------------------------------------------------------------------
def run_loop(sd, m, shape, x0, kw, method, eta):
    if method == "ddim":
        return sd.ddim_sample_loop(m, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, eta=eta)
    return sd.p_sample_loop(m, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw)


def captured_and_eager(m, shape, x0, kw, method, eta):
    outs = []
    for use_graph in (False, True):
        sd = spaced()
        sd.use_hip_graph, sd._debug_zero_noise = use_graph, True
        undo = patch_randn(randn_like=lambda v, **_: torch.zeros_like(v)) if not use_graph else (lambda: None)
        try:
            outs.append(run_loop(sd, m, shape, x0, kw, method, eta))
        finally:
            undo()
    return outs


@pytest.mark.parametrize("method,eta", (("ddim", 0.0), ("ddim", 1.0), ("ddpm", 0.0)))
def test_captured_loop_equals_eager_loop(method, eta):
    m, kw, shape, x0 = loop_setup()
    eager, captured = captured_and_eager(m, shape, x0, kw, method, eta)
    assert torch.isfinite(captured).all()
    assert rel(captured, eager) < 1e-6


def test_captured_loops_draw_noise_exactly_when_they_should():
    m, kw, shape, x0 = loop_setup()
    sd = spaced()
    sd._debug_zero_noise = True
    quiet = run_loop(sd, m, shape, x0, kw, "ddim", 1.0)
    sd._debug_zero_noise = False
    noisy = run_loop(sd, m, shape, x0, kw, "ddim", 1.0)
    assert torch.isfinite(noisy).all() and rel(noisy, quiet) > 1e-3          # eta = 1 draws fresh noise every replay
    # eta = 0 draws nothing: the same start gives the same bits, whatever the generator's state
    torch.manual_seed(1)
    a = run_loop(sd, m, shape, x0, kw, "ddim", 0.0)
    torch.manual_seed(2)
    b = run_loop(sd, m, shape, x0, kw, "ddim", 0.0)
    assert torch.equal(a, b)


def test_captured_ddim_loop_equals_eager_loop_with_bf16_storage():
    c = CASES16["small"]
    m = build16(c, storage="bf16").eval()
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    kw = {k: inp[k].to(DEV) for k in ("xf_proj", "xf_out", "length")}
    shape = (c["B"], c["T"], c["F"])
    x0 = (fill.tensor_for("g16.x0.bf16", shape) * 10.0).to(DEV)
    eager, captured = captured_and_eager(m, shape, x0, kw, "ddim", 0.0)
    assert torch.isfinite(captured).all()
    assert rel(captured, eager) < 1e-6


# ----------------------------------------------------------------------------------------------------------------------
# 11. trainers
# ----------------------------------------------------------------------------------------------------------------------
CAPS = ["a person waves", "two people hug", "a person jumps"]


def test_trainer_set_sampler_generates_with_ddim():
    c = fill.CASES["tiny"]
    m = build(c).eval()
    tr = _trainer(c, m)
    tr.set_sampler(steps=10, method="ddim")
    lens = torch.tensor([16, 12, 9])
    outs = tr.generate(CAPS, lens, c["F"], batch_size=2)
    assert len(outs) == 3 and [tuple(o.shape) for o in outs] == [(16, c["F"]), (16, c["F"]), (9, c["F"])]
    assert all(torch.isfinite(o).all() for o in outs)
    # generate_batch is ddim_sample_loop with the trainer's arguments: the same seed gives the same sample
    for eta in (0.0, 1.0):
        tr.set_sampler(steps=10, method="ddim", eta=eta)
        torch.manual_seed(3)
        got = tr.generate_batch(CAPS, lens, c["F"])
        xf_proj, xf_out = m.encode_text(CAPS, tr.device)
        torch.manual_seed(3)
        want = spaced().ddim_sample_loop(m, (3, 16, c["F"]), clip_denoised=False, eta=eta,
                                         model_kwargs=dict(xf_proj=xf_proj, xf_out=xf_out, length=lens))
        assert torch.equal(got, want)
    tr.set_sampler(steps=10, method="ddpm")
    torch.manual_seed(4)
    got = tr.generate_batch(CAPS, lens, c["F"])
    xf_proj, xf_out = m.encode_text(CAPS, tr.device)
    torch.manual_seed(4)
    want = spaced().p_sample_loop(m, (3, 16, c["F"]), clip_denoised=False,
                                  model_kwargs=dict(xf_proj=xf_proj, xf_out=xf_out, length=lens))
    assert torch.equal(got, want)


def test_trainer_without_a_sampler_uses_the_full_chain():
    c = fill.CASES["tiny"]
    m = build(c).eval()
    lens = torch.tensor([16, 12, 9])
    for reset in (False, True):
        tr = _trainer(c, m)
        if reset:
            tr.set_sampler(steps=10, method="ddim")
            tr.set_sampler(None)
        seen = []

        def spy(model, shape, **kw):
            seen.append((shape, kw))
            return torch.zeros(shape, device=DEV)

        tr.diffusion.p_sample_loop = spy
        out = tr.generate_batch(CAPS, lens, c["F"])
        assert len(seen) == 1 and seen[0][0] == (3, 16, c["F"]) and out.shape == (3, 16, c["F"])
        assert seen[0][1]["clip_denoised"] is False and set(seen[0][1]["model_kwargs"]) == {"xf_proj", "xf_out", "length"}
    for bad in (dict(steps=10, method="plms"), dict(steps=1), dict(steps=1001), dict(steps=2.5), dict(steps=10, eta=-1.0)):
        with pytest.raises(ValueError):
            tr.set_sampler(**bad)


def test_two_person_trainer_set_sampler():
    c = fill.ICASES["tiny2"]
    m = build_pair(c).eval()
    tr = _mul_trainer(c, m)
    T, Fd = c["T"], c["F"]
    for method, eta in (("ddim", 0.0), ("ddpm", 0.0)):
        tr.set_sampler(steps=10, method=method, eta=eta)
        outs = tr.generate(CAP1, CAP2, torch.tensor([T, 9]), Fd)
        assert len(outs) == 2 and all(len(o) == 2 and o[0].shape == (T, Fd) and o[1].shape == (T, Fd) for o in outs)
        assert all(torch.isfinite(o[0]).all() and torch.isfinite(o[1]).all() for o in outs)
    tr.set_sampler(None)
    seen = []
    tr.diffusion.p_sample_loop = lambda model, shape, **kw: (seen.append(shape), torch.zeros(shape, device=DEV))[1]
    tr.generate_batch(CAP1, CAP2, torch.tensor([T, 9]), Fd)
    assert seen == [(4, T, Fd)]
