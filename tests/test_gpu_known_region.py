"""Known-region conditioning on the MI355X: the contract of hig_impose_known (every masked element within the bound of
hig_q_sample and, on the full mask, bit-equal to it; every other element's bits kept; nothing around x touched, the inputs
unmodified, every refusal silent), the fused class path and an eager loop against what the reference computes with `pre_seq`
(golden G17), captured loops against eager ones, the no-op and the noise of the conditioned loops, and the trainers.

Measured on an MI355X (`pytest -s` prints the RATIO / GATE / LOOP lines this was collected from):
    hig_impose_known, largest |error| / q_sample_bound on the mask     0.982  1 x 2200003, full and Bernoulli masks
      (3 x 180001: 0.959; 3 x 4099: 0.930, the same through the scalar path; hig_q_sample itself: 0.982 over 3 x 180001 --
      three roundings under a bound that counts exactly those); bit-equal to hig_q_sample on every full mask
    fused p_sample with pre_seq against G17, rel-L2 / gate             x after the imposition 0.000 (bit for bit the
      reference's), sample 0.063, pred_xstart 0.037 (largest of the four samples)
    fused ddim_sample with known against impose-then-step              0.000 at eta 0 and eta 1
    eager 10-step pre_seq loop against G17's loop                      rel 4.7e-07 (gate 2e-4)
    conditioned captured loop against the eager one                    rel 0 for all three samplers, fp32 and bf16 storage
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hig_amd  # noqa: E402
import known_bounds as kb  # noqa: E402
from hig_amd import _lib  # noqa: E402
from hig_amd.models import gaussian_diffusion as gdm  # noqa: E402
from oracle import fill  # noqa: E402
from test_gpu_bf16_storage import CASES16  # noqa: E402
from test_gpu_bf16_storage import build as build16  # noqa: E402
from test_gpu_denoiser import _NoiseFeed, build, rel  # noqa: E402
from test_gpu_few_step import CAPS, K, loop_setup, patch_randn, spaced  # noqa: E402
from test_gpu_interaction import CAP1, CAP2  # noqa: E402
from test_gpu_interaction import _trainer as _mul_trainer  # noqa: E402
from test_gpu_interaction import build as build_pair  # noqa: E402
from test_gpu_rowops_contract import DEV, Buf, P, S, lib, ok, refused  # noqa: E402

EINVAL = -1
NAN = float("nan")


def bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------------------------
# 1. hig_impose_known
# ----------------------------------------------------------------------------------------------------------------------
def impose_call(xp, kp, mp, zp, tp, tabp, nsteps, B, per):
    return lib().hig_impose_known(xp, kp, mp, zp, tp, tabp, nsteps, B, per, S())


def run_impose_case(tag, B, per, kinds, shift=0):
    """shift = 1: x, known and z start one element, mask one byte, past their aligned bases (the scalar path)."""
    n = B * per
    worst = 0.0
    for kind in kinds:
        x, known, z, mask, t, tab = kb.impose_case(B, per, kind, seed=per)
        pad = lambda v: torch.cat([torch.zeros(shift, dtype=v.dtype), v.flatten()]).to(DEV)  # noqa: E731
        kd, zd, md, td, tabd = pad(known), pad(z), pad(mask), t.to(DEV), tab.to(DEV)
        kd0, zd0, md0 = kd.clone(), zd.clone(), md.clone()
        what = "%s %s" % (tag, kind)
        outs = []
        for _ in range(2):                                  # the second call, from the same x: the same bits
            xb = Buf.flat(n + shift)
            xb.out.zero_()
            xb.out[0, shift:].copy_(x.flatten().to(DEV))
            ok(impose_call(xb.p(shift), P(kd, shift), P(md, shift), P(zd, shift), P(td), P(tabd), kb.NSTEPS, B, per))
            xb.guards("hig_impose_known " + what)
            assert shift == 0 or xb.out[0, 0].item() == 0
            outs.append(xb.out.cpu()[0, shift:].clone())
        assert torch.equal(bits(outs[0]), bits(outs[1])), what + ": a second call gives other bits"
        for name, now, was in (("known", kd, kd0), ("z", zd, zd0)):
            assert torch.equal(bits(now), bits(was)), "%s: %s was modified" % (what, name)
        assert torch.equal(md, md0), what + ": mask was modified"
        r, same = kb.check(outs[0], x, known, z, mask, t, tab)
        print("RATIO hig_impose_known %s %.3f" % (what, r))
        assert r <= 1.0, "%s: largest |err| / bound = %.3f on the mask" % (what, r)
        assert same, what + ": an element off the mask changed its bits"
        worst = max(worst, r)
        if kind == "one":                                   # bit for bit what hig_q_sample computes for the same operands
            q = Buf.flat(n)
            ok(lib().hig_q_sample(P(kd, shift), P(zd, shift), P(td), P(tabd), kb.NSTEPS, B, per, q.p(), S()))
            assert torch.equal(bits(q.written("hig_q_sample")[0]), bits(outs[0])), what + ": differs from hig_q_sample"
    return worst


@pytest.mark.parametrize("per", kb.PER_SAMPLE)
def test_impose_known_contract(per):
    """B = 3 at t = (0, 1, nsteps // 2): per_sample 1 / 5 / 4099 -- one element; a float4 and a tail; samples that straddle
    float4 groups -- under every mask."""
    run_impose_case("B3_per%d" % per, kb.B_SMALL, per, kb.MASKS)


def test_impose_known_unaligned_pointers_take_the_scalar_path():
    run_impose_case("B3_per4099_shifted", kb.B_SMALL, 4099, kb.MASKS, shift=1)


def test_impose_known_large_extents():
    """3 x 180001: sample boundaries inside a workgroup and a scalar rest; 1 x 2200003: a second trip of the grid-stride
    loop of 2048 x 256 threads."""
    run_impose_case("3x180001", *kb.WRAP_SHAPE, ("bernoulli", "run_across_boundary", "one"))
    run_impose_case("1x2200003", *kb.BIG_SHAPE, ("bernoulli", "last_only", "one"))


def test_impose_known_refusals():
    B, per = 3, 5
    x, known, z, mask, t, tab = kb.impose_case(B, per, "alternating", seed=5)
    kd, zd, md, td, tabd = (v.contiguous().to(DEV) for v in (known, z, mask, t, tab))
    xb = Buf.flat(B * per)
    good = dict(x=xb.p(), known=P(kd), mask=P(md), z=P(zd), t=P(td), tab=P(tabd), nsteps=kb.NSTEPS, B=B, per=per)
    bad = [(k + " NULL", {k: None}) for k in ("x", "known", "mask", "z", "t", "tab")]
    bad += [("%s = %d" % (k, v), {k: v}) for k in ("nsteps", "B", "per") for v in (0, -3)]
    for what, change in bad:
        a = dict(good, **change)
        rc = impose_call(a["x"], a["known"], a["mask"], a["z"], a["t"], a["tab"], a["nsteps"], a["B"], a["per"])
        assert rc == EINVAL, "%s: returned %d" % (what, rc)
        refused(rc, (xb,), "hig_impose_known, " + what)
    # a step outside the table reads its nearest row
    tb = torch.tensor([-4, kb.NSTEPS + 7, 1], dtype=torch.int64)
    xb.out.copy_(x.view(1, -1).to(DEV))
    ok(impose_call(xb.p(), P(kd), P(md), P(zd), P(tb.to(DEV)), P(tabd), kb.NSTEPS, B, per))
    r, same = kb.check(xb.out.cpu()[0], x, known, z, mask, tb.clamp(0, kb.NSTEPS - 1), tab)
    assert r <= 1.0 and same


# ----------------------------------------------------------------------------------------------------------------------
# 2. the fused class path against the reference
# ----------------------------------------------------------------------------------------------------------------------
class Spy:
    def __init__(self, real, launches):
        self.real, self.launches = real, launches

    def __getattr__(self, name):
        self.launches.append(name)
        return getattr(self.real(), name)


def spied(call):
    launches, real = [], _lib.lib
    _lib.lib = lambda: Spy(real, launches)
    try:
        return call(), launches
    finally:
        _lib.lib = real


def gate_of(floor):
    floor = torch.as_tensor(floor)
    return torch.maximum(torch.full_like(floor, 1e-6), 4 * floor).clamp_max(1e-3)


def rel_rows(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(1), torch.as_tensor(b).double().cpu().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1)


def test_fused_pre_seq_step_matches_reference_golden(gold):
    g = gold("g17_known_region.npz")
    sd = spaced()
    x, eps, pre, t = (torch.tensor(g["pre." + k]).to(DEV) for k in ("x", "eps", "pre_seq", "t"))
    x_in, Fp = x.clone(), pre.shape[2]
    feed = _NoiseFeed("g17.s", DEV)
    undo = patch_randn(randn=feed.randn, randn_like=feed.randn_like)
    try:
        r, launches = spied(lambda: sd.p_sample(lambda *_a, **_k: eps, x, t, clip_denoised=False, pre_seq=pre))
    finally:
        undo()
    assert launches == ["hig_impose_known", "hig_p_sample_step"], launches
    assert feed.i == int(g["pre.draws"])
    gate = gate_of(g["pre.floor"])
    for key, got in (("x_after", x), ("sample", r["sample"]), ("pred_xstart", r["pred_xstart"])):
        e = rel_rows(got, g["pre." + key])
        print("GATE pre.%s %s" % (key, " ".join("%.3f" % v for v in (e / gate).tolist())))
        assert (e <= gate).all(), (key, e.tolist(), gate.tolist())
    assert torch.equal(bits(x[:, :, Fp:]), bits(x_in[:, :, Fp:]))      # written in place, the free features untouched


def test_fused_ddim_step_with_known_is_impose_then_step(gold):
    g16 = gold("g16_few_step.npz")
    sd = spaced()
    x, eps, z, t = (torch.tensor(g16[k]).to(DEV) for k in ("x", "eps", "z", "t"))
    B, T, F = x.shape
    known = (fill.tensor_for("g17.ddim.known", (B, T, F)) * 10).to(DEV)
    mask = torch.zeros(B, T, F, dtype=torch.bool, device=DEV)
    mask[:, :T // 2, :4] = True
    known[~mask] = NAN
    stub = lambda *_a, **_k: eps  # noqa: E731
    undo = patch_randn(randn_like=lambda v, **_: z)
    try:
        for eta in (0.0, 1.0):
            xa = x.clone()
            ra, launches = spied(lambda: sd.ddim_sample(stub, xa, t, clip_denoised=False, eta=eta, known=known, known_mask=mask))
            assert launches == ["hig_impose_known", "hig_ddim_step"], launches
            # impose with tensor ops, then the unconditioned step
            xb = x.clone()
            xb.copy_(torch.where(mask, sd._q_sample_ops(known, t, z), xb))
            rb = sd.ddim_sample(stub, xb, t, clip_denoised=False, eta=eta)
            gate = gate_of(g16["ddim.eta%g.clip0.floor" % eta])
            for key in ("sample", "pred_xstart"):
                e = rel_rows(ra[key], rb[key])
                print("GATE ddim.eta%g.%s %s" % (eta, key, " ".join("%.3f" % v for v in (e / gate).tolist())))
                assert (e <= gate).all(), (eta, key, e.tolist(), gate.tolist())
            assert torch.isfinite(ra["sample"]).all()
    finally:
        undo()


# ----------------------------------------------------------------------------------------------------------------------
# 3. loops against the reference
# ----------------------------------------------------------------------------------------------------------------------
def test_eager_pre_seq_loop_matches_reference_golden(gold):
    g = gold("g17_known_region.npz")
    m, kw, shape, _ = loop_setup()
    x0 = (fill.tensor_for("g17.x0", shape) * 10.0).to(DEV)
    pre = torch.tensor(g["loop.pre_seq"]).to(DEV)
    sd = spaced()
    sd.use_hip_graph = False   # injected noise sequence: the eager loop, step for step
    feed = _NoiseFeed("g17.p", DEV)
    undo = patch_randn(randn=feed.randn, randn_like=feed.randn_like)
    try:
        final = sd.p_sample_loop(m, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, pre_seq=pre)
    finally:
        undo()
    assert feed.i == int(g["loop.draws"]) == 2 * K
    e = rel(final, g["loop.sample"])
    print("LOOP pre_seq rel %.3e" % e)
    assert e < 2e-4


# ----------------------------------------------------------------------------------------------------------------------
# 4. captured equals eager; nothing known is a no-op; noise is drawn
# ----------------------------------------------------------------------------------------------------------------------
def known_for(shape, Fp=4):
    """The first Fp features of the frames < T // 2: a mask that is neither empty nor full."""
    B, T, F = shape
    known = (fill.tensor_for("g17.known.%dx%dx%d" % shape, shape) * 10.0).to(DEV)
    mask = torch.zeros(shape, dtype=torch.bool, device=DEV)
    mask[:, :T // 2, :Fp] = True
    return known, mask


def run_loop(sd, m, shape, x0, kw, method, eta, **cond):
    if method == "ddim":
        return sd.ddim_sample_loop(m, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, eta=eta, **cond)
    return sd.p_sample_loop(m, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, **cond)


def counting_replays(call):
    replays, real = [], torch.cuda.CUDAGraph.replay
    torch.cuda.CUDAGraph.replay = lambda self: (replays.append(1), real(self))[1]
    try:
        return call(), len(replays)
    finally:
        torch.cuda.CUDAGraph.replay = real


SAMPLERS = (("ddpm", 0.0), ("ddim", 0.0), ("ddim", 1.0))


def setup16():
    c = CASES16["small"]
    m = build16(c, storage="bf16").eval()
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    kw = {k: inp[k].to(DEV) for k in ("xf_proj", "xf_out", "length")}
    shape = (c["B"], c["T"], c["F"])
    return m, kw, shape, (fill.tensor_for("g17.x0.bf16", shape) * 10.0).to(DEV)


@pytest.mark.parametrize("storage", ("f32", "bf16"))
@pytest.mark.parametrize("method,eta", SAMPLERS)
def test_conditioned_captured_loop_equals_eager_loop(method, eta, storage):
    m, kw, shape, x0 = loop_setup() if storage == "f32" else setup16()
    known, mask = known_for(shape)
    outs = []
    for use_graph in (False, True):
        sd = spaced()
        sd.use_hip_graph, sd._debug_zero_noise = use_graph, True
        undo = patch_randn(randn_like=lambda v, **_: torch.zeros_like(v)) if not use_graph else (lambda: None)
        try:
            out, n = counting_replays(lambda: run_loop(sd, m, shape, x0, kw, method, eta, known=known, known_mask=mask))
        finally:
            undo()
        assert n == (K if use_graph else 0)
        outs.append(out)
    eager, captured = outs
    assert torch.isfinite(captured).all()
    e = rel(captured, eager)
    print("LOOP captured vs eager %s eta%g %s rel %.3e" % (method, eta, storage, e))
    assert e < 1e-6


@pytest.mark.parametrize("method,eta", (("ddpm", 0.0), ("ddim", 0.0)))
def test_nothing_known_is_a_no_op(method, eta):
    m, kw, shape, x0 = loop_setup()
    known, _ = known_for(shape)
    none = torch.zeros(shape, dtype=torch.bool, device=DEV)
    sd = spaced()
    sd._debug_zero_noise = True
    (plain, launches) = spied(lambda: run_loop(sd, m, shape, x0, kw, method, eta))
    assert "hig_impose_known" not in launches and ("hig_ddim_step" if method == "ddim" else "hig_p_sample_step") in launches
    (cond, launches), n = counting_replays(lambda: spied(lambda: run_loop(sd, m, shape, x0, kw, method, eta, known=known,
                                                                          known_mask=none)))
    assert n == K and "hig_impose_known" in launches
    assert torch.equal(cond, plain)


def test_nothing_known_is_a_no_op_on_the_full_chain():
    m, kw, shape, x0 = loop_setup()
    known, _ = known_for(shape)
    none = torch.zeros(shape, dtype=torch.bool, device=DEV)
    gd = hig_amd.GaussianDiffusion(betas=gdm.get_named_beta_schedule("linear", 50), model_mean_type=gdm.ModelMeanType.EPSILON,
                                   model_var_type=gdm.ModelVarType.FIXED_SMALL, loss_type=gdm.LossType.MSE)
    gd._debug_zero_noise = True
    call = lambda **c: gd.p_sample_loop(m, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, **c)  # noqa: E731
    plain, launches = spied(call)
    assert "hig_impose_known" not in launches and "hig_p_sample_step" in launches
    (cond, launches), n = counting_replays(lambda: spied(lambda: call(known=known, known_mask=none)))
    assert n == 50 and "hig_impose_known" in launches
    assert torch.equal(cond, plain)
    # and with something known the captured full chain is the eager one
    known, mask = known_for(shape)
    captured = call(known=known, known_mask=mask)
    gd.use_hip_graph = False
    undo = patch_randn(randn_like=lambda v, **_: torch.zeros_like(v))
    try:
        eager = call(known=known, known_mask=mask)
    finally:
        undo()
    assert torch.isfinite(captured).all() and rel(captured, eager) < 1e-6
    assert rel(captured, plain) > 1e-3


def test_conditioned_ddim_loop_draws_noise_at_eta_0():
    m, kw, shape, x0 = loop_setup()
    known, mask = known_for(shape)
    sd = spaced()
    torch.manual_seed(1)
    a = run_loop(sd, m, shape, x0, kw, "ddim", 0.0, known=known, known_mask=mask)
    torch.manual_seed(2)
    b = run_loop(sd, m, shape, x0, kw, "ddim", 0.0, known=known, known_mask=mask)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert not torch.equal(a, b) and rel(a, b) > 1e-6        # the imposition's noise reaches the sample through the model


# ----------------------------------------------------------------------------------------------------------------------
# 5. trainers
# ----------------------------------------------------------------------------------------------------------------------
def _trainer_n(c, m, steps):
    import types
    args = types.SimpleNamespace(device=torch.device(DEV), diffusion_steps=steps, is_train=True, lr=2e-4, batch_size=c["B"],
                                 num_epochs=1, log_every=50, save_latest=500, save_every_e=5, is_continue=False,
                                 model_dir="/tmp")
    return hig_amd.DDPMTrainer(args, m)


def test_trainer_generates_with_a_known_region():
    c = fill.CASES["tiny"]
    m = build(c).eval()
    lens = torch.tensor([16, 12, 9])
    T, F = 16, c["F"]
    known, mask = known_for((3, c["num_frames"], F))          # longer than the chunk: cut to its T
    for steps, sampler in ((1000, dict(steps=10, method="ddim")), (50, None)):
        tr = _trainer_n(c, m, steps)
        if sampler:
            tr.set_sampler(**sampler)
        torch.manual_seed(5)
        got = tr.generate_batch(CAPS, lens, F, known=known, known_mask=mask)
        xf_proj, xf_out = m.encode_text(CAPS, tr.device)
        mk = dict(xf_proj=xf_proj, xf_out=xf_out, length=lens)
        torch.manual_seed(5)
        if sampler:
            want = spaced().ddim_sample_loop(m, (3, T, F), clip_denoised=False, eta=0.0, model_kwargs=mk,
                                             known=known[:, :T], known_mask=mask[:, :T])
        else:
            want = tr.diffusion.p_sample_loop(m, (3, T, F), clip_denoised=False, model_kwargs=mk, known=known[:, :T],
                                              known_mask=mask[:, :T])
        assert got.shape == (3, T, F) and torch.isfinite(got).all() and torch.equal(got, want)
    # generate slices the pair per chunk and cuts it to the chunk's T
    seen = []

    def spy(shape, model_kwargs, known=None, known_mask=None):
        seen.append((shape, known, known_mask))
        return torch.zeros(shape, device=DEV)

    tr._sample_loop = spy
    outs = tr.generate(CAPS, lens, F, batch_size=2, known=known, known_mask=mask[:1])      # (a mask that broadcasts over N)
    assert len(outs) == 3 and [s[0] for s in seen] == [(2, 16, F), (1, 9, F)]
    assert torch.equal(seen[0][1], known[0:2, :16]) and torch.equal(seen[1][1], known[2:3, :9])
    assert torch.equal(seen[0][2].bool(), mask[0:2, :16]) and torch.equal(seen[1][2].bool(), mask[:1, :9])
    seen.clear()
    tr.generate(CAPS, lens, F, batch_size=2)
    assert [(s[1], s[2]) for s in seen] == [(None, None)] * 2


def test_two_person_trainer_generates_a_reaction():
    c = fill.ICASES["tiny2"]
    m = build_pair(c).eval()
    tr = _mul_trainer(c, m)
    T, Fd, Np = c["T"], c["F"], 2
    lens = torch.tensor([T, 9])
    known = (fill.tensor_for("g17.pair.known", (2, Np, T, Fd)) * 10.0).to(DEV)
    mask = torch.zeros(2, Np, T, Fd, dtype=torch.bool, device=DEV)
    mask[0] = (torch.arange(T, device=DEV)[None, :] < lens.to(DEV)[:, None])[:, :, None]    # person 1 is given, person 2 generated
    known[1] = NAN
    tr.set_sampler(steps=10, method="ddim", eta=0.0)
    torch.manual_seed(6)
    outs = tr.generate(CAP1, CAP2, lens, Fd, known=known, known_mask=mask)
    assert len(outs) == Np and all(len(o) == 2 and o[0].shape == (T, Fd) and o[1].shape == (T, Fd) for o in outs)
    assert all(torch.isfinite(o[0]).all() and torch.isfinite(o[1]).all() for o in outs)
    xf_proj, xf_out = m.encode_text(list(CAP1) + list(CAP2), tr.device)
    torch.manual_seed(6)
    want = spaced().ddim_sample_loop(m, (2 * Np, T, Fd), clip_denoised=False, eta=0.0,
                                     model_kwargs=dict(xf_proj=xf_proj, xf_out=xf_out, length=torch.cat([lens, lens])),
                                     known=known.flatten(0, 1), known_mask=mask.flatten(0, 1))
    assert torch.equal(torch.stack([o[0] for o in outs] + [o[1] for o in outs]), want)
    # the model batch is [person 1 of every pair; person 2 of every pair]
    seen = []
    tr._sample_loop = lambda shape, kw, known=None, known_mask=None: (seen.append((shape, known, known_mask)),
                                                                      torch.zeros(shape, device=DEV))[1]
    tr.generate(CAP1, CAP2, lens, Fd, known=known, known_mask=mask)
    (shape, k, km), = seen
    assert shape == (2 * Np, T, Fd)
    assert torch.equal(bits(k), bits(torch.cat([known[0], known[1]]))) and torch.equal(km.bool(), torch.cat([mask[0], mask[1]]))
