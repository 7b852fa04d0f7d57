"""The second-order few-step sampler on the MI355X: the contract of hig_dpm2m_step / hig_dpm2m_step_cfg (every element of the new
state and of the history within the bound of tests/dpm_bounds.py, both written in place, nothing around them touched, NaN history
never read where c_1 = 0, the scalar path bit-equal to the float4 path, every refusal silent), the guided twin against the
unguided kernel, SpacedDiffusion's fused step and its captured loop against the eager one, the order-1 loop against the
reference's DDIM golden (G16), and the trainers' set_sampler(method="dpmpp2m").

Measured on an MI355X (largest |error| / bound over all cases; `pytest -s` prints the RATIO / LOOP lines this was collected from):
    output                        bound                                                     ratio  at
    hig_dpm2m_step.x              dpm_bound                                                 0.814  3 x 180001, clip 1
    hig_dpm2m_step.hist           2 u (|a x| + |b eps|)                                     0.989  1 x 2200003, clip 0
    hig_dpm2m_step_cfg.x          cfg_bound                                                 0.827  2 x 1100002, group 1
    hig_dpm2m_step_cfg.hist       2 u (|a x| + |b eps_g|) + b e_g                           0.958  4 x 135001, group 2
hist is three roundings under a bound that counts exactly those, over 2.2 million elements (hig_ddim_step.pred_xstart: 0.995).
The fused step is bit for bit the tensor-op step on host tensors; eps_u == eps_c: the guided kernel is bit for bit the unguided
one.  Captured vs eager: rel 0 in all four cases.  Captured order=1 loop vs golden g16 loop.ddim.eta0: 6.6e-07 (gate 2e-4); vs
ddim_sample_loop at eta = 0 on the log-SNR steps: 9.5e-07."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import cfg_bounds as cb  # noqa: E402
import dpm_bounds as mb  # noqa: E402
import hig_amd  # noqa: E402
from hig_amd.models import gaussian_diffusion as gdm  # noqa: E402
from hig_amd.models.guidance import split_rows  # noqa: E402
from oracle import fill  # noqa: E402
from test_gpu_cfg import LONG, LONG1, LONG2, guided_setup  # noqa: E402
from test_gpu_denoiser import _trainer, build, rel  # noqa: E402
from test_gpu_few_step import loop_setup, patch_randn, spaced  # noqa: E402
from test_gpu_interaction import _trainer as _mul_trainer  # noqa: E402
from test_gpu_interaction import build as build_pair  # noqa: E402
from test_gpu_known_region import counting_replays, known_for, setup16, spied  # noqa: E402
from test_gpu_rowops_contract import DEV, Buf, P, S, held, lib, ok, refused  # noqa: E402

N, K = 1000, 10
EINVAL = -1
SAMPLER_KERNELS = ("hig_impose_known", "hig_p_sample_step", "hig_ddim_step", "hig_dpm2m_step", "hig_dec_timesteps",
                   "hig_advance_timesteps", "hig_cfg_combine")


def bits(t):
    return t.contiguous().view(torch.int32)


def logsnr_spaced(k=K):
    betas = gdm.get_named_beta_schedule("linear", N)
    return hig_amd.SpacedDiffusion(hig_amd.space_timesteps_logsnr(betas, k), betas=betas, model_mean_type=gdm.ModelMeanType.EPSILON,
                                   model_var_type=gdm.ModelVarType.FIXED_SMALL, loss_type=gdm.LossType.MSE)


# ----------------------------------------------------------------------------------------------------------------------
# 1. hig_dpm2m_step
# ----------------------------------------------------------------------------------------------------------------------
def run_step(case, clip, shift=0):
    """One in-place launch on guarded buffers, every operand `shift` elements past a 16-byte boundary: (x_prev, hist_out)."""
    x, eps, hist, t, tab = case
    B, per = x.shape
    n = B * per
    ed = torch.cat([torch.zeros(shift), eps.flatten()]).to(DEV)
    td, tabd = t.to(DEV), tab.to(DEV)
    xb, hb = Buf.flat(n + shift), Buf.flat(n + shift)
    xb.out.zero_(), hb.out.zero_()
    xb.out[0, shift:].copy_(x.flatten().to(DEV))
    hb.out[0, shift:].copy_(hist.flatten().to(DEV))
    ok(lib().hig_dpm2m_step(xb.p(shift), P(ed, shift), hb.p(shift), P(td), P(tabd), tab.shape[1], B, per, clip, S()))
    xo, ho = xb.written("hig_dpm2m_step x"), hb.written("hig_dpm2m_step hist")      # (no NaN left: the NaN history is gone)
    assert shift == 0 or (xo[0, 0].item() == 0 and ho[0, 0].item() == 0)
    assert torch.equal(bits(ed.cpu()[shift:]), bits(eps.flatten())), "hig_dpm2m_step modified eps"
    return xo[0, shift:].view(B, per), ho[0, shift:].view(B, per)


def check_case(tag, B, per, clips=mb.CLIPS, shift=0):
    case = mb.dpm_case(B, per, seed=per)
    x, eps, hist, t, tab = case
    assert torch.isnan(hist[tab[mb.M_C1][t] == 0]).all() and torch.isfinite(hist[tab[mb.M_C1][t] != 0]).all()
    outs = []
    for clip in clips:
        (xp, b), (x0, b0) = mb.dpm_bound(x, eps, hist, t, tab, clip)
        xo, ho = run_step(case, clip, shift)
        what = "%s clip%d shift%d" % (tag, clip, shift)
        held("hig_dpm2m_step.x_prev " + what, xo, xp, b)
        held("hig_dpm2m_step.hist " + what, ho, x0, b0)
        outs.append((xo, ho))
    return outs


@pytest.mark.parametrize("per", mb.PER_SAMPLE)
def test_dpm2m_step_contract(per):
    """B = 4 at t = (0, 1, K // 2, K - 1), K = 10 of 1000 on the log-SNR selection: the final step, both second-order rows and the
    first step in one launch, NaN history where c_1 = 0.  per_sample 1 / 5 / 4099: one element, a float4 and a rest, samples that
    start inside a float4 and a rest after many vectors.  Clip off and on."""
    check_case("B4_per%d" % per, 4, per)


def test_dpm2m_step_unaligned_pointers_give_the_aligned_bits():
    for B, per in ((4, 37), (4, 4099), (4, 8)):
        a, b = check_case("B%d_per%d" % (B, per), B, per), check_case("B%d_per%d" % (B, per), B, per, shift=1)
        for (xa, ha), (xb_, hb_) in zip(a, b):
            assert torch.equal(bits(xa), bits(xb_)) and torch.equal(bits(ha), bits(hb_)), (B, per)


def test_dpm2m_step_large_extents():
    """3 x 180001 (sample boundaries inside a float4 and inside a workgroup, a scalar rest) and 1 x 2200003 (550000 float4 groups:
    a second trip of the grid-stride loop of 2048 x 256 threads; B = 1 is t = 0, the final step)."""
    check_case("3x180001", *mb.WRAP_SHAPE, clips=(1,))
    check_case("1x2200003", *mb.BIG_SHAPE, clips=(0,))
    # the same extent on a second-order row
    x, eps, hist, t, tab = mb.dpm_case(*mb.BIG_SHAPE, seed=2, nan_hist=False)
    t = torch.tensor([mb.K // 2])
    (xp, b), (x0, b0) = mb.dpm_bound(x, eps, hist, t, tab, 1)
    xo, ho = run_step((x, eps, hist, t, tab), 1)
    held("hig_dpm2m_step.x_prev 1x2200003 t5 clip1", xo, xp, b)
    held("hig_dpm2m_step.hist 1x2200003 t5 clip1", ho, x0, b0)


def test_dpm2m_refusals_write_nothing():
    B, group, per = 4, 2, 6
    x2, eps2, hist, t2, tab = mb.cfg_case(B, group, per, seed=5)
    ed, td, tabd = (v.contiguous().to(DEV) for v in (eps2, t2, tab))
    xb, hb = Buf.flat(2 * B * per), Buf.flat(B * per)
    nan, inf = float("nan"), float("inf")
    good = dict(x=xb.p(), eps=P(ed), s=2.5, hist=hb.p(), t=P(td), tab=P(tabd), nsteps=K, B=B, group=group, per=per, clip=1)
    null = [(n + " NULL", {n: None}) for n in ("x", "eps", "hist", "t", "tab")]
    sizes = [("%s = %d" % (k, v), {k: v}) for k in ("B", "per", "nsteps") for v in (0, -2)]
    for what, change in null + sizes:
        a = dict(good, **change)
        rc = lib().hig_dpm2m_step(a["x"], a["eps"], a["hist"], a["t"], a["tab"], a["nsteps"], a["B"], a["per"], a["clip"], S())
        assert rc == EINVAL, "hig_dpm2m_step, %s: returned %d" % (what, rc)
        refused(rc, (xb, hb), "hig_dpm2m_step, " + what)
    cfg_only = [("group = 0", dict(group=0)), ("group = -2", dict(group=-2)), ("B % group != 0", dict(group=3)),
                ("scale NaN", dict(s=nan)), ("scale inf", dict(s=inf)), ("scale -inf", dict(s=-inf))]
    for what, change in null + sizes + cfg_only:
        a = dict(good, **change)
        rc = lib().hig_dpm2m_step_cfg(a["x"], a["eps"], a["s"], a["hist"], a["t"], a["tab"], a["nsteps"], a["B"], a["group"],
                                      a["per"], a["clip"], S())
        assert rc == EINVAL, "hig_dpm2m_step_cfg, %s: returned %d" % (what, rc)
        refused(rc, (xb, hb), "hig_dpm2m_step_cfg, " + what)


# ----------------------------------------------------------------------------------------------------------------------
# 2. hig_dpm2m_step_cfg
# ----------------------------------------------------------------------------------------------------------------------
def run_step_cfg(case, s, B, group, clip, shift=0):
    """(conditional rows, unconditional rows, hist_out) of one guided launch."""
    x2, eps2, hist, t2, tab = case
    per = hist.shape[1]
    ed = torch.cat([torch.zeros(shift), eps2.flatten()]).to(DEV)
    td, tabd = t2.to(DEV), tab.to(DEV)
    xb, hb = Buf.flat(2 * B * per + shift), Buf.flat(B * per + shift)
    xb.out.zero_(), hb.out.zero_()
    xb.out[0, shift:].copy_(x2.flatten().to(DEV))
    hb.out[0, shift:].copy_(hist.flatten().to(DEV))
    ok(lib().hig_dpm2m_step_cfg(xb.p(shift), P(ed, shift), s, hb.p(shift), P(td), P(tabd), tab.shape[1], B, group, per, clip, S()))
    xo, ho = xb.written("hig_dpm2m_step_cfg state"), hb.written("hig_dpm2m_step_cfg hist")
    assert shift == 0 or (xo[0, 0].item() == 0 and ho[0, 0].item() == 0)
    c, u = split_rows(xo[0, shift:].view(2 * B, per), group)
    return c, u, ho[0, shift:].view(B, per)


@pytest.mark.parametrize("B,group", ((4, 4), (4, 2)))
@pytest.mark.parametrize("per", (5, 6, 4099))
def test_dpm2m_step_cfg_contract(per, B, group):
    """group = B and group = B / 2; per 5 and 4099 run the scalar loop, per 6 (group * per % 4 == 0) the float4 path, with
    vectors that straddle samples, and there the same operands one element off give the same bits.  Unequal state rows (no
    loop produces them) show a kernel that reads the wrong one; both rows come back equal."""
    case = mb.cfg_case(B, group, per, seed=per + group, unequal=True)
    x2, eps2, hist, t2, tab = case
    for s in (2.5, -1.0, 0.0):
        for clip in mb.CLIPS:
            (xp, b), (x0, b0) = mb.cfg_bound(x2, eps2, hist, t2, tab, s, B, group, clip)
            c, u, ho = run_step_cfg(case, s, B, group, clip)
            what = "B%d_g%d_per%d s%g clip%d" % (B, group, per, s, clip)
            assert torch.equal(bits(c), bits(u)), what + ": the two rows of a sample differ"
            held("hig_dpm2m_step_cfg.x_prev " + what, c, xp, b)
            held("hig_dpm2m_step_cfg.hist " + what, ho, x0, b0)
            if group * per % 4 == 0:
                c1, u1, h1 = run_step_cfg(case, s, B, group, clip, shift=1)
                assert torch.equal(bits(c1), bits(c)) and torch.equal(bits(u1), bits(c)) and torch.equal(bits(h1), bits(ho)), what


@pytest.mark.parametrize("B,group", ((4, 4), (4, 2)))
def test_equal_branches_give_the_unguided_kernel_s_bits(B, group):
    for per in (6, 4099):
        case = mb.cfg_case(B, group, per, seed=9, equal_eps=True)
        x2, eps2, hist, t2, tab = case
        rc, _ = cb.rows(B, group)
        for clip in mb.CLIPS:
            want_x, want_h = run_step((x2[rc], eps2[rc], hist, t2[rc], tab), clip)
            c, u, ho = run_step_cfg(case, 2.5, B, group, clip)
            assert torch.equal(bits(c), bits(want_x)) and torch.equal(bits(u), bits(want_x)) and torch.equal(bits(ho), bits(want_h))


def test_dpm2m_step_cfg_large_extents():
    for B, group, per in (cb.WRAP_SHAPE, cb.BIG_SHAPE):
        case = mb.cfg_case(B, group, per, seed=3)
        x2, eps2, hist, t2, tab = case
        (xp, b), (x0, b0) = mb.cfg_bound(x2, eps2, hist, t2, tab, 2.5, B, group, 1)
        c, u, ho = run_step_cfg(case, 2.5, B, group, 1)
        assert torch.equal(bits(c), bits(u))
        held("hig_dpm2m_step_cfg.x_prev %dx%d_g%d" % (B, per, group), c, xp, b)
        held("hig_dpm2m_step_cfg.hist %dx%d_g%d" % (B, per, group), ho, x0, b0)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the class: the fused step, the loops
# ----------------------------------------------------------------------------------------------------------------------
def test_fused_step_is_the_kernel_and_agrees_with_the_tensor_op_step():
    sd = logsnr_spaced()
    x, eps, hist, t, tab = mb.dpm_case(4, 4099, seed=11)
    assert torch.equal(sd.dpm_solver_table(DEV).cpu(), tab)
    xd, ed, hd, td = (v.to(DEV) for v in (x, eps, hist, t))
    for clip in (False, True):
        (xp, b), (x0, b0) = mb.dpm_bound(x, eps, hist, t, tab, int(clip))
        r, launches = spied(lambda: sd.dpm_solver_sample(lambda *_a, **_k: ed, xd, td, prev_xstart=hd, clip_denoised=clip))
        assert launches == ["hig_dpm2m_step"], launches
        assert torch.equal(bits(xd.cpu()), bits(x)) and torch.equal(bits(hd.cpu()), bits(hist))     # the caller's tensors are left alone
        held("fused dpm_solver_sample.sample clip%d" % clip, r["sample"].cpu(), xp, b)
        held("fused dpm_solver_sample.pred_xstart clip%d" % clip, r["pred_xstart"].cpu(), x0, b0)
        host = sd.dpm_solver_sample(lambda *_a, **_k: eps, x, t, prev_xstart=hist, clip_denoised=clip)
        held("tensor-op dpm_solver_sample.sample clip%d" % clip, host["sample"], xp, b)
        held("tensor-op dpm_solver_sample.pred_xstart clip%d" % clip, host["pred_xstart"], x0, b0)
        print("FUSED vs tensor-op clip%d bitwise %s" % (clip, torch.equal(bits(r["sample"].cpu()), bits(host["sample"]))))
        # first order for the call: no history at all
        r1, launches = spied(lambda: sd.dpm_solver_sample(lambda *_a, **_k: ed, xd, td, clip_denoised=clip))
        assert launches == ["hig_dpm2m_step"]
        (xp1, b1), _ = mb.dpm_bound(x, eps, torch.zeros_like(x), t, mb.dpm_table(1), int(clip))
        held("fused dpm_solver_sample order 1 clip%d" % clip, r1["sample"].cpu(), xp1, b1)
    # a denoised_fn takes the tensor-op path on the device
    r, launches = spied(lambda: sd.dpm_solver_sample(lambda *_a, **_k: ed, xd, td, prev_xstart=hd, denoised_fn=lambda v: v))
    assert "hig_dpm2m_step" not in launches
    (xp, b), _ = mb.dpm_bound(x, eps, hist, t, tab, 1)
    held("device tensor-op dpm_solver_sample", r["sample"].cpu(), xp, b)


def loop_case(kind):
    """(model, bare model, kwargs, shape, start, conditioning) of one parametrised loop case."""
    if kind == "bf16":
        m, kw, shape, x0 = setup16()
        return m, kw, shape, x0, {}
    if kind in ("guided", "guided_known"):
        gm, m, kw, un, shape, x0 = guided_setup()
        return gm, kw, shape, x0, (dict(zip(("known", "known_mask"), known_for(shape))) if kind == "guided_known" else {})
    m, kw, shape, x0 = loop_setup()
    cond = dict(zip(("known", "known_mask"), known_for(shape))) if kind == "known" else {}
    return m, kw, shape, x0, cond


@pytest.mark.parametrize("kind", ("plain", "known", "guided", "guided_known", "bf16"))
def test_captured_loop_equals_eager_loop(kind):
    model, kw, shape, x0, cond = loop_case(kind)
    outs = []
    for use_graph in (False, True):
        sd = logsnr_spaced()
        sd.use_hip_graph, sd._debug_zero_noise = use_graph, True
        undo = patch_randn(randn_like=lambda v, **_: torch.zeros_like(v)) if not use_graph else (lambda: None)
        try:
            (out, launches), n = counting_replays(lambda: spied(lambda: sd.dpm_solver_sample_loop(
                model, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, **cond)))
        finally:
            undo()
        assert n == (K if use_graph else 0)
        ours = [x for x in launches if x.startswith(SAMPLER_KERNELS)]
        if use_graph:       # the warm-up step and the captured one: the imposition where asked for, ONE update kernel, the counter
            cfg = "_cfg" if kind.startswith("guided") else ""
            impose = ["hig_impose_known" + cfg] if kind.endswith("known") else []
            assert ours == (impose + ["hig_dpm2m_step" + cfg, "hig_advance_timesteps"]) * 2
        else:
            assert ours.count("hig_dpm2m_step") == K and "hig_ddim_step" not in ours
        outs.append(out)
    eager, captured = outs
    assert captured.shape == shape and torch.isfinite(captured).all()
    e = rel(captured, eager)
    print("LOOP dpmpp2m captured vs eager %s rel %.3e" % (kind, e))
    assert e == 0.0


def test_captured_loop_draws_no_noise_and_differs_from_first_order():
    m, kw, shape, x0 = loop_setup()
    sd = logsnr_spaced()
    run = lambda **k: sd.dpm_solver_sample_loop(m, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, **k)  # noqa: E731
    torch.manual_seed(1)
    a = run()
    torch.manual_seed(2)
    b = run()
    assert torch.equal(a, b)                                        # no noise node: the same start gives the same bits
    first = run(order=1)
    assert torch.isfinite(first).all() and rel(first, a) > 1e-4     # the history term does something
    ddim = sd.ddim_sample_loop(m, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, eta=0.0)
    e = rel(first, ddim)
    print("LOOP dpmpp2m order 1 vs ddim eta 0, log-SNR steps: rel %.3e" % e)
    assert e < 1e-5                                                 # order 1 is DDIM at eta = 0 in other arithmetic


def test_captured_first_order_loop_matches_the_reference_s_ddim_golden(gold):
    """Golden G16's DDIM eta = 0 loop (uniform steps, K = 10) through the captured order=1 solver: the gate
    test_gpu_few_step.py applies to that golden."""
    g = gold("g16_few_step.npz")
    m, kw, shape, x0 = loop_setup()
    final, n = counting_replays(lambda: spaced().dpm_solver_sample_loop(m, shape, noise=x0.clone(), clip_denoised=False,
                                                                         model_kwargs=kw, order=1))
    assert n == K
    e = rel(final, g["loop.ddim.eta0"])
    print("LOOP dpmpp2m order 1 vs g16 loop.ddim.eta0: rel %.3e" % e)
    assert e < 2e-4


# ----------------------------------------------------------------------------------------------------------------------
# 4. trainers
# ----------------------------------------------------------------------------------------------------------------------
CAPS = ["a person waves", "two people hug", "a person jumps"]


def test_trainer_generates_with_dpmpp2m():
    c = fill.CASES["tiny"]
    m = build(c).eval()
    tr = _trainer(c, m)
    F = c["F"]
    lens = torch.tensor([16, 12, 9])
    tr.set_sampler(steps=10, method="dpmpp2m")
    (outs, launches), n = counting_replays(lambda: spied(lambda: tr.generate(CAPS, lens, F, batch_size=2)))
    assert n == 2 * K and "hig_dpm2m_step" in launches and "hig_ddim_step" not in launches and "hig_p_sample_step" not in launches
    assert [tuple(o.shape) for o in outs] == [(16, F), (16, F), (9, F)] and all(torch.isfinite(o).all() for o in outs)
    torch.manual_seed(3)
    got = tr.generate_batch(CAPS, lens, F)
    xf_proj, xf_out = m.encode_text(CAPS, tr.device)
    torch.manual_seed(3)
    want = logsnr_spaced().dpm_solver_sample_loop(m, (3, 16, F), clip_denoised=False,
                                                  model_kwargs=dict(xf_proj=xf_proj, xf_out=xf_out, length=lens))
    assert torch.equal(got, want)
    # guided, with a known region: the loop called directly on the wrapper
    tr.set_sampler(steps=10, method="dpmpp2m", guidance_scale=2.5)
    known, mask = known_for((3, c["num_frames"], F))
    torch.manual_seed(5)
    (got, launches), n = counting_replays(lambda: spied(lambda: tr.generate_batch(LONG, lens, F, known=known, known_mask=mask)))
    assert n == K and "hig_dpm2m_step_cfg" in launches and "hig_impose_known_cfg" in launches
    xf_proj, xf_out = m.encode_text(LONG, tr.device)
    up, uo = m.encode_text([""], tr.device)
    gm = hig_amd.ClassifierFreeGuidedModel(m, 2.5, dict(xf_proj=up, xf_out=uo))
    torch.manual_seed(5)
    want = logsnr_spaced().dpm_solver_sample_loop(gm, (3, 16, F), clip_denoised=False,
                                                  model_kwargs=dict(xf_proj=xf_proj, xf_out=xf_out, length=lens),
                                                  known=known[:, :16], known_mask=mask[:, :16])
    assert torch.isfinite(got).all() and torch.equal(got, want)
    # back to the full chain
    tr.set_sampler(None)
    seen = []
    tr.diffusion.p_sample_loop = lambda model, shape, **kw: (seen.append(shape), torch.zeros(shape, device=DEV))[1]
    tr.generate_batch(CAPS, lens, F)
    assert seen == [(3, 16, F)]


def test_two_person_trainer_generates_with_dpmpp2m():
    c = fill.ICASES["tiny2"]
    m = build_pair(c).eval()
    tr = _mul_trainer(c, m)
    T, Fd = c["T"], c["F"]
    lens = torch.tensor([T, 9])
    tr.set_sampler(steps=10, method="dpmpp2m")
    torch.manual_seed(8)
    (outs, launches), n = counting_replays(lambda: spied(lambda: tr.generate(LONG1, LONG2, lens, Fd)))
    assert n == K and "hig_dpm2m_step" in launches
    assert len(outs) == 2 and all(len(o) == 2 and o[0].shape == (T, Fd) and o[1].shape == (T, Fd) for o in outs)
    assert all(torch.isfinite(o[0]).all() and torch.isfinite(o[1]).all() for o in outs)
    xf_proj, xf_out = m.encode_text(list(LONG1) + list(LONG2), tr.device)
    torch.manual_seed(8)
    want = logsnr_spaced().dpm_solver_sample_loop(m, (4, T, Fd), clip_denoised=False,
                                                  model_kwargs=dict(xf_proj=xf_proj, xf_out=xf_out, length=torch.cat([lens, lens])))
    assert torch.equal(torch.stack([o[0] for o in outs] + [o[1] for o in outs]), want)
    tr.set_sampler(steps=10, method="dpmpp2m", guidance_scale=2.5)
    guided, launches = spied(lambda: tr.generate(LONG1, LONG2, lens, Fd))
    assert "hig_dpm2m_step_cfg" in launches and all(torch.isfinite(o[0]).all() and torch.isfinite(o[1]).all() for o in guided)
    tr.set_sampler(None)
    seen = []
    tr.diffusion.p_sample_loop = lambda model, shape, **kw: (seen.append(shape), torch.zeros(shape, device=DEV))[1]
    tr.generate_batch(LONG1, LONG2, lens, Fd)
    assert seen == [(4, T, Fd)]
