"""Classifier-free guidance on the MI355X: the contract of hig_cfg_combine / hig_p_sample_step_cfg / hig_ddim_step_cfg /
hig_impose_known_cfg (every element within the bound of tests/cfg_bounds.py, both rows of the stacked state written with the same
bits, nothing around them touched, every refusal silent, the scalar path bit-equal to the float4 path), the wrapper and the
captured guided loops against what the reference computes with a three-line wrapper of its own (golden G19), captured against
eager, the launch sequence of a guided step, and the trainers.

Measured on an MI355X (largest |error| / bound over all cases; `pytest -s` prints the RATIO / GATE / LOOP lines this was collected
from):
    hig_cfg_combine                      0.994   three roundings under a bound that counts exactly those
    hig_ddim_step_cfg.pred_xstart        0.973   x_prev 0.661
    hig_p_sample_step_cfg.pred_xstart    0.774   x_prev 0.893 (the kernel fuses three of the roundings the bound counts)
    eps_u == eps_c: both guided steps are bit for bit the unguided kernels
Against G19 (s = 2.5), per-sample rel-L2 / max(1e-6, 4 floor): guided ddim_sample 0.000 (bit for bit the reference's, through the
wrapper and through hig_ddim_step_cfg), guided p_sample 0.073 / pred_xstart 0.046.  Captured guided K = 10 DDIM loop: rel 8.6e-07,
0.0043 of the 2e-4 gate (the fp32 reference is 7.1e-07 from its fp64 self).  Captured vs eager: rel 0 in all twelve cases.  s = 1 vs
the conditional loop 1.7e-07, s = 0 vs the unconditional loop 0.  One stacked 2 B forward vs two B forwards: rel 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import cfg_bounds as cb  # noqa: E402
import ddim_bounds as db  # noqa: E402
import hig_amd  # noqa: E402
import known_bounds as kb  # noqa: E402
import rowops_bounds as rb  # noqa: E402
from hig_amd.models import gaussian_diffusion as gdm  # noqa: E402
from hig_amd.models.guidance import split_rows, stack_rows  # noqa: E402
from oracle import fill  # noqa: E402
from test_gpu_bf16_storage import CASES16  # noqa: E402
from test_gpu_bf16_storage import build as build16  # noqa: E402
from test_gpu_denoiser import _trainer, build, rel  # noqa: E402
from test_gpu_few_step import K, loop_setup, patch_randn, spaced  # noqa: E402
from test_gpu_interaction import _trainer as _mul_trainer  # noqa: E402
from test_gpu_interaction import build as build_pair  # noqa: E402
from test_gpu_known_region import counting_replays, gate_of, known_for, rel_rows, spied  # noqa: E402
from test_gpu_rowops_contract import DEV, Buf, P, S, held, lib, ok, refused  # noqa: E402

EINVAL = -1
S_GOLD = 2.5


def bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the step kernels and the combine
# ----------------------------------------------------------------------------------------------------------------------
def step_call(kind, xp, ep, s, zp, tp, tabp, nsteps, B, group, per, eta, clip, predp):
    if kind == "ddim":
        return lib().hig_ddim_step_cfg(xp, ep, s, zp, tp, tabp, nsteps, B, group, per, eta, clip, predp, S())
    return lib().hig_p_sample_step_cfg(xp, ep, s, zp, tp, tabp, nsteps, B, group, per, predp, S())


def bounds_of(kind, x2, eps2, z, t2, tab, s, B, group, eta, clip):
    if kind == "ddim":
        return cb.ddim_bound(x2, eps2, z, t2, tab, s, B, group, eta, clip)
    return cb.p_bound(x2, eps2, z, t2, tab, s, B, group)


def run_step(kind, case, s, B, group, per, eta, clip, shift=0, with_pred=True):
    """One launch on guarded buffers; returns (both rows of the new state as (rc rows, ru rows), pred_xstart or None)."""
    x2, eps2, z, t2, tab = case
    pad = lambda v: torch.cat([torch.zeros(shift, dtype=v.dtype), v.flatten()]).to(DEV)  # noqa: E731
    ed, zd, td, tabd = pad(eps2), pad(z), t2.to(DEV), tab.to(DEV)
    xb, pb = Buf.flat(2 * B * per + shift), Buf.flat(B * per + shift)
    xb.out.zero_(), pb.out.zero_()
    xb.out[0, shift:].copy_(x2.flatten().to(DEV))
    zp = None if kind == "ddim" and eta == 0 else P(zd, shift)
    ok(step_call(kind, xb.p(shift), P(ed, shift), s, zp, P(td), P(tabd), tab.shape[1], B, group, per, eta, clip,
                 pb.p(shift) if with_pred else None))
    xb.guards(kind + " state")
    pb.guards(kind + " pred_xstart")
    assert shift == 0 or (xb.out[0, 0].item() == 0 and pb.out[0, 0].item() == 0)
    c, u = split_rows(xb.out.cpu()[0, shift:].view(2 * B, per), group)
    return c, u, (pb.out.cpu()[0, shift:].view(B, per) if with_pred else None)


def check_step(kind, tag, B, group, per, scales=cb.SCALES, etas=cb.ETAS, clips=cb.CLIPS, unequal=False, shift=0):
    case = cb.cfg_case(B, group, per, "ddim" if kind == "ddim" else "p", seed=per + B, unequal=unequal)
    x2, eps2, z, t2, tab = case
    for s in scales:
        for eta in (etas if kind == "ddim" else (0.0,)):
            for clip in (clips if kind == "ddim" else (0,)):
                zz = None if kind == "ddim" and eta == 0 else z
                (xp, b), (x0, b0) = bounds_of(kind, x2, eps2, zz, t2, tab, s, B, group, eta, clip)
                what = "%s s%g eta%g clip%d" % (tag, s, eta, clip)
                c, u, pred = run_step(kind, case, s, B, group, per, eta, clip, shift)
                assert not torch.isnan(c).any(), what
                assert torch.equal(bits(c), bits(u)), what + ": the two rows of a sample differ"
                name = "hig_ddim_step_cfg" if kind == "ddim" else "hig_p_sample_step_cfg"
                held("%s.x_prev %s" % (name, what), c, xp, b)
                held("%s.pred_xstart %s" % (name, what), pred, x0, b0)
                c2, _, none = run_step(kind, case, s, B, group, per, eta, clip, shift, with_pred=False)
                assert none is None and torch.equal(bits(c2), bits(c)), what + ": pred_xstart NULL changes the state"


@pytest.mark.parametrize("B,group", cb.BG)
@pytest.mark.parametrize("per", cb.PER_SAMPLE)
@pytest.mark.parametrize("kind", ("ddim", "p_sample_step"))
def test_step_cfg_contract(kind, per, B, group):
    """per_sample 1 / 5 / 4099 x (B, group) (1, 1) / (3, 3) / (4, 2) / (6, 3) x every scale, eta and clip value.  None of these
    has group * per % 4 == 0: they all run the scalar loop; test_vector_path_has_the_scalar_path_s_bits holds the float4 path to
    the same bound and to the same bits."""
    check_step(kind, "B%d_g%d_per%d" % (B, group, per), B, group, per)


@pytest.mark.parametrize("kind", ("ddim", "p_sample_step"))
def test_step_cfg_reads_the_state_at_the_conditional_row(kind):
    """Unequal state rows (no loop produces them): x comes from rc, and both rows are overwritten with the one result."""
    for B, group, per in ((4, 2, 5), (6, 3, 8), (3, 3, 4099)):
        check_step(kind, "unequal_B%d_g%d_per%d" % (B, group, per), B, group, per, scales=(2.5,), etas=(0.5,), clips=(1,),
                   unequal=True)


@pytest.mark.parametrize("kind", ("ddim", "p_sample_step", "combine"))
def test_vector_path_has_the_scalar_path_s_bits(kind):
    """group * per % 4 == 0 with aligned pointers takes the float4 path; the same operands one element past a 16-byte boundary
    take the scalar path: the same bits.  (4, 2, 6): a float4 straddles samples; (6, 3, 4100): many groups, sample boundaries on
    float4 boundaries; (2, 1, 4): one group per block."""
    for B, group, per in ((4, 2, 6), (6, 3, 4100), (2, 1, 4)):
        assert group * per % 4 == 0
        case = cb.cfg_case(B, group, per, "ddim" if kind != "p_sample_step" else "p", seed=7 * per)
        if kind == "combine":
            outs = [run_combine(case[1], 2.5, B, group, per, shift) for shift in (0, 1)]
            eg, e_g = cb.combine_bound(case[1], 2.5, B, group)
            held("hig_cfg_combine vec B%d_g%d_per%d" % (B, group, per), outs[0], eg, e_g)
            assert torch.equal(bits(outs[0]), bits(outs[1]))
            continue
        check_step(kind, "vec_B%d_g%d_per%d" % (B, group, per), B, group, per, scales=(2.5,), etas=(0.0, 1.0), clips=(0, 1))
        for eta, clip in ((0.0, 0), (1.0, 1)):
            a = run_step(kind, case, 2.5, B, group, per, eta, clip, shift=0)
            b = run_step(kind, case, 2.5, B, group, per, eta, clip, shift=1)
            for va, vb in zip(a, b):
                assert torch.equal(bits(va), bits(vb)), (kind, B, group, per, eta, clip)


def test_step_cfg_unaligned_and_odd_extents_take_the_scalar_path():
    for kind in ("ddim", "p_sample_step"):
        check_step(kind, "shifted_B4_g2_per37", 4, 2, 37, scales=(2.5, -1.0), etas=(0.5,), clips=(1,), shift=1)


def test_step_cfg_large_extents():
    """4 x 135001 in blocks of 2 (sample and block boundaries inside a workgroup, group * per % 4 != 0: the scalar loop wraps),
    3 x 180001 (ddim_bounds.WRAP_SHAPE) and 2 x 1100002 in blocks of 1 (550000 float4 groups: a second trip of the vector loop of
    2048 x 256 threads)."""
    for B, group, per in (cb.WRAP_SHAPE, cb.WRAP_ODD, cb.BIG_SHAPE):
        for kind in ("ddim", "p_sample_step"):
            check_step(kind, "%dx%d_g%d" % (B, per, group), B, group, per, scales=(2.5,), etas=(1.0,), clips=(1,))


def run_combine(eps2, s, B, group, per, shift=0):
    ed = torch.cat([torch.zeros(shift), eps2.flatten()]).to(DEV)
    ob = Buf.flat(B * per + shift)
    ob.out.zero_()
    ok(lib().hig_cfg_combine(P(ed, shift), s, B, group, per, ob.p(shift), S()))
    ob.guards("hig_cfg_combine")
    assert torch.equal(bits(ed.cpu()[shift:]), bits(eps2.flatten())), "hig_cfg_combine modified its input"
    return ob.out.cpu()[0, shift:].view(B, per)


@pytest.mark.parametrize("B,group", cb.BG)
@pytest.mark.parametrize("per", cb.PER_SAMPLE)
def test_cfg_combine_contract(per, B, group):
    eps2 = cb.cfg_case(B, group, per, "ddim", seed=per + B)[1]
    for s in cb.SCALES:
        eg, e_g = cb.combine_bound(eps2, s, B, group)
        held("hig_cfg_combine B%d_g%d_per%d s%g" % (B, group, per, s), run_combine(eps2, s, B, group, per), eg, e_g)


def test_cfg_combine_large_extents():
    for B, group, per in (cb.WRAP_SHAPE, cb.BIG_SHAPE):
        eps2 = cb.cfg_case(B, group, per, "ddim", seed=3)[1]
        eg, e_g = cb.combine_bound(eps2, 7.5, B, group)
        held("hig_cfg_combine %dx%d_g%d" % (B, per, group), run_combine(eps2, 7.5, B, group, per), eg, e_g)


def test_equal_branches_give_the_unguided_kernel():
    """eps_u == eps_c: the guided step is the unguided kernel on the conditional rows -- to within what the combine's one
    remaining rounding (u |eps_g|, carried through the step) allows; it is in fact bit for bit."""
    B, group, per = 4, 2, 4099
    for kind in ("ddim", "p_sample_step"):
        x2, eps2, z, t2, tab = cb.cfg_case(B, group, per, "ddim" if kind == "ddim" else "p", seed=9)
        rc, ru = cb.rows(B, group)
        eps2[ru] = eps2[rc]
        xd, ed, zd, td, tabd = (v.contiguous().to(DEV) for v in (x2[rc], eps2[rc], z, t2[rc], tab))
        o1, o0 = Buf.flat(B * per), Buf.flat(B * per)
        if kind == "ddim":
            ok(lib().hig_ddim_step(P(xd), P(ed), P(zd), P(td), P(tabd), tab.shape[1], B, per, 0.5, 1, o1.p(), o0.p(), S()))
            (_, bg), (_, bg0) = cb.ddim_bound(x2, eps2, z, t2, tab, 2.5, B, group, 0.5, 1)
            (_, bu), (_, bu0) = db.ddim_bound(x2[rc], eps2[rc], z, t2[rc], tab, 0.5, 1)
        else:
            ok(lib().hig_p_sample_step(P(xd), P(ed), P(zd), P(td), P(tabd), tab.shape[1], B, per, o1.p(), o0.p(), S()))
            (_, bg), (_, bg0) = cb.p_bound(x2, eps2, z, t2, tab, 2.5, B, group)
            (_, bu), (_, bu0) = rb.p_step_bound(x2[rc], eps2[rc], z, t2[rc], tab)
        want, want0 = o1.written("unguided x_prev").view(B, per), o0.written("unguided pred_xstart").view(B, per)
        c, u, pred = run_step(kind, (x2, eps2, z, t2, tab), 2.5, B, group, per, 0.5, 1)
        assert ((c.double() - want.double()).abs() <= bg - bu).all() and ((pred.double() - want0.double()).abs() <= bg0 - bu0).all()
        print("EQUAL %s bitwise %s" % (kind, torch.equal(bits(c), bits(want)) and torch.equal(bits(pred), bits(want0))))


def test_cfg_refusals_write_nothing():
    B, group, per = 4, 2, 6
    x2, eps2, z, t2, tab = cb.cfg_case(B, group, per, "ddim", seed=5)
    ed, zd, td, tabd = (v.contiguous().to(DEV) for v in (eps2, z, t2, tab))
    ptab = rb.ddpm_table(cb.P_NSTEPS).to(DEV)
    xb, pb, ob = Buf.flat(2 * B * per), Buf.flat(B * per), Buf.flat(B * per)
    nan, inf = float("nan"), float("inf")
    good = dict(x=xb.p(), eps=P(ed), s=2.5, z=P(zd), t=P(td), tab=P(tabd), nsteps=K, B=B, group=group, per=per, eta=0.5, clip=1,
                pred=pb.p())
    shape_bad = [("%s = %d" % (k, v), {k: v}) for k in ("B", "group", "per", "nsteps") for v in (0, -2)]
    shape_bad += [("B % group != 0", dict(group=3)), ("scale NaN", dict(s=nan)), ("scale inf", dict(s=inf)),
                  ("scale -inf", dict(s=-inf))]
    null = lambda *names: [(n + " NULL", {n: None}) for n in names]  # noqa: E731
    for what, change in null("x", "eps", "t", "tab") + shape_bad + [("z NULL with eta > 0", dict(z=None)), ("eta < 0", dict(eta=-0.5)),
                                                                     ("eta NaN", dict(eta=nan)), ("eta inf", dict(eta=inf))]:
        a = dict(good, **change)
        rc = step_call("ddim", a["x"], a["eps"], a["s"], a["z"], a["t"], a["tab"], a["nsteps"], a["B"], a["group"], a["per"],
                       a["eta"], a["clip"], a["pred"])
        assert rc == EINVAL, "hig_ddim_step_cfg, %s: returned %d" % (what, rc)
        refused(rc, (xb, pb), "hig_ddim_step_cfg, " + what)
    for what, change in null("x", "eps", "z", "t", "tab") + shape_bad:
        a = dict(dict(good, tab=P(ptab), nsteps=cb.P_NSTEPS), **change)
        rc = step_call("p", a["x"], a["eps"], a["s"], a["z"], a["t"], a["tab"], a["nsteps"], a["B"], a["group"], a["per"], 0.0, 0,
                       a["pred"])
        assert rc == EINVAL, "hig_p_sample_step_cfg, %s: returned %d" % (what, rc)
        refused(rc, (xb, pb), "hig_p_sample_step_cfg, " + what)
    for what, change in [("eps2 NULL", dict(eps=None)), ("eps_out NULL", dict(out=None))] + [c for c in shape_bad if "nsteps" not in c[0]]:
        a = dict(dict(good, out=ob.p()), **change)
        rc = lib().hig_cfg_combine(a["eps"], a["s"], a["B"], a["group"], a["per"], a["out"], S())
        assert rc == EINVAL, "hig_cfg_combine, %s: returned %d" % (what, rc)
        refused(rc, (ob,), "hig_cfg_combine, " + what)
    md = torch.ones(B * per, dtype=torch.uint8, device=DEV)
    for what, change in null("x", "known", "mask", "z", "t", "tab") + [c for c in shape_bad if "scale" not in c[0]]:
        a = dict(dict(good, known=P(zd), mask=P(md), tab=P(ptab), nsteps=cb.P_NSTEPS), **change)
        rc = lib().hig_impose_known_cfg(a["x"], a["known"], a["mask"], a["z"], a["t"], a["tab"], a["nsteps"], a["B"], a["group"],
                                        a["per"], S())
        assert rc == EINVAL, "hig_impose_known_cfg, %s: returned %d" % (what, rc)
        refused(rc, (xb,), "hig_impose_known_cfg, " + what)
    # the accepted form next to them: z NULL at eta == 0
    xb.out.copy_(x2.view(1, -1).to(DEV))
    ok(step_call("ddim", xb.p(), P(ed), 2.5, None, P(td), P(tabd), K, B, group, per, 0.0, 1, None))
    xb.written("eta 0, z NULL")


# ----------------------------------------------------------------------------------------------------------------------
# 2. hig_impose_known_cfg
# ----------------------------------------------------------------------------------------------------------------------
def run_impose_cfg(B, group, per, kind, shift=0):
    x, known, z, mask, t, tab = kb.impose_case(B, per, kind, seed=per)
    other = torch.randn(B, per, generator=torch.Generator().manual_seed(per)) + 3.0     # the unconditional rows: other bits
    x2, t2 = cb.stack(x, other, group), cb.stack(t, t, group)
    pad = lambda v: torch.cat([torch.zeros(shift, dtype=v.dtype), v.flatten()]).to(DEV)  # noqa: E731
    kd, zd, md, td, tabd = pad(known), pad(z), pad(mask), t.to(DEV), tab.to(DEV)
    # the unguided kernel on the conditional rows
    ub = Buf.flat(B * per + shift)
    ub.out.zero_()
    ub.out[0, shift:].copy_(x.flatten().to(DEV))
    ok(lib().hig_impose_known(ub.p(shift), P(kd, shift), P(md, shift), P(zd, shift), P(td), P(tabd), kb.NSTEPS, B, per, S()))
    want = ub.out.cpu()[0, shift:].view(B, per)
    xb = Buf.flat(2 * B * per + shift)
    xb.out.zero_()
    xb.out[0, shift:].copy_(x2.flatten().to(DEV))
    ok(lib().hig_impose_known_cfg(xb.p(shift), P(kd, shift), P(md, shift), P(zd, shift), P(t2.to(DEV)), P(tabd), kb.NSTEPS, B,
                                  group, per, S()))
    what = "hig_impose_known_cfg B%d g%d per%d %s shift%d" % (B, group, per, kind, shift)
    xb.guards(what)
    c, u = split_rows(xb.out.cpu()[0, shift:].view(2 * B, per), group)
    on = (mask != 0).view(B, per)
    assert torch.equal(bits(c), bits(want)), what + ": the conditional rows differ from hig_impose_known"
    assert torch.equal(bits(u)[on], bits(want)[on]), what + ": the unconditional rows differ on the mask"
    assert torch.equal(bits(u)[~on], bits(other)[~on]), what + ": an unconditional element off the mask changed its bits"
    r, same = kb.check(c, x, known, z, mask, t, tab)
    assert r <= 1.0 and same, what
    return c, u


@pytest.mark.parametrize("B,group", cb.BG)
@pytest.mark.parametrize("per", (1, 5, 8, 4099))
def test_impose_known_cfg_writes_where_impose_known_writes(per, B, group):
    """Under every mask of known_bounds, NaN in known / z off the mask: both rows get hig_impose_known's bits on the mask and
    keep their own off it.  per = 8 at group 1 / 2 / 3: the float4 path where group * per % 4 == 0."""
    for kind in kb.MASKS:
        run_impose_cfg(B, group, per, kind)


def test_impose_known_cfg_vector_and_scalar_paths_and_large_extents():
    for B, group, per in ((4, 2, 6), (6, 3, 4100)):
        for kind in ("bernoulli", "run_across_boundary", "alternating"):
            a, b = run_impose_cfg(B, group, per, kind), run_impose_cfg(B, group, per, kind, shift=1)
            assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    run_impose_cfg(*cb.WRAP_SHAPE, "bernoulli")
    run_impose_cfg(*cb.BIG_SHAPE, "bernoulli")
    run_impose_cfg(*cb.BIG_SHAPE, "last_only")


# ----------------------------------------------------------------------------------------------------------------------
# 3. the wrapper and the loops against the reference
# ----------------------------------------------------------------------------------------------------------------------
def stub_pair(ec, eu):
    """A model of two outputs: eps_c where its xf_proj row is positive, eps_u elsewhere; called on the stacked batch."""
    def model(x2, t2, xf_proj=None, xf_out=None):
        B = ec.shape[0]
        assert x2.shape[0] == 2 * B
        return torch.where(xf_proj[:, 0].view(-1, 1, 1) > 0, stack_rows(ec, ec, B), stack_rows(eu, eu, B))
    model.parameters = lambda: iter([ec])
    return model


def test_guided_steps_match_reference_golden(gold):
    g = gold("g19_cfg.npz")
    sd = spaced()
    x, ec, eu, z, t = (torch.tensor(g[k]).to(DEV) for k in ("x", "eps_c", "eps_u", "z", "t"))
    B = x.shape[0]
    kw = dict(xf_proj=torch.ones(B, 1, device=DEV), xf_out=torch.ones(B, 1, 1, device=DEV))
    un = dict(xf_proj=-torch.ones(1, 1, device=DEV), xf_out=torch.ones(1, 1, 1, device=DEV))
    model = hig_amd.ClassifierFreeGuidedModel(stub_pair(ec, eu), float(g["scale"]), un)
    undo = patch_randn(randn_like=lambda v, **_: z)
    try:
        rows, launches = spied(lambda: {
            "ddim.eta1.clip1": sd.ddim_sample(model, x.clone(), t, clip_denoised=True, eta=1.0, model_kwargs=kw),
            "ddim.eta0.clip0": sd.ddim_sample(model, x.clone(), t, clip_denoised=False, eta=0.0, model_kwargs=kw),
            "p_sample.clip0": sd.p_sample(model, x.clone(), t, clip_denoised=False, model_kwargs=kw)})
    finally:
        undo()
    assert launches == ["hig_cfg_combine", "hig_ddim_step"] * 2 + ["hig_cfg_combine", "hig_p_sample_step"], launches
    for tag, r in rows.items():
        gate = gate_of(g[tag + ".floor"])
        for key in ("sample", "pred_xstart"):
            e = rel_rows(r[key], g["%s.%s" % (tag, key)])
            print("GATE g19 %s.%s %s" % (tag, key, " ".join("%.3f" % v for v in (e / gate).tolist())))
            assert (e <= gate).all(), (tag, key, e.tolist(), gate.tolist())
    # the fused guided kernels on the same operands, on the stacked layout
    tab, ptab = sd.ddim_table(DEV).cpu(), sd.device_table(DEV).cpu()
    for tag, kind, tb, eta, clip in (("ddim.eta1.clip1", "ddim", tab, 1.0, 1), ("ddim.eta0.clip0", "ddim", tab, 0.0, 0),
                                     ("p_sample.clip0", "p", ptab, 0.0, 0)):
        case = (cb.stack(x.cpu().flatten(1), x.cpu().flatten(1), B), cb.stack(ec.cpu().flatten(1), eu.cpu().flatten(1), B),
                z.cpu().flatten(1), cb.stack(t.cpu(), t.cpu(), B), tb)
        c, u, pred = run_step(kind, case, float(g["scale"]), B, B, x[0].numel(), eta, clip)
        gate = gate_of(g[tag + ".floor"])
        for key, got in (("sample", c), ("pred_xstart", pred)):
            e = rel_rows(got, torch.tensor(g["%s.%s" % (tag, key)]).flatten(1))
            print("GATE g19 kernel %s.%s %s" % (tag, key, " ".join("%.3f" % v for v in (e / gate).tolist())))
            assert (e <= gate).all(), (tag, key, e.tolist(), gate.tolist())


def guided_setup(gold_file=None, scale=S_GOLD, storage="f32"):
    """(model under guidance, the bare model, conditional kwargs, unconditional kwargs, shape, start)."""
    if storage == "f32":
        m, kw, shape, x0 = loop_setup()
        tag = "g19.uncond"
    else:
        c = CASES16["small"]
        m = build16(c, storage="bf16").eval()
        inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
        kw = {k: inp[k].to(DEV) for k in ("xf_proj", "xf_out", "length")}
        shape = (c["B"], c["T"], c["F"])
        x0 = (fill.tensor_for("g19.x0.bf16", shape) * 10.0).to(DEV)
        tag = "g19.uncond16"
    un = dict(xf_proj=(fill.tensor_for(tag + ".xf_proj", tuple(kw["xf_proj"].shape)) * 10).to(DEV),
              xf_out=(fill.tensor_for(tag + ".xf_out", tuple(kw["xf_out"].shape)) * 10).to(DEV))
    if storage == "f32":
        x0 = (fill.tensor_for("g19.x0", shape) * 10.0).to(DEV)
    return hig_amd.ClassifierFreeGuidedModel(m, scale, un), m, kw, un, shape, x0


def run_loop(sd, model, shape, x0, kw, method, eta, **cond):
    if method == "ddim":
        return sd.ddim_sample_loop(model, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, eta=eta, **cond)
    if method == "dpmpp2m":
        return sd.dpm_solver_sample_loop(model, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, **cond)
    return sd.p_sample_loop(model, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, **cond)


def test_captured_guided_ddim_loop_matches_reference_golden(gold):
    g = gold("g19_cfg.npz")
    gm, m, kw, un, shape, x0 = guided_setup()
    assert torch.equal(un["xf_proj"].cpu(), torch.tensor(g["uncond.xf_proj"]))      # the inputs the golden was recorded with
    final, n = counting_replays(lambda: run_loop(spaced(), gm, shape, x0, kw, "ddim", 0.0))
    assert n == K and final.shape == shape                          # the captured path, one replay per kept step
    gate = max(2e-4, 2e-4, 4 * float(g["loop.floor"].max()))        # (the issue's 2e-4, the unguided loop gate, 4 x the floor)
    gate = min(gate, 1e-3)
    e = rel(final, g["loop.ddim.eta0"])
    print("LOOP g19 guided ddim eta0: rel %.3e, gate %.1e, ratio %.4f (floor %.1e)" % (e, gate, e / gate, g["loop.floor"].max()))
    assert e < gate


SAMPLER_KERNELS = ("hig_impose_known", "hig_p_sample_step", "hig_ddim_step", "hig_dpm2m_step", "hig_dec_timesteps",
                   "hig_advance_timesteps", "hig_cfg_combine")


@pytest.mark.parametrize("method,eta,with_known", (("ddim", 0.0, False), ("ddim", 1.0, True), ("ddpm", 0.0, True), ("ddpm", 0.0, False),
                                                    ("dpmpp2m", 0.0, False), ("dpmpp2m", 0.0, True)))
def test_guided_step_launches_one_cfg_kernel_for_each_unguided_one(method, eta, with_known):
    gm, m, kw, un, shape, x0 = guided_setup()
    cond = dict(zip(("known", "known_mask"), known_for(shape))) if with_known else {}
    sd = spaced()
    _, plain = spied(lambda: run_loop(sd, m, shape, x0, kw, method, eta, **cond))
    _, guided = spied(lambda: run_loop(sd, gm, shape, x0, kw, method, eta, **cond))
    ours = lambda names: [n for n in names if n.startswith(SAMPLER_KERNELS)]  # noqa: E731
    print("LAUNCHES %s eta%g known%d: %s" % (method, eta, with_known, ours(guided)))
    assert "hig_cfg_combine" not in guided
    assert [n.replace("_cfg", "") for n in guided] == plain         # launch for launch the unguided step (warm-up + capture) ...
    step = {"ddim": "hig_ddim_step", "dpmpp2m": "hig_dpm2m_step", "ddpm": "hig_p_sample_step"}[method]
    want = (["hig_impose_known_cfg"] if with_known else []) + [step + "_cfg"]
    want += ["hig_advance_timesteps"]
    assert ours(guided) == want * 2                                 # ... with one _cfg kernel in the place of each unguided one


@pytest.mark.parametrize("storage", ("f32", "bf16"))
@pytest.mark.parametrize("with_known", (False, True))
@pytest.mark.parametrize("method,eta", (("ddpm", 0.0), ("ddim", 0.0), ("ddim", 1.0)))
def test_guided_captured_loop_equals_eager_loop(method, eta, with_known, storage):
    gm, m, kw, un, shape, x0 = guided_setup(storage=storage)
    cond = dict(zip(("known", "known_mask"), known_for(shape))) if with_known else {}
    outs = []
    for use_graph in (False, True):
        sd = spaced()
        sd.use_hip_graph, sd._debug_zero_noise = use_graph, True
        undo = patch_randn(randn_like=lambda v, **_: torch.zeros_like(v)) if not use_graph else (lambda: None)
        try:
            out, n = counting_replays(lambda: run_loop(sd, gm, shape, x0, kw, method, eta, **cond))
        finally:
            undo()
        assert n == (K if use_graph else 0)
        outs.append(out)
    eager, captured = outs
    assert captured.shape == shape and torch.isfinite(captured).all()
    e = rel(captured, eager)
    print("LOOP guided captured vs eager %s eta%g known%d %s rel %.3e" % (method, eta, with_known, storage, e))
    assert e < 1e-6


def test_guided_full_chain_is_captured_and_equals_eager():
    gm, m, kw, un, shape, x0 = guided_setup()
    gd = hig_amd.GaussianDiffusion(betas=gdm.get_named_beta_schedule("linear", 50), model_mean_type=gdm.ModelMeanType.EPSILON,
                                   model_var_type=gdm.ModelVarType.FIXED_SMALL, loss_type=gdm.LossType.MSE)
    gd._debug_zero_noise = True
    known, mask = known_for(shape)
    call = lambda **c: gd.p_sample_loop(gm, shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw, **c)  # noqa: E731
    (captured, launches), n = counting_replays(lambda: spied(lambda: call(known=known, known_mask=mask)))
    assert n == 50 and [x for x in launches if x.startswith(SAMPLER_KERNELS)] == ["hig_impose_known_cfg", "hig_p_sample_step_cfg",
                                                                                  "hig_dec_timesteps"] * 2
    gd.use_hip_graph = False
    undo = patch_randn(randn_like=lambda v, **_: torch.zeros_like(v))
    try:
        eager = call(known=known, known_mask=mask)
    finally:
        undo()
    assert torch.isfinite(captured).all() and rel(captured, eager) < 1e-6


@pytest.mark.parametrize("method,eta", (("ddim", 0.0), ("ddpm", 0.0)))
def test_scale_1_is_the_conditional_loop_and_scale_0_the_unconditional_one(method, eta):
    _, m, kw, un, shape, x0 = guided_setup()
    for s, plain_kw in ((1.0, kw), (0.0, dict(kw, **un))):
        gm = hig_amd.ClassifierFreeGuidedModel(m, s, un)
        sd = spaced()
        sd._debug_zero_noise = True
        guided, n = counting_replays(lambda: run_loop(sd, gm, shape, x0, kw, method, eta))
        assert n == K
        plain = run_loop(sd, m, shape, x0, plain_kw, method, eta)
        e = rel(guided, plain)
        print("LOOP guided s%g vs unguided %s: rel %.3e" % (s, method, e))
        assert e < 1e-5
    assert rel(run_loop(sd, m, shape, x0, kw, method, eta), plain) > 1e-3       # (the two text inputs do give different samples)


def test_one_stacked_forward_is_two_forwards():
    _, m, kw, un, shape, x0 = guided_setup()
    B = shape[0]
    t = torch.tensor([3, 987][:B] * (B // 2 + 1))[:B].to(DEV)
    with torch.no_grad():
        c = m(x0, t, **kw)
        u = m(x0, t, **dict(kw, **un))
        both = m(stack_rows(x0, x0, B), stack_rows(t, t, B), xf_proj=stack_rows(kw["xf_proj"], un["xf_proj"], B),
                 xf_out=stack_rows(kw["xf_out"], un["xf_out"], B), length=stack_rows(kw["length"], kw["length"], B))
    e = max(rel(both[:B], c), rel(both[B:], u))
    print("FORWARD stacked 2B vs two B: rel %.3e" % e)
    assert e < 1e-6
    # and the wrapper's eager call is hig_cfg_combine of exactly that
    gm = hig_amd.ClassifierFreeGuidedModel(m, 2.5, un)
    with torch.no_grad():
        out, launches = spied(lambda: gm(x0, t, **kw))
    assert "hig_cfg_combine" in launches
    eg, e_g = cb.combine_bound(both.cpu().flatten(1), 2.5, B, B)
    held("wrapper on ROCm tensors", out.cpu().flatten(1), eg, e_g)


# ----------------------------------------------------------------------------------------------------------------------
# 4. trainers
# ----------------------------------------------------------------------------------------------------------------------
# Guidance scales eps_c - eps_u, so a test of it needs captions that differ from the empty one.  The stub tokenizer spends one
# token per word: the three-word captions of the other trainer tests differ from "" in 3 of the 77 context rows the text head and
# the cross-attention see, and leave guidance next to nothing to scale.  These occupy about a third of the context, as dataset
# captions do under CLIP's own tokenizer.
LONG = ["a person walks forward slowly then turns around to the left raises both arms above the head waves twice and finally sits "
        "down on a low chair with crossed legs",
        "two people approach each other from opposite sides shake hands firmly step back bow deeply and then one of them hugs the "
        "other while patting the back three times",
        "a person jumps up high lands on the right foot spins clockwise stumbles backwards regains balance stretches the arms out "
        "wide and starts jogging in a small circle"]
LONG1 = ["the first person steps forward raises the right hand and pushes the other person on the left shoulder then quickly "
         "retreats two steps and lifts both hands in apology",
         "the first person bows politely extends the right arm offers a handshake holds it for a moment then turns away and walks "
         "towards the back of the room without looking"]
LONG2 = ["the second person stumbles back after being pushed catches the balance by widening the stance shakes the head and points "
         "a finger at the first person angrily",
         "the second person accepts the handshake nods twice smiles takes one step closer pats the first person on the arm and "
         "waves goodbye while walking to the front"]

def test_trainer_generates_with_guidance():
    c = fill.CASES["tiny"]
    m = build(c).eval()
    tr = _trainer(c, m)
    lens = torch.tensor([16, 12, 9])
    F = c["F"]
    tr.set_sampler(steps=10, method="ddim", guidance_scale=2.5)
    torch.manual_seed(3)
    (outs, launches), n = counting_replays(lambda: spied(lambda: tr.generate(LONG, lens, F, batch_size=2)))
    assert n == 2 * K and "hig_ddim_step_cfg" in launches and "hig_ddim_step" not in launches
    assert [tuple(o.shape) for o in outs] == [(16, F), (16, F), (9, F)] and all(torch.isfinite(o).all() for o in outs)
    tr.set_sampler(steps=10, method="ddim", guidance_scale=None)
    torch.manual_seed(3)
    plain, launches = spied(lambda: tr.generate(LONG, lens, F, batch_size=2))
    assert "hig_ddim_step" in launches and not any(x.endswith("_cfg") for x in launches)
    e = rel(torch.cat([o.flatten() for o in outs]), torch.cat([o.flatten() for o in plain]))
    print("TRAINER guided vs unguided rel %.3e" % e)
    assert e > 1e-3
    # guidance on the full chain, and a known region under guidance
    tr50 = _trainer(dict(c), m)
    tr50.set_sampler(guidance_scale=2.5)
    assert tr50._few_step is None
    known, mask = known_for((3, c["num_frames"], F))
    tr.set_sampler(steps=10, method="ddim", guidance_scale=2.5)
    torch.manual_seed(5)
    got = tr.generate_batch(LONG, lens, F, known=known, known_mask=mask)
    assert got.shape == (3, 16, F) and torch.isfinite(got).all()
    # as the unguided known-region test holds the trainer: bit for bit the loop called directly with the same arguments
    xf_proj, xf_out = m.encode_text(LONG, tr.device)
    up, uo = m.encode_text([""], tr.device)
    gm = hig_amd.ClassifierFreeGuidedModel(m, 2.5, dict(xf_proj=up, xf_out=uo))
    assert gm.group_for(3) == 3                                     # the single-person default: [cond; uncond]
    torch.manual_seed(5)
    want = spaced().ddim_sample_loop(gm, (3, 16, F), clip_denoised=False, eta=0.0,
                                     model_kwargs=dict(xf_proj=xf_proj, xf_out=xf_out, length=lens), known=known[:, :16],
                                     known_mask=mask[:, :16])
    assert torch.equal(got, want)


def test_two_person_trainer_generates_with_guidance():
    c = fill.ICASES["tiny2"]
    m = build_pair(c).eval()
    tr = _mul_trainer(c, m)
    T, Fd = c["T"], c["F"]
    lens = torch.tensor([T, 9])
    tr.set_sampler(steps=10, method="ddim", guidance_scale=2.5)

    def gen(c1, c2):
        torch.manual_seed(8)
        outs = tr.generate(c1, c2, lens, Fd)
        assert len(outs) == 2 and all(len(o) == 2 and o[0].shape == (T, Fd) and o[1].shape == (T, Fd) for o in outs)
        assert all(torch.isfinite(o[0]).all() and torch.isfinite(o[1]).all() for o in outs)
        return outs

    (a, launches), n = counting_replays(lambda: spied(lambda: gen(LONG1, LONG2)))
    assert n == K and "hig_ddim_step_cfg" in launches
    tr.set_sampler(steps=10, method="ddim")
    plain = gen(LONG1, LONG2)
    assert rel(torch.stack([a[0][0], a[0][1]]), torch.stack([plain[0][0], plain[0][1]])) > 1e-3
    # swapping the two captions of pair 0 changes pair 0 only: a person keeps its partner in both branches
    tr.set_sampler(steps=10, method="ddim", guidance_scale=2.5)
    c1, c2 = list(LONG1), list(LONG2)
    c1[0], c2[0] = LONG2[0], LONG1[0]
    b = gen(c1, c2)
    assert torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1], b[1][1])
    assert rel(torch.stack([b[0][0], b[0][1]]), torch.stack([a[0][0], a[0][1]])) > 1e-3
    # a reaction under guidance (person 1 given): bit for bit the loop called directly on the wrapper with group = pairs, as the
    # unguided known-region test holds the trainer
    known = (fill.tensor_for("g19.pair.known", (2, 2, T, Fd)) * 10.0).to(DEV)
    mask = torch.zeros(2, 2, T, Fd, dtype=torch.bool, device=DEV)
    mask[0] = (torch.arange(T, device=DEV)[None, :] < lens.to(DEV)[:, None])[:, :, None]
    known[1] = float("nan")
    torch.manual_seed(6)
    outs = tr.generate(LONG1, LONG2, lens, Fd, known=known, known_mask=mask)
    xf_proj, xf_out = m.encode_text(list(LONG1) + list(LONG2), tr.device)
    up, uo = m.encode_text([""], tr.device)
    gm = hig_amd.ClassifierFreeGuidedModel(m, 2.5, dict(xf_proj=up, xf_out=uo), group=2)
    assert hig_amd.ClassifierFreeGuidedModel(m, 2.5, dict(xf_proj=up, xf_out=uo)).group_for(4) == 2    # the two-person default
    torch.manual_seed(6)
    want = spaced().ddim_sample_loop(gm, (4, T, Fd), clip_denoised=False, eta=0.0,
                                     model_kwargs=dict(xf_proj=xf_proj, xf_out=xf_out, length=torch.cat([lens, lens])),
                                     known=known.flatten(0, 1), known_mask=mask.flatten(0, 1))
    assert torch.isfinite(want).all() and torch.equal(torch.stack([o[0] for o in outs] + [o[1] for o in outs]), want)
    # the same through the eager wrapper: group = pairs there too
    sd = tr._few_step[0]
    sd.use_hip_graph = False
    eager = gen(LONG1, LONG2)
    assert rel(torch.stack([eager[0][0], eager[1][1]]), torch.stack([a[0][0], a[1][1]])) < 1e-5
