"""The contract of the kernels on either side of the denoiser -- hig_pair_mse (csrc/ddpm.hip), hig_recover_joints and
hig_gather_frames (csrc/pipeline.hip), hig_timestep_embedding[_bf16] (csrc/rowops.hip): every output element within a derived
bound of its fp64 value (hig_gather_frames: bit-equal to numpy), every output written, nothing around it touched.

References, bounds, inputs and the shape tables are those of tests/boundary_bounds.py (its docstring carries the derivations;
tests/test_cpu_boundary_bounds.py proves on the CPU that the bounds reject wrong arithmetic).  The entry points are called
directly, under the rules of tests/test_gpu_rowops_contract.py:
  * every output lives in a `Buf`: NaN-pattern filled, guarded above and below, checked to be fully written with the guards
    intact; the scratch of hig_pair_mse is exactly 2 R floats inside guards, its loss one guarded float;
  * pred and target of hig_pair_mse hold NaN wherever the contract says they are never read (tokens t >= clamp(len), features
    >= 4 of token 0): the loss must be finite and within its bound, dpred exactly 0 there and on every row of an unchosen
    assignment;
  * the caption assignment of every PIT pair is read off rowscale in the scratch and must be the reference's: every pair is
    decided by a margin above 4 bounds or a tie by construction, which takes the first.  rowscale itself is 1 / denom rounded
    once, or 0: held bit for bit;
  * dpred = NULL gives the same loss bits and leaves a guarded dummy untouched; two calls give the same bits everywhere;
  * an assertion message reports the largest |error| / bound and where it occurred.

Measured on an MI355X (largest |error| / bound over all cases of the output; every bound is derived, the 4 ulp of sinf / cosf
are OpenCL's full-profile figure, the ratios below are the only measurements):
    output                          bound                                                         ratio  at
    hig_pair_mse.rowloss            sum_t gam(g_tok + ceil(len / 4) + 2) l_t, g_tok = 10 + ceil(nf / 64)   0.181  1028x2x4_pit
    hig_pair_mse.loss               chosen b_row + gam(pit + ceil(n / 256) + 9) sum, / denom      0.052  259x3x5
    hig_pair_mse.dpred              gam(4) |dpred|                                                0.761  8x250x263
    hig_pair_mse.rowscale           fp32(1 / denom) or 0                                          exact  every case
    hig_pair_mse PIT assignment     margin > 4 or a tie by construction                           equal  every pair (smallest margin 2.2e5)
    hig_recover_joints              recover_bound                                                 0.944  r3_T255_J22_F263_initfirst_stats
    hig_recover_joints (T = 4097)   recover_bound; 65552 bytes of LDS: served                     0.114  r1_T4097_J2_F7
    hig_timestep_embedding          u |arg| ((2 + kappa) |e| + 3) + 4 ulp                         0.400  d512
    hig_timestep_embedding_bf16     the same + ulp16 / 2                                          0.999  d512
    hig_gather_frames               numpy, float32 and float64 statistics                         exact  every case
Smallest share of decided elements of hig_timestep_embedding_bf16: 80 % (d2, ten elements), 98 % from d = 64 on; no decided
element was wrong.  The pair-loss reductions sit where the lane-order fp32 emulation on the CPU put them (rowloss 0.04-0.18,
loss 0.003-0.05): a sum of worst cases over a tree is never approached.
Ratios above 0.5, and why.
  * hig_timestep_embedding_bf16 0.999 by construction: the bound is the fp32 bound plus HALF a bf16 ulp, and an element whose
    fp32 value lies next to a rounding boundary is off by that half ulp.  The fp32 entry (0.400) shows the arithmetic's slack.
  * hig_recover_joints 0.944 is a Y coordinate (flat index 50248 = 3 k + 1) of the case with statistics: Y passes through both
    rotations exactly, so its whole error is x sd + mean, two roundings under a bound that counts exactly those two (the fp32
    evaluation on the CPU reaches 0.972 there).  Without statistics Y is exact and the X / Z coordinates stay below 0.26.
  * hig_pair_mse.dpred 0.761 (0.54-0.70 on four smaller cases): four roundings happen (1 / denom, the difference, the product,
    the division) and four are counted; half a million elements come within a quarter of all four falling the same way.
A hand check of the file's teeth, not committed: with `(float)nf` changed to `(float)F` in pair_rowloss_kernel the five cases with
F != 4 fail at rowloss ratios of 2.4e5 to 1.2e6 (the two F = 4 cases cannot see it); with `feat(t - 1, 0)` changed to
`feat(t, 0)` in step 1 of recover_joints_kernel every case with T > 1 fails at 2.1e4 to 1.4e5.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hig_amd import _lib  # noqa: E402
from test_gpu_rowops_contract import Buf, P, S, lib, ok  # noqa: E402
import boundary_bounds as bb  # noqa: E402
from boundary_bounds import BF16  # noqa: E402

DEV = "cuda"


def held(what, out, ref, bound):
    """Every element within its bound; the message carries the largest |error| / bound and its place.  The RATIO lines (shown
    by `pytest -s`) are what the table of the module docstring was collected from."""
    ref, bound = ref.reshape(-1), bound.reshape(-1)
    err = (out.double().reshape(-1) - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    at = int(q.argmax())
    print("RATIO %s %.3f at %d" % (what, q[at], at))
    assert q[at] <= 1.0, "%s: largest |err| / bound = %.3f at flat index %d (got %.9g, fp64 %.9g, bound %.3g)" % (
        what, q[at], at, out.reshape(-1)[at], ref[at], bound[at])


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


# ----------------------------------------------------------------------------------------------------------------------
# hig_pair_mse
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,T,F,pit,with_len", bb.PAIR_SHAPES)
def test_pair_mse(R, T, F, pit, with_len):
    pred, target, length = bb.pair_case(R, T, F, pit, with_len)
    b = bb.pair_bound(pred, target, length, pit)
    pn, tn = bb.pair_poison(pred, target, length)
    pd, tg = pn.to(DEV), tn.to(DEV)
    lnd = None if length is None else length.to(DEV)
    what = "hig_pair_mse %dx%dx%d%s%s" % (R, T, F, "_pit" * pit, "" if with_len else "_nolen")

    def call(want_d):
        lo, scratch, d = Buf.flat(1), Buf.flat(2 * R), Buf.flat(R * T * F)
        ok(lib().hig_pair_mse(P(pd), P(tg), P(lnd), R, T, F, pit, lo.p(), d.p() if want_d else None, scratch.p(), S()))
        loss, sc = lo.written(what + " loss")[0], scratch.written(what + " scratch")[0]
        if not want_d:
            d.untouched(what + " dpred = NULL")
            return loss, sc, None
        return loss, sc, d.written(what + " dpred").view(R, T, F)

    loss, sc, dp = call(True)
    assert torch.isfinite(loss).all(), "%s: the loss is %s: a masked position was read" % (what, loss)
    held(what.replace(" ", ".rowloss ", 1), sc[:R], *b["rowloss"])
    rowscale = sc[R:]
    if pit:
        Pn = R // 4
        first = rowscale[:Pn] != 0
        wrong = (first != b["first"]).nonzero().flatten().tolist()
        assert not wrong, "%s: pairs %s take the other caption assignment (margins %s, ties %s)" % (
            what, wrong[:8], b["margin"][wrong[:8]].tolist(), b["tie"][wrong[:8]].tolist())
        assert first[b["tie"]].all(), "%s: a tie does not take the first assignment" % what
    bad = (bits(rowscale) != bits(b["rowscale32"])).nonzero().flatten().tolist()
    assert not bad, "%s: rowscale of rows %s is not fp32(1 / denom) on the chosen rows and 0 elsewhere" % (what, bad[:8])
    held(what.replace(" ", ".loss ", 1), loss, *b["loss"])
    held(what.replace(" ", ".dpred ", 1), dp, *b["dpred"])
    dead = ~b["live"] | (b["rowscale32"] == 0)[:, None, None]
    assert (dp[dead] == 0).all(), "%s: dpred is not exactly 0 off the mask / on an unchosen row (%d elements)" % (
        what, int((dp[dead] != 0).sum()))
    loss2, sc2, dp2 = call(True)
    assert torch.equal(bits(loss2), bits(loss)) and torch.equal(bits(sc2), bits(sc)) and torch.equal(bits(dp2), bits(dp)), \
        "%s: two calls differ" % what
    loss3, sc3, _ = call(False)
    assert torch.equal(bits(loss3), bits(loss)) and torch.equal(bits(sc3), bits(sc)), "%s: dpred = NULL changes the loss" % what


# ----------------------------------------------------------------------------------------------------------------------
# hig_recover_joints
# ----------------------------------------------------------------------------------------------------------------------
def recover_call(motion, stats, J, init_first):
    rows, T1, F = motion.shape
    md, sd = motion.contiguous().to(DEV), None if stats is None else stats.to(DEV)
    out = Buf.flat(rows * (T1 - 1) * J * 3)
    rc = lib().hig_recover_joints(P(md), P(sd), rows, T1 - 1, F, J, init_first, out.p(), S())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("rows,T,J,F,init_first,with_stats", bb.RECOVER_CASES)
def test_recover_joints(rows, T, J, F, init_first, with_stats):
    motion, stats = bb.recover_case(rows, T, J, F, init_first, with_stats)
    _, bound = bb.recover_bound(motion, stats, J, init_first)
    ref = bb.recover_ref(motion, stats, J, init_first)
    what = "hig_recover_joints r%d_T%d_J%d_F%d%s%s" % (rows, T, J, F, "_initfirst" * init_first, "_stats" * with_stats)
    rc, out = recover_call(motion, stats, J, init_first)
    _lib.check(rc)
    o = out.written(what)
    held(what, o, ref, bound)
    rc, again = recover_call(motion, stats, J, init_first)
    _lib.check(rc)
    assert torch.equal(bits(again.written(what)), bits(o)), "%s: two calls differ" % what


def test_recover_joints_above_64_kib_of_lds():
    """T = 4097: 16 T = 65552 bytes of dynamic LDS, the first size above 64 KiB.  The entry point asks the device for its
    per-workgroup limit before it launches: served, the result is within the bound and the guards are intact; refused, nothing
    was written and a T = 2 call right after succeeds.  (The MI355X this was measured on serves the call.)"""
    rows, T, J, F, init_first, with_stats = bb.RECOVER_LDS_CASE
    motion, stats = bb.recover_case(rows, T, J, F, init_first, with_stats)
    rc, out = recover_call(motion, stats, J, init_first)
    print("LDS T=%d rc=%d" % (T, rc))
    if rc == 0:
        _, bound = bb.recover_bound(motion, stats, J, init_first)
        held("hig_recover_joints r1_T4097_J2_F7", out.written("T = 4097"), bb.recover_ref(motion, stats, J, init_first), bound)
        return
    out.untouched("hig_recover_joints T = 4097")
    case = bb.RECOVER_CASES[1]
    motion, stats = bb.recover_case(*case)
    rc, out = recover_call(motion, stats, case[2], case[4])
    _lib.check(rc)
    held("hig_recover_joints after a refusal", out.written("T = 2"), bb.recover_ref(motion, stats, case[2], case[4]),
         bb.recover_bound(motion, stats, case[2], case[4])[1])


def test_recover_joints_refuses_T_above_8192():
    rows, T, J, F = 1, 8193, 1, 4
    motion = torch.zeros(rows, T + 1, F)
    rc, out = recover_call(motion, None, J, 0)
    assert rc != 0, "T = 8193 was accepted"
    out.untouched("hig_recover_joints T = 8193")


# ----------------------------------------------------------------------------------------------------------------------
# hig_timestep_embedding, hig_timestep_embedding_bf16
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", bb.TEMB_D)
def test_timestep_embedding(d):
    t = bb.temb_case()
    B = len(t)
    ref, bound = bb.temb_bound(t, d)
    td = t.to(DEV)
    out, out16 = Buf.flat(B * d), Buf.flat(B * d, BF16)
    ok(lib().hig_timestep_embedding(P(td), B, d, out.p(), S()))
    ok(lib().hig_timestep_embedding_bf16(P(td), B, d, out16.p(), S()))
    o, o16 = out.written("hig_timestep_embedding").view(B, d), out16.written("hig_timestep_embedding_bf16").view(B, d)
    held("hig_timestep_embedding d%d" % d, o, ref, bound)
    if d % 2:
        assert (o[:, -1] == 0).all() and (o16[:, -1] == 0).all(), "d = %d: the last column is not exactly 0" % d
    held("hig_timestep_embedding_bf16 d%d" % d, o16, ref, bb.bound16(ref, bound))
    frac, wrong = bb.exact16(o16, ref, bound)
    print("DECIDED hig_timestep_embedding_bf16 d%d %.3f" % (d, frac))
    assert wrong == 0, "hig_timestep_embedding_bf16 d%d: %d decided elements are not bf16(ref)" % (d, wrong)
    assert torch.equal(bits(o16), bits(o.to(BF16))), "the bf16 entry is not the fp32 entry rounded once"
    ok(lib().hig_timestep_embedding(P(td), B, d, out.p(), S()))
    assert torch.equal(bits(out.written("hig_timestep_embedding").view(B, d)), bits(o)), "two calls differ"


# ----------------------------------------------------------------------------------------------------------------------
# hig_gather_frames: bit-equal to numpy
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", (False, True))
@pytest.mark.parametrize("rows,T,F", bb.GATHER_CASES)
def test_gather_frames(rows, T, F, f64):
    bank, seq_off, frame_ix, stats = bb.gather_case(rows, T, F)
    want = torch.from_numpy(bb.gather_eval(bank, seq_off, frame_ix, stats, f64))
    bd, sod, ixd = (torch.from_numpy(a).to(DEV) for a in (bank, seq_off, frame_ix))
    std = torch.from_numpy(stats.astype(np.float64 if f64 else np.float32)).to(DEV)
    what = "hig_gather_frames r%d_T%d_F%d_%s" % (rows, T, F, "f64" if f64 else "f32")
    got = []
    for _ in range(2):
        out = Buf.flat(rows * T * F)
        ok(lib().hig_gather_frames(P(bd), P(sod), P(ixd), P(std), int(f64), rows, T, F, out.p(), S()))
        got.append(out.written(what).view(rows, T, F))
    diff = (bits(got[0]) != bits(want)).nonzero()
    assert diff.numel() == 0, "%s: %d elements differ from numpy, the first at %s (got %.9g, numpy %.9g)" % (
        what, diff.shape[0], diff[0].tolist(), got[0][tuple(diff[0])], want[tuple(diff[0])])
    assert torch.equal(bits(got[1]), bits(got[0])), "%s: two calls differ" % what
