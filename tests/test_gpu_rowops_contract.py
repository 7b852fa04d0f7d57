"""The contract of the row-wise and elementwise kernels (csrc/rowops.hip, csrc/rowops_bf16.hip, csrc/ddpm.hip): every output
element within a derived bound of its fp64 value, every output written, nothing around it touched.

References, bounds, summation depths, inputs and the shape tables are those of tests/rowops_bounds.py (its docstring
carries the derivations; tests/test_cpu_rowops_bounds.py proves on the CPU that the bounds reject wrong arithmetic).  Here
every call obeys the same rules:
  * every output lives in a `Buf` (the `Guarded` of the GEMM contract): NaN-pattern filled, a guard row above and below, and
    guard columns because every leading dimension is larger than the row -- a different padding per operand (da n + 4, x n + 8,
    dx n + 12, res n + 16; twice that for the entry points that need multiples of 8), so a swapped leading dimension shows;
  * the padding of every INPUT holds NaN: a kernel that reads beyond a row poisons its result;
  * ss is 6 n wide with scale at 2 n and shift at 3 n, as the model lays it out; dss_ld = 2 n + 4;
  * scratch and `partial` buffers have exactly the documented size, inside guards;
  * all pointers keep the alignment the entry point documents;
  * the assertion message reports the largest error / bound ratio.
The instance a shape reaches is fixed by the shape rules quoted next to the tables of tests/rowops_bounds.py.

Measured on an MI355X (largest |error| / bound over all cases of the entry point; gamma and h as derived in
tests/rowops_bounds.py -- every gamma is derived, the 1-ulp v_rsq / v_rcp / v_exp figures are the ISA manual's, the ratios below
are the only measurements):
    output                         gamma / h                                                      ratio  at
    hig_clip_adam*.gnorm           (h + 3) / 2 + 1, h = 2 + trips + 1 + 6 + 2 + 4 + 8             0.089  hig_clip_adam_shadow n3_step0
    hig_clip_adam*.m               clip_adam_bound                                                0.499  hig_clip_adam_shadow n4194307_step2
    hig_clip_adam*.p               clip_adam_bound                                                0.999  hig_clip_adam_shadow n4194307_step1
    hig_clip_adam*.v               clip_adam_bound                                                0.500  hig_clip_adam_shadow n4194307_step1
    hig_colsum                     h = ceil(rows / (4 chunks)) + 3 + colreduce(chunks)            0.063  r15_n1536
    hig_colsum_bf16                the same h                                                     0.021  r8229_n1536
    hig_gelu_bf16                  one bf16 ulp (include/hig.h)                                   0.538  n560008
    hig_layernorm                  ln_fwd_bound: d_mu, rho + 3, 1 + 1                             0.197  n4_r7_ordinary
    hig_layernorm.mean             n + 1                                                          0.200  n4_r7_const
    hig_layernorm.rstd             rho                                                            0.135  n4_r7_ordinary
    hig_ln_bf16                    ln_fwd_bound, silu G = 4, + ulp16 / 2                          1.000  n64_r32771_rps4099_ordinary_x16_sty
    hig_ln_bwd.dbeta               the same h                                                     0.173  n1024_1x1_ordinary_sty_dg_db_res
    hig_ln_bwd.dgamma              h = trips + 3 + colreduce(samples splits)                      0.165  n1024_1x1_ordinary_sty_dg_db_res
    hig_ln_bwd.dscale              h = trips + 3 + splits                                         0.263  n1024_1x1_ordinary_sty
    hig_ln_bwd.dshift              the same h                                                     0.160  n64_600x9_const_sty
    hig_ln_bwd.dx                  ln_bwd_bound, e_xh = 3 u |xhat|, H = n                         0.190  n64_600x9_const_plain_dg_res
    hig_ln_bwd_bf16.dbeta          the same h                                                     0.077  n264_2x1_ordinary_sty
    hig_ln_bwd_bf16.dgamma         h = trips + (waves - 1) + colreduce(samples splits)            0.084  n64_2x1_const_plain32
    hig_ln_bwd_bf16.dscale         h = trips + (waves - 1) + splits                               0.108  n1024_2x1_ordinary_sty_bare
    hig_ln_bwd_bf16.dshift         the same h                                                     0.127  n1024_600x17_ordinary_sty_bare
    hig_ln_bwd_bf16.dx (bf16 dx)   the same + ulp16 / 2                                           1.000  n1024_600x17_ordinary_plain16
    hig_ln_bwd_bf16.dx (fp32 dx)   ln_bwd_bound, forward e_xh, H = 2 NIT + 7                      0.210  n264_64x65_const_plain32
    hig_ln_mod_silu                ln_fwd_bound, silu G = 3                                       0.320  n768_r7_const
    hig_ln_mod_silu.mean           n + 1                                                          0.200  n4_r7_const
    hig_ln_mod_silu.rstd           rho                                                            0.135  n4_r7_ordinary
    hig_masked_mse.dpred           4                                                              0.594  3x20x150
    hig_masked_mse.loss            F + 5 + h, h = trips + 2 + ceil(blocks / 256) + 8              0.035  33x130x5
    hig_p_sample_step.pred_xstart  2                                                              0.944  3 x 180001
    hig_p_sample_step.x_prev       p_step_bound                                                   0.882  3 x 180001
    hig_q_sample                   2                                                              0.982  3 x 180001
    hig_rowstats.mean              n + 1 (d_mu)                                                   0.200  n4_r7_const
    hig_rowstats.rstd              rho: d_mu D1 / (var + eps) + (n + 5) / 2 + 2                   0.135  n4_r7_ordinary
    hig_transpose.ln               3 on the product, 1 on the sum                                 0.951  130x63
Smallest share of decided elements on ordinary rows: hig_ln_bf16 78 % (n1024_r50_rps7_ordinary_x32_sty), hig_ln_bwd_bf16.dx 94 % (n1024_2x196_ordinary_sty_bare).
Ratios above 0.5, and why.  None of them is a reduction: each belongs to a bound of one to four roundings, which a few
hundred thousand elements come close to exhausting, so there is no slack to expect.
  * the bf16 outputs (hig_ln_bf16, the bf16 dx of hig_ln_bwd_bf16) reach 1.000 by construction: the bound is the fp32 bound plus
    HALF a bf16 ulp, and an element whose fp32 value lies next to a rounding boundary is off by that half ulp.  The fp32 dx of
    the same kernel (0.210) shows the slack of the arithmetic itself; the exactness check found no decided element wrong.
  * hig_clip_adam*.p 0.999, .v 0.500, .m 0.499: p' = p - step with |step| ~ 1e-4 |p|, so the error IS the rounding of that one
    difference and the bound is u |p'| plus a few per cent; m' and v' are two roundings under a bound that counts about four.
  * hig_q_sample 0.982, pred_xstart 0.944, x_prev 0.882, hig_transpose.ln 0.951: three or four roundings under a bound that
    counts exactly those (2 u M covers two products and the sum).
  * hig_masked_mse.dpred 0.594: three roundings happen, four are counted.  hig_gelu_bf16 0.538: a correctly rounded result
    uses half of the one-ulp bound that include/hig.h states, the polynomial fit the rest.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from hig_amd import _lib  # noqa: E402
from test_gpu_gemm_contract import Guarded  # noqa: E402
import rowops_bounds as rb  # noqa: E402
from rowops_bounds import BF16, F32  # noqa: E402

DEV = "cuda"
NAN = float("nan")


def lib():
    return _lib.lib()


def S():
    return _lib.stream_ptr()


def up8(v):
    return (v + 7) // 8 * 8


class Buf(Guarded):
    """Guarded(rows, cols, ld, dtype) with a what-aware verify, a guards-only check for scratch, and `flat` buffers (one guarded
    row)."""

    def __init__(self, rows, cols, ld, dtype=F32):      # (Guarded has no default dtype; most buffers here are fp32)
        super().__init__(rows, cols, ld, dtype)

    @classmethod
    def flat(cls, size, dtype=F32):
        return cls(1, size, up8(size) + 8, dtype)      # (the run starts 16-byte aligned for fp32 and bf16)

    def p(self, off=0):
        return C.c_void_p(self.out.data_ptr() + off * self.out.element_size())

    def guards(self, what):
        b = self.buf.view(self.I + 2, self.ldc)
        keep = torch.ones_like(b, dtype=torch.bool)
        keep[1:self.I + 1, :self.J] = False
        assert (b[keep] == self.pat).all(), "%s: a store landed in the guard band" % what

    def written(self, what):
        self.guards(what)
        assert not torch.isnan(self.out.float()).any(), "%s: not every element was written" % what
        return self.out.cpu()

    def untouched(self, what):
        assert (self.buf == self.pat).all(), "%s: a refused call wrote" % what


def dev(t, ld=None):
    """The host matrix t on the device inside rows of `ld` elements whose padding is NaN (None: dense)."""
    if t is None:
        return None
    if ld is None or t.dim() != 2:
        return t.contiguous().to(DEV)
    buf = torch.full((t.shape[0], ld), NAN, dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


def P(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


def ok(rc):
    _lib.check(rc)
    torch.cuda.synchronize()


def refused(rc, bufs, what):
    torch.cuda.synchronize()
    assert rc != 0, "%s: accepted" % what
    for b in bufs:
        b.untouched(what)


def held(what, out, ref, bound):
    """Every element within its bound.  The RATIO / DECIDED lines (shown by `pytest -s`) are what the table of the module
    docstring was collected from: the largest value per entry point."""
    r = rb.ratio(out, ref, bound)
    print("RATIO %s %.3f" % (what, r))
    assert r <= 1.0, "%s: largest |err| / bound = %.3f" % (what, r)


def held16(what, out, ref, b32, need_decided=True):
    """A bf16 output: the per-element bound, and bit-exactness of every element the fp32 bound decides."""
    held(what, out, ref, rb.bound16(ref, b32))
    frac, wrong = rb.exact16(out, ref, b32)
    print("DECIDED %s %.3f" % (what, frac))
    assert wrong == 0, "%s: %d decided elements are not bf16(ref)" % (what, wrong)
    assert not need_decided or frac >= rb.MIN_DECIDED, "%s: only %.0f %% of the elements are decided" % (what, 100 * frac)


def ss_args(ss, n):
    """(pointer to the scale columns, ss_ld, shift offset) of a (samples, 6 n) modulation table."""
    return P(ss, 2 * n), 6 * n, n


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm forward, fp32
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rb.KINDS)
@pytest.mark.parametrize("rows", rb.LN32_ROWS)
@pytest.mark.parametrize("n", rb.LN32_N)
def test_ln_forward_fp32(n, rows, kind):
    """hig_rowstats, hig_layernorm, hig_ln_mod_silu: NIT 1 / 2 / 4, dead and partly live slices, idle waves, a short sample."""
    rps = rb.LN32_RPS
    x, gamma, beta, ss = rb.ln_case(kind, rows, n, rps, seed=n + rows)
    xd, gd, bd, ssd = dev(x, n + 8), dev(gamma), dev(beta), dev(ss)
    plain, mod = rb.ln_fwd_bound(x, gamma, beta, None), rb.ln_fwd_bound(x, gamma, beta, ss, rps)
    tag = "n%d_r%d_%s" % (n, rows, kind)

    def stats_held(name, st):
        st = st.written(name).view(rows, 2)
        held(name + ".mean " + tag, st[:, 0], *plain["mean"])
        held(name + ".rstd " + tag, st[:, 1], *plain["rstd"])

    st = Buf.flat(2 * rows)
    ok(lib().hig_rowstats(P(xd), n + 8, rows, n, st.p(), S()))
    stats_held("hig_rowstats", st)
    y, st = Buf(rows, n, n + 12), Buf.flat(2 * rows)
    ok(lib().hig_layernorm(P(xd), n + 8, rows, n, P(gd), P(bd), y.p(), n + 12, st.p(), S()))
    stats_held("hig_layernorm", st)
    held("hig_layernorm " + tag, y.written("hig_layernorm"), *plain["out"])
    a, st = Buf(rows, n, n + 4), Buf.flat(2 * rows)
    sp, sld, soff = ss_args(ssd, n)
    ok(lib().hig_ln_mod_silu(P(xd), n + 8, rows, n, P(gd), P(bd), sp, sld, soff, rps, a.p(), n + 4, st.p(), S()))
    stats_held("hig_ln_mod_silu", st)
    held("hig_ln_mod_silu " + tag, a.written("hig_ln_mod_silu"), *mod["out"])


@pytest.mark.parametrize("kind", rb.KINDS)
@pytest.mark.parametrize("how", ("n150", "ldx153", "base_plus_one_float"))
def test_rowstats_scalar_fallback(how, kind):
    """The three ways out of the float4 path: n % 4, ldx % 4, a base pointer that is not 16-byte aligned."""
    n, ldx, off = {"n150": (150, 156, 0), "ldx153": (152, 153, 0), "base_plus_one_float": (152, 160, 1)}[how]
    rows = 7
    x = rb.rows_input(kind, rows, n, rb.gen(n + ldx))
    buf = torch.full((rows * ldx + off,), NAN, device=DEV)
    buf[off:].view(rows, ldx)[:, :n] = x.to(DEV)
    b = rb.ln_fwd_bound(x, torch.ones(n), torch.zeros(n))
    st = Buf.flat(2 * rows)
    ok(lib().hig_rowstats(P(buf, off), ldx, rows, n, st.p(), S()))
    o = st.written("hig_rowstats").view(rows, 2)
    held("hig_rowstats.mean %s_%s" % (how, kind), o[:, 0], *b["mean"])
    held("hig_rowstats.rstd %s_%s" % (how, kind), o[:, 1], *b["rstd"])


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm forward, bf16 output
# ----------------------------------------------------------------------------------------------------------------------
def ln16_cases():
    for n in rb.LN16_N:
        yield (n,) + rb.LN16_SMALL
    for rows, rps in rb.LN16_BIG:
        yield 64, rows, rps


@pytest.mark.parametrize("kind", rb.KINDS)
@pytest.mark.parametrize("n,rows,rps", list(ln16_cases()))
def test_ln_forward_bf16(n, rows, rps, kind):
    """hig_ln_bf16: NIT 1 / 2, fp32 and bf16 rows, with and without ss; one and four rows per wave."""
    for x_bf16 in (False, True):
        x, gamma, beta, ss = rb.ln_case(kind, rows, n, rps, seed=n + rows + rps, x_bf16=x_bf16)
        ldx = n + 16
        xd, gd, bd, ssd = dev(x, ldx), dev(gamma), dev(beta), dev(ss)
        for mod in (None, ss):
            ref, b32 = rb.ln_fwd_bound(x, gamma, beta, mod, rps, fast_silu=True)["out"]
            out = Buf(rows, n, n + 8, BF16)
            sp, sld, soff = ss_args(ssd, n) if mod is not None else (None, 0, 0)
            ok(lib().hig_ln_bf16(P(xd), int(not x_bf16), ldx, rows, n, P(gd), P(bd), sp, sld, soff, rps, out.p(), n + 8, S()))
            what = "hig_ln_bf16 n%d_r%d_rps%d_%s_x%s_%s" % (n, rows, rps, kind, "16" if x_bf16 else "32", "sty" if mod is not None else "plain")
            held16(what, out.written(what), ref, b32, need_decided=kind == "ordinary")


def test_ln_bf16_refuses_more_than_65535_samples():
    rows, n = 65536, 8
    x, out = torch.zeros(rows, n, device=DEV), Buf(rows, n, n + 8, BF16)
    gamma = torch.ones(n, device=DEV)
    ss = torch.zeros(8, device=DEV)
    refused(lib().hig_ln_bf16(P(x), 1, n, rows, n, P(gamma), P(gamma), P(ss), 0, 0, 1, out.p(), n + 8, S()), [out], "65536 samples")


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ----------------------------------------------------------------------------------------------------------------------
# (form, dgamma, dbeta, res): the five reductions of hig_ln_bwd -- the fused reduce, colreduce with both gradients, with one,
# with the other, dss alone
LNB32_VARIANTS = (("sty", True, True, True), ("plain", True, True, False), ("plain", True, False, True),
                  ("plain", False, True, False), ("sty", False, False, False))


@pytest.mark.parametrize("kind", rb.KINDS)
@pytest.mark.parametrize("n,samples,rps", list(rb.lnb32_cases()))
def test_ln_backward_fp32(n, samples, rps, kind):
    da, x, stats, gamma, beta, ss, res = rb.lnb_case(kind, samples, rps, n, seed=n + samples)
    rows = samples * rps
    dad, xd, rd = dev(da, n + 4), dev(x, n + 8), dev(res, n + 16)
    std, gd, bd, ssd = dev(stats), dev(gamma), dev(beta), dev(ss)
    sp, sld, soff = ss_args(ssd, n)
    nfl = lib().hig_ln_bwd_partial_floats(rows, n, rps)
    assert nfl == samples * rb.splits_for(samples) * 4 * n
    bounds = {}
    for form, want_dg, want_db, with_res in LNB32_VARIANTS:
        mod = form == "sty"
        key = (mod, with_res)
        if key not in bounds:
            bounds[key] = rb.ln_bwd_bound(da, x, stats, gamma, beta, ss if mod else None, res if with_res else None, rps)
        b = bounds[key]
        dx, partial = Buf(rows, n, n + 12), Buf.flat(nfl)
        dg, db = Buf.flat(n) if want_dg else None, Buf.flat(n) if want_db else None
        dss = Buf(samples, 2 * n, 2 * n + 4) if mod else None
        ok(lib().hig_ln_bwd(P(dad), n + 4, P(xd), n + 8, P(std), P(gd), P(bd), sp if mod else None, sld, soff, int(mod),
                            P(rd) if with_res else None, n + 16, dx.p(), n + 12, rows, n, rps, dg.p() if dg else None,
                            db.p() if db else None, dss.p() if dss else None, 2 * n + 4, partial.p(), S()))
        what = "hig_ln_bwd n%d_%dx%d_%s_%s%s%s%s" % (n, samples, rps, kind, form, "_dg" * want_dg, "_db" * want_db, "_res" * with_res)
        partial.guards(what + " partial")
        held(what.replace(" ", ".dx ", 1), dx.written(what), *b["dx"])
        if dg:
            held(what.replace(" ", ".dgamma ", 1), dg.written(what)[0], *b["dgamma"])
        if db:
            held(what.replace(" ", ".dbeta ", 1), db.written(what)[0], *b["dbeta"])
        if dss:
            o = dss.written(what)
            held(what.replace(" ", ".dscale ", 1), o[:, :n], *b["dscale"])
            held(what.replace(" ", ".dshift ", 1), o[:, n:], *b["dshift"])


# (form, x fp32, dx fp32): the four built type forms of hig_ln_bwd_bf16
LNB16_FORMS = (("sty", 0, 0), ("plain16", 0, 0), ("plain32", 1, 1), ("mixed", 0, 1))


@pytest.mark.parametrize("kind", rb.KINDS)
@pytest.mark.parametrize("n,samples,rps", list(rb.lnb16_cases()))
def test_ln_backward_bf16(n, samples, rps, kind):
    """8 waves x 2 rows per trip (n <= 512) and 4 x 1; every call once with `res` and both gradients, and the stylization and
    the bf16 plain form once more with res NULL (the zero-byte descriptor) and dgamma = dbeta = NULL."""
    da, x, _, gamma, beta, ss, res = rb.lnb_case(kind, samples, rps, n, seed=n + samples, bf16=True)
    rows = samples * rps
    gd, bd, ssd = dev(gamma), dev(beta), dev(ss)
    sp, sld, soff = ss_args(ssd, n)
    dad = dev(da, n + 4)
    nfl = lib().hig_ln_bwd_partial_floats(rows, n, rps)
    for form, x_f32, dx_f32 in LNB16_FORMS:
        mod = form == "sty"
        xs = x if x_f32 else x.to(BF16)
        rs = res if dx_f32 else res.to(BF16)
        xd, rd = dev(xs, n + 8), dev(rs, n + 16)
        for bare in (False, True):
            if bare and form not in ("sty", "plain16"):
                continue
            b = rb.ln_bwd_bound(da, xs, None, gamma, beta, ss if mod else None, None if bare else rs, rps, bf16=True)
            dx, partial = Buf(rows, n, n + 12, F32 if dx_f32 else BF16), Buf.flat(nfl)
            dg, db = (None, None) if bare else (Buf.flat(n), Buf.flat(n))
            dss = Buf(samples, 2 * n, 2 * n + 4) if mod else None
            ok(lib().hig_ln_bwd_bf16(P(dad), n + 4, P(xd), x_f32, n + 8, P(gd), P(bd), sp if mod else None, sld, soff, int(mod),
                                     None if bare else P(rd), n + 16, dx.p(), dx_f32, n + 12, rows, n, rps, dg.p() if dg else None,
                                     db.p() if db else None, dss.p() if dss else None, 2 * n + 4, partial.p(), S()))
            what = "hig_ln_bwd_bf16 n%d_%dx%d_%s_%s%s" % (n, samples, rps, kind, form, "_bare" * bare)
            partial.guards(what + " partial")
            if dx_f32:
                held(what.replace(" ", ".dx ", 1), dx.written(what), *b["dx"])
            else:
                held16(what.replace(" ", ".dx ", 1), dx.written(what), *b["dx"], need_decided=kind == "ordinary")
            if dg:
                held(what.replace(" ", ".dgamma ", 1), dg.written(what)[0], *b["dgamma"])
                held(what.replace(" ", ".dbeta ", 1), db.written(what)[0], *b["dbeta"])
            if dss:
                o = dss.written(what)
                held(what.replace(" ", ".dscale ", 1), o[:, :n], *b["dscale"])
                held(what.replace(" ", ".dshift ", 1), o[:, n:], *b["dshift"])


# ----------------------------------------------------------------------------------------------------------------------
# column sums
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", rb.COLSUM_ROWS)
def test_colsum(rows):
    """1, 1, 3 and 512 chunks; fp32 widths include the scalar fallback (n = 3, 150)."""
    for bf16, widths in ((False, rb.COLSUM32_N), (True, rb.COLSUM16_N)):
        for n in widths:
            x = rb.rows_input("ordinary", rows, n, rb.gen(rows + n))
            x = x.to(BF16) if bf16 else x
            ldx = n + 16 if bf16 else (n + 8 if n % 4 == 0 else n + 3)
            ref, bound = rb.colsum_bound(x)
            out, partial = Buf.flat(n), Buf.flat(lib().hig_colsum_chunks(rows) * n)
            assert lib().hig_colsum_chunks(rows) == rb.colsum_chunks(rows)
            fn = lib().hig_colsum_bf16 if bf16 else lib().hig_colsum
            what = "%s r%d_n%d" % ("hig_colsum_bf16" if bf16 else "hig_colsum", rows, n)
            xd = dev(x, ldx)
            ok(fn(P(xd), ldx, rows, n, out.p(), partial.p(), S()))
            partial.written(what + " partial")
            held(what, out.written(what)[0], ref, bound)


# ----------------------------------------------------------------------------------------------------------------------
# transposes, gather / scatter, casts: exact
# ----------------------------------------------------------------------------------------------------------------------
EXTENTS = rb.EXTENTS


@pytest.mark.parametrize("rows", EXTENTS)
def test_transpose_fp32(rows):
    """hig_transpose plain (bit-equal) and with LayerNorm ((v - mean) rstd gamma + beta from the given stats: 3 roundings of
    the product, one of the sum), hig_transpose_batch (dense)."""
    g = rb.gen(rows)
    srcs, dsts = [], []
    for cols in EXTENTS:
        x, stats, gamma, beta = rb.transpose_ln_case(rows, cols, g)
        xd = dev(x, cols + 8)
        out = Buf(cols, rows, rows + 4)
        ok(lib().hig_transpose(P(xd), cols + 8, rows, cols, out.p(), rows + 4, None, None, None, S()))
        assert torch.equal(out.written("hig_transpose"), x.t()), "hig_transpose %dx%d" % (rows, cols)
        out = Buf(cols, rows, rows + 4)
        std, gd, bd = dev(stats), dev(gamma), dev(beta)
        ok(lib().hig_transpose(P(xd), cols + 8, rows, cols, out.p(), rows + 4, P(std), P(gd), P(bd), S()))
        held("hig_transpose.ln %dx%d" % (rows, cols), out.written("hig_transpose LN"), *rb.transpose_ln_bound(x, stats, gamma, beta))
        srcs.append(x.contiguous().to(DEV))
        dsts.append(Buf(cols, rows, rows))
    m = len(srcs)
    ok(lib().hig_transpose_batch(m, (C.c_void_p * m)(*[s.data_ptr() for s in srcs]), (C.c_void_p * m)(*[d.out.data_ptr() for d in dsts]),
                                 (C.c_int32 * m)(*[rows] * m), (C.c_int32 * m)(*EXTENTS), S()))
    for s, d in zip(srcs, dsts):
        assert torch.equal(d.written("hig_transpose_batch"), s.cpu().t()), "hig_transpose_batch %s" % (tuple(s.shape),)


@pytest.mark.parametrize("rows", EXTENTS)
def test_transpose_bf16(rows):
    """hig_transpose_bf16 and its batch form: bit-equal, zeros in [rows, round_up(rows, 8)), the guard starts behind them.  The
    entry points need cols % 8 == 0: the column extents are the multiples of 8 next to 1, 63 / 64, 65 and 130."""
    g = rb.gen(rows)
    r8 = (rows + 7) // 8 * 8
    cols_all = (8, 64, 72, 136)
    xs = [torch.randn(rows, c, generator=g).to(BF16) for c in cols_all]
    xds = [dev(x, c + 16) for x, c in zip(xs, cols_all)]

    def expect(x):
        e = torch.zeros(x.shape[1], r8, dtype=BF16)
        e[:, :rows] = x.t()
        return e

    for x, xd, cols in zip(xs, xds, cols_all):
        out = Buf(cols, r8, r8 + 8, BF16)
        ok(lib().hig_transpose_bf16(P(xd), cols + 16, rows, cols, out.p(), r8 + 8, S()))
        assert torch.equal(out.written("hig_transpose_bf16"), expect(x)), "hig_transpose_bf16 %dx%d" % (rows, cols)
    m = len(xs)
    outs = [Buf(c, r8, r8 + 8, BF16) for c in cols_all]
    ok(lib().hig_transpose_bf16_batch(m, (C.c_void_p * m)(*[x.data_ptr() for x in xds]), (C.c_int64 * m)(*[c + 16 for c in cols_all]),
                                      (C.c_void_p * m)(*[o.out.data_ptr() for o in outs]), (C.c_int64 * m)(*[r8 + 8] * m),
                                      (C.c_int32 * m)(*[rows] * m), (C.c_int32 * m)(*cols_all), S()))
    for x, o in zip(xs, outs):
        assert torch.equal(o.written("hig_transpose_bf16_batch"), expect(x)), "hig_transpose_bf16_batch %s" % (tuple(x.shape),)


@pytest.mark.parametrize("n", (5, 260))
def test_gather_and_scatter_add_rows(n):
    """idx at 0 and at rps - 1 (and between); the gather is bit-equal, the scatter one fp32 add, every other row keeps its bits."""
    B, rps = 3, 4
    g = rb.gen(n)
    src = torch.randn(B * rps, n, generator=g)
    idx = torch.tensor([0, rps - 1, 2], dtype=torch.int64)
    rows = torch.arange(B) * rps + idx
    out = Buf(B, n, n + 3)
    srcd, idxd = dev(src, n + 5), idx.to(DEV)
    ok(lib().hig_gather_rows(P(srcd), n + 5, B, rps, P(idxd), n, out.p(), n + 3, S()))
    assert torch.equal(out.written("hig_gather_rows"), src[rows])
    add = torch.randn(B, n, generator=g)
    dst = Buf(B * rps, n, n + 3)
    dst.out.copy_(src.to(DEV))
    addd = dev(add, n + 5)
    ok(lib().hig_scatter_add_rows(P(addd), n + 5, B, rps, P(idxd), n, dst.p(), n + 3, S()))
    want = src.clone()
    want[rows] += add
    assert torch.equal(dst.written("hig_scatter_add_rows"), want)


@pytest.mark.parametrize("n", (8, 8 * 70001))
def test_casts_and_gelu(n):
    g = rb.gen(n)
    x = torch.randn(n, generator=g) * 3
    x[:8] = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.0e38, -1.5 * 2.0 ** -126, 6.5, -6.5])   # ties, the range's ends
    o16 = Buf.flat(n, BF16)
    xd = x.to(DEV)
    ok(lib().hig_cast_bf16(P(xd), o16.p(), n, S()))
    assert torch.equal(o16.written("hig_cast_bf16")[0].view(torch.int16), x.to(BF16).view(torch.int16)), "hig_cast_bf16 is not round-to-nearest-even"
    x16 = x.to(BF16)
    o32 = Buf.flat(n)
    x16d = x16.to(DEV)
    ok(lib().hig_cast_f32(P(x16d), o32.p(), n, S()))
    assert torch.equal(o32.written("hig_cast_f32")[0].view(torch.int32), x16.float().view(torch.int32))
    z = x16.float().clamp(-6.5, 6.5).to(BF16)        # (beyond 6.5 the fit is clamped: include/hig.h states that tail apart)
    og = Buf.flat(n, BF16)
    zd = z.to(DEV)
    ok(lib().hig_gelu_bf16(P(zd), og.p(), n, S()))
    ref = rb.gelu_eval(z)
    held("hig_gelu_bf16 n%d" % n, og.written("hig_gelu_bf16")[0], ref, rb.ulp16(ref) + 2.0 ** -126)
    rows, cols = (1, 5) if n == 8 else (7001, 77)       # 7001 x 80 / 8 = 70010 threads
    src = torch.randn(rows, cols, generator=g)
    ld = (cols + 7) // 8 * 8
    op = Buf(rows, ld, ld, BF16)        # (the padding columns are output: zeros)
    srcd = dev(src, cols + 3)
    ok(lib().hig_cast_pad_bf16(P(srcd), cols + 3, rows, cols, op.p(), ld, S()))
    want = torch.zeros(rows, ld, dtype=BF16)
    want[:, :cols] = src.to(BF16)
    assert torch.equal(op.written("hig_cast_pad_bf16").view(torch.int16), want.view(torch.int16))


# ----------------------------------------------------------------------------------------------------------------------
# DDPM steps
# ----------------------------------------------------------------------------------------------------------------------
def test_q_sample_and_p_sample_step():
    """540003 elements: a second trip of the grid-stride loop (2048 x 256 threads) and sample boundaries inside a workgroup.
    t = 0 must add no noise.  In place (x_prev == x) and with pred_xstart NULL."""
    B, per, nsteps = rb.DDPM_SHAPE
    x, eps, z, t, tab = rb.ddpm_case()
    xd, ed, zd, td, tabd = (v.contiguous().to(DEV) for v in (x, eps, z, t, tab))
    out = Buf.flat(B * per)
    ok(lib().hig_q_sample(P(xd), P(ed), P(td), P(tabd), nsteps, B, per, out.p(), S()))
    held("hig_q_sample", out.written("hig_q_sample").view(B, per), *rb.q_sample_bound(x, eps, t, tab))
    (xp, b), (x0, b0) = rb.p_step_bound(x, eps, z, t, tab)
    o1, o0 = Buf.flat(B * per), Buf.flat(B * per)
    ok(lib().hig_p_sample_step(P(xd), P(ed), P(zd), P(td), P(tabd), nsteps, B, per, o1.p(), o0.p(), S()))
    held("hig_p_sample_step.x_prev", o1.written("x_prev").view(B, per), xp, b)
    held("hig_p_sample_step.pred_xstart", o0.written("pred_xstart").view(B, per), x0, b0)
    inplace = Buf.flat(B * per)
    inplace.out.copy_(xd.view(1, -1))
    ok(lib().hig_p_sample_step(inplace.p(), P(ed), P(zd), P(td), P(tabd), nsteps, B, per, inplace.p(), None, S()))
    assert torch.equal(inplace.written("in place"), o1.out.cpu()), "the in-place step differs from the out-of-place one"


@pytest.mark.parametrize("B", (1, 257))
def test_dec_timesteps(B):
    t = torch.arange(B, dtype=torch.int64) * 3 - 1
    buf = Buf.flat(2 * B, F32)      # (B int64 values in a guarded run of 8 B bytes)
    buf.out.view(torch.int64).copy_(t.to(DEV).view(1, -1))
    ok(lib().hig_dec_timesteps(buf.p(), B, S()))
    buf.guards("hig_dec_timesteps")
    assert torch.equal(buf.out.view(torch.int64).cpu()[0], t - 1)


# ----------------------------------------------------------------------------------------------------------------------
# masked loss
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,F", rb.MSE_SHAPES)
def test_masked_mse(B, T, F):
    """lengths 0, 1, T, T + 5, -2, ..; length NULL; dpred NULL; scratch of exactly HIG_NORM_BLOCKS floats."""
    pred, target, length = rb.mse_case(B, T, F, seed=B)
    pd, tg = pred.to(DEV), target.to(DEV)
    for ln, want_d in ((length, True), (None, True), (length, False)):
        (loss, bl), (dp, bd) = rb.masked_mse_bound(pred, target, ln)
        lo, scratch = Buf.flat(1), Buf.flat(_lib.NORM_BLOCKS)
        d = Buf.flat(B * T * F) if want_d else None
        lnd = None if ln is None else ln.to(DEV)
        ok(lib().hig_masked_mse(P(pd), P(tg), P(lnd), B, T, F, lo.p(), d.p() if d else None, scratch.p(), S()))
        what = "hig_masked_mse %dx%dx%d%s" % (B, T, F, "" if ln is not None else "_nolen")
        scratch.guards(what + " scratch")
        held(what.replace(" ", ".loss ", 1), lo.written(what)[0, 0], loss, bl)
        if d:
            o = d.written(what).view(B, T, F)
            held(what.replace(" ", ".dpred ", 1), o, dp, bd)
            assert (o[dp == 0] == 0).all(), "dpred is not exactly zero off the mask"


# ----------------------------------------------------------------------------------------------------------------------
# gradient norm, clip, Adam
# ----------------------------------------------------------------------------------------------------------------------
ADAM = dict(lr=2e-4, b1=0.9, b2=0.999, eps=1e-8)


@pytest.mark.parametrize("entry", ("hig_clip_adam", "hig_clip_adam_lrdev", "hig_clip_adam_shadow"))
@pytest.mark.parametrize("n", rb.ADAM_N)
def test_sumsq_clip_adam(n, entry):
    """Three steps on one state: below the clip, above it, max_norm <= 0.  4194307 floats: second trips of sumsq_kernel and
    clip_adam_kernel and the scalar tail.  lrdev / shadow: the device learning rate differs from the argument and must win;
    shadow (shadow_n = n rounded down to 4, and 0 in the last step) must be exactly bf16(p)."""
    g0 = rb.gen(n)
    host = dict(p=torch.randn(n, generator=g0), m=0.1 * torch.randn(n, generator=g0), v=0.01 * torch.rand(n, generator=g0))
    bufs = {k: Buf.flat(n) for k in host}
    for k in host:
        bufs[k].out.copy_(host[k].to(DEV).view(1, -1))
    state = Buf.flat(2)     # {float gnorm; int32 step}
    state.out.zero_()
    inv_world = 0.25
    lr_arg = ADAM["lr"] if entry == "hig_clip_adam" else 1.0     # (a wrong argument: the device value must win)
    lr_dev = torch.tensor([ADAM["lr"]], device=DEV)
    for step, max_norm in enumerate((1e6, 0.5, -1.0)):
        g = 8 * torch.randn(n, generator=g0)      # (|g| / 4 is above 0.5 even for three elements)
        gd = g.to(DEV)
        scratch = Buf.flat(_lib.NORM_BLOCKS)
        ok(lib().hig_sumsq_partial(P(gd), n, inv_world, scratch.p(), S()))
        scratch.written("hig_sumsq_partial scratch")
        bounds = rb.clip_adam_bound(host["p"], g, host["m"], host["v"], step=step, max_norm=max_norm, inv_world=inv_world, **ADAM)
        common = (bufs["p"].p(), P(gd), bufs["m"].p(), bufs["v"].p(), n, lr_arg)
        tail = (ADAM["b1"], ADAM["b2"], ADAM["eps"], max_norm, inv_world, scratch.p(), state.p(), state.p(1))
        shadow = None
        if entry == "hig_clip_adam":
            ok(lib().hig_clip_adam(*common, *tail, S()))
        elif entry == "hig_clip_adam_lrdev":
            ok(lib().hig_clip_adam_lrdev(*common, P(lr_dev), *tail, S()))
        else:
            shadow_n = n // 4 * 4 if step < 2 else 0
            shadow = Buf.flat(max(shadow_n, 4), BF16)
            ok(lib().hig_clip_adam_shadow(*common, P(lr_dev), *tail, shadow.p(), shadow_n, S()))
        what = "%s n%d_step%d" % (entry, n, step)
        state.guards(what)
        assert state.out.view(torch.int32)[0, 1].item() == step + 1, "step_dev does not count"
        held(what.replace(" ", ".gnorm ", 1), state.out.cpu()[0, 0], *bounds["gnorm"])
        for k in host:
            host[k] = bufs[k].written(what + " " + k)[0].clone()
            held(what.replace(" ", ".%s " % k, 1), host[k], *bounds[k])
        if shadow is not None:
            if shadow_n:
                assert torch.equal(shadow.written(what + " shadow")[0].view(torch.int16), host["p"][:shadow_n].to(BF16).view(torch.int16)), "the shadow is not bf16(p)"
            else:
                shadow.untouched(what + " shadow_n = 0")


# ----------------------------------------------------------------------------------------------------------------------
# refusals: non-zero, before any launch, the NaN fill intact
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = lib()
    rows, rps = 6, 3
    z = torch.zeros(rows, 1100, device=DEV)
    z16 = z.to(BF16)
    vec = torch.ones(6 * 1100, device=DEV)
    st_in = torch.ones(rows, 2, device=DEV)

    def fwd32(n, ldx, lda, what):
        a, st = Buf(rows, n, max(lda, n) + 4), Buf.flat(2 * rows)
        refused(L.hig_layernorm(P(z), ldx, rows, n, P(vec), P(vec), a.p(), lda, st.p(), S()), [a, st], "hig_layernorm " + what)
        refused(L.hig_ln_mod_silu(P(z), ldx, rows, n, P(vec), P(vec), P(vec), 0, n, rps, a.p(), lda, st.p(), S()), [a, st], "hig_ln_mod_silu " + what)

    fwd32(150, 1100, 152, "n % 4")
    fwd32(1028, 1100, 1028, "n = 1028")
    fwd32(152, 1101, 152, "ldx off by one")
    fwd32(152, 1100, 153, "lda off by one")

    def fwd16(n, ldx, ldo, what):
        o = Buf(rows, n, max(ldo, n) + 8, BF16)
        refused(L.hig_ln_bf16(P(z), 1, ldx, rows, n, P(vec), P(vec), None, 0, 0, rps, o.p(), ldo, S()), [o], "hig_ln_bf16 " + what)

    fwd16(148, 1096, 152, "n % 8")
    fwd16(1032, 1096, 1032, "n = 1032")
    fwd16(152, 1097, 152, "ldx off by one")
    fwd16(152, 1096, 153, "ldo off by one")

    def bwd32(n, ldda, ldx, ldr, lddx, what, res=True):
        dx, partial, dg, db = Buf(rows, max(n, 4), max(lddx, n, 4) + 4), Buf.flat(4096 * 64), Buf.flat(max(n, 4)), Buf.flat(max(n, 4))
        refused(L.hig_ln_bwd(P(z), ldda, P(z), ldx, P(st_in), P(vec), P(vec), None, 0, 0, 0, P(z) if res else None, ldr, dx.p(), lddx,
                             rows, n, rps, dg.p(), db.p(), None, 0, partial.p(), S()), [dx, partial, dg, db], "hig_ln_bwd " + what)

    bwd32(150, 1100, 1100, 1100, 152, "n % 4")
    bwd32(1028, 1100, 1100, 1100, 1028, "n = 1028")
    bwd32(0, 1100, 1100, 1100, 152, "n = 0")
    bwd32(-4, 1100, 1100, 1100, 152, "n < 0")
    bwd32(152, 1101, 1100, 1100, 152, "ldda off by one")
    bwd32(152, 1100, 1101, 1100, 152, "ldx off by one")
    bwd32(152, 1100, 1100, 1100, 153, "lddx off by one")
    bwd32(152, 1100, 1100, 1101, 152, "ldr off by one")

    def bwd16(n, ldda, what, x_f32=0, dx_f32=0, mod=0, dg=True, db=True):
        dx, partial = Buf(rows, n, n + 4, F32 if dx_f32 else BF16), Buf.flat(4096 * 64)
        g1, g2, dss = Buf.flat(n), Buf.flat(n), Buf(2, 2 * n, 2 * n + 4)
        xx = z if x_f32 else z16
        refused(L.hig_ln_bwd_bf16(P(z16), ldda, P(xx), x_f32, 1100, P(vec), P(vec), P(vec) if mod else None, 0, n, mod, None, 0, dx.p(),
                                  dx_f32, n + 4, rows, n, rps, g1.p() if dg else None, g2.p() if db else None, dss.p() if mod else None,
                                  2 * n + 4, partial.p(), S()), [dx, partial, g1, g2, dss], "hig_ln_bwd_bf16 " + what)

    bwd16(150, 1100, "n % 4")
    bwd16(1028, 1100, "n = 1028")
    bwd16(152, 1101, "ldda off by one")
    bwd16(152, 1100, "fp32 rows with a bf16 result", x_f32=1)
    bwd16(152, 1100, "the stylization form with fp32 rows", x_f32=1, dx_f32=1, mod=1)
    bwd16(152, 1100, "dgamma alone", db=False)
    bwd16(152, 1100, "dbeta alone", dg=False)

    out, partial = Buf.flat(16), Buf.flat(16)
    refused(L.hig_colsum_bf16(P(z16), 1096, rows, 12, out.p(), partial.p(), S()), [out, partial], "hig_colsum_bf16 n % 8")
    refused(L.hig_colsum_bf16(P(z16), 1097, rows, 16, out.p(), partial.p(), S()), [out, partial], "hig_colsum_bf16 ldx off by one")
    o = Buf(12, 8, 16, BF16)
    refused(L.hig_transpose_bf16(P(z16), 1096, rows, 12, o.p(), 16, S()), [o], "hig_transpose_bf16 cols % 8")
    o = Buf(16, 8, 16, BF16)
    refused(L.hig_transpose_bf16(P(z16), 1096, rows, 16, o.p(), 17, S()), [o], "hig_transpose_bf16 ldd off by one")
    m = 13
    srcs, s16 = [torch.zeros(2, 8, device=DEV) for _ in range(m)], [torch.zeros(2, 8, device=DEV, dtype=BF16) for _ in range(m)]
    d32, d16 = [Buf(8, 2, 2) for _ in range(m)], [Buf(8, 8, 8, BF16) for _ in range(m)]
    i32, i64 = (C.c_int32 * m), (C.c_int64 * m)
    refused(L.hig_transpose_batch(m, (C.c_void_p * m)(*[s.data_ptr() for s in srcs]), (C.c_void_p * m)(*[d.out.data_ptr() for d in d32]),
                                  i32(*[2] * m), i32(*[8] * m), S()), d32, "hig_transpose_batch with 13 matrices")
    refused(L.hig_transpose_bf16_batch(m, (C.c_void_p * m)(*[s.data_ptr() for s in s16]), i64(*[8] * m),
                                       (C.c_void_p * m)(*[d.out.data_ptr() for d in d16]), i64(*[8] * m), i32(*[2] * m), i32(*[8] * m), S()),
            d16, "hig_transpose_bf16_batch with 13 matrices")
