"""The contract of the bf16 matrix-core attention kernels (csrc/linattn16.hip): every output element of hig_linattn_ctx_mm16,
hig_linattn_apply_sty_mm16[_y], hig_attn_out16, hig_rows_out16 and hig_weight_frag16 within a derived bound of its fp64 value
-- twice: tier 1 against the definition, tier 2 against fp64 at the kernel's stated rounding points --, every output written,
nothing around it touched.

References, rounding points, bounds, inputs, tables and seeds are those of tests/linattn16_bounds.py (its docstring carries the
derivations and quotes the shape rules that select each instance; tests/test_cpu_linattn16_bounds.py proves on the CPU that the
bounds are sound and reject wrong arithmetic).  hig_linattn_ctx16_groups has no C entry point and is out of scope.  Rules:
  * every output lives in a `Buf` (NaN-pattern filled, guard rows, guard columns: every leading dimension exceeds the row,
    with a different pad per operand); h is updated in place inside its Buf with ldh = 520; stats is exactly [B rows][4][2];
  * every input sits in NaN: the columns between the row and the leading dimension, a guard row above and below, the unused
    columns of ss (scale at 2 d, shift at 3 d of 6 d + 4); K and V rows at and beyond length[b] hold NaN as well;
  * K / V / Q are column blocks of one (B rows, 3 d + 8) buffer; pointers keep exactly the documented alignment;
  * the references run on the host in fp64 (the same numbers the CPU test holds its fp32 evaluation to).

Measured on an MI355X (largest |error| / bound over all cases; every gamma is derived in tests/linattn16_bounds.py, the ratios,
the offset-kind kappa and the comparison with the unfused pair are the only measurements):
    output                              bound (tier 1 | tier 2)                                              tier 1  at                              tier 2  at
    hig_linattn_ctx_mm16.A              1.01 (u16 + g_A u) MA | g_A u M2 + allowance(P)                      0.881   hd128_B8_H4_r17_len_at16        0.527   hd128_B8_H1_r197_len_at16
    hig_linattn_ctx_mm16.kstat          maximum bit-equal; sum g_Z u Z                                       -                                       0.161   hd128_B8_H4_r16_len_noat16
    hig_linattn_ctx_mm16.At16           bit-equal to at16_order of the kernel's own A                        -                                       -
    hig_linattn_apply_sty_mm16_y.Yout   1.01 (u16 + g_y u) My + u16 |y| | hd u My2 + allowance(p) + ulp16 / 2   0.874   hd64_H8_B3_r31_ordinary40       0.999   hd64_H8_B1_r31_ordinary40
    hig_linattn_apply_sty_mm16.Out      sty_chain of the tier's y error (+ u16 |ref| | + ulp16 / 2)          0.738   hd64_H8_B3_r33_ordinary40       0.998   hd64_H4_B3_r70_peaked40
    hig_attn_out16.h                    outproj_bounds: (e_a + u16 |a|) |W| + 513 u M | 513 u M + allowance(a)   0.072   B3_r70_peaked40_nostats         0.975   B3_r70_peaked40_nostats
    hig_attn_out16.stats                128 u sum |x|; 2 d_mu sum |d| + 128 d_mu^2 + 131 u sum d^2           -                                       0.009   B3_r70_offset10_stats
    hig_rows_out16.h                    the same with the centred sty_chain (h = 14)                         0.491   B3_r70_const_stats              0.989   B3_r70_const_stats
    hig_rows_out16.stats                as above                                                             -                                       0.008   B3_r33_ordinary_stats
    hig_weight_frag16                   bit-equal to the index formula                                       -                                       -
Smallest share of decided elements where MIN_DECIDED is demanded: Out 72 % (hd128_H8_B1_r32_ordinary15), Yout 96 % (the same
case), h' of hig_attn_out16 73 % (ordinary40; 'ordinary15', exempt there, has 58 %), h' of hig_rows_out16 90 % (B1_r1_ordinary).
No decided element differed from bf16(ref) anywhere.
Tier-2 ratios above 0.5, and why.
  * The bf16 outputs (Yout, Out, h') reach 0.98 .. 1.00 by construction: the bound is the fp32 bound plus HALF a bf16 ulp, and an
    element whose fp32 value lies next to a rounding boundary is off by that half ulp.  What holds the arithmetic behind the
    rounding is the exactness of the decided elements.
  * A 0.527 (one case; every other case is below 0.1): one weight P next to a bf16 boundary that the kernel's __expf rounded
    the other way than the fp64 reference; its allowance covers the element, which is what the allowance is for.
The "offset" kind (|mean| / std of the LayerNorm input ~10 and ~100; kappa = (E[y^2] + mean^2) / (var + eps)), Out of the fused
kernel, largest error / tier-2 bound and, against the definition, its largest absolute error next to that of the unfused pair
hig_linattn_apply_bf16 + hig_ln_bf16 on the same inputs:
    case                          kappa     error / bound   fused      unfused pair
    hd64_H8_B3_r70_offset10       400       0.977           6.4e-02    1.2e-01
    hd64_H8_B3_r70_offset100      4.5e+04   0.683           4.4e-01    9.6e-01
    hd128_H4_B3_r70_offset10      480       0.923           4.9e-02    1.3e-01
    hd128_H4_B3_r70_offset100     4.2e+04   0.657           3.3e-01    9.7e-01
  The one-pass variance of apply_sty16_kernel stays inside the kappa bound (the ratios include the half ulp of the bf16 output), no output is non-finite, and the fused
  kernel is 2-3 times CLOSER to the definition than the pair: the pair rounds y to bf16 before the LayerNorm, and at
  |mean| / std = 100 that rounding (2^-9 |mean| ~ std / 5) costs more than the cancellation in sum y^2 / d - mean^2 (fp32,
  kappa u ~ 3e-3).  No kernel was changed.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import linattn16_bounds as lb  # noqa: E402
import rowops_bounds as rb  # noqa: E402
from linattn16_bounds import BF16, F32  # noqa: E402
from test_gpu_rowops_contract import DEV, Buf, P, S, lib, ok, refused  # noqa: E402

NAN = float("nan")


def gin(t, ld=None):
    """The host tensor t on the device with NaN all around it: a vector (or any contiguous block) behind 8 elements of NaN
    and before 8 more (16-byte aligned for fp32 and bf16); a matrix with ld: rows of ld elements, NaN beyond the row, a NaN
    row above and below."""
    if ld is None:
        buf = torch.full((t.numel() + 16,), NAN, dtype=t.dtype, device=DEV)
        buf[8:8 + t.numel()] = t.reshape(-1).to(DEV)
        return buf[8:8 + t.numel()].view(t.shape)
    buf = torch.full((t.shape[0] + 2, ld), NAN, dtype=t.dtype, device=DEV)
    buf[1:-1, :t.shape[1]] = t.to(DEV)
    return buf[1:-1, :t.shape[1]]


def block(parts, R, d, ld):
    """An (R, ld) NaN buffer (plus guard rows) with parts[k] (R, d) at column block k (None: left NaN) -> the list of views."""
    buf = torch.full((R + 2, ld), NAN, dtype=BF16, device=DEV)
    views = []
    for k, t in enumerate(parts):
        v = buf[1:-1, k * d:(k + 1) * d]
        if t is not None:
            v.copy_(t.to(DEV))
        views.append(v)
    return views


def ss_dev(ss, d):
    """ss (B, 6 d + 4) with NaN in every column but scale (2 d ..) and shift (3 d ..) -> (view, pointer to scale, ss_ld, shift offset)."""
    s = ss.clone()
    s[:, :2 * d] = NAN
    s[:, 4 * d:] = NAN
    v = gin(s)
    return v, P(v, 2 * d), 6 * d + 4, d


def held(what, tier, out, ref, bound):
    r = rb.ratio(out, ref, bound)
    print("RATIO %s | %s | %.3f" % (what.split(" ")[0], tier, r), "|", what)
    assert r <= 1.0, "%s, %s: largest |err| / bound = %.3f" % (what, tier, r)


def held16(what, out, pair2, need):
    """Tier 2 of a bf16 output: bound16, and bit-exactness of every element the fp32 bound decides."""
    ref, b32 = pair2
    held(what, "tier 2", out, ref, rb.bound16(ref, b32))
    frac, wrong = rb.exact16(out, ref, b32)
    print("DECIDED %s %.3f" % (what, frac))
    assert wrong == 0, "%s: %d decided elements are not bf16(ref)" % (what, wrong)
    assert not need or frac >= rb.MIN_DECIDED, "%s: only %.0f %% of the elements are decided" % (what, 100 * frac)


# ----------------------------------------------------------------------------------------------------------------------
# hig_weight_frag16
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,R,ldy", lb.FRAG_SHAPES)
def test_weight_frag16(J, R, ldy):
    """A permutation: bit-equal to the documented index formula for every element; (2080, 2048) takes the grid-stride loop
    into its second trip."""
    Y = torch.randn(J, R, generator=lb.gen(J + R)).to(BF16)
    out = Buf.flat(J * R, BF16)
    ok(lib().hig_weight_frag16(P(gin(Y, ldy)), ldy, J, R, out.p(), S()))
    got = out.written("hig_weight_frag16").view(-1)
    assert torch.equal(got.view(torch.int16), lb.weight_frag(Y).view(torch.int16))


# ----------------------------------------------------------------------------------------------------------------------
# hig_linattn_ctx_mm16
# ----------------------------------------------------------------------------------------------------------------------
CTX = list(lb.ctx_cases())


@pytest.mark.parametrize("i", range(len(CTX)), ids=[lb.ctx_id(c) for c in CTX])
def test_context_build(i):
    """ctx16_mfma_kernel<64, 3> (B H < 512), <64, 2> (B H >= 512), <128, 3>: both tiers of A, kstat, At16, with NaN in every
    K / V row at and beyond length[b]."""
    hd, B, H, rows, use_len, use_at = CTX[i]
    d, tag = H * hd, lb.ctx_id(CTX[i])
    K, V, lens = lb.ctx_case(B, rows, H, hd, 100 + i, lb.ctx_spread(rows, H), "pattern" if use_len else None)
    ld = 3 * d + 8
    _, Kd, Vd = block([None, K.view(B * rows, d), V.view(B * rows, d)], B * rows, d, ld)
    lg = None if lens is None else lens.to(DEV)
    A, ks = Buf(B * H * hd, hd, hd, F32), Buf(B * H * hd, 2, 2, F32)
    At = Buf(B * H * hd, hd, hd, BF16) if use_at else None
    ok(lib().hig_linattn_ctx_mm16(P(Kd), P(Vd), ld, B, rows, H, hd, P(lg), A.p(), ks.p(), At.p() if use_at else None, S()))
    a = A.written(tag + " A").view(B, H, hd, hd)
    kst = ks.written(tag + " kstat").view(B, H, hd, 2)
    bd = lb.ctx_bounds(K, V, lens)
    assert bd["Xk"] <= 80
    what = "hig_linattn_ctx_mm16.A " + tag
    held(what, "tier 1", a, *bd["A1"])
    held(what, "tier 2", a, *bd["A2"])
    assert torch.equal(kst[..., 0].double(), bd["kmax"]), tag + ": the column maximum is exact"
    held("hig_linattn_ctx_mm16.kstat " + tag, "tier 2", kst[..., 1], *bd["Z"])
    if lens is not None:
        e0 = lens.clamp(0, rows) == 0
        assert (a[e0] == 0).all() and (kst[e0][..., 0] == 0).all() and (kst[e0][..., 1] == 1).all(), "length 0: A = 0, kstat = (0, 1)"
    if use_at:
        got = At.written(tag + " At16").view(B, H, hd, hd)
        assert torch.equal(got.view(torch.int16), lb.at16_order(a).view(torch.int16)), tag + ": At16 is not the at16_order of the kernel's own A"


# ----------------------------------------------------------------------------------------------------------------------
# hig_linattn_apply_sty_mm16, hig_linattn_apply_sty_mm16_y
# ----------------------------------------------------------------------------------------------------------------------
APPLY = list(lb.apply_cases())


def apply_inputs(q, At, gamma, beta, ss, B, rows, H, hd):
    d = H * hd
    _, qd, _ = block([None, q, None], B * rows, d, 3 * d + 8)
    atd = gin(lb.at16_order(At.transpose(2, 3)))
    return qd, atd, gin(gamma), gin(beta), ss_dev(ss, d)


@pytest.mark.parametrize("i", range(len(APPLY)), ids=["hd%d_H%d_B%d_r%d_%s" % c for c in APPLY])
def test_apply(i):
    """All four instances of apply_sty16_kernel, with and without the second output: y (through Yout) and Out in both tiers;
    the two forms give the same Out bits."""
    hd, H, B, rows, kind = APPLY[i]
    d, R = H * hd, B * rows
    tag = "hd%d_H%d_B%d_r%d_%s" % APPLY[i]
    q, At, gamma, beta, ss = lb.apply_case(kind, B, rows, H, hd, i)
    qd, atd, gd, bd_, (ssv, ssp, ss_ld, soff) = apply_inputs(q, At, gamma, beta, ss, B, rows, H, hd)
    ldq = 3 * d + 8
    out_a, out_b, yout = Buf(R, d, d + 8, BF16), Buf(R, d, d + 8, BF16), Buf(R, d, d + 16, BF16)
    L = lib()
    ok(L.hig_linattn_apply_sty_mm16(P(qd), ldq, P(atd), P(gd), P(bd_), ssp, ss_ld, soff, out_a.p(), d + 8, B, rows, H, hd, S()))
    ok(L.hig_linattn_apply_sty_mm16_y(P(qd), ldq, P(atd), P(gd), P(bd_), ssp, ss_ld, soff, out_b.p(), d + 8, yout.p(), d + 16, B, rows, H, hd, S()))
    oa, ob, y = out_a.written(tag + " Out"), out_b.written(tag + " Out (_y)"), yout.written(tag + " Yout")
    assert torch.equal(oa.view(torch.int16), ob.view(torch.int16)), tag + ": the _y form gives other Out bits"
    b = lb.apply_bounds(q, At, gamma, beta, ss, B, rows, H, hd)
    need = lb.need_decided(kind)
    held("hig_linattn_apply_sty_mm16_y.Yout " + tag, "tier 1", y, *b["y1"])
    held16("hig_linattn_apply_sty_mm16_y.Yout " + tag, y, b["y2"], need)
    held("hig_linattn_apply_sty_mm16.Out " + tag, "tier 1", oa, *b["out1"])
    held16("hig_linattn_apply_sty_mm16.Out " + tag, oa, b["out2"], need)
    if kind.startswith("offset"):
        # the same inputs through the unfused pair hig_linattn_apply_bf16 + hig_ln_bf16 (centred variance, y rounded to bf16 in
        # between): what the fusion costs in accuracy.  Printed, not asserted: the pair has its own contracts.
        A32 = At.transpose(2, 3).float().contiguous().to(DEV)
        yp, op = Buf(R, d, d + 8, BF16), Buf(R, d, d + 8, BF16)
        ok(L.hig_linattn_apply_bf16(P(qd), ldq, P(A32), yp.p(), d + 8, B, rows, H, hd, S()))
        ok(L.hig_ln_bf16(yp.p(), 0, d + 8, R, d, P(gd), P(bd_), ssp, ss_ld, soff, rows, op.p(), d + 8, S()))
        ref = b["out1"][0]
        ef, ep = (oa.double() - ref).abs().max().item(), (op.written("pair").double() - ref).abs().max().item()
        print("OFFSET %s kappa %.3g, error / tier-2 bound %.3f: fused error %.3e, unfused pair %.3e (against the definition)"
              % (tag, b["kappa"].max().item(), rb.ratio(oa, b["out2"][0], rb.bound16(*b["out2"])), ef, ep))


# ----------------------------------------------------------------------------------------------------------------------
# hig_attn_out16, hig_rows_out16
# ----------------------------------------------------------------------------------------------------------------------
def out_call(name, fn_args, bd, W, bias, h, R, use_stats, tag, need):
    """Runs one fused out-projection on a guarded in-place h (ldh = 520) and holds h' (both tiers) and stats."""
    hb = Buf(R, 512, 520, BF16)
    hb.out.copy_(h.to(DEV))
    st = Buf.flat(R * 8) if use_stats else None
    wf, bs = gin(lb.weight_frag(W)), gin(bias)
    ok(fn_args(P(wf), P(bs), hb.p(), 520, st.p() if use_stats else None))
    h2 = hb.written(tag + " h")
    held(name + ".h " + tag, "tier 1", h2, *bd["h1"])
    held16(name + ".h " + tag, h2, bd["h2"], need)
    if use_stats:
        s = st.written(tag + " stats").view(R, 4, 2)
        held(name + ".stats " + tag, "tier 2", s, lb.panel_stats(h2), lb.panel_stats_bound(h2))


ATTN_OUT = list(lb.out_cases(lb.OUT_KINDS))
ROWS_OUT = list(lb.out_cases(lb.ROWS_KINDS))
OUT_ID = lambda c: "B%d_r%d_%s_%s" % (c[0], c[1], c[2], "stats" if c[3] else "nostats")  # noqa: E731


@pytest.mark.parametrize("i", range(len(ATTN_OUT)), ids=[OUT_ID(c) for c in ATTN_OUT])
def test_attn_out16(i):
    """apply_sty16_kernel<64, 8, 8, true>: h updated in place, stats NULL and non-NULL."""
    B, rows, kind, use_stats = ATTN_OUT[i]
    R, d = B * rows, 512
    W, bias = lb.out_params(3)
    q, At, gamma, beta, ss = lb.apply_case(kind, B, rows, 8, 64, 500 + i)
    h = lb.residual(R, 600 + i)
    qd, atd, gd, bd_, (ssv, ssp, ss_ld, soff) = apply_inputs(q, At, gamma, beta, ss, B, rows, 8, 64)
    bd = lb.attn_out_bounds(q, At, gamma, beta, ss, W, bias, h, B, rows)
    call = lambda wf, bs, hp, ldh, sp: lib().hig_attn_out16(P(qd), 3 * d + 8, P(atd), P(gd), P(bd_), ssp, ss_ld, soff, wf, bs, hp, ldh, sp, B, rows, 8, 64, S())  # noqa: E731
    out_call("hig_attn_out16", call, bd, W, bias, h, R, use_stats, OUT_ID(ATTN_OUT[i]), lb.need_decided(kind, True))
    if kind.startswith("offset"):
        print("OFFSET hig_attn_out16 %s kappa %.3g" % (OUT_ID(ATTN_OUT[i]), bd["kappa"].max().item()))


@pytest.mark.parametrize("i", range(len(ROWS_OUT)), ids=[OUT_ID(c) for c in ROWS_OUT])
def test_rows_out16(i):
    """rows_out16_kernel (centred LayerNorm): Y with ldy = 528, h in place, stats NULL and non-NULL."""
    B, rows, kind, use_stats = ROWS_OUT[i]
    R, d = B * rows, 512
    W, bias = lb.out_params(3)
    Y, gamma, beta, ss = lb.rows_case(kind, B, rows, 700 + i)
    h = lb.residual(R, 800 + i)
    yd, gd, bd_, (ssv, ssp, ss_ld, soff) = gin(Y, d + 16), gin(gamma), gin(beta), ss_dev(ss, d)
    bd = lb.rows_out_bounds(Y, gamma, beta, ss, W, bias, h, B, rows)
    call = lambda wf, bs, hp, ldh, sp: lib().hig_rows_out16(P(yd), d + 16, P(gd), P(bd_), ssp, ss_ld, soff, wf, bs, hp, ldh, sp, B, rows, d, S())  # noqa: E731
    out_call("hig_rows_out16", call, bd, W, bias, h, R, use_stats, OUT_ID(ROWS_OUT[i]), kind == "ordinary")


# ----------------------------------------------------------------------------------------------------------------------
# refusals: an error and no launch
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L, s = lib(), S()
    B, rows = 1, 4
    z16 = lambda *sh: torch.zeros(*sh, dtype=BF16, device=DEV)  # noqa: E731
    z32 = lambda *sh: torch.zeros(*sh, device=DEV)  # noqa: E731

    def apply_rc(H, hd, out, ldq=None, ldo=None, qoff=0):
        d = H * hd
        return L.hig_linattn_apply_sty_mm16(P(z16(rows, 3 * d + 8), qoff), ldq or 3 * d + 8, P(z16(H * hd * hd)), P(z32(d)), P(z32(d)), P(z32(B, 6 * d + 4), 2 * d),
                                            6 * d + 4, d, out.p(), ldo or d + 8, B, rows, H, hd, s)

    for H, hd, why in ((8, 32, "head dim 32"), (6, 64, "6 heads")):
        out = Buf(rows, H * hd, H * hd + 8, BF16)
        refused(apply_rc(H, hd, out), [out], "hig_linattn_apply_sty_mm16 " + why)
    out = Buf(rows, 512, 520, BF16)
    refused(apply_rc(8, 64, out, ldq=3 * 512 + 4), [out], "hig_linattn_apply_sty_mm16 ldq % 8")
    refused(apply_rc(8, 64, out, ldo=516), [out], "hig_linattn_apply_sty_mm16 ldo % 8")
    refused(apply_rc(8, 64, out, qoff=4), [out], "hig_linattn_apply_sty_mm16 Q misaligned")

    def ctx_rc(H, hd, A, ks, ld=None, koff=0):
        d = H * hd
        qkv = z16(rows, 3 * d + 8)
        return L.hig_linattn_ctx_mm16(P(qkv, d + koff), P(qkv, 2 * d), ld or 3 * d + 8, B, rows, H, hd, None, A.p(), ks.p(), None, s)

    A, ks = Buf(8 * 32, 32, 32, F32), Buf(8 * 32, 2, 2, F32)
    refused(ctx_rc(8, 32, A, ks), [A, ks], "hig_linattn_ctx_mm16 head dim 32")
    A, ks = Buf(64, 64, 64, F32), Buf(64, 2, 2, F32)
    refused(ctx_rc(1, 64, A, ks, ld=3 * 64 + 4), [A, ks], "hig_linattn_ctx_mm16 ld % 8")
    refused(ctx_rc(1, 64, A, ks, koff=4), [A, ks], "hig_linattn_ctx_mm16 K misaligned")

    h = Buf(rows, 512, 520, BF16)
    wf, v = z16(512 * 512), z32(512)
    ss = z32(B, 6 * 512 + 4)
    refused(L.hig_rows_out16(P(z16(rows, 256)), 256, P(v), P(v), P(ss, 1024), 6 * 512 + 4, 512, P(wf), P(v), h.p(), 520, None, B, rows, 256, s), [h], "hig_rows_out16 d = 256")
    refused(L.hig_rows_out16(P(z16(rows, 516)), 516, P(v), P(v), P(ss, 1024), 6 * 512 + 4, 512, P(wf), P(v), h.p(), 520, None, B, rows, 512, s), [h], "hig_rows_out16 ldy % 8")
    q = z16(rows, 3 * 512 + 8)
    at = z16(4 * 128 * 128)
    refused(L.hig_attn_out16(P(q), 3 * 512 + 8, P(at), P(v), P(v), P(ss, 1024), 6 * 512 + 4, 512, P(wf), P(v), h.p(), 520, None, B, rows, 4, 128, s), [h], "hig_attn_out16 4 heads")
    refused(L.hig_attn_out16(P(q), 3 * 512 + 8, P(at), P(v), P(v), P(ss, 1024), 6 * 512 + 4, 512, P(wf, 4), P(v), h.p(), 520, None, B, rows, 8, 64, s), [h], "hig_attn_out16 W_frag misaligned")
    fr = Buf.flat(32 * 16, BF16)
    refused(L.hig_weight_frag16(P(z16(32, 20)), 20, 32, 16, fr.p(), s), [fr], "hig_weight_frag16 ldy % 8")
    refused(L.hig_weight_frag16(P(z16(48, 16)), 16, 48, 16, fr.p(), s), [fr], "hig_weight_frag16 J % 32")
