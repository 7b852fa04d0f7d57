"""Proves on the CPU that the two tiers of tests/linattn16_bounds.py are sound and that they bite.  For every entry point of
csrc/linattn16.hip and with the inputs of the GPU contract's tables (tests/test_gpu_linattn16_contract.py uses the same
generators, tables and seeds):
  1. SOUNDNESS: a plain fp32 torch evaluation of each kernel's arithmetic -- softmax, statistics and accumulation in fp32,
     operands rounded to bf16 where the kernel rounds them, the chunked online softmax of the context build, the one-pass
     variance of the apply -- stays inside tier 1 and tier 2 for every input kind, at two shapes per entry point; its bf16
     outputs pass the exactness check.  The undecided-operand allowance is shown to be necessary and sufficient: with it no
     element of y is outside tier 2, without it at least one is; and tier 1 with u16 = 2^-9 in place of 2^-8 is exceeded.
  2. BITE: each mutant is rejected by the tier named for it ("gross": tier 1 already rejects it).
  3. THE CAP: every case of the tables whose kind must be decided has at least MIN_DECIDED decided elements per bf16 output,
     from the fp64 reference and the bounds alone.
No GPU, no library call."""
import pytest
import torch

import linattn16_bounds as lb
import rowops_bounds as rb
from linattn16_bounds import BF16, F32


def tier1(out16, pair):
    return rb.ratio(out16, *pair)


def rejected16(out16, ref, b32):
    """A bf16 output is rejected by tier 2: the per-element bound, or the exactness of its decided elements."""
    return rb.ratio(out16, ref, rb.bound16(ref, b32)) > 1.0 or rb.exact16(out16, ref, b32)[1] > 0


def test_weight_frag_is_the_documented_index_formula():
    for J, R, _ in lb.FRAG_SHAPES[:2]:
        Y = torch.arange(J * R).view(J, R)
        f = lb.weight_frag(Y)
        assert f.numel() == J * R
        assert all(f[lb.weight_frag_index(J, R, j, r)] == Y[j, r] for j in range(J) for r in range(R))


# ----------------------------------------------------------------------------------------------------------------------
# context build
# ----------------------------------------------------------------------------------------------------------------------
CTX_SHAPES = ((64, 8, 3, 197), (64, 8, 8, 17), (128, 8, 1, 65), (128, 8, 4, 129))      # (hd, B, H, rows): two per head dim


@pytest.mark.parametrize("spread", (15.0, 40.0))
@pytest.mark.parametrize("hd,B,H,rows", CTX_SHAPES)
def test_context_build(hd, B, H, rows, spread):
    K, V, lens = lb.ctx_case(B, rows, H, hd, 100 + rows + H, spread)
    bd = lb.ctx_bounds(K, V, lens)
    assert bd["Xk"] <= 80
    A, kmax, Z = lb.ctx_eval(K, V, lens, dtype=F32)
    assert torch.equal(kmax.double(), bd["kmax"]), "the column maximum is exact"
    assert rb.ratio(Z, *bd["Z"]) <= 1.0
    assert rb.ratio(A, *bd["A1"]) <= 1.0 and rb.ratio(A, *bd["A2"]) <= 1.0
    empty = lens.clamp(0, rows) == 0
    assert (A[empty] == 0).all() and (kmax[empty] == 0).all() and (Z[empty] == 1).all(), "length 0: A = 0, kstat = (0, 1)"
    # bite
    gross = ("mask_includes_row_len", "last_partial_kstep_dropped") + (("rescale_skipped_for_chunk_1",) if rows > 64 else ())
    for m in gross:
        Am = lb.ctx_eval(K, V, lens, mutant=m)[0]
        assert rb.ratio(Am, *bd["A1"]) > 1.0 and rb.ratio(Am, *bd["A2"]) > 1.0, "%s passes" % m
    assert torch.isnan(lb.ctx_eval(K, V, lens, mutant="mask_includes_row_len")[0]).any(), "the padded rows hold NaN: a mask off by one row shows as NaN"
    Am, _, Zm = lb.ctx_eval(K, V, lens, mutant="denominator_from_rounded_weights")
    assert rb.ratio(Am, *bd["A1"]) <= 1.0, "the rounded denominator is inside tier 1 (that is what tier 2 is for)"
    assert rb.ratio(Am, *bd["A2"]) > 1.0 and rb.ratio(Zm, *bd["Z"]) > 1.0, "denominator_from_rounded_weights passes tier 2"
    # At16: bit-equal to at16_order of A; the two 8-column halves of a block swapped is not
    At = lb.at16_order(A)
    sw = At.view(B, H, hd // 32, hd // 16, 2, 32, 8).flip(4).reshape(B, H, hd, hd)
    live = ~empty
    assert not torch.equal(sw[live], At[live])


# ----------------------------------------------------------------------------------------------------------------------
# apply + stylization front
# ----------------------------------------------------------------------------------------------------------------------
APPLY_SHAPES = ((64, 8, 3, 70), (128, 4, 1, 33))
MOD_MUTANTS = ("gamma_without_one_plus_scale", "shift_read_at_offset_0", "modulation_of_sample_b_minus_1")


@pytest.mark.parametrize("kind", lb.APPLY_KINDS)
@pytest.mark.parametrize("hd,H,B,rows", APPLY_SHAPES)
def test_apply(hd, H, B, rows, kind):
    q, At, gamma, beta, ss = lb.apply_case(kind, B, rows, H, hd, 5)
    bd = lb.apply_bounds(q, At, gamma, beta, ss, B, rows, H, hd)
    o, y = lb.apply_eval(q, At, gamma, beta, ss, B, rows, H, hd, dtype=F32)
    o16, y16 = o.to(BF16), y.to(BF16)
    assert torch.isfinite(o).all()
    assert tier1(y16, bd["y1"]) <= 1.0 and tier1(o16, bd["out1"]) <= 1.0
    assert rb.ratio(y, *bd["y2"]) <= 1.0 and rb.ratio(o, *bd["out2"]) <= 1.0
    assert not rejected16(y16, *bd["y2"]) and not rejected16(o16, *bd["out2"])
    print("%s hd%d H%d: kappa %.3g, share of p undecided %.2f %%, Out decided %.0f %%" % (kind, hd, H, bd["kappa"].max().item(), 100 * bd["und"], 100 * rb.decided(*bd["out2"]).double().mean().item()))
    if kind.startswith("ordinary"):
        gross = ("row_sum_over_one_lane_half",) + MOD_MUTANTS[:2] + (MOD_MUTANTS[2:] if B > 1 else ())
        for m in gross:
            om = lb.apply_eval(q, At, gamma, beta, ss, B, rows, H, hd, mutant=m)[0].to(BF16)
            assert tier1(om, bd["out1"]) > 1.0 and rejected16(om, *bd["out2"]), "%s passes" % m
        # a centred variance is the same function: at kappa ~ 2 the bound does not (and must not) tell it from the one-pass form
        oc = lb.apply_eval(q, At, gamma, beta, ss, B, rows, H, hd, dtype=F32, mutant="centred_variance")[0]
        assert rb.ratio(oc, *bd["out2"]) <= 1.0 and not rejected16(oc.to(BF16), *bd["out2"])
    if kind == "const":
        on = lb.apply_eval(q, At, gamma, beta, ss, B, rows, H, hd, dtype=F32, mutant="variance_not_clamped")[0]
        assert not torch.isfinite(on).all(), "without the clamp the constant rows must give a non-finite rstd (pick c0 so that they do)"
        assert tier1(on.to(BF16), bd["out1"]) > 1.0 and rejected16(on.to(BF16), *bd["out2"])


def test_centred_variance_differs_where_kappa_is_large():
    """What the kappa term is for: at |mean| / std ~ 100 the one-pass variance of an fp32 evaluation is measurably worse than
    the centred one (both inside the bound, which carries kappa)."""
    hd, H, B, rows = 128, 4, 1, 33
    q, At, gamma, beta, ss = lb.apply_case("offset100", B, rows, H, hd, 5)
    bd = lb.apply_bounds(q, At, gamma, beta, ss, B, rows, H, hd)
    ref = bd["out2"][0]
    e1 = (lb.apply_eval(q, At, gamma, beta, ss, B, rows, H, hd, dtype=F32)[0].double() - ref).abs().max().item()
    ec = (lb.apply_eval(q, At, gamma, beta, ss, B, rows, H, hd, dtype=F32, mutant="centred_variance")[0].double() - ref).abs().max().item()
    print("offset100: kappa %.3g, one-pass error %.2e, centred %.2e" % (bd["kappa"].max().item(), e1, ec))
    assert bd["kappa"].min().item() > 1e3 and e1 > 4 * ec


@pytest.mark.parametrize("kind", ("ordinary15", "ordinary40"))
def test_undecided_allowance_is_necessary_and_sufficient(kind):
    """hd = 64, H = 8, rows = 70: a softmax weight next to a bf16 rounding boundary is rounded the other way by the fp32
    evaluation; its allowance covers exactly that.  Tier 1 needs u16 = 2^-8: 2^-9 is exceeded."""
    hd, H, B, rows = 64, 8, 3, 70
    q, At, gamma, beta, ss = lb.apply_case(kind, B, rows, H, hd, 5)
    y = lb.apply_eval(q, At, gamma, beta, ss, B, rows, H, hd, dtype=F32)[1]
    with_, without = (lb.apply_bounds(q, At, gamma, beta, ss, B, rows, H, hd, allowance=a)["y2"] for a in (True, False))
    err = (y.double() - with_[0]).abs()
    assert (err > with_[1]).sum() == 0
    assert (err > without[1]).sum() >= 1, "pick a seed on which the fp32 evaluation flips a weight"
    print("%s: largest error / bound %.2f with the allowance, %.1f without (%d elements outside)" % (kind, rb.ratio(y, *with_), rb.ratio(y, *without), int((err > without[1]).sum())))
    half = lb.apply_bounds(q, At, gamma, beta, ss, B, rows, H, hd, u16=2.0 ** -9)["y1"]
    assert rb.ratio(y.to(BF16), *half) > 1.0


# ----------------------------------------------------------------------------------------------------------------------
# out-projection
# ----------------------------------------------------------------------------------------------------------------------
def stats_ratio(st, h16):
    return rb.ratio(st, lb.panel_stats(h16), lb.panel_stats_bound(h16))


def outproj_checks(a32, bd, W, bias, h, bite):
    v, st = lb.outproj_eval(a32, W, bias, h, dtype=F32)
    h16 = v.to(BF16)
    assert tier1(h16, bd["h1"]) <= 1.0 and not rejected16(h16, *bd["h2"])
    assert stats_ratio(st, h16) <= 1.0
    if not bite:
        return
    a64 = a32.double()
    hm = lb.outproj_eval(a64, W, bias, h, mutant="residual_read_from_the_updated_tile")[0].to(BF16)
    assert tier1(hm, bd["h1"]) > 1.0 and rejected16(hm, *bd["h2"]), "residual_read_from_the_updated_tile passes"
    hm = lb.outproj_eval(a32, W, bias, h, dtype=F32, mutant="bias_added_after_the_rounding")[0].to(BF16)
    assert rejected16(hm, *bd["h2"]), "bias_added_after_the_rounding passes tier 2"
    for m in ("stats_of_panel_p_plus_1", "stats_before_the_rounding"):
        assert stats_ratio(lb.outproj_eval(a32, W, bias, h, dtype=F32, mutant=m)[1], h16) > 1.0, "%s passes" % m


@pytest.mark.parametrize("kind", lb.OUT_KINDS)
@pytest.mark.parametrize("B,rows", ((3, 70), (1, 33)))
def test_attn_out(B, rows, kind):
    W, bias = lb.out_params(3)
    q, At, gamma, beta, ss = lb.apply_case(kind, B, rows, 8, 64, 7)
    h = lb.residual(B * rows, 9)
    bd = lb.attn_out_bounds(q, At, gamma, beta, ss, W, bias, h, B, rows)
    o = lb.apply_eval(q, At, gamma, beta, ss, B, rows, 8, 64, dtype=F32)[0]
    outproj_checks(o, bd, W, bias, h, kind in ("peaked40", "ordinary15", "ordinary40"))
    print("%s: share of the activated tile undecided %.1f %%, h' decided %.0f %%" % (kind, 100 * bd["und"], 100 * rb.decided(*bd["h2"]).double().mean().item()))
    if kind == "ordinary15" and B > 1:
        for m in MOD_MUTANTS:
            om = lb.apply_eval(q, At, gamma, beta, ss, B, rows, 8, 64, mutant=m)[0]
            hm = lb.outproj_eval(om, W, bias, h)[0].to(BF16)
            assert tier1(hm, bd["h1"]) > 1.0, "%s passes tier 1 of h'" % m


@pytest.mark.parametrize("kind", lb.ROWS_KINDS)
@pytest.mark.parametrize("B,rows", ((3, 70), (1, 33)))
def test_rows_out(B, rows, kind):
    W, bias = lb.out_params(3)
    Y, gamma, beta, ss = lb.rows_case(kind, B, rows, 11)
    h = lb.residual(B * rows, 9)
    bd = lb.rows_out_bounds(Y, gamma, beta, ss, W, bias, h, B, rows)
    a = lb.rows_front(Y, gamma, beta, ss, B, rows, dtype=F32)
    assert torch.isfinite(a).all()
    outproj_checks(a, bd, W, bias, h, kind == "ordinary")
    for m in MOD_MUTANTS[:2] + (MOD_MUTANTS[2:] if B > 1 else ()):
        hm = lb.outproj_eval(lb.rows_front(Y, gamma, beta, ss, B, rows, mutant=m), W, bias, h)[0].to(BF16)
        assert tier1(hm, bd["h1"]) > 1.0 and rejected16(hm, *bd["h2"]), "%s passes" % m


# ----------------------------------------------------------------------------------------------------------------------
# the cap, from the reference alone
# ----------------------------------------------------------------------------------------------------------------------
def test_min_decided_holds_for_every_case_of_the_tables():
    """'const' and the 'offset' kinds are exempt (their bound carries kappa and is not small against an ulp), as 'const' is in
    the row-op contract; behind the fused out-projection so is 'ordinary15' (see need_decided)."""
    W, bias = lb.out_params(3)
    low = []

    def check(what, pair):
        f = rb.decided(*pair).double().mean().item()
        if f < rb.MIN_DECIDED:
            low.append("%s %.3f" % (what, f))

    for i, (hd, H, B, rows, kind) in enumerate(lb.apply_cases()):
        if lb.need_decided(kind):
            bd = lb.apply_bounds(*lb.apply_case(kind, B, rows, H, hd, i), B, rows, H, hd)
            check("apply Out %s" % ((hd, H, B, rows, kind),), bd["out2"])
            check("apply Yout %s" % ((hd, H, B, rows, kind),), bd["y2"])
    for i, (B, rows, kind, _) in enumerate(lb.out_cases(lb.OUT_KINDS)):
        if lb.need_decided(kind, True):
            bd = lb.attn_out_bounds(*lb.apply_case(kind, B, rows, 8, 64, 500 + i), W, bias, lb.residual(B * rows, 600 + i), B, rows)
            check("attn_out h' %s" % ((B, rows, kind),), bd["h2"])
    for i, (B, rows, kind, _) in enumerate(lb.out_cases(lb.ROWS_KINDS)):
        if kind == "ordinary":
            bd = lb.rows_out_bounds(*lb.rows_case(kind, B, rows, 700 + i), W, bias, lb.residual(B * rows, 800 + i), B, rows)
            check("rows_out h' %s" % ((B, rows, kind),), bd["h2"])
    assert not low, "fewer than %.0f %% decided: %s" % (100 * rb.MIN_DECIDED, low)
