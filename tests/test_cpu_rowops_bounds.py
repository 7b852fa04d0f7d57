"""Proves on the CPU that the bounds of tests/rowops_bounds.py can fail -- and do not fail what is right.  For every operation
and at every shape of the GPU contract's tables (tests/test_gpu_rowops_contract.py uses the same tables and the same inputs):
  * each MUTANT named for the case, evaluated in fp64, exceeds the bound on at least one element (or, for a bf16 output,
    differs from bf16(ref) on at least one decided element);
  * a straightforward fp32 torch evaluation of the correct operation stays within the bound (and, rounded to bf16, passes the
    exactness check): a bound derived too tight shows here, before any GPU time is spent;
  * every bf16 case on ordinary rows has at least 70 % decided elements;
  * the depth helper equals hand-written values.
No GPU, no library call."""
import pytest
import torch

import rowops_bounds as rb
from rowops_bounds import BF16, F32

# where a mutant is visible: the unbiased variance on ordinary rows (on near-constant rows var << eps hides it), the epsilons
# on near-constant rows only (at var ~ 4 a different eps moves nothing beyond the rounding of fp32)
STAT_MUTANTS = {"ordinary": ("unbiased_variance", "mean_drops_last_column"),
                "const": ("eps_1e-6", "eps_2e-5", "mean_drops_last_column")}
MOD_MUTANTS = ("scale_shift_swapped", "scale_not_one_plus_scale")


def worst(outs, bounds, keys):
    return max(rb.ratio(o, *bounds[k]) for o, k in zip(outs, keys) if o is not None)


def rejected16(out, ref, b32):
    """A bf16 output is rejected by the per-element bound or by the exactness of its decided elements."""
    return rb.ratio(out, ref, rb.bound16(ref, b32)) > 1.0 or rb.exact16(out, ref, b32)[1] > 0


def test_depth_helper_equals_hand_written_values():
    # hig_colsum over 8229 rows: 512 chunks; a wave adds ceil(8229 / 2048) = 5 rows, 3 cross-wave adds; colreduce over 512 rows:
    # 8 trips of the four accumulators, (s0 + s1) + (s2 + s3), 16 across the row lanes
    assert rb.colsum_depth(8229) == 5 + 3 + (8 + 2 + 16)
    # 53 rows: 3 chunks, ceil(53 / 12) = 5 rows per wave, colreduce over 3 rows: one add, 2, 16
    assert rb.colsum_depth(53) == 5 + 3 + (1 + 2 + 16)
    # hig_ln_bwd, 16 samples of 9 rows: 32 splits, one row per wave, 3 cross-wave adds; dgamma: colreduce over 512 partial rows;
    # dscale: 32 splits in sequence
    assert rb.ln_bwd_depths(16, 9, 64, False) == (1 + 3 + 26, 1 + 3 + 32)
    # hig_ln_bwd_bf16, 600 samples of 17 rows: one split (nothing to halve), 8 waves: wave 0 adds rows 0, 8, 16; 7 cross-wave
    # adds; colreduce over 600 rows: 9 trips of four accumulators and 2 single ones, 2, 16; dscale: one split
    assert rb.ln_bwd_depths(600, 17, 64, True) == (3 + 7 + (11 + 2 + 16), 3 + 7 + 1)
    # the halved split count: 2 samples -> 64 splits -> 32 workgroups of 8 waves
    assert rb.ln_bwd16_splits(2, 64) == (32, 8, 2) and rb.ln_bwd16_splits(2, 1024) == (64, 4, 1)
    # hig_masked_mse, 33 x 130 rows: 1023 workgroups, 2 trips, 2 cross-wave levels, 4 trips of the final block, its 8 levels
    assert rb.masked_mse_depth(33, 130) == 2 + 2 + 4 + 8
    assert rb.sumsq_depth(4194307) == 2 + 4 + 1 + 6 + 2 + 4 + 8


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm forward
# ----------------------------------------------------------------------------------------------------------------------
KEYS = ("out", "mean", "rstd")


@pytest.mark.parametrize("kind", rb.KINDS)
@pytest.mark.parametrize("rows", rb.LN32_ROWS)
@pytest.mark.parametrize("n", rb.LN32_N)
def test_ln_forward_fp32(n, rows, kind):
    """hig_rowstats (mean, rstd), hig_layernorm (ss None) and hig_ln_mod_silu."""
    rps = rb.LN32_RPS
    x, gamma, beta, ss = rb.ln_case(kind, rows, n, rps, seed=n + rows)
    for mod in (None, ss):
        bounds = rb.ln_fwd_bound(x, gamma, beta, mod, rps)
        assert worst(rb.ln_fwd_eval(x, gamma, beta, mod, rps, dtype=F32), bounds, KEYS) <= 1.0
        mutants = STAT_MUTANTS[kind] + (MOD_MUTANTS if mod is not None else ())
        if mod is not None and rows > rps:
            mutants += ("sample_off_by_one",)
        for m in mutants:
            outs = rb.ln_fwd_eval(x, gamma, beta, mod, rps, mutant=m)
            assert rb.ratio(outs[0], *bounds["out"]) > 1.0, "%s passes the bound of the output" % m
            if m in STAT_MUTANTS[kind]:     # hig_rowstats sees these through its own two outputs
                assert worst(outs[1:], bounds, KEYS[1:]) > 1.0, "%s passes the bounds of the statistics" % m


def ln16_cases():
    for n in rb.LN16_N:
        yield (n,) + rb.LN16_SMALL
    for rows, rps in rb.LN16_BIG:
        yield 64, rows, rps


@pytest.mark.parametrize("kind", rb.KINDS)
@pytest.mark.parametrize("n,rows,rps", list(ln16_cases()))
def test_ln_forward_bf16(n, rows, rps, kind):
    """hig_ln_bf16: fp32 and bf16 rows, with and without ss."""
    for x_bf16 in (False, True):
        x, gamma, beta, ss = rb.ln_case(kind, rows, n, rps, seed=n + rows + rps, x_bf16=x_bf16)
        for mod in (None, ss):
            ref, b32 = rb.ln_fwd_bound(x, gamma, beta, mod, rps, fast_silu=True)["out"]
            out = rb.ln_fwd_eval(x.float(), gamma, beta, mod, rps, dtype=F32)[0].to(BF16)
            assert not rejected16(out, ref, b32)
            frac = rb.decided(ref, b32).double().mean().item()
            assert kind == "const" or frac >= rb.MIN_DECIDED, "only %.0f %% of the elements are decided" % (100 * frac)
            mutants = STAT_MUTANTS[kind] + (MOD_MUTANTS + ("sample_off_by_one",) if mod is not None else ())
            for m in mutants:
                out = rb.ln_fwd_eval(x, gamma, beta, mod, rps, mutant=m)[0].to(BF16)
                assert rejected16(out, ref, b32), "%s passes" % m


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ----------------------------------------------------------------------------------------------------------------------
BKEYS = ("dx", "dgamma", "dbeta", "dscale", "dshift")


@pytest.mark.parametrize("kind", rb.KINDS)
@pytest.mark.parametrize("n,samples,rps", list(rb.lnb32_cases()))
def test_ln_backward_fp32(n, samples, rps, kind):
    da, x, stats, gamma, beta, ss, res = rb.lnb_case(kind, samples, rps, n, seed=n + samples)
    for mod in (None, ss):
        bounds = rb.ln_bwd_bound(da, x, stats, gamma, beta, mod, res, rps)
        assert worst(rb.ln_bwd_eval(da, x, stats, gamma, beta, mod, res, rps, dtype=F32), bounds, BKEYS) <= 1.0
        red = ("dgamma", "dbeta") + (("dscale", "dshift") if mod is not None else ())
        outs = dict(zip(BKEYS, rb.ln_bwd_eval(da, x, stats, gamma, beta, mod, res, rps, mutant="reductions_drop_last_row")))
        for k in red:
            assert rb.ratio(outs[k], *bounds[k]) > 1.0, "%s without the last row of each sample passes" % k
        if mod is not None:
            for m in MOD_MUTANTS + (("sample_off_by_one",) if samples > 1 else ()):
                outs = dict(zip(BKEYS, rb.ln_bwd_eval(da, x, stats, gamma, beta, mod, res, rps, mutant=m)))
                for k in ("dx", "dgamma", "dbeta"):
                    assert rb.ratio(outs[k], *bounds[k]) > 1.0, "%s passes the bound of %s" % (m, k)


@pytest.mark.parametrize("kind", rb.KINDS)
@pytest.mark.parametrize("n,samples,rps", list(rb.lnb16_cases()))
def test_ln_backward_bf16(n, samples, rps, kind):
    """hig_ln_bwd_bf16 recomputes the statistics: the variance and epsilon mutants are visible in dx and the gradients."""
    da, x, _, gamma, beta, ss, res = rb.lnb_case(kind, samples, rps, n, seed=n + samples, bf16=True)
    for form in ("sty", "plain16", "plain32", "mixed", "sty_bare", "plain16_bare"):
        xs = x if form == "plain32" else x.to(BF16)
        rs = res.to(BF16) if form in ("sty", "plain16") else res
        bare = form.endswith("_bare")
        if bare:      # res NULL: dx is the bare difference
            form, rs = form[:-5], torch.zeros_like(res)
        mod = ss if form == "sty" else None
        bounds = rb.ln_bwd_bound(da, xs, None, gamma, beta, mod, rs, rps, bf16=True)
        outs = rb.ln_bwd_eval(da.float(), xs.float(), None, gamma, beta, mod, rs.float(), rps, dtype=F32, tree_rows=True)
        assert worst(outs[1:], bounds, BKEYS[1:]) <= 1.0
        ref, b32 = bounds["dx"]
        if form in ("sty", "plain16"):
            assert not rejected16(outs[0].to(BF16), ref, b32)
            frac = rb.decided(ref, b32).double().mean().item()
            assert kind == "const" or frac >= rb.MIN_DECIDED, "only %.0f %% of dx is decided" % (100 * frac)
        else:
            assert rb.ratio(outs[0], ref, b32) <= 1.0
        if bare or form == "mixed":      # (the arithmetic of a form above with another residual / result type: no new mutant)
            continue
        mutants = STAT_MUTANTS[kind] + ("reductions_drop_last_row",) + (MOD_MUTANTS + ("sample_off_by_one",) if mod is not None else ())
        for m in mutants:
            outs = dict(zip(BKEYS, rb.ln_bwd_eval(da, xs, None, gamma, beta, mod, rs, rps, mutant=m)))
            if m == "reductions_drop_last_row":
                keys = ("dgamma", "dbeta") + (("dscale", "dshift") if mod is not None else ())
            elif m in STAT_MUTANTS[kind]:
                keys = ("dx", "dgamma")
            else:
                keys = ("dx", "dgamma", "dbeta")
            caught = [k for k in keys if (rejected16(outs[k].to(BF16), ref, b32) if k == "dx" and form in ("sty", "plain16")
                                          else rb.ratio(outs[k], *bounds[k]) > 1.0)]
            # Every named output must show the mutant, with two exceptions that follow from the arithmetic: a wrong statistic
            # moves every TERM of dgamma by a signed 1 / (2 n) of itself, which a sum over rows averages out under a bound
            # that adds absolute values (and a shifted mean cancels in dx to first order); and on near-constant rows xhat is
            # only known to ~1e-2 (r ~ 300 times the rounding of the mean), so the sums that carry it (dgamma, dscale) have
            # a bound of their own size.  There one output must show it.
            if kind == "ordinary" and m not in STAT_MUTANTS[kind]:
                assert caught == list(keys), "%s passes in %s" % (m, sorted(set(keys) - set(caught)))
            assert caught, "%s passes in all of %s" % (m, keys)


# ----------------------------------------------------------------------------------------------------------------------
# column sums, masked loss, DDPM steps, clip + Adam, GELU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", rb.COLSUM_ROWS)
def test_colsum(rows):
    for bf16, widths in ((False, rb.COLSUM32_N), (True, rb.COLSUM16_N)):
        for n in widths:
            x = rb.rows_input("ordinary", rows, n, rb.gen(rows + n))
            x = x.to(BF16) if bf16 else x
            ref, bound = rb.colsum_bound(x)
            assert rb.ratio(rb.colsum_eval(x.float(), dtype=F32), ref, bound) <= 1.0
            mutants = ("drops_last_row",) + (("drops_last_chunk",) if rb.colsum_chunks(rows) > 1 else ())
            for m in mutants:
                assert rb.ratio(rb.colsum_eval(x, mutant=m), ref, bound) > 1.0, "%s passes" % m


@pytest.mark.parametrize("B,T,F", rb.MSE_SHAPES)
def test_masked_mse(B, T, F):
    pred, target, length = rb.mse_case(B, T, F, seed=B)
    for ln in (length, None):
        (loss, bl), (dp, bd) = rb.masked_mse_bound(pred, target, ln)
        l32, d32 = rb.masked_mse_eval(pred, target, ln, dtype=F32)
        assert rb.ratio(l32, loss, bl) <= 1.0 and rb.ratio(d32, dp, bd) <= 1.0
    lm, dm = rb.masked_mse_eval(pred, target, length, mutant="mask_t_le_length")
    (loss, bl), (dp, bd) = rb.masked_mse_bound(pred, target, length)
    assert rb.ratio(lm, loss, bl) > 1.0 and rb.ratio(dm, dp, bd) > 1.0


def test_ddpm_steps():
    x, eps, z, t, tab = rb.ddpm_case()
    (xp, b), (x0, b0) = rb.p_step_bound(x, eps, z, t, tab)
    o32 = rb.p_step_eval(x, eps, z, t, tab, dtype=F32)
    assert rb.ratio(o32[0], xp, b) <= 1.0 and rb.ratio(o32[1], x0, b0) <= 1.0
    assert rb.ratio(rb.p_step_eval(x, eps, z, t, tab, mutant="noise_at_t0")[0], xp, b) > 1.0
    ref, bq = rb.q_sample_bound(x, eps, t, tab)
    assert rb.ratio(rb.q_sample_eval(x, eps, t, tab, dtype=F32), ref, bq) <= 1.0
    assert rb.ratio(rb.q_sample_eval(x, eps, t, tab, mutant="coefficients_swapped"), ref, bq) > 1.0


@pytest.mark.parametrize("rows", rb.EXTENTS)
def test_transpose_with_layernorm(rows):
    g = rb.gen(rows)
    for cols in rb.EXTENTS:
        x, stats, gamma, beta = rb.transpose_ln_case(rows, cols, g)
        ref, bound = rb.transpose_ln_bound(x, stats, gamma, beta)
        assert rb.ratio(rb.transpose_ln_eval(x, stats, gamma, beta, dtype=F32), ref, bound) <= 1.0
        if rows > 1:
            assert rb.ratio(rb.transpose_ln_eval(x, stats, gamma, beta, mutant="stats_of_the_next_row"), ref, bound) > 1.0


ADAM = dict(lr=2e-4, b1=0.9, b2=0.999, eps=1e-8)


@pytest.mark.parametrize("n", rb.ADAM_N)
@pytest.mark.parametrize("max_norm", (1e6, 0.5, 0.0))
def test_clip_adam(n, max_norm):
    g0 = rb.gen(n)
    p, g, m, v = torch.randn(n, generator=g0), torch.randn(n, generator=g0), 0.1 * torch.randn(n, generator=g0), 0.01 * torch.rand(n, generator=g0)
    args = dict(ADAM, step=2, max_norm=max_norm, inv_world=0.25)
    bounds = rb.clip_adam_bound(p, g, m, v, **args)
    keys = ("p", "m", "v", "gnorm")
    assert worst(rb.clip_adam_eval(p, g, m, v, dtype=F32, **args), bounds, keys) <= 1.0
    assert rb.ratio(rb.clip_adam_eval(p, g, m, v, mutant="no_bias_correction", **args)[0], *bounds["p"]) > 1.0
    if max_norm == 0.5:     # inv_world = 1/4: the raw norm is above the clip, the averaged one as well, but 4 times smaller
        outs = rb.clip_adam_eval(p, g, m, v, mutant="clip_before_inv_world", **args)
        assert rb.ratio(outs[1], *bounds["m"]) > 1.0 and rb.ratio(outs[0], *bounds["p"]) > 1.0


def test_tanh_gelu_is_not_the_erf_gelu_in_bf16():
    """hig_gelu_bf16 is held to one bf16 ulp of the erf form (include/hig.h); the tanh form differs by up to ~3e-4 absolute,
    which that bound sees where the output's ulp is below it."""
    z = torch.linspace(-6, 6, 8 * 4001).to(BF16)
    ref = rb.gelu_eval(z)
    bound = rb.ulp16(ref) + 2.0 ** -126
    assert rb.ratio(rb.gelu_eval(z.float(), dtype=F32).to(BF16), ref, bound) <= 1.0
    assert rb.ratio(rb.gelu_eval(z, mutant="tanh_gelu").to(BF16), ref, bound) > 1.0


def test_ln_bwd_refuses_bad_extents_on_the_host():
    """The argument checks of hig_ln_bwd run before anything touches a device, so they can be held here: n <= 0 and (with `res`)
    an ldr that is no multiple of 4 are HIG_EINVAL, as are the conditions its bf16 twin already refused.  The pointers are
    never dereferenced."""
    import ctypes as C
    from hig_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(n, ldda=64, ldx=64, ldr=64, lddx=64, res=True):
        return L.hig_ln_bwd(p, ldda, p, ldx, p, p, p, None, 0, 0, 0, p if res else None, ldr, p, lddx, 4, n, 2, p, p, None, 0, p, None)

    EINVAL = -1
    for kw in (dict(n=0), dict(n=-4), dict(n=6), dict(n=1028), dict(n=8, ldr=65), dict(n=8, ldda=65), dict(n=8, ldx=65), dict(n=8, lddx=65)):
        assert call(**kw) == EINVAL, "hig_ln_bwd accepts %s" % kw
        assert "hig_ln_bwd" in _lib.last_error()
