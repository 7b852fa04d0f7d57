"""fp64 references, element-wise bounds, summation depths and the case tables of the row-wise and elementwise kernels
(csrc/rowops.hip, csrc/rowops_bf16.hip, csrc/ddpm.hip).  Plain torch on the host: tests/test_cpu_rowops_bounds.py proves
without a GPU that the bounds reject wrong arithmetic and accept fp32, tests/test_gpu_rowops_contract.py holds the kernels
to them.

ONE RULE (the rule of tests/test_gpu_attn_contract.py): a result differs from its fp64 value by at most gamma u M,
u = 2^-24, M = the same expression with every term replaced by its absolute value, gamma = a count of roundings.  Every
`*_eval` function below states an operation once, for any dtype and with an optional `mutant` (a deliberately wrong variant);
the reference is its fp64 evaluation, `dtype=torch.float32` is "a straightforward fp32 evaluation", and the mutants are what
the CPU test shows the bounds to reject.

Counting conventions
  * one fp32 add / multiply / correctly rounded division or sqrt: 1 (u relative to its result); a fused multiply-add counts
    as the two operations it replaces (it rounds once, so the count is an upper bound whether or not the compiler contracts).
  * rsqrtf and __builtin_amdgcn_rcpf (v_rsq_f32, v_rcp_f32): 1 ulp = 2 u.  This is the figure of the CDNA ISA manual, not a
    measurement.  v_exp_f32: 1 ulp = 2 u, same source.  OCML's expf (hig_p_sample_step): 1 ulp = 2 u, its documented bound.
  * __expf(x) = v_exp_f32(x log2 e): (2 + 2.5 |x|) u relative (the product with the rounded constant 1.5 |x| u, its own
    rounding |x| u, the instruction 2 u).
  * a reciprocal and a product: 3.
  * a bf16 output adds half a bf16 ulp of the reference (`ulp16`), and is held to EXACTNESS where the bound decides it:
    rounding is monotone, so when bf16(ref - bound) == bf16(ref + bound) every value within the bound rounds to that one
    bf16 number (`decided`); a decided element must equal bf16(ref) bit for bit.  At least 70 % of a case's elements must be
    decided (`MIN_DECIDED`), except on the near-constant rows, whose bound is ~1e-2 |ref|.
  * ROW SUMS (n <= 1024 terms): the linear worst case n u sum |t|, valid in any order.
  * LONG REDUCTIONS over rows or flat buffers (column sums, dgamma / dbeta / dss, the masked loss, the gradient norm): the
    linear bound is useless (at 8229 rows it exceeds one whole dropped row), so h u sum |t| with h = the DEPTH of the
    kernel's own summation tree: the largest number of additions one term passes through -- per-thread trips, cross-wave
    adds, the colreduce_kernel / final-block tree.  The `*_depth` helpers compute h from the quantities the host code uses
    (rows, splits_for(samples) and its halving in hig_ln_bwd16_launch, hig_colsum_chunks(rows), the grid caps); they restate
    the launch arithmetic of the .hip files and never call a kernel.

LayerNorm forward (`ln_fwd_bound`).  mu, d = x - mu, var = mean d^2, r = (var + eps)^-1/2, A = mean |x|, D1 = mean |d|:
    d_mu  = (n + 1) u A                                   n - 1 adds, the division, one spare
    rho   = d_mu D1 / (var + eps) + ((n + 5) / 2 + 2) u   relative error of r: the mean's error enters var through the cross
                                                          term 2 d_mu mean|d| (halved by the square root); the n-term sum,
                                                          subtraction, square, division and + eps (n + 5, halved); v_rsq 2
    y = g d r + b:   |g| r (d_mu + u |d|) + |g d| r (rho + 3 u) + u (|y| + |b|)
The d_mu terms carry mean |x| into every element: on a constant row r ~ 316 multiplies the rounding of the mean.
    z = y (1 + sc) + sh:   b_y |1 + sc| + 2 u |y (1 + sc)| + u |z|
    silu(z) = z sigma(z):  1.1 b_z + |silu| ((2 + 2.5 |z|) (1 - sigma) + G) u      |silu'| <= 1.1;  the exponential's error
          reaches the denominator 1 + e^-z scaled by e^-z / (1 + e^-z) = 1 - sigma;  G = 3 for the add and the division of
          hig_silu (2, one spare), G = 4 for the add, v_rcp (2) and the product of hig_silu_fast (the bf16 kernels).
stats: |mean - mu| <= d_mu, |rstd - r| <= rho r.

LayerNorm backward (`ln_bwd_bound`).  xhat = d r carries e_xh: with `stats` given (hig_ln_bwd) its own 3 roundings, 3 u
|xhat|; recomputed (hig_ln_bwd_bf16: xhat = fma(x, r, -mu r)) the forward's  r (d_mu + u |mu| + u |d|) + |xhat| (rho + 3 u).
Per element, e_(.) the absolute error of (.):
    nrm = xhat g + b          e_nrm = |g| e_xh + u |xhat g| + u |nrm|
    w = nrm (1 + sc) + sh     e_w   = e_nrm |1 + sc| + 2 u |nrm (1 + sc)| + u |w|
    s = sigma(w)              eps_s = ((2 + 2.5 |w|) (1 - s) + G') u relative   G' = 2 (add, division), 3 with v_rcp
    D = s (1 + w (1 - s))     e_D   = 0.5 e_w + s (|w| (eps_s s + 2 u (1 - s)) + u |1 + w (1 - s)|) + (eps_s + u) |D|
                                                                                 |silu''| <= 0.5
    du = da D                 e_du  = |da| e_D + u |du|                          (the dshift term)
    du nrm                    |nrm| e_du + |du| e_nrm + u |du nrm|               (the dscale term)
    dn = du (1 + sc)          e_dn  = e_du |1 + sc| + 2 u |dn|                   (the dbeta term; plain form: dn = da, e_dn = 0)
    dn xhat                   |xhat| e_dn + |dn| e_xh + u |dn xhat|              (the dgamma term)
    dxo = dn g                e_dxo = |g| e_dn + u |dxo|
    s1 = mean dxo             (mean e_dxo) + (H + 2) u mean |dxo|               H = n, the linear row sum; hig_ln_bwd_bf16: see below
    s2 = mean dxo xhat        mean (|xhat| e_dxo + |dxo| e_xh + u |dxo xhat|) + (H + 2) u mean |dxo xhat|
    dx = r (dxo - s1 - xhat s2) + res,  Min = |dxo| + |s1| + |xhat s2|:
          r (e_dxo + e_s1 + |xhat| e_s2 + |s2| e_xh + u |xhat s2| + 3 u Min) + 2 u (|dx| + |res|)
          (hig_ln_bwd_bf16, which rebuilds r: + rho r Min)
    a reduction of terms t with errors e_t over the rows:  sum e_t + h u sum |t|.
hig_ln_bwd_bf16 is the one place where a ROW sum is counted by depth as well (H = ln_bwd16_row_depth(n) = 2 NIT + 7 in s1, s2 and
in the d_mu and rho of its rebuilt statistics): with `res` NULL its bf16 dx is a difference of three terms of one size, and
under the linear n u the bound leaves fewer than 70 % of such a case decided (42 % at n = 1024), so the exactness check
would hardly bite.  The fp32 evaluation that the CPU test holds to it sums rows pairwise (`tree_rows`).

The largest error / bound ratios measured on an MI355X are tabulated in tests/test_gpu_rowops_contract.py.
"""
import math

import torch

U = 2.0 ** -24
EPS = 1e-5
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
MIN_DECIDED = 0.70
NORM_BLOCKS = 1024        # HIG_NORM_BLOCKS
COLSUM_CHUNKS = 512       # HIG_COLSUM_CHUNKS
WAVES = 4                 # waves per workgroup of the row kernels


def ulp16(r):
    """bf16 ulp of |r| (2^(e - 7) for |r| in [2^e, 2^(e + 1)); the normal range's smallest below 2^-126)."""
    e = torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def bound16(ref, bound32):
    """The bound of a bf16 output whose fp32 value is held to bound32."""
    return bound32 + 0.5 * ulp16(ref)


def decided(ref, bound32):
    """Elements whose bf16 rounding the fp32 bound decides: every value in [ref - bound, ref + bound] rounds to bf16(ref)."""
    lo, hi = (ref - bound32).to(BF16), (ref + bound32).to(BF16)
    return (lo == hi) & (lo == ref.to(BF16))


def exact16(out16, ref, bound32):
    """(fraction of decided elements, number of decided elements that differ from bf16(ref))."""
    dec = decided(ref, bound32)
    wrong = dec & ~(out16.to(BF16) == ref.to(BF16))         # (equal VALUES: -0 == +0, a NaN differs)
    return dec.double().mean().item(), int(wrong.sum())


def ratio(out, ref, bound):
    """Largest |out - ref| / bound (0 / 0 counts as 0, x / 0 as inf, a NaN output as inf)."""
    err = (out.double() - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return q.max().item() if q.numel() else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# summation depths (restating the launch arithmetic of the .hip files)
# ----------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def splits_for(samples):
    """splits_for of csrc/rowops.hip: workgroups per sample of the LayerNorm backward kernels."""
    s = 1
    while samples * s < 512 and s < 64:
        s *= 2
    return s


def ln_bwd16_splits(samples, n):
    """hig_ln_bwd16_launch: (splits, waves per workgroup, rows per wave and trip)."""
    s, nit = splits_for(samples), cdiv(n, 256)
    if nit <= 2:
        return (s // 2 if s > 1 else s), 8, 2
    return s, 4, 1


def ln_bwd16_row_depth(n):
    """A row sum of ln_bwd16_kernel (mean, variance, s1, s2): a lane adds its NIT float4 -- at most two sequential adds per
    float4 (the packed halves of s1 / s2; (a + b) + (c + d) and `+=` for the statistics) --, one add of the two halves, the
    6-level wave sum."""
    return 2 * cdiv(n, 256) + 1 + 6


def colsum_chunks(rows):
    """hig_colsum_chunks."""
    return max(1, min(COLSUM_CHUNKS, rows // 16))


def colreduce_depth(nr):
    """colreduce_kernel (and the column blocks of ln_bwd_reduce_kernel) over nr rows: row lane ry adds rows ry, ry + 16, ..
    into four accumulators 64 rows apart, the rest into the first; (s0 + s1) + (s2 + s3); 16 sequential adds across ry."""
    worst = 0
    for ry in range(16):
        r = ry
        trips = 0
        while r + 48 < nr:
            trips, r = trips + 1, r + 64
        while r < nr:
            trips, r = trips + 1, r + 16
        worst = max(worst, trips)
    return worst + 2 + 16


def colsum_depth(rows):
    """hig_colsum / hig_colsum_bf16: per-wave trips over the chunk's rows, 3 cross-wave adds, colreduce over the chunks."""
    chunks = colsum_chunks(rows)
    return cdiv(rows, WAVES * chunks) + (WAVES - 1) + colreduce_depth(chunks)


def ln_bwd_depths(samples, rps, n, bf16):
    """(h of dgamma / dbeta, h of dscale / dshift) of hig_ln_bwd (bf16: hig_ln_bwd_bf16): a wave's trips over its rows, the
    cross-wave adds, then colreduce over samples * splits partial rows / the sequential sum over a sample's splits."""
    if bf16:
        nsplit, nwv, _ = ln_bwd16_splits(samples, n)
    else:
        nsplit, nwv = splits_for(samples), WAVES
    trips = cdiv(rps, nwv * nsplit)
    return trips + (nwv - 1) + colreduce_depth(samples * nsplit), trips + (nwv - 1) + nsplit


def masked_mse_depth(B, T):
    """hig_masked_mse: a wave's trips over its rows, (w0 + w1) + (w2 + w3), the final block's per-thread trips and its 8-level
    tree over 256 threads."""
    rows = B * T
    nblk = min(cdiv(rows, 4), NORM_BLOCKS - 1)
    return cdiv(rows, 4 * nblk) + 2 + cdiv(nblk, 256) + 8


def sumsq_depth(n):
    """hig_sumsq_partial + the head of clip_adam_kernel: (a + b) + (c + d) and `s +=` per trip of a thread, the scalar tail,
    the 6-level wave sum, (r0 + r1) + (r2 + r3), then 4 trips per thread over the 1024 partials and the 8-level tree."""
    trips = max(1, cdiv(n // 4, NORM_BLOCKS * 256))
    return 2 + trips + 1 + 6 + 2 + NORM_BLOCKS // 256 + 8


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def rows_input(kind, rows, n, g):
    """'ordinary': 2 randn + 0.3.  'const': 0.5 + 2e-3 randn with one exactly constant row and one all-zero row (where there
    are rows for them)."""
    if kind == "ordinary":
        return 2 * torch.randn(rows, n, generator=g) + 0.3
    x = 0.5 + 2e-3 * torch.randn(rows, n, generator=g)
    if rows >= 2:
        x[rows // 2] = 0.5
    if rows >= 3:
        x[rows - 1] = 0.0
    return x


def ln_params(n, samples, g):
    """gamma, beta, ss (samples, 6 n): scale at column 2 n, shift at 3 n, as the model lays it out."""
    gamma = 1 + 0.5 * torch.randn(n, generator=g)
    beta = 0.3 * torch.randn(n, generator=g)
    ss = 0.5 * torch.randn(samples, 6 * n, generator=g)
    return gamma, beta, ss


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm forward: hig_rowstats, hig_layernorm, hig_ln_mod_silu, hig_ln_bf16
# ----------------------------------------------------------------------------------------------------------------------
def sample_of(rows, rps, mutant, samples):
    b = torch.arange(rows) // rps
    if mutant == "sample_off_by_one":       # the last row of a sample reads the next sample's vectors
        b = ((torch.arange(rows) + 1) // rps).clamp_max(samples - 1)
    return b


def rowsum(t, tree=False):
    """Row sums (rows, 1); tree: pairwise (depth ceil(log2 n) <= 10), the order a depth-counted bound may be held to."""
    if not tree:
        return t.sum(1, keepdim=True)
    while t.shape[1] > 1:
        if t.shape[1] % 2:
            t = torch.cat([t, torch.zeros_like(t[:, :1])], 1)
        t = t[:, 0::2] + t[:, 1::2]
    return t


def row_stats(x, eps=EPS, mutant=None, tree=False):
    n = x.shape[1]
    mu = rowsum(x, tree) / n
    if mutant == "mean_drops_last_column":
        mu = x[:, :-1].sum(1, keepdim=True) / n
    d = x - mu
    var = rowsum(d * d, tree) / ((n - 1) if mutant == "unbiased_variance" and n > 1 else n)
    if mutant == "eps_1e-6":
        eps = 1e-6
    if mutant == "eps_2e-5":
        eps = 2e-5
    return mu, d, var, (var + eps) ** -0.5


def ln_fwd_eval(x, gamma, beta, ss=None, rps=1, dtype=F64, mutant=None):
    """(out, mean, rstd): out = LN(x) gamma + beta, with ss (samples, 6 n) silu(LN (1 + scale) + shift)."""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    rows, n = x.shape
    mu, d, var, r = row_stats(x, mutant=mutant)
    y = d * r * gamma + beta
    if ss is None:
        return y, mu[:, 0], r[:, 0]
    b = sample_of(rows, rps, mutant, ss.shape[0])
    sc, sh = ss.to(dtype)[b, 2 * n:3 * n], ss.to(dtype)[b, 3 * n:4 * n]
    if mutant == "scale_shift_swapped":
        sc, sh = sh, sc
    z = y * ((0 if mutant == "scale_not_one_plus_scale" else 1) + sc) + sh
    return z * torch.sigmoid(z), mu[:, 0], r[:, 0]


def ln_fwd_terms(x, hrow=None):
    """The quantities of the forward bound: mu, d, r, d_mu, rho (each (rows, 1)).  hrow: what a row sum costs (None: n, the
    linear worst case)."""
    n = x.shape[1]
    hrow = n if hrow is None else hrow
    mu, d, var, r = row_stats(x)
    d_mu = (hrow + 1) * U * x.abs().mean(1, keepdim=True)
    rho = d_mu * d.abs().mean(1, keepdim=True) / (var + EPS) + ((hrow + 5) / 2 + 2) * U
    return mu, d, r, d_mu, rho


def ln_fwd_bound(x, gamma, beta, ss=None, rps=1, fast_silu=False):
    """{'out' | 'mean' | 'rstd': (ref, bound)} in fp64.  x: the values the kernel reads (fp32, or bf16 rows)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    rows, n = x.shape
    mu, d, r, d_mu, rho = ln_fwd_terms(x)
    y = d * r * gamma + beta
    by = gamma.abs() * r * (d_mu + U * d.abs()) + (gamma * d).abs() * r * (rho + 3 * U) + U * (y.abs() + beta.abs())
    res = {"mean": (mu[:, 0], d_mu[:, 0]), "rstd": (r[:, 0], (rho * r)[:, 0])}
    if ss is None:
        res["out"] = (y, by)
        return res
    b = torch.arange(rows) // rps
    sc1, sh = 1 + ss.double()[b, 2 * n:3 * n], ss.double()[b, 3 * n:4 * n]
    z = y * sc1 + sh
    bz = by * sc1.abs() + 2 * U * (y * sc1).abs() + U * z.abs()
    sg = torch.sigmoid(z)
    out = z * sg
    res["out"] = (out, 1.1 * bz + out.abs() * ((2 + 2.5 * z.abs()) * (1 - sg) + (4 if fast_silu else 3)) * U)
    return res


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm backward: hig_ln_bwd, hig_ln_bwd_bf16
# ----------------------------------------------------------------------------------------------------------------------
def ln_bwd_eval(da, x, stats, gamma, beta, ss, res, rps, dtype=F64, mutant=None, tree_rows=False):
    """(dx, dgamma, dbeta, dscale, dshift) of a = [silu](LN(x) (1 + scale) + shift); stats (rows, 2) = (mean, rstd) as
    hig_ln_bwd receives them, None: recomputed from x (hig_ln_bwd_bf16).  ss None: the plain form (dscale = dshift = None)."""
    da, x, gamma, beta = da.to(dtype), x.to(dtype), gamma.to(dtype), beta.to(dtype)
    rows, n = x.shape
    samples = rows // rps
    if stats is None:
        mu, _, _, r = row_stats(x, mutant=mutant, tree=tree_rows)
    else:
        mu, r = stats.to(dtype)[:, 0:1], stats.to(dtype)[:, 1:2]
    xhat = (x - mu) * r
    nrm = xhat * gamma + beta
    dsc = dsh = None
    keep = torch.ones(rows, 1, dtype=dtype)
    if mutant == "reductions_drop_last_row":
        keep[rps - 1::rps] = 0
    if ss is not None:
        b = sample_of(rows, rps, mutant, samples)
        sc, sh = ss.to(dtype)[b, 2 * n:3 * n], ss.to(dtype)[b, 3 * n:4 * n]
        if mutant == "scale_shift_swapped":
            sc, sh = sh, sc
        sc1 = (0 if mutant == "scale_not_one_plus_scale" else 1) + sc
        w = nrm * sc1 + sh
        s = torch.sigmoid(w)
        du = da * (s * (1 + w * (1 - s)))
        dsh = (du * keep).view(samples, rps, n).sum(1)
        dsc = (du * nrm * keep).view(samples, rps, n).sum(1)
        dn = du * sc1
    else:
        dn = da
    dg, db = (dn * xhat * keep).sum(0), (dn * keep).sum(0)
    dxo = dn * gamma
    s1, s2 = rowsum(dxo, tree_rows) / n, rowsum(dxo * xhat, tree_rows) / n
    dx = r * (dxo - s1 - xhat * s2)
    if res is not None:
        dx = dx + res.to(dtype)
    return dx, dg, db, dsc, dsh


def ln_bwd_bound(da, x, stats, gamma, beta, ss, res, rps, bf16=False):
    """{'dx' | 'dgamma' | 'dbeta' | 'dscale' | 'dshift': (ref, bound)}; bf16: the arithmetic of hig_ln_bwd_bf16 (statistics
    rebuilt, v_rcp in the sigmoid, its split counts).  The bound of 'dx' is that of the fp32 value (see bound16)."""
    ref = ln_bwd_eval(da, x, stats, gamma, beta, ss, res, rps)
    da, x, gamma, beta = da.double(), x.double(), gamma.double(), beta.double()
    rows, n = x.shape
    samples = rows // rps
    hrow = ln_bwd16_row_depth(n) if bf16 else n
    if stats is None:
        mu, d, r, d_mu, rho = ln_fwd_terms(x, hrow)
        xhat = d * r
        e_xh = r * (d_mu + U * mu.abs() + U * d.abs()) + xhat.abs() * (rho + 3 * U)
    else:
        mu, r = stats.double()[:, 0:1], stats.double()[:, 1:2]
        xhat = (x - mu) * r
        e_xh, rho = 3 * U * xhat.abs(), 0.0
    nrm = xhat * gamma + beta
    e_nrm = gamma.abs() * e_xh + U * (xhat * gamma).abs() + U * nrm.abs()
    h_col, h_dss = ln_bwd_depths(samples, rps, n, bf16)
    out = {}

    def over_rows(t, e_t):
        return e_t.sum(0) + h_col * U * t.abs().sum(0)

    def over_sample(t, e_t):
        return e_t.view(samples, rps, n).sum(1) + h_dss * U * t.abs().view(samples, rps, n).sum(1)

    if ss is not None:
        b = torch.arange(rows) // rps
        sc1, sh = 1 + ss.double()[b, 2 * n:3 * n], ss.double()[b, 3 * n:4 * n]
        w = nrm * sc1 + sh
        e_w = e_nrm * sc1.abs() + 2 * U * (nrm * sc1).abs() + U * w.abs()
        s = torch.sigmoid(w)
        eps_s = ((2 + 2.5 * w.abs()) * (1 - s) + (3 if bf16 else 2)) * U
        D = s * (1 + w * (1 - s))
        e_D = 0.5 * e_w + s * (w.abs() * (eps_s * s + 2 * U * (1 - s)) + U * (1 + w * (1 - s)).abs()) + (eps_s + U) * D.abs()
        du = da * D
        e_du = da.abs() * e_D + U * du.abs()
        out["dshift"] = (ref[4], over_sample(du, e_du))
        out["dscale"] = (ref[3], over_sample(du * nrm, nrm.abs() * e_du + du.abs() * e_nrm + U * (du * nrm).abs()))
        dn = du * sc1
        e_dn = e_du * sc1.abs() + 2 * U * dn.abs()
    else:
        dn, e_dn = da, torch.zeros_like(da)
    out["dbeta"] = (ref[2], over_rows(dn, e_dn))
    out["dgamma"] = (ref[1], over_rows(dn * xhat, xhat.abs() * e_dn + dn.abs() * e_xh + U * (dn * xhat).abs()))
    dxo = dn * gamma
    e_dxo = gamma.abs() * e_dn + U * dxo.abs()
    s1, s2 = dxo.mean(1, keepdim=True), (dxo * xhat).mean(1, keepdim=True)
    e_s1 = e_dxo.mean(1, keepdim=True) + (hrow + 2) * U * dxo.abs().mean(1, keepdim=True)
    e_s2 = ((xhat.abs() * e_dxo + dxo.abs() * e_xh + U * (dxo * xhat).abs()).mean(1, keepdim=True)
            + (hrow + 2) * U * (dxo * xhat).abs().mean(1, keepdim=True))
    Min = dxo.abs() + s1.abs() + (xhat * s2).abs()
    bdx = r * (e_dxo + e_s1 + xhat.abs() * e_s2 + s2.abs() * e_xh + U * (xhat * s2).abs() + 3 * U * Min) + rho * r * Min
    bdx = bdx + 2 * U * (ref[0].abs() + (0 if res is None else res.double().abs()))
    out["dx"] = (ref[0], bdx)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# column sums: hig_colsum, hig_colsum_bf16
# ----------------------------------------------------------------------------------------------------------------------
def colsum_eval(x, dtype=F64, mutant=None):
    x = x.to(dtype)
    rows = x.shape[0]
    if mutant == "drops_last_row":
        x = x[:-1]
    if mutant == "drops_last_chunk":       # the rows of the last chunk: chunk, chunk + nchunk, .. in units of 4 rows
        chunks = colsum_chunks(rows)
        x = x[(torch.arange(rows) // WAVES) % chunks != chunks - 1]
    return x.sum(0)


def colsum_bound(x):
    x = x.double()
    return x.sum(0), colsum_depth(x.shape[0]) * U * x.abs().sum(0)


# ----------------------------------------------------------------------------------------------------------------------
# hig_transpose with LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
def transpose_ln_eval(x, stats, gamma, beta, dtype=F64, mutant=None):
    """dst[c][r] = (x[r][c] - mean[r]) rstd[r] gamma[c] + beta[c], stats (rows, 2) = (mean, rstd) as given."""
    x, st, gamma, beta = x.to(dtype), stats.to(dtype), gamma.to(dtype), beta.to(dtype)
    if mutant == "stats_of_the_next_row":
        st = torch.roll(st, -1, 0)
    return ((x - st[:, :1]) * st[:, 1:] * gamma + beta).t()


def transpose_ln_bound(x, stats, gamma, beta):
    """Three roundings on the product (difference, rstd, gamma), one on the sum: 3 u |prod| + u |ref|."""
    prod = (x.double() - stats.double()[:, :1]) * stats.double()[:, 1:] * gamma.double()
    ref = prod + beta.double()
    return ref.t(), (3 * U * prod.abs() + U * ref.abs()).t()


def transpose_ln_case(rows, cols, g):
    x = torch.randn(rows, cols, generator=g)
    stats = torch.stack([torch.randn(rows, generator=g), 0.5 + torch.rand(rows, generator=g)], 1)
    return x, stats, torch.randn(cols, generator=g), torch.randn(cols, generator=g)


# ----------------------------------------------------------------------------------------------------------------------
# hig_masked_mse
# ----------------------------------------------------------------------------------------------------------------------
def masked_mse_eval(pred, target, length, dtype=F64, mutant=None):
    """(loss, dpred): loss = sum_{b, t < length[b]} mean_f (pred - target)^2 / sum_b clamp(length[b], 0, T)."""
    B, T, F = pred.shape
    p, q = pred.to(dtype), target.to(dtype)
    length = torch.full((B,), T, dtype=torch.int64) if length is None else length
    t = torch.arange(T)[None, :]
    on = (t <= length[:, None]) if mutant == "mask_t_le_length" else (t < length[:, None])
    cnt = length.clamp(0, T).sum().to(dtype)
    dlt = p - q
    loss = ((dlt * dlt).sum(2) / F * on).sum() / cnt
    return loss, on[:, :, None] * dlt * (2.0 / (F * cnt))


def masked_mse_bound(pred, target, length):
    """The terms are non-negative, so M = the loss: (F + 3) for a row's mean (difference, square: 3; F terms), one division
    by F, h over the rows, the final division.  dpred = (2 / (F cnt)) (p - q): 4; exactly 0 off the mask."""
    B, T, F = pred.shape
    loss, dp = masked_mse_eval(pred, target, length)
    return (loss, (F + 3 + 1 + masked_mse_depth(B, T) + 1) * U * loss.abs()), (dp, 4 * U * dp.abs())


# ----------------------------------------------------------------------------------------------------------------------
# DDPM steps: hig_q_sample, hig_p_sample_step
# ----------------------------------------------------------------------------------------------------------------------
(T_SQRT_AC, T_SQRT_1M_AC, T_SQRT_RECIP_AC, T_SQRT_RECIPM1_AC, T_COEF1, T_COEF2, T_LOGVAR) = range(7)


def ddpm_table(nsteps):
    """The (7, nsteps) fp32 table of a linear-beta schedule (the values only need to be plausible: the reference reads the
    same fp32 numbers the kernel reads)."""
    betas = torch.linspace(1e-4, 2e-2, nsteps, dtype=F64)
    ac = torch.cumprod(1 - betas, 0)
    acp = torch.cat([torch.ones(1, dtype=F64), ac[:-1]])
    logvar = torch.log(torch.cat([(betas * (1 - acp) / (1 - ac))[1:2], betas[1:]]))
    tab = torch.stack([ac.sqrt(), (1 - ac).sqrt(), (1 / ac).sqrt(), (1 / ac - 1).sqrt(), betas * acp.sqrt() / (1 - ac),
                       (1 - acp) * (1 - betas).sqrt() / (1 - ac), logvar])
    return tab.float()


def q_sample_eval(x0, noise, t, tab, dtype=F64, mutant=None):
    tb = tab.to(dtype)
    a, b = tb[T_SQRT_AC][t][:, None], tb[T_SQRT_1M_AC][t][:, None]
    if mutant == "coefficients_swapped":
        a, b = b, a
    return a * x0.to(dtype) + b * noise.to(dtype)


def q_sample_bound(x0, noise, t, tab):
    """xt = a x0 + b noise: two products and a sum, 2 u M."""
    tb = tab.double()
    a, b = tb[T_SQRT_AC][t][:, None], tb[T_SQRT_1M_AC][t][:, None]
    x0, noise = x0.double(), noise.double()
    return a * x0 + b * noise, 2 * U * ((a * x0).abs() + (b * noise).abs())


EXTENTS = (1, 63, 64, 65, 130)      # both sides of the fp32 transposes, the rows of the bf16 ones
DDPM_SHAPE = (3, 180001, 1000)      # B, per_sample, nsteps: 540003 elements, t = (0, 500, nsteps - 1)
ADAM_N = (3, 100003, 4194307)


def ddpm_case():
    B, per, nsteps = DDPM_SHAPE
    g = gen(11)
    x, eps, z = (torch.randn(B, per, generator=g) for _ in range(3))
    return x, eps, z, torch.tensor([0, 500, nsteps - 1], dtype=torch.int64), ddpm_table(nsteps)


def p_step_eval(x, eps, z, t, tab, dtype=F64, mutant=None):
    """(x_prev, pred_xstart) of one sampling step; rows are samples."""
    tb = tab.to(dtype)
    c = lambda k: tb[k][t][:, None]  # noqa: E731
    x, eps, z = x.to(dtype), eps.to(dtype), z.to(dtype)
    x0 = c(T_SQRT_RECIP_AC) * x - c(T_SQRT_RECIPM1_AC) * eps
    mean = c(T_COEF1) * x0 + c(T_COEF2) * x
    nz = torch.ones_like(mean[:, :1]) if mutant == "noise_at_t0" else (t != 0).to(dtype)[:, None]
    return mean + nz * torch.exp(0.5 * c(T_LOGVAR)) * z, x0


def p_step_bound(x, eps, z, t, tab):
    """x0 = A x - B eps: 2 u M0.  mean = c1 x0 + c2 x: |c1| e_x0 + 2 u M.  sd = expf(logvar / 2): 2 u, its product with z 1,
    the last sum 1 on each side: x_prev within |c1| e_x0 + 2 u (|c1 x0| + |c2 x|) + 3 u |sd z| + u (|mean| + |sd z|)."""
    tb = tab.double()
    c = lambda k: tb[k][t][:, None]  # noqa: E731
    xd, ed, zd = x.double(), eps.double(), z.double()
    xp, x0 = p_step_eval(x, eps, z, t, tab)
    e_x0 = 2 * U * ((c(T_SQRT_RECIP_AC) * xd).abs() + (c(T_SQRT_RECIPM1_AC) * ed).abs())
    mean = c(T_COEF1) * x0 + c(T_COEF2) * xd
    nzsd = (t != 0).double()[:, None] * torch.exp(0.5 * c(T_LOGVAR)) * zd
    b = (c(T_COEF1).abs() * e_x0 + 2 * U * ((c(T_COEF1) * x0).abs() + (c(T_COEF2) * xd).abs()) + 3 * U * nzsd.abs()
         + U * (mean.abs() + nzsd.abs()))
    return (xp, b), (x0, e_x0)


# ----------------------------------------------------------------------------------------------------------------------
# hig_sumsq_partial + hig_clip_adam*
# ----------------------------------------------------------------------------------------------------------------------
def clip_adam_eval(p, g, m, v, step, lr, b1, b2, eps, max_norm, inv_world, dtype=F64, mutant=None):
    """(p, m, v, gnorm) after one clip_grad_norm_ + Adam step; `step` = the count before it.  b1, b2 and their complements
    enter as the fp32 numbers the kernel holds."""
    f = lambda a: torch.tensor(a, dtype=F32).to(dtype)  # noqa: E731
    p, g, m, v = p.to(dtype), g.to(dtype), m.to(dtype), v.to(dtype)
    gnorm = ((g * f(inv_world)) ** 2).sum().sqrt()
    if mutant == "clip_before_inv_world":       # the norm of the raw gradients decides the clip coefficient
        gnorm_c = (g ** 2).sum().sqrt()
    else:
        gnorm_c = gnorm
    coef = torch.clamp(f(max_norm) / (gnorm_c + f(1e-6)), max=1.0) if max_norm > 0 else torch.ones((), dtype=dtype)
    gg = g * (coef * f(inv_world))
    ob1, ob2 = (1 - torch.tensor(b1, dtype=F32)).to(dtype), (1 - torch.tensor(b2, dtype=F32)).to(dtype)
    m = f(b1) * m + ob1 * gg
    v = f(b2) * v + ob2 * gg * gg
    t = step + 1
    bc1, bc2 = 1 - float(f(b1)) ** t, 1 - float(f(b2)) ** t
    if mutant == "no_bias_correction":
        bc1 = bc2 = 1.0
    p = p - (float(f(lr)) / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + f(eps)))
    return p, m, v, gnorm


def clip_adam_bound(p, g, m, v, step, lr, b1, b2, eps, max_norm, inv_world):
    """gnorm: the squares cost 3, the tree h, halved by the square root, + 1: e_n = ((h + 3) / 2 + 1) u relative.  The clip
    coefficient (where it is below 1) e_n + 2 (sum, division), times inv_world 1, times g 1: e_g relative on gg.
    m' = b1 m + (1 - b1) gg: u |b1 m| + (e_g + 2 u) |ob1 gg| + u |m'|.   v' likewise with 2 e_g + 3 u.
    den = sqrt(v') / sqrt(bc2) + eps: (e_v / 2 + 3 u) sqrt-term + u den (sqrt, the rounded constant, product, sum).
    p' = p - ss (m' / den): |step| (e_m / |m'| + e_den / den + 3 u) + u |p'|   (ss rounded, division, product; the difference)."""
    pr, mr, vr, gn = clip_adam_eval(p, g, m, v, step, lr, b1, b2, eps, max_norm, inv_world)
    f = lambda a: float(torch.tensor(a, dtype=F32))  # noqa: E731
    e_n = ((sumsq_depth(g.numel()) + 3) / 2 + 1) * U
    clipped = max_norm > 0 and f(max_norm) / (gn.item() + 1e-6) < 1.0
    e_g = ((e_n + 2 * U) if clipped else 0.0) + 2 * U
    coef = min(1.0, f(max_norm) / (gn.item() + 1e-6)) if max_norm > 0 else 1.0
    gg = g.double() * coef * f(inv_world)
    ob1, ob2 = float(1 - torch.tensor(b1, dtype=F32)), float(1 - torch.tensor(b2, dtype=F32))
    e_m = U * (f(b1) * m.double()).abs() + (e_g + 2 * U) * (ob1 * gg).abs() + U * mr.abs()
    e_v = U * (f(b2) * v.double()).abs() + (2 * e_g + 3 * U) * (ob2 * gg * gg).abs() + U * vr.abs()
    bc1, bc2 = 1 - f(b1) ** (step + 1), 1 - f(b2) ** (step + 1)
    sq = vr.sqrt() / math.sqrt(bc2)
    den = sq + f(eps)
    # d sqrt(v) = e_v / (2 sqrt(v)); where v' = 0 the term vanishes with it (e_v = 0 there)
    e_den = torch.where(vr > 0, e_v / (2 * vr.sqrt().clamp_min(1e-300)) / math.sqrt(bc2), torch.zeros_like(vr)) + 3 * U * sq + U * den
    stepv = (f(lr) / bc1) * (mr / den)
    e_p = (f(lr) / bc1) * (e_m / den) + stepv.abs() * (e_den / den + 3 * U) + U * pr.abs()
    return {"p": (pr, e_p), "m": (mr, e_m), "v": (vr, e_v), "gnorm": (gn, e_n * gn)}


# ----------------------------------------------------------------------------------------------------------------------
# hig_gelu_bf16
# ----------------------------------------------------------------------------------------------------------------------
def gelu_eval(z, dtype=F64, mutant=None):
    z = z.to(dtype)
    if mutant == "tanh_gelu":
        return 0.5 * z * (1 + torch.tanh(0.7978845608028654 * (z + 0.044715 * z ** 3)))
    return 0.5 * z * torch.erfc(-z / 2 ** 0.5)


# ----------------------------------------------------------------------------------------------------------------------
# the case tables (shared by the CPU and the GPU test)
# ----------------------------------------------------------------------------------------------------------------------
KINDS = ("ordinary", "const")
# hig_rowstats / hig_layernorm / hig_ln_mod_silu: NIT 1 (n <= 256), 2 (<= 512), 4 (516 and 768: the NIT = 4 instance with a dead
# slice); 260, 516: a partly live last slice.  rows 1 and 7 with 3 rows per sample: idle waves in the last workgroup, a short
# last sample.
LN32_N = (4, 64, 152, 260, 516, 768, 1024)
LN32_ROWS = (1, 7)
LN32_RPS = 3
# hig_ln_bf16: NIT 1 (n <= 512) and 2; (rows, rps): one row per wave below 32768 rows, four from there on (one and several
# workgroups per sample, the clamped rows beyond a group)
LN16_N = (8, 264, 512, 520, 1024)
LN16_SMALL = (50, 7)
LN16_BIG = ((32771, 7), (32771, 4099))      # at n = 64
# hig_ln_bwd: (samples, rps) -> splits 64, 64, 64, 32, 1: waves and whole splits with no row, a second trip with the prefetch
# of a clamped row, three trips at one split.  (600, 9) at n = 64 only.
LNB32_N = (64, 260, 768, 1024)
LNB32_SHAPES = ((1, 1), (3, 3), (2, 257), (16, 9), (600, 9))
# hig_ln_bwd_bf16: 8 waves x 2 rows per trip (n <= 512), 4 waves x 1 row; the halved split count, a dead second row in the
# last trip, one split with a second trip of one row
LNB16_N = (64, 264, 520, 1024)
LNB16_SHAPES = ((2, 1), (2, 196), (64, 65), (600, 17))
COLSUM_ROWS = (1, 15, 53, 8229)             # 1, 1, 3, 512 chunks
COLSUM32_N = (3, 150, 260, 1536)
COLSUM16_N = (8, 520, 1536)
MSE_SHAPES = ((3, 20, 150), (33, 130, 5))   # the second: 4290 rows > 4 x 1023, a second trip of the grid-stride loop


def lnb32_cases():
    for n in LNB32_N:
        for samples, rps in LNB32_SHAPES:
            if samples == 600 and n != 64:
                continue
            yield n, samples, rps


def lnb16_cases():
    for n in LNB16_N:
        for samples, rps in LNB16_SHAPES:
            yield n, samples, rps


def mse_lengths(B, T):
    pat = (0, 1, T, T + 5, -2, T // 2, T - 1)
    return torch.tensor([pat[i % len(pat)] for i in range(B)], dtype=torch.int64)


# ----------------------------------------------------------------------------------------------------------------------
# case builders (host tensors; the GPU test uploads exactly these)
# ----------------------------------------------------------------------------------------------------------------------
def ln_case(kind, rows, n, rps, seed, x_bf16=False):
    g = gen(seed)
    x = rows_input(kind, rows, n, g)
    if x_bf16:
        x = x.to(BF16)
    gamma, beta, ss = ln_params(n, cdiv(rows, rps), g)
    return x, gamma, beta, ss


def lnb_case(kind, samples, rps, n, seed, bf16=False):
    """da, x, stats (fp32 (mean, rstd) of x as an fp32 LayerNorm forward leaves them), gamma, beta, ss, res."""
    g = gen(seed)
    rows = samples * rps
    x = rows_input(kind, rows, n, g)
    da = torch.randn(rows, n, generator=g)
    res = torch.randn(rows, n, generator=g)
    gamma, beta, ss = ln_params(n, samples, g)
    if bf16:
        da = da.to(BF16)
    mu, _, _, r = row_stats(x.double())
    stats = torch.cat([mu, r], 1).float()
    return da, x, stats, gamma, beta, ss, res


def mse_case(B, T, F, seed):
    g = gen(seed)
    return torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g), mse_lengths(B, T)
