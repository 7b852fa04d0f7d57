"""fp64 definitions, the stated rounding points, element-wise bounds, input generators, case tables and mutants of the bf16
matrix-core attention kernels (csrc/linattn16.hip): hig_linattn_ctx_mm16, hig_linattn_apply_sty_mm16[_y], hig_attn_out16,
hig_rows_out16, hig_weight_frag16.  Plain torch, any device: tests/test_cpu_linattn16_bounds.py proves without a GPU that the
bounds hold for an fp32 evaluation of the same arithmetic and reject the mutants, tests/test_gpu_linattn16_contract.py holds the
kernels to them.  hig_linattn_ctx16_groups (the group-strided outputs of the batched text side) has no C entry point and is
out of scope here.

NOTATION.  u = 2^-24; u16 = 2^-8, the unit roundoff of bf16 (8 significant bits: half an ulp is at most 2^-8 of the value);
ulp16 as in tests/rowops_bounds.py; M = "the same expression with every term replaced by its absolute value"; a sum of n
terms in any order costs n u M.  The counts for __expf (2 + 2.5 |x|), reciprocal-and-product (3), the online-softmax rescale
(3 per chunk + merge) and FLOOR are those of the docstring of tests/test_gpu_attn_contract.py:
    g_p = hd + 7 + 2.5 (Xq + log hd)            a softmax weight of q        g_y = g_p + hd
    g_Z = T + 2 + 2.5 log T + 3 (n + 1)         the kstat sum                g_A = (2 + 2.5 Xk + 3 (n + 1)) + T + g_Z + 3
(the apply computes exp2(fma(q, log2 e, -max log2 e)): the rounding of the product max log2 e is common to the row and
cancels in p = e / sum e; what remains per element is the rounded constant and the rounding of the fma, inside 2.5 |x|).

TWO TIERS.  Every output of a matrix-core product is held twice.
  Tier 1, the definition: against the exact fp64 operator on the bf16 inputs as given.  The bound carries u16 M for each
  operand the kernel rounds to bf16 before a product (include/hig.h: softmax(K) in the context build, softmax(Q) in the
  apply, the activated tile in the out-projection), the fp32 counts, and u16 |ref| for a bf16 output.
  Tier 2, the arithmetic: against fp64 evaluated AT THE KERNEL'S ROUNDING POINTS (below), so that only fp32 accumulation
  and the fp32 transcendental functions differ: gamma u M, ~500 times tighter.
UNDECIDED OPERANDS.  A tier-2 reference cannot know which way the kernel rounded an operand whose fp64 value x lies within
its fp32 error of a bf16 rounding boundary.  With eb the operand's relative fp32 bound, lo = bf16(x (1 - eb)) and hi =
bf16(x (1 + eb)): the kernel's operand and the reference's are both in [lo, hi], so (hi - lo) |other operand| is added to
the bound of every output element the operand feeds (`gap16`; 0 where lo == hi, one ulp16 otherwise).  No share of outliers
is allowed anywhere.  eb = g_p u for p;  (3 + 2.5 |K - m_j|) u for P;  for an element of the activated tile the interval
is ref -+ its fp32 bound (`decided` of rowops_bounds is the same statement).

ROUNDING POINTS (the contract; the kernel lines they restate are quoted).
Context build, ctx16_mfma_kernel.  Rows in chunks of 64, m_j = running column maximum over the live rows through chunk j
(exact, so the reference knows it), rows >= len = clamp(length[b], 0, rows) masked:
    "pe[c] = (r0 + rr < len) ? __expf(kreg[i][c] - mrun[c]) : 0.f;  ksum[c] += pe[c];"     the denominator: UNROUNDED weights
    "... = bf16x4{(__bf16)pe[0], ...}"                                                     P_j = bf16(exp(K - m_j))
    "sc[c] = mrun[c] == -INFINITY ? 0.f : __expf(mrun[c] - m);  ksum[c] *= sc[c];  acc[bi][bj][e] *= f;"   the rescale
    "sScale[tid] = t > 0.f ? 1.0f / t : 0.f;  ... acc[bi][bj][4 * q] * inv"                A = numerator / denominator
  numerator = sum_j exp(m_j - m_final) sum_{r in j} P_j[r][c] V[r][l].  kstat = (m_final, denominator), (0, 1) at len 0,
  the maximum bit-equal to fp64, the sum within g_Z u.  At16 = at16_order of the kernel's own A, bit for bit
  ("At16[...hig_at16_offset(HD, l, cc)] = (__bf16)(acc[bi][bj][e] * inv)": the fp32 value that A received).
  Tier 2:  g_A u M2 + FLOOR + sum_undecided gap16(P) |V| exp(m_j - m_final) / denominator,   M2 = the numerator's M / denominator.
  Tier 1:  1.01 (u16 + g_A u) MA + FLOOR,  MA = sum_r k |V| (1.01: the products u16 g_A u of the two relative terms).
  PADDED ROWS: K and V rows at and beyond length[b] are never used ("min(r0 + row, max(len - 1, 0)) * ld" clamps the DMA to
  row len - 1, `read_k` masks by r0 + rr < len): the generators put the NaN pattern there.
Apply, apply_sty16_kernel.
    "const f32x2 pp = v[ks][e] * inv;  pfs[hh][ks][2 * e] = (__bf16)pp[0];"                p16 = bf16(softmax_hd(q))
    "acc[hh][lb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[hh][lb][ks], pfs[hh][ks], ..." y = sum_c p16[c] At16[l][c]
    "s1 += y;  s2 = __builtin_elementwise_fma(y, y, s2);"  "mean = t12[0] * (1.0f / D_)"   mean = sum y / d
    "rstd = rsqrtf(fmaxf(t12[1] * (1.0f / D_) - mean * mean, 0.f) + 1e-5f)"                var = max(sum y^2 / d - mean^2, 0)
    "sPar[c] = g * sc;  sPar[D_ + c] = fmaf(be, sc, sh);"  (sc = 1.0f + scale)             gamma' = gamma (1 + scale), beta'
    "u = fma(y, rs2, nm2);  x = fma(u, g4, b4)"  (nm2 = -mean * rstd)                      x = fma(fma(y, rstd, -mean rstd), gamma', beta')
    "w = x * -LOG2E;  den = exp2f(w) + 1.0f;  o = x * rcpf(den)"                           out = bf16(x / (1 + exp2(-x log2 e)))
    "bf16x4{(__bf16)acc[hh][lb][4 * q], ..."                                               Yout = bf16(y)
  y:  tier 2  hd u My2 + sum_undecided gap16(p) |At|;   tier 1  1.01 (u16 + g_y u) My.
Out-projection, out_gemm_rows (GEMM = true instance and rows_out16_kernel).
    "acc2[cb][4 * q] = b4.x ..."  the bias is the accumulator's initial value;  32 k-steps of 16 = 512 products of the
    bf16 activated tile a16 with W[j][r];  "v0 = acc2[cb][4 * q] + bf_lo(rq.x) ... (__bf16)v0"  h' = bf16(h + acc).
    h' tier 2:  1.01 (513 u (|bias| + sum |a16 W|) + u |h + acc|) + sum_undecided gap16(a) |W[j][r]|   (+ ulp16 / 2, `bound16`)
    h' tier 1:  1.01 (sum_r (e_a + u16 |a|) |W[j][r]| + 513 u M + u |.|) + u16 |ref|,  e_a the tier-1 fp32 bound of the tile.
    stats = hig_panel_stats16 of the bits of h' THE KERNEL WROTE, per 128-column panel: s1 = sum x within 128 u sum |x|;
    m2 = sum (x - s1 / 128)^2 within 2 d_mu sum |d| + 128 d_mu^2 + 131 u sum d^2, d_mu = 129 u mean |x| (ln_fwd_terms' d_mu).
rows_out16_kernel computes its LayerNorm CENTRED, unlike the apply:
    "mean = wave_sum(s) * (1.0f / D_);  dlt = v[e] - mean;  q = fmaf(dlt, dlt, q);  rstd = rsqrtf(wave_sum(q) * (1.0f / D_) + 1e-5f)"
    "o[e] = (__bf16)hig_silu_fast(fmaf((v[e] - mean) * rstd, gp[e], bp[e]))"     with the same gamma' / beta'.
  Its statistics are `ln_fwd_terms` of rowops_bounds (d_mu, rho) on the bf16 rows Y, an input: tier 1 and tier 2 differ only
  in the activated tile.

PROPAGATION THROUGH LAYERNORM (`sty_chain`).  y carries the error e (tier 1 or tier 2), d = y - mean, r = (var + eps)^-1/2.
A ROW SUM is counted by the DEPTH h of the kernel's own summation (`apply_row_depth`: 8 hd / 32 + 2 + H = 22 .. 42;
`ROWS_OUT_DEPTH` = 14), as rowops_bounds does for hig_ln_bwd_bf16 and for the same reason: under the linear n = d <= 1024 the
statistics alone leave fewer than 70 % of an ordinary case decided and the exactness check would hardly bite.  The fp32
evaluation that the CPU test holds to it sums rows pairwise (depth <= 10).
    d_mu = mean e + (h + 1) u mean |y|
    the variance the kernel would get in exact arithmetic from its own y is var(y + e) = var + 2 mean(d e) + var(e), off by at
    most 2 mean(|d| e) + mean(e^2)  (exact: no second-order term is dropped; first order this is the
    |xhat_i| r^2 mean_j(|d_j| e_j) of the rstd error).
    ONE-PASS FORM (apply): sum y^2 / d costs (h + 2) u E[y^2]; mean^2 carries 2 (h + 1) u |mean| mean |y| + u mean^2, and
    2 |mean| mean |y| <= E[y^2] + mean^2; the difference and + eps 2 u (var + eps): together at most
        (2 h + 6) u (E[y^2] + mean^2) = (2 h + 6) u kappa (var + eps),      kappa = (E[y^2] + mean^2) / (var + eps)
    (x 1.02: the sums are those of y + e, |e| <= 2^-7 |y| in either tier).  kappa stays in the bound: ~2 on ordinary rows,
    ~2 (mean / std)^2 on the "offset" kind -- this is where the one-pass form loses digits and the bound says how many.
    CENTRED FORM (rows_out16): ln_fwd_terms' rho, no kappa.
    D = the sum of those, relative to var + eps.  r is then off by the factor (1 + delta)^-1/2, |delta| <= D, and BECAUSE OF
    THE CLAMP AT 0 the computed r never exceeds eps^-1/2:
        rho = max( min((1 - D)^-1/2, ((var + eps) / eps)^1/2) - 1,  1 - (1 + D)^-1/2 ) + 2 u      (v_rsq: 2 u)
    which is finite on constant rows, where D is not small (without the clamp it is not: the `no_clamp` mutant).
    xhat = fma(y, r, -mean r):  e_xh = (1 + rho) r (e + d_mu + 2 u |mean|) + |xhat| (rho + 2 u)      (centred: u |d| for 2 u |mean|)
    x = fma(xhat, gamma', beta'):  e_x = |gamma'| e_xh + 3 u |xhat gamma'| + u |beta (1 + scale)| + u |beta'| + u |x|
    silu:  1.1 e_x + |silu| ((2 + 2.5 |x|) (1 - sigma) + 4) u     (|silu'| <= 1.1 globally, so no second order; G = 4 as hig_silu_fast)
    The products of two error terms are carried ((1 + rho), mean(e^2)); what is left is O(u^2 kappa) in tier 2 and O(u16^2)
    in tier 1 from the 1.02 above and is covered by a final factor 1.01.

bf16 OUTPUTS (Out, Yout, h') are held by bound16(ref, bound32) with bound32 the tier-2 bound, and bit for bit (exact16) on the
elements decided(ref, bound32) marks; at least MIN_DECIDED of an ordinary case's elements are decided, from the reference
alone.  The "const" and "offset" kinds are exempt, as "const" is in the row-op contract: their bound is not small against
an ulp by construction (kappa).

WHICH INSTANCE A SHAPE REACHES (host code of csrc/linattn16.hip):
    hig_linattn_ctx_mm16:  "if (hd == 64 && nb2_from > 0 && B * H >= nb2_from)" (nb2_from = 512) -> ctx16_mfma_kernel<64, 2>;
                           "else if (hd == 64)" -> <64, 3>;  else <128, 3>.
    hig_linattn_apply_sty_mm16[_y]:  "if (hd == 64 && H == 8) HIG_AP16(64, 8, 8); else if (hd == 64) HIG_AP16(64, 4, 4); else if
                           (H == 8) HIG_AP16(128, 8, 8); else HIG_AP16(128, 4, 4);", each "<.., false, true>" when Yout is given.
    hig_attn_out16:  apply_sty16_kernel<64, 8, 8, true>;   hig_rows_out16:  rows_out16_kernel;   both d = 512 only.
    hig_weight_frag16:  "blocks = (n + 255) / 256; if (blocks > 2048) blocks = 2048": more than 524288 16-byte pieces take a
                           second trip of the grid-stride loop ((2080, 2048): 532480).
"""
import math

import torch

import rowops_bounds as rb
from rowops_bounds import BF16, EPS, F32, F64, U
from test_gpu_attn_contract import at16_order  # noqa: F401  (re-exported; the module runs nothing on import)

U16 = 2.0 ** -8
FLOOR = 2.0 ** -120     # as in test_gpu_attn_contract.py
CH = 64
NAN = float("nan")


# ----------------------------------------------------------------------------------------------------------------------
# bf16 rounding of fp64 values (torch rounds fp64 -> fp32 -> bf16, twice; the reference needs the one correct rounding)
# ----------------------------------------------------------------------------------------------------------------------
def rne16(x):
    """fp64 -> the nearest bf16 value (ties to even), returned as fp64.  Exact: x / q is a scaling by a power of two."""
    _, ex = torch.frexp(x)                                  # |x| in [2^(ex - 1), 2^ex)
    q = torch.exp2((ex - 8).clamp_min(-133).double())       # the spacing of bf16 in that binade
    return torch.round(x / q) * q


def rnd16(x):
    """The bf16 rounding an evaluation in dtype x.dtype performs: exact for fp64, the hardware conversion for fp32."""
    return rne16(x) if x.dtype == F64 else x.to(BF16).to(x.dtype)


def gap16(x, eb_rel=None, eb_abs=None):
    """hi - lo of the module docstring: the width of the set of bf16 values an operand within its bound of x can round to."""
    b = x.abs() * eb_rel if eb_abs is None else eb_abs
    return rne16(x + b) - rne16(x - b)


def gammas(T, hd, Xq=0.0, Xk=0.0):
    """The counts of test_gpu_attn_contract.py that these kernels need."""
    n = (T + CH - 1) // CH
    g_p = hd + 7 + 2.5 * (Xq + math.log(hd))
    g_Z = T + 2 + 2.5 * math.log(T) + 3 * (n + 1)
    return {"p": g_p, "y": g_p + hd, "Z": g_Z, "A": (2 + 2.5 * Xk + 3 * (n + 1)) + T + g_Z + 3}


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------------------------------
# context build
# ----------------------------------------------------------------------------------------------------------------------
def live_rows(lens, B, T, dev, le=False):
    ln = torch.full((B,), T, dtype=torch.int64, device=dev) if lens is None else lens.to(dev).clamp(0, T)
    r = torch.arange(T, device=dev)[None]
    return ln, ((r <= ln[:, None]) if le else (r < ln[:, None]))


def ctx_eval(K, V, lens, dtype=F64, mutant=None, want_bounds=False):
    """The context build at the kernel's rounding points: K, V (B, T, H, hd) bf16 values (rows >= length may hold NaN).
    -> A (B, H, hd, hd) [c][l], kmax, Z (B, H, hd); with want_bounds also (M2, allowance) of tier 2.  dtype F32: the fp32
    emulation (chunked online softmax, P rounded to bf16, fp32 accumulation)."""
    B, T, H, hd = K.shape
    dev = K.device
    K, V = K.to(dtype), V.to(dtype)
    ln, live = live_rows(lens, B, T, dev, le=mutant == "mask_includes_row_len")
    num = torch.zeros(B, H, hd, hd, dtype=dtype, device=dev)
    M2, allow = torch.zeros_like(num), torch.zeros_like(num)
    zs = torch.zeros(B, H, hd, dtype=dtype, device=dev)
    m = torch.full((B, H, hd), float("-inf"), dtype=dtype, device=dev)
    for j, r0 in enumerate(range(0, T, CH)):
        r1 = min(r0 + CH, T)
        dead = ~live[:, r0:r1, None, None]
        Kc, Vc = K[:, r0:r1].masked_fill(dead, float("-inf")), V[:, r0:r1].masked_fill(dead, 0.0)
        mc = torch.maximum(m, Kc.amax(1))
        sc = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - mc))
        if mutant == "rescale_skipped_for_chunk_1" and j == 1:
            sc = torch.ones_like(sc)
        x = (Kc - mc[:, None]).masked_fill(dead, 0.0)
        E = torch.exp(x).masked_fill(dead, 0.0)
        Pq = rnd16(E)
        zs = zs * sc + (Pq if mutant == "denominator_from_rounded_weights" else E).sum(1)
        Pn = Pq
        if mutant == "last_partial_kstep_dropped":          # rows 16 floor(len / 16) .. len - 1 never reach the matrix cores
            rr = torch.arange(r0, r1, device=dev)[None]
            Pn = Pq.masked_fill((rr >= (ln // 16 * 16)[:, None])[:, :, None, None], 0.0)
        num = num * sc[..., None] + torch.einsum("brhc,brhl->bhcl", Pn, Vc)
        if want_bounds:
            gp = gap16(E, (3 + 2.5 * x.abs()) * U)
            allow = allow * sc[..., None] + torch.einsum("brhc,brhl->bhcl", gp, Vc.abs())
            M2 = M2 * sc[..., None] + torch.einsum("brhc,brhl->bhcl", Pq, Vc.abs())
        m = mc
    inv = torch.where(zs > 0, 1.0 / zs, torch.zeros_like(zs))
    some = (ln > 0)[:, None, None]
    A = num * inv[..., None]
    kmax, Z = torch.where(some, m, torch.zeros_like(m)), torch.where(some, zs, torch.ones_like(zs))
    if want_bounds:
        return A, kmax, Z, M2 * inv[..., None], allow * inv[..., None]
    return A, kmax, Z


def ctx_exact(K, V, lens):
    """The definition: A = softmax_r(K)^T V over the live rows, in fp64 -> A, MA, kmax, Z, Xk."""
    B, T, H, hd = K.shape
    ln, live = live_rows(lens, B, T, K.device)
    dead = ~live[:, :, None, None]
    Km, Vm = K.double().masked_fill(dead, float("-inf")), V.double().masked_fill(dead, 0.0)
    kmax = Km.amax(1).nan_to_num(neginf=0.0)
    x = (Km - kmax[:, None]).masked_fill(dead, 0.0)
    e = torch.exp(x).masked_fill(dead, 0.0)
    Z = e.sum(1)
    k = e / Z.clamp_min(1e-300)[:, None]
    some = (ln > 0)[:, None, None]
    return (torch.einsum("brhc,brhl->bhcl", k, Vm), torch.einsum("brhc,brhl->bhcl", k, Vm.abs()), kmax,
            torch.where(some, Z, torch.ones_like(Z)), x.abs().max().item())


def ctx_bounds(K, V, lens, u16=U16, allowance=True):
    """{'A1' | 'A2' | 'Z': (ref, bound), 'kmax': ref, 'Xk'}."""
    T, hd = K.shape[1], K.shape[3]
    A1, MA, kmax, Z, Xk = ctx_exact(K, V, lens)
    g = gammas(T, hd, Xk=Xk)
    A2, kmax2, Z2, M2, allow = ctx_eval(K, V, lens, want_bounds=True)
    assert torch.equal(kmax, kmax2)
    return {"A1": (A1, 1.01 * (u16 + g["A"] * U) * MA + FLOOR), "A2": (A2, g["A"] * U * M2 + FLOOR + (allow if allowance else 0.0)),
            "Z": (Z, g["Z"] * U * Z), "kmax": kmax, "Xk": Xk, "g": g}


def ctx_lengths(B, rows):
    """0, 1, rows, rows + 5, a multiple of 16, a multiple of 16 plus 1, 64 and 65, wherever rows allows, over the batch."""
    m16 = (rows - 1) // 16 * 16                 # the largest multiple of 16 below rows
    pat = [0, 1, rows, rows + 5] + [v for v in (m16, m16 + 1, 64, 65) if 1 < v < rows]
    pat = list(dict.fromkeys(pat))
    return torch.tensor([pat[i % len(pat)] for i in range(B)], dtype=torch.int64)


def ctx_case(B, rows, H, hd, seed, spread=15.0, lens="pattern"):
    """K, V (B, rows, H, hd) bf16 -- K with a logit spread of about `spread` (clipped at +-spread / 2), V with mean 0.5 --
    and lengths; rows at and beyond length[b] hold NaN."""
    g = gen(seed)
    K = (torch.randn(B, rows, H, hd, generator=g) * (spread / 6)).clamp_(-spread / 2, spread / 2).to(BF16)
    V = (torch.randn(B, rows, H, hd, generator=g) + 0.5).to(BF16)
    ln = ctx_lengths(B, rows) if lens == "pattern" else None
    if ln is not None:
        dead = torch.arange(rows)[None] >= ln[:, None]
        K[dead], V[dead] = NAN, NAN
    return K, V, ln


# (hd, B, H, rows, lengths, At16): <64, 3>: B H < 512, H in {1, 3, 8};  <64, 2>: B H >= 512;  <128, 3>: H in {1, 4}
CTX_ROWS = (1, 15, 16, 17, 63, 64, 65, 129, 197)


def ctx_cases():
    for i, rows in enumerate(CTX_ROWS):
        for H in (1, 3, 8):
            yield 64, 8, H, rows, True, (i + H) % 2 == 0
        for H in (1, 4):
            yield 128, 8, H, rows, True, (i + H) % 2 == 1
    yield 64, 3, 8, 197, False, True            # length NULL
    yield 128, 2, 4, 129, False, False
    yield 64, 64, 8, 197, True, True            # B H = 512: the two-buffer ring
    yield 64, 8, 64, 197, True, False
    yield 64, 64, 8, 17, True, True


def ctx_id(c):
    return "hd%d_B%d_H%d_r%d_%s_%s" % (c[0], c[1], c[2], c[3], "len" if c[4] else "nolen", "at16" if c[5] else "noat16")


def ctx_spread(rows, H):
    return 40.0 if (rows + H) % 2 else 15.0


# ----------------------------------------------------------------------------------------------------------------------
# apply + stylization front
# ----------------------------------------------------------------------------------------------------------------------
def modulation(ss, d, B, rows, dtype, mutant=None):
    """(1 + scale, shift) per row, (B, rows, d): ss (B, >= 4 d) with scale at column 2 d and shift at 3 d."""
    b = torch.arange(B, device=ss.device)
    if mutant == "modulation_of_sample_b_minus_1":
        b = (b - 1) % B
    s = ss.to(dtype)[b]
    sc, sh = s[:, 2 * d:3 * d], s[:, 3 * d:4 * d]
    if mutant == "shift_read_at_offset_0":
        sh = sc
    one = torch.ones((), dtype=dtype, device=ss.device)
    return (one + sc)[:, None].expand(B, rows, d), sh[:, None].expand(B, rows, d)


def silu_front(y, gamma, beta, sc1, sh, dtype, one_pass=True, mutant=None):
    """x / (1 + exp(-x)), x = fma(xhat, gamma', beta') with the statistics in the form the kernel has them."""
    shape, d = y.shape, y.shape[-1]
    y = y.reshape(-1, d)
    sc1, sh = sc1.reshape(-1, d), sh.reshape(-1, d)
    # pairwise sums: the depth-counted bound is held to a tree, as in rowops_bounds.  The mutant without the clamp sums in
    # torch's own order: a pairwise tree over the equal values of a constant row is exact and would hide what the clamp is for.
    tree = mutant != "variance_not_clamped"
    mean = rb.rowsum(y, tree) / d
    if one_pass and mutant != "centred_variance":
        var = rb.rowsum(y * y, tree) / d - mean * mean
        if mutant != "variance_not_clamped":
            var = var.clamp_min(0.0)
        rstd = (var + EPS) ** -0.5
        xhat = y * rstd - mean * rstd
    else:
        dl = y - mean
        rstd = (rb.rowsum(dl * dl, tree=True) / d + EPS) ** -0.5
        xhat = dl * rstd
    g1 = gamma.to(dtype) * (1 if mutant == "gamma_without_one_plus_scale" else sc1)
    x = xhat * g1 + (beta.to(dtype) * sc1 + sh)
    return (x * torch.sigmoid(x)).reshape(shape)


def apply_eval(q, At, gamma, beta, ss, B, rows, H, hd, dtype=F64, mutant=None, round_p=True):
    """(out, y) before their bf16 roundings, (B rows, d): q (B rows, d) bf16, At (B, H, hd, hd) [l][c] bf16.  round_p False:
    the definition (tier 1); True: the kernel's rounding point.  dtype F32: the fp32 emulation."""
    d = H * hd
    qv = q.to(dtype).view(B, rows, H, hd)
    e = torch.exp(qv - qv.amax(-1, keepdim=True))
    if mutant == "row_sum_over_one_lane_half":          # lanes lr and lr + 32 hold alternate groups of 8 channels
        half = (torch.arange(hd, device=q.device) // 8) % 2 == 0
        p = e / (e * half).sum(-1, keepdim=True)
    else:
        p = e / e.sum(-1, keepdim=True)
    if round_p:
        p = rnd16(p)
    y = torch.einsum("bnhc,bhlc->bnhl", p, At.to(dtype)).reshape(B, rows, d)
    sc1, sh = modulation(ss, d, B, rows, dtype, mutant)
    out = silu_front(y, gamma, beta, sc1, sh, dtype, True, mutant)
    return out.reshape(B * rows, d), y.reshape(B * rows, d)


def apply_row_depth(hd, H):
    """A row sum of apply_sty16_kernel (sum y, sum y^2): a lane's packed `s1 += y` over its hd / 32 column blocks of 8 pairs,
    s1[0] + s1[1], the lane pair, then the H waves (one head per wave in all four instances) in sequence."""
    return 8 * (hd // 32) + 2 + H


ROWS_OUT_DEPTH = 8 + 6      # rows_out16_kernel: 8 sequential fmas of a lane (the mean: a tree of depth 3), the 6-level wave sum


def sty_chain(y, e, gamma, beta, sc1, sh, one_pass, hrow):
    """`PROPAGATION THROUGH LAYERNORM` of the module docstring: (out, bound32, kappa per row) for rows y (R, n) fp64 carrying
    the error e (a tensor like y, or 0.0)."""
    n = y.shape[-1]
    gamma, beta = gamma.double(), beta.double()
    e = torch.zeros_like(y) + e
    mu, d, r, d_mu0, rho0 = rb.ln_fwd_terms(y, hrow)
    var = (d * d).mean(-1, keepdim=True)
    first = (2 * (d.abs() * e).mean(-1, keepdim=True) + (e * e).mean(-1, keepdim=True)) / (var + EPS)
    E2 = (y * y).mean(-1, keepdim=True)
    kappa = (E2 + mu * mu) / (var + EPS)
    d_mu = e.mean(-1, keepdim=True) + d_mu0
    D = first + (1.02 * (2 * hrow + 6) * U * kappa if one_pass else 2 * rho0)
    up = torch.minimum(torch.where(D < 1, (1 - D.clamp_max(1 - 1e-12)) ** -0.5, torch.full_like(D, float("inf"))), ((var + EPS) / EPS) ** 0.5) - 1
    rho = torch.maximum(up, 1 - (1 + D) ** -0.5) + 2 * U
    xh = d * r
    e_xh = (1 + rho) * r * (e + d_mu + (2 * U * mu.abs() if one_pass else U * d.abs())) + xh.abs() * (rho + 2 * U)
    g1, b1 = gamma * sc1, beta * sc1 + sh
    x = xh * g1 + b1
    e_x = g1.abs() * e_xh + 3 * U * (xh * g1).abs() + U * (beta * sc1).abs() + U * b1.abs() + U * x.abs()
    sg = torch.sigmoid(x)
    out = x * sg
    return out, 1.01 * (1.1 * e_x + out.abs() * ((2 + 2.5 * x.abs()) * (1 - sg) + 4) * U), kappa[..., 0]


def apply_bounds(q, At, gamma, beta, ss, B, rows, H, hd, u16=U16, allowance=True):
    """{'y1', 'out1' (tier 1: ref, bound of the bf16 output), 'y2', 'out2' (tier 2: ref, bound32 before the output rounding),
    'kappa', 'und' (share of p undecided), 'Xq'}."""
    d = H * hd
    qv = q.double().view(B, rows, H, hd)
    Xq = (qv.amax(-1) - qv.amin(-1)).max().item()
    assert Xq <= 80
    g = gammas(rows, hd, Xq=Xq)
    Atd = At.double()
    p = torch.softmax(qv, -1)
    sc1, sh = modulation(ss, d, B, rows, F64)
    sc1, sh = sc1.reshape(B * rows, d), sh.reshape(B * rows, d)
    res = {"Xq": Xq, "g": g}
    # tier 1
    y1 = torch.einsum("bnhc,bhlc->bnhl", p, Atd).reshape(B * rows, d)
    My = torch.einsum("bnhc,bhlc->bnhl", p, Atd.abs()).reshape(B * rows, d)
    e1 = 1.01 * (u16 + g["y"] * U) * My
    out1, b1, _ = sty_chain(y1, e1, gamma, beta, sc1, sh, True, apply_row_depth(hd, H))
    res["y1"], res["out1"], res["e_out1"] = (y1, e1 + u16 * y1.abs()), (out1, b1 + u16 * out1.abs()), b1
    # tier 2
    p16 = rne16(p)
    gp = gap16(p, g["p"] * U)
    y2 = torch.einsum("bnhc,bhlc->bnhl", p16, Atd).reshape(B * rows, d)
    My2 = torch.einsum("bnhc,bhlc->bnhl", p16, Atd.abs()).reshape(B * rows, d)
    e2 = hd * U * My2 + FLOOR
    if allowance:
        e2 = e2 + torch.einsum("bnhc,bhlc->bnhl", gp, Atd.abs()).reshape(B * rows, d)
    out2, b2, kappa = sty_chain(y2, e2, gamma, beta, sc1, sh, True, apply_row_depth(hd, H))
    res["y2"], res["out2"], res["kappa"], res["und"] = (y2, e2), (out2, b2), kappa, (gp != 0).double().mean().item()
    return res


def apply_case(kind, B, rows, H, hd, seed):
    """q (B rows, d) bf16, At (B, H, hd, hd) [l][c] bf16, gamma, beta (d), ss (B, 6 d + 4) fp32.
    'ordinary15' / 'ordinary40': logit spread of q about 15 / 40, At = 0.3 + randn.
    'peaked40': the spread-15 logits with one channel per (row, head) raised by 25: p is 1 - O(1e-6) there and below 5e-5
    elsewhere, so no significant weight is undecided (the kind on which h' of hig_attn_out16 must reach MIN_DECIDED).
    'offset10' / 'offset100': At = randn + a common offset chosen so that |mean| / std of the rows y is about 10 / 100.
    'const': At = 48 everywhere; every second row of q is constant (p = 1 / hd exactly: y = 48 exactly, variance 0)."""
    d = H * hd
    g = gen(seed)
    spread = 40.0 if kind == "ordinary40" else 15.0
    q = (torch.randn(B * rows, d, generator=g) * (spread / 6)).clamp_(-spread / 2, spread / 2)
    At = torch.randn(B, H, hd, hd, generator=g)
    if kind == "peaked40":
        qv = q.view(B * rows, H, hd)
        rr, hh = torch.meshgrid(torch.arange(B * rows), torch.arange(H), indexing="ij")
        qv[rr, hh, (rr + 5 * hh) % hd] += 25.0
    if kind.startswith("ordinary") or kind == "peaked40":
        At = At + 0.3
    elif kind.startswith("offset"):
        p = torch.softmax(q.to(BF16).double().view(B, rows, H, hd), -1)
        y = torch.einsum("bnhc,bhlc->bnhl", p, At.double()).reshape(B * rows, d)
        At = At + float(kind[6:]) * y.std(-1).median().item()
    else:
        At = torch.full_like(At, 48.0)
        q[1::2] = 0.5
    gamma = 1 + 0.1 * torch.randn(d, generator=g)
    beta = 0.1 * torch.randn(d, generator=g)
    ss = 0.3 * torch.randn(B, 6 * d + 4, generator=g)
    return q.to(BF16), At.to(BF16), gamma, beta, ss


APPLY_KINDS = ("ordinary15", "ordinary40", "peaked40", "offset10", "offset100", "const")
OUT_KINDS = ("peaked40",) + tuple(k for k in APPLY_KINDS if k != "peaked40")
APPLY_INSTANCES = ((64, 8), (64, 4), (128, 8), (128, 4))      # (hd, H)
APPLY_ROWS = (1, 31, 32, 33, 70)
APPLY_B = (1, 3)


def apply_cases():
    """(hd, H, B, rows, kind): both ordinary kinds at every shape, the other kinds at (3, 70) and (1, 33)."""
    for hd, H in APPLY_INSTANCES:
        for B in APPLY_B:
            for rows in APPLY_ROWS:
                yield hd, H, B, rows, "ordinary15" if (rows + B) % 2 else "ordinary40"
        for kind in APPLY_KINDS:
            yield hd, H, 3, 70, kind
        for kind in APPLY_KINDS[1:]:
            yield hd, H, 1, 33, kind


def need_decided(kind, out_projection=False):
    """The kinds whose bf16 outputs must reach MIN_DECIDED.  Behind the fused out-projection 'ordinary15' is exempt: a flip of
    one significant softmax weight moves the mean of its whole row, so with ~15 significant weights per head 15 % of the
    activated tile and with it 40 % of h' is legitimately undecided (tests/test_cpu_linattn16_bounds.py prints the shares)."""
    return kind in ("peaked40", "ordinary40") or (kind == "ordinary15" and not out_projection)


# ----------------------------------------------------------------------------------------------------------------------
# out-projection: h' = bf16(h + bias + a16 W^T), stats
# ----------------------------------------------------------------------------------------------------------------------
def panel_stats(h16):
    """(sum, centred sum of squares) per 128-column panel of the rows h16 (R, 512), in fp64 -> (R, 4, 2)."""
    x = h16.double().view(h16.shape[0], -1, 128)
    s = x.sum(-1)
    dl = x - s[..., None] / 128
    return torch.stack([s, (dl * dl).sum(-1)], -1)


def panel_stats_bound(h16):
    x = h16.double().view(h16.shape[0], -1, 128)
    s = x.sum(-1)
    dl = x - s[..., None] / 128
    d_mu = 129 * U * x.abs().mean(-1)
    return torch.stack([128 * U * x.abs().sum(-1), 2 * d_mu * dl.abs().sum(-1) + 128 * d_mu * d_mu + 131 * U * (dl * dl).sum(-1)], -1)


def outproj_eval(a, W, bias, h, dtype=F64, mutant=None, round_a=True):
    """(h' before its rounding, stats of the rounded h') from the activated tile a (R, 512) before ITS rounding."""
    a, W, bias, h = a.to(dtype), W.to(dtype), bias.to(dtype), h.to(dtype)
    a16 = rnd16(a) if round_a else a
    if mutant == "bias_added_after_the_rounding":
        v = rnd16(h + a16 @ W.t()) + bias
    else:
        v = h + (bias + a16 @ W.t())
    if mutant == "residual_read_from_the_updated_tile":
        v = rnd16(v) + (bias + a16 @ W.t())
    st = panel_stats(v if mutant == "stats_before_the_rounding" else rnd16(v))
    if mutant == "stats_of_panel_p_plus_1":
        st = torch.roll(st, -1, 1)
    return v, st.to(dtype)


def outproj_bounds(a1, e_a1, a2, e_a2, W, bias, h, u16=U16):
    """{'h1': (ref, bound of the bf16 output), 'h2': (ref, bound32)} from the tile's tier-1 / tier-2 references and fp32 bounds."""
    Wd, bd, hd_ = W.double(), bias.double(), h.double()
    Wa = Wd.abs().t()
    v1 = hd_ + (bd + a1 @ Wd.t())
    M1 = bd.abs() + a1.abs() @ Wa
    b1 = 1.01 * ((e_a1 + u16 * a1.abs()) @ Wa + 513 * U * M1 + U * v1.abs()) + u16 * v1.abs()
    a16 = rne16(a2)
    gp = gap16(a2, eb_abs=e_a2)
    v2 = hd_ + (bd + a16 @ Wd.t())
    M2 = bd.abs() + a16.abs() @ Wa
    b2 = 1.01 * (513 * U * M2 + U * v2.abs()) + gp @ Wa
    return {"h1": (v1, b1), "h2": (v2, b2), "und": (gp != 0).double().mean().item()}


def out_params(seed, d=512):
    """W (d, d) bf16 around d^-1/2, bias (d) fp32."""
    g = gen(seed)
    return (torch.randn(d, d, generator=g) * d ** -0.5).to(BF16), 0.1 * torch.randn(d, generator=g)


def residual(R, seed, d=512):
    """h around 2 in magnitude, either sign: +-(2 + randn / 4).  (|h'| then stays in [1, 4), where half a bf16 ulp is large
    against the 512-term bound: 2 randn would put 40 % of h' below 1 and leave fewer than MIN_DECIDED decided.)"""
    g = gen(seed)
    mag = 2 + 0.25 * torch.randn(R, d, generator=g)
    return (mag * (2 * torch.randint(0, 2, (R, d), generator=g) - 1)).to(BF16)


def attn_out_bounds(q, At, gamma, beta, ss, W, bias, h, B, rows):
    ab = apply_bounds(q, At, gamma, beta, ss, B, rows, 8, 64)
    res = outproj_bounds(ab["out1"][0], ab["e_out1"], ab["out2"][0], ab["out2"][1], W, bias, h)
    res["kappa"] = ab["kappa"]
    return res


def rows_case(kind, B, rows, seed, d=512):
    """Y (B rows, d) bf16, gamma, beta, ss.  'ordinary': 0.3 + randn; 'offset10' / 'offset100': 10 / 100 + randn; 'const':
    rows_input('const') of rowops_bounds."""
    g = gen(seed)
    R = B * rows
    if kind == "const":
        Y = rb.rows_input("const", R, d, g)
    else:
        Y = torch.randn(R, d, generator=g) + (0.3 if kind == "ordinary" else float(kind[6:]))
    gamma = 1 + 0.1 * torch.randn(d, generator=g)
    beta = 0.1 * torch.randn(d, generator=g)
    ss = 0.3 * torch.randn(B, 6 * d + 4, generator=g)
    return Y.to(BF16), gamma, beta, ss


def rows_front(Y, gamma, beta, ss, B, rows, dtype=F64, mutant=None):
    d = Y.shape[1]
    sc1, sh = modulation(ss, d, B, rows, dtype, mutant)
    return silu_front(Y.to(dtype).view(B, rows, d), gamma, beta, sc1, sh, dtype, False, mutant).reshape(B * rows, d)


def rows_out_bounds(Y, gamma, beta, ss, W, bias, h, B, rows):
    d = Y.shape[1]
    sc1, sh = modulation(ss, d, B, rows, F64)
    a, e_a, _ = sty_chain(Y.double(), 0.0, gamma, beta, sc1.reshape(B * rows, d), sh.reshape(B * rows, d), False, ROWS_OUT_DEPTH)
    return outproj_bounds(a, e_a, a, e_a, W, bias, h)


OUT_ROWS = (1, 33, 70)
OUT_B = (1, 3)
ROWS_KINDS = ("ordinary", "offset10", "offset100", "const")


def out_cases(kinds):
    """(B, rows, kind, stats): the ordinary kind at every shape, the others at (3, 70)."""
    for i, B in enumerate(OUT_B):
        for j, rows in enumerate(OUT_ROWS):
            yield B, rows, kinds[0], (i + j) % 2 == 0
    yield 3, 70, kinds[0], False
    for kind in kinds[1:]:
        yield 3, 70, kind, True


# ----------------------------------------------------------------------------------------------------------------------
# hig_weight_frag16
# ----------------------------------------------------------------------------------------------------------------------
FRAG_SHAPES = ((32, 16, 16), (64, 48, 48), (512, 512, 520), (2080, 2048, 2048))      # (J, R, ldy)


def weight_frag(Y):
    """Y_frag[((j / 32) (R / 16) + r / 16) 512 + (j % 32 + 32 ((r % 16) / 8)) 8 + r % 8] = Y[j][r]  (include/hig.h)."""
    J, R = Y.shape
    return Y.reshape(J // 32, 32, R // 16, 2, 8).permute(0, 2, 3, 1, 4).reshape(-1)


def weight_frag_index(J, R, j, r):
    return ((j // 32) * (R // 16) + r // 16) * 512 + (j % 32 + 32 * ((r % 16) // 8)) * 8 + r % 8
