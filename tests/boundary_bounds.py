"""fp64 references, element-wise bounds and the case tables of the kernels on either side of the denoiser: the two-person
loss hig_pair_mse (csrc/ddpm.hip), the joint recovery hig_recover_joints and the batch assembly hig_gather_frames
(csrc/pipeline.hip), the timestep embedding hig_timestep_embedding[_bf16] (csrc/rowops.hip).  Plain torch / numpy on the
host: tests/test_cpu_boundary_bounds.py proves without a GPU that the bounds reject wrong arithmetic and accept fp32,
tests/test_gpu_boundary_contract.py holds the kernels to them.

The rule and the counting conventions are those of tests/rowops_bounds.py: u = 2^-24, a result differs from its fp64 value by
at most gamma u M, gamma a count of roundings, M the expression with every term replaced by its absolute value.  n roundings
in sequence are counted as gam(n) = n u / (1 - n u).  Every `*_eval` states an operation once, for any dtype and with an
optional `mutant`; the reference is its fp64 evaluation.  No bound below was fitted to a measurement.

hig_pair_mse (`pair_bound`).  live(r, t, f) = t < clamp(len_r, 0, T) and (t > 0 or f < 4); nf = 4 on token 0, F elsewhere.
  token    l[r][t] = sum_f (p - q)^2 / nf.  The difference rounds once, which its square doubles: 2; the square 1; a lane adds
           ceil(nf / 64) of them; wave_sum is 6 levels; the division 1:   g_tok = 3 + ceil(nf / 64) + 6 + 1, relative to l (all
           terms are non-negative, so M is the value itself).
  rowloss  a wave adds the tokens t = w, w + 4, ..: at most ceil(len / 4) adds; (w0 + w1) + (w2 + w3): 2.
           b_row[r] = sum_t gam(g_tok(t) + ceil(len_r / 4) + 2) l[r][t]
  loss     sum over the chosen rows (PIT: S = L[a] + L[b] first, 1) by one block: ceil(n / 256) adds per thread (n = P under
           PIT, R without), 8 tree levels, the division by denom: k = pit + ceil(n / 256) + 8 + 1.  The token count is a sum of
           integers below 2^24 and its half: exact in fp32 (asserted), so denom carries nothing.
           b_loss = (sum_chosen b_row (1 + gam(k)) + gam(k) sum_chosen L) / denom
  rowscale 1 / denom, one correctly rounded division of an exact denominator: the kernel's value must be that fp32 number bit
           for bit, or 0 on a row of the unchosen assignment.
  dpred    rowscale 2 (p - q) / nf: the rounding rowscale inherits from 1 / denom, the difference, the product (2 is exact), the
           division: gam(4) |dpred|; exactly 0 wherever live is false and on every row whose rowscale is 0.
  PIT      S0 = L[p] + L[2P + p], S1 = L[P + p] + L[3P + p].  margin = |S0 - S1| / (the four rows' b_row + u (S0 + S1), the
           rounding of the two sums).  A pair is DECIDED when margin > 4: no rounding the bound admits can turn the comparison.
           A pair is a TIE BY CONSTRUCTION when rows P + p and 3P + p are bitwise copies of rows p and 2P + p in pred, target and
           length: then S0 == S1 in any arithmetic and the kernel must take the first.  Every pair of every case is one or the
           other (the CPU test asserts it), so no pair is skipped.

hig_recover_joints (`recover_bound`).  Reference: oracle.motion_ref (denormalize_sample, recover_person) in fp64; `recover_eval`
restates it vectorised (the CPU test holds the two to 1e-12) so that it can carry mutants and run in fp32.
  feat     x sd + mean: two roundings, e = u (|x sd| + |v|) (a contracted fma rounds once: covered).  No stats: exact.
  yaw      ang_t = fp32(sum_{s < t} rot_s), accumulated in double: delta_t = sum_{s < t} e_rot_s + u |ang_t| (+ T 2^-53 sum |rot|).
  sinf, cosf  The ROCm install documents no ulp figure for the device library's sinf / cosf (no OCML document ships with it, the
           HIP headers state none), so the 4 ulp of OpenCL's full profile are used: 4 ulp = 8 u |v|:  e_c = 8 u (|c| + delta),
           e_s likewise, around the cosine and sine of the angle the kernel holds.
  qrot3    with q = (c, (0, -s, 0)) the cross products keep one product each (the others multiply a literal zero: exact):
              x' = vx + 2 (c (-s vz) + (-s)(s vx)),   y' = vy exactly,   z' = vz + 2 (c (s vx) + s (-s vz))
           A = c s vz: two products, gam(2) |A| + |s vz| e_c + |c vz| e_s + |c s| e_vz;  B = s^2 vx: gam(2) |B| + 2 |s vx| e_s +
           s^2 e_vx;  their sum u (|A| + |B|); the factor 2 is exact; the last sum u |x'|:
              e_x' = e_vx + 2 (e_A + e_B + u (|A| + |B|)) + u |x'|            (`roty_bound`; z' with the roles exchanged)
           (c, s) = (cos a, sin a) turns (vx, vz) by 2 a, so the angle's own error delta turns the result by 2 delta: x' moves by at
           most 2 delta |z'| + 2 delta^2 |v| (the chord's first and second order), z' by 2 delta |x'| + 2 delta^2 |v|.
  root     px_t = fp32(sum_{s <= t} wx_s) in double: sum_{s <= t} e_wx_s + u |px_t|; the height ry_t = feat: e_feat.
  joints   qrot3 of the local position, then + px: e_x' + e_px + u |sum|.
  init     qrot3 with c = q0w, s = -q0y (their error: e_feat of the init row, no sinf / cosf), then + ix: + e_ix + u |out|.
Every term is u (a count) (a magnitude of that element's own operands), so a joint near the origin gets a small bound.

hig_timestep_embedding (`temb_bound`).  Reference: cos / sin of t exp(-ln(10000) i / half) in fp64 (NOT the fp32 oracle).
  e        the kernel's constant is fp32(ln 10000), off by kappa u |e| (kappa = 0.23, computed below), its product with i and
           the division by half round once each: (2 + kappa) u |e| absolute (counting the two operations alone, 2 u |e|,
           would leave the constant's rounding out).
  arg      freq = fp32(exp(double(e))): the exponent's absolute error is freq's relative error, + 1 for its rounding; t is
           exact; the product 1; one spare for the double rounding of exp:  delta = u |arg| ((2 + kappa) |e| + 3)
  out      delta + 8 u (|v| + delta)      (4 ulp for sinf / cosf as above)
The bf16 entry adds half a bf16 ulp (`bound16`) and is exact where the fp32 bound decides the rounding (`exact16`).  For odd d
the last column is exactly 0.

hig_gather_frames is exact: numpy's own ((x - mean) / sd).astype(float32) with float32 or float64 statistics (`gather_eval`).

The largest error / bound ratios measured on an MI355X are tabulated in tests/test_gpu_boundary_contract.py.
"""
import math

import numpy as np
import torch

from rowops_bounds import U, F64, F32, BF16, ratio, bound16, exact16, decided, gen, cdiv  # noqa: F401

ULP4 = 8 * U        # 4 ulp of sinf / cosf


def gam(n):
    return n * U / (1 - n * U)


# ----------------------------------------------------------------------------------------------------------------------
# hig_pair_mse
# ----------------------------------------------------------------------------------------------------------------------
# (R, T, F, pit, lengths)
PAIR_SHAPES = ((4, 5, 4, 1, True),          # the smallest legal PIT
               (8, 7, 70, 1, True),         # F % 64 != 0; pair 0 a tie by construction
               (12, 9, 263, 1, True),
               (1028, 2, 4, 1, True),       # P = 257: a second trip of the select kernel's pair loop
               (259, 3, 5, 0, True),        # R > 256 and R % 4 != 0
               (6, 4, 130, 0, False),       # length = None
               (8, 250, 263, 0, True))      # 526 000 elements > 2048 x 256 threads: pair_grad_kernel loops twice
PAIR_TIE = {(8, 7, 70): 0}                  # shape -> the pair that is a tie by construction
PAIR_MARGIN = 4.0
# mutant -> the output that must reject it
PAIR_MUTANTS = {"init_token_divided_by_F": "loss", "init_token_scored_on_all_features": "loss", "mask_t_le_len": "loss",
                "count_not_clamped_to_T": "loss", "pit_pairs_p_with_P_plus_p": "loss", "denom_not_halved_under_pit": "loss",
                "tie_takes_the_second": "dpred", "gradient_on_both_assignments": "dpred", "missing_factor_2": "dpred",
                "gradient_divides_init_token_by_F": "dpred", "rows_divided_by_their_own_length": "loss"}


def pair_mutants(R, T, F, pit, with_len):
    """The mutants that are visible at a shape."""
    m = ["missing_factor_2"]
    if F != 4:
        m += ["init_token_divided_by_F", "init_token_scored_on_all_features", "gradient_divides_init_token_by_F"]
    if with_len:
        m += ["mask_t_le_len", "count_not_clamped_to_T"]
    if pit:
        m += ["pit_pairs_p_with_P_plus_p", "denom_not_halved_under_pit", "gradient_on_both_assignments"]
    if (R, T, F) in PAIR_TIE:
        m += ["tie_takes_the_second"]
    if with_len and not pit:
        m += ["rows_divided_by_their_own_length"]
    return m


def pair_lengths(R, T):
    """0, 1, T, T + 5 and -3 in turn (R = 4 has room for the first four).  Five values: the four rows of a PIT pair (P not a
    multiple of 5) take four different ones, so at least two rows of every pair are scored."""
    pat = (T, 0, 1, T + 5, -3)
    return torch.tensor([pat[r % 5] for r in range(R)], dtype=torch.int64)


def pair_case(R, T, F, pit, with_len, seed=None):
    """(pred, target, length) without NaN.  pred ~ 3 N(0, 1), target ~ N(0, 1); under PIT the pred rows of one assignment per
    pair are scaled by 4 about the target so that the other wins: the first on even pairs, the second on odd ones (and on
    the only pair of R = 4, where the first is what a kernel that never compares would pick)."""
    g = gen(R + T + F if seed is None else seed)
    pred, target = 3 * torch.randn(R, T, F, generator=g), torch.randn(R, T, F, generator=g)
    length = pair_lengths(R, T) if with_len else None
    if pit:
        P = R // 4
        for p in range(P):
            second_wins = p % 2 == 1 or P == 1
            lose = (p, 2 * P + p) if second_wins else (P + p, 3 * P + p)
            for r in lose:
                pred[r] = target[r] + 4 * (pred[r] - target[r])
        tie = PAIR_TIE.get((R, T, F))
        if tie is not None:
            for a, b in ((tie, P + tie), (2 * P + tie, 3 * P + tie)):
                pred[b], target[b], length[b] = pred[a], target[a], length[a]
    return pred, target, length


def pair_live(length, R, T, F):
    L = torch.full((R,), T, dtype=torch.int64) if length is None else length
    tt, ff = torch.arange(T), torch.arange(F)
    return (tt[None, :, None] < L.clamp(0, T)[:, None, None]) & ((tt[:, None] > 0) | (ff[None, :] < 4))[None]


def pair_poison(pred, target, length):
    """NaN at every position the contract says is never read: tokens t >= clamp(len) and features >= 4 of token 0."""
    live = pair_live(length, *pred.shape)
    nan = torch.full_like(pred, float("nan"))
    return torch.where(live, pred, nan), torch.where(live, target, nan)


def pair_ties(pred, target, length, P):
    """Pairs that are ties by construction: rows P + p, 3P + p bitwise copies of rows p, 2P + p."""
    bits = lambda x: x.contiguous().view(torch.int32)  # noqa: E731
    same = lambda a, b: (torch.equal(bits(pred[a]), bits(pred[b])) and torch.equal(bits(target[a]), bits(target[b]))  # noqa: E731
                         and (length is None or length[a] == length[b]))
    return torch.tensor([same(p, P + p) and same(2 * P + p, 3 * P + p) for p in range(P)])


def lane_sum(sq):
    """A wave's sum over the last axis in the kernel's order: lane-strided partial sums (f = lane, lane + 64, ..), then a
    6-level tree."""
    n = sq.shape[-1]
    k = cdiv(n, 64)
    sq = torch.cat([sq, sq.new_zeros(sq.shape[:-1] + (k * 64 - n,))], -1).view(sq.shape[:-1] + (k, 64))
    acc = torch.zeros_like(sq[..., 0, :])
    for i in range(k):
        acc = acc + sq[..., i, :]
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc[..., :o] + acc[..., o:2 * o]
    return acc[..., 0]


def wave_rows(tok):
    """rowloss from (R, T) tokens: wave w adds t = w, w + 4, .. in turn, then (w0 + w1) + (w2 + w3)."""
    R, T = tok.shape
    k = cdiv(T, 4)
    tok = torch.cat([tok, tok.new_zeros(R, 4 * k - T)], 1).view(R, k, 4)
    acc = torch.zeros_like(tok[:, 0])
    for i in range(k):
        acc = acc + tok[:, i]
    return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])


def block_sum(v):
    """One 256-thread block: thread i adds v[i], v[i + 256], .., then red[i] += red[i + o] for o = 128 .. 1."""
    k = cdiv(v.numel(), 256)
    v = torch.cat([v, v.new_zeros(256 * k - v.numel())]).view(k, 256)
    acc = torch.zeros_like(v[0])
    for i in range(k):
        acc = acc + v[i]
    o = 128
    while o:
        acc = acc[:o] + acc[o:2 * o]
        o //= 2
    return acc[0]


def pair_eval(pred, target, length, pit, dtype=F64, mutant=None, kernel_order=False):
    """{'rowloss' (R), 'loss', 'rowscale' (R), 'dpred' (R, T, F), and under PIT 'S0', 'S1', 'first' (P)}.  `where`-masked, so
    NaN at the positions that are never read changes nothing.  kernel_order: the sums in the kernel's order."""
    assert mutant is None or mutant in PAIR_MUTANTS
    R, T, F = pred.shape
    p, q = pred.to(dtype), target.to(dtype)
    L = torch.full((R,), T, dtype=torch.int64) if length is None else length
    lc = L.clamp(0, T)
    tt, ff = torch.arange(T), torch.arange(F)
    on = (tt[None] <= L[:, None]) if mutant == "mask_t_le_len" else (tt[None] < L[:, None])
    fm = (tt[:, None] > 0) | (ff[None, :] < 4)
    if mutant == "init_token_scored_on_all_features":
        fm = torch.ones_like(fm)
    live = on[:, :, None] & fm[None]
    nf = torch.full((T,), F, dtype=dtype)
    nfg = nf.clone()
    if mutant != "init_token_divided_by_F":
        nf[0] = 4
    if mutant != "gradient_divides_init_token_by_F":
        nfg[0] = 4
    dl = torch.where(live, p - q, torch.zeros((), dtype=dtype))
    sq = dl * dl
    tok = (lane_sum(sq) if kernel_order else sq.sum(2)) / nf[None]
    rl = wave_rows(tok) if kernel_order else tok.sum(1)
    total = block_sum if kernel_order else torch.sum
    cnt = (L.clamp_min(0) if mutant == "count_not_clamped_to_T" else lc).sum()
    assert cnt < 2 ** 24, "the token count must stay exact in fp32"
    cnt = cnt.to(dtype)
    denom = cnt * 0.5 if pit and mutant != "denom_not_halved_under_pit" else cnt
    inv = torch.ones((), dtype=dtype) / denom
    out = {"rowloss": rl}
    if pit:
        P = R // 4
        a0, b0, a1, b1 = (torch.arange(P) + k * P for k in ((0, 1, 2, 3) if mutant == "pit_pairs_p_with_P_plus_p" else (0, 2, 1, 3)))
        S0, S1 = rl[a0] + rl[b0], rl[a1] + rl[b1]
        first = (S0 < S1) if mutant == "tie_takes_the_second" else (S0 <= S1)
        out.update(S0=S0, S1=S1, first=first)
        out["loss"] = total(torch.where(first, S0, S1)) / denom
        rs = torch.zeros(R, dtype=dtype)
        zero = torch.zeros((), dtype=dtype)
        rs[a0] = rs[b0] = torch.where(first, inv, zero)
        rs[a1] = rs[b1] = torch.where(first, zero, inv)
        if mutant == "gradient_on_both_assignments":
            rs[:] = inv
    elif mutant == "rows_divided_by_their_own_length":
        n = (lc > 0).sum().to(dtype)
        out["loss"] = (rl / lc.clamp_min(1).to(dtype)).sum() / n
        rs = 1 / (lc.clamp_min(1).to(dtype) * n)
    else:
        out["loss"] = total(rl) / denom
        rs = inv.expand(R).clone()
    out["rowscale"] = rs
    two = 1.0 if mutant == "missing_factor_2" else 2.0
    out["dpred"] = torch.where(live, rs[:, None, None] * two * (p - q) / nfg[None, :, None], torch.zeros((), dtype=dtype))
    return out


def pair_bound(pred, target, length, pit):
    """{'rowloss' | 'loss' | 'dpred': (ref, bound)}, 'rowscale32' (the fp32 values the kernel must write, bit for bit), 'live',
    and under PIT 'first', 'margin', 'tie' per pair."""
    R, T, F = pred.shape
    ref = pair_eval(pred, target, length, pit)
    L = torch.full((R,), T, dtype=torch.int64) if length is None else length
    lc = L.clamp(0, T)
    live = pair_live(length, R, T, F)
    dl = torch.where(live, pred.double() - target.double(), torch.zeros((), dtype=F64))
    nf = torch.full((T,), float(F), dtype=F64)
    nf[0] = 4
    tok = (dl * dl).sum(2) / nf[None]
    g_tok = 3 + torch.ceil(nf / 64) + 6 + 1
    b_row = (gam(g_tok[None] + torch.ceil(lc.double() / 4)[:, None] + 2) * tok).sum(1)
    rl = ref["rowloss"]
    cnt = float(lc.sum())
    denom = cnt / 2 if pit else cnt
    inv32 = (torch.ones((), dtype=F32) / torch.tensor(denom, dtype=F32))
    out = {"rowloss": (rl, b_row), "live": live}
    if pit:
        P = R // 4
        p = torch.arange(P)
        first = ref["first"]
        rows0, rows1 = torch.cat([p, 2 * P + p]), torch.cat([P + p, 3 * P + p])
        chosen = torch.zeros(R, dtype=torch.bool)
        chosen[rows0] = first.repeat(2)
        chosen[rows1] = ~first.repeat(2)
        S0, S1 = ref["S0"], ref["S1"]
        four = b_row[p] + b_row[P + p] + b_row[2 * P + p] + b_row[3 * P + p] + U * (S0 + S1)
        out.update(first=first, margin=(S0 - S1).abs() / four, tie=pair_ties(pred, target, length, P))
        n = P
    else:
        chosen = torch.ones(R, dtype=torch.bool)
        n = R
    k = gam(int(bool(pit)) + cdiv(n, 256) + 8 + 1)
    out["loss"] = (ref["loss"], (b_row[chosen].sum() * (1 + k) + k * rl[chosen].sum()) / denom)
    out["rowscale32"] = torch.where(chosen, inv32, torch.zeros((), dtype=F32))
    out["dpred"] = (ref["dpred"], gam(4) * ref["dpred"].abs())
    return out


# ----------------------------------------------------------------------------------------------------------------------
# hig_recover_joints
# ----------------------------------------------------------------------------------------------------------------------
# (rows, T, J, F, init_first, stats)
RECOVER_CASES = ((1, 1, 1, 4, 0, False),        # the smallest legal shape
                 (2, 2, 2, 7, 1, True),
                 (3, 255, 22, 263, 1, True),
                 (1, 257, 21, 263, 0, False),
                 (2, 600, 3, 12, 1, False))     # F > 4 + 3 (J - 1); rotation velocities near 0.5: the yaw reaches ~300 rad
RECOVER_LDS_CASE = (1, 4097, 2, 7, 0, False)    # 16 T bytes of LDS: the first size above 64 KiB (GPU only)
RECOVER_MUTANTS = ("yaw_sign_flipped", "inclusive_prefix", "velocity_of_frame_t", "init_rotation_skipped",
                   "init_translation_before_rotation", "mean_and_std_swapped", "init_statistics_read_at_2F",
                   "root_height_of_frame_t_minus_1")
# NOT a mutant: a prefix sum of the yaw accumulated in fp32 instead of double.  At T = 600 (the yaw reaches 299 rad in steps of
# 0.5) it puts the yaw off by 2.6e-4 = 14 u |yaw| and moves the last frames by 5e-3, where the bound is 3e-2: the root position
# inherits the SUM of 600 per-frame velocity bounds, each 2 delta |v| with delta = u |yaw| up to 1.8e-5, and a sum of worst
# cases outgrows the random walk of an fp32 accumulator.  It reached 0.29 of the bound, so it is not listed; the double
# accumulator stays pinned by the golden g12 alone.


def recover_mutants(rows, T, J, F, init_first, with_stats):
    """The mutants that are visible at a shape: the frame offsets need a second frame, the init rotation something off the Y
    axis to turn (at T = 1, J = 1 the root is at the origin), the statistics need statistics."""
    m = ["init_translation_before_rotation"]
    if T > 1:
        m += ["init_rotation_skipped", "yaw_sign_flipped", "inclusive_prefix", "velocity_of_frame_t", "root_height_of_frame_t_minus_1"]
    if with_stats:
        m += ["mean_and_std_swapped", "init_statistics_read_at_2F"]
    return m


def recover_case(rows, T, J, F, init_first, with_stats):
    """(motion (rows, T + 1, F), stats (2 F + 8) or None): feature 0 (the yaw velocity) scaled by 0.05, near 0.5 at T >= 600;
    the init row carries a normalised (cos, sin) pair in features 2, 3."""
    g = gen(rows + T + J + F)
    m = torch.randn(rows, T + 1, F, generator=g)
    m[..., 0] = 0.05 * m[..., 0] + (0.5 if T >= 600 else 0.0)
    ir = 0 if init_first else T
    m[:, ir, 2:4] = torch.nn.functional.normalize(m[:, ir, 2:4], dim=-1)
    stats = None
    if with_stats:
        mean, sd = torch.randn(F, generator=g), 1 + 0.5 * torch.randn(F, generator=g).abs()
        imean, isd = torch.randn(4, generator=g), 1 + 0.5 * torch.randn(4, generator=g).abs()
        stats = torch.cat([mean, sd, imean, isd])
    return m, stats


def recover_ref(motion, stats, J, init_first):
    """oracle.motion_ref in fp64: denormalize_sample (which also moves the init row last) then recover_person."""
    from oracle import motion_ref as MR
    m = motion.double()
    F = m.shape[2]
    if stats is not None:
        st = stats.double()
        assert init_first, "the oracle de-normalises the sampler's token order"
        m = torch.stack([MR.denormalize_sample(x, st[:F], st[F:2 * F], st[2 * F:2 * F + 4], st[2 * F + 4:]) for x in m])
    elif init_first:
        m = torch.cat([m[:, 1:], m[:, :1]], 1)
    return MR.recover_person(m, J)


def roty(c, s, vx, vz):
    """qrot3 with q = (c, (0, -s, 0)), in the kernel's order; returns (x', z') (y' = vy)."""
    uvx, uvz = -s * vz, s * vx
    return vx + 2 * (c * uvx + -s * uvz), vz + 2 * (c * uvz + s * uvx)


def prefix(x, dtype):
    """An inclusive prefix sum over axis 1 with a double accumulator, rounded to dtype (the kernel's serial lane)."""
    return x.double().cumsum(1).to(dtype)


def recover_eval(motion, stats, J, init_first, dtype=F64, mutant=None):
    """pos (rows, T, J, 3)."""
    assert mutant is None or mutant in RECOVER_MUTANTS
    rows, T1, F = motion.shape
    T = T1 - 1
    m = motion.to(dtype)
    body, init = (m[:, 1:], m[:, 0]) if init_first else (m[:, :-1], m[:, -1])
    i4 = init[:, :4]
    if stats is not None:
        st = stats.to(dtype)
        mean, sd = st[:F], st[F:2 * F]
        if mutant == "mean_and_std_swapped":
            mean, sd = sd, mean
        o = 2 * F - 4 if mutant == "init_statistics_read_at_2F" else 2 * F
        body, i4 = body * sd + mean, i4 * st[o + 4:o + 8] + st[o:o + 4]
    rot = body[..., 0]
    shifted = lambda x: torch.cat([torch.zeros_like(x[:, :1]), x[:, :-1]], 1)  # noqa: E731
    ang = rot if mutant == "inclusive_prefix" else shifted(rot)
    ang = prefix(ang, dtype)
    if mutant == "yaw_sign_flipped":
        ang = -ang
    c, s = torch.cos(ang), torch.sin(ang)
    vx, vz = (body[..., 1], body[..., 2]) if mutant == "velocity_of_frame_t" else (shifted(body[..., 1]), shifted(body[..., 2]))
    wx, wz = roty(c, s, vx, vz)
    px, pz = prefix(wx, dtype), prefix(wz, dtype)
    ry = body[..., 3]
    if mutant == "root_height_of_frame_t_minus_1":
        ry = torch.cat([ry[:, :1], ry[:, :-1]], 1)
    loc = body[..., 4:4 + 3 * (J - 1)].reshape(rows, T, J - 1, 3)
    jx, jz = roty(c[..., None], s[..., None], loc[..., 0], loc[..., 2])
    X = torch.cat([px[..., None], jx + px[..., None]], 2)
    Y = torch.cat([ry[..., None], loc[..., 1]], 2)
    Z = torch.cat([pz[..., None], jz + pz[..., None]], 2)
    ix, iz, c0, s0 = (i4[:, k, None, None] for k in range(4))
    if mutant == "init_translation_before_rotation":
        X, Z = X + ix, Z + iz
    if mutant != "init_rotation_skipped":
        X, Z = roty(c0, -s0, X, Z)
    if mutant != "init_translation_before_rotation":
        X, Z = X + ix, Z + iz
    return torch.stack([X, Y, Z], -1)


def roty_bound(c, s, e_c, e_s, vx, vz, e_vx, e_vz, delta=0.0):
    """(x', z', e_x', e_z') of roty in fp64 with the bound of the docstring.  delta: the error of the angle behind (c, s)."""
    def one(v, w, e_v, e_w, sign):      # v + 2 (sign c s w - s^2 v)
        A, B = c * s * w, s * s * v
        e_A = gam(2) * A.abs() + (s * w).abs() * e_c + (c * w).abs() * e_s + (c * s).abs() * e_w
        e_B = gam(2) * B.abs() + 2 * (s * v).abs() * e_s + s * s * e_v
        r = v + 2 * (sign * A - B)
        return r, e_v + 2 * (e_A + e_B + U * (A.abs() + B.abs())) + U * r.abs()
    x, e_x = one(vx, vz, e_vx, e_vz, -1.0)
    z, e_z = one(vz, vx, e_vz, e_vx, 1.0)
    turn = 2 * delta * delta * torch.hypot(vx, vz)
    return x, z, e_x + 2 * delta * z.abs() + turn, e_z + 2 * delta * x.abs() + turn


def recover_bound(motion, stats, J, init_first):
    """(ref, bound), each (rows, T, J, 3) in fp64.  ref is recover_eval's fp64 value (recover_ref to 1e-12, which the CPU test
    checks)."""
    rows, T1, F = motion.shape
    T = T1 - 1
    m = motion.double()
    body, init = (m[:, 1:], m[:, 0]) if init_first else (m[:, :-1], m[:, -1])
    i4 = init[:, :4]
    e_body, e_i4 = torch.zeros_like(body), torch.zeros_like(i4)
    if stats is not None:
        st = stats.double()
        mean, sd, imean, isd = st[:F], st[F:2 * F], st[2 * F:2 * F + 4], st[2 * F + 4:]
        e_body, body = U * ((body * sd).abs() + (body * sd + mean).abs()), body * sd + mean
        e_i4, i4 = U * ((i4 * isd).abs() + (i4 * isd + imean).abs()), i4 * isd + imean
    shifted = lambda x: torch.cat([torch.zeros_like(x[:, :1]), x[:, :-1]], 1)  # noqa: E731
    rot, e_rot = shifted(body[..., 0]), shifted(e_body[..., 0])
    ang = rot.cumsum(1)
    delta = e_rot.cumsum(1) + U * ang.abs() + T * 2.0 ** -53 * rot.abs().cumsum(1)
    c, s = torch.cos(ang), torch.sin(ang)
    e_c, e_s = ULP4 * (c.abs() + delta), ULP4 * (s.abs() + delta)
    wx, wz, e_wx, e_wz = roty_bound(c, s, e_c, e_s, shifted(body[..., 1]), shifted(body[..., 2]), shifted(e_body[..., 1]),
                                    shifted(e_body[..., 2]), delta)
    px, pz = wx.cumsum(1), wz.cumsum(1)
    e_px = e_wx.cumsum(1) + U * px.abs() + T * 2.0 ** -53 * wx.abs().cumsum(1)
    e_pz = e_wz.cumsum(1) + U * pz.abs() + T * 2.0 ** -53 * wz.abs().cumsum(1)
    loc = body[..., 4:4 + 3 * (J - 1)].reshape(rows, T, J - 1, 3)
    e_loc = e_body[..., 4:4 + 3 * (J - 1)].reshape(rows, T, J - 1, 3)
    jx, jz, e_jx, e_jz = roty_bound(c[..., None], s[..., None], e_c[..., None], e_s[..., None], loc[..., 0], loc[..., 2],
                                    e_loc[..., 0], e_loc[..., 2], delta[..., None])
    jx, jz = jx + px[..., None], jz + pz[..., None]
    e_jx, e_jz = e_jx + e_px[..., None] + U * jx.abs(), e_jz + e_pz[..., None] + U * jz.abs()
    X, e_X = torch.cat([px[..., None], jx], 2), torch.cat([e_px[..., None], e_jx], 2)
    Z, e_Z = torch.cat([pz[..., None], jz], 2), torch.cat([e_pz[..., None], e_jz], 2)
    Y, e_Y = torch.cat([body[..., 3, None], loc[..., 1]], 2), torch.cat([e_body[..., 3, None], e_loc[..., 1]], 2)
    ix, iz, c0, s0 = (i4[:, k, None, None] for k in range(4))
    e_ix, e_iz, e_c0, e_s0 = (e_i4[:, k, None, None] for k in range(4))
    X, Z, e_X, e_Z = roty_bound(c0, -s0, e_c0, e_s0, X, Z, e_X, e_Z)
    X, Z = X + ix, Z + iz
    e_X, e_Z = e_X + e_ix + U * X.abs(), e_Z + e_iz + U * Z.abs()
    return recover_eval(motion, stats, J, init_first), torch.stack([e_X, e_Y, e_Z], -1)


# ----------------------------------------------------------------------------------------------------------------------
# hig_timestep_embedding, hig_timestep_embedding_bf16
# ----------------------------------------------------------------------------------------------------------------------
TEMB_D = (2, 3, 64, 65, 512)
TEMB_T = (0, 1, 7, 500, 999)        # B = 5: 5 x 65 = 325 elements span two blocks raggedly
TEMB_MUTANTS = ("sin_and_cos_halves_swapped", "i_over_half_minus_1", "max_period_1000", "odd_d_last_column_cos",
                "fast_fp32_exp", "argument_rounded_to_bf16")
LN1E4 = math.log(10000.0)
LN1E4_32 = float(torch.tensor(LN1E4, dtype=F32))
KAPPA = abs(LN1E4_32 - LN1E4) / LN1E4 / U       # the rounding of the kernel's constant, in units of u: 0.23


def temb_mutants(d):
    """Visible: the frequency mutants need a second frequency (half > 1), the last column an odd d."""
    m = ["sin_and_cos_halves_swapped", "fast_fp32_exp", "argument_rounded_to_bf16"]
    if d // 2 > 1:
        m += ["i_over_half_minus_1", "max_period_1000"]
    if d % 2:
        m += ["odd_d_last_column_cos"]
    return m


def temb_case():
    return torch.tensor(TEMB_T, dtype=torch.int64)


def temb_eval(t, d, dtype=F64, mutant=None):
    """(B, d): [cos(t f_i) | sin(t f_i) | 0 if d is odd], f_i = exp(-ln(10000) i / half).  dtype fp32: the kernel's order (the
    fp32 constant, its product with i, the division; exp in double rounded once)."""
    assert mutant is None or mutant in TEMB_MUTANTS
    half = d // 2
    i = torch.arange(half).to(dtype)
    ln = math.log(1000.0) if mutant == "max_period_1000" else (LN1E4_32 if dtype == F32 else LN1E4)
    e = -torch.tensor(ln, dtype=dtype) * i / torch.tensor(half - 1 if mutant == "i_over_half_minus_1" else half, dtype=dtype)
    freq = torch.exp(e.double()).to(dtype)
    if mutant == "fast_fp32_exp":
        freq = freq * (1 + 2.0 ** -21)
    arg = t.to(dtype)[:, None] * freq
    if mutant == "argument_rounded_to_bf16":
        arg = arg.to(BF16).to(dtype)
    a, b = torch.cos(arg), torch.sin(arg)
    if mutant == "sin_and_cos_halves_swapped":
        a, b = b, a
    cols = [a, b]
    if d % 2:
        cols.append(torch.cos(t.to(dtype))[:, None] if mutant == "odd_d_last_column_cos" else torch.zeros(len(t), 1, dtype=dtype))
    return torch.cat(cols, 1)


def temb_bound(t, d):
    """(ref, bound) (B, d) in fp64; the bound of the last column of an odd d is 0."""
    half = d // 2
    e = -LN1E4 * torch.arange(half, dtype=F64) / half
    arg = t.double()[:, None] * torch.exp(e)
    delta = U * arg.abs() * ((2 + KAPPA) * e.abs() + 3)
    ref = temb_eval(t, d)
    delta = torch.cat([delta, delta] + ([torch.zeros(len(t), 1, dtype=F64)] if d % 2 else []), 1)
    return ref, delta + ULP4 * (ref.abs() + delta)


# ----------------------------------------------------------------------------------------------------------------------
# hig_gather_frames (exact)
# ----------------------------------------------------------------------------------------------------------------------
GATHER_CASES = ((1, 1, 4), (2, 2, 5), (3, 7, 300))      # (rows, T, F); token 0 is the init row
GATHER_FRAMES = 9                                       # frames per sequence of the bank
GATHER_MUTANTS = ("init_row_normalised_on_all_features", "init_row_with_body_statistics", "f64_path_in_f32",
                  "frame_ix_row_stride_T_plus_1")


def gather_mutants(rows, T, F, f64):
    m = ["init_row_with_body_statistics"]
    if F > 4:
        m += ["init_row_normalised_on_all_features"]
    if f64:
        m += ["f64_path_in_f32"]
    if rows > 1:
        m += ["frame_ix_row_stride_T_plus_1"]
    return m


def gather_case(rows, T, F):
    """(bank float32, seq_off int64 (odd), frame_ix int32 (rows, T) (descending, every frame twice), stats float64 (2 F + 8)).
    The float32 statistics of a case are stats.astype(float32); the float64 ones are not fp32 numbers, so the two paths
    differ (the CPU test asserts that they do)."""
    rng = np.random.default_rng(rows + T + F)
    seq_off = np.array([2 * r * (5 * F + 1) + 1 for r in range(rows)], dtype=np.int64)
    bank = rng.standard_normal(int(seq_off[-1]) + GATHER_FRAMES * F).astype(np.float32)
    frame_ix = np.array([[(GATHER_FRAMES - 1 - t // 2 - r) % GATHER_FRAMES for t in range(T)] for r in range(rows)], dtype=np.int32)
    stats = np.concatenate([rng.standard_normal(F), 0.5 + rng.random(F), rng.standard_normal(4), 0.5 + rng.random(4)])
    return bank, seq_off, frame_ix, stats


def gather_eval(bank, seq_off, frame_ix, stats, f64, mutant=None):
    """(rows, T, F) float32: numpy's ((x - mean) / sd).astype(float32) with float32 or float64 statistics."""
    assert mutant is None or mutant in GATHER_MUTANTS
    rows, T = frame_ix.shape
    F = (stats.size - 8) // 2
    st = stats.astype(np.float64 if f64 and mutant != "f64_path_in_f32" else np.float32)
    mean, sd, imean, isd = st[:F], st[F:2 * F], st[2 * F:2 * F + 4], st[2 * F + 4:]
    ix = frame_ix.astype(np.int64)
    if mutant == "frame_ix_row_stride_T_plus_1":
        flat = np.concatenate([ix.reshape(-1), np.zeros(rows, dtype=np.int64)])
        ix = flat[np.arange(rows)[:, None] * (T + 1) + np.arange(T)[None]]
    src = bank[(seq_off[:, None] + ix * F)[..., None] + np.arange(F)]       # (rows, T, F) float32
    out = ((src - mean) / sd).astype(np.float32)
    if mutant == "init_row_normalised_on_all_features":
        k = min(F, 4)
        init = np.concatenate([((src[:, 0, :k] - imean[:k]) / isd[:k]), ((src[:, 0, k:] - mean[k:]) / sd[k:])], 1).astype(np.float32)
    elif mutant == "init_row_with_body_statistics":
        init = np.concatenate([((src[:, 0, :4] - mean[:4]) / sd[:4]).astype(np.float32), src[:, 0, 4:]], 1)
    else:
        init = np.concatenate([((src[:, 0, :4] - imean) / isd).astype(np.float32), src[:, 0, 4:]], 1)
    out[:, 0] = init
    return out
