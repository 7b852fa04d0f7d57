"""fp64 restatements, element-wise fp32 bounds and the case tables of the per-timestep loss weights: the weighted losses
hig_masked_mse_w and hig_pair_mse_w, and the device loss history hig_loss_history_update (csrc/ddpm.hip).  Plain torch / numpy
on the host: tests/test_cpu_loss_weighting.py proves without a GPU that the bounds accept fp32 in the kernels' order and reject
a mutant each, tests/test_gpu_loss_weighting.py holds the kernels to them.

The rule and the counting conventions are those of tests/rowops_bounds.py and tests/boundary_bounds.py: u = 2^-24, a result is
within gamma u M of its fp64 value, gam(n) = n u / (1 - n u) for n roundings in sequence.  The fp32 entries of the weight table
are taken as exact (the reference reads the same fp32 numbers the kernel reads).  No bound below was fitted to a measurement.

hig_masked_mse_w (`masked_w_bound`).  w_b = wtab[clamp(t_b)] > 0, m[b][tau] = mean_f (p - q)^2.
  loss         the unweighted count of rowops_bounds.masked_mse_bound -- (F + 3) for a row's sum of squares, the division by
               F, h = masked_mse_depth over the rows, the final division -- and one more for the product w m (an fma of it
               rounds less: covered).  All terms are non-negative, so M is the loss itself: (F + 6 + h) u loss.
  dpred        ((2 / (F cnt)) w) (p - q): F cnt, 2 / x, the product with w, the difference, the product: gam(5) |dpred|;
               exactly 0 off the mask.
  sample_loss  sum_{tau < len} m / max(len, 1): (F + 3) + 1 for a row mean, one thread adds len of them in order, one
               division: gam(F + 4 + len + 1) of itself.

hig_pair_mse_w (`pair_w_bound`).  Row losses, their bound b_row, the PIT decision with its margin: boundary_bounds.pair_bound
unchanged -- the weighted kernel compares the unweighted sums.  w_p = wtab[clamp(t[p])] under PIT (row p), w_r per row without.
  rowscale     fp32(w fp32(1 / denom)) on the chosen rows, 0 elsewhere: a correctly rounded product of two fp32 numbers, so the
               kernel's value must be that number bit for bit.
  loss         sum w S / denom by one block: k = pit (S = L[a] + L[b]) + 1 (w S) + ceil(n / 256) + 8 + 1;
               b = (sum w b_S (1 + gam(k)) + gam(k) sum w S) / denom, b_S the chosen rows' b_row.
  dpred        rowscale 2 (p - q) / nf: 1 / denom, w x, the difference, the product, the division: gam(5) |dpred|; exactly 0
               off the mask, on features >= 4 of token 0 and on the unchosen rows.
  sample_loss  PIT: min(S0, S1) / (2 max(len_p, 1)) -- b_S / (2 len) and three roundings (the sum S, 2 len is exact, the
               division; one spare): b_S / (2 len) + gam(3) of itself.  Without PIT: rowloss / max(len, 1): b_row / len + gam(3).

hig_loss_history_update (`HistoryMirror`, `refresh_bound`).  The mirror is the reference's update_with_all_losses in fp64 with
the kernel's three rules added: an entry outside [0, nsteps) is skipped, a non-finite value is skipped, and what is pushed is
base_w[t] loss -- rounded to fp32 when `round32` is set, which is then the exact content of the device history (one correctly
rounded product), to be matched bit for bit.  The refresh is bounded against the mirror's fp64 refresh of those fp32 values:
  m_t          sqrt(sum_h hist^2 / H): H squares, H adds, one division: relative gam(2 H + 1) under the root, which halves it, and
               the root's own rounding: r_m = gam(2 H + 1) / 2 + u (1 + gam(2 H + 1)).
  total        a thread adds its ceil(N / 1024) values, then a 10-level tree: r_t = r_m + gam(ceil(N / 1024) + 10) (1 + r_m).
  p_t          A = (1 - u_p) (m / total): the quotient 1, 1 - u_p rounds once, the product 1; C = u_p / N: 1; the sum 1:
               b_p = A (r_m + r_t + gam(3)) (1 + 4 u + r_m + r_t) + u C + u p
               (the first-order terms; the trailing factor covers their products).
  w_t          base / (N p): N p and the quotient round once each, p carries b_p: b_w = w (b_p / p) / (1 - b_p / p) + gam(2) w (1 + b_p / p).
  not warmed up, or a total that is 0 / not finite: p = fp32(1 / N) and w = base_w exactly.
  sum_t p_t    = 1 within N u (every p_t is within u p_t + its share of the sums' roundings; asserted on the mirror's fp32 emulation).
"""
import math

import numpy as np
import torch

from rowops_bounds import U, F64, F32, ratio, gen, cdiv, masked_mse_depth  # noqa: F401
import boundary_bounds as bb
from boundary_bounds import gam

NSTEPS = 1000


def weight_table(nsteps=NSTEPS):
    """nsteps fp32 weights over 1e-4 .. 1e2, log-spaced: row 0 is the smallest, the last row the largest."""
    return torch.logspace(-4, 2, nsteps, dtype=F64).float() if nsteps > 1 else torch.tensor([3.0])


def step_weights(wtab, t, mutant=None):
    """w[clamp(t, 0, nsteps - 1)]; the mutant indexes the table by the sample's position instead of its timestep."""
    n = wtab.numel()
    idx = torch.arange(t.numel()) % n if mutant == "weight_indexed_by_b" else t.clamp(0, n - 1)
    return wtab[idx]


# ----------------------------------------------------------------------------------------------------------------------
# hig_masked_mse_w
# ----------------------------------------------------------------------------------------------------------------------
# (B, T, F)
MASKED_SHAPES = ((1, 1, 4), (3, 5, 7), (5, 9, 263), (70, 4, 4))
MASKED_MUTANTS = ("weight_indexed_by_b",)


def masked_lengths(B, T):
    """0, 1, T, T + 3 and -2 in turn, starting at T (so that B = 1 scores its only sample)."""
    pat = (T, 0, 1, T + 3, -2)
    return torch.tensor([pat[b % 5] for b in range(B)], dtype=torch.int64)


def masked_t(B, nsteps=NSTEPS):
    """0, nsteps - 1, two values outside the table and inner rows in turn."""
    pat = (nsteps - 1, 0, -3, nsteps + 5, nsteps // 3, nsteps // 2, 2 * nsteps // 3)
    return torch.tensor([pat[b % 7] for b in range(B)], dtype=torch.int64)


def masked_case(B, T, F, with_len=True):
    g = gen(7 * B + T + F)
    pred, target = 3 * torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g)
    return pred, target, (masked_lengths(B, T) if with_len else None), masked_t(B), weight_table()


def masked_poison(pred, target, length):
    """NaN at every frame off the mask: nothing there may contribute."""
    B, T, F = pred.shape
    L = torch.full((B,), T, dtype=torch.int64) if length is None else length
    on = (torch.arange(T)[None] < L[:, None])[:, :, None].expand(B, T, F)
    nan = torch.full_like(pred, float("nan"))
    return torch.where(on, pred, nan), torch.where(on, target, nan)


def masked_w_eval(pred, target, length, t, wtab, dtype=F64, mutant=None, kernel_order=False):
    """{'loss', 'dpred' (B, T, F), 'sample_loss' (B)}; `where`-masked, so NaN off the mask changes nothing.  kernel_order: the
    sums in the kernel's order (lane-strided feature sums and the wave tree; a wave adds its rows in turn, four waves per
    workgroup, the final block's tree; one thread adds a sample's rows in frame order)."""
    B, T, F = pred.shape
    p, q = pred.to(dtype), target.to(dtype)
    L = torch.full((B,), T, dtype=torch.int64) if length is None else length
    lc = L.clamp(0, T)
    on = torch.arange(T)[None] < L[:, None]
    zero = torch.zeros((), dtype=dtype)
    dl = torch.where(on[:, :, None], p - q, zero)
    sq = dl * dl
    m = (bb.lane_sum(sq) if kernel_order else sq.sum(2)) / F                       # (B, T) row means, 0 off the mask
    w = step_weights(wtab, t, mutant).to(dtype)
    cnt = lc.sum().to(dtype)
    wm = (w[:, None] * m).reshape(-1)
    if kernel_order:
        rows = B * T
        nblk = min(cdiv(rows, 4), 1023)
        trips = cdiv(rows, 4 * nblk)
        v = torch.cat([wm, wm.new_zeros(trips * 4 * nblk - rows)]).view(trips, nblk, 4)
        acc = torch.zeros_like(v[0])
        for i in range(trips):
            acc = acc + v[i]
        part = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
        loss = bb.block_sum(part) / cnt
        s = torch.zeros(B, dtype=dtype)
        for tau in range(T):
            s = s + m[:, tau]
    else:
        loss = wm.sum() / cnt
        s = m.sum(1)
    gs = (2.0 / (F * cnt)) * w
    return {"loss": loss, "dpred": torch.where(on[:, :, None], gs[:, None, None] * (p - q), zero),
            "sample_loss": s / lc.clamp_min(1).to(dtype)}


def masked_w_bound(pred, target, length, t, wtab):
    """{'loss' | 'dpred' | 'sample_loss': (ref, bound)}."""
    B, T, F = pred.shape
    ref = masked_w_eval(pred, target, length, t, wtab)
    L = torch.full((B,), T, dtype=torch.int64) if length is None else length
    lc = L.clamp(0, T).double()
    return {"loss": (ref["loss"], (F + 6 + masked_mse_depth(B, T)) * U * ref["loss"].abs()),
            "dpred": (ref["dpred"], gam(5) * ref["dpred"].abs()),
            "sample_loss": (ref["sample_loss"], gam(F + 4 + lc + 1) * ref["sample_loss"].abs())}


# ----------------------------------------------------------------------------------------------------------------------
# hig_pair_mse_w
# ----------------------------------------------------------------------------------------------------------------------
# (R, T, F, pit): R = 4, 12 and 1028 with PIT on and off; lengths 0, 1, T, T + 5, -3 (boundary_bounds.pair_lengths) and None
PAIR_W_SHAPES = ((4, 5, 4, 1, True), (4, 5, 4, 0, True), (12, 9, 263, 1, True), (12, 9, 263, 0, True), (1028, 2, 4, 1, True),
                 (1028, 2, 4, 0, True), (12, 6, 70, 1, False))
PAIR_W_MUTANTS = ("weight_indexed_by_b", "weight_before_selection_on_one_assignment")


def pair_t(R, pit, nsteps=NSTEPS):
    """One t per row, the rows of a pair sharing it (t = cat([t, t]), repeated once more under PIT).  Pair 0 takes the largest
    weight and pair 1 the smallest: with the 16 x margin of boundary_bounds.pair_case, weighting one assignment before the
    comparison turns both decisions."""
    n = R // 4 if pit else (R + 1) // 2
    t = masked_t(n, nsteps)
    return torch.cat([t] * (4 if pit else 2))[:R].contiguous()


def pair_w_case(R, T, F, pit, with_len):
    pred, target, length = bb.pair_case(R, T, F, pit, with_len)
    return pred, target, length, pair_t(R, pit), weight_table()


def pair_w_eval(pred, target, length, pit, t, wtab, dtype=F64, mutant=None, kernel_order=False):
    """boundary_bounds.pair_eval's row losses, then {'loss', 'rowscale' (R), 'dpred', 'sample_loss' (P or R), 'first' (P)}."""
    R, T, F = pred.shape
    base = bb.pair_eval(pred, target, length, pit, dtype=dtype, kernel_order=kernel_order)
    rl = base["rowloss"]
    L = torch.full((R,), T, dtype=torch.int64) if length is None else length
    lc = L.clamp(0, T)
    cnt = lc.sum().to(dtype)
    denom = cnt * 0.5 if pit else cnt
    inv = torch.ones((), dtype=dtype) / denom
    total = bb.block_sum if kernel_order else torch.sum
    zero = torch.zeros((), dtype=dtype)
    out = {"rowloss": rl}
    if pit:
        P = R // 4
        p = torch.arange(P)
        w = step_weights(wtab, t[:P], mutant if mutant == "weight_indexed_by_b" else None).to(dtype)
        S0, S1 = base["S0"], base["S1"]
        first = (w * S0 <= S1) if mutant == "weight_before_selection_on_one_assignment" else base["first"]
        sel = torch.where(first, S0, S1)
        out["first"] = first
        out["loss"] = total(w * sel) / denom
        ws = w * inv
        rs = torch.zeros(R, dtype=dtype)
        rs[p] = rs[2 * P + p] = torch.where(first, ws, zero)
        rs[P + p] = rs[3 * P + p] = torch.where(first, zero, ws)
        out["sample_loss"] = sel / (2.0 * lc[:P].clamp_min(1).to(dtype))
    else:
        w = step_weights(wtab, t, mutant).to(dtype)
        out["loss"] = total(w * rl) / denom
        rs = w * inv
        out["sample_loss"] = rl / lc.clamp_min(1).to(dtype)
    out["rowscale"] = rs
    live = bb.pair_live(length, R, T, F)
    nf = torch.full((T,), float(F), dtype=dtype)
    nf[0] = 4
    out["dpred"] = torch.where(live, rs[:, None, None] * 2.0 * (pred.to(dtype) - target.to(dtype)) / nf[None, :, None], zero)
    return out


def pair_w_bound(pred, target, length, pit, t, wtab):
    """{'loss' | 'dpred' | 'sample_loss': (ref, bound)}, 'rowscale32' (bit for bit), 'live', and what boundary_bounds.pair_bound
    gives for the unweighted part: 'rowloss', and under PIT 'first', 'margin', 'tie'."""
    R, T, F = pred.shape
    ub = bb.pair_bound(pred, target, length, pit)
    ref = pair_w_eval(pred, target, length, pit, t, wtab)
    b_row = ub["rowloss"][1]
    L = torch.full((R,), T, dtype=torch.int64) if length is None else length
    lc = L.clamp(0, T)
    cnt = float(lc.sum())
    denom = cnt / 2 if pit else cnt
    inv32 = torch.ones((), dtype=F32) / torch.tensor(denom, dtype=F32)
    out = {"rowloss": ub["rowloss"], "live": ub["live"]}
    rl = ref["rowloss"]
    if pit:
        P = R // 4
        p = torch.arange(P)
        first = ref["first"]
        w32 = step_weights(wtab, t[:P])
        a, b = torch.where(first, p, P + p), torch.where(first, 2 * P + p, 3 * P + p)
        S, b_S = rl[a] + rl[b], b_row[a] + b_row[b]
        n = P
        ws32 = w32 * inv32
        rs32 = torch.zeros(R, dtype=F32)
        rs32[p] = rs32[2 * P + p] = torch.where(first, ws32, torch.zeros((), dtype=F32))
        rs32[P + p] = rs32[3 * P + p] = torch.where(first, torch.zeros((), dtype=F32), ws32)
        ln = 2.0 * lc[:P].clamp_min(1).double()
        out.update(first=ub["first"], margin=ub["margin"], tie=ub["tie"])
    else:
        w32 = step_weights(wtab, t)
        S, b_S, n = rl, b_row, R
        rs32 = w32 * inv32
        ln = lc.clamp_min(1).double()
    w = w32.double()
    k = pit + 1 + cdiv(n, 256) + 8 + 1
    out["loss"] = (ref["loss"], ((w * b_S).sum() * (1 + gam(k)) + gam(k) * (w * S).sum()) / denom)
    out["rowscale32"] = rs32
    out["dpred"] = (ref["dpred"], gam(5) * ref["dpred"].abs())
    out["sample_loss"] = (ref["sample_loss"], b_S / ln + gam(3) * ref["sample_loss"].abs())
    return out


# ----------------------------------------------------------------------------------------------------------------------
# hig_loss_history_update
# ----------------------------------------------------------------------------------------------------------------------
HISTORY_MUTANTS = ("push_order_reversed", "refresh_one_push_early")


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


class HistoryMirror:
    """The loss history on the host in float64.  round32: the pushed value is fp32(fp32(base_w) fp32(loss)), what the device
    ring holds; otherwise base_w loss in float64 (with base_w = 1: the reference's sampler).  `update` is the push of one
    launch, `refresh` the (p, w) it leaves; `emulate32` runs the refresh in fp32 in the kernel's order."""

    def __init__(self, nsteps, H, base_w=None, uniform_prob=0.001, round32=True, mutant=None):
        assert mutant is None or mutant in HISTORY_MUTANTS
        self.N, self.H, self.round32, self.mutant = int(nsteps), int(H), round32, mutant
        self.u = float(np.float32(uniform_prob)) if round32 else float(uniform_prob)
        base = np.ones(self.N) if base_w is None else np.asarray(base_w, dtype=np.float64)
        self.base = f32(base) if round32 else base
        self.hist = np.zeros((self.N, self.H), dtype=np.float64)
        self.counts = np.zeros(self.N, dtype=np.int64)
        self.pushes = 0

    def update(self, ts, losses):
        pairs = list(zip(np.asarray(ts).tolist(), np.asarray(losses, dtype=np.float64).tolist()))
        if self.mutant == "push_order_reversed":
            pairs = pairs[::-1]
        for t, loss in pairs:
            if not 0 <= t < self.N:
                continue
            v = self.base[t] * (float(np.float32(loss)) if self.round32 else loss)
            if self.round32:
                with np.errstate(over="ignore"):
                    v = float(np.float32(v))
            if not math.isfinite(v):
                continue
            if self.counts[t] == self.H:
                self.hist[t, :-1] = self.hist[t, 1:]
                self.hist[t, -1] = v
            else:
                self.hist[t, self.counts[t]] = v
                self.counts[t] += 1
            self.pushes += 1
        return self

    def warmed_up(self):
        if self.mutant == "refresh_one_push_early":
            return int((self.H - self.counts).sum()) <= 1
        return bool((self.counts == self.H).all())

    def refresh(self):
        """(p, w) in float64; p = 1 / N and w = base_w until every ring is full (and while sum m is 0 or not finite)."""
        m = np.sqrt(np.mean(self.hist ** 2, axis=-1))
        total = m.sum()
        if not (self.warmed_up() and total > 0 and math.isfinite(total)):
            return np.full(self.N, 1.0 / self.N), self.base.copy()
        p = (1 - self.u) * (m / total) + self.u / self.N
        return p, self.base / (self.N * p)

    def emulate32(self):
        """The refresh in fp32 in the kernel's order: the squares added in ring order, a thread's timesteps in ascending
        order, the 10-level tree."""
        f = np.float32
        h = self.hist.astype(f)
        sq = np.zeros(self.N, dtype=f)
        for k in range(self.H):
            sq = sq + h[:, k] * h[:, k]
        m = np.sqrt(sq / f(self.H)).astype(f)
        trips = cdiv(self.N, 1024)
        v = np.concatenate([m, np.zeros(trips * 1024 - self.N, dtype=f)]).reshape(trips, 1024)
        acc = np.zeros(1024, dtype=f)
        for i in range(trips):
            acc = acc + v[i]
        o = 512
        while o:
            acc = acc[:o] + acc[o:2 * o]
            o //= 2
        total, fn, u = acc[0], f(self.N), f(self.u)
        base = self.base.astype(f)
        if not (self.warmed_up() and total > 0 and np.isfinite(total)):
            return np.full(self.N, f(1.0) / fn, dtype=f), base
        p = (f(1.0) - u) * (m / total) + u / fn
        return p.astype(f), (base / (fn * p)).astype(f)


def refresh_bound(mirror):
    """((p, b_p), (w, b_w), exact): the fp64 refresh of the mirror's (fp32-valued) history and its bounds; exact: the result is
    the not-warmed-up one, p = fp32(1 / N) and w = base_w bit for bit (the bounds are then 0 around those fp32 values)."""
    p, w = mirror.refresh()
    N, H = mirror.N, mirror.H
    m = np.sqrt(np.mean(mirror.hist ** 2, axis=-1))
    total = m.sum()
    if not (mirror.warmed_up() and total > 0 and math.isfinite(total)):
        p32 = np.full(N, np.float32(1.0) / np.float32(N), dtype=np.float32).astype(np.float64)
        return (p32, np.zeros(N)), (w, np.zeros(N)), True
    g = gam(2 * H + 1)
    r_m = g / 2 + U * (1 + g)
    r_t = r_m + gam(cdiv(N, 1024) + 10) * (1 + r_m)
    A, Cc = (1 - mirror.u) * (m / total), mirror.u / N
    b_p = A * (r_m + r_t + gam(3)) * (1 + 4 * U + r_m + r_t) + U * Cc + U * p
    rel = b_p / p
    b_w = w * rel / (1 - rel) + gam(2) * w * (1 + rel)
    return (p, b_p), (w, b_w), False


# (nsteps, H): one timestep, a few, a whole schedule, more timesteps than the workgroup has threads
HISTORY_SHAPES = ((1, 1), (7, 3), (1000, 10), (1500, 3), (7, 1), (1000, 1))


def history_sequence(nsteps, H, seed=0, batch=None):
    """Batches of (t, loss) that fill every ring in the LAST batch only: timesteps in a shuffled order, H rounds of them, cut
    into batches; out-of-range timesteps and NaN / inf losses are mixed in (they must change nothing), and the final batch
    goes on past the fill, so that rings shift."""
    rng = np.random.RandomState(seed + 13 * nsteps + H)
    ts = np.concatenate([rng.permutation(nsteps) for _ in range(H)]).astype(np.int64)
    losses = rng.lognormal(-1.0, 1.0, size=ts.shape).astype(np.float32)
    batch = batch or max(3, min(64, (len(ts) + 3) // 4))
    out = []
    for lo in range(0, len(ts), batch):
        t, l = ts[lo:lo + batch].copy(), losses[lo:lo + batch].copy()
        junk_t = np.array([-1, nsteps, nsteps + 7, int(t[0]), int(t[0])], dtype=np.int64)
        junk_l = np.array([0.5, 0.25, 1.0, np.nan, np.inf], dtype=np.float32)
        out.append((np.concatenate([junk_t[:3], t, junk_t[3:]]), np.concatenate([junk_l[:3], l, junk_l[3:]])))
    extra_t = rng.randint(0, nsteps, size=5).astype(np.int64)
    last_t, last_l = out[-1]
    out[-1] = (np.concatenate([last_t, extra_t]), np.concatenate([last_l, rng.lognormal(0.0, 1.0, size=5).astype(np.float32)]))
    return out
