"""References, bounds and cases of the labelling pass's two kernels (csrc/ddpm.hip: hig_q_sample_pit, hig_pair_vote) and the gate
of the pass against golden g22.  Plain torch on the host, built on tests/boundary_bounds.py (imported unchanged), whose
conventions hold: u = 2^-24, gam(n) = n u / (1 - n u), no bound fitted to a measurement.

hig_pair_vote (`vote_bound`).  Row r of pred is scored against row (g / 2) P + p of target2 (g = r / P, p = r % P); expanding
target2 to [n1, n1, n2, n2] (`expand_target`) makes that hig_pair_mse's row loss on R rows, so reference and bound of a row are
`pair_bound`'s rowloss: (L[r], b_row[r]).  An assignment sum adds two computed rows in fp32, l^ = (L^[r] + L^[r'])(1 + d),
|d| <= u:
    |l^ - l| <= B + u (l + B),    B = b_row[r] + b_row[r']                                   (`l` is the fp64 sum; all terms >= 0)
-- the two rows' bounds plus one rounding of the add.
Decision.  a = (l1 < l0).  margin = |l0 - l1| / (bound(l0) + bound(l1)); a pair is DECIDED when margin > 4 (boundary_bounds.
PAIR_MARGIN: no rounding the bound admits can turn the comparison), a TIE BY CONSTRUCTION when rows P + p and 3P + p of pred and
length are bitwise copies of rows p and 2P + p (their target rows are the same rows of target2 anyway): l0 == l1 in any
arithmetic and the kernel must answer 0.  Every pair of every case is one or the other (asserted where the cases are used).

The pass against g22 (`sums_gate`): the project's form, per value: rel <= max(1e-6, 4 x the distance of the reference's own
fp32 run from its fp64 run).
"""
import torch

import boundary_bounds as bb
from boundary_bounds import F32, F64, U, gen  # noqa: F401

# (R, T, F, lengths): the smallest legal shape; F % 4 != 0 with a tie; a long row; 257 pairs, past one workgroup's threads
VOTE_SHAPES = ((4, 1, 4, True), (12, 2, 5, True), (8, 250, 263, True), (1028, 2, 4, True), (12, 2, 5, False), (8, 250, 263, False))
VOTE_TIE = {(12, 2, 5): (0,), (8, 250, 263): (1,), (1028, 2, 4): (0, 255, 256)}     # shape -> pairs that are ties by construction


def expand_target(target2):
    """(2P, ..) [n1 | n2] -> (4P, ..) [n1, n1, n2, n2]: the copy the kernel never makes."""
    P = target2.shape[0] // 2
    return torch.cat([target2[:P], target2[:P], target2[P:], target2[P:]])


def vote_lengths(R, T):
    """T, 0, 1, T + 3 and -2 in turn: the four rows of a pair take different ones (P is no multiple of 5 in any case)."""
    pat = (T, 0, 1, T + 3, -2)
    return torch.tensor([pat[r % 5] for r in range(R)], dtype=torch.int64)


def vote_case(R, T, F, with_len):
    """(pred (R, T, F), target2 (R / 2, T, F), length (R) or None) without NaN.  pred ~ 3 N(0, 1), target2 ~ N(0, 1); the pred
    rows of one assignment per pair are scaled by 4 about their target so that the other wins: the first on even pairs, the
    second on odd ones (and on the only pair of R = 4).  The pairs of VOTE_TIE are ties by construction."""
    g = gen(7 * R + T + F + int(with_len))
    P = R // 4
    pred, target2 = 3 * torch.randn(R, T, F, generator=g), torch.randn(R // 2, T, F, generator=g)
    target = expand_target(target2)
    length = vote_lengths(R, T) if with_len else None
    for p in range(P):
        second_wins = p % 2 == 1 or P == 1
        for r in ((p, 2 * P + p) if second_wins else (P + p, 3 * P + p)):
            pred[r] = target[r] + 4 * (pred[r] - target[r])
    for tie in VOTE_TIE.get((R, T, F), ()):
        for a, b in ((tie, P + tie), (2 * P + tie, 3 * P + tie)):
            pred[b] = pred[a]
            if length is not None:
                length[b] = length[a]
    return pred, target2, length


def vote_poison(pred, target2, length):
    """NaN wherever the contract says never read: pred off its row's mask and on features >= 4 of token 0; target2 where NONE of
    the two pred rows that score against it reads."""
    R, T, F = pred.shape
    P = R // 4
    live = bb.pair_live(length, R, T, F)
    nan = torch.full_like(pred, float("nan"))
    live_t = torch.cat([live[:P] | live[P:2 * P], live[2 * P:3 * P] | live[3 * P:]])
    return torch.where(live, pred, nan), torch.where(live_t, target2, nan[:2 * P])


def vote_eval(pred, target2, length, dtype=F64, kernel_order=False):
    """(l (2, P), a (P)) in `dtype`: the two assignment sums and the decision (a tie: 0)."""
    ev = bb.pair_eval(pred, expand_target(target2), length, 1, dtype=dtype, kernel_order=kernel_order)
    l = torch.stack([ev["S0"], ev["S1"]])
    return l, (l[1] < l[0]).to(torch.int64)


def vote_bound(pred, target2, length):
    """{'l': (ref (2, P), bound (2, P)), 'a' (P), 'margin' (P), 'tie' (P bool)}."""
    R = pred.shape[0]
    P = R // 4
    target = expand_target(target2)
    b = bb.pair_bound(pred, target, length, 1)
    rl, b_row = b["rowloss"]
    p = torch.arange(P)
    l = torch.stack([rl[p] + rl[2 * P + p], rl[P + p] + rl[3 * P + p]])
    B = torch.stack([b_row[p] + b_row[2 * P + p], b_row[P + p] + b_row[3 * P + p]])
    bound = B + U * (l + B)
    margin = (l[0] - l[1]).abs() / (bound[0] + bound[1])
    return {"l": (l, bound), "a": (l[1] < l[0]).to(torch.int64), "margin": margin, "tie": bb.pair_ties(pred, target, length, P)}


def all_decided(b):
    """Every pair is decided by its margin or a tie by construction."""
    return bool(((b["margin"] > bb.PAIR_MARGIN) | b["tie"]).all())


def sums_gate(l32, l64):
    """Per value: max(1e-6, 4 x the reference's own fp32 run's relative distance from its fp64 run)."""
    l32, l64 = torch.as_tensor(l32).double(), torch.as_tensor(l64).double()
    return torch.clamp_min(4 * (l32 - l64).abs() / l64.abs(), 1e-6)
