"""The labelling pass on the MI355X: hig_q_sample_pit and hig_pair_vote (csrc/ddpm.hip) in guarded buffers, and
DDPMMulTrainer.label_votes / eval_data(opt.label_pass="hip") over cap_id models -- against the reference's own label_batch
(golden g22, tools/make_golden_label.py), against this project's label_batch path, captured against eager.

References, bounds and cases are those of tests/label_bounds.py (on top of tests/boundary_bounds.py); the entry points are
called directly under the rules of tests/test_gpu_boundary_contract.py: float outputs live in a `Buf` (NaN-pattern filled, guarded
above and below, checked to be fully written), the int32 outputs in a `Band` of the same kind, the scratch is exactly R floats,
pred and target2 hold NaN wherever the contract says they are never read, and a message carries the largest |error| / bound.

Measured on an MI355X (largest |error| / bound over all cases; the bounds are derived in tests/label_bounds.py, the ratios are
the only measurements):
    output                          bound                                                   ratio  at
    hig_pair_vote.assign_loss       b_row + b_row' + u (l + b_row + b_row')                 0.172  1028x2x4 (0.013 .. 0.122 elsewhere)
    hig_pair_vote rowloss (scratch) b_row of tests/boundary_bounds.py                       0.184  1028x2x4
    hig_pair_vote decision          margin > 4 or a tie by construction                     equal  every pair (smallest margin 8.3e4)
    hig_q_sample_pit                hig_q_sample + the four-way cat                         exact  every case
    the pass against g22            rel <= max(1e-6, 4 x the reference's fp32 distance)     0.488  value 32 (rel 4.9e-7 under the 1e-6 floor)
Against g22 the largest relative distance of an assignment sum from the reference's fp64 run is 3.3e-6, where the reference's
own fp32 run is 3.1e-6 away; all 72 decisions are the reference's.  The row sums sit where hig_pair_mse's do (0.18 of a bound
that adds worst cases over a tree).
"""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hig_amd import _lib  # noqa: E402
from hig_amd.models import gaussian_diffusion as gdm  # noqa: E402
from hig_amd.trainers import mul_ddpm_trainer as MT  # noqa: E402
from oracle import fill  # noqa: E402
from oracle import synth_dataset as SD  # noqa: E402
from test_gpu_rowops_contract import Buf, P, S, lib, ok  # noqa: E402
from test_gpu_boundary_contract import bits, held  # noqa: E402
import boundary_bounds as bb  # noqa: E402
import class_head_worker as W  # noqa: E402
import label_bounds as lb  # noqa: E402

DEV = "cuda"
GUARD = 64
PATTERN = 0x7FC0BEEF    # a NaN the kernels never produce, and no vote count
NSTEPS = 1000
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_label_votes.npz")


class Band:
    """`n` 32-bit words at `offset` words past a 16-byte boundary, guard bands of GUARD words either side."""

    def __init__(self, n, offset=0, dtype=torch.float32, fill=None):
        self.n, self.lo = n, GUARD + offset
        self.buf = torch.full((GUARD + offset + n + GUARD + 4,), PATTERN, dtype=torch.int32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.out = self.buf[self.lo:self.lo + n].view(dtype)
        if fill is not None:
            self.out.fill_(fill)

    def p(self):
        return C.c_void_p(self.out.data_ptr())

    def guards(self, what):
        assert bool((self.buf[:self.lo] == PATTERN).all() and (self.buf[self.lo + self.n:] == PATTERN).all()), \
            "%s: a store landed in a guard band" % what

    def written(self, what):
        self.guards(what)
        assert bool((self.buf[self.lo:self.lo + self.n] != PATTERN).all()), "%s: not every element was written" % what
        return self.out.cpu()

    def read(self, what):
        self.guards(what)
        return self.out.cpu()


def placed(t, offset):
    """A copy of the fp32 tensor `t` whose base is `offset` floats past a 16-byte boundary."""
    raw = torch.empty(t.numel() + 8, device=DEV)
    view = raw[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


@functools.lru_cache(maxsize=None)
def diffusion():
    return gdm.GaussianDiffusion(betas=gdm.get_named_beta_schedule("linear", NSTEPS), model_mean_type=gdm.ModelMeanType.EPSILON,
                                 model_var_type=gdm.ModelVarType.FIXED_SMALL, loss_type=gdm.LossType.MSE)


# ----------------------------------------------------------------------------------------------------------------------
# hig_q_sample_pit
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sample", [15, 84, 16 * 263])
@pytest.mark.parametrize("pairs", [1, 3, 4, 5])
def test_q_sample_pit_is_q_sample_and_the_four_way_cat(pairs, per_sample):
    """pairs * per_sample % 4 != 0 takes the scalar stream whatever the alignment; pairs = 4 with per_sample = 15 puts float4
    groups across sample boundaries (a different t either side)."""
    g = torch.Generator().manual_seed(100 * pairs + per_sample)
    rows = 2 * pairs
    x0, nz = torch.randn(rows, per_sample, generator=g) * 3, torch.randn(rows, per_sample, generator=g)
    t = torch.randperm(NSTEPS, generator=g)[:rows]                   # a different t per row
    tab, td = diffusion().device_table(torch.device(DEV)), t.to(DEV)
    want = Buf.flat(rows * per_sample)
    x0d, nzd = x0.to(DEV), nz.to(DEV)
    ok(lib().hig_q_sample(P(x0d), P(nzd), P(td), P(tab), NSTEPS, rows, per_sample, want.p(), S()))
    q = want.written("hig_q_sample").view(rows, per_sample)
    want4 = torch.cat([q[:pairs], q[:pairs], q[pairs:], q[pairs:]])
    results = []
    for off_x, off_n, off_o in ((0, 0, 0), (0, 0, 0), (1, 1, 1), (0, 0, 1), (1, 0, 0), (0, 2, 0)):      # aligned twice, then unaligned bases
        what = "hig_q_sample_pit pairs %d per_sample %d offsets %d %d %d" % (pairs, per_sample, off_x, off_n, off_o)
        xd, nd = placed(x0.to(DEV), off_x), placed(nz.to(DEV), off_n)
        out = Band(4 * pairs * per_sample, off_o)
        ok(lib().hig_q_sample_pit(P(xd), P(nd), P(td), P(tab), NSTEPS, pairs, per_sample, out.p(), S()))
        got = out.written(what).view(4 * pairs, per_sample)
        assert torch.equal(bits(got), bits(want4)), "%s: %d elements differ from hig_q_sample + cat" % (
            what, int((bits(got) != bits(want4)).sum()))
        assert torch.equal(xd.cpu(), x0) and torch.equal(nd.cpu(), nz), what + ": an input changed"
        results.append(got)
    assert all(torch.equal(bits(r), bits(results[0])) for r in results)


# ----------------------------------------------------------------------------------------------------------------------
# hig_pair_vote
# ----------------------------------------------------------------------------------------------------------------------
def swap_assignments(pred, length):
    """The same pairs with the two caption assignments exchanged: every decided pair decides the other way."""
    R = pred.shape[0]
    Pn = R // 4
    order = torch.cat([torch.arange(Pn, 2 * Pn), torch.arange(0, Pn), torch.arange(3 * Pn, R), torch.arange(2 * Pn, 3 * Pn)])
    return pred[order].contiguous(), None if length is None else length[order].contiguous()


class VoteRun:
    """One set of guarded outputs; `launch` casts one vote per pair."""

    def __init__(self, R, what, with_first=True, with_assign=True):
        self.R, self.Pn, self.what = R, R // 4, what
        self.votes = Band(2 * self.Pn, dtype=torch.int32, fill=0)
        self.first = Band(self.Pn, dtype=torch.int32)
        self.assign, self.scratch = Buf.flat(2 * self.Pn), Buf.flat(R)
        self.with_first, self.with_assign = with_first, with_assign

    def launch(self, pred, target2, length):
        R, T, F = pred.shape
        pd, tg, ln = pred.to(DEV), target2.to(DEV), None if length is None else length.to(DEV)
        ok(lib().hig_pair_vote(P(pd), P(tg), P(ln), R, T, F, self.votes.p(), self.first.p() if self.with_first else None,
                               self.assign.p() if self.with_assign else None, self.scratch.p(), S()))
        return self

    def read(self, nan_ok=False):
        """votes (P, 2), first (P), assign_loss (2, P) or None, scratch (R); nan_ok: a NaN sum is expected, guards only."""
        first = self.first.read(self.what + " first")
        if not self.with_first:
            assert (first == PATTERN).all(), self.what + ": first = NULL was written"
        if not self.with_assign:
            self.assign.untouched(self.what + " assign_loss = NULL")
        if nan_ok:
            self.assign.guards(self.what + " assign_loss")
            self.scratch.guards(self.what + " scratch")
            return (self.votes.read(self.what + " votes").view(self.Pn, 2), first, self.assign.out.cpu().view(2, self.Pn),
                    self.scratch.out.cpu()[0])
        return (self.votes.read(self.what + " votes").view(self.Pn, 2), first,
                self.assign.written(self.what + " assign_loss").view(2, self.Pn) if self.with_assign else None,
                self.scratch.written(self.what + " scratch")[0])


@pytest.mark.parametrize("R,T,F,with_len", lb.VOTE_SHAPES)
def test_pair_vote(R, T, F, with_len):
    what = "hig_pair_vote %dx%dx%d%s" % (R, T, F, "" if with_len else "_nolen")
    Pn = R // 4
    pred, target2, length = lb.vote_case(R, T, F, with_len)
    b = lb.vote_bound(pred, target2, length)
    assert lb.all_decided(b), "%s: a pair of the case is neither decided (margin > %g) nor a tie by construction" % (what, bb.PAIR_MARGIN)
    print("MARGIN %s smallest %.3g" % (what, b["margin"][~b["tie"]].min() if (~b["tie"]).any() else float("inf")))
    pn, tn = lb.vote_poison(pred, target2, length)
    a_ref = b["a"]

    # one launch: the sums within their bound of fp64, the decision the fp64 decision, a tie 0
    votes, first, assign, scratch = VoteRun(R, what).launch(pn, tn, length).read()
    assert torch.isfinite(assign).all(), "%s: an assignment sum is %s: a masked position was read" % (what, assign)
    held(what.replace(" ", ".assign_loss ", 1), assign, *b["l"])
    held(what.replace(" ", ".rowloss ", 1), scratch, *bb.pair_bound(pred, lb.expand_target(target2), length, 1)["rowloss"])
    a_dev = (assign[1] < assign[0]).to(torch.int64)
    wrong = (a_dev != a_ref).nonzero().flatten().tolist()
    assert not wrong, "%s: pairs %s take the other assignment (margins %s, ties %s)" % (
        what, wrong[:8], b["margin"][wrong[:8]].tolist(), b["tie"][wrong[:8]].tolist())
    assert (a_dev[b["tie"]] == 0).all(), "%s: a tie does not take assignment 0" % what
    assert torch.equal(first.long(), a_ref), "%s: first is not the decision" % what
    want = torch.zeros(Pn, 2, dtype=torch.int64)
    want[torch.arange(Pn), a_ref] = 1
    assert torch.equal(votes.long(), want), "%s: votes after one launch" % what

    # the assignment hig_pair_mse(pit = 1) takes on the same pred, the target expanded to R rows for it
    lo, sc, d = Buf.flat(1), Buf.flat(2 * R), Buf.flat(R * T * F)
    ln = None if length is None else length.to(DEV)
    pnd, tn4 = pn.to(DEV), lb.expand_target(tn).to(DEV)
    ok(lib().hig_pair_mse(P(pnd), P(tn4), P(ln), R, T, F, 1, lo.p(), d.p(), sc.p(), S()))
    dp = d.written(what + " hig_pair_mse dpred").view(R, T * F)
    nz = (dp != 0).any(dim=1)
    says0, says1 = nz[:Pn] | nz[2 * Pn:3 * Pn], nz[Pn:2 * Pn] | nz[3 * Pn:]
    assert not (says0 & says1).any(), "hig_pair_mse gave both assignments of a pair a gradient"
    assert (a_dev[says0] == 0).all() and (a_dev[says1] == 1).all(), "%s: not hig_pair_mse's assignment (dpred)" % what
    rowscale = sc.written(what + " hig_pair_mse scratch")[0][R:]
    assert torch.equal(a_dev, (rowscale[:Pn] == 0).to(torch.int64)), "%s: not hig_pair_mse's assignment (rowscale)" % what
    assert (says0 | says1).any(), "dpred is silent on every pair"      # (silent where both chosen rows are off the mask)

    # three launches accumulate; first is written by the first launch only; first = NULL / assign_loss = NULL change nothing
    ps, ls = swap_assignments(pred, length)
    psn, tsn = lb.vote_poison(ps, target2, ls)
    a_swapped = lb.vote_bound(ps, target2, ls)["a"]
    assert torch.equal(a_swapped[~b["tie"]], 1 - a_ref[~b["tie"]]) and (a_swapped[b["tie"]] == 0).all()
    runs = []
    for k in range(2):
        run = VoteRun(R, what + " x3")
        run.launch(pn, tn, length).launch(psn, tsn, ls).launch(psn, tsn, ls)
        runs.append(run.read())
    votes3, first3, assign3, scratch3 = runs[0]
    want3 = want.clone()
    want3[torch.arange(Pn), a_swapped] += 2
    assert torch.equal(votes3.long(), want3), "%s: votes after three launches" % what
    assert torch.equal(first3.long(), a_ref), "%s: first was rewritten by a later launch" % what
    for x, y in zip(runs[0], runs[1]):
        assert torch.equal(bits(x), bits(y)), "%s: two runs differ" % what
    bare = VoteRun(R, what + " NULLs", with_first=False, with_assign=False).launch(pn, tn, length)
    votes_b, _, _, scratch_b = bare.read()
    assert torch.equal(votes_b, votes) and torch.equal(bits(scratch_b), bits(scratch)), "%s: first / assign_loss = NULL change the vote" % what

    # a pair with a NaN sum: no vote, no first, while its neighbours vote
    Lc = torch.full((R,), T) if length is None else length.clamp(0, T)
    p_nan = next(p for p in range(Pn) if Lc[p] > 0 and not b["tie"][p])
    bad = pn.clone()
    bad[p_nan, 0, 0] = float("nan")
    votes_n, first_n, assign_n, _ = VoteRun(R, what + " NaN").launch(bad, tn, length).read(nan_ok=True)
    others = torch.arange(Pn) != p_nan
    assert torch.isnan(assign_n[0, p_nan]) and torch.equal(bits(assign_n[:, others]), bits(assign[:, others]))
    assert (votes_n[p_nan] == 0).all() and first_n[p_nan] == PATTERN, "%s: a pair with a NaN sum voted" % what
    assert torch.equal(votes_n[others], votes[others]) and torch.equal(first_n[others], first[others]), \
        "%s: the neighbours of a NaN pair did not vote as before" % what


def test_pair_vote_is_capturable():
    R, T, F = 12, 2, 5
    pred, target2, length = lb.vote_case(R, T, F, True)
    pd, tg, ln = pred.to(DEV), target2.to(DEV), length.to(DEV)
    votes, first = torch.zeros(R // 4, 2, dtype=torch.int32, device=DEV), torch.full((R // 4,), -1, dtype=torch.int32, device=DEV)
    assign, scratch = torch.zeros(2, R // 4, device=DEV), torch.zeros(R, device=DEV)

    def launch():
        _lib.check(lib().hig_pair_vote(P(pd), P(tg), P(ln), R, T, F, P(votes), P(first), P(assign), P(scratch), S()))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()
    torch.cuda.current_stream().wait_stream(s)
    votes.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        launch()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    a = lb.vote_bound(pred, target2, length)["a"]
    want = torch.zeros(R // 4, 2, dtype=torch.int64)
    want[torch.arange(R // 4), a] = 5
    assert torch.equal(votes.cpu().long(), want) and torch.equal(first.cpu().long(), a)


# ----------------------------------------------------------------------------------------------------------------------
# the loop: DDPMMulTrainer.label_votes
# ----------------------------------------------------------------------------------------------------------------------
G22 = np.load(GOLD)
CASE = dict(fill.ICASES["tiny2"], B=6, lengths=tuple(G22["lengths"].tolist()))
CASE16 = dict(B=6, T=33, F=12, d=128, H=2, L=2, ff=96, N=77, Lt=32, num_frames=40)       # what the bf16 two-person tests run
STEPS = G22["steps"].tolist()


@functools.lru_cache(maxsize=None)
def trainer(class_head="hip", storage="f32", case="tiny2"):
    return W.pit_trainer(CASE if case == "tiny2" else CASE16, storage=storage, class_head=class_head)[0]


def g22_batch(T=None, F=None):
    """g22's batch; other T / F (the bf16 case): motions of that shape under their own names, the same ids and lengths."""
    c = CASE
    if T is None:
        m1, m2 = (fill.tensor_for("g22.motion%d" % k, (c["B"], c["T"], c["F"])) * 10 for k in (1, 2))
    else:
        m1, m2 = (fill.tensor_for("g22.wide.motion%d" % k, (c["B"], T, F)) * 10 for k in (1, 2))
    return ([torch.from_numpy(G22["ids1"])], [torch.from_numpy(G22["ids2"])], m1, m2, torch.from_numpy(G22["lengths"]),
            [str(f) for f in G22["file_ids"]])


def g22_noise():
    if "noise" in G22.files:
        return torch.from_numpy(G22["noise"])
    c, (ns, nd) = CASE, G22["decisions"].shape[:2]
    return torch.stack([fill.tensor_for("g22.noise.%d" % k, (2 * c["B"], c["T"], c["F"])) * 10 for k in range(ns * nd)]).view(
        ns, nd, 2 * c["B"], c["T"], c["F"])


@functools.lru_cache(maxsize=None)
def g22_run(captured=True, class_head="hip"):
    return trainer(class_head).label_votes(g22_batch(), STEPS, draws=3, noise=g22_noise(), captured=captured, losses=True)


def votes_from(dec):
    return np.stack([(dec == a).sum(axis=1) for a in (0, 1)], axis=-1)


def test_label_votes_decides_as_the_reference_on_g22():
    r = g22_run()
    l = r["assign_loss"]
    dec = (l[:, :, 1] < l[:, :, 0]).astype(np.int64)
    assert np.array_equal(r["votes"], votes_from(dec)) and np.array_equal(r["first"], dec[0, 0])
    assert dec.shape == G22["decisions"].shape == (4, 3, 6)
    wrong = np.argwhere(dec != G22["decisions"])
    assert not len(wrong), "(step, draw, pair) %s decide against the reference" % wrong.tolist()
    rel = torch.from_numpy(np.abs(l.astype(np.float64) - G22["l64"]) / np.abs(G22["l64"]))
    gate = lb.sums_gate(G22["l32"], G22["l64"])
    q = rel / gate
    at = int(q.argmax())
    print("RATIO label_votes.g22 %.3f at %d (rel %.3g, gate %.3g; largest rel %.3g, the reference's own %.3g)" % (
        q.reshape(-1)[at], at, rel.reshape(-1)[at], gate.reshape(-1)[at], rel.max(), float(gate.max()) / 4))
    assert q.max() <= 1.0, "assignment sum %d: rel %.3g from the reference's fp64 run, gate %.3g" % (
        at, rel.reshape(-1)[at], gate.reshape(-1)[at])


def test_label_batch_decides_the_same_on_the_same_noise(monkeypatch):
    tr, batch, noise = trainer(), g22_batch(), g22_noise().to(DEV)
    ids1, ids2 = G22["ids1"].tolist(), G22["ids2"].tolist()
    dec = np.zeros_like(G22["decisions"])
    for si, t in enumerate(STEPS):
        for d in range(dec.shape[1]):
            monkeypatch.setattr(torch, "randn_like", lambda x, **k: noise[si, d].clone())
            with torch.no_grad():
                active_list = tr.label_batch(batch, None, t=t)
            monkeypatch.undo()
            for p, (a, b) in enumerate(zip(ids1, ids2)):
                v = active_list["%d_%d" % (a, b)].pop(0)
                assert v in ("%d_%d" % (a, b), "%d_%d" % (b, a))
                dec[si, d, p] = 0 if v == "%d_%d" % (a, b) else 1
    r = g22_run()
    assert np.array_equal(votes_from(dec), r["votes"]) and np.array_equal(dec[0, 0], r["first"])
    assert np.array_equal(dec, G22["decisions"])


def test_captured_equals_eager_bit_for_bit_over_two_calls():
    tr, batch, noise = trainer(), g22_batch(), g22_noise()
    runs = [tr.label_votes(batch, STEPS, draws=3, noise=noise, captured=cap, losses=True) for cap in (True, False, True, False)]
    for r in runs[1:]:
        assert np.array_equal(r["votes"], runs[0]["votes"]) and np.array_equal(r["first"], runs[0]["first"])
        assert np.array_equal(r["assign_loss"].view(np.int32), runs[0]["assign_loss"].view(np.int32))
    assert np.array_equal(runs[0]["assign_loss"].view(np.int32), g22_run()["assign_loss"].view(np.int32))


def test_hip_and_torch_class_heads_give_equal_votes():
    a, b = g22_run(), g22_run(class_head="torch")
    assert np.array_equal(a["votes"], b["votes"]) and np.array_equal(a["first"], b["first"])
    assert np.array_equal(b["votes"], votes_from(G22["decisions"]))


def test_bf16_storage_runs_and_every_pair_casts_its_votes():
    tr = trainer(storage="bf16", case="bf16")
    batch = g22_batch(CASE16["T"], CASE16["F"])
    for cap in (True, False):
        r = tr.label_votes(batch, STEPS, draws=3, captured=cap)
        assert r["votes"].shape == (4, 6, 2) and (r["votes"].sum(axis=2) == 3).all() and set(r["first"].tolist()) <= {0, 1}


def test_random_draws_give_every_pair_its_votes():
    tr, batch = trainer(), g22_batch()
    torch.manual_seed(5)
    for cap in (True, False):
        r = tr.label_votes(batch, STEPS, draws=5, captured=cap)
        assert r["votes"].shape == (4, 6, 2) and (r["votes"] >= 0).all() and (r["votes"].sum(axis=2) == 5).all()
        assert set(r["first"].tolist()) <= {0, 1} and "assign_loss" not in r
    one = tr.label_votes(batch, steps=[860], draws=2)
    assert one["votes"].shape == (1, 6, 2) and (one["votes"].sum(axis=2) == 2).all()
    with pytest.raises(ValueError, match="noise must have shape"):
        tr.label_votes(batch, STEPS, draws=3, noise=g22_noise()[:, :2])
    with pytest.raises(ValueError, match="steps"):
        tr.label_votes(batch, [1000], draws=1)


def test_a_nan_motion_raises_and_names_the_pair():
    tr, batch = trainer(), list(g22_batch())
    batch[3] = batch[3].clone()
    batch[3][2, 1, 5] = float("nan")          # person 2 of pair 2, inside its length
    for cap in (True, False):
        with pytest.raises(RuntimeError, match=r"pair 2 .*NaN.*\[2\]"):
            tr.label_votes(batch, STEPS, draws=2, captured=cap)
    r = tr.label_votes(g22_batch(), STEPS, draws=3, noise=g22_noise(), losses=True)      # and the trainer is fine afterwards
    assert np.array_equal(r["assign_loss"].view(np.int32), g22_run()["assign_loss"].view(np.int32))


# ----------------------------------------------------------------------------------------------------------------------
# eval_data under opt.label_pass
# ----------------------------------------------------------------------------------------------------------------------
TABLE = {i: caps for i, caps in enumerate(SD.CAPTIONS)}


def synth(root):
    from hig_amd.datasets.mul_dataset import Text2MotionMulDataset
    opt = SD.write(root)
    opt.cap_id, opt.is_train = True, False
    mean, std = SD.stats()
    ds = Text2MotionMulDataset(opt, mean, std, opt.split_file, caption_table=TABLE)
    c = dict(B=4, T=91, F=SD.F, d=64, H=8, L=2, ff=128, N=77, Lt=32, num_frames=90)
    return ds, c


def eval_trainer(c, **opt):
    return W.pit_trainer(c, num_workers=0, **opt)[0]


def test_eval_data_hip_model_mode_and_label_mode(tmp_path):
    ds, c = synth(str(tmp_path / "data"))
    assert len(ds) == 7                        # (4 + 3: the second batch is a short one)
    random.seed(3)                             # (the dataset draws a caption line and a window per item)
    tr = eval_trainer(c, label_pass="hip")
    calls = []
    real = tr.label_votes
    tr.label_votes = lambda *a, **k: calls.append(k.get("draws")) or real(*a, **k)
    tr.label_batch = None                      # the slow path must not be touched
    learned = tr.eval_data(ds, 0, 1, None, max_class_num=42)
    assert calls == [5, 5]
    assert len(learned) == 43 and sorted(learned) == list(range(43))
    # S001's only caption line is the pair (0, 1); whichever other keys the draws produced, a class stays or trades with a neighbour
    assert sorted(learned[0:2]) == [0, 1] and all(abs(v - i) <= 1 for i, v in enumerate(learned)) and learned[6:] == list(range(6, 43))
    out = tmp_path / "labels"
    out.mkdir()
    assert tr.eval_data(ds, 0, 1, learned, save_dir=str(out)) is None
    assert calls == [5, 5, 41, 41]
    assert sorted(os.listdir(out)) == sorted(n + ".txt" for n in ds.name_list)
    assert all((out / f).read_text() in ("0", "1") for f in os.listdir(out))
    # sharding by rank stays: rank 1 of 2 labels its own clips only
    out2 = tmp_path / "labels2"
    out2.mkdir()
    tr.eval_data(ds, 1, 2, learned, save_dir=str(out2))
    assert len(os.listdir(out2)) == 4 and calls[4:] == [41]


def test_eval_data_unset_calls_label_batch_as_before(tmp_path):
    ds, c = synth(str(tmp_path / "data"))
    tr = eval_trainer(c)
    assert MT.label_pass_option(tr.opt) == "torch"
    calls = []

    def spy(batch_data, learned_indices, t, label_mode=False):
        calls.append((t, label_mode))
        n = len(batch_data[5])
        return ([0] * n, batch_data[5]) if label_mode else {}

    tr.label_batch = spy
    tr.label_votes = None
    assert tr.eval_data(ds, 0, 1, None) == list(range(43))
    assert len(calls) == 4 * 2 * 5 and [t for t, _ in calls[::10]] == [830, 860, 890, 920] and not any(m for _, m in calls)
    del calls[:]
    out = tmp_path / "labels"
    out.mkdir()
    tr.eval_data(ds, 0, 1, list(range(43)), save_dir=str(out))
    assert len(calls) == 2 * 4 * 41 and all(m for _, m in calls) and len(os.listdir(out)) == len(ds) == 7
    assert all((out / f).read_text() == "0" for f in os.listdir(out))
