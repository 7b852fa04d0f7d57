"""The labelling pass without a device: the refusals of hig_q_sample_pit and hig_pair_vote (every check runs before anything
touches a device: the pointers are host memory and are never dereferenced), opt.label_pass, and the two host functions that
turn per-batch votes into the reference's `learned_indices` and file labels -- held to a plain restatement of the reference's
bookkeeping (lists appended in its loop order, `Counter(...).most_common()[0][0]`), tie rule included, and to what the
reference itself returned (golden g22, tools/make_golden_label.py)."""
import ctypes as C
import json
import os
import types
from collections import Counter

import numpy as np
import pytest

import hig_amd
from hig_amd import _lib
from hig_amd.trainers import mul_ddpm_trainer as MT

EINVAL = -1
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_label_votes.npz")


def host_buffers(n):
    raw = (C.c_float * (64 * n + 16))()
    base = (C.addressof(raw) + 15) // 16 * 16
    return raw, [C.c_void_p(base + 256 * i) for i in range(n)]


def test_pair_vote_refuses_bad_arguments_on_the_host():
    L = _lib.lib()
    assert _lib.EINVAL == EINVAL
    keep, (pred, tgt, length, votes, first, assign, scratch) = host_buffers(7)
    good = dict(pred=pred, target2=tgt, length=length, R=8, T=3, F=5, votes=votes, first=first, assign_loss=assign, scratch=scratch)

    def call(**kw):
        a = dict(good, **kw)
        return L.hig_pair_vote(a["pred"], a["target2"], a["length"], a["R"], a["T"], a["F"], a["votes"], a["first"],
                               a["assign_loss"], a["scratch"], None)

    for kw in (dict(pred=None), dict(target2=None), dict(votes=None), dict(scratch=None), dict(R=0), dict(R=-4), dict(R=6),
               dict(R=9), dict(T=0), dict(T=-1), dict(F=3), dict(F=0)):
        assert call(**kw) == EINVAL, "hig_pair_vote accepts %s" % kw
        assert "hig_pair_vote" in _lib.last_error()
    assert (C.c_float * 4).from_address(votes.value)[:] == [0.0] * 4      # (nothing written)
    del keep


def test_q_sample_pit_refuses_bad_arguments_on_the_host():
    L = _lib.lib()
    keep, (x0, noise, t, tab, xt4) = host_buffers(5)
    good = dict(x0=x0, noise=noise, t=t, tab=tab, nsteps=1000, pairs=2, per_sample=4, xt4=xt4)

    def call(**kw):
        a = dict(good, **kw)
        return L.hig_q_sample_pit(a["x0"], a["noise"], a["t"], a["tab"], a["nsteps"], a["pairs"], a["per_sample"], a["xt4"], None)

    for kw in (dict(x0=None), dict(noise=None), dict(t=None), dict(tab=None), dict(xt4=None), dict(nsteps=0), dict(pairs=0),
               dict(pairs=-1), dict(per_sample=0), dict(per_sample=-3), dict(pairs=2 ** 30, per_sample=2 ** 62)):
        assert call(**kw) == EINVAL, "hig_q_sample_pit accepts %s" % kw
        assert "hig_q_sample_pit" in _lib.last_error()
    del keep


def tiny(**kw):
    return hig_amd.MotionInteractionTransformer(input_feats=12, num_frames=16, latent_dim=64, ff_size=128, num_layers=2, num_heads=8,
                                                text_latent_dim=32, cap_id=True, **kw)


def test_label_pass_default_and_refusal():
    opt = types.SimpleNamespace(device="cpu", diffusion_steps=1000, is_train=False, multi=True, label_path=None, cap_id=True)
    assert MT.label_pass_option(opt) == "torch"
    hig_amd.DDPMMulTrainer(opt, tiny())
    for v in ("torch", "hip"):
        opt.label_pass = v
        assert MT.label_pass_option(opt) == v
        hig_amd.DDPMMulTrainer(opt, tiny())
    for bad in ("HIP", "", None, 1, "graph"):
        opt.label_pass = bad
        with pytest.raises(ValueError, match="label_pass"):
            MT.label_pass_option(opt)
        with pytest.raises(ValueError, match="label_pass"):
            hig_amd.DDPMMulTrainer(opt, tiny())
    assert list(MT.LABEL_STEPS) == [830, 860, 890, 920]


# ---- the reference's bookkeeping, restated plainly: decisions[b] is (steps, draws, pairs) of batch b ------------------------------
def reference_model_mode(batches, max_class_num=42):
    """eval_data with learned_indices = None: timestep-outer, batch-inner, draw, pair."""
    merged = {}
    steps = batches[0][2].shape[0]
    for s in range(steps):
        for ids1, ids2, dec in batches:
            for d in range(dec.shape[1]):
                active_list = {}
                for i, res in enumerate(dec[s, d]):
                    a, b = int(ids1[i]), int(ids2[i])
                    key = str(a) + '_' + str(b)
                    active_list.setdefault(key, []).append(str(a) + '_' + str(b) if res == 0 else str(b) + '_' + str(a))
                for key in active_list:
                    merged.setdefault(key, []).extend(active_list[key])
    learned = []
    for i in range(max_class_num + 1):
        if str(i - 1) + '_' + str(i) in merged:
            continue
        elif str(i) + '_' + str(i + 1) in merged:
            num1, num2 = Counter(merged[str(i) + '_' + str(i + 1)]).most_common()[0][0].split('_')
            learned += [int(num1), int(num2)]
        else:
            learned.append(i)
    return learned


def reference_label_mode(file_ids, active, dec):
    """eval_data with learned_indices, one batch: timestep, draw, pair."""
    lists = {}
    for s in range(dec.shape[0]):
        for d in range(dec.shape[1]):
            for i, fid in enumerate(file_ids):
                lists.setdefault(fid, []).append(0 if dec[s, d, i] == active[i] else 1)
    return [(fid, Counter(v).most_common()[0][0]) for fid, v in lists.items()]


def votes_of(dec):
    """What label_votes returns for these decisions: votes (steps, pairs, 2) and first (pairs,)."""
    votes = np.stack([(dec == a).sum(axis=1) for a in (0, 1)], axis=-1)
    return votes, dec[0, 0].copy()


def decisions(steps, draws, ones):
    """(steps, draws, pairs): pair p takes assignment 1 in exactly the (step, draw) cells listed in ones[p] (flat indices)."""
    dec = np.zeros((steps * draws, len(ones)), dtype=np.int64)
    for p, cells in enumerate(ones):
        dec[list(cells), p] = 1
    return dec.reshape(steps, draws, len(ones))


def check_model_mode(batches, max_class_num=42):
    got = MT.learned_indices_from_votes([(i1, i2) + votes_of(dec) for i1, i2, dec in batches], max_class_num)
    want = reference_model_mode(batches, max_class_num)
    assert got == want, (got, want)
    return got


def test_label_mode_majority_and_the_tie_rule_both_ways():
    file_ids, active = ["a", "b", "c", "d"], np.array([0, 1, 0, 1])
    n = 4 * 41
    #        clear majority of 1      82 / 82, first draw 0     82 / 82, first draw 1        all 0
    ones = [range(3, 120), range(82, n), range(0, 82), ()]
    dec = decisions(4, 41, ones)
    assert dec[:, :, 1].sum() == 82 and dec[:, :, 2].sum() == 82 and dec[0, 0, 1] == 0 and dec[0, 0, 2] == 1
    votes, first = votes_of(dec)
    got = MT.file_labels_from_votes(file_ids, active, votes, first)
    want = reference_label_mode(file_ids, active, dec)
    assert list(got.items()) == want
    # pair 1: active 1, first decision 0 -> the first output is 1 and wins the tie; pair 2: active 0, first decision 1 -> 1
    assert got == {"a": 1, "b": 1, "c": 1, "d": 1}
    active2 = np.array([1, 0, 1, 0])
    got2 = MT.file_labels_from_votes(file_ids, active2, votes, first)
    assert list(got2.items()) == reference_label_mode(file_ids, active2, dec) and got2 == {"a": 0, "b": 0, "c": 0, "d": 0}
    # the count decides before `first` does: one vote more for the value that did not come first
    dec3 = decisions(4, 41, [range(81, n), range(0, 81)])
    v3, f3 = votes_of(dec3)
    assert list(MT.file_labels_from_votes(["x", "y"], [0, 0], v3, f3).items()) == reference_label_mode(["x", "y"], [0, 0], dec3) \
        == [("x", 1), ("y", 0)]
    # a file id that occurs twice in a batch shares one list
    dec4 = decisions(2, 3, [(0, 1, 2), (3,), ()])
    v4, f4 = votes_of(dec4)
    assert list(MT.file_labels_from_votes(["x", "x", "y"], [0, 1, 0], v4, f4).items()) == \
        reference_label_mode(["x", "x", "y"], [0, 1, 0], dec4)


def test_model_mode_majority_ties_across_batches_partnerless_classes_and_max_class_num():
    # a clear majority, in one batch
    got = check_model_mode([([0, 2], [1, 3], decisions(4, 5, [range(0, 15), range(0, 3)]))])
    assert got[:4] == [1, 0, 2, 3] and got[4:] == list(range(4, 43))
    # the key 4_5 in three batches, 30 / 30 over them; the loader's first batch with the key decides through its first draw
    b0 = ([0, 9], [1, 10], decisions(4, 5, [(), ()]))                                   # (no 4_5 here)
    b1 = ([4, 2], [5, 3], decisions(4, 5, [range(10, 20), ()]))                         # first draw: 0
    b2 = ([4, 4], [5, 5], decisions(4, 5, [range(0, 20), ()]))                          # all 1 | all 0
    assert sum(int(d[:, :, [i for i, a in enumerate(i1) if a == 4]].sum()) for i1, _, d in (b1, b2)) == 30
    assert check_model_mode([b0, b1, b2])[4:6] == [4, 5]
    # ... and the other way: the first batch with the key opens with assignment 1, although a later batch opens with 0
    b1r = ([4, 2], [5, 3], decisions(4, 5, [range(0, 10), ()]))
    assert check_model_mode([b0, b1r, b2])[4:6] == [5, 4]
    # within one batch the lowest pair index with the key decides
    b3 = ([7, 4, 4], [8, 5, 5], decisions(2, 5, [(), range(0, 5), range(5, 10)]))       # 10 / 10, pair 1 opens with 1
    assert check_model_mode([b3])[4:6] == [5, 4]
    b3r = ([7, 4, 4], [8, 5, 5], decisions(2, 5, [(), range(5, 10), range(0, 5)]))
    assert check_model_mode([b3r])[4:6] == [4, 5]
    # a tie whose first value was cast at the first TIMESTEP of a later batch: batch-outer order must not name batch 0's later draws
    c0 = ([1], [9], decisions(4, 5, [()]))
    c1 = ([4], [5], decisions(4, 5, [range(0, 10)]))
    assert check_model_mode([c0, c1])[4:6] == [5, 4]
    # classes without a partner, keys that are not (i, i + 1), a key whose predecessor exists (skipped), a == b
    odd = ([0, 5, 11, 20, 30], [1, 3, 12, 20, 29], decisions(4, 5, [range(0, 20), range(0, 20), range(0, 20), (), range(0, 20)]))
    got = check_model_mode([odd])
    assert got[:2] == [1, 0] and 12 in got and got.index(12) < got.index(11)
    # max_class_num: the list stops there, a pair at its edge still contributes both numbers
    edge = ([41, 5], [42, 6], decisions(4, 5, [range(0, 20), ()]))
    for m in (42, 41, 6, 5):
        check_model_mode([edge], max_class_num=m)
    assert check_model_mode([edge], 41)[-2:] == [42, 41] and len(check_model_mode([edge], 5)) == 7


def test_random_decisions_agree_with_the_restatement():
    g = np.random.RandomState(7)
    for trial in range(40):
        nb = g.randint(1, 4)
        batches = []
        for _ in range(nb):
            pairs = g.randint(1, 5)
            ids1 = g.randint(0, 6, pairs)
            ids2 = np.where(g.rand(pairs) < 0.7, ids1 + 1, g.randint(0, 6, pairs))
            batches.append((ids1, ids2, (g.rand(4, 2, pairs) < 0.5).astype(np.int64)))     # 8 draws: ties are common
        check_model_mode(batches, max_class_num=7)
        ids1, ids2, dec = batches[0]
        learned = list(g.permutation(8))
        active = MT.label_active_indices(learned, ids1, ids2)
        fids = ["f%d" % g.randint(0, 3) for _ in ids1]
        assert list(MT.file_labels_from_votes(fids, active, *votes_of(dec)).items()) == reference_label_mode(fids, active, dec)


def test_g22_returns_follow_from_its_decisions():
    """What the reference's label_batch returned, per draw, from the stored decisions; and its eval_data bookkeeping over
    those draws from the votes."""
    g = np.load(GOLD)
    ids1, ids2, dec, learned = g["ids1"], g["ids2"], g["decisions"], g["learned_indices"].tolist()
    file_ids = [str(f) for f in g["file_ids"]]
    assert g["min_margin"] >= 1e-3 and dec.shape == (4, 3, 6) and set(np.unique(dec)) == {0, 1}
    active = MT.label_active_indices(learned, ids1, ids2)
    for s in range(dec.shape[0]):
        for d in range(dec.shape[1]):
            one = dec[s:s + 1, d:d + 1]
            votes, first = votes_of(one)
            # one draw: the votes ARE the decisions, so the two functions must give label_batch's returns back
            active_list = json.loads(str(g["active_list"][s, d]))
            for key, values in active_list.items():
                a, b = key.split("_")
                rows = [p for p in range(len(ids1)) if (int(ids1[p]), int(ids2[p])) == (int(a), int(b))]
                assert values == ["%s_%s" % ((a, b) if votes[0, p, 0] else (b, a)) for p in rows]
            outs = MT.file_labels_from_votes(file_ids, active, votes, first)
            assert list(outs) == file_ids and list(outs.values()) == g["outs"][s, d].tolist()
    votes, first = votes_of(dec)
    assert MT.learned_indices_from_votes([(ids1, ids2, votes, first)]) == reference_model_mode([(ids1, ids2, dec)])
    assert list(MT.file_labels_from_votes(file_ids, active, votes, first).items()) == reference_label_mode(file_ids, active, dec)


# ---- tests/label_bounds.py: the cases decide, the bound takes fp32 in the kernel's order and rejects a wrong row mapping ---------
def test_vote_cases_are_decided_and_the_bound_has_teeth():
    import torch
    import boundary_bounds as bb
    import label_bounds as lb
    for R, T, F, with_len in lb.VOTE_SHAPES:
        pred, target2, length = lb.vote_case(R, T, F, with_len)
        b = lb.vote_bound(pred, target2, length)
        ref, bound = b["l"]
        assert lb.all_decided(b), (R, T, F, with_len, b["margin"].min())
        ties = lb.VOTE_TIE.get((R, T, F), ())
        assert b["tie"].nonzero().flatten().tolist() == list(ties) and (b["a"][list(ties)] == 0).all()
        assert (ref[0][list(ties)] == ref[1][list(ties)]).all()
        assert 0 < int(b["a"].sum()) or R // 4 - len(ties) < 2
        l32, a32 = lb.vote_eval(pred, target2, length, dtype=bb.F32, kernel_order=True)
        assert ((l32.double() - ref).abs() <= bound).all() and torch.equal(a32, b["a"])
        # NaN where nothing is read changes nothing
        pn, tn = lb.vote_poison(pred, target2, length)
        assert torch.isnan(pn).any() or (T == 1 and F == 4 and not with_len)
        lp, ap = lb.vote_eval(pn, tn, length)
        assert torch.equal(lp, ref) and torch.equal(ap, b["a"])
        # scored against its own half of the noise, not against the 4-row order [n1, n2, n1, n2]
        if R > 4:
            P = R // 4
            wrong = torch.cat([target2[:P], target2[P:], target2[:P], target2[P:]])
            ev = bb.pair_eval(pred, wrong, length, 1, dtype=bb.F32, kernel_order=True)
            lw = torch.stack([ev["S0"], ev["S1"]])
            assert not ((lw.double() - ref).abs() <= bound).all()
