"""Proves on the CPU that the bounds of tests/boundary_bounds.py can fail -- and do not fail what is right.  At every shape of
the tables that tests/test_gpu_boundary_contract.py runs (the same inputs):
  * each MUTANT visible at the shape, evaluated in fp64, exceeds the bound on at least one element of the output named for
    it (hig_gather_frames is exact: it differs in at least one element);
  * a vectorised fp32 evaluation of the correct operation stays within the bound -- hig_pair_mse in the kernel's own order
    (lane-strided partial sums, the wave tree, the four waves, the block tree);
  * every PIT pair is decided (margin > 4) or a tie by construction, and both assignments win in every PIT case with more
    than one pair;
  * the references do not see the NaN that the GPU test puts where nothing may be read; the vectorised joint recovery equals
    oracle.motion_ref.
No GPU, no library call."""
import numpy as np
import pytest
import torch

import boundary_bounds as bb
from boundary_bounds import BF16, F32


# ----------------------------------------------------------------------------------------------------------------------
# hig_pair_mse
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,T,F,pit,with_len", bb.PAIR_SHAPES)
def test_pair_mse(R, T, F, pit, with_len):
    pred, target, length = bb.pair_case(R, T, F, pit, with_len)
    b = bb.pair_bound(pred, target, length, pit)
    if with_len:
        have = set(length.tolist())
        assert have >= ({0, 1, T, T + 5, -3} if R >= 5 else {0, 1, T, T + 5}) and (length > 0).any()
    # the reference never reads what the contract says is never read
    pn, tn = bb.pair_poison(pred, target, length)
    assert torch.isnan(pn).any() or (not with_len and F == 4)
    poisoned = bb.pair_eval(pn, tn, length, pit)
    for k in ("rowloss", "loss", "dpred"):
        assert torch.equal(poisoned[k], b[k][0]), "%s reads a masked position" % k
    if pit:
        P = R // 4
        settled = (b["margin"] > bb.PAIR_MARGIN) | b["tie"]
        assert settled.all(), "pair %d is neither decided nor a tie by construction (margin %.3g)" % (
            int((~settled).nonzero()[0]), b["margin"][~settled].min())
        tie = bb.PAIR_TIE.get((R, T, F))
        assert b["tie"].tolist() == [p == tie for p in range(P)]
        assert (b["first"] | ~b["tie"]).all() and (b["margin"][b["tie"]] == 0).all()
        assert P == 1 or (b["first"].any() and (~b["first"]).any()), "one assignment never wins"
        assert P > 1 or not b["first"].any()
    # fp32 in the kernel's order
    out = bb.pair_eval(pn, tn, length, pit, dtype=F32, kernel_order=True)
    for k in ("rowloss", "loss", "dpred"):
        r = bb.ratio(out[k], *b[k])
        assert r <= 1.0, "%s: the fp32 evaluation is at %.3f of its bound" % (k, r)
    assert torch.equal(out["rowscale"], b["rowscale32"]), "rowscale is not the correctly rounded 1 / denom of the chosen rows"
    if pit:
        assert torch.equal(out["first"], b["first"])
    for m in bb.pair_mutants(R, T, F, pit, with_len):
        key = bb.PAIR_MUTANTS[m]
        assert bb.ratio(bb.pair_eval(pred, target, length, pit, mutant=m)[key], *b[key]) > 1.0, "%s passes the bound of %s" % (m, key)


def test_every_pair_mutant_is_visible_somewhere():
    seen = set()
    for s in bb.PAIR_SHAPES:
        seen |= set(bb.pair_mutants(*s))
    assert seen == set(bb.PAIR_MUTANTS)


# ----------------------------------------------------------------------------------------------------------------------
# hig_recover_joints
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,T,J,F,init_first,with_stats", bb.RECOVER_CASES + (bb.RECOVER_LDS_CASE,))
def test_recover_joints(rows, T, J, F, init_first, with_stats):
    motion, stats = bb.recover_case(rows, T, J, F, init_first, with_stats)
    ref, bound = bb.recover_bound(motion, stats, J, init_first)
    assert ref.shape == (rows, T, J, 3)
    oracle = bb.recover_ref(motion, stats, J, init_first)
    assert (ref - oracle).abs().max() <= 1e-12 * max(1.0, oracle.abs().max().item()), "recover_eval is not oracle.motion_ref"
    if T >= 600:
        assert motion[:, 1:, 0].double().sum(1).abs().max() > 140, "the yaw does not get large"
    r = bb.ratio(bb.recover_eval(motion, stats, J, init_first, dtype=F32), ref, bound)
    assert r <= 1.0, "the fp32 evaluation is at %.3f of its bound" % r
    for m in bb.recover_mutants(rows, T, J, F, init_first, with_stats):
        assert bb.ratio(bb.recover_eval(motion, stats, J, init_first, mutant=m), ref, bound) > 1.0, "%s passes" % m


def test_every_recover_mutant_is_visible_somewhere():
    seen = set()
    for c in bb.RECOVER_CASES:
        seen |= set(bb.recover_mutants(*c))
    assert seen == set(bb.RECOVER_MUTANTS)


# ----------------------------------------------------------------------------------------------------------------------
# hig_timestep_embedding, hig_timestep_embedding_bf16
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", bb.TEMB_D)
def test_timestep_embedding(d):
    t = bb.temb_case()
    ref, bound = bb.temb_bound(t, d)
    assert ref.shape == (len(t), d)
    out = bb.temb_eval(t, d, dtype=F32)
    r = bb.ratio(out, ref, bound)
    assert r <= 1.0, "the fp32 evaluation is at %.3f of its bound" % r
    if d % 2:
        assert (ref[:, -1] == 0).all() and (bound[:, -1] == 0).all() and (out[:, -1] == 0).all()
    assert bb.ratio(out.to(BF16), ref, bb.bound16(ref, bound)) <= 1.0 and bb.exact16(out.to(BF16), ref, bound)[1] == 0
    for m in bb.temb_mutants(d):
        mut = bb.temb_eval(t, d, mutant=m)
        assert bb.ratio(mut, ref, bound) > 1.0, "%s passes" % m
        assert bb.ratio(mut.to(BF16), ref, bb.bound16(ref, bound)) > 1.0 or bb.exact16(mut.to(BF16), ref, bound)[1] > 0, "%s passes in bf16" % m


def test_the_high_columns_are_held_hundreds_of_times_tighter_than_2e_4():
    """What the one absolute tolerance of the older test could not see: where arg < 1 the bound is 4 ulp of the value, below
    1e-6."""
    t = bb.temb_case()
    ref, bound = bb.temb_bound(t, 512)
    assert bound[:, 255].max() < 1e-6 and bound[:, 511].max() < 1e-6 and bound[:, 0].max() > 1e-4
    assert set(m for d in bb.TEMB_D for m in bb.temb_mutants(d)) == set(bb.TEMB_MUTANTS)
    assert 0.2 < bb.KAPPA < 0.25


# ----------------------------------------------------------------------------------------------------------------------
# hig_gather_frames
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,T,F", bb.GATHER_CASES)
def test_gather_frames(rows, T, F):
    bank, seq_off, frame_ix, stats = bb.gather_case(rows, T, F)
    assert (seq_off % 2 == 1).all() and int(seq_off[-1]) + bb.GATHER_FRAMES * F <= bank.size
    assert frame_ix.min() >= 0 and frame_ix.max() < bb.GATHER_FRAMES
    if T > 2:
        assert (np.diff(frame_ix[0]) == 0).any() and (np.diff(frame_ix[0]) < 0).any(), "frame_ix neither repeats nor descends"
    o32, o64 = bb.gather_eval(bank, seq_off, frame_ix, stats, False), bb.gather_eval(bank, seq_off, frame_ix, stats, True)
    assert o32.dtype == np.float32 and o64.dtype == np.float32 and o32.shape == (rows, T, F)
    assert (o32 != o64).any(), "the float64 statistics do not tell the two paths apart"
    # the definition, spelled out for one element of the body and one of the init row
    r, t, f = rows - 1, T - 1, F - 1
    x = bank[seq_off[r] + frame_ix[r, t] * F + f]
    if t > 0:
        assert o64[r, t, f] == np.float32((np.float64(x) - stats[f]) / stats[F + f])
    x0 = bank[seq_off[r] + frame_ix[r, 0] * F + 1]
    assert o64[r, 0, 1] == np.float32((np.float64(x0) - stats[2 * F + 1]) / stats[2 * F + 5])
    for f64 in (False, True):
        good = bb.gather_eval(bank, seq_off, frame_ix, stats, f64)
        for m in bb.gather_mutants(rows, T, F, f64):
            assert (bb.gather_eval(bank, seq_off, frame_ix, stats, f64, mutant=m) != good).any(), "%s changes nothing" % m
    seen = set(m for c in bb.GATHER_CASES for m in bb.gather_mutants(*c, True))
    assert seen == set(bb.GATHER_MUTANTS)
