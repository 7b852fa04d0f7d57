"""The per-timestep loss weights without a GPU: tests/loss_weight_bounds.py accepts fp32 in the kernels' order and rejects a
mutant each; min_snr_weights gives the values of the definition; the host sampler reproduces the reference's own
LossSecondMomentResampler (golden g23); the three new entry points refuse bad arguments before any launch; bad options are a
ValueError and the loss-aware sampler refuses more than one rank."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import boundary_bounds as bb
import loss_weight_bounds as lw
from loss_weight_bounds import F32, ratio

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_loss_sampler.npz")


# ----------------------------------------------------------------------------------------------------------------------
# the bounds: sound against fp32 in the kernel's order, and each rejects its mutants
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,F", lw.MASKED_SHAPES)
@pytest.mark.parametrize("with_len", (True, False))
def test_masked_bound_accepts_fp32(B, T, F, with_len):
    pred, target, length, t, wtab = lw.masked_case(B, T, F, with_len)
    b = lw.masked_w_bound(pred, target, length, t, wtab)
    out = lw.masked_w_eval(pred, target, length, t, wtab, dtype=F32, kernel_order=True)
    for k in ("loss", "dpred", "sample_loss"):
        assert ratio(out[k], *b[k]) <= 1.0, k
    pn, tn = lw.masked_poison(pred, target, length)
    again = lw.masked_w_eval(pn, tn, length, t, wtab)
    assert all(torch.equal(again[k], b[k][0]) for k in ("loss", "dpred", "sample_loss")), "NaN off the mask leaks into the reference"


def test_masked_bound_rejects_weight_indexed_by_b():
    B, T, F = 5, 9, 263
    pred, target, length, t, wtab = lw.masked_case(B, T, F)
    b = lw.masked_w_bound(pred, target, length, t, wtab)
    out = lw.masked_w_eval(pred, target, length, t, wtab, mutant="weight_indexed_by_b")
    assert ratio(out["loss"], *b["loss"]) > 1.0 and ratio(out["dpred"], *b["dpred"]) > 1.0
    assert ratio(out["sample_loss"], *b["sample_loss"]) <= 1.0          # (the per-sample losses carry no weight)


def test_unit_table_is_the_unweighted_loss():
    """wtab == 1: the fp64 restatements coincide with the unweighted ones of rowops_bounds / boundary_bounds."""
    import rowops_bounds as rb
    pred, target, length, t, _ = lw.masked_case(5, 9, 263)
    ones = torch.ones(lw.NSTEPS)
    out = lw.masked_w_eval(pred, target, length, t, ones)
    loss, dp = rb.masked_mse_eval(pred, target, length)
    assert torch.allclose(out["loss"], loss, rtol=1e-14, atol=0) and torch.allclose(out["dpred"], dp, rtol=1e-14, atol=0)
    for pit in (0, 1):
        pred, target, length, t, _ = lw.pair_w_case(12, 9, 263, pit, True)
        out, ref = lw.pair_w_eval(pred, target, length, pit, t, ones), bb.pair_eval(pred, target, length, pit)
        for k in ("loss", "rowscale", "dpred"):
            assert torch.equal(out[k], ref[k]), k


@pytest.mark.parametrize("R,T,F,pit,with_len", lw.PAIR_W_SHAPES)
def test_pair_bound_accepts_fp32(R, T, F, pit, with_len):
    pred, target, length, t, wtab = lw.pair_w_case(R, T, F, pit, with_len)
    b = lw.pair_w_bound(pred, target, length, pit, t, wtab)
    out = lw.pair_w_eval(pred, target, length, pit, t, wtab, dtype=F32, kernel_order=True)
    for k in ("loss", "dpred", "sample_loss"):
        assert ratio(out[k], *b[k]) <= 1.0, k
    assert torch.equal(out["rowscale"].view(torch.int32), b["rowscale32"].view(torch.int32)), "rowscale is not fp32(w fp32(1 / denom))"
    if pit:
        assert torch.equal(out["first"], b["first"])
        assert ((b["margin"] > bb.PAIR_MARGIN) | b["tie"]).all(), "a pair is neither decided nor a tie by construction"


@pytest.mark.parametrize("mutant,pit", (("weight_indexed_by_b", 0), ("weight_indexed_by_b", 1),
                                        ("weight_before_selection_on_one_assignment", 1)))      # (the second exists under PIT only)
def test_pair_bound_rejects_mutant(mutant, pit):
    assert mutant in lw.PAIR_W_MUTANTS
    pred, target, length, t, wtab = lw.pair_w_case(12, 9, 263, pit, True)
    b = lw.pair_w_bound(pred, target, length, pit, t, wtab)
    out = lw.pair_w_eval(pred, target, length, pit, t, wtab, mutant=mutant)
    assert ratio(out["loss"], *b["loss"]) > 1.0 and ratio(out["dpred"], *b["dpred"]) > 1.0, mutant
    if mutant == "weight_before_selection_on_one_assignment":
        # pair 0 (weight 1e2, the first assignment 16 x cheaper) and pair 1 (weight 1e-4, the second cheaper) both turn
        assert not out["first"][0] and b["first"][0] and out["first"][1] and not b["first"][1]
        assert ratio(out["sample_loss"], *b["sample_loss"]) > 1.0


@pytest.mark.parametrize("nsteps,H", lw.HISTORY_SHAPES)
def test_refresh_bound_accepts_fp32(nsteps, H):
    seq = lw.history_sequence(nsteps, H)
    base = lw.weight_table(nsteps).numpy()
    m = lw.HistoryMirror(nsteps, H, base_w=base)
    for i, (ts, losses) in enumerate(seq):
        m.update(ts, losses)
        (p, b_p), (w, b_w), exact = lw.refresh_bound(m)
        assert exact == (i < len(seq) - 1), "the sequence must fill the last ring in its last batch"
        p32, w32 = m.emulate32()
        if exact:
            assert (p32 == p).all() and (w32 == lw.f32(base)).all()
        else:
            assert (np.abs(p32 - p) <= b_p).all() and (np.abs(w32 - w) <= b_w).all()
            assert abs(p32.astype(np.float64).sum() - 1.0) <= nsteps * lw.U
    assert m.pushes == sum(len(ts) for ts, _ in seq) - 5 * len(seq), "only the five junk entries of each batch are skipped"


@pytest.mark.parametrize("mutant", lw.HISTORY_MUTANTS)
def test_refresh_bound_rejects_mutant(mutant):
    nsteps, H = 7, 3
    seq = lw.history_sequence(nsteps, H, batch=6)
    good, bad = lw.HistoryMirror(nsteps, H), lw.HistoryMirror(nsteps, H, mutant=mutant)
    seen = False
    for ts, losses in seq:
        good.update(ts, losses)
        bad.update(ts, losses)
        (p, b_p), (w, b_w), _ = lw.refresh_bound(good)
        pm, wm = bad.refresh()
        seen |= bool((np.abs(pm - p) > b_p).any() or (np.abs(wm - w) > b_w).any())
        if mutant == "push_order_reversed":
            seen |= not np.array_equal(good.hist, bad.hist)
    assert seen, "%s passes" % mutant
    if mutant == "push_order_reversed":      # ... and is visible in the history itself: a batch repeats a timestep
        a, b = lw.HistoryMirror(2, 2), lw.HistoryMirror(2, 2, mutant=mutant)
        a.update([1, 1, 1, 1], [1.0, 2.0, 3.0, 4.0])
        b.update([1, 1, 1, 1], [1.0, 2.0, 3.0, 4.0])
        assert a.hist[1].tolist() == [3.0, 4.0] and b.hist[1].tolist() == [2.0, 1.0]


# ----------------------------------------------------------------------------------------------------------------------
# min_snr_weights
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ("linear", "cosine"))
@pytest.mark.parametrize("gamma", (1.0, 5.0, float("inf")))
def test_min_snr_weights(schedule, gamma):
    from hig_amd.models.gaussian_diffusion import get_named_beta_schedule, min_snr_weights
    betas = get_named_beta_schedule(schedule, 1000)
    ac = np.cumprod(1.0 - betas)
    w = min_snr_weights(ac, gamma)
    assert w.dtype == np.float64 and w.shape == (1000,)
    ref = np.array([min(a / (1 - a), gamma) / (a / (1 - a)) for a in ac.tolist()])
    assert np.abs(w - ref).max() <= 1e-15
    assert ((w > 0) & (w <= 1)).all()
    if gamma == float("inf"):
        assert (w == 1.0).all()
    else:
        assert w[0] < 1.0 and w[-1] == 1.0 and (np.diff(w) >= 0).all()      # the low-noise steps are the ones held down
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            min_snr_weights(ac, bad)


# ----------------------------------------------------------------------------------------------------------------------
# golden g23: the reference's own sampler
# ----------------------------------------------------------------------------------------------------------------------
def test_host_sampler_reproduces_the_reference():
    from hig_amd.models.gaussian_diffusion import (LossAwareSampler, LossSecondMomentResampler, create_named_schedule_sampler)
    g = np.load(GOLDEN)
    N, H, u = int(g["nsteps"]), int(g["history_per_term"]), float(g["uniform_prob"])
    smp = LossSecondMomentResampler(types.SimpleNamespace(num_timesteps=N), history_per_term=H, uniform_prob=u)
    assert isinstance(smp, LossAwareSampler)
    mirror = lw.HistoryMirror(N, H, uniform_prob=u, round32=False)
    for i, n in enumerate(g["n"].tolist()):
        ts, losses = g["ts"][i, :n], g["losses"][i, :n]
        smp.update_with_all_losses(ts.tolist(), losses.tolist())
        mirror.update(ts, losses)
        for hist, counts in ((smp._loss_history, smp._loss_counts), (mirror.hist, mirror.counts)):
            assert np.abs(hist - g["history"][i]).max() <= 1e-15 and np.array_equal(counts, g["counts"][i]), "call %d" % i
        assert bool(smp._warmed_up()) == bool(g["warmed_up"][i]) == mirror.warmed_up()
        assert np.abs(smp.weights() - g["weights"][i]).max() <= 1e-15, "call %d" % i
        p, w = mirror.refresh()
        wts = g["weights"][i] / g["weights"][i].sum()          # (ones before warm-up: p = 1 / N)
        assert np.abs(p - wts).max() <= 1e-15 and np.abs(w - 1 / (N * wts)).max() <= 1e-13, "call %d" % i
    assert (g["weights"][2] == 1.0).all() and abs(g["weights"][3].sum() - 1.0) <= 1e-15      # before and after warm-up
    by_name = create_named_schedule_sampler("loss-second-moment", types.SimpleNamespace(num_timesteps=N))
    assert isinstance(by_name, LossSecondMomentResampler) and by_name.history_per_term == 10
    t, weights = smp.sample(4, "cpu")
    assert t.shape == (4,) and weights.shape == (4,)


# ----------------------------------------------------------------------------------------------------------------------
# HIG_EINVAL before any HIP call, options, the world > 1 refusal
# ----------------------------------------------------------------------------------------------------------------------
EINVAL = -1


def test_entry_points_refuse_bad_arguments_on_the_host():
    """Every check runs before anything touches a device: the pointers are host memory and are never dereferenced."""
    from hig_amd import _lib
    L = _lib.lib()
    raw = (C.c_float * 512)()
    base = (C.addressof(raw) + 15) // 16 * 16
    pred, target, length, t, wtab, loss, dpred, sl, scr = [C.c_void_p(base + 64 * i) for i in range(9)]

    def masked(**kw):
        a = dict(pred=pred, target=target, length=length, t=t, wtab=wtab, nsteps=10, B=2, T=2, F=4, loss=loss, dpred=dpred,
                 sl=sl, scr=scr)
        a.update(kw)
        return L.hig_masked_mse_w(a["pred"], a["target"], a["length"], a["t"], a["wtab"], a["nsteps"], a["B"], a["T"], a["F"],
                                  a["loss"], a["dpred"], a["sl"], a["scr"], None)

    def pair(**kw):
        a = dict(pred=pred, target=target, length=length, t=t, wtab=wtab, nsteps=10, R=4, T=2, F=4, pit=1, loss=loss,
                 dpred=dpred, sl=sl, scr=scr)
        a.update(kw)
        return L.hig_pair_mse_w(a["pred"], a["target"], a["length"], a["t"], a["wtab"], a["nsteps"], a["R"], a["T"], a["F"],
                                a["pit"], a["loss"], a["dpred"], a["sl"], a["scr"], None)

    for kw in (dict(pred=None), dict(target=None), dict(t=None), dict(wtab=None), dict(loss=None), dict(scr=None),
               dict(nsteps=0), dict(nsteps=-1), dict(T=0), dict(T=-2), dict(F=0), dict(F=-1)):
        assert masked(**kw) == EINVAL, "hig_masked_mse_w accepts %s" % kw
        assert "hig_masked_mse_w" in _lib.last_error()
        assert pair(**kw) == EINVAL, "hig_pair_mse_w accepts %s" % kw
        assert "hig_pair_mse_w" in _lib.last_error()
    for kw in (dict(B=0), dict(B=-3)):
        assert masked(**kw) == EINVAL, "hig_masked_mse_w accepts %s" % kw
    for kw in (dict(R=0), dict(R=-4), dict(R=6), dict(F=3)):
        assert pair(**kw) == EINVAL, "hig_pair_mse_w accepts %s" % kw
        assert "hig_pair_mse_w" in _lib.last_error()

    hist, counts, base_w, p_out, w_out = pred, target, length, loss, dpred

    def history(**kw):
        a = dict(t=t, sl=sl, n=3, hist=hist, counts=counts, base_w=base_w, nsteps=7, H=3, u=0.001, p=p_out, w=w_out)
        a.update(kw)
        return L.hig_loss_history_update(a["t"], a["sl"], a["n"], a["hist"], a["counts"], a["base_w"], a["nsteps"], a["H"],
                                         a["u"], a["p"], a["w"], None)

    for kw in (dict(t=None), dict(sl=None), dict(n=-1), dict(hist=None), dict(counts=None), dict(base_w=None), dict(p=None),
               dict(w=None), dict(nsteps=0), dict(nsteps=-7), dict(H=0), dict(H=-1), dict(u=-0.1), dict(u=1.5),
               dict(u=float("nan")), dict(n=0, hist=None)):
        assert history(**kw) == EINVAL, "hig_loss_history_update accepts %s" % kw
        assert "hig_loss_history_update" in _lib.last_error()


def test_bad_loss_options_are_value_errors():
    from hig_amd.trainers.ddpm_trainer import loss_options
    opt = types.SimpleNamespace
    assert loss_options(opt()) == (None, 5.0, "uniform")
    assert loss_options(opt(loss_weighting="min_snr")) == ("min_snr", 5.0, "uniform")
    assert loss_options(opt(loss_weighting="min_snr", min_snr_gamma=1, sampler="loss-second-moment")) == ("min_snr", 1.0, "loss-second-moment")
    assert loss_options(opt(min_snr_gamma=float("inf")))[1] == float("inf")
    for w in ("snr", "min-snr", 1, True, ""):
        with pytest.raises(ValueError, match="loss_weighting"):
            loss_options(opt(loss_weighting=w))
    for g in (0, 0.0, -5.0, float("nan"), "5", True, None):
        with pytest.raises(ValueError, match="min_snr_gamma"):
            loss_options(opt(min_snr_gamma=g))
    for s in ("loss_second_moment", "lsm", None, 0):
        with pytest.raises(ValueError, match="sampler"):
            loss_options(opt(sampler=s))


def _trainer(monkeypatch, world, **options):
    from hig_amd.trainers import ddpm_trainer as dt
    monkeypatch.setattr(dt, "_dist_world", lambda: world)
    opt = types.SimpleNamespace(device="cpu", diffusion_steps=100, is_train=False, **options)
    return dt.DDPMTrainer(opt, torch.nn.Linear(2, 2))


def test_trainer_refuses_bad_options_at_construction(monkeypatch):
    with pytest.raises(ValueError, match="loss_weighting"):
        _trainer(monkeypatch, 1, loss_weighting="snr")
    with pytest.raises(ValueError, match="sampler"):
        _trainer(monkeypatch, 1, sampler="importance")
    tr = _trainer(monkeypatch, 1)
    assert tr.sampler_name == "uniform" and tr._loss_state("cpu") == (None, None) and tr._loss_key("cpu") is None


def test_loss_aware_sampler_refuses_more_than_one_rank(monkeypatch):
    from hig_amd.trainers.ddpm_trainer import check_loss_sampler_world
    check_loss_sampler_world("loss-second-moment", 1)
    check_loss_sampler_world("uniform", 8)
    with pytest.raises(NotImplementedError, match="gather"):
        check_loss_sampler_world("loss-second-moment", 2)
    tr = _trainer(monkeypatch, 2, sampler="loss-second-moment")
    with pytest.raises(NotImplementedError, match="gather of \\(t, loss\\)"):
        tr._draw_t(4, "cpu")
    with pytest.raises(NotImplementedError, match="gather"):
        tr._loss_state("cpu")
    # min-SNR is a static table, identical on every rank: nothing to refuse (the table itself is plain host arithmetic)
    tr = _trainer(monkeypatch, 2, loss_weighting="min_snr")
    wtab, smp = tr._loss_state(torch.device("cpu"))
    assert smp is None and wtab.dtype == torch.float32 and wtab.shape == (100,) and tr._loss_key(torch.device("cpu")) is not None
