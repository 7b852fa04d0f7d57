"""Few-step sampling without a GPU: `space_timesteps`, the tables and the timestep mapping of `SpacedDiffusion`, its tensor-op
DDIM / reverse-DDIM / ancestral steps against what the reference computes on the same strided schedule (golden G16,
tools/make_golden_few_step.py), and the teeth of the hig_ddim_step bound (tests/ddim_bounds.py): an fp32 evaluation in the
kernel's order stays inside it, every mutant lands outside."""
import types

import numpy as np
import pytest
import torch

import ddim_bounds as db
import hig_amd
from hig_amd.models import gaussian_diffusion as gdm
from hig_amd.models import spaced_diffusion as sdm

N = 1000
ETAS, CLIPS = (0.0, 0.5, 1.0), (False, True)


def spaced(k, n=N, **kw):
    args = dict(betas=gdm.get_named_beta_schedule("linear", n), model_mean_type=gdm.ModelMeanType.EPSILON,
                model_var_type=gdm.ModelVarType.FIXED_SMALL, loss_type=gdm.LossType.MSE)
    args.update(kw)
    return hig_amd.SpacedDiffusion(hig_amd.space_timesteps(n, k), **args)


def rel_rows(a, b):
    a, b = a.double().flatten(1), torch.as_tensor(b).double().flatten(1)
    return ((a - b).norm(dim=1) / b.norm(dim=1)).max().item()


def fixed_noise(z):
    """Both diffusion modules draw z from `th.randn_like` for as long as the returned undo() has not run."""
    proxy = types.SimpleNamespace(**{k: getattr(torch, k) for k in dir(torch) if not k.startswith("__")})
    proxy.randn_like = lambda x, **_: z.to(x.device)
    old = gdm.th, sdm.th
    gdm.th = sdm.th = proxy

    def undo():
        gdm.th, sdm.th = old
    return undo


# ---- 1. space_timesteps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", ((1000, 2), (1000, 10), (1000, 50), (1000, 999), (1000, 1000), (50, 7)))
def test_space_timesteps_is_the_integer_formula(n, k):
    ts = hig_amd.space_timesteps(n, k)
    assert ts == [(2 * i * (n - 1) + (k - 1)) // (2 * (k - 1)) for i in range(k)]
    assert len(ts) == k and ts[0] == 0 and ts[-1] == n - 1 and all(b > a for a, b in zip(ts, ts[1:]))
    if k == n:
        assert ts == list(range(n))


@pytest.mark.parametrize("n,k", ((1000, 1), (1000, 1001), (1000, 10.0), (1000.0, 10), (1000, "10"), (1000, None), (1000, 0),
                                 (1000, -3), (1000, True)))
def test_space_timesteps_refuses_anything_else(n, k):
    with pytest.raises(ValueError):
        hig_amd.space_timesteps(n, k)


# ---- 2. tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 10, 50, 1000))
def test_spaced_schedule_keeps_the_base_cumulative_products(k):
    """Within 1e-15 relative at the strides the fixture uses and for the identity.  A wider stride cannot keep that, and the
    reason is the number format, not the code: beta_i = 1 - r_i (r_i = abar[t_i] / abar[t_(i-1)]) is a double next to 1, so it
    carries an absolute rounding of 2^-53, and the constructor's 1 - beta_i hands r_i back with the RELATIVE error 2^-53 / r_i
    (r = 4e-5 at K = 2: 2.8e-12).  So every K is held to sum_i 2^-53 / r_i for those, plus 3 roundings per step (the
    quotient r_i, its own half ulp inside beta_i's, the running product)."""
    base = np.cumprod(1.0 - gdm.get_named_beta_schedule("linear", N))
    sd = spaced(k)
    use = hig_amd.space_timesteps(N, k)
    kept = base[np.array(use)]
    err = np.abs(sd.alphas_cumprod / kept - 1)
    r = kept / np.append(1.0, kept[:-1])
    assert (err <= np.cumsum(2.0 ** -53 / r + 3 * 2.0 ** -53)).all()
    if k in (10, 50, 1000):
        assert err.max() <= 1e-15
    assert sd.num_timesteps == k and sd.original_num_timesteps == N
    assert sd.use_timesteps == tuple(use) and list(sd.timestep_map) == use
    assert isinstance(sd, hig_amd.GaussianDiffusion)


def test_spaced_tables_equal_the_reference_tables(gold):
    g = gold("g16_few_step.npz")
    for k in (10, 50):
        sd = spaced(k)
        assert np.array_equal(np.array(sd.use_timesteps), g["k%d.use_timesteps" % k])
        names = [f.split(".", 1)[1] for f in g.files if f.startswith("k%d." % k) and not f.endswith("use_timesteps")]
        assert len(names) == 13
        for name in names:
            assert np.array_equal(getattr(sd, name), g["k%d.%s" % (k, name)]), (k, name)


def test_constructor_refusals_are_the_base_class_s():
    with pytest.raises(NotImplementedError):
        spaced(10, model_var_type=gdm.ModelVarType.LEARNED_RANGE)
    with pytest.raises(NotImplementedError):
        spaced(10, loss_type=gdm.LossType.KL)
    with pytest.raises(ValueError):
        hig_amd.SpacedDiffusion([0, 1000], betas=gdm.get_named_beta_schedule("linear", N),
                                model_mean_type=gdm.ModelMeanType.EPSILON, model_var_type=gdm.ModelVarType.FIXED_SMALL,
                                loss_type=gdm.LossType.MSE)
    for bad in ([], [3, 3, 7]):
        with pytest.raises(ValueError):
            hig_amd.SpacedDiffusion(bad, betas=gdm.get_named_beta_schedule("linear", N),
                                    model_mean_type=gdm.ModelMeanType.EPSILON, model_var_type=gdm.ModelVarType.FIXED_SMALL,
                                    loss_type=gdm.LossType.MSE)
    # the base class is what it was: its DDIM names still raise
    with pytest.raises(NotImplementedError):
        hig_amd.GaussianDiffusion(betas=gdm.get_named_beta_schedule("linear", 50), model_mean_type=gdm.ModelMeanType.EPSILON,
                                  model_var_type=gdm.ModelVarType.FIXED_SMALL, loss_type=gdm.LossType.MSE).ddim_sample_loop()


# ---- 3. the tensor-op path against the reference --------------------------------------------------------------------------
def test_tensor_op_steps_match_reference_golden(gold):
    g = gold("g16_few_step.npz")
    sd = spaced(10)
    x, eps, z, t = (torch.tensor(g[k]) for k in ("x", "eps", "z", "t"))
    assert t.tolist() == [0, 1, 5, 9]
    stub = lambda *_a, **_k: eps  # noqa: E731
    undo = fixed_noise(z)
    try:
        rows = {}
        for clip in CLIPS:
            for eta in ETAS:
                rows["ddim.eta%g.clip%d" % (eta, clip)] = sd.ddim_sample(stub, x, t, clip_denoised=clip, eta=eta)
            rows["ddim_reverse.clip%d" % clip] = sd.ddim_reverse_sample(stub, x, t, clip_denoised=clip, eta=0.0)
            rows["p_sample.clip%d" % clip] = sd.p_sample(stub, x, t, clip_denoised=clip)
    finally:
        undo()
    assert len(rows) == 10
    for tag, r in rows.items():
        for key in ("sample", "pred_xstart"):
            e = rel_rows(r[key], g["%s.%s" % (tag, key)])
            assert e < 1e-6, (tag, key, e)
        assert g[tag + ".floor"].shape == (4,) and (g[tag + ".floor"] < 1e-4).all()
    with pytest.raises(NotImplementedError):
        sd.ddim_sample(stub, x, t, cond_fn=lambda *a, **k: None)
    with pytest.raises(AssertionError):
        sd.ddim_reverse_sample(stub, x, t, eta=0.5)


# ---- 4. what the model sees ------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.seen = []

    def __call__(self, x, ts, **_):
        self.seen.append(ts.clone())
        return torch.zeros_like(x)


@pytest.mark.parametrize("rescale", (False, True))
def test_model_receives_original_timesteps(rescale):
    k = 10
    sd = spaced(k, rescale_timesteps=rescale)
    use = torch.tensor(hig_amd.space_timesteps(N, k))
    x = torch.randn(4, 5, 6, generator=torch.Generator().manual_seed(0))
    t = torch.tensor([0, 1, 5, 9])
    want = use[t].float() * (1000.0 / N) if rescale else use[t]
    calls = (lambda m: sd.p_sample(m, x, t), lambda m: sd.p_sample(m, x, t, clip_denoised=False),
             lambda m: sd.ddim_sample(m, x, t), lambda m: sd.ddim_sample(m, x, t, eta=1.0, clip_denoised=False),
             lambda m: sd.ddim_reverse_sample(m, x, t), lambda m: sd.p_mean_variance(m, x, t),
             lambda m: sd.training_losses(m, x, t))
    for call in calls:
        rec = Recorder()
        call(rec)
        assert len(rec.seen) == 1
        assert rec.seen[0].dtype == (torch.float32 if rescale else torch.int64)
        assert torch.equal(rec.seen[0], want)


def test_rescaled_timesteps_scale_by_the_original_length():
    sd = spaced(7, n=50, rescale_timesteps=True)
    rec = Recorder()
    sd.ddim_sample(rec, torch.zeros(2, 3), torch.tensor([6, 1]))
    use = hig_amd.space_timesteps(50, 7)
    assert torch.equal(rec.seen[0], torch.tensor([use[6], use[1]]).float() * (1000.0 / 50))


@pytest.mark.parametrize("loop", ("ddim_sample_loop", "p_sample_loop"))
def test_loops_call_the_model_k_times_from_the_last_kept_step_down(loop):
    k = 10
    sd = spaced(k)
    rec = Recorder()
    out = getattr(sd, loop)(rec, (2, 3, 4), noise=torch.ones(2, 3, 4), device="cpu", clip_denoised=False)
    assert out.shape == (2, 3, 4) and torch.isfinite(out).all()
    use = hig_amd.space_timesteps(N, k)
    assert [s.tolist() for s in rec.seen] == [[use[i]] * 2 for i in range(k - 1, -1, -1)]
    steps = list(sd.ddim_sample_loop_progressive(Recorder(), (2, 3, 4), noise=torch.ones(2, 3, 4), device="cpu"))
    assert len(steps) == k and set(steps[0]) == {"sample", "pred_xstart"}


# ---- 5. the bound of hig_ddim_step has teeth -------------------------------------------------------------------------------
# where each mutant is visible: the mask only where sigma[t = 0] > 0 (the shifted table) and eta > 0; eta only below 1; the
# clamp mutants only with the clamp on
VISIBLE = {"noise_at_t0": dict(shifted=True, etas=(0.5, 1.0), clips=(0, 1)),
           "sigma_ignores_eta": dict(shifted=False, etas=(0.0, 0.5), clips=(0, 1)),
           "alpha_bar_prev_is_alpha_bar": dict(shifted=False, etas=ETAS, clips=(0, 1)),
           "clamp_dropped": dict(shifted=False, etas=ETAS, clips=(1,)),
           "eps_not_rederived_after_clamp": dict(shifted=False, etas=ETAS, clips=(1,))}


@pytest.mark.parametrize("shifted", (False, True))
@pytest.mark.parametrize("per", db.PER_SAMPLE)
def test_fp32_evaluation_is_inside_the_ddim_bound(per, shifted):
    x, eps, z, t, tab = db.ddim_case(4, per, seed=per, shifted=shifted)
    for eta in db.ETAS:
        for clip in db.CLIPS:
            zz = None if eta == 0 else z
            (xp, b), (x0, b0) = db.ddim_bound(x, eps, zz, t, tab, eta, clip)
            assert torch.isfinite(xp).all() and torch.isfinite(b).all() and (b >= 0).all()
            o, o0 = db.ddim_eval(x, eps, zz, t, tab, eta, clip, dtype=db.F32)
            assert db.ratio(o, xp, b) <= 1.0 and db.ratio(o0, x0, b0) <= 1.0, (eta, clip)


@pytest.mark.parametrize("mutant", db.MUTANTS)
def test_ddim_bound_rejects_mutant(mutant):
    assert set(VISIBLE) == set(db.MUTANTS)
    v = VISIBLE[mutant]
    for per in db.PER_SAMPLE:
        x, eps, z, t, tab = db.ddim_case(4, per, seed=per, shifted=v["shifted"])
        for eta in v["etas"]:
            for clip in v["clips"]:
                zz = None if eta == 0 and mutant != "sigma_ignores_eta" else z
                (xp, b), _ = db.ddim_bound(x, eps, zz, t, tab, eta, clip)
                out = db.ddim_eval(x, eps, zz, t, tab, eta, clip, mutant=mutant)[0]
                assert db.ratio(out, xp, b) > 1.0, (mutant, per, eta, clip)


def test_ddim_reference_is_the_class_s_tensor_op_path():
    """ddim_bounds.ddim_eval in fp32 and SpacedDiffusion.ddim_sample on host tensors are the same arithmetic."""
    sd = spaced(db.K)
    tab = db.ddim_table()
    assert torch.equal(tab, torch.from_numpy(np.stack([getattr(sd, n) for n in sdm._DDIM_TAB_ORDER]).astype(np.float32)))
    x, eps, z, t, _ = db.ddim_case(4, 5, seed=5)
    undo = fixed_noise(z)
    try:
        for eta in ETAS:
            for clip in CLIPS:
                r = sd.ddim_sample(lambda *_a, **_k: eps, x, t, clip_denoised=clip, eta=eta)
                o, o0 = db.ddim_eval(x, eps, z, t, tab, eta, clip, dtype=db.F32)
                assert torch.equal(r["sample"], o) and torch.equal(r["pred_xstart"], o0)
    finally:
        undo()


# ---- trainers: argument checking needs no device ---------------------------------------------------------------------------
def test_set_sampler_validates_and_builds_the_spaced_diffusion():
    tr = hig_amd.DDPMTrainer.__new__(hig_amd.DDPMTrainer)
    tr.diffusion_steps = N
    tr.diffusion = hig_amd.GaussianDiffusion(betas=gdm.get_named_beta_schedule("linear", N),
                                             model_mean_type=gdm.ModelMeanType.EPSILON,
                                             model_var_type=gdm.ModelVarType.FIXED_SMALL, loss_type=gdm.LossType.MSE)
    tr._few_step = None
    for bad in (dict(steps=10, method="plms"), dict(steps=1), dict(steps=N + 1), dict(steps=10.5), dict(steps=10, eta=-1.0),
                dict(steps=10, eta=float("nan")), dict(steps=10, eta=float("inf"))):
        with pytest.raises(ValueError):
            tr.set_sampler(**bad)
    assert tr._few_step is None
    tr.set_sampler(steps=10, method="ddim", eta=0.5)
    sd, method, eta = tr._few_step
    assert isinstance(sd, hig_amd.SpacedDiffusion) and sd.num_timesteps == 10 and (method, eta) == ("ddim", 0.5)
    assert sd.use_timesteps == tuple(hig_amd.space_timesteps(N, 10))
    tr.set_sampler(None)
    assert tr._few_step is None


# ---- the launch helpers: argument order against the library's declared signatures ---------------------------------------------
class _Recording:
    """Stands in for the library handle: every entry returns 0 and leaves (name, args) behind."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: (self.calls.append((name, args)), 0)[1]


def test_launch_helpers_put_every_argument_where_the_entry_declares_it():
    from hig_amd import _lib
    real = _lib.lib()
    sd = spaced(10)
    X, EPS, AUX, T, TAB, XP, PRED, STREAM = 101, 102, 103, 104, 105, 106, 107, 999        # made-up pointers: nothing reads them
    KNOWN, MASK = 108, 109
    K, B, GROUP, PER, SCALE = 10, 4, 2, 7, 2.5
    updates = (("hig_p_sample_step", sd._p_update(), (), True), ("hig_ddim_step", sd._ddim_update(0.5, True), (0.5, 1), True),
               ("hig_dpm2m_step", sd._dpm_update(2, True), (1,), False))
    for name, upd, tail, has_outputs in updates:
        assert upd.entry == name and tuple(upd.tail) == tail and upd.history == (not has_outputs)
        rec = _Recording()
        gdm._launch_update(rec, upd, X, EPS, AUX, T, TAB, K, B, PER, STREAM, x_prev=XP, pred=PRED)
        gdm._launch_update(rec, upd, X, EPS, AUX, T, TAB, K, B, PER, STREAM, scale=SCALE, group=GROUP, x_prev=XP, pred=PRED)
        (plain_name, plain), (guided_name, guided) = rec.calls
        assert (plain_name, guided_name) == (name, name + "_cfg")
        assert len(plain) == len(getattr(real, plain_name).argtypes) and len(guided) == len(getattr(real, guided_name).argtypes)
        assert plain == (X, EPS, AUX, T, TAB, K, B, PER) + tail + ((XP, PRED) if has_outputs else ()) + (STREAM,)
        assert guided == (X, EPS, SCALE, AUX, T, TAB, K, B, GROUP, PER) + tail + ((PRED,) if has_outputs else ()) + (STREAM,)
        assert guided[2] == SCALE and guided[8:10] == (GROUP, PER) and plain[-1] == guided[-1] == STREAM
    rec = _Recording()
    gdm._launch_impose_known(rec, X, KNOWN, MASK, AUX, T, TAB, K, B, PER, STREAM)
    gdm._launch_impose_known(rec, X, KNOWN, MASK, AUX, T, TAB, K, B, PER, STREAM, group=GROUP)
    (plain_name, plain), (guided_name, guided) = rec.calls
    assert (plain_name, guided_name) == ("hig_impose_known", "hig_impose_known_cfg")
    assert len(plain) == len(real.hig_impose_known.argtypes) and len(guided) == len(real.hig_impose_known_cfg.argtypes)
    assert plain == (X, KNOWN, MASK, AUX, T, TAB, K, B, PER, STREAM)
    assert guided == (X, KNOWN, MASK, AUX, T, TAB, K, B, GROUP, PER, STREAM)
