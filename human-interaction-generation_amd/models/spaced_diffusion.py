"""Few-step sampling: `space_timesteps` (which K of the N training steps a sampler visits) and `SpacedDiffusion`, a
`GaussianDiffusion` over those K steps that also carries the DDIM update (codes/models/gaussian_diffusion.py:771-941).

  * The strided schedule keeps the base chain's cumulative products: betas_i = 1 - abar[t_i] / abar[t_(i-1)], so abar_i of
    the short chain IS abar[t_i] of the long one and a model trained on N steps is sampled on K of them.
  * The model never sees the index 0 .. K-1: every call made through this class hands it `timestep_map[t]` (the original
    step, int64), or that step scaled to [0, 1000) as a float when `rescale_timesteps`.
  * `p_sample` / `p_sample_loop` run the ancestral chain on the short schedule (the fused hig_p_sample_step with this
    object's own K-column table); `ddim_sample` / `ddim_sample_loop` run DDIM, fused as hig_ddim_step for fp32 ROCm tensors.
  * Every loop is captured as one hipGraph step replayed K times when the model is our MotionTransformer: the base class's
    _captured_loop, given this object's device_map -- forward at the mapped step, noise (no noise node at all when eta == 0),
    the update in place, hig_advance_timesteps.  `p_sample_loop` itself is inherited.

  * Every sampler takes known-region conditioning (`known` + `known_mask`; the ancestral family also the reference's `pre_seq`
    / `transl_req`): the known part, noised to the level of this object's own step t, is written over the state before each
    model call -- hig_impose_known, one more launch in front of the captured step.

  * `space_timesteps_logsnr` picks the K steps uniformly in log-SNR, lam = log(sqrt(abar) / sqrt(1 - abar)), instead of
    uniformly in t, and `dpm_solver_sample` / `dpm_solver_sample_loop` walk them with DPM-Solver++(2M): the x0 estimate of the
    step before is kept and extrapolated, which makes the update second order in the log-SNR step at no further model call.
    The update is linear, x_prev = c_x x + c_0 x0_i + c_1 x0_(i+1), its coefficients are computed per kept step in fp64 on the
    host (`dpm_solver_coefficients`), and for fp32 ROCm tensors it is one kernel, hig_dpm2m_step, in place on the state and the
    history.  The two belong together: on the uniform-in-t selection the last steps are huge in log-SNR and the extrapolation
    overshoots there.  order=1 is DDIM at eta = 0 in other arithmetic.  The captured loop is the same single step replayed K
    times: no noise node, one history buffer of B rows.

`GaussianDiffusion`'s four DDIM names still raise; `SpacedDiffusion(space_timesteps(N, N), ...)` is
the unstrided DDIM sampler.
"""
import numbers

import numpy as np
import torch as th

from .. import _lib
from .gaussian_diffusion import GaussianDiffusion, ModelMeanType, _Update, _extract_into_tensor, _guided, _known_args, _last_sample

_DDIM_TAB_ORDER = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "alphas_cumprod", "alphas_cumprod_prev")


def space_timesteps(num_timesteps, k):
    """The K original timesteps a K-step sampler keeps out of N: t_i = (2 i (N - 1) + (K - 1)) // (2 (K - 1)), i = 0 .. K-1
    -- i (N - 1) / (K - 1) rounded half up, in integers so that no host's float rounding decides a step.  Strictly
    increasing, from 0 to N - 1; K = N is the identity.  2 <= K <= N, both integers, or ValueError."""
    for name, v in (("num_timesteps", num_timesteps), ("k", k)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError("space_timesteps: %s must be an integer, got %r" % (name, v))
    n, k = int(num_timesteps), int(k)
    if not 2 <= k <= n:
        raise ValueError("space_timesteps: need 2 <= k <= num_timesteps, got k = %d of %d" % (k, n))
    return [(2 * i * (n - 1) + (k - 1)) // (2 * (k - 1)) for i in range(k)]


def space_timesteps_logsnr(betas, k):
    """The K original timesteps a K-step sampler keeps out of N = len(betas), uniform in log-SNR: with abar = cumprod(1 -
    betas) and lam[t] = 0.5 log(abar[t] / (1 - abar[t])) (fp64, strictly decreasing in t), t_i is the index of the lam entry
    nearest linspace(lam[0], lam[N-1], K)[i], a tie going to the lower t; then t_i = max(t_i, t_(i-1) + 1), so that duplicates
    near t = 0 move up.  Where lam falls steeply at the far end as well (the cosine schedule; K near N) that bump runs past
    N - 1; then, and only then, the mirror image follows: t_(K-1) = N - 1 and t_i = min(t_i, t_(i+1) - 1), so that duplicates
    near t = N - 1 move down.  Strictly increasing from 0 to N - 1 for every valid K.  ValueError: K no integer or outside 2 <= K
    <= N, betas not 1-D, a schedule whose log-SNR is not finite and strictly decreasing."""
    b = np.array(betas, dtype=np.float64)
    if b.ndim != 1:
        raise ValueError("space_timesteps_logsnr: betas must be 1-D, got shape %r" % (b.shape,))
    if isinstance(k, bool) or not isinstance(k, numbers.Integral):
        raise ValueError("space_timesteps_logsnr: k must be an integer, got %r" % (k,))
    n, k = int(b.shape[0]), int(k)
    if not 2 <= k <= n:
        raise ValueError("space_timesteps_logsnr: need 2 <= k <= len(betas), got k = %d of %d" % (k, n))
    abar = np.cumprod(1.0 - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = 0.5 * np.log(abar / (1.0 - abar))
    if not (np.isfinite(lam).all() and (np.diff(lam) < 0).all()):
        raise ValueError("space_timesteps_logsnr: the log-SNR of this schedule is not finite and strictly decreasing")
    steps = []
    for target in np.linspace(lam[0], lam[n - 1], k):
        t = int(np.argmin(np.abs(lam - target)))      # (argmin returns the first of equal minima: the lower t)
        steps.append(t if not steps else max(t, steps[-1] + 1))
    if steps[-1] > n - 1:
        steps[-1] = n - 1
        for i in range(k - 2, -1, -1):
            steps[i] = min(steps[i], steps[i + 1] - 1)
    if steps[0] != 0 or steps[-1] != n - 1 or any(b2 <= a for a, b2 in zip(steps, steps[1:])):
        raise ValueError("space_timesteps_logsnr: %d steps uniform in log-SNR do not fit this schedule of %d (got %d .. %d)"
                         % (k, n, steps[0], steps[-1]))
    return steps


class _MappedModel:
    """What the denoiser is called through: index 0 .. K-1 in, original timestep out."""

    def __init__(self, model, owner):
        self.model, self.owner = model, owner

    def __call__(self, x, ts, **kwargs):
        return self.model(x, self.owner.map_timesteps(ts), **kwargs)


class SpacedDiffusion(GaussianDiffusion):
    def __init__(self, use_timesteps, *, betas, model_mean_type, model_var_type, loss_type, rescale_timesteps=False):
        base_betas = np.array(betas, dtype=np.float64)
        if base_betas.ndim != 1:
            raise ValueError("SpacedDiffusion: betas must be 1-D, got shape %r" % (base_betas.shape,))
        n = int(base_betas.shape[0])
        steps = sorted(int(t) for t in use_timesteps)
        if not steps:
            raise ValueError("SpacedDiffusion: use_timesteps is empty")
        if len(set(steps)) != len(steps):
            raise ValueError("SpacedDiffusion: use_timesteps repeats a step")
        if steps[0] < 0 or steps[-1] >= n:
            raise ValueError("SpacedDiffusion: use_timesteps must lie in [0, %d), got %d .. %d" % (n, steps[0], steps[-1]))
        self.use_timesteps = tuple(steps)
        self.timestep_map = list(steps)
        self.original_num_timesteps = n
        abar = np.cumprod(1.0 - base_betas, axis=0)
        kept = abar[np.array(steps)]
        new_betas = 1.0 - kept / np.append(1.0, kept[:-1])
        super().__init__(betas=new_betas, model_mean_type=model_mean_type, model_var_type=model_var_type,
                         loss_type=loss_type, rescale_timesteps=rescale_timesteps)
        self._dev_maps = {}
        self._dev_ddim_tabs = {}
        self._dev_dpm_tabs = {}

    # ---- what the model sees ----------------------------------------------------------------
    def device_map(self, device):
        """timestep_map as an int64 device tensor, built once per device."""
        key = str(device)
        if key not in self._dev_maps:
            self._dev_maps[key] = th.tensor(self.timestep_map, dtype=th.int64, device=device)
        return self._dev_maps[key]

    def ddim_table(self, device):
        """(4, num_timesteps) fp32 table of hig_ddim_step (HIG_DDIM_TAB_ROWS), built once per device."""
        key = str(device)
        if key not in self._dev_ddim_tabs:
            tab = np.stack([getattr(self, n) for n in _DDIM_TAB_ORDER]).astype(np.float32)
            self._dev_ddim_tabs[key] = th.from_numpy(tab).to(device).contiguous()
        return self._dev_ddim_tabs[key]

    def map_timesteps(self, t):
        """Index 0 .. K-1 -> the timestep the model was trained on (scaled to [0, 1000) as a float when rescale_timesteps)."""
        orig = self.device_map(t.device)[t.long()]
        if self.rescale_timesteps:
            return orig.float() * (1000.0 / self.original_num_timesteps)
        return orig

    def _scale_timesteps(self, t):
        return t      # (the mapped model scales, against the ORIGINAL number of steps)

    def _wrap(self, model):
        if isinstance(model, _MappedModel) and model.owner is self:
            return model
        return _MappedModel(model, self)

    def p_mean_variance(self, model, *args, **kwargs):
        return super().p_mean_variance(self._wrap(model), *args, **kwargs)

    def training_losses(self, model, *args, **kwargs):
        return super().training_losses(self._wrap(model), *args, **kwargs)

    def p_sample(self, model, *args, **kwargs):
        """The ancestral step on the short schedule; the fused branch is the base class's, with this object's table."""
        return super().p_sample(self._wrap(model), *args, **kwargs)

    # ---- DDIM -------------------------------------------------------------------------------
    def _ddim_fused_ok(self, denoised_fn, cond_fn):
        return (self.model_mean_type == ModelMeanType.EPSILON and denoised_fn is None and cond_fn is None
                and not self.rescale_timesteps)

    def _ddim_update(self, eta, clip_denoised):
        # eta == 0 reads no z: the eager step draws none and the captured loop has no noise node
        return _Update("hig_ddim_step", self.ddim_table, eta != 0, False, (float(eta), int(bool(clip_denoised))))

    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0,
                    known=None, known_mask=None):
        """gaussian_diffusion.py:771-819.  For fp32 ROCm tensors on the eps-prediction branch the whole update is ONE kernel
        (either value of clip_denoised); everything else is tensor arithmetic.  The fused path draws no noise at eta == 0
        (z is never read there), the tensor-op path draws it always, as the reference does: after an eta == 0 call the
        generator's state therefore depends on which path ran, the sample does not.
        known + known_mask: the known part, noised to level t with a fresh randn_like(known), is written into the caller's x
        first (as p_sample does).  A conditioned step therefore draws noise at eta == 0 too: it is no longer a pure function
        of x."""
        if cond_fn is not None:
            raise NotImplementedError("cond_fn guidance is never used by the reference tools")
        known, known_mask = _known_args(x.shape, known, known_mask, None)
        if known is not None:
            self._impose(x, t, known, known_mask, None)
        if self._ddim_fused_ok(denoised_fn, cond_fn) and self._fused_ok(x):
            eps = self._wrap(model)(x, t, **(model_kwargs or {}))
            noise = th.randn_like(x).contiguous() if eta != 0 else None
            xc = x.contiguous()
            sample, pred = th.empty_like(xc), th.empty_like(xc)
            self._fused_update(self._ddim_update(eta, clip_denoised), xc, eps.float().contiguous(), noise, t.long().contiguous(),
                               xc.shape[0], x_prev=sample, pred=pred)
            return {"sample": sample, "pred_xstart": pred}
        out = self.p_mean_variance(model, x, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                   model_kwargs=model_kwargs)
        # eps is re-derived from the x0 estimate, which the clamp or another mean type may have changed
        eps = self._predict_eps_from_xstart(x, t, out["pred_xstart"])
        alpha_bar = _extract_into_tensor(self.alphas_cumprod, t, x.shape)
        alpha_bar_prev = _extract_into_tensor(self.alphas_cumprod_prev, t, x.shape)
        sigma = eta * th.sqrt((1 - alpha_bar_prev) / (1 - alpha_bar)) * th.sqrt(1 - alpha_bar / alpha_bar_prev)
        noise = th.randn_like(x)
        mean_pred = out["pred_xstart"] * th.sqrt(alpha_bar_prev) + th.sqrt(1 - alpha_bar_prev - sigma ** 2) * eps
        nonzero_mask = (t != 0).float().view(-1, *([1] * (len(x.shape) - 1)))
        return {"sample": mean_pred + nonzero_mask * sigma * noise, "pred_xstart": out["pred_xstart"]}

    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None, eta=0.0):
        """x_{t+1} by the deterministic reverse ODE (gaussian_diffusion.py:821-857); tensor arithmetic."""
        assert eta == 0.0, "Reverse ODE only for deterministic path"
        out = self.p_mean_variance(model, x, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                   model_kwargs=model_kwargs)
        eps = ((_extract_into_tensor(self.sqrt_recip_alphas_cumprod, t, x.shape) * x - out["pred_xstart"])
               / _extract_into_tensor(self.sqrt_recipm1_alphas_cumprod, t, x.shape))
        alpha_bar_next = _extract_into_tensor(self.alphas_cumprod_next, t, x.shape)
        mean_pred = out["pred_xstart"] * th.sqrt(alpha_bar_next) + th.sqrt(1 - alpha_bar_next) * eps
        return {"sample": mean_pred, "pred_xstart": out["pred_xstart"]}

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                         model_kwargs=None, device=None, progress=False, eta=0.0, known=None, known_mask=None):
        """gaussian_diffusion.py:859-891.  With known + known_mask every step first writes the noised known part over the
        state; the noise of that imposition is fresh every step, so a conditioned loop at eta == 0 is NOT a pure function of
        its start (the unconditioned one is)."""
        core, cfg = _guided(model, model_kwargs)
        if self._graph_ok(core, model_kwargs) and self._ddim_fused_ok(denoised_fn, cond_fn):
            known, known_mask = _known_args(shape, known, known_mask, None)
            return self._captured_loop(core, shape, noise, model_kwargs, device, self._ddim_update(eta, clip_denoised),
                                       self.device_map, known, known_mask, cfg=cfg)
        return _last_sample(self.ddim_sample_loop_progressive(
            model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
            model_kwargs=model_kwargs, device=device, progress=progress, eta=eta, known=known, known_mask=known_mask))

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                     model_kwargs=None, device=None, progress=False, eta=0.0, known=None, known_mask=None):
        """gaussian_diffusion.py:893-941: t = K-1 ... 0, no_grad."""
        return self._loop_progressive(
            lambda img, t, last, **cond: self.ddim_sample(model, img, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                                          cond_fn=cond_fn, model_kwargs=model_kwargs, eta=eta, **cond),
            model, shape, noise, device, progress, known, known_mask)

    # ---- DPM-Solver++(2M) -------------------------------------------------------------------
    def dpm_solver_coefficients(self, order=2):
        """(HIG_DPM_TAB_ROWS, K) fp64: rows a, b (the x0 estimate, x0 = a x - b eps) and c_x, c_0, c_1 of the update
        x_prev = c_x x + c_0 x0_i + c_1 x0_(i+1) of kept step i.  With al = sqrt(abar_i), sg = sqrt(1 - abar_i), lam = log(al /
        sg), the same three of the target level (alphas_cumprod_prev: alp, sgp, lamp) and h = lamp - lam:
            x_prev = (sgp / sg) x + alp (1 - e^-h) D,   D = x0_i                                       first order
                                                        D = (1 + 1 / (2 r)) x0_i - (1 / (2 r)) x0_(i+1)   second order
        r = (lam_i - lam_(i+1)) / h.  First order at i = K - 1 (no history yet) and at i = 0, where the target is sigma = 0, h
        is infinite and x_prev = x0_0: c_x = 0, c_0 = 1, c_1 = 0 exactly.  order=1: c_1 = 0 everywhere, DDIM at eta = 0."""
        if order not in (1, 2):
            raise ValueError("dpm_solver: order must be 1 or 2, got %r" % (order,))
        K = self.num_timesteps
        ac, acp = self.alphas_cumprod, self.alphas_cumprod_prev
        al, sg = np.sqrt(ac), np.sqrt(1.0 - ac)
        lam = np.log(al / sg)
        out = np.zeros((_lib.DPM_TAB_ROWS, K), dtype=np.float64)
        out[0], out[1] = self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod
        out[3, 0] = 1.0
        for i in range(1, K):
            alp, sgp = np.sqrt(acp[i]), np.sqrt(1.0 - acp[i])
            h = np.log(alp / sgp) - lam[i]
            base = alp * -np.expm1(-h)
            out[2, i] = sgp / sg[i]
            if order == 2 and i < K - 1:
                half_inv_r = 0.5 * h / (lam[i] - lam[i + 1])
                out[3, i], out[4, i] = base * (1.0 + half_inv_r), -base * half_inv_r
            else:
                out[3, i] = base
        return out

    def dpm_solver_table(self, device, order=2):
        """(5, num_timesteps) fp32 table of hig_dpm2m_step (HIG_DPM_TAB_ROWS): dpm_solver_coefficients rounded once, built once
        per device and per order."""
        key = (str(device), int(order))
        if key not in self._dev_dpm_tabs:
            tab = self.dpm_solver_coefficients(order).astype(np.float32)
            self._dev_dpm_tabs[key] = th.from_numpy(tab).to(device).contiguous()
        return self._dev_dpm_tabs[key]

    def _dpm_update(self, order, clip_denoised):
        return _Update("hig_dpm2m_step", lambda device: self.dpm_solver_table(device, order), False, True,
                       (int(bool(clip_denoised)),))

    def dpm_solver_sample(self, model, x, t, prev_xstart=None, order=2, clip_denoised=True, denoised_fn=None,
                          model_kwargs=None, known=None, known_mask=None, cond_fn=None):
        """One DPM-Solver++(2M) step: {"sample", "pred_xstart"}; pred_xstart (after denoised_fn and the clamp, as
        p_mean_variance processes it) is what the next call takes as `prev_xstart`.  prev_xstart=None forces first order for
        this call; otherwise the coefficients decide per sample (first order at t = K - 1 and at t = 0, where prev_xstart is
        not read and may hold anything).  For fp32 ROCm tensors on the eps-prediction branch without denoised_fn the update is
        ONE kernel (hig_dpm2m_step, on copies: the caller's x and prev_xstart are left alone); everything else is tensor
        arithmetic in the same operation order.  known + known_mask: as ddim_sample, written into the caller's x first."""
        if cond_fn is not None:
            raise NotImplementedError("cond_fn guidance is never used by the reference tools")
        if prev_xstart is None:
            order = 1
        coef = self.dpm_solver_coefficients(order)                         # (validates order)
        if prev_xstart is not None and tuple(prev_xstart.shape) != tuple(x.shape):
            raise ValueError("dpm_solver_sample: prev_xstart must have x's shape %r, got %r"
                             % (tuple(x.shape), tuple(prev_xstart.shape)))
        known, known_mask = _known_args(x.shape, known, known_mask, None)
        if known is not None:
            self._impose(x, t, known, known_mask, None)
        if (self._ddim_fused_ok(denoised_fn, cond_fn) and self._fused_ok(x)
                and (prev_xstart is None or self._fused_ok(prev_xstart))):
            eps = self._wrap(model)(x, t, **(model_kwargs or {}))
            sample = x.contiguous().clone()
            hist = th.empty_like(sample) if prev_xstart is None else prev_xstart.contiguous().clone()
            self._fused_update(self._dpm_update(order, clip_denoised), sample, eps.float().contiguous(), hist,
                               t.long().contiguous(), sample.shape[0])
            return {"sample": sample, "pred_xstart": hist}
        out = self.p_mean_variance(model, x, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                   model_kwargs=model_kwargs)
        x0 = out["pred_xstart"]
        c_x, c_0, c_1 = (_extract_into_tensor(coef[r], t, x.shape) for r in (2, 3, 4))
        sample = c_x * x + c_0 * x0
        if prev_xstart is not None:
            # a select, as in the kernel: the history of a sample whose c_1 is 0 is never used (it may hold NaN)
            sample = th.where(c_1 != 0, sample + c_1 * prev_xstart.to(sample.dtype), sample)
        return {"sample": sample, "pred_xstart": x0}

    def dpm_solver_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                               model_kwargs=None, device=None, progress=False, order=2, known=None, known_mask=None):
        """K model calls from pure noise, t = K-1 ... 0, the x0 estimate carried from step to step.  Deterministic without a
        known region; with known + known_mask every step first writes the freshly noised known part over the state (the history
        holds model predictions and stays valid)."""
        core, cfg = _guided(model, model_kwargs)
        if self._graph_ok(core, model_kwargs) and self._ddim_fused_ok(denoised_fn, cond_fn):
            self.dpm_solver_coefficients(order)
            known, known_mask = _known_args(shape, known, known_mask, None)
            return self._captured_loop(core, shape, noise, model_kwargs, device, self._dpm_update(order, clip_denoised),
                                       self.device_map, known, known_mask, cfg=cfg)
        return _last_sample(self.dpm_solver_sample_loop_progressive(
            model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
            model_kwargs=model_kwargs, device=device, progress=progress, order=order, known=known, known_mask=known_mask))

    def dpm_solver_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                           cond_fn=None, model_kwargs=None, device=None, progress=False, order=2,
                                           known=None, known_mask=None):
        """t = K-1 ... 0, no_grad; yields every step's {"sample", "pred_xstart"}."""
        return self._loop_progressive(
            lambda img, t, last, **cond: self.dpm_solver_sample(
                model, img, t, prev_xstart=None if last is None else last["pred_xstart"], order=order,
                clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn, model_kwargs=model_kwargs, **cond),
            model, shape, noise, device, progress, known, known_mask)
