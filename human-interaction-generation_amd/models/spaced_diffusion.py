"""Few-step sampling: `space_timesteps` (which K of the N training steps a sampler visits) and `SpacedDiffusion`, a
`GaussianDiffusion` over those K steps that also carries the DDIM update (codes/models/gaussian_diffusion.py:771-941).

  * The strided schedule keeps the base chain's cumulative products: betas_i = 1 - abar[t_i] / abar[t_(i-1)], so abar_i of
    the short chain IS abar[t_i] of the long one and a model trained on N steps is sampled on K of them.
  * The model never sees the index 0 .. K-1: every call made through this class hands it `timestep_map[t]` (the original
    step, int64), or that step scaled to [0, 1000) as a float when `rescale_timesteps`.
  * `p_sample` / `p_sample_loop` run the ancestral chain on the short schedule (the fused hig_p_sample_step with this
    object's own K-column table); `ddim_sample` / `ddim_sample_loop` run DDIM, fused as hig_ddim_step for fp32 ROCm tensors.
  * Both loops are captured as one hipGraph step replayed K times when the model is our MotionTransformer: forward at the
    mapped step, noise (no noise node at all when eta == 0), the update in place, hig_advance_timesteps.  The graph lives for
    one call: it reads the text context the warm-up step built for THIS call's xf_out.

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
    times (method "dpmpp2m"): no noise node, one history buffer of B rows.

`GaussianDiffusion`'s four DDIM names still raise; `SpacedDiffusion(space_timesteps(N, N), ...)` is
the unstrided DDIM sampler.
"""
import numbers

import numpy as np
import torch as th

from .. import _lib
from .gaussian_diffusion import (GaussianDiffusion, ModelMeanType, _extract_into_tensor, _guided, _known_args,
                                 _pre_seq_as_known, _stacked_inputs)
from .guidance import split_rows, stack_rows

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
            xc, ec = x.contiguous(), eps.float().contiguous()
            sample, pred = th.empty_like(xc), th.empty_like(xc)
            B = xc.shape[0]
            t64, tab = t.long().contiguous(), self.ddim_table(xc.device)    # (alive until the launch is enqueued)
            _lib.check(_lib.lib().hig_ddim_step(
                _lib.ptr(xc), _lib.ptr(ec), _lib.ptr(noise), _lib.ptr(t64),
                _lib.ptr(tab), self.num_timesteps, B, xc.numel() // B, float(eta),
                int(bool(clip_denoised)), _lib.ptr(sample), _lib.ptr(pred), _lib.stream_ptr()))
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
            return self._spaced_loop_graph(core, shape, noise, model_kwargs, device, "ddim", float(eta), clip_denoised,
                                           known, known_mask, cfg=cfg)
        final = None
        for sample in self.ddim_sample_loop_progressive(
                model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
                model_kwargs=model_kwargs, device=device, progress=progress, eta=eta, known=known, known_mask=known_mask):
            final = sample
        return final["sample"]

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                     model_kwargs=None, device=None, progress=False, eta=0.0, known=None, known_mask=None):
        """gaussian_diffusion.py:893-941: t = K-1 ... 0, no_grad."""
        if device is None:
            device = next(model.parameters()).device
        assert isinstance(shape, (tuple, list))
        known, known_mask = _known_args(shape, known, known_mask, None)    # (the mask is expanded once)
        cond = {} if known is None else dict(known=known.to(device), known_mask=known_mask.to(device))
        img = noise if noise is not None else th.randn(*shape, device=device)
        indices = list(range(self.num_timesteps))[::-1]
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        for i in indices:
            t = th.tensor([i] * shape[0], device=device)
            with th.no_grad():
                out = self.ddim_sample(model, img, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                       cond_fn=cond_fn, model_kwargs=model_kwargs, eta=eta, **cond)
                yield out
                img = out["sample"]

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
            sample, ec = x.contiguous().clone(), eps.float().contiguous()
            hist = th.empty_like(sample) if prev_xstart is None else prev_xstart.contiguous().clone()
            B = sample.shape[0]
            t64, tab = t.long().contiguous(), self.dpm_solver_table(sample.device, order)   # (alive until the launch is enqueued)
            _lib.check(_lib.lib().hig_dpm2m_step(_lib.ptr(sample), _lib.ptr(ec), _lib.ptr(hist), _lib.ptr(t64), _lib.ptr(tab),
                                                 self.num_timesteps, B, sample.numel() // B, int(bool(clip_denoised)),
                                                 _lib.stream_ptr()))
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
            return self._spaced_loop_graph(core, shape, noise, model_kwargs, device, "dpmpp2m", 0.0, clip_denoised,
                                           known, known_mask, cfg=cfg, order=order)
        final = None
        for sample in self.dpm_solver_sample_loop_progressive(
                model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
                model_kwargs=model_kwargs, device=device, progress=progress, order=order, known=known,
                known_mask=known_mask):
            final = sample
        return final["sample"]

    def dpm_solver_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                           cond_fn=None, model_kwargs=None, device=None, progress=False, order=2,
                                           known=None, known_mask=None):
        """t = K-1 ... 0, no_grad; yields every step's {"sample", "pred_xstart"}."""
        if device is None:
            device = next(model.parameters()).device
        assert isinstance(shape, (tuple, list))
        known, known_mask = _known_args(shape, known, known_mask, None)    # (the mask is expanded once)
        cond = {} if known is None else dict(known=known.to(device), known_mask=known_mask.to(device))
        img = noise if noise is not None else th.randn(*shape, device=device)
        indices = list(range(self.num_timesteps))[::-1]
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        prev = None
        for i in indices:
            t = th.tensor([i] * shape[0], device=device)
            with th.no_grad():
                out = self.dpm_solver_sample(model, img, t, prev_xstart=prev, order=order, clip_denoised=clip_denoised,
                                             denoised_fn=denoised_fn, cond_fn=cond_fn, model_kwargs=model_kwargs, **cond)
                yield out
                img, prev = out["sample"], out["pred_xstart"]

    # ---- captured loops -----------------------------------------------------------------------
    def _graph_ok(self, core, model_kwargs):
        return (self.use_hip_graph and hasattr(core, "_launch_forward") and model_kwargs is not None
                and model_kwargs.get("xf_proj") is not None and model_kwargs.get("xf_out") is not None)

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, pre_seq=None, transl_req=None, progress=False, known=None,
                      known_mask=None):
        """The ancestral chain over the K kept steps; captured under the base class's conditions (pre_seq and known +
        known_mask stay on the captured path, transl_req runs eagerly)."""
        core, cfg = _guided(model, model_kwargs)
        if (self._graph_ok(core, model_kwargs)
                and self._is_trainer_branch(clip_denoised, denoised_fn, cond_fn, pre_seq, transl_req)):
            known, known_mask = _known_args(shape, known, known_mask, pre_seq)
            return self._spaced_loop_graph(core, shape, noise, model_kwargs, device, "ddpm", 0.0, False, known, known_mask,
                                           pre_seq, cfg)
        final = None
        for sample in self.p_sample_loop_progressive(
                model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
                model_kwargs=model_kwargs, device=device, pre_seq=pre_seq, transl_req=transl_req, progress=progress,
                known=known, known_mask=known_mask):
            final = sample
        return final["sample"]

    def _spaced_loop_graph(self, core, shape, noise, model_kwargs, device, method, eta, clip_denoised, known=None,
                           known_mask=None, pre_seq=None, cfg=None, order=2):
        """One captured step replayed num_timesteps times: denoiser forward at the ORIGINAL timestep (t_model), fresh noise
        (ancestral, or DDIM with eta > 0: at eta == 0 the graph has no noise node and the update gets z = NULL), the update in
        place, then hig_advance_timesteps (t -= 1, t_model = map[t]).  The warm-up step outside the graph builds the text
        context of this call's xf_out, whose buffer the captured forward reads: the graph is not kept beyond the call.
        With known + known_mask (or pre_seq, turned into that pair) the step becomes
            zz.normal_() -> hig_impose_known(img, known, mask, zk, t_dev, device_table) -> forward -> update with z -> advance
        The imposition reads t_dev, the index into this object's own K-column table, not t_model.  zk (and z, where the update
        needs one) are parts of ONE buffer drawn by a single normal_(): a conditioned step has one launch more than an
        unconditioned one with noise, two more at DDIM eta == 0 -- which now draws noise and is no longer a pure function of
        its start.
        cfg (a ClassifierFreeGuidedModel around `core`): the state, both step vectors and the text inputs are kept in the stacked
        layout of models/guidance.py (2 B rows, the two rows of a sample equal); the forward runs once at 2 B and
        hig_impose_known_cfg / hig_ddim_step_cfg / hig_p_sample_step_cfg take the place of the unguided kernels, the counter
        advances 2 B entries: launch for launch the unguided step, noise for B rows, the B conditional rows returned.
        method "dpmpp2m": the update is hig_dpm2m_step[_cfg] with the table of `order`; no noise node (a known region still
        draws zk); `hist`, the x0 estimate of the step before, is one buffer of B rows (not stacked under guidance) that the
        kernel reads and rewrites in place.  Step K-1 never reads it, so what the warm-up leaves there is harmless; it is
        cleared with the state all the same."""
        if device is None:
            device = next(core.parameters()).device
        K, B = self.num_timesteps, shape[0]
        with th.no_grad():
            img = (noise.to(device).float().clone() if noise is not None
                   else th.randn(*shape, device=device)).contiguous()
            xf_proj = model_kwargs["xf_proj"].detach().float().contiguous()
            xf_out = model_kwargs["xf_out"].detach().float().contiguous()
            length = model_kwargs.get("length")
            if length is None:
                length = th.full((B,), shape[1], dtype=th.int64, device=device)
            else:
                length = th.as_tensor(length).to(device).long().contiguous()
            if cfg is not None:
                group, xf_proj, xf_out, length = _stacked_inputs(cfg, B, xf_proj, xf_out, length)
                state = stack_rows(img, img, group).contiguous()
            else:
                state = img
            rows = state.shape[0]
            tmap = self.device_map(device)
            t_dev = th.full((rows,), K - 1, dtype=th.int64, device=device)
            t_model = th.full((rows,), self.timestep_map[K - 1], dtype=th.int64, device=device)
            if method not in ("ddpm", "ddim", "dpmpp2m"):
                raise ValueError("_spaced_loop_graph: unknown method %r" % (method,))
            ddim, dpm = method == "ddim", method == "dpmpp2m"
            needs_z = method == "ddpm" or (ddim and eta != 0)
            tab = (self.dpm_solver_table(device, order) if dpm else self.ddim_table(device) if ddim
                   else self.device_table(device))
            hist = th.zeros_like(img) if dpm else None
            L = _lib.lib()
            per = img.numel() // B
            if pre_seq is not None:
                known, known_mask = _pre_seq_as_known(pre_seq.float(), img.shape, device)
            cond = known is not None
            if cond:
                known = known.to(device).float().contiguous()
                known_mask = known_mask.to(device).contiguous()
                qtab = self.device_table(device)
                zz = th.zeros(2 if needs_z else 1, *img.shape, device=device)
                zk, z = zz[0], (zz[1] if needs_z else None)
            else:
                z = th.zeros_like(img) if needs_z else None

            def step():
                if cond:
                    if not self._debug_zero_noise:
                        zz.normal_()
                    if cfg is not None:
                        _lib.check(L.hig_impose_known_cfg(_lib.ptr(state), _lib.ptr(known), _lib.ptr(known_mask), _lib.ptr(zk),
                                                          _lib.ptr(t_dev), _lib.ptr(qtab), K, B, group, per, _lib.stream_ptr()))
                    else:
                        _lib.check(L.hig_impose_known(_lib.ptr(img), _lib.ptr(known), _lib.ptr(known_mask), _lib.ptr(zk),
                                                      _lib.ptr(t_dev), _lib.ptr(qtab), K, B, per, _lib.stream_ptr()))
                eps, _ = core._launch_forward(state, t_model, length, xf_proj, xf_out, training=False)
                if needs_z and not cond and not self._debug_zero_noise:
                    z.normal_()
                if dpm and cfg is not None:
                    _lib.check(L.hig_dpm2m_step_cfg(_lib.ptr(state), _lib.ptr(eps), cfg.scale, _lib.ptr(hist), _lib.ptr(t_dev),
                                                    _lib.ptr(tab), K, B, group, per, int(bool(clip_denoised)), _lib.stream_ptr()))
                elif dpm:
                    _lib.check(L.hig_dpm2m_step(_lib.ptr(img), _lib.ptr(eps), _lib.ptr(hist), _lib.ptr(t_dev), _lib.ptr(tab), K, B,
                                                per, int(bool(clip_denoised)), _lib.stream_ptr()))
                elif cfg is not None and ddim:
                    _lib.check(L.hig_ddim_step_cfg(_lib.ptr(state), _lib.ptr(eps), cfg.scale, _lib.ptr(z), _lib.ptr(t_dev),
                                                   _lib.ptr(tab), K, B, group, per, eta, int(bool(clip_denoised)), None,
                                                   _lib.stream_ptr()))
                elif cfg is not None:
                    _lib.check(L.hig_p_sample_step_cfg(_lib.ptr(state), _lib.ptr(eps), cfg.scale, _lib.ptr(z), _lib.ptr(t_dev),
                                                       _lib.ptr(tab), K, B, group, per, None, _lib.stream_ptr()))
                elif ddim:
                    _lib.check(L.hig_ddim_step(_lib.ptr(img), _lib.ptr(eps), _lib.ptr(z), _lib.ptr(t_dev), _lib.ptr(tab), K, B,
                                               per, eta, int(bool(clip_denoised)), _lib.ptr(img), None, _lib.stream_ptr()))
                else:
                    _lib.check(L.hig_p_sample_step(_lib.ptr(img), _lib.ptr(eps), _lib.ptr(z), _lib.ptr(t_dev), _lib.ptr(tab),
                                                   K, B, per, _lib.ptr(img), None, _lib.stream_ptr()))
                _lib.check(L.hig_advance_timesteps(_lib.ptr(t_dev), _lib.ptr(tmap), K, rows, _lib.ptr(t_model),
                                                   _lib.stream_ptr()))

            # warm-up on a side stream (allocations, text context), then undo its effect
            img0 = state.clone()
            s = th.cuda.Stream()
            s.wait_stream(th.cuda.current_stream())
            with th.cuda.stream(s):
                step()
            th.cuda.current_stream().wait_stream(s)
            state.copy_(img0)
            if dpm:
                hist.zero_()
            t_dev.fill_(K - 1)
            t_model.fill_(self.timestep_map[K - 1])
            graph = th.cuda.CUDAGraph()
            with th.cuda.graph(graph, capture_error_mode="thread_local"):
                step()
            # capture does not execute: state is still (img0, K-1)
            for _ in range(K):
                graph.replay()
        return state if cfg is None else split_rows(state, group)[0].contiguous()
