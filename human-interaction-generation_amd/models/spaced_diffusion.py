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
                           known_mask=None, pre_seq=None, cfg=None):
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
        advances 2 B entries: launch for launch the unguided step, noise for B rows, the B conditional rows returned."""
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
            ddim = method == "ddim"
            needs_z = not ddim or eta != 0
            tab = self.ddim_table(device) if ddim else self.device_table(device)
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
                if cfg is not None and ddim:
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
            t_dev.fill_(K - 1)
            t_model.fill_(self.timestep_map[K - 1])
            graph = th.cuda.CUDAGraph()
            with th.cuda.graph(graph, capture_error_mode="thread_local"):
                step()
            # capture does not execute: state is still (img0, K-1)
            for _ in range(K):
                graph.replay()
        return state if cfg is None else split_rows(state, group)[0].contiguous()
