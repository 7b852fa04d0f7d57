"""MI355X-native `GaussianDiffusion`: the public surface of the reference class
(codes/models/gaussian_diffusion.py:312-1055, itself OpenAI guided-diffusion) for the branch the
trainers select -- EPSILON / FIXED_SMALL / MSE / linear betas / uniform sampler
(codes/trainers/ddpm_trainer.py:37-46) -- with

  * float64 numpy schedule tables exactly as the reference builds them (:343-380), mirrored once
    per device as an fp32 table (the `.float()` of `_extract_into_tensor`, :1137-1150) instead
    of 8 host->device copies per sampling step;
  * q_sample / the p_sample update as fused HIP kernels (hig_q_sample, hig_p_sample_step);
  * `p_sample_loop` captured as a hipGraph (one denoiser step + update + device-side step
    counter, replayed num_timesteps times) when the model is our MotionTransformer.

The other fixed-variance parametrisations of the reference class (START_X / PREVIOUS_X mean types, FIXED_LARGE
variance, the cosine schedule, q_mean_variance, the eps <-> x0 <-> x_{t-1} conversions) run as plain tensor
arithmetic on whatever device the tensors live on; only the trainers' combination takes the HIP kernels.  Not built
(no reference tool reaches them): learned variances and the KL / VLB losses that train them, DDIM, cond_fn guidance --
the enums keep their member names and those paths raise NotImplementedError instead of silently running something else.

Known-region conditioning (replacement-style in-painting, gaussian_diffusion.py:636-647): before every denoising step the known
part of the motion is noised to the current level and written over the state.  The primitive is a `known` tensor of the
sample's shape plus an element mask (`known_mask`), one hig_impose_known launch on fp32 ROCm tensors; the reference's
`pre_seq` (the first Fp features of every frame) is a special case of it, its `transl_req` stays tensor arithmetic.

Classifier-free guidance (not in the reference): a model wrapped in models/guidance.py's ClassifierFreeGuidedModel runs through
every sampler as any callable does; the captured loop keeps it (it is not stripped like a DDP wrapper) and runs the step on the
stacked batch with hig_impose_known_cfg / hig_p_sample_step_cfg.  cond_fn (classifier guidance) still raises.
"""
import collections
import enum
import math
from abc import ABC, abstractmethod

import numpy as np
import torch as th

from .. import _lib
from .guidance import ClassifierFreeGuidedModel, split_rows, stack_rows


def create_named_schedule_sampler(name, diffusion):
    """gaussian_diffusion.py:16-27."""
    if name == "uniform":
        return UniformSampler(diffusion)
    if name == "loss-second-moment":
        return LossSecondMomentResampler(diffusion)
    raise NotImplementedError(f"unknown schedule sampler: {name}")


class ScheduleSampler(ABC):
    """gaussian_diffusion.py:30-62: host-side importance sampler over timesteps."""

    @abstractmethod
    def weights(self):
        """numpy array of positive weights, one per diffusion step."""

    def sample(self, batch_size, device):
        w = self.weights()
        p = w / np.sum(w)
        indices_np = np.random.choice(len(p), size=(batch_size,), p=p)
        indices = th.from_numpy(indices_np).long().to(device)
        weights_np = 1 / (len(p) * p[indices_np])
        weights = th.from_numpy(weights_np).float().to(device)
        return indices, weights


class UniformSampler(ScheduleSampler):
    def __init__(self, diffusion):
        self.diffusion = diffusion
        self._weights = np.ones([diffusion.num_timesteps])

    def weights(self):
        return self._weights


class LossAwareSampler(ScheduleSampler):
    """gaussian_diffusion.py:74-120 without update_with_local_losses: the cross-rank gather of (t, loss) is not built."""

    @abstractmethod
    def update_with_all_losses(self, ts, losses):
        """ts: int timesteps, losses: one float per timestep; deterministic, no synchronisation."""


class LossSecondMomentResampler(LossAwareSampler):
    """gaussian_diffusion.py:123-153 on the host, in float64 (the reference's `np.int` is `int` here): the host mirror of
    hig_loss_history_update, which the trainers use through DeviceLossSecondMomentResampler."""

    def __init__(self, diffusion, history_per_term=10, uniform_prob=0.001):
        self.diffusion = diffusion
        self.history_per_term = history_per_term
        self.uniform_prob = uniform_prob
        self._loss_history = np.zeros([diffusion.num_timesteps, history_per_term], dtype=np.float64)
        self._loss_counts = np.zeros([diffusion.num_timesteps], dtype=int)

    def weights(self):
        if not self._warmed_up():
            return np.ones([self.diffusion.num_timesteps], dtype=np.float64)
        weights = np.sqrt(np.mean(self._loss_history ** 2, axis=-1))
        weights /= np.sum(weights)
        weights *= 1 - self.uniform_prob
        weights += self.uniform_prob / len(weights)
        return weights

    def update_with_all_losses(self, ts, losses):
        for t, loss in zip(ts, losses):
            if self._loss_counts[t] == self.history_per_term:
                self._loss_history[t, :-1] = self._loss_history[t, 1:]      # shift out the oldest loss term
                self._loss_history[t, -1] = loss
            else:
                self._loss_history[t, self._loss_counts[t]] = loss
                self._loss_counts[t] += 1

    def _warmed_up(self):
        return (self._loss_counts == self.history_per_term).all()


def min_snr_weights(alphas_cumprod, gamma):
    """min-SNR-gamma weights of an eps-prediction loss, w_t = min(SNR_t, gamma) / SNR_t with SNR_t = ac_t / (1 - ac_t), in
    float64; gamma = inf gives all ones.  ValueError unless gamma > 0 (NaN fails)."""
    gamma = float(gamma)
    if not gamma > 0.0:
        raise ValueError("min_snr_weights: gamma must be a number > 0, got %r" % (gamma,))
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    snr = ac / (1.0 - ac)
    return np.minimum(snr, gamma) / snr


class DeviceLossSecondMomentResampler:
    """The loss-second-moment sampler with its state on the device (include/hig.h, hig_loss_history_update): `hist`
    (nsteps, H) and `counts` (int32), the sampling probabilities `p` and the loss-weight table `w` = base_w / (N p), all fp32
    (the reference's history is float64).  base_w: the static per-timestep weights the importance weights are folded into
    (None: all ones).  `sample` draws on the device and reads nothing back; `update` is one kernel launch, capturable.
    Deviations from the reference: fp32 history, and a non-finite loss is skipped instead of recorded."""

    def __init__(self, num_timesteps, device, base_w=None, history_per_term=10, uniform_prob=0.001):
        n, H = int(num_timesteps), int(history_per_term)
        if n <= 0 or H <= 0 or not 0.0 <= float(uniform_prob) <= 1.0:
            raise ValueError("DeviceLossSecondMomentResampler: num_timesteps > 0, history_per_term > 0 and uniform_prob in [0, 1] "
                             "required, got %r, %r, %r" % (num_timesteps, history_per_term, uniform_prob))
        self.num_timesteps, self.history_per_term, self.uniform_prob = n, H, float(uniform_prob)
        base = np.ones(n) if base_w is None else np.asarray(base_w, dtype=np.float64)
        if base.shape != (n,) or not (np.isfinite(base).all() and (base > 0).all()):
            raise ValueError("DeviceLossSecondMomentResampler: base_w must be %d finite positive weights" % n)
        self.base_w = th.from_numpy(base.astype(np.float32)).to(device)
        self.hist = th.zeros(n, H, device=device, dtype=th.float32)
        self.counts = th.zeros(n, device=device, dtype=th.int32)
        self.p = th.empty(n, device=device, dtype=th.float32)
        self.w = th.empty(n, device=device, dtype=th.float32)
        self.refresh()

    def _launch(self, t, sample_loss, n):
        _lib.api.hig_loss_history_update(t, sample_loss, n, self.hist, self.counts, self.base_w, self.num_timesteps,
                                         self.history_per_term, self.uniform_prob, self.p, self.w)

    def refresh(self):
        """p and w from the history as it stands (what a launch with an empty batch does)."""
        self._launch(None, None, 0)

    def update(self, t, sample_loss):
        """Pushes base_w[t_i] * sample_loss[i] for the first len(sample_loss) entries of t (int64) in order, then refreshes p
        and w."""
        n = sample_loss.numel()
        if t.dtype != th.int64 or sample_loss.dtype != th.float32 or t.numel() < n or not (t.is_contiguous() and sample_loss.is_contiguous()):
            raise ValueError("DeviceLossSecondMomentResampler.update: t int64 and sample_loss fp32, contiguous, len(t) >= len(sample_loss)")
        self._launch(t, sample_loss, n)

    def sample(self, batch_size, device=None):
        """(t, weights): t ~ p drawn on the device by torch.multinomial, weights = w[t] (with base_w folded in)."""
        t = th.multinomial(self.p, int(batch_size), replacement=True)
        return t, self.w[t]

    def state_dict(self):
        return {"history": self.hist.cpu(), "counts": self.counts.cpu(), "history_per_term": self.history_per_term,
                "uniform_prob": self.uniform_prob}

    def load_state_dict(self, sd):
        if tuple(sd["history"].shape) != tuple(self.hist.shape):
            raise ValueError("schedule sampler state: history is %s, this sampler's is %s"
                             % (tuple(sd["history"].shape), tuple(self.hist.shape)))
        self.hist.copy_(sd["history"].to(self.hist.device, th.float32))
        self.counts.copy_(sd["counts"].to(self.counts.device, th.int32))
        self.refresh()

    def tensors(self):
        """The four state tensors (what a captured step's warm-up saves and restores)."""
        return (self.hist, self.counts, self.p, self.w)


def get_named_beta_schedule(schedule_name, num_diffusion_timesteps):
    """gaussian_diffusion.py:229-254.  "linear" (what the reference trainers ask for): betas from 1e-4 to 2e-2 at 1000
    steps, end points scaled by 1000 / N otherwise; "cosine": the alpha-bar curve cos^2((t + 0.008) / 1.008 * pi / 2)
    discretised by betas_for_alpha_bar.  float64."""
    n = num_diffusion_timesteps
    if schedule_name == "linear":
        scale = 1000 / n
        return np.linspace(scale * 0.0001, scale * 0.02, n, dtype=np.float64)
    if schedule_name == "cosine":
        return betas_for_alpha_bar(n, lambda u: math.cos((u + 0.008) / 1.008 * math.pi / 2) ** 2)
    raise NotImplementedError(f"unknown beta schedule: {schedule_name}")


def betas_for_alpha_bar(num_diffusion_timesteps, alpha_bar, max_beta=0.999):
    """gaussian_diffusion.py:256-274: beta_i = 1 - alpha_bar((i + 1) / N) / alpha_bar(i / N), capped at max_beta
    (alpha_bar: cumulative product of (1 - beta) as a function of t in [0, 1])."""
    n = num_diffusion_timesteps
    return np.array([min(1 - alpha_bar((i + 1) / n) / alpha_bar(i / n), max_beta) for i in range(n)])


class ModelMeanType(enum.Enum):
    PREVIOUS_X = enum.auto()
    START_X = enum.auto()
    EPSILON = enum.auto()


class ModelVarType(enum.Enum):
    LEARNED = enum.auto()
    FIXED_SMALL = enum.auto()
    FIXED_LARGE = enum.auto()
    LEARNED_RANGE = enum.auto()


class LossType(enum.Enum):
    MSE = enum.auto()
    RESCALED_MSE = enum.auto()
    KL = enum.auto()
    RESCALED_KL = enum.auto()

    def is_vb(self):
        return self == LossType.KL or self == LossType.RESCALED_KL


def mean_flat(tensor):
    return tensor.mean(dim=list(range(1, len(tensor.shape))))


_TAB_ORDER = ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
              "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
              "posterior_log_variance_clipped")


def _unwrap(model):
    return getattr(model, "module", model)


def _guided(model, model_kwargs):
    """(core, cfg) of a sampling call's model.  A ClassifierFreeGuidedModel around a model of ours with precomputed text on
    both branches is kept, not stripped: cfg = (scale, group or None, unconditional xf_proj, xf_out) and core = the model under
    it, whose captured loop then runs on the stacked batch.  Anything else: cfg None and core = the unwrapped model (a guided
    model that cannot be captured has no _launch_forward of its own, so it runs eagerly through its __call__)."""
    if isinstance(model, ClassifierFreeGuidedModel):
        u = model.uncond_kwargs
        if (hasattr(model.core(), "_launch_forward") and u.get("xf_proj") is not None and u.get("xf_out") is not None
                and set(u) <= {"xf_proj", "xf_out"} and model_kwargs is not None
                and all(model_kwargs.get(k) is None for k in ("text",))):
            return model.core(), model
        return model, None
    return _unwrap(model), None


def _stacked_inputs(cfg, B, xf_proj, xf_out, length):
    """(group, xf_proj, xf_out, length) of a guided captured loop, the three tensors in the stacked layout (2 B rows)."""
    group = cfg.group_for(B)
    kw = cfg.stacked_kwargs(dict(xf_proj=xf_proj, xf_out=xf_out, length=length), group)
    return group, kw["xf_proj"].float().contiguous(), kw["xf_out"].float().contiguous(), kw["length"].contiguous()


def _known_args(shape, known, known_mask, pre_seq, transl_req=None):
    """Checks the conditioning arguments of one sampling call against the sample's shape (B, T, F).  Returns (known,
    known_mask) with the mask expanded to the shape as a contiguous uint8 tensor on known's device, or (None, None) when
    neither was given.  ValueError: one of the pair without the other, known together with pre_seq, shapes that do not fit, a
    mask that is neither bool nor uint8, transl_req at B > 2 (the reference's coefficient expand fails there)."""
    shape = tuple(shape)
    if (known is None) != (known_mask is None):
        raise ValueError("known and known_mask go together: got %s without %s"
                         % (("known", "known_mask") if known_mask is None else ("known_mask", "known")))
    if known is not None and pre_seq is not None:
        raise ValueError("known / known_mask and pre_seq are two forms of the same conditioning: give one of them")
    if pre_seq is not None:
        ps = tuple(pre_seq.shape)
        if len(shape) != 3 or len(ps) != 3 or ps[:2] != shape[:2] or not 1 <= ps[2] <= shape[2]:
            raise ValueError("pre_seq must be (B, T, Fp) with Fp <= F for a sample of shape %r, got %r" % (shape, ps))
    if transl_req is not None and shape[0] > 2:
        raise ValueError("transl_req works for a batch of 1 or 2 only (the reference expands a (B,) coefficient to the 2 "
                         "frames it sets), got B = %d" % shape[0])
    if known is None:
        return None, None
    if tuple(known.shape) != shape:
        raise ValueError("known must have the sample's shape %r, got %r" % (shape, tuple(known.shape)))
    known_mask = th.as_tensor(known_mask)
    if known_mask.dtype not in (th.bool, th.uint8):
        raise ValueError("known_mask must be bool or uint8, got %s" % known_mask.dtype)
    try:
        full = th.broadcast_to(known_mask, shape)
    except RuntimeError:
        raise ValueError("known_mask of shape %r does not broadcast to the sample's shape %r"
                         % (tuple(known_mask.shape), shape)) from None
    return known, full.to(device=known.device, dtype=th.uint8).contiguous()


def _pre_seq_as_known(pre_seq, shape, device):
    """The reference's pre_seq as the primitive: known[:, :, :Fp] = pre_seq, the mask on features < Fp."""
    Fp = pre_seq.shape[2]
    known = th.zeros(*shape, device=device, dtype=th.float32)
    known[:, :, :Fp] = pre_seq.to(device)
    mask = th.zeros(*shape, device=device, dtype=th.uint8)
    mask[:, :, :Fp] = 1
    return known, mask


# A fused update as the eager steps and the captured loop launch it: the unguided entry's name (the guided one is that name plus
# "_cfg"); table(device), its fp32 coefficient table; whether it reads noise z; whether its auxiliary buffer is instead the
# history of x0 estimates, read and rewritten in place (such an entry has no x_prev / pred_xstart arguments); and the scalars
# that follow per_sample in its argument list.
_Update = collections.namedtuple("_Update", "entry table needs_z history tail")


def _launch_update(L, upd, x, eps, aux, t, tab, K, B, per, stream, scale=None, group=None, x_prev=None, pred=None):
    """ONE launch of the fused update `upd` through the gateway L (_lib.api), which holds every argument to its declared type.
        unguided (group None):  (x, eps, aux, t, tab, K, B, per, *tail, [x_prev, pred,] stream)
        guided:                 (xx, eps2, scale, aux, t2, tab, K, B, group, per, *tail, [pred,] stream), in place on xx
    aux is z (None where the update reads none) or the history; the bracketed outputs exist where upd.history is false."""
    guided = group is not None
    args = (x, eps) + ((scale,) if guided else ()) + (aux, t, tab, K, B) + ((group,) if guided else ()) + (per,) + tuple(upd.tail)
    if not upd.history:
        args += (pred,) if guided else (x_prev, pred)
    getattr(L, upd.entry + ("_cfg" if guided else ""))(*args, stream)


def _launch_impose_known(L, x, known, mask, z, t, tab, K, B, per, stream, group=None):
    """ONE hig_impose_known launch (group None) or hig_impose_known_cfg launch (`group` goes in before per) through L."""
    args = (x, known, mask, z, t, tab, K, B) + (() if group is None else (group,)) + (per, stream)
    getattr(L, "hig_impose_known" + ("" if group is None else "_cfg"))(*args)


def _last_sample(steps):
    """The sample of the last step a *_loop_progressive generator yields."""
    final = None
    for final in steps:
        pass
    return final["sample"]


class GaussianDiffusion:
    def __init__(self, *, betas, model_mean_type, model_var_type, loss_type, rescale_timesteps=False):
        if model_var_type in (ModelVarType.LEARNED, ModelVarType.LEARNED_RANGE) or loss_type.is_vb():
            # learned variances need a model with 2 C output channels and the VLB terms that train them: no reference
            # tool builds one (ddpm_trainer.py:40-45 is EPSILON / FIXED_SMALL / MSE)
            raise NotImplementedError("GaussianDiffusion: learned variances and the KL / VLB losses are not built, got "
                                      "%s / %s / %s" % (model_mean_type, model_var_type, loss_type))
        self.model_mean_type = model_mean_type
        self.model_var_type = model_var_type
        self.loss_type = loss_type
        self.rescale_timesteps = rescale_timesteps

        betas = np.array(betas, dtype=np.float64)
        self.betas = betas
        assert len(betas.shape) == 1, "betas must be 1-D"
        assert (betas > 0).all() and (betas <= 1).all()
        self.num_timesteps = int(betas.shape[0])

        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        assert self.alphas_cumprod_prev.shape == (self.num_timesteps,)
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(
            np.append(self.posterior_variance[1], self.posterior_variance[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)

        self.use_hip_graph = True      # p_sample_loop: capture the step and replay it
        self._dev_tabs = {}
        self._debug_zero_noise = False  # tests: deterministic graph-vs-eager comparison

    # ---- device-resident tables -------------------------------------------------------------
    def device_table(self, device):
        """(7, num_timesteps) fp32 table in hig.h order, built once per device."""
        key = str(device)
        if key not in self._dev_tabs:
            tab = np.stack([getattr(self, n) for n in _TAB_ORDER]).astype(np.float32)
            self._dev_tabs[key] = th.from_numpy(tab).to(device).contiguous()
        return self._dev_tabs[key]

    def _fused_ok(self, *tensors):
        return all(t.is_cuda and t.dtype == th.float32 for t in tensors)

    device_map = None      # (SpacedDiffusion: device -> its timestep_map as an int64 tensor; None: the model sees the step itself)

    def _p_update(self):
        return _Update("hig_p_sample_step", self.device_table, True, False, ())

    def _fused_update(self, upd, x, eps, aux, t, B, scale=None, group=None, x_prev=None, pred=None):
        """ONE launch of `upd` on contiguous fp32 ROCm tensors of B samples (x, eps and t stacked to 2 B rows when guided)."""
        rows = B if group is None else 2 * B
        _launch_update(_lib.api, upd, x, eps, aux, t, upd.table(x.device), self.num_timesteps, B, x.numel() // rows,
                       th.cuda.current_stream(), scale, group, x_prev, pred)

    def _impose_known(self, x, known, mask, z, t, B, group=None):
        """ONE imposition launch on contiguous tensors of B samples, in place on x (x and t stacked to 2 B rows when guided)."""
        rows = B if group is None else 2 * B
        _launch_impose_known(_lib.api, x, known, mask, z, t, self.device_table(x.device), self.num_timesteps, B, x.numel() // rows,
                             th.cuda.current_stream(), group)

    # ---- q(x_t | x_0) ---------------------------------------------------------------------
    def q_mean_variance(self, x_start, t):
        """(mean, variance, log variance) of q(x_t | x_0), each of x_start's shape (gaussian_diffusion.py:382-397)."""
        shape = x_start.shape
        return (_extract_into_tensor(self.sqrt_alphas_cumprod, t, shape) * x_start,
                _extract_into_tensor(1.0 - self.alphas_cumprod, t, shape),
                _extract_into_tensor(self.log_one_minus_alphas_cumprod, t, shape))

    def q_sample(self, x_start, t, noise=None):
        """gaussian_diffusion.py:399-417."""
        if noise is None:
            noise = th.randn_like(x_start)
        assert noise.shape == x_start.shape
        if self._fused_ok(x_start, noise) and not x_start.requires_grad and not noise.requires_grad:
            x0, nz = x_start.contiguous(), noise.contiguous()
            out = th.empty_like(x0)
            B = x0.shape[0]
            _lib.api.hig_q_sample(x0, nz, t.long().contiguous(), self.device_table(x0.device), self.num_timesteps, B, x0.numel() // B, out)
            return out
        return (_extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
                + _extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    def q_posterior_mean_variance(self, x_start, x_t, t):
        """gaussian_diffusion.py:419-441."""
        assert x_start.shape == x_t.shape
        posterior_mean = (_extract_into_tensor(self.posterior_mean_coef1, t, x_t.shape) * x_start
                          + _extract_into_tensor(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        posterior_variance = _extract_into_tensor(self.posterior_variance, t, x_t.shape)
        posterior_log_variance_clipped = _extract_into_tensor(self.posterior_log_variance_clipped, t, x_t.shape)
        return posterior_mean, posterior_variance, posterior_log_variance_clipped

    # ---- p(x_{t-1} | x_t) -------------------------------------------------------------------
    def p_mean_variance(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None):
        """Model output -> {'mean', 'variance', 'log_variance', 'pred_xstart'} of p(x_{t-1} | x_t) for the fixed
        variances (gaussian_diffusion.py:443-537).  The x0 estimate goes through denoised_fn, then the clamp; for
        START_X / EPSILON the mean is the posterior q(x_{t-1} | x_t, x0_hat), for PREVIOUS_X it is the output itself."""
        B = x.shape[0]
        assert t.shape == (B,)
        out = model(x, self._scale_timesteps(t), **(model_kwargs or {}))
        if self.model_var_type == ModelVarType.FIXED_LARGE:
            # beta_t, with the first entry taken from the posterior variance (better decoder likelihood at t = 0)
            var_tab = np.append(self.posterior_variance[1], self.betas[1:])
            variance = _extract_into_tensor(var_tab, t, x.shape)
            log_variance = _extract_into_tensor(np.log(var_tab), t, x.shape)
        else:
            variance = _extract_into_tensor(self.posterior_variance, t, x.shape)
            log_variance = _extract_into_tensor(self.posterior_log_variance_clipped, t, x.shape)

        def finish(x0):
            if denoised_fn is not None:
                x0 = denoised_fn(x0)
            return x0.clamp(-1, 1) if clip_denoised else x0

        if self.model_mean_type == ModelMeanType.PREVIOUS_X:
            pred_xstart = finish(self._predict_xstart_from_xprev(x_t=x, t=t, xprev=out))
            mean = out
        else:
            pred_xstart = finish(out if self.model_mean_type == ModelMeanType.START_X
                                 else self._predict_xstart_from_eps(x_t=x, t=t, eps=out))
            mean = self.q_posterior_mean_variance(x_start=pred_xstart, x_t=x, t=t)[0]
        assert mean.shape == log_variance.shape == pred_xstart.shape == x.shape
        return {"mean": mean, "variance": variance, "log_variance": log_variance, "pred_xstart": pred_xstart}

    def _predict_xstart_from_eps(self, x_t, t, eps):
        assert x_t.shape == eps.shape
        return (_extract_into_tensor(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t
                - _extract_into_tensor(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * eps)

    def _predict_xstart_from_xprev(self, x_t, t, xprev):
        """Posterior mean solved for x0: (x_{t-1} - coef2 x_t) / coef1 (gaussian_diffusion.py:546-554)."""
        assert x_t.shape == xprev.shape
        return (_extract_into_tensor(1.0 / self.posterior_mean_coef1, t, x_t.shape) * xprev
                - _extract_into_tensor(self.posterior_mean_coef2 / self.posterior_mean_coef1, t, x_t.shape) * x_t)

    def _predict_eps_from_xstart(self, x_t, t, pred_xstart):
        """Inverse of _predict_xstart_from_eps (gaussian_diffusion.py:556-560)."""
        return ((_extract_into_tensor(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t - pred_xstart)
                / _extract_into_tensor(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape))

    def _scale_timesteps(self, t):
        if self.rescale_timesteps:
            return t.float() * (1000.0 / self.num_timesteps)
        return t

    def _is_trainer_branch(self, clip_denoised, denoised_fn, cond_fn, pre_seq, transl_req):
        return (self.model_mean_type == ModelMeanType.EPSILON
                and self.model_var_type == ModelVarType.FIXED_SMALL and not clip_denoised
                and denoised_fn is None and cond_fn is None and transl_req is None
                and not self.rescale_timesteps)      # (pre_seq / known: imposed before the step, whichever branch follows)

    # ---- known-region conditioning ---------------------------------------------------------
    def _q_sample_ops(self, x_start, t, noise):
        """q_sample as tensor arithmetic in the reference's operation order, whatever the device."""
        return (_extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
                + _extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    def _launch_impose(self, x, known, mask, z, t):
        """ONE hig_impose_known launch on x in place (through a contiguous copy when x is a strided view)."""
        xc = x if x.is_contiguous() else x.contiguous()
        self._impose_known(xc, known.contiguous(), mask, z.contiguous(), t.long().contiguous(), xc.shape[0])
        if xc is not x:
            x.copy_(xc)

    def _impose(self, x, t, known, known_mask, pre_seq, transl_req=None):
        """x <- the known part noised to level t, in place, where it is known (gaussian_diffusion.py:636-647); `t` indexes this
        object's own schedule.  The draws are the reference's: randn_like(pre_seq) [or randn_like(known)], then randn(2) per
        transl_req item.  fp32 ROCm tensors: one hig_impose_known launch; anything else: tensor arithmetic in the
        reference's operation order (a select, so NaN in known off the mask reaches nothing).  transl_req is always tensor
        arithmetic."""
        if pre_seq is not None:
            Fp = pre_seq.shape[2]
            noise = th.randn_like(pre_seq)
            if self._fused_ok(x, pre_seq, noise):
                kf, mask = _pre_seq_as_known(pre_seq, x.shape, x.device)
                z = th.zeros_like(kf)
                z[:, :, :Fp] = noise
                self._launch_impose(x, kf, mask, z, t)
            else:
                x[:, :, :Fp] = self._q_sample_ops(pre_seq, t, noise)
        elif known is not None:
            noise = th.randn_like(known)
            if self._fused_ok(x, known, noise) and known_mask.is_cuda:
                self._launch_impose(x, known, known_mask, noise, t)
            else:
                x.copy_(th.where(known_mask.to(x.device).bool(), self._q_sample_ops(known, t, noise).to(x.dtype), x))
        if transl_req is not None:
            for item in transl_req:
                noise = th.randn(2).type_as(x)
                transl = th.Tensor(item[1:]).type_as(x)
                x[:, :2, item[0]] = self._q_sample_ops(transl, t, noise)

    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, pre_seq=None,
                 transl_req=None, model_kwargs=None, known=None, known_mask=None):
        """gaussian_diffusion.py:606-666.  On the trainers' branch the whole update
        (x0-hat, posterior mean, noise) is ONE kernel; other branches use tensor ops.
        pre_seq (B, T, Fp) / transl_req [[j, v0, v1], ...] as in the reference, or known (B, T, F) + known_mask (bool / uint8,
        broadcastable): the known part, noised to level t, is written INTO THE CALLER'S x before the model sees it."""
        if cond_fn is not None:
            raise NotImplementedError("cond_fn guidance is never used by the reference tools")
        known, known_mask = _known_args(x.shape, known, known_mask, pre_seq, transl_req)
        if known is not None or pre_seq is not None or transl_req is not None:
            self._impose(x, t, known, known_mask, pre_seq, transl_req)
        if self._is_trainer_branch(clip_denoised, denoised_fn, cond_fn, pre_seq, transl_req) and self._fused_ok(x):
            eps = model(x, t, **(model_kwargs or {}))
            noise = th.randn_like(x)
            xc = x.contiguous()
            sample, pred = th.empty_like(xc), th.empty_like(xc)
            self._fused_update(self._p_update(), xc, eps.float().contiguous(), noise.contiguous(), t.long().contiguous(),
                               xc.shape[0], x_prev=sample, pred=pred)
            return {"sample": sample, "pred_xstart": pred}
        out = self.p_mean_variance(model, x, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                   model_kwargs=model_kwargs)
        noise = th.randn_like(x)
        nonzero_mask = (t != 0).float().view(-1, *([1] * (len(x.shape) - 1)))
        sample = out["mean"] + nonzero_mask * th.exp(0.5 * out["log_variance"]) * noise
        return {"sample": sample, "pred_xstart": out["pred_xstart"]}

    def _graph_ok(self, core, model_kwargs):
        """Whether a loop over `core` with these model_kwargs can be captured: our model, its text precomputed."""
        return (self.use_hip_graph and hasattr(core, "_launch_forward") and model_kwargs is not None
                and model_kwargs.get("xf_proj") is not None and model_kwargs.get("xf_out") is not None)

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, pre_seq=None, transl_req=None, progress=False, known=None,
                      known_mask=None):
        """gaussian_diffusion.py:668-716.  pre_seq / transl_req / known + known_mask: see p_sample; the captured loop takes
        pre_seq and known (one more launch per step), a call with transl_req runs eagerly."""
        core, cfg = _guided(model, model_kwargs)
        if self._graph_ok(core, model_kwargs) and self._is_trainer_branch(clip_denoised, denoised_fn, cond_fn, pre_seq, transl_req):
            known, known_mask = _known_args(shape, known, known_mask, pre_seq)
            return self._captured_loop(core, shape, noise, model_kwargs, device, self._p_update(), self.device_map, known, known_mask,
                                       pre_seq, cfg)
        return _last_sample(self.p_sample_loop_progressive(
            model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
            cond_fn=cond_fn, model_kwargs=model_kwargs, device=device, pre_seq=pre_seq,
            transl_req=transl_req, progress=progress, known=known, known_mask=known_mask))

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                  cond_fn=None, model_kwargs=None, device=None, pre_seq=None,
                                  transl_req=None, progress=False, known=None, known_mask=None):
        """gaussian_diffusion.py:718-769: t = N-1 ... 0, fresh noise every step, no_grad."""
        return self._loop_progressive(
            lambda img, t, last, **cond: self.p_sample(model, img, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                                       cond_fn=cond_fn, model_kwargs=model_kwargs, pre_seq=pre_seq,
                                                       transl_req=transl_req, **cond),
            model, shape, noise, device, progress, known, known_mask, pre_seq, transl_req)

    def _loop_progressive(self, step, model, shape, noise, device, progress, known, known_mask, pre_seq=None, transl_req=None):
        """The eager loop of every sampler: t = num_timesteps - 1 ... 0 under no_grad, yielding step(img, t, last, **cond), where
        `last` is what the step before yielded (None at the first) and cond the checked known + known_mask, if any."""
        if device is None:
            device = next(model.parameters()).device
        assert isinstance(shape, (tuple, list))
        known, known_mask = _known_args(shape, known, known_mask, pre_seq, transl_req)    # (the mask is expanded once)
        cond = {} if known is None else dict(known=known.to(device), known_mask=known_mask.to(device))
        img = noise if noise is not None else th.randn(*shape, device=device)
        indices = list(range(self.num_timesteps))[::-1]
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        out = None
        for i in indices:
            t = th.tensor([i] * shape[0], device=device)
            with th.no_grad():
                out = step(img, t, out, **cond)
                yield out
                img = out["sample"]

    def _captured_loop(self, core, shape, noise, model_kwargs, device, upd, device_map, known=None, known_mask=None, pre_seq=None,
                       cfg=None):
        """Every sampler's loop as ONE captured hipGraph step replayed num_timesteps times.  `upd` is the fused update; with a
        device_map (SpacedDiffusion's) the model is called at t_model = map[t_dev], the original timestep, and the counter is
        hig_advance_timesteps (t -= 1, t_model = map[t]); with None it is called at t_dev itself and the counter is
        hig_dec_timesteps.

        Captured per step: denoiser forward (text context hoisted: it is step-invariant), fresh Gaussian noise where the update
        reads any (torch's graph-safe Philox; DDIM at eta == 0 and dpmpp2m have no noise node and the update gets z = NULL), the
        fused update in place, the counter.  Nothing crosses PCIe inside the loop (the reference does ~8 H2D copies and B device
        syncs per step).  The warm-up step outside the graph builds the text context of this call's xf_out, whose
        buffer the captured forward reads: the graph is not kept beyond the call.

        With known + known_mask (or pre_seq, turned into that pair) the step opens with the imposition:
            zz.normal_() -> hig_impose_known(state, known, mask, zk, t_dev, device_table) -> forward -> update with z -> counter
        It reads t_dev, the index into this object's own table, not t_model.  zk (and z, where the update needs one) are parts of
        ONE buffer drawn by a single normal_(): a conditioned step has one launch more than an unconditioned one with noise, two
        more where the update reads no noise -- such a loop now draws noise and is no longer a pure function of its start.

        cfg (a ClassifierFreeGuidedModel around `core`): the state, the step vectors and the text inputs are kept in the stacked
        layout of models/guidance.py (2 B rows, the two rows of a sample equal), the forward runs once at 2 B, the _cfg entries
        take the place of the unguided kernels and the counter advances 2 B entries: launch for launch the unguided step, noise
        for B rows, and the B conditional rows returned.

        upd.history (dpmpp2m): `hist`, the x0 estimate of the step before, is one buffer of B rows (not stacked under guidance)
        that the kernel reads and rewrites in place.  The first step never reads it, so what the warm-up leaves there is
        harmless; it is cleared with the state all the same."""
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
            guide = {}
            if cfg is not None:
                group, xf_proj, xf_out, length = _stacked_inputs(cfg, B, xf_proj, xf_out, length)
                state = stack_rows(img, img, group).contiguous()
                guide = dict(scale=cfg.scale, group=group)
            else:
                state = img
            rows = state.shape[0]
            tmap = None if device_map is None else device_map(device)
            t_dev = th.full((rows,), K - 1, dtype=th.int64, device=device)
            t_model = t_dev if tmap is None else tmap[t_dev]
            hist = th.zeros_like(img) if upd.history else None
            if pre_seq is not None:
                known, known_mask = _pre_seq_as_known(pre_seq.float(), img.shape, device)
            cond = known is not None
            if cond:
                known = known.to(device).float().contiguous()
                known_mask = known_mask.to(device).contiguous()
                zz = th.zeros(2 if upd.needs_z else 1, *img.shape, device=device)
                zk, z = zz[0], (zz[1] if upd.needs_z else None)
            else:
                z = th.zeros_like(img) if upd.needs_z else None

            def step():
                if cond:
                    if not self._debug_zero_noise:
                        zz.normal_()
                    self._impose_known(state, known, known_mask, zk, t_dev, B, guide.get("group"))
                eps, _ = core._launch_forward(state, t_model, length, xf_proj, xf_out, training=False)
                if upd.needs_z and not cond and not self._debug_zero_noise:
                    z.normal_()
                self._fused_update(upd, state, eps, hist if upd.history else z, t_dev, B, x_prev=state, **guide)
                if tmap is None:
                    _lib.api.hig_dec_timesteps(t_dev, rows)
                else:
                    _lib.api.hig_advance_timesteps(t_dev, tmap, K, rows, t_model)

            # warm-up on a side stream (allocations, text context), then undo its effect
            img0 = state.clone()
            s = th.cuda.Stream()
            s.wait_stream(th.cuda.current_stream())
            with th.cuda.stream(s):
                step()
            th.cuda.current_stream().wait_stream(s)
            state.copy_(img0)
            if upd.history:
                hist.zero_()
            t_dev.fill_(K - 1)
            if tmap is not None:
                t_model.copy_(tmap[t_dev])
            graph = th.cuda.CUDAGraph()
            with th.cuda.graph(graph, capture_error_mode="thread_local"):
                step()
            # capture does not execute: state is still (img0, K - 1)
            for _ in range(K):
                graph.replay()
        return state if cfg is None else split_rows(state, group)[0].contiguous()

    # ---- training ---------------------------------------------------------------------------
    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None, forward_twice=False):
        """gaussian_diffusion.py:978-1055, MSE branch: {'mse', 'target', 'pred'}."""
        if model_kwargs is None:
            model_kwargs = {}
        if noise is None:
            noise = th.randn_like(x_start)
        x_t = self.q_sample(x_start, t, noise=noise)
        if forward_twice:
            B = x_t.size(0) // 2
            x_t = th.cat([x_t[:B], x_t[:B], x_t[B:], x_t[B:]])
            t = th.cat([t, t])
            x_start = th.cat([x_start[:B], x_start[:B], x_start[B:], x_start[B:]])
            noise = th.cat([noise[:B], noise[:B], noise[B:], noise[B:]])
        model_output = model(x_t, self._scale_timesteps(t), **model_kwargs)
        # regression target by what the model predicts: the injected noise (the trainers' choice), x_0, or the
        # posterior mean of x_{t-1}                                                 (gaussian_diffusion.py:1041-1047)
        if self.model_mean_type == ModelMeanType.EPSILON:
            target = noise
        elif self.model_mean_type == ModelMeanType.START_X:
            target = x_start
        else:
            target = self.q_posterior_mean_variance(x_start=x_start, x_t=x_t, t=t)[0]
        assert model_output.shape == target.shape == x_start.shape
        return {"mse": mean_flat((target - model_output) ** 2).view(-1, 1).mean(-1), "target": target,
                "pred": model_output}

    # ---- names kept for API compatibility; never reached by the reference tools --------------
    def ddim_sample(self, *a, **k):
        raise NotImplementedError("DDIM sampling is not used by any reference tool")

    ddim_sample_loop = ddim_reverse_sample = ddim_sample_loop_progressive = ddim_sample

    def calc_bpd_loop(self, *a, **k):
        raise NotImplementedError("VLB / bpd evaluation is not used by any reference tool")


def _extract_into_tensor(arr, timesteps, broadcast_shape):
    """gaussian_diffusion.py:1137-1150."""
    res = th.from_numpy(np.asarray(arr)).to(device=timesteps.device)[timesteps].float()
    while len(res.shape) < len(broadcast_shape):
        res = res[..., None]
    return res.expand(broadcast_shape)
