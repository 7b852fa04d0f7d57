"""MI355X-native `DDPMTrainer`.

Public surface = what the reference's tools call on its trainer (codes/trainers/ddpm_trainer.py:29-266:
`forward` / `backward_G` / `update`, `generate` / `generate_batch`, `save` / `load`, `train`, the attribute
names and the checkpoint keys); the bodies are this project's own and are organised around ONE training step:

  * `train_step_fused(...)`   explicit launches: q_sample -> [text head] -> denoiser forward -> masked MSE ->
                              denoiser backward -> ONE flat-buffer all-reduce (RCCL) -> fused clip(0.5)+Adam;
  * `train_step_captured(...)` the same step replayed as hipGraph(s);
  * `forward(batch)` + `update()`  the reference's autograd / torch-Adam sequence, kept so driver code written
                              against the reference runs unchanged (and as the parity anchor of the fused step).

`opt.fused_step` makes `train()` take the fused step; its Adam moments then live in flat device buffers and are
written to / restored from checkpoints in torch-Adam's own `state_dict` layout, so a checkpoint resumes under either
step (and under the reference's trainer).
"""
import contextlib
import time
import warnings
from collections import OrderedDict
from os.path import join as pjoin

import torch
import torch.distributed as dist
import torch.optim as optim
from torch.nn.utils import clip_grad_norm_

from .. import _lib
from ..models.gaussian_diffusion import (DeviceLossSecondMomentResampler, GaussianDiffusion, LossType, ModelMeanType,
                                         ModelVarType, create_named_schedule_sampler, get_named_beta_schedule, min_snr_weights)
from ..models.guidance import ClassifierFreeGuidedModel, check_scale
from ..models.spaced_diffusion import SpacedDiffusion, space_timesteps, space_timesteps_logsnr
from ..parallel import (FlatGradAllReduce, OverlappedGradAllReduce, ShardedSampler, broadcast_flat, broadcast_parameters,
                        exchange_active)
from .text_source import Banked, ClassIds, ClipFeatures, Embeddings, Tokens, _core

GRAD_CLIP = 0.5                    # ddpm_trainer.py:61
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8   # torch.optim.Adam defaults, ddpm_trainer.py:222


def _dist_world():
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def ema_options(opt):
    """(decay, warmup) of the EMA of the weights that `opt` asks for, or None: opt.ema_decay None or 0 (the default) is off,
    otherwise a number in (0, 1) -- anything else is a ValueError; opt.ema_warmup (default True) ramps the decay up as
    min(decay, (1 + n) / (10 + n)) (include/hig.h, 'EMA weights')."""
    d = getattr(opt, "ema_decay", None)
    if d is None or (not isinstance(d, bool) and isinstance(d, (int, float)) and d == 0):
        return None
    if isinstance(d, bool) or not isinstance(d, (int, float)) or not 0.0 < float(d) < 1.0:
        raise ValueError("opt.ema_decay must be None, 0 (no EMA) or a number in (0, 1), got %r" % (d,))
    if float(torch.tensor(float(d), dtype=torch.float32)) >= 1.0:
        raise ValueError("opt.ema_decay = %r rounds to 1 in fp32: the average would never move" % (d,))
    return float(d), bool(getattr(opt, "ema_warmup", True))


def loss_options(opt):
    """(loss_weighting, min_snr_gamma, sampler) that `opt` asks for.  opt.loss_weighting: None (the default: the unweighted
    masked MSE) or "min_snr", w_t = min(SNR_t, gamma) / SNR_t with opt.min_snr_gamma (default 5.0, a number > 0, inf allowed);
    opt.sampler: "uniform" (the default) or "loss-second-moment", t ~ sqrt(E[loss_t^2]) with each term weighted by
    1 / (N p_t) (include/hig.h, 'Per-timestep loss weights').  Anything else is a ValueError."""
    weighting = getattr(opt, "loss_weighting", None)
    if weighting not in (None, "min_snr"):
        raise ValueError("opt.loss_weighting must be None or 'min_snr', got %r" % (weighting,))
    gamma = getattr(opt, "min_snr_gamma", 5.0)
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not float(gamma) > 0.0:
        raise ValueError("opt.min_snr_gamma must be a number > 0, got %r" % (gamma,))
    sampler = getattr(opt, "sampler", "uniform")
    if sampler not in ("uniform", "loss-second-moment"):
        raise ValueError("opt.sampler must be 'uniform' or 'loss-second-moment', got %r" % (sampler,))
    return weighting, float(gamma), sampler


def check_loss_sampler_world(sampler, world):
    """The loss-aware sampler keeps one history per process: with more than one rank every rank would have to see every
    rank's (t, loss) pairs, and that gather is not built."""
    if sampler == "loss-second-moment" and world > 1:
        raise NotImplementedError("opt.sampler = 'loss-second-moment' with %d ranks: the cross-rank gather of (t, loss) that keeps "
                                  "the ranks' loss histories identical is not built -- train with one rank, or with "
                                  "opt.sampler = 'uniform' (opt.loss_weighting = 'min_snr' needs no exchange)" % world)


class _RunningMean:
    """Sums per-key values (host floats or device scalars -- the latter without any host sync) and hands back their
    means when the ITERATION COUNT is a multiple of `period` -- the reference prints at `it % log_every == 0`
    (ddpm_trainer.py:247-256), which after a resume from a checkpoint is not every `period` additions.  Only a rank
    that prints (`read=True`) reads the device scalars back; the others just drop the sums."""

    def __init__(self, period):
        self.period, self.n, self.acc = int(period), 0, OrderedDict()

    def add(self, values, it=None, read=True):
        for k, v in values.items():
            self.acc[k] = self.acc[k] + v if k in self.acc else (v.clone() if torch.is_tensor(v) else v)
        self.n += 1
        due = (it % self.period == 0) if it is not None else (self.n >= self.period)
        if not due:
            return None
        div = self.period if it is not None else self.n      # (the reference divides by log_every whatever it summed)
        out = OrderedDict((k, float(v) / div) for k, v in self.acc.items()) if read else None
        self.n, self.acc = 0, OrderedDict()
        return out


class DDPMTrainer(object):
    # both loss options unset (what a trainer assembled without __init__ gets): every route is the unweighted one
    _loss_cfg, _loss_dev = (None, 5.0, "uniform"), None

    def __init__(self, args, encoder):
        self.opt, self.device, self.encoder = args, args.device, encoder
        self.multi = False
        self.diffusion_steps = args.diffusion_steps
        self._loss_cfg = loss_options(args)      # (a bad option is refused here, not at the first step)
        self.sampler_name = self._loss_cfg[2]
        self._loss_dev = None          # _loss_state: the device weight table and, loss-aware, the device sampler (lazy)
        # the one diffusion every reference tool builds: linear betas, eps-prediction, fixed small variance, MSE
        self.diffusion = GaussianDiffusion(betas=get_named_beta_schedule('linear', self.diffusion_steps),
                                           model_mean_type=ModelMeanType.EPSILON,
                                           model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)
        # the host sampler of that name; a loss-aware trainer replaces it by the device one at its first step (_loss_state)
        self.sampler = create_named_schedule_sampler(self.sampler_name, self.diffusion)
        if args.is_train:
            self.mse_criterion = torch.nn.MSELoss(reduction='none')
        self._fused = None
        self._few_step = None          # set_sampler: (SpacedDiffusion, method, eta), or None = the full chain
        self._guidance_scale = None    # set_sampler: the classifier-free guidance scale, or None = unguided
        ema_options(args)              # (a bad opt.ema_decay is refused here, not at the first step)
        self._ema = None               # ema_state(): the EMA of the weights, lazy
        self._ema_scope = False        # inside `with trainer.ema_weights()`
        self._sample_weights = "model"   # set_sampler: which weights `generate` samples from
        # opt.caption_bank = capacity: the model keeps the frozen tower's output per caption (models/caption_bank.py);
        # opt.text_dedup (default True with a bank): the text head runs once per distinct caption of a step
        if getattr(args, "caption_bank", None):
            _core(encoder).enable_caption_bank(args.caption_bank)
            _core(encoder).text_dedup = bool(getattr(args, "text_dedup", True))
        self.to(self.device)

    # ---- small helpers the reference exposes as static methods ----------------------------------------------
    @staticmethod
    def zero_grad(opt_list):
        any(o.zero_grad() for o in opt_list)

    @staticmethod
    def clip_norm(network_list):
        any(clip_grad_norm_(net.parameters(), GRAD_CLIP) is None for net in network_list)

    @staticmethod
    def step(opt_list):
        any(o.step() for o in opt_list)

    def to(self, device):
        if hasattr(self, "mse_criterion"):
            self.mse_criterion.to(device)
        self.encoder = self.encoder.to(device)

    def train_mode(self):
        self.encoder.train()

    def eval_mode(self):
        self.encoder.eval()

    # ---- batch staging shared by both step flavours ---------------------------------------------------------
    def _stage_batch(self, batch_data):
        """(captions, motions (B,T,F), m_lens) -> captions, x_start on the device (fp32), lengths clamped to T."""
        caption, motions, m_lens = batch_data
        x_start = motions.detach().to(self.device).float()
        T = x_start.shape[1]
        cur_len = torch.tensor([min(T, int(n)) for n in m_lens], dtype=torch.int64).to(self.device)
        return caption, x_start, cur_len

    # ---- caption dropout (classifier-free guidance needs a model that also runs on the empty caption) ------------
    def _caption_keep(self, n):
        """None at opt.cond_drop_prob == 0 (no random number is drawn: existing runs keep their random stream); otherwise a
        list of n bools from ONE torch.rand(n) on the CPU generator: False = this caption is replaced by ""."""
        p = float(getattr(self.opt, "cond_drop_prob", 0.0))
        if not 0.0 <= p <= 1.0:
            raise ValueError("opt.cond_drop_prob must lie in [0, 1], got %r" % (p,))
        if p == 0.0:
            return None
        if getattr(self.opt, "cap_id", False):
            raise NotImplementedError("cond_drop_prob: cap_id models take class embeddings, not captions -- there is no empty "
                                      "caption to drop to")
        return (torch.rand(n) >= p).tolist()

    def _drop_captions(self, caption):
        keep = self._caption_keep(len(caption))
        if keep is None:
            return caption
        return [c if k else "" for c, k in zip(caption, keep)]

    # ---- per-timestep loss weights (include/hig.h, 'Per-timestep loss weights') --------------------------------------
    def _loss_state(self, device):
        """(wtab, sampler): the device table of per-timestep weights the losses index by t and, under
        opt.sampler = "loss-second-moment", the device sampler that keeps it -- (None, None) with both options unset, where
        every route is the unweighted one.  min-SNR alone: a static table.  Loss-aware: the sampler's `w`, into which the
        static table (or ones) is folded; `self.sampler` becomes that sampler."""
        weighting, gamma, name = self._loss_cfg
        if weighting is None and name == "uniform":
            return None, None
        check_loss_sampler_world(name, _dist_world())
        st = self._loss_dev
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:      # ("cuda" is the current device: not a reason to rebuild)
            device = torch.device("cuda", torch.cuda.current_device())
        if st is None or st["base"].device != device:
            base = min_snr_weights(self.diffusion.alphas_cumprod, gamma) if weighting == "min_snr" else None
            smp = None
            if name == "loss-second-moment":
                smp = DeviceLossSecondMomentResampler(self.diffusion.num_timesteps, device, base_w=base)
                if st is not None and st["sampler"] is not None:
                    smp.load_state_dict(st["sampler"].state_dict())
                self.sampler = smp
                tab = smp.base_w
            else:
                tab = torch.from_numpy(base).float().to(device)
            st = self._loss_dev = {"base": tab, "sampler": smp}
            if self._fused is not None:
                self._fused["graphs"] = {}
        smp = st["sampler"]
        return (st["base"] if smp is None else smp.w), smp

    def _draw_t(self, n, device):
        """n timesteps from the trainer's sampler: the host sampler's (numpy's generator), or the device sampler's
        torch.multinomial, which reads nothing back."""
        self._loss_state(device)
        return self.sampler.sample(n, device)[0]

    def _weighted(self, per_sample, count, t, lens, device):
        """The autograd route's objective: sum_i w[t_i] per_sample[i] / count (what the weighted loss kernels compute) and,
        under the loss-aware sampler, the history update with per_sample[i] / lens[i] behind it -- lens: the frames an entry
        was summed over, at least 1.  wtab None: the plain sum / count."""
        wtab, smp = self._loss_state(device)
        if wtab is None:
            return per_sample.sum() / count
        w = wtab[t[:per_sample.shape[0]].clamp(0, wtab.numel() - 1)]
        loss = (w * per_sample).sum() / count
        if smp is not None:
            smp.update(t.contiguous(), (per_sample.detach() / lens).float().contiguous())
        return loss

    def _loss_load(self, ent):
        """The 'schedule_sampler' entry of a checkpoint.  The history is restored only into a loss-aware trainer whose static
        table is the one it was recorded under (the rings hold base_w[t] * loss); any other difference between the
        checkpoint's loss options and this trainer's is a warning, never silence: the run then continues under this
        trainer's options, and is not the uninterrupted one."""
        weighting, gamma, name = self._loss_cfg
        if ent is None:
            if name == "loss-second-moment":
                warnings.warn("the checkpoint has no 'schedule_sampler' entry: the loss-aware sampler starts from an empty history")
            return
        theirs = (ent.get('loss_weighting'), ent.get('min_snr_gamma'), ent.get('sampler'))
        same_base = theirs[0] == weighting and (weighting is None or theirs[1] == gamma)
        if theirs[2] != name or not same_base:
            warnings.warn("the checkpoint was written under loss options (loss_weighting, min_snr_gamma, sampler) = %r, this "
                          "trainer has %r: training continues under this trainer's options%s"
                          % (theirs, (weighting, gamma, name),
                             ", from an empty loss history" if name == "loss-second-moment" else ""))
        if name == "loss-second-moment" and theirs[2] == name and same_base and 'history' in ent:
            self._loss_state(_core(self.encoder).flat_params().flat.device)[1].load_state_dict(ent)

    def _loss_key(self, device):
        wtab, _ = self._loss_state(device)
        return None if wtab is None else self._loss_cfg + (wtab.data_ptr(),)

    # ---- the reference's step: forward() then update() --------------------------------------------------------
    def forward(self, batch_data, eval_mode=False):
        """Noises the batch at sampled timesteps and runs the denoiser (ddpm_trainer.py:97-119); leaves
        `real_noise`, `fake_noise`, `src_mask` for `backward_G`."""
        caption, x_start, cur_len = self._stage_batch(batch_data)
        caption = self._drop_captions(caption)
        self.caption, self.motions = caption, x_start
        t = self._t = self._draw_t(x_start.shape[0], x_start.device)
        terms = self.diffusion.training_losses(model=self.encoder, x_start=x_start, t=t,
                                               model_kwargs=dict(text=caption, length=cur_len))
        self.real_noise, self.fake_noise = terms['target'], terms['pred']
        self.src_mask = _core(self.encoder).generate_src_mask(x_start.shape[1], cur_len).to(x_start.device)

    def backward_G(self):
        """Masked mean over valid frames of the per-frame feature-mean squared error (ddpm_trainer.py:172-178)."""
        per_frame = self.mse_criterion(self.fake_noise, self.real_noise).mean(dim=-1)
        if self._loss_cfg[0] is None and self._loss_cfg[2] == "uniform":
            self.loss_mot_rec = (per_frame * self.src_mask).sum() / self.src_mask.sum()
        else:   # sum_b w[t_b] sum_frames / sum(mask): what hig_masked_mse_w computes
            self.loss_mot_rec = self._weighted((per_frame * self.src_mask).sum(dim=1), self.src_mask.sum(), self._t,
                                               self.src_mask.sum(dim=1).clamp_min(1), per_frame.device)
        return OrderedDict(loss_mot_rec=self.loss_mot_rec.item())

    def update(self):
        """zero_grad -> loss -> backward -> clip_grad_norm_(0.5) -> Adam (ddpm_trainer.py:180-187)."""
        self._ema_refuse_in_scope("update")
        self.zero_grad([self.opt_encoder])
        logs = self.backward_G()
        self.loss_mot_rec.backward()
        self._exchange_param_grads()
        self.clip_norm([self.encoder])
        ema = self.ema_state()         # (before the step: a new EMA starts from the weights this step updates)
        self.step([self.opt_encoder])
        if ema is not None:
            self._ema_update_after_torch_step(ema)
        _core(self.encoder).params_changed()
        return logs

    def _exchange_param_grads(self):
        """The reference ALWAYS trains through a DDP wrapper when world > 1 (tools/train.py:77-82), whose reducer
        averages the gradients during backward().  When this trainer is handed a bare model in a multi-rank group,
        the same averaging happens here (one all-reduce of the flat gradient buffer + one per parameter outside it)
        instead of silently stepping every rank on its own gradient.  A wrapped model (`.module`) already did it."""
        world = _dist_world()
        if world == 1 or hasattr(self.encoder, "module"):
            return
        # (under autograd the parameter gradients are tensors of their own -- _DenoiserFn.backward hands out copies of
        # the flat buffer's views -- so they are packed into one message here, like one DDP bucket).  The message has a
        # FIXED layout -- every trainable parameter in `parameters()` order, zeros where a rank produced no gradient --
        # so that all ranks pair the same elements (DDP's buckets are laid out once, too); the buffer and its views are
        # cached across steps.
        params = [p for p in self.encoder.parameters() if p.requires_grad]
        if not params:
            return
        key = tuple((id(p), p.numel()) for p in params)
        cache = getattr(self, "_exchange_cache", None)
        if cache is None or cache[0] != key or cache[1].device != params[0].device:
            flat = torch.zeros(sum(p.numel() for p in params), device=params[0].device, dtype=torch.float32)
            views, o = [], 0
            for p in params:
                views.append(flat[o:o + p.numel()].view(p.shape))
                o += p.numel()
            cache = self._exchange_cache = (key, flat, views)
        _, flat, views = cache
        for p, v in zip(params, views):
            if p.grad is None:
                v.zero_()
            else:
                v.copy_(p.grad)
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        flat.mul_(1.0 / world)
        for p, v in zip(params, views):
            if p.grad is None:
                p.grad = v.clone()
            else:
                p.grad.copy_(v)

    # ---- EMA of the weights (include/hig.h, 'EMA weights') -------------------------------------------------------
    def _ema_outside_params(self):
        """[(state-dict name, parameter)] of what trains outside the flat buffer: a torch text head, a trainable CLIP tower
        (no_clip=True; with clip_tower_train="flat" it is in the buffer), the class head of a cap_id model built with
        class_head="torch" (with "hip" it is in the buffer)."""
        core = _core(self.encoder)
        fp = core.flat_params()
        in_flat = {id(p) for p, _ in fp.members()}
        return [(k, p) for k, p in core.named_parameters() if p.requires_grad and id(p) not in in_flat]

    def _ema_new(self, decay, warmup, origin, num_updates):
        """An EMA that equals the current weights: an fp32 twin of the flat buffer and one twin per outside tensor."""
        fp = _core(self.encoder).flat_params()
        outside = OrderedDict()
        for k, p in self._ema_outside_params():
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise NotImplementedError("EMA: trainable parameter %s is %s%s -- the EMA kernels take contiguous fp32"
                                          % (k, p.dtype, "" if p.is_contiguous() else ", not contiguous"))
            outside[k] = p.detach().clone()
        flat = torch.zeros_like(fp.flat)
        flat.copy_(fp.flat)
        self._ema = {"flat": flat, "outside": outside, "decay": float(decay), "warmup": bool(warmup), "origin": int(origin),
                     "num_updates": int(num_updates), "ptr": fp.flat.data_ptr()}
        return self._ema

    def ema_state(self, create=True):
        """The EMA of the weights, or None when there is none: {'flat': fp32 twin of the flat parameter buffer, 'outside':
        {name: twin} for trainable tensors outside it, 'decay', 'warmup', 'origin' (the Adam step count at which it was
        switched on), 'num_updates' (host count), 'ptr'}.  Created on first use when opt.ema_decay is set (a copy of the
        current weights); an EMA that a checkpoint brought along is kept up whether or not the option is set.  Tied to the flat
        buffer's pointer as `fused_state()` is: when `.to()` re-homes the parameters the EMA moves along, and the captured
        graphs (keyed on its pointer) are dropped."""
        st = self._ema
        if st is None and (not create or ema_options(self.opt) is None):
            return None                # (EMA off: nothing is touched, not even the flat buffer)
        fp = _core(self.encoder).flat_params()
        if st is not None and st["ptr"] != fp.flat.data_ptr():
            if st["flat"].numel() == fp.flat.numel():
                st["flat"] = st["flat"].to(fp.flat.device)
                now = dict(self._ema_outside_params())
                st["outside"] = OrderedDict((k, t.to(now[k].device)) for k, t in st["outside"].items() if k in now)
                st["ptr"] = fp.flat.data_ptr()
                if self._fused is not None:
                    self._fused["graphs"] = {}
            else:
                st = self._ema = None
        if st is None and create:
            cfg = ema_options(self.opt)
            if cfg is not None:
                origin = int(self._fused["step"].item()) if self._fused is not None else 0
                st = self._ema_new(cfg[0], cfg[1], origin, 0)
        return st

    def _ema_refuse_in_scope(self, what):
        if self._ema_scope:
            raise RuntimeError("%s inside `with trainer.ema_weights()`: the model holds the averaged weights there, leave the "
                               "scope first" % what)

    def _ema_update_after_torch_step(self, st):
        """Route 3: torch.optim.Adam has stepped; one hig_ema_update over the flat buffer, one per outside tensor."""
        fp = _core(self.encoder).flat_params()
        n_host = st["num_updates"] + 1
        args = (st["decay"], int(st["warmup"]), None, st["origin"], n_host)
        _lib.api.hig_ema_update(st["flat"], fp.flat, fp.numel, *args)
        now = dict(self._ema_outside_params())
        for k, e in st["outside"].items():
            _lib.api.hig_ema_update(e, now[k].data, e.numel(), *args)
        st["num_updates"] = n_host

    def _ema_exchange(self, st):
        """Weights <-> EMA in place (hig_swap_f32): no pointer moves, so parameter tables, derived-operand caches and captured
        training graphs stay valid; what is DERIVED from the weights (bf16 shadow, text context) follows params_changed()."""
        core = _core(self.encoder)
        fp = core.flat_params()
        _lib.api.hig_swap_f32(fp.flat, st["flat"], fp.numel)
        now = dict(self._ema_outside_params())
        for k, e in st["outside"].items():
            _lib.api.hig_swap_f32(now[k].data, e, e.numel())
        core.params_changed()
        if getattr(core, "storage", "f32") == "bf16" and getattr(fp, "_shadow", None) is not None:
            fp.shadow16(core._param_version())      # eagerly: a captured training graph reads the shadow without re-deriving it

    @contextlib.contextmanager
    def ema_weights(self):
        """`with trainer.ema_weights():` -- the model computes with the averaged weights inside, and has its own back, bit for
        bit, afterwards (a pure exchange on entry and on exit).  Inside, `update`, `train_step_fused`,
        `train_step_captured` and `save` raise RuntimeError, and so does a nested entry."""
        if self._ema_scope:
            raise RuntimeError("ema_weights() is already entered: the scope does not nest")
        st = self.ema_state()
        if st is None:
            raise RuntimeError("there is no EMA of the weights: set opt.ema_decay (e.g. 0.9999) before training, or load a "
                               "checkpoint that was written with it (key 'encoder_ema')")
        self._ema_exchange(st)
        self._ema_scope = True
        try:
            yield self
        finally:
            self._ema_exchange(st)
            self._ema_scope = False

    def _sampling_weights(self):
        """The scope `generate` runs in: nothing for weights="model", `ema_weights()` for "ema" (set_sampler)."""
        return self.ema_weights() if getattr(self, "_sample_weights", "model") == "ema" else contextlib.nullcontext()

    def _ema_state_dict(self, st):
        """state-dict name -> averaged tensor, trainable parameters only (a frozen CLIP tower is not duplicated)."""
        fp = _core(self.encoder).flat_params()
        off = {id(p): o for p, o in fp.members()}
        out = OrderedDict()
        for k, p in _core(self.encoder).named_parameters():
            if id(p) in off:
                out[k] = st["flat"][off[id(p)]:off[id(p)] + p.numel()].view(p.shape).clone()
            elif k in st["outside"]:
                out[k] = st["outside"][k].clone()
        return out

    def _ema_load(self, ck):
        """The EMA side of `load`: the checkpoint's EMA when it has one (opt.ema_decay / ema_warmup, where set, override its
        decay and warm-up); otherwise, under opt.ema_decay, a copy of the loaded weights whose origin is the loaded Adam
        step."""
        self._ema = None
        cfg = ema_options(self.opt)
        if 'encoder_ema' in ck and 'ema' in ck:
            info = ck['ema']
            decay, warmup = cfg if cfg is not None else (info['decay'], info['warmup'])
            st = self._ema_new(decay, warmup, info['origin'], info['num_updates'])
            fp = _core(self.encoder).flat_params()
            off = {id(p): o for p, o in fp.members()}
            with torch.no_grad():
                for k, p in _core(self.encoder).named_parameters():
                    if k not in ck['encoder_ema']:
                        continue
                    t = ck['encoder_ema'][k].to(p.device, torch.float32)
                    if id(p) in off:
                        st["flat"][off[id(p)]:off[id(p)] + p.numel()].copy_(t.reshape(-1))
                    elif k in st["outside"]:
                        st["outside"][k].copy_(t)
        elif cfg is not None:
            steps = [int(float(e['step'])) for e in ck.get('opt_encoder', {}).get('state', {}).values() if 'step' in e]
            self._ema_new(cfg[0], cfg[1], max(steps) if steps else 0, 0)

    # ---- sampling ----------------------------------------------------------------------------------------------
    def set_sampler(self, steps=None, method="ddpm", eta=0.0, guidance_scale=None, spacing=None, weights="model"):
        """How `generate` samples.  steps=None: the full ancestral chain of `self.diffusion` (the default).  Otherwise
        `steps` of the diffusion_steps training steps, walked by the ancestral update (method="ddpm"), by DDIM with the
        given eta (method="ddim"; eta = 0 is deterministic) or by the second-order multistep solver DPM-Solver++(2M)
        (method="dpmpp2m": needs `steps`, eta must be 0).  Training always uses self.diffusion.
        spacing: which steps are kept -- "uniform" in t (space_timesteps) or "logsnr", uniform in log-SNR
        (space_timesteps_logsnr).  None: "uniform" for ddpm and ddim, "logsnr" for dpmpp2m, whose extrapolation needs it.
        guidance_scale: classifier-free guidance, eps_u + s (eps_c - eps_u) with the empty caption as the unconditional
        branch (train with opt.cond_drop_prob > 0); kept independently of `steps`, so it applies to the full chain too.
        None or 1.0: unguided, launch for launch the loop without it.  ValueError unless it is a finite number.
        weights: "model" (the default: the weights as they are) or "ema": `generate` runs inside `ema_weights()`, once
        around all its chunks; without an EMA (opt.ema_decay, or a checkpoint that has one) that call is a RuntimeError."""
        if weights not in ("model", "ema"):
            raise ValueError("set_sampler: weights must be 'model' or 'ema', got %r" % (weights,))
        if method not in ("ddpm", "ddim", "dpmpp2m"):
            raise ValueError("set_sampler: method must be 'ddpm', 'ddim' or 'dpmpp2m', got %r" % (method,))
        eta = float(eta)
        if not 0.0 <= eta < float("inf"):
            raise ValueError("set_sampler: eta must be a finite number >= 0, got %r" % (eta,))
        if method == "dpmpp2m" and steps is None:
            raise ValueError("set_sampler: method 'dpmpp2m' needs steps")
        if method == "dpmpp2m" and eta != 0.0:
            raise ValueError("set_sampler: method 'dpmpp2m' is deterministic, eta must be 0, got %r" % (eta,))
        if spacing is None:
            spacing = "logsnr" if method == "dpmpp2m" else "uniform"
        if spacing not in ("uniform", "logsnr"):
            raise ValueError("set_sampler: spacing must be 'uniform' or 'logsnr', got %r" % (spacing,))
        scale = None if guidance_scale is None else check_scale(guidance_scale, "set_sampler")
        if scale is not None and scale != 1.0 and getattr(self, "cap_id", False):
            raise NotImplementedError("guidance on a cap_id model: it takes class embeddings, there is no empty caption")
        self._guidance_scale = None if scale == 1.0 else scale
        self._sample_weights = weights
        if steps is None:
            self._few_step = None
            return
        use = (space_timesteps(self.diffusion_steps, steps) if spacing == "uniform"
               else space_timesteps_logsnr(self.diffusion.betas, steps))
        spaced = SpacedDiffusion(use, betas=self.diffusion.betas,
                                 model_mean_type=self.diffusion.model_mean_type,
                                 model_var_type=self.diffusion.model_var_type, loss_type=self.diffusion.loss_type,
                                 rescale_timesteps=self.diffusion.rescale_timesteps)
        self._few_step = (spaced, method, eta)

    def _sample_loop(self, shape, model_kwargs, known=None, known_mask=None):
        """The sampling loop `set_sampler` chose, with the arguments every reference tool passes; known + known_mask (see
        GaussianDiffusion.p_sample) go to whichever loop that is."""
        cond = {} if known is None and known_mask is None else dict(known=known, known_mask=known_mask)
        model = self._guided_encoder(shape[0])
        if self._few_step is None:
            return self.diffusion.p_sample_loop(model, shape, clip_denoised=False, progress=True,
                                                model_kwargs=model_kwargs, **cond)
        spaced, method, eta = self._few_step
        if method == "ddim":
            return spaced.ddim_sample_loop(model, shape, clip_denoised=False, progress=True,
                                           model_kwargs=model_kwargs, eta=eta, **cond)
        if method == "dpmpp2m":
            return spaced.dpm_solver_sample_loop(model, shape, clip_denoised=False, progress=True,
                                                 model_kwargs=model_kwargs, **cond)
        return spaced.p_sample_loop(model, shape, clip_denoised=False, progress=True, model_kwargs=model_kwargs,
                                    **cond)

    def _guidance_group(self, B):
        """Rows per block of the stacked layout (models/guidance.py): the whole batch here, pairs in the two-person trainer."""
        return B

    def _guided_encoder(self, B):
        """The encoder itself without guidance; with a scale, the encoder under a ClassifierFreeGuidedModel whose
        unconditional branch is the empty caption, encoded once and expanded to the batch."""
        if getattr(self, "_guidance_scale", None) is None:
            return self.encoder
        if getattr(self, "cap_id", False):
            raise NotImplementedError("guidance on a cap_id model: it takes class embeddings, there is no empty caption")
        xf_proj, xf_out = _core(self.encoder).encode_text([""], self.device)
        uncond = dict(xf_proj=xf_proj.expand(B, *xf_proj.shape[1:]), xf_out=xf_out.expand(B, *xf_out.shape[1:]))
        return ClassifierFreeGuidedModel(self.encoder, self._guidance_scale, uncond, group=self._guidance_group(B))

    def _known_for(self, known, known_mask, T):
        """The conditioning pair of one model batch (B, >= T, F) on the device, the mask expanded to known's shape, both cut to
        T frames.  One of the pair alone is passed on as it is: the diffusion object refuses it."""
        if known is None or known_mask is None:
            return known, known_mask
        known = torch.as_tensor(known).to(self.device).float()
        known_mask = torch.broadcast_to(torch.as_tensor(known_mask).to(self.device), known.shape)
        return known[:, :T], known_mask[:, :T]

    def generate_batch(self, caption, m_lens, dim_pose, known=None, known_mask=None):
        """One chunk of captions -> (B, T, dim_pose) samples: text encoded once, then the sampling loop (the 1000-step
        chain unless set_sampler chose a shorter one; captured as a hipGraph by the diffusion object); T = longest
        requested length, capped at num_frames (:121-150).  known (B, >= T, dim_pose) + known_mask (bool / uint8,
        broadcastable to it): the part of the motion that is given, imposed before every step; both are cut to T frames."""
        core = _core(self.encoder)
        xf_proj, xf_out = core.encode_text(caption, self.device)
        T = min(int(m_lens.max()), core.num_frames)
        known, known_mask = self._known_for(known, known_mask, T)
        return self._sample_loop((len(caption), T, dim_pose), dict(xf_proj=xf_proj, xf_out=xf_out, length=m_lens),
                                 known, known_mask)

    def generate(self, caption, m_lens, dim_pose, batch_size=1024, known=None, known_mask=None):
        """All captions in chunks of `batch_size` -> python list of (T_chunk, dim_pose) tensors (:152-170).  known (N, T,
        dim_pose) + known_mask: sliced per chunk, cut to the chunk's T."""
        self.encoder.eval()
        if known is not None and known_mask is not None:
            known = torch.as_tensor(known)
            known_mask = torch.broadcast_to(torch.as_tensor(known_mask), known.shape)
        samples = []
        with self._sampling_weights():
            for lo in range(0, len(caption), batch_size):
                hi = min(len(caption), lo + batch_size)
                k = known if known is None else known[lo:hi]
                km = known_mask if known_mask is None or known is None else known_mask[lo:hi]
                samples.extend(self.generate_batch(caption[lo:hi], m_lens[lo:hi], dim_pose, known=k, known_mask=km).unbind(0))
        return samples

    # ---- checkpoints (keys: opt_encoder / ep / total_it / encoder, ddpm_trainer.py:200-218) ---------------------
    def _torch_optimizer(self):
        if not hasattr(self, "opt_encoder"):
            self.opt_encoder = optim.Adam(self.encoder.parameters(), lr=self.opt.lr)
        return self.opt_encoder

    def _fused_param_slots(self):
        """[(index in encoder.parameters(), flat offset, parameter)] for everything the fused Adam has stepped."""
        fp = _core(self.encoder).flat_params()
        index = {id(p): i for i, p in enumerate(self.encoder.parameters())}
        covered = self._fused["covered"] if self._fused else 0
        return [(index[id(p)], off, p) for p, off in fp.members() if off < covered and id(p) in index]

    def _optimizer_state_dict(self):
        """torch.optim.Adam.state_dict() of the optimizer that is really in use: when the fused step has run, its
        flat moments / step counter are laid out as Adam's per-parameter `exp_avg` / `exp_avg_sq` / `step`."""
        sd = self._torch_optimizer().state_dict()
        st = self._fused
        if st is None or int(st["step"].item()) == 0:
            return sd
        step = torch.tensor(float(st["step"].item()))
        for idx, off, p in self._fused_param_slots():
            n = p.numel()
            sd['state'][idx] = {'step': step.clone(), 'exp_avg': st["m"][off:off + n].view(p.shape).clone(),
                                'exp_avg_sq': st["v"][off:off + n].view(p.shape).clone()}
        return sd

    def _adopt_optimizer_state(self, sd):
        """The inverse: Adam moments of a checkpoint into the fused step's flat buffers."""
        st = self.fused_state()
        fp = _core(self.encoder).flat_params()
        index = {id(p): i for i, p in enumerate(self.encoder.parameters())}
        steps, covered = [], 0
        with torch.no_grad():
            for p, off in fp.members():
                ent = sd['state'].get(index.get(id(p)))
                if ent is None:
                    continue
                n = p.numel()
                st["m"][off:off + n].copy_(ent['exp_avg'].reshape(-1))
                st["v"][off:off + n].copy_(ent['exp_avg_sq'].reshape(-1))
                steps.append(int(float(ent['step'])))
                covered = max(covered, off + n)
            st["step"].fill_(max(steps) if steps else 0)
        st["covered"] = max(st["covered"], covered)

    def save(self, file_name, ep, total_it):
        """The reference's four keys; with an EMA of the weights two more, which the reference's `load` ignores:
        'encoder_ema' (state-dict names -> averaged tensors, trainable parameters only: loads into a reference-layout model
        with strict=False) and 'ema' ({'decay', 'warmup', 'origin', 'num_updates'})."""
        self._ema_refuse_in_scope("save")
        ck = {'opt_encoder': self._optimizer_state_dict(), 'ep': ep, 'total_it': total_it,
              'encoder': _core(self.encoder).state_dict()}
        ema = self.ema_state()
        if ema is not None:
            ck['encoder_ema'] = self._ema_state_dict(ema)
            ck['ema'] = {k: ema[k] for k in ('decay', 'warmup', 'origin', 'num_updates')}
        weighting, gamma, name = self._loss_cfg
        if weighting is not None or name != "uniform":
            # the loss options and, loss-aware, the history the next draw depends on (the reference's `load` ignores the key)
            ent = {'sampler': name, 'loss_weighting': weighting, 'min_snr_gamma': gamma}
            if name == "loss-second-moment":
                ent.update(self._loss_state(_core(self.encoder).flat_params().flat.device)[1].state_dict())
            ck['schedule_sampler'] = ent
        torch.save(ck, file_name)

    def load(self, model_dir):
        self._ema_refuse_in_scope("load")
        ck = torch.load(model_dir, map_location=self.device)
        core = _core(self.encoder)
        core.load_state_dict(ck['encoder'], strict=True)
        core.params_changed()
        if self.opt.is_train:
            self._torch_optimizer().load_state_dict(ck['opt_encoder'])
            if getattr(self.opt, "fused_step", False) or self._fused is not None:
                self._adopt_optimizer_state(ck['opt_encoder'])
        self._ema_load(ck)       # (also with is_train False: an inference-only trainer can sample from the average)
        self._loss_load(ck.get('schedule_sampler'))
        return ck['ep'], ck.get('total_it', 0)

    # ---- the epoch loop (ddpm_trainer.py:220-266: logging and checkpoint cadence) ----------------------------------
    def _loader(self, dataset, rank, world_size):
        sampler = ShardedSampler(len(dataset), rank, world_size, shuffle=True)
        return torch.utils.data.DataLoader(dataset, batch_size=self.opt.batch_size, sampler=sampler, drop_last=True,
                                           shuffle=False, num_workers=getattr(self.opt, "num_workers", 4))

    def sync_replicas(self):
        """Rank 0's trainable parameters (and fused Adam state) to every rank.  The fused step exchanges gradients
        itself instead of wrapping the model in DDP, so the construction-time broadcast DDP would do
        (tools/train.py:77-82) happens here.  Direct `train_step_fused` users with > 1 rank call this once first."""
        if _dist_world() == 1:
            return
        core = _core(self.encoder)
        fp = core.flat_params()
        broadcast_flat(fp.flat)
        in_flat = {id(p) for p, _ in fp.members()}
        for p in core.parameters():
            if p.requires_grad and id(p) not in in_flat:
                dist.broadcast(p.data, src=0)
        if self._fused is not None:
            for k in ("m", "v"):
                broadcast_flat(self._fused[k])
            stp = self._fused["step"].to(torch.int64)
            dist.broadcast(stp, src=0)
            self._fused["step"].copy_(stp.to(torch.int32))
        ema = self.ema_state()
        if ema is not None:     # (a deterministic function of the parameters, but a resumed rank 0 must win)
            broadcast_flat(ema["flat"])
            for e in ema["outside"].values():
                dist.broadcast(e, src=0)
            cnt = torch.tensor([ema["origin"], ema["num_updates"]], dtype=torch.int64, device=fp.flat.device)
            dist.broadcast(cnt, src=0)
            ema["origin"], ema["num_updates"] = int(cnt[0]), int(cnt[1])
        core.params_changed()

    def _one_step(self, batch_data, fused):
        if fused:   # the loss stays on the device; `_RunningMean` only reads it back when it prints
            return OrderedDict(loss_mot_rec=self.train_fused_batch(
                batch_data, captured=getattr(self.opt, "fused_graph", False)))
        self.forward(batch_data)
        return self.update()

    def train(self, train_dataset, rank, world_size):
        self.to(self.device)
        self.opt_encoder = optim.Adam(self.encoder.parameters(), lr=self.opt.lr)
        latest = pjoin(self.opt.model_dir, 'latest.tar')
        first_epoch, it = self.load(latest) if self.opt.is_continue else (0, 0)
        fused = bool(getattr(self.opt, "fused_step", False))
        if world_size > 1 and _dist_world() != world_size:
            raise RuntimeError("train(world_size=%d) needs an initialised process group of that size (found %d rank(s)): "
                               "start the ranks through hig_amd.parallel.launch / torchrun" % (world_size, _dist_world()))
        if fused:
            self.sync_replicas()
        elif world_size > 1 and not hasattr(self.encoder, "module"):
            broadcast_parameters(self.encoder)      # what DDP's constructor does; the step averages the gradients itself
            _core(self.encoder).params_changed()
        loader = self._loader(train_dataset, rank, world_size)
        meter, t_start = _RunningMean(self.opt.log_every), time.time()
        for epoch in range(first_epoch, self.opt.num_epochs):
            self.train_mode()
            for i, batch_data in enumerate(loader):
                it += 1
                means = meter.add(self._one_step(batch_data, fused), it=it, read=(rank == 0))
                if means is not None and rank == 0:
                    print('epoch: %3d niter: %6d inner_iter: %4d %.0fs %s' % (
                        epoch, it, i, time.time() - t_start, ' '.join('%s: %.4f' % kv for kv in means.items())))
                if it % self.opt.save_latest == 0 and rank == 0:
                    self.save(latest, epoch, it)
            if rank == 0:
                self.save(latest, epoch, it)
                if epoch % self.opt.save_every_e == 0:
                    self.save(pjoin(self.opt.model_dir, 'ckpt_e%03d.tar' % epoch), epoch, total_it=it)

    # ------------------------------------------------------------------------------------------
    # MI355X fused step
    # ------------------------------------------------------------------------------------------
    def fused_state(self):
        """Flat Adam moments, device scalars (loss, grad norm, step, lr) and scratch of the fused step (lazy).
        Tied to the model's flat parameter buffer: when `.to()` re-homes the parameters the moments move along and
        every captured graph (which holds raw pointers into the old buffers) is dropped."""
        core = _core(self.encoder)
        fp = core.flat_params()
        fp.ensure_grad()
        ptrs = (fp.flat.data_ptr(), fp.grad.data_ptr())
        st = self._fused
        if st is not None and st["ptrs"] != ptrs:
            dev = fp.flat.device
            if st["m"].numel() == fp.flat.numel():
                for k in ("m", "v", "scratch", "mse_scratch", "loss", "gnorm", "step", "lr"):
                    st[k] = st[k].to(dev)
                st["graphs"], st["ptrs"] = {}, ptrs
            else:
                st = self._fused = None
        if st is None:
            dev = fp.flat.device
            st = self._fused = {
                "m": torch.zeros_like(fp.flat), "v": torch.zeros_like(fp.flat),
                "scratch": torch.zeros(_lib.NORM_BLOCKS, device=dev, dtype=torch.float32),
                "mse_scratch": torch.zeros(_lib.NORM_BLOCKS, device=dev, dtype=torch.float32),
                "loss": torch.zeros(1, device=dev, dtype=torch.float32),
                "gnorm": torch.zeros(1, device=dev, dtype=torch.float32),
                "step": torch.zeros(1, device=dev, dtype=torch.int32),
                "lr": torch.full((1,), float(self.opt.lr), device=dev, dtype=torch.float32),
                "lr_host": float(self.opt.lr), "covered": 0, "graphs": {}, "ptrs": ptrs,
                "allreduce": FlatGradAllReduce(),
                "overlap": OverlappedGradAllReduce(wire=getattr(self.opt, "grad_wire", "f32")),
            }
        return st

    def _set_lr(self, lr):
        """Learning rate of the next fused update: a DEVICE scalar the Adam kernel reads, so a captured step follows
        an LR schedule without re-capture.  Written eagerly (never inside a capture), only when it changes."""
        st = self.fused_state()
        lr = float(self.opt.lr if lr is None else lr)
        if lr != st["lr_host"]:
            st["lr"].fill_(lr)
            st["lr_host"] = lr

    def _text_source(self, xf_proj, xf_out, clip_out, eot, caption_batch, class_ids, token_batch=None):
        """The text arguments of a fused step as ONE source (trainers/text_source.py).  `caption_batch=` is exclusive with
        `clip_out=` / `eot=` and needs the model's bank; `class_ids=` (a cap_id model with class_head="hip") is exclusive with
        every other text argument, and so is `token_batch=` (a no_clip model with clip_tower_train="flat").  Embeddings passed
        beside a bank request or beside CLIP features are ignored."""
        core = _core(self.encoder)
        if token_batch is not None:
            if any(a is not None for a in (xf_proj, xf_out, clip_out, eot, caption_batch, class_ids)):
                raise ValueError("token_batch= is exclusive with xf_proj= / xf_out=, clip_out= / eot=, caption_batch= and class_ids=: "
                                 "the tower and the text head inside the step supply the text embeddings")
            if getattr(core, "clip_tower_train", None) != "flat":
                raise ValueError("token_batch= needs a no_clip model built with clip_tower_train='flat' (or "
                                 "HIG_CLIP_TOWER_TRAIN=flat): this model's CLIP text tower is not in the flat parameter buffer")
            return Tokens(token_batch)
        if caption_batch is not None:
            if clip_out is not None or eot is not None:
                raise ValueError("caption_batch= and clip_out= / eot= are exclusive: the bank supplies the CLIP features")
            if getattr(core, "caption_bank", None) is None:
                raise RuntimeError("caption_batch= needs the model's caption bank (opt.caption_bank / enable_caption_bank)")
        if class_ids is not None:
            if any(a is not None for a in (xf_proj, xf_out, clip_out, eot, caption_batch)):
                raise ValueError("class_ids= is exclusive with xf_proj= / xf_out=, clip_out= / eot= and caption_batch=: the class head "
                                 "supplies the text embeddings")
            core._class_head_args(class_ids)      # (refuses a model without the HIP class head, and bad ids)
            return ClassIds(class_ids)
        if caption_batch is not None:
            return Banked(caption_batch)
        if clip_out is not None:
            return ClipFeatures(clip_out, eot)
        return Embeddings(xf_proj, xf_out)

    def _fused_fwd_bwd(self, x_start, t, length, text, noise, exchange=None):
        """[text head] -> q_sample -> denoiser forward -> masked MSE -> denoiser backward [-> text head backward] into the flat
        gradient.  `text` (of `_text_source`) supplies xf_proj / xf_out -- inputs, or computed here by the text head or the class
        head, which are then trained too (the reference's full update) -- and takes their gradients behind the denoiser's backward.
        `exchange` (an OverlappedGradAllReduce that has been begun): the gradient all-reduce of each decoder layer is
        started from inside the backward."""
        xf_proj, xf_out = text.forward(self)
        dxp, dxo = self._denoise_loss_backward(x_start, t, length, xf_proj, xf_out, noise, exchange)
        text.backward(self, dxp, dxo)

    def _denoise_loss_backward(self, x_start, t, length, xf_proj, xf_out, noise, exchange):
        """The middle of `_fused_fwd_bwd`; returns the gradients of the loss with respect to xf_proj and xf_out."""
        core = _core(self.encoder)
        st = self.fused_state()
        B, T, F = x_start.shape
        if noise is None:
            noise = torch.randn_like(x_start)
        x_t = self.diffusion.q_sample(x_start, t, noise=noise)
        pred, saved = core._launch_forward(x_t, t, length, xf_proj, xf_out, training=True)
        dpred = torch.empty_like(pred)
        wtab, smp = self._loss_state(pred.device)
        if wtab is None:
            _lib.api.hig_masked_mse(pred, noise, length, B, T, F, st["loss"], dpred, st["mse_scratch"])
        else:   # the weighted twin; loss-aware: the per-sample losses, then the history update BEHIND the loss launch, so
            # this step's loss has read the table its t was drawn under
            sl = None if smp is None else self._loss_buffer(st, "sample_loss", B, pred.device)
            scr = self._loss_buffer(st, "mse_w_scratch", _lib.NORM_BLOCKS + (0 if smp is None else B * T), pred.device)
            _lib.api.hig_masked_mse_w(pred, noise, length, t, wtab, wtab.numel(), B, T, F, st["loss"], dpred, sl, scr)
            if smp is not None:
                smp.update(t, sl)
        hook = {} if exchange is None else dict(layer_hook=exchange.layer_done, comm_stream=exchange.stream)
        _, dxp, dxo = core._launch_backward(x_t, t, length, xf_out, saved, dpred, want_dx=False, **hook)
        return dxp, dxo

    @staticmethod
    def _loss_buffer(st, name, n, device):
        """The fp32 buffer of n floats that the fused state keeps under (name, n, device).  One buffer per size, never replaced
        and never freed while the state lives: every captured graph holds the raw pointer of the buffer of ITS shape and mode,
        and graphs of several shapes and modes live side by side in st["graphs"]."""
        bufs = st.setdefault("loss_buffers", {})
        key = (name, int(n), torch.device(device))
        buf = bufs.get(key)
        if buf is None:
            buf = bufs[key] = torch.zeros(int(n), device=device, dtype=torch.float32)
        return buf

    def _fwd_bwd_overlapped_exchange(self, x_start, t, length, text, noise):
        """_fused_fwd_bwd with the gradient exchange of layer l issued while layers l-1 ... 0 are still in backward
        (RCCL on a side stream); returns the world size.  Capturable: see OverlappedGradAllReduce."""
        st = self.fused_state()
        core = _core(self.encoder)
        fp = core.flat_params()
        n = self._fused_numel(text)
        ex = st["overlap"]
        want = getattr(self.opt, "grad_wire", "f32")
        if want != ex.wire:      # (the option is read when the fused state is built; changing it later used to be ignored silently)
            raise RuntimeError("opt.grad_wire changed from %r to %r after the fused training state was created: set it before the "
                               "first step (or drop the state: trainer._fused = None)" % (ex.wire, want))
        nsty = 4 if int(getattr(core.dims(1, 1, 1), "two_person", 0)) == 1 else 3   # stylization blocks per layer
        per_layer, tail = fp.layer_buckets(core.num_layers, nsty, core.latent_dim, core.time_embed_dim)
        assert per_layer[-1][1][1] - per_layer[0][1][0] == core.num_layers * nsty * 2 * core.latent_dim * core.time_embed_dim
        ex.begin(fp.grad, per_layer, tail)
        self._fused_fwd_bwd(x_start, t, length, text, noise, exchange=ex)
        return ex.finish([(fp.core_numel, n)] if n > fp.core_numel else ())

    def _fused_numel(self, text):
        """Floats of the flat buffers one fused step covers: the core, core + text head or, for a source that runs the tower
        (Tokens), everything.  text: the step's source, or a bool = its `trains_head`."""
        core = _core(self.encoder)
        fp = core.flat_params()
        with_text = bool(getattr(text, "trains_head", text))
        if getattr(text, "trains_tower", False):
            if not fp.tower_params:
                raise RuntimeError("token_batch= needs a no_clip model built with clip_tower_train='flat': this model's CLIP text "
                                   "tower is not in the flat parameter buffer")
            return fp.numel
        if fp.tower_params:
            # the tower's parameters lie behind the head in the buffers: any other source leaves them without a gradient
            raise NotImplementedError("the CLIP text tower is trainable (no_clip=True) and lives in the flat parameter buffer "
                                      "(clip_tower_train='flat'): a step from %s would silently freeze it -- pass token_batch= "
                                      "(or use forward() + update())" % (getattr(text, "kind", "these inputs"),))
        if with_text:
            if not fp.text_params:
                raise RuntimeError("this model's text head is not on the HIP path (text_head='torch', cap_id without "
                                   "class_head='hip', or an unsupported head dim): the fused step cannot train it")
            clip_net = getattr(core, "clip", None)
            if clip_net is not None and any(p.requires_grad for p in clip_net.parameters()):
                # MotionInteractionTransformer(no_clip=True) trains the CLIP tower through forward()/update()
                # (interaction_transformer.py:424-427); the fused step runs CLIP frozen, outside the step
                raise NotImplementedError("the CLIP text tower is trainable (no_clip=True): the fused step would "
                                          "silently freeze it -- use forward() + update() for this configuration")
        return fp.numel if with_text else fp.core_numel

    def _fused_clip_adam(self, world, with_text=False):   # (with_text: the step's source, or a bool = its `trains_head`)
        """g /= world; clip_grad_norm_(0.5); Adam -- one norm pass + one update pass over the flat buffers."""
        core = _core(self.encoder)
        st = self.fused_state()
        fp = core.flat_params()
        n = self._fused_numel(with_text)
        _lib.api.hig_sumsq_partial(fp.grad, n, 1.0 / world, st["scratch"])
        bf16 = getattr(core, "storage", "f32") == "bf16"
        # bf16 storage: the update kernel also writes bf16(new parameters) into the weight shadow the next forward reads
        # (fp32 master weights, no separate cast pass over the 81 M parameters)
        shadow = fp.shadow16_buffer() if bf16 else None
        ema = self.ema_state()
        args = (fp.flat, fp.grad, st["m"], st["v"], n, st["lr_host"], st["lr"], ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, GRAD_CLIP,
                1.0 / world, st["scratch"], st["gnorm"], st["step"], shadow, fp.core_numel if bf16 else 0)
        if ema is None:
            _lib.api.hig_clip_adam_shadow(*args)
        else:   # the same pass also blends the new parameters into the EMA; its update number comes from the device counter
            _lib.api.hig_clip_adam_ema(*args, ema["flat"], ema["decay"], int(ema["warmup"]), ema["origin"])
        st["covered"] = max(st["covered"], n)
        core.params_changed()
        if bf16:
            fp.shadow16_mark_current(core._param_version())

    def train_step_fused(self, x_start, t, length, xf_proj=None, xf_out=None, noise=None, lr=None, clip_out=None,
                         eot=None, caption_batch=None, class_ids=None, token_batch=None):
        """One DDPM training step on device tensors, reference semantics (ddpm_trainer.py:97-119,172-187):
          x_t = q_sample(x0, t, noise); pred = denoiser(x_t, t); loss = masked MSE(pred, noise);
          backward; grads = all_reduce(grads) / world; clip_grad_norm_(0.5); Adam.
        With text embeddings (`xf_proj`, `xf_out`) the denoiser-core parameters are updated; with CLIP features
        (`clip_out` (B, N, W) batch-first, `eot` (B,), see MotionTransformer._clip_features) the text head runs
        inside the step and EVERY trainable parameter is updated -- the reference's full update.  `caption_batch` (a
        CaptionBatch of the model's caption bank, exclusive with clip_out / eot) is that same update with the CLIP features
        fetched from the bank by hig_caption_gather.  `class_ids` (int32 on the device, one class id per model-batch row --
        4 B rows in the order c1, c2, c2, c1 in PIT mode; exclusive with every other text argument) is the full update of a
        cap_id model built with class_head="hip": the class head runs inside the step.  `token_batch` (a clip_text.TokenBatch on
        the device; exclusive with every other text argument) is the full update of a no_clip model built with
        clip_tower_train="flat": the CLIP text tower runs inside the step, once per distinct caption, and is trained too.
        With more than one rank the replicas must start identical: call `sync_replicas()` once (train() does).
        No host synchronisation: the loss stays on the device (`fused_state()['loss']`)."""
        self._ema_refuse_in_scope("train_step_fused")
        text = self._text_source(xf_proj, xf_out, clip_out, eot, caption_batch, class_ids, token_batch)
        st = self.fused_state()
        ema = self.ema_state()            # (created here, from the weights before the step, when opt.ema_decay asks for one)
        n = self._fused_numel(text)
        self._set_lr(lr)
        core = _core(self.encoder)
        fp = core.flat_params()
        if OverlappedGradAllReduce.active() and getattr(self.opt, "overlap_allreduce", True):
            world = self._fwd_bwd_overlapped_exchange(x_start, t, length, text, noise)
        else:
            self._fused_fwd_bwd(x_start, t, length, text, noise)
            world = st["allreduce"](fp.grad[:n])                                  # one all-reduce after the backward
        self._fused_clip_adam(world, text)
        if ema is not None:
            ema["num_updates"] += 1
        return st["loss"]

    def train_fused_batch(self, batch_data, captured=False, noise=None):
        """forward(batch) + update() of the reference (ddpm_trainer.py:97-119,180-187) as ONE fused step over every
        trainable parameter: batch -> device, t ~ sampler, CLIP features -> train_step_fused (eager launches: measured
        faster than the replayed graph at every batch size since the backward runs on two streams), or
        train_step_captured with captured=True (two graph launches per step, no other host work)."""
        caption, x_start, cur_len = self._stage_batch(batch_data)
        caption = self._drop_captions(caption)
        t = self._draw_t(x_start.shape[0], x_start.device)
        step = self.train_step_captured if captured else self.train_step_fused
        return step(x_start.contiguous(), t, cur_len, noise=noise, **self._text_inputs(caption))

    def _text_inputs(self, caption):
        """The text arguments of a fused step for these captions: a TokenBatch for a model whose trainable tower lives in the flat
        buffer (clip_tower_train="flat"), a CaptionBatch when the model has a caption bank (the tower runs for captions the bank
        has not met, and only for them), else the tower's output for every row."""
        core = _core(self.encoder)
        if getattr(core, "clip_tower_train", None) == "flat":
            # the tower trains inside the step: its only text input is the distinct captions' tokens (opt.text_dedup, default on)
            from ..models.clip_text import TokenBatch
            cache = core.__dict__.setdefault("_token_cache", (core._clip_tokenize, {}))
            if cache[0] is not core._clip_tokenize:
                cache = core.__dict__["_token_cache"] = (core._clip_tokenize, {})
            return dict(token_batch=TokenBatch(caption, core._tokenize, dedup=bool(getattr(self.opt, "text_dedup", True)),
                                               cache=cache[1]).to(self.device))
        bank = getattr(core, "caption_bank", None)
        if bank is not None:
            return dict(caption_batch=bank.batch(caption, self.device))
        clip_out, eot = self.clip_inputs(caption)
        return dict(clip_out=clip_out, eot=eot)

    def clip_inputs(self, caption):
        """Captions -> (clip_out (B, N, W) batch-first fp32, eot (B,)) for `train_step_fused(clip_out=...)`: the
        frozen CLIP tower on its own ops, outside the fused / captured region."""
        core = _core(self.encoder)
        tokens, feat = core._clip_features(caption, self.device)
        clip_out = feat.permute(1, 0, 2)      # (the native tower's output is batch-first already: this view IS that buffer)
        if clip_out.dtype != torch.float32:
            clip_out = clip_out.float()
        if not clip_out.is_contiguous():
            clip_out = clip_out.contiguous()
        return clip_out, tokens.argmax(dim=-1).contiguous()

    def train_step_captured(self, x_start, t, length, xf_proj=None, xf_out=None, noise=None, lr=None, clip_out=None,
                            eot=None, caption_batch=None, class_ids=None, token_batch=None):
        """The same step as hipGraphs.  Captured once per batch shape.  One rank: ONE graph (q_sample [+ text head] +
        forward + loss + backward + clip + Adam).  With a gradient exchange (more than one rank, or HIG_FORCE_EXCHANGE)
        still ONE graph: the per-layer RCCL all-reduces of `OverlappedGradAllReduce` are captured with the backward they
        overlap (RCCL's kernels are graph nodes on the communication stream's branch), so a replay costs the host one
        launch and no per-collective work.  Fallback, taken when `opt.capture_exchange` is False or the capture of the
        collectives fails: graph A = ... + backward, the all-reduce of the flat gradient enqueued eagerly on the same
        stream, graph B = clip + Adam.  Inputs are copied into static device buffers; `t` arrives from the host
        sampler through the same staging copy (the reference draws it with numpy, gaussian_diffusion.py:47-62), the
        learning rate through a device scalar (`_set_lr`).  With opt.loss_weighting / opt.sampler set the weight table, the
        loss history and p are fixed device buffers, the history update is a node of the graph, `t` (drawn on the device by
        `train_fused_batch`) is filled device to device, and the graph key carries the mode and the table.
        A graph is keyed on the shapes AND on the flat parameter /
        gradient buffers it was captured against.  Text inputs as in `train_step_fused`: embeddings, or CLIP
        features.  The EMA of the weights rides in the same update kernel (its update number comes from the device step
        counter, its origin is a constant of the graph); the graph key carries its configuration.
        With `caption_batch` the packed int32 index buffer is the static text input, copied like `t`; the graph is keyed on
        its layout (rows, U_pad), on `text_dedup` and on the bank's buffers, which are allocated once and never move.
        With `class_ids` the ids are the static text input, copied like `t`; the graph key carries their shape and that the
        class head is inside.  With `token_batch` the packed token buffer is the static text input, copied like `t`; the embedding
        index is rebuilt from it by a node of the graph, its counts stay on the device, and the key carries (rows, U_pad, dedup)."""
        self._ema_refuse_in_scope("train_step_captured")
        text = self._text_source(xf_proj, xf_out, clip_out, eot, caption_batch, class_ids, token_batch)
        st = self.fused_state()
        ema = self.ema_state()            # (created eagerly, never inside a capture)
        world = _dist_world()
        split = exchange_active()         # there is an exchange to run (more than one rank, or HIG_FORCE_EXCHANGE)
        # (gloo stages through the host: its collectives cannot be captured -- that backend always takes the split form)
        in_graph = (split and getattr(self.opt, "capture_exchange", True) and getattr(self.opt, "overlap_allreduce", True)
                    and dist.get_backend() == "nccl")
        n = self._fused_numel(text)
        self._set_lr(lr)
        statics = text.statics()
        key = ((tuple(x_start.shape), text.kind) + tuple(tuple(a.shape) for a in statics)
               + (noise is None, world, split, in_graph, st["ptrs"],
                  None if ema is None else (ema["decay"], ema["warmup"], ema["origin"], ema["flat"].data_ptr()),
                  self._loss_key(x_start.device))
               + text.key(_core(self.encoder)))
        cap = st["graphs"].get(key)
        if cap is None:
            static = {"x0": x_start.clone(), "t": t.clone(), "length": length.clone(),
                      "text": tuple(a.clone() for a in statics), "noise": None if noise is None else noise.clone()}
            static_text = text.on(static["text"])

            def part_a():
                self._fused_fwd_bwd(static["x0"], static["t"], static["length"], static_text, static["noise"])

            def whole_step_with_exchange():
                w = self._fwd_bwd_overlapped_exchange(static["x0"], static["t"], static["length"], static_text, static["noise"])
                self._fused_clip_adam(w, text)

            # warm-up (allocations, workspace pools, RCCL's communicator) on a side stream, as torch.cuda.graph requires;
            # it runs a real step, so restore parameters / moments / step counter afterwards
            core = _core(self.encoder)
            fp = core.flat_params()
            keep = (fp.flat.clone(), st["m"].clone(), st["v"].clone(), st["step"].clone(), st["covered"],
                    None if ema is None else (ema["flat"].clone(), ema["num_updates"]))
            loss_smp = self._loss_state(x_start.device)[1]      # (the warm-up's step also pushes into the loss history)
            keep_smp = None if loss_smp is None else [a.clone() for a in loss_smp.tensors()]
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                if in_graph:
                    whole_step_with_exchange()
                else:
                    part_a()
                    self._fused_clip_adam(1, text)
            torch.cuda.current_stream().wait_stream(s)

            def restore():
                with torch.no_grad():
                    fp.flat.copy_(keep[0])
                    st["m"].copy_(keep[1])
                    st["v"].copy_(keep[2])
                    st["step"].copy_(keep[3])
                    if ema is not None:     # the warm-up's update also moved the EMA
                        ema["flat"].copy_(keep[5][0])
                        ema["num_updates"] = keep[5][1]
                    if loss_smp is not None:
                        for a, b in zip(loss_smp.tensors(), keep_smp):
                            a.copy_(b)
                st["covered"] = keep[4]
                core.params_changed()
                if getattr(core, "storage", "f32") == "bf16":   # the warm-up's update also wrote the bf16 shadow: re-derive it
                    fp.shadow16(core._param_version())          # from the restored master weights, eagerly (not inside the capture)
            restore()
            # thread_local: other threads (the RCCL watchdog polls its events) may call into HIP while we capture
            ga, gb = torch.cuda.CUDAGraph(), None
            if in_graph:
                # The warm-up's collectives have finished AND the process group's watchdog thread has retired them before any
                # event is recorded under capture (once, on a loaded box, it queried an event "last recorded in a capturing
                # stream" and took the process down: profiles/r05_notes.md section 5).  Round 6: no Work handle of the exchange
                # survives its call (parallel.OverlappedGradAllReduce._reduce) and the wait is the process group's own
                # waitForPendingWorks instead of a sleep.
                from ..parallel import all_ranks_agree, drain_pending_collectives
                drain_pending_collectives()
                err = None
                try:
                    with torch.cuda.graph(ga, capture_error_mode="thread_local"):
                        whole_step_with_exchange()
                except Exception as e:      # RCCL refused the capture
                    torch.cuda.synchronize()
                    err = "%s: %s" % (type(e).__name__, e)
                # The fallback changes the collectives a rank issues per step (one flat all-reduce instead of 2 L + 2 captured
                # ones): every rank takes it, or none does.
                if not all_ranks_agree(err is None, x_start.device):
                    st.setdefault("capture_exchange_errors", {})[key] = err or "another rank could not capture the exchange"
                    st["capture_exchange_error"] = st["capture_exchange_errors"][key]
                    in_graph = False
                    ga = torch.cuda.CUDAGraph()     # graph A | eager all-reduce | graph B
                    restore()
            if not split:
                with torch.cuda.graph(ga, capture_error_mode="thread_local"):
                    part_a()
                    self._fused_clip_adam(1, text)
            elif not in_graph:
                with torch.cuda.graph(ga, capture_error_mode="thread_local"):
                    part_a()
                gb = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gb, pool=ga.pool(), capture_error_mode="thread_local"):
                    self._fused_clip_adam(world, text)
            cap = st["graphs"][key] = (static, ga, gb)
            st["captured_form"] = "one graph" if not split else ("one graph, exchange inside" if in_graph
                                                                 else "graph A | all-reduce | graph B")
            st.setdefault("captured_forms", {})[key] = st["captured_form"]      # (per graph; "captured_form" = the latest capture)
        static, ga, gb = cap
        with torch.no_grad():
            static["x0"].copy_(x_start)
            static["t"].copy_(t)
            static["length"].copy_(length)
            for buf, a in zip(static["text"], statics):
                buf.copy_(a)
            if noise is not None:
                static["noise"].copy_(noise)
        ga.replay()
        if gb is not None:
            st["allreduce"](_core(self.encoder).flat_params().grad[:n])
            gb.replay()
        if ema is not None:
            ema["num_updates"] += 1
        st["covered"] = max(st["covered"], n)
        core = _core(self.encoder)
        core.params_changed()
        if getattr(core, "storage", "f32") == "bf16":       # (the replayed update kernel has just written the shadow)
            fp = core.flat_params()
            fp.shadow16_mark_current(core._param_version())
        return st["loss"]
