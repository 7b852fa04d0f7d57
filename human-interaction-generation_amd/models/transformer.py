"""MI355X-native `MotionTransformer`: same constructor, attributes, state-dict keys and call
signature as the reference module (codes/models/transformer.py:288-426), with the per-timestep
denoiser math running in hand-written HIP kernels behind the C ABI of include/hig.h.

`encode_text`: CLIP itself (frozen; stubbed when the `clip` package is absent) runs on
its own PyTorch ops; the trainable head behind it -- text_pre_proj, the 4-layer post-norm encoder, text_ln,
the EOT gather and text_proj -- goes through hig_text_head_fwd / _bwd (`text_head="torch"` keeps it on stock
ops, e.g. for head dims the kernels do not cover).  The nn.Modules of the head are parameter containers.

There is no CPU execution path: calling the module on host tensors, or without libhig.so, raises.
"""
import ctypes as C
import math
import os

import torch
from torch import nn

from .. import _lib

try:  # the real OpenAI CLIP when installed (transformer.py:10), else the deterministic stand-in
    import clip  # type: ignore
except Exception:  # pragma: no cover - depends on the environment
    from . import stub_clip as clip
from . import clip_text


def timestep_embedding(timesteps, dim, max_period=10000):
    """Sinusoidal embedding, cos first (transformer.py:15-32).  Device tensors go through the
    HIP kernel; kept as a module-level function because reference callers import it."""
    if timesteps.is_cuda:
        t = timesteps.long().contiguous()
        out = torch.empty(t.shape[0], dim, device=t.device, dtype=torch.float32)
        _lib.api.hig_timestep_embedding(t, t.shape[0], dim, out)
        return out
    raise RuntimeError("timestep_embedding: ROCm device tensor required (no CPU fallback)")


def set_requires_grad(nets, requires_grad=False):
    """transformer.py:35-48."""
    if not isinstance(nets, list):
        nets = [nets]
    for net in nets:
        if net is not None:
            for param in net.parameters():
                param.requires_grad = requires_grad


def zero_module(module):
    """transformer.py:51-57."""
    for p in module.parameters():
        p.detach().zero_()
    return module


# --- parameter containers: same submodule / key names as the reference; math lives in HIP -----
class StylizationBlock(nn.Module):
    """Parameters of transformer.py:60-73 (emb_layers.1, norm, out_layers.2 [zero-init])."""

    def __init__(self, latent_dim, time_embed_dim, dropout):
        super().__init__()
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(time_embed_dim, 2 * latent_dim))
        self.norm = nn.LayerNorm(latent_dim)
        self.out_layers = nn.Sequential(nn.SiLU(), nn.Dropout(p=dropout),
                                        zero_module(nn.Linear(latent_dim, latent_dim)))


class _SelfAttention(nn.Module):
    """Parameters of (Linear)TemporalSelfAttention, transformer.py:91-99 / 198-206."""

    def __init__(self, latent_dim, num_head, dropout, time_embed_dim):
        super().__init__()
        self.num_head = num_head
        self.norm = nn.LayerNorm(latent_dim)
        self.query = nn.Linear(latent_dim, latent_dim)
        self.key = nn.Linear(latent_dim, latent_dim)
        self.value = nn.Linear(latent_dim, latent_dim)
        self.dropout = nn.Dropout(dropout)
        self.proj_out = StylizationBlock(latent_dim, time_embed_dim, dropout)


class _CrossAttention(nn.Module):
    """Parameters of (Linear)TemporalCrossAttention, transformer.py:124-133 / 231-240."""

    def __init__(self, latent_dim, text_latent_dim, num_head, dropout, time_embed_dim):
        super().__init__()
        self.num_head = num_head
        self.norm = nn.LayerNorm(latent_dim)
        self.text_norm = nn.LayerNorm(text_latent_dim)
        self.query = nn.Linear(latent_dim, latent_dim)
        self.key = nn.Linear(text_latent_dim, latent_dim)
        self.value = nn.Linear(text_latent_dim, latent_dim)
        self.dropout = nn.Dropout(dropout)
        self.proj_out = StylizationBlock(latent_dim, time_embed_dim, dropout)


class FFN(nn.Module):
    """Parameters of transformer.py:157-165 (linear2 zero-init)."""

    def __init__(self, latent_dim, ffn_dim, dropout, time_embed_dim):
        super().__init__()
        self.linear1 = nn.Linear(latent_dim, ffn_dim)
        self.linear2 = zero_module(nn.Linear(ffn_dim, latent_dim))
        self.activation = nn.GELU()
        self.dropout = nn.Dropout(dropout)
        self.proj_out = StylizationBlock(latent_dim, time_embed_dim, dropout)


class _DecoderLayer(nn.Module):
    """transformer.py:173-194 / 264-285: sa_block -> ca_block -> ffn."""

    def __init__(self, latent_dim, text_latent_dim, time_embed_dim, ffn_dim, num_head, dropout):
        super().__init__()
        self.sa_block = _SelfAttention(latent_dim, num_head, dropout, time_embed_dim)
        self.ca_block = _CrossAttention(latent_dim, text_latent_dim, num_head, dropout, time_embed_dim)
        self.ffn = FFN(latent_dim, ffn_dim, dropout, time_embed_dim)


def _core_param_order(model):
    """(global table, per-layer tables) as lists of parameter groups in hig.h table order.
    A group with several parameters must be laid out contiguously (fused GEMM operand); an empty
    group is a NULL table entry (the two-person entries of a single-person model)."""
    blocks = list(model.temporal_decoder_blocks)

    def sty_blocks(b):  # stylization order the kernels index `ss` with: sa, ca, [int_ca], ffn
        ic = [b.int_ca_block.proj_out] if hasattr(b, "int_ca_block") else []
        return [b.sa_block.proj_out, b.ca_block.proj_out] + ic + [b.ffn.proj_out]

    stys = [s for b in blocks for s in sty_blocks(b)]
    two = hasattr(model, "joint_embed2")
    glob = [
        [model.sequence_embedding],
        [model.joint_embed.weight], [model.joint_embed.bias],
        [model.time_embed[0].weight], [model.time_embed[0].bias],
        [model.time_embed[2].weight], [model.time_embed[2].bias],
        [s.emb_layers[1].weight for s in stys], [s.emb_layers[1].bias for s in stys],
        [model.out.weight], [model.out.bias],
        [model.joint_embed2.weight] if two else [], [model.joint_embed2.bias] if two else [],
        [model.out2.weight] if two else [], [model.out2.bias] if two else [],
    ]
    layers = []
    for b in blocks:
        sa, ca, ff = b.sa_block, b.ca_block, b.ffn
        lay = [
            [sa.norm.weight], [sa.norm.bias],
            [sa.query.weight, sa.key.weight, sa.value.weight], [sa.query.bias, sa.key.bias, sa.value.bias],
            [sa.proj_out.norm.weight], [sa.proj_out.norm.bias],
            [sa.proj_out.out_layers[2].weight], [sa.proj_out.out_layers[2].bias],
            [ca.norm.weight], [ca.norm.bias], [ca.text_norm.weight], [ca.text_norm.bias],
            [ca.query.weight], [ca.query.bias],
            [ca.key.weight, ca.value.weight], [ca.key.bias, ca.value.bias],
            [ca.proj_out.norm.weight], [ca.proj_out.norm.bias],
            [ca.proj_out.out_layers[2].weight], [ca.proj_out.out_layers[2].bias],
            [ff.linear1.weight], [ff.linear1.bias], [ff.linear2.weight], [ff.linear2.bias],
            [ff.proj_out.norm.weight], [ff.proj_out.norm.bias],
            [ff.proj_out.out_layers[2].weight], [ff.proj_out.out_layers[2].bias],
        ]
        if hasattr(b, "int_ca_block"):
            ic = b.int_ca_block
            lay += [
                [ic.norm.weight], [ic.norm.bias],
                [ic.query.weight, ic.key.weight, ic.value.weight], [ic.query.bias, ic.key.bias, ic.value.bias],
                [ic.proj_out.norm.weight], [ic.proj_out.norm.bias],
                [ic.proj_out.out_layers[2].weight], [ic.proj_out.out_layers[2].bias],
            ]
        else:
            lay += [[] for _ in range(8)]
        layers.append(lay)
    assert len(glob) == _lib.NGLOBAL and all(len(l) == _lib.NLAYER for l in layers)
    return glob, layers


class _FlatParams:
    """One contiguous fp32 device buffer holding every denoiser-core parameter (and a twin for
    gradients) so that (a) q/k/v, key/value and the 3L stylization `emb_layers` matrices are
    single fused-GEMM operands, (b) the RCCL all-reduce and the fused clip+Adam see ONE buffer.
    The nn.Parameters become views into it; state-dict names/shapes are untouched.
    The text-head parameters (when the model has a HIP text head) follow the core in the same
    buffer -- `[0, core_numel)` core, `[core_numel, numel)` text head -- so the fused training step
    can update everything that is trainable with one all-reduce and one clip+Adam.  With
    `clip_tower_train="flat"` (a `no_clip` model) the trainable CLIP text tower follows the text head:
    `tower_params` / `tower_offsets`.  The bf16 weight shadow stays core-only."""

    ALIGN = 64  # floats (256 B)

    def __init__(self, model):
        glob, layers = _core_param_order(model)
        groups = glob + [g for l in layers for g in l]
        self.params = [p for g in groups for p in g]          # denoiser core, hig.h table order
        dev = self.params[0].device
        assert all(p.device == dev and p.dtype == torch.float32 for p in self.params)
        offs, o = [], 0
        self.group_offsets = []
        for g in groups:
            o = (o + self.ALIGN - 1) // self.ALIGN * self.ALIGN
            self.group_offsets.append(o if g else None)
            for p in g:
                offs.append(o)
                o += p.numel()
        self.core_numel = (o + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.offsets = offs
        # text head (HIG_T_* / HIG_TL_* order), one aligned group per tensor
        self.text_params = list(model._text_params()) if model._has_hip_text_head() else []
        if not self.text_params and model._has_hip_class_head():
            # a cap_id model with class_head="hip": the class head's three tensors stand where the text head goes
            self.text_params = list(model._class_params())
        if not all(p.device == dev and p.dtype == torch.float32 for p in self.text_params):
            self.text_params = []
        self.text_offsets, o = [], self.core_numel
        for p in self.text_params:
            self.text_offsets.append(o)
            o += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        # the trainable CLIP tower (clip_tower_train="flat"; clip_text._tower_tensors order), one aligned group per tensor, behind
        # the text head: `[core_numel + head, numel)`.  A new option does not fall back: what cannot be placed raises.
        self.tower_params, self.tower_offsets = [], []
        if getattr(model, "clip_tower_train", None) == "flat":
            why = None if self.text_params and model._has_hip_text_head() else "the text head is not on the HIP path"
            # (on the host only the layout exists -- the CPU tests read it -- and the rule's device clause has nothing to say)
            why = why or clip_text.tower_refusal(model.clip, dev if dev.type == "cuda" else None, trainable=True)
            if why is not None:
                raise RuntimeError("clip_tower_train='flat': the CLIP text tower cannot join the flat parameter buffer: " + why)
            self.tower_params = list(clip_text._tower_tensors(model.clip))
            for p in self.tower_params:
                self.tower_offsets.append(o)
                o += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.numel = o
        self.flat = torch.zeros(self.numel, device=dev, dtype=torch.float32)
        with torch.no_grad():
            for p, off in self.members():
                view = self.flat[off:off + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
        if self.tower_params:
            model._clip_train_table = None      # (its pointers were the tensors' old homes)
        self.grad = None
        self.grad_views = None
        self._ptr_key = None
        self._ptable = None
        self._gtable = None

    def members(self):
        """[(parameter, flat offset)] of everything that lives in the buffer: the core, the text (or class) head, the tower."""
        return list(zip(self.params + self.text_params + self.tower_params, self.offsets + self.text_offsets + self.tower_offsets))

    def tower_grad_table(self):
        """Pointer table (clip_text._tower_tensors order) into the flat GRADIENT buffer."""
        self.ensure_grad()
        return (C.c_void_p * len(self.tower_offsets))(*[self.grad.data_ptr() + 4 * o for o in self.tower_offsets])

    def table(self, base_ptr):
        n = len(self.group_offsets)
        arr = (C.c_void_p * n)()
        for i, off in enumerate(self.group_offsets):
            arr[i] = None if off is None else base_ptr + 4 * off
        return arr

    def param_table(self):
        key = self.flat.data_ptr()
        if self._ptr_key != key:
            self._ptable, self._ptr_key = self.table(key), key
        return self._ptable

    def ensure_grad(self):
        if self.grad is None:
            self.grad = torch.zeros_like(self.flat)
            self.grad_views = [self.grad[o:o + p.numel()].view(p.shape)
                               for p, o in zip(self.params, self.offsets)]
            self._gtable = self.table(self.grad.data_ptr())
        return self._gtable

    def text_grad_table(self, slots):
        """Pointer table (HIG_T_* order, NULL where `slots` is False) into the flat GRADIENT buffer."""
        self.ensure_grad()
        arr = (C.c_void_p * len(slots))()
        it = iter(self.text_offsets)
        for i, present in enumerate(slots):
            arr[i] = self.grad.data_ptr() + 4 * next(it) if present else None
        return arr

    def layer_param(self, l, slot, n):
        """The first n floats of group `slot` (_lib.L_*) of decoder layer l in the flat buffer; None for an empty group."""
        o = self.group_offsets[_lib.NGLOBAL + l * _lib.NLAYER + slot]
        return None if o is None else self.flat[o:o + n]

    def layer_buckets(self, num_layers, nsty, d, E):
        """Element ranges [(start, stop), ...] of the flat gradient that are FINAL when decoder layer l's backward is
        done (`per_layer[l]`: the layer's own parameters + its rows of the stacked stylization emb_layers.1.weight), and
        the ranges that are only final at the end of the backward (`tail`: the global parameters)."""
        ng, nl = _lib.NGLOBAL, _lib.NLAYER
        offs = self.group_offsets

        def first_of_layer(l):
            return next(o for o in offs[ng + l * nl: ng + (l + 1) * nl] if o is not None)

        starts = [first_of_layer(l) for l in range(num_layers)] + [self.core_numel]
        o_w = offs[_lib.P_STY_EMB_W]
        rows = nsty * 2 * d * E
        per_layer = [[(starts[l], starts[l + 1]), (o_w + l * rows, o_w + (l + 1) * rows)] for l in range(num_layers)]
        tail = [(0, o_w), (o_w + num_layers * rows, starts[0])]
        return per_layer, tail

    def shadow16(self, version):
        """bf16 shadow of the flat buffer (same offsets, 2 bytes per element) and its pointer table, rebuilt by one
        cast kernel whenever `version` (the caller's view of "the parameters changed") moves."""
        if getattr(self, "_shadow", None) is None or self._shadow.data_ptr() != getattr(self, "_shadow_ptr", None):
            self._shadow = torch.empty(self.core_numel, device=self.flat.device, dtype=torch.bfloat16)
            self._shadow_ptr = self._shadow.data_ptr()
            n = len(self.group_offsets)
            self._stable = (C.c_void_p * n)()
            for i, off in enumerate(self.group_offsets):
                self._stable[i] = None if off is None else self._shadow_ptr + 2 * off
            self._shadow_version = None
        if self._shadow_version != (version, self.flat.data_ptr()):
            _lib.api.hig_cast_bf16(self.flat, self._shadow, self.core_numel)
            self._shadow_version = (version, self.flat.data_ptr())
        return self._stable

    def shadow16_buffer(self):
        """The bf16 shadow tensor itself (allocated, contents unspecified): hig_clip_adam_shadow writes it."""
        if getattr(self, "_shadow", None) is None or self._shadow.data_ptr() != getattr(self, "_shadow_ptr", None):
            self.shadow16(object())       # allocate + one cast; the sentinel version never matches again
        return self._shadow

    def shadow16_mark_current(self, version):
        """The optimizer kernel has just written bf16(parameters) into the shadow: `version` is current without a cast pass."""
        self._shadow_version = (version, self.flat.data_ptr())

    def valid(self):
        base, end = self.flat.data_ptr(), self.flat.data_ptr() + 4 * self.numel
        return all(p.is_cuda and base <= p.data_ptr() < end for p in self.params[:3] + self.params[-3:]) \
            and all(p.data_ptr() == base + 4 * o for p, o in zip(self.params[:8], self.offsets[:8])) \
            and all(p.data_ptr() == base + 4 * o for p, o in zip(self.text_params, self.text_offsets)) \
            and all(p.data_ptr() == base + 4 * o for p, o in zip(self.tower_params, self.tower_offsets))


class _DerivedTable:
    """A derived-operand table of include/hig.h (_lib.D32_* / _lib.D16_*): `nlayer` slots per layer for L layers, then the
    globals; NULL where nothing is set.  Keeps the tensors it points to alive."""

    def __init__(self, nlayer, nglobal, L):
        self.nlayer, self.L = nlayer, L
        self.ptrs = (C.c_void_p * (nlayer * L + nglobal))()
        self.bufs = []

    def set_layer(self, l, slot, t):
        self._set(self.nlayer * l + slot, t)

    def set_global(self, slot, t):
        self._set(self.nlayer * self.L + slot, t)

    def _set(self, i, t):
        self.bufs.append(t)
        self.ptrs[i] = t.data_ptr()


_POISON = __import__("os").environ.get("HIG_POISON", "0") == "1"


class _WorkspacePool:
    """Scratch buffers keyed by (kind, bytes).  A forward that needs its activations kept for
    backward holds its buffer until backward returns it."""

    def __init__(self):
        self.free = {}

    def take(self, kind, nbytes, device):
        lst = self.free.setdefault((kind, nbytes, str(device)), [])
        buf = lst.pop() if lst else torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
        if _POISON:   # debugging aid (HIG_POISON=1): every scratch byte starts as NaN, so a kernel that reads
            buf.fill_(0xFF)   # workspace it did not write first shows up as NaN in the outputs
        return buf

    def give(self, kind, buf, device):
        self.free.setdefault((kind, buf.numel(), str(device)), []).append(buf)


class _DenoiserFn(torch.autograd.Function):
    """Autograd boundary: forward = hig_text_context + hig_denoiser_fwd(training=1),
    backward = hig_denoiser_bwd.  Parameter gradients come back as copies of the views of the
    flat gradient buffer (the fused trainer path reads the flat buffer directly instead)."""

    @staticmethod
    def forward(ctx, model, x, t, length, xf_proj, xf_out, *params):
        out, saved = model._launch_forward(x, t, length, xf_proj, xf_out, training=True)
        ctx.model, ctx.saved = model, saved
        ctx.save_for_backward(x, t, length, xf_out)
        ctx.need = (x.requires_grad, xf_proj.requires_grad, xf_out.requires_grad)
        return out

    @staticmethod
    def backward(ctx, dout):
        model = ctx.model
        x, t, length, xf_out = ctx.saved_tensors
        dx, dxp, dxo = model._launch_backward(x, t, length, xf_out, ctx.saved, dout.contiguous(),
                                              want_dx=ctx.need[0])
        ctx.saved = None
        pg = tuple(g.clone() for g in model._flat.grad_views)
        return (None, dx if ctx.need[0] else None, None, None, dxp if ctx.need[1] else None,
                dxo if ctx.need[2] else None) + pg


class _TextHeadFn(torch.autograd.Function):
    """Autograd boundary of the text head (hig_text_head_fwd / _bwd): CLIP features (B, N, W) and the
    EOT indices in, (xf_proj, xf_out) out; the parameters are passed so autograd routes their
    gradients (one flat scratch buffer per backward, returned as views)."""

    @staticmethod
    def forward(ctx, model, clip_out, eot, *params):
        xf_proj, xf_out, saved = model._launch_text_head(clip_out, eot, training=True)
        ctx.model, ctx.saved = model, saved
        ctx.save_for_backward(clip_out, eot, xf_out)
        ctx.need_clip = clip_out.requires_grad
        return xf_proj, xf_out

    @staticmethod
    def backward(ctx, dxf_proj, dxf_out):
        clip_out, eot, xf_out = ctx.saved_tensors
        grads, dclip = ctx.model._launch_text_head_backward(clip_out, eot, xf_out, ctx.saved, dxf_out, dxf_proj,
                                                           ctx.need_clip)
        ctx.saved = None
        return (None, dclip, None) + tuple(grads)


class MotionTransformer(nn.Module):
    """Drop-in for the reference class (transformer.py:288-426)."""

    def __init__(self, input_feats, num_frames=240, latent_dim=512, ff_size=1024, num_layers=8,
                 num_heads=8, dropout=0, activation="gelu", num_text_layers=4, text_latent_dim=256,
                 text_ff_size=2048, text_num_heads=4, no_clip=False, no_eff=False, **kargs):
        super().__init__()
        if dropout != 0:
            # every reference tool uses the constructor default p=0; the fused
            # kernels implement exactly that
            raise NotImplementedError("dropout != 0 is not supported by the fused denoiser")
        self.num_frames = num_frames
        self.latent_dim = latent_dim
        self.ff_size = ff_size
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.dropout = dropout
        self.activation = activation
        self.input_feats = input_feats
        self.time_embed_dim = latent_dim * 4
        self.text_latent_dim = text_latent_dim
        self.no_eff = no_eff
        self.sequence_embedding = nn.Parameter(torch.randn(num_frames, latent_dim))

        # Text side: CLIP + the parameter containers of the text head (transformer.py:318-340)
        # (`clip_model=`: a module used in place of clip.load's, e.g. models.clip_text.load_text_tower(...))
        self.clip = kargs["clip_model"] if kargs.get("clip_model") is not None else clip.load('ViT-B/32', "cpu")[0]
        if no_clip:
            self.clip.initialize_parameters()
        else:
            set_requires_grad(self.clip, False)
        if text_latent_dim != 512:
            self.text_pre_proj = nn.Linear(512, text_latent_dim)
        else:
            self.text_pre_proj = nn.Identity()
        layer = nn.TransformerEncoderLayer(d_model=text_latent_dim, nhead=text_num_heads,
                                           dim_feedforward=text_ff_size, dropout=dropout,
                                           activation=activation)
        self.textTransEncoder = nn.TransformerEncoder(layer, num_layers=num_text_layers,
                                                      enable_nested_tensor=False)
        self.text_ln = nn.LayerNorm(text_latent_dim)
        self.text_proj = nn.Sequential(nn.Linear(text_latent_dim, self.time_embed_dim))
        self._init_clip_route(kargs)

        # Denoiser core (parameters only; the math is in libhig.so)
        self.joint_embed = nn.Linear(self.input_feats, self.latent_dim)
        self.time_embed = nn.Sequential(
            nn.Linear(self.latent_dim, self.time_embed_dim),
            nn.SiLU(),
            nn.Linear(self.time_embed_dim, self.time_embed_dim),
        )
        self.temporal_decoder_blocks = nn.ModuleList(
            _DecoderLayer(latent_dim, text_latent_dim, self.time_embed_dim, ff_size, num_heads, dropout)
            for _ in range(num_layers))
        self.out = zero_module(nn.Linear(self.latent_dim, self.input_feats))

        # product arithmetic of the forward GEMMs: "f32" (exact fp32 MFMA, default), "bf16x3"
        # (split-bf16, ~1e-5 relative, 16x-rate MFMA) or "bf16"; HIG_PREC overrides the default
        import os
        self.precision = kargs.get("precision", os.environ.get("HIG_PREC", "f32"))
        # "hip": the text head runs through hig_text_head_fwd/_bwd; "torch": stock PyTorch-ROCm ops
        self.text_head = kargs.get("text_head", os.environ.get("HIG_TEXT_HEAD", "hip"))
        # "f32": fp32 activations / weights (default).  "bf16": bf16 activations + a bf16 shadow of the weight
        # matrices, fp32 accumulation and statistics (BASELINE configs 3 / 5) -- inference only
        self.storage = kargs.get("storage", os.environ.get("HIG_STORAGE", "f32"))
        self._flat = None
        self._pool = _WorkspacePool()
        self._textctx_cache = None
        self._param_epoch = 0
        # inference only: keep the cross-attention text context of the last `xf_out` (it is step-invariant, so the
        # sampling loop computes it once); False = recompute on every forward, as the reference does (:144-150)
        self.cache_text_context = True

    # ---- nn.Module plumbing -------------------------------------------------------------
    def _init_clip_route(self, kargs):
        # `clip_tokenize=`: a callable used in place of the module-level clip.tokenize (the BPE vocabulary is data the stub
        # does not have).  `clip_tower`: "hip" runs a qualifying frozen tower through hig_clip_text_fwd (clip_text.tower_refusal
        # is the rule; the stub and a trainable tower never qualify), "torch" keeps the tower on stock PyTorch ops.
        self._clip_tokenize = kargs.get("clip_tokenize")
        self.clip_tower = kargs.get("clip_tower", os.environ.get("HIG_CLIP_TOWER", "hip"))
        if self.clip_tower not in ("hip", "torch"):
            raise ValueError("clip_tower must be 'hip' or 'torch' (got %r)" % (self.clip_tower,))
        self._clip_table = None
        # `caption_bank=capacity`: keep the frozen tower's output per caption string on the device (models/caption_bank.py) and
        # fetch it by slot instead of running the tower; None / 0 (the default): no bank, nothing launches differently.
        # `text_dedup` (with a bank): run the text head once per DISTINCT caption where no autograd graph is asked for.
        self._caption_bank = None
        self.text_dedup = bool(kargs.get("text_dedup", True))
        if kargs.get("caption_bank"):
            self.enable_caption_bank(kargs["caption_bank"])

    @property
    def caption_bank(self):
        return getattr(self, "_caption_bank", None)

    def enable_caption_bank(self, capacity, spill=None):
        """Turn the caption bank on with `capacity` persistent slots (157 696 bytes each at N = 77, W = 512); ValueError for a
        trainable tower or a cap_id model.  None / 0 turns it off."""
        if not capacity:
            self._caption_bank = None
            return None
        from .caption_bank import DEFAULT_SPILL, CaptionBank
        self._caption_bank = CaptionBank(self, capacity, DEFAULT_SPILL if spill is None else spill)
        return self._caption_bank

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._flat = None            # .to()/.cuda()/.float() re-home parameters: re-flatten lazily
        self._textctx_cache = None
        self._clip_table = None
        if self.caption_bank is not None:
            self._caption_bank.clear()
        return r

    def params_changed(self):
        """Tell the model its parameters were modified behind autograd's back (a fused optimizer kernel writing the
        flat buffer, a checkpoint load): drops everything derived from them."""
        self._param_epoch += 1
        self._textctx_cache = None

    def _load_from_state_dict(self, *a, **k):
        self._textctx_cache = None
        self._clip_table = None
        if self.caption_bank is not None:
            self._caption_bank.clear()
        return super()._load_from_state_dict(*a, **k)

    def _textctx_param_version(self):
        """Sum of the autograd version counters of every parameter the text context is built from.  The
        nn.Parameters are re-homed VIEWS of the flat buffer, so an in-place update through them (torch optimizers,
        load_state_dict, p.copy_) bumps THEIR counter, never the flat buffer's."""
        v = self._param_epoch
        for blk in self.temporal_decoder_blocks:
            ca = blk.ca_block
            for p in (ca.key.weight, ca.key.bias, ca.value.weight, ca.value.bias, ca.text_norm.weight, ca.text_norm.bias):
                v += p._version
        return v

    def _param_version(self):
        """Moves whenever any core parameter may have changed (see `_textctx_param_version`)."""
        return self._param_epoch + sum(p._version for p in self.flat_params().params)

    def _bf16(self):
        if self.storage not in ("f32", "bf16"):
            raise ValueError("storage must be 'f32' or 'bf16' (got %r)" % (self.storage,))
        return self.storage == "bf16"

    def flat_params(self):
        """Flat fp32 buffer aliasing every core parameter (built on first use on the device)."""
        if self._flat is None or not self._flat.valid():
            if not self.out.weight.is_cuda:
                raise RuntimeError("MotionTransformer: parameters must live on a ROCm device "
                                   "(call .to('cuda')); there is no CPU fallback")
            self._flat = _FlatParams(self)
        return self._flat

    def core_parameters(self):
        return list(self.flat_params().params)

    # ---- reference API ------------------------------------------------------------------
    def _clip_features(self, text, device):
        """Frozen CLIP text tower up to ln_final (transformer.py:381-388): tokens + (L, B, 512)."""
        with torch.no_grad():
            text = self._tokenize(text).to(device)
            table = self._clip_native_table(text)
            if table is not None:   # the frozen tower in HIP (csrc/cliptext.hip); always exact-fp32 products
                return text, clip_text.tower_forward(table, text, self._pool).permute(1, 0, 2)
            x = self.clip.token_embedding(text).type(self.clip.dtype)
            x = x + self.clip.positional_embedding.type(self.clip.dtype)
            x = x.permute(1, 0, 2)
            x = self.clip.transformer(x)
            x = self.clip.ln_final(x).type(self.clip.dtype)
        return text, x

    def _tokenize(self, text):
        return (self._clip_tokenize or clip.tokenize)(text, truncate=True)

    def _clip_native_table(self, tokens):
        """The pointer table of the tower when `_clip_features` takes the native route for these tokens, else None: the flag
        is "hip", the tokens are on a ROCm device and clip_text.tower_refusal finds nothing (checked once, when the table is
        built; a tower that did not qualify is asked again only after `_apply` or a load)."""
        if self.clip_tower != "hip" or not tokens.is_cuda or getattr(self, "no_clip", False):
            return None
        if not hasattr(getattr(self.clip, "transformer", None), "resblocks"):
            return None
        t = self._clip_table
        if isinstance(t, clip_text.TowerTable) and (t.device != tokens.device or t.stale()):
            t = None
        if t is None:
            try:
                t = clip_text.TowerTable(self.clip, tokens.device)
            except clip_text.TowerRefused:
                t = False
            self._clip_table = t
        return t or None

    def _text_head_torch(self, text, x, eot=None):
        """transformer.py:389-397 on stock torch ops (`text_head="torch"`); eot: the EOT positions when there are no tokens."""
        x = self.text_pre_proj(x)
        xf_out = self.textTransEncoder(x)
        xf_out = self.text_ln(xf_out)
        xf_proj = self.text_proj(xf_out[text.argmax(dim=-1) if eot is None else eot, torch.arange(xf_out.shape[1])])
        xf_out = xf_out.permute(1, 0, 2)
        return xf_proj, xf_out

    def encode_text(self, text, device):
        """transformer.py:380-397.  CLIP stays on its own (frozen / stubbed) ops; the trainable head
        after it -- text_pre_proj, the post-norm encoder, text_ln, EOT gather, text_proj -- runs in
        the HIP kernels.  With a caption bank the CLIP features come from hig_caption_gather instead of the
        tower, and where no autograd graph is asked for (and `text_dedup`) the head runs on the distinct captions only."""
        if self.caption_bank is not None:
            return self._encode_text_banked(text, device)
        text, x = self._clip_features(text, device)
        return self._text_head(text, x)

    def _encode_text_banked(self, text, device):
        from .caption_bank import expand_rows
        bank = self._caption_bank
        cb = bank.batch([text] if isinstance(text, str) else list(text), device)
        wants_graph = torch.is_grad_enabled() and any(p.requires_grad for p in self._text_params())
        if wants_graph or not self.text_dedup:
            clip_out, eot = bank.gather(cb.slot, cb.rows)
            return self._text_head(None, clip_out.permute(1, 0, 2), eot=eot)
        clip_out, eot = bank.gather(cb.uniq_slot, cb.U_pad)
        xf_proj, xf_out = self._text_head(None, clip_out.permute(1, 0, 2), eot=eot)
        return (expand_rows(xf_proj.detach().contiguous(), cb.inv, cb.rows),
                expand_rows(xf_out.detach().contiguous(), cb.inv, cb.rows))

    def _text_head(self, text, x, eot=None):
        """tokens (B, N) + CLIP features (N, B, W) -> xf_proj (B, E), xf_out (B, N, Lt); eot (B,): the EOT positions, for
        features that come without their tokens (the caption bank)."""
        if self.text_head == "torch":
            return self._text_head_torch(text, x, eot)
        if not x.is_cuda:
            raise RuntimeError("encode_text: ROCm device required (no CPU fallback); pass text_head='torch' "
                               "to run the text head on stock PyTorch ops")
        clip_out = x.permute(1, 0, 2).float().contiguous()
        eot = (text.argmax(dim=-1) if eot is None else eot).contiguous()
        tp = self._text_params()
        if torch.is_grad_enabled() and (clip_out.requires_grad or any(p.requires_grad for p in tp)):
            return _TextHeadFn.apply(self, clip_out, eot, *tp)
        xf_proj, xf_out, _ = self._launch_text_head(clip_out, eot, training=False)
        return xf_proj, xf_out

    def generate_src_mask(self, T, length):
        """(B, T) float CPU mask, mask[i, j] = j < length[i] (transformer.py:399-405); the
        trainer calls this directly (ddpm_trainer.py:116-119).  The kernels build their own
        mask from `length` on the device."""
        length = torch.as_tensor(length).detach().to("cpu", torch.int64).view(-1)
        return (torch.arange(T)[None, :] < length[:, None]).float()

    def dims(self, B, T, N):
        return _lib.Dims(B=B, T=T, F=self.input_feats, d=self.latent_dim, H=self.num_heads,
                         ff=self.ff_size, L=self.num_layers, N=N, Lt=self.text_latent_dim,
                         num_frames=self.num_frames,
                         attn_kind=_lib.ATTN_FULL if self.no_eff else _lib.ATTN_LINEAR,
                         prec={"f32": _lib.PREC_F32, "bf16x3": _lib.PREC_BF16X3, "bf16": _lib.PREC_BF16}[self.precision],
                         storage=_lib.STORE_BF16 if getattr(self, "storage", "f32") == "bf16" else _lib.STORE_F32)

    def forward(self, x, timesteps, length=None, text=None, xf_proj=None, xf_out=None):
        """x: (B, T, F) -> (B, T, F)   (transformer.py:407-426)."""
        B, T = x.shape[0], x.shape[1]
        if xf_proj is None or xf_out is None:
            xf_proj, xf_out = self.encode_text(text, x.device)
        if not x.is_cuda:
            raise RuntimeError("MotionTransformer.forward: ROCm device tensors required "
                               "(no CPU fallback; the CPU restatement lives in oracle/ for tests only)")
        assert x.shape[2] == self.input_feats and T <= self.num_frames
        return self._run(x, timesteps, length, xf_proj, xf_out)

    def _run(self, x, timesteps, length, xf_proj, xf_out):
        """Normalise the inputs and launch (through autograd when anything requires grad)."""
        B, T = x.shape[0], x.shape[1]
        dev = x.device
        x = x.float().contiguous()
        t = timesteps.to(dev).long().contiguous()
        assert t.shape == (B,)
        if length is None:
            length = torch.full((B,), T, dtype=torch.int64, device=dev)
        else:
            length = torch.as_tensor(length).to(dev).long().contiguous()
        xf_proj = xf_proj.float().contiguous()
        xf_out = xf_out.float().contiguous()
        fp = self.flat_params()
        needs_grad = torch.is_grad_enabled() and (
            x.requires_grad or xf_proj.requires_grad or xf_out.requires_grad
            or any(p.requires_grad for p in fp.params))
        if needs_grad:
            self._check_bf16_training()
            return _DenoiserFn.apply(self, x, t, length, xf_proj, xf_out, *fp.params)
        out, _ = self._launch_forward(x, t, length, xf_proj, xf_out, training=False)
        return out

    def _check_bf16_training(self):
        """storage='bf16' trains the single-person AND the two-person model with linear attention (hig_denoiser_fwd_bf16_train /
        _bwd_bf16: fp32 master weights, gradients and optimizer state; bf16 activations and matrix products)."""
        if self._bf16() and self.no_eff:
            raise NotImplementedError("storage='bf16' trains with linear attention only (no_eff: train with fp32 storage; "
                                      "precision='bf16x3' / 'bf16' select reduced-precision products there)")

    # ---- launches -----------------------------------------------------------------------
    def _text_context(self, dims, xf_out, training):
        """Cross-attention text side (all layers).  Cached on (storage, version) of xf_out and the
        parameter version, so the 1000-step sampling loop computes it once (it is step-invariant)."""
        fp = self.flat_params()
        use_cache = not training and self.cache_text_context
        if use_cache:
            key = (xf_out.data_ptr(), xf_out._version, tuple(xf_out.shape), fp.flat.data_ptr(),
                   fp.flat._version, self._textctx_param_version(), self.precision, self.storage)
            if self._textctx_cache is not None and self._textctx_cache[0] == key:
                return self._textctx_cache[1]
        nbytes = _lib.api.hig_textctx_bytes(dims, training)
        if training:
            buf = self._pool.take("textctx_t", nbytes, xf_out.device)
        elif use_cache:
            buf = torch.empty(nbytes, dtype=torch.uint8, device=xf_out.device)
        else:   # one reusable buffer: the caller's forward consumes it on the same stream before the next call
            buf = self._pool.take("textctx_i", nbytes, xf_out.device)
            self._pool.give("textctx_i", buf, xf_out.device)
        if self._bf16() and training:
            _lib.api.hig_text_context_bf16_train(dims, fp.param_table(), fp.shadow16(self._param_version()), xf_out, buf)
        elif self._bf16():
            _lib.api.hig_text_context_bf16(dims, fp.param_table(), fp.shadow16(self._param_version()), xf_out, buf)
        else:
            _lib.api.hig_text_context(dims, fp.param_table(), xf_out, buf, training)
        if use_cache:
            self._textctx_cache = (key, buf, xf_out)  # keep xf_out alive so the key stays unique
        return buf

    @staticmethod
    def _frag16(W16):
        """(J, R) bf16 weight -> the same elements in the operand order of v_mfma_f32_32x32x16_bf16 (hig_weight_frag16):
        blocks of 32 rows x 16 reduce elements, each 64 lanes x 8 elements, lane = j % 32 + 32 ((r % 16) / 8)."""
        J, R = W16.shape
        return W16.view(J // 32, 32, R // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()

    def _text_kv_fold(self, fp):
        """The batched text side's operands (include/hig.h, the TEXT_* derived globals): [key; value](LN_text(xf)) =
        xhat (gamma (.) W)^T + (W beta + b) with xhat = (xf - mean) rstd the same in every layer (transformer.py:146,150), so
        the folded weights of ALL layers stacked make ONE GEMM.  Returns the stacked fp32 weights (L 2d, Lt), all keys in front
        of all values ([K_0 .. K_{L-1} | V_0 .. V_{L-1}]: one context-build launch for all layers), the bias' in the same
        order, and Lt ones / Lt zeros (the affine-free LayerNorm of the text rows).  fp64 arithmetic, fp32 results."""
        d, Lt = self.latent_dim, self.text_latent_dim
        wt, bt = [], []
        for l in range(self.num_layers):
            g_t, b_t = fp.layer_param(l, _lib.L_CA_TNORM_W, Lt).double(), fp.layer_param(l, _lib.L_CA_TNORM_B, Lt).double()
            Wkv = fp.layer_param(l, _lib.L_CA_KV_W, 2 * d * Lt).view(2 * d, Lt).double()
            bkv = fp.layer_param(l, _lib.L_CA_KV_B, 2 * d).double()
            wt.append((Wkv * g_t[None, :]).float())         # rows [0, d): key, [d, 2 d): value
            bt.append((bkv + Wkv @ b_t).float())
        Wt = torch.cat([w[:d] for w in wt] + [w[d:] for w in wt], 0).contiguous()
        Bt = torch.cat([b[:d] for b in bt] + [b[d:] for b in bt], 0).contiguous()
        return Wt, Bt, torch.ones(Lt, device=Wt.device), torch.zeros(Lt, device=Wt.device)

    def _derived16(self, fp):
        """Operands of the bf16-storage forward derived from the parameters, kept next to the bf16 shadow and rebuilt
        when the parameters change (`derived` of hig_denoiser_fwd_bf16, slots _lib.D16_*), NULL where a piece does not apply
        (the library then runs its LayerNorm kernel / pads per call):
        the LayerNorm-folded projections (d = 512 or 1024) -- self-attention q/k/v, cross-attention query, q/k/v of the
        person <-> person attention (two-person model; interaction_transformer.py:181-190) -- as W' (bf16), colsum, bias',
        computed in fp32; the stylization-out weights (d = 512) in matrix-core operand order (_frag16) for the fused kernels
        hig_attn_out16 / hig_rows_out16; the joint_embed weight (transformer.py:418) rounded to bf16 and padded to a multiple
        of 32 columns; and (linear attention) the batched text side of _text_kv_fold with its weights rounded to bf16."""
        ver = (self._param_version(), fp.flat.data_ptr())
        if getattr(self, "_derived", None) is None or self._derived[0] != ver:
            d, L, Lt = self.latent_dim, self.num_layers, self.text_latent_dim
            tab = _DerivedTable(_lib.D16_NLAYER, _lib.D16_NGLOBAL, L)
            with torch.no_grad():
                if not self.no_eff and Lt % 8 == 0:
                    Wt, Bt, ones, zeros = self._text_kv_fold(fp)
                    tab.set_global(_lib.D16_TEXT_KV_W, Wt.to(torch.bfloat16).contiguous())
                    tab.set_global(_lib.D16_TEXT_KV_B, Bt)
                    tab.set_global(_lib.D16_TEXT_ONES, ones)
                    tab.set_global(_lib.D16_TEXT_ZEROS, zeros)
                # (W' slot; LayerNorm weight, bias; Linear weight, bias; output rows): W', colsum, bias' at slot, slot + 1, + 2
                folds = ((_lib.D16_SA_QKV_W, _lib.L_SA_NORM_W, _lib.L_SA_NORM_B, _lib.L_SA_QKV_W, _lib.L_SA_QKV_B, 3 * d),
                         (_lib.D16_CA_Q_W, _lib.L_CA_NORM_W, _lib.L_CA_NORM_B, _lib.L_CA_Q_W, _lib.L_CA_Q_B, d),
                         (_lib.D16_INT_QKV_W, _lib.L_INT_NORM_W, _lib.L_INT_NORM_B, _lib.L_INT_QKV_W, _lib.L_INT_QKV_B, 3 * d))
                frags = ((_lib.D16_SA_STY_OUT_FRAG, _lib.L_SA_STY_OUT_W), (_lib.D16_CA_STY_OUT_FRAG, _lib.L_CA_STY_OUT_W),
                         (_lib.D16_INT_STY_OUT_FRAG, _lib.L_INT_STY_OUT_W), (_lib.D16_FFN_STY_OUT_FRAG, _lib.L_FFN_STY_OUT_W))
                for l in range(L if d in (512, 1024) else 0):
                    for slot, nw, nb, wi, bi, rows in folds:
                        gamma = fp.layer_param(l, nw, d)
                        if gamma is None:           # (the interaction block exists in the two-person model only)
                            continue
                        beta, b = fp.layer_param(l, nb, d), fp.layer_param(l, bi, rows)
                        W = fp.layer_param(l, wi, rows * d).view(rows, d)
                        Wp = (W * gamma[None, :]).to(torch.bfloat16).contiguous()
                        tab.set_layer(l, slot, Wp)
                        tab.set_layer(l, slot + 1, Wp.float().sum(dim=1).contiguous())
                        tab.set_layer(l, slot + 2, (b + W @ beta).contiguous())
                    for slot, wi in frags:
                        w = fp.layer_param(l, wi, d * d) if d == 512 else None
                        if w is not None:
                            tab.set_layer(l, slot, self._frag16(w.view(d, d).to(torch.bfloat16)))
                F = self.input_feats
                Fp = (F + 31) // 32 * 32
                wj = torch.zeros(d, Fp, device=fp.flat.device, dtype=torch.bfloat16)
                wj[:, :F] = self.joint_embed.weight.detach().to(torch.bfloat16)
                tab.set_global(_lib.D16_JOINT_W, wj)
            self._derived = (ver, tab)
        return self._derived[1].ptrs

    def _derived32(self, fp):
        """Operands of the fp32 inference forward derived from the parameters, rebuilt when they change (`derived32` of
        hig_denoiser_fwd_x, slots _lib.D32_*): per layer the LayerNorm-folded self-attention q/k/v and cross-attention query
        projections as W', colsum, bias', and (linear attention) the batched text side of _text_kv_fold.  fp64 arithmetic for
        the derived vectors, fp32 storage; latent_dim % 128 == 0 only (NULL table otherwise)."""
        d = self.latent_dim
        if d % 128 != 0 or d > 1024:
            return None
        ver = (self._param_version(), fp.flat.data_ptr())
        if getattr(self, "_derived_f32", None) is None or self._derived_f32[0] != ver:
            L = self.num_layers
            tab = _DerivedTable(_lib.D32_NLAYER, _lib.D32_NGLOBAL, L)
            # (W' slot; LayerNorm weight, bias; Linear weight, bias; output rows): W', colsum, bias' at slot, slot + 1, + 2
            folds = ((_lib.D32_SA_QKV_W, _lib.L_SA_NORM_W, _lib.L_SA_NORM_B, _lib.L_SA_QKV_W, _lib.L_SA_QKV_B, 3 * d),
                     (_lib.D32_CA_Q_W, _lib.L_CA_NORM_W, _lib.L_CA_NORM_B, _lib.L_CA_Q_W, _lib.L_CA_Q_B, d))
            with torch.no_grad():
                for l in range(L):
                    for slot, nw, nb, wi, bi, rows in folds:
                        gamma, beta = fp.layer_param(l, nw, d).double(), fp.layer_param(l, nb, d).double()
                        W, b = fp.layer_param(l, wi, rows * d).view(rows, d).double(), fp.layer_param(l, bi, rows).double()
                        Wp = (W * gamma[None, :]).float().contiguous()
                        tab.set_layer(l, slot, Wp)
                        tab.set_layer(l, slot + 1, Wp.double().sum(dim=1).float().contiguous())
                        tab.set_layer(l, slot + 2, (b + W @ beta).float().contiguous())
                if not self.no_eff:
                    for slot, t in zip((_lib.D32_TEXT_KV_W, _lib.D32_TEXT_KV_B, _lib.D32_TEXT_ONES, _lib.D32_TEXT_ZEROS),
                                       self._text_kv_fold(fp)):
                        tab.set_global(slot, t)
            self._derived_f32 = (ver, tab)
        return self._derived_f32[1].ptrs

    def _launch_forward(self, x, t, length, xf_proj, xf_out, training):
        B, T, N = x.shape[0], x.shape[1], xf_out.shape[1]
        assert xf_out.shape == (B, N, self.text_latent_dim) and xf_proj.shape == (B, self.time_embed_dim)
        api = _lib.api
        fp = self.flat_params()
        dims = self.dims(B, T, N)
        if training:
            self._check_bf16_training()
        nbytes = api.hig_workspace_bytes(dims, training)
        out = torch.empty(B, T, self.input_feats, device=x.device, dtype=torch.float32)
        bf16 = self._bf16()
        # per call: the reference's forward (text side recomputed every call, transformer.py:144-150) as ONE library call, which
        # is handed xf_out and builds the text side itself, on a side stream next to the first layers (hig_denoiser_fwd_text;
        # bf16 storage: embedding chain and text side next to the frame-row launches)
        per_call = not training and not self.cache_text_context
        if per_call:
            textctx = self._pool.take("textctx_i", api.hig_textctx_bytes(dims, 0), x.device)
        else:
            textctx = self._text_context(dims, xf_out, training)
        ws = self._pool.take("fwd_t" if training else "fwd_i", nbytes, x.device)
        if training:
            if bf16:
                api.hig_denoiser_fwd_bf16_train(dims, fp.param_table(), fp.shadow16(self._param_version()), x, t, length, xf_proj,
                                                textctx, out, ws)
            else:
                api.hig_denoiser_fwd(dims, fp.param_table(), x, t, length, xf_proj, textctx, out, ws, 1)
            return out, (dims, ws, textctx)
        # inference: the LayerNorm-folded projections (derived per parameter version)
        text = xf_out if per_call else None
        if bf16:
            api.hig_denoiser_fwd_bf16_x(dims, fp.param_table(), fp.shadow16(self._param_version()), self._derived16(fp), x, t, length,
                                        xf_proj, text, textctx, out, ws)
        else:
            api.hig_denoiser_fwd_x(dims, fp.param_table(), self._derived32(fp), x, t, length, xf_proj, text, textctx, out, ws, 0)
        self._pool.give("fwd_i", ws, x.device)
        if per_call:
            self._pool.give("textctx_i", textctx, x.device)
        return out, None

    def _launch_backward(self, x, t, length, xf_out, saved, dout, want_dx=False, layer_hook=None, comm_stream=None):
        """layer_hook(l): called on the host once decoder layer l's backward is enqueued and `comm_stream` (a
        torch.cuda.Stream) has been made to wait for it -- the data-parallel exchange of layer l's gradients can start
        there while the earlier layers are still in backward (hig_denoiser_bwd_hooked)."""
        dims, ws, textctx = saved
        api = _lib.api
        fp = self.flat_params()
        gtable = fp.ensure_grad()
        B, T, N = dims.B, dims.T, dims.N
        dev = x.device
        bws = self._pool.take("bwd", api.hig_bwd_workspace_bytes(dims), dev)
        dx = torch.empty_like(x) if want_dx else None
        dxp = torch.empty(B, self.time_embed_dim, device=dev, dtype=torch.float32)
        dxo = torch.empty(B, N, self.text_latent_dim, device=dev, dtype=torch.float32)
        bf16 = dims.storage == _lib.STORE_BF16
        # the four entries take the same arguments; bf16 storage adds the weight shadow, a hooked one the hook behind the stream
        args = [dims, fp.param_table()] + ([fp.shadow16(self._param_version())] if bf16 else []) + \
               [x, t, length, xf_out, textctx, ws, dout, gtable, dx, dxp, dxo, bws, torch.cuda.current_stream()]
        if layer_hook is None:      # (the hooked entries refuse a null hook)
            (api.hig_denoiser_bwd_bf16 if bf16 else api.hig_denoiser_bwd)(*args)
        else:
            errors = []

            def _hook(_user, layer):          # an exception must not unwind through the C frames
                try:
                    layer_hook(int(layer))
                except BaseException as e:  # noqa: BLE001
                    errors.append(e)

            cb = _lib.LAYER_HOOK(_hook)
            (api.hig_denoiser_bwd_bf16_hooked if bf16 else api.hig_denoiser_bwd_hooked)(*args, cb, None, comm_stream)
            if errors:
                raise errors[0]
        self._pool.give("bwd", bws, dev)
        self._pool.give("fwd_t", ws, dev)
        self._pool.give("textctx_t", textctx, dev)
        return dx, dxp, dxo


    # ---- text head (hig_text_head_*) -------------------------------------------------------
    def _has_hip_text_head(self):
        """True when this model owns a text head the HIP kernels cover (not cap_id, head dim in 8..128)."""
        if getattr(self, "text_head", "hip") != "hip" or not hasattr(self, "textTransEncoder"):
            return False
        l0 = self.textTransEncoder.layers[0]
        return self.text_latent_dim // l0.self_attn.num_heads in (8, 16, 32, 64, 128)

    def _has_hip_class_head(self):
        """True for a cap_id model whose class head runs through hig_class_head_fwd / _bwd (MotionInteractionTransformer,
        class_head="hip"); this model has no class head."""
        return False

    def _text_params(self):
        """Text-head parameters in hig.h table order (HIG_T_*, then HIG_TL_* per layer)."""
        pre = self.text_pre_proj
        glob = [getattr(pre, "weight", None), getattr(pre, "bias", None), self.text_ln.weight, self.text_ln.bias,
                self.text_proj[0].weight, self.text_proj[0].bias]
        lay = []
        for l in self.textTransEncoder.layers:
            lay += [l.self_attn.in_proj_weight, l.self_attn.in_proj_bias, l.self_attn.out_proj.weight,
                    l.self_attn.out_proj.bias, l.norm1.weight, l.norm1.bias, l.linear1.weight, l.linear1.bias,
                    l.linear2.weight, l.linear2.bias, l.norm2.weight, l.norm2.bias]
        assert len(glob) == _lib.T_NGLOBAL and len(lay) == _lib.T_NLAYER * len(self.textTransEncoder.layers)
        self._text_slots = [p is not None for p in glob + lay]
        return [p for p in glob + lay if p is not None]

    def _text_dims(self, B, N, W):
        l0 = self.textTransEncoder.layers[0]
        return _lib.TextDims(B=B, N=N, W=W, Lt=self.text_latent_dim, H=l0.self_attn.num_heads,
                             ff=l0.linear1.out_features, L=len(self.textTransEncoder.layers), E=self.time_embed_dim,
                             prec={"f32": _lib.PREC_F32, "bf16x3": _lib.PREC_BF16X3, "bf16": _lib.PREC_BF16}[self.precision])

    def _text_table(self, tensors):
        """c_void_p table with NULL in the slots of an Identity text_pre_proj."""
        arr = (C.c_void_p * len(self._text_slots))()
        it = iter(tensors)
        for i, present in enumerate(self._text_slots):
            arr[i] = next(it).data_ptr() if present else None
        return arr

    def _launch_text_head(self, clip_out, eot, training):
        B, N, W = clip_out.shape
        tp = self._text_params()
        for p in tp:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError("text head: parameters must be contiguous fp32 ROCm tensors")
        dims = self._text_dims(B, N, W)
        nbytes = _lib.api.hig_text_head_workspace_bytes(dims, training)
        dev = clip_out.device
        ws = self._pool.take("txt_t" if training else "txt_i", nbytes, dev)
        xf_out = torch.empty(B, N, self.text_latent_dim, device=dev, dtype=torch.float32)
        xf_proj = torch.empty(B, self.time_embed_dim, device=dev, dtype=torch.float32)
        _lib.api.hig_text_head_fwd(dims, self._text_table(tp), clip_out, eot, xf_out, xf_proj, ws, training)
        if not training:
            self._pool.give("txt_i", ws, dev)
            return xf_proj, xf_out, None
        return xf_proj, xf_out, (dims, ws)

    def _launch_text_head_backward(self, clip_out, eot, xf_out, saved, dxf_out, dxf_proj, want_dclip,
                                   into_flat=False):
        """into_flat: write the parameter gradients into the flat gradient buffer (fused training step)
        instead of a fresh scratch buffer (autograd path)."""
        dims, ws = saved
        tp = self._text_params()
        dev = clip_out.device
        if into_flat:
            fp = self.flat_params()
            assert len(fp.text_params) == len(tp), "text head is not part of the flat parameter buffer"
            grads, gtable = None, fp.text_grad_table(self._text_slots)
        else:
            offs, o = [], 0
            for p in tp:
                offs.append(o)
                o += (p.numel() + 63) // 64 * 64
            gflat = torch.empty(o, device=dev, dtype=torch.float32)
            grads = [gflat[off:off + p.numel()].view(p.shape) for p, off in zip(tp, offs)]
            gtable = self._text_table(grads)
        dclip = torch.empty_like(clip_out) if want_dclip else None
        bws = self._pool.take("txt_bwd", _lib.api.hig_text_head_bwd_workspace_bytes(dims), dev)
        _lib.api.hig_text_head_bwd(dims, self._text_table(tp), clip_out, eot, xf_out, ws,
                                   None if dxf_out is None else dxf_out.contiguous(),
                                   None if dxf_proj is None else dxf_proj.contiguous(), gtable, dclip, bws)
        self._pool.give("txt_bwd", bws, dev)
        self._pool.give("txt_t", ws, dev)
        return grads, dclip
