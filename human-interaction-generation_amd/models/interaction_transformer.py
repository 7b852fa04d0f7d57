"""MI355X-native `MotionInteractionTransformer`: the two-person denoiser of the reference
(codes/models/interaction_transformer.py:396-616), same constructor, attributes, state-dict keys
and call signature, running through the same C ABI as the single-person model with
`hig_dims.two_person` set (include/hig.h).

Batch convention (reference :577-583): x = cat([person 1 of every pair, person 2 of every pair]);
token 0 of each sample is the init-pose row (4 features through `joint_embed2`, read back through
`out2`), tokens 1.. are motion frames.  Each decoder layer adds a person<->person linear cross
attention (`int_ca_block`, :167-207) between the text cross-attention and the FFN.

Only the linear-attention variant is built (`no_eff=True` raises: the reference's `no_eff` layer for
this model, :369-394, drops the interaction attention altogether and no reference tool selects it).
"""
import ctypes as C
import os

import torch
from torch import nn

from .. import _lib
from . import clip_text
from .transformer import (FFN, MotionTransformer, StylizationBlock, _CrossAttention, _SelfAttention,
                          _WorkspacePool, clip, set_requires_grad, timestep_embedding, zero_module)

__all__ = ["MotionInteractionTransformer", "timestep_embedding", "zero_module", "set_requires_grad"]


class _InteractionCrossAttention(nn.Module):
    """Parameters of LinearTemporalInteractionCrossAttention (:167-179): one LayerNorm shared by both
    persons, query / key / value (d, d), stylization projection."""

    def __init__(self, latent_dim, num_head, dropout, time_embed_dim):
        super().__init__()
        self.num_head = num_head
        self.norm = nn.LayerNorm(latent_dim)
        self.query = nn.Linear(latent_dim, latent_dim)
        self.key = nn.Linear(latent_dim, latent_dim)
        self.value = nn.Linear(latent_dim, latent_dim)
        self.dropout = nn.Dropout(dropout)
        self.proj_out = StylizationBlock(latent_dim, time_embed_dim, dropout)


class _InteractionDecoderLayer(nn.Module):
    """:334-367: sa_block -> ca_block -> [int_ca_block] -> ffn (submodule order = state-dict order)."""

    def __init__(self, latent_dim, text_latent_dim, time_embed_dim, ffn_dim, num_head, dropout, no_cross_attn):
        super().__init__()
        self.no_cross_attn = no_cross_attn
        self.sa_block = _SelfAttention(latent_dim, num_head, dropout, time_embed_dim)
        self.ca_block = _CrossAttention(latent_dim, text_latent_dim, num_head, dropout, time_embed_dim)
        if not no_cross_attn:
            self.int_ca_block = _InteractionCrossAttention(latent_dim, num_head, dropout, time_embed_dim)
        self.ffn = FFN(latent_dim, ffn_dim, dropout, time_embed_dim)


class MotionInteractionTransformer(MotionTransformer):
    """Drop-in for the reference class (interaction_transformer.py:396-616)."""

    def __init__(self, input_feats, num_frames=240, latent_dim=512, ff_size=1024, num_layers=8,
                 num_heads=8, dropout=0, activation="gelu", num_text_layers=4, text_latent_dim=256,
                 text_ff_size=2048, text_num_heads=4, no_clip=False, no_eff=False, no_cross_attn=False,
                 cap_id=False, **kargs):
        nn.Module.__init__(self)
        if dropout != 0:
            raise NotImplementedError("dropout != 0 is not supported by the fused denoiser")
        if no_eff:
            raise NotImplementedError("MotionInteractionTransformer: only the linear-attention layers are built")
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
        self.cap_id = cap_id
        self.no_eff = False
        self.no_cross_attn = no_cross_attn

        # Text side: CLIP / class embeddings + the parameter containers of the text head (:421-462)
        if self.cap_id:
            self.cap_embedding = nn.Parameter(torch.randn(43, text_latent_dim))
            self.text_proj = nn.Sequential(nn.Linear(text_latent_dim, self.time_embed_dim))
        else:
            self.clip = kargs["clip_model"] if kargs.get("clip_model") is not None else clip.load('ViT-B/32', "cpu")[0]
            self.no_clip = no_clip
            if no_clip:
                self.clip.d_type = self.clip.token_embedding.weight.dtype
                self.clip.initialize_parameters()
                for name in ("visual", "logit_scale", "text_projection"):
                    if hasattr(self.clip, name):
                        delattr(self.clip, name)
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

        # Denoiser core (parameters only; :464-509)
        self.sequence_embedding = nn.Parameter(torch.randn(num_frames, latent_dim))
        self.two_embed = True
        self.joint_embed = nn.Linear(self.input_feats, self.latent_dim)
        self.joint_embed2 = nn.Linear(4, self.latent_dim)
        self.time_embed = nn.Sequential(
            nn.Linear(self.latent_dim, self.time_embed_dim),
            nn.SiLU(),
            nn.Linear(self.time_embed_dim, self.time_embed_dim),
        )
        self.temporal_decoder_blocks = nn.ModuleList(
            _InteractionDecoderLayer(latent_dim, text_latent_dim, self.time_embed_dim, ff_size, num_heads,
                                     dropout, no_cross_attn)
            for _ in range(num_layers))
        self.out = zero_module(nn.Linear(self.latent_dim, self.input_feats))
        self.out2 = zero_module(nn.Linear(self.latent_dim, self.input_feats))

        self.precision = kargs.get("precision", os.environ.get("HIG_PREC", "f32"))
        self.text_head = kargs.get("text_head", os.environ.get("HIG_TEXT_HEAD", "hip"))
        self.storage = kargs.get("storage", os.environ.get("HIG_STORAGE", "f32"))   # "bf16": inference with bf16 activations
        self._init_clip_route(kargs)
        # `clip_tower_train` (with `no_clip`): "hip" runs a qualifying TRAINABLE tower through hig_clip_text_fwd_train /
        # hig_clip_text_bwd (clip_text.tower_refusal(trainable=True) is the rule), "torch" (the default) keeps it on torch ops.
        # "flat" does what "hip" does and also places the tower's parameters behind the text head in the flat parameter buffer
        # (transformer._FlatParams), so that the fused / captured training step trains them (`token_batch=` of the trainer's
        # steps); it needs a `no_clip` model and a tower the rule accepts, and raises otherwise.
        self.clip_tower_train = kargs.get("clip_tower_train", os.environ.get("HIG_CLIP_TOWER_TRAIN", "torch"))
        if self.clip_tower_train not in ("hip", "torch", "flat"):
            raise ValueError("clip_tower_train must be 'hip', 'torch' or 'flat' (got %r)" % (self.clip_tower_train,))
        if self.clip_tower_train == "flat" and (self.cap_id or not getattr(self, "no_clip", False)):
            raise ValueError("clip_tower_train='flat' needs a model that trains its CLIP text tower (no_clip=True, not cap_id): this "
                             "one's tower is %s" % ("absent (cap_id)" if self.cap_id else "frozen"))
        self._clip_train_table = None
        self.clip_train_stats = {"native_forwards": 0, "native_backwards": 0, "native_inference": 0}
        # `class_head` (with `cap_id`): "hip" puts cap_embedding and text_proj into the flat buffer behind the core and lets the
        # fused / captured training step run them through hig_class_head_fwd / _bwd (`class_ids=` of the trainer's steps);
        # "torch" (the default) keeps them outside it, on torch ops and torch.optim.Adam.  Without `cap_id` it has no effect.
        self.class_head = kargs.get("class_head", os.environ.get("HIG_CLASS_HEAD", "torch"))
        if self.class_head not in ("hip", "torch"):
            raise ValueError("class_head must be 'hip' or 'torch' (got %r)" % (self.class_head,))
        self._flat = None
        self._pool = _WorkspacePool()
        self._textctx_cache = None
        self._param_epoch = 0
        self.cache_text_context = True

    def _apply(self, fn, *a, **k):
        self._clip_train_table = None
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):
        self._clip_train_table = None
        return super()._load_from_state_dict(*a, **k)

    def _clip_train_native_table(self, tokens):
        """The pointer table of the trainable tower when `encode_text` takes the native route for these tokens, else None: the
        model is `no_clip`, the option is "hip", the tokens are on a ROCm device and clip_text.tower_refusal(trainable=True)
        finds nothing (asked once; a tower that did not qualify is asked again only after `_apply` or a load)."""
        if self.clip_tower_train not in ("hip", "flat") or not tokens.is_cuda or not getattr(self, "no_clip", False):
            return None
        if not hasattr(getattr(self.clip, "transformer", None), "resblocks"):
            return None
        if self.clip_tower_train == "flat":
            self.flat_params()      # (re-homes the tower first: the table below holds the flat buffer's pointers)
        t = self._clip_train_table
        if isinstance(t, clip_text.TrainTowerTable) and (t.device != tokens.device or t.stale()):
            t = None
        if t is None:
            try:
                t = clip_text.TrainTowerTable(self.clip, tokens.device)
            except clip_text.TowerRefused:
                t = False
            self._clip_train_table = t
        return t or None

    # ---- reference API ------------------------------------------------------------------
    def load_my_state_dict(self, state_dict, opt):
        """Partial checkpoint loading (:511-530): language-only / motion-only / whatever matches."""
        own_state = self.state_dict()
        for name, param in state_dict.items():
            is_text = 'clip' in name or 'text' in name
            if opt.only_language:
                if name not in own_state or not is_text:
                    print(name)
                    continue
            elif opt.only_motion:
                if name not in own_state or is_text:
                    print(name)
                    continue
            else:
                if name not in own_state:
                    if not (opt.cap_id and is_text):
                        print(name)
                    continue
            if isinstance(param, torch.nn.parameter.Parameter):
                param = param.data
            own_state[name].copy_(param)
        self.params_changed()

    def encode_text(self, text, device):
        """:532-556; with `no_clip` the CLIP text tower is trained too (no no_grad)."""
        if not self.no_clip:
            return MotionTransformer.encode_text(self, text, device)
        tokens_host = self._tokenize(text)
        text = tokens_host.to(device)
        table = self._clip_train_native_table(text)
        if table is not None:   # the trainable tower in HIP (csrc/cliptext.hip); exact-fp32 products
            ids = text.long()   # (the `clip` package's tokenizer hands out int32 in some versions; the entries take int64)
            if torch.is_grad_enabled() and any(p.requires_grad for p in table.tensors):
                index = clip_text.EmbedIndex(tokens_host, table.vocab).to(text.device)
                x = clip_text._ClipTowerFn.apply(self, table, ids, index, *table.tensors)
            else:
                x = clip_text.tower_forward(table, ids, self._pool)
                self.clip_train_stats["native_inference"] += 1
            return self._text_head(text, x.permute(1, 0, 2))
        # clip_tower_train="torch", or a tower the rule refuses: stock torch ops
        x = self.clip.token_embedding(text).type(self.clip.d_type)
        x = x + self.clip.positional_embedding.type(self.clip.d_type)
        x = x.permute(1, 0, 2)
        x = self.clip.transformer(x)
        x = self.clip.ln_final(x).type(self.clip.d_type)
        return self._text_head(text, x)

    def flat_tower_table(self):
        """The TrainTowerTable of a tower that lives in the flat parameter buffer (clip_tower_train="flat"), its pointers the
        buffer's: what the fused / captured step's Tokens source runs the tower through.  No fallback: raises when the model has
        no such tower."""
        fp = self.flat_params()
        if not fp.tower_params:
            raise RuntimeError("token_batch= needs a no_clip model built with clip_tower_train='flat' (or HIG_CLIP_TOWER_TRAIN=flat): "
                               "this model's CLIP text tower is not in the flat parameter buffer")
        t = self._clip_train_table
        if not isinstance(t, clip_text.TrainTowerTable) or t.device != fp.flat.device or t.stale():
            t = self._clip_train_table = clip_text.TrainTowerTable(self.clip, fp.flat.device)
        assert all(a is b for a, b in zip(t.tensors, fp.tower_params))
        return t

    def get_class_embedding(self, text):
        """:558-563: caption ids -> learned class embeddings (cap_id models)."""
        text = torch.cat(text)
        xf_proj = self.cap_embedding[text]
        xf_out = xf_proj.unsqueeze(1)
        xf_proj = self.text_proj(xf_proj)
        return xf_proj, xf_out

    # ---- class head in HIP (hig_class_head_*; class_head="hip") ---------------------------------------------
    def _has_hip_class_head(self):
        return bool(self.cap_id) and self.class_head == "hip"

    def _class_params(self):
        """The class head's parameters in the order they take in the flat buffer behind the core."""
        return [self.cap_embedding, self.text_proj[0].weight, self.text_proj[0].bias]

    def _class_head_args(self, ids):
        if not self._has_hip_class_head():
            raise RuntimeError("class_ids= needs a cap_id model built with class_head='hip' (or HIG_CLASS_HEAD=hip): this model's "
                               "class head is on torch ops, outside the flat buffer")
        if not (ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 1 and ids.is_contiguous()):
            raise ValueError("class_ids must be a contiguous 1-d int32 ROCm tensor, one id per model-batch row")
        tp = self._class_params()
        if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in tp):
            raise RuntimeError("class head: parameters must be contiguous fp32 ROCm tensors")
        classes, Lt = self.cap_embedding.shape
        return tp, int(classes), int(Lt), int(self.time_embed_dim), int(ids.numel())

    def _launch_class_head(self, ids):
        """ids (rows,) int32 -> xf_proj (rows, E), xf_out (rows, 1, Lt): text_proj once per class, rows fetched by id."""
        tp, classes, Lt, E, rows = self._class_head_args(ids)
        dev = ids.device
        ws = self._pool.take("cls_f", _lib.api.hig_class_head_workspace_bytes(classes, Lt, E, 0), dev)
        xf_out = torch.empty(rows, 1, Lt, device=dev, dtype=torch.float32)
        xf_proj = torch.empty(rows, E, device=dev, dtype=torch.float32)
        _lib.api.hig_class_head_fwd(classes, Lt, E, rows, tp[0], tp[1], tp[2], ids, xf_out, xf_proj, ws)
        self._pool.give("cls_f", ws, dev)
        return xf_proj, xf_out

    def _launch_class_head_backward(self, ids, dxf_out, dxf_proj):
        """Writes the gradients of cap_embedding, text_proj.0.weight and text_proj.0.bias into the flat gradient buffer."""
        tp, classes, Lt, E, rows = self._class_head_args(ids)
        dev = ids.device
        fp = self.flat_params()
        fp.ensure_grad()
        assert len(fp.text_params) == 3 and all(a is b for a, b in zip(fp.text_params, tp)), \
            "the class head is not part of the flat parameter buffer"
        g_emb, g_w, g_b = (C.c_void_p(fp.grad.data_ptr() + 4 * o) for o in fp.text_offsets)
        ws = self._pool.take("cls_b", _lib.api.hig_class_head_workspace_bytes(classes, Lt, E, 1), dev)
        _lib.api.hig_class_head_bwd(classes, Lt, E, rows, tp[0], tp[1], ids, None if dxf_out is None else dxf_out.contiguous(),
                                    None if dxf_proj is None else dxf_proj.contiguous(), g_emb, g_w, g_b, ws)
        self._pool.give("cls_b", ws, dev)

    def dims(self, B, T, N):
        d = MotionTransformer.dims(self, B, T, N)
        d.two_person = 2 if self.no_cross_attn else 1
        return d

    def forward(self, x, timesteps, length=None, text=None, xf_proj=None, xf_out=None):
        """x: (2B, T, F) = cat([x1, x2]) -> (2B, T, F)   (:577-616)."""
        B2, T = x.shape[0], x.shape[1]
        if self.cap_id:
            xf_proj, xf_out = self.get_class_embedding(text)
        elif xf_proj is None or xf_out is None:
            xf_proj, xf_out = self.encode_text(text, x.device)
        if not x.is_cuda:
            raise RuntimeError("MotionInteractionTransformer.forward: ROCm device tensors required "
                               "(no CPU fallback; the CPU restatement lives in oracle/ for tests only)")
        assert B2 % 2 == 0 and x.shape[2] == self.input_feats and T - 1 <= self.num_frames
        return self._run(x, timesteps, length, xf_proj, xf_out)
