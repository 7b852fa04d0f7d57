"""The text tower of OpenAI CLIP (clip/model.py: `Transformer` of `ResidualAttentionBlock`s under `CLIP.encode_text`) as a
stand-alone module, and its native route.

`MotionTransformer._clip_features` runs the frozen tower in front of the text head (transformer.py:381-388).  The `clip`
package brings the tower as stock torch ops; this module has

  * `ClipTextTransformer` / `ClipTextModel`: the same structure and state-dict names on stock torch ops, so OpenAI's weights
    load without the package.  This forward is the YARDSTICK of the native route, never its fallback;
  * `load_text_tower`: a state dict, a checkpoint of this project (`clip.` keys) or a file -> `ClipTextModel`;
  * `tower_refusal` / `TowerTable` / `tower_forward`: the rule that says whether hig_clip_text_fwd (csrc/cliptext.hip) can run
    a given tower, its pointer table, and the call;
  * `TrainTowerTable` / `EmbedIndex` / `tower_forward_train` / `tower_backward` / `_ClipTowerFn`: the same for a TRAINABLE tower
    (`MotionInteractionTransformer(no_clip=True, clip_tower_train="hip")`) through hig_clip_text_fwd_train / hig_clip_text_bwd,
    with the embedding gradient's inverted index built on the host from the tokenizer's CPU tokens;
  * `TokenBatch` / `DeviceEmbedIndex` / `tower_backward_dev`: the tower inside the fused / captured training step
    (`clip_tower_train="flat"`, trainers/text_source.py: Tokens): the distinct captions' tokens with their row maps as one
    packed upload, the index built on the device by hig_clip_embed_index_build, and hig_clip_text_bwd_dev writing the
    gradients into the flat gradient buffer.

The BPE vocabulary is data this repository does not carry: without the `clip` package the caller supplies the tokenizer
(`MotionTransformer(clip_model=..., clip_tokenize=...)`).
"""
import ctypes as C
import math
import os
import re
from collections import OrderedDict

import torch
from torch import nn

HEAD_DIM = 64          # what hig_causal_attn_fwd is built for
MAX_TOKENS = 128


class QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


def causal_mask(context_length):
    """CLIP.build_attention_mask: additive, -inf above the diagonal."""
    return torch.full((context_length, context_length), float("-inf")).triu_(1)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model, n_head, attn_mask=None):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = nn.LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, d_model * 4)), ("gelu", QuickGELU()),
                                              ("c_proj", nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = nn.LayerNorm(d_model)
        self.attn_mask = attn_mask        # a plain attribute, as in OpenAI's class: not part of the state dict

    def attention(self, x):
        mask = self.attn_mask
        if mask is not None:
            self.attn_mask = mask = mask.to(dtype=x.dtype, device=x.device)
        return self.attn(x, x, x, need_weights=False, attn_mask=mask)[0]

    def forward(self, x):
        x = x + self.attention(self.ln_1(x))
        return x + self.mlp(self.ln_2(x))


class ClipTextTransformer(nn.Module):
    """Sequence-first (N, B, W) -> (N, B, W) on stock torch ops; every block carries the causal mask."""

    def __init__(self, width=512, layers=12, heads=8, context_length=77):
        super().__init__()
        self.width, self.layers, self.heads, self.context_length = width, layers, heads, context_length
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads, causal_mask(context_length)) for _ in range(layers)])

    def forward(self, x):
        return self.resblocks(x)


class ClipTextModel(nn.Module):
    """The attributes `_clip_features` and the stub touch: token_embedding, positional_embedding, transformer, ln_final,
    text_projection, logit_scale, dtype, initialize_parameters."""

    def __init__(self, width=512, layers=12, heads=8, context_length=77, vocab_size=49408, embed_dim=512):
        super().__init__()
        self.context_length, self.vocab_size = context_length, vocab_size
        self.transformer = ClipTextTransformer(width, layers, heads, context_length)
        self.token_embedding = nn.Embedding(vocab_size, width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, width))
        self.ln_final = nn.LayerNorm(width)
        self.text_projection = nn.Parameter(torch.empty(width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        self.initialize_parameters()

    @property
    def dtype(self):
        return self.token_embedding.weight.dtype

    def initialize_parameters(self, generator=None):
        """CLIP.initialize_parameters' standard deviations (the text side)."""
        t = self.transformer
        n = lambda p, std: nn.init.normal_(p, std=std, generator=generator)   # noqa: E731
        n(self.token_embedding.weight, 0.02)
        n(self.positional_embedding, 0.01)
        proj_std = (t.width ** -0.5) * ((2 * t.layers) ** -0.5)
        attn_std = t.width ** -0.5
        fc_std = (2 * t.width) ** -0.5
        for block in t.resblocks:
            n(block.attn.in_proj_weight, attn_std)
            n(block.attn.out_proj.weight, proj_std)
            n(block.mlp.c_fc.weight, fc_std)
            n(block.mlp.c_proj.weight, proj_std)
        n(self.text_projection, t.width ** -0.5)

    def features(self, tokens):
        """tokens (B, N) -> ln_final's output, sequence-first (N, B, W): the lines of `_clip_features` on torch ops."""
        x = self.token_embedding(tokens).type(self.dtype) + self.positional_embedding.type(self.dtype)
        return self.ln_final(self.transformer(x.permute(1, 0, 2))).type(self.dtype)


_NOT_WEIGHTS = ("input_resolution", "context_length", "vocab_size")   # scalars OpenAI's TorchScript archive keeps as buffers


def load_text_tower(source):
    """A `ClipTextModel` (fp32, on the CPU) from
      * a state dict of CLIP (OpenAI's names; `visual.*` is dropped),
      * a state dict or checkpoint of this project, whose tower keys start with `clip.` (everything else is dropped),
      * a path that torch.jit.load (OpenAI's ViT-B-32.pt is a TorchScript archive) or torch.load opens.
    Width, layers and heads = width / 64 are read off the shapes."""
    if isinstance(source, (str, os.PathLike)):
        try:
            source = torch.jit.load(source, map_location="cpu").state_dict()
        except RuntimeError:
            source = torch.load(source, map_location="cpu", weights_only=False)
    if isinstance(source, nn.Module):
        source = source.state_dict()
    for wrap in ("state_dict", "encoder"):
        if isinstance(source, dict) and wrap in source and isinstance(source[wrap], dict):
            source = source[wrap]
    sd = {k: v for k, v in source.items() if torch.is_tensor(v)}
    if any(k.startswith("clip.") for k in sd):
        sd = {k[len("clip."):]: v for k, v in sd.items() if k.startswith("clip.")}
    sd = {k: v for k, v in sd.items() if not k.startswith("visual.") and k not in _NOT_WEIGHTS}
    if "ln_final.weight" not in sd or "positional_embedding" not in sd or "token_embedding.weight" not in sd:
        raise ValueError("load_text_tower: no CLIP text tower in these %d keys" % len(sd))
    width = sd["ln_final.weight"].shape[0]
    blocks = {int(m.group(1)) for m in (re.match(r"transformer\.resblocks\.(\d+)\.", k) for k in sd) if m}
    if not blocks or blocks != set(range(len(blocks))) or width % HEAD_DIM:
        raise ValueError("load_text_tower: blocks %s of width %d are not a CLIP text tower" % (sorted(blocks), width))
    embed_dim = sd["text_projection"].shape[1] if "text_projection" in sd else width
    model = ClipTextModel(width, len(blocks), width // HEAD_DIM, sd["positional_embedding"].shape[0],
                          sd["token_embedding.weight"].shape[0], embed_dim)
    missing, unexpected = model.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    if unexpected or set(missing) - {"text_projection", "logit_scale"}:
        raise ValueError("load_text_tower: missing %s, unexpected %s" % (missing, unexpected))
    return model


# ---- the native route ----------------------------------------------------------------------------------------------------------
def _tower_tensors(clip_model):
    """The tower's parameters in the order of include/hig.h: HIG_CT_*, then HIG_CTL_* per layer."""
    out = [clip_model.token_embedding.weight, clip_model.positional_embedding, clip_model.ln_final.weight, clip_model.ln_final.bias]
    for b in clip_model.transformer.resblocks:
        out += [b.ln_1.weight, b.ln_1.bias, b.attn.in_proj_weight, b.attn.in_proj_bias, b.attn.out_proj.weight, b.attn.out_proj.bias,
                b.ln_2.weight, b.ln_2.bias, b.mlp.c_fc.weight, b.mlp.c_fc.bias, b.mlp.c_proj.weight, b.mlp.c_proj.bias]
    return out


def tower_refusal(clip_model, device=None, trainable=False):
    """None when hig_clip_text_fwd computes what `clip_model`'s torch ops compute, else the reason it does not: the tower has
    `resblocks` of OpenAI's structure, every tower parameter is a frozen contiguous fp32 tensor (on `device`, when given),
    the head dim is 64, there are at most 128 tokens and every block's `attn_mask` is the causal one (compared on the host).
    trainable=True: the same rule for hig_clip_text_fwd_train / hig_clip_text_bwd, where parameters may require grad."""
    blocks = getattr(getattr(clip_model, "transformer", None), "resblocks", None)
    if blocks is None or len(blocks) == 0:
        return "the tower has no resblocks"
    try:
        tensors = _tower_tensors(clip_model)
    except AttributeError as e:
        return "a block is not a ResidualAttentionBlock (%s)" % e
    if any(t is None for t in tensors):
        return "a block lacks in_proj_weight or a bias"
    for t in tensors:
        if t.dtype != torch.float32:
            return "a tower parameter is %s, not fp32" % t.dtype
        if t.requires_grad and not trainable:
            return "a tower parameter requires grad (the backward is not built)"
        if not t.is_contiguous():
            return "a tower parameter is not contiguous"
        if device is not None and (not t.is_cuda or t.device != torch.device(device)):
            return "a tower parameter lives on %s, not on %s" % (t.device, device)
    N, W = clip_model.positional_embedding.shape
    if clip_model.token_embedding.weight.shape[1] != W or clip_model.ln_final.weight.shape[0] != W:
        return "widths disagree"
    if N > MAX_TOKENS:
        return "%d tokens (the causal attention covers %d)" % (N, MAX_TOKENS)
    want = None
    for b in blocks:
        a = b.attn
        if a.embed_dim != W or a.embed_dim // a.num_heads != HEAD_DIM:
            return "head dim %d, not %d" % (a.embed_dim // a.num_heads, HEAD_DIM)
        if getattr(a, "batch_first", False) or a.bias_k is not None or a.add_zero_attn or a.dropout != 0:
            return "an attention option the kernels do not cover"
        if b.mlp.c_fc.weight.shape != (4 * W, W) or b.mlp.c_proj.weight.shape != (W, 4 * W):
            return "an FFN that is not 4 W wide"
        if b.ln_1.eps != 1e-5 or b.ln_2.eps != 1e-5:
            return "a LayerNorm eps other than 1e-5"
        mask = getattr(b, "attn_mask", None)
        if mask is None or tuple(mask.shape) != (N, N):
            return "a block without an (N, N) attn_mask"
        if want is None:
            want = causal_mask(N)
        if mask.dtype == torch.bool or not torch.equal(mask.detach().float().cpu(), want):
            return "an attn_mask that is not the causal one"
    if clip_model.ln_final.eps != 1e-5:
        return "a LayerNorm eps other than 1e-5"
    return None


def clip_dims(B, N, W, H, L, vocab, prec=0):
    """The HIG_CD_* slots of hig_clip_text_fwd / hig_clip_text_workspace_bytes as a ctypes array."""
    from .. import _lib
    d = (C.c_int32 * _lib.CD_NSLOTS)()
    for slot, v in (("B", B), ("N", N), ("W", W), ("H", H), ("L", L), ("VOCAB", vocab), ("PREC", prec)):
        d[getattr(_lib, "CD_" + slot)] = v
    return d


class TowerRefused(ValueError):
    """tower_refusal's reason, raised by TowerTable."""


class TowerTable:
    """The pointer table of a qualifying tower, built once: the tensors (kept alive), their addresses in hig.h's order and
    the shape.  `stale()` says whether a parameter has been moved or un-frozen since."""
    TRAINABLE = False

    def __init__(self, clip_model, device):
        why = tower_refusal(clip_model, device, trainable=self.TRAINABLE)
        if why is not None:
            raise TowerRefused("CLIP text tower: " + why)
        from .. import _lib
        self.tensors = _tower_tensors(clip_model)
        blocks = clip_model.transformer.resblocks
        assert len(self.tensors) == _lib.CT_NGLOBAL + _lib.CTL_NLAYER * len(blocks)
        self.ptrs = tuple(t.data_ptr() for t in self.tensors)
        self.table = (C.c_void_p * len(self.ptrs))(*self.ptrs)
        self.N, self.W = clip_model.positional_embedding.shape
        self.H, self.L = blocks[0].attn.num_heads, len(blocks)
        self.vocab = clip_model.token_embedding.weight.shape[0]
        self.device = torch.device(device)

    def stale(self):
        return any(t.data_ptr() != p or (t.requires_grad and not self.TRAINABLE) for t, p in zip(self.tensors, self.ptrs))


_PREC = {"f32": 0, "bf16x3": 1, "bf16": 2}


def tower_forward(table, tokens, pool=None, precision="f32"):
    """tokens (B, N) int64 on the table's device -> ln_final's output (B, N, W), batch-first, through hig_clip_text_fwd on the
    current stream.  There is no fallback: a refusal of the library raises."""
    from .. import _lib
    if tokens.dim() != 2 or tokens.shape[1] != table.N or tokens.dtype != torch.int64 or tokens.device != table.device:
        raise RuntimeError("CLIP text tower: tokens must be (B, %d) int64 on %s" % (table.N, table.device))
    tokens = tokens.contiguous()
    B = tokens.shape[0]
    dims = clip_dims(B, table.N, table.W, table.H, table.L, table.vocab, _PREC[precision])
    nbytes = _lib.api.hig_clip_text_workspace_bytes(dims)
    ws = pool.take("clip", nbytes, table.device) if pool is not None else torch.empty(nbytes, dtype=torch.uint8, device=table.device)
    out = torch.empty(B, table.N, table.W, device=table.device, dtype=torch.float32)
    _lib.api.hig_clip_text_fwd(dims, table.table, tokens, out, ws)
    if pool is not None:
        pool.give("clip", ws, table.device)
    return out


# ---- the native training route -------------------------------------------------------------------------------------------------
class TrainTowerTable(TowerTable):
    """TowerTable under tower_refusal(trainable=True): parameters may require grad; stale when one has moved."""
    TRAINABLE = True


def embed_chunk():
    from .. import _lib
    return _lib.CLIP_EMBED_CHUNK


class EmbedIndex:
    """The inverted index hig_clip_embed_bwd takes (include/hig.h), built on the host from the tokenizer's CPU tokens (B, N):
    per distinct id in [0, vocab) the rows b N + n that hold it in ascending order, cut into chunks of `chunk` rows; all of it
    int32 in ONE packed buffer (`host`; `to(device)` uploads it from pinned memory).  Fields: order, chunk_seg, chunk_order,
    id_seg, ids, pos_order, pos_seg (numpy views of `host`), n_live, n_chunks, n_ids."""

    FIELDS = ("order", "chunk_seg", "chunk_order", "id_seg", "ids", "pos_order", "pos_seg")

    def __init__(self, tokens, vocab, chunk=None):
        import numpy as np
        chunk = embed_chunk() if chunk is None else int(chunk)
        tok = np.asarray(tokens.detach().cpu().numpy() if torch.is_tensor(tokens) else tokens, dtype=np.int64)
        assert tok.ndim == 2 and chunk > 0
        B, N = tok.shape
        flat = tok.reshape(-1)
        rows = np.nonzero((flat >= 0) & (flat < vocab))[0]
        rows = rows[np.argsort(flat[rows], kind="stable")]                 # grouped by id, ascending row inside an id
        ids, counts = np.unique(flat[rows], return_counts=True)
        per_id = (counts + chunk - 1) // chunk                              # chunks of every id
        starts = np.concatenate([[0], np.cumsum(counts)])[:-1]
        chunk_seg = [np.arange(s, s + c, chunk) for s, c in zip(starts, counts)]
        chunk_seg = np.concatenate(chunk_seg + [np.array([len(rows)])]) if len(ids) else np.zeros(1, np.int64)
        self.B, self.N, self.vocab, self.chunk = B, N, int(vocab), chunk
        self.n_live, self.n_chunks, self.n_ids = len(rows), len(chunk_seg) - 1, len(ids)
        parts = [rows, chunk_seg, np.arange(self.n_chunks), np.concatenate([[0], np.cumsum(per_id)]), ids,
                 (np.arange(B)[None, :] * N + np.arange(N)[:, None]).reshape(-1), np.arange(N + 1) * B]
        packed = np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])
        assert B * N < 2 ** 31 and packed.size == self.numel()
        self.host = torch.from_numpy(packed.astype(np.int32))
        view, o = self.host.numpy(), 0
        for name, p in zip(self.FIELDS, parts):
            setattr(self, name, view[o:o + len(p)])
            o += len(p)
        self.dev = None

    def numel(self):
        return (self.n_live + (self.n_chunks + 1) + self.n_chunks + (self.n_ids + 1) + self.n_ids + self.B * self.N + (self.N + 1))

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and not self.host.is_pinned():
            self.host = self.host.pin_memory()
        self.dev = self.host.to(device, non_blocking=True)
        return self


def embed_grad_restated(dx0, index, W):
    """The fp32 sum hig_clip_embed_bwd is defined as, in numpy: each chunk added in list order from its first row, then an id's
    chunk sums in chunk order from the first; dpos[n] over b ascending.  dx0 (B N, W) -> (dtok (vocab, W), dpos (N, W))."""
    import numpy as np
    dx0 = np.asarray(dx0, dtype=np.float32).reshape(index.B * index.N, W)
    dtok = np.zeros((index.vocab, W), dtype=np.float32)
    for u in range(index.n_ids):
        total = None
        for c in range(index.id_seg[u], index.id_seg[u + 1]):
            members = index.order[index.chunk_seg[c]:index.chunk_seg[c + 1]]
            part = dx0[members[0]].copy()
            for r in members[1:]:
                part = (part + dx0[r]).astype(np.float32)
            total = part if total is None else (total + part).astype(np.float32)
        dtok[index.ids[u]] = total
    dpos = np.zeros((index.N, W), dtype=np.float32)
    for n in range(index.N):
        acc = dx0[n].copy()
        for b in range(1, index.B):
            acc = (acc + dx0[b * index.N + n]).astype(np.float32)
        dpos[n] = acc
    return dtok, dpos


def _train_dims(table, B):
    return clip_dims(B, table.N, table.W, table.H, table.L, table.vocab, 0)


def _check_tokens(table, tokens):
    if tokens.dim() != 2 or tokens.shape[1] != table.N or tokens.dtype != torch.int64 or tokens.device != table.device:
        raise RuntimeError("CLIP text tower: tokens must be (B, %d) int64 on %s" % (table.N, table.device))


def tower_forward_train(table, tokens, pool=None):
    """hig_clip_text_fwd_train on the current stream: (out (B, N, W), saved).  `saved` goes to tower_backward, which returns its
    buffer to the pool."""
    from .. import _lib
    _check_tokens(table, tokens)
    tokens = tokens.contiguous()
    B = tokens.shape[0]
    dims = _train_dims(table, B)
    nbytes = _lib.api.hig_clip_text_train_bytes(dims)
    ws = pool.take("clip_t", nbytes, table.device) if pool is not None else torch.empty(nbytes, dtype=torch.uint8, device=table.device)
    out = torch.empty(B, table.N, table.W, device=table.device, dtype=torch.float32)
    _lib.api.hig_clip_text_fwd_train(dims, table.table, tokens, out, ws)
    return out, (dims, ws, B)


def tower_backward(table, index, dout, saved, pool=None):
    """hig_clip_text_bwd: upstream dout (B, N, W) -> the gradients of table.tensors, in that order, as views of one fresh buffer."""
    from .. import _lib
    dims, ws, B = saved
    dev = table.device
    if index.dev is None or index.dev.device != dev or (index.B, index.N, index.vocab) != (B, table.N, table.vocab):
        raise RuntimeError("CLIP text tower: the embedding index does not belong to these tokens")
    dout = dout.contiguous()
    assert dout.shape == (B, table.N, table.W) and dout.dtype == torch.float32
    offs, o = [], 0
    for p in table.tensors:
        offs.append(o)
        o += (p.numel() + 63) // 64 * 64
    gflat = torch.empty(o, device=dev, dtype=torch.float32)
    grads = [gflat[off:off + p.numel()].view(p.shape) for p, off in zip(table.tensors, offs)]
    gtable = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
    nb = _lib.api.hig_clip_text_bwd_workspace_bytes(dims)
    bws = pool.take("clip_bwd", nb, dev) if pool is not None else torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.api.hig_clip_text_bwd(dims, table.table, index.dev, index.n_live, index.n_chunks, index.n_ids, dout, ws, gtable, bws)
    if pool is not None:
        pool.give("clip_bwd", bws, dev)
        pool.give("clip_t", ws, dev)
    return grads


class _ClipTowerFn(torch.autograd.Function):
    """Autograd boundary of the trainable tower (hig_clip_text_fwd_train / hig_clip_text_bwd): tokens in, ln_final's output
    (B, N, W) out; the tower's parameters are passed so that autograd routes their gradients, which come back as ordinary
    tensors (views of one buffer per backward)."""

    @staticmethod
    def forward(ctx, owner, table, tokens, index, *params):
        out, saved = tower_forward_train(table, tokens, owner._pool)
        ctx.owner, ctx.table, ctx.index, ctx.saved = owner, table, index, saved
        owner.clip_train_stats["native_forwards"] += 1
        return out

    @staticmethod
    def backward(ctx, dout):
        grads = tower_backward(ctx.table, ctx.index, dout, ctx.saved, ctx.owner._pool)
        ctx.saved = None
        ctx.owner.clip_train_stats["native_backwards"] += 1
        return (None, None, None, None) + tuple(g if p.requires_grad else None for g, p in zip(grads, ctx.table.tensors))


# ---- the trainable tower inside the fused / captured step ------------------------------------------------------------------------
class TokenBatch:
    """The text input of a fused step that trains the tower (trainers/text_source.py: Tokens), built on the host: the tokens of
    the step's DISTINCT captions and the row maps that expand the text side's output to the model batch and sum its upstream
    gradients back -- `inv`, `order`, `seg` exactly as the caption bank's CaptionBatch builds them (distinct captions in order
    of first appearance, U rounded up by `padded_unique`).  Padding entries repeat the first distinct caption's tokens and have
    empty segments, so their upstream gradient is exactly zero.  dedup=False: the identity maps over all rows (U = U_pad = rows).
    Everything is int32 words of ONE packed buffer (`host`; `to(device)` uploads it from pinned memory):
        tokens (U_pad, N) int64 | eot (U_pad,) int64 | inv (rows,) | order (rows,) | seg (U_pad + 1,) | U
    whose layout depends on (rows, U_pad, N) alone: a captured step copies `dev` into its static twin.
    `cache`: a dict caption -> (token row, eot) kept by the caller, so that the tokenizer never runs on a caption twice."""

    def __init__(self, captions, tokenize, dedup=True, cache=None):
        from .caption_bank import padded_unique
        captions = list(captions)
        rows = len(captions)
        if rows == 0:
            raise ValueError("TokenBatch: no captions")
        if not all(isinstance(c, str) for c in captions):
            raise TypeError("TokenBatch: captions must be strings")
        cache = {} if cache is None else cache
        missing = [c for c in dict.fromkeys(captions) if c not in cache]
        self.tokenizer_rows = len(missing)
        if missing:
            tok = tokenize(missing).to("cpu", torch.int64)      # (the model's `_tokenize`: one call for all of them)
            for c, row in zip(missing, tok):
                cache[c] = (row.clone(), int(row.argmax()))
        if dedup:
            index, uniq, inv = {}, [], []
            for c in captions:
                u = index.get(c)
                if u is None:
                    u = index[c] = len(uniq)
                    uniq.append(c)
                inv.append(u)
            U, U_pad = len(uniq), padded_unique(len(uniq))
        else:
            uniq, inv, U, U_pad = captions, list(range(rows)), rows, rows
        count = [0] * U
        for u in inv:
            count[u] += 1
        seg = [0] * (U_pad + 1)
        for u in range(U):
            seg[u + 1] = seg[u] + count[u]
        for u in range(U, U_pad):
            seg[u + 1] = rows
        order, cursor = [0] * rows, seg[:U]
        for r, u in enumerate(inv):
            order[cursor[u]] = r
            cursor[u] += 1
        padded = uniq + [uniq[0]] * (U_pad - U)
        tokens = torch.stack([cache[c][0] for c in padded])
        eot = torch.tensor([cache[c][1] for c in padded], dtype=torch.int64)
        self.rows, self.U, self.U_pad, self.N, self.dedup = rows, U, U_pad, int(tokens.shape[1]), bool(dedup)
        host = torch.cat([tokens.reshape(-1).view(torch.int32), eot.view(torch.int32),
                          torch.tensor(inv + order + seg + [U], dtype=torch.int32)])
        assert host.numel() == self.numel(rows, U_pad, self.N)
        self._bind(host, None)

    @staticmethod
    def layout(rows, U_pad, N):
        """name -> (first int32 word, one past the last); tokens and eot are int64, two words each."""
        out, o = {}, 0
        for name, n in (("tokens", 2 * U_pad * N), ("eot", 2 * U_pad), ("inv", rows), ("order", rows), ("seg", U_pad + 1)):
            out[name] = (o, o + n)
            o += n
        return out

    @staticmethod
    def numel(rows, U_pad, N):
        return 2 * U_pad * N + 2 * U_pad + 2 * rows + U_pad + 2

    def _bind(self, host, dev):
        self.host, self.dev = host, dev
        for name, (lo, hi) in self.layout(self.rows, self.U_pad, self.N).items():
            for suffix, buf in (("_host", host), ("", dev)):
                v = None if buf is None else buf[lo:hi]
                if v is not None and name in ("tokens", "eot"):
                    v = v.view(torch.int64)
                    v = v.view(self.U_pad, self.N) if name == "tokens" else v
                setattr(self, name + suffix, v)

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and not self.host.is_pinned():
            self.host = self.host.pin_memory()
        self._bind(self.host, self.host.to(device, non_blocking=True))
        return self

    def on_buffer(self, dev):
        """The same request read from another device buffer of the same layout (the static input of a captured step)."""
        assert dev.shape == self.host.shape and dev.dtype == torch.int32
        twin = object.__new__(TokenBatch)
        twin.rows, twin.U, twin.U_pad, twin.N, twin.dedup, twin.tokenizer_rows = self.rows, self.U, self.U_pad, self.N, self.dedup, 0
        twin._bind(self.host, dev)
        return twin


def index_capacity(B, N, vocab, chunk=None):
    """The capacity layout of hig_clip_embed_index_build (include/hig.h) restated: {name: (first int32, entries)}, the total, and
    (cap_ids, cap_chunks)."""
    chunk = embed_chunk() if chunk is None else int(chunk)
    M = B * N
    cap_ids = min(M, vocab)
    cap_chunks = (M + chunk - 1) // chunk + cap_ids
    out, o = {}, 0
    for name, n in zip(EmbedIndex.FIELDS, (M, cap_chunks + 1, cap_chunks, cap_ids + 1, cap_ids, M, N + 1)):
        out[name] = (o, n)
        o += n
    return out, o, (cap_ids, cap_chunks)


class DeviceEmbedIndex:
    """The buffers of hig_clip_embed_index_build for one (B, N, vocab): `index` (the capacity layout), `counts` (n_live, n_chunks,
    n_ids) and the sort's scratch, allocated once -- a captured step holds their pointers.  `build(tokens)` launches the entry on
    the current stream; `live()` reads the live prefix of every array back (tests and tools only: it synchronises)."""

    def __init__(self, B, N, vocab, device):
        from .. import _lib
        ints, nbytes = _lib.api.hig_clip_embed_index_cap_ints(B, N, vocab), _lib.api.hig_clip_embed_index_scratch_bytes(B, N, vocab)
        self.B, self.N, self.vocab, self.device = B, N, vocab, torch.device(device)
        self.index = torch.zeros(ints, dtype=torch.int32, device=device)
        self.counts = torch.zeros(3, dtype=torch.int32, device=device)
        self.scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)

    def build(self, tokens):
        from .. import _lib
        assert tokens.shape == (self.B, self.N) and tokens.dtype == torch.int64 and tokens.is_contiguous() and tokens.device == self.index.device
        _lib.api.hig_clip_embed_index_build(tokens, self.B, self.N, self.vocab, self.index, self.counts, self.scratch)
        return self

    def live(self):
        lay = index_capacity(self.B, self.N, self.vocab)[0]
        n_live, n_chunks, n_ids = (int(v) for v in self.counts.cpu())
        host = self.index.cpu().numpy()
        lens = (n_live, n_chunks + 1, n_chunks, n_ids + 1, n_ids, self.B * self.N, self.N + 1)
        return (n_live, n_chunks, n_ids), {name: host[lay[name][0]:lay[name][0] + n] for name, n in zip(EmbedIndex.FIELDS, lens)}


def tower_backward_dev(table, dindex, dout, saved, gtable, pool=None):
    """hig_clip_text_bwd_dev: upstream dout (B, N, W) -> the gradients of table.tensors written through `gtable` (a c_void_p table in
    that order: the fused step points it into the flat gradient buffer), with the embedding pass on the device-built index."""
    from .. import _lib
    dims, ws, B = saved
    dev = table.device
    if (dindex.B, dindex.N, dindex.vocab) != (B, table.N, table.vocab) or dindex.index.device != dev:
        raise RuntimeError("CLIP text tower: the embedding index does not belong to these tokens")
    dout = dout.contiguous()
    assert dout.shape == (B, table.N, table.W) and dout.dtype == torch.float32
    nb = _lib.api.hig_clip_text_bwd_workspace_bytes(dims)
    bws = pool.take("clip_bwd", nb, dev) if pool is not None else torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.api.hig_clip_text_bwd_dev(dims, table.table, dindex.index, dindex.counts, dout, ws, gtable, bws)
    if pool is not None:
        pool.give("clip_bwd", bws, dev)
        pool.give("clip_t", ws, dev)
