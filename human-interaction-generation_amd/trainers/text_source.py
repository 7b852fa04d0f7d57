"""Where the fused / captured training step gets its text embeddings from: one small class per source, resolved once per step
by `DDPMTrainer._text_source`.  Every source has
    kind, trains_head    its name in the key of a captured graph; whether the step also covers the parameters behind the core
    trains_tower         (Tokens only; absent = False) whether it also covers the CLIP text tower behind the text head
    statics()            the device tensors a captured step copies into static buffers before every replay
    on(statics)          the same source reading from those buffers
    key(core)            what else the key of a captured graph must tell apart
    forward(trainer)     -> (xf_proj, xf_out), keeping on the instance what `backward` needs
    backward(trainer, dxf_proj, dxf_out)    the head's gradients into the flat gradient, behind the denoiser's backward
"""
from ..models.caption_bank import expand_rows, segment_sum_rows


def _core(encoder):
    """The bare model under a DDP-style wrapper (the reference reaches for `.module` first, :116-119)."""
    return getattr(encoder, "module", encoder)


class _Tensors:
    """A source that is nothing but the step's device tensors: they are its statics."""

    def __init__(self, *tensors):
        self.tensors = tensors

    def statics(self):
        return self.tensors

    def on(self, statics):
        return type(self)(*statics)

    def key(self, core):
        return ()


class Embeddings(_Tensors):
    """`xf_proj=, xf_out=`: text embeddings computed outside the step; nothing runs here and the denoiser core alone is trained."""
    kind, trains_head = "embeddings", False

    def forward(self, trainer):
        return self.tensors

    def backward(self, trainer, dxf_proj, dxf_out):
        pass


class ClipFeatures(_Tensors):
    """`clip_out=` (B, N, W), `eot=` (B,): the text head runs inside the step, forward and backward, and is trained too."""
    kind, trains_head = "clip", True

    def forward(self, trainer):
        xf_proj, xf_out, tsaved = _core(trainer.encoder)._launch_text_head(*self.tensors, training=True)
        self._saved = (xf_out, tsaved)
        return xf_proj, xf_out

    def backward(self, trainer, dxf_proj, dxf_out):
        (xf_out, tsaved), self._saved = self._saved, None
        _core(trainer.encoder)._launch_text_head_backward(*self.tensors, xf_out, tsaved, dxf_out, dxf_proj,
                                                          want_dclip=False, into_flat=True)


class ClassIds(_Tensors):
    """`class_ids=`: int32 ids on the device, one per model-batch row, of a cap_id model built with class_head="hip": the class
    head (hig_class_head_fwd / _bwd) stands where the text head stands and is trained."""
    kind, trains_head = "class_ids", True

    def key(self, core):
        return (("class_head", tuple(self.tensors[0].shape)),)

    def forward(self, trainer):
        return _core(trainer.encoder)._launch_class_head(*self.tensors)

    def backward(self, trainer, dxf_proj, dxf_out):
        _core(trainer.encoder)._launch_class_head_backward(*self.tensors, dxf_out, dxf_proj)


class Tokens:
    """`token_batch=`, a clip_text.TokenBatch, on a `no_clip` model built with clip_tower_train="flat": the trainable CLIP text
    tower runs inside the step on the U_pad distinct captions and is trained with the text head and the core.  Forward:
    hig_clip_embed_index_build on the static tokens, hig_clip_text_fwd_train, the text head, two hig_rows_gather_f32 to the model
    batch.  Backward: two hig_rows_segment_sum_f32, the text head's backward (which also hands back d(clip_out)), then
    hig_clip_text_bwd_dev with a gradient table that points into the flat gradient at `tower_offsets` -- written, not accumulated;
    the alignment gaps stay zero, so the step's one hig_sumsq_partial is the joint norm over every parameter."""
    kind, trains_head, trains_tower = "tokens", True, True

    def __init__(self, token_batch):
        self.tb = token_batch

    def statics(self):
        return (self.tb.dev,)        # the one packed int32 buffer: the step's only text input

    def on(self, statics):
        return Tokens(self.tb.on_buffer(*statics))

    def key(self, core):
        return ((self.tb.rows, self.tb.U_pad, self.tb.dedup),)

    def forward(self, trainer):
        from ..models import clip_text
        core, tb = _core(trainer.encoder), self.tb
        table = core.flat_tower_table()
        if tb.N != table.N:
            raise ValueError("token_batch holds %d tokens per caption, the tower takes %d" % (tb.N, table.N))
        # one index per (U_pad, N, vocab), allocated once and never freed: a captured graph holds its pointers
        cache = core.__dict__.setdefault("_tower_index_cache", {})
        key = (tb.U_pad, table.N, table.vocab, table.device)
        dindex = cache.get(key)
        if dindex is None:
            dindex = cache[key] = clip_text.DeviceEmbedIndex(tb.U_pad, table.N, table.vocab, table.device)
        dindex.build(tb.tokens)
        clip_out, tsaved = clip_text.tower_forward_train(table, tb.tokens, core._pool)
        xp_u, xo_u, hsaved = core._launch_text_head(clip_out, tb.eot, training=True)
        self._saved = (table, dindex, clip_out, tsaved, xo_u, hsaved)
        return expand_rows(xp_u, tb.inv, tb.rows), expand_rows(xo_u, tb.inv, tb.rows)

    def backward(self, trainer, dxf_proj, dxf_out):
        from ..models import clip_text
        core, tb = _core(trainer.encoder), self.tb
        (table, dindex, clip_out, tsaved, xo_u, hsaved), self._saved = self._saved, None
        dxp_u = segment_sum_rows(dxf_proj.contiguous(), tb.order, tb.seg, tb.U_pad)
        dxo_u = segment_sum_rows(dxf_out.contiguous(), tb.order, tb.seg, tb.U_pad)
        _, dclip = core._launch_text_head_backward(clip_out, tb.eot, xo_u, hsaved, dxo_u, dxp_u, want_dclip=True, into_flat=True)
        clip_text.tower_backward_dev(table, dindex, dclip, tsaved, core.flat_params().tower_grad_table(), core._pool)


class Banked:
    """`caption_batch=`, a CaptionBatch of the model's caption bank: hig_caption_gather stands where the tower stood.  With
    `text_dedup` the head runs on the U_pad distinct captions, two hig_rows_gather_f32 expand its outputs to the model batch and
    `backward` sums the upstream gradients back, in row order; without it the gather fetches every row."""
    kind, trains_head = "bank", True

    def __init__(self, caption_batch):
        self.cb = caption_batch

    def statics(self):
        return (self.cb.dev,)        # the one packed int32 index buffer

    def on(self, statics):
        return Banked(self.cb.on_buffer(*statics))

    def key(self, core):
        """The buffer's layout, whether the head runs deduplicated, and the bank's buffers (allocated once, they never move)."""
        bank = core.caption_bank
        return ((self.cb.rows, self.cb.U_pad, bool(core.text_dedup), bank.feat.data_ptr(), bank.eot.data_ptr()),)

    def forward(self, trainer):
        core, cb = _core(trainer.encoder), self.cb
        self._dedup = bool(core.text_dedup)
        if not self._dedup:
            self._head = ClipFeatures(*core.caption_bank.gather(cb.slot, cb.rows))
            return self._head.forward(trainer)
        self._head = ClipFeatures(*core.caption_bank.gather(cb.uniq_slot, cb.U_pad))
        xp_u, xo_u = self._head.forward(trainer)
        return expand_rows(xp_u, cb.inv, cb.rows), expand_rows(xo_u, cb.inv, cb.rows)

    def backward(self, trainer, dxf_proj, dxf_out):
        cb = self.cb
        head, self._head = self._head, None
        if self._dedup:     # the head ran on the distinct captions: their rows' gradients, added in row order
            dxf_proj = segment_sum_rows(dxf_proj.contiguous(), cb.order, cb.seg, cb.U_pad)
            dxf_out = segment_sum_rows(dxf_out.contiguous(), cb.order, cb.seg, cb.U_pad)
        head.backward(trainer, dxf_proj, dxf_out)
