"""MI355X-native forward of the reference's two evaluation classifiers:
`MotionEncoder` (codes/models/interaction_transformer.py:641-741) -- class logits plus the pooled
feature that FID / diversity / multimodality are computed on -- and `MotionConsistencyEvalModel`
(:743-829) -- real/fake logits from a learned [cls] token.  Same constructors, attributes,
state-dict keys (checkpoints `best_eval_model.pth` load with strict=True) and call signatures.

By default inference only, which is how the reference's evaluation uses them (EvaluatorModelWrapper,
codes/datasets/evaluator.py:468-493: `.eval()`, under no_grad): the whole forward is ONE C-ABI call,
`hig_eval_encoder_fwd` (include/hig.h, csrc/evalnet.hip); there is no CPU fallback.

Built with `trainable=True` they also train, the way the reference's tools/train_evaluation_model.py and
tools/train_consistency_evaluation_model.py train them: under enabled gradients `forward` is a
`torch.autograd.Function` over `hig_eval_encoder_fwd_train` / `hig_eval_encoder_bwd`, so
`pred, _ = encoder(m1, m2, length=m_lens); lossFn(pred, class_id).backward(); opt.step()` runs unchanged
(`MotionEncoder`'s feature output is differentiable too; the inputs are not).  `time_embed.*` and
`init_pos_embedding` take no part in the forward and get no gradient (`.grad` stays None), as in the
reference.  Training runs exact-fp32 products only (precision "f32"); `trainers.EvalModelTrainer` is the
loop, with the whole step as four C-ABI calls.
"""
import ctypes as C
import os

import torch
from torch import nn

from .. import _lib
from .transformer import _WorkspacePool, zero_module

__all__ = ["MotionEncoder", "MotionConsistencyEvalModel", "softmax_xent"]

_PREC = {"f32": _lib.PREC_F32, "bf16x3": _lib.PREC_BF16X3, "bf16": _lib.PREC_BF16}


def softmax_xent(logits, labels, want_dlogits=True, loss=None):
    """nn.CrossEntropyLoss() (mean) of fp32 device logits (B, C) in one launch of `hig_softmax_xent`:
    -> (loss (device scalar, no host sync), dlogits = (softmax - onehot) / B or None, pred = row argmax (B) int64).
    A label outside [0, C) is refused here, on the host, when `labels` is a host tensor or a sequence; device labels are
    the caller's to have checked (checking them here would be a host sync per step)."""
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError("softmax_xent: logits must be fp32 (B, C), got %s %s" % (logits.dtype, tuple(logits.shape)))
    B, Cn = logits.shape
    if not (B > 0 and 0 < Cn <= 1024):
        raise ValueError("softmax_xent: B > 0 and 0 < C <= 1024 (got B=%d C=%d)" % (B, Cn))
    labels = torch.as_tensor(labels)
    if labels.numel() != B or labels.dtype.is_floating_point:
        raise ValueError("softmax_xent: labels must be %d integer class indices" % B)
    if not labels.is_cuda:
        if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= Cn):
            raise ValueError("softmax_xent: label outside [0, %d)" % Cn)
    if not logits.is_cuda:
        raise RuntimeError("softmax_xent: ROCm device tensors required (no CPU fallback)")
    labels = labels.detach().to(logits.device, torch.int64).view(-1).contiguous()
    logits = logits.detach().contiguous()
    dev = logits.device
    loss = torch.empty((), device=dev, dtype=torch.float32) if loss is None else loss
    dlogits = torch.empty_like(logits) if want_dlogits else None
    pred = torch.empty(B, device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        _lib.api.hig_softmax_xent(logits, labels, B, Cn, loss, dlogits, pred)
    return loss, dlogits, pred


class _EvalTrainFn(torch.autograd.Function):
    """Autograd boundary of the `trainable=True` classifiers: forward = hig_eval_encoder_fwd_train, backward =
    hig_eval_encoder_bwd.  The parameters ride along as inputs so that autograd routes their gradients."""

    @staticmethod
    def forward(ctx, model, x1, x2, length, class_num, *params):
        logits, feature, saved = model._launch_train(x1, x2, length, class_num)
        ctx.model, ctx.saved = model, saved
        ctx.set_materialize_grads(False)
        return (logits, feature) if feature is not None else logits

    @staticmethod
    def backward(ctx, dlogits, dfeature=None):
        if ctx.saved is None:
            raise RuntimeError("%s: backward through this forward a second time -- its activations went back to the "
                               "workspace pool after the first (retain_graph is not supported)" % type(ctx.model).__name__)
        saved, ctx.saved = ctx.saved, None
        grads = ctx.model._launch_bwd(saved, dlogits, dfeature)
        return (None,) * 5 + tuple(grads)


class _EvalEncoderBase(nn.Module):
    """Parameter containers shared by both classifiers (:654-690 / :760-790).  `time_embed` and
    `init_pos_embedding` are never used by the reference's forward but are part of its state dict."""

    _cls_token = 0

    def __init__(self, input_feats, num_frames, latent_dim, ff_size, num_layers, num_heads, dropout, activation,
                 kargs):
        super().__init__()
        if dropout != 0:
            raise NotImplementedError("dropout != 0 is not supported (the evaluator runs in eval mode)")
        if activation != "gelu":
            raise NotImplementedError("only the reference's activation='gelu' is built")
        self.num_frames = num_frames
        self.latent_dim = latent_dim
        self.ff_size = ff_size
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.dropout = dropout
        self.activation = activation
        self.input_feats = input_feats
        self.time_embed_dim = latent_dim * 4
        self.sequence_embedding = nn.Parameter(torch.randn(num_frames, latent_dim))
        self.init_pos_embedding = nn.Parameter(torch.randn(1, latent_dim))
        self.precision = kargs.get("precision", os.environ.get("HIG_PREC", "f32"))
        self.trainable = bool(kargs.get("trainable", False))
        self._pool = _WorkspacePool()

    def _build_trunk(self):
        d = self.latent_dim
        self.joint_embed1 = nn.Linear(self.input_feats, d)
        self.joint_embed2 = nn.Linear(4, d)
        self.time_embed = nn.Sequential(nn.Linear(d, self.time_embed_dim), nn.SiLU(),
                                        nn.Linear(self.time_embed_dim, self.time_embed_dim))
        layer = nn.TransformerEncoderLayer(d_model=d, nhead=self.num_heads, dim_feedforward=self.ff_size,
                                           dropout=self.dropout, activation=self.activation, batch_first=True)
        self.motionTransEncoder = nn.TransformerEncoder(layer, num_layers=self.num_layers,
                                                        enable_nested_tensor=False)

    # hig.h table: HIG_EV_* globals, then per layer the HIG_TL_* block
    def _globals(self):
        raise NotImplementedError

    def _slots(self):
        ps = list(self._globals())
        for layer in self.motionTransEncoder.layers:
            a = layer.self_attn
            ps += [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
                   layer.norm1.weight, layer.norm1.bias, layer.linear1.weight, layer.linear1.bias,
                   layer.linear2.weight, layer.linear2.bias, layer.norm2.weight, layer.norm2.bias]
        return ps

    def trained_parameters(self):
        """The parameters the forward uses, in table order: what training gives a gradient (everything but
        `time_embed.*` and `init_pos_embedding`)."""
        return [p for p in self._slots() if p is not None]

    def _table(self, tensors=None):
        """The C table of the parameters, or of `tensors`: one tensor per trained parameter, in table order (gradients)."""
        ps = self._slots()
        if tensors is not None:
            it = iter(tensors)
            ps = [None if p is None else next(it) for p in ps]
        arr = (C.c_void_p * len(ps))()
        for i, p in enumerate(ps):
            if p is None:
                arr[i] = None
                continue
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError("evaluation classifier: parameters must be contiguous fp32 ROCm tensors "
                                   "(no CPU fallback; the CPU restatement lives in oracle/ for tests only)")
            arr[i] = p.data_ptr()
        return arr

    def _src_mask_block(self, T, length):
        length = torch.as_tensor(length).detach().to("cpu", torch.int64).view(-1)
        return (torch.arange(T)[None, :] < length[:, None]).float()

    def _launch(self, x1, x2, length, class_num, want_feature):
        if self.trainable and torch.is_grad_enabled():
            if x1.requires_grad or x2.requires_grad:
                raise ValueError("%s: there is no gradient for x1 / x2 -- detach the inputs" % type(self).__name__)
            self._check_shapes(x1, x2, length, ValueError)
            if not (x1.is_cuda and x2.is_cuda):
                raise RuntimeError("%s.forward: ROCm device tensors required (no CPU fallback)" % type(self).__name__)
            out = _EvalTrainFn.apply(self, x1, x2, length, class_num, *self.trained_parameters())
            return out if want_feature else (out, None)
        if not (x1.is_cuda and x2.is_cuda):
            raise RuntimeError("%s.forward: ROCm device tensors required (no CPU fallback)" % type(self).__name__)
        if torch.is_grad_enabled() and self.training:
            raise NotImplementedError("%s: inference only -- call .eval() / torch.no_grad() like the reference's "
                                      "EvaluatorModelWrapper does" % type(self).__name__)
        x1, x2, length, dims = self._prepare(x1, x2, length, class_num)
        B, dev = x1.shape[0], x1.device
        ws = self._pool.take("eval_ws", _lib.api.hig_eval_encoder_workspace_bytes(dims), dev)
        logits = torch.empty(B, class_num, device=dev, dtype=torch.float32)
        feature = torch.empty(B, self.latent_dim, device=dev, dtype=torch.float32) if want_feature else None
        table = self._table()
        with torch.cuda.device(dev):
            _lib.api.hig_eval_encoder_fwd(dims, table, x1, x2, length, logits, feature, ws)
        self._pool.give("eval_ws", ws, dev)   # stream-ordered reuse: the next call launches behind this one
        return logits, feature

    def _check_shapes(self, x1, x2, length, shape_error):
        if x1.dim() != 3 or x2.shape != x1.shape or x1.shape[2] != self.input_feats or not 2 <= x1.shape[1] <= self.num_frames + 1:
            raise shape_error("%s: x1, x2 must both be (B, T, %d) with 2 <= T <= %d, got %s and %s"
                              % (type(self).__name__, self.input_feats, self.num_frames + 1, tuple(x1.shape), tuple(x2.shape)))
        if length is None:
            raise ValueError("length is required (the reference indexes it unconditionally)")
        if torch.as_tensor(length).numel() != x1.shape[0]:
            raise shape_error("%s: length must hold one entry per pair (%d)" % (type(self).__name__, x1.shape[0]))

    def _prepare(self, x1, x2, length, class_num, shape_error=AssertionError):
        self._check_shapes(x1, x2, length, shape_error)
        B, T, F_ = x1.shape
        dev = x1.device
        x1 = x1.detach().float().contiguous()
        x2 = x2.detach().float().contiguous()
        length = torch.as_tensor(length).detach().to(dev, torch.int64).view(-1).contiguous()
        dims = _lib.EvalDims(B=B, T=T, F=F_, d=self.latent_dim, H=self.num_heads, ff=self.ff_size,
                             L=self.num_layers, C=class_num, cls=self._cls_token, prec=_PREC[self.precision])
        return x1, x2, length, dims

    def _launch_train(self, x1, x2, length, class_num):
        """hig_eval_encoder_fwd_train -> (logits, feature or None, what the backward needs).  The activation workspace is
        held until `_launch_bwd` (or `_release`) returns it to the pool."""
        if not (x1.is_cuda and x2.is_cuda):
            raise RuntimeError("%s.forward: ROCm device tensors required (no CPU fallback)" % type(self).__name__)
        if self.precision != "f32":
            raise NotImplementedError("%s: training runs exact-fp32 products only (precision='f32'), not %r"
                                      % (type(self).__name__, self.precision))
        x1, x2, length, dims = self._prepare(x1, x2, length, class_num, shape_error=ValueError)
        B, dev = x1.shape[0], x1.device
        ws = self._pool.take("eval_train_ws", _lib.api.hig_eval_encoder_train_workspace_bytes(dims), dev)
        logits = torch.empty(B, class_num, device=dev, dtype=torch.float32)
        feature = None if self._cls_token else torch.empty(B, self.latent_dim, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.api.hig_eval_encoder_fwd_train(dims, self._table(), x1, x2, length, logits, feature, ws)
        return logits, feature, (dims, x1, x2, length, ws, [p._version for p in self.trained_parameters()])

    def _release(self, saved):
        self._pool.give("eval_train_ws", saved[4], saved[4].device)

    def _launch_bwd(self, saved, dlogits, dfeature, grads=None):
        """hig_eval_encoder_bwd.  grads: one fp32 device tensor per trained parameter (table order) to write into; None
        allocates them.  The kernel sequence writes rows [0, T - 1) of sequence_embedding's gradient, the rows the forward read;
        the rows behind them are zeroed here on every call (T may change from one batch to the next).  Returns the list.  The
        activation workspace goes back to the pool whether or not the call succeeds."""
        try:
            return self._bwd(saved, dlogits, dfeature, grads)
        finally:
            self._release(saved)

    def _bwd(self, saved, dlogits, dfeature, grads):
        dims, x1, x2, length, ws, versions = saved
        dev = x1.device
        ps = self.trained_parameters()
        if versions != [p._version for p in ps]:
            raise RuntimeError("%s: a parameter was modified in place between forward and backward; the kept activations "
                               "no longer belong to it" % type(self).__name__)
        if grads is None:
            grads = [torch.empty_like(p) for p in ps]
        grads[0][dims.T - 1:].zero_()          # sequence_embedding is the table's first slot (HIG_EV_SEQ_EMB)
        if dlogits is None:
            dlogits = torch.zeros(dims.B, dims.C, device=dev, dtype=torch.float32)
        dlogits = dlogits.detach().float().contiguous()
        if dfeature is not None:
            dfeature = dfeature.detach().float().contiguous()
        bws = self._pool.take("eval_bwd_ws", _lib.api.hig_eval_encoder_bwd_workspace_bytes(dims), dev)
        with torch.cuda.device(dev):
            _lib.api.hig_eval_encoder_bwd(dims, self._table(), x1, x2, length, ws, dlogits, dfeature, self._table(grads), bws)
        self._pool.give("eval_bwd_ws", bws, dev)
        return grads


class MotionEncoder(_EvalEncoderBase):
    """Drop-in for the reference class (interaction_transformer.py:641-741)."""

    def __init__(self, input_feats, num_frames=240, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8,
                 dropout=0, class_num=26, activation="gelu", **kargs):
        super().__init__(input_feats, num_frames, latent_dim, ff_size, num_layers, num_heads, dropout, activation,
                         kargs)
        self._build_trunk()
        self.out1 = zero_module(nn.Linear(latent_dim, latent_dim))
        self.out2 = zero_module(nn.Linear(latent_dim, latent_dim))
        self.fin_proj = nn.Sequential(nn.Linear(latent_dim, class_num))

    def _globals(self):
        return (self.sequence_embedding, self.joint_embed1.weight, self.joint_embed1.bias,
                self.joint_embed2.weight, self.joint_embed2.bias, self.out1.weight, self.out1.bias,
                self.out2.weight, self.out2.bias, self.fin_proj[0].weight, self.fin_proj[0].bias, None)

    def generate_src_mask(self, T, length):
        """(B, 2T) float CPU mask: each person's tokens t < length[b] (:695-704)."""
        m = self._src_mask_block(T, length)
        return torch.cat([m, m], dim=1)

    def forward(self, x1, x2, length=None, text=None, xf_proj=None, xf_out=None):
        """x1, x2: (B, T, input_feats) -> (class logits (B, class_num), pooled feature (B, latent_dim))."""
        return self._launch(x1, x2, length, self.fin_proj[0].out_features, True)


class MotionConsistencyEvalModel(_EvalEncoderBase):
    """Drop-in for the reference class (interaction_transformer.py:743-829)."""

    _cls_token = 1

    def __init__(self, input_feats, num_frames=240, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8,
                 dropout=0, interaction_class_num=26, class_num=2, activation="gelu", **kargs):
        super().__init__(input_feats, num_frames, latent_dim, ff_size, num_layers, num_heads, dropout, activation,
                         kargs)
        self.cls_input = nn.Parameter(torch.randn(1, 1, latent_dim))
        self._build_trunk()
        self.cls_output = nn.Sequential(nn.Linear(latent_dim, class_num))

    def _globals(self):
        return (self.sequence_embedding, self.joint_embed1.weight, self.joint_embed1.bias,
                self.joint_embed2.weight, self.joint_embed2.bias, None, None, None, None,
                self.cls_output[0].weight, self.cls_output[0].bias, self.cls_input)

    def generate_src_mask(self, T, length):
        """(B, 1 + 2T) float CPU mask: the [cls] token, then each person's tokens t < length[b] (:792-801)."""
        m = self._src_mask_block(T, length)
        return torch.cat([torch.ones(m.shape[0], 1), m, m], dim=1)

    def forward(self, x1, x2, length=None, text=None, xf_proj=None, xf_out=None):
        """x1, x2: (B, T, input_feats) -> logits (B, class_num)."""
        return self._launch(x1, x2, length, self.cls_output[0].out_features, False)[0]
