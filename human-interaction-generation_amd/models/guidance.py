"""Classifier-free guidance: eps_g = eps_u + s (eps_c - eps_u), the conditional and the unconditional noise estimate taken from
ONE model call on a stacked batch.

The unconditional branch is the same model on the empty caption (`cond_drop_prob` of the trainers teaches it that input); no
weight and no state-dict entry belongs to it.

Stacked layout (include/hig.h, hig_cfg_combine).  For B samples and a `group` with B % group == 0, sample b has its conditional
row at 2 (b // group) group + b % group and its unconditional row `group` further, in a batch of 2 B rows:

    group = B          [cond; uncond]                                  the single-person model
    group = pairs      [p1 cond, p1 uncond, p2 cond, p2 uncond]        the two-person model (model batch = [p1; p2]): row i of the
                                                                       stacked batch still meets row i + half in the interaction
                                                                       attention, so a person keeps its partner in both branches

`ClassifierFreeGuidedModel` is a callable with the model's signature and works with every sampler entry of GaussianDiffusion /
SpacedDiffusion, on any device.  The captured loops recognise it and keep the whole state stacked instead (one fused
hig_*_step_cfg per step, no combine launch): see `GaussianDiffusion._captured_loop`.
"""
import math

import torch as th

from .. import _lib

_STACKED_KEYS = ("xf_proj", "xf_out", "length", "text")


def stack_rows(cond, uncond, group):
    """(B, ...) + (B, ...) -> (2 B, ...) in the stacked layout.  Lists (captions) are stacked as lists."""
    if isinstance(cond, (list, tuple)):
        B = len(cond)
        assert len(uncond) == B and B % group == 0
        out = []
        for g in range(0, B, group):
            out += list(cond[g:g + group]) + list(uncond[g:g + group])
        return out
    B = cond.shape[0]
    assert uncond.shape == cond.shape and B % group == 0
    rest = tuple(cond.shape[1:])
    return th.stack([cond.reshape(B // group, group, *rest), uncond.reshape(B // group, group, *rest)], dim=1).reshape(
        2 * B, *rest)


def split_rows(stacked, group):
    """(2 B, ...) in the stacked layout -> (conditional rows, unconditional rows), each (B, ...) (views where possible)."""
    B2 = stacked.shape[0]
    assert B2 % (2 * group) == 0
    rest = tuple(stacked.shape[1:])
    v = stacked.reshape(B2 // (2 * group), 2, group, *rest)
    return v[:, 0].reshape(B2 // 2, *rest), v[:, 1].reshape(B2 // 2, *rest)


def check_scale(scale, who):
    """The guidance scale as a float; ValueError unless it is a finite number."""
    try:
        s = float(scale)
    except (TypeError, ValueError):
        raise ValueError("%s: guidance scale must be a finite number, got %r" % (who, scale)) from None
    if not math.isfinite(s):
        raise ValueError("%s: guidance scale must be a finite number, got %r" % (who, scale))
    return s


def _expand_rows(u, like):
    """The unconditional counterpart of one keyword: one row (or one caption) stands for the whole batch."""
    if isinstance(like, (list, tuple)):
        u = [u] if isinstance(u, str) else list(u)
        return u * len(like) if len(u) == 1 and len(like) != 1 else u
    u = th.as_tensor(u).to(like.device)
    if u.shape[0] == 1 and like.shape[0] != 1:
        u = u.expand(like.shape[0], *u.shape[1:])
    return u.to(like.dtype) if u.is_floating_point() else u


def default_group(core, B):
    """B for a single-person model, B // 2 (= pairs) for a two-person one (its batch is [person 1 of every pair; person 2])."""
    two = 0
    if hasattr(core, "dims") and hasattr(core, "_launch_forward"):
        two = int(getattr(core.dims(2, 1, 1), "two_person", 0))
    if two:
        if B % 2:
            raise ValueError("a two-person model takes an even batch, got %d" % B)
        return B // 2
    return B


class ClassifierFreeGuidedModel:
    """model(x, t, **kw) -> eps_u + scale (eps_c - eps_u).  `uncond_kwargs` holds the unconditional counterpart of every
    conditioning keyword that differs between the branches (`xf_proj` + `xf_out`, or `text` captions); a counterpart with one
    row serves the whole batch; a keyword without one (`length`) is the same in both branches.  `group`: see the module
    docstring; None = B for a single-person model, B // 2 for a two-person one."""

    def __init__(self, model, scale, uncond_kwargs, group=None):
        self.model = model
        self.scale = check_scale(scale, "ClassifierFreeGuidedModel")
        self.uncond_kwargs = dict(uncond_kwargs or {})
        if not any(k in self.uncond_kwargs for k in ("xf_proj", "xf_out", "text")):
            raise ValueError("ClassifierFreeGuidedModel: uncond_kwargs needs the unconditional xf_proj + xf_out, or text")
        if group is not None and (isinstance(group, bool) or int(group) != group or group <= 0):
            raise ValueError("ClassifierFreeGuidedModel: group must be a positive integer, got %r" % (group,))
        self.group = None if group is None else int(group)

    # ---- what the samplers and the trainers ask of a model --------------------------------------------------
    def parameters(self):
        return self.model.parameters()

    def eval(self):
        self.model.eval()
        return self

    def train(self, mode=True):
        self.model.train(mode)
        return self

    def core(self):
        return getattr(self.model, "module", self.model)

    def group_for(self, B):
        g = default_group(self.core(), B) if self.group is None else self.group
        if B % g:
            raise ValueError("ClassifierFreeGuidedModel: batch %d is no multiple of group %d" % (B, g))
        return g

    def stacked_kwargs(self, kwargs, group):
        """The model's keywords in the stacked layout, the unconditional rows taken from `uncond_kwargs`."""
        for k in self.uncond_kwargs:
            if k not in kwargs or kwargs[k] is None:
                raise ValueError("ClassifierFreeGuidedModel: uncond_kwargs has %r but the call does not" % k)
        out = {}
        for k, v in kwargs.items():
            if v is None or k not in _STACKED_KEYS:
                out[k] = v
                continue
            if not isinstance(v, (list, tuple)):
                v = th.as_tensor(v)
            u = _expand_rows(self.uncond_kwargs[k], v) if k in self.uncond_kwargs else v
            out[k] = stack_rows(v, u, group)
        return out

    def combine(self, out2, B, group):
        """eps_g of the stacked output: hig_cfg_combine on fp32 ROCm tensors, the same three operations as tensor arithmetic
        anywhere else."""
        if out2.is_cuda and out2.dtype == th.float32 and not out2.requires_grad:
            o2 = out2.contiguous()
            out = th.empty(B, *o2.shape[1:], device=o2.device, dtype=th.float32)
            _lib.api.hig_cfg_combine(o2, self.scale, B, group, o2.numel() // (2 * B), out)
            return out
        c, u = split_rows(out2, group)
        d = c - u
        sd = d * self.scale
        return u + sd

    def __call__(self, x, t, **kwargs):
        B = x.shape[0]
        group = self.group_for(B)
        out2 = self.model(stack_rows(x, x, group), stack_rows(t, t, group), **self.stacked_kwargs(kwargs, group))
        return self.combine(out2, B, group)
