"""The two fp32 encoder training chains on the device, held launch by launch: one hig_eval_encoder_fwd_train + hig_eval_encoder_bwd
(MotionEncoder and consistency model) or one hig_text_head_fwd (training) + hig_text_head_bwd per case, the backward with the
debug tap set (hig_enc_bwd_debug_tap); then EVERY buffer a launch of the two calls wrote -- emb, h, kpad, every layer's saved
activations, o, feat, the logits / xf_out, xf_proj, the tapped and the surviving backward buffers, every parameter gradient, dclip
-- is held per element to the bound of the launch that wrote it, with that launch's operands taken from the device's own buffers
(tests/enc_step_bounds.py in check mode).  That the stages form the models is what tests/test_cpu_enc_step_bounds.py shows; nothing
here bounds a whole model.

Around the walk, in the manner of `Region` and `Guarded`: the workspaces, the tap, the outputs and the gradient table start as a
NaN pattern and sit between guard bands; every traced buffer must have been written and every buffer of the trace is held (the
walk's `seen`); the bands, the gaps between the gradients and the rows of d(sequence_embedding) the call does not own keep their
bits, and so do the slots a call has no business with (x0 under the identity pre-projection, DGATH without dxf_proj).  The layout
totals are the three *_workspace_bytes / *_tap_bytes of each model.  A tap shorter than *_tap_bytes is refused before anything is
written, and so is a tapped backward on a capturing stream.  The rows of padded tokens of every tapped d(.) of the evaluator are
exact zeros (stage kind pad_zero).  A second backward without the tap reproduces every gradient bit for bit; hig_eval_encoder_fwd
(prec f32, its own guarded workspace) gives logits and feature bit-equal to the training forward's, the inference text head
xf_out and xf_proj.  The attention launch counters move by exactly L forward and L backward launches of the kernel the case is
meant to reach (VALU at head dim 8, the matrix cores at 64 and 128), as hig_attn_plan names them; hig_gemm_plan names the tiled
fp32 kernel for the in-projection and for the K = 4 joint_embed2 GEMM.

Largest |error| / bound per stage kind on an MI355X (the case and the buffer that gave it; ('g', s) / ('gl', l, s): the gradient of
slot s of the table / of layer l):
    stage kind     evaluation classifiers                          text head
    attn           0.156  hd8 con lse[1]                            0.097  pre no_dclip lse[1]
    attn_bwd       0.253  hd8 enc delta[0]                          0.259  pre no_dxf_out delta[0]
    colsum         0.095  hd64 enc postmp                           0.060  pre no_dclip d(text_proj.0.bias)
    copy           0.000  (bit-equal everywhere)                    0.000
    gather         -                                                0.000  (bit-equal)
    gemm32         0.387  d512 con dh_L                             0.325  identity no_dclip d(text_proj.0.weight)
    gemm32_dgelu   0.009  hd8 enc dfeature dz[1]                    0.021  pre no_dclip dz[0]
    gemm32_gelu    0.012  hd8 con f[0]                              0.026  pre no_dclip f[0]
    head_scale     0.986  hd8 enc dfeature gn                       -
    ln             0.399  hd64 con x1[1]                            0.315  pre no_dclip x1[0]
    ln_bwd         0.139  hd8 enc dfeature dr1[0]                   0.218  pre no_dxf_out dr1[0]
    masked_mean    0.363  d1024 enc feat                            -
    pad_zero       0.000  (exact zeros everywhere)                  -
    pool           0.500  d1024 enc pool2                           -
    scatter        -                                                0.988  identity no_dclip dxf_total
    xsum           0.091  d1024 enc d(in_proj_bias)[0]              0.013  pre no_dxf_out d(in_proj_bias)[1]
Ratios above 0.5 belong to bounds of ONE rounding, which a few thousand elements come close to exhausting: head_scale's gn (one
product, u |gn|), the scatter (one add, u |result|), pool2 (one rounding happens, two terms are counted).  No stage failed, so no
kernel and no bound was changed for this test.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import enc_step_bounds as eb  # noqa: E402
import test_gpu_attn_contract as AC  # noqa: E402  (helpers only: nothing of it is collected from here)
from attn_dispatch_cases import full_paths, plan as attn_plan  # noqa: E402
from gemm_dispatch_cases import BIAS, fake_desc, plan as gemm_plan  # noqa: E402
from hig_amd import _lib  # noqa: E402
from test_gpu_bf16_step_contract import GUARD, PAT16, PAT32, Region  # noqa: E402

DEV = "cuda"
F32, U8 = torch.float32, torch.uint8


def layout(fn, dims, which, n):
    arr = (C.c_int64 * n)()
    assert fn(C.byref(dims), which, arr, n) == n
    return list(arr)


class Grads:
    """The gradient table: one Region, every gradient 256-byte aligned with a gap of 256 bytes behind it."""

    def __init__(self, P):
        self.shapes, self.off, o = {}, {}, 0
        keys = [(("g", s), t) for s, t in enumerate(P.glob)] + [(("gl", l, s), t) for l, row in enumerate(P.lay) for s, t in enumerate(row)]
        self.order = [k for k, _ in keys]
        for k, t in keys:
            if t is not None:
                self.shapes[k], self.off[k] = tuple(t.shape), o
                o += (t.numel() * 4 + 255) // 256 * 256 + 256
        self.region = Region(o)
        self.covered = torch.zeros(o // 4, dtype=torch.bool, device=DEV)
        for k, off in self.off.items():
            self.covered[off // 4:off // 4 + int(torch.tensor(self.shapes[k]).prod())] = True

    def view(self, k):
        return self.region.view(self.off[k], self.shapes[k], F32)

    def table(self):
        return (C.c_void_p * len(self.order))(*[self.region.buf.data_ptr() + GUARD + self.off[k] if k in self.off else None for k in self.order])

    def words(self):
        return self.region.view(0, (self.region.n // 4,), torch.int32)

    def reset(self):
        self.region.buf.fill_(PAT16)


def param_table(P):
    dev = [None if t is None else t.to(DEV).contiguous() for t in list(P.glob) + [t for row in P.lay for t in row]]
    return dev, (C.c_void_p * len(dev))(*[None if t is None else t.data_ptr() for t in dev])


def fview(region, off, shape, dtype=F32):
    return region.view(off * 4, shape, dtype)


def layer_trace(tr, D, ws, fw, slots, tap, tp):
    """The per-layer buffers of the training forward (slots: name -> layout index) and of the tap."""
    rows, wide, stat, hs = (D.M, D.n), (D.M, 3 * D.n), (D.M, 2), (D.B, D.H, D.S)
    shapes = {"qkv": wide, "lse": hs, "att": rows, "r1": rows, "st1": stat, "x1": rows, "z": (D.M, D.ff), "f": (D.M, D.ff), "r2": rows, "st2": stat,
              "x2": rows}
    taps = (("dh_in", _lib.ETAP_DH_IN, rows), ("dr2", _lib.ETAP_DR2, rows), ("dz", _lib.ETAP_DZ, (D.M, D.ff)), ("dx1", _lib.ETAP_DX1, rows),
            ("dr1", _lib.ETAP_DR1, rows), ("datt", _lib.ETAP_DATT, rows), ("dqkv", _lib.ETAP_DQKV, wide), ("delta", _lib.ETAP_DELTA, hs))
    for l in range(D.L):
        base = fw[slots["LAYER0"]] + fw[slots["LSTRIDE"]] * l
        for key, shape in shapes.items():
            tr[(key, l)] = fview(ws, base + fw[slots[key.upper()]], shape)
        tbase = tp[_lib.ETAP_LAYER0] + tp[_lib.ETAP_LSTRIDE] * l
        for key, slot, shape in taps:
            tr[(key, l)] = fview(tap, tbase + tp[slot], shape)


def finish(name, tr, walk_cls, P, D, inp):
    """Every traced buffer written; the walk in check mode over the trace; every buffer of the trace held."""
    for key, t in tr.items():
        if t.dtype == U8:
            assert (t <= 1).all(), "%s: not every byte was written" % (key,)
        else:
            assert torch.isfinite(t).all(), "%s: not every element was written" % (key,)
    walk = walk_cls(P, D, inp, eb.REF, trace={k: v.cpu() for k, v in tr.items()}).run()
    assert walk.seen == set(tr), (walk.seen ^ set(tr))
    for kind, (ratio, key) in sorted(walk.worst.items()):
        print("RATIO %s | %s | %.3f | %s" % (name, kind, ratio, key))
    bad = {k: v for k, v in walk.worst.items() if not v[0] <= 1.0}
    assert not bad, "%s: stages beyond their bound: %s" % (name, bad)
    return walk.worst


def attention_launches(D, before):
    """Exactly L forward and L backward launches of the kernels hig_attn_plan names for the shape, which are the ones the case is
    meant to reach."""
    moved = {n: a - b for n, a, b in zip(AC.PATHS, AC.counts(), before) if a != b}
    fwd, bwd = full_paths(D.hd)
    assert attn_plan("full_fwd", "f32", D.B, D.S, D.H, D.hd, Tk=D.S, chip_cus=AC.ncu())[1] == fwd
    assert attn_plan("full_bwd", "f32", D.B, D.S, D.H, D.hd, Tk=D.S, chip_cus=AC.ncu())[1] == bwd
    assert moved == {fwd: D.L, bwd: D.L}, moved


def refused_untouched(rc, grads, tap):
    torch.cuda.synchronize()
    assert rc == _lib.EINVAL and (grads.words() == PAT32).all() and (tap.buf == PAT16).all(), (rc, _lib.last_error())


# ---- the evaluation classifiers ---------------------------------------------------------------------------------------------
EFW = {k: getattr(_lib, "EFW_" + k) for k in ("LAYER0", "LSTRIDE", "QKV", "LSE", "ATT", "R1", "ST1", "X1", "Z", "F", "R2", "ST2", "X2")}
TFW = {k: getattr(_lib, "TFW_" + k) for k in EFW}


@pytest.mark.parametrize("kind,dfeature", [("enc", True), ("enc", False), ("con", False)])
@pytest.mark.parametrize("name", list(eb.EVAL_CASES))
def test_every_stage_of_the_evaluator_step_within_its_bound(name, kind, dfeature):
    c, D, P, inp = eb.eval_setup(name, kind)
    if not dfeature:
        inp = dict(inp, dfeature=None)
    L, S = _lib.lib(), _lib.stream_ptr()
    dims = _lib.EvalDims(B=D.B, T=D.T, F=D.F, d=D.d, H=D.H, ff=D.ff, L=D.L, C=D.C, cls=D.cls, prec=_lib.PREC_F32)
    fw = layout(L.hig_eval_encoder_layout, dims, _lib.ENC_LAYOUT_FWD, _lib.EFW_NSLOTS)
    bw = layout(L.hig_eval_encoder_layout, dims, _lib.ENC_LAYOUT_BWD, _lib.EBW_NSLOTS)
    tp = layout(L.hig_eval_encoder_layout, dims, _lib.ENC_LAYOUT_TAP, _lib.ETAP_NSLOTS)
    assert fw[_lib.EFW_TOTAL] * 4 == L.hig_eval_encoder_train_workspace_bytes(C.byref(dims))
    assert bw[_lib.EBW_TOTAL] * 4 == L.hig_eval_encoder_bwd_workspace_bytes(C.byref(dims))
    assert tp[_lib.ETAP_TOTAL] * 4 == L.hig_eval_encoder_bwd_tap_bytes(C.byref(dims))
    assert tp[_lib.ETAP_DXF_TOTAL] == tp[_lib.ETAP_DGATH] == -1 and (fw[_lib.EFW_O] == -1) == (bw[_lib.EBW_POOL1] == -1) == bool(D.cls)
    ws, bws, tap = Region(fw[_lib.EFW_TOTAL] * 4), Region(bw[_lib.EBW_TOTAL] * 4), Region(tp[_lib.ETAP_TOTAL] * 4)
    iws = Region(L.hig_eval_encoder_workspace_bytes(C.byref(dims)))
    logits, feature = Region(D.B * D.C * 4), Region(D.B * D.d * 4)
    grads = Grads(P)
    keep, ptab = param_table(P)
    gtab = grads.table()
    x1, x2, length, dl = (inp[k].to(DEV).contiguous() for k in ("x1", "x2", "length", "dlogits"))
    dfe = None if inp["dfeature"] is None else inp["dfeature"].to(DEV).contiguous()
    fptr = None if D.cls else feature.ptr()
    assert attn_plan("full_fwd", "f32", D.B, D.S, D.H, D.hd, Tk=D.S, chip_cus=AC.ncu())[1] == {8: "FULL_FWD", 64: "FULL_FWD_MFMA", 128: "FULL_FWD_MFMA"}[D.hd]
    assert gemm_plan("f32", fake_desc("f32", D.M, 3 * D.d, D.d, BIAS))[1] == {"TILED32": 1}
    assert gemm_plan("f32", fake_desc("f32", D.B, D.d, 4, BIAS))[1] == {"TILED32": 1}
    before = AC.counts()

    _lib.check(L.hig_eval_encoder_fwd_train(C.byref(dims), ptab, _lib.ptr(x1), _lib.ptr(x2), _lib.ptr(length), logits.ptr(), fptr, ws.ptr(), S))

    def backward(with_tap, tap_bytes=None):
        grads.reset()
        bws.buf.fill_(PAT16)
        _lib.check(L.hig_enc_bwd_debug_tap(tap.ptr() if with_tap else None, tap.n if tap_bytes is None else tap_bytes))
        try:
            return L.hig_eval_encoder_bwd(C.byref(dims), ptab, _lib.ptr(x1), _lib.ptr(x2), _lib.ptr(length), ws.ptr(), _lib.ptr(dl), _lib.ptr(dfe), gtab,
                                          bws.ptr(), S)
        finally:
            _lib.check(L.hig_enc_bwd_debug_tap(None, 0))

    refused_untouched(backward(True, tap.n - 256), grads, tap)       # a short tap: refused before anything is written
    _lib.check(backward(True))
    torch.cuda.synchronize()
    attention_launches(D, before)
    first = grads.region.buf.clone()
    for r_ in (ws, bws, tap, logits, feature, grads.region):
        assert r_.intact(), "a store landed in a guard band"
    assert (grads.words()[~grads.covered] == PAT32).all(), "a store landed between the gradients"
    seq = grads.view(("g", _lib.EV_SEQ_EMB))
    assert (seq.view(torch.int32)[D.T - 1:] == PAT32).all(), "rows of d(sequence_embedding) at or beyond T - 1 are the caller's"

    # ---- the trace ----
    tr = {"emb": fview(ws, fw[_lib.EFW_EMB], (2 * D.B * D.T, D.d)), "h": fview(ws, fw[_lib.EFW_H], (D.M, D.d)),
          "kpad": fview(ws, fw[_lib.EFW_KPAD], (D.B, D.S), U8), "logits": logits.view(0, (D.B, D.C), F32)}
    layer_trace(tr, D, ws, fw, EFW, tap, tp)
    rows, bd = (D.M, D.d), (D.B, D.d)
    tr["dh_L"], tr["dh0"] = fview(tap, tp[_lib.ETAP_DH_L], rows), fview(tap, tp[_lib.ETAP_DH_0], rows)
    assert torch.equal(fview(bws, bw[_lib.EBW_DB], rows), tr["dh0"]), "what the backward leaves in dB is what the tap saw"
    if not D.cls:
        tr["o"], tr["feat"], tr["feature"] = fview(ws, fw[_lib.EFW_O], rows), fview(ws, fw[_lib.EFW_FEAT], bd), feature.view(0, bd, F32)
        for key in ("dft", "g", "gn", "g2", "pool1", "pool2", "u1", "u2"):
            tr[key] = fview(bws, bw[getattr(_lib, "EBW_" + key.upper())], bd)
    for key, slot, shape in (("xcat", _lib.EBW_XCAT, (2 * D.B * D.T, D.F)), ("dmove", _lib.EBW_DMOVE, (2 * D.B * D.T, D.d)),
                             ("dinit", _lib.EBW_DINIT, (2 * D.B, D.d)), ("postmp", _lib.EBW_POSTMP, (D.T, D.d))):
        tr[key] = fview(bws, bw[slot], shape)
    for k in grads.off:
        tr[k] = grads.view(k)
    tr[("g", _lib.EV_SEQ_EMB)] = seq[:D.T - 1]
    finish("%s %s%s" % (name, kind, " dfeature" if dfeature else ""), tr, eb.EvalWalk, P, D, inp)

    # ---- the same bits without the tap; the inference forward ----
    _lib.check(backward(False))
    torch.cuda.synchronize()
    assert torch.equal(grads.region.buf, first), "the backward without the tap gives other bits"
    lg2, ft2 = Region(D.B * D.C * 4), Region(D.B * D.d * 4)
    _lib.check(L.hig_eval_encoder_fwd(C.byref(dims), ptab, _lib.ptr(x1), _lib.ptr(x2), _lib.ptr(length), lg2.ptr(), None if D.cls else ft2.ptr(), iws.ptr(), S))
    torch.cuda.synchronize()
    assert iws.intact() and lg2.intact() and ft2.intact(), "a store landed in a guard band of the inference forward"
    assert torch.equal(lg2.buf, logits.buf) and torch.equal(ft2.buf, feature.buf), "hig_eval_encoder_fwd differs from the training forward"
    del keep


# ---- the text head ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", eb.TEXT_VARIANTS)
@pytest.mark.parametrize("name", list(eb.TEXT_CASES))
def test_every_stage_of_the_text_head_step_within_its_bound(name, variant):
    c, D, P, inp = eb.text_setup(name, variant)
    L, S = _lib.lib(), _lib.stream_ptr()
    dims = _lib.TextDims(B=D.B, N=D.N, W=D.W, Lt=D.Lt, H=D.H, ff=D.ff, L=D.L, E=D.E, prec=_lib.PREC_F32)
    fw = layout(L.hig_text_head_layout, dims, _lib.ENC_LAYOUT_FWD, _lib.TFW_NSLOTS)
    bw = layout(L.hig_text_head_layout, dims, _lib.ENC_LAYOUT_BWD, _lib.TBW_NSLOTS)
    tp = layout(L.hig_text_head_layout, dims, _lib.ENC_LAYOUT_TAP, _lib.ETAP_NSLOTS)
    assert fw[_lib.TFW_TOTAL] * 4 == L.hig_text_head_workspace_bytes(C.byref(dims), 1)
    assert bw[_lib.TBW_TOTAL] * 4 == L.hig_text_head_bwd_workspace_bytes(C.byref(dims))
    assert tp[_lib.ETAP_TOTAL] * 4 == L.hig_text_head_bwd_tap_bytes(C.byref(dims)) and tp[_lib.ETAP_DH_L] == tp[_lib.ETAP_DH_0] == -1
    ws, bws, tap = Region(fw[_lib.TFW_TOTAL] * 4), Region(bw[_lib.TBW_TOTAL] * 4), Region(tp[_lib.ETAP_TOTAL] * 4)
    iws = Region(L.hig_text_head_workspace_bytes(C.byref(dims), 0))
    xf_out, xf_proj, dclip = Region(D.M * D.Lt * 4), Region(D.B * D.E * 4), Region(D.M * D.W * 4)
    grads = Grads(P)
    keep, ptab = param_table(P)
    gtab = grads.table()
    clip, eot = inp["clip_out"].to(DEV).contiguous(), inp["eot"].to(DEV)
    dxo = None if inp["dxf_out"] is None else inp["dxf_out"].to(DEV).contiguous()
    dxp = None if inp["dxf_proj"] is None else inp["dxf_proj"].to(DEV).contiguous()
    assert attn_plan("full_fwd", "f32", D.B, D.S, D.H, D.hd, Tk=D.S, chip_cus=AC.ncu())[1] == {8: "FULL_FWD", 64: "FULL_FWD_MFMA"}[D.hd]
    before = AC.counts()

    _lib.check(L.hig_text_head_fwd(C.byref(dims), ptab, _lib.ptr(clip), _lib.ptr(eot), xf_out.ptr(), xf_proj.ptr(), ws.ptr(), 1, S))

    def backward(with_tap, tap_bytes=None):
        grads.reset()
        bws.buf.fill_(PAT16)
        dclip.buf.fill_(PAT16)
        _lib.check(L.hig_enc_bwd_debug_tap(tap.ptr() if with_tap else None, tap.n if tap_bytes is None else tap_bytes))
        try:
            return L.hig_text_head_bwd(C.byref(dims), ptab, _lib.ptr(clip), _lib.ptr(eot), xf_out.ptr(), ws.ptr(), _lib.ptr(dxo), _lib.ptr(dxp), gtab,
                                       dclip.ptr() if inp["want_dclip"] else None, bws.ptr(), S)
        finally:
            _lib.check(L.hig_enc_bwd_debug_tap(None, 0))

    refused_untouched(backward(True, tap.n - 256), grads, tap)
    _lib.check(backward(True))
    torch.cuda.synchronize()
    attention_launches(D, before)
    first = [grads.region.buf.clone(), dclip.buf.clone()]
    for r_ in (ws, bws, tap, xf_out, xf_proj, dclip, grads.region):
        assert r_.intact(), "a store landed in a guard band"
    assert (grads.words()[~grads.covered] == PAT32).all(), "a store landed between the gradients"

    # ---- the trace ----
    rows = (D.M, D.Lt)
    tr = {"gath": fview(ws, fw[_lib.TFW_GATH], (D.B, D.Lt)), "stf": fview(ws, fw[_lib.TFW_STF], (D.M, 2)), "xf_out": xf_out.view(0, rows, F32),
          "xf_proj": xf_proj.view(0, (D.B, D.E), F32), "dxf_total": fview(tap, tp[_lib.ETAP_DXF_TOTAL], rows), "dh0": fview(bws, bw[_lib.TBW_DB], rows)}
    x0 = fview(ws, fw[_lib.TFW_X0], rows)
    if D.pre:
        tr["x0"] = x0
    else:
        assert (x0.view(torch.int32) == PAT32).all(), "the identity pre-projection writes no x0"
    dgath = fview(tap, tp[_lib.ETAP_DGATH], (D.B, D.Lt))
    if dxp is not None:
        tr["dgath"] = dgath
        assert torch.equal(fview(bws, bw[_lib.TBW_DGATH], (D.B, D.Lt)), dgath), "what the backward leaves in dgath is what the tap saw"
    else:
        assert (dgath.view(torch.int32) == PAT32).all(), "no dxf_proj: nothing to tap in DGATH"
    if inp["want_dclip"]:
        tr["dclip"] = dclip.view(0, (D.M, D.W), F32)
    else:
        assert (dclip.buf == PAT16).all()
    layer_trace(tr, D, ws, fw, TFW, tap, tp)
    for k in grads.off:
        tr[k] = grads.view(k)
    finish("text %s %s" % (name, variant), tr, eb.TextWalk, P, D, inp)

    # ---- the same bits without the tap; the inference forward ----
    _lib.check(backward(False))
    torch.cuda.synchronize()
    assert torch.equal(grads.region.buf, first[0]) and torch.equal(dclip.buf, first[1]), "the backward without the tap gives other bits"
    xo2, xp2 = Region(D.M * D.Lt * 4), Region(D.B * D.E * 4)
    _lib.check(L.hig_text_head_fwd(C.byref(dims), ptab, _lib.ptr(clip), _lib.ptr(eot), xo2.ptr(), xp2.ptr(), iws.ptr(), 0, S))
    torch.cuda.synchronize()
    assert iws.intact() and xo2.intact() and xp2.intact(), "a store landed in a guard band of the inference forward"
    assert torch.equal(xo2.buf, xf_out.buf) and torch.equal(xp2.buf, xf_proj.buf), "the inference forward differs from the training forward"
    del keep


# ---- a capturing stream ---------------------------------------------------------------------------------------------------------
def test_a_capturing_stream_with_a_tap_set_is_refused():
    c, D, P, inp = eb.text_setup("pre", "all")
    L = _lib.lib()
    dims = _lib.TextDims(B=D.B, N=D.N, W=D.W, Lt=D.Lt, H=D.H, ff=D.ff, L=D.L, E=D.E, prec=_lib.PREC_F32)
    nb = [L.hig_text_head_workspace_bytes(C.byref(dims), 1), L.hig_text_head_bwd_workspace_bytes(C.byref(dims)), L.hig_text_head_bwd_tap_bytes(C.byref(dims))]
    ws, bws, tap = (torch.zeros(n, dtype=U8, device=DEV) for n in nb)
    grads = Grads(P)
    keep, ptab = param_table(P)
    gtab = grads.table()
    clip, eot, dxo, dxp = (inp[k].to(DEV).contiguous() for k in ("clip_out", "eot", "dxf_out", "dxf_proj"))
    xf_out, xf_proj = torch.zeros(D.M, D.Lt, device=DEV), torch.zeros(D.B, D.E, device=DEV)
    _lib.check(L.hig_text_head_fwd(C.byref(dims), ptab, _lib.ptr(clip), _lib.ptr(eot), _lib.ptr(xf_out), _lib.ptr(xf_proj), _lib.ptr(ws), 1, _lib.stream_ptr()))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    _lib.check(L.hig_enc_bwd_debug_tap(_lib.ptr(tap), nb[2]))
    try:
        with torch.cuda.graph(graph):
            rc = L.hig_text_head_bwd(C.byref(dims), ptab, _lib.ptr(clip), _lib.ptr(eot), _lib.ptr(xf_out), _lib.ptr(ws), _lib.ptr(dxo), _lib.ptr(dxp), gtab,
                                     None, _lib.ptr(bws), _lib.stream_ptr())
    finally:
        _lib.check(L.hig_enc_bwd_debug_tap(None, 0))
    assert rc == _lib.EINVAL and "capturing" in _lib.last_error()
    torch.cuda.synchronize()
    assert (grads.words() == PAT32).all() and not tap.any() and not bws.any()
    del keep
