"""The fp32-storage training step on the device, held stage by stage: one call each of hig_text_context and hig_denoiser_fwd
(training = 1) and hig_denoiser_bwd with the debug tap set (hig_denoiser_bwd_debug_tap), then EVERY buffer a launch of the three
wrote -- the saved activations and LayerNorm statistics, the text context, the tapped transients (d(a), dy, the d(scale, shift)
slices, dz1, every dh, dqkv, dA, dkv, dxfn, delta, each layer's W^T, dxf_out as it stands behind each layer), every parameter
gradient, out, dx, dxf_proj, dxf_out -- is held per element to the bound of the launch that wrote it, with that launch's operands
taken from the device's own buffers (tests/f32_step_bounds.py, `Walk` in check mode).  That the stages form the model is what
tests/test_cpu_f32_step_bounds.py shows; nothing here bounds the whole model.  dims.prec is HIG_PREC_F32 throughout.

Around the walk: the workspaces, the tap, the gradient table and the results start as a NaN pattern and sit between guard bands.
Production hands these calls torch.empty memory, so a read before the write, or a ragged last chunk that leaks the rows behind an
operand into a sum, is a real bug: here it surfaces as a NaN in a result that is held per element.  Every traced buffer must have
been written; the bands and the gaps between the groups of the gradient buffer must keep their bits.  REACH (the GEMM and attention
path counters the three calls move, the plan slots) is asserted per case.  A second backward without the tap, a second with it, and
one through hig_denoiser_bwd_hooked with a hook and a comm_stream reproduce the gradient table, dx, dxf_proj and dxf_out bit for bit
-- except the stylization `emb_layers.1.weight` rows (HIG_P_STY_EMB_W), which the hooked form computes per layer on the
weight-gradient stream (one split-free GEMM per layer instead of one at the end): they are held to their gemm32 stage bound.  With
and without the tap the same path counters move.  hig_denoiser_fwd_text (one call, the text side forked onto the third stream)
leaves the same bits in every traced forward buffer as the two separate calls.

The default eager backward forks every weight gradient onto a second stream; the switches are read once per process, so the
flipped forms run in child processes (tests/f32_step_worker.py), one at a time, each under its own time limit, none after one that
ended by a signal, an abort or its limit: HIG_BWD_OVERLAP=0 (one stream; small, pairs, rows520, full), HIG_TEXT_FORK=0 and
HIG_FWD_SPLIT=1 (small, pairs, rows520; no case has the 8192 rows at which the plan grants the split, which the child asserts).
Each child returns its worst ratios and a SHA-256 of every result; they must equal this process's (forked) results bit for bit:
the kernels and the per-stream order are the same and there are no float atomics.

Largest |error| / bound per stage kind on an MI355X (case and buffer that gave it; ('g', s) / ('gl', l, s): the gradient of slot
HIG_P_* s / of layer l's slot HIG_L_* s).  The flipped forms return the same bits as the default ones, hence the same ratios at the
cases they run (small, pairs, rows520, full); none reaches 0.9:
    stage kind      default forms (eight cases)            flipped forms (child processes)
    apply           0.093  narrow y1[0]                     0.062  rows520 HIG_BWD_OVERLAP=0 y1[0]
    apply_bwd       0.123  narrow ca_dA[0]                  0.058  pairs HIG_BWD_OVERLAP=0 int_dA[0]
    colsum          0.105  hd128 d(joint_embed.bias)        0.096  rows520 HIG_BWD_OVERLAP=0 d(joint_embed.bias)
    copy            0.000  (bit-equal everywhere)           0.000
    ctx             0.141  narrow kstc[0]                   0.116  pairs HIG_BWD_OVERLAP=0 ksti[1]
    ctx_bwd         0.108  pairs ca_dkv[0]                  0.108  pairs HIG_BWD_OVERLAP=0 ca_dkv[0]
    dsilu           0.640  full dte_h                       0.640  full HIG_BWD_OVERLAP=0 dte_h
    full            0.166  full lse1[0]                     0.166  full HIG_BWD_OVERLAP=0 lse1[0]
    full_bwd        0.031  full sa_dqkv[0]                  0.031  full HIG_BWD_OVERLAP=0 sa_dqkv[0]
    gemm32          0.445  full_hd128 ('g', 3)              0.439  small HIG_BWD_OVERLAP=0 ('g', 3)
    gemm32_dgelu    0.015  narrow ffn_dz[0]                 0.010  rows520 HIG_BWD_OVERLAP=0 ffn_dz[0]
    gemm32_gelu     0.011  narrow f1[0]                     0.010  rows520 HIG_BWD_OVERLAP=0 f1[0]
    gemm32_ln       0.034  narrow kv[0]                     0.025  pairs HIG_BWD_OVERLAP=0 kv[1]
    ln              0.083  narrow stt                       0.045  pairs HIG_BWD_OVERLAP=0 stt
    ln_bwd          0.223  full ('gl', 0, 11)               0.223  full HIG_BWD_OVERLAP=0 ('gl', 0, 11)
    ln_sty          0.113  narrow a3[0]                     0.076  rows520 HIG_BWD_OVERLAP=0 a1[0]
    temb            0.353  hd128 te                         0.341  pairs HIG_BWD_OVERLAP=0 te
    wgrad32         0.227  pairs ('g', 13)                  0.227  pairs HIG_BWD_OVERLAP=0 ('g', 13)
    xsum            0.193  narrow ('gl', 0, 15)             0.053  small HIG_BWD_OVERLAP=0 ('gl', 1, 3)
The gemm32 stages of the time path in the hooked form (where HIG_P_STY_EMB_W comes from one GEMM per layer): 0.445 at full_hd128.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_step_bounds as sb  # noqa: E402
import f32_step_bounds as fb  # noqa: E402
import test_gpu_attn_contract as AC  # noqa: E402
import test_gpu_gemm_contract as gm  # noqa: E402
from attn_dispatch_cases import PATHS as ATTN_PATHS  # noqa: E402
from gemm_dispatch_cases import PATHS as GEMM_PATHS  # noqa: E402
from hig_amd import _lib  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT16, PAT32 = 0x7FD5, 0x7FD57FD5
GUARD = 4096
F32, I64 = torch.float32, torch.int64


class Region:
    """nbytes of device memory between two guard bands, all of it the NaN pattern."""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.n = nbytes
        self.buf = torch.full(((nbytes + 2 * GUARD) // 2,), PAT16, dtype=torch.int16, device=DEV)

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD)

    def view(self, off, shape, dtype=F32):
        n = int(torch.tensor(shape).prod()) * torch.empty((), dtype=dtype).element_size()
        assert 0 <= off and off + n <= self.n, (off, n, self.n)
        return self.buf.view(torch.uint8)[GUARD + off:GUARD + off + n].view(dtype).view(shape)

    def intact(self):
        g = GUARD // 2
        return bool((self.buf[:g] == PAT16).all() and (self.buf[-g:] == PAT16).all())


def layout(dims, which, n):
    arr = (C.c_int64 * n)()
    assert _lib.lib().hig_f32_train_layout(C.byref(dims), which, arr, n) == n
    return list(arr)


def moved(before):
    torch.cuda.synchronize()
    g = {n: a - b for n, a, b in zip(GEMM_PATHS, gm.counts(), before[0]) if a != b}
    a = {n: a - b for n, a, b in zip(ATTN_PATHS, AC.counts(), before[1]) if a != b}
    return g, a


def counters():
    torch.cuda.synchronize()
    return gm.counts(), AC.counts()


def run_case(name, repeats=True, one_call=False):
    """One step of case `name` -> {'worst': {kind: (ratio, buffer)}, 'sched': ..., 'paths': ..., 'sha': {result: sha256}}."""
    c = fb.CASES[name]
    D = fb.Dims(c)
    m = fb.build_model(c, DEV).train()
    assert m.precision == "f32" and m.storage == "f32"
    P = sb.Params(m)
    inp = fb.case_inputs(c)
    Lb, L, S = _lib, _lib.lib(), _lib.stream_ptr()
    dims = m.dims(D.B, D.T, D.N)
    fp = m.flat_params()
    ptab, gtab = fp.param_table(), fp.ensure_grad()
    fw, tx = layout(dims, Lb.LAYOUT32_FWD, Lb.FW32_NSLOTS), layout(dims, Lb.LAYOUT32_TEXT, Lb.TX32_NSLOTS)
    bw, tp = layout(dims, Lb.LAYOUT32_BWD, Lb.BW32_NSLOTS), layout(dims, Lb.LAYOUT32_TAP, Lb.TAP32_NSLOTS)
    assert fw[Lb.FW32_TOTAL] == L.hig_workspace_bytes(C.byref(dims), 1) and tx[Lb.TX32_TOTAL] == L.hig_textctx_bytes(C.byref(dims), 1)
    assert bw[Lb.BW32_TOTAL] == L.hig_bwd_workspace_bytes(C.byref(dims)) and tp[Lb.TAP32_TOTAL] == L.hig_denoiser_bwd_tap_bytes(C.byref(dims))
    ws, tc, bws, tap = Region(fw[Lb.FW32_TOTAL]), Region(tx[Lb.TX32_TOTAL]), Region(bw[Lb.BW32_TOTAL]), Region(tp[Lb.TAP32_TOTAL])
    res = {k: Region(n * 4) for k, n in (("out", D.M * D.F), ("dx", D.M * D.F), ("dxf_proj", D.B * D.E), ("dxf_out", D.Mt * D.Lt))}
    g = {k: inp[k].to(DEV).contiguous() for k in ("x", "t", "length", "xf_proj", "xf_out")}
    d = D.d
    paths = {}

    # ---- the forward entries ----
    def forward(ws_, tc_, out_, fused):
        before = counters()
        if fused:
            _lib.check(L.hig_denoiser_fwd_text(C.byref(dims), ptab, _lib.ptr(g["x"]), _lib.ptr(g["t"]), _lib.ptr(g["length"]), _lib.ptr(g["xf_proj"]),
                                               _lib.ptr(g["xf_out"]), tc_.ptr(), out_.ptr(), ws_.ptr(), 1, S))
            sched = _lib.denoiser_last_schedule()
        else:
            _lib.check(L.hig_text_context(C.byref(dims), ptab, _lib.ptr(g["xf_out"]), tc_.ptr(), 1, S))
            assert _lib.denoiser_last_schedule()["entry"] == Lb.DN_ENTRY_TEXT32
            _lib.check(L.hig_denoiser_fwd(C.byref(dims), ptab, _lib.ptr(g["x"]), _lib.ptr(g["t"]), _lib.ptr(g["length"]), _lib.ptr(g["xf_proj"]),
                                          tc_.ptr(), out_.ptr(), ws_.ptr(), 1, S))
            sched = _lib.denoiser_last_schedule()
        assert sched["entry"] == Lb.DN_ENTRY_FWD32 and not sched["fuse_apply"] and not sched["fold32"]
        return sched, moved(before)

    sched_f, paths["fwd"] = forward(ws, tc, res["out"], one_call)
    out = res["out"].view(0, (D.B, D.T, D.F))
    assert torch.isfinite(out).all(), "not every element of out was written"
    inp["dout"] = fb.masked_mse_grad(out.cpu(), inp["target"], inp["length"])
    dout = inp["dout"].to(DEV).contiguous()
    gbits = fp.grad.view(torch.int32)
    covered = torch.zeros(fp.grad.numel(), dtype=torch.bool, device=DEV)
    for p, o in zip(fp.params, fp.offsets):
        covered[o:o + p.numel()] = True
    bargs = (C.byref(dims), ptab, _lib.ptr(g["x"]), _lib.ptr(g["t"]), _lib.ptr(g["length"]), _lib.ptr(g["xf_out"]), tc.ptr(), ws.ptr(), _lib.ptr(dout),
             gtab, res["dx"].ptr(), res["dxf_proj"].ptr(), res["dxf_out"].ptr(), bws.ptr(), S)

    def backward(with_tap, hooked=False):
        gbits.fill_(PAT32)
        for k in ("dx", "dxf_proj", "dxf_out"):
            res[k].buf.fill_(PAT16)
        bws.buf.fill_(PAT16)
        tap.buf.fill_(PAT16)
        before = counters()
        _lib.check(L.hig_denoiser_bwd_debug_tap(tap.ptr() if with_tap else None, tap.n))
        try:
            if hooked:
                seen = []
                cb = _lib.LAYER_HOOK(lambda user, layer: seen.append(int(layer)))
                comm = torch.cuda.Stream()
                _lib.check(L.hig_denoiser_bwd_hooked(*bargs, cb, None, C.c_void_p(comm.cuda_stream)))
                assert seen == list(range(D.L - 1, -1, -1))
            else:
                _lib.check(L.hig_denoiser_bwd(*bargs))
        finally:
            _lib.check(L.hig_denoiser_bwd_debug_tap(None, 0))
        mv = moved(before)
        assert (gbits[~covered] == PAT32).all(), "a store landed between the groups of the gradient buffer"
        assert torch.isfinite(fp.grad[covered]).all(), "not every parameter gradient was written"
        assert with_tap or (tap.buf == PAT16).all()
        return [fp.grad.clone()] + [res[k].buf.clone() for k in ("dx", "dxf_proj", "dxf_out")] + [tap.buf.clone()], mv

    # a short tap is refused before any launch: nothing is written
    _lib.check(L.hig_denoiser_bwd_debug_tap(tap.ptr(), tap.n - 256))
    gbits.fill_(PAT32)
    rc = L.hig_denoiser_bwd(*bargs)
    _lib.check(L.hig_denoiser_bwd_debug_tap(None, 0))
    torch.cuda.synchronize()
    assert rc == Lb.EINVAL and str(tap.n) in _lib.last_error() and (gbits == PAT32).all() and (tap.buf == PAT16).all()

    first, paths["bwd"] = backward(True)
    sched_b = _lib.denoiser_last_schedule()
    assert sched_b["entry"] == Lb.DN_ENTRY_BWD32
    for r_ in [ws, tc, bws, tap] + list(res.values()):
        assert r_.intact(), "a store landed in a guard band"

    # ---- the trace ----
    tr = {}
    ctx, kst, lse = (D.B, D.H, D.hd, D.hd), (D.B, D.H, D.hd, 2), (D.B, D.H, D.T)
    rows, wide, st, ffs = (D.M, d), (D.M, 3 * d), (D.M, 2), (D.M, D.ff)
    for key, slot, shape in (("te", Lb.FW32_TE, (D.B, d)), ("te_h", Lb.FW32_TE_H, (D.B, D.E)), ("emb", Lb.FW32_EMB, (D.B, D.E)),
                             ("ss", Lb.FW32_SS, (D.B, D.ss_ld)), ("h0", Lb.FW32_H0, rows)):
        tr[key] = ws.view(fw[slot], shape)
    per_layer = [("st1", Lb.FW32_ST1, st), ("xn1", Lb.FW32_XN1, rows), ("qkv", Lb.FW32_QKV, wide), ("y1", Lb.FW32_Y1, rows), ("st2", Lb.FW32_ST2, st),
                 ("a1", Lb.FW32_A1S, rows), ("h1", Lb.FW32_H1, rows), ("st3", Lb.FW32_ST3, st), ("xn2", Lb.FW32_XN2, rows), ("qc", Lb.FW32_QC, rows),
                 ("y2", Lb.FW32_Y2, rows), ("st4", Lb.FW32_ST4, st), ("a2", Lb.FW32_A2S, rows), ("h2", Lb.FW32_H2, rows), ("z1", Lb.FW32_Z1, ffs),
                 ("f1", Lb.FW32_F1, ffs), ("y3", Lb.FW32_Y3, rows), ("st5", Lb.FW32_ST5, st), ("a3", Lb.FW32_A3S, rows), ("h3", Lb.FW32_H3, rows)]
    per_layer += [("lse1", Lb.FW32_LSE1, lse), ("lse2", Lb.FW32_LSE2, lse)] if D.full else [("A1", Lb.FW32_A1, ctx), ("kst1", Lb.FW32_KST1, kst)]
    if D.inter:
        per_layer += [("st6", Lb.FW32_ST6, st), ("xn3", Lb.FW32_XN3, rows), ("iqkv", Lb.FW32_IQKV, wide), ("Ai", Lb.FW32_AI, ctx), ("ksti", Lb.FW32_KSTI, kst),
                      ("y4", Lb.FW32_Y4, rows), ("st7", Lb.FW32_ST7, st), ("a4", Lb.FW32_A4S, rows), ("h2b", Lb.FW32_H2B, rows)]
    if D.two:
        lenp = ws.view(fw[Lb.FW32_LENP], (D.B,), I64)
        assert torch.equal(lenp.cpu(), sb.swap_halves(inp["length"])), "the partner lengths are not the swapped lengths"
    sl = (D.B, 2 * d)
    wt_n = ((11 if D.inter else 7) * d * d + 2 * d * D.ff + 2 * d * D.Lt,)
    tap_layer = [("wT", Lb.TAP32_WT, wt_n)]
    blocks = [("ffn", Lb.TAP32_FFN_T1), ("ca", Lb.TAP32_CA_T1), ("sa", Lb.TAP32_SA_T1)] + ([("int", Lb.TAP32_INT_T1)] if D.inter else [])
    for pre, s0 in blocks:
        tap_layer += [(pre + "_t1", s0, rows), (pre + "_dy", s0 + 1, rows), (pre + "_dss", s0 + 2, sl)]
    tap_layer += [("ffn_dz", Lb.TAP32_FFN_DZ, ffs), ("ffn_dh", Lb.TAP32_FFN_DH, rows), ("ca_dq", Lb.TAP32_CA_DQ, rows), ("ca_t2", Lb.TAP32_CA_T2, rows),
                  ("ca_dh", Lb.TAP32_CA_DH, rows), ("ca_dkv", Lb.TAP32_CA_DKV, (D.Mt, 2 * d)), ("ca_dxfn", Lb.TAP32_CA_DXFN, (D.Mt, D.Lt)),
                  ("ca_dxf_out", Lb.TAP32_CA_DXF_OUT, (D.Mt, D.Lt)), ("sa_dqkv", Lb.TAP32_SA_DQKV, wide), ("sa_t2", Lb.TAP32_SA_T2, rows),
                  ("sa_dh", Lb.TAP32_SA_DH, rows)]
    tap_layer += [("ca_delta", Lb.TAP32_CA_DELTA, lse), ("sa_delta", Lb.TAP32_SA_DELTA, lse)] if D.full else [("ca_dA", Lb.TAP32_CA_DA, ctx),
                                                                                                                 ("sa_dA", Lb.TAP32_SA_DA, ctx)]
    if D.inter:
        tap_layer += [("int_dqkv", Lb.TAP32_INT_DQKV, wide), ("int_dA", Lb.TAP32_INT_DA, ctx), ("int_t2", Lb.TAP32_INT_T2, rows),
                      ("int_dh", Lb.TAP32_INT_DH, rows)]
    fwd_keys = ["te", "te_h", "emb", "ss", "h0", "stt"]
    tr["stt"] = tc.view(tx[Lb.TX32_STT], (D.Mt, 2))
    for l in range(D.L):
        base = fw[Lb.FW32_LAYER0] + fw[Lb.FW32_LSTRIDE] * l
        for key, slot, shape in per_layer:
            tr[(key, l)] = ws.view(base + fw[slot], shape)
        tr[("kv", l)] = tc.view(tx[Lb.TX32_KV] + tx[Lb.TX32_KV_STRIDE] * l, (D.Mt, 2 * d))
        if not D.full:
            tbase = tx[Lb.TX32_LAYER0] + tx[Lb.TX32_LSTRIDE] * l
            tr[("Ac", l)], tr[("kstc", l)] = tc.view(tbase + tx[Lb.TX32_AC], ctx), tc.view(tbase + tx[Lb.TX32_KSTC], kst)
        fwd_keys += [(k_, l) for k_, _, _ in per_layer] + [("kv", l)] + ([] if D.full else [("Ac", l), ("kstc", l)])
        pbase = tp[Lb.TAP32_LAYER0] + tp[Lb.TAP32_LSTRIDE] * l
        for key, slot, shape in tap_layer:
            tr[(key, l)] = tap.view(pbase + tp[slot], shape)
    once = [("dhL", Lb.TAP32_DHL, rows), ("dtmp_emb", Lb.TAP32_DTMP_EMB, (D.B, D.E)), ("dtmp_te", Lb.TAP32_DTMP_TE, (D.B, D.E))]
    if D.two:
        once += [("doutm", Lb.TAP32_DOUTM, (D.M, D.F)), ("tok0g", Lb.TAP32_TOK0, (D.B, d)), ("postmp", Lb.TAP32_POSTMP, (D.T, d))]
    for key, slot, shape in once:
        tr[key] = tap.view(tp[slot], shape)
    for key, slot, shape in (("dss", Lb.BW32_DSS, (D.B, D.ss_ld)), ("demb", Lb.BW32_DEMB, (D.B, D.E)), ("dte_h", Lb.BW32_DTE_H, (D.B, D.E))):
        tr[key] = bws.view(bw[slot], shape)
    for s_, t_ in enumerate(P.glob):
        if t_ is not None:
            o = fp.group_offsets[s_]
            tr[("g", s_)] = fp.grad[o:o + t_.numel()].view(t_.shape)
    for l in range(D.L):
        for s_, t_ in enumerate(P.lay[l]):
            if t_ is not None:
                o = fp.group_offsets[Lb.NGLOBAL + l * Lb.NLAYER + s_]
                tr[("gl", l, s_)] = fp.grad[o:o + t_.numel()].view(t_.shape)
    tr["out"] = res["out"].view(0, (D.M, D.F))
    tr["dx"] = res["dx"].view(0, (D.M, D.F))
    tr["dxf_proj"] = res["dxf_proj"].view(0, (D.B, D.E))
    tr["dxf_out"] = res["dxf_out"].view(0, (D.Mt, D.Lt))
    for key, t_ in tr.items():
        assert torch.isfinite(t_).all(), "%s: not every element was written (or a NaN of the unwritten workspace was read)" % (key,)
    dev_tr = tr
    tr = {k: v.cpu() for k, v in tr.items()}

    walk = fb.Walk(P, D, inp, fb.REF, trace=tr).run()
    assert walk.seen == set(tr), walk.seen ^ set(tr)
    assert walk.spread <= 80
    sha = {k: hashlib.sha256(t_.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
           for k, t_ in (("grad", first[0]), ("out", res["out"].buf), ("dx", first[1]), ("dxf_proj", first[2]), ("dxf_out", first[3]))}

    if repeats:
        again, mv_a = backward(False)
        tapped, mv_t = backward(True)
        assert mv_a == paths["bwd"] == mv_t, "the tap changes which kernels run: %s / %s / %s" % (paths["bwd"], mv_a, mv_t)
        for i, (a, b_, t_) in enumerate(zip(first, again, tapped)):
            assert i == 4 or torch.equal(a.view(torch.int16), b_.view(torch.int16)), "the backward without the tap gives other bits (%d)" % i
            assert torch.equal(a.view(torch.int16), t_.view(torch.int16)), "a second backward with the tap gives other bits (%d)" % i
        hooked, _ = backward(False, hooked=True)
        o = fp.group_offsets[Lb.P_STY_EMB_W]
        n = P.glob[Lb.P_STY_EMB_W].numel()
        same = torch.ones(first[0].numel(), dtype=torch.bool, device=DEV)
        same[o:o + n] = False
        assert torch.equal(first[0].view(torch.int32)[same], hooked[0].view(torch.int32)[same]), "the hooked backward gives other gradient bits"
        for a, h in zip(first[1:4], hooked[1:4]):
            assert torch.equal(a.view(torch.int16), h.view(torch.int16)), "the hooked backward gives other bits"
        # HIG_P_STY_EMB_W: one GEMM per layer in the hooked form: held to its stage bound
        tr_h = dict(tr)
        tr_h[("g", Lb.P_STY_EMB_W)] = hooked[0][o:o + n].view(P.glob[Lb.P_STY_EMB_W].shape).cpu()
        ck = fb.Walk(P, D, inp, fb.REF, trace=tr_h)
        ck.time_path_bwd()
        assert all(v[0] <= 1.0 for v in ck.worst.values()), ck.worst
        walk.worst["gemm32 (hooked, time path)"] = max(((r_, k_) for kind, (r_, k_) in ck.worst.items() if kind == "gemm32"), key=lambda v: v[0])
        # the text side forked inside one call (hig_denoiser_fwd_text) leaves the same bits
        if not one_call:
            ws2, tc2, out2 = Region(ws.n), Region(tc.n), Region(res["out"].n)
            sched2, _ = forward(ws2, tc2, out2, True)
            assert ws2.intact() and tc2.intact() and out2.intact()
            assert torch.equal(out2.buf, res["out"].buf), "hig_denoiser_fwd_text gives other bits in out"
            for key in fwd_keys:
                src = dev_tr[key]
                reg, reg2 = (tc, tc2) if (key == "stt" or (isinstance(key, tuple) and key[0] in ("kv", "Ac", "kstc"))) else (ws, ws2)
                off = src.data_ptr() - reg.buf.data_ptr() - GUARD
                assert torch.equal(reg2.view(off, tuple(src.shape)), src), "hig_denoiser_fwd_text gives other bits in %s" % (key,)
            paths["text_fork"] = sched2["text_fork"]
    return {"worst": walk.worst, "sched_f": sched_f, "sched_b": sched_b, "paths": paths, "sha": sha}


def held(name, r, tag=""):
    for kind, (ratio, key) in sorted(r["worst"].items()):
        print("RATIO %s%s | %s | %.3f | %s" % (name, tag, kind, ratio, key))
    bad = {k: v for k, v in r["worst"].items() if not v[0] <= 1.0}
    assert not bad, "%s%s: stages beyond their bound: %s" % (name, tag, bad)


RESULTS = {}


@pytest.mark.parametrize("name", list(fb.CASES))
def test_every_stage_of_the_step_within_its_bound(name):
    r = RESULTS[name] = run_case(name)
    print("PATHS %s %s" % (name, json.dumps(r["paths"], sort_keys=True)))
    print("SHA %s %s" % (name, json.dumps(r["sha"], sort_keys=True)))
    held(name, r)
    # the default eager backward forks the weight gradients; a training forward never fuses the attention front nor folds LayerNorm
    assert r["sched_b"]["wgrad_fork"] == 1 and not r["sched_f"]["split"], (r["sched_b"], r["sched_f"])
    assert r["paths"].get("text_fork") == 1
    fb.assert_reach(name, r["paths"])


CHILDREN = (("HIG_BWD_OVERLAP", "0", ("small", "pairs", "rows520", "full")), ("HIG_TEXT_FORK", "0", ("small", "pairs", "rows520")),
            ("HIG_FWD_SPLIT", "1", ("small", "pairs", "rows520")))
STOP = []           # set once a child ended by a signal, an abort or its time limit: no further child is started


def child(knob, value, cases):
    if STOP:
        return {"error": "not started: %s" % STOP[0]}
    env = dict(os.environ, OMP_NUM_THREADS="4", **{knob: value})
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "f32_step_worker.py")] + list(cases)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        STOP.append("the %s=%s child ended with status %d" % (knob, value, r.returncode))
    if r.returncode != 0:
        return {"error": "status %d\n" % r.returncode + r.stdout[-2000:] + r.stderr[-2000:]}
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("STEP ")][-1][len("STEP "):])


@pytest.mark.parametrize("knob,value,cases", CHILDREN)
def test_the_flipped_forms_give_the_same_bits_within_the_same_bounds(knob, value, cases):
    res = child(knob, value, cases)
    assert "error" not in res, res["error"]
    for name in cases:
        r = res[name]
        held(name, {"worst": {k: tuple(v) for k, v in r["worst"].items()}}, " %s=%s" % (knob, value))
        if knob == "HIG_BWD_OVERLAP":
            assert r["sched_b"]["wgrad_fork"] == 0
        if knob == "HIG_TEXT_FORK":
            assert r["sched_f"]["text_fork"] == 0
        if knob == "HIG_FWD_SPLIT":
            assert r["sched_f"]["split"] == 0, "no case has the rows at which the plan grants the split"
        if name not in RESULTS:
            RESULTS[name] = run_case(name, repeats=False)
        assert r["sha"] == RESULTS[name]["sha"], "%s=%s: %s gives other bits than the default forms: %s" % (
            knob, value, name, [k for k in r["sha"] if r["sha"][k] != RESULTS[name]["sha"][k]])


def test_a_capturing_stream_with_a_tap_set_is_refused():
    c = fb.CASES["small"]
    D = fb.Dims(c)
    m = fb.build_model(c, DEV).train()
    inp = fb.case_inputs(c)
    gi = {k: inp[k].to(DEV) for k in ("x", "t", "length", "xf_proj", "xf_out")}
    dims = m.dims(D.B, D.T, D.N)
    L = _lib.lib()
    fp = m.flat_params()
    n = L.hig_denoiser_bwd_tap_bytes(C.byref(dims))
    tapbuf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    bufs = [torch.zeros(k, dtype=torch.uint8, device=DEV) for k in (L.hig_workspace_bytes(C.byref(dims), 1), L.hig_textctx_bytes(C.byref(dims), 1),
                                                                    L.hig_bwd_workspace_bytes(C.byref(dims)))]
    dout, dxp, dxo = torch.zeros_like(gi["x"]), torch.zeros(D.B, D.E, device=DEV), torch.zeros(D.B, D.N, D.Lt, device=DEV)
    ptab, gtab = fp.param_table(), fp.ensure_grad()
    before = fp.grad.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    _lib.check(L.hig_denoiser_bwd_debug_tap(_lib.ptr(tapbuf), n))
    try:
        with torch.cuda.graph(graph):
            rc = L.hig_denoiser_bwd(C.byref(dims), ptab, _lib.ptr(gi["x"]), _lib.ptr(gi["t"]), _lib.ptr(gi["length"]), _lib.ptr(gi["xf_out"]),
                                    _lib.ptr(bufs[1]), _lib.ptr(bufs[0]), _lib.ptr(dout), gtab, None, _lib.ptr(dxp), _lib.ptr(dxo), _lib.ptr(bufs[2]),
                                    _lib.stream_ptr())
    finally:
        _lib.check(L.hig_denoiser_bwd_debug_tap(None, 0))
    assert rc == _lib.EINVAL and "capturing" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(fp.grad, before) and not tapbuf.any()
