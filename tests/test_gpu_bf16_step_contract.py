"""The bf16-storage training step on the device, held stage by stage: one call each of hig_text_context_bf16_train,
hig_denoiser_fwd_bf16_train and hig_denoiser_bwd_bf16 (with the debug tap set), then EVERY buffer a launch of the three wrote --
the saved activations, the text context, the tapped gradients, every parameter gradient, out, dx, dxf_proj, dxf_out -- is held
per element to the bound of the launch that wrote it, with that launch's operands taken from the device's own buffers
(tests/bf16_step_bounds.py, `Walk` in check mode).  That the stages form the model is what tests/test_cpu_bf16_step_bounds.py
shows; nothing here bounds the whole model.

Around the walk, in the manner of `Guarded`: the workspaces, the tap and the results start as a NaN pattern (0x7FD5 in every
16-bit half: a NaN as bf16 and as fp32) and sit between guard bands; every traced buffer must have been written, the bands and
the gaps of the gradient buffer must keep their bits.  The rows M .. Mp of a weight gradient's operands are whatever follows the
operand in the workspace (the kernels read the row-major operands with a ragged last chunk, nothing is padded): a leak would add
terms to a gradient that is held per element.  The At16 copies equal at16_order of the device's own A, the partner lengths are
the swapped lengths, and hig_denoiser_last_schedule / hig_gemm_bf16_plan report the forms each case is meant to reach.  A second
backward without the tap and one through hig_denoiser_bwd_bf16_hooked reproduce the gradient table, dx, dxf_proj and dxf_out bit
for bit.  The flipped forms (HIG_BWD_OVERLAP=1, HIG_EDGE16=0, HIG_FUSE_APPLY=0, HIG_CTX16=0: read once per process) run the cases
`small`, `pairs` and `fused` in child processes (tests/bf16_step_worker.py); `fused` is where the last two change the form.

Largest |error| / bound per stage kind on an MI355X (case that gave it); a bf16 result reaches 1.000 by construction where the
fp32 bound is small against half an ulp:
    stage kind     default forms                          flipped forms (child processes)
    apply          0.999  wsp16 y2[0]                     0.999  fused HIG_BWD_OVERLAP=1 y1[0]
    apply_bwd      0.491  wsp16 ca_dA[0]                  0.424  small HIG_CTX16=0 ca_dA[0]
    colsum         0.094  wsp16 d(time_embed.0.bias)      0.083  pairs HIG_CTX16=0 d(stylization bias)
    copy           0.000  (bit-equal everywhere)          0.000
    ctx            0.933  wsp16 Ac[0]                     0.905  fused HIG_BWD_OVERLAP=1 Ac[1]
    ctx_bwd        0.599  wsp16 ca_dkv[0]                 0.606  fused HIG_FUSE_APPLY=0 ca_dkv[0]
    dsilu          0.618  pairs dte_h                     0.636  pairs HIG_CTX16=0 dte_h
    edge           0.999  pairs d(h_L)                    0.999  pairs HIG_BWD_OVERLAP=1 d(h_L)
    gelu           0.982  hd128 f1[1]                     0.982  pairs HIG_CTX16=0 f1[1]
    gemm16         0.997  small kv[0]                     0.997  small HIG_BWD_OVERLAP=1 kv[0]
    gemm16_dgelu   0.492  pairs ffn_dz[0]                 0.492  pairs HIG_BWD_OVERLAP=1 ffn_dz[0]
    gemm16_gelu    0.463  wsp16 f1[0]                     (the single-launch FFN is reached at 2156 rows only)
    gemm32         0.469  fused d(time_embed.0.weight)    0.476  fused HIG_FUSE_APPLY=0 d(time_embed.0.weight)
    joint          1.000  d192 h0                         1.000  pairs HIG_BWD_OVERLAP=1 h0
    ln             0.999  pairs xfn[1]                    0.999  pairs HIG_BWD_OVERLAP=1 xfn[1]
    ln_bwd         1.000  small ca_dh[1]                  1.000  small HIG_BWD_OVERLAP=1 ca_dh[1]
    ln_sty         0.999  pairs a4[0]                     0.999  pairs HIG_BWD_OVERLAP=1 a4[0]
    temb           0.416  wsp16 te                        0.341  pairs HIG_BWD_OVERLAP=1 te
    wgrad16        0.013  d192 d(ca proj_out bias)[1]     0.013  fused HIG_EDGE16=0 d(sa qkv bias)[0]
`gelu` at 0.982 is the tail term of the bf16 GELU beyond |z| = 6.5 nearly attained (the FFN pre-activations of layer 1 reach
there); without that term of include/hig.h the ratio was 1e9 and more at five of the six cases.  The forms the plans choose:
only `wsp16` (H = 8, 2156 rows) and `fused` (H = 4, M = 98) fuse the attention front and run the F-wide edges on the bf16
matrix cores; the four small cases (H = 2 or 3; hig_edge16_layout does not fit into M d floats) take the unfused pair and the
fp32 edge whatever HIG_FUSE_APPLY and HIG_EDGE16 say, so those two switches change the form at `fused` alone.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_step_bounds as sb  # noqa: E402
import linattn16_bounds as lb  # noqa: E402
from gemm_dispatch_cases import GELU, fake_desc, plan  # noqa: E402
from hig_amd import _lib  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT16, PAT32 = 0x7FD5, 0x7FD57FD5
GUARD = 4096
BF16, F32, I64 = torch.bfloat16, torch.float32, torch.int64
FLIPPED = (("HIG_BWD_OVERLAP", "1", "wgrad_fork", 1), ("HIG_EDGE16", "0", "edge16", 0), ("HIG_FUSE_APPLY", "0", "fuse_front", 0),
           ("HIG_CTX16", "0", "ctx_mm16", 0))


class Region:
    """nbytes of device memory between two guard bands, all of it the NaN pattern."""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.n = nbytes
        self.buf = torch.full(((nbytes + 2 * GUARD) // 2,), PAT16, dtype=torch.int16, device=DEV)

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD)

    def view(self, off, shape, dtype):
        n = int(torch.tensor(shape).prod()) * torch.empty((), dtype=dtype).element_size()
        assert 0 <= off and off + n <= self.n, (off, n, self.n)
        return self.buf.view(torch.uint8)[GUARD + off:GUARD + off + n].view(dtype).view(shape)

    def intact(self):
        g = GUARD // 2
        return bool((self.buf[:g] == PAT16).all() and (self.buf[-g:] == PAT16).all())


def layout(dims, which, n):
    arr = (C.c_int64 * n)()
    assert _lib.lib().hig_bf16_train_layout(C.byref(dims), which, arr, n) == n
    return list(arr)


def schedule():
    arr = (C.c_int32 * _lib.DN_PLAN_NSLOTS)()
    entry = _lib.lib().hig_denoiser_last_schedule(arr, _lib.DN_PLAN_NSLOTS)
    return entry, dict(zip(_lib.DN_PLAN_SLOTS, arr))


def run_case(name, repeats=True):
    """One step of case `name` -> {'worst': {kind: (ratio, buffer)}, 'forms': ..., 'wgrad_fork': ...}."""
    c = sb.CASES[name]
    D = sb.Dims(c)
    m = sb.build_model(c, DEV, storage="bf16").train()
    P = sb.Params(m)
    inp = sb.case_inputs(c)
    L, S = _lib.lib(), _lib.stream_ptr()
    dims = m.dims(D.B, D.T, D.N)
    fp = m.flat_params()
    ptab, s16 = fp.param_table(), fp.shadow16(m._param_version())
    gtab = fp.ensure_grad()
    fw = layout(dims, _lib.LAYOUT16_FWD, _lib.FW16_NSLOTS)
    tx = layout(dims, _lib.LAYOUT16_TEXT, _lib.TX16_NSLOTS)
    bw = layout(dims, _lib.LAYOUT16_BWD, _lib.BW16_NSLOTS)
    tp = layout(dims, _lib.LAYOUT16_TAP, _lib.TAP16_NSLOTS)
    assert fw[_lib.FW16_TOTAL] == L.hig_workspace_bytes(C.byref(dims), 1) and tx[_lib.TX16_TOTAL] == L.hig_textctx_bytes(C.byref(dims), 1)
    assert bw[_lib.BW16_TOTAL] == L.hig_bwd_workspace_bytes(C.byref(dims)) and tp[_lib.TAP16_TOTAL] == L.hig_denoiser_bwd_bf16_tap_bytes(C.byref(dims))
    assert bw[_lib.BW16_MP] == (D.M + 63) // 64 * 64 and bw[_lib.BW16_MTP] == (D.Mt + 63) // 64 * 64
    ws, tc, bws, tap = Region(fw[_lib.FW16_TOTAL]), Region(tx[_lib.TX16_TOTAL]), Region(bw[_lib.BW16_TOTAL]), Region(tp[_lib.TAP16_TOTAL])
    res = {k: Region(n * 4) for k, n in (("out", D.M * D.F), ("dx", D.M * D.F), ("dxf_proj", D.B * D.E), ("dxf_out", D.Mt * D.Lt))}
    g = {k: inp[k].to(DEV).contiguous() for k in ("x", "t", "length", "xf_proj", "xf_out")}
    d = D.d

    # ---- the three entries ----
    _lib.check(L.hig_text_context_bf16_train(C.byref(dims), ptab, s16, _lib.ptr(g["xf_out"]), tc.ptr(), S))
    e, sched_t = schedule()
    assert e == _lib.DN_ENTRY_TEXT16
    _lib.check(L.hig_denoiser_fwd_bf16_train(C.byref(dims), ptab, s16, _lib.ptr(g["x"]), _lib.ptr(g["t"]), _lib.ptr(g["length"]), _lib.ptr(g["xf_proj"]),
                                             tc.ptr(), res["out"].ptr(), ws.ptr(), S))
    e, sched_f = schedule()
    assert e == _lib.DN_ENTRY_FWD16_TRAIN and sched_f["ctx_mm16"] == sched_t["ctx_mm16"]
    out = res["out"].view(0, (D.B, D.T, D.F), F32)
    assert torch.isfinite(out).all(), "not every element of out was written"
    inp["dout"] = sb.masked_mse_grad(out.cpu(), inp["target"], inp["length"])
    dout = inp["dout"].to(DEV).contiguous()
    gbits = fp.grad.view(torch.int32)
    covered = torch.zeros(fp.grad.numel(), dtype=torch.bool, device=DEV)
    for p, o in zip(fp.params, fp.offsets):
        covered[o:o + p.numel()] = True

    def backward(with_tap, hooked=False):
        gbits.fill_(PAT32)
        for k in ("dx", "dxf_proj", "dxf_out"):
            res[k].buf.fill_(PAT16)
        bws.buf.fill_(PAT16)
        _lib.check(L.hig_denoiser_bwd_bf16_debug_tap(tap.ptr() if with_tap else None, tap.n))
        args = (C.byref(dims), ptab, s16, _lib.ptr(g["x"]), _lib.ptr(g["t"]), _lib.ptr(g["length"]), _lib.ptr(g["xf_out"]), tc.ptr(), ws.ptr(),
                _lib.ptr(dout), gtab, res["dx"].ptr(), res["dxf_proj"].ptr(), res["dxf_out"].ptr(), bws.ptr(), S)
        try:
            if hooked:
                seen = []
                cb = _lib.LAYER_HOOK(lambda user, layer: seen.append(int(layer)))
                _lib.check(L.hig_denoiser_bwd_bf16_hooked(*args, cb, None, None))
                assert seen == list(range(D.L - 1, -1, -1))
            else:
                _lib.check(L.hig_denoiser_bwd_bf16(*args))
        finally:
            _lib.check(L.hig_denoiser_bwd_bf16_debug_tap(None, 0))
        torch.cuda.synchronize()
        assert (gbits[~covered] == PAT32).all(), "a store landed between the groups of the gradient buffer"
        assert torch.isfinite(fp.grad[covered]).all(), "not every parameter gradient was written"
        return [fp.grad.clone()] + [res[k].buf.clone() for k in ("dx", "dxf_proj", "dxf_out")]

    # a short tap is refused before any launch: nothing is written
    _lib.check(L.hig_denoiser_bwd_bf16_debug_tap(tap.ptr(), tap.n - 256))
    gbits.fill_(PAT32)
    rc = L.hig_denoiser_bwd_bf16(C.byref(dims), ptab, s16, _lib.ptr(g["x"]), _lib.ptr(g["t"]), _lib.ptr(g["length"]), _lib.ptr(g["xf_out"]), tc.ptr(),
                                 ws.ptr(), _lib.ptr(dout), gtab, res["dx"].ptr(), res["dxf_proj"].ptr(), res["dxf_out"].ptr(), bws.ptr(), S)
    _lib.check(L.hig_denoiser_bwd_bf16_debug_tap(None, 0))
    torch.cuda.synchronize()
    assert rc == _lib.EINVAL and (gbits == PAT32).all() and (tap.buf == PAT16).all()

    first = backward(True)
    e, sched_b = schedule()
    assert e == _lib.DN_ENTRY_BWD16
    for r_ in [ws, tc, bws, tap] + list(res.values()):
        assert r_.intact(), "a store landed in a guard band"

    # ---- the trace ----
    tr = {}
    ctx = (D.B, D.H, D.hd, D.hd)
    rows, wide, kst = (D.M, d), (D.M, 3 * d), (D.B, D.H, D.hd, 2)
    for key, slot, shape, dt in (("te", _lib.FW16_TE, (D.B, d), F32), ("te_h", _lib.FW16_TE_H, (D.B, D.E), F32), ("emb", _lib.FW16_EMB, (D.B, D.E), F32),
                                 ("ss", _lib.FW16_SS, (D.B, D.ss_ld), F32), ("h0", _lib.FW16_H0, rows, BF16)):
        tr[key] = ws.view(fw[slot], shape, dt)
    per_layer = [("xn1", _lib.FW16_XN1, rows, BF16), ("qkv", _lib.FW16_QKV, wide, BF16), ("A1", _lib.FW16_A1, ctx, F32), ("kst1", _lib.FW16_KST1, kst, F32),
                 ("y1", _lib.FW16_Y1, rows, BF16), ("a1", _lib.FW16_A1S, rows, BF16), ("h1", _lib.FW16_H1, rows, BF16), ("xn2", _lib.FW16_XN2, rows, BF16),
                 ("qc", _lib.FW16_QC, rows, BF16), ("y2", _lib.FW16_Y2, rows, BF16), ("a2", _lib.FW16_A2S, rows, BF16), ("h2", _lib.FW16_H2, rows, BF16),
                 ("z1", _lib.FW16_Z1, (D.M, D.ff), BF16), ("f1", _lib.FW16_F1, (D.M, D.ff), BF16), ("y3", _lib.FW16_Y3, rows, BF16),
                 ("a3", _lib.FW16_A3S, rows, BF16), ("h3", _lib.FW16_H3, rows, BF16)]
    at16 = [("A1", _lib.FW16_AT1)]
    if D.two:
        tr["tok0"] = ws.view(fw[_lib.FW16_TOK0], (D.B, d), F32)
        lenp = ws.view(fw[_lib.FW16_LENP], (D.B,), I64)
        assert torch.equal(lenp.cpu(), sb.swap_halves(inp["length"])), "the partner lengths are not the swapped lengths"
        per_layer += [("xn3", _lib.FW16_XN3, rows, BF16), ("iqkv", _lib.FW16_IQKV, wide, BF16), ("Ai", _lib.FW16_AI, ctx, F32),
                      ("ksti", _lib.FW16_KSTI, kst, F32), ("y4", _lib.FW16_Y4, rows, BF16), ("a4", _lib.FW16_A4S, rows, BF16), ("h2b", _lib.FW16_H2B, rows, BF16)]
        at16.append(("Ai", _lib.FW16_ATI))
    else:
        assert fw[_lib.FW16_TOK0] == -1 and fw[_lib.FW16_H2B] == -1 and tp[_lib.TAP16_INT_DA] == -1
    tap_layer = [("dh_in", _lib.TAP16_DH_IN, rows, BF16), ("ffn_t1", _lib.TAP16_FFN_T1, rows, BF16), ("ffn_dy", _lib.TAP16_FFN_DY, rows, BF16),
                 ("ffn_dz", _lib.TAP16_FFN_DZ, (D.M, D.ff), BF16), ("ffn_dh", _lib.TAP16_FFN_DH, rows, BF16),
                 ("ca_t1", _lib.TAP16_CA_T1, rows, BF16), ("ca_dy", _lib.TAP16_CA_DY, rows, BF16), ("ca_dq", _lib.TAP16_CA_DQ, rows, BF16),
                 ("ca_dA", _lib.TAP16_CA_DA, ctx, F32), ("ca_t2", _lib.TAP16_CA_T2, rows, BF16), ("ca_dh", _lib.TAP16_CA_DH, rows, BF16),
                 ("ca_dkv", _lib.TAP16_CA_DKV, (D.Mt, 2 * d), BF16), ("ca_dxfn", _lib.TAP16_CA_DXFN, (D.Mt, D.Lt), BF16),
                 ("ca_dxf_out", _lib.TAP16_CA_DXF_OUT, (D.Mt, D.Lt), F32),
                 ("sa_t1", _lib.TAP16_SA_T1, rows, BF16), ("sa_dy", _lib.TAP16_SA_DY, rows, BF16), ("sa_dqkv", _lib.TAP16_SA_DQKV, wide, BF16),
                 ("sa_dA", _lib.TAP16_SA_DA, ctx, F32), ("sa_t2", _lib.TAP16_SA_T2, rows, BF16), ("sa_dh", _lib.TAP16_SA_DH, rows, BF16)]
    if D.two:
        tap_layer += [("int_t1", _lib.TAP16_INT_T1, rows, BF16), ("int_dy", _lib.TAP16_INT_DY, rows, BF16), ("int_dqkv", _lib.TAP16_INT_DQKV, wide, BF16),
                      ("int_dA", _lib.TAP16_INT_DA, ctx, F32), ("int_t2", _lib.TAP16_INT_T2, rows, BF16), ("int_dh", _lib.TAP16_INT_DH, rows, BF16)]
    for l in range(D.L):
        base = fw[_lib.FW16_LAYER0] + fw[_lib.FW16_LSTRIDE] * l
        for key, slot, shape, dt in per_layer:
            tr[(key, l)] = ws.view(base + fw[slot], shape, dt)
        tbase = tx[_lib.TX16_LAYER0] + tx[_lib.TX16_LSTRIDE] * l
        for key, slot, shape, dt in (("xfn", _lib.TX16_XFN, (D.Mt, D.Lt), BF16), ("kv", _lib.TX16_KV, (D.Mt, 2 * d), BF16), ("Ac", _lib.TX16_AC, ctx, F32),
                                     ("kstc", _lib.TX16_KSTC, kst, F32)):
            tr[(key, l)] = tc.view(tbase + tx[slot], shape, dt)
        for key, slot in at16:
            got = ws.view(base + fw[slot], ctx, BF16)
            assert torch.equal(got.view(torch.int16), lb.at16_order(tr[(key, l)]).view(torch.int16)), "At16 is not at16_order of the device's own A"
        got = tc.view(tbase + tx[_lib.TX16_ATC], ctx, BF16)
        assert torch.equal(got.view(torch.int16), lb.at16_order(tr[("Ac", l)]).view(torch.int16)), "Atc is not at16_order of the device's own A_c"
        pbase = tp[_lib.TAP16_LAYER0] + tp[_lib.TAP16_LSTRIDE] * l
        for key, slot, shape, dt in tap_layer:
            tr[(key, l)] = tap.view(pbase + tp[slot], shape, dt)
    once = [("dhL", _lib.TAP16_DHL, rows, BF16), ("dtmp_emb", _lib.TAP16_DTMP_EMB, (D.B, D.E), F32), ("demb", _lib.TAP16_DEMB, (D.B, D.E), F32),
            ("dtmp_te", _lib.TAP16_DTMP_TE, (D.B, D.E), F32), ("dte_h", _lib.TAP16_DTE_H, (D.B, D.E), F32), ("dss", _lib.TAP16_DSS, (D.B, D.ss_ld), F32)]
    if D.two:
        once += [("tok0g", _lib.TAP16_TOK0, (D.B, d), F32), ("postmp", _lib.TAP16_POSTMP, (D.T, d), F32)]
    for key, slot, shape, dt in once:
        tr[key] = tap.view(tp[slot], shape, dt)
    # (what the backward leaves in its workspace is what the tap saw)
    for key, slot in (("dss", _lib.BW16_DSS), ("demb", _lib.BW16_DEMB), ("dte_h", _lib.BW16_DTE_H)):
        assert torch.equal(bws.view(bw[slot], tr[key].shape, F32), tr[key]), key
    for s_, t_ in enumerate(P.glob):
        if t_ is not None:
            o = fp.group_offsets[s_]
            tr[("g", s_)] = fp.grad[o:o + t_.numel()].view(t_.shape)
    for l in range(D.L):
        for s_, t_ in enumerate(P.lay[l]):
            if t_ is not None:
                o = fp.group_offsets[_lib.NGLOBAL + l * _lib.NLAYER + s_]
                tr[("gl", l, s_)] = fp.grad[o:o + t_.numel()].view(t_.shape)
    tr["out"] = res["out"].view(0, (D.M, D.F), F32)
    tr["dx"] = res["dx"].view(0, (D.M, D.F), F32)
    tr["dxf_proj"] = res["dxf_proj"].view(0, (D.B, D.E), F32)
    tr["dxf_out"] = res["dxf_out"].view(0, (D.Mt, D.Lt), F32)
    for key, t_ in tr.items():
        assert torch.isfinite(t_.float()).all(), "%s: not every element was written" % (key,)
    tr = {k: v.cpu() for k, v in tr.items()}

    # ---- the forms the call took, and the walk ----
    ffn = plan("bf16", fake_desc("bf16", D.M, D.ff, d, GELU, aux=True))
    forms = sb.plan_forms(D, "WSP16" in ffn[1], sched_f["fuse_front"], sched_f["ctx_mm16"], sched_b["edge16"])
    assert not sched_b["edge16"] or sched_b["Fp"] == D.Fp
    walk = sb.Walk(P, D, inp, forms, sb.REF, trace=tr).run()

    if repeats:
        again = backward(False)
        hooked = backward(False, hooked=True)
        for a, b_, h in zip(first, again, hooked):
            assert torch.equal(a.view(torch.int16), b_.view(torch.int16)), "the backward without the tap gives other bits"
            assert torch.equal(a.view(torch.int16), h.view(torch.int16)), "the hooked backward gives other bits"
    return {"worst": walk.worst, "forms": forms, "wgrad_fork": int(sched_b["wgrad_fork"])}


def held(name, r, tag=""):
    for kind, (ratio, key) in sorted(r["worst"].items()):
        print("RATIO %s%s | %s | %.3f | %s" % (name, tag, kind, ratio, key))
    bad = {k: v for k, v in r["worst"].items() if not v[0] <= 1.0}
    assert not bad, "%s%s: stages beyond their bound: %s" % (name, tag, bad)


def forms_tuple(f):
    return tuple(bool(f[k]) for k in ("joint_kernel", "ffn_wsp16", "fuse_front", "ctx_mm16", "edge16"))


@pytest.mark.parametrize("name", list(sb.CASES))
def test_every_stage_of_the_step_within_its_bound(name):
    r = run_case(name)
    print("FORMS %s %s wgrad_fork %d" % (name, r["forms"], r["wgrad_fork"]))
    held(name, r)
    assert forms_tuple(r["forms"]) == sb.REACH[name] and not r["wgrad_fork"], (r["forms"], r["wgrad_fork"])


CHILD_CASES = ("small", "pairs", "fused")


def child(env_extra):
    env = dict(os.environ, OMP_NUM_THREADS="4", **env_extra)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_step_worker.py")] + list(CHILD_CASES), env=env, capture_output=True, text=True,
                           timeout=300)
    except subprocess.TimeoutExpired:
        return {"error": "the child ran into its time limit"}
    if r.returncode != 0:
        return {"error": r.stdout[-2000:] + r.stderr[-2000:]}
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("STEP ")][-1][len("STEP "):])


@pytest.fixture(scope="module")
def children():
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=4) as pool:
        return dict(zip([k for k, _, _, _ in FLIPPED], pool.map(lambda j: child({j[0]: j[1]}), FLIPPED)))


@pytest.mark.parametrize("knob,value,form,expect", FLIPPED)
def test_the_flipped_forms_within_the_same_bounds(knob, value, form, expect, children):
    res = children[knob]
    assert "error" not in res, res["error"]
    for name in CHILD_CASES:
        r = res[name]
        got = r["wgrad_fork"] if form == "wgrad_fork" else int(r["forms"][form])
        print("FORMS %s %s=%s %s wgrad_fork %d" % (name, knob, value, r["forms"], r["wgrad_fork"]))
        held(name, {"worst": {k: tuple(v) for k, v in r["worst"].items()}}, " %s=%s" % (knob, value))
        assert got == expect, "%s=%s: %s is %d in case %s" % (knob, value, form, got, name)
        # (every other form stays what the case reaches by default)
        want = dict(zip(("joint_kernel", "ffn_wsp16", "fuse_front", "ctx_mm16", "edge16"), sb.REACH[name]))
        assert all(bool(r["forms"][k]) == v for k, v in want.items() if k != form), (knob, name, r["forms"])


def test_a_capturing_stream_with_a_tap_set_is_refused():
    c = sb.CASES["small"]
    D = sb.Dims(c)
    m = sb.build_model(c, DEV, storage="bf16").train()
    inp = sb.case_inputs(c)
    gi = {k: inp[k].to(DEV) for k in ("x", "t", "length", "xf_proj", "xf_out")}
    x = gi["x"].clone().requires_grad_(True)
    out = m(x, gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"])      # (allocates everything before the capture)
    out.sum().backward()
    dims = m.dims(D.B, D.T, D.N)
    L = _lib.lib()
    fp = m.flat_params()
    n = L.hig_denoiser_bwd_bf16_tap_bytes(C.byref(dims))
    tapbuf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    bufs = [torch.zeros(k, dtype=torch.uint8, device=DEV) for k in (L.hig_workspace_bytes(C.byref(dims), 1), L.hig_textctx_bytes(C.byref(dims), 1),
                                                                    L.hig_bwd_workspace_bytes(C.byref(dims)))]
    dout, dxp, dxo = torch.zeros_like(gi["x"]), torch.zeros(D.B, D.E, device=DEV), torch.zeros(D.B, D.N, D.Lt, device=DEV)
    ptab, s16, gtab = fp.param_table(), fp.shadow16(m._param_version()), fp.ensure_grad()
    before = fp.grad.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    _lib.check(L.hig_denoiser_bwd_bf16_debug_tap(_lib.ptr(tapbuf), n))
    try:
        with torch.cuda.graph(graph):
            rc = L.hig_denoiser_bwd_bf16(C.byref(dims), ptab, s16, _lib.ptr(gi["x"]), _lib.ptr(gi["t"]), _lib.ptr(gi["length"]), _lib.ptr(gi["xf_out"]),
                                         _lib.ptr(bufs[1]), _lib.ptr(bufs[0]), _lib.ptr(dout), gtab, None, _lib.ptr(dxp), _lib.ptr(dxo), _lib.ptr(bufs[2]),
                                         _lib.stream_ptr())
    finally:
        _lib.check(L.hig_denoiser_bwd_bf16_debug_tap(None, 0))
    assert rc == _lib.EINVAL and "capturing" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(fp.grad, before) and not tapbuf.any()
