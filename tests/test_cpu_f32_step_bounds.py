"""tests/f32_step_bounds.py without a GPU: the stages compose to the model, an fp32 stand-in of the fp32-storage training step stays
within every stage's bound, every composition mutant breaks one, every softmax spread of every case stays within the validity
condition of the attention bounds, the layout tables of hig_f32_train_layout are what the size entries say, the tap's refusals hold,
and the REACH table is what the plans answer at 256 CUs.

Composition is what allows tests/test_gpu_f32_step_contract.py to hold the device stage by stage: that test never compares the step
with the model, only each launch with its own operands.  Here the same stage functions, chained in fp64, are the oracle
(oracle.denoiser_ref / oracle.interaction_ref) and torch autograd of it under the masked-MSE loss.
"""
import ctypes as C
import functools

import pytest
import torch

import bf16_step_bounds as sb
import f32_step_bounds as fb
from hig_amd import _lib
from oracle import denoiser_ref as R
from oracle import diffusion_ref as Dm
from oracle import interaction_ref as I

CASES = tuple(fb.CASES)


@functools.lru_cache(maxsize=None)
def setup(name):
    c = fb.CASES[name]
    m = fb.build_model(c)
    return c, fb.Dims(c), sb.Params(m), fb.case_inputs(c), m


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def oracle(name, perm=None):
    """The oracle in fp64 and its autograd under the masked-MSE loss -> out, {group: gradient}, dx, dxf_proj, dxf_out.  perm: the
    samples in another order (every sum over the batch is then taken in another order), results put back."""
    c, D, P, inp, _ = setup(name)
    p = P.oracle_dict()
    idx = torch.arange(D.B) if perm is None else perm
    x, xp, xo = (inp[k][idx].double().requires_grad_(True) for k in ("x", "xf_proj", "xf_out"))
    if c["two"]:
        out = I.interaction_forward(p, x, inp["t"][idx], inp["length"][idx], xp, xo, c["H"], c["L"], no_cross_attn=c["two"] == 2)
    else:
        out = R.denoiser_forward(p, x, inp["t"][idx], inp["length"][idx], xp, xo, c["H"], c["L"], no_eff=bool(c["full"]))
    Dm.masked_mse(out, inp["target"][idx].double(), R.src_mask(c["T"], inp["length"][idx]).double()).backward()
    inv = torch.argsort(idx)
    return out.detach()[inv], P.grouped({n: v.grad for n, v in p.items()}), x.grad[inv], xp.grad[inv], xo.grad[inv]


def compare(name, a, b):
    """The largest relative difference (per tensor: largest |difference| over largest |value|) between two (out, grads, dx,
    dxf_proj, dxf_out); the key.bias gradients of linear attention, exact zeros in the model, are held to 1e-12 of the largest
    gradient instead."""
    c, D, P, _, _ = setup(name)
    worst = max(rel(a[0].reshape(b[0].shape), b[0]), rel(a[2].reshape(b[2].shape), b[2]), rel(a[3].reshape(b[3].shape), b[3]),
                rel(a[4].reshape(b[4].shape), b[4]))
    gmax = max(v.abs().max().item() for v in b[1].values())
    d = D.d
    for k, ref in b[1].items():
        got = a[1][k]
        assert got.shape == ref.shape, k
        names = P.gnames[k[1]] if k[0] == "g" else P.lnames[k[1]][k[2]]
        if any(n.endswith(".key.bias") for n in names):           # softmax over the rows is blind to a key bias
            r0 = d * [n.endswith(".key.bias") for n in names].index(True)
            assert got[r0:r0 + d].abs().max().item() <= 1e-12 * gmax and ref[r0:r0 + d].abs().max().item() <= 1e-12 * gmax, k
            keep = torch.ones(len(ref), dtype=torch.bool)
            keep[r0:r0 + d] = False
            got, ref = got[keep], ref[keep]
        worst = max(worst, rel(got, ref))
    return worst


@functools.lru_cache(maxsize=None)
def exact(name):
    c, D, P, inp, _ = setup(name)
    ref = oracle(name)
    te = R.timestep_embedding(inp["t"], c["d"]).double()             # (the oracle takes the timestep embedding in fp32)
    inp = dict(inp, dout=fb.masked_mse_grad(ref[0], inp["target"], inp["length"]))
    return ref, inp, fb.Walk(P, D, inp, fb.EXACT, te=te).run()


@pytest.mark.parametrize("name", CASES)
def test_the_stages_compose_to_the_model(name):
    """Chain mode, fp64: out, every parameter gradient, dx, dxf_proj and dxf_out equal the oracle and torch autograd of it at fp64
    rounding -- gated a decade above what the oracle shows against itself with the samples in another order."""
    c, D, P, _, _ = setup(name)
    ref, inp, w = exact(name)
    h = D.B // 2
    perm = torch.cat([torch.arange(h - 1, -1, -1), torch.arange(D.B - 1, h - 1, -1)]) if c["two"] else torch.arange(D.B - 1, -1, -1)
    noise = compare(name, oracle(name, perm), ref)
    got = (w.out["out"], {k: v for k, v in w.out.items() if isinstance(k, tuple) and k[0] in ("g", "gl")}, w.out["dx"], w.out["dxf_proj"], w.out["dxf_out"])
    assert set(got[1]) == set(ref[1])
    err = compare(name, got, ref)
    print("composition %s: chain against the oracle %.2e, the oracle against itself reordered %.2e" % (name, err, noise))
    assert 1e-17 < noise < 1e-12
    assert err <= 10 * noise


@pytest.mark.parametrize("name", CASES)
def test_every_softmax_spread_within_the_attention_bounds_validity(name):
    """The EXACT chain through the check: every stage reproduces itself (ratio far below 1), and the largest logit spread any
    softmax of the case meets is at most 80."""
    c, D, P, _, _ = setup(name)
    _, inp, w = exact(name)
    ck = fb.Walk(P, D, inp, fb.REF, trace=w.out).run()
    print("spread %s: %.2f" % (name, ck.spread))
    assert 0 < ck.spread <= 80
    # (the chain was handed the oracle's timestep embedding, which the oracle takes in fp32: that one stage sits at fp32 distance)
    # (full attention: the check's reference carries the fp32 rounding of the -1e5 offset on the rows at and beyond a length, to the
    # 2^-7 grid there, which an fp64 chain does not have: those two kinds are not expected to reproduce themselves)
    bad = {k: v for k, v in ck.worst.items() if k not in ("full", "full_bwd") and not v[0] <= (1.0 if k == "temb" else 1e-3)}
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def standin(name, mutant=None):
    c, D, P, inp, _ = setup(name)
    hooked = mutant in fb.HOOKED_MUTANTS
    clean = fb.Walk(P, D, inp, fb.STANDIN)
    clean.text_context()
    clean.forward()
    inp = dict(inp, dout=fb.masked_mse_grad(clean.out["out"].reshape(D.B, D.T, D.F), inp["target"], inp["length"]))
    s = fb.Walk(P, D, inp, fb.STANDIN, mutant=mutant, hooked=hooked).run()
    return inp, s.out


@pytest.mark.parametrize("name", CASES)
def test_the_standin_stays_within_every_bound(name):
    c, D, P, _, _ = setup(name)
    inp, trace = standin(name)
    ck = fb.Walk(P, D, inp, fb.REF, trace=trace).run()
    print("standin %s: " % name + ", ".join("%s %.3f" % (k, v[0]) for k, v in sorted(ck.worst.items())))
    assert ck.seen == set(trace) - {"dxf_out_run"}, (ck.seen ^ set(trace))
    assert len(ck.worst) >= 12
    assert all(v[0] <= 1.0 for v in ck.worst.values()), {k: v for k, v in ck.worst.items() if not v[0] <= 1.0}


MUTANT_CASE = {m: ("pairs" if m in fb.TWO_PERSON_MUTANTS else "full" if m in fb.FULL_MUTANTS else "small") for m in fb.MUTANTS}


@pytest.mark.parametrize("mutant", fb.MUTANTS)
def test_every_mutant_breaks_a_bound(mutant):
    """One composition fault in the stand-in: at least one stage is beyond its bound."""
    name = MUTANT_CASE[mutant]
    c, D, P, _, _ = setup(name)
    inp, trace = standin(name, mutant)
    ck = fb.Walk(P, D, inp, fb.REF, trace=trace).run()
    bad = {k: v for k, v in ck.worst.items() if not v[0] <= 1.0}
    print("mutant %s: %s" % (mutant, ", ".join("%s %.3g at %s" % (k, v[0], v[1]) for k, v in sorted(bad.items()))))
    assert bad, mutant


def test_the_linear_cross_attention_mutant_also_shows_on_linear_attention():
    c, D, P, _, _ = setup("small")
    inp, trace = standin("small", "cross_masked_with_motion_lengths")
    ck = fb.Walk(P, D, inp, fb.REF, trace=trace).run()
    assert any(not v[0] <= 1.0 for v in ck.worst.values())


# ----------------------------------------------------------------------------------------------------------------------
# the library's hooks, as far as they go without a device
# ----------------------------------------------------------------------------------------------------------------------
def layout(dims, which, n):
    arr = (C.c_int64 * n)()
    assert _lib.lib().hig_f32_train_layout(C.byref(dims), which, arr, n) == n
    return list(arr)


def slot_bytes(D):
    """The extent in bytes of every named slot of the four tables (what the step writes there)."""
    L = _lib
    row, wide, st, ctx, kst, lse = D.M * D.d * 4, D.M * 3 * D.d * 4, D.M * 2 * 4, D.B * D.H * D.hd * D.hd * 4, D.B * D.d * 2 * 4, D.B * D.H * D.T * 4
    be, ssb, ffb = D.B * D.E * 4, D.B * D.ss_ld * 4, D.M * D.ff * 4
    fw = {L.FW32_TE: D.B * D.d * 4, L.FW32_TE_H: be, L.FW32_EMB: be, L.FW32_SS: ssb, L.FW32_H0: row, L.FW32_LENP: D.B * 8}
    fwl = {L.FW32_ST1: st, L.FW32_XN1: row, L.FW32_QKV: wide, L.FW32_A1: ctx, L.FW32_KST1: kst, L.FW32_LSE1: lse, L.FW32_Y1: row, L.FW32_ST2: st,
           L.FW32_A1S: row, L.FW32_H1: row, L.FW32_ST3: st, L.FW32_XN2: row, L.FW32_QC: row, L.FW32_LSE2: lse, L.FW32_Y2: row, L.FW32_ST4: st,
           L.FW32_A2S: row, L.FW32_H2: row, L.FW32_Z1: ffb, L.FW32_F1: ffb, L.FW32_Y3: row, L.FW32_ST5: st, L.FW32_A3S: row, L.FW32_H3: row,
           L.FW32_ST6: st, L.FW32_XN3: row, L.FW32_IQKV: wide, L.FW32_AI: ctx, L.FW32_KSTI: kst, L.FW32_Y4: row, L.FW32_ST7: st, L.FW32_A4S: row,
           L.FW32_H2B: row}
    kvb, xfb = D.Mt * 2 * D.d * 4, D.Mt * D.Lt * 4
    bw = {L.BW32_DHA: row, L.BW32_DHB: row, L.BW32_T1: row, L.BW32_T2: row, L.BW32_TFF: ffb, L.BW32_DQKV: wide, L.BW32_DA: ctx, L.BW32_DELTA: lse,
          L.BW32_DKV: kvb, L.BW32_DXFN: xfb, L.BW32_DSS: ssb, L.BW32_DEMB: be, L.BW32_DTMP: be, L.BW32_DTE_H: be, L.BW32_TOK0: D.B * D.d * 4,
          L.BW32_DOUTM: D.M * D.F * 4, L.BW32_POSTMP: D.T * D.d * 4, L.BW32_SLABS: 4, L.BW32_COLPART: 4, L.BW32_COLPART_W: 4, L.BW32_LNPART: 4,
          L.BW32_WT: ((11 if D.inter else 7) * D.d * D.d + 2 * D.d * D.ff + 2 * D.d * D.Lt) * 4, L.BW32_TA: 4, L.BW32_TB: 4, L.BW32_ATTN: 4,
          L.BW32_GTAIL: 4}
    tp = {L.TAP32_DHL: row, L.TAP32_DOUTM: D.M * D.F * 4, L.TAP32_TOK0: D.B * D.d * 4, L.TAP32_POSTMP: D.T * D.d * 4, L.TAP32_DTMP_EMB: be,
          L.TAP32_DTMP_TE: be}
    tpl = {s: row for s in range(L.TAP32_LSTRIDE + 1, L.TAP32_TOTAL)}
    tpl[L.TAP32_WT] = bw[L.BW32_WT]
    for s in (L.TAP32_FFN_DSS, L.TAP32_INT_DSS, L.TAP32_CA_DSS, L.TAP32_SA_DSS):
        tpl[s] = D.B * 2 * D.d * 4
    tpl[L.TAP32_FFN_DZ] = ffb
    tpl[L.TAP32_SA_DQKV] = tpl[L.TAP32_INT_DQKV] = wide
    tpl[L.TAP32_SA_DA] = tpl[L.TAP32_INT_DA] = tpl[L.TAP32_CA_DA] = ctx
    tpl[L.TAP32_SA_DELTA] = tpl[L.TAP32_CA_DELTA] = lse
    tpl[L.TAP32_CA_DKV] = kvb
    tpl[L.TAP32_CA_DXFN] = tpl[L.TAP32_CA_DXF_OUT] = xfb
    return fw, fwl, bw, tp, tpl


def disjoint(offs, sizes, end):
    spans = sorted((offs[s], offs[s] + sizes[s]) for s in sizes if offs[s] >= 0)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[0][0] >= 0 and spans[-1][1] <= end, spans


@pytest.mark.parametrize("name", CASES)
def test_the_layout_tables(name):
    c, D, P, inp, m = setup(name)
    L, lib = _lib, _lib.lib()
    dims = m.dims(D.B, D.T, D.N)
    fw, tx = layout(dims, L.LAYOUT32_FWD, L.FW32_NSLOTS), layout(dims, L.LAYOUT32_TEXT, L.TX32_NSLOTS)
    bw, tp = layout(dims, L.LAYOUT32_BWD, L.BW32_NSLOTS), layout(dims, L.LAYOUT32_TAP, L.TAP32_NSLOTS)
    assert fw[L.FW32_TOTAL] == lib.hig_workspace_bytes(C.byref(dims), 1) and tx[L.TX32_TOTAL] == lib.hig_textctx_bytes(C.byref(dims), 1)
    assert bw[L.BW32_TOTAL] == lib.hig_bwd_workspace_bytes(C.byref(dims)) and tp[L.TAP32_TOTAL] == lib.hig_denoiser_bwd_tap_bytes(C.byref(dims))
    sfw, sfwl, sbw, stp, stpl = slot_bytes(D)
    # -1 exactly where the model has no such buffer
    inter = {L.FW32_ST6, L.FW32_XN3, L.FW32_IQKV, L.FW32_AI, L.FW32_KSTI, L.FW32_Y4, L.FW32_ST7, L.FW32_A4S, L.FW32_H2B}
    lin, full = {L.FW32_A1, L.FW32_KST1, L.FW32_AI, L.FW32_KSTI}, {L.FW32_LSE1, L.FW32_LSE2}
    for s in range(L.FW32_NSLOTS):
        absent = (s in inter and not D.inter) or (s in lin and D.full) or (s in full and not D.full) or (s == L.FW32_LENP and not D.two)
        assert (fw[s] == -1) == absent, (s, fw[s])
    assert (tx[L.TX32_AC] == -1) == D.full and (tx[L.TX32_KSTC] == -1) == D.full and all(tx[s] >= 0 for s in (L.TX32_STT, L.TX32_KV, L.TX32_LAYER0))
    for s in range(L.BW32_NSLOTS):
        absent = (s == L.BW32_DA and D.full) or (s == L.BW32_DELTA and not D.full) or (s in (L.BW32_TOK0, L.BW32_DOUTM, L.BW32_POSTMP) and not D.two)
        assert (bw[s] == -1) == absent, (s, bw[s])
    tint = set(range(L.TAP32_INT_T1, L.TAP32_INT_DH + 1))
    tlin, tfull, ttwo = {L.TAP32_INT_DA, L.TAP32_CA_DA, L.TAP32_SA_DA}, {L.TAP32_CA_DELTA, L.TAP32_SA_DELTA}, {L.TAP32_DOUTM, L.TAP32_TOK0, L.TAP32_POSTMP}
    for s in range(L.TAP32_NSLOTS):
        absent = (s in tint and not D.inter) or (s in tlin and D.full) or (s in tfull and not D.full) or (s in ttwo and not D.two)
        assert (tp[s] == -1) == absent, (s, tp[s])
    # no two slots overlap, and every one lies inside its region
    disjoint(fw, sfw, fw[L.FW32_LAYER0])
    disjoint(fw, sfwl, fw[L.FW32_LSTRIDE])
    assert fw[L.FW32_LAYER0] + D.L * fw[L.FW32_LSTRIDE] == fw[L.FW32_TOTAL]
    kvb = D.Mt * 2 * D.d * 4
    assert tx[L.TX32_STT] + D.Mt * 8 <= tx[L.TX32_LAYER0] and tx[L.TX32_LAYER0] + D.L * tx[L.TX32_LSTRIDE] <= tx[L.TX32_KV]
    assert kvb <= tx[L.TX32_KV_STRIDE] and tx[L.TX32_KV] + D.L * tx[L.TX32_KV_STRIDE] == tx[L.TX32_TOTAL]
    if not D.full:
        disjoint(tx, {L.TX32_AC: D.B * D.H * D.hd * D.hd * 4, L.TX32_KSTC: D.B * D.d * 8}, tx[L.TX32_LSTRIDE])
    disjoint(bw, sbw, bw[L.BW32_TOTAL])
    disjoint(tp, stp, tp[L.TAP32_LAYER0])
    disjoint(tp, stpl, tp[L.TAP32_LSTRIDE])
    assert tp[L.TAP32_LAYER0] + D.L * tp[L.TAP32_LSTRIDE] == tp[L.TAP32_TOTAL]
    # n_out is respected, unknown tables and bf16 storage are refused
    v = (C.c_int64 * 4)(-7, -7, -7, -7)
    assert lib.hig_f32_train_layout(C.byref(dims), L.LAYOUT32_TAP, v, 3) == L.TAP32_NSLOTS and v[2] == tp[2] and v[3] == -7
    assert lib.hig_f32_train_layout(C.byref(dims), L.LAYOUT32_FWD, None, 64) == L.FW32_NSLOTS
    assert lib.hig_f32_train_layout(C.byref(dims), 4, v, 4) == L.EINVAL and lib.hig_f32_train_layout(C.byref(dims), -1, v, 4) == L.EINVAL
    assert lib.hig_f32_train_layout(None, L.LAYOUT32_FWD, v, 4) < 0


def test_bf16_storage_and_bad_tap_buffers_are_refused_without_a_device():
    L, lib = _lib, _lib.lib()
    c = sb.CASES["small"]
    m16 = sb.build_model(c, storage="bf16")
    d16 = m16.dims(c["B"], c["T"], c["N"])
    v = (C.c_int64 * 4)()
    assert lib.hig_f32_train_layout(C.byref(d16), L.LAYOUT32_FWD, v, 4) == L.EINVAL and "HIG_STORE_F32" in L.last_error()
    assert lib.hig_denoiser_bwd_tap_bytes(C.byref(d16)) == L.EINVAL and lib.hig_denoiser_bwd_tap_bytes(None) < 0
    _, D, P, inp, m = setup("small")
    dims = m.dims(D.B, D.T, D.N)
    need = lib.hig_denoiser_bwd_tap_bytes(C.byref(dims))
    assert need > 0
    fake = C.c_void_p(4096)
    assert lib.hig_denoiser_bwd_debug_tap(fake, 0) == L.EINVAL and lib.hig_denoiser_bwd_debug_tap(fake, -4) == L.EINVAL
    try:
        # a tap shorter than the dims need: the backward is refused before any HIP call (every pointer here is made up)
        assert lib.hig_denoiser_bwd_debug_tap(fake, need - 4) == 0
        args = [C.c_void_p(4096)] * 13
        rc = lib.hig_denoiser_bwd(C.byref(dims), args[0], args[1], args[2], args[3], args[4], args[5], args[6], args[7], args[8], args[9], args[10],
                                  args[11], args[12], None)
        assert rc == L.EINVAL and str(need) in L.last_error() and str(need - 4) in L.last_error()
    finally:
        assert lib.hig_denoiser_bwd_debug_tap(None, 0) == 0


# ----------------------------------------------------------------------------------------------------------------------
# reach
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_reach_is_what_the_plans_answer_at_256_cus(name):
    """REACH against hig_attn_plan (every attention call of the step), hig_gemm_plan (the GEMMs with dense operands) and
    hig_denoiser_plan (the schedule slots the GPU test asserts)."""
    c, D, P, inp, m = setup(name)
    reach = fb.REACH[name]
    assert fb.planned_attn(c) == set(reach["attn"]), (fb.planned_attn(c), reach["attn"])
    assert fb.planned_gemm(c) <= reach["fwd"] | reach["bwd"], (fb.planned_gemm(c), reach)
    dims = m.dims(D.B, D.T, D.N)
    fwd = _lib.denoiser_plan(dims, _lib.DN_ENTRY_FWD32, training=1, has_xf_out=1, switches={})
    assert (fwd["fuse_apply"], fwd["fold32"], fwd["split"], fwd["text_fork"], fwd["text_batched"]) == (0, 0, 0, 1, 0), fwd
    bwd = _lib.denoiser_plan(dims, _lib.DN_ENTRY_BWD32, training=1, switches={})
    assert bwd["wgrad_fork"] == 1 and _lib.denoiser_plan(dims, _lib.DN_ENTRY_BWD32, training=1, switches={"HIG_BWD_OVERLAP": 0})["wgrad_fork"] == 0
    assert _lib.denoiser_plan(dims, _lib.DN_ENTRY_FWD32, training=1, has_xf_out=1, switches={"HIG_TEXT_FORK": 0})["text_fork"] == 0
    assert _lib.denoiser_plan(dims, _lib.DN_ENTRY_FWD32, training=1, has_xf_out=1, switches={"HIG_FWD_SPLIT": 1})["split"] == 0


def test_every_path_of_the_baseline_training_shapes_is_reached_or_named():
    """What the plans answer for the fp32 training shapes of BASELINE.md: every attention path and every dense-GEMM path is
    reached by some case, or named in NOT_COVERED with its reason (and then reached by none)."""
    reached = {"gemm": set().union(*[r["fwd"] | r["bwd"] for r in fb.REACH.values()]), "attn": set().union(*[r["attn"] for r in fb.REACH.values()])}
    for k in ("gemm", "attn"):
        assert not reached[k] & set(fb.NOT_COVERED[k]), reached[k] & set(fb.NOT_COVERED[k])
    for shape in fb.BASELINE_SHAPES.values():
        assert fb.planned_attn(shape) <= reached["attn"] | set(fb.NOT_COVERED["attn"]), fb.planned_attn(shape) - reached["attn"]
        assert fb.planned_gemm(shape) <= reached["gemm"] | set(fb.NOT_COVERED["gemm"]), fb.planned_gemm(shape) - reached["gemm"]
