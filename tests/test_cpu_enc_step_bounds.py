"""tests/enc_step_bounds.py without a GPU: the stages of the text head and of the evaluation classifiers compose to the models,
an fp32 stand-in of each chain stays within every stage's bound, and every composition mutant breaks one.

Composition is what allows tests/test_gpu_enc_step_contract.py to hold the device stage by stage: that test never compares a
chain with its model, only each launch with its own operands.  Here the same stage functions, chained in fp64, are the oracles
(oracle.text_head_ref, oracle.eval_models_ref) and torch autograd of them for the upstream gradients of the case -- gated, as in
tests/test_cpu_bf16_step_bounds.py, a decade above what the oracle shows against itself with the samples in another order.
The library's two hooks (hig_text_head_layout / hig_eval_encoder_layout, hig_enc_bwd_debug_tap) are held here as far as they go
without a device: slot counts, totals, -1 members, refusals, and a short tap refused before any HIP call.
"""
import ctypes as C
import functools

import pytest
import torch

import enc_step_bounds as eb
from hig_amd import _lib
from oracle import eval_models_ref as R
from oracle import text_head_ref as TH

KINDS = ("enc", "con")


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def compare(got, ref, n):
    """Largest relative difference (per tensor: largest |difference| over largest |value|) over {name: tensor}; the key third of an
    in_proj_bias gradient, an exact zero in the model, is held to 1e-12 of the largest gradient instead."""
    assert set(got) == set(ref), set(got) ^ set(ref)
    gmax = max(v.abs().max().item() for v in ref.values())
    worst = 0.0
    for k, r in ref.items():
        g = got[k].reshape(r.shape)
        if k.endswith("in_proj_bias"):
            assert g[n:2 * n].abs().max().item() <= 1e-12 * gmax and r[n:2 * n].abs().max().item() <= 1e-12 * gmax, k
            g, r = torch.cat([g[:n], g[2 * n:]]), torch.cat([r[:n], r[2 * n:]])
        worst = max(worst, rel(g, r))
    return worst


def named_results(P, out, extra):
    """{state-dict name: gradient} + the chain's outputs named in `extra` ({result name: buffer key})."""
    res = {"grad." + n: out[("g", s)] for s, n in enumerate(P.gnames) if n is not None}
    for l, row in enumerate(P.lnames):
        res.update({"grad." + n: out[("gl", l, s)] for s, n in enumerate(row)})
    res.update({k: out[key] for k, key in extra.items()})
    return res


# ---- the evaluation classifiers ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def esetup(name, kind, dfeature=True):
    c, D, P, inp = eb.eval_setup(name, kind)
    if not dfeature:
        inp = dict(inp, dfeature=None)
    return c, D, P, inp


def eval_oracle(name, kind, dfeature, perm=None):
    c, D, P, inp = esetup(name, kind, dfeature)
    p = P.oracle_dict()
    idx = torch.arange(D.B) if perm is None else perm
    x1, x2, length = inp["x1"][idx].double(), inp["x2"][idx].double(), inp["length"][idx]
    if kind == "enc":
        logits, feat = R.motion_encoder_forward(p, x1, x2, length, D.H)
    else:
        logits, feat = R.consistency_forward(p, x1, x2, length, D.H), None
    loss = (logits * inp["dlogits"][idx].double()).sum()
    if inp["dfeature"] is not None:
        loss = loss + (feat * inp["dfeature"][idx].double()).sum()
    loss.backward()
    inv = torch.argsort(idx)
    res = {"grad." + k: v.grad for k, v in p.items()}
    res["logits"] = logits.detach()[inv]
    if kind == "enc":
        res["feat"] = feat.detach()[inv]
    return res


@pytest.mark.parametrize("kind,dfeature", [("enc", True), ("enc", False), ("con", False)])     # (the consistency model has no feature output)
@pytest.mark.parametrize("name", list(eb.EVAL_CASES))
def test_the_evaluator_stages_compose_to_the_model(name, kind, dfeature):
    c, D, P, inp = esetup(name, kind, dfeature)
    ref = eval_oracle(name, kind, dfeature)
    noise = compare(eval_oracle(name, kind, dfeature, torch.arange(D.B - 1, -1, -1)), ref, D.d)
    w = eb.EvalWalk(P, D, inp, eb.EXACT).run()
    got = named_results(P, w.out, {"logits": "logits", "feat": "feat"} if kind == "enc" else {"logits": "logits"})
    seq = torch.zeros(D.num_frames, D.d, dtype=torch.float64)
    seq[:D.T - 1] = got["grad.sequence_embedding"]           # (the call writes the rows the forward read; the rest are the caller's zeros)
    got["grad.sequence_embedding"] = seq
    err = compare(got, ref, D.d)
    print("composition %s %s: chain against the oracle %.2e, the oracle against itself reordered %.2e" % (name, kind, err, noise))
    assert 1e-17 < noise < 1e-13
    assert err <= 10 * noise


def traced(walk_cls, P, D, inp, mutant=None):
    trace = walk_cls(P, D, inp, eb.STANDIN, mutant=mutant).run().out
    return walk_cls(P, D, inp, eb.REF, trace=trace).run().worst


def report(what, worst):
    print("%s: " % what + ", ".join("%s %.3f" % (k, v[0]) for k, v in sorted(worst.items())))
    return {k: v for k, v in worst.items() if not v[0] <= 1.0}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(eb.EVAL_CASES))
def test_the_evaluator_standin_stays_within_every_bound(name, kind):
    c, D, P, inp = esetup(name, kind)
    worst = traced(eb.EvalWalk, P, D, inp)
    assert set(worst) >= {"gemm32", "gemm32_gelu", "gemm32_dgelu", "xsum", "attn", "attn_bwd", "ln", "ln_bwd", "colsum", "copy", "pad_zero"}
    assert kind == "con" or set(worst) >= {"masked_mean", "pool", "head_scale"}
    assert not report("standin %s %s" % (name, kind), worst)


@pytest.mark.parametrize("mutant", eb.EVAL_MUTANTS + eb.LAYER_MUTANTS)
def test_every_evaluator_mutant_breaks_a_bound(mutant):
    """One composition fault in the stand-in: at least one stage is beyond its bound.  `hd8` gives it something to show on: two
    layers, four pairs with different lengths, a padded tail."""
    kind = "con" if mutant == "cls_marked_padded" else "enc"
    c, D, P, inp = esetup("hd8", kind)
    bad = report("mutant %s" % mutant, traced(eb.EvalWalk, P, D, inp, mutant))
    assert bad, mutant


# ---- the text head ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tsetup(name, variant):
    return eb.text_setup(name, variant)


def text_oracle(name, variant, perm=None):
    c, D, P, inp = tsetup(name, variant)
    p = P.oracle_dict()
    idx = torch.arange(D.B) if perm is None else perm
    clip = inp["clip_out"][idx].double().requires_grad_(True)
    xf_proj, xf_out = TH.text_head_forward(p, clip, inp["eot"][idx], D.H, D.L)
    loss = 0.0
    if inp["dxf_out"] is not None:
        loss = loss + (xf_out * inp["dxf_out"][idx].double()).sum()
    if inp["dxf_proj"] is not None:
        loss = loss + (xf_proj * inp["dxf_proj"][idx].double()).sum()
    loss.backward()
    inv = torch.argsort(idx)
    res = {"grad." + k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in p.items()}
    res.update({"xf_proj": xf_proj.detach()[inv], "xf_out": xf_out.detach()[inv]})
    if inp["want_dclip"]:
        res["dclip"] = clip.grad[inv]
    return res


@pytest.mark.parametrize("variant", eb.TEXT_VARIANTS)
@pytest.mark.parametrize("name", list(eb.TEXT_CASES))
def test_the_text_head_stages_compose_to_the_model(name, variant):
    c, D, P, inp = tsetup(name, variant)
    ref = text_oracle(name, variant)
    noise = compare(text_oracle(name, variant, torch.arange(D.B - 1, -1, -1)), ref, D.Lt)
    w = eb.TextWalk(P, D, inp, eb.EXACT).run()
    extra = {"xf_proj": "xf_proj", "xf_out": "xf_out"}
    if inp["want_dclip"]:
        extra["dclip"] = "dclip"
    err = compare(named_results(P, w.out, extra), ref, D.Lt)
    print("composition text %s %s: chain against the oracle %.2e, the oracle against itself reordered %.2e" % (name, variant, err, noise))
    assert 1e-17 < noise < 1e-13
    assert err <= 10 * noise


@pytest.mark.parametrize("variant", eb.TEXT_VARIANTS)
@pytest.mark.parametrize("name", list(eb.TEXT_CASES))
def test_the_text_head_standin_stays_within_every_bound(name, variant):
    c, D, P, inp = tsetup(name, variant)
    worst = traced(eb.TextWalk, P, D, inp)
    assert set(worst) >= {"gemm32", "gemm32_gelu", "gemm32_dgelu", "xsum", "attn", "attn_bwd", "ln", "ln_bwd", "gather"}
    assert ("scatter" in worst) == (inp["dxf_proj"] is not None)
    assert not report("standin text %s %s" % (name, variant), worst)


@pytest.mark.parametrize("mutant", eb.TEXT_MUTANTS + eb.LAYER_MUTANTS)
def test_every_text_head_mutant_breaks_a_bound(mutant):
    """`pre` has two layers and a pre-projection; the identity mutant needs the case without one."""
    c, D, P, inp = tsetup("identity" if mutant == "identity_pre_reads_x0" else "pre", "all")
    bad = report("mutant %s" % mutant, traced(eb.TextWalk, P, D, inp, mutant))
    assert bad, mutant


# ---- the library's two hooks, as far as they go without a device ------------------------------------------------------------
def table(fn, dims, which, n, n_out=None):
    arr = (C.c_int64 * (n + 1))(*([-7] * (n + 1)))
    return fn(C.byref(dims), which, arr, n if n_out is None else n_out), list(arr)


def test_the_layout_hooks_answer_by_named_slot_without_a_hip_call():
    L = _lib.lib()
    for name, c in eb.EVAL_CASES.items():
        for cls in (0, 1):
            e = _lib.EvalDims(B=c["B"], T=c["T"], F=c["F"], d=c["d"], H=c["H"], ff=c["ff"], L=c["L"], C=2 if cls else 26, cls=cls, prec=_lib.PREC_F32)
            for which, n, tot, total in ((_lib.ENC_LAYOUT_FWD, _lib.EFW_NSLOTS, _lib.EFW_TOTAL, L.hig_eval_encoder_train_workspace_bytes),
                                         (_lib.ENC_LAYOUT_BWD, _lib.EBW_NSLOTS, _lib.EBW_TOTAL, L.hig_eval_encoder_bwd_workspace_bytes),
                                         (_lib.ENC_LAYOUT_TAP, _lib.ETAP_NSLOTS, _lib.ETAP_TOTAL, L.hig_eval_encoder_bwd_tap_bytes)):
                rc, v = table(L.hig_eval_encoder_layout, e, which, n)
                assert rc == n and v[n] == -7 and v[tot] * 4 == total(C.byref(e)) > 0, (name, cls, which)
                assert all(x >= -1 and x <= v[tot] for x in v[:n])
                assert table(L.hig_eval_encoder_layout, e, which, n, 3) == (n, v[:3] + [-7] * (n - 2))          # n_out is respected
                assert L.hig_eval_encoder_layout(C.byref(e), which, None, n) == n
            fw, bw, tp = (table(L.hig_eval_encoder_layout, e, w, n)[1] for w, n in ((0, _lib.EFW_NSLOTS), (1, _lib.EBW_NSLOTS), (2, _lib.ETAP_NSLOTS)))
            head = [bw[getattr(_lib, "EBW_" + k)] for k in ("DFT", "G", "GN", "G2", "POOL1", "POOL2", "U1", "U2")]
            assert all((x == -1) == bool(cls) for x in head + [fw[_lib.EFW_O], fw[_lib.EFW_FEAT]])
            assert tp[_lib.ETAP_DXF_TOTAL] == tp[_lib.ETAP_DGATH] == -1 and tp[_lib.ETAP_DH_L] == 0 and tp[_lib.ETAP_DH_0] > 0
            S = cls + 2 * c["T"]
            assert fw[_lib.EFW_LSTRIDE] >= fw[_lib.EFW_X2] + c["B"] * S * c["d"] and fw[_lib.EFW_TOTAL] == fw[_lib.EFW_LAYER0] + c["L"] * fw[_lib.EFW_LSTRIDE]
            assert tp[_lib.ETAP_TOTAL] == tp[_lib.ETAP_LAYER0] + c["L"] * tp[_lib.ETAP_LSTRIDE] and tp[_lib.ETAP_LSTRIDE] >= tp[_lib.ETAP_DELTA] + c["B"] * c["H"] * S
    for name, c in eb.TEXT_CASES.items():
        t = _lib.TextDims(B=c["B"], N=c["N"], W=c["W"], Lt=c["Lt"], H=c["H"], ff=c["ff"], L=c["L"], E=c["E"], prec=_lib.PREC_F32)
        for which, n, tot, total in ((_lib.ENC_LAYOUT_FWD, _lib.TFW_NSLOTS, _lib.TFW_TOTAL, lambda d: L.hig_text_head_workspace_bytes(d, 1)),
                                     (_lib.ENC_LAYOUT_BWD, _lib.TBW_NSLOTS, _lib.TBW_TOTAL, L.hig_text_head_bwd_workspace_bytes),
                                     (_lib.ENC_LAYOUT_TAP, _lib.ETAP_NSLOTS, _lib.ETAP_TOTAL, L.hig_text_head_bwd_tap_bytes)):
            rc, v = table(L.hig_text_head_layout, t, which, n)
            assert rc == n and v[n] == -7 and v[tot] * 4 == total(C.byref(t)) > 0, (name, which)
        tp = table(L.hig_text_head_layout, t, _lib.ENC_LAYOUT_TAP, _lib.ETAP_NSLOTS)[1]
        assert tp[_lib.ETAP_DH_L] == tp[_lib.ETAP_DH_0] == -1 and tp[_lib.ETAP_DXF_TOTAL] == 0 and tp[_lib.ETAP_DGATH] > 0
    # an unknown table, NULL dims, dims the entry refuses
    for fn, ok, bad in ((L.hig_eval_encoder_layout, e, _lib.EvalDims(B=4, T=1, F=15, d=64, H=8, ff=128, L=2, C=26, cls=0, prec=0)),
                        (L.hig_text_head_layout, t, _lib.TextDims(B=2, N=77, W=64, Lt=28, H=4, ff=64, L=2, E=128, prec=0))):
        assert fn(C.byref(ok), 3, None, 0) == _lib.EINVAL and fn(C.byref(ok), -1, None, 0) == _lib.EINVAL and "no layout table" in _lib.last_error()
        assert fn(None, 0, None, 0) == _lib.EINVAL and fn(C.byref(bad), 0, None, 0) == _lib.EINVAL
    assert L.hig_eval_encoder_bwd_tap_bytes(None) == _lib.EINVAL and L.hig_text_head_bwd_tap_bytes(None) == _lib.EINVAL


def test_both_chains_lay_the_layer_block_and_the_layer_scratch_out_alike():
    """The same (B, S, n, ff, H): the text head at N = 24 tokens and the MotionEncoder `hd8` at S = 2 T = 24 share the per-layer
    block of the forward tables slot for slot, and the extents of the layer backward's own scratch members."""
    L = _lib.lib()
    c = eb.EVAL_CASES["hd8"]
    assert (c["B"], 2 * c["T"], c["d"], c["H"], c["ff"]) == (4, 24, 64, 8, 128)
    e = _lib.EvalDims(B=c["B"], T=c["T"], F=c["F"], d=c["d"], H=c["H"], ff=c["ff"], L=c["L"], C=26, cls=0, prec=_lib.PREC_F32)
    t = _lib.TextDims(B=4, N=24, W=64, Lt=64, H=8, ff=128, L=2, E=128, prec=_lib.PREC_F32)
    tf, tb = (table(L.hig_text_head_layout, t, w, n)[1] for w, n in ((_lib.ENC_LAYOUT_FWD, _lib.TFW_NSLOTS), (_lib.ENC_LAYOUT_BWD, _lib.TBW_NSLOTS)))
    ef, ebw = (table(L.hig_eval_encoder_layout, e, w, n)[1] for w, n in ((_lib.ENC_LAYOUT_FWD, _lib.EFW_NSLOTS), (_lib.ENC_LAYOUT_BWD, _lib.EBW_NSLOTS)))
    block = ("QKV", "LSE", "ATT", "R1", "ST1", "X1", "Z", "F", "R2", "ST2", "X2")
    assert len(block) == 11 and _lib.TFW_X2 - _lib.TFW_QKV == _lib.EFW_X2 - _lib.EFW_QKV == 10
    for k in block + ("LSTRIDE",):
        assert tf[getattr(_lib, "TFW_" + k)] == ef[getattr(_lib, "EFW_" + k)] >= 0, k
    assert tf[_lib.TFW_QKV] == 0 and tf[_lib.TFW_LSTRIDE] > tf[_lib.TFW_X2]

    def extent(v, names, prefix, k):           # from member k to the next member of its table
        at = v[getattr(_lib, prefix + k)]
        later = [v[getattr(_lib, prefix + m)] for m in names if m != "SLAB_FLOATS" and v[getattr(_lib, prefix + m)] > at]
        return min(later) - at
    tnames = [n[4:] for n in dir(_lib) if n.startswith("TBW_") and n != "TBW_NSLOTS"]
    enames = [n[4:] for n in dir(_lib) if n.startswith("EBW_") and n != "EBW_NSLOTS"]
    assert len(tnames) == _lib.TBW_NSLOTS and len(enames) == _lib.EBW_NSLOTS
    M = 4 * 24
    for k, floats in (("DFF", M * 128), ("DQKV", M * 3 * 64), ("DELTA", 4 * 8 * 24)):
        assert extent(tb, tnames, "TBW_", k) == extent(ebw, enames, "EBW_", k) == (floats + 63) // 64 * 64, k


def test_a_short_tap_is_refused_before_any_hip_call():
    """No device here: a call that got as far as a HIP call would fail with another code (or fault on the made-up addresses)."""
    L = _lib.lib()
    fake = C.c_void_p(1 << 24)
    c = eb.TEXT_CASES["pre"]
    t = _lib.TextDims(B=c["B"], N=c["N"], W=c["W"], Lt=c["Lt"], H=c["H"], ff=c["ff"], L=c["L"], E=c["E"], prec=_lib.PREC_F32)
    ttab = (C.c_void_p * (_lib.T_NGLOBAL + c["L"] * _lib.TL_NLAYER))(*([1 << 24] * (_lib.T_NGLOBAL + c["L"] * _lib.TL_NLAYER)))
    c = eb.EVAL_CASES["hd8"]
    e = _lib.EvalDims(B=c["B"], T=c["T"], F=c["F"], d=c["d"], H=c["H"], ff=c["ff"], L=c["L"], C=26, cls=0, prec=_lib.PREC_F32)
    etab = (C.c_void_p * (_lib.EV_NGLOBAL + c["L"] * _lib.TL_NLAYER))(*([1 << 24] * (_lib.EV_NGLOBAL + c["L"] * _lib.TL_NLAYER)))
    assert L.hig_enc_bwd_debug_tap(fake, 0) == _lib.EINVAL and L.hig_enc_bwd_debug_tap(fake, -4) == _lib.EINVAL
    try:
        assert L.hig_enc_bwd_debug_tap(fake, L.hig_text_head_bwd_tap_bytes(C.byref(t)) - 4) == 0
        assert L.hig_text_head_bwd(C.byref(t), ttab, fake, fake, fake, fake, fake, fake, ttab, fake, fake, None) == _lib.EINVAL
        assert "tap buffer" in _lib.last_error()
        assert L.hig_enc_bwd_debug_tap(fake, L.hig_eval_encoder_bwd_tap_bytes(C.byref(e)) - 4) == 0
        assert L.hig_eval_encoder_bwd(C.byref(e), etab, fake, fake, fake, fake, fake, None, etab, fake, None) == _lib.EINVAL
        assert "tap buffer" in _lib.last_error()
    finally:
        assert L.hig_enc_bwd_debug_tap(None, 0) == 0


def test_the_mutant_lists_are_the_ones_the_tests_run():
    assert set(eb.MUTANTS) == set(eb.EVAL_MUTANTS + eb.LAYER_MUTANTS + eb.TEXT_MUTANTS) and len(set(eb.MUTANTS)) == len(eb.MUTANTS) == 21
    assert set(eb.ENC_ONLY) <= set(eb.EVAL_MUTANTS) and _lib.TL_NLAYER == len(eb.TL_NAMES)
