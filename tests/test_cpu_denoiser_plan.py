"""How a denoiser call is scheduled, asked of the plan entry (hig_denoiser_plan, csrc/denoiser_plan.hip) without a GPU: it is a
pure function of the entry point, the checked dims, the training / per-call-text flags, the facts of the derived-operand table,
whether the caller's stream is capturing, the switches, the CU count and whether the fp32 weight-stationary GEMM is active.
tests/test_gpu_denoiser_schedule.py asserts on the device that the entry points ran what this plan names.

The rules are restated here as tables of expected fields, not as their implementation:
  - the default plan of every benchmarked configuration and of every entry code;
  - every threshold at both of its sides;
  - every switch tests/test_gpu_knobs.py flips: which plan fields it changes, and that it changes no other -- a switch that
    stopped having an effect fails here;
  - what a capture in progress clears, and nothing else;
  - purity."""
import ctypes as C
import os

import pytest

from hig_amd import _lib  # noqa: E402
from test_gpu_knobs import KNOBS  # noqa: E402

TEXT32, TEXT16, FWD32, FWD16, TRAIN16, BWD32, BWD16 = range(7)
TABLE, GLOBALS, KVALL = _lib.DN_FACT_TABLE, _lib.DN_FACT_TEXT_GLOBALS, _lib.DN_FACT_KVALL
D32, D16 = TABLE | GLOBALS, TABLE | GLOBALS | KVALL            # a complete derived-operand table (bf16, linear attention: the slot exists)
BF16_ENTRIES = (TEXT16, FWD16, TRAIN16, BWD16)
CFG2 = dict(B=64, T=196, F=150, d=512, H=8, ff=1024, L=8)
CFG3 = dict(CFG2, B=32)
CFG5 = dict(CFG2, B=32, T=300, d=1024, L=12)
TWO = dict(CFG2, T=91, F=263, two=1)


def dims(entry, B=64, T=196, F=150, d=512, H=8, ff=1024, L=8, full=0, prec=0, two=0):
    return _lib.Dims(B=B, T=T, F=F, d=d, H=H, ff=ff, L=L, N=77, Lt=256, num_frames=max(T, 196), attn_kind=full, prec=prec, two_person=two,
                     storage=int(entry in BF16_ENTRIES))


def plan(entry, training=0, xf=0, facts=0, cap=0, cus=256, wsp=1, sw=None, **shape):
    """The plan with the switches at their defaults except `sw` ({name: value}): never the environment's."""
    return _lib.denoiser_plan(dims(entry, **shape), entry, training, xf, facts, cap, cus, wsp, dict(sw or {}))


def on(p):
    """The non-zero fields of a plan, `entry` apart."""
    return {k: v for k, v in p.items() if v and k != "entry"}


def ones(*names, **values):
    return dict({n: 1 for n in names}, **values)


# ---- the default plan of each benchmarked configuration, and of each entry code, at 256 CUs with the fp32 weight-stationary GEMM ----
DEFAULTS = [
    ("config2_fp32_per_call_text", FWD32, dict(CFG2, xf=1, facts=D32), ones("text_batched", "fuse_apply", "fold32")),
    ("config2_fp32_cached_text", FWD32, dict(CFG2, facts=TABLE), ones("fuse_apply", "fold32")),
    ("config2_fp32_no_derived_operands", FWD32, dict(CFG2, xf=1), ones("text_fork", "fuse_apply", "wants_side_stream")),
    ("config3_bf16", FWD16, dict(CFG3, xf=1, facts=D16), ones("text_batched", "ctx_mm16", "joint16", "fuse_apply", "fuse_mm16", "fuse_out")),
    ("config5_bf16", FWD16, dict(CFG5, xf=1, facts=D16),
     ones("text_batched", "fork_emb", "ctx_mm16", "joint16", "fuse_apply", "fuse_mm16", "wants_side_stream")),
    ("two_person_training_fp32_fwd", FWD32, dict(TWO, training=1), {}),
    ("two_person_training_fp32_bwd", BWD32, dict(TWO, training=1), ones("wgrad_fork", "wants_side_stream")),
    ("two_person_training_bf16_fwd", TRAIN16, dict(TWO, training=1), ones("fuse_front", "ctx_mm16")),
    ("two_person_training_bf16_bwd", BWD16, dict(TWO, training=1), ones("edge16", Fp=288)),
    ("text32", TEXT32, dict(CFG2), {}),
    ("text32_training", TEXT32, dict(CFG2, training=1), {}),
    ("text16", TEXT16, dict(CFG2, facts=KVALL), ones("ctx_mm16")),
    ("text16_training", TEXT16, dict(CFG2, training=1, facts=KVALL), ones("ctx_mm16")),
    ("fwd16_cached_text", FWD16, dict(CFG2, facts=D16), ones("ctx_mm16", "joint16", "fuse_apply", "fuse_mm16", "fuse_out", "wants_side_stream")),
    ("train16", TRAIN16, dict(CFG2, training=1), ones("fuse_front", "ctx_mm16")),
    ("bwd32", BWD32, dict(CFG2, training=1), ones("wgrad_fork", "wants_side_stream")),
    ("bwd16", BWD16, dict(CFG2, training=1), ones("edge16", Fp=160)),
]


@pytest.mark.parametrize("name,entry,call,expect", DEFAULTS, ids=[r[0] for r in DEFAULTS])
def test_default_plan(name, entry, call, expect):
    p = plan(entry, **call)
    assert p["entry"] == entry and on(p) == expect


def test_config5_forks_the_embedding_chain_because_its_modulation_weight_is_256_mb():
    E, ss_ld = 4 * CFG5["d"], 3 * CFG5["L"] * 2 * CFG5["d"]
    assert E * ss_ld * 2 >= 256 << 20 > 4 * 512 * (3 * 8 * 2 * 512) * 2      # config 5 over, config 3 under
    assert plan(FWD16, xf=1, facts=D16, **CFG5)["fork_emb"] == 1 and plan(FWD16, xf=1, facts=D16, **CFG3)["fork_emb"] == 0
    # the smallest d = 1024 model over the limit: 6 layers (4096 x 6144 L x 2 bytes)
    assert [plan(FWD16, facts=D16, **dict(CFG5, L=L))["fork_emb"] for L in (5, 6)] == [0, 1]


# ---- thresholds, both sides ----
def test_split_rule():
    """B >= 16 and B T >= 8192, single-person; unset it is on for the bf16 product modes and where the weight-stationary kernel is off."""
    for prec, wsp, default_on in ((0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 0, 1), (2, 1, 1)):
        assert plan(FWD32, B=16, T=512, prec=prec, wsp=wsp)["split"] == default_on, (prec, wsp)
    for B, T, expect in ((16, 512, 1), (16, 511, 0), (15, 547, 0), (15, 1024, 0), (17, 482, 1), (17, 481, 0)):
        p = plan(FWD32, B=B, T=T, prec=1)
        assert (p["split"], p["wants_side_stream"]) == (expect, expect), (B, T)
        assert plan(FWD32, B=B, T=T, sw={"HIG_FWD_SPLIT": 1})["split"] == expect      # forced on: the shape rule still holds
    assert plan(FWD32, B=16, T=512, prec=1, two=2)["split"] == 0                       # two-person: whole batch only


@pytest.mark.parametrize("cus,n,B_on", [(256, 1, 96), (128, 1, 48), (256, 4, 128), (128, 4, 64), (256, 2, 64)])
def test_fuse_out_limit(cus, n, B_on):
    """ceil(T / 32) B <= 3 workgroups per CU (HIG_FUSE_OUT = n >= 2: n per CU), T = 256: 8 strips per sample."""
    sw = {"HIG_FUSE_OUT": n}
    assert 8 * B_on == cus * (n if n >= 2 else 3)
    assert plan(FWD16, B=B_on, T=256, cus=cus, sw=sw)["fuse_out"] == 1 and plan(FWD16, B=B_on + 1, T=256, cus=cus, sw=sw)["fuse_out"] == 0
    assert plan(FWD16, B=B_on, T=257, cus=cus, sw=sw)["fuse_out"] == 0               # a ninth strip
    for shape in (dict(d=256, H=4), dict(d=1024, H=8), dict(d=512, H=4)):               # built for d = 512, head dim 64, 8 heads
        assert plan(FWD16, B=4, T=64, cus=cus, sw=sw, **shape)["fuse_out"] == 0


@pytest.mark.parametrize("H", [2, 4, 8, 16])
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_fused_apply_shapes(H, hd):
    d = H * hd
    for training in (0, 1):
        for full in (0, 1):
            shape = dict(B=4, T=64, d=d, H=H, ff=256, full=full)
            if d > 1024:                                                         # no such model: the dims check refuses
                with pytest.raises(RuntimeError, match="<= 1024"):
                    plan(FWD32, training=training, **shape)
                continue
            assert plan(FWD32, training=training, **shape)["fuse_apply"] == int(not training and not full and hd == 64 and H in (4, 8))
            if hd == 32:                                                         # bf16 storage: head dim 64 / 128
                with pytest.raises(RuntimeError, match="head dim 64 or 128"):
                    plan(FWD16, **shape)
                continue
            mm16 = int(H in (4, 8))
            if training:
                if not full:
                    assert plan(TRAIN16, training=1, **shape)["fuse_front"] == mm16
            else:
                p = plan(FWD16, **shape)
                assert (p["fuse_mm16"], p["fuse_apply"]) == (mm16, mm16)
                q = plan(FWD16, sw={"HIG_FUSE_APPLY": 1}, **shape)                # the fp32-MFMA fused kernel: any served head dim, 4 or 8 heads
                assert (q["fuse_mm16"], q["fuse_apply"], q["fuse_out"]) == (0, mm16, 0)


@pytest.mark.parametrize("d", [64, 128, 1024, 1152])
def test_fold32(d):
    for facts in (0, TABLE):
        for training in (0, 1):
            if d > 1024:
                with pytest.raises(RuntimeError, match="<= 1024"):
                    plan(FWD32, training=training, facts=facts, B=2, T=16, d=d, H=9)
                continue
            assert plan(FWD32, training=training, facts=facts, B=2, T=16, d=d, H=8)["fold32"] == int(bool(facts) and not training and d % 128 == 0)


def test_text_fork_layer_limits():
    """One event per layer: 32 of them; the bf16 forward keeps the last for the embedding chain."""
    assert [plan(FWD32, xf=1, B=2, T=16, L=L)["text_fork"] for L in (32, 33)] == [1, 0]
    for L, expect in ((31, 1), (32, 0)):
        p = plan(FWD16, xf=1, facts=KVALL, B=2, T=16, L=L)
        assert (p["fork_text"], p["wants_side_stream"]) == (expect, expect)
    assert plan(FWD32, xf=0, B=2, T=16)["text_fork"] == 0 and plan(FWD16, xf=0, facts=KVALL, B=2, T=16)["fork_text"] == 0


def test_edge16_scratch_limit():
    """The padded edge operands must fit the (M, d) fp32 buffer.  F = 150 -> Fp = 160, d = 512: two (M, 160) bf16 matrices in
    256-byte granules + 163 840 + 2 x 327 680 + 768 bytes <= 2048 M first holds at M = 583 (1 193 216 <= 1 193 984; at 582:
    1 192 704 > 1 191 936)."""
    def fits(M, Fp=160, d=512):
        up = lambda v: -(-v // 256) * 256
        return 2 * up(M * Fp * 2) + up(d * Fp * 2) + 2 * up(Fp * d * 4) + up(Fp * 4) <= M * d * 4
    assert fits(583) and not fits(582)
    assert on(plan(BWD16, training=1, B=1, T=583)) == ones("edge16", Fp=160)
    assert on(plan(BWD16, training=1, B=1, T=582)) == {}
    assert on(plan(BWD16, training=1, B=11, T=53)) == ones("edge16", Fp=160) and on(plan(BWD16, training=1, B=2, T=291)) == {}   # M = 583 / 582
    assert plan(BWD16, training=1, B=64, T=196, F=263)["Fp"] == 288
    assert plan(BWD16, training=1, B=32768, T=205, F=150)["edge16"] == 0          # M Fp >= 2^30: 32-bit element offsets
    with pytest.raises(RuntimeError):                                               # d not a multiple of 8: no such model (head dim 125)
        plan(BWD16, training=1, d=500, H=4)


# ---- every switch the knob test flips: exactly these fields change, on exactly these calls ----
PROBES = {
    "fwd32": (FWD32, dict(CFG2, xf=1, facts=D32)),
    "fwd32_plain": (FWD32, dict(CFG2, xf=1)),
    "fwd32_split": (FWD32, dict(B=16, T=512, wsp=0)),
    "text32": (TEXT32, dict(CFG2)),
    "fwd16": (FWD16, dict(CFG3, xf=1, facts=D16)),
    "fwd16_plain": (FWD16, dict(CFG3, xf=1, facts=KVALL)),
    "fwd16_config5": (FWD16, dict(CFG5, facts=D16)),
    "text16": (TEXT16, dict(CFG3, facts=KVALL)),
    "train16": (TRAIN16, dict(CFG2, training=1)),
    "bwd32": (BWD32, dict(CFG2, training=1)),
    "bwd32_captured": (BWD32, dict(CFG2, training=1, cap=1)),
    "bwd16": (BWD16, dict(CFG2, training=1)),
}
OFF, ON = (1, 0), (0, 1)      # (default, flipped)
SIDE_OFF, SIDE_ON = {"wants_side_stream": OFF}, {"wants_side_stream": ON}
FLIPS = {
    ("HIG_BWD_OVERLAP", "0"): {"fwd32_plain": dict(SIDE_OFF, text_fork=OFF), "fwd32_split": dict(SIDE_OFF, split=OFF),
                               "fwd16_plain": dict(SIDE_OFF, fork_text=OFF), "fwd16_config5": dict(SIDE_OFF, fork_emb=OFF),
                               "bwd32": dict(SIDE_OFF, wgrad_fork=OFF)},
    ("HIG_BWD_OVERLAP", "1"): {"bwd32_captured": dict(SIDE_ON, wgrad_fork=ON), "bwd16": dict(SIDE_ON, wgrad_fork=ON)},
    ("HIG_TEXT_FORK", "0"): {"fwd32_plain": dict(SIDE_OFF, text_fork=OFF)},
    ("HIG_FWD_SPLIT", "0"): {"fwd32_split": dict(SIDE_OFF, split=OFF)},
    ("HIG_LNFOLD32", "0"): {"fwd32": dict(fold32=OFF)},
    ("HIG_CTX16", "0"): {n: dict(ctx_mm16=OFF) for n in ("fwd16", "fwd16_plain", "fwd16_config5", "text16", "train16")},
    ("HIG_FWD16_FORK", "0"): {"fwd16_plain": dict(SIDE_OFF, fork_text=OFF), "fwd16_config5": dict(SIDE_OFF, fork_emb=OFF)},
    ("HIG_JOINT16", "0"): {n: dict(joint16=OFF) for n in ("fwd16", "fwd16_plain", "fwd16_config5")},
    ("HIG_FUSE_APPLY", "0"): {"fwd16": dict(fuse_apply=OFF, fuse_mm16=OFF, fuse_out=OFF), "fwd16_plain": dict(fuse_apply=OFF, fuse_mm16=OFF, fuse_out=OFF),
                              "fwd16_config5": dict(fuse_apply=OFF, fuse_mm16=OFF), "train16": dict(fuse_front=OFF)},
    ("HIG_FUSE_OUT", "0"): {n: dict(fuse_out=OFF) for n in ("fwd16", "fwd16_plain")},
    ("HIG_EDGE16", "0"): {"bwd16": dict(edge16=OFF, Fp=(160, 0))},
    # (the per-layer form is worth forking: the text side moves to the third stream)
    ("HIG_TEXT_BATCH", "0"): {"fwd32": dict(SIDE_ON, text_batched=OFF, text_fork=ON), "fwd16": dict(SIDE_ON, text_batched=OFF, fork_text=ON)},
}


def test_the_flip_table_covers_every_denoiser_switch_of_the_knob_test():
    flipped = {k for k, _ in KNOBS}
    assert set(_lib.DN_SWITCHES) <= flipped, set(_lib.DN_SWITCHES) - flipped
    assert set(FLIPS) == {(k, v) for k, v in KNOBS if k in _lib.DN_SWITCHES}
    assert all(any(changes for changes in row.values()) for row in FLIPS.values()), "a switch without an effect"


@pytest.mark.parametrize("knob,value", sorted(FLIPS), ids=["%s=%s" % kv for kv in sorted(FLIPS)])
def test_a_flipped_switch_changes_exactly_its_fields(knob, value):
    for name, (entry, call) in PROBES.items():
        before, after = plan(entry, **call), plan(entry, sw={knob: int(value)}, **call)
        changed = {k: (before[k], after[k]) for k in before if before[k] != after[k]}
        assert changed == FLIPS[(knob, value)].get(name, {}), (knob, value, name)


@pytest.mark.parametrize("overlap", [-1, 0, 1])
@pytest.mark.parametrize("cap", [0, 1])
def test_weight_gradient_fork(overlap, cap):
    """fp32: forked for eager launches, under capture only on request; bf16 storage: only on request; 0: never."""
    sw = {"HIG_BWD_OVERLAP": overlap}
    for entry, expect in ((BWD32, overlap == 1 or (overlap == -1 and not cap)), (BWD16, overlap == 1)):
        p = plan(entry, training=1, cap=cap, sw=sw, **CFG2)
        assert (p["wgrad_fork"], p["wants_side_stream"]) == (int(expect), int(expect)), (entry, overlap, cap)


# ---- a capture in progress ----
def test_capturing_clears_the_forward_forks_the_split_and_the_eager_backward_fork_and_nothing_else():
    cleared = {"fwd32_plain": {"text_fork"}, "fwd32_split": {"split"}, "fwd16_plain": {"fork_text"}, "fwd16_config5": {"fork_emb"}, "bwd32": {"wgrad_fork"}}
    for name, (entry, call) in PROBES.items():
        if "cap" in call:
            continue
        eager, captured = plan(entry, **call), plan(entry, cap=1, **call)
        changed = {k for k in eager if eager[k] != captured[k]}
        expect = cleared.get(name, set())
        assert changed == (expect | {"wants_side_stream"} if expect else set()), name
        assert all(captured[k] == 0 for k in changed)
    both = plan(FWD16, xf=1, facts=KVALL, cap=1, sw={"HIG_FWD16_FORK": 3}, **CFG3)
    assert (both["fork_emb"], both["fork_text"], both["wants_side_stream"]) == (0, 0, 0)
    assert plan(BWD32, training=1, cap=1, sw={"HIG_BWD_OVERLAP": 1}, **CFG2)["wgrad_fork"] == 1


# ---- purity, and the entry's own refusals ----
def test_the_plan_is_a_pure_function_and_null_switches_are_the_process_switches():
    env = {n: int(os.environ[n]) for n in _lib.DN_SWITCHES if n in os.environ}
    for name, (entry, call) in PROBES.items():
        assert plan(entry, **call) == plan(entry, **call)
        c = dict(call)
        args = (c.pop("training", 0), c.pop("xf", 0), c.pop("facts", 0), c.pop("cap", 0), c.pop("cus", 256), c.pop("wsp", 1))
        assert _lib.denoiser_plan(dims(entry, **c), entry, *args, switches=None) == _lib.denoiser_plan(dims(entry, **c), entry, *args, switches=env), name


def test_refusals_and_short_outputs():
    L = _lib.lib()
    out = (C.c_int32 * _lib.DN_PLAN_NSLOTS)(*([7] * _lib.DN_PLAN_NSLOTS))
    bad = dims(FWD32, T=500)
    bad.num_frames = 196
    assert L.hig_denoiser_plan(C.byref(bad), FWD32, 0, 0, 0, 0, 256, 1, None, out, _lib.DN_PLAN_NSLOTS) == -1 and "num_frames" in _lib.last_error()
    assert L.hig_denoiser_plan(None, FWD32, 0, 0, 0, 0, 256, 1, None, out, _lib.DN_PLAN_NSLOTS) == -1
    for entry in (-1, 7):
        assert L.hig_denoiser_plan(C.byref(dims(FWD32)), entry, 0, 0, 0, 0, 256, 1, None, out, _lib.DN_PLAN_NSLOTS) == -1
    assert L.hig_denoiser_plan(C.byref(dims(FWD32)), FWD16, 0, 0, 0, 0, 256, 1, None, out, _lib.DN_PLAN_NSLOTS) == -1      # fp32 dims, bf16 entry
    assert "storage" in _lib.last_error() and list(out) == [7] * _lib.DN_PLAN_NSLOTS                                       # nothing written
    assert L.hig_denoiser_plan(C.byref(dims(FWD32)), FWD32, 0, 0, 0, 0, 256, 1, None, None, _lib.DN_PLAN_NSLOTS) == 0
    assert L.hig_denoiser_plan(C.byref(dims(FWD32)), FWD32, 0, 0, 0, 0, 256, 1, None, out, 4) == 0
    assert list(out)[:4] == [FWD32, 0, 0, 1] and list(out)[4:] == [7] * (_lib.DN_PLAN_NSLOTS - 4)                          # entry, -, -, fuse_apply
