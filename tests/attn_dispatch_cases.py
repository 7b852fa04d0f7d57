"""The attention dispatch cases both suites hold the library to: tests/test_gpu_attn_contract.py runs them on the device and
reads the launch counters and hig_attn_last_split, tests/test_cpu_attn_plan.py asks the plan entry (hig_attn_plan,
csrc/attn_plan.hip) the same questions without one.  Plain data and the `plan` helper; no fixtures."""
import ctypes as C

from hig_amd import _lib

PATHS = ("CTX", "CTX_MFMA", "CTX_PART", "APPLY", "APPLY_MFMA", "APPLY_WAVE64", "APPLY_STY", "APPLY_STY_WAVE64", "APPLY_BWD",
         "APPLY_BWD_MFMA", "CTX_BWD", "CTX_BWD_MFMA", "FULL_FWD", "FULL_FWD_MFMA", "FULL_BWD", "FULL_BWD_MFMA")
PATH_NAME = {getattr(_lib, "ATTN_PATH_" + n): n for n in PATHS}
ENTRIES = ("ctx", "apply", "apply_sty", "apply_bwd", "ctx_bwd", "full_fwd", "full_bwd")
ENTRY = {n: getattr(_lib, "ATTN_ENTRY_" + n.upper()) for n in ENTRIES}
F32, BF16 = "f32", "bf16"
IO = {F32: _lib.ATTN_IO_F32, BF16: _lib.ATTN_IO_BF16}
ALL = _lib.ATTN_FACTS_ALL
CH = 64                 # rows per chunk of the linear-attention kernels


def plan(entry, io, B, rows, H, hd, Tk=0, scratch=True, facts=ALL, chip_cus=256, big_lds_ok=1):
    """What the library plans for one call of `entry` ('ctx', 'apply', ... of ENTRIES) with `io` rows (F32 / BF16):
    (return code, path name or None, split, variant).  chip_cus 0: the current device's."""
    path, split, variant = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    rc = _lib.lib().hig_attn_plan(ENTRY[entry], IO.get(io, io), B, rows, Tk, H, hd, int(scratch), facts, chip_cus, big_lds_ok,
                                  C.byref(path), C.byref(split), C.byref(variant))
    assert (rc == 0) == (path.value in PATH_NAME) and (rc == 0 or (path.value, split.value) == (-1, 0)), (rc, path.value, split.value)
    return rc, PATH_NAME.get(path.value), split.value, variant.value


def in_regime(regime, split, nblocks):
    """'one': a single workgroup walks every block; 'all': one workgroup per block; 'partial': strictly between."""
    return {"one": split == 1, "all": split == nblocks, "partial": 1 < split < nblocks}[regime]


def regime_bh(name, H, n):
    """B * H of the named occupancy regime on a device with n compute units."""
    return {"few": 7 * H, "2/5": (2 * n // 5) // H * H, "half": n // 2, "ncu-H": n - H, "ncu": n, "2ncu": 2 * n, "4ncu": 4 * n}[name]


# which table entry is which call: (entry of ENTRIES, scratch given)
CALLS = {"ctx_s": ("ctx", True), "ctx_n": ("ctx", False), "apply": ("apply", False), "apply_bwd": ("apply_bwd", True), "ctx_bwd": ("ctx_bwd", True)}

MFMA_ONE = {"ctx_s": ("CTX_MFMA", "one"), "ctx_n": ("CTX_MFMA", "one"), "apply_bwd": ("APPLY_BWD_MFMA", "one"),
            "ctx_bwd": ("CTX_BWD_MFMA", "one")}
MFMA_ALL = {"ctx_s": ("CTX_PART", "all"), "ctx_n": ("CTX_MFMA", "one"), "apply_bwd": ("APPLY_BWD_MFMA", "all"),
            "ctx_bwd": ("CTX_BWD_MFMA", "all")}
MFMA_PART = {"ctx_s": ("CTX_PART", "all"), "ctx_n": ("CTX_MFMA", "one"), "apply_bwd": ("APPLY_BWD_MFMA", "partial"),
             "ctx_bwd": ("CTX_BWD_MFMA", "partial")}
VALU = {"ctx_s": ("CTX", "one"), "ctx_n": ("CTX", "one"), "apply": ("APPLY", "all"), "apply_bwd": ("APPLY_BWD", "all"),
        "ctx_bwd": ("CTX_BWD", "all")}
WAVE = ("APPLY_WAVE64", "one")

# (id, io, hd, H, B * H regime, T, what each entry must run).  One chunk (T <= 64) is 'one' and 'all' at once; the rows say
# 'all' for the kernels that launch a workgroup per chunk and 'one' for those that walk.
# apply_mfma_kernel has no 'partial' row at fp32 / hd 64: rows >= 128 go to apply_wave64_kernel, and the two chunks of
# T < 128 leave nothing strictly between 1 and 2.
LIN_TABLE = [
    # VALU kernels: T not a multiple of 64, H not a power of two
    ("valu-hd8", F32, 8, 3, "few", 63, VALU), ("valu-hd16", F32, 16, 5, "few", 65, VALU), ("valu-hd32", F32, 32, 3, "few", 129, VALU),
    ("valu-hd32-T1", F32, 32, 6, "few", 1, VALU), ("valu-hd16-T300", F32, 16, 3, "few", 300, VALU),
    # fp32, head dim 64: few (sample, head) pairs -> one workgroup per chunk; every T edge
    ("f32-hd64-few-T1", F32, 64, 8, "few", 1, dict(MFMA_ALL, ctx_s=("CTX_MFMA", "one"), apply=("APPLY_MFMA", "all"))),
    ("f32-hd64-few-T63", F32, 64, 8, "few", 63, dict(MFMA_ALL, ctx_s=("CTX_MFMA", "one"), apply=("APPLY_MFMA", "all"))),
    ("f32-hd64-few-T64", F32, 64, 4, "few", 64, dict(MFMA_ALL, ctx_s=("CTX_MFMA", "one"), apply=("APPLY_MFMA", "all"))),
    ("f32-hd64-few-T65", F32, 64, 8, "few", 65, dict(MFMA_ALL, apply=("APPLY_MFMA", "all"))),
    ("f32-hd64-few-T127", F32, 64, 8, "few", 127, dict(MFMA_ALL, apply=("APPLY_MFMA", "all"))),
    ("f32-hd64-few-T128", F32, 64, 8, "few", 128, dict(MFMA_ALL, apply=WAVE)),
    ("f32-hd64-few-T129", F32, 64, 8, "few", 129, dict(MFMA_ALL, apply=WAVE)),
    ("f32-hd64-few-T196", F32, 64, 8, "few", 196, dict(MFMA_ALL, apply=WAVE)),
    ("f32-hd64-few-T300", F32, 64, 8, "few", 300, dict(MFMA_ALL, apply=WAVE)),
    # the partial walk: 5 chunks over 3 and over 2 workgroups
    ("f32-hd64-2/5-T300", F32, 64, 2, "2/5", 300, dict(MFMA_PART, apply=WAVE)),
    ("f32-hd64-half-T300", F32, 64, 8, "half", 300, dict(MFMA_PART, apply=WAVE)),
    ("f32-hd64-ncu-H-T300", F32, 64, 8, "ncu-H", 300, dict(MFMA_PART, apply=WAVE)),
    ("f32-hd64-half-T196", F32, 64, 4, "half", 196, dict(MFMA_PART, apply=WAVE)),
    # the chip is full: one workgroup walks everything, scratch or not
    ("f32-hd64-ncu-T196", F32, 64, 8, "ncu", 196, dict(MFMA_ONE, apply=WAVE)),
    ("f32-hd64-2ncu-T129", F32, 64, 8, "2ncu", 129, dict(MFMA_ONE, apply=WAVE)),
    ("f32-hd64-ncu-T127", F32, 64, 8, "ncu", 127, dict(MFMA_ONE, apply=("APPLY_MFMA", "all"))),
    ("f32-hd64-4ncu-T65", F32, 64, 8, "4ncu", 65, dict(MFMA_ONE, apply=("APPLY_MFMA", "one"))),
    # fp32, head dim 128 (apply_mfma_kernel aims at one workgroup per CU)
    ("f32-hd128-few-T65", F32, 128, 4, "few", 65, dict(MFMA_ALL, apply=("APPLY_MFMA", "all"))),
    ("f32-hd128-few-T300", F32, 128, 8, "few", 300, dict(MFMA_ALL, apply=("APPLY_MFMA", "all"))),
    ("f32-hd128-2/5-T300", F32, 128, 2, "2/5", 300, dict(MFMA_PART, apply=("APPLY_MFMA", "partial"))),
    ("f32-hd128-half-T300", F32, 128, 8, "half", 300, dict(MFMA_PART, apply=("APPLY_MFMA", "partial"))),
    ("f32-hd128-ncu-H-T196", F32, 128, 4, "ncu-H", 196, dict(MFMA_PART, apply=("APPLY_MFMA", "partial"))),
    ("f32-hd128-ncu-T129", F32, 128, 8, "ncu", 129, dict(MFMA_ONE, apply=("APPLY_MFMA", "one"))),
    ("f32-hd128-2ncu-T128", F32, 128, 8, "2ncu", 128, dict(MFMA_ONE, apply=("APPLY_MFMA", "one"))),
    # bf16 I/O, head dim 64 (apply_mfma_kernel aims at four workgroups per CU) and 128
    ("bf16-hd64-few-T196", BF16, 64, 8, "few", 196, dict(MFMA_ALL, apply=("APPLY_MFMA", "all"))),
    ("bf16-hd64-2/5-T300", BF16, 64, 2, "2/5", 300, dict(MFMA_PART, apply=("APPLY_MFMA", "all"))),
    ("bf16-hd64-half-T300", BF16, 64, 8, "half", 300, dict(MFMA_PART, apply=("APPLY_MFMA", "all"))),
    ("bf16-hd64-ncu-T300", BF16, 64, 8, "ncu", 300, dict(MFMA_ONE, apply=("APPLY_MFMA", "partial"))),
    ("bf16-hd64-2ncu-T300", BF16, 64, 8, "2ncu", 300, dict(MFMA_ONE, apply=("APPLY_MFMA", "partial"))),
    ("bf16-hd64-4ncu-T65", BF16, 64, 8, "4ncu", 65, dict(MFMA_ONE, apply=("APPLY_MFMA", "one"))),
    ("bf16-hd128-few-T129", BF16, 128, 4, "few", 129, dict(MFMA_ALL, apply=("APPLY_MFMA", "all"))),
    ("bf16-hd128-2/5-T300", BF16, 128, 2, "2/5", 300, dict(MFMA_PART, apply=("APPLY_MFMA", "partial"))),
    ("bf16-hd128-half-T300", BF16, 128, 8, "half", 300, dict(MFMA_PART, apply=("APPLY_MFMA", "partial"))),
    ("bf16-hd128-ncu-T196", BF16, 128, 8, "ncu", 196, dict(MFMA_ONE, apply=("APPLY_MFMA", "one"))),
]

# hig_linattn_apply_sty / _bf16: (io, hd, H, path, regime); regime None: the strips of apply_sty_wave64_kernel are a
# launch-geometry choice, its split is only required to lie in 1 .. number of 16-row tiles
APPLY_STY = [(F32, 64, 8, "APPLY_STY_WAVE64", None), (F32, 64, 4, "APPLY_STY_WAVE64", None), (F32, 128, 8, "APPLY_STY", "one"),
             (BF16, 64, 8, "APPLY_STY", "one"), (BF16, 128, 4, "APPLY_STY", "one")]
APPLY_STY_T = [1, 77, 196]
APPLY_STY_B = 3


def full_paths(hd):
    """(forward, backward) path of full attention at head dim hd with the default switches."""
    return ("FULL_FWD_MFMA", "FULL_BWD_MFMA") if hd >= 64 else ("FULL_FWD", "FULL_BWD")
