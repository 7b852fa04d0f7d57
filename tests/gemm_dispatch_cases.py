"""The GEMM dispatch cases both suites hold the library to: tests/test_gpu_gemm_contract.py runs them on the device and reads
the launch counters, tests/test_cpu_gemm_plan.py asks the plan entries (hig_gemm_bf16_plan / hig_gemm_plan) the same questions
without one.  Plain data and descriptor builders; no fixtures."""
import ctypes as C

from hig_amd import _lib

PATHS = ("TILED32", "WSP32", "TAIL32", "WGRAD_WSP32", "SPLIT32", "WSP16", "WS16", "FEWROW16", "TILED16", "SPLIT16", "WGRAD16")
PATH_NAME = {getattr(_lib, "GEMM_PATH_" + n): n for n in PATHS}
NONE, BIAS, GELU, BIAS_RES, RES, DGELU, SILU, RES_SILU = (_lib.EPI_NONE, _lib.EPI_BIAS, _lib.EPI_BIAS_GELU, _lib.EPI_BIAS_RES,
                                                           _lib.EPI_RES, _lib.EPI_DGELU, _lib.EPI_BIAS_SILU, _lib.EPI_BIAS_RES_SILU)
HAS_BIAS = (BIAS, GELU, BIAS_RES, SILU, RES_SILU)
HAS_RES = (BIAS_RES, RES, DGELU, RES_SILU)

# ---------------------------------------------------------------------------------------------------------------------
# dispatch table: (entry, I, J, K, epilogue, c_f32, res_f32, ldc) -> the path it must take.  The edges of every rule of the plan:
# min_rows (2047 / 2048), few rows (64 / 65), K in {256, 512, 1024, 1536}, J % 128 != 0, fp32 C / residual, ldc % 8 != 0.
# ---------------------------------------------------------------------------------------------------------------------
DISPATCH = [
    ("bf16", 2048, 512, 512, BIAS, 0, 0, None, {"WSP16": 1}),
    ("bf16", 2047, 512, 512, BIAS, 0, 0, None, {"TILED16": 1}),
    ("bf16", 2048, 512, 512, BIAS, 0, 0, 520, {"WSP16": 1}),              # guard columns, ldc % 8 == 0
    ("bf16", 2048, 512, 512, BIAS_RES, 0, 0, 516, {"TILED16": 1}),        # ldc % 8 != 0
    ("bf16", 2048, 512, 512, BIAS, 1, 0, None, {"TILED16": 1}),           # fp32 C
    ("bf16", 2048, 512, 512, BIAS_RES, 0, 1, None, {"TILED16": 1}),       # fp32 residual
    ("bf16", 2048, 384, 512, DGELU, 0, 0, None, {"WSP16": 1}),
    ("bf16", 2048, 512, 512, GELU, 0, 0, None, {"WSP16": 1}),             # with the pre-activation `aux`
    ("bf16", 2048, 256, 512, RES_SILU, 0, 0, None, {"WSP16": 1}),
    ("bf16", 2048, 512, 256, GELU, 0, 0, None, {"WS16": 1}),
    ("bf16", 2047, 512, 256, GELU, 0, 0, None, {"TILED16": 1}),
    ("bf16", 2048, 384, 1024, BIAS_RES, 0, 0, None, {"WS16": 1}),
    ("bf16", 3000, 512, 1536, BIAS, 0, 0, None, {"TILED16": 1}),
    ("bf16", 2048, 200, 512, BIAS, 0, 0, None, {"TILED16": 1}),           # J % 128 != 0
    ("bf16", 64, 512, 256, BIAS_RES, 0, 0, None, {"FEWROW16": 1}),
    ("bf16", 65, 512, 256, BIAS_RES, 0, 0, None, {"TILED16": 1}),
    ("bf16", 64, 512, 192, SILU, 0, 0, None, {"TILED16": 1}),             # K < 256
    ("bf16", 40, 1024, 2048, NONE, 1, 0, None, {"FEWROW16": 1}),
    ("bf16", 33, 96, 320, GELU, 0, 0, 104, {"FEWROW16": 1}),
    ("f32", 2048, 512, 512, BIAS, 1, 0, None, {"WSP32": 1}),
    ("f32", 2047, 512, 512, BIAS, 1, 0, None, {"TILED32": 1}),
    ("f32", 2048, 512, 256, NONE, 1, 0, None, {"WSP32": 1}),
    ("f32", 2048, 512, 1024, BIAS_RES, 1, 0, 520, {"WSP32": 1}),
    ("f32", 2048, 512, 1536, BIAS_RES, 1, 0, None, {"WSP32": 2}),         # two passes over the reduce range
    ("f32", 2048, 512, 1280, BIAS, 1, 0, None, {"TILED32": 1}),
    ("f32", 2048, 200, 512, BIAS, 1, 0, None, {"TILED32": 1}),
    ("f32", 2048, 512, 512, RES, 1, 0, 514, {"TILED32": 1}),              # ldc % 4 != 0
    ("f32", 2048, 256, 512, GELU, 1, 0, None, {"WSP32": 1}),
    ("f32", 2048, 256, 512, DGELU, 1, 0, None, {"WSP32": 1}),
    ("ws", 2047, 576, 768, BIAS_RES, 1, 0, None, {"TAIL32": 1}),          # 288 64x64 tiles: the last round of 32 is cut along K
    ("f32", 2047, 576, 768, BIAS_RES, 1, 0, None, {"TILED32": 1}),
]


def dispatch_uses_aux(entry, epi, expect):
    """test_dispatch_table passes the pre-activation `aux` with every GELU call that a kernel writing it serves."""
    return epi == GELU and (entry != "bf16" or "WSP16" in expect)


# LayerNorm-fold operands / a bf16 `aux` on a shape no kernel that implements them serves: HIG_EUNSUPPORTED (-3), no launch.
# (entry, I, J, K, epilogue, operand): operand "stats_out" = row_stats_out set, "aux" = the pre-activation output asked for
UNSERVED = [
    ("bf16", 2047, 512, 512, BIAS_RES, "stats_out"),
    ("bf16", 2047, 512, 512, GELU, "aux"),
    ("f32", 2048, 200, 512, BIAS_RES, "stats_out"),
]


def desc(entry, I, J, K, epi, X, W, out, ldc, c_f32=0, bias=0, res=0, ldr=None, res_f32=0, aux=0, ldaux=None,
         stats_out=0, stats_in=0, colsum=0):
    """The descriptor of one call from ADDRESSES (device pointers on the GPU, made-up ones for the plan entries; 0 = NULL):
    X (I, K) and W (J, K) dense.  The fp32 entries take the z of DGELU through `aux`."""
    f32 = entry != "bf16"
    d = _lib.GemmDesc() if f32 else _lib.Gemm16Desc()
    d.X, d.ldx, d.Y, d.ldy, d.C, d.ldc = X, K, W, K, out, ldc
    d.I, d.J, d.R, d.epi = I, J, K, epi
    if f32:
        d.prec, d.xf = _lib.PREC_F32, _lib.XF_NONE
    else:
        d.c_f32, d.res_f32 = int(c_f32), int(res_f32)
    d.bias = bias or None
    if res:
        d.res, d.ldr = res, J if ldr is None else ldr
    if aux:
        d.aux, d.ldaux = aux, J if ldaux is None else ldaux
    d.row_stats_out, d.row_stats_in, d.ln_colsum = stats_out or None, stats_in or None, colsum or None
    return d


A = 1 << 24   # made-up operand addresses: distinct, 4 KiB aligned, never dereferenced by a plan entry


def fake_desc(entry, I, J, K, epi, c_f32=0, res_f32=0, ldc=None, ldr=None, ldaux=None, aux=False, fold="", colsum=True,
              inplace=False, c_mis=0, res_mis=0):
    """`desc` with made-up addresses, the operands each epilogue needs present (c_mis / res_mis: bytes C / res are off
    alignment by; inplace: res aliases C)."""
    f32 = entry != "bf16"
    out = 3 * A + c_mis
    need_res = epi in (BIAS_RES, RES, RES_SILU) or (epi == DGELU and not f32)
    res = (out if inplace else 5 * A + res_mis) if need_res else 0
    return desc(entry, I, J, K, epi, 1 * A, 2 * A, out, J if ldc is None else ldc, c_f32=c_f32 or f32,
                bias=4 * A if epi in HAS_BIAS else 0, res=res, ldr=(J if ldc is None else ldc) if inplace else ldr, res_f32=res_f32,
                aux=6 * A if aux or (epi == DGELU and f32) else 0, ldaux=ldaux,
                stats_out=7 * A if fold == "out" else 0, stats_in=7 * A if fold == "in" else 0,
                colsum=8 * A if fold == "in" and colsum else 0)


def plan(entry, d, chip_cus=0):
    """What the library plans for descriptor d of `entry` ('bf16': hig_gemm_bf16, 'f32': hig_gemm, 'ws': hig_gemm_ws):
    (return code, {path name: launches}, variant).  chip_cus 0: the current device's."""
    path, n, variant = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    out = (C.byref(path), C.byref(n), C.byref(variant))
    if entry == "bf16":
        rc = _lib.lib().hig_gemm_bf16_plan(C.byref(d), chip_cus, *out)
    else:
        rc = _lib.lib().hig_gemm_plan(C.byref(d), int(entry == "ws"), chip_cus, *out)
    moved = {PATH_NAME[path.value]: n.value} if n.value else {}
    assert (rc == 0 or not moved) and (moved or path.value == -1), (rc, path.value, n.value)
    return rc, moved, variant.value
