"""bf16-storage path (hig_dims.storage == HIG_STORE_BF16; BASELINE configs 3 and 5: "bf16 storage, fp32 accumulate").
Kernel-level checks are against fp64 references evaluated on the SAME bf16-rounded operands (so only accumulation
order and the final rounding differ); the whole model is held to the fp32 CPU oracle with the error REPORTED and
bounded at the bf16 level (expect ~1e-2, not gated at 1e-3)."""
import ctypes as C
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import hig_amd  # noqa: E402
from hig_amd import _lib  # noqa: E402
from hig_amd.models import gaussian_diffusion as gdm  # noqa: E402
from oracle import denoiser_ref as R  # noqa: E402
from oracle import fill  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bf(t):
    return t.to(torch.bfloat16)


def at16_order(A):
    """The transposed, bf16-rounded context matrices in the element order the library keeps them in (hig_at16_offset,
    csrc/hig_common.h): At[l][c] = bf16(A[c][l]) cut into the 32 (l) x 16 (c) operand blocks of v_mfma_f32_32x32x16_bf16, each
    block 64 lanes x 8 elements, lane = l % 32 + 32 ((c % 16) / 8).  A: (B, H, hd, hd) indexed [c][l]."""
    B, H, hd, _ = A.shape
    At = bf(A.transpose(2, 3)).contiguous()                                   # [l][c]
    v = At.view(B, H, hd // 32, 32, hd // 16, 2, 8)                           # (lb, l32, ks, half, j)
    return v.permute(0, 1, 2, 4, 5, 3, 6).contiguous().view(B, H, hd, hd)     # (lb, ks, half, l32, j)


EPIS = {"none": _lib.EPI_NONE, "bias": _lib.EPI_BIAS, "gelu": _lib.EPI_BIAS_GELU, "res": _lib.EPI_BIAS_RES,
        "silu": _lib.EPI_BIAS_SILU, "res_silu": _lib.EPI_BIAS_RES_SILU}


# (I, J, R, epi, c_f32, res_f32, the GEMM path that must serve the case)
GEMM16_CASES = [
    (300, 200, 64, "bias", 0, 0, "TILED16"), (128, 128, 512, "none", 0, 0, "TILED16"), (1000, 1024, 512, "gelu", 0, 0, "TILED16"),
    (777, 512, 1024, "res", 0, 0, "TILED16"), (64, 2048, 2048, "res_silu", 0, 1, "FEWROW16"), (32, 2048, 512, "silu", 0, 0, "FEWROW16"),
    (500, 150, 512, "bias", 1, 0, "TILED16"), (6272, 1536, 512, "bias", 0, 0, "WSP16"), (45, 96, 96, "res", 1, 1, "TILED16"),
    (2464, 1024, 256, "bias", 0, 0, "WS16"), (70, 264, 32, "gelu", 0, 0, "TILED16"), (12544, 512, 512, "res", 0, 0, "WSP16"),
    # many rows at K = 512 (the weight-stationary kernel with specialised waves, gemm_wsp16.hip), incl. ragged edges in both
    # directions: N % 128 != 0 and an fp32 output leave it to the tiled kernel
    (12544, 1024, 512, "gelu", 0, 0, "WSP16"), (12544, 1536, 512, "bias", 0, 0, "WSP16"), (12500, 1000, 512, "res", 0, 0, "TILED16"),
    (9600, 1024, 1024, "res_silu", 1, 1, "TILED16"),
    # a handful of rows (gemm_fewrow16_kernel: <= 64 rows, N % 32 == 0, K % 64 == 0, K >= 256): one and two row blocks,
    # every epilogue, bf16 / fp32 outputs and residuals, the in-place residual
    (1, 512, 256, "bias", 0, 0, "FEWROW16"), (33, 96, 320, "res", 0, 0, "FEWROW16"), (40, 2048, 2048, "none", 1, 0, "FEWROW16"),
    (7, 64, 2048, "gelu", 0, 0, "FEWROW16"), (64, 1024, 512, "res", 1, 0, "FEWROW16"), (32, 2048, 2048, "res_silu", 0, 1, "FEWROW16"),
    (17, 160, 1024, "silu", 1, 0, "FEWROW16"),
    # the weight-stationary kernels (>= 2048 rows, N % 128 == 0, bf16 out): gemm_ws16.hip at K = 256 / 1024 (every epilogue,
    # both panel widths, the K-split variant), gemm_wsp16.hip at K = 512; ragged row counts, row counts that leave some
    # workgroups of an XCD without a tile
    (6272, 512, 1024, "bias", 0, 0, "WS16"), (9600, 1024, 1024, "res", 0, 0, "WS16"), (4000, 3072, 1024, "gelu", 0, 0, "WS16"),
    (6250, 512, 512, "res", 0, 0, "WSP16"), (2049, 256, 256, "gelu", 0, 0, "WS16"), (3001, 384, 512, "res_silu", 0, 0, "WSP16"),
    (2100, 1536, 512, "silu", 0, 0, "WSP16"), (12544, 512, 512, "none", 0, 0, "WSP16"), (2464, 1024, 256, "res", 0, 0, "WS16"),
    (6272, 1024, 512, "gelu", 0, 0, "WSP16"), (2177, 640, 1024, "res", 0, 0, "WS16"),
    # K = 1024 with a residual: the residual tile lands in the staging buffer itself (no LDS left for its own)
    (6250, 512, 1024, "res_silu", 0, 0, "WS16"), (2050, 128, 1024, "res", 0, 0, "WS16"), (12544, 1024, 1024, "res", 0, 0, "WS16")]
GEMM16_PATH = {case[:6]: case[6] for case in GEMM16_CASES}


@pytest.mark.parametrize("I,J,R,epi,c_f32,res_f32", [case[:6] for case in GEMM16_CASES])
def test_gemm_bf16_all_epilogues_and_ragged_shapes(I, J, R, epi, c_f32, res_f32):
    g = torch.Generator().manual_seed(I * 7 + J * 3 + R)
    X, Y = bf(torch.randn(I, R, generator=g)), bf(torch.randn(J, R, generator=g) / R ** 0.5)
    bias = torch.randn(J, generator=g)
    res = torch.randn(I, J, generator=g)
    res = res if res_f32 else bf(res)
    Xd, Yd, bd, rd = X.to(DEV), Y.to(DEV), bias.to(DEV), res.to(DEV)
    out = torch.full((I, J), float("nan"), device=DEV, dtype=torch.float32 if c_f32 else torch.bfloat16)
    d = _lib.Gemm16Desc()
    d.X, d.ldx, d.Y, d.ldy, d.C, d.ldc, d.c_f32 = Xd.data_ptr(), R, Yd.data_ptr(), R, out.data_ptr(), J, c_f32
    d.I, d.J, d.R, d.epi = I, J, R, EPIS[epi]
    d.bias = bd.data_ptr() if epi != "none" else None
    if "res" in epi:
        d.res, d.ldr, d.res_f32 = rd.data_ptr(), J, res_f32
    path = GEMM16_PATH[(I, J, R, epi, c_f32, res_f32)]
    served = getattr(_lib, "GEMM_PATH_" + path)

    def launch():   # ... on the kernel this case is for (hig_gemm_path_launches)
        before = _lib.lib().hig_gemm_path_launches(served)
        _lib.check(_lib.lib().hig_gemm_bf16(C.byref(d), _lib.stream_ptr()))
        assert _lib.lib().hig_gemm_path_launches(served) - before == 1, "not served by the %s path" % path
    launch()
    if "res" in epi and not c_f32 and not res_f32:
        # the residual stream is updated IN PLACE by the stylization-out GEMMs (C aliases res)
        inplace = rd.clone()
        d.C, d.res = inplace.data_ptr(), inplace.data_ptr()
        launch()
        assert torch.equal(inplace, out)
        d.C, d.res = out.data_ptr(), rd.data_ptr()
    ref = X.double() @ Y.double().t()
    if epi != "none":
        ref = ref + bias.double()
    if "res" in epi:
        ref = ref + res.double()
    if epi == "gelu":
        ref = torch.nn.functional.gelu(ref)
    if "silu" in epi:
        ref = torch.nn.functional.silu(ref)
    assert torch.isfinite(out.float()).all()
    e = rel(out.float(), ref)
    assert e < (2e-6 if c_f32 else 3e-3), e           # fp32 out: accumulation order only; bf16 out: one rounding (2^-9)
    if not c_f32:   # the bf16 result must be the correctly rounded fp32 value almost everywhere
        exact = bf(ref.float()).float()
        assert (out.float().cpu() != exact).float().mean().item() < 0.02


@pytest.mark.parametrize("nwj", ["2", "4", "8", "44"])
@pytest.mark.parametrize("I,J,R,epi", [(6272, 512, 512, "res"), (12544, 1024, 512, "gelu"), (3001, 768, 512, "bias"),
                                       (2049, 256, 256, "silu"), (7000, 1536, 512, "none")])
def test_gemm_ws16_every_variant(I, J, R, epi, nwj, monkeypatch):
    """The three shapes of the weight-stationary kernel (HIG_BF16_WS_NWJ: 8 waves x 32 columns, 4 x 32, 4 x 64), each
    forced on shapes the default rule would give to another one.  The knob is read once per process, so the forced
    runs happen in a child process."""
    import subprocess
    code = (
        "import sys, torch, ctypes as C; sys.path.insert(0, %r); from hig_amd import _lib\n"
        "I, J, R, epi = %d, %d, %d, %r\n"
        "g = torch.Generator().manual_seed(I + J + R)\n"
        "X = torch.randn(I, R, generator=g).to(torch.bfloat16); Y = (torch.randn(J, R, generator=g) / R ** 0.5).to(torch.bfloat16)\n"
        "b = torch.randn(J, generator=g); r = torch.randn(I, J, generator=g).to(torch.bfloat16)\n"
        "Xd, Yd, bd, rd = X.cuda(), Y.cuda(), b.cuda(), r.cuda()\n"
        "out = torch.full((I, J), float('nan'), device='cuda', dtype=torch.bfloat16)\n"
        "d = _lib.Gemm16Desc()\n"
        "d.X, d.ldx, d.Y, d.ldy, d.C, d.ldc, d.c_f32 = Xd.data_ptr(), R, Yd.data_ptr(), R, out.data_ptr(), J, 0\n"
        "d.I, d.J, d.R = I, J, R\n"
        "d.epi = {'none': _lib.EPI_NONE, 'bias': _lib.EPI_BIAS, 'gelu': _lib.EPI_BIAS_GELU, 'res': _lib.EPI_BIAS_RES, 'silu': _lib.EPI_BIAS_SILU}[epi]\n"
        "d.bias = bd.data_ptr() if epi != 'none' else None\n"
        "if epi == 'res': d.res, d.ldr, d.res_f32 = rd.data_ptr(), J, 0\n"
        "n0 = _lib.lib().hig_gemm_path_launches(_lib.GEMM_PATH_WS16)\n"
        "for _ in range(3): _lib.check(_lib.lib().hig_gemm_bf16(C.byref(d), _lib.stream_ptr()))\n"
        "assert _lib.lib().hig_gemm_path_launches(_lib.GEMM_PATH_WS16) - n0 == 3, 'not served by gemm_ws16'\n"
        "ref = X.double() @ Y.double().t()\n"
        "if epi != 'none': ref = ref + b.double()\n"
        "if epi == 'res': ref = ref + r.double()\n"
        "if epi == 'gelu': ref = torch.nn.functional.gelu(ref)\n"
        "if epi == 'silu': ref = torch.nn.functional.silu(ref)\n"
        "o = out.float().cpu().double()\n"
        "assert torch.isfinite(o).all()\n"
        "e = ((o - ref).norm() / ref.norm()).item(); assert e < 3e-3, e\n"
        "assert (out.float().cpu() != ref.float().to(torch.bfloat16).float()).float().mean().item() < 0.02\n"
        "print('ok', e)\n" % (ROOT, I, J, R, epi))
    env = dict(os.environ, HIG_BF16_WS_NWJ=nwj)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("I,J,d", [(6272, 1536, 512), (12544, 512, 512), (2049, 512, 512), (3000, 1536, 512),
                                   (9600, 3072, 1024), (2400, 1024, 1024), (2077, 3072, 1024)])
def test_layernorm_folded_into_the_weight_stationary_gemm(I, J, d):
    """LayerNorm(x) W^T + b without a LayerNorm kernel (hig_gemm16_desc.row_stats_*): the GEMM that PRODUCES x also writes
    (sum, centred sum of squares) of its bf16 output rows per 128-column panel; the consumer runs on the un-normalised x with
    W' = gamma (.) W and applies rstd / mean / column sums / bias' in its epilogue.  Checked: the statistics against the
    producer's own output, the consumer against the fp64 LayerNorm + Linear of the same bf16 x (transformer.py:108-110).
    d = 1024: the K-split variants of the kernel (eight panels per row; the consumer with one staging buffer)."""
    g = torch.Generator().manual_seed(I + J)
    L = _lib.lib()
    # producer: h = a Wo^T + bo + h_old (a stylization-out GEMM), with statistics
    a16, Wo = bf(torch.randn(I, d, generator=g)), bf(torch.randn(d, d, generator=g) / d ** 0.5)
    bo = torch.randn(d, generator=g)
    hold = bf(torch.randn(I, d, generator=g) * 3 + 1.5)               # (a mean far from zero: the fold must cancel it)
    ad, Wod, bod = a16.to(DEV), Wo.to(DEV), bo.to(DEV)
    h = hold.to(DEV).clone()
    stats = torch.full((I, d // 128, 2), float("nan"), device=DEV)
    dsc = _lib.Gemm16Desc()
    dsc.X, dsc.ldx, dsc.Y, dsc.ldy, dsc.C, dsc.ldc, dsc.c_f32 = ad.data_ptr(), d, Wod.data_ptr(), d, h.data_ptr(), d, 0
    dsc.I, dsc.J, dsc.R, dsc.epi, dsc.bias = I, d, d, _lib.EPI_BIAS_RES, bod.data_ptr()
    dsc.res, dsc.ldr, dsc.res_f32 = h.data_ptr(), d, 0
    dsc.row_stats_out = stats.data_ptr()
    _lib.check(L.hig_gemm_bf16(C.byref(dsc), _lib.stream_ptr()))
    ref_h = a16.double() @ Wo.double().t() + bo.double() + hold.double()
    assert rel(h.float(), ref_h) < 3e-3
    hp = h.float().double().cpu().view(I, d // 128, 128)
    assert rel(stats[:, :, 0], hp.sum(-1)) < 1e-5 and rel(stats[:, :, 1], ((hp - hp.mean(-1, keepdim=True)) ** 2).sum(-1)) < 1e-5
    # consumer: LN(h) W^T + b through the folded operands
    gamma, beta = 1 + 0.2 * torch.randn(d, generator=g), 0.3 * torch.randn(d, generator=g)
    W, b = torch.randn(J, d, generator=g) / d ** 0.5, torch.randn(J, generator=g)
    Wp = bf(W * gamma[None, :])
    cs, bp = Wp.float().sum(1), b + W @ beta
    out = torch.full((I, J), float("nan"), device=DEV, dtype=torch.bfloat16)
    Wpd, csd, bpd = Wp.to(DEV), cs.to(DEV), bp.to(DEV)
    c2 = _lib.Gemm16Desc()
    c2.X, c2.ldx, c2.Y, c2.ldy, c2.C, c2.ldc, c2.c_f32 = h.data_ptr(), d, Wpd.data_ptr(), d, out.data_ptr(), J, 0
    c2.I, c2.J, c2.R, c2.epi, c2.bias = I, J, d, _lib.EPI_BIAS, bpd.data_ptr()
    c2.row_stats_in, c2.ln_colsum = stats.data_ptr(), csd.data_ptr()
    _lib.check(L.hig_gemm_bf16(C.byref(c2), _lib.stream_ptr()))
    hd = h.float().double().cpu()
    ref = torch.nn.functional.layer_norm(hd, (d,), gamma.double(), beta.double(), 1e-5) @ W.double().t() + b.double()
    assert torch.isfinite(out.float()).all()
    assert rel(out.float(), ref) < 4e-3
    # shapes the kernel does not serve must fail loudly, not silently drop the LayerNorm
    c2.I = 100
    with pytest.raises(RuntimeError, match="LayerNorm-fold"):
        _lib.check(L.hig_gemm_bf16(C.byref(c2), _lib.stream_ptr()))


def test_gemm_bf16_rejects_what_it_cannot_run():
    X = torch.zeros(64, 48, device=DEV, dtype=torch.bfloat16)
    out = torch.zeros(64, 64, device=DEV, dtype=torch.bfloat16)
    d = _lib.Gemm16Desc()
    d.X, d.ldx, d.Y, d.ldy, d.C, d.ldc = X.data_ptr(), 48, X.data_ptr(), 48, out.data_ptr(), 64
    d.I, d.J, d.R, d.epi = 64, 64, 48, _lib.EPI_NONE
    with pytest.raises(RuntimeError, match="multiple of 32"):
        _lib.check(_lib.lib().hig_gemm_bf16(C.byref(d), _lib.stream_ptr()))


@pytest.mark.parametrize("rows,n,mod,x_f32", [(392, 512, True, 0), (392, 512, False, 0), (154, 256, False, 1),
                                               (50, 1024, True, 0), (7, 64, True, 0),
                                               # (>= 32 768 rows: four rows per wave, the per-column vectors in registers)
                                               (33005, 512, True, 0), (32768, 256, False, 0), (40001, 1024, True, 0)])
def test_layernorm_and_stylization_front_bf16(rows, n, mod, x_f32):
    g = torch.Generator().manual_seed(rows + n)
    x = torch.randn(rows, n, generator=g) * 2 + 0.3
    x = x if x_f32 else bf(x)
    gamma, beta = 1 + 0.1 * torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)
    rps = 7
    nb = (rows + rps - 1) // rps
    ss = 0.3 * torch.randn(nb, 2 * n, generator=g)
    out = torch.full((rows, n), float("nan"), device=DEV, dtype=torch.bfloat16)
    xd, gd_, bd, sd = x.to(DEV), gamma.to(DEV), beta.to(DEV), ss.to(DEV)
    _lib.check(_lib.lib().hig_ln_bf16(_lib.ptr(xd), x_f32, n, rows, n, _lib.ptr(gd_), _lib.ptr(bd),
                                      _lib.ptr(sd) if mod else None, 2 * n, n, rps, _lib.ptr(out), n, _lib.stream_ptr()))
    ref = torch.nn.functional.layer_norm(x.double(), (n,), gamma.double(), beta.double(), 1e-5)
    if mod:
        sc = ss[:, :n].double().repeat_interleave(rps, 0)[:rows]
        sh = ss[:, n:].double().repeat_interleave(rps, 0)[:rows]
        ref = torch.nn.functional.silu(ref * (1 + sc) + sh)
    assert rel(out.float(), ref) < 3e-3


@pytest.mark.parametrize("hd,H,B,T", [(64, 8, 4, 196), (128, 4, 3, 300), (64, 2, 40, 77), (64, 8, 64, 50)])
def test_linear_attention_bf16_io_matches_fp32_kernels(hd, H, B, T):
    """bf16 loads / stores against the fp32 entry points fed the bf16-rounded values: the context build is the same arithmetic
    (bit-equal); `apply` runs its product on the bf16 matrix cores (p and A rounded to bf16, fp32 accumulation, fp32 softmax):
    equal to the operand rounding."""
    d = H * hd
    g = torch.Generator().manual_seed(hd + B + T)
    qkv16 = bf(torch.randn(B * T, 3 * d, generator=g)).to(DEV)
    qkv32 = qkv16.float()
    lens = torch.randint(1, T + 1, (B,), generator=g).to(DEV)
    L = _lib.lib()
    scr = torch.zeros(L.hig_linattn_ctx_scratch_floats(B, T, H, hd), device=DEV)
    A16, A32 = torch.empty(B, H, hd, hd, device=DEV), torch.empty(B, H, hd, hd, device=DEV)
    k16, k32 = torch.empty(B, d, 2, device=DEV), torch.empty(B, d, 2, device=DEV)
    At = torch.full((B, H, hd, hd), float("nan"), device=DEV, dtype=torch.bfloat16)
    _lib.check(L.hig_linattn_ctx_bf16(qkv16.data_ptr() + 2 * d, qkv16.data_ptr() + 4 * d, 3 * d, B, T, H, hd, _lib.ptr(lens),
                                      _lib.ptr(A16), _lib.ptr(k16), _lib.ptr(scr), _lib.ptr(At), _lib.stream_ptr()))
    assert torch.equal(At, at16_order(A16))     # the transposed, rounded copy for linattn16.hip
    _lib.check(L.hig_linattn_ctx(qkv32.data_ptr() + 4 * d, qkv32.data_ptr() + 8 * d, 3 * d, B, T, H, hd, _lib.ptr(lens),
                                 _lib.ptr(A32), _lib.ptr(k32), _lib.ptr(scr), _lib.stream_ptr()))
    assert torch.equal(A16, A32) and torch.equal(k16, k32)          # identical arithmetic on identical values
    y16 = torch.full((B * T, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    y32 = torch.empty(B * T, d, device=DEV)
    _lib.check(L.hig_linattn_apply_bf16(_lib.ptr(qkv16), 3 * d, _lib.ptr(A16), _lib.ptr(y16), d, B, T, H, hd, _lib.stream_ptr()))
    _lib.check(L.hig_linattn_apply(_lib.ptr(qkv32), 3 * d, _lib.ptr(A32), _lib.ptr(y32), d, B, T, H, hd, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.isfinite(y16.float()).all()
    assert rel(y16.float(), y32) < 5e-3, rel(y16.float(), y32)


@pytest.mark.parametrize("hd,H,B,T", [(64, 8, 5, 196), (128, 8, 2, 300), (64, 4, 3, 33), (128, 4, 2, 64)])
def test_fused_apply_stylization_front_matches_the_two_kernel_sequence(hd, H, B, T):
    """hig_linattn_apply_sty_bf16 == hig_linattn_apply (fp32 y) followed by the stylization front: the fused kernel
    keeps y in fp32 registers, so it is compared with the fp32 apply + an fp64 LayerNorm / modulation / SiLU."""
    d = H * hd
    g = torch.Generator().manual_seed(hd + H + B + T)
    q16 = bf(torch.randn(B * T, d, generator=g) * 2).to(DEV)
    A = (torch.randn(B, H, hd, hd, generator=g) * 0.5).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
    ss = (0.3 * torch.randn(B, 2 * d, generator=g)).to(DEV)
    L = _lib.lib()
    out = torch.full((B * T, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    _lib.check(L.hig_linattn_apply_sty_bf16(_lib.ptr(q16), d, _lib.ptr(A), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ss),
                                            2 * d, d, _lib.ptr(out), d, B, T, H, hd, _lib.stream_ptr()))
    y32 = torch.empty(B * T, d, device=DEV)
    q32 = q16.float()
    _lib.check(L.hig_linattn_apply(_lib.ptr(q32), d, _lib.ptr(A), _lib.ptr(y32), d, B, T, H, hd, _lib.stream_ptr()))
    ref = torch.nn.functional.layer_norm(y32.double().cpu(), (d,), gamma.double().cpu(), beta.double().cpu(), 1e-5)
    sc = ss[:, :d].double().cpu().repeat_interleave(T, 0)
    sh = ss[:, d:].double().cpu().repeat_interleave(T, 0)
    ref = torch.nn.functional.silu(ref * (1 + sc) + sh)
    assert torch.isfinite(out.float()).all()
    assert rel(out.float(), ref) < 3e-3
    assert (out.float().cpu() != bf(ref.float()).float()).float().mean().item() < 0.03   # correctly rounded almost everywhere


@pytest.mark.parametrize("H,B,T,hd", [(8, 4, 196, 64), (8, 32, 196, 64), (2, 40, 77, 64), (8, 3, 300, 64), (4, 5, 1, 64), (8, 2, 64, 64),
                                      (8, 2, 65, 64), (8, 4, 300, 128), (4, 3, 77, 128), (2, 5, 129, 128), (8, 2, 1, 128)])
def test_context_build_on_the_bf16_matrix_cores(H, B, T, hd):
    """hig_linattn_ctx_mm16 (csrc/linattn16.hip: online column softmax over row chunks, k^T v on v_mfma_f32_32x32x16_bf16 with
    transpose reads) against the definition in fp64 on the same bf16 K / V -- exp(K - max) and V are rounded to bf16 for the
    product, so A is held at the bf16 level, the statistics (column max, column sum) at the fp32 level -- with ragged and
    zero lengths, one and many chunks, and the transposed bf16 copy checked against the kernel's own A."""
    d = H * hd
    g = torch.Generator().manual_seed(H + B + T)
    qkv16 = bf(torch.randn(B * T, 3 * d, generator=g) * 1.5).to(DEV)
    lens = torch.randint(0, T + 1, (B,), generator=g)
    lens[0] = T
    L = _lib.lib()
    A = torch.full((B, H, hd, hd), float("nan"), device=DEV)
    kst = torch.full((B, d, 2), float("nan"), device=DEV)
    At = torch.full((B, H, hd, hd), float("nan"), device=DEV, dtype=torch.bfloat16)
    _lib.check(L.hig_linattn_ctx_mm16(qkv16.data_ptr() + 2 * d, qkv16.data_ptr() + 4 * d, 3 * d, B, T, H, hd, _lib.ptr(lens.to(DEV)),
                                      _lib.ptr(A), _lib.ptr(kst), _lib.ptr(At), _lib.stream_ptr()))
    x = qkv16.double().cpu().view(B, T, 3, H, hd)
    K, V = x[:, :, 1], x[:, :, 2]
    mask = (torch.arange(T)[None, :] < lens[:, None])[:, :, None, None]
    Km = torch.where(mask, K, torch.full_like(K, float("-inf")))
    mx = Km.max(dim=1).values                                            # (B, H, hd)
    p = torch.where(mask, torch.exp(K - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))[:, None]), torch.zeros_like(K))
    s = p.sum(dim=1)
    ref = torch.einsum("bthc,bthl->bhcl", p, V) / torch.where(s > 0, s, torch.ones_like(s))[..., None]
    Ac = A.double().cpu()
    assert torch.isfinite(Ac).all()
    live = lens > 0
    assert rel(Ac[live], ref[live]) < 4e-3
    assert Ac[~live].abs().max().item() == 0.0 if (~live).any() else True      # empty samples: zero context
    ks = kst.double().cpu().view(B, H, hd, 2)
    assert torch.equal(ks[live][..., 0], mx[live])                            # running maximum == column maximum
    assert rel(ks[live][..., 1], s[live]) < 1e-5
    assert torch.equal(At.cpu(), at16_order(A).cpu())


@pytest.mark.parametrize("H,B,T,hd", [(8, 5, 196, 64), (8, 32, 196, 64), (4, 3, 33, 64), (8, 2, 1, 64), (4, 7, 91, 64),
                                      (8, 3, 300, 128), (4, 5, 45, 128), (8, 2, 31, 128)])
def test_fused_apply_stylization_front_on_the_bf16_matrix_cores(H, B, T, hd):
    """hig_linattn_apply_sty_mm16 (csrc/linattn16.hip): softmax(q) and the context matrices are rounded to bf16 for the
    hd x hd products (fp32 accumulate) -- the rounding the bf16 storage mode applies to every other matrix operand.  Held
    (a) to exactly that arithmetic in fp64 (bf16-rounded p and A, fp64 products, LayerNorm / modulation / SiLU): only the
    accumulation order, the fp32 softmax and the final rounding differ; (b) to the unrounded reference at the bf16 level."""
    d = H * hd
    g = torch.Generator().manual_seed(H + B + T)
    q16 = bf(torch.randn(B * T, d, generator=g) * 2).to(DEV)
    A = (torch.randn(B, H, hd, hd, generator=g) * 0.5).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
    ss = (0.3 * torch.randn(B, 2 * d, generator=g)).to(DEV)
    out = torch.full((B * T, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    At = at16_order(A)
    _lib.check(_lib.lib().hig_linattn_apply_sty_mm16(_lib.ptr(q16), d, _lib.ptr(At), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ss),
                                                     2 * d, d, _lib.ptr(out), d, B, T, H, hd, _lib.stream_ptr()))
    q = q16.double().cpu().view(B, T, H, hd)
    p = torch.softmax(q, dim=-1)

    def front(y):
        y = torch.nn.functional.layer_norm(y.reshape(B * T, d), (d,), gamma.double().cpu(), beta.double().cpu(), 1e-5)
        sc = ss[:, :d].double().cpu().repeat_interleave(T, 0)
        sh = ss[:, d:].double().cpu().repeat_interleave(T, 0)
        return torch.nn.functional.silu(y * (1 + sc) + sh)

    Ad = A.double().cpu()
    ref16 = front(torch.einsum("bthc,bhcl->bthl", bf(p.float()).double(), bf(Ad.float()).double()))
    ref = front(torch.einsum("bthc,bhcl->bthl", p, Ad))
    assert torch.isfinite(out.float()).all()
    assert rel(out.float(), ref16) < 3e-3
    assert (out.float().cpu() != bf(ref16.float()).float()).float().mean().item() < 0.05
    assert rel(out.float(), ref) < 1e-2
    # the training form: the same activated rows, bit for bit, and y = softmax(q) . A itself as a second output
    out2 = torch.full((B * T, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    y16 = torch.full((B * T, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    _lib.check(_lib.lib().hig_linattn_apply_sty_mm16_y(_lib.ptr(q16), d, _lib.ptr(At), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ss),
                                                       2 * d, d, _lib.ptr(out2), d, _lib.ptr(y16), d, B, T, H, hd, _lib.stream_ptr()))
    assert torch.equal(out2, out)
    yref = torch.einsum("bthc,bhcl->bthl", bf(p.float()).double(), bf(Ad.float()).double()).reshape(B * T, d)
    assert torch.isfinite(y16.float()).all() and rel(y16.float(), yref) < 3e-3


@pytest.mark.parametrize("B,T,with_stats", [(32, 196, True), (5, 91, False), (3, 1, True), (16, 196, False), (40, 196, True),
                                            (64, 50, True), (96, 33, False)])
def test_attention_output_projection_fused_into_the_apply_kernel(B, T, with_stats):
    """hig_attn_out16 = hig_linattn_apply_sty_mm16, then the stylization-out GEMM with the residual update (and the row
    statistics of the LayerNorm fold), as ONE launch: a workgroup keeps its 32 activated rows in LDS and streams the weight in
    matrix-core operand order.  Same products in the same order as the two-launch sequence: h and the statistics must match it
    bit for bit."""
    H, hd, d = 8, 64, 512
    M = B * T
    g = torch.Generator().manual_seed(B * 1000 + T)
    q16 = bf(torch.randn(M, 3 * d, generator=g) * 2).to(DEV)
    A = (torch.randn(B, H, hd, hd, generator=g) * 0.5).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
    ss = (0.3 * torch.randn(B, 2 * d, generator=g)).to(DEV)
    W = bf(torch.randn(d, d, generator=g) / d ** 0.5).to(DEV)
    bias = torch.randn(d, generator=g).to(DEV)
    h0 = bf(torch.randn(M, d, generator=g) * 2).to(DEV)
    At = at16_order(A)
    L = _lib.lib()
    # reference sequence: apply + stylization front, then the weight-stationary (or tiled) GEMM with the in-place residual
    a = torch.full((M, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    _lib.check(L.hig_linattn_apply_sty_mm16(_lib.ptr(q16), 3 * d, _lib.ptr(At), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ss),
                                            2 * d, d, _lib.ptr(a), d, B, T, H, hd, _lib.stream_ptr()))
    h_ref = h0.clone()
    st_ref = torch.full((M, 4, 2), float("nan"), device=DEV)
    dsc = _lib.Gemm16Desc()
    dsc.X, dsc.ldx, dsc.Y, dsc.ldy, dsc.C, dsc.ldc, dsc.c_f32 = a.data_ptr(), d, W.data_ptr(), d, h_ref.data_ptr(), d, 0
    dsc.I, dsc.J, dsc.R, dsc.epi, dsc.bias = M, d, d, _lib.EPI_BIAS_RES, bias.data_ptr()
    dsc.res, dsc.ldr, dsc.res_f32 = h_ref.data_ptr(), d, 0
    if with_stats and M >= 2048:
        dsc.row_stats_out = st_ref.data_ptr()
    _lib.check(L.hig_gemm_bf16(C.byref(dsc), _lib.stream_ptr()))
    # fused
    Wf = torch.full((d * d,), float("nan"), device=DEV, dtype=torch.bfloat16)
    _lib.check(L.hig_weight_frag16(_lib.ptr(W), d, d, d, _lib.ptr(Wf), _lib.stream_ptr()))
    assert torch.equal(Wf, hig_amd.MotionTransformer._frag16(W).reshape(-1))
    h = h0.clone()
    st = torch.full((M, 4, 2), float("nan"), device=DEV)
    _lib.check(L.hig_attn_out16(_lib.ptr(q16), 3 * d, _lib.ptr(At), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ss), 2 * d, d,
                                _lib.ptr(Wf), _lib.ptr(bias), _lib.ptr(h), d, _lib.ptr(st) if with_stats else None, B, T, H, hd,
                                _lib.stream_ptr()))
    assert torch.isfinite(h.float()).all()
    # (the stand-alone GEMM -- gemm_wsp16.hip from 2048 rows up, else the tiled kernel -- sums the products of a row in another
    # order than the fused kernel and adds its bias after them: equal up to the last rounding, not bit for bit)
    assert (h != h_ref).float().mean().item() < 0.02 and rel(h.float(), h_ref.float()) < 2e-3
    if with_stats:
        hp = h.float().double().cpu().view(M, 4, 128)
        assert rel(st[:, :, 0], hp.sum(-1)) < 1e-5 and rel(st[:, :, 1], ((hp - hp.mean(-1, keepdim=True)) ** 2).sum(-1)) < 1e-5
        if M >= 2048:   # the stand-alone GEMM's statistics describe ITS rounded rows: close, not identical
            assert rel(st, st_ref) < 5e-3


@pytest.mark.parametrize("B,T", [(32, 196), (5, 91), (3, 1), (64, 50)])
def test_fused_attention_block_against_its_fp64_definition(B, T):
    """hig_attn_out16 against the DEFINITION of the block it replaces, in fp64 on the same bf16 operands (not against the
    two-launch HIP sequence): softmax_hd(q) . A -> LayerNorm -> (1 + scale), shift -> SiLU -> Linear + bias + residual
    (transformer.py:111-118 then :81-86).  The kernel rounds softmax(q) and A to bf16 for the hd x hd products and the
    activated rows to bf16 for the projection (the storage mode's rounding of every matrix operand); the reference does the
    same roundings, everything else in fp64.  The unrounded definition is held at the bf16 level beside it."""
    H, hd, d = 8, 64, 512
    M = B * T
    g = torch.Generator().manual_seed(B * 31 + T)
    q16 = bf(torch.randn(M, 3 * d, generator=g) * 2).to(DEV)
    A = (torch.randn(B, H, hd, hd, generator=g) * 0.5).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
    ss = (0.3 * torch.randn(B, 2 * d, generator=g)).to(DEV)
    W = bf(torch.randn(d, d, generator=g) / d ** 0.5).to(DEV)
    bias = torch.randn(d, generator=g).to(DEV)
    h0 = bf(torch.randn(M, d, generator=g) * 2).to(DEV)
    At = at16_order(A)
    Wf = hig_amd.MotionTransformer._frag16(W).reshape(-1).contiguous()
    h = h0.clone()
    st = torch.full((M, 4, 2), float("nan"), device=DEV)
    _lib.check(_lib.lib().hig_attn_out16(_lib.ptr(q16), 3 * d, _lib.ptr(At), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ss), 2 * d, d,
                                         _lib.ptr(Wf), _lib.ptr(bias), _lib.ptr(h), d, _lib.ptr(st), B, T, H, hd, _lib.stream_ptr()))
    q = q16[:, :d].double().cpu().view(B, T, H, hd)
    p = torch.softmax(q, dim=-1)
    Ad = A.double().cpu()
    sc = ss[:, :d].double().cpu().repeat_interleave(T, 0)
    sh = ss[:, d:].double().cpu().repeat_interleave(T, 0)

    def block(p_, A_, round_a):
        y = torch.einsum("bthc,bhcl->bthl", p_, A_).reshape(M, d)
        a = torch.nn.functional.silu(torch.nn.functional.layer_norm(y, (d,), gamma.double().cpu(), beta.double().cpu(), 1e-5) * (1 + sc) + sh)
        if round_a:
            a = bf(a.float()).double()
        return a @ W.double().cpu().t() + bias.double().cpu() + h0.double().cpu()

    ref16 = block(bf(p.float()).double(), bf(Ad.float()).double(), True)
    ref = block(p, Ad, False)
    assert torch.isfinite(h.float()).all()
    e16, e = rel(h.float(), ref16), rel(h.float(), ref)
    print("hig_attn_out16 B=%d T=%d: rel-L2 %.2e vs its own roundings in fp64, %.2e vs the unrounded definition" % (B, T, e16, e))
    assert e16 < 3e-3 and e < 8e-3
    assert (h.float().cpu() != bf(ref16.float()).float()).float().mean().item() < 0.06   # correctly rounded almost everywhere
    hp = h.float().double().cpu().view(M, 4, 128)
    assert rel(st[:, :, 0], hp.sum(-1)) < 1e-5


@pytest.mark.parametrize("B,T,with_stats", [(32, 196, True), (5, 91, False), (3, 1, True), (48, 196, True), (70, 65, False)])
def test_stylization_block_of_stored_rows_as_one_kernel(B, T, with_stats):
    """hig_rows_out16: LayerNorm -> (1 + scale) / shift -> SiLU -> Linear -> residual add of the stylization block behind the
    FFN (transformer.py:81-86) as one launch, against the definition in fp64 on the same bf16 operands and against the
    two-launch sequence (hig_ln_bf16 + hig_gemm_bf16) it replaces."""
    d = 512
    M = B * T
    g = torch.Generator().manual_seed(B * 77 + T)
    y16 = bf(torch.randn(M, d, generator=g) * 2 + 0.3).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
    ss = (0.3 * torch.randn(B, 2 * d, generator=g)).to(DEV)
    W = bf(torch.randn(d, d, generator=g) / d ** 0.5).to(DEV)
    bias = torch.randn(d, generator=g).to(DEV)
    h0 = bf(torch.randn(M, d, generator=g) * 2).to(DEV)
    L = _lib.lib()
    Wf = hig_amd.MotionTransformer._frag16(W).reshape(-1).contiguous()
    h = h0.clone()
    st = torch.full((M, 4, 2), float("nan"), device=DEV)
    _lib.check(L.hig_rows_out16(_lib.ptr(y16), d, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ss), 2 * d, d, _lib.ptr(Wf), _lib.ptr(bias),
                                _lib.ptr(h), d, _lib.ptr(st) if with_stats else None, B, T, d, _lib.stream_ptr()))
    # the two launches it replaces
    a = torch.empty(M, d, device=DEV, dtype=torch.bfloat16)
    _lib.check(L.hig_ln_bf16(_lib.ptr(y16), 0, d, M, d, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ss), 2 * d, d, T, _lib.ptr(a), d,
                             _lib.stream_ptr()))
    h2 = h0.clone()
    dsc = _lib.Gemm16Desc()
    dsc.X, dsc.ldx, dsc.Y, dsc.ldy, dsc.C, dsc.ldc, dsc.c_f32 = a.data_ptr(), d, W.data_ptr(), d, h2.data_ptr(), d, 0
    dsc.I, dsc.J, dsc.R, dsc.epi, dsc.bias = M, d, d, _lib.EPI_BIAS_RES, bias.data_ptr()
    dsc.res, dsc.ldr, dsc.res_f32 = h2.data_ptr(), d, 0
    _lib.check(L.hig_gemm_bf16(C.byref(dsc), _lib.stream_ptr()))
    # fp64 definition (activations rounded to bf16 where the kernel rounds them)
    yd = y16.double().cpu()
    sc = ss[:, :d].double().cpu().repeat_interleave(T, 0)
    sh = ss[:, d:].double().cpu().repeat_interleave(T, 0)
    act = torch.nn.functional.silu(torch.nn.functional.layer_norm(yd, (d,), gamma.double().cpu(), beta.double().cpu(), 1e-5) * (1 + sc) + sh)
    ref = bf(act.float()).double() @ W.double().cpu().t() + bias.double().cpu() + h0.double().cpu()
    assert torch.isfinite(h.float()).all()
    assert rel(h.float(), ref) < 3e-3
    assert rel(h.float(), h2.float()) < 3e-3 and (h != h2).float().mean().item() < 0.05
    if with_stats:
        hp = h.float().double().cpu().view(M, 4, 128)
        assert rel(st[:, :, 0], hp.sum(-1)) < 1e-5 and rel(st[:, :, 1], ((hp - hp.mean(-1, keepdim=True)) ** 2).sum(-1)) < 1e-5


@pytest.mark.parametrize("M,T,F,d,shift", [(6272, 196, 150, 512, 0), (333, 37, 263, 256, 0), (70, 7, 12, 128, 1),
                                           (9600, 300, 150, 1024, 0), (129, 43, 151, 128, 0), (64, 8, 32, 128, 0)])
def test_joint_embed_bf16_kernel(M, T, F, d, shift):
    """hig_joint_embed_bf16 (joint_embed + sequence_embedding of the bf16-storage forward, transformer.py:418-419):
    x and the weight are rounded to bf16, products accumulate in fp32, bias and the positional row are added in fp32,
    the result is rounded to bf16 once -- compared with exactly that arithmetic in fp64 (correctly rounded almost
    everywhere) and with the fp32 reference at the bf16 level."""
    g = torch.Generator().manual_seed(M + F)
    x = torch.randn(M, F, generator=g) * 2
    W, b = torch.randn(d, F, generator=g) * 0.1, torch.randn(d, generator=g) * 0.1
    pos = torch.randn(T + 3, d, generator=g) * 0.5
    L = _lib.lib()
    out = torch.full((M, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    scratch = torch.empty(L.hig_joint_embed_bf16_scratch_bytes(F, d), dtype=torch.uint8, device=DEV)
    xg, Wg, bg, pg = x.to(DEV), W.to(DEV), b.to(DEV), pos.to(DEV)
    _lib.check(L.hig_joint_embed_bf16(_lib.ptr(xg), M, F, _lib.ptr(Wg), _lib.ptr(bg), _lib.ptr(pg), d, T, shift,
                                      _lib.ptr(out), d, d, _lib.ptr(scratch), _lib.stream_ptr()))
    tp = torch.arange(M) % T - shift
    padd = torch.where((tp >= 0)[:, None], pos[tp.clamp_min(0)].double(), torch.zeros(1, d, dtype=torch.float64))
    ref16 = bf(x).double() @ bf(W).double().T + b.double() + padd          # the kernel's arithmetic
    ref32 = x.double() @ W.double().T + b.double() + padd                  # the reference's
    o = out.float().cpu()
    assert torch.isfinite(o).all()
    assert (o != bf(ref16.float()).float()).float().mean().item() < 0.02
    assert rel(o, ref32) < 6e-3
    # the same with the weight padded / rounded by the caller (what the model keeps next to its bf16 shadow): same bits
    Fp = (F + 31) // 32 * 32
    wpad = torch.zeros(d, Fp, device=DEV, dtype=torch.bfloat16)
    wpad[:, :F] = Wg.to(torch.bfloat16)
    out2 = torch.full((M, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    _lib.check(L.hig_joint_embed_bf16_w(_lib.ptr(xg), M, F, _lib.ptr(wpad), _lib.ptr(bg), _lib.ptr(pg), d, T, shift,
                                        _lib.ptr(out2), d, d, _lib.stream_ptr()))
    assert torch.equal(out2, out)


def build(c, **kw):
    m = hig_amd.MotionTransformer(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                  num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"], **kw)
    m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    return m.to(DEV)


CASES16 = {
    "width": fill.CASES["width"],                                                            # config-2 model, hd = 64
    "hd128": dict(B=3, T=75, F=150, d=256, H=2, L=3, ff=512, N=77, Lt=64, num_frames=80, lengths=(75, 40, 1), t=(0, 999, 313)),
    "small": dict(B=2, T=33, F=12, d=128, H=2, L=2, ff=96, N=77, Lt=32, num_frames=40, lengths=(33, 5), t=(7, 650)),
    "wide8": dict(B=2, T=70, F=150, d=1024, H=8, L=2, ff=1024, N=77, Lt=256, num_frames=80, lengths=(70, 33), t=(5, 900)),
    # BASELINE config 5 as specified (T = 300, d = 1024, head dim 128, bf16 storage), two layers deep; 8 x 300 = 2400 rows,
    # so every large GEMM runs on the weight-stationary kernel (K = 1024: its K-split variant)
    "config5": dict(B=8, T=300, F=150, d=1024, H=8, L=2, ff=1024, N=77, Lt=256, num_frames=300,
                    lengths=(300, 211, 300, 1, 150, 299, 64, 300), t=(5, 900, 0, 999, 313, 650, 77, 500)),
    # the config-2 model on enough rows (16 x 196 = 3136) for the weight-stationary kernel's K = 512 / 256 variants
    "width16": dict(fill.CASES["width"], B=16, lengths=(196, 77, 196, 1, 120, 196, 50, 196) * 2,
                    t=(0, 999, 500, 250, 7, 650, 313, 900) * 2),
}


@pytest.mark.parametrize("case", sorted(CASES16))
def test_bf16_storage_forward_against_fp32_oracle(case):
    """Whole denoiser with bf16 activations and weights vs the fp32 CPU oracle on the same inputs: the error is the
    accumulated bf16 rounding of ~25 residual-stream updates -- reported, bounded at the bf16 level, and clearly
    above fp32 noise (the bf16 path really ran).  The fp32-storage bf16-PRODUCT mode is shown beside it."""
    c = CASES16[case]
    m = build(c, storage="bf16").eval()
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    gi = {k: v.to(DEV) for k, v in inp.items()}
    with torch.no_grad():
        out = m(gi["x"], gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"])
        m.storage, m.precision = "f32", "bf16"
        out_prod = m(gi["x"], gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"])
        p = fill.core_params(c["F"], c["d"], c["ff"], c["L"], c["Lt"], c["num_frames"])
        ref = R.denoiser_forward(p, inp["x"], inp["t"], inp["length"], inp["xf_proj"], inp["xf_out"], c["H"], c["L"])
    e, e_prod = rel(out, ref), rel(out_prod, ref)
    print("bf16 storage %s: rel-L2 vs fp32 oracle %.3e (bf16 products with fp32 storage: %.3e)" % (case, e, e_prod))
    assert out.dtype == torch.float32 and torch.isfinite(out).all()
    assert 1e-4 < e < 3e-2, e
    mx = ((out.cpu() - ref).abs().max() / ref.abs().max()).item()
    assert mx < 6e-2, mx


@pytest.mark.parametrize("B,Tq,Tk,H,hd,lens", [(2, 196, 196, 8, 64, (196, 77)), (2, 130, 77, 4, 64, None),
                                                (1, 300, 300, 2, 128, (211,)), (3, 70, 77, 8, 128, None)])
def test_full_attention_bf16_io_equals_the_fp32_kernel_on_the_same_values(B, Tq, Tk, H, hd, lens):
    """hig_fullattn_fwd_bf16 (no_eff attention of the bf16-storage forward) == hig_fullattn_fwd on the bf16-rounded inputs,
    output rounded to bf16 once: the bf16 kernel is the fp32 matrix-core kernel with bf16 loads / stores."""
    d = H * hd
    g = torch.Generator().manual_seed(B + Tq + hd)
    q16 = bf(torch.randn(B * Tq, d, generator=g) * 1.5).to(DEV)
    kv16 = bf(torch.randn(B * Tk, 2 * d, generator=g) * 1.5).to(DEV)
    lg = None if lens is None else torch.tensor(lens).to(DEV)
    L, s = _lib.lib(), _lib.stream_ptr()
    y16 = torch.full((B * Tq, d), float("nan"), device=DEV, dtype=torch.bfloat16)
    _lib.check(L.hig_fullattn_fwd_bf16(_lib.ptr(q16), d, _lib.ptr(kv16), kv16.data_ptr() + 2 * d, 2 * d, B, Tq, Tk, H, hd,
                                       _lib.ptr(lg), _lib.ptr(y16), d, s))
    q32, kv32 = q16.float(), kv16.float()
    y32 = torch.empty(B * Tq, d, device=DEV)
    lse = torch.empty(B * H * Tq, device=DEV)
    _lib.check(L.hig_fullattn_fwd(_lib.ptr(q32), d, _lib.ptr(kv32), kv32.data_ptr() + 4 * d, 2 * d, B, Tq, Tk, H, hd,
                                  _lib.ptr(lg), _lib.ptr(y32), d, _lib.ptr(lse), s))
    torch.cuda.synchronize()
    assert torch.equal(y16, bf(y32))


@pytest.mark.parametrize("case", ["width", "hd128", "config5"])
def test_bf16_storage_no_eff_forward_against_fp32_oracle(case):
    """storage='bf16' with no_eff=True (full softmax attention on the matrix cores, bf16 Q / K / V / Y): valid rows of a
    ragged batch against the fp32 CPU oracle (padded query rows carry the reference's -1e5-quantised logits, App. B-3)."""
    c = CASES16[case]
    m = build(c, storage="bf16", no_eff=True).eval()
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    gi = {k: v.to(DEV) for k, v in inp.items()}
    with torch.no_grad():
        out = m(gi["x"], gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"])
        p = fill.core_params(c["F"], c["d"], c["ff"], c["L"], c["Lt"], c["num_frames"])
        ref = R.denoiser_forward(p, inp["x"], inp["t"], inp["length"], inp["xf_proj"], inp["xf_out"], c["H"], c["L"], no_eff=True)
    assert torch.isfinite(out).all()
    errs = []
    for b, n in enumerate(c["lengths"]):
        n = min(n, c["T"])
        if n:
            errs.append(rel(out[b, :n], ref[b, :n]))
    print("bf16 storage, no_eff, %s: rel-L2 of the valid rows vs fp32 oracle %s" % (case, ["%.2e" % e for e in errs]))
    assert all(1e-4 < e < 3e-2 for e in errs), errs


def test_bf16_storage_sees_parameter_updates_and_refuses_unsupported_head_dims():
    c = CASES16["small"]
    m = build(c, storage="bf16").eval()
    gi = {k: v.to(DEV) for k, v in fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"]).items()}

    def fwd():
        with torch.no_grad():
            return m(gi["x"], gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"])

    a = fwd()
    assert torch.equal(a, fwd())
    with torch.no_grad():
        m.temporal_decoder_blocks[0].ffn.linear1.weight.mul_(1.25)       # the bf16 shadow must be rebuilt
    b = fwd()
    assert not torch.equal(a, b)
    m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    assert torch.equal(a, fwd())
    bad = build(fill.CASES["config1"], storage="bf16").eval()             # head dim 16: not built for bf16 storage
    c1 = fill.CASES["config1"]
    g1 = {k: v.to(DEV) for k, v in fill.inputs(c1["B"], c1["T"], c1["F"], c1["d"], c1["N"], c1["Lt"], c1["lengths"], c1["t"]).items()}
    with torch.no_grad(), pytest.raises(RuntimeError, match="head dim"):
        bad(g1["x"], g1["t"], length=g1["length"], xf_proj=g1["xf_proj"], xf_out=g1["xf_out"])


@pytest.mark.parametrize("case", ["width16", "config5", "small"])
def test_bf16_per_call_text_side_on_the_side_stream_equals_the_cached_form(case):
    """hig_denoiser_fwd_bf16_x with xf_out (the reference's per-call forward: text side and, for the d = 1024 models, the
    embedding chain on a library-owned stream next to the frame-row launches) against the text context built first on the
    caller's stream (cache_text_context=True), on every one of a run of back-to-back calls with changing inputs (a missing join
    would show as a stale or half-written context: the inputs of consecutive calls differ by far more than the tolerance).
    Linear attention: the per-call form is the BATCHED text side (one key/value GEMM over the stacked, text_norm-folded bf16
    weights of all layers, one context build over L H heads; round 6) -- another rounding sequence of the same arithmetic, so
    the two forms agree at the bf16 level (rel-L2 <= 2e-2: ~8e-3 measured at the config-2 width, where each form is ~1.3e-2
    from the fp32 oracle), the per-call form is no further from the fp32 CPU oracle than the cached one (+ 10 %), and each is
    bitwise repeatable."""
    c = CASES16[case]
    m = build(c, storage="bf16").eval()
    base = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    g = torch.Generator().manual_seed(11)
    outs = {}
    for cached in (True, False):
        m.cache_text_context = cached
        res = []
        for k in range(6):
            gi = {key: v.to(DEV) for key, v in base.items()}
            gk = torch.Generator().manual_seed(100 + k)
            gi["xf_out"] = (base["xf_out"] + 0.5 * torch.randn(base["xf_out"].shape, generator=gk)).to(DEV)
            gi["xf_proj"] = (base["xf_proj"] + 0.5 * torch.randn(base["xf_proj"].shape, generator=gk)).to(DEV)
            gi["x"] = (base["x"] + 0.1 * k).to(DEV)
            with torch.no_grad():
                res.append(m(gi["x"], gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"]))
        torch.cuda.synchronize()
        outs[cached] = res
    errs = []
    for a, b in zip(outs[True], outs[False]):
        assert torch.isfinite(b).all()
        errs.append(rel(b, a))
    print("bf16 per-call (batched text side) vs cached form, rel-L2 per call:", ["%.2e" % e for e in errs])
    assert max(errs) < 2e-2, errs
    if case != "config5":                                        # (the oracle at 8 x 300 rows x d = 1024 is minutes of host time)
        n = min(c["B"], 2)
        gk = torch.Generator().manual_seed(100)
        xo = base["xf_out"] + 0.5 * torch.randn(base["xf_out"].shape, generator=gk)
        xp = base["xf_proj"] + 0.5 * torch.randn(base["xf_proj"].shape, generator=gk)
        with torch.no_grad():
            p = fill.core_params(c["F"], c["d"], c["ff"], c["L"], c["Lt"], c["num_frames"])
            ref = R.denoiser_forward(p, base["x"][:n], base["t"][:n], base["length"][:n], xp[:n], xo[:n], c["H"], c["L"])
        e_call, e_cached = rel(outs[False][0][:n], ref), rel(outs[True][0][:n], ref)
        print("vs the fp32 oracle: per-call (batched) %.3e, cached (per layer) %.3e" % (e_call, e_cached))
        assert e_call < 3e-2 and e_call < 1.1 * e_cached + 1e-3, (e_call, e_cached)
    assert rel(outs[False][0], outs[False][1]) > 5e-2          # consecutive calls really differ
    m.cache_text_context = False                                # the last call again: same bits
    with torch.no_grad():
        again = m(gi["x"], gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"])
    assert torch.equal(again, outs[False][-1])
    del g


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_per_call_forward_under_stream_capture_equals_eager(storage):
    """The per-call forward (text side inside the call) forks its B-row work onto library-owned streams when launched eagerly and
    must run in order on the capturing stream under hipGraph capture: captured and replayed == eager, bit for bit."""
    c = CASES16["width16"]
    m = build(c, storage=storage).eval()
    m.cache_text_context = False
    gi = {k: v.to(DEV) for k, v in fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"]).items()}

    def fwd():
        with torch.no_grad():
            return m(gi["x"], gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"])

    ref = fwd().clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fwd()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fwd()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.equal(out, ref)


def test_config3_bf16_storage_captured_1000_step_loop():
    """BASELINE config 3 as specified: 1000-step p_sample_loop, B=32, T=196, bf16 storage, hipGraph-captured; against the
    eager loop with the noise zeroed on both sides (same kernels in the same order), finite over the whole chain."""
    c = dict(fill.CASES["width"], B=32)
    m = build(c, storage="bf16").eval()
    with torch.no_grad():
        m.out.weight.mul_(0.05)
        m.out.bias.mul_(0.05)
    g = torch.Generator().manual_seed(11)
    kw = {"xf_proj": torch.randn(32, 4 * c["d"], generator=g).to(DEV),
          "xf_out": torch.randn(32, c["N"], c["Lt"], generator=g).to(DEV),
          "length": torch.tensor([196] * 20 + list(range(100, 196, 8)), device=DEV)}
    x0 = torch.randn(32, 196, c["F"], generator=g).to(DEV)
    outs = []
    for use_graph in (False, True):
        gd = hig_amd.GaussianDiffusion(betas=gdm.get_named_beta_schedule("linear", 1000),
                                       model_mean_type=gdm.ModelMeanType.EPSILON,
                                       model_var_type=gdm.ModelVarType.FIXED_SMALL, loss_type=gdm.LossType.MSE)
        gd.use_hip_graph, gd._debug_zero_noise = use_graph, True
        old = gdm.th
        if not use_graph:
            proxy = types.SimpleNamespace(**{k: getattr(torch, k) for k in dir(torch) if not k.startswith("__")})
            proxy.randn_like = lambda x, **_: torch.zeros_like(x)
            gdm.th = proxy
        try:
            outs.append(gd.p_sample_loop(m, x0.shape, noise=x0.clone(), clip_denoised=False, model_kwargs=kw))
        finally:
            gdm.th = old
    assert torch.isfinite(outs[0]).all() and torch.isfinite(outs[1]).all()
    assert rel(outs[1], outs[0]) < 1e-5


def test_bf16_storage_unfused_regime_against_fp32_oracle():
    """The bf16-storage forward as `generate` runs it (ddpm_trainer.py:152: hundreds of captions per call): B = 120, T = 196
    is 840 workgroups of 32 rows -- beyond the 3 per CU the fused stylization blocks serve -- so every stylization block
    runs as apply + weight-stationary GEMM with the LayerNorm fold, at M = 23 520 rows.  Whole model (config-2 width, two
    layers) against the fp32 CPU oracle on the same inputs."""
    c = dict(fill.CASES["width"], B=120, L=2, lengths=tuple([196, 77, 196, 1, 120, 196, 50, 150] * 15),
             t=tuple([0, 999, 500, 250, 7, 650, 313, 900] * 15))
    m = build(c, storage="bf16").eval()
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    gi = {k: v.to(DEV) for k, v in inp.items()}
    with torch.no_grad():
        out = m(gi["x"], gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"])
        p = fill.core_params(c["F"], c["d"], c["ff"], c["L"], c["Lt"], c["num_frames"])
        ref = R.denoiser_forward(p, inp["x"], inp["t"], inp["length"], inp["xf_proj"], inp["xf_out"], c["H"], c["L"])
    e = rel(out, ref)
    per = [rel(out[b], ref[b]) for b in range(0, c["B"], 17)]
    print("bf16 storage, un-fused regime (B=120, T=196, L=2): rel-L2 vs fp32 oracle %.3e (per sample %s)" % (e, ["%.1e" % v for v in per]))
    assert torch.isfinite(out).all()
    assert 1e-4 < e < 3e-2, e
    assert max(per) < 5e-2, per


def test_generate_batch_size_1024_bf16_storage():
    """`DDPMTrainer.generate(..., batch_size=1024)` (ddpm_trainer.py:152) is the largest batch the reference asks of the
    denoiser: B = 1024, T = 196 -> M = 200 704 rows through the 32-bit buffer descriptors / grids of the weight-stationary
    GEMM, the bf16-matrix-core attention kernels and the >= 32 768-row LayerNorm variant.  One forward, slice-checked against
    the fp32 CPU oracle (samples are independent), and a 50-step captured sampling loop compared with the same loop at B = 4
    on the same leading samples (noise zeroed: the loop is then a deterministic function of x_T per sample)."""
    c = dict(fill.CASES["width"], B=1024, lengths=tuple([196, 77, 196, 1, 120, 196, 50, 150] * 128),
             t=tuple([0, 999, 500, 250, 7, 650, 313, 900] * 128))
    m = build(c, storage="bf16").eval()
    with torch.no_grad():
        m.out.weight.mul_(0.05)
        m.out.bias.mul_(0.05)
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    gi = {k: v.to(DEV) for k, v in inp.items()}
    with torch.no_grad():
        out = m(gi["x"], gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"])
    assert out.shape == (1024, 196, c["F"]) and torch.isfinite(out).all()
    p = {k: v.detach().cpu() for k, v in m.state_dict().items() if not k.startswith("clip.")}
    for lo in (0, 1020):      # first and last samples of the batch (row offsets 0 and ~200 000)
        sl = slice(lo, lo + 4)
        with torch.no_grad():
            ref = R.denoiser_forward(p, inp["x"][sl], inp["t"][sl], inp["length"][sl], inp["xf_proj"][sl], inp["xf_out"][sl], c["H"], c["L"])
        e = rel(out[sl], ref)
        print("B=1024 forward, samples %d..%d: rel-L2 vs fp32 oracle %.3e" % (lo, lo + 3, e))
        assert 1e-4 < e < 3e-2, e
    # fifty captured sampling steps at B = 1024 against the same fifty steps at B = 4
    kw = {"xf_proj": gi["xf_proj"], "xf_out": gi["xf_out"], "length": gi["length"]}
    x0 = gi["x"]
    outs = []
    for nb in (1024, 4):
        gd = hig_amd.GaussianDiffusion(betas=gdm.get_named_beta_schedule("linear", 50), model_mean_type=gdm.ModelMeanType.EPSILON,
                                       model_var_type=gdm.ModelVarType.FIXED_SMALL, loss_type=gdm.LossType.MSE)
        gd.use_hip_graph, gd._debug_zero_noise = True, True
        kwn = {k: v[:nb].contiguous() for k, v in kw.items()}
        outs.append(gd.p_sample_loop(m, (nb,) + tuple(x0.shape[1:]), noise=x0[:nb].clone(), clip_denoised=False, model_kwargs=kwn))
    assert torch.isfinite(outs[0]).all()
    e = rel(outs[0][:4], outs[1])
    print("50 captured sampling steps, B=1024 vs B=4 on the same samples: rel-L2 %.3e" % e)
    assert e < 3e-2, e


@pytest.mark.parametrize("ratio", [1, 10, 100, 1000])
def test_layernorm_fold_with_a_large_common_offset(ratio):
    """LayerNorm fold (hig_gemm16_desc.row_stats_*) on residual rows whose |mean| / std is `ratio`: the consumer must not lose
    the variance to cancellation.  The producer's panel statistics are (sum, sum of squared deviations from the panel mean);
    the consumer merges the four panels (Chan et al.) instead of forming E[x^2] - mean^2.  Reference: fp64 LayerNorm + Linear
    on the SAME bf16 rows the producer wrote (transformer.py:108-110)."""
    d, I, J = 512, 4096, 512
    g = torch.Generator().manual_seed(ratio)
    L = _lib.lib()
    a16, Wo = bf(torch.randn(I, d, generator=g) * 0.01), bf(torch.randn(d, d, generator=g) / d ** 0.5)
    bo = 0.01 * torch.randn(d, generator=g)
    hold = bf(torch.randn(I, d, generator=g) + float(ratio))
    ad, Wod, bod = a16.to(DEV), Wo.to(DEV), bo.to(DEV)
    h = hold.to(DEV).clone()
    stats = torch.full((I, 4, 2), float("nan"), device=DEV)
    dsc = _lib.Gemm16Desc()
    dsc.X, dsc.ldx, dsc.Y, dsc.ldy, dsc.C, dsc.ldc, dsc.c_f32 = ad.data_ptr(), d, Wod.data_ptr(), d, h.data_ptr(), d, 0
    dsc.I, dsc.J, dsc.R, dsc.epi, dsc.bias = I, d, d, _lib.EPI_BIAS_RES, bod.data_ptr()
    dsc.res, dsc.ldr, dsc.res_f32 = h.data_ptr(), d, 0
    dsc.row_stats_out = stats.data_ptr()
    _lib.check(L.hig_gemm_bf16(C.byref(dsc), _lib.stream_ptr()))
    gamma, beta = 1 + 0.2 * torch.randn(d, generator=g), 0.3 * torch.randn(d, generator=g)
    W, b = torch.randn(J, d, generator=g) / d ** 0.5, torch.randn(J, generator=g)
    Wp = bf(W * gamma[None, :])
    cs, bp = Wp.float().sum(1), b + W @ beta
    out = torch.full((I, J), float("nan"), device=DEV, dtype=torch.bfloat16)
    Wpd, csd, bpd = Wp.to(DEV), cs.to(DEV), bp.to(DEV)
    c2 = _lib.Gemm16Desc()
    c2.X, c2.ldx, c2.Y, c2.ldy, c2.C, c2.ldc, c2.c_f32 = h.data_ptr(), d, Wpd.data_ptr(), d, out.data_ptr(), J, 0
    c2.I, c2.J, c2.R, c2.epi, c2.bias = I, J, d, _lib.EPI_BIAS, bpd.data_ptr()
    c2.row_stats_in, c2.ln_colsum = stats.data_ptr(), csd.data_ptr()
    _lib.check(L.hig_gemm_bf16(C.byref(c2), _lib.stream_ptr()))
    hd_ = h.float().double().cpu()
    # what the folded form computes, in fp64: rstd (x W'^T) - rstd mean colsum + bias'  (W' = bf16(gamma W))
    mean, var = hd_.mean(1, keepdim=True), hd_.var(1, unbiased=False, keepdim=True)
    rstd = (var + 1e-5).rsqrt()
    ref_fold = rstd * (hd_ @ Wp.double().t()) - rstd * mean * cs.double()[None, :] + bp.double()[None, :]
    ref = torch.nn.functional.layer_norm(hd_, (d,), gamma.double(), beta.double(), 1e-5) @ W.double().t() + b.double()
    e_fold, e = rel(out.float(), ref_fold), rel(out.float(), ref)
    print("LayerNorm fold at |mean|/std = %d: rel-L2 %.2e vs the folded form in fp64, %.2e vs LayerNorm + Linear" % (ratio, e_fold, e))
    assert torch.isfinite(out.float()).all()
    # the statistics themselves: the variance the consumer derives must be the rows' variance
    assert e_fold < 4e-3, (ratio, e_fold)
