"""The contract of every GEMM path: which kernel served a call, that it wrote every output and nothing around it, and an
element-wise bound against fp64.

Every call goes through `run`, which
  - asserts that exactly the expected HIG_GEMM_PATH_* counters moved (hig_gemm_path_launches; two launches for the
    two-pass K > 1024 form of the fp32 weight-stationary kernel), and that the plan entry (hig_gemm_bf16_plan /
    hig_gemm_plan), asked before the call, named exactly those;
  - fills C (and `aux`) with a NaN pattern first and checks that every output was written;
  - puts C inside guard rows above and below, and guard columns where ldc > J, and checks they kept their bits.
`check` then holds every element to a bound computed from the operands in fp64:
    |C - ref| <= gamma ||X_i||_2 ||W_j||_2 + 2^-23 (|bias_j| + |res_ij|)      gamma = 2 K 2^-24
(Cauchy-Schwarz bounds sum_k |x_ik w_jk| by the row norms, so this is rigorous for fp32 accumulation at O(IJ) cost, and
still ~100x below the error of one missing 32-element k-step), plus 2^-8 |ref| for bf16 outputs, plus the activation
bounds stated next to the HIG_EPI_* defines of include/hig.h for the activation epilogues.  The assertion message reports
the largest ratio of error to bound.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from hig_amd import _lib  # noqa: E402
from gemm_dispatch_cases import (BIAS, BIAS_RES, DGELU, DISPATCH, GELU, HAS_BIAS, HAS_RES, NONE, PATHS, RES, RES_SILU, SILU,  # noqa: E402
                                 UNSERVED, dispatch_uses_aux, plan)

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = {torch.float32: (torch.int32, 0x7FC0BEEF), torch.bfloat16: (torch.int16, 0x7FD5)}   # NaN patterns

# the element-wise bounds of the activation epilogues (include/hig.h, next to HIG_EPI_BIAS_GELU / _DGELU / _BIAS_SILU)
GELU32_PER_Z = 4e-7       # fp32 GELU: |out - gelu(z)| <= 4e-7 |z| + 2^-23 |gelu(z)|
DGELU_ABS = 4e-7          # gelu'(z) of the epilogues: |d - gelu'(z)| <= 4e-7 + 2^-23 |gelu'(z)| (fp32), + 1 bf16 ulp (bf16)
GELU16_TAIL = 4.1e-11     # bf16 GELU, |z| > 6.5: + 4.1e-11 |z| (the fit is clamped at 6.5; Q(6.5) = 4.016e-11)
FLOOR16 = 2.0 ** -126     # bf16 GELU / SiLU: + the smallest normal (outputs below it may be flushed)
LIP = 1.13                # max |gelu'| = 1.1289, max |silu'| = 1.0998: how a pre-activation error reaches the output


def lib():
    return _lib.lib()


def counts():
    return [lib().hig_gemm_path_launches(getattr(_lib, "GEMM_PATH_" + n)) for n in PATHS]


def counted(call, expect, planned=None):
    """call() -> rc; asserts rc == 0 and that exactly the path counters in `expect` ({name: launches}) moved.  planned:
    (entry, descriptor) of the call where a plan entry covers it -- the plan, asked BEFORE the call, must have named exactly
    the counters that moved."""
    foreseen = plan(*planned) if planned else None
    before = counts()
    _lib.check(call())
    torch.cuda.synchronize()
    moved = {n: a - b for n, a, b in zip(PATHS, counts(), before) if a != b}
    assert moved == expect, "expected launches %s, got %s" % (expect, moved)
    if planned:
        assert foreseen[0] == 0 and foreseen[1] == moved, "the plan named %s (rc %d), the call moved %s" % (foreseen[1], foreseen[0], moved)


def ulp16(r):
    """bf16 ulp of |r| (2^(e - 7) for |r| in [2^e, 2^(e + 1)); the normal range's smallest below 2^-126)."""
    e = torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


class Guarded:
    """An (I, J) output inside an (I + 2, ldc) buffer filled with a NaN pattern: row 0, row I + 1 and columns J .. ldc - 1
    are guard bands that must keep their bits."""

    def __init__(self, I, J, ldc, dtype):
        self.I, self.J, self.ldc, self.dtype = I, J, ldc, dtype
        itype, pat = SENTINEL[dtype]
        self.pat = pat
        self.buf = torch.full(((I + 2) * ldc,), pat, dtype=itype, device=DEV)
        self.out = self.buf.view(dtype)[ldc:ldc + I * ldc].view(I, ldc)[:, :J]

    def ptr(self):
        return self.out.data_ptr()

    def verify(self):
        b = self.buf.view(self.I + 2, self.ldc)
        keep = torch.ones_like(b, dtype=torch.bool)
        keep[1:self.I + 1, :self.J] = False
        assert (b[keep] == self.pat).all(), "a store landed in the guard band around C"
        assert torch.isfinite(self.out.float()).all(), "not every output was written"


def rnd(*shape, gen, scale=1.0):
    return torch.randn(*shape, generator=gen, device=DEV) * scale


def desc32(X, W, out, ldc, I, J, K, epi, bias, res, aux, x_rs=0, y_rs=0):
    d = _lib.GemmDesc()
    d.X, d.ldx, d.x_rs = X.data_ptr(), X.stride(0), x_rs
    d.Y, d.ldy, d.y_rs = W.data_ptr(), W.stride(0), y_rs
    d.C, d.ldc = out, ldc
    d.I, d.J, d.R, d.epi, d.prec = I, J, K, epi, _lib.PREC_F32
    d.xf = _lib.XF_NONE
    if bias is not None:
        d.bias = bias.data_ptr()
    if res is not None:
        d.res, d.ldr = res.data_ptr(), res.stride(0)
    if aux is not None:
        d.aux, d.ldaux = aux.data_ptr(), aux.stride(0)
    return d


def desc16(X, W, out, ldc, c_f32, I, J, K, epi, bias, res, aux):
    d = _lib.Gemm16Desc()
    d.X, d.ldx, d.Y, d.ldy = X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0)
    d.C, d.ldc, d.c_f32 = out, ldc, c_f32
    d.I, d.J, d.R, d.epi = I, J, K, epi
    if bias is not None:
        d.bias = bias.data_ptr()
    if res is not None:
        d.res, d.ldr, d.res_f32 = res.data_ptr(), res.stride(0), int(res.dtype == torch.float32)
    if aux is not None:
        d.aux, d.ldaux = aux.data_ptr(), aux.stride(0)
    return d


def run(entry, X, W, expect, epi=NONE, bias=None, res=None, c_f32=None, ldc=None, with_aux=False, inplace=False):
    """One call of `entry` ('f32': hig_gemm, 'ws': hig_gemm_ws, 'bf16': hig_gemm_bf16) on X (I, K), W (J, K); returns
    (C, aux) after the path, NaN-fill and guard checks.  inplace: C aliases res (bf16 residual, ldc = J)."""
    I, K = X.shape
    J = W.shape[0]
    f32_entry = entry in ("f32", "ws")
    c_f32 = True if f32_entry else bool(c_f32)
    dt = torch.float32 if c_f32 else torch.bfloat16
    ldc = J if ldc is None else ldc
    aux = None
    if with_aux:
        aux = torch.full((I, J), float("nan"), device=DEV, dtype=torch.float32 if f32_entry else torch.bfloat16)
    if inplace:
        g = None
        out = res.clone()
        optr, ldc_ = out.data_ptr(), J
        res_ = out
    else:
        g = Guarded(I, J, ldc, dt)
        optr, ldc_, res_ = g.ptr(), ldc, res
    if f32_entry:
        d = desc32(X, W, optr, ldc_, I, J, K, epi, bias, res_, aux)
        if entry == "ws":
            ws = torch.zeros(lib().hig_gemm_tail_ws_bytes(), dtype=torch.uint8, device=DEV)
            call = lambda: lib().hig_gemm_ws(C.byref(d), ws.data_ptr(), ws.numel(), _lib.stream_ptr())  # noqa: E731
        else:
            call = lambda: lib().hig_gemm(C.byref(d), _lib.stream_ptr())  # noqa: E731
    else:
        d = desc16(X, W, optr, ldc_, int(c_f32), I, J, K, epi, bias, res_, aux)
        call = lambda: lib().hig_gemm_bf16(C.byref(d), _lib.stream_ptr())  # noqa: E731
    counted(call, expect, (entry, d))
    if g is not None:
        g.verify()
        out = g.out
    if aux is not None:
        assert torch.isfinite(aux.float()).all(), "not every aux output was written"
    return out, aux


def linear_ref(X, W, epi, bias, res):
    """(pre-activation in fp64, its bound): acc + bias + res, gamma ||X_i|| ||W_j|| + 2^-23 (|bias| + |res|)."""
    Xd, Wd = X.double(), W.double()
    K = X.shape[1]
    pre = Xd @ Wd.t()
    bnd = (2 * K * 2.0 ** -24) * torch.outer(Xd.norm(dim=1), Wd.norm(dim=1))
    if epi in HAS_BIAS:
        pre = pre + bias.double()
        bnd = bnd + 2.0 ** -23 * bias.double().abs()
    if epi in (BIAS_RES, RES, RES_SILU):
        pre = pre + res.double()
        bnd = bnd + 2.0 ** -23 * res.double().abs()
    return pre, bnd


def gelu64(z):
    return 0.5 * z * torch.erfc(-z / 2 ** 0.5)


def dgelu64(z):
    return 0.5 * torch.erfc(-z / 2 ** 0.5) + z * torch.exp(-0.5 * z * z) / (2 * torch.pi) ** 0.5


def silu64(z):
    return z * torch.sigmoid(z)


def act_bound(epi, z, ref, bf16_out):
    """The bound of include/hig.h for the activation of `epi` at pre-activation z (fp64), result ref."""
    if epi == GELU:
        if bf16_out:
            return ulp16(ref) + FLOOR16 + (z.abs() > 6.5).double() * GELU16_TAIL * z.abs()
        return GELU32_PER_Z * z.abs() + 2.0 ** -23 * ref.abs()
    if epi in (SILU, RES_SILU):
        return ulp16(ref) + FLOOR16
    if epi == DGELU:
        return (ulp16(ref) if bf16_out else 2.0 ** -23 * ref.abs()) + DGELU_ABS
    raise ValueError(epi)


def check(out, ref, bnd, what=""):
    err = (out.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)   # (an exact zero bound admits only an exact result)
    worst = ratio.max().item()
    if not worst <= 1.0:
        i = int(ratio.argmax())
        r, c = divmod(i, ref.shape[1])
        bad = int((ratio > 1).sum())
        raise AssertionError("%s: %d elements beyond the bound, worst err / bound = %.3g at (%d, %d): got %r, fp64 %r, bound %.3g"
                             % (what, bad, worst, r, c, out[r, c].item(), ref[r, c].item(), bnd[r, c].item()))
    return worst


def gemm_bound(X, W, epi=NONE, bias=None, res=None, bf16_out=False, bf16_aux=False):
    """(ref, bound, pre-activation, its bound as `aux` is held) of one call: the linear bound, composed with the activation
    bounds.  The last two are None for HIG_EPI_DGELU, which has no pre-activation output."""
    if epi == DGELU:
        acc, bnd = linear_ref(X, W, NONE, None, None)
        z = res.double()
        d = dgelu64(z)
        ref = acc * d
        return ref, LIP * bnd + acc.abs() * act_bound(DGELU, z, d, False) + (ulp16(ref) if bf16_out else 2.0 ** -23 * ref.abs()), None, None
    pre, bnd = linear_ref(X, W, epi, bias, res)
    aux_bnd = bnd + (2.0 ** -8 * pre.abs() if bf16_aux else 0)        # the pre-activation output: the same linear bound, rounded like C
    if epi in (GELU, SILU, RES_SILU):
        ref = gelu64(pre) if epi == GELU else silu64(pre)
        return ref, LIP * bnd + act_bound(epi, pre, ref, bf16_out), pre, aux_bnd
    return pre, bnd + (2.0 ** -8 * pre.abs() if bf16_out else 0), pre, aux_bnd


def check_gemm(out, X, W, epi=NONE, bias=None, res=None, aux=None, what=""):
    """Element-wise bound of one call (gemm_bound)."""
    ref, bnd, pre, aux_bnd = gemm_bound(X, W, epi, bias, res, out.dtype == torch.bfloat16, aux is not None and aux.dtype == torch.bfloat16)
    if aux is not None:
        check(aux, pre, aux_bnd, what + " aux")
    return check(out, ref, bnd, what)


def operands(entry, I, J, K, epi, seed, res_f32=False):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    X, W = rnd(I, K, gen=gen), rnd(J, K, gen=gen, scale=K ** -0.5)
    bias = rnd(J, gen=gen) if epi in HAS_BIAS else None
    res = rnd(I, J, gen=gen) if epi in HAS_RES else None
    if entry == "bf16":
        X, W = X.bfloat16(), W.bfloat16()
        if res is not None and not res_f32:
            res = res.bfloat16()
    return X, W, bias, res


# the dispatch table (DISPATCH) and the unserved cases (UNSERVED): tests/gemm_dispatch_cases.py, shared with tests/test_cpu_gemm_plan.py
@pytest.mark.parametrize("entry,I,J,K,epi,c_f32,res_f32,ldc,expect", DISPATCH)
def test_dispatch_table(entry, I, J, K, epi, c_f32, res_f32, ldc, expect):
    X, W, bias, res = operands(entry, I, J, K, epi, seed=I + 3 * J + 7 * K + epi, res_f32=res_f32)
    if epi == DGELU and entry != "bf16":   # the fp32 entry takes z through `aux`
        g = Guarded(I, J, ldc or J, torch.float32)
        d = desc32(X, W, g.ptr(), ldc or J, I, J, K, epi, None, None, res)
        counted(lambda: lib().hig_gemm(C.byref(d), _lib.stream_ptr()), expect, ("f32", d))
        g.verify()
        check_gemm(g.out, X, W, DGELU, res=res, what=str(expect))
        return
    with_aux = dispatch_uses_aux(entry, epi, expect)
    out, ax = run(entry, X, W, expect, epi, bias, res, c_f32, ldc, with_aux=with_aux)
    check_gemm(out, X, W, epi, bias, res, ax, what=str(expect))


def test_every_path_constant_is_asserted_by_the_dispatch_tests():
    named = set()
    for case in DISPATCH:
        named |= set(case[-1])
    named |= {"WGRAD_WSP32", "SPLIT32", "SPLIT16", "WGRAD16"}   # test_split_forms_dispatch
    assert named == set(PATHS) and len(PATHS) == _lib.GEMM_NPATHS


@pytest.mark.parametrize("I,J,R,splits,expect", [(512, 512, 4096, 8, "WGRAD_WSP32"), (500, 512, 4096, 8, "SPLIT32")])
def test_split_forms_dispatch(I, J, R, splits, expect):
    """hig_gemm_split (weight gradients dW = dC^T act, both operands reduce-slow): wgrad_wsp32.hip, and the tiled kernel
    over slabs for what it declines; hig_gemm_bf16_split and hig_wgrad_bf16 are held to exactness below."""
    gen = torch.Generator(device=DEV).manual_seed(I + J + R)
    dC, act = rnd(R, I, gen=gen), rnd(R, J, gen=gen)
    out = torch.full((I, J), float("nan"), device=DEV)
    d = desc32(dC, act, out.data_ptr(), J, I, J, R, NONE, None, None, None, x_rs=1, y_rs=1)
    nsl = lib().hig_gemm_split_scratch_floats(C.byref(d), splits)
    slabs = torch.empty(nsl, device=DEV)
    counted(lambda: lib().hig_gemm_split(C.byref(d), splits, slabs.data_ptr(), nsl, _lib.stream_ptr()), {expect: 1})
    check_gemm(out, dC.t(), act.t(), what=expect)


def test_unserved_fold_and_aux_operands_raise():
    """LayerNorm-fold operands / a bf16 `aux` on a shape no kernel that implements them serves (UNSERVED): an error, no launch --
    and the plan says so beforehand."""
    before = counts()
    for entry, I, J, K, epi, operand in UNSERVED:
        X, W, bias, res = operands(entry, I, J, K, epi, seed=5)
        out = torch.empty(I, J, device=DEV, dtype=torch.bfloat16 if entry == "bf16" else torch.float32)
        extra = torch.empty(I, max(J, 8), device=DEV, dtype=torch.float32 if operand == "stats_out" else out.dtype)
        if entry == "bf16":
            d = desc16(X, W, out.data_ptr(), J, 0, I, J, K, epi, bias, res, extra if operand == "aux" else None)
        else:
            d = desc32(X, W, out.data_ptr(), J, I, J, K, epi, bias, res, None)
        if operand == "stats_out":
            d.row_stats_out = extra.data_ptr()
        assert plan(entry, d)[:2] == (-3, {}), (entry, I, J, K, epi, operand)
        call = lib().hig_gemm_bf16 if entry == "bf16" else lib().hig_gemm
        assert call(C.byref(d), _lib.stream_ptr()) == -3, (entry, I, J, K, epi, operand)
    torch.cuda.synchronize()
    assert counts() == before


# ---------------------------------------------------------------------------------------------------------------------
# exact on small integers: X, W in {-4 .. 4}, integer bias and bf16 residual -- fp32 accumulation of those products is exact,
# so a bf16 result is torch's round-to-nearest-even of the exact value, bit for bit, on every path and linear epilogue
# ---------------------------------------------------------------------------------------------------------------------
def int_operands(I, J, K, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    X = torch.randint(-4, 5, (I, K), generator=gen, device=DEV).bfloat16()
    W = torch.randint(-4, 5, (J, K), generator=gen, device=DEV).bfloat16()
    bias = torch.randint(-64, 65, (J,), generator=gen, device=DEV).float()
    res = torch.randint(-256, 257, (I, J), generator=gen, device=DEV).bfloat16()
    return X, W, bias, res


def exact_value(X, W, epi, bias, res):
    v = X.double() @ W.double().t()
    if epi in HAS_BIAS:
        v = v + bias.double()
    if epi in (BIAS_RES, RES):
        v = v + res.double()
    return v


def exact_linear_epilogues(I, J, K, path, c_f32=0):
    X, W, bias, res = int_operands(I, J, K, seed=I + J + K)
    for epi in (NONE, BIAS, RES, BIAS_RES):
        v = exact_value(X, W, epi, bias, res)
        want = v.float() if c_f32 else v.float().bfloat16()
        served = "TILED16" if path == "FEWROW16" and epi == RES else path   # (the few-row kernel has no EPI_RES)
        out, _ = run("bf16", X, W, {served: 1}, epi, bias, res, c_f32)
        assert torch.equal(out.view(torch.int16 if not c_f32 else torch.int32),
                           want.view(torch.int16 if not c_f32 else torch.int32)), (path, epi, (out.double() - v).abs().max().item())
        if epi in (RES, BIAS_RES) and not c_f32:   # the in-place residual update (plain stores instead of write-through)
            out2, _ = run("bf16", X, W, {served: 1}, epi, bias, res, 0, inplace=True)
            assert torch.equal(out2.view(torch.int16), want.view(torch.int16)), (path, epi, "in place")


@pytest.mark.parametrize("I,J,K,path,c_f32", [(2048, 256, 512, "WSP16", 0), (2048, 256, 256, "WS16", 0), (2048, 384, 1024, "WS16", 0),
                                              (48, 256, 512, "FEWROW16", 0), (48, 256, 512, "FEWROW16", 1),
                                              (1000, 256, 512, "TILED16", 0), (1000, 256, 512, "TILED16", 1)])
def test_bf16_paths_exact_on_small_integers(I, J, K, path, c_f32):
    exact_linear_epilogues(I, J, K, path, c_f32)


def test_ws16_k512_exact_on_small_integers():
    """gemm_ws16 at K = 512 is reached only with its variant forced (HIG_BF16_WS_NWJ, read once per process: a child)."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_gemm_contract as t\n"
            "t.exact_linear_epilogues(2048, 256, 512, 'WS16'); t.exact_linear_epilogues(3001, 384, 512, 'WS16'); print('ok')\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, HIG_BF16_WS_NWJ="4")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_split_and_wgrad_bf16_exact_on_small_integers():
    """hig_gemm_bf16_split (fp32 C over split-R slabs) and hig_wgrad_bf16 (dW = dC^T act, dbias = column sums of dC)."""
    Xt, Wt, _, _ = int_operands(256, 384, 4096, seed=11)          # X (256, 4096), W (384, 4096)
    out = torch.full((256, 384), float("nan"), device=DEV)
    d = desc16(Xt, Wt, out.data_ptr(), 384, 1, 256, 384, 4096, NONE, None, None, None)
    nsl = lib().hig_gemm_bf16_split_scratch_floats(C.byref(d), 0)
    slabs = torch.empty(nsl, device=DEV)
    counted(lambda: lib().hig_gemm_bf16_split(C.byref(d), 0, slabs.data_ptr(), nsl, _lib.stream_ptr()), {"SPLIT16": 1})
    assert torch.equal(out, (Xt.double() @ Wt.double().t()).float())
    rows, J, K = 4096, 256, 384
    gen = torch.Generator(device=DEV).manual_seed(12)
    dC = torch.randint(-4, 5, (rows, J), generator=gen, device=DEV).bfloat16()
    act = torch.randint(-4, 5, (rows, K), generator=gen, device=DEV).bfloat16()
    dW = torch.full((J, K), float("nan"), device=DEV)
    db = torch.full((J,), float("nan"), device=DEV)
    nsl = lib().hig_wgrad_bf16_scratch_floats(J, K, 0)
    slabs = torch.empty(nsl, device=DEV)
    counted(lambda: lib().hig_wgrad_bf16(dC.data_ptr(), J, act.data_ptr(), K, rows, J, K, dW.data_ptr(), db.data_ptr(), 0,
                                         slabs.data_ptr(), nsl, _lib.stream_ptr()), {"WGRAD16": 1})
    assert torch.equal(dW, (dC.double().t() @ act.double()).float())
    assert torch.equal(db, dC.double().sum(0).float())


# ---------------------------------------------------------------------------------------------------------------------
# row-group / segment edges of the weight-stationary kernels: row groups left empty, with one tile, uneven; one-panel last
# segments of gemm_wsp32 with fewer 16-row tiles than workgroups (nt == 0).  Element-wise bound, bitwise repeatability, and
# batch-split invariance where both halves stay on the kernel (>= 2048 rows each): a weight-stationary kernel's per-row sum
# order does not depend on its tile schedule.
# ---------------------------------------------------------------------------------------------------------------------
def edges(entry, I, J, K, epi, path):
    X, W, bias, res = operands(entry, I, J, K, epi, seed=I * 5 + J + K)
    out, _ = run(entry, X, W, {path: 1}, epi, bias, res)
    check_gemm(out, X, W, epi, bias, res, what="%s %s" % (path, (I, J, K)))
    again, _ = run(entry, X, W, {path: 1}, epi, bias, res)
    assert torch.equal(again, out), "not bitwise repeatable"
    if I >= 4096:
        h = I // 2
        top, _ = run(entry, X[:h], W, {path: 1}, epi, bias, None if res is None else res[:h])
        bot, _ = run(entry, X[h:], W, {path: 1}, epi, bias, None if res is None else res[h:])
        assert torch.equal(top, out[:h]) and torch.equal(bot, out[h:]), "rows [:%d] / [%d:] alone differ from the whole launch" % (h, h)


@pytest.mark.parametrize("J", [128, 384, 1536, 3072])
@pytest.mark.parametrize("I", [2048, 2049, 2080, 4098, 8191, 8224])
def test_wsp16_row_group_edges(I, J):
    edges("bf16", I, J, 512, BIAS_RES, "WSP16")


@pytest.mark.parametrize("I,J,K,epi", [(3000, 576, 512, BIAS_RES), (2500, 96, 1024, BIAS_RES), (2050, 384, 256, BIAS),
                                       (6000, 576, 512, BIAS_RES), (5000, 96, 1024, RES), (4100, 384, 256, BIAS)])
def test_wsp32_one_panel_segment_edges(I, J, K, epi):
    edges("f32", I, J, K, epi, "WSP32")


# ---------------------------------------------------------------------------------------------------------------------
# activation epilogues over their whole input range.  X[i, k] = [k == i mod K] makes C[i, j] = W[j, i mod K] exactly on every
# path, so W carries chosen pre-activations; DGELU: W all ones (acc = 1), z through `res` (bf16) / `aux` (fp32).
# ---------------------------------------------------------------------------------------------------------------------
def bf16_normals(limit=64.0):
    """Every normal bf16 value with |z| <= limit, and +-0 (subnormals are left out: the matrix cores may flush them)."""
    v = (torch.arange(1 << 16, dtype=torch.int32) << 16).view(torch.float32)
    keep = torch.isfinite(v) & (v.abs() <= limit) & ((v.abs() >= 2.0 ** -126) | (v == 0))
    return v[keep]


def f32_grid(n=20001):
    g = torch.logspace(-6, 3, n, dtype=torch.float64).float()
    return torch.cat([-g.flip(0), torch.zeros(1), g])


def one_hot(I, K, dtype):
    X = torch.zeros(I, K, device=DEV, dtype=dtype)
    X[torch.arange(I), torch.arange(I) % K] = 1
    return X


def carrying(values, I, J, K, dtype):
    """W (J, K) whose first min(I, K) columns hold `values` (zeros after); Z (I, J) = W[j, i mod K], what the one-hot X yields."""
    m = min(I, K)
    assert J * m >= values.numel()
    W = torch.zeros(J, K, dtype=dtype)
    flat = torch.zeros(J * m, dtype=dtype)
    flat[:values.numel()] = values.to(dtype)
    W[:, :m] = flat.view(J, m)
    Z = W[:, torch.arange(I) % K].t().contiguous()
    return W.to(DEV), Z.double().to(DEV)


BF16_ACT = [("WSP16", 2048, 128, 512), ("WS16", 2048, 256, 256), ("FEWROW16", 64, 544, 256), ("TILED16", 1000, 128, 512)]


@pytest.mark.parametrize("path,I,J,K", BF16_ACT)
def test_bf16_activations_over_every_normal_input(path, I, J, K):
    vals = bf16_normals()
    X = one_hot(I, K, torch.bfloat16)
    W, Z = carrying(vals, I, J, K, torch.bfloat16)
    zero_b = torch.zeros(J, device=DEV)
    for epi in (GELU, SILU, RES_SILU):
        res = torch.zeros(I, J, device=DEV, dtype=torch.bfloat16) if epi == RES_SILU else None
        aux = epi == GELU and path == "WSP16"
        out, ax = run("bf16", X, W, {path: 1}, epi, zero_b, res, with_aux=aux)
        ref = gelu64(Z) if epi == GELU else silu64(Z)
        check(out, ref, act_bound(epi, Z, ref, True), "%s epi %d" % (path, epi))
        if aux:   # (z + 0: an fp32 sum that starts from +0 turns a -0 into +0)
            want = (Z + 0.0).float().bfloat16()
            bad = (ax.view(torch.int16) != want.view(torch.int16)).nonzero()
            assert bad.numel() == 0, "aux != z at %d elements, first %s: %r against %r" % (
                bad.shape[0], bad[0].tolist(), ax[tuple(bad[0])].item(), want[tuple(bad[0])].item())
    if path == "FEWROW16":
        return   # (the few-row kernel has no DGELU epilogue: such calls go to the tiled kernel, covered by TILED16)
    ones = torch.ones(J, K, device=DEV, dtype=torch.bfloat16)
    assert I * J >= vals.numel()
    z = torch.zeros(I * J)
    z[:vals.numel()] = vals
    z = z.view(I, J).bfloat16().to(DEV)
    out, _ = run("bf16", X, ones, {path: 1}, DGELU, None, z)
    ref = dgelu64(z.double())
    check(out, ref, act_bound(DGELU, z.double(), ref, True), "%s dgelu" % path)


@pytest.mark.parametrize("path,I,J,K", [("WSP32", 2048, 128, 512), ("TILED32", 1000, 128, 512)])
def test_f32_gelu_and_dgelu_over_a_dense_grid(path, I, J, K):
    vals = f32_grid()
    X = one_hot(I, K, torch.float32)
    W, Z = carrying(vals, I, J, K, torch.float32)
    out, ax = run("f32", X, W, {path: 1}, GELU, torch.zeros(J, device=DEV), with_aux=True)
    ref = gelu64(Z)
    check(out, ref, act_bound(GELU, Z, ref, False), "%s gelu" % path)
    assert torch.equal(ax, Z.float()), "aux != z"
    z = torch.zeros(I * J)
    z[:vals.numel()] = vals
    z = z.view(I, J).to(DEV)
    g = Guarded(I, J, J, torch.float32)
    ones = torch.ones(J, K, device=DEV)
    d = desc32(X, ones, g.ptr(), J, I, J, K, DGELU, None, None, z)
    counted(lambda: lib().hig_gemm(C.byref(d), _lib.stream_ptr()), {path: 1}, ("f32", d))
    g.verify()
    ref = dgelu64(z.double())
    check(g.out, ref, act_bound(DGELU, z.double(), ref, False), "%s dgelu" % path)
