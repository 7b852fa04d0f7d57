"""The contract of every attention kernel (csrc/linattn.hip, csrc/fullattn.hip): which kernel served a call and in which
split regime, that it wrote every output element and nothing around it, and an element-wise bound against fp64.

Every library call goes through `counted`, which first asks the plan (hig_attn_plan with the device's CU count; the expected
paths and regimes are the tables of tests/attn_dispatch_cases.py, which tests/test_cpu_attn_plan.py holds the plan to without a
GPU), then asserts that exactly the planned and expected HIG_ATTN_PATH_* counter moved (by one), that hig_attn_last_split() is
the planned split, and holds it to the regime the case is named for:
    'one'      gridDim.y == 1: one workgroup walks every chunk of a (sample, head);
    'all'      gridDim.y == number of chunks / blocks: one workgroup each;
    'partial'  strictly between: workgroups walk several chunks each AND their partial results are merged.
Shapes are built from the device's CU count (B * H is stated as a multiple of it), so a case keeps its regime on a part that
is not 256 CUs; where a shape does not reach its regime on another part the case skips and says why (on 256 CUs it fails).  Outputs live in `Guarded`
buffers: filled with a NaN pattern, with a guard row above and below and guard columns (leading dimension = row + 8).

THE BOUND.  One rule: a result differs from its fp64 value by at most  gamma 2^-24 M (+ 2^-120, see FLOOR),  M = the same
expression with every term replaced by its absolute value, gamma = a count of roundings.  Counting conventions (u = 2^-24):
  * a sum of n terms in ANY order (sequential, tree, matrix core, partial sums merged later) is off by at most n u times the sum
    of the absolute terms -- the linear worst case, the one the GEMM contract uses (gamma = 2 K there).  It is what makes one
    gamma valid for every split regime of a kernel, which is the point of this file; the measured multiples grow like the
    square root of the depth and are printed next to gamma.  A gamma here is therefore dominated by the reduction length
    (T = 300 rows give ~ 700, not the 27 that one fp32 evaluation in torch's order happens to need).
  * the kernels use __expf(x) = v_exp_f32(x * log2(e)): the argument x = logit - max carries one rounding (u |x|), the product
    with the rounded constant 1.5 u |x|, the instruction 2 u: a relative error of (2 + 2.5 |x|) u.  |x| is at most the logit
    spread X of the softmax it belongs to, so a softmax WEIGHT costs 2 + 2.5 X; in a softmax DENOMINATOR the weights average
    |x| to sum_c p_c |x_c| <= log(n).  X is measured from the case's inputs (never from a result) and every test input keeps
    X <= 80: beyond e^-87 the fp32 exponential leaves the normal range and no relative bound holds.
  * a division by the denominator is a reciprocal and a product: 3.
Linear attention (p = row softmax of q over hd channels, spread Xq; k = column softmax of K over the live rows, spread Xk;
T = rows, n = number of 64-row chunks, every online-softmax rescale is an exponential and a product: 3 per chunk + merge):
    p weight   g_p  = (2 + 2.5 Xq) + (hd + 2 + 2.5 log hd) + 3                                    = hd + 7 + 2.5 (Xq + log hd)
    kstat sum  g_Z  = T + 2 + 2.5 log T + 3 (n + 1)
    A          g_A  = (2 + 2.5 Xk + 3 (n + 1)) + T + g_Z + 3                                      (numerator, sum, denominator, division)
    y          g_y  = g_p + hd
    dA         g_dA = g_p + T + 1
    dQ         g_dQ = 2 g_p + 2 hd + 2        t = dy . A^T costs hd, the inner sum g_p + hd + hd, the difference 1, the outer p g_p + 1
    k weight of the backward, rebuilt from kstat:  g_k = 8 + 2.5 Xk   (difference, exponential, the fp32 kstat, reciprocal, product)
    dV         g_dV = g_k + hd
    dK         g_dK = 2 g_k + hd + T + 2      the column term costs g_k + hd + T over the rows (hd + 1 from A and dA on the matrix cores)
bf16 I/O: the inputs are rounded to bf16 once and the SAME values go to the kernel and the reference; a bf16 output adds
2^-8 |ref|; where the product itself runs on bf16 operands (apply_mfma_kernel, apply_bwd_mfma_kernel and ctx_bwd_mfma_kernel
with bf16 rows round both operands as they leave LDS) 2 * 2^-8 M is added.  The context build with bf16 rows is the fp32
arithmetic on the same values: bit-equal to hig_linattn_ctx.
The M of y, dQ, dV and dK are built from |A| and |dA| of the fp32 operand the call was given (A and dA are inputs of those
entry points), which is never larger than the sum_r k |v| form.
Full attention: see `full_bounds`.
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from hig_amd import _lib  # noqa: E402
from attn_dispatch_cases import (APPLY_STY, APPLY_STY_B, APPLY_STY_T, CALLS, LIN_TABLE, MFMA_ALL, MFMA_ONE, MFMA_PART, PATHS, VALU, WAVE,  # noqa: E402
                                 full_paths, in_regime, plan)
import attn_dispatch_cases  # noqa: E402

DEV = "cuda"
U = 2.0 ** -24
FLOOR = 2.0 ** -120     # products of two weights near e^-80 reach the subnormal range, which the matrix cores flush
CH = 64                 # rows per chunk of the linear-attention kernels
SENTINEL = {torch.float32: (torch.int32, 0x7FC0BEEF), torch.bfloat16: (torch.int16, 0x7FD5)}   # NaN patterns
F32, BF16 = torch.float32, torch.bfloat16
IO = {attn_dispatch_cases.F32: F32, attn_dispatch_cases.BF16: BF16}   # the shared tables name the I/O type, this file uses the dtype
IO_NAME = {v: k for k, v in IO.items()}


def lib():
    return _lib.lib()


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def counts():
    assert _lib.ATTN_NPATHS == len(PATHS) and lib().hig_attn_path_launches(len(PATHS)) == -1
    return [lib().hig_attn_path_launches(getattr(_lib, "ATTN_PATH_" + n)) for n in PATHS]


def planned(entry, io, B, rows, H, hd, Tk=0, scratch=True):
    """What hig_attn_plan answers for this call on the device at hand (its CU count, big dynamic LDS granted): (path, split)."""
    rc, path, split, _ = plan(entry, IO_NAME[io], B, rows, H, hd, Tk=Tk, scratch=scratch, chip_cus=ncu(), big_lds_ok=1)
    assert rc == 0, "the plan refuses the call (%d)" % rc
    return path, split


def counted(call, path, regime, nblocks, ask):
    """call() -> rc; asks the plan first (ask = the arguments of `planned`), then asserts rc == 0, that exactly the planned
    counter, which is that of `path`, moved by one, that hig_attn_last_split() is the planned split, and the split regime (see
    the module docstring; nblocks = the chunks / blocks one (sample, head) has).  Returns the split."""
    want = planned(*ask)
    before = counts()
    _lib.check(call())
    torch.cuda.synchronize()
    moved = {n: a - b for n, a, b in zip(PATHS, counts(), before) if a != b}
    assert moved == {want[0]: 1}, "the plan named %s, the call launched %s" % (want[0], moved)
    assert moved == {path: 1}, "expected one launch of %s, got %s" % (path, moved)
    split = lib().hig_attn_last_split()
    assert split == want[1], "the plan named split %d, the call reports %d" % (want[1], split)
    ok = in_regime(regime, split, nblocks)
    if not ok and ncu() != 256:   # the table is written for (and never skips on) the 256 CUs of the MI355X
        pytest.skip("split %d of %d blocks: the '%s' regime of %s is not reached by this shape with %d CUs" % (split, nblocks, regime, path, ncu()))
    assert ok, "%s: split %d of %d blocks is not the '%s' regime" % (path, split, nblocks, regime)
    return split


class Guarded:
    """A (rows, cols) output inside a (rows + 2, cols + pad) buffer filled with a NaN pattern: row 0, row rows + 1 and the last
    `pad` columns are guard bands that must keep their bits.  pad = 0 for the outputs whose entry point takes no leading
    dimension (A, kstat, At16, dA, lse): guard rows only."""

    def __init__(self, rows, cols, dtype=F32, pad=8):
        self.rows, self.cols, self.ld, self.dtype = rows, cols, cols + pad, dtype
        itype, self.pat = SENTINEL[dtype]
        self.buf = torch.full(((rows + 2) * self.ld,), self.pat, dtype=itype, device=DEV)
        self.out = self.buf.view(dtype)[self.ld:self.ld + rows * self.ld].view(rows, self.ld)[:, :cols]

    def ptr(self, col=0):
        return C.c_void_p(self.out.data_ptr() + col * self.out.element_size())

    def verify(self, what):
        b = self.buf.view(self.rows + 2, self.ld)
        keep = torch.ones_like(b, dtype=torch.bool)
        keep[1:self.rows + 1, :self.cols] = False
        assert (b[keep] == self.pat).all(), "%s: a store landed in the guard band" % what
        assert torch.isfinite(self.out.float()).all(), "%s: not every element was written" % what
        return self.out


def P(t, col=0):
    return None if t is None else C.c_void_p(t.data_ptr() + col * t.element_size())


def at16_order(A):
    """The transposed, bf16-rounded context matrices in the element order the library keeps them in (hig_at16_offset,
    csrc/hig_common.h; the same statement as in test_gpu_bf16_storage.py).  A: (B, H, hd, hd) indexed [c][l]."""
    B, H, hd, _ = A.shape
    At = A.transpose(2, 3).to(BF16).contiguous()                              # [l][c]
    v = At.view(B, H, hd // 32, 32, hd // 16, 2, 8)                           # (lb, l32, ks, half, j)
    return v.permute(0, 1, 2, 4, 5, 3, 6).contiguous().view(B, H, hd, hd)     # (lb, ks, half, l32, j)


def held(what, out, ref, bound, report, M=None, gamma=None):
    """Every element of `out` within `bound` of `ref`.  Records the largest |err| / bound in `report` and, given M and gamma,
    the measured multiple of 2^-24 M next to the derived gamma."""
    err = (out.double() - ref).abs()
    ratio = (err / bound).max().item()
    report.append("%s %.3f" % (what, ratio) + ("" if M is None else " (%.1f of %.0f)" % ((err / (U * M + FLOOR)).max().item(), gamma)))
    assert ratio <= 1.0, "%s: |err| / bound = %.3f at %s" % (what, ratio, tuple(torch.nonzero(err / bound == (err / bound).max())[0].tolist()))
    return ratio


# ----------------------------------------------------------------------------------------------------------------------
# linear attention
# ----------------------------------------------------------------------------------------------------------------------
def lengths_for(B, T):
    """0, 1, 63, 64, 65, T - 1, T (those that fit in T), repeated over the batch."""
    pat = sorted({v for v in (0, 1, 63, 64, 65, T - 1, T) if 0 <= v <= T})
    return torch.tensor([pat[i % len(pat)] for i in range(B)], dtype=torch.int64)


def lin_inputs(B, T, H, hd, seed, adversarial=False, lens=None):
    """qkv (B T, 3 d) and dy (B T, d), fp32 on the host.  Plain: randn * 4 clipped to +-15 (spread <= 30).  adversarial: see
    test_linear_adversarial_logits."""
    d = H * hd
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B, T, 3 * d, generator=g) * 4).clamp_(-15, 15)
    dy = torch.randn(B, T, d, generator=g)
    if adversarial:
        q, k = qkv[..., :d], qkv[..., d:2 * d]
        k.clamp_(-9, 9)
        for b in range(B):
            n = int(lens[b]) if lens is not None else T
            if n < 1:
                continue
            last0 = ((n - 1) // CH) * CH                      # first row of the last live chunk
            ramp = torch.linspace(0, 1, n) if n > 1 else torch.zeros(1)
            for c in range(d):
                kind = c % 6
                if kind == 0:
                    k[b, 0, c] += 60                          # the column maximum in the first row
                elif kind == 1:
                    k[b, n - 1, c] += 60                      # ... in the last live row
                elif kind == 2:
                    k[b, last0 + (c // 6) % (n - last0), c] += 60   # ... in the last chunk only
                elif kind == 3:
                    k[b, :n, c] = 39 - 78 * ramp + k[b, :n, c] / 9  # falls by 78 (+-1) from the first chunk to the last
                elif kind == 4:
                    k[b, :n, c] = -39 + 78 * ramp + k[b, :n, c] / 9  # rises by 78
        qv = q.reshape(B * T, H, hd).clone()
        qv[0::3] = qv[0::3].clamp(-1, 1)
        idx = torch.arange(0, B * T, 3)
        qv[idx, :, idx % hd] += 78                            # one channel 78 above the rest (+-1)
        qv[1::3] = 3.0                                        # rows of equal values
        qkv[..., :d] = qv.reshape(B, T, d)
    return qkv.reshape(B * T, 3 * d), dy.reshape(B * T, d)


def lin_reference(qkv, dy, A32, dA32, B, T, H, hd, lens):
    """fp64 statement of the four operators on the device, with the magnitudes M of the module docstring.  qkv, dy: the values
    the kernels get (fp32 or bf16), A32 / dA32: the fp32 operands handed to apply / apply_bwd / ctx_bwd (None: not needed)."""
    d = H * hd
    x = qkv.double().view(B, T, 3, H, hd)
    q, K, V = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    live = (torch.arange(T, device=DEV)[None] < lens.to(DEV)[:, None]) if lens is not None else torch.ones(B, T, dtype=torch.bool, device=DEV)
    lm = live[:, :, None, None]
    r = {}
    p = torch.softmax(q, -1)
    Km = K.masked_fill(~lm, float("-inf"))
    kmax = Km.amax(1)                                                          # (B, H, hd)
    e = torch.exp(Km - kmax[:, None].nan_to_num(neginf=0.0)).masked_fill(~lm, 0.0)
    Z = e.sum(1)
    k = e / Z.clamp_min(1e-300)[:, None]
    v = V * lm
    r["Xq"] = (q.amax(-1) - q.amin(-1)).max().item()
    r["Xk"] = (kmax[:, None] - K).masked_fill(~lm, 0.0).max().item()
    empty = ~live.any(1)
    r["kmax"] = kmax.masked_fill(empty[:, None, None], 0.0).reshape(B, d)
    r["Z"] = Z.masked_fill(empty[:, None, None], 1.0).reshape(B, d)
    r["A"] = torch.einsum("bnhc,bnhl->bhcl", k, v)
    r["MA"] = torch.einsum("bnhc,bnhl->bhcl", k, v.abs())
    if A32 is not None:
        Ad, dyd = A32.double(), dy.double().view(B, T, H, hd)
        r["y"] = torch.einsum("bnhc,bhcl->bnhl", p, Ad).reshape(B * T, d)
        r["My"] = torch.einsum("bnhc,bhcl->bnhl", p, Ad.abs()).reshape(B * T, d)
        r["dA"] = torch.einsum("bnhc,bnhl->bhcl", p, dyd)
        r["MdA"] = torch.einsum("bnhc,bnhl->bhcl", p, dyd.abs())
        t = torch.einsum("bnhl,bhcl->bnhc", dyd, Ad)
        Tm = torch.einsum("bnhl,bhcl->bnhc", dyd.abs(), Ad.abs())
        r["dQ"] = (p * (t - (p * t).sum(-1, keepdim=True))).reshape(B * T, d)
        r["MdQ"] = (p * (Tm + (p * Tm).sum(-1, keepdim=True))).reshape(B * T, d)
    if dA32 is not None:
        dAd = dA32.double()
        r["dV"] = (torch.einsum("bnhc,bhcl->bnhl", k, dAd) * lm).reshape(B * T, d)
        r["MdV"] = (torch.einsum("bnhc,bhcl->bnhl", k, dAd.abs()) * lm).reshape(B * T, d)
        s = torch.einsum("bnhl,bhcl->bnhc", v, dAd)
        Sm = torch.einsum("bnhl,bhcl->bnhc", v.abs(), dAd.abs())
        r["dK"] = (k * (s - (k * s).sum(1, keepdim=True))).reshape(B * T, d)
        r["MdK"] = (k * (Sm + (k * Sm).sum(1, keepdim=True))).reshape(B * T, d)
    r["live"] = live.reshape(B * T)
    return r


def lin_gammas(T, hd, Xq, Xk):
    """The rounding counts of the module docstring."""
    n = (T + CH - 1) // CH
    g_p = hd + 7 + 2.5 * (Xq + math.log(hd))
    g_Z = T + 2 + 2.5 * math.log(T) + 3 * (n + 1)
    g_k = 8 + 2.5 * Xk
    return {"Z": g_Z, "A": (2 + 2.5 * Xk + 3 * (n + 1)) + T + g_Z + 3, "y": g_p + hd, "dA": g_p + T + 1,
            "dQ": 2 * g_p + 2 * hd + 2, "dV": g_k + hd, "dK": 2 * g_k + hd + T + 2}


def run_linear(B, T, H, hd, io, expect, seed=0, use_lens=True, adversarial=False, entries=None, inputs=None):
    """Runs ctx (with and without scratch), apply, apply_bwd and ctx_bwd of one storage type on one set of inputs.  expect:
    {entry: (path, regime)} for the entries 'ctx_s' (scratch), 'ctx_n' (NULL scratch), 'apply', 'apply_bwd', 'ctx_bwd'.  Every
    entry is called twice on fresh NaN-filled guarded outputs and must give the same bits (fixed-order merges); returns
    (results, report lines)."""
    d, L, s = H * hd, lib(), _lib.stream_ptr()
    nchunk = (T + CH - 1) // CH
    lens = lengths_for(B, T) if use_lens else None
    qkv_h, dy_h = inputs if inputs is not None else lin_inputs(B, T, H, hd, seed, adversarial, lens)
    qkv, dy = qkv_h.to(DEV).to(io), dy_h.to(DEV).to(io)
    lg = None if lens is None else lens.to(DEV)
    bf = io == BF16
    ref = lin_reference(qkv, dy, None, None, B, T, H, hd, lens)
    assert ref["Xq"] <= 80 and ref["Xk"] <= 80, "test inputs must keep every logit spread at or under 80"
    g = lin_gammas(T, hd, ref["Xq"], ref["Xk"])
    # the fp32 operands of the later entry points: the fp64 results rounded once (each entry is judged on its own arithmetic)
    A32 = ref["A"].float()
    kst32 = torch.stack([ref["kmax"], ref["Z"]], -1).float().contiguous()
    ref.update({k_: v_ for k_, v_ in lin_reference(qkv, dy, A32, None, B, T, H, hd, lens).items() if k_ not in ref})
    dA32 = ref["dA"].float()
    ref.update({k_: v_ for k_, v_ in lin_reference(qkv, dy, None, dA32, B, T, H, hd, lens).items() if k_ not in ref})
    out16 = 2.0 ** -8 if bf else 0.0
    mm16 = 2 * 2.0 ** -8 if bf else 0.0     # products on bf16 operands (apply / apply_bwd / ctx_bwd with bf16 rows)
    res, report = {}, ["%s B=%d T=%d H=%d hd=%d Xq=%.0f Xk=%.0f:" % ("bf16" if bf else "fp32", B, T, H, hd, ref["Xq"], ref["Xk"])]
    Kp, Vp = P(qkv, d), P(qkv, 2 * d)
    mult = lambda name, m: () if bf else (ref[m], g[name])   # noqa: E731  (bf16: the 2^-8 terms dominate, only |err| / bound is shown)

    def twice(entry, make, call, nblocks):
        path, regime = expect[entry]
        outs = []
        for _ in range(2):
            bufs = make()
            split = counted(lambda: call(*bufs), path, regime, nblocks, (CALLS[entry][0], io, B, T, H, hd, 0, CALLS[entry][1]))
            outs.append([b_.verify(entry) for b_ in bufs if isinstance(b_, Guarded)])
        for a, b_ in zip(*outs):
            assert torch.equal(a, b_), "%s: two calls on the same inputs differ" % entry
        report.append("%s -> %s split %d/%d;" % (entry, path, split, nblocks))
        return outs[0]

    for entry in ("ctx_s", "ctx_n"):
        if entries is not None and entry not in entries:
            continue
        scr = torch.zeros(L.hig_linattn_ctx_scratch_floats(B, T, H, hd), device=DEV) if entry == "ctx_s" else None
        make = lambda: (Guarded(B * H * hd, hd, pad=0), Guarded(B * d, 2, pad=0)) + ((Guarded(B * H * hd, hd, BF16, pad=0),) if bf else ())  # noqa: E731
        if bf:
            call = lambda A, ks, At: L.hig_linattn_ctx_bf16(Kp, Vp, 3 * d, B, T, H, hd, P(lg), A.ptr(), ks.ptr(), P(scr), At.ptr(), s)  # noqa: E731
        else:
            call = lambda A, ks: L.hig_linattn_ctx(Kp, Vp, 3 * d, B, T, H, hd, P(lg), A.ptr(), ks.ptr(), P(scr), s)  # noqa: E731
        outs = twice(entry, make, call, nchunk)
        A, ks = outs[0].reshape(B, H, hd, hd), outs[1].reshape(B, d, 2)
        held(entry + " A", A, ref["A"], g["A"] * U * ref["MA"] + FLOOR, report, ref["MA"], g["A"])
        assert torch.equal(ks[..., 0].double(), ref["kmax"]), entry + ": the column maximum is exact"
        held(entry + " kstat", ks[..., 1], ref["Z"], g["Z"] * U * ref["Z"], report, ref["Z"], g["Z"])
        if lens is not None:
            e0 = (lens == 0).to(DEV)
            assert (A[e0] == 0).all() and (ks[e0][..., 0] == 0).all() and (ks[e0][..., 1] == 1).all(), "length 0: A = 0, kstat = (0, 1)"
        if bf:
            assert torch.equal(outs[2].reshape(B, H, hd, hd), at16_order(A)), entry + ": At16 is not the at16_order of A"
        res[entry] = (A, ks)

    if entries is None or "apply" in entries:
        make = lambda: (Guarded(B * T, d, io),)  # noqa: E731
        fn = L.hig_linattn_apply_bf16 if bf else L.hig_linattn_apply
        call = lambda Y: fn(P(qkv), 3 * d, P(A32), Y.ptr(), Y.ld, B, T, H, hd, s)  # noqa: E731
        y, = twice("apply", make, call, nchunk)
        held("y", y, ref["y"], (g["y"] * U + mm16) * ref["My"] + out16 * ref["y"].abs() + FLOOR, report, *mult("y", "My"))
        res["apply"] = y

    if entries is None or "apply_bwd" in entries:
        scr = torch.zeros(L.hig_linattn_bwd_scratch_floats(B, T, H, hd), device=DEV)
        make = lambda: (Guarded(B * T, d, io), Guarded(B * H * hd, hd, pad=0))  # noqa: E731
        fn = L.hig_linattn_apply_bwd_bf16 if bf else L.hig_linattn_apply_bwd
        call = lambda dQ, dA: fn(P(dy), d, P(qkv), 3 * d, P(A32), dQ.ptr(), dQ.ld, dA.ptr(), B, T, H, hd, P(scr), s)  # noqa: E731
        dQ, dA = twice("apply_bwd", make, call, nchunk)
        held("dQ", dQ, ref["dQ"], (g["dQ"] * U + mm16) * ref["MdQ"] + out16 * ref["dQ"].abs() + FLOOR, report, *mult("dQ", "MdQ"))
        held("dA", dA.reshape(B, H, hd, hd), ref["dA"], (g["dA"] * U + mm16) * ref["MdA"] + FLOOR, report, *mult("dA", "MdA"))
        res["apply_bwd"] = (dQ, dA)

    if entries is None or "ctx_bwd" in entries:
        scr = torch.zeros(L.hig_linattn_bwd_scratch_floats(B, T, H, hd), device=DEV)
        make = lambda: (Guarded(B * T, d, io), Guarded(B * T, d, io))  # noqa: E731
        if bf:
            call = lambda dK, dV: L.hig_linattn_ctx_bwd_bf16(P(dA32), P(A32), Kp, Vp, 3 * d, P(kst32), P(lg), dK.ptr(), dV.ptr(), dK.ld,  # noqa: E731
                                                             B, T, H, hd, s)
        else:
            call = lambda dK, dV: L.hig_linattn_ctx_bwd(P(dA32), P(A32), Kp, Vp, 3 * d, P(kst32), P(lg), dK.ptr(), dV.ptr(), dK.ld,  # noqa: E731
                                                        B, T, H, hd, P(scr), s)
        dK, dV = twice("ctx_bwd", make, call, nchunk)
        held("dV", dV, ref["dV"], (g["dV"] * U + mm16) * ref["MdV"] + out16 * ref["dV"].abs() + FLOOR, report, *mult("dV", "MdV"))
        held("dK", dK, ref["dK"], (g["dK"] * U + mm16) * ref["MdK"] + out16 * ref["dK"].abs() + FLOOR, report, *mult("dK", "MdK"))
        dead = ~ref["live"]
        assert (dK[dead] == 0).all() and (dV[dead] == 0).all(), "rows at or beyond the length: dK = dV = 0 exactly"
        res["ctx_bwd"] = (dK, dV)
    report.append("gamma " + " ".join("%s=%.0f" % kv for kv in g.items()))
    print(" ".join(report))
    return res, report


def batch_for(bh, H):
    """B with B * H == bh, or a skip when H does not divide it on this device."""
    if bh < H or bh % H:
        pytest.skip("B * H = %d is not a multiple of H = %d on a device with %d CUs" % (bh, H, ncu()))
    return bh // H


def regime_bh(name, H):
    """B * H of the named occupancy regime on the device at hand."""
    return attn_dispatch_cases.regime_bh(name, H, ncu())


@pytest.mark.parametrize("case", LIN_TABLE, ids=[c[0] for c in LIN_TABLE])
def test_linear_dispatch_table(case):
    """One row per (entry, path, split regime): the launch counters and hig_attn_last_split prove the row ran what it names,
    every output is NaN-filled and guarded, every element is held to the bound of the module docstring, and every sample
    length of `lengths_for` (0, 1, 63, 64, 65, T - 1, T) is in the batch: length 0 gives A = 0, kstat = (0, 1) and zero
    gradients, rows at or beyond the length get dK = dV = 0 exactly."""
    _, io, hd, H, regime, T, expect = case
    run_linear(batch_for(regime_bh(regime, H), H), T, H, hd, IO[io], expect, seed=T + hd)


@pytest.mark.parametrize("hd,H,regime,expect", [(64, 8, "few", dict(MFMA_ALL, apply=("APPLY_MFMA", "all"))),
                                                 (128, 4, "ncu", dict(MFMA_ONE, apply=("APPLY_MFMA", "one"))),
                                                 (32, 4, "few", VALU)], ids=["hd64-few", "hd128-ncu", "hd32"])
def test_linear_text_side_no_length_pointer(hd, H, regime, expect):
    """T = 77 with length == NULL (the text side of cross attention): every row is live."""
    run_linear(batch_for(regime_bh(regime, H), H), 77, H, hd, F32, expect, seed=77, use_lens=False)


ADVERSARIAL = [
    ("ctx_kernel+apply_kernel", F32, 32, 3, "few", 196, VALU),
    ("ctx_part+ctx_mfma+wave64", F32, 64, 8, "few", 300, dict(MFMA_ALL, apply=WAVE)),
    ("ctx_mfma-walk+apply_mfma-f32", F32, 128, 8, "ncu", 196, dict(MFMA_ONE, apply=("APPLY_MFMA", "one"))),
    ("partial-hd128", F32, 128, 8, "half", 300, dict(MFMA_PART, apply=("APPLY_MFMA", "partial"))),
    ("partial-hd64", F32, 64, 8, "half", 300, dict(MFMA_PART, apply=WAVE)),
    ("bf16-hd64", BF16, 64, 8, "ncu", 300, dict(MFMA_ONE, apply=("APPLY_MFMA", "partial"))),
    ("bf16-hd128-part", BF16, 128, 8, "half", 300, dict(MFMA_PART, apply=("APPLY_MFMA", "partial"))),
]


@pytest.mark.parametrize("case", ADVERSARIAL, ids=[c[0] for c in ADVERSARIAL])
def test_linear_adversarial_logits(case):
    """Logit spreads up to 80 (asserted on the inputs; beyond e^-87 fp32 has no relative accuracy left) on every context-build and
    apply path.  Columns of K, by index mod 6: the maximum (+60) in the first row / in the last live row / in the last live
    chunk only (everything accumulated before is rescaled by about e^-60); values falling by 78 from the first chunk to the
    last / rising by 78; plain.  Query rows: one channel 78 above the rest; all channels equal; plain.  Then a finite 1e4 is
    put in K and in V on the masked rows: every result must be bit-identical to the call with the plain values there."""
    _, io, hd, H, regime, T, expect = case
    B = batch_for(regime_bh(regime, H), H)
    lens = lengths_for(B, T)
    qkv, dy = lin_inputs(B, T, H, hd, 5, adversarial=True, lens=lens)
    base, _ = run_linear(B, T, H, hd, io, expect, inputs=(qkv, dy))
    d = H * hd
    dead = (torch.arange(T)[None] >= lens[:, None]).reshape(B * T)
    poisoned = qkv.clone()
    poisoned[dead, d:] = 1e4
    again, _ = run_linear(B, T, H, hd, io, expect, inputs=(poisoned, dy), entries=("ctx_s", "ctx_n", "ctx_bwd"))
    for entry in ("ctx_s", "ctx_n", "ctx_bwd"):
        for a, b in zip(base[entry], again[entry]):
            assert torch.equal(a, b), "%s: a finite value on a masked row reached the result" % entry


@pytest.mark.parametrize("io,hd,H,regime,T,apply", [(F32, 32, 4, "few", 129, ("APPLY", "all")), (F32, 64, 8, "half", 196, WAVE),
                                                     (F32, 64, 8, "ncu", 100, ("APPLY_MFMA", "all")),
                                                     (F32, 128, 8, "ncu", 300, ("APPLY_MFMA", "one")),
                                                     (BF16, 64, 8, "2ncu", 300, ("APPLY_MFMA", "partial"))],
                         ids=["apply_kernel", "wave64", "apply_mfma-hd64", "apply_mfma-hd128", "apply_mfma-bf16"])
def test_apply_forward_does_not_depend_on_the_batch_split(io, hd, H, regime, T, apply):
    """A row of y depends on its own q and on A[b, h] only, whichever workgroup computes it: the two halves of a batch, run on
    their own (half the (sample, head) pairs: another split of the chunks), give the bits of the whole.  The context build and
    the backward kernels change PATH and summation order with B * H (partial sums per workgroup), so equal bits are not
    their contract: test_linear_dispatch_table holds the same shapes to the bound at ncu / 2, ncu and 2 ncu instead."""
    B = batch_for(regime_bh(regime, H), H)
    d, L, s = H * hd, lib(), _lib.stream_ptr()
    qkv_h, _ = lin_inputs(B, T, H, hd, 9)
    qkv = qkv_h.to(DEV).to(io)
    A = torch.randn(B, H, hd, hd, generator=torch.Generator().manual_seed(1)).to(DEV)
    fn = L.hig_linattn_apply_bf16 if io == BF16 else L.hig_linattn_apply
    nchunk = (T + CH - 1) // CH
    whole = Guarded(B * T, d, io)
    counted(lambda: fn(P(qkv), 3 * d, P(A), whole.ptr(), whole.ld, B, T, H, hd, s), apply[0], apply[1], nchunk, ("apply", io, B, T, H, hd))
    y = whole.verify("whole")
    h = B // 2
    for lo, n in ((0, h), (h, B - h)):
        part = Guarded(n * T, d, io)
        _lib.check(fn(P(qkv[lo * T:]), 3 * d, P(A[lo:]), part.ptr(), part.ld, n, T, H, hd, s))
        torch.cuda.synchronize()
        assert torch.equal(part.verify("half"), y[lo * T:(lo + n) * T]), "a half of the batch differs from the whole"


@pytest.mark.parametrize("io,hd,H,path,regime", [(IO[c[0]],) + c[1:] for c in APPLY_STY])
@pytest.mark.parametrize("T", APPLY_STY_T)
def test_apply_sty_dispatch_and_guards(io, hd, H, path, regime, T):
    """hig_linattn_apply_sty / _bf16: which kernel runs, every output written, nothing around it (the values are held by
    test_gpu_apply_sty32.py and test_gpu_bf16_storage.py).  The strips of apply_sty_wave64_kernel are a launch-geometry
    choice, not a regime of this file: its split is only required to lie in 1 .. number of 16-row tiles."""
    B, d, L, s = APPLY_STY_B, H * hd, lib(), _lib.stream_ptr()
    g = torch.Generator().manual_seed(T)
    q = (torch.randn(B * T, d, generator=g) * 2).to(DEV).to(io)
    A = (torch.randn(B, H, hd, hd, generator=g) * 0.5).to(DEV)
    gamma, beta, ss = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV), (0.3 * torch.randn(B, 2 * d, generator=g)).to(DEV)
    fn = L.hig_linattn_apply_sty_bf16 if io == BF16 else L.hig_linattn_apply_sty
    outs = []
    for _ in range(2):
        o = Guarded(B * T, d, io)
        before = counts()
        _lib.check(fn(P(q), d, P(A), P(gamma), P(beta), P(ss), 2 * d, d, o.ptr(), o.ld, B, T, H, hd, s))
        torch.cuda.synchronize()
        assert {n: a - b for n, a, b in zip(PATHS, counts(), before) if a != b} == {path: 1}
        split = lib().hig_attn_last_split()
        assert (path, split) == planned("apply_sty", io, B, T, H, hd), "the call did not do what its plan named"
        assert split == 1 if regime == "one" else 1 <= split <= (T + 15) // 16
        outs.append(o.verify(path))
    assert torch.equal(*outs), "two calls on the same inputs differ"


# ----------------------------------------------------------------------------------------------------------------------
# full attention
# ----------------------------------------------------------------------------------------------------------------------
def full_reference(q, kv, dy, B, Tq, Tk, H, hd, qlen, kpad, lse_in=None, y_in=None):
    """fp64 statement of no_eff attention with the magnitudes of `full_bounds`.  Rows n >= qlen[b] carry the reference's -1e5
    offset WITH its fp32 rounding (logits quantised to 2^-7 there).  The backward is stated on what hig_fullattn_bwd is GIVEN:
    w = exp(S - lse_in), delta = sum_l dy y_in (each entry point is judged on its own arithmetic, as for linear attention)."""
    d = H * hd
    qd, kd, vd = q.double().view(B, Tq, H, hd), kv.double()[:, :d].reshape(B, Tk, H, hd), kv.double()[:, d:].reshape(B, Tk, H, hd)
    isq = 1.0 / math.sqrt(hd)
    S = torch.einsum("bnhd,bmhd->bhnm", qd, kd) * isq
    MS = torch.einsum("bnhd,bmhd->bhnm", qd.abs(), kd.abs()) * isq
    valid = torch.ones(B, Tq, dtype=torch.bool, device=q.device) if qlen is None else torch.arange(Tq, device=q.device)[None] < qlen[:, None]
    S0 = S
    S = torch.where(valid[:, None, :, None], S, (S.float() + (-100000.0)).double())
    if kpad is not None:
        km = kpad.bool()[:, None, None, :]
        S, S0, MS = S.masked_fill(km, float("-inf")), S0.masked_fill(km, float("-inf")), MS.masked_fill(km, 0.0)
    lse = torch.logsumexp(S, -1)
    w = torch.exp(S - lse[..., None])
    r = {"valid": valid, "lse": lse, "w": w, "Smax": S0.abs().masked_fill(S0.isinf(), 0.0).amax(-1), "MSmax": MS.amax(-1),
         "X": (lse[..., None] - S).masked_fill(S.isinf(), 0.0).amax(-1), "MS": MS, "S0": S0, "S": S, "va": vd.abs()}
    r["y"] = torch.einsum("bhnm,bmhl->bnhl", w, vd)
    r["My"] = torch.einsum("bhnm,bmhl->bnhl", w, vd.abs())
    if dy is not None:
        dyd = dy.double().view(B, Tq, H, hd)
        dP, aP = torch.einsum("bnhl,bmhl->bhnm", dyd, vd), torch.einsum("bnhl,bmhl->bhnm", dyd.abs(), vd.abs())
        lse_b = lse_in.double().reshape(B, H, Tq)
        w = r["wb"] = torch.exp(S - lse_b[..., None])
        r["xb"] = (lse_b[..., None] - S).abs().masked_fill(S.isinf(), 0.0)
        r["lse_b"] = lse_b
        y_b = y_in.double().reshape(B, Tq, H, hd)
        dS = w * (dP - (dyd * y_b).sum(-1).permute(0, 2, 1)[..., None])
        r["MdS"] = w * (aP + (dyd.abs() * y_b.abs()).sum(-1).permute(0, 2, 1)[..., None])
        r["dQ"] = torch.einsum("bhnm,bmhd->bnhd", dS, kd) * isq
        r["dK"] = torch.einsum("bhnm,bnhd->bmhd", dS, qd) * isq
        r["dV"] = torch.einsum("bhnm,bnhl->bmhl", w, dyd)
        r["qa"], r["ka"], r["dya"] = qd.abs() * isq, kd.abs() * isq, dyd.abs()
    return r


def full_bounds(r, B, Tq, Tk, H, hd):
    """Per-row rounding counts of the full-attention kernels (u = 2^-24), by the conventions of the module docstring:
      logit      S = q . k / sqrt(hd): hd + 1 roundings relative to MS = sum_d |q_d k_d| / sqrt(hd), so an absolute error of
                 (hd + 1) MS u, plus u (|S| + |lse|) for each difference S - max / S - lse it enters:
                 delta_nm = (hd + 3) MS_nm + 3 (|S_nm| + |lse_n|)                    (in units of u, absolute)
      weight     w_nm = exp(S - lse): the numerator costs e_nm = delta_nm + 2 + 2.5 (lse_n - S_nm) (the exponential; the test
                 inputs keep lse_n - S_nm <= 80 + log Tk), the denominator the w-weighted mean of e plus the running sum's Tk
                 terms and one rescale (3) per 32-key chunk:  D_n = sum_m w_nm e_nm + Tk + 3 ceil(Tk / 32) + 3
      y          sum_m w_nm (e_nm + D_n + Tk + 2) |v_ml|
      lse        the issue's form, absolute: g_lse u (1 + max_m |S_nm|), g_lse = (hd + 2) + Tk + 3 ceil(Tk / 32) + 6.5 log Tk + 8
                 (the dot product, the sum, the rescales, 2.5 log Tk of exponential arguments + 4 log Tk for __logf and the
                 final sum).  The dot product's share is really proportional to MS, not to |S|: this form is tight only while
                 the cancellation inside q . k is mild, which holds for every input here (the measured multiple is printed).
      backward   w is rebuilt per element as exp(S - lse) from the lse the call is GIVEN (no sum, no rescale):
                 g_wb(n, m) = (hd + 2) MS_nm + 2 (|S_nm| + |lse_n|) + 2.5 |S_nm - lse_n| + 4.
                 dS = w (dP - delta), dP = dy . v^T (hd), delta = sum_l dy y (hd + 1): g_dS = g_wb + 2 hd + 3 on
                 MdS = w (|dy| . |v| + sum_l |dy y|);  dQ sums g_dS + Tk + 2 over the keys, dK g_dS + Tq + 2 and dV g_wb + Tq + 2 over
                 the query rows, each term with its own count.  Rows n >= qlen[b] have dy = 0: every term they feed is exactly 0.
      The counts of the weights are large (thousands at hd 128) because a logit's worst case is LINEAR in hd times
      MS = sum_d |q_d k_d| / sqrt(hd) ~ 16 - 40 here, and a logit's absolute error is a weight's relative error; the measured
      multiples (printed) stay near the square root of that.
    Rows n >= qlen[b]: the logits are quantised to the fp32 grid at 1e5, 2^-7; the kernel's fp32 logit can land one grid step from
    the reference's, in the maximum and in every term of the sum: 3 * 2^-7 relative on the weights (y) and absolute on lse,
    on those rows only."""
    nk = (Tk + 31) // 32
    lse_mag = torch.where(r["valid"][:, None, :], r["lse"].abs(), torch.zeros_like(r["lse"]))   # (B, H, Tq); the offset rows: see below
    S0a = r["S0"].abs().masked_fill(r["S0"].isinf(), 0.0)
    x = (r["lse"][..., None] - r["S"]).masked_fill(r["S"].isinf(), 0.0)
    e = (hd + 3) * r["MS"] + 3 * (S0a + lse_mag[..., None]) + 2 + 2.5 * x
    D = (r["w"] * e).sum(-1) + Tk + 3 * nk + 3
    g_w = e.amax(-1) + D
    g_lse = (hd + 2) + Tk + 3 * nk + 6.5 * math.log(Tk) + 8
    pad = (~r["valid"])[:, None, :].double() * 3 * 2.0 ** -7
    b = {"g_w": g_w, "g_lse": g_lse}
    b["lse"] = g_lse * U * (1 + r["Smax"]) + pad
    b["y"] = U * torch.einsum("bhnm,bmhl->bnhl", r["w"] * (e + (D + Tk + 2 + pad / U)[..., None]), r["va"]) + FLOOR
    if "MdS" in r:
        live = r["valid"][:, None, :, None]
        g_wb = (hd + 2) * r["MS"] + 2 * (r["S0"].abs().masked_fill(r["S0"].isinf(), 0.0) + r["lse_b"].abs()[..., None] * live) + 2.5 * r["xb"] + 4
        g_dS = g_wb + 2 * hd + 3
        b["g_wb"] = g_wb.max().item()
        b["dQ"] = U * torch.einsum("bhnm,bmhd->bnhd", (g_dS + Tk + 2) * r["MdS"], r["ka"]) + FLOOR
        b["dK"] = U * torch.einsum("bhnm,bnhd->bmhd", (g_dS + Tq + 2) * r["MdS"], r["qa"]) + FLOOR
        b["dV"] = U * torch.einsum("bhnm,bnhl->bmhl", (g_wb + Tq + 2) * r["wb"], r["dya"]) + FLOOR
        b["MdQ"] = torch.einsum("bhnm,bmhd->bnhd", r["MdS"], r["ka"])
        b["MdK"] = torch.einsum("bhnm,bnhd->bmhd", r["MdS"], r["qa"])
        b["MdV"] = torch.einsum("bhnm,bnhl->bmhl", r["wb"], r["dya"])
    return b


def full_inputs(B, Tq, Tk, H, hd, seed, spread80=False):
    d = H * hd
    g = torch.Generator().manual_seed(seed)
    q, kv, dy = torch.randn(B * Tq, d, generator=g) * 1.5, torch.randn(B * Tk, 2 * d, generator=g) * 1.5, torch.randn(B * Tq, d, generator=g)
    if spread80 and Tk > 40:
        # one late key chunk whose logits stand ~ 70 above the rest: k rows there are 70 sqrt(hd) / |q|^2 times the query
        # direction of the sample's first row (spread asserted <= 80 + log Tk through X in the bound)
        kk = kv.view(B, Tk, 2 * d)[:, :, :d].reshape(B, Tk, H, hd)
        q0 = q.view(B, Tq, H, hd)[:, 0]
        lo = ((Tk - 1) // 32) * 32 - 32
        kk[:, lo:lo + 32] = kk[:, lo:lo + 32] * 0.05 + (60 * math.sqrt(hd) * q0 / q0.square().sum(-1, keepdim=True))[:, None]
        kv.view(B, Tk, 2 * d)[:, :, :d] = kk.reshape(B, Tk, d)
    return q, kv, dy


def run_full(B, Tq, Tk, H, hd, io, fwd_path, bwd_path, qlens=None, kpad=None, seed=0, spread80=False, backward=True):
    """The forward (twice, same bits) on NaN-filled guarded y / lse, held to `full_bounds`; then hig_fullattn_bwd (twice) fed the
    forward's own y and lse, dy zeroed on the rows at or beyond qlen.  Asserts the path counters and, for the forward, that the
    split is the number of query blocks of its launch geometry."""
    d, L, s = H * hd, lib(), _lib.stream_ptr()
    bf = io == BF16
    q_h, kv_h, dy_h = full_inputs(B, Tq, Tk, H, hd, seed, spread80)
    q, kv = q_h.to(DEV).to(io), kv_h.to(DEV).to(io)
    lg = None if qlens is None else torch.tensor(qlens, dtype=torch.int64, device=DEV)
    kp = None if kpad is None else kpad.to(DEV)
    valid_h = torch.ones(B, Tq, dtype=torch.bool) if qlens is None else torch.arange(Tq)[None] < torch.tensor(qlens)[:, None]
    dy = (dy_h * valid_h.reshape(-1, 1)).to(DEV)     # rows at or beyond qlen take no gradient
    r = full_reference(q, kv, None, B, Tq, Tk, H, hd, lg, kp)
    assert r["X"][r["valid"][:, None, :].expand_as(r["X"])].max().item() <= 80 + math.log(Tk), "logit spread above 80"
    report = ["%s B=%d Tq=%d Tk=%d H=%d hd=%d:" % ("bf16" if bf else "fp32", B, Tq, Tk, H, hd)]
    rows_per_wg = 64 if fwd_path == "FULL_FWD" else None
    outs = []
    for _ in range(2):
        y, lse = Guarded(B * Tq, d, io), Guarded(B * H, Tq, pad=0)
        if bf:
            call = lambda: L.hig_fullattn_fwd_bf16(P(q), d, P(kv), P(kv, d), 2 * d, B, Tq, Tk, H, hd, P(lg), y.ptr(), y.ld, s)  # noqa: E731
        elif kp is not None:
            call = lambda: L.hig_fullattn_fwd_kpad(P(q), d, P(kv), P(kv, d), 2 * d, B, Tq, Tk, H, hd, P(lg), P(kp), y.ptr(), y.ld, lse.ptr(), s)  # noqa: E731
        else:
            call = lambda: L.hig_fullattn_fwd(P(q), d, P(kv), P(kv, d), 2 * d, B, Tq, Tk, H, hd, P(lg), y.ptr(), y.ld, lse.ptr(), s)  # noqa: E731
        before = counts()
        _lib.check(call())
        torch.cuda.synchronize()
        assert {n: a - b_ for n, a, b_ in zip(PATHS, counts(), before) if a != b_} == {fwd_path: 1}
        split = lib().hig_attn_last_split()
        assert (fwd_path, split) == planned("full_fwd", io, B, Tq, H, hd, Tk), "the call did not do what its plan named"
        if rows_per_wg:
            assert split == (Tq + rows_per_wg - 1) // rows_per_wg
        else:   # 32 query rows per wave, 2 / 4 / 8 waves (HIG_FULLATTN_WAVES; test_gpu_knobs.py): one of the three grids
            assert split in {(Tq + 32 * w - 1) // (32 * w) for w in (2, 4, 8)}
        outs.append((y.verify("y"), None if bf else lse.verify("lse")))
    assert torch.equal(outs[0][0], outs[1][0]) and (bf or torch.equal(outs[0][1], outs[1][1])), "two forward calls differ"
    y, lse = outs[0]
    report.append("fwd -> %s split %d;" % (fwd_path, split))
    b = full_bounds(r, B, Tq, Tk, H, hd)
    gy = (b["g_w"] + Tk + 2).max().item()
    inf = torch.full((), float("inf"), device=DEV, dtype=torch.float64)   # (the printed multiples leave the 2^-7-quantised rows out)
    My, Ml = torch.where(r["valid"][:, :, None, None], r["My"], inf), torch.where(r["valid"][:, None, :], 1 + r["Smax"], inf)
    held("y", y.reshape(B, Tq, H, hd), r["y"], b["y"] + (2.0 ** -8 * r["y"].abs() if bf else 0), report, *(() if bf else (My, gy)))
    if not bf:
        held("lse", lse.reshape(B, H, Tq), r["lse"], b["lse"], report, Ml, b["g_lse"])
    if backward and not bf:
        r = full_reference(q, kv, dy, B, Tq, Tk, H, hd, lg, kp, lse_in=lse, y_in=y)
        b = full_bounds(r, B, Tq, Tk, H, hd)
        outs = []
        for _ in range(2):
            dq, dk, dv = Guarded(B * Tq, d), Guarded(B * Tk, d), Guarded(B * Tk, d)
            delta = torch.zeros(B * H * Tq, device=DEV)
            y32 = y.contiguous()
            before = counts()
            _lib.check(L.hig_fullattn_bwd(P(dy), d, P(y32), d, P(q), d, P(kv), P(kv, d), 2 * d, B, Tq, Tk, H, hd, P(lg), P(lse.contiguous()),
                                          P(delta), dq.ptr(), dq.ld, dk.ptr(), dv.ptr(), dk.ld, s))
            torch.cuda.synchronize()
            assert {n: a - b_ for n, a, b_ in zip(PATHS, counts(), before) if a != b_} == {bwd_path: 1}
            assert (bwd_path, lib().hig_attn_last_split()) == planned("full_bwd", F32, B, Tq, H, hd, Tk), "the call did not do what its plan named"
            outs.append((dq.verify("dQ"), dk.verify("dK"), dv.verify("dV")))
        for a, b_ in zip(*outs):
            assert torch.equal(a, b_), "two backward calls differ"
        dq, dk, dv = outs[0]
        gb = b["g_wb"] + 2 * hd + 3 + max(Tq, Tk) + 2
        held("dQ", dq.reshape(B, Tq, H, hd), r["dQ"], b["dQ"], report, b["MdQ"], gb)
        held("dK", dk.reshape(B, Tk, H, hd), r["dK"], b["dK"], report, b["MdK"], gb)
        held("dV", dv.reshape(B, Tk, H, hd), r["dV"], b["dV"], report, b["MdV"], gb)
        assert (dq.reshape(B, Tq, d)[~r["valid"]] == 0).all(), "query rows at or beyond qlen with dy = 0: dQ = 0"
    report.append("gamma max: g_w %.0f g_lse %.0f" % (b["g_w"].max().item(), b["g_lse"]))
    print(" ".join(report))


paths_for = full_paths


FULL_TABLE = [
    # (hd, H, B, Tq, Tk, qlens): Tq / Tk on both sides of the key chunk (32), of a workgroup's query rows (256 forward, 128 for
    # the hd-128 backward, 64 on the VALU), and 1; Tq != Tk (77 text keys); qlen 0, 1, Tq - 1, Tq
    (8, 3, 2, 31, 33, None), (16, 5, 4, 65, 65, (0, 1, 64, 65)), (32, 4, 4, 129, 129, (0, 1, 128, 129)), (32, 3, 2, 64, 77, None), (32, 2, 2, 1, 1, None),
    (64, 8, 4, 196, 196, (0, 1, 195, 196)), (64, 4, 2, 1, 77, None), (64, 2, 4, 257, 257, (257, 0, 1, 256)), (64, 4, 2, 255, 31, None),
    (64, 2, 3, 256, 32, None), (64, 8, 2, 32, 33, (31, 32)), (64, 2, 1, 300, 1, None),
    (128, 4, 4, 129, 129, (0, 1, 128, 129)), (128, 2, 2, 127, 77, None), (128, 2, 4, 300, 300, (300, 299, 1, 0)), (128, 8, 1, 1, 1, None),
    (128, 2, 2, 128, 255, None), (128, 2, 2, 256, 257, None),
]


@pytest.mark.parametrize("hd,H,B,Tq,Tk,qlens", FULL_TABLE)
def test_full_attention_forward_backward(hd, H, B, Tq, Tk, qlens):
    """hig_fullattn_fwd and hig_fullattn_bwd (fed the forward's own y and lse): y, lse, dQ, dK, dV per element (full_bounds),
    rows at or beyond qlen under their 2^-7 quantisation and contributing nothing to dK / dV (their dy is 0 in the kernel's input
    and in the reference)."""
    run_full(B, Tq, Tk, H, hd, F32, *paths_for(hd), qlens=qlens, seed=Tq + Tk + hd)


@pytest.mark.parametrize("hd,H,Tq,Tk", [(32, 4, 130, 130), (64, 4, 196, 196), (128, 2, 300, 300), (64, 8, 70, 77)])
def test_full_attention_logit_spread_in_a_late_key_chunk(hd, H, Tq, Tk):
    """One 32-key chunk late in the sequence holds logits ~ 60 - 80 above all others for some query rows: everything
    accumulated before it is rescaled by e^-60 .. e^-80."""
    run_full(2, Tq, Tk, H, hd, F32, *paths_for(hd), qlens=(Tq, Tq - 1) if Tq == Tk else None, seed=3, spread80=True)


def kpad_masks(B, Tk):
    """Per sample: the first chunk all padding / whole 32-key chunks of padding in the middle / all keys but the last / all but
    the first / none.  (A sample whose keys are ALL padded is outside the contract -- include/hig.h; torch gives NaN.)"""
    m = torch.zeros(B, Tk, dtype=torch.uint8)
    m[0, :min(32, Tk - 1)] = 1
    m[1, min(10, Tk - 1):max(Tk - 10, min(10, Tk - 1))] = 1
    m[2, :Tk - 1] = 1
    m[3, 1:] = 1
    return m


@pytest.mark.parametrize("hd,H,Tq,Tk,qlens", [(32, 4, 150, 150, None), (64, 8, 196, 196, (196, 77, 1, 0, 195)), (64, 4, 91, 91, None),
                                               (128, 4, 150, 150, (150, 149, 1, 0, 75)), (128, 2, 33, 300, None), (64, 8, 300, 65, None)])
def test_full_attention_key_padding(hd, H, Tq, Tk, qlens):
    """torch's key-padding mask on the VALU kernel AND on the matrix-core forward the evaluator encoders run (head dim 64 /
    128), combined with qlen."""
    run_full(5, Tq, Tk, H, hd, F32, *paths_for(hd), qlens=qlens, kpad=kpad_masks(5, Tk), seed=11, backward=False)


@pytest.mark.parametrize("hd,H,B,Tq,Tk,qlens", [(64, 8, 2, 196, 196, (196, 77)), (64, 4, 2, 130, 77, None), (128, 2, 2, 300, 300, (211, 0)),
                                                 (128, 8, 3, 1, 77, None), (64, 2, 2, 257, 33, None)])
def test_full_attention_bf16_io(hd, H, B, Tq, Tk, qlens):
    """hig_fullattn_fwd_bf16: the fp32 matrix-core arithmetic on bf16 loads, one bf16 rounding of y (+ 2^-8 |ref|)."""
    run_full(B, Tq, Tk, H, hd, BF16, "FULL_FWD_MFMA", None, qlens=qlens, seed=Tq + hd, backward=False)
