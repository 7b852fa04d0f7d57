"""hig_linattn_apply_sty at fp32 storage, head dim 64 (apply_sty_wave64_kernel, csrc/linattn.hip): the inference forward's
attention epilogue -- softmax_hd(q) . A[b,h], LayerNorm over d, (1 + scale) / shift, SiLU -- as one kernel, against an fp64
statement of the same and against the two-kernel sequence hig_linattn_apply + hig_ln_mod_silu it replaces in the forward.
All tests need the MI355X."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hig_amd import _lib  # noqa: E402

DEV = "cuda"
HD = 64


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def make(B, T, H, ldq_mode, seed, a_scale=0.5):
    d = H * HD
    g = torch.Generator().manual_seed(seed)
    ldq = 3 * d if ldq_mode == "3d" else d
    q = (torch.randn(B * T, ldq, generator=g) * 2).to(DEV)            # queries in the first d columns of a row of ldq
    A = (torch.randn(B, H, HD, HD, generator=g) * a_scale).to(DEV)
    gamma = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(d, generator=g)).to(DEV)
    ss = (0.3 * torch.randn(B, 6 * d, generator=g)).to(DEV)           # one (scale, shift) pair inside a stacked table
    return dict(B=B, T=T, H=H, d=d, ldq=ldq, q=q, A=A, gamma=gamma, beta=beta, ss=ss)


def ss_ptr(c):
    return c["ss"].data_ptr() + 8 * c["d"]                            # the pair at columns 2 d .. 4 d


def fused(c, out=None, ldo=None, b0=0, nb=None):
    """The entry on the samples [b0, b0 + nb); `out` is a pointer or None (a fresh (B T, d) tensor is returned)."""
    B, T, H, d = c["B"], c["T"], c["H"], c["d"]
    nb = B - b0 if nb is None else nb
    ret = None
    if out is None:
        ret = torch.full((B * T, d), float("nan"), device=DEV)
        out, ldo = ret.data_ptr() + b0 * T * d * 4, d
    _lib.check(_lib.lib().hig_linattn_apply_sty(
        c["q"].data_ptr() + b0 * T * c["ldq"] * 4, c["ldq"], c["A"].data_ptr() + b0 * H * HD * HD * 4, c["gamma"].data_ptr(),
        c["beta"].data_ptr(), ss_ptr(c) + b0 * 6 * d * 4, 6 * d, d, out, ldo, nb, T, H, HD, _lib.stream_ptr()))
    return ret


def pair(c):
    B, T, H, d = c["B"], c["T"], c["H"], c["d"]
    L, s = _lib.lib(), _lib.stream_ptr()
    y = torch.empty(B * T, d, device=DEV)
    two = torch.empty(B * T, d, device=DEV)
    st = torch.empty(B * T, 2, device=DEV)
    _lib.check(L.hig_linattn_apply(c["q"].data_ptr(), c["ldq"], c["A"].data_ptr(), y.data_ptr(), d, B, T, H, HD, s))
    _lib.check(L.hig_ln_mod_silu(y.data_ptr(), d, B * T, d, c["gamma"].data_ptr(), c["beta"].data_ptr(), ss_ptr(c), 6 * d, d, T,
                                 two.data_ptr(), d, st.data_ptr(), s))
    torch.cuda.synchronize()
    return two


def ref64(c):
    """fp64 on the device: softmax -> einsum -> layer_norm -> modulation -> SiLU; also the pieces the per-element bound needs."""
    B, T, H, d = c["B"], c["T"], c["H"], c["d"]
    qd = c["q"][:, :d].double().view(B, T, H, HD)
    yd = torch.einsum("bthc,bhcl->bthl", torch.softmax(qd, -1), c["A"].double()).reshape(B * T, d)
    ln = F.layer_norm(yd, (d,), c["gamma"].double(), c["beta"].double(), 1e-5)
    sc = c["ss"][:, 2 * d:3 * d].double().repeat_interleave(T, 0)
    sh = c["ss"][:, 3 * d:4 * d].double().repeat_interleave(T, 0)
    return F.silu(ln * (1 + sc) + sh), yd, sc, sh


CASES = [(64, 196, 8, "3d"), (64, 196, 8, "d"), (32, 196, 8, "3d"), (32, 196, 8, "d"), (64, 196, 4, "3d"), (32, 196, 4, "d")]
CASES += [(3, T, H, m) for T in (1, 15, 16, 17, 91, 300) for H, m in ((8, "3d"), (4, "d"))]


@pytest.mark.parametrize("B,T,H,ldq_mode", CASES)
def test_fused_matches_fp64_and_the_two_kernel_sequence(B, T, H, ldq_mode):
    """rel-L2 < 2e-6 against fp64 and against apply + ln_mod_silu (the project's gate for this pair of kernels)."""
    c = make(B, T, H, ldq_mode, seed=B + T + H)
    out = fused(c)
    two = pair(c)
    ref = ref64(c)[0]
    e_f, e_p, e_fp = rel(out, ref), rel(two, ref), rel(out, two)
    print("B=%d T=%d H=%d ldq=%s: fused-fp64 %.3g  pair-fp64 %.3g  fused-pair %.3g" % (B, T, H, ldq_mode, e_f, e_p, e_fp))
    assert torch.isfinite(out).all()
    assert e_f < 2e-6 and e_p < 2e-6
    assert e_fp < 2e-6


@pytest.mark.parametrize("ldq_mode", ["3d", "d"])
def test_fused_error_per_element_against_the_pair(ldq_mode):
    """Element by element at the benchmarked shape: |fused - fp64| <= |pair - fp64| + 38 * 2^-24 * Mz.

    What differs between the fused kernel and the pair, from the kernels as built: the attention output y is bit-identical
    (same loads, softmax and MFMA operand order), and gamma, beta, 1 + scale, shift are NOT recombined -- the expression
    silu(((y - mean) * rstd * gamma + beta) * (1 + scale) + shift) is ln_mod_silu_kernel's.  Only the row's mean and rstd come
    from differently ordered sums.  With u = 2^-24 (one fp32 rounding), yhat = (y - mean) rstd, g = |gamma (1 + scale)|,
    S = rstd * avg_i |y_i| of the row, and the pre-activation's magnitude  Mz = g (S + |yhat|) + |beta (1 + scale)| + |shift|:
      * mean: a sum of 512 terms through a tree of depth k is off by at most k u sum|y_i|.  pair: 3 levels in the lane (two
        float4), 6 across the wave, one division: 10.  fused: 2 + 4 in the lane (four float4 added in turn), 2 across the lane
        groups, 7 across the heads, one multiplication: 16.  |d mean| rstd g <= 26 u g S.
      * rstd: sums of non-negative squares, each square carrying 3 roundings (subtract, multiply, add); the error of the mean
        enters in second order in both forms.  pair: 3 + 9 levels + division = 13; fused: 3 + (6 + 2) within the head, 8 fused
        multiply-adds between the heads, the final fma and the multiplication by 1/d = 22.  rsqrt halves the relative error of
        its argument and adds 2 u (1 ulp) in each kernel: |d rstd| / rstd <= (13 + 22) / 2 u + 4 u < 22 u, times g |yhat|.
        Both: <= 26 u g (S + |yhat|) <= 26 u Mz.
      * the unchanged operations see inputs that differ in the last bits, so their own roundings need not fall the same way as
        in the pair: subtract, two multiplies, two multiply-adds up to the pre-activation (each at most u Mz; hipcc may fuse them
        differently in the two kernels), and exp, add, divide in the SiLU (|silu(z)| <= |z|): 4 + 4 = 8 u Mz.
      * SiLU's slope is at most 1.1:  (26 + 8) * 1.1 = 37.4 -> 38 roundings of Mz.
    The count was derived from the kernel, not from what it measured (measured excess: printed below)."""
    c = make(64, 196, 8, ldq_mode, seed=7)
    d = c["d"]
    out = fused(c).double()
    two = pair(c).double()
    ref, yd, sc, sh = ref64(c)
    mean = yd.mean(1, keepdim=True)
    rstd = torch.rsqrt(yd.var(1, unbiased=False, keepdim=True) + 1e-5)
    g = (c["gamma"].double() * (1 + sc)).abs()
    mz = g * (rstd * yd.abs().mean(1, keepdim=True) + ((yd - mean) * rstd).abs()) + (c["beta"].double() * (1 + sc)).abs() + sh.abs()
    e_f, e_p = (out - ref).abs(), (two - ref).abs()
    excess = (e_f - e_p) / (2.0 ** -24 * mz)
    print("ldq=%s: max |pair - fp64| %.3g, max |fused - fp64| %.3g, max excess %.2f roundings of Mz (allowed 38), fused != pair in %.1f %% of the elements"
          % (ldq_mode, e_p.max().item(), e_f.max().item(), excess.max().item(), 100.0 * (out != two).double().mean().item()))
    assert (excess <= 38).all()


@pytest.mark.parametrize("B,T,H", [(64, 196, 8), (3, 91, 4), (2, 17, 8), (2, 1, 8)])
def test_fused_writes_every_result_element_and_nothing_else(B, T, H):
    """`out` with guard rows in front and behind and guard columns (ldo > d), all NaN: the (B T, d) result is written, the guards
    are not; a context of zeros (every row of y constant: variance 0) gives finite output."""
    G, pad = 16, 16
    for a_scale in (0.5, 0.0):
        c = make(B, T, H, "3d", seed=11 + T, a_scale=a_scale)
        d = c["d"]
        ldo = d + pad
        buf = torch.full((B * T + 2 * G, ldo), float("nan"), device=DEV)
        fused(c, out=buf.data_ptr() + G * ldo * 4, ldo=ldo)
        torch.cuda.synchronize()
        assert torch.isfinite(buf[G:G + B * T, :d]).all()
        assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + B * T:]).all() and torch.isnan(buf[:, d:]).all()
        if a_scale == 0.0:   # y == 0: LN(y) = beta
            sc = c["ss"][:, 2 * d:3 * d].repeat_interleave(T, 0)
            sh = c["ss"][:, 3 * d:4 * d].repeat_interleave(T, 0)
            assert rel(buf[G:G + B * T, :d], F.silu(c["beta"] * (1 + sc) + sh)) < 2e-6
        else:
            assert rel(buf[G:G + B * T, :d], ref64(c)[0]) < 2e-6


@pytest.mark.parametrize("B,T,H", [(64, 196, 8), (32, 196, 8), (4, 91, 4), (6, 300, 8)])
def test_fused_is_bit_repeatable_and_batch_split_invariant(B, T, H):
    """Two calls give the same bits, and the samples [0, B) in one call == two calls on the halves (the strips a sample is cut
    into depend on the batch size of the call; a row's result must not): the forward's half-batch and captured-equals-eager
    properties rest on both."""
    c = make(B, T, H, "3d", seed=5 + B)
    a = fused(c)
    b = fused(c)
    halves = torch.full_like(a, float("nan"))
    fused(c, out=halves.data_ptr(), ldo=c["d"], b0=0, nb=B // 2)
    fused(c, out=halves.data_ptr() + (B // 2) * T * c["d"] * 4, ldo=c["d"], b0=B // 2, nb=B - B // 2)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(a, halves)
