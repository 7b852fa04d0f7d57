"""Reference, bound, mutants and inputs of hig_impose_known (csrc/ddpm.hip), by the rule of tests/rowops_bounds.py.

The operation, per element i of sample b = i // per_sample, (a, b) = rows sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod
of the fp32 table at t[b]:
    mask[i] != 0:  x[i] = a known[i] + b z[i]     two products and a sum: within q_sample_bound = 2 u (|a known| + |b z|) of fp64
    mask[i] == 0:  x[i] keeps its bits            (checked on the int32 view: NaN payloads and -0.0 count)
The inputs carry NaN in known and z wherever the mask is 0 and a few NaN / -0.0 in x there, so that anything but a select shows.

Mutants (what `check` must reject): blend_instead_of_select (m val + (1 - m) x: 0 * NaN off the mask), coefficients_swapped,
t_of_sample_0_for_all, mask_shifted_by_one (mask[i - 1] decides element i).  `visible` says on which masks a mutant can show
at all: none on the empty mask, the blend and the shift not on the full one.
"""
import torch

from rowops_bounds import (F32, F64, T_SQRT_1M_AC, T_SQRT_AC, U, ddpm_table, gen, q_sample_bound,  # noqa: F401
                           q_sample_eval, ratio)

MUTANTS = ("blend_instead_of_select", "coefficients_swapped", "t_of_sample_0_for_all", "mask_shifted_by_one")
MASKS = ("zero", "one", "alternating", "bernoulli", "last_only", "run_across_boundary")
NSTEPS = 1000
PER_SAMPLE = (1, 5, 4099)           # B = 3: one element; a float4 and a tail; samples straddling float4 groups
B_SMALL = 3
WRAP_SHAPE = (3, 180001)            # sample boundaries inside a workgroup, a scalar rest
BIG_SHAPE = (1, 2200003)            # 550000 groups > 2048 x 256 threads: a second trip of the grid-stride loop
NAN = float("nan")


def make_mask(kind, B, per, seed=0):
    """(B * per,) uint8."""
    n = B * per
    m = torch.zeros(n, dtype=torch.uint8)
    if kind == "one":
        m[:] = 1
    elif kind == "alternating":
        m[::2] = 1
    elif kind == "bernoulli":            # Bernoulli(1/2) with the set bytes drawn from {1, 2, 255}: any nonzero byte means known
        g = gen(7000 + seed)
        on = torch.rand(n, generator=g) < 0.5
        vals = torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.randint(0, 3, (n,), generator=g)]
        m = torch.where(on, vals, m)
    elif kind == "last_only":
        m[n - 1] = 1
    elif kind == "run_across_boundary":  # a run of ones from the middle of a float4 across the boundary of samples 0 | 1
        edge = per if B > 1 else n // 2
        lo = max(0, edge - 6)
        lo += (2 - lo) % 4               # (the third element of its float4)
        m[lo:min(n, edge + 6)] = 1
    else:
        assert kind == "zero", kind
    return m


def impose_case(B, per, kind, seed=0):
    """x, known, z (B, per) fp32, mask (B * per,) uint8, t = (0, 1, nsteps // 2, nsteps - 1) cycled over B, the fp32 table.
    known and z are NaN wherever the mask is 0; x holds a NaN and a -0.0 there (where there is room)."""
    g = gen(3000 + seed)
    x, known, z = (torch.randn(B, per, generator=g) for _ in range(3))
    mask = make_mask(kind, B, per, seed)
    off = (mask == 0).view(B, per)
    known[off], z[off] = NAN, NAN
    idx = off.flatten().nonzero().flatten()
    if idx.numel() >= 2:
        x.view(-1)[idx[0]] = -0.0
        x.view(-1)[idx[-1]] = NAN
    base = (0, 1, NSTEPS // 2, NSTEPS - 1)
    t = torch.tensor([base[i % 4] for i in range(B)], dtype=torch.int64)
    return x, known, z, mask, t, ddpm_table(NSTEPS)


def impose_eval(x, known, z, mask, t, tab, dtype=F32, mutant=None):
    """x after the imposition, in the kernel's order (fp32: product, product, sum, nothing fused); rows are samples."""
    B, per = x.shape
    m = mask.view(B, per)
    if mutant == "mask_shifted_by_one":
        m = torch.cat([torch.zeros(1, dtype=torch.uint8), mask[:-1]]).view(B, per)
    tt = t[:1].expand(B) if mutant == "t_of_sample_0_for_all" else t
    val = q_sample_eval(known, z, tt, tab, dtype=dtype, mutant=mutant if mutant == "coefficients_swapped" else None)
    if mutant == "blend_instead_of_select":
        w = (m != 0).to(dtype)
        return (w * val + (1 - w) * x.to(dtype)).to(F32)
    return torch.where(m != 0, val.to(F32), x)


def visible(mutant, mask, t, B, per):
    """Whether the mutant changes anything on this mask."""
    on = (mask != 0).view(B, per)
    if mutant == "coefficients_swapped":
        return bool(on.any())
    if mutant == "t_of_sample_0_for_all":
        return any(bool(on[b].any()) and int(t[b]) != int(t[0]) for b in range(B))
    if mutant == "blend_instead_of_select":
        return bool((~on).any())                   # (0 * NaN off the mask)
    shifted = torch.cat([torch.zeros(1, dtype=torch.bool), on.flatten()[:-1]])
    return bool((shifted != on.flatten()).any())


def check(out, x, known, z, mask, t, tab):
    """(largest |err| / bound over the masked elements, whether every other element kept x's bits)."""
    B, per = x.shape
    on = (mask != 0).view(B, per)
    out = out.view(B, per)
    k0, z0 = torch.where(on, known, torch.zeros_like(known)), torch.where(on, z, torch.zeros_like(z))
    ref, bound = q_sample_bound(k0, z0, t, tab)
    r = ratio(out[on], ref[on], bound[on])
    same = torch.equal(out.contiguous().view(torch.int32)[~on], x.contiguous().view(torch.int32)[~on])
    return r, same


# ---- injected noise (the named sequence the goldens were recorded with) -----------------------------------------------------
class NoiseFeed:
    """Draw i of prefix p is fill.tensor_for("p.i", shape) * 10, as oracle.make_golden._NoiseFeed hands it to the reference."""

    def __init__(self, prefix, dev="cpu"):
        self.prefix, self.i, self.dev = prefix, 0, dev

    def _next(self, shape):
        from oracle import fill
        v = (fill.tensor_for("%s.%d" % (self.prefix, self.i), tuple(shape)) * 10.0).to(self.dev)
        self.i += 1
        return v

    def randn(self, *shape, device=None, **_):
        return self._next(shape)

    def randn_like(self, x, **_):
        return self._next(x.shape)


def patch_noise(randn=None, randn_like=None):
    """Replaces th.randn / th.randn_like in both diffusion modules until the returned undo() runs."""
    import types

    from hig_amd.models import gaussian_diffusion as gdm
    from hig_amd.models import spaced_diffusion as sdm
    proxy = types.SimpleNamespace(**{k: getattr(torch, k) for k in dir(torch) if not k.startswith("__")})
    if randn is not None:
        proxy.randn = randn
    if randn_like is not None:
        proxy.randn_like = randn_like
    old = gdm.th, sdm.th
    gdm.th = sdm.th = proxy

    def undo():
        gdm.th, sdm.th = old
    return undo
