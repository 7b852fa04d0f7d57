"""fp64 definition, element-wise bound, host weight helper and mutants of the EMA of the weights (csrc/ddpm.hip:
clip_adam_kernel<true>, ema_update_kernel; include/hig.h, 'EMA weights').  Plain torch on the host, the rule of
tests/rowops_bounds.py and tests/dpm_bounds.py: a result differs from its fp64 value by at most gamma u M.
tests/test_cpu_ema.py proves without a GPU that the bound accepts fp32 and rejects the mutants, tests/test_gpu_ema.py holds
the kernels and the trainer to it.

Definition.  For EMA update number n (n = 1 at the first update after the EMA was switched on, smaller values count as 1):
    d_n = decay                               warmup == 0
    d_n = min(decay, (1 + n) / (10 + n))      warmup == 1
    w   = fp32(1 - d_n)                       in fp64, rounded once
    e'  = e + w (p' - e)                      fp32 per element; p' = the parameter AFTER the step's Adam update
`ema_weight(n, decay, warmup)` evaluates the first three lines for the `decay` it is given, a double.  The kernels receive the
decay as a float, so whoever models them passes `f32(decay)`: for the option value 0.9999 the warm-up ends at n = 89990 (where
(1 + n) / (10 + n) reaches 0.9999), for the float the kernel sees (0.99989998340606689...) at n = 89976.

Bound of the blend (`ema_bound`).  w is an exact fp32 input, p' is the fp32 number the Adam part produced and is taken as exact.
    d = p' - e          u |d|
    t = w d             u |w d|, plus the difference's error scaled by w: u |w| |d|
    e' = e + t          u |e'|
    total               (2 u |w (p' - e)| + u |e'|) (1 + 2^-20) + 2^-126
A fused multiply-add (what the kernels use: fmaf(w, p' - e, e)) rounds t and the sum once, so it stays inside.  The factor
1 + 2^-20 covers the second-order terms (the last rounding is relative to the computed e', not to the reference), 2^-126 a
product flushed below the normal range.  Over a trajectory the recurrence is a contraction (e' = (1 - w) e + w p', 0 < w < 1):
an error already in e is scaled by 1 - w < 1, so after k steps the error is at most the SUM of the k per-step bounds
(`ema_recurrence`).

Mutants (`ema_step_eval(..., mutant=)`) and where each must show:
    ema_of_old_params   blends p from before the update           wherever p' != p
    weight_is_decay     e + d (p' - e)                            everywhere (d ~ 1 instead of w ~ 1e-3)
    warmup_off_by_one   n - 1 in the warm-up: 1/10 first, not 2/11   warmup == 1, before the warm-up ends
    origin_ignored      n = step + 1                              warmup == 1, ema_origin > 0, before the warm-up ends
    tail_skipped        the last n & 3 elements keep e            sizes that are no multiple of 4

Lerp against convex form (`drift_experiment`).  4096 elements, 5000 steps of about 1e-4 (normal, with a constant drift of a
quarter of that), parameters of scale 0.02 and 1.0, the EMA kept in fp32 in both forms and compared with the fp64 recurrence
over the same fp32 parameters; largest absolute error at the end.  The convex form is the one in common use,
e.mul_(d).add_(p', alpha=1 - d): d and 1 - d are each rounded to fp32 from the double option value.
    scale  decay    lerp form   convex form   convex, d + w == 1      as first measured when the form was chosen
    0.02   0.999    2.7e-7      2.4e-6        4.8e-7                  3.1e-7   3.4e-6
    0.02   0.9999   2.3e-7      9.7e-6        3.2e-7                  2.4e-7   5.9e-6
    1.0    0.999    6.8e-6      5.6e-5        4.9e-6                  3.7e-6   4.8e-5
    1.0    0.9999   4.2e-5      3.9e-4        7.7e-5                  5.5e-5   3.2e-4
(seed 0, torch CPU; the last two columns are another trajectory of the same recipe.)  The lerp form is 8 to 40 times
closer, and the third column says why: the two separately rounded weights of the convex form do not sum to 1
(fp32(0.999) + fp32(0.001) - 1 = 1.3e-8), which biases its fixed point by (d + w - 1) / (1 - d) |p| = 1.3e-5 |p| at 0.999 and
1.7e-4 |p| at 0.9999; the lerp form has one weight and no such bias, whatever w rounds to.  With weights that sum to 1
exactly the convex form rounds u |e| twice per step where the lerp form rounds u |e'| once and u |w (p' - e)| twice: within
a factor of 2, not separable from the scatter of a maximum over 4096 elements (third row).  Only the ordering of the first
two columns is asserted.  The EMA buffer is fp32 with no compensation term; the first column IS its long-run drift against
fp64, recorded as measured: it grows with |e| / sqrt(w) (u |e'| per step, about 1 / w steps of memory).
"""
import torch

from rowops_bounds import U, ratio, clip_adam_eval  # noqa: F401  (re-exported: the tests take them from here)

F64, F32 = torch.float64, torch.float32
SECOND_ORDER = 1.0 + 2.0 ** -20
TINY = 2.0 ** -126

MUTANTS = ("ema_of_old_params", "weight_is_decay", "warmup_off_by_one", "origin_ignored", "tail_skipped")
SIZES = (3, 1027, 4194307)      # tail only; one partial sweep; more than one grid-stride sweep of 2048 x 256 x 4


def f32(x):
    """The double that equals fp32(x)."""
    return float(torch.tensor(x, dtype=F32))


def update_number(step, origin):
    """n of the update that the step taken at Adam step count `step` (the count BEFORE it) makes; at least 1."""
    return max(1, step + 1 - origin)


def ema_weight(n, decay, warmup, mutant=None):
    """w = fp32(1 - d_n) as a double, for the double `decay` as it is given (the kernels' decay is f32(decay))."""
    n = max(1, int(n))
    d = float(decay)
    if warmup:
        m = n - 1 if mutant == "warmup_off_by_one" else n
        d = min(d, (1.0 + m) / (10.0 + m))
    return f32(1.0 - d)


def blend(e, p, w, dtype=F64, fma=False):
    """e + w (p - e) in `dtype`; fma: the product and the sum rounded once (fp32 only: evaluated in fp64, where the product
    of two fp32 numbers is exact, and rounded to fp32)."""
    if dtype == F64:
        e, p = e.to(F64), p.to(F64)
        return e + w * (p - e)
    e, p = e.to(F32), p.to(F32)
    d = p - e
    wt = torch.tensor(w, dtype=F32)
    if fma:
        return (wt.double() * d.double() + e.double()).to(F32)
    return e + wt * d


def ema_step_eval(e, p_old, p_new, step, origin, decay, warmup, dtype=F64, fma=False, mutant=None):
    """The EMA after the step taken at Adam step count `step`; decay as the kernel sees it (rounded to fp32 here)."""
    d32 = f32(decay)
    n = step + 1 if mutant == "origin_ignored" else update_number(step, origin)
    w = d32 if mutant == "weight_is_decay" else ema_weight(n, d32, warmup, mutant=mutant)
    out = blend(e, p_old if mutant == "ema_of_old_params" else p_new, w, dtype, fma)
    if mutant == "tail_skipped":
        k = e.numel() & 3
        if k:
            out = out.clone()
            out[-k:] = e.to(out.dtype)[-k:]
    return out


def ema_bound(e, p_new, w):
    """(fp64 reference, per-element bound) of one blend with the exact fp32 weight w."""
    ref = blend(e, p_new, w)
    t = w * (p_new.double() - e.double())
    return ref, (2 * U * t.abs() + U * ref.abs()) * SECOND_ORDER + TINY


def ema_step_bound(e, p_new, step, origin, decay, warmup):
    return ema_bound(e, p_new, ema_weight(update_number(step, origin), f32(decay), warmup))


def ema_recurrence(e0, snapshots, first_step, origin, decay, warmup):
    """(fp64 EMA, bound) after blending the parameter snapshots of steps first_step, first_step + 1, .. into e0: the fp64
    recurrence, and the sum of the per-step bounds (a contraction: errors add at most)."""
    e = e0.double()
    total = torch.zeros_like(e)
    for i, p in enumerate(snapshots):
        e, b = ema_step_bound(e, p, first_step + i, origin, decay, warmup)
        total += b
    return e, total


DRIFT_CASES = ((0.02, 0.999), (0.02, 0.9999), (1.0, 0.999), (1.0, 0.9999))


def drift_experiment(scale, decay, elems=4096, steps=5000, seed=0, complementary=False):
    """(largest error of the lerp form, of the convex form) of an fp32 EMA against the fp64 recurrence: see the module
    docstring.  complementary: the convex form with w = fp32(1 - fp32(decay)), so that d + w == 1 exactly."""
    g = torch.Generator().manual_seed(seed)
    p = (scale * torch.randn(elems, generator=g)).to(F32)
    drift = 0.25 * torch.sign(torch.randn(elems, generator=g))
    d32 = f32(decay)
    w = f32(1.0 - d32)
    dt, wt = torch.tensor(d32, dtype=F32), torch.tensor(w, dtype=F32)
    wc = wt if complementary else torch.tensor(1.0 - decay, dtype=F32)
    lerp, convex, ref = p.clone(), p.clone(), p.double()
    for _ in range(steps):
        p = p + (1e-4 * (drift + torch.randn(elems, generator=g))).to(F32)
        lerp = lerp + wt * (p - lerp)
        convex = dt * convex + wc * p
        ref = ref + w * (p.double() - ref)
    return (lerp.double() - ref).abs().max().item(), (convex.double() - ref).abs().max().item()
