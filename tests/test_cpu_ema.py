"""The EMA of the weights without a GPU: tests/ema_bounds.py accepts fp32 and rejects its mutants, the weight helper gives the
values of the definition, the three entry points refuse bad arguments before any launch, and a bad option is a ValueError."""
import ctypes as C
import types

import pytest
import torch

import ema_bounds as eb
from ema_bounds import F32

ADAM = dict(lr=2e-4, b1=0.9, b2=0.999, eps=1e-8, max_norm=0.5, inv_world=1.0)


def case(n, seed):
    """(e, p, p') of n elements: parameters, an EMA that lags them a little, and the parameters one Adam step later."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    e = p + 1e-3 * torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g)
    m, v = 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g)
    p_new = eb.clip_adam_eval(p, grad, m, v, step=0, dtype=F32, **ADAM)[0]
    return e, p, p_new


@pytest.mark.parametrize("n", (3, 1027, 100003))
@pytest.mark.parametrize("warmup", (0, 1))
@pytest.mark.parametrize("step,origin", ((0, 0), (1, 0), (2, 1), (5, 3)))
def test_bound_accepts_fp32_with_and_without_fma(n, warmup, step, origin):
    e, p, p_new = case(n, n + step)
    ref, bound = eb.ema_step_bound(e, p_new, step, origin, 0.999, warmup)
    for fma in (False, True):
        out = eb.ema_step_eval(e, p, p_new, step, origin, 0.999, warmup, dtype=F32, fma=fma)
        assert eb.ratio(out, ref, bound) <= 1.0, "fma=%s" % fma
    assert torch.equal(eb.ema_step_eval(e, p, p_new, step, origin, 0.999, warmup), ref)


# where each mutant must show: (n, step, origin, warmup)
NAMED = {
    "ema_of_old_params": (1027, 0, 0, 0),
    "weight_is_decay": (1027, 0, 0, 0),
    "warmup_off_by_one": (1027, 0, 0, 1),      # first update: 1/10 instead of 2/11
    "origin_ignored": (1027, 2, 2, 1),         # first update of an EMA switched on at step 2: n = 1, not 3
    "tail_skipped": (1027, 0, 0, 0),           # 1027 & 3 = 3
}


@pytest.mark.parametrize("mutant", eb.MUTANTS)
def test_bound_rejects_every_mutant(mutant):
    n, step, origin, warmup = NAMED[mutant]
    e, p, p_new = case(n, 7)
    ref, bound = eb.ema_step_bound(e, p_new, step, origin, 0.999, warmup)
    out = eb.ema_step_eval(e, p, p_new, step, origin, 0.999, warmup, mutant=mutant)
    assert eb.ratio(out, ref, bound) > 1.0, "%s passes the bound" % mutant
    if mutant == "tail_skipped":       # ... and only through the tail
        assert eb.ratio(out[:n - 3], ref[:n - 3], bound[:n - 3]) <= 1.0


def test_recurrence_bound_is_the_sum_of_the_steps():
    e, p, p_new = case(1027, 3)
    snaps = [p_new + 1e-4 * i for i in range(5)]
    ref, bound = eb.ema_recurrence(e, snaps, 0, 0, 0.999, 1)
    out = e.clone()
    for i, s in enumerate(snaps):
        out = eb.ema_step_eval(out, s, s, i, 0, 0.999, 1, dtype=F32, fma=True)
    assert eb.ratio(out, ref, bound) <= 1.0


def test_ema_weight_values():
    assert eb.ema_weight(1, 0.9999, 1) == eb.f32(1.0 - 2.0 / 11.0)            # n = 1: d = 2 / 11
    assert eb.ema_weight(0, 0.9999, 1) == eb.ema_weight(1, 0.9999, 1) == eb.ema_weight(-3, 0.9999, 1)     # clamped to 1
    const = eb.f32(1.0 - 0.9999)
    first = next(n for n in range(89900, 90100) if eb.ema_weight(n, 0.9999, 1) == const)
    assert first == 89990                                                     # (1 + n) / (10 + n) reaches 0.9999
    assert all(eb.ema_weight(n, 0.9999, 1) == const for n in (89990, 89991, 10 ** 6, 2 ** 31 - 1))
    assert eb.ema_weight(89989, 0.9999, 1) == eb.f32(1.0 - 89990.0 / 89999.0) > const
    # the float the kernels receive is a little smaller than 0.9999: their warm-up ends 14 updates sooner
    d32 = eb.f32(0.9999)
    c32 = eb.f32(1.0 - d32)
    assert next(n for n in range(89900, 90100) if eb.ema_weight(n, d32, 1) == c32) == 89976
    for n in (1, 2, 89990, 10 ** 6):                                          # warmup = 0: the constant decay
        assert eb.ema_weight(n, 0.9999, 0) == const and eb.ema_weight(n, 0.5, 0) == 0.5
    assert eb.update_number(0, 0) == 1 and eb.update_number(5, 3) == 3 and eb.update_number(0, 4) == 1


@pytest.mark.parametrize("scale,decay", eb.DRIFT_CASES)
def test_lerp_form_drifts_less_than_the_convex_form(scale, decay):
    lerp, convex = eb.drift_experiment(scale, decay)
    print("DRIFT scale %g decay %g: lerp %.1e convex %.1e" % (scale, decay, lerp, convex))
    assert lerp < convex


EINVAL = -1


def test_entry_points_refuse_bad_arguments_on_the_host():
    """Every check runs before anything touches a device: the pointers are host memory and are never dereferenced."""
    from hig_amd import _lib
    L = _lib.lib()
    raw = (C.c_float * 256)()
    base = (C.addressof(raw) + 15) // 16 * 16                 # a 16-byte aligned run inside
    bufs = [C.c_void_p(base + 64 * i) for i in range(8)]
    p, g, m, v, scr, st, sh, ema = bufs

    def fused(ema=ema, decay=0.999, warmup=1, origin=0, n=8):
        return L.hig_clip_adam_ema(p, g, m, v, n, 2e-4, None, 0.9, 0.999, 1e-8, 0.5, 1.0, scr, st, st, None, 0, ema, decay,
                                   warmup, origin, None)

    def update(ema=ema, decay=0.999, warmup=1, origin=0, n=8, src=p):
        return L.hig_ema_update(ema, src, n, decay, warmup, None, origin, 1, None)

    bad = [dict(ema=None), dict(decay=0.0), dict(decay=1.0), dict(decay=1.5), dict(warmup=2), dict(origin=-1), dict(n=0),
           dict(n=-4)]
    for kw in bad:
        assert fused(**kw) == EINVAL, "hig_clip_adam_ema accepts %s" % kw
        assert "hig_clip_adam_ema" in _lib.last_error()
        assert update(**kw) == EINVAL, "hig_ema_update accepts %s" % kw
        assert "hig_ema_update" in _lib.last_error()
    assert fused(ema=C.c_void_p(ema.value + 4)) == EINVAL, "hig_clip_adam_ema accepts an ema that is 4 bytes off"
    assert "16-byte" in _lib.last_error()
    assert update(src=None) == EINVAL
    a, b = bufs[0], bufs[1]                                   # 64 bytes = 16 floats apart
    for kw in (dict(a=None), dict(b=None), dict(n=0), dict(n=-1), dict(n=17), dict(n=17, a=b, b=a), dict(a=a, b=a, n=1),
               dict(b=C.c_void_p(a.value + 4), n=2)):
        args = dict(a=a, b=b, n=16)
        args.update(kw)
        assert L.hig_swap_f32(args["a"], args["b"], args["n"], None) == EINVAL, "hig_swap_f32 accepts %s" % kw
        assert "hig_swap_f32" in _lib.last_error()


def test_bad_ema_decay_is_a_value_error():
    from hig_amd.trainers.ddpm_trainer import ema_options
    opt = types.SimpleNamespace
    assert ema_options(opt()) is None and ema_options(opt(ema_decay=None)) is None and ema_options(opt(ema_decay=0)) is None
    assert ema_options(opt(ema_decay=0.0)) is None
    assert ema_options(opt(ema_decay=0.9999)) == (0.9999, True)
    assert ema_options(opt(ema_decay=0.5, ema_warmup=False)) == (0.5, False)
    for d in (1, 1.0, 1.5, -0.1, "0.999", True, float("nan"), 1.0 - 1e-12):
        with pytest.raises(ValueError, match="ema_decay"):
            ema_options(opt(ema_decay=d))
