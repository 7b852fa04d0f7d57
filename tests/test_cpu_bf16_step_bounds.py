"""tests/bf16_step_bounds.py without a GPU: the stages compose to the model, an fp32 stand-in of the bf16-storage training step
stays within every stage's bound, and every composition mutant breaks one.

Composition is what allows tests/test_gpu_bf16_step_contract.py to hold the device stage by stage: that test never compares the
step with the model, only each launch with its own operands.  Here the same stage functions, chained in fp64 without any rounding,
are the oracle (oracle.denoiser_ref / oracle.interaction_ref) and torch autograd of it under the masked-MSE loss.
"""
import functools

import pytest
import torch

import bf16_step_bounds as sb
from oracle import denoiser_ref as R
from oracle import diffusion_ref as Dm
from oracle import interaction_ref as I

# (ffn_wsp16, fuse_front, ctx_mm16, edge16): what the plans choose at the shape (sb.REACH), and every form flipped
FORMS = {"default": None, "flipped": "flipped"}
CASES = tuple(sb.CASES)          # the cases of the GPU test, the 2156-row one included


@functools.lru_cache(maxsize=None)
def setup(name):
    c = sb.CASES[name]
    m = sb.build_model(c)
    return c, sb.Dims(c), sb.Params(m), sb.case_inputs(c)


def forms_of(name, which):
    c, D, _, _ = setup(name)
    _, wsp, fuse, mm16, edge = sb.REACH[name]
    if which == "flipped":
        wsp, fuse, mm16, edge = not wsp, not fuse, not mm16, not edge
    return sb.plan_forms(D, wsp, fuse, mm16, edge)


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def oracle(name, perm=None):
    """The oracle in fp64 and its autograd under the masked-MSE loss -> out, {group: gradient}, dx, dxf_proj, dxf_out.  perm: the
    samples in another order (every sum over the batch is then taken in another order), results put back."""
    c, D, P, inp = setup(name)
    p = P.oracle_dict()
    idx = torch.arange(D.B) if perm is None else perm
    x, xp, xo = (inp[k][idx].double().requires_grad_(True) for k in ("x", "xf_proj", "xf_out"))
    fwd = I.interaction_forward if c["two"] else R.denoiser_forward
    out = fwd(p, x, inp["t"][idx], inp["length"][idx], xp, xo, c["H"], c["L"])
    Dm.masked_mse(out, inp["target"][idx].double(), R.src_mask(c["T"], inp["length"][idx]).double()).backward()
    inv = torch.argsort(idx)
    return out.detach()[inv], P.grouped({n: v.grad for n, v in p.items()}), x.grad[inv], xp.grad[inv], xo.grad[inv]


def compare(name, a, b):
    """The largest relative difference (per tensor: largest |difference| over largest |value|) between two (out, grads, dx,
    dxf_proj, dxf_out); the key.bias gradients, exact zeros in the model, are held to 1e-12 of the largest gradient instead."""
    c, D, P, _ = setup(name)
    worst = max(rel(a[0].reshape(b[0].shape), b[0]), rel(a[2].reshape(b[2].shape), b[2]), rel(a[3].reshape(b[3].shape), b[3]),
                rel(a[4].reshape(b[4].shape), b[4]))
    gmax = max(v.abs().max().item() for v in b[1].values())
    d = D.d
    for k, ref in b[1].items():
        got = a[1][k]
        assert got.shape == ref.shape, k
        names = P.gnames[k[1]] if k[0] == "g" else P.lnames[k[1]][k[2]]
        if any(n.endswith(".key.bias") for n in names):           # [query; key; value] or [key; value] biases: the key rows
            r0 = d * [n.endswith(".key.bias") for n in names].index(True)
            assert got[r0:r0 + d].abs().max().item() <= 1e-12 * gmax and ref[r0:r0 + d].abs().max().item() <= 1e-12 * gmax, k
            keep = torch.ones(len(ref), dtype=torch.bool)
            keep[r0:r0 + d] = False
            got, ref = got[keep], ref[keep]
        worst = max(worst, rel(got, ref))
    return worst


@pytest.mark.parametrize("name", CASES)
def test_the_stages_compose_to_the_model(name):
    """Chain mode, fp64, no rounding: out, every parameter gradient, dx, dxf_proj and dxf_out equal the oracle and torch autograd of
    it at fp64 rounding -- gated a decade above what the oracle shows against itself with the samples in another order."""
    c, D, P, inp = setup(name)
    ref = oracle(name)
    h = D.B // 2
    perm = torch.cat([torch.arange(h - 1, -1, -1), torch.arange(D.B - 1, h - 1, -1)]) if c["two"] else torch.arange(D.B - 1, -1, -1)
    noise = compare(name, oracle(name, perm), ref)
    te = R.timestep_embedding(inp["t"], c["d"]).double()             # (the oracle takes the timestep embedding in fp32)
    w = sb.Walk(P, D, dict(inp, dout=sb.masked_mse_grad(ref[0], inp["target"], inp["length"])), forms_of(name, None), sb.EXACT, te=te).run()
    got = (w.out["out"], {k: v for k, v in w.out.items() if isinstance(k, tuple) and k[0] in ("g", "gl")}, w.out["dx"], w.out["dxf_proj"], w.out["dxf_out"])
    assert set(got[1]) == set(ref[1])
    err = compare(name, got, ref)
    print("composition %s: chain against the oracle %.2e, the oracle against itself reordered %.2e" % (name, err, noise))
    assert 1e-17 < noise < 1e-13
    assert err <= 10 * noise


@functools.lru_cache(maxsize=None)
def standin(name, which, mutant=None):
    c, D, P, inp = setup(name)
    forms = forms_of(name, which)
    clean = sb.Walk(P, D, inp, forms, sb.STANDIN)
    clean.text_context()
    clean.forward()
    inp = dict(inp, dout=sb.masked_mse_grad(clean.out["out"].reshape(D.B, D.T, D.F), inp["target"], inp["length"]))
    s = sb.Walk(P, D, inp, forms, sb.STANDIN, mutant=mutant).run()
    return inp, forms, s.out


@pytest.mark.parametrize("which", list(FORMS))
@pytest.mark.parametrize("name", CASES)
def test_the_standin_stays_within_every_bound(name, which):
    """The fp32 stand-in (bf16 roundings on) through the teacher-forced check of every stage, in the forms the plans choose at the
    case's shape and with all four flipped."""
    c, D, P, _ = setup(name)
    inp, forms, trace = standin(name, which)
    ck = sb.Walk(P, D, inp, forms, sb.REF, trace=trace).run()
    print("standin %s %s: " % (name, which) + ", ".join("%s %.3f" % (k, v[0]) for k, v in sorted(ck.worst.items())))
    assert len(ck.worst) >= 17
    assert all(v[0] <= 1.0 for v in ck.worst.values()), {k: v for k, v in ck.worst.items() if not v[0] <= 1.0}


# where each mutant shows: the two-person ones need the two-person model, the FFN one the single-launch form
MUTANT_CASE = {m: ("pairs" if m in sb.TWO_PERSON_MUTANTS else "small", "flipped" if m == "ffn_f_from_rounded_z" else "default") for m in sb.MUTANTS}


@pytest.mark.parametrize("mutant", sb.MUTANTS)
def test_every_mutant_breaks_a_bound(mutant):
    """One composition fault in the stand-in: at least one stage is beyond its bound.  The cases give it something to show on:
    distinct modulation per block, partner lengths that differ, L = 2, num_frames > T."""
    name, which = MUTANT_CASE[mutant]
    c, D, P, _ = setup(name)
    inp, forms, trace = standin(name, which, mutant)
    ck = sb.Walk(P, D, inp, forms, sb.REF, trace=trace).run()
    bad = {k: v for k, v in ck.worst.items() if not v[0] <= 1.0}
    print("mutant %s: %s" % (mutant, ", ".join("%s %.3g at %s" % (k, v[0], v[1]) for k, v in sorted(bad.items()))))
    assert bad, mutant
