"""Known-region conditioning without a GPU: the tensor-op `p_sample` with `pre_seq` and with `transl_req` against what the
reference computes (golden G17, tools/make_golden_known.py), the refusals, the equivalence of `pre_seq` and the (known,
known_mask) pair it stands for, and the teeth of the hig_impose_known check (tests/known_bounds.py): an fp32 evaluation in the
kernel's order passes it, every mutant lands outside on the inputs the GPU test uses."""
import pytest
import torch

import hig_amd
import known_bounds as kb
from hig_amd.models import gaussian_diffusion as gdm

N, K = 1000, 10


def spaced(k=K, n=N):
    return hig_amd.SpacedDiffusion(hig_amd.space_timesteps(n, k), betas=gdm.get_named_beta_schedule("linear", n),
                                   model_mean_type=gdm.ModelMeanType.EPSILON, model_var_type=gdm.ModelVarType.FIXED_SMALL,
                                   loss_type=gdm.LossType.MSE)


def rel_rows(a, b):
    a, b = torch.as_tensor(a).double().flatten(1), torch.as_tensor(b).double().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1)


def fed(prefix, call):
    feed = kb.NoiseFeed(prefix)
    undo = kb.patch_noise(randn=feed.randn, randn_like=feed.randn_like)
    try:
        return call(), feed.i
    finally:
        undo()


# ---- 1. the tensor-op path against the reference ------------------------------------------------------------------------------
def test_tensor_op_pre_seq_step_matches_reference_golden(gold):
    g = gold("g17_known_region.npz")
    sd = spaced()
    x, eps, pre, t = (torch.tensor(g["pre." + k]) for k in ("x", "eps", "pre_seq", "t"))
    assert t.tolist() == [0, 1, K // 2, K - 1] and tuple(x.shape) == (4, 5, 6) and tuple(pre.shape) == (4, 5, 4)
    Fp, x_in = pre.shape[2], x.clone()
    r, draws = fed("g17.s", lambda: sd.p_sample(lambda *_a, **_k: eps, x, t, clip_denoised=False, pre_seq=pre))
    assert draws == int(g["pre.draws"]) == 2              # randn_like(pre_seq), then randn_like(x)
    for key, got in (("x_after", x), ("sample", r["sample"]), ("pred_xstart", r["pred_xstart"])):
        e = rel_rows(got, g["pre." + key])
        assert (e < 1e-6).all(), (key, e.tolist())
    assert g["pre.floor"].shape == (4,) and (g["pre.floor"] < 1e-4).all()
    # x was written in place: the known features changed, the others kept their bits
    assert not torch.equal(x[:, :, :Fp], x_in[:, :, :Fp])
    assert torch.equal(x[:, :, Fp:].contiguous().view(torch.int32), x_in[:, :, Fp:].contiguous().view(torch.int32))


@pytest.mark.parametrize("B", (1, 2))
def test_tensor_op_transl_req_step_matches_reference_golden(gold, B):
    g = gold("g17_known_region.npz")
    sd = spaced()
    tag = "transl.b%d" % B
    x, eps, t = (torch.tensor(g["%s.%s" % (tag, k)]) for k in ("x", "eps", "t"))
    req = [[int(j), float(v0), float(v1)] for j, v0, v1 in g["transl_req"]]
    x_in = x.clone()
    r, draws = fed("g17.t%d" % B, lambda: sd.p_sample(lambda *_a, **_k: eps, x, t, clip_denoised=False, transl_req=req))
    assert draws == int(g[tag + ".draws"]) == len(req) + 1    # randn(2) per item, then randn_like(x)
    for key, got in (("x_after", x), ("sample", r["sample"]), ("pred_xstart", r["pred_xstart"])):
        e = rel_rows(got, g["%s.%s" % (tag, key)])
        assert (e < 1e-6).all(), (key, e.tolist())
    assert (g[tag + ".floor"] < 1e-4).all()
    touched = torch.zeros_like(x, dtype=torch.bool)
    for j, _v0, _v1 in req:
        touched[:, :2, j] = True
    assert not torch.equal(x[touched], x_in[touched])
    assert torch.equal(x[~touched].view(torch.int32), x_in[~touched].view(torch.int32))


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals():
    sd = spaced()
    stub = lambda xx, *_a, **_k: torch.zeros_like(xx)  # noqa: E731
    x3, x4 = torch.zeros(3, 5, 6), torch.zeros(4, 5, 6)
    t3, t4 = torch.tensor([0, 1, 5]), torch.tensor([0, 1, 5, 9])
    known, mask = torch.zeros(4, 5, 6), torch.ones(4, 5, 6, dtype=torch.bool)
    bad = (("transl_req at B = 3", lambda: sd.p_sample(stub, x3, t3, transl_req=[[0, 0.5, 0.25]])),
           ("pre_seq with fewer frames", lambda: sd.p_sample(stub, x4, t4, pre_seq=torch.zeros(4, 3, 4))),
           ("pre_seq wider than the sample", lambda: sd.p_sample(stub, x4, t4, pre_seq=torch.zeros(4, 5, 7))),
           ("pre_seq 2-D", lambda: sd.p_sample(stub, x4, t4, pre_seq=torch.zeros(4, 5))),
           ("known without known_mask", lambda: sd.p_sample(stub, x4, t4, known=known)),
           ("known_mask without known", lambda: sd.p_sample(stub, x4, t4, known_mask=mask)),
           ("known with pre_seq", lambda: sd.p_sample(stub, x4, t4, known=known, known_mask=mask, pre_seq=torch.zeros(4, 5, 4))),
           ("known of another shape", lambda: sd.p_sample(stub, x4, t4, known=torch.zeros(4, 5, 5), known_mask=mask)),
           ("a mask that does not broadcast", lambda: sd.p_sample(stub, x4, t4, known=known, known_mask=torch.ones(4, 3, 6, dtype=torch.bool))),
           ("a float mask", lambda: sd.p_sample(stub, x4, t4, known=known, known_mask=torch.ones(4, 5, 6))),
           ("ddim_sample, known alone", lambda: sd.ddim_sample(stub, x4, t4, known=known)),
           ("ddim loop, mask alone", lambda: sd.ddim_sample_loop(stub, (4, 5, 6), device="cpu", known_mask=mask)),
           ("p loop, transl_req at B = 3", lambda: sd.p_sample_loop(stub, (3, 5, 6), device="cpu", transl_req=[[0, 0.5, 0.25]])),
           ("p loop, known with pre_seq", lambda: sd.p_sample_loop(stub, (4, 5, 6), device="cpu", known=known, known_mask=mask,
                                                                  pre_seq=torch.zeros(4, 5, 4))))
    for what, call in bad:
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + ": accepted")
    assert not x3.any() and not x4.any()                    # nothing was written before the refusal
    # what tests pin elsewhere stays: cond_fn still raises NotImplementedError
    with pytest.raises(NotImplementedError):
        sd.p_sample(stub, x4, t4, cond_fn=lambda *a, **k: None)


# ---- 3. pre_seq is (known, known_mask) -------------------------------------------------------------------------------------
def test_pre_seq_equals_the_known_pair_built_by_hand():
    sd = spaced()
    g = torch.Generator().manual_seed(17)
    B, T, F, Fp = 4, 5, 6, 4
    x, eps, zk, z = (torch.randn(B, T, F, generator=g) for _ in range(4))
    pre = torch.randn(B, T, Fp, generator=g)
    t = torch.tensor([0, 1, K // 2, K - 1])
    known = torch.full((B, T, F), float("nan"))            # (off the mask known may hold anything)
    known[:, :, :Fp] = pre
    stub = lambda *_a, **_k: eps  # noqa: E731

    def run(**kw):
        order = [zk, z]

        def randn_like(v, **_):
            return order.pop(0)[..., :v.shape[-1]]
        xx = x.clone()
        undo = kb.patch_noise(randn_like=randn_like)
        try:
            r = sd.p_sample(stub, xx, t, clip_denoised=False, **kw)
        finally:
            undo()
        assert not order
        return xx, r

    xa, ra = run(pre_seq=pre)
    for mask in (torch.arange(F) < Fp,                                              # broadcast from (F,)
                 (torch.arange(F) < Fp).expand(B, T, F).to(torch.uint8) * 255):     # any nonzero byte means known
        xb, rb = run(known=known, known_mask=mask)
        assert torch.equal(xa, xb) and torch.isfinite(xb).all()
        assert torch.equal(ra["sample"], rb["sample"]) and torch.equal(ra["pred_xstart"], rb["pred_xstart"])
    # DDIM: the conditioned step is the imposition followed by the unconditioned step
    xc, xd = x.clone(), xa.clone()
    undo = kb.patch_noise(randn_like=lambda v, **_: zk)
    try:
        rc = sd.ddim_sample(stub, xc, t, clip_denoised=False, eta=1.0, known=known, known_mask=torch.arange(F) < Fp)
        rd = sd.ddim_sample(stub, xd, t, clip_denoised=False, eta=1.0)
    finally:
        undo()
    assert torch.equal(xc, xa) and torch.equal(rc["sample"], rd["sample"])


@pytest.mark.parametrize("loop", ("p_sample_loop", "ddim_sample_loop"))
def test_eager_loops_impose_before_every_model_call(loop):
    """What the model is shown at every step holds the known part at that step's noise level (zero noise: exactly
    sqrt(abar_t) known), and nothing of it elsewhere."""
    sd = spaced()
    B, T, F = 2, 3, 4
    known = torch.full((B, T, F), 2.0)
    mask = torch.zeros(B, T, F, dtype=torch.bool)
    mask[:, :2, :3] = True
    seen = []

    def model(xx, ts, **_):
        seen.append(xx.clone())
        return torch.zeros_like(xx)
    undo = kb.patch_noise(randn_like=lambda v, **_: torch.zeros_like(v))
    try:
        out = getattr(sd, loop)(model, (B, T, F), noise=torch.ones(B, T, F), device="cpu", clip_denoised=False, known=known,
                                known_mask=mask)
    finally:
        undo()
    assert len(seen) == K and torch.isfinite(out).all()
    for i, xx in zip(range(K - 1, -1, -1), seen):
        want = torch.tensor(sd.sqrt_alphas_cumprod[i]).float() * 2.0
        assert torch.equal(xx[mask], want.expand(int(mask.sum())))
    assert not torch.equal(seen[-1][~mask], seen[0][~mask])


# ---- 4. the check of hig_impose_known has teeth ----------------------------------------------------------------------------
SHAPES = tuple((kb.B_SMALL, per) for per in kb.PER_SAMPLE)


@pytest.mark.parametrize("kind", kb.MASKS)
@pytest.mark.parametrize("B,per", SHAPES)
def test_fp32_evaluation_passes_the_check(B, per, kind):
    x, known, z, mask, t, tab = kb.impose_case(B, per, kind, seed=per)
    assert torch.isnan(known.flatten()[mask == 0]).all() and torch.isnan(z.flatten()[mask == 0]).all()
    out = kb.impose_eval(x, known, z, mask, t, tab)
    r, same = kb.check(out, x, known, z, mask, t, tab)
    assert r <= 1.0 and same, (r, same)
    if kind == "zero":
        assert torch.equal(out.view(torch.int32), x.view(torch.int32))


@pytest.mark.parametrize("mutant", kb.MUTANTS)
def test_check_rejects_mutant(mutant):
    caught = 0
    for B, per in SHAPES:
        for kind in kb.MASKS:
            x, known, z, mask, t, tab = kb.impose_case(B, per, kind, seed=per)
            if not kb.visible(mutant, mask, t, B, per):
                continue
            r, same = kb.check(kb.impose_eval(x, known, z, mask, t, tab, mutant=mutant), x, known, z, mask, t, tab)
            assert r > 1.0 or not same, (mutant, B, per, kind, r, same)
            caught += 1
    # visible where it should be: on every mask with both kinds of bytes at per_sample 5 and 4099, at the least
    assert caught >= 2 * 3, (mutant, caught)
