"""Pins the oracle (CPU restatement) to vectors produced by the reference itself
(oracle/make_golden.py).  CPU only."""
import numpy as np
import pytest
import torch

from oracle import denoiser_ref as R
from oracle import diffusion_ref as D
from oracle import fill


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def test_g1_schedule_tables_exact(gold):
    g = gold("g1_schedule.npz")
    for n in (1000, 50):
        tb = D.tables(D.linear_betas(n))
        for name in D.TABLE_NAMES:
            assert np.array_equal(tb[name], g["n%d.%s" % (n, name)]), name
    tb = D.tables(D.linear_betas(1000))
    # known answers probed from the reference
    assert tb["betas"][0] == 1e-4 and tb["betas"][999] == 0.02
    assert abs(tb["alphas_cumprod"][999] - 4.035829765375676e-05) < 1e-18
    assert abs(tb["posterior_log_variance_clipped"][0] - (-9.81672513529567)) < 1e-12


@pytest.mark.parametrize("case", ["tiny", "config1", "width"])
@pytest.mark.parametrize("no_eff", [False, True])
def test_g2_denoiser_forward(gold, case, no_eff):
    g = gold("g2_denoiser_fwd.npz")
    c = fill.CASES[case]
    tag = "%s.%s" % (case, "full" if no_eff else "lin")
    p = fill.core_params(c["F"], c["d"], c["ff"], c["L"], c["Lt"], c["num_frames"])
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    with torch.no_grad():
        out, inter = R.denoiser_forward(p, inp["x"], inp["t"], inp["length"], inp["xf_proj"],
                                        inp["xf_out"], c["H"], c["L"], no_eff=no_eff,
                                        return_intermediates=True)
    tol = 1e-3 if no_eff else 2e-6  # the reference's own fp32 floor is 1.9e-4 for no_eff
    assert rel(out, g[tag + ".out"]) < tol
    if case != "width":
        for k in ("sa0", "ca0", "ffn0"):
            assert rel(inter[k], g[tag + "." + k]) < tol, k


def _g3_backward(case, dtype):
    c = fill.CASES[case]
    p = {k: v.to(dtype).requires_grad_(True) for k, v in
         fill.core_params(c["F"], c["d"], c["ff"], c["L"], c["Lt"], c["num_frames"]).items()}
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    x, xp, xo = (inp[k].to(dtype).clone().requires_grad_(True) for k in ("x", "xf_proj", "xf_out"))
    out = R.denoiser_forward(p, x, inp["t"], inp["length"], xp, xo, c["H"], c["L"])
    r = fill.tensor_for("loss.r." + case, out.shape).to(dtype) * 10.0
    (out * r).sum().backward()
    return p, x, xp, xo


@pytest.mark.parametrize("case", ["tiny", "config1"])
def test_g3_denoiser_backward(gold, case):
    g = gold("g3_denoiser_bwd.npz")
    tag = case + ".lin"
    p, x, xp, xo = _g3_backward(case, torch.float32)
    assert rel(x.grad, g[tag + ".dx"]) < 1e-5
    assert rel(xp.grad, g[tag + ".dxf_proj"]) < 1e-5
    assert rel(xo.grad, g[tag + ".dxf_out"]) < 1e-5
    tot = torch.sqrt(sum((v.grad.double() ** 2).sum() for v in p.values())).item()
    # key.bias grads are mathematically 0 (column softmax is shift invariant).  In fp32 both the golden value and ours are
    # rounding noise of a cancelling sum, of the size of the abs floor below, whose realisation depends on the host's
    # reduction order (thread count, vector width).  So the fp32 pass must only show them to be zero at fp32 resolution,
    # and the SAME oracle in float64 (where they come out ~1e-14 on any host) is held to the golden with the usual gate.
    p64 = None
    for k in g.files:
        if k.startswith(tag + ".g."):
            name = k[len(tag) + 3:]
            b = torch.as_tensor(g[k]).double()
            if name.endswith(".key.bias"):
                assert p[name].grad.double().norm() <= torch.finfo(torch.float32).eps * tot, k
                if p64 is None:
                    p64 = _g3_backward(case, torch.float64)[0]
                a = p64[name].grad
            else:
                a = p[name].grad.double()
            assert (a - b).norm() <= 1e-5 * b.norm() + 1e-6 * b.numel() ** 0.5, k
    assert abs(tot - float(g[tag + ".gnorm_core"])) / float(g[tag + ".gnorm_core"]) < 1e-5


def test_g4_diffusion_elementwise(gold):
    g = gold("g4_diffusion.npz")
    tb = D.tables(D.linear_betas(1000))
    x, eps, t = torch.tensor(g["x"]), torch.tensor(g["eps"]), torch.tensor(g["t"])
    z0 = fill.tensor_for("g4.z.0", x.shape) * 10.0
    z1 = fill.tensor_for("g4.z.1", x.shape) * 10.0
    assert torch.equal(D.q_sample(tb, x, t, z0), torch.tensor(g["q_sample"]))
    sample, x0, mean, logv = D.p_step(tb, x, t, eps, z1)
    assert torch.equal(x0, torch.tensor(g["pred_xstart"]))
    assert torch.equal(mean, torch.tensor(g["mean"]))
    assert torch.equal(logv, torch.tensor(g["log_variance"]))
    assert torch.equal(sample, torch.tensor(g["p_sample"]))
    assert torch.equal(sample[0], mean[0])  # t == 0: no noise
    noise = fill.tensor_for("g4.noise", x.shape) * 10
    mse = ((noise - eps) ** 2).mean(dim=(1, 2))
    assert rel(mse, g["tl_mse"]) < 1e-6


def test_g5_mini_loop(gold):
    g = gold("g5_loop.npz")
    c = fill.CASES["tiny"]
    p = fill.core_params(c["F"], c["d"], c["ff"], c["L"], c["Lt"], c["num_frames"])
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    tb = D.tables(D.linear_betas(50))
    shape = (c["B"], c["T"], c["F"])
    img = fill.tensor_for("g5.z.0", shape) * 10.0
    k = 1
    with torch.no_grad():
        for i in range(49, -1, -1):
            t = torch.full((c["B"],), i, dtype=torch.int64)
            eps = R.denoiser_forward(p, img, t, inp["length"], inp["xf_proj"], inp["xf_out"],
                                     c["H"], c["L"])
            z = fill.tensor_for("g5.z.%d" % k, shape) * 10.0
            k += 1
            img = D.p_step(tb, img, t, eps, z)[0]
    assert rel(img, g["final"]) < 1e-4


def test_properties_padding_and_permutation():
    c = fill.CASES["tiny"]
    p = fill.core_params(c["F"], c["d"], c["ff"], c["L"], c["Lt"], c["num_frames"])
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    with torch.no_grad():
        full = R.denoiser_forward(p, inp["x"], inp["t"], inp["length"], inp["xf_proj"],
                                  inp["xf_out"], c["H"], c["L"])
        # padding invariance (interaction_transformer.py:831-854 smoke): sample 1 truncated to its length
        n = c["lengths"][1]
        tr = R.denoiser_forward(p, inp["x"][1:2, :n], inp["t"][1:2], torch.tensor([n]),
                                inp["xf_proj"][1:2], inp["xf_out"][1:2], c["H"], c["L"])
        assert rel(tr, full[1:2, :n]) < 1e-5
        perm = torch.tensor([1, 0])
        pr = R.denoiser_forward(p, inp["x"][perm], inp["t"][perm], inp["length"][perm],
                                inp["xf_proj"][perm], inp["xf_out"][perm], c["H"], c["L"])
        assert rel(pr, full[perm]) < 1e-6


# ---- two-person path -----------------------------------------------------------
from oracle import interaction_ref as IR  # noqa: E402


def _iinputs(c):
    B = c["B"]
    return fill.inputs(2 * B, c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"] * 2, c["t"] * 2)


@pytest.mark.parametrize("case", ["tiny2", "config1x2"])
def test_g8_interaction_forward_backward(gold, case):
    g = gold("g8_interaction.npz")
    c = fill.ICASES[case]
    inp = _iinputs(c)
    for nca in (True, False):
        tag = case + (".nocross" if nca else "")
        p = {k: v.requires_grad_(True) for k, v in
             fill.interaction_params(c["F"], c["d"], c["ff"], c["L"], c["Lt"], c["num_frames"], no_cross_attn=nca).items()}
        x, xp, xo = (inp[k].clone().requires_grad_(True) for k in ("x", "xf_proj", "xf_out"))
        out = IR.interaction_forward(p, x, inp["t"], inp["length"], xp, xo, c["H"], c["L"], no_cross_attn=nca)
        assert rel(out, g[tag + ".out"]) < 2e-6
    r = fill.tensor_for("loss.r." + case, out.shape) * 10.0
    (out * r).sum().backward()
    assert rel(x.grad, g[case + ".dx"]) < 1e-5 and rel(xp.grad, g[case + ".dxf_proj"]) < 1e-5
    assert rel(xo.grad, g[case + ".dxf_out"]) < 1e-5
    for k in g.files:
        if k.startswith(case + ".g."):
            a, b = p[k[len(case) + 3:]].grad.double(), torch.as_tensor(g[k]).double()
            assert (a - b).norm() <= 1e-5 * b.norm() + 1e-6 * b.numel() ** 0.5, k
    tot = torch.sqrt(sum((v.grad.double() ** 2).sum() for v in p.values())).item()
    assert abs(tot - float(g[case + ".gnorm_core"])) / float(g[case + ".gnorm_core"]) < 1e-5


def test_pit_loss_symmetry():
    """PIT loss (mul_ddpm_trainer.py:234-243): swapping the caption assignment groups leaves it unchanged."""
    n, T, Fd = 8, 5, 6
    pred, tgt = fill.tensor_for("pit.pred", (n, T, Fd)), fill.tensor_for("pit.tgt", (n, T, Fd))
    mask = torch.ones(n, T)
    a = IR.pit_loss(pred, tgt, mask)
    perm = torch.tensor([2, 3, 0, 1, 6, 7, 4, 5])   # (m1|c1, m1|c2, m2|c2, m2|c1) -> swap c1 <-> c2 groups
    b = IR.pit_loss(pred[perm], tgt[perm], mask)
    assert torch.allclose(a, b)
    assert IR.pit_loss(pred, tgt, mask) <= IR.labelled_loss(pred, tgt, mask) * 2 + 1e-6


# ---- text head ---------------------------------------------------------------------
from oracle import text_head_ref as TH  # noqa: E402

TEXT_CAPTIONS = ["a person shakes hands with another person", "two people hug", "one pushes the other away and "
                 "then they both walk in a circle while waving their arms above their heads slowly", "bow"]


def text_case(case):
    """Stub-CLIP features of the golden captions + name-seeded text-head parameters."""
    import hig_amd
    from hig_amd.models import stub_clip
    c = fill.CASES[case]
    m = hig_amd.MotionTransformer(c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                  num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"], text_head="torch")
    sd = fill.fill_state_dict(m.state_dict())
    tokens, x = m._clip_features(TEXT_CAPTIONS, "cpu")
    assert tokens.argmax(-1).tolist() == [len(s.split()) + 1 for s in TEXT_CAPTIONS] and stub_clip.EOT == 49407
    p = {k: v for k, v in sd.items() if k.startswith("text")}
    return c, p, x.permute(1, 0, 2).contiguous(), tokens.argmax(-1)


@pytest.mark.parametrize("case", ["tiny", "config1"])
def test_g10_text_head_forward_backward(gold, case):
    g = gold("g10_text_head.npz")
    c, p, clip_out, eot = text_case(case)
    p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xf_proj, xf_out = TH.text_head_forward(p, clip_out, eot, 4, 4)
    assert rel(xf_proj, g[case + ".xf_proj"]) < 2e-6 and rel(xf_out, g[case + ".xf_out"]) < 2e-6
    r1 = fill.tensor_for("g10.r1." + case, xf_proj.shape) * 10.0
    r2 = fill.tensor_for("g10.r2." + case, xf_out.shape) * 10.0
    ((xf_proj * r1).sum() + (xf_out * r2).sum()).backward()
    tot = torch.sqrt(sum((v.grad.double() ** 2).sum() for v in p.values())).item()
    assert abs(tot - float(g[case + ".gnorm_text"])) < 1e-5 * tot
    for k in g.files:
        if k.startswith(case + ".g."):
            ref = torch.tensor(g[k])
            got = p[k[len(case) + 3:]].grad
            if got.shape != ref.shape:
                got = got[:64, :64]
            assert (got - ref).norm().item() < 2e-5 * ref.norm().item() + 1e-7 * tot, k
