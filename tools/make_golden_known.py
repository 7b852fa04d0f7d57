"""Golden G17 (tests/golden/g17_known_region.npz): what the REFERENCE computes when part of the motion is known -- single
`p_sample` steps with `pre_seq` and with `transl_req` on a strided schedule, with a stub model and injected noise, each with
the reference's own distance from an fp64 evaluation of the same formulas (`floor`), and one 10-step `p_sample_loop` with
`pre_seq` over the reference MotionTransformer.  Runs only where the reference checkout exists; nothing of it is copied, only
inputs and outputs.

    python tools/make_golden_known.py

As in G16 the reference's GaussianDiffusion is fed the respaced betas and its model is wrapped to see timestep_map[t].  The
noise is the named sequence of oracle.make_golden._NoiseFeed: draw i of prefix p is fill.tensor_for("p.i", shape) * 10, so a
test replays it from the prefix; the number of draws each call made is stored next to its outputs.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import fill  # noqa: E402
from oracle import make_golden as mg  # noqa: E402
from make_golden_few_step import N, K, ref_diffusion, rel_rows, respaced  # noqa: E402

FP = 4                                               # features fixed by pre_seq in the single step
LOOP_FP = 5                                          # ... and in the loop (F = 12)
TRANSL = [[0, 0.5, -0.25], [3, 1.0, 0.75]]           # [[feature, value at frame 0, value at frame 1], ...]
TRANSL_T = {1: (K // 2,), 2: (1, K - 1)}


def col(gd, name, t):
    return np.asarray(getattr(gd, name))[t]


def ancestral64(gd, x, eps, z, t):
    """fp64 (sample, pred_xstart) of the ancestral step from the (already imposed) x."""
    c = lambda name: col(gd, name, t)[:, None, None]  # noqa: E731
    x0 = c("sqrt_recip_alphas_cumprod") * x - c("sqrt_recipm1_alphas_cumprod") * eps
    nz = (t != 0).astype(np.float64)[:, None, None]
    return (c("posterior_mean_coef1") * x0 + c("posterior_mean_coef2") * x
            + nz * np.exp(0.5 * c("posterior_log_variance_clipped")) * z), x0


def run(gd, prefix, fn):
    feed = mg._NoiseFeed(prefix)
    undo = mg._patch_noise(feed)
    try:
        with torch.no_grad():
            return fn(), feed.i
    finally:
        undo()


def main():
    mg.install_stubs()
    use, betas = respaced(N, K)
    gd = ref_diffusion(betas)
    out = {"use_timesteps": np.array(use, dtype=np.int64), "transl_req": np.array(TRANSL, dtype=np.float64)}

    # ---- pre_seq, one step: B = 4 at t = (0, 1, K // 2, K - 1), draws = randn_like(pre_seq), randn_like(x) ---------------
    shape = (4, 5, 6)
    x, eps = fill.tensor_for("g17.x", shape) * 10, fill.tensor_for("g17.eps", shape) * 10
    pre = fill.tensor_for("g17.pre", shape[:2] + (FP,)) * 10
    zk, z = fill.tensor_for("g17.s.0", pre.shape) * 10, fill.tensor_for("g17.s.1", shape) * 10
    t = torch.tensor([0, 1, K // 2, K - 1])
    stub = lambda *_a, **_k: eps  # noqa: E731
    xin = x.clone()
    r, draws = run(gd, "g17.s", lambda: gd.p_sample(stub, xin, t, clip_denoised=False, pre_seq=pre))
    assert draws == 2
    tn = t.numpy()
    x64 = x.double().numpy().copy()
    x64[:, :, :FP] = (col(gd, "sqrt_alphas_cumprod", tn)[:, None, None] * pre.double().numpy()
                      + col(gd, "sqrt_one_minus_alphas_cumprod", tn)[:, None, None] * zk.double().numpy())
    s64, p64 = ancestral64(gd, x64, eps.double().numpy(), z.double().numpy(), tn)
    out.update({"pre.x": x.numpy(), "pre.eps": eps.numpy(), "pre.pre_seq": pre.numpy(), "pre.zk": zk.numpy(), "pre.z": z.numpy(),
                "pre.t": tn, "pre.x_after": xin.numpy(), "pre.sample": r["sample"].numpy(),
                "pre.pred_xstart": r["pred_xstart"].numpy(), "pre.draws": np.int64(draws),
                "pre.floor": np.maximum.reduce([rel_rows(xin.numpy(), x64), rel_rows(r["sample"].numpy(), s64),
                                                rel_rows(r["pred_xstart"].numpy(), p64)])})

    # ---- transl_req, one step at B = 1 and B = 2: draws = randn(2) per item, then randn_like(x) --------------------------
    for B in (1, 2):
        tag = "transl.b%d" % B
        shape = (B, 5, 6)
        x, eps = fill.tensor_for("g17.tx%d" % B, shape) * 10, fill.tensor_for("g17.te%d" % B, shape) * 10
        t = torch.tensor(TRANSL_T[B])
        stub = lambda *_a, **_k: eps  # noqa: E731
        xin = x.clone()
        r, draws = run(gd, "g17.t%d" % B, lambda: gd.p_sample(stub, xin, t, clip_denoised=False, transl_req=TRANSL))
        assert draws == len(TRANSL) + 1
        tn = t.numpy()
        x64 = x.double().numpy().copy()
        for i, item in enumerate(TRANSL):
            nz = (fill.tensor_for("g17.t%d.%d" % (B, i), (2,)) * 10).double().numpy()
            # the reference expands the (B,) coefficients to the 2 frames: frame j is noised to the level of t[j % B]
            a = np.broadcast_to(col(gd, "sqrt_alphas_cumprod", tn), (2,))
            b = np.broadcast_to(col(gd, "sqrt_one_minus_alphas_cumprod", tn), (2,))
            x64[:, :2, item[0]] = a * np.array(item[1:], dtype=np.float32).astype(np.float64) + b * nz
        z = (fill.tensor_for("g17.t%d.%d" % (B, len(TRANSL)), shape) * 10).double().numpy()
        s64, p64 = ancestral64(gd, x64, eps.double().numpy(), z, tn)
        out.update({tag + ".x": x.numpy(), tag + ".eps": eps.numpy(), tag + ".t": tn, tag + ".x_after": xin.numpy(),
                    tag + ".sample": r["sample"].numpy(), tag + ".pred_xstart": r["pred_xstart"].numpy(),
                    tag + ".draws": np.int64(draws),
                    tag + ".floor": np.maximum.reduce([rel_rows(xin.numpy(), x64), rel_rows(r["sample"].numpy(), s64),
                                                       rel_rows(r["pred_xstart"].numpy(), p64)])})

    # ---- loop: CASES["tiny"], reference MotionTransformer seeing timestep_map[t], pre_seq fixing the first features -------
    c = fill.CASES["tiny"]
    m = mg.build_ref_model(c, False)
    tmap = torch.tensor(use)
    mapped = lambda xx, ts, **kw: m(xx, tmap[ts], **kw)  # noqa: E731
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    kw = {"xf_proj": inp["xf_proj"], "xf_out": inp["xf_out"], "length": inp["length"]}
    shape = (c["B"], c["T"], c["F"])
    x_init = fill.tensor_for("g17.x0", shape) * 10
    pre = fill.tensor_for("g17.pre_loop", shape[:2] + (LOOP_FP,)) * 10
    final, draws = run(gd, "g17.p", lambda: gd.p_sample_loop(mapped, shape, noise=x_init.clone(), clip_denoised=False,
                                                            model_kwargs=kw, device="cpu", pre_seq=pre))
    assert draws == 2 * K and np.isfinite(final.numpy()).all()
    out.update({"loop.pre_seq": pre.numpy(), "loop.sample": final.numpy(), "loop.draws": np.int64(draws)})

    path = os.path.join(ROOT, "tests", "golden", "g17_known_region.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    for k, v in sorted(out.items()):
        if k.endswith(".floor"):
            print("  %-20s %s" % (k, " ".join("%.1e" % f for f in v)))


if __name__ == "__main__":
    main()
