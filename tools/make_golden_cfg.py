"""Golden G19 (tests/golden/g19_cfg.npz): classifier-free guidance computed with the REFERENCE's GaussianDiffusion and
MotionTransformer.  The reference has no guidance of its own: the guided model is a three-line wrapper of this script, u + s (c -
u) around two calls of the reference model, the unconditional call on other text embeddings.  Stored: one guided p_sample step
and one guided ddim_sample step with a stub model and injected noise at s = 2.5, each with the reference's own distance from an
fp64 evaluation of the same formulas (`floor`); a guided K = 10 DDIM loop (eta = 0) over the reference MotionTransformer on
fill.CASES["tiny"], the same loop with the model and its inputs in fp64, and the per-sample rel-L2 distance between the two (the
loop's floor).  Runs only where the reference checkout exists; nothing of it is copied, only inputs and outputs.

    python tools/make_golden_cfg.py
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
from make_golden_few_step import ref_diffusion, rel_rows, respaced, steps64  # noqa: E402

N, K, S = 1000, 10, 2.5


def guided(model, s, uncond):
    """The wrapper: eps_u + s (eps_c - eps_u), the unconditional call with `uncond` in place of the same keywords."""
    def call(x, ts, **kw):
        c, u = model(x, ts, **kw), model(x, ts, **dict(kw, **uncond))
        return u + s * (c - u)
    return call


def main():
    mg.install_stubs()
    out = {"scale": np.float32(S)}
    use, betas = respaced(N, K)
    gd = ref_diffusion(betas)

    # ---- single steps: one batch at t = (0, 1, K // 2, K - 1), a stub model with two outputs, z injected ------------------
    shape = (4, 5, 6)
    x, ec, eu = (fill.tensor_for("g19." + n, shape) * 10 for n in ("x", "eps_c", "eps_u"))
    z = fill.tensor_for("g19.s.0", shape) * 10             # what a fresh _NoiseFeed("g19.s") hands out first
    t = torch.tensor([0, 1, K // 2, K - 1])
    out.update(x=x.numpy(), eps_c=ec.numpy(), eps_u=eu.numpy(), z=z.numpy(), t=t.numpy())
    stub = guided(lambda _x, _t, which="c": ec if which == "c" else eu, S, dict(which="u"))
    eg64 = eu.double() + float(np.float32(S)) * (ec.double() - eu.double())

    def once(fn, **kw):
        undo = mg._patch_noise(mg._NoiseFeed("g19.s"))
        try:
            return fn(stub, x, t, model_kwargs=dict(which="c"), **kw)
        finally:
            undo()

    for tag, r, eta, clip, pick in (("ddim.eta1.clip1", once(gd.ddim_sample, clip_denoised=True, eta=1.0), 1.0, True, 0),
                                    ("ddim.eta0.clip0", once(gd.ddim_sample, clip_denoised=False, eta=0.0), 0.0, False, 0),
                                    ("p_sample.clip0", once(gd.p_sample, clip_denoised=False), 0.0, False, 2)):
        ref = steps64(gd, x, eg64, z, t.numpy(), eta, clip)
        out[tag + ".sample"], out[tag + ".pred_xstart"] = r["sample"].numpy(), r["pred_xstart"].numpy()
        out[tag + ".floor"] = np.maximum(rel_rows(r["sample"].numpy(), ref[pick]), rel_rows(r["pred_xstart"].numpy(), ref[3]))

    # ---- the loop: CASES["tiny"], reference MotionTransformer seeing timestep_map[t], K = 10 of 1000, DDIM eta = 0 --------
    c = fill.CASES["tiny"]
    tmap = torch.tensor(use)
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    shape = (c["B"], c["T"], c["F"])
    un = dict(xf_proj=fill.tensor_for("g19.uncond.xf_proj", tuple(inp["xf_proj"].shape)) * 10,
              xf_out=fill.tensor_for("g19.uncond.xf_out", tuple(inp["xf_out"].shape)) * 10)
    out["uncond.xf_proj"], out["uncond.xf_out"] = un["xf_proj"].numpy(), un["xf_out"].numpy()
    x_init = fill.tensor_for("g19.x0", shape) * 10
    import models.transformer as ref_tm
    embed = ref_tm.timestep_embedding
    for tag, dt in (("loop.ddim.eta0", torch.float32), ("loop.ddim.eta0.f64", torch.float64)):
        m = mg.build_ref_model(c, False).to(dt)
        # (the sinusoidal embedding is an fp32 quantity by definition, in the reference and in the kernels: the fp64 run takes
        # the same fp32 numbers and only widens them)
        ref_tm.timestep_embedding = lambda ts, dim, _dt=dt, **k: embed(ts, dim, **k).to(_dt)
        mapped = lambda xx, ts, _m=m, **kw: _m(xx, tmap[ts], **kw)  # noqa: E731
        kw = {"xf_proj": inp["xf_proj"].to(dt), "xf_out": inp["xf_out"].to(dt), "length": inp["length"]}
        g = guided(mapped, S, {k: v.to(dt) for k, v in un.items()})
        with torch.no_grad():
            r = gd.ddim_sample_loop(g, shape, noise=x_init.clone().to(dt), clip_denoised=False, model_kwargs=kw, device="cpu",
                                    eta=0.0)
        out[tag] = r.numpy()
        assert np.isfinite(out[tag]).all(), tag
    ref_tm.timestep_embedding = embed
    out["loop.floor"] = rel_rows(out["loop.ddim.eta0"], out["loop.ddim.eta0.f64"])
    path = os.path.join(ROOT, "tests", "golden", "g19_cfg.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    for k, v in sorted(out.items()):
        if k.endswith("floor"):
            print("  %-28s %s" % (k, " ".join("%.1e" % f for f in np.atleast_1d(v))))


if __name__ == "__main__":
    main()
