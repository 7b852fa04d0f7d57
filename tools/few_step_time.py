"""Times the sampling loops at BASELINE config 3's shape (B = 32, T = 196, the config-2 model) on the MI355X: the full
1000-step chain through plain GaussianDiffusion (the path every earlier commit has) next to SpacedDiffusion's strided ancestral
and DDIM (eta = 0) loops at K = 1000 / 100 / 50 / 20, with fp32 and with bf16 storage.

    python tools/few_step_time.py [--repeats 5] [--ks 1000,100,50,20] [--out FILE] [--known | --guided]
                                  [--methods ddpm,ddim] [--spacing uniform]

--methods: which strided loops every K gets, out of ddpm, ddim (eta = 0) and dpmpp2m (DPM-Solver++(2M), dpm_solver_sample_loop);
the full 1000-step chain is timed only when ddpm is among them.  --spacing: uniform (space_timesteps), logsnr
(space_timesteps_logsnr) or both; the replay time does not depend on which steps are kept, the sample does.  With dpmpp2m and
ddim both listed, DPM lines at the end give the second-order step against DDIM at the same K and spacing, in the same run:
the difference is the history buffer's 8 bytes per element.

--known: what known-region conditioning adds to a step.  Instead of the list above, every K gets its strided ancestral and DDIM
(eta = 0) loops twice, unconditioned (the path without hig_impose_known, launch for launch the parent commit's) and with the
first half of the frames known (`known` + `known_mask`), alternating in the same run.

--guided: what classifier-free guidance costs a step.  Every K gets its strided ancestral and DDIM (eta = 0) loops three times,
alternating in the same run: guided at B (ClassifierFreeGuidedModel, scale 2.5: the stacked 2 B forward and the _cfg kernels),
unguided at B (the path without guidance, launch for launch the parent commit's) and unguided at 2 B (the same forward the
guided step runs, next to the unguided update kernels).  The summary lines at the end give guided / (2 x unguided at B) and
guided - unguided at 2 B per storage and sampler.

Per loop and repeat it reports
  * call_ms    host clock around one whole call, between device synchronisations: warm-up step, capture and K replays (text
               encoding excluded, as in bench.py) -- what a user of generate() waits for;
  * replay_ms  device events around the K replays of that call (first replay's launch to the end of the last);
  * step_us    replay_ms / K;
  * setup      (call_ms - replay_ms) / call_ms: the share spent in warm-up and capture, which a graph kept across calls
               would save.
The first call of every loop kind is reported on its own (`first`): it also pays for allocations and code loading.  The
repeats then go round all loops in turn, so the loops being compared alternate; median and min .. max over the repeats.
One JSON line per loop at the end.  Needs the GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hig_amd  # noqa: E402
from hig_amd.models import gaussian_diffusion as gdm  # noqa: E402

CFG = dict(B=32, T=196, F=150, d=512, H=8, L=8, ff=1024, N=77, Lt=256)
N = 1000


def build_model(c, device):
    torch.manual_seed(0)
    m = hig_amd.MotionTransformer(input_feats=c["F"], num_frames=c["T"], latent_dim=c["d"], ff_size=c["ff"],
                                  num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"])
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith("out.") or ".ffn.linear2." in name or ".out_layers.2." in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)      # un-zero the zero-initialised tensors
    return m.to(device).eval()


def diffusion_args():
    return dict(betas=gdm.get_named_beta_schedule("linear", N), model_mean_type=gdm.ModelMeanType.EPSILON,
                model_var_type=gdm.ModelVarType.FIXED_SMALL, loss_type=gdm.LossType.MSE)


class ReplayClock:
    """Device events around the graph replays of one call: the first replay records the start, stop() the end."""

    def __init__(self):
        self.real = torch.cuda.CUDAGraph.replay
        self.count, self.start = 0, None

    def __enter__(self):
        clock = self

        def replay(graph):
            if clock.start is None:
                clock.start = torch.cuda.Event(enable_timing=True)
                clock.start.record()
            clock.count += 1
            return clock.real(graph)

        torch.cuda.CUDAGraph.replay = replay
        return self

    def __exit__(self, *exc):
        torch.cuda.CUDAGraph.replay = self.real

    def stop(self):
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        end.synchronize()
        return self.start.elapsed_time(end) if self.start is not None else float("nan")     # (no replay at all: count says so)


def timed_call(fn, k):
    torch.cuda.synchronize()
    with ReplayClock() as clock:
        t0 = time.perf_counter()
        out = fn()
        replay_ms = clock.stop()
        call_ms = (time.perf_counter() - t0) * 1e3
    assert clock.count == k, "expected %d graph replays, saw %d: the captured path did not run" % (k, clock.count)
    assert torch.isfinite(out).all()
    return dict(call_ms=call_ms, replay_ms=replay_ms, step_us=replay_ms / k * 1e3, setup=(call_ms - replay_ms) / call_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ks", default="1000,100,50,20")
    ap.add_argument("--out", default=None)
    ap.add_argument("--known", action="store_true")
    ap.add_argument("--guided", action="store_true")
    ap.add_argument("--methods", default="ddpm,ddim")
    ap.add_argument("--spacing", default="uniform", choices=("uniform", "logsnr", "both"))
    a = ap.parse_args()
    methods = a.methods.split(",")
    if not methods or any(m not in ("ddpm", "ddim", "dpmpp2m") for m in methods):
        raise SystemExit("--methods: a comma-separated list out of ddpm, ddim, dpmpp2m")
    spacings = ("uniform", "logsnr") if a.spacing == "both" else (a.spacing,)
    if a.known and a.guided:
        raise SystemExit("--known and --guided are two different comparisons: give one of them")
    if not torch.cuda.is_available():
        raise SystemExit("few_step_time.py needs the MI355X")
    dev = torch.device("cuda:0")
    c = CFG
    model = build_model(c, dev)
    model.cache_text_context = True
    g = torch.Generator().manual_seed(1000)
    kw = {"xf_proj": torch.randn(c["B"], 4 * c["d"], generator=g).to(dev), "xf_out": torch.randn(c["B"], c["N"], c["Lt"], generator=g).to(dev),
          "length": torch.full((c["B"],), c["T"], dtype=torch.int64, device=dev)}
    shape = (c["B"], c["T"], c["F"])
    x0 = torch.randn(*shape, generator=g).to(dev)
    known = torch.randn(*shape, generator=g).to(dev)
    known_mask = torch.zeros(shape, dtype=torch.bool, device=dev)
    known_mask[:, :c["T"] // 2] = True
    un = {"xf_proj": torch.randn(c["B"], 4 * c["d"], generator=g).to(dev), "xf_out": torch.randn(c["B"], c["N"], c["Lt"], generator=g).to(dev)}
    kw2 = {k: torch.cat([v, un.get(k, v)]) for k, v in kw.items()}       # the unguided loop at 2 B: the guided forward's inputs
    shape2, x02 = (2 * c["B"],) + shape[1:], torch.cat([x0, x0])
    loops = [] if a.known or a.guided or "ddpm" not in methods else [("GaussianDiffusion ddpm", N, lambda: hig_amd.GaussianDiffusion(**diffusion_args()), "p")]
    variants = (("", ""), (" + known", "k")) if a.known else ((" guided", "g"), ("", ""), (" at 2B", "2")) if a.guided else (("", ""),)
    names = dict(ddpm=("ddpm", "p"), ddim=("ddim eta=0", "d"), dpmpp2m=("dpmpp2m", "m"))

    def kept(k, spacing):
        return hig_amd.space_timesteps(N, k) if spacing == "uniform" else hig_amd.space_timesteps_logsnr(diffusion_args()["betas"], k)

    for k in (int(v) for v in a.ks.split(",")):
        for name, kind in (names[m] for m in methods):
            for spacing in spacings:
                for tag, suffix in variants:
                    loops.append(("SpacedDiffusion %s%s%s" % (name, "" if spacing == "uniform" else " logsnr", tag), k,
                                  lambda k=k, spacing=spacing: hig_amd.SpacedDiffusion(kept(k, spacing), **diffusion_args()),
                                  kind + suffix))
    results = []
    for storage in ("f32", "bf16"):
        model.precision, model.storage = ("bf16", "bf16") if storage == "bf16" else ("f32", "f32")

        def caller(gd, kind):
            cond = dict(known=known, known_mask=known_mask) if kind.endswith("k") else {}
            mdl = hig_amd.ClassifierFreeGuidedModel(model, 2.5, un) if kind.endswith("g") else model
            sh, start, mk = (shape2, x02, kw2) if kind.endswith("2") else (shape, x0, kw)
            if kind[0] == "p":
                return lambda: gd.p_sample_loop(mdl, sh, noise=start, clip_denoised=False, model_kwargs=mk, **cond)
            if kind[0] == "m":
                return lambda: gd.dpm_solver_sample_loop(mdl, sh, noise=start, clip_denoised=False, model_kwargs=mk, **cond)
            return lambda: gd.ddim_sample_loop(mdl, sh, noise=start, clip_denoised=False, model_kwargs=mk, eta=0.0, **cond)

        calls = [(name, k, caller(make(), kind)) for name, k, make, kind in loops]
        firsts = [timed_call(call, k) for _, k, call in calls]
        # the repeats go round all loops, so that the loops being compared alternate and host drift falls on all alike
        reps = [[] for _ in calls]
        for r in range(a.repeats):
            for i, (_, k, call) in enumerate(calls):
                reps[i].append(timed_call(call, k))
            print("# %s storage: round %d of %d done" % (storage, r + 1, a.repeats), flush=True)
        for (name, k, _), first, rep in zip(calls, firsts, reps):
            row = dict(storage=storage, loop=name, K=k, first=first, repeats=rep)
            for key in ("call_ms", "replay_ms", "step_us", "setup"):
                vals = [r[key] for r in rep]
                row[key] = dict(median=statistics.median(vals), min=min(vals), max=max(vals))
            results.append(row)
            print("%-5s %-34s K=%-4d first call %8.1f ms (setup %4.1f %%) | call %8.1f ms [%8.1f .. %8.1f]  step %7.1f us "
                  "[%7.1f .. %7.1f]  setup %4.1f %% [%4.1f .. %4.1f]" % (
                      storage, name, k, first["call_ms"], 100 * first["setup"], row["call_ms"]["median"], row["call_ms"]["min"],
                      row["call_ms"]["max"], row["step_us"]["median"], row["step_us"]["min"], row["step_us"]["max"],
                      100 * row["setup"]["median"], 100 * row["setup"]["min"], 100 * row["setup"]["max"]), flush=True)
    if a.guided:
        by = {(r["storage"], r["loop"], r["K"]): r["step_us"] for r in results}
        for (storage, loop, k), g_us in by.items():
            if not loop.endswith(" guided"):
                continue
            base = loop[:-len(" guided")]
            b_us, b2_us = by[(storage, base, k)], by[(storage, base + " at 2B", k)]
            print("GUIDED %-5s %-26s K=%-4d guided %7.1f us  unguided at B %7.1f us [%7.1f .. %7.1f]  at 2B %7.1f us  "
                  "guided / (2 x at B) %.3f  guided - at 2B %+6.1f us" % (
                      storage, base, k, g_us["median"], b_us["median"], b_us["min"], b_us["max"], b2_us["median"],
                      g_us["median"] / (2 * b_us["median"]), g_us["median"] - b2_us["median"]), flush=True)
    if "dpmpp2m" in methods and "ddim" in methods:
        by = {(r["storage"], r["loop"], r["K"]): r for r in results}
        for (storage, loop, k), row in by.items():
            if not loop.startswith("SpacedDiffusion dpmpp2m"):
                continue
            base = by[(storage, loop.replace("dpmpp2m", "ddim eta=0"), k)]
            m_us, d_us = row["step_us"], base["step_us"]
            print("DPM %-5s %-40s K=%-4d step %7.1f us [%7.1f .. %7.1f]  ddim %7.1f us [%7.1f .. %7.1f]  difference %+6.1f us  | "
                  "call %7.1f ms [%7.1f .. %7.1f]  ddim %7.1f ms" % (
                      storage, loop, k, m_us["median"], m_us["min"], m_us["max"], d_us["median"], d_us["min"], d_us["max"],
                      m_us["median"] - d_us["median"], row["call_ms"]["median"], row["call_ms"]["min"], row["call_ms"]["max"],
                      base["call_ms"]["median"]), flush=True)
    lines = [json.dumps(r) for r in results]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
