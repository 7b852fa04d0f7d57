"""Times what the per-timestep loss weights cost on one MI355X: the fused and the captured training step of config 2's model
(B = 64, T = 196, F = 150, d = 512, H = 8, L = 8, ff = 1024) in fp32 and in bf16 storage, in three variants:

  * plain        both options unset: hig_masked_mse, the path as it was before the options existed, in the same run;
  * min_snr      opt.loss_weighting = "min_snr": hig_masked_mse_w reading a static table;
  * min_snr_lsm  min-SNR + opt.sampler = "loss-second-moment": hig_masked_mse_w with the per-sample losses, then
                 hig_loss_history_update; t is drawn from the device sampler before every call (torch.multinomial, no host read),
                 which is part of what this variant costs and is inside the timed window.

    python tools/loss_weight_time.py [--steps 50] [--warmup 10] [--repeats 5] [--storage f32,bf16] [--out FILE]

EXPECTATION, written down before the first run.  Per step the weighted loss reads one 4 KB table (1000 floats, cache-resident
after the first wave) and multiplies once per row; loss-aware sampling adds B = 64 floats of sample_loss, B T = 12544 floats of
row means (50 KB written and read once), one workgroup more in the loss's final launch, one small launch (the history update:
1000 threads scanning 64 timesteps and 10 ring entries each, ~40 KB of history read) and the draw.  Against a step of tens of
milliseconds that is a launch floor or two -- of the order of 10 us -- well under 1 % of a step; the draw's torch launches
(multinomial, the copy of t) are host-side work of the same order.  The comparison that matters is the difference against
`plain` set beside `plain`'s own min .. max over the repeats.

The variants of one storage are three trainers over ONE model: they share the parameters, the gradient buffer and the
workspace, and each has its own options, Adam moments and captured graphs.  Models built separately differ in step time by more
than the effect looked for.

Per variant: device events around `--steps` back-to-back calls after `--warmup`, divided by the steps; the repeats go round
the variants in turn, so that the variants being compared alternate in one process; median [min .. max] over the repeats, and
each variant's median difference from `plain` of the same route.  One JSON line per (storage, route, variant) at the end.
Needs the GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hig_amd  # noqa: E402
from tools.ema_time import CFG, build, timed  # noqa: E402

VARIANTS = (("plain", {}), ("min_snr", dict(loss_weighting="min_snr", min_snr_gamma=5.0)),
            ("min_snr_lsm", dict(loss_weighting="min_snr", min_snr_gamma=5.0, sampler="loss-second-moment")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--storage", default="f32,bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_weight_time.py needs the MI355X")
    if a.steps < 50:
        raise SystemExit("--steps must be at least 50")
    dev = torch.device("cuda:0")
    c = CFG
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(c["B"], c["T"], c["F"], generator=g).to(dev)
    t_fixed = torch.randint(0, 1000, (c["B"],), generator=g).to(dev)
    lens = torch.randint(20, c["T"] + 1, (c["B"],), generator=g)
    lens[0] = c["T"]
    lens = lens.to(dev)
    xf_proj = torch.randn(c["B"], 4 * c["d"], generator=g).to(dev)
    xf_out = torch.randn(c["B"], c["N"], c["Lt"], generator=g).to(dev)
    results = []
    for storage in a.storage.split(","):
        model = build(c, storage, dev)
        trainers = {}
        for name, opt in VARIANTS:
            args = types.SimpleNamespace(device=dev, diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=c["B"], num_epochs=1,
                                         log_every=10 ** 9, save_latest=10 ** 9, save_every_e=1, is_continue=False,
                                         model_dir="unused", **opt)
            tr = trainers[name] = hig_amd.DDPMTrainer(args, model)
            if opt.get("sampler") == "loss-second-moment":
                # a warmed-up history: the refresh takes its real branch and p is not uniform
                hg = torch.Generator().manual_seed(5)
                tr.train_step_fused(x0, t_fixed, lens, xf_proj=xf_proj, xf_out=xf_out)      # (builds the device sampler)
                tr.sampler.load_state_dict({"history": torch.rand(1000, tr.sampler.history_per_term, generator=hg) + 0.1,
                                            "counts": torch.full((1000,), tr.sampler.history_per_term, dtype=torch.int32)})
        calls = []
        for route in ("fused", "captured"):
            for name, opt in VARIANTS:
                def call(tr=trainers[name], drawn="sampler" in opt, route=route):
                    t = tr.sampler.sample(c["B"], dev)[0] if drawn else t_fixed
                    (tr.train_step_captured if route == "captured" else tr.train_step_fused)(x0, t, lens, xf_proj=xf_proj, xf_out=xf_out)

                call()
                calls.append((route, name, call))
        reps = {(route, name): [] for route, name, _ in calls}
        for r in range(a.repeats):
            for route, name, fn in calls:
                reps[(route, name)].append(timed(fn, a.steps, a.warmup))
            print("# %s: round %d of %d done" % (storage, r + 1, a.repeats), flush=True)
        for route, name, _ in calls:
            vals, base = reps[(route, name)], reps[(route, "plain")]
            med, bmed = statistics.median(vals), statistics.median(base)
            row = dict(storage=storage, route=route, variant=name, ms=dict(median=med, min=min(vals), max=max(vals)), repeats=vals,
                       steps=a.steps, diff_from_plain_ms=med - bmed, diff_from_plain_pct=100.0 * (med - bmed) / bmed,
                       plain_spread_pct=100.0 * (max(base) - min(base)) / bmed)
            results.append(row)
            print("%-5s %-9s %-12s %8.3f ms [%8.3f .. %8.3f]  %+7.3f ms (%+6.2f %%) against plain, whose min .. max spans %.2f %%"
                  % (storage, route, name, med, min(vals), max(vals), row["diff_from_plain_ms"], row["diff_from_plain_pct"],
                     row["plain_spread_pct"]), flush=True)
        del calls, trainers, model
        torch.cuda.empty_cache()
    lines = [json.dumps(r) for r in results]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
