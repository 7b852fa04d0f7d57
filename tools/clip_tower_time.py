"""Times the frozen CLIP text tower at the ViT-B/32 text shape (W = 512, H = 8, L = 12, N = 77, vocabulary 49408, weights drawn
with CLIP's own standard deviations) on the MI355X, at B = 1, 32 and 64, in one run:

  * hip     hig_clip_text_fwd (csrc/cliptext.hip) behind models.clip_text.tower_forward;
  * torch   the torch-ops forward of the same module on the device (ClipTextModel.features): what a user with the `clip`
            package runs without the native route;
  * step    one DDPMTrainer.train_step_fused(clip_out=..., eot=...) of config 2's model (T = 196, F = 150, d = 512, L = 8,
            ff = 1024, Lt = 256) at the same B, fp32 and bf16 storage -- the step the tower precedes, so that its share of a
            step can be read off.

    python tools/clip_tower_time.py [--steps 50] [--warmup 10] [--repeats 5] [--batches 1,32,64] [--storage f32,bf16] [--out FILE]

Per path: device events around `--steps` back-to-back calls after `--warmup`, divided by the steps; the repeats go round the
paths in turn, so that the paths being compared alternate; median [min .. max] over the repeats.  Also prints the tower's
algorithmic FLOPs (GEMMs, and the causal half of the attention products) and the rate that is.  One JSON line per (B, path)
at the end.  Needs the GPU; there is no fallback.
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
from hig_amd.models import clip_text  # noqa: E402

TOWER = dict(W=512, H=8, L=12, N=77, vocab=49408)
CFG = dict(T=196, F=150, d=512, H=8, L=8, ff=1024, Lt=256)


def tower_flops(B):
    W, L, N = TOWER["W"], TOWER["L"], TOWER["N"]
    per_token = W * 3 * W + W * W + 2 * W * 4 * W                 # in_proj, out_proj, c_fc, c_proj
    attn = 2 * W * (N + 1) / 2                                    # q.k and p.v over the (n + 1) / 2 live keys of a mean row
    return 2 * B * N * L * (per_token + attn)


def build_tower(dev):
    m = clip_text.ClipTextModel(TOWER["W"], TOWER["L"], TOWER["H"], TOWER["N"], TOWER["vocab"])
    m.initialize_parameters(generator=torch.Generator().manual_seed(0))
    for p in m.parameters():
        p.requires_grad_(False)
    return m.to(dev)


def make_trainer(B, storage, dev):
    torch.manual_seed(0)
    c = CFG
    m = hig_amd.MotionTransformer(input_feats=c["F"], num_frames=c["T"], latent_dim=c["d"], ff_size=c["ff"], num_layers=c["L"],
                                  num_heads=c["H"], text_latent_dim=c["Lt"], storage=storage)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in m.out.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.02)      # un-zero the zero-initialised output projection
    args = types.SimpleNamespace(device=dev, diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=B, num_epochs=1,
                                 log_every=10 ** 9, save_latest=10 ** 9, save_every_e=1, is_continue=False, model_dir="unused")
    return hig_amd.DDPMTrainer(args, m.to(dev).train())


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="1,32,64")
    ap.add_argument("--storage", default="f32,bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_tower_time.py needs the MI355X")
    if a.steps < 50:
        raise SystemExit("--steps must be at least 50")
    dev = torch.device("cuda:0")
    tower = build_tower(dev)
    table = clip_text.TowerTable(tower, dev)
    pool = hig_amd.models.transformer._WorkspacePool()
    results = []
    for B in [int(b) for b in a.batches.split(",")]:
        g = torch.Generator().manual_seed(7 + B)
        tokens = torch.zeros(B, TOWER["N"], dtype=torch.int64)
        for b in range(B):                                          # SOT, ids, EOT, padding: lengths 3 .. 77
            n = 3 + (b * 37) % 75
            tokens[b, 0], tokens[b, n - 1] = 49406, 49407
            tokens[b, 1:n - 1] = torch.randint(1, 49406, (n - 2,), generator=g)
        tokens = tokens.to(dev)
        x0 = torch.randn(B, CFG["T"], CFG["F"], generator=g).to(dev)
        t = torch.randint(0, 1000, (B,), generator=g).to(dev)
        lens = torch.randint(20, CFG["T"] + 1, (B,), generator=g)
        lens[0] = CFG["T"]
        lens = lens.to(dev)
        with torch.no_grad():
            clip_out = clip_text.tower_forward(table, tokens, pool).contiguous()
            ref = tower.features(tokens).permute(1, 0, 2)
        eot = tokens.argmax(-1).contiguous()
        agree = ((clip_out.double() - ref.double()).norm() / ref.double().norm()).item()

        def hip():
            clip_text.tower_forward(table, tokens, pool)

        def torch_ops():
            with torch.no_grad():
                tower.features(tokens)

        paths = [("hip", hip), ("torch", torch_ops)]
        for storage in a.storage.split(","):
            tr = make_trainer(B, storage, dev)
            paths.append(("step_" + storage, lambda tr=tr: tr.train_step_fused(x0, t, lens, clip_out=clip_out, eot=eot)))
        reps = {name: [] for name, _ in paths}
        for r in range(a.repeats):
            for name, fn in paths:
                reps[name].append(timed(fn, a.steps, a.warmup))
            print("# B=%d: round %d of %d done" % (B, r + 1, a.repeats), flush=True)
        med = {name: statistics.median(v) for name, v in reps.items()}
        flops = tower_flops(B)
        for name, _ in paths:
            v = reps[name]
            row = dict(B=B, path=name, ms=dict(median=med[name], min=min(v), max=max(v)), repeats=v, steps=a.steps,
                       hip_vs_torch_rel=agree)
            note = ""
            if name in ("hip", "torch"):
                row["flops"] = flops
                note = "  %6.1f GFLOP -> %5.1f TFLOP/s" % (flops / 1e9, flops / med[name] / 1e9)
            else:
                row["tower_share"] = med["hip"] / (med["hip"] + med[name])
                note = "  the HIP tower is %4.1f %% of tower + step" % (100 * row["tower_share"])
            results.append(row)
            print("B=%-3d %-10s %8.3f ms [%8.3f .. %8.3f]%s" % (B, name, med[name], min(v), max(v), note), flush=True)
        del paths
        torch.cuda.empty_cache()
    lines = [json.dumps(r) for r in results]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
