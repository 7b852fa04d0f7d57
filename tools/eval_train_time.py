"""Times one training step of the evaluation classifiers at the reference evaluator's own shape (B = 32, T = 91 tokens per
person, F = 259, d = 512, H = 8, ff = 1024, L = 8, ragged lengths) on the MI355X, for both classes:

  * fused      EvalModelTrainer.train_step_fused: hig_eval_encoder_fwd_train -> hig_softmax_xent -> hig_eval_encoder_bwd ->
               hig_clip_adam on flat buffers;
  * autograd   the same kernels through torch.autograd.Function, F.cross_entropy and torch.optim.Adam (the reference's lines);
  * forward    the inference forward hig_eval_encoder_fwd at the same shape -- the only path the classifiers had before.

    python tools/eval_train_time.py [--steps 50] [--warmup 10] [--repeats 5] [--paths fused,autograd,forward] [--out FILE]

--paths fused (with --repeats 1) is the run to put under `rocprofv3 --kernel-trace --stats` for a per-kernel breakdown of the step.

Per path: device events around `--steps` back-to-back calls after `--warmup`, divided by the steps; the repeats go round the
three paths in turn, so that the paths being compared alternate; median [min .. max] over the repeats.  Also prints the
step's algorithmic FLOPs from the shapes (GEMMs and attention products; backward = twice the forward) and the rate the
fused step reaches.  One JSON line per (model, path) at the end.  Needs the GPU; there is no fallback.
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

CFG = dict(B=32, T=91, F=259, d=512, H=8, ff=1024, L=8, num_frames=196)


def forward_flops(c, cls, class_num):
    """Multiply-adds x 2 of one forward: embeddings, L layers (in_proj, QK^T, PV, out_proj, FFN), head."""
    B, T, F, d, ff, L = (c[k] for k in ("B", "T", "F", "d", "ff", "L"))
    S = cls + 2 * T
    M = B * S
    emb = 2 * B * T * F * d + 2 * B * 4 * d
    layer = M * (3 * d * d + d * d + 2 * d * ff) + 2 * B * S * S * d
    head = B * d * class_num if cls else M * d * d + 2 * B * d * d + B * d * class_num
    return 2 * (emb + L * layer + head)


def build(cls_, c, dev, **kw):
    torch.manual_seed(0)
    m = cls_(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"], num_layers=c["L"],
             num_heads=c["H"], **kw)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith("out1.") or name.startswith("out2."):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)      # un-zero the zero-initialised tensors
    return m.to(dev)


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
    ap.add_argument("--paths", default="fused,autograd,forward")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_train_time.py needs the MI355X")
    if a.steps < 50:
        raise SystemExit("--steps must be at least 50")
    dev = torch.device("cuda:0")
    c = CFG
    g = torch.Generator().manual_seed(7)
    x1, x2 = torch.randn(c["B"], c["T"], c["F"], generator=g).to(dev), torch.randn(c["B"], c["T"], c["F"], generator=g).to(dev)
    lens = torch.randint(20, c["T"] + 1, (c["B"],), generator=g)
    lens[0] = c["T"]
    lens = lens.to(dev)
    opt = types.SimpleNamespace(lr=2e-4, num_epochs=2, log_every=50, dim_pose=c["F"], model_dir="unused")
    results = []
    for kind, cls_, class_num in (("encoder", hig_amd.MotionEncoder, 26), ("consistency", hig_amd.MotionConsistencyEvalModel, 2)):
        labels = torch.randint(0, class_num, (c["B"],), generator=g).to(dev)
        fused_m, auto_m, plain_m = (build(cls_, c, dev, trainable=True).train(), build(cls_, c, dev, trainable=True).train(),
                                    build(cls_, c, dev).eval())
        fused_t, auto_t = hig_amd.EvalModelTrainer(opt, fused_m, kind=kind), hig_amd.EvalModelTrainer(opt, auto_m, kind=kind)

        def forward():
            with torch.no_grad():
                plain_m(x1, x2, length=lens)

        paths = [("fused", lambda: fused_t.train_step_fused(x1, x2, lens, labels)),
                 ("autograd", lambda: auto_t.train_step(x1, x2, lens, labels)),
                 ("forward", forward)]
        paths = [p for p in paths if p[0] in a.paths.split(",")]
        reps = {name: [] for name, _ in paths}
        for r in range(a.repeats):
            for name, fn in paths:
                reps[name].append(timed(fn, a.steps, a.warmup))
            print("# %s: round %d of %d done" % (kind, r + 1, a.repeats), flush=True)
        fwd = forward_flops(c, 0 if kind == "encoder" else 1, class_num)
        med = {name: statistics.median(v) for name, v in reps.items()}
        for name, _ in paths:
            v = reps[name]
            row = dict(model=kind, path=name, ms=dict(median=med[name], min=min(v), max=max(v)), repeats=v, steps=a.steps,
                       ratio_to_forward=med[name] / med.get("forward", float("nan")), flops=(fwd if name == "forward" else 3 * fwd))
            results.append(row)
            print("%-11s %-8s %8.3f ms [%8.3f .. %8.3f]  = %5.2f x forward   %6.1f GFLOP -> %6.1f TFLOP/s" % (
                kind, name, med[name], min(v), max(v), row["ratio_to_forward"], row["flops"] / 1e9, row["flops"] / med[name] / 1e9), flush=True)
    lines = [json.dumps(r) for r in results]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
