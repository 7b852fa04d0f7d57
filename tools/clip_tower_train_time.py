"""Times TRAINING the CLIP text tower at the ViT-B/32 text shape (W = 512, H = 8, L = 12, N = 77, vocabulary 49408, weights
drawn with CLIP's own standard deviations) on the MI355X, in one run:

  * hip     hig_clip_text_fwd_train + hig_clip_text_bwd (csrc/cliptext.hip, csrc/cliptext_bwd.hip) behind
            models.clip_text.tower_forward_train / tower_backward, the embedding index built and uploaded inside the timed call;
  * torch   forward + backward of the same module on torch ops on the device (ClipTextModel.features under autograd): the only
            route `no_clip=True` training had before the native one;
  both at B = 1, 32 and 64 captions, and
  * step_hip / step_torch   one DDPMMulTrainer.forward() + update() of the two-person model (T = 196, F = 150, d = 512, L = 8,
            ff = 1024, Lt = 256, no_clip=True) at 32 pairs (PIT mode: 128 tower rows) with clip_tower_train="hip" / "torch".

    python tools/clip_tower_train_time.py [--steps 50] [--warmup 10] [--repeats 5] [--batches 1,32,64] [--pairs 32] [--out FILE]

Per path: device events around `--steps` back-to-back calls after `--warmup`, divided by the steps; the repeats go round the
paths in turn, so that the routes being compared alternate in one process; median [min .. max] over the repeats.  Also prints
what the training forward keeps at 32 and at 480 captions (hig_clip_text_train_bytes).  One JSON line per (B, path) at the end.
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
from hig_amd import _lib  # noqa: E402
from hig_amd.models import clip_text, stub_clip  # noqa: E402

TOWER = dict(W=512, H=8, L=12, N=77, vocab=49408)
CFG = dict(T=196, F=150, d=512, H=8, L=8, ff=1024, Lt=256)


def tower_flops(B):
    """Forward GEMMs and the causal half of the attention products; the backward does twice the GEMMs and 5 / 2 the attention."""
    W, L, N = TOWER["W"], TOWER["L"], TOWER["N"]
    per_token = W * 3 * W + W * W + 2 * W * 4 * W
    attn = 2 * W * (N + 1) / 2
    return 2 * B * N * L * (3 * per_token + 3.5 * attn)


def build_tower(dev):
    m = clip_text.ClipTextModel(TOWER["W"], TOWER["L"], TOWER["H"], TOWER["N"], TOWER["vocab"])
    m.initialize_parameters(generator=torch.Generator().manual_seed(0))
    return m.to(dev)


def make_tokens(B, g):
    tokens = torch.zeros(B, TOWER["N"], dtype=torch.int64)
    for b in range(B):                                          # SOT, ids, EOT, padding: lengths 3 .. 77
        n = 3 + (b * 37) % 75
        tokens[b, 0], tokens[b, n - 1] = 49406, 49407
        tokens[b, 1:n - 1] = torch.randint(1, 49406, (n - 2,), generator=g)
    return tokens


def make_trainer(route, pairs, dev):
    torch.manual_seed(0)
    c = CFG
    tower = clip_text.ClipTextModel(TOWER["W"], TOWER["L"], TOWER["H"], TOWER["N"], stub_clip.VOCAB)
    m = hig_amd.MotionInteractionTransformer(input_feats=c["F"], num_frames=c["T"], latent_dim=c["d"], ff_size=c["ff"], num_layers=c["L"],
                                             num_heads=c["H"], text_latent_dim=c["Lt"], no_clip=True, clip_model=tower,
                                             clip_tokenize=stub_clip.tokenize, clip_tower_train=route)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for mod in (m.out, m.out2):
            for p in mod.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)  # un-zero the zero-initialised output projections
    args = types.SimpleNamespace(device=dev, diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=pairs, num_epochs=1,
                                 log_every=10 ** 9, save_latest=10 ** 9, save_every_e=1, is_continue=False, model_dir="unused",
                                 multi=True, label_path=None, cap_id=False)
    tr = hig_amd.DDPMMulTrainer(args, m.to(dev).train())
    tr.opt_encoder = torch.optim.Adam(m.parameters(), lr=2e-4)
    return tr


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


def measure(paths, a, label):
    reps = {name: [] for name, _ in paths}
    for r in range(a.repeats):
        for name, fn in paths:
            reps[name].append(timed(fn, a.steps, a.warmup))
        print("# %s: round %d of %d done" % (label, r + 1, a.repeats), flush=True)
    return reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="1,32,64")
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_tower_train_time.py needs the MI355X")
    if a.steps < 50:
        raise SystemExit("--steps must be at least 50")
    dev = torch.device("cuda:0")
    for B in (32, 480):
        dims = clip_text.clip_dims(B, TOWER["N"], TOWER["W"], TOWER["H"], TOWER["L"], TOWER["vocab"])
        print("saved by the training forward at %3d captions: %d bytes (%.1f MB); backward workspace %d bytes" % (
            B, _lib.lib().hig_clip_text_train_bytes(dims), _lib.lib().hig_clip_text_train_bytes(dims) / 1e6,
            _lib.lib().hig_clip_text_bwd_workspace_bytes(dims)), flush=True)
    tower = build_tower(dev)
    table = clip_text.TrainTowerTable(tower, dev)
    pool = hig_amd.models.transformer._WorkspacePool()
    results = []
    for B in [int(b) for b in a.batches.split(",")] if a.batches else []:
        g = torch.Generator().manual_seed(7 + B)
        host_tokens = make_tokens(B, g)
        tokens = host_tokens.to(dev)
        dout = torch.randn(B, TOWER["N"], TOWER["W"], generator=g).to(dev)

        def hip():
            index = clip_text.EmbedIndex(host_tokens, TOWER["vocab"]).to(dev)
            out, saved = clip_text.tower_forward_train(table, tokens, pool)
            return out, clip_text.tower_backward(table, index, dout, saved, pool)

        def torch_ops():
            for p in tower.parameters():
                p.grad = None
            out = tower.features(tokens).permute(1, 0, 2)
            out.backward(dout)
            return out

        out, grads = hip()
        ref = torch_ops()
        agree = ((out.double() - ref.double()).norm() / ref.double().norm()).item()
        gw = tower.transformer.resblocks[0].mlp.c_fc.weight.grad
        agree_g = ((grads[4 + 8].double() - gw.double()).norm() / gw.double().norm()).item()
        paths = [("hip", hip), ("torch", torch_ops)]
        reps = measure(paths, a, "B=%d" % B)
        med = {name: statistics.median(v) for name, v in reps.items()}
        flops = tower_flops(B)
        for name, _ in paths:
            v = reps[name]
            results.append(dict(B=B, path=name, ms=dict(median=med[name], min=min(v), max=max(v)), repeats=v, steps=a.steps, flops=flops,
                                out_rel=agree, c_fc_grad_rel=agree_g))
            print("B=%-3d %-10s %8.3f ms [%8.3f .. %8.3f]  %6.1f GFLOP -> %5.1f TFLOP/s" % (B, name, med[name], min(v), max(v), flops / 1e9,
                                                                                         flops / med[name] / 1e9), flush=True)
        print("B=%-3d torch / hip = %.2f   (outputs agree to %.1e, layer 0 c_fc gradient to %.1e)" % (B, med["torch"] / med["hip"], agree, agree_g),
              flush=True)
        for p in tower.parameters():
            p.grad = None
        torch.cuda.empty_cache()
    if a.pairs > 0:
        P_, c = a.pairs, CFG
        g = torch.Generator().manual_seed(3)
        words = ["walk", "wave", "push", "shake", "hands", "turn", "left", "right", "slowly", "jump", "a", "person", "the", "other", "and"]
        pick = lambda n: " ".join(words[int(i)] for i in torch.randint(0, len(words), (n,), generator=g))   # noqa: E731
        cap1, cap2 = [pick(4 + i % 9) for i in range(P_)], [pick(3 + i % 11) for i in range(P_)]
        m1, m2 = torch.randn(P_, c["T"], c["F"], generator=g), torch.randn(P_, c["T"], c["F"], generator=g)
        lens = torch.randint(20, c["T"] + 1, (P_,), generator=g)
        batch = (cap1, cap2, m1.to(dev), m2.to(dev), lens, None)
        trainers = {r: make_trainer(r, P_, dev) for r in ("hip", "torch")}

        def step(tr):
            tr.forward(batch)
            return tr.update()

        paths = [("step_" + r, lambda tr=tr: step(tr)) for r, tr in trainers.items()]
        reps = measure(paths, a, "%d pairs" % P_)
        stats = trainers["hip"].encoder.clip_train_stats
        assert stats["native_forwards"] == stats["native_backwards"] > 0 and trainers["torch"].encoder.clip_train_stats["native_forwards"] == 0
        med = {name: statistics.median(v) for name, v in reps.items()}
        for name, _ in paths:
            v = reps[name]
            results.append(dict(pairs=P_, path=name, ms=dict(median=med[name], min=min(v), max=max(v)), repeats=v, steps=a.steps))
            print("%d pairs %-10s %8.3f ms [%8.3f .. %8.3f]" % (P_, name, med[name], min(v), max(v)), flush=True)
        print("%d pairs: step_torch / step_hip = %.2f" % (P_, med["step_torch"] / med["step_hip"]), flush=True)
    lines = [json.dumps(r) for r in results]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
