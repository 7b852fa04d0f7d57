"""Times one training step of the two-person reference-size model (T = 196, F = 150, d = 512, L = 8, ff = 1024, Lt = 256) that
trains its CLIP text tower (no_clip=True; the ViT-B/32 text shape W = 512, H = 8, L = 12, N = 77, vocabulary 49408), PIT mode, at
32 pairs (128 text rows) and 120 pairs (480 text rows), captions drawn from a 43-entry table -- in one run, on the MI355X:

  * step_hip        DDPMMulTrainer.forward() + update() with clip_tower_train="hip": autograd, torch.optim.Adam, the tower on every
                    row.  The only route this configuration had before the tower joined the flat buffers: the yardstick;
  * fused_rows      train_fused_batch with clip_tower_train="flat" and opt.text_dedup = False: the fused step, the tower on every row;
  * fused_dedup     the same with caption dedup: the tower and the text head on the U_pad distinct captions;
  * captured_dedup  train_fused_batch(captured=True): the same step replayed as one graph;
  * index_rows / index_dedup   hig_clip_embed_index_build alone, 50 launches inside one replayed graph, for the undeduplicated and
                    the deduplicated token matrix;
  * host_index_rows / host_index_dedup   clip_text.EmbedIndex (numpy, on the host) for the same tokens, on the host clock, without
                    its upload.

    python tools/tower_step_time.py [--steps 50] [--warmup 10] [--repeats 5] [--pairs 32,120] [--out FILE]

Per path: device events around `--steps` back-to-back calls after `--warmup`, divided by the steps; the repeats go round the
paths in turn, so that the routes being compared alternate in one process; median [min .. max] over the repeats.  One JSON line
per (pairs, path) at the end.  Needs the GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hig_amd  # noqa: E402
from hig_amd.models import clip_text, stub_clip  # noqa: E402

TOWER = dict(W=512, H=8, L=12, N=77, vocab=49408)
CFG = dict(T=196, F=150, d=512, H=8, L=8, ff=1024, Lt=256)
WORDS = ["walk", "wave", "push", "shake", "hands", "turn", "left", "right", "slowly", "jump", "a", "person", "the", "other", "and"]


def caption_table(g):
    return [" ".join(WORDS[int(i)] for i in torch.randint(0, len(WORDS), (3 + k % 11,), generator=g)) for k in range(43)]


def make_trainer(route, pairs, dev, **opt):
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
                                 multi=True, label_path=None, cap_id=False, **opt)
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


def host_timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / steps


def index_graph(tokens, launches):
    """`launches` hig_clip_embed_index_build of `tokens` inside one graph -> a callable that replays it."""
    B, N = tokens.shape
    dix = clip_text.DeviceEmbedIndex(B, N, TOWER["vocab"], tokens.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dix.build(tokens)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(launches):
            dix.build(tokens)
    return graph.replay, dix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", default="32,120")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tower_step_time.py needs the MI355X")
    if a.steps < 50:
        raise SystemExit("--steps must be at least 50")
    dev = torch.device("cuda:0")
    results = []
    for P_ in [int(p) for p in a.pairs.split(",")]:
        c = CFG
        g = torch.Generator().manual_seed(3 + P_)
        table = caption_table(g)
        cap1 = [table[int(i)] for i in torch.randint(0, 43, (P_,), generator=g)]
        cap2 = [table[int(i)] for i in torch.randint(0, 43, (P_,), generator=g)]
        m1, m2 = torch.randn(P_, c["T"], c["F"], generator=g), torch.randn(P_, c["T"], c["F"], generator=g)
        lens = torch.randint(20, c["T"] + 1, (P_,), generator=g)
        batch = (cap1, cap2, m1.to(dev), m2.to(dev), lens, None)
        rows = cap1 + cap2 + cap2 + cap1
        trainers = {"step_hip": make_trainer("hip", P_, dev),
                    "fused_rows": make_trainer("flat", P_, dev, fused_step=True, text_dedup=False),
                    "fused_dedup": make_trainer("flat", P_, dev, fused_step=True),
                    "captured_dedup": make_trainer("flat", P_, dev, fused_step=True, fused_graph=True)}

        def autograd_step(tr=trainers["step_hip"]):
            tr.forward(batch)
            return tr.update()

        paths = [("step_hip", autograd_step),
                 ("fused_rows", lambda tr=trainers["fused_rows"]: tr.train_fused_batch(batch)),
                 ("fused_dedup", lambda tr=trainers["fused_dedup"]: tr.train_fused_batch(batch)),
                 ("captured_dedup", lambda tr=trainers["captured_dedup"]: tr.train_fused_batch(batch, captured=True))]
        tok = lambda caps: stub_clip.tokenize(caps, truncate=True)   # noqa: E731
        tb_rows, tb_dedup = clip_text.TokenBatch(rows, tok, dedup=False).to(dev), clip_text.TokenBatch(rows, tok).to(dev)
        per_graph = 50
        host = {}
        for name, tb in (("rows", tb_rows), ("dedup", tb_dedup)):
            replay, dix = index_graph(tb.tokens, per_graph)
            replay()
            torch.cuda.synchronize()
            ix = clip_text.EmbedIndex(tb.tokens_host, TOWER["vocab"])
            counts, live = dix.live()
            assert counts == (ix.n_live, ix.n_chunks, ix.n_ids) and all((live[f] == getattr(ix, f)).all() for f in ix.FIELDS)
            paths.append(("index_" + name, replay))
            host["host_index_" + name] = lambda t=tb.tokens_host: clip_text.EmbedIndex(t, TOWER["vocab"])
            print("%d pairs: %s token matrix %d x %d, index counts (live, chunks, ids) = %s" % (P_, name, tb.U_pad, tb.N, counts), flush=True)
        reps = {name: [] for name, _ in paths}
        reps.update({name: [] for name in host})
        for r in range(a.repeats):
            for name, fn in paths:
                ms = timed(fn, a.steps, a.warmup)
                reps[name].append(ms / per_graph if name.startswith("index_") else ms)
            for name, fn in host.items():
                reps[name].append(host_timed(fn, a.steps, a.warmup))
            print("# %d pairs: round %d of %d done" % (P_, r + 1, a.repeats), flush=True)
        st = trainers["step_hip"].encoder.clip_train_stats
        assert st["native_forwards"] == st["native_backwards"] > 0
        assert len(trainers["captured_dedup"].fused_state()["graphs"]) == 1
        med = {name: statistics.median(v) for name, v in reps.items()}
        for name, v in reps.items():
            results.append(dict(pairs=P_, path=name, U_pad=tb_dedup.U_pad, ms=dict(median=med[name], min=min(v), max=max(v)), repeats=v,
                                steps=a.steps))
            print("%3d pairs %-18s %9.4f ms [%9.4f .. %9.4f]" % (P_, name, med[name], min(v), max(v)), flush=True)
        print("%d pairs (U_pad %d): step_hip - fused_rows = %.2f ms, fused_rows - fused_dedup = %.2f ms, fused_dedup - captured_dedup = %.2f ms"
              % (P_, tb_dedup.U_pad, med["step_hip"] - med["fused_rows"], med["fused_rows"] - med["fused_dedup"],
                 med["fused_dedup"] - med["captured_dedup"]), flush=True)
        del trainers, paths
        torch.cuda.empty_cache()
    lines = [json.dumps(r) for r in results]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
