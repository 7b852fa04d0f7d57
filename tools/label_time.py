"""Times the labelling pass -- step (1-2) of the reference's recipe, `tools/label_data.py --save_label` -- for ONE batch in label
mode (4 timesteps x 41 noise draws) on the MI355X, over its three routes, in one process:

  * torch      `eval_data` under opt.label_pass = "torch": 164 `label_batch` calls, each rebuilding the class embeddings, going
               through `training_losses` (q_sample, four torch.cat copies), the model's `forward()`, the loss as torch ops and a
               `.cpu()`;
  * captured   `eval_data` under opt.label_pass = "hip": one `label_votes` call, its step (normal_, hig_q_sample_pit, the
               inference forward, hig_pair_vote) captured once and replayed 164 times, 5 transfers;
  * eager      `label_votes(captured=False)` and the same bookkeeping: the same launches without the graph.

Every timed call is the whole batch with its host work (staging, the text side, the capture, the votes' bookkeeping, the label
files).  Shapes: config 2's two-person model (T = 196, F = 150, d = 512, L = 8, ff = 1024, Lt = 256, 43 classes, cap_id: one
text token) at 32 pairs, the model batch being 128 rows; fp32 and bf16 storage.  Beside them, per call inside one replayed
hipGraph (no host gaps): the plain `_launch_forward(training=False)` at the same 128 rows, and the draw's other launches
(normal_, hig_q_sample_pit, hig_pair_vote) alone.

Expectation, written down before the first run, none of it measured.  A native draw is one inference forward at 128 rows plus
four small launches (normal_, hig_q_sample_pit, the two kernels of hig_pair_vote) that move, per element of the 64-row state,
4 B (z written) + 16 B (x0 and z read, two rows of x_t written) + 12 B (two rows of pred and z read): 32 B x 1.9 M elements =
60 MB, 15 - 25 us at HBM rate, beside a forward of several milliseconds.  So a captured draw should cost the plain forward
plus under 1 %, and the eager one the same wherever the forward's launches keep the queue full.  The torch route adds to the
same denoiser kernels, per draw: the class head as torch ops (an index, a 128 x 256 x 2048 GEMM), q_sample plus four cat copies
of 3.8 M floats, the `forward()` bookkeeping (dims, flat-parameter checks), about a dozen elementwise / reduction passes over
128 x 196 x 150 floats for the loss, and a device wait: some 30 launches and 0.3 GB of traffic, 0.3 - 0.6 ms, plus the idle time
of a queue drained 164 times.  No ratio is promised; with a forward of several milliseconds the whole surcharge may stay under
10 %.

    python tools/label_time.py [--repeats 5] [--pairs 32] [--storage f32,bf16] [--out FILE]

Per route: device events and a host clock around the batch; the repeats go round the routes in turn, so that the routes being
compared alternate; median [min .. max] over the repeats.  One JSON line per result at the end.  Needs the GPU; there is no
fallback.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hig_amd  # noqa: E402
from hig_amd import _lib  # noqa: E402
from hig_amd.trainers import mul_ddpm_trainer as MT  # noqa: E402

CFG = dict(T=196, F=150, d=512, H=8, L=8, ff=1024, Lt=256)
CLASSES = 43
DRAWS = 41


class OneBatch(torch.utils.data.Dataset):
    """`pairs` clips in the loader's cap_id item format: ([id1], [id2], motion1, motion2, length, file id)."""

    def __init__(self, pairs, seed=0):
        g = np.random.RandomState(seed)
        self.ids1 = g.randint(0, CLASSES - 1, pairs)
        self.ids2 = self.ids1 + 1
        self.m = g.standard_normal((2, pairs, CFG["T"], CFG["F"])).astype(np.float32)
        self.lens = g.randint(20, CFG["T"] + 1, pairs)
        self.lens[0] = CFG["T"]

    def __len__(self):
        return len(self.ids1)

    def __getitem__(self, i):
        return [int(self.ids1[i])], [int(self.ids2[i])], self.m[0, i], self.m[1, i], int(self.lens[i]), "clip%04d" % i


def make_trainer(pairs, storage, label_pass, dev):
    torch.manual_seed(0)
    c = CFG
    m = hig_amd.MotionInteractionTransformer(input_feats=c["F"], num_frames=c["T"], latent_dim=c["d"], ff_size=c["ff"],
                                             num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"], storage=storage,
                                             cap_id=True, class_head="hip")
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for mod in (m.out, m.out2):
            for p in mod.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)   # un-zero the zero-initialised output projections
    args = types.SimpleNamespace(device=dev, diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=pairs, num_epochs=1,
                                 log_every=10 ** 9, save_latest=10 ** 9, save_every_e=1, is_continue=False, model_dir="unused",
                                 multi=True, label_path=None, cap_id=True, label_pass=label_pass, num_workers=0)
    return hig_amd.DDPMMulTrainer(args, m.to(dev).eval())


def timed_batch(fn):
    """(device ms, host ms) of one call of fn, the device drained before and after."""
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end), (time.perf_counter() - t0) * 1e3


def timed_graph(fn, steps, warmup=3):
    """ms per call of `fn` inside ONE replayed hipGraph of `steps` calls: no host gap between the launches."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(steps):
            fn()
    graph.replay()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    graph.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--storage", default="f32,bf16")
    ap.add_argument("--graph-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("label_time.py needs the MI355X")
    dev = torch.device("cuda:0")
    B = a.pairs
    ds = OneBatch(B)
    learned = list(range(CLASSES))
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=B)))
    results = []
    save_dir = tempfile.mkdtemp(prefix="hig_label_time_")
    print("# %d pairs, %d model-batch rows, %d draws x %d timesteps" % (B, 4 * B, DRAWS, len(MT.LABEL_STEPS)), flush=True)
    for storage in a.storage.split(","):
        tr_torch, tr_hip = make_trainer(B, storage, "torch", dev), make_trainer(B, storage, "hip", dev)
        tr_hip.encoder._pool = tr_torch.encoder._pool     # one set of workspaces: the routes run in turn, never at once

        def eager():
            r = tr_hip.label_votes(batch, MT.LABEL_STEPS, draws=DRAWS, captured=False)
            active = MT.label_active_indices(learned, batch[0][0].numpy(), batch[1][0].numpy())
            for key, label in MT.file_labels_from_votes(list(batch[5]), active, r["votes"], r["first"]).items():
                with open(os.path.join(save_dir, key + '.txt'), 'w') as f:
                    f.write(str(label))

        routes = [("torch", lambda: tr_torch.eval_data(ds, 0, 1, learned, save_dir=save_dir)),
                  ("captured", lambda: tr_hip.eval_data(ds, 0, 1, learned, save_dir=save_dir)),
                  ("eager", eager)]
        for _, fn in routes:        # once unmeasured: allocations, derived operands
            fn()
        reps = {name: ([], []) for name, _ in routes}
        for r in range(a.repeats):
            for name, fn in routes:
                d, h = timed_batch(fn)
                reps[name][0].append(d)
                reps[name][1].append(h)
            print("# %s: round %d of %d done" % (storage, r + 1, a.repeats), flush=True)
        base = statistics.median(reps["torch"][1])
        ndraw = DRAWS * len(MT.LABEL_STEPS)
        for name, _ in routes:
            d, h = summary(reps[name][0]), summary(reps[name][1])
            row = dict(storage=storage, route=name, pairs=B, device_ms=d, host_ms=h, per_draw_ms=h["median"] / ndraw,
                       vs_torch=h["median"] / base, repeats_device=reps[name][0], repeats_host=reps[name][1])
            results.append(row)
            print("%-5s %-9s device %9.2f ms [%9.2f .. %9.2f]  host %9.2f ms [%9.2f .. %9.2f]  %.3f ms per draw  %.3f x torch" % (
                storage, name, d["median"], d["min"], d["max"], h["median"], h["min"], h["max"], row["per_draw_ms"],
                row["vs_torch"]), flush=True)
        # the plain forward at the same rows, and the draw's other launches, per call in a replayed graph
        core = tr_hip.encoder
        T, F = CFG["T"], CFG["F"]
        x4 = torch.randn(4 * B, T, F, device=dev)
        x2, z = torch.randn(2 * B, T, F, device=dev), torch.zeros(2 * B, T, F, device=dev)
        t4, t2 = torch.full((4 * B,), 860, dtype=torch.int64, device=dev), torch.full((2 * B,), 860, dtype=torch.int64, device=dev)
        len4 = torch.as_tensor(batch[4]).repeat(4).to(dev)
        ids = torch.cat([batch[0][0], batch[1][0], batch[1][0], batch[0][0]]).to(torch.int32).to(dev)
        xf_proj, xf_out = core._launch_class_head(ids)
        votes, first = torch.zeros(B, 2, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        assign, scratch = torch.zeros(2, B, device=dev), torch.zeros(4 * B, device=dev)
        tab, L, P = tr_hip.diffusion.device_table(dev), _lib.lib(), _lib.ptr

        def forward():
            core._launch_forward(x4, t4, len4, xf_proj, xf_out, training=False)

        def rest():
            z.normal_()
            _lib.check(L.hig_q_sample_pit(P(x2), P(z), P(t2), P(tab), 1000, B, T * F, P(x4), _lib.stream_ptr()))
            _lib.check(L.hig_pair_vote(P(x4), P(z), P(len4), 4 * B, T, F, P(votes), P(first), P(assign), P(scratch),
                                       _lib.stream_ptr()))

        for name, fn in (("forward_128_rows", forward), ("normal_+q_sample_pit+pair_vote", rest)):
            v = [timed_graph(fn, a.graph_steps) for _ in range(a.repeats)]
            s = summary(v)
            results.append(dict(storage=storage, route=name, pairs=B, ms=s, repeats=v))
            print("%-5s %-32s %9.4f ms [%9.4f .. %9.4f]  per call in a replayed graph of %d" % (
                storage, name, s["median"], s["min"], s["max"], a.graph_steps), flush=True)
        del tr_torch, tr_hip, core, routes
        torch.cuda.empty_cache()
    lines = [json.dumps(r) for r in results]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
