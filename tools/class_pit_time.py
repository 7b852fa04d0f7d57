"""Times the PIT step of a class-id (cap_id) model on the MI355X -- step (1-1) of the reference's recipe, `tools/train.py --multi
--cap_id` without a label file -- over its three routes, in one process:

  * autograd   `forward(batch)` + `update()`: the reference's sequence through autograd and torch.optim.Adam, the only route a
               cap_id model had before the class head went into the flat buffer (class_head="torch");
  * fused      `train_fused_batch(batch)` with class_head="hip": hig_class_head_fwd, the denoiser, hig_pair_mse, the backward,
               hig_class_head_bwd, one clip + Adam pass over the flat buffers;
  * captured   `train_fused_batch(batch, captured=True)`: the same step replayed as one hipGraph.

Every timed call includes its host work (batch staging, the sampler's t, the id conversion, `.item()` of the autograd route's
log).  Shapes: config 2's model (T = 196, F = 150, d = 512, L = 8, ff = 1024, Lt = 256, 43 classes) at 32 and 160 pairs, the
model batch being the 4 rows per pair c1, c2, c2, c1; fp32 and bf16 storage.  Also, per call inside ONE replayed hipGraph of
`--steps` calls (no host gaps): the two class-head calls as the step makes them, and the two sums by key alone.

Expectation, written down before the first run, none of it measured.  The class head is 3 launches forward (one 43 x E x Lt
GEMM and two row gathers writing rows x (Lt + E) floats: 5.9 MB at 640 rows) and 5 backward (two sums by key reading the same
5.9 MB once, a column sum and two 43-row GEMMs): some 10 - 30 us per step, nothing beside a step of 50 - 250 ms.  All three
routes launch the same denoiser kernels, so the routes differ by what surrounds them: the autograd route adds the loss as
torch ops over (4 B, T, F) (about ten passes over 19 M elements at 160 pairs), a clone of every gradient view (81 M floats),
clip_grad_norm_ and Adam as multi-tensor launches over some 400 tensors (4 arrays of 81 M floats read and written), and a host
read of the loss per step; a few hundred extra launches and 3 - 4 GB of traffic, 3 - 8 ms.  So fused and captured should come out
within 1 % of each other and 1 - 4 % under the autograd route at 160 pairs in fp32, more at 32 pairs and with bf16 storage,
where the same surcharge stands beside a shorter step and the autograd route re-casts the bf16 shadow after torch's Adam.

    python tools/class_pit_time.py [--steps 50] [--warmup 10] [--repeats 5] [--cases pit32,pit160] [--storage f32,bf16] [--out FILE]

Per route: device events around `--steps` back-to-back calls after `--warmup`, divided by the steps; the repeats go round the
routes in turn, so that the routes being compared alternate; median [min .. max] over the repeats.  One JSON line per result
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
from hig_amd import _lib  # noqa: E402

CFG = dict(T=196, F=150, d=512, H=8, L=8, ff=1024, Lt=256)
CASES = {"pit32": 32, "pit160": 160}
CLASSES = 43


def make_trainer(B, storage, class_head, dev):
    torch.manual_seed(0)
    c = CFG
    m = hig_amd.MotionInteractionTransformer(input_feats=c["F"], num_frames=c["T"], latent_dim=c["d"], ff_size=c["ff"],
                                             num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"], storage=storage,
                                             cap_id=True, class_head=class_head)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for mod in (m.out, m.out2):
            for p in mod.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)   # un-zero the zero-initialised output projections
    args = types.SimpleNamespace(device=dev, diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=B, num_epochs=1,
                                 log_every=10 ** 9, save_latest=10 ** 9, save_every_e=1, is_continue=False, model_dir="unused",
                                 multi=True, label_path=None, cap_id=True)
    tr = hig_amd.DDPMMulTrainer(args, m.to(dev).train())
    tr.opt_encoder = torch.optim.Adam(tr.encoder.parameters(), lr=args.lr)
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


def timed_graph(fn, steps, warmup):
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default="pit32,pit160")
    ap.add_argument("--storage", default="f32,bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("class_pit_time.py needs the MI355X")
    dev = torch.device("cuda:0")
    results = []

    def report(row, note=""):
        results.append(row)
        ms = row["ms"]
        print("%-7s %-5s %-22s %9.4f ms [%9.4f .. %9.4f]%s" % (row["case"], row.get("storage", ""), row["route"], ms["median"],
                                                              ms["min"], ms["max"], note), flush=True)

    for case in a.cases.split(","):
        B = CASES[case]
        rows = 4 * B
        g = torch.Generator().manual_seed(7 + B)
        # 16 batches of class ids the steps cycle through; the motions stay on the device, as a device-resident loader hands them
        batches = []
        motion1 = torch.randn(B, CFG["T"], CFG["F"], generator=g).to(dev)
        motion2 = torch.randn(B, CFG["T"], CFG["F"], generator=g).to(dev)
        lens = torch.randint(20, CFG["T"] + 1, (B,), generator=g)
        lens[0] = CFG["T"]
        for _ in range(16):
            c1, c2 = (torch.randint(0, CLASSES, (B,), generator=g) for _ in range(2))
            batches.append(([c1], [c2], motion1, motion2, lens, None))
        print("# %s: %d pairs, %d model-batch rows" % (case, B, rows), flush=True)
        for storage in a.storage.split(","):
            tr_auto = make_trainer(B, storage, "torch", dev)
            tr_hip = make_trainer(B, storage, "hip", dev)
            tr_hip.encoder._pool = tr_auto.encoder._pool     # one set of workspaces: the routes run in turn, never at once
            count = [0]

            def batch():
                count[0] += 1
                return batches[count[0] % len(batches)]

            def autograd():
                tr_auto.forward(batch())
                tr_auto.update()

            routes = [("autograd", autograd), ("fused", lambda: tr_hip.train_fused_batch(batch())),
                      ("captured", lambda: tr_hip.train_fused_batch(batch(), captured=True))]
            reps = {name: [] for name, _ in routes}
            for r in range(a.repeats):
                for name, fn in routes:
                    reps[name].append(timed(fn, a.steps, a.warmup))
                print("# %s %s: round %d of %d done" % (case, storage, r + 1, a.repeats), flush=True)
            base = statistics.median(reps["autograd"])
            for name, _ in routes:
                s = summary(reps[name])
                report(dict(case=case, storage=storage, route=name, rows=rows, ms=s, repeats=reps[name], steps=a.steps,
                            vs_autograd=s["median"] / base), "  %.3f x forward() + update()" % (s["median"] / base))
            # the two class-head calls as the step makes them, per call in a replayed graph
            core = tr_hip.encoder
            ids = torch.randint(0, CLASSES, (rows,), generator=g).to(torch.int32).to(dev)
            dxo = torch.randn(rows, 1, CFG["Lt"], device=dev)
            dxp = torch.randn(rows, core.time_embed_dim, device=dev)
            for name, fn in (("class_head_fwd", lambda: core._launch_class_head(ids)),
                             ("class_head_bwd", lambda: core._launch_class_head_backward(ids, dxo, dxp))):
                v = [timed_graph(fn, a.steps, a.warmup) for _ in range(a.repeats)]
                report(dict(case=case, storage=storage, route=name, rows=rows, ms=summary(v), repeats=v, steps=a.steps),
                       "  per call in a replayed graph of %d" % a.steps)
            del tr_auto, tr_hip, core, routes
            torch.cuda.empty_cache()
        # the sums by key alone, at this case's shapes
        ids = torch.randint(0, CLASSES, (rows,), generator=g).to(torch.int32).to(dev)
        for what, width in (("sum_by_key dxf_out", CFG["Lt"]), ("sum_by_key dxf_proj", 4 * CFG["d"])):
            src = torch.randn(rows, width, device=dev)

            def by_key():
                out = torch.empty(CLASSES, width, device=dev)
                _lib.check(_lib.lib().hig_rows_sum_by_key_f32(_lib.ptr(src), _lib.ptr(ids), rows, width, CLASSES, _lib.ptr(out),
                                                             _lib.stream_ptr()))

            v = [timed_graph(by_key, a.steps, a.warmup) for _ in range(a.repeats)]
            nbytes = (rows + CLASSES) * width * 4
            s = summary(v)
            report(dict(case=case, route=what, rows=rows, bytes=nbytes, ms=s, repeats=v, steps=a.steps),
                   "  %.2f MB read + written, %.0f GB/s (per launch in a replayed graph of %d)" % (
                       nbytes / 1e6, nbytes / s["median"] / 1e6, a.steps))
    lines = [json.dumps(r) for r in results]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
