"""Times the evaluation protocol on the MI355X for `set_sampler(steps=20, method="dpmpp2m")`: what one scoring pass over the
generated set costs by the device route (`GeneratedMotionSet.batches`: one `hig_eval_pairs_build` launch per batch, results
kept on the device by `score_loaders`) and by the host route (`host_batches`: the reference's per-sample numpy indexing of
CPU copies, uploaded per batch), and what share of one replication the scoring pass is next to generation.

    python tools/evaluation_time.py [--repeats 5] [--copies 18] [--out FILE]

Data and weights: the synthetic two-person dataset of oracle/synth_dataset.py through `Text2MotionDatasetV2`, every clip
`--copies` times (its 7 usable clips are too few for a batch of 32, let alone for the reference's diversity_times = 300, so
the run passes smaller *_times instead of inventing motions), a `fill`-initialised `MotionInteractionTransformer` at the
reference's size (263 features, 196 frames, d = 512, 8 layers) and `fill`-initialised classifiers at the evaluator's size.  No
checkpoint exists, so the metric values mean nothing; the times do not depend on them.

The driver itself never touches the GPU.  Every device step is a child process of its own under `timeout`; the first step that
fails, faults or runs out of time ends the run, nothing is tried again.
  step `scoring`   both routes through the same classifiers in the same process, alternating, `--repeats` times after one
                   untimed round; host clock between device synchronisations; median [min .. max].  Also timed: the
                   unchanged `evaluate_matching_score` on the host route (it waits for the device in every batch).
  step `share`     one `evaluation()` replication taken apart: generation, scoring of the generated set (device route),
                   scoring of the ground truth, multimodality; the scoring pass as a share of the sum.
One JSON line per step (appended to --out).  Needs the GPU; there is no fallback.
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMITS = {"scoring": 300, "share": 300}     # seconds per device step
MM_NUM_REPEATS, MM_NUM_TIMES, BATCH = 10, 5, 32


class Repeated(object):
    """Every item of a dataset `copies` times (each visit draws its own caption and window)."""

    def __init__(self, dataset, copies):
        self.dataset, self.copies = dataset, copies

    def __len__(self):
        return len(self.dataset) * self.copies

    def __getitem__(self, item):
        return self.dataset[item % len(self.dataset)]


def setup(copies):
    import numpy as np
    import torch
    import hig_amd
    from hig_amd.datasets import EvaluatorModelWrapper, Text2MotionDatasetV2
    from hig_amd.datasets.evaluator import build_models
    from oracle import fill
    from oracle import synth_dataset as SD
    dev = torch.device("cuda:0")
    tmp = tempfile.TemporaryDirectory(prefix="hig_eval_time_")       # (kept alive by the namespace returned below)
    root = tmp.name
    dopt = SD.write(root)
    mean, std = SD.stats(np.float32)
    table = {50 + i: caps for i, caps in enumerate(SD.CAPTIONS)}
    gt_dataset = Repeated(Text2MotionDatasetV2(dopt, mean, std, dopt.split_file, caption_table=table), copies)
    model = hig_amd.MotionInteractionTransformer(input_feats=SD.F, num_frames=196, latent_dim=512, ff_size=1024, num_layers=8,
                                                 num_heads=8, text_latent_dim=256)
    model.load_state_dict(fill.fill_state_dict(model.state_dict()), strict=True)
    targs = types.SimpleNamespace(device=dev, diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=BATCH, num_epochs=1,
                                  log_every=50, save_latest=500, save_every_e=5, is_continue=False, model_dir=root, multi=True,
                                  label_path=None, cap_id=False)
    trainer = hig_amd.DDPMMulTrainer(targs, model.to(dev).eval())
    trainer.set_sampler(steps=20, method="dpmpp2m")
    copt = types.SimpleNamespace(dim_pose=SD.F, max_motion_length=196, num_layers=8, latent_dim=512)
    enc, con = build_models(copt, load=False)
    for m in (enc, con):
        m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    wrapper = EvaluatorModelWrapper(types.SimpleNamespace(dataset_name="ntu_mul", device=dev), models=(enc, con))
    opt = types.SimpleNamespace(device=dev, dim_pose=SD.F, cap_id=False)
    return types.SimpleNamespace(opt=opt, trainer=trainer, wrapper=wrapper, gt_dataset=gt_dataset, dev=dev, tmp=tmp)


def gt_batches(gt_dataset):
    import numpy as np
    import torch
    items = [gt_dataset[i] for i in range(len(gt_dataset))]
    out = []
    for lo in range(0, len(items), BATCH):
        b = items[lo:lo + BATCH]
        out.append((torch.tensor([it[0] for it in b]), [it[1] for it in b], [it[2] for it in b],
                    torch.from_numpy(np.stack([it[3] for it in b])), torch.from_numpy(np.stack([it[4] for it in b])),
                    torch.tensor([it[5] for it in b])))
    return out


def clocked(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(vals):
    return dict(median=statistics.median(vals), min=min(vals), max=max(vals))


def fmt(s):
    return "%8.2f ms [%8.2f .. %8.2f]" % (s["median"], s["min"], s["max"])


def generated(w):
    from hig_amd.datasets import GeneratedMotionSet
    return GeneratedMotionSet(w.opt, w.trainer, w.gt_dataset, MM_NUM_REPEATS)


def step_scoring(a):
    import torch
    from hig_amd.datasets import evaluate_matching_score
    from hig_amd.evaluation import score_loaders
    w = setup(a.copies)
    random.seed(1)
    torch.manual_seed(1)
    s = generated(w)
    routes = [("device route, score_loaders", lambda: score_loaders(w.wrapper, {"g": s.batches(BATCH, True)})),
              ("host route, score_loaders", lambda: score_loaders(w.wrapper, {"g": s.host_batches(BATCH, True)})),
              ("host route, evaluate_matching_score", lambda: evaluate_matching_score(w.wrapper, {"g": s.host_batches(BATCH, True)}))]
    scored = len(s) - len(s) % BATCH
    results = []
    for _, fn in routes:       # untimed round: allocations, code loading, the one-off host copies of the host route
        random.seed(2)
        results.append(fn())
    for other in results[1:]:
        assert (results[0][1]["g"] == other[1]["g"]).all() and results[0][0]["g"] == other[0]["g"], "the routes disagree"
    times = [[] for _ in routes]
    for r in range(a.repeats):
        for i, (_, fn) in enumerate(routes):
            random.seed(3 + r)
            times[i].append(clocked(fn)[0])
        print("# scoring: round %d of %d done" % (r + 1, a.repeats), flush=True)
    moved = 2 * scored * 91 * w.opt.dim_pose * 4
    row = dict(step="scoring", items=len(s), scored=scored, batches=scored // BATCH, bytes_built=moved, repeats=a.repeats,
               routes={name: dict(spread(t), all=t) for (name, _), t in zip(routes, times)})
    for (name, _), t in zip(routes, times):
        print("SCORING %-38s %s  (%d pairs in %d batches)" % (name, fmt(spread(t)), scored, scored // BATCH), flush=True)
    return row


def step_share(a):
    import numpy as np
    import torch
    from hig_amd.evaluation import evaluate_multimodality, score_loaders
    w = setup(a.copies)
    gt = gt_batches(w.gt_dataset)
    parts = dict(generation=[], scoring_generated=[], scoring_ground_truth=[], multimodality=[])
    for r in range(a.repeats + 1):
        random.seed(10 + r)
        torch.manual_seed(10 + r)
        np.random.seed(10 + r)
        t_gen, s = clocked(lambda: generated(w))
        t_score, _ = clocked(lambda: score_loaders(w.wrapper, {"g": s.batches(BATCH, True)}))
        t_gt, _ = clocked(lambda: score_loaders(w.wrapper, {"ground truth": gt}))
        t_mm, _ = clocked(lambda: evaluate_multimodality(w.wrapper, {"g": s.mm_sets(), "ground truth": s.gt_mm_sets()}, MM_NUM_TIMES))
        if r == 0:
            continue            # the first replication also pays for allocations, code loading and the graph's first capture
        for k, v in zip(parts, (t_gen, t_score, t_gt, t_mm)):
            parts[k].append(v)
        print("# share: replication %d of %d done" % (r, a.repeats), flush=True)
    med = {k: statistics.median(v) for k, v in parts.items()}
    total = sum(med.values())
    for k, v in parts.items():
        print("SHARE %-22s %s  %5.1f %% of a replication" % (k, fmt(spread(v)), 100 * med[k] / total), flush=True)
    return dict(step="share", items=len(s), repeats=a.repeats, parts={k: dict(spread(v), all=v) for k, v in parts.items()},
                scoring_share=med["scoring_generated"] / total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--copies", type=int, default=18)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(STEP_LIMITS))
    a = ap.parse_args()
    if a.step:        # a child: one device step
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("evaluation_time.py needs the MI355X")
        row = dict(scoring=step_scoring, share=step_share)[a.step](a)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
        return
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for step in ("scoring", "share"):       # the children write straight to this process's stdout
        cmd = ["timeout", "-k", "10", str(STEP_LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--repeats", str(a.repeats), "--copies", str(a.copies)] + (["--out", os.path.abspath(a.out)] if a.out else [])
        status = subprocess.run(cmd).returncode
        if status != 0:
            raise SystemExit("step %s ended with status %d: stopping, nothing further is started on the GPU" % (step, status))


if __name__ == "__main__":
    main()
