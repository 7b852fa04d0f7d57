"""Times the fused training step with and without the caption bank (models/caption_bank.py) on the MI355X, in one run:

  * parent   `clip_inputs(captions)` + `train_step_fused(clip_out=..., eot=...)`: every caption tokenised and sent through the
             frozen tower, the text head on every row -- the path without the bank;
  * bank     `bank.batch(captions)` + `train_step_fused(caption_batch=...)` with text_dedup off: hig_caption_gather stands where
             the tower stood, the head still runs on every row;
  * dedup    the same with text_dedup on: the head's forward and backward on the U_pad distinct captions, two row gathers and two
             segment sums around the denoiser.

The tower has the ViT-B/32 text shape (W = 512, H = 8, L = 12, N = 77, vocabulary 49408, CLIP-init weights) on the native route;
the tokenizer is the stub's word hash (the BPE vocabulary is data this repository does not carry).  Captions are drawn from a
43-entry table plus "".  Shapes: config 2's model (T = 196, F = 150, d = 512, L = 8, ff = 1024, Lt = 256) single-person at
B = 32 and 64, and the two-person PIT step (model batch c1 + c2 + c2 + c1 = 4 rows per pair) at 32 and 120 pairs; fp32 and bf16
storage.  Every timed call includes its host work (tokenizer, dict lookups, the packed index upload).  Also times the first
step of a fresh bank (its fills) and, per launch inside a replayed hipGraph of `--steps` launches (no host gaps, one output
buffer per launch), the three row kernels alone at the shapes the steps give them and the denoiser's own per-caption text side
(`_text_context`: the stacked key / value GEMM and the context build) on every row against on U_pad rows -- what running that
side per distinct caption, which is not built, would reclaim.

    python tools/caption_bank_time.py [--steps 50] [--warmup 10] [--repeats 5] [--cases single32,single64,pit32,pit120]
                                      [--storage f32,bf16] [--out FILE]

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
from hig_amd.models import caption_bank as CBK  # noqa: E402
from hig_amd.models import clip_text, stub_clip  # noqa: E402

TOWER = dict(W=512, H=8, L=12, N=77, vocab=49408)
CFG = dict(T=196, F=150, d=512, H=8, L=8, ff=1024, Lt=256)
CASES = {"single32": (False, 32), "single64": (False, 64), "pit32": (True, 32), "pit120": (True, 120)}
VERBS = ("shakes hands with", "pushes", "hugs", "points at", "pats the back of", "kicks", "punches", "waves at", "bows to",
         "hands an object to", "follows", "walks towards", "walks away from", "whispers to", "high-fives")
TABLE = (["a person %s the other person" % v for v in VERBS] + ["one person %s another while standing" % v for v in VERBS]
         + ["two people: the first %s the second slowly" % v for v in VERBS[:13]])
assert len(TABLE) == 43 and len(set(TABLE)) == 43


def build_tower():
    m = clip_text.ClipTextModel(TOWER["W"], TOWER["L"], TOWER["H"], TOWER["N"], TOWER["vocab"])
    m.initialize_parameters(generator=torch.Generator().manual_seed(0))
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def make_trainer(two, B, storage, dev, tower):
    torch.manual_seed(0)
    c = CFG
    cls = hig_amd.MotionInteractionTransformer if two else hig_amd.MotionTransformer
    m = cls(input_feats=c["F"], num_frames=c["T"], latent_dim=c["d"], ff_size=c["ff"], num_layers=c["L"], num_heads=c["H"],
            text_latent_dim=c["Lt"], storage=storage, clip_model=tower, clip_tokenize=stub_clip.tokenize, caption_bank=1024)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for mod in [m.out] + ([m.out2] if two else []):
            for p in mod.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)   # un-zero the zero-initialised output projection
    args = types.SimpleNamespace(device=dev, diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=B, num_epochs=1,
                                 log_every=10 ** 9, save_latest=10 ** 9, save_every_e=1, is_continue=False, model_dir="unused",
                                 multi=True, label_path=None, cap_id=False)
    return (hig_amd.DDPMMulTrainer if two else hig_amd.DDPMTrainer)(args, m.to(dev).train())


def draw_captions(two, B, g, p_empty=0.1):
    """One step's caption list: B captions (single-person) or the 4 B rows c1 + c2 + c2 + c1 of the PIT step."""
    def draw(n):
        ids = torch.randint(0, len(TABLE), (n,), generator=g).tolist()
        drop = (torch.rand(n, generator=g) < p_empty).tolist()
        return ["" if d else TABLE[i] for i, d in zip(ids, drop)]
    if not two:
        return draw(B)
    c1, c2 = draw(B), draw(B)
    return c1 + c2 + c2 + c1


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
    """ms per call of `fn` inside ONE replayed hipGraph of `steps` calls: no host gap between the launches, and every call
    writes an output buffer of its own (the graph's pool), so a 10 us kernel is not timed at the host's call rate."""
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
    ap.add_argument("--cases", default="single32,single64,pit32,pit120")
    ap.add_argument("--storage", default="f32,bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("caption_bank_time.py needs the MI355X")
    if a.steps < 50:
        raise SystemExit("--steps must be at least 50")
    dev = torch.device("cuda:0")
    tower = build_tower()
    results = []

    def report(row, note=""):
        results.append(row)
        ms = row["ms"]
        print("%-9s %-5s %-16s %9.3f ms [%9.3f .. %9.3f]%s" % (row["case"], row.get("storage", ""), row["route"], ms["median"],
                                                             ms["min"], ms["max"], note), flush=True)

    for case in a.cases.split(","):
        two, B = CASES[case]
        g = torch.Generator().manual_seed(7 + B)
        lists = [draw_captions(two, B, g) for _ in range(16)]             # the steps cycle through these requests
        rows = len(lists[0])
        persons = 2 * B if two else B
        x0 = torch.randn(persons, CFG["T"], CFG["F"], generator=g).to(dev)
        t = torch.randint(0, 1000, (B,), generator=g).to(dev)
        lens = torch.randint(20, CFG["T"] + 1, (B,), generator=g)
        lens[0] = CFG["T"]
        lens = lens.to(dev)
        uniq = [len(set(c)) for c in lists]
        print("# %s: %d text rows per step, %d .. %d distinct captions (U_pad %d .. %d)" % (
            case, rows, min(uniq), max(uniq), CBK.padded_unique(min(uniq)), CBK.padded_unique(max(uniq))), flush=True)
        for storage in a.storage.split(","):
            tr = make_trainer(two, B, storage, dev, tower)
            core = tr.encoder
            bank = core.caption_bank
            count = [0]

            def captions():
                count[0] += 1
                return lists[count[0] % len(lists)]

            def parent():
                clip_out, eot = tr.clip_inputs(captions())
                tr.train_step_fused(x0, t, lens, clip_out=clip_out, eot=eot)

            def banked(dedup):
                core.text_dedup = dedup
                tr.train_step_fused(x0, t, lens, caption_batch=bank.batch(captions(), dev))

            # the first step of a fresh bank: its fills (tower calls of 8 captions) and the step itself, after one parent
            # step has paid for the first-use allocations of the denoiser's workspaces
            parent()
            torch.cuda.synchronize()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before = dict(bank.stats)
            start.record()
            banked(True)
            end.record()
            end.synchronize()
            report(dict(case=case, storage=storage, route="first_step", rows=rows, fills=bank.stats["fills"] - before["fills"],
                        ms=summary([start.elapsed_time(end)])),
                   "  %d fills of %d captions" % (bank.stats["fills"] - before["fills"], CBK.FILL_CHUNK))
            routes = [("parent", parent), ("bank", lambda: banked(False)), ("bank_dedup", lambda: banked(True))]
            reps = {name: [] for name, _ in routes}
            for r in range(a.repeats):
                for name, fn in routes:
                    reps[name].append(timed(fn, a.steps, a.warmup))
                print("# %s %s: round %d of %d done" % (case, storage, r + 1, a.repeats), flush=True)
            base = statistics.median(reps["parent"])
            for name, _ in routes:
                s = summary(reps[name])
                report(dict(case=case, storage=storage, route=name, rows=rows, ms=s, repeats=reps[name], steps=a.steps,
                            vs_parent=s["median"] / base, bank_stats=dict(bank.stats)),
                       "  %.3f x the parent path" % (s["median"] / base))
            # what the follow-up would reclaim: the denoiser's own per-caption text side (the stacked key / value GEMM and the
            # cross-attention context build of every layer, hig_text_context*) on every row against on U_pad rows
            U_hi = CBK.padded_unique(max(uniq))
            for n_txt in (rows, U_hi):
                xf = torch.randn(n_txt, TOWER["N"], CFG["Lt"], device=dev)
                dims = core.dims(n_txt, CFG["T"], TOWER["N"])

                def text_side():
                    core._pool.give("textctx_t", core._text_context(dims, xf, training=True), dev)

                v = [timed_graph(text_side, a.steps, a.warmup) for _ in range(a.repeats)]
                report(dict(case=case, storage=storage, route="text_context %d" % n_txt, rows=n_txt, ms=summary(v), repeats=v,
                            steps=a.steps), "  the denoiser's text side on %d rows (graph replay)" % n_txt)
            del tr, core, bank, routes
            torch.cuda.empty_cache()

        # the three kernels alone, at this case's shapes
        N, W, Lt, E = TOWER["N"], TOWER["W"], CFG["Lt"], 4 * CFG["d"]
        bank = CBK.CaptionBank(types.SimpleNamespace(clip=tower, cap_id=False), 64)
        bank.feat = torch.randn(64 + bank.spill, N, W, device=dev)
        bank.eot = torch.zeros(64 + bank.spill, dtype=torch.int64, device=dev)
        U_pad = CBK.padded_unique(max(uniq))
        inv = torch.randint(0, max(uniq), (rows,), generator=g)
        order = torch.argsort(inv, stable=True).to(torch.int32).to(dev)
        seg = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(inv, minlength=U_pad), 0)]).to(torch.int32).to(dev)
        inv32 = inv.to(torch.int32).to(dev)
        xo_u, xp_u = torch.randn(U_pad, N, Lt, device=dev), torch.randn(U_pad, E, device=dev)
        dxo, dxp = torch.randn(rows, N, Lt, device=dev), torch.randn(rows, E, device=dev)
        kernels = [("caption_gather rows", lambda: bank.gather(inv32, rows), 2 * rows * N * W * 4),
                   ("caption_gather U_pad", lambda: bank.gather(inv32[:U_pad], U_pad), 2 * U_pad * N * W * 4),
                   ("rows_gather xf_out", lambda: CBK.expand_rows(xo_u, inv32, rows), 2 * rows * N * Lt * 4),
                   ("rows_gather xf_proj", lambda: CBK.expand_rows(xp_u, inv32, rows), 2 * rows * E * 4),
                   ("segment_sum dxo", lambda: CBK.segment_sum_rows(dxo, order, seg, U_pad), (rows + U_pad) * N * Lt * 4),
                   ("segment_sum dxp", lambda: CBK.segment_sum_rows(dxp, order, seg, U_pad), (rows + U_pad) * E * 4)]
        for name, fn, nbytes in kernels:
            v = [timed_graph(fn, a.steps, a.warmup) for _ in range(a.repeats)]
            s = summary(v)
            report(dict(case=case, route=name, rows=rows, U_pad=U_pad, bytes=nbytes, ms=s, repeats=v, steps=a.steps),
                   "  %.1f MB read + written, %.0f GB/s (per launch in a replayed graph of %d)" % (
                       nbytes / 1e6, nbytes / s["median"] / 1e6, a.steps))
        del bank, xo_u, xp_u, dxo, dxp
        torch.cuda.empty_cache()
    lines = [json.dumps(r) for r in results]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
