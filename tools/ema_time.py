"""Times what the EMA of the weights costs on one MI355X, on config 2's model (B = 64, T = 196, F = 150, d = 512, H = 8,
L = 8, ff = 1024) in fp32 and in bf16 storage:

  * adam / adam_ema      the update pass alone: hig_clip_adam_shadow (the path without an EMA) against hig_clip_adam_ema;
  * adam_then_ema        hig_clip_adam_shadow followed by a separate hig_ema_update (what folding the blend in saves);
  * step / step_ema      the whole fused step (DDPMTrainer.train_step_fused) without and with opt.ema_decay;
  * scope                one `with trainer.ema_weights(): pass` -- an exchange on entry and one on exit.

    python tools/ema_time.py [--steps 50] [--warmup 10] [--repeats 5] [--storage f32,bf16] [--out FILE]

Per variant: device events around `--steps` back-to-back calls after `--warmup`, divided by the steps; the repeats go round
the variants in turn, so that the variants being compared alternate in one process; median [min .. max] over the repeats.
The update passes run on copies of the trainer's buffers (a fixed gradient: the arithmetic does not matter to a streaming
pass).  Also prints the bytes each pass moves per element and the rate that is.  One JSON line per (storage, variant) at the
end.  Needs the GPU; there is no fallback.
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
from hig_amd.trainers.ddpm_trainer import ADAM_BETAS, ADAM_EPS, GRAD_CLIP  # noqa: E402

CFG = dict(B=64, T=196, F=150, d=512, H=8, L=8, ff=1024, N=77, Lt=256)
DECAY = 0.9999


def build(c, storage, dev):
    torch.manual_seed(0)
    m = hig_amd.MotionTransformer(input_feats=c["F"], num_frames=c["T"], latent_dim=c["d"], ff_size=c["ff"], num_layers=c["L"],
                                  num_heads=c["H"], text_latent_dim=c["Lt"], storage=storage)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in m.out.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.02)      # un-zero the zero-initialised output projection
    return m.to(dev).train()


def make_trainer(c, storage, dev, **opt):
    args = types.SimpleNamespace(device=dev, diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=c["B"], num_epochs=1,
                                 log_every=10 ** 9, save_latest=10 ** 9, save_every_e=1, is_continue=False, model_dir="unused", **opt)
    return hig_amd.DDPMTrainer(args, build(c, storage, dev))


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
    ap.add_argument("--storage", default="f32,bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_time.py needs the MI355X")
    if a.steps < 50:
        raise SystemExit("--steps must be at least 50")
    dev = torch.device("cuda:0")
    c = CFG
    L = _lib.lib()
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(c["B"], c["T"], c["F"], generator=g).to(dev)
    t = torch.randint(0, 1000, (c["B"],), generator=g).to(dev)
    lens = torch.randint(20, c["T"] + 1, (c["B"],), generator=g)
    lens[0] = c["T"]
    lens = lens.to(dev)
    xf_proj = torch.randn(c["B"], 4 * c["d"], generator=g).to(dev)
    xf_out = torch.randn(c["B"], c["N"], c["Lt"], generator=g).to(dev)
    results = []
    for storage in a.storage.split(","):
        plain, avg = make_trainer(c, storage, dev), make_trainer(c, storage, dev, ema_decay=DECAY)

        def step(tr):
            tr.train_step_fused(x0, t, lens, xf_proj=xf_proj, xf_out=xf_out)

        step(plain)
        step(avg)
        fp, st = plain.encoder.flat_params(), plain.fused_state()
        n = fp.core_numel
        bf16 = storage == "bf16"
        # the update passes on copies: parameters, moments, an EMA, a counter of their own
        p, m, v, e = fp.flat.clone(), st["m"].clone(), st["v"].clone(), fp.flat.clone()
        count = st["step"].clone()
        shadow = fp.shadow16_buffer().clone() if bf16 else None
        head = (_lib.ptr(p), _lib.ptr(fp.grad), _lib.ptr(m), _lib.ptr(v), n, st["lr_host"], _lib.ptr(st["lr"]), ADAM_BETAS[0],
                ADAM_BETAS[1], ADAM_EPS, GRAD_CLIP, 1.0, _lib.ptr(st["scratch"]), _lib.ptr(st["gnorm"]), _lib.ptr(count),
                _lib.ptr(shadow), n if bf16 else 0)

        def adam():
            _lib.check(L.hig_clip_adam_shadow(*head, _lib.stream_ptr()))

        def adam_ema():
            _lib.check(L.hig_clip_adam_ema(*head, _lib.ptr(e), DECAY, 1, 0, _lib.stream_ptr()))

        def adam_then_ema():
            adam()
            _lib.check(L.hig_ema_update(_lib.ptr(e), _lib.ptr(p), n, DECAY, 1, _lib.ptr(count), 0, 0, _lib.stream_ptr()))

        def scope():
            with avg.ema_weights():
                pass

        base = 30 if bf16 else 28
        variants = [("adam", adam, base), ("adam_ema", adam_ema, base + 8), ("adam_then_ema", adam_then_ema, base + 12),
                    ("step", lambda: step(plain), None), ("step_ema", lambda: step(avg), None),
                    ("scope", scope, 2 * 16 + (6 * 2 if bf16 else 0))]       # (bf16 storage: each exchange re-derives the shadow, 4 + 2 B)
        reps = {name: [] for name, _, _ in variants}
        for r in range(a.repeats):
            for name, fn, _ in variants:
                reps[name].append(timed(fn, a.steps, a.warmup))
            print("# %s: round %d of %d done" % (storage, r + 1, a.repeats), flush=True)
        for name, _, bpe in variants:
            vals = reps[name]
            med = statistics.median(vals)
            row = dict(storage=storage, variant=name, ms=dict(median=med, min=min(vals), max=max(vals)), repeats=vals, steps=a.steps,
                       elements=n, bytes_per_element=bpe, tb_per_s=None if bpe is None else bpe * n / med / 1e9)
            results.append(row)
            rate = "" if bpe is None else "  %2d B/element -> %5.2f TB/s" % (bpe, row["tb_per_s"])
            print("%-5s %-14s %8.3f ms [%8.3f .. %8.3f]%s" % (storage, name, med, min(vals), max(vals), rate), flush=True)
        del plain, avg
        torch.cuda.empty_cache()
    lines = [json.dumps(r) for r in results]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
