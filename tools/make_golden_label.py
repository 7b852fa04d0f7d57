"""Golden G22 (tests/golden/g22_label_votes.npz): the REFERENCE's labelling pass -- step (1-2) of its recipe,
`tools/label_data.py` -- draw by draw: `DDPMMulTrainer.label_batch` (codes/trainers/mul_ddpm_trainer.py:343-402) over
`MotionInteractionTransformer(cap_id=True)` on `fill` weights, case `tiny2` widened to 6 pairs (lengths with T, 2 and 9, ids
with a repeated class and a repeated pair), at the pass's four timesteps and 3 draws each, the noise injected as for g9.  Runs
only where the reference checkout exists; nothing of it is copied, only inputs and outputs.

    python tools/make_golden_label.py

Per draw `label_batch` is called twice on the same noise: with learned_indices = None (the model-mode return, `active_list`)
and with LEARNED in label mode (`(outs, file_id)`).  The two assignment sums it compares are not returned; they are rebuilt
from what the call leaves on the trainer (fake_noise, real_noise, src_mask) with the reference's own expressions, and again from
an fp64 run of the same module on the same inputs (`diffusion.training_losses(forward_twice=True)` on a `.double()` copy: the
schedule coefficients stay the fp32-rounded ones of `_extract_into_tensor`).  The decisions rebuilt from the fp32 sums must
reproduce both returns, which the script asserts.

Condition on the inputs, asserted: every (step, draw, pair) has |l1 - l0| / mean(l0, l1) >= 1e-3 in the fp64 run, so no case has
to be left out of a decision comparison.  The noise is `fill`'s named sequence (g22.noise.<k>, k = 3 step + draw); should that
sequence miss the condition, torch.randn under the first of the seeds 0, 1, .. that meets it is stored in the file under `noise`
instead.  (It does miss it: 2.9e-4 at pair 5; seed 0 gives 3.4e-5, seed 1 2.6e-3 with a median of 5e-2, and is what the file
holds.)

Stored:
    ids1, ids2, lengths      the class ids of the two captions of each pair; the lengths
    steps                    the four timesteps
    l32, l64                 (steps, draws, 2, pairs) the two assignment sums, fp32 run and fp64 run
    decisions                (steps, draws, pairs) 0: [c1, c2] is cheaper (or a tie), 1: [c2, c1]
    learned_indices          the LEARNED of the label-mode calls
    file_ids                 the batch's file ids
    active_list              (steps, draws) JSON of the model-mode return
    outs                     (steps, draws, pairs) the label-mode return
    min_margin               the smallest relative margin of the fp64 run
    [noise, noise_seed]      (steps, draws, 2 pairs, T, F) and its seed, only when `fill`'s sequence missed the condition
"""
import json
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from oracle import fill  # noqa: E402
from oracle import make_golden as mg  # noqa: E402

PAIRS, DRAWS = 6, 3
STEPS = (830, 860, 890, 920)
IDS1, IDS2 = [3, 41, 7, 3, 0, 12], [4, 3, 8, 4, 1, 13]          # class 3 three times, the pair (3, 4) twice
LENGTHS = (16, 9, 2, 16, 12, 5)
FILE_IDS = ["clip%03d" % i for i in range(PAIRS)]
LEARNED = list(range(43))
for _a in (3, 7, 12):                                            # three learned swaps: (4, 3), (8, 7), (13, 12)
    LEARNED[_a], LEARNED[_a + 1] = LEARNED[_a + 1], LEARNED[_a]
MARGIN = 1e-3


class _Feed:
    """mg._NoiseFeed with a settable position, or a fixed tensor per position."""

    def __init__(self, stored=None):
        self.k, self.stored = 0, stored

    def _next(self, shape):
        if self.stored is not None:
            return self.stored[self.k].clone()
        return fill.tensor_for("g22.noise.%d" % self.k, shape) * 10.0

    def randn(self, *shape, device=None, **_):
        return self._next(shape)

    def randn_like(self, x, **_):
        return self._next(x.shape).to(x.dtype)          # (the fp64 run gets the same fp32 values)


def assign_sums(pred, target, mask):
    """The reference's expressions (mul_ddpm_trainer.py:372-377) on any dtype: (2, pairs)."""
    init = ((pred[:, 0, :4] - target[:, 0, :4]) ** 2).mean(dim=-1)
    move = ((pred[:, 1:] - target[:, 1:]) ** 2).mean(dim=-1)
    loss = torch.cat([init.unsqueeze(1), move], dim=1)
    rows = loss.shape[0]
    return (loss * mask).sum(dim=1).view(2, rows // 2).sum(dim=0).view(2, rows // 4)


def timestep_embedding64(t, dim, max_period=10000):
    """The sinusoidal embedding (cos first) in fp64: the reference computes it in fp32 whatever the module's dtype, which its
    fp64 run cannot take."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / half)
    args = t[:, None].double() * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    return torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1) if dim % 2 else emb


def run(stored):
    import models.interaction_transformer as it
    import trainers.mul_ddpm_trainer as tr
    temb32 = it.timestep_embedding
    it.timestep_embedding = lambda t, dim: timestep_embedding64(t, dim) if run.fp64 else temb32(t, dim)
    c = dict(fill.ICASES["tiny2"], B=PAIRS, lengths=LENGTHS)
    m = mg.build_ref_interaction(c, cap_id=True).eval()
    m64 = mg.build_ref_interaction(c, cap_id=True).double().eval()
    args = types.SimpleNamespace(device=torch.device("cpu"), diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=PAIRS,
                                 num_epochs=1, log_every=50, save_latest=500, save_every_e=5, is_continue=False, model_dir="/tmp",
                                 multi=True, label_path=None, cap_id=True)
    trainer = tr.DDPMMulTrainer(args, m)
    T, Fd = c["T"], c["F"]
    motion1 = fill.tensor_for("g22.motion1", (PAIRS, T, Fd)) * 10
    motion2 = fill.tensor_for("g22.motion2", (PAIRS, T, Fd)) * 10
    # the loader's default collate hands a cap_id batch its captions as one-element lists of id tensors
    batch = ([torch.tensor(IDS1)], [torch.tensor(IDS2)], motion1, motion2, torch.tensor(LENGTHS), FILE_IDS)
    feed = _Feed(stored)
    undo = mg._patch_noise(feed)
    l32 = np.zeros((len(STEPS), DRAWS, 2, PAIRS), dtype=np.float32)
    l64 = np.zeros((len(STEPS), DRAWS, 2, PAIRS), dtype=np.float64)
    outs = np.zeros((len(STEPS), DRAWS, PAIRS), dtype=np.int64)
    active_lists = []
    try:
        with torch.no_grad():
            for si, t in enumerate(STEPS):
                active_lists.append([])
                for d in range(DRAWS):
                    feed.k = si * DRAWS + d
                    active_lists[si].append(trainer.label_batch(batch, None, t=t))
                    l32[si, d] = assign_sums(trainer.fake_noise, trainer.real_noise, trainer.src_mask).numpy()
                    o, fids = trainer.label_batch(batch, LEARNED, t=t, label_mode=True)
                    assert list(fids) == FILE_IDS
                    outs[si, d] = o
                    x0 = torch.cat([motion1, motion2]).double()
                    tt = torch.full((2 * PAIRS,), t, dtype=torch.long)
                    caption = [torch.tensor(IDS1), torch.tensor(IDS2), torch.tensor(IDS2), torch.tensor(IDS1)]
                    len4 = torch.tensor(LENGTHS * 4)
                    run.fp64 = True
                    o64 = trainer.diffusion.training_losses(model=m64, x_start=x0, t=tt,
                                                            model_kwargs={"text": caption, "length": len4}, forward_twice=True)
                    run.fp64 = False
                    assert o64["pred"].dtype == torch.float64 and o64["target"].dtype == torch.float64
                    l64[si, d] = assign_sums(o64["pred"], o64["target"], trainer.src_mask.double()).numpy()
    finally:
        undo()
        it.timestep_embedding, run.fp64 = temb32, False
    return l32, l64, outs, active_lists


run.fp64 = False


def rel_margin(l64):
    return np.abs(l64[:, :, 1] - l64[:, :, 0]) / (0.5 * (l64[:, :, 0] + l64[:, :, 1]))


def main():
    mg.install_stubs()
    stored, seed = None, -1
    l32, l64, outs, active_lists = run(None)
    margin = rel_margin(l64)
    c = fill.ICASES["tiny2"]
    while margin.min() < MARGIN and seed < 7:       # fill's sequence, then torch.randn under seed 0, 1, ..: the first that holds
        print("%s gives a relative margin of %.2e" % ("fill's sequence" if seed < 0 else "seed %d" % seed, margin.min()))
        seed += 1
        stored = torch.randn(len(STEPS) * DRAWS, 2 * PAIRS, c["T"], c["F"], generator=torch.Generator().manual_seed(seed))
        l32, l64, outs, active_lists = run(stored)
        margin = rel_margin(l64)
    assert margin.min() >= MARGIN, "smallest relative margin %.2e < %.0e" % (margin.min(), MARGIN)
    decisions = np.argmin(l32, axis=2)                       # (torch.min's index on a tie is the first too)
    assert np.array_equal(decisions, np.argmin(l64, axis=2)), "the fp32 run and the fp64 run decide differently"
    # both returns of label_batch follow from the decisions
    active = np.argmin([[LEARNED[i] for i in IDS1], [LEARNED[i] for i in IDS2]], axis=0)
    for si in range(len(STEPS)):
        for d in range(DRAWS):
            want = {}
            for p, (a, b) in enumerate(zip(IDS1, IDS2)):
                want.setdefault("%d_%d" % (a, b), []).append("%d_%d" % ((a, b) if decisions[si, d, p] == 0 else (b, a)))
            assert want == active_lists[si][d], (si, d)
            assert np.array_equal(outs[si, d], (decisions[si, d] != active).astype(np.int64)), (si, d)
    out = {"ids1": np.array(IDS1, dtype=np.int64), "ids2": np.array(IDS2, dtype=np.int64),
           "lengths": np.array(LENGTHS, dtype=np.int64), "steps": np.array(STEPS, dtype=np.int64), "l32": l32, "l64": l64,
           "decisions": decisions.astype(np.int64), "learned_indices": np.array(LEARNED, dtype=np.int64),
           "file_ids": np.array(FILE_IDS), "active_list": np.array([[json.dumps(a) for a in row] for row in active_lists]),
           "outs": outs, "min_margin": np.float64(margin.min())}
    if stored is not None:
        out["noise_seed"] = np.int64(seed)
        out["noise"] = stored.view(len(STEPS), DRAWS, 2 * PAIRS, c["T"], c["F"]).numpy()
    path = os.path.join(mg.GOLD, "g22_label_votes.npz")
    np.savez_compressed(path, **out)
    rel32 = np.abs(l32.astype(np.float64) - l64) / np.abs(l64)
    print("wrote %s (%d bytes): smallest relative margin %.2e (median %.2e), decisions %s, fp32 run within %.2e of fp64"
          % (path, os.path.getsize(path), margin.min(), np.median(margin), np.bincount(decisions.reshape(-1)).tolist(),
             rel32.max()))


if __name__ == "__main__":
    main()
