"""Golden G20 (tests/golden/g20_evaluation.npz): what the REFERENCE's generated-motion datasets hand to the evaluation
classifiers -- `EvaluationDataset.__getitem__` and `MMGeneratedDataset.__getitem__` (codes/datasets/evaluator.py:143-166,
346-387) -- on deterministic `fill` motions under a fixed `random` seed.  Both classes are instantiated WITHOUT their
constructors (those load a checkpoint and sample): `generated_motion` / `dataset` and `max_motion_length` are set directly.
Runs only where the reference checkout exists; nothing of it is copied, only inputs and outputs.

    python tools/make_golden_evaluation.py

Stored:
    seed                       what `random.seed` got before the sequence below
    lens                       m_len of the seven items: 2, 21, 90, 91, 92, 150, 196 (n = m_len - 1 = 1, 20, 89, 90, 91, 149, 195)
    motion1, motion2           (7, 196, F) the items' motions, rows at and beyond m_len NaN (they were cut off before the call)
    item.motion1, item.motion2 (7, 91, F) `EvaluationDataset[i]` for i = 0 .. 6, in that order
    item.length                the m_length each call returned
    mm.lens                    lengths of ONE class's multimodality motions, in list order, with ties (motions: `mm.motion1/2`)
    mm.out1, mm.out2, mm.out_lens   what `MMGeneratedDataset[0]` returned for them right after the seven calls above
    next_draw                  `random.random()` after the whole sequence: pins how many draws it consumed
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from oracle import fill  # noqa: E402
from oracle import make_golden as mg  # noqa: E402

SEED = 20
F = 7
LENS = [2, 21, 90, 91, 92, 150, 196]
MM_LENS = [150, 92, 150, 21, 92, 196, 91, 2, 196]
T_MAX = 196


def motions(tag, lens):
    """(len(lens), T_MAX, F) float32, NaN at and beyond each m_len."""
    out = np.full((len(lens), T_MAX, F), np.nan, dtype=np.float32)
    for i, n in enumerate(lens):
        out[i, :n] = (fill.tensor_for("g20.%s.%d" % (tag, i), (n, F)) * 10.0).numpy()
    return out


def main():
    mg.install_stubs()
    if not hasattr(np, "int"):
        np.int = int      # MMGeneratedDataset builds np.array(m_lens, dtype=np.int)
    from datasets.evaluator import EvaluationDataset, MMGeneratedDataset
    m1, m2 = motions("m1", LENS), motions("m2", LENS)
    q1, q2 = motions("q1", MM_LENS), motions("q2", MM_LENS)
    ds = EvaluationDataset.__new__(EvaluationDataset)
    ds.max_motion_length = 90
    ds.generated_motion = [dict(motion1=m1[i, :n].copy(), motion2=m2[i, :n].copy(), length=n, caption1="a", caption2="b",
                                cap_id=i % 3) for i, n in enumerate(LENS)]
    mm = MMGeneratedDataset.__new__(MMGeneratedDataset)
    mm.max_motion_length = 90
    mm.dataset = [dict(cap_id=0, mm_motions=[dict(motion1=q1[i, :n].copy(), motion2=q2[i, :n].copy(), length=n)
                                             for i, n in enumerate(MM_LENS)])]
    random.seed(SEED)
    items = [ds[i] for i in range(len(LENS))]
    o1, o2, olens = mm[0]
    nxt = random.random()
    out = dict(seed=np.int64(SEED), lens=np.array(LENS, dtype=np.int64), motion1=m1, motion2=m2,
               **{"item.motion1": np.stack([it[3] for it in items]), "item.motion2": np.stack([it[4] for it in items]),
                  "item.length": np.array([it[5] for it in items], dtype=np.int64),
                  "mm.lens": np.array(MM_LENS, dtype=np.int64), "mm.motion1": q1, "mm.motion2": q2,
                  "mm.out1": o1, "mm.out2": o2, "mm.out_lens": np.asarray(olens, dtype=np.int64)},
               next_draw=np.float64(nxt))
    assert out["item.motion1"].shape == (len(LENS), 91, F) and o1.shape == (len(MM_LENS), 91, F)
    assert all(np.isfinite(out[k]).all() for k in ("item.motion1", "item.motion2", "mm.out1", "mm.out2"))
    path = os.path.join(ROOT, "tests", "golden", "g20_evaluation.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; next draw", nxt)


if __name__ == "__main__":
    main()
