"""Golden G23 (tests/golden/g23_loss_sampler.npz): the REFERENCE's own `LossSecondMomentResampler`
(codes/models/gaussian_diffusion.py:123-153) fed a recorded sequence of `update_with_all_losses` calls, its state after every
call.  Runs only where the reference checkout exists; nothing of it is copied, only inputs and outputs.

    python tools/make_golden_loss_sampler.py

The reference's class writes `np.int`, which current numpy no longer has, so it runs in a child process of this script in which
`np.int = int` is set before the import; the alias never reaches anything else.

The sequence (SEQUENCE below): nsteps = 7, H = 3, uniform_prob = 0.001.  Call 0 repeats a timestep inside one batch; call 1
pushes four losses under one timestep, so that a ring of three overflows within one call; after call 2 some rings are still
short (weights() is all ones: not warmed up); call 3 fills the last ring (warmed up: the first real weights()); call 4 shifts
three full rings once more.

Stored:
    nsteps, history_per_term, uniform_prob
    ts, losses               (calls, longest call) the recorded sequence, rows padded with -1 / nan;  n: the calls' lengths
    history                  (calls, nsteps, H) float64 `_loss_history` after each call
    counts                   (calls, nsteps) `_loss_counts` after each call
    weights                  (calls, nsteps) float64 `weights()` after each call
    warmed_up                (calls,) `_warmed_up()` after each call
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

NSTEPS, H, UNIFORM_PROB = 7, 3, 0.001
SEQUENCE = (
    ((0, 1, 2, 2, 3), (0.5, 0.25, 1.5, 0.75, 0.125)),
    ((4, 4, 4, 4, 5), (0.1, 0.2, 0.3, 0.4, 2.0)),
    ((0, 0, 1, 1, 2, 3, 3, 5, 5, 6), (0.6, 0.7, 0.35, 0.3, 0.9, 0.15, 0.2, 1.75, 1.5, 3.0)),
    ((6, 6), (2.5, 2.75)),
    ((0, 6, 6, 3), (0.55, 2.25, 2.0, 0.175)),
)


def child(path):
    """Inside the child process: the reference's class on SEQUENCE; the result goes to the .npz file `path`."""
    np.int = int                     # (what the reference's __init__ asks numpy for)
    from oracle import make_golden as mg
    mg.install_stubs()
    from models.gaussian_diffusion import LossSecondMomentResampler

    class Steps:
        num_timesteps = NSTEPS

    smp = LossSecondMomentResampler(Steps(), history_per_term=H, uniform_prob=UNIFORM_PROB)
    out = {"history": [], "counts": [], "weights": [], "warmed_up": []}
    for ts, losses in SEQUENCE:
        smp.update_with_all_losses(list(ts), list(losses))
        out["history"].append(np.array(smp._loss_history, dtype=np.float64))
        out["counts"].append(np.array(smp._loss_counts, dtype=np.int64))
        out["weights"].append(np.array(smp.weights(), dtype=np.float64))
        out["warmed_up"].append(bool(smp._warmed_up()))
    np.savez(path, **{k: np.stack(v) for k, v in out.items()})


def main():
    with tempfile.TemporaryDirectory() as tmp:
        part = os.path.join(tmp, "child.npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", part], check=True)
        with np.load(part) as f:
            got = {k: f[k] for k in f.files}
    longest = max(len(ts) for ts, _ in SEQUENCE)
    ts = np.full((len(SEQUENCE), longest), -1, dtype=np.int64)
    losses = np.full((len(SEQUENCE), longest), np.nan, dtype=np.float64)
    for i, (a, b) in enumerate(SEQUENCE):
        ts[i, :len(a)], losses[i, :len(b)] = a, b
    assert list(got["warmed_up"]) == [False, False, False, True, True], got["warmed_up"]
    assert (got["weights"][2] == 1.0).all() and not (got["weights"][3] == 1.0).any()
    path = os.path.join(ROOT, "tests", "golden", "g23_loss_sampler.npz")
    np.savez_compressed(path, nsteps=NSTEPS, history_per_term=H, uniform_prob=UNIFORM_PROB, ts=ts, losses=losses,
                        n=np.array([len(a) for a, _ in SEQUENCE]), **got)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    child(sys.argv[2]) if sys.argv[1:2] == ["--child"] else main()
