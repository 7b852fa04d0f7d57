"""Golden G18 (tests/golden/g18_eval_train.npz, g18_eval_train_update.npz): what the REFERENCE computes when its two
evaluation classifiers are trained the way tools/train_evaluation_model.py and tools/train_consistency_evaluation_model.py
train them -- its own MotionEncoder / MotionConsistencyEvalModel in .train(), nn.CrossEntropyLoss, torch.optim.Adam -- on
EVAL_CASES["tiny"] with the parameters of fill.fill_state_dict and labels (7 b + 3) % C.  Runs only where the reference
checkout exists; nothing of it is copied, only inputs and outputs.

    python tools/make_golden_eval_train.py

Per model (prefix "enc." / "con."):
    loss, logits                         one forward on the fixed batch
    grad.<name>                          every parameter's gradient (fp32 reference)
    none                                 names of the parameters whose .grad is None after backward
    floor.<name>                         rel-L2 distance of that fp32 gradient from the reference run in fp64 (model.double())
    losses                               the losses of five Adam steps on the fixed batch (lr 2e-4 encoder, 4e-5 consistency)
    upd_floor.<name>, upd_floor          rel-L2 distance of the fp32 reference's total update p_5 - p_0 from the fp64
                                         reference's: per parameter, and over the concatenation of the trained parameters
                                         WITHOUT the key thirds [d:2d] of every in_proj_bias (their gradient is rounding
                                         noise around an exact zero, which Adam divides by itself)
    upd_floor_all                        the same over everything
and in the second file (the two together would pass the size limit of a committed file):
    upd64.<name>                         p_5 - p_0 of the fp64 reference, stored as float32
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from oracle import fill  # noqa: E402
from oracle import make_golden as mg  # noqa: E402
from oracle.eval_models_ref import EVAL_CASES, eval_inputs  # noqa: E402

STEPS = 5
LR = {"enc": 2e-4, "con": 2e-4 / 5}


def labels_for(B, C):
    return torch.tensor([(7 * b + 3) % C for b in range(B)], dtype=torch.int64)


def key_third(name, d):
    """The slice of `name` left out of the update comparison (None: nothing)."""
    return slice(d, 2 * d) if name.endswith("self_attn.in_proj_bias") else None


def rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    n = np.linalg.norm(ref)
    return float(np.linalg.norm(a - ref) / n) if n > 0 else float(np.linalg.norm(a - ref))


def build(kind, c, dtype):
    from models.interaction_transformer import MotionConsistencyEvalModel, MotionEncoder
    kw = dict(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"], num_layers=c["L"],
              num_heads=c["H"])
    m = (MotionEncoder if kind == "enc" else MotionConsistencyEvalModel)(**kw)
    m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    m = m.to(dtype)
    m.train()
    return m


def run(kind, c, dtype):
    """-> (loss, logits, {name: grad or None}, five losses, {name: p_5 - p_0})."""
    x1, x2, length = eval_inputs("tiny", c)
    x1, x2 = x1.to(dtype), x2.to(dtype)
    m = build(kind, c, dtype)
    fwd = (lambda: m(x1, x2, length=length)[0]) if kind == "enc" else (lambda: m(x1, x2, length=length))
    lossfn = torch.nn.CrossEntropyLoss()
    logits = fwd()
    y = labels_for(c["B"], logits.shape[1])
    loss = lossfn(logits, y)
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}
    m = build(kind, c, dtype)
    p0 = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = torch.optim.Adam(m.parameters(), lr=LR[kind])
    losses = []
    for _ in range(STEPS):
        step_loss = lossfn(fwd(), y)
        opt.zero_grad()
        step_loss.backward()
        opt.step()
        losses.append(float(step_loss))
    upd = {k: (p.detach() - p0[k]) for k, p in m.named_parameters()}
    return float(loss), logits.detach(), grads, losses, upd


def main():
    mg.install_stubs()
    torch.manual_seed(0)
    c = EVAL_CASES["tiny"]
    out, out_upd = {}, {}
    for kind in ("enc", "con"):
        loss32, logits32, g32, losses32, u32 = run(kind, c, torch.float32)
        loss64, _, g64, losses64, u64 = run(kind, c, torch.float64)
        out[kind + ".loss"], out[kind + ".logits"] = np.float64(loss32), logits32.numpy()
        out[kind + ".loss64"] = np.float64(loss64)
        out[kind + ".losses"], out[kind + ".losses64"] = np.array(losses32), np.array(losses64)
        none = [k for k, g in g32.items() if g is None]
        assert none == [k for k, g in g64.items() if g is None]
        out[kind + ".none"] = np.array(none)
        cat32, cat64, all32, all64 = [], [], [], []
        for k, g in g32.items():
            if g is None:
                assert float(u32[k].abs().max()) == 0.0, "Adam moved a parameter that has no gradient: " + k
                continue
            out["%s.grad.%s" % (kind, k)] = g.numpy()
            out["%s.floor.%s" % (kind, k)] = np.float64(rel(g.numpy(), g64[k].numpy()))
            out["%s.upd_floor.%s" % (kind, k)] = np.float64(rel(u32[k].numpy(), u64[k].numpy()))
            out_upd["%s.upd64.%s" % (kind, k)] = u64[k].numpy().astype(np.float32)
            keep = np.ones(u32[k].shape, dtype=bool)
            sl = key_third(k, c["d"])
            if sl is not None:
                keep[sl] = False
            cat32.append(u32[k].numpy()[keep].ravel()), cat64.append(u64[k].numpy()[keep].ravel())
            all32.append(u32[k].numpy().ravel()), all64.append(u64[k].numpy().ravel())
        out[kind + ".upd_floor"] = np.float64(rel(np.concatenate(cat32), np.concatenate(cat64)))
        out[kind + ".upd_floor_all"] = np.float64(rel(np.concatenate(all32), np.concatenate(all64)))
        print("%s: loss %.8f (fp64 %.8f), losses rel %.1e, grad floors %.1e .. %.1e, update floor %.2e (all: %.2e), no gradient: %s"
              % (kind, loss32, loss64, rel(losses32, losses64), min(v for k, v in out.items() if k.startswith(kind + ".floor.")),
                 max(v for k, v in out.items() if k.startswith(kind + ".floor.")), out[kind + ".upd_floor"],
                 out[kind + ".upd_floor_all"], none))
    gold = os.path.join(ROOT, "tests", "golden")
    for name, d in (("g18_eval_train.npz", out), ("g18_eval_train_update.npz", out_upd)):
        path = os.path.join(gold, name)
        np.savez_compressed(path, **d)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
