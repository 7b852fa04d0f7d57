"""Training the evaluation classifiers, the part that needs no GPU:

  * the fp64 oracle (oracle/eval_models_ref.py) under autograd with F.cross_entropy reproduces what the REFERENCE's own
    MotionEncoder / MotionConsistencyEvalModel compute in .train() (tests/golden/g18_eval_train.npz, written by
    tools/make_golden_eval_train.py): loss, every parameter's gradient to 10x that parameter's stored `floor` (the fp32
    reference's own rel-L2 distance from its fp64 self), and the set of parameters without a gradient;
  * the host logic of the `trainable=True` classes, of `softmax_xent` and of `EvalModelTrainer`.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hig_amd  # noqa: E402
from hig_amd import _lib  # noqa: E402
from hig_amd.models.evaluation_models import softmax_xent  # noqa: E402
from oracle import fill  # noqa: E402
from oracle import eval_models_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
UNUSED = {"init_pos_embedding", "time_embed.0.weight", "time_embed.0.bias", "time_embed.2.weight", "time_embed.2.bias"}


def labels_for(B, C):
    return torch.tensor([(7 * b + 3) % C for b in range(B)], dtype=torch.int64)


def oracle_params(kind, c, class_num, dtype=torch.float64):
    shapes = R.param_shapes(kind, c["F"], c["d"], c["ff"], c["L"], c["num_frames"], class_num)
    return {k: fill.tensor_for(k, s).to(dtype).requires_grad_(True) for k, s in shapes.items()}


def oracle_loss(kind, p, c, feat_weight=0.0):
    x1, x2, length = R.eval_inputs("tiny", c)
    x1, x2 = x1.double(), x2.double()
    if kind == "enc":
        logits, feat = R.motion_encoder_forward(p, x1, x2, length, c["H"])
    else:
        logits, feat = R.consistency_forward(p, x1, x2, length, c["H"]), None
    loss = F.cross_entropy(logits, labels_for(c["B"], logits.shape[1]))
    if feat_weight:
        loss = loss + feat_weight * feat.square().sum()
    return loss, logits


@pytest.mark.parametrize("kind,class_num", [("enc", 26), ("con", 2)])
def test_oracle_gradients_reproduce_the_reference(kind, class_num):
    g = np.load(os.path.join(GOLD, "g18_eval_train.npz"))
    c = R.EVAL_CASES["tiny"]
    p = oracle_params(kind, c, class_num)
    loss, logits = oracle_loss(kind, p, c)
    loss.backward()
    # the losses: the fp64 reference to fp64 rounding, the fp32 reference to fp32 rounding of ~ a hundred operations
    assert abs(loss.item() - float(g[kind + ".loss64"])) <= 1e-12 * abs(loss.item())
    assert abs(loss.item() - float(g[kind + ".loss"])) <= 1e-6 * abs(loss.item())
    assert (logits.detach() - torch.from_numpy(g[kind + ".logits"]).double()).norm() <= 1e-5 * logits.norm()
    none = {k for k, v in p.items() if v.grad is None}
    assert none == set(g[kind + ".none"].tolist()) == UNUSED
    worst = (0.0, None)
    for k, v in p.items():
        if v.grad is None:
            continue
        ref = torch.from_numpy(g["%s.grad.%s" % (kind, k)]).double()
        floor = float(g["%s.floor.%s" % (kind, k)])
        err = ((v.grad - ref).norm() / ref.norm()).item()
        worst = max(worst, (err / floor, k))
        assert floor > 0 and err <= 10 * floor, "%s: rel-L2 %.2e is %.1f x its floor %.2e" % (k, err, err / floor, floor)
    print("%s: worst multiple of the reference's own floor %.2f (%s)" % (kind, *worst))


def tiny_model(cls, **kw):
    c = R.EVAL_CASES["tiny"]
    m = cls(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"], num_layers=c["L"],
            num_heads=c["H"], **kw)
    m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    return m, c


@pytest.mark.parametrize("cls", [hig_amd.MotionEncoder, hig_amd.MotionConsistencyEvalModel])
def test_trainable_flag_host_logic(cls):
    plain, c = tiny_model(cls)
    train, _ = tiny_model(cls, trainable=True)
    assert plain.trainable is False and train.trainable is True
    assert list(plain.state_dict()) == list(train.state_dict())          # keys and order as before
    x1, x2, length = R.eval_inputs("tiny", c)
    for m in (plain, train):                                             # no CPU fallback, with or without the flag
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.train()(x1, x2, length=length)
    with pytest.raises(ValueError, match="no gradient for x1 / x2"):
        train(x1.clone().requires_grad_(True), x2, length=length)
    with pytest.raises(ValueError, match="must both be"):
        train(x1, x2[:, :, :-1], length=length)
    with pytest.raises(ValueError, match="must both be"):
        train(x1[:, :1], x2[:, :1], length=length)
    with pytest.raises(ValueError, match="one entry per pair"):
        train(x1, x2, length=length[:-1])
    with pytest.raises(ValueError, match="length is required"):
        train(x1, x2)
    names = {k for k, v in train.named_parameters() if any(v is t for t in train.trained_parameters())}
    assert {k for k, _ in train.named_parameters()} - names == UNUSED
    with torch.no_grad():                                                # under no_grad the flag changes nothing
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            train(x1, x2, length=length)


def test_softmax_xent_refusals():
    logits = torch.zeros(3, 26)
    for bad in ([0, 26, 1], [0, -1, 1]):
        with pytest.raises(ValueError, match="label outside"):
            softmax_xent(logits, torch.tensor(bad))
    with pytest.raises(ValueError, match="integer class indices"):
        softmax_xent(logits, torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="integer class indices"):
        softmax_xent(logits, torch.tensor([0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="fp32"):
        softmax_xent(logits.double(), torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError, match="C <= 1024"):
        softmax_xent(torch.zeros(2, 1025), torch.tensor([0, 1]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        softmax_xent(logits, torch.tensor([0, 25, 1]))


def opt_for(tmp_path, **kw):
    return types.SimpleNamespace(lr=2e-4, num_epochs=4, log_every=2, dim_pose=15, model_dir=str(tmp_path / "model"), **kw)


def test_trainer_learning_rate_and_kind(tmp_path):
    enc, _ = tiny_model(hig_amd.MotionEncoder)
    con, _ = tiny_model(hig_amd.MotionConsistencyEvalModel)
    assert hig_amd.EvalModelTrainer is hig_amd.trainers.EvalModelTrainer and "EvalModelTrainer" in hig_amd.__all__
    te = hig_amd.EvalModelTrainer(opt_for(tmp_path), enc, kind="encoder")
    tc = hig_amd.EvalModelTrainer(opt_for(tmp_path), con, kind="consistency")
    assert te.lr == 2e-4 and tc.lr == 2e-4 / 5 and te.class_num == 26 and tc.class_num == 2
    with pytest.raises(ValueError):
        hig_amd.EvalModelTrainer(opt_for(tmp_path), enc, kind="other")
    with pytest.raises(RuntimeError, match="trainable=True"):
        te.train_step_fused(None, None, None, None)
    # the tuple formats and feature cuts of the two scripts
    m1, m2 = torch.randn(2, 5, 19), torch.randn(2, 5, 19)
    lab, a, b, lens = te.unpack((torch.tensor([3, 4]), m1, m2, torch.tensor([5, 2]), None))
    assert a.shape == (2, 5, 15) and torch.equal(a, m1[:, :, :15]) and lab.tolist() == [3, 4] and lens.tolist() == [5, 2]
    assert not lab.is_cuda                                               # host labels: the ones softmax_xent range-checks
    lab, a, b, lens = tc.unpack((None, m1, m2, torch.tensor([5, 2]), None, torch.tensor([1, 0])))
    assert b.shape == (2, 5, 15) and torch.equal(b, m2[:, :, :-4]) and lab.tolist() == [1, 0]


def test_trainer_epoch_range_and_checkpoint_round_trip(tmp_path):
    """`for epoch in range(1, opt.num_epochs)` (num_epochs - 1 passes, as in the reference), best_eval_model.pth on every
    improvement of the validation accuracy, and a checkpoint that loads with strict=True into a default-built model.  The
    step and the forward are stubbed: on this side of the library only the loop is under test."""
    model, c = tiny_model(hig_amd.MotionEncoder)
    opt = opt_for(tmp_path)
    tr = hig_amd.EvalModelTrainer(opt, model, kind="encoder")
    steps, evals = [], iter([0.25, 0.5, 0.5])
    x = torch.zeros(3, c["T"], 19)
    batches = [(torch.tensor([0, 1, 2]), x, x, torch.tensor([12, 7, 1]), None)] * 3

    def step(m1, m2, lens, labels):
        steps.append(m1.shape)
        with torch.no_grad():
            model.out1.bias.add_(1.0)
        return torch.tensor(0.5), torch.tensor([0, 1, 0])

    tr.train_step = step
    tr.evaluate = lambda loader: next(evals)
    train_acc, val_acc = tr.train(batches, batches)
    assert len(steps) == 3 * (opt.num_epochs - 1) and steps[0] == (3, c["T"], 15)
    assert val_acc == [0.25, 0.5, 0.5] and train_acc == [pytest.approx(2 / 3)] * 3 and tr.train_losses == [pytest.approx(0.5)] * 3
    assert tr.best_acc == 0.5
    path = os.path.join(opt.model_dir, "best_eval_model.pth")
    sd = torch.load(path, map_location="cpu")
    fresh, _ = tiny_model(hig_amd.MotionEncoder)                          # default-built: inference
    fresh.load_state_dict(sd, strict=True)
    assert list(sd) == list(model.state_dict())
    # saved at the end of epoch 2 (the second improvement), not touched by epoch 3
    moved = fresh.out1.bias.detach() - fill.fill_state_dict(model.state_dict())["out1.bias"]
    assert (moved - 6.0).abs().max() < 1e-5 and (model.out1.bias.detach() - fresh.out1.bias.detach() - 3.0).abs().max() < 1e-5
    from hig_amd.datasets.evaluator import build_models
    o = types.SimpleNamespace(dim_pose=c["F"] + 4, max_motion_length=c["num_frames"], num_layers=c["L"], latent_dim=c["d"])
    assert list(build_models(o, load=False)[0].state_dict()) == list(sd)


def test_new_symbols_are_declared_and_bound():
    for s in ("hig_fullattn_bwd_kpad", "hig_softmax_xent", "hig_eval_encoder_train_workspace_bytes",
              "hig_eval_encoder_bwd_workspace_bytes", "hig_eval_encoder_fwd_train", "hig_eval_encoder_bwd"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib(), s)
    with open(os.path.join(ROOT, "include", "hig.h")) as f:
        header = f.read()
    assert "int hig_fullattn_bwd_kpad(" in header and "const uint8_t* kpad, hig_stream_t stream);" in header
    # the workspace sizes answer on the host, and refuse what the forward refuses
    L = _lib.lib()
    import ctypes as C
    dims = _lib.EvalDims(B=3, T=12, F=15, d=64, H=8, ff=128, L=2, C=26, cls=0, prec=_lib.PREC_F32)
    assert L.hig_eval_encoder_train_workspace_bytes(C.byref(dims)) > L.hig_eval_encoder_workspace_bytes(C.byref(dims)) > 0
    assert L.hig_eval_encoder_bwd_workspace_bytes(C.byref(dims)) > 0
    dims.H = 5
    assert L.hig_eval_encoder_train_workspace_bytes(C.byref(dims)) == -1 and L.hig_eval_encoder_bwd_workspace_bytes(C.byref(dims)) == -1
