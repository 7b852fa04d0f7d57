"""Training loop of the two evaluation classifiers, after the reference's two scripts
(codes/tools/train_evaluation_model.py and codes/tools/train_consistency_evaluation_model.py):

    kind "encoder"      MotionEncoder, batches (class_id, motion1, motion2, m_lens, _), features [:, :, :opt.dim_pose],
                        Adam(lr = opt.lr)
    kind "consistency"  MotionConsistencyEvalModel, batches (cap_id, motion1, motion2, m_lens, _, label), features
                        [:, :, :-4], Adam(lr = opt.lr / 5)

`for epoch in range(1, opt.num_epochs)`: one pass over the training loader, one over the validation loader,
`best_eval_model.pth` (`torch.save(model.state_dict())`) whenever the validation accuracy improves.  The datasets are the
caller's: any loader that yields these tuples will do.

With a `trainable=True` model a step is four C-ABI calls on flat device buffers (`train_step_fused`):
hig_eval_encoder_fwd_train -> hig_softmax_xent -> hig_eval_encoder_bwd -> hig_clip_adam(max_norm = 0: no clipping, torch's
Adam defaults).  `train_step` is the same step through autograd and `torch.optim.Adam`, the reference's own lines.
"""
import os
from collections import OrderedDict

import torch

from .. import _lib
from ..models.evaluation_models import softmax_xent

__all__ = ["EvalModelTrainer"]

ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8       # torch.optim.Adam's defaults, as both scripts use them
_ALIGN = 64                                      # floats: every parameter starts on a 256-byte boundary of the flat buffers


class EvalModelTrainer:
    def __init__(self, opt, model, kind="encoder"):
        if kind not in ("encoder", "consistency"):
            raise ValueError("kind must be 'encoder' or 'consistency', got %r" % (kind,))
        self.opt, self.model, self.kind = opt, model, kind
        self.lr = opt.lr if kind == "encoder" else opt.lr / 5
        head = model.fin_proj[0] if kind == "encoder" else model.cls_output[0]
        self.class_num = head.out_features
        self.log_every = max(int(getattr(opt, "log_every", 50)), 1)
        self.accuracy_train_results, self.accuracy_val_results, self.train_losses = [], [], []
        self.best_acc = 0
        self._fused = None
        self._optimizer = None

    # ---- batches ---------------------------------------------------------------------------------------------------------
    def unpack(self, batch):
        """-> (labels, motion1, motion2, m_lens) with the features cut the way the kind's script cuts them.  The labels are
        handed on as a HOST tensor: `softmax_xent` checks the range of host labels only (a check of device labels would be a
        read-back per step), so the loop's labels are always checked."""
        if self.kind == "encoder":
            labels, motion1, motion2, m_lens, _ = batch
            cut = slice(None, self.opt.dim_pose)
        else:
            _, motion1, motion2, m_lens, _, labels = batch
            cut = slice(None, -4)
        dev = next(self.model.parameters()).device
        return (torch.as_tensor(labels).cpu(), motion1.to(dev).float()[:, :, cut], motion2.to(dev).float()[:, :, cut], m_lens)

    def _logits(self, motion1, motion2, m_lens):
        out = self.model(motion1, motion2, length=m_lens)
        return out[0] if self.kind == "encoder" else out

    # ---- the step through autograd (the reference's lines) ---------------------------------------------------------------
    def train_step(self, motion1, motion2, m_lens, labels):
        if self._optimizer is None:
            self._optimizer = torch.optim.Adam(self.model.parameters(), lr=self.lr)
        pred = self._logits(motion1, motion2, m_lens)
        loss = torch.nn.functional.cross_entropy(pred, torch.as_tensor(labels).to(pred.device))
        self._optimizer.zero_grad()
        loss.backward()
        self._optimizer.step()
        return loss.detach(), pred.detach().max(dim=1).indices

    # ---- the fused step --------------------------------------------------------------------------------------------------
    def fused_state(self):
        """Flat parameter / gradient / Adam-moment buffers over the parameters the forward uses (`time_embed.*` and
        `init_pos_embedding` stay outside: no gradient, no update).  The parameters become views of the flat buffer; when
        `.to()` has re-homed them since, the buffers are rebuilt around the new storage and the moments move along."""
        params = self.model.trained_parameters()
        st = self._fused
        if st is not None and all(p.data_ptr() == v.data_ptr() for p, v in zip(params, st["views"])):
            return st
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError("EvalModelTrainer: the fused step needs the model on a ROCm device (no CPU fallback)")
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        flat = torch.zeros(n, device=dev, dtype=torch.float32)
        grad = torch.zeros(n, device=dev, dtype=torch.float32)   # (the padding between parameters stays 0: Adam leaves it alone)
        views, gviews = [], []
        for p, o in zip(params, offs):
            v = flat[o:o + p.numel()].view(p.shape)
            v.copy_(p.data)
            p.data = v
            views.append(v)
            gviews.append(grad[o:o + p.numel()].view(p.shape))
        new = {"flat": flat, "grad": grad, "views": views, "gviews": gviews, "n": n,
               "m": torch.zeros_like(flat), "v": torch.zeros_like(flat),
               "step": torch.zeros(1, device=dev, dtype=torch.int32),
               "scratch": torch.zeros(_lib.NORM_BLOCKS, device=dev, dtype=torch.float32),
               "loss": torch.zeros((), device=dev, dtype=torch.float32)}
        if st is not None and st["n"] == n:
            for k in ("m", "v", "step"):
                new[k].copy_(st[k])
        self._fused = new
        return new

    def train_step_fused(self, motion1, motion2, m_lens, labels):
        """One step as four C-ABI calls; -> (loss, predicted classes), both on the device, nothing read back.  Host labels
        are range-checked; device labels are taken as they are (a label outside [0, C) then adds no one-hot term)."""
        model = self.model
        if not getattr(model, "trainable", False):
            raise RuntimeError("EvalModelTrainer.train_step_fused needs a model built with trainable=True")
        st = self.fused_state()
        logits, _, saved = model._launch_train(motion1, motion2, m_lens, self.class_num)
        try:
            loss, dlogits, pred = softmax_xent(logits, labels, loss=st["loss"])
        except Exception:
            model._release(saved)
            raise
        model._launch_bwd(saved, dlogits, None, grads=st["gviews"])
        with torch.cuda.device(st["flat"].device):
            _lib.api.hig_clip_adam(st["flat"], st["grad"], st["m"], st["v"], st["n"], self.lr, ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS,
                                   0.0, 1.0, st["scratch"], None, st["step"])
        return loss.clone(), pred

    # ---- the loop --------------------------------------------------------------------------------------------------------
    def save(self, path):
        """`torch.save(model.state_dict())` with every tensor on its own storage (a view of the flat buffer would drag the
        whole buffer into the file).  Loads with strict=True into a default-built model."""
        torch.save(OrderedDict((k, v.detach().clone()) for k, v in self.model.state_dict().items()), path)

    def evaluate(self, loader):
        self.model.eval()
        hits, seen = None, 0
        for batch in loader:
            labels, motion1, motion2, m_lens = self.unpack(batch)
            with torch.no_grad():
                pred = self._logits(motion1, motion2, m_lens).max(dim=1).indices
            h = (pred == labels.to(pred.device)).sum()
            hits = h if hits is None else hits + h
            seen += labels.numel()
        return float(hits) / seen if seen else 0.0

    def train(self, train_loader, val_loader, plot=False):
        """-> (train accuracies, validation accuracies), one entry per epoch.  Loss and accuracy are read back once per
        `opt.log_every` steps (and at the end of an epoch), never per step."""
        opt = self.opt
        os.makedirs(opt.model_dir, exist_ok=True)
        fused = bool(getattr(self.model, "trainable", False))
        for epoch in range(1, opt.num_epochs):
            self.model.train()
            hits, seen, loss_sum, last_loss, pending = 0, 0, 0.0, float("nan"), []

            def flush():   # the one read-back: hits and losses of the steps since the last one
                nonlocal hits, seen, loss_sum, last_loss
                if pending:
                    hits += int(torch.stack([h for h, _, _ in pending]).sum())
                    vals = torch.stack([v for _, v, _ in pending]).tolist()
                    loss_sum += sum(v * n for v, (_, _, n) in zip(vals, pending))
                    seen += sum(n for _, _, n in pending)
                    last_loss = vals[-1]
                    del pending[:]

            for i, batch in enumerate(train_loader):
                labels, motion1, motion2, m_lens = self.unpack(batch)
                step = self.train_step_fused if fused else self.train_step
                loss, pred = step(motion1, motion2, m_lens, labels)
                pending.append(((pred == labels.to(pred.device)).sum(), loss, labels.numel()))
                if (i + 1) % self.log_every == 0:
                    flush()
                    print("epoch %d step %d: loss %.4f acc %.4f" % (epoch, i + 1, last_loss, hits / max(seen, 1)))
            flush()
            self.accuracy_train_results.append(hits / max(seen, 1))
            self.train_losses.append(loss_sum / max(seen, 1))
            self.accuracy_val_results.append(self.evaluate(val_loader))
            if self.best_acc < self.accuracy_val_results[-1]:
                self.best_acc = self.accuracy_val_results[-1]
                self.save(os.path.join(opt.model_dir, "best_eval_model.pth"))
                print("best acc: ", self.best_acc)
                print("model saved")
            if plot:
                self._plot()
            print(epoch, "epoch done")
        return self.accuracy_train_results, self.accuracy_val_results

    def _plot(self):
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        import numpy as np
        os.makedirs("result", exist_ok=True)
        name = "eval_model" if self.kind == "encoder" else "eval_consitency_model"
        plt.plot(np.arange(len(self.accuracy_train_results)) + 1, self.accuracy_train_results)
        plt.plot(np.arange(len(self.accuracy_val_results)) + 1, self.accuracy_val_results)
        plt.xlabel("Epoch")
        plt.ylabel("Accuracy")
        plt.savefig("result/%s_acc.jpg" % name)
        plt.close()
