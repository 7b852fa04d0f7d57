"""The evaluation run of the reference (codes/tools/evaluation.py:56-264) over the generated sets of
`datasets/evaluator.py`: per replication accuracy, consistency and activations per loader, FID against the 'ground truth'
activations, diversity, multimodality; then mean and 1.96 std / sqrt(replications) per metric and loader.

    trainer.set_sampler(steps=20, method="dpmpp2m", guidance_scale=2.5)
    res = hig_amd.evaluation(EvaluatorModelWrapper(opt), gt_batches,
                             {"text2motion": lambda: GeneratedMotionSet(opt, trainer, gt_dataset, 20)}, replication_times=20)

The scoring pass (`score_loaders`) stands beside `datasets.evaluate_matching_score`, which is unchanged: the same numbers, but
hits, consistency flags, features and logits stay device tensors until a loader is done and come back in ONE transfer, so
the host never waits for the device between batches.  The metric functions are those of `utils/metrics.py` (golden g14) and
draw from numpy's global generator as the reference does; the windows of the generated sets draw from Python's `random`.

Not built: confusion-matrix plots, R-precision / matching score (no reference tool calls them), the argument parsing of
tools/evaluation.py.
"""
import os
from collections import OrderedDict
from datetime import datetime

import numpy as np
import torch

from .datasets.evaluator import evaluate_fid
from .utils.metrics import calculate_diversity, calculate_multimodality

GROUND_TRUTH = 'ground truth'
METRICS = ('Acc', 'FID', 'FID2', 'Consistency', 'Diversity', 'MultiModality')


def _say(log, line):
    if log is not None:
        print(line, file=log, flush=True)


def score_loaders(eval_wrapper, motion_loaders):
    """`evaluate_matching_score` (tools/evaluation.py:56-112 without the plots) with the per-batch results kept on the
    device: -> (acc_dict, activation_dict, activation2_dict, consistency_dict), activations as numpy arrays.  Batches are
    `(class_id, _, _, motions1, motions2, m_lens)`; host tensors are moved by the wrapper, device tensors are used as they
    are.  Per loader: one concatenation of [feature | logits | hit | consistent] rows and one copy to the host."""
    acc_dict, consistency_dict = OrderedDict(), OrderedDict()
    activation_dict, activation2_dict = OrderedDict(), OrderedDict()
    for name, loader in motion_loaders.items():
        rows = []
        for batch in loader:
            class_id, _, _, motions1, motions2, m_lens = batch
            fin, feat, cons = eval_wrapper.get_motion_embeddings(motions1=motions1, motions2=motions2, m_lens=m_lens)
            class_id = torch.as_tensor(class_id).to(fin.device, non_blocking=True).view(-1)
            hit = (fin.max(dim=1).indices == class_id).to(feat.dtype)
            consistent = (cons.max(dim=1).indices == 0).to(feat.dtype)
            rows.append(torch.cat([feat, fin.to(feat.dtype), hit[:, None], consistent[:, None]], dim=1))
        if not rows:
            raise ValueError("loader %r yielded no batch" % (name,))
        d, c = feat.shape[1], fin.shape[1]
        table = torch.cat(rows, dim=0).cpu().numpy()          # the loader's only device-to-host transfer
        activation_dict[name] = np.ascontiguousarray(table[:, :d])
        activation2_dict[name] = np.ascontiguousarray(table[:, d:d + c])
        acc_dict[name] = float(table[:, d + c].sum()) / len(table)        # (0 / 1 flags: the fp32 sum is exact)
        consistency_dict[name] = float(table[:, d + c + 1].sum()) / len(table)
    return acc_dict, activation_dict, activation2_dict, consistency_dict


def evaluate_diversity(activation_dict, diversity_times, log=None):
    """tools/evaluation.py:138-146."""
    out = OrderedDict()
    for name, act in activation_dict.items():
        out[name] = calculate_diversity(act, diversity_times)
        _say(log, f'---> [{name}] Diversity: {out[name]:.4f}')
    return out


def evaluate_multimodality(eval_wrapper, mm_sets_by_name, mm_num_times, log=None):
    """tools/evaluation.py:149-169: per loader the features of every class's `(motions1, motions2, m_lens)` set stacked to
    (classes, repeats, dim) -> `calculate_multimodality`; 0 for a loader without a set.  The reference stacks with
    torch.cat, so every class must bring the same number of repeats."""
    out = OrderedDict()
    for name, sets in mm_sets_by_name.items():
        feats = [eval_wrapper.get_motion_embeddings(m1, m2, lens)[1] for m1, m2, lens in sets]
        if not feats:
            out[name] = 0
        else:
            if len({f.shape[0] for f in feats}) != 1:
                raise ValueError("multimodality of %r: the classes bring %s repeats; all must bring the same number"
                                 % (name, sorted({f.shape[0] for f in feats})))
            out[name] = calculate_multimodality(torch.stack(feats, dim=0).cpu().numpy(), mm_num_times)
        _say(log, f'---> [{name}] Multimodality: {out[name]:.4f}')
    return out


def get_metric_statistics(values, replication_times):
    """tools/evaluation.py:172-176 -> (mean, 1.96 std / sqrt(replication_times)) over the replications (axis 0)."""
    values = np.asarray(values)
    mean = np.mean(values, axis=0)
    std = np.std(values, axis=0)
    return mean, 1.96 * std / np.sqrt(replication_times)


def evaluation(eval_wrapper, gt_batches, make_generated, replication_times=1, diversity_times=300, mm_num_times=15,
               batch_size=32, log=None):
    """tools/evaluation.py:179-264.  -> OrderedDict with the reference's keys 'Acc', 'FID', 'FID2', 'Consistency',
    'Diversity', 'MultiModality', each {loader name: (mean, conf_interval)} over the replications.

    gt_batches      the ground-truth loader: an iterable (walked once per replication) of
                    `(class_id, caption1, caption2, motions1, motions2, m_lens)` batches, not dropped
    make_generated  {name: callable -> a `GeneratedMotionSet`}; called once per replication, so every replication samples
                    anew with whatever `set_sampler` selected.  Its `batches(batch_size, drop_last=True)` is the loader
                    `name`, its `mm_sets()` the multimodality sets of `name`, its `gt_mm_sets()` those of 'ground truth'
                    (as in the reference, the last getter's win)
    log             a file object or a path: gets the reference's `---> [name] ...` lines

    'FID2' is the FID of `activation2_dict`, the class logits, against the ground truth's.  The reference declares the key
    and never fills it; here it is filled."""
    opened = isinstance(log, (str, os.PathLike))
    f = open(log, 'w') if opened else log
    try:
        all_metrics = OrderedDict((k, OrderedDict()) for k in METRICS)
        for replication in range(replication_times):
            motion_loaders, mm_sets = OrderedDict(), OrderedDict()
            motion_loaders[GROUND_TRUTH] = gt_batches
            for name, getter in make_generated.items():
                generated = getter()
                motion_loaders[name] = generated.batches(batch_size=batch_size, drop_last=True)
                mm_sets[name] = generated.mm_sets()
                mm_sets[GROUND_TRUTH] = generated.gt_mm_sets()
            _say(f, f'==================== Replication {replication} ====================')
            _say(f, f'Time: {datetime.now()}')
            acc, acti, acti2, consistency = score_loaders(eval_wrapper, motion_loaders)
            _say(f, f'Time: {datetime.now()}')
            fid = evaluate_fid(acti)
            for name, v in fid.items():
                _say(f, f'---> [{name}] FID: {v:.4f}')
            fid2 = evaluate_fid(acti2)
            for name, v in fid2.items():
                _say(f, f'---> [{name}] FID2: {v:.4f}')
            _say(f, f'Time: {datetime.now()}')
            diversity = evaluate_diversity(acti, diversity_times, f)
            _say(f, f'Time: {datetime.now()}')
            multimodality = evaluate_multimodality(eval_wrapper, mm_sets, mm_num_times, f)
            _say(f, '!!! DONE !!!')
            for key, per_loader in (('Acc', acc), ('FID', fid), ('FID2', fid2), ('Consistency', consistency),
                                    ('Diversity', diversity), ('MultiModality', multimodality)):
                for name, v in per_loader.items():
                    all_metrics[key].setdefault(name, []).append(v)
        result = OrderedDict()
        for metric_name, per_loader in all_metrics.items():
            _say(f, '========== %s Summary ==========' % metric_name)
            result[metric_name] = OrderedDict()
            for name, values in per_loader.items():
                mean, conf_interval = get_metric_statistics(np.array(values, dtype=np.float64), replication_times)
                result[metric_name][name] = (mean, conf_interval)
                _say(f, f'---> [{name}] Mean: {mean:.4f} CInterval: {conf_interval:.4f}')
        return result
    finally:
        if opened:
            f.close()
