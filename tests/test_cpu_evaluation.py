"""The evaluation protocol on the host: the row rule of the generated sets against the reference's own classes (golden g20,
bit for bit, the number of `random` draws included), the marking rule and the length sort against hand-written expectations,
`evaluation()` on a fake wrapper with prescribed embeddings, and the draw order of the `Text2MotionDatasetV2` mirror."""
import io
import random
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from hig_amd.datasets import Text2MotionDatasetV2, eval_frame_plan, eval_frame_rows, evaluate_matching_score
from hig_amd.datasets.evaluator import mark_multimodality, mm_length_order
from hig_amd.datasets.mul_dataset import frame_indices
from hig_amd.evaluation import (evaluate_diversity, evaluate_multimodality, evaluation, get_metric_statistics,
                                score_loaders)
from hig_amd.utils.metrics import calculate_activation_statistics, calculate_frechet_distance
from oracle import synth_dataset as SD


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the row rule ------------------------------------------------------------------------------------------------------
def test_frame_plan_and_rows_reproduce_the_reference_bit_for_bit(gold):
    g = gold("g20_evaluation.npz")
    lens, mm_lens = g["lens"], g["mm.lens"]
    assert lens.tolist() == [2, 21, 90, 91, 92, 150, 196]
    random.seed(int(g["seed"]))
    shift = eval_frame_plan(lens)                          # the seven EvaluationDataset.__getitem__ calls, in order
    assert shift.dtype == np.int32 and (shift[:3] == 0).all() and shift[3] == 0 and shift[4] == 0
    assert 0 <= shift[5] <= 149 - 91 and 0 <= shift[6] <= 195 - 91
    for i, n in enumerate(lens):
        rows = eval_frame_rows(n, shift[i])
        assert rows.shape == (91,) and rows[0] == 0 and rows.max() < n
        for src, out in (("motion1", "item.motion1"), ("motion2", "item.motion2")):
            assert np.array_equal(bits(g[src][i][rows]), bits(g[out][i])), (i, n)
    assert g["item.length"].tolist() == lens.tolist()
    mm_shift = eval_frame_plan(mm_lens)                    # then MMGeneratedDataset[0]: list order, sorted afterwards
    order = mm_length_order(mm_lens)
    assert np.array_equal(mm_lens[order], g["mm.out_lens"])
    for k, i in enumerate(order):
        rows = eval_frame_rows(mm_lens[i], mm_shift[i])
        assert np.array_equal(bits(g["mm.motion1"][i][rows]), bits(g["mm.out1"][k])), (k, i)
        assert np.array_equal(bits(g["mm.motion2"][i][rows]), bits(g["mm.out2"][k])), (k, i)
    assert random.random() == float(g["next_draw"]), "the plan consumed another number of draws than the reference"


def test_frame_plan_draws_only_where_the_reference_does():
    class Counting:
        def __init__(self):
            self.calls = []

        def randint(self, a, b):
            self.calls.append((a, b))
            return b

    rng = Counting()
    shift = eval_frame_plan([2, 90, 91, 92, 93, 196], rng=rng)
    assert rng.calls == [(0, 0), (0, 0), (0, 1), (0, 104)]         # n = 90 and 91 draw from [0, 0]; n < 90 draws nothing
    assert shift.tolist() == [0, 0, 0, 0, 1, 104]
    rng = Counting()
    assert eval_frame_plan([10, 11, 12, 13], frames=10, rng=rng).tolist() == [0, 0, 0, 1] and len(rng.calls) == 3
    assert eval_frame_rows(2, 0, 10).tolist() == [0] + [1] * 10
    assert eval_frame_rows(10, 0, 10).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9]
    assert eval_frame_rows(11, 0, 10).tolist() == list(range(11))
    assert eval_frame_rows(13, 2, 10).tolist() == [0] + list(range(3, 13))
    for bad in ((13, 3, 10), (13, -1, 10), (1, 0, 10)):
        with pytest.raises(ValueError):
            eval_frame_rows(*bad)


def test_marking_rule_first_three_of_each_class():
    # 3 classes, mm_num_repeats = 2: count <= 2 marks, so each class gets exactly its first three items
    classes = [0, 1, 0, 2, 2, 0, 0, 1, 2, 2, 1, 1, 0, 2, 1]
    assert mark_multimodality(classes, 2) == [0, 1, 2, 3, 4, 5, 7, 8, 10]
    marked = mark_multimodality(classes, 2)
    for c in range(3):
        met = [i for i, k in enumerate(classes) if k == c]
        assert [i for i in marked if classes[i] == c] == met[:3]
    assert mark_multimodality([5, 5], 20) == [0, 1] and mark_multimodality([], 2) == []


def test_mm_length_sort_is_the_reference_argsort_reversed_with_ties():
    lens = [150, 92, 150, 21, 92, 196, 91, 2, 196]
    order = mm_length_order(lens)
    assert order.tolist() == np.argsort(np.array(lens, dtype=int))[::-1].tolist()
    assert [lens[i] for i in order] == sorted(lens, reverse=True)
    assert order.flags["C_CONTIGUOUS"]


# ---- evaluation() on a fake wrapper -------------------------------------------------------------------------------------
D, C = 6, 4


class FakeWrapper:
    """The embeddings are written into the motions: motions1[:, 0, :D] feature, [:, 1, :C] logits, [:, 2, :2] consistency."""

    def get_motion_embeddings(self, motions1, motions2, m_lens, keep_dim=False):
        m = torch.as_tensor(motions1).float()
        return m[:, 1, :C], m[:, 0, :D], m[:, 2, :2]


def fake_motions(n, seed, classes, hit, consistent):
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(n, 3, D)
    m[:, 0] = torch.randn(n, D, generator=g)
    m[:, 1, :C] = torch.randn(n, C, generator=g) * 0.1
    for i in range(n):
        m[i, 1, (classes[i] + (0 if hit[i] else 1)) % C] = 5.0
        m[i, 2, 0 if consistent[i] else 1] = 1.0
    return m


def as_batches(m, classes, bs, drop_last):
    n = len(m)
    stop = n - n % bs if drop_last else n
    return [(torch.tensor(classes[lo:min(lo + bs, stop)]), None, None, m[lo:min(lo + bs, stop)], m[lo:min(lo + bs, stop)],
             torch.full((min(lo + bs, stop) - lo,), 3)) for lo in range(0, stop, bs)]


class FakeSet:
    made = 0

    def __init__(self, n, with_mm=True):
        FakeSet.made += 1
        self.seed = 100 + FakeSet.made
        self.classes = [i % C for i in range(n)]
        self.hit = [i % 3 != 0 for i in range(n)]
        self.consistent = [i % 4 != 1 for i in range(n)]
        self.m = fake_motions(n, self.seed, self.classes, self.hit, self.consistent)
        self.with_mm = with_mm
        self.seen = []

    def batches(self, batch_size=32, drop_last=True, rng=random):
        self.seen.append((batch_size, drop_last))
        return iter(as_batches(self.m, self.classes, batch_size, drop_last))

    def _sets(self, seed):
        if not self.with_mm:
            return iter(())
        return iter([(fake_motions(5, seed + c, [c] * 5, [True] * 5, [True] * 5),) * 2 + (torch.full((5,), 3),) for c in range(3)])

    def mm_sets(self, rng=random):
        return self._sets(self.seed * 7)

    def gt_mm_sets(self, rng=random):
        return self._sets(self.seed * 11)


def gt_loader(n=11, bs=4):
    classes = [i % C for i in range(n)]
    m = fake_motions(n, 7, classes, [i % 5 != 0 for i in range(n)], [True] * n)
    return as_batches(m, classes, bs, False), m


def test_score_loaders_equals_the_unchanged_matching_score():
    gt, _ = gt_loader()
    s = FakeSet(10)
    loaders = lambda: OrderedDict([("ground truth", gt), ("text2motion", s.batches(4, True))])      # noqa: E731
    a = score_loaders(FakeWrapper(), loaders())
    b = evaluate_matching_score(FakeWrapper(), loaders())
    for got, want in zip(a, b):
        assert list(got) == list(want) == ["ground truth", "text2motion"]
        for k in got:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    assert a[1]["ground truth"].shape == (11, D) and a[1]["text2motion"].shape == (8, D)      # not dropped / drop_last
    assert a[2]["text2motion"].shape == (8, C)
    assert a[0]["text2motion"] == sum(s.hit[:8]) / 8 and a[3]["text2motion"] == sum(s.consistent[:8]) / 8


@pytest.mark.parametrize("R", [1, 3])
def test_evaluation_on_prescribed_embeddings(R):
    gt, gt_m = gt_loader()
    sets = []

    def make():
        sets.append(FakeSet(10))
        return sets[-1]

    log = io.StringIO()
    np.random.seed(5)
    res = evaluation(FakeWrapper(), gt, {"text2motion": make}, replication_times=R, diversity_times=6, mm_num_times=3,
                     batch_size=4, log=log)
    assert list(res) == ["Acc", "FID", "FID2", "Consistency", "Diversity", "MultiModality"]
    assert len(sets) == R and all(s.seen == [(4, True)] for s in sets)
    for key in res:
        want = ["text2motion", "ground truth"] if key == "MultiModality" else ["ground truth", "text2motion"]
        assert list(res[key]) == want, key
        for name, (mean, ci) in res[key].items():
            assert np.isfinite(mean) and np.isfinite(ci) and ci >= 0, (key, name)
    # drop_last: 8 of the 10 generated items are scored
    accs = [sum(s.hit[:8]) / 8 for s in sets]
    assert res["Acc"]["text2motion"][0] == np.mean(accs)
    assert res["Acc"]["ground truth"][0] == np.mean([sum(i % 5 != 0 for i in range(11)) / 11] * R)
    assert res["Consistency"]["ground truth"] == (1.0, 0.0)
    # FID per replication, from the prescribed features; conf_interval = 1.96 std / sqrt(R)
    mu, cov = calculate_activation_statistics(gt_m[:, 0].numpy())
    fids = [calculate_frechet_distance(mu, cov, *calculate_activation_statistics(s.m[:8, 0].numpy())) for s in sets]
    mean, ci = res["FID"]["text2motion"]
    assert mean == pytest.approx(np.mean(fids), rel=1e-12) and ci == pytest.approx(1.96 * np.std(fids) / np.sqrt(R), rel=1e-9, abs=1e-15)
    assert res["FID"]["ground truth"][0] == pytest.approx(calculate_frechet_distance(mu, cov, mu, cov), abs=1e-12)
    if R == 1:
        assert all(ci == 0 for key in res for _, ci in res[key].values())
    else:
        assert res["FID"]["text2motion"][1] > 0 and res["Diversity"]["text2motion"][1] > 0
    assert res["MultiModality"]["text2motion"][0] > 0
    # the log carries the reference's lines
    text = log.getvalue()
    assert text.count("==================== Replication") == R and text.count("!!! DONE !!!") == R
    for r in range(R):
        assert "==================== Replication %d ====================" % r in text
    assert "---> [text2motion] FID: %.4f" % fids[0] in text
    assert text.count("---> [ground truth] Diversity: ") == R and text.count("---> [text2motion] Multimodality: ") == R
    for key in res:
        assert "========== %s Summary ==========" % key in text
    mean, ci = res["Acc"]["text2motion"]
    assert "---> [text2motion] Mean: %.4f CInterval: %.4f" % (mean, ci) in text


def test_statistics_and_the_loader_without_sets(tmp_path):
    mean, ci = get_metric_statistics(np.array([1.0, 2.0, 6.0]), 3)
    assert mean == 3.0 and ci == pytest.approx(1.96 * np.std([1.0, 2.0, 6.0]) / np.sqrt(3))
    assert get_metric_statistics(np.array([4.0]), 1) == (4.0, 0.0)
    mm = evaluate_multimodality(FakeWrapper(), OrderedDict([("none", iter(())), ("some", FakeSet(4)._sets(3))]), 3)
    assert mm["none"] == 0 and mm["some"] > 0
    with pytest.raises(AssertionError):       # calculate_diversity needs more samples than pairs, as in the reference
        evaluate_diversity({"x": np.zeros((4, 3))}, 4)
    gt, _ = gt_loader()
    path = tmp_path / "eval.log"
    res = evaluation(FakeWrapper(), gt, {"text2motion": lambda: FakeSet(10, with_mm=False)}, diversity_times=6, mm_num_times=3,
                     batch_size=4, log=str(path))
    assert res["MultiModality"]["text2motion"] == (0.0, 0.0) and res["MultiModality"]["ground truth"] == (0.0, 0.0)
    assert "---> [text2motion] Multimodality: 0.0000" in path.read_text()


# ---- the ground-truth set ------------------------------------------------------------------------------------------------
TABLE = {50: SD.CAPTIONS[0], 51: SD.CAPTIONS[1], 52: SD.CAPTIONS[2], 53: SD.CAPTIONS[3]}


def test_v2_mirror_draws_the_caption_before_the_window(tmp_path):
    opt = SD.write(str(tmp_path))
    mean, std = SD.stats()
    kept = mean.copy(), std.copy()
    ds = Text2MotionDatasetV2(opt, mean, std, opt.split_file, caption_table=TABLE)
    assert np.array_equal(mean, kept[0]) and np.array_equal(std, kept[1]), "the statistics were adjusted"
    names = [n for n, f in sorted(SD.SEQS, key=lambda s: s[1]) if 20 <= f + 1 < 200]
    assert list(ds.name_list) == names and len(ds) == len(names) and ds.pointer == 0
    first_caps = [c[0] for c in SD.CAPTIONS]
    random.seed(99)
    items = [ds[i] for i in range(len(ds))]
    after = random.random()
    random.seed(99)
    for name, (class_id, cap1, cap2, m1, m2, m_len) in zip(names, items):
        d = ds.data_dict[name]
        caps = random.choice(d["text"])["captions"]                  # first draw: the caption
        frame_ix = frame_indices(d["motion"].shape[1] - 1)            # then the window (a draw only for >= 90 frames)
        assert (cap1, cap2) == tuple(caps) and class_id == first_caps.index(caps[0])
        assert m_len == d["length"] == d["motion"].shape[1] and m1.shape == m2.shape == (91, SD.F)
        raw1, raw2 = d["motion"][0][frame_ix], d["motion"][1][frame_ix]
        for raw, got in ((raw1, m1), (raw2, m2)):
            assert np.array_equal(got[1:], (raw[1:] - ds.mean) / ds.std)
            assert np.array_equal(got[0, :4], (raw[0, :4] - ds.init_mean) / ds.init_std) and np.array_equal(got[0, 4:], raw[0, 4:])
    assert random.random() == after
    # several captions and a long clip exist, so the order of the two draws matters in this data
    assert any(len(ds.data_dict[n]["text"]) > 1 and ds.data_dict[n]["motion"].shape[1] - 1 > 91 for n in names)
    opt_id = types.SimpleNamespace(**dict(vars(opt), cap_id=True))
    item = Text2MotionDatasetV2(opt_id, mean, std, opt.split_file, caption_table=TABLE)[0]
    assert isinstance(item[1], list) and isinstance(item[1][0], int) and len(item) == 6


# ---- hig_eval_pairs_build's host check (returns before any HIP call, so it runs here) -----------------------------------
def test_pairs_build_refuses_invalid_plans_without_a_device():
    import ctypes as C
    from hig_amd import _lib
    L = _lib.lib()
    F, W = 7, 90
    off = np.array([0, 196 * F], dtype=np.int64)
    floats = 2 * 196 * F
    fake = C.c_void_p(4096)       # never dereferenced: every call below is refused, or N = 0

    def call(m_len, shift, N=1, off=off, floats=floats, F_out=3, T_out=W + 1):
        m_len, shift = np.array([m_len], dtype=np.int32), np.array([shift], dtype=np.int32)
        hp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        return L.hig_eval_pairs_build(fake, fake, fake, fake, hp(off), hp(m_len), hp(shift), floats, N, F, F_out, T_out, fake, None)

    for m_len, shift, word in ((150, 60, "window"), (91, 1, "window"), (1, 0, "m_len"), (0, 0, "m_len"), (150, -1, "negative"),
                               (89, -1, "negative")):
        assert call(m_len, shift) == -1 and word in _lib.last_error(), (m_len, shift, _lib.last_error())
    assert call(150, 0, off=np.array([0, floats - 149 * F], dtype=np.int64)) == -1 and "outside" in _lib.last_error()
    assert call(150, 0, off=np.array([-1, 0], dtype=np.int64)) == -1
    assert call(150, 0, F_out=8) == -1 and call(150, 0, F_out=0) == -1 and call(150, 0, T_out=1) == -1
    assert call(89, 0, T_out=2 ** 31 - 1) == -1      # (no overflow on the way to the grid size)
    assert call(150, 0, N=-1) == -1 and call(150, 0, N=40000) == -1
    assert call(150, 0, N=0) == 0
