"""The evaluation protocol on the MI355X: `hig_eval_pairs_build` against `eval_frame_rows` applied to the same bytes (bit for
bit, NaN beyond every m_len, guard rows around the output, an unaligned base pointer), its host-side refusals,
`GeneratedMotionSet`'s device route against its host route, and `evaluation()` end to end on the two-person `tiny2` model."""
import ctypes as C
import random
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hig_amd  # noqa: E402
from hig_amd import _lib  # noqa: E402
from hig_amd.datasets import (EvaluatorModelWrapper, GeneratedMotionSet, eval_frame_plan, eval_frame_rows,  # noqa: E402
                              evaluate_matching_score)
from hig_amd.datasets.evaluator import mm_length_order  # noqa: E402
from hig_amd.evaluation import evaluation, score_loaders  # noqa: E402
from hig_amd.utils.metrics import calculate_activation_statistics, calculate_frechet_distance  # noqa: E402
from oracle import fill  # noqa: E402
from oracle.eval_models_ref import EVAL_CASES  # noqa: E402
from test_gpu_interaction import _trainer as _mul_trainer  # noqa: E402
from test_gpu_interaction import build as build_pair  # noqa: E402

DEV = "cuda"
EINVAL = -1
SENTINEL = -12345.5
LENS90 = [2, 21, 90, 91, 92, 150, 196]
LENS10 = [2, 10, 11, 12, 13, 30]


def bits(t):
    return t.contiguous().view(torch.int32)


def hp(a):
    return a.ctypes.data_as(C.c_void_p)


class Source:
    """N pairs laid out as `generate` leaves them: two chunks of different T (92 and 196 rows per person-sample), person 1 of a
    chunk's pairs, then person 2.  One flat host buffer, NaN wherever no motion has a row (also at and beyond every m_len)."""

    def __init__(self, lens, F_in, chunk_T=(92, 196), seed=0):
        g = torch.Generator().manual_seed(seed)
        self.lens, self.F = list(lens), F_in
        where = [0 if n <= chunk_T[0] else 1 for n in lens]
        count = [where.count(0), where.count(1)]
        start = [0, 2 * count[0] * chunk_T[0] * F_in]
        self.floats = start[1] + 2 * count[1] * chunk_T[1] * F_in
        self.flat = torch.full((self.floats,), float("nan"))
        seen, off = [0, 0], np.zeros((2, len(lens)), dtype=np.int64)
        for i, n in enumerate(lens):
            c = where[i]
            for p in range(2):
                off[p, i] = start[c] + ((p * count[c] + seen[c]) * chunk_T[c]) * F_in
                self.flat[off[p, i]: off[p, i] + n * F_in] = torch.randn(n * F_in, generator=g)
            seen[c] += 1
        self.off = np.ascontiguousarray(off.reshape(-1))
        self.m_len = np.asarray(lens, dtype=np.int32)

    def motion(self, p, i):
        o = int(self.off[p * len(self.lens) + i])
        return self.flat[o: o + self.lens[i] * self.F].view(self.lens[i], self.F)

    def expected(self, shift, frames, F_out):
        rows = [eval_frame_rows(n, s, frames) for n, s in zip(self.lens, shift)]
        return torch.stack([self.motion(p, i)[torch.from_numpy(rows[i])][:, :F_out] for p in range(2) for i in range(len(self.lens))])


def launch(src, shift, frames, F_out, lead=0, host=None, dev=None, out=None):
    """One call on a guarded output.  lead: floats the source sits past a 16-byte boundary.  host / dev: overrides of the host /
    device copies of (off, m_len, shift).  -> (rc, buffer incl. guard rows, rows)."""
    N, T_out = len(src.lens), frames + 1
    base = torch.zeros(lead + src.floats)
    base[lead:] = src.flat
    base_d = base.to(DEV)
    shift = np.asarray(shift, dtype=np.int32)
    h = [src.off, src.m_len, shift] if host is None else [np.ascontiguousarray(a) for a in host]
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in ((src.off, src.m_len, shift) if dev is None else dev)]
    rows = 2 * N * T_out
    buf = torch.full((rows + 2, F_out), SENTINEL, device=DEV) if out is None else out
    rc = _lib.lib().hig_eval_pairs_build(
        C.c_void_p(base_d.data_ptr() + 4 * lead), _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), hp(h[0]), hp(h[1]), hp(h[2]),
        src.floats, N, src.F, F_out, T_out, C.c_void_p(buf.data_ptr() + 4 * F_out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, buf.cpu(), rows


def plans(lens, frames, seed):
    """The drawn plan and the largest shift the entry accepts (n - frames: one past what the reference ever draws)."""
    return [eval_frame_plan(lens, frames, random.Random(seed)),
            np.array([max(0, n - 1 - frames) for n in lens], dtype=np.int32)]


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F_in,F_out", [(263, 259), (263, 263), (7, 3), (12, 12)])
@pytest.mark.parametrize("frames,lens", [(90, LENS90), (10, LENS10)])
def test_eval_pairs_build_is_eval_frame_rows_bit_for_bit(frames, lens, F_in, F_out):
    src = Source(lens, F_in, seed=F_in + frames)
    for shift in plans(lens, frames, 3):
        want = src.expected(shift, frames, F_out)
        assert torch.isfinite(want).all()
        outs = []
        for lead in (0, 1):       # a base pointer one float past the aligned one: the same bytes
            rc, buf, rows = launch(src, shift, frames, F_out, lead=lead)
            _lib.check(rc)
            assert (buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all(), "a store landed in a guard row"
            got = buf[1:-1].view(2 * len(lens), frames + 1, F_out)
            assert torch.isfinite(got).all(), "a row at or beyond m_len was read, or an element was not written"
            assert torch.equal(bits(got), bits(want)), (shift.tolist(), lead)
            outs.append(got)
        assert torch.equal(bits(outs[0]), bits(outs[1]))
    assert (plans(lens, frames, 3)[1] > 0).any()


def test_eval_pairs_build_more_than_one_grid_row_of_pairs():
    """40 pairs (80 person-samples, what a batch of 32 and more looks like), all lengths round the threshold."""
    lens = [(2, 9, 10, 11, 12, 25, 92)[i % 7] for i in range(40)]
    src = Source(lens, 12, seed=1)
    shift = eval_frame_plan(lens, 10, random.Random(4))
    rc, buf, rows = launch(src, shift, 10, 8)
    _lib.check(rc)
    assert (buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all()
    assert torch.equal(bits(buf[1:-1].view(80, 11, 8)), bits(src.expected(shift, 10, 8)))


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------
def test_invalid_plans_are_refused_on_the_host_before_any_launch():
    """Every invalid entry is built so that its rows would still lie inside the source if the kernel ran: the motions physically
    have 196 rows, the plans declare fewer."""
    lens = [196, 196, 196]
    src = Source(lens, 7, seed=2)
    assert torch.isfinite(src.flat).all()
    good_len, good_shift = np.array([150, 150, 150], dtype=np.int32), np.array([5, 0, 59], dtype=np.int32)
    src.m_len = good_len
    rc, buf, _ = launch(src, good_shift, 90, 3)
    _lib.check(rc)
    assert not (buf[1:-1] == SENTINEL).any()
    bad = [("shift + W > n", good_len, [5, 0, 60], "window"),                  # rows up to 150 of 196
           ("shift + W > n at n = W", [150, 91, 150], [5, 1, 0], "window"),   # rows up to 91
           ("m_len < 2", [150, 150, 1], [5, 0, 0], "m_len"),                   # the kernel would read row 0 only
           ("negative shift", good_len, [-1, 0, 0], "negative")]               # rows from 0
    for what, m_len, shift, word in bad:
        m_len, shift = np.asarray(m_len, dtype=np.int32), np.asarray(shift, dtype=np.int32)
        rc, buf, _ = launch(src, shift, 90, 3, host=(src.off, m_len, shift), dev=(src.off, m_len, shift))
        assert rc == EINVAL, "%s: returned %d" % (what, rc)
        assert word in _lib.last_error(), (what, _lib.last_error())
        assert (buf == SENTINEL).all(), "%s: a refused call wrote" % what
    # a motion outside the extent the caller named; sizes; null pointers -- the device copies stay valid throughout
    off = src.off.copy()
    off[4] = src.floats - 149 * 7
    for what, kw in (("offset past src_floats", dict(host=(off, good_len, good_shift))),
                     ("negative offset", dict(host=(np.where(np.arange(6) == 1, -7, src.off), good_len, good_shift)))):
        rc, buf, _ = launch(src, good_shift, 90, 3, **kw)
        assert rc == EINVAL and (buf == SENTINEL).all(), what
    rc, buf, _ = launch(src, good_shift, 90, 8)          # F_out > F_in (the guarded buffer is sized for it)
    assert rc == EINVAL and (buf == SENTINEL).all()
    L = _lib.lib()
    assert L.hig_eval_pairs_build(None, None, None, None, None, None, None, 0, 0, 7, 3, 91, None, _lib.stream_ptr()) == 0   # N = 0
    assert L.hig_eval_pairs_build(None, None, None, None, None, None, None, 0, 2, 7, 3, 91, None, _lib.stream_ptr()) == EINVAL
    assert L.hig_eval_pairs_build(None, None, None, None, None, None, None, 0, -1, 7, 3, 91, None, _lib.stream_ptr()) == EINVAL
    torch.cuda.synchronize()


# ---- 3. / 4. the generated set and the run -------------------------------------------------------------------------------
FRAMES = 10
PAIR_LENS = [20, 5, 11, 12, 2, 16, 10, 13]          # n = 19, 4, 10, 11, 1, 15, 9, 12 round the threshold of 10 frames
PAIR_CLASS = [0, 1, 0, 1, 2, 0, 1, 2]
CAPS1 = ["one pushes the other", "two people hug", "a person hands a cup over", "they shake hands"]
CAPS2 = ["one is pushed by the other", "two people hug", "a person receives a cup", "they shake hands"]


class Chunked:
    """The trainer with `generate` cut into chunks of 5 pairs, so that the set holds chunks of different T (20 and 11 in the order used below)."""

    def __init__(self, trainer):
        self.trainer, self.T = trainer, []

    def eval_mode(self):
        self.trainer.eval_mode()

    def to(self, device):
        self.trainer.to(device)

    def generate(self, caption1, caption2, m_lens, dim_pose):
        out = self.trainer.generate(caption1, caption2, m_lens, dim_pose, batch_size=5)
        self.T = [o[0].shape[0] for o in out]
        return out


@pytest.fixture(scope="module")
def world():
    c = fill.ICASES["tiny2"]
    F = c["F"]
    model = build_pair(c).eval()
    trainer = _mul_trainer(c, model)
    trainer.set_sampler(steps=2, method="ddim")
    e = EVAL_CASES["tiny"]
    kw = dict(input_feats=F - 4, num_frames=e["num_frames"], latent_dim=e["d"], ff_size=e["ff"], num_layers=e["L"], num_heads=e["H"])
    enc, con = hig_amd.MotionEncoder(**kw), hig_amd.MotionConsistencyEvalModel(**kw)
    for m in (enc, con):
        m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    wrapper = EvaluatorModelWrapper(types.SimpleNamespace(dataset_name="ntu_mul", device=torch.device(DEV)), models=(enc, con))
    gt = [(PAIR_CLASS[i], CAPS1[i % 4], CAPS2[i % 4], (fill.tensor_for("eval.gt1.%d" % i, (FRAMES + 1, F)) * 10).numpy(),
           (fill.tensor_for("eval.gt2.%d" % i, (FRAMES + 1, F)) * 10).numpy(), PAIR_LENS[i]) for i in range(8)]
    opt = types.SimpleNamespace(device=torch.device(DEV), dim_pose=F, cap_id=False)
    return types.SimpleNamespace(opt=opt, trainer=Chunked(trainer), wrapper=wrapper, gt=gt, F=F)


def make_set(w, seed=11):
    torch.manual_seed(seed)
    return GeneratedMotionSet(w.opt, w.trainer, w.gt, 1, frames=FRAMES, order=[3, 0, 5, 1, 7, 2, 6, 4])


def gt_batches(w, bs=4):
    out = []
    for lo in range(0, len(w.gt), bs):
        items = w.gt[lo:lo + bs]
        out.append((torch.tensor([it[0] for it in items]), [it[1] for it in items], [it[2] for it in items],
                    torch.from_numpy(np.stack([it[3] for it in items])), torch.from_numpy(np.stack([it[4] for it in items])),
                    torch.tensor([it[5] for it in items])))
    return out


def test_generated_set_device_route_equals_host_route(world):
    w = world
    s = make_set(w)
    order = [3, 0, 5, 1, 7, 2, 6, 4]
    assert len(s) == 8 and s.lengths.tolist() == [PAIR_LENS[i] for i in order]
    assert sorted(set(w.trainer.T)) == [11, 20], "the set should hold chunks of different T"
    assert s.mm_indices == [0, 1, 2, 3, 4, 7]          # classes 1 0 0 1 2 0 1 2: the first two of each
    assert all(m.is_cuda for pair in s.motions for m in pair)
    for bs, drop in ((3, True), (3, False), (8, True)):
        random.seed(21)
        dev = list(s.batches(bs, drop))
        after = random.random()
        random.seed(21)
        host = list(s.host_batches(bs, drop))
        assert random.random() == after, "the two routes consume different numbers of draws"
        assert len(dev) == len(host) == (8 // bs if drop else -(-8 // bs))
        for a, b in zip(dev, host):
            assert a[3].is_cuda and a[3].shape == b[3].shape == (len(b[0]), FRAMES + 1, w.F)
            assert torch.equal(a[0].cpu(), b[0]) and a[1] == b[1] and a[2] == b[2] and torch.equal(a[5].cpu(), b[5])
            assert torch.isfinite(a[3]).all() and torch.isfinite(a[4]).all()
            assert torch.equal(bits(a[3].cpu()), bits(b[3])) and torch.equal(bits(a[4].cpu()), bits(b[4]))
            ea, eb = w.wrapper.get_motion_embeddings(a[3], a[4], a[5]), w.wrapper.get_motion_embeddings(b[3], b[4], b[5])
            for x, y in zip(ea, eb):
                assert torch.equal(bits(x.cpu()), bits(y.cpu())), "same bytes, same wrapper, other embeddings"
    random.seed(22)
    dev = list(s.mm_sets())
    random.seed(22)
    host = list(s.host_mm_sets())
    assert len(dev) == len(host) == 3
    for (a1, a2, al), (b1, b2, bl) in zip(dev, host):
        assert torch.equal(al.cpu(), bl) and bl.tolist() == sorted(bl.tolist(), reverse=True) and len(bl) == 2
        assert torch.equal(bits(a1.cpu()), bits(b1)) and torch.equal(bits(a2.cpu()), bits(b2))
    # the sort is the reference's, applied after the draws: class 0 holds the items met at 1, 2 (lengths 20, 16)
    lens0 = s.lengths[[1, 2]]
    assert host[0][2].tolist() == lens0[mm_length_order(lens0)].tolist()
    gt_sets = list(s.gt_mm_sets())
    assert len(gt_sets) == 3 and all(m1.shape == (2, FRAMES + 1, w.F) and not m1.is_cuda for m1, _, _ in gt_sets)
    assert all(max(l.tolist()) <= FRAMES + 1 for _, _, l in gt_sets)


def test_evaluation_runs_end_to_end(world, tmp_path):
    w = world
    made, states = [], []

    def make():
        states.append(random.getstate())
        made.append(make_set(w, seed=30 + len(made)))
        return made[-1]

    gt = gt_batches(w)
    random.seed(5)
    np.random.seed(5)
    res = evaluation(w.wrapper, gt, {"text2motion": make}, replication_times=2, diversity_times=4, mm_num_times=1, batch_size=4,
                     log=str(tmp_path / "eval.log"))
    assert list(res) == ["Acc", "FID", "FID2", "Consistency", "Diversity", "MultiModality"] and len(made) == 2
    for key in res:
        assert set(res[key]) == {"ground truth", "text2motion"}
        for name, (mean, ci) in res[key].items():
            print("EVAL %s [%s] mean %.6g conf %.6g" % (key, name, mean, ci))
            assert np.isfinite(mean) and np.isfinite(ci), (key, name)
    _, acti, _, _ = evaluate_matching_score(w.wrapper, {"ground truth": gt})
    mu, cov = calculate_activation_statistics(acti["ground truth"])
    assert res["FID"]["ground truth"][0] == calculate_frechet_distance(mu, cov, mu, cov) and res["FID"]["ground truth"][1] == 0
    accs, cons = [], []
    for state, s in zip(states, made):
        random.setstate(state)
        acc, _, _, con = evaluate_matching_score(w.wrapper, {"text2motion": s.host_batches(4, True)})
        accs.append(acc["text2motion"])
        cons.append(con["text2motion"])
    assert res["Acc"]["text2motion"][0] == np.mean(accs) and res["Consistency"]["text2motion"][0] == np.mean(cons)
    acc, _, _, con = score_loaders(w.wrapper, {"ground truth": gt})
    gacc, _, _, gcon = evaluate_matching_score(w.wrapper, {"ground truth": gt})
    assert acc["ground truth"] == gacc["ground truth"] and con["ground truth"] == gcon["ground truth"]
    text = (tmp_path / "eval.log").read_text()
    assert text.count("---> [text2motion] FID: ") == 2 and "========== MultiModality Summary ==========" in text
