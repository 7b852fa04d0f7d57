"""The caption bank on the MI355X: the three row kernels of csrc/textrows.hip bit for bit, the bank behind
MotionTransformer.encode_text and the fused / captured training steps (models/caption_bank.py), and the gate that lets the text
head run once per distinct caption.

Dedup gate (the project's form): per parameter, the rel-L2 distance of the deduplicated route from the fp64 stock-torch text head
<= max(1e-6, 4 x the distance of the parent's route -- the head on every row).  The key third of every in_proj_bias is left out
(its gradient is rounding noise around an exact zero, tests/test_gpu_eval_train.py)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_bounds as CB  # noqa: E402
import hig_amd  # noqa: E402
from hig_amd import _lib  # noqa: E402
from hig_amd.models import caption_bank as CBK  # noqa: E402
from hig_amd.models import clip_text as CT  # noqa: E402
from hig_amd.models import stub_clip  # noqa: E402
from oracle import fill  # noqa: E402
from test_gpu_denoiser import make_diffusion, rel  # noqa: E402

DEV = "cuda"
N = 77
GUARD = 64              # floats either side of an output
PATTERN = 0x7FC0BEEF    # a NaN the kernels never produce


def S():
    return _lib.stream_ptr()


def bits(t):
    return t.contiguous().view(torch.int32)


class Band:
    """`n` floats at `offset` floats past a 16-byte boundary, guard bands of GUARD floats either side."""

    def __init__(self, n, offset=0):
        self.n, self.lo = n, GUARD + offset
        self.buf = torch.full((GUARD + offset + n + GUARD + 4,), PATTERN, dtype=torch.int32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.out = self.buf[self.lo:self.lo + n].view(torch.float32)
        assert self.out.data_ptr() % 16 == (4 * offset) % 16

    def ptr(self):
        return C.c_void_p(self.out.data_ptr())

    def intact(self):
        return bool((self.buf[:self.lo] == PATTERN).all() and (self.buf[self.lo + self.n:] == PATTERN).all())

    def written(self):
        return bool((self.buf[self.lo:self.lo + self.n] != PATTERN).all())


def placed(t, offset):
    """A copy of the fp32 tensor `t` whose base is `offset` floats past a 16-byte boundary."""
    raw = torch.empty(t.numel() + 8, device=DEV)
    view = raw[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ---- gather ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_floats", [4, 7, 1028])
def test_rows_gather_is_bit_equal_to_indexing_and_an_index_out_of_range_gives_nan(row_floats):
    n_src, n_out = 3, 5
    g = torch.Generator().manual_seed(row_floats)
    src = torch.randn(n_src, row_floats, generator=g)
    eot_src = torch.tensor([11, 22, 33], dtype=torch.int64, device=DEV)
    for idx in ([2, 0, 2, 1, 0], [2, 3, -1, 0, 1]):
        live = torch.tensor([0 <= i < n_src for i in idx])
        idx_dev = i32(idx)
        want = src[[i if 0 <= i < n_src else 0 for i in idx]]
        for off_src, off_dst in ((0, 0), (1, 1), (0, 1), (1, 0)):        # an unaligned base takes the element-wise path
            s = placed(src.to(DEV), off_src)
            out = Band(n_out * row_floats, off_dst)
            _lib.check(_lib.lib().hig_rows_gather_f32(C.c_void_p(s.data_ptr()), n_src, _lib.ptr(idx_dev), n_out, row_floats,
                                                     out.ptr(), S()))
            eot = torch.full((n_out + 2,), -7, dtype=torch.int64, device=DEV)
            both = Band(n_out * row_floats, off_dst)
            _lib.check(_lib.lib().hig_caption_gather(C.c_void_p(s.data_ptr()), _lib.ptr(eot_src), n_src, _lib.ptr(idx_dev), n_out,
                                                    row_floats, both.ptr(), C.c_void_p(eot.data_ptr() + 8), S()))
            torch.cuda.synchronize()
            for what, b in (("hig_rows_gather_f32", out), ("hig_caption_gather", both)):
                assert b.intact(), "%s: a store landed in a guard band" % what
                assert b.written(), "%s: not every element was written" % what
                got = b.out.view(n_out, row_floats).cpu()
                assert torch.equal(bits(got[live]), bits(want[live])), (what, off_src, off_dst)
                assert torch.isnan(got[~live]).all() and not torch.isnan(got[live]).any()
            assert eot.tolist() == [-7] + [int(eot_src[i]) if 0 <= i < n_src else 0 for i in idx] + [-7]


# ---- segment sum -----------------------------------------------------------------------------------------------------------
def list_order_sum(src, order, seg):
    """float32 sums taken in list order, starting from the first member; an empty segment is +0.0."""
    out = np.zeros((len(seg) - 1, src.shape[1]), dtype=np.float32)
    for u in range(len(seg) - 1):
        for k, j in enumerate(range(seg[u], seg[u + 1])):
            out[u] = src[order[j]] if k == 0 else (out[u] + src[order[j]]).astype(np.float32)
    return out


@pytest.mark.parametrize("row_floats", [4, 7, 1028])
def test_segment_sum_is_the_float32_sum_in_list_order(row_floats):
    n_src, order, seg = 7, [5, 0, 3, 2, 6, 1], [0, 3, 3, 4, 6]            # sizes 3, 0, 1, 2; row 4 is in no list
    g = torch.Generator().manual_seed(100 + row_floats)
    src = torch.randn(n_src, row_floats, generator=g) * 10.0 ** (torch.rand(n_src, row_floats, generator=g) * 8 - 4)
    src[4] = float("nan")
    want = list_order_sum(src.numpy(), order, seg)
    assert np.isfinite(want).all()
    if row_floats == 1028:                                                # magnitudes 1e-4 .. 1e4: the order matters
        assert not np.array_equal(want[0], list_order_sum(src.numpy(), [3, 0, 5, 2, 6, 1], seg)[0])
    results, order_dev, seg_dev = [], i32(order), i32(seg)
    for off_src, off_dst in ((0, 0), (1, 1), (1, 0)):
        s = placed(src.to(DEV), off_src)
        out = Band((len(seg) - 1) * row_floats, off_dst)
        _lib.check(_lib.lib().hig_rows_segment_sum_f32(C.c_void_p(s.data_ptr()), n_src, _lib.ptr(order_dev), _lib.ptr(seg_dev),
                                                      len(seg) - 1, row_floats, out.ptr(), S()))
        torch.cuda.synchronize()
        assert out.intact(), "hig_rows_segment_sum_f32: a store landed in a guard band"
        got = out.out.view(len(seg) - 1, row_floats).cpu()
        assert not torch.isnan(got).any(), "the row no list names was read"
        assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32)), (off_src, off_dst)
        assert (bits(got[1]) == 0).all()                                  # the empty segment: +0.0, not -0.0
        results.append(got)
    assert all(torch.equal(bits(r), bits(results[0])) for r in results)


def test_segment_sum_over_many_rows_and_more_than_one_workgroup_per_segment():
    """1 300 rows over 44 + 20 segments at the width of dxf_out (77 x 256): every work split the launcher can choose."""
    rows, U, U_pad, width = 1300, 44, 64, 77 * 256
    g = torch.Generator().manual_seed(9)
    inv = torch.randint(0, U, (rows,), generator=g)
    src = torch.randn(rows, 8, generator=g).repeat(1, width // 8)          # (cheap to sum on the host)
    order = torch.argsort(inv, stable=True).tolist()
    counts = torch.bincount(inv, minlength=U_pad).tolist()
    seg = [0]
    for c in counts:
        seg.append(seg[-1] + c)
    want = list_order_sum(src[:, :8].numpy(), order, seg)
    order_dev, seg_dev, inv_dev = i32(order), i32(seg), i32(inv.tolist())
    out = CBK.segment_sum_rows(src.to(DEV), order_dev, seg_dev, U_pad)
    back = CBK.expand_rows(out, inv_dev, rows)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.int32), np.tile(want, (1, width // 8)).view(np.int32))
    assert torch.equal(back, out[inv.to(DEV)])


# ---- the bank ---------------------------------------------------------------------------------------------------------------
TINY = dict(B=4, T=16, F=12, d=64, H=8, L=2, ff=128, Lt=64, num_frames=16)
CAPS = ["a person waves the right hand", "two people shake hands and then one of them walks slowly away to the left", "jump",
        "one pushes the other", "a person bows", "kick", "a person sits down", "two people hug", "run", "a person claps",
        "one person points at the other"]


@functools.lru_cache(maxsize=None)
def tower_weights():
    return CB.tower_weights(512, 8, 2, N, stub_clip.VOCAB, seed=11)


def clip_model(kind):
    return stub_clip.StubCLIP() if kind == "stub" else CT.load_text_tower(tower_weights())


def build(kind="stub", cls=None, c=TINY, **kw):
    cls = cls or hig_amd.MotionTransformer
    m = cls(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"], num_layers=c["L"], num_heads=c["H"],
            text_latent_dim=c["Lt"], text_num_heads=4, text_ff_size=128, num_text_layers=2, clip_model=clip_model(kind),
            clip_tokenize=stub_clip.tokenize, **kw)
    m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    return m.to(DEV)


def trainer(m, cls=None, **kw):
    args = types.SimpleNamespace(device=torch.device(DEV), diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=4, num_epochs=1,
                                 log_every=50, save_latest=500, save_every_e=5, is_continue=False, model_dir="/tmp", **kw)
    return (cls or hig_amd.DDPMTrainer)(args, m)


class TowerCalls:
    """Counts what runs the tower and the tokenizer, whichever route `_clip_features` takes: ln_final's forward (torch ops),
    clip_text.tower_forward (the native route) and the tokenizer.  Install it before the bank's first request: a changed
    tokenizer empties the bank."""

    def __init__(self, m, monkeypatch):
        self.tower = self.tokenizer = 0
        m.clip.ln_final.register_forward_hook(lambda *_: self._count("tower"))
        real_forward, real_tok = CT.tower_forward, m._clip_tokenize
        monkeypatch.setattr(CT, "tower_forward", lambda *a, **k: (self._count("tower"), real_forward(*a, **k))[1])
        m._clip_tokenize = lambda *a, **k: (self._count("tokenizer"), real_tok(*a, **k))[1]

    def _count(self, what):
        setattr(self, what, getattr(self, what) + 1)


@pytest.mark.parametrize("kind", ["stub", "native"])
def test_every_slot_holds_the_tower_output_of_its_fill_chunk_and_a_repeat_never_runs_the_tower(kind, monkeypatch):
    m = build(kind, caption_bank=32).eval()
    bank = m.caption_bank
    calls = TowerCalls(m, monkeypatch)
    tokens = stub_clip.tokenize(CAPS[:2], truncate=True).to(DEV)
    assert (m._clip_native_table(tokens) is not None) == (kind == "native")
    with torch.no_grad():
        first = m.encode_text(CAPS + CAPS[:3], DEV)
    assert calls.tower == 2 and calls.tokenizer == 2 and bank.stats["tower_calls"] == 2 and bank.stats["tokenizer_calls"] == 2
    assert bank.stats["misses"] == len(CAPS) and len(bank) == len(CAPS)
    for c in CAPS:
        chunk, i = bank.chunk_of[c]
        assert len(chunk) == CBK.FILL_CHUNK
        tok, x = m._clip_features(list(chunk), DEV)
        assert torch.equal(bits(bank.feat[bank.slots[c]]), bits(x.permute(1, 0, 2)[i])), c
        assert int(bank.eot[bank.slots[c]]) == int(tok[i].argmax())
    # the same captions again, in another order and with other duplicates: no tower, no tokenizer
    again = [CAPS[i] for i in (7, 7, 2, 10, 0, 2, 5, 1, 3, 4, 6, 8, 9, 9, 9)]
    stats, seen = dict(bank.stats), (calls.tower, calls.tokenizer)
    with torch.no_grad():
        xp, xo = m.encode_text(again, DEV)
    assert (calls.tower, calls.tokenizer) == seen
    assert bank.stats["tower_calls"] == stats["tower_calls"] and bank.stats["tokenizer_calls"] == stats["tokenizer_calls"]
    assert bank.stats["hits"] == stats["hits"] + len(again) and bank.stats["misses"] == stats["misses"]
    for r, c in enumerate(again):                                          # every row got its own caption's embedding
        assert rel(xp[r], first[0][CAPS.index(c)]) < 2e-5 and rel(xo[r], first[1][CAPS.index(c)]) < 2e-5


@pytest.mark.parametrize("kind", ["stub", "native"])
def test_a_row_is_the_same_bits_whichever_request_first_met_it_and_overflow_is_counted(kind):
    m = build(kind).eval()
    one, two = CBK.CaptionBank(m, 8), CBK.CaptionBank(m, 8)
    one.batch(CAPS[:3], DEV)
    one.batch(CAPS[3:4], DEV)
    two.batch(CAPS[3:4], DEV)
    assert one.slots[CAPS[3]] == 3 and two.slots[CAPS[3]] == 0
    assert torch.equal(bits(one.feat[3]), bits(two.feat[0])) and int(one.eot[3]) == int(two.eot[0])
    small = CBK.CaptionBank(m, 2)
    cb = small.batch([CAPS[0], CAPS[1], CAPS[2], CAPS[3], CAPS[2]], DEV)
    assert cb.slot.tolist() == [0, 1, 2, 3, 2] and small.stats["overflow_rows"] == 3 and len(small) == 2
    clip_out, eot = small.gather(cb.slot, cb.rows)
    tok, x = m._clip_features(CAPS[:4] + [""] * 4, DEV)
    assert torch.equal(bits(clip_out), bits(x.permute(1, 0, 2)[[0, 1, 2, 3, 2]]))
    assert torch.equal(eot, tok.argmax(-1)[[0, 1, 2, 3, 2]])


def test_the_bank_is_empty_again_after_the_tower_may_have_changed():
    m = build("native", caption_bank=8).eval()
    bank = m.caption_bank
    for change in ("param", "to", "load"):
        bank.batch(CAPS[:3], DEV)
        assert len(bank) == 3
        calls = bank.stats["tower_calls"]
        if change == "param":
            with torch.no_grad():
                m.clip.ln_final.bias.add_(0.5)
        elif change == "to":
            m.to(DEV)
            assert len(bank) == 0
        else:
            m.load_state_dict(m.state_dict())
            assert len(bank) == 0
        cb = bank.batch(CAPS[:1], DEV)
        assert len(bank) == 1 and bank.stats["tower_calls"] == calls + 1, change
        tok, x = m._clip_features(CAPS[:1] + [""] * 7, DEV)
        assert torch.equal(bits(bank.gather(cb.slot, 1)[0][0]), bits(x[:, 0]))


# ---- plumbing: exact by construction ------------------------------------------------------------------------------------------
def step_inputs(rows, T, F, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = (torch.randn(rows, T, F, generator=g) * 3).to(DEV)
    noise = torch.randn(rows, T, F, generator=g).to(DEV)
    return x0, noise


def state_of(m, tr):
    st = tr.fused_state()
    out = {k: v.detach().clone() for k, v in m.state_dict().items() if not k.startswith("clip.")}
    out["adam.m"], out["adam.v"] = st["m"].clone(), st["v"].clone()
    return out


def assert_same_state(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), "%s: %s differs" % (what, k)


def test_fused_step_with_a_caption_batch_equals_the_step_fed_the_banks_rows():
    c = TINY
    caps = [CAPS[0], CAPS[1], CAPS[0], CAPS[2]]
    x0, noise = step_inputs(c["B"], c["T"], c["F"], 1)
    t, length = torch.tensor([3, 987, 500, 40]).to(DEV), torch.tensor([16, 9, 1, 12]).to(DEV)
    m1, m2 = build(caption_bank=8, text_dedup=False).train(), build().train()
    t1, t2 = trainer(m1), trainer(m2)
    bank = m1.caption_bank
    cb = bank.batch(caps, DEV)
    l1 = t1.train_step_fused(x0, t, length, noise=noise, caption_batch=cb).clone()
    sl = cb.slot.long()
    l2 = t2.train_step_fused(x0, t, length, noise=noise, clip_out=bank.feat[sl], eot=bank.eot[sl]).clone()
    assert torch.equal(l1, l2) and torch.isfinite(l1).all()
    assert_same_state(state_of(m1, t1), state_of(m2, t2), "single-person step")
    with pytest.raises(ValueError, match="exclusive"):
        t1.train_step_fused(x0, t, length, noise=noise, caption_batch=cb, clip_out=bank.feat[sl], eot=bank.eot[sl])
    with pytest.raises(RuntimeError, match="caption bank"):
        t2.train_step_fused(x0, t, length, noise=noise, caption_batch=cb)


def pit_trainer(m):
    return trainer(m, hig_amd.DDPMMulTrainer, multi=True, label_path=None, cap_id=False)


PIT = dict(TINY, num_frames=20)


def test_two_person_pit_step_with_a_caption_batch_equals_the_step_fed_the_banks_rows():
    c, P = PIT, 2
    c1, c2 = [CAPS[0], CAPS[1]], [CAPS[2], CAPS[0]]
    caps = c1 + c2 + c2 + c1                                              # the model batch of the PIT step: 4 P rows
    x0, noise = step_inputs(2 * P, c["T"], c["F"], 2)
    t, length = torch.tensor([3, 700]).to(DEV), torch.tensor([16, 9]).to(DEV)
    two = hig_amd.MotionInteractionTransformer
    m1, m2 = build(cls=two, c=c, caption_bank=8, text_dedup=False).train(), build(cls=two, c=c).train()
    t1, t2 = pit_trainer(m1), pit_trainer(m2)
    bank = m1.caption_bank
    cb = bank.batch(caps, DEV)
    assert cb.rows == 4 * P and cb.U == 3
    l1 = t1.train_step_fused(x0, t, length, noise=noise, caption_batch=cb).clone()
    sl = cb.slot.long()
    l2 = t2.train_step_fused(x0, t, length, noise=noise, clip_out=bank.feat[sl], eot=bank.eot[sl]).clone()
    assert torch.equal(l1, l2) and torch.isfinite(l1).all()
    assert_same_state(state_of(m1, t1), state_of(m2, t2), "PIT step")
    # and with the head on the distinct captions: the same loss within the step's tolerance, through train_fused_batch
    m3 = build(cls=two, c=c, caption_bank=8).train()
    t3 = pit_trainer(m3)
    t3.sampler.sample = lambda bs, dev: (t.to(dev), torch.ones(bs))
    l3 = t3.train_fused_batch((c1, c2, x0[:P].cpu(), x0[P:].cpu(), length.cpu(), None), noise=noise)
    assert abs(l3.item() - l2.item()) < 1e-5 * abs(l2.item())
    assert m3.caption_bank.stats["tower_calls"] == 1 and len(m3.caption_bank) == 3


# ---- the dedup gate -----------------------------------------------------------------------------------------------------------
def fp64_head(m, clip_out, eot, r1, r2):
    """xf_proj, xf_out and every parameter gradient of the stock-torch text head in fp64 on the CPU."""
    ref = build_cpu_twin(m)
    xp, xo = ref._text_head_torch(None, clip_out.double().cpu().permute(1, 0, 2), eot.cpu())
    ((xp * r1.double().cpu()).sum() + (xo * r2.double().cpu()).sum()).backward()
    named = dict(ref.named_parameters())
    return xp.detach(), xo.detach(), {k: named[k].grad for k in named if k.startswith("text")}


def build_cpu_twin(m):
    c = TINY
    ref = hig_amd.MotionTransformer(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                    num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"], text_num_heads=4, text_ff_size=128,
                                    num_text_layers=2, clip_model=stub_clip.StubCLIP(), clip_tokenize=stub_clip.tokenize)
    ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    return ref.double().train()


def head_grads(m, grads):
    names = {id(p): k for k, p in m.named_parameters()}
    return {names[id(p)]: g.detach().double().cpu() for p, g in zip(m._text_params(), grads)}


def distance(got, ref, name):
    got, ref = got.double().cpu(), ref.double().cpu()
    if name.endswith("in_proj_bias"):
        d = ref.shape[0] // 3
        got, ref = torch.cat([got[:d], got[2 * d:]]), torch.cat([ref[:d], ref[2 * d:]])
    return ((got - ref).norm() / ref.norm()).item()


def test_the_head_on_distinct_captions_is_as_close_to_fp64_as_the_head_on_every_row():
    m = build(caption_bank=8).train()
    bank = m.caption_bank
    rows_of = [0, 1, 2, 0, 3, 3, 1, 0, 2, 3, 0, 1]                          # 12 rows over 4 distinct captions
    cb = bank.batch([CAPS[i] for i in rows_of], DEV)
    assert (cb.rows, cb.U, cb.U_pad) == (12, 4, 8)
    g = torch.Generator().manual_seed(12)
    dxp = torch.randn(12, 4 * TINY["d"], generator=g).to(DEV)
    dxo = torch.randn(12, N, TINY["Lt"], generator=g).to(DEV)
    clip12, eot12 = bank.gather(cb.slot, 12)
    # route (a): the parent's launches at 12 rows
    xp_a, xo_a, saved = m._launch_text_head(clip12, eot12, training=True)
    grads_a, _ = m._launch_text_head_backward(clip12, eot12, xo_a, saved, dxo, dxp, False)
    grads_a = head_grads(m, grads_a)
    # route (b): U_pad = 8 rows + gather + segment sums
    clip8, eot8 = bank.gather(cb.uniq_slot, cb.U_pad)
    xp_u, xo_u, saved = m._launch_text_head(clip8, eot8, training=True)
    xp_b, xo_b = CBK.expand_rows(xp_u, cb.inv, 12), CBK.expand_rows(xo_u, cb.inv, 12)
    dxp_u, dxo_u = CBK.segment_sum_rows(dxp, cb.order, cb.seg, 8), CBK.segment_sum_rows(dxo, cb.order, cb.seg, 8)
    assert (bits(dxp_u[4:]) == 0).all() and (bits(dxo_u[4:]) == 0).all()   # the padding's upstream gradient is exactly zero
    grads_b, _ = m._launch_text_head_backward(clip8, eot8, xo_u, saved, dxo_u, dxp_u, False)
    grads_b = head_grads(m, grads_b)
    torch.cuda.synchronize()
    xp64, xo64, g64 = fp64_head(m, clip12, eot12, dxp, dxo)
    worst = (0.0, None)
    for what, a, b, ref in (("xf_proj", xp_a, xp_b, xp64), ("xf_out", xo_a, xo_b, xo64)):
        da, db = distance(a, ref, what), distance(b, ref, what)
        print("dedup forward %-8s (a) %.3e (b) %.3e" % (what, da, db))
        assert db <= max(1e-6, 4 * da), what
    assert set(g64) == set(grads_a) == set(grads_b)
    for k in sorted(g64):
        da, db = distance(grads_a[k], g64[k], k), distance(grads_b[k], g64[k], k)
        worst = max(worst, (db / max(da, 1e-30), k))
        print("dedup gradient %-50s (a) %.3e (b) %.3e" % (k, da, db))
        assert db <= max(1e-6, 4 * da), k
    print("dedup gate: worst (b) / (a) = %.2f at %s" % worst)


# ---- the whole step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["stub", "native"])
def test_a_step_with_bank_and_dedup_tracks_the_parent_step_and_the_tower_runs_in_step_one_only(kind, monkeypatch):
    c = TINY
    caps = [CAPS[0], CAPS[1], CAPS[0], CAPS[2]]
    t_fixed = torch.tensor([3, 987, 500, 40])
    x0, noise = step_inputs(c["B"], c["T"], c["F"], 3)
    losses = {}
    for mode in ("parent", "bank"):
        m = build(kind, **({"caption_bank": 16} if mode == "bank" else {})).train()
        tr = trainer(m)
        tr.sampler.sample = lambda bs, dev: (t_fixed.to(dev), torch.ones(bs))
        calls = TowerCalls(m, monkeypatch)
        losses[mode] = tr.train_fused_batch((caps, x0.cpu(), torch.tensor([16, 9, 1, 12])), noise=noise).item()
    print("one fused step (%s CLIP): parent %.8f, bank + dedup %.8f" % (kind, losses["parent"], losses["bank"]))
    assert abs(losses["bank"] - losses["parent"]) < 1e-5 * abs(losses["parent"])
    assert m.caption_bank.stats["tower_calls"] == 1 and (calls.tower, calls.tokenizer) == (1, 1)   # m: the banked model
    for k in range(4):
        order = [(k + i) % 4 for i in (0, 0, 1, 3)]                         # other orders, other duplicates
        loss = tr.train_fused_batch(([caps[i] for i in order], x0.cpu(), torch.tensor([16, 9, 1, 12])), noise=noise)
        assert torch.isfinite(loss).all()
    assert (calls.tower, calls.tokenizer) == (1, 1)
    assert m.caption_bank.stats["tower_calls"] == 1 and m.caption_bank.stats["tokenizer_calls"] == 1
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert int(tr.fused_state()["step"].item()) == 5


def test_a_step_with_bank_and_dedup_runs_with_bf16_storage():
    """The two routes hand the denoiser text embeddings that differ in the last fp32 bits; behind them every activation is
    rounded to bf16, so the losses are held to one bf16 ulp (2^-8 relative), not to the fp32 step's 1e-5."""
    c = dict(B=4, T=33, F=12, d=128, H=2, L=2, ff=96, Lt=64, num_frames=40)
    caps = [CAPS[0], CAPS[1], CAPS[0], CAPS[0]]
    x0, noise = step_inputs(4, c["T"], c["F"], 5)
    t_fixed = torch.tensor([7, 650, 3, 999])
    losses = {}
    for mode in ("parent", "bank"):
        m = build(c=c, storage="bf16", **({"caption_bank": 16} if mode == "bank" else {})).train()
        tr = trainer(m)
        tr.sampler.sample = lambda bs, dev: (t_fixed.to(dev), torch.ones(bs))
        losses[mode] = tr.train_fused_batch((caps, x0.cpu(), torch.tensor([33, 5, 20, 33])), noise=noise).item()
        assert all(torch.isfinite(p).all() for p in m.parameters())
    print("one fused step, bf16 storage: parent %.8f, bank + dedup %.8f" % (losses["parent"], losses["bank"]))
    assert abs(losses["bank"] - losses["parent"]) < 2.0 ** -8 * abs(losses["parent"])


# ---- the captured route -------------------------------------------------------------------------------------------------------
def test_captured_step_equals_fused_step_bit_for_bit_over_replays_and_a_second_u_pad():
    c, B = TINY, 10
    requests = [[CAPS[i] for i in (0, 1, 0, 2, 2, 1, 0, 0, 1, 2)],          # U = 3
                [CAPS[i] for i in (4, 3, 2, 1, 0, 0, 1, 2, 3, 4)],          # U = 5: other captions, the same U_pad = 8
                CAPS[:10]]                                                  # U = 10: U_pad = 16, a second graph
    length = torch.tensor([16, 9, 1, 12, 16, 3, 16, 8, 16, 2]).to(DEV)
    mf, mc = build(caption_bank=16).train(), build(caption_bank=16).train()
    tf, tc = trainer(mf), trainer(mc)
    for k, caps in enumerate(requests):
        x0, noise = step_inputs(B, c["T"], c["F"], 20 + k)
        t = torch.tensor([(37 * i + 11 * k) % 1000 for i in range(B)]).to(DEV)
        lf = tf.train_step_fused(x0, t, length, noise=noise, caption_batch=mf.caption_bank.batch(caps, DEV)).clone()
        lc = tc.train_step_captured(x0, t, length, noise=noise, caption_batch=mc.caption_bank.batch(caps, DEV)).clone()
        torch.cuda.synchronize()
        assert torch.equal(lf, lc) and torch.isfinite(lf).all(), k
        assert_same_state(state_of(mf, tf), state_of(mc, tc), "captured step %d" % k)
        assert len(tc.fused_state()["graphs"]) == (1 if k < 2 else 2)


# ---- samplers -------------------------------------------------------------------------------------------------------------------
def test_generate_of_both_trainers_and_the_guided_sampler_with_the_bank_on():
    c = TINY
    caps = [CAPS[0], CAPS[1], CAPS[0], CAPS[2]]
    lens = torch.tensor([16, 9, 12, 16])
    out = {}
    for mode in ("off", "on"):
        m = build(**({"caption_bank": 8} if mode == "on" else {})).eval()
        tr = trainer(m)
        tr.diffusion = make_diffusion(50)
        res = []
        for scale in (None, 2.0):
            tr.set_sampler(guidance_scale=scale)
            torch.manual_seed(7)
            with torch.no_grad():
                res.append(torch.stack(tr.generate(caps, lens, c["F"])))
        two = build(cls=hig_amd.MotionInteractionTransformer, c=PIT, **({"caption_bank": 8} if mode == "on" else {})).eval()
        tr2 = pit_trainer(two)
        tr2.diffusion = make_diffusion(50)
        torch.manual_seed(8)
        with torch.no_grad():
            pairs = tr2.generate(caps[:2], caps[2:], lens[:2], c["F"])
        res.append(torch.stack([torch.stack(p) for p in pairs]))
        out[mode] = res
        if mode == "on":
            assert m.caption_bank.stats["tower_calls"] == 2 and set(m.caption_bank.slots) == set(caps) | {""}
            assert two.caption_bank.stats["tower_calls"] == 1
    for what, a, b in zip(("generate", "guided generate", "two-person generate"), out["on"], out["off"]):
        assert torch.isfinite(a).all() and a.abs().max() > 0
        print("%s, bank on vs off: %.2e" % (what, rel(a, b)))
        assert rel(a, b) < 2e-5, what
