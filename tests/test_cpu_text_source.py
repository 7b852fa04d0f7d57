"""The text sources of the fused / captured training step without a GPU (trainers/text_source.py): which source
`DDPMTrainer._text_source` resolves each argument set to, what a captured step would copy and key on, and that a source moved
onto static buffers is the same source.  What the sources launch needs the device (tests/test_gpu_text_source.py)."""
import types

import pytest
import torch

import hig_amd
from hig_amd.trainers import text_source as TS
from test_cpu_caption_bank import tiny
from test_cpu_class_head import tiny as tiny_class


def trainer(m, cls=None, **kw):
    opt = types.SimpleNamespace(device="cpu", diffusion_steps=1000, is_train=False, **kw)
    return (cls or hig_amd.DDPMTrainer)(opt, m)


def class_trainer():
    m = tiny_class(cap_id=True, class_head="hip")
    m._class_head_args = lambda ids: None         # (the model's own check wants the ids on the device: test_cpu_class_head.py)
    return trainer(m, hig_amd.DDPMMulTrainer, multi=True, label_path=None, cap_id=True), m


def test_resolver_returns_one_source_per_argument_set_with_the_steps_precedence():
    m = tiny(caption_bank=8)
    tr = trainer(m)
    xp, xo, clip, eot = torch.zeros(3, 256), torch.zeros(3, 77, 64), torch.zeros(3, 77, 512), torch.zeros(3, dtype=torch.int64)
    cb = m.caption_bank.batch(["a", "b", "a"])
    ids = torch.zeros(4, dtype=torch.int32)
    emb = tr._text_source(xp, xo, None, None, None, None)
    assert type(emb) is TS.Embeddings and emb.tensors[0] is xp and emb.tensors[1] is xo and emb.forward(tr) is emb.tensors
    feat = tr._text_source(None, None, clip, eot, None, None)
    assert type(feat) is TS.ClipFeatures and feat.tensors[0] is clip and feat.tensors[1] is eot
    bank = tr._text_source(None, None, None, None, cb, None)
    assert type(bank) is TS.Banked and bank.cb is cb
    ctr, _ = class_trainer()
    cls = ctr._text_source(None, None, None, None, None, ids)
    assert type(cls) is TS.ClassIds and len(cls.tensors) == 1 and cls.tensors[0] is ids
    # what the steps accept together: embeddings beside CLIP features or beside a bank request are ignored
    assert type(tr._text_source(xp, xo, clip, eot, None, None)) is TS.ClipFeatures
    assert type(tr._text_source(xp, None, clip, eot, None, None)) is TS.ClipFeatures
    assert type(tr._text_source(xp, xo, None, None, cb, None)) is TS.Banked
    assert type(tr._text_source(None, xo, None, None, cb, None)) is TS.Banked
    # nothing at all is the embeddings source, as before: the step fails on its missing inputs, not the resolver
    assert type(tr._text_source(None, None, None, None, None, None)) is TS.Embeddings
    assert [s.kind for s in (emb, feat, bank, cls)] == ["embeddings", "clip", "bank", "class_ids"]


def test_refusals_come_in_the_steps_order_bank_first_then_class_ids():
    m = tiny(caption_bank=8)
    tr = trainer(m)
    cb = m.caption_bank.batch(["a"])
    ids = torch.zeros(4, dtype=torch.int32)
    for kw in (dict(clip_out=torch.zeros(1)), dict(eot=torch.zeros(1))):
        with pytest.raises(ValueError, match="caption_batch= and clip_out= / eot= are exclusive"):
            tr._text_source(None, None, kw.get("clip_out"), kw.get("eot"), cb, None)
    with pytest.raises(RuntimeError, match="needs the model's caption bank"):
        trainer(tiny())._text_source(None, None, None, None, cb, None)
    ctr, _ = class_trainer()
    with pytest.raises(RuntimeError, match="needs the model's caption bank"):      # (not the ids' refusal: the bank's comes first)
        ctr._text_source(None, None, None, None, cb, ids)
    with pytest.raises(ValueError, match="class_ids= is exclusive"):
        ctr._text_source(torch.zeros(1), None, None, None, None, ids)


def test_trains_head_and_statics():
    m = tiny(caption_bank=8)
    xp, xo, clip, eot = torch.zeros(3, 256), torch.zeros(3, 77, 64), torch.zeros(3, 77, 512), torch.zeros(3, dtype=torch.int64)
    cb = m.caption_bank.batch(["a", "b", "a"])
    ids = torch.zeros(4, dtype=torch.int32)
    sources = (TS.Embeddings(xp, xo), TS.ClipFeatures(clip, eot), TS.Banked(cb), TS.ClassIds(ids))
    assert [s.trains_head for s in sources] == [False, True, True, True]
    assert [[tuple(a.shape) for a in s.statics()] for s in sources] == [[(3, 256), (3, 77, 64)], [(3, 77, 512), (3,)],
                                                                         [(3 * 3 + 2 * 8 + 2,)], [(4,)]]
    assert sources[0].statics()[0] is xp and sources[1].statics()[1] is eot
    assert sources[2].statics()[0] is cb.dev and sources[3].statics()[0] is ids


def test_on_gives_the_same_source_reading_from_the_static_buffers():
    m = tiny(caption_bank=8)
    xp, xo, clip, eot = torch.zeros(3, 256), torch.zeros(3, 77, 64), torch.zeros(3, 77, 512), torch.zeros(3, dtype=torch.int64)
    cb = m.caption_bank.batch(["a", "b", "a"])
    ids = torch.tensor([3, 41, 4, 3], dtype=torch.int32)
    for src in (TS.Embeddings(xp, xo), TS.ClipFeatures(clip, eot), TS.Banked(cb), TS.ClassIds(ids)):
        static = tuple(a.clone() for a in src.statics())
        twin = src.on(static)
        assert type(twin) is type(src) and twin is not src and twin.kind == src.kind
        assert len(twin.statics()) == len(static) and all(a is b for a, b in zip(twin.statics(), static))
        assert all(a is b for a, b in zip(twin.on(src.statics()).statics(), src.statics()))      # and back again
        assert twin.key(m) == src.key(m)
    banked = TS.Banked(cb).on((cb.dev.clone(),))
    assert (banked.cb.rows, banked.cb.U, banked.cb.U_pad) == (cb.rows, cb.U, cb.U_pad) and banked.cb.host is cb.host
    for name in ("slot", "uniq_slot", "inv", "order", "seg"):           # the index arrays are views of the NEW buffer
        assert torch.equal(getattr(banked.cb, name), getattr(cb, name))
        assert getattr(banked.cb, name).data_ptr() != getattr(cb, name).data_ptr()


def test_key_of_a_bank_request_is_its_layout_the_dedup_switch_and_the_banks_buffers():
    m = tiny(caption_bank=32)
    bank = m.caption_bank
    a = TS.Banked(bank.batch(["a", "b", "a", "c"]))                     # U = 3: U_pad = 8
    b = TS.Banked(bank.batch(["d", "d", "e", "f"]))                     # other captions, the same (rows, U_pad)
    assert a.cb.U_pad == b.cb.U_pad == 8 and a.key(m) == b.key(m)
    assert a.key(m) == ((4, 8, True, bank.feat.data_ptr(), bank.eot.data_ptr()),)
    wide = TS.Banked(bank.batch(["c%d" % i for i in range(9)] + ["c0"] * 3))
    narrow = TS.Banked(bank.batch(["c0"] * 12))
    assert (wide.cb.rows, wide.cb.U_pad, narrow.cb.rows, narrow.cb.U_pad) == (12, 16, 12, 8)
    assert wide.key(m) != narrow.key(m)                                 # the same rows, another U_pad
    with_dedup = a.key(m)
    m.text_dedup = False
    assert a.key(m) != with_dedup and a.key(m)[0][:2] == with_dedup[0][:2]
    assert TS.Embeddings(None, None).key(m) == () and TS.ClipFeatures(None, None).key(m) == ()


def test_key_of_class_ids_says_that_the_class_head_is_inside_and_for_how_many_rows():
    ids = torch.zeros(8, dtype=torch.int32)
    assert ("class_head", (8,)) in TS.ClassIds(ids).key(None)
    assert TS.ClassIds(ids).key(None) != TS.ClassIds(ids[:4]).key(None)
