"""The caption bank without a GPU (models/caption_bank.py): the index arrays of a request against a plain Python restatement,
the padding rule, the overflow slots, the refusals, the argument checks of the three row entry points (csrc/textrows.hip) and
the option left unset.  The stub CLIP runs on the CPU, so the bank's planning and its fills are exercised here; the gathers
themselves need the device (tests/test_gpu_caption_bank.py)."""
import ctypes as C
import types

import pytest
import torch

import hig_amd
from hig_amd import _lib
from hig_amd.models import caption_bank as CBK
from hig_amd.models import stub_clip


def tiny(cls=None, **kw):
    cls = cls or hig_amd.MotionTransformer
    return cls(input_feats=12, num_frames=16, latent_dim=64, ff_size=128, num_layers=2, num_heads=8, text_latent_dim=64,
               text_num_heads=4, text_ff_size=128, num_text_layers=2, clip_model=stub_clip.StubCLIP(),
               clip_tokenize=stub_clip.tokenize, **kw)


def restate(captions, slot_of):
    """inv, order, seg, uniq_slot, slot of a caption list, the slow way."""
    uniq = []
    for c in captions:
        if c not in uniq:
            uniq.append(c)
    U = len(uniq)
    U_pad = 8
    while U_pad < U:
        U_pad *= 2
    inv = [uniq.index(c) for c in captions]
    members = [[r for r, u in enumerate(inv) if u == v] for v in range(U)] + [[] for _ in range(U_pad - U)]
    order = [r for m in members for r in m]
    seg = [0]
    for m in members:
        seg.append(seg[-1] + len(m))
    uniq_slot = [slot_of[c] for c in uniq] + [slot_of[uniq[0]]] * (U_pad - U)
    return dict(U=U, U_pad=U_pad, inv=inv, order=order, seg=seg, uniq_slot=uniq_slot, slot=[slot_of[c] for c in captions])


def same(cb, want):
    assert (cb.U, cb.U_pad, cb.rows) == (want["U"], want["U_pad"], len(want["inv"]))
    for k in ("slot", "uniq_slot", "inv", "order", "seg"):
        assert getattr(cb, k + "_host").tolist() == want[k], k
        assert getattr(cb, k).dtype == torch.int32 and getattr(cb, k).tolist() == want[k], k
    assert cb.host.dtype == torch.int32 and cb.host.numel() == 3 * cb.rows + 2 * cb.U_pad + 2 and int(cb.host[-1]) == cb.U
    assert cb.dev.data_ptr() == cb.slot.data_ptr()                       # ONE packed buffer: the arrays are its views


def test_caption_batch_with_duplicates_and_a_miss():
    m = tiny(caption_bank=16)
    bank = m.caption_bank
    first = bank.batch(["wave", "jump", "wave"])
    assert bank.slots == {"wave": 0, "jump": 1} and bank.stats["misses"] == 2 and bank.stats["hits"] == 0
    same(first, restate(["wave", "jump", "wave"], bank.slots))
    captions = ["jump", "kick", "wave", "jump", "jump", "kick", "wave"]     # "kick" is the miss
    cb = bank.batch(captions)
    assert bank.slots == {"wave": 0, "jump": 1, "kick": 2}
    want = restate(captions, bank.slots)
    same(cb, want)
    # the padding rule: U = 3 gives U_pad = 8; five padding entries repeat uniq_slot[0] and have empty segments
    assert (cb.U, cb.U_pad) == (3, 8) and cb.uniq_slot.tolist()[3:] == [1] * 5
    seg = cb.seg.tolist()
    assert len(seg) == 9 and all(seg[u] == seg[u + 1] == len(captions) for u in range(3, 8))
    assert sorted(cb.order.tolist()) == list(range(len(captions)))
    for u in range(cb.U):                                                # each list ascending: the sum order is the row order
        rows = cb.order.tolist()[seg[u]:seg[u + 1]]
        assert rows == sorted(rows) and all(captions[r] == captions[rows[0]] for r in rows)
    assert bank.stats["misses"] == 3 and bank.stats["hits"] == 5 and bank.stats["tower_calls"] == 2
    assert bank.stats["tokenizer_calls"] == 2 and bank.stats["overflow_rows"] == 0 and bank.stats["fills"] == 2
    assert [CBK.padded_unique(u) for u in (1, 8, 9, 16, 17, 44)] == [8, 8, 16, 16, 32, 64]


def test_fill_chunks_hold_exactly_eight_captions_and_slots_hold_their_rows():
    m = tiny(caption_bank=32)
    bank = m.caption_bank
    seen = []
    real = m._clip_features
    m._clip_features = lambda text, device: (seen.append(list(text)), real(text, device))[1]
    captions = ["c%d" % i for i in range(11)]
    bank.batch(captions + captions[:3])
    assert [len(s) for s in seen] == [8, 8] and seen[1] == captions[8:] + [""] * 5 and bank.stats["fills"] == 2
    for c in captions:
        chunk, i = bank.chunk_of[c]
        tokens, x = real(list(chunk), "cpu")
        assert torch.equal(bank.feat[bank.slots[c]], x.permute(1, 0, 2)[i]) and int(bank.eot[bank.slots[c]]) == int(tokens[i].argmax())
    assert bank.feat.shape == (32 + bank.spill, 77, 512) and bank.eot.dtype == torch.int64


def test_overflow_goes_to_transient_slots_behind_the_persistent_ones():
    m = tiny(caption_bank=2)
    bank = m.caption_bank
    ptr = None
    for _ in range(2):                                                   # the overflow is recomputed each time
        cb = bank.batch(["a", "b", "c", "d", "c"])
        assert bank.slots == {"a": 0, "b": 1} and len(bank) == 2
        assert cb.slot.tolist() == [0, 1, 2, 3, 2] and cb.uniq_slot.tolist()[:4] == [0, 1, 2, 3]
        assert ptr in (None, bank.feat.data_ptr())                       # allocated once, at full size
        ptr = bank.feat.data_ptr()
    assert bank.stats["overflow_rows"] == 6 and bank.stats["misses"] == 2 and bank.stats["hits"] == 2
    assert bank.stats["tower_calls"] == 2
    tokens, x = m._clip_features(["c", "d"] + [""] * 6, "cpu")
    assert torch.equal(bank.feat[2], x[:, 0]) and torch.equal(bank.feat[3], x[:, 1])
    small = hig_amd.models.caption_bank.CaptionBank(m, 1, spill=1)
    with pytest.raises(RuntimeError, match="capacity"):
        small.batch(["a", "b", "c"])


def test_the_bank_refuses_a_trainable_tower_and_cap_id_models():
    with pytest.raises(ValueError, match="trainable"):
        tiny(no_clip=True, caption_bank=8)
    with pytest.raises(ValueError, match="cap_id"):
        tiny(hig_amd.MotionInteractionTransformer, cap_id=True, caption_bank=8)
    with pytest.raises(ValueError, match="trainable"):
        tiny(hig_amd.MotionInteractionTransformer, no_clip=True).enable_caption_bank(8)
    m = tiny(caption_bank=8)
    m.caption_bank.batch(["a"])
    m.clip.ln_final.weight.requires_grad_(True)                          # un-frozen behind the bank's back
    with pytest.raises(ValueError, match="trainable"):
        m.caption_bank.batch(["a"])
    for bad in (-1, 2.5, True, "8"):
        with pytest.raises(ValueError, match="capacity"):
            tiny().enable_caption_bank(bad)
    opt = types.SimpleNamespace(device="cpu", diffusion_steps=1000, is_train=False, caption_bank=4, multi=True, label_path=None,
                                cap_id=True)
    with pytest.raises(ValueError, match="cap_id"):
        hig_amd.DDPMMulTrainer(opt, tiny(hig_amd.MotionInteractionTransformer, cap_id=True))


def test_the_bank_empties_itself_when_the_tower_may_have_changed():
    m = tiny(caption_bank=8)
    bank = m.caption_bank
    for change in ("param", "to", "load", "tokenizer", "flag"):
        bank.batch(["a", "b"])
        assert len(bank) == 2
        calls = bank.stats["tower_calls"]
        if change == "param":
            with torch.no_grad():
                m.clip.positional_embedding.add_(1.0)
        elif change == "to":
            m.to("cpu")
            assert len(bank) == 0
        elif change == "load":
            m.load_state_dict(m.state_dict())
            assert len(bank) == 0
        elif change == "tokenizer":
            m._clip_tokenize = lambda text, truncate=True: stub_clip.tokenize(text, truncate=truncate)
        else:
            m.clip_tower = "torch"
        bank.batch(["a"])
        assert len(bank) == 1 and bank.stats["tower_calls"] == calls + 1, change
        tokens, x = m._clip_features(["a"] + [""] * 7, "cpu")
        assert torch.equal(bank.feat[0], x[:, 0])


def test_row_entry_points_refuse_null_pointers_and_negative_sizes_before_any_device_call():
    L = _lib.lib()
    EINVAL = _lib.EINVAL
    raw = (C.c_float * 256)()
    base = (C.addressof(raw) + 15) // 16 * 16
    a, b, c, d, e = (C.c_void_p(base + 64 * i) for i in range(5))

    def gather(src=a, n_src=3, idx=b, n_out=2, row_floats=4, dst=c):
        return L.hig_rows_gather_f32(src, n_src, idx, n_out, row_floats, dst, None)

    def caption(feat=a, eot_src=b, n_slots=3, slot=c, rows=2, row_floats=4, clip_out=d, eot=e):
        return L.hig_caption_gather(feat, eot_src, n_slots, slot, rows, row_floats, clip_out, eot, None)

    def segsum(src=a, n_src=3, order=b, seg=c, n_seg=2, row_floats=4, dst=d):
        return L.hig_rows_segment_sum_f32(src, n_src, order, seg, n_seg, row_floats, dst, None)

    cases = ((gather, "hig_rows_gather_f32", ("src", "idx", "dst"), ("n_src", "n_out", "row_floats")),
             (caption, "hig_caption_gather", ("feat", "eot_src", "slot", "clip_out", "eot"), ("n_slots", "rows", "row_floats")),
             (segsum, "hig_rows_segment_sum_f32", ("src", "order", "seg", "dst"), ("n_src", "n_seg", "row_floats")))
    for fn, name, pointers, sizes in cases:
        for p in pointers:
            assert fn(**{p: None}) == EINVAL, "%s accepts %s = NULL" % (name, p)
            assert name in _lib.last_error()
        for s in sizes:
            assert fn(**{s: -1}) == EINVAL, "%s accepts %s = -1" % (name, s)
            assert name in _lib.last_error()
    assert gather(dst=C.c_void_p(c.value + 2)) == EINVAL and caption(eot=C.c_void_p(e.value + 4)) == EINVAL
    assert segsum(order=C.c_void_p(b.value + 1)) == EINVAL
    # nothing to do is no error, and launches nothing
    assert gather(n_out=0) == 0 and caption(rows=0) == 0 and segsum(n_seg=0) == 0 and segsum(row_floats=0) == 0
    assert gather(row_floats=0) == 0


def test_the_option_left_unset_constructs_no_bank():
    m = tiny()
    assert m.caption_bank is None and m._caption_bank is None
    assert tiny(caption_bank=None).caption_bank is None and tiny(caption_bank=0).caption_bank is None
    assert not any("caption" in k for k in m.state_dict())
    two = tiny(hig_amd.MotionInteractionTransformer, cap_id=True)
    assert two.caption_bank is None
    for opt in (types.SimpleNamespace(), types.SimpleNamespace(caption_bank=None), types.SimpleNamespace(caption_bank=0)):
        opt.device, opt.diffusion_steps, opt.is_train = "cpu", 1000, False
        tr = hig_amd.DDPMTrainer(opt, m)
        assert m.caption_bank is None and tr._text_inputs.__func__ is hig_amd.DDPMTrainer._text_inputs
    on = tiny(caption_bank=8)
    assert on.caption_bank.capacity == 8 and on.text_dedup is True and not any("caption" in k for k in on.state_dict())
    assert tiny(caption_bank=8, text_dedup=False).text_dedup is False
    opt = types.SimpleNamespace(device="cpu", diffusion_steps=1000, is_train=False, caption_bank=4, text_dedup=False)
    hig_amd.DDPMTrainer(opt, m)
    assert m.caption_bank.capacity == 4 and m.text_dedup is False
    m.enable_caption_bank(None)
    assert m.caption_bank is None
    with pytest.raises(ValueError, match="exclusive"):
        on_tr = hig_amd.DDPMTrainer(types.SimpleNamespace(device="cpu", diffusion_steps=1000, is_train=False), on)
        on_tr._text_source(None, None, torch.zeros(1), None, on.caption_bank.batch(["a"]), None)
