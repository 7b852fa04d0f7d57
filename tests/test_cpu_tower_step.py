"""The CLIP text tower inside the fused / captured training step, without a GPU: clip_text.TokenBatch against a plain
restatement, the capacity layout of the device-built embedding index against the host EmbedIndex, every refusal of the new
entries before any HIP call, the "flat" option's refusals and flat-buffer layout, and the exclusivity of `token_batch=`.
What the entries and the step compute needs the device (tests/test_gpu_tower_step.py)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import clip_bounds as CB
import hig_amd
import tower_step_bounds as SB
from hig_amd import _lib
from hig_amd.models import clip_text as CT
from hig_amd.models import stub_clip
from hig_amd.models.transformer import _FlatParams
from hig_amd.trainers import text_source as TS


def tokenize(captions):
    return stub_clip.tokenize(captions, truncate=True)


# ---- TokenBatch -----------------------------------------------------------------------------------------------------------------------
CAPTION_SETS = {
    "repeats": ["a b", "c", "c", "a b", "d e f", "a b"],
    "one": ["same words"] * 5,
    "eight": ["w%d" % i for i in range(8)] + ["w3", "w0"],          # U = 8 = U_pad: no padding entry
    "nine": ["w%d" % i for i in range(9)],                          # U = 9: U_pad = 16, seven padding entries
    "empty caption": ["x", "", "x", ""],                            # caption dropout: "" is one more caption
}


@pytest.mark.parametrize("name", list(CAPTION_SETS))
@pytest.mark.parametrize("dedup", [True, False])
def test_token_batch_against_a_plain_restatement(name, dedup):
    caps = CAPTION_SETS[name]
    calls = []

    def counting(c):
        calls.append(list(c))
        return tokenize(c)
    tb = CT.TokenBatch(caps, counting, dedup=dedup)
    want = SB.token_batch_restated(caps, tokenize, dedup)
    rows = len(caps)
    assert (tb.rows, tb.U, tb.U_pad, tb.N, tb.dedup) == (rows, want["U"], want["U_pad"], 77, dedup)
    assert tb.host.dtype == torch.int32 and tb.host.numel() == CT.TokenBatch.numel(rows, tb.U_pad, 77) and int(tb.host[-1]) == tb.U
    assert tb.tokens_host.dtype == torch.int64 and tb.tokens_host.shape == (tb.U_pad, 77) and tb.eot_host.dtype == torch.int64
    for field in ("tokens", "eot", "inv", "order", "seg"):
        assert np.array_equal(getattr(tb, field + "_host").numpy(), want[field]), field
    # every field is a view of the ONE packed buffer, in the documented order
    lay = CT.TokenBatch.layout(rows, tb.U_pad, 77)
    assert list(lay) == ["tokens", "eot", "inv", "order", "seg"] and lay["tokens"][0] == 0 and lay["seg"][1] == tb.host.numel() - 1
    assert tb.inv_host.data_ptr() == tb.host.data_ptr() + 4 * lay["inv"][0]
    # the tokenizer ran once, on the distinct captions only
    assert len(calls) == 1 and sorted(calls[0]) == sorted(set(caps)) and tb.tokenizer_rows == len(set(caps))
    if dedup:
        assert tb.U == len(set(caps)) and tb.U_pad >= 8 and tb.U_pad & (tb.U_pad - 1) == 0
        seg = tb.seg_host.numpy()
        assert (seg[tb.U:] == rows).all()                                                  # padding entries: empty segments
        assert all(torch.equal(tb.tokens_host[u], tb.tokens_host[0]) for u in range(tb.U, tb.U_pad))
        for r, c in enumerate(caps):                                                       # a row's tokens are its caption's
            assert torch.equal(tb.tokens_host[tb.inv_host[r]], tokenize([c])[0])
    else:
        assert tb.U == tb.U_pad == rows and list(tb.inv_host) == list(range(rows)) == list(tb.order_host)
        assert list(tb.seg_host) == list(range(rows + 1))


def test_token_batch_cache_keeps_the_tokenizer_off_a_caption_it_has_met_and_refusals():
    calls, cache = [], {}

    def counting(c):
        calls.append(list(c))
        return tokenize(c)
    a = CT.TokenBatch(["p", "q", "p"], counting, cache=cache)
    b = CT.TokenBatch(["q", "r", "r", "p"], counting, cache=cache)
    assert calls == [["p", "q"], ["r"]] and (a.tokenizer_rows, b.tokenizer_rows) == (2, 1) and set(cache) == {"p", "q", "r"}
    c = CT.TokenBatch(["q", "p"], counting, cache=cache)
    assert len(calls) == 2 and c.tokenizer_rows == 0
    assert torch.equal(c.tokens_host[:2], tokenize(["q", "p"]))
    with pytest.raises(ValueError):
        CT.TokenBatch([], tokenize)
    with pytest.raises(TypeError):
        CT.TokenBatch(["a", 3], tokenize)
    # the twin on another buffer of the same layout reads that buffer
    other = a.host.clone()
    twin = a.on_buffer(other)
    assert (twin.rows, twin.U, twin.U_pad, twin.dedup) == (a.rows, a.U, a.U_pad, a.dedup) and twin.dev is other
    assert twin.tokens.data_ptr() == other.data_ptr() and torch.equal(twin.seg, a.seg_host)


def test_tokens_source_statics_key_and_twin():
    tb = CT.TokenBatch(["a", "b", "a", "c"], tokenize)
    tb._bind(tb.host, tb.host.clone())           # (a host stand-in for the device copy)
    src = TS.Tokens(tb)
    assert (src.kind, src.trains_head, src.trains_tower) == ("tokens", True, True)
    assert len(src.statics()) == 1 and src.statics()[0] is tb.dev
    assert src.key(None) == ((4, 8, True),)
    assert TS.Tokens(CT.TokenBatch(["d", "e", "d", "d"], tokenize)).key(None) == src.key(None)       # other captions, the same shape
    assert TS.Tokens(CT.TokenBatch(["a", "b", "a", "c"], tokenize, dedup=False)).key(None) == ((4, 4, False),)
    static = tb.dev.clone()
    twin = src.on((static,))
    assert type(twin) is TS.Tokens and twin.statics()[0] is static and twin.key(None) == src.key(None)
    assert [getattr(s, "trains_tower", False) for s in (TS.Embeddings(None, None), TS.ClipFeatures(None, None), TS.ClassIds(torch.zeros(1)))] == [False] * 3


# ---- the capacity layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, N, vocab", [(1, 1, 1), (3, 8, 64), (1, 64, 5), (1, 65, 5), (4, 77, 300)])
@pytest.mark.parametrize("kind", ["captions", "distinct", "equal", "mixed"])
def test_capacity_layout_restated_equals_the_host_index_on_the_live_prefix(B, N, vocab, kind):
    chunk = _lib.CLIP_EMBED_CHUNK
    tok = SB.pattern(kind, B, N, vocab, seed=B * N)
    counts, arrays, total = SB.capacity_restated(tok, vocab, chunk)
    ix = CT.EmbedIndex(torch.from_numpy(tok), vocab)
    assert counts == (ix.n_live, ix.n_chunks, ix.n_ids)
    for name, n in SB.live_lengths(counts, B, N).items():
        assert np.array_equal(arrays[name][:n], getattr(ix, name)), name
        assert (arrays[name][n:] == SB.SENTINEL).all()
    # the offsets depend on (B, N, vocab) alone: the library's total, the module's restatement, and the documented capacities
    lay, ints, (cap_ids, cap_chunks) = CT.index_capacity(B, N, vocab)
    assert ints == total == _lib.lib().hig_clip_embed_index_cap_ints(B, N, vocab)
    assert cap_ids == min(B * N, vocab) and cap_chunks == -(-B * N // chunk) + cap_ids
    assert [lay[f][1] for f in CT.EmbedIndex.FIELDS] == [len(arrays[f]) for f in CT.EmbedIndex.FIELDS]
    assert [lay[f][0] for f in CT.EmbedIndex.FIELDS] == list(np.cumsum([0] + [len(arrays[f]) for f in CT.EmbedIndex.FIELDS])[:-1])
    assert counts[1] <= min(cap_chunks, B * N) and counts[2] <= cap_ids


# ---- the entries' refusals, before any HIP call ---------------------------------------------------------------------------------------
def test_every_new_entry_refuses_without_a_device():
    L = _lib.lib()
    p = C.c_void_p(16)
    E, Uu = _lib.EINVAL, _lib.EUNSUPPORTED
    # hig_clip_embed_index_build(tokens, B, N, vocab, index, counts, scratch, stream)
    build = lambda **kw: L.hig_clip_embed_index_build(*[kw.get(n, d) for n, d in (   # noqa: E731
        ("tokens", p), ("B", 8), ("N", 77), ("vocab", 49408), ("index", p), ("counts", p), ("scratch", p), ("stream", None))])
    assert build(tokens=None) == E and build(index=None) == E and build(counts=None) == E and build(scratch=None) == E
    assert build(B=-1) == E and build(N=0) == E and build(vocab=0) == E and "bad extent" in _lib.last_error()
    assert build(tokens=C.c_void_p(20)) == E and "unaligned" in _lib.last_error()
    assert build(index=C.c_void_p(18)) == E and build(counts=C.c_void_p(18)) == E and build(scratch=C.c_void_p(17)) == E
    assert build(B=852, N=77) == Uu and "65535" in _lib.last_error()                  # 65 604 rows: one caption past the keys' range
    assert build(B=65536, N=1) == Uu and build(B=65535, N=1, vocab=65537) == Uu and "vocab" in _lib.last_error()
    assert L.hig_clip_embed_index_scratch_bytes(65536, 1, 10) == -1 and L.hig_clip_embed_index_scratch_bytes(1, 1, 65537) == -1
    assert L.hig_clip_embed_index_scratch_bytes(1, 1, 1) == 8 and L.hig_clip_embed_index_scratch_bytes(480, 77, 49408) == 65536 * 4
    assert L.hig_clip_embed_index_scratch_bytes(32768, 1, 8) == 32768 * 4 and L.hig_clip_embed_index_scratch_bytes(32769, 1, 8) == 65536 * 4
    assert L.hig_clip_embed_index_scratch_bytes(-1, 1, 8) == -1 and L.hig_clip_embed_index_scratch_bytes(1, 0, 8) == -1
    assert L.hig_clip_embed_index_cap_ints(-1, 77, 10) == -1 and L.hig_clip_embed_index_cap_ints(1, 0, 10) == -1
    assert L.hig_clip_embed_index_cap_ints(1, 77, 0) == -1
    assert L.hig_clip_embed_index_cap_ints(2, 77, 100) == 154 + (3 + 100 + 1) + (3 + 100) + 101 + 100 + 154 + 78
    # hig_clip_embed_bwd_dev(dx0, B, N, W, vocab, index, counts, scratch, dtok, dpos, stream)
    emb = lambda **kw: L.hig_clip_embed_bwd_dev(*[kw.get(n, d) for n, d in (   # noqa: E731
        ("dx0", p), ("B", 2), ("N", 77), ("W", 512), ("vocab", 100), ("index", p), ("counts", p), ("scratch", p), ("dtok", p), ("dpos", p),
        ("stream", None))])
    assert emb(dx0=None) == E and emb(index=None) == E and emb(counts=None) == E and emb(scratch=None) == E
    assert emb(dtok=None) == E and emb(dpos=None) == E and "null" in _lib.last_error()
    assert emb(W=0) == E and emb(vocab=0) == E and emb(B=-1) == E and emb(N=0) == E and "bad extent" in _lib.last_error()
    assert emb(index=C.c_void_p(18)) == E and emb(counts=C.c_void_p(18)) == E and "unaligned" in _lib.last_error()
    assert L.hig_clip_embed_bwd_dev_scratch_floats(2, 77, 512, 100) == (min(3 + 100, 154) + 100) * 512
    assert L.hig_clip_embed_bwd_dev_scratch_floats(2, 77, 512, 49408) == (154 + 154) * 512        # never more than 2 M W
    assert L.hig_clip_embed_bwd_dev_scratch_floats(2, 77, 0, 100) == -1 and L.hig_clip_embed_bwd_dev_scratch_floats(-1, 77, 8, 100) == -1
    # hig_clip_text_bwd_dev(dims, params, index, counts, dout, saved, grads, bwd_workspace, stream)
    n_tab = 4 + 12 * 12
    table = (C.c_void_p * n_tab)(*([8] * n_tab))
    good = CT.clip_dims(2, 77, 512, 8, 12, 49408)
    for dims, code, word in ((CT.clip_dims(1, 77, 512, 16, 12, 49408), Uu, "head dim 32"), (CT.clip_dims(1, 129, 512, 8, 12, 49408), Uu, "N=129"),
                             (CT.clip_dims(1, 77, 512, 8, 12, 49408, prec=1), Uu, "exact fp32"), (CT.clip_dims(0, 77, 512, 8, 12, 49408), E, "positive")):
        assert L.hig_clip_text_bwd_dev(dims, table, p, p, p, p, table, p, None) == code and word in _lib.last_error()
    bwd = lambda **kw: L.hig_clip_text_bwd_dev(*[kw.get(n, d) for n, d in (   # noqa: E731
        ("dims", good), ("params", table), ("index", p), ("counts", p), ("dout", p), ("saved", p), ("grads", table), ("ws", p), ("stream", None))])
    assert bwd(params=None) == E and bwd(grads=None) == E and "null table" in _lib.last_error()
    assert bwd(index=None) == E and bwd(counts=None) == E and bwd(dout=None) == E and bwd(saved=None) == E and bwd(ws=None) == E
    assert bwd(index=C.c_void_p(18)) == E and "unaligned" in _lib.last_error()
    holed = (C.c_void_p * n_tab)(*([8] * n_tab))
    holed[5] = None
    assert bwd(grads=holed) == E and "hig_clip_text_bwd_dev: null parameter or gradient 5" in _lib.last_error()
    # the host-index entry keeps its messages
    assert L.hig_clip_text_bwd(good, table, p, 10, 5, 5, p, p, holed, p, None) == E and "hig_clip_text_bwd: null parameter or gradient 5" in _lib.last_error()


# ---- the option --------------------------------------------------------------------------------------------------------------------------
def two_person(layers=1, **kw):
    tower = CT.load_text_tower(CB.tower_weights(128, 2, layers, 77, stub_clip.VOCAB, seed=11))
    return hig_amd.MotionInteractionTransformer(input_feats=12, num_frames=16, latent_dim=64, ff_size=128, num_layers=2, num_heads=8,
                                                text_latent_dim=64, text_num_heads=4, text_ff_size=128, num_text_layers=1,
                                                clip_model=tower, clip_tokenize=stub_clip.tokenize, **kw)


def test_flat_needs_a_model_that_trains_its_tower(monkeypatch):
    monkeypatch.delenv("HIG_CLIP_TOWER_TRAIN", raising=False)
    with pytest.raises(ValueError, match="clip_tower_train='flat' needs a model that trains its CLIP text tower"):
        two_person(clip_tower_train="flat")                                              # no_clip unset: the tower is frozen
    with pytest.raises(ValueError, match="clip_tower_train='flat' needs"):
        hig_amd.MotionInteractionTransformer(input_feats=12, num_frames=16, latent_dim=64, ff_size=128, num_layers=2, num_heads=8,
                                             text_latent_dim=32, cap_id=True, clip_tower_train="flat")
    with pytest.raises(ValueError, match="'hip', 'torch' or 'flat'"):
        two_person(no_clip=True, clip_tower_train="triton")
    assert two_person(no_clip=True, clip_tower_train="flat").clip_tower_train == "flat"
    monkeypatch.setenv("HIG_CLIP_TOWER_TRAIN", "flat")
    assert two_person(no_clip=True).clip_tower_train == "flat"
    # a tower the rule refuses is an error, not a silent fallback: here the torch text head, and a tower that is not fp32
    with pytest.raises(RuntimeError, match="cannot join the flat parameter buffer: the text head is not on the HIP path"):
        _FlatParams(two_person(no_clip=True, text_head="torch"))
    half = two_person(no_clip=True)
    half.clip.half()
    with pytest.raises(RuntimeError, match="cannot join the flat parameter buffer: a tower parameter is torch.float16"):
        _FlatParams(half)


def test_flat_buffer_layout_with_the_option_and_todays_size_without(monkeypatch):
    monkeypatch.delenv("HIG_CLIP_TOWER_TRAIN", raising=False)
    sizes = {}
    for option in ("torch", "hip", None):
        m = two_person(layers=2, no_clip=True, **({} if option is None else {"clip_tower_train": option}))
        fp = _FlatParams(m)
        assert fp.tower_params == [] and fp.tower_offsets == []
        head = sum((p.numel() + 63) // 64 * 64 for p in fp.text_params)
        assert fp.numel == fp.core_numel + head                                          # today's size: the core and the text head
        assert all(p.data_ptr() < fp.flat.data_ptr() or p.data_ptr() >= fp.flat.data_ptr() + 4 * fp.numel for p in m.clip.parameters())
        sizes[option] = fp.numel
    assert len(set(sizes.values())) == 1
    m = two_person(layers=2, no_clip=True, clip_tower_train="flat")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    fp = _FlatParams(m)
    assert list(m.state_dict()) == list(before) and all(torch.equal(before[k], v) for k, v in m.state_dict().items())
    tower = CT._tower_tensors(m.clip)
    assert [id(p) for p in fp.tower_params] == [id(p) for p in tower] and len(tower) == 4 + 12 * 2
    assert fp.tower_offsets[0] == sizes["hip"] and all(o % _FlatParams.ALIGN == 0 for o in fp.tower_offsets)
    for (p, o), nxt in zip(zip(fp.tower_params, fp.tower_offsets), fp.tower_offsets[1:] + [fp.numel]):
        assert p.data_ptr() == fp.flat.data_ptr() + 4 * o and nxt == o + (p.numel() + 63) // 64 * 64
    assert len(fp.members()) == len(fp.params) + len(fp.text_params) + len(tower)
    assert set(id(p) for p in m.clip.parameters()) == set(id(p) for p in tower)          # the whole tower, nothing of it outside
    assert m._clip_train_table is None
    # writing through a parameter writes the buffer (valid() wants the device: tests/test_gpu_tower_step.py)
    with torch.no_grad():
        m.clip.ln_final.bias.fill_(3.0)
    o = fp.tower_offsets[3]
    assert (fp.flat[o:o + 128] == 3.0).all() and (fp.flat[o + 128:fp.tower_offsets[4]] == 0).all()


# ---- token_batch= ---------------------------------------------------------------------------------------------------------------------
def trainer(m, **kw):
    opt = types.SimpleNamespace(device="cpu", diffusion_steps=1000, is_train=False, multi=True, label_path=None, cap_id=False, **kw)
    return hig_amd.DDPMMulTrainer(opt, m)


def test_token_batch_is_exclusive_with_every_other_text_argument_and_needs_the_option():
    tb = CT.TokenBatch(["a", "b", "b", "a"], tokenize)
    tr = trainer(two_person(no_clip=True, clip_tower_train="flat"))
    src = tr._text_source(None, None, None, None, None, None, tb)
    assert type(src) is TS.Tokens and src.tb is tb
    assert type(tr._text_source(None, None, None, None, None, None, token_batch=tb)) is TS.Tokens
    z = torch.zeros(1)
    for args in ((z, None, None, None, None, None), (None, z, None, None, None, None), (None, None, z, None, None, None),
                 (None, None, None, z, None, None), (None, None, None, None, object(), None), (None, None, None, None, None, z.int())):
        with pytest.raises(ValueError, match="token_batch= is exclusive"):
            tr._text_source(*args, token_batch=tb)
    for option in ("hip", "torch"):
        with pytest.raises(ValueError, match="token_batch= needs a no_clip model built with clip_tower_train='flat'"):
            trainer(two_person(no_clip=True, clip_tower_train=option))._text_source(None, None, None, None, None, None, tb)
    # the steps take the argument (on the parent commit: TypeError), and refuse it in the same words before touching the device
    for step in (tr.train_step_fused, tr.train_step_captured):
        with pytest.raises(ValueError, match="token_batch= is exclusive"):
            step(z, z, z, clip_out=z, token_batch=tb)
    # without the argument the resolver is today's
    assert type(tr._text_source(z, z, None, None, None, None)) is TS.Embeddings


def test_text_inputs_builds_the_token_batch_for_such_a_model_and_honours_text_dedup():
    m = two_person(no_clip=True, clip_tower_train="flat")
    caps = ["a b", "c", "c", "a b"]
    got = trainer(m)._text_inputs(caps)
    assert list(got) == ["token_batch"] and (got["token_batch"].rows, got["token_batch"].U, got["token_batch"].U_pad) == (4, 2, 8)
    again = trainer(m)._text_inputs(caps + ["d"])
    assert again["token_batch"].tokenizer_rows == 1                                       # the model's cache: only "d" was new
    off = trainer(m, text_dedup=False)._text_inputs(caps)["token_batch"]
    assert (off.U, off.U_pad, off.dedup) == (4, 4, False)
