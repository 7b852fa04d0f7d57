"""The CLIP text tower's adjoint without a GPU: the bounds of tests/clip_train_bounds.py against fp32 emulations of the kernels'
arithmetic and against wrong arithmetic, the fp64 statements against torch.autograd, the embedding index against a plain
restatement, the qualifying rule, the option's default and every new entry's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import clip_bounds as CB
import clip_train_bounds as TB
import hig_amd
from hig_amd import _lib
from hig_amd.models import clip_text as CT
from hig_amd.models import stub_clip
from oracle import fill


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------
def _ratios(got, r, b):
    return {n: ((torch.from_numpy(np.asarray(g)).double() - r[n]).abs() / b[n]).max().item() for n, g in zip(("dQ", "dK", "dV"), got)}


@pytest.mark.parametrize("B, H, N, spread", [(2, 2, 33, None), (1, 1, 77, None), (1, 2, 77, 40.0), (1, 1, 128, None)])
def test_causal_backward_bound_is_sound_and_rejects_wrong_arithmetic(B, H, N, spread):
    qkv, dy, lse, y, fwd = TB.causal_bwd_inputs(B, H, N, seed=N + B, spread=spread)
    q, k, v = CB.split_qkv(qkv, B, N, H)
    dy4, y4 = dy.reshape(B, N, H, CB.HD), y.reshape(B, N, H, CB.HD)
    r = TB.causal_bwd_reference(q, k, v, dy4, lse, y4)
    b = TB.causal_bwd_bounds(r)
    good = _ratios(TB.causal_bwd_f32(q, k, v, dy4, lse, y4), r, b)
    print("causal backward B %d H %d N %d spread %s: fp32 emulation |err| / bound %s" % (B, H, N, spread, good))
    assert max(good.values()) <= 1.0
    # the lse the forward hands over, emulated in fp32, within its own bound
    s32 = (np.einsum("bnhd,bmhd->bhnm", q.numpy(), k.numpy()).astype(np.float32) * np.float32(0.125)).astype(np.float32)
    s32 = np.where(fwd["live"].numpy(), s32, -np.inf)
    mx = s32.max(-1)
    lse32 = mx + np.log(np.exp(s32 - mx[..., None]).astype(np.float32).sum(-1, dtype=np.float32)).astype(np.float32)
    assert ((torch.from_numpy(lse32).double() - fwd["lse"]).abs() / TB.lse_bound(fwd)).max() <= 1.0
    assert ((fwd["lse"] + 1e-3 - fwd["lse"]).abs() / TB.lse_bound(fwd)).max() > 1.0
    wrong = {"key n + 1 included": dict(shift=1), "no delta": dict(with_delta=False), "no 1/8 on dK": dict(dk_scale=1.0),
             "1 / sqrt(W)": dict(scale=1.0 / (H * CB.HD) ** 0.5)}
    for what, kw in wrong.items():
        if what == "1 / sqrt(W)" and H == 1:
            continue                                                                   # W == 64: the same scale
        bad = _ratios(TB.causal_bwd_f32(q, k, v, dy4, lse, y4, **kw), r, b)
        print("    %s: %s" % (what, bad))
        assert max(bad.values()) > 1.0, what
        if what == "no 1/8 on dK":
            assert bad["dK"] > 1.0 and bad["dQ"] <= 1.0 and bad["dV"] <= 1.0


def test_quick_gelu_backward_bound_is_sound_and_rejects_wrong_arithmetic():
    z = CB.quick_gelu_grid(200001)
    g = torch.Generator().manual_seed(3)
    dy = torch.randn(z.shape, generator=g) * 10.0 ** (torch.rand(z.shape, generator=g) * 4 - 2)
    ref, bound = TB.quick_gelu_grad_ref(z, dy), TB.quick_gelu_grad_bound(z, dy)
    ratio = lambda got: ((torch.from_numpy(got).double() - ref).abs() / bound).max().item()   # noqa: E731
    good = ratio(TB.quick_gelu_grad_f32(z.numpy(), dy.numpy()))
    print("QuickGELU backward: fp32 emulation |err| / bound = %.3f" % good)
    assert good <= 1.0
    assert ratio(TB.quick_gelu_grad_f32(z.numpy(), dy.numpy(), c=1.7)) > 1.0
    assert ratio(TB.quick_gelu_grad_f32(z.numpy(), dy.numpy(), drop_one_minus_s=True)) > 1.0
    # the derivative against autograd on the torch-ops module
    zz = z[:4096].double().requires_grad_(True)
    CT.QuickGELU()(zz).backward(dy[:4096].double())
    assert torch.allclose(zz.grad, ref[:4096], rtol=1e-12, atol=1e-300)


# ---- the fp64 statements against autograd -----------------------------------------------------------------------------------------------
def test_the_fp64_adjoint_equals_autograd_on_the_torch_ops_module():
    W, H, L, N, vocab, B = 128, 2, 2, 9, 40, 3
    sd = CB.tower_weights(W, H, L, N, vocab, seed=2)
    tokens = CB.tower_tokens(B, N, vocab, seed=2)
    dout = TB.upstream(B, N, W)
    mine = TB.tower_adjoint_fp64(sd, tokens, H, dout)
    m = CT.load_text_tower(sd).double()
    (m.features(tokens).permute(1, 0, 2) * dout.double()).sum().backward()
    auto = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert set(mine) == set(auto) == set(sd)
    for name in sd:
        scale = auto[name].abs().max().item()
        assert (mine[name] - auto[name]).abs().max().item() <= 1e-10 * max(scale, 1.0), name
    for i in range(L):   # the key third of the in-projection's bias: exactly zero in exact arithmetic
        gb = auto["transformer.resblocks.%d.attn.in_proj_bias" % i]
        assert gb[W:2 * W].abs().max() < 1e-12 * gb.abs().max()


# ---- the embedding index ------------------------------------------------------------------------------------------------------------------
def embed_case(W, seed=0):
    """(tokens (B, N), vocab): ids repeated 1, 2, C, C + 1 and 3 C + 5 times and two ids out of range."""
    Cn = _lib.CLIP_EMBED_CHUNK
    vocab, N = 64, 11
    reps = {3: 1, 9: 2, 17: Cn, 30: Cn + 1, 0: 3 * Cn + 5}
    ids = [t for t, n in reps.items() for _ in range(n)] + [vocab, -1]
    ids += [41] * (-len(ids) % N)
    g = torch.Generator().manual_seed(seed)
    ids = torch.tensor(ids)[torch.randperm(len(ids), generator=g)]
    return ids.view(-1, N), vocab, reps


def test_the_embedding_index_against_a_plain_restatement():
    Cn = _lib.CLIP_EMBED_CHUNK
    tokens, vocab, reps = embed_case(6)
    B, N = tokens.shape
    ix = CT.EmbedIndex(tokens, vocab)
    lists = TB.embed_index_restated(tokens, vocab, Cn)
    assert ix.chunk == Cn and ix.n_ids == len(lists) and ix.n_live == B * N - 2
    assert ix.host.dtype == torch.int32 and ix.host.numel() == _lib.lib().hig_clip_embed_index_ints(B, N, ix.n_live, ix.n_chunks, ix.n_ids)
    assert list(ix.ids) == sorted(lists) and list(ix.chunk_order) == list(range(ix.n_chunks))
    for u, t in enumerate(ix.ids):
        chunks = [list(ix.order[ix.chunk_seg[c]:ix.chunk_seg[c + 1]]) for c in range(ix.id_seg[u], ix.id_seg[u + 1])]
        assert chunks == lists[int(t)]
        rows = sum(chunks, [])
        assert rows == sorted(rows) and all(tokens.view(-1)[r] == t for r in rows)
        assert [len(c) for c in chunks[:-1]] == [Cn] * (len(chunks) - 1) and 1 <= len(chunks[-1]) <= Cn
    assert {t: len(lists[t]) for t in reps} == {3: 1, 9: 1, 17: 1, 30: 2, 0: 4}       # lengths 1, 2, C, C + 1, 3 C + 5
    assert vocab not in lists and -1 not in lists
    assert list(ix.pos_seg) == [n * B for n in range(N + 1)]
    assert list(ix.pos_order) == [b * N + n for n in range(N) for b in range(B)]
    # the chunked sum: the module's restatement over the index equals the one over the plain lists, and it is NOT the
    # unchunked running sum where a list is longer than a chunk
    g = torch.Generator().manual_seed(1)
    dx0 = (torch.randn(B * N, 6, generator=g) * 10.0 ** (torch.rand(B * N, 1, generator=g) * 8 - 4)).numpy()
    dtok, dpos = CT.embed_grad_restated(dx0, ix, 6)
    assert np.array_equal(dtok, TB.embed_grad_from_lists(dx0, lists, vocab))
    assert np.array_equal(dpos, np.stack([dx0.reshape(B, N, 6)[:, n].cumsum(0, dtype=np.float32)[-1] for n in range(N)]))
    unused = sorted(set(range(vocab)) - set(lists))
    assert not dtok[unused].any() and not np.signbit(dtok[unused]).any()
    running = np.zeros(6, np.float32)
    for r in sum(lists[0], []):
        running = (running + dx0[r]).astype(np.float32)
    assert not np.array_equal(running, dtok[0]) and np.allclose(running, dtok[0], rtol=1e-4, atol=1e-2)
    empty = CT.EmbedIndex(torch.full((2, 3), -5), vocab)
    assert (empty.n_live, empty.n_chunks, empty.n_ids) == (0, 0, 0) and list(empty.chunk_seg) == [0] and list(empty.id_seg) == [0]


# ---- the rule and the option -------------------------------------------------------------------------------------------------------------
def test_the_trainable_rule_and_the_unchanged_default():
    m = CT.load_text_tower(CB.tower_weights(128, 2, 2, 77, 64, seed=1))
    assert all(p.requires_grad for p in m.parameters())
    assert CT.tower_refusal(m) == "a tower parameter requires grad (the backward is not built)"
    assert CT.tower_refusal(m, None) == CT.tower_refusal(m, trainable=False)
    assert CT.tower_refusal(m, trainable=True) is None
    for p in m.parameters():
        p.requires_grad_(False)
    assert CT.tower_refusal(m) is None and CT.tower_refusal(m, trainable=True) is None
    for p in m.parameters():
        p.requires_grad_(True)
    assert "not fp32" in CT.tower_refusal(CT.load_text_tower(CB.tower_weights(128, 2, 1, 77, 64)).half(), trainable=True)
    assert "head dim" in CT.tower_refusal(CT.ClipTextModel(128, 1, 4, 77, 64, 128), trainable=True)
    wide = CT.ClipTextModel(64, 1, 1, 129, 64, 64)
    assert "129 tokens" in CT.tower_refusal(wide, trainable=True)
    m.transformer.resblocks[1].attn_mask = torch.zeros(77, 77)
    assert "causal" in CT.tower_refusal(m, trainable=True)
    m.transformer.resblocks[1].attn_mask = CT.causal_mask(77)
    assert CT.tower_refusal(m, trainable=True) is None
    assert "lives on" in CT.tower_refusal(m, "cuda:0", trainable=True)
    assert "resblocks" in CT.tower_refusal(stub_clip.StubCLIP(), trainable=True)
    with pytest.raises(CT.TowerRefused):
        CT.TrainTowerTable(m, "cuda:0")
    assert issubclass(CT.TrainTowerTable, CT.TowerTable) and CT.TrainTowerTable.TRAINABLE and not CT.TowerTable.TRAINABLE


def _two_person(**kw):
    c = fill.CASES["config1"]
    tower = CT.load_text_tower(CB.tower_weights(512, 8, 1, 77, stub_clip.VOCAB, seed=11))
    return hig_amd.MotionInteractionTransformer(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                                num_layers=1, num_heads=c["H"], text_latent_dim=c["Lt"], no_clip=True,
                                                clip_model=tower, clip_tokenize=stub_clip.tokenize, **kw)


def test_the_option_defaults_to_torch(monkeypatch):
    monkeypatch.delenv("HIG_CLIP_TOWER_TRAIN", raising=False)
    m = _two_person()
    assert m.clip_tower_train == "torch" and m.clip_train_stats == {"native_forwards": 0, "native_backwards": 0, "native_inference": 0}
    assert _two_person(clip_tower_train="hip").clip_tower_train == "hip"
    monkeypatch.setenv("HIG_CLIP_TOWER_TRAIN", "hip")
    assert _two_person().clip_tower_train == "hip"
    with pytest.raises(ValueError):
        _two_person(clip_tower_train="triton")
    # on the CPU the option changes nothing: the torch lines run, the graph reaches the tower
    m = _two_person(clip_tower_train="hip", text_head="torch")
    xf_proj, xf_out = m.encode_text(["a person waves"], "cpu")
    xf_proj.sum().backward()
    assert m.clip.transformer.resblocks[0].mlp.c_fc.weight.grad is not None and m.clip_train_stats["native_forwards"] == 0


# ---- the entries' refusals, before any HIP call -------------------------------------------------------------------------------------------
def test_every_new_entry_refuses_without_a_device():
    L = _lib.lib()
    p = C.c_void_p(16)
    E, Uu = _lib.EINVAL, _lib.EUNSUPPORTED
    # hig_causal_attn_fwd_train
    assert L.hig_causal_attn_fwd_train(p, 64, p, p, 64, 1, 77, 1, p, 64, None, None) == E and "lse" in _lib.last_error()
    assert L.hig_causal_attn_fwd_train(p, 64, p, p, 64, 1, 129, 1, p, 64, p, None) == Uu and "N=129" in _lib.last_error()
    assert L.hig_causal_attn_fwd_train(p, 64, p, p, 63, 1, 77, 1, p, 64, p, None) == E and "leading" in _lib.last_error()
    # hig_causal_attn_bwd(dY, lddy, Y, ldy, Q, ldq, K, V, ldk, B, N, H, hd, lse, delta, dQ, lddq, dK, dV, lddk, stream)
    bwd = lambda **kw: L.hig_causal_attn_bwd(*[kw.get(n, d) for n, d in (   # noqa: E731
        ("dY", p), ("lddy", 64), ("Y", p), ("ldy", 64), ("Q", p), ("ldq", 64), ("K", p), ("V", p), ("ldk", 64), ("B", 1), ("N", 77), ("H", 1),
        ("hd", 64), ("lse", p), ("delta", p), ("dQ", p), ("lddq", 64), ("dK", p), ("dV", p), ("lddk", 64), ("stream", None))])
    assert bwd(N=129) == Uu and "N=129" in _lib.last_error()
    assert bwd(hd=32) == Uu and "head dim 32" in _lib.last_error()
    assert bwd(lse=None) == E and bwd(delta=None) == E and bwd(dV=None) == E and bwd(N=0) == E and bwd(B=-1) == E
    assert bwd(H=2) == E and "leading" in _lib.last_error()
    assert bwd(lddq=63) == E and bwd(lddk=0) == E
    assert bwd(B=0) == 0                                                               # nothing to do, nothing launched
    # the QuickGELU pair
    assert L.hig_quick_gelu_bwd(None, p, p, 4, None) == E and L.hig_quick_gelu_bwd(p, None, p, 4, None) == E
    assert L.hig_quick_gelu_bwd(p, p, None, 4, None) == E and L.hig_quick_gelu_bwd(p, p, p, -1, None) == E
    assert L.hig_quick_gelu_bwd(p, p, p, 0, None) == 0
    assert L.hig_quick_gelu_to(None, p, 4, None) == E and L.hig_quick_gelu_to(p, None, 4, None) == E and L.hig_quick_gelu_to(p, p, -1, None) == E
    assert L.hig_quick_gelu_to(p, p, 0, None) == 0
    # hig_clip_embed_bwd(dx0, B, N, W, vocab, index, n_live, n_chunks, n_ids, scratch, dtok, dpos, stream)
    emb = lambda **kw: L.hig_clip_embed_bwd(*[kw.get(n, d) for n, d in (   # noqa: E731
        ("dx0", p), ("B", 2), ("N", 77), ("W", 512), ("vocab", 100), ("index", p), ("n_live", 100), ("n_chunks", 40), ("n_ids", 30),
        ("scratch", p), ("dtok", p), ("dpos", p), ("stream", None))])
    assert emb(dx0=None) == E and emb(index=None) == E and emb(scratch=None) == E and emb(dtok=None) == E and emb(dpos=None) == E
    assert emb(W=0) == E and emb(vocab=0) == E and emb(B=-1) == E
    assert emb(n_live=155) == E and "counts" in _lib.last_error()
    assert emb(n_chunks=101) == E and emb(n_ids=41) == E and emb(n_ids=0) == E and emb(n_live=-1) == E
    assert emb(index=C.c_void_p(18)) == E and "unaligned" in _lib.last_error()
    assert L.hig_clip_embed_index_ints(2, 77, 100, 40, 30) == 100 + 41 + 40 + 31 + 30 + 154 + 78
    assert L.hig_clip_embed_index_ints(2, 77, -1, 0, 0) == -1
    # the tower's training pair
    n_tab = 4 + 12 * 12
    table = (C.c_void_p * n_tab)(*([8] * n_tab))
    good = CT.clip_dims(2, 77, 512, 8, 12, 49408)
    for dims, code, word in ((CT.clip_dims(1, 77, 512, 16, 12, 49408), Uu, "head dim 32"), (CT.clip_dims(1, 129, 512, 8, 12, 49408), Uu, "N=129"),
                             (CT.clip_dims(1, 77, 512, 8, 12, 49408, prec=1), Uu, "exact fp32"), (CT.clip_dims(1, 77, 512, 8, 12, 49408, prec=2), Uu, "exact fp32"),
                             (CT.clip_dims(1, 77, 500, 8, 12, 49408), E, "divisible"), (CT.clip_dims(0, 77, 512, 8, 12, 49408), E, "positive")):
        assert L.hig_clip_text_train_bytes(dims) == -1 and word in _lib.last_error()
        assert L.hig_clip_text_bwd_workspace_bytes(dims) == -1 and word in _lib.last_error()
        assert L.hig_clip_text_fwd_train(dims, table, p, p, p, None) == code and word in _lib.last_error()
        assert L.hig_clip_text_bwd(dims, table, p, 10, 5, 5, p, p, table, p, None) == code and word in _lib.last_error()
    assert L.hig_clip_text_fwd_train(good, None, p, p, p, None) == E and L.hig_clip_text_fwd_train(good, table, None, p, p, None) == E
    assert L.hig_clip_text_fwd_train(good, table, p, None, p, None) == E and L.hig_clip_text_fwd_train(good, table, p, p, None, None) == E
    table[5] = None
    assert L.hig_clip_text_fwd_train(good, table, p, p, p, None) == E and "parameter 5" in _lib.last_error()
    full = (C.c_void_p * n_tab)(*([8] * n_tab))
    assert L.hig_clip_text_bwd(good, full, p, 10, 5, 5, p, p, table, p, None) == E and "gradient 5" in _lib.last_error()
    assert L.hig_clip_text_bwd(good, full, None, 10, 5, 5, p, p, full, p, None) == E and L.hig_clip_text_bwd(good, full, p, 10, 5, 5, None, p, full, p, None) == E
    assert L.hig_clip_text_bwd(good, full, p, 10, 5, 5, p, None, full, p, None) == E and L.hig_clip_text_bwd(good, full, p, 10, 5, 5, p, p, None, p, None) == E
    assert L.hig_clip_text_bwd(good, full, p, 10, 5, 5, p, p, full, None, None) == E
    assert L.hig_clip_text_bwd(good, full, p, 155, 5, 5, p, p, full, p, None) == E and "counts" in _lib.last_error()
    # what the training forward keeps: N (W + 2) + L N (10 W + 4 + H) floats per caption (include/hig.h), in 256-byte granules
    per = 77 * (512 + 2) + 12 * 77 * (10 * 512 + 4 + 8)
    assert per * 4 == 19126184
    one, two = L.hig_clip_text_train_bytes(CT.clip_dims(1, 77, 512, 8, 12, 49408)), L.hig_clip_text_train_bytes(CT.clip_dims(33, 77, 512, 8, 12, 49408))
    assert 0 <= (two - one) / 32 - (per + 77 * 5 * 512) * 4 < 64 * 256
    assert L.hig_clip_text_bwd_workspace_bytes(good) > 0
