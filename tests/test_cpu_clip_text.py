"""The CLIP text tower without a GPU: the torch-ops module against an independent fp64 restatement, its state-dict names, the
loader, the rule that decides the native route, the soundness of the two derived bounds of tests/clip_bounds.py (an fp32
emulation stays inside, wrong arithmetic does not) and the refusals of the library that return before any HIP call."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clip_bounds as CB
import hig_amd
from hig_amd import _lib
from hig_amd.models import clip_text as CT
from hig_amd.models import stub_clip


def small_tower(W=128, H=2, L=2, vocab=300, seed=3):
    sd = CB.tower_weights(W, H, L, 77, vocab, seed)
    m = CT.load_text_tower(sd)
    for p in m.parameters():
        p.requires_grad_(False)
    return sd, m


def test_torch_ops_module_equals_the_independent_fp64_restatement():
    sd, m = small_tower()
    tokens = CB.tower_tokens(3, 77, 300)
    got = m.double().features(tokens).permute(1, 0, 2)
    ref = CB.tower_fp64(sd, tokens, 2)
    assert got.dtype == torch.float64 and got.shape == ref.shape == (3, 77, 128)
    assert CB.rel_per_sample(got, ref).max().item() < 1e-12


def test_state_dict_names_are_openai_clips():
    m = CT.ClipTextModel(width=128, layers=2, heads=2, context_length=77, vocab_size=50, embed_dim=32)
    block = ["attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "ln_1.weight", "ln_1.bias",
             "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias", "ln_2.weight", "ln_2.bias"]
    want = ["positional_embedding", "text_projection", "logit_scale"]
    want += ["transformer.resblocks.%d.%s" % (i, k) for i in range(2) for k in block]
    want += ["token_embedding.weight", "ln_final.weight", "ln_final.bias"]
    assert list(m.state_dict()) == want
    assert m.text_projection.shape == (128, 32) and m.dtype == torch.float32
    assert abs(m.logit_scale.item() - math.log(1 / 0.07)) < 1e-6
    # CLIP's standard deviations
    g = torch.Generator().manual_seed(0)
    big = CT.ClipTextModel(width=512, layers=2, heads=8, vocab_size=2000)
    big.initialize_parameters(generator=g)
    b = big.transformer.resblocks[1]
    for t, std in ((big.token_embedding.weight, 0.02), (big.positional_embedding, 0.01), (b.attn.in_proj_weight, 512 ** -0.5),
                   (b.attn.out_proj.weight, 512 ** -0.5 * 4 ** -0.5), (b.mlp.c_fc.weight, 1024 ** -0.5), (b.mlp.c_proj.weight, 512 ** -0.5 * 4 ** -0.5)):
        assert abs(t.std().item() / std - 1) < 0.05
    assert torch.equal(b.attn_mask, CT.causal_mask(77)) and b.attn_mask[3, 4] == float("-inf") and b.attn_mask[4, 3] == 0


def test_load_text_tower_round_trips_a_prefixed_state_dict_with_a_visual_tower(tmp_path):
    sd, m = small_tower(L=3)
    ck = {"clip." + k: v.half() if i % 2 else v for i, (k, v) in enumerate(m.state_dict().items())}   # some fp16, as in OpenAI's archive
    ck["clip.visual.conv1.weight"] = torch.zeros(4, 3, 2, 2)
    ck["clip.input_resolution"] = torch.tensor(224)
    ck["text_ln.weight"] = torch.zeros(7)
    ck["out.weight"] = torch.zeros(7, 7)
    got = CT.load_text_tower(ck)
    assert (got.transformer.width, got.transformer.layers, got.transformer.heads, got.context_length, got.vocab_size) == (128, 3, 2, 77, 300)
    assert list(got.state_dict()) == list(m.state_dict()) and all(v.dtype == torch.float32 for v in got.state_dict().values())
    for k, v in m.state_dict().items():
        want = ck["clip." + k].float()
        assert torch.equal(got.state_dict()[k], want), k
    # OpenAI's own names, no prefix, no text_projection; and a file
    plain = {k: v for k, v in sd.items()}
    plain["visual.proj"] = torch.zeros(3, 3)
    torch.save({"state_dict": plain}, tmp_path / "tower.pt")
    again = CT.load_text_tower(str(tmp_path / "tower.pt"))
    assert all(torch.equal(again.state_dict()[k], v) for k, v in sd.items())
    with pytest.raises(ValueError, match="no CLIP text tower"):
        CT.load_text_tower({"visual.proj": torch.zeros(3, 3)})


def test_the_qualifying_rule():
    _, m = small_tower()
    assert CT.tower_refusal(m) is None
    assert "not on" in CT.tower_refusal(m, "cuda:0")                             # a host tower never takes the native route
    assert "resblocks" in CT.tower_refusal(stub_clip.StubCLIP())
    assert "fp32" in CT.tower_refusal(small_tower()[1].half())
    t = small_tower()[1]
    t.transformer.resblocks[1].mlp.c_fc.bias.requires_grad_(True)
    assert "requires grad" in CT.tower_refusal(t)
    t = CT.ClipTextModel(width=128, layers=1, heads=4, vocab_size=50)           # head dim 32
    for p in t.parameters():
        p.requires_grad_(False)
    assert "head dim 32" in CT.tower_refusal(t)
    for wrong in (None, torch.zeros(77, 77), CT.causal_mask(77).T.contiguous(), torch.full((77, 77), float("-inf")).triu_(2)):
        t = small_tower()[1]
        t.transformer.resblocks[0].attn_mask = wrong
        assert "attn_mask" in CT.tower_refusal(t)
    # the model: the stub, a host tower and a trainable tower all stay on the lines they ran before
    tokens = torch.zeros(2, 77, dtype=torch.int64)
    stub = hig_amd.MotionTransformer(input_feats=12, latent_dim=64, num_layers=1, num_heads=1)
    assert stub.clip_tower == "hip" and stub._clip_native_table(tokens) is None
    own = hig_amd.MotionTransformer(input_feats=12, latent_dim=64, num_layers=1, num_heads=1, clip_model=small_tower()[1],
                                    clip_tokenize=lambda text, truncate=False: tokens)
    assert own._clip_native_table(tokens) is None and not any(p.requires_grad for p in own.clip.parameters())
    assert "clip.transformer.resblocks.0.ln_1.weight" in own.state_dict() and not any("attn_mask" in k or "_clip" in k for k in own.state_dict())
    text, x = own._clip_features(["a", "b"], "cpu")                              # torch ops, through the supplied tokenizer
    assert torch.equal(text, tokens) and x.shape == (77, 2, 128)
    assert torch.equal(x, own.clip.features(tokens))
    with pytest.raises(ValueError, match="clip_tower"):
        hig_amd.MotionTransformer(input_feats=12, latent_dim=64, num_layers=1, num_heads=1, clip_tower="triton")


def test_quick_gelu_bound_is_sound_and_rejects_wrong_arithmetic():
    z = CB.quick_gelu_grid(200001, seed=1)
    ref, bound = CB.quick_gelu_ref(z), CB.quick_gelu_bound(z)
    worst = lambda y: ((torch.from_numpy(np.asarray(y)).double() - ref).abs() / bound).max().item()   # noqa: E731
    inside = worst(CB.quick_gelu_f32(z.numpy()))
    print("QuickGELU fp32 emulation: %.3f of the bound" % inside)
    assert inside <= 1.0
    z64 = z.double()
    wrong = {"constant 1.7": CB.quick_gelu_f32(z.numpy(), c=1.7),
             "exact GELU": (0.5 * z64 * (1 + torch.erf(z64 / math.sqrt(2)))).float().numpy(),
             "tanh GELU": (0.5 * z64 * (1 + torch.tanh(math.sqrt(2 / math.pi) * (z64 + 0.044715 * z64 ** 3)))).float().numpy()}
    for name, y in wrong.items():
        assert worst(y) > 100, name
    # the bound is a few roundings where the function is well conditioned
    mid = (z.abs() >= 1e-3) & (z.abs() <= 8)
    assert (bound[mid] / (CB.U * ref[mid].abs())).max().item() < 40


@pytest.mark.parametrize("B, H, N, spread", [(2, 2, 33, None), (1, 2, 77, None), (1, 2, 128, 40.0)])
def test_causal_bound_is_sound_and_rejects_wrong_arithmetic(B, H, N, spread):
    qkv = CB.causal_inputs(B, H, N, seed=N, spread=spread)
    q, k, v = CB.split_qkv(qkv, B, N, H)
    r = CB.causal_reference(q, k, v)
    assert r["spread"] <= 80 and (spread is None or abs(r["spread"] - spread) < 1e-3 * spread)
    bound = CB.causal_bound(r)
    worst = lambda y: ((torch.as_tensor(y).double() - r["y"]).abs() / bound).max().item()   # noqa: E731
    inside = worst(CB.causal_f32(q.numpy(), k.numpy(), v.numpy()))
    print("causal attention fp32 emulation (B %d H %d N %d): %.3f of the bound" % (B, H, N, inside))
    assert inside <= 1.0
    assert worst(CB.causal_f32(q.numpy(), k.numpy(), v.numpy(), shift=1)) > 100                       # key n + 1 in the softmax
    assert worst(CB.causal_f32(q.numpy(), k.numpy(), v.numpy(), scale=1 / math.sqrt(H * CB.HD))) > 100   # 1 / sqrt(W)
    assert worst(CB.causal_reference(q, k, v, shift=1)["y"]) > 100
    assert torch.equal(r["y"][:, 0], v[:, 0].double())                                                # row 0 is V's row 0


def test_workspace_size_and_the_refusals_need_no_device():
    L = _lib.lib()
    al = lambda n: (n + 63) // 64 * 64   # noqa: E731
    for B, N, W, H in ((1, 77, 512, 8), (3, 77, 128, 2), (2, 128, 1024, 16), (5, 1, 64, 1)):
        M = B * N
        want = al(M * W) + al(M * 2) + 2 * (4 * al(M * W) + al(M * 2) + al(M * 3 * W) + al(M * 4 * W))
        assert L.hig_clip_text_workspace_bytes(CT.clip_dims(B, N, W, H, 12, 49408)) == 4 * want
    assert _lib.CD_NSLOTS == 7 and _lib.CT_NGLOBAL == 4 and _lib.CTL_NLAYER == 12
    for dims, code, word in ((CT.clip_dims(1, 77, 512, 16, 12, 49408), _lib.EUNSUPPORTED, "head dim 32"),
                             (CT.clip_dims(1, 129, 512, 8, 12, 49408), _lib.EUNSUPPORTED, "N=129"),
                             (CT.clip_dims(1, 77, 500, 8, 12, 49408), _lib.EINVAL, "divisible"),
                             (CT.clip_dims(0, 77, 512, 8, 12, 49408), _lib.EINVAL, "positive"),
                             (CT.clip_dims(1, 77, 512, 8, 12, 49408, prec=7), _lib.EINVAL, "prec")):
        assert L.hig_clip_text_workspace_bytes(dims) == -1 and word in _lib.last_error()
        table = (C.c_void_p * (4 + 12 * 12))(*([8] * (4 + 12 * 12)))
        assert L.hig_clip_text_fwd(dims, table, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None) == code and word in _lib.last_error()
    good = CT.clip_dims(1, 77, 512, 8, 12, 49408)
    assert L.hig_clip_text_workspace_bytes(None) == -1
    assert L.hig_clip_text_fwd(good, None, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None) == _lib.EINVAL
    assert L.hig_clip_text_fwd(good, table, None, C.c_void_p(8), C.c_void_p(8), None) == _lib.EINVAL and "null" in _lib.last_error()
    table[5] = None
    assert L.hig_clip_text_fwd(good, table, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None) == _lib.EINVAL and "parameter 5" in _lib.last_error()
    p = C.c_void_p(16)
    assert L.hig_causal_attn_fwd(p, 64, p, p, 64, 1, 129, 1, p, 64, None) == _lib.EUNSUPPORTED and "N=129" in _lib.last_error()
    assert L.hig_causal_attn_fwd(None, 64, p, p, 64, 1, 77, 1, p, 64, None) == _lib.EINVAL
    assert L.hig_causal_attn_fwd(p, 64, p, p, 64, 1, 77, 2, p, 128, None) == _lib.EINVAL and "leading" in _lib.last_error()
    assert L.hig_clip_embed(None, p, p, 1, 77, 512, 10, p, 512, None) == _lib.EINVAL
    assert L.hig_clip_embed(p, p, p, 1, 77, 512, 10, p, 511, None) == _lib.EINVAL
    assert L.hig_quick_gelu(None, 4, None) == _lib.EINVAL and L.hig_quick_gelu(p, -1, None) == _lib.EINVAL
    assert L.hig_quick_gelu(p, 0, None) == 0 and L.hig_clip_embed(p, p, p, 0, 77, 512, 10, p, 512, None) == 0
