"""The class head of cap_id models without a GPU: the `class_head` option, the argument checks of the new entry points
(hig_rows_sum_by_key_f32 in csrc/textrows.hip, hig_class_head_* in csrc/classhead.hip), the flat-buffer layout with the option
on and off, and an fp64 restatement of the per-class forward and backward that csrc/classhead.hip launches, held against
torch.autograd of text_proj(cap_embedding[ids]).  The launches themselves need the device (tests/test_gpu_class_head.py)."""
import ctypes as C
import types

import pytest
import torch

import hig_amd
from hig_amd import _lib
from hig_amd.models import stub_clip
from hig_amd.models.transformer import _FlatParams


def tiny(**kw):
    return hig_amd.MotionInteractionTransformer(input_feats=12, num_frames=16, latent_dim=64, ff_size=128, num_layers=2, num_heads=8,
                                                text_latent_dim=32, **kw)


def test_option_default_values_and_refusal(monkeypatch):
    monkeypatch.delenv("HIG_CLASS_HEAD", raising=False)
    assert tiny(cap_id=True).class_head == "torch" and not tiny(cap_id=True)._has_hip_class_head()
    on = tiny(cap_id=True, class_head="hip")
    assert on.class_head == "hip" and on._has_hip_class_head()
    assert [tuple(p.shape) for p in on._class_params()] == [(43, 32), (256, 32), (256,)]
    with pytest.raises(ValueError, match="class_head"):
        tiny(cap_id=True, class_head="triton")
    monkeypatch.setenv("HIG_CLASS_HEAD", "hip")
    assert tiny(cap_id=True)._has_hip_class_head()
    assert tiny(cap_id=True, class_head="torch").class_head == "torch"          # the argument wins over the environment
    monkeypatch.setenv("HIG_CLASS_HEAD", "nope")
    with pytest.raises(ValueError, match="class_head"):
        tiny(cap_id=True)
    # the single-person model has no class head at all
    assert not hig_amd.MotionTransformer._has_hip_class_head(on)


def test_flat_buffer_places_the_class_head_behind_the_core_only_with_the_option():
    off = tiny(cap_id=True)
    names = list(off.state_dict())
    shapes = {k: tuple(v.shape) for k, v in off.state_dict().items()}
    fp_off = _FlatParams(off)
    assert fp_off.text_params == [] and fp_off.numel == fp_off.core_numel
    on = tiny(cap_id=True, class_head="hip")
    on.load_state_dict(off.state_dict(), strict=True)
    fp = _FlatParams(on)
    assert fp.core_numel == fp_off.core_numel
    assert [id(p) for p in fp.text_params] == [id(p) for p in on._class_params()]
    assert fp.text_offsets[0] == fp.core_numel and all(o % _FlatParams.ALIGN == 0 for o in fp.text_offsets)
    assert fp.numel == fp.text_offsets[-1] + 256 and fp.numel > fp.core_numel
    for p, o in zip(fp.text_params, fp.text_offsets):
        assert p.data_ptr() == fp.flat.data_ptr() + 4 * o
    # state-dict names and shapes do not move, and the values went into the buffer unchanged
    assert list(on.state_dict()) == names and {k: tuple(v.shape) for k, v in on.state_dict().items()} == shapes
    for k, v in off.state_dict().items():
        assert torch.equal(on.state_dict()[k], v), k
    # a checkpoint of the option-on model loads into a default-built one
    tiny(cap_id=True).load_state_dict(on.state_dict(), strict=True)
    # without cap_id the option has no effect
    plain = tiny(class_head="hip", clip_model=stub_clip.StubCLIP(), clip_tokenize=stub_clip.tokenize, text_ff_size=64,
                 num_text_layers=1)
    assert not plain._has_hip_class_head()
    assert len(_FlatParams(plain).text_params) == len(plain._text_params())      # (the text head, as for every caption model)


def test_state_dict_of_the_option_on_model_is_the_reference_cap_id_contract(gold):
    """Names in order and shapes of the reference's MotionInteractionTransformer(cap_id=True) (golden g21, `keys.*`): what a
    checkpoint written with class_head="hip" needs to load into the reference with strict=True."""
    from oracle import fill
    g = gold("g21_class_pit.npz")
    c = fill.ICASES["config1x2"]
    keys = [k[5:] for k in g.files if k.startswith("keys.")]
    assert "cap_embedding" in keys and "text_proj.0.weight" in keys and not any(k.startswith("clip.") for k in keys)
    for kw in (dict(), dict(class_head="hip")):
        m = hig_amd.MotionInteractionTransformer(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                                 num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"], cap_id=True, **kw)
        _FlatParams(m)                     # (re-homing the parameters into the flat buffer moves no name and no shape)
        sd = m.state_dict()
        assert list(sd) == keys
        assert all(tuple(sd[k].shape) == tuple(g["keys." + k]) for k in keys)


def test_new_entry_points_refuse_bad_arguments_before_any_device_call():
    L = _lib.lib()
    EINVAL = _lib.EINVAL
    raw = (C.c_float * 512)()
    base = (C.addressof(raw) + 15) // 16 * 16
    p = [C.c_void_p(base + 64 * i) for i in range(12)]

    def bykey(src=p[0], key=p[1], rows=4, row_floats=4, n_keys=3, dst=p[2]):
        return L.hig_rows_sum_by_key_f32(src, key, rows, row_floats, n_keys, dst, None)

    def fwd(classes=43, Lt=32, E=64, rows=4, emb=p[0], W=p[1], b=p[2], ids=p[3], xf_out=p[4], xf_proj=p[5], workspace=p[6]):
        return L.hig_class_head_fwd(classes, Lt, E, rows, emb, W, b, ids, xf_out, xf_proj, workspace, None)

    def bwd(classes=43, Lt=32, E=64, rows=4, emb=p[0], W=p[1], ids=p[2], dxf_out=p[3], dxf_proj=p[4], g_emb=p[5], g_W=p[6], g_b=p[7],
            workspace=p[8]):
        return L.hig_class_head_bwd(classes, Lt, E, rows, emb, W, ids, dxf_out, dxf_proj, g_emb, g_W, g_b, workspace, None)

    cases = ((bykey, "hig_rows_sum_by_key_f32", ("src", "key", "dst"), ("rows", "row_floats", "n_keys")),
             (fwd, "hig_class_head_fwd", ("emb", "W", "b", "ids", "xf_out", "xf_proj", "workspace"), ("classes", "Lt", "E", "rows")),
             (bwd, "hig_class_head_bwd", ("emb", "W", "ids", "g_emb", "g_W", "g_b", "workspace"), ("classes", "Lt", "E", "rows")))
    for fn, name, pointers, sizes in cases:
        for q in pointers:
            assert fn(**{q: None}) == EINVAL, "%s accepts %s = NULL" % (name, q)
            assert name in _lib.last_error()
        for s in sizes:
            for bad in (0, -1):
                assert fn(**{s: bad}) == EINVAL, "%s accepts %s = %d" % (name, s, bad)
                assert name in _lib.last_error()
    assert bykey(key=C.c_void_p(p[1].value + 2)) == EINVAL and bykey(dst=C.c_void_p(p[2].value + 1)) == EINVAL
    assert fwd(Lt=30) == EINVAL and bwd(E=62) == EINVAL
    # the size query: positive, the backward's is the larger, -1 for what the entries refuse
    f, b = L.hig_class_head_workspace_bytes(43, 256, 2048, 0), L.hig_class_head_workspace_bytes(43, 256, 2048, 1)
    assert f >= 43 * 2048 * 4 and b >= 43 * (2048 + 256) * 4 and f % 256 == 0 and b % 256 == 0
    for bad in ((0, 256, 2048), (43, 0, 2048), (43, 256, -4), (43, 254, 2048)):
        assert L.hig_class_head_workspace_bytes(*bad, 0) == -1 and L.hig_class_head_workspace_bytes(*bad, 1) == -1
    assert _lib.ROWS_KEY_CHUNK == 1024


def restated_forward(emb, W, b, ids):
    """What hig_class_head_fwd launches, in the order it launches it: text_proj once per class, then two gathers."""
    P = emb @ W.t() + b
    return P[ids], emb[ids].unsqueeze(1)


def restated_backward(emb, W, ids, dxf_out, dxf_proj):
    """What hig_class_head_bwd launches: the two sums by id in ascending row order, then three (C, .) products."""
    classes = emb.shape[0]
    dP = torch.zeros(classes, dxf_proj.shape[1], dtype=emb.dtype)
    dO = torch.zeros(classes, emb.shape[1], dtype=emb.dtype)
    for r, k in enumerate(ids.tolist()):
        dP[k] += dxf_proj[r]
        dO[k] += dxf_out[r, 0]
    return dO + dP @ W, dP.t() @ emb, dP.sum(dim=0)


@pytest.mark.parametrize("ids", [[3, 41, 4, 3], [7, 7, 7, 7, 7, 7], [0, 42, 42, 1, 0, 5, 41, 41]])
def test_per_class_restatement_equals_autograd_of_the_per_row_head(ids):
    """Repeated ids (their gradients add) and unused classes (their rows of g_emb are exactly zero)."""
    g = torch.Generator().manual_seed(len(ids))
    classes, Lt, E = 43, 32, 128
    emb = torch.randn(classes, Lt, generator=g, dtype=torch.float64, requires_grad=True)
    W = torch.randn(E, Lt, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(E, generator=g, dtype=torch.float64, requires_grad=True)
    ids = torch.tensor(ids)
    xo = emb[ids]
    xp = torch.nn.functional.linear(xo, W, b)
    rp = torch.randn(xp.shape, generator=g, dtype=torch.float64)
    ro = torch.randn(len(ids), 1, Lt, generator=g, dtype=torch.float64)
    ((xp * rp).sum() + (xo.unsqueeze(1) * ro).sum()).backward()
    with torch.no_grad():
        xf_proj, xf_out = restated_forward(emb, W, b, ids)
        g_emb, g_W, g_b = restated_backward(emb, W, ids, ro, rp)

    def close(a, ref):
        return (a - ref).norm().item() <= 1e-12 * max(ref.norm().item(), 1e-300)

    assert close(xf_proj, xp.detach()) and torch.equal(xf_out[:, 0], xo.detach())
    assert close(g_emb, emb.grad) and close(g_W, W.grad) and close(g_b, b.grad)
    unused = sorted(set(range(classes)) - set(ids.tolist()))
    assert unused and g_emb[unused].abs().max().item() == 0.0 and emb.grad[unused].abs().max().item() == 0.0


def test_trainer_refuses_class_ids_beside_other_text_arguments_and_without_the_option():
    opt = types.SimpleNamespace(device="cpu", diffusion_steps=1000, is_train=False, multi=True, label_path=None, cap_id=True)
    tr = hig_amd.DDPMMulTrainer(opt, tiny(cap_id=True, class_head="hip"))
    ids = torch.zeros(4, dtype=torch.int32)
    tr._text_source(None, None, None, None, None, None)
    for kw in (dict(xf_proj=torch.zeros(1)), dict(xf_out=torch.zeros(1)), dict(clip_out=torch.zeros(1)), dict(eot=torch.zeros(1)),
               dict(caption_batch=object())):
        args = dict(xf_proj=None, xf_out=None, clip_out=None, eot=None, caption_batch=None)
        args.update(kw)
        # (the steps refuse a caption_batch= without a bank before they look at the ids: a stand-in bank lets the ids' refusal show)
        tr.encoder._caption_bank = object() if "caption_batch" in kw else None
        with pytest.raises(ValueError, match="exclusive"):
            tr._text_source(class_ids=ids, **args)
    tr.encoder._caption_bank = None
    with pytest.raises(ValueError, match="int32"):      # (a host tensor: the ids must already be on the device)
        tr._text_source(None, None, None, None, None, ids)
    off = hig_amd.DDPMMulTrainer(opt, tiny(cap_id=True))
    with pytest.raises(RuntimeError, match="class_head='hip'"):
        off._text_source(None, None, None, None, None, ids)
