"""The CLIP text tower on the MI355X (csrc/cliptext.hip): the three kernels against fp64 under the derived bounds of
tests/clip_bounds.py, the whole tower against an fp64 restatement, and the route behind MotionTransformer._clip_features.

Outputs live in the `Guarded` buffers of the attention contract (a NaN pattern, guard rows and guard columns).

Whole-tower gate (the project's precedent): per-sample rel-L2 distance from fp64 <= max(1e-6, 4 x the distance of the fp32
torch-ops forward, run on the CPU, from the same fp64 result).  Measured on the MI355X, worst sample of each case, as
`HIP distance / torch-ops distance`:
    W 128 H 2 L 2 B 3 vocab 1000      7.1e-7 / 6.1e-7 = 1.15
    W 512 H 8 L 2 B 2 vocab 49408     1.22e-6 / 6.2e-7 = 2.03
    W 512 H 8 L 12 B 2                1.34e-6 / 6.3e-7 = 2.14
prec bf16x3 (gate 5e-5): 1.06e-5 at L = 2, 1.16e-5 at L = 12.
"""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_bounds as CB  # noqa: E402
import hig_amd  # noqa: E402
from hig_amd import _lib  # noqa: E402
from hig_amd.models import clip_text as CT  # noqa: E402
from hig_amd.models import stub_clip  # noqa: E402
from oracle import fill  # noqa: E402
from test_gpu_attn_contract import Guarded, P  # noqa: E402

DEV = "cuda"
N = 77


def lib():
    return _lib.lib()


def stream():
    return _lib.stream_ptr()


# ---- embed -------------------------------------------------------------------------------------------------------------------
def test_embed_is_bit_equal_and_an_id_out_of_range_reads_no_row():
    B, W, vocab = 3, 512, 1000
    g = torch.Generator().manual_seed(5)
    emb, pos = torch.randn(vocab, W, generator=g).to(DEV), torch.randn(N, W, generator=g).to(DEV)
    tok = torch.randint(0, vocab, (B, N), generator=g)
    tok[0, 0], tok[1, 5], tok[2, N - 1], tok[2, 3] = 0, vocab - 1, -1, vocab
    tok[1, 9], tok[1, 10] = 2 ** 40, -2 ** 40
    out = Guarded(B * N, W)
    _lib.check(lib().hig_clip_embed(P(emb), P(pos), P(tok.to(DEV)), B, N, W, vocab, out.ptr(), out.ld, stream()))
    torch.cuda.synchronize()
    got = out.verify("hig_clip_embed").view(B, N, W)
    live = (tok >= 0) & (tok < vocab)
    want = torch.where(live[..., None].to(DEV), emb[tok.clamp(0, vocab - 1).to(DEV)] + pos[None], pos[None].expand(B, N, W))
    assert torch.equal(got, want)
    assert (~live).sum() == 4 and torch.equal(got[2, N - 1], pos[N - 1]) and torch.equal(got[2, 3], pos[3])


# ---- QuickGELU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 1027, 65541])
def test_quick_gelu_within_its_derived_bound(n):
    z = CB.quick_gelu_grid(n, seed=n)
    ref, bound = CB.quick_gelu_ref(z), CB.quick_gelu_bound(z)
    for off in (0, 1):                                     # 16-byte aligned (float4 body + tail) and not (element by element)
        buf = Guarded(1, n + off, pad=8 + (-(n + off)) % 4)    # rows of whole float4: buf.out starts 16-byte aligned
        assert buf.out.data_ptr() % 16 == 0
        buf.out[0, off:] = z.to(DEV)
        if off:
            buf.out[0, 0] = 1.0
        _lib.check(lib().hig_quick_gelu(buf.ptr(off), n, stream()))
        torch.cuda.synchronize()
        got = buf.verify("hig_quick_gelu")[0]
        assert off == 0 or got[0].item() == 1.0
        ratio = ((got[off:].double().cpu() - ref).abs() / bound).max().item()
        print("hig_quick_gelu n=%d offset %d: worst |err| / bound = %.3f" % (n, off, ratio))
        assert ratio <= 1.0


# ---- causal attention --------------------------------------------------------------------------------------------------------
def run_causal(qkv, B, H, Nk, finite=True):
    """The tower's call: Q, K, V are the three column blocks of one (B N, 3 W) buffer.  finite=False: the inputs hold NaN on
    purpose, so only the guard bands are checked."""
    W = H * CB.HD
    y = Guarded(B * Nk, W)
    _lib.check(lib().hig_causal_attn_fwd(P(qkv), 3 * W, P(qkv, W), P(qkv, 2 * W), 3 * W, B, Nk, H, y.ptr(), y.ld, stream()))
    torch.cuda.synchronize()
    if finite:
        y.verify("hig_causal_attn_fwd")
    else:
        band = torch.ones(y.rows + 2, y.ld, dtype=torch.bool, device=DEV)
        band[1:y.rows + 1, :y.cols] = False
        assert (y.buf.view(y.rows + 2, y.ld)[band] == y.pat).all(), "a store landed in the guard band"
    return y.out.reshape(B, Nk, H, CB.HD).clone()


CAUSAL = [(1, 1, 1), (2, 2, 33), (3, 2, 64), (2, 1, 65), (1, 8, 77), (1, 1, 128)]


@pytest.mark.parametrize("B, H, Nk", CAUSAL)
def test_causal_attention_within_its_bound_and_blind_to_later_keys(B, H, Nk):
    qkv = CB.causal_inputs(B, H, Nk, seed=B * 1000 + Nk)
    q, k, v = CB.split_qkv(qkv, B, Nk, H)
    r = CB.causal_reference(q, k, v)
    assert r["spread"] <= 80
    dev = qkv.to(DEV)
    got = run_causal(dev, B, H, Nk)
    ratio = ((got.double().cpu() - r["y"]).abs() / CB.causal_bound(r)).max().item()
    print("hig_causal_attn_fwd B %d H %d N %d: logit spread %.1f, worst |err| / bound = %.4f" % (B, H, Nk, r["spread"], ratio))
    assert ratio <= 1.0
    assert torch.equal(got[:, 0].cpu(), v[:, 0])                                  # one live key: weight 1, bit for bit
    W = H * CB.HD
    for n0 in sorted({n for n in (0, 31, 32, Nk - 2) if 0 <= n < Nk - 1}):        # keys m > n0 are skipped, not masked
        bad = dev.clone().view(B, Nk, 3 * W)
        bad[:, n0 + 1:, W:] = float("nan")
        again = run_causal(bad.view(B * Nk, 3 * W), B, H, Nk, finite=False)
        assert torch.equal(again[:, :n0 + 1], got[:, :n0 + 1]), n0
        assert torch.isnan(again[:, n0 + 1:]).all()


def test_causal_attention_with_unaligned_operands_is_bit_equal():
    """Operands that are not 16-byte aligned are staged element by element instead of by float4: same arithmetic, same bits."""
    B, H, Nk = 2, 2, 77
    W = H * CB.HD
    qkv = CB.causal_inputs(B, H, Nk, seed=4).to(DEV)
    want = run_causal(qkv, B, H, Nk)
    shifted = torch.empty(B * Nk * 3 * W + 1, device=DEV)
    shifted[1:] = qkv.flatten()
    moved = shifted[1:].view(B * Nk, 3 * W)
    assert moved.data_ptr() % 16 == 4
    assert torch.equal(run_causal(moved, B, H, Nk), want)


def test_causal_attention_subtracts_the_row_maximum():
    B, H, Nk = 2, 2, 77
    qkv = CB.causal_inputs(B, H, Nk, seed=9, spread=40.0)
    q, k, v = CB.split_qkv(qkv, B, Nk, H)
    r = CB.causal_reference(q, k, v)
    assert 39.9 < r["spread"] < 40.1 and r["S"].abs().max() > 20
    got = run_causal(qkv.to(DEV), B, H, Nk)
    ratio = ((got.double().cpu() - r["y"]).abs() / CB.causal_bound(r)).max().item()
    print("hig_causal_attn_fwd at logit spread %.1f: worst |err| / bound = %.4f" % (r["spread"], ratio))
    assert ratio <= 1.0


# ---- the whole tower ---------------------------------------------------------------------------------------------------------
TOWERS = {"w128": dict(W=128, H=2, L=2, B=3, vocab=1000), "w512": dict(W=512, H=8, L=2, B=2, vocab=49408),
          "w512_l12": dict(W=512, H=8, L=12, B=2, vocab=1000)}


@functools.lru_cache(maxsize=None)
def tower_case(name):
    """(state dict, frozen module on the device, tokens, fp64 result, per-sample distance of the fp32 torch-ops forward on
    the CPU from it): computed once per case and shared."""
    c = TOWERS[name]
    sd = CB.tower_weights(c["W"], c["H"], c["L"], N, c["vocab"], seed=len(name))
    tokens = CB.tower_tokens(c["B"], N, c["vocab"], seed=len(name))
    ref = CB.tower_fp64(sd, tokens, c["H"])
    m = CT.load_text_tower(sd)
    for p in m.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        torch_dist = CB.rel_per_sample(m.features(tokens).permute(1, 0, 2), ref)
    return sd, m.to(DEV), tokens, ref, torch_dist


def run_tower(table, tokens, precision="f32"):
    out = CT.tower_forward(table, tokens.to(DEV), None, precision)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(TOWERS))
def test_whole_tower_against_fp64(name):
    sd, m, tokens, ref, torch_dist = tower_case(name)
    table = CT.TowerTable(m, torch.device(DEV, 0))
    dist = CB.rel_per_sample(run_tower(table, tokens), ref)
    print("tower %s: HIP %s, torch-ops fp32 %s, ratio %s" % (name, dist.tolist(), torch_dist.tolist(), (dist / torch_dist).tolist()))
    assert torch.isfinite(dist).all()
    assert (dist <= torch.clamp(4 * torch_dist, min=1e-6)).all()
    # the torch-ops forward of the same module ON THE DEVICE is the route the flag "torch" keeps: the two agree as closely
    with torch.no_grad():
        dev = CB.rel_per_sample(m.features(tokens.to(DEV)).permute(1, 0, 2), ref)
    print("tower %s: torch-ops on the device %s" % (name, dev.tolist()))


@pytest.mark.parametrize("name", ["w512", "w512_l12"])
def test_whole_tower_split_bf16_products(name):
    """prec bf16x3 through the tower's GEMMs, at the 5e-5 test_gpu_text_head.py holds that mode to at L = 2.
    Measured on the MI355X: 1.06e-5 at L = 2, 1.16e-5 at L = 12."""
    sd, m, tokens, ref, torch_dist = tower_case(name)
    table = CT.TowerTable(m, torch.device(DEV, 0))
    dist = CB.rel_per_sample(run_tower(table, tokens, "bf16x3"), ref)
    print("tower %s bf16x3: %s (exact fp32 on torch ops: %s)" % (name, dist.tolist(), torch_dist.tolist()))
    assert (dist <= 5e-5).all()


def test_samples_are_independent():
    sd, m, tokens, ref, _ = tower_case("w128")
    table = CT.TowerTable(m, torch.device(DEV, 0))
    a = run_tower(table, tokens)
    other = tokens.clone()
    other[1] = CB.tower_tokens(3, N, TOWERS["w128"]["vocab"], seed=77)[2]
    assert not torch.equal(other[1], tokens[1])
    b = run_tower(table, other)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1])


def test_captured_equals_eager():
    sd, m, tokens, ref, _ = tower_case("w128")
    c = TOWERS["w128"]
    table = CT.TowerTable(m, torch.device(DEV, 0))
    second = CB.tower_tokens(c["B"], N, c["vocab"], seed=31)
    eager = [run_tower(table, t).clone() for t in (tokens, second)]
    dims = CT.clip_dims(c["B"], N, c["W"], c["H"], c["L"], c["vocab"])
    ws = torch.empty(lib().hig_clip_text_workspace_bytes(dims), dtype=torch.uint8, device=DEV)
    static_tok, out = tokens.to(DEV).clone(), torch.empty(c["B"], N, c["W"], device=DEV)
    call = lambda: _lib.check(lib().hig_clip_text_fwd(dims, table.table, P(static_tok), P(out), P(ws), stream()))   # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for t, want in ((second, eager[1]), (tokens, eager[0])):
        static_tok.copy_(t.to(DEV))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


# ---- behind MotionTransformer --------------------------------------------------------------------------------------------------
CAPTIONS = ["a person waves the right hand", "two people shake hands and then one of them walks slowly away to the left", "jump"]


def own_tower(L=2):
    m = CT.load_text_tower(CB.tower_weights(512, 8, L, N, stub_clip.VOCAB, seed=11))
    return m


def build(flag, cls=None, **kw):
    c = fill.CASES["config1"]
    cls = cls or hig_amd.MotionTransformer
    m = cls(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"], num_layers=c["L"], num_heads=c["H"],
            text_latent_dim=c["Lt"], clip_tower=flag, **kw)
    m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    return m.to(DEV)


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_encode_text_and_a_fused_step_under_both_flags():
    c = fill.CASES["config1"]
    res = {}
    for flag in ("hip", "torch"):
        m = build(flag, clip_model=own_tower(), clip_tokenize=stub_clip.tokenize).train()
        tokens = stub_clip.tokenize(CAPTIONS, truncate=True).to(DEV)
        assert (m._clip_native_table(tokens) is not None) == (flag == "hip")
        with torch.no_grad():
            xf_proj, xf_out = m.encode_text(CAPTIONS, DEV)
        text, feat = m._clip_features(CAPTIONS, DEV)
        assert torch.equal(text, tokens) and feat.shape == (N, 3, 512) and not feat.requires_grad
        assert feat.permute(1, 0, 2).is_contiguous() == (flag == "hip")           # the head's .contiguous() is free
        args = types.SimpleNamespace(device=torch.device(DEV), diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=c["B"],
                                     num_epochs=1, log_every=50, save_latest=500, save_every_e=5, is_continue=False, model_dir="/tmp")
        tr = hig_amd.DDPMTrainer(args, m)
        clip_out, eot = tr.clip_inputs(CAPTIONS[:c["B"]])
        assert clip_out.shape == (c["B"], N, 512) and clip_out.is_contiguous()
        motions = (fill.tensor_for("ct.motions", (c["B"], c["T"], c["F"])) * 10).to(DEV)
        noise = fill.tensor_for("ct.noise", motions.shape).to(DEV)
        loss = tr.train_step_fused(motions, torch.tensor(c["t"]).to(DEV), torch.tensor(c["lengths"]).to(DEV), noise=noise,
                                   clip_out=clip_out, eot=eot)
        res[flag] = (xf_proj, xf_out, loss.item(), feat)
        assert all(p.grad is None and not p.requires_grad for p in m.clip.parameters())
    print("encode_text hip vs torch: clip features %.2e xf_proj %.2e xf_out %.2e; fused loss %.8f vs %.8f" % (
        rel(res["hip"][3], res["torch"][3]), rel(res["hip"][0], res["torch"][0]), rel(res["hip"][1], res["torch"][1]),
        res["hip"][2], res["torch"][2]))
    assert rel(res["hip"][0], res["torch"][0]) < 2e-5 and rel(res["hip"][1], res["torch"][1]) < 2e-5
    assert abs(res["hip"][2] - res["torch"][2]) < 1e-5 * abs(res["torch"][2])


def test_the_table_is_dropped_when_parameters_move_and_the_rule_is_asked_again():
    m = build("hip", clip_model=own_tower(), clip_tokenize=stub_clip.tokenize)
    tokens = stub_clip.tokenize(CAPTIONS, truncate=True).to(DEV)
    t1 = m._clip_native_table(tokens)
    assert t1 is not None and m._clip_native_table(tokens) is t1                  # built once
    a = m._clip_features(CAPTIONS, DEV)[1]
    m.load_state_dict(m.state_dict())
    assert m._clip_table is None
    m.to(DEV)
    t2 = m._clip_native_table(tokens)
    assert t2 is not None and t2 is not t1 and torch.equal(m._clip_features(CAPTIONS, DEV)[1], a)
    m.clip.ln_final.weight.requires_grad_(True)                                   # un-frozen behind the table's back
    assert m._clip_native_table(tokens) is None
    m.clip.ln_final.weight.requires_grad_(False)
    m.half()
    assert m._clip_native_table(tokens) is None                                   # fp16 weights stay on torch ops


def test_the_stub_and_a_trainable_tower_stay_on_torch_ops():
    feats = {}
    for flag in ("hip", "torch"):
        m = build(flag, clip_model=stub_clip.StubCLIP(), clip_tokenize=stub_clip.tokenize)   # what clip.load gives without the package
        tokens, x = m._clip_features(CAPTIONS, DEV)
        feats[flag] = x
        assert m._clip_native_table(tokens) is None
    assert torch.equal(feats["hip"], feats["torch"])
    c = fill.CASES["config1"]
    two = hig_amd.MotionInteractionTransformer(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                               num_layers=1, num_heads=c["H"], text_latent_dim=c["Lt"], no_clip=True,
                                               clip_model=own_tower(), clip_tokenize=stub_clip.tokenize).to(DEV)
    tokens = stub_clip.tokenize(CAPTIONS, truncate=True).to(DEV)
    assert two.clip_tower == "hip" and two._clip_native_table(tokens) is None
    assert all(p.requires_grad for p in two.clip.transformer.parameters())
    xf_proj, xf_out = two.encode_text(CAPTIONS, DEV)
    assert xf_out.shape == (3, N, c["Lt"]) and xf_proj.requires_grad               # the trainable tower is part of the graph
    xf_proj.sum().backward()
    assert two.clip.transformer.resblocks[0].mlp.c_fc.weight.grad is not None
