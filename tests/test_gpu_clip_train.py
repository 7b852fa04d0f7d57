"""Training the CLIP text tower on the MI355X (csrc/cliptext_bwd.hip, the training entries of csrc/cliptext.hip): the kernels
against fp64 under the derived bounds of tests/clip_train_bounds.py, the embedding gradient bit for bit against its numpy
restatement, the whole tower's gradients against fp64 torch.autograd, and the route behind
MotionInteractionTransformer(no_clip=True, clip_tower_train="hip").

Every output lives in a `Guarded` buffer of the attention contract (a NaN pattern, guard rows and guard columns).

Whole-tower gate (the project's standing one for the tower and the dedup head): per parameter, rel-L2 distance from the fp64
torch.autograd gradient <= max(1e-6, 4 x the distance of the fp32 torch-ops gradient, computed on the CPU, from the same fp64
one).  One class of entries is left out and no other: the key third [W:2W] of every attn.in_proj_bias.  Its true gradient is
exactly zero (a bias on the keys shifts every logit of a row by the same amount, and softmax is shift-invariant), so both fp32
routes hold only rounding noise there and a relative distance means nothing; the HIP values there are held to the noise level
instead: their norm relative to the bias's other two thirds is at most 10 x (tests/test_gpu_eval_train.py's factor for the same
entries) what the CPU fp32 route shows.

Measured on the MI355X (largest |err| / bound, or HIP distance / torch distance):
    lse 0.039;  dQ 0.0033, dK 0.0059, dV 0.022 (spread 40: 0.0033 / 0.0034 / 0.016);  QuickGELU derivative 0.61
    tower W 128 L 2 B 3: 1.44;  W 512 H 8 L 2 vocab 49408: 3.07 (ln_final.bias, 5.7e-7 against 1.9e-7);  W 128 L 1 B 27: 1.63
    key thirds: HIP 1.3e-7 .. 6.8e-7 of the other two thirds, the CPU fp32 route 1.4e-7 .. 5.4e-7
    route: worst 3.46 (a text-head bias);  three trainer steps: total update 0.81 .. 1.45 of the torch route's distance from fp64,
    losses 14.857300 / 10.429654 / 8.045968 against the torch route's 14.857301 / 10.429654 / 8.045966
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_bounds as CB  # noqa: E402
import clip_train_bounds as TB  # noqa: E402
import hig_amd  # noqa: E402
from hig_amd import _lib  # noqa: E402
from hig_amd.models import clip_text as CT  # noqa: E402
from hig_amd.models import stub_clip  # noqa: E402
from oracle import fill  # noqa: E402
from test_gpu_attn_contract import Guarded, P  # noqa: E402

DEV = "cuda"
N = 77
HD = CB.HD


def lib():
    return _lib.lib()


def stream():
    return _lib.stream_ptr()


def bands_kept(g, what):
    """The guard bands of a buffer whose payload may hold NaN on purpose."""
    band = torch.ones(g.rows + 2, g.ld, dtype=torch.bool, device=DEV)
    band[1:g.rows + 1, :g.cols] = False
    assert (g.buf.view(g.rows + 2, g.ld)[band] == g.pat).all(), "%s: a store landed in the guard band" % what


# ---- hig_causal_attn_fwd_train ---------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (2, 2, 33), (1, 1, 64), (1, 1, 65), (3, 2, 77), (1, 1, 128)]


@pytest.mark.parametrize("B, H, Nk", SHAPES)
def test_training_forward_of_the_attention_same_y_and_lse_within_its_bound(B, H, Nk):
    W = H * HD
    qkv = CB.causal_inputs(B, H, Nk, seed=B * 1000 + Nk)
    r = CB.causal_reference(*CB.split_qkv(qkv, B, Nk, H))
    dev = qkv.to(DEV)
    y0, y1, lse = Guarded(B * Nk, W), Guarded(B * Nk, W), Guarded(B * H, Nk, pad=0)
    _lib.check(lib().hig_causal_attn_fwd(P(dev), 3 * W, P(dev, W), P(dev, 2 * W), 3 * W, B, Nk, H, y0.ptr(), y0.ld, stream()))
    _lib.check(lib().hig_causal_attn_fwd_train(P(dev), 3 * W, P(dev, W), P(dev, 2 * W), 3 * W, B, Nk, H, y1.ptr(), y1.ld, lse.ptr(), stream()))
    torch.cuda.synchronize()
    assert torch.equal(y0.verify("hig_causal_attn_fwd"), y1.verify("hig_causal_attn_fwd_train"))
    got = lse.verify("lse").reshape(B, H, Nk).double().cpu()
    ratio = ((got - r["lse"]).abs() / TB.lse_bound(r)).max().item()
    print("hig_causal_attn_fwd_train B %d H %d N %d: lse worst |err| / bound = %.4f" % (B, H, Nk, ratio))
    assert ratio <= 1.0


# ---- hig_causal_attn_bwd ---------------------------------------------------------------------------------------------------------------
class BwdRun:
    """One call of hig_causal_attn_bwd the way the tower makes it: Q, K, V column blocks of one (B N, 3 W) buffer, dQ, dK, dV
    column blocks of one guarded (B N, 3 W) buffer."""

    def __init__(self, qkv, dy, lse, y, B, H, Nk, finite=True, hd=HD, n_arg=None):
        W = H * HD
        ld = lambda t: t.stride(0)   # noqa: E731
        self.out, self.delta = Guarded(B * Nk, 3 * W), Guarded(B * H, Nk, pad=0)
        o = self.out
        self.rc = lib().hig_causal_attn_bwd(P(dy), ld(dy), P(y), ld(y), P(qkv), ld(qkv), P(qkv, W), P(qkv, 2 * W), ld(qkv), B,
                                            Nk if n_arg is None else n_arg, H, hd, P(lse), self.delta.ptr(), o.ptr(), o.ld, o.ptr(W), o.ptr(2 * W),
                                            o.ld, stream())
        torch.cuda.synchronize()
        if self.rc != 0:
            return
        if finite:
            o.verify("hig_causal_attn_bwd")
            self.delta.verify("delta")
        else:
            bands_kept(o, "hig_causal_attn_bwd"), bands_kept(self.delta, "delta")
        self.dQ, self.dK, self.dV = (o.out[:, i * W:(i + 1) * W].reshape(B, Nk, H, HD).clone() for i in range(3))


def bwd_case(B, H, Nk, seed, spread=None):
    qkv, dy, lse, y, fwd = TB.causal_bwd_inputs(B, H, Nk, seed, spread)
    q, k, v = CB.split_qkv(qkv, B, Nk, H)
    r = TB.causal_bwd_reference(q, k, v, dy.reshape(B, Nk, H, HD), lse, y.reshape(B, Nk, H, HD))
    return tuple(t.to(DEV) for t in (qkv, dy, lse, y)), r, fwd


def held(run, r, what):
    b = TB.causal_bwd_bounds(r)
    ratios = {n: ((getattr(run, n).double().cpu() - r[n]).abs() / b[n]).max().item() for n in ("dQ", "dK", "dV")}
    dl = ((run.delta.out.reshape(r["delta"].shape).double().cpu() - r["delta"]).abs().max() / r["delta"].abs().max()).item()
    print("hig_causal_attn_bwd %s: worst |err| / bound %s (delta rel %.1e)" % (what, {n: round(x, 4) for n, x in ratios.items()}, dl))
    assert max(ratios.values()) <= 1.0, ratios
    return ratios


@pytest.mark.parametrize("B, H, Nk", SHAPES + [(1, 2, 2)])
def test_causal_backward_within_its_bounds_twice_the_same_bits_and_blind_to_what_it_must_not_see(B, H, Nk):
    (qkv, dy, lse, y), r, _ = bwd_case(B, H, Nk, seed=B * 1000 + Nk)
    W = H * HD
    a = BwdRun(qkv, dy, lse, y, B, H, Nk)
    _lib.check(a.rc)
    held(a, r, "B %d H %d N %d" % (B, H, Nk))
    b = BwdRun(qkv, dy, lse, y, B, H, Nk)
    assert torch.equal(a.out.out, b.out.out) and torch.equal(a.delta.out, b.delta.out)
    nan = float("nan")
    for n0 in sorted({n for n in (0, 31, 32, 63, 64, Nk - 2) if 0 <= n < Nk - 1}):
        # no K or V row beyond n0 enters a query row <= n0
        bad = qkv.clone().view(B, Nk, 3 * W)
        bad[:, n0 + 1:, W:] = nan
        c = BwdRun(bad.view(B * Nk, 3 * W), dy, lse, y, B, H, Nk, finite=False)
        assert torch.equal(c.dQ[:, :n0 + 1], a.dQ[:, :n0 + 1]), n0
        # no Q, dY, Y, lse row below n0 enters a key row >= n0
        n1 = n0 + 1
        bq, bdy, by, bl = qkv.clone().view(B, Nk, 3 * W), dy.clone().view(B, Nk, W), y.clone().view(B, Nk, W), lse.clone()
        bq[:, :n1, :W], bdy[:, :n1], by[:, :n1], bl[:, :, :n1] = nan, nan, nan, nan
        d = BwdRun(bq.view(B * Nk, 3 * W), bdy.view(B * Nk, W), bl, by.view(B * Nk, W), B, H, Nk, finite=False)
        assert torch.equal(d.dK[:, n1:], a.dK[:, n1:]) and torch.equal(d.dV[:, n1:], a.dV[:, n1:]), n1


def test_causal_backward_at_logit_spread_40():
    B, H, Nk = 2, 2, 77
    (qkv, dy, lse, y), r, fwd = bwd_case(B, H, Nk, seed=9, spread=40.0)
    assert 39.9 < fwd["spread"] < 40.1
    a = BwdRun(qkv, dy, lse, y, B, H, Nk)
    _lib.check(a.rc)
    held(a, r, "at logit spread %.1f" % fwd["spread"])


def test_causal_backward_with_unaligned_operands_is_bit_equal():
    """Base + 4 bytes and an odd leading dimension: staged element by element instead of by float4, the same arithmetic."""
    B, H, Nk = 2, 2, 77
    W = H * HD
    (qkv, dy, lse, y), r, _ = bwd_case(B, H, Nk, seed=4)
    want = BwdRun(qkv, dy, lse, y, B, H, Nk)

    def moved(t):
        rows, cols = t.shape
        buf = torch.zeros(rows * (cols + 1) + 1, device=DEV)
        view = buf[1:].view(rows, cols + 1)[:, :cols]
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.stride(0) % 2 == 1
        return view

    got = BwdRun(moved(qkv), moved(dy), lse, moved(y), B, H, Nk)
    _lib.check(got.rc)
    assert torch.equal(got.out.out, want.out.out) and torch.equal(got.delta.out, want.delta.out)


def test_causal_backward_refuses_129_tokens_and_head_dim_32_and_launches_nothing():
    B, H, Nk = 1, 1, 128
    (qkv, dy, lse, y), r, _ = bwd_case(B, H, Nk, seed=1)
    for kw, word in ((dict(n_arg=129), "N=129"), (dict(hd=32), "head dim 32")):
        run = BwdRun(qkv, dy, lse, y, B, H, Nk, **kw)
        assert run.rc == _lib.EUNSUPPORTED and word in _lib.last_error()
        assert (run.out.buf == run.out.pat).all() and (run.delta.buf == run.delta.pat).all()


# ---- hig_quick_gelu_bwd ----------------------------------------------------------------------------------------------------------------
def gelu_inputs(n):
    z = CB.quick_gelu_grid(n, seed=n)
    g = torch.Generator().manual_seed(n)
    dy = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 4 - 2)
    return z, dy


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 200001])
def test_quick_gelu_backward_within_its_bound_in_place_and_unaligned(n):
    z, dy = gelu_inputs(n)
    assert (dy > 0).any() or n < 3
    ref, bound = TB.quick_gelu_grad_ref(z, dy), TB.quick_gelu_grad_bound(z, dy)
    results = []
    for off in (0, 1):                                     # 16-byte aligned (float4 body + tail) and not (element by element)
        zz = torch.zeros(n + off + 4, device=DEV)[off:off + n].copy_(z.to(DEV))
        dd = torch.zeros(n + off + 4, device=DEV)[off:off + n].copy_(dy.to(DEV))
        buf = Guarded(1, n + off, pad=8 + (-(n + off)) % 4)
        assert buf.out.data_ptr() % 16 == 0 and zz.data_ptr() % 16 == 4 * off
        if off:
            buf.out[0, 0] = 1.0
        _lib.check(lib().hig_quick_gelu_bwd(P(zz), P(dd), buf.ptr(off), n, stream()))
        torch.cuda.synchronize()
        got = buf.verify("hig_quick_gelu_bwd")[0]
        assert off == 0 or got[0].item() == 1.0
        ratio = ((got[off:].double().cpu() - ref).abs() / bound).max().item()
        print("hig_quick_gelu_bwd n=%d offset %d: worst |err| / bound = %.3f" % (n, off, ratio))
        assert ratio <= 1.0
        results.append(got[off:].clone())
        buf.out[0, off:] = dy.to(DEV)                      # in place: dz = dy
        _lib.check(lib().hig_quick_gelu_bwd(P(zz), buf.ptr(off), buf.ptr(off), n, stream()))
        torch.cuda.synchronize()
        assert torch.equal(buf.verify("hig_quick_gelu_bwd in place")[0][off:], results[-1])
    assert torch.equal(results[0], results[1])
    # the out-of-place forward the training route keeps z with: hig_quick_gelu's bits
    zz = z.to(DEV)
    out = Guarded(1, n, pad=8 + (-n) % 4)
    _lib.check(lib().hig_quick_gelu_to(P(zz), out.ptr(), n, stream()))
    inplace = zz.clone()
    _lib.check(lib().hig_quick_gelu(P(inplace), n, stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.verify("hig_quick_gelu_to")[0], inplace) and torch.equal(zz.cpu(), z)


# ---- hig_clip_embed_bwd ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 6])
def test_embedding_gradient_is_the_chunked_sum_bit_for_bit(W):
    from test_cpu_clip_train import embed_case
    tokens, vocab, reps = embed_case(W, seed=W)
    B, Nn = tokens.shape
    g = torch.Generator().manual_seed(W)
    dx0 = torch.randn(B * Nn, W, generator=g) * 10.0 ** (torch.rand(B * Nn, 1, generator=g) * 8 - 4)
    assert dx0.abs().max() > 1e3 and dx0.abs().min() < 1e-3
    ix = CT.EmbedIndex(tokens, vocab).to(DEV)
    want_tok, want_pos = CT.embed_grad_restated(dx0.numpy(), ix, W)
    dtok, dpos = Guarded(vocab, W, pad=0), Guarded(Nn, W, pad=0)
    scratch = Guarded(ix.n_chunks + ix.n_ids, W, pad=0)
    src = dx0.to(DEV)
    for _ in range(2):
        _lib.check(lib().hig_clip_embed_bwd(P(src), B, Nn, W, vocab, P(ix.dev), ix.n_live, ix.n_chunks, ix.n_ids, scratch.ptr(), dtok.ptr(),
                                            dpos.ptr(), stream()))
        torch.cuda.synchronize()
        scratch.verify("scratch")
        got_tok, got_pos = dtok.verify("dtok").cpu().numpy(), dpos.verify("dpos").cpu().numpy()
        assert np.array_equal(got_tok.view(np.int32), want_tok.view(np.int32))       # bit for bit, the sign of zero included
        assert np.array_equal(got_pos.view(np.int32), want_pos.view(np.int32))
    unused = sorted(set(range(vocab)) - set(int(t) for t in ix.ids))
    assert len(unused) > 50 and not got_tok[unused].view(np.int32).any()             # exactly +0.0
    assert np.array_equal(want_pos, np.stack([dx0.numpy().reshape(B, Nn, W)[:, n].cumsum(0, dtype=np.float32)[-1] for n in range(Nn)]))


# ---- the whole tower --------------------------------------------------------------------------------------------------------------------
TOWERS = {"w128": dict(W=128, H=2, L=2, B=3, vocab=64), "w512": dict(W=512, H=8, L=2, B=2, vocab=49408),
          "w128_rows2079": dict(W=128, H=2, L=1, B=27, vocab=64)}    # 27 x 77 = 2 079 rows: past the 2 048 where wgrad_wsp32 takes over


@functools.lru_cache(maxsize=None)
def tower_case(name):
    """(trainable module on the device, tokens, upstream, fp64 autograd gradients, fp32 torch-ops gradients on the CPU): once."""
    c = TOWERS[name]
    sd = CB.tower_weights(c["W"], c["H"], c["L"], N, c["vocab"], seed=len(name))
    tokens = CB.tower_tokens(c["B"], N, c["vocab"], seed=len(name))
    dout = TB.upstream(c["B"], N, c["W"])
    grads = {}
    for dtype in (torch.float64, torch.float32):
        m = CT.load_text_tower(sd).to(dtype)
        (m.features(tokens).permute(1, 0, 2) * dout.to(dtype)).sum().backward()
        grads[dtype] = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert c["B"] * N > 2048 or name != "w128_rows2079"
    return CT.load_text_tower(sd).to(DEV), tokens, dout, grads[torch.float64], grads[torch.float32]


def names_in_table_order(m):
    by_ptr = {p.data_ptr(): k for k, p in m.named_parameters()}
    return [by_ptr[t.data_ptr()] for t in CT._tower_tensors(m)]


def gate_gradients(what, got, ref64, ref32, W):
    """The 4x gate per parameter (module docstring); got / ref64 / ref32: {name: tensor}.  Returns the worst HIP / torch ratio."""
    worst = (0.0, None)
    for name, r in ref64.items():
        a, t = got[name].double().cpu(), ref32[name].double()
        third = TB.key_third(name, W)
        if third is not None:
            keep = torch.ones(r.numel(), dtype=torch.bool)
            keep[third] = False
            noise, noise32 = (a[third].norm() / a[keep].norm()).item(), (t[third].norm() / t[keep].norm()).item()
            print("%s %s key third (true gradient 0): HIP %.2e, torch fp32 %.2e of the other two thirds" % (what, name, noise, noise32))
            assert noise <= 10 * noise32, name
            a, t, r = a[keep], t[keep], r[keep]
        dist, floor = TB.rel(a, r), TB.rel(t, r)
        ratio = dist / floor if floor > 0 else (0.0 if dist == 0 else float("inf"))    # (a gradient both routes get exactly: 0 / 0)
        print("%s %-50s HIP %.2e / torch fp32 %.2e = %.2f" % (what, name, dist, floor, ratio))
        assert np.isfinite(dist) and dist <= max(1e-6, 4 * floor), name
        worst = max(worst, (ratio, name))
    print("%s: worst HIP distance / torch distance %.2f (%s)" % (what, *worst))
    return worst


def guarded_tower_call(table, tokens, dout, c):
    """hig_clip_text_fwd_train + hig_clip_text_bwd with the output and every gradient in a guarded buffer (no leading dimension
    goes through the table: guard rows only) and guard rows around the two workspaces -> (out, [gradients in table order])."""
    dims = CT.clip_dims(c["B"], N, c["W"], c["H"], c["L"], c["vocab"])
    out = Guarded(c["B"] * N, c["W"], pad=0)
    grads = [Guarded(p.shape[0] if p.dim() == 2 else 1, p.shape[-1], pad=0) for p in table.tensors]
    saved = Guarded(1, lib().hig_clip_text_train_bytes(dims) // 4, pad=0)
    bws = Guarded(1, lib().hig_clip_text_bwd_workspace_bytes(dims) // 4, pad=0)
    gtable = (C.c_void_p * len(grads))(*[g.out.data_ptr() for g in grads])
    ix = CT.EmbedIndex(tokens, c["vocab"]).to(DEV)
    tok, d_out = tokens.to(DEV), dout.to(DEV)
    _lib.check(lib().hig_clip_text_fwd_train(dims, table.table, P(tok), out.ptr(), saved.ptr(), stream()))
    _lib.check(lib().hig_clip_text_bwd(dims, table.table, P(ix.dev), ix.n_live, ix.n_chunks, ix.n_ids, P(d_out), saved.ptr(), gtable, bws.ptr(),
                                       stream()))
    torch.cuda.synchronize()
    bands_kept(saved, "saved"), bands_kept(bws, "backward workspace")
    return out.verify("hig_clip_text_fwd_train").view(c["B"], N, c["W"]), [g.verify("gradient %d" % i).view(p.shape)
                                                                           for i, (g, p) in enumerate(zip(grads, table.tensors))]


@pytest.mark.parametrize("name", list(TOWERS))
def test_whole_tower_gradients_against_fp64_autograd(name):
    m, tokens, dout, ref64, ref32 = tower_case(name)
    c = TOWERS[name]
    table = CT.TrainTowerTable(m, torch.device(DEV, 0))
    frozen = copy.deepcopy(m)
    for p in frozen.parameters():
        p.requires_grad_(False)
    want = CT.tower_forward(CT.TowerTable(frozen, torch.device(DEV, 0)), tokens.to(DEV))
    out, grads = guarded_tower_call(table, tokens, dout, c)
    assert torch.equal(out, want)                                                    # the training forward: hig_clip_text_fwd's bits
    got = dict(zip(names_in_table_order(m), grads))
    assert set(got) == set(ref64)
    gate_gradients("tower " + name, got, ref64, ref32, c["W"])
    # the Python wrappers the route goes through: the same bits
    out2, saved = CT.tower_forward_train(table, tokens.to(DEV))
    grads2 = CT.tower_backward(table, CT.EmbedIndex(tokens, c["vocab"]).to(DEV), dout.to(DEV), saved)
    torch.cuda.synchronize()
    assert torch.equal(out2, want) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


def test_captured_training_forward_and_backward_equal_eager():
    m, tokens, dout, _, _ = tower_case("w128")
    c = TOWERS["w128"]
    table = CT.TrainTowerTable(m, torch.device(DEV, 0))
    second = CB.tower_tokens(c["B"], N, c["vocab"], seed=31)
    eager = []
    for t in (tokens, second):
        out, saved = CT.tower_forward_train(table, t.to(DEV))
        grads = CT.tower_backward(table, CT.EmbedIndex(t, c["vocab"]).to(DEV), dout.to(DEV), saved)
        torch.cuda.synchronize()
        eager.append((out.clone(), [g.clone() for g in grads]))
    dims = CT.clip_dims(c["B"], N, c["W"], c["H"], c["L"], c["vocab"])
    saved = torch.empty(lib().hig_clip_text_train_bytes(dims), dtype=torch.uint8, device=DEV)
    bws = torch.empty(lib().hig_clip_text_bwd_workspace_bytes(dims), dtype=torch.uint8, device=DEV)
    static_tok, out, d_out = tokens.to(DEV).clone(), torch.empty(c["B"], N, c["W"], device=DEV), dout.to(DEV)
    # the index's size depends on the tokens: the captured call reads a buffer as long as the longest of the two, and its counts
    # are host arguments -- so one graph per index shape; here both token sets are captured each in its own graph
    for t, (want_out, want_grads) in ((second, eager[1]), (tokens, eager[0])):
        ix = CT.EmbedIndex(t, c["vocab"]).to(DEV)
        grads = [torch.empty_like(p) for p in table.tensors]
        gtable = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])

        def call():
            _lib.check(lib().hig_clip_text_fwd_train(dims, table.table, P(static_tok), P(out), P(saved), stream()))
            _lib.check(lib().hig_clip_text_bwd(dims, table.table, P(ix.dev), ix.n_live, ix.n_chunks, ix.n_ids, P(d_out), P(saved), gtable, P(bws),
                                               stream()))
        static_tok.copy_(t.to(DEV))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()                                                                    # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        for _ in range(2):
            out.fill_(float("nan"))
            for g in grads:
                g.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want_out)
            for g, w, p in zip(grads, want_grads, names_in_table_order(m)):
                assert torch.equal(g, w), p


# ---- the route ----------------------------------------------------------------------------------------------------------------------------
CAPTIONS = ["a person waves the right hand", "two people shake hands and then one of them walks slowly away to the left", "jump"]


def build(**kw):
    c = fill.CASES["config1"]
    tower = CT.load_text_tower(CB.tower_weights(512, 8, 2, N, stub_clip.VOCAB, seed=11))
    m = hig_amd.MotionInteractionTransformer(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                             num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"], no_clip=True,
                                             clip_model=tower, clip_tokenize=stub_clip.tokenize, **kw)
    sd = fill.fill_state_dict(m.state_dict())
    sd.update({"clip." + k: v for k, v in CB.tower_weights(512, 8, 2, N, stub_clip.VOCAB, seed=11).items()})   # (no_clip re-initialises the tower)
    m.load_state_dict(sd, strict=True)
    return m


def text_grads(m, device):
    m.zero_grad(set_to_none=True)
    xf_proj, xf_out = m.encode_text(CAPTIONS, device)
    (xf_proj.sum() + xf_out.square().sum()).backward()
    names = [k for k, _ in m.named_parameters() if k.startswith(("clip.", "text"))]
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if k in names}, (xf_proj.detach(), xf_out.detach())


@functools.lru_cache(maxsize=None)
def route_references():
    """The text side's gradients of the same model on torch ops, on the CPU: in fp64 and in fp32."""
    out = {}
    for dtype in (torch.float64, torch.float32):
        m = build(text_head="torch").to(dtype)
        m.clip.d_type = dtype
        out[dtype] = text_grads(m, "cpu")[0]
    return out[torch.float64], out[torch.float32]


def test_the_route_runs_natively_and_its_gradients_hold_the_gate():
    ref64, ref32 = route_references()
    m = build(clip_tower_train="hip").to(DEV).train()
    assert all(p.requires_grad for p in m.clip.parameters())
    assert m._clip_native_table(stub_clip.tokenize(CAPTIONS, truncate=True).to(DEV)) is None      # the frozen rule still refuses it
    got, (xf_proj, xf_out) = text_grads(m, DEV)
    torch.cuda.synchronize()
    assert m.clip_train_stats == {"native_forwards": 1, "native_backwards": 1, "native_inference": 0}
    assert set(got) == set(ref64) and any(k.startswith("clip.transformer") for k in got) and any(k.startswith("textTransEncoder") for k in got)
    gate_gradients("route", got, ref64, ref32, 512)
    # grad disabled: the inference forward, the same features
    with torch.no_grad():
        p2, o2 = m.encode_text(CAPTIONS, DEV)
    assert m.clip_train_stats == {"native_forwards": 1, "native_backwards": 1, "native_inference": 1}
    assert torch.equal(o2, xf_out) and torch.equal(p2, xf_proj)


def test_the_default_stays_on_the_torch_lines():
    m = build().to(DEV).train()
    assert m.clip_tower_train == "torch"
    got, _ = text_grads(m, DEV)
    assert m.clip_train_stats == {"native_forwards": 0, "native_backwards": 0, "native_inference": 0}
    twin = build().to(DEV).train()
    twin.zero_grad(set_to_none=True)
    text = stub_clip.tokenize(CAPTIONS, truncate=True).to(DEV)                       # the torch lines, spelt out
    x = twin.clip.token_embedding(text).type(twin.clip.d_type) + twin.clip.positional_embedding.type(twin.clip.d_type)
    x = twin.clip.ln_final(twin.clip.transformer(x.permute(1, 0, 2))).type(twin.clip.d_type)
    xf_proj, xf_out = twin._text_head(text, x)
    (xf_proj.sum() + xf_out.square().sum()).backward()
    for k, p in twin.named_parameters():
        if k in got:
            assert torch.equal(p.grad, got[k]), k
    # a tower the rule refuses runs the torch lines too, silently
    half = build(clip_tower_train="hip", text_head="torch").to(DEV).half()
    half.clip.d_type = torch.float16
    assert half._clip_train_native_table(text) is None


# ---- training steps -----------------------------------------------------------------------------------------------------------------------
CAP1 = ["a person shakes hands with another person", "one pushes the other"]
CAP2 = ["a person receives a handshake", "one is pushed by the other"]
STEPS = 3


def step_inputs():
    c = dict(fill.ICASES["config1x2"], L=fill.CASES["config1"]["L"])          # the two-person inputs for the model `build` makes
    B, T, Fd = c["B"], c["T"], c["F"]
    motions = [(fill.tensor_for("clip_train.m%d.%d" % (p, s), (B, T, Fd)) * 10) for s in range(STEPS) for p in (1, 2)]
    noises = [fill.tensor_for("clip_train.noise.%d" % s, (2 * B, T, Fd)) * 10.0 for s in range(STEPS)]
    return c, motions, noises


def tower_params(m):
    return {k: p.detach().double().cpu().clone() for k, p in m.named_parameters() if k.startswith("clip.")}


def run_trainer(option):
    """STEPS DDPMMulTrainer.forward() + update() steps in PIT mode with injected t and noise -> (losses, total update of every
    tower parameter, the stats)."""
    import types
    from test_gpu_denoiser import _patch
    c, motions, noises = step_inputs()
    m = build(**({} if option is None else {"clip_tower_train": option})).to(DEV).train()
    args = types.SimpleNamespace(device=torch.device(DEV), diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=c["B"], num_epochs=1,
                                 log_every=50, save_latest=500, save_every_e=5, is_continue=False, model_dir="/tmp", multi=True,
                                 label_path=None, cap_id=False)
    trainer = hig_amd.DDPMMulTrainer(args, m)
    trainer.opt_encoder = torch.optim.Adam(m.parameters(), lr=2e-4)
    t_fixed = torch.tensor(c["t"])
    trainer.sampler.sample = lambda bs, dev: (t_fixed.to(dev), torch.ones(bs))
    before, losses = tower_params(m), []
    for s in range(STEPS):
        undo = _patch(type("F", (), {"randn": None, "randn_like": staticmethod(lambda x, s=s, **_: noises[s].to(DEV))})())
        try:
            trainer.forward((CAP1, CAP2, motions[2 * s], motions[2 * s + 1], torch.tensor(c["lengths"]), None))
            losses.append(trainer.update()["loss_mot_rec"])
        finally:
            undo()
    torch.cuda.synchronize()
    after = tower_params(m)
    return losses, {k: after[k] - before[k] for k in before}, dict(m.clip_train_stats), trainer.diffusion


def fp64_updates(diffusion):
    """The same steps in fp64 on torch ops, on the CPU: the text side through the model's own modules, the denoiser through the
    oracle's functional forward, then the PIT loss, clip_grad_norm_(0.5) and torch.optim.Adam."""
    from oracle import interaction_ref as IR
    from torch.nn.utils import clip_grad_norm_
    c, motions, noises = step_inputs()
    m = build(text_head="torch").double()
    m.clip.d_type = torch.float64
    opt = torch.optim.Adam(m.parameters(), lr=2e-4)
    named = dict(m.named_parameters())
    core = {k: named[k] for k in fill.interaction_params(c["F"], c["d"], c["ff"], c["L"], c["Lt"], c["num_frames"])}
    B, T = c["B"], c["T"]
    t = torch.tensor(c["t"])
    t2 = torch.cat([t, t])
    sa = torch.from_numpy(diffusion.sqrt_alphas_cumprod)[t2][:, None, None]
    sb = torch.from_numpy(diffusion.sqrt_one_minus_alphas_cumprod)[t2][:, None, None]
    before, losses = tower_params(m), []
    for s in range(STEPS):
        x0, nz = torch.cat([motions[2 * s], motions[2 * s + 1]]).double(), noises[s].double()
        x_t = sa * x0 + sb * nz
        x_t = torch.cat([x_t[:B], x_t[:B], x_t[B:], x_t[B:]])
        target = torch.cat([nz[:B], nz[:B], nz[B:], nz[B:]])
        length = torch.tensor(c["lengths"] * 4)
        xf_proj, xf_out = m.encode_text(CAP1 + CAP2 + CAP2 + CAP1, "cpu")
        pred = IR.interaction_forward(core, x_t, torch.cat([t2, t2]), length, xf_proj, xf_out, c["H"], c["L"])
        mask = (torch.arange(T)[None, :] < length[:, None]).double()
        loss = IR.pit_loss(pred, target, mask)
        opt.zero_grad()
        loss.backward()
        clip_grad_norm_(m.parameters(), 0.5)
        opt.step()
        losses.append(loss.item())
    after = tower_params(m)
    return losses, {k: after[k] - before[k] for k in before}


def test_three_trainer_steps_train_the_tower_natively():
    """Losses: option on against option off within 1e-5 relative (the gate tests/test_gpu_eval_train.py holds its autograd route to).
    The total update p_after - p_before of every tower parameter, against the fp64 torch run: within 4 x what the fp32 torch route
    (option off) is; the key third of every in_proj_bias left out (module docstring), nothing else."""
    loss_on, upd_on, stats, diffusion = run_trainer("hip")
    loss_off, upd_off, stats_off, _ = run_trainer(None)
    assert stats == {"native_forwards": STEPS, "native_backwards": STEPS, "native_inference": 0}
    assert stats_off == {"native_forwards": 0, "native_backwards": 0, "native_inference": 0}
    loss64, upd64 = fp64_updates(diffusion)
    print("losses: hip %s, torch %s, fp64 %s" % (loss_on, loss_off, loss64))
    for a, b, r in zip(loss_on, loss_off, loss64):
        assert abs(a - b) <= 1e-5 * abs(b) and abs(a - r) <= 1e-5 * abs(r)
    worst = (0.0, None)
    for k, r in upd64.items():
        a, t = upd_on[k], upd_off[k]
        third = TB.key_third(k, 512)
        if third is not None:
            keep = torch.ones(r.numel(), dtype=torch.bool)
            keep[third] = False
            a, t, r = a[keep], t[keep], r[keep]
        assert r.norm() > 0, k
        dist, floor = TB.rel(a, r), TB.rel(t, r)
        ratio = dist / floor if floor > 0 else (0.0 if dist == 0 else float("inf"))
        print("update %-50s HIP %.2e / torch fp32 %.2e = %.2f" % (k, dist, floor, ratio))
        worst = max(worst, (ratio, k))
        assert dist <= 4 * floor, k
    print("total update over %d steps: worst HIP distance / torch distance %.2f (%s)" % (STEPS, *worst))
