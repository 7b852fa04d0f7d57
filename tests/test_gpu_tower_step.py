"""The CLIP text tower inside the fused / captured training step, on the MI355X: the embedding index built on the device
(csrc/clipindex.hip) against the host index, exactly; the embedding gradient and the tower's adjoint on that index against the
host-index entries, bit for bit; one captured graph replayed over different token sets; and the step itself
(MotionInteractionTransformer(no_clip=True, clip_tower_train="flat") + `token_batch=`) against forward() + update(), against
fp64, with and without caption dedup, captured against fused, and through save / load.

The gates are stated in tests/tower_step_bounds.py.  Model of the step tests: `config1` two-person with the W 512, H 8, L 2 tower
of tests/test_gpu_clip_train.py, 3 pairs in PIT mode (12 text rows, 4 .. 5 distinct captions, U_pad = 8), three steps.

Left out of the two update gates, and nothing else: the key third of every attn.in_proj_bias (the tower's and the text head's).
Its true gradient is exactly zero -- a bias on the keys shifts every logit of a row by the same amount and softmax is
shift-invariant -- so every fp32 route holds rounding noise there and Adam's division by sqrt(v) turns that noise into full-size
steps of random sign (tests/test_gpu_clip_train.py leaves the same entries out for the same reason).

Measured on the MI355X:
    losses: fused (dedup off) 15.795628 / 9.482726 / 7.622094 == forward() + update() under "hip", bit for bit; the torch route
    15.795628 / 9.482727 / 7.622095, fp64 15.795629 / 9.482724 / 7.622095
    total update against fp64, fused distance / torch route's distance (gate 4): worst 2.57 (clip.token_embedding.weight, 5.96e-5
    against 2.32e-5), then 1.96 (textTransEncoder.layers.2.norm1.bias), 1.80 (out.weight); the tower's matrices 0.99 .. 1.00
    dedup on against off: losses equal; worst distance / gate 0.393 (textTransEncoder.layers.1.self_attn.in_proj_bias)
"""
import atexit
import copy
import ctypes as C
import functools
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hig_amd  # noqa: E402
import tower_step_bounds as SB  # noqa: E402
import tower_step_worker as W  # noqa: E402
from hig_amd import _lib  # noqa: E402
from hig_amd.models import clip_text as CT  # noqa: E402
from hig_amd.models import stub_clip  # noqa: E402
from test_gpu_attn_contract import Guarded, P  # noqa: E402

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
N = 77
GUARD, PAT = 64, 0x5A5A5A5A
CHUNK = _lib.CLIP_EMBED_CHUNK


def lib():
    return _lib.lib()


def stream():
    return _lib.stream_ptr()


def bits(t):
    return t.contiguous().view(torch.int32)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    return port


_WORKER = None
if torch.cuda.device_count() >= 1:      # (counting devices does not initialise the GPU)
    _out = tempfile.mkdtemp(prefix="hig_towerstep_")
    _log = open(os.path.join(_out, "rank0.log"), "wb")
    _WORKER = (_out, subprocess.Popen([sys.executable, os.path.join(HERE, "tower_step_worker.py"), _free_port(), _out],
                                      env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), stdout=_log, stderr=subprocess.STDOUT))
    atexit.register(lambda: _WORKER[1].poll() is None and _WORKER[1].kill())


class IBand:
    """n int32 behind and in front of GUARD guard ints that must keep their pattern."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), PAT, dtype=torch.int32, device=DEV)
        self.out = self.buf[GUARD:GUARD + n]

    def ptr(self):
        return C.c_void_p(self.out.data_ptr())

    def intact(self):
        return bool((self.buf[:GUARD] == PAT).all() and (self.buf[GUARD + self.n:] == PAT).all())

    def untouched(self):
        return bool((self.buf == PAT).all())


def bands_kept(g, what):
    """The guard bands of a Guarded buffer whose payload need not be written everywhere (or may hold NaN on purpose)."""
    band = torch.ones(g.rows + 2, g.ld, dtype=torch.bool, device=DEV)
    band[1:g.rows + 1, :g.cols] = False
    assert (g.buf.view(g.rows + 2, g.ld)[band] == g.pat).all(), "%s: a store landed in the guard band" % what


# ---- hig_clip_embed_index_build ----------------------------------------------------------------------------------------------------------
def device_index(tok, vocab):
    """One guarded call -> (counts, the whole capacity buffer as numpy)."""
    B, Nn = tok.shape
    ints, nbytes = lib().hig_clip_embed_index_cap_ints(B, Nn, vocab), lib().hig_clip_embed_index_scratch_bytes(B, Nn, vocab)
    assert ints > 0 and nbytes > 0 and nbytes % 4 == 0
    index, counts, scratch = IBand(ints), IBand(3), IBand(nbytes // 4)
    tokens = torch.from_numpy(tok).to(DEV)
    _lib.check(lib().hig_clip_embed_index_build(P(tokens), B, Nn, vocab, index.ptr(), counts.ptr(), scratch.ptr(), stream()))
    torch.cuda.synchronize()
    assert index.intact() and counts.intact() and scratch.intact(), "hig_clip_embed_index_build: a store landed in a guard band"
    return tuple(counts.out.cpu().tolist()), index.out.cpu().numpy()


def stub_tokens(B):
    """B captions of a 43-entry table through the stub tokenizer: SOT, word ids, EOT, then token 0 -- one list of many chunks."""
    g = np.random.RandomState(B)
    words = "a person two people one the other shakes hands pushes waves walks slowly away left right jumps hugs bows".split()
    table = [" ".join(words[j] for j in g.randint(0, len(words), g.randint(1, 14))) for _ in range(43)]
    return stub_clip.tokenize([table[i] for i in g.randint(0, 43, B)], truncate=True).numpy()


INDEX_CASES = ([(B, Nn, v, kind) for B, Nn, v in ((1, 1, 1), (3, 8, 64), (1, 77, 49408), (8, 77, 49408))
                for kind in ("captions", "distinct", "equal", "mixed")]
               + [(1, 64, 5, "equal"), (1, 65, 5, "equal"), (1, 64, 5, "mixed"), (1, 65, 5, "mixed")]       # B N = 64 | 65: the chunk boundary
               + [(SB.SORT_TILE, 1, 64, "mixed"), (SB.SORT_TILE + 1, 1, 64, "mixed"),                       # 32 768 | 32 769 keys: one LDS tile | two
                  (SB.SORT_TILE + 1, 1, 49408, "distinct"), (480, 77, 49408, "captions"),                    # 36 960 rows: the 120-pair PIT batch
                  (SB.MAX_ROWS, 1, SB.MAX_VOCAB, "distinct")])                                               # the last covered row and id


@pytest.mark.parametrize("B, Nn, vocab, kind", INDEX_CASES, ids=["%dx%d-v%d-%s" % c for c in INDEX_CASES])
def test_index_build_equals_the_host_index_exactly(B, Nn, vocab, kind):
    tok = stub_tokens(B) if (kind == "captions" and vocab == stub_clip.VOCAB and Nn == N) else SB.pattern(kind, B, Nn, vocab, seed=B + Nn)
    assert tok.shape == (B, Nn) and tok.dtype == np.int64
    ix = CT.EmbedIndex(torch.from_numpy(tok), vocab)
    counts, got = device_index(tok, vocab)
    assert counts == (ix.n_live, ix.n_chunks, ix.n_ids), (counts, (ix.n_live, ix.n_chunks, ix.n_ids))
    lay = CT.index_capacity(B, Nn, vocab)[0]
    for name, n in SB.live_lengths(counts, B, Nn).items():
        lo = lay[name][0]
        assert n <= lay[name][1] and np.array_equal(got[lo:lo + n], getattr(ix, name)), name
    if B * Nn <= 4096:      # the plain restatement too (a python loop over the rows)
        rc, arrays, _ = SB.capacity_restated(tok, vocab, CHUNK)
        assert rc == counts and all(np.array_equal(got[lay[f][0]:lay[f][0] + n], arrays[f][:n]) for f, n in SB.live_lengths(counts, B, Nn).items())
    if kind == "captions" and B * Nn > 4 * CHUNK:
        assert ix.id_seg[1] - ix.id_seg[0] > 1 and ix.ids[0] == 0                        # token 0: one list of many chunks
    if kind == "mixed":
        assert ix.n_live < B * Nn                                                         # ids -1 and vocab are not live
    counts2, again = device_index(tok, vocab)
    assert counts2 == counts and np.array_equal(again, got)                               # two runs: the same bits


def test_index_build_refuses_one_row_past_its_range_with_nothing_written():
    L = lib()
    index, counts, scratch = IBand(1 << 18), IBand(3), IBand(1 << 16)
    tokens = torch.zeros(SB.MAX_ROWS + 1, dtype=torch.int64, device=DEV)
    for B, Nn, vocab in ((SB.MAX_ROWS + 1, 1, 64), (1, SB.MAX_ROWS + 1, 64), (852, 77, 49408), (8, 77, SB.MAX_VOCAB + 1)):
        assert L.hig_clip_embed_index_build(P(tokens), B, Nn, vocab, index.ptr(), counts.ptr(), scratch.ptr(), stream()) == _lib.EUNSUPPORTED
        assert "cover" in _lib.last_error() and L.hig_clip_embed_index_scratch_bytes(B, Nn, vocab) == -1
    torch.cuda.synchronize()
    assert index.untouched() and counts.untouched() and scratch.untouched()


# ---- hig_clip_embed_bwd_dev --------------------------------------------------------------------------------------------------------------
def embed_pair(dx0, tokens, vocab, W):
    """dtok, dpos through hig_clip_embed_bwd under the host index and through hig_clip_embed_bwd_dev under the device index."""
    B, Nn = tokens.shape
    ix = CT.EmbedIndex(tokens, vocab).to(DEV)
    dix = CT.DeviceEmbedIndex(B, Nn, vocab, DEV).build(tokens.to(DEV))
    out = []
    for dev_route in (False, True):
        dtok, dpos = Guarded(vocab, W, pad=0), Guarded(Nn, W, pad=0)
        if dev_route:
            floats = lib().hig_clip_embed_bwd_dev_scratch_floats(B, Nn, W, vocab)
            assert floats > 0 and floats % W == 0 and floats <= 2 * B * Nn * W
            scratch = Guarded(floats // W, W, pad=0)
            _lib.check(lib().hig_clip_embed_bwd_dev(P(dx0), B, Nn, W, vocab, P(dix.index), P(dix.counts), scratch.ptr(), dtok.ptr(), dpos.ptr(),
                                                    stream()))
        else:
            scratch = Guarded(ix.n_chunks + ix.n_ids, W, pad=0)
            _lib.check(lib().hig_clip_embed_bwd(P(dx0), B, Nn, W, vocab, P(ix.dev), ix.n_live, ix.n_chunks, ix.n_ids, scratch.ptr(), dtok.ptr(),
                                                dpos.ptr(), stream()))
        torch.cuda.synchronize()
        for g, what in ((scratch, "scratch"), (dtok, "dtok"), (dpos, "dpos")):
            bands_kept(g, what)
        out.append((dtok.out.clone(), dpos.out.clone()))
    return ix, out


@pytest.mark.parametrize("W", [128, 6])
def test_embedding_gradient_on_the_device_index_is_the_host_index_entry_bit_for_bit(W):
    from test_cpu_clip_train import embed_case
    tokens, vocab, _ = embed_case(W, seed=W)
    B, Nn = tokens.shape
    g = torch.Generator().manual_seed(W)
    dx0 = torch.randn(B * Nn, W, generator=g) * 10.0 ** (torch.rand(B * Nn, 1, generator=g) * 8 - 4)
    ix, ((tok_h, pos_h), (tok_d, pos_d)) = embed_pair(dx0.to(DEV), tokens, vocab, W)
    want_tok, want_pos = CT.embed_grad_restated(dx0.numpy(), ix, W)
    for got_tok, got_pos in ((tok_h, pos_h), (tok_d, pos_d)):
        assert np.array_equal(got_tok.cpu().numpy().view(np.int32), want_tok.view(np.int32))      # bit for bit, the sign of zero included
        assert np.array_equal(got_pos.cpu().numpy().view(np.int32), want_pos.view(np.int32))
    unused = sorted(set(range(vocab)) - set(int(t) for t in ix.ids))
    assert len(unused) > 50 and not bits(tok_d[unused]).any()                                     # exactly +0.0
    # rows whose id is dead (-1, vocab) are in no list: NaN there reaches no token gradient
    dead = ((tokens.view(-1) < 0) | (tokens.view(-1) >= vocab)).nonzero().flatten()
    assert len(dead) == 2
    poisoned = dx0.clone()
    poisoned[dead] = float("nan")
    _, ((tok_hn, pos_hn), (tok_dn, pos_dn)) = embed_pair(poisoned.to(DEV), tokens, vocab, W)
    assert torch.equal(bits(tok_dn), bits(tok_d)) and torch.equal(bits(tok_hn), bits(tok_d))
    assert torch.equal(bits(pos_dn), bits(pos_hn)) and torch.isnan(pos_dn).any()                  # (dpos sums every row, as before)


# ---- hig_clip_text_bwd_dev -----------------------------------------------------------------------------------------------------------------
def tower_grads(table, c, tokens, dout, route, dix=None):
    """hig_clip_text_fwd_train + the adjoint with every gradient in a guarded buffer; route "host" | "dev"."""
    dims = CT.clip_dims(c["B"], N, c["W"], c["H"], c["L"], c["vocab"])
    out = Guarded(c["B"] * N, c["W"], pad=0)
    grads = [Guarded(p.shape[0] if p.dim() == 2 else 1, p.shape[-1], pad=0) for p in table.tensors]
    saved = Guarded(1, lib().hig_clip_text_train_bytes(dims) // 4, pad=0)
    bws = Guarded(1, lib().hig_clip_text_bwd_workspace_bytes(dims) // 4, pad=0)
    gtable = (C.c_void_p * len(grads))(*[g.out.data_ptr() for g in grads])
    tok, d_out = tokens.to(DEV), dout.to(DEV)
    _lib.check(lib().hig_clip_text_fwd_train(dims, table.table, P(tok), out.ptr(), saved.ptr(), stream()))
    if route == "host":
        ix = CT.EmbedIndex(tokens, c["vocab"]).to(DEV)
        _lib.check(lib().hig_clip_text_bwd(dims, table.table, P(ix.dev), ix.n_live, ix.n_chunks, ix.n_ids, P(d_out), saved.ptr(), gtable, bws.ptr(),
                                           stream()))
    else:
        dix = CT.DeviceEmbedIndex(c["B"], N, c["vocab"], DEV).build(tok)
        _lib.check(lib().hig_clip_text_bwd_dev(dims, table.table, P(dix.index), P(dix.counts), P(d_out), saved.ptr(), gtable, bws.ptr(), stream()))
    torch.cuda.synchronize()
    bands_kept(saved, "saved"), bands_kept(bws, "backward workspace")
    return [g.verify("gradient %d" % i).view(p.shape).clone() for i, (g, p) in enumerate(zip(grads, table.tensors))]


def test_tower_adjoint_on_the_device_index_is_the_host_index_entry_bit_for_bit():
    from test_gpu_clip_train import TOWERS, tower_case
    m, tokens, dout, _, _ = tower_case("w128")
    c = TOWERS["w128"]
    assert (c["W"], c["H"], c["L"], c["vocab"], c["B"]) == (128, 2, 2, 64, 3)
    table = CT.TrainTowerTable(m, torch.device(DEV, 0))
    host, dev = tower_grads(table, c, tokens, dout, "host"), tower_grads(table, c, tokens, dout, "dev")
    for i, (a, b) in enumerate(zip(host, dev)):
        assert torch.equal(bits(a), bits(b)), "gradient %d" % i
    assert host[0].abs().sum() > 0 and host[1].abs().sum() > 0


def test_one_captured_graph_serves_three_token_sets_of_a_shape():
    """Index build + adjoint captured once, replayed with three different token sets: each replay equals the eager host-index
    route for ITS tokens.  A count baked into the graph fails the second replay."""
    import clip_bounds as CB
    from test_gpu_clip_train import TOWERS, tower_case
    m, tokens, dout, _, _ = tower_case("w128")
    c = TOWERS["w128"]
    table = CT.TrainTowerTable(m, torch.device(DEV, 0))
    sets = [tokens, CB.tower_tokens(c["B"], N, c["vocab"], seed=31), torch.from_numpy(SB.pattern("mixed", c["B"], N, c["vocab"], seed=5))]
    host_counts = [(ix.n_live, ix.n_chunks, ix.n_ids) for ix in (CT.EmbedIndex(t, c["vocab"]) for t in sets)]
    assert len(set(host_counts)) == 3, host_counts                                        # three different counts: the test has teeth
    eager = []
    for t in sets:
        out, saved = CT.tower_forward_train(table, t.to(DEV))
        grads = CT.tower_backward(table, CT.EmbedIndex(t, c["vocab"]).to(DEV), dout.to(DEV), saved)
        torch.cuda.synchronize()
        eager.append([g.clone() for g in grads])
    dims = CT.clip_dims(c["B"], N, c["W"], c["H"], c["L"], c["vocab"])
    saved = torch.empty(lib().hig_clip_text_train_bytes(dims), dtype=torch.uint8, device=DEV)
    bws = torch.empty(lib().hig_clip_text_bwd_workspace_bytes(dims), dtype=torch.uint8, device=DEV)
    static_tok, out, d_out = sets[2].to(DEV).clone(), torch.empty(c["B"], N, c["W"], device=DEV), dout.to(DEV)
    dix = CT.DeviceEmbedIndex(c["B"], N, c["vocab"], DEV)
    grads = [torch.empty_like(p) for p in table.tensors]
    gtable = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])

    def call():
        dix.build(static_tok)
        _lib.check(lib().hig_clip_text_fwd_train(dims, table.table, P(static_tok), P(out), P(saved), stream()))
        _lib.check(lib().hig_clip_text_bwd_dev(dims, table.table, P(dix.index), P(dix.counts), P(d_out), P(saved), gtable, P(bws), stream()))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for k in (0, 1, 2, 0):
        static_tok.copy_(sets[k].to(DEV))
        for g in grads:
            g.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert tuple(dix.counts.cpu().tolist()) == host_counts[k]
        for i, (g, w) in enumerate(zip(grads, eager[k])):
            assert torch.equal(bits(g), bits(w)), "replay with token set %d: gradient %d" % (k, i)


# ---- the step -----------------------------------------------------------------------------------------------------------------------------
def named(m):
    return {k: p.detach().double().cpu().clone() for k, p in m.named_parameters()}


@functools.lru_cache(maxsize=None)
def fused_run(dedup, steps=W.STEPS):
    """STEPS fused steps -> (losses, total update of every parameter, token_embedding before and after)."""
    m = W.build(clip_tower_train="flat").to(DEV).train()
    tr = W.pit_trainer(m)
    before, losses = named(m), []
    for k in range(steps):
        losses.append(W.fused_step(tr, m, k, dedup=dedup).item())
    torch.cuda.synchronize()
    after = named(m)
    fp = m.flat_params()
    assert fp.tower_params and tr.fused_state()["covered"] == fp.numel and tr.fused_state()["step"].item() == steps
    return losses, {k: after[k] - before[k] for k in before}, (before["clip.token_embedding.weight"], after["clip.token_embedding.weight"])


@functools.lru_cache(maxsize=None)
def autograd_run(option):
    """The same steps through DDPMMulTrainer.forward() + update() (torch.optim.Adam) with injected t and noise."""
    from test_gpu_denoiser import _patch
    c = W.case()
    m = W.build(**({} if option is None else {"clip_tower_train": option})).to(DEV).train()
    tr = W.pit_trainer(m)
    tr.opt_encoder = torch.optim.Adam(m.parameters(), lr=2e-4)
    t_fixed = torch.tensor(c["t"])
    tr.sampler.sample = lambda bs, dev: (t_fixed.to(dev), torch.ones(bs))
    before, losses = named(m), []
    for k in range(W.STEPS):
        m1, m2, noise = W.motions(k)
        undo = _patch(type("F", (), {"randn": None, "randn_like": staticmethod(lambda x, noise=noise, **_: noise.to(DEV))})())
        try:
            tr.forward((list(W.CAP1[k]), list(W.CAP2[k]), m1, m2, torch.tensor(c["lengths"]), None))
            losses.append(tr.update()["loss_mot_rec"])
        finally:
            undo()
    torch.cuda.synchronize()
    after = named(m)
    return losses, {k: after[k] - before[k] for k in before}, dict(m.clip_train_stats), tr.diffusion


@functools.lru_cache(maxsize=None)
def fp64_run():
    """The same steps in fp64 on torch ops, on the CPU: the text side through the model's own modules, the denoiser through the
    oracle's functional forward, then the PIT loss, clip_grad_norm_(0.5) and torch.optim.Adam."""
    from oracle import fill
    from oracle import interaction_ref as IR
    from torch.nn.utils import clip_grad_norm_
    diffusion = autograd_run("hip")[3]
    c = W.case()
    m = W.build(text_head="torch").double()
    m.clip.d_type = torch.float64
    opt = torch.optim.Adam(m.parameters(), lr=2e-4)
    params = dict(m.named_parameters())
    core = {k: params[k] for k in fill.interaction_params(c["F"], c["d"], c["ff"], c["L"], c["Lt"], c["num_frames"])}
    B, T = c["B"], c["T"]
    t = torch.tensor(c["t"])
    t2 = torch.cat([t, t])
    sa = torch.from_numpy(diffusion.sqrt_alphas_cumprod)[t2][:, None, None]
    sb = torch.from_numpy(diffusion.sqrt_one_minus_alphas_cumprod)[t2][:, None, None]
    before, losses = named(m), []
    for k in range(W.STEPS):
        m1, m2, noise = W.motions(k)
        x0, nz = torch.cat([m1, m2]).double(), noise.double()
        x_t = sa * x0 + sb * nz
        x_t = torch.cat([x_t[:B], x_t[:B], x_t[B:], x_t[B:]])
        target = torch.cat([nz[:B], nz[:B], nz[B:], nz[B:]])
        length = torch.tensor(c["lengths"] * 4)
        xf_proj, xf_out = m.encode_text(W.rows_of(k), "cpu")
        pred = IR.interaction_forward(core, x_t, torch.cat([t2, t2]), length, xf_proj, xf_out, c["H"], c["L"])
        mask = (torch.arange(T)[None, :] < length[:, None]).double()
        loss = IR.pit_loss(pred, target, mask)
        opt.zero_grad()
        loss.backward()
        clip_grad_norm_(m.parameters(), 0.5)
        opt.step()
        losses.append(loss.item())
    after = named(m)
    return losses, {k: after[k] - before[k] for k in before}


def distances(upd, upd64):
    """{name: rel-L2 of the total update from the fp64 one}, the key third of every attn.in_proj_bias left out."""
    out = {}
    for k, r in upd64.items():
        a, r = SB.without_key_third(k, upd[k], r)
        assert r.norm() > 0, k
        out[k] = SB.rel(a, r)
    return out


def test_fused_step_without_dedup_against_forward_update_and_fp64():
    """Losses: fused (dedup off) against forward() + update() under "hip" within 1e-5 relative, per step.  Total update of every
    parameter against fp64: within 4 x the distance of the torch route (forward() + update() with the tower on torch ops).
    Measured on the MI355X: see the figures this test prints (recorded in the README's section)."""
    loss_f, upd_f, _ = fused_run(False)
    loss_h, _, stats, _ = autograd_run("hip")
    loss_t, upd_t, stats_t, _ = autograd_run(None)
    loss64, upd64 = fp64_run()
    assert stats == {"native_forwards": W.STEPS, "native_backwards": W.STEPS, "native_inference": 0} and stats_t["native_forwards"] == 0
    print("losses: fused %s, hip %s, torch %s, fp64 %s" % (loss_f, loss_h, loss_t, loss64))
    for a, b in zip(loss_f, loss_h):
        assert abs(a - b) <= SB.LOSS_REL * abs(b), (a, b)
    assert set(upd_f) == set(upd64) == set(upd_t)
    d_f, d_t = distances(upd_f, upd64), distances(upd_t, upd64)
    worst, failed = (0.0, None), []
    for k in upd64:
        ratio = d_f[k] / d_t[k] if d_t[k] > 0 else (0.0 if d_f[k] == 0 else float("inf"))
        print("update %-58s fused %.2e / torch fp32 %.2e = %.2f" % (k, d_f[k], d_t[k], ratio))
        worst = max(worst, (ratio, k))
        if not d_f[k] <= SB.UPDATE_FACTOR * d_t[k]:
            failed.append((k, d_f[k], d_t[k]))
    print("total update over %d steps: worst fused distance / torch distance %.2f (%s)" % (W.STEPS, *worst))
    assert not failed, failed


def test_dedup_on_against_off_holds_the_caption_banks_gate():
    """Per parameter: rel-L2 of the total update from fp64 with dedup <= max(1e-6, 4 x that without)."""
    loss_on, upd_on, _ = fused_run(True)
    loss_off, upd_off, _ = fused_run(False)
    _, upd64 = fp64_run()
    print("losses: dedup on %s, off %s" % (loss_on, loss_off))
    for a, b in zip(loss_on, loss_off):
        assert abs(a - b) <= SB.LOSS_REL * abs(b), (a, b)
    d_on, d_off = distances(upd_on, upd64), distances(upd_off, upd64)
    worst, failed = (0.0, None), []
    for k in upd64:
        gate = max(SB.DEDUP_FLOOR, SB.DEDUP_FACTOR * d_off[k])
        print("dedup %-59s on %.2e off %.2e gate %.2e" % (k, d_on[k], d_off[k], gate))
        worst = max(worst, (d_on[k] / gate, k))
        if not d_on[k] <= gate:
            failed.append((k, d_on[k], gate))
    print("dedup: worst distance / gate %.3f (%s)" % worst)
    assert not failed, failed
    assert any(not torch.equal(upd_on[k], upd_off[k]) for k in upd64)      # (another order of fp32 sums: not the same bits)


@pytest.mark.parametrize("dedup", [True, False])
def test_token_embedding_rows_no_caption_used_keep_their_bits(dedup):
    _, _, (before, after) = fused_run(dedup)
    used = set()
    for k in range(W.STEPS):
        used |= set(stub_clip.tokenize(W.rows_of(k), truncate=True).view(-1).tolist())
    unused = torch.tensor(sorted(set(range(stub_clip.VOCAB)) - used))
    assert len(unused) > 49000 and torch.equal(before[unused], after[unused])
    moved = torch.tensor(sorted(used))
    assert (before[moved] != after[moved]).any(dim=1).all()                # and every row a caption used did move


def lossaware(**extra):
    return dict(loss_weighting="min_snr", min_snr_gamma=5.0, sampler="loss-second-moment", ema_decay=0.99, **extra)


def step_state(tr, m):
    st, ema = tr.fused_state(), tr.ema_state()
    out = [m.flat_params().flat, st["m"], st["v"], st["loss"], st["gnorm"], st["step"], ema["flat"]]
    smp = tr._loss_state(m.flat_params().flat.device)[1]
    return out + list(smp.tensors()), ema["num_updates"]


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_captured_step_equals_the_fused_step_bit_for_bit_over_three_caption_lists(storage):
    """Under min-SNR weighting + loss-aware sampling, with an EMA: loss, parameters, both moments, gradient norm, the EMA and its
    count and the loss history, after each of three steps whose caption lists differ and share (rows, U_pad): ONE graph."""
    twins = []
    for _ in range(2):
        m = W.build(clip_tower_train="flat", storage=storage, heads=2 if storage == "bf16" else None).to(DEV).train()   # (bf16: head dim 64)
        twins.append((W.pit_trainer(m, **lossaware()), m))
    (tf, mf), (tc, mc) = twins
    for k in range(W.STEPS):
        t = torch.tensor([(v + 77 * k) % 1000 for v in W.case()["t"]], device=DEV)
        W.fused_step(tf, mf, k, t=t)
        W.fused_step(tc, mc, k, captured=True, t=t)
        torch.cuda.synchronize()
        (a, na), (b, nb) = step_state(tf, mf), step_state(tc, mc)
        diff = [i for i, (x, y) in enumerate(zip(a, b)) if not torch.equal(bits(x) if x.dtype == torch.float32 else x, bits(y) if y.dtype == torch.float32 else y)]
        assert not diff and na == nb == k + 1, (storage, k, diff, na, nb)
        assert torch.isfinite(a[3]).all()
    graphs = tc.fused_state()["graphs"]
    assert len(graphs) == 1 and not tf.fused_state()["graphs"] and next(iter(graphs))[1] == "tokens"
    fp = mc.flat_params()
    o = fp.tower_offsets[0]
    assert not torch.equal(tc.ema_state()["flat"][o:], fp.flat[o:])        # the EMA's twin covers the tower, and lags it


def test_save_load_continue_ema_and_the_reference_layout(tmp_path):
    def fresh():
        m = W.build(clip_tower_train="flat").to(DEV).train()
        return W.pit_trainer(m, fused_step=True, ema_decay=0.99), m
    ta, ma = fresh()
    for k in range(W.STEPS):
        W.fused_step(ta, ma, k)
    tb, mb = fresh()
    for k in range(W.STEPS - 1):
        W.fused_step(tb, mb, k)
    path = str(tmp_path / "latest.tar")
    tb.save(path, 0, W.STEPS - 1)
    ck = torch.load(path, map_location="cpu")
    # 'encoder_ema' carries the tower; the optimizer state is torch.optim.Adam's over a reference-layout model
    tower_keys = {k for k in ck["encoder"] if k.startswith("clip.")}
    assert len(tower_keys) == 4 + 12 * W.TOWER["L"] and tower_keys <= set(ck["encoder_ema"])
    fpb, stb = mb.flat_params(), tb.fused_state()
    o = fpb.tower_offsets[0]
    assert torch.equal(ck["encoder_ema"]["clip.token_embedding.weight"].view(-1), tb.ema_state()["flat"][o:o + fpb.tower_params[0].numel()].cpu())
    plain = W.build(text_head="torch")
    plain.load_state_dict(ck["encoder"], strict=True)
    adam = torch.optim.Adam(plain.parameters(), lr=2e-4)
    adam.load_state_dict(ck["opt_encoder"])
    by_name = dict(plain.named_parameters())
    names = {id(p): k for k, p in mb.named_parameters()}
    for p, off in zip(fpb.tower_params, fpb.tower_offsets):
        ent = adam.state[by_name[names[id(p)]]]
        assert float(ent["step"]) == W.STEPS - 1
        assert torch.equal(ent["exp_avg"].view(-1), stb["m"][off:off + p.numel()].cpu()), names[id(p)]
        assert torch.equal(ent["exp_avg_sq"].view(-1), stb["v"][off:off + p.numel()].cpu()), names[id(p)]
    # load -> continue equals uninterrupted
    tc, mc = fresh()
    assert tc.load(path) == (0, W.STEPS - 1)
    W.fused_step(tc, mc, W.STEPS - 1)
    torch.cuda.synchronize()
    for what, a, b in (("flat", ma.flat_params().flat, mc.flat_params().flat), ("m", ta.fused_state()["m"], tc.fused_state()["m"]),
                       ("v", ta.fused_state()["v"], tc.fused_state()["v"]), ("ema", ta.ema_state()["flat"], tc.ema_state()["flat"]),
                       ("loss", ta.fused_state()["loss"], tc.fused_state()["loss"])):
        assert torch.equal(bits(a), bits(b)), what
    assert ta.ema_state()["num_updates"] == tc.ema_state()["num_updates"] == W.STEPS and tc.fused_state()["step"].item() == W.STEPS
    # the ema_weights() scope: the averaged tower inside, the model's own bits back outside
    own = ma.flat_params().flat.clone()
    with ta.ema_weights():
        inside = ma.clip.ln_final.weight.detach().clone()
    assert torch.equal(bits(ma.flat_params().flat), bits(own))
    o3 = ma.flat_params().tower_offsets[2]
    assert torch.equal(bits(inside), bits(ta.ema_state()["flat"][o3:o3 + inside.numel()])) and not torch.equal(inside, ma.clip.ln_final.weight.detach())
    # encode_text under no_grad: the model that trained equals a model loaded from its state dict
    sd = copy.deepcopy(ma.state_dict())
    other = W.build(clip_tower_train="hip").to(DEV).eval()
    other.load_state_dict(sd, strict=True)
    ma.eval()
    with torch.no_grad():
        p1, o1 = ma.encode_text(W.rows_of(0), DEV)
        p2, o2 = other.encode_text(W.rows_of(0), DEV)
    assert torch.equal(bits(p1), bits(p2)) and torch.equal(bits(o1), bits(o2))
    assert ma.clip_train_stats["native_inference"] == 1 and ma.flat_params().valid()


def test_autograd_route_keeps_working_on_the_rehomed_tower():
    """forward() + update() with "flat" is forward() + update() with "hip", bit for bit: the same kernels on the same values, the
    parameters merely live in the flat buffer."""
    loss_h, upd_h, _, _ = autograd_run("hip")
    loss_f, upd_f, stats, _ = autograd_run("flat")
    assert stats == {"native_forwards": W.STEPS, "native_backwards": W.STEPS, "native_inference": 0}
    assert loss_f == loss_h and all(torch.equal(upd_f[k], upd_h[k]) for k in upd_h)


def test_every_other_source_still_refuses_this_model():
    c = W.case()
    m = W.build(clip_tower_train="flat").to(DEV).train()
    tr = W.pit_trainer(m)
    m1, m2, noise = W.motions(0)
    x0, t, length = torch.cat([m1, m2]).to(DEV), torch.tensor(c["t"], device=DEV), torch.tensor(c["lengths"], device=DEV)
    rows = 4 * c["B"]
    clip_out, eot = torch.zeros(rows, N, 512, device=DEV), torch.zeros(rows, dtype=torch.int64, device=DEV)
    xp, xo = torch.zeros(rows, 4 * c["d"], device=DEV), torch.zeros(rows, N, c["Lt"], device=DEV)
    before = m.flat_params().flat.clone()
    for step in (tr.train_step_fused, tr.train_step_captured):
        with pytest.raises(NotImplementedError, match="would silently freeze it"):
            step(x0, t, length, noise=noise.to(DEV), clip_out=clip_out, eot=eot)
        with pytest.raises(NotImplementedError, match="would silently freeze it"):
            step(x0, t, length, noise=noise.to(DEV), xf_proj=xp, xf_out=xo)
    with pytest.raises(ValueError, match="trainable parameters"):
        m.enable_caption_bank(16)
    assert torch.equal(m.flat_params().flat, before)
    # and a "hip" model keeps today's refusal, in today's words, with today's buffer
    hip = W.build(clip_tower_train="hip").to(DEV).train()
    th = W.pit_trainer(hip)
    with pytest.raises(NotImplementedError, match="use forward\\(\\) \\+ update\\(\\) for this configuration"):
        th.train_step_fused(x0, t, length, noise=noise.to(DEV), clip_out=clip_out, eot=eot)
    fp = hip.flat_params()
    assert fp.tower_params == [] and fp.numel == fp.core_numel + sum((p.numel() + 63) // 64 * 64 for p in fp.text_params)
    with pytest.raises(ValueError, match="token_batch= needs"):
        W.fused_step(th, hip, 0)


NEW_ENTRIES = ("hig_clip_embed_index_build", "hig_clip_embed_bwd_dev", "hig_clip_text_bwd_dev", "hig_clip_embed_index_cap_ints",
               "hig_clip_embed_index_scratch_bytes", "hig_clip_embed_bwd_dev_scratch_floats")


def test_with_the_option_unset_no_new_entry_is_called(monkeypatch):
    from test_gpu_loss_weighting import counted
    proxy = counted(monkeypatch)
    autograd_run.__wrapped__("hip")
    assert proxy.calls.get("hig_clip_text_bwd") == W.STEPS and not [n for n in NEW_ENTRIES if n in proxy.calls], proxy.calls
    proxy.calls.clear()
    m = W.build(clip_tower_train="flat").to(DEV).train()
    W.fused_step(W.pit_trainer(m), m, 0)
    assert proxy.calls.get("hig_clip_embed_index_build") == 1 and proxy.calls.get("hig_clip_text_bwd_dev") == 1
    assert "hig_clip_text_bwd" not in proxy.calls and proxy.calls.get("hig_rows_gather_f32") == 2 and proxy.calls.get("hig_sumsq_partial") == 1


def test_exchange_on_one_rank_is_the_identity_for_the_tower_step():
    assert _WORKER is not None, "the worker process was not started"
    outdir, proc = _WORKER
    code = proc.wait(timeout=600)
    log = open(os.path.join(outdir, "rank0.log"), errors="replace").read()
    assert code == 0, log[-6000:]
    got = torch.load(os.path.join(outdir, "tower_step.pt"))
    assert "HIG_FORCE_EXCHANGE" not in os.environ
    ref = W.exchange_step()                                   # this process: no process group, no exchange
    assert got["numel"] > got["tower0"] > got["core_numel"]
    # 2 L + 2 ranges of the core and ONE tail range (core_numel, n) over the text head and the tower
    assert got["n_allreduce"] == 2 * got["L"] + 3, got["n_allreduce"]
    assert got["loss"] == ref["loss"] and got["gnorm"] == ref["gnorm"] and got["step"] == ref["step"] == 1
    for k in ("flat", "m", "v"):
        assert torch.equal(got[k], ref[k]), k
    assert (got["m"][got["tower0"]:] != 0).any()              # the tower's gradient went through the exchange and into Adam
