"""Class-id (cap_id) models on the fused and the captured training step, on the MI355X: hig_rows_sum_by_key_f32 bit for bit in
guarded buffers, the class head's two entries (csrc/classhead.hip) against fp64, and DDPMMulTrainer with
MotionInteractionTransformer(cap_id=True, class_head="hip") -- against the autograd sequence over ALL trainable parameters,
against the reference's own step (golden g21, tools/make_golden_class_pit.py), captured against fused, bf16 storage, EMA,
the gradient exchange on one rank, and the option left unset.

Head gate (the project's form for the tower and the dedup route): rel-L2 from the fp64 value <= max(1e-6, 4 x the distance of
the same fp32 torch ops on the CPU from fp64).

The dead tensors.  With ONE text token the softmax over the keys of the text cross-attention is 1, so the per-layer
ca_block.norm / ca_block.query / ca_block.key tensors have a true gradient of zero; what any implementation computes for them
is rounding noise (5e-10 .. 5e-9 and exact zeros on the CPU reference), which Adam's first step turns into steps of about lr.
They are held to `finite and |step| <= 1.01 lr`, every other parameter to the gate of its test."""
import atexit
import ctypes as C
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
from hig_amd import _lib  # noqa: E402
from oracle import fill  # noqa: E402
import class_head_worker as W  # noqa: E402
import ema_bounds as eb  # noqa: E402
from test_gpu_caption_bank import Band, bits, i32, placed  # noqa: E402

DEV = "cuda"
LR = 2e-4
HERE = os.path.dirname(os.path.abspath(__file__))
DEAD = (".ca_block.norm.", ".ca_block.query.", ".ca_block.key.")
IDS1, IDS2 = [3, 41], [4, 3]


def S():
    return _lib.stream_ptr()


def dead(name):
    return any(d in name for d in DEAD)


# The exchange test needs one more process on the GPU, and a process that has initialised the GPU must not start another
# program on the GPU boxes (tests/conftest.py starts its workers after collection for that reason).  A test module has no
# collection hook, so the worker starts when this module is imported -- collection imports every module before any test body
# runs -- and only where there is a device; the test waits for it.
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    return port


_WORKER = None
if torch.cuda.device_count() >= 1:      # (counting devices does not initialise the GPU)
    _out = tempfile.mkdtemp(prefix="hig_classhead_")
    _log = open(os.path.join(_out, "rank0.log"), "wb")
    _WORKER = (_out, subprocess.Popen([sys.executable, os.path.join(HERE, "class_head_worker.py"), _free_port(), _out],
                                      env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), stdout=_log, stderr=subprocess.STDOUT))
    atexit.register(lambda: _WORKER[1].poll() is None and _WORKER[1].kill())


# ---- hig_rows_sum_by_key_f32 ---------------------------------------------------------------------------------------------
def by_key_sum(src, key, n_keys):
    """float32 sums in ascending row order, starting from the first member; a key without rows is +0.0."""
    out = np.zeros((n_keys, src.shape[1]), dtype=np.float32)
    seen = set()
    for r, k in enumerate(key):
        if 0 <= k < n_keys:
            out[k] = src[r] if k not in seen else (out[k] + src[r]).astype(np.float32)
            seen.add(k)
    return out


def key_patterns(rows, g):
    """(n_keys, keys): one key with strays, 43 keys with three in use and strays, and every row on one key of 43."""
    pick = torch.randint(0, 5, (rows,), generator=g).tolist()
    yield 1, [(0, 0, 0, -1, 1)[p] for p in pick]
    yield 43, [(3, 41, 4, -1, 43)[p] for p in pick]
    yield 43, [7] * rows


@pytest.mark.parametrize("row_floats", [1, 3, 5, 32, 2048])
def test_rows_sum_by_key_is_the_float32_sum_in_ascending_row_order(row_floats):
    chunk = _lib.ROWS_KEY_CHUNK
    assert chunk == 1024
    for rows in (1, 7, 640, chunk, chunk + 1):
        g = torch.Generator().manual_seed(1000 * row_floats + rows)
        src = torch.randn(rows, row_floats, generator=g) * 10.0 ** (torch.rand(rows, row_floats, generator=g) * 8 - 4)
        for n_keys, key in key_patterns(rows, g):
            stray = torch.tensor([not 0 <= k < n_keys for k in key])
            poisoned = src.clone()
            poisoned[stray] = float("nan")            # a row whose key is -1 or n_keys is never read
            want = by_key_sum(src.numpy(), key, n_keys)
            assert np.isfinite(want).all()
            used = sorted({k for k in key if 0 <= k < n_keys})
            key_dev = i32(key)
            results = []
            for off_src, off_dst, run in ((0, 0, 0), (0, 0, 1), (1, 1, 0), (1, 0, 0)):       # aligned twice, then unaligned bases
                s = placed(poisoned.to(DEV), off_src)
                out = Band(n_keys * row_floats, off_dst)
                _lib.check(_lib.lib().hig_rows_sum_by_key_f32(C.c_void_p(s.data_ptr()), _lib.ptr(key_dev), rows, row_floats, n_keys,
                                                             out.ptr(), S()))
                torch.cuda.synchronize()
                what = (rows, row_floats, n_keys, off_src, off_dst)
                assert out.intact(), "hig_rows_sum_by_key_f32: a store landed in a guard band %s" % (what,)
                assert out.written(), "hig_rows_sum_by_key_f32: not every element was written %s" % (what,)
                got = out.out.view(n_keys, row_floats).cpu()
                assert not torch.isnan(got).any(), "a row with a key out of range was read %s" % (what,)
                assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32)), what
                unused = [k for k in range(n_keys) if k not in used]
                assert (bits(got[unused]) == 0).all(), "a key without rows is not +0.0 %s" % (what,)
                results.append(got)
            assert all(torch.equal(bits(r), bits(results[0])) for r in results)
    if row_floats == 2048:        # magnitudes 1e-4 .. 1e4: the order of the rows matters, so the test can tell
        flipped = by_key_sum(src.numpy()[::-1].copy(), [7] * rows, 43)
        assert not np.array_equal(flipped[7], want[7])


def test_rows_sum_by_key_is_capturable():
    rows, row_floats, n_keys = 640, 256, 43
    g = torch.Generator().manual_seed(3)
    src = torch.randn(rows, row_floats, generator=g).to(DEV)
    key = torch.randint(0, n_keys, (rows,), generator=g).to(torch.int32).to(DEV)
    out = torch.full((n_keys, row_floats), float("nan"), device=DEV)

    def launch():
        _lib.check(_lib.lib().hig_rows_sum_by_key_f32(_lib.ptr(src), _lib.ptr(key), rows, row_floats, n_keys, _lib.ptr(out), S()))

    launch()
    torch.cuda.synchronize()
    eager = out.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        launch()
    key.copy_((key + 1) % n_keys)         # the replay reads the keys as they are then
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out.roll(-1, 0).cpu()), bits(eager.cpu()))
    assert np.array_equal(eager.cpu().numpy().view(np.int32),
                          by_key_sum(src.cpu().numpy(), ((key - 1) % n_keys).cpu().tolist(), n_keys).view(np.int32))


# ---- the head's two entries ----------------------------------------------------------------------------------------------
def rel64(a, ref):
    return ((a.double().cpu() - ref).norm() / ref.norm()).item()


def head_reference(emb, Wt, b, ids, rp, ro, dtype):
    """xf_proj and the three gradients of  sum(xf_proj rp) + sum(xf_out ro)  through torch ops on the CPU in `dtype`."""
    e, w, bb = (t.to(dtype).clone().requires_grad_(True) for t in (emb, Wt, b))
    xo = e[ids]
    xp = torch.nn.functional.linear(xo, w, bb)
    ((xp * rp.to(dtype)).sum() + (xo.unsqueeze(1) * ro.to(dtype)).sum()).backward()
    return dict(xf_proj=xp.detach(), g_emb=e.grad, g_W=w.grad, g_b=bb.grad)


def launch_head(classes, Lt, E, rows, emb, Wt, b, ids, rp, ro):
    L = _lib.lib()
    ws_f = torch.empty(L.hig_class_head_workspace_bytes(classes, Lt, E, 0), dtype=torch.uint8, device=DEV)
    ws_b = torch.empty(L.hig_class_head_workspace_bytes(classes, Lt, E, 1), dtype=torch.uint8, device=DEV)
    out = dict(xf_out=Band(rows * Lt), xf_proj=Band(rows * E), g_emb=Band(classes * Lt), g_W=Band(E * Lt), g_b=Band(E))

    def run():
        _lib.check(L.hig_class_head_fwd(classes, Lt, E, rows, _lib.ptr(emb), _lib.ptr(Wt), _lib.ptr(b), _lib.ptr(ids),
                                        out["xf_out"].ptr(), out["xf_proj"].ptr(), _lib.ptr(ws_f), S()))
        _lib.check(L.hig_class_head_bwd(classes, Lt, E, rows, _lib.ptr(emb), _lib.ptr(Wt), _lib.ptr(ids), _lib.ptr(ro), _lib.ptr(rp),
                                        out["g_emb"].ptr(), out["g_W"].ptr(), out["g_b"].ptr(), _lib.ptr(ws_b), S()))
    return out, run


@pytest.mark.parametrize("Lt, E", [(32, 256), (256, 512), (256, 256), (32, 512)])
def test_class_head_entries_against_fp64_and_captured_equals_eager(Lt, E):
    classes, ids_host = 43, [3, 41, 4, 3, 4, 3, 3, 41]
    rows = len(ids_host)
    g = torch.Generator().manual_seed(Lt + E)
    emb, Wt, b = torch.randn(classes, Lt, generator=g), torch.randn(E, Lt, generator=g) / Lt ** 0.5, torch.randn(E, generator=g)
    rp, ro = torch.randn(rows, E, generator=g), torch.randn(rows, 1, Lt, generator=g)
    ids_t = torch.tensor(ids_host)
    ref = head_reference(emb, Wt, b, ids_t, rp, ro, torch.float64)
    cpu32 = head_reference(emb, Wt, b, ids_t, rp, ro, torch.float32)
    dev = [t.to(DEV) for t in (emb, Wt, b)] + [i32(ids_host), rp.to(DEV), ro.to(DEV)]
    out, run = launch_head(classes, Lt, E, rows, *dev)
    run()
    torch.cuda.synchronize()
    for k, band in out.items():
        assert band.intact() and band.written(), k
    got = {k: band.out.clone() for k, band in out.items()}
    assert torch.equal(bits(got["xf_out"].view(rows, Lt).cpu()), bits(emb[ids_t]))
    xp = got["xf_proj"].view(rows, E).cpu()
    for i in range(rows):
        for j in range(i):
            if ids_host[i] == ids_host[j]:
                assert torch.equal(bits(xp[i]), bits(xp[j])), (i, j)
    shapes = dict(xf_proj=(rows, E), g_emb=(classes, Lt), g_W=(E, Lt), g_b=(E,))
    for k, shape in shapes.items():
        gate = max(1e-6, 4 * rel64(cpu32[k], ref[k]))
        err = rel64(got[k].view(shape), ref[k])
        print("class head Lt %d E %d: %s rel-L2 %.2e (gate %.2e)" % (Lt, E, k, err, gate))
        assert err <= gate, (k, err, gate)
    unused = sorted(set(range(classes)) - set(ids_host))
    assert (bits(got["g_emb"].view(classes, Lt)[unused].cpu()) == 0).all()          # exactly +0.0
    # captured == eager
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        run()
    for band in out.values():
        band.out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for k, band in out.items():
        assert band.intact() and torch.equal(bits(band.out), bits(got[k])), k


def test_class_head_gives_nan_rows_for_an_id_out_of_range():
    classes, Lt, E = 43, 32, 256
    tr, m = W.pit_trainer(dict(W.CASE, Lt=Lt, d=64, ff=64))
    xp, xo = m._launch_class_head(i32([3, 43, -1, 0]))
    torch.cuda.synchronize()
    assert xo.shape == (4, 1, Lt) and xp.shape == (4, E)
    assert torch.isnan(xp[1:3]).all() and torch.isnan(xo[1:3]).all() and torch.isfinite(xp[[0, 3]]).all()
    assert torch.equal(xo[0, 0], m.cap_embedding[3]) and classes == m.cap_embedding.shape[0]


# ---- the trainer -------------------------------------------------------------------------------------------------------------
def step_inputs(c, tag, with_label):
    B, T, Fd = c["B"], c["T"], c["F"]
    x0 = (fill.tensor_for(tag + ".x0", (2 * B, T, Fd)) * 10).to(DEV)
    noise = (fill.tensor_for(tag + ".noise", x0.shape) * 10).to(DEV)
    tt, length = torch.tensor(c["t"], device=DEV), torch.tensor(c["lengths"], device=DEV)
    c1, c2 = torch.tensor(IDS1, device=DEV), torch.tensor(IDS2, device=DEV)
    text = [c1, c2] if with_label else [c1, c2, c2, c1]
    return x0, noise, tt, length, text, torch.cat(text).to(torch.int32)


@pytest.mark.parametrize("with_label", [False, True])
def test_fused_class_step_equals_the_autograd_sequence_over_all_parameters(with_label):
    """train_step_fused(class_ids=) == training_losses + backward_G + clip_grad_norm_ + Adam over EVERY trainable parameter of a
    default-built (torch class head) model."""
    c = fill.ICASES["config1x2"]
    B, T = c["B"], c["T"]
    rows = 2 * B if with_label else 4 * B
    x0, noise, tt, length, text, ids = step_inputs(c, "cls.fused", with_label)
    label = "labels/" if with_label else None
    tr1, m1 = W.pit_trainer(c, label_path=label, class_head="torch")
    assert m1.flat_params().text_params == []
    opt = torch.optim.Adam(m1.parameters(), lr=LR)
    len_rows = torch.cat([length] * (rows // B))
    out = tr1.diffusion.training_losses(m1, x0, torch.cat([tt, tt]), noise=noise, forward_twice=not with_label,
                                        model_kwargs={"text": text, "length": len_rows})
    tr1.real_noise, tr1.fake_noise = out["target"], out["pred"]
    tr1.src_mask = m1.generate_src_mask(T, len_rows).to(DEV)
    tr1.backward_G()
    tr1.loss_mot_rec.backward()
    gn = torch.nn.utils.clip_grad_norm_(m1.parameters(), 0.5)
    opt.step()
    tr2, m2 = W.pit_trainer(c, label_path=label)
    before = {k: v.clone() for k, v in m2.state_dict().items()}
    l2 = tr2.train_step_fused(x0, tt, length, noise=noise, class_ids=ids)
    st = tr2.fused_state()
    print("fused class step (with_label %s): loss %.6f / %.6f, norm %.6f / %.6f" % (with_label, l2.item(), tr1.loss_mot_rec.item(),
                                                                                     st["gnorm"].item(), gn.item()))
    assert abs(l2.item() - tr1.loss_mot_rec.item()) < 1e-5 * abs(l2.item())
    assert abs(st["gnorm"].item() - gn.item()) < 1e-4 * gn.item()
    trainable = {k for k, p in m2.named_parameters() if p.requires_grad}
    assert {"cap_embedding", "text_proj.0.weight", "text_proj.0.bias"} <= trainable
    worst = {}
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        if dead(k):
            step = (b - before[k]).abs().max().item()
            assert torch.isfinite(b).all() and step <= 1.01 * LR, (k, step)
        else:
            worst[k] = (a - b).abs().max().item()
            assert worst[k] < 5e-6, (k, worst[k])
    print("   largest parameter distance %.2e (%s)" % max((v, k) for k, v in worst.items()))
    for k in ("cap_embedding", "text_proj.0.weight", "text_proj.0.bias"):
        assert not torch.equal(m2.state_dict()[k], before[k]), "%s did not train" % k
    used = sorted(set(IDS1 + IDS2))
    unused = [k for k in range(43) if k not in used]
    assert torch.equal(m2.cap_embedding[unused], before["cap_embedding"][unused])       # a zero gradient: Adam does not move them


def test_pit_class_fused_batch_matches_reference_golden(gold):
    """train_fused_batch(captured=True) of a cap_id model reproduces the reference's own DDPMMulTrainer.forward + update (golden
    g21) at g9's gates.  On the parent commit the call raises NotImplementedError."""
    g = gold("g21_class_pit.npz")
    c = fill.ICASES["config1x2"]
    trainer, m = W.pit_trainer(c)
    B, T, Fd = c["B"], c["T"], c["F"]
    motion1 = fill.tensor_for("g9.motion1", (B, T, Fd)) * 10
    motion2 = fill.tensor_for("g9.motion2", (B, T, Fd)) * 10
    t_fixed = torch.tensor(c["t"])
    trainer.sampler.sample = lambda bs, dev: (t_fixed.to(dev), torch.ones(bs))
    noise = (fill.tensor_for("g9.noise.0", (2 * B, T, Fd)) * 10).to(DEV)
    batch = ([torch.tensor(g["ids1"])], [torch.tensor(g["ids2"])], motion1, motion2, torch.tensor(c["lengths"]), None)
    loss = trainer.train_fused_batch(batch, captured=True, noise=noise)
    st = trainer.fused_state()
    print("g21: loss %.6f / %.6f, norm %.6f / %.6f" % (loss.item(), float(g["loss_mot_rec"]), st["gnorm"].item(), float(g["gnorm"])))
    assert abs(loss.item() - float(g["loss_mot_rec"])) < 1e-4 * float(g["loss_mot_rec"])
    assert abs(st["gnorm"].item() - float(g["gnorm"])) < 2e-4 * float(g["gnorm"])
    sd = m.state_dict()
    named = [k[2:] for k in g.files if k.startswith("p.")]
    assert {"cap_embedding", "text_proj.0.weight", "text_proj.0.bias"} <= set(named) and not any(dead(k) for k in named)
    for k in named:
        assert (sd[k].cpu() - torch.tensor(g["p." + k])).abs().max().item() < 2e-5, k


def test_captured_class_step_equals_the_fused_one_bit_for_bit():
    """Two replays; the second with other ids, against a fused step with those ids: parameters and both moments."""
    c = fill.ICASES["config1x2"]
    x0, noise, tt, length, _, ids = step_inputs(c, "cls.cap", False)
    ids_b = i32([7, 7, 0, 42, 0, 42, 7, 7])
    (tra, ma), (trb, mb) = W.pit_trainer(c), W.pit_trainer(c)
    for k, step_ids in enumerate((ids, ids_b)):
        la = tra.train_step_fused(x0, tt, length, noise=noise, class_ids=step_ids)
        lb = trb.train_step_captured(x0, tt, length, noise=noise, class_ids=step_ids)
        assert la.item() == lb.item(), (k, la.item(), lb.item())
        sa, sb = tra.fused_state(), trb.fused_state()
        assert torch.equal(ma.flat_params().flat, mb.flat_params().flat), k
        assert torch.equal(sa["m"], sb["m"]) and torch.equal(sa["v"], sb["v"]), k
        assert sa["gnorm"].item() == sb["gnorm"].item() and sa["step"].item() == sb["step"].item() == k + 1
    assert len(trb.fused_state()["graphs"]) == 1                                   # one graph served both id sets
    key = next(iter(trb.fused_state()["graphs"]))
    assert ("class_head", (8,)) in key


def test_class_step_with_bf16_storage_tracks_the_fp32_step():
    """The gates of test_fused_training_step_with_bf16_storage_tracks_the_fp32_step; the class head stays exact fp32 behind the
    bf16 core and the shadow covers the core only."""
    c = W.CASE
    B = c["B"]
    x0 = (fill.tensor_for("cls.bf16.x0", (2 * B, c["T"], c["F"])) * 10).to(DEV)
    g = torch.Generator().manual_seed(5)
    noises = [torch.randn(x0.shape, generator=g).to(DEV) for _ in range(3)]
    tt, length = torch.tensor(c["t"], device=DEV), torch.tensor(c["lengths"], device=DEV)
    ids = i32(W.PIT_IDS[0])
    runs = {}
    for storage in ("f32", "bf16"):
        tr, m = W.pit_trainer(c, storage=storage)
        start = m.flat_params().flat.clone()
        losses, gns = [], []
        for k in range(3):
            losses.append(tr.train_step_fused(x0, tt, length, noise=noises[k], class_ids=ids).item())
            gns.append(tr.fused_state()["gnorm"].item())
            if storage == "bf16":
                fp = m.flat_params()
                assert fp.shadow16_buffer().numel() == fp.core_numel < fp.numel
                assert torch.equal(fp.shadow16_buffer(), fp.flat[:fp.core_numel].to(torch.bfloat16))
        runs[storage] = (losses, gns, m.flat_params().flat - start)
    (l32, g32, u32), (l16, g16, u16) = runs["f32"], runs["bf16"]
    print("class step: loss fp32 %s / bf16 storage %s; grad norm %s / %s" % (l32, l16, g32, g16))
    for a, b in zip(l32, l16):
        assert abs(a - b) < 1e-2 * abs(a)
    for a, b in zip(g32, g16):
        assert abs(a - b) < 2e-2 * abs(a)
    cos = (u32.double() * u16.double()).sum() / (u32.double().norm() * u16.double().norm())
    print("   three-step parameter update: cosine %.5f" % cos.item())
    assert cos.item() > 0.97
    (tra, ma), (trb, mb) = W.pit_trainer(c, storage="bf16"), W.pit_trainer(c, storage="bf16")
    for k in range(3):
        la = tra.train_step_fused(x0, tt, length, noise=noises[k], class_ids=ids)
        lb = trb.train_step_captured(x0, tt, length, noise=noises[k], class_ids=ids)
        assert la.item() == lb.item(), (k, la.item(), lb.item())
    fa, fb = ma.flat_params(), mb.flat_params()
    assert torch.equal(fa.flat, fb.flat) and torch.equal(fa.shadow16_buffer(), fb.shadow16_buffer())


def test_ema_covers_the_class_head_inside_the_flat_twin(tmp_path):
    decay = 0.999
    c = fill.ICASES["config1x2"]
    x0, noise, tt, length, _, ids = step_inputs(c, "cls.ema", False)
    tr, m = W.pit_trainer(c, ema_decay=decay, ema_warmup=False)
    assert tr._ema_outside_params() == []
    e0 = m.flat_params().flat.clone()
    tr.train_step_fused(x0, tt, length, noise=noise, class_ids=ids)
    st = tr.ema_state()
    assert len(st["outside"]) == 0 and st["num_updates"] == 1 and st["flat"].numel() == m.flat_params().numel
    ref, bound = eb.ema_step_bound(e0, m.flat_params().flat, 0, 0, decay, 0)
    r = eb.ratio(st["flat"], ref, bound)
    print("RATIO class head ema %.3f" % r)
    assert r <= 1.0
    fp = m.flat_params()
    o = fp.text_offsets[0]
    assert not torch.equal(st["flat"][o:o + 43 * c["Lt"]], e0[o:o + 43 * c["Lt"]])          # the twin of cap_embedding moved
    path = str(tmp_path / "ck.tar")
    tr.save(path, 0, 1)
    ck = torch.load(path, map_location="cpu")
    assert {"cap_embedding", "text_proj.0.weight", "text_proj.0.bias"} <= set(ck["encoder_ema"])
    assert torch.equal(ck["encoder_ema"]["cap_embedding"], st["flat"][o:o + 43 * c["Lt"]].view(43, c["Lt"]).cpu())
    plain = hig_amd.MotionInteractionTransformer(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                                 num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"], cap_id=True)
    assert plain.class_head == "torch"
    plain.load_state_dict(ck["encoder"], strict=True)
    assert torch.equal(plain.cap_embedding.detach(), m.cap_embedding.detach().cpu())


def test_exchange_on_one_rank_is_the_identity_for_the_class_step():
    assert _WORKER is not None, "the worker process was not started"
    outdir, proc = _WORKER
    code = proc.wait(timeout=600)
    log = open(os.path.join(outdir, "rank0.log"), errors="replace").read()
    assert code == 0, log[-6000:]
    got = torch.load(os.path.join(outdir, "class_head.pt"))
    assert "HIG_FORCE_EXCHANGE" not in os.environ
    ref = W.exchange_steps()                                  # this process: no process group, no exchange
    assert got["captured_form"] == "one graph, exchange inside" and ref["captured_form"] == "one graph"
    assert got["numel"] > got["core_numel"]
    # 2 L + 2 ranges of the core and the tail range (core_numel, n) of the class head, per step: 2 eager + warm-up + capture
    assert got["n_allreduce"] == 4 * (2 * got["L"] + 3), got["n_allreduce"]
    assert got["losses"] == ref["losses"] and got["gnorm"] == ref["gnorm"] and got["step"] == ref["step"] == 4
    for k in ("flat", "m", "v"):
        assert torch.equal(got[k], ref[k]), k


def test_option_unset_keeps_the_refusal_and_the_core_sized_buffer():
    c = fill.ICASES["tiny2"]
    tr, m = W.pit_trainer(c, class_head="torch")
    fp = m.flat_params()
    assert fp.text_params == [] and fp.numel == fp.core_numel
    assert {k for k, _ in tr._ema_outside_params()} == {"cap_embedding", "text_proj.0.weight", "text_proj.0.bias"}
    B, T, Fd = c["B"], c["T"], c["F"]
    batch = ([torch.tensor([3, 41])], [torch.tensor([4, 3])], torch.zeros(B, T, Fd), torch.zeros(B, T, Fd), torch.tensor(c["lengths"]),
             None)
    with pytest.raises(NotImplementedError, match="forward\\(\\)/update\\(\\)"):
        tr.train_fused_batch(batch)
    with pytest.raises(RuntimeError, match="class_head='hip'"):
        tr.train_step_fused(torch.zeros(2 * B, T, Fd, device=DEV), torch.tensor(c["t"], device=DEV),
                            torch.tensor(c["lengths"], device=DEV), class_ids=i32([3, 41, 4, 3, 4, 3, 3, 41]))
    with pytest.raises(RuntimeError, match="cannot train it"):
        tr._fused_numel(True)
