"""The gateway on the MI355X: a call through _lib.api launches what the raw ctypes route launches (same bits), a refused call
launches nothing, and an omitted stream is torch's current stream at the time of the call, so the call is captured.

The raw route below (L.hig_x(_lib.ptr(a), ..., _lib.stream_ptr()) under _lib.check) is how the package called the library before
the gateway existed, written out here once more: the two routes share the kernels and nothing else."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import hig_amd  # noqa: E402
from hig_amd import _lib  # noqa: E402
from oracle import fill  # noqa: E402

DEV = "cuda"
B, T, F = 2, 3, 5
SENTINEL = -12345.5


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def mse_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    pred, target = torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g)
    return pred.to(DEV), target.to(DEV), torch.tensor([3, 1], dtype=torch.int64, device=DEV)


def mse_outputs():
    return (torch.full((1,), SENTINEL, device=DEV), torch.full((B, T, F), SENTINEL, device=DEV),
            torch.zeros(_lib.NORM_BLOCKS, device=DEV))


def raw_masked_mse(pred, target, length):
    loss, dpred, scratch = mse_outputs()
    P = _lib.ptr
    _lib.check(_lib.lib().hig_masked_mse(P(pred), P(target), P(length), B, T, F, P(loss), P(dpred), P(scratch), _lib.stream_ptr()))
    return loss, dpred


def test_masked_mse_through_the_gateway_has_the_raw_routes_bits():
    pred, target, length = mse_inputs(0)
    want_loss, want_dpred = raw_masked_mse(pred, target, length)
    loss, dpred, scratch = mse_outputs()
    assert _lib.api.hig_masked_mse(pred, target, length, B, T, F, loss, dpred, scratch) is None
    assert torch.equal(bits(loss), bits(want_loss)) and torch.equal(bits(dpred), bits(want_dpred))
    assert torch.isfinite(loss).all() and (loss != SENTINEL).all() and (dpred != SENTINEL).all()
    # the stream given in full, as a torch stream and as an address: the same launch
    for stream in (torch.cuda.current_stream(), torch.cuda.current_stream().cuda_stream, _lib.stream_ptr()):
        loss2, dpred2, scratch2 = mse_outputs()
        _lib.api.hig_masked_mse(pred, target, length, B, T, F, loss2, dpred2, scratch2, stream)
        assert torch.equal(bits(loss2), bits(want_loss)) and torch.equal(bits(dpred2), bits(want_dpred))


def tiny_model():
    c = fill.CASES["tiny"]
    m = hig_amd.MotionTransformer(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                  num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"])
    m.load_state_dict(fill.fill_state_dict(m.state_dict()))
    m = m.to(DEV).eval()
    inp = {k: v.to(DEV) for k, v in fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"]).items()}
    return c, m, inp


def test_struct_taking_entries_and_the_tiny_forward_have_the_raw_routes_bits():
    c, m, inp = tiny_model()
    L, P = _lib.lib(), _lib.ptr
    dims = m.dims(c["B"], c["T"], c["N"])
    for training in (0, 1):
        assert _lib.api.hig_workspace_bytes(dims, training) == L.hig_workspace_bytes(C.byref(dims), training) > 0
        assert _lib.api.hig_textctx_bytes(dims, training) == L.hig_textctx_bytes(C.byref(dims), training) > 0
    assert _lib.api.hig_bwd_workspace_bytes(dims) == L.hig_bwd_workspace_bytes(C.byref(dims)) > 0
    # the inference forward as the package launched it by the raw route: text context, then hig_denoiser_fwd_x on the cached context
    x, t, length, xf_proj, xf_out = (inp[k].contiguous() for k in ("x", "t", "length", "xf_proj", "xf_out"))
    fp = m.flat_params()
    textctx = torch.empty(L.hig_textctx_bytes(C.byref(dims), 0), dtype=torch.uint8, device=DEV)
    _lib.check(L.hig_text_context(C.byref(dims), fp.param_table(), P(xf_out), P(textctx), 0, _lib.stream_ptr()))
    ws = torch.empty(L.hig_workspace_bytes(C.byref(dims), 0), dtype=torch.uint8, device=DEV)
    want = torch.full((c["B"], c["T"], c["F"]), SENTINEL, device=DEV)
    _lib.check(L.hig_denoiser_fwd_x(C.byref(dims), fp.param_table(), m._derived32(fp), P(x), P(t), P(length), P(xf_proj), None,
                                    P(textctx), P(want), P(ws), 0, _lib.stream_ptr()))
    assert m.cache_text_context
    got, saved = m._launch_forward(x, t, length, xf_proj, xf_out, training=False)
    assert saved is None and torch.isfinite(want).all() and torch.equal(bits(got), bits(want))
    with torch.no_grad():
        assert torch.equal(bits(m(x, t, length=length, xf_proj=xf_proj, xf_out=xf_out)), bits(want))


def test_refusals_happen_before_the_launch():
    pred, target, length = mse_inputs(1)
    loss, dpred, scratch = mse_outputs()
    scratch.fill_(SENTINEL)
    with pytest.raises(TypeError, match=r"hig_masked_mse.*`length` \(const int64_t\*\).*cuda tensor of torch\.int32"):
        _lib.api.hig_masked_mse(pred, target, length.to(torch.int32), B, T, F, loss, dpred, scratch)
    with pytest.raises(RuntimeError, match=r"hig_masked_mse.*`pred`.*needs ROCm device tensors \(got a cpu tensor\); there is no CPU fallback"):
        _lib.api.hig_masked_mse(pred.cpu(), target, length, B, T, F, loss, dpred, scratch)
    with pytest.raises(TypeError, match="hig_masked_mse takes 10 arguments"):
        _lib.api.hig_masked_mse(pred, target, length, B, T, F, loss, dpred)
    with pytest.raises(TypeError, match=r"`B` \(int32_t\)"):
        _lib.api.hig_masked_mse(pred, target, length, torch.tensor(B, device=DEV), T, F, loss, dpred, scratch)
    torch.cuda.synchronize()
    assert (loss == SENTINEL).all() and (dpred == SENTINEL).all() and (scratch == SENTINEL).all()


def _graph_nodes_and_edges(graph):
    """(nodes, [(from, to), ...]) of a kept torch.cuda.CUDAGraph, asked of the HIP runtime torch runs on."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    for fn in (hip.hipGraphGetNodes, hip.hipGraphGetEdges):
        fn.restype = C.c_int
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphGetEdges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    g, n, e = C.c_void_p(graph.raw_cuda_graph()), C.c_size_t(0), C.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, C.byref(n)) == 0 and hip.hipGraphGetEdges(g, None, None, C.byref(e)) == 0
    src, dst = (C.c_void_p * max(e.value, 1))(), (C.c_void_p * max(e.value, 1))()
    if e.value:
        assert hip.hipGraphGetEdges(g, src, dst, C.byref(e)) == 0
    return n.value, [(src[i], dst[i]) for i in range(e.value)]


def test_an_omitted_stream_is_the_current_stream_at_the_time_of_the_call():
    pred, target, length = mse_inputs(2)
    loss, dpred, scratch = mse_outputs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # warm-up on a side stream: the call follows torch's current stream
        _lib.api.hig_masked_mse(pred, target, length, B, T, F, loss, dpred, scratch)
    torch.cuda.current_stream().wait_stream(side)
    first_loss, first_dpred = raw_masked_mse(pred, target, length)
    torch.cuda.synchronize()
    assert torch.equal(bits(loss), bits(first_loss)) and torch.equal(bits(dpred), bits(first_dpred))
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        _lib.api.hig_masked_mse(pred, target, length, B, T, F, loss, dpred, scratch)
    new_pred, new_target, _ = mse_inputs(3)                 # refill the static inputs, spoil the outputs, replay
    pred.copy_(new_pred)
    target.copy_(new_target)
    length.copy_(torch.tensor([2, 3]))
    loss.fill_(SENTINEL)
    dpred.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    want_loss, want_dpred = raw_masked_mse(new_pred, new_target, length)
    assert torch.equal(bits(loss), bits(want_loss)) and torch.equal(bits(dpred), bits(want_dpred))
    assert not torch.equal(bits(loss), bits(first_loss))
    # what was captured is the entry's launches as one chain: no parallel branches
    nodes, edges = _graph_nodes_and_edges(graph)
    assert nodes >= 1 and len(edges) == nodes - 1
    assert len({a for a, _ in edges}) == len(edges) == len({b for _, b in edges})
