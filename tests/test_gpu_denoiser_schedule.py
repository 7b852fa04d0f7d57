"""The schedule the denoiser entry points really ran (hig_denoiser_last_schedule) against the plan asked with the facts the test
knows (hig_denoiser_plan, which tests/test_cpu_denoiser_plan.py holds to the rules without a GPU), on the smallest shapes that
reach every branch: everything goes through the Python model, so the real entry points build the call.  Where a plan field
selects a kernel, the launch counters must agree.  Run as a script it is the child process of the tests that need another
switch setting (the switches are read once per process): it prints one JSON line and saves its output."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import hig_amd  # noqa: E402
from hig_amd import _lib  # noqa: E402
from oracle import fill  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD32, FWD16, TRAIN16, BWD32, BWD16 = _lib.DN_ENTRY_FWD32, _lib.DN_ENTRY_FWD16, _lib.DN_ENTRY_FWD16_TRAIN, _lib.DN_ENTRY_BWD32, _lib.DN_ENTRY_BWD16
D32 = _lib.DN_FACT_TABLE | _lib.DN_FACT_TEXT_GLOBALS
D16 = D32 | _lib.DN_FACT_KVALL
# (a): 8192 rows in 16 samples -- the smallest batch the split rule takes; head dim 64 with 4 heads -- the fused apply
A = dict(B=16, T=512, F=150, d=256, H=4, L=2, ff=512, N=77, Lt=256, num_frames=512, lengths=(512, 77, 300, 1) * 4, t=(0, 999, 500, 250) * 4)
FORKS = ("text_fork", "split", "fork_emb", "fork_text", "wgrad_fork", "wants_side_stream")


def build(c, **kw):
    m = hig_amd.MotionTransformer(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                  num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"], **kw)
    m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    return m.to(DEV)


def inputs(c):
    return {k: v.to(DEV) for k, v in fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"]).items()}


def forward(m, gi):
    with torch.no_grad():
        return m(gi["x"], gi["t"], length=gi["length"], xf_proj=gi["xf_proj"], xf_out=gi["xf_out"])


def planned(m, c, entry, training=0, xf=0, facts=0, capturing=0):
    """hig_denoiser_plan for this model's dims on the device at hand, with the process's switches."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    wsp32 = int(cus == 256 and os.environ.get("HIG_F32_WSP", "1") != "0")
    return _lib.denoiser_plan(m.dims(c["B"], c["T"], c["N"]), entry, training, xf, facts, capturing, 0, wsp32, None)


def attn_launches():
    L = _lib.lib()
    return [L.hig_attn_path_launches(p) for p in range(_lib.ATTN_NPATHS)]


def gemm_launches():
    L = _lib.lib()
    return [L.hig_gemm_path_launches(p) for p in range(_lib.GEMM_NPATHS)]


def moved(before, after):
    return {p: b - a for p, (a, b) in enumerate(zip(before, after)) if b != a}


def captured_forward(m, gi):
    """The forward under torch.cuda.graph after a warm-up on a side stream: (replayed output, the schedule the captured call ran)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        forward(m, gi)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = forward(m, gi)
        sched = _lib.denoiser_last_schedule()
    g.replay()
    torch.cuda.synchronize()
    return out, sched


def child_main(mode, out_path):
    m = build(A, precision="bf16x3" if mode == "bf16x3" else "f32").eval()
    m.cache_text_context = False
    gi = inputs(A)
    out = forward(m, gi)
    sched = _lib.denoiser_last_schedule()
    plan = planned(m, A, FWD32, xf=1, facts=D32)
    cap_out, cap_sched = captured_forward(m, gi)
    torch.save(out.cpu(), out_path)
    print("SCHEDULE " + json.dumps({"ran": sched, "planned": plan, "captured": cap_sched,
                                    "captured_plan": planned(m, A, FWD32, xf=1, facts=D32, capturing=1),
                                    "captured_vs_eager": float(((cap_out - out).double().norm() / out.double().norm()).item())}))


if __name__ == "__main__":
    child_main(sys.argv[1], sys.argv[2])
    sys.exit(0)


@pytest.fixture(scope="module")
def model_a():
    m = build(A).eval()
    m.cache_text_context = False
    return m, inputs(A)


@pytest.fixture(scope="module")
def out_a(model_a):
    """The per-call fp32 forward of (a), computed once: (output, the schedule it ran, attention launches it made)."""
    m, gi = model_a
    forward(m, gi)                                   # derived operands, workspaces
    before = attn_launches()
    out = forward(m, gi)
    return out.clone(), _lib.denoiser_last_schedule(), moved(before, attn_launches())


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """Both child processes once, side by side: {mode: (schedule record, output)}."""
    from concurrent.futures import ThreadPoolExecutor
    tmp = tmp_path_factory.mktemp("schedule")
    jobs = {"bf16x3": {}, "forked": {"HIG_FWD_SPLIT": "1", "HIG_TEXT_BATCH": "0"}}

    def run(mode):
        path = str(tmp / (mode + ".pt"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, path], env=dict(os.environ, OMP_NUM_THREADS="4", **jobs[mode]),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("SCHEDULE ")][-1]
        return json.loads(line[len("SCHEDULE "):]), torch.load(path)

    with ThreadPoolExecutor(max_workers=2) as pool:
        return dict(zip(jobs, pool.map(run, jobs)))


def test_fp32_per_call_forward_runs_its_plan(model_a, out_a):
    """(a): text batched (one grouped context build), apply fused with the stylization front (2 L launches of the wave kernel, none of
    the unfused apply kernels), LayerNorm folded, nothing forked; the output is the cached-text forward's at the tolerance the
    per-call form has always been held to (tests/test_gpu_trainer_state.py: 2e-6 rel-L2, another rounding order of the text side)."""
    m, gi = model_a
    out, sched, attn = out_a
    plan = planned(m, A, FWD32, xf=1, facts=D32)
    assert sched == plan
    assert {k: v for k, v in sched.items() if v and k != "entry"} == {"text_batched": 1, "fuse_apply": 1, "fold32": 1}
    L = A["L"]
    assert attn.get(_lib.ATTN_PATH_APPLY_STY_WAVE64, 0) == 2 * L
    assert attn.get(_lib.ATTN_PATH_APPLY_WAVE64, 0) == 0 and attn.get(_lib.ATTN_PATH_APPLY_MFMA, 0) == 0 and attn.get(_lib.ATTN_PATH_APPLY, 0) == 0
    # context builds: the layers' self-attention (L launches of the kernel the attention plan names) + ONE grouped build of the text side
    path, split = C.c_int32(), C.c_int32()
    assert _lib.lib().hig_attn_plan(_lib.ATTN_ENTRY_CTX, _lib.ATTN_IO_F32, A["B"], A["T"], 0, A["H"], 64, 1, _lib.ATTN_FACTS_ALL, 0, 1,
                                    C.byref(path), C.byref(split), None) == 0
    ctx = {p: attn.get(p, 0) for p in (_lib.ATTN_PATH_CTX, _lib.ATTN_PATH_CTX_MFMA, _lib.ATTN_PATH_CTX_PART)}
    expect = {_lib.ATTN_PATH_CTX: 0, _lib.ATTN_PATH_CTX_MFMA: 1, _lib.ATTN_PATH_CTX_PART: 0}
    expect[path.value] += L
    assert ctx == expect
    m.cache_text_context = True
    try:
        cached = forward(m, gi)
        cached_sched = _lib.denoiser_last_schedule()
    finally:
        m.cache_text_context = False
    assert cached_sched == planned(m, A, FWD32, xf=0, facts=D32) and cached_sched["text_batched"] == 0
    err = ((out - cached).double().norm() / cached.double().norm()).item()
    print("per-call vs cached text: rel-L2 %.3e" % err)
    assert torch.isfinite(out).all() and err < 2e-6


def test_split_forward_in_a_child_process(out_a, children):
    """(b): with bf16x3 products the split rule's default is on at (a)'s shape: the call reports `split` and computes (a)'s unsplit
    output at the 2e-4 relative level of tests/test_gpu_knobs.py (norms).  With HIG_FWD_SPLIT=1 and HIG_TEXT_BATCH=0 the text side
    is forked because it is not batched, together with the split (two tail scratches); under capture both calls report neither."""
    ref = out_a[0].cpu().double()
    for mode, expect in (("bf16x3", {"text_batched": 1, "text_fork": 0, "split": 1}), ("forked", {"text_batched": 0, "text_fork": 1, "split": 1})):
        rec, out = children[mode]
        assert rec["ran"] == rec["planned"], mode
        assert {k: rec["ran"][k] for k in expect} == expect and rec["ran"]["wants_side_stream"] == 1, mode
        assert rec["captured"] == rec["captured_plan"] and not any(rec["captured"][k] for k in FORKS), mode
        n, n_ref = out.double().norm().item(), ref.norm().item()
        print("%s: |out| %.9e, (a) %.9e, rel-L2 of the difference %.3e, captured vs eager %.3e"
              % (mode, n, n_ref, ((out.double() - ref).norm() / ref.norm()).item(), rec["captured_vs_eager"]))
        assert torch.isfinite(out).all() and abs(n - n_ref) <= 2e-4 * n_ref, mode
        assert rec["captured_vs_eager"] <= 2e-4, mode                # (half batches sum in another order than the captured whole batch)


def test_captured_forward_reports_no_fork_and_replays_the_eager_bits(model_a, out_a):
    """(c): tests/test_gpu_full_size.py claims this at B = 32; here at the small shape with the schedule asserted."""
    m, gi = model_a
    out, sched = captured_forward(m, gi)
    assert sched == planned(m, A, FWD32, xf=1, facts=D32, capturing=1)
    assert not any(sched[k] for k in FORKS)
    assert torch.equal(out, out_a[0])


def test_bf16_forward_runs_its_plan():
    """(d): d = 512, 8 heads: every stylization block is one launch (fuse_out), so a layer launches 4 bf16 GEMMs instead of 7; the
    embedding chain and the output projection are 4 more, the batched text side one, and joint_embed runs its own kernel (no fp32 GEMM)."""
    c = dict(B=4, T=64, F=150, d=512, H=8, L=2, ff=1024, N=77, Lt=256, num_frames=64, lengths=(64, 17, 33, 1), t=(0, 999, 500, 250))
    m = build(c, storage="bf16").eval()
    m.cache_text_context = False
    gi = inputs(c)
    forward(m, gi)
    before = gemm_launches()
    out = forward(m, gi)
    gemms = moved(before, gemm_launches())
    sched = _lib.denoiser_last_schedule()
    plan = planned(m, c, FWD16, xf=1, facts=D16)
    assert sched == plan
    assert {k: v for k, v in sched.items() if v and k != "entry"} == dict.fromkeys(("text_batched", "ctx_mm16", "joint16", "fuse_apply", "fuse_mm16", "fuse_out"), 1)
    bf16 = sum(gemms.get(p, 0) for p in (_lib.GEMM_PATH_WSP16, _lib.GEMM_PATH_WS16, _lib.GEMM_PATH_FEWROW16, _lib.GEMM_PATH_TILED16))
    fp32 = sum(gemms.get(p, 0) for p in (_lib.GEMM_PATH_TILED32, _lib.GEMM_PATH_WSP32, _lib.GEMM_PATH_TAIL32, _lib.GEMM_PATH_SPLIT32))
    L = c["L"]
    assert bf16 == 4 + (1 if plan["text_batched"] else L) + L * (7 - 3 * plan["fuse_out"]), gemms
    assert fp32 == (0 if plan["joint16"] else 1), gemms
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_training_step_runs_its_plan(storage):
    """(e): the weight gradients of the fp32 backward go to the second stream when launched eagerly; bf16 storage keeps them on the
    caller's.  (The model's own launchers, called on this thread: the schedule record is per thread, autograd's is another.)"""
    c = dict(B=2, T=64, F=150, d=256, H=4, L=1, ff=512, N=77, Lt=256, num_frames=64, lengths=(64, 17), t=(3, 987))
    m = build(c, storage=storage).train()
    gi = inputs(c)
    bf = storage == "bf16"
    out, saved = m._launch_forward(gi["x"], gi["t"], gi["length"], gi["xf_proj"], gi["xf_out"], training=True)
    fwd = _lib.denoiser_last_schedule()
    assert fwd == planned(m, c, TRAIN16 if bf else FWD32, training=1)
    assert {k: v for k, v in fwd.items() if v and k != "entry"} == ({"fuse_front": 1, "ctx_mm16": 1} if bf else {})
    dx, dxp, dxo = m._launch_backward(gi["x"], gi["t"], gi["length"], gi["xf_out"], saved, torch.ones_like(out), want_dx=True)
    bwd = _lib.denoiser_last_schedule()
    torch.cuda.synchronize()
    assert bwd == planned(m, c, BWD16 if bf else BWD32, training=1)
    assert (bwd["wgrad_fork"], bwd["wants_side_stream"]) == ((0, 0) if bf else (1, 1))
    assert all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in (dx, dxp, dxo))
