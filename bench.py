#!/usr/bin/env python3
"""Benchmark of the hot path (BASELINE.json) on N MI355X GPUs of one node.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5 --full   (+ roofline, cpu_baseline and every extra)
    python bench.py --gpus N --steps K --warmup W          (spawns its own N ranks, one per GPU; or, equivalently:)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

N = 1 -- headline = denoiser-forward frames/s at BASELINE config 2 (B=64, T=196, d=512, L=8, F=150, ff=1024,
fp32): one "step" = one full MotionTransformer forward on (x_t, t, text_emb) resident in HBM, INCLUDING the
cross-attention text side (key/value projections + context of all layers) that the reference computes on every
call (transformer.py:144-150); the variant with that step-invariant work hoisted (what the sampling loop does) is
reported in `extra`.
N > 1 -- headline = data-parallel TRAINING step frames/s (BASELINE config 4: B=64 per GPU, q_sample + forward +
masked MSE + backward + RCCL all-reduce of the flat gradient over xGMI + clip + Adam), weak scaling; the forward
(no collective) goes to `extra`.

Synthetic data (x_t, t, length, xf_proj, xf_out ~ seed 0; zero-init parameters overwritten with N(0, 0.02) so no
work is skipped).  Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps of the headline and
prints the line (`ms_per_step` = milliseconds of one timed step); `--dump-outputs DIR` also writes what the last timed
step computed (N = 1: the forward's output; N > 1: rank 0's loss and a seeded sample of the updated parameters) as
DIR/<name>.npy.  Everything else below runs only with `--full`.  Beside the headline: `roofline` for the dominant kernel class
(the fp32 FFN GEMM), `cpu_baseline` = the oracle (CPU restatement of the reference, pinned by tests/golden) timed
on the host cores, and in `extra` the train step, the REAL 1000-step hipGraph DDPM sampling loop (fp32 products and
bf16 storage), the bf16-storage forwards, the HBM-bound kernels, the two-person model, text head and evaluator.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CFG = dict(B=64, T=196, F=150, d=512, H=8, L=8, ff=1024, N=77, Lt=256)
FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense, spec


def flops_per_frame_fwd(c):
    """SURVEY 8d algorithmic FLOPs per frame of one forward."""
    d, ff, F, L, T, N, Lt, hd = c["d"], c["ff"], c["F"], c["L"], c["T"], c["N"], c["Lt"], c["d"] // c["H"]
    E = 4 * d
    per_tok = 4 * F * d + L * (14 * d * d + 4 * d * ff + 6 * hd * d)
    per_sample = L * (4 * N * Lt * d + 2 * N * hd * d + 12 * E * d) + 2 * (d * E + E * E)
    return per_tok + per_sample / T


def build_model(c, device, no_eff=False):
    import hig_amd
    torch.manual_seed(0)
    m = hig_amd.MotionTransformer(input_feats=c["F"], num_frames=c["T"], latent_dim=c["d"], ff_size=c["ff"],
                                  num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"], no_eff=no_eff)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith("out.") or ".ffn.linear2." in name or ".out_layers.2." in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)  # un-zero the zero_module tensors
    return m.to(device)


def make_inputs(c, device, rank):
    g = torch.Generator().manual_seed(1000 + rank)
    B, T = c["B"], c["T"]
    return dict(
        x=torch.randn(B, T, c["F"], generator=g).to(device),
        t=torch.randint(0, 1000, (B,), generator=g).to(device),
        length=torch.full((B,), T, dtype=torch.int64).to(device),
        xf_proj=torch.randn(B, 4 * c["d"], generator=g).to(device),
        xf_out=torch.randn(B, c["N"], c["Lt"], generator=g).to(device),
        x0=torch.randn(B, T, c["F"], generator=g).to(device),
    )


def timed(fn, steps, warmup, world):
    """W untimed + exactly K timed steps, barrier + synchronize on both sides, MAX over ranks."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([el], device="cuda", dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        el = tt.item()
    return el


def rocprof_kernel_avg_us():
    """Average duration of the FFN linear1 launches of THIS microbenchmark in the committed rocprofv3 kernel trace of the
    same command (profiles/r*_ffn_gemm_trace.json, written by tools/summarize_profiles.py from the launches between the two
    hig_marker_kernel marks) -- the profile-side number the live `avg_launch_ms` must agree with; None if no profile is there."""
    import glob
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r*_ffn_gemm_trace.json")))
    if not files:
        return None
    try:
        d = json.load(open(files[-1]))
        return {"avg_us": d["avg_us"], "launches": d["launches"], "source": "profiles/" + os.path.basename(files[-1])}
    except Exception:   # noqa: BLE001
        return None


def ffn_gemm_roofline(c, device, reps=32):
    """Dominant kernel class: the FFN linear1 GEMM (M=B*T, K=d, N=ff) with its bias+GELU epilogue, launched
    through the same C-ABI entry the forward uses and timed with HIP events on torch's stream (= the launch stream).
    Launches rotate through 8 activation / output buffer pairs (8 x 77 MB = 617 MB > the 256 MiB Infinity Cache), so
    like inside the forward the activation operand comes from HBM, not from a cache left hot by the previous launch."""
    from hig_amd import _lib
    M, K, Nn = c["B"] * c["T"], c["d"], c["ff"]
    NB = 8
    Xs = [torch.randn(M, K, device=device) for _ in range(NB)]
    outs = [torch.empty(M, Nn, device=device) for _ in range(NB)]
    W = torch.randn(Nn, K, device=device) * 0.05
    b = torch.randn(Nn, device=device)
    descs = []
    for X, out in zip(Xs, outs):
        d = _lib.GemmDesc()
        d.X, d.ldx, d.x_rs, d.Y, d.ldy, d.y_rs = X.data_ptr(), K, 0, W.data_ptr(), K, 0
        d.C, d.ldc, d.I, d.J, d.R = out.data_ptr(), Nn, M, Nn, K
        d.xf, d.epi, d.prec, d.bias = _lib.XF_NONE, _lib.EPI_BIAS_GELU, _lib.PREC_F32, b.data_ptr()
        descs.append(d)
    L = _lib.lib()
    # the split-tail scratch hig_denoiser_fwd hands its GEMMs (hig_gemm_ws): same kernel, same tile schedule as in the forward
    tail = torch.zeros(L.hig_gemm_tail_ws_bytes(), dtype=torch.uint8, device=device)
    # warm-up: 25 rounds over the operand sets (~25 ms).  A process that comes here from host-side work finds the chip's memory side
    # idle: the first ~100 launches of a fresh process run 10-15 % slower than the steady state (tools/ffn_gemm_pmc.py warm: 120-124 us
    # by kernel trace for the first 20 launches, 105 us for launches 300-400, at an unchanged shader clock)
    for i in range(25 * NB):
        _lib.check(L.hig_gemm_ws(C.byref(descs[i % NB]), tail.data_ptr(), tail.numel(), _lib.stream_ptr()))
    # 5 batches of `reps` launches, each bracketed by HIP events; the MEDIAN batch average is reported (one batch right
    # after the heavy training-step section read 7 % slow on some boxes while the in-situ rocprofv3 average of the same
    # kernel stayed at 0.122 ms: clock / thermal state, not the kernel)
    batch_ms = []
    _lib.check(L.hig_debug_marker(1, _lib.stream_ptr()))   # named marks in a rocprofv3 kernel trace: the launches between
    for _ in range(5):                                      # marker 1 and marker 2 are this microbenchmark's
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(reps):
            _lib.check(L.hig_gemm_ws(C.byref(descs[i % NB]), tail.data_ptr(), tail.numel(), _lib.stream_ptr()))
        e1.record()
        torch.cuda.synchronize()
        batch_ms.append(e0.elapsed_time(e1) / reps)
    _lib.check(L.hig_debug_marker(2, _lib.stream_ptr()))
    ms = sorted(batch_ms)[2]
    flops = 2.0 * M * K * Nn
    ach = flops / (ms * 1e-3) / 1e12
    traffic, src = pmc_traffic_bytes()
    return {"bound": "mfma",
            "kernel": "gemm_wsp32_kernel<KW=512,EPI_BIAS_GELU> (FFN linear1: M=%d K=%d N=%d; weight-stationary, 16 column panels x "
                      "16 row groups of 49 tiles of 16 rows on the 256 CUs, as in the forward; HIG_F32_WSP=0: the tiled "
                      "gemm_f32_kernel<64,64,...> of rounds 1-5)" % (M, K, Nn),
            "achieved": round(ach, 2), "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach / FP32_MFMA_PEAK_TFLOPS, 4), "traffic": traffic, "traffic_source": src,
            "flops_per_launch": flops, "avg_launch_ms": round(ms, 4), "kernel_avg_us_rocprof": rocprof_kernel_avg_us(),
            "batch_avg_launch_ms": [round(v, 4) for v in batch_ms],
            "how": "median of 5 batches of %d launches rotating over %d operand sets (HBM-resident activations) after 200 warm-up "
                   "launches, HIP events on the launch stream" % (reps, NB)}


def ffn_gemm_bf16_roofline(c, device, reps=32):
    """The same FFN linear1 shape on the bf16-storage GEMM (hig_gemm_bf16: bf16 operands DMA-ed into LDS,
    v_mfma_f32_32x32x16_bf16, bias + GELU + bf16 store), against the dense bf16 MFMA peak (2.5 PFLOP/s)."""
    from hig_amd import _lib
    M, K, Nn = c["B"] * c["T"], c["d"], c["ff"]
    NB = 12
    Xs = [torch.randn(M, K, device=device).to(torch.bfloat16) for _ in range(NB)]
    outs = [torch.empty(M, Nn, device=device, dtype=torch.bfloat16) for _ in range(NB)]
    W = (torch.randn(Nn, K, device=device) * 0.05).to(torch.bfloat16)
    b = torch.randn(Nn, device=device)
    descs = []
    for X, out in zip(Xs, outs):
        d = _lib.Gemm16Desc()
        d.X, d.ldx, d.Y, d.ldy, d.C, d.ldc, d.c_f32 = X.data_ptr(), K, W.data_ptr(), K, out.data_ptr(), Nn, 0
        d.I, d.J, d.R, d.epi, d.bias = M, Nn, K, _lib.EPI_BIAS_GELU, b.data_ptr()
        descs.append(d)
    L = _lib.lib()
    for i in range(NB):
        _lib.check(L.hig_gemm_bf16(C.byref(descs[i]), _lib.stream_ptr()))
    # median of 5 batches, a sync and a short sleep ahead of the first: a host stall inside ONE timed region (this runs right
    # behind the CPU-oracle legs) must not become the recorded figure
    torch.cuda.synchronize()
    time.sleep(0.05)
    batch_ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(reps):
            _lib.check(L.hig_gemm_bf16(C.byref(descs[i % NB]), _lib.stream_ptr()))
        e1.record()
        torch.cuda.synchronize()
        batch_ms.append(e0.elapsed_time(e1) / reps)
    ms = sorted(batch_ms)[2]
    flops = 2.0 * M * K * Nn
    ach = flops / (ms * 1e-3) / 1e12
    by = (M * K + Nn * K + M * Nn) * 2
    return {"bound": "mfma (nominal).  Measured (profiles/r05_notes.md sections 2, 7 and 9: s_memtime stamps, tools/coissue_probe.hip, "
                     "lds_read_probe.hip, a K-split variant with twice the waves that did NOT get faster): a 32 x 128 tile costs "
                     "~2.2 K cycles against 1.0 K of MFMA issue -- per tile the four service waves spend ~780 cycles issuing the "
                     "eight LDS-DMA instructions of the next X tile (the CU's fetch path takes ~11 B/clk per wave) and ~1.5 K on the "
                     "GELU epilogue, in order; without an epilogue the tile sits at ~1.4 K cycles on the CU's LDS pipe",
            "kernel": "gemm_wsp16_kernel<EPI_BIAS_GELU> (weight-stationary, specialised matrix / service waves; FFN linear1, bf16 "
                      "storage: M=%d K=%d N=%d, bias+GELU)" % (M, K, Nn),
            "achieved": round(ach, 1), "peak": 2500.0, "unit": "TFLOP/s", "frac": round(ach / 2500.0, 4),
            "avg_launch_ms": round(ms, 4), "batch_avg_launch_ms": [round(v, 4) for v in batch_ms],
            "algorithmic_GB_per_s": round(by / ms / 1e6, 0),
            "how": "median of 5 batches of %d launches rotating over %d operand sets (%.0f MB > Infinity Cache), HIP events" %
                   (reps, NB, NB * by / 1e6)}


def hbm_kernel_rooflines(c, device, reps=30):
    """HBM-bound kernels of the path through the C ABI: achieved GB/s = algorithmic bytes (each operand read or
    written once) / launch time measured with HIP events on the launch stream; peak 8 TB/s."""
    from hig_amd import _lib
    L, s = _lib.lib(), _lib.stream_ptr()
    B, T, H, d = c["B"], c["T"], c["H"], c["d"]
    hd, M = d // H, c["B"] * c["T"]
    P = lambda t: t.data_ptr()
    qkv = torch.randn(M, 3 * d, device=device)
    y, a = torch.empty(M, d, device=device), torch.empty(M, d, device=device)
    dy = torch.randn(M, d, device=device)
    A = torch.randn(B, H, hd, hd, device=device) * 0.1
    kst, st = torch.zeros(B, d, 2, device=device), torch.empty(M, 2, device=device)
    scr = torch.zeros(L.hig_linattn_ctx_scratch_floats(B, T, H, hd), device=device)
    bscr = torch.zeros(L.hig_linattn_bwd_scratch_floats(B, T, H, hd), device=device)
    dqkv, dA = torch.empty_like(qkv), torch.empty_like(A)
    lg = torch.full((B,), T, dtype=torch.int64, device=device)
    g, be = torch.ones(d, device=device), torch.zeros(d, device=device)
    ss = torch.randn(B, 2 * d, device=device) * 0.1
    stream_mb = M * d * 4 / 1e6
    cases = {
        "linattn_ctx (k^T v)": (2 * stream_mb, lambda: L.hig_linattn_ctx(P(qkv) + 4 * d, P(qkv) + 8 * d, 3 * d, B, T, H, hd, P(lg), P(A), P(kst), P(scr), s)),
        "linattn_apply (q A)": (2 * stream_mb, lambda: L.hig_linattn_apply(P(qkv), 3 * d, P(A), P(y), d, B, T, H, hd, s)),
        "linattn_apply_bwd": (3 * stream_mb, lambda: L.hig_linattn_apply_bwd(P(dy), d, P(qkv), 3 * d, P(A), P(dqkv), 3 * d, P(dA), B, T, H, hd, P(bscr), s)),
        "linattn_ctx_bwd": (4 * stream_mb, lambda: L.hig_linattn_ctx_bwd(P(dA), P(A), P(qkv) + 4 * d, P(qkv) + 8 * d, 3 * d, P(kst), P(lg), P(dqkv) + 4 * d, P(dqkv) + 8 * d, 3 * d, B, T, H, hd, P(bscr), s)),
        "ln_mod_silu (stylization front)": (2 * stream_mb, lambda: L.hig_ln_mod_silu(P(y), d, M, d, P(g), P(be), P(ss), 2 * d, d, T, P(a), d, P(st), s)),
        "layernorm": (2 * stream_mb, lambda: L.hig_layernorm(P(y), d, M, d, P(g), P(be), P(a), d, P(st), s)),
    }
    out = {}
    torch.cuda.synchronize()
    time.sleep(0.05)               # (this runs right behind the CPU-oracle legs: let the host settle before the first case)
    for name, (mb, fn) in cases.items():
        for _ in range(3):
            _lib.check(fn())
        batch_us = []
        for _ in range(5):         # median of 5 batches: one host stall inside a timed region must not become the figure
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                _lib.check(fn())
            e1.record()
            torch.cuda.synchronize()
            batch_us.append(e0.elapsed_time(e1) / reps * 1e3)
        us = sorted(batch_us)[2]
        out[name] = {"us": round(us, 1), "algorithmic_MB": round(mb, 1), "GB_per_s": round(mb / us * 1e3, 0),
                     "frac_of_8TB_s": round(mb / us * 1e3 / 8000.0, 3), "batch_us": [round(v, 1) for v in batch_us]}
    return out


def pmc_traffic_bytes():
    """(HBM bytes per launch of the FFN GEMM, where the figure comes from).  PMC counters cannot be read from inside
    the timed process, so this is NOT a measurement of this run: it is the figure of the committed rocprofv3 PMC
    passes of the same kernel and shape ((2 x FETCH_SIZE + WRITE_SIZE) x 1024 per the guide's gfx950 correction,
    tools/ffn_gemm_pmc.py -> profiles/rNN_ffn_gemm_pmc.json); (None, None) when no profile has been committed."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_ffn_gemm_pmc.json")))
    if not files:
        return None, None
    try:
        return (json.load(open(files[-1])).get("traffic_bytes"),
                "committed rocprofv3 --pmc passes of this kernel (%s), not collected in this run" %
                os.path.relpath(files[-1], ROOT))
    except Exception:
        return None, None


def cpu_baseline(c, model, inp, gpu_out):
    """The oracle (oracle/denoiser_ref.py + oracle/diffusion_ref.py == reference arithmetic, pinned by tests/golden)
    on the host cores, same batch as the GPU step -- the three legs BASELINE.md section 3 names:
      value           forward frames/s at B=64, T=196 (median of 3 after a warm-up);
      legs.fwd_bwd    forward + masked-MSE + backward through torch autograd, frames/s (median of 3);
      legs.p_sample   5 `p_sample` steps (denoiser forward + DDPM update) at B=32, extrapolated x200 to the 1000-step
                      loop (stated as extrapolated: the full CPU loop takes minutes).
    Thread count: torch's intra-op pool oversubscribes badly on many-core hosts (256 threads: 69 s per forward), so
    probe 8, 16, 32, ... threads with one forward each while it keeps getting faster and use the best setting."""
    from oracle import denoiser_ref as R
    from oracle import diffusion_ref as D
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    p = {k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith("clip.")}
    ci = {k: v.cpu() for k, v in inp.items()}

    def one():
        t0 = time.perf_counter()
        with torch.no_grad():
            r = R.denoiser_forward(p, ci["x"], ci["t"], ci["length"], ci["xf_proj"], ci["xf_out"], c["H"], c["L"])
        return time.perf_counter() - t0, r

    best_n, best_t, n = None, None, min(8, avail)
    while True:
        torch.set_num_threads(n)
        one()                      # warm-up at this setting
        tt, _ = one()
        if best_t is None or tt < best_t:
            best_n, best_t = n, tt
        if tt > 1.15 * best_t or n * 2 > avail or n >= 64:
            break
        n *= 2
    torch.set_num_threads(best_n)
    times, ref = [], None
    for _ in range(3):
        tt, ref = one()
        times.append(tt)
    med = statistics.median(times)
    rel = ((gpu_out.double().cpu() - ref.double()).norm() / ref.double().norm()).item()
    legs = {}
    # ---- forward + backward (training arithmetic: masked MSE against the noise, all core parameter gradients) ----
    core_names = [k for k in p if not (k.startswith("text") or k.startswith("clip"))]
    pg = {k: (v.clone().requires_grad_(True) if k in core_names else v) for k, v in p.items()}
    mask = R.src_mask(c["T"], ci["length"])

    def fwd_bwd():
        t0 = time.perf_counter()
        pred = R.denoiser_forward(pg, ci["x"], ci["t"], ci["length"], ci["xf_proj"], ci["xf_out"], c["H"], c["L"])
        D.masked_mse(pred, ci["x0"], mask).backward()
        for k in core_names:
            pg[k].grad = None
        return time.perf_counter() - t0

    fwd_bwd()
    fb = statistics.median([fwd_bwd() for _ in range(3)])
    legs["fwd_bwd"] = {"value": round(c["B"] * c["T"] / fb, 1), "unit": "frames/s",
                       "sample": "3 timed forward+loss+backward passes of the full batch (median %.0f ms)" % (fb * 1e3)}
    del pg
    # ---- DDPM sampling: 5 p_sample steps at B = 32, extrapolated to the 1000-step loop ----
    Bs = 32
    tb = D.tables(D.linear_betas(1000))
    xs = ci["x"][:Bs].clone()
    kw = (ci["length"][:Bs], ci["xf_proj"][:Bs], ci["xf_out"][:Bs])
    g = torch.Generator().manual_seed(3)

    def p_step(i):
        nonlocal xs
        t0 = time.perf_counter()
        tt_ = torch.full((Bs,), 999 - i, dtype=torch.int64)
        with torch.no_grad():
            eps = R.denoiser_forward(p, xs, tt_, kw[0], kw[1], kw[2], c["H"], c["L"])
            xs = D.p_step(tb, xs, tt_, eps, torch.randn(xs.shape, generator=g))[0]
        return time.perf_counter() - t0

    p_step(0)
    ps = statistics.median([p_step(i + 1) for i in range(5)])
    legs["p_sample"] = {"value": round(Bs / (ps * 1000.0), 4), "unit": "samples/s (1000-step loop)",
                        "sample": "5 timed p_sample steps at B=%d (median %.0f ms/step), EXTRAPOLATED x1000 steps"
                                  % (Bs, ps * 1e3)}
    return {"value": round(c["B"] * c["T"] / med, 1), "unit": "frames/s", "cores": best_n, "kind": "port",
            "sample": "3 timed forwards of the full B=%d x T=%d batch (median %.0f ms), fp32 torch CPU oracle, "
                      "%d threads (best of a doubling probe; host exposes %d)" % (c["B"], c["T"], med * 1e3, best_n, avail),
            "legs": legs}, rel


def oracle_slice_error(c, model, inp, gpu_out, n=2):
    """rel-L2 of the first `n` samples of a GPU forward against the CPU oracle run on just those samples (samples are
    independent, so the slice of the full-batch output is comparable): pins the bf16 numbers of this file to the
    reference's arithmetic rather than to the fp32 GPU path."""
    from oracle import denoiser_ref as R
    p = {k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith("clip.")}
    ci = {k: v[:n].cpu() for k, v in inp.items() if k in ("x", "t", "length", "xf_proj", "xf_out")}
    # (host hygiene: with the default pool -- one thread per core of a 128-256-thread host -- the OpenMP workers keep spinning
    # for a while after the oracle returns, and on some boxes the launching thread of the NEXT timed GPU region then loses its
    # core: an eager forward of ~150 launches measured 10 ms instead of 3.3.  A small pool and a pause keep the checker out
    # of the measurement.)
    nthr = torch.get_num_threads()
    torch.set_num_threads(min(nthr, 16))
    try:
        with torch.no_grad():
            ref = R.denoiser_forward(p, ci["x"], ci["t"], ci["length"], ci["xf_proj"], ci["xf_out"], c["H"], c["L"])
    finally:
        torch.set_num_threads(nthr)
    time.sleep(0.3)
    return ((gpu_out[:n].double().cpu() - ref.double()).norm() / ref.double().norm()).item()


SAMPLING_MODES = ("f32", "bf16", "bf16s")
MODE_TEXT = {"f32": "exact fp32 products, fp32 storage", "bf16": "bf16 products, fp32 storage",
             "bf16s": "bf16 STORAGE (bf16 activations + bf16 weight shadow, fp32 accumulate / statistics)"}


def set_mode(model, mode):
    """'f32' / 'bf16x3' / 'bf16' = product arithmetic with fp32 storage; 'bf16s' = bf16 storage."""
    model.precision = "bf16" if mode == "bf16s" else mode
    if hasattr(model, "storage"):
        model.storage = "bf16" if mode == "bf16s" else "f32"


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks as fresh child processes -- as the reference's launcher
    spawns its own (tools/train.py:92-102, mp.spawn) -- BEFORE this process has made any GPU call (it never does: no HIP call,
    no exec from a process that initialised the GPU), relay rank 0's JSON line, exit non-zero if any rank failed.  One rank per
    GPU over RCCL; with fewer GPUs than ranks (a 1-GPU box: self-test only) the ranks share devices over gloo."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ndev = torch.cuda.device_count()          # (counting devices does not initialise the GPU)
    env = dict(os.environ, WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if ndev < n:
        env.setdefault("HIG_DIST_BACKEND", "gloo")
    procs = []
    for r in range(n):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=e,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    import threading
    chunks, bad = [], None
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)   # (drains rank 0's pipe while it runs)
    reader.start()
    try:
        while any(p.poll() is None for p in procs):
            bad = next(((r, p.returncode) for r, p in enumerate(procs) if p.poll() not in (None, 0)), None)
            if bad is not None:
                break
            time.sleep(0.2)
    finally:
        for p in procs:                                       # a rank died: its peers would wait in a collective for ever
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    reader.join(timeout=10)
    out = b"".join(c for c in chunks if c)
    sys.stdout.write(out.decode(errors="replace"))
    sys.stdout.flush()
    if bad is None:
        bad = next(((r, p.returncode) for r, p in enumerate(procs) if p.returncode != 0), None)
    if bad is not None:
        sys.exit("bench.py: rank %d exited with code %s" % bad)
    sys.exit(0)


SHAPE_TXT = ("B=%d/GPU T=196 F=150 d=512 L=8 H=8 ff=1024 N=77 Lt=256, linear attention, text embeddings "
             "supplied (CLIP stubbed)")
DUMP_LIMIT_BYTES = 64 << 20


def common_fields(a, world):
    return {"n_gpus": world, "steps": a.steps, "warmup": a.warmup, "higher_is_better": True,
            "scaling": "strong" if a.strong else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic"}


def headline_config(B):
    return {"workload": "MotionTransformer forward incl. the per-call cross-attention text side, BASELINE "
                        "config 2: " + SHAPE_TXT % B, "parallelism": "dp1"}


def dump_outputs(outdir, arrays):
    """`--dump-outputs DIR`: each tensor as DIR/<name>.npy in float32 (float64 tensors stay float64), so that two builds
    run with the same arguments -- same seeded inputs and parameters -- can be compared output for output."""
    import numpy as np
    host = {k: v.detach().cpu() for k, v in arrays.items()}
    host = {k: (v if v.dtype == torch.float64 else v.float()).numpy() for k, v in host.items()}
    total = sum(v.nbytes for v in host.values())
    if total > DUMP_LIMIT_BYTES:
        raise RuntimeError("--dump-outputs: %d bytes exceed the %d-byte limit" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(outdir, exist_ok=True)
    for k, v in host.items():
        np.save(os.path.join(outdir, k + ".npy"), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra", action="store_true")
    ap.add_argument("--ddpm-steps", type=int, default=1000, help="diffusion steps of the sampling loop (the real loop: 1000)")
    ap.add_argument("--strong", action="store_true",
                    help="strong scaling (SURVEY 8d config 4): global batch 512 split over the ranks instead of 64 per rank")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, run everything else this file measures: roofline, CPU baseline, extras "
                         "(other precisions, shapes, models), and at N > 1 the forward and the single-GPU reference")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (rank 0)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus > 1 and "RANK" not in os.environ:
        spawn_ranks(a.gpus)                   # (does not return)
    ndev = torch.cuda.device_count()
    local = local % max(ndev, 1)   # (several ranks may share a GPU only in the gloo self-test below)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("TORCH_NCCL_CUDA_EVENT_CACHE", "0")   # (collectives are captured into the step's graph: parallel.py)
        backend = os.environ.get("HIG_DIST_BACKEND", "nccl")  # "nccl" == RCCL over xGMI; gloo: 1-GPU self-test
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)

    import hig_amd
    from hig_amd.parallel import broadcast_parameters
    c = dict(CFG)
    if a.strong:
        assert 512 % world == 0, "--strong splits a global batch of 512"
        c["B"] = 512 // world
    model = build_model(c, device).eval()
    broadcast_parameters(model)
    inp = make_inputs(c, device, rank)
    B, T = c["B"], c["T"]

    def fwd():
        with torch.no_grad():
            return model(inp["x"], inp["t"], length=inp["length"], xf_proj=inp["xf_proj"], xf_out=inp["xf_out"])

    # One forward = everything the reference computes per call, including the cross-attention text side
    # (transformer.py:144-150): the text-context cache (a product feature for the sampling loop) is OFF here.
    model.cache_text_context = False
    gflop = flops_per_frame_fwd(c) * B * T / 1e9          # executed == algorithmic: nothing is hoisted
    fwd_res = None
    if world == 1 or a.full:                  # (N > 1 headlines the training step: the forward is an extra there)
        last = {}

        def fwd_step():
            last["out"] = fwd()

        el = timed(fwd_step, a.steps, a.warmup, world)
        fwd_res = {"frames_per_s": round(B * T * a.steps * world / el, 1), "ms_per_step": round(el / a.steps * 1e3, 4),
                   "fwd_tflops": round(gflop * a.steps * world / el / 1e3, 2)}
        if world == 1 and a.dump_outputs:
            dump_outputs(a.dump_outputs, {"denoiser_out": last["out"]})
        del last
    if world == 1 and not a.full:
        # a plain run: the headline and nothing else
        res = dict({"metric": "denoiser-fwd frames/s @ B=64·T=196", "value": fwd_res["frames_per_s"],
                    "unit": "frames/s", "ms_per_step": fwd_res["ms_per_step"]}, **common_fields(a, world))
        res["config"] = headline_config(B)
        res["fwd_tflops"] = fwd_res["fwd_tflops"]
        print(json.dumps(res))
        return

    # ---- training step: q_sample + fwd + masked MSE + bwd (+ RCCL all-reduce) + clip + Adam ----
    import types
    args = types.SimpleNamespace(device=device, diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=B,
                                 num_epochs=1, log_every=50, save_latest=500, save_every_e=5,
                                 is_continue=False, model_dir="/tmp")
    trainer = hig_amd.DDPMTrainer(args, model.train())
    trainer.sync_replicas()
    noise = torch.randn_like(inp["x0"])

    def train_step_eager():
        trainer.train_step_fused(inp["x0"], inp["t"], inp["length"], inp["xf_proj"], inp["xf_out"], noise=noise)

    def train_step_graph():
        trainer.train_step_captured(inp["x0"], inp["t"], inp["length"], inp["xf_proj"], inp["xf_out"], noise=noise)

    def train_step_graph_split():
        trainer.opt.capture_exchange = False
        train_step_graph()

    def train_step_graph_overlapped():
        trainer.opt.capture_exchange = True
        train_step_graph()

    train_step, step_form, form_probe = train_step_eager, "eager launches, per-layer all-reduces overlapped with the backward", None
    if world > 1:
        # Three forms of the same data-parallel step: (a) eager launches with the gradient exchange issued layer by layer from
        # inside the backward (RCCL on a side stream); (b) hipGraph A (fwd + bwd) | ONE flat all-reduce | hipGraph B (clip +
        # Adam); (c) ONE hipGraph holding the step AND the per-layer all-reduces of (a) -- the overlap without the host cost
        # (RCCL at world 1, profiles/r05_rccl_world1_probe.json: (a) pays +1.0 ms of host time for the 18 collectives, (c)
        # +0.04 ms).  All are timed during warm-up (3 steps each, max over ranks) and the fastest one is the step the K timed
        # steps run; (c) is probed last, and a refused capture leaves the choice between (a) and (b).
        forms = [(train_step_eager, step_form, "eager_overlapped_ms"),
                 (train_step_graph_split, "hipGraph A (fwd+bwd) | one flat RCCL all-reduce | hipGraph B (clip+Adam)", "graphs_flat_allreduce_ms"),
                 (train_step_graph_overlapped, "one hipGraph: fwd + bwd with the per-layer RCCL all-reduces captured beside it + clip + Adam",
                  "one_graph_overlapped_ms")]
        probe = []
        for fn, _, _ in forms:
            try:
                probe.append(timed(fn, 3, 2, world))
            except Exception as e:       # noqa: BLE001  (reported in the line; every rank fails alike or the max below is inf)
                probe.append(float("inf"))
                print("bench: step form refused on rank %d: %s" % (rank, e), file=sys.stderr)
        if trainer.fused_state().get("captured_form") != "one graph, exchange inside":
            probe[2] = float("inf")            # (the trainer fell back to the split form -- on every rank alike, parallel.all_ranks_agree)
        pick = torch.tensor(probe, device=device, dtype=torch.float64)
        dist.all_reduce(pick, op=dist.ReduceOp.MAX)      # (every rank sees the same vector, so every rank picks the same form)
        form_probe = {k: (round(pick[j].item() / 3 * 1e3, 3) if pick[j].item() != float("inf") else None)
                      for j, (_, _, k) in enumerate(forms)}
        best = int(torch.argmin(pick).item())
        train_step, step_form = forms[best][0], forms[best][1]
        trainer.sync_replicas()

    def train_what(mode):
        return ("q_sample+fwd+masked-MSE+bwd+%sclip(0.5)+Adam, B=%d/GPU, %s GEMM products, fp32 accumulate/storage/"
                "optimizer" % ("RCCL all-reduce(%.0f MB)+" % (model.flat_params().core_numel * 4 / 1e6)
                               if world > 1 else "", B, mode))

    train_res = None
    if world > 1 or not a.no_extra:
        ksteps = a.steps if world > 1 else max(3, min(a.steps, 10))
        el_t = timed(train_step, ksteps, max(2, a.warmup if world > 1 else 2), world)
        train_res = {"frames_per_s": round(B * T * ksteps * world / el_t, 1),
                     "ms_per_step": round(el_t / ksteps * 1e3, 4), "steps": ksteps, "what": train_what("f32"),
                     "step_form": step_form}
        if form_probe:
            train_res["step_form_probe"] = form_probe
        if world > 1 and rank == 0 and a.dump_outputs:
            # what the caller of the timed step holds after it: the loss and the updated parameters (a seeded sample)
            flat = model.flat_params()
            idx = torch.randperm(flat.core_numel, generator=torch.Generator().manual_seed(0))[:1 << 20].to(device)
            dump_outputs(a.dump_outputs, {"train_loss": trainer.fused_state()["loss"],
                                          "params_sample": flat.flat[:flat.core_numel][idx]})
    model.eval()

    common = common_fields(a, world)
    shape_txt = SHAPE_TXT % B
    if world == 1:
        res = dict({"metric": "denoiser-fwd frames/s @ B=64·T=196", "value": fwd_res["frames_per_s"],
                    "unit": "frames/s", "ms_per_step": fwd_res["ms_per_step"]}, **common)
        res["config"] = headline_config(B)
        res["fwd_tflops"] = fwd_res["fwd_tflops"]
    else:
        # BASELINE config 4: data-parallel training, weak scaling (B=64 per GPU; --strong: global 512 split)
        res = dict({"metric": "DP train-step frames/s @ %s·T=196 (1→8 GPU scaling)" %
                              ("global B=512" if a.strong else "B=64/GPU"),
                    "value": train_res["frames_per_s"], "unit": "frames/s", "ms_per_step": train_res["ms_per_step"]},
                   **common)
        res["config"] = {"workload": "DDPM training step (q_sample + denoiser fwd + masked MSE + bwd + RCCL all-reduce "
                                     "of the flat gradient + clip 0.5 + Adam), BASELINE config 4: " + shape_txt,
                         "parallelism": "dp%d, batch sharded, one %.0f MB all-reduce per step over xGMI" %
                                        (world, model.flat_params().core_numel * 4 / 1e6)}
        res["train_tflops"] = round(3 * gflop * train_res["steps"] * world /
                                    (train_res["ms_per_step"] * train_res["steps"] * 1e-3) / 1e3, 2)

    if world > 1 and a.full:
        # scaling reference measured in the SAME job: the identical step with the gradient exchange switched off, i.e.
        # what one GPU does alone (the N = 1 run of this script headlines the forward, not the training step)
        fst = trainer.fused_state()
        keep = (getattr(args, "overlap_allreduce", True), fst["allreduce"])
        args.overlap_allreduce, fst["allreduce"] = False, (lambda g: world)
        model.train()
        el_l = timed(train_step, ksteps, 2, world)
        args.overlap_allreduce, fst["allreduce"] = keep
        trainer.sync_replicas()
        model.eval()
        res["single_gpu_reference"] = {
            "ms_per_step": round(el_l / ksteps * 1e3, 4), "frames_per_s_per_gpu": round(B * T * ksteps / el_l, 1),
            "what": "the same training step with the gradient exchange skipped (max over ranks): value / (n_gpus x this) "
                    "is the weak-scaling efficiency of the data-parallel step"}

    extra = {}
    if world > 1 and a.full:
        extra["fwd_f32"] = dict(fwd_res, what="denoiser forward incl. text side, no collective (independent batches)")
    if a.full and not a.no_extra:
        extra["train_step_f32"] = train_res
        # ---- the forward as the sampling loop runs it: step-invariant text context hoisted (cached) ----
        model.cache_text_context = True
        ref_out = fwd().clone()
        el_h = timed(fwd, max(5, a.steps // 2), 2, world)
        extra["fwd_f32_text_hoisted"] = {
            "frames_per_s": round(B * T * max(5, a.steps // 2) * world / el_h, 1),
            "ms_per_step": round(el_h / max(5, a.steps // 2) * 1e3, 3),
            "what": "same forward with the cross-attention text context (key/value projections + context builds of the 8 layers) computed once "
                    "and cached -- what every step of p_sample_loop runs; NOT the headline"}
        model.cache_text_context = False
        # ---- same forward with the reduced-product GEMM modes (opt-in `precision=`) ----------
        for mode in ("bf16x3", "bf16", "bf16s"):
            set_mode(model, mode)
            el_m = timed(fwd, max(5, a.steps // 2), 2, world)
            out_m = fwd()
            err = ((out_m.double() - ref_out.double()).norm() / ref_out.double().norm()).item()
            extra["fwd_" + mode] = {"frames_per_s": round(B * T * max(5, a.steps // 2) * world / el_m, 1),
                                    "ms_per_step": round(el_m / max(5, a.steps // 2) * 1e3, 3),
                                    "rel_l2_vs_f32_path": float("%.2e" % err)}
            if rank == 0 and not a.no_cpu_baseline:
                extra["fwd_" + mode]["rel_l2_vs_cpu_oracle"] = float("%.2e" % oracle_slice_error(c, model, inp, out_m))
        set_mode(model, "f32")
        extra["fwd_bf16s"]["what"] = MODE_TEXT["bf16s"] + " -- BASELINE configs 3 / 5 arithmetic; incl. the per-call text side"
        extra["fwd_bf16s"]["fwd_tflops"] = round(gflop / extra["fwd_bf16s"]["ms_per_step"], 1)
        extra["fwd_bf16x3"]["what"] = ("split-bf16 products (hi*hi+hi*lo+lo*hi on v_mfma_f32_32x32x16_bf16), fp32 "
                                       "accumulate/storage: inside the 1e-3 fp32 parity gate; not the headline")
        extra["fwd_bf16"]["what"] = "single bf16 product, fp32 accumulate/storage"
        model.train()
        ksteps = max(3, min(a.steps, 10))
        model.precision = "bf16x3"
        el_t = timed(train_step, ksteps, 2, world)
        extra["train_step_bf16x3"] = {"frames_per_s": round(B * T * ksteps * world / el_t, 1),
                                      "ms_per_step": round(el_t / ksteps * 1e3, 3), "steps": ksteps,
                                      "what": train_what("bf16x3")}
        model.precision = "f32"
        # ---- bf16-STORAGE training step (round 4): fp32 master weights / gradients / Adam state, bf16 activations kept for
        # the backward, forward / data-gradient / weight-gradient GEMMs on the bf16 matrix cores, the Adam kernel writes the
        # bf16 weight shadow.  Own trainer (own flat state), same inputs; eager and hipGraph replay.
        if hasattr(model, "storage"):
            try:
                m16 = build_model(c, device).train()
                m16.storage = "bf16"
                tr16 = hig_amd.DDPMTrainer(args, m16)

                def step16():
                    tr16.train_step_fused(inp["x0"], inp["t"], inp["length"], inp["xf_proj"], inp["xf_out"], noise=noise)

                def step16_cap():
                    tr16.train_step_captured(inp["x0"], inp["t"], inp["length"], inp["xf_proj"], inp["xf_out"], noise=noise)

                el_16 = timed(step16, ksteps, 2, world)
                loss16 = float(tr16.fused_state()["loss"].item())
                el_16c = timed(step16_cap, ksteps, 2, world)
                trainer.train_step_fused(inp["x0"], inp["t"], inp["length"], inp["xf_proj"], inp["xf_out"], noise=noise)
                best16 = min(el_16, el_16c)
                extra["train_step_bf16s"] = {
                    "frames_per_s": round(B * T * ksteps * world / best16, 1), "ms_per_step": round(best16 / ksteps * 1e3, 3),
                    "ms_per_step_eager": round(el_16 / ksteps * 1e3, 3), "ms_per_step_hipgraph": round(el_16c / ksteps * 1e3, 3),
                    "train_tflops": round(3 * gflop / (best16 / ksteps * 1e3), 1), "loss_after_warmup": round(loss16, 5),
                    "steps": ksteps,
                    "what": "q_sample+fwd+masked-MSE+bwd+clip(0.5)+Adam, B=%d/GPU, bf16 STORAGE: bf16 activations / bf16 "
                            "matrix products (forward, data and weight gradients), fp32 accumulation, fp32 master weights, "
                            "gradients and optimizer state; the better of eager launches and hipGraph replay" % B}
                del tr16, m16
            except Exception as e:   # noqa: BLE001 -- an extra must not take the headline down
                extra["train_step_bf16s"] = {"error": repr(e)[:300]}
        # the reference's FULL update (text head trained too), as captured hipGraph(s): CLIP features in
        caps = ["a person walks towards another person and shakes hands number %d" % i for i in range(B)]
        clip_out, eot = trainer.clip_inputs(caps)

        def full_step():
            trainer.train_step_captured(inp["x0"], inp["t"], inp["length"], noise=noise, clip_out=clip_out, eot=eot)

        def full_step_eager():
            trainer.train_step_fused(inp["x0"], inp["t"], inp["length"], noise=noise, clip_out=clip_out, eot=eot)

        el_f = timed(full_step, ksteps, 2, world)
        el_e = timed(full_step_eager, ksteps, 2, world)
        best = min(el_f, el_e)
        extra["train_step_full_f32"] = {
            "frames_per_s": round(B * T * ksteps * world / best, 1), "ms_per_step": round(best / ksteps * 1e3, 3),
            "ms_per_step_hipgraph": round(el_f / ksteps * 1e3, 3), "ms_per_step_eager": round(el_e / ksteps * 1e3, 3),
            "what": "as train_step_f32 plus the text head forward/backward inside the step and its %.1f M parameters in "
                    "the same all-reduce / clip / Adam; the better of hipGraph replay and eager launches (the backward's "
                    "second stream overlaps better when launched eagerly)" % (
                        (model.flat_params().numel - model.flat_params().core_numel) / 1e6)}
        model.eval()
        if world == 1:
            # ---- DDPM sampling: the REAL 1000-step hipGraph-captured p_sample_loop at B=32 (BASELINE config 3) ----
            from hig_amd.models import gaussian_diffusion as gdm
            nst = a.ddpm_steps

            def diffusion(n):
                return hig_amd.GaussianDiffusion(betas=gdm.get_named_beta_schedule("linear", n),
                                                 model_mean_type=gdm.ModelMeanType.EPSILON,
                                                 model_var_type=gdm.ModelVarType.FIXED_SMALL,
                                                 loss_type=gdm.LossType.MSE)

            gd, gd_warm = diffusion(nst), diffusion(50)
            Bs = 32
            kw = {"xf_proj": inp["xf_proj"][:Bs].contiguous(), "xf_out": inp["xf_out"][:Bs].contiguous(),
                  "length": inp["length"][:Bs].contiguous()}
            model.cache_text_context = True     # the loop's own hoist of the step-invariant text side
            for mode in SAMPLING_MODES:
                if mode == "bf16s" and not hasattr(model, "storage"):
                    continue
                set_mode(model, mode)
                gd_warm.p_sample_loop(model, (Bs, T, c["F"]), clip_denoised=False, model_kwargs=kw)  # allocations
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                smp = gd.p_sample_loop(model, (Bs, T, c["F"]), clip_denoised=False, model_kwargs=kw)
                torch.cuda.synchronize()
                el_s = time.perf_counter() - t0
                extra["ddpm_sampling_" + mode] = {
                    "samples_per_s": round(Bs / (el_s * (1000.0 / nst)), 3),
                    "loop_seconds": round(el_s, 3), "ms_per_denoise_step": round(el_s / nst * 1e3, 4),
                    "finite": bool(torch.isfinite(smp).all()),
                    "what": "p_sample_loop B=32 T=196, %s: %d replays of the captured step actually run (text encoding "
                            "excluded, graph capture included)%s" % (
                                MODE_TEXT[mode], nst, "" if nst == 1000 else ", scaled x%.1f to 1000" % (1000.0 / nst))}
            # ---- the same loop at the batch sizes generation really runs at (ddpm_trainer.py:152 `generate(..., batch_size=1024)`,
            # the evaluation tools sample hundreds of captions per call): bf16 storage, all 1000 steps ----
            set_mode(model, "bf16s")
            by_batch = {}
            for Bg in (128, 512):
                cg = dict(c, B=Bg)
                ig = make_inputs(cg, device, rank)
                kwg = {"xf_proj": ig["xf_proj"], "xf_out": ig["xf_out"], "length": ig["length"]}
                gd_warm.p_sample_loop(model, (Bg, T, c["F"]), clip_denoised=False, model_kwargs=kwg)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                smp = gd.p_sample_loop(model, (Bg, T, c["F"]), clip_denoised=False, model_kwargs=kwg)
                torch.cuda.synchronize()
                el_s = time.perf_counter() - t0
                by_batch["B%d" % Bg] = {"samples_per_s": round(Bg / (el_s * (1000.0 / nst)), 3),
                                        "ms_per_denoise_step": round(el_s / nst * 1e3, 4),
                                        "finite": bool(torch.isfinite(smp).all())}
                if not a.no_cpu_baseline:
                    # the denoiser of THIS batch size (the un-fused regime: more than 3 workgroups of 32 rows per CU) held to
                    # the CPU oracle on a 2-sample slice of one forward -- the loop itself draws its own noise, so the
                    # check is on the step's arithmetic, not on the final sample
                    with torch.no_grad():
                        og = model(ig["x"], ig["t"], length=ig["length"], xf_proj=ig["xf_proj"], xf_out=ig["xf_out"])
                    by_batch["B%d" % Bg]["rel_l2_vs_cpu_oracle"] = float("%.2e" % oracle_slice_error(cg, model, ig, og))
                    del og
                del ig, kwg, smp
            by_batch["B32"] = {k: extra["ddpm_sampling_bf16s"][k] for k in ("samples_per_s", "ms_per_denoise_step", "finite")}
            by_batch["what"] = "p_sample_loop T=196, bf16 storage, captured step replayed %d times, by batch size" % nst
            extra["ddpm_sampling_bf16s_by_batch"] = by_batch
            set_mode(model, "f32")
            model.cache_text_context = False
            # ---- two-person denoiser: 32 pairs x 91 tokens x 263 features, fwd and fwd+bwd ----
            torch.manual_seed(0)
            c2 = dict(c, B=64, T=91, F=263)
            m2 = hig_amd.MotionInteractionTransformer(input_feats=c2["F"], num_frames=196, latent_dim=c2["d"],
                                                      ff_size=c2["ff"], num_layers=c2["L"], num_heads=c2["H"],
                                                      text_latent_dim=c2["Lt"])
            with torch.no_grad():
                for name, p in m2.named_parameters():
                    if name.startswith("out") or ".ffn.linear2." in name or ".out_layers.2." in name:
                        p.copy_(torch.randn(p.shape) * 0.02)
            m2 = m2.to(device)
            i2 = make_inputs(c2, device, rank)

            def fwd2():
                with torch.no_grad():
                    return m2(i2["x"], i2["t"], length=i2["length"], xf_proj=i2["xf_proj"], xf_out=i2["xf_out"])

            def fwdbwd2():
                out, saved = m2._launch_forward(i2["x"], i2["t"], i2["length"], i2["xf_proj"], i2["xf_out"], training=True)
                m2._launch_backward(i2["x"], i2["t"], i2["length"], i2["xf_out"], saved, i2["x0"], want_dx=False)

            k2 = max(5, a.steps // 2)
            e_f, e_fb = timed(fwd2, k2, 2, 1), timed(fwdbwd2, k2, 2, 1)
            # PIT training step (what tools/train.py runs): 16 pairs -> 64 model rows [m1|c1, m1|c2, m2|c2, m2|c1]
            args2 = types.SimpleNamespace(device=device, diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=16,
                                          num_epochs=1, log_every=50, save_latest=500, save_every_e=5, is_continue=False,
                                          model_dir="/tmp", multi=True, label_path=None, cap_id=False)
            tr2 = hig_amd.DDPMMulTrainer(args2, m2.train())
            x0p, tp, lp = i2["x0"][:32].contiguous(), i2["t"][:16].contiguous(), i2["length"][:16].contiguous()
            nz2 = torch.randn_like(x0p)

            def pit_step():
                tr2.train_step_captured(x0p, tp, lp, i2["xf_proj"], i2["xf_out"], noise=nz2)

            e_pit = timed(pit_step, k2, 2, 1)
            # the same PIT step with bf16 storage (fp32 master weights + bf16 shadow / activations): its own trainer over a copy
            # of the model, so that the fp32 step's captured graph and Adam state stay untouched
            m2b = hig_amd.MotionInteractionTransformer(input_feats=c2["F"], num_frames=196, latent_dim=c2["d"], ff_size=c2["ff"],
                                                       num_layers=c2["L"], num_heads=c2["H"], text_latent_dim=c2["Lt"], storage="bf16")
            m2b.load_state_dict(m2.state_dict())
            m2b = m2b.to(device)
            tr2b = hig_amd.DDPMMulTrainer(args2, m2b.train())

            traj16 = []

            def pit_step16():
                tr2b.train_step_captured(x0p, tp, lp, i2["xf_proj"], i2["xf_out"], noise=nz2)
                traj16.append(tr2b.fused_state()["loss"].clone())      # (a device copy: no host synchronisation in the timed loop)

            e_pit16 = timed(pit_step16, k2, 2, 1)
            loss_pit32, loss_pit16 = tr2.fused_state()["loss"].item(), tr2b.fused_state()["loss"].item()
            del tr2b, m2b
            m2.eval()
            m2.storage = "bf16"          # bf16 storage of the two-person forward (inference)
            e_f16 = timed(fwd2, k2, 2, 1)
            # the 1000-step loop of the two-person model (what mul_ddpm_trainer.py:164-222 `generate_batch` runs): 32 pairs
            loops2 = {}
            kw2 = {"xf_proj": i2["xf_proj"], "xf_out": i2["xf_out"], "length": i2["length"]}
            m2.cache_text_context = True
            for st2 in ("bf16", "f32"):
                m2.storage = st2
                gd_warm.p_sample_loop(m2, (c2["B"], c2["T"], c2["F"]), clip_denoised=False, model_kwargs=kw2)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                smp2 = gd.p_sample_loop(m2, (c2["B"], c2["T"], c2["F"]), clip_denoised=False, model_kwargs=kw2)
                torch.cuda.synchronize()
                el2 = time.perf_counter() - t0
                loops2[st2] = {"pairs_per_s": round(32 / (el2 * (1000.0 / nst)), 3), "ms_per_denoise_step": round(el2 / nst * 1e3, 4),
                               "finite": bool(torch.isfinite(smp2).all())}
            m2.cache_text_context = False
            m2.storage = "f32"
            extra["two_person"] = {
                "ddpm_sampling_1000_steps": dict(loops2, what="p_sample_loop of the two-person model, 32 pairs x 91 tokens, "
                                                 "captured step replayed %d times; keys = storage" % nst),
                "pit_train_step_ms": round(e_pit / k2 * 1e3, 3),
                "pit_train_pairs_per_s": round(16 * k2 / e_pit, 1),
                "pit_train_step_ms_bf16_storage": round(e_pit16 / k2 * 1e3, 3),
                "pit_train_pairs_per_s_bf16_storage": round(16 * k2 / e_pit16, 1),
                "pit_loss_after_the_timed_steps": {"f32": round(loss_pit32, 5), "bf16_storage": round(loss_pit16, 5)},
                "pit_loss_by_step_bf16_storage": [round(v.item(), 4) for v in traj16],
                "fwd_frames_per_s": round(c2["B"] * c2["T"] * k2 / e_f, 1), "fwd_ms": round(e_f / k2 * 1e3, 3),
                "fwd_ms_bf16_storage": round(e_f16 / k2 * 1e3, 3),
                "fwd_bwd_frames_per_s": round(c2["B"] * c2["T"] * k2 / e_fb, 1), "fwd_bwd_ms": round(e_fb / k2 * 1e3, 3),
                "what": "MotionInteractionTransformer, 32 pairs (model batch 64) x 91 tokens x 263 features, d=512 L=8, "
                        "f32 products; frames = person-tokens.  pit_train_step: 16 pairs run twice (64 rows), q_sample + "
                        "fwd + PIT loss + bwd + clip + Adam as one hipGraph"}
            # ---- BASELINE config 5 shape: long sequence, wide model (hd = 128), bf16 products ----
            c5 = dict(c, B=32, T=300, d=1024, L=12, H=8, ff=1024)
            m5 = build_model(c5, device).eval()
            i5 = make_inputs(c5, device, rank)

            def fwd5():
                with torch.no_grad():
                    return m5(i5["x"], i5["t"], length=i5["length"], xf_proj=i5["xf_proj"], xf_out=i5["xf_out"])

            r5 = {}
            m5.cache_text_context = False
            for mode in ("f32", "bf16", "bf16s"):
                set_mode(m5, mode)
                e5 = timed(fwd5, 5, 2, 1)
                r5[mode] = (e5 / 5 * 1e3, fwd5().double())
            g5 = flops_per_frame_fwd(c5) * c5["B"] * c5["T"] / 1e9
            extra["config5_long_sequence"] = {
                "fwd_ms_f32": round(r5["f32"][0], 3), "fwd_ms_bf16_products": round(r5["bf16"][0], 3),
                "fwd_ms_bf16_storage": round(r5["bf16s"][0], 3),
                "frames_per_s_bf16_storage": round(c5["B"] * c5["T"] / r5["bf16s"][0] * 1e3, 1),
                "fwd_tflops_f32": round(g5 / r5["f32"][0], 1), "fwd_tflops_bf16_storage": round(g5 / r5["bf16s"][0], 1),
                "rel_l2_bf16_products_vs_f32": float("%.2e" % ((r5["bf16"][1] - r5["f32"][1]).norm() / r5["f32"][1].norm()).item()),
                "rel_l2_bf16_storage_vs_f32": float("%.2e" % ((r5["bf16s"][1] - r5["f32"][1]).norm() / r5["f32"][1].norm()).item()),
                "rel_l2_vs_cpu_oracle": None if a.no_cpu_baseline else {
                    k: float("%.2e" % oracle_slice_error(c5, m5, i5, r5[m][1]))
                    for k, m in (("f32", "f32"), ("bf16_products", "bf16"), ("bf16_storage", "bf16s"))},
                "what": "MotionTransformer forward B=32 T=300 d=1024 L=12 H=8 (head dim 128) ff=1024, text side included: "
                        "fp32; bf16 products with fp32 storage; bf16 storage (BASELINE config 5)"}
            del m5, i5, r5
            torch.cuda.empty_cache()
            # ---- text head: encode_text after CLIP, fwd+bwd, HIP vs stock torch ops ----
            caps = ["a person walks towards another person and shakes hands number %d" % i for i in range(B)]
            th = {}
            for mode in ("hip", "torch"):
                model.text_head = mode
                model.train()
                tok, feat = model._clip_features(caps, device)

                def text_step():
                    xp, xo = model._text_head(tok, feat)
                    (xp.sum() + xo.sum()).backward()

                e_t = min(timed(text_step, k2, 2, 1), timed(text_step, k2, 1, 1))   # first pass may still be allocating
                th[mode] = round(e_t / k2 * 1e3, 3)
            model.text_head = "hip"
            model.eval()
            model.zero_grad(set_to_none=True)
            extra["text_head"] = {"fwd_bwd_ms_hip": th["hip"], "fwd_bwd_ms_stock_torch": th["torch"],
                                  "what": "text_pre_proj + 4-layer encoder (77 tokens, d=256, ff=2048) + text_ln + "
                                          "text_proj, fwd+bwd at B=64, fp32: hig_text_head_* vs nn.TransformerEncoder "
                                          "on PyTorch-ROCm"}
            # ---- SURVEY 8d variants of the headline forward: ragged lengths, F = 263, ff = 4 d ----
            var = {}
            g_v = torch.Generator().manual_seed(77)
            ragged = torch.randint(40, T + 1, (B,), generator=g_v).to(device)

            def fwd_ragged():
                with torch.no_grad():
                    return model(inp["x"], inp["t"], length=ragged, xf_proj=inp["xf_proj"], xf_out=inp["xf_out"])

            e_v = timed(fwd_ragged, k2, 2, 1) / k2 * 1e3
            var["lengths_U40_T"] = {"fwd_ms": round(e_v, 3), "frames_per_s": round(B * T / e_v * 1e3, 1),
                                    "what": "benchmark B: length ~ U{40..196}; padded frames are still computed "
                                            "(as in the reference), frames/s counts all B*T"}
            for tag, cv in (("F263", dict(c, F=263)), ("ff2048", dict(c, ff=2048))):
                mv = build_model(cv, device).eval()
                iv = make_inputs(cv, device, rank)

                def fwd_v():
                    with torch.no_grad():
                        return mv(iv["x"], iv["t"], length=iv["length"], xf_proj=iv["xf_proj"], xf_out=iv["xf_out"])

                e_v = timed(fwd_v, k2, 2, 1) / k2 * 1e3
                var[tag] = {"fwd_ms": round(e_v, 3), "frames_per_s": round(B * T / e_v * 1e3, 1),
                            "fwd_tflops": round(flops_per_frame_fwd(cv) * B * T / e_v / 1e9, 1)}
                del mv, iv
            # no_eff=True (full softmax attention, transformer.py:196-285): config 2 and the config-5 shape (head dim 128)
            for tag, cv in (("no_eff", c), ("no_eff_config5_shape", dict(c, B=32, T=300, d=1024, L=12, H=8, ff=1024))):
                mv = build_model(cv, device, no_eff=True).eval()
                iv = make_inputs(cv, device, rank)
                mv.cache_text_context = False
                e_v = timed(fwd_v, k2, 2, 1) / k2 * 1e3
                var[tag] = {"fwd_ms": round(e_v, 3), "frames_per_s": round(cv["B"] * cv["T"] / e_v * 1e3, 1)}
                set_mode(mv, "bf16s")            # bf16 storage: bf16 Q / K / V / Y through the same matrix-core kernels
                var[tag]["fwd_ms_bf16_storage"] = round(timed(fwd_v, k2, 2, 1) / k2 * 1e3, 3)
                set_mode(mv, "f32")
                if tag == "no_eff":
                    mv.train()
                    xg = iv["x"].clone().requires_grad_(True)

                    def fwdbwd_v():
                        out = mv(xg, iv["t"], length=iv["length"], xf_proj=iv["xf_proj"], xf_out=iv["xf_out"])
                        out.backward(iv["x0"])

                    var[tag]["fwd_bwd_ms"] = round(timed(fwdbwd_v, k2, 2, 1) / k2 * 1e3, 3)
                del mv, iv
            var["no_eff"]["what"] = ("config 2 with no_eff=True: flash attention on v_mfma_f32_32x32x2_f32 (fullattn.hip), "
                                     "T x T scores never written")
            var["no_eff_config5_shape"]["what"] = "B=32 T=300 d=1024 L=12 H=8 (head dim 128), no_eff=True, fp32"
            var["F263"]["what"] = "the reference's real feature width (dim_pose 263), otherwise config 2"
            var["ff2048"]["what"] = "north-star FFN shape ff = 4 d, otherwise config 2"
            extra["config2_variants"] = var
            torch.cuda.empty_cache()
            # ---- evaluator feature extraction: both classifiers on a batch of generated pairs ----
            Be, Te, Fe = 256, 91, 259
            enc = hig_amd.MotionEncoder(Fe, num_frames=196).to(device).eval()
            con = hig_amd.MotionConsistencyEvalModel(Fe, num_frames=196).to(device).eval()
            with torch.no_grad():
                for mod in (enc.out1, enc.out2):        # zero-initialised heads would make the comparison 0 == 0
                    mod.weight.normal_(0, 0.02)
            g_e = torch.Generator(device="cpu").manual_seed(5)
            ex1 = torch.randn(Be, Te, Fe, generator=g_e).to(device)
            ex2 = torch.randn(Be, Te, Fe, generator=g_e).to(device)
            elen = torch.randint(20, Te + 1, (Be,), generator=g_e).to(device)

            def eval_hip():
                with torch.no_grad():
                    return enc(ex1, ex2, length=elen) + (con(ex1, ex2, length=elen),)

            def eval_stock():   # the same parameters through stock PyTorch-ROCm ops (nn.TransformerEncoder)
                with torch.no_grad():
                    m = (torch.arange(Te, device=device)[None] < elen[:, None])
                    outs = []
                    for net in (enc, con):
                        hs = []
                        for x in (ex1, ex2):
                            mv = net.joint_embed1(x[:, 1:]) + net.sequence_embedding[None, :Te - 1]
                            hs.append(torch.cat([net.joint_embed2(x[:, 0, :4])[:, None], mv], 1))
                        if net is con:
                            h = torch.cat([net.cls_input.expand(Be, 1, -1)] + hs, 1)
                            pad = ~torch.cat([m[:, :1] | True, m, m], 1)
                            outs.append(net.cls_output(net.motionTransEncoder(h, src_key_padding_mask=pad)[:, 0]))
                        else:
                            mk = torch.cat([m, m], 1)
                            h = net.motionTransEncoder(torch.cat(hs, 1), src_key_padding_mask=~mk)
                            o = net.out1(h)
                            o[:, 0], o[:, Te] = net.out2(h[:, 0]), net.out2(h[:, Te])
                            w = mk[..., None].float()
                            ft = (o * w).sum(1) / w.sum(1)
                            outs += [net.fin_proj(ft), ft]
                    return outs

            e_h = timed(eval_hip, k2, 2, 1) / k2 * 1e3
            e_s = timed(eval_stock, k2, 2, 1) / k2 * 1e3
            oh, os_ = eval_hip(), eval_stock()
            extra["evaluator"] = {
                "pairs_per_s_hip": round(Be / e_h * 1e3, 1), "ms_hip": round(e_h, 3), "ms_stock_torch": round(e_s, 3),
                "rel_l2_feature_vs_stock": float("%.2e" % ((oh[1] - os_[1]).norm() / os_[1].norm()).item()),
                "what": "MotionEncoder + MotionConsistencyEvalModel forward (get_motion_embeddings) on 256 generated pairs "
                        "x 91 tokens x 259 features, d=512 L=8 H=8, fp32: hig_eval_encoder_fwd vs the same parameters "
                        "through nn.TransformerEncoder on PyTorch-ROCm"}
            del enc, con, ex1, ex2
    if rank == 0:
        if not a.no_extra and world == 1:
            extra["hbm_bound_kernels"] = hbm_kernel_rooflines(c, device)
            import glob
            pm = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_kernels_pmc.json")))
            extra["hbm_bound_kernels"]["counter_based"] = ("FETCH_SIZE / WRITE_SIZE passes of the same kernels: %s (not collected "
                                                           "in this run)" % (os.path.relpath(pm[-1], ROOT) if pm else "none committed"))
            extra["roofline_bf16_ffn_gemm"] = ffn_gemm_bf16_roofline(c, device)
        if a.full:
            res["roofline"] = ffn_gemm_roofline(c, device)
        if not a.no_cpu_baseline and world == 1:
            gpu_out = fwd()
            cb, rel = cpu_baseline(c, model, inp, gpu_out)
            res["cpu_baseline"] = cb
            extra["parity_rel_l2_vs_cpu_oracle"] = float("%.3e" % rel)
            sp = {"fwd": round(fwd_res["frames_per_s"] / cb["value"], 1)}
            if train_res is not None:
                sp["fwd_bwd(gpu: whole train step)"] = round(train_res["frames_per_s"] / cb["legs"]["fwd_bwd"]["value"], 1)
            for mode in SAMPLING_MODES:
                if "ddpm_sampling_" + mode in extra:
                    sp["sampling_" + mode] = round(extra["ddpm_sampling_" + mode]["samples_per_s"] /
                                                   cb["legs"]["p_sample"]["value"], 1)
            extra["gpu_over_cpu"] = sp
        res["extra"] = extra
        print(json.dumps(res))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
