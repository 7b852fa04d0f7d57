// How a denoiser call is scheduled: hig_denoiser_plan_for (every entry point of denoiser.hip).
//
// Host code only.  A plan is a pure function of the call (hig_denoiser_call: entry, the checked extents, the training and
// per-call-text flags, the facts the entry point read off its derived-operand table, whether the caller's stream is being
// captured), the switches (hig_denoiser_switches), the chip's CU count and whether the fp32 weight-stationary GEMM is active:
// no HIP call, no error state, no operand dereferenced.  The entry points build the call, plan it here, ask for the library's
// streams where the plan wants them (denoiser.hip: plan_entry, which clears the fork fields when they cannot be had), and
// run their launch sequence branching on plan fields only.
//
// Two questions stay at the launch site:
//  - whether a layer's derived slot is non-null (`folded(k)` of the fp32 forward, the fragment / fold slots of the bf16
//    forward): that reads an operand, it is not a policy;
//  - the bf16 training forward's question to hig_gemm16_plan (does the specialised-wave kernel serve linear1 with its second
//    output?): a query of the GEMM plan, answered there.
#include "hig_host.h"

namespace {

bool mm16_hd(int hd) { return hd == 64 || hd == 128; }
bool sty_heads(int H) { return H == 4 || H == 8; }   // the fused apply kernels keep H / 4 heads per wave
bool has(const hig_denoiser_call& c, int fact) { return (c.facts & fact) != 0; }

// Does the text side run in its batched form (one key/value GEMM + one context build for all layers)?  Inference, linear
// attention, and the caller's derived-operand table carries the stacked folded weights (HIG_D32_TEXT_* / HIG_D16_TEXT_*);
// bf16 storage: its text layout has the `kvall` slot (linear attention).  HIG_TEXT_BATCH=0 keeps the per-layer form.
bool text_batched(const hig_denoiser_call& c, const hig_denoiser_switches& sw, bool bf16) {
  if (!c.has_xf_out || !sw.text_batch || c.training || c.full || !has(c, HIG_DN_FACT_TEXT_GLOBALS)) return false;
  return !bf16 || has(c, HIG_DN_FACT_KVALL);
}
// Context build of the bf16-storage entries: the bf16-matrix-core kernel of linattn16.hip where it is built (head dim 64 /
// 128), else the fp32-MFMA kernels with bf16 loads (HIG_CTX16=0 forces those).
bool ctx_mm16(const hig_denoiser_call& c, const hig_denoiser_switches& sw) { return sw.ctx16 && mm16_hd(c.hd); }
// HIG_FUSE_APPLY: 2 (default) = the bf16-matrix-core kernel of linattn16.hip where it is built, 1 = the fp32-MFMA fused
// kernel, 0 = apply + row kernel (the inference forward and the training forward read the same switch)
bool fuse_mm16(const hig_denoiser_call& c, const hig_denoiser_switches& sw) {
  return sw.fuse_apply == 2 && mm16_hd(c.hd) && sty_heads(c.H);
}

void plan_fwd32(const hig_denoiser_call& c, const hig_denoiser_switches& sw, bool forks_ok, bool wsp32_active, hig_denoiser_plan_t& p) {
  const int64_t M = (int64_t)c.B * c.T, ss_ld = (int64_t)c.nsty * c.L * 2 * c.d;
  p.text_batched = text_batched(c, sw, false);
  // The cross-attention text side (hig_denoiser_fwd_text): layer l's context matrices are first needed in front of layer l's
  // cross-attention, a third of a layer into the forward -- its 2 L launches (key/value GEMMs over B N rows, context builds)
  // run on a third stream next to the first layers, one event per layer (events only: eager launches; under capture, or
  // without the library's streams, they run first on the caller's stream as hig_text_context would).
  // (the batched form is two whole-chip launches: next to the first layers' GEMMs -- one workgroup per CU each -- they only take
  // turns with them, 6.04 ms forked against 5.98 in front at config 2; it runs first on the caller's stream)
  p.text_fork = forks_ok && c.has_xf_out && sw.text_fork && c.L <= HIG_MAX_TEXT_LAYERS && !p.text_batched;
  // inference + linear attention, head dim 64 with 4 or 8 heads: `apply` and the stylization front that follows it run as ONE
  // kernel (hig_linattn_apply_sty -> apply_sty_wave64_kernel, linattn.hip): the (M, d) attention output y never reaches HBM, its
  // workspace slots (y1, y2) and the statistics slots (st2, st4) are not written.  Self and cross attention of every layer.
  // Everything else keeps the pair apply + ln_mod_silu: training (the backward reads y and the LayerNorm statistics), full
  // attention, and head dim 128 (only the older fused kernel exists there, and it lost: 83.8 against 71.1 us per attention).
  // The entry wants 16-byte aligned rows and parameter vectors: d and the row stride of the scale / shift table are multiples
  // of 4 floats here (d = 64 H); the workspace slots and the parameter blocks sit at 16-byte aligned offsets (the entry checks
  // and fails loudly, it never falls back).
  // Measured per attention, fused against the pair (profiles/r07_notes.md): 28.2-28.7 against 31.2-31.5 us at B = 64, T = 196,
  // 15.8-16.0 against 20.6-21.4 at B = 32 (the sampling loop), 17.0-17.8 against 21.8-22.8 at T = 91 (the two-person shape; 9.9-10.6
  // against 12.8-13.2 at B = 32): no row threshold, unlike hig_linattn_apply's.
  p.fuse_apply = !c.training && !c.full && c.hd == 64 && sty_heads(c.H) && ss_ld % 4 == 0;
  // LayerNorm fold (fp32 storage): inference only, d a multiple of 128, operands derived by the caller per parameter version
  p.fold32 = sw.lnfold32 && has(c, HIG_DN_FACT_TABLE) && !c.training && c.d % 128 == 0 && c.d <= 1024;
  // Two halves of the batch on two streams (single-person model, enough rows): the second half runs on the library's
  // side stream, forked after the per-sample prologue and joined before returning (events only: capturable).  An
  // in-order stream leaves the chip idle in every kernel's tail and ramp-up; two independent chains of the same
  // kernels fill those gaps (two whole forwards side by side: 5.85 ms each against 6.6 alone).
  // (Round 6: with the exact-fp32 products on the weight-stationary kernel -- one workgroup per CU, every launch fills the chip
  // by itself -- two half-batch chains no longer fit side by side, and each half pays the kernel's fixed cost on half the rows:
  // B = 64 forward 5.85 ms split against 5.78 ms on one stream.  Unset, the split is therefore kept for the bf16 product modes
  // and for chips where that kernel declines.)
  const int split_env = sw.fwd_split >= 0 ? sw.fwd_split : ((c.prec == HIG_PREC_F32 && wsp32_active) ? 0 : 1);
  // (M >= 8192: measured at B = 64.  Half batches run other tile schedules than the whole batch -- other split-tail
  // geometry, so sums in another order, last-bit differences (2e-7 rel-L2) -- and the B = 32 sampling step is expected to
  // equal its captured form bit for bit (tests/test_gpu_full_size.py), so small batches stay on one stream.)
  // (eager launches only: replayed from a hipGraph the two branches cost more than they gain -- captured training step
  // 21.2 -> 22.2 ms, against 20.4 -> 20.2 ms eager; forward 6.23 -> 6.10 ms eager)
  p.split = forks_ok && split_env && !c.two && c.B >= 16 && M >= 8192;
  p.wants_side_stream = p.text_fork || p.split;
}

void plan_fwd16(const hig_denoiser_call& c, const hig_denoiser_switches& sw, bool forks_ok, int cus, hig_denoiser_plan_t& p) {
  const int64_t ss_ld = (int64_t)c.nsty * c.L * 2 * c.d;
  p.text_batched = text_batched(c, sw, true);
  p.ctx_mm16 = ctx_mm16(c, sw);
  // Everything that hangs off the B conditioning rows instead of the M frame rows -- the embedding chain (its last GEMM reads
  // every stylization block's (2 d, E) weight: 604 MB at the config-5 shape, HBM-bound) and the cross-attention text side --
  // is first needed a few launches into layer 0 / in front of layer l's cross-attention.  Launched eagerly with the library's
  // streams available, both run on the third stream next to the frame-row launches (events only; HIG_FWD16_FORK=0, a capture
  // in progress or no side streams: everything in order on the caller's stream).
  // Measured (tools/fwd16_fork.sh, same call, per-call text: off / text / both): config 2 B = 64 1.718 / 1.667 / 1.657-1.672 ms,
  // B = 32 1.158 / 1.134 / 1.121; config-5 shape 4.83 / 4.71 / 4.66-4.70; with the text side cached, forking the embedding
  // chain alone COSTS 2-6 % at config 2 (its 35 us of launches are shorter than the two event waits they add): it is forked
  // only when its modulation weight is large (>= 256 MB: the d = 1024 models).
  // (round 6: the BATCHED text side -- three launches, two of them chip-wide -- is faster in front of the frame-row launches than
  // next to them: B = 64 1.488 against 1.540 ms, per-layer form 1.539 forked / 1.603 in front; not forked by default)
  // HIG_FWD16_FORK: bit 0 embedding chain, bit 1 text side.  (Unset and without a per-call text side bit 1 stays set: the
  // entry then asks for the library's streams -- creating them on first use -- and forks nothing.)
  const int fork_env = sw.fwd16_fork >= 0 ? sw.fwd16_fork : ((p.text_batched ? 0 : 2) | (((int64_t)c.E * ss_ld * 2 >= (256ll << 20)) ? 1 : 0));
  p.wants_side_stream = forks_ok && fork_env && c.L < HIG_MAX_TEXT_LAYERS;   // (the last text event joins the embedding chain)
  p.fork_emb = p.wants_side_stream && (fork_env & 1);
  p.fork_text = p.wants_side_stream && (fork_env & 2) && c.has_xf_out;
  // K1 as its own kernel pair (weight padded / rounded to bf16, x rounded in LDS, bf16 MFMA): 31 -> ~8 us at B = 32
  p.joint16 = sw.joint16 && c.d % 128 == 0 && c.F <= 512;
  // attention output -> stylization block.  With 4 or 8 heads the `y = q A` product, the LayerNorm, the modulation and
  // the SiLU are ONE kernel (y never leaves the chip); otherwise apply + row kernel.
  // (the fp32-MFMA fused kernel is opt-in: measured equal at B = 64 and 4 % slower at B = 32 -- its fp32 MFMAs serialise 128
  // per wave behind poorly coalesced query loads; profiles/r02_notes.md)
  p.fuse_mm16 = fuse_mm16(c, sw);
  p.fuse_apply = (sw.fuse_apply == 1 || p.fuse_mm16) && sty_heads(c.H);
  // hig_attn_out16 / hig_rows_out16 (a whole stylization block as one launch) for the small batches: there the launches are
  // bound by the per-launch floor (~4.4 us) and a fetch-bound projection.  Two of their workgroups (one per 32 rows of a sample)
  // are resident per CU; same-call A/B, forward, fused vs not: B = 32 (224 workgroups) 0.996 vs 1.097 ms, B = 40 1.221 vs
  // 1.262, B = 64 (448) 1.521 vs 1.614, B = 73 1.640 vs 1.733, B = 96 (672) 2.067 vs 2.100, B = 128 (896) 2.512 vs 2.516,
  // B = 256 4.393 vs 4.377: used up to 3 workgroups per CU (768).  HIG_FUSE_OUT=0 switches it off, n >= 2 moves the limit to n per CU.
  p.fuse_out = sw.fuse_out && p.fuse_mm16 && c.d == 512 && c.hd == 64 && c.H == 8 &&
               ((int64_t)c.T + 31) / 32 * c.B <= (int64_t)cus * (sw.fuse_out >= 2 ? sw.fuse_out : 3);
}

// The F-wide edges of the bf16 backward on the bf16 matrix kernels too (HIG_EDGE16=0: the fp32 kernels on fp32 copies): d(out)
// and x are rounded to bf16 rows padded to Fp = F rounded up to 32 (hig_cast_pad_bf16), the data gradient d(h_L) = d(out) W_out
// is a bf16 GEMM over Fp (W_out^T padded with zero columns), the two weight gradients run on wgrad16 into padded fp32 scratch
// and are copied into place.  Scratch (hig_edge16_layout): the first of the two (M, d) fp32 buffers the fp32 path needs.
void plan_edge16(const hig_denoiser_call& c, const hig_denoiser_switches& sw, hig_denoiser_plan_t& p) {
  const int64_t M = (int64_t)c.B * c.T, Fp = ((int64_t)c.F + 31) / 32 * 32;
  // (the row-count limit first: beyond it the byte offsets are not formed)
  p.edge16 = sw.edge16 && c.d % 8 == 0 && M < (1ll << 30) && M * Fp < (1ll << 30) && hig_edge16_layout(M, Fp, c.d).end <= M * c.d * 4;
  p.Fp = p.edge16 ? (int32_t)Fp : 0;
}

}  // namespace

const hig_denoiser_switches& hig_denoiser_switch_values() {
  auto env_int = [](const char* v, int dflt) { return v ? atoi(v) : dflt; };
  static const hig_denoiser_switches sw = {
      env_int(getenv("HIG_TEXT_BATCH"), 1),    // 0: the per-layer form of the text side
      env_int(getenv("HIG_TEXT_FORK"), 1),     // 0: the fp32 forward's text side on the caller's stream
      env_int(getenv("HIG_FWD_SPLIT"), -1),    // 0 / 1: never / always (shape permitting) halve the fp32 forward over two streams
      env_int(getenv("HIG_LNFOLD32"), 1),      // 0: no LayerNorm fold in the fp32 forward
      env_int(getenv("HIG_FWD16_FORK"), -1),   // bit 0 embedding chain, bit 1 text side of the bf16 forward on the third stream
      env_int(getenv("HIG_CTX16"), 1),         // 0: bf16 context builds on the fp32-MFMA kernels
      env_int(getenv("HIG_JOINT16"), 1),       // 0: joint_embed of the bf16 forward through the fp32 GEMM + cast
      env_int(getenv("HIG_FUSE_APPLY"), 2),    // 2 / 1 / 0: bf16-matrix-core fused apply / fp32-MFMA fused apply / apply + row kernel
      env_int(getenv("HIG_FUSE_OUT"), 1),      // 0: no one-launch stylization block; n >= 2: up to n of its workgroups per CU
      env_int(getenv("HIG_EDGE16"), 1),        // 0: the F-wide edges of the bf16 backward on the fp32 kernels
      env_int(getenv("HIG_BWD_OVERLAP"), -1),  // -1 each form's own default, 0 nothing forked anywhere, 1 weight gradients forked in every form
  };
  return sw;
}

hig_denoiser_plan_t hig_denoiser_plan_for(const hig_denoiser_call& c, const hig_denoiser_switches& sw, int cus, bool wsp32_active) {
  hig_denoiser_plan_t p = {};
  p.entry = c.entry;
  // HIG_BWD_OVERLAP=0 keeps everything on the caller's stream: it vetoes every fork, the forward's included.  The forward
  // forks are for eager launches only.
  const bool forks_ok = sw.bwd_overlap != 0 && !c.capturing;
  switch (c.entry) {
    case HIG_DN_ENTRY_TEXT32:
      p.text_batched = text_batched(c, sw, false);
      break;
    case HIG_DN_ENTRY_TEXT16:
      p.text_batched = text_batched(c, sw, true);
      p.ctx_mm16 = ctx_mm16(c, sw);
      break;
    case HIG_DN_ENTRY_FWD32:
      plan_fwd32(c, sw, forks_ok, wsp32_active, p);
      break;
    case HIG_DN_ENTRY_FWD16:
      plan_fwd16(c, sw, forks_ok, cus, p);
      break;
    case HIG_DN_ENTRY_FWD16_TRAIN:
      // attention output -> stylization front: y = softmax(q) . A, LayerNorm, modulation, SiLU as ONE kernel that also writes y
      p.fuse_front = fuse_mm16(c, sw);
      p.ctx_mm16 = ctx_mm16(c, sw);
      break;
    case HIG_DN_ENTRY_BWD32:
      // Eager launches: the weight gradients go to the second stream.  Under stream capture they stay on the caller's (unless
      // HIG_BWD_OVERLAP=1): the replayed graph did not turn the fork into overlap -- config 2, captured fp32 step 21.6-21.7 ms
      // forked against 21.2 on one stream, while eager launches gain a millisecond from it (20.4 against 21.3).
      p.wgrad_fork = sw.bwd_overlap == 1 || forks_ok;
      break;
    case HIG_DN_ENTRY_BWD16:
      // bf16 storage: the weight gradients stay on the caller's stream unless HIG_BWD_OVERLAP=1 asks for the fork.  The kernels of
      // this mode are one-workgroup-per-CU designs (gemm_wsp16: 159 KB of LDS, wgrad16x: 128 KB + twelve waves): two of them cannot
      // share a CU, so a weight gradient on the second stream delays the workgroups of the data-gradient GEMM CU by CU instead of
      // filling idle slots -- config 2, captured step: 7.27 ms on one stream, 7.40 forked (7.72 with the LayerNorm reductions
      // forked as well).  The fp32 step keeps the fork (tiled kernels, several workgroups per CU: 20.4 vs 21.4 ms eager).
      p.wgrad_fork = sw.bwd_overlap == 1;
      plan_edge16(c, sw, p);
      break;
    default:
      p.entry = -1;
      break;
  }
  if (c.entry == HIG_DN_ENTRY_BWD32 || c.entry == HIG_DN_ENTRY_BWD16) p.wants_side_stream = p.wgrad_fork;
  return p;
}
