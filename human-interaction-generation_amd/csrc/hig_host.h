// Host-side helpers shared by the orchestration translation units (denoiser.hip and, through enc_layers.h, the encoder chains).
#pragma once
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "hig_common.h"

int hig_gemm_launch(const hig_gemm_desc& g, int splits, float* slabs, hipStream_t st);
// one launch of the GEMM kernel of `path` (HIG_GEMM_PATH_*): called at the launch site (gemm.hip, hig_gemm_path_launches)
void hig_gemm_path_count(int path);
// one launch of the attention kernel of `path` (HIG_ATTN_PATH_*) with gridDim.y = split (linattn.hip, hig_attn_path_launches)
void hig_attn_path_count(int path, int split);
// I <= 64 rows with EPI_BIAS / EPI_BIAS_RES: split-R over `scratch` so the weight streams through ~1024 workgroups
int hig_gemm_few_rows(const hig_gemm_desc& g, float* scratch, int64_t scratch_floats, hipStream_t st);

// Scratch for the split tail of the exact-fp32 GEMM (gemm.hip, KArgs): the launches that follow on this thread may
// park partial sums in it.  HIG_GEMM_TAIL_BYTES long, 16-byte aligned; its first HIG_GEMM_TAIL_CNT_BYTES (tickets)
// must be zero before the first launch and are left zero by every launch.  One scratch serves one stream at a time.
// nullptr switches the tail off.
constexpr int64_t HIG_GEMM_TAIL_CNT_BYTES = 1024;
constexpr int64_t HIG_GEMM_TAIL_BYTES = HIG_GEMM_TAIL_CNT_BYTES + 256 * 16384;   // 256 slices of a 64x64 tile
void hig_gemm_set_tail_scratch(void* ws, int64_t bytes);

// Chip geometry of the CURRENT device, read once per device with hipDeviceGetAttribute (never a literal in a launch
// rule): compute units, and XCDs = CUs / 32 (a gfx950 XCD has 32 active CUs; an MI355X in SPX mode reports 256 -> 8, a
// CPX partition 32 -> 1).  Round-counting tile rules, persistent grid sizes and the residency limits of the fused
// kernels are derived from these; kernels whose block -> XCD mapping is compiled for 8 XCDs decline on anything else.
int hig_chip_cus();
inline int hig_chip_xcds() { const int c = hig_chip_cus() / 32; return c < 1 ? 1 : c; }

int hig_gemm16_launch(const hig_gemm16_desc& g, hipStream_t st);
// split-R form of the tiled bf16 kernel + deterministic slab reduction (weight gradients); splits == 0: library rule
int hig_gemm16_split_launch(const hig_gemm16_desc& g, int splits, float* slabs, int64_t slab_floats, hipStream_t st);
// dW = dC^T . act (+ dbias = column sums of dC) straight from the row-major bf16 operands (wgrad16.hip: transpose reads)
// (deferred != NULL: the slab reduction is left to hig_wgrad16_reduce_batch, which sums up to HIG_WG_RB_MAX gradients in one launch)
struct hig_wg_reduce {
  const float* slabs; int nsplit; int64_t slab;   // nsplit slabs of `slab` floats: [J x K | J] each
  int64_t n4; float* out;                          // J K / 4 float4 of dW
  int64_t nb4; float* dbias;                       // J / 4 float4 of dbias (0: none)
};
constexpr int HIG_WG_RB_MAX = 12;
int hig_wgrad16_launch(const void* dC, int64_t ldd, const void* act, int64_t ldx, int64_t rows, int J, int K, float* dW, float* dbias,
                       int splits, float* slabs, int64_t slab_floats, hipStream_t st, hig_wg_reduce* deferred = nullptr);
int hig_wgrad16_reduce_batch(const hig_wg_reduce* entries, int n, hipStream_t st);
// up to HIG_WG_GROUP_MAX gradients in one launch of the kernel (wgrad16.hip)
struct hig_wg_problem {
  const void* dC; int64_t ldd; const void* act; int64_t ldx; int64_t rows; int J, K; float* dW; float* dbias; int splits;   // splits 0: the rule
};
constexpr int HIG_WG_GROUP_MAX = 4;
int hig_wgrad16_launch_group(const hig_wg_problem* probs, int n, float* slabs, int64_t slab_floats, hipStream_t st, hig_wg_reduce* deferred,
                             int64_t* used_floats);
int64_t hig_wgrad16_rule_floats(int64_t rows, int J, int K, int64_t room);   // slab floats the split rule takes, given `room`
// out[e] = sum_s slabs[s * slab + e], e < n (n % 4 == 0, 16-byte aligned), in split order (gemm.hip)
int hig_reduce_slabs(const float* slabs, int splits, int64_t slab, int64_t n, float* out, hipStream_t st);
// ---- which kernel serves a GEMM call (gemm_plan.hip): decided apart from the launch ----
// The GEMM switches ("Switches"), each read once per process by hig_gemm_switch_values().
struct hig_gemm_switches {
  int wsp16, ws16, ws_rows, ws_nwj, lnfold, lnfold1024, fewrow16, tile16;   // HIG_BF16_WSP, _WS, _WS_ROWS, _WS_NWJ, HIG_LNFOLD, HIG_LNFOLD1024, HIG_BF16_FEWROW, _TILE
  int wsp32, tile32, tail32;                                                // HIG_F32_WSP, HIG_GEMM_TILE, HIG_GEMM_TAIL
  int few_rows_split;                                                       // HIG_FEW_ROWS_SPLIT (hig_gemm_few_rows)
};
const hig_gemm_switches& hig_gemm_switch_values();
// rc == HIG_OK: `launches` launches of the kernel of `path` (HIG_GEMM_PATH_*; -1 and 0 launches: an empty problem) in the
// instance `variant` names; else the error the entry point returns, with its message.
struct hig_plan { int rc, path, launches, variant; char msg[256]; };
#define HIG_WSP_VARIANT(xt, aux) ((xt) + 4 * ((aux) ? 1 : 0))           /* gemm_wsp16 / gemm_wsp32: the XT / AUX instance (XT 1: fold producer, 2: consumer) */
#define HIG_WS16_VARIANT(nwj, role) ((nwj) + 256 * (role))              /* gemm_ws16: nwj code 8 / 4 / 2 / 44, fold role as XT */
#define HIG_TILE16_VARIANT(rows, bk, ns) ((rows) * 1000 + (bk) * 10 + (ns))   /* tiled bf16 kernel: tile rows, k-tile, ring stages */
#define HIG_TILE32_VARIANT(tile, tail) ((tile) + 16 * (tail))           /* tiled fp32 kernel: tile 0 .. 3 = 128x128, 64x128, 128x64, 64x64; tail slices (1: none) */
hig_plan hig_gemm16_plan(const hig_gemm16_desc& g, const hig_gemm_switches& sw, int cus);
// unsplit launches of hig_gemm_launch; tail_ws_bytes: room behind the tickets of the split-tail scratch (0: none set)
hig_plan hig_gemm32_plan(const hig_gemm_desc& g, int64_t tail_ws_bytes, const hig_gemm_switches& sw, int cus);
bool hig_gemm_ws16_lnfold_ok(int64_t rows, int d);
// the launchers of the kernels a plan names (each in its kernel's file; called from hig_gemm16_launch / hig_gemm_launch only)
int hig_gemm_wsp16_launch(const hig_gemm16_desc& g, int variant, hipStream_t st);
int hig_gemm_ws16_launch(const hig_gemm16_desc& g, int variant, hipStream_t st);
int hig_gemm_wsp32_launch(const hig_gemm_desc& g, int variant, hipStream_t st);
constexpr int64_t HIG_GEMM_TAIL_UNIT_BYTES = 256 * 16 * 4;   // one workgroup's parked partial sums of a 64x64 tile
// gemm_wsp32's column panels as at most HIG_P32_MAXSEG segments of a power-of-two panel count (<= 256 each); -1: more
constexpr int HIG_P32_MAXSEG = 3;
inline int hig_wsp32_segments(int np, int* seg_p0, int* seg_np) {
  int nseg = 0, p0 = 0;
  for (int s = 0; s < HIG_P32_MAXSEG; ++s) { seg_p0[s] = 0; seg_np[s] = 1; }
  while (np > 0) {
    int n = 256;
    while (n > np) n >>= 1;
    if (nseg == HIG_P32_MAXSEG) return -1;
    seg_p0[nseg] = p0; seg_np[nseg] = n; ++nseg;
    p0 += n; np -= n;
  }
  return nseg;
}
// K = 1536 / 2048 through gemm_wsp32 in two passes: C = X[:, :1024] W[:, :1024]^T (+ bias / res), then C += X[:, 1024:] W[:, 1024:]^T
// with C as its own residual (a lane re-reads exactly the element it stores two tiles later)
inline void hig_gemm32_two_pass(const hig_gemm_desc& g, hig_gemm_desc* p1, hig_gemm_desc* p2) {
  *p1 = g; p1->R = 1024;
  *p2 = g; p2->X = g.X + 1024; p2->Y = g.Y + 1024; p2->R = g.R - 1024;
  p2->epi = HIG_EPI_RES; p2->bias = nullptr; p2->res = g.C; p2->ldr = g.ldc;
}
// the vector-load form of the tiled fp32 kernel: aligned operands, whole k-tiles, whole float4 quads of a reduce-slow operand
inline bool hig_gemm32_fast(const hig_gemm_desc& g) {
  auto vec = [](const void* p, int64_t ld) { return ld % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  return vec(g.X, g.ldx) && vec(g.Y, g.ldy) && g.R % 32 == 0 && g.R > 0 && (!g.x_rs || (g.I % 4 == 0 && g.I >= 4)) && (!g.y_rs || (g.J % 4 == 0 && g.J >= 4));
}
// the (x_rs, y_rs, xf, xf_on_y, epi) combinations the tiled fp32 kernel is built for
#ifdef HIG_GEMM_PROBE  // compile-time aid: build a single combination
#define HIG_GEMM32_COMBOS(CASE) CASE(0, 0, HIG_XF_NONE, 0, HIG_EPI_BIAS_GELU)
#else
#define HIG_GEMM32_COMBOS(CASE)                                                                                       \
  /* forward (activations x weight^T) */                                                                              \
  CASE(0, 0, HIG_XF_NONE, 0, HIG_EPI_NONE) CASE(0, 0, HIG_XF_NONE, 0, HIG_EPI_BIAS) CASE(0, 0, HIG_XF_NONE, 0, HIG_EPI_BIAS_GELU) \
  CASE(0, 0, HIG_XF_NONE, 0, HIG_EPI_BIAS_POS) CASE(0, 0, HIG_XF_NONE, 0, HIG_EPI_BIAS_RES)                           \
  CASE(0, 0, HIG_XF_NONE, 0, HIG_EPI_RES) /* dgrad through a transposed weight copy */                                \
  CASE(0, 0, HIG_XF_NONE, 0, HIG_EPI_DGELU) CASE(0, 0, HIG_XF_LN, 0, HIG_EPI_BIAS) CASE(0, 0, HIG_XF_LN_MOD_SILU, 0, HIG_EPI_BIAS_RES) \
  CASE(0, 0, HIG_XF_SILU, 0, HIG_EPI_BIAS) CASE(0, 0, HIG_XF_SILU, 0, HIG_EPI_BIAS_RES)                               \
  CASE(0, 0, HIG_XF_SILU, 0, HIG_EPI_NONE) /* split-R partials of the few-row GEMMs */                                \
  /* dgrad (dC x weight) */                                                                                           \
  CASE(0, 1, HIG_XF_NONE, 0, HIG_EPI_NONE) CASE(0, 1, HIG_XF_NONE, 0, HIG_EPI_RES) CASE(0, 1, HIG_XF_NONE, 0, HIG_EPI_DGELU) \
  /* wgrad (dC^T x activations) */                                                                                    \
  CASE(1, 1, HIG_XF_NONE, 0, HIG_EPI_NONE) CASE(1, 1, HIG_XF_LN, 1, HIG_EPI_NONE) CASE(1, 1, HIG_XF_LN_MOD_SILU, 1, HIG_EPI_NONE) \
  CASE(1, 1, HIG_XF_SILU, 1, HIG_EPI_NONE)
#endif
// "instantiate this launcher for the runtime epilogue": f(std::integral_constant<int, E>) for the E of the list that equals
// `epi`; `none` when the list does not hold it
template <int... E> struct hig_epi_list {};
using hig_epi16_fewrow = hig_epi_list<HIG_EPI_NONE, HIG_EPI_BIAS, HIG_EPI_BIAS_GELU, HIG_EPI_BIAS_RES, HIG_EPI_BIAS_SILU, HIG_EPI_BIAS_RES_SILU>;
using hig_epi16_all = hig_epi_list<HIG_EPI_NONE, HIG_EPI_BIAS, HIG_EPI_BIAS_GELU, HIG_EPI_BIAS_RES, HIG_EPI_BIAS_SILU, HIG_EPI_BIAS_RES_SILU, HIG_EPI_RES, HIG_EPI_DGELU>;
template <int... E, class F>
int hig_with_epi(hig_epi_list<E...>, int epi, int none, F&& f) {
  int rc = none;
  (void)(((epi == E) && ((rc = f(std::integral_constant<int, E>{})), true)) || ...);
  return rc;
}
// ---- which kernel serves an attention call, and with which split (attn_plan.hip): decided apart from the launch ----
// The attention switches ("Switches"), each read once per process by hig_attn_switch_values().
struct hig_attn_switches {
  int apply_wave;       // HIG_APPLY_WAVE: 0 keeps fp32 head dim 64 off apply_wave64_kernel
  int fullattn_waves;   // HIG_FULLATTN_WAVES: 2 / 4 / 8 forces the waves per workgroup of the matrix-core full-attention kernels (0: the rule)
  int fullattn_valu;    // HIG_FULLATTN_VALU: != 0 keeps head dim 64 of full attention on the VALU kernels
};
const hig_attn_switches& hig_attn_switch_values();
// What a decision may depend on, and nothing else.  entry: HIG_ATTN_ENTRY_*; io: HIG_ATTN_IO_*; rows = Tq and Tk = keys for
// full attention (Tk unused otherwise); facts: HIG_ATTN_FACT_* (include/hig.h) -- what the entry point read off its
// operands' null-ness, low pointer bits and leading dimensions.
struct hig_attn_call {
  int entry, io;
  int B, rows, Tk, H, hd;
  bool has_scratch;
  int facts;
};
// The facts of a call whose input rows (pointers and leading dimensions in bytes OR-ed together: `in`), output rows
// (`out`) and fp32 parameter vectors (`par`) have these low bits.
inline int hig_attn_facts(bool operands, uintptr_t in, uintptr_t out, uintptr_t par = 0, bool out_i32 = true) {
  return (operands ? HIG_ATTN_FACT_OPERANDS : 0) | ((in & 7) ? 0 : HIG_ATTN_FACT_IN8) | ((in & 15) ? 0 : HIG_ATTN_FACT_IN16) |
         ((out & 7) ? 0 : HIG_ATTN_FACT_OUT8) | ((out & 15) ? 0 : HIG_ATTN_FACT_OUT16) | ((par & 15) ? 0 : HIG_ATTN_FACT_PAR16) |
         (out_i32 ? HIG_ATTN_FACT_OUT_I32 : 0);
}
inline uintptr_t hig_low_bits(const void* p) { return reinterpret_cast<uintptr_t>(p); }
inline uintptr_t hig_low_bits(int64_t ld, int elem_bytes) { return (uintptr_t)ld * (uintptr_t)elem_bytes; }
// rc == HIG_OK: the kernel of `path` (HIG_ATTN_PATH_*) runs with `split` (what hig_attn_last_split reports: gridDim.y, the
// number of chunks, or the strips per sample) in the instance `variant` names; else the error the entry point returns.
// variant: full attention on the matrix cores: waves per workgroup (2 / 4 / 8); hig_linattn_apply_bwd: HIG_ATTN_VARIANT_MERGE
// when the dA partials go to scratch and chunk_sum_kernel adds them up (0: the single partial IS dA); 0 everywhere else.
struct hig_attn_plan_t { int rc, path, split, variant; char msg[160]; };
#define HIG_ATTN_VARIANT_MERGE 1
hig_attn_plan_t hig_attn_plan_for(const hig_attn_call& c, const hig_attn_switches& sw, int cus, bool big_lds_ok);
bool hig_attn_mfma_hd(int hd);   // head dims the matrix-core linear-attention kernels are built for
// Steps 1 - 3 of every attention entry point: plan the call for this device, refuse with the plan's error or count the launch
// (the one place a planned call is counted).  Step 4 is the entry's switch on p->path into a launcher next to the kernel, which
// takes the plan's split and variant and decides nothing.
inline int hig_attn_plan_entry(hig_attn_plan_t* p, const hig_attn_call& c, bool big_lds_ok = true) {
  *p = hig_attn_plan_for(c, hig_attn_switch_values(), hig_chip_cus(), big_lds_ok);
  if (p->rc != HIG_OK) return hig_set_error(p->rc, "%s", p->msg);
  hig_attn_path_count(p->path, p->split);
  return HIG_OK;
}
// ---- how a denoiser call is scheduled (denoiser_plan.hip): decided apart from its launch sequence ----
// The denoiser switches ("Switches"), each read once per process by hig_denoiser_switch_values().  The order is
// that of hig_denoiser_plan's `switches` array (include/hig.h).
struct hig_denoiser_switches {
  int32_t text_batch, text_fork, fwd_split, lnfold32, fwd16_fork, ctx16, joint16, fuse_apply, fuse_out, edge16, bwd_overlap;
};
static_assert(sizeof(hig_denoiser_switches) == HIG_DN_NSWITCHES * sizeof(int32_t), "one int32 per switch, in the documented order");
const hig_denoiser_switches& hig_denoiser_switch_values();
// What a decision may depend on, and nothing else.  entry: HIG_DN_ENTRY_*; the checked extents of the call's dims; facts:
// HIG_DN_FACT_* (what the entry point read off its derived-operand table); capturing: the caller's stream is under capture.
struct hig_denoiser_call {
  int entry;
  int B, T, F, d, E, ff, L, H, hd, N, nsty, two, full, prec;
  bool training, has_xf_out;
  int facts;
  bool capturing;
};
// Named 0 / 1 answers (Fp: the padded feature count of edge16) in the order of the HIG_DN_PLAN_* slots; what an entry does not
// decide stays 0.  The fork fields (text_fork, split, fork_emb, fork_text, wgrad_fork) say what the call wants: the entry point
// clears them when the library's streams cannot be had.
struct hig_denoiser_plan_t {
  int32_t entry;
  int32_t text_batched, text_fork, fuse_apply, fold32, split;        // fp32 forward / text context (text_batched, fuse_apply: bf16 too)
  int32_t fork_emb, fork_text, ctx_mm16, joint16, fuse_mm16, fuse_out;   // bf16 forward / text context
  int32_t fuse_front;                                                 // bf16 training forward
  int32_t wgrad_fork;                                                 // backward
  int32_t edge16, Fp;                                                 // bf16 backward
  int32_t wants_side_stream;                                          // the entry asks for the library's streams at all
};
static_assert(sizeof(hig_denoiser_plan_t) == HIG_DN_PLAN_NSLOTS * sizeof(int32_t), "one int32 per HIG_DN_PLAN_* slot");
hig_denoiser_plan_t hig_denoiser_plan_for(const hig_denoiser_call& c, const hig_denoiser_switches& sw, int cus, bool wsp32_active);
constexpr int HIG_MAX_TEXT_LAYERS = 32;   // per-layer events of the forked text side (denoiser.hip: SideStream)
// Byte offsets of the bf16 backward's padded edge operands in its first (M, d) fp32 buffer: d(out) and x as bf16 (M, Fp),
// W_out^T as bf16 (d, Fp), the padded fp32 gradients of W_out (Fp, d) and W_joint (d, Fp), the padded bias gradient.
struct hig_edge16_offsets { int64_t dout, x, wot, dwo, dwj, dbo, end; };
inline hig_edge16_offsets hig_edge16_layout(int64_t M, int64_t Fp, int d) {
  auto up256 = [](int64_t v) { return (v + 255) / 256 * 256; };
  hig_edge16_offsets e;
  e.dout = 0;
  e.x = e.dout + up256(M * Fp * 2);
  e.wot = e.x + up256(M * Fp * 2);
  e.dwo = e.wot + up256((int64_t)d * Fp * 2);
  e.dwj = e.dwo + up256(Fp * d * 4);
  e.dbo = e.dwj + up256((int64_t)d * Fp * 4);
  e.end = e.dbo + up256(Fp * 4);
  return e;
}
// linattn.hip: context build of G groups of H heads in one launch (the batched text side); 1 = shape not served
int hig_linattn_ctx_groups(const float* K, const float* V, int64_t ld, int32_t B, int32_t rows, int32_t H, int32_t G, int32_t hd,
                           float* A, int64_t a_gs, float* kstat, int64_t k_gs, hipStream_t st);
int hig_linattn_ctx16_groups(const void* K, const void* V, int64_t ld, int32_t B, int32_t rows, int32_t H, int32_t G, int32_t hd,
                             float* A, int64_t a_gs, float* kstat, int64_t k_gs, void* At16, int64_t at_gs, hipStream_t st);   // (linattn16.hip, bf16 rows)
// weight gradients dW = dC^T . act over >= 2048 rows, I and J multiples of 128, tiles x splits <= 256 (wgrad_wsp32.hip): writes
// the split-R slabs (+ per-split column sums of dC) of hig_gemm_launch(splits > 1); HIG_OK = launched, 1 = shape not served, < 0 = error
int hig_wgrad_wsp32_try(const hig_gemm_desc& g, int splits, float* slabs, int64_t slab, float* xsum, int64_t xsum_stride, hipStream_t st);
bool hig_gemm_wsp32_active();   // that kernel is switched on and the chip has the 256 CUs its work split is written for

// rowops.hip: fill / copy as kernels (never hipMemsetAsync / hipMemcpyAsync on a stream that may be under capture: see there)
int hig_zero_async(void* p, int64_t bytes, hipStream_t st);
int hig_copy_async(void* dst, const void* src, int64_t bytes, hipStream_t st);
// textrows.hip: hig_rows_segment_sum_f32 over the first *n_seg_dev of cap_seg segments (a count kept on the device)
int hig_rows_segment_sum_dev(const float* src, int32_t n_src, const int32_t* order, const int32_t* seg, int32_t cap_seg,
                             const int32_t* n_seg_dev, int64_t row_floats, float* dst, hig_stream_t stream);
// The capacity layout of the embedding index built on the device (include/hig.h, hig_clip_embed_index_build): int32 offsets of
// the seven arrays, a function of (B, N, vocab) only.  part_rows: the rows the chunk partials can take (n_chunks <= n_live <= M).
struct hig_clip_index_layout_t {
  int64_t M, cap_ids, cap_chunks, part_rows;
  int64_t order, chunk_seg, chunk_order, id_seg, ids, pos_order, pos_seg, total;
};
inline hig_clip_index_layout_t hig_clip_index_layout(int64_t B, int64_t N, int64_t vocab) {
  hig_clip_index_layout_t l;
  l.M = B * N;
  l.cap_ids = l.M < vocab ? l.M : vocab;
  l.cap_chunks = (l.M + HIG_CLIP_EMBED_CHUNK - 1) / HIG_CLIP_EMBED_CHUNK + l.cap_ids;
  l.part_rows = l.cap_chunks < l.M ? l.cap_chunks : l.M;
  l.order = 0;
  l.chunk_seg = l.order + l.M;
  l.chunk_order = l.chunk_seg + l.cap_chunks + 1;
  l.id_seg = l.chunk_order + l.cap_chunks;
  l.ids = l.id_seg + l.cap_ids + 1;
  l.pos_order = l.ids + l.cap_ids;
  l.pos_seg = l.pos_order + l.M;
  l.total = l.pos_seg + N + 1;
  return l;
}
// the buffer of hig_enc_bwd_debug_tap (texthead.hip; include/hig.h): NULL, 0 in every real run
void hig_enc_tap_buffer(float** buf, int64_t* bytes);

namespace {

inline int64_t al(int64_t floats) { return (floats + 63) & ~(int64_t)63; }  // 256-byte granules

struct G {  // small builder for gemm descriptors
  hig_gemm_desc g;
  G(const float* X, int64_t ldx, int xrs, const float* Y, int64_t ldy, int yrs, float* C, int64_t ldc,
    int64_t I, int64_t J, int64_t R) {
    memset(&g, 0, sizeof(g));
    g.X = X; g.ldx = ldx; g.x_rs = xrs; g.Y = Y; g.ldy = ldy; g.y_rs = yrs; g.C = C; g.ldc = ldc;
    g.I = (int)I; g.J = (int)J; g.R = (int)R;
    g.xf = HIG_XF_NONE; g.epi = HIG_EPI_NONE; g.prec = HIG_PREC_F32;
  }
  G& prec(int p) { g.prec = p; return *this; }  // forward products: HIG_PREC_* of the plan
  G& epi(int e, const float* bias = nullptr) { g.epi = e; g.bias = bias; return *this; }
  G& res(const float* r, int64_t ldr) { g.res = r; g.ldr = ldr; return *this; }
  G& aux(float* a, int64_t lda) { g.aux = a; g.ldaux = lda; return *this; }
  G& pos(const float* p, int64_t ldp, int T) { g.pos = p; g.ldpos = ldp; g.T = T; return *this; }
  G& silu(int on_y) { g.xf = HIG_XF_SILU; g.xf_on_y = on_y; return *this; }
  G& ln(int on_y, const float* stats, const float* gamma, const float* beta) {
    g.xf = HIG_XF_LN; g.xf_on_y = on_y; g.stats = stats; g.gamma = gamma; g.beta = beta; return *this;
  }
  G& xsum(float* out) { g.xcolsum = out; return *this; }   // wgrad: also the bias gradient (column sums of dC)
  G& mod(const float* ss, int64_t ss_ld, int shift_off, int rows_per_sample) {
    g.xf = HIG_XF_LN_MOD_SILU; g.ss = ss; g.ss_ld = ss_ld; g.ss_shift_off = shift_off;
    g.rows_per_sample = rows_per_sample; return *this;
  }
};

// Weight-gradient GEMMs (dW = dC^T . act over the M rows).  Tile: exact-fp32 products run 64x64 tiles (four resident
// workgroups per CU, 4x fewer split-R slabs to write and sum than with 128x128: forward+backward 20.6 -> 20.2 ms),
// the bf16 product modes 128x128 (14.9 vs 15.2 ms bf16x3, 12.9 vs 13.5 ms bf16) -- same-box sweeps in
// profiles/r01_notes.md.
inline int wgrad_tile(int64_t I, int64_t J, int prec) {
  if (!(I > 64 && J > 64)) return 64;
  return prec == HIG_PREC_F32 ? 64 : 128;
}

// Split the reduce range so that tiles x splits fills, but does not exceed, the workgroups that are resident at once
// (128x128: 2 per CU = 512, 64 KB of LDS each; 64x64: 4 per CU = 1024) -- one more would start a second, nearly empty
// round (768 in flight cost the training step 0.6 ms; profiles/r01_notes.md).
inline int wgrad_splits(int64_t I, int64_t J, int64_t R, int64_t slab_floats, int prec) {
  const int bi = wgrad_tile(I, J, prec);
  const int64_t tiles = ((I + bi - 1) / bi) * ((J + bi - 1) / bi);
  const int target = (bi == 128 ? 2 : 4) * hig_chip_cus();
  int64_t s = target / tiles;
  const int64_t maxs = R / 256 > 1 ? R / 256 : 1;
  if (s > maxs) s = maxs;
  while (s > 1 && s * (I * J + I) > slab_floats) --s;   // slabs + the per-split column sums of X behind them
  if ((I * J) % 4 != 0) s = 1;
  return (int)(s < 1 ? 1 : s);
}

}  // namespace

// rowops.hip: hig_ln_bwd_bf16 with the reductions of its partial table left to hig_ln_bwd16_reduce_batch (one launch for up to
// HIG_LN_RB_MAX calls; each call needs its own partial table until then)
struct hig_ln_reduce {
  const float* partial; int samples, nsplit, n;
  float* dgamma; float* dbeta;
  int shift_off; float* dss; int64_t dss_ld;       // dss == NULL: a plain LayerNorm (no modulation gradients)
  int nb_col, nb_dss;
};
constexpr int HIG_LN_RB_MAX = 8;
int hig_ln_bwd16_launch(const void* da, int64_t ldda, const void* x, int32_t x_f32, int64_t ldx, const float* gamma,
                        const float* beta, const float* ss, int64_t ss_ld, int32_t ss_shift_off, int32_t mod_silu,
                        const void* res, int64_t ldr, void* dx, int32_t dx_f32, int64_t lddx, int64_t rows, int32_t n,
                        int32_t rows_per_sample, float* dgamma, float* dbeta, float* dss, int64_t dss_ld,
                        float* partial, hig_stream_t stream, hig_ln_reduce* deferred);
int hig_ln_bwd16_reduce_batch(const hig_ln_reduce* entries, int n, hipStream_t st);
