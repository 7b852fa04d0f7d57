// Which kernel serves a GEMM call: hig_gemm16_plan (hig_gemm_bf16) and hig_gemm32_plan (hig_gemm / hig_gemm_ws).
//
// Host code only.  A plan is a pure function of the descriptor, the switches (hig_gemm_switches) and the chip's CU count:
// no HIP call, no error state, no launch counted, no operand pointer dereferenced (only their null-ness and alignment are
// read).  The entry points validate-and-plan here, then switch on plan.path into the launcher of the kernel's own file
// (hig_gemm16_launch, gemm_bf16.hip; gemm_dispatch, gemm.hip); the kernels, their launch_* templates and the measurements
// behind every threshold below stay in those files.  Every eligibility condition is one named predicate used from one place;
// where two kernels differ (the residual's alignment) the difference is a parameter.
#include <stdarg.h>
#include <stdio.h>

#include "gemm16_epi.h"
#include "hig_host.h"

namespace {

int env_int(const char* v, int dflt) { return v ? atoi(v) : dflt; }

hig_plan served(int path, int variant, int launches = 1) {
  hig_plan p;
  p.rc = HIG_OK; p.path = path; p.launches = launches; p.variant = variant; p.msg[0] = 0;
  return p;
}
hig_plan refused(int rc, const char* fmt, ...) {
  hig_plan p = served(-1, 0, 0);
  p.rc = rc;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(p.msg, sizeof(p.msg), fmt, ap);
  va_end(ap);
  return p;
}
#define PLAN_REQUIRE(cond, ...) do { if (!(cond)) return refused(HIG_EINVAL, __VA_ARGS__); } while (0)

// ---- the predicates ----
bool aligned(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }
// rows x ld elements stay below the 32-bit byte offsets of the weight-stationary kernels' DMA descriptors (2^31 bytes)
bool fits_offsets(int64_t rows, int64_t ld, int elem_bytes) { return rows <= 0 || ld <= ((1ll << 31) / elem_bytes - 1) / rows; }
// the weight-stationary kernels' work split is compiled for 8 XCDs x 32 CUs (block b -> XCD b & 7): another partitioning of
// the chip gets the tiled kernels, whose grids follow the CU count
bool ws_chip(int cus) { return cus == 256; }
template <int... E> bool epi_in(hig_epi_list<E...>, int epi) { return ((epi == E) || ...); }
// LayerNorm fold: a producer's rows are the consumer's X rows (J of the one = R of the other)
bool fold_producer(const hig_gemm16_desc& g) { return g.epi == HIG_EPI_BIAS_RES && g.J == g.R && !g.row_stats_in; }
bool fold_consumer(const hig_gemm16_desc& g) { return g.epi == HIG_EPI_BIAS && g.ln_colsum; }

// What the two bf16 weight-stationary kernels ask of the operands alike (NULL: served).  res_align: bytes the residual must
// be aligned to -- gemm_wsp16 reads it in 16-byte pieces, gemm_ws16 in 8-byte ones.
const char* ws16_operands(const hig_gemm16_desc& g, const hig_gemm_switches& sw, int cus, int res_align) {
  if (!ws_chip(cus)) return "the device does not report 256 compute units (8 XCDs x 32)";
  if (g.c_f32 || (g.res && g.res_f32)) return "fp32 output / residual";
  if (g.I < sw.ws_rows) return "too few rows";
  if (!(g.ldc % 8 == 0 && aligned(g.C, 16))) return "C not 16-byte aligned / ldc not a multiple of 8";
  if (!fits_offsets(g.I, g.ldx, 2) || !fits_offsets(g.J, g.ldy, 2) || (g.res && !fits_offsets(g.I, g.ldr, 2)) ||
      !fits_offsets(g.I, g.ldc, 2) || (g.aux && !fits_offsets(g.I, g.ldaux, 2)))
    return "operand beyond the 32-bit byte offsets of the DMA descriptors";
  if (epi_has_res(g.epi) && !(g.ldr % (res_align / 2) == 0 && aligned(g.res, res_align)))
    return res_align == 16 ? "residual not 16-byte aligned / ldr not a multiple of 8" : "residual not 8-byte aligned / ldr not a multiple of 4";
  return nullptr;
}

// gemm_wsp16.hip: K = 512, 128-column panels (at most 256), a forced gemm_ws16 variant switches it off.  -1: not served.
int wsp16_variant(const hig_gemm16_desc& g, const hig_gemm_switches& sw, int cus) {
  if (!sw.wsp16 || sw.ws_nwj || g.R != 512 || g.J % 128 != 0 || g.J / 128 > 256) return -1;
  if (ws16_operands(g, sw, cus, 16) || !epi_in(hig_epi16_all{}, g.epi)) return -1;
  if (g.aux && !(g.epi == HIG_EPI_BIAS_GELU && g.ldaux % 8 == 0 && aligned(g.aux, 16))) return -1;
  if ((g.row_stats_out && !fold_producer(g)) || (g.row_stats_in && !fold_consumer(g))) return -1;
  return HIG_WSP_VARIANT(g.row_stats_out ? 1 : g.row_stats_in ? 2 : 0, g.aux != nullptr);
}

// gemm_ws16.hip.  NULL: served, *nwj holds the variant: 8 = eight waves x 32 columns, 4 = four waves x 32 columns, 2 = four
// waves x 64 columns (256-column panels), 44 = four waves x 32 columns laid out for two workgroups per CU.
const char* ws16_variant(const hig_gemm16_desc& g, const hig_gemm_switches& sw, int cus, int* nwj_out) {
  if (!sw.ws16) return "the weight-stationary kernel is switched off (HIG_BF16_WS=0)";
  if (!(g.R == 256 || g.R == 512 || g.R == 1024)) return "reduce extent not in {256, 512, 1024}";
  if (const char* why = ws16_operands(g, sw, cus, 8)) return why;
  if (!epi_in(hig_epi16_all{}, g.epi)) return "epilogue not built for this kernel";
  const bool bias_only = g.epi == HIG_EPI_NONE || g.epi == HIG_EPI_BIAS;
  // columns per CU: the weight panel is fetched once per workgroup (cols x K x 2 bytes at the CU's ~30 B/clk), the X
  // rows once per panel -- the sum is smallest near cols = sqrt(M N / 256)
  // (measured, tools/gemm16_bench.py: the 8-wave variant wins for the wide bias-only launches -- q/k/v at M = 12 544: 28 us
  // against 38 -- ; with a GELU or residual epilogue it spills registers at 256 per wave and the 4-wave variant wins)
  int nwj = 8;
  if (g.R == 1024 || (int64_t)g.I * g.J < (int64_t)256 * 192 * 192 || !bias_only) nwj = 4;
  // GELU: every wave is bound by instruction issue (the erf arithmetic alone is 13 instructions per output, ~4 cycles
  // each from one wave); two 4-wave workgroups per CU put a second, independent wave on every SIMD: FFN linear1 at
  // M = 12 544 28.5 -> 25.2 us, at M = 6 272 17.2 -> 15.1 us
  if (g.epi == HIG_EPI_BIAS_GELU && g.R != 1024) nwj = 44;
  // residual epilogues at K = 512: two workgroups per CU from 8 192 rows up (same-call A/B, forward: B = 64 1.630 -> 1.613 ms,
  // B = 512 8.72 -> 8.55 ms; B = 32 1.056 -> 1.066: the 3-4 tiles of a workgroup there are too few to share a CU)
  if (epi_has_res(g.epi) && g.R == 512 && g.I >= 8192) nwj = 44;
  else if (g.row_stats_out) nwj = 4;            // (the statistics are per 128-column panel)
  const int f = sw.ws_nwj;                      // HIG_BF16_WS_NWJ: a variant is forced where it exists
  if (g.row_stats_out) { if (f == 44) nwj = 44; }
  else if (f == 4 || (f == 8 && g.R != 1024) || (f == 2 && g.R == 512) || (f == 44 && g.R != 1024)) nwj = f;
  if (nwj == 8 && (!bias_only || g.row_stats_in)) nwj = 4;   // (the 8-wave variant: bias-only epilogues, no fold consumer)
  if ((nwj == 8 || nwj == 2) && g.J % 256 != 0) nwj = 4;
  const int bn = (nwj == 4 || nwj == 44) ? 128 : 256;
  if (g.J % bn != 0) return "J not a multiple of 128";
  if (g.J / bn > 32) return "more than 32 column panels";
  *nwj_out = nwj;
  return nullptr;
}

// The few-row kernel (gemm_bf16.hip): I <= 64, J a multiple of 32 with at most 512 column blocks (beyond that the tiled
// kernel already has every CU busy), reduce range a multiple of 64 of at least 256.
bool fewrow16_serves(const hig_gemm16_desc& g, const hig_gemm_switches& sw) {
  return sw.fewrow16 && g.I <= 64 && g.J % 32 == 0 && g.J / 32 <= 512 && g.R % 64 == 0 && g.R >= 256 && epi_in(hig_epi16_fewrow{}, g.epi);
}

// Tile and DMA ring of the tiled bf16 kernel (measurements: launch16_tile, gemm_bf16.hip).  Every launch of this model is a
// short-K problem (K = 256 ... 2048): per-tile fixed costs (first DMA, epilogue) and the number of ROUNDS the tiles take on
// the chip decide, not the MFMA rate.  Candidates: 128 x 128 (2 resident workgroups per CU) and 64 x 128 (3 per CU).  Rule:
// estimated time = rounds x relative cost of one tile (fitted to tools/gemm16_bench.py at M = 6272 and 12544,
// profiles/r02_notes.md: a 64 x 128 tile costs 0.75 of a 128 x 128 one, not the 0.5 of its area -- it re-reads the same
// weight panel for half the rows).
int tiled16_variant(const hig_gemm16_desc& g, const hig_gemm_switches& sw, int cus) {
  auto tiles = [&](int bm, int bn) { return (((int64_t)g.I + bm - 1) / bm) * (((int64_t)g.J + bn - 1) / bn); };
  auto rounds = [](int64_t t, int slots) { return (t + slots - 1) / slots; };
  int rows = (sw.tile16 == 64 || sw.tile16 == 128) ? sw.tile16 : 0;   // HIG_BF16_TILE forces one
  if (!rows) {
    const int64_t t128 = tiles(128, 128);
    const double c128 = (double)rounds(t128, 2 * cus) * 1.0, c64 = (double)rounds(tiles(64, 128), 3 * cus) * 0.75;
    rows = 128;
    if (t128 < cus ? c64 <= c128 * 1.25 : c64 < c128) rows = 64;   // (first: too few big tiles to occupy the chip)
  }
  // ring shapes: 64 rows, three stages of BK 64 from K = 512 up; 128 rows, four stages of BK 32 from 8 192 rows up
  if (rows == 64 && g.R % 64 == 0 && g.R >= 512) return HIG_TILE16_VARIANT(64, 64, 3);
  if (rows == 128 && g.I >= 8192 && g.R >= 512) return HIG_TILE16_VARIANT(128, 32, 4);
  if (g.R % 64 == 0) return HIG_TILE16_VARIANT(rows, 64, 2);
  return HIG_TILE16_VARIANT(rows, 32, 3);
}

// ---- exact-fp32 entry ----
bool built32(const hig_gemm_desc& g) {
#define CASE(xrs, yrs, xfv, ony, epiv) \
  if (g.x_rs == xrs && g.y_rs == yrs && g.xf == xfv && (g.xf == HIG_XF_NONE || g.xf_on_y == ony) && g.epi == epiv) return true;
  HIG_GEMM32_COMBOS(CASE)
#undef CASE
  return false;
}

// gemm_wsp32.hip: K = 256 / 512 / 1024, reduce-contiguous 16-byte aligned operands, >= 2048 rows (below that a workgroup has
// < 4 tiles per segment to pay its weight phase with), 32 x (4 / (K / 256)) column panels in at most three power-of-two
// segments.  -1: not served.
int wsp32_variant(const hig_gemm_desc& g, const hig_gemm_switches& sw, int cus) {
  if (!sw.wsp32 || !ws_chip(cus)) return -1;
  if (g.prec != HIG_PREC_F32 || g.x_rs || g.y_rs || g.xf != HIG_XF_NONE || g.xcolsum) return -1;
  if (!(g.R == 256 || g.R == 512 || g.R == 1024) || g.I < 2048) return -1;
  const int bn = 32 * (4 / (g.R / 256));
  int seg_p0[HIG_P32_MAXSEG], seg_np[HIG_P32_MAXSEG];
  if (g.J % bn != 0 || g.J / bn > 256 || hig_wsp32_segments(g.J / bn, seg_p0, seg_np) < 0) return -1;
  auto operand = [&](const void* p, int64_t ld) { return p && ld % 4 == 0 && aligned(p, 16) && fits_offsets(g.I, ld, 4); };
  if (!(operand(g.X, g.ldx) && operand(g.C, g.ldc) && g.ldy % 4 == 0 && aligned(g.Y, 16) && fits_offsets(g.J, g.ldy, 4))) return -1;
  const bool has_bias = g.epi == HIG_EPI_BIAS || g.epi == HIG_EPI_BIAS_GELU || g.epi == HIG_EPI_BIAS_RES;
  const bool has_res = g.epi == HIG_EPI_BIAS_RES || g.epi == HIG_EPI_RES;
  const bool has_aux = g.epi == HIG_EPI_DGELU || (g.epi == HIG_EPI_BIAS_GELU && g.aux);
  if ((has_bias && !(g.bias && aligned(g.bias, 16))) || (has_res && !operand(g.res, g.ldr)) || (has_aux && !operand(g.aux, g.ldaux))) return -1;
  const bool folds = g.row_stats_out || g.row_stats_in;
  if (g.row_stats_out && !(g.R == 512 && g.epi == HIG_EPI_BIAS_RES && !g.row_stats_in && aligned(g.row_stats_out, 8))) return -1;
  if (g.row_stats_in && !(g.R == 512 && g.epi == HIG_EPI_BIAS && g.ln_colsum && aligned(g.row_stats_in, 16) && aligned(g.ln_colsum, 16))) return -1;
  // K = 256 (the text side's key/value projection, transformer.py:146,150): plain / bias epilogue only
  if (g.R == 256 ? (folds || g.aux || !(g.epi == HIG_EPI_NONE || g.epi == HIG_EPI_BIAS)) : !(has_bias || has_res || g.epi == HIG_EPI_NONE || g.epi == HIG_EPI_DGELU))
    return -1;
  return HIG_WSP_VARIANT(g.row_stats_out ? 1 : g.row_stats_in ? 2 : 0, g.epi == HIG_EPI_BIAS_GELU && g.aux);
}

// Tile of the tiled fp32 kernel for an unsplit launch: index into {128x128, 64x128, 128x64, 64x64} (measurements:
// launch_sized, gemm.hip).  fp32 MFMA is slow enough (64 cycles per 32x32x2) that every tile shape is MFMA-bound, so what
// matters is how evenly the tiles spread over the CUs: the shape with the smallest rounds x tile-area x overhead.
int tiled32_tile(const hig_gemm_desc& g, const hig_gemm_switches& sw, int cus) {
  if (g.x_rs) return wgrad_tile(g.I, g.J, g.prec) == 128 ? 0 : 3;   // weight-gradient layout: the rule of hig_host.h
  if (g.row_stats_out || g.row_stats_in) return 3;                  // the LayerNorm fold lives in the 64 x 64 tile's staged epilogue
  if (sw.tile32 >= 0) return sw.tile32 < 3 ? sw.tile32 : 3;         // HIG_GEMM_TILE
  auto tiles = [&](int bi, int bj) { return (((int64_t)g.I + bi - 1) / bi) * (((int64_t)g.J + bj - 1) / bj); };
  if (g.prec != HIG_PREC_F32) return tiles(128, 128) >= 300 ? 0 : 3;   // bf16 products: 128x128 once it occupies the chip
  if (tiles(64, 64) > cus) return 3;                                // exact fp32: 64x64 beyond one tile per CU
  struct Cand { int bi, bj; double ovh; };
  const Cand cands[4] = {{128, 128, 1.00}, {64, 128, 1.02}, {128, 64, 1.03}, {64, 64, 1.04}};
  int best = 0;
  double best_cost = 1e300;
  for (int c = 0; c < 4; ++c) {
    const double cost = (double)((tiles(cands[c].bi, cands[c].bj) + cus - 1) / cus) * cands[c].bi * cands[c].bj * cands[c].ovh;
    if (cost < best_cost) { best_cost = cost; best = c; }
  }
  return best;
}

// Split tail of the 64x64 tile (KArgs, gemm.hip): M = 12 544 leaves every GEMM of the model a last round that fills 12-37 % of
// the chip (N = 512: 1568 tiles = 6 x 256 + 32): cut those remainder tiles along the reduce range so that the last round
// costs 1/s of a tile.  Exact-fp32 products, whole rounds in front, reduce slices of >= 2 k-tiles.  1: no tail.
int tiled32_tail(const hig_gemm_desc& g, int tile, int64_t tail_ws_bytes, const hig_gemm_switches& sw, int cus) {
  const int64_t ntiles = (((int64_t)g.I + 63) / 64) * (((int64_t)g.J + 63) / 64);
  if (!sw.tail32 || tile != 3 || g.x_rs || !hig_gemm32_fast(g) || g.prec != HIG_PREC_F32 || tail_ws_bytes <= 0 || ntiles <= cus || ntiles % cus == 0)
    return 1;
  const int rem = (int)(ntiles % cus), nkt = g.R / 32;
  int s = 1;
  while (2 * s * rem <= cus && nkt % (2 * s) == 0 && nkt / (2 * s) >= 2) s *= 2;
  return (rem <= HIG_GEMM_TAIL_CNT_BYTES / 4 && (int64_t)rem * s * HIG_GEMM_TAIL_UNIT_BYTES <= tail_ws_bytes) ? s : 1;
}

}  // namespace

const hig_gemm_switches& hig_gemm_switch_values() {
  static const hig_gemm_switches sw = {
      env_int(getenv("HIG_BF16_WSP"), 1),        // 0: gemm_wsp16 off
      env_int(getenv("HIG_BF16_WS"), 1),         // 0: gemm_ws16 off
      env_int(getenv("HIG_BF16_WS_ROWS"), 2048), // rows from which the bf16 weight-stationary kernels serve
      env_int(getenv("HIG_BF16_WS_NWJ"), 0),     // 8 / 4 / 2 / 44: force that gemm_ws16 variant
      env_int(getenv("HIG_LNFOLD"), 1),          // 0: no LayerNorm fold in the bf16 forward
      env_int(getenv("HIG_LNFOLD1024"), 1),      // 0: none at d = 1024
      env_int(getenv("HIG_BF16_FEWROW"), 1),     // 0: the few-row kernel off
      env_int(getenv("HIG_BF16_TILE"), 0),       // 64 / 128: force the tiled bf16 kernel's tile rows
      env_int(getenv("HIG_F32_WSP"), 1),         // 0: gemm_wsp32 (and wgrad_wsp32) off
      env_int(getenv("HIG_GEMM_TILE"), -1),      // 0 .. 3: force the tiled fp32 kernel's tile
      env_int(getenv("HIG_GEMM_TAIL"), 1),       // 0: no split tail
      env_int(getenv("HIG_FEW_ROWS_SPLIT"), 1),  // 0: the few-row GEMMs unsplit
  };
  return sw;
}

bool hig_gemm_wsp32_active() { return hig_gemm_switch_values().wsp32 && ws_chip(hig_chip_cus()); }

hig_plan hig_gemm16_plan(const hig_gemm16_desc& g, const hig_gemm_switches& sw, int cus) {
  PLAN_REQUIRE(g.X && g.Y && g.C, "hig_gemm_bf16: null operand");
  PLAN_REQUIRE(g.I >= 0 && g.J >= 0 && g.R > 0, "hig_gemm_bf16: bad extent");
  if (g.I == 0 || g.J == 0) return served(-1, 0, 0);
  if (g.R % 32 != 0) return refused(HIG_EUNSUPPORTED, "hig_gemm_bf16: the reduce extent must be a multiple of 32 (got %d)", g.R);
  PLAN_REQUIRE(g.ldx % 8 == 0 && g.ldy % 8 == 0 && aligned(g.X, 16) && aligned(g.Y, 16),
               "hig_gemm_bf16: operands must be 16-byte aligned with leading dimensions that are multiples of 8");
  if (epi_has_bias(g.epi)) PLAN_REQUIRE(g.bias, "hig_gemm_bf16: epilogue %d needs a bias", g.epi);
  if (epi_has_res(g.epi)) PLAN_REQUIRE(g.res, "hig_gemm_bf16: epilogue %d needs `res`", g.epi);
  // many rows, K = 512: the weight-stationary kernel with specialised waves; only it writes `aux`
  const int wsp = wsp16_variant(g, sw, cus);
  if (wsp >= 0) return served(HIG_GEMM_PATH_WSP16, wsp);
  if (g.aux) return refused(HIG_EUNSUPPORTED, "hig_gemm_bf16: `aux` (pre-activation output) on a shape gemm_wsp16 does not serve");
  // many rows, short reduce range: the weight-stationary kernel.  Only these two implement the LayerNorm fold (the tiled /
  // few-row kernels know nothing of row_stats_* / ln_colsum: a producer would silently skip the statistics, a consumer would
  // multiply un-normalised rows by W'), so with fold operands a decline is an error.
  const bool fold = g.row_stats_out || g.row_stats_in;
  if (fold && !((g.R == 512 || g.R == 1024) && (g.row_stats_out ? fold_producer(g) : fold_consumer(g))))
    return refused(HIG_EUNSUPPORTED, "hig_gemm_bf16: LayerNorm-fold operands on a shape the weight-stationary kernel does not serve");
  int nwj = 0;
  const char* why = ws16_variant(g, sw, cus, &nwj);
  if (!why) return served(HIG_GEMM_PATH_WS16, HIG_WS16_VARIANT(nwj, g.row_stats_out ? 1 : g.row_stats_in ? 2 : 0));
  if (fold) return refused(HIG_EUNSUPPORTED, "hig_gemm_bf16: LayerNorm-fold operands, but %s", why);
  if (fewrow16_serves(g, sw)) return served(HIG_GEMM_PATH_FEWROW16, 0);
  if (!epi_in(hig_epi16_all{}, g.epi)) return refused(HIG_EUNSUPPORTED, "hig_gemm_bf16: epilogue %d not built", g.epi);
  return served(HIG_GEMM_PATH_TILED16, tiled16_variant(g, sw, cus));
}

hig_plan hig_gemm32_plan(const hig_gemm_desc& g, int64_t tail_ws_bytes, const hig_gemm_switches& sw, int cus) {
  PLAN_REQUIRE(g.X && g.Y && g.C, "hig_gemm: null operand");
  PLAN_REQUIRE(g.I >= 0 && g.J >= 0 && g.R >= 0, "hig_gemm: negative extent");
  if (g.I == 0 || g.J == 0) return served(-1, 0, 0);
  if (g.xf != HIG_XF_NONE) {
    // transformed operand: features must come in whole float4 quads
    const int nfeat = g.xf_on_y ? g.J : g.R;
    PLAN_REQUIRE(nfeat % 4 == 0, "hig_gemm: fused transform needs feature count %% 4 == 0 (got %d)", nfeat);
    if (g.xf != HIG_XF_SILU) PLAN_REQUIRE(g.stats && g.gamma && g.beta, "hig_gemm: LN transform needs stats/gamma/beta");
    if (g.xf == HIG_XF_LN_MOD_SILU) PLAN_REQUIRE(g.ss && g.rows_per_sample > 0, "hig_gemm: modulation needs ss");
  }
  if (g.xcolsum)
    PLAN_REQUIRE(g.x_rs == 1 && g.prec == HIG_PREC_F32 && g.I % 4 == 0 && (g.xf == HIG_XF_NONE || g.xf_on_y),
                 "hig_gemm: xcolsum needs a reduce-slow X operand, fp32 products, I %% 4 == 0");
  if (g.row_stats_out || g.row_stats_in) {   // LayerNorm fold: gemm_wsp32 and the LDS-staged epilogue of the 64-column tiles implement it
    const bool ok = g.x_rs == 0 && g.y_rs == 0 && g.xf == HIG_XF_NONE && g.J % 64 == 0 && g.R % 32 == 0 && g.ldc % 4 == 0 &&
                    g.ldx % 4 == 0 && g.ldy % 4 == 0 && aligned(g.X, 16) && aligned(g.Y, 16) && aligned(g.C, 16) && aligned(g.bias, 16) &&
                    (g.row_stats_out ? (g.epi == HIG_EPI_BIAS_RES && !g.row_stats_in && g.res && g.ldr % 4 == 0 && aligned(g.res, 16) && aligned(g.row_stats_out, 8))
                                     : (g.epi == HIG_EPI_BIAS && g.ln_colsum && g.R % 128 == 0 && aligned(g.row_stats_in, 16) && aligned(g.ln_colsum, 16)));
    if (!ok) return refused(HIG_EUNSUPPORTED, "hig_gemm: LayerNorm-fold operands on a launch that cannot apply them "
                                               "(needs reduce-contiguous aligned operands, J %% 64 == 0, EPI_BIAS_RES producer / EPI_BIAS consumer with R %% 128 == 0)");
  }
  // exact-fp32 products, K = 256 / 512 / 1024, many rows: the weight-stationary kernel with specialised waves
  const int wsp = wsp32_variant(g, sw, cus);
  if (wsp >= 0) return served(HIG_GEMM_PATH_WSP32, wsp);
  // K = 1536 / 2048 (the data gradient of the stacked q/k/v projection: dqkv (M, 3d) . Wqkv): that kernel's weight panel holds
  // at most K = 1024, so the reduce range goes through it in two passes (gemm_dispatch, gemm.hip: 153 us at M = 12 544 against
  // 197 us on the tiled kernel); the second pass has C as its residual and 64-column panels at most
  if (g.R > 1024 && g.R <= 2048 && g.J % 64 == 0 &&
      (g.epi == HIG_EPI_NONE || g.epi == HIG_EPI_RES || g.epi == HIG_EPI_BIAS || g.epi == HIG_EPI_BIAS_RES)) {
    hig_gemm_desc p1, p2;
    hig_gemm32_two_pass(g, &p1, &p2);
    const int v1 = wsp32_variant(p1, sw, cus);
    if (v1 >= 0 && wsp32_variant(p2, sw, cus) >= 0) return served(HIG_GEMM_PATH_WSP32, v1, 2);
  }
  if (!built32(g))
    return refused(HIG_EUNSUPPORTED, "hig_gemm: combination x_rs=%d y_rs=%d xf=%d on_y=%d epi=%d not built", g.x_rs, g.y_rs, g.xf, g.xf_on_y, g.epi);
  const int tile = tiled32_tile(g, sw, cus), tail = tiled32_tail(g, tile, tail_ws_bytes, sw, cus);
  return served(tail > 1 ? HIG_GEMM_PATH_TAIL32 : HIG_GEMM_PATH_TILED32, HIG_TILE32_VARIANT(tile, tail));
}

// Can a d-wide LayerNorm in front of the GEMMs over `rows` rows be folded into them in the bf16 forward (the producer of the
// rows writes their statistics, the consumers apply them)?  Yes where every launch of the fold plans onto a kernel that
// implements it: the producer (d x d, EPI_BIAS_RES, row_stats_out) and the consumers (q/k/v: J = 3 d, cross-attention query:
// J = d; EPI_BIAS, row_stats_in + ln_colsum), dense aligned operands.  HIG_LNFOLD=0: off; HIG_LNFOLD1024=0: off at d = 1024.
bool hig_gemm_ws16_lnfold_ok(int64_t rows, int d, const hig_gemm_switches& sw, int cus) {
  if (!sw.lnfold || (d == 1024 && !sw.lnfold1024) || rows <= 0 || rows > INT32_MAX || d <= 0 || d > (1 << 20)) return false;
  void* const some = reinterpret_cast<void*>((uintptr_t)4096);   // an aligned non-null address: plans read no operand
  auto on_fold_kernel = [&](int J, int epi, bool producer) {
    hig_gemm16_desc g;
    memset(&g, 0, sizeof(g));
    g.X = g.Y = g.res = some; g.C = some; g.bias = static_cast<const float*>(some);
    g.ldx = g.ldy = g.ldr = d; g.ldc = J;
    g.I = (int)rows; g.J = J; g.R = d; g.epi = epi;
    if (producer) g.row_stats_out = static_cast<float*>(some);
    else g.row_stats_in = g.ln_colsum = static_cast<const float*>(some);
    const hig_plan p = hig_gemm16_plan(g, sw, cus);
    return p.rc == HIG_OK && (p.path == HIG_GEMM_PATH_WSP16 || p.path == HIG_GEMM_PATH_WS16);
  };
  return on_fold_kernel(d, HIG_EPI_BIAS_RES, true) && on_fold_kernel(3 * d, HIG_EPI_BIAS, false) && on_fold_kernel(d, HIG_EPI_BIAS, false);
}
bool hig_gemm_ws16_lnfold_ok(int64_t rows, int d) { return hig_gemm_ws16_lnfold_ok(rows, d, hig_gemm_switch_values(), hig_chip_cus()); }

static int plan_out(const hig_plan& p, int32_t* path, int32_t* launches, int32_t* variant) {
  if (path) *path = p.path;
  if (launches) *launches = p.launches;
  if (variant) *variant = p.variant;
  return p.rc;
}
extern "C" int hig_gemm_bf16_plan(const hig_gemm16_desc* g, int32_t chip_cus, int32_t* path, int32_t* launches, int32_t* variant) {
  if (!g) return HIG_EINVAL;
  return plan_out(hig_gemm16_plan(*g, hig_gemm_switch_values(), chip_cus > 0 ? chip_cus : hig_chip_cus()), path, launches, variant);
}
extern "C" int hig_gemm_plan(const hig_gemm_desc* g, int32_t has_tail_scratch, int32_t chip_cus, int32_t* path, int32_t* launches, int32_t* variant) {
  if (!g) return HIG_EINVAL;
  return plan_out(hig_gemm32_plan(*g, has_tail_scratch ? HIG_GEMM_TAIL_BYTES - HIG_GEMM_TAIL_CNT_BYTES : 0, hig_gemm_switch_values(),
                                  chip_cus > 0 ? chip_cus : hig_chip_cus()), path, launches, variant);
}
extern "C" int hig_gemm_bf16_lnfold_plan(int64_t rows, int32_t d, int32_t chip_cus) {
  return hig_gemm_ws16_lnfold_ok(rows, d, hig_gemm_switch_values(), chip_cus > 0 ? chip_cus : hig_chip_cus()) ? 1 : 0;
}
