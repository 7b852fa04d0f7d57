// Launch sequences of the text head: text_pre_proj -> post-norm TransformerEncoder
// -> text_ln -> EOT gather -> text_proj.  Reference: MotionTransformer.__init__ / encode_text
// (codes/models/transformer.py:324-340, 389-397) over torch's nn.TransformerEncoderLayer
// (norm_first=False, activation "gelu", dropout 0):
//     x = norm1(x + out_proj(softmax(q k^T / sqrt(hd)) v));   x = norm2(x + linear2(gelu(linear1(x))))
// Host code only (kernels live in gemm / fullattn / rowops; the layer itself in enc_layers.h); hipGraph-capturable like the denoiser.
#include "hig_common.h"
#include "enc_layers.h"

namespace {

struct TDims {
  int B, N, W, Lt, H, ff, L, E, hd, prec, pre;
  int64_t M;
  EncShape enc() const { return {B, N, Lt, ff, H, hd}; }
};

int check_tdims(const hig_text_dims* p, const void* const* params, TDims& D) {
  HIG_REQUIRE(p, "null text dims");
  D.B = p->B; D.N = p->N; D.W = p->W; D.Lt = p->Lt; D.H = p->H; D.ff = p->ff; D.L = p->L; D.E = p->E;
  HIG_REQUIRE(D.B > 0 && D.N > 0 && D.W > 0 && D.Lt > 0 && D.H > 0 && D.ff > 0 && D.L > 0 && D.E > 0,
              "hig_text_dims: every extent must be positive");
  HIG_REQUIRE(D.Lt % D.H == 0, "hig_text_dims: Lt=%d not divisible by H=%d", D.Lt, D.H);
  D.hd = D.Lt / D.H;
  HIG_TRY(hig_enc_check_hd("hig text head", D.hd));
  HIG_REQUIRE(D.Lt % 4 == 0 && D.W % 4 == 0 && D.ff % 4 == 0 && D.E % 4 == 0 && D.Lt <= 1024,
              "hig_text_dims: W, Lt, ff, E must be multiples of 4 and Lt <= 1024");
  HIG_TRY(hig_enc_check_prec(p->prec));
  D.prec = p->prec;
  D.pre = 1;
  if (params) {
    D.pre = params[HIG_T_PRE_W] != nullptr;
    HIG_REQUIRE(D.pre || D.W == D.Lt, "hig text head: identity text_pre_proj needs W == Lt");
  }
  D.M = (int64_t)D.B * D.N;
  return HIG_OK;
}

// Forward workspace (floats) by HIG_TFW_* slot; the per-layer block is repeated L times when training.
using TFwd = std::array<int64_t, HIG_TFW_NSLOTS>;
TFwd tfwd_layout(const TDims& D, int training) {
  TFwd w;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += al(n); return r; };
  w[HIG_TFW_X0] = take(D.M * D.Lt);
  w[HIG_TFW_GATH] = take((int64_t)D.B * D.Lt);
  w[HIG_TFW_STF] = take(D.M * 2);
  w[HIG_TFW_LAYER0] = o;
  o = 0;
  hig_enc_block_layout(take, &w[HIG_TFW_QKV], D.enc());
  w[HIG_TFW_LSTRIDE] = training ? o : 0;
  // inference ping-pongs x2 between two blocks so a layer never overwrites its own input
  w[HIG_TFW_TOTAL] = w[HIG_TFW_LAYER0] + (training ? o * D.L : 2 * o);
  return w;
}

// Backward workspace (floats) by HIG_TBW_* slot.
using TBwd = std::array<int64_t, HIG_TBW_NSLOTS>;
constexpr EncScratchSlots TBW_SCRATCH = {HIG_TBW_DFF,   HIG_TBW_DQKV,        HIG_TBW_DELTA,   HIG_TBW_WT,    HIG_TBW_TA, HIG_TBW_TB,
                                         HIG_TBW_SLABS, HIG_TBW_SLAB_FLOATS, HIG_TBW_COLPART, HIG_TBW_LNPART};
TBwd tbwd_layout(const TDims& D) {
  TBwd w;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += al(n); return r; };
  w[HIG_TBW_DA] = take(D.M * D.Lt);
  w[HIG_TBW_DB] = take(D.M * D.Lt);
  w[HIG_TBW_DC] = take(D.M * D.Lt);
  hig_enc_scratch_grads(take, w.data(), TBW_SCRATCH, D.enc());
  w[HIG_TBW_DGATH] = take((int64_t)D.B * D.Lt);
  int64_t big = (int64_t)3 * D.Lt * D.Lt;
  for (int64_t v : {(int64_t)D.ff * D.Lt, (int64_t)D.Lt * D.W, (int64_t)D.E * D.Lt}) big = v > big ? v : big;
  const int64_t wide = 3 * D.Lt > D.ff ? 3 * D.Lt : D.ff;
  hig_enc_scratch_work(take, w.data(), TBW_SCRATCH, D.enc(), big, {{D.M, 3 * D.Lt}, {D.M, D.ff}, {D.B, D.E}}, wide * D.M,
                       (int64_t)(D.ff > D.W ? D.ff : D.W) * D.M);
  w[HIG_TBW_TOTAL] = o;
  return w;
}

float* g_enc_tap = nullptr;           // diagnostic only (hig_enc_bwd_debug_tap): NULL in every real run
int64_t g_enc_tap_bytes = 0;

}  // namespace

// ---- test hooks (include/hig.h): the two layouts above and the tap's, by named slot; the tap buffer of both backwards ----
void hig_enc_tap_buffer(float** buf, int64_t* bytes) { *buf = g_enc_tap; *bytes = g_enc_tap_bytes; }
extern "C" int hig_enc_bwd_debug_tap(void* buf, int64_t bytes) {
  if (buf && bytes <= 0) return hig_set_error(HIG_EINVAL, "hig_enc_bwd_debug_tap: a tap buffer of %lld bytes", (long long)bytes);
  g_enc_tap = static_cast<float*>(buf);
  g_enc_tap_bytes = buf ? bytes : 0;
  return HIG_OK;
}
extern "C" int64_t hig_text_head_bwd_tap_bytes(const hig_text_dims* dims) {
  TDims D;
  if (check_tdims(dims, nullptr, D) != HIG_OK) return HIG_EINVAL;
  return hig_enc_tap_layout(true, D.enc(), D.L).off[HIG_ETAP_TOTAL] * 4;
}
extern "C" int hig_text_head_layout(const hig_text_dims* dims, int32_t which, int64_t* out, int32_t n_out) {
  TDims D;
  if (check_tdims(dims, nullptr, D) != HIG_OK) return HIG_EINVAL;   // (the message is check_tdims's)
  if (which == HIG_ENC_LAYOUT_FWD) return hig_enc_publish(tfwd_layout(D, 1).data(), HIG_TFW_NSLOTS, out, n_out);
  if (which == HIG_ENC_LAYOUT_BWD) return hig_enc_publish(tbwd_layout(D).data(), HIG_TBW_NSLOTS, out, n_out);
  if (which == HIG_ENC_LAYOUT_TAP) return hig_enc_publish(hig_enc_tap_layout(true, D.enc(), D.L).off, HIG_ETAP_NSLOTS, out, n_out);
  return hig_set_error(HIG_EINVAL, "hig_text_head_layout: no layout table %d", which);
}

extern "C" int64_t hig_text_head_workspace_bytes(const hig_text_dims* dims, int training) {
  TDims D;
  if (check_tdims(dims, nullptr, D) != HIG_OK) return -1;
  return tfwd_layout(D, training)[HIG_TFW_TOTAL] * 4;
}
extern "C" int64_t hig_text_head_bwd_workspace_bytes(const hig_text_dims* dims) {
  TDims D;
  if (check_tdims(dims, nullptr, D) != HIG_OK) return -1;
  return tbwd_layout(D)[HIG_TBW_TOTAL] * 4;
}

extern "C" int hig_text_head_fwd(const hig_text_dims* dims, const void* const* params, const float* clip_out,
                                 const int64_t* eot, float* xf_out, float* xf_proj, void* workspace,
                                 int training, hig_stream_t stream) {
  TDims D;
  HIG_REQUIRE(params, "hig_text_head_fwd: null params");
  HIG_TRY(check_tdims(dims, params, D));
  HIG_REQUIRE(clip_out && eot && xf_out && xf_proj && workspace, "hig_text_head_fwd: null argument");
  const TFwd w = tfwd_layout(D, training);
  const Tab P(params, HIG_T_NGLOBAL, HIG_TL_NLAYER);
  float* ws = static_cast<float*>(workspace);
  hipStream_t st = hig_stream(stream);
  const int Lt = D.Lt;
  const int64_t M = D.M;
  const int64_t blk = w[HIG_TFW_TOTAL] - w[HIG_TFW_LAYER0];  // inference: two half blocks
  const float* xin = clip_out;
  if (D.pre) {
    HIG_TRY(hig_gemm_launch(G(clip_out, D.W, 0, P[HIG_T_PRE_W], D.W, 0, ws + w[HIG_TFW_X0], Lt, M, Lt, D.W)
                                .epi(HIG_EPI_BIAS, P[HIG_T_PRE_B]).prec(D.prec).g, 1, nullptr, st));
    xin = ws + w[HIG_TFW_X0];
  }
  for (int l = 0; l < D.L; ++l) {
    float* lb = ws + w[HIG_TFW_LAYER0] + (training ? w[HIG_TFW_LSTRIDE] * l : (l & 1) * (blk / 2));
    const EncLayer a = hig_enc_block_at(lb, &w[HIG_TFW_QKV], training != 0);   // (the GELU pre-activation z: kept when training)
    HIG_TRY(hig_enc_layer_fwd(D.enc(), P.layer(l), a, xin, nullptr, D.prec, stream));
    xin = a.x2;
  }
  HIG_TRY(hig_layernorm(xin, Lt, M, Lt, P[HIG_T_LN_W], P[HIG_T_LN_B], xf_out, Lt, ws + w[HIG_TFW_STF], stream));
  HIG_TRY(hig_gather_rows(xf_out, Lt, D.B, D.N, eot, Lt, ws + w[HIG_TFW_GATH], Lt, stream));
  HIG_TRY(hig_gemm_launch(G(ws + w[HIG_TFW_GATH], Lt, 0, P[HIG_T_PROJ_W], Lt, 0, xf_proj, D.E, D.B, D.E, Lt)
                              .epi(HIG_EPI_BIAS, P[HIG_T_PROJ_B]).g, 1, nullptr, st));
  return HIG_OK;
}

extern "C" int hig_text_head_bwd(const hig_text_dims* dims, const void* const* params, const float* clip_out,
                                 const int64_t* eot, const float* xf_out, const void* workspace,
                                 const float* dxf_out, const float* dxf_proj, void* const* grads, float* dclip,
                                 void* bwd_workspace, hig_stream_t stream) {
  (void)xf_out;
  TDims D;
  HIG_REQUIRE(params, "hig_text_head_bwd: null params");
  HIG_TRY(check_tdims(dims, params, D));
  HIG_REQUIRE(clip_out && eot && workspace && grads && bwd_workspace, "hig_text_head_bwd: null argument");
  const TFwd w = tfwd_layout(D, 1);
  const TBwd bw = tbwd_layout(D);
  const Tab P(params, HIG_T_NGLOBAL, HIG_TL_NLAYER);
  const Tab Gr(grads, HIG_T_NGLOBAL, HIG_TL_NLAYER);
  const float* ws = static_cast<const float*>(workspace);
  float* b = static_cast<float*>(bwd_workspace);
  hipStream_t st = hig_stream(stream);
  const int Lt = D.Lt, E = D.E;
  const int64_t M = D.M;
  EncBwd e(D.enc(), D.prec, b, bw.data(), TBW_SCRATCH, stream);
  HIG_TRY(e.tap_begin(true, D.L, "hig_text_head_bwd"));
  float* lnp = e.lnp;

  float* dA = b + bw[HIG_TBW_DA];
  float* dB = b + bw[HIG_TBW_DB];
  float* dC = b + bw[HIG_TBW_DC];
  float* dgath = b + bw[HIG_TBW_DGATH];
  const float* gath = ws + w[HIG_TFW_GATH];
  // ---- d(xf_out) total = upstream + scatter of d(text_proj input) at the EOT rows -------------
  if (dxf_out) {
    HIG_TRY(hig_copy_async(dA, dxf_out, (size_t)M * Lt * 4, st));
  } else {
    HIG_TRY(hig_zero_async(dA, (size_t)M * Lt * 4, st));
  }
  if (dxf_proj) {
    HIG_TRY(e.colsum(dxf_proj, E, D.B, E, Gr[HIG_T_PROJ_B]));
    HIG_TRY(hig_gemm_launch(G(dxf_proj, E, 1, gath, Lt, 1, Gr[HIG_T_PROJ_W], Lt, E, Lt, D.B).g, 1, nullptr, st));
    HIG_TRY(hig_gemm_launch(G(dxf_proj, E, 0, P[HIG_T_PROJ_W], Lt, 1, dgath, Lt, D.B, Lt, E).g, 1, nullptr, st));
    HIG_TRY(e.tap_copy(HIG_ETAP_DGATH, -1, dgath));
    HIG_TRY(hig_scatter_add_rows(dgath, Lt, D.B, D.N, eot, Lt, dA, Lt, stream));
  } else {
    HIG_TRY(hig_zero_async(Gr[HIG_T_PROJ_B], (size_t)E * 4, st));
    HIG_TRY(hig_zero_async(Gr[HIG_T_PROJ_W], (size_t)E * Lt * 4, st));
  }
  HIG_TRY(e.tap_copy(HIG_ETAP_DXF_TOTAL, -1, dA));
  // ---- text_ln ---------------------------------------------------------------------------
  auto layer = [&](int l) { return hig_enc_block_at(ws + w[HIG_TFW_LAYER0] + w[HIG_TFW_LSTRIDE] * l, &w[HIG_TFW_QKV]); };
  HIG_TRY(hig_ln_bwd(dA, Lt, layer(D.L - 1).x2, Lt, ws + w[HIG_TFW_STF], P[HIG_T_LN_W], P[HIG_T_LN_B], nullptr, 0, 0, 0,
                     nullptr, 0, dB, Lt, M, Lt, D.N, Gr[HIG_T_LN_W], Gr[HIG_T_LN_B], nullptr, 0, lnp, stream));
  float* d = dB;      // d(x2 of layer l)
  float* t1 = dA;     // scratch (M, Lt)
  float* t2 = dC;
  for (int l = D.L - 1; l >= 0; --l) {
    const float* xin = l == 0 ? (D.pre ? ws + w[HIG_TFW_X0] : clip_out) : layer(l - 1).x2;
    HIG_TRY(hig_enc_layer_bwd(e, l, P.layer(l), Gr.layer(l), layer(l), xin, nullptr, d, t1, t2));
  }
  // ---- text_pre_proj -----------------------------------------------------------------------
  if (D.pre) {
    HIG_TRY(e.wgrad_act(d, Lt, clip_out, D.W, Gr[HIG_T_PRE_W], M, Gr[HIG_T_PRE_B]));
    if (dclip) HIG_TRY(e.dgrad(d, P[HIG_T_PRE_W], Lt, D.W, M, dclip, HIG_EPI_NONE, nullptr, nullptr));
  } else if (dclip) {
    HIG_TRY(hig_copy_async(dclip, d, (size_t)M * Lt * 4, st));
  }
  return HIG_OK;
}
