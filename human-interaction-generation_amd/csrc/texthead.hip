// Launch sequences of the text head: text_pre_proj -> post-norm TransformerEncoder
// -> text_ln -> EOT gather -> text_proj.  Reference: MotionTransformer.__init__ / encode_text
// (codes/models/transformer.py:324-340, 389-397) over torch's nn.TransformerEncoderLayer
// (norm_first=False, activation "gelu", dropout 0):
//     x = norm1(x + out_proj(softmax(q k^T / sqrt(hd)) v));   x = norm2(x + linear2(gelu(linear1(x))))
// Host code only (kernels live in gemm / fullattn / rowops); hipGraph-capturable like the denoiser.
#include "hig_common.h"
#include "hig_host.h"

namespace {

struct TDims {
  int B, N, W, Lt, H, ff, L, E, hd, prec, pre;
  int64_t M;
};

int check_tdims(const hig_text_dims* p, const void* const* params, TDims& D) {
  HIG_REQUIRE(p, "null text dims");
  D.B = p->B; D.N = p->N; D.W = p->W; D.Lt = p->Lt; D.H = p->H; D.ff = p->ff; D.L = p->L; D.E = p->E;
  HIG_REQUIRE(D.B > 0 && D.N > 0 && D.W > 0 && D.Lt > 0 && D.H > 0 && D.ff > 0 && D.L > 0 && D.E > 0,
              "hig_text_dims: every extent must be positive");
  HIG_REQUIRE(D.Lt % D.H == 0, "hig_text_dims: Lt=%d not divisible by H=%d", D.Lt, D.H);
  D.hd = D.Lt / D.H;
  if (!(D.hd == 8 || D.hd == 16 || D.hd == 32 || D.hd == 64 || D.hd == 128))
    return hig_set_error(HIG_EUNSUPPORTED, "hig text head: head dim %d not in {8,16,32,64,128}", D.hd);
  HIG_REQUIRE(D.Lt % 4 == 0 && D.W % 4 == 0 && D.ff % 4 == 0 && D.E % 4 == 0 && D.Lt <= 1024,
              "hig_text_dims: W, Lt, ff, E must be multiples of 4 and Lt <= 1024");
  if (p->prec != HIG_PREC_F32 && p->prec != HIG_PREC_BF16X3 && p->prec != HIG_PREC_BF16)
    return hig_set_error(HIG_EINVAL, "hig: unknown prec=%d", p->prec);
  D.prec = p->prec;
  D.pre = 1;
  if (params) {
    D.pre = params[HIG_T_PRE_W] != nullptr;
    HIG_REQUIRE(D.pre || D.W == D.Lt, "hig text head: identity text_pre_proj needs W == Lt");
  }
  D.M = (int64_t)D.B * D.N;
  return HIG_OK;
}

// Forward workspace (floats); the per-layer block is repeated L times when training.
struct TFwd {
  int64_t x0, gath, stf, layer0, lstride;
  int64_t qkv, lse, att, r1, st1, x1, z, f, r2, st2, x2;
  int64_t total;
};
TFwd tfwd_layout(const TDims& D, int training) {
  TFwd w;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += al(n); return r; };
  w.x0 = take(D.M * D.Lt);
  w.gath = take((int64_t)D.B * D.Lt);
  w.stf = take(D.M * 2);
  w.layer0 = o;
  o = 0;
  w.qkv = take(D.M * 3 * D.Lt);
  w.lse = take((int64_t)D.B * D.H * D.N);
  w.att = take(D.M * D.Lt);
  w.r1 = take(D.M * D.Lt);
  w.st1 = take(D.M * 2);
  w.x1 = take(D.M * D.Lt);
  w.z = take(D.M * D.ff);
  w.f = take(D.M * D.ff);
  w.r2 = take(D.M * D.Lt);
  w.st2 = take(D.M * 2);
  w.x2 = take(D.M * D.Lt);
  w.lstride = training ? o : 0;
  // inference ping-pongs x2 between two blocks so a layer never overwrites its own input
  w.total = w.layer0 + (training ? o * D.L : 2 * o);
  return w;
}

struct TBwd {
  int64_t dA, dB, dC, dff, dqkv, delta, dgath, wT, tA, tB, slabs, slab_floats, colpart, lnpart, total;
};
TBwd tbwd_layout(const TDims& D) {
  TBwd w;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += al(n); return r; };
  w.dA = take(D.M * D.Lt);
  w.dB = take(D.M * D.Lt);
  w.dC = take(D.M * D.Lt);
  w.dff = take(D.M * D.ff);
  w.dqkv = take(D.M * 3 * D.Lt);
  w.delta = take((int64_t)D.B * D.H * D.N);
  w.dgath = take((int64_t)D.B * D.Lt);
  int64_t big = (int64_t)3 * D.Lt * D.Lt;
  const int64_t outs[] = {(int64_t)D.ff * D.Lt, (int64_t)D.Lt * D.W, (int64_t)D.E * D.Lt};
  for (int64_t v : outs) big = v > big ? v : big;
  w.wT = take(big);
  const int64_t wide = 3 * D.Lt > D.ff ? 3 * D.Lt : D.ff;
  w.tA = take(wide * D.M);
  w.tB = take((int64_t)(D.ff > D.W ? D.ff : D.W) * D.M);
  w.slab_floats = big * 16 > (int64_t)1536 * 128 * 128 ? big * 16 : (int64_t)1536 * 128 * 128;
  w.slabs = take(w.slab_floats);
  int64_t colp = 0;
  const int64_t uses[][2] = {{D.M, 3 * D.Lt}, {D.M, D.ff}, {D.B, D.E}};
  for (auto& u : uses) {
    const int64_t v = (int64_t)hig_colsum_chunks(u[0]) * u[1];
    colp = v > colp ? v : colp;
  }
  w.colpart = take(colp);
  w.lnpart = take(hig_ln_bwd_partial_floats(D.M, D.Lt, D.N));
  w.total = o;
  return w;
}

inline const float* TP(const void* const* t, int idx) { return static_cast<const float*>(t[idx]); }
inline const float* TPL(const void* const* t, int l, int idx) {
  return static_cast<const float*>(t[HIG_T_NGLOBAL + l * HIG_TL_NLAYER + idx]);
}
inline float* TG(void* const* t, int idx) { return static_cast<float*>(t[idx]); }
inline float* TGL(void* const* t, int l, int idx) {
  return static_cast<float*>(t[HIG_T_NGLOBAL + l * HIG_TL_NLAYER + idx]);
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
  return hig_enc_tap_layout(true, D.B, D.N, D.Lt, D.ff, D.H, D.L).off[HIG_ETAP_TOTAL] * 4;
}
extern "C" int hig_text_head_layout(const hig_text_dims* dims, int32_t which, int64_t* out, int32_t n_out) {
  TDims D;
  if (check_tdims(dims, nullptr, D) != HIG_OK) return HIG_EINVAL;   // (the message is check_tdims's)
  int64_t v[HIG_TFW_NSLOTS > HIG_TBW_NSLOTS ? HIG_TFW_NSLOTS : HIG_TBW_NSLOTS];
  static_assert(HIG_ETAP_NSLOTS <= HIG_TFW_NSLOTS, "v holds the longest table");
  int n = 0;
  if (which == HIG_ENC_LAYOUT_FWD) {
    const TFwd w = tfwd_layout(D, 1);
    n = HIG_TFW_NSLOTS;
    v[HIG_TFW_X0] = w.x0; v[HIG_TFW_GATH] = w.gath; v[HIG_TFW_STF] = w.stf; v[HIG_TFW_LAYER0] = w.layer0; v[HIG_TFW_LSTRIDE] = w.lstride;
    v[HIG_TFW_QKV] = w.qkv; v[HIG_TFW_LSE] = w.lse; v[HIG_TFW_ATT] = w.att; v[HIG_TFW_R1] = w.r1; v[HIG_TFW_ST1] = w.st1; v[HIG_TFW_X1] = w.x1;
    v[HIG_TFW_Z] = w.z; v[HIG_TFW_F] = w.f; v[HIG_TFW_R2] = w.r2; v[HIG_TFW_ST2] = w.st2; v[HIG_TFW_X2] = w.x2; v[HIG_TFW_TOTAL] = w.total;
  } else if (which == HIG_ENC_LAYOUT_BWD) {
    const TBwd w = tbwd_layout(D);
    n = HIG_TBW_NSLOTS;
    v[HIG_TBW_DA] = w.dA; v[HIG_TBW_DB] = w.dB; v[HIG_TBW_DC] = w.dC; v[HIG_TBW_DFF] = w.dff; v[HIG_TBW_DQKV] = w.dqkv; v[HIG_TBW_DELTA] = w.delta;
    v[HIG_TBW_DGATH] = w.dgath; v[HIG_TBW_WT] = w.wT; v[HIG_TBW_TA] = w.tA; v[HIG_TBW_TB] = w.tB; v[HIG_TBW_SLABS] = w.slabs;
    v[HIG_TBW_SLAB_FLOATS] = w.slab_floats; v[HIG_TBW_COLPART] = w.colpart; v[HIG_TBW_LNPART] = w.lnpart; v[HIG_TBW_TOTAL] = w.total;
  } else if (which == HIG_ENC_LAYOUT_TAP) {
    const EncTap t = hig_enc_tap_layout(true, D.B, D.N, D.Lt, D.ff, D.H, D.L);
    n = HIG_ETAP_NSLOTS;
    for (int s = 0; s < HIG_ETAP_NSLOTS; ++s) v[s] = t.off[s];
  } else {
    return hig_set_error(HIG_EINVAL, "hig_text_head_layout: no layout table %d", which);
  }
  for (int s = 0; out && s < n && s < n_out; ++s) out[s] = v[s];
  return n;
}

extern "C" int64_t hig_text_head_workspace_bytes(const hig_text_dims* dims, int training) {
  TDims D;
  if (check_tdims(dims, nullptr, D) != HIG_OK) return -1;
  return tfwd_layout(D, training).total * 4;
}
extern "C" int64_t hig_text_head_bwd_workspace_bytes(const hig_text_dims* dims) {
  TDims D;
  if (check_tdims(dims, nullptr, D) != HIG_OK) return -1;
  return tbwd_layout(D).total * 4;
}

extern "C" int hig_text_head_fwd(const hig_text_dims* dims, const void* const* params, const float* clip_out,
                                 const int64_t* eot, float* xf_out, float* xf_proj, void* workspace,
                                 int training, hig_stream_t stream) {
  TDims D;
  HIG_REQUIRE(params, "hig_text_head_fwd: null params");
  HIG_TRY(check_tdims(dims, params, D));
  HIG_REQUIRE(clip_out && eot && xf_out && xf_proj && workspace, "hig_text_head_fwd: null argument");
  const TFwd w = tfwd_layout(D, training);
  float* ws = static_cast<float*>(workspace);
  hipStream_t st = hig_stream(stream);
  const int Lt = D.Lt, ff = D.ff;
  const int64_t M = D.M;
  const int64_t blk = w.total - w.layer0;  // inference: two half blocks
  const float* xin = clip_out;
  if (D.pre) {
    HIG_TRY(hig_gemm_launch(G(clip_out, D.W, 0, TP(params, HIG_T_PRE_W), D.W, 0, ws + w.x0, Lt, M, Lt, D.W)
                                .epi(HIG_EPI_BIAS, TP(params, HIG_T_PRE_B)).prec(D.prec).g, 1, nullptr, st));
    xin = ws + w.x0;
  }
  for (int l = 0; l < D.L; ++l) {
    float* lb = ws + w.layer0 + (training ? w.lstride * l : (l & 1) * (blk / 2));
    HIG_TRY(hig_gemm_launch(G(xin, Lt, 0, TPL(params, l, HIG_TL_IN_W), Lt, 0, lb + w.qkv, 3 * Lt, M, 3 * Lt, Lt)
                                .epi(HIG_EPI_BIAS, TPL(params, l, HIG_TL_IN_B)).prec(D.prec).g, 1, nullptr, st));
    HIG_TRY(hig_fullattn_fwd(lb + w.qkv, 3 * Lt, lb + w.qkv + Lt, lb + w.qkv + 2 * Lt, 3 * Lt, D.B, D.N, D.N, D.H, D.hd,
                             nullptr, lb + w.att, Lt, lb + w.lse, stream));
    HIG_TRY(hig_gemm_launch(G(lb + w.att, Lt, 0, TPL(params, l, HIG_TL_OUT_W), Lt, 0, lb + w.r1, Lt, M, Lt, Lt)
                                .epi(HIG_EPI_BIAS_RES, TPL(params, l, HIG_TL_OUT_B)).res(xin, Lt).prec(D.prec).g,
                            1, nullptr, st));
    HIG_TRY(hig_layernorm(lb + w.r1, Lt, M, Lt, TPL(params, l, HIG_TL_N1_W), TPL(params, l, HIG_TL_N1_B), lb + w.x1, Lt,
                          lb + w.st1, stream));
    HIG_TRY(hig_gemm_launch(G(lb + w.x1, Lt, 0, TPL(params, l, HIG_TL_FF1_W), Lt, 0, lb + w.f, ff, M, ff, Lt)
                                .epi(HIG_EPI_BIAS_GELU, TPL(params, l, HIG_TL_FF1_B))
                                .aux(training ? lb + w.z : nullptr, ff).prec(D.prec).g, 1, nullptr, st));
    HIG_TRY(hig_gemm_launch(G(lb + w.f, ff, 0, TPL(params, l, HIG_TL_FF2_W), ff, 0, lb + w.r2, Lt, M, Lt, ff)
                                .epi(HIG_EPI_BIAS_RES, TPL(params, l, HIG_TL_FF2_B)).res(lb + w.x1, Lt).prec(D.prec).g,
                            1, nullptr, st));
    HIG_TRY(hig_layernorm(lb + w.r2, Lt, M, Lt, TPL(params, l, HIG_TL_N2_W), TPL(params, l, HIG_TL_N2_B), lb + w.x2, Lt,
                          lb + w.st2, stream));
    xin = lb + w.x2;
  }
  HIG_TRY(hig_layernorm(xin, Lt, M, Lt, TP(params, HIG_T_LN_W), TP(params, HIG_T_LN_B), xf_out, Lt, ws + w.stf, stream));
  HIG_TRY(hig_gather_rows(xf_out, Lt, D.B, D.N, eot, Lt, ws + w.gath, Lt, stream));
  HIG_TRY(hig_gemm_launch(G(ws + w.gath, Lt, 0, TP(params, HIG_T_PROJ_W), Lt, 0, xf_proj, D.E, D.B, D.E, Lt)
                              .epi(HIG_EPI_BIAS, TP(params, HIG_T_PROJ_B)).g, 1, nullptr, st));
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
  const float* ws = static_cast<const float*>(workspace);
  float* b = static_cast<float*>(bwd_workspace);
  hipStream_t st = hig_stream(stream);
  const int Lt = D.Lt, ff = D.ff, E = D.E;
  const int64_t M = D.M;
  EncBwd e;
  e.B = D.B; e.S = D.N; e.n = Lt; e.ff = ff; e.H = D.H; e.hd = D.hd; e.prec = D.prec; e.M = M;
  e.slabs = b + bw.slabs; e.slab_floats = bw.slab_floats;
  e.colp = b + bw.colpart; e.lnp = b + bw.lnpart; e.wT = b + bw.wT; e.tA = b + bw.tA; e.tB = b + bw.tB;
  e.dff = b + bw.dff; e.dqkv = b + bw.dqkv; e.delta = b + bw.delta;
  e.stream = stream;
  HIG_TRY(e.tap_begin(true, D.L, "hig_text_head_bwd"));
  float* lnp = e.lnp;

  float* dA = b + bw.dA;
  float* dB = b + bw.dB;
  float* dC = b + bw.dC;
  // ---- d(xf_out) total = upstream + scatter of d(text_proj input) at the EOT rows -------------
  if (dxf_out) {
    HIG_TRY(hig_copy_async(dA, dxf_out, (size_t)M * Lt * 4, st));
  } else {
    HIG_TRY(hig_zero_async(dA, (size_t)M * Lt * 4, st));
  }
  if (dxf_proj) {
    HIG_TRY(e.colsum(dxf_proj, E, D.B, E, TG(grads, HIG_T_PROJ_B)));
    HIG_TRY(hig_gemm_launch(G(dxf_proj, E, 1, ws + w.gath, Lt, 1, TG(grads, HIG_T_PROJ_W), Lt, E, Lt, D.B).g, 1, nullptr, st));
    HIG_TRY(hig_gemm_launch(G(dxf_proj, E, 0, TP(params, HIG_T_PROJ_W), Lt, 1, b + bw.dgath, Lt, D.B, Lt, E).g, 1, nullptr, st));
    HIG_TRY(e.tap_copy(HIG_ETAP_DGATH, -1, b + bw.dgath));
    HIG_TRY(hig_scatter_add_rows(b + bw.dgath, Lt, D.B, D.N, eot, Lt, dA, Lt, stream));
  } else {
    HIG_TRY(hig_zero_async(TG(grads, HIG_T_PROJ_B), (size_t)E * 4, st));
    HIG_TRY(hig_zero_async(TG(grads, HIG_T_PROJ_W), (size_t)E * Lt * 4, st));
  }
  HIG_TRY(e.tap_copy(HIG_ETAP_DXF_TOTAL, -1, dA));
  // ---- text_ln ---------------------------------------------------------------------------
  const float* xL = ws + w.layer0 + w.lstride * (D.L - 1) + w.x2;
  HIG_TRY(hig_ln_bwd(dA, Lt, xL, Lt, ws + w.stf, TP(params, HIG_T_LN_W), TP(params, HIG_T_LN_B), nullptr, 0, 0, 0,
                     nullptr, 0, dB, Lt, M, Lt, D.N, TG(grads, HIG_T_LN_W), TG(grads, HIG_T_LN_B), nullptr, 0, lnp, stream));
  float* d = dB;      // d(x2 of layer l)
  float* t1 = dA;     // scratch (M, Lt)
  float* t2 = dC;
  for (int l = D.L - 1; l >= 0; --l) {
    const float* lb = ws + w.layer0 + w.lstride * l;
    const float* xin = l == 0 ? (D.pre ? ws + w.x0 : clip_out) : ws + w.layer0 + w.lstride * (l - 1) + w.x2;
    const EncLayerAct a = {lb + w.qkv, lb + w.lse, lb + w.att, lb + w.r1, lb + w.st1, lb + w.x1, lb + w.z, lb + w.f, lb + w.r2, lb + w.st2};
    HIG_TRY(hig_enc_layer_bwd(e, l, params + HIG_T_NGLOBAL + l * HIG_TL_NLAYER, grads + HIG_T_NGLOBAL + l * HIG_TL_NLAYER, a, xin, nullptr, d, t1,
                              t2));
  }
  // ---- text_pre_proj -----------------------------------------------------------------------
  if (D.pre) {
    HIG_TRY(e.wgrad_act(d, Lt, clip_out, D.W, TG(grads, HIG_T_PRE_W), M, TG(grads, HIG_T_PRE_B)));
    if (dclip) HIG_TRY(e.dgrad(d, TP(params, HIG_T_PRE_W), Lt, D.W, M, dclip, HIG_EPI_NONE, nullptr, nullptr));
  } else if (dclip) {
    HIG_TRY(hig_copy_async(dclip, d, (size_t)M * Lt * 4, st));
  }
  return HIG_OK;
}
