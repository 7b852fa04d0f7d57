// Evaluator feature extraction: forward of the reference's two scoring classifiers,
// MotionEncoder (codes/models/interaction_transformer.py:641-741) and MotionConsistencyEvalModel
// (:743-829), as they are called by EvaluatorModelWrapper.get_motion_embeddings
// (codes/datasets/evaluator.py:479-493), and their training step (tools/train_evaluation_model.py,
// tools/train_consistency_evaluation_model.py): the same forward with every layer's activations kept, its adjoint, and
// nn.CrossEntropyLoss.
//
//   h[b] = [cls_input?] ++ embed(x1[b]) ++ embed(x2[b])            (S = cls + 2T tokens)
//   embed(x)[0] = joint_embed2(x[0, :4]);  embed(x)[t>=1] = joint_embed1(x[t]) + sequence_embedding[t-1]
//   L x post-norm nn.TransformerEncoderLayer (gelu, dropout 0) with key padding mask
//        pad[b][cls + p*T + t] = (t >= length[b])
//   MotionEncoder: o = out2(h[token 0 of a person]) / out1(h[other tokens]);
//                  feature = sum_valid o / #valid;  logits = fin_proj(feature)
//   Consistency:   logits = cls_output(h[cls token])
// Host code + a few small row kernels; the GEMMs, LayerNorm and attention are the shared ones, and the backward of a layer is
// the text head's (hig_enc_layer_fwd / hig_enc_layer_bwd, enc_layers.h).
#include "hig_common.h"
#include "enc_layers.h"

namespace {

struct EDims {
  int B, T, F, d, H, ff, L, C, cls, hd, prec, S;
  int64_t M;
  EncShape enc() const { return {B, S, d, ff, H, hd}; }
};

int check_edims(const hig_eval_dims* p, EDims& D) {
  HIG_REQUIRE(p, "null eval dims");
  D.B = p->B; D.T = p->T; D.F = p->F; D.d = p->d; D.H = p->H; D.ff = p->ff; D.L = p->L; D.C = p->C;
  D.cls = p->cls ? 1 : 0;
  HIG_REQUIRE(D.B > 0 && D.T > 1 && D.F >= 4 && D.d > 0 && D.H > 0 && D.ff > 0 && D.L > 0 && D.C > 0,
              "hig_eval_dims: every extent must be positive (T >= 2, F >= 4)");
  HIG_REQUIRE(D.d % D.H == 0, "hig_eval_dims: d=%d not divisible by H=%d", D.d, D.H);
  D.hd = D.d / D.H;
  HIG_TRY(hig_enc_check_hd("hig eval encoder", D.hd));
  HIG_REQUIRE(D.d % 4 == 0 && D.ff % 4 == 0 && D.d <= 1024, "hig_eval_dims: d, ff must be multiples of 4 and d <= 1024");
  HIG_TRY(hig_enc_check_prec(p->prec));
  D.prec = p->prec;
  D.S = D.cls + 2 * D.T;
  D.M = (int64_t)D.B * D.S;
  return HIG_OK;
}

struct EWs {
  int64_t emb, h, kpad, qkv, lse, att, r1, st, x1, f, r2, xa, xb, feat, total;
};
EWs ews_layout(const EDims& D) {
  EWs w;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += al(n); return r; };
  w.emb = take((int64_t)2 * D.B * D.T * D.d);   // [person][b][t][d]
  w.h = take(D.M * D.d);
  w.kpad = take((D.M + 3) / 4);                 // bytes
  w.qkv = take(D.M * 3 * D.d);
  w.lse = take((int64_t)D.B * D.H * D.S);
  w.att = take(D.M * D.d);
  w.r1 = take(D.M * D.d);
  w.st = take(D.M * 2);
  w.x1 = take(D.M * D.d);
  w.f = take(D.M * D.ff);
  w.r2 = take(D.M * D.d);
  w.xa = take(D.M * D.d);
  w.xb = take(D.M * D.d);
  w.feat = take((int64_t)D.B * D.d);
  w.total = o;
  return w;
}

using ETab = Tab<const void>;   // a parameter table: P[HIG_EV_*], P(l, HIG_TL_*)
inline ETab etab(const void* const* t) { return ETab(t, HIG_EV_NGLOBAL, HIG_TL_NLAYER); }

// Row (b, s) of h: the [cls] vector, or row (p, b, t) of the per-person embeddings; also the key padding byte.
__global__ __launch_bounds__(128) void assemble_kernel(const float* __restrict__ emb, const float* __restrict__ cls_in,
                                                       const int64_t* __restrict__ length, float* __restrict__ h,
                                                       uint8_t* __restrict__ kpad, int B, int T, int d, int cls) {
  const int S = cls + 2 * T;
  const int64_t row = blockIdx.x;
  const int b = (int)(row / S), s = (int)(row % S);
  const float* src;
  bool pad = false;
  if (s < cls) {
    src = cls_in;
  } else {
    const int p = (s - cls) / T, t = (s - cls) % T;
    src = emb + (((int64_t)p * B + b) * T + t) * d;
    pad = t >= length[b];
  }
  float* dst = h + row * d;
  for (int c = 4 * threadIdx.x; c < d; c += 4 * 128)
    *reinterpret_cast<float4*>(dst + c) = *reinterpret_cast<const float4*>(src + c);
  if (threadIdx.x == 0) kpad[row] = pad ? 1 : 0;
}

// feature[b][c] = sum over both persons' tokens t < length[b] of o[b][cls + p*T + t][c], divided by their count
// (interaction_transformer.py:739-740: (cat([output1, output2]) * src_mask).sum(1) / src_mask.sum(1)).
__global__ __launch_bounds__(256) void masked_mean_kernel(const float* __restrict__ o, const int64_t* __restrict__ length,
                                                          float* __restrict__ feat, int T, int cls, int d) {
  const int b = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= d) return;
  const int S = cls + 2 * T;
  int64_t len = length[b];
  if (len > T) len = T;
  if (len < 0) len = 0;
  const float* ob = o + ((int64_t)b * S + cls) * d + c;
  float acc = 0.f;
  for (int p = 0; p < 2; ++p)
    for (int t = 0; t < (int)len; ++t) acc += ob[((int64_t)p * T + t) * d];
  feat[(int64_t)b * d + c] = acc / (float)(2 * len);
}


// ---- training ---------------------------------------------------------------------------------------------------------
// Forward workspace (floats) by HIG_EFW_* slot: the inference prefix, then one activation block per layer (the text head's).
using ETrain = std::array<int64_t, HIG_EFW_NSLOTS>;
ETrain etrain_layout(const EDims& D) {
  ETrain w;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += al(n); return r; };
  w[HIG_EFW_EMB] = take((int64_t)2 * D.B * D.T * D.d);
  w[HIG_EFW_H] = take(D.M * D.d);
  w[HIG_EFW_KPAD] = take((D.M + 3) / 4);
  w[HIG_EFW_O] = take(D.cls ? 0 : D.M * D.d);
  w[HIG_EFW_FEAT] = take((int64_t)D.B * D.d);
  w[HIG_EFW_LAYER0] = o;
  o = 0;
  hig_enc_block_layout(take, &w[HIG_EFW_QKV], D.enc());
  w[HIG_EFW_LSTRIDE] = o;
  w[HIG_EFW_TOTAL] = w[HIG_EFW_LAYER0] + o * D.L;
  return w;
}

// Backward workspace (floats) by HIG_EBW_* slot: the layers' scratch, the MotionEncoder head ((B, d) each), the embedding.
using EBwd = std::array<int64_t, HIG_EBW_NSLOTS>;
constexpr EncScratchSlots EBW_SCRATCH = {HIG_EBW_DFF,   HIG_EBW_DQKV,        HIG_EBW_DELTA,   HIG_EBW_WT,    -1, -1,
                                         HIG_EBW_SLABS, HIG_EBW_SLAB_FLOATS, HIG_EBW_COLPART, HIG_EBW_LNPART};
constexpr int EBW_HEAD[] = {HIG_EBW_DFT, HIG_EBW_G, HIG_EBW_GN, HIG_EBW_G2, HIG_EBW_POOL1, HIG_EBW_POOL2, HIG_EBW_U1, HIG_EBW_U2};
EBwd ebwd_layout(const EDims& D) {
  EBwd w;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += al(n); return r; };
  const int64_t d = D.d, R = (int64_t)2 * D.B * D.T;
  w[HIG_EBW_DA] = take(D.M * d);
  w[HIG_EBW_DB] = take(D.M * d);
  w[HIG_EBW_DC] = take(D.M * d);
  hig_enc_scratch_grads(take, w.data(), EBW_SCRATCH, D.enc());
  int64_t big = 3 * d * d;
  if ((int64_t)D.ff * d > big) big = (int64_t)D.ff * d;
  if ((int64_t)d * D.F > big) big = (int64_t)d * D.F;
  hig_enc_scratch_work(take, w.data(), EBW_SCRATCH, D.enc(), big,
                       {{D.M, 3 * d}, {D.M, D.ff}, {D.B, D.C}, {D.B, d}, {R, d}, {2 * D.B, (int64_t)D.T * d}});
  for (int s : EBW_HEAD) w[s] = take((int64_t)D.B * d);
  w[HIG_EBW_XCAT] = take(R * D.F);
  w[HIG_EBW_DMOVE] = take(R * d);
  w[HIG_EBW_DINIT] = take((int64_t)2 * D.B * d);
  w[HIG_EBW_POSTMP] = take((int64_t)D.T * d);
  w[HIG_EBW_TOTAL] = o;
  return w;
}

__device__ __forceinline__ int clamp_len(const int64_t* length, int b, int T) {
  int64_t len = length[b];
  if (len > T) len = T;
  if (len < 0) len = 0;
  return (int)len;
}

// The MotionEncoder's masked mean is linear in h: with g[b] = d(feature)[b] / (2 len_b),
//   d(out1.weight) = g^T pool1, d(out1.bias) = sum_b 2 (len_b - 1) g[b]    pool1[b] = sum of h over the valid tokens t >= 1 of both persons
//   d(out2.weight) = g^T pool2, d(out2.bias) = sum_b 2 g[b]                pool2[b] = h of the two init-pose tokens
//   d(h)[b][s] = g[b] . out2.weight on a valid init-pose token, g[b] . out1.weight on any other valid token, 0 on a padded one
// so the (M, d) gradient of o is never written.
__global__ __launch_bounds__(256) void pool_kernel(const float* __restrict__ h, const int64_t* __restrict__ length,
                                                   float* __restrict__ pool1, float* __restrict__ pool2, int T, int d) {
  const int b = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= d) return;
  const int len = clamp_len(length, b, T);
  const float* hb = h + (int64_t)b * 2 * T * d + c;
  float a1 = 0.f, a2 = 0.f;
  for (int p = 0; p < 2; ++p) {
    if (len > 0) a2 += hb[(int64_t)p * T * d];
    for (int t = 1; t < len; ++t) a1 += hb[((int64_t)p * T + t) * d];
  }
  pool1[(int64_t)b * d + c] = a1;
  pool2[(int64_t)b * d + c] = a2;
}
__global__ __launch_bounds__(256) void head_scale_kernel(const float* __restrict__ dft, const int64_t* __restrict__ length,
                                                         float* __restrict__ g, float* __restrict__ gn, float* __restrict__ g2,
                                                         int T, int d) {
  const int b = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= d) return;
  const int len = clamp_len(length, b, T);
  const int64_t i = (int64_t)b * d + c;
  const float v = len > 0 ? dft[i] / (float)(2 * len) : 0.f;
  g[i] = v;
  gn[i] = (float)(len > 0 ? 2 * (len - 1) : 0) * v;
  g2[i] = len > 0 ? 2.f * v : 0.f;
}
// d(h) rows of the MotionEncoder (cls == 0): grid = M rows
__global__ __launch_bounds__(128) void unpool_kernel(const float* __restrict__ u1, const float* __restrict__ u2,
                                                     const int64_t* __restrict__ length, float* __restrict__ dh, int T, int d) {
  const int S = 2 * T;
  const int64_t row = blockIdx.x;
  const int b = (int)(row / S), t = (int)(row % S) % T;
  const bool valid = t < clamp_len(length, b, T);
  const float* src = (t == 0 ? u2 : u1) + (int64_t)b * d;
  float* dst = dh + row * d;
  for (int c = 4 * threadIdx.x; c < d; c += 4 * 128)
    *reinterpret_cast<float4*>(dst + c) = valid ? *reinterpret_cast<const float4*>(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// Adjoint of assemble_kernel: row (p, b, t) of the per-person blocks takes row (b, cls + p T + t) of d(h); the init-pose rows
// (t = 0: joint_embed2, no positional term) go to dinit (p, b) and leave zeros behind, so that the joint_embed1 /
// sequence_embedding adjoints see the motion rows only.  grid = 2 B T rows
__global__ __launch_bounds__(128) void unassemble_kernel(const float* __restrict__ dh, float* __restrict__ dmove,
                                                         float* __restrict__ dinit, int B, int T, int d, int cls) {
  const int S = cls + 2 * T;
  const int64_t row = blockIdx.x;
  const int t = (int)(row % T), pb = (int)(row / T), p = pb / B, b = pb % B;
  const float* src = dh + ((int64_t)b * S + cls + (int64_t)p * T + t) * d;
  float* dst = dmove + row * d;
  float* ini = dinit + (int64_t)pb * d;
  for (int c = 4 * threadIdx.x; c < d; c += 4 * 128) {
    const float4 v = *reinterpret_cast<const float4*>(src + c);
    if (t == 0) {
      *reinterpret_cast<float4*>(ini + c) = v;
      *reinterpret_cast<float4*>(dst + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      *reinterpret_cast<float4*>(dst + c) = v;
    }
  }
}

// nn.CrossEntropyLoss(): one workgroup of four waves, wave w takes rows w, w + 4, ...; a row's maximum, sum and argmax are
// wave reductions, the loss is summed per wave in row order and the four partial sums in a fixed order: no atomics.
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}
__global__ __launch_bounds__(256) void softmax_xent_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                           int B, int C, float* __restrict__ loss, float* __restrict__ dlogits,
                                                           int64_t* __restrict__ pred) {
  __shared__ float s_part[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float invB = 1.0f / (float)B;
  float acc = 0.f;
  for (int b = wave; b < B; b += 4) {
    const float* row = logits + (int64_t)b * C;
    float mx = -INFINITY;
    int arg = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
      const float v = row[c];
      if (v > mx) { mx = v; arg = c; }
    }
    const float wm = wave_max(mx);
    arg = wave_min_int(mx == wm ? arg : 0x7fffffff);   // the first index that holds the maximum
    float se = 0.f;
    for (int c = lane; c < C; c += 64) se += expf(row[c] - wm);
    se = wave_sum(se);
    const int64_t lab = labels[b];
    const bool ok = lab >= 0 && lab < C;
    acc += (wm + logf(se)) - (ok ? row[lab] : 0.f);
    if (dlogits) {
      float* drow = dlogits + (int64_t)b * C;
      for (int c = lane; c < C; c += 64) drow[c] = (expf(row[c] - wm) / se - ((ok && c == (int)lab) ? 1.f : 0.f)) * invB;
    }
    if (pred && lane == 0) pred[b] = arg < C ? arg : 0;
  }
  if (lane == 0) s_part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *loss = ((s_part[0] + s_part[1]) + (s_part[2] + s_part[3])) * invB;
}

// what both training entry points ask of a table (parameters or gradients) before the first launch
int check_train(const EDims& D, const void* const* table, const char* who) {
  const ETab P = etab(table);
  if (D.prec != HIG_PREC_F32)
    return hig_set_error(HIG_EUNSUPPORTED, "%s: training the evaluation classifiers runs exact-fp32 products only (prec f32)", who);
  HIG_REQUIRE(P[HIG_EV_SEQ_EMB] && P[HIG_EV_JOINT1_W] && P[HIG_EV_JOINT1_B] && P[HIG_EV_JOINT2_W] &&
                  P[HIG_EV_JOINT2_B] && P[HIG_EV_HEAD_W] && P[HIG_EV_HEAD_B],
              "%s: missing embedding / head slots", who);
  if (D.cls)
    HIG_REQUIRE(P[HIG_EV_CLS_IN], "%s: consistency model needs cls_input", who);
  else
    HIG_REQUIRE(P[HIG_EV_OUT1_W] && P[HIG_EV_OUT1_B] && P[HIG_EV_OUT2_W] && P[HIG_EV_OUT2_B],
                "%s: MotionEncoder needs out1 / out2", who);
  for (int l = 0; l < D.L; ++l)
    for (int i = 0; i < HIG_TL_NLAYER; ++i) HIG_REQUIRE(P(l, i), "%s: layer %d lacks slot %d", who, l, i);
  return HIG_OK;
}

// The forward both entry points launch; they differ in where a layer's activations live (layer_of(l)) and in whether the GELU
// pre-activation is kept (z != NULL).  o: (M, d) scratch of the MotionEncoder head; feat: where its pooled feature goes.
template <class LayerOf>
int eval_forward(const EDims& D, const void* const* params, const float* x1, const float* x2, const int64_t* length,
                 float* logits, float* emb, float* h, uint8_t* kpad, float* o, float* feat, int prec, LayerOf layer_of,
                 hig_stream_t stream) {
  const ETab P = etab(params);
  hipStream_t st = hig_stream(stream);
  const int d = D.d, T = D.T, S = D.S;
  const int64_t M = D.M, BT = (int64_t)D.B * T;
  // per-person embeddings: every row through joint_embed1 (+ sequence_embedding[t-1]), then the init-pose rows
  // (t = 0) overwritten with joint_embed2 of their first 4 features (:717-720 / :814-817)
  const float* xs[2] = {x1, x2};
  for (int p = 0; p < 2; ++p) {
    float* e = emb + p * BT * d;
    G ge(xs[p], D.F, 0, P[HIG_EV_JOINT1_W], D.F, 0, e, d, BT, d, D.F);
    ge.epi(HIG_EPI_BIAS_POS, P[HIG_EV_JOINT1_B]).pos(P[HIG_EV_SEQ_EMB], d, T).prec(prec);
    ge.g.pos_shift = 1;
    HIG_TRY(hig_gemm_launch(ge.g, 1, nullptr, st));
    HIG_TRY(hig_gemm_launch(G(xs[p], (int64_t)T * D.F, 0, P[HIG_EV_JOINT2_W], 4, 0, e, (int64_t)T * d, D.B, d, 4)
                                .epi(HIG_EPI_BIAS, P[HIG_EV_JOINT2_B]).g, 1, nullptr, st));
  }
  hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)M), dim3(128), 0, st, emb, P[HIG_EV_CLS_IN], length, h, kpad, D.B,
                     T, d, D.cls);
  HIG_CHECK_LAUNCH();

  const float* xin = h;
  for (int l = 0; l < D.L; ++l) {
    const EncLayer a = layer_of(l);
    HIG_TRY(hig_enc_layer_fwd(D.enc(), P.layer(l), a, xin, kpad, prec, stream));
    xin = a.x2;
  }

  if (D.cls) {  // logits from the [cls] token's row of each pair
    return hig_gemm_launch(G(xin, (int64_t)S * d, 0, P[HIG_EV_HEAD_W], d, 0, logits, D.C, D.B, D.C, d)
                               .epi(HIG_EPI_BIAS, P[HIG_EV_HEAD_B]).g, 1, nullptr, st);
  }
  HIG_TRY(hig_gemm_launch(G(xin, d, 0, P[HIG_EV_OUT1_W], d, 0, o, d, M, d, d)
                              .epi(HIG_EPI_BIAS, P[HIG_EV_OUT1_B]).prec(prec).g, 1, nullptr, st));
  for (int p = 0; p < 2; ++p)
    HIG_TRY(hig_gemm_launch(G(xin + (int64_t)p * T * d, (int64_t)S * d, 0, P[HIG_EV_OUT2_W], d, 0,
                              o + (int64_t)p * T * d, (int64_t)S * d, D.B, d, d)
                                .epi(HIG_EPI_BIAS, P[HIG_EV_OUT2_B]).g, 1, nullptr, st));
  hipLaunchKernelGGL(masked_mean_kernel, dim3(D.B, (d + 255) / 256), dim3(256), 0, st, o, length, feat, T, D.cls, d);
  HIG_CHECK_LAUNCH();
  return hig_gemm_launch(G(feat, d, 0, P[HIG_EV_HEAD_W], d, 0, logits, D.C, D.B, D.C, d)
                             .epi(HIG_EPI_BIAS, P[HIG_EV_HEAD_B]).g, 1, nullptr, st);
}

}  // namespace

extern "C" int64_t hig_eval_encoder_workspace_bytes(const hig_eval_dims* dims) {
  EDims D;
  if (check_edims(dims, D) != HIG_OK) return -1;
  return ews_layout(D).total * 4;
}

extern "C" int hig_eval_encoder_fwd(const hig_eval_dims* dims, const void* const* params, const float* x1,
                                    const float* x2, const int64_t* length, float* logits, float* feature,
                                    void* workspace, hig_stream_t stream) {
  EDims D;
  HIG_TRY(check_edims(dims, D));
  HIG_REQUIRE(params && x1 && x2 && length && logits && workspace, "hig_eval_encoder_fwd: null argument");
  const ETab P = etab(params);
  HIG_REQUIRE(P[HIG_EV_SEQ_EMB] && P[HIG_EV_JOINT1_W] && P[HIG_EV_JOINT2_W] && P[HIG_EV_HEAD_W],
              "hig_eval_encoder_fwd: missing embedding / head parameters");
  if (D.cls)
    HIG_REQUIRE(P[HIG_EV_CLS_IN], "hig_eval_encoder_fwd: consistency model needs cls_input");
  else
    HIG_REQUIRE(P[HIG_EV_OUT1_W] && P[HIG_EV_OUT2_W], "hig_eval_encoder_fwd: MotionEncoder needs out1 / out2");
  const EWs w = ews_layout(D);
  float* ws = static_cast<float*>(workspace);
  // one activation block, the layer output ping-ponging between xa and xb so that a layer never overwrites its own input; the
  // head's o reuses r1
  auto layer_of = [&](int l) {
    return EncLayer{ws + w.qkv, ws + w.lse, ws + w.att, ws + w.r1, ws + w.st, ws + w.x1, nullptr, ws + w.f, ws + w.r2, ws + w.st,
                     ws + ((l & 1) ? w.xb : w.xa)};
  };
  return eval_forward(D, params, x1, x2, length, logits, ws + w.emb, ws + w.h, reinterpret_cast<uint8_t*>(ws + w.kpad), ws + w.r1,
                      feature ? feature : ws + w.feat, D.prec, layer_of, stream);
}

extern "C" int64_t hig_eval_encoder_train_workspace_bytes(const hig_eval_dims* dims) {
  EDims D;
  if (check_edims(dims, D) != HIG_OK) return -1;
  return etrain_layout(D)[HIG_EFW_TOTAL] * 4;
}
extern "C" int64_t hig_eval_encoder_bwd_workspace_bytes(const hig_eval_dims* dims) {
  EDims D;
  if (check_edims(dims, D) != HIG_OK) return -1;
  return ebwd_layout(D)[HIG_EBW_TOTAL] * 4;
}
// ---- test hooks (include/hig.h): the training layouts above and the tap's, by named slot ----
extern "C" int64_t hig_eval_encoder_bwd_tap_bytes(const hig_eval_dims* dims) {
  EDims D;
  if (check_edims(dims, D) != HIG_OK) return HIG_EINVAL;
  return hig_enc_tap_layout(false, D.enc(), D.L).off[HIG_ETAP_TOTAL] * 4;
}
extern "C" int hig_eval_encoder_layout(const hig_eval_dims* dims, int32_t which, int64_t* out, int32_t n_out) {
  EDims D;
  if (check_edims(dims, D) != HIG_OK) return HIG_EINVAL;   // (the message is check_edims's)
  if (which == HIG_ENC_LAYOUT_FWD) {
    ETrain w = etrain_layout(D);
    if (D.cls) w[HIG_EFW_O] = w[HIG_EFW_FEAT] = -1;      // (the MotionEncoder head)
    return hig_enc_publish(w.data(), HIG_EFW_NSLOTS, out, n_out);
  }
  if (which == HIG_ENC_LAYOUT_BWD) {
    EBwd w = ebwd_layout(D);
    if (D.cls)
      for (int s : EBW_HEAD) w[s] = -1;
    return hig_enc_publish(w.data(), HIG_EBW_NSLOTS, out, n_out);
  }
  if (which == HIG_ENC_LAYOUT_TAP) return hig_enc_publish(hig_enc_tap_layout(false, D.enc(), D.L).off, HIG_ETAP_NSLOTS, out, n_out);
  return hig_set_error(HIG_EINVAL, "hig_eval_encoder_layout: no layout table %d", which);
}

extern "C" int hig_eval_encoder_fwd_train(const hig_eval_dims* dims, const void* const* params, const float* x1,
                                          const float* x2, const int64_t* length, float* logits, float* feature,
                                          void* workspace, hig_stream_t stream) {
  EDims D;
  HIG_TRY(check_edims(dims, D));
  HIG_REQUIRE(params && x1 && x2 && length && logits && workspace, "hig_eval_encoder_fwd_train: null argument");
  HIG_TRY(check_train(D, params, "hig_eval_encoder_fwd_train"));
  const ETrain w = etrain_layout(D);
  float* ws = static_cast<float*>(workspace);
  // one block per layer, the GELU pre-activation z kept
  auto layer_of = [&](int l) { return hig_enc_block_at(ws + w[HIG_EFW_LAYER0] + w[HIG_EFW_LSTRIDE] * l, &w[HIG_EFW_QKV]); };
  // the pooled feature is kept in the workspace (the backward's fin_proj weight gradient reads it) and copied out
  HIG_TRY(eval_forward(D, params, x1, x2, length, logits, ws + w[HIG_EFW_EMB], ws + w[HIG_EFW_H],
                       reinterpret_cast<uint8_t*>(ws + w[HIG_EFW_KPAD]), ws + w[HIG_EFW_O], ws + w[HIG_EFW_FEAT], HIG_PREC_F32, layer_of,
                       stream));
  if (!D.cls && feature) HIG_TRY(hig_copy_async(feature, ws + w[HIG_EFW_FEAT], (int64_t)D.B * D.d * 4, hig_stream(stream)));
  return HIG_OK;
}

extern "C" int hig_eval_encoder_bwd(const hig_eval_dims* dims, const void* const* params, const float* x1, const float* x2,
                                    const int64_t* length, const void* workspace, const float* dlogits,
                                    const float* dfeature, void* const* grads, void* bwd_workspace, hig_stream_t stream) {
  EDims D;
  HIG_TRY(check_edims(dims, D));
  HIG_REQUIRE(params && x1 && x2 && length && workspace && dlogits && grads && bwd_workspace, "hig_eval_encoder_bwd: null argument");
  HIG_TRY(check_train(D, params, "hig_eval_encoder_bwd"));
  HIG_TRY(check_train(D, grads, "hig_eval_encoder_bwd (gradient table)"));
  HIG_REQUIRE(!(D.cls && dfeature), "hig_eval_encoder_bwd: the consistency model has no feature output");
  const ETrain w = etrain_layout(D);
  const EBwd bw = ebwd_layout(D);
  const ETab P = etab(params);
  const Tab Gr(grads, HIG_EV_NGLOBAL, HIG_TL_NLAYER);
  const float* ws = static_cast<const float*>(workspace);
  float* b = static_cast<float*>(bwd_workspace);
  hipStream_t st = hig_stream(stream);
  const int d = D.d, T = D.T, S = D.S, C = D.C, F = D.F;
  const int64_t M = D.M, BT = (int64_t)D.B * T;
  const uint8_t* kpad = reinterpret_cast<const uint8_t*>(ws + w[HIG_EFW_KPAD]);
  EncBwd e(D.enc(), HIG_PREC_F32, b, bw.data(), EBW_SCRATCH, stream);
  HIG_TRY(e.tap_begin(false, D.L, "hig_eval_encoder_bwd"));

  float* dA = b + bw[HIG_EBW_DA];
  float* dB = b + bw[HIG_EBW_DB];
  float* dC = b + bw[HIG_EBW_DC];
  float *dft = b + bw[HIG_EBW_DFT], *g = b + bw[HIG_EBW_G], *gn = b + bw[HIG_EBW_GN], *g2 = b + bw[HIG_EBW_G2];
  float *pool1 = b + bw[HIG_EBW_POOL1], *pool2 = b + bw[HIG_EBW_POOL2], *u1 = b + bw[HIG_EBW_U1], *u2 = b + bw[HIG_EBW_U2];
  float* postmp = b + bw[HIG_EBW_POSTMP];
  const float* feat = ws + w[HIG_EFW_FEAT];
  auto layer = [&](int l) { return hig_enc_block_at(ws + w[HIG_EFW_LAYER0] + w[HIG_EFW_LSTRIDE] * l, &w[HIG_EFW_QKV]); };
  const float* xL = layer(D.L - 1).x2;
  // ---- head: d(h of the last layer) into dB ---------------------------------------------------------------------------
  HIG_TRY(e.colsum(dlogits, C, D.B, C, Gr[HIG_EV_HEAD_B]));
  if (D.cls) {
    // logits = cls_output(h[b][0])
    HIG_TRY(hig_gemm_launch(G(dlogits, C, 1, xL, (int64_t)S * d, 1, Gr[HIG_EV_HEAD_W], d, C, d, D.B).g, 1, nullptr, st));
    HIG_TRY(hig_zero_async(dB, M * d * 4, st));
    HIG_TRY(hig_gemm_launch(G(dlogits, C, 0, P[HIG_EV_HEAD_W], d, 1, dB, (int64_t)S * d, D.B, d, C).g, 1, nullptr, st));
  } else {
    HIG_TRY(hig_gemm_launch(G(dlogits, C, 1, feat, d, 1, Gr[HIG_EV_HEAD_W], d, C, d, D.B).g, 1, nullptr, st));
    // d(feature) total = upstream + dlogits . fin_proj.weight
    G gf(dlogits, C, 0, P[HIG_EV_HEAD_W], d, 1, dft, d, D.B, d, C);
    if (dfeature) gf.epi(HIG_EPI_RES).res(dfeature, d);
    HIG_TRY(hig_gemm_launch(gf.g, 1, nullptr, st));
    const dim3 gb(D.B, (d + 255) / 256);
    hipLaunchKernelGGL(head_scale_kernel, gb, dim3(256), 0, st, dft, length, g, gn, g2, T, d);
    HIG_CHECK_LAUNCH();
    hipLaunchKernelGGL(pool_kernel, gb, dim3(256), 0, st, xL, length, pool1, pool2, T, d);
    HIG_CHECK_LAUNCH();
    HIG_TRY(hig_gemm_launch(G(g, d, 1, pool1, d, 1, Gr[HIG_EV_OUT1_W], d, d, d, D.B).g, 1, nullptr, st));
    HIG_TRY(hig_gemm_launch(G(g, d, 1, pool2, d, 1, Gr[HIG_EV_OUT2_W], d, d, d, D.B).g, 1, nullptr, st));
    HIG_TRY(e.colsum(gn, d, D.B, d, Gr[HIG_EV_OUT1_B]));
    HIG_TRY(e.colsum(g2, d, D.B, d, Gr[HIG_EV_OUT2_B]));
    HIG_TRY(hig_gemm_launch(G(g, d, 0, P[HIG_EV_OUT1_W], d, 1, u1, d, D.B, d, d).g, 1, nullptr, st));
    HIG_TRY(hig_gemm_launch(G(g, d, 0, P[HIG_EV_OUT2_W], d, 1, u2, d, D.B, d, d).g, 1, nullptr, st));
    hipLaunchKernelGGL(unpool_kernel, dim3((unsigned)M), dim3(128), 0, st, u1, u2, length, dB, T, d);
    HIG_CHECK_LAUNCH();
  }
  HIG_TRY(e.tap_copy(HIG_ETAP_DH_L, -1, dB));
  // ---- layers ------------------------------------------------------------------------------------------------------------
  float* dh = dB;
  for (int l = D.L - 1; l >= 0; --l) {
    const float* xin = l == 0 ? ws + w[HIG_EFW_H] : layer(l - 1).x2;
    HIG_TRY(hig_enc_layer_bwd(e, l, P.layer(l), Gr.layer(l), layer(l), xin, kpad, dh, dA, dC));
  }
  HIG_TRY(e.tap_copy(HIG_ETAP_DH_0, -1, dh));
  // ---- embedding -----------------------------------------------------------------------------------------------------------
  if (D.cls) HIG_TRY(e.colsum(dh, (int64_t)S * d, D.B, d, Gr[HIG_EV_CLS_IN]));   // the [cls] rows, summed over the batch
  float* dmove = b + bw[HIG_EBW_DMOVE];
  float* dinit = b + bw[HIG_EBW_DINIT];
  float* xcat = b + bw[HIG_EBW_XCAT];
  hipLaunchKernelGGL(unassemble_kernel, dim3((unsigned)(2 * BT)), dim3(128), 0, st, dh, dmove, dinit, D.B, T, d, D.cls);
  HIG_CHECK_LAUNCH();
  HIG_TRY(hig_copy_async(xcat, x1, BT * F * 4, st));
  HIG_TRY(hig_copy_async(xcat + BT * F, x2, BT * F * 4, st));
  // joint_embed2: the init-pose rows (t = 0), first 4 features
  HIG_TRY(e.colsum(dinit, d, 2 * D.B, d, Gr[HIG_EV_JOINT2_B]));
  HIG_TRY(e.wgrad(G(dinit, d, 1, xcat, (int64_t)T * F, 1, Gr[HIG_EV_JOINT2_W], 4, d, 4, 2 * D.B)));
  // joint_embed1: the rows t >= 1 (the forward overwrote its t = 0 rows: they are zero in dmove)
  HIG_TRY(e.colsum(dmove, d, 2 * BT, d, Gr[HIG_EV_JOINT1_B]));
  HIG_TRY(e.wgrad(G(dmove, d, 1, xcat, F, 1, Gr[HIG_EV_JOINT1_W], F, d, F, 2 * BT)));
  // d(sequence_embedding)[t - 1] = sum over persons and samples of row t: column sums of dmove viewed as (2 B, T d), row 0 dropped
  // (the table's rows at or beyond T - 1 were never read: the caller zeroes their gradient, include/hig.h)
  HIG_TRY(e.colsum(dmove, (int64_t)T * d, 2 * D.B, T * d, postmp));
  HIG_TRY(hig_copy_async(Gr[HIG_EV_SEQ_EMB], postmp + d, (int64_t)(T - 1) * d * 4, st));
  return HIG_OK;
}

extern "C" int hig_softmax_xent(const float* logits, const int64_t* labels, int32_t B, int32_t C, float* loss, float* dlogits,
                                int64_t* pred, hig_stream_t stream) {
  HIG_REQUIRE(logits && labels && loss && B > 0 && C > 0 && C <= 1024, "hig_softmax_xent: bad arguments (0 < C <= 1024)");
  hipLaunchKernelGGL(softmax_xent_kernel, dim3(1), dim3(256), 0, hig_stream(stream), logits, labels, B, C, loss, dlogits, pred);
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}
