// The frozen CLIP text tower in front of the text head (MotionTransformer._clip_features, transformer.py:381-388, over OpenAI
// CLIP's Transformer of ResidualAttentionBlocks): pre-norm, causal, QuickGELU, inference only.
//     x = token_embedding[tokens] + positional_embedding
//     per layer:  x = x + out_proj(attn(ln_1(x)));   x = x + c_proj(quick_gelu(c_fc(ln_2(x))))
//     out = ln_final(x)
// Three kernels live here -- the embedding front, QuickGELU and the causal attention -- and the launch sequence, which is host
// code in the style of texthead.hip: GEMMs through hig_gemm_launch, norms through hig_layernorm, hipGraph-capturable.
#include "hig_common.h"
#include "enc_layers.h"

namespace {

// ---- out[row][:] = tok_emb[tokens[row]][:] + pos_emb[row % N][:]; an id outside [0, vocab) reads no embedding row ----------
__global__ __launch_bounds__(256) void clip_embed_kernel(const float* __restrict__ tok_emb, const float* __restrict__ pos_emb,
                                                          const int64_t* __restrict__ tokens, int N, int W, int vocab,
                                                          float* __restrict__ out, int64_t ldo) {
  const int64_t row = blockIdx.x;
  const int n = (int)(row % N);
  const int64_t id = tokens[row];
  const bool live = id >= 0 && id < vocab;
  const float* e = tok_emb + (live ? id : 0) * W;
  const float* p = pos_emb + (int64_t)n * W;
  for (int c = threadIdx.x; c < W; c += blockDim.x) out[row * ldo + c] = live ? e[c] + p[c] : p[c];
}

// ---- z * sigmoid(1.702 z) = z * rcp(1 + exp2(-1.702 log2(e) z)): v_exp_f32 and v_rcp_f32, no division sequence ------------
__device__ __forceinline__ float quick_gelu(float z) {
  constexpr float c = (float)(-1.702 * 1.44269504088896340736);   // rounded once
  return z * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z * c));
}
// n4 float4 (x 16-byte aligned, else n4 == 0), then the n - 4 n4 elements behind them one by one
__global__ __launch_bounds__(256) void quick_gelu_kernel(float* __restrict__ x, int64_t n4, int64_t n) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  float4* x4 = reinterpret_cast<float4*>(x);
  for (int64_t i = gid; i < n4; i += step) {
    float4 v = x4[i];
    v.x = quick_gelu(v.x); v.y = quick_gelu(v.y); v.z = quick_gelu(v.z); v.w = quick_gelu(v.w);
    x4[i] = v;
  }
  for (int64_t i = 4 * n4 + gid; i < n; i += step) x[i] = quick_gelu(x[i]);
}

// ---- causal attention, head dim 64, N <= 128 -------------------------------------------------------------------------------
// grid (B * H, query blocks of CA_QB rows), eight waves.  A workgroup stages the K and V rows 0 .. last row of its block in LDS
// (dynamic: 2 x N x 64 x 4 bytes, 39 KB at N = 77 -- four workgroups per compute unit -- and 64 KB at N = 128) and each wave
// takes every eighth query row n of the block:
//   scores   lane l owns keys l and l + 64; it reads its key's 64 channels as sixteen ds_read_b128 and multiplies them with
//            q_n, whose channels come out of the wave's registers one v_readlane each.  K sits at [m][slot ^ (m & 15)] in
//            16-byte slots: the sixteen lanes of every ds_read_b128 group then hit sixteen different slots of the 256-byte
//            bank row (the plain [m][c] form puts all of them on one).  A lane whose key is m > n walks key n instead and
//            its score is dropped: no K row beyond n is ever read.
//   softmax  maximum and sum over the wave by DPP; dead lanes hold -inf / 0.
//   output   lane l owns channel l: y_l = sum_{m <= n} p_m V[m][l], p_m out of lane m's register by v_readlane, the loop
//            ending at n: no V row beyond n is ever read.  V sits at [m][l]: a row is one conflict-free 256-byte read.
// VEC: the operands are 16-byte aligned with leading dimensions of whole float4 (the tower's are): staged by float4.
constexpr int CA_HD = 64, CA_NMAX = 128, CA_QB = 32, CA_NT = 512;

__device__ __forceinline__ float lane_value(float v, int lane) {   // `lane` uniform over the wave
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// q . k over the 64 channels of key row `m` (four partial sums)
__device__ __forceinline__ float key_score(const float* kS, int m, float q) {
  const float4* k = reinterpret_cast<const float4*>(kS + m * CA_HD);
  const int x = m & 15;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const float4 kv = k[s ^ x];
    a0 = fmaf(lane_value(q, 4 * s), kv.x, a0);
    a1 = fmaf(lane_value(q, 4 * s + 1), kv.y, a1);
    a2 = fmaf(lane_value(q, 4 * s + 2), kv.z, a2);
    a3 = fmaf(lane_value(q, 4 * s + 3), kv.w, a3);
  }
  return (a0 + a1) + (a2 + a3);
}

// LSE (the training forward): also lse[b][h][n] = mx + log(sum) of row n's n + 1 live keys, one store of lane 0 behind the
// row's sum; nothing else of the kernel depends on the flag, so Y has the same bits in both instances.
template <bool VEC, bool LSE>
__global__ __launch_bounds__(CA_NT) void causal_attn_kernel(const float* __restrict__ Q, int64_t ldq, const float* __restrict__ K,
                                                             const float* __restrict__ V, int64_t ldk, int N, int H,
                                                             float* __restrict__ Y, int64_t ldy, float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) float ca_lds[];
  float* kS = ca_lds;                 // N x 64
  float* vS = ca_lds + N * CA_HD;     // N x 64
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int q0 = blockIdx.y * CA_QB;
  const int qend = min(q0 + CA_QB, N);   // this block's query rows are q0 .. qend - 1, its keys 0 .. qend - 1
  const int64_t base = (int64_t)b * N;
  const int col = h * CA_HD;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if constexpr (VEC) {
    // qend x 16 float4 per operand, at most 4 per thread: every load is issued before the first store
    float4 kk[4], vv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = u * CA_NT + threadIdx.x, m = idx >> 4;
      kk[u] = vv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < qend) {
        const int64_t g = (base + m) * ldk + col + 4 * (idx & 15);
        kk[u] = *reinterpret_cast<const float4*>(K + g);
        vv[u] = *reinterpret_cast<const float4*>(V + g);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = u * CA_NT + threadIdx.x, m = idx >> 4;
      if (m < qend) {
        *reinterpret_cast<float4*>(kS + m * CA_HD + 4 * ((idx & 15) ^ (m & 15))) = kk[u];
        *reinterpret_cast<float4*>(vS + 4 * idx) = vv[u];
      }
    }
  } else {
    for (int idx = threadIdx.x; idx < qend * CA_HD; idx += CA_NT) {
      const int m = idx >> 6, c = idx & 63;
      const int64_t g = (base + m) * ldk + col + c;
      kS[m * CA_HD + 4 * ((c >> 2) ^ (m & 15)) + (c & 3)] = K[g];
      vS[idx] = V[g];
    }
  }
  __syncthreads();
  for (int n = q0 + wave; n < qend; n += CA_NT / 64) {
    const float q = Q[(base + n) * ldq + col + lane];
    const bool live0 = lane <= n, live1 = lane + 64 <= n;
    const float a0 = key_score(kS, min(lane, n), q);
    float a1 = 0.f;
    if (n >= 64) a1 = key_score(kS, min(lane + 64, n), q);   // uniform: the second key of every lane exists only from row 64 on
    const float s0 = live0 ? a0 * 0.125f : -INFINITY, s1 = live1 ? a1 * 0.125f : -INFINITY;   // 1 / sqrt(64), exact
    const float mx = wave_max(fmaxf(s0, s1));               // key 0 is live in every row: mx is finite
    const float p0 = live0 ? __expf(s0 - mx) : 0.f, p1 = live1 ? __expf(s1 - mx) : 0.f;
    const float sum = wave_sum(p0 + p1);
    const float inv = 1.0f / sum;
    if constexpr (LSE) {
      if (lane == 0) lse[(int64_t)blockIdx.x * N + n] = mx + __logf(sum);
    }
    float y = lane_value(p0, 0) * vS[lane];
    // keys lo .. hi, whose weights sit in lanes lo - off .. of `p`: eight V rows in flight per step
    auto add_keys = [&](float p, int lo, int hi, int off) {
      int m = lo;
      for (; m + 7 <= hi; m += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = vS[(m + i) * CA_HD + lane];
#pragma unroll
        for (int i = 0; i < 8; ++i) y = fmaf(lane_value(p, m + i - off), v[i], y);
      }
      for (; m <= hi; ++m) y = fmaf(lane_value(p, m - off), vS[m * CA_HD + lane], y);
    };
    add_keys(p0, 1, min(n, 63), 0);
    add_keys(p1, 64, n, 64);
    Y[(base + n) * ldy + col + lane] = y * inv;
  }
}

// ---- the tower's launch sequence ---------------------------------------------------------------------------------------------
struct CDims {
  int B, N, W, H, L, vocab, prec;
  int64_t M;
  EncShape enc() const { return {B, N, W, 4 * W, H, CA_HD}; }
};

int check_cdims(const int32_t* p, CDims& D) {
  HIG_REQUIRE(p, "null clip dims");
  D.B = p[HIG_CD_B]; D.N = p[HIG_CD_N]; D.W = p[HIG_CD_W]; D.H = p[HIG_CD_H]; D.L = p[HIG_CD_L];
  D.vocab = p[HIG_CD_VOCAB]; D.prec = p[HIG_CD_PREC];
  HIG_REQUIRE(D.B > 0 && D.N > 0 && D.W > 0 && D.H > 0 && D.L > 0 && D.vocab > 0, "clip dims: every extent must be positive");
  HIG_REQUIRE(D.W % D.H == 0, "clip dims: W=%d not divisible by H=%d", D.W, D.H);
  if (D.W / D.H != CA_HD)
    return hig_set_error(HIG_EUNSUPPORTED, "hig clip text tower: head dim %d (W=%d / H=%d), built for 64 only", D.W / D.H, D.W, D.H);
  if (D.N > CA_NMAX)
    return hig_set_error(HIG_EUNSUPPORTED, "hig clip text tower: N=%d tokens, the causal attention covers N <= %d", D.N, CA_NMAX);
  if (D.W > 1024) return hig_set_error(HIG_EUNSUPPORTED, "hig clip text tower: W=%d, hig_layernorm covers rows of <= 1024", D.W);
  HIG_TRY(hig_enc_check_prec(D.prec));
  D.M = (int64_t)D.B * D.N;
  return HIG_OK;
}
int check_train(const int32_t* dims, CDims& D, const char* who) {
  HIG_TRY(check_cdims(dims, D));
  if (D.prec != HIG_PREC_F32) return hig_set_error(HIG_EUNSUPPORTED, "%s: prec=%d, the tower trains with exact fp32 products only", who, D.prec);
  return HIG_OK;
}

// Inference workspace (floats): the embedded rows and ln_final's statistics, then two layer blocks.
struct CFwd {
  int64_t x0, stf, layer0, block;
  int64_t h, st, qkv, att, x1, f, x2;
  int64_t total;
};
CFwd cfwd_layout(const CDims& D) {
  CFwd w;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += al(n); return r; };
  w.x0 = take(D.M * D.W);
  w.stf = take(D.M * 2);
  w.layer0 = o;
  o = 0;
  w.h = take(D.M * D.W);          // ln_1(x), then ln_2(x1)
  w.st = take(D.M * 2);
  w.qkv = take(D.M * 3 * D.W);
  w.att = take(D.M * D.W);
  w.x1 = take(D.M * D.W);
  w.f = take(D.M * 4 * D.W);
  w.x2 = take(D.M * D.W);
  w.block = o;
  // layer l works in block l & 1, so a layer never overwrites its own input (the x2 of layer l - 1)
  w.total = w.layer0 + 2 * w.block;
  return w;
}

// What hig_clip_text_fwd_train keeps (floats): the embedded rows and ln_final's statistics, then per layer the two LayerNorms'
// statistics, qkv, lse, the attention output, x1, the FFN's pre-activation z and x2 (the next layer's input).  The LayerNorm
// outputs and quick_gelu(z) are not kept: the adjoint rebuilds them (hig_layernorm, hig_quick_gelu_to), bit for bit.  Behind the
// layers: the two buffers the forward itself rebuilds per layer (h, f).
struct CTrain {
  int64_t x0, stf, layer0, lstride;
  int64_t st1, qkv, lse, att, x1, st2, z, x2;
  int64_t h, f, total;
};
CTrain ctrain_layout(const CDims& D) {
  CTrain w;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += al(n); return r; };
  w.x0 = take(D.M * D.W);
  w.stf = take(D.M * 2);
  w.layer0 = o;
  o = 0;
  w.st1 = take(D.M * 2);
  w.qkv = take(D.M * 3 * D.W);
  w.lse = take((int64_t)D.B * D.H * D.N);
  w.att = take(D.M * D.W);
  w.x1 = take(D.M * D.W);
  w.st2 = take(D.M * 2);
  w.z = take(D.M * 4 * D.W);
  w.x2 = take(D.M * D.W);
  w.lstride = o;
  o = w.layer0 + w.lstride * D.L;
  w.h = take(D.M * D.W);
  w.f = take(D.M * 4 * D.W);
  w.total = o;
  return w;
}

// The adjoint's workspace (floats): d / t1 / t2 / h (M, W), h's statistics, f (M, 4 W), the shared backward scratch, and the
// embedding pass's chunk partials and per-id sums (at most B N rows each).  An array by slot, unlike CFwd and CTrain above,
// because the shared scratch layout and EncBwd's binding (enc_layers.h) address a chain's table by slot.
enum { CBW_D = 0, CBW_T1, CBW_T2, CBW_H, CBW_HST, CBW_F, CBW_DFF, CBW_DQKV, CBW_DELTA, CBW_WT, CBW_SLABS, CBW_SLAB_FLOATS, CBW_COLPART,
       CBW_LNPART, CBW_EMB, CBW_TOTAL, CBW_NSLOTS };
using CBwd = std::array<int64_t, CBW_NSLOTS>;
constexpr EncScratchSlots CBW_SCRATCH = {CBW_DFF, CBW_DQKV, CBW_DELTA, CBW_WT, -1, -1, CBW_SLABS, CBW_SLAB_FLOATS, CBW_COLPART, CBW_LNPART};
CBwd cbwd_layout(const CDims& D) {
  CBwd w;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += al(n); return r; };
  const int64_t ff = 4 * (int64_t)D.W;
  for (int s : {CBW_D, CBW_T1, CBW_T2, CBW_H}) w[s] = take(D.M * D.W);
  w[CBW_HST] = take(D.M * 2);
  w[CBW_F] = take(D.M * ff);
  hig_enc_scratch_grads(take, w.data(), CBW_SCRATCH, D.enc());
  hig_enc_scratch_work(take, w.data(), CBW_SCRATCH, D.enc(), ff * D.W /* c_fc / c_proj */, {{D.M, ff}});
  w[CBW_EMB] = take(2 * D.M * D.W);
  w[CBW_TOTAL] = o;
  return w;
}

// Where one layer of the tower works: ln_1 / ln_2's output h and their statistics, qkv, the attention's row log-sum-exps, its
// output, x1, the FFN's pre-activation z, f = quick_gelu(z), x2.
struct CLayer {
  float *h, *st1, *st2, *qkv, *lse, *att, *x1, *z, *f, *x2;
};
// The forward both entry points launch; they differ in where layer l works (layer_of(l)), in whether lse is kept (lse != NULL:
// hig_causal_attn_fwd_train) and in whether z is (z != f: hig_quick_gelu_to, else QuickGELU in place).
template <class LayerOf>
int clip_forward(const CDims& D, const void* const* params, const int64_t* tokens, float* out, float* x0, float* stf, LayerOf layer_of,
                 hig_stream_t stream) {
  const Tab P(params, HIG_CT_NGLOBAL, HIG_CTL_NLAYER);
  hipStream_t st = hig_stream(stream);
  const int W = D.W, ff = 4 * D.W;
  const int64_t M = D.M;
  HIG_TRY(hig_clip_embed(P[HIG_CT_TOK_EMB], P[HIG_CT_POS_EMB], tokens, D.B, D.N, W, D.vocab, x0, W, stream));
  const float* xin = x0;
  for (int l = 0; l < D.L; ++l) {
    const CLayer a = layer_of(l);
    HIG_TRY(hig_layernorm(xin, W, M, W, P(l, HIG_CTL_LN1_W), P(l, HIG_CTL_LN1_B), a.h, W, a.st1, stream));
    HIG_TRY(hig_gemm_launch(G(a.h, W, 0, P(l, HIG_CTL_IN_W), W, 0, a.qkv, 3 * W, M, 3 * W, W)
                                .epi(HIG_EPI_BIAS, P(l, HIG_CTL_IN_B)).prec(D.prec).g, 1, nullptr, st));
    if (a.lse)
      HIG_TRY(hig_causal_attn_fwd_train(a.qkv, 3 * W, a.qkv + W, a.qkv + 2 * W, 3 * W, D.B, D.N, D.H, a.att, W, a.lse, stream));
    else
      HIG_TRY(hig_causal_attn_fwd(a.qkv, 3 * W, a.qkv + W, a.qkv + 2 * W, 3 * W, D.B, D.N, D.H, a.att, W, stream));
    HIG_TRY(hig_gemm_launch(G(a.att, W, 0, P(l, HIG_CTL_OUT_W), W, 0, a.x1, W, M, W, W)
                                .epi(HIG_EPI_BIAS_RES, P(l, HIG_CTL_OUT_B)).res(xin, W).prec(D.prec).g, 1, nullptr, st));
    HIG_TRY(hig_layernorm(a.x1, W, M, W, P(l, HIG_CTL_LN2_W), P(l, HIG_CTL_LN2_B), a.h, W, a.st2, stream));
    HIG_TRY(hig_gemm_launch(G(a.h, W, 0, P(l, HIG_CTL_FC_W), W, 0, a.z, ff, M, ff, W)
                                .epi(HIG_EPI_BIAS, P(l, HIG_CTL_FC_B)).prec(D.prec).g, 1, nullptr, st));
    if (a.z != a.f)
      HIG_TRY(hig_quick_gelu_to(a.z, a.f, M * ff, stream));
    else
      HIG_TRY(hig_quick_gelu(a.f, M * ff, stream));
    HIG_TRY(hig_gemm_launch(G(a.f, ff, 0, P(l, HIG_CTL_PROJ_W), ff, 0, a.x2, W, M, W, ff)
                                .epi(HIG_EPI_BIAS_RES, P(l, HIG_CTL_PROJ_B)).res(a.x1, W).prec(D.prec).g, 1, nullptr, st));
    xin = a.x2;
  }
  return hig_layernorm(xin, W, M, W, P[HIG_CT_LNF_W], P[HIG_CT_LNF_B], out, W, stf, stream);
}

}  // namespace

extern "C" int hig_clip_embed(const float* tok_emb, const float* pos_emb, const int64_t* tokens, int32_t B, int32_t N, int32_t W,
                              int32_t vocab, float* out, int64_t ldo, hig_stream_t stream) {
  HIG_REQUIRE(tok_emb && pos_emb && tokens && out, "hig_clip_embed: null argument");
  HIG_REQUIRE(B >= 0 && N > 0 && W > 0 && vocab > 0 && ldo >= W, "hig_clip_embed: bad extent (B=%d N=%d W=%d vocab=%d ldo=%lld)", B, N,
              W, vocab, (long long)ldo);
  if (B == 0) return HIG_OK;
  hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)((int64_t)B * N)), dim3(256), 0, hig_stream(stream), tok_emb, pos_emb, tokens,
                     N, W, vocab, out, ldo);
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}

extern "C" int hig_quick_gelu(float* x, int64_t n, hig_stream_t stream) {
  HIG_REQUIRE(x && n >= 0, "hig_quick_gelu: null argument or negative length");
  if (n == 0) return HIG_OK;
  const int64_t n4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? n / 4 : 0;
  const int64_t items = n4 > 0 ? n4 : n;
  int64_t blocks = (items + 255) / 256;
  const int64_t cap = (int64_t)hig_chip_cus() * 8;   // grid-stride beyond eight workgroups per compute unit
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(quick_gelu_kernel, dim3((unsigned)blocks), dim3(256), 0, hig_stream(stream), x, n4, n);
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}

namespace {
// the one launch site of causal_attn_kernel: lse == NULL is hig_causal_attn_fwd, else hig_causal_attn_fwd_train
int causal_fwd_launch(const float* Q, int64_t ldq, const float* K, const float* V, int64_t ldk, int32_t B, int32_t N, int32_t H, float* Y,
                      int64_t ldy, float* lse, hig_stream_t stream) {
  HIG_REQUIRE(Q && K && V && Y, "hig_causal_attn_fwd: null argument");
  HIG_REQUIRE(B >= 0 && N > 0 && H > 0, "hig_causal_attn_fwd: bad extent (B=%d N=%d H=%d)", B, N, H);
  if (N > CA_NMAX)
    return hig_set_error(HIG_EUNSUPPORTED, "hig_causal_attn_fwd: N=%d, built for N <= %d (head dim 64)", N, CA_NMAX);
  const int64_t d = (int64_t)H * CA_HD;
  HIG_REQUIRE(ldq >= d && ldk >= d && ldy >= d, "hig_causal_attn_fwd: a leading dimension below H * 64 = %lld", (long long)d);
  HIG_REQUIRE((int64_t)B * H <= 0x7fffffff, "hig_causal_attn_fwd: B * H beyond the grid");
  if (B == 0) return HIG_OK;
  const dim3 grid((unsigned)(B * H), (unsigned)((N + CA_QB - 1) / CA_QB));
  const size_t lds = (size_t)2 * N * CA_HD * sizeof(float);   // <= 64 KB
  const bool vec = ((reinterpret_cast<uintptr_t>(K) | reinterpret_cast<uintptr_t>(V)) & 15) == 0 && ldk % 4 == 0;
#define CA_FWD(VECV, LSEV)                                                                                                        \
  hipLaunchKernelGGL((causal_attn_kernel<VECV, LSEV>), grid, dim3(CA_NT), lds, hig_stream(stream), Q, ldq, K, V, ldk, N, H, Y, ldy, lse)
  if (lse) { if (vec) CA_FWD(true, true); else CA_FWD(false, true); }
  else { if (vec) CA_FWD(true, false); else CA_FWD(false, false); }
#undef CA_FWD
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}
}  // namespace

extern "C" int hig_causal_attn_fwd(const float* Q, int64_t ldq, const float* K, const float* V, int64_t ldk, int32_t B, int32_t N,
                                   int32_t H, float* Y, int64_t ldy, hig_stream_t stream) {
  return causal_fwd_launch(Q, ldq, K, V, ldk, B, N, H, Y, ldy, nullptr, stream);
}

extern "C" int hig_causal_attn_fwd_train(const float* Q, int64_t ldq, const float* K, const float* V, int64_t ldk, int32_t B, int32_t N,
                                         int32_t H, float* Y, int64_t ldy, float* lse, hig_stream_t stream) {
  HIG_REQUIRE(lse, "hig_causal_attn_fwd_train: null lse");
  return causal_fwd_launch(Q, ldq, K, V, ldk, B, N, H, Y, ldy, lse, stream);
}

extern "C" int64_t hig_clip_text_workspace_bytes(const int32_t* dims) {
  CDims D;
  if (check_cdims(dims, D) != HIG_OK) return -1;
  return cfwd_layout(D).total * 4;
}
extern "C" int64_t hig_clip_text_train_bytes(const int32_t* dims) {
  CDims D;
  if (check_train(dims, D, "hig_clip_text_train_bytes") != HIG_OK) return -1;
  return ctrain_layout(D).total * 4;
}
extern "C" int64_t hig_clip_text_bwd_workspace_bytes(const int32_t* dims) {
  CDims D;
  if (check_train(dims, D, "hig_clip_text_bwd_workspace_bytes") != HIG_OK) return -1;
  return cbwd_layout(D)[CBW_TOTAL] * 4;
}

extern "C" int hig_clip_text_fwd(const int32_t* dims, const void* const* params, const int64_t* tokens, float* out, void* workspace,
                                 hig_stream_t stream) {
  CDims D;
  HIG_REQUIRE(params, "hig_clip_text_fwd: null params");
  HIG_TRY(check_cdims(dims, D));
  HIG_REQUIRE(tokens && out && workspace, "hig_clip_text_fwd: null argument");
  for (int i = 0; i < HIG_CT_NGLOBAL + D.L * HIG_CTL_NLAYER; ++i) HIG_REQUIRE(params[i], "hig_clip_text_fwd: null parameter %d", i);
  const CFwd w = cfwd_layout(D);
  float* ws = static_cast<float*>(workspace);
  // one statistics buffer, no lse, QuickGELU in place on f
  auto layer_of = [&](int l) {
    float* lb = ws + w.layer0 + (l & 1) * w.block;
    return CLayer{lb + w.h, lb + w.st, lb + w.st, lb + w.qkv, nullptr, lb + w.att, lb + w.x1, lb + w.f, lb + w.f, lb + w.x2};
  };
  return clip_forward(D, params, tokens, out, ws + w.x0, ws + w.stf, layer_of, stream);
}

// ---- training: the forward that keeps what the adjoint needs, and the adjoint ---------------------------------------------------
extern "C" int hig_clip_text_fwd_train(const int32_t* dims, const void* const* params, const int64_t* tokens, float* out, void* saved,
                                       hig_stream_t stream) {
  CDims D;
  HIG_REQUIRE(params, "hig_clip_text_fwd_train: null params");
  HIG_TRY(check_train(dims, D, "hig_clip_text_fwd_train"));
  HIG_REQUIRE(tokens && out && saved, "hig_clip_text_fwd_train: null argument");
  for (int i = 0; i < HIG_CT_NGLOBAL + D.L * HIG_CTL_NLAYER; ++i) HIG_REQUIRE(params[i], "hig_clip_text_fwd_train: null parameter %d", i);
  const CTrain w = ctrain_layout(D);
  float* ws = static_cast<float*>(saved);
  // the launches of hig_clip_text_fwd on the same operand values: the attention also writes lse, and QuickGELU goes from z to
  // f instead of overwriting z
  auto layer_of = [&](int l) {
    float* lb = ws + w.layer0 + l * w.lstride;
    return CLayer{ws + w.h, lb + w.st1, lb + w.st2, lb + w.qkv, lb + w.lse, lb + w.att, lb + w.x1, lb + w.z, ws + w.f, lb + w.x2};
  };
  return clip_forward(D, params, tokens, out, ws + w.x0, ws + w.stf, layer_of, stream);
}

namespace {
// Everything of the adjoint in front of the embedding pass, shared by hig_clip_text_bwd and hig_clip_text_bwd_dev: checks the
// tables and buffers, runs ln_final and the layers in reverse, and leaves d(x0) (B N, W) at *dx0 and the embedding pass's
// scratch at *emb.
int text_bwd_front(const char* who, const int32_t* dims, const void* const* params, const float* dout, const void* saved, void* const* grads,
                   void* bwd_workspace, hig_stream_t stream, CDims& D, const float** dx0, float** emb) {
  HIG_REQUIRE(params && grads, "%s: null table", who);
  HIG_TRY(check_train(dims, D, who));
  HIG_REQUIRE(dout && saved && bwd_workspace, "%s: null argument", who);
  for (int i = 0; i < HIG_CT_NGLOBAL + D.L * HIG_CTL_NLAYER; ++i)
    HIG_REQUIRE(params[i] && grads[i], "%s: null parameter or gradient %d", who, i);
  const CTrain w = ctrain_layout(D);
  const CBwd bw = cbwd_layout(D);
  const Tab P(params, HIG_CT_NGLOBAL, HIG_CTL_NLAYER);
  const Tab Gr(grads, HIG_CT_NGLOBAL, HIG_CTL_NLAYER);
  const float* ws = static_cast<const float*>(saved);
  float* b = static_cast<float*>(bwd_workspace);
  const int W = D.W, ff = 4 * D.W;
  const int64_t M = D.M;
  const EncBwd e(D.enc(), HIG_PREC_F32, b, bw.data(), CBW_SCRATCH, stream);
  float* d = b + bw[CBW_D];      // d(x2 of layer l), then d(its input)
  float* t1 = b + bw[CBW_T1];
  float* t2 = b + bw[CBW_T2];
  float* h = b + bw[CBW_H];
  float* hst = b + bw[CBW_HST];
  float* f = b + bw[CBW_F];
  // ---- ln_final --------------------------------------------------------------------------------------------------------------
  const float* xL = ws + w.layer0 + w.lstride * (D.L - 1) + w.x2;
  HIG_TRY(hig_ln_bwd(dout, W, xL, W, ws + w.stf, P[HIG_CT_LNF_W], P[HIG_CT_LNF_B], nullptr, 0, 0, 0, nullptr, 0, d, W, M,
                     W, D.N, Gr[HIG_CT_LNF_W], Gr[HIG_CT_LNF_B], nullptr, 0, e.lnp, stream));
  for (int l = D.L - 1; l >= 0; --l) {
    const float* lb = ws + w.layer0 + w.lstride * l;
    const float* xin = l == 0 ? ws + w.x0 : ws + w.layer0 + w.lstride * (l - 1) + w.x2;
    auto p = [&](int i) { return P(l, i); };
    auto g = [&](int i) { return Gr(l, i); };
    // x2 = x1 + c_proj(f), f = quick_gelu(z)
    HIG_TRY(hig_quick_gelu_to(lb + w.z, f, M * ff, stream));
    HIG_TRY(e.wgrad_act(d, W, f, ff, g(HIG_CTL_PROJ_W), M, g(HIG_CTL_PROJ_B)));
    HIG_TRY(e.dgrad(d, p(HIG_CTL_PROJ_W), W, ff, M, e.dff, HIG_EPI_NONE, nullptr, nullptr));
    HIG_TRY(hig_quick_gelu_bwd(lb + w.z, e.dff, e.dff, M * ff, stream));                      // dff = d(z)
    // z = c_fc(ln_2(x1))
    HIG_TRY(hig_layernorm(lb + w.x1, W, M, W, p(HIG_CTL_LN2_W), p(HIG_CTL_LN2_B), h, W, hst, stream));
    HIG_TRY(e.wgrad_act(e.dff, ff, h, W, g(HIG_CTL_FC_W), M, g(HIG_CTL_FC_B)));
    HIG_TRY(e.dgrad(e.dff, p(HIG_CTL_FC_W), ff, W, M, t1, HIG_EPI_NONE, nullptr, nullptr));  // t1 = d(ln_2's output)
    HIG_TRY(hig_ln_bwd(t1, W, lb + w.x1, W, lb + w.st2, p(HIG_CTL_LN2_W), p(HIG_CTL_LN2_B), nullptr, 0, 0, 0, d, W, t2, W, M, W, D.N,
                       g(HIG_CTL_LN2_W), g(HIG_CTL_LN2_B), nullptr, 0, e.lnp, stream));    // t2 = d(x1) = d(x2) + the norm's
    // x1 = xin + out_proj(att)
    HIG_TRY(e.wgrad_act(t2, W, lb + w.att, W, g(HIG_CTL_OUT_W), M, g(HIG_CTL_OUT_B)));
    HIG_TRY(e.dgrad(t2, p(HIG_CTL_OUT_W), W, W, M, t1, HIG_EPI_NONE, nullptr, nullptr));     // t1 = d(att)
    const float* qkv = lb + w.qkv;
    HIG_TRY(hig_causal_attn_bwd(t1, W, lb + w.att, W, qkv, 3 * W, qkv + W, qkv + 2 * W, 3 * W, D.B, D.N, D.H, CA_HD, lb + w.lse, e.delta,
                                e.dqkv, 3 * W, e.dqkv + W, e.dqkv + 2 * W, 3 * W, stream));
    // qkv = in_proj(ln_1(xin))
    HIG_TRY(hig_layernorm(xin, W, M, W, p(HIG_CTL_LN1_W), p(HIG_CTL_LN1_B), h, W, hst, stream));
    HIG_TRY(e.wgrad_act(e.dqkv, 3 * W, h, W, g(HIG_CTL_IN_W), M, g(HIG_CTL_IN_B)));
    HIG_TRY(e.dgrad(e.dqkv, p(HIG_CTL_IN_W), 3 * W, W, M, t1, HIG_EPI_NONE, nullptr, nullptr));   // t1 = d(ln_1's output)
    HIG_TRY(hig_ln_bwd(t1, W, xin, W, lb + w.st1, p(HIG_CTL_LN1_W), p(HIG_CTL_LN1_B), nullptr, 0, 0, 0, t2, W, d, W, M, W, D.N,
                       g(HIG_CTL_LN1_W), g(HIG_CTL_LN1_B), nullptr, 0, e.lnp, stream));    // d = d(xin) = d(x1) + the norm's
  }
  *dx0 = d;
  *emb = b + bw[CBW_EMB];
  return HIG_OK;
}
}  // namespace

extern "C" int hig_clip_text_bwd(const int32_t* dims, const void* const* params, const int32_t* index, int32_t n_live, int32_t n_chunks,
                                 int32_t n_ids, const float* dout, const void* saved, void* const* grads, void* bwd_workspace,
                                 hig_stream_t stream) {
  CDims D;
  HIG_REQUIRE(params && grads, "hig_clip_text_bwd: null table");
  HIG_TRY(check_train(dims, D, "hig_clip_text_bwd"));
  HIG_REQUIRE(index && dout && saved && bwd_workspace, "hig_clip_text_bwd: null argument");
  HIG_REQUIRE(n_live >= 0 && n_live <= D.M && n_chunks >= 0 && n_chunks <= n_live && n_ids >= 0 && n_ids <= n_chunks && (n_live == 0) == (n_ids == 0),
              "hig_clip_text_bwd: index counts (live %d, chunks %d, ids %d) that no %lld rows give", n_live, n_chunks, n_ids, (long long)D.M);
  const float* d;
  float* emb;
  HIG_TRY(text_bwd_front("hig_clip_text_bwd", dims, params, dout, saved, grads, bwd_workspace, stream, D, &d, &emb));
  return hig_clip_embed_bwd(d, D.B, D.N, D.W, D.vocab, index, n_live, n_chunks, n_ids, emb, static_cast<float*>(grads[HIG_CT_TOK_EMB]),
                            static_cast<float*>(grads[HIG_CT_POS_EMB]), stream);
}

// the same launches up to d(x0), then the embedding pass on the device-built index (hig_clip_embed_index_build)
extern "C" int hig_clip_text_bwd_dev(const int32_t* dims, const void* const* params, const int32_t* index, const int32_t* counts,
                                     const float* dout, const void* saved, void* const* grads, void* bwd_workspace, hig_stream_t stream) {
  CDims D;
  HIG_REQUIRE(params && grads, "hig_clip_text_bwd_dev: null table");
  HIG_TRY(check_train(dims, D, "hig_clip_text_bwd_dev"));
  HIG_REQUIRE(index && counts && dout && saved && bwd_workspace, "hig_clip_text_bwd_dev: null argument");
  HIG_REQUIRE(((reinterpret_cast<uintptr_t>(index) | reinterpret_cast<uintptr_t>(counts)) & 3) == 0, "hig_clip_text_bwd_dev: unaligned buffer");
  const float* d;
  float* emb;
  HIG_TRY(text_bwd_front("hig_clip_text_bwd_dev", dims, params, dout, saved, grads, bwd_workspace, stream, D, &d, &emb));
  return hig_clip_embed_bwd_dev(d, D.B, D.N, D.W, D.vocab, index, counts, emb, static_cast<float*>(grads[HIG_CT_TOK_EMB]),
                                static_cast<float*>(grads[HIG_CT_POS_EMB]), stream);
}
