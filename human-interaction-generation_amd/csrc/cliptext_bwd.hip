// The kernels of the CLIP text tower's adjoint (the launch sequences are in cliptext.hip): the causal attention backward, the
// QuickGELU derivative (and the out-of-place QuickGELU that lets the training forward keep the pre-activation), and the row
// scatter behind the embedding gradient's two segment sums.  Exact fp32, no float atomics, every sum in a fixed order.
#include "hig_common.h"
#include "hig_host.h"

namespace {

constexpr int CB_HD = 64, CB_NMAX = 128, CB_RB = 32, CB_NT = 512;   // the forward's geometry (cliptext.hip: CA_*)

__device__ __forceinline__ float lane_value(float v, int lane) {   // `lane` uniform over the wave
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// Rows sit in LDS at [r][slot ^ (r & 15)] in 16-byte slots, as the forward keeps K: the sixteen lanes of a ds_read_b128 group
// that walk sixteen different rows hit sixteen different slots, and the 64 lanes that read one row's 64 channels (row_at) hit
// 64 different words of its 256 bytes.
// x . row r over the 64 channels, x's channels out of the wave's registers (four partial sums: the forward's key_score)
__device__ __forceinline__ float row_dot(const float* S, int r, float x) {
  const float4* p = reinterpret_cast<const float4*>(S + r * CB_HD);
  const int z = r & 15;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const float4 v = p[s ^ z];
    a0 = fmaf(lane_value(x, 4 * s), v.x, a0);
    a1 = fmaf(lane_value(x, 4 * s + 1), v.y, a1);
    a2 = fmaf(lane_value(x, 4 * s + 2), v.z, a2);
    a3 = fmaf(lane_value(x, 4 * s + 3), v.w, a3);
  }
  return (a0 + a1) + (a2 + a3);
}
__device__ __forceinline__ float row_at(const float* S, int r, int c) { return S[r * CB_HD + 4 * ((c >> 2) ^ (r & 15)) + (c & 3)]; }

// rows r0 .. r1 - 1 of a strided operand's 64-channel head block -> dst[r - r0][.]
template <bool VEC>
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, int64_t ld, int64_t base, int col, int r0, int r1, float* dst) {
  const int rows = r1 - r0;
  if constexpr (VEC) {
    for (int idx = threadIdx.x; idx < rows * 16; idx += CB_NT) {
      const int r = idx >> 4, s = idx & 15;
      const float4 v = *reinterpret_cast<const float4*>(src + (base + r0 + r) * ld + col + 4 * s);
      *reinterpret_cast<float4*>(dst + r * CB_HD + 4 * (s ^ (r & 15))) = v;
    }
  } else {
    for (int idx = threadIdx.x; idx < rows * CB_HD; idx += CB_NT) {
      const int r = idx >> 6, c = idx & 63;
      dst[r * CB_HD + 4 * ((c >> 2) ^ (r & 15)) + (c & 3)] = src[(base + r0 + r) * ld + col + c];
    }
  }
}

// ---- query side: delta_n = sum_l dY_nl Y_nl and dQ_n = sum_{m <= n} dS_nm k_m / 8 -------------------------------------------
// grid (B * H, blocks of CB_RB query rows), eight waves; the workgroup stages K and V rows 0 .. qend - 1 and each wave takes every
// eighth row n of the block.  Lane l owns keys l and l + 64 for the scores (s = q_n . k_m / 8, dP = dY_n . v_m, w = exp(s - lse_n),
// dS = w (dP - delta_n)) and channel l for the sum over the keys, which runs m = 0 .. n in ascending order.  A lane whose key is
// beyond n walks key n and its dS is an exact zero that no sum reads: no K or V row beyond n enters row n.
template <bool VEC>
__global__ __launch_bounds__(CB_NT) void causal_bwd_q_kernel(const float* __restrict__ dY, int64_t lddy, const float* __restrict__ Y,
                                                              int64_t ldy, const float* __restrict__ Q, int64_t ldq,
                                                              const float* __restrict__ K, const float* __restrict__ V, int64_t ldk,
                                                              const float* __restrict__ lse, int N, int H, float* __restrict__ delta,
                                                              float* __restrict__ dQ, int64_t lddq) {
  extern __shared__ __attribute__((aligned(16))) float cb_lds[];
  float* kS = cb_lds;                 // N x 64
  float* vS = cb_lds + N * CB_HD;     // N x 64
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int q0 = blockIdx.y * CB_RB;
  const int qend = min(q0 + CB_RB, N);
  const int64_t base = (int64_t)b * N;
  const int col = h * CB_HD;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  stage_rows<VEC>(K, ldk, base, col, 0, qend, kS);
  stage_rows<VEC>(V, ldk, base, col, 0, qend, vS);
  __syncthreads();
  for (int n = q0 + wave; n < qend; n += CB_NT / 64) {
    const int64_t row = base + n;
    const float q = Q[row * ldq + col + lane], dy = dY[row * lddy + col + lane], y = Y[row * ldy + col + lane];
    const float dl = wave_sum(dy * y);
    const float ls = lse[(int64_t)blockIdx.x * N + n];
    if (lane == 0) delta[(int64_t)blockIdx.x * N + n] = dl;
    const int m0 = min(lane, n);
    const float s0 = row_dot(kS, m0, q) * 0.125f, p0 = row_dot(vS, m0, dy);
    const float ds0 = lane <= n ? __expf(s0 - ls) * (p0 - dl) : 0.f;
    float ds1 = 0.f;
    if (n >= 64) {   // uniform: the second key of every lane exists only from row 64 on
      const int m1 = min(lane + 64, n);
      const float s1 = row_dot(kS, m1, q) * 0.125f, p1 = row_dot(vS, m1, dy);
      ds1 = lane + 64 <= n ? __expf(s1 - ls) * (p1 - dl) : 0.f;
    }
    float acc = 0.f;
    const int hi0 = min(n, 63);
#pragma unroll 8
    for (int m = 0; m <= hi0; ++m) acc = fmaf(lane_value(ds0, m), row_at(kS, m, lane), acc);
#pragma unroll 8
    for (int m = 64; m <= n; ++m) acc = fmaf(lane_value(ds1, m - 64), row_at(kS, m, lane), acc);
    dQ[row * lddq + col + lane] = acc * 0.125f;
  }
}

// ---- key side: dK_m = sum_{n >= m} dS_nm q_n / 8 and dV_m = sum_{n >= m} w_nm dY_n ---------------------------------------------
// grid (B * H, blocks of CB_RB keys), eight waves; the workgroup stages Q and dY rows m0 .. N - 1 and each wave takes every eighth
// key m of the block.  Lane l owns queries m + l and m + l + 64 for the scores and channel l for the two sums over the queries,
// which run n = m .. N - 1 in ascending order.  lse and delta are read at the live rows only: no query row below m enters key m.
template <bool VEC>
__global__ __launch_bounds__(CB_NT) void causal_bwd_kv_kernel(const float* __restrict__ dY, int64_t lddy, const float* __restrict__ Q,
                                                               int64_t ldq, const float* __restrict__ K, const float* __restrict__ V,
                                                               int64_t ldk, const float* __restrict__ lse, const float* __restrict__ delta,
                                                               int N, int H, float* __restrict__ dK, float* __restrict__ dV, int64_t lddk) {
  extern __shared__ __attribute__((aligned(16))) float cb_lds[];
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int m0 = blockIdx.y * CB_RB;
  const int mend = min(m0 + CB_RB, N);
  float* qS = cb_lds;                         // (N - m0) x 64
  float* yS = cb_lds + (N - m0) * CB_HD;      // (N - m0) x 64
  const int64_t base = (int64_t)b * N;
  const int col = h * CB_HD;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  stage_rows<VEC>(Q, ldq, base, col, m0, N, qS);
  stage_rows<VEC>(dY, lddy, base, col, m0, N, yS);
  __syncthreads();
  const float* lse_h = lse + (int64_t)blockIdx.x * N;
  const float* del_h = delta + (int64_t)blockIdx.x * N;
  for (int m = m0 + wave; m < mend; m += CB_NT / 64) {
    const int64_t row = base + m;
    const float k = K[row * ldk + col + lane], v = V[row * ldk + col + lane];
    const int cnt = N - m;   // live queries m .. N - 1
    const int n0 = min(m + lane, N - 1);
    const float s0 = row_dot(qS, n0 - m0, k) * 0.125f, p0 = row_dot(yS, n0 - m0, v);
    const bool live0 = lane < cnt;
    const float w0 = live0 ? __expf(s0 - lse_h[n0]) : 0.f;
    const float ds0 = live0 ? w0 * (p0 - del_h[n0]) : 0.f;
    float w1 = 0.f, ds1 = 0.f;
    if (cnt > 64) {   // uniform
      const int n1 = min(m + lane + 64, N - 1);
      const float s1 = row_dot(qS, n1 - m0, k) * 0.125f, p1 = row_dot(yS, n1 - m0, v);
      const bool live1 = lane + 64 < cnt;
      w1 = live1 ? __expf(s1 - lse_h[n1]) : 0.f;
      ds1 = live1 ? w1 * (p1 - del_h[n1]) : 0.f;
    }
    float ak = 0.f, av = 0.f;
    const int r = m - m0;
    const int c0 = min(cnt, 64);
#pragma unroll 4
    for (int j = 0; j < c0; ++j) {
      ak = fmaf(lane_value(ds0, j), row_at(qS, r + j, lane), ak);
      av = fmaf(lane_value(w0, j), row_at(yS, r + j, lane), av);
    }
#pragma unroll 4
    for (int j = 64; j < cnt; ++j) {
      ak = fmaf(lane_value(ds1, j - 64), row_at(qS, r + j, lane), ak);
      av = fmaf(lane_value(w1, j - 64), row_at(yS, r + j, lane), av);
    }
    dK[row * lddk + col + lane] = ak * 0.125f;
    dV[row * lddk + col + lane] = av;
  }
}

// ---- QuickGELU: y = z s, dy/dz = s (1 + x (1 - s)), x = 1.702 z, s = sigmoid(x) = rcp(1 + exp2(c z)) -------------------------------
__device__ __forceinline__ float quick_gelu_fn(float z) {   // cliptext.hip's quick_gelu, bit for bit
  constexpr float c = (float)(-1.702 * 1.44269504088896340736);
  return z * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z * c));
}
// 1 - s is e s (e = exp(-x)) for x >= 0, where 1 - s would cancel, and 1 - s for x < 0, where e s would overflow
__device__ __forceinline__ float quick_gelu_grad(float z, float dy) {
  constexpr float c = (float)(-1.702 * 1.44269504088896340736);
  const float e = __builtin_amdgcn_exp2f(z * c);
  const float s = __builtin_amdgcn_rcpf(1.0f + e);
  const float x = 1.702f * z;
  const float t = z >= 0.f ? e * s : 1.0f - s;
  return dy * (s * fmaf(x, t, 1.0f));
}
__global__ __launch_bounds__(256) void quick_gelu_to_kernel(const float* __restrict__ z, float* __restrict__ y, int64_t n4, int64_t n) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  const float4* z4 = reinterpret_cast<const float4*>(z);
  float4* y4 = reinterpret_cast<float4*>(y);
  for (int64_t i = gid; i < n4; i += step) {
    float4 v = z4[i];
    v.x = quick_gelu_fn(v.x); v.y = quick_gelu_fn(v.y); v.z = quick_gelu_fn(v.z); v.w = quick_gelu_fn(v.w);
    y4[i] = v;
  }
  for (int64_t i = 4 * n4 + gid; i < n; i += step) y[i] = quick_gelu_fn(z[i]);
}
// dz may be dy: every element is read before it is written, by the thread that writes it
__global__ __launch_bounds__(256) void quick_gelu_bwd_kernel(const float* __restrict__ z, const float* dy, float* dz, int64_t n4, int64_t n) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  const float4* z4 = reinterpret_cast<const float4*>(z);
  const float4* g4 = reinterpret_cast<const float4*>(dy);
  float4* o4 = reinterpret_cast<float4*>(dz);
  for (int64_t i = gid; i < n4; i += step) {
    const float4 v = z4[i], g = g4[i];
    float4 o;
    o.x = quick_gelu_grad(v.x, g.x); o.y = quick_gelu_grad(v.y, g.y); o.z = quick_gelu_grad(v.z, g.z); o.w = quick_gelu_grad(v.w, g.w);
    o4[i] = o;
  }
  for (int64_t i = 4 * n4 + gid; i < n; i += step) dz[i] = quick_gelu_grad(z[i], dy[i]);
}

// ---- dst[ids[u]][:] = src[u][:], u < n_ids; an id outside [0, vocab) writes nothing ---------------------------------------------
// DEVN: n_ids is a capacity (it sizes the grid) and *n_dev the count, kept on the device; rows at or past it are not touched.
template <bool DEVN>
__global__ __launch_bounds__(256) void scatter_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ ids, int n_ids,
                                                            const int32_t* __restrict__ n_dev, int W, int vocab, float* __restrict__ dst) {
  if constexpr (DEVN) {
    const int live = *n_dev;
    n_ids = live < n_ids ? (live < 0 ? 0 : live) : n_ids;
  }
  for (int u = blockIdx.x; u < n_ids; u += gridDim.x) {
    const int id = ids[u];
    if (id < 0 || id >= vocab) continue;
    for (int c = threadIdx.x; c < W; c += blockDim.x) dst[(int64_t)id * W + c] = src[(int64_t)u * W + c];
  }
}

int elementwise_blocks(int64_t items) {
  int64_t blocks = (items + 255) / 256;
  const int64_t cap = (int64_t)hig_chip_cus() * 8;   // grid-stride beyond eight workgroups per compute unit
  return (int)(blocks > cap ? cap : blocks);
}

}  // namespace

extern "C" int hig_causal_attn_bwd(const float* dY, int64_t lddy, const float* Y, int64_t ldy, const float* Q, int64_t ldq, const float* K,
                                   const float* V, int64_t ldk, int32_t B, int32_t N, int32_t H, int32_t hd, const float* lse, float* delta,
                                   float* dQ, int64_t lddq, float* dK, float* dV, int64_t lddk, hig_stream_t stream) {
  HIG_REQUIRE(dY && Y && Q && K && V && lse && delta && dQ && dK && dV, "hig_causal_attn_bwd: null argument");
  HIG_REQUIRE(B >= 0 && N > 0 && H > 0 && hd > 0, "hig_causal_attn_bwd: bad extent (B=%d N=%d H=%d hd=%d)", B, N, H, hd);
  if (hd != CB_HD) return hig_set_error(HIG_EUNSUPPORTED, "hig_causal_attn_bwd: head dim %d, built for 64 only", hd);
  if (N > CB_NMAX) return hig_set_error(HIG_EUNSUPPORTED, "hig_causal_attn_bwd: N=%d, built for N <= %d (head dim 64)", N, CB_NMAX);
  const int64_t d = (int64_t)H * CB_HD;
  HIG_REQUIRE(lddy >= d && ldy >= d && ldq >= d && ldk >= d && lddq >= d && lddk >= d,
              "hig_causal_attn_bwd: a leading dimension below H * 64 = %lld", (long long)d);
  HIG_REQUIRE((int64_t)B * H <= 0x7fffffff, "hig_causal_attn_bwd: B * H beyond the grid");
  if (B == 0) return HIG_OK;
  const dim3 grid((unsigned)(B * H), (unsigned)((N + CB_RB - 1) / CB_RB));
  const size_t lds = (size_t)2 * N * CB_HD * sizeof(float);   // <= 64 KB
  auto vec = [](const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; };
  hipStream_t st = hig_stream(stream);
  if (vec(K, ldk) && vec(V, ldk))
    hipLaunchKernelGGL(causal_bwd_q_kernel<true>, grid, dim3(CB_NT), lds, st, dY, lddy, Y, ldy, Q, ldq, K, V, ldk, lse, N, H, delta, dQ, lddq);
  else
    hipLaunchKernelGGL(causal_bwd_q_kernel<false>, grid, dim3(CB_NT), lds, st, dY, lddy, Y, ldy, Q, ldq, K, V, ldk, lse, N, H, delta, dQ, lddq);
  HIG_CHECK_LAUNCH();
  if (vec(Q, ldq) && vec(dY, lddy))
    hipLaunchKernelGGL(causal_bwd_kv_kernel<true>, grid, dim3(CB_NT), lds, st, dY, lddy, Q, ldq, K, V, ldk, lse, delta, N, H, dK, dV, lddk);
  else
    hipLaunchKernelGGL(causal_bwd_kv_kernel<false>, grid, dim3(CB_NT), lds, st, dY, lddy, Q, ldq, K, V, ldk, lse, delta, N, H, dK, dV, lddk);
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}

extern "C" int hig_quick_gelu_to(const float* z, float* y, int64_t n, hig_stream_t stream) {
  HIG_REQUIRE(z && y && n >= 0, "hig_quick_gelu_to: null argument or negative length");
  if (n == 0) return HIG_OK;
  const int64_t n4 = ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(y)) & 15) == 0 ? n / 4 : 0;
  hipLaunchKernelGGL(quick_gelu_to_kernel, dim3((unsigned)elementwise_blocks(n4 > 0 ? n4 : n)), dim3(256), 0, hig_stream(stream), z, y, n4, n);
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}

extern "C" int hig_quick_gelu_bwd(const float* z, const float* dy, float* dz, int64_t n, hig_stream_t stream) {
  HIG_REQUIRE(z && dy && dz && n >= 0, "hig_quick_gelu_bwd: null argument or negative length");
  if (n == 0) return HIG_OK;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dz);
  const int64_t n4 = (bits & 15) == 0 ? n / 4 : 0;
  hipLaunchKernelGGL(quick_gelu_bwd_kernel, dim3((unsigned)elementwise_blocks(n4 > 0 ? n4 : n)), dim3(256), 0, hig_stream(stream), z, dy, dz,
                     n4, n);
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}

extern "C" int64_t hig_clip_embed_index_ints(int32_t B, int32_t N, int32_t n_live, int32_t n_chunks, int32_t n_ids) {
  if (B < 0 || N <= 0 || n_live < 0 || n_chunks < 0 || n_ids < 0) return -1;
  return (int64_t)n_live + (n_chunks + 1) + n_chunks + (n_ids + 1) + n_ids + (int64_t)B * N + (N + 1);
}

extern "C" int hig_clip_embed_bwd(const float* dx0, int32_t B, int32_t N, int32_t W, int32_t vocab, const int32_t* index, int32_t n_live,
                                  int32_t n_chunks, int32_t n_ids, float* scratch, float* dtok, float* dpos, hig_stream_t stream) {
  HIG_REQUIRE(dx0 && index && scratch && dtok && dpos, "hig_clip_embed_bwd: null argument");
  HIG_REQUIRE(B >= 0 && N > 0 && W > 0 && vocab > 0, "hig_clip_embed_bwd: bad extent (B=%d N=%d W=%d vocab=%d)", B, N, W, vocab);
  const int64_t M = (int64_t)B * N;
  HIG_REQUIRE(M <= 0x7fffffff, "hig_clip_embed_bwd: B * N beyond an int32 row index");
  HIG_REQUIRE(n_live >= 0 && n_live <= M && n_chunks >= 0 && n_chunks <= n_live && n_ids >= 0 && n_ids <= n_chunks && (n_live == 0) == (n_ids == 0),
              "hig_clip_embed_bwd: index counts (live %d, chunks %d, ids %d) that no %lld rows give", n_live, n_chunks, n_ids, (long long)M);
  HIG_REQUIRE((reinterpret_cast<uintptr_t>(index) & 3) == 0 && (reinterpret_cast<uintptr_t>(scratch) & 3) == 0, "hig_clip_embed_bwd: unaligned buffer");
  hipStream_t st = hig_stream(stream);
  // the packed index (include/hig.h): order | chunk_seg | chunk_order | id_seg | ids | pos_order | pos_seg
  const int32_t* order = index;
  const int32_t* chunk_seg = order + n_live;
  const int32_t* chunk_order = chunk_seg + n_chunks + 1;
  const int32_t* id_seg = chunk_order + n_chunks;
  const int32_t* ids = id_seg + n_ids + 1;
  const int32_t* pos_order = ids + n_ids;
  const int32_t* pos_seg = pos_order + M;
  float* partial = scratch;                           // (n_chunks, W)
  float* usum = scratch + (int64_t)n_chunks * W;      // (n_ids, W)
  HIG_TRY(hig_zero_async(dtok, (int64_t)vocab * W * 4, st));
  if (B == 0) return hig_zero_async(dpos, (int64_t)N * W * 4, st);
  HIG_TRY(hig_rows_segment_sum_f32(dx0, (int32_t)M, order, chunk_seg, n_chunks, W, partial, stream));
  HIG_TRY(hig_rows_segment_sum_f32(partial, n_chunks, chunk_order, id_seg, n_ids, W, usum, stream));
  if (n_ids > 0) {
    const int cap = hig_chip_cus() * 8;
    hipLaunchKernelGGL(scatter_rows_kernel<false>, dim3((unsigned)(n_ids < cap ? n_ids : cap)), dim3(256), 0, st, usum, ids, n_ids,
                       (const int32_t*)nullptr, W, vocab, dtok);
    HIG_CHECK_LAUNCH();
  }
  return hig_rows_segment_sum_f32(dx0, (int32_t)M, pos_order, pos_seg, N, W, dpos, stream);
}

extern "C" int64_t hig_clip_embed_bwd_dev_scratch_floats(int32_t B, int32_t N, int32_t W, int32_t vocab) {
  if (B < 0 || N <= 0 || W <= 0 || vocab <= 0 || (int64_t)B * N > 0x7fffffff) return -1;
  const hig_clip_index_layout_t l = hig_clip_index_layout(B, N, vocab);
  return (l.part_rows + l.cap_ids) * W;
}

// hig_clip_embed_bwd on the capacity layout: the same four launches on grids sized by the capacities, each reading its count
// from `counts` on the device.
extern "C" int hig_clip_embed_bwd_dev(const float* dx0, int32_t B, int32_t N, int32_t W, int32_t vocab, const int32_t* index,
                                      const int32_t* counts, float* scratch, float* dtok, float* dpos, hig_stream_t stream) {
  HIG_REQUIRE(dx0 && index && counts && scratch && dtok && dpos, "hig_clip_embed_bwd_dev: null argument");
  HIG_REQUIRE(B >= 0 && N > 0 && W > 0 && vocab > 0, "hig_clip_embed_bwd_dev: bad extent (B=%d N=%d W=%d vocab=%d)", B, N, W, vocab);
  HIG_REQUIRE((int64_t)B * N <= 0x7fffffff, "hig_clip_embed_bwd_dev: B * N beyond an int32 row index");
  HIG_REQUIRE(((reinterpret_cast<uintptr_t>(index) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(scratch)) & 3) == 0,
              "hig_clip_embed_bwd_dev: unaligned buffer");
  const hig_clip_index_layout_t l = hig_clip_index_layout(B, N, vocab);
  HIG_REQUIRE(l.cap_chunks <= 0x7fffffff, "hig_clip_embed_bwd_dev: chunk capacity beyond int32");
  hipStream_t st = hig_stream(stream);
  const int32_t M = (int32_t)l.M, cap_chunks = (int32_t)l.part_rows, cap_ids = (int32_t)l.cap_ids;
  float* partial = scratch;                              // (part_rows, W)
  float* usum = scratch + l.part_rows * W;               // (cap_ids, W)
  HIG_TRY(hig_zero_async(dtok, (int64_t)vocab * W * 4, st));
  if (B == 0) return hig_zero_async(dpos, (int64_t)N * W * 4, st);
  HIG_TRY(hig_rows_segment_sum_dev(dx0, M, index + l.order, index + l.chunk_seg, cap_chunks, counts + 1, W, partial, stream));
  HIG_TRY(hig_rows_segment_sum_dev(partial, cap_chunks, index + l.chunk_order, index + l.id_seg, cap_ids, counts + 2, W, usum, stream));
  const int cap = hig_chip_cus() * 8;
  hipLaunchKernelGGL(scatter_rows_kernel<true>, dim3((unsigned)(cap_ids < cap ? cap_ids : cap)), dim3(256), 0, st, usum, index + l.ids,
                     cap_ids, counts + 2, W, vocab, dtok);
  HIG_CHECK_LAUNCH();
  return hig_rows_segment_sum_f32(dx0, M, index + l.pos_order, index + l.pos_seg, N, W, dpos, stream);
}
