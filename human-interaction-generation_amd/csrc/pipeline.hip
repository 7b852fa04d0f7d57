// Kernels either side of the denoiser: batch assembly from the HBM-resident motion
// bank.  Reference arithmetic: Text2MotionMulDataset.__getitem__, codes/datasets/mul_dataset.py:203-209
// (frame gather + Z-normalisation; the init-pose row is normalised on its first 4 features only).
#include "hig_common.h"

namespace {

// One workgroup per (row r, token t): F contiguous floats gathered from frame `frame_ix[r][t]` of the
// sequence starting at bank + seq_off[r].  ST = float or double: the type numpy promoted to when it
// normalised (float64 statistics make numpy compute in double and round once on the store).
template <typename ST>
__global__ __launch_bounds__(256) void gather_frames_kernel(const float* __restrict__ bank,
                                                            const int64_t* __restrict__ seq_off,
                                                            const int32_t* __restrict__ frame_ix,
                                                            const ST* __restrict__ stats, int T, int F,
                                                            float* __restrict__ out) {
  const int r = blockIdx.y, t = blockIdx.x;
  const float* src = bank + seq_off[r] + (int64_t)frame_ix[(int64_t)r * T + t] * F;
  float* dst = out + ((int64_t)r * T + t) * F;
  const ST* mean = stats;
  const ST* sd = stats + F;
  const ST* imean = stats + 2 * F;
  const ST* isd = imean + 4;
  for (int f = threadIdx.x; f < F; f += blockDim.x) {
    const float x = src[f];
    float y;
    if (t == 0)
      y = f < 4 ? (float)(((ST)x - imean[f]) / isd[f]) : x;
    else
      y = (float)(((ST)x - mean[f]) / sd[f]);
    dst[f] = y;
  }
}

// ---- evaluation inputs from generated motions --------------------------------------------
// Reference: EvaluationDataset.__getitem__ / MMGeneratedDataset.__getitem__, codes/datasets/evaluator.py:143-166,
// 346-387, restated on the un-rotated motion (row 0 = init pose, rows 1 .. n = frames, n = m_len - 1), W = T_out - 1:
//   out row 0 = src row 0;   n < W: out row j = src row min(j, n);   n >= W: out row j = src row shift + j.
// One wave per output row, EVAL_ROWS rows per workgroup; a row is F_out contiguous floats out of a source row of F_in.
// 16-byte accesses only on a row whose source AND destination address are both 16-byte aligned (F_in = 263 and
// F_out = 259 / 263 rows are not, three times out of four); plain dword accesses otherwise.  A pure copy either way.
constexpr int EVAL_ROWS = 4;

__global__ __launch_bounds__(64 * EVAL_ROWS) void eval_pairs_build_kernel(
    const float* __restrict__ src, const int64_t* __restrict__ src_off, const int32_t* __restrict__ m_len,
    const int32_t* __restrict__ shift, int N, int F_in, int F_out, int T_out, float* __restrict__ out) {
  const int r = blockIdx.y;                               // person-sample: person 1 of all pairs, then person 2
  const int j = blockIdx.x * EVAL_ROWS + threadIdx.y;     // output row
  if (j >= T_out) return;
  const int pair = r < N ? r : r - N;
  const int n = m_len[pair] - 1, W = T_out - 1;
  const int s = j == 0 ? 0 : (n < W ? (j < n ? j : n) : shift[pair] + j);
  const float* srow = src + src_off[r] + (int64_t)s * F_in;
  float* drow = out + ((int64_t)r * T_out + j) * F_out;
  const int lane = threadIdx.x;
  int done = 0;
  if ((((uintptr_t)srow | (uintptr_t)drow) & 15) == 0) {
    const int nv = F_out >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(srow);
    float4* d4 = reinterpret_cast<float4*>(drow);
    for (int v = lane; v < nv; v += 64) d4[v] = s4[v];
    done = nv << 2;
  }
  for (int f = done + lane; f < F_out; f += 64) drow[f] = srow[f];
}

// ---- post-sampling joint recovery ------------------------------------------------------
// Reference: recover_root_rot_pos / recover_from_ric2 (codes/utils/motion_process.py:362-382, 418-462),
// qinv / qrot (codes/utils/quaternion.py:16-20, 54-73) and the de-normalisation in
// tools/visualization.py:146-152.  One workgroup per person-sample; the two prefix sums over time run
// serially in one lane with a double accumulator (what torch's CPU cumsum does for float tensors).
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 cross3(V3 a, V3 b) {
  return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// v + 2 * (w * (u x v) + u x (u x v)),  q = (w, u)
__device__ __forceinline__ V3 qrot3(float w, V3 u, V3 v) {
  const V3 uv = cross3(u, v);
  const V3 uuv = cross3(u, uv);
  return V3{v.x + 2.f * (w * uv.x + uuv.x), v.y + 2.f * (w * uv.y + uuv.y), v.z + 2.f * (w * uv.z + uuv.z)};
}

__global__ __launch_bounds__(256) void recover_joints_kernel(const float* __restrict__ motion, const float* __restrict__ stats,
                                                             int T, int F, int J, int init_first,
                                                             float* __restrict__ pos) {
  extern __shared__ float sh[];
  float* ang = sh;           // [T] root yaw
  float* px = sh + T;        // [T] root x
  float* pz = sh + 2 * T;    // [T] root z
  float* ry = sh + 3 * T;    // [T] root height
  const int r = blockIdx.x;
  const float* m = motion + (int64_t)r * (T + 1) * F;
  const float* body = m + (init_first ? F : 0);      // T rows of F
  const float* init = m + (init_first ? 0 : (int64_t)T * F);
  const float* mean = stats;
  const float* sd = stats ? stats + F : nullptr;
  auto feat = [&](int t, int f) -> float {
    const float x = body[(int64_t)t * F + f];
    return stats ? x * sd[f] + mean[f] : x;
  };
  auto ifeat = [&](int f) -> float { return stats ? init[f] * stats[2 * F + 4 + f] + stats[2 * F + f] : init[f]; };
  // step 1: yaw[t] = sum_{s<t} rot_vel[s]
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    ang[t] = t > 0 ? feat(t - 1, 0) : 0.f;
    ry[t] = feat(t, 3);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int t = 0; t < T; ++t) {
      acc += (double)ang[t];
      ang[t] = (float)acc;
    }
  }
  __syncthreads();
  // step 2: root XZ velocity of frame t-1 rotated into the world frame, then summed over time
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    V3 v{0.f, 0.f, 0.f};
    if (t > 0) {
      v.x = feat(t - 1, 1);
      v.z = feat(t - 1, 2);
    }
    const V3 w = qrot3(cosf(ang[t]), V3{-0.f, -sinf(ang[t]), -0.f}, v);
    px[t] = w.x;
    pz[t] = w.z;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ax = 0.0, az = 0.0;
    for (int t = 0; t < T; ++t) {
      ax += (double)px[t];
      az += (double)pz[t];
      px[t] = (float)ax;
      pz[t] = (float)az;
    }
  }
  __syncthreads();
  // step 3: every (frame, joint): local -> root-yaw frame -> + root XZ -> init rotation -> + init XZ
  const float q0w = ifeat(2), q0y = ifeat(3), ix = ifeat(0), iz = ifeat(1);
  float* out = pos + (int64_t)r * T * J * 3;
  for (int e = threadIdx.x; e < T * J; e += blockDim.x) {
    const int t = e / J, j = e % J;
    V3 p;
    if (j == 0) {
      p = V3{px[t], ry[t], pz[t]};
    } else {
      const int f = 4 + 3 * (j - 1);
      p = qrot3(cosf(ang[t]), V3{-0.f, -sinf(ang[t]), -0.f}, V3{feat(t, f), feat(t, f + 1), feat(t, f + 2)});
      p.x += px[t];
      p.z += pz[t];
    }
    p = qrot3(q0w, V3{0.f, q0y, 0.f}, p);
    p.x += ix;
    p.z += iz;
    out[(int64_t)e * 3] = p.x;
    out[(int64_t)e * 3 + 1] = p.y;
    out[(int64_t)e * 3 + 2] = p.z;
  }
}

// Bytes of LDS one workgroup of the current device may ask for (hipDeviceAttributeMaxSharedMemoryPerBlock), read once per
// device; 0 when the device cannot be asked.
int lds_bytes_per_workgroup() {
  static int cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  int v = __atomic_load_n(&cache[dev], __ATOMIC_RELAXED);
  if (v == 0) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v < 0) v = 0;
    __atomic_store_n(&cache[dev], v, __ATOMIC_RELAXED);
  }
  return v;
}

}  // namespace

extern "C" int hig_recover_joints(const float* motion, const float* stats, int32_t rows, int32_t T, int32_t F,
                                  int32_t joints, int32_t init_first, float* pos, hig_stream_t stream) {
  HIG_REQUIRE(motion && pos, "hig_recover_joints: null argument");
  HIG_REQUIRE(rows >= 0 && T > 0 && T <= 8192 && joints >= 1 && F >= 4 + 3 * (joints - 1),
              "hig_recover_joints: need 0 < T <= 8192 and F >= 4 + 3 * (joints - 1)");
  if (rows == 0) return HIG_OK;
  // The four per-frame arrays live in dynamic LDS.  The HIP headers ask for no opt-in above a default size on AMD devices
  // (hipFuncAttributeMaxDynamicSharedMemorySize is documented as ignored there), so the device's per-workgroup limit is the
  // whole condition, and it is checked here rather than found out by a launch.
  const size_t lds = (size_t)4 * T * sizeof(float);
  const int lds_max = lds_bytes_per_workgroup();
  HIG_REQUIRE(lds <= (size_t)lds_max, "hig_recover_joints: T = %d needs %zu bytes of LDS, a workgroup of this device has %d", T,
              lds, lds_max);
  hipLaunchKernelGGL(recover_joints_kernel, dim3(rows), dim3(256), lds, hig_stream(stream),
                     motion, stats, T, F, joints, init_first, pos);
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}

extern "C" int hig_eval_pairs_build(const float* src, const int64_t* src_off, const int32_t* m_len, const int32_t* shift,
                                    const int64_t* src_off_host, const int32_t* m_len_host, const int32_t* shift_host,
                                    int64_t src_floats, int32_t N, int32_t F_in, int32_t F_out, int32_t T_out, float* out,
                                    hig_stream_t stream) {
  HIG_REQUIRE(N >= 0 && 2 * (int64_t)N <= 65535, "hig_eval_pairs_build: 0 <= 2 N <= 65535 required");
  if (N == 0) return HIG_OK;
  HIG_REQUIRE(src && src_off && m_len && shift && src_off_host && m_len_host && shift_host && out,
              "hig_eval_pairs_build: null argument");
  HIG_REQUIRE(T_out >= 2 && T_out <= (1 << 20) && F_out >= 1 && F_out <= F_in && F_in <= (1 << 20) && src_floats >= 0,
              "hig_eval_pairs_build: 2 <= T_out <= 2^20, 1 <= F_out <= F_in <= 2^20, src_floats >= 0 required");
  const int W = T_out - 1;
  for (int i = 0; i < N; ++i) {
    const int64_t len = m_len_host[i], sh = shift_host[i], n = len - 1;
    HIG_REQUIRE(len >= 2, "hig_eval_pairs_build: m_len[%d] = %d, need an init-pose row and one frame", i, (int)len);
    HIG_REQUIRE(sh >= 0, "hig_eval_pairs_build: shift[%d] = %d is negative", i, (int)sh);
    HIG_REQUIRE(n < W || sh + W <= n, "hig_eval_pairs_build: shift[%d] = %d puts the window of %d frames past frame %d", i,
                (int)sh, W, (int)n);
    for (int p = 0; p < 2; ++p) {
      const int64_t off = src_off_host[(int64_t)p * N + i];
      HIG_REQUIRE(off >= 0 && off <= src_floats && len * F_in <= src_floats - off,
                  "hig_eval_pairs_build: person %d of pair %d lies outside src[0, src_floats)", p + 1, i);
    }
  }
  const dim3 grid((T_out + EVAL_ROWS - 1) / EVAL_ROWS, 2 * N);
  hipLaunchKernelGGL(eval_pairs_build_kernel, grid, dim3(64, EVAL_ROWS), 0, hig_stream(stream), src, src_off, m_len, shift, N,
                     F_in, F_out, T_out, out);
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}

extern "C" int hig_gather_frames(const float* bank, const int64_t* seq_off, const int32_t* frame_ix,
                                 const void* stats, int32_t stats_f64, int32_t rows, int32_t T, int32_t F,
                                 float* out, hig_stream_t stream) {
  HIG_REQUIRE(bank && seq_off && frame_ix && stats && out, "hig_gather_frames: null argument");
  HIG_REQUIRE(rows >= 0 && T > 0 && F >= 4, "hig_gather_frames: rows >= 0, T > 0, F >= 4 required");
  if (rows == 0) return HIG_OK;
  const dim3 grid(T, rows);
  if (stats_f64)
    hipLaunchKernelGGL(gather_frames_kernel<double>, grid, dim3(256), 0, hig_stream(stream), bank, seq_off, frame_ix,
                       static_cast<const double*>(stats), T, F, out);
  else
    hipLaunchKernelGGL(gather_frames_kernel<float>, grid, dim3(256), 0, hig_stream(stream), bank, seq_off, frame_ix,
                       static_cast<const float*>(stats), T, F, out);
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}
