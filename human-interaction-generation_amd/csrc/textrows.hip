// Whole-row movement for the caption bank (models/caption_bank.py): the text side of a training step runs once per DISTINCT
// caption, so rows are fetched from the bank by slot, expanded to the model batch by index, and the two upstream gradients
// are summed back to one row per distinct caption.
//     hig_rows_gather_f32        dst[r][:] = src[idx[r]][:]
//     hig_caption_gather         the same gather plus eot[r] = eot_src[slot[r]], one launch
//     hig_rows_segment_sum_f32   dst[u][:] = sum over j in [seg[u], seg[u+1]) of src[order[j]][:], in list order
// All three share one work split.  A row is cut into `parts` column ranges and a work item is (row, part); workgroups stride
// over the items, and the grid is sized from the chip (eight workgroups per compute unit at most), not from the row count: five
// rows of 39 424 floats and 1 300 rows of 2 048 floats both fill the chip.  The row of an item is uniform over its workgroup, so
// its index is one scalar load per item, never one per element.  VEC: row_floats % 4 == 0 and both bases 16-byte aligned ->
// every row starts 16-byte aligned and a thread moves float4; otherwise the same loop moves single floats (the same bits).
#include <math.h>

#include "hig_common.h"
#include "hig_host.h"

namespace {

constexpr int TR_NT = 256;

template <bool VEC>
struct RowElem { using type = float; };
template <>
struct RowElem<true> { using type = float4; };

__device__ __forceinline__ float tr_nan(float) { return __builtin_nanf(""); }
__device__ __forceinline__ float4 tr_nan(float4) { const float q = __builtin_nanf(""); return make_float4(q, q, q, q); }
__device__ __forceinline__ float tr_add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 tr_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float tr_zero(float) { return 0.f; }
__device__ __forceinline__ float4 tr_zero(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }

// nvec: elements (float4 or float) per row.  An index outside [0, n_src) reads nothing: the row becomes quiet NaN (and its eot
// 0, a token every caption has), so a plumbing bug shows in the loss instead of faulting.  eot_src / eot NULL: the plain gather.
template <bool VEC>
__global__ __launch_bounds__(TR_NT) void rows_gather_kernel(const float* __restrict__ src, int n_src, const int32_t* __restrict__ idx,
                                                            int n_out, int64_t nvec, int parts, float* __restrict__ dst,
                                                            const int64_t* __restrict__ eot_src, int64_t* __restrict__ eot) {
  using E = typename RowElem<VEC>::type;
  const int64_t items = (int64_t)n_out * parts;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int r = (int)(item / parts), part = (int)(item % parts);
    const int s = idx[r];
    const bool live = s >= 0 && s < n_src;
    const E* in = reinterpret_cast<const E*>(src) + (live ? (int64_t)s : 0) * nvec;
    E* out = reinterpret_cast<E*>(dst) + (int64_t)r * nvec;
    const int64_t step = (int64_t)parts * TR_NT;
    if (live) {
#pragma unroll 4
      for (int64_t c = (int64_t)part * TR_NT + threadIdx.x; c < nvec; c += step) out[c] = in[c];
    } else {
      for (int64_t c = (int64_t)part * TR_NT + threadIdx.x; c < nvec; c += step) out[c] = tr_nan(E{});
    }
    if (eot && part == 0 && threadIdx.x == 0) eot[r] = live ? eot_src[s] : 0;
  }
}

// One thread per (segment, column): it walks its segment's list and adds in list order, starting from the first member, so
// the sum is the same bits on every run and for every grid.  No atomics; rows that `order` does not name are never read.  The
// lists here are short and even (at most about 1 300 rows over 44 segments, the captions of one step), so the chunked form
// that splits long lists over several waves would buy nothing: one walker per column it is.  An entry of `order` outside
// [0, n_src) reads nothing and contributes NaN.
// DEVN: n_seg is a capacity (it sizes the launch) and *n_dev the number of segments, a count that lives on the device
// (hig_clip_embed_index_build); items at or past it exit without a read or a write.  A segment's sum does not depend on the flag.
template <bool VEC, bool DEVN>
__global__ __launch_bounds__(TR_NT) void rows_segment_sum_kernel(const float* __restrict__ src, int n_src,
                                                                 const int32_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                                 int n_seg, const int32_t* __restrict__ n_dev, int64_t nvec, int parts,
                                                                 float* __restrict__ dst) {
  using E = typename RowElem<VEC>::type;
  if constexpr (DEVN) {
    const int live = *n_dev;
    n_seg = live < n_seg ? (live < 0 ? 0 : live) : n_seg;
  }
  const int64_t items = (int64_t)n_seg * parts;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int u = (int)(item / parts), part = (int)(item % parts);
    int lo = seg[u];
    const int hi = seg[u + 1];
    lo = lo < 0 ? 0 : lo;
    const E* in = reinterpret_cast<const E*>(src);
    E* out = reinterpret_cast<E*>(dst) + (int64_t)u * nvec;
    const int64_t step = (int64_t)parts * TR_NT;
    for (int64_t c = (int64_t)part * TR_NT + threadIdx.x; c < nvec; c += step) {
      E acc = tr_zero(E{});
      for (int j = lo; j < hi; ++j) {
        const int s = order[j];
        const E v = (s >= 0 && s < n_src) ? in[(int64_t)s * nvec + c] : tr_nan(E{});
        acc = j == lo ? v : tr_add(acc, v);
      }
      out[c] = acc;
    }
  }
}

// dst[k][:] = the rows r of src with key[r] == k, added in ascending r starting from the first member: the sum by class id of
// the class head (classhead.hip), whose step copies the ids to the device and builds no index on the host.  One wave per
// workgroup and one (key, `width` columns) item at a time.  The wave reads the keys once, a chunk of HIG_ROWS_KEY_CHUNK rows
// at a time, 64 keys per load; a ballot keeps the members' order, and the chunk's member rows go to LDS as an ascending list,
// which the wave then walks four rows at a time (the loads are independent, the adds stay in row order).  No atomics; a row
// whose key no item owns -- any key outside [0, n_keys) -- is never read; a key without rows stores +0.0.
constexpr int BK_NT = 64;

template <bool VEC>
__global__ __launch_bounds__(BK_NT) void rows_sum_by_key_kernel(const float* __restrict__ src, const int32_t* __restrict__ key, int rows,
                                                                int64_t nvec, int n_keys, int parts, int width, float* __restrict__ dst) {
  using E = typename RowElem<VEC>::type;
  __shared__ int32_t members[HIG_ROWS_KEY_CHUNK];
  const int lane = threadIdx.x;
  const int64_t items = (int64_t)n_keys * parts;
  const E* in = reinterpret_cast<const E*>(src);
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int k = (int)(item / parts), part = (int)(item % parts);
    const int64_t c = (int64_t)part * width + lane;
    const bool active = lane < width && c < nvec;
    E acc = tr_zero(E{});
    bool any = false;
    for (int64_t r0 = 0; r0 < rows; r0 += HIG_ROWS_KEY_CHUNK) {
      const int nr = rows - r0 < HIG_ROWS_KEY_CHUNK ? (int)(rows - r0) : HIG_ROWS_KEY_CHUNK;
      int count = 0;
      for (int b = 0; b < nr; b += BK_NT) {
        const int j = b + lane;
        const bool m = j < nr && key[r0 + j] == k;
        const unsigned long long mask = __ballot(m);
        if (m) members[count + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)(r0 + j);
        count += __popcll(mask);
      }
      __syncthreads();
      if (active) {
        int i = 0;
        for (; i + 4 <= count; i += 4) {
          const E v0 = in[(int64_t)members[i] * nvec + c], v1 = in[(int64_t)members[i + 1] * nvec + c];
          const E v2 = in[(int64_t)members[i + 2] * nvec + c], v3 = in[(int64_t)members[i + 3] * nvec + c];
          acc = any ? tr_add(acc, v0) : v0;
          acc = tr_add(tr_add(tr_add(acc, v1), v2), v3);
          any = true;
        }
        for (; i < count; ++i) {
          const E v = in[(int64_t)members[i] * nvec + c];
          acc = any ? tr_add(acc, v) : v;
          any = true;
        }
      }
      __syncthreads();   // the next chunk, or the next item, rewrites the list
    }
    if (active) reinterpret_cast<E*>(dst)[(int64_t)k * nvec + c] = acc;
  }
}

struct RowSplit { bool vec; int64_t nvec; int parts, grid; };

// parts: as many column ranges per row as it takes to put eight workgroups on every compute unit, at most one range per TR_NT
// elements; grid: the items, capped at that target (the kernels stride over the rest).
RowSplit row_split(const void* a, const void* b, int64_t rows, int64_t row_floats) {
  RowSplit s;
  s.vec = row_floats % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
  s.nvec = s.vec ? row_floats / 4 : row_floats;
  const int64_t target = (int64_t)hig_chip_cus() * 8;
  const int64_t parts_max = (s.nvec + TR_NT - 1) / TR_NT;
  int64_t parts = (target + rows - 1) / rows;
  parts = parts < 1 ? 1 : (parts > parts_max ? parts_max : parts);
  const int64_t items = rows * parts;
  s.parts = (int)parts;
  s.grid = (int)(items < target ? items : target);
  return s;
}

int gather_launch(const char* who, const float* src, int32_t n_src, const int32_t* idx, int32_t n_out, int64_t row_floats, float* dst,
                  const int64_t* eot_src, int64_t* eot, hig_stream_t stream) {
  HIG_REQUIRE(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(idx)) & 3) == 0 &&
              ((reinterpret_cast<uintptr_t>(eot_src) | reinterpret_cast<uintptr_t>(eot)) & 7) == 0,
              "%s: float / int32 pointers must be 4-byte aligned, int64 pointers 8-byte aligned", who);
  HIG_REQUIRE(row_floats < ((int64_t)1 << 40), "%s: row_floats %lld is out of range", who, (long long)row_floats);
  if (n_out == 0 || (row_floats == 0 && !eot)) return HIG_OK;
  const RowSplit s = row_split(src, dst, n_out, row_floats > 0 ? row_floats : 1);
  const int64_t nvec = row_floats > 0 ? s.nvec : 0;
  if (s.vec)
    hipLaunchKernelGGL(rows_gather_kernel<true>, dim3(s.grid), dim3(TR_NT), 0, hig_stream(stream), src, (int)n_src, idx, (int)n_out, nvec,
                       s.parts, dst, eot_src, eot);
  else
    hipLaunchKernelGGL(rows_gather_kernel<false>, dim3(s.grid), dim3(TR_NT), 0, hig_stream(stream), src, (int)n_src, idx, (int)n_out, nvec,
                       s.parts, dst, eot_src, eot);
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}

}  // namespace

extern "C" int hig_rows_gather_f32(const float* src, int32_t n_src, const int32_t* idx, int32_t n_out, int64_t row_floats, float* dst,
                                   hig_stream_t stream) {
  HIG_REQUIRE(src && idx && dst, "hig_rows_gather_f32: src, idx and dst must be non-null");
  HIG_REQUIRE(n_src >= 0 && n_out >= 0 && row_floats >= 0, "hig_rows_gather_f32: negative size (n_src %d, n_out %d, row_floats %lld)",
              (int)n_src, (int)n_out, (long long)row_floats);
  return gather_launch("hig_rows_gather_f32", src, n_src, idx, n_out, row_floats, dst, nullptr, nullptr, stream);
}

extern "C" int hig_caption_gather(const float* feat, const int64_t* eot_src, int32_t n_slots, const int32_t* slot, int32_t rows,
                                  int64_t row_floats, float* clip_out, int64_t* eot, hig_stream_t stream) {
  HIG_REQUIRE(feat && eot_src && slot && clip_out && eot, "hig_caption_gather: feat, eot_src, slot, clip_out and eot must be non-null");
  HIG_REQUIRE(n_slots >= 0 && rows >= 0 && row_floats >= 0, "hig_caption_gather: negative size (n_slots %d, rows %d, row_floats %lld)",
              (int)n_slots, (int)rows, (long long)row_floats);
  return gather_launch("hig_caption_gather", feat, n_slots, slot, rows, row_floats, clip_out, eot_src, eot, stream);
}

namespace {
// the one launch site of rows_segment_sum_kernel: n_dev == NULL is hig_rows_segment_sum_f32, else hig_rows_segment_sum_dev
int segment_sum_launch(const float* src, int32_t n_src, const int32_t* order, const int32_t* seg, int32_t n_seg, const int32_t* n_dev,
                       int64_t row_floats, float* dst, hig_stream_t stream) {
  const RowSplit s = row_split(src, dst, n_seg, row_floats);
#define TR_SEG(VECV, DEVV)                                                                                                        \
  hipLaunchKernelGGL((rows_segment_sum_kernel<VECV, DEVV>), dim3(s.grid), dim3(TR_NT), 0, hig_stream(stream), src, (int)n_src, order, seg, \
                     (int)n_seg, n_dev, s.nvec, s.parts, dst)
  if (n_dev) { if (s.vec) TR_SEG(true, true); else TR_SEG(false, true); }
  else { if (s.vec) TR_SEG(true, false); else TR_SEG(false, false); }
#undef TR_SEG
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}
}  // namespace

extern "C" int hig_rows_segment_sum_f32(const float* src, int32_t n_src, const int32_t* order, const int32_t* seg, int32_t n_seg,
                                        int64_t row_floats, float* dst, hig_stream_t stream) {
  HIG_REQUIRE(src && order && seg && dst, "hig_rows_segment_sum_f32: src, order, seg and dst must be non-null");
  HIG_REQUIRE(n_src >= 0 && n_seg >= 0 && row_floats >= 0, "hig_rows_segment_sum_f32: negative size (n_src %d, n_seg %d, row_floats %lld)",
              (int)n_src, (int)n_seg, (long long)row_floats);
  HIG_REQUIRE(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(order) |
                reinterpret_cast<uintptr_t>(seg)) & 3) == 0, "hig_rows_segment_sum_f32: pointers must be 4-byte aligned");
  HIG_REQUIRE(row_floats < ((int64_t)1 << 40), "hig_rows_segment_sum_f32: row_floats %lld is out of range", (long long)row_floats);
  if (n_seg == 0 || row_floats == 0) return HIG_OK;
  return segment_sum_launch(src, n_src, order, seg, n_seg, nullptr, row_floats, dst, stream);
}

// hig_host.h: the same sum over the first *n_seg_dev of cap_seg segments; the grid is sized by cap_seg, so the launch does not
// depend on the count and a captured graph serves every batch.  Arguments are the caller's (cliptext_bwd.hip), checked there.
int hig_rows_segment_sum_dev(const float* src, int32_t n_src, const int32_t* order, const int32_t* seg, int32_t cap_seg,
                             const int32_t* n_seg_dev, int64_t row_floats, float* dst, hig_stream_t stream) {
  HIG_REQUIRE(src && order && seg && n_seg_dev && dst && n_src >= 0 && cap_seg >= 0 && row_floats >= 0,
              "hig_rows_segment_sum_dev: null argument or negative size");
  if (cap_seg == 0 || row_floats == 0) return HIG_OK;
  return segment_sum_launch(src, n_src, order, seg, cap_seg, n_seg_dev, row_floats, dst, stream);
}

// The only parallelism is keys x columns (a key's rows are added in order by one lane per column), so the column range of an
// item narrows from a full wave (64 elements) down to 16 (256 contiguous bytes per row as float4) until there are four
// one-wave items per compute unit or the ranges cannot narrow further: 43 keys of 2 048 floats give 1 376 items, 43 keys of
// 256 floats 172.  The grid is the items, capped at 32 per compute unit (the kernel strides over the rest).
extern "C" int hig_rows_sum_by_key_f32(const float* src, const int32_t* key, int32_t rows, int64_t row_floats, int32_t n_keys, float* dst,
                                       hig_stream_t stream) {
  HIG_REQUIRE(src && key && dst, "hig_rows_sum_by_key_f32: src, key and dst must be non-null");
  HIG_REQUIRE(rows > 0 && row_floats > 0 && n_keys > 0, "hig_rows_sum_by_key_f32: sizes must be positive (rows %d, row_floats %lld, n_keys %d)",
              (int)rows, (long long)row_floats, (int)n_keys);
  HIG_REQUIRE(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(key)) & 3) == 0,
              "hig_rows_sum_by_key_f32: pointers must be 4-byte aligned");
  HIG_REQUIRE(row_floats < ((int64_t)1 << 32), "hig_rows_sum_by_key_f32: row_floats %lld is out of range", (long long)row_floats);
  const bool vec = row_floats % 4 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  const int64_t nvec = vec ? row_floats / 4 : row_floats;
  const int64_t cus = hig_chip_cus();
  int width = BK_NT;
  while (width > 16 && (int64_t)n_keys * ((nvec + width - 1) / width) < 4 * cus) width /= 2;
  const int64_t parts = (nvec + width - 1) / width;
  const int64_t items = (int64_t)n_keys * parts;
  const int grid = (int)(items < 32 * cus ? items : 32 * cus);
  if (vec)
    hipLaunchKernelGGL(rows_sum_by_key_kernel<true>, dim3(grid), dim3(BK_NT), 0, hig_stream(stream), src, key, (int)rows, nvec, (int)n_keys,
                       (int)parts, width, dst);
  else
    hipLaunchKernelGGL(rows_sum_by_key_kernel<false>, dim3(grid), dim3(BK_NT), 0, hig_stream(stream), src, key, (int)rows, nvec, (int)n_keys,
                       (int)parts, width, dst);
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}
