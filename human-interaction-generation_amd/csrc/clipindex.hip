// The embedding-gradient index of the CLIP text tower, built on the device from the tokens (include/hig.h,
// hig_clip_embed_index_build): what models/clip_text.py's EmbedIndex builds on the host, in a capacity layout whose offsets
// depend on (B, N, vocab) only, with the three counts left on the device.  One workgroup: the rows are sorted by the key
// id << 16 | row (all live keys are distinct, so the sorted order IS "ids ascending, rows ascending inside an id"; a row whose id
// lies outside [0, vocab) gets 0xFFFFFFFF and sorts behind every live one), then three block scans find the id boundaries,
// the chunk cuts and the counts.  Integer work only; no atomics; the launch is a function of (B, N, vocab).
#include "hig_common.h"
#include "hig_host.h"

namespace {

constexpr int IX_NT = 1024;
constexpr int IX_TILE = 32768;            // keys sorted in LDS at a time: 128 KiB of the compute unit's 160
constexpr uint32_t IX_DEAD = 0xFFFFFFFFu;
constexpr int64_t IX_MAX_ROWS = 65535;    // row < 2^16, and (65535 << 16 | 65535) is the dead key
constexpr int64_t IX_MAX_VOCAB = 65536;

// one compare-exchange pass (k, j) of the bitonic network over `count` keys whose first has the global index g0
__device__ __forceinline__ void bitonic_pass(uint32_t* s, int count, int g0, int k, int j) {
  for (int p = threadIdx.x; p < (count >> 1); p += IX_NT) {
    const int lo = p & (j - 1);
    const int i = ((p - lo) << 1) + lo;
    const uint32_t a = s[i], b = s[i + j];
    const bool asc = ((g0 + i) & k) == 0;
    if ((a > b) == asc) { s[i] = b; s[i + j] = a; }
  }
}

// exclusive scan of one int per thread over the workgroup (sum, or max with -1 in front); buf: 2 * IX_NT ints
template <bool MAX>
__device__ __forceinline__ int block_scan_excl(int v, int* buf, int* total) {
  const int t = threadIdx.x;
  int* a = buf;
  int* b = buf + IX_NT;
  a[t] = v;
  __syncthreads();
  for (int d = 1; d < IX_NT; d <<= 1) {
    int x = a[t];
    if (t >= d) x = MAX ? max(x, a[t - d]) : x + a[t - d];
    b[t] = x;
    __syncthreads();
    int* c = a; a = b; b = c;
  }
  *total = a[IX_NT - 1];
  const int ex = t > 0 ? a[t - 1] : (MAX ? -1 : 0);
  __syncthreads();
  return ex;
}

// P: the padded key count (a power of two >= max(M, 2)); tile = min(P, IX_TILE) keys of dynamic LDS; skeys: P keys of scratch.
__global__ __launch_bounds__(IX_NT) void clip_index_build_kernel(const int64_t* __restrict__ tokens, int M, int B, int N, int vocab, int P,
                                                                 int tile, uint32_t* skeys, int32_t* __restrict__ order,
                                                                 int32_t* __restrict__ chunk_seg, int32_t* __restrict__ chunk_order,
                                                                 int32_t* __restrict__ id_seg, int32_t* __restrict__ ids,
                                                                 int32_t* __restrict__ pos_order, int32_t* __restrict__ pos_seg,
                                                                 int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t ix_keys[];
  __shared__ int ix_scan[2 * IX_NT];
  __shared__ int ix_live;
  const int tid = threadIdx.x;
  // ---- the position side does not depend on the tokens: pos_order is n-major, pos_seg = 0, B, 2 B, ... ------------------------------
  for (int i = tid; i < M; i += IX_NT) {
    const int n = i / B, b = i - n * B;
    pos_order[i] = b * N + n;
  }
  for (int n = tid; n <= N; n += IX_NT) pos_seg[n] = n * B;
  if (tid == 0) ix_live = 0;
  // ---- sort: every tile on its own in LDS (directions by the global index), then the merges across tiles ----------------------------
  for (int g0 = 0; g0 < P; g0 += tile) {
    for (int i = tid; i < tile; i += IX_NT) {
      const int r = g0 + i;
      uint32_t key = IX_DEAD;
      if (r < M) {
        const int64_t t = tokens[r];
        if (t >= 0 && t < vocab) key = ((uint32_t)t << 16) | (uint32_t)r;
      }
      ix_keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= tile; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        bitonic_pass(ix_keys, tile, g0, k, j);
        __syncthreads();
      }
    for (int i = tid; i < tile; i += IX_NT) skeys[g0 + i] = ix_keys[i];
    __syncthreads();
  }
  for (int k = tile << 1; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= tile; j >>= 1) {   // partners in different tiles: through the scratch
      bitonic_pass(skeys, P, 0, k, j);
      __syncthreads();
    }
    for (int g0 = 0; g0 < P; g0 += tile) {
      for (int i = tid; i < tile; i += IX_NT) ix_keys[i] = skeys[g0 + i];
      __syncthreads();
      for (int j = tile >> 1; j > 0; j >>= 1) {
        bitonic_pass(ix_keys, tile, g0, k, j);
        __syncthreads();
      }
      for (int i = tid; i < tile; i += IX_NT) skeys[g0 + i] = ix_keys[i];
      __syncthreads();
    }
  }
  // ---- the index: thread t owns the sorted positions [lo, hi) -------------------------------------------------------------------------
  const int per = (M + IX_NT - 1) / IX_NT;
  const int lo = min(tid * per, M), hi = min(lo + per, M);
  // A: heads (the first row of an id) in the range, and the last of them
  int heads = 0, last_head = -1;
  for (int i = lo; i < hi; ++i) {
    const uint32_t key = skeys[i];
    if (key == IX_DEAD) break;   // sorted: every key behind a dead one is dead
    const bool head = i == 0 || (skeys[i - 1] >> 16) != (key >> 16);
    if (head) { ++heads; last_head = i; }
    if (i + 1 == M || skeys[i + 1] == IX_DEAD) ix_live = i + 1;   // one thread at most
  }
  int n_ids, unused;
  const int u0 = block_scan_excl<false>(heads, ix_scan, &n_ids);
  const int start0 = block_scan_excl<true>(last_head, ix_scan, &unused);   // the head of the list that is open at `lo`
  // B: chunk cuts in the range: every HIG_CLIP_EMBED_CHUNK-th row of an id's list, from its head
  int cuts = 0, start = start0;
  for (int i = lo; i < hi; ++i) {
    const uint32_t key = skeys[i];
    if (key == IX_DEAD) break;
    if (i == 0 || (skeys[i - 1] >> 16) != (key >> 16)) start = i;
    if (((i - start) % HIG_CLIP_EMBED_CHUNK) == 0) ++cuts;
  }
  int n_chunks;
  const int c0 = block_scan_excl<false>(cuts, ix_scan, &n_chunks);
  // C: write
  int u = u0, c = c0;
  start = start0;
  for (int i = lo; i < hi; ++i) {
    const uint32_t key = skeys[i];
    if (key == IX_DEAD) break;
    order[i] = (int32_t)(key & 0xFFFFu);
    if (i == 0 || (skeys[i - 1] >> 16) != (key >> 16)) {
      start = i;
      ids[u] = (int32_t)(key >> 16);
      id_seg[u] = c;
      ++u;
    }
    if (((i - start) % HIG_CLIP_EMBED_CHUNK) == 0) {
      chunk_seg[c] = i;
      chunk_order[c] = c;
      ++c;
    }
  }
  if (tid == 0) {
    const int n_live = ix_live;   // (the scans' barriers lie between its one write and this read)
    counts[0] = n_live;
    counts[1] = n_chunks;
    counts[2] = n_ids;
    id_seg[n_ids] = n_chunks;
    chunk_seg[n_chunks] = n_live;
  }
}

int padded_keys(int64_t M) {
  int P = 2;
  while (P < M) P <<= 1;
  return P;
}

// HIG_OK when the entry covers (B, N, vocab); the error it returns otherwise
int check_index_shape(const char* who, int32_t B, int32_t N, int32_t vocab) {
  HIG_REQUIRE(B >= 0 && N > 0 && vocab > 0, "%s: bad extent (B=%d N=%d vocab=%d)", who, B, N, vocab);
  if ((int64_t)B * N > IX_MAX_ROWS || vocab > IX_MAX_VOCAB)
    return hig_set_error(HIG_EUNSUPPORTED, "%s: B N = %lld rows, vocab %d; the keys cover B N <= %lld and vocab <= %lld", who,
                         (long long)B * N, vocab, (long long)IX_MAX_ROWS, (long long)IX_MAX_VOCAB);
  return HIG_OK;
}

}  // namespace

extern "C" int64_t hig_clip_embed_index_cap_ints(int32_t B, int32_t N, int32_t vocab) {
  if (B < 0 || N <= 0 || vocab <= 0 || (int64_t)B * N > 0x7fffffff) return -1;
  return hig_clip_index_layout(B, N, vocab).total;
}

extern "C" int64_t hig_clip_embed_index_scratch_bytes(int32_t B, int32_t N, int32_t vocab) {
  if (check_index_shape("hig_clip_embed_index_scratch_bytes", B, N, vocab) != HIG_OK) return -1;
  return (int64_t)padded_keys((int64_t)B * N) * 4;
}

extern "C" int hig_clip_embed_index_build(const int64_t* tokens, int32_t B, int32_t N, int32_t vocab, int32_t* index, int32_t* counts,
                                          void* scratch, hig_stream_t stream) {
  HIG_REQUIRE(tokens && index && counts && scratch, "hig_clip_embed_index_build: null argument");
  HIG_TRY(check_index_shape("hig_clip_embed_index_build", B, N, vocab));
  HIG_REQUIRE((reinterpret_cast<uintptr_t>(tokens) & 7) == 0 &&
                  ((reinterpret_cast<uintptr_t>(index) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(scratch)) & 3) == 0,
              "hig_clip_embed_index_build: unaligned buffer");
  const hig_clip_index_layout_t l = hig_clip_index_layout(B, N, vocab);
  const int P = padded_keys(l.M);
  const int tile = P < IX_TILE ? P : IX_TILE;
  static const int big_lds_rc = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&clip_index_build_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               IX_TILE * 4) == hipSuccess ? 0 : 1;
  }();
  if (big_lds_rc != 0) return hig_set_error(HIG_EHIP, "hig_clip_embed_index_build: cannot reserve %d bytes of LDS", IX_TILE * 4);
  hipLaunchKernelGGL(clip_index_build_kernel, dim3(1), dim3(IX_NT), (size_t)tile * 4, hig_stream(stream), tokens, (int)l.M, (int)B, (int)N,
                     (int)vocab, P, tile, static_cast<uint32_t*>(scratch), index + l.order, index + l.chunk_seg, index + l.chunk_order,
                     index + l.id_seg, index + l.ids, index + l.pos_order, index + l.pos_seg, counts);
  HIG_CHECK_LAUNCH();
  return HIG_OK;
}
