// Launch sequences of the class head of a cap_id model (reference: get_class_embedding, codes/models/interaction_transformer.py:
// 558-563): xf_out = cap_embedding[ids], xf_proj = text_proj(cap_embedding[ids]).  The head is computed per CLASS, not per row:
// text_proj runs once over the C rows of the table and the model batch fetches its rows by id; backward, the two upstream
// gradients are summed by id (hig_rows_sum_by_key_f32: in row order, no atomics, no host-built index) and the three parameter
// gradients follow from the (C, .) sums.  Host code only (kernels live in gemm / rowops / textrows); hipGraph-capturable.
#include "hig_common.h"
#include "hig_host.h"

namespace {

struct CDims { int C, Lt, E; };

int check_cdims(int32_t C, int32_t Lt, int32_t E, const char* who, CDims& D) {
  HIG_REQUIRE(C > 0 && Lt > 0 && E > 0, "%s: every extent must be positive (C %d, Lt %d, E %d)", who, (int)C, (int)Lt, (int)E);
  HIG_REQUIRE(Lt % 4 == 0 && E % 4 == 0, "%s: Lt and E must be multiples of 4 (Lt %d, E %d)", who, (int)Lt, (int)E);
  D.C = C; D.Lt = Lt; D.E = E;
  return HIG_OK;
}

// floats; forward: P (C, E).  backward: dP (C, E), dO (C, Lt), the column-sum partials of g_b
struct CFwd { int64_t P, total; };
CFwd cfwd_layout(const CDims& D) {
  CFwd w;
  w.P = 0;
  w.total = al((int64_t)D.C * D.E);
  return w;
}
struct CBwd { int64_t dP, dO, colpart, total; };
CBwd cbwd_layout(const CDims& D) {
  CBwd w;
  int64_t o = 0;
  auto take = [&](int64_t n) { int64_t r = o; o += al(n); return r; };
  w.dP = take((int64_t)D.C * D.E);
  w.dO = take((int64_t)D.C * D.Lt);
  w.colpart = take((int64_t)hig_colsum_chunks(D.C) * D.E);
  w.total = o;
  return w;
}

}  // namespace

extern "C" int64_t hig_class_head_workspace_bytes(int32_t C, int32_t Lt, int32_t E, int32_t backward) {
  CDims D;
  if (check_cdims(C, Lt, E, "hig_class_head_workspace_bytes", D) != HIG_OK) return -1;
  return (backward ? cbwd_layout(D).total : cfwd_layout(D).total) * 4;
}

extern "C" int hig_class_head_fwd(int32_t C, int32_t Lt, int32_t E, int32_t rows, const float* emb, const float* W, const float* b,
                                  const int32_t* ids, float* xf_out, float* xf_proj, void* workspace, hig_stream_t stream) {
  CDims D;
  HIG_TRY(check_cdims(C, Lt, E, "hig_class_head_fwd", D));
  HIG_REQUIRE(rows > 0, "hig_class_head_fwd: rows must be positive (got %d)", (int)rows);
  HIG_REQUIRE(emb && W && b && ids && xf_out && xf_proj && workspace, "hig_class_head_fwd: null argument");
  float* P = static_cast<float*>(workspace) + cfwd_layout(D).P;
  HIG_TRY(hig_gemm_launch(G(emb, Lt, 0, W, Lt, 0, P, E, C, E, Lt).epi(HIG_EPI_BIAS, b).g, 1, nullptr, hig_stream(stream)));
  HIG_TRY(hig_rows_gather_f32(emb, C, ids, rows, Lt, xf_out, stream));
  return hig_rows_gather_f32(P, C, ids, rows, E, xf_proj, stream);
}

extern "C" int hig_class_head_bwd(int32_t C, int32_t Lt, int32_t E, int32_t rows, const float* emb, const float* W, const int32_t* ids,
                                  const float* dxf_out, const float* dxf_proj, float* g_emb, float* g_W, float* g_b, void* workspace,
                                  hig_stream_t stream) {
  CDims D;
  HIG_TRY(check_cdims(C, Lt, E, "hig_class_head_bwd", D));
  HIG_REQUIRE(rows > 0, "hig_class_head_bwd: rows must be positive (got %d)", (int)rows);
  HIG_REQUIRE(emb && W && ids && g_emb && g_W && g_b && workspace, "hig_class_head_bwd: null argument");
  const CBwd w = cbwd_layout(D);
  float* ws = static_cast<float*>(workspace);
  float* dP = ws + w.dP;
  float* dO = ws + w.dO;
  hipStream_t st = hig_stream(stream);
  if (dxf_proj) {
    HIG_TRY(hig_rows_sum_by_key_f32(dxf_proj, ids, rows, E, C, dP, stream));
  } else {
    HIG_TRY(hig_zero_async(dP, (int64_t)C * E * 4, st));
  }
  if (dxf_out) {
    HIG_TRY(hig_rows_sum_by_key_f32(dxf_out, ids, rows, Lt, C, dO, stream));
  } else {
    HIG_TRY(hig_zero_async(dO, (int64_t)C * Lt * 4, st));
  }
  HIG_TRY(hig_colsum(dP, E, C, E, g_b, ws + w.colpart, stream));
  // g_W[e][l] = sum_c dP[c][e] emb[c][l]: the weight-gradient form of the text head's text_proj (both operands reduce-slow)
  HIG_TRY(hig_gemm_launch(G(dP, E, 1, emb, Lt, 1, g_W, Lt, E, Lt, C).g, 1, nullptr, st));
  // g_emb = dO + dP W: the data-gradient form with the upstream sum as the residual
  return hig_gemm_launch(G(dP, E, 0, W, Lt, 1, g_emb, Lt, C, Lt, E).epi(HIG_EPI_RES).res(dO, Lt).g, 1, nullptr, st);
}
