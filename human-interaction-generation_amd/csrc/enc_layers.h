// Host-side pieces of the three fp32 encoder chains (texthead.hip, evalnet.hip, cliptext.hip), each stated once: the typed view
// of a parameter table, the two dims checks, the post-norm layer's activation block, its forward and its backward, the debug tap
// of the backward, and the backward scratch with the GEMM forms that work in it.  Included by those three files only.
#pragma once
#include <array>
#include <initializer_list>
#include <type_traits>

#include "hig_host.h"

namespace {

// A parameter (V = const void) or gradient (V = void) table read as fp32: t[i] is a global slot, t(l, i) slot i of layer l.
template <class V> struct Tab {
  using F = std::conditional_t<std::is_const_v<V>, const float, float>;
  V* const* t; int nglobal, nlayer;
  Tab(V* const* t_, int nglobal_, int nlayer_) : t(t_), nglobal(nglobal_), nlayer(nlayer_) {}
  F* operator[](int i) const { return static_cast<F*>(t[i]); }
  F* operator()(int l, int i) const { return static_cast<F*>(t[nglobal + l * nlayer + i]); }
  V* const* layer(int l) const { return t + nglobal + l * nlayer; }
};

inline int hig_enc_check_prec(int prec) {
  if (prec != HIG_PREC_F32 && prec != HIG_PREC_BF16X3 && prec != HIG_PREC_BF16) return hig_set_error(HIG_EINVAL, "hig: unknown prec=%d", prec);
  return HIG_OK;
}
inline int hig_enc_check_hd(const char* who, int hd) {   // the head dims hig_fullattn_fwd / _bwd are built for
  if (!(hd == 8 || hd == 16 || hd == 32 || hd == 64 || hd == 128))
    return hig_set_error(HIG_EUNSUPPORTED, "%s: head dim %d not in {8,16,32,64,128}", who, hd);
  return HIG_OK;
}
// what a layout hook hands out: the first n_out of the table's n slots; returns n
inline int hig_enc_publish(const int64_t* v, int n, int64_t* out, int32_t n_out) {
  for (int s = 0; out && s < n && s < n_out; ++s) out[s] = v[s];
  return n;
}

// The extents every piece below is sized by: samples, tokens per sample, model width, FFN width, heads, head dim.
struct EncShape {
  int B, S, n, ff, H, hd;
  int64_t M() const { return (int64_t)B * S; }
};

// ---- one post-norm nn.TransformerEncoderLayer (gelu, dropout 0), shared by the text head and the evaluator ----
//     x1 = norm1(xin + out_proj(att(in_proj(xin))));   x2 = norm2(x1 + linear2(gelu(linear1(x1))))
// The buffers of one layer: F = float for the forward that writes them, const float for the backward that reads them.  In the
// training workspaces they are one block, in the order of HIG_TFW_QKV .. _X2 and HIG_EFW_QKV .. _X2 (include/hig.h).
template <class F> struct EncLayerOf {
  F *qkv, *lse, *att, *r1, *st1, *x1, *z, *f, *r2, *st2, *x2;
};
using EncLayer = EncLayerOf<float>;
using EncLayerAct = EncLayerOf<const float>;
enum { ENC_QKV = 0, ENC_LSE, ENC_ATT, ENC_R1, ENC_ST1, ENC_X1, ENC_Z, ENC_F, ENC_R2, ENC_ST2, ENC_X2, ENC_NBLOCK };
static_assert(HIG_TFW_X2 - HIG_TFW_QKV == ENC_X2 && HIG_EFW_X2 - HIG_EFW_QKV == ENC_X2 && HIG_TFW_Z - HIG_TFW_QKV == ENC_Z &&
                  HIG_EFW_Z - HIG_EFW_QKV == ENC_Z,
              "both published tables hold the block in this order");
// lays the block out through the caller's `take`: o[ENC_*] = the member's offset
template <class Take> void hig_enc_block_layout(Take&& take, int64_t* o, const EncShape& s) {
  const int64_t M = s.M();
  o[ENC_QKV] = take(M * 3 * s.n);
  o[ENC_LSE] = take((int64_t)s.B * s.H * s.S);
  o[ENC_ATT] = take(M * s.n);
  o[ENC_R1] = take(M * s.n);
  o[ENC_ST1] = take(M * 2);
  o[ENC_X1] = take(M * s.n);
  o[ENC_Z] = take(M * s.ff);
  o[ENC_F] = take(M * s.ff);
  o[ENC_R2] = take(M * s.n);
  o[ENC_ST2] = take(M * 2);
  o[ENC_X2] = take(M * s.n);
}
// the block at `base`; keep_z = false: a forward that does not keep the GELU pre-activation
template <class F> EncLayerOf<F> hig_enc_block_at(F* base, const int64_t* o, bool keep_z = true) {
  return {base + o[ENC_QKV], base + o[ENC_LSE], base + o[ENC_ATT], base + o[ENC_R1], base + o[ENC_ST1], base + o[ENC_X1],
          keep_z ? base + o[ENC_Z] : nullptr, base + o[ENC_F], base + o[ENC_R2], base + o[ENC_ST2], base + o[ENC_X2]};
}

// P: the layer's HIG_TL_* block of the parameter table.  kpad: key-padding bytes (B, S), or NULL (the text head).  a.z == NULL:
// the FF1 GEMM has no second output.
inline int hig_enc_layer_fwd(const EncShape& s, const void* const* P, const EncLayer& a, const float* xin, const uint8_t* kpad, int prec,
                             hig_stream_t stream) {
  auto p = [&](int i) { return static_cast<const float*>(P[i]); };
  hipStream_t st = hig_stream(stream);
  const int n = s.n, ff = s.ff;
  const int64_t M = s.M();
  HIG_TRY(hig_gemm_launch(G(xin, n, 0, p(HIG_TL_IN_W), n, 0, a.qkv, 3 * n, M, 3 * n, n).epi(HIG_EPI_BIAS, p(HIG_TL_IN_B)).prec(prec).g, 1,
                          nullptr, st));
  HIG_TRY(hig_fullattn_fwd_kpad(a.qkv, 3 * n, a.qkv + n, a.qkv + 2 * n, 3 * n, s.B, s.S, s.S, s.H, s.hd, nullptr, kpad, a.att, n, a.lse,
                                stream));
  HIG_TRY(hig_gemm_launch(G(a.att, n, 0, p(HIG_TL_OUT_W), n, 0, a.r1, n, M, n, n).epi(HIG_EPI_BIAS_RES, p(HIG_TL_OUT_B)).res(xin, n)
                              .prec(prec).g, 1, nullptr, st));
  HIG_TRY(hig_layernorm(a.r1, n, M, n, p(HIG_TL_N1_W), p(HIG_TL_N1_B), a.x1, n, a.st1, stream));
  G g1(a.x1, n, 0, p(HIG_TL_FF1_W), n, 0, a.f, ff, M, ff, n);
  g1.epi(HIG_EPI_BIAS_GELU, p(HIG_TL_FF1_B)).prec(prec);
  if (a.z) g1.aux(a.z, ff);
  HIG_TRY(hig_gemm_launch(g1.g, 1, nullptr, st));
  HIG_TRY(hig_gemm_launch(G(a.f, ff, 0, p(HIG_TL_FF2_W), ff, 0, a.r2, n, M, n, ff).epi(HIG_EPI_BIAS_RES, p(HIG_TL_FF2_B)).res(a.x1, n)
                              .prec(prec).g, 1, nullptr, st));
  return hig_layernorm(a.r2, n, M, n, p(HIG_TL_N2_W), p(HIG_TL_N2_B), a.x2, n, a.st2, stream);
}

// ---- the debug tap of the two post-norm backwards (hig_enc_bwd_debug_tap, include/hig.h), in floats: off[slot] is an absolute
// offset for the slots written once and an offset from the layer's base for the per-layer ones; -1 where the chain has no such
// buffer ----
struct EncTap {
  int64_t off[HIG_ETAP_NSLOTS], floats[HIG_ETAP_NSLOTS];
};
// text: the text head (DXF_TOTAL, DGATH) or the evaluator (DH_L, DH_0)
inline EncTap hig_enc_tap_layout(bool text, const EncShape& s, int64_t L) {
  EncTap t;
  const int64_t row = s.M() * s.n;
  for (int i = 0; i < HIG_ETAP_NSLOTS; ++i) t.floats[i] = row;      // (most slots are one (M, n) matrix)
  t.floats[HIG_ETAP_DXF_TOTAL] = text ? row : -1;
  t.floats[HIG_ETAP_DGATH] = text ? (int64_t)s.B * s.n : -1;
  t.floats[HIG_ETAP_DH_L] = t.floats[HIG_ETAP_DH_0] = text ? -1 : row;
  t.floats[HIG_ETAP_DZ] = s.M() * s.ff;
  t.floats[HIG_ETAP_DQKV] = 3 * row;
  t.floats[HIG_ETAP_DELTA] = (int64_t)s.B * s.H * s.S;
  int64_t o = 0;
  auto take = [&](int i) { t.off[i] = t.floats[i] < 0 ? -1 : o; if (t.floats[i] > 0) o += al(t.floats[i]); };
  for (int i = 0; i < HIG_ETAP_LAYER0; ++i) take(i);
  t.off[HIG_ETAP_LAYER0] = o;
  o = 0;
  for (int i = HIG_ETAP_LSTRIDE + 1; i < HIG_ETAP_TOTAL; ++i) take(i);
  t.off[HIG_ETAP_LSTRIDE] = o;
  t.off[HIG_ETAP_TOTAL] = t.off[HIG_ETAP_LAYER0] + o * L;
  return t;
}

// ---- the scratch a backward sequence owns, and the three GEMM forms every such sequence is made of ----
// Where a chain's layout table holds each member (tA / tB -1: the chain runs exact-fp32 products only and has none).
struct EncScratchSlots {
  int dff, dqkv, delta, wT, tA, tB, slabs, slab_floats, colpart, lnpart;
};
// The layout, through the caller's `take`, in two runs (the text head keeps a member of its own between them): the gradients a
// layer's backward passes on ...
template <class Take> void hig_enc_scratch_grads(Take&& take, int64_t* v, const EncScratchSlots& m, const EncShape& s) {
  v[m.dff] = take(s.M() * s.ff);
  v[m.dqkv] = take(s.M() * 3 * s.n);
  v[m.delta] = take((int64_t)s.B * s.H * s.S);
}
// ... and what its GEMMs and row kernels work in.  big: the largest weight the chain transposes or splits; colsum_uses: the
// (rows, cols) of every hig_colsum that works in colpart; tA / tB: floats of the two transposed operands of the bf16 product
// modes (al(0) == 0: nothing where unused).
template <class Take>
void hig_enc_scratch_work(Take&& take, int64_t* v, const EncScratchSlots& m, const EncShape& s, int64_t big,
                          std::initializer_list<std::array<int64_t, 2>> colsum_uses, int64_t tA = 0, int64_t tB = 0) {
  v[m.wT] = take(big);
  const int64_t oA = take(tA), oB = take(tB);
  if (m.tA >= 0) v[m.tA] = oA;
  if (m.tB >= 0) v[m.tB] = oB;
  // split-R slabs of the weight-gradient GEMMs: sixteen of the largest weight, never less than 1536 tiles of 128 x 128
  v[m.slab_floats] = big * 16 > (int64_t)1536 * 128 * 128 ? big * 16 : (int64_t)1536 * 128 * 128;
  v[m.slabs] = take(v[m.slab_floats]);
  int64_t colp = 0;
  for (const auto& u : colsum_uses) {
    const int64_t c = (int64_t)hig_colsum_chunks(u[0]) * u[1];
    colp = c > colp ? c : colp;
  }
  v[m.colpart] = take(colp);
  v[m.lnpart] = take(hig_ln_bwd_partial_floats(s.M(), s.n, s.S));
}

struct EncBwd : EncShape {
  int prec;                           // HIG_PREC_*
  float *slabs; int64_t slab_floats;  // split-R slabs of the weight-gradient GEMMs
  float *colp, *lnp, *wT, *tA, *tB;   // column-sum partials, LayerNorm partials, W^T, the two transposed operands (bf16 product modes)
  float *dff, *dqkv, *delta;          // (M, ff), (M, 3n), (B, H, S)
  hig_stream_t stream;
  float* tap = nullptr;               // the debug tap (tap_begin): NULL in every real run
  EncTap tl;
  hipStream_t st() const { return hig_stream(stream); }

  // the scratch at `base`, laid out by hig_enc_scratch_grads / _work into v
  EncBwd(const EncShape& s, int prec_, float* base, const int64_t* v, const EncScratchSlots& m, hig_stream_t stream_)
      : EncShape(s), prec(prec_), slabs(base + v[m.slabs]), slab_floats(v[m.slab_floats]), colp(base + v[m.colpart]),
        lnp(base + v[m.lnpart]), wT(base + v[m.wT]), tA(m.tA < 0 ? nullptr : base + v[m.tA]), tB(m.tB < 0 ? nullptr : base + v[m.tB]),
        dff(base + v[m.dff]), dqkv(base + v[m.dqkv]), delta(base + v[m.delta]), stream(stream_) {}

  // Before the first launch of a backward: takes the process's tap buffer, if one is set; a buffer too short for these dims is
  // refused before any HIP call, a capturing stream before any launch.
  int tap_begin(bool text, int L, const char* who) {
    float* buf = nullptr;
    int64_t bytes = 0;
    hig_enc_tap_buffer(&buf, &bytes);
    tap = nullptr;
    if (!buf) return HIG_OK;
    tl = hig_enc_tap_layout(text, *this, L);
    if (bytes < tl.off[HIG_ETAP_TOTAL] * 4)
      return hig_set_error(HIG_EINVAL, "%s: the tap buffer has %lld bytes, these dims need %lld", who, (long long)bytes,
                           (long long)(tl.off[HIG_ETAP_TOTAL] * 4));
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st(), &cap) != hipSuccess || cap != hipStreamCaptureStatusNone)
      return hig_set_error(HIG_EINVAL, "%s: a debug tap is set and the stream is capturing", who);
    tap = buf;
    return HIG_OK;
  }
  // copies `src` into the tap's slot (of layer l, or l < 0: a slot written once) behind the launch that wrote it
  int tap_copy(int slot, int l, const float* src) const {
    if (!tap) return HIG_OK;
    float* dst = tap + tl.off[slot] + (l < 0 ? 0 : tl.off[HIG_ETAP_LAYER0] + tl.off[HIG_ETAP_LSTRIDE] * l);
    return hig_copy_async(dst, src, tl.floats[slot] * 4, st());
  }

  int wgrad(G gd) const {
    const int s = wgrad_splits(gd.g.I, gd.g.J, gd.g.R, slab_floats, gd.g.prec);
    return hig_gemm_launch(gd.g, s, slabs, st());
  }
  // dW[n][k] = sum_m dC[m][n] * act[m][k]; bf16 product modes transpose both operands first
  // dbias = column sums of dC (the bias gradient): from the wgrad GEMM itself in the exact-fp32 path
  int wgrad_act(const float* dC, int n_out, const float* act, int k_in, float* out, int64_t rows, float* dbias) const {
    if (prec != HIG_PREC_F32 && rows % 32 == 0) {
      HIG_TRY(hig_colsum(dC, n_out, rows, n_out, dbias, colp, stream));
      HIG_TRY(hig_transpose(dC, n_out, (int)rows, n_out, tA, rows, nullptr, nullptr, nullptr, stream));
      HIG_TRY(hig_transpose(act, k_in, (int)rows, k_in, tB, rows, nullptr, nullptr, nullptr, stream));
      return wgrad(G(tA, rows, 0, tB, rows, 0, out, k_in, n_out, k_in, rows).prec(prec));
    }
    G gd(dC, n_out, 1, act, k_in, 1, out, k_in, n_out, k_in, rows);
    if (n_out % 4 == 0) gd.xsum(dbias);
    else HIG_TRY(hig_colsum(dC, n_out, rows, n_out, dbias, colp, stream));
    return wgrad(gd);
  }
  // dX = dC . W with W (out_f, in_f) transposed first, so both operands are reduce-contiguous
  int dgrad(const float* dC, const float* W, int out_f, int in_f, int64_t rows, float* dX, int epi, const float* res,
            float* aux) const {
    HIG_TRY(hig_transpose(W, in_f, out_f, in_f, wT, out_f, nullptr, nullptr, nullptr, stream));
    G gd(dC, out_f, 0, wT, out_f, 0, dX, in_f, rows, in_f, out_f);
    gd.prec(prec);
    if (epi == HIG_EPI_RES) gd.epi(HIG_EPI_RES).res(res, in_f);
    if (epi == HIG_EPI_DGELU) gd.epi(HIG_EPI_DGELU).aux(aux, in_f);
    return hig_gemm_launch(gd.g, 1, nullptr, st());
  }
  int colsum(const float* src, int64_t ld, int64_t rows, int n_, float* dst) const {
    return hig_colsum(src, ld, rows, n_, dst, colp, stream);
  }
};

// The backward of the post-norm layer.  P / Gr: the layer's HIG_TL_* block of the parameter / gradient table.  a: what the
// training forward kept of the layer.  d: in d(x2), out d(xin); t1, t2: (M, n) scratch.  kpad: the forward's key-padding bytes
// (B, S), or NULL.  l: the layer's index (names the tap's per-layer block).
inline int hig_enc_layer_bwd(const EncBwd& e, int l, const void* const* P, void* const* Gr, const EncLayerAct& a, const float* xin,
                             const uint8_t* kpad, float* d, float* t1, float* t2) {
  auto p = [&](int i) { return static_cast<const float*>(P[i]); };
  auto g = [&](int i) { return static_cast<float*>(Gr[i]); };
  const int n = e.n, ff = e.ff;
  const int64_t M = e.M();
  HIG_TRY(e.tap_copy(HIG_ETAP_DH_IN, l, d));
  // norm2: x2 = LN(r2)
  HIG_TRY(hig_ln_bwd(d, n, a.r2, n, a.st2, p(HIG_TL_N2_W), p(HIG_TL_N2_B), nullptr, 0, 0, 0, nullptr, 0, t1, n, M, n, e.S,
                     g(HIG_TL_N2_W), g(HIG_TL_N2_B), nullptr, 0, e.lnp, e.stream));
  const float* dr2 = t1;
  HIG_TRY(e.tap_copy(HIG_ETAP_DR2, l, dr2));
  // r2 = x1 + linear2(gelu(z)),  z = linear1(x1)
  HIG_TRY(e.wgrad_act(dr2, n, a.f, ff, g(HIG_TL_FF2_W), M, g(HIG_TL_FF2_B)));
  HIG_TRY(e.dgrad(dr2, p(HIG_TL_FF2_W), n, ff, M, e.dff, HIG_EPI_DGELU, nullptr, const_cast<float*>(a.z)));
  const float* dz = e.dff;
  HIG_TRY(e.tap_copy(HIG_ETAP_DZ, l, dz));
  HIG_TRY(e.wgrad_act(dz, ff, a.x1, n, g(HIG_TL_FF1_W), M, g(HIG_TL_FF1_B)));
  HIG_TRY(e.dgrad(dz, p(HIG_TL_FF1_W), ff, n, M, t2, HIG_EPI_RES, dr2, nullptr));  // t2 = d(x1)
  HIG_TRY(e.tap_copy(HIG_ETAP_DX1, l, t2));
  // norm1: x1 = LN(r1)
  HIG_TRY(hig_ln_bwd(t2, n, a.r1, n, a.st1, p(HIG_TL_N1_W), p(HIG_TL_N1_B), nullptr, 0, 0, 0, nullptr, 0, t1, n, M, n, e.S,
                     g(HIG_TL_N1_W), g(HIG_TL_N1_B), nullptr, 0, e.lnp, e.stream));
  const float* dr1 = t1;
  HIG_TRY(e.tap_copy(HIG_ETAP_DR1, l, dr1));
  // r1 = xin + out_proj(att)
  HIG_TRY(e.wgrad_act(dr1, n, a.att, n, g(HIG_TL_OUT_W), M, g(HIG_TL_OUT_B)));
  HIG_TRY(e.dgrad(dr1, p(HIG_TL_OUT_W), n, n, M, t2, HIG_EPI_NONE, nullptr, nullptr));  // t2 = d(att)
  HIG_TRY(e.tap_copy(HIG_ETAP_DATT, l, t2));
  float* dqkv = e.dqkv;
  HIG_TRY(hig_fullattn_bwd_kpad(t2, n, a.att, n, a.qkv, 3 * n, a.qkv + n, a.qkv + 2 * n, 3 * n, e.B, e.S, e.S, e.H, e.hd, nullptr,
                                a.lse, e.delta, dqkv, 3 * n, dqkv + n, dqkv + 2 * n, 3 * n, kpad, e.stream));
  HIG_TRY(e.tap_copy(HIG_ETAP_DQKV, l, dqkv));
  HIG_TRY(e.tap_copy(HIG_ETAP_DELTA, l, e.delta));
  HIG_TRY(e.wgrad_act(dqkv, 3 * n, xin, n, g(HIG_TL_IN_W), M, g(HIG_TL_IN_B)));
  return e.dgrad(dqkv, p(HIG_TL_IN_W), 3 * n, n, M, d, HIG_EPI_RES, dr1, nullptr);   // d = d(xin)
}

}  // namespace
