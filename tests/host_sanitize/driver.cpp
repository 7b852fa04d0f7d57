// Host-side entry points of libhig under AddressSanitizer + UndefinedBehaviorSanitizer (sanitizers on
// the CPU build only; GPU ASan is not available on this pool).  Everything called here returns BEFORE any HIP call:
// size / layout queries (hig_*_bytes, *_scratch_*), and argument validation that must reject bad descriptors with an
// error code -- never read through a null pointer, never overflow an index computation.  Built by `make sanitize`
// (csrc/Makefile: every .hip compiled --cuda-host-only with -fsanitize=address,undefined) and run by
// tests/test_cpu_host.py::test_host_entry_points_under_asan_ubsan.
#include <initializer_list>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hig.h"

// The objects are compiled --cuda-host-only: there is no device image to register.  These definitions (in the executable,
// so they win over libamdhip64's) turn the module constructors of the translation units into no-ops.
extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
void __hipRegisterManagedVar(void**, void**, void*, const char*, size_t, unsigned) {}
void __hipUnregisterFatBinary(void**) {}
}

static int failures = 0;
#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "driver.cpp:%d: expectation failed: %s\n", __LINE__, #cond); \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static hig_dims dims(int B, int T, int F, int d, int H, int ff, int L, int two, int storage, int attn, int prec) {
  hig_dims D;
  memset(&D, 0, sizeof(D));
  D.B = B; D.T = T; D.F = F; D.d = d; D.H = H; D.ff = ff; D.L = L; D.N = 77; D.Lt = 256; D.num_frames = T > 196 ? T : 196;
  D.attn_kind = attn; D.prec = prec; D.two_person = two; D.storage = storage;
  return D;
}

int main() {
  char msg[512];
  EXPECT(hig_version() > 0);
  // ---- workspace layouts over a sweep of legal shapes (every index computation of the layout builders) ----
  const int shapes[][7] = {{2, 16, 12, 64, 8, 128, 2},    {2, 60, 150, 128, 8, 256, 4},  {64, 196, 150, 512, 8, 1024, 8},
                           {32, 300, 150, 1024, 8, 1024, 12}, {64, 91, 263, 512, 8, 1024, 8}, {1, 1, 4, 32, 4, 32, 1},
                           {1024, 196, 263, 512, 8, 2048, 8}};
  for (const auto& s : shapes)
    for (int two = 0; two <= 2; ++two)
      for (int storage = 0; storage <= 1; ++storage)
        for (int attn = 0; attn <= 1; ++attn) {
          if (two && (s[0] & 1)) continue;
          hig_dims D = dims(s[0], s[1], s[2], s[3], s[4], s[5], s[6], two, storage, attn, 0);
          const int hd = D.d / D.H;
          const bool bf16_ok = (hd == 64 || hd == 128) && !(two && attn);
          for (int training = 0; training <= 1; ++training) {
            const int64_t w = hig_workspace_bytes(&D, training), t = hig_textctx_bytes(&D, training);
            // bf16 storage: inference for head dim 64 / 128; training with linear attention (single-person and two-person)
            const bool bf16_train_ok = bf16_ok && !attn;
            if (storage == 1 && (!bf16_ok || (training && !bf16_train_ok))) { EXPECT(w < 0 && t < 0); continue; }
            if (two && attn) { EXPECT(w < 0); continue; }
            EXPECT(w > 0 && t > 0);
          }
          if (storage == 0 && !(two && attn)) EXPECT(hig_bwd_workspace_bytes(&D) > 0);
          if (storage == 1) EXPECT((hig_bwd_workspace_bytes(&D) > 0) == (bf16_ok && !attn));
        }
  // ---- illegal dims: rejected with a message, nothing dereferenced ----
  {
    hig_dims D = dims(2, 16, 12, 64, 8, 128, 2, 0, 0, 0, 0);
    hig_dims bad = D; bad.H = 7;              EXPECT(hig_workspace_bytes(&bad, 0) < 0);
    bad = D; bad.T = 500;                     EXPECT(hig_workspace_bytes(&bad, 0) < 0);      // T > num_frames
    bad = D; bad.B = 0;                       EXPECT(hig_workspace_bytes(&bad, 0) < 0);
    bad = D; bad.L = -1;                      EXPECT(hig_workspace_bytes(&bad, 1) < 0);
    bad = D; bad.prec = 99;                   EXPECT(hig_workspace_bytes(&bad, 0) < 0);
    bad = D; bad.two_person = 1; bad.B = 3;   EXPECT(hig_workspace_bytes(&bad, 0) < 0);
    EXPECT(hig_workspace_bytes(nullptr, 0) < 0);
    EXPECT(hig_last_error(msg, sizeof(msg)) >= 0 && strlen(msg) > 0);
    EXPECT(hig_last_error(msg, 4) >= 0 && strlen(msg) <= 3);                               // truncation, no overrun
    // entry points with null arguments / mismatched storage
    EXPECT(hig_denoiser_fwd(&D, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) != HIG_OK);
    EXPECT(hig_denoiser_fwd_bf16(&D, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != HIG_OK);
    EXPECT(hig_cast_pad_bf16(nullptr, 150, 8, 150, nullptr, 160, nullptr) != HIG_OK);
    EXPECT(hig_denoiser_fwd_bf16_x(&D, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != HIG_OK);
    EXPECT(hig_text_context(&D, nullptr, nullptr, nullptr, 0, nullptr) != HIG_OK);
    // round 4: the bf16-storage training entry points (fp32-storage dims, null arguments, shapes they do not train)
    EXPECT(hig_denoiser_fwd_bf16_train(&D, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != HIG_OK);
    EXPECT(hig_denoiser_bwd_bf16(&D, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != HIG_OK);
    {
      hig_dims T16 = dims(2, 60, 150, 512, 8, 1024, 2, 0, 1, 0, 0);
      EXPECT(hig_text_context_bf16_train(&T16, nullptr, nullptr, nullptr, nullptr, nullptr) != HIG_OK);
      EXPECT(hig_denoiser_fwd_bf16_train(&T16, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != HIG_OK);
      T16.attn_kind = HIG_ATTN_FULL;
      EXPECT(hig_workspace_bytes(&T16, 1) < 0 && hig_workspace_bytes(&T16, 0) > 0);
    }
    EXPECT(hig_ln_bwd_bf16(nullptr, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, 0, nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr) != HIG_OK);
    EXPECT(hig_colsum_bf16(nullptr, 0, 0, 0, nullptr, nullptr, nullptr) != HIG_OK);
    EXPECT(hig_transpose_bf16_batch(13, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != HIG_OK);
    EXPECT(hig_gemm_bf16_split(nullptr, 0, nullptr, 0, nullptr) != HIG_OK);
    EXPECT(hig_clip_adam_shadow(nullptr, nullptr, nullptr, nullptr, 0, 0.f, nullptr, 0.f, 0.f, 0.f, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr, 0, nullptr) != HIG_OK);
  }
  // ---- scratch-size queries ----
  EXPECT(hig_gemm_tail_ws_bytes() > 0);
  EXPECT(hig_joint_embed_bf16_scratch_bytes(150, 512) == 512 * 160 * 2);
  EXPECT(hig_joint_embed_bf16_scratch_bytes(0, 512) < 0 && hig_joint_embed_bf16_scratch_bytes(150, -1) < 0);
  for (int hd : {8, 16, 32, 64, 128})
    for (int B : {1, 32, 64, 1024}) {
      EXPECT(hig_linattn_ctx_scratch_floats(B, 196, 8, hd) >= 0);
      EXPECT(hig_linattn_bwd_scratch_floats(B, 196, 8, hd) >= 0);
    }
  EXPECT(hig_ln_bwd_partial_floats(12544, 512, 196) > 0);
  EXPECT(hig_colsum_chunks(12544) > 0 && hig_colsum_chunks(1) > 0);
  // ---- GEMM descriptors: validation before any launch ----
  {
    hig_gemm_desc g;
    memset(&g, 0, sizeof(g));
    EXPECT(hig_gemm(nullptr, nullptr) != HIG_OK);
    EXPECT(hig_gemm(&g, nullptr) != HIG_OK);                           // null operands
    EXPECT(hig_gemm_split_scratch_floats(&g, 4) >= 0 || hig_gemm_split_scratch_floats(&g, 4) < 0);
    EXPECT(hig_gemm_ws(&g, nullptr, 0, nullptr) != HIG_OK);
    float dummy[64] = {0};
    g.X = dummy; g.Y = dummy; g.C = dummy; g.I = -5; g.J = 4; g.R = 4; g.ldx = 4; g.ldy = 4; g.ldc = 4;
    EXPECT(hig_gemm(&g, nullptr) != HIG_OK);                           // negative extent
    hig_gemm16_desc h;
    memset(&h, 0, sizeof(h));
    EXPECT(hig_gemm_bf16(nullptr, nullptr) != HIG_OK);
    EXPECT(hig_gemm_bf16(&h, nullptr) != HIG_OK);
    alignas(16) static unsigned short b16[64 * 48];
    h.X = b16; h.Y = b16; h.C = b16; h.I = 64; h.J = 64; h.R = 48; h.ldx = 48; h.ldy = 48; h.ldc = 64;
    EXPECT(hig_gemm_bf16(&h, nullptr) == HIG_EUNSUPPORTED);            // R % 32 != 0
    // round-3 entry points: argument validation before any launch
    alignas(16) static float f32v[512];
    EXPECT(hig_attn_out16(nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, 1, 1, 8, 64, nullptr) != HIG_OK);
    EXPECT(hig_attn_out16(b16, 1536, b16, f32v, f32v, f32v, 1024, 512, b16, f32v, b16, 512, nullptr, 1, 4, 4, 64, nullptr) == HIG_EUNSUPPORTED);   // 4 heads
    EXPECT(hig_attn_out16(b16, 1535, b16, f32v, f32v, f32v, 1024, 512, b16, f32v, b16, 512, nullptr, 1, 4, 8, 64, nullptr) != HIG_OK);            // ldq % 8
    EXPECT(hig_rows_out16(nullptr, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, 1, 1, 512, nullptr) != HIG_OK);
    EXPECT(hig_rows_out16(b16, 512, f32v, f32v, f32v, 1024, 512, b16, f32v, b16, 512, nullptr, 1, 4, 256, nullptr) == HIG_EUNSUPPORTED);          // d != 512
    EXPECT(hig_weight_frag16(b16, 40, 33, 40, b16, nullptr) != HIG_OK);                                                                           // J % 32 != 0
    EXPECT(hig_weight_frag16(nullptr, 0, 0, 0, nullptr, nullptr) != HIG_OK);
    EXPECT(hig_joint_embed_bf16_w(nullptr, 0, 0, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, 0, 0, nullptr) != HIG_OK);
    EXPECT(hig_joint_embed_bf16_w(f32v, 4, 600, b16, f32v, f32v, 512, 4, 0, b16, 512, 512, nullptr) == HIG_EUNSUPPORTED);                         // F > 512
    EXPECT(hig_linattn_ctx_mm16(b16, b16, 1536, 1, 4, 8, 32, nullptr, f32v, f32v, nullptr, nullptr) == HIG_EUNSUPPORTED);                         // head dim 32
    EXPECT(hig_linattn_apply_sty_mm16(b16, 1536, b16, f32v, f32v, f32v, 1024, 512, b16, 512, 1, 4, 3, 64, nullptr) == HIG_EUNSUPPORTED);         // 3 heads
    EXPECT(hig_timestep_embedding_bf16(nullptr, 1, 64, nullptr, nullptr) != HIG_OK);
    // hig_recover_joints: a null pointer and T > 8192 are refused before any HIP call.  (Its third refusal, 16 T bytes above the
    // device's per-workgroup LDS limit, asks the device first, so it is not exercised here: tests/test_gpu_boundary_contract.py.)
    EXPECT(hig_recover_joints(nullptr, nullptr, 1, 2, 4, 1, 0, nullptr, nullptr) == HIG_EINVAL);
    EXPECT(hig_recover_joints(f32v, nullptr, 1, 8193, 4, 1, 0, f32v, nullptr) == HIG_EINVAL);
    EXPECT(hig_recover_joints(f32v, nullptr, 1, 0, 4, 1, 0, f32v, nullptr) == HIG_EINVAL);
    EXPECT(hig_pair_mse(f32v, f32v, nullptr, 6, 2, 4, 1, f32v, nullptr, f32v, nullptr) == HIG_EINVAL);                  // PIT with R % 4 != 0
    EXPECT(hig_pair_mse(f32v, f32v, nullptr, 4, 2, 3, 1, f32v, nullptr, f32v, nullptr) == HIG_EINVAL);                  // F < 4
    EXPECT(hig_gather_frames(f32v, nullptr, nullptr, f32v, 0, 1, 1, 4, f32v, nullptr) == HIG_EINVAL);
    h.R = 32; h.ldx = 33;
    EXPECT(hig_gemm_bf16(&h, nullptr) == HIG_EINVAL);                  // leading dimension not a multiple of 8
    h.ldx = 48; h.epi = HIG_EPI_BIAS_RES; h.bias = reinterpret_cast<const float*>(dummy);
    EXPECT(hig_gemm_bf16(&h, nullptr) == HIG_EINVAL);                  // residual epilogue without a residual
    h.I = 0; h.epi = HIG_EPI_NONE;
    EXPECT(hig_gemm_bf16(&h, nullptr) == HIG_OK);                      // empty problem: nothing to launch
    EXPECT(hig_cast_bf16(nullptr, nullptr, 8, nullptr) != HIG_OK);
    EXPECT(hig_cast_bf16(dummy, b16, 0, nullptr) == HIG_OK);
    EXPECT(hig_joint_embed_bf16(nullptr, 4, 150, nullptr, nullptr, nullptr, 512, 196, 0, nullptr, 512, 512, nullptr, nullptr) != HIG_OK);
  }
  // ---- GEMM plan entries: pure host functions; null, misaligned, zero, negative and huge arguments, never a dereference ----
  {
    int32_t path = 0, launches = 0, variant = 0;
    EXPECT(hig_gemm_bf16_plan(nullptr, 256, &path, &launches, &variant) == HIG_EINVAL);
    EXPECT(hig_gemm_plan(nullptr, 1, 256, &path, &launches, &variant) == HIG_EINVAL);
    const uintptr_t base = (uintptr_t)1 << 32;                       // made-up addresses: nothing may read through them
    const int extents[] = {-5, 0, 1, 64, 65, 200, 512, 2047, 2048, 12544, INT32_MAX};
    const int64_t lds[] = {-8, 0, 8, 512, 516, 520, (int64_t)1 << 20, (int64_t)1 << 40, INT64_MAX};
    int served = 0, refused = 0;
    for (int I : extents) for (int J : extents) for (int R : {-32, 0, 32, 192, 256, 512, 1024, 1536, 2048, INT32_MAX}) for (int64_t ld : lds)
      for (int epi = -1; epi <= 9; ++epi) for (int mis : {0, 2, 8}) for (int cus : {128, 256}) {
        hig_gemm16_desc h;
        memset(&h, 0, sizeof(h));
        h.X = reinterpret_cast<const void*>(base); h.Y = reinterpret_cast<const void*>(2 * base); h.C = reinterpret_cast<void*>(3 * base + mis);
        h.ldx = ld; h.ldy = ld; h.ldc = ld; h.ldr = ld; h.ldaux = ld; h.I = I; h.J = J; h.R = R; h.epi = epi;
        h.c_f32 = mis == 2; h.res_f32 = mis == 8;
        if (epi & 1) h.bias = reinterpret_cast<const float*>(4 * base);
        if (epi & 2) h.res = reinterpret_cast<const void*>(5 * base + mis);
        if (epi == 2 && mis) h.aux = reinterpret_cast<void*>(6 * base);
        if (epi == 3 && mis == 2) h.row_stats_out = reinterpret_cast<float*>(7 * base);
        if (epi == 1 && mis == 2) { h.row_stats_in = reinterpret_cast<const float*>(7 * base); h.ln_colsum = mis ? reinterpret_cast<const float*>(8 * base) : nullptr; }
        int rc = hig_gemm_bf16_plan(&h, cus, &path, &launches, &variant);
        EXPECT((rc == HIG_OK && launches >= 0 && launches <= 1 && (launches == 0) == (path == -1)) || (rc < 0 && launches == 0 && path == -1));
        rc == HIG_OK ? ++served : ++refused;
        hig_gemm_desc g;
        memset(&g, 0, sizeof(g));
        g.X = reinterpret_cast<const float*>(base); g.Y = reinterpret_cast<const float*>(2 * base); g.C = reinterpret_cast<float*>(3 * base + mis);
        g.ldx = ld; g.ldy = ld; g.ldc = ld; g.ldr = ld; g.ldaux = ld; g.I = I; g.J = J; g.R = R; g.epi = epi;
        g.x_rs = mis == 8 && (epi & 1); g.y_rs = mis == 8;
        if (epi & 1) g.bias = reinterpret_cast<const float*>(4 * base);
        if (epi & 2) g.res = reinterpret_cast<const float*>(5 * base + mis);
        if (epi == 2 || epi == 6) g.aux = reinterpret_cast<float*>(6 * base);
        if (epi == 3 && mis == 2) g.row_stats_out = reinterpret_cast<float*>(7 * base);
        if (epi == 1 && mis == 2) { g.row_stats_in = reinterpret_cast<const float*>(7 * base); g.ln_colsum = reinterpret_cast<const float*>(8 * base); }
        rc = hig_gemm_plan(&g, mis == 0, cus, &path, &launches, nullptr);
        EXPECT((rc == HIG_OK && launches >= 0 && launches <= 2 && (launches == 0) == (path == -1)) || (rc < 0 && launches == 0 && path == -1));
      }
    EXPECT(served > 1000 && refused > 1000);
    EXPECT(hig_gemm_bf16_plan(nullptr, 0, nullptr, nullptr, nullptr) == HIG_EINVAL && hig_gemm_plan(nullptr, 0, 0, nullptr, nullptr, nullptr) == HIG_EINVAL);
    for (int64_t rows : {(int64_t)-1, (int64_t)0, (int64_t)2048, (int64_t)12544, (int64_t)1 << 40, INT64_MAX})
      for (int d : {-512, 0, 256, 500, 512, 1024, INT32_MAX})
        EXPECT((hig_gemm_bf16_lnfold_plan(rows, d, 256) | 1) == 1);
    EXPECT(hig_gemm_bf16_lnfold_plan(12544, 512, 256) == 1 && hig_gemm_bf16_lnfold_plan(12544, 512, 128) == 0);
  }
  // ---- attention plan entry: a pure host function; null out-pointers, zero, negative and INT32_MAX extents, every entry x I/O x
  // head dim x operand facts; then the entry points' own refusals (planned, so returned before any launch) ----
  {
    int32_t path = 0, split = 0, variant = 0;
    const int extents[] = {-5, 0, 1, 64, 65, 196, 4096, INT32_MAX};
    int served = 0, refused = 0;
    for (int entry = -1; entry <= HIG_ATTN_ENTRY_FULL_BWD + 1; ++entry) for (int io = -1; io <= 2; ++io)
      for (int hd : {-64, 0, 8, 16, 32, 48, 64, 128, 256, INT32_MAX}) for (int B : extents) for (int rows : extents) for (int H : {-1, 0, 3, 4, 8, INT32_MAX})
        for (int facts : {0, HIG_ATTN_FACT_OPERANDS, HIG_ATTN_FACTS_ALL & ~HIG_ATTN_FACT_IN16, HIG_ATTN_FACTS_ALL, -1}) for (int cus : {1, 256, INT32_MAX})
          for (int lds = 0; lds <= 1; ++lds) {
            const int rc = hig_attn_plan(entry, io, B, rows, rows, H, hd, lds, facts, cus, lds, &path, &split, &variant);
            EXPECT((rc == HIG_OK && path >= 0 && path < HIG_ATTN_NPATHS && split >= 1 && variant >= 0) || (rc < 0 && path == -1 && split == 0));
            if (entry < 0 || entry > HIG_ATTN_ENTRY_FULL_BWD || io < 0 || io > 1 || B <= 0 || rows <= 0) EXPECT(rc == HIG_EINVAL);
            if (facts == HIG_ATTN_FACTS_ALL) EXPECT(hig_attn_plan(entry, io, B, rows, rows, H, hd, lds, facts, cus, lds, nullptr, nullptr, nullptr) == rc);
            rc == HIG_OK ? ++served : ++refused;
          }
    EXPECT(served > 1000 && refused > 1000);
    alignas(16) static float q[64];
    EXPECT(hig_linattn_apply(nullptr, 64, q, q, 64, 1, 1, 1, 64, nullptr) == HIG_EINVAL);
    EXPECT(hig_linattn_apply(q, 64, q, q, 64, 1, 1, 1, 48, nullptr) == HIG_EINVAL);                                  // head dim
    EXPECT(hig_linattn_apply(q, 64, q, q + 1, 64, 1, 1, 1, 64, nullptr) == HIG_EINVAL);                              // Y off 16 bytes
    EXPECT(hig_linattn_apply_bf16(q, 64, q, q, 64, 1, 1, 1, 32, nullptr) == HIG_EUNSUPPORTED);
    EXPECT(hig_linattn_ctx_bf16(q, q, 66, 1, 1, 1, 64, nullptr, q, q, nullptr, nullptr, nullptr) == HIG_EINVAL);     // ld % 4
    EXPECT(hig_linattn_apply_bwd(q, 64, q, 64, q, q, 64, q, 1, 1, 1, 128, nullptr, nullptr) == HIG_EINVAL);          // no scratch
    EXPECT(hig_linattn_ctx_bwd_bf16(q, q, q, q, 64, q, nullptr, q, q, INT64_MAX, 1, 1, 1, 64, nullptr) == HIG_EINVAL);
    EXPECT(hig_linattn_apply_sty(q, 256, q, q, q, q, 512, 256, q, 256, 1, 1, 3, 64, nullptr) == HIG_EUNSUPPORTED);   // 3 heads
    EXPECT(hig_linattn_apply_sty(q, 256, q, q, q, q, 512, 256, q, INT64_MAX - 3, 1, INT32_MAX, 4, 64, nullptr) == HIG_EINVAL);   // output rows beyond 2 GiB
    EXPECT(hig_fullattn_fwd(q, 64, q, q, 64, 1, 1, 0, 1, 64, nullptr, q, 64, q, nullptr) == HIG_EINVAL);             // no keys
    EXPECT(hig_fullattn_fwd_bf16(q, 64, q, q, 64, 1, 1, 1, 1, 32, nullptr, q, 64, nullptr) == HIG_EUNSUPPORTED);
    EXPECT(hig_fullattn_bwd(q, 64, q, 64, q, 64, q, q, 64, 1, 1, 1, 1, 64, nullptr, q, q, q, 64, q, q + 2, 64, nullptr) == HIG_EINVAL);
  }
  // ---- denoiser plan entry: a pure host function behind the dims check; every entry code from -1 to one past the last, extents
  // 0, 1, the thresholds +- 1 and INT32_MAX, every switch at -1, 0, 1, 2 and 1000, `out` NULL and n_out too small ----
  {
    const int NS = HIG_DN_PLAN_NSLOTS, CANARY = 0x5a5a5a5a;
    int32_t out[HIG_DN_PLAN_NSLOTS + 1];
    long served = 0, refused = 0;
    const int32_t dflt[HIG_DN_NSWITCHES] = {1, 1, -1, 1, -1, 1, 1, 2, 1, 1, -1};
    auto ask = [&](const hig_dims& D, int entry, int flags, int facts, int cus, const int32_t* sw, int n_out) {
      for (int i = 0; i <= NS; ++i) out[i] = CANARY;
      const int rc = hig_denoiser_plan(&D, entry, flags & 1, (flags >> 1) & 1, facts, (flags >> 2) & 1, cus, (flags >> 3) & 1, sw, out, n_out);
      const int wrote = rc == HIG_OK ? (n_out < 0 ? 0 : n_out > NS ? NS : n_out) : 0;
      for (int i = wrote; i <= NS; ++i) EXPECT(out[i] == CANARY);
      if (rc != HIG_OK) { EXPECT(rc < 0); ++refused; return rc; }
      ++served;
      EXPECT(hig_denoiser_plan(&D, entry, flags & 1, (flags >> 1) & 1, facts, (flags >> 2) & 1, cus, (flags >> 3) & 1, sw, nullptr, n_out) == HIG_OK);
      if (wrote == NS) {
        EXPECT(out[HIG_DN_PLAN_ENTRY] == entry && out[HIG_DN_PLAN_FP] >= 0 && out[HIG_DN_PLAN_FP] % 32 == 0 && (out[HIG_DN_PLAN_FP] > 0) == out[HIG_DN_PLAN_EDGE16]);
        for (int i = 1; i < NS; ++i) if (i != HIG_DN_PLAN_FP) EXPECT(out[i] == 0 || out[i] == 1);
        const int forks = out[HIG_DN_PLAN_TEXT_FORK] | out[HIG_DN_PLAN_SPLIT] | out[HIG_DN_PLAN_FORK_EMB] | out[HIG_DN_PLAN_FORK_TEXT] | out[HIG_DN_PLAN_WGRAD_FORK];
        EXPECT(!forks || out[HIG_DN_PLAN_WANTS_SIDE_STREAM]);
      }
      return rc;
    };
    const int ext[] = {0, 1, 15, 16, 17, 31, 32, 33, 511, 512, 513, 8191, 8192, 8193, INT32_MAX};
    for (int entry = -1; entry <= HIG_DN_ENTRY_BWD16 + 1; ++entry) for (int storage = 0; storage <= 1; ++storage)
      for (int B : ext) for (int T : ext) for (int L : {0, 1, 31, 32, 33, INT32_MAX}) for (int F : {0, 150, 513, INT32_MAX}) for (int d : {0, 64, 512, 1024, INT32_MAX})
        for (int flags = 0; flags < 16; flags += 1 + (B & 1)) {
          hig_dims D = dims(B, T, F, d, 8, 1024, L, (T & 1) ? 0 : (B & 2), storage, 0, flags % 3);
          D.num_frames = INT32_MAX;
          const int rc = ask(D, entry, flags, (flags * 3 + (L & 7)) & 7, (flags & 4) ? 128 : 256, nullptr, NS);
          if (entry < 0 || entry > HIG_DN_ENTRY_BWD16 || B <= 0 || T <= 0 || L <= 0 || F <= 0 || d <= 0 || d > 1024) EXPECT(rc < 0);
        }
    const hig_dims shapes16[] = {dims(32, 196, 150, 512, 8, 1024, 8, 0, 1, 0, 0), dims(96, 256, 150, 512, 8, 1024, 8, 0, 1, 0, 0), dims(97, 256, 150, 512, 8, 1024, 8, 0, 1, 0, 0),
                                 dims(32, 300, 150, 1024, 8, 1024, 12, 0, 1, 0, 0), dims(64, 91, 263, 512, 8, 1024, 8, 1, 1, 0, 0), dims(1, 583, 150, 512, 8, 1024, 8, 0, 1, 0, 0)};
    const hig_dims shapes32[] = {dims(64, 196, 150, 512, 8, 1024, 8, 0, 0, 0, 0), dims(16, 512, 150, 256, 4, 512, 2, 0, 0, 0, 1), dims(16, 511, 150, 256, 4, 512, 33, 0, 0, 0, 2),
                                 dims(64, 91, 263, 512, 8, 1024, 8, 1, 0, 0, 0), dims(2, 196, 150, 512, 8, 1024, 8, 0, 0, 1, 0)};
    for (int entry = 0; entry <= HIG_DN_ENTRY_BWD16; ++entry) {
      const bool bf = entry == HIG_DN_ENTRY_TEXT16 || entry == HIG_DN_ENTRY_FWD16 || entry == HIG_DN_ENTRY_FWD16_TRAIN || entry == HIG_DN_ENTRY_BWD16;
      for (int s = 0; s < (bf ? 6 : 5); ++s) for (int flags = 0; flags < 16; ++flags) for (int facts = 0; facts < 8; ++facts) for (int cus : {1, 128, 256, INT32_MAX}) {
        const hig_dims& D = bf ? shapes16[s] : shapes32[s];
        for (int k = 0; k < HIG_DN_NSWITCHES; ++k) for (int v : {-1, 0, 1, 2, 1000, INT32_MAX, INT32_MIN}) {
          int32_t sw[HIG_DN_NSWITCHES];
          memcpy(sw, dflt, sizeof(sw));
          sw[k] = v;
          EXPECT(ask(D, entry, flags, facts, cus, sw, NS) == HIG_OK);
        }
        for (int v : {-1, 0, 1, 2, 1000}) {
          int32_t sw[HIG_DN_NSWITCHES];
          for (int k = 0; k < HIG_DN_NSWITCHES; ++k) sw[k] = v;
          EXPECT(ask(D, entry, flags, facts, cus, sw, NS) == HIG_OK);
        }
        for (int n_out : {INT32_MIN, -1, 0, 1, NS - 1, NS + 1, INT32_MAX}) EXPECT(ask(D, entry, flags, facts, cus, dflt, n_out) == HIG_OK);
      }
    }
    EXPECT(served > 1000 && refused > 1000);
    EXPECT(hig_denoiser_plan(nullptr, 0, 0, 0, 0, 0, 256, 1, nullptr, out, NS) == HIG_EINVAL);
    EXPECT(hig_denoiser_last_schedule(out, NS) == -1 && hig_denoiser_last_schedule(nullptr, 0) == -1);       // no entry point has run here
  }
  // ---- sampler entries (ddpm.hip): the fused updates, the impositions and the combine.  Every call below is refused, and a
  // refusal returns before any HIP call; the pointers are made up, nothing may read through them.  The last case is an extent
  // B * per_sample (twice that over the stacked layout) that does not fit an int64: refused, not computed.  (hig_p_sample_step
  // does not look at nsteps, hig_cfg_combine has none.) ----
  {
    struct A { float* p[5]; uint8_t* mask; float scale, eta; int32_t nsteps, B, group; int64_t per; };   // p: x, eps | known, aux, t, tab
    enum { X = 0, EPS, AUX, T, TAB, NP, MASK = NP };
    const uintptr_t base = (uintptr_t)1 << 32;
    A good;
    for (int i = 0; i < NP; ++i) good.p[i] = reinterpret_cast<float*>(base * (i + 1));
    good.mask = reinterpret_cast<uint8_t*>(base * 7);
    good.scale = 2.5f; good.eta = 0.5f; good.nsteps = 10; good.B = 4; good.group = 2; good.per = 6;
    struct E { const char* name; int (*call)(const A&); unsigned required; bool guided, has_scale, has_eta, checks_nsteps; };
    const unsigned all = (1u << NP) - 1;
    const E entries[] = {
        {"hig_p_sample_step", [](const A& a) { return hig_p_sample_step(a.p[X], a.p[EPS], a.p[AUX], reinterpret_cast<const int64_t*>(a.p[T]), a.p[TAB], a.nsteps, a.B, a.per, a.p[X], nullptr, nullptr); }, all, false, false, false, false},
        {"hig_p_sample_step_cfg", [](const A& a) { return hig_p_sample_step_cfg(a.p[X], a.p[EPS], a.scale, a.p[AUX], reinterpret_cast<const int64_t*>(a.p[T]), a.p[TAB], a.nsteps, a.B, a.group, a.per, nullptr, nullptr); }, all, true, true, false, true},
        {"hig_ddim_step", [](const A& a) { return hig_ddim_step(a.p[X], a.p[EPS], a.p[AUX], reinterpret_cast<const int64_t*>(a.p[T]), a.p[TAB], a.nsteps, a.B, a.per, a.eta, 1, a.p[X], nullptr, nullptr); }, all, false, false, true, true},
        {"hig_ddim_step_cfg", [](const A& a) { return hig_ddim_step_cfg(a.p[X], a.p[EPS], a.scale, a.p[AUX], reinterpret_cast<const int64_t*>(a.p[T]), a.p[TAB], a.nsteps, a.B, a.group, a.per, a.eta, 1, nullptr, nullptr); }, all, true, true, true, true},
        {"hig_dpm2m_step", [](const A& a) { return hig_dpm2m_step(a.p[X], a.p[EPS], a.p[AUX], reinterpret_cast<const int64_t*>(a.p[T]), a.p[TAB], a.nsteps, a.B, a.per, 1, nullptr); }, all, false, false, false, true},
        {"hig_dpm2m_step_cfg", [](const A& a) { return hig_dpm2m_step_cfg(a.p[X], a.p[EPS], a.scale, a.p[AUX], reinterpret_cast<const int64_t*>(a.p[T]), a.p[TAB], a.nsteps, a.B, a.group, a.per, 1, nullptr); }, all, true, true, false, true},
        {"hig_impose_known", [](const A& a) { return hig_impose_known(a.p[X], a.p[EPS], a.mask, a.p[AUX], reinterpret_cast<const int64_t*>(a.p[T]), a.p[TAB], a.nsteps, a.B, a.per, nullptr); }, all | 1u << MASK, false, false, false, true},
        {"hig_impose_known_cfg", [](const A& a) { return hig_impose_known_cfg(a.p[X], a.p[EPS], a.mask, a.p[AUX], reinterpret_cast<const int64_t*>(a.p[T]), a.p[TAB], a.nsteps, a.B, a.group, a.per, nullptr); }, all | 1u << MASK, true, false, false, true},
        {"hig_cfg_combine", [](const A& a) { return hig_cfg_combine(a.p[EPS], a.scale, a.B, a.group, a.per, a.p[X], nullptr); }, 1u << X | 1u << EPS, true, true, false, false},
    };
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    for (const E& e : entries) {
      int refusals = 0;
      auto refused = [&](const A& a) {
        const int rc = e.call(a);
        if (rc != HIG_EINVAL) fprintf(stderr, "driver.cpp: %s returned %d, refusal %d\n", e.name, rc, refusals);
        EXPECT(rc == HIG_EINVAL);
        EXPECT(hig_last_error(msg, sizeof(msg)) >= 0 && strstr(msg, e.name) != nullptr);
        ++refusals;
      };
      A a;
      for (int i = 0; i <= MASK; ++i) {
        if (!(e.required >> i & 1)) continue;
        if (i == AUX && e.has_eta) continue;                         // (z may be NULL at eta == 0: its own case below)
        a = good;
        if (i == MASK) a.mask = nullptr; else a.p[i] = nullptr;
        refused(a);
      }
      for (int v : {0, -2, INT32_MIN}) {
        a = good; a.B = v; refused(a);
        a = good; a.per = v; refused(a);
        if (e.checks_nsteps) { a = good; a.nsteps = v; refused(a); }
        if (e.guided) { a = good; a.group = v; refused(a); }
      }
      a = good; a.per = INT64_MIN; refused(a);
      if (e.guided) { a = good; a.group = 3; refused(a); }             // B % group != 0
      if (e.has_scale) for (float v : {nan, inf, -inf}) { a = good; a.scale = v; refused(a); }
      if (e.has_eta) {
        for (float v : {-1.0f, nan, inf, -inf}) { a = good; a.eta = v; refused(a); }
        a = good; a.p[AUX] = nullptr; refused(a);                      // z == NULL with eta != 0
      }
      a = good; a.per = INT64_MAX / (e.guided ? 4 : 2); refused(a);    // 4 [x 2] rows of that many elements
      a = good; a.per = INT64_MAX; refused(a);
      a = good; a.B = INT32_MAX; a.group = e.guided ? INT32_MAX : a.group; a.per = INT64_MAX / INT32_MAX + 1; refused(a);
      EXPECT(refusals >= 11);
    }
  }
  // ---- diagnostics pointers: set and cleared ----
  EXPECT(hig_gemm_bf16_debug_stamps(nullptr) == HIG_OK && hig_gemm_ws16_debug_stamps(nullptr) == HIG_OK &&
         hig_gemm_debug_stamps(nullptr) == HIG_OK);
  // ---- the layouts of the bf16 training step by named slot, and the tap of its backward: refusals before any HIP call ----
  {
    hig_dims T16 = dims(4, 21, 12, 128, 2, 96, 2, 1, 1, 0, 0);       // two-person, bf16 storage, linear attention
    hig_dims F32 = dims(4, 21, 12, 128, 2, 96, 2, 1, 0, 0, 0);
    int64_t v[64];
    const int tables[][2] = {{HIG_LAYOUT16_FWD, HIG_FW16_NSLOTS}, {HIG_LAYOUT16_TEXT, HIG_TX16_NSLOTS}, {HIG_LAYOUT16_BWD, HIG_BW16_NSLOTS},
                             {HIG_LAYOUT16_TAP, HIG_TAP16_NSLOTS}};
    for (const auto& t : tables) {
      for (int64_t& x : v) x = -7;
      EXPECT(hig_bf16_train_layout(&T16, t[0], v, 64) == t[1]);
      for (int s = 0; s < 64; ++s) EXPECT(s < t[1] ? v[s] >= 0 : v[s] == -7);         // (the two-person model has every member)
      for (int64_t& x : v) x = -7;
      EXPECT(hig_bf16_train_layout(&T16, t[0], v, 3) == t[1] && v[2] >= 0 && v[3] == -7);   // n_out is respected
      EXPECT(hig_bf16_train_layout(&T16, t[0], nullptr, 64) == t[1]);
    }
    EXPECT(hig_bf16_train_layout(&T16, HIG_LAYOUT16_FWD, v, 64) == HIG_FW16_NSLOTS && v[HIG_FW16_TOTAL] == hig_workspace_bytes(&T16, 1));
    EXPECT(hig_bf16_train_layout(&T16, HIG_LAYOUT16_TEXT, v, 64) == HIG_TX16_NSLOTS && v[HIG_TX16_TOTAL] == hig_textctx_bytes(&T16, 1));
    EXPECT(hig_bf16_train_layout(&T16, HIG_LAYOUT16_BWD, v, 64) == HIG_BW16_NSLOTS && v[HIG_BW16_TOTAL] == hig_bwd_workspace_bytes(&T16) &&
           v[HIG_BW16_MP] == 128);
    EXPECT(hig_bf16_train_layout(&T16, HIG_LAYOUT16_TAP, v, 64) == HIG_TAP16_NSLOTS && v[HIG_TAP16_TOTAL] == hig_denoiser_bwd_bf16_tap_bytes(&T16));
    hig_dims one = T16; one.two_person = 0;
    EXPECT(hig_bf16_train_layout(&one, HIG_LAYOUT16_TAP, v, 64) == HIG_TAP16_NSLOTS && v[HIG_TAP16_INT_DA] == -1 && v[HIG_TAP16_TOK0] == -1 &&
           v[HIG_TAP16_SA_DH] > 0);
    EXPECT(hig_bf16_train_layout(&one, HIG_LAYOUT16_FWD, v, 64) == HIG_FW16_NSLOTS && v[HIG_FW16_H2B] == -1 && v[HIG_FW16_LENP] == -1);
    EXPECT(hig_bf16_train_layout(&T16, 4, v, 64) == HIG_EINVAL && hig_bf16_train_layout(&T16, -1, v, 64) == HIG_EINVAL);
    EXPECT(hig_bf16_train_layout(nullptr, HIG_LAYOUT16_FWD, v, 64) < 0 && hig_bf16_train_layout(&F32, HIG_LAYOUT16_FWD, v, 64) == HIG_EINVAL);
    EXPECT(hig_denoiser_bwd_bf16_tap_bytes(nullptr) < 0 && hig_denoiser_bwd_bf16_tap_bytes(&F32) == HIG_EINVAL);
    const int64_t need = hig_denoiser_bwd_bf16_tap_bytes(&T16);
    EXPECT(need > 0 && need % 256 == 0);
    void* fake = reinterpret_cast<void*>((uintptr_t)1 << 32);
    EXPECT(hig_denoiser_bwd_bf16_debug_tap(fake, 0) == HIG_EINVAL && hig_denoiser_bwd_bf16_debug_tap(fake, -1) == HIG_EINVAL);
    // a tap buffer one byte short: the backward is refused before it touches the device or any of its arguments
    EXPECT(hig_denoiser_bwd_bf16_debug_tap(fake, need - 1) == HIG_OK);
    const void* tab[1] = {nullptr};
    void* gtab[1] = {nullptr};
    const float* ff = static_cast<const float*>(fake);
    const int64_t* fi = static_cast<const int64_t*>(fake);
    EXPECT(hig_denoiser_bwd_bf16(&T16, tab, tab, ff, fi, fi, ff, fake, fake, ff, gtab, nullptr, static_cast<float*>(fake), static_cast<float*>(fake), fake,
                                 nullptr) == HIG_EINVAL);
    EXPECT(hig_last_error(msg, sizeof(msg)) >= 0 && strstr(msg, "tap buffer") != nullptr);
    EXPECT(hig_denoiser_bwd_bf16_debug_tap(nullptr, 0) == HIG_OK);
  }
  // ---- the same for the fp32 training step (hig_f32_train_layout, hig_denoiser_bwd_debug_tap) ----
  {
    hig_dims T32 = dims(4, 21, 12, 128, 2, 96, 2, 1, 0, 0, 0);       // two-person, fp32 storage, linear attention
    hig_dims B16 = dims(4, 21, 12, 128, 2, 96, 2, 1, 1, 0, 0);
    int64_t v[64];
    const int tables[][2] = {{HIG_LAYOUT32_FWD, HIG_FW32_NSLOTS}, {HIG_LAYOUT32_TEXT, HIG_TX32_NSLOTS}, {HIG_LAYOUT32_BWD, HIG_BW32_NSLOTS},
                             {HIG_LAYOUT32_TAP, HIG_TAP32_NSLOTS}};
    for (const auto& t : tables) {
      for (int64_t& x : v) x = -7;
      EXPECT(hig_f32_train_layout(&T32, t[0], v, 64) == t[1]);
      for (int s = t[1]; s < 64; ++s) EXPECT(v[s] == -7);
      for (int64_t& x : v) x = -7;
      EXPECT(hig_f32_train_layout(&T32, t[0], v, 3) == t[1] && v[2] >= 0 && v[3] == -7);   // n_out is respected
      EXPECT(hig_f32_train_layout(&T32, t[0], nullptr, 64) == t[1]);
    }
    EXPECT(hig_f32_train_layout(&T32, HIG_LAYOUT32_FWD, v, 64) == HIG_FW32_NSLOTS && v[HIG_FW32_TOTAL] == hig_workspace_bytes(&T32, 1) &&
           v[HIG_FW32_H2B] > 0 && v[HIG_FW32_LSE1] == -1);
    EXPECT(hig_f32_train_layout(&T32, HIG_LAYOUT32_TEXT, v, 64) == HIG_TX32_NSLOTS && v[HIG_TX32_TOTAL] == hig_textctx_bytes(&T32, 1));
    EXPECT(hig_f32_train_layout(&T32, HIG_LAYOUT32_BWD, v, 64) == HIG_BW32_NSLOTS && v[HIG_BW32_TOTAL] == hig_bwd_workspace_bytes(&T32) &&
           v[HIG_BW32_DELTA] == -1 && v[HIG_BW32_TOK0] > 0);
    EXPECT(hig_f32_train_layout(&T32, HIG_LAYOUT32_TAP, v, 64) == HIG_TAP32_NSLOTS && v[HIG_TAP32_TOTAL] == hig_denoiser_bwd_tap_bytes(&T32) &&
           v[HIG_TAP32_INT_DA] >= 0 && v[HIG_TAP32_SA_DELTA] == -1);
    hig_dims one = T32; one.two_person = 0;
    EXPECT(hig_f32_train_layout(&one, HIG_LAYOUT32_TAP, v, 64) == HIG_TAP32_NSLOTS && v[HIG_TAP32_INT_DA] == -1 && v[HIG_TAP32_TOK0] == -1 &&
           v[HIG_TAP32_SA_DH] > 0);
    EXPECT(hig_f32_train_layout(&one, HIG_LAYOUT32_FWD, v, 64) == HIG_FW32_NSLOTS && v[HIG_FW32_H2B] == -1 && v[HIG_FW32_LENP] == -1);
    EXPECT(hig_f32_train_layout(&T32, 4, v, 64) == HIG_EINVAL && hig_f32_train_layout(&T32, -1, v, 64) == HIG_EINVAL);
    EXPECT(hig_f32_train_layout(nullptr, HIG_LAYOUT32_FWD, v, 64) < 0 && hig_f32_train_layout(&B16, HIG_LAYOUT32_FWD, v, 64) == HIG_EINVAL);
    EXPECT(hig_denoiser_bwd_tap_bytes(nullptr) < 0 && hig_denoiser_bwd_tap_bytes(&B16) == HIG_EINVAL);
    const int64_t need = hig_denoiser_bwd_tap_bytes(&T32);
    EXPECT(need > 0 && need % 256 == 0);
    void* fake = reinterpret_cast<void*>((uintptr_t)1 << 32);
    EXPECT(hig_denoiser_bwd_debug_tap(fake, 0) == HIG_EINVAL && hig_denoiser_bwd_debug_tap(fake, -1) == HIG_EINVAL);
    // a tap buffer one byte short: the backward is refused before it touches the device or any of its arguments
    EXPECT(hig_denoiser_bwd_debug_tap(fake, need - 1) == HIG_OK);
    const void* tab[1] = {nullptr};
    void* gtab[1] = {nullptr};
    const float* ff = static_cast<const float*>(fake);
    const int64_t* fi = static_cast<const int64_t*>(fake);
    EXPECT(hig_denoiser_bwd(&T32, tab, ff, fi, fi, ff, fake, fake, ff, gtab, nullptr, static_cast<float*>(fake), static_cast<float*>(fake), fake,
                            nullptr) == HIG_EINVAL);
    EXPECT(hig_last_error(msg, sizeof(msg)) >= 0 && strstr(msg, "tap buffer") != nullptr);
    EXPECT(hig_denoiser_bwd_debug_tap(nullptr, 0) == HIG_OK);
  }
  // ---- the encoder chains (text head, evaluation classifiers, CLIP text tower): the layouts by named slot and the eleven size
  // queries over small dims.  None makes a HIP call. ----
  {
    auto tdims = [](int B, int N, int W, int Lt, int H, int ff, int L, int E) {
      hig_text_dims t;
      memset(&t, 0, sizeof(t));
      t.B = B; t.N = N; t.W = W; t.Lt = Lt; t.H = H; t.ff = ff; t.L = L; t.E = E; t.prec = HIG_PREC_F32;
      return t;
    };
    auto edims = [](int B, int T, int F, int d, int H, int ff, int L, int cls) {
      hig_eval_dims e;
      memset(&e, 0, sizeof(e));
      e.B = B; e.T = T; e.F = F; e.d = d; e.H = H; e.ff = ff; e.L = L; e.C = cls ? 2 : 26; e.cls = cls; e.prec = HIG_PREC_F32;
      return e;
    };
    int64_t v[64];
    static_assert(HIG_TFW_NSLOTS < 64 && HIG_TBW_NSLOTS < 64 && HIG_EFW_NSLOTS < 64 && HIG_EBW_NSLOTS < 64 && HIG_ETAP_NSLOTS < 64, "v holds every table");
    // a table of n slots whose slot `total` times 4 is `bytes`: every offset a multiple of 64 floats inside the total (`extent`: a
    // slot that is a length, not an offset), -1 exactly on the slots of `absent`, n_out respected, a NULL out allowed
    auto held = [&](auto layout, const auto& D, int which, int n, int total, int extent, int64_t bytes, std::initializer_list<int> absent) {
      for (int64_t& x : v) x = -7;
      EXPECT(layout(&D, which, v, 64) == n);
      EXPECT(bytes > 0 && v[total] * 4 == bytes);
      for (int s = 0; s < 64; ++s) {
        bool gone = false;
        for (int a : absent) gone = gone || a == s;
        if (s >= n) EXPECT(v[s] == -7);
        else if (gone) EXPECT(v[s] == -1);
        else if (s == extent) EXPECT(v[s] > 0);
        else EXPECT(v[s] >= 0 && v[s] % 64 == 0 && v[s] <= v[total]);
      }
      const int64_t v2 = v[2];
      for (int64_t& x : v) x = -7;
      EXPECT(layout(&D, which, v, 3) == n && v[2] == v2 && v[3] == -7);
      for (int64_t& x : v) x = -7;
      EXPECT(layout(&D, which, v, 0) == n && layout(&D, which, v, -1) == n && v[0] == -7);
      EXPECT(layout(&D, which, nullptr, 64) == n);
      EXPECT(layout(&D, 3, v, 64) == HIG_EINVAL && layout(&D, -1, v, 64) == HIG_EINVAL && v[0] == -7);
    };
    const hig_text_dims texts[] = {tdims(4, 24, 64, 64, 8, 128, 2, 128), tdims(3, 77, 64, 32, 4, 64, 2, 128), tdims(3, 77, 128, 128, 2, 128, 1, 256)};
    for (const hig_text_dims& t : texts) {
      held(hig_text_head_layout, t, HIG_ENC_LAYOUT_FWD, HIG_TFW_NSLOTS, HIG_TFW_TOTAL, -1, hig_text_head_workspace_bytes(&t, 1), {});
      held(hig_text_head_layout, t, HIG_ENC_LAYOUT_BWD, HIG_TBW_NSLOTS, HIG_TBW_TOTAL, HIG_TBW_SLAB_FLOATS, hig_text_head_bwd_workspace_bytes(&t), {});
      held(hig_text_head_layout, t, HIG_ENC_LAYOUT_TAP, HIG_ETAP_NSLOTS, HIG_ETAP_TOTAL, -1, hig_text_head_bwd_tap_bytes(&t), {HIG_ETAP_DH_L, HIG_ETAP_DH_0});
      // inference: the prefix and two layer blocks, whatever L is
      EXPECT(hig_text_head_layout(&t, HIG_ENC_LAYOUT_FWD, v, 64) == HIG_TFW_NSLOTS);
      EXPECT(hig_text_head_workspace_bytes(&t, 0) == (v[HIG_TFW_LAYER0] + 2 * v[HIG_TFW_LSTRIDE]) * 4);
      EXPECT(v[HIG_TFW_TOTAL] == v[HIG_TFW_LAYER0] + t.L * v[HIG_TFW_LSTRIDE]);
    }
    for (int cls = 0; cls <= 1; ++cls) {
      const hig_eval_dims evals[] = {edims(4, 12, 15, 64, 8, 128, 2, cls), edims(4, 33, 15, 128, 2, 128, 2, cls), edims(4, 5, 15, 1024, 8, 64, 1, cls)};
      for (const hig_eval_dims& e : evals) {
        if (cls) {
          held(hig_eval_encoder_layout, e, HIG_ENC_LAYOUT_FWD, HIG_EFW_NSLOTS, HIG_EFW_TOTAL, -1, hig_eval_encoder_train_workspace_bytes(&e), {HIG_EFW_O, HIG_EFW_FEAT});
          held(hig_eval_encoder_layout, e, HIG_ENC_LAYOUT_BWD, HIG_EBW_NSLOTS, HIG_EBW_TOTAL, HIG_EBW_SLAB_FLOATS, hig_eval_encoder_bwd_workspace_bytes(&e),
               {HIG_EBW_DFT, HIG_EBW_G, HIG_EBW_GN, HIG_EBW_G2, HIG_EBW_POOL1, HIG_EBW_POOL2, HIG_EBW_U1, HIG_EBW_U2});
        } else {
          held(hig_eval_encoder_layout, e, HIG_ENC_LAYOUT_FWD, HIG_EFW_NSLOTS, HIG_EFW_TOTAL, -1, hig_eval_encoder_train_workspace_bytes(&e), {});
          held(hig_eval_encoder_layout, e, HIG_ENC_LAYOUT_BWD, HIG_EBW_NSLOTS, HIG_EBW_TOTAL, HIG_EBW_SLAB_FLOATS, hig_eval_encoder_bwd_workspace_bytes(&e), {});
        }
        held(hig_eval_encoder_layout, e, HIG_ENC_LAYOUT_TAP, HIG_ETAP_NSLOTS, HIG_ETAP_TOTAL, -1, hig_eval_encoder_bwd_tap_bytes(&e), {HIG_ETAP_DXF_TOTAL, HIG_ETAP_DGATH});
        const int64_t inf = hig_eval_encoder_workspace_bytes(&e);
        EXPECT(inf > 0 && inf % 256 == 0);
      }
    }
    // illegal and NULL dims: every entry refuses, with the message of the dims check
    {
      hig_text_dims t = texts[0];
      hig_eval_dims e = edims(4, 12, 15, 64, 8, 128, 2, 0);
      auto text_refused = [&](const hig_text_dims* p) {
        return hig_text_head_layout(p, HIG_ENC_LAYOUT_FWD, v, 64) == HIG_EINVAL && hig_text_head_workspace_bytes(p, 0) == -1 && hig_text_head_workspace_bytes(p, 1) == -1 &&
               hig_text_head_bwd_workspace_bytes(p) == -1 && hig_text_head_bwd_tap_bytes(p) == HIG_EINVAL;
      };
      auto eval_refused = [&](const hig_eval_dims* p) {
        return hig_eval_encoder_layout(p, HIG_ENC_LAYOUT_BWD, v, 64) == HIG_EINVAL && hig_eval_encoder_workspace_bytes(p) == -1 &&
               hig_eval_encoder_train_workspace_bytes(p) == -1 && hig_eval_encoder_bwd_workspace_bytes(p) == -1 && hig_eval_encoder_bwd_tap_bytes(p) == HIG_EINVAL;
      };
      EXPECT(text_refused(nullptr) && eval_refused(nullptr));
      hig_text_dims tb = t; tb.B = 0;      EXPECT(text_refused(&tb));
      tb = t; tb.H = 5;                    EXPECT(text_refused(&tb));                          // Lt % H
      tb = t; tb.Lt = 28; tb.H = 4;        EXPECT(text_refused(&tb));                          // head dim 7
      EXPECT(hig_last_error(msg, sizeof(msg)) >= 0 && strcmp(msg, "hig text head: head dim 7 not in {8,16,32,64,128}") == 0);
      tb = t; tb.ff = 130;                 EXPECT(text_refused(&tb));
      tb = t; tb.Lt = 2048; tb.H = 16;     EXPECT(text_refused(&tb));                          // Lt > 1024
      tb = t; tb.prec = 7;                 EXPECT(text_refused(&tb));
      EXPECT(hig_last_error(msg, sizeof(msg)) >= 0 && strcmp(msg, "hig: unknown prec=7") == 0);
      tb = t; tb.L = INT32_MIN;            EXPECT(text_refused(&tb));
      hig_eval_dims eb = e; eb.T = 1;      EXPECT(eval_refused(&eb));
      eb = e; eb.F = 3;                    EXPECT(eval_refused(&eb));
      eb = e; eb.d = 48; eb.H = 4;         EXPECT(eval_refused(&eb));                          // head dim 12
      EXPECT(hig_last_error(msg, sizeof(msg)) >= 0 && strcmp(msg, "hig eval encoder: head dim 12 not in {8,16,32,64,128}") == 0);
      eb = e; eb.d = 2048; eb.H = 16;      EXPECT(eval_refused(&eb));                          // d > 1024
      eb = e; eb.prec = -1;                EXPECT(eval_refused(&eb));
      eb = e; eb.C = 0;                    EXPECT(eval_refused(&eb));
    }
    // the tower: positive sizes in whole 256-byte granules; training sizes only with exact-fp32 products
    {
      auto cd = [](int32_t* d, int B, int N, int W, int H, int L, int vocab, int prec) {
        for (int i = 0; i < HIG_CD_NSLOTS; ++i) d[i] = 0;
        d[HIG_CD_B] = B; d[HIG_CD_N] = N; d[HIG_CD_W] = W; d[HIG_CD_H] = H; d[HIG_CD_L] = L; d[HIG_CD_VOCAB] = vocab; d[HIG_CD_PREC] = prec;
      };
      int32_t d[HIG_CD_NSLOTS];
      const int towers[][6] = {{3, 77, 128, 2, 2, 64}, {2, 20, 512, 8, 2, 49408}, {27, 77, 128, 2, 1, 64}, {1, 128, 64, 1, 1, 2}};
      for (const auto& c : towers) {
        cd(d, c[0], c[1], c[2], c[3], c[4], c[5], HIG_PREC_F32);
        const int64_t inf = hig_clip_text_workspace_bytes(d), tr = hig_clip_text_train_bytes(d), bw = hig_clip_text_bwd_workspace_bytes(d);
        EXPECT(inf > 0 && tr > 0 && bw > 0 && inf % 256 == 0 && tr % 256 == 0 && bw % 256 == 0);
        EXPECT(bw >= (int64_t)1536 * 128 * 128 * 4);                                           // (the split-R slabs alone)
        cd(d, c[0], c[1], c[2], c[3], c[4], c[5], HIG_PREC_BF16);
        EXPECT(hig_clip_text_workspace_bytes(d) == inf && hig_clip_text_train_bytes(d) == -1 && hig_clip_text_bwd_workspace_bytes(d) == -1);
        EXPECT(hig_last_error(msg, sizeof(msg)) >= 0 && strstr(msg, "hig_clip_text_bwd_workspace_bytes: prec=") != nullptr);
      }
      auto refused = [&]() { return hig_clip_text_workspace_bytes(d) == -1 && hig_clip_text_train_bytes(d) == -1 && hig_clip_text_bwd_workspace_bytes(d) == -1; };
      cd(d, 3, 77, 128, 4, 2, 64, 0);    EXPECT(refused());                                    // head dim 32
      cd(d, 3, 129, 128, 2, 2, 64, 0);   EXPECT(refused());                                    // N > 128
      cd(d, 3, 77, 2048, 32, 2, 64, 0);  EXPECT(refused());                                    // W > 1024
      cd(d, 0, 77, 128, 2, 2, 64, 0);    EXPECT(refused());
      cd(d, 3, 77, 128, 2, 2, 64, 9);    EXPECT(refused());
      EXPECT(hig_last_error(msg, sizeof(msg)) >= 0 && strcmp(msg, "hig: unknown prec=9") == 0);
      EXPECT(hig_clip_text_workspace_bytes(nullptr) == -1 && hig_clip_text_train_bytes(nullptr) == -1 && hig_clip_text_bwd_workspace_bytes(nullptr) == -1);
    }
  }
  if (failures) {
    fprintf(stderr, "%d expectation(s) failed\n", failures);
    return 1;
  }
  printf("host entry points clean\n");
  return 0;
}
