// Which kernel serves an attention call, and with which split: hig_attn_plan_for (every entry point of linattn.hip and
// fullattn.hip).
//
// Host code only.  A plan is a pure function of the call (hig_attn_call: extents, entry, I/O type, the facts the entry point
// read off its operands), the switches (hig_attn_switches), the chip's CU count and whether the device grants the big
// dynamic LDS: no HIP call, no error state, no launch counted, no operand dereferenced.  The entry points build the call,
// plan it here, then switch on plan.path into a launcher next to the kernel, which decides nothing.  Every eligibility
// condition is one named predicate used from one place; the one split rule is walk_split, its targets are the named
// functions next to it, each with the measurement behind it.
#include <stdarg.h>
#include <stdio.h>

#include "hig_host.h"

namespace {

constexpr int CH = 64;   // rows per chunk of the linear-attention kernels and per block of the VALU full-attention kernels

hig_attn_plan_t served(int path, int64_t split, int variant = 0) {
  hig_attn_plan_t p;
  p.rc = HIG_OK; p.path = path; p.split = (int)split; p.variant = variant; p.msg[0] = 0;
  return p;
}
hig_attn_plan_t refused(int rc, const char* fmt, ...) {
  hig_attn_plan_t p = served(-1, 0);
  p.rc = rc;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(p.msg, sizeof(p.msg), fmt, ap);
  va_end(ap);
  return p;
}

int64_t blocks_of(int64_t rows, int per) { return (rows + per - 1) / per; }

// ---- the split rule ----
// Chunk-walking workgroups: aim at `target` workgroups on the chip, i.e. ceil(target / BH) of them share the `blocks` chunks
// of one (sample, head), at least one and at most one per chunk.
int64_t walk_split(int64_t target, int64_t BH, int64_t blocks) {
  const int64_t gy = (target + BH - 1) / BH;
  return gy < 1 ? 1 : (gy > blocks ? blocks : gy);
}
// apply_mfma_kernel: enough workgroups to fill the chip (~4 per CU), each staging A[b,h] once.
// (hd = 128 keeps 97 KB of LDS per workgroup = one per CU: fewer, longer-lived workgroups; measured with
// tools/attn_time.py: 61 -> 47 us at config 5, neutral at hd = 64)
// (re-swept in round 2, profiles/r02_attn_sweep.md: hd = 128 at 256 / 512 / 1024 workgroups: 42.4 / 48.7 / 58.9 us)
int64_t apply_target(int hd, int cus) { return (int64_t)(hd == 128 ? 1 : 4) * cus; }
// apply_bwd_mfma_kernel / ctx_bwd_mfma_kernel (dA accumulated in registers across a workgroup's chunks): ~3 per CU resident.
// measured (tools/attn_time.py): one workgroup per (sample, head) walking all its chunks is fastest once
// B * H fills the chip (config 2: 49 -> 38 us, config 5: 135 -> 77 us) and needs no partial sums at all
int64_t bwd_target(int cus) { return cus; }
// ctx_mfma_kernel walks every chunk of a (sample, head) once there are enough pairs to fill the chip with walking
// workgroups; below that, with scratch, row chunks in parallel + a merge: 4-5x the workgroups of the one-per-pair kernel
bool ctx_walks(int64_t BH, int cus) { return BH >= cus; }
// apply_sty_wave64_kernel, strips per sample: enough workgroups for the 16 wave slots of each of the 256 CUs (two 8-wave or
// four 4-wave workgroups), then the fewest strips with that many tiles each (a strip's start-up -- 16 KB of A per wave from
// L2 -- is paid once per workgroup).  B = 64, T = 196, H = 8: 7 strips of 2 tiles; B = 32: 13 strips of one.  Measured
// against half and twice the slots (profiles/r07_notes.md): within 0.5 us at B = 32, 1 - 2 us slower at B = 64 with twice.
constexpr int APPLY_STY_WAVE_SLOTS = 256 * 16;
int64_t strip_split(int H, int B, int64_t tiles) {
  int64_t nstrip = APPLY_STY_WAVE_SLOTS / H / B;
  nstrip = nstrip < 1 ? 1 : (nstrip > tiles ? tiles : nstrip);
  const int64_t per = (tiles + nstrip - 1) / nstrip;
  return (tiles + per - 1) / per;
}
// Waves per workgroup of the matrix-core full-attention kernels (HIG_FULLATTN_WAVES = 2 / 4 / 8 forces one).  From the sweep
// in profiles/r02_attn_sweep.md: 8 waves (256 rows share each staged 32-row chunk; <= 256 registers per lane, two waves per
// SIMD) win the forward at both head dims and the backward at head dim 64; the head-dim-128 backward needs more than 256
// registers per lane: its 8- and 2-wave instances spilled, were never selected and are not built, so it runs 4, always.
int full_waves(bool backward, int hd, const hig_attn_switches& sw) {
  if (backward && hd == 128) return 4;
  const int f = sw.fullattn_waves;
  return (f == 2 || f == 4 || f == 8) ? f : 8;
}

// ---- the predicates ----
bool any_hd(int hd) { return hd == 8 || hd == 16 || hd == 32 || hd == 64 || hd == 128; }
// the matrix-core backward kernels of linear attention: head dim 128 needs 135 KB of dynamic LDS (of the 160 KB per CU)
bool bwd_mfma_hd(int hd, bool big_lds_ok) { return hd == 64 || (hd == 128 && big_lds_ok); }
// HIG_FULLATTN_VALU=1 keeps head dim 64 on the VALU kernels (A/B measurements); head dim 128 is matrix-core only
bool full_mfma_hd(int hd, const hig_attn_switches& sw) { return hd == 128 || (hd == 64 && !sw.fullattn_valu); }
bool sty_heads(int H) { return H == 4 || H == 8; }   // the fused apply keeps H / 4 heads per wave
bool rows_aligned(const hig_attn_call& c, int in_bytes, int out_bytes) {
  const int want = (in_bytes == 16 ? HIG_ATTN_FACT_IN16 : in_bytes == 8 ? HIG_ATTN_FACT_IN8 : 0) |
                   (out_bytes == 16 ? HIG_ATTN_FACT_OUT16 : out_bytes == 8 ? HIG_ATTN_FACT_OUT8 : 0);
  return (c.facts & want) == want;
}
// exact fp32, head dim 64: the wave-autonomous kernel (16-row tiles per wave, no barrier in the loop)
// (short sequences keep the chunk-walking kernel: T = 91 has 6 tiles for 4 waves, 11.3 against 10.1 us at B = 64)
bool wave_apply(const hig_attn_call& c, const hig_attn_switches& sw) {
  return sw.apply_wave && c.io == HIG_ATTN_IO_F32 && c.hd == 64 && c.rows >= 128 && rows_aligned(c, 16, 16);
}

// What each entry point asks before it looks at the shape.  hd_rule: which head dims it serves; hd_rc / hd_msg: what an
// unserved one returns (the fp32 linear-attention entries call it a bad argument, the others unsupported).
enum HdRule { HD_ANY, HD_MFMA, HD_BWD_MFMA, HD_STY };
struct EntrySpec {
  const char* name;
  bool needs_H, needs_Tk, needs_scratch;
  HdRule hd_rule; int hd_rc; const char* hd_msg;
  int in_bytes, out_bytes; bool par; const char* align_msg;
};
const char LIN_HD[] = "hig_linattn: head dim %d not in {8,16,32,64,128}";
const char LIN16_HD[] = "hig_linattn: bf16 storage is built for head dim 64 / 128 (got %d)";
const char FULL_HD[] = "hig_fullattn: head dim %d not in {8,16,32,64,128}";
const EntrySpec SPECS[7][2] = {
    {{"hig_linattn_ctx", true, false, false, HD_ANY, HIG_EINVAL, LIN_HD, 0, 0, false, ""},
     {"hig_linattn_ctx_bf16", true, false, false, HD_MFMA, HIG_EUNSUPPORTED, LIN16_HD, 8, 0, false, "K/V must be 8-byte aligned"}},
    {{"hig_linattn_apply", true, false, false, HD_ANY, HIG_EINVAL, LIN_HD, 16, 16, false, "Q/Y must be 16-byte aligned"},
     {"hig_linattn_apply_bf16", true, false, false, HD_MFMA, HIG_EUNSUPPORTED, LIN16_HD, 8, 16, false,
      "Q rows must be 8-byte aligned, Y rows 16-byte aligned"}},
    {{"hig_linattn_apply_sty", false, false, false, HD_STY, HIG_EUNSUPPORTED, nullptr, 16, 16, true, "alignment"},
     {"hig_linattn_apply_sty_bf16", false, false, false, HD_STY, HIG_EUNSUPPORTED, nullptr, 16, 16, true, "alignment"}},
    {{"hig_linattn_apply_bwd", true, false, true, HD_ANY, HIG_EINVAL, LIN_HD, 16, 16, false, "Q/dY/dQ must be 16-byte aligned"},
     {"hig_linattn_apply_bwd_bf16", true, false, true, HD_BWD_MFMA, HIG_EUNSUPPORTED, "hig_linattn_apply_bwd_bf16: head dim 64 or 128 (got %d)",
      8, 16, false, "Q / dY rows must be 8-byte aligned, dQ rows 16-byte aligned"}},
    {{"hig_linattn_ctx_bwd", true, false, true, HD_ANY, HIG_EINVAL, LIN_HD, 0, 16, false, "dK/dV must be 16-byte aligned"},
     {"hig_linattn_ctx_bwd_bf16", true, false, false, HD_BWD_MFMA, HIG_EUNSUPPORTED, "hig_linattn_ctx_bwd_bf16: head dim 64 or 128 (got %d)",
      8, 16, false, "K / V rows must be 8-byte aligned, dK / dV rows 16-byte aligned"}},
    {{"hig_fullattn_fwd", true, true, false, HD_ANY, HIG_EUNSUPPORTED, FULL_HD, 16, 16, false, "operands must be 16-byte aligned"},
     {"hig_fullattn_fwd_bf16", true, true, false, HD_MFMA, HIG_EUNSUPPORTED, "hig_fullattn_fwd_bf16: head dim %d not in {64,128}", 8, 8, false,
      "operands must be 8-byte aligned"}},
    {{"hig_fullattn_bwd", true, true, false, HD_ANY, HIG_EUNSUPPORTED, FULL_HD, 16, 16, false, "operands must be 16-byte aligned"},
     {nullptr, false, false, false, HD_ANY, 0, nullptr, 0, 0, false, nullptr}},
};

}  // namespace

bool hig_attn_mfma_hd(int hd) { return hd == 64 || hd == 128; }

const hig_attn_switches& hig_attn_switch_values() {
  auto env_int = [](const char* v, int dflt) { return v ? atoi(v) : dflt; };
  static const hig_attn_switches sw = {
      env_int(getenv("HIG_APPLY_WAVE"), 1),       // 0: apply_wave64_kernel off
      env_int(getenv("HIG_FULLATTN_WAVES"), 0),   // 2 / 4 / 8: force the waves per workgroup
      env_int(getenv("HIG_FULLATTN_VALU"), 0),    // != 0: head dim 64 of full attention on the VALU kernels
  };
  return sw;
}

hig_attn_plan_t hig_attn_plan_for(const hig_attn_call& c, const hig_attn_switches& sw, int cus, bool big_lds_ok) {
  const bool bf = c.io == HIG_ATTN_IO_BF16;
  if (c.entry < 0 || c.entry > HIG_ATTN_ENTRY_FULL_BWD || (c.io != HIG_ATTN_IO_F32 && !bf) || !SPECS[c.entry][c.io].name)
    return refused(HIG_EINVAL, "hig_attn_plan: no entry point %d with I/O type %d", c.entry, c.io);
  const EntrySpec& e = SPECS[c.entry][c.io];
  // 1. arguments  2. head dim (and heads)  3. alignment: every entry point, in this order
  if (!((c.facts & HIG_ATTN_FACT_OPERANDS) && (!e.needs_scratch || c.has_scratch) && c.B > 0 && c.rows > 0 && (!e.needs_Tk || c.Tk > 0) &&
        (!e.needs_H || c.H > 0)))
    return refused(HIG_EINVAL, "%s: bad arguments", e.name);
  if (e.hd_rule == HD_STY) {
    if (!hig_attn_mfma_hd(c.hd) || !sty_heads(c.H))
      return refused(HIG_EUNSUPPORTED, "%s: built for head dim 64 / 128 and 4 or 8 heads (got %d, %d)", e.name, c.hd, c.H);
  } else if (!(e.hd_rule == HD_ANY ? any_hd(c.hd) : e.hd_rule == HD_MFMA ? hig_attn_mfma_hd(c.hd) : bwd_mfma_hd(c.hd, big_lds_ok))) {
    return refused(e.hd_rc, e.hd_msg, c.hd);
  }
  if (!rows_aligned(c, e.in_bytes, e.out_bytes) || (e.par && !(c.facts & HIG_ATTN_FACT_PAR16)))
    return refused(HIG_EINVAL, "%s: %s", e.name, e.align_msg);

  const int64_t BH = (int64_t)c.B * c.H, nchunk = blocks_of(c.rows, CH);
  const bool mfma = hig_attn_mfma_hd(c.hd);
  switch (c.entry) {
    case HIG_ATTN_ENTRY_CTX:
      if (!mfma) return served(HIG_ATTN_PATH_CTX, 1);
      if (!ctx_walks(BH, cus) && c.has_scratch && nchunk > 1) return served(HIG_ATTN_PATH_CTX_PART, nchunk);
      return served(HIG_ATTN_PATH_CTX_MFMA, 1);
    case HIG_ATTN_ENTRY_APPLY:
      if (!mfma) return served(HIG_ATTN_PATH_APPLY, nchunk);
      if (wave_apply(c, sw)) return served(HIG_ATTN_PATH_APPLY_WAVE64, 1);
      return served(HIG_ATTN_PATH_APPLY_MFMA, walk_split(apply_target(c.hd, cus), BH, nchunk));
    case HIG_ATTN_ENTRY_APPLY_STY:
      if (bf || c.hd != 64) return served(HIG_ATTN_PATH_APPLY_STY, 1);
      // the wave-autonomous kernel (32-bit byte offsets into a sample's rows of Out)
      if (!(c.facts & HIG_ATTN_FACT_OUT_I32)) return refused(HIG_EINVAL, "hig_linattn_apply_sty: a sample's output rows exceed 2 GiB");
      return served(HIG_ATTN_PATH_APPLY_STY_WAVE64, strip_split(c.H, c.B, blocks_of(c.rows, 16)));
    case HIG_ATTN_ENTRY_APPLY_BWD: {
      // without the big LDS the fp32 entry falls back to the VALU kernel at head dim 128 (one workgroup and one partial per chunk)
      if (!bwd_mfma_hd(c.hd, big_lds_ok)) return served(HIG_ATTN_PATH_APPLY_BWD, nchunk, HIG_ATTN_VARIANT_MERGE);
      const int64_t nparts = walk_split(bwd_target(cus), BH, nchunk);   // dA partials per (sample, head)
      return served(HIG_ATTN_PATH_APPLY_BWD_MFMA, nparts, nparts > 1 ? HIG_ATTN_VARIANT_MERGE : 0);
    }
    case HIG_ATTN_ENTRY_CTX_BWD:
      if (!bwd_mfma_hd(c.hd, big_lds_ok)) return served(HIG_ATTN_PATH_CTX_BWD, nchunk);
      return served(HIG_ATTN_PATH_CTX_BWD_MFMA, walk_split(bwd_target(cus), BH, nchunk));   // single pass (the column term comes from A and dA)
    default: {
      const bool backward = c.entry == HIG_ATTN_ENTRY_FULL_BWD;
      if (!bf && !full_mfma_hd(c.hd, sw)) return served(backward ? HIG_ATTN_PATH_FULL_BWD : HIG_ATTN_PATH_FULL_FWD, blocks_of(c.rows, CH));
      const int waves = full_waves(backward, c.hd, sw);
      return served(backward ? HIG_ATTN_PATH_FULL_BWD_MFMA : HIG_ATTN_PATH_FULL_FWD_MFMA, blocks_of(c.rows, 32 * waves), waves);
    }
  }
}

extern "C" int hig_attn_plan(int32_t entry, int32_t io, int32_t B, int32_t rows, int32_t Tk, int32_t H, int32_t hd, int32_t has_scratch,
                             int32_t facts, int32_t chip_cus, int32_t big_lds_ok, int32_t* path, int32_t* split, int32_t* variant) {
  const hig_attn_plan_t p = hig_attn_plan_for(hig_attn_call{entry, io, B, rows, Tk, H, hd, has_scratch != 0, facts}, hig_attn_switch_values(),
                                              chip_cus > 0 ? chip_cus : hig_chip_cus(), big_lds_ok != 0);
  if (path) *path = p.path;
  if (split) *split = p.split;
  if (variant) *variant = p.variant;
  return p.rc;
}
