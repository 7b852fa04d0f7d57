"""Which kernel serves an attention call and with which split, asked of the plan entry (hig_attn_plan, csrc/attn_plan.hip)
without a GPU: it is a pure function of the extents, the operand facts, the switches, the CU count and whether the device
grants the big dynamic LDS.  tests/test_gpu_attn_contract.py asserts on the device that a call moves exactly the counter its
plan named and reports the plan's split; a dispatch regression therefore fails here first.

  - the dispatch table of tests/attn_dispatch_cases.py (shared with the GPU suite) at 256 CUs, and again at 32 / 128 / 304;
  - the split rule at the smallest shapes at which it can go wrong, against clamp(ceil(target / BH), 1, chunks) and the
    strips rule, both restated here in Python;
  - every entry's refusals with the code they have always had;
  - tests/golden/attn_dispatch_parity.json: 1388 calls of the attention entry points answered by the library as it was BEFORE
    the plan existed (decision, validation and launch interleaved in every entry), each with the counter it moved and
    hig_attn_last_split, or the error code, recorded on an MI355X.  The plan reproduces every one."""
import ctypes as C
import json
import os

import pytest

from hig_amd import _lib  # noqa: E402
from attn_dispatch_cases import (ALL, APPLY_STY, APPLY_STY_B, APPLY_STY_T, BF16, CALLS, CH, ENTRIES, F32, LIN_TABLE, PATHS,  # noqa: E402
                                 full_paths, in_regime, plan, regime_bh)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN8, IN16, OUT8, OUT16, PAR16, OUT_I32, OPERANDS = (_lib.ATTN_FACT_IN8, _lib.ATTN_FACT_IN16, _lib.ATTN_FACT_OUT8, _lib.ATTN_FACT_OUT16,
                                                      _lib.ATTN_FACT_PAR16, _lib.ATTN_FACT_OUT_I32, _lib.ATTN_FACT_OPERANDS)
EINVAL, EUNSUPPORTED = -1, -3


def cdiv(a, b):
    return -(-a // b)


def batch_of(regime, H, cus, nchunk):
    """B of the named regime on a chip of `cus` CUs, or None where the regime does not exist there: H must divide B * H, and
    'few' (an absolute 7 H pairs, the only regime that does not scale with the chip) means few enough that a workgroup per
    chunk stays within one per CU: ceil(cus / BH) >= nchunk."""
    bh = regime_bh(regime, H, cus)
    if bh < H or bh % H or (regime == "few" and cdiv(cus, bh) < nchunk):
        return None
    return bh // H


def check_row(case, cus):
    _, io, hd, H, regime, T, expect = case
    nchunk = cdiv(T, CH)
    B = batch_of(regime, H, cus, nchunk)
    if B is None:
        return 0
    for entry, (path, reg) in expect.items():
        name, scratch = CALLS[entry]
        rc, got, split, _ = plan(name, io, B, T, H, hd, scratch=scratch, chip_cus=cus)
        assert (rc, got) == (0, path), (case[0], entry, cus, rc, got)
        assert in_regime(reg, split, nchunk), "%s %s at %d CUs: split %d of %d is not '%s'" % (case[0], entry, cus, split, nchunk, reg)
    return 1


@pytest.mark.parametrize("case", LIN_TABLE, ids=[c[0] for c in LIN_TABLE])
def test_linear_table_is_planned_at_256_cus(case):
    assert check_row(case, 256) == 1, "every row of the table exists on 256 CUs"


@pytest.mark.parametrize("cus", [32, 128, 304])
def test_the_cu_count_is_an_input(cus):
    """The same rows with B * H recomputed for another chip reach the same paths and regimes."""
    assert sum(check_row(case, cus) for case in LIN_TABLE) >= 20


@pytest.mark.parametrize("cus", [32, 128, 256, 304])
def test_head_dim_128_backward_without_the_big_lds(cus):
    """The matrix-core backward kernels need 135 KB of dynamic LDS at head dim 128: where the device does not grant it the fp32
    entries run the VALU kernels (one workgroup per chunk, partial sums merged), the bf16 entries have no kernel."""
    for T in (1, 65, 300):
        for B in (1, cus // 8, cus):
            assert plan("apply_bwd", F32, B, T, 8, 128, chip_cus=cus, big_lds_ok=0) == (0, "APPLY_BWD", cdiv(T, CH), 1)
            assert plan("ctx_bwd", F32, B, T, 8, 128, chip_cus=cus, big_lds_ok=0) == (0, "CTX_BWD", cdiv(T, CH), 0)
            for entry in ("apply_bwd", "ctx_bwd"):
                assert plan(entry, BF16, B, T, 8, 128, chip_cus=cus, big_lds_ok=0)[:2] == (EUNSUPPORTED, None)
                assert plan(entry, BF16, B, T, 8, 128, facts=OPERANDS, chip_cus=cus, big_lds_ok=0)[0] == EUNSUPPORTED, "the head dim comes before the alignment"
                assert plan(entry, BF16, B, T, 8, 64, chip_cus=cus, big_lds_ok=0)[1] == plan(entry, F32, B, T, 8, 64, chip_cus=cus, big_lds_ok=0)[1]
                assert plan(entry, F32, B, T, 8, 128, chip_cus=cus, big_lds_ok=1)[1].endswith("_BWD_MFMA")


def walk(target, BH, chunks):
    return min(max(cdiv(target, BH), 1), chunks)


@pytest.mark.parametrize("cus", [256, 104])
def test_split_rule_at_its_edges(cus):
    """T on the chunk edges and on the 128-row threshold of the wave kernel, B * H just below, at and just above every target:
    split == clamp(ceil(target / BH), 1, chunks) with the targets of csrc/attn_plan.hip (4 CUs for apply_mfma_kernel at head
    dim 64, 1 CU at 128, 1 CU for both backward kernels; the context build walks from B * H >= CUs)."""
    H = 8
    for T in (1, 63, 64, 65, 127, 128, 129):
        n = cdiv(T, CH)
        for BH in (cus - H, cus, cus + H, 4 * cus - H, 4 * cus, 4 * cus + H):
            B = BH // H
            for io in (F32, BF16):
                for hd in (64, 128):
                    want = ("APPLY_WAVE64", 1) if (io, hd) == (F32, 64) and T >= 128 else ("APPLY_MFMA", walk((4 if hd == 64 else 1) * cus, BH, n))
                    assert plan("apply", io, B, T, H, hd, chip_cus=cus)[:3] == (0,) + want, (T, BH, io, hd)
                    nparts = walk(cus, BH, n)
                    assert plan("apply_bwd", io, B, T, H, hd, chip_cus=cus) == (0, "APPLY_BWD_MFMA", nparts, int(nparts > 1)), (T, BH, io, hd)
                    assert plan("ctx_bwd", io, B, T, H, hd, chip_cus=cus) == (0, "CTX_BWD_MFMA", nparts, 0), (T, BH, io, hd)
                    part = BH < cus and n > 1
                    assert plan("ctx", io, B, T, H, hd, scratch=True, chip_cus=cus)[:3] == ((0, "CTX_PART", n) if part else (0, "CTX_MFMA", 1))
                    assert plan("ctx", io, B, T, H, hd, scratch=False, chip_cus=cus)[:3] == (0, "CTX_MFMA", 1)
    # a misaligned fp32 call never reaches the wave kernel: it is refused; HIG_APPLY_WAVE is covered by tests/test_gpu_knobs.py
    assert plan("apply", F32, 4, 128, H, 64, facts=ALL & ~IN16)[0] == EINVAL


def strips(B, T, H):
    tiles = cdiv(T, 16)
    n = min(max(256 * 16 // H // B, 1), tiles)
    return cdiv(tiles, cdiv(tiles, n))


@pytest.mark.parametrize("B,T", [(64, 196), (32, 196), (1, 16), (1, 17), (4096, 196)])
def test_strips_rule(B, T):
    """apply_sty_wave64_kernel: workgroups for 16 wave slots on each of 256 CUs, then the fewest strips with that many tiles
    each; whatever the chip (the slots are a constant of the kernel's tuning)."""
    for H in (4, 8):
        for cus in (256, 64):
            assert plan("apply_sty", F32, B, T, H, 64, chip_cus=cus)[:3] == (0, "APPLY_STY_WAVE64", strips(B, T, H))
    assert (strips(64, 196, 8), strips(32, 196, 8), strips(1, 16, 8), strips(1, 17, 8), strips(4096, 196, 8)) == (7, 13, 1, 2, 1)


@pytest.mark.parametrize("io,hd,H,path,regime", APPLY_STY)
def test_apply_sty_paths(io, hd, H, path, regime):
    for T in APPLY_STY_T:
        rc, got, split, _ = plan("apply_sty", io, APPLY_STY_B, T, H, hd)
        assert (rc, got) == (0, path) and (split == 1 if regime == "one" else 1 <= split <= cdiv(T, 16))


def test_full_attention_paths_and_variants():
    """variant = waves per workgroup of the matrix-core kernels (0 on the VALU kernels), split = the query side's blocks."""
    for hd in (8, 16, 32, 64, 128):
        fwd, bwd = full_paths(hd)
        for Tq in (1, 77, 196, 257):
            if hd < 64:
                assert plan("full_fwd", F32, 2, Tq, 4, hd, Tk=77) == (0, fwd, cdiv(Tq, 64), 0)
                assert plan("full_bwd", F32, 2, Tq, 4, hd, Tk=77) == (0, bwd, cdiv(Tq, 64), 0)
                assert plan("full_fwd", BF16, 2, Tq, 4, hd, Tk=77)[:2] == (EUNSUPPORTED, None)
            else:
                wb = 4 if hd == 128 else 8
                assert plan("full_fwd", F32, 2, Tq, 4, hd, Tk=77) == (0, fwd, cdiv(Tq, 256), 8)
                assert plan("full_fwd", BF16, 2, Tq, 4, hd, Tk=77) == (0, fwd, cdiv(Tq, 256), 8)
                assert plan("full_bwd", F32, 2, Tq, 4, hd, Tk=77) == (0, bwd, cdiv(Tq, 32 * wb), wb)
    assert plan("full_bwd", BF16, 2, 77, 4, 64, Tk=77)[0] == EINVAL, "full attention has no bf16 backward"


# per entry and I/O type: (input, output) row alignment in bytes it asks for, the code of an unserved head dim, scratch required
ASKS = {("ctx", F32): (0, 0, EINVAL, False), ("ctx", BF16): (8, 0, EUNSUPPORTED, False),
        ("apply", F32): (16, 16, EINVAL, False), ("apply", BF16): (8, 16, EUNSUPPORTED, False),
        ("apply_sty", F32): (16, 16, EUNSUPPORTED, False), ("apply_sty", BF16): (16, 16, EUNSUPPORTED, False),
        ("apply_bwd", F32): (16, 16, EINVAL, True), ("apply_bwd", BF16): (8, 16, EUNSUPPORTED, True),
        ("ctx_bwd", F32): (0, 16, EINVAL, True), ("ctx_bwd", BF16): (8, 16, EUNSUPPORTED, False),
        ("full_fwd", F32): (16, 16, EUNSUPPORTED, False), ("full_fwd", BF16): (8, 8, EUNSUPPORTED, False),
        ("full_bwd", F32): (16, 16, EUNSUPPORTED, False)}


@pytest.mark.parametrize("entry,io", list(ASKS), ids=["%s-%s" % k for k in ASKS])
def test_refusals_keep_their_codes(entry, io):
    need_in, need_out, hd_rc, needs_scratch = ASKS[(entry, io)]
    ok = dict(B=4, rows=130, H=4, hd=64, Tk=77)

    def rc(facts=ALL, scratch=True, **over):
        a = dict(ok, **over)
        got = plan(entry, io, a["B"], a["rows"], a["H"], a["hd"], Tk=a["Tk"], scratch=scratch, facts=facts)
        assert got[0] == 0 or got[1:] == (None, 0, 0)
        return got[0]

    assert rc() == 0
    # bad arguments come first, whatever else is wrong with the call
    for bad in (dict(B=0), dict(B=-1), dict(rows=0), dict(rows=-5)) + ((dict(Tk=0),) if entry.startswith("full") else ()):
        assert rc(**bad) == EINVAL and rc(hd=48, **bad) == EINVAL and rc(facts=0, **bad) == EINVAL
    assert rc(facts=ALL & ~OPERANDS) == EINVAL and rc(facts=ALL & ~OPERANDS, hd=48) == EINVAL
    assert rc(H=0) == (EUNSUPPORTED if entry == "apply_sty" else EINVAL)
    assert rc(scratch=False) == (EINVAL if needs_scratch else 0)
    # then the head dim (before the alignment)
    for hd in (48, 0, 256, -64):
        assert rc(hd=hd) == hd_rc and rc(hd=hd, facts=OPERANDS) == hd_rc
    assert rc(hd=32) == (0 if hd_rc == EINVAL or (entry.startswith("full") and io == F32) else EUNSUPPORTED)
    if entry == "apply_sty":
        assert [rc(H=h) for h in (2, 3, 4, 8, 16)] == [EUNSUPPORTED, EUNSUPPORTED, 0, 0, EUNSUPPORTED]
        assert rc(facts=ALL & ~PAR16) == EINVAL
        assert rc(facts=ALL & ~OUT_I32) == (EINVAL if io == F32 else 0) and rc(facts=ALL & ~OUT_I32, hd=128) == 0
    # then the alignment each entry asks for, and no more than that
    assert rc(facts=ALL & ~IN16) == (EINVAL if need_in == 16 else 0)
    assert rc(facts=ALL & ~IN16 & ~IN8) == (EINVAL if need_in else 0)
    assert rc(facts=ALL & ~OUT16) == (EINVAL if need_out == 16 else 0)
    assert rc(facts=ALL & ~OUT16 & ~OUT8) == (EINVAL if need_out else 0)


def test_plan_entry_never_crashes_on_nonsense():
    L = _lib.lib()
    big = 2 ** 31 - 1
    for entry in range(-1, 9):
        for io in (-1, 0, 1, 2):
            for ext in (0, -1, 1, big):
                for hd in (64, 128, 8, 0, big):
                    rc = L.hig_attn_plan(entry, io, ext, ext, ext, ext, hd, 1, ALL, 256, 1, None, None, None)
                    path, split = C.c_int32(-7), C.c_int32(-7)
                    assert L.hig_attn_plan(entry, io, ext, ext, ext, ext, hd, 1, ALL, 256, 1, C.byref(path), C.byref(split), None) == rc
                    if not (0 <= entry < len(ENTRIES) and io in (0, 1)) or ext <= 0:
                        assert rc == EINVAL and (path.value, split.value) == (-1, 0)
                    if rc == 0:
                        assert 0 <= path.value < len(PATHS) and split.value >= 1


def parity_points():
    with open(os.path.join(ROOT, "tests", "golden", "attn_dispatch_parity.json")) as f:
        table = json.load(f)
    return table["fields"], table["points"]


def test_plan_reproduces_the_dispatch_of_the_entry_points_it_replaced():
    fields, points = parity_points()
    assert len(points) >= 300
    wrong, seen = [], set()
    for row in points:
        p = dict(zip(fields, row))
        rc, path, split, _ = plan(p["entry"], p["io"], p["B"], p["rows"], p["H"], p["hd"], Tk=p["Tk"],
                                  scratch=p["scratch"], facts=p["facts"], chip_cus=256, big_lds_ok=1)
        want = (0, p["path"], p["split"]) if p["rc"] == 0 else (p["rc"], None, 0)
        if (rc, path, split) != want:
            wrong.append((row, (rc, path, split)))
        seen.add(p["path"] if p["rc"] == 0 else p["rc"])
    assert not wrong, "%d of %d calls planned differently from what the parent library did: %s" % (len(wrong), len(points), wrong[:5])
    assert seen >= set(PATHS) | {EINVAL, EUNSUPPORTED}, "the record must cover all 16 paths and both refusal codes"
