"""Which kernel serves a GEMM call, asked of the plan entries (hig_gemm_bf16_plan / hig_gemm_plan, csrc/gemm_plan.hip) without a
GPU: they are pure functions of the descriptor, the switches and the CU count, and never dereference an operand, so made-up
aligned addresses and chip_cus = 256 stand in for an MI355X.  tests/test_gpu_gemm_contract.py asserts on the device that a
call moves exactly the launch counters its plan named; a dispatch regression therefore fails here first.

  - the dispatch table and the unserved cases of tests/gemm_dispatch_cases.py (shared with the GPU suite);
  - on a chip that is not 8 XCDs x 32 CUs (chip_cus = 128) every weight-stationary case falls to a tiled / few-row kernel;
  - the LayerNorm-fold eligibility of the bf16 forward IS "every launch of the fold plans onto WSP16 / WS16";
  - tests/golden/gemm_dispatch_parity.json: 877 calls of hig_gemm_bf16 / hig_gemm / hig_gemm_ws answered by the library as
    it was BEFORE the plan existed (the chain of `_try` functions), each with the launch counters it moved or the error code
    it returned, recorded on an MI355X.  The plan reproduces every one."""
import json
import os

import pytest

from hig_amd import _lib  # noqa: E402
from gemm_dispatch_cases import BIAS, BIAS_RES, DISPATCH, UNSERVED, dispatch_uses_aux, fake_desc, plan  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHT_STATIONARY = {"WSP16", "WS16", "WSP32"}
FALLBACK = {"TILED16", "FEWROW16", "TILED32", "TAIL32"}


def case_desc(entry, I, J, K, epi, c_f32, res_f32, ldc, expect):
    return fake_desc(entry, I, J, K, epi, c_f32=c_f32, res_f32=res_f32, ldc=ldc, aux=dispatch_uses_aux(entry, epi, expect))


@pytest.mark.parametrize("entry,I,J,K,epi,c_f32,res_f32,ldc,expect", DISPATCH)
def test_dispatch_table_is_planned(entry, I, J, K, epi, c_f32, res_f32, ldc, expect):
    rc, moved, _ = plan(entry, case_desc(entry, I, J, K, epi, c_f32, res_f32, ldc, expect), chip_cus=256)
    assert (rc, moved) == (0, expect)


@pytest.mark.parametrize("entry,I,J,K,epi,c_f32,res_f32,ldc,expect", [c for c in DISPATCH if set(c[-1]) & WEIGHT_STATIONARY])
def test_another_chip_geometry_gets_the_tiled_kernels(entry, I, J, K, epi, c_f32, res_f32, ldc, expect):
    """The weight-stationary kernels' work split is compiled for 8 XCDs x 32 CUs.  (Without the bf16 `aux`: only gemm_wsp16
    writes it, so with it such a chip gets an error -- asserted too.)"""
    rc, moved, _ = plan(entry, fake_desc(entry, I, J, K, epi, c_f32=c_f32, res_f32=res_f32, ldc=ldc, aux=entry != "bf16" and dispatch_uses_aux(entry, epi, expect)), chip_cus=128)
    assert rc == 0 and len(moved) == 1 and set(moved) <= FALLBACK and list(moved.values()) == [1], (rc, moved)
    if entry == "bf16" and dispatch_uses_aux(entry, epi, expect):
        assert plan(entry, case_desc(entry, I, J, K, epi, c_f32, res_f32, ldc, expect), chip_cus=128)[:2] == (-3, {})


@pytest.mark.parametrize("entry,I,J,K,epi,operand", UNSERVED)
def test_unserved_fold_and_aux_operands_are_refused(entry, I, J, K, epi, operand):
    d = fake_desc(entry, I, J, K, epi, aux=operand == "aux", fold="out" if operand == "stats_out" else "")
    assert plan(entry, d, chip_cus=256)[:2] == (-3, {})


def test_variant_codes():
    """The instance inside the kernel (include/hig.h, next to the plan entries)."""
    def variant(*a, **k):
        rc, _, v = plan(a[0], fake_desc(*a, **k), chip_cus=256)
        assert rc == 0
        return v
    assert variant("bf16", 2048, 512, 512, BIAS) == 0
    assert variant("bf16", 2048, 512, 512, _lib.EPI_BIAS_GELU, aux=True) == 4
    assert variant("bf16", 2048, 512, 512, BIAS_RES, fold="out") == 1 and variant("bf16", 2048, 1536, 512, BIAS, fold="in") == 2
    assert variant("bf16", 12544, 1536, 256, BIAS) == 8 and variant("bf16", 12544, 1024, 256, _lib.EPI_BIAS_GELU) == 44
    assert variant("bf16", 12544, 1024, 1024, BIAS_RES, fold="out") == 4 + 256 and variant("bf16", 12544, 3072, 1024, BIAS, fold="in") == 4 + 512
    assert variant("bf16", 6272, 512, 1536, BIAS) == 64643 and variant("bf16", 12544, 512, 1536, BIAS) == 128324
    assert variant("f32", 2048, 512, 1536, BIAS_RES) == 0 and variant("f32", 2048, 512, 512, BIAS, fold="in") == 2
    assert variant("ws", 2047, 576, 768, BIAS_RES) == 3 + 16 * 8 and variant("f32", 2047, 576, 768, BIAS_RES) == 3 + 16


@pytest.mark.parametrize("d", [256, 512, 1024])
def test_lnfold_eligibility_is_the_plan_of_its_launches(d):
    """hig_gemm_ws16_lnfold_ok (reached through hig_gemm_bf16_lnfold_plan) == every launch of the fold lands on a kernel that
    implements it: the producer (d x d, EPI_BIAS_RES, row_stats_out) and the consumers (J = 3 d and J = d, EPI_BIAS, row_stats_in +
    ln_colsum).  Rows around the row threshold and around the 2^30-element limit of the widest consumer's output."""
    lim = 2 ** 30 // (3 * d)                   # rows x 3 d bf16 elements = 2^31 bytes: the offset limit of the widest consumer
    half = 2 ** 30 // (3 * 2 * d)              # ... = 2^30 bytes
    seen = set()
    for cus in (256, 128):
        for rows in (2047, 2048, 12544, half - 1, half, half + 1, lim - 1, lim, lim + 1):
            launches = [fake_desc("bf16", rows, d, d, BIAS_RES, fold="out"), fake_desc("bf16", rows, 3 * d, d, BIAS, fold="in"),
                        fake_desc("bf16", rows, d, d, BIAS, fold="in")]
            plans = [plan("bf16", g, chip_cus=cus) for g in launches]
            want = all(rc == 0 and set(moved) <= {"WSP16", "WS16"} and moved for rc, moved, _ in plans)
            assert bool(_lib.lib().hig_gemm_bf16_lnfold_plan(rows, d, cus)) == want, (rows, d, cus, plans)
            seen.add((cus, want))
    assert seen == ({(256, False), (128, False)} if d == 256 else {(256, True), (256, False), (128, False)})


def parity_points():
    with open(os.path.join(ROOT, "tests", "golden", "gemm_dispatch_parity.json")) as f:
        table = json.load(f)
    return table["fields"], table["points"]


def test_plan_reproduces_the_dispatch_of_the_try_chain_it_replaced():
    fields, points = parity_points()
    assert len(points) >= 300
    wrong = []
    for row in points:
        p, result = dict(zip(fields, row[:-1])), row[-1]
        entry = p.pop("entry")
        rc, moved, _ = plan(entry, fake_desc(entry, p.pop("I"), p.pop("J"), p.pop("K"), p.pop("epi"), **p), chip_cus=256)
        got = moved if rc == 0 else rc
        if got != result:
            wrong.append((entry, row, got))
    assert not wrong, "%d of %d calls planned differently from what the parent library did: %s" % (len(wrong), len(points), wrong[:5])
    served = set()
    for row in points:
        served |= set(row[-1]) if isinstance(row[-1], dict) else {row[-1]}
    assert served >= {"TILED32", "WSP32", "TAIL32", "WSP16", "WS16", "FEWROW16", "TILED16", -3}
