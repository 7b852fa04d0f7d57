"""hig_fullattn_bwd_kpad: the full-attention backward under torch's key-padding mask, per element.

The contract and its bounds are those of tests/test_gpu_attn_contract.py (`full_reference(..., kpad=...)`, `full_bounds`),
which until now ran only the forward with a mask.  Here the backward is fed the forward's own y / lse from
hig_fullattn_fwd_kpad and held to the same per-element bounds on dQ, dK and dV, on all four kernels (VALU head dim 8 / 16 /
32, matrix cores head dim 64 / 128), with the five masks of `kpad_masks` plus one shaped like the evaluator's: [cls], then two
blocks with a padded tail.  A padded key's probability is exactly 0: its dK / dV rows are exact zeros.  Outputs are NaN-filled
and guarded, two calls give equal bits, the path counter and split are the plan's, and with kpad = NULL the entry point is
hig_fullattn_bwd bit for bit.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_attn_contract as AC  # noqa: E402  (helpers only: nothing of it is collected from here)
from hig_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

DEV, F32, P = AC.DEV, torch.float32, AC.P


def evaluator_mask(Tk):
    """(1, Tk): [cls] when Tk is odd, then two blocks of (Tk - cls) / 2 tokens, the last 40 % of each padded."""
    cls = Tk % 2
    T = (Tk - cls) // 2
    keep = max(1, (3 * T) // 5)
    m = torch.zeros(1, Tk, dtype=torch.uint8)
    for p in range(2):
        m[0, cls + p * T + keep:cls + (p + 1) * T] = 1
    return m


def forward(q, kv, B, Tq, Tk, H, hd, lg, kp):
    d = H * hd
    y, lse = torch.empty(B * Tq, d, device=DEV), torch.empty(B * H, Tq, device=DEV)
    _lib.check(AC.lib().hig_fullattn_fwd_kpad(P(q), d, P(kv), P(kv, d), 2 * d, B, Tq, Tk, H, hd, P(lg), P(kp), P(y), d, P(lse),
                                              _lib.stream_ptr()))
    return y, lse


def backward(entry, dy, y, q, kv, B, Tq, Tk, H, hd, lg, lse, kp, bwd_path):
    """One guarded call of hig_fullattn_bwd (`entry` "plain") or hig_fullattn_bwd_kpad -> (dQ, dK, dV)."""
    d, L = H * hd, AC.lib()
    dq, dk, dv = AC.Guarded(B * Tq, d), AC.Guarded(B * Tk, d), AC.Guarded(B * Tk, d)
    delta = torch.zeros(B * H * Tq, device=DEV)
    args = (P(dy), d, P(y), d, P(q), d, P(kv), P(kv, d), 2 * d, B, Tq, Tk, H, hd, P(lg), P(lse), P(delta), dq.ptr(), dq.ld,
            dk.ptr(), dv.ptr(), dk.ld)
    before = AC.counts()
    if entry == "plain":
        _lib.check(L.hig_fullattn_bwd(*args, _lib.stream_ptr()))
    else:
        _lib.check(L.hig_fullattn_bwd_kpad(*args, P(kp), _lib.stream_ptr()))
    torch.cuda.synchronize()
    moved = {n: a - b for n, a, b in zip(AC.PATHS, AC.counts(), before) if a != b}
    assert moved == {bwd_path: 1}, moved
    assert (bwd_path, L.hig_attn_last_split()) == AC.planned("full_bwd", F32, B, Tq, H, hd, Tk), "the call did not do what its plan named"
    return dq.verify("dQ"), dk.verify("dK"), dv.verify("dV")


SHAPES = [
    # (hd, H, Tq, Tk, qlens)
    (8, 3, 31, 33, None), (16, 5, 65, 65, None), (32, 4, 150, 150, (150, 149, 1, 0, 75, 90)),                 # VALU
    (64, 8, 183, 183, (183, 77, 1, 0, 182, 92)), (64, 4, 33, 65, None), (64, 8, 300, 65, None),                 # matrix cores
    (128, 2, 33, 300, None), (128, 4, 150, 150, None),
]


@pytest.mark.parametrize("hd,H,Tq,Tk,qlens", SHAPES)
def test_backward_under_a_key_padding_mask(hd, H, Tq, Tk, qlens):
    B, d = 6, H * hd
    kpad = torch.cat([AC.kpad_masks(5, Tk), evaluator_mask(Tk)])
    assert kpad.shape == (B, Tk) and (kpad.sum(1) < Tk).all()         # (all keys padded: outside the contract)
    q_h, kv_h, dy_h = AC.full_inputs(B, Tq, Tk, H, hd, seed=11 + hd)
    q, kv, kp = q_h.to(DEV), kv_h.to(DEV), kpad.to(DEV)
    lg = None if qlens is None else torch.tensor(qlens, dtype=torch.int64, device=DEV)
    valid_h = torch.ones(B, Tq, dtype=torch.bool) if qlens is None else torch.arange(Tq)[None] < torch.tensor(qlens)[:, None]
    dy = (dy_h * valid_h.reshape(-1, 1)).to(DEV)                       # rows at or beyond qlen take no gradient
    y, lse = forward(q, kv, B, Tq, Tk, H, hd, lg, kp)
    r = AC.full_reference(q, kv, dy, B, Tq, Tk, H, hd, lg, kp, lse_in=lse, y_in=y)
    assert r["X"][r["valid"][:, None, :].expand_as(r["X"])].max().item() <= 80 + math.log(Tk), "logit spread above 80"
    b = AC.full_bounds(r, B, Tq, Tk, H, hd)
    bwd_path = AC.paths_for(hd)[1]
    outs = [backward("kpad", dy, y, q, kv, B, Tq, Tk, H, hd, lg, lse, kp, bwd_path) for _ in range(2)]
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_), "two backward calls differ"
    dq, dk, dv = outs[0]
    report = ["kpad bwd B=%d Tq=%d Tk=%d H=%d hd=%d -> %s:" % (B, Tq, Tk, H, hd, bwd_path)]
    gb = b["g_wb"] + 2 * hd + 3 + max(Tq, Tk) + 2
    AC.held("dQ", dq.reshape(B, Tq, H, hd), r["dQ"], b["dQ"], report, b["MdQ"], gb)
    AC.held("dK", dk.reshape(B, Tk, H, hd), r["dK"], b["dK"], report, b["MdK"], gb)
    AC.held("dV", dv.reshape(B, Tk, H, hd), r["dV"], b["dV"], report, b["MdV"], gb)
    print(" ".join(report))
    padded = kp.bool()
    assert (dk.reshape(B, Tk, d)[padded] == 0).all() and (dv.reshape(B, Tk, d)[padded] == 0).all(), "a padded key's dK / dV rows are exact zeros"
    assert (dq.reshape(B, Tq, d)[~r["valid"]] == 0).all(), "query rows at or beyond qlen with dy = 0: dQ = 0"
    # a key that is padded has no say: its K / V rows may hold anything finite
    kv2 = kv.clone()
    kv2.view(B, Tk, 2 * d)[padded] = 7.5
    for a, b_ in zip(outs[0], backward("kpad", dy, y, q, kv2, B, Tq, Tk, H, hd, lg, lse, kp, bwd_path)):
        assert torch.equal(a, b_), "the K / V rows of a padded key reached the result"


@pytest.mark.parametrize("hd,H,B,Tq,Tk,qlens", [(64, 8, 4, 196, 196, (0, 1, 195, 196)), (32, 4, 4, 129, 129, (0, 1, 128, 129))])
def test_without_a_mask_it_is_the_unmasked_backward_bit_for_bit(hd, H, B, Tq, Tk, qlens):
    q_h, kv_h, dy_h = AC.full_inputs(B, Tq, Tk, H, hd, seed=Tq + Tk + hd)
    q, kv = q_h.to(DEV), kv_h.to(DEV)
    lg = torch.tensor(qlens, dtype=torch.int64, device=DEV)
    dy = (dy_h * (torch.arange(Tq)[None] < torch.tensor(qlens)[:, None]).reshape(-1, 1)).to(DEV)
    y, lse = forward(q, kv, B, Tq, Tk, H, hd, lg, None)
    bwd_path = AC.paths_for(hd)[1]
    plain = backward("plain", dy, y, q, kv, B, Tq, Tk, H, hd, lg, lse, None, bwd_path)
    null = backward("kpad", dy, y, q, kv, B, Tq, Tk, H, hd, lg, lse, None, bwd_path)
    zeros = backward("kpad", dy, y, q, kv, B, Tq, Tk, H, hd, lg, lse, torch.zeros(B, Tk, dtype=torch.uint8, device=DEV), bwd_path)
    for name, a, b_, c in zip(("dQ", "dK", "dV"), plain, null, zeros):
        assert torch.equal(a, b_), "%s: kpad = NULL differs from hig_fullattn_bwd" % name
        assert torch.equal(a, c), "%s: an all-zero mask differs from no mask" % name
