"""The per-timestep loss weights on the MI355X: hig_masked_mse_w, hig_pair_mse_w and hig_loss_history_update held to the bounds of
tests/loss_weight_bounds.py inside guarded buffers, and the training routes end to end on the oracle's `tiny` / `tiny2` cases.

The entries.  pred and target hold NaN wherever the contract says nothing may contribute and start 4 bytes off a 16-byte
boundary; every output lies between guard bands; with a table of ones the weighted instance returns the bits of hig_masked_mse /
hig_pair_mse; the PIT decisions are the unweighted kernel's; two calls give the same bits.  The history kernel is run batch by
batch beside the host mirror: counts equal, the history bit for bit the fp32-rounded pushes, p and w within their bounds (and
exactly 1 / N and base_w until the launch in which the last ring fills), sum p = 1 within N u, and the recorded sequence of golden
g23 reproduced.

End to end.  The fused step under min-SNR against the autograd route and against an fp64 restatement of three steps (the
oracle's denoiser in double, the weighted loss, clip_grad_norm_ and torch Adam), gated as the project gates whole routes: rel-L2
over all trainable parameters <= max(1e-6, 4 x the distance of the same restatement in fp32 on the CPU).  With a table of ones
forced through the weighted route the step is the unweighted step bit for bit; the captured step is the fused step bit for bit
under min-SNR + loss-aware sampling, history and tables included, for PIT, labelled and bf16 storage (on `tiny` at two heads of
64, the smallest head the bf16 kernels take); a checkpoint written
mid-run resumes to the uninterrupted run's bits; with both options unset no new entry is ever called.

The `RATIO` and `GATE` lines (`pytest -s`) are what README.md's table was collected from.
"""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hig_amd  # noqa: E402
from hig_amd import _lib  # noqa: E402
from hig_amd.models.gaussian_diffusion import DeviceLossSecondMomentResampler, min_snr_weights  # noqa: E402
from oracle import denoiser_ref as DR  # noqa: E402
from oracle import fill  # noqa: E402
from test_gpu_rowops_contract import Buf, P, S, lib, ok  # noqa: E402
from test_gpu_boundary_contract import held, bits  # noqa: E402
import test_gpu_interaction as TI  # noqa: E402
import boundary_bounds as bb  # noqa: E402
import loss_weight_bounds as lw  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_loss_sampler.npz")
NB = _lib.NORM_BLOCKS


def off16(t):
    """t on the device, its first element 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    lead = (-(buf.data_ptr() // t.element_size()) % (16 // t.element_size()) + 1) % (16 // t.element_size())
    out = buf[lead:lead + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 or t.element_size() != 4
    return out


def same(a, b):
    return torch.equal(bits(a), bits(b))


# ----------------------------------------------------------------------------------------------------------------------
# hig_masked_mse_w
# ----------------------------------------------------------------------------------------------------------------------
def masked_call(pd, tg, ln, td, wd, B, T, F, want_sl=True, want_d=True, what="hig_masked_mse_w"):
    lo, d, sl = Buf.flat(1), Buf.flat(B * T * F), Buf.flat(B)
    scratch = Buf.flat(NB + (B * T if want_sl else 0))
    ok(lib().hig_masked_mse_w(P(pd), P(tg), P(ln), P(td), P(wd), wd.numel(), B, T, F, lo.p(), d.p() if want_d else None,
                              sl.p() if want_sl else None, scratch.p(), S()))
    scratch.guards(what + " scratch")
    loss = lo.written(what + " loss")[0]
    dp = d.written(what + " dpred").view(B, T, F) if want_d else d.untouched(what + " dpred = NULL")
    s = sl.written(what + " sample_loss") .view(B) if want_sl else sl.untouched(what + " sample_loss = NULL")
    return loss, dp, s


@pytest.mark.parametrize("with_len", (True, False))
@pytest.mark.parametrize("B,T,F", lw.MASKED_SHAPES)
def test_masked_mse_w(B, T, F, with_len):
    pred, target, length, t, wtab = lw.masked_case(B, T, F, with_len)
    b = lw.masked_w_bound(pred, target, length, t, wtab)
    pn, tn = lw.masked_poison(pred, target, length)
    pd, tg, td, wd = off16(pn), off16(tn), t.to(DEV), off16(wtab)
    ln = None if length is None else length.to(DEV)
    what = "hig_masked_mse_w %dx%dx%d%s" % (B, T, F, "" if with_len else "_nolen")
    loss, dp, sl = masked_call(pd, tg, ln, td, wd, B, T, F, what=what)
    assert torch.isfinite(loss).all() and torch.isfinite(sl).all(), "%s: a masked position was read" % what
    held(what.replace(" ", ".loss ", 1), loss, *b["loss"])
    held(what.replace(" ", ".dpred ", 1), dp, *b["dpred"])
    held(what.replace(" ", ".sample_loss ", 1), sl, *b["sample_loss"])
    L = torch.full((B,), T, dtype=torch.int64) if length is None else length
    off = ~(torch.arange(T)[None] < L[:, None])
    assert (dp[off] == 0).all(), "%s: dpred is not exactly 0 off the mask" % what
    loss2, dp2, sl2 = masked_call(pd, tg, ln, td, wd, B, T, F, what=what)
    assert same(loss, loss2) and same(dp, dp2) and same(sl, sl2), "%s: two calls differ" % what
    loss3, dp3, _ = masked_call(pd, tg, ln, td, wd, B, T, F, want_sl=False, what=what)
    assert same(loss, loss3) and same(dp, dp3), "%s: sample_loss = NULL changes the loss" % what
    loss4, _, sl4 = masked_call(pd, tg, ln, td, wd, B, T, F, want_d=False, what=what)
    assert same(loss, loss4) and same(sl, sl4), "%s: dpred = NULL changes the loss" % what
    # a table of ones: the unweighted entry's bits
    ones = torch.ones(lw.NSTEPS, device=DEV)
    loss1, dp1, sl1 = masked_call(pd, tg, ln, td, ones, B, T, F, what=what + " w=1")
    lo, d, scratch = Buf.flat(1), Buf.flat(B * T * F), Buf.flat(NB)
    ok(lib().hig_masked_mse(P(pd), P(tg), P(ln), B, T, F, lo.p(), d.p(), scratch.p(), S()))
    scratch.guards(what + " unweighted scratch")
    assert same(loss1, lo.written(what)[0]) and same(dp1, d.written(what).view(B, T, F)), "%s: w = 1 is not hig_masked_mse" % what
    assert same(sl1, sl), "%s: the per-sample losses depend on the table" % what


# ----------------------------------------------------------------------------------------------------------------------
# hig_pair_mse_w
# ----------------------------------------------------------------------------------------------------------------------
def pair_call(pd, tg, ln, td, wd, R, T, F, pit, want_sl=True, what="hig_pair_mse_w"):
    n = R // 4 if pit else R
    lo, d, sl, scratch = Buf.flat(1), Buf.flat(R * T * F), Buf.flat(n), Buf.flat(2 * R)
    ok(lib().hig_pair_mse_w(P(pd), P(tg), P(ln), P(td), P(wd), wd.numel(), R, T, F, pit, lo.p(), d.p(),
                            sl.p() if want_sl else None, scratch.p(), S()))
    s = sl.written(what + " sample_loss").view(n) if want_sl else sl.untouched(what + " sample_loss = NULL")
    return lo.written(what + " loss")[0], d.written(what + " dpred").view(R, T, F), s, scratch.written(what + " scratch")[0]


@pytest.mark.parametrize("R,T,F,pit,with_len", lw.PAIR_W_SHAPES)
def test_pair_mse_w(R, T, F, pit, with_len):
    pred, target, length, t, wtab = lw.pair_w_case(R, T, F, pit, with_len)
    b = lw.pair_w_bound(pred, target, length, pit, t, wtab)
    pn, tn = bb.pair_poison(pred, target, length)
    pd, tg, td, wd = off16(pn), off16(tn), t.to(DEV), off16(wtab)
    ln = None if length is None else length.to(DEV)
    what = "hig_pair_mse_w %dx%dx%d%s%s" % (R, T, F, "_pit" * pit, "" if with_len else "_nolen")
    loss, dp, sl, sc = pair_call(pd, tg, ln, td, wd, R, T, F, pit, what=what)
    assert torch.isfinite(loss).all() and torch.isfinite(sl).all(), "%s: a masked position was read" % what
    held(what.replace(" ", ".rowloss ", 1), sc[:R], *b["rowloss"])
    rowscale = sc[R:]
    bad = (bits(rowscale) != bits(b["rowscale32"])).nonzero().flatten().tolist()
    assert not bad, "%s: rowscale of rows %s is not fp32(w fp32(1 / denom)) on the chosen rows and 0 elsewhere" % (what, bad[:8])
    held(what.replace(" ", ".loss ", 1), loss, *b["loss"])
    held(what.replace(" ", ".dpred ", 1), dp, *b["dpred"])
    held(what.replace(" ", ".sample_loss ", 1), sl, *b["sample_loss"])
    dead = ~b["live"] | (b["rowscale32"] == 0)[:, None, None]
    assert (dp[dead] == 0).all(), "%s: dpred is not exactly 0 off the mask / on an unchosen row" % what
    loss2, dp2, sl2, sc2 = pair_call(pd, tg, ln, td, wd, R, T, F, pit, what=what)
    assert same(loss, loss2) and same(dp, dp2) and same(sl, sl2) and same(sc, sc2), "%s: two calls differ" % what
    loss3, dp3, _, sc3 = pair_call(pd, tg, ln, td, wd, R, T, F, pit, want_sl=False, what=what)
    assert same(loss, loss3) and same(dp, dp3) and same(sc, sc3), "%s: sample_loss = NULL changes the loss" % what
    # a table of ones: the unweighted entry's bits, and its PIT decisions under any table
    ones = torch.ones(lw.NSTEPS, device=DEV)
    loss1, dp1, sl1, sc1 = pair_call(pd, tg, ln, td, ones, R, T, F, pit, what=what + " w=1")
    lo, d, scratch = Buf.flat(1), Buf.flat(R * T * F), Buf.flat(2 * R)
    ok(lib().hig_pair_mse(P(pd), P(tg), P(ln), R, T, F, pit, lo.p(), d.p(), scratch.p(), S()))
    usc = scratch.written(what)[0]
    assert same(loss1, lo.written(what)[0]) and same(dp1, d.written(what).view(R, T, F)) and same(sc1, usc), \
        "%s: w = 1 is not hig_pair_mse" % what
    assert same(sl1, sl), "%s: the per-sample losses depend on the table" % what
    if pit:
        Pn = R // 4
        first = rowscale[:Pn] != 0
        assert torch.equal(first, usc[R:R + Pn] != 0), "%s: the weights move a PIT decision" % what
        assert torch.equal(first, b["first"]) and first[b["tie"]].all(), "%s: not the reference's assignment" % what


# ----------------------------------------------------------------------------------------------------------------------
# hig_loss_history_update
# ----------------------------------------------------------------------------------------------------------------------
class State:
    """hist, counts, p and w of one history inside one sentinel-filled allocation each: the 16 elements on either side of a
    payload must keep their bits."""
    FPAT, IPAT = -7.25e30, 0x5A5A5A5A

    def __init__(self, nsteps, H, base_w, u=0.001):
        self.N, self.H, self.u = nsteps, H, u
        self.base = torch.as_tensor(base_w, dtype=torch.float32).to(DEV)
        self.bufs = {}
        for name, n, dt, pat, init in (("hist", nsteps * H, torch.float32, self.FPAT, 0.0), ("counts", nsteps, torch.int32, self.IPAT, 0),
                                       ("p", nsteps, torch.float32, self.FPAT, float("nan")), ("w", nsteps, torch.float32, self.FPAT, float("nan"))):
            buf = torch.full((n + 32,), pat, dtype=dt, device=DEV)
            buf[16:16 + n] = init
            self.bufs[name] = (buf, n, pat)

    def view(self, name):
        buf, n, _ = self.bufs[name]
        return buf[16:16 + n]

    def update(self, ts, losses):
        t = None if ts is None else torch.as_tensor(ts, dtype=torch.int64).to(DEV)
        sl = None if losses is None else torch.as_tensor(losses, dtype=torch.float32).to(DEV)
        ok(lib().hig_loss_history_update(P(t), P(sl), 0 if t is None else t.numel(), P(self.view("hist")), P(self.view("counts")),
                                         P(self.base), self.N, self.H, self.u, P(self.view("p")), P(self.view("w")), S()))
        for name, (buf, n, pat) in self.bufs.items():
            assert (buf[:16] == pat).all() and (buf[16 + n:] == pat).all(), "hig_loss_history_update wrote outside %s" % name
        return (self.view("hist").view(self.N, self.H).cpu().numpy(), self.view("counts").cpu().numpy(),
                self.view("p").cpu().numpy(), self.view("w").cpu().numpy())


def check_against_mirror(what, got, mirror):
    hist, counts, p, w = got
    assert np.array_equal(counts, mirror.counts), "%s: counts" % what
    assert np.array_equal(hist.view(np.int32), mirror.hist.astype(np.float32).view(np.int32)), "%s: the history is not the fp32 pushes" % what
    (pr, b_p), (wr, b_w), exact = lw.refresh_bound(mirror)
    if exact:
        assert np.array_equal(p, pr.astype(np.float32)) and np.array_equal(w.view(np.int32), mirror.base.astype(np.float32).view(np.int32)), \
            "%s: not warmed up, but p != 1 / N or w != base_w" % what
    else:
        for name, out, ref, bound in (("p", p, pr, b_p), ("w", w, wr, b_w)):
            q = np.abs(out.astype(np.float64) - ref) / bound
            print("RATIO %s.%s %.3f" % (what, name, q.max()))
            assert q.max() <= 1.0, "%s.%s: largest |err| / bound = %.3f at %d" % (what, name, q.max(), q.argmax())
        assert abs(p.astype(np.float64).sum() - 1.0) <= mirror.N * lw.U, "%s: sum p = 1 + %.3g" % (what, p.astype(np.float64).sum() - 1)
    return exact


@pytest.mark.parametrize("nsteps,H", lw.HISTORY_SHAPES)
def test_loss_history_follows_the_mirror(nsteps, H):
    seq = lw.history_sequence(nsteps, H)
    base = lw.weight_table(nsteps).numpy()
    st, mirror = State(nsteps, H, base), lw.HistoryMirror(nsteps, H, base_w=base)
    what = "hig_loss_history_update N%d_H%d" % (nsteps, H)
    got = st.update(None, None)                                   # the refresh alone, on an empty history
    assert check_against_mirror(what + " empty", got, mirror)
    for i, (ts, losses) in enumerate(seq):
        mirror.update(ts, losses)
        exact = check_against_mirror("%s batch %d" % (what, i), st.update(ts, losses), mirror)
        assert exact == (i < len(seq) - 1), "%s: warmed up at batch %d of %d" % (what, i, len(seq))
    again = st.update(None, None)                                 # n = 0 pushes nothing and gives the same tables
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(again, st.update(None, None)))
    check_against_mirror(what + " refresh", again, mirror)


def test_loss_history_shifts_inside_one_launch_and_skips_what_it_must():
    """Four entries under one timestep at H = 2: the ring keeps the last two, in batch order.  Out-of-range timesteps, NaN and
    +-inf losses, and a product that overflows change nothing."""
    st, mirror = State(3, 2, [1.0, 2.0, 3e38]), lw.HistoryMirror(3, 2, base_w=[1.0, 2.0, 3e38])
    ts, losses = [1, 1, 1, 1], [1.0, 2.0, 3.0, 4.0]
    hist, counts, _, _ = st.update(ts, losses)
    mirror.update(ts, losses)
    assert hist[1].tolist() == [6.0, 8.0] and counts.tolist() == [0, 2, 0]
    junk_t, junk_l = [-1, 3, 2 ** 40, 0, 0, 0, 2], [1.0, 1.0, 1.0, float("nan"), float("inf"), float("-inf"), 10.0]
    got = st.update(junk_t, junk_l)
    mirror.update(junk_t, junk_l)
    assert mirror.pushes == 4 and got[1].tolist() == [0, 2, 0]
    check_against_mirror("skips", got, mirror)
    ts, losses = [0, 2, 0, 2], [0.5, 1e-30, 0.25, 2e-30]
    mirror.update(ts, losses)
    assert not check_against_mirror("filled", st.update(ts, losses), mirror)


def test_loss_history_reproduces_the_reference_sequence():
    """Golden g23 (the reference's own sampler, float64) through the kernel: counts exact, the history its fp32 rounding, and
    weights() before and after warm-up within the refresh bound of the fp32 history plus the rounding of the pushes."""
    g = np.load(GOLDEN)
    N, H, u = int(g["nsteps"]), int(g["history_per_term"]), float(g["uniform_prob"])
    st, mirror = State(N, H, np.ones(N), u), lw.HistoryMirror(N, H, uniform_prob=u)
    for i, n in enumerate(g["n"].tolist()):
        ts, losses = g["ts"][i, :n], g["losses"][i, :n]
        got = st.update(ts, losses)
        mirror.update(ts, losses)
        exact = check_against_mirror("g23 call %d" % i, got, mirror)
        assert exact == (not bool(g["warmed_up"][i]))
        assert np.array_equal(got[1], g["counts"][i]) and np.array_equal(got[0], g["history"][i].astype(np.float32))
        ref = g["weights"][i] / g["weights"][i].sum()
        # the fp32 history is within u of the float64 one per entry: m_t, the total and the quotient move by at most 3 u
        (_, b_p), _, _ = lw.refresh_bound(mirror)
        assert (np.abs(got[2].astype(np.float64) - ref) <= b_p + 3 * lw.U * ref).all(), "g23 call %d: p" % i


def test_device_sampler_draws_on_the_device_and_round_trips_its_state():
    smp = DeviceLossSecondMomentResampler(7, DEV, history_per_term=3)
    assert same(smp.p.cpu(), torch.full((7,), 1.0).float() / torch.tensor(7.0)) and same(smp.w.cpu(), torch.ones(7))
    g = np.load(GOLDEN)
    for i, n in enumerate(g["n"].tolist()):
        smp.update(torch.as_tensor(g["ts"][i, :n]).to(DEV), torch.as_tensor(g["losses"][i, :n], dtype=torch.float32).to(DEV))
    assert np.array_equal(smp.counts.cpu().numpy(), g["counts"][-1])
    torch.manual_seed(3)
    t, w = smp.sample(4096)
    assert t.is_cuda and t.dtype == torch.int64 and t.shape == (4096,) and same(w.cpu(), smp.w[t].cpu())
    freq = torch.bincount(t, minlength=7).double().cpu() / 4096
    assert (freq - smp.p.double().cpu()).abs().max() < 0.04, "the draw does not follow p: %s against %s" % (freq, smp.p)
    other = DeviceLossSecondMomentResampler(7, DEV, history_per_term=3)
    other.load_state_dict(smp.state_dict())
    assert all(same(a.cpu(), b.cpu()) for a, b in zip(smp.tensors(), other.tensors()))
    with pytest.raises(ValueError):
        other.load_state_dict(DeviceLossSecondMomentResampler(7, DEV, history_per_term=4).state_dict())


# ----------------------------------------------------------------------------------------------------------------------
# end to end: the training routes
# ----------------------------------------------------------------------------------------------------------------------
TINY, TINY2 = fill.CASES["tiny"], fill.ICASES["tiny2"]
# bf16 storage needs a head dim of 64 or 128, which `tiny` (64 / 8) has not: the same case at two heads of 64
TINY16 = dict(TINY, d=128, H=2)
# t per step: low-noise steps, where the min-SNR weights are far from 1, beside high-noise ones
STEP_T = ((3, 987), (40, 500), (0, 120), (700, 15), (999, 8))


def build1(storage=None):
    c = TINY if storage is None else TINY16
    kw = {} if storage is None else dict(storage=storage)
    m = hig_amd.MotionTransformer(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"],
                                  num_layers=c["L"], num_heads=c["H"], text_latent_dim=c["Lt"], **kw)
    m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    return m.to(DEV).train()


def opts(c, **extra):
    return dict(device=torch.device(DEV), diffusion_steps=1000, is_train=True, lr=2e-4, batch_size=c["B"], num_epochs=1,
                log_every=50, save_latest=500, save_every_e=5, is_continue=False, model_dir="/tmp", **extra)


def trainer1(m, **extra):
    return hig_amd.DDPMTrainer(types.SimpleNamespace(**opts(TINY, **extra)), m)


def trainer2(m, label, **extra):
    return hig_amd.DDPMMulTrainer(types.SimpleNamespace(**opts(TINY2, multi=True, label_path=label, cap_id=False, **extra)), m)


def inputs1(i, c=TINY):
    gi = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    x0 = fill.tensor_for("lossw.x0.%d" % i, (c["B"], c["T"], c["F"])) * 10
    nz = fill.tensor_for("lossw.nz.%d" % i, x0.shape) * 10
    return x0, torch.tensor(STEP_T[i]), gi["length"], gi["xf_proj"], gi["xf_out"], nz


def inputs2(i, rows):
    c = TINY2
    B, T, F = c["B"], c["T"], c["F"]
    x0 = fill.tensor_for("lossw2.x0.%d" % i, (2 * B, T, F)) * 10
    nz = fill.tensor_for("lossw2.nz.%d" % i, x0.shape) * 10
    xp = fill.tensor_for("lossw2.xp", (rows, 4 * c["d"])) * 10
    xo = fill.tensor_for("lossw2.xo", (rows, c["N"], c["Lt"])) * 10
    return x0, torch.tensor(STEP_T[i]), torch.tensor(c["lengths"]), xp, xo, nz


def dev(args):
    return [a.to(DEV) for a in args]


def flat_of(tr):
    return tr.encoder.flat_params().flat


def fused_state_bits(tr):
    st = tr.fused_state()
    out = [flat_of(tr), st["m"], st["v"], st["loss"], st["step"]]
    smp = tr._loss_state(flat_of(tr).device)[1]
    return out + (list(smp.tensors()) if smp is not None else [])


def all_same(a, b):
    return [i for i, (x, y) in enumerate(zip(a, b)) if not torch.equal(x, y)]


def restated_steps(dtype, weights, n_steps=3):
    """Three training steps of `tiny` on the CPU in `dtype`: the oracle's denoiser, q_sample with the fp32 schedule table,
    sum_b w[t_b] sum_frames mean_f (eps - noise)^2 / sum(mask), clip_grad_norm_(0.5), torch Adam.  -> {name: parameter}."""
    c = TINY
    p = {k: v.to(dtype).requires_grad_(True) for k, v in fill.core_params(c["F"], c["d"], c["ff"], c["L"], c["Lt"], c["num_frames"]).items()}
    opt = torch.optim.Adam(list(p.values()), lr=2e-4)
    gd = TI.make_diffusion(1000)
    sa = torch.from_numpy(gd.sqrt_alphas_cumprod).float().to(dtype)
    sb = torch.from_numpy(gd.sqrt_one_minus_alphas_cumprod).float().to(dtype)
    w = torch.as_tensor(weights).float().to(dtype)
    for i in range(n_steps):
        x0, t, ln, xp, xo, nz = inputs1(i)
        x0, nz, xp, xo = (a.to(dtype) for a in (x0, nz, xp, xo))
        xt = sa[t][:, None, None] * x0 + sb[t][:, None, None] * nz
        pred = DR.denoiser_forward(p, xt, t, ln, xp, xo, c["H"], c["L"])
        mask = (torch.arange(c["T"])[None] < ln[:, None]).to(dtype)
        per = (((pred - nz) ** 2).mean(-1) * mask).sum(1)
        loss = (w[t] * per).sum() / mask.sum()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(p.values()), 0.5)
        opt.step()
    return {k: v.detach() for k, v in p.items()}


def rel_all(got, ref):
    """rel-L2 over all the parameters of `ref` at once."""
    num = sum(((got[k].double().cpu() - ref[k].double()) ** 2).sum() for k in ref)
    return float((num / sum((ref[k].double() ** 2).sum() for k in ref)).sqrt())


def test_fused_min_snr_step_against_autograd_and_fp64():
    gamma = 5.0
    weights = min_snr_weights(TI.make_diffusion(1000).alphas_cumprod, gamma)
    ref, cpu32 = restated_steps(torch.float64, weights), restated_steps(torch.float32, weights)
    floor = rel_all(cpu32, ref)
    plain = restated_steps(torch.float64, np.ones(1000))
    assert rel_all(plain, ref) > 1e-5, "the three steps cannot tell the weighted objective from the unweighted one"
    # the fused route
    m = build1()
    tr = trainer1(m, loss_weighting="min_snr", min_snr_gamma=gamma)
    for i in range(3):
        tr.train_step_fused(*dev(inputs1(i)[:5]), noise=inputs1(i)[5].to(DEV))
    fused = {k: v.detach() for k, v in m.state_dict().items() if k in ref}
    assert set(fused) == set(ref)
    # the autograd route: training_losses + backward_G + clip + torch Adam over the same parameters
    m2 = build1()
    tr2 = trainer1(m2, loss_weighting="min_snr", min_snr_gamma=gamma)
    opt = torch.optim.Adam(m2.core_parameters(), lr=2e-4)
    for i in range(3):
        x0, t, ln, xp, xo, nz = dev(inputs1(i))
        out = tr2.diffusion.training_losses(m2, x0, t, model_kwargs={"xf_proj": xp, "xf_out": xo, "length": ln}, noise=nz)
        tr2.real_noise, tr2.fake_noise, tr2._t = out["target"], out["pred"], t
        tr2.src_mask = m2.generate_src_mask(TINY["T"], ln).to(DEV)
        opt.zero_grad()
        tr2.backward_G()
        tr2.loss_mot_rec.backward()
        torch.nn.utils.clip_grad_norm_(m2.core_parameters(), 0.5)
        opt.step()
        m2.params_changed()
    auto = {k: v.detach() for k, v in m2.state_dict().items() if k in ref}
    gate = max(1e-6, 4 * floor)
    d_fused, d_auto = rel_all(fused, ref), rel_all(auto, ref)
    print("GATE min_snr fused %.3e autograd %.3e cpu32 floor %.3e gate %.3e ratio %.3f / %.3f (unweighted fp64 %.3e away)"
          % (d_fused, d_auto, floor, gate, d_fused / gate, d_auto / gate, rel_all(plain, ref)))
    assert d_fused <= gate, "fused route: rel-L2 %.3e above %.3e" % (d_fused, gate)
    assert d_auto <= gate, "autograd route: rel-L2 %.3e above %.3e" % (d_auto, gate)


class Counting:
    """libhig with every call counted by name."""

    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call


NEW_ENTRIES = ("hig_masked_mse_w", "hig_pair_mse_w", "hig_loss_history_update")


def counted(monkeypatch):
    real = _lib.lib()
    proxy = Counting(real)
    monkeypatch.setattr(_lib, "_lib", proxy)
    return proxy


def test_unit_table_through_the_weighted_route_is_the_unweighted_step(monkeypatch):
    """gamma = inf makes the min-SNR table all ones: loss, parameters and both Adam moments of three steps are the unweighted
    step's bits, single-person and PIT -- and the unweighted trainer, with both options unset, launches what it always did:
    no new entry is called."""
    proxy = counted(monkeypatch)
    a, b = trainer1(build1()), trainer1(build1(), loss_weighting="min_snr", min_snr_gamma=float("inf"))
    for i in range(3):
        a.train_step_fused(*dev(inputs1(i)[:5]), noise=inputs1(i)[5].to(DEV))
        assert not [n for n in NEW_ENTRIES if n in proxy.calls], "options unset, yet %s ran" % proxy.calls
        base = dict(proxy.calls)
        b.train_step_fused(*dev(inputs1(i)[:5]), noise=inputs1(i)[5].to(DEV))
        new = {k: v - base.get(k, 0) for k, v in proxy.calls.items() if v != base.get(k, 0)}
        assert new.pop("hig_masked_mse_w") == 1 and "hig_masked_mse" not in new and "hig_loss_history_update" not in new
        assert not all_same(fused_state_bits(a), fused_state_bits(b)), "step %d: %s differ" % (i, all_same(fused_state_bits(a), fused_state_bits(b)))
        proxy.calls = {k: v for k, v in proxy.calls.items() if k not in NEW_ENTRIES}
    assert (b._loss_state(torch.device(DEV, 0))[0] == 1).all()
    c2 = TINY2
    a2, b2 = trainer2(TI.build(c2).train(), None), trainer2(TI.build(c2).train(), None, loss_weighting="min_snr", min_snr_gamma=float("inf"))
    for i in range(2):
        args = dev(inputs2(i, 4 * c2["B"]))
        a2.train_step_fused(*args[:5], noise=args[5])
        assert not [n for n in NEW_ENTRIES if n in proxy.calls]
        b2.train_step_fused(*args[:5], noise=args[5])
        assert proxy.calls.pop("hig_pair_mse_w") == 1
        assert not all_same(fused_state_bits(a2), fused_state_bits(b2)), "PIT step %d differs" % i
    # ... and the batch route draws from the host sampler as before
    a.sampler.sample = lambda bs, d: (torch.tensor(STEP_T[0]).to(d), torch.ones(bs))
    assert a._draw_t(2, torch.device(DEV, 0)).tolist() == list(STEP_T[0])


def lossaware(**extra):
    return dict(loss_weighting="min_snr", min_snr_gamma=5.0, sampler="loss-second-moment", **extra)


def seeded_history(tr):
    """A warmed-up history (every ring full, values from a fixed generator) so that p and w are real, not the uniform ones."""
    smp = tr._loss_state(torch.device(DEV, 0))[1]
    g = torch.Generator().manual_seed(5)
    smp.load_state_dict({"history": torch.rand(smp.num_timesteps, smp.history_per_term, generator=g) + 0.1,
                         "counts": torch.full((smp.num_timesteps,), smp.history_per_term, dtype=torch.int32)})
    assert not (smp.p == smp.p[0]).all()
    return smp


@pytest.mark.parametrize("kind", ("single", "single_bf16", "pit", "labelled"))
def test_captured_step_is_the_fused_step_under_min_snr_and_loss_aware_sampling(kind):
    """Three replays against three eager steps: parameters, moments, loss, step counter, hist, counts, p and w bit for bit.
    Fails when the capture's warm-up step leaks into the loss history."""
    def make():
        if kind.startswith("single"):
            return trainer1(build1("bf16" if kind.endswith("bf16") else None), **lossaware())
        return trainer2(TI.build(TINY2).train(), "labels/" if kind == "labelled" else None, **lossaware())

    def args(i):
        if kind.startswith("single"):
            return dev(inputs1(i, TINY16 if kind.endswith("bf16") else TINY))
        return dev(inputs2(i, (2 if kind == "labelled" else 4) * TINY2["B"]))

    eager, cap = make(), make()
    seeded_history(eager), seeded_history(cap)
    for i in range(3):
        a = args(i)
        eager.train_step_fused(*a[:5], noise=a[5])
        cap.train_step_captured(*a[:5], noise=a[5])
        diff = all_same(fused_state_bits(eager), fused_state_bits(cap))
        assert not diff, "%s step %d: entries %s of (flat, m, v, loss, step, hist, counts, p, w) differ" % (kind, i, diff)
    smp = eager._loss_state(torch.device(DEV, 0))[1]
    assert int(smp.counts.sum()) == smp.num_timesteps * smp.history_per_term       # (full rings stay full)
    assert len(cap.fused_state()["graphs"]) == 1
    # the history moved: the rings of this run's timesteps end in this run's losses
    t_last = torch.tensor(STEP_T[2], device=DEV)
    g = torch.Generator().manual_seed(5)
    seed = torch.rand(smp.num_timesteps, smp.history_per_term, generator=g) + 0.1
    assert not torch.equal(smp.hist[t_last].cpu(), seed[t_last.cpu()])


def test_loss_aware_batch_route_draws_on_the_device_and_weights_the_autograd_route_alike():
    """train_fused_batch draws t from the device sampler; forward() + update() under the same options applies the same
    weights and feeds the same history (per-sample losses within fp32 of the fused step's)."""
    tr = trainer1(build1(), **lossaware())
    smp = seeded_history(tr)
    assert tr.sampler is smp
    torch.manual_seed(11)
    t = tr._draw_t(64, torch.device(DEV, 0))
    assert t.is_cuda and t.dtype == torch.int64 and int(t.min()) >= 0 and int(t.max()) < 1000
    x0, t, ln, xp, xo, nz = dev(inputs1(0))
    before = smp.hist[t].clone()
    tr.train_step_fused(x0, t, ln, xp, xo, noise=nz)
    pushed = smp.hist[t][:, -1].clone()
    assert torch.equal(smp.hist[t][:, :-1], before[:, 1:]), "a full ring did not shift by one"
    # the autograd route on a twin: same loss (to fp32), same pushes (to fp32)
    tw = trainer1(build1(), **lossaware())
    smp2 = seeded_history(tw)
    out = tw.diffusion.training_losses(tw.encoder, x0, t, model_kwargs={"xf_proj": xp, "xf_out": xo, "length": ln}, noise=nz)
    tw.real_noise, tw.fake_noise, tw._t = out["target"], out["pred"], t
    tw.src_mask = tw.encoder.generate_src_mask(TINY["T"], ln).to(DEV)
    logs = tw.backward_G()
    fused_loss = float(tr.fused_state()["loss"])
    assert abs(logs["loss_mot_rec"] - fused_loss) <= 1e-5 * abs(fused_loss)
    assert torch.allclose(smp2.hist[t][:, -1], pushed, rtol=1e-5, atol=0)
    assert torch.equal(smp2.counts, smp.counts)


@pytest.mark.parametrize("captured", (False, True))
def test_resume_equals_the_uninterrupted_run(tmp_path, captured):
    """Two steps, save, two more == load into a fresh trainer, the same two: parameters, moments and the sampler's state."""
    f = str(tmp_path / "latest.tar")

    def run(tr, steps):
        for i in steps:
            a = dev(inputs1(i))
            (tr.train_step_captured if captured else tr.train_step_fused)(*a[:5], noise=a[5])

    t1 = trainer1(build1(), fused_step=True, **lossaware())
    seeded_history(t1)
    run(t1, range(2))
    t1.save(f, 0, 2)
    run(t1, range(2, 4))
    ck = torch.load(f)
    ent = ck["schedule_sampler"]
    assert ent["sampler"] == "loss-second-moment" and ent["loss_weighting"] == "min_snr" and ent["min_snr_gamma"] == 5.0
    assert ent["history"].shape == (1000, 10) and ent["counts"].shape == (1000,) and ent["history_per_term"] == 10
    t2 = trainer1(build1(), fused_step=True, **lossaware())
    assert t2.load(f) == (0, 2)
    run(t2, range(2, 4))
    diff = all_same(fused_state_bits(t1), fused_state_bits(t2))
    assert not diff, "entries %s of (flat, m, v, loss, step, hist, counts, p, w) differ after the resume" % diff
    # an unweighted trainer writes no such key, and loads this file without one
    t3 = trainer1(build1(), fused_step=True)
    t3.save(f + ".plain", 0, 0)
    assert "schedule_sampler" not in torch.load(f + ".plain")
    with pytest.warns(UserWarning, match="loss options"):      # other options than the file's: said, not silent
        assert t3.load(f) == (0, 2)
    assert t3._loss_state(torch.device(DEV, 0)) == (None, None)
    # another static table than the one the rings were recorded under: the history is not taken over
    t4 = trainer1(build1(), fused_step=True, **dict(lossaware(), min_snr_gamma=1.0))
    with pytest.warns(UserWarning, match="empty loss history"):
        t4.load(f)
    assert int(t4._loss_state(torch.device(DEV, 0))[1].counts.sum()) == 0
    # "cuda" names the device the state lives on: nothing is rebuilt
    smp = t2._loss_state(torch.device(DEV, 0))[1]
    assert t2._loss_state("cuda")[1] is smp and t2._loss_state(torch.device("cuda"))[1] is smp


def test_captured_graphs_of_two_shapes_keep_their_buffers():
    """Shape X, shape Y, shape X again on one captured trainer, beside the same eager steps: the graphs of both shapes stay in
    the cache, and the replay of X after Y's capture must still own its scratch and per-sample buffers (Y's are other sizes).
    Fails when a buffer a captured graph points into is replaced."""
    def cut(a, B, T):
        x0, t, ln, xp, xo, nz = a
        return [x0[:B, :T].contiguous(), t[:B].contiguous(), ln[:B].clamp(max=T), xp[:B].contiguous(), xo[:B].contiguous(),
                nz[:B, :T].contiguous()]

    shapes = ((2, 16), (1, 12), (2, 16), (1, 12))
    eager, cap = trainer1(build1(), **lossaware()), trainer1(build1(), **lossaware())
    seeded_history(eager), seeded_history(cap)
    for i, (B, T) in enumerate(shapes):
        a = cut(dev(inputs1(i)), B, T)
        eager.train_step_fused(*a[:5], noise=a[5])
        cap.train_step_captured(*a[:5], noise=a[5])
        # poison whatever the allocator holds free: a graph that replays on a freed buffer would read this
        junk = [torch.full((n,), float("nan"), device=DEV) for n in (1, 2, 12, 32, 1024 + 12, 1024 + 32, 4096)]
        del junk
        diff = all_same(fused_state_bits(eager), fused_state_bits(cap))
        assert not diff, "step %d (B %d, T %d): entries %s of (flat, m, v, loss, step, hist, counts, p, w) differ" % (i, B, T, diff)
    st = cap.fused_state()
    assert len(st["graphs"]) == 2
    sizes = sorted(k[:2] for k in st["loss_buffers"])
    assert sizes == [("mse_w_scratch", NB + 12), ("mse_w_scratch", NB + 32), ("sample_loss", 1), ("sample_loss", 2)], sizes


CAP = ["a person waves", "a person sits down"]


@pytest.mark.parametrize("kind", ("single", "pit", "labelled"))
def test_forward_update_and_the_fused_batch_route_agree_under_both_options(kind):
    """The reference's own entry points with the options set: forward() draws t from the device sampler and keeps it, update()
    weights the loss and pushes the per-sample losses; train_fused_batch on a twin, seeded alike and given forward()'s noise,
    draws the same t and must report the same loss and leave the same history (pairs: one entry per pair under PIT, at
    min(S0, S1) / (2 len); one per row with labels) -- the fused side being hig_masked_mse_w / hig_pair_mse_w, held to their
    bounds above."""
    c = TINY if kind == "single" else TINY2
    B, T, F = c["B"], c["T"], c["F"]
    lens = torch.tensor(c["lengths"])

    def make():
        if kind == "single":
            return trainer1(build1(), **lossaware())
        return trainer2(TI.build(TINY2).train(), "labels/" if kind == "labelled" else None, **lossaware())

    if kind == "single":
        batch = (CAP, fill.tensor_for("lossw.fwd.m", (B, T, F)) * 10, lens)
    else:
        batch = (TI.CAP1, TI.CAP2, fill.tensor_for("lossw.fwd.m1", (B, T, F)) * 10, fill.tensor_for("lossw.fwd.m2", (B, T, F)) * 10, lens, None)
    auto, fused = make(), make()
    smp_a, smp_f = seeded_history(auto), seeded_history(fused)
    before = smp_a.hist.clone()
    auto.opt_encoder = torch.optim.Adam(auto.encoder.parameters(), lr=2e-4)
    torch.manual_seed(23)
    auto.forward(batch)
    t = auto._t
    assert auto.sampler is smp_a and t.is_cuda and t.dtype == torch.int64 and t.numel() == (B if kind == "single" else 2 * B)
    if kind != "single":
        assert torch.equal(t[:B], t[B:]), "the two persons of a pair do not share t"
    assert len(set(t[:B].tolist())) == B, "the seed draws one t twice: the pushes could not be told apart"
    noise = auto.real_noise
    if kind == "pit":
        assert noise.shape[0] == 4 * B
        noise = torch.cat([noise[:B], noise[2 * B:3 * B]])
    logs = auto.update()
    torch.manual_seed(23)
    loss = fused.train_fused_batch(batch, noise=noise.contiguous())
    assert abs(logs["loss_mot_rec"] - float(loss)) <= 1e-5 * abs(float(loss)), (logs, float(loss))
    assert torch.equal(smp_a.counts, smp_f.counts)
    moved = (smp_a.hist != before).any(dim=1).nonzero().flatten()
    assert sorted(moved.tolist()) == sorted(t[:B].tolist()), "the history moved at %s, t is %s" % (moved.tolist(), t.tolist())
    assert torch.allclose(smp_a.hist, smp_f.hist, rtol=1e-5, atol=0), "the two routes push different losses"
    if kind == "labelled":      # one entry per row: the ring of a pair's t took both persons' losses
        assert torch.equal(smp_a.hist[t[:B]][:, :-2], before[t[:B]][:, 2:])
    else:
        assert torch.equal(smp_a.hist[t[:B]][:, :-1], before[t[:B]][:, 1:])
