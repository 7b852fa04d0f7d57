"""The fp32-storage training step (hig_text_context and hig_denoiser_fwd with training = 1, hig_denoiser_bwd[_hooked];
csrc/denoiser.hip) restated launch by launch, with the element-wise bound of every launch and the composition mutants, in the
form of tests/bf16_step_bounds.py, whose `Walk` supplies the buffers (get / put), the parameters, the GEMM stages, the
linear-attention context build and backward, and the time / text embedding path.  Plain torch on the host:
tests/test_cpu_f32_step_bounds.py proves without a GPU that the stages compose to the model (oracle.denoiser_ref /
oracle.interaction_ref under autograd), that an fp32 stand-in stays within the bounds and that every mutant breaks one;
tests/test_gpu_f32_step_contract.py holds the device to the same walk.

Everything here is for dims.prec == HIG_PREC_F32 and storage == HIG_STORE_F32.  The bf16x3 and bf16 product modes of fp32 storage
have no per-element GEMM bound in this project: they stay with their present tests (tests/test_gpu_kernels.py,
tests/test_gpu_denoiser.py).  The captured (hipGraph) step keeps its eager-equals-captured test and is not walked here.

ONE WALK, THREE USES (see tests/bf16_step_bounds.py): chain EXACT (fp64: the operator itself), chain STANDIN (fp32 torch, one
composition `mutant` switched on), and `check`: every stage evaluated in fp64 on operands read from a TRACE (the device's own
buffers) and the traced result held to the stage's bound.  Nothing here bounds the whole model.  A stage takes the bound its
kernel already has in this repository:
  ln / ln_sty     rowops_bounds.ln_fwd_bound: the rows, and the (mean, rstd) pairs hig_rowstats / hig_layernorm / hig_ln_mod_silu
                  save (hig_silu: G = 3)
  ln_bwd          rowops_bounds.ln_bwd_bound(bf16=False) with the SAVED statistics the call is given: dx, dgamma, dbeta, dscale, dshift
  colsum          rowops_bounds.colsum_bound;   temb   boundary_bounds.temb_bound;   dsilu   bf16_step_bounds.dsilu_bound
  gemm32          test_gpu_gemm_contract.linear_ref: gamma ||X_i|| ||W_j|| + 2^-23 (|bias| + |res|), gamma = 2 K 2^-24; the positional
                  term of HIG_EPI_BIAS_POS is a residual.  A SiLU-on-load operand costs silu_operand_error through Cauchy-Schwarz
                  (bf16_step_bounds.gemm32).  The bound is on the sum in ANY order: it holds for the few-row split over the reduce
                  range (hig_gemm_few_rows), for the split tail and for split-R slabs alike.
  gemm32_gelu / gemm32_dgelu   gemm_bound with GELU32_PER_Z / DGELU_ABS (act_bound); the saved pre-activation z1 the linear bound
  gemm32_ln       an operand LayerNorm'ed as it is loaded from the statistics the call is GIVEN, (x - mean) rstd gamma + beta
                  (xf_apply, csrc/gemm.hip): the text key / value projection and the CA_KV_W gradient.  The same construction as
                  SiLU-on-load: the reference is the exact LayerNorm of the rows, the operand's own error e_ln is the `out` bound of
                  ln_fwd_bound (which is built from exactly this expression on statistics within their bounds -- the walk holds the
                  statistics to those bounds where they are written), and it reaches the sum through Cauchy-Schwarz:
                  + ||e_ln,i|| ||w_j|| (forward), + ||dC_:,n|| ||e_ln,:,k|| (weight gradient).
  wgrad32         the linear bound over the rows (K = rows), valid for any number of split-R slabs.  xsum: the bias gradient the
                  GEMM sums on the side, rows terms in any order: rows u sum |dC| (column counts that are no multiple of 4 take
                  hig_colsum instead: `colsum`).
  ctx / apply / apply_bwd / ctx_bwd   lin_gammas of test_gpu_attn_contract.py: g u M + 2^-120, M from the |A|, |dA| the call is
                  given; the column term of dK and the key weights from the device's own A and kstat (teacher forcing; the note in
                  tests/bf16_step_bounds.py applies)
  full / full_bwd test_gpu_attn_contract.full_reference / full_bounds: y, lse; dQ, dK, dV from the lse and y the call is GIVEN;
                  delta = sum_l dy y over hd channels: (hd + 1) u sum |dy y| (tests/enc_step_bounds.py)
  copy            bit-equal: each layer's W^T, doutm, the init-pose rows tok0, the shifted d(sequence_embedding) and its zero tail,
                  dxf_proj, dxf_out, the d(scale, shift) table against its tapped slices
`MUTANTS` are faults of COMPOSITION -- a stage handed the wrong buffer, slice, offset, length or generation of a reused scratch.

CASES are the smallest shapes at which each form still exists (B is the model batch); REACH lists what the step moves at each.
Paths the BASELINE.md training shapes reach that no case here reaches are listed in NOT_COVERED with the reason.
"""
import math

import torch

import bf16_step_bounds as sb
import boundary_bounds as bb
import linattn16_bounds as lb
import rowops_bounds as rb
import test_gpu_attn_contract as AC        # (full_reference, full_bounds, lin_gammas: the module runs nothing on import)
import test_gpu_gemm_contract as gm
from hig_amd import _lib
from linattn16_bounds import FLOOR
from rowops_bounds import F32, F64, U

MUTANTS = ("sty_reads_next_block_slice", "contexts_not_swapped", "partner_lengths_not_swapped", "position_shift_missing",
           "w1_dgrad_residual_dropped", "ln_bwd_res_dropped_at_prenorm", "dxf_out_last_term_only", "dxf_out_accumulates_at_last_layer",
           "dgrad_previous_layer_weights", "ca_kv_wgrad_unnormalised_rows", "cross_masked_with_motion_lengths", "doutm_init_rows_not_zeroed",
           "init_rows_left_in_dh_for_joint_embed", "dx_init_row_all_features", "seq_emb_zero_tail_missing", "w_emb_rows_from_wrong_layer",
           "wgrad_reads_dh_after_swap", "bias_grad_misses_one_split")
TWO_PERSON_MUTANTS = ("contexts_not_swapped", "partner_lengths_not_swapped", "position_shift_missing", "doutm_init_rows_not_zeroed",
                      "init_rows_left_in_dh_for_joint_embed", "dx_init_row_all_features")
FULL_MUTANTS = ("cross_masked_with_motion_lengths",)
HOOKED_MUTANTS = ("w_emb_rows_from_wrong_layer",)
STALE = 1.0
EXACT, STANDIN, REF = sb.Ar(F64, False), sb.Ar(F32, False), sb.Ar(F64, False)

CASES = {
    "small": dict(B=2, T=33, F=12, d=128, H=2, L=2, ff=96, N=77, Lt=32, num_frames=40, lengths=(33, 5), t=(7, 650), two=0, full=0),
    # head dim 8: the VALU attention kernels; F % 4 != 0: `out` takes the column-sum path, a gradient with (I J) % 4 != 0 is unsplit
    "narrow": dict(B=3, T=20, F=10, d=64, H=8, L=1, ff=36, N=5, Lt=12, num_frames=20, lengths=(20, 1, 7), t=(0, 999, 313), two=0, full=0),
    "hd128": dict(B=3, T=75, F=150, d=256, H=2, L=2, ff=512, N=77, Lt=64, num_frames=80, lengths=(75, 40, 1), t=(0, 999, 313), two=0, full=0),
    "pairs": dict(B=4, T=21, F=12, d=128, H=2, L=2, ff=96, N=77, Lt=32, num_frames=40, lengths=(21, 9, 13, 21), t=(7, 650, 3, 999), two=1, full=0),
    "pairs_nocross": dict(B=4, T=21, F=12, d=128, H=2, L=2, ff=96, N=77, Lt=32, num_frames=40, lengths=(21, 9, 13, 21), t=(7, 650, 3, 999), two=2,
                          full=0),
    "full": dict(B=2, T=33, F=12, d=128, H=2, L=2, ff=96, N=77, Lt=32, num_frames=40, lengths=(33, 5), t=(7, 650), two=0, full=1),
    "full_hd128": dict(B=2, T=70, F=12, d=256, H=2, L=1, ff=96, N=77, Lt=32, num_frames=70, lengths=(70, 23), t=(7, 650), two=0, full=1),
    # M = 520 >= 512: the first size at which wgrad_splits splits the rows (slabs, the column sums parked behind them); three 64-row
    # chunks with a ragged one
    "rows520": dict(B=4, T=130, F=12, d=128, H=2, L=1, ff=96, N=77, Lt=32, num_frames=130, lengths=(130, 64, 1, 129), t=(7, 650, 3, 999), two=0,
                    full=0),
}


class Dims(sb.Dims):
    def __init__(self, c):
        super().__init__(c)
        self.full, self.inter = bool(c["full"]), c["two"] == 1
        self.nsty = 4 if self.inter else 3
        self.ss_ld = self.nsty * self.L * 2 * self.d


def build_model(c, device="cpu", **kw):
    if c["full"]:
        kw["no_eff"] = True
    if c["two"] == 2:
        kw["no_cross_attn"] = True
    return sb.build_model(c, device, **kw)


# ----------------------------------------------------------------------------------------------------------------------
# full attention in a walk's arithmetic (the chains; the check uses test_gpu_attn_contract.full_reference / full_bounds)
# ----------------------------------------------------------------------------------------------------------------------
def full_scores(q, k, qlen, B, Tq, Tk, H, hd):
    s = torch.einsum("bnhd,bmhd->bhnm", q.reshape(B, Tq, H, hd), k.reshape(B, Tk, H, hd)) / math.sqrt(hd)
    if qlen is not None:        # the reference's mask lands on the QUERY axis: -1e5 on every logit of a row at or beyond the length
        off = (torch.arange(Tq)[None] >= qlen[:, None]).to(s.dtype) * -100000.0
        s = s + off[:, None, :, None]
    return s


def full_fwd(q, k, v, qlen, B, Tq, Tk, H, hd):
    """-> y (B Tq, d), lse (B, H, Tq)."""
    s = full_scores(q, k, qlen, B, Tq, Tk, H, hd)
    y = torch.einsum("bhnm,bmhl->bnhl", torch.softmax(s, -1), v.reshape(B, Tk, H, hd))
    return y.reshape(B * Tq, H * hd), torch.logsumexp(s, -1)


def full_bwd(dy, y, q, k, v, lse, qlen, B, Tq, Tk, H, hd):
    """hig_fullattn_bwd -> dq (B Tq, d), dk, dv (B Tk, d), delta (B, H, Tq).  A chain's lse is the log-sum-exp of these very
    logits, so the fp64 chain takes the weights as their softmax: exp(s - lse) would round lse at the 1e5 of the offset rows
    (1e-11 relative in fp64, against the 1e-15 the composition test gates at).  The fp32 stand-in does what the kernel does."""
    s = full_scores(q, k, qlen, B, Tq, Tk, H, hd)
    dyh, yh = dy.reshape(B, Tq, H, hd), y.reshape(B, Tq, H, hd)
    w = torch.softmax(s, -1) if s.dtype == F64 else torch.exp(s - lse[..., None])
    delta = (dyh * yh).sum(-1).permute(0, 2, 1)
    dS = w * (torch.einsum("bnhl,bmhl->bhnm", dyh, v.reshape(B, Tk, H, hd)) - delta[..., None]) / math.sqrt(hd)
    dq = torch.einsum("bhnm,bmhd->bnhd", dS, k.reshape(B, Tk, H, hd))
    dk = torch.einsum("bhnm,bnhd->bmhd", dS, q.reshape(B, Tq, H, hd))
    dv = torch.einsum("bhnm,bnhl->bmhl", w, dyh)
    return dq.reshape(B * Tq, H * hd), dk.reshape(B * Tk, H * hd), dv.reshape(B * Tk, H * hd), delta


# ----------------------------------------------------------------------------------------------------------------------
# the walk
# ----------------------------------------------------------------------------------------------------------------------
class Walk(sb.Walk):
    """trace None: a chain in arithmetic `ar` (its buffers end up in self.out); else a check of `trace` (ar is REF), self.worst =
    {stage kind: (largest |error| / bound, the buffer that gave it)}, self.seen the buffers held.  self.spread: the largest softmax
    spread met (the validity condition of the attention bounds: <= 80)."""
    u16 = 0.0

    def __init__(self, P, D, inp, ar=REF, trace=None, mutant=None, te=None, hooked=False):
        assert mutant is None or (mutant in MUTANTS and trace is None)
        assert mutant not in HOOKED_MUTANTS or hooked
        self.P, self.D, self.inp, self.ar, self.src, self.mut, self.te = P, D, inp, ar, trace, mutant, te
        self.forms = {"ctx_mm16": False}
        self.check = trace is not None
        self.out, self.worst, self.seen, self.spread = {}, {}, set(), 0.0

    def put(self, kind, key, value, bound=None, bf16=False, sel=None):
        self.seen.add(key)
        super().put(kind, key, value, bound, False, sel)

    # ---- stages ----
    def lnf(self, kind, kx, kst, x, gamma, beta, ss=None, rps=1):
        """hig_layernorm / hig_ln_mod_silu (kx None: hig_rowstats): the rows and the (mean, rstd) pairs they save."""
        if not self.check:
            y, mu, r = rb.ln_fwd_eval(x, gamma, beta, ss, rps, dtype=self.ar.dtype)
            if kx is not None:
                self.out[kx] = y
            self.out[kst] = torch.stack([mu, r], 1)
            return
        b = rb.ln_fwd_bound(x, gamma, beta, ss, rps)
        if kx is not None:
            self.put(kind, kx, b["out"][0], lambda: b["out"][1])
        self.put(kind, kst, b["mean"][0], lambda: b["mean"][1], sel=lambda t: t[:, 0])
        self.put(kind, kst, b["rstd"][0], lambda: b["rstd"][1], sel=lambda t: t[:, 1])

    def lnb(self, da, x, stats, gamma, beta, ss, res, rps):
        """hig_ln_bwd with the statistics it is given -> {name: (value, bound callable)}."""
        names = ("dx", "dgamma", "dbeta", "dscale", "dshift")
        if not self.check:
            v = rb.ln_bwd_eval(da, x, stats, gamma, beta, ss, res, rps, dtype=self.ar.dtype)
            return {n: (v[i], None) for i, n in enumerate(names) if v[i] is not None}
        b = rb.ln_bwd_bound(da, x, stats, gamma, beta, ss, res, rps, bf16=False)
        return {n: (b[n][0], (lambda n=n: b[n][1])) for n in names if n in b}

    def ln_operand(self, x, stats, gamma, beta):
        """An operand LayerNorm'ed on load -> (values, None | its own error e_ln (rows, n))."""
        if not self.check:
            return (x - stats[:, :1]) * stats[:, 1:] * gamma + beta, None
        b = rb.ln_fwd_bound(x, gamma, beta)
        return b["out"][0], b["out"][1]

    def gelu_gemm(self, l, h):
        """linear1 with the GELU epilogue: f1, and the pre-activation z1 it saves."""
        W1, b1 = self.pl(l, _lib.L_FFN_W1), self.pl(l, _lib.L_FFN_B1)
        pre = h @ W1.t() + b1
        bd = gm.gemm_bound(h, W1, gm.GELU, b1, None, False, False) if self.check else None
        self.put("gemm32", ("z1", l), pre, (lambda: bd[3]) if self.check else None)
        self.put("gemm32_gelu", ("f1", l), rb.gelu_eval(pre, dtype=self.ar.dtype), (lambda: bd[1]) if self.check else None)

    def wg(self, key_w, key_b, dC, act, e_act=None, xsum=True):
        """A weight gradient dW = dC^T act over the rows and the bias gradient of the same Linear (xsum: summed by the GEMM; else
        hig_colsum).  e_act: the own error of an operand transformed on load."""
        rows = dC.shape[0]
        dCb = dC
        if self.mut == "bias_grad_misses_one_split" and key_b == ("gl", 0, _lib.L_SA_QKV_B):
            dCb = dC[rows // 3:]            # (the first rows: those at and beyond a sample's length carry exact zeros)

        def bound():
            b = gm.linear_ref(dC.t(), act.t(), gm.NONE, None, None)[1]
            return b if e_act is None else b + torch.outer(dC.norm(dim=0), e_act.norm(dim=0))
        self.put("wgrad32", key_w, dC.t() @ act, bound)
        if key_b is None:
            return
        if xsum:
            self.put("xsum", key_b, dCb.sum(0), lambda: rows * U * dC.abs().sum(0))
        else:
            self.put("colsum", key_b, dCb.sum(0), lambda: rb.colsum_bound(dC)[1])

    def lens(self):
        return self.inp["length"]

    def run(self):
        self.text_context()
        self.forward()
        self.backward()
        return self

    def note_spread(self, x):
        self.spread = max(self.spread, float(x))

    # ---- hig_text_context(training = 1) ----
    def text_context(self):
        D, L, d = self.D, _lib, self.D.d
        xf = self.ar.c(self.inp["xf_out"]).reshape(D.Mt, D.Lt)
        one, zero = torch.ones(D.Lt, dtype=self.ar.dtype), torch.zeros(D.Lt, dtype=self.ar.dtype)
        self.lnf("ln", None, "stt", xf, one, zero)
        for l in range(D.L):
            xn, e = self.ln_operand(xf, self.get("stt"), self.pl(l, L.L_CA_TNORM_W), self.pl(l, L.L_CA_TNORM_B))
            W, b = self.pl(l, L.L_CA_KV_W), self.pl(l, L.L_CA_KV_B)
            self.put("gemm32_ln", ("kv", l), xn @ W.t() + b,
                     lambda xn=xn, e=e, W=W, b=b: gm.linear_ref(xn, W, gm.BIAS, b, None)[1] + torch.outer(e.norm(dim=1), W.norm(dim=1)))
            if not D.full:
                kv = self.get(("kv", l))
                lens = self.lens().clamp_max(D.N) if self.mut == "cross_masked_with_motion_lengths" else None
                self.context(("Ac", l), ("kstc", l), kv[:, :d], kv[:, d:], D.N, lens)

    def context(self, kA, kst, K, V, rows, lens):
        if self.check:
            D = self.D
            self.note_spread(lb.ctx_exact(sb.heads(K, D.B, rows, D.H, D.hd), sb.heads(V, D.B, rows, D.H, D.hd), lens)[4])
        super().context(kA, kst, K, V, rows, lens)

    # ---- attention forward ----
    def apply(self, ky, q, A):
        """hig_linattn_apply: y = softmax(q) A, A (B', H, hd, hd) [c][l] as the consumer samples see it."""
        D = self.D
        B = A.shape[0]
        qv = sb.heads(q, B, D.T, D.H, D.hd)
        p = torch.softmax(qv, -1)
        y = torch.einsum("bnhc,bhcl->bnhl", p, A).reshape(B * D.T, D.d)

        def by():
            Xq = (qv.amax(-1) - qv.amin(-1)).max().item()
            self.note_spread(Xq)
            assert Xq <= 80
            My = torch.einsum("bnhc,bhcl->bnhl", p, A.abs()).reshape(B * D.T, D.d)
            return AC.lin_gammas(D.T, D.hd, Xq, 0.0)["y"] * U * My + FLOOR
        self.put("apply", ky, y, by)

    def full_attention(self, ky, klse, q, kv, Tk, qlen):
        D, d = self.D, self.D.d
        if not self.check:
            self.out[ky], self.out[klse] = full_fwd(q, kv[:, :d], kv[:, d:], qlen, D.B, D.T, Tk, D.H, D.hd)
            return
        r = AC.full_reference(q.contiguous(), kv.contiguous(), None, D.B, D.T, Tk, D.H, D.hd, qlen, None)
        self.note_spread(r["X"].max().item() - math.log(Tk))
        assert r["X"].max().item() <= 80 + math.log(Tk), "logit spread above 80"
        b = AC.full_bounds(r, D.B, D.T, Tk, D.H, D.hd)
        self.put("full", ky, r["y"].reshape(D.M, d), lambda: b["y"].reshape(D.M, d))
        self.put("full", klse, r["lse"], lambda: b["lse"])

    def full_attention_bwd(self, l, pre, dy, y, q, kv, lse, Tk, qlen):
        """-> (pre_dq | sa_dqkv), ca_dkv, pre_delta."""
        D, d = self.D, self.D.d
        Rk = D.B * Tk
        if not self.check:
            dq, dk, dv, delta = full_bwd(dy, y, q, kv[:, :d], kv[:, d:], lse, qlen, D.B, D.T, Tk, D.H, D.hd)
            self.out[(pre + "_delta", l)] = delta
            if pre == "ca":
                self.out[("ca_dq", l)], self.out[("ca_dkv", l)] = dq, torch.cat([dk, dv], 1)
            else:
                self.out[("sa_dqkv", l)] = torch.cat([dq, dk, dv], 1)
            return
        r = AC.full_reference(q.contiguous(), kv.contiguous(), dy.contiguous(), D.B, D.T, Tk, D.H, D.hd, qlen, None, lse_in=lse, y_in=y.contiguous())
        b = AC.full_bounds(r, D.B, D.T, Tk, D.H, D.hd)
        if pre == "ca":
            self.put("full_bwd", ("ca_dq", l), r["dQ"].reshape(D.M, d), lambda: b["dQ"].reshape(D.M, d))
            self.put("full_bwd", ("ca_dkv", l), r["dK"].reshape(Rk, d), lambda: b["dK"].reshape(Rk, d), sel=lambda t: t[:, :d])
            self.put("full_bwd", ("ca_dkv", l), r["dV"].reshape(Rk, d), lambda: b["dV"].reshape(Rk, d), sel=lambda t: t[:, d:])
        else:
            for i, name in enumerate(("dQ", "dK", "dV")):
                self.put("full_bwd", ("sa_dqkv", l), r[name].reshape(D.M, d), lambda name=name: b[name].reshape(D.M, d),
                         sel=lambda t, i=i: t[:, i * d:(i + 1) * d])
        t = dy.reshape(D.B, D.T, D.H, D.hd) * y.reshape(D.B, D.T, D.H, D.hd)
        self.put("full_bwd", (pre + "_delta", l), t.sum(-1).permute(0, 2, 1), lambda: (D.hd + 1) * U * t.abs().sum(-1).permute(0, 2, 1))

    def sty_front(self, l, slot, ky, ka, kst, norm_w, norm_b, ss_rows=None):
        """hig_ln_mod_silu: a = silu(LN(y) (1 + scale) + shift) with block `slot`'s slice of the modulation table."""
        D = self.D
        if self.mut == "sty_reads_next_block_slice" and slot == 0 and l == 0:
            slot = 1
        ss = self.get("ss")
        if ss_rows is not None:
            ss = ss[ss_rows]
        s6 = sb.ss6(ss, (D.nsty * l + slot) * 2 * D.d, D.d)
        self.lnf("ln_sty", ka, kst, self.get(ky), self.pl(l, norm_w), self.pl(l, norm_b), s6, D.T)

    def sty_out32(self, l, ka, res, kh, out_w, out_b):
        self.put("gemm32", kh, *self.gemm32(self.get(ka), self.pl(l, out_w), self.pl(l, out_b), res))

    # ---- hig_denoiser_fwd(training = 1) ----
    def forward(self):
        D, L, ar, mut, d = self.D, _lib, self.ar, self.mut, self.D.d
        x = ar.c(self.inp["x"]).reshape(D.M, D.F)
        if self.te is not None:
            self.out["te"] = ar.c(self.te)
        else:
            self.put("temb", "te", bb.temb_eval(self.inp["t"], d, dtype=ar.dtype), lambda: bb.temb_bound(self.inp["t"], d)[1])
        self.put("gemm32", "te_h", *self.gemm32(self.get("te"), self.pg(L.P_TE0_W), self.pg(L.P_TE0_B)))
        self.put("gemm32", "emb", *self.gemm32(self.get("te_h"), self.pg(L.P_TE2_W), self.pg(L.P_TE2_B), ar.c(self.inp["xf_proj"]), silu_x=True))
        self.put("gemm32", "ss", *self.gemm32(self.get("emb"), self.pg(L.P_STY_EMB_W), self.pg(L.P_STY_EMB_B), silu_x=True))
        # h0 = joint_embed(x) + sequence_embedding (two-person: frame t >= 1 gets row t - 1; the init-pose rows through joint_embed2)
        shift = 1 if (D.two and mut != "position_shift_missing") else 0
        tpos = torch.arange(D.T) - shift
        pos = (self.pg(L.P_SEQ_EMB)[tpos.clamp_min(0)] * (tpos >= 0).to(ar.dtype)[:, None]).repeat(D.B, 1)
        h0, bnd = self.gemm32(x, self.pg(L.P_JOINT_W), self.pg(L.P_JOINT_B), pos)
        first = torch.arange(D.M) % D.T == 0
        if D.two:
            v0, b0 = self.gemm32(ar.c(self.inp["x"])[:, 0, :4], self.pg(L.P_JOINT2_W), self.pg(L.P_JOINT2_B))
            h0 = h0.clone()
            h0[first] = v0
            inner = bnd

            def bnd():
                b = inner().clone()
                b[first] = b0()
                return b
        self.put("gemm32", "h0", h0, bnd)
        length = self.lens()
        len_partner = sb.swap_halves(length) if (D.two and mut != "partner_lengths_not_swapped") else length
        hin = "h0"
        for l in range(D.L):
            # ---- self attention ----
            self.lnf("ln", ("xn1", l), ("st1", l), self.get(hin), self.pl(l, L.L_SA_NORM_W), self.pl(l, L.L_SA_NORM_B))
            self.put("gemm32", ("qkv", l), *self.gemm32(self.get(("xn1", l)), self.pl(l, L.L_SA_QKV_W), self.pl(l, L.L_SA_QKV_B)))
            qkv = self.get(("qkv", l))
            if D.full:
                self.full_attention(("y1", l), ("lse1", l), qkv[:, :d], qkv[:, d:], D.T, length)
            else:
                self.context(("A1", l), ("kst1", l), qkv[:, d:2 * d], qkv[:, 2 * d:], D.T, length)
                self.apply(("y1", l), qkv[:, :d], self.get(("A1", l)))
            self.sty_front(l, 0, ("y1", l), ("a1", l), ("st2", l), L.L_SA_STY_NORM_W, L.L_SA_STY_NORM_B)
            self.sty_out32(l, ("a1", l), self.get(hin), ("h1", l), L.L_SA_STY_OUT_W, L.L_SA_STY_OUT_B)
            # ---- cross attention ----
            self.lnf("ln", ("xn2", l), ("st3", l), self.get(("h1", l)), self.pl(l, L.L_CA_NORM_W), self.pl(l, L.L_CA_NORM_B))
            self.put("gemm32", ("qc", l), *self.gemm32(self.get(("xn2", l)), self.pl(l, L.L_CA_Q_W), self.pl(l, L.L_CA_Q_B)))
            if D.full:
                self.full_attention(("y2", l), ("lse2", l), self.get(("qc", l)), self.get(("kv", l)), D.N,
                                    length if mut == "cross_masked_with_motion_lengths" else None)
            else:
                self.apply(("y2", l), self.get(("qc", l)), self.get(("Ac", l)))
            self.sty_front(l, 1, ("y2", l), ("a2", l), ("st4", l), L.L_CA_STY_NORM_W, L.L_CA_STY_NORM_B)
            self.sty_out32(l, ("a2", l), self.get(("h1", l)), ("h2", l), L.L_CA_STY_OUT_W, L.L_CA_STY_OUT_B)
            hffn = ("h2", l)
            if D.inter:
                # ---- person <-> person: key / value from the partner's stream, masked with the consumer's length ----
                self.lnf("ln", ("xn3", l), ("st6", l), self.get(("h2", l)), self.pl(l, L.L_INT_NORM_W), self.pl(l, L.L_INT_NORM_B))
                self.put("gemm32", ("iqkv", l), *self.gemm32(self.get(("xn3", l)), self.pl(l, L.L_INT_QKV_W), self.pl(l, L.L_INT_QKV_B)))
                iqkv = self.get(("iqkv", l))
                self.context(("Ai", l), ("ksti", l), iqkv[:, d:2 * d], iqkv[:, 2 * d:], D.T, len_partner)
                Ai = self.get(("Ai", l))
                self.apply(("y4", l), iqkv[:, :d], Ai if mut == "contexts_not_swapped" else sb.swap_halves(Ai))
                self.sty_front(l, 2, ("y4", l), ("a4", l), ("st7", l), L.L_INT_STY_NORM_W, L.L_INT_STY_NORM_B)
                self.sty_out32(l, ("a4", l), self.get(("h2", l)), ("h2b", l), L.L_INT_STY_OUT_W, L.L_INT_STY_OUT_B)
                hffn = ("h2b", l)
            # ---- FFN ----
            self.gelu_gemm(l, self.get(hffn))
            self.put("gemm32", ("y3", l), *self.gemm32(self.get(("f1", l)), self.pl(l, L.L_FFN_W2), self.pl(l, L.L_FFN_B2)))
            self.sty_front(l, D.nsty - 1, ("y3", l), ("a3", l), ("st5", l), L.L_FFN_STY_NORM_W, L.L_FFN_STY_NORM_B)
            self.sty_out32(l, ("a3", l), self.get(hffn), ("h3", l), L.L_FFN_STY_OUT_W, L.L_FFN_STY_OUT_B)
            hin = ("h3", l)
        hL = self.get(hin)
        out, bnd = self.gemm32(hL, self.pg(L.P_OUT_W), self.pg(L.P_OUT_B))
        if D.two:
            o2, b2 = self.gemm32(hL[first], self.pg(L.P_OUT2_W), self.pg(L.P_OUT2_B))
            out = out.clone()
            out[first] = o2
            inner2 = bnd

            def bnd():
                b = inner2().clone()
                b[first] = b2()
                return b
        self.put("gemm32", "out", out, bnd)

    # ---- hig_denoiser_bwd[_hooked] ----
    def sty_bwd(self, l, slot, dh, ky, ka, kst, norm_w, norm_b, out_w, out_b, pre):
        D, L = self.D, _lib
        self.wg(("gl", l, out_w), ("gl", l, out_b), dh, self.get(ka))
        Wl = l + 1 if (self.mut == "dgrad_previous_layer_weights" and pre == "ffn" and l + 1 < D.L) else l
        self.put("gemm32", (pre + "_t1", l), *self.gemm32(dh, self.pl(Wl, out_w).t()))
        off = (D.nsty * l + slot) * 2 * D.d
        r = self.lnb(self.get((pre + "_t1", l)), self.get(ky), self.get(kst), self.pl(l, norm_w), self.pl(l, norm_b), sb.ss6(self.get("ss"), off, D.d),
                     None, D.T)
        self.put("ln_bwd", (pre + "_dy", l), *r["dx"])
        self.put("ln_bwd", ("gl", l, norm_w), *r["dgamma"])
        self.put("ln_bwd", ("gl", l, norm_b), *r["dbeta"])
        if self.check:
            self.put("ln_bwd", (pre + "_dss", l), *r["dscale"], sel=lambda t: t[:, :D.d])
            self.put("ln_bwd", (pre + "_dss", l), *r["dshift"], sel=lambda t: t[:, D.d:])
            self.put("copy", "dss", self.get((pre + "_dss", l)), None, sel=lambda t: t[:, off:off + 2 * D.d])
        else:
            self.out[(pre + "_dss", l)] = torch.cat([r["dscale"][0], r["dshift"][0]], 1)
            self.dss[:, off:off + 2 * D.d] = self.out[(pre + "_dss", l)]

    def prenorm_bwd(self, l, pre, kx, kst, norm_w, norm_b, dh, qkv_w):
        """t2 = dq . W, then the pre-norm's backward with the residual-stream gradient as `res` -> the next dh."""
        dq = self.get((pre + ("_dq" if pre == "ca" else "_dqkv"), l))
        self.put("gemm32", (pre + "_t2", l), *self.gemm32(dq, self.pl(l, qkv_w).t()))
        res = None if (self.mut == "ln_bwd_res_dropped_at_prenorm" and pre == "ca") else dh
        r = self.lnb(self.get((pre + "_t2", l)), self.get(kx), self.get(kst), self.pl(l, norm_w), self.pl(l, norm_b), None, res, self.D.T)
        self.put("ln_bwd", (pre + "_dh", l), *r["dx"])
        self.put("ln_bwd", ("gl", l, norm_w), *r["dgamma"])
        self.put("ln_bwd", ("gl", l, norm_b), *r["dbeta"])

    def wT(self, l):
        """One layer's transposed weights in the order of BwdLayout::wT (csrc/denoiser.hip)."""
        L = _lib
        slots = [L.L_FFN_STY_OUT_W, L.L_FFN_W2, L.L_FFN_W1, L.L_CA_STY_OUT_W, L.L_CA_Q_W, L.L_CA_KV_W, L.L_SA_STY_OUT_W, L.L_SA_QKV_W]
        if self.D.inter:
            slots += [L.L_INT_STY_OUT_W, L.L_INT_QKV_W]
        return torch.cat([self.pl(l, s).t().reshape(-1) for s in slots])

    def backward(self):
        D, L, ar, mut, d = self.D, _lib, self.ar, self.mut, self.D.d
        x = ar.c(self.inp["x"]).reshape(D.M, D.F)
        dout = ar.c(self.inp["dout"]).reshape(D.M, D.F)
        first = torch.arange(D.M) % D.T == 0
        hL = self.get(("h3", D.L - 1))
        xsum_F = D.F % 4 == 0
        if not self.check:
            self.dss = torch.zeros(D.B, D.ss_ld, dtype=ar.dtype)
        # ---- output projection ----
        dout_m = dout
        if D.two:
            self.put("copy", "doutm", dout if mut == "doutm_init_rows_not_zeroed" else dout.masked_fill(first[:, None], 0.0), None)
            dout_m = self.get("doutm")
            d0 = dout[first]
            self.put("colsum", ("g", L.P_OUT2_B), d0.sum(0), lambda: rb.colsum_bound(d0)[1])
            self.wg(("g", L.P_OUT2_W), None, d0, hL[first])
            tok, btok = self.gemm32(d0, self.pg(L.P_OUT2_W).t())
        self.put("colsum", ("g", L.P_OUT_B), dout_m.sum(0), lambda: rb.colsum_bound(dout_m)[1])
        self.wg(("g", L.P_OUT_W), None, dout_m, hL)
        dhL, bdh = self.gemm32(dout_m, self.pg(L.P_OUT_W).t())
        if D.two:
            dhL = dhL.clone()
            dhL[first] = tok
            inner = bdh

            def bdh():
                b = inner().clone()
                b[first] = btok()
                return b
        self.put("gemm32", "dhL", dhL, bdh)
        dh_key = "dhL"
        if not self.check:
            self.out["dxf_out_run"] = torch.full((D.Mt, D.Lt), STALE, dtype=ar.dtype)
        xf = ar.c(self.inp["xf_out"]).reshape(D.Mt, D.Lt)
        for l in range(D.L - 1, -1, -1):
            hin = "h0" if l == 0 else ("h3", l - 1)
            hffn = ("h2b", l) if D.inter else ("h2", l)
            self.put("copy", ("wT", l), self.wT(l), None)
            dh = self.get(dh_key)
            # ---- FFN ----
            self.sty_bwd(l, D.nsty - 1, dh, ("y3", l), ("a3", l), ("st5", l), L.L_FFN_STY_NORM_W, L.L_FFN_STY_NORM_B, L.L_FFN_STY_OUT_W,
                         L.L_FFN_STY_OUT_B, "ffn")
            dy3 = self.get(("ffn_dy", l))
            self.wg(("gl", l, L.L_FFN_W2), ("gl", l, L.L_FFN_B2), dy3, self.get(("f1", l)))
            W2t, z = self.pl(l, L.L_FFN_W2).t(), self.get(("z1", l))
            acc = dy3 @ W2t.t()
            dz = acc * (gm.dgelu64(z) if acc.dtype == F64 else gm.dgelu64(z.double()).to(acc.dtype))
            self.put("gemm32_dgelu", ("ffn_dz", l), dz, lambda: gm.gemm_bound(dy3, W2t, gm.DGELU, None, z)[1])
            dz = self.get(("ffn_dz", l))
            self.wg(("gl", l, L.L_FFN_W1), ("gl", l, L.L_FFN_B1), dz, self.get(hffn))
            self.put("gemm32", ("ffn_dh", l), *self.gemm32(dz, self.pl(l, L.L_FFN_W1).t(), res=None if mut == "w1_dgrad_residual_dropped" else dh))
            dh = self.get(("ffn_dh", l))
            if mut == "wgrad_reads_dh_after_swap":     # the FFN block's stylization-out gradient, run behind the swap
                self.out[("gl", l, L.L_FFN_STY_OUT_W)] = dh.t() @ self.get(("a3", l))
            if D.inter:
                # ---- person <-> person ----
                self.sty_bwd(l, 2, dh, ("y4", l), ("a4", l), ("st7", l), L.L_INT_STY_NORM_W, L.L_INT_STY_NORM_B, L.L_INT_STY_OUT_W,
                             L.L_INT_STY_OUT_B, "int")
                iqkv = self.get(("iqkv", l))
                self.attn_bwd(l, "int", self.get(("int_dy", l)), iqkv[:, :d], self.get(("Ai", l)), iqkv[:, d:2 * d], iqkv[:, 2 * d:],
                              self.get(("ksti", l)), sb.swap_halves(self.lens()), D.T, swap=True)
                self.wg(("gl", l, L.L_INT_QKV_W), ("gl", l, L.L_INT_QKV_B), self.get(("int_dqkv", l)), self.get(("xn3", l)))
                self.prenorm_bwd(l, "int", ("h2", l), ("st6", l), L.L_INT_NORM_W, L.L_INT_NORM_B, dh, L.L_INT_QKV_W)
                dh = self.get(("int_dh", l))
            # ---- cross attention ----
            self.sty_bwd(l, 1, dh, ("y2", l), ("a2", l), ("st4", l), L.L_CA_STY_NORM_W, L.L_CA_STY_NORM_B, L.L_CA_STY_OUT_W, L.L_CA_STY_OUT_B, "ca")
            kv = self.get(("kv", l))
            if D.full:
                self.full_attention_bwd(l, "ca", self.get(("ca_dy", l)), self.get(("y2", l)), self.get(("qc", l)), kv, self.get(("lse2", l)), D.N, None)
            else:
                self.attn_bwd(l, "ca", self.get(("ca_dy", l)), self.get(("qc", l)), self.get(("Ac", l)), kv[:, :d], kv[:, d:], self.get(("kstc", l)),
                              None, D.N)
            self.wg(("gl", l, L.L_CA_Q_W), ("gl", l, L.L_CA_Q_B), self.get(("ca_dq", l)), self.get(("xn2", l)))
            self.prenorm_bwd(l, "ca", ("h1", l), ("st3", l), L.L_CA_NORM_W, L.L_CA_NORM_B, dh, L.L_CA_Q_W)
            dh = self.get(("ca_dh", l))
            dkv = self.get(("ca_dkv", l))
            if mut == "ca_kv_wgrad_unnormalised_rows":
                xn, e = xf, None
            else:
                xn, e = self.ln_operand(xf, self.get("stt"), self.pl(l, L.L_CA_TNORM_W), self.pl(l, L.L_CA_TNORM_B))
            self.wg(("gl", l, L.L_CA_KV_W), ("gl", l, L.L_CA_KV_B), dkv, xn, e)
            self.put("gemm32", ("ca_dxfn", l), *self.gemm32(dkv, self.pl(l, L.L_CA_KV_W).t()))
            prev = ("ca_dxf_out", l + 1) if l + 1 < D.L else (None if (self.check or mut != "dxf_out_accumulates_at_last_layer") else "dxf_out_run")
            if mut == "dxf_out_last_term_only":
                prev = None
            r = self.lnb(self.get(("ca_dxfn", l)), xf, self.get("stt"), self.pl(l, L.L_CA_TNORM_W), self.pl(l, L.L_CA_TNORM_B), None,
                         None if prev is None else self.get(prev), D.N)
            self.put("ln_bwd", ("ca_dxf_out", l), *r["dx"])
            self.put("ln_bwd", ("gl", l, L.L_CA_TNORM_W), *r["dgamma"])
            self.put("ln_bwd", ("gl", l, L.L_CA_TNORM_B), *r["dbeta"])
            # ---- self attention ----
            self.sty_bwd(l, 0, dh, ("y1", l), ("a1", l), ("st2", l), L.L_SA_STY_NORM_W, L.L_SA_STY_NORM_B, L.L_SA_STY_OUT_W, L.L_SA_STY_OUT_B, "sa")
            qkv = self.get(("qkv", l))
            if D.full:
                self.full_attention_bwd(l, "sa", self.get(("sa_dy", l)), self.get(("y1", l)), qkv[:, :d], qkv[:, d:], self.get(("lse1", l)), D.T,
                                        self.lens())
            else:
                self.attn_bwd(l, "sa", self.get(("sa_dy", l)), qkv[:, :d], self.get(("A1", l)), qkv[:, d:2 * d], qkv[:, 2 * d:],
                              self.get(("kst1", l)), self.lens(), D.T)
            self.wg(("gl", l, L.L_SA_QKV_W), ("gl", l, L.L_SA_QKV_B), self.get(("sa_dqkv", l)), self.get(("xn1", l)))
            self.prenorm_bwd(l, "sa", hin, ("st1", l), L.L_SA_NORM_W, L.L_SA_NORM_B, dh, L.L_SA_QKV_W)
            dh_key = ("sa_dh", l)
        self.put("copy", "dxf_out", self.get(("ca_dxf_out", 0)), None)
        if not self.check:
            self.out["dss"] = self.dss
        # ---- joint_embed + sequence_embedding ----
        dh0 = self.get(dh_key)
        if D.two:
            self.put("copy", "tok0g", dh0[first], None)
            tok0 = self.get("tok0g")
            self.put("colsum", ("g", L.P_JOINT2_B), tok0.sum(0), lambda: rb.colsum_bound(tok0)[1])
            self.wg(("g", L.P_JOINT2_W), None, tok0, ar.c(self.inp["x"])[:, 0, :4])
            if mut != "init_rows_left_in_dh_for_joint_embed":
                dh0 = dh0.masked_fill(first[:, None], 0.0)
        Tpos = D.T - 1 if D.two else D.T
        flat = dh0.reshape(D.B, D.T * d)
        self.put("colsum", ("g", L.P_JOINT_B), dh0.sum(0), lambda: rb.colsum_bound(dh0)[1])
        self.wg(("g", L.P_JOINT_W), None, dh0, x)
        dpos, bpos = flat.sum(0).reshape(D.T, d), (lambda: rb.colsum_bound(flat)[1].reshape(D.T, d))
        if D.two:
            self.put("colsum", "postmp", dpos, bpos)
            dpos, bpos = self.get("postmp")[1:], None
        seq = torch.cat([dpos, torch.zeros(D.num_frames - Tpos, d, dtype=ar.dtype)], 0)
        if mut == "seq_emb_zero_tail_missing":
            seq[Tpos:] = STALE
        if bpos is None or not self.check:
            self.put("copy" if D.two else "colsum", ("g", L.P_SEQ_EMB), seq, None)
        else:
            self.put("colsum", ("g", L.P_SEQ_EMB), seq, lambda: torch.cat([bpos(), torch.zeros(D.num_frames - Tpos, d, dtype=F64)], 0))
        dx, bdx = self.gemm32(dh0, self.pg(L.P_JOINT_W).t())
        if D.two:
            dx4, b4 = self.gemm32(self.get("tok0g"), self.pg(L.P_JOINT2_W).t())
            dx = dx.clone()
            rest = dx[first][:, 4:] if mut != "dx_init_row_all_features" else (self.get("tok0g") @ self.pg(L.P_JOINT_W))[:, 4:]
            dx[first] = torch.cat([dx4, rest], 1)
            inner2 = bdx

            def bdx():
                b = inner2().clone()
                b[first] = torch.cat([b4(), b[first][:, 4:]], 1)
                return b
        self.put("gemm32", "dx", dx, bdx)
        self.time_path_bwd()


def case_inputs(c):
    return sb.case_inputs(c)


masked_mse_grad = sb.masked_mse_grad


# ----------------------------------------------------------------------------------------------------------------------
# reach: which kernels the step runs at each case
# ----------------------------------------------------------------------------------------------------------------------
# The HIG_GEMM_PATH_* / HIG_ATTN_PATH_* counters one step moves on 256 CUs, as sets: `fwd` the text context and the forward, `bwd` the
# backward.  tests/test_gpu_f32_step_contract.py asserts them on the device, tests/test_cpu_f32_step_bounds.py holds the attention
# sets and the dense GEMMs to hig_attn_plan / hig_gemm_plan without one.  SPLIT32 in `fwd` is the few-row split of the three
# conditioning GEMMs (two where one of them is too small to split: narrow); SPLIT32 in `bwd` is a weight gradient over split-R slabs
# (rows520: nine of them, with the column sums parked behind the slabs) or the split d(silu(emb)) GEMM (ss_ld >= 2048: hd128, pairs).
_LIN = {"APPLY_MFMA", "CTX_MFMA", "CTX_PART", "APPLY_BWD_MFMA", "CTX_BWD_MFMA"}
REACH = {
    "small": dict(fwd={"SPLIT32", "TILED32"}, bwd={"TILED32"}, attn=_LIN),
    "narrow": dict(fwd={"SPLIT32", "TILED32"}, bwd={"TILED32"}, attn={"APPLY", "CTX", "APPLY_BWD", "CTX_BWD"}),
    "hd128": dict(fwd={"SPLIT32", "TILED32"}, bwd={"SPLIT32", "TILED32"}, attn=_LIN - {"CTX_MFMA"}),
    "pairs": dict(fwd={"SPLIT32", "TILED32"}, bwd={"SPLIT32", "TILED32"}, attn=_LIN),
    "pairs_nocross": dict(fwd={"SPLIT32", "TILED32"}, bwd={"TILED32"}, attn=_LIN),
    "full": dict(fwd={"SPLIT32", "TILED32"}, bwd={"TILED32"}, attn={"FULL_FWD_MFMA", "FULL_BWD_MFMA"}),
    "full_hd128": dict(fwd={"SPLIT32", "TILED32"}, bwd={"TILED32"}, attn={"FULL_FWD_MFMA", "FULL_BWD_MFMA"}),
    "rows520": dict(fwd={"SPLIT32", "TILED32"}, bwd={"SPLIT32", "TILED32"}, attn={"APPLY_WAVE64", "CTX_PART", "APPLY_BWD_MFMA", "CTX_BWD_MFMA"}),
}
# Paths the BASELINE.md fp32 training shapes (config 1: B2 T60 F150 d128 H8 L4 ff256; config 2: B64 T196 F150 d512 H8 L8 ff1024) plan
# that no case above reaches, with the reason.  The weight-stationary kernels need thousands of rows (2048 and more: a case of that
# size costs minutes of fp64 on the host); they keep their per-element contracts in tests/test_gpu_gemm_contract.py and
# tests/test_gpu_gemm_wsp32.py.
NOT_COVERED = {"gemm": {"WSP32": "the weight-stationary kernel: 2048 rows and more", "TAIL32": "its split tail: the same",
                        "WGRAD_WSP32": "the weight-stationary weight gradient: the same"},
               "attn": {}}
BASELINE_SHAPES = {"config1": dict(B=2, T=60, F=150, d=128, H=8, L=4, ff=256, N=77, Lt=256, two=0, full=0),
                   "config2": dict(B=64, T=196, F=150, d=512, H=8, L=8, ff=1024, N=77, Lt=256, two=0, full=0)}


def attn_calls(c):
    """(entry, B, rows, Tk, scratch) of every attention call of one step at shape c."""
    B, T, N = c["B"], c["T"], c["N"]
    if c["full"]:
        return [("full_fwd", B, T, T, False), ("full_fwd", B, T, N, False), ("full_bwd", B, T, T, False), ("full_bwd", B, T, N, False)]
    calls = [("ctx", B, T, 0, True), ("ctx", B, N, 0, True), ("apply", B, T, 0, False), ("apply_bwd", B, T, 0, True), ("ctx_bwd", B, T, 0, True),
             ("ctx_bwd", B, N, 0, True)]
    if c["two"] == 1:
        calls += [("apply", B // 2, T, 0, False), ("apply_bwd", B // 2, T, 0, True)]
    return calls


def planned_attn(c, chip_cus=256):
    from attn_dispatch_cases import F32 as IO32, plan
    got = set()
    for entry, B, rows, Tk, scratch in attn_calls(c):
        rc, path, _, _ = plan(entry, IO32, B, rows, c["H"], c["d"] // c["H"], Tk=Tk, scratch=scratch, chip_cus=chip_cus)
        assert rc == 0, (entry, rc)
        got.add(path)
    return got


def dense_gemms(c):
    """(I, J, K, epilogue, aux) of the step's GEMMs with dense operands and no operand transform: the ones
    gemm_dispatch_cases.fake_desc can state.  The reduce-slow, SiLU- / LayerNorm-on-load, few-row and split-R forms are reached
    through the entries of csrc/denoiser.hip only and are held by the device counters."""
    M, Mt, d, ff, F, Lt = c["B"] * c["T"], c["B"] * c["N"], c["d"], c["ff"], c["F"], c["Lt"]
    g = [(M, 3 * d, d, gm.BIAS, False), (M, d, d, gm.BIAS_RES, False), (M, d, d, gm.BIAS, False), (M, ff, d, gm.GELU, True), (M, d, ff, gm.BIAS, False),
         (M, F, d, gm.BIAS, False), (M, d, d, gm.NONE, False), (M, ff, d, gm.DGELU, False), (M, d, ff, gm.RES, False), (M, d, 3 * d, gm.NONE, False),
         (Mt, Lt, 2 * d, gm.NONE, False)]
    return g


def planned_gemm(c, chip_cus=256):
    from gemm_dispatch_cases import fake_desc, plan
    got = set()
    for I, J, K, epi, aux in dense_gemms(c):
        rc, mv, _ = plan("ws", fake_desc("ws", I, J, K, epi, aux=aux), chip_cus)
        assert rc == 0, (I, J, K, epi, rc)
        got |= set(mv)
    return got


def assert_reach(name, paths):
    """paths: {'fwd' | 'bwd': ({gemm path: launches}, {attention path: launches})} as the device counted them."""
    got = {"fwd": set(paths["fwd"][0]), "bwd": set(paths["bwd"][0]), "attn": set(paths["fwd"][1]) | set(paths["bwd"][1])}
    assert got == REACH[name], (name, got, REACH[name])
