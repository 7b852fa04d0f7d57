"""The two fp32 encoder training chains -- the text head (hig_text_head_fwd with training = 1, hig_text_head_bwd; csrc/texthead.hip)
and the evaluation classifiers (hig_eval_encoder_fwd_train, hig_eval_encoder_bwd; csrc/evalnet.hip) over the layer both share
(hig_enc_layer_fwd, hig_enc_layer_bwd; csrc/enc_layers.h) -- restated launch by launch, with the element-wise bound of every launch and the
composition mutants, in the form of tests/bf16_step_bounds.py (whose `Walk` supplies the buffers, `put` and the GEMM stages).
Plain torch on the host: tests/test_cpu_enc_step_bounds.py proves without a GPU that the stages compose to oracle.text_head_ref /
oracle.eval_models_ref under autograd, that an fp32 stand-in stays within the bounds and that every mutant breaks one;
tests/test_gpu_enc_step_contract.py holds the device to the same walk.

ONE WALK, THREE USES (see tests/bf16_step_bounds.py): chain EXACT (fp64, the operator itself), chain STANDIN (fp32, `mutant`
switches ONE composition fault on), and `check`: every stage evaluated in fp64 on operands read from a TRACE (the device's own
buffers) and the traced result held to the stage's bound.  Nothing here bounds a whole model.  A stage's bound is the bound its
kernel already has:
  gemm32          test_gpu_gemm_contract.linear_ref: gamma ||X_i|| ||W_j|| + 2^-23 (|bias| + |res|), gamma = 2 K 2^-24.  The
                  positional term of HIG_EPI_BIAS_POS is a residual (pos_shift = 1: none on row 0).  Weight gradients are the same
                  bound over the rows (K = M, whatever the split); row-strided operands change no count.
  gemm32_gelu / gemm32_dgelu   gemm_bound with act_bound of the fp32 GELU / gelu' epilogues; the pre-activation z the linear bound
  xsum            the bias gradient the weight-gradient GEMM sums on the side: M terms in any order, M u sum |dC|
  attn / attn_bwd test_gpu_attn_contract.full_reference / full_bounds with the key-padding mask (y, lse; dQ, dK, dV from the lse and
                  y the call is GIVEN).  delta = sum_l dy y over the head's hd channels: hd products, hd - 1 adds: (hd + 1) u sum |dy y|
  ln / ln_bwd     rowops_bounds.ln_fwd_bound (out, mean, rstd), ln_bwd_bound with the saved statistics (dx, dgamma, dbeta)
  colsum          rowops_bounds.colsum_bound
  gather          bit-equal;   scatter   one fp32 add on the EOT rows (u |result|), every other row bit-equal
NEW STAGES, from their operation count (u = 2^-24; `/` is IEEE division: hipcc's default, the Makefile passes no fast-math flag):
  copy            bit-equal: assemble_kernel (h rows, kpad[b][s] = (t >= length[b]), the [cls] byte 0), unpool_kernel (u2 on a
                  person's token 0, u1 on the others, exact zeros on padded rows), unassemble_kernel (dinit, dmove with exact zeros
                  on the init-pose rows), hig_copy_async (xcat, the feature output), the shifted d(sequence_embedding), zeroed
                  gradients, each layer's incoming d(x2)
  masked_mean     acc = sequential sum of n = 2 len terms: n u sum |t|; one division: |acc err| / n + u |feature|
  pool            pool1 = sequential sum of 2 (len - 1) terms: 2 (len - 1) u sum |t|; pool2 two terms: 2 u sum |t|
  head_scale      g = dft / (2 len): u |g|;  gn = 2 (len - 1) g, an exactly representable integer times the g the kernel holds:
                  u |gn|;  g2 = 2 g: exact
  pad_zero        the rows of padded tokens (t >= length[b]) of every d(.) buffer of the evaluator's backward: exact zeros
                  (include/hig.h: "an exact-zero gradient through every layer")
`MUTANTS` are faults of COMPOSITION -- a stage handed the wrong buffer, row, offset, count or generation of a reused scratch --;
the stages themselves have their own mutants in the modules named above.
"""
import math

import torch

import bf16_step_bounds as sb
import rowops_bounds as rb
import test_gpu_attn_contract as AC        # (full_reference, full_bounds: the module runs nothing on import)
import test_gpu_gemm_contract as gm
from hig_amd import _lib
from oracle import eval_models_ref as R
from oracle import fill
from rowops_bounds import F32, F64, U

EVAL_MUTANTS = ("position_shift_missing", "init_row_not_overwritten", "init_row_features_beyond_four", "emb_indexed_b_p",
                "person2_masked_by_s", "cls_marked_padded", "mean_divided_by_len", "out2_on_person1_only", "out1_bias_weighted_2len",
                "padded_dh_rows_nonzero", "init_rows_left_in_dmove", "seq_emb_not_shifted")
LAYER_MUTANTS = ("dr2_residual_dropped", "dr1_residual_dropped", "in_proj_wgrad_reads_own_x2", "norm1_bwd_given_st2",
                 "dgrad_previous_layer_weights")
TEXT_MUTANTS = ("scatter_at_eot_plus_1", "dxf_out_dropped", "text_ln_bwd_on_layer_L_minus_2", "identity_pre_reads_x0")
MUTANTS = EVAL_MUTANTS + LAYER_MUTANTS + TEXT_MUTANTS
ENC_ONLY = ("mean_divided_by_len", "out2_on_person1_only", "out1_bias_weighted_2len", "padded_dh_rows_nonzero")
STALE = 1.0         # what a stand-in's unwritten buffers hold
EXACT, STANDIN, REF = sb.Ar(F64, False), sb.Ar(F32, False), sb.Ar(F64, False)

# the cases of tests/test_gpu_enc_step_contract.py: the smallest that reach each form.  Every evaluator case has lengths 1, T, one
# above T and an interior one; every text case an EOT at row 0 and at row N - 1.
EVAL_CASES = {
    "hd8": dict(B=4, T=12, F=15, d=64, H=8, ff=128, L=2, num_frames=16, length=(12, 7, 1, 15)),          # VALU attention
    "hd64": dict(B=4, T=33, F=15, d=128, H=2, ff=128, L=2, num_frames=40, length=(33, 17, 1, 40)),       # S = 66 / 67: a second 64-key chunk
    "d512": dict(B=4, T=5, F=15, d=512, H=8, ff=64, L=1, num_frames=8, length=(5, 3, 1, 9)),             # the second column block of pool / head_scale
    "d1024": dict(B=4, T=5, F=15, d=1024, H=8, ff=64, L=1, num_frames=8, length=(5, 3, 1, 9)),           # the second float4 trip; head dim 128
}
TEXT_CASES = {
    "pre": dict(B=3, N=77, W=64, Lt=32, H=4, ff=64, L=2, E=128, eot=(0, 76, 40), pre=1),
    "identity": dict(B=3, N=77, W=128, Lt=128, H=2, ff=128, L=1, E=256, eot=(76, 0, 5), pre=0),          # text_pre_proj = nn.Identity
}
TEXT_VARIANTS = ("all", "no_dxf_out", "no_dxf_proj", "no_dclip")
TL_NAMES = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "norm1.weight",
            "norm1.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm2.weight", "norm2.bias")


class Params:
    """The parameters by the slots of include/hig.h (HIG_EV_* / HIG_T_*, then HIG_TL_* per layer): glob[slot] (None: a slot the
    model lacks), lay[l][slot] fp32 host tensors, gnames / lnames their state-dict names."""

    def __init__(self, named, gnames, prefix, L):
        self.named, self.gnames = named, gnames
        self.lnames = [[prefix % l + s for s in TL_NAMES] for l in range(L)]
        self.glob = [None if n is None else named[n] for n in gnames]
        self.lay = [[named[n] for n in row] for row in self.lnames]

    def oracle_dict(self, dtype=F64):
        return {k: v.to(dtype).clone().requires_grad_(True) for k, v in self.named.items()}


class EDims:
    def __init__(self, c, kind):
        for k in ("B", "T", "F", "d", "H", "ff", "L", "num_frames"):
            setattr(self, k, c[k])
        self.kind, self.cls, self.C = kind, int(kind == "con"), 26 if kind == "enc" else 2
        self.S = self.cls + 2 * self.T
        self.n, self.hd, self.M = self.d, self.d // self.H, self.B * self.S


class TDims:
    def __init__(self, c):
        for k in ("B", "N", "W", "Lt", "H", "ff", "L", "E", "pre"):
            setattr(self, k, c[k])
        self.S, self.n, self.hd, self.M = self.N, self.Lt, self.Lt // self.H, self.B * self.N


def eval_setup(name, kind):
    """(case, dims, params, inputs) of an evaluator case: name-seeded parameters and inputs (oracle/fill.py), d(logits) and
    d(feature) included."""
    c = EVAL_CASES[name]
    D = EDims(c, kind)
    L = _lib
    shapes = R.param_shapes(kind, c["F"], c["d"], c["ff"], c["L"], c["num_frames"])
    named = {k: fill.tensor_for(k, s) for k, s in shapes.items() if not k.startswith(("time_embed", "init_pos"))}
    gn = [None] * L.EV_NGLOBAL
    for slot, nm in ((L.EV_SEQ_EMB, "sequence_embedding"), (L.EV_JOINT1_W, "joint_embed1.weight"), (L.EV_JOINT1_B, "joint_embed1.bias"),
                     (L.EV_JOINT2_W, "joint_embed2.weight"), (L.EV_JOINT2_B, "joint_embed2.bias")):
        gn[slot] = nm
    if kind == "enc":
        for slot, nm in ((L.EV_OUT1_W, "out1.weight"), (L.EV_OUT1_B, "out1.bias"), (L.EV_OUT2_W, "out2.weight"), (L.EV_OUT2_B, "out2.bias"),
                         (L.EV_HEAD_W, "fin_proj.0.weight"), (L.EV_HEAD_B, "fin_proj.0.bias")):
            gn[slot] = nm
    else:
        for slot, nm in ((L.EV_HEAD_W, "cls_output.0.weight"), (L.EV_HEAD_B, "cls_output.0.bias"), (L.EV_CLS_IN, "cls_input")):
            gn[slot] = nm
    P = Params(named, gn, "motionTransEncoder.layers.%d.", c["L"])
    tag = "enc_step.%s.%s." % (name, kind)
    inp = {"x1": fill.tensor_for(tag + "x1", (D.B, D.T, D.F)) * 10.0, "x2": fill.tensor_for(tag + "x2", (D.B, D.T, D.F)) * 10.0,
           "length": torch.tensor(c["length"], dtype=torch.int64), "dlogits": fill.tensor_for(tag + "dlogits", (D.B, D.C)) * 10.0,
           "dfeature": fill.tensor_for(tag + "dfeature", (D.B, D.d)) * 10.0 if kind == "enc" else None}
    return c, D, P, inp


def text_setup(name, variant="all"):
    """(case, dims, params, inputs) of a text head case; variant: which of dxf_out, dxf_proj, dclip is NULL."""
    c = TEXT_CASES[name]
    D = TDims(c)
    L = _lib
    named = {"text_ln.weight": (D.Lt,), "text_ln.bias": (D.Lt,), "text_proj.0.weight": (D.E, D.Lt), "text_proj.0.bias": (D.E,)}
    if D.pre:
        named.update({"text_pre_proj.weight": (D.Lt, D.W), "text_pre_proj.bias": (D.Lt,)})
    pre = "textTransEncoder.layers.%d."
    for l in range(D.L):
        for s, shp in zip(TL_NAMES, ((3 * D.Lt, D.Lt), (3 * D.Lt,), (D.Lt, D.Lt), (D.Lt,), (D.Lt,), (D.Lt,), (D.ff, D.Lt), (D.ff,), (D.Lt, D.ff),
                                     (D.Lt,), (D.Lt,), (D.Lt,))):
            named[pre % l + s] = shp
    named = {k: fill.tensor_for(k, s) for k, s in named.items()}
    gn = [None] * L.T_NGLOBAL
    for slot, nm in ((L.T_LN_W, "text_ln.weight"), (L.T_LN_B, "text_ln.bias"), (L.T_PROJ_W, "text_proj.0.weight"), (L.T_PROJ_B, "text_proj.0.bias")):
        gn[slot] = nm
    if D.pre:
        gn[L.T_PRE_W], gn[L.T_PRE_B] = "text_pre_proj.weight", "text_pre_proj.bias"
    P = Params(named, gn, pre, D.L)
    tag = "enc_step.text.%s." % name
    inp = {"clip_out": fill.tensor_for(tag + "clip", (D.B, D.N, D.W)) * 10.0, "eot": torch.tensor(c["eot"], dtype=torch.int64),
           "dxf_out": None if variant == "no_dxf_out" else fill.tensor_for(tag + "dxf_out", (D.B, D.N, D.Lt)) * 10.0,
           "dxf_proj": None if variant == "no_dxf_proj" else fill.tensor_for(tag + "dxf_proj", (D.B, D.E)) * 10.0,
           "want_dclip": variant != "no_dclip"}
    return c, D, P, inp


# ----------------------------------------------------------------------------------------------------------------------
# full attention with the key-padding mask, in a walk's arithmetic (the chains; the check uses test_gpu_attn_contract)
# ----------------------------------------------------------------------------------------------------------------------
def attn_scores(qkv, kpad, B, S, H, hd):
    n = H * hd
    q, k, v = (qkv[:, i * n:(i + 1) * n].reshape(B, S, H, hd) for i in range(3))
    s = torch.einsum("bnhd,bmhd->bhnm", q, k) / math.sqrt(hd)
    if kpad is not None:
        s = s.masked_fill(kpad[:, None, None, :], float("-inf"))
    return q, k, v, s


def attn_fwd(qkv, kpad, B, S, H, hd):
    """-> y (M, n), lse (B, H, S)."""
    _, _, v, s = attn_scores(qkv, kpad, B, S, H, hd)
    lse = torch.logsumexp(s, -1)
    y = torch.einsum("bhnm,bmhl->bnhl", torch.exp(s - lse[..., None]), v)
    return y.reshape(B * S, H * hd), lse


def attn_bwd(dy, y, qkv, lse, kpad, B, S, H, hd):
    """hig_fullattn_bwd_kpad on what it is given -> dqkv (M, 3 n), delta (B, H, S)."""
    q, k, v, s = attn_scores(qkv, kpad, B, S, H, hd)
    dyh, yh = dy.reshape(B, S, H, hd), y.reshape(B, S, H, hd)
    w = torch.exp(s - lse[..., None])
    delta = (dyh * yh).sum(-1).permute(0, 2, 1)
    dS = w * (torch.einsum("bnhl,bmhl->bhnm", dyh, v) - delta[..., None]) / math.sqrt(hd)
    dq, dk, dv = torch.einsum("bhnm,bmhd->bnhd", dS, k), torch.einsum("bhnm,bnhd->bmhd", dS, q), torch.einsum("bhnm,bnhl->bmhl", w, dyh)
    return torch.cat([t.reshape(B * S, H * hd) for t in (dq, dk, dv)], 1), delta


# ----------------------------------------------------------------------------------------------------------------------
# the walk: the encoder layer both chains share
# ----------------------------------------------------------------------------------------------------------------------
class EncWalk(sb.Walk):
    """sb.Walk's buffers (get / put), parameters (pg / pl) and GEMM stages (gemm32, wgrad16) over an encoder chain.  trace None:
    a chain in arithmetic `ar` (its buffers end up in self.out); else a check of `trace`, self.worst = {stage kind: (largest
    |error| / bound, the buffer that gave it)}."""

    def __init__(self, P, D, inp, ar=REF, trace=None, mutant=None):
        assert mutant is None or (mutant in MUTANTS and trace is None)
        self.P, self.D, self.inp, self.ar, self.src, self.mut = P, D, inp, ar, trace, mutant
        self.check = trace is not None
        self.out, self.worst, self.seen = {}, {}, set()

    def put(self, kind, key, value, bound=None, bf16=False, sel=None):
        self.seen.add(key)          # (a check ends with every buffer of the trace held: seen == the trace's keys)
        super().put(kind, key, value, bound, bf16, sel)

    def run(self):
        self.forward()
        self.backward()
        return self

    def kpad(self):
        return None

    # ---- stages ----
    def ln_fwd(self, kx, kst, x, gamma, beta):
        """hig_layernorm: the rows and the (mean, rstd) pairs it saves."""
        if not self.check:
            y, mu, r = rb.ln_fwd_eval(x, gamma, beta, dtype=self.ar.dtype)
            self.out[kx], self.out[kst] = y, torch.stack([mu, r], 1)
            return
        b = rb.ln_fwd_bound(x, gamma, beta)
        self.put("ln", kx, b["out"][0], lambda: b["out"][1])
        self.put("ln", kst, b["mean"][0], lambda: b["mean"][1], sel=lambda t: t[:, 0])
        self.put("ln", kst, b["rstd"][0], lambda: b["rstd"][1], sel=lambda t: t[:, 1])

    def ln_bwd(self, kdx, kg, kb, da, x, stats, gamma, beta):
        """hig_ln_bwd with the forward's statistics: dx, dgamma, dbeta."""
        if not self.check:
            v = rb.ln_bwd_eval(da, x, stats, gamma, beta, None, None, self.D.S, dtype=self.ar.dtype)
            self.out[kdx], self.out[kg], self.out[kb] = v[0], v[1], v[2]
            return
        b = rb.ln_bwd_bound(da, x, stats, gamma, beta, None, None, self.D.S)
        for key, name in ((kdx, "dx"), (kg, "dgamma"), (kb, "dbeta")):
            self.put("ln_bwd", key, b[name][0], lambda name=name: b[name][1])

    def wg(self, key_w, key_b, dC, act):
        """A weight gradient and the bias gradient its GEMM sums on the side."""
        dW, bW, db, bb_ = self.wgrad16(dC, act)
        self.put("gemm32", key_w, dW, bW)
        self.put("xsum", key_b, db, bb_)

    def colsum(self, key, x, shape=None):
        shape = x.shape[1:] if shape is None else shape
        self.put("colsum", key, x.sum(0).reshape(shape), lambda: rb.colsum_bound(x)[1].reshape(shape))

    def attention(self, l):
        D, kp = self.D, self.kpad()
        qkv = self.get(("qkv", l))
        if not self.check:
            self.out[("att", l)], self.out[("lse", l)] = attn_fwd(qkv, kp, D.B, D.S, D.H, D.hd)
            return
        r = AC.full_reference(qkv[:, :D.n].contiguous(), qkv[:, D.n:].contiguous(), None, D.B, D.S, D.S, D.H, D.hd, None, kp)
        assert r["X"].max().item() <= 80 + math.log(D.S), "logit spread above 80"
        b = AC.full_bounds(r, D.B, D.S, D.S, D.H, D.hd)
        self.put("attn", ("att", l), r["y"].reshape(D.M, D.n), lambda: b["y"].reshape(D.M, D.n))
        self.put("attn", ("lse", l), r["lse"], lambda: b["lse"])

    def attention_bwd(self, l):
        D, kp = self.D, self.kpad()
        qkv, dy, y, lse = self.get(("qkv", l)), self.get(("datt", l)), self.get(("att", l)), self.get(("lse", l))
        if not self.check:
            self.out[("dqkv", l)], self.out[("delta", l)] = attn_bwd(dy, y, qkv, lse, kp, D.B, D.S, D.H, D.hd)
            return
        r = AC.full_reference(qkv[:, :D.n].contiguous(), qkv[:, D.n:].contiguous(), dy.contiguous(), D.B, D.S, D.S, D.H, D.hd, None, kp,
                              lse_in=lse, y_in=y.contiguous())
        b = AC.full_bounds(r, D.B, D.S, D.S, D.H, D.hd)
        for i, name in enumerate(("dQ", "dK", "dV")):
            self.put("attn_bwd", ("dqkv", l), r[name].reshape(D.M, D.n), lambda name=name: b[name].reshape(D.M, D.n),
                     sel=lambda t, i=i: t[:, i * D.n:(i + 1) * D.n])
        t = dy.reshape(D.B, D.S, D.H, D.hd) * y.reshape(D.B, D.S, D.H, D.hd)
        self.put("attn_bwd", ("delta", l), t.sum(-1).permute(0, 2, 1), lambda: (D.hd + 1) * U * t.abs().sum(-1).permute(0, 2, 1))

    def layer_fwd(self, l, xin):
        L = _lib
        self.put("gemm32", ("qkv", l), *self.gemm32(xin, self.pl(l, L.TL_IN_W), self.pl(l, L.TL_IN_B)))
        self.attention(l)
        self.put("gemm32", ("r1", l), *self.gemm32(self.get(("att", l)), self.pl(l, L.TL_OUT_W), self.pl(l, L.TL_OUT_B), xin))
        self.ln_fwd(("x1", l), ("st1", l), self.get(("r1", l)), self.pl(l, L.TL_N1_W), self.pl(l, L.TL_N1_B))
        x1, W1, b1 = self.get(("x1", l)), self.pl(l, L.TL_FF1_W), self.pl(l, L.TL_FF1_B)
        pre = x1 @ W1.t() + b1
        bd = gm.gemm_bound(x1, W1, gm.GELU, b1, None, False, False) if self.check else None
        self.put("gemm32", ("z", l), pre, (lambda: bd[3]) if self.check else None)
        self.put("gemm32_gelu", ("f", l), rb.gelu_eval(pre, dtype=self.ar.dtype), (lambda: bd[1]) if self.check else None)
        self.put("gemm32", ("r2", l), *self.gemm32(self.get(("f", l)), self.pl(l, L.TL_FF2_W), self.pl(l, L.TL_FF2_B), x1))
        self.ln_fwd(("x2", l), ("st2", l), self.get(("r2", l)), self.pl(l, L.TL_N2_W), self.pl(l, L.TL_N2_B))

    def layer_bwd(self, l, xin, own_x2, kout):
        """hig_enc_layer_bwd: from ('dh_in', l) = d(x2) to `kout` = d(xin).  t1 holds dr2, then dr1; t2 d(x1), then d(att)."""
        D, L, mut = self.D, _lib, self.mut
        d = self.get(("dh_in", l))
        self.ln_bwd(("dr2", l), ("gl", l, L.TL_N2_W), ("gl", l, L.TL_N2_B), d, self.get(("r2", l)), self.get(("st2", l)), self.pl(l, L.TL_N2_W),
                    self.pl(l, L.TL_N2_B))
        dr2 = self.get(("dr2", l))
        self.wg(("gl", l, L.TL_FF2_W), ("gl", l, L.TL_FF2_B), dr2, self.get(("f", l)))
        lw = l + 1 if (mut == "dgrad_previous_layer_weights" and l + 1 < D.L) else l
        W2t, z = self.pl(lw, L.TL_FF2_W).t(), self.get(("z", l))
        acc = dr2 @ W2t.t()
        dz = acc * (gm.dgelu64(z) if acc.dtype == F64 else gm.dgelu64(z.double()).to(acc.dtype))
        self.put("gemm32_dgelu", ("dz", l), dz, lambda: gm.gemm_bound(dr2, W2t, gm.DGELU, None, z)[1])
        dz = self.get(("dz", l))
        self.wg(("gl", l, L.TL_FF1_W), ("gl", l, L.TL_FF1_B), dz, self.get(("x1", l)))
        self.put("gemm32", ("dx1", l), *self.gemm32(dz, self.pl(l, L.TL_FF1_W).t(), None, None if mut == "dr2_residual_dropped" else dr2))
        st = self.get(("st2" if mut == "norm1_bwd_given_st2" else "st1", l))
        self.ln_bwd(("dr1", l), ("gl", l, L.TL_N1_W), ("gl", l, L.TL_N1_B), self.get(("dx1", l)), self.get(("r1", l)), st, self.pl(l, L.TL_N1_W),
                    self.pl(l, L.TL_N1_B))
        dr1 = self.get(("dr1", l))
        self.wg(("gl", l, L.TL_OUT_W), ("gl", l, L.TL_OUT_B), dr1, self.get(("att", l)))
        self.put("gemm32", ("datt", l), *self.gemm32(dr1, self.pl(l, L.TL_OUT_W).t()))
        self.attention_bwd(l)
        dqkv = self.get(("dqkv", l))
        self.wg(("gl", l, L.TL_IN_W), ("gl", l, L.TL_IN_B), dqkv, own_x2 if (mut == "in_proj_wgrad_reads_own_x2" and l > 0) else xin)
        self.put("gemm32", kout, *self.gemm32(dqkv, self.pl(l, L.TL_IN_W).t(), None, None if mut == "dr1_residual_dropped" else dr1))

    def layers_bwd(self, x_first):
        """The layers L - 1 .. 0: layer l's d(xin) is layer l - 1's incoming d(x2), the last one 'dh0'."""
        for l in range(self.D.L - 1, -1, -1):
            xin = x_first() if l == 0 else self.get(("x2", l - 1))
            self.layer_bwd(l, xin, self.get(("x2", l)), "dh0" if l == 0 else ("dh_in", l - 1))
            self.after_layer_bwd(l)

    def after_layer_bwd(self, l):
        pass


# ----------------------------------------------------------------------------------------------------------------------
# the text head
# ----------------------------------------------------------------------------------------------------------------------
class TextWalk(EncWalk):
    def clip(self):
        return self.ar.c(self.inp["clip_out"]).reshape(self.D.M, self.D.W)

    def eot_rows(self, shift=0):
        D = self.D
        return torch.arange(D.B) * D.N + (self.inp["eot"] + shift).clamp_max(D.N - 1)

    def forward(self):
        D, L = self.D, _lib
        if D.pre:
            self.put("gemm32", "x0", *self.gemm32(self.clip(), self.pg(L.T_PRE_W), self.pg(L.T_PRE_B)))
        elif not self.check:
            self.out["x0"] = torch.full((D.M, D.Lt), STALE, dtype=self.ar.dtype)         # (never written: the identity reads clip_out)
        for l in range(D.L):
            self.layer_fwd(l, (self.get("x0") if D.pre else self.clip()) if l == 0 else self.get(("x2", l - 1)))
        self.ln_fwd("xf_out", "stf", self.get(("x2", D.L - 1)), self.pg(L.T_LN_W), self.pg(L.T_LN_B))
        self.put("gather", "gath", self.get("xf_out")[self.eot_rows()], None)
        self.put("gemm32", "xf_proj", *self.gemm32(self.get("gath"), self.pg(L.T_PROJ_W), self.pg(L.T_PROJ_B)))

    def backward(self):
        D, L, ar, mut = self.D, _lib, self.ar, self.mut
        dxo, dxp = self.inp["dxf_out"], ar.c(self.inp["dxf_proj"])
        zeros = torch.zeros(D.M, D.Lt, dtype=ar.dtype)
        base = zeros if dxo is None else ar.c(dxo).reshape(D.M, D.Lt)
        if dxp is not None:
            self.colsum(("g", L.T_PROJ_B), dxp)
            self.put("gemm32", ("g", L.T_PROJ_W), *self.gemm32(dxp.t(), self.get("gath").t()))
            self.put("gemm32", "dgath", *self.gemm32(dxp, self.pg(L.T_PROJ_W).t()))
            rows = self.eot_rows(1 if mut == "scatter_at_eot_plus_1" else 0)
            tot = (zeros if mut == "dxf_out_dropped" else base).clone()
            tot[rows] += self.get("dgath")

            def bound():
                b = torch.zeros(D.M, D.Lt, dtype=F64)
                b[rows] = U * tot[rows].abs()
                return b
            self.put("scatter", "dxf_total", tot, bound)
        else:
            self.put("copy", ("g", L.T_PROJ_B), torch.zeros(D.E, dtype=ar.dtype), None)
            self.put("copy", ("g", L.T_PROJ_W), torch.zeros(D.E, D.Lt, dtype=ar.dtype), None)
            self.put("copy", "dxf_total", base, None)
        lx = D.L - 2 if (mut == "text_ln_bwd_on_layer_L_minus_2" and D.L > 1) else D.L - 1
        self.ln_bwd(("dh_in", D.L - 1), ("g", L.T_LN_W), ("g", L.T_LN_B), self.get("dxf_total"), self.get(("x2", lx)), self.get("stf"),
                    self.pg(L.T_LN_W), self.pg(L.T_LN_B))
        self.layers_bwd(lambda: self.get("x0") if (D.pre or mut == "identity_pre_reads_x0") else self.clip())
        d0 = self.get("dh0")
        if D.pre:
            self.wg(("g", L.T_PRE_W), ("g", L.T_PRE_B), d0, self.clip())
            if self.inp["want_dclip"]:
                self.put("gemm32", "dclip", *self.gemm32(d0, self.pg(L.T_PRE_W).t()))
        elif self.inp["want_dclip"]:
            self.put("copy", "dclip", d0, None)


# ----------------------------------------------------------------------------------------------------------------------
# the evaluation classifiers
# ----------------------------------------------------------------------------------------------------------------------
class EvalWalk(EncWalk):
    def kpad(self):
        return self.get("kpad") > 0.5

    def lens(self):
        return self.inp["length"].clamp(0, self.D.T)

    def tok0(self, first_only=False):
        """Rows of h that hold a person's init-pose token (the MotionEncoder: S = 2 T)."""
        s = torch.arange(self.D.M) % self.D.S
        return s == 0 if first_only else s % self.D.T == 0

    def forward(self):
        D, L, ar, mut = self.D, _lib, self.ar, self.mut
        B, T, d = D.B, D.T, D.d
        # joint_embed1 + sequence_embedding[t - 1] on every row, then the init-pose rows (t = 0) overwritten by joint_embed2 of
        # their first four features
        tpos = torch.arange(T) - (0 if mut == "position_shift_missing" else 1)
        pos = (self.pg(L.EV_SEQ_EMB)[tpos.clamp_min(0)] * (tpos >= 0).to(ar.dtype)[:, None]).repeat(B, 1)
        first = torch.arange(B * T) % T == 0
        vals, bnds = [], []
        for p in range(2):
            x = ar.c(self.inp["x%d" % (p + 1)])
            v, b1 = self.gemm32(x.reshape(B * T, D.F), self.pg(L.EV_JOINT1_W), self.pg(L.EV_JOINT1_B), pos)
            v0, b0 = self.gemm32(x[:, 0, 4:8] if mut == "init_row_features_beyond_four" else x[:, 0, :4], self.pg(L.EV_JOINT2_W), self.pg(L.EV_JOINT2_B))
            if mut != "init_row_not_overwritten":
                v = v.clone()
                v[first] = v0
            vals.append(v)
            bnds.append((b1, b0))

        def bound():
            out = []
            for b1, b0 in bnds:
                b = b1().clone()
                b[first] = b0()
                out.append(b)
            return torch.cat(out, 0)
        self.put("gemm32", "emb", torch.cat(vals, 0), bound)
        # assemble_kernel: [cls,] person 1, person 2 on the token axis; the key-padding bytes
        emb = self.get("emb")
        emb = emb.reshape(B, 2, T, d).transpose(0, 1) if mut == "emb_indexed_b_p" else emb.reshape(2, B, T, d)
        parts = [emb[0], emb[1]]
        t = torch.arange(T)
        length = self.inp["length"]
        pad1 = t[None] >= length[:, None]
        pad2 = (T + t)[None] >= length[:, None] if mut == "person2_masked_by_s" else pad1
        pads = [pad1, pad2]
        if D.cls:
            parts.insert(0, self.pg(L.EV_CLS_IN).reshape(1, 1, d).expand(B, 1, d))
            pads.insert(0, torch.full((B, 1), mut == "cls_marked_padded"))
        self.put("copy", "h", torch.cat(parts, 1).reshape(D.M, d), None)
        self.put("copy", "kpad", torch.cat(pads, 1).to(ar.dtype), None)
        for l in range(D.L):
            self.layer_fwd(l, self.get("h") if l == 0 else self.get(("x2", l - 1)))
        xL = self.get(("x2", D.L - 1))
        if D.cls:
            self.put("gemm32", "logits", *self.gemm32(xL.reshape(B, D.S, d)[:, 0], self.pg(L.EV_HEAD_W), self.pg(L.EV_HEAD_B)))
            return
        # out1 on every row, out2 over the two init-pose rows of each pair; the masked mean; fin_proj
        o, bo = self.gemm32(xL, self.pg(L.EV_OUT1_W), self.pg(L.EV_OUT1_B))
        sel, true_sel = self.tok0(mut == "out2_on_person1_only"), self.tok0()
        o = o.clone()
        o[sel] = self.gemm32(xL[sel], self.pg(L.EV_OUT2_W), self.pg(L.EV_OUT2_B))[0]

        def bound_o():
            b = bo().clone()
            b[true_sel] = self.gemm32(xL[true_sel], self.pg(L.EV_OUT2_W), self.pg(L.EV_OUT2_B))[1]()
            return b
        self.put("gemm32", "o", o, bound_o)
        ob, ln = self.get("o").reshape(B, 2, T, d), self.lens()
        m = (t[None] < ln[:, None]).to(ar.dtype)[:, None, :, None]
        cnt = (ln if mut == "mean_divided_by_len" else 2 * ln).to(ar.dtype)[:, None]
        feat = (ob * m).sum((1, 2)) / cnt
        self.put("masked_mean", "feat", feat, lambda: (2 * ln)[:, None] * U * (ob.abs() * m).sum((1, 2)) / cnt + U * feat.abs())
        self.put("gemm32", "logits", *self.gemm32(self.get("feat"), self.pg(L.EV_HEAD_W), self.pg(L.EV_HEAD_B)))
        self.put("copy", "feature", self.get("feat"), None)

    def pad_rows(self):
        """Rows of an (M, .) buffer that belong to padded tokens."""
        return (self.get("kpad") > 0.5).reshape(-1)

    def pad_zero(self, key):
        if self.check:
            pr = self.pad_rows()
            z = self.src[key][pr]
            self.put("pad_zero", key, torch.zeros_like(z, dtype=F64), None, sel=lambda t: t[pr])

    def after_layer_bwd(self, l):
        for k in ("dh_in", "dr2", "dz", "dx1", "dr1", "datt", "dqkv"):
            self.pad_zero((k, l))

    def backward(self):
        D, L, ar, mut = self.D, _lib, self.ar, self.mut
        B, T, d, S = D.B, D.T, D.d, D.S
        dl, dfe = ar.c(self.inp["dlogits"]), ar.c(self.inp["dfeature"])
        xL = self.get(("x2", D.L - 1))
        self.colsum(("g", L.EV_HEAD_B), dl)
        if D.cls:
            self.put("gemm32", ("g", L.EV_HEAD_W), *self.gemm32(dl.t(), xL.reshape(B, S, d)[:, 0].t()))
            v, bv = self.gemm32(dl, self.pg(L.EV_HEAD_W).t())
            cls_rows = torch.arange(D.M) % S == 0
            dh = torch.zeros(D.M, d, dtype=ar.dtype)
            dh[cls_rows] = v

            def bound():
                b = torch.zeros(D.M, d, dtype=F64)
                b[cls_rows] = bv()
                return b
            self.put("gemm32", "dh_L", dh, bound)
        else:
            ln = self.lens()
            self.put("gemm32", ("g", L.EV_HEAD_W), *self.gemm32(dl.t(), self.get("feat").t()))
            self.put("gemm32", "dft", *self.gemm32(dl, self.pg(L.EV_HEAD_W).t(), None, dfe))
            # head_scale_kernel: g = d(feature) / (2 len), gn = 2 (len - 1) g, g2 = 2 g
            g = self.get("dft") / (2 * ln).to(ar.dtype)[:, None]
            self.put("head_scale", "g", g, lambda: U * g.abs())
            g = self.get("g")
            gn = (2 * ln if mut == "out1_bias_weighted_2len" else 2 * (ln - 1)).to(ar.dtype)[:, None] * g
            self.put("head_scale", "gn", gn, lambda: U * gn.abs())
            self.put("head_scale", "g2", 2 * g, None)
            # pool_kernel: pool1 = sum of h over the valid tokens t >= 1 of both persons, pool2 = h of the two init-pose tokens
            hb, t = xL.reshape(B, 2, T, d), torch.arange(T)
            m1 = ((t[None] >= 1) & (t[None] < ln[:, None])).to(ar.dtype)[:, None, :, None]
            self.put("pool", "pool1", (hb * m1).sum((1, 2)), lambda: (2 * (ln - 1))[:, None] * U * (hb.abs() * m1).sum((1, 2)))
            self.put("pool", "pool2", hb[:, 0, 0] + hb[:, 1, 0], lambda: 2 * U * (hb[:, 0, 0].abs() + hb[:, 1, 0].abs()))
            self.put("gemm32", ("g", L.EV_OUT1_W), *self.gemm32(g.t(), self.get("pool1").t()))
            self.put("gemm32", ("g", L.EV_OUT2_W), *self.gemm32(g.t(), self.get("pool2").t()))
            self.colsum(("g", L.EV_OUT1_B), self.get("gn"))
            self.colsum(("g", L.EV_OUT2_B), self.get("g2"))
            self.put("gemm32", "u1", *self.gemm32(g, self.pg(L.EV_OUT1_W).t()))
            self.put("gemm32", "u2", *self.gemm32(g, self.pg(L.EV_OUT2_W).t()))
            # unpool_kernel: u2 on a valid init-pose token, u1 on any other valid token, exact zeros on a padded one
            u1, u2 = self.get("u1"), self.get("u2")
            dh = u1[:, None, None, :].expand(B, 2, T, d).clone()
            dh[:, :, 0] = u2[:, None]
            if mut != "padded_dh_rows_nonzero":
                dh = dh * (t[None] < ln[:, None]).to(ar.dtype)[:, None, :, None]
            self.put("copy", "dh_L", dh.reshape(D.M, d), None)
        self.pad_zero("dh_L")
        self.put("copy", ("dh_in", D.L - 1), self.get("dh_L"), None)
        self.layers_bwd(lambda: self.get("h"))
        self.pad_zero("dh0")
        # ---- embedding ----
        dh0 = self.get("dh0").reshape(B, S, d)
        if D.cls:
            self.colsum(("g", L.EV_CLS_IN), dh0[:, 0], (1, 1, d))
        per = dh0[:, D.cls:].reshape(B, 2, T, d).transpose(0, 1)          # unassemble_kernel: [person][b][t]
        dmove = per.clone()
        if mut != "init_rows_left_in_dmove":
            dmove[:, :, 0] = 0
        self.put("copy", "dinit", per[:, :, 0].reshape(2 * B, d), None)
        self.put("copy", "dmove", dmove.reshape(2 * B * T, d), None)
        self.put("copy", "xcat", torch.cat([ar.c(self.inp["x1"]).reshape(B * T, D.F), ar.c(self.inp["x2"]).reshape(B * T, D.F)], 0), None)
        dinit, dmove, xcat = self.get("dinit"), self.get("dmove"), self.get("xcat")
        self.colsum(("g", L.EV_JOINT2_B), dinit)
        self.put("gemm32", ("g", L.EV_JOINT2_W), *self.gemm32(dinit.t(), xcat.reshape(2 * B, T * D.F)[:, :4].t()))
        self.colsum(("g", L.EV_JOINT1_B), dmove)
        self.put("gemm32", ("g", L.EV_JOINT1_W), *self.gemm32(dmove.t(), xcat.t()))
        # d(sequence_embedding)[t - 1] = the column sums of dmove viewed as (2 B, T d), row 0 dropped
        self.colsum("postmp", dmove.reshape(2 * B, T * d), (T, d))
        pm = self.get("postmp")
        self.put("copy", ("g", L.EV_SEQ_EMB), pm[:T - 1] if mut == "seq_emb_not_shifted" else pm[1:], None)
