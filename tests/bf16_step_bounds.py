"""The bf16-storage training step (hig_text_context_bf16_train, hig_denoiser_fwd_bf16_train, hig_denoiser_bwd_bf16[_hooked];
csrc/denoiser.hip) restated launch by launch, with the element-wise bound of every launch and the composition mutants.  Plain
torch on the host: tests/test_cpu_bf16_step_bounds.py proves without a GPU that the stages compose to the model, that an fp32
stand-in of the step stays within the bounds and that every mutant breaks one; tests/test_gpu_bf16_step_contract.py holds the
device to the same walk.

ONE WALK, THREE USES.  `Walk` goes through the launches of the three entries in their order.  Every launch is a STAGE: a
function of the buffers the launch reads that returns the launch's result before the rounding of its storage type and, when
asked, the bound of that result.  What the walk does with a stage depends on where its operands come from:
  chain, EXACT    (fp64, no rounding anywhere, the master weights): the stages feed each other; the result is the operator
                  itself -- the CPU test holds it to oracle.denoiser_ref / oracle.interaction_ref and to torch autograd of it.
                  This is what lets a stage-wise check say that the stages form the model.
  chain, STANDIN  (fp32, bf16 roundings at every buffer and at the kernels' stated rounding points, the bf16 weight shadow):
                  a stand-in for the device; `mutant` switches ONE composition fault on.
  check           the operands of every stage are read from a TRACE (the device's buffers, or a stand-in's): "teacher
                  forcing".  The stage is evaluated in fp64 on those operands and the traced result is held to the stage's
                  bound; the walk records the largest |error| / bound per stage kind.
Nothing here bounds the whole model.  A stage's bound is the bound its kernel already has:
  ln / ln_sty     rowops_bounds.ln_fwd_bound (silu G = 4), bound16
  ln_bwd          rowops_bounds.ln_bwd_bound(bf16=True): dx (bound16 for bf16 rows), dgamma, dbeta, dscale, dshift
  gemm16          test_gpu_gemm_contract.gemm_bound: gamma ||X_i|| ||W_j|| + 2^-23 (|bias| + |res|), gamma = 2 K 2^-24, with
                  act_bound for the GELU / gelu' epilogues; bound16 for a bf16 C without an activation
  wgrad16         the same linear bound over the rows (K = M); the bias gradient a sum of M terms in any order: M u sum |dC|
  gemm32          the linear bound on fp32 operands.  Where the kernel applies SiLU to an operand as it loads it (hig_silu:
                  the exponential (2 + 2.5 |z|)(1 - sigma), the add and the division: 3) the operand's own error e_s =
                  |silu| ((2 + 2.5 |z|)(1 - sigma) + 3) u reaches the sum through Cauchy-Schwarz: + ||e_s|| ||w_j||.
  ctx             linattn16_bounds.ctx_bounds tier 2 (plan.ctx_mm16), else g_A u MA of test_gpu_attn_contract.py
  apply           linattn16_bounds.apply_bounds tier 2 for the fused front (y and a), else (g_y u + 2 u16) My, bound16
  apply_bwd / ctx_bwd   the bf16-row backward terms of test_gpu_attn_contract.py: (g u + 2 u16) M, bound16 on the rows.  The
                  column term of dK is stated as the kernel computes it, sum_l A[c][l] dA[c][l] from the A it is GIVEN
                  (csrc/linattn.hip, "needs no pass over the rows"), and the key weights from the kstat it is given: a
                  teacher-forced reference must use the device's own A and kstat there.
  gelu            act_bound of the bf16 GELU: one bf16 ulp, and 4.1e-11 |z| beyond |z| = 6.5 (include/hig.h);   colsum   rowops_bounds.colsum_bound;   temb   boundary_bounds.temb_bound
  dsilu           out = a silu'(z), silu' = s (1 + z (1 - s)), s = 1 / (1 + __expf(-z)) (hig_dsilu): the e_D of
                  rowops_bounds with e_w = 0 and G' = 2:  |a| e_D + u |out|
  joint           h0: hig_joint_embed_bf16 (x and W rounded to bf16, the reduce range padded with zeros to Fp: the linear bound with
                  K = Fp, + 2^-23 (|bias| + |pos|)) or, where d % 128 != 0, the fp32 GEMM on the master weight; bound16.  The
                  init-pose rows of the two-person model are a cast of the fp32 rows `tok0`: fp32 bound 0.
  edge            d(h_L): the bf16 GEMM over Fp on the rounded d(out) (plan.edge16) or the fp32 GEMM on the master weight, the
                  init-pose rows through out2 in fp32; bound16
  copy            bit-equal (the shifted d(sequence_embedding), its zero tail, dxf_proj, the init-pose rows, each layer's incoming dh)
What a mutant is: `MUTANTS` are faults of COMPOSITION -- a stage handed the wrong buffer, slice, offset or length -- switched on in a
chain; the stages themselves have their own mutants in the bounds modules named above.
"""
import torch

import boundary_bounds as bb
import linattn16_bounds as lb
import rowops_bounds as rb
import test_gpu_gemm_contract as gm         # (gemm_bound, linear_ref: the module runs nothing on import)
from hig_amd import _lib
from linattn16_bounds import FLOOR, U16
from rowops_bounds import F32, F64, U
from test_gpu_attn_contract import lin_gammas

MUTANTS = ("sty_reads_next_block_slice", "b0_offset_dropped", "contexts_not_swapped", "partner_lengths_not_swapped",
           "position_shift_missing", "sty_out_residual_from_layer_input", "ragged_context_one_frame_early",
           "ffn_f_from_rounded_z", "wgrad_reads_dh_after_swap", "w1_dgrad_residual_dropped", "ln_bwd_res_dropped_at_prenorm",
           "dxf_out_last_term_only", "dxf_out_accumulates_at_last_layer", "dgrad_previous_layer_weights",
           "wgrad_pad_rows_nonzero", "seq_emb_zero_tail_missing", "w_emb_rows_from_wrong_layer")
TWO_PERSON_MUTANTS = ("b0_offset_dropped", "contexts_not_swapped", "partner_lengths_not_swapped", "position_shift_missing")
STALE = 1.0         # what a stand-in's result buffers hold before the step (a mutant that leaves one unwritten shows it)

# the cases of tests/test_gpu_bf16_step_contract.py (B is the model's batch: 2 pairs in the two-person case)
CASES = {
    "small": dict(B=2, T=33, F=12, d=128, H=2, L=2, ff=96, N=77, Lt=32, num_frames=40, lengths=(33, 5), t=(7, 650), two=0),
    "hd128": dict(B=3, T=75, F=150, d=256, H=2, L=2, ff=512, N=77, Lt=64, num_frames=80, lengths=(75, 40, 1), t=(0, 999, 313), two=0),
    "d192": dict(B=2, T=33, F=12, d=192, H=3, L=2, ff=96, N=77, Lt=32, num_frames=40, lengths=(33, 5), t=(7, 650), two=0),
    "pairs": dict(B=4, T=21, F=12, d=128, H=2, L=2, ff=96, N=77, Lt=32, num_frames=40, lengths=(21, 9, 13, 21), t=(7, 650, 3, 999), two=1),
    "wsp16": dict(B=11, T=196, F=150, d=512, H=8, L=1, ff=1024, N=77, Lt=256, num_frames=196,
                  lengths=(196, 77, 196, 1, 120, 196, 50, 196, 33, 195, 64), t=(0, 999, 500, 250, 7, 650, 313, 900, 1, 42, 777), two=0),
    # the smallest shape at which the plan fuses the attention front (H in {4, 8}) and runs the F-wide edges on the bf16 matrix
    # cores (hig_edge16_layout must fit into M d floats: M >= 93 at d = 256, Fp = 32): neither happens at the four small cases above
    "fused": dict(B=2, T=49, F=12, d=256, H=4, L=2, ff=96, N=77, Lt=32, num_frames=56, lengths=(49, 17), t=(7, 650), two=0),
}
# what hig_denoiser_plan / hig_gemm_bf16_plan choose at each case by default (256 CUs): (joint_embed kernel, WSP16 FFN, fused
# front, bf16 context build, bf16 F-wide edge)
REACH = {"small": (True, False, False, True, False), "hd128": (True, False, False, True, False), "d192": (False, False, False, True, False),
         "pairs": (True, False, False, True, False), "wsp16": (True, True, True, True, True), "fused": (True, False, True, True, True)}


class Ar:
    """The arithmetic of a walk: dtype, and whether buffers and the kernels' rounding points round to bf16.  `emulate`: also
    round where a kernel's contract is stated against the unrounded definition (the stand-in does, a reference does not)."""

    def __init__(self, dtype, rounding, emulate=False):
        self.dtype, self.rounding, self.emulate = dtype, rounding, emulate

    def c(self, x):
        return None if x is None else x.to(self.dtype)

    def r16(self, x):
        return lb.rnd16(x) if self.rounding else x


EXACT, STANDIN, REF = Ar(F64, False), Ar(F32, True, True), Ar(F64, True)


class Dims:
    def __init__(self, c):
        for k in ("B", "T", "F", "d", "H", "L", "ff", "N", "Lt", "num_frames", "two"):
            setattr(self, k, c[k])
        self.hd, self.E, self.M, self.Mt = self.d // self.H, 4 * self.d, self.B * self.T, self.B * self.N
        self.nsty = 4 if self.two else 3
        self.ss_ld = self.nsty * self.L * 2 * self.d
        self.Fp = (self.F + 31) // 32 * 32


class Params:
    """The parameters by the slots of include/hig.h (HIG_P_*, HIG_L_*), as the flat buffer groups them: glob[slot],
    lay[l][slot] fp32 host tensors; `names` the state-dict names of each group, in order."""

    def __init__(self, model):
        from hig_amd.models.transformer import _core_param_order
        name_of = {id(p): n for n, p in model.named_parameters()}
        glob, layers = _core_param_order(model)

        def group(g):
            return (torch.cat([p.detach().float().cpu() for p in g], 0) if g else None), [name_of[id(p)] for p in g]

        self.glob, self.gnames = zip(*[group(g) for g in glob])
        self.lay, self.lnames = [], []
        for lay in layers:
            t, n = zip(*[group(g) for g in lay])
            self.lay.append(t)
            self.lnames.append(n)

    def oracle_dict(self, dtype=F64):
        """{state-dict name: leaf tensor} for the oracles, split out of the groups."""
        out = {}
        for t, names in list(zip(self.glob, self.gnames)) + [z for l in range(len(self.lay)) for z in zip(self.lay[l], self.lnames[l])]:
            if t is not None:
                for name, part in zip(names, t.chunk(len(names), 0)):
                    out[name] = part.to(dtype).clone().requires_grad_(True)
        return out

    def grouped(self, by_name):
        """{name: tensor} (e.g. the oracle's gradients) -> {('g', slot) | ('gl', l, slot): tensor} in the groups' layout."""
        out = {}
        for s, names in enumerate(self.gnames):
            if names:
                out[("g", s)] = torch.cat([by_name[n] for n in names], 0)
        for l in range(len(self.lay)):
            for s, names in enumerate(self.lnames[l]):
                if names:
                    out[("gl", l, s)] = torch.cat([by_name[n] for n in names], 0)
        return out


def silu(x):
    return x * torch.sigmoid(x)


def dsilu(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def silu_operand_error(z):
    """e_s of the module docstring for hig_silu(z), z fp64."""
    sg = torch.sigmoid(z)
    return silu(z).abs() * ((2 + 2.5 * z.abs()) * (1 - sg) + 3) * U


def dsilu_bound(a, z):
    """|a| e_D + u |a silu'(z)| (module docstring)."""
    s = torch.sigmoid(z)
    eps_s = ((2 + 2.5 * z.abs()) * (1 - s) + 2) * U
    D = dsilu(z)
    e_D = s * (z.abs() * (eps_s * s + 2 * U * (1 - s)) + U * (1 + z * (1 - s)).abs()) + (eps_s + U) * D.abs()
    return a.abs() * e_D + U * (a * D).abs()


def ss6(ss, off, d):
    """The (B, 2 d) slice [scale | shift] at column `off` of the modulation table, in the layout rowops_bounds and
    linattn16_bounds index (scale at column 2 d, shift at 3 d)."""
    return torch.cat([torch.zeros(ss.shape[0], 2 * d, dtype=ss.dtype), ss[:, off:off + 2 * d]], 1)


def heads(x, B, rows, H, hd):
    return x.reshape(B, rows, H, hd)


def swap_halves(x):
    h = x.shape[0] // 2
    return torch.cat([x[h:], x[:h]], 0)


# ----------------------------------------------------------------------------------------------------------------------
# the attention backward with bf16 rows (hig_linattn_apply_bwd_bf16, hig_linattn_ctx_bwd_bf16)
# ----------------------------------------------------------------------------------------------------------------------
def apply_bwd(dy, q, A, want_bound, u16=U16):
    """dy, q (B, T, H, hd), A (B, H, hd, hd) [c][l] -> dq like q, dA like A, and their fp32 bounds (u16 = 0: the fp32 rows of
    hig_linattn_apply_bwd, tests/f32_step_bounds.py)."""
    p = torch.softmax(q, -1)
    t = torch.einsum("bnhl,bhcl->bnhc", dy, A)
    dq = p * (t - (p * t).sum(-1, keepdim=True))
    dA = torch.einsum("bnhc,bnhl->bhcl", p, dy)
    if not want_bound:
        return dq, dA, None, None
    T, hd = q.shape[1], q.shape[3]
    Xq = (q.amax(-1) - q.amin(-1)).max().item()
    assert Xq <= 80
    g = lin_gammas(T, hd, Xq, 0.0)
    Tm = torch.einsum("bnhl,bhcl->bnhc", dy.abs(), A.abs())
    MdQ = p * (Tm + (p * Tm).sum(-1, keepdim=True))
    MdA = torch.einsum("bnhc,bnhl->bhcl", p, dy.abs())
    return dq, dA, (g["dQ"] * U + 2 * u16) * MdQ + FLOOR, (g["dA"] * U + 2 * u16) * MdA + FLOOR


def ctx_bwd(dA, A, K, V, kst, lens, want_bound, u16=U16):
    """dA, A (B, H, hd, hd); K, V (B, T, H, hd); kst (B, H, hd, 2) = (column maximum, denominator) as the forward left them;
    -> dK, dV like K (exact zeros at and beyond the length) and their fp32 bounds."""
    B, T, H, hd = K.shape
    _, live = lb.live_rows(lens, B, T, K.device)
    lm = live[:, :, None, None]
    x = (K - kst[..., 0][:, None]).masked_fill(~lm, 0.0)
    k = (torch.exp(x) / kst[..., 1][:, None]).masked_fill(~lm, 0.0)
    v = V.masked_fill(~lm, 0.0)
    dV = torch.einsum("bnhc,bhcl->bnhl", k, dA) * lm
    s = torch.einsum("bnhl,bhcl->bnhc", v, dA)
    col = (A * dA).sum(-1)[:, None]
    dK = k * (s - col)
    if not want_bound:
        return dK, dV, None, None
    Xk = x.abs().max().item()
    assert Xk <= 80
    g = lin_gammas(T, hd, 0.0, Xk)
    Sm = torch.einsum("bnhl,bhcl->bnhc", v.abs(), dA.abs())
    MdK = k * (Sm + (A.abs() * dA.abs()).sum(-1)[:, None])
    MdV = torch.einsum("bnhc,bhcl->bnhl", k, dA.abs()) * lm
    return dK, dV, (g["dK"] * U + 2 * u16) * MdK + FLOOR, (g["dV"] * U + 2 * u16) * MdV + FLOOR


# ----------------------------------------------------------------------------------------------------------------------
# the walk
# ----------------------------------------------------------------------------------------------------------------------
class Walk:
    """See the module docstring.  trace None: a chain in arithmetic `ar` (its buffers end up in self.out); else a check of
    `trace` (ar is REF), self.worst = {stage kind: (largest |error| / bound, the buffer that gave it)}.
    forms: joint_kernel, ffn_wsp16, fuse_front, ctx_mm16, edge16 (booleans: the forms the call took)."""
    u16 = U16           # what a product on bf16 rows adds to the attention backward's bounds (0 in the fp32 walk that subclasses this)

    def __init__(self, P, D, inp, forms, ar=REF, trace=None, mutant=None, te=None):
        assert mutant is None or (mutant in MUTANTS and trace is None)
        self.P, self.D, self.inp, self.forms, self.ar, self.src, self.mut, self.te = P, D, inp, forms, ar, trace, mutant, te
        self.check = trace is not None
        self.out, self.worst = {}, {}

    # ---- buffers ----
    def get(self, key):
        return (self.src if self.check else self.out)[key].to(self.ar.dtype)

    def put(self, kind, key, value, bound=None, bf16=False, sel=None):
        """A stage's result: stored (chain), or held against the trace (check).  bound: a callable giving the fp32 bound
        (None: bit-equal)."""
        if not self.check:
            self.out[key] = self.ar.r16(value) if bf16 else value
            return
        got = self.src[key] if sel is None else sel(self.src[key])
        assert got.shape == value.shape, (key, got.shape, value.shape)
        b32 = torch.zeros_like(value) if bound is None else bound() + torch.zeros_like(value)
        r = rb.ratio(got, value, rb.bound16(value, b32) if bf16 else b32)
        if r >= self.worst.get(kind, (-1.0, None))[0]:
            self.worst[kind] = (r, key)

    def pg(self, slot):
        return self.ar.c(self.P.glob[slot])

    def pl(self, l, slot):
        return self.ar.c(self.P.lay[l][slot])

    def w16(self, W):
        return self.ar.r16(W)

    # ---- primitives: each returns (value, bound callable) ----
    def gemm16(self, X, W, epi=None, bias=None, res=None):
        """hig_gemm_bf16: X (I, K), W (J, K) bf16 values; epi None | 'res' | 'dgelu' (res = z)."""
        acc = X @ W.t()
        if epi == "dgelu":
            v = acc * gm.dgelu64(res) if acc.dtype == F64 else acc * gm.dgelu64(res.double()).to(acc.dtype)
            # (the contract counts a whole bf16 ulp for the output; bound16 adds half of it, the other half stays in b32)
            return v, lambda: gm.gemm_bound(X, W, gm.DGELU, None, res, True)[1] - 0.5 * rb.ulp16(v)
        if bias is not None:
            acc = acc + bias
        if res is not None:
            acc = acc + res
        e = gm.BIAS_RES if (bias is not None and res is not None) else gm.BIAS if bias is not None else gm.RES if res is not None else gm.NONE
        return acc, lambda: gm.gemm_bound(X, W, e, bias, res)[1]

    def wgrad16(self, dC, act):
        """hig_wgrad16: dW = dC^T act (fp32), db = column sums of dC."""
        rows = dC.shape[0]
        return (dC.t() @ act, lambda: gm.linear_ref(dC.t(), act.t(), gm.NONE, None, None)[1],
                dC.sum(0), lambda: rows * U * dC.abs().sum(0))

    def gemm32(self, X, W, bias=None, res=None, silu_x=False, silu_w=False):
        """The fp32 kernels: X (I, K) W (J, K)^T; silu_x / silu_w: SiLU applied to that operand as it is loaded."""
        Xs, Ws = (silu(X) if silu_x else X), (silu(W) if silu_w else W)
        v = Xs @ Ws.t()
        if bias is not None:
            v = v + bias
        if res is not None:
            v = v + res

        def bound():
            e = gm.BIAS_RES if (bias is not None and res is not None) else gm.BIAS if bias is not None else gm.RES if res is not None else gm.NONE
            b = gm.linear_ref(Xs, Ws, e, bias, res)[1]
            if silu_x:
                b = b + torch.outer(silu_operand_error(X).norm(dim=1), Ws.norm(dim=1))
            if silu_w:
                b = b + torch.outer(Xs.norm(dim=1), silu_operand_error(W).norm(dim=1))
            return b
        return v, bound

    def ln(self, x, gamma, beta, ss=None, rps=1):
        v = rb.ln_fwd_eval(x, gamma, beta, ss, rps, dtype=self.ar.dtype)[0]
        return v, lambda: rb.ln_fwd_bound(x, gamma, beta, ss, rps, fast_silu=True)["out"][1]

    def ln_bwd(self, da, x, gamma, beta, ss, res, rps):
        """hig_ln_bwd_bf16 -> {name: (value, bound callable)} for dx, dgamma, dbeta, dscale, dshift."""
        names = ("dx", "dgamma", "dbeta", "dscale", "dshift")
        if not self.check:
            v = rb.ln_bwd_eval(da, x, None, gamma, beta, ss, res, rps, dtype=self.ar.dtype, tree_rows=self.ar.dtype == F32)
            return {n: (v[i], None) for i, n in enumerate(names)}
        b = rb.ln_bwd_bound(da, x, None, gamma, beta, ss, res, rps, bf16=True)
        return {n: (b[n][0], (lambda n=n: b[n][1])) for n in names if n in b}

    # ---- the three entries ----
    def run(self):
        self.text_context()
        self.forward()
        self.backward()
        return self

    def lens(self):
        return self.inp["length"]

    def text_context(self):
        D, L = self.D, _lib
        xf = self.ar.c(self.inp["xf_out"]).reshape(D.Mt, D.Lt)
        for l in range(D.L):
            self.put("ln", ("xfn", l), *self.ln(xf, self.pl(l, L.L_CA_TNORM_W), self.pl(l, L.L_CA_TNORM_B)), bf16=True)
            self.put("gemm16", ("kv", l), *self.gemm16(self.get(("xfn", l)), self.w16(self.pl(l, L.L_CA_KV_W)), bias=self.pl(l, L.L_CA_KV_B)), bf16=True)
            kv = self.get(("kv", l))
            self.context(("Ac", l), ("kstc", l), kv[:, :D.d], kv[:, D.d:], D.N, None)

    def context(self, kA, kst, K, V, rows, lens):
        """One context build: A (B, H, hd, hd) fp32 and kstat (B, H, hd, 2)."""
        D = self.D
        K, V = heads(K, D.B, rows, D.H, D.hd), heads(V, D.B, rows, D.H, D.hd)
        mm16 = self.forms["ctx_mm16"] and self.ar.rounding
        if mm16:
            A, kmax, Z = lb.ctx_eval(K, V, lens, dtype=self.ar.dtype)
        else:
            A, MA, kmax, Z, Xk = lb.ctx_exact(K, V, lens)
            A, kmax, Z = A.to(self.ar.dtype), kmax.to(self.ar.dtype), Z.to(self.ar.dtype)

        def bounds():
            if mm16:
                return lb.ctx_bounds(K, V, lens)
            g = lb.gammas(rows, D.hd, Xk=Xk)
            return {"A2": (A, g["A"] * U * MA + FLOOR), "Z": (Z, g["Z"] * U * Z)}
        bd = bounds() if self.check else None
        self.put("ctx", kA, A, (lambda: bd["A2"][1]) if self.check else None)
        if self.check:
            self.put("ctx", kst, kmax, None, sel=lambda t: t[..., 0])            # the column maximum is exact
            self.put("ctx", kst, Z, lambda: bd["Z"][1], sel=lambda t: t[..., 1])
        else:
            self.out[kst] = torch.stack([kmax, Z], -1)

    def front(self, l, slot, q, A, ky, ka, norm_w, norm_b, ss_rows=None):
        """attn_front: y = softmax(q) A and a = silu(LN(y) (1 + scale) + shift), fused (one kernel, both from the fp32 y) or as
        hig_linattn_apply_bf16 + hig_ln_bf16.  A: (B, H, hd, hd) [c][l] as the consumer sample sees it."""
        D, ar = self.D, self.ar
        if self.mut == "sty_reads_next_block_slice" and slot == 0 and l == 0:
            slot = 1
        ss = self.get("ss")
        if ss_rows is not None:
            ss = ss[ss_rows]
        s6 = ss6(ss, (D.nsty * l + slot) * 2 * D.d, D.d)
        gamma, beta = self.pl(l, norm_w), self.pl(l, norm_b)
        if self.forms["fuse_front"]:
            At = ar.r16(A.transpose(2, 3))
            a, y = lb.apply_eval(q, At, gamma, beta, s6, D.B, D.T, D.H, D.hd, dtype=ar.dtype, round_p=ar.rounding)
            bd = lb.apply_bounds(q, At, gamma, beta, s6, D.B, D.T, D.H, D.hd) if self.check else None
            self.put("apply", ky, y, (lambda: bd["y2"][1]) if self.check else None, bf16=True)
            self.put("apply", ka, a, (lambda: bd["out2"][1]) if self.check else None, bf16=True)
            return
        qv = heads(q, D.B, D.T, D.H, D.hd)
        p = torch.softmax(qv, -1)
        Ae = A
        if ar.emulate:
            p, Ae = ar.r16(p), ar.r16(A)
        y = torch.einsum("bnhc,bhcl->bnhl", p, Ae).reshape(D.M, D.d)

        def by():
            Xq = (qv.amax(-1) - qv.amin(-1)).max().item()
            assert Xq <= 80
            My = torch.einsum("bnhc,bhcl->bnhl", p, A.abs()).reshape(D.M, D.d)
            return (lin_gammas(D.T, D.hd, Xq, 0.0)["y"] * U + 2 * U16) * My + FLOOR
        self.put("apply", ky, y, by, bf16=True)
        self.put("ln_sty", ka, *self.ln(self.get(ky), gamma, beta, s6, D.T), bf16=True)

    def sty_out(self, l, ka, h_in, kh, out_w, out_b):
        self.put("gemm16", kh, *self.gemm16(self.get(ka), self.w16(self.pl(l, out_w)), bias=self.pl(l, out_b), res=h_in), bf16=True)

    def forward(self):
        D, L, ar, mut = self.D, _lib, self.ar, self.mut
        x = ar.c(self.inp["x"]).reshape(D.M, D.F)
        # K0: the per-sample embedding chain, fp32 on the master weights
        if self.te is not None:
            self.out["te"] = ar.c(self.te)
        else:
            self.put("temb", "te", bb.temb_eval(self.inp["t"], D.d, dtype=ar.dtype), lambda: bb.temb_bound(self.inp["t"], D.d)[1])
        self.put("gemm32", "te_h", *self.gemm32(self.get("te"), self.pg(L.P_TE0_W), self.pg(L.P_TE0_B)))
        self.put("gemm32", "emb", *self.gemm32(self.get("te_h"), self.pg(L.P_TE2_W), self.pg(L.P_TE2_B), ar.c(self.inp["xf_proj"]), silu_x=True))
        self.put("gemm32", "ss", *self.gemm32(self.get("emb"), self.pg(L.P_STY_EMB_W), self.pg(L.P_STY_EMB_B), silu_x=True))
        # K1: h0 = joint_embed(x) + sequence_embedding, rounded once
        shift = 1 if (D.two and mut != "position_shift_missing") else 0
        tpos = torch.arange(D.T) - shift
        pos = self.pg(L.P_SEQ_EMB)[tpos.clamp_min(0)] * (tpos >= 0).to(ar.dtype)[:, None]
        pos = pos.repeat(D.B, 1)
        Wj, bj = self.pg(L.P_JOINT_W), self.pg(L.P_JOINT_B)
        if self.forms["joint_kernel"]:      # x and W rounded to bf16, zero columns up to Fp
            pad = torch.zeros(1, D.Fp - D.F, dtype=ar.dtype)
            h0, bnd = self.gemm32(torch.cat([ar.r16(x), pad.expand(D.M, -1)], 1), torch.cat([ar.r16(Wj), pad.expand(D.d, -1)], 1), bj, pos)
        else:
            h0, bnd = self.gemm32(x, Wj, bj, pos)
        if D.two:       # the init-pose rows: joint_embed2 on the first 4 features, no positional term
            x0 = ar.c(self.inp["x"])[:, 0, :4]
            self.put("gemm32", "tok0", *self.gemm32(x0, self.pg(L.P_JOINT2_W), self.pg(L.P_JOINT2_B)))
            first = torch.arange(D.M) % D.T == 0
            h0 = h0.clone()
            h0[first] = self.get("tok0")
            inner = bnd
            bnd = lambda: inner().masked_fill(first[:, None], 0.0)     # noqa: E731  (a cast of the fp32 rows)
        self.put("joint", "h0", h0, bnd, bf16=True)
        length = self.lens()
        len_partner = swap_halves(length) if (D.two and mut != "partner_lengths_not_swapped") else length
        hin = "h0"
        for l in range(D.L):
            d = D.d
            # ---- self attention ----
            self.put("ln", ("xn1", l), *self.ln(self.get(hin), self.pl(l, L.L_SA_NORM_W), self.pl(l, L.L_SA_NORM_B)), bf16=True)
            self.put("gemm16", ("qkv", l), *self.gemm16(self.get(("xn1", l)), self.w16(self.pl(l, L.L_SA_QKV_W)), bias=self.pl(l, L.L_SA_QKV_B)), bf16=True)
            qkv = self.get(("qkv", l))
            sa_len = length
            if mut == "ragged_context_one_frame_early":
                sa_len = torch.where(length < D.T, length - 1, length)
            self.context(("A1", l), ("kst1", l), qkv[:, d:2 * d], qkv[:, 2 * d:], D.T, sa_len)
            self.front(l, 0, qkv[:, :d], self.get(("A1", l)), ("y1", l), ("a1", l), L.L_SA_STY_NORM_W, L.L_SA_STY_NORM_B)
            self.sty_out(l, ("a1", l), self.get(hin), ("h1", l), L.L_SA_STY_OUT_W, L.L_SA_STY_OUT_B)
            # ---- cross attention ----
            self.put("ln", ("xn2", l), *self.ln(self.get(("h1", l)), self.pl(l, L.L_CA_NORM_W), self.pl(l, L.L_CA_NORM_B)), bf16=True)
            self.put("gemm16", ("qc", l), *self.gemm16(self.get(("xn2", l)), self.w16(self.pl(l, L.L_CA_Q_W)), bias=self.pl(l, L.L_CA_Q_B)), bf16=True)
            self.front(l, 1, self.get(("qc", l)), self.get(("Ac", l)), ("y2", l), ("a2", l), L.L_CA_STY_NORM_W, L.L_CA_STY_NORM_B)
            res = self.get(hin) if mut == "sty_out_residual_from_layer_input" else self.get(("h1", l))
            self.sty_out(l, ("a2", l), res, ("h2", l), L.L_CA_STY_OUT_W, L.L_CA_STY_OUT_B)
            hffn = ("h2", l)
            if D.two:
                # ---- person <-> person: key / value from the partner's stream, masked with the consumer's length ----
                self.put("ln", ("xn3", l), *self.ln(self.get(("h2", l)), self.pl(l, L.L_INT_NORM_W), self.pl(l, L.L_INT_NORM_B)), bf16=True)
                self.put("gemm16", ("iqkv", l), *self.gemm16(self.get(("xn3", l)), self.w16(self.pl(l, L.L_INT_QKV_W)), bias=self.pl(l, L.L_INT_QKV_B)), bf16=True)
                iqkv = self.get(("iqkv", l))
                self.context(("Ai", l), ("ksti", l), iqkv[:, d:2 * d], iqkv[:, 2 * d:], D.T, len_partner)
                Ai = self.get(("Ai", l))
                rows = torch.arange(D.B)
                if mut == "b0_offset_dropped":
                    rows = rows % (D.B // 2)
                self.front(l, 2, iqkv[:, :d], Ai if mut == "contexts_not_swapped" else swap_halves(Ai), ("y4", l), ("a4", l),
                           L.L_INT_STY_NORM_W, L.L_INT_STY_NORM_B, ss_rows=rows)
                self.sty_out(l, ("a4", l), self.get(("h2", l)), ("h2b", l), L.L_INT_STY_OUT_W, L.L_INT_STY_OUT_B)
                hffn = ("h2b", l)
            # ---- FFN ----
            W1, b1 = self.w16(self.pl(l, L.L_FFN_W1)), self.pl(l, L.L_FFN_B1)
            h = self.get(hffn)
            if self.forms["ffn_wsp16"]:     # one launch: f and z both from the fp32 pre-activation
                pre = h @ W1.t() + b1
                bd = gm.gemm_bound(h, W1, gm.GELU, b1, None, True, False) if self.check else None
                self.put("gemm16", ("z1", l), pre, (lambda: bd[3]) if self.check else None, bf16=True)
                src = ar.r16(pre) if mut == "ffn_f_from_rounded_z" else pre
                f = rb.gelu_eval(src, dtype=ar.dtype)
                # (the bf16 GELU is held to a whole bf16 ulp: half of it is what bound16 adds)
                self.put("gemm16_gelu", ("f1", l), f, (lambda: bd[1] - 0.5 * rb.ulp16(f)) if self.check else None, bf16=True)
            else:
                self.put("gemm16", ("z1", l), *self.gemm16(h, W1, bias=b1), bf16=True)
                z = self.get(("z1", l))
                f = rb.gelu_eval(z, dtype=ar.dtype)
                # (hig_gelu_bf16 is the epilogue's bf16 GELU: a whole bf16 ulp, the smallest normal, and beyond |z| = 6.5, where the
                # fit is clamped, the tail include/hig.h states -- act_bound; half of the ulp is what bound16 adds)
                self.put("gelu", ("f1", l), f, lambda: gm.act_bound(gm.GELU, z, f, True) - 0.5 * rb.ulp16(f), bf16=True)
            self.put("gemm16", ("y3", l), *self.gemm16(self.get(("f1", l)), self.w16(self.pl(l, L.L_FFN_W2)), bias=self.pl(l, L.L_FFN_B2)), bf16=True)
            s6 = ss6(self.get("ss"), (D.nsty * l + D.nsty - 1) * 2 * d, d)
            self.put("ln_sty", ("a3", l), *self.ln(self.get(("y3", l)), self.pl(l, L.L_FFN_STY_NORM_W), self.pl(l, L.L_FFN_STY_NORM_B), s6, D.T), bf16=True)
            self.sty_out(l, ("a3", l), self.get(hffn), ("h3", l), L.L_FFN_STY_OUT_W, L.L_FFN_STY_OUT_B)
            hin = ("h3", l)
        # K6: out = Linear(d, F)(h_L), fp32; the init-pose rows through out2
        hL = self.get(hin)
        out, bnd = self.gemm16(hL, self.w16(self.pg(L.P_OUT_W)), bias=self.pg(L.P_OUT_B))
        if D.two:
            first = torch.arange(D.M) % D.T == 0
            o2, b2 = self.gemm16(hL[first], self.w16(self.pg(L.P_OUT2_W)), bias=self.pg(L.P_OUT2_B))
            out = out.clone()
            out[first] = o2
            inner = bnd

            def bnd():
                b = inner().clone()
                b[first] = b2()
                return b
        self.put("gemm16", "out", out, bnd)

    # ---- backward ----
    def wg(self, key_w, key_b, dC, act):
        """One weight gradient of the grouped launches (its bias gradient in the same pass)."""
        dW, bW, db, bb_ = self.wgrad16(dC, act)
        self.put("wgrad16", key_w, dW, bW)
        if key_b is not None:
            self.put("wgrad16", key_b, db, bb_)

    def sty_bwd(self, l, slot, dh, ky, ka, norm_w, norm_b, out_w, out_b, pre):
        D, L = self.D, _lib
        self.wg(("gl", l, out_w), ("gl", l, out_b), dh, self.get(ka))
        Wl = l + 1 if (self.mut == "dgrad_previous_layer_weights" and pre == "ffn" and l + 1 < D.L) else l
        self.put("gemm16", (pre + "_t1", l), *self.gemm16(dh, self.w16(self.pl(Wl, out_w)).t()), bf16=True)
        off = (D.nsty * l + slot) * 2 * D.d
        r = self.ln_bwd(self.get((pre + "_t1", l)), self.get(ky), self.pl(l, norm_w), self.pl(l, norm_b), ss6(self.get("ss"), off, D.d), None, D.T)
        self.put("ln_bwd", (pre + "_dy", l), *r["dx"], bf16=True)
        self.put("ln_bwd", ("gl", l, norm_w), *r["dgamma"])
        self.put("ln_bwd", ("gl", l, norm_b), *r["dbeta"])
        if self.check:
            self.put("ln_bwd", "dss", *r["dscale"], sel=lambda t: t[:, off:off + D.d])
            self.put("ln_bwd", "dss", *r["dshift"], sel=lambda t: t[:, off + D.d:off + 2 * D.d])
        else:
            self.dss[:, off:off + D.d], self.dss[:, off + D.d:off + 2 * D.d] = r["dscale"][0], r["dshift"][0]

    def prenorm_bwd(self, l, pre, kx, norm_w, norm_b, dh, qkv_w):
        """t2 = dqkv . W, then the pre-norm's backward with the residual-stream gradient as `res` -> the next dh."""
        L = _lib
        dq = self.get((pre + ("_dq" if pre == "ca" else "_dqkv"), l))
        self.put("gemm16", (pre + "_t2", l), *self.gemm16(dq, self.w16(self.pl(l, qkv_w)).t()), bf16=True)
        res = None if (self.mut == "ln_bwd_res_dropped_at_prenorm" and pre == "ca") else dh
        r = self.ln_bwd(self.get((pre + "_t2", l)), self.get(kx), self.pl(l, norm_w), self.pl(l, norm_b), None, res, self.D.T)
        self.put("ln_bwd", (pre + "_dh", l), *r["dx"], bf16=True)
        self.put("ln_bwd", ("gl", l, norm_w), *r["dgamma"])
        self.put("ln_bwd", ("gl", l, norm_b), *r["dbeta"])

    def attn_bwd(self, l, pre, dy, q, A, K, V, kst, lens, rows, swap=False):
        """apply_bwd (dq, dA) and ctx_bwd (dk, dv) of one attention; swap: the person <-> person routing of A and dA."""
        D, ar, d = self.D, self.ar, self.D.d
        hv = lambda t, r: heads(t, D.B, r, D.H, D.hd)      # noqa: E731
        dq, dA, bq, bA = apply_bwd(hv(dy, D.T), hv(q, D.T), swap_halves(A) if swap else A, self.check, self.u16)
        if swap:
            dA, bA = swap_halves(dA), (swap_halves(bA) if self.check else None)
        self.put("apply_bwd", (pre + "_dA", l), dA, (lambda: bA) if self.check else None)
        dAb = self.get((pre + "_dA", l))
        dK, dV, bK, bV = ctx_bwd(dAb, A, hv(K, rows), hv(V, rows), kst, lens, self.check, self.u16)
        R = D.B * rows
        if pre == "ca":
            self.put("apply_bwd", ("ca_dq", l), dq.reshape(D.M, d), (lambda: bq.reshape(D.M, d)) if self.check else None, bf16=True)
            self.put("ctx_bwd", ("ca_dkv", l), torch.cat([dK.reshape(R, d), dV.reshape(R, d)], 1),
                     (lambda: torch.cat([bK.reshape(R, d), bV.reshape(R, d)], 1)) if self.check else None, bf16=True)
            return
        if self.check:
            key = (pre + "_dqkv", l)
            self.put("apply_bwd", key, dq.reshape(R, d), lambda: bq.reshape(R, d), bf16=True, sel=lambda t: t[:, :d])
            self.put("ctx_bwd", key, dK.reshape(R, d), lambda: bK.reshape(R, d), bf16=True, sel=lambda t: t[:, d:2 * d])
            self.put("ctx_bwd", key, dV.reshape(R, d), lambda: bV.reshape(R, d), bf16=True, sel=lambda t: t[:, 2 * d:])
        else:
            self.out[(pre + "_dqkv", l)] = ar.r16(torch.cat([dq.reshape(R, d), dK.reshape(R, d), dV.reshape(R, d)], 1))

    def backward(self):
        D, L, ar, mut, d = self.D, _lib, self.ar, self.mut, self.D.d
        x = ar.c(self.inp["x"]).reshape(D.M, D.F)
        dout = ar.c(self.inp["dout"]).reshape(D.M, D.F)
        first = torch.arange(D.M) % D.T == 0
        hL = self.get(("h3", D.L - 1))
        edge16 = self.forms["edge16"]
        if not self.check:
            self.dss = torch.zeros(D.B, D.ss_ld, dtype=ar.dtype)
        # ---- output projection ----
        dout_m = dout.masked_fill(first[:, None], 0.0) if D.two else dout
        if D.two:
            d0 = dout[first]
            self.put("colsum", ("g", L.P_OUT2_B), d0.sum(0), lambda: rb.colsum_bound(d0)[1])
            self.put("gemm32", ("g", L.P_OUT2_W), *self.gemm32(d0.t(), hL[first].t()))
            tok, btok = self.gemm32(d0, self.pg(L.P_OUT2_W).t())
        if edge16:
            d16 = ar.r16(dout_m)
            dW, bW, db, bdb = self.wgrad16(d16, hL)
            self.put("wgrad16", ("g", L.P_OUT_W), dW, bW)
            self.put("wgrad16", ("g", L.P_OUT_B), db, bdb)
            pad = torch.zeros(1, D.Fp - D.F, dtype=ar.dtype)
            dhL, bdh = self.gemm16(torch.cat([d16, pad.expand(D.M, -1)], 1), torch.cat([self.w16(self.pg(L.P_OUT_W)).t(), pad.expand(d, -1)], 1))
        else:
            self.put("colsum", ("g", L.P_OUT_B), dout_m.sum(0), lambda: rb.colsum_bound(dout_m)[1])
            self.put("gemm32", ("g", L.P_OUT_W), *self.gemm32(dout_m.t(), hL.t()))
            dhL, bdh = self.gemm32(dout_m, self.pg(L.P_OUT_W).t())
        if D.two:
            dhL = dhL.clone()
            dhL[first] = tok
            inner = bdh

            def bdh():
                b = inner().clone()
                b[first] = btok()
                return b
        self.put("edge", "dhL", dhL, bdh, bf16=True)
        dh_key = "dhL"
        if not self.check:
            self.out["dxf_out_run"] = torch.full((D.Mt, D.Lt), STALE, dtype=ar.dtype)
        for l in range(D.L - 1, -1, -1):
            hin = "h0" if l == 0 else ("h3", l - 1)
            hffn = ("h2b", l) if D.two else ("h2", l)
            if self.check:
                self.put("copy", ("dh_in", l), self.get(dh_key), None)
            else:
                self.out[("dh_in", l)] = self.get(dh_key)
            dh = self.get(("dh_in", l))
            # ---- FFN ----
            self.sty_bwd(l, D.nsty * 0 + D.nsty - 1, dh, ("y3", l), ("a3", l), L.L_FFN_STY_NORM_W, L.L_FFN_STY_NORM_B, L.L_FFN_STY_OUT_W, L.L_FFN_STY_OUT_B, "ffn")
            dy3 = self.get(("ffn_dy", l))
            f1 = self.get(("f1", l))
            if mut == "wgrad_pad_rows_nonzero":       # the rows M .. Mp of both operands hold ones
                npad = (D.M + 63) // 64 * 64 - D.M
                self.out[("gl", l, L.L_FFN_W2)] = dy3.t() @ f1 + npad
                self.out[("gl", l, L.L_FFN_B2)] = dy3.sum(0) + npad
            else:
                self.wg(("gl", l, L.L_FFN_W2), ("gl", l, L.L_FFN_B2), dy3, f1)
            self.put("gemm16_dgelu", ("ffn_dz", l), *self.gemm16(dy3, self.w16(self.pl(l, L.L_FFN_W2)).t(), "dgelu", res=self.get(("z1", l))), bf16=True)
            dz = self.get(("ffn_dz", l))
            self.wg(("gl", l, L.L_FFN_W1), ("gl", l, L.L_FFN_B1), dz, self.get(hffn))
            res = None if mut == "w1_dgrad_residual_dropped" else dh
            self.put("gemm16", ("ffn_dh", l), *self.gemm16(dz, self.w16(self.pl(l, L.L_FFN_W1)).t(), res=res), bf16=True)
            dh = self.get(("ffn_dh", l))
            if mut == "wgrad_reads_dh_after_swap":     # the FFN group's stylization-out gradient, launched behind the swap
                self.out[("gl", l, L.L_FFN_STY_OUT_W)] = dh.t() @ self.get(("a3", l))
            if D.two:
                # ---- person <-> person ----
                self.sty_bwd(l, 2, dh, ("y4", l), ("a4", l), L.L_INT_STY_NORM_W, L.L_INT_STY_NORM_B, L.L_INT_STY_OUT_W, L.L_INT_STY_OUT_B, "int")
                iqkv = self.get(("iqkv", l))
                self.attn_bwd(l, "int", self.get(("int_dy", l)), iqkv[:, :d], self.get(("Ai", l)), iqkv[:, d:2 * d], iqkv[:, 2 * d:],
                              self.get(("ksti", l)), swap_halves(self.lens()), D.T, swap=True)
                self.wg(("gl", l, L.L_INT_QKV_W), ("gl", l, L.L_INT_QKV_B), self.get(("int_dqkv", l)), self.get(("xn3", l)))
                self.prenorm_bwd(l, "int", ("h2", l), L.L_INT_NORM_W, L.L_INT_NORM_B, dh, L.L_INT_QKV_W)
                dh = self.get(("int_dh", l))
            # ---- cross attention ----
            self.sty_bwd(l, 1, dh, ("y2", l), ("a2", l), L.L_CA_STY_NORM_W, L.L_CA_STY_NORM_B, L.L_CA_STY_OUT_W, L.L_CA_STY_OUT_B, "ca")
            kv = self.get(("kv", l))
            self.attn_bwd(l, "ca", self.get(("ca_dy", l)), self.get(("qc", l)), self.get(("Ac", l)), kv[:, :d], kv[:, d:], self.get(("kstc", l)), None, D.N)
            self.wg(("gl", l, L.L_CA_Q_W), ("gl", l, L.L_CA_Q_B), self.get(("ca_dq", l)), self.get(("xn2", l)))
            self.prenorm_bwd(l, "ca", ("h1", l), L.L_CA_NORM_W, L.L_CA_NORM_B, dh, L.L_CA_Q_W)
            dh = self.get(("ca_dh", l))
            dkv = self.get(("ca_dkv", l))
            self.wg(("gl", l, L.L_CA_KV_W), ("gl", l, L.L_CA_KV_B), dkv, self.get(("xfn", l)))
            self.put("gemm16", ("ca_dxfn", l), *self.gemm16(dkv, self.w16(self.pl(l, L.L_CA_KV_W)).t()), bf16=True)
            prev = ("ca_dxf_out", l + 1) if l + 1 < D.L else (None if (self.check or mut != "dxf_out_accumulates_at_last_layer") else "dxf_out_run")
            if mut == "dxf_out_last_term_only":
                prev = None
            xf = ar.c(self.inp["xf_out"]).reshape(D.Mt, D.Lt)
            r = self.ln_bwd(self.get(("ca_dxfn", l)), xf, self.pl(l, L.L_CA_TNORM_W), self.pl(l, L.L_CA_TNORM_B), None,
                            None if prev is None else self.get(prev), D.N)
            self.put("ln_bwd", ("ca_dxf_out", l), *r["dx"])
            self.put("ln_bwd", ("gl", l, L.L_CA_TNORM_W), *r["dgamma"])
            self.put("ln_bwd", ("gl", l, L.L_CA_TNORM_B), *r["dbeta"])
            # ---- self attention ----
            self.sty_bwd(l, 0, dh, ("y1", l), ("a1", l), L.L_SA_STY_NORM_W, L.L_SA_STY_NORM_B, L.L_SA_STY_OUT_W, L.L_SA_STY_OUT_B, "sa")
            qkv = self.get(("qkv", l))
            self.attn_bwd(l, "sa", self.get(("sa_dy", l)), qkv[:, :d], self.get(("A1", l)), qkv[:, d:2 * d], qkv[:, 2 * d:], self.get(("kst1", l)),
                          self.lens(), D.T)
            self.wg(("gl", l, L.L_SA_QKV_W), ("gl", l, L.L_SA_QKV_B), self.get(("sa_dqkv", l)), self.get(("xn1", l)))
            self.prenorm_bwd(l, "sa", hin, L.L_SA_NORM_W, L.L_SA_NORM_B, dh, L.L_SA_QKV_W)
            dh_key = ("sa_dh", l)
        if self.check:
            self.put("copy", "dxf_out", self.get(("ca_dxf_out", 0)), None)
        else:
            self.out["dxf_out"] = self.get(("ca_dxf_out", 0))
            self.out["dss"] = self.dss
        # ---- joint_embed + sequence_embedding ----
        dh0 = self.get(dh_key)
        if D.two:
            self.put("copy", "tok0g", dh0[first], None)
            tok0 = self.get("tok0g")
            self.put("colsum", ("g", L.P_JOINT2_B), tok0.sum(0), lambda: rb.colsum_bound(tok0)[1])
            self.put("gemm32", ("g", L.P_JOINT2_W), *self.gemm32(tok0.t(), ar.c(self.inp["x"])[:, 0, :4].t()))
            dh0 = dh0.masked_fill(first[:, None], 0.0)
        Tpos = D.T - 1 if D.two else D.T
        flat = dh0.reshape(D.B, D.T * d)
        if edge16:
            dW, bW, db, bdb = self.wgrad16(dh0, ar.r16(x))
            self.put("wgrad16", ("g", L.P_JOINT_W), dW, bW)
            self.put("wgrad16", ("g", L.P_JOINT_B), db, bdb)
        else:
            self.put("colsum", ("g", L.P_JOINT_B), dh0.sum(0), lambda: rb.colsum_bound(dh0)[1])
            self.put("gemm32", ("g", L.P_JOINT_W), *self.gemm32(dh0.t(), x.t()))
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
            dx[first] = torch.cat([dx4, dx[first][:, 4:]], 1)
            inner2 = bdx

            def bdx():
                b = inner2().clone()
                b[first] = torch.cat([b4(), b[first][:, 4:]], 1)
                return b
        self.put("gemm32", "dx", dx, bdx)
        self.time_path_bwd()

    def time_path_bwd(self):
        """The time / text embedding path (fp32 in either storage): from dss to the gradients of the embedding chain and dxf_proj."""
        D, L, mut, d = self.D, _lib, self.mut, self.D.d
        dss, emb, te_h, te = self.get("dss"), self.get("emb"), self.get("te_h"), self.get("te")
        self.put("colsum", ("g", L.P_STY_EMB_B), dss.sum(0), lambda: rb.colsum_bound(dss)[1])
        dsrc = dss
        if mut == "w_emb_rows_from_wrong_layer":
            rl = D.nsty * 2 * d
            dsrc = torch.cat([dss[:, ((l + 1) % D.L) * rl:((l + 1) % D.L + 1) * rl] for l in range(D.L)], 1)
        self.put("gemm32", ("g", L.P_STY_EMB_W), *self.gemm32(dsrc.t(), emb.t(), silu_w=True))
        self.put("gemm32", "dtmp_emb", *self.gemm32(dss, self.pg(L.P_STY_EMB_W).t()))
        dtmp = self.get("dtmp_emb")
        self.put("dsilu", "demb", dtmp * dsilu(emb), lambda: dsilu_bound(dtmp, emb))
        demb = self.get("demb")
        self.put("copy", "dxf_proj", demb, None)
        self.put("colsum", ("g", L.P_TE2_B), demb.sum(0), lambda: rb.colsum_bound(demb)[1])
        self.put("gemm32", ("g", L.P_TE2_W), *self.gemm32(demb.t(), te_h.t(), silu_w=True))
        self.put("gemm32", "dtmp_te", *self.gemm32(demb, self.pg(L.P_TE2_W).t()))
        dtmp = self.get("dtmp_te")
        self.put("dsilu", "dte_h", dtmp * dsilu(te_h), lambda: dsilu_bound(dtmp, te_h))
        dte_h = self.get("dte_h")
        self.put("colsum", ("g", L.P_TE0_B), dte_h.sum(0), lambda: rb.colsum_bound(dte_h)[1])
        self.put("gemm32", ("g", L.P_TE0_W), *self.gemm32(dte_h.t(), te.t()))


def plan_forms(D, ffn_wsp16, fuse_front, ctx_mm16, edge16):
    """The forms of a call: joint_embed's follows from d and F alone (hig_denoiser_fwd_bf16_train, K1); the others are what
    hig_gemm_bf16_plan and hig_denoiser_last_schedule report."""
    return dict(joint_kernel=D.d % 128 == 0 and D.F <= 512, ffn_wsp16=bool(ffn_wsp16), fuse_front=bool(fuse_front), ctx_mm16=bool(ctx_mm16),
                edge16=bool(edge16))


# ----------------------------------------------------------------------------------------------------------------------
# models, inputs and the loss the cases share
# ----------------------------------------------------------------------------------------------------------------------
def build_model(c, device="cpu", **kw):
    """The model of case c with the oracle's name-seeded parameters (oracle/fill.py)."""
    import hig_amd
    from oracle import fill
    cls = hig_amd.MotionInteractionTransformer if c["two"] else hig_amd.MotionTransformer
    m = cls(input_feats=c["F"], num_frames=c["num_frames"], latent_dim=c["d"], ff_size=c["ff"], num_layers=c["L"], num_heads=c["H"],
            text_latent_dim=c["Lt"], **kw)
    m.load_state_dict(fill.fill_state_dict(m.state_dict()), strict=True)
    return m.to(device)


def case_inputs(c):
    """x, t, length, xf_proj, xf_out and the loss target of case c (host, fp32)."""
    from oracle import fill
    inp = fill.inputs(c["B"], c["T"], c["F"], c["d"], c["N"], c["Lt"], c["lengths"], c["t"])
    inp["target"] = fill.tensor_for("full.target", inp["x"].shape) * 10.0
    return inp


def masked_mse_grad(out, target, length):
    """d(loss) / d(out) of loss = sum_bt mask mean_f (out - target)^2 / sum mask (oracle.diffusion_ref.masked_mse)."""
    B, T, F = out.shape
    mask = (torch.arange(T)[None] < length[:, None]).to(out.dtype)
    return 2 * (out - target.to(out.dtype)) * mask[..., None] / (F * mask.sum())
