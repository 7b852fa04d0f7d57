"""Bounds, an fp64 restatement and the weight builders of the CLIP text tower (csrc/cliptext.hip), shared by
tests/test_cpu_clip_text.py (which holds the bounds to fp32 emulations and to wrong arithmetic, without a GPU) and
tests/test_gpu_clip_text.py (which holds the kernels to them).

The bounds follow the rounding-count conventions of tests/test_gpu_attn_contract.py's docstring (u = 2^-24: a result differs
from its fp64 value by at most gamma u M; a sum of n terms in any order costs n; __expf(x) = v_exp_f32(x log2 e) costs
2 + 2.5 |x|; a division by a denominator costs 3).

QUICKGELU.  y = z * rcp(1 + exp2(c z)), c = fl(-1.702 log2 e), x = 1.702 z:
    the argument c z carries the constant's rounding and the product's: 2 u |x| absolute in the exponent, so 2 |x| u relative
    in e = exp(-x); v_exp_f32 itself 2 u (one ulp):                                          e costs 2 + 2 |x|
    s = 1 + e: e's error enters with the weight e / (1 + e) = sigmoid(-x), the sum rounds once: (2 + 2 |x|) sigmoid(-x) + 1
    v_rcp_f32 (one ulp) and the product with z: 3
        gamma(x) = 4 + (2 + 2 |x|) sigmoid(-x)
    plus an absolute floor: the two instructions flush results below 2^-126 to zero, so the sigmoid factor can be off by
    2^-126 where it is that small (x < -87), and the product by as much again:              |z| 2^-125
        |y - y64| <= gamma(x) u |y64| + 2^-125 |z|
    (gamma is ~ 5 for z >= 0 and grows like 3.4 |z| on the negative side, where y itself decays like e^-1.7|z|.)

CAUSAL ATTENTION.  `full_bounds`' y form of the attention contract with Tk replaced by the n + 1 live keys of row n:
    e_nm = (hd + 3) MS_nm + 3 (|S_nm| + |lse_n|) + 2 + 2.5 (lse_n - S_nm)         MS = sum_d |q_d k_d| / sqrt(hd)
    D_n  = sum_{m <= n} w_nm e_nm + (n + 1) + 3 ceil((n + 1) / 32) + 3
    |y_nl - y64_nl| <= u sum_{m <= n} w_nm (e_nm + D_n + (n + 1) + 2) |v_ml| + 2^-120
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
FLOOR = 2.0 ** -120
HD = 64
SOT, EOT = 49406, 49407


# ---- QuickGELU ---------------------------------------------------------------------------------------------------------------
def quick_gelu_ref(z):
    z = z.double()
    return z * torch.sigmoid(1.702 * z)


def quick_gelu_bound(z):
    z = z.double()
    x = 1.702 * z
    gamma = 4 + (2 + 2 * x.abs()) * torch.sigmoid(-x)
    return gamma * U * quick_gelu_ref(z).abs() + 2.0 ** -125 * z.abs()


def quick_gelu_grid(n, seed=0):
    """n values, 1e-6 <= |z| <= 1e3, log-dense, both signs, in a seeded random order (so every lane sees every range)."""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 9.0 - 6.0)
    mag[0], mag[-1] = 1e-6, 1e3
    sign = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0).double()
    return (mag * sign).float()


def quick_gelu_f32(z, c=1.702):
    """The kernel's arithmetic in numpy fp32 (flushing what the two instructions flush)."""
    z = np.asarray(z, dtype=np.float32)
    k = np.float32(-c * 1.44269504088896340736)
    tiny = np.float32(2.0 ** -126)
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp2(z * k, dtype=np.float32)
        e = np.where(e < tiny, np.float32(0), e)
        r = (np.float32(1) / (np.float32(1) + e)).astype(np.float32)
        r = np.where(r < tiny, np.float32(0), r)
        return (z * r).astype(np.float32)


# ---- causal attention --------------------------------------------------------------------------------------------------------
def causal_reference(q, k, v, scale=1.0 / 8.0, shift=0):
    """fp64 causal attention and the quantities of its bound.  q, k, v: (B, N, H, hd).  Row n sees keys m <= n + shift
    (shift != 0 builds the WRONG results the CPU test rejects)."""
    q, k, v = q.double(), k.double(), v.double()
    B, N, H, hd = q.shape
    S = torch.einsum("bnhd,bmhd->bhnm", q, k) * scale
    MS = torch.einsum("bnhd,bmhd->bhnm", q.abs(), k.abs()) * scale
    live = torch.arange(N)[None, :] <= torch.arange(N)[:, None] + shift        # [n][m]
    Sm = S.masked_fill(~live, float("-inf"))
    lse = torch.logsumexp(Sm, -1)
    w = torch.exp(Sm - lse[..., None])
    y = torch.einsum("bhnm,bmhl->bnhl", w, v)
    spread = (Sm.amax(-1) - S.masked_fill(~live, float("inf")).amin(-1)).max().item()
    return {"S": S, "MS": MS, "live": live, "lse": lse, "w": w, "y": y, "va": v.abs(), "spread": spread}


def causal_bound(r):
    """(B, N, H, hd) per-element bound on y (module docstring)."""
    N = r["S"].shape[-1]
    live = r["live"]
    keys = torch.arange(1, N + 1, dtype=torch.float64)                          # n + 1 live keys in row n
    x = (r["lse"][..., None] - r["S"]).masked_fill(~live, 0.0)
    e = ((HD + 3) * r["MS"] + 3 * (r["S"].abs() + r["lse"].abs()[..., None]) + 2 + 2.5 * x).masked_fill(~live, 0.0)
    D = (r["w"] * e).sum(-1) + keys + 3 * torch.ceil(keys / 32) + 3            # (B, H, N)
    return U * torch.einsum("bhnm,bmhl->bnhl", r["w"] * (e + (D + keys + 2)[..., None]), r["va"]) + FLOOR


def causal_f32(q, k, v, scale=0.125, shift=0):
    """Causal attention in numpy fp32, the kernel's order of operations up to the order inside the sums."""
    q, k, v = (np.asarray(t, dtype=np.float32) for t in (q, k, v))
    B, N, H, hd = q.shape
    y = np.zeros_like(q)
    for n in range(N):
        m = min(N, n + 1 + shift)
        s = (np.einsum("bhd,bmhd->bhm", q[:, n], k[:, :m]).astype(np.float32) * np.float32(scale)).astype(np.float32)
        p = np.exp((s - s.max(-1, keepdims=True)).astype(np.float32)).astype(np.float32)
        inv = (np.float32(1) / p.sum(-1, dtype=np.float32)).astype(np.float32)
        y[:, n] = np.einsum("bhm,bmhl->bhl", p, v[:, :m]).astype(np.float32) * inv[..., None]
    return y


def causal_inputs(B, H, N, seed, spread=None):
    """One (B N, 3 W) fp32 buffer whose column blocks are Q, K, V -- how the tower calls the kernel.  spread: Q is scaled so
    that the largest logit spread of a row is this value."""
    g = torch.Generator().manual_seed(seed)
    W = H * HD
    qkv = torch.randn(B * N, 3 * W, generator=g) * 1.5
    if spread is not None and N > 1:
        q, k, v = split_qkv(qkv, B, N, H)
        qkv[:, :W] *= spread / causal_reference(q, k, v)["spread"]
    return qkv


def split_qkv(qkv, B, N, H):
    W = H * HD
    return tuple(qkv[:, i * W:(i + 1) * W].reshape(B, N, H, HD) for i in range(3))


# ---- the tower ---------------------------------------------------------------------------------------------------------------
def tower_weights(W, H, L, N=77, vocab=49408, seed=0):
    """A state dict under OpenAI's names, fp32, drawn with CLIP.initialize_parameters' standard deviations (which keep the
    logit spread of every softmax near 1); the LayerNorm scales are 1 + 0.1 n, the biases 0.02 n, so that every parameter
    of the table shows in the output."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *shape: torch.randn(*shape, generator=g)   # noqa: E731
    proj_std, attn_std, fc_std = (W ** -0.5) * ((2 * L) ** -0.5), W ** -0.5, (2 * W) ** -0.5
    sd = {"token_embedding.weight": n(vocab, W) * 0.02, "positional_embedding": n(N, W) * 0.01,
          "ln_final.weight": 1 + 0.1 * n(W), "ln_final.bias": 0.02 * n(W)}
    for i in range(L):
        p = "transformer.resblocks.%d." % i
        sd[p + "ln_1.weight"], sd[p + "ln_1.bias"] = 1 + 0.1 * n(W), 0.02 * n(W)
        sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"] = n(3 * W, W) * attn_std, 0.02 * n(3 * W)
        sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = n(W, W) * proj_std, 0.02 * n(W)
        sd[p + "ln_2.weight"], sd[p + "ln_2.bias"] = 1 + 0.1 * n(W), 0.02 * n(W)
        sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = n(4 * W, W) * fc_std, 0.02 * n(4 * W)
        sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = n(W, 4 * W) * proj_std, 0.02 * n(W)
    return sd


def tower_tokens(B, N=77, vocab=49408, seed=0):
    """SOT, random ids, EOT, zero padding; lengths from 3 to N (the first sample is the shortest, the second the longest).
    With a small vocabulary SOT / EOT are its two largest ids, so that EOT stays the arg-max."""
    g = torch.Generator().manual_seed(1000 + seed)
    sot, eot = (SOT, EOT) if vocab > EOT else (vocab - 2, vocab - 1)
    lengths = [3, N] + [int(torch.randint(4, N, (1,), generator=g)) for _ in range(max(B - 2, 0))]
    out = torch.zeros(B, N, dtype=torch.int64)
    for b, n in enumerate(lengths[:B]):
        out[b, 0], out[b, n - 1] = sot, eot
        out[b, 1:n - 1] = torch.randint(1, sot, (n - 2,), generator=g)
    return out


def _ln64(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * w + b


def tower_fp64(sd, tokens, H):
    """ln_final's output (B, N, W) in fp64 from the state dict alone: plain matmuls, no nn.Module."""
    p = {k: v.double() for k, v in sd.items()}
    B, N = tokens.shape
    W = p["ln_final.weight"].shape[0]
    hd = W // H
    L = 1 + max(int(k.split(".")[2]) for k in p if k.startswith("transformer.resblocks."))
    x = p["token_embedding.weight"][tokens] + p["positional_embedding"][None]
    dead = torch.arange(N)[None, :] > torch.arange(N)[:, None]
    for i in range(L):
        g = lambda name: p["transformer.resblocks.%d.%s" % (i, name)]   # noqa: E731
        h = _ln64(x, g("ln_1.weight"), g("ln_1.bias"))
        qkv = h @ g("attn.in_proj_weight").T + g("attn.in_proj_bias")
        q, k, v = (t.reshape(B, N, H, hd).permute(0, 2, 1, 3) for t in qkv.split(W, dim=-1))
        s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
        a = torch.softmax(s.masked_fill(dead, float("-inf")), -1) @ v
        x = x + a.permute(0, 2, 1, 3).reshape(B, N, W) @ g("attn.out_proj.weight").T + g("attn.out_proj.bias")
        h = _ln64(x, g("ln_2.weight"), g("ln_2.bias"))
        z = h @ g("mlp.c_fc.weight").T + g("mlp.c_fc.bias")
        x = x + (z * torch.sigmoid(1.702 * z)) @ g("mlp.c_proj.weight").T + g("mlp.c_proj.bias")
    return _ln64(x, p["ln_final.weight"], p["ln_final.bias"])


def rel_per_sample(a, ref):
    """Per-sample relative L2 distance of (B, ...) tensors, in fp64 on the CPU."""
    a, ref = a.detach().double().cpu().flatten(1), ref.detach().double().cpu().flatten(1)
    return (a - ref).norm(dim=1) / ref.norm(dim=1)
