"""Bounds, fp64 statements and fp32 emulations of the CLIP text tower's adjoint (csrc/cliptext_bwd.hip, the training entries of
csrc/cliptext.hip), shared by tests/test_cpu_clip_train.py (which holds the bounds to fp32 emulations and to wrong arithmetic,
without a GPU) and tests/test_gpu_clip_train.py (which holds the kernels to them).  tests/clip_bounds.py is imported for the
forward's statements and the weight builders.

Rounding-count conventions: tests/test_gpu_attn_contract.py's docstring (u = 2^-24; a sum of n terms in any order costs n;
__expf(x) costs 2 + 2.5 |x|; a reciprocal and a product 3).

CAUSAL BACKWARD.  The backward form of `full_bounds` with the causal counts.  The kernel is judged on what it is GIVEN (lse, Y):
    w_nm is rebuilt per element from the given lse:   g_wb = (hd + 2) MS + 2 (|S| + |lse|) + 2.5 |S - lse| + 4
    dS = w (dY . v - delta):                          g_dS = g_wb + 2 hd + 3   on MdS = w (|dY| . |v| + sum_l |dY Y|)
    dQ_n sums its n + 1 live keys:                    (g_dS + (n + 1) + 2) MdS |k| / 8
    dK_m sums its N - m live queries:                 (g_dS + (N - m) + 2) MdS |q| / 8
    dV_m sums its N - m live queries:                 (g_wb + (N - m) + 2) w |dY|
    lse_n: `full_bounds`' lse form with Tk = n + 1:   g_lse = (hd + 2) + (n + 1) + 3 ceil((n + 1) / 32) + 6.5 log(n + 1) + 8,
                                                      |lse - lse64| <= g_lse u (1 + max_{m <= n} |S_nm|)
each plus the 2^-120 floor of the attention contract.

QUICKGELU BACKWARD.  dz = dy s (1 + x t), x = fl(1.702 z), s = rcp(1 + e), e = exp2(c z), t = 1 - s formed as e s for z >= 0 and
as 1 - s for z < 0 (csrc/cliptext_bwd.hip: quick_gelu_grad).  The derivative changes sign near x = -1.28, so the bound is on
magnitudes, G = 1 + |x| (1 - s):
    s      as in quick_gelu_bound, without the product with z:   g_s = 3 + (2 + 2 |x|) sigmoid(-x)
    x      the rounded constant and the product:                  2
    t      z >= 0: e (2 + 2 |x|), s (g_s) and their product (1):  g_t = 6 + (2 + 2 |x|) (1 + sigmoid(-x))
           z <  0: s's absolute error g_s s against 1 - s >= 1/2, and the difference (1):
                                                                  g_t = 4 + (2 + 2 |x|) sigmoid(x)      (s / (1 - s) * sigmoid(-x) = s)
    1 + x t  one fma: the product term carries 2 + g_t on |x| t, the sum rounds once against G:   (2 + g_t) rho + 1,
           rho = |x| (1 - s) / G  (<= 1)
    the products with s and with dy:  g_s + 1 + 1
        gamma(x) = g_s + 3 + (2 + g_t) rho
    (about 6 at x = 0, 6 + 2 |x| e^-|x| (..) for large positive x, where rho vanishes, and ~ 9 + 4 |x| e^-|x| on the negative
    side.)  Absolute floor: v_exp_f32 and v_rcp_f32 flush results below 2^-126, so s (x < -87) or e (x > 87) can be off by
    2^-126 where they are that small; the factor they enter is at most 1 + |x|:   2^-125 |dy| (1 + |x|)
        |dz - dz64| <= gamma(x) u |dy| s (1 + |x| (1 - s)) + 2^-125 |dy| (1 + |x|)
"""
import numpy as np
import torch

import clip_bounds as CB

U = CB.U
FLOOR = CB.FLOOR
HD = CB.HD


# ---- causal attention backward -----------------------------------------------------------------------------------------------------
def causal_bwd_reference(q, k, v, dy, lse_in, y_in, scale=1.0 / 8.0):
    """fp64 statement of hig_causal_attn_bwd on what it is given, with the magnitudes of its bound.  q, k, v, dy, y_in:
    (B, N, H, hd); lse_in (B, H, N)."""
    q, k, v, dy, y_in, lse_in = (t.double() for t in (q, k, v, dy, y_in, lse_in))
    N = q.shape[1]
    live = torch.arange(N)[None, :] <= torch.arange(N)[:, None]                        # [n][m]
    S = torch.einsum("bnhd,bmhd->bhnm", q, k) * scale
    MS = torch.einsum("bnhd,bmhd->bhnm", q.abs(), k.abs()) * scale
    x = (S - lse_in[..., None]).masked_fill(~live, float("-inf"))
    w = torch.exp(x)
    dP = torch.einsum("bnhl,bmhl->bhnm", dy, v)
    aP = torch.einsum("bnhl,bmhl->bhnm", dy.abs(), v.abs())
    delta = (dy * y_in).sum(-1).permute(0, 2, 1)                                        # (B, H, N)
    adelta = (dy.abs() * y_in.abs()).sum(-1).permute(0, 2, 1)
    dS = w * (dP - delta[..., None])
    r = {"S": S, "MS": MS, "live": live, "w": w, "lse": lse_in, "dS": dS, "MdS": w * (aP + adelta[..., None]), "delta": delta,
         "dQ": torch.einsum("bhnm,bmhd->bnhd", dS, k) * scale, "dK": torch.einsum("bhnm,bnhd->bmhd", dS, q) * scale,
         "dV": torch.einsum("bhnm,bnhl->bmhl", w, dy), "qa": q.abs() * scale, "ka": k.abs() * scale, "dya": dy.abs()}
    return r


def causal_bwd_bounds(r):
    """Per-element bounds on dQ, dK, dV (module docstring), each (B, N, H, hd)."""
    N = r["S"].shape[-1]
    live = r["live"]
    g_wb = ((HD + 2) * r["MS"] + 2 * (r["S"].abs() + r["lse"].abs()[..., None]) + 2.5 * (r["S"] - r["lse"][..., None]).abs() + 4)
    g_wb = g_wb.masked_fill(~live, 0.0)
    g_dS = g_wb + 2 * HD + 3
    keys = torch.arange(1, N + 1, dtype=torch.float64)[:, None]                          # n + 1 live keys of row n
    queries = (N - torch.arange(N, dtype=torch.float64))[None, :]                         # N - m live queries of key m
    return {"dQ": U * torch.einsum("bhnm,bmhd->bnhd", (g_dS + keys + 2) * r["MdS"], r["ka"]) + FLOOR,
            "dK": U * torch.einsum("bhnm,bnhd->bmhd", (g_dS + queries + 2) * r["MdS"], r["qa"]) + FLOOR,
            "dV": U * torch.einsum("bhnm,bnhl->bmhl", (g_wb + queries + 2) * r["w"], r["dya"]) + FLOOR}


def lse_bound(r):
    """(B, H, N) bound on the forward's lse; r = CB.causal_reference(...)."""
    N = r["S"].shape[-1]
    keys = torch.arange(1, N + 1, dtype=torch.float64)
    g = (HD + 2) + keys + 3 * torch.ceil(keys / 32) + 6.5 * torch.log(keys) + 8
    smax = r["S"].abs().masked_fill(~r["live"], 0.0).amax(-1)
    return g * U * (1 + smax)


def causal_bwd_f32(q, k, v, dy, lse_in, y_in, scale=0.125, shift=0, with_delta=True, dk_scale=None):
    """The kernels' arithmetic in numpy fp32, up to the order inside the sums.  The keyword arguments build the WRONG results
    the CPU test rejects: shift = 1 lets row n see key n + 1, with_delta=False drops the - delta term, dk_scale replaces the
    1/8 on dK, scale the one on the logits and dQ."""
    q, k, v, dy, y_in, lse_in = (np.asarray(t, dtype=np.float32) for t in (q, k, v, dy, y_in, lse_in))
    N = q.shape[1]
    f = np.float32
    live = np.arange(N)[None, :] <= np.arange(N)[:, None] + shift
    s = (np.einsum("bnhd,bmhd->bhnm", q, k).astype(f) * f(scale)).astype(f)
    with np.errstate(over="ignore"):
        w = np.where(live, np.exp((s - lse_in[..., None]).astype(f)).astype(f), f(0))
    dP = np.einsum("bnhl,bmhl->bhnm", dy, v).astype(f)
    delta = np.transpose((dy * y_in).astype(f).sum(-1, dtype=f), (0, 2, 1))
    dS = (w * ((dP - delta[..., None]).astype(f) if with_delta else dP)).astype(f)
    dQ = (np.einsum("bhnm,bmhd->bnhd", dS, k).astype(f) * f(scale)).astype(f)
    dK = (np.einsum("bhnm,bnhd->bmhd", dS, q).astype(f) * f(scale if dk_scale is None else dk_scale)).astype(f)
    dV = np.einsum("bhnm,bnhl->bmhl", w, dy).astype(f)
    return dQ, dK, dV


def causal_bwd_inputs(B, H, N, seed, spread=None):
    """qkv as CB.causal_inputs gives it, an upstream dY (B N, W), and the fp64 forward (lse, y) the backward is handed in fp32."""
    qkv = CB.causal_inputs(B, H, N, seed, spread)
    g = torch.Generator().manual_seed(7000 + seed)
    dy = torch.randn(B * N, H * HD, generator=g)
    q, k, v = CB.split_qkv(qkv, B, N, H)
    fwd = CB.causal_reference(q, k, v)
    return qkv, dy, fwd["lse"].float(), fwd["y"].float().reshape(B * N, H * HD), fwd


# ---- QuickGELU backward ----------------------------------------------------------------------------------------------------------
def quick_gelu_grad_ref(z, dy):
    z, dy = z.double(), dy.double()
    x = 1.702 * z
    s = torch.sigmoid(x)
    return dy * s * (1 + x * torch.sigmoid(-x))


def quick_gelu_grad_bound(z, dy):
    z, dy = z.double(), dy.double()
    x = 1.702 * z
    ax, s, sm = x.abs(), torch.sigmoid(x), torch.sigmoid(-x)
    g_s = 3 + (2 + 2 * ax) * sm
    g_t = torch.where(z >= 0, 6 + (2 + 2 * ax) * (1 + sm), 4 + (2 + 2 * ax) * s)
    G = 1 + ax * sm
    gamma = g_s + 3 + (2 + g_t) * (ax * sm / G)
    return gamma * U * dy.abs() * s * G + 2.0 ** -125 * dy.abs() * (1 + ax)


def quick_gelu_grad_f32(z, dy, c=1.702, drop_one_minus_s=False):
    """The kernel's arithmetic in numpy fp32 (flushing what the two instructions flush).  c = 1.7 and drop_one_minus_s build the
    WRONG results the CPU test rejects."""
    f = np.float32
    z, dy = np.asarray(z, dtype=f), np.asarray(dy, dtype=f)
    k = f(-c * 1.44269504088896340736)
    tiny = f(2.0 ** -126)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = np.exp2((z * k).astype(f), dtype=f)
        e = np.where(e < tiny, f(0), e)
        s = (f(1) / (f(1) + e)).astype(f)
        s = np.where(s < tiny, f(0), s)
        x = (f(c) * z).astype(f)
        es = np.where(np.isinf(e), f(0), (e * s).astype(f))
        t = np.where(z >= 0, es, (f(1) - s).astype(f))
        if drop_one_minus_s:
            t = np.ones_like(t)
        inner = (x.astype(np.float64) * t.astype(np.float64) + 1.0).astype(f)          # one fma
        return (dy * (s * inner).astype(f)).astype(f)


# ---- the embedding gradient ---------------------------------------------------------------------------------------------------------
def embed_index_restated(tokens, vocab, chunk):
    """{id: [chunks, each a list of rows b N + n]} in plain Python: ascending rows per id, cut into chunks of `chunk`."""
    B, N = tokens.shape
    lists = {}
    for b in range(B):
        for n in range(N):
            t = int(tokens[b, n])
            if 0 <= t < vocab:
                lists.setdefault(t, []).append(b * N + n)
    return {t: [rows[i:i + chunk] for i in range(0, len(rows), chunk)] for t, rows in sorted(lists.items())}


def embed_grad_from_lists(dx0, lists, vocab):
    """The chunked fp32 sum from the plain lists: the statement of hig_clip_embed_bwd's token gradient."""
    dx0 = np.asarray(dx0, dtype=np.float32)
    out = np.zeros((vocab, dx0.shape[1]), dtype=np.float32)
    for t, chunks in lists.items():
        total = None
        for rows in chunks:
            part = dx0[rows[0]].copy()
            for r in rows[1:]:
                part = (part + dx0[r]).astype(np.float32)
            total = part if total is None else (total + part).astype(np.float32)
        out[t] = total
    return out


# ---- the whole tower's adjoint in fp64, from the state dict alone ----------------------------------------------------------------
def _ln_parts(x, w, b):
    mu = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    xh = (x - mu) * rstd
    return xh * w + b, xh, rstd


def _ln_bwd(dy, xh, rstd, w):
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).flatten(0, -2).sum(0), dy.flatten(0, -2).sum(0)


def tower_adjoint_fp64(sd, tokens, H, dout):
    """{state-dict name: gradient} of sum(out * dout), out = ln_final's output (B, N, W): the sequence of hig_clip_text_bwd in
    fp64 with the three adjoints stated here (causal_bwd_reference, quick_gelu_grad_ref, the embedding sums)."""
    p = {k: v.double() for k, v in sd.items()}
    B, N = tokens.shape
    W = p["ln_final.weight"].shape[0]
    L = 1 + max(int(k.split(".")[2]) for k in p if k.startswith("transformer.resblocks."))
    vocab = p["token_embedding.weight"].shape[0]
    live_tok = (tokens >= 0) & (tokens < vocab)
    x = torch.where(live_tok[..., None], p["token_embedding.weight"][tokens.clamp(0, vocab - 1)], torch.zeros((), dtype=torch.float64))
    x = x + p["positional_embedding"][None]
    kept = []
    for i in range(L):
        g = lambda name: p["transformer.resblocks.%d.%s" % (i, name)]   # noqa: E731
        h1, xh1, r1 = _ln_parts(x, g("ln_1.weight"), g("ln_1.bias"))
        qkv = h1 @ g("attn.in_proj_weight").T + g("attn.in_proj_bias")
        q, k, v = (t.reshape(B, N, H, HD) for t in qkv.split(W, dim=-1))
        fwd = CB.causal_reference(q, k, v)
        att = fwd["y"].reshape(B, N, W)
        x1 = x + att @ g("attn.out_proj.weight").T + g("attn.out_proj.bias")
        h2, xh2, r2 = _ln_parts(x1, g("ln_2.weight"), g("ln_2.bias"))
        z = h2 @ g("mlp.c_fc.weight").T + g("mlp.c_fc.bias")
        f = z * torch.sigmoid(1.702 * z)
        kept.append((h1, xh1, r1, q, k, v, fwd, att, h2, xh2, r2, z, f))
        x = x1 + f @ g("mlp.c_proj.weight").T + g("mlp.c_proj.bias")
    _, xhf, rf = _ln_parts(x, p["ln_final.weight"], p["ln_final.bias"])
    G = {}
    d, G["ln_final.weight"], G["ln_final.bias"] = _ln_bwd(dout.double(), xhf, rf, p["ln_final.weight"])
    flat = lambda t: t.reshape(B * N, -1)   # noqa: E731
    for i in reversed(range(L)):
        pre = "transformer.resblocks.%d." % i
        g = lambda name: p[pre + name]   # noqa: E731
        h1, xh1, r1, q, k, v, fwd, att, h2, xh2, r2, z, f = kept[i]
        G[pre + "mlp.c_proj.weight"], G[pre + "mlp.c_proj.bias"] = flat(d).T @ flat(f), flat(d).sum(0)
        dz = quick_gelu_grad_ref(z, d @ g("mlp.c_proj.weight"))
        G[pre + "mlp.c_fc.weight"], G[pre + "mlp.c_fc.bias"] = flat(dz).T @ flat(h2), flat(dz).sum(0)
        dn, G[pre + "ln_2.weight"], G[pre + "ln_2.bias"] = _ln_bwd(dz @ g("mlp.c_fc.weight"), xh2, r2, g("ln_2.weight"))
        dx1 = d + dn
        G[pre + "attn.out_proj.weight"], G[pre + "attn.out_proj.bias"] = flat(dx1).T @ flat(att), flat(dx1).sum(0)
        datt = (dx1 @ g("attn.out_proj.weight")).reshape(B, N, H, HD)
        r = causal_bwd_reference(q, k, v, datt, fwd["lse"], fwd["y"])
        dqkv = torch.cat([r[n].reshape(B, N, W) for n in ("dQ", "dK", "dV")], -1)
        G[pre + "attn.in_proj_weight"], G[pre + "attn.in_proj_bias"] = flat(dqkv).T @ flat(h1), flat(dqkv).sum(0)
        dn, G[pre + "ln_1.weight"], G[pre + "ln_1.bias"] = _ln_bwd(dqkv @ g("attn.in_proj_weight"), xh1, r1, g("ln_1.weight"))
        d = dx1 + dn
    G["positional_embedding"] = d.sum(0)
    dtok = torch.zeros(vocab, W, dtype=torch.float64)
    dtok.index_add_(0, tokens[live_tok], d[live_tok])
    G["token_embedding.weight"] = dtok
    return G


def upstream(B, N, W):
    """A closed-form upstream gradient (B, N, W), fp32: every element different, magnitudes near 1, both signs."""
    i = torch.arange(B * N * W, dtype=torch.float64).reshape(B, N, W)
    return (torch.sin(0.37 * i + 0.11) + 0.25 * torch.cos(0.013 * i)).float()


def rel(a, ref):
    a, ref = a.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten()
    return ((a - ref).norm() / ref.norm()).item()


def key_third(name, W):
    """The slice of `attn.in_proj_bias` whose true gradient is exactly zero (the softmax is invariant under a shift of every
    logit of a row, which is what a bias on the keys is), or None for any other parameter."""
    return slice(W, 2 * W) if ".resblocks." in name and name.endswith("attn.in_proj_bias") else None
