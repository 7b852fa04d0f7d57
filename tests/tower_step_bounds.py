"""Restatements, cases and gates of the tower-in-the-step tests (tests/test_cpu_tower_step.py, tests/test_gpu_tower_step.py):
the CLIP text tower trained by the fused / captured step (clip_tower_train="flat", trainers/text_source.py: Tokens) and the
embedding index built on the device (csrc/clipindex.hip).

Nothing here comes from what the code under test gives:
  * `token_batch_restated` states clip_text.TokenBatch's arrays from the captions alone: distinct captions in order of first
    appearance, U rounded up to a power of two (at least 8), padding = the first distinct caption with an empty segment;
  * `capacity_restated` states hig_clip_embed_index_build's result from the tokens alone (include/hig.h): rows grouped by id,
    ids ascending, rows ascending inside an id, lists cut every HIG_CLIP_EMBED_CHUNK rows, in the capacity layout whose offsets
    depend on (B, N, vocab) only.  Entries beyond the live prefix are unspecified: the restatement leaves a sentinel there and the
    tests compare live prefixes;
  * the index is integer work and the embedding gradient is DEFINED as one fp32 sum (clip_text.embed_grad_restated), so both are
    held bit for bit; the bound of the step's tests is the one the issue sets, restated at each test.

Gates of the step (the ones the CLIP-training and caption-bank sections already use):
  LOSS_REL       1e-5: fused step without dedup against forward() + update() under clip_tower_train="hip", per step;
  update gate    total update of every parameter over the steps: rel-L2 distance from an fp64 run <= 4 x the distance of the fp32
                 torch route (forward() + update() on torch ops) from the same fp64 run;
  dedup gate     per parameter: rel-L2 from fp64 with dedup <= max(1e-6, 4 x that without dedup).
The key third [W:2W] of every attn.in_proj_bias is left out of the two update gates, and nothing else is: its true gradient is
exactly zero (a bias on the keys shifts every logit of a row by the same amount and softmax is shift-invariant), so every fp32
route holds rounding noise there, which Adam's division by sqrt(v) amplifies to full-size steps of random sign.
"""
import numpy as np
import torch

LOSS_REL = 1e-5
UPDATE_FACTOR = 4.0
DEDUP_FLOOR, DEDUP_FACTOR = 1e-6, 4.0
SENTINEL = -7
MAX_ROWS, MAX_VOCAB = 65535, 65536      # what the keys id << 16 | row cover (include/hig.h)
SORT_TILE = 32768                       # keys sorted in LDS at a time: the one capacity boundary of the sort


def padded_unique_restated(U):
    p = 8
    while p < U:
        p *= 2
    return p


def token_batch_restated(captions, tokenize, dedup=True):
    """{tokens (U_pad, N), eot (U_pad,), inv (rows,), order (rows,), seg (U_pad + 1,), U, U_pad} from the captions alone."""
    rows = len(captions)
    if dedup:
        uniq = []
        for c in captions:
            if c not in uniq:
                uniq.append(c)
        U, U_pad = len(uniq), padded_unique_restated(len(uniq))
        inv = [uniq.index(c) for c in captions]
    else:
        uniq, U, U_pad, inv = list(captions), rows, rows, list(range(rows))
    members = [[r for r in range(rows) if inv[r] == u] for u in range(U)] + [[] for _ in range(U_pad - U)]
    seg = np.concatenate([[0], np.cumsum([len(m) for m in members])])
    tokens = tokenize(uniq + [uniq[0]] * (U_pad - U)).numpy().astype(np.int64)
    return dict(tokens=tokens, eot=tokens.argmax(axis=1), inv=np.array(inv), order=np.array(sum(members, []), dtype=np.int64),
                seg=seg, U=U, U_pad=U_pad)


def capacity_restated(tokens, vocab, chunk):
    """-> (counts (n_live, n_chunks, n_ids), {name: int64 array of its CAPACITY, SENTINEL beyond the live prefix}, total ints)."""
    tok = np.asarray(tokens, dtype=np.int64)
    B, N = tok.shape
    M = B * N
    cap_ids = min(M, vocab)
    cap_chunks = (M + chunk - 1) // chunk + cap_ids
    flat = tok.reshape(-1)
    lists = {}
    for r in range(M):
        if 0 <= flat[r] < vocab:
            lists.setdefault(int(flat[r]), []).append(r)
    order, chunk_seg, id_seg, ids = [], [], [], []
    for t in sorted(lists):
        ids.append(t)
        id_seg.append(len(chunk_seg))
        for lo in range(0, len(lists[t]), chunk):
            chunk_seg.append(len(order) + lo)
        order += lists[t]
    n_live, n_chunks, n_ids = len(order), len(chunk_seg), len(ids)
    chunk_seg.append(n_live)
    id_seg.append(n_chunks)
    assert n_ids <= cap_ids and n_chunks <= cap_chunks

    def cap(values, n):
        out = np.full(n, SENTINEL, dtype=np.int64)
        out[:len(values)] = values
        return out
    arrays = dict(order=cap(order, M), chunk_seg=cap(chunk_seg, cap_chunks + 1), chunk_order=cap(list(range(n_chunks)), cap_chunks),
                  id_seg=cap(id_seg, cap_ids + 1), ids=cap(ids, cap_ids),
                  pos_order=np.array([b * N + n for n in range(N) for b in range(B)], dtype=np.int64).reshape(-1),
                  pos_seg=np.arange(N + 1, dtype=np.int64) * B)
    total = sum(len(a) for a in arrays.values())
    return (n_live, n_chunks, n_ids), arrays, total


def live_lengths(counts, B, N):
    n_live, n_chunks, n_ids = counts
    return dict(order=n_live, chunk_seg=n_chunks + 1, chunk_order=n_chunks, id_seg=n_ids + 1, ids=n_ids, pos_order=B * N, pos_seg=N + 1)


# ---- token patterns of the index tests ---------------------------------------------------------------------------------------------
def pattern(kind, B, N, vocab, seed=0):
    """(B, N) int64 tokens.  captions: what a tokenizer gives -- a few words, then token 0 pads (one id's list of many chunks);
    distinct: no id twice (as far as vocab allows); equal: one id; mixed: ids -1 and `vocab` among random ones."""
    g = np.random.RandomState(seed)
    M = B * N
    if kind == "captions":
        tok = np.zeros((B, N), dtype=np.int64)
        for b in range(B):
            ids = ([vocab - 2] + list(1 + g.randint(0, max(vocab - 3, 1), g.randint(0, 12))) + [vocab - 1])[:N]
            tok[b, :len(ids)] = ids
        return np.clip(tok, 0, vocab - 1)      # (the stub tokenizer's shape: SOT, word ids, EOT, zeros)
    if kind == "distinct":
        return (g.permutation(max(M, vocab))[:M] % vocab).reshape(B, N).astype(np.int64)
    if kind == "equal":
        return np.full((B, N), vocab // 2, dtype=np.int64)
    if kind == "mixed":
        tok = g.randint(0, vocab, (B, N)).astype(np.int64)
        flat = tok.reshape(-1)
        flat[g.permutation(M)[:max(1, M // 5)]] = -1
        flat[g.permutation(M)[:max(1, M // 7)]] = vocab
        return tok
    raise KeyError(kind)


# ---- the step's gates -----------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return ((a - b).norm() / b.norm()).item()


def key_third(name, numel):
    """Index range of the key third of an attn.in_proj_bias -- the CLIP tower's (`clip. ... .attn.in_proj_bias`) and the text head's
    (`textTransEncoder. ... .self_attn.in_proj_bias`) -- of `numel` = 3 W entries, else None."""
    if name.endswith("attn.in_proj_bias"):
        assert numel % 3 == 0
        return slice(numel // 3, 2 * numel // 3)
    return None


def without_key_third(name, *tensors):
    """The tensors flattened, the key third cut out of an attn.in_proj_bias; anything else as it is."""
    third = key_third(name, tensors[0].numel())
    if third is None:
        return tuple(t.reshape(-1) for t in tensors)
    keep = torch.ones(tensors[0].numel(), dtype=torch.bool)
    keep[third] = False
    return tuple(t.reshape(-1)[keep] for t in tensors)
