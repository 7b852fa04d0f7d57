"""Caption bank: the frozen CLIP tower's output per caption string, computed once and kept on the device.

Captions come from a small fixed table, the tower is frozen, so its output for a caption is a constant of the run.  The bank
keeps `feat` (capacity + spill, N, W) fp32 and `eot` (capacity + spill,) int64 on the device and a host dict caption -> slot.
A step asks `bank.batch(captions)`: misses are sent through `MotionTransformer._clip_features` (whatever route that takes) in
chunks of exactly FILL_CHUNK captions padded with "", so the tower always sees one shape and a caption's row is the same
bits whichever step first met it.  The answer is a `CaptionBatch`: int32 index arrays, packed in one buffer and uploaded with
one copy, from which hig_caption_gather fetches the rows (csrc/textrows.hip) -- per model row, or per DISTINCT caption with the
inverted index that expands the text head's output and sums its upstream gradients back (`text_dedup`).

There is no eviction: when the persistent slots are full, the misses of a request go to the transient slots behind them and
are recomputed each time; the step still makes one gather over one buffer.  The buffers are allocated once at their full
size, so a pointer that a captured graph holds stays valid while the bank fills.

The bank refuses a tower with a trainable parameter and cap_id models (ValueError), and empties itself when the tower may have
changed: the model's `_apply` / `_load_from_state_dict`, a moved sum of the tower parameters' `_version`, a changed
`clip_tower` flag or tokenizer.
"""
import torch

from .. import _lib

FILL_CHUNK = 8      # captions per tower call of a fill, padded with ""
DEFAULT_SPILL = 64  # transient slots behind the persistent ones


def padded_unique(U):
    """U rounded up to a power of two, at least 8: the captured step then needs only a handful of graph shapes."""
    p = 8
    while p < U:
        p *= 2
    return p


class CaptionBatch:
    """The index arrays of one request, all int32, views of ONE packed buffer `dev` (`host` is its host twin):
        slot       (rows,)       bank slot of every model row
        uniq_slot  (U_pad,)      bank slot of every distinct caption, in order of first appearance; padding repeats uniq_slot[0]
        inv        (rows,)       row -> index of its caption in uniq_slot
        order, seg (rows,), (U_pad + 1,)   CSR of inv: the rows of distinct caption u are order[seg[u]:seg[u + 1]], ascending;
                                 padding entries have empty segments, so their upstream gradient is exactly zero
        U          the number of distinct captions (also the last element of the buffer)
    The layout depends on (rows, U_pad) alone: a captured step copies `dev` into its static twin."""

    def __init__(self, rows, U, U_pad, host, dev):
        self.rows, self.U, self.U_pad, self.host, self.dev = rows, U, U_pad, host, dev
        for name, (lo, hi) in self.layout(rows, U_pad).items():
            setattr(self, name, dev[lo:hi])
            setattr(self, name + "_host", host[lo:hi])

    @staticmethod
    def layout(rows, U_pad):
        out, o = {}, 0
        for name, n in (("slot", rows), ("uniq_slot", U_pad), ("inv", rows), ("order", rows), ("seg", U_pad + 1)):
            out[name] = (o, o + n)
            o += n
        return out

    @staticmethod
    def numel(rows, U_pad):
        return 3 * rows + 2 * U_pad + 2

    def on_buffer(self, dev):
        """The same request read from another device buffer of the same layout (the static input of a captured step)."""
        assert dev.shape == self.dev.shape and dev.dtype == torch.int32
        return CaptionBatch(self.rows, self.U, self.U_pad, self.host, dev)


class CaptionBank:

    def __init__(self, model, capacity, spill=DEFAULT_SPILL):
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError("CaptionBank: capacity must be a positive int, got %r" % (capacity,))
        if getattr(model, "cap_id", False) or not hasattr(model, "clip"):
            raise ValueError("CaptionBank: a cap_id model takes class embeddings, there is no CLIP tower to bank")
        if any(p.requires_grad for p in model.clip.parameters()):
            raise ValueError("CaptionBank: the CLIP tower has trainable parameters (no_clip=True): its output is not a constant "
                             "of the run")
        self.model, self.capacity, self.spill = model, int(capacity), int(spill)
        self.N, self.W = (int(v) for v in model.clip.positional_embedding.shape)
        self.feat = self.eot = None
        self.slots = {}
        self.chunk_of = {}           # caption -> (the FILL_CHUNK captions of the tower call that made its row, its position)
        self.stats = dict(hits=0, misses=0, tower_calls=0, tokenizer_calls=0, overflow_rows=0, fills=0)
        self._sig = None

    # ---- validity ----------------------------------------------------------------------------------------------------
    def clear(self):
        """Forget every caption (the buffers stay: a captured graph may hold their pointers)."""
        self.slots, self.chunk_of, self._sig = {}, {}, None

    def __len__(self):
        return len(self.slots)

    def _signature(self):
        m = self.model
        return (sum(p._version for p in m.clip.parameters()), any(p.requires_grad for p in m.clip.parameters()), m.clip_tower,
                m._clip_tokenize)

    def _validate(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        sig = self._signature()
        if sig[1]:
            raise ValueError("CaptionBank: the CLIP tower has become trainable: its output is no longer a constant of the run")
        if self._sig is not None and (sig[0] != self._sig[0] or sig[2] != self._sig[2] or sig[3] is not self._sig[3]):
            self.clear()
        if self.feat is None or self.feat.device != device:
            self.clear()
            n = self.capacity + self.spill
            self.feat = torch.zeros(n, self.N, self.W, device=device, dtype=torch.float32)
            self.eot = torch.zeros(n, device=device, dtype=torch.int64)
        self._sig = sig
        return device

    # ---- fills (off the hot path) --------------------------------------------------------------------------------------
    def _fill(self, captions, slots, device):
        """Rows of `captions` through the tower into `slots`, FILL_CHUNK at a time."""
        for lo in range(0, len(captions), FILL_CHUNK):
            part = list(captions[lo:lo + FILL_CHUNK])
            chunk = tuple(part + [""] * (FILL_CHUNK - len(part)))
            tokens, x = self.model._clip_features(list(chunk), device)
            self.stats["tower_calls"] += 1
            self.stats["tokenizer_calls"] += 1
            self.stats["fills"] += 1
            rows = x.detach().permute(1, 0, 2).float()
            e = tokens.argmax(dim=-1)
            for i, (c, s) in enumerate(zip(part, slots[lo:lo + FILL_CHUNK])):
                self.feat[s].copy_(rows[i])
                self.eot[s].copy_(e[i])
                self.chunk_of[c] = (chunk, i)

    # ---- a request -----------------------------------------------------------------------------------------------------
    def batch(self, captions, device=None):
        """Index arrays for the model batch whose row r has caption captions[r]; fills what the bank does not hold yet."""
        captions = list(captions)
        rows = len(captions)
        if rows == 0:
            raise ValueError("CaptionBank.batch: no captions")
        if not all(isinstance(c, str) for c in captions):
            raise TypeError("CaptionBank.batch: captions must be strings")
        device = self._validate(device if device is not None else next(self.model.text_ln.parameters()).device)
        index, uniq, inv = {}, [], []
        for c in captions:
            u = index.get(c)
            if u is None:
                u = index[c] = len(uniq)
                uniq.append(c)
            inv.append(u)
        U = len(uniq)
        missing = [c for c in uniq if c not in self.slots]
        keep = missing[:self.capacity - len(self.slots)]
        over = missing[len(keep):]
        if len(over) > self.spill:
            raise RuntimeError("CaptionBank: %d captions of one request do not fit (%d slots are full, %d transient slots): raise "
                               "the capacity" % (len(over), self.capacity, self.spill))
        new_slots = list(range(len(self.slots), len(self.slots) + len(keep)))
        transient = {c: self.capacity + k for k, c in enumerate(over)}
        count = [0] * U
        for u in inv:
            count[u] += 1
        self.stats["misses"] += len(keep)
        self.stats["overflow_rows"] += sum(count[index[c]] for c in over)
        self.stats["hits"] += rows - sum(count[index[c]] for c in missing)
        if missing:
            self._fill(keep + over, new_slots + [transient[c] for c in over], device)
            self.slots.update(zip(keep, new_slots))
        uniq_slot = [self.slots[c] if c in self.slots else transient[c] for c in uniq]
        U_pad = padded_unique(U)
        seg = [0] * (U_pad + 1)
        for u in range(U):
            seg[u + 1] = seg[u] + count[u]
        for u in range(U, U_pad):
            seg[u + 1] = rows
        order, cursor = [0] * rows, seg[:U]
        for r, u in enumerate(inv):
            order[cursor[u]] = r
            cursor[u] += 1
        packed = [uniq_slot[u] for u in inv] + uniq_slot + [uniq_slot[0]] * (U_pad - U) + inv + order + seg + [U]
        assert len(packed) == CaptionBatch.numel(rows, U_pad)
        host = torch.tensor(packed, dtype=torch.int32)
        if device.type == "cuda":
            host = host.pin_memory()
        return CaptionBatch(rows, U, U_pad, host, host.to(device, non_blocking=True))

    # ---- launches ------------------------------------------------------------------------------------------------------
    def gather(self, slot, n):
        """hig_caption_gather: (clip_out (n, N, W), eot (n,)) of the n bank slots in the device int32 array `slot`."""
        clip_out = torch.empty(n, self.N, self.W, device=self.feat.device, dtype=torch.float32)
        eot = torch.empty(n, device=self.feat.device, dtype=torch.int64)
        _lib.api.hig_caption_gather(self.feat, self.eot, self.feat.shape[0], slot, n, self.N * self.W, clip_out, eot)
        return clip_out, eot


def expand_rows(src, idx, n_out):
    """hig_rows_gather_f32: out[r] = src[idx[r]] over the leading dimension (src contiguous fp32, idx device int32)."""
    assert src.is_contiguous() and src.dtype == torch.float32
    out = torch.empty((n_out,) + tuple(src.shape[1:]), device=src.device, dtype=torch.float32)
    _lib.api.hig_rows_gather_f32(src, src.shape[0], idx, n_out, src[0].numel(), out)
    return out


def segment_sum_rows(src, order, seg, n_seg):
    """hig_rows_segment_sum_f32: out[u] = the rows order[seg[u]:seg[u + 1]] of src added in that order."""
    assert src.is_contiguous() and src.dtype == torch.float32
    out = torch.empty((n_seg,) + tuple(src.shape[1:]), device=src.device, dtype=torch.float32)
    _lib.api.hig_rows_segment_sum_f32(src, src.shape[0], order, seg, n_seg, src[0].numel(), out)
    return out
