"""Static description of a gradient bucket and of the packed payloads exchanged for it.

A *bucket* is a contiguous range of the flat gradient buffer holding whole parameter tensors
(see ``parallel/flat.py``).  Each tensor is cut into *chunks* of ``CHUNK`` = 8192 elements; a chunk
is the unit of work of every encode/decode kernel and the base of the 16-bit sparse indices.

Top-k semantics follow the reference exactly: per tensor, ``k = max(1, int(numel * ratio))``
(``Compresssor/TopK.py:7``).  Selected entries are emitted sorted by index, so an entry is stored as
a chunk-local ``uint16`` offset plus its code, and one ``uint16`` count per chunk says how many
entries each chunk owns.  That is what gets VGG-11 at top-1 % + 8-bit QSGD to ~132x fewer bytes than
dense fp32 instead of the 80x that int32 indices would give.

Dense selections index better with a bitmap: a tensor whose k is above ~1/16 of its elements
(the report's K = 0.4, or small tensors sent whole) stores one bit per element (uint32 words,
``bitmap`` section) instead of 2 bytes per entry; the choice is made per tensor at plan time from
k and numel alone, so every rank still sends the same fixed size.  At K = 0.4 with 8-bit codes
that is 0.525 B per element against the list's 1.2 B and the report's 0.8 B (value + index byte).

Payload layouts (every section starts 16-byte aligned; all ranks send identical sizes, so the
exchange is a fixed-size all-gather with no size handshake):

``topk_qsgd``: scales f32[T] | counts u16[C] | idx u16[K] | codes i8[K] (bits=8) or nibbles[K/2]
``topk``     : scales f32[T] (unused, kept for a uniform header) | counts | idx | values f32[K]
``qsgd``     : scales f32[T] | codes i8[D'] or nibbles  (dense; D' = numels padded to 16 per tensor)
``sign``     : scales f32[C] | bits u32[256 C]  (one scale per chunk; chunk c owns words [256 c,
               256 c + 256), element i of the chunk is bit i & 31 of word i >> 5, padding bits 0)
``vote``     : bits u32[256 C]  (Distributed Lion: the words and bit addressing of ``sign``, no
               scales section; exactly 1024 C bytes)
``mx``       : scales u8[L / 32] | codes u8[L] (bits=8, FP8 E4M3) or nibbles u8[L / 2] (bits=4, FP4
               E2M1; the low nibble is the even element).  L = the bucket's padded length; element
               i of the bucket is code i and its E8M0 scale is byte i >> 5; pads are written as 0
``tern``     : scales f32[T] | codes u32[D' / 16]  (TernGrad; D' as for ``qsgd``, so every tensor
               starts on a word; element i of a tensor is bits 2 (i & 15) .. 2 (i & 15) + 1 of word
               code0 / 16 + (i >> 4); 0 = 0, 1 = +1, 3 = -1, 2 is never written, pad codes are 0)
``intsgd``   : codes i8[L]  (IntSGD; L as for ``mx``; element i of the bucket is byte i, a two's
               complement integer in [-q, q], q = floor(127 / world); pads are written as 0; the
               all-reduce sums the bytes in place)
``thresh``   : counts u16[C] | idx u16[S] | values f32[S]  (threshold-search sparsifier; chunk c owns
               the slots [slot0_c, slot0_c + cap_c) of both sections, S = the sum of cap_c
               (``thresh_slots``); its first counts[c] slots hold the sent entries in increasing
               chunk-local index with their exact fp32 values, the rest index 0 and value +0.0)
"""
from dataclasses import dataclass, field
from typing import List

import math
import os

import torch

from .rng import mix32_int

CHUNK = 8192
BM_WORDS = CHUNK // 32  # bitmap words per chunk
MX_BLOCK = 32  # positions sharing one scale byte (OCP Microscaling v1.0)
# predictive top-k encode (ops/csrc/topk_codec.hip): a tensor keeps at most this many candidates
# (elements at or above its predicted threshold) per step: CAND_K_MULT * k + CAND_SLACK, capped at
# numel; more (or fewer than k) and that tensor takes the exact full-pass path for the step
CAND_K_MULT = 8
CAND_SLACK = 4096
# ... but a tensor of at most this many elements keeps all of them (bound 0, never a miss;
# EWDML_CAND_ALL_MAX, default 0 = off: measured slower, profiles/ab/README.md "Round 6")
CAND_ALL_MAX = int(os.environ.get("EWDML_CAND_ALL_MAX", "0"))


def cand_cap(n: int, k: int) -> int:
    """Candidate-list capacity of a tensor of n elements keeping k."""
    return n if n <= CAND_ALL_MAX else min(n, CAND_K_MULT * k + CAND_SLACK)


def _align(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


@dataclass
class BucketPlan:
    """Tensors of one bucket.  ``offsets`` are element offsets relative to the bucket start."""

    numels: List[int]
    offsets: List[int]
    ratio: float = 1.0
    bucket_offset: int = 0  # element offset of the bucket inside the flat buffer
    length: int = 0  # bucket length in elements (>= last offset + numel; includes align pad)
    # tensors of at most this many elements are sent whole (k = numel): BatchNorm scales/shifts
    # and biases, whose sparsified updates would otherwise arrive once per ~1/ratio steps
    dense_below: int = 0
    # "auto": per tensor, u16 index list or a 1-bit-per-element bitmap, whichever is smaller;
    # "list": always the index list
    index_mode: str = "auto"
    ks: List[int] = field(default_factory=list)
    chunk_tensor: List[int] = field(default_factory=list)
    chunk_start: List[int] = field(default_factory=list)  # relative to bucket start
    chunk_len: List[int] = field(default_factory=list)
    tensor_chunk0: List[int] = field(default_factory=list)
    tensor_nchunks: List[int] = field(default_factory=list)
    tensor_entry0: List[int] = field(default_factory=list)
    tensor_code0: List[int] = field(default_factory=list)  # dense code offset (16-aligned)
    tensor_idx0: List[int] = field(default_factory=list)  # index-list position (-1: bitmap)
    tensor_bm0: List[int] = field(default_factory=list)  # bitmap word offset (-1: index list)
    tensor_cap: List[int] = field(default_factory=list)  # candidate capacity (predictive encode)
    tensor_cap0: List[int] = field(default_factory=list)  # its offset in the candidate list

    def __post_init__(self):
        assert len(self.numels) == len(self.offsets) and self.numels
        if not self.length:
            self.length = self.offsets[-1] + self.numels[-1]
        self.ks = [n if n <= self.dense_below else max(1, int(n * self.ratio))
                   for n in self.numels]
        if self.index_mode not in ("auto", "list"):
            raise ValueError("index_mode must be 'auto' or 'list'")
        e = c = ix = bw = 0
        for t, (n, off) in enumerate(zip(self.numels, self.offsets)):
            nch = (n + CHUNK - 1) // CHUNK
            self.tensor_chunk0.append(len(self.chunk_tensor))
            self.tensor_nchunks.append(nch)
            for j in range(nch):
                self.chunk_tensor.append(t)
                self.chunk_start.append(off + j * CHUNK)
                self.chunk_len.append(min(CHUNK, n - j * CHUNK))
            self.tensor_entry0.append(e)
            e += self.ks[t]
            self.tensor_code0.append(c)
            c += _align(n, 16)
            words = (n + 31) // 32  # chunk j's words start at 256 j: one flat bit per element
            if self.index_mode == "auto" and 4 * words < 2 * self.ks[t]:
                self.tensor_idx0.append(-1)
                self.tensor_bm0.append(bw)
                bw += words
            else:
                self.tensor_idx0.append(ix)
                self.tensor_bm0.append(-1)
                ix += self.ks[t]
        self.total_k = e
        self.total_codes = c
        self.total_idx = ix
        self.total_bm_words = bw
        cap0 = 0
        for n, k in zip(self.numels, self.ks):
            cap = cand_cap(n, k)
            self.tensor_cap.append(cap)
            self.tensor_cap0.append(cap0)
            cap0 += cap
        self.total_cap = cap0

    @property
    def num_tensors(self) -> int:
        return len(self.numels)

    @property
    def num_chunks(self) -> int:
        return len(self.chunk_tensor)

    @property
    def numel(self) -> int:
        return sum(self.numels)

    # ---- device tables consumed by the kernels -------------------------------------------
    @property
    def tensor_cblocks(self) -> List[int]:
        """Blocks per tensor of the predictive encode's candidate passes (one per CHUNK
        candidates of capacity)."""
        return [max(1, (c + CHUNK - 1) // CHUNK) for c in self.tensor_cap]

    @property
    def num_cblocks(self) -> int:
        return sum(self.tensor_cblocks)

    def tensor_table(self, device) -> torch.Tensor:
        """int32 [T, 12]: offset, numel, k, chunk0, nchunks, entry0, code0, idx0, bm0, cap0, cap,
        candidate blocks (csrc/common.h TensorRow)."""
        rows = [[o, n, k, c0, nc, e0, d0, i0, b0, q0, q, nb]
                for o, n, k, c0, nc, e0, d0, i0, b0, q0, q, nb in zip(
                    self.offsets, self.numels, self.ks, self.tensor_chunk0, self.tensor_nchunks,
                    self.tensor_entry0, self.tensor_code0, self.tensor_idx0, self.tensor_bm0,
                    self.tensor_cap0, self.tensor_cap, self.tensor_cblocks)]
        return torch.tensor(rows, dtype=torch.int32, device=device)

    def cblock_table(self, device) -> torch.Tensor:
        """int32 [G, 2]: tensor, block index within the tensor (predictive encode passes)."""
        rows = [[t, j] for t, nb in enumerate(self.tensor_cblocks) for j in range(nb)]
        return torch.tensor(rows, dtype=torch.int32, device=device)

    def thresh_slots(self):
        """Per chunk row of the ``thresh`` codec: (cap, slot0, S).  ``cap[c]`` entries at most are
        sent from chunk c -- the whole chunk where its tensor goes whole (``k == numel``), else
        the chunk's share of the tensor's k, ``max(1, ceil(k * len / numel))`` -- into the slots
        ``[slot0[c], slot0[c] + cap[c])``; ``S`` is their sum."""
        cap = []
        for t, ln in zip(self.chunk_tensor, self.chunk_len):
            k, n = self.ks[t], self.numels[t]
            cap.append(ln if k == n else max(1, (k * ln + n - 1) // n))
        slot0, s = [], 0
        for c in cap:
            slot0.append(s)
            s += c
        return cap, slot0, s

    def thresh_table(self, device) -> torch.Tensor:
        """int32 [C, 2]: cap, slot0 of every chunk row (csrc/thresh_codec.hip int2 slots)."""
        cap, slot0, _ = self.thresh_slots()
        return torch.tensor(list(zip(cap, slot0)), dtype=torch.int32, device=device)

    def chunk_table(self, device) -> torch.Tensor:
        """int32 [C, 4]: tensor, start (rel. bucket), len, local chunk index."""
        rows = []
        for c, (t, s, ln) in enumerate(zip(self.chunk_tensor, self.chunk_start, self.chunk_len)):
            rows.append([t, s, ln, c - self.tensor_chunk0[t]])
        return torch.tensor(rows, dtype=torch.int32, device=device)


@dataclass(frozen=True)
class Layout:
    """Byte offsets of the payload sections for one bucket and one codec."""

    kind: str
    bits: int
    scales: int
    counts: int
    idx: int
    codes: int
    nbytes: int
    bitmap: int = 0  # byte offset of the uint32 bitmap words (top-k kinds)

    @staticmethod
    def build(kind: str, plan: BucketPlan, bits: int = 8) -> "Layout":
        T, C, K = plan.num_tensors, plan.num_chunks, plan.total_k
        scales = 0
        off = _align(4 * T)
        bitmap = 0
        if kind in ("topk_qsgd", "topk"):
            counts = off
            off = _align(off + 2 * C)
            idx = off
            off = _align(off + 2 * plan.total_idx)
            bitmap = off
            off = _align(off + 4 * plan.total_bm_words)
            codes = off
            if kind == "topk":
                off += 4 * K
            else:
                off += K if bits == 8 else (K + 1) // 2
        elif kind == "qsgd":
            counts = idx = off
            codes = off
            off += plan.total_codes if bits == 8 else plan.total_codes // 2
        elif kind == "sign":
            # one scale per chunk, then the chunks' bit words (`codes` is their byte offset)
            bits = 1
            off = _align(4 * C)
            counts = idx = codes = off
            off += 4 * BM_WORDS * C
        elif kind == "vote":
            # the chunks' bit words and nothing else (`codes` is their byte offset): 1024 C bytes
            bits = 1
            scales = counts = idx = codes = 0
            off = 4 * BM_WORDS * C
        elif kind == "mx":
            # one E8M0 scale byte per 32 positions of the padded bucket, then one FP8 / FP4 code
            # per position (`codes` is their byte offset); addressed by the bucket's flat index
            if bits not in (4, 8):
                raise ValueError("the mx codec sends 8-bit (E4M3) or 4-bit (E2M1) elements")
            # every chunk row owns the positions up to the next row's start (the kernels write the
            # pad's zeros from there): tensors packed at the next multiple of 64, as
            # parallel/flat.py lays them out
            L = plan.length
            ends = [_align(o + n, 64) for o, n in zip(plan.offsets, plan.numels)]
            if list(plan.offsets) + [L] != [0] + ends:
                raise ValueError("the mx codec needs a bucket of tensors packed at multiples of 64 "
                                 "elements from offset 0")
            off = _align(L // MX_BLOCK)
            counts = idx = codes = off
            off += L * bits // 8
        elif kind == "intsgd":
            # one int8 code per position of the padded bucket and nothing else: the all-reduce
            # sums the whole payload.  Addressed by the bucket's flat index and packed as for mx
            # (a chunk row owns the positions up to the next row's start)
            bits = 8
            L = plan.length
            ends = [_align(o + n, 64) for o, n in zip(plan.offsets, plan.numels)]
            if list(plan.offsets) + [L] != [0] + ends:
                raise ValueError("the intsgd codec needs a bucket of tensors packed at multiples "
                                 "of 64 elements from offset 0")
            scales = counts = idx = codes = 0
            off = L
        elif kind == "tern":
            # one scaler per tensor, then 2-bit codes, 16 to a word (`codes` is their byte offset)
            bits = 2
            counts = idx = codes = off
            off += plan.total_codes // 4
        elif kind == "thresh":
            # no scales: one count per chunk row, then the chunks' slots -- a u16 chunk-local index
            # and an fp32 value each (`codes` is the values' byte offset)
            bits = 32
            S = plan.thresh_slots()[2]
            counts = 0
            idx = _align(2 * C)
            codes = _align(idx + 2 * S)
            off = codes + 4 * S
        else:
            raise ValueError(kind)
        return Layout(kind, bits, scales, counts, idx, codes, _align(off), bitmap)


MAX_SEGMENTS = 128  # EW_MAX_T in ops/csrc/common.h: the kernels' pointer-table capacity


class TwoStagePlan:
    """One bucket of the two-stage sign all-reduce or vote (``parallel/twostage.py``), cut into one
    shard per rank by ``parallel.sharded.shard_plans``.

    ``plan``: the bucket's *shard-major* plan -- one "tensor" per segment (a tensor crossing a cut
    is two segments, each chunked from its own start), so its chunk list is the shards' chunk
    lists one after the other and one launch covers every shard.  ``shards[r] = (start, length,
    BucketPlan | None, Layout | None, chunk0)``: shard r's own plan (offsets relative to its
    start), its sign layout and its first chunk in ``plan``.

    The exchange's buffers are ``[N, P]`` byte rows, ``P`` the largest shard payload; row r holds
    shard r's payload ``scales f32[C_r] | bits u32[256 C_r]`` from byte 0.  ``slots[c] = (byte
    offset of chunk c's scale, byte offset of its 256 words)`` inside such a buffer -- the same
    table addresses the push rows (row r goes to rank r) and the all-gathered pull rows (row r
    came from owner r).  Row padding and alignment pads are never written.

    ``kind="vote"`` (the two-stage vote, ``TwoStageVoteExchange``): a shard's layout is the vote
    codec's, ``bits u32[256 C_r]`` from byte 0 of its row and nothing else, so ``P = 1024 * max
    C_r``.  ``slots[c]`` keeps its two-int shape so the device table and its checks are shared
    with the sign codec; there is no scale, and both ints are the byte offset of the chunk's
    words (the kernels read the second)."""

    def __init__(self, bucket_plan: BucketPlan, shards, kind: str = "sign"):
        if kind not in ("sign", "vote"):
            raise ValueError(f"two-stage plans are built for the sign or the vote codec, not "
                             f"{kind!r}")
        self.kind = kind
        self.N = len(shards)
        numels, offsets = [], []
        self.shards = []
        c0 = 0
        for s0, ln, sp in shards:
            lay = Layout.build(kind, sp) if sp is not None else None
            self.shards.append((s0, ln, sp, lay, c0))
            if sp is not None:
                numels += sp.numels
                offsets += [s0 + o for o in sp.offsets]
                c0 += sp.num_chunks
        if len(numels) > MAX_SEGMENTS:
            raise ValueError(f"bucket has {len(numels)} tensor segments after sharding (max "
                             f"{MAX_SEGMENTS}): use smaller buckets (--bucket-mb)")
        self.plan = BucketPlan(numels, offsets, 1.0, bucket_plan.bucket_offset,
                               bucket_plan.length)
        assert self.plan.num_chunks == c0
        self.P = max([lay.nbytes for _, _, _, lay, _ in self.shards if lay is not None])
        if self.N * self.P >= 1 << 31:
            raise ValueError("two-stage row buffer of 2 GiB or more: use smaller buckets")
        self.max_shard = max(ln for _, ln, _, _, _ in self.shards)
        self.slots = []
        for r, (_, _, sp, lay, _) in enumerate(self.shards):
            if sp is None:
                continue
            words = [r * self.P + lay.codes + 4 * BM_WORDS * c for c in range(sp.num_chunks)]
            if kind == "vote":
                self.slots += [(w, w) for w in words]
            else:
                self.slots += [(r * self.P + lay.scales + 4 * c, w) for c, w in enumerate(words)]
        self.slot_end = max(w for _, w in self.slots) + 4 * BM_WORDS

    def slot_table(self, device) -> torch.Tensor:
        """int32 [C, 2]: byte offsets of every chunk's scale and words (csrc int2 slots)."""
        return torch.tensor(self.slots, dtype=torch.int32, device=device)


POWERSGD_RANKS = (1, 2, 4, 8)
# torch's powerSGD_hook min_compression_rate: a tensor viewed as [n, m] is compressed when
# n * m >= this * r * (n + m); fixed, decided at plan time
POWERSGD_MIN_COMPRESSION_RATE = 2
PSGD_ROWS = 8192  # elements a project block aims at (its rows: PSGD_ROWS // m, 4..64)
PSGD_COLS = 256  # columns of a back-project / reconstruct tile: one per thread
PSGD_SPLIT_ROWS = 64  # fewest rows of a tile's row split ...
PSGD_MAX_SPLITS = 16  # ... and the most splits per matrix


class LowRankPlan:
    """One bucket of PowerSGD (Vogels et al., NeurIPS 2019; ``parallel/powersgd.py``).

    A tensor of shape ``s`` with ``len(s) >= 2`` is the matrix ``[n, m] = [s[0], numel / s[0]]``
    and is compressed at rank r when ``n * m >= 2 r (n + m)`` (then ``min(n, m) > 2 r``: the
    effective rank is always r); every other tensor is *dense* and travels whole.

    ``mats[t] = (offset in the bucket, n, m, p_off, q_off, index in the bucket)``: the matrix's
    ``[n, r]`` block of the P buffer and its ``[m, r]`` block of the Q buffer, row-major, packed
    one after the other without padding.  ``dense[d] = (offset, numel, tail_off, index)``: the
    dense tensors follow the P blocks in the P buffer (``tail_off`` is an offset into that
    buffer), so they share its all-reduce.  ``p_floats`` = P blocks + dense tail, ``q_floats`` =
    Q blocks.

    Kernel work lists (``ops/csrc/powersgd.hip``): ``row_items`` = (0, matrix, row0, rows) row
    groups of the project launch followed by (1, dense, start, len) copies of at most CHUNK
    elements; ``tile_items`` = (0, matrix, column tile, row split) of the back-project and
    reconstruct launches, followed by the same dense items.  A matrix whose rows are cut into S
    > 1 splits owns S slabs of ``m * r`` floats (``slab_off``) and one arrival counter per column
    tile (``tick_off``)."""

    def __init__(self, bucket_plan: BucketPlan, shapes, rank: int):
        if rank not in POWERSGD_RANKS:
            raise ValueError(f"PowerSGD rank must be one of {POWERSGD_RANKS}, not {rank!r}")
        shapes = [tuple(int(v) for v in s) for s in shapes]
        if len(shapes) != bucket_plan.num_tensors:
            raise ValueError("one shape per tensor of the bucket")
        if bucket_plan.num_tensors > MAX_SEGMENTS:
            raise ValueError(f"bucket has {bucket_plan.num_tensors} tensors (max {MAX_SEGMENTS})")
        self.plan, self.rank, self.shapes = bucket_plan, rank, shapes
        self.mats, self.dense = [], []
        p = q = 0
        for t, (s, off, numel) in enumerate(zip(shapes, bucket_plan.offsets, bucket_plan.numels)):
            n = s[0] if s else 1
            m = numel // max(n, 1)
            if n * m != numel:
                raise ValueError(f"shape {s} does not hold {numel} elements")
            if len(s) >= 2 and n * m >= POWERSGD_MIN_COMPRESSION_RATE * rank * (n + m):
                self.mats.append((off, n, m, p, q, t))
                p += n * rank
                q += m * rank
            else:
                self.dense.append((off, numel, 0, t))
        self.p_factor_floats = p
        for d, (off, numel, _, t) in enumerate(self.dense):
            self.dense[d] = (off, numel, p, t)
            p += numel
        self.p_floats, self.q_floats = p, q
        if max(p, q, 1) >= 1 << 31:
            raise ValueError("PowerSGD factor buffer of 2^31 floats or more: use smaller buckets")
        # work lists
        dense_items = [(1, d, s0, min(CHUNK, numel - s0))
                       for d, (_, numel, _, _) in enumerate(self.dense)
                       for s0 in range(0, numel, CHUNK)]
        self.row_items, self.tile_items, self.split = [], [], []
        slab = tick = 0
        for i, (_, n, m, _, _, _) in enumerate(self.mats):
            rows = max(4, min(64, PSGD_ROWS // m))
            self.row_items += [(0, i, r0, min(rows, n - r0)) for r0 in range(0, n, rows)]
            per = max(PSGD_SPLIT_ROWS, -(-n // PSGD_MAX_SPLITS))
            S, tiles = -(-n // per), -(-m // PSGD_COLS)
            self.split.append((per, S, slab if S > 1 else -1, tick if S > 1 else -1))
            if S > 1:
                slab += S * m * rank
                tick += tiles
            self.tile_items += [(0, i, jt, z) for jt in range(tiles) for z in range(S)]
        self.num_mat_tiles = len(self.tile_items)
        self.row_items += dense_items
        self.tile_items += dense_items
        self.slab_floats, self.num_tickets = slab, tick

    @property
    def compressed(self):
        """Indices (in the bucket) of the compressed tensors."""
        return [t for *_, t in self.mats]

    def mat_table(self, device) -> torch.Tensor:
        """int32 [max(1, T_m), 12]: offset, n, m, p_off, q_off, rows per split, splits, slab_off,
        tick_off, 0, 0, 0 (csrc PsgdMat)."""
        rows = [[off, n, m, p, q, per, S, so, to, 0, 0, 0]
                for (off, n, m, p, q, _), (per, S, so, to) in zip(self.mats, self.split)]
        return torch.tensor(rows or [[0] * 12], dtype=torch.int32, device=device)

    def dense_table(self, device) -> torch.Tensor:
        """int32 [max(1, T_d), 4]: offset, numel, offset in the P buffer, 0 (csrc PsgdDense)."""
        rows = [[off, numel, tail, 0] for off, numel, tail, _ in self.dense]
        return torch.tensor(rows or [[0] * 4], dtype=torch.int32, device=device)

    def row_table(self, device) -> torch.Tensor:
        """int32 [W, 4]: the project launch's work items (one block each)."""
        return torch.tensor(self.row_items, dtype=torch.int32, device=device)

    def tile_table(self, device) -> torch.Tensor:
        """int32 [W, 4]: the back-project (first ``num_mat_tiles``) and reconstruct items."""
        return torch.tensor(self.tile_items, dtype=torch.int32, device=device)


SKETCH_ROWS = (1, 3, 5)  # odd: the median of a coordinate's row values is one of them
# summation order of a count-sketch table entry (ops/csrc/sketch_codec.hip k_sketch_accum and
# compress/oracle.py sketch_accumulate): chunks in groups of this many consecutive chunk indices
SKETCH_SUM_GROUP = 64


class SketchPlan:
    """One bucket of the count-sketch exchange (``parallel/sketch.py``; SketchedSGD, Ivkin et al.,
    NeurIPS 2019) over the bucket's top-k ``BucketPlan``.

    A tensor with ``k == numel`` is *dense*: it is not sketched, always selected whole and keeps
    no residual.  ``K`` = the sum of ``k`` over the sketched tensors and the table has ``rows``
    rows of ``W = CHUNK * max(1, ceil(width * K / CHUNK))`` fp32 columns (``W >= CHUNK``: two
    elements of one chunk never share a column).

    The hash is a per-chunk rotation.  In row ``j`` chunk ``c`` (its index in the bucket) is
    shifted by ``shifts[j][c] = (mix32((c * 8 + j) ^ sk_key) * W) >> 32`` and its element at
    chunk-local position ``p`` lands in column ``(p + shifts[j][c]) mod W`` with the sign bit
    ``j`` of ``mix32(gidx ^ sg_key)``, ``gidx = bucket_offset + offset`` (the QSGD streams'
    index).  ``set_shift`` overrides one shift (the tests' wrap and no-wrap edges).

    ``chunk_rows[c] = (start, len)`` with ``len = 0`` for the chunks of dense tensors."""

    def __init__(self, bucket_plan: BucketPlan, rows: int, width: float, sk_key: int,
                 sg_key: int):
        if rows not in SKETCH_ROWS:
            raise ValueError(f"sketch rows must be one of {SKETCH_ROWS}, not {rows!r}")
        if not float(width) > 0.0:
            raise ValueError(f"sketch width must be > 0, not {width!r}")
        if bucket_plan.num_tensors > MAX_SEGMENTS:
            raise ValueError(f"bucket has {bucket_plan.num_tensors} tensors (max {MAX_SEGMENTS})")
        self.plan, self.rows, self.width = bucket_plan, int(rows), float(width)
        self.sk_key, self.sg_key = sk_key & 0xFFFFFFFF, sg_key & 0xFFFFFFFF
        p = bucket_plan
        self.dense = [k == n for k, n in zip(p.ks, p.numels)]
        self.sketched = [t for t, d in enumerate(self.dense) if not d]
        self.K = sum(p.ks[t] for t in self.sketched)
        self.dense_elems = sum(n for n, d in zip(p.numels, self.dense) if d)
        self.W = CHUNK * max(1, math.ceil(self.width * self.K / CHUNK))
        if self.rows * self.W >= 1 << 31:
            raise ValueError("sketch table of 2^31 floats or more: use smaller buckets")
        self.table_floats = self.rows * self.W
        self.chunk_rows = [(s, 0 if self.dense[t] else ln) for t, s, ln in
                           zip(p.chunk_tensor, p.chunk_start, p.chunk_len)]
        self.shifts = [[(mix32_int((c * 8 + j) ^ self.sk_key) * self.W) >> 32
                        for c in range(p.num_chunks)] for j in range(self.rows)]

    def set_shift(self, row: int, chunk: int, shift: int):
        if not 0 <= shift < self.W:
            raise ValueError("a shift is a column of the table")
        self.shifts[row][chunk] = int(shift)

    @property
    def payload_floats(self) -> int:
        """fp32 values the two all-reduces move: the table and one value per selected element."""
        return self.table_floats + self.K + self.dense_elems

    def row_table(self, device) -> torch.Tensor:
        """int32 [C, 2]: start (rel. bucket), sketched length (0: a dense tensor's chunk)."""
        return torch.tensor(self.chunk_rows, dtype=torch.int32, device=device)

    def shift_table(self, device) -> torch.Tensor:
        """int32 [R, C]: the column shift of every chunk in every row."""
        return torch.tensor(self.shifts, dtype=torch.int32, device=device)
