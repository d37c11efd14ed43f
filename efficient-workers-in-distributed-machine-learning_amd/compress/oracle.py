"""Pure-torch reference implementations of every codec (the "oracle").

These define the exact semantics the HIP kernels in ``ops/csrc`` implement; on CPU (Gloo tests,
``BASELINE.json`` config #1) they are also the execution path.  The HIP kernels reproduce them
bit-for-bit for the top-k selection, the codes and the decoded sums (the kernel file is compiled
with ``-ffp-contract=off`` so no FMA changes a rounding); only L2 norms may differ in the last bit
because the GPU sums squares in a different (but fixed) order.

Reference semantics being reproduced:
  * QSGD (``Compresssor/qsgd.py:12-40``): level = floor(s*|g|/norm) + Bernoulli(frac), code =
    sign*level, decode = norm/s*code.  Differences, all deliberate:
    codes are real int8/int4 (the reference ships fp32 "levels"), s <= 127 so the code fits int8
    (the reference's s=128 overflows), a zero norm yields zeros instead of NaN, and the uniform
    variates come from the counter RNG in ``rng.py``.
  * Top-k (``Compresssor/TopK.py:5-35``): k = max(1, int(numel*ratio)) largest |g| per tensor.  Ties
    at the threshold are broken by lowest index (torch.topk leaves them unspecified), entries are
    stored sorted by index.
  * Scaled sign with error feedback (no reference counterpart; 1-bit SGD, Seide et al. 2014, and
    EF-signSGD, Karimireddy et al. 2019): per 8192-element chunk the mean |g + residual| and one
    bit per element.  The chunk sum is written in the kernel's own order (``_sign_chunk_sums``),
    so scales, bits and residuals are bitwise the kernel's.  With ``rot_key`` the signs are taken
    of a randomised Hadamard rotation of every chunk (DRIVE / EDEN, Vargaftik et al. 2021 / 2022;
    ``fwht``, ``hsign_flip``): the butterfly stages run in the kernel's order, bitwise again.
  * 1-bit Adam's compressed stage (no reference counterpart; Tang et al., ICML 2021):
    ``encode_sign_momentum`` (the sign encode of the error-compensated momentum candidate) and
    ``onebit_adam_apply`` (averaged momentum, frozen-variance step), bitwise the kernels'.
  * 1-bit LAMB's compressed stage (no reference counterpart; Li et al., 2021): the same sender
    with weight decay 0 and ``onebit_lamb_apply`` (averaged momentum, fresh variance, per-tensor
    factor on the frozen trust ratio), bitwise the kernels'.
  * Block floating point (no reference counterpart; OCP Microscaling v1.0, Rouhani et al. 2023):
    ``encode_mx`` -- one power-of-two scale byte per 32 elements, FP8 E4M3 or FP4 E2M1 elements
    rounded to nearest even and saturated, with error feedback; bitwise the kernels'.
  * TernGrad (no reference counterpart: ``SURVEY.md`` section 4 records an attempt that did not
    build; Wen et al., NeurIPS 2017): ``encode_tern`` -- stochastic ternary codes at 2 bits per
    element, one fp32 scaler per tensor clipped at ``clip`` times the tensor's root mean square
    (about zero, not about the mean); the sum of squares runs in the kernel's order
    (``_tern_sumsq``), so scalers, codes and residuals are bitwise the kernels'.
  * Count sketch (no reference counterpart; SketchedSGD, Ivkin et al., NeurIPS 2019): ``sketch_*``
    -- the table of the error-compensated gradient under a per-chunk rotation hash, summed in the
    kernel's one order, the median estimate and the gather of the selected coordinates; bitwise
    the kernels'.
  * Threshold-search sparsification (no reference counterpart; RedSync, Fang et al. 2019; MSTopK,
    Shi et al. 2021; hard-threshold sparsification, Sahu et al. 2021): ``encode_thresh`` -- per
    8192-element chunk everything at or above a canonical bf16-level threshold, with plain error
    feedback; the threshold does not depend on how it is searched, so payloads and residuals are
    bitwise the kernels'.
  * IntSGD (no reference counterpart; Mishchenko et al., ICLR 2022): ``encode_intsgd`` --
    stochastic int8 codes of ``g * alpha`` clamped to ``floor(127 / N)``, summed by all-reduce --
    ``intsgd_apply`` and the scale rule ``intsgd_alpha``, whose sums run in the kernels' order;
    bitwise the kernels'.
"""
import numpy as np
import torch

from . import rng
from .plan import CHUNK, BucketPlan, Layout


def _section(buf: torch.Tensor, start: int, count: int, dtype: torch.dtype) -> torch.Tensor:
    nbytes = count * torch.empty((), dtype=dtype).element_size()
    return buf[start:start + nbytes].view(dtype)


def topk_indices(x: torch.Tensor, k: int) -> torch.Tensor:
    """Sorted int64 indices of the k largest |x| (ties -> lowest index)."""
    n = x.numel()
    if k >= n:
        return torch.arange(n, dtype=torch.int64, device=x.device)
    key = x.abs().contiguous().view(torch.int32)
    kth = torch.topk(key, k, sorted=False).values.min()
    gt = key > kth
    need = k - int(gt.sum())
    sel = gt.clone()
    if need > 0:
        sel[(key == kth).nonzero().flatten()[:need]] = True
    return sel.nonzero().flatten()


def inv_scale(levels: int, scale: float) -> float:
    """fp32 ``levels / scale`` (0 for a zero scale), rounded exactly like the kernels' IEEE divide."""
    scale = np.float32(scale)
    if not scale > 0:
        return 0.0
    return float(np.float32(levels) / scale)


def dequant_step(levels: int, scale: float) -> float:
    """fp32 ``scale * fp32(1/levels)``: the value of one code unit."""
    return float(np.float32(scale) * np.float32(1.0 / levels))


def quantize(vals: torch.Tensor, scale: float, levels: int, gidx: torch.Tensor,
             key: int) -> torch.Tensor:
    """Stochastic QSGD rounding of ``vals`` against ``scale`` -> int32 codes in [-levels, levels]."""
    lvl = vals.abs() * inv_scale(levels, scale)
    fl = torch.floor(lvl)
    u = rng.uniform(gidx, key)
    q = fl + (u < (lvl - fl)).to(torch.float32)
    q = torch.clamp(q, max=float(levels))
    q = torch.where(vals < 0, -q, q)
    return q.to(torch.int32)


def _pack4(codes: torch.Tensor) -> torch.Tensor:
    c = (codes & 0xF).to(torch.uint8)
    if c.numel() % 2:
        c = torch.cat([c, c.new_zeros(1)])
    return c[0::2] | (c[1::2] << 4)


def _unpack4(b: torch.Tensor, n: int) -> torch.Tensor:
    lo = (b & 0xF).to(torch.int32)
    hi = (b >> 4).to(torch.int32)
    c = torch.stack([lo, hi], 1).flatten()[:n]
    return torch.where(c >= 8, c - 16, c)


def _scale_of(vals: torch.Tensor, norm: str) -> float:
    if vals.numel() == 0:
        return 0.0
    if norm == "max":
        return float(vals.abs().max())
    if norm == "l2":
        return float(np.float32(vals.to(torch.float64).norm()))
    raise ValueError(f"unknown QSGD norm {norm!r}")


# ---------------------------------------------------------------------------------------------
# error feedback with momentum correction (DGC)
# ---------------------------------------------------------------------------------------------
def dgc_accumulate(g: torch.Tensor, residual: torch.Tensor, velocity: torch.Tensor, momentum: float,
                   dampening: float = 0.0, nesterov: bool = False, weight_decay: float = 0.0,
                   param: torch.Tensor = None, lr: float = None) -> torch.Tensor:
    """Momentum correction of Deep Gradient Compression (Lin et al., ICLR 2018): the momentum is
    applied on the worker *before* sparsification and the residual accumulates the velocity,
    not the raw gradient.  Updates ``velocity`` in place and returns ``residual + d`` (the vector
    to compress), with (every product and sum rounded to fp32 separately, as the kernels do)::

        g' = g + wd * p                    (weight decay folded in locally)
        u  = m * u + (1 - dampening) * g'
        d  = g' + m * u  (Nesterov)  |  u
        e  = residual + d

    The receiver then applies ``p -= lr * mean(sent)`` with no second momentum.  Plain error
    feedback with the momentum after the decode (``--ef-mode plain``) lets the residual hold ~99 %
    of the gradient mass, which the post-decode momentum later amplifies: ResNet-50's loss spikes
    far above chance (VERDICT r2 Weak #1)."""
    f32 = np.float32
    if weight_decay != 0.0:
        g = g + param * float(f32(weight_decay))
    velocity.copy_(velocity * float(f32(momentum)) + g * float(f32(1.0 - dampening)))
    d = g + velocity * float(f32(momentum)) if nesterov else velocity
    if lr is not None:  # error feedback on the update (lr inside): --ef-mode local
        d = d * float(f32(lr))
    return residual + d


# ---------------------------------------------------------------------------------------------
# encode
# ---------------------------------------------------------------------------------------------
def encode_topk(g: torch.Tensor, plan: BucketPlan, layout: Layout, levels: int, norm: str,
                key: int, residual: torch.Tensor = None, dgc: dict = None,
                ef21: bool = False) -> torch.Tensor:
    """Top-k (+QSGD when ``layout.kind == 'topk_qsgd'``) of one bucket -> uint8 payload.

    ``g`` is the bucket's flat fp32 gradient (length ``plan.length``).  With ``residual`` (error
    feedback) the compressed vector is ``g + residual`` and ``residual`` is overwritten with what was
    not transmitted.  With ``dgc`` (``{velocity, momentum, dampening, nesterov, weight_decay,
    param}``: momentum correction, :func:`dgc_accumulate`) the compressed vector is ``residual +
    d`` and the velocity is cleared at the transmitted coordinates (momentum factor masking;
    ``dgc["mask"] = False`` keeps it, and ``dgc["lr"]`` accumulates lr-scaled updates).  With
    ``ef21`` (EF21, Richtarik et al. 2021) ``residual`` is this rank's running gradient estimate
    h: the compressed vector is ``g - h`` and ``h += sent``; the receivers add the average of
    the sent vectors to the global estimate and step on that (``parallel/engine.py``).
    """
    vel = None
    g_in = g
    if dgc is not None:
        vel = dgc["velocity"] if dgc.get("mask", True) else None
        g = dgc_accumulate(g, residual, dgc["velocity"], dgc["momentum"],
                           dgc.get("dampening", 0.0), dgc.get("nesterov", False),
                           dgc.get("weight_decay", 0.0), dgc.get("param"), dgc.get("lr"))
    elif ef21:
        g = g - residual
    elif residual is not None:
        g = g + residual
    out = torch.zeros(layout.nbytes, dtype=torch.uint8, device=g.device)
    T, C, K = plan.num_tensors, plan.num_chunks, plan.total_k
    scales = _section(out, layout.scales, T, torch.float32)
    counts = _section(out, layout.counts, C, torch.int16)
    idx = _section(out, layout.idx, plan.total_idx, torch.int16)
    bm = _section(out, layout.bitmap, plan.total_bm_words, torch.int32)
    codes_all = []
    sent = torch.zeros_like(g) if residual is not None else None
    for t in range(T):
        off, n, k = plan.offsets[t], plan.numels[t], plan.ks[t]
        x = g[off:off + n]
        sel = topk_indices(x, k)
        vals = x[sel]
        if vel is not None:
            vel[off + sel] = 0.0
        c0, nch = plan.tensor_chunk0[t], plan.tensor_nchunks[t]
        counts[c0:c0 + nch] = torch.bincount(sel // CHUNK, minlength=nch).to(torch.int16)
        if plan.tensor_bm0[t] >= 0:  # one bit per element, flat over the tensor's chunks
            words = torch.zeros((n + 31) // 32, dtype=torch.int64, device=g.device)
            words.index_add_(0, sel // 32, torch.ones_like(sel) << (sel % 32))
            words = ((words + (1 << 31)) % (1 << 32)) - (1 << 31)  # uint32 bits as int32
            w0 = plan.tensor_bm0[t]
            bm[w0:w0 + words.numel()] = words.to(torch.int32)
        else:
            i0 = plan.tensor_idx0[t]
            idx[i0:i0 + k] = (sel % CHUNK).to(torch.int16)
        scale = _scale_of(vals, norm)
        scales[t] = scale  # plain top-k keeps the scale in the header too (uniform layout)
        if layout.kind == "topk":
            codes_all.append(vals.to(torch.float32))
            if sent is not None:
                sent[off + sel] = vals
            continue
        q = quantize(vals, scale, levels, plan.bucket_offset + off + sel, key)
        codes_all.append(q)
        if sent is not None:
            sent[off + sel] = q.to(torch.float32) * dequant_step(levels, scale)
    codes = torch.cat(codes_all)
    if layout.kind == "topk":
        _section(out, layout.codes, K, torch.float32).copy_(codes)
    elif layout.bits == 8:
        _section(out, layout.codes, K, torch.int8).copy_(codes.to(torch.int8))
    else:
        p = _pack4(codes)
        out[layout.codes:layout.codes + p.numel()] = p
    if ef21:
        residual.copy_(residual + sent)
    elif residual is not None:
        residual.copy_(g - sent)
    del g_in
    return out


def encode_qsgd(g: torch.Tensor, plan: BucketPlan, layout: Layout, levels: int, norm: str,
                key: int, residual: torch.Tensor = None) -> torch.Tensor:
    """Dense QSGD of every element of the bucket -> uint8 payload (reference Method 4)."""
    if residual is not None:
        g = g + residual
    out = torch.zeros(layout.nbytes, dtype=torch.uint8, device=g.device)
    T = plan.num_tensors
    scales = _section(out, layout.scales, T, torch.float32)
    codes = torch.zeros(plan.total_codes, dtype=torch.int32, device=g.device)
    sent = torch.zeros_like(g) if residual is not None else None
    for t in range(T):
        off, n, d0 = plan.offsets[t], plan.numels[t], plan.tensor_code0[t]
        x = g[off:off + n]
        scale = _scale_of(x, norm)
        scales[t] = scale
        gidx = plan.bucket_offset + off + torch.arange(n, device=g.device)
        q = quantize(x, scale, levels, gidx, key)
        codes[d0:d0 + n] = q
        if sent is not None:
            sent[off:off + n] = q.to(torch.float32) * dequant_step(levels, scale)
    if layout.bits == 8:
        _section(out, layout.codes, plan.total_codes, torch.int8).copy_(codes.to(torch.int8))
    else:
        p = _pack4(codes)
        out[layout.codes:layout.codes + p.numel()] = p
    if residual is not None:
        residual.copy_(g - sent)
    return out


# ---------------------------------------------------------------------------------------------
# scaled sign with error feedback (1-bit SGD / EF-signSGD), one scale per chunk
# ---------------------------------------------------------------------------------------------
_SIGN_THREADS = 256  # the kernel's block: thread t owns elements 4t .. 4t + 3 of each 1024-slab


def _sign_chunk_sums(a: torch.Tensor) -> torch.Tensor:
    """fp32 sums of the rows of ``a`` (fp32 [C, CHUNK], non-negative, padding 0) in the order of
    ``ops/csrc/sign_codec.hip``, every add rounded to fp32:

    * thread t (0..255) adds, from 0, the elements ``u * 1024 + 4 t + j`` for u = 0..7 outer and
      j = 0..3 inner;
    * per wave of 64 threads the shuffle-down tree: ``x[:32] += x[32:]``, ``x[:16] += x[16:32]``,
      ..., ``x[:1] += x[1:2]``;
    * then ``(((0 + w0) + w1) + w2) + w3`` over the four waves."""
    C = a.shape[0]
    x = a.reshape(C, CHUNK // (4 * _SIGN_THREADS), _SIGN_THREADS, 4)
    s = torch.zeros(C, _SIGN_THREADS, dtype=torch.float32, device=a.device)
    for u in range(x.shape[1]):
        for j in range(4):
            s = s + x[:, u, :, j]
    w = s.reshape(C, _SIGN_THREADS // 64, 64)
    d = 32
    while d:
        w = w[:, :, :d] + w[:, :, d:2 * d]
        d >>= 1
    tot = torch.zeros(C, dtype=torch.float32, device=a.device)
    for i in range(w.shape[1]):
        tot = tot + w[:, i, 0]
    return tot


def _sign_gather(plan: BucketPlan, device):
    """(index [C, CHUNK] into the bucket, valid mask, fp32 chunk lengths)."""
    start = torch.tensor(plan.chunk_start, dtype=torch.int64, device=device)
    ln = torch.tensor(plan.chunk_len, dtype=torch.int64, device=device)
    ar = torch.arange(CHUNK, dtype=torch.int64, device=device)
    valid = ar[None, :] < ln[:, None]
    pos = torch.where(valid, start[:, None] + ar[None, :], torch.zeros_like(ar)[None, :])
    return pos, valid, ln.to(torch.float32)


# The rotated form (``--sign-rotate hadamard``; DRIVE / EDEN, Vargaftik et al. 2021 / 2022): every
# chunk row, always over all CHUNK positions (0 past its length), is rotated by y = H(D e) before
# the signs are taken, and the decoded row is rotated back by D(H(.)) * 2^-13.
#
#   * D flips sign bits (an xor of bit 31, so NaN and +/-0 agree with the kernel): word w of chunk
#     row c is ``mix32((c * 256 + w) ^ rot_key)`` and its bit k belongs to element 32 w + k, the
#     addressing of the packed sign words.  ``rot_key = hsign_rot_key(seed, bucket)`` depends on no
#     step and no rank: the rotation is the same on every rank, so it is linear across them.
#   * H is the unnormalised Walsh-Hadamard transform, one butterfly stage per index bit b in the
#     order HSIGN_STAGE_BITS: new[i] = x[i] + x[i | 1 << b], new[i | 1 << b] = x[i] - x[i | 1 << b],
#     every one a separately rounded fp32 operation.  The order is the kernel's (``ops/csrc/
#     sign_codec.hip ew_fwht``): with i = u << 10 | wave << 8 | lane << 2 | j the register-local
#     bits (j: 0, 1; u: 10, 11, 12) come first, then the lane bits 2..7, then the wave bits 8, 9.
#     H H = 2^13 I, so the same stages run in both directions.
HSIGN_STAGE_BITS = (0, 1, 10, 11, 12, 2, 3, 4, 5, 6, 7, 8, 9)
HSIGN_INV = 2.0 ** -13
ROT_TAG = 0x48534731  # "HSG1": the rank slot of stream_key, so no QSGD stream shares the key


def hsign_rot_key(seed: int, bucket: int) -> int:
    """The rotation key of bucket ``bucket``: a host constant, passed to the kernels as a uint32."""
    return rng.stream_key(seed, bucket, ROT_TAG)


def fwht(x: torch.Tensor) -> torch.Tensor:
    """H of the rows of ``x`` (fp32 ``[C, CHUNK]``), stage by stage in HSIGN_STAGE_BITS order."""
    C = x.shape[0]
    for b in HSIGN_STAGE_BITS:
        v = x.reshape(C, CHUNK >> (b + 1), 2, 1 << b)
        lo, hi = v[:, :, 0], v[:, :, 1]
        x = torch.stack((lo + hi, lo - hi), dim=2).reshape(C, CHUNK)
    return x


def hsign_flip(x: torch.Tensor, rot_key: int, row0: int = 0) -> torch.Tensor:
    """D of the rows of ``x`` (fp32 ``[C, CHUNK]``; row r is chunk row ``row0 + r``)."""
    C = x.shape[0]
    w = torch.arange(row0 * (CHUNK // 32), (row0 + C) * (CHUNK // 32), dtype=torch.int64,
                     device=x.device)
    words = rng.mix32(w ^ (rot_key & rng.M32))
    sh = torch.arange(32, dtype=torch.int64, device=x.device)
    flip = ((words[:, None] >> sh) & 1).reshape(C, CHUNK)
    bits = x.contiguous().view(torch.int32).to(torch.int64) ^ (flip << 31)
    bits = ((bits + (1 << 31)) % (1 << 32)) - (1 << 31)
    return bits.to(torch.int32).view(torch.float32)


def hsign_unrotate(a: torch.Tensor, rot_key: int) -> torch.Tensor:
    """``D(H(a)) * 2^-13`` of the rows of ``a``: the inverse of ``H(D .)``."""
    return hsign_flip(fwht(a), rot_key) * torch.tensor(HSIGN_INV, dtype=torch.float32)


def encode_sign(g: torch.Tensor, plan: BucketPlan, layout: Layout,
                residual: torch.Tensor = None, rot_key: int = None) -> torch.Tensor:
    """Scaled sign of one bucket -> uint8 payload (``scales f32[C] | bits u32[256 C]``).

    Per chunk: ``e = g + residual`` (``e = g`` without error feedback), ``scale = sum|e| / len``
    (the fixed-order fp32 sum of :func:`_sign_chunk_sums`, one fp32 divide), ``bit = e < 0``
    (+0, -0 and NaN give 0), decoded value ``d = -scale if bit else scale``, and ``residual = e -
    d``.  Bits past the chunk's length are 0.

    ``rot_key`` (:func:`hsign_rot_key`): the rotated form.  The same quantiser runs on ``y = H(D
    e)`` with length CHUNK for every chunk (``scale = sum|y| / 8192``, all 8192 bits meaningful),
    and ``residual = D(H(y - d)) * 2^-13`` on the chunk's own positions: the residual stays in the
    original domain."""
    if layout.kind != "sign":
        raise ValueError(f"encode_sign given a {layout.kind!r} layout")
    g = g.to(torch.float32)
    e = g + residual if residual is not None else g
    C = plan.num_chunks
    pos, valid, lens = _sign_gather(plan, g.device)
    E = torch.where(valid, e[pos], torch.zeros((), dtype=torch.float32, device=g.device))
    if rot_key is not None:
        E = fwht(hsign_flip(E, rot_key))
        lens = torch.full_like(lens, float(CHUNK))
    scale = _sign_chunk_sums(E.abs()) / lens
    neg = E < 0
    out = torch.zeros(layout.nbytes, dtype=torch.uint8, device=g.device)
    _section(out, layout.scales, C, torch.float32).copy_(scale)
    sh = torch.arange(32, dtype=torch.int64, device=g.device)
    words = (neg.reshape(C, CHUNK // 32, 32).to(torch.int64) << sh).sum(-1)
    words = ((words + (1 << 31)) % (1 << 32)) - (1 << 31)  # uint32 bits as int32
    _section(out, layout.codes, C * (CHUNK // 32), torch.int32).copy_(
        words.to(torch.int32).flatten())
    if residual is not None:
        d = torch.where(neg, -scale[:, None], scale[:, None])
        R = E - d
        if rot_key is not None:
            R = hsign_unrotate(R, rot_key)
        residual[pos[valid]] = R[valid]
    return out


def encode_sign_momentum(g: torch.Tensor, plan: BucketPlan, layout: Layout,
                         residual: torch.Tensor, exp_avg: torch.Tensor, beta1: float,
                         weight_decay: float = 0.0, param: torch.Tensor = None) -> torch.Tensor:
    """1-bit Adam's compressed stage (Tang et al., ICML 2021), sender side: :func:`encode_sign`
    with error feedback of the momentum candidate (every product and sum rounded to fp32
    separately, ``1 - beta1`` formed in fp32, as the kernel does)::

        g' = g + wd * p                     (only when wd != 0)
        u  = m * beta1 + (1 - beta1) * g'
        e  = u + residual

    ``exp_avg`` (m, the same on every rank), ``param`` and ``g`` are only read."""
    if residual is None:
        raise ValueError("the momentum encode always runs with error feedback")
    f32 = np.float32
    g = g.to(torch.float32)
    if weight_decay != 0.0:
        g = g + param * float(f32(weight_decay))
    b1 = f32(beta1)
    u = exp_avg * float(b1) + g * float(f32(1.0) - b1)
    return encode_sign(u, plan, layout, residual)


def onebit_adam_apply(recv: torch.Tensor, plan: BucketPlan, layout: Layout, param: torch.Tensor,
                      exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, inv_n: float,
                      lr_step: float, eps: float) -> None:
    """1-bit Adam's compressed stage, receiver side, on the bucket views ``param`` / ``exp_avg`` /
    ``exp_avg_sq``: ``m = inv_n * sum_r decode(r)`` (rank order, from 0) for every element of
    every tensor, then ``p -= lr_step * (m / (sqrt(v) + eps))`` where the frozen ``v > 0`` -- a
    coordinate that never saw a gradient keeps its parameter.  ``exp_avg_sq`` is only read, and
    positions between tensors are not touched."""
    f32 = np.float32
    m_all = decode_sum(recv, plan, layout, 0, inv_n)
    for off, n in zip(plan.offsets, plan.numels):
        sl = slice(off, off + n)
        m, v, p = m_all[sl], exp_avg_sq[sl], param[sl]
        exp_avg[sl] = m
        # the correctly rounded fp32 square root (the kernel's sqrtf): through fp64, whose 53
        # bits make the second rounding harmless -- torch's vectorised CPU fp32 sqrt is not
        # correctly rounded on every build (1 ulp low on ~0.5 % of inputs with AVX-512)
        root = v.to(torch.float64).sqrt().to(torch.float32)
        step = (m / (root + float(f32(eps)))) * float(f32(lr_step))
        param[sl] = torch.where(v > 0, p - step, p)


def onebit_lamb_apply(recv: torch.Tensor, plan: BucketPlan, layout: Layout, param: torch.Tensor,
                      exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                      exp_avg_sq_fresh: torch.Tensor, tensors, r_frozen: torch.Tensor,
                      last_factor: torch.Tensor, inv_n: float, lr: float, b1: float, b2: float,
                      eps: float, wd: float, step: int, freeze_step: int, factor_min: float = 0.5,
                      factor_max: float = 4.0, factor_threshold: float = 0.1, bc1: float = None):
    """1-bit LAMB's compressed stage (Li et al., 2021), receiver side, on the bucket views
    ``param`` / ``exp_avg`` / ``exp_avg_sq`` (frozen, only read) / ``exp_avg_sq_fresh``; ``tensors``
    are the bucket's ``(offset, numel, adapts)`` rows, ``r_frozen`` / ``last_factor`` (only read)
    their fp32 entries.  Every operation is rounded to fp32 on its own; ``1 - b1`` and ``1 - b2``
    are formed in fp32 (as the momentum encode forms its ``1 - beta1``), ``bc1 = 1 - b1^step``
    and ``1 - b2^freeze_step`` in double, then rounded (``bc1``: the caller's value instead)::

        m     = inv_n * sum_r decode(r)                      (rank order, from 0)
        g     = (m - m_old * b1) / (1 - b1)
        vf    = vf * b2 + (1 - b2) * (g * g)                 exp_avg = m, exp_avg_sq_fresh = vf
        q     = (sqrt(v) + eps) / (sqrt(vf) + eps)           where the frozen v > 0
        f_raw = max(0, max q)                                a NaN q does not enter
        u     = (m / bc1) / (sqrt(v / bc2(freeze_step)) + eps) [+ wd * p]
        p    -= (lr * r) * u                                 where v > 0

    with ``r = 1`` for a tensor that does not adapt, ``r = r_frozen`` when ``f_raw == 0`` (both keep
    their ``last_factor``), and otherwise ``f = clamp(clamp(f_raw, factor_min, factor_max),
    last_factor * (1 - factor_threshold), last_factor * (1 + factor_threshold))``, ``r = r_frozen
    * f``.  Positions between tensors are not touched.  Returns ``(ratios, factors)``: the
    tensors' ``r`` and their new ``last_factor``."""
    f32 = np.float32
    if step <= freeze_step or freeze_step < 1:
        raise ValueError("the compressed stage starts after freeze_step >= 1")
    m_all = decode_sum(recv, plan, layout, 0, inv_n)
    b1f, b2f, epsf, wdf = f32(b1), f32(b2), f32(eps), f32(wd)
    omb1, omb2 = f32(1.0) - b1f, f32(1.0) - b2f
    bc1 = f32(1.0 - b1 ** step) if bc1 is None else f32(bc1)
    bc2w = f32(1.0 - b2 ** freeze_step)
    fmin, fmax = f32(factor_min), f32(factor_max)
    lo_k, hi_k = f32(1.0) - f32(factor_threshold), f32(1.0) + f32(factor_threshold)

    def root(x):  # the correctly rounded fp32 square root: see onebit_adam_apply
        return x.to(torch.float64).sqrt().to(torch.float32)

    def over(x, c):  # x / c as an elementwise IEEE divide (never a product with 1 / c)
        return x / torch.full_like(x, float(c))

    ratios = torch.ones(len(tensors), dtype=torch.float32, device=param.device)
    factors = last_factor.clone()
    for t, (off, n, adapts) in enumerate(tensors):
        sl = slice(off, off + n)
        m, v, p = m_all[sl], exp_avg_sq[sl], param[sl]
        g = over(m - exp_avg[sl] * float(b1f), omb1)
        vf = exp_avg_sq_fresh[sl] * float(b2f) + (g * g) * float(omb2)
        exp_avg[sl] = m
        exp_avg_sq_fresh[sl] = vf
        live = v > 0
        q = (root(v) + float(epsf)) / (root(vf) + float(epsf))
        q = q[live & ~torch.isnan(q)]
        f_raw = f32(max(0.0, float(q.max()))) if q.numel() else f32(0.0)
        r = f32(1.0)
        if adapts:
            r = f32(r_frozen[t])
            if f_raw != 0:
                lf = f32(last_factor[t])
                f = min(max(f_raw, fmin), fmax)
                f = min(max(f, lf * lo_k), lf * hi_k)
                r = r * f
                factors[t] = float(f)
        ratios[t] = float(r)
        u = over(m, bc1) / (root(over(v, bc2w)) + float(epsf))
        if wd != 0:
            u = u + p * float(wdf)
        param[sl] = torch.where(live, p - u * float(f32(lr) * r), p)
    return ratios, factors


def sign_reduce_encode(recv: torch.Tensor, plan: BucketPlan, layout: Layout, inv_n: float,
                       server_resid: torch.Tensor) -> torch.Tensor:
    """The two-stage sign all-reduce's owner step (``parallel/twostage.py``) for one shard:
    ``recv`` (uint8 ``[N, >= layout.nbytes]``) holds the N workers' payloads of the shard; their
    rank-ordered sum from 0 times ``inv_n`` is sign-compressed again with the *server* residual
    (updated in place).  By definition ``encode_sign(decode_sum(recv, plan, layout, 0, inv_n),
    plan, layout, server_resid)``: no numerics of its own."""
    mean = decode_sum(recv[:, :layout.nbytes], plan, layout, 0, inv_n)
    return encode_sign(mean, plan, layout, server_resid)


def onebit_lr_step(lr: float, beta1: float, beta2: float, step: int, freeze_step: int) -> float:
    """``lr * sqrt(1 - beta2^freeze_step) / (1 - beta1^step)``: the variance's bias correction
    stays at its value of the freeze step, the momentum's follows the 1-based ``step``.  In
    double precision with the betas rounded to fp32 first, as the kernel holds them (at a small
    ``freeze_step`` 1 - beta2^freeze_step magnifies beta2's rounding a thousandfold), so the
    host value and the one the kernel derives from the device step counter agree to fp32."""
    import math

    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    return lr * math.sqrt(1 - b2 ** freeze_step) / (1 - b1 ** step)


def _sign_rows(pay: torch.Tensor, plan: BucketPlan, layout: Layout) -> torch.Tensor:
    """``+/- scale`` of every position of every chunk row of one payload: fp32 ``[C, CHUNK]``."""
    C = plan.num_chunks
    scale = _section(pay, layout.scales, C, torch.float32)
    words = _section(pay, layout.codes, C * (CHUNK // 32), torch.int32).to(torch.int64)
    sh = torch.arange(32, dtype=torch.int64, device=pay.device)
    neg = ((words[:, None] >> sh) & 1).reshape(C, CHUNK).bool()
    return torch.where(neg, -scale[:, None], scale[:, None])


def _sign_scatter(d: torch.Tensor, plan: BucketPlan) -> torch.Tensor:
    pos, valid, _ = _sign_gather(plan, d.device)
    out = torch.zeros(plan.length, dtype=torch.float32, device=d.device)
    out[pos[valid]] = d[valid]
    return out


def _sign_decoded(pay: torch.Tensor, plan: BucketPlan, layout: Layout) -> torch.Tensor:
    return _sign_scatter(_sign_rows(pay, plan, layout), plan)


def _hsign_decoded_sum(recv: torch.Tensor, plan: BucketPlan, layout: Layout,
                       rot_key: int) -> torch.Tensor:
    """The rotated codec's receive side: the rank-ordered sum from 0 of ``+/- scale_r`` over all
    CHUNK positions of every row (the rotation is shared, so the sum commutes with it), one
    inverse transform ``D(H(.)) * 2^-13``, and the chunk's own positions of the result."""
    a = torch.zeros(plan.num_chunks, CHUNK, dtype=torch.float32, device=recv.device)
    for r in range(recv.shape[0]):
        a = a + _sign_rows(recv[r], plan, layout)
    return _sign_scatter(hsign_unrotate(a, rot_key), plan)


# ---------------------------------------------------------------------------------------------
# block floating point: OCP Microscaling (MX) v1.0, 32 elements per power-of-two E8M0 scale
# ---------------------------------------------------------------------------------------------
# bits -> (exponent bits, mantissa bits, exponent bias, largest finite value, emax)
MX_FORMATS = {8: (4, 3, 7, 448.0, 8), 4: (2, 1, 1, 6.0, 2)}
MX_NAMES = {"fp8": 8, "fp4": 4}  # FP8 E4M3 | FP4 E2M1


def _pow2(k: torch.Tensor) -> torch.Tensor:
    """fp64 ``2^k`` of an int64 tensor, built from the exponent field (|k| <= 1022)."""
    return ((k + 1023) << 52).view(torch.float64)


def mx_scale_bytes(e: torch.Tensor, bits: int) -> torch.Tensor:
    """The E8M0 scale byte (int64) of every row of ``e`` (fp32 ``[B, 32]``): with ``em`` the
    exponent field of the largest ``bits(e) & 0x7fffffff`` of the block (an unsigned integer
    maximum, so a NaN is not dropped), ``s = clamp(em - emax, 0, 254)``, and ``0xFF`` where ``em
    == 255`` (the block holds an inf or a NaN)."""
    emax = MX_FORMATS[bits][4]
    mag = e.contiguous().view(torch.int32).to(torch.int64) & 0x7FFFFFFF
    em = mag.max(dim=1).values >> 23
    return torch.where(em == 255, torch.full_like(em, 255), (em - emax).clamp(0, 254))


def mx_quantize(e: torch.Tensor, s: torch.Tensor, bits: int) -> torch.Tensor:
    """Element codes (uint8 ``[B, 32]``) of the blocks ``e`` (fp32 ``[B, 32]``) under the scale
    bytes ``s`` (:func:`mx_scale_bytes`): ``q = e / 2^(s - 127)`` exactly (fp64), rounded to
    nearest even on the format's grid and saturated to its largest finite value (448, code 0x7E,
    for E4M3; 6, code 0x7, for E2M1).  The code's sign bit is ``e``'s sign bit, so a negative
    value that rounds to zero and -0.0 itself give the code of -0.  A block with ``s == 0xFF``
    gets codes 0."""
    _, mb, bias, top, _ = MX_FORMATS[bits]
    dead = (s == 255)[:, None]
    a = e.abs().to(torch.float64) * _pow2(127 - s.clamp(max=254))[:, None]
    a = torch.where(dead, torch.zeros_like(a), a).clamp(max=top)
    ex = ((a.view(torch.int64) >> 52) & 0x7FF) - 1023  # floor(log2 a); -1023 for 0
    ex = ex.clamp(min=1 - bias)  # below the smallest normal the grid keeps its spacing
    n = torch.round(a * _pow2(mb - ex)).to(torch.int64)  # half to even; 0 .. 2^(mb + 1)
    # n < 2^mb: a subnormal code; n == 2^(mb + 1) carries into the exponent field
    mag = ((ex + bias - 1) << mb) + n
    neg = (e.contiguous().view(torch.int32).to(torch.int64) >> 31) & 1
    code = torch.where(dead, torch.zeros_like(mag), mag | (neg << (bits - 1)))
    return code.to(torch.uint8)


def mx_dequantize(codes: torch.Tensor, s: torch.Tensor, bits: int) -> torch.Tensor:
    """fp32 ``value(code) * 2^(s - 127)`` of every element of the blocks ``codes`` (uint8 ``[B,
    32]``): exact in fp32 for every code the encode writes (at most 4 significant bits, no smaller
    than 2^-136).  A block with ``s == 0xFF`` is NaN (0x7FC00000) on all 32 positions, and so are
    E4M3's own NaN codes 0x7F / 0xFF, which no encode writes."""
    _, mb, bias, _, _ = MX_FORMATS[bits]
    c = codes.to(torch.int64)
    mag = c & ((1 << (bits - 1)) - 1)
    ef, m = mag >> mb, mag & ((1 << mb) - 1)
    val = torch.where(ef == 0, m.to(torch.float64) * 2.0 ** (1 - bias - mb),
                      ((1 << mb) + m).to(torch.float64) * _pow2(ef - bias - mb))
    d = (val * _pow2(s.clamp(max=254) - 127)[:, None]).to(torch.float32)
    d = torch.where((c >> (bits - 1)) == 1, -d, d)
    nan = (s == 255)[:, None]
    if bits == 8:
        nan = nan | (mag == 0x7F)
    return torch.where(nan, torch.full_like(d, float("nan")), d)


def _mx_mask(plan: BucketPlan, device) -> torch.Tensor:
    """True on the positions of the padded bucket that belong to a tensor."""
    own = torch.zeros(plan.length, dtype=torch.bool, device=device)
    for off, n in zip(plan.offsets, plan.numels):
        own[off:off + n] = True
    return own


def encode_mx(g: torch.Tensor, plan: BucketPlan, layout: Layout,
              residual: torch.Tensor = None) -> torch.Tensor:
    """MXFP8 / MXFP4 of one bucket -> uint8 payload (``scales u8[L / 32] | codes``; ``L =
    plan.length``, ``layout.bits`` 8: one E4M3 byte per position, 4: E2M1 nibbles, the low nibble
    the even position).

    ``e = g + residual`` (``e = g`` without error feedback) on the tensors' positions and 0 on the
    pads between them; every 32 consecutive positions of the bucket are one block
    (:func:`mx_scale_bytes`, :func:`mx_quantize`); ``residual = e - d`` with ``d`` the decoded
    value (:func:`mx_dequantize`), one fp32 subtract, NaN on every position of a block that held
    an inf or a NaN.  Pads encode as scale 0 and code 0, so every byte of the payload is written.

    Where the OCP text is silent the gfx950 conversion instructions were measured to agree with
    the choices made here (``profiles/validation/mx.md``): the sign of a zero code is the input's
    and the low nibble of an FP4 byte is the even element; a non-finite block decodes to the quiet
    NaN 0x7FC00000, which the kernels form themselves.  Saturation is this function's, not the
    E4M3 instruction's: that one answers its NaN code above 464 and the kernel clamps first."""
    if layout.kind != "mx":
        raise ValueError(f"encode_mx given a {layout.kind!r} layout")
    bits, L = layout.bits, plan.length
    g = g.to(torch.float32)[:L]
    e = g + residual[:L] if residual is not None else g
    own = _mx_mask(plan, g.device)
    E = torch.where(own, e, torch.zeros((), dtype=torch.float32, device=g.device)).reshape(-1, 32)
    s = mx_scale_bytes(E, bits)
    codes = mx_quantize(E, s, bits)
    out = torch.zeros(layout.nbytes, dtype=torch.uint8, device=g.device)
    out[layout.scales:layout.scales + L // 32] = s.to(torch.uint8)
    flat = codes.flatten()
    if bits == 4:
        flat = flat[0::2] | (flat[1::2] << 4)
    out[layout.codes:layout.codes + flat.numel()] = flat
    if residual is not None:
        R = (E - mx_dequantize(codes, s, bits)).flatten()
        residual[:L][own] = R[own]
    return out


def _mx_decoded(pay: torch.Tensor, plan: BucketPlan, layout: Layout) -> torch.Tensor:
    """One payload decoded on the tensors' positions (0 on the pads): fp32 ``[plan.length]``."""
    bits, L = layout.bits, plan.length
    s = pay[layout.scales:layout.scales + L // 32].to(torch.int64)
    c = pay[layout.codes:layout.codes + L * bits // 8]
    if bits == 4:
        c = torch.stack([c & 0xF, c >> 4], 1).flatten()
    d = mx_dequantize(c.reshape(-1, 32), s, bits).flatten()
    return torch.where(_mx_mask(plan, pay.device), d, torch.zeros_like(d))


# ---------------------------------------------------------------------------------------------
# TernGrad (Wen et al., NeurIPS 2017): ternary codes, one clipped fp32 scaler per tensor
# ---------------------------------------------------------------------------------------------
TERN_CLIP = 2.5  # the paper's clipping constant c: |g| is capped at c * sigma per layer


def _tern_sumsq(x: torch.Tensor) -> float:
    """The fp32 sum of ``x * x`` over one tensor in the order of ``ops/csrc/tern_codec.hip``,
    every product and every add rounded to fp32:

    * per 8192-chunk the order of :func:`_sign_chunk_sums` (``k_tern_stats``; positions past the
      tensor's end add +0);
    * across the tensor's chunks (``k_tern_scale``, one block per tensor) thread t (0..255) adds,
      from 0, the chunk partials ``t, t + 256, t + 512, ...``; then the same wave shuffle tree
      over the 256 threads and ``(((0 + w0) + w1) + w2) + w3`` over the four waves.  A tensor of
      up to 256 chunks therefore adds its partials by the tree alone."""
    n = x.numel()
    nch = (n + CHUNK - 1) // CHUNK
    rows = torch.zeros(nch * CHUNK, dtype=torch.float32, device=x.device)
    rows[:n] = x * x
    part = _sign_chunk_sums(rows.reshape(nch, CHUNK))
    u = (nch + _SIGN_THREADS - 1) // _SIGN_THREADS
    p = torch.zeros(u * _SIGN_THREADS, dtype=torch.float32, device=x.device)
    p[:nch] = part
    p = p.reshape(u, _SIGN_THREADS)
    s = torch.zeros(_SIGN_THREADS, dtype=torch.float32, device=x.device)
    for k in range(u):
        s = s + p[k]
    w = s.reshape(_SIGN_THREADS // 64, 64)
    d = 32
    while d:
        w = w[:, :d] + w[:, d:2 * d]
        d >>= 1
    tot = torch.zeros((), dtype=torch.float32, device=x.device)
    for i in range(w.shape[0]):
        tot = tot + w[i, 0]
    return float(tot)


def tern_scale(x: torch.Tensor, clip: float) -> float:
    """The clipped scaler of one tensor: ``min(max|x|, clip * rms)`` with ``rms = sqrtf(sumsq /
    n)`` -- :func:`_tern_sumsq`, one fp32 divide, one correctly rounded fp32 square root, one fp32
    product, ``fminf``; ``clip == 0``: ``max|x|``."""
    f32 = np.float32
    n = x.numel()
    if n == 0:
        return 0.0
    absmax = f32(float(x.abs().max()))
    if not clip > 0:
        return float(absmax)
    rms = np.sqrt(f32(_tern_sumsq(x)) / f32(n))
    return float(np.fmin(absmax, f32(clip) * rms))


def _pack2(codes: torch.Tensor) -> torch.Tensor:
    """int32 codes in {-1, 0, 1} (a multiple of 16 of them) -> uint32 words as int32: element i is
    bits ``2 (i & 15) .. + 1`` of word ``i >> 4``, 2-bit two's complement (0, 1, 3 = -1)."""
    sh = 2 * torch.arange(16, dtype=torch.int64, device=codes.device)
    words = ((codes.to(torch.int64) & 3).reshape(-1, 16) << sh).sum(-1)
    words = ((words + (1 << 31)) % (1 << 32)) - (1 << 31)
    return words.to(torch.int32)


def _unpack2(words: torch.Tensor) -> torch.Tensor:
    sh = 2 * torch.arange(16, dtype=torch.int64, device=words.device)
    c = ((words.to(torch.int64)[:, None] >> sh) & 3).flatten()
    return ((c ^ 2) - 2).to(torch.int32)


def encode_tern(g: torch.Tensor, plan: BucketPlan, layout: Layout, clip: float, key: int,
                residual: torch.Tensor = None) -> torch.Tensor:
    """TernGrad of one bucket -> uint8 payload (``scales f32[T] | codes u32[D' / 16]``, 2 bits per
    element; ``D' = plan.total_codes``, pad codes 0).

    Per tensor, with ``x = g`` (``g + residual`` under error feedback): ``scale`` =
    :func:`tern_scale` ``(x, clip)``, the codes are ``quantize(x, scale, 1, gidx, key)`` -- QSGD's
    stochastic rule at one level on QSGD's streams (``gidx = bucket_offset + off + i``): ``|x| /
    scale`` is the probability of a non-zero code, capped at 1, so an element above the clipped
    scaler codes ``sign(x)`` -- and the decoded value is ``code * dequant_step(1, scale)``.  A zero
    scale gives zero codes.  ``residual = x - decoded`` with the unclipped ``x``: what clipping
    removes is fed back.  Without clipping (``clip == 0``) the codec is unbiased and equals
    ``encode_qsgd(levels=1, norm="max")`` code for code.

    Two deliberate deviations from the paper.  ``rms`` is the second moment about zero, not the
    standard deviation about the mean: the paper models a layer's gradient as a zero-mean
    Gaussian, and the centred form would give sigma = 0 (a zeroed tensor, every step) for a
    one-element or constant tensor and cancels catastrophically in fp32.  And every rank sends
    its own scaler, which the all-gather decode applies to that rank's codes: the paper's scaler
    sharing (for summing ternaries on a parameter server) is not implemented.

    Inputs are taken to be finite; a non-finite gradient behaves as in the QSGD codec (the
    integer maximum keeps a NaN or an inf as the scale and the decoded values are not finite)."""
    if layout.kind != "tern":
        raise ValueError(f"encode_tern given a {layout.kind!r} layout")
    g = g.to(torch.float32)
    if residual is not None:
        g = g + residual
    out = torch.zeros(layout.nbytes, dtype=torch.uint8, device=g.device)
    T = plan.num_tensors
    scales = _section(out, layout.scales, T, torch.float32)
    codes = torch.zeros(plan.total_codes, dtype=torch.int32, device=g.device)
    sent = torch.zeros_like(g) if residual is not None else None
    for t in range(T):
        off, n, d0 = plan.offsets[t], plan.numels[t], plan.tensor_code0[t]
        x = g[off:off + n]
        scale = tern_scale(x, clip)
        scales[t] = scale
        gidx = plan.bucket_offset + off + torch.arange(n, device=g.device)
        q = quantize(x, scale, 1, gidx, key)
        codes[d0:d0 + n] = q
        if sent is not None:
            sent[off:off + n] = q.to(torch.float32) * dequant_step(1, scale)
    _section(out, layout.codes, plan.total_codes // 16, torch.int32).copy_(_pack2(codes))
    if residual is not None:
        residual.copy_(g - sent)
    return out


def _tern_decoded(pay: torch.Tensor, plan: BucketPlan, layout: Layout) -> torch.Tensor:
    """One payload decoded on the tensors' positions (0 between them): fp32 ``[plan.length]``."""
    T = plan.num_tensors
    scales = _section(pay, layout.scales, T, torch.float32)
    codes = _unpack2(_section(pay, layout.codes, plan.total_codes // 16, torch.int32)).to(
        torch.float32)
    out = torch.zeros(plan.length, dtype=torch.float32, device=pay.device)
    for t in range(T):
        off, n, d0 = plan.offsets[t], plan.numels[t], plan.tensor_code0[t]
        out[off:off + n] = codes[d0:d0 + n] * dequant_step(1, float(scales[t]))
    return out


# ---------------------------------------------------------------------------------------------
# Threshold-search sparsifier (RedSync, Fang et al. 2019; MSTopK, Shi et al. 2021; hard-threshold
# sparsification, Sahu et al. 2021): per chunk, everything above a bf16-level threshold
# ---------------------------------------------------------------------------------------------
THRESH_LEVELS = 32768  # levels 0 .. 32767; the threshold J lies in [0, THRESH_LEVELS]


def thresh_level(x: torch.Tensor) -> torch.Tensor:
    """int32 level of every fp32 element: the bf16 truncation of ``|x|``, ``(bits & 0x7fffffff)
    >> 16``, 15 bits and monotone in ``|x|`` (an inf is 0x7f80, a NaN lies above it)."""
    return (x.contiguous().view(torch.int32) & 0x7FFFFFFF) >> 16


def thresh_threshold(lev: torch.Tensor, cap: int) -> int:
    """The smallest J in [0, 32768] with ``#{lev >= J} <= cap``: 0 when everything fits, else one
    above the (cap + 1)-th largest level (all ties at that level are left out)."""
    n = lev.numel()
    if n <= cap:
        return 0
    return int(torch.sort(lev, descending=True).values[cap]) + 1


def encode_thresh(g: torch.Tensor, plan: BucketPlan, layout: Layout,
                  residual: torch.Tensor = None) -> torch.Tensor:
    """Threshold sparsification of one bucket -> uint8 payload (``counts u16[C] | idx u16[S] |
    values f32[S]``, ``plan.thresh_slots``).

    ``acc = g`` (``g + residual`` under error feedback).  Per chunk row c with capacity ``cap_c``:
    ``J_c`` = :func:`thresh_threshold` of the chunk's :func:`thresh_level`; the elements with ``lev
    >= J_c`` are sent in increasing chunk-local index with their exact fp32 ``acc``, at most
    ``cap_c`` of them by the choice of ``J_c`` (ties at the boundary level are all left out, so an
    all-equal chunk longer than its capacity sends nothing); unused slots hold index 0 and +0.0.
    ``residual`` = 0 where sent, ``acc`` elsewhere.  Nothing is special-cased: a NaN or an inf has
    a high level and is sent."""
    if layout.kind != "thresh":
        raise ValueError(f"encode_thresh given a {layout.kind!r} layout")
    acc = g.to(torch.float32)
    if residual is not None:
        acc = acc + residual
    cap, slot0, S = plan.thresh_slots()
    C = plan.num_chunks
    out = torch.zeros(layout.nbytes, dtype=torch.uint8, device=acc.device)
    counts = _section(out, layout.counts, C, torch.int16)
    idx = _section(out, layout.idx, S, torch.int16)
    vals = _section(out, layout.codes, S, torch.float32)
    for c in range(C):
        s0, n = plan.chunk_start[c], plan.chunk_len[c]
        x = acc[s0:s0 + n]
        lev = thresh_level(x)
        sel = (lev >= thresh_threshold(lev, cap[c])).nonzero().flatten()
        m = sel.numel()
        counts[c] = m if m < 32768 else m - 65536
        idx[slot0[c]:slot0[c] + m] = sel.to(torch.int16)
        vals[slot0[c]:slot0[c] + m] = x[sel]
        if residual is not None:  # the chunk's own positions only, as the kernel writes them
            left = x.clone()
            left[sel] = 0.0
            residual[s0:s0 + n] = left
    return out


def _thresh_entries(pay: torch.Tensor, plan: BucketPlan, layout: Layout):
    """(bucket positions, values) of one ``thresh`` payload.  A count is clamped to the chunk's
    capacity and an index at or past the chunk's length is ignored, as the decode kernel does: a
    corrupt row never reaches outside its chunk."""
    cap, slot0, S = plan.thresh_slots()
    C = plan.num_chunks
    counts = _section(pay, layout.counts, C, torch.int16).to(torch.int64) & 0xFFFF
    idx = _section(pay, layout.idx, S, torch.int16).to(torch.int64) & 0xFFFF
    vals = _section(pay, layout.codes, S, torch.float32)
    pos, out = [], []
    for c in range(C):
        m = min(int(counts[c]), cap[c])
        i = idx[slot0[c]:slot0[c] + m]
        ok = i < plan.chunk_len[c]
        pos.append(plan.chunk_start[c] + i[ok])
        out.append(vals[slot0[c]:slot0[c] + m][ok])
    return torch.cat(pos), torch.cat(out)


# ---------------------------------------------------------------------------------------------
# decode: sum over ranks (in rank order) of the dequantised payloads, times ``scale``
# ---------------------------------------------------------------------------------------------
def _decoded_entries(pay: torch.Tensor, plan: BucketPlan, layout: Layout, levels: int):
    T, C, K = plan.num_tensors, plan.num_chunks, plan.total_k
    scales = _section(pay, layout.scales, T, torch.float32)
    counts = _section(pay, layout.counts, C, torch.int16).to(torch.int64)
    idx = _section(pay, layout.idx, plan.total_idx, torch.int16).to(torch.int64) & 0xFFFF
    bm = _section(pay, layout.bitmap, plan.total_bm_words, torch.int32).to(torch.int64) \
        & 0xFFFFFFFF
    if layout.kind == "topk":
        vals = _section(pay, layout.codes, K, torch.float32)
    elif layout.bits == 8:
        vals = _section(pay, layout.codes, K, torch.int8).to(torch.float32)
    else:
        vals = _unpack4(pay[layout.codes:layout.codes + (K + 1) // 2], K).to(torch.float32)
    pos = torch.zeros(K, dtype=torch.int64, device=pay.device)
    bits = torch.arange(32, device=pay.device)
    for t in range(T):
        off, n, k, e0 = plan.offsets[t], plan.numels[t], plan.ks[t], plan.tensor_entry0[t]
        if plan.tensor_bm0[t] >= 0:  # entries in element order: the set bits, ascending
            w0 = plan.tensor_bm0[t]
            w = bm[w0:w0 + (n + 31) // 32]
            el = (((w[:, None] >> bits) & 1).flatten()).nonzero().flatten()[:k]
            pos[e0:e0 + el.numel()] = off + el
        else:  # chunk of every entry from the per-chunk counts, then the chunk-local index
            c0, nch, i0 = plan.tensor_chunk0[t], plan.tensor_nchunks[t], plan.tensor_idx0[t]
            ch = torch.repeat_interleave(torch.arange(nch, device=pay.device),
                                         counts[c0:c0 + nch])[:k]
            pos[e0:e0 + ch.numel()] = off + ch * CHUNK + idx[i0:i0 + ch.numel()]
    if layout.kind != "topk":
        tensor_of_entry = torch.repeat_interleave(
            torch.arange(T, device=pay.device),
            torch.tensor(plan.ks, dtype=torch.int64, device=pay.device))
        step = scales * float(np.float32(1.0 / levels))
        vals = vals * step[tensor_of_entry]
    return pos, vals


def decode_sum(recv: torch.Tensor, plan: BucketPlan, layout: Layout, levels: int,
               scale: float, rot_key: int = None) -> torch.Tensor:
    """``recv``: uint8 [N, nbytes].  Returns fp32 [plan.length] = scale * sum_r decode(r).
    ``rot_key``: the rotated sign codec (``scale`` multiplies the inverse transform's output)."""
    if rot_key is not None:
        if layout.kind != "sign":
            raise ValueError(f"only the sign codec is rotated, not {layout.kind!r}")
        return (_hsign_decoded_sum(recv, plan, layout, rot_key)
                * torch.tensor(scale, dtype=torch.float32))
    acc = torch.zeros(plan.length, dtype=torch.float32, device=recv.device)
    for r in range(recv.shape[0]):
        if layout.kind in ("topk", "topk_qsgd"):
            pos, vals = _decoded_entries(recv[r], plan, layout, levels)
            acc.index_add_(0, pos, vals)
        elif layout.kind == "sign":
            acc += _sign_decoded(recv[r], plan, layout)
        elif layout.kind == "mx":
            acc += _mx_decoded(recv[r], plan, layout)
        elif layout.kind == "tern":
            acc += _tern_decoded(recv[r], plan, layout)
        elif layout.kind == "thresh":  # an index appears once per row: the order is the ranks'
            pos, vals = _thresh_entries(recv[r], plan, layout)
            acc.index_add_(0, pos, vals)
        else:
            acc += _dense_decoded(recv[r], plan, layout, levels)
    return acc * torch.tensor(scale, dtype=torch.float32)


def _dense_decoded(pay, plan, layout, levels):
    T = plan.num_tensors
    scales = _section(pay, layout.scales, T, torch.float32)
    if layout.bits == 8:
        codes = _section(pay, layout.codes, plan.total_codes, torch.int8).to(torch.float32)
    else:
        codes = _unpack4(pay[layout.codes:layout.codes + plan.total_codes // 2],
                         plan.total_codes).to(torch.float32)
    out = torch.zeros(plan.length, dtype=torch.float32, device=pay.device)
    for t in range(T):
        off, n, d0 = plan.offsets[t], plan.numels[t], plan.tensor_code0[t]
        out[off:off + n] = codes[d0:d0 + n] * dequant_step(levels, float(scales[t]))
    return out


# ---------------------------------------------------------------------------------------------
# optimizers with explicit gradients (reference ``optim/sgd.py:59-91``, ``optim/adam.py:38-94``)
# ---------------------------------------------------------------------------------------------
def sgd_apply(p, buf, g, lr, momentum, dampening, weight_decay, nesterov, first):
    d_p = g
    if weight_decay != 0:
        d_p = d_p + weight_decay * p
    if momentum != 0:
        if first:
            buf.copy_(d_p)
        else:
            buf.mul_(momentum).add_(d_p, alpha=1 - dampening)
        d_p = d_p + momentum * buf if nesterov else buf
    p.add_(d_p, alpha=-lr)


def adam_apply(p, m, v, vmax, g, lr, beta1, beta2, eps, weight_decay, step, amsgrad):
    """Adam / AMSGrad in the reference form (``denom = sqrt(v) + eps``).  The betas are rounded to
    the state's dtype first and ``1 - beta`` is formed in it, as ``ew_adam`` does in fp32:
    ``1 - fp32(0.999)`` and ``fp32(1 - 0.999)`` differ by 1.3e-5 relative, and so would
    ``exp_avg_sq`` between the CPU and the kernel.  The bias correction uses the same rounded
    betas (the kernel's device-step path), so the decay and its correction stay consistent."""
    import math
    one = torch.ones((), dtype=p.dtype)
    b1, b2 = torch.tensor(beta1, dtype=p.dtype), torch.tensor(beta2, dtype=p.dtype)
    c1, c2 = float(one - b1), float(one - b2)
    beta1, beta2 = float(b1), float(b2)
    if weight_decay != 0:
        g = g + weight_decay * p
    m.mul_(beta1).add_(g, alpha=c1)
    v.mul_(beta2).addcmul_(g, g, value=c2)
    if amsgrad:
        torch.maximum(vmax, v, out=vmax)
        denom = vmax.sqrt().add_(eps)
    else:
        denom = v.sqrt().add_(eps)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    p.addcdiv_(m, denom, value=-lr * math.sqrt(bc2) / bc1)


# ---------------------------------------------------------------------------------------------
# Lion (Chen et al. 2023) and Distributed Lion's 1-bit vote (Liu et al. 2024).  The definition of
# ``ops/csrc/lion.hip``: fp32 throughout, every product and sum rounded on its own, the betas, the
# weight decay and the lr rounded to fp32 first and ``1 - beta`` formed in fp32.  With beta1 =
# beta2 = 0 the vote is signSGD with majority vote (Bernstein et al. 2018), with beta1 = beta2
# Signum.
# ---------------------------------------------------------------------------------------------
def _lion_betas(beta1: float, beta2: float):
    f32 = np.float32
    b1, b2 = f32(beta1), f32(beta2)
    return float(b1), float(f32(1.0) - b1), float(b2), float(f32(1.0) - b2)


def _lion_step(p: torch.Tensor, d: torch.Tensor, lr: float, weight_decay: float) -> torch.Tensor:
    """``p - lr * (d + wd * p)`` (``wd == 0``: ``p - lr * d``, no product with p)."""
    wd = float(np.float32(weight_decay))
    if wd != 0.0:
        d = d + p * wd
    return p - d * float(np.float32(lr))


def lion_apply(p, m, g, lr, beta1, beta2, weight_decay):
    """Dense Lion on the flat views ``p`` / ``m`` with the already scaled gradient ``g``::

        c = m * b1 + (1 - b1) * g
        u = sign(c)                       (-1, 0, +1; 0 and NaN give 0)
        p = p - lr * (u + wd * p)
        m = m * b2 + (1 - b2) * g"""
    b1, c1, b2, c2 = _lion_betas(beta1, beta2)
    g = g.to(torch.float32)
    c = m * b1 + g * c1
    u = (c > 0).to(torch.float32) - (c < 0).to(torch.float32)
    p.copy_(_lion_step(p, u, lr, weight_decay))
    m.copy_(m * b2 + g * c2)


def encode_vote(g: torch.Tensor, plan: BucketPlan, layout: Layout, exp_avg: torch.Tensor,
                beta1: float, beta2: float, step: int, rank: int) -> torch.Tensor:
    """This rank's vote of one bucket -> uint8 payload (``bits u32[256 C]``); ``exp_avg`` (the
    rank's own momentum, the bucket's view) is updated in place.  ``g`` is the raw local gradient.

    ``c = m * b1 + (1 - b1) * g``; the bit of chunk-local element i is ``(c < 0) | ((c == 0) & ((i
    + step + rank) & 1))`` with the 1-based ``step``: set = -1, clear = +1, NaN gives 0, and an
    exact zero (+0 or -0), which one bit cannot say, votes by that parity so that its votes cancel
    over two steps and across an even world.  Bits past a chunk's length are 0.  Then ``m = m * b2
    + (1 - b2) * g`` at every element of every tensor."""
    if layout.kind != "vote":
        raise ValueError(f"encode_vote given a {layout.kind!r} layout")
    b1, c1, b2, c2 = _lion_betas(beta1, beta2)
    g = g.to(torch.float32)[:plan.length]
    m = exp_avg[:plan.length]
    C = plan.num_chunks
    pos, valid, _ = _sign_gather(plan, g.device)
    c = (m * b1 + g * c1)[pos]
    odd = ((torch.arange(CHUNK, dtype=torch.int64, device=g.device) + int(step) + int(rank)) & 1
           ).bool()
    neg = ((c < 0) | ((c == 0) & odd[None, :])) & valid
    out = torch.zeros(layout.nbytes, dtype=torch.uint8, device=g.device)
    sh = torch.arange(32, dtype=torch.int64, device=g.device)
    words = (neg.reshape(C, CHUNK // 32, 32).to(torch.int64) << sh).sum(-1)
    words = ((words + (1 << 31)) % (1 << 32)) - (1 << 31)  # uint32 bits as int32
    _section(out, layout.codes, C * (CHUNK // 32), torch.int32).copy_(
        words.to(torch.int32).flatten())
    m[pos[valid]] = (m * b2 + g * c2)[pos[valid]]
    return out


def vote_counts(recv: torch.Tensor, plan: BucketPlan, layout: Layout) -> torch.Tensor:
    """int32 ``[C, CHUNK]``: ``s = N - 2 * (set bits over the N rows of recv)`` per chunk element."""
    C, N = plan.num_chunks, recv.shape[0]
    sh = torch.arange(32, dtype=torch.int64, device=recv.device)
    cnt = torch.zeros(C, CHUNK, dtype=torch.int32, device=recv.device)
    for r in range(N):
        words = _section(recv[r], layout.codes, C * (CHUNK // 32), torch.int32).to(torch.int64)
        cnt += ((words[:, None] >> sh) & 1).reshape(C, CHUNK).to(torch.int32)
    return N - 2 * cnt


def vote_apply(recv: torch.Tensor, plan: BucketPlan, layout: Layout, param: torch.Tensor,
               lr: float, weight_decay: float, aggregate: str, inv_n: float) -> None:
    """The receive side of the vote on the bucket view ``param`` (``recv``: uint8 ``[N, nbytes]``):
    ``s`` of :func:`vote_counts`, ``d = (s > 0) - (s < 0)`` (``majority``; a tie gives 0) or
    ``float(s) * inv_n`` (``average``; ``inv_n`` the fp32 value of 1 / N), then ``p = p - lr * (d
    + wd * p)``.  Integer arithmetic up to ``d``: every rank forms the same update.  Positions
    between tensors are not touched."""
    if layout.kind != "vote":
        raise ValueError(f"vote_apply given a {layout.kind!r} layout")
    if aggregate not in ("majority", "average"):
        raise ValueError("aggregate must be 'majority' or 'average'")
    s = vote_counts(recv, plan, layout)
    if aggregate == "majority":
        d = torch.sign(s).to(torch.float32)
    else:
        d = s.to(torch.float32) * float(np.float32(inv_n))
    pos, valid, _ = _sign_gather(plan, recv.device)
    at = pos[valid]
    param[at] = _lion_step(param[at], d[valid], lr, weight_decay)


def vote_reduce(recv: torch.Tensor, plan: BucketPlan, layout: Layout,
                owner_row: int) -> torch.Tensor:
    """The two-stage vote's owner step (``parallel/twostage.py TwoStageVoteExchange``): the N votes
    on one shard (``recv``: uint8 ``[N, >= nbytes]``, ``plan`` / ``layout`` the shard's) -> one
    uint8 payload of the same layout.  ``s`` of :func:`vote_counts`; the output bit is ``(s < 0)
    | ((s == 0) & bit of row owner_row)``: one bit cannot say 0, so the owner's own vote decides a
    tie -- deterministic, integer, and decided per shard (no rank decides globally).  Ties cannot
    occur at odd N.  Padding bits are 0 in every row, so ``s = N > 0`` and they stay 0.

    The push that fills ``recv`` is :func:`encode_vote` of every shard over its own plan.
    ``shard_plans`` cuts at multiples of ``CHUNK`` and tensor offsets are multiples of 64, so every
    element has the same chunk-local index parity in its shard's plan as in the bucket's plan:
    the pushed votes are the very bits of the all-gather encode, placed elsewhere.  The pull is
    :func:`vote_apply` of the owner's row alone (``majority``, N = 1: ``d = 1 - 2 * bit``).  At
    odd N the two-stage result is therefore bitwise the all-gather majority vote's, and at even N
    wherever ``s != 0``."""
    if layout.kind != "vote":
        raise ValueError(f"vote_reduce given a {layout.kind!r} layout")
    N = recv.shape[0]
    if not 0 <= int(owner_row) < N:
        raise ValueError(f"owner row {owner_row} is not one of the {N} received rows")
    C = plan.num_chunks
    s = vote_counts(recv, plan, layout)
    sh = torch.arange(32, dtype=torch.int64, device=recv.device)
    own = _section(recv[owner_row], layout.codes, C * (CHUNK // 32), torch.int32).to(torch.int64)
    own = ((own[:, None] >> sh) & 1).reshape(C, CHUNK).bool()
    neg = (s < 0) | ((s == 0) & own)
    words = (neg.reshape(C, CHUNK // 32, 32).to(torch.int64) << sh).sum(-1)
    words = ((words + (1 << 31)) % (1 << 32)) - (1 << 31)  # uint32 bits as int32
    out = torch.zeros(layout.nbytes, dtype=torch.uint8, device=recv.device)
    _section(out, layout.codes, C * (CHUNK // 32), torch.int32).copy_(
        words.to(torch.int32).flatten())
    return out


# Layer-wise trust ratios (LARS: You et al., 2017; LAMB: You et al., ICLR 2020).  The definition
# of ``ops/csrc/layerwise.hip``.  ``p`` / ``g`` / the state are views of one flat range and
# ``tensors`` its ``(offset, numel, adapts)`` rows: every norm runs over a tensor's own ``numel``
# elements, never over the alignment padding, and a tensor that does not adapt (``ndim < 2``:
# biases, BatchNorm scales) or that has a zero norm takes ratio 1.  ``g`` is already scaled.
# Both return the tensors' ratios (fp32).
def _l2(x):
    return (x * x).sum().sqrt()


def lars_apply(p, buf, g, tensors, lr, momentum, dampening, weight_decay, nesterov, first, eta):
    """``r = eta |p| / (|g| + wd |p|)``, then :func:`sgd_apply` on ``r (g + wd p)`` with its own
    weight decay off."""
    ratios = torch.ones(len(tensors), dtype=torch.float32, device=p.device)
    for t, (off, n, adapts) in enumerate(tensors):
        pt, gt = p[off:off + n], g[off:off + n]
        pn, gn = _l2(pt), _l2(gt)
        if adapts and float(pn) > 0 and float(gn) > 0:
            ratios[t] = eta * pn / (gn + weight_decay * pn)
        d = gt
        if weight_decay != 0:
            d = d + weight_decay * pt
        d = ratios[t] * d
        sgd_apply(pt, buf[off:off + n], d, lr, momentum, dampening, 0.0, nesterov, first)
    return ratios


def lamb_apply(p, m, v, g, tensors, lr, beta1, beta2, eps, weight_decay, step):
    """Adam's moments, ``u = m^ / (sqrt(v^) + eps) + wd p``, ``r = |p| / |u|``, ``p -= lr r u``
    (``step`` is 1-based; no clamp on ``|p|``, no gradient clipping)."""
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    ratios = torch.ones(len(tensors), dtype=torch.float32, device=p.device)
    for t, (off, n, adapts) in enumerate(tensors):
        pt, gt = p[off:off + n], g[off:off + n]
        mt, vt = m[off:off + n], v[off:off + n]
        mt.mul_(beta1).add_(gt, alpha=1 - beta1)
        vt.mul_(beta2).addcmul_(gt, gt, value=1 - beta2)
        u = (mt / bc1) / ((vt / bc2).sqrt() + eps)
        if weight_decay != 0:
            u = u + weight_decay * pt
        pn, un = _l2(pt), _l2(u)
        if adapts and float(pn) > 0 and float(un) > 0:
            ratios[t] = pn / un
        pt.add_(u, alpha=-(lr * float(ratios[t])))
    return ratios


# ---------------------------------------------------------------------------------------------
# Global-norm gradient clipping of one rank's local gradient (DGC's local gradient clipping;
# ``torch.nn.utils.clip_grad_norm_`` at a world of one).  The CPU path and the definition of the
# arithmetic of ``ops/csrc/clip.hip``, up to the order of the fp32 sums (free here, a fixed tree
# with an fp64 total there).
# ---------------------------------------------------------------------------------------------
CLIP_EPS = 1e-6  # torch's clip_grad_norm_ epsilon


def clip_grad_norm_(grads, max_norm: float):
    """``norm`` = the L2 norm over every element of ``grads`` (fp32 or bf16 tensors; bf16 enters
    as its exact fp32 value), ``coef = min(1, max_norm / (norm + 1e-6))``, and every tensor set to
    ``g * coef`` in place by one fp32 multiply (bf16: the fp32 product rounded to nearest even).
    A NaN norm leaves ``coef`` at 1 as C's ``fminf`` does; the NaN elements themselves stay.
    Returns ``(norm, coef)`` as 0-dim fp32 tensors."""
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError("max_norm must be > 0")
    grads = list(grads)
    norms = torch.stack([torch.linalg.vector_norm(g.detach().float()) for g in grads])
    norm = torch.linalg.vector_norm(norms)
    q = torch.tensor(max_norm, dtype=torch.float32, device=norm.device) / (norm + CLIP_EPS)
    coef = torch.where(q < 1.0, q, torch.ones_like(q))
    for g in grads:
        g = g.detach()
        if g.dtype == torch.float32:
            g.mul_(coef)
        else:
            g.copy_((g.float() * coef).to(g.dtype))
    return norm, coef


OUTER_KINDS = ("sgd", "nesterov")


def outer_apply(anchor, data, momentum, delta, lr, mu, nesterov, shadow=None, stats=None):
    """Local SGD's outer step on the flat fp32 views, in place (the CPU path and the definition of
    ``ops/csrc/outer.hip``'s arithmetic; every product and sum rounded on its own)::

        u      = u * mu + d
        s      = d + u * mu        (nesterov)      |      s = u
        anchor = anchor + lr * s
        data   = anchor            (and the bf16 shadow, rounded to nearest even)

    ``torch.optim.SGD(lr, momentum=mu, nesterov=...)`` on the pseudo-gradient ``-d`` with the
    momentum buffer starting from the first gradient (= from zero, dampening 0): heavy ball is
    SlowMo / BMUF, Nesterov with 0.7 / 0.9 DiLoCo.  With ``lr = 1, mu = 0`` and ``sgd`` it is
    ``anchor + d`` bit for bit (``u * 0`` is +0, so a ``d`` of -0 enters as +0: that changes a bit
    only where ``anchor`` itself is -0).

    ``stats`` (fp32 ``[ceil(n / 8192), 2]``): per row of 8192 elements the sums of squares of
    ``d`` and of the new ``u``, formed in fp64 here (the kernel's fp32 tree is within
    ``ops.CLIP_SUM_CHAIN + 1`` roundings of it)."""
    lr, mu = float(np.float32(lr)), float(np.float32(mu))
    d = delta.to(torch.float32)
    momentum.copy_(momentum * mu + d)
    s = d + momentum * mu if nesterov else momentum
    anchor.copy_(anchor + s * lr)
    data.copy_(anchor)
    if shadow is not None:
        shadow.copy_(anchor)
    if stats is not None:
        rows = stats.shape[0]
        pad = rows * CHUNK - d.numel()
        for k, v in enumerate((d, momentum)):
            sq = torch.nn.functional.pad(v.double(), (0, pad)).view(rows, CHUNK)
            stats[:, k] = (sq * sq).sum(1).to(torch.float32)


# ---------------------------------------------------------------------------------------------
# PowerSGD (Vogels et al., NeurIPS 2019; torch's ``powerSGD_hook``): rank-r factors of the
# error-compensated gradient matrices of one bucket (``plan.LowRankPlan``).  The CPU path and the
# definition of the arithmetic of ``ops/csrc/powersgd.hip``.  Every function works in ``dtype``
# on buffers of that dtype (fp32; the tests run the same code in fp64).
# ---------------------------------------------------------------------------------------------
POWERSGD_EPS = 1e-8  # torch's _orthogonalize_gram_schmidt epsilon


def _psgd_block(buf, off, rows, r):
    return buf[off:off + rows * r].view(rows, r)


def powersgd_project(grad, resid, q, lrp, dtype=torch.float32):
    """``resid <- M = grad + resid`` on the compressed tensors (in place; dense tensors keep no
    residual) and the P buffer: ``P_t = M_t Q_t`` per matrix, the dense gradients in the tail."""
    r = lrp.rank
    p = torch.zeros(lrp.p_floats, dtype=dtype, device=grad.device)
    for off, n, m, po, qo, _ in lrp.mats:
        M = resid[off:off + n * m].view(n, m)
        M.add_(grad[off:off + n * m].view(n, m).to(dtype))
        _psgd_block(p, po, n, r).copy_(M @ _psgd_block(q, qo, m, r).to(dtype))
    for off, numel, tail, _ in lrp.dense:
        p[tail:tail + numel] = grad[off:off + numel].to(dtype)
    return p


def powersgd_orthogonalize(p, lrp, inv_n=1.0, dtype=torch.float32):
    """In place: every P block times ``inv_n`` (the all-reduce's average), then modified
    Gram-Schmidt over its columns in order, ``col /= (|col| + 1e-8)`` (torch's
    ``_orthogonalize_gram_schmidt`` with its non-zero epsilon).  The dense tail is not touched."""
    r = lrp.rank
    inv = torch.tensor(inv_n, dtype=torch.float32).to(dtype)
    for _, n, _, po, _, _ in lrp.mats:
        P = _psgd_block(p, po, n, r)
        P.mul_(inv)
        for c in range(r):
            col = P[:, c:c + 1]
            col.div_(torch.sqrt((col * col).sum()) + POWERSGD_EPS)
            if c + 1 < r:
                rest = P[:, c + 1:]
                rest.sub_((col * rest).sum(dim=0, keepdim=True) * col)
    return p


def powersgd_backproject(resid, p, lrp, dtype=torch.float32):
    """The Q buffer: ``Q_t = M_t^T P_t`` per matrix (``resid`` holds M)."""
    r = lrp.rank
    q = torch.zeros(lrp.q_floats, dtype=dtype, device=p.device)
    for off, n, m, po, qo, _ in lrp.mats:
        M = resid[off:off + n * m].view(n, m)
        _psgd_block(q, qo, m, r).copy_(M.t() @ _psgd_block(p, po, n, r))
    return q


def powersgd_reconstruct_apply(resid, p, q, lrp, inv_n=1.0, param=None, mom=None, hp=None,
                               first=False, grad_out=None, dtype=torch.float32):
    """``Qa = q * inv_n``; per matrix ``g^ = P Qa^T`` with ``g^[i, j] = ((P[i,0] Qa[j,0] + P[i,1]
    Qa[j,1]) + ...)`` in ascending k, every multiply and add rounded on its own, and ``resid <- M
    - g^``; a dense tensor's ``g^`` is its tail times ``inv_n``.  ``grad_out`` (bucket view)
    receives ``g^``; ``param`` / ``mom`` / ``hp``: the SGD step with ``g^`` (``sgd_apply``).
    Returns ``Qa``, the next step's warm start.  The kernel reproduces all of it bit for bit."""
    r = lrp.rank
    inv = torch.tensor(inv_n, dtype=torch.float32).to(dtype)
    qa = q[:lrp.q_floats] * inv
    pieces = []
    for off, n, m, po, qo, _ in lrp.mats:
        P, Q = _psgd_block(p, po, n, r), _psgd_block(qa, qo, m, r)
        g = P[:, 0:1] * Q[:, 0][None, :]
        for k in range(1, r):
            g = g + P[:, k:k + 1] * Q[:, k][None, :]
        M = resid[off:off + n * m].view(n, m)
        M.sub_(g)
        pieces.append((off, n * m, g.reshape(-1)))
    for off, numel, tail, _ in lrp.dense:
        pieces.append((off, numel, p[tail:tail + numel] * inv))
    for off, numel, g in pieces:
        if grad_out is not None:
            grad_out[off:off + numel].copy_(g)
        if param is not None:
            sgd_apply(param[off:off + numel], None if mom is None else mom[off:off + numel], g,
                      hp["lr"], hp["momentum"], hp["dampening"], hp["weight_decay"],
                      hp["nesterov"], first)
    return qa


def powersgd_init_q(lrp, seed: int, bucket: int, dtype=torch.float32):
    """The initial Q buffer: per matrix, counter-RNG uniforms (``rng.uniform``, key of (seed,
    bucket, tensor)) mapped to [-1, 1), orthogonalised once.  The same on every rank."""
    r = lrp.rank
    q = torch.zeros(lrp.q_floats, dtype=dtype)
    for _, _, m, _, qo, t in lrp.mats:
        u = rng.uniform(torch.arange(m * r, dtype=torch.int64), rng.stream_key(seed, bucket, t))
        Q = _psgd_block(q, qo, m, r)
        Q.copy_((u * 2.0 - 1.0).to(dtype).view(m, r))
        for c in range(r):
            col = Q[:, c:c + 1]
            col.div_(torch.sqrt((col * col).sum()) + POWERSGD_EPS)
            if c + 1 < r:
                rest = Q[:, c + 1:]
                rest.sub_((col * rest).sum(dim=0, keepdim=True) * col)
    return q


# ---------------------------------------------------------------------------------------------
# Count sketch (SketchedSGD, Ivkin et al., NeurIPS 2019; no reference counterpart): the table of
# the error-compensated gradient of one bucket (``plan.SketchPlan``), the per-coordinate estimate
# from the summed table, and the gather of the selected coordinates' own values.  The CPU path
# and the definition of every bit of ``ops/csrc/sketch_codec.hip``.  The selection between the
# estimate and the gather is the project's top-k (``encode_topk`` of the estimate in the ``topk``
# layout: its count / index / bitmap sections are the selection) and the apply is ``decode_sum``
# of the one summed payload.
# ---------------------------------------------------------------------------------------------
SKETCH_SHIFT_TAG = 0x534B5348  # "SKSH": the rank slot of stream_key, as ROT_TAG
SKETCH_SIGN_TAG = 0x534B5347  # "SKSG"


def sketch_keys(seed: int, bucket: int):
    """(sk_key, sg_key) of a bucket: the keys of the column shifts and of the signs, the same on
    every rank and every step."""
    return (rng.stream_key(seed, bucket, SKETCH_SHIFT_TAG),
            rng.stream_key(seed, bucket, SKETCH_SIGN_TAG))


def _sketch_hash(sp, start: int, ln: int, device) -> torch.Tensor:
    """``mix32(gidx ^ sg_key)`` of ``ln`` consecutive elements from bucket offset ``start``; bit
    j is their sign in row j."""
    gidx = sp.plan.bucket_offset + start + torch.arange(ln, dtype=torch.int64, device=device)
    return rng.mix32((gidx & rng.M32) ^ sp.sg_key)


def _sketch_signed(x: torch.Tensor, h: torch.Tensor, j: int) -> torch.Tensor:
    return torch.where(((h >> j) & 1).bool(), -x, x)


def sketch_stage(grad: torch.Tensor, resid: torch.Tensor, sp) -> None:
    """``resid <- acc = grad + resid`` on the sketched tensors (in place; a dense tensor keeps no
    residual)."""
    for t in sp.sketched:
        off, n = sp.plan.offsets[t], sp.plan.numels[t]
        resid[off:off + n] = grad[off:off + n] + resid[off:off + n]


def sketch_accumulate(resid: torch.Tensor, sp) -> torch.Tensor:
    """The table ``T[R][W]`` (flat, row-major) of the staged ``resid``.  Per row: the chunks in
    groups of ``SKETCH_SUM_GROUP`` consecutive chunk indices; within a group sequential fp32 adds
    in ascending chunk order from +0.0, then the group partials in ascending group order from
    +0.0.  (A chunk adds nothing to the columns outside its image, which is bitwise adding +0.0:
    no sum here is ever -0.0.)"""
    from .plan import SKETCH_SUM_GROUP

    W = sp.W
    table = torch.zeros(sp.rows * W, dtype=torch.float32, device=resid.device)
    C = sp.plan.num_chunks
    for j in range(sp.rows):
        total = table[j * W:(j + 1) * W]
        for g0 in range(0, C, SKETCH_SUM_GROUP):
            part = torch.zeros(W, dtype=torch.float32, device=resid.device)
            for c in range(g0, min(g0 + SKETCH_SUM_GROUP, C)):
                start, ln = sp.chunk_rows[c]
                if ln == 0:
                    continue
                o = sp.shifts[j][c]
                v = _sketch_signed(resid[start:start + ln],
                                   _sketch_hash(sp, start, ln, resid.device), j)
                head = min(ln, W - o)
                part[o:o + head] += v[:head]
                if head < ln:  # the image wraps
                    part[:ln - head] += v[head:]
            total += part
    return table


def _cx(a, b):
    s = b < a
    return torch.where(s, b, a), torch.where(s, a, b)


def sketch_median(v):
    """The median of 1, 3 or 5 tensors by a compare-exchange network (a select on ``b < a``: no
    arithmetic; equal values and NaNs stay in place), as the kernel's ``sk_median``."""
    v = list(v)
    if len(v) == 3:
        order = ((0, 1), (1, 2), (0, 1))
    elif len(v) == 5:
        order = ((0, 1), (3, 4), (2, 4), (2, 3), (1, 4), (0, 3), (0, 2), (1, 3), (1, 2))
    elif len(v) == 1:
        order = ()
    else:
        raise ValueError("the median network takes 1, 3 or 5 values")
    for a, b in order:
        v[a], v[b] = _cx(v[a], v[b])
    return v[len(v) // 2]


def sketch_estimate(table: torch.Tensor, sp) -> torch.Tensor:
    """fp32 [plan.length]: ``est[i]`` = the median over the rows of ``sign_j(i) * T[j][(p +
    o[j][c]) mod W]``; 0 on dense tensors and pads."""
    W = sp.W
    est = torch.zeros(sp.plan.length, dtype=torch.float32, device=table.device)
    for c, (start, ln) in enumerate(sp.chunk_rows):
        if ln == 0:
            continue
        h = _sketch_hash(sp, start, ln, table.device)
        p = torch.arange(ln, dtype=torch.int64, device=table.device)
        est[start:start + ln] = sketch_median(
            [_sketch_signed(table[j * W + (p + sp.shifts[j][c]) % W], h, j)
             for j in range(sp.rows)])
    return est


def sketch_select(est: torch.Tensor, sp, layout: Layout) -> torch.Tensor:
    """The ``topk`` payload of the estimate: per tensor ``topk_indices(est, k)`` in its count /
    index / bitmap sections (the values section holds the estimates until the gather)."""
    if layout.kind != "topk":
        raise ValueError("the sketch selects through the plain top-k layout")
    return encode_topk(est, sp.plan, layout, 0, "max", 0)


def sketch_gather(payload: torch.Tensor, grad: torch.Tensor, resid: torch.Tensor, sp,
                  layout: Layout) -> None:
    """The payload's values section <- this rank's ``acc`` at the selected coordinates in payload
    order (``grad`` itself on dense tensors), and ``resid[selected] = 0`` (in place)."""
    pos, _ = _decoded_entries(payload, sp.plan, layout, 0)
    src = resid.clone()
    for t, d in enumerate(sp.dense):
        if d:
            off, n = sp.plan.offsets[t], sp.plan.numels[t]
            src[off:off + n] = grad[off:off + n]
    _section(payload, layout.codes, sp.plan.total_k, torch.float32).copy_(src[pos])
    resid[pos] = 0.0  # dense tensors' residual is 0 already


# ---------------------------------------------------------------------------------------------
# IntSGD (Mishchenko, Wang, Kovalev, Richtarik, ICLR 2022; no reference counterpart): every rank
# multiplies its gradient by the same scale ``alpha``, rounds stochastically to integers and the
# int8 codes are summed by a plain all-reduce.  The CPU path and the definition of every bit of
# ``ops/csrc/intsgd_codec.hip``.
# ---------------------------------------------------------------------------------------------
INTSGD_BETA = 0.9  # the moving average of the squared update norm
INTSGD_EPS2 = 1e-16


def intsgd_q(world: int) -> int:
    """The largest code of one rank: ``floor(127 / world)``, so no sum of ``world`` codes leaves
    int8's [-127, 127]."""
    if not 1 <= int(world) <= 127:
        raise ValueError(f"IntSGD's int8 wire holds the sum of at most 127 ranks' codes, not of "
                         f"{world} (q = floor(127 / world) would be 0)")
    return 127 // int(world)


def _f32t(v: float, device) -> torch.Tensor:
    return torch.tensor(v, dtype=torch.float32, device=device)


def encode_intsgd(g: torch.Tensor, plan: BucketPlan, layout: Layout, alpha: float, inv_a: float,
                  q: int, key: int, residual: torch.Tensor = None):
    """IntSGD of one bucket -> (uint8 payload ``codes i8[L]``, int32 saturation count per chunk
    row); ``L = plan.length``, pads 0, every byte written.

    ``acc = g`` (``g + residual`` under error feedback).  Per element of a tensor: ``y = acc *
    alpha`` (one fp32 multiply), ``f = floorf(y)``, ``u = uniform(gidx, key)`` on QSGD's streams
    (``gidx = bucket_offset + position``), ``code = f + (u < y - f)`` -- ``y - f`` is exact in
    fp32, so an integer ``y`` never moves and negatives round correctly -- clamped to ``[-q, q]``;
    an inf clamps, a NaN codes 0.  An element whose ``y`` was NaN or lay outside ``[-q, q]`` counts
    as saturated.  ``residual = acc - float(code) * inv_a``: what clipping removes is fed back.
    ``alpha`` / ``inv_a`` are fp32 values (:func:`intsgd_alpha`), the same on every rank."""
    if layout.kind != "intsgd":
        raise ValueError(f"encode_intsgd given a {layout.kind!r} layout")
    L, dev = plan.length, g.device
    acc = g.to(torch.float32)[:L]
    if residual is not None:
        acc = acc + residual[:L]
    own = _mx_mask(plan, dev)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    y = acc * _f32t(alpha, dev)
    fl = torch.floor(y)
    u = rng.uniform(plan.bucket_offset + torch.arange(L, dtype=torch.int64, device=dev), key)
    code = fl + (u < (y - fl)).to(torch.float32)
    code = torch.clamp(code, -float(q), float(q))
    code = torch.where(torch.isnan(y) | ~own, zero, code)
    icode = code.to(torch.int32)
    out = torch.zeros(layout.nbytes, dtype=torch.uint8, device=dev)
    out[:L] = icode.to(torch.int8).view(torch.uint8)
    satm = own & ~((y >= -float(q)) & (y <= float(q)))
    sat = torch.tensor([int(satm[s0:s0 + n].sum()) for s0, n in
                        zip(plan.chunk_start, plan.chunk_len)], dtype=torch.int32, device=dev)
    if residual is not None:
        left = acc - icode.to(torch.float32) * _f32t(inv_a, dev)
        residual[:L][own] = left[own]
    return out, sat


def intsgd_update_partials(p_new: torch.Tensor, p_old: torch.Tensor,
                           plan: BucketPlan) -> torch.Tensor:
    """fp32 ``[C]``: per chunk row the sum of ``(p_new - p_old)^2`` over the tensor's own
    elements -- each fp32 difference taken once, squared, and summed through ``k_clip_norm``'s
    tree (:func:`_sign_chunk_sums`; a chain of ``ops.CLIP_SUM_CHAIN`` additions at most)."""
    pos, valid, _ = _sign_gather(plan, p_new.device)
    d = (p_new[:plan.length] - p_old[:plan.length])[pos]
    d = torch.where(valid, d, torch.zeros((), dtype=torch.float32, device=d.device))
    return _sign_chunk_sums(d * d)


def intsgd_apply(summed: torch.Tensor, plan: BucketPlan, layout: Layout, inv_na: float,
                 param: torch.Tensor, mom: torch.Tensor, hp: dict, first: bool,
                 partials: torch.Tensor = None) -> None:
    """The receive side on the bucket views ``param`` / ``mom``: ``s`` = the summed byte read as
    int8 (0x80 is -128: nothing is special-cased), ``g^ = float(s) * inv_na``, then
    :func:`sgd_apply` per tensor.  ``partials`` (fp32 ``[C]``) receives
    :func:`intsgd_update_partials` of the step."""
    if layout.kind != "intsgd":
        raise ValueError(f"intsgd_apply given a {layout.kind!r} layout")
    L = plan.length
    g = summed[:L].view(torch.int8).to(torch.float32) * _f32t(inv_na, summed.device)
    old = param[:L].clone() if partials is not None else None
    for off, n in zip(plan.offsets, plan.numels):
        sgd_apply(param[off:off + n], None if mom is None else mom[off:off + n], g[off:off + n],
                  hp["lr"], hp["momentum"], hp["dampening"], hp["weight_decay"], hp["nesterov"],
                  first)
    if partials is not None:
        partials.copy_(intsgd_update_partials(param, old, plan))


def intsgd_alpha(partials: torch.Tensor, r: float, steps: int, lr: float, numel: int,
                 world: int) -> dict:
    """The scale after an update, this project's form of the paper's Algorithm 2.  ``S`` = all
    chunk rows' partials (every bucket's, in index order) summed sequentially in fp64; ``r = S``
    the first time (``steps == 0``), else ``beta r + (1 - beta) S``; in fp64 ``alpha = lr
    sqrt(numel) / sqrt(2 world r + eps2)`` with the fp32 ``lr``, rounded to fp32; ``inv_a = fl32(1
    / alpha)`` and ``inv_na = fl32(1 / (alpha world))`` of the rounded ``alpha``, both 0 when it is
    0.  ``r`` stays fp64.  Returns the new state ``{r, s_last, alpha, inv_a, inv_na, steps}``."""
    import math

    s = 0.0
    for v in partials.detach().to("cpu", torch.float64).tolist():
        s += v
    r = INTSGD_BETA * float(r) + (1.0 - INTSGD_BETA) * s if steps else s
    den = 2.0 * float(world) * r + INTSGD_EPS2
    num = float(np.float32(lr)) * math.sqrt(float(numel))
    with np.errstate(all="ignore"):
        a64 = num / math.sqrt(den) if den >= 0.0 else float("nan")  # a NaN r: a NaN scale
        alpha = np.float32(a64)
        inv_a = inv_na = np.float32(0.0)
        if alpha != 0:
            inv_a = np.float32(np.float64(1.0) / np.float64(alpha))
            inv_na = np.float32(np.float64(1.0) / (np.float64(alpha) * np.float64(world)))
    return dict(r=r, s_last=s, alpha=float(alpha), inv_a=float(inv_a), inv_na=float(inv_na),
                steps=int(steps) + 1)
