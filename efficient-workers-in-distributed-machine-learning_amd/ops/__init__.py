"""Python entry points of the hand-written gfx950 kernels (``ops/csrc/*.hip``).

Every wrapper validates shapes/dtypes/alignment on the host (a kernel launched on a bad operand can
fault the whole GPU node), then launches on torch's *current* HIP stream so calls compose with
``torch.cuda.stream(...)`` and are captured by ``torch.cuda.graph``.

These wrappers only accept device tensors.  CPU execution (Gloo tests) goes through the torch
oracle in ``compress/oracle.py``; there is no silent fallback on the GPU: if the extension is not
built, :func:`require` raises.
"""
import importlib
import os

import torch

_IMPORT_ERROR = None
try:  # torch is imported first so the extension binds to torch's already-loaded HIP runtime
    _ALT = os.environ.get("EWDML_EXT")  # A/B of a compile-time variant: another built _C .so
    if _ALT:
        import importlib.util
        import sys as _sys

        _spec = importlib.util.spec_from_file_location(__name__ + "._C", _ALT)
        _C = importlib.util.module_from_spec(_spec)
        _spec.loader.exec_module(_C)
        _sys.modules[__name__ + "._C"] = _C
    else:
        _C = importlib.import_module(__name__ + "._C")
except ImportError as e:  # pragma: no cover - depends on the build
    _C = None
    _IMPORT_ERROR = e

VK_Q8, VK_Q4, VK_F32 = 0, 1, 2

_SYNC_DEBUG = os.environ.get("EWDML_SYNC_DEBUG") == "1"


class _SyncDebug:
    """``--sync-debug`` / EWDML_SYNC_DEBUG=1: synchronise the device after every custom kernel
    launch so a fault, race or bad operand is reported at the launch that caused it."""

    def __init__(self, mod):
        self._m = mod

    def __getattr__(self, name):
        f = getattr(self._m, name)
        if not callable(f):
            return f

        def call(*a, **k):
            r = f(*a, **k)
            if _SYNC_DEBUG:
                torch.cuda.synchronize()
            return r
        return call


def set_sync_debug(on: bool = True):
    global _SYNC_DEBUG
    _SYNC_DEBUG = bool(on)


def available() -> bool:
    return _C is not None


def require():
    if _C is None:
        raise RuntimeError(
            "ewdml HIP extension is not built or failed to load "
            f"({_IMPORT_ERROR}); run `python -m ewdml.ops.build` (or __graft_entry__.build())")
    return _SyncDebug(_C) if _SYNC_DEBUG else _C


def library_path():
    return getattr(_C, "__file__", None)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def _args(cls, **fields):
    """An argument struct of the extension (``csrc/ewdml_ops.h``, bound as a class in
    ``csrc/bindings.cpp``) filled by field name: every field not named stays zero, and a name the
    struct does not have raises ``AttributeError``."""
    a = cls()
    for name, value in fields.items():
        setattr(a, name, value)
    return a


def _tables(dp):
    """The chunk and tensor tables of a bucket's ``DevicePlan``, as argument fields."""
    return dict(chunks=_ptr(dp.chunks), num_chunks=dp.plan.num_chunks,
                tensors=_ptr(dp.tensors), num_tensors=dp.plan.num_tensors)


def _rows(recv, nranks, stride):
    """The gathered payloads a receive side reads: ``nranks`` rows ``stride`` bytes apart."""
    return dict(recv=_ptr(recv), nranks=nranks, stride=stride)


def _check(t, dtype, name, align=16, dense=False):
    """``dense``: any non-overlapping dense layout is fine (the kernel reads the tensor in memory
    order, e.g. a channels_last conv-weight gradient matching its channels_last parameter)."""
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not (t.is_contiguous() or (dense and t.dim() == 4
                                  and t.is_contiguous(memory_format=torch.channels_last))):
        raise ValueError(f"{name} must be contiguous")
    if t.data_ptr() % align:
        raise ValueError(f"{name} must be {align}-byte aligned")


class DevicePlan:
    """Device-resident tables + scratch for one bucket (built once, reused every step)."""

    def __init__(self, plan, device):
        self.plan = plan
        self.tensors = plan.tensor_table(device)
        self.chunks = plan.chunk_table(device)
        self.cblocks = plan.cblock_table(device)  # predictive top-k encode's candidate passes
        C, T = plan.num_chunks, plan.num_tensors
        nbytes = max(require().topk_scratch_bytes(T, C, plan.length, plan.total_cap),
                     require().qsgd_scratch_bytes(T, C))
        self.scratch = torch.zeros(nbytes, dtype=torch.uint8, device=device)


# EWDML_TOPK_PREDICT=0: every top-k encode takes the full passes (A/B of the predictive encode)
_TOPK_PREDICT = os.environ.get("EWDML_TOPK_PREDICT", "1") != "0"
_LB_FAULT = [False]


def set_lookback_fault(on: bool):
    """Test hook: the next top-k encodes' first chunks skip their look-back word, so every later
    chunk of a tensor polls to the bound and reports through the error counter."""
    _LB_FAULT[0] = bool(on)


def topk_stats(dp) -> dict:
    """Counters of a bucket's top-k encodes (synchronises): ``lookback_errors`` (write blocks that
    gave up waiting on a predecessor's look-back word: their payload offsets are wrong -- must be
    0), and the tensor-encodes of the predictive encode on the ``fast`` (candidates only) and the
    ``full`` path (``full_by_tensor``: the first 28 tensors' share of the latter, as [too few
    candidates, too many] pairs)."""
    v = require().topk_stats(_ptr(dp.scratch), dp.plan.num_tensors, dp.plan.num_chunks)
    e, fast, full = v[:3]
    return {"lookback_errors": e, "fast": fast, "full": full,
            "full_by_tensor": [[x & 0xFFFF, x >> 16] for x in v[3:3 + dp.plan.num_tensors]]}


_GRAPH_NODE_TYPES = ["kernel", "memcpy", "memset", "host", "graph", "empty", "wait_event",
                     "event_record", "ext_semas_signal", "ext_semas_wait", "mem_alloc", "mem_free",
                     "memcpy_from_symbol", "memcpy_to_symbol", "batch_mem_op", "t15"]


def graph_info(graph, dot_path: str = "") -> dict:
    """Node / edge counts of a captured graph kept with ``torch.cuda.CUDAGraph(keep_graph=True)``
    (``raw_cuda_graph()``): a straight line has no forks or joins and one root."""
    v = require().graph_info(int(graph), dot_path)
    types = {_GRAPH_NODE_TYPES[i]: int(c) for i, c in enumerate(v[5:]) if c}
    return {"nodes": v[0], "edges": v[1], "forks": v[2], "joins": v[3], "roots": v[4],
            "linear": v[2] == 0 and v[3] == 0 and v[4] <= 1, "types": types}


def topk_lookback_errors(dp) -> int:
    """Times a top-k write block gave up waiting on a predecessor's look-back word (bounded spin;
    0 unless something is badly wrong).  Synchronises."""
    return require().topk_lookback_errors(_ptr(dp.scratch), dp.plan.num_tensors,
                                          dp.plan.num_chunks)


def _check_bucket(dp, grad, name="grad"):
    _check(grad, torch.float32, name)
    if grad.numel() < dp.plan.length:
        raise ValueError(f"{name} has {grad.numel()} elements, bucket needs {dp.plan.length}")


MAX_TENSORS_PER_BUCKET = 128  # EW_MAX_T in csrc/common.h


def grad_pointers(dp, grad):
    """(pointers, bf16 bit mask) of a bucket's per-tensor gradients.  ``grad`` is the bucket's
    flat fp32 view (tensors at the plan offsets) or a list with one fp32/bf16 tensor per plan
    tensor (autograd's own ``p.grad`` tensors, read in place)."""
    plan = dp.plan
    if plan.num_tensors > MAX_TENSORS_PER_BUCKET:
        raise ValueError(f"bucket has {plan.num_tensors} tensors (max {MAX_TENSORS_PER_BUCKET})")
    mask = [0] * (MAX_TENSORS_PER_BUCKET // 32)
    if torch.is_tensor(grad):
        _check_bucket(dp, grad)
        base = grad.data_ptr()
        return [base + 4 * o for o in plan.offsets], mask
    if len(grad) != plan.num_tensors:
        raise ValueError(f"{len(grad)} gradients for a bucket of {plan.num_tensors} tensors")
    ptrs = []
    for i, (t, n) in enumerate(zip(grad, plan.numels)):
        if t.dtype == torch.bfloat16:
            _check(t, torch.bfloat16, "grad tensor", align=8, dense=True)
            mask[i >> 5] |= 1 << (i & 31)
        else:
            _check(t, torch.float32, "grad tensor", dense=True)
        if t.numel() != n:
            raise ValueError(f"gradient has {t.numel()} elements, plan expects {n}")
        ptrs.append(t.data_ptr())
    return ptrs, mask


def _check_shadow(dp, shadow):
    if shadow is not None:
        _check(shadow, torch.bfloat16, "shadow", align=8)
        if shadow.numel() < dp.plan.length:
            raise ValueError("shadow too small for the bucket")


def _keyp(key_tensor):
    if key_tensor is None:
        return 0
    if not key_tensor.is_cuda or key_tensor.dtype != torch.int32 or key_tensor.numel() < 1:
        raise ValueError("key_tensor must be a device int32 tensor")
    return key_tensor.data_ptr()


def _encode_dst(payload, layout):
    """An encode's destination: a uint8 buffer of at least the layout's bytes."""
    _check(payload, torch.uint8, "payload")
    if payload.numel() < layout.nbytes:
        raise ValueError("payload too small")


def _recv_rows(recv, layout) -> int:
    """A decode's source: the gathered ``[nranks, layout.nbytes]`` payloads; returns nranks."""
    _check(recv, torch.uint8, "recv")
    if recv.dim() != 2 or recv.shape[1] != layout.nbytes or not 1 <= recv.shape[0] <= 64:
        raise ValueError(f"recv must be [nranks, {layout.nbytes}] with 1 <= nranks <= 64")
    return recv.shape[0]


def _step(dp, param, mom, grad_out, shadow, lr, momentum, dampening, weight_decay, grad_scale,
          nesterov, first, key_state, key_seed, key_rank, lr_tensor, need_mom=False):
    """The receive-side step every ``*_decode_apply`` ends in, checked against the bucket of
    ``dp`` and packed for the extension: the decoded mean to ``grad_out`` and / or the fused SGD
    step on ``param`` (``mom`` None: a step without momentum, unless the kernel reads the buffer
    regardless: ``need_mom``)."""
    apply = param is not None
    if apply:
        _check_bucket(dp, param, "param")
        if mom is not None:
            _check_bucket(dp, mom, "mom")
        elif need_mom or momentum != 0.0 or nesterov:
            raise ValueError("a momentum step needs the momentum buffer")
    if grad_out is not None:
        _check_bucket(dp, grad_out, "grad_out")
    if not apply and grad_out is None:
        raise ValueError("nothing to do: pass param/mom and/or grad_out")
    _check_shadow(dp, shadow)
    return require().StepArgs(
        param=_ptr(param), mom=_ptr(mom) if apply else 0, grad_out=_ptr(grad_out),
        shadow=_ptr(shadow), lr=lr, momentum=momentum, dampening=dampening,
        weight_decay=weight_decay, grad_scale=grad_scale, nesterov=int(nesterov),
        first=int(first), apply=int(apply), key_state=_keyp(key_state),
        key_seed=key_seed & 0xFFFFFFFF, key_rank=key_rank & 0xFFFFFFFF, lr_ptr=_lrp(lr_tensor))


def topk_encode(dp: DevicePlan, grad, payload, layout, levels: int, norm: str, key: int,
                resid=None, key_tensor=None, dgc=None, apply=None, predict=None):
    """``predict`` False: this encode takes the exact full passes whatever EWDML_TOPK_PREDICT
    says (the count sketch's selection, whose input is not a gradient that drifts slowly).

    ``dgc``: momentum-corrected error feedback, ``{velocity, momentum, dampening, nesterov,
    weight_decay, param}`` (bucket views; compress/oracle.py dgc_accumulate).

    ``apply`` (a world of one, where the all-gathered payload is this rank's own): the write pass
    also applies the update ``topk_decode_apply`` would with no momentum buffer --
    ``{param, lr, lr_tensor, grad_scale, shadow, key_state, key_seed, key_rank}``: at each sent
    coordinate p -= lr * grad_scale * sent (and the bf16 shadow), then the RNG key state moves to
    the next step; bitwise the decode's result (tests/kernels/test_hip_codecs.py)."""
    C = require()
    ptrs, mask = grad_pointers(dp, grad)
    _encode_dst(payload, layout)
    if resid is not None:
        _check_bucket(dp, resid, "resid")
    if layout.kind == "topk":
        vk = VK_F32
    elif layout.bits == 8:
        vk = VK_Q8
    else:
        vk = VK_Q4
    if vk != VK_F32 and not (1 <= levels <= (127 if layout.bits == 8 else 7)):
        raise ValueError(f"levels={levels} does not fit {layout.bits}-bit codes")
    vel = par = lrt = None
    mom = damp1 = wd = 0.0
    nest, dmask = 0, 1
    if dgc is not None:
        if resid is None:
            raise ValueError("momentum correction needs the residual")
        vel, mom = dgc["velocity"], float(dgc["momentum"])
        _check_bucket(dp, vel, "velocity")
        damp1 = float(1.0 - dgc.get("dampening", 0.0))
        wd = float(dgc.get("weight_decay", 0.0))
        nest = int(bool(dgc.get("nesterov", False)))
        dmask = int(bool(dgc.get("mask", True)))
        if dgc.get("lr") is not None:  # error feedback on the update: the lr inside
            lrt = dgc.get("lr_t")
            if lrt is None:
                raise ValueError("lr-scaled accumulation on the GPU needs the device lr (lr_t)")
        if wd != 0.0:
            par = dgc["param"]
            _check_bucket(dp, par, "param")
    C.topk_encode(_args(
        C.TopkEncodeArgs, resid=_ptr(resid), scratch=_ptr(dp.scratch), payload=_ptr(payload),
        payload_bytes=layout.nbytes, scales_off=layout.scales, counts_off=layout.counts,
        idx_off=layout.idx, codes_off=layout.codes, bitmap_off=layout.bitmap, value_kind=vk,
        norm_l2=1 if norm == "l2" else 0, levels=float(levels), inv_levels=float(1.0 / levels),
        key=key & 0xFFFFFFFF, bucket_offset=dp.plan.bucket_offset & 0xFFFFFFFF,
        key_ptr=_keyp(key_tensor), stream=_stream(), vel=_ptr(vel), param=_ptr(par),
        dgc_momentum=mom, dgc_damp1=damp1, dgc_wd=wd, dgc_nesterov=nest, dgc_mask=dmask,
        dgc_lr_ptr=_lrp(lrt), bucket_len=dp.plan.length, cblocks=_ptr(dp.cblocks),
        num_cblocks=dp.plan.num_cblocks,
        predict=int(_TOPK_PREDICT if predict is None else bool(predict)),
        lb_fault=int(_LB_FAULT[0]),
        max_k=int(max(dp.plan.ks)) if dp.plan.ks else 0, **_tables(dp),
        **_apply_args(dp, apply, norm), dgc_stamps=_stamps_ptr(dp, dgc)), ptrs, mask)


def _stamps_ptr(dp, dgc):
    """The producer-staging stamp words of a momentum-corrected encode (``dgc["stamps"]``:
    int32 [T] device tensor, 1 = that tensor's producer already staged it this step)."""
    st = None if dgc is None else dgc.get("stamps")
    if st is None:
        return 0
    _check(st, torch.int32, "stamps", align=4)
    if st.numel() < dp.plan.num_tensors:
        raise ValueError("one stamp word per tensor of the bucket")
    return st.data_ptr()


def topk_one_launch(dp) -> bool:
    """Whether this bucket's top-k encode runs as the one-launch kernel (k_pk_one: every chunk
    block resident)."""
    return _TOPK_PREDICT and dp.plan.num_chunks <= require().topk_one_max_blocks()


def _apply_args(dp, apply, norm):
    """The ``apply_*`` fields of a top-k encode (``apply`` None: off, none of them set)."""
    if apply is None:
        return {}
    if not _TOPK_PREDICT or norm != "max":
        raise ValueError("the write-pass apply needs the predictive (max-norm) encode")
    param = apply["param"]
    _check_bucket(dp, param, "param")
    _check_shadow(dp, apply.get("shadow"))
    ks = apply.get("key_state")
    if ks is not None:
        _check(ks, torch.int32, "key_state", align=4)
    dense = "mom" in apply  # receiver-side momentum SGD over every element (one-launch only)
    mom = apply.get("mom")
    if dense:
        if mom is None or not topk_one_launch(dp):
            raise ValueError("the dense write-pass apply needs the momentum buffer and the "
                             "one-launch encode")
        _check_bucket(dp, mom, "mom")
    return dict(
        apply_param=_ptr(param), apply_shadow=_ptr(apply.get("shadow")),
        apply_lr=float(apply["lr"]), apply_lr_ptr=_lrp(apply.get("lr_tensor")),
        apply_scale=float(apply.get("grad_scale", 1.0)), apply_key_state=_ptr(ks),
        apply_key_seed=int(apply.get("key_seed", 0)) & 0xFFFFFFFF,
        apply_key_rank=int(apply.get("key_rank", 0)) & 0xFFFFFFFF, apply_mom_set=int(dense),
        apply_mom=_ptr(mom), apply_momentum=float(apply.get("momentum", 0.0)),
        apply_dampening=float(apply.get("dampening", 0.0)),
        apply_wd=float(apply.get("weight_decay", 0.0)),
        apply_nesterov=int(bool(apply.get("nesterov", False))),
        apply_first=int(bool(apply.get("first", False))))


def _lrp(lr_tensor):
    """Device fp32 learning rate read by the kernels at run time (None: the ``lr`` argument)."""
    if lr_tensor is None:
        return 0
    if not lr_tensor.is_cuda or lr_tensor.dtype != torch.float32 or lr_tensor.numel() < 1:
        raise ValueError("lr_tensor must be a device fp32 tensor")
    return lr_tensor.data_ptr()


def topk_decode_apply(dp: DevicePlan, recv, layout, levels: int, param=None, mom=None,
                      grad_out=None, lr=0.0, momentum=0.0, dampening=0.0, weight_decay=0.0,
                      grad_scale=1.0, nesterov=False, first=False, shadow=None,
                      key_state=None, key_seed=0, key_rank=0, lr_tensor=None):
    C = require()
    nranks = _recv_rows(recv, layout)
    step = _step(dp, param, mom, grad_out, shadow, lr, momentum, dampening, weight_decay,
                 grad_scale, nesterov, first, key_state, key_seed, key_rank, lr_tensor)
    vk = VK_F32 if layout.kind == "topk" else (VK_Q8 if layout.bits == 8 else VK_Q4)
    C.topk_decode_apply(_args(
        C.TopkDecodeArgs, **_rows(recv, nranks, layout.nbytes), chunks=_ptr(dp.chunks),
        tensors=_ptr(dp.tensors), num_chunks=dp.plan.num_chunks, scales_off=layout.scales,
        counts_off=layout.counts, idx_off=layout.idx, codes_off=layout.codes,
        bitmap_off=layout.bitmap, value_kind=vk, inv_levels=float(1.0 / levels), step=step,
        stream=_stream()))


def qsgd_encode(dp: DevicePlan, grad, payload, layout, levels: int, norm: str, key: int,
                resid=None, key_tensor=None):
    C = require()
    ptrs, mask = grad_pointers(dp, grad)
    _encode_dst(payload, layout)
    if resid is not None:
        _check_bucket(dp, resid, "resid")
    if not (1 <= levels <= (127 if layout.bits == 8 else 7)):
        raise ValueError(f"levels={levels} does not fit {layout.bits}-bit codes")
    C.qsgd_encode(_args(
        C.QsgdEncodeArgs, resid=_ptr(resid), **_tables(dp), scratch=_ptr(dp.scratch),
        payload=_ptr(payload), payload_bytes=layout.nbytes, scales_off=layout.scales,
        codes_off=layout.codes, bits=layout.bits, norm_l2=1 if norm == "l2" else 0,
        levels=float(levels), inv_levels=float(1.0 / levels), key=key & 0xFFFFFFFF,
        bucket_offset=dp.plan.bucket_offset & 0xFFFFFFFF, key_ptr=_keyp(key_tensor),
        stream=_stream()), ptrs, mask)


def qsgd_decode_apply(dp: DevicePlan, recv, layout, levels: int, param=None, mom=None,
                      grad_out=None, lr=0.0, momentum=0.0, dampening=0.0, weight_decay=0.0,
                      grad_scale=1.0, nesterov=False, first=False, shadow=None,
                      key_state=None, key_seed=0, key_rank=0, lr_tensor=None):
    C = require()
    nranks = _recv_rows(recv, layout)
    step = _step(dp, param, mom, grad_out, shadow, lr, momentum, dampening, weight_decay,
                 grad_scale, nesterov, first, key_state, key_seed, key_rank, lr_tensor,
                 need_mom=True)  # k_qsgd_decode_apply reads the buffer whenever it applies
    C.qsgd_decode_apply(_args(
        C.QsgdDecodeArgs, **_rows(recv, nranks, layout.nbytes), chunks=_ptr(dp.chunks),
        tensors=_ptr(dp.tensors), num_chunks=dp.plan.num_chunks, scales_off=layout.scales,
        codes_off=layout.codes, bits=layout.bits, inv_levels=float(1.0 / levels), step=step,
        stream=_stream()))


class SignTables:
    """Device chunk table of a sign-codec plan without the top-k / QSGD scratch of
    :class:`DevicePlan` (the two-stage exchange's per-shard plans)."""

    def __init__(self, plan, device):
        self.plan = plan
        self.chunks = plan.chunk_table(device)


class SignSlots(SignTables):
    """Device tables of one bucket of the two-stage sign exchange (``compress/plan.py
    TwoStagePlan``): the shard-major chunk table and the per-chunk slot table of the ``[N, P]``
    row buffers.  Pass it as both ``dp`` and ``slots`` of the sign wrappers."""

    def __init__(self, ts, device):
        super().__init__(ts.plan, device)
        self.ts = ts
        self.table = ts.slot_table(device)
        self.nbytes = ts.N * ts.P  # bytes of a row buffer
        # the host copy of the table decides whether a buffer holds every slot (the kernels
        # cannot): scales 4-byte, words 16-byte aligned, nothing past slot_end
        if (len(ts.slots) != ts.plan.num_chunks or ts.slot_end > self.nbytes
                or any(a < 0 or a % 4 or w % 16 or a + 4 > self.nbytes
                       or w + 4 * 256 > self.nbytes for a, w in ts.slots)):
            raise ValueError("two-stage slot table does not fit its row buffer")


def _check_slots(dp, slots, buf, name):
    """``buf`` is the ``[N, P]`` row buffer the slot table of ``slots`` addresses."""
    if not isinstance(slots, SignSlots) or slots.plan is not dp.plan:
        raise ValueError("slots must be the SignSlots of the same bucket as dp")
    _check(buf, torch.uint8, name)
    if buf.numel() < slots.nbytes:
        raise ValueError(f"{name} has {buf.numel()} bytes, the slot table addresses "
                         f"{slots.nbytes}")
    return _ptr(slots.table), slots.ts.slot_end


def _check_sign_layout(dp, layout):
    C = dp.plan.num_chunks
    if layout.kind != "sign":
        raise ValueError(f"sign codec given a {layout.kind!r} layout")
    if (layout.scales % 16 or layout.codes % 16 or layout.codes < layout.scales + 4 * C
            or layout.nbytes < layout.codes + 1024 * C):
        raise ValueError("sign layout does not match the bucket plan")


def _sign_payload(dp, payload, layout, slots):
    """Checks of an encode's destination; returns the fields that address it and the bucket."""
    if slots is not None:  # the [N, P] row buffer: every chunk goes to its slot
        sp, end = _check_slots(dp, slots, payload, "payload")
        dst = dict(payload_bytes=payload.numel(), slots=sp, slot_end=end)
    else:
        _check_sign_layout(dp, layout)
        _encode_dst(payload, layout)
        dst = dict(payload_bytes=layout.nbytes, scales_off=layout.scales, bits_off=layout.codes)
    return dict(dst, payload=_ptr(payload), chunks=_ptr(dp.chunks),
                num_chunks=dp.plan.num_chunks, num_tensors=dp.plan.num_tensors)


def _rot(rot_key, slots):
    """The rotate / rot_key fields of the sign wrappers: ``rot_key`` None is the unrotated codec."""
    if rot_key is None:
        return {}
    if slots is not None:
        raise ValueError("the rotated sign codec has no slot-addressed (two-stage) form")
    return dict(rotate=1, rot_key=int(rot_key) & 0xFFFFFFFF)


def sign_encode(dp, grad, payload, layout, resid=None, slots=None, rot_key=None):
    """Scaled sign of one bucket (``csrc/sign_codec.hip``): per chunk the mean ``|e|`` and one bit
    per element, ``e = grad + resid`` with ``resid`` (error feedback) overwritten by what was not
    sent.  One launch, no scratch; bitwise ``compress/oracle.py encode_sign``.  ``slots``
    (:class:`SignSlots`, also ``dp``): ``payload`` is the two-stage exchange's ``[N, P]`` row
    buffer and every chunk is written to its slot (``layout`` unused; pads are not written).
    ``rot_key`` (``oracle.hsign_rot_key``): the Hadamard-rotated form, ``k_hsign_encode``."""
    C = require()
    rot = _rot(rot_key, slots)
    ptrs, mask = grad_pointers(dp, grad)
    dst = _sign_payload(dp, payload, layout, slots)
    if resid is not None:
        _check_bucket(dp, resid, "resid")
    C.sign_encode(_args(C.SignEncodeArgs, resid=_ptr(resid), stream=_stream(), **dst, **rot),
                  ptrs, mask)


def sign_reduce_encode(dp, recv, layout, inv_n, sresid, out):
    """The two-stage exchange's owner step for one shard (``dp``: :class:`SignTables` of the
    shard's plan): ``e = inv_n * sum over the rows of recv (rank order) of +/- scale + sresid``,
    formed in registers and encoded into ``out``; ``sresid`` (shard-relative) is overwritten with
    what was not sent.  ``recv`` is ``[N, P]`` with ``P >= layout.nbytes``; only the scales and
    words of ``out`` are written.  Bitwise ``compress/oracle.py sign_reduce_encode``."""
    C = require()
    _check_sign_layout(dp, layout)
    _check(recv, torch.uint8, "recv")
    if recv.dim() != 2 or recv.shape[0] < 1 or recv.shape[0] > 64:
        raise ValueError("recv must be [nranks, P] with 1 <= nranks <= 64")
    if recv.shape[1] < layout.nbytes or recv.shape[1] % 16:
        raise ValueError(f"recv rows must be 16-byte multiples of at least {layout.nbytes} bytes "
                         "(row stride >= payload)")
    _check(out, torch.uint8, "out")
    if out.numel() < layout.nbytes:
        raise ValueError("out too small")
    if sresid is None:
        raise ValueError("the owner step needs the server residual")
    _check_bucket(dp, sresid, "sresid")
    C.sign_reduce_encode(_args(
        C.SignReduceArgs, **_rows(recv, recv.shape[0], recv.shape[1]), chunks=_ptr(dp.chunks),
        num_chunks=dp.plan.num_chunks, scales_off=layout.scales, bits_off=layout.codes,
        inv_n=float(inv_n), sresid=_ptr(sresid), out=_ptr(out), out_bytes=out.numel(),
        stream=_stream()))


def _sign_recv(dp, recv, layout, slots):
    """Checks of a decode's source; returns the fields that address it and the chunk table."""
    if slots is not None:  # the gathered [N, P] row buffer, read as one slot-addressed payload
        sp, end = _check_slots(dp, slots, recv, "recv")
        src = dict(_rows(recv, 1, recv.numel()), slots=sp, slot_end=end)
    else:
        _check_sign_layout(dp, layout)
        src = dict(_rows(recv, _recv_rows(recv, layout), layout.nbytes),
                   scales_off=layout.scales, bits_off=layout.codes)
    return dict(src, chunks=_ptr(dp.chunks), num_chunks=dp.plan.num_chunks)


def sign_decode_apply(dp, recv, layout, param=None, mom=None, grad_out=None, lr=0.0,
                      momentum=0.0, dampening=0.0, weight_decay=0.0, grad_scale=1.0,
                      nesterov=False, first=False, shadow=None, key_state=None, key_seed=0,
                      key_rank=0, lr_tensor=None, slots=None, rot_key=None):
    """``grad_out = grad_scale * sum over the rows of recv (rank order) of +/- scale`` and / or the
    fused SGD step on ``param`` (``mom`` None: a step without momentum).  ``slots``
    (:class:`SignSlots`, also ``dp``): ``recv`` is the two-stage exchange's gathered ``[N, P]``
    buffer, every chunk read once from its slot (``layout`` unused).  ``rot_key``: the rotated
    form, ``k_hsign_decode_apply`` (the summed rows go through one inverse transform; bitwise
    ``oracle.decode_sum(..., rot_key=rot_key)``)."""
    C = require()
    rot = _rot(rot_key, slots)
    src = _sign_recv(dp, recv, layout, slots)
    step = _step(dp, param, mom, grad_out, shadow, lr, momentum, dampening, weight_decay,
                 grad_scale, nesterov, first, key_state, key_seed, key_rank, lr_tensor)
    C.sign_decode_apply(_args(C.SignDecodeArgs, step=step, stream=_stream(), **src, **rot))


def _check_mx_layout(dp, layout):
    """The layout must be the one the plan gives (the kernels take the packing rule it checks
    for granted); built once per plan and element width."""
    if layout.kind != "mx":
        raise ValueError(f"mx codec given a {layout.kind!r} layout")
    known = dp.__dict__.setdefault("_mx_layouts", {})
    if layout.bits not in known:
        from ..compress.plan import Layout
        known[layout.bits] = Layout.build("mx", dp.plan, layout.bits)
    if layout != known[layout.bits]:
        raise ValueError("mx layout does not match the bucket plan")


def mx_encode(dp, grad, payload, layout, resid=None, soft=False):
    """MXFP8 / MXFP4 of one bucket (``csrc/mx_codec.hip``; ``layout.bits`` 8 or 4): one E8M0 scale
    byte per 32 elements and one FP8 E4M3 / FP4 E2M1 code per element of ``e = grad + resid``, with
    ``resid`` (error feedback) overwritten by what was not sent.  One launch, no scratch; every
    byte of the payload is written; bitwise ``compress/oracle.py encode_mx``.  ``soft``: the
    software conversions instead of the hardware's (the same bytes: a cross-check for tests)."""
    C = require()
    _check_mx_layout(dp, layout)
    ptrs, mask = grad_pointers(dp, grad)
    _encode_dst(payload, layout)
    if resid is not None:
        _check_bucket(dp, resid, "resid")
    C.mx_encode(_args(
        C.MxEncodeArgs, resid=_ptr(resid), chunks=_ptr(dp.chunks), payload=_ptr(payload),
        payload_bytes=layout.nbytes, length=dp.plan.length, num_tensors=dp.plan.num_tensors,
        num_chunks=dp.plan.num_chunks, scales_off=layout.scales, codes_off=layout.codes,
        bits=layout.bits, soft=int(bool(soft)), stream=_stream()), ptrs, mask)


def mx_decode_apply(dp, recv, layout, param=None, mom=None, grad_out=None, lr=0.0,
                    momentum=0.0, dampening=0.0, weight_decay=0.0, grad_scale=1.0,
                    nesterov=False, first=False, shadow=None, key_state=None, key_seed=0,
                    key_rank=0, lr_tensor=None, soft=False):
    """``grad_out = grad_scale * sum over the rows of recv (rank order) of the decoded MX
    payloads`` and / or the fused SGD step on ``param`` (``mom`` None: a step without momentum);
    bitwise ``oracle.decode_sum``.  ``soft``: as in :func:`mx_encode`."""
    C = require()
    _check_mx_layout(dp, layout)
    nranks = _recv_rows(recv, layout)
    step = _step(dp, param, mom, grad_out, shadow, lr, momentum, dampening, weight_decay,
                 grad_scale, nesterov, first, key_state, key_seed, key_rank, lr_tensor)
    C.mx_decode_apply(_args(
        C.MxDecodeArgs, **_rows(recv, nranks, layout.nbytes), length=dp.plan.length,
        chunks=_ptr(dp.chunks), num_chunks=dp.plan.num_chunks, scales_off=layout.scales,
        codes_off=layout.codes, bits=layout.bits, soft=int(bool(soft)), step=step,
        stream=_stream()))


def _check_tern_layout(dp, layout):
    """The layout must be the one the plan gives (the kernels derive every code word's address
    from the plan's tables); built once per plan."""
    if layout.kind != "tern":
        raise ValueError(f"tern codec given a {layout.kind!r} layout")
    known = dp.__dict__.get("_tern_layout")
    if known is None:
        from ..compress.plan import Layout
        known = dp.__dict__["_tern_layout"] = Layout.build("tern", dp.plan)
    if layout != known:
        raise ValueError("tern layout does not match the bucket plan")


def tern_encode(dp: DevicePlan, grad, payload, layout, clip: float, key: int, resid=None,
                key_tensor=None):
    """TernGrad of one bucket (``csrc/tern_codec.hip``): one fp32 scaler per tensor, ``min(max|x|,
    clip * rms(x))`` (``clip == 0``: ``max|x|``), and one stochastic 2-bit code per element of ``x =
    grad + resid``, with ``resid`` (error feedback) overwritten by what was not sent.  ``key``: the
    step's stream key (``key_tensor``: read from device memory instead, for captured graphs).
    Three launches; every byte of the payload is written; bitwise ``compress/oracle.py
    encode_tern``."""
    C = require()
    _check_tern_layout(dp, layout)
    ptrs, mask = grad_pointers(dp, grad)
    _encode_dst(payload, layout)
    if resid is not None:
        _check_bucket(dp, resid, "resid")
    if not float(clip) >= 0.0:
        raise ValueError("tern clip must be >= 0")
    C.tern_encode(_args(
        C.TernEncodeArgs, resid=_ptr(resid), **_tables(dp), scratch=_ptr(dp.scratch),
        payload=_ptr(payload), payload_bytes=layout.nbytes, total_codes=dp.plan.total_codes,
        scales_off=layout.scales, codes_off=layout.codes, clip=float(clip),
        key=key & 0xFFFFFFFF, bucket_offset=dp.plan.bucket_offset & 0xFFFFFFFF,
        key_ptr=_keyp(key_tensor), stream=_stream()), ptrs, mask)


def tern_decode_apply(dp: DevicePlan, recv, layout, param=None, mom=None, grad_out=None, lr=0.0,
                      momentum=0.0, dampening=0.0, weight_decay=0.0, grad_scale=1.0,
                      nesterov=False, first=False, shadow=None, key_state=None, key_seed=0,
                      key_rank=0, lr_tensor=None):
    """``grad_out = grad_scale * sum over the rows of recv (rank order) of code * that row's
    scaler`` and / or the fused SGD step on ``param`` (``mom`` None: a step without momentum);
    bitwise ``oracle.decode_sum``."""
    C = require()
    _check_tern_layout(dp, layout)
    nranks = _recv_rows(recv, layout)
    step = _step(dp, param, mom, grad_out, shadow, lr, momentum, dampening, weight_decay,
                 grad_scale, nesterov, first, key_state, key_seed, key_rank, lr_tensor)
    C.tern_decode_apply(_args(
        C.TernDecodeArgs, **_rows(recv, nranks, layout.nbytes), **_tables(dp),
        total_codes=dp.plan.total_codes, scales_off=layout.scales, codes_off=layout.codes,
        step=step, stream=_stream()))


def _thresh_tables(dp, layout):
    """The fields that address a ``thresh`` payload of ``dp``'s bucket.  The layout must be the
    one the plan gives (the kernels take every slot from the plan's table); layout and device
    table are built once per plan."""
    if layout.kind != "thresh":
        raise ValueError(f"thresh codec given a {layout.kind!r} layout")
    known = dp.__dict__.get("_thresh")
    if known is None:
        from ..compress.plan import Layout
        known = dp.__dict__["_thresh"] = (Layout.build("thresh", dp.plan),
                                          dp.plan.thresh_table(dp.chunks.device),
                                          dp.plan.thresh_slots()[2])
    if layout != known[0]:
        raise ValueError("thresh layout does not match the bucket plan")
    return dict(chunks=_ptr(dp.chunks), num_chunks=dp.plan.num_chunks, slots=_ptr(known[1]),
                total_slots=known[2], counts_off=layout.counts, idx_off=layout.idx,
                codes_off=layout.codes)


def _thresh_ints(t, dp, name):
    """A per-chunk int32 device vector of the thresh encode (None: not passed)."""
    if t is None:
        return 0
    _check(t, torch.int32, name, align=4)
    if t.numel() < dp.plan.num_chunks:
        raise ValueError(f"{name} needs one int32 per chunk row ({dp.plan.num_chunks})")
    return t.data_ptr()


def thresh_encode(dp, grad, payload, layout, resid=None, state=None, passes=None):
    """Threshold sparsification of one bucket (``csrc/thresh_codec.hip``): per chunk row the
    entries of ``acc = grad + resid`` at or above the chunk's canonical bf16-level threshold, in
    index order with their fp32 values, and ``resid`` (error feedback) overwritten with 0 where
    sent and ``acc`` elsewhere.  One launch, no scratch; every byte of the payload is written;
    bitwise ``compress/oracle.py encode_thresh``.  ``state`` (int32 per chunk row): last encode's
    thresholds, where the search starts, rewritten -- a warm start only, the payload does not
    depend on it (None: a cold start).  ``passes`` (int32 per chunk row, probes): receives the
    counting passes every chunk took."""
    C = require()
    tab = _thresh_tables(dp, layout)
    ptrs, mask = grad_pointers(dp, grad)
    _encode_dst(payload, layout)
    if resid is not None:
        _check_bucket(dp, resid, "resid")
    C.thresh_encode(_args(
        C.ThreshEncodeArgs, resid=_ptr(resid), payload=_ptr(payload), payload_bytes=layout.nbytes,
        num_tensors=dp.plan.num_tensors, state=_thresh_ints(state, dp, "state"),
        dbg_passes=_thresh_ints(passes, dp, "passes"), stream=_stream(), **tab), ptrs, mask)


def thresh_decode_apply(dp, recv, layout, param=None, mom=None, grad_out=None, lr=0.0,
                        momentum=0.0, dampening=0.0, weight_decay=0.0, grad_scale=1.0,
                        nesterov=False, first=False, shadow=None, key_state=None, key_seed=0,
                        key_rank=0, lr_tensor=None):
    """``grad_out = grad_scale * sum over the rows of recv (rank order) of the scattered entries``
    and / or the fused SGD step on ``param`` (``mom`` None: a step without momentum); a count
    above the chunk's capacity is cut to it and an index past the chunk's length is dropped;
    bitwise ``oracle.decode_sum``."""
    C = require()
    tab = _thresh_tables(dp, layout)
    nranks = _recv_rows(recv, layout)
    step = _step(dp, param, mom, grad_out, shadow, lr, momentum, dampening, weight_decay,
                 grad_scale, nesterov, first, key_state, key_seed, key_rank, lr_tensor)
    C.thresh_decode_apply(_args(
        C.ThreshDecodeArgs, **_rows(recv, nranks, layout.nbytes), step=step, stream=_stream(),
        **tab))


def thresh_kernel_info() -> dict:
    """Registers, scratch bytes per thread and static LDS bytes of the loaded thresh kernels (the
    runtime's view of the compiler's resource report)."""
    v = require().thresh_kernel_info()
    names = ("k_thr_encode<EF>", "k_thr_encode", "k_thr_decode_apply")
    return {n: {"vgprs": v[3 * i], "scratch_bytes": v[3 * i + 1], "lds_bytes": v[3 * i + 2]}
            for i, n in enumerate(names)}


# IntSGD's scale state of one model (csrc/intsgd_codec.hip IntState): f64 {r, S of the last step}
# | f32 {alpha, inv_a, inv_na} | i32 steps the rule has run
INTSGD_STATE_BYTES = 32


def _check_int_layout(dp, layout):
    """The layout must be the one the plan gives (the kernels take its packing rule for
    granted); built once per plan."""
    if layout.kind != "intsgd":
        raise ValueError(f"intsgd codec given a {layout.kind!r} layout")
    known = dp.__dict__.get("_int_layout")
    if known is None:
        from ..compress.plan import Layout
        known = dp.__dict__["_int_layout"] = Layout.build("intsgd", dp.plan)
    if layout != known:
        raise ValueError("intsgd layout does not match the bucket plan")


def _int_state(state):
    _check(state, torch.uint8, "state", align=8)
    if state.numel() != INTSGD_STATE_BYTES:
        raise ValueError(f"the IntSGD state holds {INTSGD_STATE_BYTES} bytes")
    return _ptr(state)


def _int_rows(dp, t, dtype, name):
    """A per-chunk-row side buffer of one bucket: ``num_chunks`` words."""
    _check(t, dtype, name, align=4)
    if t.numel() != dp.plan.num_chunks:
        raise ValueError(f"{name} holds one entry per chunk row ({dp.plan.num_chunks})")
    return _ptr(t)


def int_encode(dp: DevicePlan, grad, payload, layout, state, sat, q: int, key: int, resid=None,
               key_tensor=None):
    """IntSGD of one bucket (``csrc/intsgd_codec.hip``): one int8 code per element of ``acc = grad
    + resid``, ``round_stochastic(acc * alpha)`` clamped to ``[-q, q]``, with ``alpha`` / ``inv_a``
    read from ``state`` on the device and ``resid`` (error feedback) overwritten by what was not
    sent; ``sat`` (int32 per chunk row) receives the saturated elements' count.  One launch; every
    byte of the payload is written; bitwise ``compress/oracle.py encode_intsgd``."""
    C = require()
    _check_int_layout(dp, layout)
    ptrs, mask = grad_pointers(dp, grad)
    _encode_dst(payload, layout)
    if resid is not None:
        _check_bucket(dp, resid, "resid")
    if not 1 <= int(q) <= 127:
        raise ValueError("q must be in [1, 127]")
    C.int_encode(_args(
        C.IntEncodeArgs, resid=_ptr(resid), chunks=_ptr(dp.chunks), payload=_ptr(payload),
        state=_int_state(state), sat=_int_rows(dp, sat, torch.int32, "sat"),
        payload_bytes=layout.nbytes, length=dp.plan.length, num_tensors=dp.plan.num_tensors,
        num_chunks=dp.plan.num_chunks, q=int(q), key=key & 0xFFFFFFFF,
        bucket_offset=dp.plan.bucket_offset & 0xFFFFFFFF, key_ptr=_keyp(key_tensor),
        stream=_stream()), ptrs, mask)


def int_decode_apply(dp: DevicePlan, summed, layout, state, partials, param, mom=None, lr=0.0,
                     momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first=False,
                     shadow=None, key_state=None, key_seed=0, key_rank=0, lr_tensor=None):
    """The receive side of IntSGD: ``g^ = float(int8 of summed) * inv_na`` (``inv_na`` from
    ``state``), the fused SGD step on ``param`` (``mom`` None: a step without momentum) and, into
    ``partials`` (fp32 per chunk row), the sums of ``(p_new - p_old)^2``; bitwise
    ``oracle.intsgd_apply``."""
    C = require()
    _check_int_layout(dp, layout)
    _check(summed, torch.uint8, "summed")
    if summed.numel() != layout.nbytes:
        raise ValueError(f"the summed payload holds {layout.nbytes} bytes")
    step = _step(dp, param, mom, None, shadow, lr, momentum, dampening, weight_decay, 1.0,
                 nesterov, first, key_state, key_seed, key_rank, lr_tensor)
    C.int_decode_apply(_args(
        C.IntDecodeArgs, recv=_ptr(summed), chunks=_ptr(dp.chunks), state=_int_state(state),
        partials=_int_rows(dp, partials, torch.float32, "partials"), length=dp.plan.length,
        num_chunks=dp.plan.num_chunks, step=step, stream=_stream()))


def int_update_norm(dp: DevicePlan, param, prev, partials):
    """``partials`` (fp32 per chunk row) = the sums of ``(param - prev)^2`` of one bucket, the
    very partials :func:`int_decode_apply` writes; bitwise ``oracle.intsgd_update_partials``."""
    _check_bucket(dp, param, "param")
    _check_bucket(dp, prev, "prev")
    C = require()
    C.int_update_norm(_args(
        C.IntNormArgs, param=_ptr(param), prev=_ptr(prev), chunks=_ptr(dp.chunks),
        partials=_int_rows(dp, partials, torch.float32, "partials"), length=dp.plan.length,
        num_chunks=dp.plan.num_chunks, stream=_stream()))


def int_alpha(partials, state, lr: float, numel: int, world: int, lr_tensor=None):
    """One single-block launch: the model's ``partials`` summed in fp64 in index order, the
    moving average ``r`` and ``alpha``, ``inv_a``, ``inv_na`` into ``state``; ``lr_tensor`` (device
    fp32) overrides ``lr``.  Bitwise ``oracle.intsgd_alpha``."""
    _check(partials, torch.float32, "partials", align=4)
    if not 1 <= int(world) <= 127 or int(numel) < 1:
        raise ValueError("world must be in [1, 127] and numel >= 1")
    C = require()
    C.int_alpha(_args(
        C.IntAlphaArgs, partials=_ptr(partials), state=_int_state(state), lr_ptr=_lrp(lr_tensor),
        total_chunks=partials.numel(), world=int(world), numel=float(numel), lr=float(lr),
        stream=_stream()))


def sign_encode_momentum(dp, grad, payload, layout, resid, exp_avg, beta1,
                         weight_decay=0.0, param=None, slots=None):
    """1-bit Adam's momentum encode: :func:`sign_encode` of ``exp_avg * beta1 + (1 - beta1) * (grad
    + weight_decay * param) + resid``.  ``exp_avg``, ``param`` and the gradients are only read;
    ``resid`` (required) is overwritten.  Bitwise ``compress/oracle.py encode_sign_momentum``.
    ``slots``: as in :func:`sign_encode`."""
    C = require()
    ptrs, mask = grad_pointers(dp, grad)
    dst = _sign_payload(dp, payload, layout, slots)
    if resid is None or exp_avg is None:
        raise ValueError("the momentum encode needs the residual and exp_avg")
    _check_bucket(dp, resid, "resid")
    _check_bucket(dp, exp_avg, "exp_avg")
    if weight_decay != 0.0:
        if param is None:
            raise ValueError("weight decay needs the parameters")
        _check_bucket(dp, param, "param")
    else:
        param = None
    C.sign_encode(_args(
        C.SignEncodeArgs, resid=_ptr(resid), mom_exp_avg=_ptr(exp_avg), mom_param=_ptr(param),
        mom_beta1=float(beta1), mom_wd=float(weight_decay), stream=_stream(), **dst), ptrs, mask)


def sign_decode_onebit(dp, recv, layout, param, exp_avg, exp_avg_sq, inv_n, lr_step,
                       eps, beta1=0.9, beta2=0.999, freeze_step=1, shadow=None, step=None, lr=0.0,
                       lr_tensor=None, key_state=None, key_seed=0, key_rank=0, slots=None):
    """1-bit Adam's fused receive side: ``exp_avg = inv_n * sum over the rows of recv (rank order)
    of +/- scale``, then ``param -= lr_step * exp_avg / (sqrt(exp_avg_sq) + eps)`` where
    ``exp_avg_sq > 0`` (read only).  ``step`` (int32 device tensor, optional): the kernel reads t =
    step + 1 and derives ``lr_step = lr * sqrt(1 - beta2^freeze_step) / (1 - beta1^t)`` on the
    device (``lr_step`` is then ignored).  ``slots``: as in :func:`sign_decode_apply`."""
    C = require()
    src = _sign_recv(dp, recv, layout, slots)
    for t, nm in ((param, "param"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        if t is None:
            raise ValueError(f"the 1-bit Adam step needs {nm}")
        _check_bucket(dp, t, nm)
    if int(freeze_step) < 1:
        raise ValueError("freeze_step must be >= 1")
    if step is not None:
        _check(step, torch.int32, "step", align=4)
    _check_shadow(dp, shadow)
    C.sign_decode_onebit(_args(
        C.SignOnebitArgs, **src, param=_ptr(param), exp_avg=_ptr(exp_avg),
        exp_avg_sq=_ptr(exp_avg_sq), shadow=_ptr(shadow), lr_step=float(lr_step),
        inv_n=float(inv_n), eps=float(eps), beta1=float(beta1), beta2=float(beta2),
        freeze_step=int(freeze_step), step=_ptr(step), lr=float(lr), lr_ptr=_lrp(lr_tensor),
        stream=_stream(), key_state=_keyp(key_state), key_seed=key_seed & 0xFFFFFFFF,
        key_rank=key_rank & 0xFFFFFFFF))


class OnebitLambTables:
    """Per-tensor device state of one bucket for 1-bit LAMB's receive side, in the order of the
    bucket's tensor table: ``adapt`` (int32 [T]), ``r_frozen`` / ``ratio`` (fp32 [T]),
    ``last_factor`` (fp32 [2, T], possibly two column ranges of a wider table: a step reads the row
    of the previous step's parity and writes its own) and ``partials`` (fp32, one per chunk
    row)."""

    def __init__(self, dp, adapt, r_frozen, last_factor, ratio, partials):
        T, C = dp.plan.num_tensors, dp.plan.num_chunks
        _check(adapt, torch.int32, "adapt", align=4)
        for t, nm in ((r_frozen, "r_frozen"), (ratio, "ratio"), (partials, "partials")):
            _check(t, torch.float32, nm, align=4)
        _check(last_factor[0], torch.float32, "last_factor", align=4)
        if (adapt.numel() != T or r_frozen.numel() != T or ratio.numel() != T
                or tuple(last_factor.shape) != (2, T) or last_factor.stride(0) < T
                or partials.numel() != C):
            raise ValueError(f"1-bit LAMB tables of {T} tensors / {C} chunks: adapt, r_frozen and "
                             f"ratio hold {T} entries, last_factor [2, {T}], partials {C}")
        if any(o % 4 for o in dp.plan.offsets):
            raise ValueError("tensor offsets must be multiples of 4 elements (16-byte loads)")
        self.dp = dp
        self.adapt, self.r_frozen, self.last_factor = adapt, r_frozen, last_factor
        self.ratio, self.partials = ratio, partials


def onebit_lamb_step(lt: OnebitLambTables, recv, layout, param, exp_avg, exp_avg_sq,
                     exp_avg_sq_fresh, inv_n, *, lr, betas=(0.9, 0.999), eps=1e-8,
                     weight_decay=0.0, t, freeze_step, factor_min=0.5, factor_max=4.0,
                     factor_threshold=0.1, bc1=None, step=None, lr_tensor=None, shadow=None,
                     key_state=None, key_seed=0, key_rank=0):
    """1-bit LAMB's receive side of one bucket in two launches (``csrc/sign_codec.hip``; bitwise
    ``compress/oracle.py onebit_lamb_apply``): ``k_sign_decode_lamb_stage`` (``exp_avg`` = the
    mean of the decoded momenta, ``exp_avg_sq_fresh``, per-chunk ``max q``) and
    ``k_lamb_onebit_apply`` (per tensor the factor and ``r = r_frozen * f`` -> ``lt.ratio``, the
    new ``lt.last_factor`` row, the step where ``exp_avg_sq > 0``, the bf16 shadow).  ``t`` is the
    1-based step (``> freeze_step``) and ``bc1`` its ``1 - beta1^t``; ``step`` (int32 device
    tensor, optional): the kernels read ``t = step + 1`` and derive ``bc1`` on the device."""
    C = require()
    dp = lt.dp
    src = _sign_recv(dp, recv, layout, None)
    for x, nm in ((param, "param"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"),
                  (exp_avg_sq_fresh, "exp_avg_sq_fresh")):
        if x is None:
            raise ValueError(f"the 1-bit LAMB step needs {nm}")
        _check_bucket(dp, x, nm)
    if int(freeze_step) < 1 or (step is None and int(t) <= int(freeze_step)):
        raise ValueError("the compressed stage starts after freeze_step >= 1")
    if step is not None:
        _check(step, torch.int32, "step", align=4)
    _check_shadow(dp, shadow)
    b1, b2 = betas
    args = _args(
        C.SignLambArgs, **src, tensors=_ptr(dp.tensors), num_tensors=dp.plan.num_tensors,
        param=_ptr(param), exp_avg=_ptr(exp_avg), exp_avg_sq=_ptr(exp_avg_sq),
        exp_avg_sq_fresh=_ptr(exp_avg_sq_fresh), shadow=_ptr(shadow), adapt=_ptr(lt.adapt),
        partials=_ptr(lt.partials), r_frozen=_ptr(lt.r_frozen),
        last_factor=_ptr(lt.last_factor), lf_stride=lt.last_factor.stride(0),
        ratio=_ptr(lt.ratio), lr=float(lr), inv_n=float(inv_n), beta1=float(b1), beta2=float(b2),
        eps=float(eps), weight_decay=float(weight_decay),
        bc1=float(1.0 - b1 ** t if bc1 is None else bc1), bc2w=1.0 - b2 ** int(freeze_step),
        factor_min=float(factor_min), factor_max=float(factor_max),
        factor_threshold=float(factor_threshold), t=int(t), freeze_step=int(freeze_step),
        step=_ptr(step), lr_ptr=_lrp(lr_tensor), stream=_stream(), key_state=_keyp(key_state),
        key_seed=key_seed & 0xFFFFFFFF, key_rank=key_rank & 0xFFFFFFFF)
    C.sign_decode_lamb_stage(args)
    C.lamb_onebit_apply(args)


class LowRankTables:
    """Device tables, slabs and arrival counters of one bucket of PowerSGD (``compress/plan.py
    LowRankPlan``).  The kernels trust the tables, so the host copy is checked here: every
    matrix, dense tensor and work item must lie inside the bucket and the factor buffers."""

    def __init__(self, lrp, device):
        from ..compress.plan import CHUNK, PSGD_COLS

        self.lrp, self.plan = lrp, lrp.plan
        L, r = lrp.plan.length, lrp.rank
        for (off, n, m, po, qo, _), (per, S, so, to) in zip(lrp.mats, lrp.split):
            tiles = -(-m // PSGD_COLS)
            if (off < 0 or n < 1 or m < 1 or off + n * m > L or po < 0 or qo < 0
                    or po + n * r > lrp.p_factor_floats or qo + m * r > lrp.q_floats
                    or per < 1 or S != -(-n // per) or (S > 1 and (
                        so < 0 or so + S * m * r > lrp.slab_floats or to < 0
                        or to + tiles > lrp.num_tickets))):
                raise ValueError("PowerSGD matrix table does not fit its buffers")
        for off, numel, tail, _ in lrp.dense:
            if (off < 0 or numel < 1 or off + numel > L or tail < lrp.p_factor_floats
                    or tail + numel > lrp.p_floats):
                raise ValueError("PowerSGD dense table does not fit its buffers")
        for items, tiled in ((lrp.row_items, False), (lrp.tile_items, True)):
            for kind, i, a, b in items:
                if kind == 1:
                    good = (0 <= i < len(lrp.dense) and 0 <= a and 1 <= b <= CHUNK
                            and a + b <= lrp.dense[i][1])
                elif tiled:
                    good = (0 <= i < len(lrp.mats) and 0 <= a < -(-lrp.mats[i][2] // PSGD_COLS)
                            and 0 <= b < lrp.split[i][1])
                else:
                    good = 0 <= i < len(lrp.mats) and 0 <= a and b >= 1 and \
                        a + b <= lrp.mats[i][1]
                if not good:
                    raise ValueError("PowerSGD work list does not fit its plan")
        if [it[0] for it in lrp.tile_items[:lrp.num_mat_tiles]].count(0) != lrp.num_mat_tiles:
            raise ValueError("PowerSGD tile list: the matrix items come first")
        self.mats = lrp.mat_table(device)
        self.dense = lrp.dense_table(device)
        self.rows = lrp.row_table(device)
        self.tiles = lrp.tile_table(device)
        self.slabs = torch.zeros(max(4, lrp.slab_floats), dtype=torch.float32, device=device)
        # zero at allocation; every back-project launch leaves them zeroed
        self.tickets = torch.zeros(max(1, lrp.num_tickets), dtype=torch.int32, device=device)


def _psgd_buf(t, n, name):
    _check(t, torch.float32, name)
    if t.numel() < n:
        raise ValueError(f"{name} has {t.numel()} floats, the plan needs {n}")


def _psgd(launch, lt, items, num_items, grad=None, resid=None, p=None, q=None, inv_n=1.0,
          q_out=None, step=None):
    """Launch ``psgd_<launch>`` of the extension."""
    C = require()
    lrp = lt.lrp
    _psgd_buf(p, lrp.p_floats, "p")
    for t, nm in ((grad, "grad"), (resid, "resid")):
        if t is not None:
            _check_bucket(lt, t, nm)
    for t, nm in ((q, "q"), (q_out, "q_out")):
        if t is not None:
            _psgd_buf(t, lrp.q_floats, nm)
    getattr(C, "psgd_" + launch)(_args(
        C.PsgdArgs, rank=lrp.rank, mats=_ptr(lt.mats), num_mats=len(lrp.mats),
        dense=_ptr(lt.dense), num_dense=len(lrp.dense), items=_ptr(items), num_items=num_items,
        bucket_len=lrp.plan.length, p_floats=lrp.p_floats, q_floats=lrp.q_floats,
        grad=_ptr(grad), resid=_ptr(resid), p=_ptr(p), q=_ptr(q), slabs=_ptr(lt.slabs),
        slab_floats=lrp.slab_floats, tickets=_ptr(lt.tickets), num_tickets=lrp.num_tickets,
        inv_n=float(inv_n), q_out=_ptr(q_out), step=C.StepArgs() if step is None else step,
        stream=_stream()))


def psgd_project(lt: LowRankTables, grad, resid, q, p):
    """PowerSGD launch 1 (``csrc/powersgd.hip``): ``resid <- M = grad + resid`` on the compressed
    tensors, ``p`` = the ``M Q`` factors followed by the dense tensors' gradients.  ``grad`` and
    ``resid`` are the bucket's flat views."""
    if grad is None or resid is None or q is None:
        raise ValueError("the project launch needs grad, resid and q")
    _psgd("project", lt, lt.rows, len(lt.lrp.row_items), grad=grad, resid=resid, p=p, q=q)


def psgd_orth(lt: LowRankTables, p, inv_n: float):
    """PowerSGD launch 2: every P block times ``inv_n``, then modified Gram-Schmidt."""
    _psgd("orth", lt, None, 0, p=p, inv_n=inv_n)


def psgd_backproject(lt: LowRankTables, resid, p, q):
    """PowerSGD launch 3: ``q`` = the ``M^T P`` factors (``resid`` holds M)."""
    if resid is None or q is None:
        raise ValueError("the back-project launch needs resid and q")
    _psgd("backproject", lt, lt.tiles, lt.lrp.num_mat_tiles, resid=resid, p=p, q=q)


def psgd_decode_apply(lt: LowRankTables, resid, p, q, q_out, inv_n, param=None, mom=None,
                      grad_out=None, lr=0.0, momentum=0.0, dampening=0.0, weight_decay=0.0,
                      nesterov=False, first=False, shadow=None, lr_tensor=None):
    """PowerSGD launch 4: ``q_out = q * inv_n``, ``g^ = P q_out^T`` (dense tensors: ``p``'s tail
    times ``inv_n``), ``resid <- M - g^`` and the fused SGD step on ``param`` with ``g^``
    (``param`` None: write ``g^`` to ``grad_out`` only).  Bitwise ``compress/oracle.py
    powersgd_reconstruct_apply``."""
    if resid is None or q is None or q_out is None:
        raise ValueError("the reconstruct launch needs resid, q and q_out")
    if q.data_ptr() == q_out.data_ptr():
        raise ValueError("q_out must not be q: other blocks still read q")
    step = _step(lt, param, mom, grad_out, shadow, lr, momentum, dampening, weight_decay, 1.0,
                 nesterov, first, None, 0, 0, lr_tensor)
    _psgd("decode_apply", lt, lt.tiles, len(lt.lrp.tile_items), resid=resid, p=p, q=q,
          inv_n=inv_n, q_out=q_out, step=step)


# Count sketch (csrc/sketch_codec.hip): a table entry sums its chunks in groups of this many
# consecutive chunk indices, sequentially within a group and then over the groups (SK_GROUP;
# compress/plan.py SKETCH_SUM_GROUP and compress/oracle.py sketch_accumulate mirror it)
SKETCH_SUM_GROUP = 64


class SketchTables:
    """Device tables of one bucket of the count-sketch exchange (``compress/plan.py
    SketchPlan``), checked once against the buffers the kernels index with them."""

    def __init__(self, sp, device):
        from ..compress.plan import SKETCH_SUM_GROUP as plan_group

        if not (require().sketch_sum_group() == SKETCH_SUM_GROUP == plan_group):
            raise RuntimeError("the sketch summation group of the kernel, ops and the plan differ")
        self.sp, self.plan = sp, sp.plan
        L, C = sp.plan.length, sp.plan.num_chunks
        if len(sp.chunk_rows) != C or len(sp.shifts) != sp.rows:
            raise ValueError("sketch tables do not fit their plan")
        for start, ln in sp.chunk_rows:
            if not (0 <= ln <= 8192 and 0 <= start and start + ln <= L and start % 4 == 0):
                raise ValueError("sketch chunk row outside the bucket, or not at a multiple of 4 "
                                 "elements")
        for row in sp.shifts:
            if len(row) != C or not all(0 <= o < sp.W for o in row):
                raise ValueError("sketch shift outside the table")
        self.rows = sp.row_table(device)
        self.shifts = sp.shift_table(device)

    def args(self, **fields):
        sp = self.sp
        return _args(require().SketchArgs, rows=_ptr(self.rows), shifts=_ptr(self.shifts),
                     stream=_stream(), num_chunks=sp.plan.num_chunks, sketch_rows=sp.rows,
                     width=sp.W, bucket_len=sp.plan.length, sg_key=sp.sg_key,
                     bucket_offset=sp.plan.bucket_offset & 0xFFFFFFFF, **fields)


def _sketch_table(st: SketchTables, table):
    _check(table, torch.float32, "table")
    if table.numel() < st.sp.table_floats:
        raise ValueError(f"table has {table.numel()} floats, the sketch needs "
                         f"{st.sp.table_floats}")


def sketch_stage(st: SketchTables, grad, resid):
    """Sketch launch 1: ``resid <- grad + resid`` on the sketched tensors of the bucket."""
    _check_bucket(st, grad)
    _check_bucket(st, resid, "resid")
    require().sketch_stage(st.args(grad=_ptr(grad), resid=_ptr(resid)))


def sketch_accum(st: SketchTables, resid, table):
    """Sketch launch 2: ``table`` = the ``[R, W]`` count sketch of the staged ``resid``, bitwise
    ``compress/oracle.py sketch_accumulate`` and the same from run to run."""
    _check_bucket(st, resid, "resid")
    _sketch_table(st, table)
    require().sketch_accum(st.args(resid=_ptr(resid), table=_ptr(table)))


def sketch_estimate(st: SketchTables, table, est):
    """Sketch launch 3: ``est`` = per element the median of its rows' signed table entries
    (dense tensors and pads are not written: they keep the buffer's zeros)."""
    _sketch_table(st, table)
    _check_bucket(st, est, "est")
    require().sketch_estimate(st.args(table=_ptr(table), est=_ptr(est)))


def sketch_gather(st: SketchTables, dp: DevicePlan, payload, layout, grad, resid):
    """Sketch launch 4 (after ``topk_encode`` of the estimate into ``payload``): the payload's
    values <- ``resid`` at the selected coordinates (``grad`` on dense tensors), ``resid`` cleared
    there."""
    if layout.kind != "topk" or dp.plan is not st.plan:
        raise ValueError("the sketch gathers through its own plan's plain top-k payload")
    _encode_dst(payload, layout)
    _check_bucket(st, grad)
    _check_bucket(st, resid, "resid")
    p = st.plan
    require().sketch_gather(st.args(
        grad=_ptr(grad), resid=_ptr(resid), payload=_ptr(payload), payload_bytes=layout.nbytes,
        total_k=p.total_k, total_idx=p.total_idx, total_bm_words=p.total_bm_words,
        counts_off=layout.counts, idx_off=layout.idx, codes_off=layout.codes,
        bitmap_off=layout.bitmap, chunks=_ptr(dp.chunks), tensors=_ptr(dp.tensors),
        num_tensors=p.num_tensors))


_GDT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def sgd_flat(param, mom, grad, lr, momentum=0.0, dampening=0.0, weight_decay=0.0,
             grad_scale=1.0, nesterov=False, first=False, shadow=None, lr_tensor=None):
    C = require()
    _check(param, torch.float32, "param")
    _check(mom, torch.float32, "mom")
    if grad.dtype not in _GDT:
        raise TypeError(f"unsupported grad dtype {grad.dtype}")
    _check(grad, grad.dtype, "grad", align=8)
    n = param.numel()
    if mom.numel() != n or grad.numel() != n or n % 4:
        raise ValueError("param/mom/grad must have equal numel, a multiple of 4")
    if shadow is not None:
        _check(shadow, torch.bfloat16, "shadow", align=8)
        if shadow.numel() != n:
            raise ValueError("shadow must match param")
    C.sgd_flat(_args(
        C.SgdFlatArgs, param=_ptr(param), mom=_ptr(mom), grad=_ptr(grad), shadow=_ptr(shadow),
        n=n, grad_dtype=_GDT[grad.dtype], lr=lr, momentum=momentum, dampening=dampening,
        weight_decay=weight_decay, grad_scale=grad_scale, nesterov=int(nesterov),
        first=int(first), stream=_stream(), lr_ptr=_lrp(lr_tensor)))


def _adam_args(C, **fields):
    """``AdamFlatArgs`` of :func:`adam_flat`: ``lr_step`` carries both bias corrections, so
    ``bc2_sqrt`` is always 1."""
    return _args(C.AdamFlatArgs, bc2_sqrt=1.0, **fields)


def adam_flat(param, exp_avg, exp_avg_sq, max_exp_avg_sq, grad, lr_step, beta1, beta2, eps,
              weight_decay=0.0, grad_scale=1.0, amsgrad=False, shadow=None, step=None, lr=0.0,
              lr_tensor=None):
    """Adam/AMSGrad over flat fp32 buffers.  ``step`` (int32 device tensor, optional): the kernel
    reads t = step + 1 and derives ``lr_step = lr * sqrt(1 - beta2^t) / (1 - beta1^t)`` on the
    device, so a captured graph follows the step count (``lr_step`` is then ignored)."""
    C = require()
    if step is not None:
        _check(step, torch.int32, "step", align=4)
    for t, nm in ((param, "param"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _check(t, torch.float32, nm)
    if amsgrad:
        if max_exp_avg_sq is None:
            raise ValueError("amsgrad needs max_exp_avg_sq")
        _check(max_exp_avg_sq, torch.float32, "max_exp_avg_sq")
    if grad.dtype not in _GDT:
        raise TypeError(f"unsupported grad dtype {grad.dtype}")
    _check(grad, grad.dtype, "grad", align=8)
    n = param.numel()
    if n % 4 or grad.numel() != n or exp_avg.numel() != n or exp_avg_sq.numel() != n:
        raise ValueError("flat buffers must have equal numel, a multiple of 4")
    if amsgrad and max_exp_avg_sq.numel() != n:
        raise ValueError("max_exp_avg_sq must match param")
    if shadow is not None:
        _check(shadow, torch.bfloat16, "shadow", align=8)
        if shadow.numel() != n:
            raise ValueError("shadow must match param")
    C.adam_flat(_adam_args(
        C, param=_ptr(param), exp_avg=_ptr(exp_avg), exp_avg_sq=_ptr(exp_avg_sq),
        max_exp_avg_sq=_ptr(max_exp_avg_sq), grad=_ptr(grad), shadow=_ptr(shadow), n=n,
        grad_dtype=_GDT[grad.dtype], lr_step=lr_step, beta1=beta1, beta2=beta2, eps=eps,
        weight_decay=weight_decay, grad_scale=grad_scale, amsgrad=int(amsgrad),
        stream=_stream(), step=_ptr(step), lr=float(lr), lr_ptr=_lrp(lr_tensor)))


def lion_flat(param, exp_avg, grad, lr, beta1, beta2, weight_decay=0.0, grad_scale=1.0,
              shadow=None, lr_tensor=None):
    """Lion over flat fp32 buffers (``csrc/lion.hip``; bitwise ``compress/oracle.py lion_apply``
    on ``grad * grad_scale``): any ``numel`` (16-byte accesses, scalar tail)."""
    C = require()
    _check(param, torch.float32, "param")
    _check(exp_avg, torch.float32, "exp_avg")
    if grad.dtype not in _GDT:
        raise TypeError(f"unsupported grad dtype {grad.dtype}")
    _check(grad, grad.dtype, "grad", align=16 if grad.dtype == torch.float32 else 8)
    n = param.numel()
    if n < 1 or grad.numel() != n or exp_avg.numel() != n:
        raise ValueError("flat buffers must have equal, non-zero numel")
    if shadow is not None:
        _check(shadow, torch.bfloat16, "shadow", align=8)
        if shadow.numel() != n:
            raise ValueError("shadow must match param")
    C.lion_flat(_args(
        C.LionFlatArgs, param=_ptr(param), exp_avg=_ptr(exp_avg), grad=_ptr(grad),
        shadow=_ptr(shadow), n=n, grad_dtype=_GDT[grad.dtype], lr=float(lr), beta1=float(beta1),
        beta2=float(beta2), weight_decay=float(weight_decay), grad_scale=float(grad_scale),
        stream=_stream(), lr_ptr=_lrp(lr_tensor)))


OUTER_ROW = 8192  # elements per block of k_outer_apply, and per row of its outer_stats


def outer_rows(n: int) -> int:
    """Rows of ``outer_stats`` (fp32 ``[rows, 2]``) for a flat range of ``n`` elements."""
    return (int(n) + OUTER_ROW - 1) // OUTER_ROW


def outer_apply(anchor, data, momentum, delta, lr, mu, nesterov, shadow=None, stats=None):
    """Local SGD's outer step over flat fp32 buffers in one launch (``csrc/outer.hip``; bitwise
    ``compress/oracle.py outer_apply``): ``momentum = momentum * mu + delta``, ``anchor += lr *
    (delta + momentum * mu if nesterov else momentum)``, ``data = anchor`` (and its bf16
    ``shadow``).  Any ``numel`` (16-byte accesses, scalar tail).  ``stats`` (fp32 ``[outer_rows(n),
    2]``): per row of 8192 elements the sums of squares of ``delta`` and of the new ``momentum``,
    through ``k_clip_norm``'s tree (``CLIP_SUM_CHAIN``)."""
    C = require()
    _check(anchor, torch.float32, "anchor")
    _check(data, torch.float32, "data")
    _check(momentum, torch.float32, "momentum")
    _check(delta, torch.float32, "delta")
    n = anchor.numel()
    if n < 1 or data.numel() != n or momentum.numel() != n or delta.numel() != n:
        raise ValueError("flat buffers must have equal, non-zero numel")
    if len({t.data_ptr() for t in (anchor, data, momentum, delta)}) != 4:
        raise ValueError("anchor, data, momentum and delta must be four buffers")
    if shadow is not None:
        _check(shadow, torch.bfloat16, "shadow", align=8)
        if shadow.numel() != n:
            raise ValueError("shadow must match anchor")
    rows = 0
    if stats is not None:
        _check(stats, torch.float32, "stats", align=4)
        rows = outer_rows(n)
        if stats.dim() != 2 or tuple(stats.shape) != (rows, 2):
            raise ValueError(f"stats must be fp32 [{rows}, 2], one row per {OUTER_ROW} elements")
    lr, mu = float(lr), float(mu)
    if not (0.0 < lr < float("inf")):
        raise ValueError("outer lr must be finite and > 0")
    if not 0.0 <= mu < 1.0:
        raise ValueError("outer momentum must be in [0, 1)")
    C.outer_apply(_args(
        C.OuterArgs, anchor=_ptr(anchor), data=_ptr(data), momentum=_ptr(momentum),
        delta=_ptr(delta), shadow=_ptr(shadow), stats=_ptr(stats), n=n, stats_rows=rows, lr=lr,
        mu=mu, nesterov=int(bool(nesterov)), stream=_stream()))


def _check_vote_layout(dp, layout):
    if layout.kind != "vote":
        raise ValueError(f"vote codec given a {layout.kind!r} layout")
    if layout.codes % 16 or layout.nbytes < layout.codes + 1024 * dp.plan.num_chunks:
        raise ValueError("vote layout does not match the bucket plan")


def _check_vote_slots(dp, slots, buf, name):
    """As :func:`_check_slots`, for the slot table of a ``TwoStagePlan`` of kind ``vote``."""
    if getattr(getattr(slots, "ts", None), "kind", None) != "vote":
        raise ValueError("the vote kernels take the slot table of a vote two-stage plan")
    return _check_slots(dp, slots, buf, name)


def lion_encode(dp, grad, payload, layout, exp_avg, beta1, beta2, step, rank, step_tensor=None,
                slots=None):
    """Distributed Lion's vote of one bucket (``csrc/lion.hip``): one bit per element, the sign of
    ``exp_avg * beta1 + (1 - beta1) * grad`` (an exact zero votes by the parity of index + step +
    rank), then ``exp_avg = exp_avg * beta2 + (1 - beta2) * grad``.  ``step``: the 1-based step,
    read as ``step_tensor + 1`` (int32 device counter) when given.  One launch; bitwise
    ``compress/oracle.py encode_vote``.  ``slots`` (:class:`SignSlots` of a vote two-stage plan,
    also ``dp``): ``payload`` is the two-stage vote's ``[N, P]`` row buffer and every chunk's
    words are written to its slot (``layout`` unused; nothing else is written)."""
    C = require()
    ptrs, mask = grad_pointers(dp, grad)
    if slots is not None:
        sp, end = _check_vote_slots(dp, slots, payload, "payload")
        nbytes, codes = payload.numel(), 0
    else:
        _check_vote_layout(dp, layout)
        _encode_dst(payload, layout)
        nbytes, codes, sp, end = layout.nbytes, layout.codes, 0, 0
    _check_bucket(dp, exp_avg, "exp_avg")
    if step_tensor is not None:
        _check(step_tensor, torch.int32, "step", align=4)
    C.lion_encode(_args(
        C.LionEncodeArgs, exp_avg=_ptr(exp_avg), chunks=_ptr(dp.chunks), payload=_ptr(payload),
        payload_bytes=nbytes, num_tensors=dp.plan.num_tensors, num_chunks=dp.plan.num_chunks,
        bits_off=codes, beta1=float(beta1), beta2=float(beta2), step=int(step),
        step_ptr=_ptr(step_tensor), rank=int(rank), stream=_stream(), slots=sp, slot_end=end),
        ptrs, mask)


def vote_reduce(dp, recv, layout, owner_row, out):
    """The two-stage vote's owner step for one shard (``dp``: :class:`SignTables` of the shard's
    plan, ``layout`` its vote layout): per element ``s = N - 2 * (set bits over the rows of
    recv)``; the bit written to ``out`` is ``(s < 0) | (s == 0 & the bit of row owner_row)``.
    ``recv`` is ``[N, P]`` with ``P >= layout.nbytes``; only the words of ``out`` are written and
    no parameter is touched.  Bitwise ``compress/oracle.py vote_reduce``."""
    C = require()
    _check_vote_layout(dp, layout)
    _check(recv, torch.uint8, "recv")
    if recv.dim() != 2 or not 1 <= recv.shape[0] <= 1 << 20:
        raise ValueError("recv must be [nranks, P]")
    if recv.shape[1] < layout.nbytes or recv.shape[1] % 16:
        raise ValueError(f"recv rows must be 16-byte multiples of at least {layout.nbytes} bytes "
                         "(row stride >= payload)")
    if not 0 <= int(owner_row) < recv.shape[0]:
        raise ValueError(f"owner row {owner_row} is not one of the {recv.shape[0]} received rows")
    _check(out, torch.uint8, "out")
    if out.numel() < layout.nbytes:
        raise ValueError("out too small")
    C.vote_reduce(_args(
        C.VoteReduceArgs, **_rows(recv, recv.shape[0], recv.shape[1]), owner=int(owner_row),
        num_chunks=dp.plan.num_chunks, bits_off=layout.codes, out=_ptr(out),
        out_bytes=out.numel(), stream=_stream()))


def lion_vote_apply(dp, recv, layout, param, lr, weight_decay=0.0, aggregate="majority",
                    inv_n=None, shadow=None, lr_tensor=None, key_state=None, key_seed=0,
                    key_rank=0, slots=None):
    """The receive side of the vote: per element ``s = N - 2 * (set bits over the rows of recv)``,
    ``d = sign(s)`` (``majority``) or ``s * inv_n`` (``average``; ``inv_n`` defaults to 1 / N),
    ``param -= lr * (d + weight_decay * param)``.  Bitwise ``compress/oracle.py vote_apply``.
    ``slots`` (:class:`SignSlots` of a vote two-stage plan, also ``dp``): ``recv`` is the
    two-stage vote's gathered ``[N, P]`` buffer, every chunk's words read once from its slot and
    ``d = 1 - 2 * bit`` (``layout`` unused; ``majority`` only)."""
    C = require()
    if aggregate not in ("majority", "average"):
        raise ValueError("aggregate must be 'majority' or 'average'")
    if slots is not None:
        if aggregate != "majority":
            raise ValueError("the slot-addressed apply takes each bit as the direction: majority")
        sp, end = _check_vote_slots(dp, slots, recv, "recv")
        n, stride, codes = 1, recv.numel(), 0
    else:
        _check_vote_layout(dp, layout)
        _check(recv, torch.uint8, "recv")
        if recv.dim() != 2 or recv.shape[1] != layout.nbytes or not 1 <= recv.shape[0] <= 1 << 20:
            raise ValueError(f"recv must be [nranks, {layout.nbytes}]")
        n, stride, codes, sp, end = recv.shape[0], layout.nbytes, layout.codes, 0, 0
    _check_bucket(dp, param, "param")
    _check_shadow(dp, shadow)
    C.lion_vote_apply(_args(
        C.LionVoteArgs, **_rows(recv, n, stride), chunks=_ptr(dp.chunks),
        num_chunks=dp.plan.num_chunks, bits_off=codes, param=_ptr(param), shadow=_ptr(shadow),
        lr=float(lr), weight_decay=float(weight_decay),
        inv_n=float(1.0 / n if inv_n is None else inv_n), average=int(aggregate == "average"),
        lr_ptr=_lrp(lr_tensor), stream=_stream(), key_state=_keyp(key_state),
        key_seed=key_seed & 0xFFFFFFFF, key_rank=key_rank & 0xFFFFFFFF, slots=sp, slot_end=end))


# Longest chain of fp32 additions behind one chunk's sum of squares in k_lw_stage
# (csrc/layerwise.hip): 32 serial terms per thread + 6 shuffle levels + 3 across the waves.  The
# per-tensor sums over the chunks are fp64.
LAYERWISE_SUM_CHAIN = 41
LAYERWISE_KINDS = {"lars": 0, "lamb": 1}


class LayerwisePlan:
    """Device tables of one flat range (a bucket or the whole model) for the layer-wise
    optimizers: the range's ``BucketPlan`` tables and its views of the optimizer's per-tensor
    ``adapt`` flags (int32), ``ratio`` output (fp32) and per-chunk ``partials`` (fp32 [C, 2])."""

    def __init__(self, plan, adapt, ratio, partials):
        T, C = plan.num_tensors, plan.num_chunks
        _check(adapt, torch.int32, "adapt", align=4)
        _check(ratio, torch.float32, "ratio", align=4)
        _check(partials, torch.float32, "partials", align=4)
        if adapt.numel() != T or ratio.numel() != T or partials.numel() != 2 * C:
            raise ValueError(f"layer-wise plan of {T} tensors / {C} chunks: adapt, ratio must "
                             f"hold {T} entries and partials {2 * C}")
        if any(o % 4 for o in plan.offsets):
            raise ValueError("tensor offsets must be multiples of 4 elements (16-byte loads)")
        if max(o + n for o, n in zip(plan.offsets, plan.numels)) > plan.length:
            raise ValueError("a tensor reaches past the range")
        if plan.length >= 1 << 31:
            raise ValueError("flat range of 2^31 elements or more")
        self.plan = plan
        self.adapt, self.ratio, self.partials = adapt, ratio, partials
        self.tensors = plan.tensor_table(adapt.device)
        self.chunks = plan.chunk_table(adapt.device)


def _layerwise_args(C, betas, t, **fields):
    """``LayerwiseArgs`` with the betas of step ``t`` (1-based): in double (``beta1d`` /
    ``beta2d``), rounded to fp32 as C's ``(float)`` does (``beta1`` / ``beta2``: the float field
    takes the same double), and LAMB's bias corrections ``bc1`` / ``bc2``."""
    b1, b2 = betas
    return _args(C.LayerwiseArgs, beta1=float(b1), beta2=float(b2), beta1d=float(b1),
                 beta2d=float(b2), bc1=1.0 - b1 ** t, bc2=1.0 - b2 ** t, **fields)


def layerwise_step(lw: LayerwisePlan, kind: str, param, grad, state1, state2=None, *, lr,
                   weight_decay=0.0, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8, eta=0.001,
                   momentum=0.0, dampening=0.0, nesterov=False, first=False, t=1, step=None,
                   lr_tensor=None, shadow=None):
    """One LARS (``state1`` = momentum buffer) or LAMB (``state1`` / ``state2`` = ``exp_avg`` /
    ``exp_avg_sq``) step of the flat range ``lw`` describes, in two launches: ``k_lw_stage``
    (per-chunk sums of squares; LAMB's moments) and ``k_lw_apply`` (trust ratios -> ``lw.ratio``,
    the step, the bf16 shadow).  ``step`` (int32 device tensor, optional): the kernels read the
    0-based step count from it (``t = step + 1``) instead of the host's ``t`` / ``first``."""
    C = require()
    if kind not in LAYERWISE_KINDS:
        raise ValueError(f"unknown layer-wise rule {kind!r}")
    n = lw.plan.length
    if grad.dtype not in _GDT:
        raise TypeError(f"unsupported grad dtype {grad.dtype}")
    _check(param, torch.float32, "param")
    _check(grad, grad.dtype, "grad", align=16 if grad.dtype == torch.float32 else 8)
    states = [(state1, "exp_avg"), (state2, "exp_avg_sq")] if kind == "lamb" else \
        [(state1, "mom")]
    for s, nm in states:
        if s is None:
            raise ValueError(f"the {kind} step needs {nm}")
        _check(s, torch.float32, nm)
    for s, nm in [(param, "param"), (grad, "grad")] + states:
        if s.numel() < n:
            raise ValueError(f"{nm} has {s.numel()} elements, the range needs {n}")
    _check_shadow(lw, shadow)
    if step is not None:
        _check(step, torch.int32, "step", align=4)
    args = _layerwise_args(
        C, betas, t, kind=LAYERWISE_KINDS[kind], param=_ptr(param), grad=_ptr(grad),
        grad_dtype=_GDT[grad.dtype], state1=_ptr(state1),
        state2=_ptr(state2) if kind == "lamb" else 0, shadow=_ptr(shadow),
        chunks=_ptr(lw.chunks), num_chunks=lw.plan.num_chunks, tensors=_ptr(lw.tensors),
        adapt=_ptr(lw.adapt), partials=_ptr(lw.partials), ratio=_ptr(lw.ratio), lr=float(lr),
        eps=float(eps), weight_decay=float(weight_decay), grad_scale=float(grad_scale),
        eta=float(eta), momentum=float(momentum), dampening=float(dampening),
        nesterov=int(bool(nesterov)), first=int(bool(first)), step=_ptr(step),
        lr_ptr=_lrp(lr_tensor), stream=_stream())
    C.layerwise_stage(args)
    C.layerwise_apply(args)


# Longest chain of fp32 additions behind one chunk's sum of squares in k_clip_norm
# (csrc/clip.hip), k_lw_stage's tree: 32 serial terms per thread + 6 shuffle levels + 3 across
# the waves.  The model-wide sum over the chunks is fp64.
CLIP_SUM_CHAIN = 41


class _ClipBucket:
    """One bucket's plan, device chunk table and first row in the model-wide partials."""

    def __init__(self, plan, device, chunk0):
        self.plan, self.chunk0 = plan, chunk0
        self.chunks = plan.chunk_table(device)


class ClipPlan:
    """Device state of the global-norm gradient clip over a whole model: per bucket (``plans``,
    the model's ``BucketPlan`` s in bucket order) the chunk table, and model-wide the per-chunk
    ``partials`` (fp32, one per chunk row in bucket order, then chunk order) and
    ``state`` = fp32 ``{norm, coef}``, rewritten by every step."""

    def __init__(self, plans, device):
        require()
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("ClipPlan holds device tables: it needs a GPU device")
        if not plans:
            raise ValueError("ClipPlan needs at least one bucket")
        self.buckets, n = [], 0
        for plan in plans:
            if plan.num_tensors > MAX_TENSORS_PER_BUCKET:
                raise ValueError(f"bucket has {plan.num_tensors} tensors (max "
                                 f"{MAX_TENSORS_PER_BUCKET})")
            if any(o % 4 for o in plan.offsets):
                raise ValueError("tensor offsets must be multiples of 4 elements (16-byte loads)")
            if max(o + k for o, k in zip(plan.offsets, plan.numels)) > plan.length:
                raise ValueError("a tensor reaches past its bucket")
            if plan.length >= 1 << 31:
                raise ValueError("bucket of 2^31 elements or more")
            self.buckets.append(_ClipBucket(plan, device, n))
            n += plan.num_chunks
        self.total_chunks = n
        self.partials = torch.zeros(n, dtype=torch.float32, device=device)
        self.state = torch.zeros(2, dtype=torch.float32, device=device)


def _clip_args(cp, bi, grads, max_norm):
    if not isinstance(cp, ClipPlan):
        raise TypeError("expected an ops.ClipPlan")
    if not 0 <= bi < len(cp.buckets):
        raise ValueError(f"bucket {bi} of a clip plan of {len(cp.buckets)}")
    b = cp.buckets[bi]
    ptrs, mask = grad_pointers(b, grads)
    dev = cp.partials.device
    for t in ([grads] if torch.is_tensor(grads) else grads):
        if t.device != dev:
            raise ValueError("gradients and clip plan live on different devices")
    return _args(
        require().ClipArgs, num_tensors=b.plan.num_tensors, chunks=_ptr(b.chunks),
        num_chunks=b.plan.num_chunks, partials=_ptr(cp.partials), chunk0=b.chunk0,
        total_chunks=cp.total_chunks, state=_ptr(cp.state), max_norm=float(max_norm),
        stream=_stream()), ptrs, mask


def clip_norm(cp: ClipPlan, bi: int, grads):
    """Launch ``k_clip_norm`` for bucket ``bi``: the per-chunk sums of squares of its gradients
    (``grads`` as for :func:`pack_grads`: the bucket's flat fp32 view, or one fp32 / bf16 tensor per
    plan tensor) into ``cp.partials``.  Every bucket's norm launch precedes any
    :func:`clip_scale`."""
    require().clip_norm(*_clip_args(cp, bi, grads, 1.0))


def clip_scale(cp: ClipPlan, bi: int, grads, max_norm: float):
    """Launch ``k_clip_scale`` for bucket ``bi``: ``coef = min(1, max_norm / (norm + 1e-6))`` from
    all of ``cp.partials``, the bucket's gradients scaled in place unless ``coef == 1``; bucket 0
    stores ``cp.state = {norm, coef}``."""
    max_norm = float(max_norm)
    if not max_norm > 0.0 or max_norm != max_norm:
        raise ValueError("max_norm must be > 0")
    require().clip_scale(*_clip_args(cp, bi, grads, max_norm))


_DDT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def pack_grads(dp, grads, dst, scale=1.0):
    """Gather the bucket's per-tensor gradients into the flat ``dst`` (fp32/bf16/fp16), * scale."""
    C = require()
    ptrs, mask = grad_pointers(dp, grads)
    if dst.dtype not in _DDT:
        raise TypeError("dst must be fp32, bf16 or fp16")
    _check(dst, dst.dtype, "dst", align=8)
    if dst.numel() < dp.plan.length:
        raise ValueError("dst too small for the bucket")
    C.pack_grads(ptrs, mask, dp.plan.num_tensors, _ptr(dp.chunks), dp.plan.num_chunks, _ptr(dst),
                 _DDT[dst.dtype], float(scale), _stream())


def sgd_ptrs(dp, grads, param, mom, lr, momentum=0.0, dampening=0.0, weight_decay=0.0,
             grad_scale=1.0, nesterov=False, first=False, shadow=None, lr_tensor=None):
    """SGD of one bucket (``param`` / ``mom`` / ``shadow``: its flat views) from autograd's
    per-tensor gradients, read in place through the pointer table (one launch)."""
    C = require()
    ptrs, mask = grad_pointers(dp, grads)
    for t, nm in ((param, "param"), (mom, "mom")):
        _check(t, torch.float32, nm)
        if t.numel() < dp.plan.length:
            raise ValueError(f"{nm} too small for the bucket")
    _check_shadow(dp, shadow)
    C.sgd_ptrs(ptrs, mask, dp.plan.num_tensors, _ptr(dp.chunks), dp.plan.num_chunks, _args(
        C.SgdFlatArgs, param=_ptr(param), mom=_ptr(mom), shadow=_ptr(shadow), lr=lr,
        momentum=momentum, dampening=dampening, weight_decay=weight_decay,
        grad_scale=grad_scale, nesterov=int(nesterov), first=int(first), stream=_stream(),
        lr_ptr=_lrp(lr_tensor)))


def cast_scale(src, dst, scale=1.0):
    C = require()
    _check(src, torch.float32, "src")
    if dst.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError("dst must be bf16 or fp16")
    _check(dst, dst.dtype, "dst", align=8)
    if src.numel() != dst.numel() or src.numel() % 4:
        raise ValueError("src/dst must have equal numel, a multiple of 4")
    C.cast_scale(_ptr(src), _ptr(dst), src.numel(), float(scale),
                 int(dst.dtype == torch.bfloat16), _stream())



# int32 words of a grid arrival ticket (common.h ew_grid_last: 8 sub-counters + 1 top, 128 B
# apart); zero-initialised, left zeroed by every launch
TICKET_INTS = 9 * 32


def make_batch(src, labels, perm, state, done, out, out_y, mean, inv_std, pad=4, augment=True,
               seed=0, rank=0):
    """Fused batch construction (``csrc/data.hip``): ``out[b] = normalise(augment(src[perm[pos*B
    + b]]))``, ``out_y[b] = labels[...]`` with ``pos = state[0]`` (advanced by the kernel)."""
    C_ = require()
    B = out.shape[0]
    N, C, H, W = src.shape
    if src.dtype != torch.uint8 or not src.is_contiguous() or not src.is_cuda:
        raise ValueError("src must be a contiguous uint8 device tensor [N, C, H, W]")
    if C > 4 or len(mean) != C or len(inv_std) != C:
        raise ValueError("make_batch supports C <= 4 channels with per-channel mean/std")
    if tuple(out.shape) != (B, C, H, W) or out.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("out must be fp32/bf16 [B, C, H, W]")
    cl = not out.is_contiguous()
    if cl and not out.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("out must be NCHW- or channels_last-contiguous")
    for t, dt, n in ((labels, torch.int64, "labels"), (perm, torch.int64, "perm"),
                     (state, torch.int64, "state"), (out_y, torch.int64, "out_y"),
                     (done, torch.int32, "done")):
        _check(t, dt, n, align=4)
    if done.numel() < TICKET_INTS:
        raise ValueError(f"done must hold TICKET_INTS ({TICKET_INTS}) zeroed int32")
    if state.numel() != 2 or out_y.numel() != B or labels.numel() != N:
        raise ValueError("state must be int64[2], out_y int64[B], labels int64[N]")
    if perm.numel() < B or B * H * W >= 2 ** 31:
        raise ValueError("perm shorter than one batch / batch too large")
    if augment and 2 * pad + 1 > 256:
        raise ValueError("pad too large")
    C_.make_batch(_ptr(src), _ptr(labels), _ptr(perm), perm.numel(), _ptr(state), _ptr(done), _ptr(out),
                  _ptr(out_y), B, C, H, W, int(pad), int(bool(augment)),
                  int(out.dtype == torch.bfloat16), int(cl), int(seed) & 0xFFFFFFFF,
                  int(rank) & 0xFFFFFFFF, [float(v) for v in mean], [float(v) for v in inv_std],
                  _stream())

def flag_signal(flags, i: int):
    """Stream hand-off (``csrc/stream_flag.hip``): bump counter ``i`` of the int32 ``flags`` (one
    128-B line per counter) on the current stream."""
    _check(flags, torch.int32, "flags", align=128)
    if not 0 <= i < flags.numel() // 32:
        raise ValueError("flag index out of range")
    require().flag_signal(flags.data_ptr() + 128 * i, _stream())


def flag_wait(flags, i: int, seen: int, need: int, err: int):
    """Wait on the current stream until counter ``i`` of ``flags`` has moved ``need`` more times
    than this wait's private ``seen`` counter (also a line of ``flags``) recorded; ``err``: the
    line counting a poll bound reached."""
    _check(flags, torch.int32, "flags", align=128)
    n = flags.numel() // 32
    if not all(0 <= j < n for j in (i, seen, err)) or need < 1:
        raise ValueError("flag index out of range")
    b = flags.data_ptr()
    require().flag_wait(b + 128 * i, b + 128 * seen, int(need), b + 128 * err, _stream())


def build(force: bool = False) -> str:
    from .build import build as _b
    return _b(force=force)


def hip_required() -> bool:
    """True when running on a GPU box where the HIP path must be used (fail loudly otherwise)."""
    return torch.cuda.is_available() and os.environ.get("EWDML_ALLOW_NO_EXT") != "1"
