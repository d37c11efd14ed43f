"""Run configuration and the ``distributed_nn.py`` command line.

Every flag of the reference CLI (``src/distributed_nn.py:24-72``) is accepted with the same name
and default; the ones the reference parses but never uses keep their meaning documented below.
New flags select the exchange method, codec, topology and the MI355X execution options.

Method presets (``--method``; ``Report.zip:main.tex:80-119``):
  1  vanilla PS: push dense grads to rank 0, server steps, pull dense *weights*
  2  QSGD push, dense weight pull
  3  push + pull dense gradients (the reference's live HEAD path) -> dense all-reduce
  4  QSGD both ways
  5  top-k -> QSGD both ways (ratio --topk-ratio; the report used 0.4)
  6  method 5 + communicate every --sync-every (default 20) steps + best-worker selection
Methods 1 and 2 imply ``--topology ps``; 3-6 default to the all-to-all topology (every GPU is a
worker, no idle server); ``--topology ps`` reproduces the reference's star for any method.
"""
import argparse
import dataclasses
from dataclasses import dataclass, field
from typing import Optional


def _str2bool(v) -> bool:
    if isinstance(v, bool):
        return v
    # reference `--enable-gpu` is `type=bool`: any non-empty string is True (distributed_nn.py:68)
    return str(v).strip().lower() not in ("", "0", "false", "no", "off", "none")


# density stages of the error-feedback warm-up (DGC's exponentially decreasing density)
EF_WARMUP_STAGES = (0.25, 0.125, 0.0625, 0.03125, 0.015625)


@dataclass
class Config:
    # ---- reference flags (distributed_nn.py:24-72) -----------------------------------------
    batch_size: int = 128
    test_batch_size: int = 500
    epochs: int = 100
    max_steps: int = 10000
    lr: float = 0.01
    momentum: float = 0.5
    no_cuda: bool = False
    seed: int = 1
    log_interval: int = 10
    network: str = "LeNet"
    mode: str = "normal"  # straggler mode; 'kill' enables the --kill-threshold step timeout
    kill_threshold: float = 7.0  # seconds a PS k-of-n push may lag the k-th arrival in kill mode
    dataset: str = "MNIST"
    comm_type: str = "Bcast"  # accepted; the all-to-all exchange needs no choice here
    num_aggregate: int = 5  # PS k-of-n: with --topology ps --mode kill the server averages the
    #                         first k worker gradients to arrive (parallel/ps.py)
    eval_freq: int = 50  # checkpoint (and evaluation) cadence in steps
    train_dir: str = "output/models/"
    compress_grad: str = "compress"  # 'none' forces --compress none (reference switch)
    gather_type: str = "gather"  # accepted for compatibility
    enable_gpu: bool = False
    local_rank: Optional[int] = None
    # ---- exchange / compression ---------------------------------------------------------------
    method: Optional[int] = None
    # none | fp16 | bf16 | qsgd | topk | topk_qsgd | sign | powersgd | vote | mx | tern | sketch |
    # thresh | intsgd
    compress: str = "topk_qsgd"
    powersgd_rank: int = 4  # --compress powersgd: rank of the factors (1, 2, 4 or 8)
    # --compress sketch (count sketch, parallel/sketch.py): rows of the table, 1, 3 or 5 (None: 3;
    # odd, so the median is one of the row values) and table columns per selected element, > 0
    # (None: 2.0); k per tensor is --topk-ratio / --topk-dense-below's
    sketch_rows: Optional[int] = None
    sketch_width: Optional[float] = None
    # --compress sign: none | hadamard (the signs of a randomised Hadamard rotation of every chunk,
    # DRIVE / EDEN; the same payload, one inverse transform on the receiver)
    sign_rotate: str = "none"
    # --compress mx (OCP Microscaling block floating point, one power-of-two scale byte per 32
    # elements): fp8 (MXFP8, E4M3 elements) | fp4 (MXFP4, E2M1) (None: fp8)
    mx_format: Optional[str] = None
    # --compress tern (TernGrad: ternary codes, one scaler per tensor): the scaler is min(max|g|,
    # tern_clip * rms(g)); 0 = no clipping (None: 2.5, the paper's constant)
    tern_clip: Optional[float] = None
    topk_ratio: float = 0.01
    topk_dense_below: int = 0  # tensors of <= N elements go whole (k = numel) through top-k codecs
    qsgd_levels: int = 127
    qsgd_bits: int = 8
    qsgd_norm: str = "max"  # max | l2 (the reference's L2 norm)
    topology: str = "allgather"  # allgather (all-to-all) | ps (rank-0 parameter server) |
    #                               sharded (every rank owns 1/N of each bucket: parallel/sharded.py)
    #                               | twostage (sign codec: sharded owners with worker and server
    #                               error feedback, parallel/twostage.py)
    pull: str = "grad"  # ps topology: pull averaged 'grad' or server 'weights'
    pull_compress: Optional[str] = None  # ps topology: codec of the pull (default = push codec)
    sync_every: int = 1  # local SGD: exchange every H steps (method 6)
    sync_mode: str = "grad"  # grad: compressed gradient on sync steps | model: compressed delta
    sync_mode_default: bool = True  # --sync-mode not given (--method 6 then selects 'model')
    select_best: bool = False  # method 6: adopt the weights of the best-accuracy rank at sync
    # local SGD in model mode: none | sgd (SlowMo / BMUF: heavy-ball momentum on the averaged
    # delta) | nesterov (DiLoCo: 0.7 / 0.9).  anchor += outer_lr * step(momentum, delta)
    outer_optimizer: str = "none"
    outer_lr: Optional[float] = None  # None: 1.0; > 0
    outer_momentum: Optional[float] = None  # None: 0.0; in [0, 1)
    # None (auto): on for the top-k codecs -- top-k at 1 % without error feedback trains 10-80x
    # slower than dense (profiles/validation/ef_stability_r03.md) -- and for the sign codec
    # (scaled sign is biased without its residual), off otherwise;
    # --no-error-feedback gives the reference's Methods 5/6 as published (no residual)
    error_feedback: Optional[bool] = None
    # dgc: momentum correction + momentum factor masking (the sender runs the momentum before
    # top-k; oracle.dgc_accumulate) | plain: residual of the raw gradient, momentum after decode
    ef_mode: str = "dgc"
    # top-k density warm-up (DGC's "exponentially decreasing sparsity"): comma-separated ratios
    # used in turn over the first --topk-warmup-epochs epochs, then --topk-ratio (e.g. "0.25,0.0625,
    # 0.015625"); each change re-plans the payloads (and re-captures a HIP graph)
    topk_warmup: str = ""
    topk_warmup_epochs: float = 2.0
    # auto: --error-feedback with a top-k codec brings its stability recipe unless set explicitly:
    # the density warm-up 25 % -> 12.5 % -> 6.25 % -> 3.125 % -> 1.5625 % (stages above
    # --topk-ratio) over --topk-warmup-epochs, and a linear lr warm-up from 0.1 lr over 2 epochs
    # (measured on ResNet-50: profiles/validation/ef_stability_r03.md) | none
    ef_warmup: str = "auto"
    bucket_mb: float = 16.0
    overlap: bool = True
    overlap_splits: int = 1  # --hip-graph segmented: comm graphs per step (split points)
    predivide: float = 1.0  # Horovod gradient_predivide_factor
    sync_bn: bool = False  # broadcast BN running stats from rank 0 at every checkpoint/eval
    # ---- optimizer -------------------------------------------------------------------------------
    # sgd | adam | amsgrad | onebit_adam (1-bit Adam) | lars | lamb (layer-wise trust ratios) |
    # onebit_lamb (1-bit LAMB) |
    # lion: optim/flat.py
    optimizer: str = "sgd"
    adam_eps: float = 1e-8  # epsilon of adam / amsgrad / onebit_adam
    # onebit_adam / onebit_lamb: dense steps before the variance is frozen and the sign-compressed
    # momentum exchange starts (required, >= 1)
    onebit_warmup_steps: Optional[int] = None
    lars_eta: Optional[float] = None  # lars: trust coefficient (None: 0.001)
    # lion: "B1,B2" (None: 0.9,0.99), each in [0, 1); resolved to a tuple of two floats
    lion_betas: Optional[str] = None
    # --compress vote (Distributed Lion's 1-bit exchange): majority | average of the received
    # signs (None: majority)
    vote_aggregate: Optional[str] = None
    # --compress vote: allgather (every rank receives every rank's bits) | twostage (workers ->
    # shard owners -> workers, one bit each way: parallel/twostage.py TwoStageVoteExchange)
    # (None: allgather)
    vote_exchange: Optional[str] = None
    # clip this rank's raw gradient by its global L2 norm before the exchange reads it (DGC's
    # local gradient clipping, parallel/clip.py): coef = min(1, C / (norm + 1e-6)); None: off
    clip_grad_norm: Optional[float] = None
    clip_scale_world: bool = False  # the threshold becomes C / sqrt(N), N workers (DGC's rule)
    weight_decay: float = 0.0
    dampening: float = 0.0
    nesterov: bool = False
    lr_scale_world: bool = False  # Horovod: lr *= world size
    lr_warmup_epochs: float = 0.0  # Horovod LearningRateWarmupCallback: lr/W -> lr linearly
    lr_warmup_start: Optional[float] = None  # warm-up's first lr as a fraction of lr (None: 1/W)
    lr_decay_epochs: str = ""  # e.g. "30,60,90": multiply lr by --lr-decay at these epochs
    lr_decay: float = 0.1
    # ---- execution -------------------------------------------------------------------------------
    device: str = "auto"  # auto | cuda | cpu
    # none (fp32 compute: the reference's precision, the default) | bf16 | fp16 (autocast compute
    # dtype; master weights fp32 either way)
    amp: str = "none"
    param_dtype: str = "auto"  # auto: conv/linear weights kept in bf16 (fp32 master) under bf16
    #                            autocast on the GPU all-to-all path | fp32
    channels_last: bool = False  # alias of layout="nhwc"
    layout: str = "auto"  # auto (nhwc on the GPU when the fused NHWC kernels run) | nchw | nhwc
    fused_nn: str = "on"  # on: conv-BN-ReLU-pool groups / 2x2 pools through ops/csrc/nn.hip | off
    fused_data: str = "on"  # on: training batches built by one graph-capturable kernel (GPU) | off
    # auto (full where the step can be captured, else eager) | off | split (graphs around eager
    # RCCL calls) | full (one graph) | segmented (linear compute segments + per-bucket comm graphs
    # on their own stream: collectives overlap backward)
    hip_graph: str = "auto"
    graph_warmup: int = 3  # eager steps (>= 1) before capture: MIOpen find, handles, momentum

    data_dir: Optional[str] = None  # None -> synthetic data of the dataset's shape
    synthetic_size: int = 0
    # > 0: train on the test split minus its last N samples and evaluate on those N (for data
    # directories that hold only a test split, e.g. the reference's MNIST t10k files)
    holdout_from_test: int = 0
    augment: bool = True
    # ---- checkpoint / metrics / faults -----------------------------------------------------------
    ckpt_dir: Optional[str] = None  # defaults to train_dir
    resume: bool = False
    legacy_ckpt: bool = True  # also write <train_dir>/model_step_ (the evaluator's file)
    eval_on_ckpt: bool = False
    metrics_file: Optional[str] = None  # per-step JSONL
    profile: int = 0  # wrap N steps in torch.profiler
    roctx: bool = False  # roctx ranges per phase (rocprofv3 --marker-trace)
    # per-step phase times (forward / backward / encode / collective / decode_update, or per graph
    # segment) from HIP events on the step's stream, in the JSONL and summary.json; serialises the
    # eager step (no side stream) and makes --hip-graph auto split the graph at the collectives
    phase_timing: bool = False
    # weight gradients of the MFMA convs on a second stream, beside the backward-data chain
    # (auto = on for deep conv nets, >= 30 convolutions, with pointer-mode gradients).  Measured
    # +1.7 % on ResNet-50 CIFAR and -6 % on VGG-11, but the fork / join per conv makes the
    # captured graph a DAG whose replay costs ~5 ms of host time per ResNet-50 step (0.12 ms
    # linear): off by default (profiles/ab/README.md)
    wgrad_stream: str = "off"
    summary_file: Optional[str] = None  # rank 0's run summary (default <train_dir>/summary.json)
    inject_fault: Optional[str] = None  # "rank:step" -> that rank raises at that step (tests)
    comm_timeout: float = 600.0
    sync_debug: bool = False  # synchronise after every custom kernel (race / fault localisation)
    quiet: bool = False

    def resolved(self) -> "Config":
        c = dataclasses.replace(self)
        if c.method is not None:
            m = int(c.method)
            if m not in range(1, 7):
                raise ValueError("--method must be in 1..6")
            if m == 1:
                c.topology, c.pull, c.compress = "ps", "weights", "none"
            elif m == 2:
                c.topology, c.pull, c.compress = "ps", "weights", "qsgd"
            elif m == 3:
                c.compress = "none"
            elif m == 4:
                c.compress = "qsgd"
            elif m in (5, 6):
                c.compress = "topk_qsgd"
            if m == 6:
                if c.sync_every == 1:
                    c.sync_every = 20
                c.select_best = True
                if c.sync_mode_default:  # compressed model delta, winner's delta adopted
                    c.sync_mode = "model"
        if c.compress_grad.lower() == "none":
            c.compress = "none"
        if c.sign_rotate not in ("none", "hadamard"):
            raise ValueError("--sign-rotate must be none or hadamard")
        if c.sign_rotate != "none":
            # the rotated sign codec (compress/oracle.py encode_sign, rot_key): the all-gather
            # exchange's encode and decode are rotated, nothing else is
            why = None
            if c.compress != "sign":
                why = f"rotates the sign codec: it needs --compress sign, not {c.compress!r}"
            elif c.topology == "twostage":
                why = ("does not run with --topology twostage: the owner re-encode would need a "
                       "transform pair of its own (the natural next step)")
            elif c.optimizer in ("onebit_adam", "onebit_lamb"):
                why = (f"does not run with --optimizer {c.optimizer}: its fused decode is not "
                       f"rotated")
            if why is not None:
                raise ValueError("--sign-rotate " + c.sign_rotate + " " + why)
        if c.compress == "mx":
            # MXFP8 / MXFP4 (compress/oracle.py encode_mx): the all-gather exchange's encode and
            # fused decode, with that exchange's residual; nothing else has an mx form
            if c.mx_format is None:
                c.mx_format = "fp8"
            why = None
            if c.mx_format not in ("fp8", "fp4"):
                why = f"sends fp8 or fp4 elements: --mx-format {c.mx_format!r} is neither"
            elif c.topology != "allgather":
                why = (f"runs the all-gather exchange, which keeps its residual: it does not run "
                       f"with --topology {c.topology} (no ps, sharded or two-stage form is built)")
            elif c.sync_every > 1:
                why = ("keeps its residual in the all-gather exchange: it does not run with "
                       "--sync-every > 1")
            elif c.select_best:
                why = ("keeps its residual in the all-gather exchange: it does not run with "
                       "--select-best")
            elif c.optimizer in ("onebit_adam", "onebit_lamb"):
                why = (f"is not the sign codec: --optimizer {c.optimizer} exchanges "
                       f"sign-compressed momentum (--compress sign)")
            elif c.pull_compress is not None:
                why = ("has no parameter-server form: --pull-compress belongs to --topology ps")
            if why is not None:
                raise ValueError("--compress mx " + why)
            if c.error_feedback is None:  # block floating point rounds to nearest: biased
                c.error_feedback = True
        elif c.mx_format is not None:
            raise ValueError("--mx-format belongs to --compress mx")
        if c.pull_compress == "mx":
            raise ValueError("--pull-compress mx: the mx codec has no parameter-server form")
        if c.compress == "tern":
            # TernGrad (compress/oracle.py encode_tern): the all-gather exchange's encode and fused
            # decode, every rank's codes decoded with its own scaler; nothing else has a tern form
            if c.tern_clip is None:
                c.tern_clip = 2.5
            why = None
            if not float(c.tern_clip) >= 0.0:
                why = f"clips at a multiple of the rms: --tern-clip {c.tern_clip!r} must be >= 0"
            elif c.topology != "allgather":
                why = (f"decodes every rank's codes with that rank's scaler in the all-gather "
                       f"exchange: it does not run with --topology {c.topology} (no ps, sharded or "
                       f"two-stage form is built)")
            elif c.sync_every > 1:
                why = ("is built into the all-gather exchange's every-step path: it does not run "
                       "with --sync-every > 1")
            elif c.select_best:
                why = ("is built into the all-gather exchange's every-step path: it does not run "
                       "with --select-best")
            elif c.optimizer in ("onebit_adam", "onebit_lamb"):
                why = (f"is not the sign codec: --optimizer {c.optimizer} exchanges "
                       f"sign-compressed momentum (--compress sign)")
            elif c.pull_compress is not None:
                why = ("has no parameter-server form: --pull-compress belongs to --topology ps")
            if why is not None:
                raise ValueError("--compress tern " + why)
            if c.error_feedback is None:  # unbiased apart from clipping; the paper runs without
                c.error_feedback = False
        elif c.tern_clip is not None:
            raise ValueError("--tern-clip belongs to --compress tern")
        if c.pull_compress == "tern":
            raise ValueError("--pull-compress tern: the tern codec has no parameter-server form")
        if c.compress == "thresh":
            # the threshold-search sparsifier (compress/oracle.py encode_thresh): the all-gather
            # exchange's encode and fused decode with that exchange's plain residual; k per tensor
            # is --topk-ratio / --topk-dense-below's.  --qsgd-bits / --qsgd-levels and --ef-warmup
            # none are accepted and unused (the values travel as fp32; there is no warm-up)
            why = None
            if c.topology != "allgather":
                why = (f"runs the all-gather exchange, which keeps its residual: it does not run "
                       f"with --topology {c.topology} (no ps, sharded or two-stage form is built)")
            elif c.sync_every > 1:
                why = ("keeps its residual in the all-gather exchange's every-step path: it does "
                       "not run with --sync-every > 1")
            elif c.select_best:
                why = ("keeps its residual in the all-gather exchange's every-step path: it does "
                       "not run with --select-best")
            elif c.pull_compress is not None:
                why = "has no parameter-server form: --pull-compress belongs to --topology ps"
            elif c.ef_mode != Config.ef_mode:
                why = (f"keeps a plain residual with the momentum on the receiver: --ef-mode "
                       f"{c.ef_mode} is not supported (leave --ef-mode unset)")
            elif c.optimizer in ("onebit_adam", "onebit_lamb"):
                why = (f"is not the sign codec: --optimizer {c.optimizer} exchanges "
                       f"sign-compressed momentum (--compress sign)")
            if why is not None:
                raise ValueError("--compress thresh " + why)
            if c.error_feedback is None:  # what lies below the threshold is never sent without it
                c.error_feedback = True
        if c.pull_compress == "thresh":
            raise ValueError("--pull-compress thresh: the thresh codec has no parameter-server "
                             "form")
        if c.compress == "intsgd":
            # IntSGD (parallel/intsgd.py): int8 codes under one model-wide scale, summed by one
            # all-reduce per bucket; the scale follows the norm of the last SGD update.  Error
            # feedback either way; --qsgd-bits / --qsgd-levels and --ef-warmup none are accepted
            # and unused (the wire is int8 with q = floor(127 / world) levels; no warm-up)
            why = None
            if c.optimizer != "sgd":
                why = (f"ties its quantisation step to the last update's norm over lr, which is a "
                       f"gradient only under SGD (about 1 per element under Adam-like rules, so "
                       f"the step would dwarf every gradient): it needs --optimizer sgd, not "
                       f"{c.optimizer!r}")
            elif c.topology != "allgather":
                why = (f"sums its codes by all-reduce on every rank: it does not run with "
                       f"--topology {c.topology} (no ps, sharded or two-stage form is built)")
            elif c.sync_every > 1:
                why = ("measures the update of every step for its scale: it does not run with "
                       "--sync-every > 1")
            elif c.select_best:
                why = "sums all workers' codes: it does not run with --select-best"
            elif c.pull_compress is not None:
                why = "has no parameter-server form: --pull-compress belongs to --topology ps"
            elif c.predivide != 1.0:
                why = ("averages the summed codes with 1 / (alpha N) in its decode: it does not "
                       "run with --predivide other than 1")
            elif c.ef_mode != Config.ef_mode:
                why = (f"keeps a plain residual with the momentum on the receiver: --ef-mode "
                       f"{c.ef_mode} is not supported (leave --ef-mode unset)")
            elif c.hip_graph in ("full", "segmented"):
                why = (f"issues its all-reduces between two graphs: --hip-graph {c.hip_graph} is "
                       f"not supported (auto resolves to split)")
            if why is not None:
                raise ValueError("--compress intsgd " + why)
            if c.error_feedback is None:  # unbiased apart from clipping; the paper runs without
                c.error_feedback = False
            if c.hip_graph == "auto":  # graph A -> eager int8 all-reduces -> graph B
                c.hip_graph = "split"
        if c.pull_compress == "intsgd":
            raise ValueError("--pull-compress intsgd: the intsgd codec has no parameter-server "
                             "form")
        if c.compress == "vote":
            # Distributed Lion (parallel/engine.py GradientExchange, vote mode): every rank sends
            # the sign of its own Lion update, one bit per element and no magnitude, so only Lion
            # can step on it and nothing that scales or compensates a magnitude applies
            why = None
            if c.optimizer != "lion":
                why = (f"carries no magnitudes, only Lion's sign update can step on it: it needs "
                       f"--optimizer lion, not {c.optimizer!r}")
            elif c.topology != "allgather":
                why = (f"is an all-gather of every rank's bits: it does not run with --topology "
                       f"{c.topology} (the vote's own sharded form is --vote-exchange twostage)")
            elif c.sync_every > 1:
                why = "votes every step: it does not run with --sync-every > 1"
            elif c.select_best:
                why = "takes the vote of all workers: it does not run with --select-best"
            elif c.predivide != 1.0:
                why = ("counts signs, there is nothing to pre-divide: it does not run with "
                       "--predivide other than 1")
            elif c.error_feedback:
                why = ("sends no magnitude that a residual could compensate: it does not run "
                       "with --error-feedback")
            if why is not None:
                raise ValueError("--compress vote " + why)
            c.error_feedback = False
            if c.vote_aggregate is None:
                c.vote_aggregate = "majority"
            if c.vote_aggregate not in ("majority", "average"):
                raise ValueError("--vote-aggregate must be majority or average")
            if c.vote_exchange is None:
                c.vote_exchange = "allgather"
            if c.vote_exchange not in ("allgather", "twostage"):
                raise ValueError("--vote-exchange must be allgather or twostage")
            if c.vote_exchange == "twostage":
                # workers -> shard owners -> workers (parallel/twostage.py TwoStageVoteExchange)
                why = None
                if c.vote_aggregate == "average":
                    why = ("sends one bit per element back from the shard owners, and a mean "
                           "does not fit one bit: it does not run with --vote-aggregate average")
                elif c.hip_graph in ("full", "segmented"):
                    why = (f"issues its two collectives and the owner step between two graphs: "
                           f"--hip-graph {c.hip_graph} is not supported (auto resolves to split)")
                if why is not None:
                    raise ValueError("--vote-exchange twostage " + why)
                if c.hip_graph == "auto":  # graph A -> eager collectives + owner step -> graph B
                    c.hip_graph = "split"
        elif c.vote_aggregate is not None:
            raise ValueError("--vote-aggregate belongs to --compress vote")
        elif c.vote_exchange is not None:
            raise ValueError("--vote-exchange belongs to --compress vote")
        if c.optimizer == "lion":
            try:
                raw = c.lion_betas or "0.9,0.99"  # a tuple when an already resolved Config
                betas = tuple(float(v) for v in (raw.split(",") if isinstance(raw, str) else raw))
            except (TypeError, ValueError):
                betas = ()
            if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
                raise ValueError(f"--lion-betas takes B1,B2 with each in [0, 1), not "
                                 f"{c.lion_betas!r}")
            c.lion_betas = betas
        elif c.lion_betas is not None:
            raise ValueError("--lion-betas belongs to --optimizer lion")
        if c.error_feedback is None:
            # only the all-gather exchange keeps a residual (parallel/engine.py
            # GradientExchange); the parameter-server / sharded exchanges have none, so their
            # top-k runs keep the reference's schedule (no EF warm-up) and record no EF
            c.error_feedback = ((c.compress in ("topk", "topk_qsgd", "sign")
                                 and c.topology == "allgather")
                                or (c.compress == "sign" and c.topology == "twostage")
                                or c.compress in ("powersgd", "sketch"))
        if c.optimizer == "onebit_lamb":
            # 1-bit LAMB's compressed stage is the sign codec's all-gather with its residual, as
            # 1-bit Adam's; refused ahead of the exchanges' own checks so the reason names it
            why = None
            if c.onebit_warmup_steps is None or int(c.onebit_warmup_steps) < 1:
                why = "needs --onebit-warmup-steps N >= 1 (the dense LAMB steps before the freeze)"
            elif c.compress != "sign":
                why = "exchanges sign-compressed momentum: it needs --compress sign"
            elif c.topology == "twostage":
                why = ("runs the all-gather exchange: --topology twostage (the natural next "
                       "step, as for 1-bit Adam) is not built yet")
            elif c.topology != "allgather":
                why = (f"keeps its residual in the all-gather exchange: it does not run with "
                       f"--topology {c.topology}")
            elif c.sync_every > 1:
                why = "exchanges its momentum every step: it does not run with --sync-every > 1"
            elif c.select_best:
                why = "averages all workers' momenta: it does not run with --select-best"
            elif not c.error_feedback:
                why = ("compresses the error-compensated momentum: it does not run with "
                       "--no-error-feedback")
            elif c.predivide != 1.0:
                why = ("averages decoded momenta with 1/N: it does not run with --predivide "
                       "other than 1")
            elif c.lars_eta is not None:
                why = "takes LAMB's trust ratios, which have no eta: --lars-eta belongs to lars"
            if why is not None:
                raise ValueError("--optimizer onebit_lamb " + why)
        if c.topology == "twostage":
            # the two-stage sign all-reduce (parallel/twostage.py): both of its quantisations
            # are error-compensated, and the owners average with 1/N
            why = None
            if c.compress != "sign":
                why = (f"is the sign codec's exchange: it needs --compress sign, not "
                       f"{c.compress!r}")
            elif not c.error_feedback:
                why = ("compensates both of its quantisations with a residual: it does not run "
                       "with --no-error-feedback")
            elif c.sync_every > 1:
                why = "exchanges every step: it does not run with --sync-every > 1"
            elif c.select_best:
                why = "averages all workers: it does not run with --select-best"
            elif c.predivide != 1.0:
                why = ("averages on the shard owners with 1/N: it does not run with --predivide "
                       "other than 1")
            elif c.hip_graph in ("full", "segmented"):
                why = (f"issues its two collectives and the owner step between two graphs: "
                       f"--hip-graph {c.hip_graph} is not supported (auto resolves to split)")
            if why is not None:
                raise ValueError("--topology twostage " + why)
        elif c.compress == "sign" and (c.topology != "allgather" or c.sync_every > 1
                                       or c.select_best):
            # scaled sign is biased without error feedback, and only GradientExchange keeps one
            raise ValueError("--compress sign needs the all-gather exchange's residual: it does "
                             "not run with --topology ps / sharded, --sync-every > 1 or "
                             "--select-best (those exchanges keep no error feedback); "
                             "--topology twostage is the sign codec's sharded exchange")
        if c.compress == "powersgd":
            # PowerSGD (parallel/powersgd.py): two dependent all-reduces of rank-r factors per
            # bucket, always with its residual, averaged with 1/N inside its kernels
            why = None
            if c.powersgd_rank not in (1, 2, 4, 8):
                why = f"supports ranks 1, 2, 4 and 8, not --powersgd-rank {c.powersgd_rank}"
            elif c.topology != "allgather":
                why = (f"averages its factors by all-reduce on every rank: it does not run with "
                       f"--topology {c.topology}")
            elif c.sync_every > 1:
                why = "exchanges every step: it does not run with --sync-every > 1"
            elif c.select_best:
                why = "averages all workers: it does not run with --select-best"
            elif not c.error_feedback:
                why = ("is a biased compressor that relies on its residual: it does not run with "
                       "--no-error-feedback")
            elif c.predivide != 1.0:
                why = ("averages its factors with 1/N in its kernels: it does not run with "
                       "--predivide other than 1")
            elif c.hip_graph in ("full", "segmented"):
                why = (f"issues its two all-reduces, the orthogonalisation and the back-projection "
                       f"between two graphs: --hip-graph {c.hip_graph} is not supported (auto "
                       f"resolves to split)")
            elif c.optimizer == "onebit_adam":
                why = ("is not the sign codec: --optimizer onebit_adam exchanges sign-compressed "
                       "momentum (--compress sign)")
            if why is not None:
                raise ValueError("--compress powersgd " + why)
        elif c.powersgd_rank != Config.powersgd_rank:
            raise ValueError("--powersgd-rank belongs to --compress powersgd")
        if c.compress == "sketch":
            # the count sketch (parallel/sketch.py): two dependent all-reduces per bucket (the
            # table, then the selected coordinates' values), always with its plain residual,
            # averaged with 1/N in its decode
            if c.sketch_rows is None:
                c.sketch_rows = 3
            if c.sketch_width is None:
                c.sketch_width = 2.0
            why = None
            if c.sketch_rows not in (1, 3, 5):
                why = (f"takes the median of an odd number of rows: --sketch-rows must be 1, 3 or "
                       f"5, not {c.sketch_rows}")
            elif not float(c.sketch_width) > 0.0:
                why = (f"sizes its table in columns per selected element: --sketch-width must be "
                       f"> 0, not {c.sketch_width!r}")
            elif c.topology != "allgather":
                why = (f"sums its tables by all-reduce on every rank: it does not run with "
                       f"--topology {c.topology}")
            elif c.sync_every > 1:
                why = "exchanges every step: it does not run with --sync-every > 1"
            elif c.select_best:
                why = "sums all workers' sketches: it does not run with --select-best"
            elif not c.error_feedback:
                why = ("sends only the heavy coordinates and relies on its residual for the rest: "
                       "it does not run with --no-error-feedback")
            elif c.ef_mode != Config.ef_mode:
                why = (f"keeps a plain residual with the momentum on the receiver: --ef-mode "
                       f"{c.ef_mode} is not supported (leave --ef-mode unset)")
            elif c.predivide != 1.0:
                why = ("averages the summed values with 1/N in its decode: it does not run with "
                       "--predivide other than 1")
            elif c.pull_compress is not None:
                why = "has no parameter-server form: --pull-compress belongs to --topology ps"
            elif c.hip_graph in ("full", "segmented"):
                why = (f"issues its two all-reduces, the estimate, the selection and the gather "
                       f"between two graphs: --hip-graph {c.hip_graph} is not supported (auto "
                       f"resolves to split)")
            elif c.optimizer in ("onebit_adam", "onebit_lamb"):
                why = (f"is not the sign codec: --optimizer {c.optimizer} exchanges "
                       f"sign-compressed momentum (--compress sign)")
            if why is not None:
                raise ValueError("--compress sketch " + why)
            if c.hip_graph == "auto":  # graph A -> eager all-reduces, select, gather -> graph B
                c.hip_graph = "split"
        elif c.sketch_rows is not None:
            raise ValueError("--sketch-rows belongs to --compress sketch")
        elif c.sketch_width is not None:
            raise ValueError("--sketch-width belongs to --compress sketch")
        if c.pull_compress == "sketch":
            raise ValueError("--pull-compress sketch: the sketch codec has no parameter-server "
                             "form")
        if c.optimizer == "onebit_adam":
            # the compressed stage is the sign codec's all-gather with its residual; every option
            # that changes what is exchanged, or that scales it, breaks the momentum's linearity
            why = None
            if c.onebit_warmup_steps is None or int(c.onebit_warmup_steps) < 1:
                why = "needs --onebit-warmup-steps N >= 1 (the dense Adam steps before the freeze)"
            elif c.compress != "sign":
                why = "exchanges sign-compressed momentum: it needs --compress sign"
            elif not c.error_feedback:
                why = ("compresses the error-compensated momentum: it does not run with "
                       "--no-error-feedback")
            elif c.predivide != 1.0:
                why = ("averages decoded momenta with 1/N: it does not run with --predivide "
                       "other than 1")
            if why is not None:
                raise ValueError("--optimizer onebit_adam " + why)
        elif c.onebit_warmup_steps is not None and c.optimizer != "onebit_lamb":
            raise ValueError("--onebit-warmup-steps belongs to --optimizer onebit_adam / "
                             "onebit_lamb")
        if c.optimizer == "lars":
            if c.lars_eta is None:
                c.lars_eta = 0.001
            if not c.lars_eta > 0:
                raise ValueError("--lars-eta must be > 0")
        elif c.lars_eta is not None:
            raise ValueError("--lars-eta belongs to --optimizer lars")
        if c.clip_grad_norm is not None:
            # the clip scales every gradient of the rank once, after backward and before any
            # encode (parallel/clip.py); the exchanges below do not take a clipper
            why = None
            if not float(c.clip_grad_norm) > 0:
                why = f"must be > 0, not {c.clip_grad_norm!r}"
            elif c.topology in ("ps", "sharded"):
                why = (f"clips ahead of the all-to-all, two-stage and PowerSGD exchanges: "
                       f"--topology {c.topology} is out of scope")
            elif c.sync_every > 1:
                why = ("clips the gradient of an exchanged step: local steps "
                       "(--sync-every > 1) are out of scope")
            elif c.select_best:
                why = "clips the gradient of an exchanged step: --select-best is out of scope"
            elif c.hip_graph == "segmented":
                why = ("needs every gradient before any encode, so there is nothing to overlap: "
                       "it does not run with --hip-graph segmented")
            if why is not None:
                raise ValueError("--clip-grad-norm " + why)
        elif c.clip_scale_world:
            raise ValueError("--clip-scale-world divides the --clip-grad-norm threshold by "
                             "sqrt(N): it needs --clip-grad-norm")
        if c.outer_optimizer not in ("none", "sgd", "nesterov"):
            raise ValueError("--outer-optimizer must be none, sgd or nesterov")
        if c.outer_optimizer != "none":
            # SlowMo / BMUF (sgd) and DiLoCo (nesterov): the averaged model delta of a sync steps
            # the common anchor as a pseudo-gradient (parallel/local_sgd.py, ops/csrc/outer.hip)
            if c.outer_lr is None:
                c.outer_lr = 1.0
            if c.outer_momentum is None:
                c.outer_momentum = 0.0
            why = None
            if c.sync_every <= 1:
                why = ("steps on the model delta of H local steps: it needs --sync-every > 1")
            elif c.sync_mode != "model":
                why = ("steps on the averaged model delta: --sync-mode grad exchanges a gradient "
                       "and re-broadcasts the replicas, there is no delta (it needs --sync-mode "
                       "model)")
            elif not (0.0 < float(c.outer_lr) < float("inf")):
                why = f"needs --outer-lr > 0, not {c.outer_lr!r}"
            elif not 0.0 <= float(c.outer_momentum) < 1.0:
                why = f"needs --outer-momentum in [0, 1), not {c.outer_momentum!r}"
            elif c.outer_optimizer == "nesterov" and float(c.outer_momentum) == 0.0:
                why = ("looks ahead along its momentum: it needs --outer-momentum > 0 (torch's "
                       "rule for nesterov)")
            if why is not None:
                raise ValueError(f"--outer-optimizer {c.outer_optimizer} " + why)
        elif c.outer_lr is not None:
            raise ValueError("--outer-lr belongs to --outer-optimizer sgd / nesterov")
        elif c.outer_momentum is not None:
            raise ValueError("--outer-momentum belongs to --outer-optimizer sgd / nesterov")
        if c.ef_mode == "ef21" and c.error_feedback and c.device != "cpu" and not c.no_cuda:
            import os

            # the EF21 encode exists only in the torch oracle (flat gradient views)
            if not (os.environ.get("EWDML_ORACLE") == "1"
                    and os.environ.get("EWDML_GRAD_VIEWS") == "1"):
                import torch

                if c.device == "cuda" or torch.cuda.is_available():
                    raise ValueError("--ef-mode ef21 has no HIP encode kernel: run it on the CPU, "
                                     "or on the GPU with EWDML_ORACLE=1 EWDML_GRAD_VIEWS=1")
        if (c.ef_warmup == "auto" and c.error_feedback and c.compress in ("topk", "topk_qsgd")
                and c.sync_every == 1 and not c.select_best):
            stages = [r for r in EF_WARMUP_STAGES if r > c.topk_ratio]
            if not c.topk_warmup:
                c.topk_warmup = ",".join(f"{r:g}" for r in stages)
            if stages and c.lr_warmup_epochs <= 0:
                c.lr_warmup_epochs = 2.0
                if c.lr_warmup_start is None:
                    c.lr_warmup_start = 0.1
        if c.topology not in ("allgather", "ps", "sharded", "twostage"):
            raise ValueError("--topology must be allgather, ps, sharded or twostage")
        if c.graph_warmup < 1:
            raise ValueError("--graph-warmup must be >= 1 (one eager step initialises the stream)")
        if c.ckpt_dir is None:
            c.ckpt_dir = c.train_dir
        if c.channels_last:
            c.layout = "nhwc"
        return c


def build_parser(prog="distributed_nn.py") -> argparse.ArgumentParser:
    d = Config()
    p = argparse.ArgumentParser(prog=prog, description="MI355X gradient-compressed data-parallel "
                                "training (parameter-server / all-reduce / top-k + QSGD)")
    a = p.add_argument
    # reference flags
    a("--batch-size", type=int, default=d.batch_size)
    a("--test-batch-size", type=int, default=d.test_batch_size)
    a("--epochs", type=int, default=d.epochs)
    a("--max-steps", type=int, default=d.max_steps)
    a("--lr", type=float, default=d.lr)
    a("--momentum", type=float, default=d.momentum)
    a("--no-cuda", action="store_true", default=False)
    a("--seed", type=int, default=d.seed)
    a("--log-interval", type=int, default=d.log_interval)
    a("--network", type=str, default=d.network)
    a("--mode", type=str, default=d.mode)
    a("--kill-threshold", type=float, default=d.kill_threshold)
    a("--dataset", type=str, default=d.dataset)
    a("--comm-type", type=str, default=d.comm_type)
    a("--num-aggregate", type=int, default=d.num_aggregate)
    a("--eval-freq", type=int, default=d.eval_freq)
    a("--train-dir", type=str, default=d.train_dir)
    a("--compress-grad", type=str, default=d.compress_grad)
    a("--gather-type", type=str, default=d.gather_type)
    a("--enable-gpu", type=_str2bool, default=d.enable_gpu)
    a("--local_rank", "--local-rank", dest="local_rank", type=int, default=None)
    # exchange
    a("--method", type=int, default=None, choices=range(1, 7))
    a("--compress", type=str, default=d.compress,
      choices=["none", "fp16", "bf16", "qsgd", "topk", "topk_qsgd", "sign", "powersgd", "vote",
               "mx", "tern", "sketch", "thresh", "intsgd"])
    a("--sketch-rows", type=int, default=None)
    a("--sketch-width", type=float, default=None)
    a("--mx-format", type=str, default=None, choices=["fp8", "fp4"])
    a("--tern-clip", type=float, default=None)
    a("--vote-aggregate", type=str, default=None, choices=["majority", "average"])
    a("--vote-exchange", type=str, default=None, choices=["allgather", "twostage"])
    a("--powersgd-rank", type=int, default=d.powersgd_rank)
    a("--sign-rotate", type=str, default=d.sign_rotate, choices=["none", "hadamard"])
    a("--topk-ratio", type=float, default=d.topk_ratio)
    a("--topk-dense-below", type=int, default=d.topk_dense_below)
    a("--qsgd-levels", type=int, default=d.qsgd_levels)
    a("--qsgd-bits", type=int, default=d.qsgd_bits, choices=[4, 8])
    a("--qsgd-norm", type=str, default=d.qsgd_norm, choices=["max", "l2"])
    a("--topology", type=str, default=d.topology, choices=["allgather", "ps", "sharded", "twostage"])
    a("--pull", type=str, default=d.pull, choices=["grad", "weights"])
    a("--pull-compress", type=str, default=None,
      choices=["none", "fp16", "bf16", "qsgd", "topk", "topk_qsgd"])
    a("--sync-every", type=int, default=d.sync_every)
    a("--sync-mode", type=str, default=None, choices=["grad", "model"])
    a("--select-best", action="store_true", default=False)
    a("--outer-optimizer", type=str, default=d.outer_optimizer,
      choices=["none", "sgd", "nesterov"])
    a("--outer-lr", type=float, default=None)
    a("--outer-momentum", type=float, default=None)
    a("--error-feedback", dest="error_feedback", action="store_true", default=None)
    a("--no-error-feedback", dest="error_feedback", action="store_false")
    a("--ef-mode", type=str, default=d.ef_mode, choices=["dgc", "plain", "local", "ef21"])
    a("--topk-warmup", type=str, default=d.topk_warmup)
    a("--topk-warmup-epochs", type=float, default=d.topk_warmup_epochs)
    a("--ef-warmup", type=str, default=d.ef_warmup, choices=["auto", "none"])
    a("--bucket-mb", type=float, default=d.bucket_mb)
    a("--no-overlap", dest="overlap", action="store_false", default=True)
    a("--overlap-splits", type=int, default=d.overlap_splits)
    a("--predivide", type=float, default=d.predivide)
    a("--sync-bn", "--sync-bn-buffers", dest="sync_bn", action="store_true", default=False)
    # optimizer
    a("--optimizer", type=str, default=d.optimizer,
      choices=["sgd", "adam", "amsgrad", "onebit_adam", "lars", "lamb", "lion",
               "onebit_lamb"])
    a("--lion-betas", type=str, default=None)
    a("--adam-eps", type=float, default=d.adam_eps)
    a("--onebit-warmup-steps", type=int, default=None)
    a("--lars-eta", type=float, default=None)
    a("--clip-grad-norm", type=float, default=None)
    a("--clip-scale-world", action="store_true", default=False)
    a("--weight-decay", type=float, default=d.weight_decay)
    a("--dampening", type=float, default=d.dampening)
    a("--nesterov", action="store_true", default=False)
    a("--lr-scale-world", action="store_true", default=False)
    a("--lr-warmup-epochs", type=float, default=d.lr_warmup_epochs)
    a("--lr-warmup-start", type=float, default=None)
    a("--lr-decay-epochs", type=str, default=d.lr_decay_epochs)
    a("--lr-decay", type=float, default=d.lr_decay)
    # execution
    a("--device", type=str, default=d.device, choices=["auto", "cuda", "cpu"])
    a("--amp", type=str, default=d.amp, choices=["bf16", "fp16", "none"])
    a("--param-dtype", type=str, default=d.param_dtype, choices=["auto", "fp32"])
    a("--channels-last", action="store_true", default=False)
    a("--layout", type=str, default=d.layout, choices=["auto", "nchw", "nhwc"])
    a("--fused-nn", type=str, default=d.fused_nn, choices=["on", "off"])
    a("--fused-data", type=str, default=d.fused_data, choices=["on", "off"])
    a("--hip-graph", type=str, default=d.hip_graph,
      choices=["auto", "off", "split", "full", "segmented"])
    a("--graph-warmup", type=int, default=d.graph_warmup)
    a("--data-dir", type=str, default=None)
    a("--holdout-from-test", type=int, default=d.holdout_from_test)
    a("--synthetic-size", type=int, default=0)
    a("--no-augment", dest="augment", action="store_false", default=True)
    # checkpoint / metrics / faults
    a("--ckpt-dir", type=str, default=None)
    a("--resume", action="store_true", default=False)
    a("--no-legacy-ckpt", dest="legacy_ckpt", action="store_false", default=True)
    a("--eval-on-ckpt", action="store_true", default=False)
    a("--metrics-file", type=str, default=None)
    a("--profile", type=int, default=0)
    a("--roctx", action="store_true", default=False)
    a("--phase-timing", action="store_true", default=False)
    a("--wgrad-stream", choices=["auto", "on", "off"], default=d.wgrad_stream)
    a("--summary-file", type=str, default=None)
    a("--inject-fault", type=str, default=None)
    a("--comm-timeout", type=float, default=d.comm_timeout)
    a("--sync-debug", action="store_true", default=False)
    a("--quiet", action="store_true", default=False)
    return p


def parse_args(argv=None, prog="distributed_nn.py") -> Config:
    ns = build_parser(prog).parse_args(argv)
    ns.sync_mode_default = ns.sync_mode is None
    if ns.sync_mode is None:
        ns.sync_mode = Config.sync_mode
    fields = {f.name for f in dataclasses.fields(Config)}
    return Config(**{k: v for k, v in vars(ns).items() if k in fields}).resolved()
