// Host-side entry points of the ewdml HIP kernels (C++ only, no HIP types), bound to Python in
// bindings.cpp.  Pointers are device addresses passed as integers; `stream` is a hipStream_t.
//
// The *Args structs of the codecs and optimizers are the Python interface: bindings.cpp binds each
// as a class whose fields ops/__init__.py sets by name, so a new field needs one F(field) there
// (and nothing else).  T() in Python is T{}: every field zero, but for an embedded StepArgs, which
// starts as Python's StepArgs() does: all zero with grad_scale 1.  GradSrc members are not bound.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>
#include <stddef.h>
#include <stdint.h>

// Where an encode (or the clip) reads a bucket's gradients: one base pointer per tensor.
struct GradSrc {
  const uintptr_t* grad_ptrs;  // per-tensor gradient base pointers (host array, n_grad_ptrs)
  int n_grad_ptrs;
  const uint32_t* bf16_mask;   // bit t: tensor t's gradient is bf16
  int n_bf16_mask;
};

// What the receive side of every exchange does with a bucket's decoded mean g * grad_scale: write
// it to grad_out and / or (apply) take the fused SGD step on param / mom (mom 0: a step without
// momentum) with the bf16 shadow.  The bucket views hold the bucket's length in elements.
struct StepArgs {
  uintptr_t param, mom, grad_out, shadow;
  float lr, momentum, dampening, weight_decay, grad_scale;
  int nesterov, first, apply;
  uintptr_t key_state;  // nullable int32[2] {step, key}: advanced to the next step (HIP graphs)
  uint32_t key_seed, key_rank;
  uintptr_t lr_ptr;  // nullable device fp32 learning rate (overrides lr)
};

// The checks every decode entry point makes before its launch (need_mom: the kernel reads the
// momentum buffer whatever the momentum is)
inline void ew_step_check(const std::string& who, const StepArgs& s, bool need_mom) {
  if (s.apply && !s.param) throw std::runtime_error(who + ": apply needs the parameters");
  if (!s.apply && !s.grad_out) throw std::runtime_error(who + ": nothing to write");
  if (s.apply && !s.mom && (need_mom || s.momentum != 0.0f || s.nesterov))
    throw std::runtime_error(who + ": a momentum step needs the momentum buffer");
  if ((s.param | s.mom | s.grad_out) % 16 || s.shadow % 8 || (s.key_state | s.lr_ptr) % 4)
    throw std::runtime_error(who + ": misaligned operand");
}

struct TopkEncodeArgs {
  GradSrc src;
  uintptr_t resid, chunks, tensors, scratch, payload, stream;
  long long payload_bytes;
  int num_tensors, num_chunks;
  int scales_off, counts_off, idx_off, codes_off, bitmap_off;
  int value_kind;  // 0 = int8 QSGD, 1 = int4 QSGD, 2 = fp32 values (plain top-k)
  int norm_l2;     // 0 = max-norm scale, 1 = L2 norm of the selected values
  float levels, inv_levels;
  uint32_t key, bucket_offset;
  uintptr_t key_ptr;  // optional device uint32 overriding `key` (graph replay)
  // error feedback with momentum correction (DGC; compress/oracle.py dgc_accumulate): per-rank
  // velocity (0: plain error feedback) and the bucket's fp32 parameters (read when dgc_wd != 0)
  uintptr_t vel, param;
  float dgc_momentum, dgc_damp1, dgc_wd;  // damp1 = 1 - dampening
  int dgc_nesterov;
  int dgc_mask;          // clear the velocity at sent coordinates (DGC) or keep it (local)
  uintptr_t dgc_lr_ptr;  // nullable device lr: residual accumulates lr-scaled updates
  long long bucket_len;  // elements (sizes the candidate list in the scratch)
  // predictive encode (max-norm scale only): candidate-pass block table (CBlockRow[num_cblocks])
  uintptr_t cblocks;
  int num_cblocks;
  int predict;
  int lb_fault;  // test hook: tensors' first chunks skip their look-back word (lb_err path)
  int max_k;     // largest per-tensor k of the bucket (0: unknown)
  // world of one (the all-gather is this rank's payload): the write pass also applies the update
  // the decode would, p -= lr * scale * sent at each sent coordinate (momentum-corrected error
  // feedback: no receiver momentum); apply_param 0 = off.  apply_key_state: advance the RNG key
  // state {step, key} after every block read the key (the last bucket's decode did it)
  uintptr_t apply_param, apply_shadow, apply_lr_ptr, apply_key_state;
  float apply_lr, apply_scale;
  uint32_t apply_key_seed, apply_key_rank;
  // dense variant (receiver-side momentum SGD over every element; one-launch encodes only)
  uintptr_t dgc_stamps;  // nullable u32[T]: producer-staged tensors (dgc_stage.h)
  int apply_mom_set;
  uintptr_t apply_mom;
  float apply_momentum, apply_dampening, apply_wd;
  int apply_nesterov, apply_first;
};

struct TopkDecodeArgs {
  uintptr_t recv, chunks, tensors, stream;
  long long stride;
  int nranks, num_chunks;
  int scales_off, counts_off, idx_off, codes_off, bitmap_off;
  int value_kind;
  float inv_levels;
  StepArgs step;
};

struct QsgdEncodeArgs {
  GradSrc src;
  uintptr_t resid, chunks, tensors, scratch, payload, stream;
  long long payload_bytes;
  int num_tensors, num_chunks;
  int scales_off, codes_off, bits, norm_l2;
  float levels, inv_levels;
  uint32_t key, bucket_offset;
  uintptr_t key_ptr;
};

struct QsgdDecodeArgs {
  uintptr_t recv, chunks, tensors, stream;
  long long stride;
  int nranks, num_chunks;
  int scales_off, codes_off, bits;
  float inv_levels;
  StepArgs step;  // the kernel reads step.mom whenever it applies
};

// scaled sign with error feedback (sign_codec.hip): scales f32[C] | bits u32[256 * C]
struct SignEncodeArgs {
  GradSrc src;
  uintptr_t resid, chunks, payload, stream;  // resid 0: no error feedback
  long long payload_bytes;
  int num_tensors, num_chunks;
  int scales_off, bits_off;
  // 1-bit Adam's momentum encode (mom_exp_avg != 0; needs resid): the compressed vector is
  // exp_avg * beta1 + (1 - beta1) * (g + wd * param) + resid; exp_avg and param are only read
  uintptr_t mom_exp_avg, mom_param;
  float mom_beta1, mom_wd;
  // slot-addressed form (slots != 0; the two-stage exchange): int2 per chunk = byte offsets of its
  // scale and of its 256 words in `payload`, an [N, P] row buffer of payload_bytes bytes; slot_end
  // = the largest offset a slot reaches.  scales_off / bits_off are unused and no pad is written
  uintptr_t slots;
  long long slot_end;
  // the rotated form (rotate != 0; --sign-rotate hadamard): the signs are taken of H(D e) over all
  // 8192 positions of every chunk row and the residual is rotated back; rot_key picks D.  No
  // slot-addressed and no momentum form
  int rotate;
  uint32_t rot_key;
};

// the two-stage exchange's owner step (sign_codec.hip k_sign_reduce_encode): the rows of recv
// (stride bytes apart, the shard's layout in each) summed in rank order, times inv_n, plus the
// server residual, re-encoded into `out` (same layout); sresid is updated in place
struct SignReduceArgs {
  uintptr_t recv, chunks, sresid, out, stream;
  long long stride, out_bytes;
  int nranks, num_chunks;
  int scales_off, bits_off;
  float inv_n;
};

// 1-bit Adam's fused decode -> exp_avg = mean -> frozen-variance step (sign_codec.hip)
struct SignOnebitArgs {
  uintptr_t recv, chunks, param, exp_avg, exp_avg_sq, shadow, stream;  // exp_avg_sq is read only
  long long stride;
  int nranks, num_chunks;
  int scales_off, bits_off;
  float lr_step, inv_n, eps, beta1, beta2;
  int freeze_step;
  uintptr_t step;    // nullable int32 device step counter: lr_step derived on the device
  double lr;         // base lr for the device-side lr_step
  uintptr_t lr_ptr;  // nullable device fp32 base lr (overrides lr)
  uintptr_t key_state;  // see StepArgs
  uint32_t key_seed, key_rank;
  uintptr_t slots;  // see SignEncodeArgs: recv is the gathered row buffer (stride = its bytes),
  long long slot_end;  // nranks must be 1
};

// 1-bit LAMB's receive side (sign_codec.hip k_sign_decode_lamb_stage / k_lamb_onebit_apply): both
// launches take the same arguments.  tensors / adapt / r_frozen / ratio hold num_tensors entries
// in the order of the bucket's tensor table, last_factor two such rows lf_stride entries apart
// (indexed by the step's parity), partials one fp32 per chunk row.
struct SignLambArgs {
  uintptr_t recv, chunks, tensors, stream;
  uintptr_t param, exp_avg, exp_avg_sq, exp_avg_sq_fresh, shadow;  // exp_avg_sq is read only
  uintptr_t adapt, partials, r_frozen, last_factor, ratio;
  long long stride;
  int nranks, num_chunks, num_tensors, lf_stride;
  int scales_off, bits_off;
  double beta1, beta2;
  float lr, inv_n, eps, weight_decay;
  float bc1;   // 1 - beta1^t of the host's t (derived on the device when step is set)
  float bc2w;  // 1 - beta2^freeze_step
  float factor_min, factor_max, factor_threshold;
  int t, freeze_step;  // the host's 1-based step (replaced by *step + 1 when step is set)
  uintptr_t step;      // nullable int32 device step counter
  uintptr_t lr_ptr;    // nullable device fp32 lr (overrides lr)
  uintptr_t key_state;  // see StepArgs; advanced by the apply launch
  uint32_t key_seed, key_rank;
};

struct SignDecodeArgs {
  uintptr_t recv, chunks, stream;
  long long stride;
  int nranks, num_chunks;
  int scales_off, bits_off;
  StepArgs step;
  uintptr_t slots;  // see SignOnebitArgs
  long long slot_end;
  int rotate;  // see SignEncodeArgs: one inverse transform of the summed rows (slots must be 0)
  uint32_t rot_key;
};

// MXFP8 / MXFP4 block floating point with error feedback (mx_codec.hip): scales u8[length / 32] |
// codes u8[length * bits / 8], length = the bucket's padded length.  soft != 0: the conversions in
// software instead of v_cvt_scalef32_pk_* (the same bytes; the tests' cross-check)
struct MxEncodeArgs {
  GradSrc src;
  uintptr_t resid, chunks, payload, stream;  // resid 0: no error feedback
  long long payload_bytes, length;
  int num_tensors, num_chunks;
  int scales_off, codes_off, bits, soft;
};

struct MxDecodeArgs {
  uintptr_t recv, chunks, stream;
  long long stride, length;
  int nranks, num_chunks;
  int scales_off, codes_off, bits, soft;
  StepArgs step;
};

// TernGrad ternary codes with a clipped per-tensor scaler (tern_codec.hip): scales f32[T] | codes
// u32[total_codes / 16], 2 bits per element.  scratch: ew_qsgd_scratch_bytes(T, C) bytes.  clip:
// scale = min(max|x|, clip * rms(x)); 0 = no clipping
struct TernEncodeArgs {
  GradSrc src;
  uintptr_t resid, chunks, tensors, scratch, payload, stream;  // resid 0: no error feedback
  long long payload_bytes, total_codes;
  int num_tensors, num_chunks;
  int scales_off, codes_off;
  float clip;
  uint32_t key, bucket_offset;
  uintptr_t key_ptr;  // nullable device uint32 key (overrides key)
};

struct TernDecodeArgs {
  uintptr_t recv, chunks, tensors, stream;
  long long stride, total_codes;
  int nranks, num_tensors, num_chunks;
  int scales_off, codes_off;
  StepArgs step;
};

// Threshold-search sparsifier (thresh_codec.hip): counts u16[C] | idx u16[total_slots] | values
// f32[total_slots] at counts_off / idx_off / codes_off.  slots: int2 [C] {cap, slot0} per chunk row
// (compress/plan.py thresh_table).  state (nullable int32[C]): the thresholds of the last encode,
// read as the search's starting points and rewritten -- the payload does not depend on it.
// dbg_passes (nullable int32[C], probes): the counting passes every chunk took
struct ThreshEncodeArgs {
  GradSrc src;
  uintptr_t resid, chunks, slots, payload, state, dbg_passes, stream;  // resid 0: no error feedback
  long long payload_bytes, total_slots;
  int num_tensors, num_chunks;
  int counts_off, idx_off, codes_off;
};

struct ThreshDecodeArgs {
  uintptr_t recv, chunks, slots, stream;
  long long stride, total_slots;
  int nranks, num_chunks;
  int counts_off, idx_off, codes_off;
  StepArgs step;
};

// PowerSGD rank-r factors of one bucket (powersgd.hip; compress/plan.py LowRankPlan).  mats /
// dense / items are the plan's device tables; p / q the factor buffers of p_floats / q_floats
// fp32.  The bucket views (grad, resid, param, mom, grad_out, shadow) hold bucket_len elements.
struct PsgdArgs {
  uintptr_t mats, dense, items, stream;
  int rank, num_mats, num_dense, num_items;
  long long bucket_len, p_floats, q_floats;
  uintptr_t grad, resid, p, q;
  // back-project: the row splits' slabs (slab_floats fp32) and the zeroed arrival counters
  uintptr_t slabs, tickets;
  long long slab_floats;
  int num_tickets;
  // orthogonalise / reconstruct: the all-reduce's 1/N; reconstruct: q_out receives q * inv_n
  float inv_n;
  uintptr_t q_out;
  StepArgs step;  // reconstruct only: grad_scale 1, no key advance
};

// Count sketch of one bucket (sketch_codec.hip; compress/plan.py SketchPlan).  rows: int2 [C]
// {start, sketched length (0: a dense tensor's chunk)}; shifts: int32 [R][C] column shifts;
// table: fp32 [R][width].  The bucket views (grad, resid, est) hold bucket_len elements.  The
// gather walks the index sections of a `topk` payload (chunks / tensors: the bucket's DevicePlan
// tables) and overwrites its fp32 values section.
struct SketchArgs {
  uintptr_t rows, shifts, stream;
  int num_chunks, sketch_rows;
  long long width, bucket_len;
  uint32_t sg_key, bucket_offset;
  uintptr_t grad, resid, table, est;
  // gather only
  uintptr_t chunks, tensors, payload;
  long long payload_bytes, total_k, total_idx, total_bm_words;
  int num_tensors, counts_off, idx_off, codes_off, bitmap_off;
};

// IntSGD (intsgd_codec.hip): payload codes i8[length], element i of the padded bucket is byte i.
// state: the model's scale state, 32 bytes = f64 {r, S of the last step} | f32 {alpha, inv_a,
// inv_na} | i32 steps the rule has run.  sat: u32 per chunk row of this bucket, rewritten by
// every encode.  q = floor(127 / world): the clamp of a code
struct IntEncodeArgs {
  GradSrc src;
  uintptr_t resid, chunks, payload, state, sat, stream;  // resid 0: no error feedback
  long long payload_bytes, length;
  int num_tensors, num_chunks, q;
  uint32_t key, bucket_offset;
  uintptr_t key_ptr;  // nullable device uint32 key (overrides key)
};

// The receive side: recv = the summed codes of one bucket (one row).  partials: fp32 per chunk row
// of this bucket, the sum of (p_new - p_old)^2 in k_clip_norm's order.  step: always applies
// (grad_scale must be 1, no grad_out)
struct IntDecodeArgs {
  uintptr_t recv, chunks, state, partials, stream;
  long long length;
  int num_chunks;
  StepArgs step;
};

// The same partials from the bucket's parameters and a previous copy of them
struct IntNormArgs {
  uintptr_t param, prev, chunks, partials, stream;
  long long length;
  int num_chunks;
};

// One block: S = the partials summed in fp64 in index order, r = steps ? beta r + (1 - beta) S : S,
// alpha = fl32(lr sqrt(numel) / sqrt(2 world r + eps2)), inv_a = fl32(1 / alpha), inv_na = fl32(1 /
// (alpha world)) (both 0 when alpha == 0); lr_ptr (nullable device fp32) overrides lr
struct IntAlphaArgs {
  uintptr_t partials, state, lr_ptr, stream;
  int total_chunks, world;
  double numel;
  float lr;
};

struct SgdFlatArgs {
  uintptr_t param, mom, grad, shadow, stream;
  long long n;
  int grad_dtype;  // 0 = fp32, 1 = bf16, 2 = fp16
  float lr, momentum, dampening, weight_decay, grad_scale;
  int nesterov, first;
  uintptr_t lr_ptr;
};

struct AdamFlatArgs {
  uintptr_t param, exp_avg, exp_avg_sq, max_exp_avg_sq, grad, shadow, stream;
  long long n;
  int grad_dtype;
  float lr_step, beta1, beta2, eps, weight_decay, grad_scale, bc2_sqrt;
  int amsgrad;
  uintptr_t step;  // int32 device step counter (nullable: use lr_step as given)
  double lr;       // base lr for the device-side bias correction
  uintptr_t lr_ptr;  // nullable device fp32 base lr (overrides lr)
};

// Lion over a flat range (lion.hip k_lion_flat): the calling shape of AdamFlatArgs; n need not be
// a multiple of 4 (scalar tail)
struct LionFlatArgs {
  uintptr_t param, exp_avg, grad, shadow, stream;
  long long n;
  int grad_dtype;  // 0 = fp32, 1 = bf16, 2 = fp16
  float lr, beta1, beta2, weight_decay, grad_scale;
  uintptr_t lr_ptr;  // nullable device fp32 lr (overrides lr)
};

// Distributed Lion's 1-bit vote (lion.hip): payload = bits u32[256 * C] from bits_off, nothing else.
// Encode: this rank's exp_avg (the bucket's view) is read and rewritten.  step: the 1-based step
// of the exact-zero dither, read as *step_ptr + 1 when step_ptr (int32 device counter) is set.
struct LionEncodeArgs {
  GradSrc src;
  uintptr_t exp_avg, chunks, payload, stream;
  long long payload_bytes;
  int num_tensors, num_chunks;
  int bits_off;
  float beta1, beta2;
  int step, rank;
  uintptr_t step_ptr;
  // slot-addressed form (slots != 0; the two-stage vote's push): int2 per chunk, .y = the byte
  // offset of its 256 words in `payload`, an [N, P] row buffer of payload_bytes bytes (.x, the sign
  // codec's scale offset, is not read); slot_end = the largest offset a slot reaches; bits_off is
  // unused
  uintptr_t slots;
  long long slot_end;
};

// Apply: s = nranks - 2 * (set bits over the rows of recv, stride bytes apart); d = sign(s)
// (average 0) or float(s) * inv_n (average 1); p -= lr * (d + weight_decay * p)
struct LionVoteArgs {
  uintptr_t recv, chunks, param, shadow, stream;
  long long stride;
  int nranks, num_chunks;
  int bits_off;
  float lr, weight_decay, inv_n;
  int average;
  uintptr_t lr_ptr;
  uintptr_t key_state;  // see StepArgs
  uint32_t key_seed, key_rank;
  uintptr_t slots;  // see LionEncodeArgs: recv is the gathered row buffer (stride = its bytes),
  long long slot_end;  // nranks must be 1 and average 0 (d = 1 - 2 * bit)
};

// The two-stage vote's owner step: per element of the owner's shard (num_chunks chunks, words from
// bits_off of every row) s = nranks - 2 * (set bits over the rows of recv, stride bytes apart); the
// bit written to `out` (out_bytes bytes, same layout) is (s < 0) | (s == 0 & the bit of row owner)
struct VoteReduceArgs {
  uintptr_t recv, out, stream;
  long long stride, out_bytes;
  int nranks, owner, num_chunks;
  int bits_off;
};
void ew_lion_flat(const LionFlatArgs& a);
void ew_lion_encode(const LionEncodeArgs& a);
void ew_lion_vote_apply(const LionVoteArgs& a);
void ew_vote_reduce(const VoteReduceArgs& a);

// LARS / LAMB over a flat range (layerwise.hip): chunks / tensors are the range's BucketPlan
// tables; param, grad, state1, state2 and shadow its views.  adapt int32[T] (1: the tensor takes a
// trust ratio), ratio fp32[T] (out), partials fp32[2 * num_chunks] (stage -> apply).
struct LayerwiseArgs {
  uintptr_t param, grad, state1, state2, shadow, chunks, tensors, adapt, partials, ratio, stream;
  int num_chunks;
  int kind;        // 0 = LARS (state1 = momentum buffer), 1 = LAMB (state1 / state2 = exp_avg / _sq)
  int grad_dtype;  // 0 = fp32, 1 = bf16, 2 = fp16
  float lr, beta1, beta2, eps, weight_decay, grad_scale, eta, momentum, dampening;
  float bc1, bc2;  // LAMB: 1 - beta^t of this step (used when step is 0)
  // the betas in double: 1 - beta and 1 - beta^t are formed in double and rounded once, as the
  // oracle's python scalars are
  double beta1d, beta2d;
  int nesterov, first;
  uintptr_t step;    // nullable int32 device step counter: t = *step + 1, first = (*step == 0)
  uintptr_t lr_ptr;  // nullable device fp32 lr (overrides lr)
};
void ew_layerwise_stage(const LayerwiseArgs& a);
void ew_layerwise_apply(const LayerwiseArgs& a);

// Global-norm gradient clipping (clip.hip), one bucket per call: the bucket's gradients through
// the pointer table of pack_grads, its chunk table, and the model-wide partials fp32[total_chunks]
// in which this bucket's rows start at chunk0.  ew_clip_norm of every bucket comes before any
// ew_clip_scale; the scale of the bucket with chunk0 == 0 stores state fp32[2] = {norm, coef}.
struct ClipArgs {
  GradSrc src;
  int num_tensors, num_chunks, chunk0, total_chunks;
  uintptr_t chunks, partials, state, stream;
  float max_norm;
};
void ew_clip_norm(const ClipArgs& a);
void ew_clip_scale(const ClipArgs& a);

// Local SGD's outer optimizer over a flat range (outer.hip k_outer_apply): u = u * mu + delta;
// s = nesterov ? delta + u * mu : u; anchor += lr * s; data = anchor (and its bf16 shadow).  n
// need not be a multiple of 4 (scalar tail).  stats (nullable): fp32 [stats_rows, 2], one row per
// 8192 elements = {sum of delta^2, sum of the new u^2}.
struct OuterArgs {
  uintptr_t anchor, data, momentum, delta, shadow, stats, stream;
  long long n, stats_rows;
  float lr, mu;
  int nesterov;
};
void ew_outer_apply(const OuterArgs& a);

size_t ew_topk_scratch_bytes(int num_tensors, int num_chunks, long long bucket_len,
                             long long total_cap);
std::vector<int> ew_topk_stats(uintptr_t scratch, int num_tensors, int num_chunks);
std::vector<long long> ew_graph_info(uintptr_t graph, const std::string& dot_path);
// largest candidate-block count the fused select kernel takes (0: always three kernels)
int ew_topk_fused_select_max_blocks();
int ew_topk_one_max_blocks();
void ew_flag_signal(uintptr_t flag, uintptr_t stream);
void ew_flag_wait(uintptr_t flag, uintptr_t seen, int need, uintptr_t err, uintptr_t stream);
std::vector<unsigned long long> ew_topk_one_stamps();
int ew_topk_lookback_errors(uintptr_t scratch, int num_tensors, int num_chunks);
void ew_topk_encode(const TopkEncodeArgs& a);
void ew_topk_decode_apply(const TopkDecodeArgs& a);

size_t ew_qsgd_scratch_bytes(int num_tensors, int num_chunks);
void ew_qsgd_encode(const QsgdEncodeArgs& a);
void ew_qsgd_decode_apply(const QsgdDecodeArgs& a);

void ew_sign_encode(const SignEncodeArgs& a);
void ew_sign_decode_apply(const SignDecodeArgs& a);
void ew_mx_encode(const MxEncodeArgs& a);
void ew_mx_decode_apply(const MxDecodeArgs& a);
void ew_tern_encode(const TernEncodeArgs& a);
void ew_tern_decode_apply(const TernDecodeArgs& a);
void ew_thresh_encode(const ThreshEncodeArgs& a);
void ew_thresh_decode_apply(const ThreshDecodeArgs& a);
std::vector<int> ew_thresh_kernel_info();
void ew_sign_decode_onebit(const SignOnebitArgs& a);
void ew_sign_decode_lamb_stage(const SignLambArgs& a);
void ew_lamb_onebit_apply(const SignLambArgs& a);
void ew_sign_reduce_encode(const SignReduceArgs& a);

void ew_psgd_project(const PsgdArgs& a);
void ew_psgd_orth(const PsgdArgs& a);
void ew_psgd_backproject(const PsgdArgs& a);
void ew_psgd_decode_apply(const PsgdArgs& a);
void ew_sketch_stage(const SketchArgs& a);
void ew_sketch_accum(const SketchArgs& a);
void ew_sketch_estimate(const SketchArgs& a);
void ew_sketch_gather(const SketchArgs& a);
int ew_sketch_sum_group();
void ew_int_encode(const IntEncodeArgs& a);
void ew_int_decode_apply(const IntDecodeArgs& a);
void ew_int_update_norm(const IntNormArgs& a);
void ew_int_alpha(const IntAlphaArgs& a);

void ew_sgd_flat(const SgdFlatArgs& a);
void ew_adam_flat(const AdamFlatArgs& a);
// fp32 forward conv GEMMs through LDS-DMA staging (k_cf_gemm_gl) when on (-1: query only);
// returns the previous setting
int ew_cf_set_glds(int on);
int ew_cf_set_inred(int on);
void ew_cf_defer_reduce();
void ew_cf_flush_reduce();
void ew_cf_arm_bn_fin(uintptr_t part, int nblk, int C, long long M, uintptr_t stats, uintptr_t coef,
                      uintptr_t dgamma, uintptr_t dbeta, uintptr_t dcbias, int cb_bf16);
int ew_cf_flush_bn_fin(uintptr_t stream);
void ew_cf_arm_wgout(uintptr_t src, int split, uintptr_t dw, int Nc, int C);
int ew_cf_flush_wgout(uintptr_t stream);
// SGD of one bucket from its per-tensor gradients (pointer table; a.grad / a.n / a.grad_dtype
// unused): param / mom / shadow are the bucket's flat views, chunk rows address them
void ew_sgd_ptrs(const uintptr_t* grad_ptrs, int n_ptrs, const uint32_t* bf16_mask, int n_mask,
                 int num_tensors, uintptr_t chunks, int num_chunks, const SgdFlatArgs& a);
void ew_pack_grads(const uintptr_t* grad_ptrs, int n_ptrs, const uint32_t* bf16_mask, int n_mask,
                   int num_tensors, uintptr_t chunks, int num_chunks, uintptr_t dst,
                   int dst_dtype, float scale, uintptr_t stream);
// dst (bf16 when to_bf16 else fp16) = src * scale
void ew_cast_scale(uintptr_t src, uintptr_t dst, long long n, float scale, int to_bf16,
                   uintptr_t stream);

// ---- model-side kernels (nn.hip) ----
// NHWC BatchNorm + ReLU [+ 2x2 max pool]; h/y/dy/dx bf16 or fp32 ([N,H,W,C] memory), C % 8 == 0
// mode: 0 relu, 2 identity, 3 relu(bn + res) (pool = 1 forces relu + 2x2 pool)
struct BnFwdArgs {
  uintptr_t h, res, y, code, stats, part;        // stats fp32 [4][C]; part: ew_bn_part_floats() floats
  uintptr_t gamma, beta, cbias, rmean, rvar, nbt;  // fp32 [C] (nullable; cbias fp32 or bf16),
  //                                                  nbt int64 (nullable): incremented once
  long long N;
  int H, W, C;
  int is_bf16, pool, training, cb_bf16, mode;
  float momentum, eps;  // momentum < 0: cumulative average over *nbt batches
  uintptr_t stream;
  int pre_nblk;  // > 0: `part` already holds [2][pre_nblk][C] partial sums (skip the stats pass)
  int phase;     // 0: statistics + apply, 1: statistics only (the consumer applies: lazy), 2: apply
};
struct BnBwdArgs {
  uintptr_t h, res, dy, code, stats, coef, part, dx, dres;  // coef fp32 [2][C]
  uintptr_t dgamma, dbeta, dcbias;               // [C] outputs (nullable), dcbias bf16 if cb_bf16
  long long N;
  int H, W, C;  // of h (pre-pool)
  int is_bf16, pool, cb_bf16, mode;
  uintptr_t stream;
  int pre_nblk;  // > 0: `part` already holds [2][pre_nblk][C] sums (sum dz, sum dz*(h-mean))
  int phase;     // 0: statistics + apply, 1: statistics only (coef, dgamma, dbeta), 2: apply
};
// NHWC global average pool: forward x [N, HW, C] -> y [N, C]; backward x = dy [N, C] -> y = dx
// [N, HW, C] (C % 8 == 0)
void ew_gap_nhwc(uintptr_t x, uintptr_t y, long long N, int HW, int C, int is_bf16, int backward,
                 uintptr_t stream);
int ew_bn_part_floats();
void ew_bn_relu_fwd(const BnFwdArgs& a);
void ew_bn_relu_bwd(const BnBwdArgs& a);
void ew_maxpool2_nhwc(uintptr_t x, uintptr_t y, uintptr_t code, long long N, int H, int W, int C,
                      int is_bf16, int backward, uintptr_t stream);
// NHWC 3x3 / stride 2 / pad 1 max pool (C % 8 == 0): forward y + 1-byte tap codes, backward dx
// (x = dy, y = dx) gathered from the windows whose code points at each pixel
void ew_maxpool3s2_nhwc(uintptr_t x, uintptr_t y, uintptr_t code, long long N, int H, int W,
                        int C, int is_bf16, int backward, uintptr_t stream);
// NCHW 2x2 max pool: rows = N*C*H/2
void ew_maxpool2_fwd(uintptr_t x, uintptr_t y, uintptr_t code, long long rows, int W, int is_bf16,
                     uintptr_t stream);
void ew_maxpool2_bwd(uintptr_t dy, uintptr_t code, uintptr_t dx, long long rows, int W,
                     int is_bf16, uintptr_t stream);

// ---- fused input pipeline (data.hip) ----
struct MakeBatchArgs {
  uintptr_t src;     // uint8 [N, C, H, W] dataset
  uintptr_t labels;  // int64 [N]
  uintptr_t perm;    // int64 [>= (pos+1)*B] this rank's sample order for the epoch
  uintptr_t state;   // int64 [2] {pos, epoch}; pos advanced by the kernel
  uintptr_t done;    // uint32 [1] zero-initialised block counter (kernel resets it)
  long long perm_len;
  uintptr_t out, out_y;  // fp32/bf16 [B, C, H, W] (NCHW or channels_last), int64 [B]
  int B, C, H, W, pad, augment, out_bf16, channels_last;
  uint32_t seed, rank;
  float mean[4], inv_std[4];
  uintptr_t stream;
};
void ew_make_batch(const MakeBatchArgs& a);

// ---- 3x3 (pad 1) or 1x1 (pad 0) stride-1 convolution, NHWC bf16, MFMA implicit GEMM (conv.hip) ----
// x [N,H,W,C], w [Nc,k,k,C] (channels_last weight memory), y/dy [N,H,W,Nc]; ws: fp32 split slabs
// (ws_floats of them); ksize 3 or 1
long long ew_conv_ws_floats();
// bnpart (nullable): fp32 [2][rows][Nc] BatchNorm partial sums (sum, sum of squares) of y for the
// BN that follows; returns rows (0 when not written: split-K launch or capacity too small)
int ew_conv_fwd(uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t ws, long long ws_floats,
                long long N, int H, int W, int C, int Nc, int ksize, uintptr_t bnpart,
                long long bnpart_floats, uintptr_t stream);
// bn_h (nullable): also write the BN-backward sums [2][rows][C] (sum dz, sum dz*(h-mean)) of the
// BN(+residual bn_res)(+ReLU)(+pool: bn_code) layer whose output gradient dx is into bnpart;
// returns rows (0: not written).  addend (nullable, [rows][C] bf16): dx = this GEMM + addend.
int ew_conv_bwd_data(uintptr_t dy, uintptr_t w, uintptr_t dx, uintptr_t ws,
                     long long ws_floats, long long N, int H, int W, int C, int Nc, int ksize,
                     uintptr_t bn_h, uintptr_t bn_res, uintptr_t bn_code, uintptr_t bn_stats,
                     int bn_relu, uintptr_t bnpart, long long bnpart_floats, uintptr_t addend,
                     uintptr_t stream);
void ew_conv_wgrad(uintptr_t dy, uintptr_t x, uintptr_t dw, uintptr_t ws, long long ws_floats,
                   long long N, int H, int W, int C, int Nc, int ksize, uintptr_t stream);
// int32 words of a grid arrival ticket (common.h ew_grid_last): 8 sub-counters + 1 top, 128 B apart
#define EW_TICKET_INTS (9 * 32)

// classifier-head Linear (head.hip), bf16 or fp32 (is_f32) tensors: forward z = drop_out(act(drop_in(x) w^T + b)) (+ y = the
// pre-activation), backward dw, db, dx from dz in one launch; dropout = (counter, salt, p)
void ew_head_fwd(uintptr_t x, uintptr_t w, uintptr_t b, uintptr_t z, uintptr_t y, int B, int N,
                 int K, int relu, uintptr_t ctr_in, uint32_t salt_in, float p_in,
                 uintptr_t ctr_out, uint32_t salt_out, float p_out, uintptr_t stream,
                 int is_f32);
void ew_head_fwd_ce(uintptr_t x, uintptr_t w, uintptr_t b, uintptr_t z, int B, int N, int K,
                    uintptr_t yl, uintptr_t lossrow, uintptr_t loss, uintptr_t lse, uintptr_t dlog,
                    uintptr_t tick, uintptr_t stream, int is_f32);
void ew_head_bwd_bn(uintptr_t dz, uintptr_t y, uintptr_t x, uintptr_t w, uintptr_t dx,
                    uintptr_t dw, uintptr_t db, int B, int N, int K, int relu, uintptr_t ctr_out,
                    uint32_t salt_out, float p_out, uintptr_t ctr_in, uint32_t salt_in,
                    float p_in, int advance, uintptr_t bn_h, uintptr_t bn_code,
                    uintptr_t bn_stats, uintptr_t bn_coef, uintptr_t bn_dgamma,
                    uintptr_t bn_dbeta, uintptr_t bn_dcbias, int bn_cb_bf16, uintptr_t bn_tick,
                    uintptr_t stream);
void ew_head_bwd(uintptr_t dz, uintptr_t y, uintptr_t x, uintptr_t w, uintptr_t dx, uintptr_t dw,
                 uintptr_t db, int db_bf16, int B, int N, int K, int relu, uintptr_t ctr_out,
                 uint32_t salt_out, float p_out, uintptr_t ctr_in, uint32_t salt_in, float p_in,
                 int advance, uintptr_t stream, int is_f32);
// stem conv: 3x3 / pad 1 over C = 3 input channels (x [N,H,W,3], w [Nc,3,3,3] channels_last);
// forward returns the BN partial rows written (0: none); wgrad uses ws as its partial slab
int ew_conv_stem_fwd(uintptr_t x, uintptr_t w, uintptr_t y, long long N, int H, int W, int Nc,
                     uintptr_t bnpart, long long bnpart_floats, uintptr_t stream);
void ew_conv_stem_wgrad(uintptr_t dy, uintptr_t x, uintptr_t dw, uintptr_t ws,
                        long long ws_floats, long long N, int H, int W, int Nc, uintptr_t stream);

// ---- the same convolutions in fp32 (conv_f32.hip, v_mfma_f32_16x16x4_f32): fp32 tensors and
// BN operands, same argument meaning as the bf16 entry points above
int ew_conv_f32_fwd(uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t ws, long long ws_floats,
                    long long N, int H, int W, int C, int Nc, int ksize, uintptr_t bnpart,
                    long long bnpart_floats, uintptr_t stream);
int ew_conv_f32_bwd_data(uintptr_t dy, uintptr_t w, uintptr_t dx, uintptr_t ws,
                         long long ws_floats, long long N, int H, int W, int C, int Nc, int ksize,
                         uintptr_t bn_h, uintptr_t bn_res, uintptr_t bn_code, uintptr_t bn_stats,
                         int bn_relu, uintptr_t bnpart, long long bnpart_floats, uintptr_t addend,
                         uintptr_t stream);
void ew_conv_f32_wgrad(uintptr_t dy, uintptr_t x, uintptr_t dw, uintptr_t ws, long long ws_floats,
                       long long N, int H, int W, int C, int Nc, int ksize, uintptr_t stream);
int ew_conv_f32_fwd_lz(uintptr_t h, uintptr_t stats, uintptr_t nbt, uintptr_t w, uintptr_t y,
                       uintptr_t ws, long long ws_floats, long long N, int H, int W, int C, int Nc,
                       uintptr_t bnpart, long long bnpart_floats, uintptr_t stream);
void ew_conv_f32_wgrad_lz(uintptr_t dy, uintptr_t h, uintptr_t stats, uintptr_t dw, uintptr_t ws,
                          long long ws_floats, long long N, int H, int W, int C, int Nc,
                          uintptr_t stream);
// stride-2 3x3 / pad 1 and 1x1 / pad 0 (H, W = the input map, even; y / dy are H/2 x W/2)
int ew_conv_f32_fwd_s2(uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t ws, long long ws_floats,
                       long long N, int H, int W, int C, int Nc, int ksize, uintptr_t bnpart,
                       long long bnpart_floats, uintptr_t stream);
void ew_conv_f32_bwd_data_s2(uintptr_t dy, uintptr_t w, uintptr_t dx, long long N, int H, int W,
                             int C, int Nc, int ksize, uintptr_t addend, uintptr_t stream);
void ew_conv_f32_wgrad_s2(uintptr_t dy, uintptr_t x, uintptr_t dw, uintptr_t ws,
                          long long ws_floats, long long N, int H, int W, int C, int Nc, int ksize,
                          uintptr_t stream);
int ew_conv_f32_stem_fwd(uintptr_t x, uintptr_t w, uintptr_t y, long long N, int H, int W, int Nc,
                         uintptr_t bnpart, long long bnpart_floats, uintptr_t stream);
void ew_conv_f32_stem_wgrad(uintptr_t dy, uintptr_t x, uintptr_t dw, uintptr_t ws,
                            long long ws_floats, long long N, int H, int W, int Nc,
                            uintptr_t stream);
// the same with dy formed from the BatchNorm(+ReLU)(+pool) backward of the stem's output
void ew_conv_f32_stem_wgrad_bn(uintptr_t h, uintptr_t dnext, uintptr_t code, uintptr_t stats,
                               uintptr_t coef, int pool, uintptr_t x, uintptr_t dw, uintptr_t ws,
                               long long ws_floats, long long N, int H, int W, int Nc,
                               uintptr_t stream);
// ---- fp32 3x3 convolutions by Winograd F(m x m, 3x3), m = 2 or 4 (winograd_f32.hip): U[a^2][Nc][C]
// (a = m + 2) from the channels_last weight (standalone, or inside the forward when w != 0);
// forward / backward data over caller-allocated V (a^2 * N*H*W/m^2 * C_in floats) and Mo
// (a^2 * N*H*W/m^2 * C_out floats); return the BN partial rows written (0: none)
void ew_wino_f32_weight(uintptr_t w, uintptr_t U, int Nc, int C, int m, uintptr_t stream);
int ew_wino_f32_fwd(uintptr_t x, uintptr_t w, uintptr_t U, uintptr_t y, uintptr_t V, uintptr_t Mo,
                    long long N, int H, int W, int C, int Nc, int m, uintptr_t bnpart,
                    long long bnpart_floats, uintptr_t stream);
int ew_wino_f32_bwd_data(uintptr_t dy, uintptr_t w, uintptr_t U, uintptr_t dx, uintptr_t V,
                         uintptr_t Mo, long long N, int H, int W, int C, int Nc, int m,
                         uintptr_t bn_h, uintptr_t bn_res, uintptr_t bn_code, uintptr_t bn_stats,
                         int bn_relu, uintptr_t bnpart, long long bnpart_floats,
                         uintptr_t addend, uintptr_t D, uintptr_t wo_src, int wo_split,
                         uintptr_t wo_dw, int wo_Nc, int wo_C, uintptr_t stream);
// the same with the BatchNorm(+ReLU)(+2x2 pool) layer in front applied in the input transform
// (forward; its pool codes written here) / the BatchNorm backward of this conv's output formed
// in the input transform (backward data): winograd_f32.hip WgSrc
int ew_wino_f32_fwd_bn(uintptr_t bn_h, uintptr_t bn_stats, uintptr_t bn_code, uintptr_t nbt,
                       int pool, uintptr_t w, uintptr_t U, uintptr_t y, uintptr_t V,
                       uintptr_t Mo, long long N, int H, int W, int C, int Nc, int m,
                       uintptr_t bnpart, long long bnpart_floats, uintptr_t stream);
int ew_wino_f32_bwd_data_bn(uintptr_t out_h, uintptr_t out_dnext, uintptr_t out_code,
                            uintptr_t out_stats, uintptr_t out_coef, int out_pool, uintptr_t w,
                            uintptr_t U, uintptr_t dx, uintptr_t V, uintptr_t Mo, long long N,
                            int H, int W, int C, int Nc, int m, uintptr_t bn_h, uintptr_t bn_res,
                            uintptr_t bn_code, uintptr_t bn_stats, int bn_relu, uintptr_t bnpart,
                            long long bnpart_floats, uintptr_t addend, uintptr_t D,
                            uintptr_t wo_src, int wo_split, uintptr_t wo_dw, int wo_Nc, int wo_C,
                            uintptr_t stream);
// (wo_*: another layer's deferred weight-gradient output transform riding in the input launch)
int ew_wino_f32_wgrad(uintptr_t dy, uintptr_t V, uintptr_t dw, uintptr_t D, int d_ready,
                      uintptr_t U_scratch, uintptr_t ws, long long ws_floats, long long N, int H,
                      int W, int C, int Nc, int m, int defer_out, uintptr_t stream);
void ew_wino_f32_wgrad_out(uintptr_t src, int split, uintptr_t dw, int Nc, int C, int m,
                           uintptr_t stream);
// the output transform y = A^T Mo A alone, with the forward's (bn_h 0) or the backward-data
// epilogue (tests, probes; any tile count); tpb > 0: that many tiles per block
int ew_wino_f32_output(uintptr_t Mo, uintptr_t y, long long N, int H, int W, int Nc, int m,
                       uintptr_t bn_h, uintptr_t bn_res, uintptr_t bn_code, uintptr_t bn_stats,
                       int bn_relu, uintptr_t bnpart, long long bnpart_floats, uintptr_t addend,
                       int tpb, uintptr_t stream);
// which kernel runs the output transforms (EWDML_WG_OUT_PIPE at load): 0 the general one, 1 the
// pipelined, mode-specialised one (an epilogue without an instance raises), 2 (default) the
// pipelined one for the instances measured faster in a step, the general one otherwise;
// on < 0: query; returns the previous
int ew_wg_set_out_pipe(int on);

// ---- fp32 3x3 convolutions over 2x2 maps as dense position GEMMs (smallmap_f32.hip): slab
// workspace floats and ticket ints (zeroed once; the kernels leave them zero) for N, C, Nc
long long ew_sm_f32_ws_floats(long long N, int C, int Nc);
int ew_sm_set_fence(int on);  // split-K hand-off with fences (1) or write-through (0); returns the previous
long long ew_sm_f32_counters(long long N, int C, int Nc);
int ew_sm_f32_fwd(uintptr_t x, uintptr_t bn_h, uintptr_t bn_stats, uintptr_t nbt, uintptr_t w,
                  uintptr_t y, uintptr_t slab, long long slab_floats, uintptr_t cnt,
                  long long cnt_ints, long long N, int C, int Nc, uintptr_t bnpart,
                  long long bnpart_floats, uintptr_t stream);
int ew_sm_f32_bwd(uintptr_t x, uintptr_t bn_h, uintptr_t bn_stats, uintptr_t dy,
                  uintptr_t out_h, uintptr_t out_dnext, uintptr_t out_code, uintptr_t out_stats,
                  uintptr_t out_coef, int out_pool, uintptr_t w, uintptr_t dx, uintptr_t dw,
                  uintptr_t slab, long long slab_floats, uintptr_t cnt, long long cnt_ints,
                  long long N, int C, int Nc, uintptr_t pb_h, uintptr_t pb_res, uintptr_t pb_code,
                  uintptr_t pb_stats, int pb_relu, uintptr_t bnpart, long long bnpart_floats,
                  uintptr_t fin_coef, uintptr_t fin_dgamma, uintptr_t fin_dbeta,
                  uintptr_t fin_dcbias, int fin_cb_bf16, long long fin_M, uintptr_t stream,
                  uintptr_t st_vel = 0, uintptr_t st_resid = 0, uintptr_t st_param = 0,
                  float st_momentum = 0.0f, float st_damp1 = 1.0f, float st_wd = 0.0f,
                  int st_nesterov = 0, uintptr_t st_lr = 0, uintptr_t st_stamp = 0);

// ---- LeNet's fp32 training step in four launches (lenet_f32.hip): persistent workspace floats
// and ticket ints (zeroed once; the kernels leave them zero) for batch B
long long ew_lenet_ws_floats(int B);
int ew_lenet_counters(int B);
void ew_lenet_set_prof(uintptr_t buf);  // probes: phase stamps of the conv backward (0: off)
void ew_lenet_fwd(uintptr_t x, uintptr_t w1, uintptr_t b1, uintptr_t w2, uintptr_t b2,
                  uintptr_t wf1, uintptr_t bf1, uintptr_t wf2, uintptr_t bf2, uintptr_t y, int B,
                  int K, uintptr_t a1, uintptr_t code1, uintptr_t a2, uintptr_t code2,
                  uintptr_t h1, uintptr_t logits, uintptr_t dlogits, uintptr_t dh1,
                  uintptr_t lossrow, uintptr_t loss, uintptr_t ws, long long ws_floats,
                  uintptr_t cnt, int cnt_ints, uintptr_t stream, uintptr_t bsrc = 0,
                  uintptr_t blabels = 0, uintptr_t bperm = 0, long long bperm_len = 0,
                  uintptr_t bstate = 0, uintptr_t bdone = 0, float bmean = 0.0f,
                  float binv_std = 1.0f);
void ew_lenet_bwd(uintptr_t x, uintptr_t w2, uintptr_t wf1, uintptr_t a1, uintptr_t code1,
                  uintptr_t a2, uintptr_t code2, uintptr_t h1, uintptr_t dlogits, uintptr_t dh1,
                  uintptr_t gscale, int B, int K, uintptr_t dp2, uintptr_t dw1, uintptr_t db1,
                  uintptr_t dw2, uintptr_t db2, uintptr_t dwf1, uintptr_t dbf1, uintptr_t dwf2,
                  uintptr_t dbf2, uintptr_t ws, long long ws_floats, uintptr_t cnt, int cnt_ints,
                  uintptr_t stream);

// ---- VGG classifier tail (fc2 + ReLU + fc3 + cross-entropy) and its backward (head_tail.hip)
long long ew_tail_ws_floats(int B, int N2);
int ew_tail_counters(int B);
void ew_tail_fwd(uintptr_t h1, uintptr_t w2, uintptr_t b2, uintptr_t w3, uintptr_t b3, uintptr_t y,
                 int B, int K1, int N2, int K, uintptr_t h2, uintptr_t logits, uintptr_t dlogits,
                 uintptr_t dh2, uintptr_t lossrow, uintptr_t loss, uintptr_t ws,
                 long long ws_floats, uintptr_t cnt, int cnt_ints, uintptr_t stream);
void ew_tail_bwd(uintptr_t h1, uintptr_t h2, uintptr_t dh2, uintptr_t dlogits, uintptr_t w2,
                 uintptr_t gscale, int B, int K1, int N2, int K, uintptr_t dh1, uintptr_t dw2,
                 uintptr_t db2, uintptr_t dw3, uintptr_t db3, uintptr_t stream);

// ---- RCCL communicator issuing collectives on the caller's stream (rccl_comm.hip) ----
// dtype codes: 0 f32, 1 bf16, 2 f16, 3 u8, 4 i32, 5 f64, 6 i64; op: 0 sum, 1 max, 2 min, 3 avg
std::string ew_rccl_unique_id();
int ew_rccl_version();
uintptr_t ew_rccl_init(const std::string& uid, int nranks, int rank, int device);
void ew_rccl_destroy(uintptr_t h);
void ew_rccl_abort(uintptr_t h);
uintptr_t ew_rccl_watchdog_start(uintptr_t comm, int device, double timeout_s, int exit_code);
void ew_rccl_watch(uintptr_t wd, uintptr_t stream);
int ew_rccl_watch_pending(uintptr_t wd);
void ew_rccl_watchdog_stop(uintptr_t wd);
uintptr_t ew_test_flag_alloc();
void ew_test_flag_free(uintptr_t f);
void ew_watchdog_release_flag(uintptr_t wd, uintptr_t f);
void ew_test_spin(uintptr_t flag, double max_s, uintptr_t stream);
void ew_rccl_all_gather(uintptr_t h, uintptr_t send, uintptr_t recv, long long count, int dtype,
                        uintptr_t stream);
void ew_rccl_all_reduce(uintptr_t h, uintptr_t send, uintptr_t recv, long long count, int dtype,
                        int op, uintptr_t stream);
void ew_rccl_reduce_scatter(uintptr_t h, uintptr_t send, uintptr_t recv, long long count,
                            int dtype, int op, uintptr_t stream);
void ew_rccl_broadcast(uintptr_t h, uintptr_t send, uintptr_t recv, long long count, int dtype,
                       int root, uintptr_t stream);
void ew_rccl_all_to_all(uintptr_t h, uintptr_t send, uintptr_t recv, long long count, int dtype,
                        int nranks, uintptr_t stream);

// ---- cross-entropy loss (nn.hip): mean over B rows of [B, K] logits (bf16 or fp32), int64 labels
void ew_cross_entropy_fwd(uintptr_t x, uintptr_t y, int B, int K, int is_bf16, uintptr_t loss,
                          uintptr_t lse, uintptr_t stream, uintptr_t dx);
void ew_cross_entropy_bwd(uintptr_t x, uintptr_t y, uintptr_t lse, uintptr_t grad, int B, int K,
                          int is_bf16, uintptr_t dx, uintptr_t stream);

// ---- classifier-head activation + dropout (nn.hip), bf16 [rows, C]; ctr int32[2] per layer
void ew_act_dropout_fwd(uintptr_t y, uintptr_t z, int n, float p, int relu, uintptr_t ctr,
                        uint32_t salt, uintptr_t stream);
void ew_act_dropout_bwd(uintptr_t dz, uintptr_t y, uintptr_t dy, uintptr_t db, int db_bf16,
                        int rows, int C, float p, int relu, uintptr_t ctr, uint32_t salt,
                        uintptr_t stream);
