// pybind11 module `_C` exposing the HIP kernel launchers.  Compiled with g++ (no HIP or torch
// headers needed here); the launchers live in the *.hip translation units built by hipcc.
// The Python wrappers in ops/__init__.py validate tensors and pass raw device pointers and the
// current hipStream_t of torch (so every launch is ordered on, and graph-capturable from, the
// caller's stream).
//
// The codec and optimizer launchers take the argument structs of ewdml_ops.h, bound here as
// classes: Python fills them by field name (ops._args) and each field is named once, below.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <vector>

#include "ewdml_ops.h"

namespace py = pybind11;
using Ptrs = std::vector<uintptr_t>;
using Mask = std::vector<uint32_t>;

// the gradient source of an encode, from the pointer list and bf16 mask of ops.grad_pointers
static GradSrc grad_src(const Ptrs& grads, const Mask& mask) {
  return GradSrc{grads.data(), (int)grads.size(), mask.data(), (int)mask.size()};
}

// f(args, grads, mask) of the entry points that read gradients through the pointer table: `src`
// points into host arrays that must outlive the call, so it is set here and never bound
template <class A, void (*fn)(const A&)>
static void with_grads(A a, const Ptrs& grads, const Mask& mask) {
  a.src = grad_src(grads, mask);
  fn(a);
}

// StepArgs() of Python, and the `step` member of a new decode's arguments: a gradient scale of 1
static StepArgs default_step() {
  StepArgs s{};
  s.grad_scale = 1.0f;
  return s;
}
template <class A>
static A zero_with_step() {
  A a{};
  a.step = default_step();
  return a;
}

// EW_ARGS(T, F(field) ...): class T with T() = T{} (every field zero) and its read/write fields;
// EW_ARGS_STEP: the same for a struct that embeds the receive-side step as `step`
#define F(f) .def_readwrite(#f, &A::f)
#define EW_ARGS(T, ...)                                                 \
  {                                                                     \
    using A = T;                                                        \
    py::class_<A>(m, #T).def(py::init([] { return A{}; })) __VA_ARGS__; \
  }
#define EW_ARGS_STEP(T, ...)                                                   \
  {                                                                            \
    using A = T;                                                               \
    py::class_<A>(m, #T).def(py::init(&zero_with_step<A>)) F(step) __VA_ARGS__; \
  }

PYBIND11_MODULE(_C, m) {
  m.doc() = "ewdml CDNA4 (gfx950) kernels";
  m.attr("arch") = "gfx950";

  {  // the receive-side step of every *_decode_apply and of psgd (ops._step builds it)
    using A = StepArgs;
    const StepArgs d = default_step();
    py::class_<A>(m, "StepArgs")
        .def(py::init([](uintptr_t param, uintptr_t mom, uintptr_t grad_out, uintptr_t shadow,
                         float lr, float momentum, float dampening, float weight_decay,
                         float grad_scale, int nesterov, int first, int apply,
                         uintptr_t key_state, uint32_t key_seed, uint32_t key_rank,
                         uintptr_t lr_ptr) {
               return StepArgs{param, mom, grad_out, shadow, lr, momentum, dampening,
                               weight_decay, grad_scale, nesterov, first, apply, key_state,
                               key_seed, key_rank, lr_ptr};
             }),
             py::arg("param") = 0, py::arg("mom") = 0, py::arg("grad_out") = 0,
             py::arg("shadow") = 0, py::arg("lr") = 0.0f, py::arg("momentum") = 0.0f,
             py::arg("dampening") = 0.0f, py::arg("weight_decay") = 0.0f,
             py::arg("grad_scale") = d.grad_scale, py::arg("nesterov") = 0, py::arg("first") = 0,
             py::arg("apply") = 0, py::arg("key_state") = 0, py::arg("key_seed") = 0,
             py::arg("key_rank") = 0, py::arg("lr_ptr") = 0)
        F(param) F(mom) F(grad_out) F(shadow) F(lr) F(momentum) F(dampening) F(weight_decay)
        F(grad_scale) F(nesterov) F(first) F(apply) F(key_state) F(key_seed) F(key_rank)
        F(lr_ptr);
  }

  EW_ARGS(TopkEncodeArgs,
          F(resid) F(chunks) F(tensors) F(scratch) F(payload) F(stream) F(payload_bytes)
          F(num_tensors) F(num_chunks) F(scales_off) F(counts_off) F(idx_off) F(codes_off)
          F(bitmap_off) F(value_kind) F(norm_l2) F(levels) F(inv_levels) F(key) F(bucket_offset)
          F(key_ptr) F(vel) F(param) F(dgc_momentum) F(dgc_damp1) F(dgc_wd) F(dgc_nesterov)
          F(dgc_mask) F(dgc_lr_ptr) F(bucket_len) F(cblocks) F(num_cblocks) F(predict)
          F(lb_fault) F(max_k) F(apply_param) F(apply_shadow) F(apply_lr_ptr)
          F(apply_key_state) F(apply_lr) F(apply_scale) F(apply_key_seed) F(apply_key_rank)
          F(dgc_stamps) F(apply_mom_set) F(apply_mom) F(apply_momentum) F(apply_dampening)
          F(apply_wd) F(apply_nesterov) F(apply_first))
  EW_ARGS_STEP(TopkDecodeArgs,
               F(recv) F(chunks) F(tensors) F(stream) F(stride) F(nranks) F(num_chunks)
               F(scales_off) F(counts_off) F(idx_off) F(codes_off) F(bitmap_off) F(value_kind)
               F(inv_levels))
  EW_ARGS(QsgdEncodeArgs,
          F(resid) F(chunks) F(tensors) F(scratch) F(payload) F(stream) F(payload_bytes)
          F(num_tensors) F(num_chunks) F(scales_off) F(codes_off) F(bits) F(norm_l2) F(levels)
          F(inv_levels) F(key) F(bucket_offset) F(key_ptr))
  EW_ARGS_STEP(QsgdDecodeArgs,
               F(recv) F(chunks) F(tensors) F(stream) F(stride) F(nranks) F(num_chunks)
               F(scales_off) F(codes_off) F(bits) F(inv_levels))
  EW_ARGS(SignEncodeArgs,
          F(resid) F(chunks) F(payload) F(stream) F(payload_bytes) F(num_tensors) F(num_chunks)
          F(scales_off) F(bits_off) F(mom_exp_avg) F(mom_param) F(mom_beta1) F(mom_wd) F(slots)
          F(slot_end) F(rotate) F(rot_key))
  EW_ARGS(SignReduceArgs,
          F(recv) F(chunks) F(sresid) F(out) F(stream) F(stride) F(out_bytes) F(nranks)
          F(num_chunks) F(scales_off) F(bits_off) F(inv_n))
  EW_ARGS(SignOnebitArgs,
          F(recv) F(chunks) F(param) F(exp_avg) F(exp_avg_sq) F(shadow) F(stream) F(stride)
          F(nranks) F(num_chunks) F(scales_off) F(bits_off) F(lr_step) F(inv_n) F(eps) F(beta1)
          F(beta2) F(freeze_step) F(step) F(lr) F(lr_ptr) F(key_state) F(key_seed) F(key_rank)
          F(slots) F(slot_end))
  EW_ARGS(SignLambArgs,
          F(recv) F(chunks) F(tensors) F(stream) F(param) F(exp_avg) F(exp_avg_sq)
          F(exp_avg_sq_fresh) F(shadow) F(adapt) F(partials) F(r_frozen) F(last_factor) F(ratio)
          F(stride) F(nranks) F(num_chunks) F(num_tensors) F(lf_stride) F(scales_off)
          F(bits_off) F(beta1) F(beta2) F(lr) F(inv_n) F(eps) F(weight_decay) F(bc1) F(bc2w)
          F(factor_min) F(factor_max) F(factor_threshold) F(t) F(freeze_step) F(step) F(lr_ptr)
          F(key_state) F(key_seed) F(key_rank))
  EW_ARGS_STEP(SignDecodeArgs,
               F(recv) F(chunks) F(stream) F(stride) F(nranks) F(num_chunks) F(scales_off)
               F(bits_off) F(slots) F(slot_end) F(rotate) F(rot_key))
  EW_ARGS(MxEncodeArgs,
          F(resid) F(chunks) F(payload) F(stream) F(payload_bytes) F(length) F(num_tensors)
          F(num_chunks) F(scales_off) F(codes_off) F(bits) F(soft))
  EW_ARGS_STEP(MxDecodeArgs,
               F(recv) F(chunks) F(stream) F(stride) F(length) F(nranks) F(num_chunks)
               F(scales_off) F(codes_off) F(bits) F(soft))
  EW_ARGS(TernEncodeArgs,
          F(resid) F(chunks) F(tensors) F(scratch) F(payload) F(stream) F(payload_bytes)
          F(total_codes) F(num_tensors) F(num_chunks) F(scales_off) F(codes_off) F(clip) F(key)
          F(bucket_offset) F(key_ptr))
  EW_ARGS_STEP(TernDecodeArgs,
               F(recv) F(chunks) F(tensors) F(stream) F(stride) F(total_codes) F(nranks)
               F(num_tensors) F(num_chunks) F(scales_off) F(codes_off))
  EW_ARGS(ThreshEncodeArgs,
          F(resid) F(chunks) F(slots) F(payload) F(state) F(dbg_passes) F(stream)
          F(payload_bytes) F(total_slots) F(num_tensors) F(num_chunks) F(counts_off) F(idx_off)
          F(codes_off))
  EW_ARGS_STEP(ThreshDecodeArgs,
               F(recv) F(chunks) F(slots) F(stream) F(stride) F(total_slots) F(nranks)
               F(num_chunks) F(counts_off) F(idx_off) F(codes_off))
  EW_ARGS_STEP(PsgdArgs,
               F(mats) F(dense) F(items) F(stream) F(rank) F(num_mats) F(num_dense) F(num_items)
               F(bucket_len) F(p_floats) F(q_floats) F(grad) F(resid) F(p) F(q) F(slabs)
               F(tickets) F(slab_floats) F(num_tickets) F(inv_n) F(q_out))
  EW_ARGS(SketchArgs,
          F(rows) F(shifts) F(stream) F(num_chunks) F(sketch_rows) F(width) F(bucket_len)
          F(sg_key) F(bucket_offset) F(grad) F(resid) F(table) F(est) F(chunks) F(tensors)
          F(payload) F(payload_bytes) F(total_k) F(total_idx) F(total_bm_words) F(num_tensors)
          F(counts_off) F(idx_off) F(codes_off) F(bitmap_off))
  EW_ARGS(IntEncodeArgs,
          F(resid) F(chunks) F(payload) F(state) F(sat) F(stream) F(payload_bytes) F(length)
          F(num_tensors) F(num_chunks) F(q) F(key) F(bucket_offset) F(key_ptr))
  EW_ARGS_STEP(IntDecodeArgs,
               F(recv) F(chunks) F(state) F(partials) F(stream) F(length) F(num_chunks))
  EW_ARGS(IntNormArgs, F(param) F(prev) F(chunks) F(partials) F(stream) F(length) F(num_chunks))
  EW_ARGS(IntAlphaArgs,
          F(partials) F(state) F(lr_ptr) F(stream) F(total_chunks) F(world) F(numel) F(lr))
  EW_ARGS(SgdFlatArgs,
          F(param) F(mom) F(grad) F(shadow) F(stream) F(n) F(grad_dtype) F(lr) F(momentum)
          F(dampening) F(weight_decay) F(grad_scale) F(nesterov) F(first) F(lr_ptr))
  EW_ARGS(AdamFlatArgs,
          F(param) F(exp_avg) F(exp_avg_sq) F(max_exp_avg_sq) F(grad) F(shadow) F(stream) F(n)
          F(grad_dtype) F(lr_step) F(beta1) F(beta2) F(eps) F(weight_decay) F(grad_scale)
          F(bc2_sqrt) F(amsgrad) F(step) F(lr) F(lr_ptr))
  EW_ARGS(LionFlatArgs,
          F(param) F(exp_avg) F(grad) F(shadow) F(stream) F(n) F(grad_dtype) F(lr) F(beta1)
          F(beta2) F(weight_decay) F(grad_scale) F(lr_ptr))
  EW_ARGS(LionEncodeArgs,
          F(exp_avg) F(chunks) F(payload) F(stream) F(payload_bytes) F(num_tensors)
          F(num_chunks) F(bits_off) F(beta1) F(beta2) F(step) F(rank) F(step_ptr) F(slots)
          F(slot_end))
  EW_ARGS(LionVoteArgs,
          F(recv) F(chunks) F(param) F(shadow) F(stream) F(stride) F(nranks) F(num_chunks)
          F(bits_off) F(lr) F(weight_decay) F(inv_n) F(average) F(lr_ptr) F(key_state)
          F(key_seed) F(key_rank) F(slots) F(slot_end))
  EW_ARGS(VoteReduceArgs,
          F(recv) F(out) F(stream) F(stride) F(out_bytes) F(nranks) F(owner) F(num_chunks)
          F(bits_off))
  EW_ARGS(LayerwiseArgs,
          F(param) F(grad) F(state1) F(state2) F(shadow) F(chunks) F(tensors) F(adapt)
          F(partials) F(ratio) F(stream) F(num_chunks) F(kind) F(grad_dtype) F(lr) F(beta1)
          F(beta2) F(eps) F(weight_decay) F(grad_scale) F(eta) F(momentum) F(dampening) F(bc1)
          F(bc2) F(beta1d) F(beta2d) F(nesterov) F(first) F(step) F(lr_ptr))
  EW_ARGS(ClipArgs,
          F(num_tensors) F(num_chunks) F(chunk0) F(total_chunks) F(chunks) F(partials) F(state)
          F(stream) F(max_norm))
  EW_ARGS(OuterArgs,
          F(anchor) F(data) F(momentum) F(delta) F(shadow) F(stats) F(stream) F(n) F(stats_rows)
          F(lr) F(mu) F(nesterov))

  m.def("topk_scratch_bytes", &ew_topk_scratch_bytes);
  m.def("topk_lookback_errors", &ew_topk_lookback_errors);
  m.def("topk_stats", &ew_topk_stats);
  m.def("graph_info", &ew_graph_info);
  m.def("qsgd_scratch_bytes", &ew_qsgd_scratch_bytes);

  m.def("topk_encode", &with_grads<TopkEncodeArgs, ew_topk_encode>);
  m.def("qsgd_encode", &with_grads<QsgdEncodeArgs, ew_qsgd_encode>);
  m.def("sign_encode", &with_grads<SignEncodeArgs, ew_sign_encode>);
  m.def("mx_encode", &with_grads<MxEncodeArgs, ew_mx_encode>);
  m.def("tern_encode", &with_grads<TernEncodeArgs, ew_tern_encode>);
  m.def("thresh_encode", &with_grads<ThreshEncodeArgs, ew_thresh_encode>);
  m.def("lion_encode", &with_grads<LionEncodeArgs, ew_lion_encode>);
  m.def("int_encode", &with_grads<IntEncodeArgs, ew_int_encode>);
  m.def("clip_norm", &with_grads<ClipArgs, ew_clip_norm>);
  m.def("clip_scale", &with_grads<ClipArgs, ew_clip_scale>);

  m.def("topk_decode_apply", &ew_topk_decode_apply);
  m.def("qsgd_decode_apply", &ew_qsgd_decode_apply);
  m.def("sign_reduce_encode", &ew_sign_reduce_encode);
  m.def("sign_decode_onebit", &ew_sign_decode_onebit);
  m.def("sign_decode_lamb_stage", &ew_sign_decode_lamb_stage);
  m.def("lamb_onebit_apply", &ew_lamb_onebit_apply);
  m.def("sign_decode_apply", &ew_sign_decode_apply);
  m.def("mx_decode_apply", &ew_mx_decode_apply);
  m.def("tern_decode_apply", &ew_tern_decode_apply);
  m.def("thresh_decode_apply", &ew_thresh_decode_apply);
  m.def("thresh_kernel_info", &ew_thresh_kernel_info);
  m.def("psgd_project", &ew_psgd_project);
  m.def("psgd_orth", &ew_psgd_orth);
  m.def("psgd_backproject", &ew_psgd_backproject);
  m.def("psgd_decode_apply", &ew_psgd_decode_apply);
  m.def("sketch_stage", &ew_sketch_stage);
  m.def("sketch_accum", &ew_sketch_accum);
  m.def("sketch_estimate", &ew_sketch_estimate);
  m.def("sketch_gather", &ew_sketch_gather);
  m.def("sketch_sum_group", &ew_sketch_sum_group);
  m.def("int_decode_apply", &ew_int_decode_apply);
  m.def("int_update_norm", &ew_int_update_norm);
  m.def("int_alpha", &ew_int_alpha);
  m.def("sgd_flat", &ew_sgd_flat);
  m.def("adam_flat", &ew_adam_flat);
  m.def("lion_flat", &ew_lion_flat);
  m.def("lion_vote_apply", &ew_lion_vote_apply);
  m.def("vote_reduce", &ew_vote_reduce);
  m.def("layerwise_stage", &ew_layerwise_stage);
  m.def("layerwise_apply", &ew_layerwise_apply);
  m.def("outer_apply", &ew_outer_apply);

  m.def("cast_scale", &ew_cast_scale);

  // these two launchers take the pointer table as raw arrays, not as a GradSrc
  m.def("pack_grads",
        [](const Ptrs& grads, const Mask& mask, int T, uintptr_t chunks, int C, uintptr_t dst,
           int dst_dtype, float scale, uintptr_t stream) {
          ew_pack_grads(grads.data(), (int)grads.size(), mask.data(), (int)mask.size(), T, chunks,
                        C, dst, dst_dtype, scale, stream);
        });

  m.def("sgd_ptrs",
        [](const Ptrs& grads, const Mask& mask, int T, uintptr_t chunks, int C,
           const SgdFlatArgs& a) {
          ew_sgd_ptrs(grads.data(), (int)grads.size(), mask.data(), (int)mask.size(), T, chunks,
                      C, a);
        });

  m.def("cf_set_glds", &ew_cf_set_glds);
  m.def("cf_set_inred", &ew_cf_set_inred);
  m.def("cf_defer_reduce", &ew_cf_defer_reduce);
  m.def("cf_flush_reduce", &ew_cf_flush_reduce);
  m.def("cf_arm_bn_fin", &ew_cf_arm_bn_fin);
  m.def("cf_flush_bn_fin", &ew_cf_flush_bn_fin);
  m.def("cf_arm_wgout", &ew_cf_arm_wgout);
  m.def("cf_flush_wgout", &ew_cf_flush_wgout);
  m.def("bn_part_floats", &ew_bn_part_floats);
  m.def("bn_relu_fwd",
        [](uintptr_t h, uintptr_t res, uintptr_t y, uintptr_t code, uintptr_t stats,
           uintptr_t part, uintptr_t gamma, uintptr_t beta, uintptr_t cbias, uintptr_t rmean,
           uintptr_t rvar, uintptr_t nbt, long long N, int H, int W, int C, int is_bf16,
           int pool, int mode, int training, float momentum, float eps, int cb_bf16,
           uintptr_t stream, int pre_nblk, int phase) {
          BnFwdArgs a{};
          a.pre_nblk = pre_nblk;
          a.phase = phase;
          a.h = h; a.res = res; a.y = y; a.code = code; a.stats = stats; a.part = part;
          a.gamma = gamma; a.beta = beta; a.cbias = cbias; a.rmean = rmean; a.rvar = rvar;
          a.nbt = nbt; a.N = N; a.H = H; a.W = W; a.C = C;
          a.is_bf16 = is_bf16; a.pool = pool; a.mode = mode; a.training = training;
          a.momentum = momentum; a.eps = eps; a.cb_bf16 = cb_bf16; a.stream = stream;
          ew_bn_relu_fwd(a);
        });
  m.def("bn_relu_bwd",
        [](uintptr_t h, uintptr_t res, uintptr_t dy, uintptr_t code, uintptr_t stats,
           uintptr_t coef, uintptr_t part, uintptr_t dx, uintptr_t dres, uintptr_t dgamma,
           uintptr_t dbeta, uintptr_t dcbias, long long N, int H, int W, int C, int is_bf16,
           int pool, int mode, int cb_bf16, uintptr_t stream, int pre_nblk, int phase) {
          BnBwdArgs a{};
          a.phase = phase;
          a.h = h; a.res = res; a.dy = dy; a.code = code; a.stats = stats; a.coef = coef;
          a.part = part; a.dx = dx; a.dres = dres; a.dgamma = dgamma; a.dbeta = dbeta;
          a.dcbias = dcbias; a.N = N; a.H = H; a.W = W; a.C = C; a.is_bf16 = is_bf16;
          a.pool = pool; a.mode = mode; a.cb_bf16 = cb_bf16; a.stream = stream;
          a.pre_nblk = pre_nblk;
          ew_bn_relu_bwd(a);
        });
  m.def("act_dropout_fwd", &ew_act_dropout_fwd);
  m.def("act_dropout_bwd", &ew_act_dropout_bwd);
  m.def("cross_entropy_fwd", &ew_cross_entropy_fwd);
  m.def("cross_entropy_bwd", &ew_cross_entropy_bwd);
  m.def("conv_ws_floats", &ew_conv_ws_floats);
  m.def("conv_fwd", &ew_conv_fwd);
  m.def("conv_bwd_data", &ew_conv_bwd_data);
  m.def("conv_wgrad", &ew_conv_wgrad);
  m.def("conv_stem_fwd", &ew_conv_stem_fwd);
  m.def("head_fwd", &ew_head_fwd);
  m.def("head_fwd_ce", &ew_head_fwd_ce);
  m.def("head_bwd", &ew_head_bwd);
  m.def("head_bwd_bn", &ew_head_bwd_bn);
  m.def("conv_stem_wgrad", &ew_conv_stem_wgrad);
  m.def("rccl_unique_id", [] { return pybind11::bytes(ew_rccl_unique_id()); });
  m.def("rccl_version", &ew_rccl_version);
  m.def("rccl_init", [](pybind11::bytes uid, int nranks, int rank, int device) {
    return ew_rccl_init(std::string(uid), nranks, rank, device);
  });
  m.def("rccl_destroy", &ew_rccl_destroy);
  m.def("rccl_abort", &ew_rccl_abort);
  m.def("rccl_watchdog_start", &ew_rccl_watchdog_start);
  m.def("rccl_watch", &ew_rccl_watch);
  m.def("rccl_watch_pending", &ew_rccl_watch_pending);
  m.def("rccl_watchdog_stop", &ew_rccl_watchdog_stop,
        pybind11::call_guard<pybind11::gil_scoped_release>());
  m.def("test_flag_alloc", &ew_test_flag_alloc);
  m.def("test_flag_free", &ew_test_flag_free);
  m.def("watchdog_release_flag", &ew_watchdog_release_flag);
  m.def("test_spin", &ew_test_spin);
  m.def("rccl_all_gather", &ew_rccl_all_gather);
  m.def("rccl_all_reduce", &ew_rccl_all_reduce);
  m.def("rccl_reduce_scatter", &ew_rccl_reduce_scatter);
  m.def("rccl_broadcast", &ew_rccl_broadcast);
  m.def("rccl_all_to_all", &ew_rccl_all_to_all);
  m.def("conv_f32_fwd", &ew_conv_f32_fwd);
  m.def("conv_f32_bwd_data", &ew_conv_f32_bwd_data);
  m.def("conv_f32_wgrad", &ew_conv_f32_wgrad);
  m.def("conv_f32_fwd_lz", &ew_conv_f32_fwd_lz);
  m.def("conv_f32_wgrad_lz", &ew_conv_f32_wgrad_lz);
  m.def("conv_f32_fwd_s2", &ew_conv_f32_fwd_s2);
  m.def("conv_f32_bwd_data_s2", &ew_conv_f32_bwd_data_s2);
  m.def("conv_f32_wgrad_s2", &ew_conv_f32_wgrad_s2);
  m.def("conv_f32_stem_fwd", &ew_conv_f32_stem_fwd);
  m.def("conv_f32_stem_wgrad", &ew_conv_f32_stem_wgrad);
  m.def("conv_f32_stem_wgrad_bn", &ew_conv_f32_stem_wgrad_bn);
  m.def("wino_f32_weight", &ew_wino_f32_weight);
  m.def("wino_f32_fwd", &ew_wino_f32_fwd);
  m.def("wino_f32_bwd_data", &ew_wino_f32_bwd_data);
  m.def("wino_f32_wgrad", &ew_wino_f32_wgrad);
  m.def("wino_f32_wgrad_out", &ew_wino_f32_wgrad_out);
  m.def("wino_f32_output", &ew_wino_f32_output);
  m.def("wg_set_out_pipe", &ew_wg_set_out_pipe);
  m.def("wino_f32_fwd_bn", &ew_wino_f32_fwd_bn);
  m.def("wino_f32_bwd_data_bn", &ew_wino_f32_bwd_data_bn);
  m.def("sm_f32_ws_floats", &ew_sm_f32_ws_floats);
  m.def("sm_f32_counters", &ew_sm_f32_counters);
  m.def("sm_f32_fwd", &ew_sm_f32_fwd);
  m.def("sm_set_fence", &ew_sm_set_fence);
  m.def("topk_fused_select_max_blocks", &ew_topk_fused_select_max_blocks);
  m.def("topk_one_max_blocks", &ew_topk_one_max_blocks);
  m.def("flag_signal", &ew_flag_signal);
  m.def("flag_wait", &ew_flag_wait);
  m.def("topk_one_stamps", &ew_topk_one_stamps);
  m.def("sm_f32_bwd", &ew_sm_f32_bwd);
  m.def("lenet_ws_floats", &ew_lenet_ws_floats);
  m.def("lenet_counters", &ew_lenet_counters);
  m.def("lenet_set_prof", &ew_lenet_set_prof);
  m.def("lenet_fwd", &ew_lenet_fwd);
  m.def("tail_ws_floats", &ew_tail_ws_floats);
  m.def("tail_counters", &ew_tail_counters);
  m.def("tail_fwd", &ew_tail_fwd);
  m.def("tail_bwd", &ew_tail_bwd);
  m.def("lenet_bwd", &ew_lenet_bwd);
  m.def("maxpool2_nhwc", &ew_maxpool2_nhwc);
  m.def("maxpool3s2_nhwc", &ew_maxpool3s2_nhwc);
  m.def("gap_nhwc", &ew_gap_nhwc);
  m.def("maxpool2_fwd", &ew_maxpool2_fwd);
  m.def("maxpool2_bwd", &ew_maxpool2_bwd);
  m.def("ticket_ints", [] { return EW_TICKET_INTS; });
  m.def("make_batch",
        [](uintptr_t src, uintptr_t labels, uintptr_t perm, long long perm_len, uintptr_t state,
           uintptr_t done, uintptr_t out, uintptr_t out_y, int B, int C, int H, int W, int pad, int augment,
           int out_bf16, int channels_last, uint32_t seed, uint32_t rank,
           const std::vector<float>& mean, const std::vector<float>& inv_std, uintptr_t stream) {
          MakeBatchArgs a{};
          a.src = src; a.labels = labels; a.perm = perm; a.perm_len = perm_len; a.state = state; a.done = done;
          a.out = out; a.out_y = out_y; a.B = B; a.C = C; a.H = H; a.W = W; a.pad = pad;
          a.augment = augment; a.out_bf16 = out_bf16; a.channels_last = channels_last;
          a.seed = seed; a.rank = rank;
          for (int c = 0; c < 4; ++c) {
            a.mean[c] = c < (int)mean.size() ? mean[c] : 0.0f;
            a.inv_std[c] = c < (int)inv_std.size() ? inv_std[c] : 1.0f;
          }
          a.stream = stream;
          ew_make_batch(a);
        });
}
