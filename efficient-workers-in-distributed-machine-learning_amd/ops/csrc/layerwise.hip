// Layer-wise trust-ratio optimizers over the flat parameter buffer: LARS (You et al., 2017) and
// LAMB (You et al., ICLR 2020).  gfx950, wave64, float4 I/O.  compress/oracle.py lars_apply /
// lamb_apply define the arithmetic.
//
// A step over a flat range (one bucket or the whole model) is two launches, one block per
// 8192-element chunk row of the range's plan (BucketPlan.chunk_table / tensor_table):
//
//   k_lw_stage  per chunk, the two fp32 partial sums of squares partials[c] = {sum p^2, sum x^2}
//               with x = g (LARS) or x = u (LAMB, whose m and v are updated and stored here);
//   k_lw_apply  every block sums its tensor's partials in fp64 in a fixed order, forms the trust
//               ratio r (all blocks of a tensor compute the same r: no grid barrier), applies the
//               step and writes the bf16 shadow; the tensor's first block stores r.
//
// No float atomics: the sums are a fixed tree, so results are bitwise reproducible and do not
// depend on whether a tensor is stepped with its bucket or with the whole model.
//
// Chunk reduction, longest chain of fp32 additions L = 41 (ops.LAYERWISE_SUM_CHAIN): a thread
// adds its 32 squares in element order into a zero accumulator (32), the wave's shuffle tree has
// 6 levels, and thread 0 adds the four wave sums in wave order (3).
#include "common.h"
#include "ewdml_ops.h"

namespace {

struct LwArgs {
  float* p;
  float* s1;  // LARS: momentum buffer; LAMB: exp_avg
  float* s2;  // LAMB: exp_avg_sq
  const void* g;
  uint16_t* shadow;
  const ChunkRow* chunks;
  const TensorRow* tensors;
  const int* adapt;
  float* partials;
  float* ratio;
  const int* step;      // nullable device step counter: t = *step + 1, first = (*step == 0)
  const float* lr_ptr;  // nullable device lr
  float lr, beta1, beta2, eps, weight_decay, grad_scale, eta, momentum, dampening;
  float bc1, bc2;  // LAMB bias corrections 1 - beta^t (host values, replaced when step is set)
  float omb1, omb2;  // 1 - beta, formed in double
  double beta1d, beta2d;
  int nesterov, first;
};

// lr, t and everything derived from them, read once per block from device memory
__device__ __forceinline__ void lw_resolve(LwArgs& a) {
  if (a.lr_ptr) a.lr = *a.lr_ptr;
  if (a.step) {
    const int s = *a.step;
    const double t = (double)(s + 1);
    a.first = s == 0;
    a.bc1 = (float)(1.0 - pow(a.beta1d, t));
    a.bc2 = (float)(1.0 - pow(a.beta2d, t));
  }
}

__device__ __forceinline__ float lw_ld1(const void* g, long long i, int gt) {
  if (gt == 0) return reinterpret_cast<const float*>(g)[i];
  if (gt == 1) return ew_bf16f(reinterpret_cast<const uint16_t*>(g)[i]);
  return __half2float(reinterpret_cast<const __half*>(g)[i]);
}

// LAMB's update direction from the (already updated) moments
__device__ __forceinline__ float lw_lamb_u(float m, float v, float p, const LwArgs& a) {
  float u = (m / a.bc1) / (sqrtf(v / a.bc2) + a.eps);
  if (a.weight_decay != 0.0f) u = u + a.weight_decay * p;
  return u;
}

// one element of the stage pass; returns the value whose square joins the second sum
template <int LAMB>
__device__ __forceinline__ float lw_stage1(float p, float& m, float& v, float raw,
                                           const LwArgs& a) {
  const float g = raw * a.grad_scale;
  if (!LAMB) return g;
  m = m * a.beta1 + a.omb1 * g;
  v = v * a.beta2 + a.omb2 * (g * g);
  return lw_lamb_u(m, v, p, a);
}

template <int LAMB, int GT>
__global__ __launch_bounds__(EW_BLOCK) void k_lw_stage(LwArgs a) {
  __shared__ float ws[2 * EW_WAVES];
  lw_resolve(a);
  const ChunkRow c = a.chunks[blockIdx.x];
  float sp = 0.0f, sx = 0.0f;
#pragma unroll 2
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    if (i >= c.len) break;
    const long long o = (long long)c.start + i;
    if (i + 3 < c.len) {  // 16-byte body
      float gv[4];
      ew_load_grad4<GT>(a.g, o, gv);
      const float4 pv = *reinterpret_cast<const float4*>(a.p + o);
      float4 mv = make_float4(0.f, 0.f, 0.f, 0.f), vv = mv;
      if (LAMB) {
        mv = *reinterpret_cast<const float4*>(a.s1 + o);
        vv = *reinterpret_cast<const float4*>(a.s2 + o);
      }
      const float x0 = lw_stage1<LAMB>(pv.x, mv.x, vv.x, gv[0], a);
      const float x1 = lw_stage1<LAMB>(pv.y, mv.y, vv.y, gv[1], a);
      const float x2 = lw_stage1<LAMB>(pv.z, mv.z, vv.z, gv[2], a);
      const float x3 = lw_stage1<LAMB>(pv.w, mv.w, vv.w, gv[3], a);
      if (LAMB) {
        *reinterpret_cast<float4*>(a.s1 + o) = mv;
        *reinterpret_cast<float4*>(a.s2 + o) = vv;
      }
      sp += pv.x * pv.x; sp += pv.y * pv.y; sp += pv.z * pv.z; sp += pv.w * pv.w;
      sx += x0 * x0; sx += x1 * x1; sx += x2 * x2; sx += x3 * x3;
    } else {  // scalar tail of a tensor's last chunk
      for (int j = 0; i + j < c.len; ++j) {
        const float pv = a.p[o + j];
        float mv = 0.0f, vv = 0.0f;
        if (LAMB) { mv = a.s1[o + j]; vv = a.s2[o + j]; }
        const float x = lw_stage1<LAMB>(pv, mv, vv, lw_ld1(a.g, o + j, GT), a);
        if (LAMB) { a.s1[o + j] = mv; a.s2[o + j] = vv; }
        sp += pv * pv;
        sx += x * x;
      }
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  sp = ew_wave_sum(sp);
  sx = ew_wave_sum(sx);
  if (lane == 0) { ws[w] = sp; ws[EW_WAVES + w] = sx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tp = ws[0], tx = ws[EW_WAVES];
#pragma unroll
    for (int i = 1; i < EW_WAVES; ++i) { tp += ws[i]; tx += ws[EW_WAVES + i]; }
    a.partials[2 * blockIdx.x] = tp;
    a.partials[2 * blockIdx.x + 1] = tx;
  }
}

__device__ __forceinline__ double lw_wave_sum_d(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// The tensor's two sums of squares in fp64 and its trust ratio, the same value in every thread of
// every block of the tensor: thread i adds chunks i, i + 256, ... in order, then the wave tree
// and the four waves in order.
template <int LAMB>
__device__ __forceinline__ float lw_ratio(const LwArgs& a, const ChunkRow& c, double* wd,
                                          float* rs) {
  const TensorRow T = a.tensors[c.tensor];
  double sp = 0.0, sx = 0.0;
  for (int j = threadIdx.x; j < T.nchunks; j += EW_BLOCK) {
    sp += (double)a.partials[2 * (T.chunk0 + j)];
    sx += (double)a.partials[2 * (T.chunk0 + j) + 1];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  sp = lw_wave_sum_d(sp);
  sx = lw_wave_sum_d(sx);
  if (lane == 0) { wd[w] = sp; wd[EW_WAVES + w] = sx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tp = wd[0], tx = wd[EW_WAVES];
#pragma unroll
    for (int i = 1; i < EW_WAVES; ++i) { tp += wd[i]; tx += wd[EW_WAVES + i]; }
    double r = 1.0;
    if (a.adapt[c.tensor] && tp > 0.0 && tx > 0.0) {
      const double pn = sqrt(tp), xn = sqrt(tx);
      r = LAMB ? pn / xn : (double)a.eta * pn / (xn + (double)a.weight_decay * pn);
    }
    *rs = (float)r;
    if (c.local == 0) a.ratio[c.tensor] = (float)r;
  }
  __syncthreads();
  return *rs;
}

__device__ __forceinline__ void lw_lars1(float& p, float& b, float raw, float r, const LwArgs& a,
                                         const SgdArgs& sa) {
  float d = raw * a.grad_scale;
  if (a.weight_decay != 0.0f) d = d + a.weight_decay * p;
  ew_sgd(p, b, r * d, sa);
}

template <int LAMB, int GT>
__global__ __launch_bounds__(EW_BLOCK) void k_lw_apply(LwArgs a) {
  __shared__ double wd[2 * EW_WAVES];
  __shared__ float rs;
  lw_resolve(a);
  const ChunkRow c = a.chunks[blockIdx.x];
  const float r = lw_ratio<LAMB>(a, c, wd, &rs);
  // LARS: the SGD rule on r * (g + wd * p) with its own weight decay off
  SgdArgs sa{a.lr, a.momentum, a.dampening, 0.0f, 1.0f, a.nesterov, a.first};
  const float step = a.lr * r;  // LAMB
  const bool mom = !LAMB && a.momentum != 0.0f;
#pragma unroll 2
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    if (i >= c.len) break;
    const long long o = (long long)c.start + i;
    if (i + 3 < c.len) {
      float4 pv = *reinterpret_cast<const float4*>(a.p + o);
      if (LAMB) {
        const float4 mv = *reinterpret_cast<const float4*>(a.s1 + o);
        const float4 vv = *reinterpret_cast<const float4*>(a.s2 + o);
        pv.x = pv.x - step * lw_lamb_u(mv.x, vv.x, pv.x, a);
        pv.y = pv.y - step * lw_lamb_u(mv.y, vv.y, pv.y, a);
        pv.z = pv.z - step * lw_lamb_u(mv.z, vv.z, pv.z, a);
        pv.w = pv.w - step * lw_lamb_u(mv.w, vv.w, pv.w, a);
      } else {
        float gv[4];
        ew_load_grad4<GT>(a.g, o, gv);
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (mom) bv = *reinterpret_cast<const float4*>(a.s1 + o);
        lw_lars1(pv.x, bv.x, gv[0], r, a, sa);
        lw_lars1(pv.y, bv.y, gv[1], r, a, sa);
        lw_lars1(pv.z, bv.z, gv[2], r, a, sa);
        lw_lars1(pv.w, bv.w, gv[3], r, a, sa);
        if (mom) *reinterpret_cast<float4*>(a.s1 + o) = bv;
      }
      *reinterpret_cast<float4*>(a.p + o) = pv;
      if (a.shadow) {
        const float wv[4] = {pv.x, pv.y, pv.z, pv.w};
        ew_st4_bf16(a.shadow + o, 4, wv);
      }
    } else {
      for (int j = 0; i + j < c.len; ++j) {
        float pv = a.p[o + j];
        if (LAMB) {
          pv = pv - step * lw_lamb_u(a.s1[o + j], a.s2[o + j], pv, a);
        } else {
          float bv = mom ? a.s1[o + j] : 0.0f;
          lw_lars1(pv, bv, lw_ld1(a.g, o + j, GT), r, a, sa);
          if (mom) a.s1[o + j] = bv;
        }
        a.p[o + j] = pv;
        if (a.shadow) a.shadow[o + j] = ew_f2bf(pv);
      }
    }
  }
}

LwArgs lw_args(const LayerwiseArgs& h) {
  LwArgs a{};
  a.p = reinterpret_cast<float*>(h.param);
  a.s1 = reinterpret_cast<float*>(h.state1);
  a.s2 = reinterpret_cast<float*>(h.state2);
  a.g = reinterpret_cast<const void*>(h.grad);
  a.shadow = reinterpret_cast<uint16_t*>(h.shadow);
  a.chunks = reinterpret_cast<const ChunkRow*>(h.chunks);
  a.tensors = reinterpret_cast<const TensorRow*>(h.tensors);
  a.adapt = reinterpret_cast<const int*>(h.adapt);
  a.partials = reinterpret_cast<float*>(h.partials);
  a.ratio = reinterpret_cast<float*>(h.ratio);
  a.step = reinterpret_cast<const int*>(h.step);
  a.lr_ptr = reinterpret_cast<const float*>(h.lr_ptr);
  a.lr = h.lr; a.beta1 = h.beta1; a.beta2 = h.beta2; a.eps = h.eps;
  a.weight_decay = h.weight_decay; a.grad_scale = h.grad_scale; a.eta = h.eta;
  a.momentum = h.momentum; a.dampening = h.dampening;
  a.bc1 = h.bc1; a.bc2 = h.bc2;
  a.beta1d = h.beta1d; a.beta2d = h.beta2d;
  a.omb1 = (float)(1.0 - h.beta1d); a.omb2 = (float)(1.0 - h.beta2d);
  a.nesterov = h.nesterov; a.first = h.first;
  return a;
}

void lw_validate(const LayerwiseArgs& h) {
  if (h.kind < 0 || h.kind > 1 || h.grad_dtype < 0 || h.grad_dtype > 2)
    throw std::runtime_error("ewdml layerwise: unknown rule or gradient dtype");
  if (h.num_chunks < 1 || !h.param || !h.grad || !h.chunks || !h.tensors || !h.adapt ||
      !h.partials || !h.ratio)
    throw std::runtime_error("ewdml layerwise: missing operand");
  if (h.kind == 1 ? (!h.state1 || !h.state2) : (h.momentum != 0.0f && !h.state1))
    throw std::runtime_error("ewdml layerwise: missing optimizer state");
}

}  // namespace

#define LW_LAUNCH(K, LAMB)                                                                      \
  do {                                                                                          \
    const dim3 grid(h.num_chunks), block(EW_BLOCK);                                             \
    hipStream_t s = (hipStream_t)h.stream;                                                      \
    if (h.grad_dtype == 0) hipLaunchKernelGGL((K<LAMB, 0>), grid, block, 0, s, a);              \
    else if (h.grad_dtype == 1) hipLaunchKernelGGL((K<LAMB, 1>), grid, block, 0, s, a);         \
    else hipLaunchKernelGGL((K<LAMB, 2>), grid, block, 0, s, a);                                \
  } while (0)

void ew_layerwise_stage(const LayerwiseArgs& h) {
  lw_validate(h);
  const LwArgs a = lw_args(h);
  if (h.kind == 1) LW_LAUNCH(k_lw_stage, 1);
  else LW_LAUNCH(k_lw_stage, 0);
  EW_CHECK_LAUNCH();
}

void ew_layerwise_apply(const LayerwiseArgs& h) {
  lw_validate(h);
  const LwArgs a = lw_args(h);
  if (h.kind == 1) hipLaunchKernelGGL((k_lw_apply<1, 0>), dim3(h.num_chunks), dim3(EW_BLOCK), 0,
                                      (hipStream_t)h.stream, a);  // LAMB reads no gradient
  else LW_LAUNCH(k_lw_apply, 0);
  EW_CHECK_LAUNCH();
}
