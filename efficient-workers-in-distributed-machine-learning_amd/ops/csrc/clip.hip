// Global-norm gradient clipping of one rank's local gradient (DGC's local gradient clipping;
// torch.nn.utils.clip_grad_norm_ at a world of one).  gfx950, wave64.  compress/oracle.py
// clip_grad_norm_ defines the arithmetic.
//
// A step is two launches per bucket, one block per 8192-element chunk row of the bucket's plan
// (BucketPlan.chunk_table), every bucket's k_clip_norm before any k_clip_scale:
//
//   k_clip_norm   per chunk, the fp32 partial sum of squares, written into the model-wide
//                 partials[chunk0 + c] (chunk0: the chunks of the buckets before this one);
//   k_clip_scale  every block sums ALL the model's partials in fp64 in a fixed order, forms
//                 norm = (float)sqrt(sum) and coef = fminf(1, C / (norm + 1e-6f)) (all blocks of
//                 all buckets compute the same bits: no grid barrier, no finalize launch), and
//                 unless coef == 1.0f multiplies its chunk row in place by coef (one fp32
//                 multiply; bf16 tensors take the fp32 product rounded to nearest even).  The
//                 first block of the first bucket stores clip_state = {norm, coef}.
//
// The gradients are read and written through the per-tensor pointer table of pack_grads /
// sgd_ptrs (GradPtrs; ops.grad_pointers covers the flat view too), so only a tensor's own
// elements are touched: the alignment padding between tensors is neither read nor written.
// A thread owns elements [4t, 4t + 4) of each of a chunk's 8 slabs: 16-byte accesses for fp32
// tensors, 8-byte ones for bf16, scalar ones for the last 1..3 elements of a tensor.  Tensors
// start 16-byte (bf16: 8-byte) aligned and chunks are 8192 elements, so there is no head.
//
// No float atomics: the sums are a fixed tree, so the result is bitwise reproducible and -- the
// model-wide chunk order being tensor order, then chunk order within the tensor -- does not depend
// on where the buckets are cut.
//
// Chunk reduction, longest chain of fp32 additions L = 41 (ops.CLIP_SUM_CHAIN), k_lw_stage's
// tree: a thread adds its 32 squares in element order into a zero accumulator (32; elements past
// the tensor's end enter as +0, which changes no bit), the wave's shuffle tree has 6 levels, and
// thread 0 adds the four wave sums in wave order (3).
#include "common.h"
#include "ewdml_ops.h"

namespace {

__global__ __launch_bounds__(EW_BLOCK) void k_clip_norm(GradPtrs gp,
                                                        const ChunkRow* __restrict__ chunks,
                                                        float* __restrict__ partials) {
  __shared__ float ws[EW_WAVES];
  const ChunkRow c = chunks[blockIdx.x];
  float4 v[EW_CU];
  ew_ld_chunk(gp, nullptr, c, v);
  float s = 0.0f;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    s += v[u].x * v[u].x; s += v[u].y * v[u].y; s += v[u].z * v[u].z; s += v[u].w * v[u].w;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  s = ew_wave_sum(s);
  if (lane == 0) ws[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = ws[0];
#pragma unroll
    for (int i = 1; i < EW_WAVES; ++i) t += ws[i];
    partials[blockIdx.x] = t;
  }
}

__device__ __forceinline__ double clip_wave_sum_d(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// The model's sum of squares in fp64 and the coefficient, the same bits in every block of every
// bucket: thread i adds partials i, i + 256, ... in order, then the wave tree and the four waves
// in order (k_lw_apply's sum over a tensor's partials, here over the whole model's).
__device__ __forceinline__ float clip_coef(const float* __restrict__ partials, int total,
                                           float max_norm, float* state, double* wd, float* cs) {
  double s = 0.0;
  for (int j = threadIdx.x; j < total; j += EW_BLOCK) s += (double)partials[j];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  s = clip_wave_sum_d(s);
  if (lane == 0) wd[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wd[0];
#pragma unroll
    for (int i = 1; i < EW_WAVES; ++i) t += wd[i];
    const float norm = (float)sqrt(t);
    const float coef = fminf(1.0f, max_norm / (norm + 1e-6f));
    *cs = coef;
    if (state && blockIdx.x == 0) {
      state[0] = norm;
      state[1] = coef;
    }
  }
  __syncthreads();
  return *cs;
}

__global__ __launch_bounds__(EW_BLOCK) void k_clip_scale(GradPtrs gp,
                                                         const ChunkRow* __restrict__ chunks,
                                                         const float* __restrict__ partials,
                                                         int total, float max_norm,
                                                         float* state) {
  __shared__ double wd[EW_WAVES];
  __shared__ float cs;
  const float coef = clip_coef(partials, total, max_norm, state, wd, &cs);
  if (coef == 1.0f) return;  // bitwise the multiply by 1: nothing to move
  const ChunkRow c = chunks[blockIdx.x];
  const size_t off = (size_t)c.local * EW_CHUNK;
  const bool bf = (gp.bf16[c.tensor >> 5] >> (c.tensor & 31)) & 1u;
  void* base = const_cast<void*>(gp.p[c.tensor]);
  if (!bf) {
    float* g = reinterpret_cast<float*>(base) + off;
#pragma unroll 2
    for (int u = 0; u < EW_CU; ++u) {
      const int i = ew_chunk_idx(u);
      if (i >= c.len) break;
      if (i + 3 < c.len) {
        float4 x = *reinterpret_cast<const float4*>(g + i);
        x.x = x.x * coef; x.y = x.y * coef; x.z = x.z * coef; x.w = x.w * coef;
        *reinterpret_cast<float4*>(g + i) = x;
      } else {
        for (int j = 0; i + j < c.len; ++j) g[i + j] = g[i + j] * coef;
      }
    }
  } else {
    uint16_t* g = reinterpret_cast<uint16_t*>(base) + off;
#pragma unroll 2
    for (int u = 0; u < EW_CU; ++u) {
      const int i = ew_chunk_idx(u);
      if (i >= c.len) break;
      if (i + 3 < c.len) {
        const uint2 r = *reinterpret_cast<const uint2*>(g + i);
        const float y[4] = {ew_bf16f(r.x) * coef, ew_bf16f(r.x >> 16) * coef,
                            ew_bf16f(r.y) * coef, ew_bf16f(r.y >> 16) * coef};
        ew_st4_bf16(g + i, 4, y);
      } else {
        for (int j = 0; i + j < c.len; ++j) g[i + j] = ew_f2bf(ew_bf16f(g[i + j]) * coef);
      }
    }
  }
}

void clip_validate(const ClipArgs& a) {
  if (a.num_chunks < 1 || !a.chunks || !a.partials || !a.src.grad_ptrs)
    throw std::runtime_error("ewdml clip: missing operand");
  if (a.chunk0 < 0 || a.total_chunks < 1 || (long long)a.chunk0 + a.num_chunks > a.total_chunks)
    throw std::runtime_error("ewdml clip: the bucket's chunks reach past the model's partials");
}

}  // namespace

void ew_clip_norm(const ClipArgs& a) {
  clip_validate(a);
  GradPtrs g;
  ew_fill_ptrs(g, a.src, a.num_tensors);
  hipLaunchKernelGGL(k_clip_norm, dim3(a.num_chunks), dim3(EW_BLOCK), 0, (hipStream_t)a.stream, g,
                     reinterpret_cast<const ChunkRow*>(a.chunks),
                     reinterpret_cast<float*>(a.partials) + a.chunk0);
  EW_CHECK_LAUNCH();
}

void ew_clip_scale(const ClipArgs& a) {
  clip_validate(a);
  if (!(a.max_norm > 0.0f)) throw std::runtime_error("ewdml clip: max_norm must be > 0");
  GradPtrs g;
  ew_fill_ptrs(g, a.src, a.num_tensors);
  // the first bucket's first block stores clip_state
  float* state = a.chunk0 == 0 ? reinterpret_cast<float*>(a.state) : nullptr;
  if (a.chunk0 == 0 && !state) throw std::runtime_error("ewdml clip: missing clip_state");
  hipLaunchKernelGGL(k_clip_scale, dim3(a.num_chunks), dim3(EW_BLOCK), 0, (hipStream_t)a.stream, g,
                     reinterpret_cast<const ChunkRow*>(a.chunks),
                     reinterpret_cast<const float*>(a.partials), a.total_chunks, a.max_norm,
                     state);
  EW_CHECK_LAUNCH();
}
