// The outer optimizer of local SGD's model-delta exchange (parallel/local_sgd.py): SlowMo (Wang et
// al. 2020) and BMUF (Chen & Huo 2016) as heavy-ball momentum on the averaged delta, DiLoCo
// (Douillard et al. 2023) as Nesterov momentum.  gfx950, wave64.  compress/oracle.py outer_apply
// defines the arithmetic.
//
// At a sync step the wrapped exchange has left the averaged decoded delta d (under --select-best
// the winner's) in the flat gradient buffer.  One launch, one block per 8192-element row of the
// flat range, fp32 with every operation rounded on its own (-ffp-contract=off):
//
//   u      = u * mu + d
//   s      = d + u * mu      (NESTEROV)      |      s = u
//   anchor = anchor + lr * s
//   data   = anchor          (and the bf16 shadow, rounded to nearest even)
//
// d, u and anchor are read once; u, anchor, data and the shadow are written once: 3 words read
// and 3 + 1/2 written per parameter.  The range is the whole flat buffer, alignment padding
// included: there d = u = 0, so u stays 0 and anchor and data keep their value.
//
// A thread owns elements [4t, 4t + 4) of each of a row's 8 slabs and issues every load of the row
// before it uses one: 16-byte accesses, scalar ones for the last 1..3 elements of the range.
//
// The same launch writes stats[row] = {sum of d^2, sum of the new u^2} over the row, fp32, through
// k_clip_norm's fixed tree (ops.CLIP_SUM_CHAIN = 41: 32 squares per thread in element order into
// a zero accumulator, elements past the range entering as +0, 6 shuffle levels, the four wave sums
// in wave order).  No atomics, no grid barrier; the host sums the rows in fp64 when it logs.
#include "common.h"
#include "ewdml_ops.h"

namespace {

// A row as ew_ld_chunk holds a chunk: thread t's elements [4t, 4t + 4) of each slab, positions
// past len read as 0.
__device__ __forceinline__ void outer_ld_row(const float* __restrict__ src, int len,
                                             float4 (&v)[EW_CU]) {
  if (len == EW_CHUNK) {
#pragma unroll
    for (int k = 0; k < EW_CU; ++k) v[k] = *reinterpret_cast<const float4*>(src + ew_chunk_idx(k));
  } else {  // the last row
#pragma unroll
    for (int k = 0; k < EW_CU; ++k) {
      const int i = ew_chunk_idx(k);
      if (i + 3 < len) {
        v[k] = *reinterpret_cast<const float4*>(src + i);
      } else {
        v[k] = make_float4(i < len ? src[i] : 0.0f, i + 1 < len ? src[i + 1] : 0.0f,
                           i + 2 < len ? src[i + 2] : 0.0f, 0.0f);
      }
    }
  }
}

template <bool NESTEROV>
__device__ __forceinline__ void outer_step(float d, float& u, float& a, float lr, float mu,
                                           float& sd, float& su) {
  u = u * mu + d;
  const float s = NESTEROV ? d + u * mu : u;
  a = a + lr * s;
  sd += d * d;
  su += u * u;
}

// The row's three operands are 96 VGPRs and the kernel takes 129: 3 waves per SIMD, each with 24
// 16-byte loads in flight.  Asking for 4 waves (<= 128 VGPRs) makes the allocator spill to
// scratch, so it is not asked for.
template <bool NESTEROV, bool SHADOW>
__global__ __launch_bounds__(EW_BLOCK) void k_outer_apply(
    const float* __restrict__ delta, float* __restrict__ mom, float* __restrict__ anchor,
    float* __restrict__ data, uint16_t* __restrict__ shadow, long long n, float lr, float mu,
    float* __restrict__ stats) {
  __shared__ float ws[2 * EW_WAVES];
  const long long base = (long long)blockIdx.x * EW_CHUNK;
  const long long rest = n - base;
  const int len = rest < EW_CHUNK ? (int)rest : EW_CHUNK;
  float4 d[EW_CU], u[EW_CU], a[EW_CU];
  outer_ld_row(delta + base, len, d);
  outer_ld_row(mom + base, len, u);
  outer_ld_row(anchor + base, len, a);
  float sd = 0.0f, su = 0.0f;
#pragma unroll
  for (int k = 0; k < EW_CU; ++k) {
    outer_step<NESTEROV>(d[k].x, u[k].x, a[k].x, lr, mu, sd, su);
    outer_step<NESTEROV>(d[k].y, u[k].y, a[k].y, lr, mu, sd, su);
    outer_step<NESTEROV>(d[k].z, u[k].z, a[k].z, lr, mu, sd, su);
    outer_step<NESTEROV>(d[k].w, u[k].w, a[k].w, lr, mu, sd, su);
  }
  ew_st_chunk(mom + base, len, u);
  ew_st_chunk(anchor + base, len, a);
  ew_st_chunk(data + base, len, a);
  if (SHADOW) {
    uint16_t* sh = shadow + base;
#pragma unroll
    for (int k = 0; k < EW_CU; ++k) {
      const int i = ew_chunk_idx(k);
      if (i >= len) continue;
      const float w[4] = {a[k].x, a[k].y, a[k].z, a[k].w};
      ew_st4_bf16(sh + i, len - i, w);
    }
  }
  if (stats) {  // uniform over the grid
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    sd = ew_wave_sum(sd);
    su = ew_wave_sum(su);
    if (lane == 0) {
      ws[w] = sd;
      ws[EW_WAVES + w] = su;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float td = ws[0], tu = ws[EW_WAVES];
#pragma unroll
      for (int i = 1; i < EW_WAVES; ++i) {
        td += ws[i];
        tu += ws[EW_WAVES + i];
      }
      stats[2 * (size_t)blockIdx.x] = td;
      stats[2 * (size_t)blockIdx.x + 1] = tu;
    }
  }
}

}  // namespace

void ew_outer_apply(const OuterArgs& a) {
  if (a.n <= 0 || !a.anchor || !a.data || !a.momentum || !a.delta)
    throw std::runtime_error("ewdml outer: the step needs anchor, data, momentum and the delta");
  const long long rows = (a.n + EW_CHUNK - 1) / EW_CHUNK;
  if (rows > 0x7fffffffLL) throw std::runtime_error("ewdml outer: too many rows for one grid");
  if (a.stats && a.stats_rows < rows)
    throw std::runtime_error("ewdml outer: outer_stats holds " + std::to_string(a.stats_rows) +
                             " rows, the range has " + std::to_string(rows));
  if (!(a.lr > 0.0f) || !(a.lr < INFINITY) || !(a.mu >= 0.0f) || !(a.mu < 1.0f))
    throw std::runtime_error("ewdml outer: lr must be finite and > 0, mu in [0, 1)");
  auto* d = reinterpret_cast<const float*>(a.delta);
  auto* u = reinterpret_cast<float*>(a.momentum);
  auto* an = reinterpret_cast<float*>(a.anchor);
  auto* p = reinterpret_cast<float*>(a.data);
  auto* sh = reinterpret_cast<uint16_t*>(a.shadow);
  auto* st = reinterpret_cast<float*>(a.stats);
#define EW_OUTER(NEST, SHAD)                                                                   \
  hipLaunchKernelGGL((k_outer_apply<NEST, SHAD>), dim3((unsigned)rows), dim3(EW_BLOCK), 0,     \
                     (hipStream_t)a.stream, d, u, an, p, sh, a.n, a.lr, a.mu, st)
  if (a.nesterov) {
    if (sh) EW_OUTER(true, true);
    else EW_OUTER(true, false);
  } else {
    if (sh) EW_OUTER(false, true);
    else EW_OUTER(false, false);
  }
#undef EW_OUTER
  EW_CHECK_LAUNCH();
}
