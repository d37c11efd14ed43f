// PowerSGD (Vogels et al., NeurIPS 2019): rank-r factors of the error-compensated gradient
// matrices of one flat bucket, and the fused reconstruct -> residual -> SGD pass.  gfx950, wave64.
//
// A compressed tensor is the row-major matrix M[n, m] at element `off` of the bucket (compress/
// plan.py LowRankPlan); its factors are the [n, R] block of the P buffer and the [m, R] block of
// the Q buffer, R in {1, 2, 4, 8} (a template parameter: the factors of a row live in registers).
// Four launches per bucket and step, each bit-identical from run to run:
//
//   k_psgd_project       M = g + residual (stored into the residual buffer, which holds M until
//                        the last kernel), P = M Q; the dense tensors' gradients go to P's tail
//   -- all-reduce P --
//   k_psgd_orth          P *= 1/N, then modified Gram-Schmidt over P's columns
//   k_psgd_backproject   Q = M^T P
//   -- all-reduce Q --
//   k_psgd_decode_apply  Qa = Q / N (kept as the next warm start), g^ = P Qa^T, residual = M - g^,
//                        the SGD step with g^ (dense tensors: with tail / N)
//
// Summation orders are fixed: a project row is reduced by one wave (every lane adds its elements
// in ascending order -- scalar head, 16-byte body, scalar tail -- then the shuffle tree); a
// back-project column is one thread's sum over the rows of its split in ascending order, and the
// splits' slabs are added in split order by the tile's last-arriving block (agent-scope release /
// acquire around the arrival counter); no floating-point atomics.  g^ is formed as compress/
// oracle.py powersgd_reconstruct_apply writes it -- ((P[i,0] Qa[j,0] + P[i,1] Qa[j,1]) + ...),
// every multiply and add rounded on its own (-ffp-contract=off) -- so the reconstruct pass matches
// the oracle bit for bit.
#include "common.h"
#include "ewdml_ops.h"

namespace {

struct PsgdMat {  // mirrors LowRankPlan.mat_table()
  int off, n, m, p_off, q_off, per, splits, slab_off, tick_off, z0, z1, z2;
};
struct PsgdDense {  // mirrors LowRankPlan.dense_table()
  int off, numel, tail, z;
};
struct PsgdItem {  // mirrors LowRankPlan.row_table() / tile_table()
  int kind, idx, a, b;
};

#define PS_COLS 256  // columns of a back-project / reconstruct tile (plan.PSGD_COLS)
#define PS_U 4       // rows (project: 16-byte groups per lane) in flight per thread

// Row `row` of an [*, R] factor block.  A block starts at a multiple of R floats of a 16-byte
// aligned buffer, so the row is R * 4 bytes aligned.
template <int R>
__device__ __forceinline__ void ps_ldr(const float* __restrict__ f, size_t row, float (&v)[R]) {
  const float* s = f + row * R;
  if (R == 8) {
    const float4 a = *reinterpret_cast<const float4*>(s);
    const float4 b = *reinterpret_cast<const float4*>(s + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4 % R] = b.x; v[5 % R] = b.y; v[6 % R] = b.z; v[7 % R] = b.w;
  } else if (R == 4) {
    const float4 a = *reinterpret_cast<const float4*>(s);
    v[0] = a.x; v[1 % R] = a.y; v[2 % R] = a.z; v[3 % R] = a.w;
  } else if (R == 2) {
    const float2 a = *reinterpret_cast<const float2*>(s);
    v[0] = a.x; v[1 % R] = a.y;
  } else {
    v[0] = s[0];
  }
}

// acc += e * Q[j, :]
template <int R>
__device__ __forceinline__ void ps_axpy(const float* __restrict__ qb, int j, float e,
                                        float (&acc)[R]) {
  float qv[R];
  ps_ldr<R>(qb, (size_t)j, qv);
#pragma unroll
  for (int k = 0; k < R; ++k) acc[k] = acc[k] + e * qv[k];
}

template <int R>
__global__ __launch_bounds__(EW_BLOCK) void k_psgd_project(
    const float* __restrict__ g, float* __restrict__ res, const float* __restrict__ q,
    float* __restrict__ p, const PsgdMat* __restrict__ mats, const PsgdDense* __restrict__ dense,
    const PsgdItem* __restrict__ items) {
  const PsgdItem it = items[blockIdx.x];
  if (it.kind == 1) {  // a dense tensor's gradient, copied behind the P factors
    const PsgdDense d = dense[it.idx];
    const float* src = g + (size_t)d.off + it.a;
    float* dst = p + (size_t)d.tail + it.a;
    for (int i = threadIdx.x; i < it.b; i += EW_BLOCK) dst[i] = src[i];
    return;
  }
  const PsgdMat mt = mats[it.idx];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float* qb = q + mt.q_off;
  for (int row = it.a + w; row < it.a + it.b; row += EW_WAVES) {
    const size_t base = (size_t)mt.off + (size_t)row * mt.m;  // the row's first element
    int head = (int)((4 - (base & 3)) & 3);  // scalar elements up to the next 16-byte boundary
    head = head < mt.m ? head : mt.m;
    const int nb4 = (mt.m - head) >> 2, tail0 = head + 4 * nb4;
    const float* gr = g + base;
    float* rr = res + base;
    float acc[R];
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] = 0.0f;
    if (lane < head) {
      const float e = gr[lane] + rr[lane];
      rr[lane] = e;
      ps_axpy<R>(qb, lane, e, acc);
    }
    for (int v0 = lane; v0 < nb4; v0 += 64 * PS_U) {
      float4 gv[PS_U], rv[PS_U];
#pragma unroll
      for (int u = 0; u < PS_U; ++u) {
        const int v = v0 + 64 * u;
        if (v < nb4) {
          gv[u] = *reinterpret_cast<const float4*>(gr + head + 4 * v);
          rv[u] = *reinterpret_cast<const float4*>(rr + head + 4 * v);
        }
      }
#pragma unroll
      for (int u = 0; u < PS_U; ++u) {
        const int v = v0 + 64 * u;
        if (v < nb4) {
          const int j = head + 4 * v;
          const float4 e = make_float4(gv[u].x + rv[u].x, gv[u].y + rv[u].y, gv[u].z + rv[u].z,
                                       gv[u].w + rv[u].w);
          *reinterpret_cast<float4*>(rr + j) = e;
          ps_axpy<R>(qb, j, e.x, acc);
          ps_axpy<R>(qb, j + 1, e.y, acc);
          ps_axpy<R>(qb, j + 2, e.z, acc);
          ps_axpy<R>(qb, j + 3, e.w, acc);
        }
      }
    }
    if (tail0 + lane < mt.m) {
      const int j = tail0 + lane;
      const float e = gr[j] + rr[j];
      rr[j] = e;
      ps_axpy<R>(qb, j, e, acc);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] = ew_wave_sum(acc[k]);
    if (lane == 0) {
      float* dst = p + (size_t)mt.p_off + (size_t)row * R;
#pragma unroll
      for (int k = 0; k < R; ++k) dst[k] = acc[k];
    }
  }
}

// Block sums of K values in a fixed order (wave trees, then waves 0..3), returned in every thread.
template <int K>
__device__ __forceinline__ void ps_block_sums(float (&v)[K], float (*red)[8]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = ew_wave_sum(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[w][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float s = red[0][k];
#pragma unroll
    for (int i = 1; i < EW_WAVES; ++i) s = s + red[i][k];
    v[k] = s;
  }
  __syncthreads();
}

// One block per matrix: P *= inv_n, then modified Gram-Schmidt over the columns in order with
// col /= (|col| + 1e-8) (compress/oracle.py powersgd_orthogonalize).  Thread t owns rows t, t +
// 256, ...: it is the only reader and writer of them, the column sums cross the block.
template <int R>
__global__ __launch_bounds__(EW_BLOCK) void k_psgd_orth(float* __restrict__ p,
                                                        const PsgdMat* __restrict__ mats,
                                                        float inv_n) {
  __shared__ float red[EW_WAVES][8];
  const PsgdMat mt = mats[blockIdx.x];
  float* P = p + mt.p_off;
  const int n = mt.n, t = threadIdx.x;
  for (int i = t; i < n; i += EW_BLOCK)
#pragma unroll
    for (int k = 0; k < R; ++k) P[(size_t)i * R + k] = P[(size_t)i * R + k] * inv_n;
#pragma unroll
  for (int c = 0; c < R; ++c) {
    float s[1] = {0.0f};
    for (int i = t; i < n; i += EW_BLOCK) {
      const float x = P[(size_t)i * R + c];
      s[0] = s[0] + x * x;
    }
    ps_block_sums<1>(s, red);
    const float den = sqrtf(s[0]) + 1e-8f;
    for (int i = t; i < n; i += EW_BLOCK) P[(size_t)i * R + c] = P[(size_t)i * R + c] / den;
    if (c + 1 < R) {
      float d[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = 0.0f;
      for (int i = t; i < n; i += EW_BLOCK) {
        const float col = P[(size_t)i * R + c];
#pragma unroll
        for (int e = c + 1; e < R; ++e) d[e] = d[e] + col * P[(size_t)i * R + e];
      }
      ps_block_sums<8>(d, red);
      for (int i = t; i < n; i += EW_BLOCK) {
        const float col = P[(size_t)i * R + c];
#pragma unroll
        for (int e = c + 1; e < R; ++e)
          P[(size_t)i * R + e] = P[(size_t)i * R + e] - d[e] * col;
      }
    }
  }
}

// Q[j, :] = sum over i of M[i, j] P[i, :].  One block per (matrix, column tile, row split): thread
// t owns column tile * 256 + t and adds its split's rows in ascending order (the loads of a row
// are coalesced along j; P[i, :] is uniform).  One split: the sums are Q.  Several: every block
// stores its sums into its slab and takes a ticket of the tile's counter; the last to arrive adds
// the slabs in split order.  The slab stores are published by an agent-scope release before the
// ticket and read behind an agent-scope acquire after it; the winner leaves the counter at zero.
template <int R>
__global__ __launch_bounds__(EW_BLOCK) void k_psgd_backproject(
    const float* __restrict__ res, const float* __restrict__ p, float* __restrict__ q,
    float* __restrict__ slabs, int* __restrict__ tickets, const PsgdMat* __restrict__ mats,
    const PsgdItem* __restrict__ items) {
  __shared__ int s_last;
  const PsgdItem it = items[blockIdx.x];
  const PsgdMat mt = mats[it.idx];
  const int j = it.a * PS_COLS + (int)threadIdx.x;
  const bool ok = j < mt.m;
  const int r0 = it.b * mt.per, r1 = min(mt.n, r0 + mt.per);
  const float* P = p + mt.p_off;
  float acc[R];
#pragma unroll
  for (int k = 0; k < R; ++k) acc[k] = 0.0f;
  if (ok) {
    const float* M = res + (size_t)mt.off + j;
    int i = r0;
    for (; i + 2 * PS_U <= r1; i += 2 * PS_U) {
      float mv[2 * PS_U];
#pragma unroll
      for (int u = 0; u < 2 * PS_U; ++u) mv[u] = M[(size_t)(i + u) * mt.m];
#pragma unroll
      for (int u = 0; u < 2 * PS_U; ++u) {
        float pv[R];
        ps_ldr<R>(P, (size_t)(i + u), pv);
#pragma unroll
        for (int k = 0; k < R; ++k) acc[k] = acc[k] + mv[u] * pv[k];
      }
    }
    for (; i < r1; ++i) {
      const float mv = M[(size_t)i * mt.m];
      float pv[R];
      ps_ldr<R>(P, (size_t)i, pv);
#pragma unroll
      for (int k = 0; k < R; ++k) acc[k] = acc[k] + mv * pv[k];
    }
  }
  float* qd = q + (size_t)mt.q_off + (size_t)j * R;
  if (mt.splits == 1) {
    if (ok) {
#pragma unroll
      for (int k = 0; k < R; ++k) qd[k] = acc[k];
    }
    return;
  }
  if (ok) {
    float* sd = slabs + (size_t)mt.slab_off + ((size_t)it.b * mt.m + j) * R;
#pragma unroll
    for (int k = 0; k < R; ++k) sd[k] = acc[k];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int* cnt = tickets + mt.tick_off + it.a;
    const int last =
        __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == mt.splits - 1;
    if (last) {
      __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    s_last = last;
  }
  __syncthreads();
  if (!s_last || !ok) return;
  float s[R];
  ps_ldr<R>(slabs + (size_t)mt.slab_off, (size_t)j, s);
  for (int z = 1; z < mt.splits; ++z) {
    float v[R];
    ps_ldr<R>(slabs + (size_t)mt.slab_off, (size_t)z * mt.m + j, v);
#pragma unroll
    for (int k = 0; k < R; ++k) s[k] = s[k] + v[k];
  }
#pragma unroll
  for (int k = 0; k < R; ++k) qd[k] = s[k];
}

struct PsgdOut {  // the reconstruct pass's destinations (bucket views; nullable but param)
  float* param;
  float* mom;
  float* grad_out;
  uint16_t* shadow;
  int apply;
};

__device__ __forceinline__ void ps_step(const PsgdOut& o, const SgdArgs& sa, size_t e, float gv) {
  if (o.grad_out) o.grad_out[e] = gv;
  if (o.apply) {
    float pv = o.param[e], bv = o.mom ? o.mom[e] : 0.0f;
    ew_sgd(pv, bv, gv, sa);
    o.param[e] = pv;
    if (o.mom) o.mom[e] = bv;
    if (o.shadow) o.shadow[e] = ew_f2bf(pv);
  }
}

// One block per (matrix, column tile, row split) and per dense item.  Thread t keeps Qa[j, :] =
// Q[j, :] * inv_n of its column in registers (the split-0 block of a tile also writes it to q_out)
// and walks the rows of its split: g^ = ((P[i,0] Qa[0] + P[i,1] Qa[1]) + ...), residual = M - g^,
// then the SGD element update with g^ (or only grad_out = g^).
template <int R>
__global__ __launch_bounds__(EW_BLOCK) void k_psgd_decode_apply(
    float* __restrict__ res, const float* __restrict__ p, const float* __restrict__ q,
    float* __restrict__ q_out, float inv_n, PsgdOut o, SgdArgs sa,
    const PsgdMat* __restrict__ mats, const PsgdDense* __restrict__ dense,
    const PsgdItem* __restrict__ items) {
  const PsgdItem it = items[blockIdx.x];
  ew_sgd_resolve(sa);
  if (it.kind == 1) {  // a dense tensor: the averaged gradient from P's tail
    const PsgdDense d = dense[it.idx];
    for (int i = threadIdx.x; i < it.b; i += EW_BLOCK)
      ps_step(o, sa, (size_t)d.off + it.a + i, p[(size_t)d.tail + it.a + i] * inv_n);
    return;
  }
  const PsgdMat mt = mats[it.idx];
  const int j = it.a * PS_COLS + (int)threadIdx.x;
  if (j >= mt.m) return;
  const int r0 = it.b * mt.per, r1 = min(mt.n, r0 + mt.per);
  const float* P = p + mt.p_off;
  float qa[R];
  ps_ldr<R>(q + mt.q_off, (size_t)j, qa);
#pragma unroll
  for (int k = 0; k < R; ++k) qa[k] = qa[k] * inv_n;
  if (it.b == 0) {
    float* qo = q_out + (size_t)mt.q_off + (size_t)j * R;
#pragma unroll
    for (int k = 0; k < R; ++k) qo[k] = qa[k];
  }
  const size_t col = (size_t)mt.off + j;
  for (int i = r0; i < r1; i += PS_U) {
    float mv[PS_U];
#pragma unroll
    for (int u = 0; u < PS_U; ++u)
      if (i + u < r1) mv[u] = res[col + (size_t)(i + u) * mt.m];
#pragma unroll
    for (int u = 0; u < PS_U; ++u) {
      if (i + u < r1) {
        float pv[R];
        ps_ldr<R>(P, (size_t)(i + u), pv);
        float gv = pv[0] * qa[0];
#pragma unroll
        for (int k = 1; k < R; ++k) gv = gv + pv[k] * qa[k];
        const size_t e = col + (size_t)(i + u) * mt.m;
        res[e] = mv[u] - gv;
        ps_step(o, sa, e, gv);
      }
    }
  }
}

void ps_check(const PsgdArgs& a, const char* who, bool need_items) {
  const std::string w = std::string("ewdml powersgd ") + who + ": ";
  if (a.rank != 1 && a.rank != 2 && a.rank != 4 && a.rank != 8)
    throw std::runtime_error(w + "rank must be 1, 2, 4 or 8");
  if (!a.mats || !a.dense || (need_items && (!a.items || a.num_items <= 0)))
    throw std::runtime_error(w + "needs the plan's device tables");
  if (a.num_mats < 0 || a.num_dense < 0 || a.bucket_len <= 0 || a.p_floats <= 0 ||
      a.q_floats < 0 || !a.p)
    throw std::runtime_error(w + "empty bucket or factor buffer");
}

}  // namespace

#define PS_LAUNCH(kern, grid, stream, ...)                                                   \
  do {                                                                                       \
    switch (a.rank) {                                                                        \
      case 1: hipLaunchKernelGGL((kern<1>), dim3(grid), dim3(EW_BLOCK), 0,                   \
                                 (hipStream_t)(stream), __VA_ARGS__); break;                 \
      case 2: hipLaunchKernelGGL((kern<2>), dim3(grid), dim3(EW_BLOCK), 0,                   \
                                 (hipStream_t)(stream), __VA_ARGS__); break;                 \
      case 4: hipLaunchKernelGGL((kern<4>), dim3(grid), dim3(EW_BLOCK), 0,                   \
                                 (hipStream_t)(stream), __VA_ARGS__); break;                 \
      default: hipLaunchKernelGGL((kern<8>), dim3(grid), dim3(EW_BLOCK), 0,                  \
                                  (hipStream_t)(stream), __VA_ARGS__); break;                \
    }                                                                                        \
    EW_CHECK_LAUNCH();                                                                       \
  } while (0)

void ew_psgd_project(const PsgdArgs& a) {
  ps_check(a, "project", true);
  if (!a.grad || !a.resid || (a.num_mats > 0 && !a.q))
    throw std::runtime_error("ewdml powersgd project: needs grad, resid and q");
  PS_LAUNCH(k_psgd_project, a.num_items, a.stream, reinterpret_cast<const float*>(a.grad),
            reinterpret_cast<float*>(a.resid), reinterpret_cast<const float*>(a.q),
            reinterpret_cast<float*>(a.p), reinterpret_cast<const PsgdMat*>(a.mats),
            reinterpret_cast<const PsgdDense*>(a.dense),
            reinterpret_cast<const PsgdItem*>(a.items));
}

void ew_psgd_orth(const PsgdArgs& a) {
  ps_check(a, "orth", false);
  if (a.num_mats == 0) return;
  PS_LAUNCH(k_psgd_orth, a.num_mats, a.stream, reinterpret_cast<float*>(a.p),
            reinterpret_cast<const PsgdMat*>(a.mats), a.inv_n);
}

void ew_psgd_backproject(const PsgdArgs& a) {
  ps_check(a, "backproject", false);
  if (a.num_mats == 0) return;
  if (!a.items || a.num_items <= 0 || !a.resid || !a.q)
    throw std::runtime_error("ewdml powersgd backproject: needs the tile items, resid and q");
  if (a.slab_floats > 0 && (!a.slabs || !a.tickets || a.num_tickets <= 0))
    throw std::runtime_error("ewdml powersgd backproject: row splits need slabs and counters");
  PS_LAUNCH(k_psgd_backproject, a.num_items, a.stream, reinterpret_cast<const float*>(a.resid),
            reinterpret_cast<const float*>(a.p), reinterpret_cast<float*>(a.q),
            reinterpret_cast<float*>(a.slabs), reinterpret_cast<int*>(a.tickets),
            reinterpret_cast<const PsgdMat*>(a.mats), reinterpret_cast<const PsgdItem*>(a.items));
}

void ew_psgd_decode_apply(const PsgdArgs& a) {
  ps_check(a, "decode", true);
  if (!a.resid || (a.num_mats > 0 && (!a.q || !a.q_out)))
    throw std::runtime_error("ewdml powersgd decode: needs resid, q and q_out");
  const StepArgs& st = a.step;
  ew_step_check("ewdml powersgd decode", st, false);
  const SgdArgs sa = ew_sgd_args(st);
  PsgdOut o{reinterpret_cast<float*>(st.param), reinterpret_cast<float*>(st.mom),
            reinterpret_cast<float*>(st.grad_out), reinterpret_cast<uint16_t*>(st.shadow),
            st.apply};
  PS_LAUNCH(k_psgd_decode_apply, a.num_items, a.stream, reinterpret_cast<float*>(a.resid),
            reinterpret_cast<const float*>(a.p), reinterpret_cast<const float*>(a.q),
            reinterpret_cast<float*>(a.q_out), a.inv_n, o, sa,
            reinterpret_cast<const PsgdMat*>(a.mats), reinterpret_cast<const PsgdDense*>(a.dense),
            reinterpret_cast<const PsgdItem*>(a.items));
}
