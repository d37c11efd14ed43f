// Muon (Jordan et al., 2024) over the flat parameter buffer: momentum SGD whose update of every
// weight matrix is the momentum orthogonalised by Newton-Schulz iterations.  gfx950, wave64.
// compress/oracle.py muon_apply / muon_orthogonalize define the arithmetic.
//
// A step over a flat range (one bucket or the whole model) is 1 + 3 * ns_steps launches, whatever
// the number of tensors: every launch walks a work-item list built at plan time (ops.MuonPlan).
//
//   k_muon_momentum  one block per 8192-element chunk row: mom = momentum * mom + g, u = mom (or
//                    g + momentum * mom); a vector takes its momentum-SGD step here (with the bf16
//                    shadow); a matrix writes u into the X workspace and the chunk's sum of
//                    squares of u into partials[chunk] (k_lw_stage's fixed tree);
//   k_muon_gram      A = X X^T, 64 x 64 tiles with j >= i only, mirrored on store.  The long
//                    dimension is cut into slabs of kper columns, one block per (tile, slab); the
//                    tile's last block to arrive adds the slabs in slab order (release / acquire
//                    around an arrival counter, as k_psgd_backproject);
//   k_muon_poly      B = b A + c A A: the same tile walk over A (symmetric, so both operands are
//                    row panels of A), b A in the epilogue;
//   k_muon_update    X' = a X + B X into the other X buffer; on the last iteration the epilogue
//                    is the parameter step p = p (1 - lr wd) - lr sqrt(max(1, n / m)) X' with the
//                    bf16 shadow, and X' is never stored.
//
// X lives in the tensor's own [n, m] layout; the Newton-Schulz orientation [r, c] = [min, max] is
// a pair of strides (rs, cs) in the matrix table, so a tall tensor is read and written through
// strides and never copied.  In iteration 0 X is u, and every load of it applies 1 / (|u| + 1e-7):
// each block sums the tensor's chunk partials in fp64 in a fixed order (lw_ratio's), so all blocks
// hold the same value and the host never reads the norm.
//
// The product: a block of 4 waves owns a 64 x 64 output tile, wave (wr, wc) its 32 x 32 quarter =
// 2 x 2 MFMA tiles.  A 32-deep k-step of both operands (64 rows x 32 k each) is staged in LDS as
// [row][k] with a padded row, double-buffered: the global loads of step s + 1 are issued before
// the MFMAs of step s and stored after them, one barrier per step.  A lane's fragment is 8
// consecutive k of one row (k = 8 * (lane >> 4) ...), the same k permutation in both operands, as
// in head.hip.  T = float: fp32 in LDS, eight v_mfma_f32_16x16x4_f32 per fragment pair (exact
// fp32 products, fp32 accumulation).  T = uint16_t: the staging write rounds to bf16 (nearest
// even), one v_mfma_f32_16x16x32_bf16 per pair; sums, a X, b A and what is stored stay fp32.
// Rows and k past the matrix are loaded as zeros (predicated), nothing is padded in memory.
//
// No float atomics: every sum has a fixed order, so a step is bitwise reproducible.
#include "common.h"
#include "ewdml_ops.h"

namespace {

typedef __bf16 mu_bf16x8 __attribute__((ext_vector_type(8)));
typedef float mu_f32x4 __attribute__((ext_vector_type(4)));
typedef float mu_f32x8 __attribute__((ext_vector_type(8)));
typedef unsigned short mu_u16x8 __attribute__((ext_vector_type(8)));

constexpr int MU_TILE = 64;  // output tile edge (ops.MUON_TILE)
constexpr int MU_K = 32;     // k-step (ops.MUON_K)
constexpr float MU_A = 3.4445f, MU_B = -4.7750f, MU_C = 2.0315f;

struct MuonMat {  // mirrors ops.MuonPlan.mats rows (int32 x 16)
  int off;        // the tensor's offset in the flat range
  int n, m;       // its own shape [n, m]
  int r, c;       // min / max of them: the Newton-Schulz orientation [r, c]
  int rs, cs;     // X(i, k) of that orientation = x[i * rs + k * cs]
  int x_off;      // offset in both X workspaces (multiple of 4)
  int a_off;      // offset of the r x r matrices in the A and B workspaces
  int slab_off;   // gram slabs: [tile][slab][4096] floats (splits > 1)
  int tick_off;   // arrival counters, one per upper tile (splits > 1)
  int splits, kper;  // slabs of the long dimension and their length (a multiple of MU_K)
  int part0, nparts;  // the tensor's rows in the chunk partials
  int pad;
};
struct MuonItem {  // mirrors ops.MuonPlan work lists (int32 x 6)
  int mat, ti, tj, slab, tile, pad;
};

struct MuArgs {
  const MuonMat* mats;
  const MuonItem* items;
  const float* xin;
  float* xout;
  float* A;
  float* B;
  float* slabs;
  int* tickets;
  const float* partials;
  float* param;
  uint16_t* shadow;
  const float* lr_ptr;
  float lr, weight_decay;
  int first, last;
};

template <typename T>
struct MuT;
template <>
struct MuT<float> {
  typedef float E;
  typedef mu_f32x8 v8;
  static constexpr int LD = MU_K + 4;  // padded LDS row, in elements (16-byte multiples)
  __device__ static __forceinline__ void st8(E* d, const float (&v)[8]) {
    *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
  __device__ static __forceinline__ v8 ld8(const E* s) {
    const float4 lo = *reinterpret_cast<const float4*>(s);
    const float4 hi = *reinterpret_cast<const float4*>(s + 4);
    v8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return v;
  }
  __device__ static __forceinline__ mu_f32x4 mma(const v8& a, const v8& b, mu_f32x4 acc) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc, 0, 0, 0);
    return acc;
  }
};
template <>
struct MuT<uint16_t> {
  typedef uint16_t E;
  typedef mu_u16x8 v8;
  static constexpr int LD = MU_K + 8;
  __device__ static __forceinline__ void st8(E* d, const float (&v)[8]) {
    uint4 o;
    o.x = (uint32_t)ew_f2bf(v[0]) | ((uint32_t)ew_f2bf(v[1]) << 16);
    o.y = (uint32_t)ew_f2bf(v[2]) | ((uint32_t)ew_f2bf(v[3]) << 16);
    o.z = (uint32_t)ew_f2bf(v[4]) | ((uint32_t)ew_f2bf(v[5]) << 16);
    o.w = (uint32_t)ew_f2bf(v[6]) | ((uint32_t)ew_f2bf(v[7]) << 16);
    *reinterpret_cast<uint4*>(d) = o;
  }
  __device__ static __forceinline__ v8 ld8(const E* s) {
    return __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(s));
  }
  __device__ static __forceinline__ mu_f32x4 mma(const v8& a, const v8& b, mu_f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mu_bf16x8, a),
                                                   __builtin_bit_cast(mu_bf16x8, b), acc, 0, 0, 0);
  }
};

// One operand of a product: element (row, k) = base[row * rs + k * cs] * scale for row < rows and
// k < kend, zero outside.
struct MuSrc {
  const float* base;
  long long rs, cs;
  int rows;
  float scale;
};

// This thread's 8 consecutive k of one row of a 64 x 32 operand tile.  With k contiguous in
// memory a thread takes 8 neighbours of a row (two 16-byte loads when aligned and whole), else
// the 64 rows run across the threads so that a wave's loads of one k are contiguous.
__device__ __forceinline__ void mu_tile_pos(const MuSrc& s, int& row, int& kk) {
  const int t = threadIdx.x;
  if (s.cs == 1) { row = t >> 2; kk = (t & 3) * 8; }
  else { row = t & 63; kk = (t >> 6) * 8; }
}
__device__ __forceinline__ void mu_load8(const MuSrc& s, int grow, int gk, int kend,
                                         float (&v)[8]) {
  const bool rok = grow < s.rows;
  const float* p = s.base + (long long)grow * s.rs + (long long)gk * s.cs;
  if (rok && s.cs == 1 && gk + 8 <= kend && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const float4 lo = *reinterpret_cast<const float4*>(p);
    const float4 hi = *reinterpret_cast<const float4*>(p + 4);
    v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
    v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (rok && gk + j < kend) ? p[(long long)j * s.cs] : 0.0f;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = v[j] * s.scale;
}

// acc[fa][fb] += the 64 x 64 tile (rows arow0.. of `a`) x (rows brow0.. of `b`)^T over k in
// [kbeg, kend).  acc[fa][fb][q] is element (32 wr + 16 fa + 4 (lane >> 4) + q, 32 wc + 16 fb +
// (lane & 15)) of the tile.
template <typename T>
__device__ __forceinline__ void mu_gemm(const MuSrc& a, int arow0, const MuSrc& b, int brow0,
                                        int kbeg, int kend, mu_f32x4 (&acc)[2][2]) {
  using H = MuT<T>;
  typedef typename H::E E;
  typedef typename H::v8 v8;
  __shared__ __attribute__((aligned(16))) E lds[2][2][MU_TILE * H::LD];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  int ar, ak, br, bk;
  mu_tile_pos(a, ar, ak);
  mu_tile_pos(b, br, bk);
  const int steps = (kend - kbeg + MU_K - 1) / MU_K;
  float va[8], vb[8];
  mu_load8(a, arow0 + ar, kbeg + ak, kend, va);
  mu_load8(b, brow0 + br, kbeg + bk, kend, vb);
  H::st8(&lds[0][0][ar * H::LD + ak], va);
  H::st8(&lds[0][1][br * H::LD + bk], vb);
  __syncthreads();
  const int fo = (lane & 15) * H::LD + 8 * (lane >> 4);
  for (int s = 0; s < steps; ++s) {
    const int cur = s & 1;
    const bool more = s + 1 < steps;
    if (more) {
      const int k0 = kbeg + (s + 1) * MU_K;
      mu_load8(a, arow0 + ar, k0 + ak, kend, va);
      mu_load8(b, brow0 + br, k0 + bk, kend, vb);
    }
    v8 fa[2], fb[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      fa[f] = H::ld8(&lds[cur][0][(32 * wr + 16 * f) * H::LD + fo]);
      fb[f] = H::ld8(&lds[cur][1][(32 * wc + 16 * f) * H::LD + fo]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = H::mma(fa[i], fb[j], acc[i][j]);
    if (more) {
      H::st8(&lds[cur ^ 1][0][ar * H::LD + ak], va);
      H::st8(&lds[cur ^ 1][1][br * H::LD + bk], vb);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ double mu_wave_sum_d(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// 1 / (|u|_F + 1e-7) of a matrix from its chunk partials, the same value in every thread of every
// block: thread i adds partials i, i + 256, ... in fp64 in order, then the wave tree and the four
// waves in order.
__device__ __forceinline__ float mu_inv_norm(const float* partials, const MuonMat& mt) {
  __shared__ double wd[EW_WAVES];
  __shared__ float inv;
  double s = 0.0;
  for (int j = threadIdx.x; j < mt.nparts; j += EW_BLOCK) s += (double)partials[mt.part0 + j];
  s = mu_wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) wd[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wd[0];
#pragma unroll
    for (int i = 1; i < EW_WAVES; ++i) t += wd[i];
    inv = (float)(1.0 / (sqrt(t) + 1e-7));
  }
  __syncthreads();
  return inv;
}

// A = X X^T (POLY 0) or B = b A + c A A (POLY 1): one block per upper tile (and slab).
template <typename T, int POLY>
__global__ __launch_bounds__(EW_BLOCK) void k_muon_syrk(MuArgs a) {
  __shared__ int s_last;
  const MuonItem it = a.items[blockIdx.x];
  const MuonMat mt = a.mats[it.mat];
  const int r = mt.r;
  const float* Ain = a.A + mt.a_off;
  MuSrc src;
  int kbeg = 0, kend = r;
  if (POLY) {
    src = MuSrc{Ain, r, 1, r, 1.0f};
  } else {
    const float scale = a.first ? mu_inv_norm(a.partials, mt) : 1.0f;
    src = MuSrc{a.xin + mt.x_off, mt.rs, mt.cs, r, scale};
    kbeg = it.slab * mt.kper;
    kend = min(mt.c, kbeg + mt.kper);
  }
  mu_f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = mu_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  mu_gemm<T>(src, it.ti * MU_TILE, src, it.tj * MU_TILE, kbeg, kend, acc);

  const int t = threadIdx.x;
  if (!POLY && mt.splits > 1) {
    float* tile = a.slabs + (size_t)mt.slab_off + (size_t)it.tile * mt.splits * (MU_TILE * MU_TILE);
    float* mine = tile + (size_t)it.slab * (MU_TILE * MU_TILE);
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int q = 0; q < 4; ++q) mine[(f * 4 + q) * EW_BLOCK + t] = acc[f >> 1][f & 1][q];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      int* cnt = a.tickets + mt.tick_off + it.tile;
      const int last = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT) == mt.splits - 1;
      if (last) {
        __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float* p = tile + (f * 4 + q) * EW_BLOCK + t;
        float s = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int z = 1; z < mt.splits; ++z)
          s = s + __hip_atomic_load(p + (size_t)z * (MU_TILE * MU_TILE), __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
        acc[f >> 1][f & 1][q] = s;
      }
  }
  float* out = (POLY ? a.B : a.A) + mt.a_off;
  const int lane = t & 63, wv = t >> 6;
  const int i0 = it.ti * MU_TILE + 32 * (wv >> 1) + 4 * (lane >> 4);
  const int j0 = it.tj * MU_TILE + 32 * (wv & 1) + (lane & 15);
#pragma unroll
  for (int fa = 0; fa < 2; ++fa)
#pragma unroll
    for (int fb = 0; fb < 2; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + 16 * fa + q, j = j0 + 16 * fb;
        if (i >= r || j >= r) continue;
        float v = acc[fa][fb][q];
        if (POLY) v = MU_B * Ain[(size_t)i * r + j] + MU_C * v;
        out[(size_t)i * r + j] = v;
        if (it.ti != it.tj) out[(size_t)j * r + i] = v;
      }
}

// X' = a X + B X, or on the last iteration the parameter step with X' = O.
template <typename T>
__global__ __launch_bounds__(EW_BLOCK) void k_muon_update(MuArgs a) {
  const MuonItem it = a.items[blockIdx.x];
  const MuonMat mt = a.mats[it.mat];
  const int r = mt.r, c = mt.c;
  const float scale = a.first ? mu_inv_norm(a.partials, mt) : 1.0f;
  const float* X = a.xin + mt.x_off;
  const MuSrc bsrc{a.B + mt.a_off, r, 1, r, 1.0f};
  const MuSrc xsrc{X, mt.cs, mt.rs, c, scale};  // rows = the output's columns, k runs over r
  mu_f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = mu_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  mu_gemm<T>(bsrc, it.ti * MU_TILE, xsrc, it.tj * MU_TILE, 0, r, acc);

  const float lr = a.lr_ptr ? *a.lr_ptr : a.lr;
  const float decay = 1.0f - lr * a.weight_decay;
  const float step = lr * sqrtf(fmaxf(1.0f, (float)mt.n / (float)mt.m));
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i0 = it.ti * MU_TILE + 32 * (wv >> 1) + 4 * (lane >> 4);
  const int j0 = it.tj * MU_TILE + 32 * (wv & 1) + (lane & 15);
#pragma unroll
  for (int fa = 0; fa < 2; ++fa)
#pragma unroll
    for (int fb = 0; fb < 2; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + 16 * fa + q, k = j0 + 16 * fb;
        if (i >= r || k >= c) continue;
        const size_t e = (size_t)i * mt.rs + (size_t)k * mt.cs;
        const float v = MU_A * (X[e] * scale) + acc[fa][fb][q];
        if (!a.last) {
          a.xout[(size_t)mt.x_off + e] = v;
        } else {
          const size_t pe = (size_t)mt.off + e;
          const float pv = a.param[pe] * decay - step * v;
          a.param[pe] = pv;
          if (a.shadow) a.shadow[pe] = ew_f2bf(pv);
        }
      }
}

struct MuMomArgs {
  float* p;
  float* mom;
  const void* g;
  uint16_t* shadow;
  const ChunkRow* chunks;
  const int* xoff;  // per tensor: its offset in the X workspace, -1 for a vector
  float* x;
  float* partials;
  const float* lr_ptr;
  float lr, aux_ratio, momentum, weight_decay, grad_scale;
  int nesterov;
};

// one element: the momentum update; returns u.  A vector (!mat) also takes its step.
__device__ __forceinline__ float mu_mom1(float& p, float& m, float raw, bool mat, float lr_aux,
                                         const MuMomArgs& a) {
  const float g = raw * a.grad_scale;
  m = m * a.momentum + g;
  const float u = a.nesterov ? g + m * a.momentum : m;
  if (!mat) {
    float d = u;
    if (a.weight_decay != 0.0f) d = u + p * a.weight_decay;
    p = p - d * lr_aux;
  }
  return u;
}

template <int GT>
__global__ __launch_bounds__(EW_BLOCK) void k_muon_momentum(MuMomArgs a) {
  __shared__ float ws[EW_WAVES];
  const float lr_aux = (a.lr_ptr ? *a.lr_ptr : a.lr) * a.aux_ratio;
  const ChunkRow c = a.chunks[blockIdx.x];
  const int xo = a.xoff[c.tensor];
  const bool mat = xo >= 0;
  float* xd = a.x + (mat ? (size_t)xo + (size_t)c.local * EW_CHUNK : 0);
  float sx = 0.0f;
#pragma unroll 2
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    if (i >= c.len) break;
    const long long o = (long long)c.start + i;
    if (i + 3 < c.len) {  // 16-byte body
      float gv[4];
      ew_load_grad4<GT>(a.g, o, gv);
      float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!mat) pv = *reinterpret_cast<const float4*>(a.p + o);
      float4 mv = *reinterpret_cast<const float4*>(a.mom + o);
      float4 uv;
      uv.x = mu_mom1(pv.x, mv.x, gv[0], mat, lr_aux, a);
      uv.y = mu_mom1(pv.y, mv.y, gv[1], mat, lr_aux, a);
      uv.z = mu_mom1(pv.z, mv.z, gv[2], mat, lr_aux, a);
      uv.w = mu_mom1(pv.w, mv.w, gv[3], mat, lr_aux, a);
      *reinterpret_cast<float4*>(a.mom + o) = mv;
      if (mat) {
        *reinterpret_cast<float4*>(xd + i) = uv;
        sx += uv.x * uv.x; sx += uv.y * uv.y; sx += uv.z * uv.z; sx += uv.w * uv.w;
      } else {
        *reinterpret_cast<float4*>(a.p + o) = pv;
        if (a.shadow) {
          const float wv[4] = {pv.x, pv.y, pv.z, pv.w};
          ew_st4_bf16(a.shadow + o, 4, wv);
        }
      }
    } else {  // scalar tail of a tensor's last chunk
      for (int j = 0; i + j < c.len; ++j) {
        float pv = mat ? 0.0f : a.p[o + j];
        float mv = a.mom[o + j];
        float raw;
        if (GT == 0) raw = reinterpret_cast<const float*>(a.g)[o + j];
        else if (GT == 1) raw = ew_bf16f(reinterpret_cast<const uint16_t*>(a.g)[o + j]);
        else raw = __half2float(reinterpret_cast<const __half*>(a.g)[o + j]);
        const float uv = mu_mom1(pv, mv, raw, mat, lr_aux, a);
        a.mom[o + j] = mv;
        if (mat) {
          xd[i + j] = uv;
          sx += uv * uv;
        } else {
          a.p[o + j] = pv;
          if (a.shadow) a.shadow[o + j] = ew_f2bf(pv);
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  sx = ew_wave_sum(sx);
  if (lane == 0) ws[w] = sx;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tx = ws[0];
#pragma unroll
    for (int i = 1; i < EW_WAVES; ++i) tx += ws[i];
    a.partials[blockIdx.x] = tx;
  }
}

MuArgs mu_args(const MuonArgs& h) {
  if (h.num_items < 1 || !h.mats || !h.items || !h.x_in || !h.a_buf || !h.b_buf || !h.partials)
    throw std::runtime_error("ewdml muon: missing operand");
  if (h.ns_bf16 < 0 || h.ns_bf16 > 1)
    throw std::runtime_error("ewdml muon: unknown Newton-Schulz dtype");
  if ((h.x_in | h.x_out | h.a_buf | h.b_buf | h.slabs | h.param) % 16 || h.shadow % 2 ||
      (h.tickets | h.partials | h.lr_ptr) % 4)
    throw std::runtime_error("ewdml muon: misaligned operand");
  MuArgs a{};
  a.mats = reinterpret_cast<const MuonMat*>(h.mats);
  a.items = reinterpret_cast<const MuonItem*>(h.items);
  a.xin = reinterpret_cast<const float*>(h.x_in);
  a.xout = reinterpret_cast<float*>(h.x_out);
  a.A = reinterpret_cast<float*>(h.a_buf);
  a.B = reinterpret_cast<float*>(h.b_buf);
  a.slabs = reinterpret_cast<float*>(h.slabs);
  a.tickets = reinterpret_cast<int*>(h.tickets);
  a.partials = reinterpret_cast<const float*>(h.partials);
  a.param = reinterpret_cast<float*>(h.param);
  a.shadow = reinterpret_cast<uint16_t*>(h.shadow);
  a.lr_ptr = reinterpret_cast<const float*>(h.lr_ptr);
  a.lr = h.lr;
  a.weight_decay = h.weight_decay;
  a.first = h.first;
  a.last = h.last;
  return a;
}

}  // namespace

// K<T, ...> over the work list, T picked by the Newton-Schulz dtype
#define MU_LAUNCH(KF, KB)                                                          \
  do {                                                                             \
    const dim3 grid(h.num_items), block(EW_BLOCK);                                 \
    hipStream_t s = (hipStream_t)h.stream;                                         \
    if (h.ns_bf16) hipLaunchKernelGGL(KB, grid, block, 0, s, a);                   \
    else hipLaunchKernelGGL(KF, grid, block, 0, s, a);                             \
  } while (0)

void ew_muon_momentum(const MuonArgs& h) {
  if (h.num_chunks < 1 || !h.param || !h.mom || !h.grad || !h.chunks || !h.xoff || !h.x_out ||
      !h.partials)
    throw std::runtime_error("ewdml muon: missing operand");
  if (h.grad_dtype < 0 || h.grad_dtype > 2)
    throw std::runtime_error("ewdml muon: unknown gradient dtype");
  if ((h.param | h.mom | h.x_out) % 16 || h.grad % 8 || h.shadow % 8 ||
      (h.partials | h.lr_ptr | h.xoff) % 4)
    throw std::runtime_error("ewdml muon: misaligned operand");
  MuMomArgs a{};
  a.p = reinterpret_cast<float*>(h.param);
  a.mom = reinterpret_cast<float*>(h.mom);
  a.g = reinterpret_cast<const void*>(h.grad);
  a.shadow = reinterpret_cast<uint16_t*>(h.shadow);
  a.chunks = reinterpret_cast<const ChunkRow*>(h.chunks);
  a.xoff = reinterpret_cast<const int*>(h.xoff);
  a.x = reinterpret_cast<float*>(h.x_out);
  a.partials = reinterpret_cast<float*>(h.partials);
  a.lr_ptr = reinterpret_cast<const float*>(h.lr_ptr);
  a.lr = h.lr; a.aux_ratio = h.aux_ratio; a.momentum = h.momentum;
  a.weight_decay = h.weight_decay; a.grad_scale = h.grad_scale;
  a.nesterov = h.nesterov;
  const dim3 grid(h.num_chunks), block(EW_BLOCK);
  hipStream_t s = (hipStream_t)h.stream;
  if (h.grad_dtype == 0) hipLaunchKernelGGL((k_muon_momentum<0>), grid, block, 0, s, a);
  else if (h.grad_dtype == 1) hipLaunchKernelGGL((k_muon_momentum<1>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_muon_momentum<2>), grid, block, 0, s, a);
  EW_CHECK_LAUNCH();
}

void ew_muon_gram(const MuonArgs& h) {
  const MuArgs a = mu_args(h);
  if (!h.slabs || !h.tickets) throw std::runtime_error("ewdml muon: the gram needs its slabs");
  MU_LAUNCH((k_muon_syrk<float, 0>), (k_muon_syrk<uint16_t, 0>));
  EW_CHECK_LAUNCH();
}

void ew_muon_poly(const MuonArgs& h) {
  const MuArgs a = mu_args(h);
  MU_LAUNCH((k_muon_syrk<float, 1>), (k_muon_syrk<uint16_t, 1>));
  EW_CHECK_LAUNCH();
}

void ew_muon_update(const MuonArgs& h) {
  const MuArgs a = mu_args(h);
  if (h.last ? !h.param : !h.x_out)
    throw std::runtime_error("ewdml muon: the update needs its destination");
  MU_LAUNCH((k_muon_update<float>), (k_muon_update<uint16_t>));
  EW_CHECK_LAUNCH();
}
