// GaLore (Zhao et al., ICML 2024) over the flat parameter buffer: Adam whose two moments of every
// weight matrix live in a rank-r subspace of its short side, refreshed from the gradient every
// update_gap steps by a subspace iteration.  gfx950, wave64.  compress/oracle.py galore_apply
// defines the arithmetic.
//
// A tensor is viewed as [n, m]; its oriented form is [s, l] = [short, long], G(i, j) = g[off + i rs
// + j cs] with the pair of strides in the matrix table (ops.GalorePlan), so a tall tensor is never
// copied.  P is [s, r] row-major, the low-rank moments are R's shape ([r, m] or [n, r]) and are
// addressed through a second pair of strides.  Every launch walks a work list built at plan time.
//
// One product serves three kernels (gl_product): out[r-index][column] = sum_k A[k][r-index] *
// B(k, column), A a row-major [K, r] matrix (P or Z), B the gradient read through two strides with
// grad_scale applied.  A block of 4 waves owns 64 columns; wave w owns 16 of them and ALL r rows:
// r / 16 accumulator tiles of v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 sums).  K runs
// through double-buffered LDS panels of 16 k (A: [k][r], B: [k][64], padded rows); the loads of
// panel s + 1 are issued before the MFMAs of panel s and stored after them, one barrier a panel.
// Rows, columns and k past the matrix are predicated zeros; nothing is padded in memory.  The
// rank is rounded up to RT in {16, 32, 64, 128} for the register tiles only.
//
//   k_gl_step    item = (matrix, strip of 64 long-side columns).  (a) R = P^T G of the strip, K =
//                s.  (b) Adam in the accumulator registers against the M and V tiles, each read
//                and written once.  (c) back-projection: for every slab of 32 short-side rows,
//                P[slab, :] N with K = r, then p = p (1 - lr wd) - lr alpha (P N) and the bf16
//                shadow.  The accumulator layout of (a) -- lane (g, c) holds rows 16 f + 4 g + q
//                of column c -- IS the B-operand layout of (c) when MFMA e of k-block f takes
//                k = 16 f + 4 g + e from lane group g, and P's fragment is then one 16-byte LDS
//                read.  So N never leaves the registers: not to LDS, not to memory.
//   k_gl_dense   Adam with full moments for vectors and matrices with s <= r, per chunk row.
//   k_gl_sketch  Z = G^T P ([l, r]): phase (a) alone, stored.
//   k_gl_range   Y = G Z ([s, r]): the same product with A = Z and the strides swapped; K = l is
//                cut into slabs, one block per (64 rows, slab), and the tile's last block to
//                arrive adds the slabs in slab order (release / acquire around an arrival
//                counter, as k_muon_gram).
//   k_gl_orth    P = orth(Y), one workgroup per matrix: classical Gram-Schmidt in column order
//                with one re-orthogonalisation; dots are fp32 products summed in fp64 in a fixed
//                order, norms fp64.  A column whose norm after the first pass is at most 2^-12
//                of its norm before is set to zero.
//
// The three refresh kernels are launched every step and exit at once unless step % update_gap ==
// 0 (device step counter), so a captured step replays unchanged.  No float atomics: every sum has
// a fixed order, a step is bitwise reproducible and does not depend on the range it is part of.
#include "common.h"
#include "ewdml_ops.h"

namespace {

typedef float gl_f32x4 __attribute__((ext_vector_type(4)));

constexpr int GL_W = 64;          // columns of a work item (ops.GALORE_W)
constexpr int GL_KS = 16;         // k rows of a panel
constexpr int GL_LDG = GL_W + 16; // padded row of the B panel: the 4 lane groups hit 4 bank groups
constexpr int GL_SLAB = 32;       // short-side rows of a back-projection slab
constexpr double GL_ZERO = 1.0 / 4096.0;

struct GlMat {  // mirrors ops.GalorePlan.mats rows (int32 x 16)
  int off;      // the tensor's offset in the flat range
  int s, l;     // short and long side
  int rs, cs;   // G(i, j) = g[off + i rs + j cs]
  int p0;       // offset of P in proj
  int s0;       // offset of the low-rank moments in m_lr / v_lr
  int mk, mj;   // M(k, j) = m_lr[s0 + k mk + j mj]
  int z0, y0;   // offsets of Z [l, r] and Y [s, r] in the workspaces
  int part0;    // range slabs: [tile][slab][64 RT] floats (splits > 1)
  int tick0;    // arrival counters, one per 64-row tile
  int splits, kper;  // slabs of the long side and their length (a multiple of GL_KS)
  int pad;
};
struct GlItem {  // step / sketch: mat, strip.  range: mat, tile of 64 rows, slab, tile index
  int mat, a, b, tile;
};
struct GlChunk {  // a dense tensor's chunk row: start in the range, len, offset in m / v
  int start, len, s0, pad;
};

struct GlArgs {
  float* p;
  float* proj;
  float* m_lr;
  float* v_lr;
  float* m;
  float* v;
  const void* g;
  uint16_t* shadow;
  const GlMat* mats;
  const GlItem* items;
  const GlItem* ritems;
  const GlChunk* ditems;
  float* z;
  float* y;
  float* parts;
  int* tickets;
  const int* step;      // nullable device step counter: t = *step + 1
  const float* lr_ptr;  // nullable device lr
  int rank, gap, refresh, t;
  float lr, beta1, omb1, beta2, omb2, eps, weight_decay, scale, grad_scale;
};

template <int RT>
struct GlCfg {
  static constexpr int NT = RT / 16;
  static constexpr int LDP = RT == 16 ? 16 : RT + 16;  // padded row of the A panel
  static constexpr int APT = RT == 128 ? 2 : 1;        // 16-byte slots of an A panel per thread
  static constexpr int LDC = RT + 4;                   // padded row of a P slab
  static constexpr int SPT = RT <= 32 ? 1 : RT / 32;   // 16-byte slots of a P slab per thread
  static constexpr int PANEL = GL_KS * (LDP + GL_LDG);
  static constexpr int ARENA = 2 * PANEL > 2 * GL_SLAB * LDC ? 2 * PANEL : 2 * GL_SLAB * LDC;
};

__device__ __forceinline__ bool gl_refresh(const GlArgs& a) {
  return a.step ? (*a.step % a.gap) == 0 : a.refresh != 0;
}

struct GlHyp {
  float bc1, bc2, keep, step_lr, step_dense;
};
// b^t by squaring, the multiplications in oracle.galore_pow's order: the same double on both sides
__device__ __forceinline__ double gl_pow(double b, int t) {
  double r = 1.0;
  for (; t > 0; t >>= 1) {
    if (t & 1) r = r * b;
    b = b * b;
  }
  return r;
}

// the step's scalars, formed in double and rounded once (oracle.galore_scalars)
__device__ __forceinline__ GlHyp gl_resolve(const GlArgs& a) {
  const double lr = (double)(a.lr_ptr ? *a.lr_ptr : a.lr);
  const int t = a.step ? *a.step + 1 : a.t;
  GlHyp h;
  h.bc1 = (float)(1.0 - gl_pow((double)a.beta1, t));
  h.bc2 = (float)(1.0 - gl_pow((double)a.beta2, t));
  h.keep = (float)(1.0 - lr * (double)a.weight_decay);
  h.step_lr = (float)(lr * (double)a.scale);
  h.step_dense = (float)lr;
  return h;
}

// one element of Adam: the moments in place, returns N
__device__ __forceinline__ float gl_adam1(float& m, float& v, float r, const GlArgs& a,
                                          const GlHyp& h) {
  m = m * a.beta1 + r * a.omb1;
  v = v * a.beta2 + (r * r) * a.omb2;
  return (m / h.bc1) / (sqrtf(v / h.bc2) + a.eps);
}

template <int GT>
__device__ __forceinline__ float gl_ld1(const void* g, long long i) {
  if (GT == 0) return reinterpret_cast<const float*>(g)[i];
  if (GT == 1) return ew_bf16f(reinterpret_cast<const uint16_t*>(g)[i]);
  return __half2float(reinterpret_cast<const __half*>(g)[i]);
}

// This thread's 16-byte slots of the A panel rows k0 .. k0 + 15 of the row-major [K, r] matrix A
template <int RT>
__device__ __forceinline__ void gl_ld_a(const float* A, int r, int k0, int kend,
                                        float4 (&v)[GlCfg<RT>::APT]) {
#pragma unroll
  for (int u = 0; u < GlCfg<RT>::APT; ++u) {
    const int idx = (int)threadIdx.x + EW_BLOCK * u;
    const int row = idx / (RT / 4), c4 = 4 * (idx % (RT / 4));
    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (idx < 4 * RT && k0 + row < kend && c4 < r)
      v[u] = *reinterpret_cast<const float4*>(A + (long long)(k0 + row) * r + c4);
  }
}
template <int RT>
__device__ __forceinline__ void gl_st_a(float* la, const float4 (&v)[GlCfg<RT>::APT]) {
#pragma unroll
  for (int u = 0; u < GlCfg<RT>::APT; ++u) {
    const int idx = (int)threadIdx.x + EW_BLOCK * u;
    const int row = idx / (RT / 4), c4 = 4 * (idx % (RT / 4));
    if (idx < 4 * RT) *reinterpret_cast<float4*>(la + row * GlCfg<RT>::LDP + c4) = v[u];
  }
}

// This thread's 4 elements of the B panel: B(k, c) = g[goff + k ks + c cs] * scale, zero for
// k >= kend or c >= cend.  cc (cs == 1): 4 neighbours of one k; else (ks == 1) 4 k of one column.
template <int GT>
__device__ __forceinline__ void gl_ld_b(const void* g, long long goff, long long ks, long long cs,
                                        bool cc, int k0, int kend, int c0, int cend, float scale,
                                        float (&v)[4]) {
  const int t = threadIdx.x;
  const int k = k0 + (cc ? (t >> 4) : 4 * (t & 3));
  const int c = c0 + (cc ? 4 * (t & 15) : (t >> 2));
  const long long o = goff + (long long)k * ks + (long long)c * cs;
  const int kn = cc ? 1 : 4, cn = cc ? 4 : 1;
  if (k + kn <= kend && c + cn <= cend && (o & 3) == 0) {
    ew_load_grad4<GT>(g, o, v);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = cc ? (k < kend && c + e < cend) : (k + e < kend && c < cend);
      v[e] = ok ? gl_ld1<GT>(g, o + e) : 0.0f;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = v[e] * scale;
}
__device__ __forceinline__ void gl_st_b(float* lb, bool cc, const float (&v)[4]) {
  const int t = threadIdx.x;
  if (cc) {
    *reinterpret_cast<float4*>(lb + (t >> 4) * GL_LDG + 4 * (t & 15)) =
        make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) lb[(4 * (t & 3) + e) * GL_LDG + (t >> 2)] = v[e];
  }
}

// acc[f][q] += sum over k in [kbeg, kend) of A[k][16 f + 4 (lane >> 4) + q] * B(k, c0 + 16 wave +
// (lane & 15)).  Ends with a barrier: lds is free on return.
template <int RT, int GT>
__device__ __forceinline__ void gl_product(const float* A, int r, const void* g, long long goff,
                                           long long ks, long long cs, int kbeg, int kend, int c0,
                                           int cend, float scale, float* lds,
                                           gl_f32x4 (&acc)[RT / 16]) {
  using C = GlCfg<RT>;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g4 = lane >> 4, ln = lane & 15;
  const bool cc = cs == 1;
  float4 va[C::APT];
  float vb[4];
  gl_ld_a<RT>(A, r, kbeg, kend, va);
  gl_ld_b<GT>(g, goff, ks, cs, cc, kbeg, kend, c0, cend, scale, vb);
  gl_st_a<RT>(lds, va);
  gl_st_b(lds + GL_KS * C::LDP, cc, vb);
  __syncthreads();
  const int steps = (kend - kbeg + GL_KS - 1) / GL_KS;
  for (int s = 0; s < steps; ++s) {
    const int cur = s & 1;
    const bool more = s + 1 < steps;
    if (more) {
      const int k0 = kbeg + (s + 1) * GL_KS;
      gl_ld_a<RT>(A, r, k0, kend, va);
      gl_ld_b<GT>(g, goff, ks, cs, cc, k0, kend, c0, cend, scale, vb);
    }
    const float* pa = lds + cur * C::PANEL;
    const float* pb = pa + GL_KS * C::LDP;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int kk = 4 * e + g4;
      const float b = pb[kk * GL_LDG + 16 * w + ln];
#pragma unroll
      for (int f = 0; f < C::NT; ++f)
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[kk * C::LDP + 16 * f + ln], b, acc[f], 0,
                                                      0, 0);
    }
    if (more) {
      float* na = lds + (cur ^ 1) * C::PANEL;
      gl_st_a<RT>(na, va);
      gl_st_b(na + GL_KS * C::LDP, cc, vb);
    }
    __syncthreads();
  }
}

// This thread's 16-byte slots of rows i0 .. i0 + 31 of P
template <int RT>
__device__ __forceinline__ void gl_ld_slab(const float* P, int r, int i0, int s,
                                           float4 (&v)[GlCfg<RT>::SPT]) {
#pragma unroll
  for (int u = 0; u < GlCfg<RT>::SPT; ++u) {
    const int idx = (int)threadIdx.x + EW_BLOCK * u;
    const int row = idx / (RT / 4), c4 = 4 * (idx % (RT / 4));
    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < GL_SLAB && i0 + row < s && c4 < r)
      v[u] = *reinterpret_cast<const float4*>(P + (long long)(i0 + row) * r + c4);
  }
}
template <int RT>
__device__ __forceinline__ void gl_st_slab(float* ls, const float4 (&v)[GlCfg<RT>::SPT]) {
#pragma unroll
  for (int u = 0; u < GlCfg<RT>::SPT; ++u) {
    const int idx = (int)threadIdx.x + EW_BLOCK * u;
    const int row = idx / (RT / 4), c4 = 4 * (idx % (RT / 4));
    if (row < GL_SLAB) *reinterpret_cast<float4*>(ls + row * GlCfg<RT>::LDC + c4) = v[u];
  }
}

// One strip of one matrix: the sketch (Z's strip) or the whole step.
template <int RT, int GT, int SKETCH>
__device__ __forceinline__ void gl_strip(const GlArgs& a, float* lds) {
  using C = GlCfg<RT>;
  const GlItem it = a.items[blockIdx.x];
  const GlMat mt = a.mats[it.mat];
  const int r = a.rank, c0 = GL_W * it.a;
  const float* P = a.proj + mt.p0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g4 = lane >> 4, ln = lane & 15;
  const int j = c0 + 16 * w + ln;
  gl_f32x4 acc[C::NT];
#pragma unroll
  for (int f = 0; f < C::NT; ++f) acc[f] = gl_f32x4{0.f, 0.f, 0.f, 0.f};
  // (a) R = P^T G of the strip
  gl_product<RT, GT>(P, r, a.g, mt.off, mt.rs, mt.cs, 0, mt.s, c0, mt.l, a.grad_scale, lds, acc);
  if (SKETCH) {
    float* Z = a.z + mt.z0;
    if (j < mt.l) {
#pragma unroll
      for (int f = 0; f < C::NT; ++f) {
        const int k = 16 * f + 4 * g4;
        if (k < r)
          *reinterpret_cast<float4*>(Z + (long long)j * r + k) =
              make_float4(acc[f][0], acc[f][1], acc[f][2], acc[f][3]);
      }
    }
    return;
  }
  // (b) Adam in the accumulators: acc becomes N
  const GlHyp h = gl_resolve(a);
#pragma unroll
  for (int f = 0; f < C::NT; ++f) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = 16 * f + 4 * g4 + q;
      float n = 0.0f;
      if (k < r && j < mt.l) {
        const long long e = (long long)mt.s0 + (long long)k * mt.mk + (long long)j * mt.mj;
        float m = a.m_lr[e], v = a.v_lr[e];
        n = gl_adam1(m, v, acc[f][q], a, h);
        a.m_lr[e] = m;
        a.v_lr[e] = v;
      }
      acc[f][q] = n;
    }
  }
  // (c) back-projection, slab by slab of the short side
  const int nsl = (mt.s + GL_SLAB - 1) / GL_SLAB;
  float4 vp[C::SPT];
  gl_ld_slab<RT>(P, r, 0, mt.s, vp);
  gl_st_slab<RT>(lds, vp);
  __syncthreads();
  for (int sl = 0; sl < nsl; ++sl) {
    const int cur = sl & 1;
    const bool more = sl + 1 < nsl;
    if (more) gl_ld_slab<RT>(P, r, GL_SLAB * (sl + 1), mt.s, vp);
    const float* ps = lds + cur * (GL_SLAB * C::LDC);
#pragma unroll
    for (int t2 = 0; t2 < GL_SLAB / 16; ++t2) {
      const int i0 = GL_SLAB * sl + 16 * t2;
      if (i0 >= mt.s) break;
      gl_f32x4 out = gl_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < C::NT; ++kb) {
        const float4 pv =
            *reinterpret_cast<const float4*>(ps + (16 * t2 + ln) * C::LDC + 16 * kb + 4 * g4);
        out = __builtin_amdgcn_mfma_f32_16x16x4f32(pv.x, acc[kb][0], out, 0, 0, 0);
        out = __builtin_amdgcn_mfma_f32_16x16x4f32(pv.y, acc[kb][1], out, 0, 0, 0);
        out = __builtin_amdgcn_mfma_f32_16x16x4f32(pv.z, acc[kb][2], out, 0, 0, 0);
        out = __builtin_amdgcn_mfma_f32_16x16x4f32(pv.w, acc[kb][3], out, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + 4 * g4 + q;
        if (i < mt.s && j < mt.l) {
          const long long e = (long long)mt.off + (long long)i * mt.rs + (long long)j * mt.cs;
          const float pv = a.p[e] * h.keep - h.step_lr * out[q];
          a.p[e] = pv;
          if (a.shadow) a.shadow[e] = ew_f2bf(pv);
        }
      }
    }
    if (more) gl_st_slab<RT>(lds + (cur ^ 1) * (GL_SLAB * C::LDC), vp);
    __syncthreads();
  }
}

template <int RT, int GT>
__global__ __launch_bounds__(EW_BLOCK) void k_gl_step(GlArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[GlCfg<RT>::ARENA];
  gl_strip<RT, GT, 0>(a, lds);
}

template <int RT, int GT>
__global__ __launch_bounds__(EW_BLOCK) void k_gl_sketch(GlArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[2 * GlCfg<RT>::PANEL];
  if (!gl_refresh(a)) return;
  gl_strip<RT, GT, 1>(a, lds);
}

// Y = G Z: out[k][i] = sum_j Z[j][k] G(i, j) over the item's slab of j
template <int RT, int GT>
__global__ __launch_bounds__(EW_BLOCK) void k_gl_range(GlArgs a) {
  using C = GlCfg<RT>;
  __shared__ __attribute__((aligned(16))) float lds[2 * C::PANEL];
  __shared__ int s_last;
  if (!gl_refresh(a)) return;
  const GlItem it = a.ritems[blockIdx.x];
  const GlMat mt = a.mats[it.mat];
  const int r = a.rank, c0 = GL_W * it.a;
  const int kbeg = it.b * mt.kper, kend = min(mt.l, kbeg + mt.kper);
  gl_f32x4 acc[C::NT];
#pragma unroll
  for (int f = 0; f < C::NT; ++f) acc[f] = gl_f32x4{0.f, 0.f, 0.f, 0.f};
  gl_product<RT, GT>(a.z + mt.z0, r, a.g, mt.off, mt.cs, mt.rs, kbeg, kend, c0, mt.s,
                     a.grad_scale, lds, acc);
  const int t = threadIdx.x;
  if (mt.splits > 1) {
    constexpr int TILE = GL_W * RT;
    float* tile = a.parts + (size_t)mt.part0 + (size_t)it.tile * mt.splits * TILE;
    float* mine = tile + (size_t)it.b * TILE;
#pragma unroll
    for (int f = 0; f < C::NT; ++f)
#pragma unroll
      for (int q = 0; q < 4; ++q) mine[(f * 4 + q) * EW_BLOCK + t] = acc[f][q];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      int* cnt = a.tickets + mt.tick0 + it.tile;
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
    for (int f = 0; f < C::NT; ++f)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float* p = tile + (f * 4 + q) * EW_BLOCK + t;
        float s = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int z = 1; z < mt.splits; ++z)
          s = s + __hip_atomic_load(p + (size_t)z * TILE, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
        acc[f][q] = s;
      }
  }
  const int lane = t & 63, w = t >> 6, g4 = lane >> 4, ln = lane & 15;
  const int i = c0 + 16 * w + ln;
  float* Y = a.y + mt.y0;
  if (i < mt.s) {
#pragma unroll
    for (int f = 0; f < C::NT; ++f) {
      const int k = 16 * f + 4 * g4;
      if (k < r)
        *reinterpret_cast<float4*>(Y + (long long)i * r + k) =
            make_float4(acc[f][0], acc[f][1], acc[f][2], acc[f][3]);
    }
  }
}

__device__ __forceinline__ double gl_wave_sum_d(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// sqrt of the fp64 sum of squares of column c of Y, the same value in every thread: thread i adds
// rows i, i + 256, ... in order, then the wave tree and the four waves in order
__device__ __forceinline__ double gl_col_norm(const float* Y, int s, int r, int c, double* wd) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < s; i += EW_BLOCK) {
    const double y = (double)Y[(long long)i * r + c];
    acc += y * y;
  }
  acc = gl_wave_sum_d(acc);
  __syncthreads();  // wd may still be read from the previous call
  if ((threadIdx.x & 63) == 0) wd[threadIdx.x >> 6] = acc;
  __syncthreads();
  return sqrt(((wd[0] + wd[1]) + wd[2]) + wd[3]);
}

// One Gram-Schmidt pass of column c of Y against columns 0 .. c - 1 of P: h = P^T y, y -= P h
__device__ __forceinline__ void gl_gs_pass(const float* P, float* Y, int s, int r, int c,
                                           double (*dsum)[128], float* hs) {
  const int jj = threadIdx.x & 63, rg = threadIdx.x >> 6;
  double d0 = 0.0, d1 = 0.0;
  for (int i = rg; i < s; i += EW_WAVES) {
    const float y = Y[(long long)i * r + c];
    const float* pr = P + (long long)i * r;
    if (jj < c) d0 += (double)(pr[jj] * y);
    if (jj + 64 < c) d1 += (double)(pr[jj + 64] * y);
  }
  dsum[rg][jj] = d0;
  dsum[rg][jj + 64] = d1;
  __syncthreads();
  if (threadIdx.x < 128) {
    const int q = threadIdx.x;
    hs[q] = q < c ? (float)(((dsum[0][q] + dsum[1][q]) + dsum[2][q]) + dsum[3][q]) : 0.0f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < s; i += EW_BLOCK) {
    const float* pr = P + (long long)i * r;
    float sub = 0.0f;
    for (int q = 0; q < c; ++q) sub += pr[q] * hs[q];
    Y[(long long)i * r + c] = Y[(long long)i * r + c] - sub;
  }
  __syncthreads();
}

__global__ __launch_bounds__(EW_BLOCK) void k_gl_orth(GlArgs a) {
  __shared__ double dsum[EW_WAVES][128];
  __shared__ double wd[EW_WAVES];
  __shared__ float hs[128];
  if (!gl_refresh(a)) return;
  const GlMat mt = a.mats[blockIdx.x];
  const int r = a.rank, s = mt.s;
  float* P = a.proj + mt.p0;
  float* Y = a.y + mt.y0;
  for (int c = 0; c < r; ++c) {
    const double n0 = gl_col_norm(Y, s, r, c, wd);
    gl_gs_pass(P, Y, s, r, c, dsum, hs);
    const double n1 = gl_col_norm(Y, s, r, c, wd);
    float den = 1.0f;
    bool keep = n1 > GL_ZERO * n0;  // uniform: every thread holds the same norms
    if (keep) {
      gl_gs_pass(P, Y, s, r, c, dsum, hs);
      den = (float)gl_col_norm(Y, s, r, c, wd);
    }
    for (int i = threadIdx.x; i < s; i += EW_BLOCK)
      P[(long long)i * r + c] = keep ? Y[(long long)i * r + c] / den : 0.0f;
    __syncthreads();
  }
}

template <int GT>
__global__ __launch_bounds__(EW_BLOCK) void k_gl_dense(GlArgs a) {
  const GlChunk c = a.ditems[blockIdx.x];
  const GlHyp h = gl_resolve(a);
  float* m = a.m + c.s0;
  float* v = a.v + c.s0;
#pragma unroll 2
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    if (i >= c.len) break;
    const long long o = (long long)c.start + i;
    const int nv = c.len - i >= 4 ? 4 : c.len - i;
    float g[4], pv[4], mv[4], vv[4];
    if (nv == 4) {
      ew_load_grad4<GT>(a.g, o, g);
      const float4 p4 = *reinterpret_cast<const float4*>(a.p + o);
      const float4 m4 = *reinterpret_cast<const float4*>(m + i);
      const float4 v4 = *reinterpret_cast<const float4*>(v + i);
      pv[0] = p4.x; pv[1] = p4.y; pv[2] = p4.z; pv[3] = p4.w;
      mv[0] = m4.x; mv[1] = m4.y; mv[2] = m4.z; mv[3] = m4.w;
      vv[0] = v4.x; vv[1] = v4.y; vv[2] = v4.z; vv[3] = v4.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g[k] = k < nv ? gl_ld1<GT>(a.g, o + k) : 0.0f;
        pv[k] = k < nv ? a.p[o + k] : 0.0f;
        mv[k] = k < nv ? m[i + k] : 0.0f;
        vv[k] = k < nv ? v[i + k] : 1.0f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float n = gl_adam1(mv[k], vv[k], g[k] * a.grad_scale, a, h);
      pv[k] = pv[k] * h.keep - h.step_dense * n;
    }
    if (nv == 4) {
      *reinterpret_cast<float4*>(a.p + o) = make_float4(pv[0], pv[1], pv[2], pv[3]);
      *reinterpret_cast<float4*>(m + i) = make_float4(mv[0], mv[1], mv[2], mv[3]);
      *reinterpret_cast<float4*>(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
      if (a.shadow) ew_st4_bf16(a.shadow + o, 4, pv);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < nv) {
          a.p[o + k] = pv[k];
          m[i + k] = mv[k];
          v[i + k] = vv[k];
          if (a.shadow) a.shadow[o + k] = ew_f2bf(pv[k]);
        }
      }
    }
  }
}

GlArgs gl_args(const GaloreArgs& h) {
  if (h.grad_dtype < 0 || h.grad_dtype > 2)
    throw std::runtime_error("ewdml galore: unknown gradient dtype");
  if (h.rank < 16 || h.rank > 128 || h.rank % 16 || h.update_gap < 1)
    throw std::runtime_error("ewdml galore: the rank is a multiple of 16 in 16..128, the gap >= 1");
  if (h.num_items < 0 || h.num_ritems < 0 || h.num_ditems < 0 || h.num_mats < 0 || !h.param ||
      !h.grad ||
      (h.num_mats > 0 && (h.num_items < 1 || h.num_ritems < 1 || !h.proj || !h.m_lr || !h.v_lr ||
                          !h.mats || !h.items || !h.ritems || !h.z || !h.y || !h.parts ||
                          !h.tickets)) ||
      (h.num_ditems > 0 && (!h.m || !h.v || !h.ditems)))
    throw std::runtime_error("ewdml galore: missing operand");
  if ((h.param | h.proj | h.m_lr | h.v_lr | h.m | h.v | h.z | h.y | h.parts) % 16 || h.grad % 8 ||
      h.shadow % 8 || (h.tickets | h.step | h.lr_ptr) % 4)
    throw std::runtime_error("ewdml galore: misaligned operand");
  GlArgs a{};
  a.p = reinterpret_cast<float*>(h.param);
  a.proj = reinterpret_cast<float*>(h.proj);
  a.m_lr = reinterpret_cast<float*>(h.m_lr);
  a.v_lr = reinterpret_cast<float*>(h.v_lr);
  a.m = reinterpret_cast<float*>(h.m);
  a.v = reinterpret_cast<float*>(h.v);
  a.g = reinterpret_cast<const void*>(h.grad);
  a.shadow = reinterpret_cast<uint16_t*>(h.shadow);
  a.mats = reinterpret_cast<const GlMat*>(h.mats);
  a.items = reinterpret_cast<const GlItem*>(h.items);
  a.ritems = reinterpret_cast<const GlItem*>(h.ritems);
  a.ditems = reinterpret_cast<const GlChunk*>(h.ditems);
  a.z = reinterpret_cast<float*>(h.z);
  a.y = reinterpret_cast<float*>(h.y);
  a.parts = reinterpret_cast<float*>(h.parts);
  a.tickets = reinterpret_cast<int*>(h.tickets);
  a.step = reinterpret_cast<const int*>(h.step);
  a.lr_ptr = reinterpret_cast<const float*>(h.lr_ptr);
  a.rank = h.rank; a.gap = h.update_gap; a.refresh = h.refresh; a.t = h.t;
  a.lr = h.lr; a.beta1 = h.beta1; a.omb1 = (float)(1.0 - (double)h.beta1);
  a.beta2 = h.beta2; a.omb2 = (float)(1.0 - (double)h.beta2);
  a.eps = h.eps; a.weight_decay = h.weight_decay; a.scale = h.scale; a.grad_scale = h.grad_scale;
  return a;
}

}  // namespace

// K<RT, GT> over N blocks, RT the rank rounded up to a register tile count, GT the gradient type
#define GL_BY_GT(K, RT, N)                                                                 \
  do {                                                                                     \
    const dim3 grid(N), block(EW_BLOCK);                                                   \
    hipStream_t s = (hipStream_t)h.stream;                                                 \
    if (h.grad_dtype == 0) hipLaunchKernelGGL((K<RT, 0>), grid, block, 0, s, a);           \
    else if (h.grad_dtype == 1) hipLaunchKernelGGL((K<RT, 1>), grid, block, 0, s, a);      \
    else hipLaunchKernelGGL((K<RT, 2>), grid, block, 0, s, a);                             \
  } while (0)
#define GL_LAUNCH(K, N)                          \
  do {                                           \
    if (h.rank <= 16) GL_BY_GT(K, 16, N);        \
    else if (h.rank <= 32) GL_BY_GT(K, 32, N);   \
    else if (h.rank <= 64) GL_BY_GT(K, 64, N);   \
    else GL_BY_GT(K, 128, N);                    \
  } while (0)

void ew_galore_sketch(const GaloreArgs& h) {
  const GlArgs a = gl_args(h);
  if (h.num_mats < 1) return;  // a range of dense tensors
  GL_LAUNCH(k_gl_sketch, h.num_items);
  EW_CHECK_LAUNCH();
}

void ew_galore_range(const GaloreArgs& h) {
  const GlArgs a = gl_args(h);
  if (h.num_mats < 1) return;
  GL_LAUNCH(k_gl_range, h.num_ritems);
  EW_CHECK_LAUNCH();
}

void ew_galore_orth(const GaloreArgs& h) {
  const GlArgs a = gl_args(h);
  if (h.num_mats < 1) return;
  hipLaunchKernelGGL(k_gl_orth, dim3(h.num_mats), dim3(EW_BLOCK), 0, (hipStream_t)h.stream, a);
  EW_CHECK_LAUNCH();
}

void ew_galore_step(const GaloreArgs& h) {
  const GlArgs a = gl_args(h);
  if (h.num_mats < 1) return;
  GL_LAUNCH(k_gl_step, h.num_items);
  EW_CHECK_LAUNCH();
}

void ew_galore_dense(const GaloreArgs& h) {
  const GlArgs a = gl_args(h);
  if (h.num_ditems < 1) return;
  const dim3 grid(h.num_ditems), block(EW_BLOCK);
  hipStream_t s = (hipStream_t)h.stream;
  if (h.grad_dtype == 0) hipLaunchKernelGGL((k_gl_dense<0>), grid, block, 0, s, a);
  else if (h.grad_dtype == 1) hipLaunchKernelGGL((k_gl_dense<1>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_gl_dense<2>), grid, block, 0, s, a);
  EW_CHECK_LAUNCH();
}
