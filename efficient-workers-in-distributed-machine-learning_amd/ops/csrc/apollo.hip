// APOLLO (Zhu et al., MLSys 2025) over the flat parameter buffer: Adam moments of a rank-r random
// projection R = P^T G of every weight matrix, used only to estimate a learning-rate scale per
// long-side column (or one per tensor), which is applied to the full-rank raw gradient.  gfx950,
// wave64.  compress/oracle.py apollo_apply defines the arithmetic.
//
// A tensor is viewed as [n, m]; its oriented form is [s, l] = [short, long], G(i, j) = g[off + i rs
// + j cs] with the pair of strides in the matrix table (ops.ApolloPlan), so a tall tensor is never
// copied.  P [s, r] is +-1 / sqrt(r): the sign of P(k, i) is bit i % 32 of the word ew_mix32((4 k +
// i / 32) ^ key), key = ew_stream_key(seed, epoch, the tensor's index in the whole model), epoch =
// (t - 1) / update_gap from the device step counter.  P is never stored: it is a function of
// integers, the same in a bucket's step and in a whole-model step, and it changes with the epoch
// inside a captured step with no host action.
//
//   k_ap_stats   item = (matrix, strip of 64 long-side columns), 4 waves.  Wave w owns 16 columns
//                and all RT = roundup(r) rows: RT / 16 accumulator tiles of v_mfma_f32_16x16x4_f32.
//                K runs over the short side in panels of 16 through double-buffered LDS: the G
//                panel [16][64] (padded rows) and, beside it, the panel's 16 x RT / 32 sign words,
//                each computed by one thread one panel ahead.  The A operand of an MFMA is 1.0f
//                with the lane's bit OR-ed into its sign (0.0f for a row >= r), so +-g sums are
//                exact products; 1 / sqrt(r) is applied once to the accumulators.  The B fragments
//                a wave reads are its 16 x 16 G values of the panel, once each: the column squares
//                c_j are accumulated from them.  After the K loop: Adam in the accumulator
//                registers against the M and V tiles (each read and written once), num_j = sum_i
//                Rn^2 and den_j = sum_i R^2 per lane and across the four lane groups in group
//                order, s_j = sqrt(num_j / den_j) into the matrix's [l] workspace (channel scale),
//                and one partial (sum num, sum den, sum s_j^2 c_j, sum c_j) per strip.
//   k_ap_apply   item = (matrix, chunk of the tensor's flat range in memory order).  Every block
//                adds the matrix's strip partials in strip order in double: the update norm u, the
//                tensor-type scale, and the norm-growth limiter lim = max(u / u_prev, 1.01) / 1.01
//                against the stored norm.  Then p = p (1 - lr wd) - (lr alpha / lim) s_j g and the
//                bf16 shadow.  The stored norm is [matrix][2], indexed by the step's parity: every
//                block reads slot (t - 1) & 1 and the matrix's first block writes slot t & 1.
//
// Tensors outside the projection take GaLore's dense launch (ew_galore_dense).  No float atomics:
// every sum has a fixed order, a step is bitwise reproducible and does not depend on the range it
// is part of.
#include "common.h"
#include "ewdml_ops.h"

namespace {

typedef float ap_f32x4 __attribute__((ext_vector_type(4)));

constexpr int AP_W = 64;          // columns of a work item (ops.APOLLO_W)
constexpr int AP_KS = 16;         // k rows of a panel
constexpr int AP_LDG = AP_W + 16; // padded row of the G panel: the 4 lane groups hit 4 bank groups
constexpr double AP_GAMMA = 1.01; // the norm-growth limiter's threshold (oracle.APOLLO_GAMMA)

struct ApMat {  // mirrors ops.ApolloPlan.mats rows (int32 x 16)
  int off;      // the tensor's offset in the flat range
  int s, l;     // short and long side
  int rs, cs;   // G(i, j) = g[off + i rs + j cs]
  int s0;       // offset of the low-rank moments in m_lr / v_lr
  int mk, mj;   // M(k, j) = m_lr[s0 + k mk + j mj]
  int gidx;     // the tensor's index in the whole model: P's key
  int w0;       // offset of s_j [l] in the workspace
  int it0, ns;  // the matrix's first strip item and its number of strips
  int wide;     // n <= m: the long index of a flat element is idx % l, else idx / s
  int pad[3];
};
struct ApItem {  // stats: mat, strip.  apply: mat, chunk of EW_CHUNK elements
  int mat, a, pad0, pad1;
};

struct ApArgs {
  float* p;
  float* m_lr;
  float* v_lr;
  const void* g;
  uint16_t* shadow;
  const ApMat* mats;
  const ApItem* items;
  const ApItem* aitems;
  float* sj;
  float* parts;
  float* norms;
  const int* step;      // nullable device step counter: t = *step + 1
  const float* lr_ptr;  // nullable device lr
  int rank, gap, tensor_scale, t;
  uint32_t seed;
  float lr, beta1, omb1, beta2, omb2, eps, weight_decay, scale, grad_scale;
};

template <int RT>
struct ApCfg {
  static constexpr int NT = RT / 16;
  static constexpr int NW = RT <= 32 ? 1 : RT / 32;  // sign words of one k
  static constexpr int PANEL = AP_KS * (AP_LDG + NW);
};

struct ApHyp {
  int t, epoch;
  float bc1, bc2, keep, rs;
  double step;  // lr alpha, divided by lim before it is rounded
};
// b^t by squaring, the multiplications in oracle.galore_pow's order: the same double on both sides
__device__ __forceinline__ double ap_pow(double b, int t) {
  double r = 1.0;
  for (; t > 0; t >>= 1) {
    if (t & 1) r = r * b;
    b = b * b;
  }
  return r;
}

// the step's scalars, formed in double and rounded once (oracle.galore_scalars)
__device__ __forceinline__ ApHyp ap_resolve(const ApArgs& a) {
  const double lr = (double)(a.lr_ptr ? *a.lr_ptr : a.lr);
  ApHyp h;
  h.t = a.step ? *a.step + 1 : a.t;
  h.epoch = (h.t - 1) / a.gap;
  h.bc1 = (float)(1.0 - ap_pow((double)a.beta1, h.t));
  h.bc2 = (float)(1.0 - ap_pow((double)a.beta2, h.t));
  h.keep = (float)(1.0 - lr * (double)a.weight_decay);
  h.rs = (float)(1.0 / sqrt((double)a.rank));
  h.step = lr * (double)a.scale;
  return h;
}

// one element of Adam (galore.hip gl_adam1): the moments in place, returns the normalised R
__device__ __forceinline__ float ap_adam1(float& m, float& v, float r, const ApArgs& a,
                                          const ApHyp& h) {
  m = m * a.beta1 + r * a.omb1;
  v = v * a.beta2 + (r * r) * a.omb2;
  return (m / h.bc1) / (sqrtf(v / h.bc2) + a.eps);
}

template <int GT>
__device__ __forceinline__ float ap_ld1(const void* g, long long i) {
  if (GT == 0) return reinterpret_cast<const float*>(g)[i];
  if (GT == 1) return ew_bf16f(reinterpret_cast<const uint16_t*>(g)[i]);
  return __half2float(reinterpret_cast<const __half*>(g)[i]);
}

// This thread's 4 elements of the G panel: B(k, c) = g[goff + k ks + c cs] * scale, zero for
// k >= kend or c >= cend.  cc (cs == 1): 4 neighbours of one k; else (ks == 1) 4 k of one column.
template <int GT>
__device__ __forceinline__ void ap_ld_b(const void* g, long long goff, long long ks, long long cs,
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
      v[e] = ok ? ap_ld1<GT>(g, o + e) : 0.0f;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = v[e] * scale;
}
__device__ __forceinline__ void ap_st_b(float* lb, bool cc, const float (&v)[4]) {
  const int t = threadIdx.x;
  if (cc) {
    *reinterpret_cast<float4*>(lb + (t >> 4) * AP_LDG + 4 * (t & 15)) =
        make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) lb[(4 * (t & 3) + e) * AP_LDG + (t >> 2)] = v[e];
  }
}

// This thread's sign word of the panel at k0 (threads 0 .. 16 NW - 1: k = k0 + t / NW, word t % NW):
// oracle.apollo_signs.  Words of k past the matrix are never used: their G rows are zeros.
template <int RT>
__device__ __forceinline__ uint32_t ap_word(uint32_t key, int k0) {
  constexpr int NW = ApCfg<RT>::NW;
  const uint32_t t = threadIdx.x;
  return ew_mix32((4u * ((uint32_t)k0 + t / NW) + t % NW) ^ key);
}

// v of the lane groups 0..3 of this lane's column, added in group order: the same in all 4 lanes
__device__ __forceinline__ float ap_groups(float v, int ln) {
  const float x0 = __shfl(v, ln, 64), x1 = __shfl(v, ln + 16, 64);
  const float x2 = __shfl(v, ln + 32, 64), x3 = __shfl(v, ln + 48, 64);
  return ((x0 + x1) + x2) + x3;
}
// the sum over the 16 columns of a wave: a butterfly, the same in every lane
__device__ __forceinline__ float ap_cols(float v) {
#pragma unroll
  for (int d = 8; d > 0; d >>= 1) v = v + __shfl_xor(v, d, 64);
  return v;
}

template <int RT, int GT>
__global__ __launch_bounds__(EW_BLOCK) void k_ap_stats(ApArgs a) {
  using C = ApCfg<RT>;
  __shared__ __attribute__((aligned(16))) float lds[2 * C::PANEL];
  __shared__ float wsum[EW_WAVES][4];
  const ApItem it = a.items[blockIdx.x];
  const ApMat mt = a.mats[it.mat];
  const ApHyp h = ap_resolve(a);
  const uint32_t key = ew_stream_key(a.seed, (uint32_t)h.epoch, (uint32_t)mt.gidx);
  const int r = a.rank, c0 = AP_W * it.a;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g4 = lane >> 4, ln = lane & 15;
  const int j = c0 + 16 * w + ln;
  const bool cc = mt.cs == 1, signer = (int)threadIdx.x < AP_KS * C::NW;
  ap_f32x4 acc[C::NT];
#pragma unroll
  for (int f = 0; f < C::NT; ++f) acc[f] = ap_f32x4{0.f, 0.f, 0.f, 0.f};
  float csq = 0.0f;
  // (a) the +-g sums of the strip and its column squares
  float vb[4];
  uint32_t vw = 0;
  ap_ld_b<GT>(a.g, mt.off, mt.rs, mt.cs, cc, 0, mt.s, c0, mt.l, a.grad_scale, vb);
  if (signer) vw = ap_word<RT>(key, 0);
  ap_st_b(lds, cc, vb);
  if (signer) reinterpret_cast<uint32_t*>(lds + AP_KS * AP_LDG)[threadIdx.x] = vw;
  __syncthreads();
  const int steps = (mt.s + AP_KS - 1) / AP_KS;
  for (int s = 0; s < steps; ++s) {
    const int cur = s & 1;
    const bool more = s + 1 < steps;
    if (more) {
      const int k0 = (s + 1) * AP_KS;
      ap_ld_b<GT>(a.g, mt.off, mt.rs, mt.cs, cc, k0, mt.s, c0, mt.l, a.grad_scale, vb);
      if (signer) vw = ap_word<RT>(key, k0);
    }
    const float* pb = lds + cur * C::PANEL;
    const uint32_t* pw = reinterpret_cast<const uint32_t*>(pb + AP_KS * AP_LDG);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int kk = 4 * e + g4;
      const float b = pb[kk * AP_LDG + 16 * w + ln];
      csq = csq + b * b;
#pragma unroll
      for (int f = 0; f < C::NT; ++f) {
        // bit (16 f + ln) % 32 of word (16 f + ln) / 32 into the sign of 1.0f
        const uint32_t word = pw[kk * C::NW + f / 2];
        const uint32_t one = 0x3f800000u | ((word >> (16 * (f & 1) + ln)) << 31);
        const float av = 16 * f + ln < r ? __uint_as_float(one) : 0.0f;
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b, acc[f], 0, 0, 0);
      }
    }
    if (more) {
      float* nb = lds + (cur ^ 1) * C::PANEL;
      ap_st_b(nb, cc, vb);
      if (signer) reinterpret_cast<uint32_t*>(nb + AP_KS * AP_LDG)[threadIdx.x] = vw;
    }
    __syncthreads();
  }
  // (b) Adam in the accumulators, the lane's share of num_j and den_j
  float num = 0.0f, den = 0.0f;
#pragma unroll
  for (int f = 0; f < C::NT; ++f) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = 16 * f + 4 * g4 + q;
      if (k < r && j < mt.l) {
        const float rv = acc[f][q] * h.rs;
        const long long e = (long long)mt.s0 + (long long)k * mt.mk + (long long)j * mt.mj;
        float m = a.m_lr[e], v = a.v_lr[e];
        const float n = ap_adam1(m, v, rv, a, h);
        a.m_lr[e] = m;
        a.v_lr[e] = v;
        num = num + n * n;
        den = den + rv * rv;
      }
    }
  }
  // (c) the column's sums across the lane groups, its scale, the strip's partial
  num = ap_groups(num, ln);
  den = ap_groups(den, ln);
  csq = ap_groups(csq, ln);
  float su = 0.0f;
  if (!a.tensor_scale) {
    const float sj = den > 0.0f ? sqrtf(num / den) : 0.0f;
    if (g4 == 0 && j < mt.l) a.sj[mt.w0 + j] = sj;
    su = (sj * sj) * csq;
  }
  num = ap_cols(num);
  den = ap_cols(den);
  su = ap_cols(su);
  csq = ap_cols(csq);
  if (lane == 0) {
    wsum[w][0] = num; wsum[w][1] = den; wsum[w][2] = su; wsum[w][3] = csq;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int c = threadIdx.x;
    a.parts[4 * (long long)(mt.it0 + it.a) + c] =
        ((wsum[0][c] + wsum[1][c]) + wsum[2][c]) + wsum[3][c];
  }
}

template <int GT>
__global__ __launch_bounds__(EW_BLOCK) void k_ap_apply(ApArgs a) {
  const ApItem it = a.aitems[blockIdx.x];
  const ApMat mt = a.mats[it.mat];
  const ApHyp h = ap_resolve(a);
  // the matrix's sums in strip order: the same in every block and thread
  double sn = 0.0, sd = 0.0, su = 0.0, sc = 0.0;
  const float* pp = a.parts + 4 * (long long)mt.it0;
  for (int z = 0; z < mt.ns; ++z) {
    sn += (double)pp[4 * z];
    sd += (double)pp[4 * z + 1];
    su += (double)pp[4 * z + 2];
    sc += (double)pp[4 * z + 3];
  }
  float st = 0.0f;
  double u = sqrt(su);
  if (a.tensor_scale) {
    st = sd > 0.0 ? (float)sqrt(sn / sd) : 0.0f;
    u = sqrt(((double)st * (double)st) * sc);
  }
  const int par = h.t & 1;
  const double up = (double)a.norms[2 * it.mat + (par ^ 1)];
  const double lim = up > 0.0 ? fmax(u / up, AP_GAMMA) / AP_GAMMA : 1.0;
  const float coef = (float)(h.step / lim);
  if (it.a == 0 && threadIdx.x == 0) a.norms[2 * it.mat + par] = (float)(u / lim);

  const int start = EW_CHUNK * it.a;
  const int left = mt.s * mt.l - start;
  const int len = left < EW_CHUNK ? left : EW_CHUNK;
  const int rowlen = mt.wide ? mt.l : mt.s;  // a row of the tensor in memory
  const float* sj = a.sj + mt.w0;
#pragma unroll 2
  for (int uu = 0; uu < EW_CU; ++uu) {
    const int i = ew_chunk_idx(uu);
    if (i >= len) break;
    const long long o = (long long)mt.off + start + i;
    const int nv = len - i >= 4 ? 4 : len - i;
    int row = (start + i) / rowlen, col = (start + i) - row * rowlen;
    float g[4], pv[4];
    if (nv == 4) {
      ew_load_grad4<GT>(a.g, o, g);
      const float4 p4 = *reinterpret_cast<const float4*>(a.p + o);
      pv[0] = p4.x; pv[1] = p4.y; pv[2] = p4.z; pv[3] = p4.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g[k] = k < nv ? ap_ld1<GT>(a.g, o + k) : 0.0f;
        pv[k] = k < nv ? a.p[o + k] : 0.0f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float sv = st;
      if (!a.tensor_scale) sv = k < nv ? sj[mt.wide ? col : row] : 0.0f;
      pv[k] = pv[k] * h.keep - (coef * sv) * (g[k] * a.grad_scale);
      if (++col == rowlen) {
        col = 0;
        ++row;
      }
    }
    if (nv == 4) {
      *reinterpret_cast<float4*>(a.p + o) = make_float4(pv[0], pv[1], pv[2], pv[3]);
      if (a.shadow) ew_st4_bf16(a.shadow + o, 4, pv);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < nv) {
          a.p[o + k] = pv[k];
          if (a.shadow) a.shadow[o + k] = ew_f2bf(pv[k]);
        }
      }
    }
  }
}

ApArgs ap_args(const ApolloArgs& h) {
  if (h.grad_dtype < 0 || h.grad_dtype > 2)
    throw std::runtime_error("ewdml apollo: unknown gradient dtype");
  if ((h.rank != 1 && (h.rank < 16 || h.rank > 128 || h.rank % 16)) || h.update_gap < 1)
    throw std::runtime_error(
        "ewdml apollo: the rank is 1 or a multiple of 16 in 16..128, the gap >= 1");
  if (h.scale_type < 0 || h.scale_type > 1)
    throw std::runtime_error("ewdml apollo: the scale type is 0 (channel) or 1 (tensor)");
  if (h.num_mats < 1 || h.num_items < 1 || h.num_aitems < 1 || !h.param || !h.grad || !h.m_lr ||
      !h.v_lr || !h.mats || !h.items || !h.aitems || !h.sj || !h.parts || !h.norms)
    throw std::runtime_error("ewdml apollo: missing operand");
  if ((h.param | h.sj | h.parts) % 16 || h.grad % 8 || h.shadow % 8 ||
      (h.m_lr | h.v_lr | h.norms | h.step | h.lr_ptr) % 4)
    throw std::runtime_error("ewdml apollo: misaligned operand");
  ApArgs a{};
  a.p = reinterpret_cast<float*>(h.param);
  a.m_lr = reinterpret_cast<float*>(h.m_lr);
  a.v_lr = reinterpret_cast<float*>(h.v_lr);
  a.g = reinterpret_cast<const void*>(h.grad);
  a.shadow = reinterpret_cast<uint16_t*>(h.shadow);
  a.mats = reinterpret_cast<const ApMat*>(h.mats);
  a.items = reinterpret_cast<const ApItem*>(h.items);
  a.aitems = reinterpret_cast<const ApItem*>(h.aitems);
  a.sj = reinterpret_cast<float*>(h.sj);
  a.parts = reinterpret_cast<float*>(h.parts);
  a.norms = reinterpret_cast<float*>(h.norms);
  a.step = reinterpret_cast<const int*>(h.step);
  a.lr_ptr = reinterpret_cast<const float*>(h.lr_ptr);
  a.rank = h.rank; a.gap = h.update_gap; a.tensor_scale = h.scale_type; a.t = h.t;
  a.seed = h.seed;
  a.lr = h.lr; a.beta1 = h.beta1; a.omb1 = (float)(1.0 - (double)h.beta1);
  a.beta2 = h.beta2; a.omb2 = (float)(1.0 - (double)h.beta2);
  a.eps = h.eps; a.weight_decay = h.weight_decay; a.scale = h.scale; a.grad_scale = h.grad_scale;
  return a;
}

}  // namespace

// k_ap_stats<RT, GT> over the strips, RT the rank rounded up to a register tile count
#define AP_BY_GT(RT)                                                                            \
  do {                                                                                          \
    if (h.grad_dtype == 0) hipLaunchKernelGGL((k_ap_stats<RT, 0>), grid, block, 0, s, a);       \
    else if (h.grad_dtype == 1) hipLaunchKernelGGL((k_ap_stats<RT, 1>), grid, block, 0, s, a);  \
    else hipLaunchKernelGGL((k_ap_stats<RT, 2>), grid, block, 0, s, a);                         \
  } while (0)

void ew_apollo_stats(const ApolloArgs& h) {
  const ApArgs a = ap_args(h);
  const dim3 grid(h.num_items), block(EW_BLOCK);
  hipStream_t s = (hipStream_t)h.stream;
  if (h.rank <= 16) AP_BY_GT(16);
  else if (h.rank <= 32) AP_BY_GT(32);
  else if (h.rank <= 64) AP_BY_GT(64);
  else AP_BY_GT(128);
  EW_CHECK_LAUNCH();
}

void ew_apollo_apply(const ApolloArgs& h) {
  const ApArgs a = ap_args(h);
  const dim3 grid(h.num_aitems), block(EW_BLOCK);
  hipStream_t s = (hipStream_t)h.stream;
  if (h.grad_dtype == 0) hipLaunchKernelGGL((k_ap_apply<0>), grid, block, 0, s, a);
  else if (h.grad_dtype == 1) hipLaunchKernelGGL((k_ap_apply<1>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_ap_apply<2>), grid, block, 0, s, a);
  EW_CHECK_LAUNCH();
}
