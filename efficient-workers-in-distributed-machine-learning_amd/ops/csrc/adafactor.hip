// Adafactor over the flat parameter buffer (Shazeer and Stern, ICML 2018) with an external
// learning rate: every dim >= 2 tensor, viewed as [n, m] = [shape[0], numel / shape[0]], keeps one
// row vector R and one column vector C of second-moment statistics instead of n m values; a vector
// keeps its full v.  gfx950, wave64.  compress/oracle.py adafactor_apply defines the arithmetic.
//
// The work of a flat range (a bucket or the whole model) is a list built once (ops.AdafactorPlan):
// the matrix tiles first, AF_ROWS x AF_COLS = 32 x 256 elements each (the size of a chunk), then
// one item per 8192-element chunk row of a vector.  A workgroup is 256 threads; in a tile wave w
// takes rows w, w + 4, ... (8 of them) and lane l columns 4 l .. 4 l + 3: one 16-byte load per row
// when m % 4 == 0 (tensor offsets are multiples of 4), dword loads otherwise, chosen per matrix.
// All of a lane's loads are issued before the first is used.  A step is four launches:
//
//   k_af_stats   (tiles) q = g^2 + 1e-30.  Row partial: the lane's 4 values in order, then the
//                wave's shuffle tree -> rowpart[strip][row].  Column partial: a lane accumulates
//                its 4 columns over its rows in row order, the four waves are combined through LDS
//                in wave order -> colpart[band][col].
//   k_af_factor  one block per 256 rows or 256 columns of a matrix, a thread per entry: the strip
//                (band) partials summed in index order in fp64, the mean rounded to fp32 once, R
//                (C) updated in place -- the only writer of the state -- and 1 / sqrt(C) written to
//                the cfac workspace.  A row block also leaves the fp64 sum of its new R in rsum.
//   k_af_rms     (all items) u and one partial {sum u^2, sum p^2} per item; a vector's v is updated
//                here.  p is read only in the scale-parameter instantiation.
//   k_af_apply   (all items) every block sums its tensor's item partials in fp64 in a fixed order,
//                so all blocks of a tensor hold the same clip factor and alpha with no grid
//                barrier; u is recomputed, the step applied, mom updated when beta1 > 0, and p and
//                the bf16 shadow written.
//
// mean(R) is the fp64 sum of rsum's entries (lane-strided, then the wave tree) over n; the tile's
// waves form it and 1 / sqrt(R_i / mean R) themselves, as a matrix's R is spread over many factor
// blocks: one block per matrix would walk all its partials (83 k of them for a 512 x 4608 filter)
// behind a single workgroup.
//
// No float atomics: every sum is a fixed tree, so a step is bitwise reproducible and does not
// depend on whether a tensor is stepped with its bucket or with the whole model.  beta2_t and lr
// are read from device memory when given, so a captured step replays the current ones.  With a
// step counter beta2_t is the device's double pow, the oracle's is Python's: the two may differ in
// the last fp64 bit, and at a step where that bit decides the rounding to fp32 the state differs
// from the oracle's by one ulp of beta2_t (runs on the device still agree with each other).
//
// Longest chain of fp32 additions behind a row or a column sum, L = 11
// (ops.ADAFACTOR_SUM_CHAIN).  Row: 4 values into a zero accumulator (4) + 6 shuffle levels = 10.
// Column: 8 rows into a zero accumulator (8) + the four waves in order (3) = 11.  The first
// addition of either chain is 0 + q, which is exact, so L roundings also cover the one of q's own
// g * g (dropping the + 1e-30 costs a relative 1e-30 / g^2, under 2^-60 for |g| > 2e-6; where
// g = 0, q is the constant itself).  The sums over strips and bands are fp64 and are rounded to fp32 once, with the
// division of the mean.
#include "common.h"
#include "ewdml_ops.h"

namespace {

#define AF_ROWS EW_AF_ROWS
#define AF_COLS EW_AF_COLS
#define AF_RPW (AF_ROWS / EW_WAVES)  // rows of a tile per wave
#define AF_EPS1 1e-30f
#define AF_EPS2 1e-3

struct AfItem {  // a tile (tens[tensor].n > 0): band, strip; a vector chunk: start in the range, len
  int tensor, a, b, pad;
};
struct AfTen {  // mirrors ops.AdafactorPlan.tens
  // s0 / s1: offset of R / C in row / col (cfac is indexed like col), or s0 of v for a vector;
  // rp0 / cp0 / rs0: the matrix's rows of rowpart [nstrips, n], colpart [nbands, m], rsum [nsegs]
  int off, numel, n, m, item0, nitems, s0, s1, rp0, cp0, rs0, nbands, nstrips, nsegs, pad0, pad1;
};
struct AfFItem {  // k_af_factor: entries [256 seg, 256 seg + 256) of R (is_col 0) or of C
  int tensor, is_col, seg, pad;
};

struct AfArgs {
  float* p;
  float* row;
  float* col;
  float* v;
  float* mom;
  const void* g;
  uint16_t* shadow;
  const AfItem* items;
  const AfTen* tens;
  const AfFItem* fitems;
  float* rowpart;
  float* colpart;
  float* cfac;
  double* rsum;
  float* partials;
  const int* step;      // nullable device step counter: t = *step + 1
  const float* lr_ptr;  // nullable device lr
  double decay;
  float lr, beta1, omb1, clip, weight_decay, grad_scale, b2, omb2;
};

// lr and beta2_t = 1 - t^-decay (formed in double, rounded once) from device memory
__device__ __forceinline__ void af_resolve(AfArgs& a) {
  if (a.lr_ptr) a.lr = *a.lr_ptr;
  if (a.step) {
    const double b2 = 1.0 - pow((double)(*a.step + 1), -a.decay);
    a.b2 = (float)b2;
    a.omb2 = (float)(1.0 - b2);
  }
}

template <int GT>
__device__ __forceinline__ float af_ld1(const void* g, long long i) {
  if (GT == 0) return reinterpret_cast<const float*>(g)[i];
  if (GT == 1) return ew_bf16f(reinterpret_cast<const uint16_t*>(g)[i]);
  return __half2float(reinterpret_cast<const __half*>(g)[i]);
}

// A lane's 4 consecutive elements at offset o, nv of them inside the row; vec: one 16-byte access
template <int GT>
__device__ __forceinline__ void af_ldg(const void* g, long long o, int nv, bool vec, float out[4]) {
  if (vec) {
    ew_load_grad4<GT>(g, o, out);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = k < nv ? af_ld1<GT>(g, o + k) : 0.0f;
  }
}
__device__ __forceinline__ void af_ldf(const float* s, long long o, int nv, bool vec, float out[4]) {
  af_ldg<0>(s, o, nv, vec, out);
}
__device__ __forceinline__ void af_stf(float* d, long long o, int nv, bool vec, const float x[4]) {
  if (vec) {
    *reinterpret_cast<float4*>(d + o) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nv) d[o + k] = x[k];
  }
}

// where a lane stands in its tile
struct AfLane {
  int i0;     // the wave's first row; its rows are i0 + 4 r, r < AF_RPW, while < n
  int j;      // the lane's first column
  int nv;     // its columns inside the matrix: 0..4
  bool vec;   // 16-byte accesses (m % 4 == 0, so nv is 4)
};
__device__ __forceinline__ AfLane af_lane(const AfItem& it, const AfTen& T) {
  AfLane L;
  L.i0 = AF_ROWS * it.a + (int)(threadIdx.x >> 6);
  L.j = AF_COLS * it.b + 4 * (int)(threadIdx.x & 63);
  const int left = T.m - L.j;
  L.nv = left >= 4 ? 4 : (left > 0 ? left : 0);
  L.vec = (T.m & 3) == 0 && L.nv == 4;
  return L;
}
__device__ __forceinline__ long long af_at(const AfTen& T, int i, int j) {
  return (long long)T.off + (long long)i * T.m + j;
}

__device__ __forceinline__ double af_wave_sum_d(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// mean(R) of a matrix, the same value in every lane of every wave of every block
__device__ __forceinline__ float af_mean_r(const AfArgs& a, const AfTen& T) {
  double s = 0.0;
  for (int k = threadIdx.x & 63; k < T.nsegs; k += 64) s += a.rsum[T.rs0 + k];
  s = __shfl(af_wave_sum_d(s), 0, 64);
  return (float)(s / (double)T.n);
}

template <int GT>
__global__ __launch_bounds__(EW_BLOCK) void k_af_stats(AfArgs a) {
  __shared__ float cs[EW_WAVES][AF_COLS];
  const AfItem it = a.items[blockIdx.x];
  const AfTen T = a.tens[it.tensor];
  const AfLane L = af_lane(it, T);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float g[AF_RPW][4];
#pragma unroll
  for (int r = 0; r < AF_RPW; ++r) {
    const int i = L.i0 + EW_WAVES * r;
    if (i < T.n) af_ldg<GT>(a.g, af_at(T, i, L.j), L.nv, L.vec, g[r]);
  }
  float ca[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int r = 0; r < AF_RPW; ++r) {
    const int i = L.i0 + EW_WAVES * r;
    if (i >= T.n) break;  // uniform in the wave
    float rs = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < L.nv) {
        const float x = g[r][k] * a.grad_scale;
        const float q = x * x + AF_EPS1;
        rs += q;
        ca[k] += q;
      }
    }
    rs = ew_wave_sum(rs);
    if (lane == 0) a.rowpart[T.rp0 + (long long)it.b * T.n + i] = rs;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) cs[w][4 * lane + k] = ca[k];
  __syncthreads();
  const int t = threadIdx.x, j = AF_COLS * it.b + t;
  float s = cs[0][t];
#pragma unroll
  for (int i = 1; i < EW_WAVES; ++i) s += cs[i][t];
  if (j < T.m) a.colpart[T.cp0 + (long long)it.a * T.m + j] = s;
}

__global__ __launch_bounds__(EW_BLOCK) void k_af_factor(AfArgs a) {
  __shared__ double wd[EW_WAVES];
  af_resolve(a);
  const AfFItem f = a.fitems[blockIdx.x];
  const AfTen T = a.tens[f.tensor];
  const int e = EW_BLOCK * f.seg + (int)threadIdx.x;
  if (f.is_col) {
    if (e >= T.m) return;
    double s = 0.0;
    for (int b = 0; b < T.nbands; ++b) s += (double)a.colpart[T.cp0 + (long long)b * T.m + e];
    const float mean = (float)(s / (double)T.n);
    const float c = a.col[T.s1 + e] * a.b2 + a.omb2 * mean;
    a.col[T.s1 + e] = c;
    a.cfac[T.s1 + e] = 1.0f / sqrtf(c);
    return;
  }
  double r64 = 0.0;
  if (e < T.n) {
    double s = 0.0;
    for (int b = 0; b < T.nstrips; ++b) s += (double)a.rowpart[T.rp0 + (long long)b * T.n + e];
    const float mean = (float)(s / (double)T.m);
    const float r = a.row[T.s0 + e] * a.b2 + a.omb2 * mean;
    a.row[T.s0 + e] = r;
    r64 = (double)r;
  }
  r64 = af_wave_sum_d(r64);
  if ((threadIdx.x & 63) == 0) wd[threadIdx.x >> 6] = r64;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = wd[0];
#pragma unroll
    for (int i = 1; i < EW_WAVES; ++i) s += wd[i];
    a.rsum[T.rs0 + f.seg] = s;
  }
}

// the block's two sums in a fixed order -> partials[2 item], [2 item + 1]
__device__ __forceinline__ void af_put_partials(const AfArgs& a, float su, float sp, float* ws) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  su = ew_wave_sum(su);
  sp = ew_wave_sum(sp);
  if (lane == 0) { ws[w] = su; ws[EW_WAVES + w] = sp; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tu = ws[0], tp = ws[EW_WAVES];
#pragma unroll
    for (int i = 1; i < EW_WAVES; ++i) { tu += ws[i]; tp += ws[EW_WAVES + i]; }
    a.partials[2 * blockIdx.x] = tu;
    a.partials[2 * blockIdx.x + 1] = tp;
  }
}

// SP: the scale-parameter instantiation, the only one that reads p
template <int GT, int SP>
__global__ __launch_bounds__(EW_BLOCK) void k_af_rms(AfArgs a) {
  __shared__ float ws[2 * EW_WAVES];
  const AfItem it = a.items[blockIdx.x];
  const AfTen T = a.tens[it.tensor];
  float su = 0.0f, sp = 0.0f;
  if (T.n > 0) {
    const AfLane L = af_lane(it, T);
    float g[AF_RPW][4], p[AF_RPW][4], cf[4];
#pragma unroll
    for (int r = 0; r < AF_RPW; ++r) {
      const int i = L.i0 + EW_WAVES * r;
      if (i < T.n) {
        af_ldg<GT>(a.g, af_at(T, i, L.j), L.nv, L.vec, g[r]);
        if (SP) af_ldf(a.p, af_at(T, i, L.j), L.nv, L.vec, p[r]);
      }
    }
    af_ldf(a.cfac, (long long)T.s1 + L.j, L.nv, L.vec, cf);
    const float mr = af_mean_r(a, T);
#pragma unroll
    for (int r = 0; r < AF_RPW; ++r) {
      const int i = L.i0 + EW_WAVES * r;
      if (i >= T.n) break;
      const float rf = 1.0f / sqrtf(a.row[T.s0 + i] / mr);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < L.nv) {
          const float u = ((g[r][k] * a.grad_scale) * rf) * cf[k];
          su += u * u;
          if (SP) sp += p[r][k] * p[r][k];
        }
      }
    }
  } else {  // a vector's chunk row: v is updated and stored here
    af_resolve(a);
    float* v = a.v + T.s0 + (it.a - T.off);
#pragma unroll 2
    for (int c = 0; c < EW_CU; ++c) {
      const int i = ew_chunk_idx(c);
      if (i >= it.b) break;
      const int nv = it.b - i >= 4 ? 4 : it.b - i;
      const bool vec = nv == 4;
      float g[4], x[4], pv[4];
      af_ldg<GT>(a.g, (long long)it.a + i, nv, vec, g);
      af_ldf(v, i, nv, vec, x);
      if (SP) af_ldf(a.p, (long long)it.a + i, nv, vec, pv);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < nv) {
          const float gs = g[k] * a.grad_scale;
          x[k] = x[k] * a.b2 + a.omb2 * (gs * gs + AF_EPS1);
          const float u = gs / sqrtf(x[k]);
          su += u * u;
          if (SP) sp += pv[k] * pv[k];
        }
      }
      af_stf(v, i, nv, vec, x);
    }
  }
  af_put_partials(a, su, sp, ws);
}

// a = alpha / max(1, RMS(u) / clip) and 1 - alpha wd of the block's tensor, the same values in
// every thread of every block of the tensor: thread i adds items i, i + 256, ... in order in
// fp64, then the wave tree and the four waves in order
template <int SP>
__device__ __forceinline__ void af_scalars(const AfArgs& a, const AfTen& T, double* wd, float* sc,
                                           float& step, float& keep) {
  double su = 0.0, sp = 0.0;
  for (int j = threadIdx.x; j < T.nitems; j += EW_BLOCK) {
    su += (double)a.partials[2 * (T.item0 + j)];
    if (SP) sp += (double)a.partials[2 * (T.item0 + j) + 1];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  su = af_wave_sum_d(su);
  sp = af_wave_sum_d(sp);
  if (lane == 0) { wd[w] = su; wd[EW_WAVES + w] = sp; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tu = wd[0], tp = wd[EW_WAVES];
#pragma unroll
    for (int i = 1; i < EW_WAVES; ++i) { tu += wd[i]; tp += wd[EW_WAVES + i]; }
    const double den = fmax(1.0, sqrt(tu / (double)T.numel) / (double)a.clip);
    float alpha = a.lr;
    if (SP) alpha = (float)((double)a.lr * fmax(AF_EPS2, sqrt(tp / (double)T.numel)));
    sc[0] = (float)((double)alpha / den);
    sc[1] = (float)(1.0 - (double)alpha * (double)a.weight_decay);
  }
  __syncthreads();
  step = sc[0];
  keep = sc[1];
}

// one element: the step (through mom when MOM) and the parameter
template <int MOM>
__device__ __forceinline__ void af_step1(float& p, float& mo, float u, float step, float keep,
                                         const AfArgs& a) {
  float s = u * step;
  if (MOM) {
    mo = mo * a.beta1 + s * a.omb1;
    s = mo;
  }
  p = p * keep - s;
}

template <int GT, int SP, int MOM>
__global__ __launch_bounds__(EW_BLOCK) void k_af_apply(AfArgs a) {
  __shared__ double wd[2 * EW_WAVES];
  __shared__ float sc[2];
  if (a.lr_ptr) a.lr = *a.lr_ptr;
  const AfItem it = a.items[blockIdx.x];
  const AfTen T = a.tens[it.tensor];
  float step, keep;
  af_scalars<SP>(a, T, wd, sc, step, keep);
  if (T.n > 0) {
    const AfLane L = af_lane(it, T);
    float g[AF_RPW][4], p[AF_RPW][4], mo[AF_RPW][4], cf[4];
#pragma unroll
    for (int r = 0; r < AF_RPW; ++r) {
      const int i = L.i0 + EW_WAVES * r;
      if (i < T.n) {
        const long long o = af_at(T, i, L.j);
        af_ldg<GT>(a.g, o, L.nv, L.vec, g[r]);
        af_ldf(a.p, o, L.nv, L.vec, p[r]);
        if (MOM) af_ldf(a.mom, o, L.nv, L.vec, mo[r]);
      }
    }
    af_ldf(a.cfac, (long long)T.s1 + L.j, L.nv, L.vec, cf);
    const float mr = af_mean_r(a, T);
#pragma unroll
    for (int r = 0; r < AF_RPW; ++r) {
      const int i = L.i0 + EW_WAVES * r;
      if (i >= T.n) break;
      const long long o = af_at(T, i, L.j);
      const float rf = 1.0f / sqrtf(a.row[T.s0 + i] / mr);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float u = ((g[r][k] * a.grad_scale) * rf) * cf[k];
        af_step1<MOM>(p[r][k], mo[r][k], u, step, keep, a);
      }
      af_stf(a.p, o, L.nv, L.vec, p[r]);
      if (MOM) af_stf(a.mom, o, L.nv, L.vec, mo[r]);
      if (a.shadow) {
        if (L.vec) {
          ew_st4_bf16(a.shadow + o, 4, p[r]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < L.nv) a.shadow[o + k] = ew_f2bf(p[r][k]);
        }
      }
    }
  } else {
    const float* v = a.v + T.s0 + (it.a - T.off);
#pragma unroll 2
    for (int c = 0; c < EW_CU; ++c) {
      const int i = ew_chunk_idx(c);
      if (i >= it.b) break;
      const int nv = it.b - i >= 4 ? 4 : it.b - i;
      const bool vec = nv == 4;
      const long long o = (long long)it.a + i;
      float g[4], x[4], pv[4], mo[4];
      af_ldg<GT>(a.g, o, nv, vec, g);
      af_ldf(v, i, nv, vec, x);
      af_ldf(a.p, o, nv, vec, pv);
      if (MOM) af_ldf(a.mom, o, nv, vec, mo);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < nv) {
          const float u = (g[k] * a.grad_scale) / sqrtf(x[k]);
          af_step1<MOM>(pv[k], mo[k], u, step, keep, a);
        }
      }
      af_stf(a.p, o, nv, vec, pv);
      if (MOM) af_stf(a.mom, o, nv, vec, mo);
      if (a.shadow) {
        if (vec) {
          ew_st4_bf16(a.shadow + o, 4, pv);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < nv) a.shadow[o + k] = ew_f2bf(pv[k]);
        }
      }
    }
  }
}

AfArgs af_args(const AdafactorArgs& h) {
  if (h.grad_dtype < 0 || h.grad_dtype > 2)
    throw std::runtime_error("ewdml adafactor: unknown gradient dtype");
  if (h.num_items < 1 || h.num_tiles < 0 || h.num_tiles > h.num_items || h.num_fitems < 0 ||
      !h.param || !h.grad || !h.items || !h.tensors || !h.partials ||
      (h.num_tiles > 0 && (h.num_fitems < 1 || !h.row || !h.col || !h.fitems || !h.rowpart ||
                           !h.colpart || !h.cfac || !h.rsum)) ||
      (h.num_tiles < h.num_items && !h.v) || (h.beta1 != 0.0f && !h.mom))
    throw std::runtime_error("ewdml adafactor: missing operand");
  AfArgs a{};
  a.p = reinterpret_cast<float*>(h.param);
  a.row = reinterpret_cast<float*>(h.row);
  a.col = reinterpret_cast<float*>(h.col);
  a.v = reinterpret_cast<float*>(h.v);
  a.mom = reinterpret_cast<float*>(h.mom);
  a.g = reinterpret_cast<const void*>(h.grad);
  a.shadow = reinterpret_cast<uint16_t*>(h.shadow);
  a.items = reinterpret_cast<const AfItem*>(h.items);
  a.tens = reinterpret_cast<const AfTen*>(h.tensors);
  a.fitems = reinterpret_cast<const AfFItem*>(h.fitems);
  a.rowpart = reinterpret_cast<float*>(h.rowpart);
  a.colpart = reinterpret_cast<float*>(h.colpart);
  a.cfac = reinterpret_cast<float*>(h.cfac);
  a.rsum = reinterpret_cast<double*>(h.rsum);
  a.partials = reinterpret_cast<float*>(h.partials);
  a.step = reinterpret_cast<const int*>(h.step);
  a.lr_ptr = reinterpret_cast<const float*>(h.lr_ptr);
  a.decay = h.decay;
  a.lr = h.lr; a.beta1 = h.beta1; a.omb1 = (float)(1.0 - (double)h.beta1); a.clip = h.clip;
  a.weight_decay = h.weight_decay; a.grad_scale = h.grad_scale;
  a.b2 = h.beta2; a.omb2 = h.omb2;
  return a;
}

}  // namespace

#define AF_BY_GT(K, N, ...)                                                                     \
  do {                                                                                          \
    const dim3 grid(N), block(EW_BLOCK);                                                        \
    hipStream_t s = (hipStream_t)h.stream;                                                      \
    if (h.grad_dtype == 0) hipLaunchKernelGGL((K<0, ##__VA_ARGS__>), grid, block, 0, s, a);     \
    else if (h.grad_dtype == 1) hipLaunchKernelGGL((K<1, ##__VA_ARGS__>), grid, block, 0, s, a); \
    else hipLaunchKernelGGL((K<2, ##__VA_ARGS__>), grid, block, 0, s, a);                       \
  } while (0)

void ew_adafactor_stats(const AdafactorArgs& h) {
  const AfArgs a = af_args(h);
  if (h.num_tiles < 1) return;  // a range of vectors
  AF_BY_GT(k_af_stats, h.num_tiles);
  EW_CHECK_LAUNCH();
}

void ew_adafactor_factor(const AdafactorArgs& h) {
  const AfArgs a = af_args(h);
  if (h.num_tiles < 1) return;
  hipLaunchKernelGGL(k_af_factor, dim3(h.num_fitems), dim3(EW_BLOCK), 0, (hipStream_t)h.stream, a);
  EW_CHECK_LAUNCH();
}

void ew_adafactor_rms(const AdafactorArgs& h) {
  const AfArgs a = af_args(h);
  if (h.scale_parameter) AF_BY_GT(k_af_rms, h.num_items, 1);
  else AF_BY_GT(k_af_rms, h.num_items, 0);
  EW_CHECK_LAUNCH();
}

void ew_adafactor_apply(const AdafactorArgs& h) {
  const AfArgs a = af_args(h);
  const int mom = h.beta1 != 0.0f;
  if (h.scale_parameter && mom) AF_BY_GT(k_af_apply, h.num_items, 1, 1);
  else if (h.scale_parameter) AF_BY_GT(k_af_apply, h.num_items, 1, 0);
  else if (mom) AF_BY_GT(k_af_apply, h.num_items, 0, 1);
  else AF_BY_GT(k_af_apply, h.num_items, 0, 0);
  EW_CHECK_LAUNCH();
}
