// 8-bit Adam over the flat parameter buffer (Dettmers et al., "8-bit Optimizers via Block-wise
// Quantization", ICLR 2022): both moments live as one byte per element plus one fp32 absmax per
// 256-element block.  gfx950, wave64.  compress/oracle.py adam8_apply defines the arithmetic and
// the format; the kernel is bitwise against it.
//
// One launch, one 256-thread workgroup per ChunkRow of the range's plan.  A quantisation block is
// 256 consecutive elements of one tensor, so a chunk holds up to 32 of them and block j of chunk c
// owns absmax slot 32 c + j.  One wave owns one block at a time (wave w takes blocks w, w + 4, ...:
// up to 8 trips), a lane 4 consecutive elements of it: a float4 of parameters, 4 gradients, and
// one 32-bit word of each moment's codes, 256 B per wave and moment.  Per trip:
//
//   dequantise   m = map_s[code_m] * absmax_m, v = map_u[code_v] * absmax_v   (maps in LDS)
//   update       ew_adam's rule; the parameter steps from the unquantised new m and v
//   reduce       the block's new absmax of m and of v: the wave's shuffle tree (common.h), no LDS
//                exchange and no barrier, since a block never leaves its wave
//   prefetch     the next trip's global loads are issued here, ahead of ...
//   requantise   x = value / absmax, code = #{k : mid[k] < x}; the codes and the two absmax go out
//
// The new moments stay in registers from the update to the requantise.  The two 256-entry maps,
// their midpoints and the quantiser's decade tables (4.25 KB) are filled into LDS once per
// workgroup behind the only barrier, with the device-step path's lr_step, which one thread forms.
//
// Quantiser: the closed form.  The maps are piecewise uniform (decade i = [10^(i-7), 10^(i-6)] cut
// into n_i equal bins, an entry per bin mean), so inside a decade the nearest entry is the bin
// that holds x.  The decade comes from a tree of three compares against constants, the bin from
// one multiply-add with the decade's (lower edge, bins per unit, first rank) read from LDS as one
// float4, and the guess is then walked to the exact answer against `mid`: down while
// mid[k - 1] >= x, up while mid[k] < x.  What the walk leaves is #{k : mid[k] < x} whatever the guess was (mid ascends), so
// the result equals torch.bucketize on the oracle's midpoints bit for bit and the closed form only
// decides how many compares it takes: two when the guess is right, three just above a decade's
// edge, where the last narrow bin of the decade below reaches a bin width into this one.  That is
// 3 to 4 LDS reads per value where the 8-step binary search makes 8 dependent ones; with two
// values per element the search would be the kernel's largest LDS consumer by far.
//
// A short last block or chunk: a lane whose 4 elements are not all inside the tensor loads and
// stores its valid ones one by one; elements past the end enter neither absmax and are never
// written, so alignment padding between tensors is untouched.
#include "common.h"
#include "ewdml_ops.h"

namespace {

#define A8_QBLOCK 256                      // elements per quantisation block
#define A8_SLOTS (EW_CHUNK / A8_QBLOCK)    // absmax slots per chunk
#define A8_ZERO 127u                       // code of 0.0 in the signed map
// float offsets into the table (ops.Adam8Plan lays it out; ewdml_ops.h EW_ADAM8_TABLE_FLOATS)
#define A8_MAP_S 0
#define A8_MAP_U 256
#define A8_MID_S 512
#define A8_MID_U 768
#define A8_DEC_S 1024  // 8 x float4 {lower edge, bins per unit, first rank, 0}
#define A8_DEC_U 1056

struct A8Args {
  float* p;
  uint8_t* cm;
  uint8_t* cv;
  float* am;
  float* av;
  const void* g;
  uint16_t* shadow;
  const ChunkRow* chunks;
  const float* table;
  const int* step;      // nullable device step counter, as AdamFlatArgs.step
  const float* lr_ptr;  // nullable device base lr
  double lr;
  float lr_step, beta1, beta2, eps, weight_decay, grad_scale;
};

// ew_adam_resolve's rule (optim.hip): lr_step of step t = *step + 1 from the fp32 betas in double
__device__ __forceinline__ void a8_resolve(A8Args& a) {
  if (a.step) {
    const double t = (double)(*a.step + 1);
    const double lr = a.lr_ptr ? (double)*a.lr_ptr : a.lr;
    a.lr_step = (float)(lr * sqrt(1.0 - pow((double)a.beta2, t)) /
                        (1.0 - pow((double)a.beta1, t)));
  }
}

// what a lane holds of one quantisation block: 4 consecutive elements, n of them inside the tensor
struct A8Trip {
  float p[4], g[4];
  uint32_t cm, cv;  // 4 codes each, element k in byte k
  float am, av;     // the block's absmax of the last step
  int n;
  long long o;      // offset of the lane's first element in the range
};

template <int GT>
__device__ __forceinline__ float a8_ld1(const void* g, long long i) {
  if (GT == 0) return reinterpret_cast<const float*>(g)[i];
  if (GT == 1) return ew_bf16f(reinterpret_cast<const uint16_t*>(g)[i]);
  return __half2float(reinterpret_cast<const __half*>(g)[i]);
}

template <int GT>
__device__ __forceinline__ void a8_load(const A8Args& a, const ChunkRow& c, int j, int lane,
                                        A8Trip& t) {
  const int i = A8_QBLOCK * j + 4 * lane;
  const int left = c.len - i;
  t.n = left >= 4 ? 4 : (left > 0 ? left : 0);
  t.o = (long long)c.start + i;
  t.am = a.am[A8_SLOTS * blockIdx.x + j];
  t.av = a.av[A8_SLOTS * blockIdx.x + j];
  if (t.n == 4) {
    const float4 pv = *reinterpret_cast<const float4*>(a.p + t.o);
    t.p[0] = pv.x; t.p[1] = pv.y; t.p[2] = pv.z; t.p[3] = pv.w;
    ew_load_grad4<GT>(a.g, t.o, t.g);
    t.cm = *reinterpret_cast<const uint32_t*>(a.cm + t.o);
    t.cv = *reinterpret_cast<const uint32_t*>(a.cv + t.o);
  } else {
    t.cm = A8_ZERO * 0x01010101u;
    t.cv = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      t.p[k] = 0.0f;
      t.g[k] = 0.0f;
      if (k < t.n) {
        t.p[k] = a.p[t.o + k];
        t.g[k] = a8_ld1<GT>(a.g, t.o + k);
        t.cm = (t.cm & ~(0xffu << (8 * k))) | ((uint32_t)a.cm[t.o + k] << (8 * k));
        t.cv |= (uint32_t)a.cv[t.o + k] << (8 * k);
      }
    }
  }
}

// #{k : mid[k] < x} over the 255 ascending midpoints, walked from the guess k
__device__ __forceinline__ uint32_t a8_walk(const float* mid, float x, int k) {
  k = k < 0 ? 0 : (k > 255 ? 255 : k);
  while (k > 0 && !(mid[k - 1] < x)) --k;
  while (k < 255 && mid[k] < x) ++k;
  return (uint32_t)k;
}

// rank of a >= 0 among the non-negative entries of a map (0 = the entry 0.0), closed-form guess
__device__ __forceinline__ int a8_rank(const float4* dec, float a) {
  const int d = a >= 1e-4f ? (a >= 1e-2f ? (a >= 1e-1f ? 7 : 6) : (a >= 1e-3f ? 5 : 4))
                           : (a >= 1e-6f ? (a >= 1e-5f ? 3 : 2) : (a >= 1e-7f ? 1 : 0));
  const float4 e = dec[d];
  return (int)((a - e.x) * e.y + e.z);
}

__device__ __forceinline__ uint32_t a8_quant_m(const float* lds, float m, float amax) {
  const float x = amax > 0.0f ? m / amax : 0.0f;
  const int r = a8_rank(reinterpret_cast<const float4*>(lds + A8_DEC_S), fabsf(x));
  return a8_walk(lds + A8_MID_S, x, x < 0.0f ? (int)A8_ZERO - r : (int)A8_ZERO + r);
}

__device__ __forceinline__ uint32_t a8_quant_v(const float* lds, float v, float amax) {
  const float x = amax > 0.0f ? v / amax : 0.0f;
  const uint32_t k = a8_walk(lds + A8_MID_U, x,
                             a8_rank(reinterpret_cast<const float4*>(lds + A8_DEC_U), x));
  return (v > 0.0f && k == 0u) ? 1u : k;  // a v > 0 never dequantises to 0
}

// the wave's maximum of non-negative floats, in every lane (bit patterns order as the values do)
__device__ __forceinline__ float a8_wave_max(float v) {
  return __uint_as_float(__shfl(ew_wave_max_u(__float_as_uint(v)), 0, 64));
}

template <int GT>
__global__ __launch_bounds__(EW_BLOCK) void k_adam8(A8Args a) {
  __shared__ float4 lds4[EW_ADAM8_TABLE_FLOATS / 4];
  float* lds = reinterpret_cast<float*>(lds4);
  __shared__ float lr_step_s;
  for (int k = threadIdx.x; k < EW_ADAM8_TABLE_FLOATS; k += EW_BLOCK) lds[k] = a.table[k];
  if (threadIdx.x == 0) {  // the double pow of the device-step path once per workgroup
    a8_resolve(a);
    lr_step_s = a.lr_step;
  }
  const ChunkRow c = a.chunks[blockIdx.x];
  const float omb1 = 1.0f - a.beta1, omb2 = 1.0f - a.beta2;
  const int lane = threadIdx.x & 63;
  const int nblk = (c.len + A8_QBLOCK - 1) / A8_QBLOCK;
  __syncthreads();
  a.lr_step = lr_step_s;

  int j = threadIdx.x >> 6;
  A8Trip t;
  if (j < nblk) a8_load<GT>(a, c, j, lane, t);
  for (; j < nblk; j += EW_WAVES) {
    const int n = t.n;
    const long long o = t.o;
    float m[4], v[4];
    float mx = 0.0f, vx = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      m[k] = lds[A8_MAP_S + ((t.cm >> (8 * k)) & 0xffu)] * t.am;
      v[k] = lds[A8_MAP_U + ((t.cv >> (8 * k)) & 0xffu)] * t.av;
      float g = t.g[k] * a.grad_scale;
      if (a.weight_decay != 0.0f) g = g + a.weight_decay * t.p[k];
      m[k] = m[k] * a.beta1 + omb1 * g;
      v[k] = v[k] * a.beta2 + omb2 * (g * g);
      t.p[k] = t.p[k] - a.lr_step * (m[k] / (sqrtf(v[k]) + a.eps));
      if (k >= n) { m[k] = 0.0f; v[k] = 0.0f; }
      mx = fmaxf(mx, fabsf(m[k]));
      vx = fmaxf(vx, v[k]);
    }
    if (n == 4) {
      *reinterpret_cast<float4*>(a.p + o) = make_float4(t.p[0], t.p[1], t.p[2], t.p[3]);
      if (a.shadow) ew_st4_bf16(a.shadow + o, 4, t.p);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < n) {
          a.p[o + k] = t.p[k];
          if (a.shadow) a.shadow[o + k] = ew_f2bf(t.p[k]);
        }
      }
    }
    mx = a8_wave_max(mx);
    vx = a8_wave_max(vx);

    if (j + EW_WAVES < nblk) a8_load<GT>(a, c, j + EW_WAVES, lane, t);  // under the requantise

    uint32_t wm = 0u, wv = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      wm |= a8_quant_m(lds, m[k], mx) << (8 * k);
      wv |= a8_quant_v(lds, v[k], vx) << (8 * k);
    }
    if (n == 4) {
      *reinterpret_cast<uint32_t*>(a.cm + o) = wm;
      *reinterpret_cast<uint32_t*>(a.cv + o) = wv;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < n) {
          a.cm[o + k] = (uint8_t)(wm >> (8 * k));
          a.cv[o + k] = (uint8_t)(wv >> (8 * k));
        }
      }
    }
    if (lane == 0) {
      a.am[A8_SLOTS * blockIdx.x + j] = mx;
      a.av[A8_SLOTS * blockIdx.x + j] = vx;
    }
  }
}

}  // namespace

void ew_adam8_step(const Adam8Args& h) {
  if (h.grad_dtype < 0 || h.grad_dtype > 2)
    throw std::runtime_error("ewdml adam8: unknown gradient dtype");
  if (h.num_chunks < 1 || !h.param || !h.grad || !h.code_m || !h.code_v || !h.absmax_m ||
      !h.absmax_v || !h.chunks || !h.table)
    throw std::runtime_error("ewdml adam8: missing operand");
  A8Args a{};
  a.p = reinterpret_cast<float*>(h.param);
  a.cm = reinterpret_cast<uint8_t*>(h.code_m);
  a.cv = reinterpret_cast<uint8_t*>(h.code_v);
  a.am = reinterpret_cast<float*>(h.absmax_m);
  a.av = reinterpret_cast<float*>(h.absmax_v);
  a.g = reinterpret_cast<const void*>(h.grad);
  a.shadow = reinterpret_cast<uint16_t*>(h.shadow);
  a.chunks = reinterpret_cast<const ChunkRow*>(h.chunks);
  a.table = reinterpret_cast<const float*>(h.table);
  a.step = reinterpret_cast<const int*>(h.step);
  a.lr_ptr = reinterpret_cast<const float*>(h.lr_ptr);
  a.lr = h.lr;
  a.lr_step = h.lr_step; a.beta1 = h.beta1; a.beta2 = h.beta2; a.eps = h.eps;
  a.weight_decay = h.weight_decay; a.grad_scale = h.grad_scale;
  const dim3 grid(h.num_chunks), block(EW_BLOCK);
  hipStream_t s = (hipStream_t)h.stream;
  if (h.grad_dtype == 0) hipLaunchKernelGGL(k_adam8<0>, grid, block, 0, s, a);
  else if (h.grad_dtype == 1) hipLaunchKernelGGL(k_adam8<1>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_adam8<2>, grid, block, 0, s, a);
  EW_CHECK_LAUNCH();
}
