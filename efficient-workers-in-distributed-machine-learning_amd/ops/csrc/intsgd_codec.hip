// IntSGD (Mishchenko, Wang, Kovalev, Richtarik, ICLR 2022): every rank multiplies its gradient by
// the same scale alpha, rounds stochastically to integers in [-q, q], q = floor(127 / world), and
// the int8 codes are summed by a plain all-reduce; the receive side reads the one summed row.
// gfx950, wave64.  compress/oracle.py encode_intsgd / intsgd_apply / intsgd_alpha define every bit.
//
// Payload (compress/plan.py `intsgd`): codes i8[L], L the bucket's padded length; element i of the
// bucket is byte i.  As in mx_codec.hip a chunk row owns the positions from its start to the next
// row's start (the bucket's end for the last row), so the zeros of the pads behind a tensor are
// written by its last row and every byte of the payload is written by every encode.
//
// The scale lives in device memory (IntState, one per model) and is never a kernel argument, so a
// captured step follows it:
//   k_int_encode<EF>     one launch per bucket, one block per chunk row.  A thread owns the 16
//                        consecutive elements [16 t, 16 t + 16) of each half of the row: four
//                        16-byte loads (two 8-byte ones of a bf16 gradient) and one whole 16-byte
//                        store of codes per half; no read-modify-write, no scratch, no atomics,
//                        and no LDS but the four words that hand the waves' saturation counts to
//                        thread 0.
//   k_int_decode_apply   one launch per bucket: g^ = float(int8 sum) * inv_na, ew_sgd, the bf16
//                        shadow, the key advance, and the row's fp32 partial of (p_new - p_old)^2 in
//                        k_clip_norm's order (ew_ld_chunk's register layout: 32 serial terms per
//                        thread, the wave tree, the four waves): no second pass over the parameters.
//   k_int_update_norm    the same partials from the parameters and a previous copy (the dense
//                        first step; the tests' cross-check of the fused partials).
//   k_int_alpha          one block per step: the fp64 sum of all partials in index order (staged
//                        through LDS 1024 at a time, added by thread 0), the moving average r and
//                        alpha, inv_a, inv_na.
#include "common.h"
#include "ewdml_ops.h"

namespace {

struct IntState {  // ops.INTSGD_STATE_BYTES = 32
  double r, s_last;
  float alpha, inv_a, inv_na;
  int steps;
};

#define INT_PER 16                     // codes of one 16-byte store
#define INT_HALF (INT_PER * EW_BLOCK)  // a row is two halves of 4096 elements

// one element: the code in [-q, q] (a NaN codes 0) and whether y lay outside [-q, q] or was NaN
__device__ __forceinline__ int int_code(float acc, float alpha, float qf, uint32_t gidx,
                                        uint32_t key, uint32_t& sat) {
  const float y = acc * alpha;
  const float f = floorf(y);
  const float u = ew_uniform(gidx, key);
  float code = f + ((u < (y - f)) ? 1.0f : 0.0f);
  code = fminf(fmaxf(code, -qf), qf);
  if (y != y) code = 0.0f;
  sat += (y >= -qf && y <= qf) ? 0u : 1u;
  return (int)code;
}

template <bool EF>
__global__ __launch_bounds__(EW_BLOCK) void k_int_encode(
    GradPtrs gp, float* __restrict__ resid, const ChunkRow* __restrict__ chunks,
    uint8_t* __restrict__ codes, const IntState* __restrict__ st, uint32_t* __restrict__ sat,
    int length, int q, uint32_t key_arg, const uint32_t* __restrict__ keyp,
    uint32_t bucket_offset) {
  __shared__ uint32_t ws[EW_WAVES];
  const uint32_t key = keyp ? *keyp : key_arg;
  const ChunkRow c = chunks[blockIdx.x];
  // the positions this row writes: 64 | span <= EW_CHUNK (the layout's packing rule)
  const int span = (blockIdx.x + 1 < gridDim.x ? chunks[blockIdx.x + 1].start : length) - c.start;
  const float alpha = st->alpha, inv_a = st->inv_a, qf = (float)q;
  const uint32_t gbase = bucket_offset + (uint32_t)c.start;
  float x[2][INT_PER];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int k = 0; k < INT_PER / 4; ++k) {
      const int i = h * INT_HALF + INT_PER * (int)threadIdx.x + 4 * k;
      float xs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (i < c.len) ew_ld4t(gp, nullptr, c, i, xs);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[h][4 * k + j] = xs[j];
    }
  }
  if (EF) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int k = 0; k < INT_PER / 4; ++k) {
        const int i = h * INT_HALF + INT_PER * (int)threadIdx.x + 4 * k;
        float rs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i < c.len) ew_ld4t(gp, resid, c, i, rs);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[h][4 * k + j] = x[h][4 * k + j] + rs[j];
      }
    }
  }
  uint32_t nsat = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i0 = h * INT_HALF + INT_PER * (int)threadIdx.x;
    uint32_t w[INT_PER / 4];
#pragma unroll
    for (int k = 0; k < INT_PER / 4; ++k) {
      w[k] = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = i0 + 4 * k + j;
        int cd = 0;
        if (i < c.len) {  // the pad behind the tensor codes 0 and is not counted
          cd = int_code(x[h][4 * k + j], alpha, qf, gbase + (uint32_t)i, key, nsat);
          if (EF) x[h][4 * k + j] = x[h][4 * k + j] - (float)cd * inv_a;
        }
        w[k] |= ((uint32_t)cd & 0xffu) << (8 * j);
      }
    }
    if (i0 < span)  // 16 | span: the whole store lies inside the row's positions
      *reinterpret_cast<uint4*>(codes + c.start + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    if (EF) {
      float* r = resid + c.start;
#pragma unroll
      for (int k = 0; k < INT_PER / 4; ++k) {
        const int i = i0 + 4 * k;
        if (i + 3 < c.len) {
          *reinterpret_cast<float4*>(r + i) = make_float4(x[h][4 * k], x[h][4 * k + 1],
                                                          x[h][4 * k + 2], x[h][4 * k + 3]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (i + j < c.len) r[i + j] = x[h][4 * k + j];
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  nsat = ew_wave_sum_u(nsat);
  if (lane == 0) ws[wv] = nsat;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = ws[0];
#pragma unroll
    for (int i = 1; i < EW_WAVES; ++i) t += ws[i];
    sat[blockIdx.x] = t;
  }
}

// the row's partial in k_clip_norm's order; valid in thread 0
__device__ __forceinline__ void int_store_partial(float s, float* ws, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  s = ew_wave_sum(s);
  if (lane == 0) ws[wv] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = ws[0];
#pragma unroll
    for (int i = 1; i < EW_WAVES; ++i) t += ws[i];
    *out = t;
  }
}

__global__ __launch_bounds__(EW_BLOCK) void k_int_decode_apply(
    const uint8_t* __restrict__ codes, const ChunkRow* __restrict__ chunks,
    const IntState* __restrict__ st, float* __restrict__ partials, float* __restrict__ param,
    float* __restrict__ mom, uint16_t* __restrict__ shadow, SgdArgs sa) {
  __shared__ float ws[EW_WAVES];
  const ChunkRow c = chunks[blockIdx.x];
  ew_sgd_resolve(sa);
  ew_key_advance(sa);
  const float inv_na = st->inv_na;
  float* p = param + c.start;
  float* b = mom ? mom + c.start : nullptr;
  uint16_t* sh = shadow ? shadow + c.start : nullptr;
  const uint8_t* cd = codes + c.start;
  uint32_t w[EW_CU];
  float pv[EW_CU][4], bv[EW_CU][4];
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    w[u] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) pv[u][j] = bv[u][j] = 0.0f;
    if (i + 3 < c.len) {
      w[u] = *reinterpret_cast<const uint32_t*>(cd + i);
      const float4 p4 = *reinterpret_cast<const float4*>(p + i);
      pv[u][0] = p4.x; pv[u][1] = p4.y; pv[u][2] = p4.z; pv[u][3] = p4.w;
      if (b) {
        const float4 b4 = *reinterpret_cast<const float4*>(b + i);
        bv[u][0] = b4.x; bv[u][1] = b4.y; bv[u][2] = b4.z; bv[u][3] = b4.w;
      }
    } else if (i < c.len) {  // 4 | i and 64 | the row's span: the whole word exists
      w[u] = *reinterpret_cast<const uint32_t*>(cd + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i + j < c.len) {
          pv[u][j] = p[i + j];
          if (b) bv[u][j] = b[i + j];
        }
      }
    }
  }
  float s = 0.0f;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float old = pv[u][j];
      if (i + j < c.len) {
        const float gv = (float)(int)(int8_t)(w[u] >> (8 * j)) * inv_na;
        ew_sgd(pv[u][j], bv[u][j], gv, sa);
      }
      const float d = pv[u][j] - old;  // past the tensor's end: 0 - 0
      s += d * d;
    }
    if (i + 3 < c.len) {
      *reinterpret_cast<float4*>(p + i) = make_float4(pv[u][0], pv[u][1], pv[u][2], pv[u][3]);
      if (b) *reinterpret_cast<float4*>(b + i) = make_float4(bv[u][0], bv[u][1], bv[u][2], bv[u][3]);
      if (sh) ew_st4_bf16(sh + i, 4, pv[u]);
    } else if (i < c.len) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i + j < c.len) {
          p[i + j] = pv[u][j];
          if (b) b[i + j] = bv[u][j];
          if (sh) sh[i + j] = ew_f2bf(pv[u][j]);
        }
      }
    }
  }
  int_store_partial(s, ws, partials + blockIdx.x);
}

__global__ __launch_bounds__(EW_BLOCK) void k_int_update_norm(const float* __restrict__ param,
                                                              const float* __restrict__ prev,
                                                              const ChunkRow* __restrict__ chunks,
                                                              float* __restrict__ partials) {
  __shared__ float ws[EW_WAVES];
  const ChunkRow c = chunks[blockIdx.x];
  const float* p = param + c.start;
  const float* o = prev + c.start;
  float pv[EW_CU][4], ov[EW_CU][4];
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
#pragma unroll
    for (int j = 0; j < 4; ++j) pv[u][j] = ov[u][j] = 0.0f;
    if (i + 3 < c.len) {
      const float4 p4 = *reinterpret_cast<const float4*>(p + i);
      const float4 o4 = *reinterpret_cast<const float4*>(o + i);
      pv[u][0] = p4.x; pv[u][1] = p4.y; pv[u][2] = p4.z; pv[u][3] = p4.w;
      ov[u][0] = o4.x; ov[u][1] = o4.y; ov[u][2] = o4.z; ov[u][3] = o4.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i + j < c.len) {
          pv[u][j] = p[i + j];
          ov[u][j] = o[i + j];
        }
      }
    }
  }
  float s = 0.0f;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = pv[u][j] - ov[u][j];
      s += d * d;
    }
  int_store_partial(s, ws, partials + blockIdx.x);
}

#define INT_TILE (4 * EW_BLOCK)
#define INT_BETA 0.9
#define INT_EPS2 1e-16

__global__ __launch_bounds__(EW_BLOCK) void k_int_alpha(const float* __restrict__ partials,
                                                        int total, IntState* __restrict__ st,
                                                        const float* __restrict__ lr_ptr,
                                                        float lr_arg, int world, double numel) {
  __shared__ float tile[INT_TILE];
  double s = 0.0;
  for (int base = 0; base < total; base += INT_TILE) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = k * EW_BLOCK + (int)threadIdx.x;
      tile[j] = base + j < total ? partials[base + j] : 0.0f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = total - base < INT_TILE ? total - base : INT_TILE;
      for (int j = 0; j < n; ++j) s += (double)tile[j];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int steps = st->steps;
    const double r = steps ? INT_BETA * st->r + (1.0 - INT_BETA) * s : s;
    const double lr = (double)(lr_ptr ? *lr_ptr : lr_arg);
    const float alpha = (float)(lr * sqrt(numel) / sqrt(2.0 * (double)world * r + INT_EPS2));
    float inv_a = 0.0f, inv_na = 0.0f;
    if (alpha != 0.0f) {
      inv_a = (float)(1.0 / (double)alpha);
      inv_na = (float)(1.0 / ((double)alpha * (double)world));
    }
    st->r = r;
    st->s_last = s;
    st->alpha = alpha;
    st->inv_a = inv_a;
    st->inv_na = inv_na;
    st->steps = steps + 1;
  }
}

// codes i8[length] must lie inside `bytes`; 64 | length (the layout's packing rule)
void int_fit(const std::string& who, int num_chunks, long long length, long long bytes) {
  if (num_chunks <= 0) throw std::runtime_error(who + ": empty bucket");
  if (length <= 0 || length % 64 || length > 0x7fffffffLL)
    throw std::runtime_error(who + ": the bucket length must be a positive multiple of 64");
  if (bytes < length) throw std::runtime_error(who + ": the codes do not fit the payload");
}

}  // namespace

#define EW_LAUNCH(kern, grid, stream, ...) \
  hipLaunchKernelGGL(kern, dim3(grid), dim3(EW_BLOCK), 0, (hipStream_t)(stream), __VA_ARGS__)

void ew_int_encode(const IntEncodeArgs& a) {
  int_fit("ewdml intsgd", a.num_chunks, a.length, a.payload_bytes);
  if (!a.chunks || !a.payload || !a.state || !a.sat)
    throw std::runtime_error("ewdml intsgd: missing operand");
  if ((a.payload | a.resid) % 16 || a.state % 8 || (a.chunks | a.sat | a.key_ptr) % 4)
    throw std::runtime_error("ewdml intsgd: misaligned operand");
  if (a.q < 1 || a.q > 127) throw std::runtime_error("ewdml intsgd: q must be in [1, 127]");
  GradPtrs g;
  ew_fill_ptrs(g, a.src, a.num_tensors);
  auto* chunks = reinterpret_cast<const ChunkRow*>(a.chunks);
  auto* pay = reinterpret_cast<uint8_t*>(a.payload);
  auto* st = reinterpret_cast<const IntState*>(a.state);
  auto* sat = reinterpret_cast<uint32_t*>(a.sat);
  auto* keyp = reinterpret_cast<const uint32_t*>(a.key_ptr);
  float* resid = reinterpret_cast<float*>(a.resid);
  if (resid)
    EW_LAUNCH(k_int_encode<true>, a.num_chunks, a.stream, g, resid, chunks, pay, st, sat,
              (int)a.length, a.q, a.key, keyp, a.bucket_offset);
  else
    EW_LAUNCH(k_int_encode<false>, a.num_chunks, a.stream, g, resid, chunks, pay, st, sat,
              (int)a.length, a.q, a.key, keyp, a.bucket_offset);
  EW_CHECK_LAUNCH();
}

void ew_int_decode_apply(const IntDecodeArgs& a) {
  int_fit("ewdml intsgd decode", a.num_chunks, a.length, a.length);
  if (!a.recv || !a.chunks || !a.state || !a.partials)
    throw std::runtime_error("ewdml intsgd decode: missing operand");
  const StepArgs& s = a.step;
  ew_step_check("ewdml intsgd decode", s, false);
  if (!s.apply || s.grad_out || s.grad_scale != 1.0f)
    throw std::runtime_error("ewdml intsgd decode: the fused step only (grad_scale 1, no grad_out)");
  if (a.recv % 16 || a.state % 8 || (a.chunks | a.partials) % 4)
    throw std::runtime_error("ewdml intsgd decode: misaligned operand");
  EW_LAUNCH(k_int_decode_apply, a.num_chunks, a.stream, reinterpret_cast<const uint8_t*>(a.recv),
            reinterpret_cast<const ChunkRow*>(a.chunks),
            reinterpret_cast<const IntState*>(a.state), reinterpret_cast<float*>(a.partials),
            reinterpret_cast<float*>(s.param), reinterpret_cast<float*>(s.mom),
            reinterpret_cast<uint16_t*>(s.shadow), ew_sgd_args(s));
  EW_CHECK_LAUNCH();
}

void ew_int_update_norm(const IntNormArgs& a) {
  int_fit("ewdml intsgd norm", a.num_chunks, a.length, a.length);
  if (!a.param || !a.prev || !a.chunks || !a.partials)
    throw std::runtime_error("ewdml intsgd norm: missing operand");
  if ((a.param | a.prev) % 16 || (a.chunks | a.partials) % 4)
    throw std::runtime_error("ewdml intsgd norm: misaligned operand");
  EW_LAUNCH(k_int_update_norm, a.num_chunks, a.stream, reinterpret_cast<const float*>(a.param),
            reinterpret_cast<const float*>(a.prev), reinterpret_cast<const ChunkRow*>(a.chunks),
            reinterpret_cast<float*>(a.partials));
  EW_CHECK_LAUNCH();
}

void ew_int_alpha(const IntAlphaArgs& a) {
  if (!a.partials || !a.state || a.total_chunks < 1)
    throw std::runtime_error("ewdml intsgd alpha: missing operand");
  if (a.state % 8 || (a.partials | a.lr_ptr) % 4)
    throw std::runtime_error("ewdml intsgd alpha: misaligned operand");
  if (a.world < 1 || a.world > 127 || !(a.numel >= 1.0))
    throw std::runtime_error("ewdml intsgd alpha: world must be in [1, 127] and numel >= 1");
  EW_LAUNCH(k_int_alpha, 1, a.stream, reinterpret_cast<const float*>(a.partials), a.total_chunks,
            reinterpret_cast<IntState*>(a.state), reinterpret_cast<const float*>(a.lr_ptr), a.lr,
            a.world, a.numel);
  EW_CHECK_LAUNCH();
}
