// Block floating point of a flat gradient bucket: OCP Microscaling (MX) v1.0, 32 consecutive
// elements under one power-of-two E8M0 scale, FP8 E4M3 (BITS = 8) or FP4 E2M1 (BITS = 4) elements,
// with error feedback, and the fused decode -> rank-ordered sum -> SGD on the receive side.
// gfx950, wave64.
//
// Payload (compress/plan.py, kind "mx"): scales u8[L / 32] | codes u8[L] or nibbles u8[L / 2], L the
// bucket's padded length.  Element i of the bucket is code byte i (nibble i & 1 of byte i >> 1) and
// its scale is byte i >> 5.  Tensors start on multiples of 64, so a block never spans two of them.
//
// A chunk row owns the positions from its start to the next row's start (the bucket's end for the
// last row): its own len elements and, for a tensor's last row, the zeros of the pad behind them.
// In ew_ld_chunk's register layout (thread t holds elements u * 1024 + 4 t + j) an MX block is the
// 8 lanes t >> 3 of one slab, so the scale is an integer maximum over three lane exchanges: no LDS,
// no scratch, no second launch, no RNG.  The rule (compress/oracle.py mx_scale_bytes / mx_quantize
// / mx_dequantize, bit for bit): em = exponent field of max(bits(e) & 0x7fffffff), s = max(em -
// emax, 0), or 0xFF with codes 0 when em == 255; q = e / 2^(s - 127) rounded to nearest even and
// saturated; d = value(code) * 2^(s - 127); residual = e - d.
//
// The conversions are CDNA4's v_cvt_scalef32_pk_{fp8,fp4}_f32 and v_cvt_scalef32_pk_f32_{fp8,fp4}
// (the scale operand is a float whose exponent field is the E8M0 byte).  SOFT instances do the same
// in integer and fp32 arithmetic; they are the cross-check of the boundary test
// (tests/kernels/test_mx_codec_hip.py, profiles/validation/mx.md) and are never launched by the
// trainer.
#include "common.h"
#include "ewdml_ops.h"

namespace {

typedef short mx_v2s __attribute__((ext_vector_type(2)));
typedef float mx_v2f __attribute__((ext_vector_type(2)));

template <int BITS> struct MxFmt;
template <> struct MxFmt<8> { static constexpr int MB = 3, BIAS = 7, EMAX = 8; };
template <> struct MxFmt<4> { static constexpr int MB = 1, BIAS = 1, EMAX = 2; };
template <int BITS> __device__ __forceinline__ float mx_top() { return BITS == 8 ? 448.0f : 6.0f; }

// the value lane ^ D of the same 8-lane group holds: quad permutes (DPP) inside a quad
template <int D>
__device__ __forceinline__ uint32_t mx_lane_xor(uint32_t x) {
  if (D == 1)  // quad_perm [1, 0, 3, 2]
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xf, 0xf, false);
  if (D == 2)  // quad_perm [2, 3, 0, 1]
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xf, 0xf, false);
  return (uint32_t)__shfl_xor((int)x, D, 64);
}

// the scale byte of the block this thread's four elements belong to (all 8 lanes get it)
template <int BITS>
__device__ __forceinline__ uint32_t mx_scale_byte(const float4& e) {
  uint32_t m = max(max(ew_key(e.x), ew_key(e.y)), max(ew_key(e.z), ew_key(e.w)));
  m = max(m, mx_lane_xor<1>(m));
  m = max(m, mx_lane_xor<2>(m));
  m = max(m, mx_lane_xor<4>(m));
  const uint32_t em = m >> 23;
  return em == 255u ? 255u : (em > (uint32_t)MxFmt<BITS>::EMAX ? em - MxFmt<BITS>::EMAX : 0u);
}

// 2^(s - 127) as the conversions' scale operand (only its exponent field is read) ...
__device__ __forceinline__ float mx_scale_operand(uint32_t s) { return __uint_as_float(s << 23); }
// ... and as an fp32 factor (s <= 254): 2^-127 is the denormal 0x00400000
__device__ __forceinline__ float mx_scale_value(uint32_t s) {
  return __uint_as_float(s ? s << 23 : 0x00400000u);
}

// software round-to-nearest-even of |e| * inv (inv = 2^(127 - s)) onto the grid, saturated
template <int BITS>
__device__ __forceinline__ uint32_t mx_soft_code(float e, float inv) {
  constexpr int MB = MxFmt<BITS>::MB, BIAS = MxFmt<BITS>::BIAS;
  const float a = fminf(fabsf(e) * inv, mx_top<BITS>());
  uint32_t mag;
  if (a < __uint_as_float((uint32_t)(128 - BIAS) << 23)) {  // below the smallest normal 2^(1 - BIAS)
    mag = (uint32_t)rintf(a * __uint_as_float((uint32_t)(127 + MB + BIAS - 1) << 23));
  } else {
    uint32_t b = __float_as_uint(a);
    b += ((b >> (23 - MB)) & 1u) + ((1u << (22 - MB)) - 1u);
    mag = (b >> (23 - MB)) - ((uint32_t)(127 - BIAS) << MB);
  }
  return mag | ((__float_as_uint(e) >> 31) << (BITS - 1));
}

// software value(code) * x (x = mx_scale_value(s)): exact in fp32
template <int BITS>
__device__ __forceinline__ float mx_soft_value(uint32_t code, float x) {
  constexpr int MB = MxFmt<BITS>::MB, BIAS = MxFmt<BITS>::BIAS;
  const uint32_t mag = code & ((1u << (BITS - 1)) - 1u);
  const float v = (mag >> MB) == 0u
      ? (float)mag * __uint_as_float((uint32_t)(127 + 1 - BIAS - MB) << 23)
      : __uint_as_float((mag << (23 - MB)) + ((uint32_t)(127 - BIAS) << 23));
  return __uint_as_float(__float_as_uint(v * x) | ((code >> (BITS - 1)) << 31));
}

// The codes of four elements under scale byte s (< 255): a dword of four FP8 bytes, or 16 bits of
// four FP4 nibbles, element j in byte / nibble j
template <int BITS, bool SOFT>
__device__ __forceinline__ uint32_t mx_pack4(const float4& e, uint32_t s) {
  if (SOFT) {
    const float inv = __uint_as_float((254u - s) << 23);
    const uint32_t c0 = mx_soft_code<BITS>(e.x, inv), c1 = mx_soft_code<BITS>(e.y, inv);
    const uint32_t c2 = mx_soft_code<BITS>(e.z, inv), c3 = mx_soft_code<BITS>(e.w, inv);
    return c0 | (c1 << BITS) | (c2 << (2 * BITS)) | (c3 << (3 * BITS));
  }
  const float sc = mx_scale_operand(s);
  if (BITS == 8) {
    // the E4M3 conversion rounds before it looks at the range and answers the NaN code 0x7F for
    // |q| > 464 instead of saturating (the E2M1 one saturates: it has no NaN code), so the band
    // (448, 512) X the scale rule leaves is clamped to 448 X = 1.75 * 2^(s + 8 - 127) first
    const float top = __uint_as_float(((s + 8u) << 23) | 0x00600000u);
    const float x = __builtin_amdgcn_fmed3f(e.x, -top, top), y = __builtin_amdgcn_fmed3f(e.y, -top, top);
    const float z = __builtin_amdgcn_fmed3f(e.z, -top, top), v = __builtin_amdgcn_fmed3f(e.w, -top, top);
    mx_v2s o = {0, 0};
    o = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(o, x, y, sc, false);
    o = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(o, z, v, sc, true);
    return (uint32_t)(uint16_t)o.x | ((uint32_t)(uint16_t)o.y << 16);
  }
  uint32_t w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, e.x, e.y, sc, 0);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, e.z, e.w, sc, 1);
  return w & 0xffffu;
}

// The four values mx_pack4's word decodes to under scale byte s (< 255)
template <int BITS, bool SOFT>
__device__ __forceinline__ void mx_unpack4(uint32_t w, uint32_t s, float (&d)[4]) {
  if (SOFT) {
    const float x = mx_scale_value(s);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      d[j] = mx_soft_value<BITS>((w >> (BITS * j)) & ((1u << BITS) - 1u), x);
    return;
  }
  const float sc = mx_scale_operand(s);
  mx_v2f lo, hi;
  if (BITS == 8) {
    lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, sc, false);
    hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, sc, true);
  } else {
    lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 0);
    hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 1);
  }
  d[0] = lo.x; d[1] = lo.y; d[2] = hi.x; d[3] = hi.y;
}

#define MX_NAN 0x7FC00000u

// One block per chunk row, one launch per bucket.  `length` = the bucket's padded length L.
template <int BITS, bool EF, bool SOFT>
__global__ __launch_bounds__(EW_BLOCK) void k_mx_encode(GradPtrs gp, float* __restrict__ resid,
                                                        const ChunkRow* __restrict__ chunks,
                                                        uint8_t* __restrict__ payload,
                                                        int scales_off, int codes_off, int length) {
  const ChunkRow c = chunks[blockIdx.x];
  // the positions this row writes: 64 | span <= EW_CHUNK (the layout's packing rule)
  const int span = (blockIdx.x + 1 < gridDim.x ? chunks[blockIdx.x + 1].start : length) - c.start;
  float4 e[EW_CU];
  ew_ld_chunk(gp, nullptr, c, e);  // positions past c.len read as 0: scale 0, code 0
  if (EF) {
    float4 r[EW_CU];
    ew_ld_chunk(gp, resid, c, r);
#pragma unroll
    for (int u = 0; u < EW_CU; ++u)
      e[u] = make_float4(e[u].x + r[u].x, e[u].y + r[u].y, e[u].z + r[u].z, e[u].w + r[u].w);
  }
  if (blockIdx.x == 0) {  // the scales section's alignment pad: payloads compare bytewise
    const int pad0 = scales_off + (length >> 5);  // even, as is codes_off
    if (pad0 + 2 * (int)threadIdx.x < codes_off)
      *reinterpret_cast<uint16_t*>(payload + pad0 + 2 * threadIdx.x) = 0;
  }
  uint8_t* codes = payload + codes_off + (BITS == 8 ? c.start : c.start >> 1);
  uint32_t sw[2] = {0u, 0u};  // this group's scale bytes of slabs 0..3 and 4..7
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    const uint32_t s = mx_scale_byte<BITS>(e[u]);
    sw[u >> 2] |= s << (8 * (u & 3));
    const bool dead = s == 255u;  // the block holds an inf or a NaN: codes 0, decodes to NaN
    const uint32_t sl = dead ? 0u : s;
    const uint32_t w = dead ? 0u : mx_pack4<BITS, SOFT>(e[u], sl);
    if (i < span) {
      if (BITS == 8) *reinterpret_cast<uint32_t*>(codes + i) = w;
      else *reinterpret_cast<uint16_t*>(codes + (i >> 1)) = (uint16_t)w;
    }
    if (EF) {
      float d[4];
      mx_unpack4<BITS, SOFT>(w, sl, d);
      if (dead) d[0] = d[1] = d[2] = d[3] = __uint_as_float(MX_NAN);
      e[u] = make_float4(e[u].x - d[0], e[u].y - d[1], e[u].z - d[2], e[u].w - d[3]);
    }
  }
  // scale byte u * 32 + g of the row belongs to group g = t >> 3 of slab u.  Even groups fetch
  // their right neighbour's bytes and lane k of the group stores slab k's pair: one 16-bit store
  const uint32_t n0 = (uint32_t)__shfl_xor((int)sw[0], 8, 64);
  const uint32_t n1 = (uint32_t)__shfl_xor((int)sw[1], 8, 64);
  const int k = threadIdx.x & 7, g = threadIdx.x >> 3;
  if (!(g & 1) && k * (4 * EW_BLOCK) + 32 * g < span) {
    const int sh = 8 * (k & 3);
    const uint32_t mine = ((k < 4 ? sw[0] : sw[1]) >> sh) & 0xffu;
    const uint32_t right = ((k < 4 ? n0 : n1) >> sh) & 0xffu;
    *reinterpret_cast<uint16_t*>(payload + scales_off + (c.start >> 5) + k * (EW_BLOCK / 8) + g) =
        (uint16_t)(mine | (right << 8));
  }
  if (EF) ew_st_chunk(resid + c.start, c.len, e);
}

// One block per chunk row: the N received rows decoded and summed in rank order from 0.0f
// (oracle.decode_sum), then ew_chunk_apply
template <int BITS, bool SOFT>
__global__ __launch_bounds__(EW_BLOCK) void k_mx_decode_apply(
    const uint8_t* __restrict__ recv, int nranks, long long stride,
    const ChunkRow* __restrict__ chunks, int scales_off, int codes_off, float* __restrict__ param,
    float* __restrict__ mom, float* __restrict__ grad_out, uint16_t* __restrict__ shadow,
    SgdArgs sa, int apply) {
  const ChunkRow c = chunks[blockIdx.x];
  ew_sgd_resolve(sa);
  ew_key_advance(sa);
  const size_t scale_at = (size_t)scales_off + (c.start >> 5) + (threadIdx.x >> 3);
  const size_t codes_at = (size_t)codes_off + (BITS == 8 ? c.start : c.start >> 1);
  float acc[EW_CU][4];
#pragma unroll
  for (int u = 0; u < EW_CU; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[u][j] = 0.0f;
  for (int r = 0; r < nranks; ++r) {
    const uint8_t* pay = recv + r * stride;
    uint32_t w[EW_CU], s[EW_CU];
    // a slab with an element of the chunk lies inside the row's span: its codes and scale exist
#pragma unroll
    for (int u = 0; u < EW_CU; ++u) {
      const int i = ew_chunk_idx(u);
      w[u] = 0u;
      s[u] = 0u;
      if (i < c.len) {
        s[u] = pay[scale_at + u * (EW_BLOCK / 8)];
        if (BITS == 8) w[u] = *reinterpret_cast<const uint32_t*>(pay + codes_at + i);
        else w[u] = *reinterpret_cast<const uint16_t*>(pay + codes_at + (i >> 1));
      }
    }
#pragma unroll
    for (int u = 0; u < EW_CU; ++u) {
      const bool dead = s[u] == 255u;
      float d[4];
      mx_unpack4<BITS, SOFT>(w[u], dead ? 0u : s[u], d);
      if (dead) d[0] = d[1] = d[2] = d[3] = __uint_as_float(MX_NAN);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[u][j] = acc[u][j] + d[j];
    }
  }
  ew_chunk_apply(acc, c, param, mom, grad_out, shadow, sa, apply);
}

}  // namespace

#define EW_LAUNCH(kern, grid, stream, ...) \
  hipLaunchKernelGGL(kern, dim3(grid), dim3(EW_BLOCK), 0, (hipStream_t)(stream), __VA_ARGS__)

// The two sections must lie inside `bytes`: scales u8[L / 32] | codes u8[L * bits / 8]
static void ew_mx_fit(const std::string& who, int bits, int scales_off, int codes_off,
                      long long length, long long bytes) {
  if (bits != 8 && bits != 4) throw std::runtime_error(who + ": elements are 8 or 4 bits wide");
  if (length <= 0 || length % 64 || length > 0x7fffffffLL)
    throw std::runtime_error(who + ": the bucket length must be a positive multiple of 64");
  if (scales_off < 0 || scales_off % 16 || codes_off % 16 ||
      codes_off < scales_off + length / 32 || bytes < codes_off + length * bits / 8 ||
      bytes > 0x7fffffffLL)
    throw std::runtime_error(who + ": payload sections do not fit the payload");
}

template <int BITS, bool SOFT>
static void ew_mx_encode_launch(const MxEncodeArgs& a, const GradPtrs& g) {
  auto* chunks = reinterpret_cast<const ChunkRow*>(a.chunks);
  auto* pay = reinterpret_cast<uint8_t*>(a.payload);
  float* resid = reinterpret_cast<float*>(a.resid);
  if (resid)
    EW_LAUNCH((k_mx_encode<BITS, true, SOFT>), a.num_chunks, a.stream, g, resid, chunks, pay,
              a.scales_off, a.codes_off, (int)a.length);
  else
    EW_LAUNCH((k_mx_encode<BITS, false, SOFT>), a.num_chunks, a.stream, g, resid, chunks, pay,
              a.scales_off, a.codes_off, (int)a.length);
}

void ew_mx_encode(const MxEncodeArgs& a) {
  if (a.num_chunks <= 0) throw std::runtime_error("ewdml mx: empty bucket");
  ew_mx_fit("ewdml mx", a.bits, a.scales_off, a.codes_off, a.length, a.payload_bytes);
  if (!a.chunks || !a.payload) throw std::runtime_error("ewdml mx: missing table");
  if ((a.payload | a.resid) % 16 || a.chunks % 4)
    throw std::runtime_error("ewdml mx: misaligned operand");
  GradPtrs g;
  ew_fill_ptrs(g, a.src, a.num_tensors);
  if (a.bits == 8) {
    if (a.soft) ew_mx_encode_launch<8, true>(a, g);
    else ew_mx_encode_launch<8, false>(a, g);
  } else {
    if (a.soft) ew_mx_encode_launch<4, true>(a, g);
    else ew_mx_encode_launch<4, false>(a, g);
  }
  EW_CHECK_LAUNCH();
}

template <int BITS, bool SOFT>
static void ew_mx_decode_launch(const MxDecodeArgs& a, const SgdArgs& sa) {
  EW_LAUNCH((k_mx_decode_apply<BITS, SOFT>), a.num_chunks, a.stream,
            reinterpret_cast<const uint8_t*>(a.recv), a.nranks, a.stride,
            reinterpret_cast<const ChunkRow*>(a.chunks), a.scales_off, a.codes_off,
            reinterpret_cast<float*>(a.step.param), reinterpret_cast<float*>(a.step.mom),
            reinterpret_cast<float*>(a.step.grad_out),
            reinterpret_cast<uint16_t*>(a.step.shadow), sa, a.step.apply);
}

void ew_mx_decode_apply(const MxDecodeArgs& a) {
  if (a.num_chunks <= 0 || a.nranks <= 0 || a.nranks > EW_MAX_RANKS)
    throw std::runtime_error("ewdml mx decode: nothing to decode, or too many ranks");
  ew_mx_fit("ewdml mx decode", a.bits, a.scales_off, a.codes_off, a.length, a.stride);
  if (!a.recv || !a.chunks) throw std::runtime_error("ewdml mx decode: missing table");
  ew_step_check("ewdml mx decode", a.step, false);
  if (a.recv % 16 || a.stride % 4 || a.chunks % 4)
    throw std::runtime_error("ewdml mx decode: misaligned operand");
  const SgdArgs sa = ew_sgd_args(a.step);
  if (a.bits == 8) {
    if (a.soft) ew_mx_decode_launch<8, true>(a, sa);
    else ew_mx_decode_launch<8, false>(a, sa);
  } else {
    if (a.soft) ew_mx_decode_launch<4, true>(a, sa);
    else ew_mx_decode_launch<4, false>(a, sa);
  }
  EW_CHECK_LAUNCH();
}
