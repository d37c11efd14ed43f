// Scaled sign with error feedback (1-bit SGD, EF-signSGD: Seide et al. 2014, Karimireddy et al.
// 2019) of a flat gradient bucket, and the fused decode -> average -> SGD on the receive side.
// gfx950, wave64.
//
// Every chunk is independent: one block loads it once, forms e = g + residual, sums |e| in a fixed
// order, writes scale = sum / len, one bit per element (e < 0) and the new residual e -/+ scale.
// No scratch, no memset, no cross-block hand-off, no RNG: one launch per bucket.
//
// Payload (compress/plan.py, kind "sign"): scales f32[C] | bits u32[256 * C].  Chunk c owns words
// [256 c, 256 c + 256); element i of the chunk is bit i & 31 of word i >> 5.  Words and bits past
// the chunk's length are written as 0 on every encode.
//
// The summation order is part of the contract (compress/oracle.py _sign_chunk_sums reproduces it,
// so scales, bits and residuals match the oracle bit for bit): thread t adds, from 0.0f, elements
// u * 1024 + 4 t + j for u = 0..7 outer, j = 0..3 inner; then ew_block_sum.
//
// 1-bit Adam's compressed stage (Tang et al. 2021; optim/flat.py FlatOnebitAdam) reuses both sides:
// k_sign_encode<true, true> forms the momentum candidate in front of the same encode, and
// k_sign_decode_onebit writes the averaged momentum and takes the frozen-variance step
// (compress/oracle.py encode_sign_momentum / onebit_adam_apply, bit for bit).  1-bit LAMB (Li et
// al. 2021; FlatOnebitLamb) takes the same encode with weight decay 0 and a two-launch receive
// side, k_sign_decode_lamb_stage / k_lamb_onebit_apply (onebit_lamb_apply, bit for bit).
//
// The two-stage sign all-reduce (parallel/twostage.py) adds a slot-addressed form of all three:
// `slots` (nullable int2 per chunk) holds the byte offsets of the chunk's scale and of its 256
// words inside an [N, P] row buffer (row r = shard r's scales | bits), so one launch covers every
// shard of a bucket.  Pads of that buffer are zero at allocation and never written.  Its owner
// step, k_sign_reduce_encode, decodes the N received rows of a shard straight into the encode's
// register layout (compress/oracle.py sign_reduce_encode, bit for bit).
#include "common.h"
#include "ewdml_ops.h"

namespace {

// 1-bit Adam's compressed stage (MOM): what is compressed is the momentum candidate
// u = m * beta1 + (1 - beta1) * (g + wd * p), formed here from the shared exp_avg m (read only)
struct SignMom {
  const float* m;  // the bucket's exp_avg
  const float* p;  // the bucket's fp32 parameters (read when wd != 0)
  float beta1, wd;
};

// Byte offsets of a chunk's scale and of its first word: the bucket's own layout, or the slot table
__device__ __forceinline__ void ew_sign_where(const int2* __restrict__ slots, int scales_off,
                                              int bits_off, size_t& scale_at, size_t& words_at) {
  if (slots) {
    const int2 sl = slots[blockIdx.x];
    scale_at = (size_t)sl.x;
    words_at = (size_t)sl.y;
  } else {
    scale_at = (size_t)scales_off + 4 * (size_t)blockIdx.x;
    words_at = (size_t)bits_off + 4 * (size_t)blockIdx.x * EW_BM_WORDS;
  }
}

// The encode of the chunk held in e (0 past len): the fixed-order sum of |e|, the scale, the
// packed words, and e left as the residual e -/+ scale.  wsf / s_scale: the block's LDS.
__device__ __forceinline__ void ew_sign_pack(float4 (&e)[EW_CU], int len, float* scale_out,
                                             uint32_t* words, float* wsf, float* s_scale) {
  float s = 0.0f;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    s = s + fabsf(e[u].x);
    s = s + fabsf(e[u].y);
    s = s + fabsf(e[u].z);
    s = s + fabsf(e[u].w);
  }
  const float total = ew_block_sum(s, wsf);
  if (threadIdx.x == 0) {
    const float sc = total / (float)len;
    *s_scale = sc;
    *scale_out = sc;
  }
  __syncthreads();
  const float scale = *s_scale;

  // thread t holds elements 4t .. 4t + 3 of each slab: a nibble of word u * 32 + (t >> 3).  The 8
  // lanes of a word OR their nibbles together (all 8 end up with the word); lane k of the group
  // then stores slab k's word, so the block's 256 words go out as one dword store per thread.
  const int k = threadIdx.x & 7;
  uint32_t mine = 0;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    uint32_t w = (uint32_t)(e[u].x < 0.0f) | ((uint32_t)(e[u].y < 0.0f) << 1) |
                 ((uint32_t)(e[u].z < 0.0f) << 2) | ((uint32_t)(e[u].w < 0.0f) << 3);
    w <<= 4 * k;
    w |= __shfl_xor(w, 1, 64);
    w |= __shfl_xor(w, 2, 64);
    w |= __shfl_xor(w, 4, 64);
    mine = (u == k) ? w : mine;
  }
  words[k * (EW_BLOCK / 8) + (threadIdx.x >> 3)] = mine;

#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    e[u].x = e[u].x - (e[u].x < 0.0f ? -scale : scale);
    e[u].y = e[u].y - (e[u].y < 0.0f ? -scale : scale);
    e[u].z = e[u].z - (e[u].z < 0.0f ? -scale : scale);
    e[u].w = e[u].w - (e[u].w < 0.0f ? -scale : scale);
  }
}

template <bool EF, bool MOM>
__global__ __launch_bounds__(EW_BLOCK) void k_sign_encode(GradPtrs gp, float* __restrict__ resid,
                                                          const ChunkRow* __restrict__ chunks,
                                                          uint8_t* __restrict__ payload,
                                                          int scales_off, int bits_off,
                                                          SignMom mo,
                                                          const int2* __restrict__ slots) {
  __shared__ float wsf[EW_WAVES];
  __shared__ float s_scale;
  const ChunkRow c = chunks[blockIdx.x];
  float4 e[EW_CU];
  ew_ld_chunk(gp, nullptr, c, e);  // positions past c.len read as 0: |e| = 0, bit = 0
  if (MOM) {  // m and p read as 0 past c.len too: u = 0 there
    float4 m[EW_CU];
    ew_ld_chunk(gp, mo.m, c, m);
    if (mo.wd != 0.0f) {
      float4 p[EW_CU];
      ew_ld_chunk(gp, mo.p, c, p);
#pragma unroll
      for (int u = 0; u < EW_CU; ++u)
        e[u] = make_float4(e[u].x + mo.wd * p[u].x, e[u].y + mo.wd * p[u].y,
                           e[u].z + mo.wd * p[u].z, e[u].w + mo.wd * p[u].w);
    }
    const float b1 = mo.beta1, c1 = 1.0f - mo.beta1;
#pragma unroll
    for (int u = 0; u < EW_CU; ++u)
      e[u] = make_float4(m[u].x * b1 + c1 * e[u].x, m[u].y * b1 + c1 * e[u].y,
                         m[u].z * b1 + c1 * e[u].z, m[u].w * b1 + c1 * e[u].w);
  }
  if (EF) {
    float4 r[EW_CU];
    ew_ld_chunk(gp, resid, c, r);
#pragma unroll
    for (int u = 0; u < EW_CU; ++u)
      e[u] = make_float4(e[u].x + r[u].x, e[u].y + r[u].y, e[u].z + r[u].z, e[u].w + r[u].w);
  }
  if (!slots && blockIdx.x == 0) {  // the scales section's alignment pad: payloads compare bytewise
    const int nslots = (bits_off - scales_off) >> 2;
    for (int i = (int)gridDim.x + (int)threadIdx.x; i < nslots; i += EW_BLOCK)
      reinterpret_cast<float*>(payload + scales_off)[i] = 0.0f;
  }
  size_t scale_at, words_at;
  ew_sign_where(slots, scales_off, bits_off, scale_at, words_at);
  ew_sign_pack(e, c.len, reinterpret_cast<float*>(payload + scale_at),
               reinterpret_cast<uint32_t*>(payload + words_at), wsf, &s_scale);
  if (EF) ew_st_chunk(resid + c.start, c.len, e);
}

// ---- the rotated form (--sign-rotate hadamard; DRIVE / EDEN, Vargaftik et al. 2021 / 2022) -----
// The chunk row, always all EW_CHUNK positions of it, is rotated by y = H(D e) before the signs
// are taken and the decoded row is rotated back by D(H(.)) * 2^-13 (compress/oracle.py fwht /
// hsign_flip, bit for bit).  D flips sign bits chosen by rot_key, a host constant of the bucket
// that is the same on every rank and every step; H is the unnormalised Walsh-Hadamard transform
// of the 8192 values held across the block's registers, one butterfly stage per index bit.  With
// element i = u << 10 | wave << 8 | lane << 2 | j (ew_chunk_idx) the stages run in the order
// oracle.HSIGN_STAGE_BITS: bits 0, 1 (j) and 10..12 (u) inside a thread, bits 2..7 across the
// lanes of a wave, bits 8, 9 across the four waves through LDS.  Every butterfly is one fp32 add:
// the upper element's x[i] - x[i | bit] is formed as x[i] + (-x[i | bit]), which rounds the same.

// D: word w = u * 32 + (t >> 3) of chunk row c is mix32((c * 256 + w) ^ rot_key); thread t's four
// elements of slab u are bits 4 (t & 7) .. + 3 of it, the nibble ew_sign_pack writes
__device__ __forceinline__ float ew_flip(float x, uint32_t bit) {
  return __uint_as_float(__float_as_uint(x) ^ (bit << 31));
}
__device__ __forceinline__ void ew_hs_flip(float4 (&e)[EW_CU], uint32_t rot_key) {
  const uint32_t w0 = blockIdx.x * EW_BM_WORDS + (threadIdx.x >> 3);
  const int shift = 4 * (threadIdx.x & 7);
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const uint32_t nib = ew_mix32((w0 + u * (EW_BLOCK / 8)) ^ rot_key) >> shift;
    e[u] = make_float4(ew_flip(e[u].x, nib & 1u), ew_flip(e[u].y, (nib >> 1) & 1u),
                       ew_flip(e[u].z, (nib >> 2) & 1u), ew_flip(e[u].w, (nib >> 3) & 1u));
  }
}

// one butterfly between two values of the same thread
__device__ __forceinline__ void ew_bfly(float& a, float& b) {
  const float s = a + b, d = a - b;
  a = s;
  b = d;
}

// the value lane ^ D holds: quad permutes (DPP, no LDS crossbar) inside a quad, ds_bpermute beyond
template <int D>
__device__ __forceinline__ float ew_lane_xor(float x) {
  if (D == 1)  // quad_perm [1, 0, 3, 2]
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, false));
  if (D == 2)  // quad_perm [2, 3, 0, 1]
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, false));
  return __shfl_xor(x, D, 64);
}

// the stage of lane bit D: the lower lane keeps x + other, the upper lane other - x
template <int D>
__device__ __forceinline__ void ew_fwht_lanes(float4 (&e)[EW_CU]) {
  const uint32_t up = ((threadIdx.x & D) != 0) ? 1u : 0u;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    e[u].x = ew_flip(e[u].x, up) + ew_lane_xor<D>(e[u].x);
    e[u].y = ew_flip(e[u].y, up) + ew_lane_xor<D>(e[u].y);
    e[u].z = ew_flip(e[u].z, up) + ew_lane_xor<D>(e[u].z);
    e[u].w = ew_flip(e[u].w, up) + ew_lane_xor<D>(e[u].w);
  }
}

// H of the block's chunk, in place.  xch: EW_CU * EW_BLOCK float4 of LDS (32 KiB), free again on
// return.  Every thread of the block must call it.
__device__ __forceinline__ void ew_fwht(float4 (&e)[EW_CU], float4* xch) {
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {  // bits 0, 1
    ew_bfly(e[u].x, e[u].y);
    ew_bfly(e[u].z, e[u].w);
    ew_bfly(e[u].x, e[u].z);
    ew_bfly(e[u].y, e[u].w);
  }
#pragma unroll
  for (int m = 1; m < EW_CU; m <<= 1)  // bits 10, 11, 12
#pragma unroll
    for (int u = 0; u < EW_CU; ++u)
      if (!(u & m)) {
        ew_bfly(e[u].x, e[u | m].x);
        ew_bfly(e[u].y, e[u | m].y);
        ew_bfly(e[u].z, e[u | m].z);
        ew_bfly(e[u].w, e[u | m].w);
      }
  ew_fwht_lanes<1>(e);  // bits 2 .. 7
  ew_fwht_lanes<2>(e);
  ew_fwht_lanes<4>(e);
  ew_fwht_lanes<8>(e);
  ew_fwht_lanes<16>(e);
  ew_fwht_lanes<32>(e);
  // bits 8, 9: the same lane of the four waves.  After bit 8 wave w holds v0 +/- v1 (w < 2) or
  // v2 +/- v3, minus in the odd waves; bit 9 pairs waves w and w ^ 2, minus in waves 2 and 3
  const int lane = threadIdx.x & 63;
  const uint32_t odd = (threadIdx.x >> 6) & 1u, top = (threadIdx.x >> 7) & 1u;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) xch[u * EW_BLOCK + threadIdx.x] = e[u];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const float4 v0 = xch[u * EW_BLOCK + lane], v1 = xch[u * EW_BLOCK + 64 + lane];
    const float4 v2 = xch[u * EW_BLOCK + 128 + lane], v3 = xch[u * EW_BLOCK + 192 + lane];
    const float4 lo = make_float4(v0.x + ew_flip(v1.x, odd), v0.y + ew_flip(v1.y, odd),
                                  v0.z + ew_flip(v1.z, odd), v0.w + ew_flip(v1.w, odd));
    const float4 hi = make_float4(v2.x + ew_flip(v3.x, odd), v2.y + ew_flip(v3.y, odd),
                                  v2.z + ew_flip(v3.z, odd), v2.w + ew_flip(v3.w, odd));
    e[u] = make_float4(lo.x + ew_flip(hi.x, top), lo.y + ew_flip(hi.y, top),
                       lo.z + ew_flip(hi.z, top), lo.w + ew_flip(hi.w, top));
  }
  __syncthreads();
}

// the inverse rotation of a row held in e: D(H(e)) * 2^-13
__device__ __forceinline__ void ew_hs_unrotate(float4 (&e)[EW_CU], uint32_t rot_key, float4* xch) {
  ew_fwht(e, xch);
  ew_hs_flip(e, rot_key);
  const float inv = 1.0f / (float)EW_CHUNK;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u)
    e[u] = make_float4(e[u].x * inv, e[u].y * inv, e[u].z * inv, e[u].w * inv);
}

// The rotated encode: one block per chunk row, one launch per bucket.  The quantiser is
// ew_sign_pack over all EW_CHUNK positions of y (scale = sum|y| / 8192, every bit meaningful); with
// error feedback the residual goes back through the inverse rotation and only the chunk's own
// positions are stored, so the residual buffer keeps its meaning
template <bool EF>
__global__ __launch_bounds__(EW_BLOCK) void k_hsign_encode(GradPtrs gp, float* __restrict__ resid,
                                                           const ChunkRow* __restrict__ chunks,
                                                           uint8_t* __restrict__ payload,
                                                           int scales_off, int bits_off,
                                                           uint32_t rot_key) {
  __shared__ float4 xch[EW_CU * EW_BLOCK];
  __shared__ float wsf[EW_WAVES];
  __shared__ float s_scale;
  const ChunkRow c = chunks[blockIdx.x];
  float4 e[EW_CU];
  ew_ld_chunk(gp, nullptr, c, e);  // positions past c.len read as 0
  if (EF) {
    float4 r[EW_CU];
    ew_ld_chunk(gp, resid, c, r);
#pragma unroll
    for (int u = 0; u < EW_CU; ++u)
      e[u] = make_float4(e[u].x + r[u].x, e[u].y + r[u].y, e[u].z + r[u].z, e[u].w + r[u].w);
  }
  if (blockIdx.x == 0) {  // the scales section's alignment pad: payloads compare bytewise
    const int nslots = (bits_off - scales_off) >> 2;
    for (int i = (int)gridDim.x + (int)threadIdx.x; i < nslots; i += EW_BLOCK)
      reinterpret_cast<float*>(payload + scales_off)[i] = 0.0f;
  }
  ew_hs_flip(e, rot_key);
  ew_fwht(e, xch);
  size_t scale_at, words_at;
  ew_sign_where(nullptr, scales_off, bits_off, scale_at, words_at);
  ew_sign_pack(e, EW_CHUNK, reinterpret_cast<float*>(payload + scale_at),
               reinterpret_cast<uint32_t*>(payload + words_at), wsf, &s_scale);
  if (EF) {
    ew_hs_unrotate(e, rot_key, xch);
    ew_st_chunk(resid + c.start, c.len, e);
  }
}

// The rank-ordered sum, from 0.0f, of +/- scale_r over the rows of recv for this block's chunk:
// acc[u][j] is element ew_chunk_idx(u) + j, which is the encode's e[u] layout.
__device__ __forceinline__ void ew_sign_acc(const uint8_t* __restrict__ recv, int nranks,
                                            long long stride, size_t scale_at, size_t words_at,
                                            float (&acc)[EW_CU][4]) {
  const int shift = 4 * (threadIdx.x & 7);
#pragma unroll
  for (int u = 0; u < EW_CU; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[u][j] = 0.0f;
  for (int r = 0; r < nranks; ++r) {
    const uint8_t* pay = recv + r * stride;
    const float scale = *reinterpret_cast<const float*>(pay + scale_at);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(pay + words_at) + (threadIdx.x >> 3);
    uint32_t w[EW_CU];
#pragma unroll
    for (int u = 0; u < EW_CU; ++u) w[u] = words[u * (EW_BLOCK / 8)];
#pragma unroll
    for (int u = 0; u < EW_CU; ++u) {
      const uint32_t nib = w[u] >> shift;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[u][j] = acc[u][j] + (((nib >> j) & 1u) ? -scale : scale);
    }
  }
}

// The two-stage exchange's owner step for one shard: e = (sum over the N received rows) * inv_n +
// server residual, formed in registers, then the encode of e into the owner's row.  Reads the
// received rows and the server residual; writes the owner's row (scales and words only: its pads
// stay as allocated) and the server residual.  chunks / sresid are relative to the shard's start.
__global__ __launch_bounds__(EW_BLOCK) void k_sign_reduce_encode(
    const uint8_t* __restrict__ recv, int nranks, long long stride,
    const ChunkRow* __restrict__ chunks, int scales_off, int bits_off, float inv_n,
    float* __restrict__ sresid, uint8_t* __restrict__ out) {
  __shared__ float wsf[EW_WAVES];
  __shared__ float s_scale;
  const ChunkRow c = chunks[blockIdx.x];
  size_t scale_at, words_at;
  ew_sign_where(nullptr, scales_off, bits_off, scale_at, words_at);
  float acc[EW_CU][4];
  ew_sign_acc(recv, nranks, stride, scale_at, words_at, acc);
  float4 e[EW_CU];
  const float* sr = sresid + c.start;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i + 3 < c.len) {
      const float4 r4 = *reinterpret_cast<const float4*>(sr + i);
      r[0] = r4.x; r[1] = r4.y; r[2] = r4.z; r[3] = r4.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j < c.len) r[j] = sr[i + j];
    }
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)  // padding bits decode to +scale: positions past c.len are 0
      v[j] = (i + j < c.len) ? (acc[u][j] * inv_n + r[j]) : 0.0f;
    e[u] = make_float4(v[0], v[1], v[2], v[3]);
  }
  ew_sign_pack(e, c.len, reinterpret_cast<float*>(out + scale_at),
               reinterpret_cast<uint32_t*>(out + words_at), wsf, &s_scale);
  ew_st_chunk(sresid + c.start, c.len, e);
}

__global__ __launch_bounds__(EW_BLOCK) void k_sign_decode_apply(
    const uint8_t* __restrict__ recv, int nranks, long long stride,
    const ChunkRow* __restrict__ chunks, int scales_off, int bits_off, float* __restrict__ param,
    float* __restrict__ mom, float* __restrict__ grad_out, uint16_t* __restrict__ shadow,
    SgdArgs sa, int apply, const int2* __restrict__ slots) {
  const ChunkRow c = chunks[blockIdx.x];
  ew_sgd_resolve(sa);
  ew_key_advance(sa);
  size_t scale_at, words_at;
  ew_sign_where(slots, scales_off, bits_off, scale_at, words_at);
  float acc[EW_CU][4];
  ew_sign_acc(recv, nranks, stride, scale_at, words_at, acc);
  ew_chunk_apply(acc, c, param, mom, grad_out, shadow, sa, apply);
}

// The rotated decode: the N ranks' +/- scale are summed in the rotated domain over all EW_CHUNK
// positions (the rotation is shared, so it commutes with the sum), then one inverse transform
// whatever N is, then k_sign_decode_apply's tail
__global__ __launch_bounds__(EW_BLOCK) void k_hsign_decode_apply(
    const uint8_t* __restrict__ recv, int nranks, long long stride,
    const ChunkRow* __restrict__ chunks, int scales_off, int bits_off, float* __restrict__ param,
    float* __restrict__ mom, float* __restrict__ grad_out, uint16_t* __restrict__ shadow,
    SgdArgs sa, int apply, uint32_t rot_key) {
  __shared__ float4 xch[EW_CU * EW_BLOCK];
  const ChunkRow c = chunks[blockIdx.x];
  ew_sgd_resolve(sa);
  ew_key_advance(sa);
  size_t scale_at, words_at;
  ew_sign_where(nullptr, scales_off, bits_off, scale_at, words_at);
  float acc[EW_CU][4];
  ew_sign_acc(recv, nranks, stride, scale_at, words_at, acc);
  float4 e[EW_CU];
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) e[u] = make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
  ew_hs_unrotate(e, rot_key, xch);
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    acc[u][0] = e[u].x; acc[u][1] = e[u].y; acc[u][2] = e[u].z; acc[u][3] = e[u].w;
  }
  ew_chunk_apply(acc, c, param, mom, grad_out, shadow, sa, apply);
}

// 1-bit Adam's receive side: m = (sum over ranks of +/- scale, rank order, from 0) * inv_n for
// every element, then p -= lr_step * (m / (sqrtf(v) + eps)) where the frozen v > 0 (a coordinate
// whose variance is still 0 never saw a gradient: it keeps its parameter).  v is only read.
struct OnebitArgs {
  float lr_step, inv_n, eps, beta1, beta2;
  int freeze_step;
  // device step counter (nullable): t = *step + 1, and lr_step = lr * sqrt(1 - beta2^freeze_step)
  // / (1 - beta1^t) is formed here, so a captured graph follows the step count and the lr
  const int* step;
  double lr;
  const float* lr_ptr;
};

__device__ __forceinline__ void ew_onebit(float& p, float m, float v, const OnebitArgs& a) {
  if (v > 0.0f) p = p - a.lr_step * (m / (sqrtf(v) + a.eps));
}

__global__ __launch_bounds__(EW_BLOCK) void k_sign_decode_onebit(
    const uint8_t* __restrict__ recv, int nranks, long long stride,
    const ChunkRow* __restrict__ chunks, int scales_off, int bits_off, float* __restrict__ param,
    float* __restrict__ mom, const float* __restrict__ var, uint16_t* __restrict__ shadow,
    OnebitArgs oa, SgdArgs key, const int2* __restrict__ slots) {
  const ChunkRow c = chunks[blockIdx.x];
  if (oa.step) {
    const double t = (double)(*oa.step + 1);
    const double lr = oa.lr_ptr ? (double)*oa.lr_ptr : oa.lr;
    oa.lr_step = (float)(lr * sqrt(1.0 - pow((double)oa.beta2, (double)oa.freeze_step)) /
                         (1.0 - pow((double)oa.beta1, t)));
  }
  ew_key_advance(key);
  size_t scale_at, words_at;
  ew_sign_where(slots, scales_off, bits_off, scale_at, words_at);
  float acc[EW_CU][4];
  ew_sign_acc(recv, nranks, stride, scale_at, words_at, acc);
  float* p = param + c.start;
  float* b = mom + c.start;
  const float* vq = var + c.start;
  uint16_t* sh = shadow ? shadow + c.start : nullptr;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    if (i >= c.len) continue;
    float mv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) mv[j] = acc[u][j] * oa.inv_n;
    if (i + 3 < c.len) {
      const float4 p4 = *reinterpret_cast<const float4*>(p + i);
      const float4 v4 = *reinterpret_cast<const float4*>(vq + i);
      float pv[4] = {p4.x, p4.y, p4.z, p4.w};
      const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) ew_onebit(pv[j], mv[j], vv[j], oa);
      *reinterpret_cast<float4*>(b + i) = make_float4(mv[0], mv[1], mv[2], mv[3]);
      *reinterpret_cast<float4*>(p + i) = make_float4(pv[0], pv[1], pv[2], pv[3]);
      if (sh) ew_st4_bf16(sh + i, 4, pv);
    } else {  // the last elements of a tensor
      for (int j = 0; j < 4 && i + j < c.len; ++j) {
        float pv = p[i + j];
        ew_onebit(pv, mv[j], vq[i + j], oa);
        b[i + j] = mv[j];
        p[i + j] = pv;
        if (sh) sh[i + j] = ew_f2bf(pv);
      }
    }
  }
}

// 1-bit LAMB's receive side (Li et al. 2021; optim/flat.py FlatOnebitLamb; compress/oracle.py
// onebit_lamb_apply, bit for bit): two launches per bucket, one block per chunk row.
//
//   k_sign_decode_lamb_stage  m = mean of the decoded momenta, the gradient it implies
//                             g = (m - m_old * beta1) / (1 - beta1), the fresh variance
//                             vf = vf * beta2 + (1 - beta2) * g * g; stores m and vf and, per
//                             chunk, max q with q = (sqrtf(v) + eps) / (sqrtf(vf) + eps) over the
//                             coordinates whose frozen v > 0;
//   k_lamb_onebit_apply       every block takes the maximum over its tensor's chunk partials (all
//                             blocks of a tensor compute the same factor and ratio: no grid
//                             barrier, no float atomic, no finalize launch), then
//                             p -= lr * r * u where v > 0; the tensor's first block stores r and
//                             the new last_factor.
//
// last_factor holds two rows, lf_stride entries apart.  Step t (1-based) reads row (t - 1) & 1 and
// writes row t & 1, and writes every tensor's entry (the old value where the factor stays): other
// blocks of the same launch read the row that no block of that launch writes.
struct LambOnebitArgs {
  float* param;
  float* mom;        // exp_avg
  const float* var;  // the frozen exp_avg_sq: read only
  float* varf;       // exp_avg_sq_fresh
  uint16_t* shadow;
  const TensorRow* tensors;
  const int* adapt;
  float* partials;  // one fp32 per chunk row: the chunk's max q
  const float* r_frozen;
  float* last_factor;  // two rows, lf_stride apart
  float* ratio;
  const int* step;      // nullable device step counter: t = *step + 1
  const float* lr_ptr;  // nullable device lr
  double beta1d;
  float lr, inv_n, beta1, beta2, omb1, omb2, eps, weight_decay;
  float bc1;   // 1 - beta1^t (host value, replaced when step is set)
  float bc2w;  // 1 - beta2^freeze_step
  float factor_min, factor_max, factor_threshold;
  int t, lf_stride;
};

// lr, t and bc1(t) read once per block from device memory (layerwise.hip lw_resolve)
__device__ __forceinline__ void ew_lamb1_resolve(LambOnebitArgs& a) {
  if (a.lr_ptr) a.lr = *a.lr_ptr;
  if (a.step) {
    const int s = *a.step;
    a.t = s + 1;
    a.bc1 = (float)(1.0 - pow(a.beta1d, (double)(s + 1)));
  }
}

__device__ __forceinline__ float ew_wave_fmax(float v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_down(v, d, 64));
  return v;  // valid in lane 0
}

// Block maximum (fmaxf: a NaN never enters, the start is the caller's 0); valid in thread 0
__device__ __forceinline__ float ew_block_fmax(float v, float* ws) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  v = ew_wave_fmax(v);
  if (lane == 0) ws[w] = v;
  __syncthreads();
  float s = 0.0f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < EW_WAVES; ++i) s = fmaxf(s, ws[i]);
  }
  return s;
}

// one element of the stage pass: vf is updated, q joins the thread's maximum where v > 0
__device__ __forceinline__ void ew_lamb1_stage(float m, float m_old, float v, float& vf,
                                               float& qmax, const LambOnebitArgs& a) {
  const float g = (m - m_old * a.beta1) / a.omb1;
  vf = vf * a.beta2 + a.omb2 * (g * g);
  if (v > 0.0f) qmax = fmaxf(qmax, (sqrtf(v) + a.eps) / (sqrtf(vf) + a.eps));
}

__global__ __launch_bounds__(EW_BLOCK) void k_sign_decode_lamb_stage(
    const uint8_t* __restrict__ recv, int nranks, long long stride,
    const ChunkRow* __restrict__ chunks, int scales_off, int bits_off, LambOnebitArgs a) {
  __shared__ float ws[EW_WAVES];
  const ChunkRow c = chunks[blockIdx.x];
  size_t scale_at, words_at;
  ew_sign_where(nullptr, scales_off, bits_off, scale_at, words_at);
  float acc[EW_CU][4];
  ew_sign_acc(recv, nranks, stride, scale_at, words_at, acc);
  float* b = a.mom + c.start;
  float* vf = a.varf + c.start;
  const float* vq = a.var + c.start;
  float qmax = 0.0f;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    if (i >= c.len) continue;
    float mv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) mv[j] = acc[u][j] * a.inv_n;
    if (i + 3 < c.len) {
      const float4 o4 = *reinterpret_cast<const float4*>(b + i);
      const float4 v4 = *reinterpret_cast<const float4*>(vq + i);
      const float4 f4 = *reinterpret_cast<const float4*>(vf + i);
      const float ov[4] = {o4.x, o4.y, o4.z, o4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
      float fv[4] = {f4.x, f4.y, f4.z, f4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) ew_lamb1_stage(mv[j], ov[j], vv[j], fv[j], qmax, a);
      *reinterpret_cast<float4*>(b + i) = make_float4(mv[0], mv[1], mv[2], mv[3]);
      *reinterpret_cast<float4*>(vf + i) = make_float4(fv[0], fv[1], fv[2], fv[3]);
    } else {  // the last elements of a tensor
      for (int j = 0; j < 4 && i + j < c.len; ++j) {
        float fv = vf[i + j];
        ew_lamb1_stage(mv[j], b[i + j], vq[i + j], fv, qmax, a);
        b[i + j] = mv[j];
        vf[i + j] = fv;
      }
    }
  }
  const float cmax = ew_block_fmax(qmax, ws);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = cmax;
}

// LAMB's update direction with the variance's bias correction held at the freeze step
__device__ __forceinline__ void ew_lamb1_step(float& p, float m, float v, float step,
                                              const LambOnebitArgs& a) {
  if (v > 0.0f) {
    float u = (m / a.bc1) / (sqrtf(v / a.bc2w) + a.eps);
    if (a.weight_decay != 0.0f) u = u + a.weight_decay * p;
    p = p - step * u;
  }
}

__global__ __launch_bounds__(EW_BLOCK) void k_lamb_onebit_apply(
    const ChunkRow* __restrict__ chunks, LambOnebitArgs a, SgdArgs key) {
  __shared__ float ws[EW_WAVES];
  __shared__ float rs;
  ew_lamb1_resolve(a);
  ew_key_advance(key);
  const ChunkRow c = chunks[blockIdx.x];
  const TensorRow T = a.tensors[c.tensor];
  float fm = 0.0f;
  for (int j = threadIdx.x; j < T.nchunks; j += EW_BLOCK) fm = fmaxf(fm, a.partials[T.chunk0 + j]);
  const float f_raw = ew_block_fmax(fm, ws);
  if (threadIdx.x == 0) {
    const float lf = a.last_factor[((a.t - 1) & 1) * a.lf_stride + c.tensor];
    float r = 1.0f, f_new = lf;
    if (a.adapt[c.tensor]) {
      r = a.r_frozen[c.tensor];
      if (f_raw != 0.0f) {
        float f = fminf(fmaxf(f_raw, a.factor_min), a.factor_max);
        f = fminf(fmaxf(f, lf * (1.0f - a.factor_threshold)), lf * (1.0f + a.factor_threshold));
        r = r * f;
        f_new = f;
      }
    }
    rs = r;
    if (c.local == 0) {
      a.ratio[c.tensor] = r;
      a.last_factor[(a.t & 1) * a.lf_stride + c.tensor] = f_new;
    }
  }
  __syncthreads();
  const float step = a.lr * rs;
  float* p = a.param + c.start;
  const float* b = a.mom + c.start;
  const float* vq = a.var + c.start;
  uint16_t* sh = a.shadow ? a.shadow + c.start : nullptr;
#pragma unroll 2
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    if (i >= c.len) break;
    if (i + 3 < c.len) {
      const float4 p4 = *reinterpret_cast<const float4*>(p + i);
      const float4 m4 = *reinterpret_cast<const float4*>(b + i);
      const float4 v4 = *reinterpret_cast<const float4*>(vq + i);
      float pv[4] = {p4.x, p4.y, p4.z, p4.w};
      const float mv[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) ew_lamb1_step(pv[j], mv[j], vv[j], step, a);
      *reinterpret_cast<float4*>(p + i) = make_float4(pv[0], pv[1], pv[2], pv[3]);
      if (sh) ew_st4_bf16(sh + i, 4, pv);
    } else {  // the last elements of a tensor
      for (int j = 0; j < 4 && i + j < c.len; ++j) {
        float pv = p[i + j];
        ew_lamb1_step(pv, b[i + j], vq[i + j], step, a);
        p[i + j] = pv;
        if (sh) sh[i + j] = ew_f2bf(pv);
      }
    }
  }
}

}  // namespace

#define EW_LAUNCH(kern, grid, stream, ...) \
  hipLaunchKernelGGL(kern, dim3(grid), dim3(EW_BLOCK), 0, (hipStream_t)(stream), __VA_ARGS__)

// The payload sections (or, slot-addressed, every slot of the table: slot_end is the largest byte
// offset any of them reaches, from the host copy of the table) must lie inside `bytes`.
static void ew_sign_fit(const std::string& who, uintptr_t slots, long long slot_end, int scales_off,
                        int bits_off, int C, long long bytes) {
  if (slots) {
    if (slot_end < 4LL * EW_BM_WORDS + 4 || slot_end > bytes || slot_end > 0x7fffffffLL)
      throw std::runtime_error(who + ": the slot table does not fit the row buffer");
    return;
  }
  if (scales_off < 0 || scales_off % 16 || bits_off % 16 || bits_off < scales_off + 4LL * C ||
      bytes < bits_off + 4LL * EW_BM_WORDS * C)
    throw std::runtime_error(who + ": payload sections do not fit the payload");
}

void ew_sign_encode(const SignEncodeArgs& a) {
  const int C = a.num_chunks;
  if (C <= 0) throw std::runtime_error("ewdml sign: empty bucket");
  ew_sign_fit("ewdml sign", a.slots, a.slot_end, a.scales_off, a.bits_off, C, a.payload_bytes);
  auto* chunks = reinterpret_cast<const ChunkRow*>(a.chunks);
  auto* slots = reinterpret_cast<const int2*>(a.slots);
  GradPtrs g;
  ew_fill_ptrs(g, a.src, a.num_tensors);
  float* resid = reinterpret_cast<float*>(a.resid);
  auto* pay = reinterpret_cast<uint8_t*>(a.payload);
  const SignMom mo{reinterpret_cast<const float*>(a.mom_exp_avg),
                   reinterpret_cast<const float*>(a.mom_param), a.mom_beta1, a.mom_wd};
  if (a.rotate) {
    if (slots || mo.m)
      throw std::runtime_error("ewdml sign: the rotated encode has no slot-addressed and no "
                               "momentum form");
    if (!chunks || !pay) throw std::runtime_error("ewdml sign: missing table");
    if ((a.payload | a.resid) % 16 || a.chunks % 4)
      throw std::runtime_error("ewdml sign: misaligned operand");
    if (resid)
      EW_LAUNCH((k_hsign_encode<true>), C, a.stream, g, resid, chunks, pay, a.scales_off,
                a.bits_off, a.rot_key);
    else
      EW_LAUNCH((k_hsign_encode<false>), C, a.stream, g, resid, chunks, pay, a.scales_off,
                a.bits_off, a.rot_key);
  } else if (mo.m) {  // 1-bit Adam's momentum encode: error feedback always on
    if (!resid) throw std::runtime_error("ewdml sign: the momentum encode needs the residual");
    if (mo.wd != 0.0f && !mo.p)
      throw std::runtime_error("ewdml sign: weight decay needs the parameters");
    EW_LAUNCH((k_sign_encode<true, true>), C, a.stream, g, resid, chunks, pay, a.scales_off,
              a.bits_off, mo, slots);
  } else if (resid) {
    EW_LAUNCH((k_sign_encode<true, false>), C, a.stream, g, resid, chunks, pay, a.scales_off,
              a.bits_off, mo, slots);
  } else {
    EW_LAUNCH((k_sign_encode<false, false>), C, a.stream, g, resid, chunks, pay, a.scales_off,
              a.bits_off, mo, slots);
  }
  EW_CHECK_LAUNCH();
}

void ew_sign_reduce_encode(const SignReduceArgs& a) {
  const int C = a.num_chunks;
  if (C <= 0 || a.nranks <= 0 || a.nranks > EW_MAX_RANKS)
    throw std::runtime_error("ewdml sign reduce: nothing to reduce, or too many ranks");
  ew_sign_fit("ewdml sign reduce", 0, 0, a.scales_off, a.bits_off, C, a.stride);
  ew_sign_fit("ewdml sign reduce", 0, 0, a.scales_off, a.bits_off, C, a.out_bytes);
  if (!a.recv || !a.out || !a.sresid || !a.chunks)
    throw std::runtime_error("ewdml sign reduce: needs the received rows, the server residual "
                             "and the owner's row");
  EW_LAUNCH(k_sign_reduce_encode, C, a.stream, reinterpret_cast<const uint8_t*>(a.recv), a.nranks,
            a.stride, reinterpret_cast<const ChunkRow*>(a.chunks), a.scales_off, a.bits_off,
            a.inv_n, reinterpret_cast<float*>(a.sresid), reinterpret_cast<uint8_t*>(a.out));
  EW_CHECK_LAUNCH();
}

void ew_sign_decode_onebit(const SignOnebitArgs& a) {
  const int C = a.num_chunks;
  if (C <= 0 || a.nranks <= 0) throw std::runtime_error("ewdml 1-bit Adam: nothing to decode");
  if (a.slots && a.nranks != 1)
    throw std::runtime_error("ewdml 1-bit Adam: the slot-addressed decode reads one row buffer");
  ew_sign_fit("ewdml 1-bit Adam", a.slots, a.slot_end, a.scales_off, a.bits_off, C, a.stride);
  if (!a.param || !a.exp_avg || !a.exp_avg_sq)
    throw std::runtime_error("ewdml 1-bit Adam: the step needs param, exp_avg and exp_avg_sq");
  if (a.freeze_step < 1) throw std::runtime_error("ewdml 1-bit Adam: freeze_step must be >= 1");
  OnebitArgs oa{a.lr_step, a.inv_n, a.eps, a.beta1, a.beta2, a.freeze_step,
                reinterpret_cast<const int*>(a.step), a.lr,
                reinterpret_cast<const float*>(a.lr_ptr)};
  SgdArgs key{};
  key.key_state = reinterpret_cast<uint32_t*>(a.key_state);
  key.key_seed = a.key_seed;
  key.key_rank = a.key_rank;
  EW_LAUNCH(k_sign_decode_onebit, C, a.stream, reinterpret_cast<const uint8_t*>(a.recv), a.nranks,
            a.stride, reinterpret_cast<const ChunkRow*>(a.chunks), a.scales_off, a.bits_off,
            reinterpret_cast<float*>(a.param), reinterpret_cast<float*>(a.exp_avg),
            reinterpret_cast<const float*>(a.exp_avg_sq), reinterpret_cast<uint16_t*>(a.shadow),
            oa, key, reinterpret_cast<const int2*>(a.slots));
  EW_CHECK_LAUNCH();
}

static LambOnebitArgs ew_lamb1_args(const SignLambArgs& h) {
  if (h.num_chunks <= 0 || h.num_tensors <= 0 || h.lf_stride < h.num_tensors)
    throw std::runtime_error("ewdml 1-bit LAMB: nothing to step");
  if (!h.chunks || !h.tensors || !h.adapt || !h.partials || !h.r_frozen || !h.last_factor ||
      !h.ratio)
    throw std::runtime_error("ewdml 1-bit LAMB: missing table");
  if (!h.param || !h.exp_avg || !h.exp_avg_sq || !h.exp_avg_sq_fresh)
    throw std::runtime_error("ewdml 1-bit LAMB: the step needs param, exp_avg, exp_avg_sq and "
                             "exp_avg_sq_fresh");
  if ((h.param | h.exp_avg | h.exp_avg_sq | h.exp_avg_sq_fresh) % 16 || h.shadow % 8 ||
      (h.partials | h.r_frozen | h.last_factor | h.ratio | h.adapt | h.step | h.lr_ptr) % 4)
    throw std::runtime_error("ewdml 1-bit LAMB: misaligned operand");
  if (h.freeze_step < 1 || (!h.step && h.t <= h.freeze_step))
    throw std::runtime_error("ewdml 1-bit LAMB: the compressed stage starts after freeze_step >= 1");
  LambOnebitArgs a{};
  a.param = reinterpret_cast<float*>(h.param);
  a.mom = reinterpret_cast<float*>(h.exp_avg);
  a.var = reinterpret_cast<const float*>(h.exp_avg_sq);
  a.varf = reinterpret_cast<float*>(h.exp_avg_sq_fresh);
  a.shadow = reinterpret_cast<uint16_t*>(h.shadow);
  a.tensors = reinterpret_cast<const TensorRow*>(h.tensors);
  a.adapt = reinterpret_cast<const int*>(h.adapt);
  a.partials = reinterpret_cast<float*>(h.partials);
  a.r_frozen = reinterpret_cast<const float*>(h.r_frozen);
  a.last_factor = reinterpret_cast<float*>(h.last_factor);
  a.ratio = reinterpret_cast<float*>(h.ratio);
  a.step = reinterpret_cast<const int*>(h.step);
  a.lr_ptr = reinterpret_cast<const float*>(h.lr_ptr);
  a.beta1d = h.beta1;
  a.lr = h.lr; a.inv_n = h.inv_n; a.eps = h.eps; a.weight_decay = h.weight_decay;
  a.beta1 = (float)h.beta1; a.beta2 = (float)h.beta2;
  a.omb1 = 1.0f - a.beta1; a.omb2 = 1.0f - a.beta2;  // formed in fp32, as the momentum encode's
  a.bc1 = h.bc1;
  a.bc2w = h.bc2w;
  a.factor_min = h.factor_min; a.factor_max = h.factor_max;
  a.factor_threshold = h.factor_threshold;
  a.t = h.t; a.lf_stride = h.lf_stride;
  return a;
}

void ew_sign_decode_lamb_stage(const SignLambArgs& h) {
  if (h.nranks <= 0) throw std::runtime_error("ewdml 1-bit LAMB: nothing to decode");
  if (!h.recv || h.recv % 16 || h.stride % 16)
    throw std::runtime_error("ewdml 1-bit LAMB: the received rows must be 16-byte aligned");
  ew_sign_fit("ewdml 1-bit LAMB", 0, 0, h.scales_off, h.bits_off, h.num_chunks, h.stride);
  const LambOnebitArgs a = ew_lamb1_args(h);
  EW_LAUNCH(k_sign_decode_lamb_stage, h.num_chunks, h.stream,
            reinterpret_cast<const uint8_t*>(h.recv), h.nranks, h.stride,
            reinterpret_cast<const ChunkRow*>(h.chunks), h.scales_off, h.bits_off, a);
  EW_CHECK_LAUNCH();
}

void ew_lamb_onebit_apply(const SignLambArgs& h) {
  const LambOnebitArgs a = ew_lamb1_args(h);
  SgdArgs key{};
  key.key_state = reinterpret_cast<uint32_t*>(h.key_state);
  key.key_seed = h.key_seed;
  key.key_rank = h.key_rank;
  EW_LAUNCH(k_lamb_onebit_apply, h.num_chunks, h.stream,
            reinterpret_cast<const ChunkRow*>(h.chunks), a, key);
  EW_CHECK_LAUNCH();
}

void ew_sign_decode_apply(const SignDecodeArgs& a) {
  const int C = a.num_chunks;
  if (C <= 0 || a.nranks <= 0) throw std::runtime_error("ewdml sign decode: nothing to decode");
  if (a.slots && a.nranks != 1)
    throw std::runtime_error("ewdml sign decode: the slot-addressed decode reads one row buffer");
  ew_sign_fit("ewdml sign decode", a.slots, a.slot_end, a.scales_off, a.bits_off, C, a.stride);
  const StepArgs& st = a.step;
  ew_step_check("ewdml sign decode", st, false);
  const SgdArgs sa = ew_sgd_args(st);
  if (a.rotate) {
    if (a.slots)
      throw std::runtime_error("ewdml sign decode: the rotated decode has no slot-addressed form");
    if (!a.recv || !a.chunks) throw std::runtime_error("ewdml sign decode: missing table");
    if (a.recv % 16 || a.stride % 4 || a.chunks % 4)
      throw std::runtime_error("ewdml sign decode: misaligned operand");
    EW_LAUNCH(k_hsign_decode_apply, C, a.stream, reinterpret_cast<const uint8_t*>(a.recv),
              a.nranks, a.stride, reinterpret_cast<const ChunkRow*>(a.chunks), a.scales_off,
              a.bits_off, reinterpret_cast<float*>(st.param), reinterpret_cast<float*>(st.mom),
              reinterpret_cast<float*>(st.grad_out), reinterpret_cast<uint16_t*>(st.shadow), sa,
              st.apply, a.rot_key);
    EW_CHECK_LAUNCH();
    return;
  }
  EW_LAUNCH(k_sign_decode_apply, C, a.stream, reinterpret_cast<const uint8_t*>(a.recv), a.nranks,
            a.stride, reinterpret_cast<const ChunkRow*>(a.chunks), a.scales_off, a.bits_off,
            reinterpret_cast<float*>(st.param), reinterpret_cast<float*>(st.mom),
            reinterpret_cast<float*>(st.grad_out), reinterpret_cast<uint16_t*>(st.shadow), sa,
            st.apply, reinterpret_cast<const int2*>(a.slots));
  EW_CHECK_LAUNCH();
}
