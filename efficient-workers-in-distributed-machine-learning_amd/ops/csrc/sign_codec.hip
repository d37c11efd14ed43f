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
#include "common.h"
#include "ewdml_ops.h"

namespace {

template <bool EF>
__global__ __launch_bounds__(EW_BLOCK) void k_sign_encode(GradPtrs gp, float* __restrict__ resid,
                                                          const ChunkRow* __restrict__ chunks,
                                                          uint8_t* __restrict__ payload,
                                                          int scales_off, int bits_off) {
  __shared__ float wsf[EW_WAVES];
  __shared__ float s_scale;
  const ChunkRow c = chunks[blockIdx.x];
  float4 e[EW_CU];
  ew_ld_chunk(gp, nullptr, c, e);  // positions past c.len read as 0: |e| = 0, bit = 0
  if (EF) {
    float4 r[EW_CU];
    ew_ld_chunk(gp, resid, c, r);
#pragma unroll
    for (int u = 0; u < EW_CU; ++u)
      e[u] = make_float4(e[u].x + r[u].x, e[u].y + r[u].y, e[u].z + r[u].z, e[u].w + r[u].w);
  }
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
    const float sc = total / (float)c.len;
    s_scale = sc;
    reinterpret_cast<float*>(payload + scales_off)[blockIdx.x] = sc;
  }
  if (blockIdx.x == 0) {  // the scales section's alignment pad: payloads compare bytewise
    const int slots = (bits_off - scales_off) >> 2;
    for (int i = (int)gridDim.x + (int)threadIdx.x; i < slots; i += EW_BLOCK)
      reinterpret_cast<float*>(payload + scales_off)[i] = 0.0f;
  }
  __syncthreads();
  const float scale = s_scale;

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
  uint32_t* words = reinterpret_cast<uint32_t*>(payload + bits_off) + (size_t)blockIdx.x * EW_BM_WORDS;
  words[k * (EW_BLOCK / 8) + (threadIdx.x >> 3)] = mine;

  if (EF) {
#pragma unroll
    for (int u = 0; u < EW_CU; ++u) {
      e[u].x = e[u].x - (e[u].x < 0.0f ? -scale : scale);
      e[u].y = e[u].y - (e[u].y < 0.0f ? -scale : scale);
      e[u].z = e[u].z - (e[u].z < 0.0f ? -scale : scale);
      e[u].w = e[u].w - (e[u].w < 0.0f ? -scale : scale);
    }
    ew_st_chunk(resid + c.start, c.len, e);
  }
}

__global__ __launch_bounds__(EW_BLOCK) void k_sign_decode_apply(
    const uint8_t* __restrict__ recv, int nranks, long long stride,
    const ChunkRow* __restrict__ chunks, int scales_off, int bits_off, float* __restrict__ param,
    float* __restrict__ mom, float* __restrict__ grad_out, uint16_t* __restrict__ shadow,
    SgdArgs sa, int apply) {
  const ChunkRow c = chunks[blockIdx.x];
  ew_sgd_resolve(sa);
  ew_key_advance(sa);
  const int shift = 4 * (threadIdx.x & 7);
  const size_t word0 = (size_t)blockIdx.x * EW_BM_WORDS + (threadIdx.x >> 3);
  float acc[EW_CU][4];
#pragma unroll
  for (int u = 0; u < EW_CU; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[u][j] = 0.0f;
  for (int r = 0; r < nranks; ++r) {
    const uint8_t* pay = recv + r * stride;
    const float scale = reinterpret_cast<const float*>(pay + scales_off)[blockIdx.x];
    const uint32_t* words = reinterpret_cast<const uint32_t*>(pay + bits_off) + word0;
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
  float* p = param + c.start;
  float* b = mom ? mom + c.start : nullptr;
  float* go = grad_out ? grad_out + c.start : nullptr;
  uint16_t* sh = shadow ? shadow + c.start : nullptr;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    if (i >= c.len) continue;
    float gv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gv[j] = acc[u][j] * sa.grad_scale;
    if (i + 3 < c.len) {
      if (go) *reinterpret_cast<float4*>(go + i) = make_float4(gv[0], gv[1], gv[2], gv[3]);
      if (apply) {
        const float4 p4 = *reinterpret_cast<const float4*>(p + i);
        const float4 b4 = b ? *reinterpret_cast<const float4*>(b + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        float pv[4] = {p4.x, p4.y, p4.z, p4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) ew_sgd(pv[j], bv[j], gv[j], sa);
        *reinterpret_cast<float4*>(p + i) = make_float4(pv[0], pv[1], pv[2], pv[3]);
        if (b) *reinterpret_cast<float4*>(b + i) = make_float4(bv[0], bv[1], bv[2], bv[3]);
        if (sh) ew_st4_bf16(sh + i, 4, pv);
      }
    } else {  // the last elements of a tensor
      for (int j = 0; j < 4 && i + j < c.len; ++j) {
        if (go) go[i + j] = gv[j];
        if (apply) {
          float pv = p[i + j], bv = b ? b[i + j] : 0.0f;
          ew_sgd(pv, bv, gv[j], sa);
          p[i + j] = pv;
          if (b) b[i + j] = bv;
          if (sh) sh[i + j] = ew_f2bf(pv);
        }
      }
    }
  }
}

}  // namespace

#define EW_LAUNCH(kern, grid, stream, ...) \
  hipLaunchKernelGGL(kern, dim3(grid), dim3(EW_BLOCK), 0, (hipStream_t)(stream), __VA_ARGS__)

void ew_sign_encode(const SignEncodeArgs& a) {
  const int C = a.num_chunks;
  if (C <= 0) throw std::runtime_error("ewdml sign: empty bucket");
  if (a.scales_off % 16 || a.bits_off % 16 || a.bits_off < a.scales_off + 4LL * C ||
      a.payload_bytes < a.bits_off + 4LL * EW_BM_WORDS * C)
    throw std::runtime_error("ewdml sign: payload sections do not fit the payload");
  auto* chunks = reinterpret_cast<const ChunkRow*>(a.chunks);
  GradPtrs g;
  ew_fill_ptrs(g, a.grad_ptrs, a.n_grad_ptrs, a.num_tensors, a.bf16_mask, a.n_bf16_mask);
  float* resid = reinterpret_cast<float*>(a.resid);
  auto* pay = reinterpret_cast<uint8_t*>(a.payload);
  if (resid)
    EW_LAUNCH(k_sign_encode<true>, C, a.stream, g, resid, chunks, pay, a.scales_off, a.bits_off);
  else
    EW_LAUNCH(k_sign_encode<false>, C, a.stream, g, resid, chunks, pay, a.scales_off, a.bits_off);
  EW_CHECK_LAUNCH();
}

void ew_sign_decode_apply(const SignDecodeArgs& a) {
  const int C = a.num_chunks;
  if (C <= 0 || a.nranks <= 0) throw std::runtime_error("ewdml sign decode: nothing to decode");
  if (a.scales_off % 16 || a.bits_off % 16 || a.bits_off < a.scales_off + 4LL * C ||
      a.stride < a.bits_off + 4LL * EW_BM_WORDS * C)
    throw std::runtime_error("ewdml sign decode: payload sections do not fit the payload");
  if (a.apply && !a.param) throw std::runtime_error("ewdml sign decode: apply needs the parameters");
  if (!a.apply && !a.grad_out) throw std::runtime_error("ewdml sign decode: nothing to write");
  if (a.apply && !a.mom && (a.momentum != 0.0f || a.nesterov))
    throw std::runtime_error("ewdml sign decode: a momentum step needs the momentum buffer");
  SgdArgs sa{a.lr, a.momentum, a.dampening, a.weight_decay, a.grad_scale, a.nesterov, a.first,
             reinterpret_cast<uint32_t*>(a.key_state), a.key_seed, a.key_rank};
  sa.lr_ptr = reinterpret_cast<const float*>(a.lr_ptr);
  EW_LAUNCH(k_sign_decode_apply, C, a.stream, reinterpret_cast<const uint8_t*>(a.recv), a.nranks,
            a.stride, reinterpret_cast<const ChunkRow*>(a.chunks), a.scales_off, a.bits_off,
            reinterpret_cast<float*>(a.param), reinterpret_cast<float*>(a.mom),
            reinterpret_cast<float*>(a.grad_out), reinterpret_cast<uint16_t*>(a.shadow), sa,
            a.apply);
  EW_CHECK_LAUNCH();
}
