// Lion (Chen et al. 2023) over the flat parameter buffer, and Distributed Lion's 1-bit exchange
// (Liu et al. 2024): every rank sends the sign of its own update direction, one bit per element
// and nothing else, and every rank applies the majority vote or the average of the received
// signs.  gfx950, wave64.
//
// All arithmetic is fp32 with every operation rounded on its own (-ffp-contract=off), 1 - beta
// formed in fp32 (compress/oracle.py lion_apply / encode_vote / vote_apply, bit for bit):
//
//   c = m * beta1 + (1 - beta1) * g          u = sign(c)   (0 and NaN give 0)
//   p = p - lr * (u + wd * p)                (wd == 0: p = p - lr * u)
//   m = m * beta2 + (1 - beta2) * g
//
// Payload (compress/plan.py, kind "vote"): bits u32[256 * C] and nothing else.  Chunk c owns words
// [256 c, 256 c + 256); element i of the chunk is bit i & 31 of word i >> 5; a set bit is -1, a
// clear bit +1; bits past the chunk's length are 0.  One bit cannot say 0, so an exact zero votes
// by the parity of i + step + rank: its votes cancel over two steps and across an even world.
//
// The decode counts set bits in integers, so every rank forms the same update by construction.
//
// The two-stage vote (parallel/twostage.py TwoStageVoteExchange) adds a slot-addressed form of the
// encode and of the apply -- `slots` (int2 per chunk of the shard-major plan, compress/plan.py
// TwoStagePlan kind "vote") holds in .y the byte offset of the chunk's 256 words inside an [N, P]
// row buffer (.x is the sign codec's scale offset and is not read) -- and the owner step
// k_vote_reduce, which turns the N votes on a shard into one bit per element again.
#include "common.h"
#include "ewdml_ops.h"

namespace {

struct LionArgs {
  float lr, beta1, beta2, wd, grad_scale;
  const float* lr_ptr;  // nullable device lr (overrides lr)
};

__device__ __forceinline__ void ew_lion_resolve(LionArgs& a) {
  if (a.lr_ptr) a.lr = *a.lr_ptr;
}

// p -= lr * (d + wd * p): the step both the dense kernel (d = sign(c)) and the vote take
__device__ __forceinline__ void ew_lion_step(float& p, float d, float lr, float wd) {
  if (wd != 0.0f) d = d + wd * p;
  p = p - lr * d;
}

__device__ __forceinline__ void ew_lion(float& p, float& m, float g, const LionArgs& a, float c1,
                                        float c2) {
  const float c = m * a.beta1 + c1 * g;
  ew_lion_step(p, (float)(c > 0.0f) - (float)(c < 0.0f), a.lr, a.wd);
  m = m * a.beta2 + c2 * g;
}

template <int GT>
__device__ __forceinline__ float ew_load_grad1(const void* g, long long i) {
  if (GT == 0) return reinterpret_cast<const float*>(g)[i];
  if (GT == 1) return ew_bf16f(reinterpret_cast<const uint16_t*>(g)[i]);
  return __half2float(reinterpret_cast<const __half*>(g)[i]);
}

template <int GT>
__global__ __launch_bounds__(EW_BLOCK) void k_lion_flat(float* __restrict__ p, float* __restrict__ m,
                                                        const void* __restrict__ g, long long n,
                                                        uint16_t* __restrict__ shadow, LionArgs a) {
  ew_lion_resolve(a);
  const float c1 = 1.0f - a.beta1, c2 = 1.0f - a.beta2;
  const long long n4 = n / 4;
  for (long long i = blockIdx.x * (long long)EW_BLOCK + threadIdx.x; i < n4;
       i += (long long)gridDim.x * EW_BLOCK) {
    float gv[4];
    ew_load_grad4<GT>(g, 4 * i, gv);
    float4 pv = reinterpret_cast<float4*>(p)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    ew_lion(pv.x, mv.x, gv[0] * a.grad_scale, a, c1, c2);
    ew_lion(pv.y, mv.y, gv[1] * a.grad_scale, a, c1, c2);
    ew_lion(pv.z, mv.z, gv[2] * a.grad_scale, a, c1, c2);
    ew_lion(pv.w, mv.w, gv[3] * a.grad_scale, a, c1, c2);
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    if (shadow) {
      const float w[4] = {pv.x, pv.y, pv.z, pv.w};
      ew_st4_bf16(shadow + 4 * i, 4, w);
    }
  }
  // the last n % 4 elements
  const long long t = 4 * n4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    float pv = p[t], mv = m[t];
    ew_lion(pv, mv, ew_load_grad1<GT>(g, t) * a.grad_scale, a, c1, c2);
    p[t] = pv;
    m[t] = mv;
    if (shadow) shadow[t] = ew_f2bf(pv);
  }
}

// The vote of one element: -1 (bit set) when c < 0, and an exact zero by the parity `odd` of
// i + step + rank.  NaN compares false twice: bit 0.
__device__ __forceinline__ uint32_t ew_lion_bit(float c, bool valid, uint32_t odd) {
  return (uint32_t)(valid && (c < 0.0f || (c == 0.0f && odd)));
}

// SLOT: chunk c's words go to byte slots[c].y of `payload` (the two-stage push's [N, P] rows)
// and bits_off is not read; otherwise to the bucket's own layout (slots is not read).
template <bool SLOT>
__global__ __launch_bounds__(EW_BLOCK) void k_lion_encode(GradPtrs gp, float* __restrict__ mom,
                                                          const ChunkRow* __restrict__ chunks,
                                                          uint8_t* __restrict__ payload,
                                                          int bits_off, float beta1, float beta2,
                                                          int step, const int* __restrict__ step_ptr,
                                                          int rank, const int2* __restrict__ slots) {
  const ChunkRow c = chunks[blockIdx.x];
  if (step_ptr) step = *step_ptr + 1;  // the 1-based step of this replay
  float4 g[EW_CU], m[EW_CU];
  ew_ld_chunk(gp, nullptr, c, g);  // positions past c.len read as 0 and are masked below
  ew_ld_chunk(gp, mom, c, m);
  const float c1 = 1.0f - beta1, c2 = 1.0f - beta2;
  // element i = ew_chunk_idx(u) + j has the parity of j: ew_chunk_idx is a multiple of 4
  const uint32_t sr = (uint32_t)(step + rank) & 1u;

  // the nibble / shuffle packing of ew_sign_pack (sign_codec.hip): thread t holds elements 4t ..
  // 4t + 3 of each slab, a nibble of word u * 32 + (t >> 3); lane k of a group of 8 stores slab
  // k's word, so the block's 256 words go out as one dword store per thread
  const int k = threadIdx.x & 7;
  uint32_t mine = 0;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    const float cx = m[u].x * beta1 + c1 * g[u].x, cy = m[u].y * beta1 + c1 * g[u].y;
    const float cz = m[u].z * beta1 + c1 * g[u].z, cw = m[u].w * beta1 + c1 * g[u].w;
    uint32_t w = ew_lion_bit(cx, i < c.len, sr) | (ew_lion_bit(cy, i + 1 < c.len, sr ^ 1u) << 1) |
                 (ew_lion_bit(cz, i + 2 < c.len, sr) << 2) |
                 (ew_lion_bit(cw, i + 3 < c.len, sr ^ 1u) << 3);
    w <<= 4 * k;
    w |= __shfl_xor(w, 1, 64);
    w |= __shfl_xor(w, 2, 64);
    w |= __shfl_xor(w, 4, 64);
    mine = (u == k) ? w : mine;
  }
  const size_t words_at =
      SLOT ? (size_t)slots[blockIdx.x].y : (size_t)bits_off + 4 * (size_t)blockIdx.x * EW_BM_WORDS;
  uint32_t* words = reinterpret_cast<uint32_t*>(payload + words_at);
  words[k * (EW_BLOCK / 8) + (threadIdx.x >> 3)] = mine;

#pragma unroll
  for (int u = 0; u < EW_CU; ++u)
    m[u] = make_float4(m[u].x * beta2 + c2 * g[u].x, m[u].y * beta2 + c2 * g[u].y,
                       m[u].z * beta2 + c2 * g[u].z, m[u].w * beta2 + c2 * g[u].w);
  ew_st_chunk(mom + c.start, c.len, m);
}

// s = N - 2 * (set bits over the N rows), an integer; majority: d = sign(s), a tie gives 0;
// average: d = float(s) * inv_n.  SLOT (the two-stage pull; nranks = 1, so d = 1 - 2 * bit): chunk
// c's words are read at byte slots[c].y of `recv`, the gathered [N, P] rows.
template <bool AVG, bool SLOT>
__global__ __launch_bounds__(EW_BLOCK) void k_lion_vote_apply(
    const uint8_t* __restrict__ recv, int nranks, long long stride,
    const ChunkRow* __restrict__ chunks, int bits_off, float* __restrict__ param,
    uint16_t* __restrict__ shadow, LionArgs a, float inv_n, SgdArgs key,
    const int2* __restrict__ slots) {
  const ChunkRow c = chunks[blockIdx.x];
  ew_lion_resolve(a);
  ew_key_advance(key);
  const int shift = 4 * (threadIdx.x & 7);
  int cnt[EW_CU][4];
#pragma unroll
  for (int u = 0; u < EW_CU; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt[u][j] = 0;
  const size_t words_at =
      SLOT ? (size_t)slots[blockIdx.x].y : (size_t)bits_off + 4 * (size_t)blockIdx.x * EW_BM_WORDS;
  for (int r = 0; r < nranks; ++r) {
    const uint32_t* words =
        reinterpret_cast<const uint32_t*>(recv + r * stride + words_at) + (threadIdx.x >> 3);
    uint32_t w[EW_CU];
#pragma unroll
    for (int u = 0; u < EW_CU; ++u) w[u] = words[u * (EW_BLOCK / 8)];
#pragma unroll
    for (int u = 0; u < EW_CU; ++u) {
      const uint32_t nib = w[u] >> shift;
#pragma unroll
      for (int j = 0; j < 4; ++j) cnt[u][j] += (int)((nib >> j) & 1u);
    }
  }
  float* p = param + c.start;
  uint16_t* sh = shadow ? shadow + c.start : nullptr;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    if (i >= c.len) continue;
    float d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = nranks - 2 * cnt[u][j];
      d[j] = AVG ? (float)s * inv_n : (float)((s > 0) - (s < 0));
    }
    if (i + 3 < c.len) {
      const float4 p4 = *reinterpret_cast<const float4*>(p + i);
      float pv[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) ew_lion_step(pv[j], d[j], a.lr, a.wd);
      *reinterpret_cast<float4*>(p + i) = make_float4(pv[0], pv[1], pv[2], pv[3]);
      if (sh) ew_st4_bf16(sh + i, 4, pv);
    } else {  // the last elements of a tensor
      for (int j = 0; j < 4 && i + j < c.len; ++j) {
        float pv = p[i + j];
        ew_lion_step(pv, d[j], a.lr, a.wd);
        p[i + j] = pv;
        if (sh) sh[i + j] = ew_f2bf(pv);
      }
    }
  }
}

// The two-stage vote's owner step: one block per chunk of the owner's shard.  Per element s = N -
// 2 * (set bits over the N rows of recv), counted in integer registers as above; the output bit is
// (s < 0) | (s == 0 & the bit of row `owner`): one bit cannot say 0, so the owner's own vote breaks
// a tie.  Padding bits are 0 in every row, so s = N > 0 and they stay 0: no chunk table is read.
// Packed as in k_lion_encode, one dword store per thread into the owner's row `out`.
__global__ __launch_bounds__(EW_BLOCK) void k_vote_reduce(const uint8_t* __restrict__ recv,
                                                          int nranks, long long stride, int owner,
                                                          int bits_off, uint8_t* __restrict__ out) {
  const int k = threadIdx.x & 7, shift = 4 * k;
  int cnt[EW_CU][4];
  uint32_t own[EW_CU];
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    own[u] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt[u][j] = 0;
  }
  const size_t words_at = (size_t)bits_off + 4 * (size_t)blockIdx.x * EW_BM_WORDS;
  for (int r = 0; r < nranks; ++r) {
    const uint32_t* words =
        reinterpret_cast<const uint32_t*>(recv + r * stride + words_at) + (threadIdx.x >> 3);
    uint32_t w[EW_CU];
#pragma unroll
    for (int u = 0; u < EW_CU; ++u) w[u] = words[u * (EW_BLOCK / 8)];
#pragma unroll
    for (int u = 0; u < EW_CU; ++u) {
      const uint32_t nib = (w[u] >> shift) & 15u;
      own[u] = (r == owner) ? nib : own[u];
#pragma unroll
      for (int j = 0; j < 4; ++j) cnt[u][j] += (int)((nib >> j) & 1u);
    }
  }
  uint32_t mine = 0;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = nranks - 2 * cnt[u][j];
      w |= (uint32_t)(s < 0 || (s == 0 && ((own[u] >> j) & 1u))) << j;
    }
    w <<= shift;
    w |= __shfl_xor(w, 1, 64);
    w |= __shfl_xor(w, 2, 64);
    w |= __shfl_xor(w, 4, 64);
    mine = (u == k) ? w : mine;
  }
  reinterpret_cast<uint32_t*>(out + words_at)[k * (EW_BLOCK / 8) + (threadIdx.x >> 3)] = mine;
}

inline int ew_lion_grid(long long n4) {
  long long b = (n4 + EW_BLOCK - 1) / EW_BLOCK;
  return (int)(b < 2048 ? (b > 0 ? b : 1) : 2048);  // 8 blocks per CU, grid-stride the rest
}

}  // namespace

#define EW_LAUNCH(kern, grid, stream, ...) \
  hipLaunchKernelGGL(kern, dim3(grid), dim3(EW_BLOCK), 0, (hipStream_t)(stream), __VA_ARGS__)

void ew_lion_flat(const LionFlatArgs& a) {
  if (a.n <= 0 || !a.param || !a.exp_avg || !a.grad)
    throw std::runtime_error("ewdml lion: the step needs param, exp_avg and the gradient");
  LionArgs la{a.lr, a.beta1, a.beta2, a.weight_decay, a.grad_scale,
              reinterpret_cast<const float*>(a.lr_ptr)};
  auto* p = reinterpret_cast<float*>(a.param);
  auto* m = reinterpret_cast<float*>(a.exp_avg);
  auto* g = reinterpret_cast<const void*>(a.grad);
  auto* sh = reinterpret_cast<uint16_t*>(a.shadow);
  const int grid = ew_lion_grid(a.n / 4);
  if (a.grad_dtype == 0) EW_LAUNCH(k_lion_flat<0>, grid, a.stream, p, m, g, a.n, sh, la);
  else if (a.grad_dtype == 1) EW_LAUNCH(k_lion_flat<1>, grid, a.stream, p, m, g, a.n, sh, la);
  else EW_LAUNCH(k_lion_flat<2>, grid, a.stream, p, m, g, a.n, sh, la);
  EW_CHECK_LAUNCH();
}

// The payload's words (256 per chunk from bits_off, 16-byte aligned) must lie inside `bytes`.
static void ew_vote_fit(const std::string& who, int bits_off, int C, long long bytes) {
  if (bits_off < 0 || bits_off % 16 || bytes < bits_off + 4LL * EW_BM_WORDS * C)
    throw std::runtime_error(who + ": the bit words do not fit the payload");
}

// Slot-addressed: every slot of the table must lie inside the row buffer.  slot_end is the largest
// byte offset a slot reaches (compress/plan.py TwoStagePlan; ops/__init__.py checks each slot).
static void ew_vote_slots_fit(const std::string& who, long long slot_end, long long bytes) {
  if (slot_end < 4LL * EW_BM_WORDS || slot_end > bytes || slot_end > 0x7fffffffLL)
    throw std::runtime_error(who + ": the slot table does not fit the row buffer");
}

void ew_lion_encode(const LionEncodeArgs& a) {
  const int C = a.num_chunks;
  if (C <= 0) throw std::runtime_error("ewdml lion encode: empty bucket");
  if (a.slots) ew_vote_slots_fit("ewdml lion encode", a.slot_end, a.payload_bytes);
  else ew_vote_fit("ewdml lion encode", a.bits_off, C, a.payload_bytes);
  if (!a.exp_avg || !a.payload || !a.chunks)
    throw std::runtime_error("ewdml lion encode: needs exp_avg, the payload and the chunk table");
  GradPtrs g;
  ew_fill_ptrs(g, a.src, a.num_tensors);
  auto* mom = reinterpret_cast<float*>(a.exp_avg);
  auto* chunks = reinterpret_cast<const ChunkRow*>(a.chunks);
  auto* payload = reinterpret_cast<uint8_t*>(a.payload);
  auto* step_ptr = reinterpret_cast<const int*>(a.step_ptr);
  auto* slots = reinterpret_cast<const int2*>(a.slots);
  if (slots)
    EW_LAUNCH(k_lion_encode<true>, C, a.stream, g, mom, chunks, payload, a.bits_off, a.beta1,
              a.beta2, a.step, step_ptr, a.rank, slots);
  else
    EW_LAUNCH(k_lion_encode<false>, C, a.stream, g, mom, chunks, payload, a.bits_off, a.beta1,
              a.beta2, a.step, step_ptr, a.rank, slots);
  EW_CHECK_LAUNCH();
}

void ew_vote_reduce(const VoteReduceArgs& a) {
  const int C = a.num_chunks;
  if (C <= 0 || a.nranks <= 0) throw std::runtime_error("ewdml vote reduce: nothing to reduce");
  if (a.owner < 0 || a.owner >= a.nranks)
    throw std::runtime_error("ewdml vote reduce: the owner row is not one of the received rows");
  if (a.stride % 16) throw std::runtime_error("ewdml vote reduce: rows must be 16-byte multiples");
  ew_vote_fit("ewdml vote reduce", a.bits_off, C, a.stride);
  ew_vote_fit("ewdml vote reduce (out)", a.bits_off, C, a.out_bytes);
  if (!a.recv || !a.out) throw std::runtime_error("ewdml vote reduce: needs the rows and the output");
  EW_LAUNCH(k_vote_reduce, C, a.stream, reinterpret_cast<const uint8_t*>(a.recv), a.nranks,
            a.stride, a.owner, a.bits_off, reinterpret_cast<uint8_t*>(a.out));
  EW_CHECK_LAUNCH();
}

void ew_lion_vote_apply(const LionVoteArgs& a) {
  const int C = a.num_chunks;
  if (C <= 0 || a.nranks <= 0) throw std::runtime_error("ewdml lion vote: nothing to decode");
  if (a.slots) {
    if (a.nranks != 1 || a.average)
      throw std::runtime_error("ewdml lion vote: the slot-addressed apply reads one row buffer and "
                               "takes its bit as the direction");
    ew_vote_slots_fit("ewdml lion vote", a.slot_end, a.stride);
  } else {
    ew_vote_fit("ewdml lion vote", a.bits_off, C, a.stride);
  }
  if (!a.recv || !a.param || !a.chunks)
    throw std::runtime_error("ewdml lion vote: needs the received rows, the parameters and the "
                             "chunk table");
  LionArgs la{a.lr, 0.0f, 0.0f, a.weight_decay, 1.0f, reinterpret_cast<const float*>(a.lr_ptr)};
  SgdArgs key{};
  key.key_state = reinterpret_cast<uint32_t*>(a.key_state);
  key.key_seed = a.key_seed;
  key.key_rank = a.key_rank;
  auto* recv = reinterpret_cast<const uint8_t*>(a.recv);
  auto* chunks = reinterpret_cast<const ChunkRow*>(a.chunks);
  auto* p = reinterpret_cast<float*>(a.param);
  auto* sh = reinterpret_cast<uint16_t*>(a.shadow);
  auto* slots = reinterpret_cast<const int2*>(a.slots);
  if (slots)
    EW_LAUNCH((k_lion_vote_apply<false, true>), C, a.stream, recv, a.nranks, a.stride, chunks,
              a.bits_off, p, sh, la, a.inv_n, key, slots);
  else if (a.average)
    EW_LAUNCH((k_lion_vote_apply<true, false>), C, a.stream, recv, a.nranks, a.stride, chunks,
              a.bits_off, p, sh, la, a.inv_n, key, slots);
  else
    EW_LAUNCH((k_lion_vote_apply<false, false>), C, a.stream, recv, a.nranks, a.stride, chunks,
              a.bits_off, p, sh, la, a.inv_n, key, slots);
  EW_CHECK_LAUNCH();
}
