// Threshold-search sparsification of a flat gradient bucket (RedSync's threshold binary search,
// Fang et al. 2019; MSTopK, Shi et al. 2021; hard-threshold sparsification under error feedback,
// Sahu et al. 2021), and the fused decode -> rank-ordered sum -> SGD on the receive side.  gfx950,
// wave64.
//
// Every chunk row is independent: one block loads its 8192 elements into registers, forms acc = g +
// residual, finds the chunk's threshold there and writes the entries at or above it, in index
// order, into slots the chunk owns.  One launch per bucket; no cross-block hand-off, no grid
// barrier, no look-back, no scratch buffer, no atomics, no RNG.
//
// Payload (compress/plan.py, kind "thresh"): counts u16[C] | idx u16[S] | values f32[S].  Chunk c
// owns the slots [slot0_c, slot0_c + cap_c) (the `slots` table, int2 {cap, slot0} per chunk row);
// its first counts[c] slots hold the sent entries, the rest index 0 and value +0.0.  Every byte is
// written by every encode, the alignment pads (each under 16 bytes) by block 0.
//
// Threshold (compress/oracle.py thresh_threshold, bit for bit): lev = (bits(acc) & 0x7fffffff) >>
// 16, the bf16 truncation of |acc|; J = the smallest integer in [0, 32768] with #{lev >= J} <= cap.
// J is canonical, so how it is searched cannot change the payload: the search starts at the J the
// chunk had last step (`state`, a warm start only), gallops away from it while it is on the wrong
// side -- two candidates per counting pass, 1, 2, 4, 8, ... levels apart -- and trisects once J is
// bracketed.  A cold start takes at most 20 passes; the loop bound is THR_PASSES.
//
// A counting pass: every thread counts its 32 levels (kept biased by one, 0 = past the chunk's end,
// two to a register) against both candidates into one word, a wave shuffle tree, then the four
// waves' partials through LDS (two buffers, so a pass costs one barrier).  The compaction takes a
// ballot per element position: the sent elements of lower lanes are a masked bit count, the waves'
// totals per slab go through LDS, and the entries leave in index order.
#include "common.h"
#include "ewdml_ops.h"

#include <vector>

namespace {

#define THR_MAXJ 32768
#define THR_PASSES 32

__device__ __forceinline__ uint32_t thr_lev1(float x, bool valid) {
  return valid ? ((__float_as_uint(x) & 0x7fffffffu) >> 16) + 1u : 0u;
}

// #{lev1 >= ta} | #{lev1 >= tb} << 16 over the thread's 32 elements
__device__ __forceinline__ uint32_t thr_count2(const uint32_t (&L)[2 * EW_CU], uint32_t ta,
                                               uint32_t tb) {
  uint32_t na = 0, nb = 0;
#pragma unroll
  for (int k = 0; k < 2 * EW_CU; ++k) {
    const uint32_t lo = L[k] & 0xffffu, hi = L[k] >> 16;
    na += (uint32_t)(lo >= ta) + (uint32_t)(hi >= ta);
    nb += (uint32_t)(lo >= tb) + (uint32_t)(hi >= tb);
  }
  return na | (nb << 16);
}

// the block's sum in every thread; ws: EW_WAVES words nobody has written since the barrier before
// the last
__device__ __forceinline__ uint32_t thr_block_sum(uint32_t v, uint32_t* ws) {
  v = ew_wave_sum_u(v);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < EW_WAVES; ++i) s += ws[i];
  return s;
}

__device__ __forceinline__ uint32_t thr_below(unsigned long long m) {  // set bits of lower lanes
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the capacity of a chunk row cut to what the sections hold (a table that does not fit its payload
// writes and reads nothing)
__device__ __forceinline__ int thr_cap(const int2 sl, int S) {
  return (sl.y < 0 || sl.y > S) ? 0 : min(sl.x, S - sl.y);
}

template <bool EF>
__global__ __launch_bounds__(EW_BLOCK) void k_thr_encode(
    GradPtrs gp, float* __restrict__ resid, const ChunkRow* __restrict__ chunks,
    const int2* __restrict__ slots, uint8_t* __restrict__ payload, int counts_off, int idx_off,
    int vals_off, int S, int nbytes, int* __restrict__ state, int* __restrict__ dbg_passes) {
  __shared__ uint32_t ws[2][EW_WAVES];
  __shared__ uint32_t wtot[EW_CU][EW_WAVES];
  const ChunkRow c = chunks[blockIdx.x];
  const int2 sl = slots[blockIdx.x];
  const int cap = thr_cap(sl, S);
  float4 e[EW_CU];
  ew_ld_chunk(gp, nullptr, c, e);  // positions past c.len read as 0 and get level 0: never sent
  if (EF) {
    float4 r[EW_CU];
    ew_ld_chunk(gp, resid, c, r);
#pragma unroll
    for (int u = 0; u < EW_CU; ++u)
      e[u] = make_float4(e[u].x + r[u].x, e[u].y + r[u].y, e[u].z + r[u].z, e[u].w + r[u].w);
  }
  uint32_t L[2 * EW_CU];
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    L[2 * u] = thr_lev1(e[u].x, i < c.len) | (thr_lev1(e[u].y, i + 1 < c.len) << 16);
    L[2 * u + 1] = thr_lev1(e[u].z, i + 2 < c.len) | (thr_lev1(e[u].w, i + 3 < c.len) << 16);
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) {  // the three alignment pads: payloads compare bytewise
    uint16_t* p16 = reinterpret_cast<uint16_t*>(payload);
    const int a0 = counts_off + 2 * (int)gridDim.x + 2 * (int)threadIdx.x;
    const int a1 = idx_off + 2 * S + 2 * (int)threadIdx.x;
    const int a2 = vals_off + 4 * S + 2 * (int)threadIdx.x;
    if (a0 < idx_off) p16[a0 >> 1] = 0;
    if (a1 < vals_off) p16[a1 >> 1] = 0;
    if (a2 < nbytes) p16[a2 >> 1] = 0;
  }

  // f(J) = #{lev >= J} <= cap is monotone; f(lo) is false (lo = -1: nothing known), f(hi) true
  int lo = -1, hi = THR_MAXJ;
  int prev = state ? state[blockIdx.x] : 0;
  prev = min(max(prev, 0), THR_MAXJ);
  int dir = 0, step = 1, passes = 0;  // dir 0: the first pass, +-1: galloping, 2: bracketed
  for (int k = 0; k < THR_PASSES && hi - lo > 1; ++k) {
    int c1, c2;
    if (dir == 0) {
      c1 = prev - 1;
      c2 = prev;
    } else if (dir == 1) {
      c1 = lo + step;
      c2 = lo + 3 * step;
    } else if (dir == -1) {
      c1 = hi - 3 * step;
      c2 = hi - step;
    } else {
      const int d = hi - lo;
      c1 = lo + d / 3;
      c2 = lo + (2 * d) / 3;
    }
    c1 = min(max(c1, lo + 1), hi - 1);
    c2 = min(max(c2, lo + 1), hi - 1);
    const uint32_t n = thr_block_sum(thr_count2(L, (uint32_t)c1 + 1u, (uint32_t)c2 + 1u), ws[k & 1]);
    const bool t1 = (int)(n & 0xffffu) <= cap, t2 = (int)(n >> 16) <= cap;  // t1 implies t2
    if (dir == 0) {
      dir = !t2 ? 1 : (t1 ? -1 : 2);
    } else if (dir == 1) {
      if (t2) dir = 2; else step *= 4;
    } else if (dir == -1) {
      if (!t1) dir = 2; else step *= 4;
    }
    lo = t2 ? (t1 ? lo : c1) : c2;
    hi = t1 ? c1 : (t2 ? c2 : hi);
    ++passes;
  }

  // ordered compaction: element u * 1024 + 4 t + j goes after every sent element of the slabs
  // below u, of the waves below this one in slab u, and of the lower lanes and js in this wave
  const uint32_t T = (uint32_t)hi + 1u;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t below[EW_CU], flags = 0;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const uint32_t f0 = (L[2 * u] & 0xffffu) >= T, f1 = (L[2 * u] >> 16) >= T;
    const uint32_t f2 = (L[2 * u + 1] & 0xffffu) >= T, f3 = (L[2 * u + 1] >> 16) >= T;
    const unsigned long long m0 = __ballot(f0), m1 = __ballot(f1), m2 = __ballot(f2),
                             m3 = __ballot(f3);
    below[u] = thr_below(m0) + thr_below(m1) + thr_below(m2) + thr_below(m3);
    if (lane == 0) wtot[u][w] = __popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3);
    flags |= (f0 | (f1 << 1) | (f2 << 2) | (f3 << 3)) << (4 * u);
  }
  __syncthreads();
  uint32_t run = 0, base[EW_CU];
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    base[u] = 0;
#pragma unroll
    for (int ww = 0; ww < EW_WAVES; ++ww) {
      base[u] = (ww == w) ? run : base[u];
      run += wtot[u][ww];
    }
  }
  const int total = min((int)run, cap);  // run <= cap by the choice of J

  uint16_t* idxs = reinterpret_cast<uint16_t*>(payload + idx_off) + sl.y;
  float* vals = reinterpret_cast<float*>(payload + vals_off) + sl.y;
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const int i = ew_chunk_idx(u);
    int pos = (int)(base[u] + below[u]);
    const uint32_t f = flags >> (4 * u);
    if (f & 1u) {
      if (pos < cap) { idxs[pos] = (uint16_t)i; vals[pos] = e[u].x; }
      ++pos;
      e[u].x = 0.0f;
    }
    if (f & 2u) {
      if (pos < cap) { idxs[pos] = (uint16_t)(i + 1); vals[pos] = e[u].y; }
      ++pos;
      e[u].y = 0.0f;
    }
    if (f & 4u) {
      if (pos < cap) { idxs[pos] = (uint16_t)(i + 2); vals[pos] = e[u].z; }
      ++pos;
      e[u].z = 0.0f;
    }
    if (f & 8u) {
      if (pos < cap) { idxs[pos] = (uint16_t)(i + 3); vals[pos] = e[u].w; }
      e[u].w = 0.0f;
    }
  }
  for (int s = total + (int)threadIdx.x; s < cap; s += EW_BLOCK) {  // the slots not used
    idxs[s] = 0;
    vals[s] = 0.0f;
  }
  if (threadIdx.x == 0) {
    reinterpret_cast<uint16_t*>(payload + counts_off)[blockIdx.x] = (uint16_t)total;
    if (state) state[blockIdx.x] = hi;
    if (dbg_passes) dbg_passes[blockIdx.x] = passes;
  }
  if (EF) ew_st_chunk(resid + c.start, c.len, e);
}

// One block per chunk row: a 32 KiB fp32 tile of the chunk in LDS, zeroed; the ranks' entries are
// added in rank order with a barrier between ranks (an index appears once per row, so an element's
// order is the rank order); then the tail every fused decode has.  A count is cut to the chunk's
// capacity and an index at or past the chunk's length is dropped (compress/oracle.py
// _thresh_entries): a corrupt row cannot reach outside the tile.
__global__ __launch_bounds__(EW_BLOCK) void k_thr_decode_apply(
    const uint8_t* __restrict__ recv, int nranks, long long stride,
    const ChunkRow* __restrict__ chunks, const int2* __restrict__ slots, int counts_off,
    int idx_off, int vals_off, int S, float* __restrict__ param, float* __restrict__ mom,
    float* __restrict__ grad_out, uint16_t* __restrict__ shadow, SgdArgs sa, int apply) {
  __shared__ float4 tile4[EW_CHUNK / 4];
  float* tile = reinterpret_cast<float*>(tile4);
  const ChunkRow c = chunks[blockIdx.x];
  ew_sgd_resolve(sa);
  ew_key_advance(sa);
  const int2 sl = slots[blockIdx.x];
  const int cap = thr_cap(sl, S);
#pragma unroll
  for (int u = 0; u < EW_CU; ++u)
    tile4[u * EW_BLOCK + threadIdx.x] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  __syncthreads();
  for (int r = 0; r < nranks; ++r) {
    const uint8_t* pay = recv + r * stride;
    const int cnt = min((int)reinterpret_cast<const uint16_t*>(pay + counts_off)[blockIdx.x], cap);
    const uint16_t* idxs = reinterpret_cast<const uint16_t*>(pay + idx_off) + sl.y;
    const float* vals = reinterpret_cast<const float*>(pay + vals_off) + sl.y;
    for (int s = threadIdx.x; s < cnt; s += EW_BLOCK) {
      const int i = idxs[s];
      const float v = vals[s];
      if (i < c.len) tile[i] = tile[i] + v;
    }
    __syncthreads();
  }
  float acc[EW_CU][4];
#pragma unroll
  for (int u = 0; u < EW_CU; ++u) {
    const float4 v = tile4[u * EW_BLOCK + threadIdx.x];  // elements ew_chunk_idx(u) .. + 3
    acc[u][0] = v.x; acc[u][1] = v.y; acc[u][2] = v.z; acc[u][3] = v.w;
  }
  ew_chunk_apply(acc, c, param, mom, grad_out, shadow, sa, apply);
}

}  // namespace

#define EW_LAUNCH(kern, grid, stream, ...) \
  hipLaunchKernelGGL(kern, dim3(grid), dim3(EW_BLOCK), 0, (hipStream_t)(stream), __VA_ARGS__)

// counts u16[C] | idx u16[S] | values f32[S], every section 16-byte aligned and every pad under 16
// bytes, must make up `bytes`
static void ew_thresh_fit(const std::string& who, int C, long long S, int counts_off, int idx_off,
                          int vals_off, long long bytes) {
  if (C <= 0 || S <= 0 || S > 0x3fffffffLL) throw std::runtime_error(who + ": empty bucket");
  const long long e0 = counts_off + 2LL * C, e1 = idx_off + 2 * S, e2 = vals_off + 4 * S;
  if (counts_off < 0 || counts_off % 16 || idx_off % 16 || vals_off % 16 || idx_off < e0 ||
      idx_off - e0 >= 16 || vals_off < e1 || vals_off - e1 >= 16 || bytes < e2 || bytes - e2 >= 16 ||
      bytes > 0x7fffffffLL)
    throw std::runtime_error(who + ": payload sections do not fit the payload");
}

void ew_thresh_encode(const ThreshEncodeArgs& a) {
  const int C = a.num_chunks;
  ew_thresh_fit("ewdml thresh", C, a.total_slots, a.counts_off, a.idx_off, a.codes_off,
                a.payload_bytes);
  if (!a.chunks || !a.slots || !a.payload) throw std::runtime_error("ewdml thresh: missing table");
  if ((a.payload | a.resid) % 16 || (a.chunks | a.state | a.dbg_passes) % 4 || a.slots % 8)
    throw std::runtime_error("ewdml thresh: misaligned operand");
  GradPtrs g;
  ew_fill_ptrs(g, a.src, a.num_tensors);
  float* resid = reinterpret_cast<float*>(a.resid);
  auto* chunks = reinterpret_cast<const ChunkRow*>(a.chunks);
  auto* slots = reinterpret_cast<const int2*>(a.slots);
  auto* pay = reinterpret_cast<uint8_t*>(a.payload);
  int* state = reinterpret_cast<int*>(a.state);
  int* dbg = reinterpret_cast<int*>(a.dbg_passes);
  if (resid)
    EW_LAUNCH(k_thr_encode<true>, C, a.stream, g, resid, chunks, slots, pay, a.counts_off,
              a.idx_off, a.codes_off, (int)a.total_slots, (int)a.payload_bytes, state, dbg);
  else
    EW_LAUNCH(k_thr_encode<false>, C, a.stream, g, resid, chunks, slots, pay, a.counts_off,
              a.idx_off, a.codes_off, (int)a.total_slots, (int)a.payload_bytes, state, dbg);
  EW_CHECK_LAUNCH();
}

void ew_thresh_decode_apply(const ThreshDecodeArgs& a) {
  const int C = a.num_chunks;
  if (a.nranks <= 0 || a.nranks > EW_MAX_RANKS)
    throw std::runtime_error("ewdml thresh decode: nothing to decode, or too many ranks");
  ew_thresh_fit("ewdml thresh decode", C, a.total_slots, a.counts_off, a.idx_off, a.codes_off,
                a.stride);
  if (!a.recv || !a.chunks || !a.slots)
    throw std::runtime_error("ewdml thresh decode: missing table");
  if (a.recv % 16 || a.stride % 16 || a.chunks % 4 || a.slots % 8)
    throw std::runtime_error("ewdml thresh decode: misaligned operand");
  const StepArgs& st = a.step;
  ew_step_check("ewdml thresh decode", st, false);
  const SgdArgs sa = ew_sgd_args(st);
  EW_LAUNCH(k_thr_decode_apply, C, a.stream, reinterpret_cast<const uint8_t*>(a.recv), a.nranks,
            a.stride, reinterpret_cast<const ChunkRow*>(a.chunks),
            reinterpret_cast<const int2*>(a.slots), a.counts_off, a.idx_off, a.codes_off,
            (int)a.total_slots, reinterpret_cast<float*>(st.param),
            reinterpret_cast<float*>(st.mom), reinterpret_cast<float*>(st.grad_out),
            reinterpret_cast<uint16_t*>(st.shadow), sa, st.apply);
  EW_CHECK_LAUNCH();
}

// the loaded code objects' resources: {registers, scratch bytes per thread, static LDS bytes} of
// k_thr_encode<true>, k_thr_encode<false> and k_thr_decode_apply
std::vector<int> ew_thresh_kernel_info() {
  std::vector<int> out;
  const void* fns[3] = {reinterpret_cast<const void*>(&k_thr_encode<true>),
                        reinterpret_cast<const void*>(&k_thr_encode<false>),
                        reinterpret_cast<const void*>(&k_thr_decode_apply)};
  for (const void* f : fns) {
    hipFuncAttributes at;
    EW_CHECK(hipFuncGetAttributes(&at, f));
    out.push_back(at.numRegs);
    out.push_back((int)at.localSizeBytes);
    out.push_back((int)at.sharedSizeBytes);
  }
  return out;
}
