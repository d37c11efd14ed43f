// TernGrad (Wen et al., NeurIPS 2017): stochastic ternary codes {-1, 0, +1} of a flat gradient
// bucket at 2 bits per element with one clipped fp32 scaler per tensor, and the fused decode ->
// average -> SGD on the receive side.  gfx950, wave64.  Payload (compress/plan.py `tern`):
// scales f32[T] | codes u32[D' / 16]; element i of a tensor is bits 2 (i & 15) .. + 1 of word
// code0 / 16 + (i >> 4); 0 = 0, 1 = +1, 3 = -1.
//
// Encode, three launches (the hand-offs are kernel boundaries; the sums keep one fixed order, so
// the scaler is bitwise compress/oracle.py encode_tern's):
//   stats  one block per chunk, one read: the chunk's sum of squares by ew_block_sum, the tensor's
//          largest |x| as an integer maximum, and under EF the staging of e = g + residual;
//   scale  one block per tensor: thread t adds the chunk partials t, t + 256, ... from 0, then
//          ew_block_sum; rms = sqrtf(total / n), scale = fminf(absmax, clip * rms) (clip == 0:
//          absmax); also zeroes the alignment pads of the payload;
//   quant  one block per chunk, one read: a thread quantises 4 consecutive elements into one byte
//          (ew_quantize at levels = 1) and the four lanes of a quad combine their bytes with two
//          __shfl_xor, so every store is a whole 32-bit word written by one lane: no
//          read-modify-write, no atomics on the payload, no scratch.  Codes past a tensor's end
//          inside its last word are 0.
// Decode: a thread owns 4 consecutive elements; the four lanes of a quad read the same code word
// (one 64-byte request per wave and rank serves 1024 elements).
#include "common.h"
#include "ewdml_ops.h"

namespace {

template <bool EF>
__global__ __launch_bounds__(EW_BLOCK) void k_tern_stats(GradPtrs gp, float* __restrict__ resid,
                                                         const ChunkRow* __restrict__ chunks,
                                                         float* __restrict__ chunk_sq,
                                                         uint32_t* __restrict__ maxkey) {
  __shared__ float wsf[EW_WAVES];
  const ChunkRow c = chunks[blockIdx.x];
  float sq = 0.0f;
  uint32_t km = 0;
  for (int i = 4 * threadIdx.x; i < c.len; i += 4 * EW_BLOCK) {
    float xs[4];
    ew_ld4t(gp, nullptr, c, i, xs);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i + j < c.len) {
        float x = xs[j];
        if (EF) {  // stage e = g + residual in the residual buffer
          x = x + resid[c.start + i + j];
          resid[c.start + i + j] = x;
        }
        sq = sq + x * x;
        km = max(km, ew_key(x));
      }
    }
  }
  km = ew_wave_max_u(km);
  if ((threadIdx.x & 63) == 0) atomicMax(&maxkey[c.tensor], km);
  const float s = ew_block_sum(sq, wsf);
  if (threadIdx.x == 0) chunk_sq[blockIdx.x] = s;
}

// pad_lo .. codes_off and codes_end .. nbytes are the payload's alignment pads (whole words)
__global__ __launch_bounds__(EW_BLOCK) void k_tern_scale(const TensorRow* __restrict__ tensors,
                                                         const float* __restrict__ chunk_sq,
                                                         const uint32_t* __restrict__ maxkey,
                                                         float* __restrict__ inv_out,
                                                         uint8_t* __restrict__ payload,
                                                         int scales_off, int pad_lo, int codes_off,
                                                         int codes_end, int nbytes, float clip) {
  __shared__ float wsf[EW_WAVES];
  const int t = blockIdx.x;
  const TensorRow tr = tensors[t];
  float sq = 0.0f;
  for (int j = threadIdx.x; j < tr.nchunks; j += EW_BLOCK) sq = sq + chunk_sq[tr.chunk0 + j];
  const float total = ew_block_sum(sq, wsf);
  if (threadIdx.x == 0) {
    float scale = __uint_as_float(maxkey[t]);
    if (clip > 0.0f) {
      const float rms = sqrtf(total / (float)tr.numel);
      scale = fminf(scale, clip * rms);
    }
    reinterpret_cast<float*>(payload + scales_off)[t] = scale;
    inv_out[t] = scale > 0.0f ? 1.0f / scale : 0.0f;
  }
  if (t == 0) {
    const int lo = pad_lo + 4 * (int)threadIdx.x, hi = codes_end + 4 * (int)threadIdx.x;
    if (lo < codes_off) *reinterpret_cast<uint32_t*>(payload + lo) = 0u;
    if (hi < nbytes) *reinterpret_cast<uint32_t*>(payload + hi) = 0u;
  }
}

template <bool EF>
__global__ __launch_bounds__(EW_BLOCK) void k_tern_quant(
    GradPtrs gp, float* __restrict__ resid, const ChunkRow* __restrict__ chunks,
    const TensorRow* __restrict__ tensors, const float* __restrict__ inv_arr,
    uint8_t* __restrict__ payload, int scales_off, int codes_off, uint32_t key_arg,
    const uint32_t* __restrict__ keyp, uint32_t bucket_offset) {
  const uint32_t key = keyp ? *keyp : key_arg;
  const ChunkRow c = chunks[blockIdx.x];
  const TensorRow tr = tensors[c.tensor];
  const float* flat = EF ? resid : nullptr;
  const float inv = inv_arr[c.tensor];
  // one code unit: scale * (1 / levels) at levels = 1
  const float step = reinterpret_cast<const float*>(payload + scales_off)[c.tensor];
  const uint32_t gbase = bucket_offset + (uint32_t)c.start;
  // first code word of the chunk: code0 and EW_CHUNK are multiples of 16
  uint32_t* words = reinterpret_cast<uint32_t*>(payload + codes_off) +
                    ((tr.code0 + c.local * EW_CHUNK) >> 4);
  const int sub = threadIdx.x & 3;
  // the trip count is uniform over the block: every lane takes part in the shuffles
  for (int base = 0; base < c.len; base += 4 * EW_BLOCK) {
    const int i = base + 4 * (int)threadIdx.x;
    float xs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i < c.len) ew_ld4t(gp, flat, c, i, xs);
    uint32_t b = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i + j < c.len) {
        const int q = ew_quantize(xs[j], inv, 1.0f, gbase + (uint32_t)(i + j), key);
        if (EF) resid[c.start + i + j] = xs[j] - (float)q * step;
        b |= ((uint32_t)q & 3u) << (2 * j);
      }
    }
    uint32_t w = b << (8 * sub);
    w |= (uint32_t)__shfl_xor((int)w, 1, 64);
    w |= (uint32_t)__shfl_xor((int)w, 2, 64);
    // the quad's 16 elements start at i - 4 * sub; its word exists when the first of them does
    if (sub == 0 && i < c.len) words[i >> 4] = w;
  }
}

__global__ __launch_bounds__(EW_BLOCK) void k_tern_decode_apply(
    const uint8_t* __restrict__ recv, int nranks, long long stride,
    const ChunkRow* __restrict__ chunks, const TensorRow* __restrict__ tensors, int scales_off,
    int codes_off, float* __restrict__ param, float* __restrict__ mom,
    float* __restrict__ grad_out, uint16_t* __restrict__ shadow, SgdArgs sa, int apply) {
  const ChunkRow c = chunks[blockIdx.x];
  ew_sgd_resolve(sa);
  const TensorRow tr = tensors[c.tensor];
  ew_key_advance(sa);
  const size_t word0 = (size_t)((tr.code0 + c.local * EW_CHUNK) >> 4);
  const int sh = 8 * (threadIdx.x & 3);
  float* p = param + c.start;
  float* b = mom ? mom + c.start : nullptr;
  float* go = grad_out ? grad_out + c.start : nullptr;
  for (int i = 4 * threadIdx.x; i < c.len; i += 4 * EW_BLOCK) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < nranks; ++r) {
      const uint8_t* pay = recv + r * stride;
      const float step = reinterpret_cast<const float*>(pay + scales_off)[c.tensor];
      const uint32_t w = reinterpret_cast<const uint32_t*>(pay + codes_off)[word0 + (i >> 4)] >> sh;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = (int)(((w >> (2 * j)) & 3u) ^ 2u) - 2;  // 2-bit two's complement
        const float prod = (float)q * step;
        acc[j] = acc[j] + prod;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i + j < c.len) {
        const float gv = acc[j] * sa.grad_scale;
        if (go) go[i + j] = gv;
        if (apply) {
          float pv = p[i + j], bv = b ? b[i + j] : 0.0f;
          ew_sgd(pv, bv, gv, sa);
          p[i + j] = pv;
          if (b) b[i + j] = bv;
          if (shadow) shadow[c.start + i + j] = ew_f2bf(pv);
        }
      }
    }
  }
}

}  // namespace

#define EW_LAUNCH(kern, grid, stream, ...) \
  hipLaunchKernelGGL(kern, dim3(grid), dim3(EW_BLOCK), 0, (hipStream_t)(stream), __VA_ARGS__)

// scales f32[T] | codes u32[total_codes / 16] must lie inside `bytes`
static void ew_tern_fit(const std::string& who, int T, int C, int scales_off, int codes_off,
                        long long total_codes, long long bytes) {
  if (T <= 0 || C <= 0 || T > EW_MAX_T)
    throw std::runtime_error(who + ": empty or oversized bucket");
  if (total_codes <= 0 || total_codes % 16 || total_codes > 0x7fffffffLL)
    throw std::runtime_error(who + ": the code count must be a positive multiple of 16");
  if (scales_off < 0 || scales_off % 16 || codes_off % 16 || codes_off < scales_off + 4 * T ||
      bytes % 4 || bytes < codes_off + total_codes / 4 || bytes > 0x7fffffffLL)
    throw std::runtime_error(who + ": payload sections do not fit the payload");
}

void ew_tern_encode(const TernEncodeArgs& a) {
  const int T = a.num_tensors, C = a.num_chunks;
  ew_tern_fit("ewdml tern", T, C, a.scales_off, a.codes_off, a.total_codes, a.payload_bytes);
  if (!a.chunks || !a.tensors || !a.scratch || !a.payload)
    throw std::runtime_error("ewdml tern: missing table");
  if ((a.payload | a.resid) % 16 || (a.chunks | a.tensors | a.scratch | a.key_ptr) % 4)
    throw std::runtime_error("ewdml tern: misaligned operand");
  if (!(a.clip >= 0.0f)) throw std::runtime_error("ewdml tern: clip must be >= 0");
  const int pad_lo = a.scales_off + 4 * T, codes_end = a.codes_off + (int)(a.total_codes / 4);
  if (a.codes_off - pad_lo > 4 * EW_BLOCK || a.payload_bytes - codes_end > 4 * EW_BLOCK)
    throw std::runtime_error("ewdml tern: alignment pads larger than one block writes");
  auto* chunks = reinterpret_cast<const ChunkRow*>(a.chunks);
  auto* tensors = reinterpret_cast<const TensorRow*>(a.tensors);
  // scratch (ew_qsgd_scratch_bytes): maxkey[T] | chunk_sq[C] | inv[T]
  uint32_t* maxkey = reinterpret_cast<uint32_t*>(a.scratch);
  float* chunk_sq = reinterpret_cast<float*>(maxkey + T);
  float* inv = chunk_sq + C;
  hipStream_t s = (hipStream_t)a.stream;
  EW_CHECK(hipMemsetAsync(reinterpret_cast<void*>(a.scratch), 0, ew_qsgd_scratch_bytes(T, C), s));
  GradPtrs g;
  ew_fill_ptrs(g, a.src, T);
  float* resid = reinterpret_cast<float*>(a.resid);
  auto* pay = reinterpret_cast<uint8_t*>(a.payload);
  auto* keyp = reinterpret_cast<const uint32_t*>(a.key_ptr);
  if (resid)
    EW_LAUNCH(k_tern_stats<true>, C, s, g, resid, chunks, chunk_sq, maxkey);
  else
    EW_LAUNCH(k_tern_stats<false>, C, s, g, resid, chunks, chunk_sq, maxkey);
  EW_LAUNCH(k_tern_scale, T, s, tensors, chunk_sq, maxkey, inv, pay, a.scales_off, pad_lo,
            a.codes_off, codes_end, (int)a.payload_bytes, a.clip);
  if (resid)
    EW_LAUNCH(k_tern_quant<true>, C, s, g, resid, chunks, tensors, inv, pay, a.scales_off,
              a.codes_off, a.key, keyp, a.bucket_offset);
  else
    EW_LAUNCH(k_tern_quant<false>, C, s, g, resid, chunks, tensors, inv, pay, a.scales_off,
              a.codes_off, a.key, keyp, a.bucket_offset);
  EW_CHECK_LAUNCH();
}

void ew_tern_decode_apply(const TernDecodeArgs& a) {
  if (a.nranks <= 0 || a.nranks > EW_MAX_RANKS)
    throw std::runtime_error("ewdml tern decode: nothing to decode, or too many ranks");
  ew_tern_fit("ewdml tern decode", a.num_tensors, a.num_chunks, a.scales_off, a.codes_off,
              a.total_codes, a.stride);
  if (!a.recv || !a.chunks || !a.tensors)
    throw std::runtime_error("ewdml tern decode: missing table");
  const StepArgs& st = a.step;
  ew_step_check("ewdml tern decode", st, false);
  if (a.recv % 16 || (a.chunks | a.tensors) % 4)
    throw std::runtime_error("ewdml tern decode: misaligned operand");
  EW_LAUNCH(k_tern_decode_apply, a.num_chunks, a.stream, reinterpret_cast<const uint8_t*>(a.recv),
            a.nranks, a.stride, reinterpret_cast<const ChunkRow*>(a.chunks),
            reinterpret_cast<const TensorRow*>(a.tensors), a.scales_off, a.codes_off,
            reinterpret_cast<float*>(st.param), reinterpret_cast<float*>(st.mom),
            reinterpret_cast<float*>(st.grad_out), reinterpret_cast<uint16_t*>(st.shadow),
            ew_sgd_args(st), st.apply);
  EW_CHECK_LAUNCH();
}
