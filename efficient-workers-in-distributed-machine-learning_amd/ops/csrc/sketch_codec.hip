// Count-sketch gradient exchange (SketchedSGD, Ivkin et al., NeurIPS 2019): the kernels around the
// two all-reduces of parallel/sketch.py.  compress/oracle.py (sketch_*) defines every result bit
// for bit; compress/plan.py SketchPlan holds the tables.
//
//   k_sketch_stage     resid <- g + resid on the sketched chunk rows (the error-compensated
//                      gradient `acc` lives in the residual from here on)
//   k_sketch_accum     the table T[R][W]: T[j][b] = sum of sign * acc over the chunks whose rotated
//                      image covers column b
//   k_sketch_estimate  est[i] = median over the rows of sign_j(i) * T[j][column_j(i)]
//   k_sketch_gather    walks the index sections of the `topk` payload that the top-k encode wrote
//                      for est (the selection), overwrites its values with acc at the selected
//                      coordinates (g on dense tensors) and clears the residual there
//
// The hash is a rotation per (row, chunk): chunk c's element p lands in column (p + o[j][c]) mod W,
// W a multiple of EW_CHUNK, so a chunk's image is one run of columns (with at most one wrap) and a
// column receives at most one element of a chunk.  That makes the table a gather: the block that
// owns (row j, a tile of SK_TILE columns) walks the chunks in ascending order, skips (wave-uniform
// test) those whose image misses its tile, and adds the one element of each remaining chunk that
// falls on each of its columns -- no atomics, no partial tables, one order.  The order is the
// oracle's: within a group of SK_GROUP consecutive chunk indices sequential fp32 adds from +0.0 in
// ascending chunk order, then the group partials in ascending group order from +0.0 (a chunk that
// does not cover a column adds nothing, which is bitwise adding +0.0).
//
// The sign of element i in row j is bit j of ew_mix32(gidx ^ sg_key), gidx the element's index in
// the flat buffer, applied by xor on the sign bit: no arithmetic, so -0.0, infinities and NaNs
// follow the oracle's torch.where(bit, -x, x).
#include "common.h"

namespace {

constexpr int SK_TILE = 1024;  // columns per accumulate block: 4 per thread, EW_BLOCK apart
constexpr int SK_COLS = SK_TILE / EW_BLOCK;
constexpr int SK_GROUP = 64;   // compress/plan.py SKETCH_SUM_GROUP
constexpr int SK_MAX_ROWS = 5;

struct SkRow {  // mirrors SketchPlan.row_table()
  int start, len;
};

__device__ __forceinline__ float sk_flip(float x, uint32_t h, int j) {
  return __uint_as_float(__float_as_uint(x) ^ (((h >> j) & 1u) << 31));
}

// compare-exchange of the median networks: a select on one ordered compare, as the oracle's
// torch.where(b < a, ...): equal values (+0.0 / -0.0) and NaNs stay where they are
#define SK_CX(a, b)            \
  do {                         \
    const bool s_ = (b) < (a); \
    const float lo_ = s_ ? (b) : (a), hi_ = s_ ? (a) : (b); \
    (a) = lo_;                 \
    (b) = hi_;                 \
  } while (0)

template <int R>
__device__ __forceinline__ float sk_median(float (&v)[R]) {
  if constexpr (R == 3) {
    SK_CX(v[0], v[1]);
    SK_CX(v[1], v[2]);
    SK_CX(v[0], v[1]);
  } else if constexpr (R == 5) {  // a 9-comparator sorting network of five values
    SK_CX(v[0], v[1]);
    SK_CX(v[3], v[4]);
    SK_CX(v[2], v[4]);
    SK_CX(v[2], v[3]);
    SK_CX(v[1], v[4]);
    SK_CX(v[0], v[3]);
    SK_CX(v[0], v[2]);
    SK_CX(v[1], v[3]);
    SK_CX(v[1], v[2]);
  }
  return v[R / 2];
}

__global__ __launch_bounds__(EW_BLOCK) void k_sketch_stage(const float* __restrict__ g,
                                                           float* __restrict__ resid,
                                                           const SkRow* __restrict__ rows) {
  const SkRow r = rows[blockIdx.x];
  if (r.len == 0) return;  // a dense tensor keeps no residual
  const float* gs = g + r.start;
  float* rs = resid + r.start;
  // 16-byte accesses and a scalar tail: the bucket views are 16-byte aligned and every chunk row
  // starts at a multiple of 4 elements (ops.SketchTables checks both)
  const int n4 = r.len >> 2;
  for (int i = threadIdx.x; i < n4; i += EW_BLOCK) {
    const float4 a = reinterpret_cast<const float4*>(gs)[i];
    float4 b = reinterpret_cast<const float4*>(rs)[i];
    b.x = a.x + b.x;
    b.y = a.y + b.y;
    b.z = a.z + b.z;
    b.w = a.w + b.w;
    reinterpret_cast<float4*>(rs)[i] = b;
  }
  for (int i = (n4 << 2) + threadIdx.x; i < r.len; i += EW_BLOCK) rs[i] = gs[i] + rs[i];
}

// grid (W / SK_TILE, R).  `acc` is the staged residual; rows / shifts are read at wave-uniform
// addresses (scalar loads), the elements at consecutive addresses across the lanes.
__global__ __launch_bounds__(EW_BLOCK) void k_sketch_accum(const float* __restrict__ acc,
                                                           const SkRow* __restrict__ rows,
                                                           const int* __restrict__ shifts, int C,
                                                           int W, uint32_t sg_key, uint32_t boff,
                                                           float* __restrict__ table) {
  const int j = blockIdx.y, t0 = blockIdx.x * SK_TILE;
  const int* sh = shifts + (size_t)j * C;
  float total[SK_COLS];
#pragma unroll
  for (int u = 0; u < SK_COLS; ++u) total[u] = 0.0f;
  for (int g0 = 0; g0 < C; g0 += SK_GROUP) {
    float part[SK_COLS];
#pragma unroll
    for (int u = 0; u < SK_COLS; ++u) part[u] = 0.0f;
    const int g1 = min(g0 + SK_GROUP, C);
    for (int c = g0; c < g1; ++c) {
      const SkRow r = rows[c];
      if (r.len == 0) continue;
      const int o = sh[c];
      int d = t0 - o;  // where the tile's first column falls in the chunk's image
      if (d < 0) d += W;
      // the image [o, o + len) mod W meets the tile iff the tile starts inside it or it starts
      // inside the tile
      if (!(d < r.len || W - d < SK_TILE)) continue;
#pragma unroll
      for (int u = 0; u < SK_COLS; ++u) {
        int p = t0 + (int)threadIdx.x + u * EW_BLOCK - o;
        if (p < 0) p += W;
        if (p < r.len) {
          const uint32_t h = ew_mix32((boff + (uint32_t)(r.start + p)) ^ sg_key);
          part[u] = part[u] + sk_flip(acc[r.start + p], h, j);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < SK_COLS; ++u) total[u] = total[u] + part[u];
  }
#pragma unroll
  for (int u = 0; u < SK_COLS; ++u)
    table[(size_t)j * W + t0 + threadIdx.x + u * EW_BLOCK] = total[u];
}

// one block per chunk row; the R table reads of consecutive elements are consecutive columns
// (one wrap per row at most)
template <int R>
__global__ __launch_bounds__(EW_BLOCK) void k_sketch_estimate(const float* __restrict__ table,
                                                              const SkRow* __restrict__ rows,
                                                              const int* __restrict__ shifts, int C,
                                                              int W, uint32_t sg_key, uint32_t boff,
                                                              float* __restrict__ est) {
  const int c = blockIdx.x;
  const SkRow r = rows[c];
  if (r.len == 0) return;  // dense tensors: est stays 0
  int o[R];
#pragma unroll
  for (int j = 0; j < R; ++j) o[j] = shifts[(size_t)j * C + c];
  for (int p = threadIdx.x; p < r.len; p += EW_BLOCK) {
    const uint32_t h = ew_mix32((boff + (uint32_t)(r.start + p)) ^ sg_key);
    float v[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      int col = p + o[j];
      if (col >= W) col -= W;
      v[j] = sk_flip(table[(size_t)j * W + col], h, j);
    }
    est[r.start + p] = sk_median<R>(v);
  }
}

// one block per chunk of the bucket's top-k plan (dense tensors included).  The entries of a chunk
// start at entry0 + the counts of the tensor's earlier chunks (k_topk_decode_sparse's walk).
__global__ __launch_bounds__(EW_BLOCK) void k_sketch_gather(
    const float* __restrict__ g, float* __restrict__ resid, const ChunkRow* __restrict__ chunks,
    const TensorRow* __restrict__ tensors, uint8_t* __restrict__ pay, int counts_off, int idx_off,
    int codes_off, int bitmap_off) {
  __shared__ uint32_t ws[EW_WAVES];
  const ChunkRow c = chunks[blockIdx.x];
  const TensorRow tr = tensors[c.tensor];
  const uint16_t* counts = reinterpret_cast<const uint16_t*>(pay + counts_off) + tr.chunk0;
  uint32_t s = 0;
  for (int q = threadIdx.x; q < c.local; q += EW_BLOCK) s += counts[q];
  uint32_t before;
  ew_block_excl_scan(s, ws, before);
  const uint32_t off = (uint32_t)tr.entry0 + before;
  const uint32_t cnt = counts[c.local];
  const uint32_t eend = (uint32_t)(tr.entry0 + tr.k);  // never past the tensor's entries
  const bool dense = tr.k == tr.numel;
  const float* src = dense ? g : resid;
  float* vals = reinterpret_cast<float*>(pay + codes_off);
  if (tr.bm0 < 0) {
    const uint16_t* idx = reinterpret_cast<const uint16_t*>(pay + idx_off) + tr.idx0 +
                          (off - (uint32_t)tr.entry0);
    for (uint32_t e = threadIdx.x; e < cnt && off + e < eend; e += EW_BLOCK) {
      const int i = idx[e];
      if (i < c.len) {
        vals[off + e] = src[c.start + i];
        if (!dense) resid[c.start + i] = 0.0f;
      }
    }
  } else {
    // bitmap: thread t owns word t (elements 32 t .. 32 t + 31) of the chunk
    const uint32_t* bw = reinterpret_cast<const uint32_t*>(pay + bitmap_off) + tr.bm0 +
                         c.local * EW_BM_WORDS;
    uint32_t word = (int)threadIdx.x * 32 < c.len ? bw[threadIdx.x] : 0u;
    uint32_t tot;
    uint32_t e = ew_block_excl_scan((uint32_t)__popc(word), ws, tot);
    while (word) {
      const int b = __ffs(word) - 1;
      word &= word - 1u;
      const int i = (int)threadIdx.x * 32 + b;
      if (e < cnt && off + e < eend && i < c.len) {
        vals[off + e] = src[c.start + i];
        if (!dense) resid[c.start + i] = 0.0f;
      }
      ++e;
    }
  }
}

}  // namespace

#define EW_LAUNCH(kern, grid, stream, ...) \
  hipLaunchKernelGGL(kern, dim3(grid), dim3(EW_BLOCK), 0, (hipStream_t)(stream), __VA_ARGS__)

int ew_sketch_sum_group() { return SK_GROUP; }

// the tables every launch reads (their contents are checked against the buffers where they are
// built: ops.SketchTables)
static void ew_sketch_check(const std::string& who, const SketchArgs& a) {
  if (!a.rows || !a.shifts || a.num_chunks <= 0) throw std::runtime_error(who + ": missing table");
  if (a.sketch_rows != 1 && a.sketch_rows != 3 && a.sketch_rows != 5)
    throw std::runtime_error(who + ": 1, 3 or 5 rows");
  if (a.width < EW_CHUNK || a.width % EW_CHUNK || a.sketch_rows * a.width >= (1LL << 31))
    throw std::runtime_error(who + ": the width is a multiple of the chunk below 2^31 / rows");
  if (a.bucket_len <= 0 || a.bucket_len >= (1LL << 31))
    throw std::runtime_error(who + ": bucket length missing");
  if ((a.rows | a.shifts) % 4 || (a.grad | a.resid | a.table | a.est) % 16)
    throw std::runtime_error(who + ": misaligned operand");
}

void ew_sketch_stage(const SketchArgs& a) {
  ew_sketch_check("ewdml sketch stage", a);
  if (!a.grad || !a.resid) throw std::runtime_error("ewdml sketch stage: missing operand");
  EW_LAUNCH(k_sketch_stage, a.num_chunks, a.stream, reinterpret_cast<const float*>(a.grad),
            reinterpret_cast<float*>(a.resid), reinterpret_cast<const SkRow*>(a.rows));
  EW_CHECK_LAUNCH();
}

void ew_sketch_accum(const SketchArgs& a) {
  ew_sketch_check("ewdml sketch accumulate", a);
  if (!a.resid || !a.table) throw std::runtime_error("ewdml sketch accumulate: missing operand");
  hipLaunchKernelGGL(k_sketch_accum, dim3((unsigned)(a.width / SK_TILE), a.sketch_rows),
                     dim3(EW_BLOCK), 0, (hipStream_t)a.stream,
                     reinterpret_cast<const float*>(a.resid),
                     reinterpret_cast<const SkRow*>(a.rows),
                     reinterpret_cast<const int*>(a.shifts), a.num_chunks, (int)a.width, a.sg_key,
                     a.bucket_offset, reinterpret_cast<float*>(a.table));
  EW_CHECK_LAUNCH();
}

void ew_sketch_estimate(const SketchArgs& a) {
  ew_sketch_check("ewdml sketch estimate", a);
  if (!a.table || !a.est) throw std::runtime_error("ewdml sketch estimate: missing operand");
#define EW_SK_EST(R)                                                                            \
  EW_LAUNCH(k_sketch_estimate<R>, a.num_chunks, a.stream, reinterpret_cast<const float*>(a.table), \
            reinterpret_cast<const SkRow*>(a.rows), reinterpret_cast<const int*>(a.shifts),     \
            a.num_chunks, (int)a.width, a.sg_key, a.bucket_offset,                              \
            reinterpret_cast<float*>(a.est))
  if (a.sketch_rows == 1) EW_SK_EST(1);
  else if (a.sketch_rows == 3) EW_SK_EST(3);
  else EW_SK_EST(5);
#undef EW_SK_EST
  EW_CHECK_LAUNCH();
}

void ew_sketch_gather(const SketchArgs& a) {
  ew_sketch_check("ewdml sketch gather", a);
  if (!a.grad || !a.resid || !a.chunks || !a.tensors || !a.payload)
    throw std::runtime_error("ewdml sketch gather: missing operand");
  if (a.num_tensors <= 0 || a.num_tensors > EW_MAX_T)
    throw std::runtime_error("ewdml sketch gather: tensor count");
  // counts u16[C] | idx u16[total_idx] | bitmap u32[total_bm_words] | values f32[total_k]
  if (a.counts_off < 0 || a.idx_off < 0 || a.bitmap_off < 0 || a.codes_off < 0 ||
      a.total_k < 0 || a.total_idx < 0 || a.total_bm_words < 0 ||
      a.counts_off + 2LL * a.num_chunks > a.payload_bytes ||
      a.idx_off + 2LL * a.total_idx > a.payload_bytes ||
      a.bitmap_off + 4LL * a.total_bm_words > a.payload_bytes ||
      a.codes_off + 4LL * a.total_k > a.payload_bytes)
    throw std::runtime_error("ewdml sketch gather: a payload section does not fit");
  if (a.payload % 16 || a.counts_off % 2 || a.idx_off % 2 || a.bitmap_off % 4 || a.codes_off % 4 ||
      (a.chunks | a.tensors) % 4)
    throw std::runtime_error("ewdml sketch gather: misaligned operand");
  EW_LAUNCH(k_sketch_gather, a.num_chunks, a.stream, reinterpret_cast<const float*>(a.grad),
            reinterpret_cast<float*>(a.resid), reinterpret_cast<const ChunkRow*>(a.chunks),
            reinterpret_cast<const TensorRow*>(a.tensors), reinterpret_cast<uint8_t*>(a.payload),
            a.counts_off, a.idx_off, a.codes_off, a.bitmap_off);
  EW_CHECK_LAUNCH();
}
