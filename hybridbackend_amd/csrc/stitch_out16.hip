// The 16-bit stitch (include/hbk.h, "16-bit outputs", hbk_lookup_fwd_runs_out16): a group lookup over SEGMENTED tables
// -- the received rows of the sharded step, W runs per column -- that writes bf16 / fp16 rows: out[s] = round(f[s]),
// f[s] the fp32 row of hbk_group_lookup_fwd (fp32 rows, fp16 rows of the fused wire) or hbk_lowp_lookup_fwd_runs (a
// 16-bit table's own bits) over the same runs, rounded once per element to nearest even.
//
// How the work is split:
//   - the lane that HOLDS an id resolves it, once, to the element offset of its row inside the buffer; the row's lanes
//     get that offset by shuffle.  (The fp32 stitches hand the row number round and every lane of the row walks
//     run_start in global memory.)  The run table lives in registers: lane k of a wave holds run_start[k] and
//     run_base[k], read once per wave; a row's run is the last k with run_start[k] <= r, found by broadcasting the
//     table lane by lane (v_readlane, no memory, no LDS) against the 64 rows the wave's lanes hold at that moment --
//     n_runs compares for 64 ids.  A ballot serves ONE row per instruction and a wave holds 64 different ones, so
//     the broadcast form is the one kept.  More than 64 runs: the holding lane walks the arrays in memory.
//   - the STORE side picks the lane width W (a lane's W sums leave as one 16-, 8- or 2-byte non-temporal store) and
//     the LOAD side follows the run alignment: run bases are multiples of 4 elements (hbk_sharded_layout's padding),
//     not of 8, so a W = 8 lane feeds its store with two loads that need 4-element alignment only: 2 x 16 bytes of
//     fp32 rows, 2 x 8 bytes of 16-bit rows.
//   - one id per segment: a lane issues kRunsU row loads before its first store; ragged: lane `sub` of a row's group
//     owns id j0 + sub, and the next chunk's ids are fetched (and resolved behind the adds) while this chunk's rows
//     are in flight.
//
// The sums are lookup_out16.hip's, expression for expression; per-element sums are independent, so neither W nor the
// lane layout can change a bit.  No LDS, no atomics, no workspace, no host read.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "lookup_common.h"
#include "lowp_elems.h"

namespace hbk {
namespace {

constexpr int kRunsBlock = 256;
constexpr int kRunsWaves = kRunsBlock / kWave;
constexpr int kRunsMaxCols = 64;   // columns per launch (one lane per column in the tile search)
constexpr int kRunsU = 4;          // independent row loads per lane (one id per segment)
constexpr int kRunsSegIters = 4;   // segments per lane group and wave (ragged)
constexpr uint64_t kNoOff = 1ull << 63;   // no row: no element offset of a buffer has this pattern

struct RunCol {
  const void* table;
  const void* ids;
  const int32_t* splits;
  const float* weights;
  uint16_t* out;
  const int64_t* run_start;
  const int64_t* run_base;
  int64_t n_seg;
  uint64_t rows;
  int32_t dim;
  int32_t chunks;       // lane chunks per row
  int32_t out_stride;   // elements between output rows
  int32_t n_runs;
  uint8_t lpr_log2;
  uint8_t ids64;
  uint8_t combiner;
  uint8_t src_dtype;    // HBK_OUT16_TABLE_FP32 | HBK_LOWP_BF16 | HBK_LOWP_FP16
  uint8_t out_bf16;
};

struct RunArgs {
  int32_t n_cols;
  int32_t tile_start[kRunsMaxCols + 1];
  RunCol col[kRunsMaxCols];
};
static_assert(sizeof(RunArgs) <= 16384, "kernarg budget");

// a column's run table in registers: lane k holds run k (n_runs <= kWave)
struct RunRegs {
  int64_t start, base;
};

__device__ inline RunRegs load_runs(const RunCol& c) {
  RunRegs t = {0, 0};
  const int lane = lane_id();
  if (c.n_runs <= kWave && lane < c.n_runs) {
    t.start = c.run_start[lane];
    t.base = c.run_base[lane];
  }
  return t;
}

__device__ inline int64_t readlane_i64(int64_t v, int k) {   // k is uniform
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, k);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), k);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// id -> element offset of its row, or kNoOff outside [0, rows).  Called by every lane of the wave together (an idle
// lane passes -1).  The run is the one hbk_group_lookup_fwd's walk ends on: the last k with run_start[k] <= r, so an
// empty run (run_start[k] == run_start[k + 1]) is stepped over and a negative base is added as it is.
__device__ inline uint64_t resolve(const RunCol& c, const RunRegs& t, int64_t id) {
  const uint64_t r = (uint64_t)id;
  int64_t rs, rb;
  if (c.n_runs <= kWave) {   // (uniform)
    rs = readlane_i64(t.start, 0);
    rb = readlane_i64(t.base, 0);
    for (int k = 1; k < c.n_runs; ++k) {
      const int64_t s = readlane_i64(t.start, k);
      const int64_t b = readlane_i64(t.base, k);
      const bool take = (uint64_t)s <= r;
      rs = take ? s : rs;
      rb = take ? b : rb;
    }
  } else {
    if (id < 0 || r >= c.rows) return kNoOff;
    int k = 0;
    while (k + 1 < c.n_runs && (uint64_t)c.run_start[k + 1] <= r) ++k;
    rs = c.run_start[k];
    rb = c.run_base[k];
  }
  if (id < 0 || r >= c.rows) return kNoOff;
  return (uint64_t)rb + (r - (uint64_t)rs) * (uint64_t)c.dim;
}

// W elements at element `off` of the buffer, as fp32.  W = 8 is two loads of 4: `off` is a multiple of 4 only.
template <int W>
__device__ inline void load_src(const RunCol& c, uint64_t off, float (&v)[W]) {
  if (c.src_dtype == HBK_OUT16_TABLE_FP32) {   // (uniform: one column per workgroup)
    const float* t = static_cast<const float*>(c.table) + off;
    if constexpr (W == 1) {
      v[0] = *t;
    } else {
#pragma unroll
      for (int i = 0; i < W; i += 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(t + i);
        v[i] = x.x;
        v[i + 1] = x.y;
        v[i + 2] = x.z;
        v[i + 3] = x.w;
      }
    }
  } else {
    const uint16_t* t = static_cast<const uint16_t*>(c.table) + off;
    const bool bf16 = c.src_dtype == HBK_LOWP_BF16;
    if constexpr (W == 1) {
      v[0] = upcast(*t, bf16);
    } else {
      u32x2 p[W / 4];
#pragma unroll
      for (int i = 0; i < W / 4; ++i) p[i] = *reinterpret_cast<const u32x2*>(t + 4 * i);
#pragma unroll
      for (int i = 0; i < W / 2; ++i) {
        const uint32_t w = p[i / 2][i % 2];
        v[2 * i] = upcast(w & 0xffffu, bf16);
        v[2 * i + 1] = upcast(w >> 16, bf16);
      }
    }
  }
}

__device__ inline uint32_t round_out(float x, bool bf16) { return bf16 ? bf16_nearest(x) : fp16_nearest(x); }

// W sums rounded and stored at element `off` as ONE store (W = 8: 16-byte aligned, W = 4: 8-byte aligned), streamed
template <int W>
__device__ inline void store_out16(uint16_t* out, int64_t off, bool bf16, const float (&v)[W]) {
  if constexpr (W == 1) {
    __builtin_nontemporal_store((uint16_t)round_out(v[0], bf16), out + off);
  } else if constexpr (W == 4) {
    u32x2 p;
#pragma unroll
    for (int i = 0; i < 2; ++i) p[i] = round_out(v[2 * i], bf16) | (round_out(v[2 * i + 1], bf16) << 16);
    __builtin_nontemporal_store(p, reinterpret_cast<u32x2*>(out + off));
  } else {
    u32x4 p;
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = round_out(v[2 * i], bf16) | (round_out(v[2 * i + 1], bf16) << 16);
    __builtin_nontemporal_store(p, reinterpret_cast<u32x4*>(out + off));
  }
}

// one id per segment: out[s, :] = round(row(ids[s])), times the segment's weight when weighted
template <int W>
__device__ inline void stitch_rows(const RunCol& c, int64_t wave_row0) {
  const int lane = lane_id();
  const int lpr_log2 = c.lpr_log2;
  const int rpi = kWave >> lpr_log2;   // rows per wave instruction
  const int sub = lane & ((1 << lpr_log2) - 1);
  const int grp = lane >> lpr_log2;
  const int64_t n_seg = c.n_seg;
  const bool wgt = c.weights != nullptr;   // (uniform: one column per wave)
  const bool obf16 = c.out_bf16 != 0;
  const RunRegs runs = load_runs(c);

  // slot q (0 <= q < U * rpi) lives in register q >> 6 of lane q & 63: its id, resolved by this lane
  uint64_t offreg[kRunsU];
  float wreg[kRunsU];
  const int n_slots = kRunsU * rpi;
  int64_t idreg[kRunsU];
#pragma unroll
  for (int k = 0; k < kRunsU; ++k) {
    idreg[k] = -1;
    wreg[k] = 0.f;
    const int q = k * kWave + lane;
    const int64_t s = wave_row0 + q;
    if (q < n_slots && s < n_seg) {
      idreg[k] = load_id(c.ids, c.ids64, s);
      if (wgt) wreg[k] = __builtin_nontemporal_load(c.weights + s);
    }
  }
#pragma unroll
  for (int k = 0; k < kRunsU; ++k) {
    offreg[k] = kNoOff;
    if (k * kWave < n_slots) offreg[k] = resolve(c, runs, idreg[k]);   // (uniform)
  }
  float v[kRunsU][W];
  const bool live = sub < c.chunks;
  // every row load of the lane is issued before the first store
#pragma unroll
  for (int u = 0; u < kRunsU; ++u) {
    const int q0 = u * rpi;   // a multiple of rpi (a power of two <= 64): q0 >> 6 is uniform
    const int k = q0 >> 6;
    uint64_t src = offreg[0];
#pragma unroll
    for (int kk = 1; kk < kRunsU; ++kk) src = (k == kk) ? offreg[kk] : src;
    const uint64_t off = shfl_u64(src, (q0 & (kWave - 1)) + grp);
#pragma unroll
    for (int i = 0; i < W; ++i) v[u][i] = 0.f;
    if (live && off != kNoOff) load_src<W>(c, off + (uint64_t)sub * W, v[u]);
    if (wgt) {
      float w = wreg[0];
#pragma unroll
      for (int kk = 1; kk < kRunsU; ++kk) w = (k == kk) ? wreg[kk] : w;
      w = __shfl(w, (q0 & (kWave - 1)) + grp, kWave);
      const float div = c.combiner == HBK_COMBINER_MEAN    ? w
                        : c.combiner == HBK_COMBINER_SQRTN ? sqrtf(w * w)
                                                           : 1.f;
      if (off != kNoOff && div != 0.f) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
          v[u][i] = v[u][i] * w;
          if (c.combiner != HBK_COMBINER_SUM) v[u][i] = v[u][i] / div;
        }
      } else {
#pragma unroll
        for (int i = 0; i < W; ++i) v[u][i] = 0.f;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kRunsU; ++u) {
    const int64_t s = wave_row0 + u * rpi + grp;
    if (live && s < n_seg) store_out16<W>(c.out, s * (int64_t)c.out_stride + (int64_t)sub * W, obf16, v[u]);
  }
}

// ragged segments: out[s, :] = round(combine_j row(ids[j])) in id order, from +0
template <int W>
__device__ inline void stitch_segments(const RunCol& c, int64_t wave_seg0) {
  const int lane = lane_id();
  const int lpr_log2 = c.lpr_log2;
  const int lpr = 1 << lpr_log2;
  const int rpi = kWave >> lpr_log2;
  const int sub = lane & (lpr - 1);
  const int grp = lane >> lpr_log2;
  const int grp_lane0 = grp << lpr_log2;
  const int64_t n_seg = c.n_seg;
  const bool live = sub < c.chunks;
  const bool wgt = c.weights != nullptr;
  const bool obf16 = c.out_bf16 != 0;
  const RunRegs runs = load_runs(c);

  for (int it = 0; it < kRunsSegIters; ++it) {
    const int64_t s = wave_seg0 + (int64_t)it * rpi + grp;
    int32_t beg = 0, end = 0;
    if (s < n_seg) {
      beg = c.splits[s];
      end = c.splits[s + 1];
    }
    float acc[W];
#pragma unroll
    for (int i = 0; i < W; ++i) acc[i] = 0.f;
    float wsum = 0.f;   // weighted: W_s or Q_s
    int32_t j0 = beg;
    int64_t myid = -1;
    float myw = 0.f;
    if (j0 + sub < end) {
      myid = load_id(c.ids, c.ids64, j0 + sub);
      if (wgt) myw = __builtin_nontemporal_load(c.weights + j0 + sub);
    }
    uint64_t myoff = resolve(c, runs, myid);
    while (__any(j0 < end)) {
      int64_t nextid = -1;
      float nextw = 0.f;
      const int32_t j1 = j0 + lpr;
      if (j1 + sub < end) {
        nextid = load_id(c.ids, c.ids64, j1 + sub);
        if (wgt) nextw = __builtin_nontemporal_load(c.weights + j1 + sub);
      }
      const int32_t cnt = end - j0;   // ids of this group still to add (may be <= 0)
      for (int t0 = 0; t0 < lpr; t0 += 4) {
        float v[4][W];
        bool p[4];
        float w[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int tt = t0 + t;
          const uint64_t off = shfl_u64(myoff, grp_lane0 + (tt & (lpr - 1)));
          p[t] = tt < lpr && tt < cnt;
          w[t] = 0.f;
          if (wgt) {
            w[t] = __shfl(myw, grp_lane0 + (tt & (lpr - 1)), kWave);
            p[t] = p[t] && off != kNoOff;   // an invalid row adds neither term nor weight
          }
#pragma unroll
          for (int i = 0; i < W; ++i) v[t][i] = 0.f;
          if (p[t] && live && off != kNoOff) load_src<W>(c, off + (uint64_t)sub * W, v[t]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (!p[t]) continue;
          if (wgt) {
#pragma unroll
            for (int i = 0; i < W; ++i) acc[i] = acc[i] + v[t][i] * w[t];
            wsum = wsum + (c.combiner == HBK_COMBINER_SQRTN ? w[t] * w[t] : w[t]);
          } else {
#pragma unroll
            for (int i = 0; i < W; ++i) acc[i] = acc[i] + v[t][i];
          }
        }
      }
      myoff = resolve(c, runs, nextid);   // behind the adds: the ids have had the rows' latency to arrive
      myw = nextw;
      j0 = j1;
    }
    const int32_t n = end - beg;
    if (wgt) {
      if (c.combiner != HBK_COMBINER_SUM) {
        const float div = c.combiner == HBK_COMBINER_MEAN ? wsum : sqrtf(wsum);
#pragma unroll
        for (int i = 0; i < W; ++i) acc[i] = div != 0.f ? acc[i] / div : 0.f;
      }
    } else if (n > 0 && c.combiner == HBK_COMBINER_MEAN) {
      const float fn = (float)n;
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] = acc[i] / fn;
    } else if (n > 0 && c.combiner == HBK_COMBINER_SQRTN) {
      const float fn = sqrtf((float)n);
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] = acc[i] / fn;
    }
    if (live && s < n_seg) store_out16<W>(c.out, s * (int64_t)c.out_stride + (int64_t)sub * W, obf16, acc);
  }
}

// one kernel for the one-id-per-segment columns (CSR = false) and one for the ragged ones, per lane width
template <bool CSR, int W>
__global__ __launch_bounds__(kRunsBlock) void stitch_out16_kernel(const RunArgs a) {
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const int64_t tile = b - a.tile_start[ci];
  const RunCol& c = a.col[ci];
  const int wave = (int)(threadIdx.x >> 6);
  const int rpi = kWave >> c.lpr_log2;
  const int64_t first = (tile * kRunsWaves + wave) * (int64_t)((CSR ? kRunsSegIters : kRunsU) * rpi);
  if (first >= c.n_seg) return;
  if constexpr (CSR) {
    stitch_segments<W>(c, first);
  } else {
    stitch_rows<W>(c, first);
  }
}

template <bool CSR>
void launch_stitch(int w, const RunArgs& a, unsigned tiles, hipStream_t stream) {
  if (w == 8) {
    hipLaunchKernelGGL((stitch_out16_kernel<CSR, 8>), dim3(tiles), dim3(kRunsBlock), 0, stream, a);
  } else if (w == 4) {
    hipLaunchKernelGGL((stitch_out16_kernel<CSR, 4>), dim3(tiles), dim3(kRunsBlock), 0, stream, a);
  } else {
    hipLaunchKernelGGL((stitch_out16_kernel<CSR, 1>), dim3(tiles), dim3(kRunsBlock), 0, stream, a);
  }
}

// The default lane width (chunk_elems = 0) where a column allows both: 8 elements from this dim on, else 4, as
// lookup_out16.hip's kOutWide8FromDim.  Measured over 4-aligned bases (profiles/sharded_out16.txt, two runs agreeing):
// 8 is 5 % faster over fp32 rows at dim 64 and 128, 6 % and 29 % over bf16 rows; at dim 16 it is 2 % slower with one id
// per segment and 24 - 36 % slower on the ragged shape.
constexpr int kRunsWide8FromDim = 64;

}  // namespace
}  // namespace hbk

using namespace hbk;

extern "C" int hbk_lookup_fwd_runs_out16(int32_t n_cols, const hbk_out16_runs_column_t* cols, hbk_stream_t stream_) {
  static const char* kWho = "hbk_lookup_fwd_runs_out16";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", kWho, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", kWho);
  // every column is checked and classified before the first launch: elements per lane (1, 4, 8) and kind
  struct Classified {
    int w;   // 0: nothing to do (no segments)
    int chunks, lpr_log2;
  };
  std::vector<Classified> cls((size_t)std::max(n_cols, 1));
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_out16_lookup_column_t& h = cols[c].col;
    const bool fp32 = h.table_dtype == HBK_OUT16_TABLE_FP32;
    HBK_REQUIRE(fp32 || h.table_dtype == HBK_LOWP_BF16 || h.table_dtype == HBK_LOWP_FP16,
                "%s: column %d: table_dtype must be HBK_OUT16_TABLE_FP32, HBK_LOWP_BF16 or HBK_LOWP_FP16, got %d",
                kWho, c, h.table_dtype);
    HBK_REQUIRE(h.out_dtype == HBK_LOWP_BF16 || h.out_dtype == HBK_LOWP_FP16,
                "%s: column %d: out_dtype must be HBK_LOWP_BF16 or HBK_LOWP_FP16, got %d", kWho, c, h.out_dtype);
    HBK_REQUIRE(h.dim >= 1, "%s: column %d: dim must be >= 1, got %d", kWho, c, h.dim);
    HBK_REQUIRE(h.rows >= 0 && h.n_ids >= 0 && h.n_segments >= 0, "%s: column %d: negative size", kWho, c);
    HBK_REQUIRE(cols[c].n_runs >= 1 && cols[c].run_start != nullptr && cols[c].run_base != nullptr,
                "%s: column %d: bad segmented-table description (n_runs >= 1, run_start and run_base device arrays)",
                kWho, c);
    HBK_REQUIRE(h.ids_dtype == HBK_INT32 || h.ids_dtype == HBK_INT64, "%s: column %d: ids must be int32 or int64",
                kWho, c);
    HBK_REQUIRE(h.bucket == 0 && h.divisor == 1,
                "%s: column %d: ids are row numbers here: bucket must be 0 and divisor 1, got %lld and %d", kWho, c,
                (long long)h.bucket, h.divisor);
    HBK_REQUIRE(h.combiner >= HBK_COMBINER_SUM && h.combiner <= HBK_COMBINER_SQRTN,
                "%s: column %d: unknown combiner %d", kWho, c, h.combiner);
    HBK_REQUIRE(h.chunk_elems == 0 || h.chunk_elems == 4 || h.chunk_elems == 8,
                "%s: column %d: chunk_elems must be 0, 4 or 8, got %d", kWho, c, h.chunk_elems);
    HBK_REQUIRE(h.reserved == 0 && cols[c].reserved == 0, "%s: column %d: the reserved words must be 0, got %d and %d",
                kWho, c, h.reserved, cols[c].reserved);
    HBK_REQUIRE(h.row_splits != nullptr || h.n_segments == h.n_ids,
                "%s: column %d: n_segments (%lld) must equal n_ids (%lld) when row_splits is NULL", kWho, c,
                (long long)h.n_segments, (long long)h.n_ids);
    HBK_REQUIRE(h.n_ids < (1ll << 31) && h.n_segments < (1ll << 31),
                "%s: column %d: more than 2^31-1 ids/segments", kWho, c);
    HBK_REQUIRE(h.out_stride == 0 || h.out_stride >= h.dim, "%s: column %d: out_stride %d is smaller than dim %d",
                kWho, c, h.out_stride, h.dim);
    HBK_REQUIRE(((uintptr_t)h.table & (fp32 ? 3 : 1)) == 0, "%s: column %d: table must be aligned to its element",
                kWho, c);
    HBK_REQUIRE(((uintptr_t)h.out & 1) == 0, "%s: column %d: out must be 2-byte aligned", kWho, c);
    cls[(size_t)c].w = 0;
    if (h.n_segments == 0) continue;
    HBK_REQUIRE(h.table != nullptr || h.rows == 0, "%s: column %d: table is NULL", kWho, c);
    HBK_REQUIRE(h.out != nullptr, "%s: column %d: out is NULL", kWho, c);
    HBK_REQUIRE(h.ids != nullptr || h.n_ids == 0, "%s: column %d: ids is NULL", kWho, c);
    // the store side decides; the loads of either vector width need the buffer and the run bases on a 4-element
    // boundary only (the bases are device data: a promise of the caller's, hbk_sharded_layout keeps it)
    const uintptr_t out_bits = (uintptr_t)h.out | ((uintptr_t)(uint32_t)h.out_stride * 2);
    const bool src4 = (uintptr_t)h.table % (fp32 ? 16 : 8) == 0;
    const bool can4 = h.dim % 4 == 0 && out_bits % 8 == 0 && src4;
    const bool can8 = h.dim % 8 == 0 && out_bits % 16 == 0 && src4;
    const bool want8 = h.chunk_elems == 8 || (h.chunk_elems == 0 && h.dim >= kRunsWide8FromDim);
    const int w = can8 && want8 ? 8 : can4 ? 4 : 1;
    HBK_REQUIRE(h.dim <= (w > 1 ? 256 : 64),
                "%s: column %d: dim %d: at most 256 when dim %% 4 == 0, out and its stride are 8-byte aligned and the "
                "buffer is 16-byte (fp32) or 8-byte (16-bit) aligned, 64 otherwise", kWho, c, h.dim);
    cls[(size_t)c].w = w;
    cls[(size_t)c].chunks = h.dim / w;
    cls[(size_t)c].lpr_log2 = ceil_log2_u32((uint32_t)(h.dim / w));
  }
  hipStream_t stream = as_stream(stream_);
  static const int kWidths[3] = {4, 8, 1};
  for (int csr = 0; csr < 2; ++csr) {
    for (int w : kWidths) {
      int32_t c0 = 0;
      while (c0 < n_cols) {
        RunArgs args;
        int32_t k = 0;
        int64_t tiles = 0;
        args.tile_start[0] = 0;
        for (; c0 < n_cols && k < kRunsMaxCols; ++c0) {
          const hbk_out16_lookup_column_t& h = cols[c0].col;
          if (cls[(size_t)c0].w != w || (h.row_splits != nullptr) != (csr != 0)) continue;
          RunCol& d = args.col[k];
          d.table = h.table;
          d.ids = h.ids;
          d.splits = h.row_splits;
          d.weights = h.id_weights;
          d.out = static_cast<uint16_t*>(h.out);
          d.run_start = cols[c0].run_start;
          d.run_base = cols[c0].run_base;
          d.n_seg = h.n_segments;
          d.rows = (uint64_t)h.rows;
          d.dim = h.dim;
          d.chunks = cls[(size_t)c0].chunks;
          d.out_stride = h.out_stride > 0 ? h.out_stride : h.dim;
          d.n_runs = cols[c0].n_runs;
          d.lpr_log2 = (uint8_t)cls[(size_t)c0].lpr_log2;
          d.ids64 = h.ids_dtype == HBK_INT64;
          d.combiner = (uint8_t)h.combiner;
          d.src_dtype = (uint8_t)h.table_dtype;
          d.out_bf16 = h.out_dtype == HBK_LOWP_BF16;
          const int64_t rpi = kWave >> d.lpr_log2;
          const int64_t per_block = kRunsWaves * rpi * (csr ? kRunsSegIters : kRunsU);
          tiles += (h.n_segments + per_block - 1) / per_block;
          HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", kWho);
          ++k;
          args.tile_start[k] = (int32_t)tiles;
        }
        if (k == 0) continue;
        args.n_cols = k;
        if (csr) {
          launch_stitch<true>(w, args, (unsigned)tiles, stream);
        } else {
          launch_stitch<false>(w, args, (unsigned)tiles, stream);
        }
        HBK_HIP_OK(hipGetLastError());
      }
    }
  }
  return HBK_OK;
}
