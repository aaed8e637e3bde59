// 16-bit outputs (include/hbk.h, "16-bit outputs"): the group lookup's forward over fp32, bf16 or fp16 tables that
// writes bf16 / fp16 rows -- out[s] = round(f[s]), f[s] the fp32 row of hbk_group_lookup_fwd (fp32 table) or
// hbk_lowp_lookup_fwd (16-bit table), rounded once per element to nearest even.
//
//   hbk_group_lookup_fwd_out16   ragged, weighted columns over either table type.  Written fresh: lookup_fwd.hip's
//                                tiles carry segmented tables, output slots, D16, hot rows and the clip, and
//                                lowp_tables.hip's store side is built around 16-byte fp32 stores.  Here the STORE
//                                side picks the lane width: a row is owned by LPR = pow2(dim / W) adjacent lanes of W
//                                consecutive elements each, and a lane's W sums leave as ONE store -- W = 8: 16 bytes
//                                (fed by two 16-byte loads of an fp32 table, one of a 16-bit table), W = 4: 8 bytes,
//                                W = 1: 2 bytes, which touch no neighbouring byte (a column is a block of a wider
//                                tensor; what lies between blocks survives).  Pairs are packed into 4-byte words in
//                                registers: output memory is never read.  Ids and weights are read once per wave,
//                                non-temporally, and handed to the row's lanes by shuffle; a one-id-per-segment lane
//                                issues kOutU row loads before its first store; a ragged lane group fetches the next
//                                chunk of ids while this chunk's rows are in flight.
//
// The sums are those of lowp_tables.hip's forward, expression for expression (and so of lookup_fwd.hip's): per-element
// sums are independent, so neither W nor the lane layout can change a bit.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "lookup_common.h"
#include "lowp_elems.h"

namespace hbk {
namespace {

constexpr int kOutBlock = 256;
constexpr int kOutWaves = kOutBlock / kWave;
constexpr int kOutMaxCols = 64;   // columns per launch (one lane per column in the tile search)
constexpr int kOutU = 4;          // independent row loads per lane (one id per segment)
constexpr int kOutSegIters = 4;   // segments per lane group and wave (ragged)

struct OutCol {
  const void* table;
  const void* ids;
  const int32_t* splits;
  const float* weights;
  uint16_t* out;
  int64_t n_seg;
  IdMap map;
  int32_t dim;
  int32_t chunks;       // lane chunks per row
  int32_t out_stride;   // elements between output rows
  uint8_t lpr_log2;
  uint8_t ids64;
  uint8_t combiner;
  uint8_t table_dtype;  // HBK_OUT16_TABLE_FP32 | HBK_LOWP_BF16 | HBK_LOWP_FP16
  uint8_t out_bf16;
};

struct OutArgs {
  int32_t n_cols;
  int32_t tile_start[kOutMaxCols + 1];
  OutCol col[kOutMaxCols];
};
static_assert(sizeof(OutArgs) <= 16384, "kernarg budget");

// W elements of a row starting at element `off`, as fp32 (the branch is uniform: one column per workgroup)
template <int W>
__device__ inline void load_row(const OutCol& c, uint64_t off, float (&v)[W]) {
  if (c.table_dtype == HBK_OUT16_TABLE_FP32) {
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
    load_elems<W>(static_cast<const uint16_t*>(c.table), off, c.table_dtype == HBK_LOWP_BF16, v);
  }
}

__device__ inline uint32_t round16(float x, bool bf16) { return bf16 ? bf16_nearest(x) : fp16_nearest(x); }

// W sums rounded and stored at element `off` as one store (W = 8: 16-byte aligned, W = 4: 8-byte aligned), streamed
template <int W>
__device__ inline void store_row(uint16_t* out, int64_t off, bool bf16, const float (&v)[W]) {
  if constexpr (W == 1) {
    __builtin_nontemporal_store((uint16_t)round16(v[0], bf16), out + off);
  } else if constexpr (W == 4) {
    u32x2 p;
#pragma unroll
    for (int i = 0; i < 2; ++i) p[i] = round16(v[2 * i], bf16) | (round16(v[2 * i + 1], bf16) << 16);
    __builtin_nontemporal_store(p, reinterpret_cast<u32x2*>(out + off));
  } else {
    u32x4 p;
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = round16(v[2 * i], bf16) | (round16(v[2 * i + 1], bf16) << 16);
    __builtin_nontemporal_store(p, reinterpret_cast<u32x4*>(out + off));
  }
}

// one id per segment: out[s, :] = round(table[row(ids[s]), :]), times the segment's weight when weighted
template <int W>
__device__ inline void out16_gather_rows(const OutCol& c, int64_t wave_row0) {
  const int lane = lane_id();
  const int lpr_log2 = c.lpr_log2;
  const int rpi = kWave >> lpr_log2;   // rows per wave instruction
  const int sub = lane & ((1 << lpr_log2) - 1);
  const int grp = lane >> lpr_log2;
  const int64_t n_seg = c.n_seg;
  const bool wgt = c.weights != nullptr;   // (uniform: one column per wave)
  const bool obf16 = c.out_bf16 != 0;

  // ids: slot q (0 <= q < U * rpi) lives in register q >> 6 of lane q & 63
  uint64_t rowreg[kOutU];
  float wreg[kOutU];
  const int n_slots = kOutU * rpi;
#pragma unroll
  for (int k = 0; k < kOutU; ++k) {
    rowreg[k] = kNoRow;
    wreg[k] = 0.f;
    const int q = k * kWave + lane;
    const int64_t s = wave_row0 + q;
    if (q < n_slots && s < n_seg) {
      rowreg[k] = id_to_row(c.map, load_id(c.ids, c.ids64, s));
      if (wgt) wreg[k] = __builtin_nontemporal_load(c.weights + s);
    }
  }
  float v[kOutU][W];
  const bool live = sub < c.chunks;
  // every row load of the lane is issued before the first store
#pragma unroll
  for (int u = 0; u < kOutU; ++u) {
    const int q0 = u * rpi;   // a multiple of rpi (a power of two <= 64): q0 >> 6 is uniform
    const int k = q0 >> 6;
    uint64_t src = rowreg[0];
#pragma unroll
    for (int kk = 1; kk < kOutU; ++kk) src = (k == kk) ? rowreg[kk] : src;
    const uint64_t r = shfl_u64(src, (q0 & (kWave - 1)) + grp);
#pragma unroll
    for (int i = 0; i < W; ++i) v[u][i] = 0.f;
    if (live && r != kNoRow) load_row<W>(c, r * (uint64_t)c.dim + (uint64_t)sub * W, v[u]);
    if (wgt) {
      float w = wreg[0];
#pragma unroll
      for (int kk = 1; kk < kOutU; ++kk) w = (k == kk) ? wreg[kk] : w;
      w = __shfl(w, (q0 & (kWave - 1)) + grp, kWave);
      const float div = c.combiner == HBK_COMBINER_MEAN    ? w
                        : c.combiner == HBK_COMBINER_SQRTN ? sqrtf(w * w)
                                                           : 1.f;
      if (r != kNoRow && div != 0.f) {
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
  for (int u = 0; u < kOutU; ++u) {
    const int64_t s = wave_row0 + u * rpi + grp;
    if (live && s < n_seg) store_row<W>(c.out, s * (int64_t)c.out_stride + (int64_t)sub * W, obf16, v[u]);
  }
}

// ragged segments: out[s, :] = round(combine_j table[row(ids[j]), :]) in id order, from +0.  Lane `sub` of a group
// owns id j0 + sub of the group's segment; the next chunk of ids is fetched while this chunk's rows are in flight.
template <int W>
__device__ inline void out16_combine_segments(const OutCol& c, int64_t wave_seg0) {
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

  for (int it = 0; it < kOutSegIters; ++it) {
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
    uint64_t myrow = kNoRow;
    float myw = 0.f;
    if (j0 + sub < end) {
      myrow = id_to_row(c.map, load_id(c.ids, c.ids64, j0 + sub));
      if (wgt) myw = __builtin_nontemporal_load(c.weights + j0 + sub);
    }
    while (__any(j0 < end)) {
      uint64_t nextrow = kNoRow;
      float nextw = 0.f;
      const int32_t j1 = j0 + lpr;
      if (j1 + sub < end) {
        nextrow = id_to_row(c.map, load_id(c.ids, c.ids64, j1 + sub));
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
          const uint64_t r = shfl_u64(myrow, grp_lane0 + (tt & (lpr - 1)));
          p[t] = tt < lpr && tt < cnt;
          w[t] = 0.f;
          if (wgt) {
            w[t] = __shfl(myw, grp_lane0 + (tt & (lpr - 1)), kWave);
            p[t] = p[t] && r != kNoRow;   // an invalid row adds neither term nor weight
          }
#pragma unroll
          for (int i = 0; i < W; ++i) v[t][i] = 0.f;
          if (p[t] && live && r != kNoRow) load_row<W>(c, r * (uint64_t)c.dim + (uint64_t)sub * W, v[t]);
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
      myrow = nextrow;
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
    if (live && s < n_seg) store_row<W>(c.out, s * (int64_t)c.out_stride + (int64_t)sub * W, obf16, acc);
  }
}

// one kernel for the one-id-per-segment columns (CSR = false) and one for the ragged ones, per lane width
template <bool CSR, int W>
__global__ __launch_bounds__(kOutBlock) void lookup_out16_kernel(const OutArgs a) {
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const int64_t tile = b - a.tile_start[ci];
  const OutCol& c = a.col[ci];
  const int wave = (int)(threadIdx.x >> 6);
  const int rpi = kWave >> c.lpr_log2;
  const int64_t first = (tile * kOutWaves + wave) * (int64_t)((CSR ? kOutSegIters : kOutU) * rpi);
  if (first >= c.n_seg) return;
  if constexpr (CSR) {
    out16_combine_segments<W>(c, first);
  } else {
    out16_gather_rows<W>(c, first);
  }
}

template <bool CSR>
void launch_out16(int w, const OutArgs& a, unsigned tiles, hipStream_t stream) {
  if (w == 8) {
    hipLaunchKernelGGL((lookup_out16_kernel<CSR, 8>), dim3(tiles), dim3(kOutBlock), 0, stream, a);
  } else if (w == 4) {
    hipLaunchKernelGGL((lookup_out16_kernel<CSR, 4>), dim3(tiles), dim3(kOutBlock), 0, stream, a);
  } else {
    hipLaunchKernelGGL((lookup_out16_kernel<CSR, 1>), dim3(tiles), dim3(kOutBlock), 0, stream, a);
  }
}

// The default lane width (chunk_elems = 0) where a column allows both: 8 elements from this dim on, else 4.  Measured
// (profiles/out16_lookup.txt, two runs agreeing): over bf16 tables 8 is 16 - 19 % faster at dim 64 and 128 and 6 %
// (one id per segment) / 16 % (ragged) slower at dim 16, where it halves the lanes -- and with them the ids in flight
// -- of a row's group; over fp32 tables 8 is ahead by under 1 % at dim 64 and 128, by 2 % at dim 16 with one id per
// segment and 19 % slower on the ragged dim-16 shape.
constexpr int kOutWide8FromDim = 64;

}  // namespace
}  // namespace hbk

using namespace hbk;

extern "C" int hbk_group_lookup_fwd_out16(int32_t n_cols, const hbk_out16_lookup_column_t* cols,
                                          hbk_stream_t stream_) {
  static const char* kWho = "hbk_group_lookup_fwd_out16";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", kWho, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", kWho);
  // every column is checked and classified before the first launch: elements per lane (1, 4, 8) and kind
  struct Classified {
    int w;   // 0: nothing to do (no segments)
    int chunks, lpr_log2;
  };
  std::vector<Classified> cls((size_t)std::max(n_cols, 1));
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_out16_lookup_column_t& h = cols[c];
    const bool fp32 = h.table_dtype == HBK_OUT16_TABLE_FP32;
    HBK_REQUIRE(fp32 || h.table_dtype == HBK_LOWP_BF16 || h.table_dtype == HBK_LOWP_FP16,
                "%s: column %d: table_dtype must be HBK_OUT16_TABLE_FP32, HBK_LOWP_BF16 or HBK_LOWP_FP16, got %d",
                kWho, c, h.table_dtype);
    HBK_REQUIRE(h.out_dtype == HBK_LOWP_BF16 || h.out_dtype == HBK_LOWP_FP16,
                "%s: column %d: out_dtype must be HBK_LOWP_BF16 or HBK_LOWP_FP16, got %d", kWho, c, h.out_dtype);
    HBK_REQUIRE(h.dim >= 1, "%s: column %d: dim must be >= 1, got %d", kWho, c, h.dim);
    HBK_REQUIRE(h.rows >= 0 && h.n_ids >= 0 && h.n_segments >= 0, "%s: column %d: negative size", kWho, c);
    HBK_REQUIRE(h.ids_dtype == HBK_INT32 || h.ids_dtype == HBK_INT64, "%s: column %d: ids must be int32 or int64",
                kWho, c);
    HBK_REQUIRE(h.bucket >= 0, "%s: column %d: bucket must be >= 0", kWho, c);
    HBK_REQUIRE(h.divisor >= 1, "%s: column %d: divisor must be >= 1", kWho, c);
    HBK_REQUIRE(h.combiner >= HBK_COMBINER_SUM && h.combiner <= HBK_COMBINER_SQRTN,
                "%s: column %d: unknown combiner %d", kWho, c, h.combiner);
    HBK_REQUIRE(h.chunk_elems == 0 || h.chunk_elems == 4 || h.chunk_elems == 8,
                "%s: column %d: chunk_elems must be 0, 4 or 8, got %d", kWho, c, h.chunk_elems);
    HBK_REQUIRE(h.reserved == 0, "%s: column %d: the reserved word must be 0, got %d", kWho, c, h.reserved);
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
    // the store side decides: one 16-byte or one 8-byte store per lane needs `out` and its pitch on that boundary
    const uintptr_t out_bits = (uintptr_t)h.out | ((uintptr_t)(uint32_t)h.out_stride * 2);
    const uintptr_t table_bits = (uintptr_t)h.table;
    const bool can4 = h.dim % 4 == 0 && out_bits % 8 == 0 && table_bits % (fp32 ? 16 : 8) == 0;
    const bool can8 = h.dim % 8 == 0 && out_bits % 16 == 0 && table_bits % 16 == 0;
    const bool want8 = h.chunk_elems == 8 || (h.chunk_elems == 0 && h.dim >= kOutWide8FromDim);
    const int w = can8 && want8 ? 8 : can4 ? 4 : 1;
    HBK_REQUIRE(h.dim <= (w > 1 ? 256 : 64),
                "%s: column %d: dim %d: at most 256 when dim %% 4 == 0, out and its stride are 8-byte aligned and the "
                "table is 16-byte (fp32) or 8-byte (16-bit) aligned, 64 otherwise", kWho, c, h.dim);
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
        OutArgs args;
        int32_t k = 0;
        int64_t tiles = 0;
        args.tile_start[0] = 0;
        for (; c0 < n_cols && k < kOutMaxCols; ++c0) {
          const hbk_out16_lookup_column_t& h = cols[c0];
          if (cls[(size_t)c0].w != w || (h.row_splits != nullptr) != (csr != 0)) continue;
          OutCol& d = args.col[k];
          d.table = h.table;
          d.ids = h.ids;
          d.splits = h.row_splits;
          d.weights = h.id_weights;
          d.out = static_cast<uint16_t*>(h.out);
          d.n_seg = h.n_segments;
          d.map = make_idmap(h.bucket, h.divisor, h.rows);
          d.dim = h.dim;
          d.chunks = cls[(size_t)c0].chunks;
          d.out_stride = h.out_stride > 0 ? h.out_stride : h.dim;
          d.lpr_log2 = (uint8_t)cls[(size_t)c0].lpr_log2;
          d.ids64 = h.ids_dtype == HBK_INT64;
          d.combiner = (uint8_t)h.combiner;
          d.table_dtype = (uint8_t)h.table_dtype;
          d.out_bf16 = h.out_dtype == HBK_LOWP_BF16;
          const int64_t rpi = kWave >> d.lpr_log2;
          const int64_t per_block = kOutWaves * rpi * (csr ? kOutSegIters : kOutU);
          tiles += (h.n_segments + per_block - 1) / per_block;
          HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", kWho);
          ++k;
          args.tile_start[k] = (int32_t)tiles;
        }
        if (k == 0) continue;
        args.n_cols = k;
        if (csr) {
          launch_out16<true>(w, args, (unsigned)tiles, stream);
        } else {
          launch_out16<false>(w, args, (unsigned)tiles, stream);
        }
        HBK_HIP_OK(hipGetLastError());
      }
    }
  }
  return HBK_OK;
}
