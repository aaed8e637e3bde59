// Low-precision tables (include/hbk.h, "Low-precision tables"): rows of bf16 / fp16 elements, fp32 sums, fp32
// optimizer slots.
//
//   hbk_lowp_lookup_fwd      the forward: gather 2-byte rows, upcast exactly, combine in fp32 with the order and
//                            the start of the sum of lookup_fwd.hip's gather_rows / combine_segments -- the
//                            result is hbk_group_lookup_fwd on the upcast table, bit for bit.  Written fresh:
//                            that file's tiles carry segmented tables, output slots, D16, hot rows and the clip,
//                            this path has none of them.  A row is owned by LPR = pow2(dim / W) adjacent lanes, W
//                            elements each (W = 4: one 8-byte load, W = 8: one 16-byte load, W = 1: unaligned or
//                            dim % 4 != 0); ids are read once per wave, non-temporally, and handed to the row's
//                            lanes by shuffle; outputs are streamed with non-temporal 16-byte stores.
//   hbk_lowp_gather_rows_n   the owner gather of the sharded step onto a 16-bit wire: the gather's tiles without the
//                            upcast -- rows copied as bit patterns (8, 4 or 1 elements per lane), four row loads per
//                            lane in flight before the first store.
//   hbk_lowp_lookup_fwd_runs the requester's stitch over the received 16-bit rows: the forward's device functions
//                            instantiated over a column that carries a segmented table's run_start / run_base; the
//                            plain instantiations keep their code (the row offset is an overload on the column type).
//
// The element helpers (the upcast, the roundings) live in lowp_elems.h.  The backward is the fp32 reduce in its emit
// form, which never reads the table; the optimizer step on its slices, hbk_lowp_apply_slices_n, is sparse_apply.hip's
// walk over 16-bit rows and lives there.
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.h"
#include "lookup_common.h"
#include "lowp_elems.h"

namespace hbk {
namespace {

// W fp32 outputs at float offset `off` (W >= 4: 16-byte aligned), streamed
template <int W>
__device__ inline void store_out(float* out, int64_t off, const float (&v)[W]) {
  if constexpr (W == 1) {
    __builtin_nontemporal_store(v[0], out + off);
  } else {
#pragma unroll
    for (int i = 0; i < W; i += 4) {
      const f32x4 x = {v[i], v[i + 1], v[i + 2], v[i + 3]};
      __builtin_nontemporal_store(x, reinterpret_cast<f32x4*>(out + off + i));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// forward

constexpr int kFwdBlock = 256;
constexpr int kFwdWaves = kFwdBlock / kWave;
constexpr int kFwdMaxCols = 64;   // columns per launch (one lane per column in the tile search)
constexpr int kFwdU = 2;          // independent row loads per lane (one id per segment), as the fp32 gather
constexpr int kFwdSegIters = 4;   // segments per lane group and wave (ragged)

struct FwdCol {
  const uint16_t* table;
  const void* ids;
  const int32_t* splits;
  const float* weights;
  float* out;
  int64_t n_seg;
  IdMap map;
  int32_t dim;
  int32_t chunks;       // lane chunks per row
  int32_t out_stride;   // floats between output rows
  uint8_t lpr_log2;
  uint8_t ids64;
  uint8_t combiner;
  uint8_t bf16;
};

// the same column over a segmented table (hbk_lowp_lookup_fwd_runs): logical rows [run_start[k], run_start[k+1])
// live at table + run_base[k] elements (hbk_lookup_column_t's run tables)
struct FwdColRuns : FwdCol {
  const int64_t* run_start;
  const int64_t* run_base;
  int32_t n_runs;
  int32_t pad_;
};

template <typename Col>
struct FwdArgsT {
  int32_t n_cols;
  int32_t tile_start[kFwdMaxCols + 1];
  Col col[kFwdMaxCols];
};
typedef FwdArgsT<FwdCol> FwdArgs;
typedef FwdArgsT<FwdColRuns> FwdArgsRuns;
static_assert(sizeof(FwdArgs) <= 16384 && sizeof(FwdArgsRuns) <= 16384, "kernarg budget");

// element offset of logical row r inside the table (the segmented form: row_offset of lookup_fwd.hip)
__device__ inline uint64_t row_elem_offset(const FwdCol& c, uint64_t r) { return r * (uint64_t)c.dim; }
__device__ inline uint64_t row_elem_offset(const FwdColRuns& c, uint64_t r) {
  int k = 0;
  while (k + 1 < c.n_runs && (uint64_t)c.run_start[k + 1] <= r) ++k;
  return (uint64_t)c.run_base[k] + (r - (uint64_t)c.run_start[k]) * (uint64_t)c.dim;
}

// one id per segment: out[s, :] = upcast(table[row(ids[s]), :]), times the segment's weight when weighted
// (gather_rows of lookup_fwd.hip: the same expressions in the same order)
template <int W, typename Col>
__device__ inline void lowp_gather_rows(const Col& c, int64_t wave_row0) {
  const int lane = lane_id();
  const int lpr_log2 = c.lpr_log2;
  const int rpi = kWave >> lpr_log2;   // rows per wave instruction
  const int sub = lane & ((1 << lpr_log2) - 1);
  const int grp = lane >> lpr_log2;
  const int64_t n_seg = c.n_seg;
  const bool wgt = c.weights != nullptr;   // (uniform: one column per wave)
  const bool bf16 = c.bf16 != 0;

  // ids: slot q (0 <= q < U * rpi) lives in register q >> 6 of lane q & 63
  uint64_t rowreg[kFwdU];
  float wreg[kFwdU];
  const int n_slots = kFwdU * rpi;
#pragma unroll
  for (int k = 0; k < kFwdU; ++k) {
    rowreg[k] = kNoRow;
    wreg[k] = 0.f;
    const int q = k * kWave + lane;
    const int64_t s = wave_row0 + q;
    if (q < n_slots && s < n_seg) {
      rowreg[k] = id_to_row(c.map, load_id(c.ids, c.ids64, s));
      if (wgt) wreg[k] = __builtin_nontemporal_load(c.weights + s);
    }
  }
  float v[kFwdU][W];
  const bool live = sub < c.chunks;
#pragma unroll
  for (int u = 0; u < kFwdU; ++u) {
    const int q0 = u * rpi;   // a multiple of rpi (a power of two <= 64): q0 >> 6 is uniform
    const int k = q0 >> 6;
    uint64_t src = rowreg[0];
#pragma unroll
    for (int kk = 1; kk < kFwdU; ++kk) src = (k == kk) ? rowreg[kk] : src;
    const uint64_t r = shfl_u64(src, (q0 & (kWave - 1)) + grp);
#pragma unroll
    for (int i = 0; i < W; ++i) v[u][i] = 0.f;
    if (live && r != kNoRow) load_elems<W>(c.table, row_elem_offset(c, r) + (uint64_t)sub * W, bf16, v[u]);
    if (wgt) {
      float w = wreg[0];
#pragma unroll
      for (int kk = 1; kk < kFwdU; ++kk) w = (k == kk) ? wreg[kk] : w;
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
  for (int u = 0; u < kFwdU; ++u) {
    const int64_t s = wave_row0 + u * rpi + grp;
    if (live && s < n_seg) store_out<W>(c.out, s * (int64_t)c.out_stride + (int64_t)sub * W, v[u]);
  }
}

// ragged segments: out[s, :] = combine_j upcast(table[row(ids[j]), :]) in id order, from +0 (combine_segments
// of lookup_fwd.hip: the same expressions in the same order).  Lane `sub` of a group owns id j0 + sub of the
// group's segment; the next chunk of ids is fetched while this chunk's rows are in flight.
template <int W, typename Col>
__device__ inline void lowp_combine_segments(const Col& c, int64_t wave_seg0) {
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
  const bool bf16 = c.bf16 != 0;

  for (int it = 0; it < kFwdSegIters; ++it) {
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
          if (p[t] && live && r != kNoRow) {
            load_elems<W>(c.table, row_elem_offset(c, r) + (uint64_t)sub * W, bf16, v[t]);
          }
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
    if (live && s < n_seg) store_out<W>(c.out, s * (int64_t)c.out_stride + (int64_t)sub * W, acc);
  }
}

// one kernel for the one-id-per-segment columns (CSR = false) and one for the ragged ones, per lane width
template <bool CSR, int W, typename Args>
__device__ inline void lowp_lookup_fwd_body(const Args& a) {
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const int64_t tile = b - a.tile_start[ci];
  const auto& c = a.col[ci];
  const int wave = (int)(threadIdx.x >> 6);
  const int rpi = kWave >> c.lpr_log2;
  const int64_t first = (tile * kFwdWaves + wave) * (int64_t)((CSR ? kFwdSegIters : kFwdU) * rpi);
  if (first >= c.n_seg) return;
  if constexpr (CSR) {
    lowp_combine_segments<W>(c, first);
  } else {
    lowp_gather_rows<W>(c, first);
  }
}

template <bool CSR, int W>
__global__ __launch_bounds__(kFwdBlock) void lowp_lookup_fwd_kernel(const FwdArgs a) {
  lowp_lookup_fwd_body<CSR, W>(a);
}
// the stitch of the sharded step's 16-bit wire: the same tiles over a segmented table
template <bool CSR, int W>
__global__ __launch_bounds__(kFwdBlock) void lowp_lookup_fwd_runs_kernel(const FwdArgsRuns a) {
  lowp_lookup_fwd_body<CSR, W>(a);
}

template <bool CSR>
void launch_fwd(int w, const FwdArgs& a, unsigned tiles, hipStream_t stream) {
  if (w == 8) {
    hipLaunchKernelGGL((lowp_lookup_fwd_kernel<CSR, 8>), dim3(tiles), dim3(kFwdBlock), 0, stream, a);
  } else if (w == 4) {
    hipLaunchKernelGGL((lowp_lookup_fwd_kernel<CSR, 4>), dim3(tiles), dim3(kFwdBlock), 0, stream, a);
  } else {
    hipLaunchKernelGGL((lowp_lookup_fwd_kernel<CSR, 1>), dim3(tiles), dim3(kFwdBlock), 0, stream, a);
  }
}
template <bool CSR>
void launch_fwd(int w, const FwdArgsRuns& a, unsigned tiles, hipStream_t stream) {
  if (w == 8) {
    hipLaunchKernelGGL((lowp_lookup_fwd_runs_kernel<CSR, 8>), dim3(tiles), dim3(kFwdBlock), 0, stream, a);
  } else if (w == 4) {
    hipLaunchKernelGGL((lowp_lookup_fwd_runs_kernel<CSR, 4>), dim3(tiles), dim3(kFwdBlock), 0, stream, a);
  } else {
    hipLaunchKernelGGL((lowp_lookup_fwd_runs_kernel<CSR, 1>), dim3(tiles), dim3(kFwdBlock), 0, stream, a);
  }
}

bool dtype_ok(int32_t d) { return d == HBK_LOWP_BF16 || d == HBK_LOWP_FP16; }

// the column of a plain call and of a call over segmented tables: what the host loop reads of either
inline const hbk_lowp_lookup_column_t& lookup_col(const hbk_lowp_lookup_column_t& h) { return h; }
inline const hbk_lowp_lookup_column_t& lookup_col(const hbk_lowp_lookup_runs_column_t& h) { return h.col; }
inline void set_runs(FwdCol&, const hbk_lowp_lookup_column_t&) {}
inline void set_runs(FwdColRuns& d, const hbk_lowp_lookup_runs_column_t& h) {
  d.run_start = h.run_start;
  d.run_base = h.run_base;
  d.n_runs = h.n_runs;
  d.pad_ = 0;
}
inline bool runs_ok(const hbk_lowp_lookup_column_t&) { return true; }
inline bool runs_ok(const hbk_lowp_lookup_runs_column_t& h) {
  return h.n_runs >= 1 && h.run_start != nullptr && h.run_base != nullptr;
}

// HostCol = hbk_lowp_lookup_column_t (Args = FwdArgs) or hbk_lowp_lookup_runs_column_t (Args = FwdArgsRuns)
template <typename Args, typename HostCol>
int lowp_lookup_fwd(const char* kWho, int32_t n_cols, const HostCol* cols_, hbk_stream_t stream_) {
  constexpr bool kRuns = std::is_same<HostCol, hbk_lowp_lookup_runs_column_t>::value;
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", kWho, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols_ != nullptr, "%s: cols is NULL", kWho);
  auto cols = [&](int32_t c) -> const hbk_lowp_lookup_column_t& { return lookup_col(cols_[c]); };
  // every column is checked and classified before the first launch: elements per lane (1, 4, 8) and kind
  struct Classified {
    int w;      // 0: nothing to do (no segments)
    int chunks, lpr_log2;
    int blocks;   // 1, or (wide_rows) the column blocks of kWideBlock elements a wide row is served in
  };
  constexpr int kWideBlock = 64;   // one element per lane: a lane group holds at most a wave
  std::vector<Classified> cls((size_t)std::max(n_cols, 1));
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_lowp_lookup_column_t& h = cols(c);
    HBK_REQUIRE(dtype_ok(h.table_dtype), "%s: column %d: table_dtype must be HBK_LOWP_BF16 or HBK_LOWP_FP16, got %d",
                kWho, c, h.table_dtype);
    HBK_REQUIRE(h.dim >= 1, "%s: column %d: dim must be >= 1, got %d", kWho, c, h.dim);
    HBK_REQUIRE(h.rows >= 0 && h.n_ids >= 0 && h.n_segments >= 0, "%s: column %d: negative size", kWho, c);
    HBK_REQUIRE(runs_ok(cols_[c]), "%s: column %d: bad segmented-table description (n_runs >= 1, run_start and "
                "run_base device arrays)", kWho, c);
    HBK_REQUIRE(h.ids_dtype == HBK_INT32 || h.ids_dtype == HBK_INT64, "%s: column %d: ids must be int32 or int64",
                kWho, c);
    HBK_REQUIRE(h.bucket >= 0, "%s: column %d: bucket must be >= 0", kWho, c);
    HBK_REQUIRE(h.divisor >= 1, "%s: column %d: divisor must be >= 1", kWho, c);
    HBK_REQUIRE(h.combiner >= HBK_COMBINER_SUM && h.combiner <= HBK_COMBINER_SQRTN,
                "%s: column %d: unknown combiner %d", kWho, c, h.combiner);
    HBK_REQUIRE(h.chunk_elems == 0 || h.chunk_elems == 4 || h.chunk_elems == 8,
                "%s: column %d: chunk_elems must be 0, 4 or 8, got %d", kWho, c, h.chunk_elems);
    HBK_REQUIRE(h.wide_rows == 0 || h.wide_rows == 1, "%s: column %d: wide_rows must be 0 or 1, got %d", kWho, c,
                h.wide_rows);
    HBK_REQUIRE(h.row_splits != nullptr || h.n_segments == h.n_ids,
                "%s: column %d: n_segments (%lld) must equal n_ids (%lld) when row_splits is NULL", kWho, c,
                (long long)h.n_segments, (long long)h.n_ids);
    HBK_REQUIRE(h.n_ids < (1ll << 31) && h.n_segments < (1ll << 31),
                "%s: column %d: more than 2^31-1 ids/segments", kWho, c);
    HBK_REQUIRE(h.out_stride == 0 || h.out_stride >= h.dim, "%s: column %d: out_stride %d is smaller than dim %d",
                kWho, c, h.out_stride, h.dim);
    HBK_REQUIRE(((uintptr_t)h.table & 1) == 0, "%s: column %d: table must be 2-byte aligned", kWho, c);
    HBK_REQUIRE(((uintptr_t)h.out & 3) == 0, "%s: column %d: out must be 4-byte aligned", kWho, c);
    cls[(size_t)c].w = 0;
    if (h.n_segments == 0) continue;
    HBK_REQUIRE(h.table != nullptr || h.rows == 0, "%s: column %d: table is NULL", kWho, c);
    HBK_REQUIRE(h.out != nullptr, "%s: column %d: out is NULL", kWho, c);
    HBK_REQUIRE(h.ids != nullptr || h.n_ids == 0, "%s: column %d: ids is NULL", kWho, c);
    const uintptr_t out_bits = (uintptr_t)h.out | ((uintptr_t)(uint32_t)h.out_stride * 4);
    const bool vec = h.dim % 4 == 0 && (uintptr_t)h.table % 8 == 0 && out_bits % 16 == 0;
    // 8 elements per lane by default from dim 64 on: measured (profiles/lowp_tables.txt) 5 - 8 % faster than 4 at
    // dim 64, undecided at dim 128 (-1.8 % and +3.0 % in two runs), 9 - 12 % (one id per segment) and 15 % (ragged)
    // slower at dim 16, where it halves the lanes -- and with them the ids in flight -- of a row's group
    int w = vec ? 4 : 1;
    // (a segmented table's run bases are promised to be multiples of 4 elements only -- the padding of
    // hbk_sharded_layout --, so 8 elements per lane are taken there when the caller asks: chunk_elems = 8)
    const bool want8 = h.chunk_elems == 8 || (!kRuns && h.chunk_elems == 0 && h.dim >= 64);
    if (vec && want8 && h.dim % 8 == 0 && (uintptr_t)h.table % 16 == 0) w = 8;
    // wide_rows: a row of one element per lane wider than a wave goes in column blocks of kWideBlock elements, each a
    // column of its own to the kernel (per-element sums are independent: no bit depends on the split)
    const bool wide = h.wide_rows != 0 && !vec && h.dim > kWideBlock;
    HBK_REQUIRE(h.dim <= (vec || wide ? 256 : 64),
                "%s: column %d: dim %d: at most 256 when dim %% 4 == 0, the table is 8-byte aligned and out and its "
                "stride are 16-byte aligned, 64 otherwise", kWho, c, h.dim);
    cls[(size_t)c].w = w;
    cls[(size_t)c].chunks = h.dim / w;
    cls[(size_t)c].lpr_log2 = ceil_log2_u32((uint32_t)(h.dim / w));
    cls[(size_t)c].blocks = wide ? (h.dim + kWideBlock - 1) / kWideBlock : 1;
  }
  hipStream_t stream = as_stream(stream_);
  static const int kWidths[3] = {4, 8, 1};
  for (int csr = 0; csr < 2; ++csr) {
    for (int w : kWidths) {
      int32_t c0 = 0;
      while (c0 < n_cols) {
        Args args;
        int32_t k = 0;
        int64_t tiles = 0;
        args.tile_start[0] = 0;
        while (c0 < n_cols && k < kFwdMaxCols) {
          const int32_t ci = c0;
          const hbk_lowp_lookup_column_t& h = cols(ci);
          if (cls[(size_t)ci].w != w || (h.row_splits != nullptr) != (csr != 0)) {
            ++c0;
            continue;
          }
          const int blocks = cls[(size_t)ci].blocks;   // (at most 4: they fit an empty launch)
          if (k + blocks > kFwdMaxCols) break;          // the next launch takes the column whole
          ++c0;
          for (int b = 0; b < blocks; ++b) {
            // block b: elements [b * kWideBlock, ...) of every row and of every output row; d.dim stays the pitch
            const int first = b * kWideBlock;
            const int chunks = blocks == 1 ? cls[(size_t)ci].chunks : std::min(kWideBlock, h.dim - first);
            auto& d = args.col[k];
            set_runs(d, cols_[ci]);
            d.table = static_cast<const uint16_t*>(h.table) + first;
            d.ids = h.ids;
            d.splits = h.row_splits;
            d.weights = h.id_weights;
            d.out = h.out + first;
            d.n_seg = h.n_segments;
            d.map = make_idmap(h.bucket, h.divisor, h.rows);
            d.dim = h.dim;
            d.chunks = chunks;
            d.out_stride = h.out_stride > 0 ? h.out_stride : h.dim;
            d.lpr_log2 = (uint8_t)(blocks == 1 ? cls[(size_t)ci].lpr_log2 : (int)ceil_log2_u32((uint32_t)chunks));
            d.ids64 = h.ids_dtype == HBK_INT64;
            d.combiner = (uint8_t)h.combiner;
            d.bf16 = h.table_dtype == HBK_LOWP_BF16;
            const int64_t rpi = kWave >> d.lpr_log2;
            const int64_t per_block = kFwdWaves * rpi * (csr ? kFwdSegIters : kFwdU);
            tiles += (h.n_segments + per_block - 1) / per_block;
            HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", kWho);
            ++k;
            args.tile_start[k] = (int32_t)tiles;
          }
        }
        if (k == 0) continue;
        args.n_cols = k;
        if (csr) {
          launch_fwd<true>(w, args, (unsigned)tiles, stream);
        } else {
          launch_fwd<false>(w, args, (unsigned)tiles, stream);
        }
        HBK_HIP_OK(hipGetLastError());
      }
    }
  }
  return HBK_OK;
}

// ---------------------------------------------------------------------------------------------------------
// owner gather onto a 16-bit wire: out16[s, :] = table16[row(ids[s]), :] as bits (hbk_lowp_gather_rows_n)
//
// The tiles of lowp_gather_rows without the upcast: a row is owned by pow2(dim / W) adjacent lanes of W elements
// each, ids are read once per wave and handed to the row's lanes by shuffle, and a lane issues the loads of all
// its kBitsU rows before the first store.  The rows are half the bytes of the fp32 gather's, so a lane keeps
// twice the rows in flight for the same bytes.

constexpr int kBitsU = 4;   // independent row loads per lane

struct BitsCol {
  const uint16_t* table;
  const void* ids;
  uint16_t* out;
  int64_t n_seg;
  IdMap map;
  int32_t dim;
  int32_t chunks;       // lane chunks per row
  int32_t out_stride;   // elements between output rows
  uint8_t lpr_log2;
  uint8_t ids64;
};

struct BitsArgs {
  int32_t n_cols;
  int32_t tile_start[kFwdMaxCols + 1];
  BitsCol col[kFwdMaxCols];
};
static_assert(sizeof(BitsArgs) <= 16384, "kernarg budget");

template <int W>
struct BitsVec;
template <>
struct BitsVec<1> { typedef uint16_t type; };
template <>
struct BitsVec<4> { typedef u32x2 type; };
template <>
struct BitsVec<8> { typedef u32x4 type; };

// The stores into the send buffer are non-temporal although the exchange reads that buffer next: against plain
// stores the kernel alone was 3 % (dim 16), 8 % (dim 64) and 7 % (dim 128) faster, the ranges of 7 rounds apart
// (profiles/lowp_sharded.txt)
template <int W>
__global__ __launch_bounds__(kFwdBlock) void lowp_gather_bits_kernel(const BitsArgs a) {
  typedef typename BitsVec<W>::type V;
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const int64_t tile = b - a.tile_start[ci];
  const BitsCol& c = a.col[ci];
  const int wave = (int)(threadIdx.x >> 6);
  const int lpr_log2 = c.lpr_log2;
  const int rpi = kWave >> lpr_log2;   // rows per wave instruction
  const int64_t wave_row0 = (tile * kFwdWaves + wave) * (int64_t)(kBitsU * rpi);
  const int64_t n_seg = c.n_seg;
  if (wave_row0 >= n_seg) return;
  const int sub = lane & ((1 << lpr_log2) - 1);
  const int grp = lane >> lpr_log2;

  // ids: slot q (0 <= q < U * rpi) lives in register q >> 6 of lane q & 63
  uint64_t rowreg[kBitsU];
  const int n_slots = kBitsU * rpi;
#pragma unroll
  for (int k = 0; k < kBitsU; ++k) {
    rowreg[k] = kNoRow;
    const int q = k * kWave + lane;
    const int64_t s = wave_row0 + q;
    if (q < n_slots && s < n_seg) rowreg[k] = id_to_row(c.map, load_id(c.ids, c.ids64, s));
  }
  V v[kBitsU];
  const bool live = sub < c.chunks;
#pragma unroll
  for (int u = 0; u < kBitsU; ++u) {
    const int q0 = u * rpi;   // a multiple of rpi (a power of two <= 64): q0 >> 6 is uniform
    const int k = q0 >> 6;
    uint64_t src = rowreg[0];
#pragma unroll
    for (int kk = 1; kk < kBitsU; ++kk) src = (k == kk) ? rowreg[kk] : src;
    const uint64_t r = shfl_u64(src, (q0 & (kWave - 1)) + grp);
    v[u] = V{};   // (a row outside the table: 0x0000 elements, +0 in either type)
    if (live && r != kNoRow) {
      v[u] = *reinterpret_cast<const V*>(c.table + r * (uint64_t)c.dim + (uint64_t)sub * W);
    }
  }
#pragma unroll
  for (int u = 0; u < kBitsU; ++u) {
    const int64_t s = wave_row0 + u * rpi + grp;
    if (live && s < n_seg) {
      V* const o = reinterpret_cast<V*>(c.out + s * (int64_t)c.out_stride + (int64_t)sub * W);
      __builtin_nontemporal_store(v[u], o);
    }
  }
}

int lowp_gather_rows_n(int32_t n_cols, const hbk_lowp_gather_column_t* cols, hbk_stream_t stream_) {
  static const char* kWho = "lowp_gather_rows_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", kWho, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", kWho);
  std::vector<int> width((size_t)std::max(n_cols, 1), 0);   // elements per lane; 0: nothing to do
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_lowp_gather_column_t& h = cols[c];
    HBK_REQUIRE(h.dim >= 1, "%s: column %d: dim must be >= 1, got %d", kWho, c, h.dim);
    HBK_REQUIRE(h.rows >= 0 && h.n_ids >= 0, "%s: column %d: negative size", kWho, c);
    HBK_REQUIRE(h.ids_dtype == HBK_INT32 || h.ids_dtype == HBK_INT64, "%s: column %d: ids must be int32 or int64",
                kWho, c);
    HBK_REQUIRE(h.bucket >= 0, "%s: column %d: bucket must be >= 0", kWho, c);
    HBK_REQUIRE(h.divisor >= 1, "%s: column %d: divisor must be >= 1", kWho, c);
    HBK_REQUIRE(h.n_ids < (1ll << 31), "%s: column %d: more than 2^31-1 ids", kWho, c);
    HBK_REQUIRE(h.out_stride == 0 || h.out_stride >= h.dim, "%s: column %d: out_stride %d is smaller than dim %d",
                kWho, c, h.out_stride, h.dim);
    HBK_REQUIRE(((uintptr_t)h.table & 1) == 0 && ((uintptr_t)h.out & 1) == 0,
                "%s: column %d: table and out must be 2-byte aligned", kWho, c);
    if (h.n_ids == 0) continue;
    HBK_REQUIRE(h.table != nullptr || h.rows == 0, "%s: column %d: table is NULL", kWho, c);
    HBK_REQUIRE(h.out != nullptr, "%s: column %d: out is NULL", kWho, c);
    HBK_REQUIRE(h.ids != nullptr, "%s: column %d: ids is NULL", kWho, c);
    const uintptr_t bits = (uintptr_t)h.table | (uintptr_t)h.out | ((uintptr_t)(uint32_t)h.out_stride * 2);
    int w = 1;
    if (h.dim % 8 == 0 && bits % 16 == 0) {
      w = 8;
    } else if (h.dim % 4 == 0 && bits % 8 == 0) {
      w = 4;
    }
    HBK_REQUIRE(h.dim <= (w > 1 ? 256 : 64),
                "%s: column %d: dim %d: at most 256 when dim %% 4 == 0 and the table, out and its stride are 8-byte "
                "aligned, 64 otherwise", kWho, c, h.dim);
    width[(size_t)c] = w;
  }
  hipStream_t stream = as_stream(stream_);
  static const int kWidths[3] = {8, 4, 1};
  for (int w : kWidths) {
    int32_t c0 = 0;
    while (c0 < n_cols) {
      BitsArgs args;
      int32_t k = 0;
      int64_t tiles = 0;
      args.tile_start[0] = 0;
      while (c0 < n_cols && k < kFwdMaxCols) {
        const int32_t ci = c0++;
        if (width[(size_t)ci] != w) continue;
        const hbk_lowp_gather_column_t& h = cols[ci];
        BitsCol& d = args.col[k];
        d.table = static_cast<const uint16_t*>(h.table);
        d.ids = h.ids;
        d.out = static_cast<uint16_t*>(h.out);
        d.n_seg = h.n_ids;
        d.map = make_idmap(h.bucket, h.divisor, h.rows);
        d.dim = h.dim;
        d.chunks = h.dim / w;
        d.out_stride = h.out_stride > 0 ? h.out_stride : h.dim;
        d.lpr_log2 = (uint8_t)ceil_log2_u32((uint32_t)d.chunks);
        d.ids64 = h.ids_dtype == HBK_INT64;
        const int64_t per_block = (int64_t)kFwdWaves * (kWave >> d.lpr_log2) * kBitsU;
        tiles += (h.n_ids + per_block - 1) / per_block;
        HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", kWho);
        ++k;
        args.tile_start[k] = (int32_t)tiles;
      }
      if (k == 0) continue;
      args.n_cols = k;
      if (w == 8) {
        hipLaunchKernelGGL(lowp_gather_bits_kernel<8>, dim3((unsigned)tiles), dim3(kFwdBlock), 0, stream, args);
      } else if (w == 4) {
        hipLaunchKernelGGL(lowp_gather_bits_kernel<4>, dim3((unsigned)tiles), dim3(kFwdBlock), 0, stream, args);
      } else {
        hipLaunchKernelGGL(lowp_gather_bits_kernel<1>, dim3((unsigned)tiles), dim3(kFwdBlock), 0, stream, args);
      }
      HBK_HIP_OK(hipGetLastError());
    }
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_lowp_lookup_fwd(int32_t n_cols, const hbk_lowp_lookup_column_t* cols, hbk_stream_t stream) {
  return hbk::lowp_lookup_fwd<hbk::FwdArgs>("lowp_lookup_fwd", n_cols, cols, stream);
}

extern "C" int hbk_lowp_lookup_fwd_runs(int32_t n_cols, const hbk_lowp_lookup_runs_column_t* cols,
                                        hbk_stream_t stream) {
  return hbk::lowp_lookup_fwd<hbk::FwdArgsRuns>("lowp_lookup_fwd_runs", n_cols, cols, stream);
}

extern "C" int hbk_lowp_gather_rows_n(int32_t n_cols, const hbk_lowp_gather_column_t* cols, hbk_stream_t stream) {
  return hbk::lowp_gather_rows_n(n_cols, cols, stream);
}
