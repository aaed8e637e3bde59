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
//   hbk_lowp_apply_slices_n  the optimizer step on IndexedSlices: sparse_apply.hip's walk (wave tasks of
//                            kLowpItems rows per lane group, n_unique scanned on the device, grid-stride) with
//                            another load and store of w -- upcast a row, step it with the SAME rule functors
//                            (sparse_rules.h), round it back (nearest even, or stochastic for bf16).
//
//   hbk_lowp_gather_rows_n   the owner gather of the sharded step onto a 16-bit wire: the gather's tiles without the
//                            upcast -- rows copied as bit patterns (8, 4 or 1 elements per lane), four row loads per
//                            lane in flight before the first store.
//   hbk_lowp_lookup_fwd_runs the requester's stitch over the received 16-bit rows: the forward's device functions
//                            instantiated over a column that carries a segmented table's run_start / run_base; the
//                            plain instantiations keep their code (the row offset is an overload on the column type).
//
// The backward between the two is the fp32 reduce in its emit form, which never reads the table.
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.h"
#include "lookup_common.h"
#include "sparse_rules.h"

namespace hbk {
namespace {

// ---------------------------------------------------------------------------------------------------------
// element types

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ inline float up_bf16(uint32_t h) { return __uint_as_float(h << 16); }
__device__ inline float up_fp16(uint32_t h) {
  const uint16_t b = (uint16_t)h;
  _Float16 x;
  __builtin_memcpy(&x, &b, 2);
  return (float)x;
}
__device__ inline float upcast(uint32_t h, bool bf16) { return bf16 ? up_bf16(h) : up_fp16(h); }

// W elements of a row starting at element `off` (W = 4: 8-byte aligned, W = 8: 16-byte aligned), upcast
template <int W>
__device__ inline void load_elems(const uint16_t* table, uint64_t off, bool bf16, float (&v)[W]) {
  if constexpr (W == 1) {
    v[0] = upcast(table[off], bf16);
  } else if constexpr (W == 4) {
    const u32x2 p = *reinterpret_cast<const u32x2*>(table + off);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      v[2 * i] = upcast(p[i] & 0xffffu, bf16);
      v[2 * i + 1] = upcast(p[i] >> 16, bf16);
    }
  } else {
    const u32x4 p = *reinterpret_cast<const u32x4*>(table + off);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = upcast(p[i] & 0xffffu, bf16);
      v[2 * i + 1] = upcast(p[i] >> 16, bf16);
    }
  }
}

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
  };
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
    HBK_REQUIRE(h.dim <= (vec ? 256 : 64),
                "%s: column %d: dim %d: at most 256 when dim %% 4 == 0, the table is 8-byte aligned and out and its "
                "stride are 16-byte aligned, 64 otherwise", kWho, c, h.dim);
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
        Args args;
        int32_t k = 0;
        int64_t tiles = 0;
        args.tile_start[0] = 0;
        while (c0 < n_cols && k < kFwdMaxCols) {
          const int32_t ci = c0++;
          const hbk_lowp_lookup_column_t& h = cols(ci);
          if (cls[(size_t)ci].w != w || (h.row_splits != nullptr) != (csr != 0)) continue;
          auto& d = args.col[k];
          set_runs(d, cols_[ci]);
          d.table = static_cast<const uint16_t*>(h.table);
          d.ids = h.ids;
          d.splits = h.row_splits;
          d.weights = h.id_weights;
          d.out = h.out;
          d.n_seg = h.n_segments;
          d.map = make_idmap(h.bucket, h.divisor, h.rows);
          d.dim = h.dim;
          d.chunks = cls[(size_t)ci].chunks;
          d.out_stride = h.out_stride > 0 ? h.out_stride : h.dim;
          d.lpr_log2 = (uint8_t)cls[(size_t)ci].lpr_log2;
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

// ---------------------------------------------------------------------------------------------------------
// apply

constexpr int kLowpMaxCols = 64;   // columns per apply launch
constexpr int kLowpBlock = 256;
constexpr int kLowpWaves = kLowpBlock / kWave;
constexpr int kLowpItems = 4;      // rows per lane group in flight
constexpr int kLowpBlocksPerCU = 8;
static_assert(kLowpMaxCols <= kWave, "one lane per column in the task scan");

struct LowpCol {
  uint16_t* w;
  float* s0;
  float* s1;
  const int64_t* urows;
  const float* grows;   // [cap, dim] contiguous
  const int32_t* nu;
  int64_t rows;
  int32_t cap;
  int32_t dim;
  int32_t index;        // the column's index in the CALL (the noise is keyed by it)
  uint8_t lpr_log2;
  uint8_t vec4;
  uint8_t bf16;
};

struct LowpRound {
  const uint32_t* step;   // NULL: round to nearest even
  uint32_t seed;
};

template <typename P>
struct LowpArgs {
  LowpCol c[kLowpMaxCols];
  P p;
  LowpRound round;
  int32_t n_cols;
};

// murmur3's finalizer, and the noise of include/hbk.h
__device__ inline uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__device__ inline uint32_t noise_base(uint32_t seed, uint32_t step, int32_t c) {
  return fmix32(seed ^ fmix32(step + 0x9E3779B9u * ((uint32_t)c + 1u)));
}
__device__ inline uint32_t noise_row(uint32_t base, int64_t r) {
  return fmix32(fmix32(base ^ (uint32_t)(uint64_t)r) ^ (uint32_t)((uint64_t)r >> 32));
}
__device__ inline uint32_t noise_elem(uint32_t rowh, int k) {
  return fmix32(rowh + 0x9E3779B9u * ((uint32_t)k + 1u));
}

// fp32 -> bf16, round to nearest even (a NaN stays a NaN: 0x7FC0)
__device__ inline uint32_t bf16_nearest(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// fp32 -> bf16, stochastic: nearest when the exponent field is all ones, else add 16 bits of noise and cut
__device__ inline uint32_t bf16_stochastic(float x, uint32_t noise) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7f800000u) == 0x7f800000u) return bf16_nearest(x);
  return (u + (noise & 0xffffu)) >> 16;
}
__device__ inline uint32_t fp16_nearest(float x) {
  const _Float16 h = (_Float16)x;
  uint16_t b;
  __builtin_memcpy(&b, &h, 2);
  return b;
}

// element k0 + i of row r rounded to the table's type
__device__ inline uint32_t round_elem(float x, bool bf16, bool stochastic, uint32_t rowh, int k) {
  if (!bf16) return fp16_nearest(x);
  return stochastic ? bf16_stochastic(x, noise_elem(rowh, k)) : bf16_nearest(x);
}

// a lane chunk of a row of the table: load + upcast, round + store.  V = f32x4: 4 elements (8 bytes), V = float: one
__device__ inline f32x4 load_w(const uint16_t* p, bool bf16, f32x4) {
  float v[4];
  load_elems<4>(p, 0, bf16, v);
  return f32x4{v[0], v[1], v[2], v[3]};
}
__device__ inline float load_w(const uint16_t* p, bool bf16, float) { return upcast(*p, bf16); }
__device__ inline void store_w(uint16_t* p, f32x4 v, bool bf16, bool stochastic, uint32_t rowh, int k0) {
  u32x2 o;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    o[i] = round_elem(v[2 * i], bf16, stochastic, rowh, k0 + 2 * i) |
           (round_elem(v[2 * i + 1], bf16, stochastic, rowh, k0 + 2 * i + 1) << 16);
  }
  *reinterpret_cast<u32x2*>(p) = o;
}
__device__ inline void store_w(uint16_t* p, float v, bool bf16, bool stochastic, uint32_t rowh, int k0) {
  *p = (uint16_t)round_elem(v, bf16, stochastic, rowh, k0);
}

// one task: rows base + k * groups + grp (k < kLowpItems) of column c; W elements per lane chunk -- slot_task of
// sparse_apply.hip with the table's load and store replaced (no clip, no pitch, no emit rule).  A lane issues
// the w / slot / slot / g loads of all its rows before any arithmetic.
template <typename V, int W, typename Rule>
__device__ inline void lowp_task(const LowpCol& c, int64_t base, int64_t n, const Rule& rule, const LowpRound& round,
                                 uint32_t step) {
  const int lane = lane_id();
  const int lpr = c.lpr_log2;
  const int grp = lane >> lpr;
  const int sub = lane & ((1 << lpr) - 1);
  const int groups = kWave >> lpr;
  const bool lane_on = sub * W < c.dim;
  const bool bf16 = c.bf16 != 0;
  const bool stochastic = round.step != nullptr;
  int64_t r[kLowpItems];
  bool on[kLowpItems];
#pragma unroll
  for (int k = 0; k < kLowpItems; ++k) {
    const int64_t u = base + (int64_t)k * groups + grp;
    on[k] = lane_on && u < n;
    r[k] = on[k] ? __builtin_nontemporal_load(c.urows + u) : 0;
    on[k] = on[k] && (uint64_t)r[k] < (uint64_t)c.rows;   // (holes: -1, or anything outside the table)
  }
  V w[kLowpItems], s0[kLowpItems], s1[kLowpItems], g[kLowpItems];
#pragma unroll
  for (int k = 0; k < kLowpItems; ++k) w[k] = s0[k] = s1[k] = g[k] = zero_v<V>();
  float acc[Rule::kRowwise ? kLowpItems : 1], sq[Rule::kRowwise ? kLowpItems : 1];
  if constexpr (Rule::kRowwise) {
#pragma unroll
    for (int k = 0; k < kLowpItems; ++k) acc[k] = 0.0f;
  }
#pragma unroll
  for (int k = 0; k < kLowpItems; ++k) {
    if (!on[k]) continue;
    const int64_t u = base + (int64_t)k * groups + grp;
    const int64_t off = r[k] * c.dim + sub * W;
    w[k] = load_w(c.w + off, bf16, V());
    if constexpr (Rule::kSlots >= 1) s0[k] = *reinterpret_cast<const V*>(c.s0 + off);
    if constexpr (Rule::kSlots >= 2) s1[k] = *reinterpret_cast<const V*>(c.s1 + off);
    if constexpr (Rule::kRowwise) acc[k] = c.s0[r[k]];
    g[k] = __builtin_nontemporal_load(reinterpret_cast<const V*>(c.grows + u * c.dim + sub * W));
  }
  if constexpr (Rule::kRowwise) {
    // every lane of the wave takes part (lanes without a row or past dim pass +0.0f)
#pragma unroll
    for (int k = 0; k < kLowpItems; ++k) sq[k] = group_sum(chunk_sum(g[k] * g[k]), lpr);
  }
  const uint32_t nbase = stochastic ? noise_base(round.seed, step, c.index) : 0u;
#pragma unroll
  for (int k = 0; k < kLowpItems; ++k) {
    if (!on[k]) continue;
    const int64_t off = r[k] * c.dim + sub * W;
    const uint32_t rowh = stochastic ? noise_row(nbase, r[k]) : 0u;
    if constexpr (Rule::kRowwise) {
      float rate;
      const float na = rule.row(acc[k], sq[k], (float)c.dim, &rate);
      if (sub == 0) c.s0[r[k]] = na;
      store_w(c.w + off, w[k] - rate * g[k], bf16, stochastic, rowh, sub * W);
    } else {
      const Stepped<V> o = rule(w[k], s0[k], s1[k], g[k]);
      if constexpr (Rule::kSlots >= 1) *reinterpret_cast<V*>(c.s0 + off) = o.s0;
      if constexpr (Rule::kSlots >= 2) *reinterpret_cast<V*>(c.s1 + off) = o.s1;
      store_w(c.w + off, o.w, bf16, stochastic, rowh, sub * W);
    }
  }
}

// the body of every apply kernel (slot_apply_body of sparse_apply.hip): wave 0 reads the columns' n_unique
// (clamped to the capacity) and scans their task counts into LDS, lane 0 runs the rule's setup; after the
// barrier every wave walks the tasks grid-stride
template <typename Rule>
__device__ inline void lowp_apply_body(const LowpArgs<typename Rule::Params>& a) {
  __shared__ int64_t s_end[kLowpMaxCols];   // inclusive prefix of the columns' task counts
  __shared__ int64_t s_n[kLowpMaxCols];     // their n_unique (clamped to the capacity)
  if (threadIdx.x < kWave) {
    const int lane = (int)threadIdx.x;
    int64_t tasks = 0;
    if (lane < a.n_cols) {
      const LowpCol& c = a.c[lane];
      const int64_t n = min(max(__builtin_nontemporal_load(c.nu), 0), c.cap);
      const int64_t rpt = (int64_t)(kWave >> c.lpr_log2) * kLowpItems;
      tasks = (n + rpt - 1) / rpt;
      s_n[lane] = n;
    }
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int64_t t = __shfl_up(tasks, d, kWave);
      if (lane >= d) tasks += t;
    }
    if (lane < a.n_cols) s_end[lane] = tasks;
    if (lane == 0) Rule::setup(a.p);
  }
  __syncthreads();
  const typename Rule::State st = Rule::state();
  const uint32_t step = a.round.step != nullptr ? *a.round.step : 0u;   // (read before the advance launch writes it)
  const int64_t total = s_end[a.n_cols - 1];
  int ci = 0;
  for (int64_t t = (int64_t)blockIdx.x * kLowpWaves + threadIdx.x / kWave; t < total;
       t += (int64_t)gridDim.x * kLowpWaves) {
    while (s_end[ci] <= t) ++ci;   // (t only grows: the column only moves forward)
    const LowpCol& col = a.c[ci];
    const int64_t t0 = ci == 0 ? 0 : s_end[ci - 1];
    const int64_t base = (t - t0) * ((int64_t)(kWave >> col.lpr_log2) * kLowpItems);
    if (col.vec4) {
      lowp_task<f32x4, 4, Rule>(col, base, s_n[ci], Rule(a.p, st), a.round, step);
    } else {
      lowp_task<float, 1, Rule>(col, base, s_n[ci], Rule(a.p, st), a.round, step);
    }
  }
}

template <typename Rule>
__global__ __launch_bounds__(kLowpBlock) void lowp_apply_kernel(LowpArgs<typename Rule::Params> a) {
  lowp_apply_body<Rule>(a);
}

// TF's _finish (adam_finish_kernel of sparse_apply.hip): beta1^t, beta2^t -> beta1^(t+1), beta2^(t+1)
__global__ void lowp_adam_finish_kernel(float* powers, float beta1, float beta2) {
  if (threadIdx.x == 0) {
    powers[0] = powers[0] * beta1;
    powers[1] = powers[1] * beta2;
  }
}

// the step counter of the stochastic rounding, behind the apply in stream order
__global__ void lowp_advance_kernel(uint32_t* step) {
  if (threadIdx.x == 0) step[0] = step[0] + 1u;
}

// the launches of one call: launch(args, blocks, stream) sets args.p and launches the rule's kernel
template <typename P, typename Launch>
int launch_lowp(int32_t n_cols, const hbk_lowp_slices_column_t* cols, const std::vector<RowShape>& shapes,
                float* const* s0, float* const* s1, const LowpRound& round, hipStream_t stream, Launch launch) {
  for (int32_t c0 = 0; c0 < n_cols; c0 += kLowpMaxCols) {
    LowpArgs<P> a;
    memset(&a, 0, sizeof(a));
    a.round = round;
    int64_t tasks = 0;
    int k = 0;
    for (int32_t c = c0; c < std::min(n_cols, c0 + kLowpMaxCols); ++c) {
      const hbk_lowp_slices_column_t& h = cols[c];
      if (h.capacity <= 0 || h.rows <= 0) continue;
      LowpCol& d = a.c[k];
      d.w = static_cast<uint16_t*>(h.table);
      d.s0 = s0 != nullptr ? s0[c] : nullptr;
      d.s1 = s1 != nullptr ? s1[c] : nullptr;
      d.urows = h.unique_rows;
      d.grows = h.grad_rows;
      d.nu = h.n_unique;
      d.rows = h.rows;
      d.cap = (int32_t)h.capacity;
      d.dim = h.dim;
      d.index = c;
      d.lpr_log2 = shapes[(size_t)c].lpr_log2;
      d.vec4 = shapes[(size_t)c].vec4;
      d.bf16 = h.table_dtype == HBK_LOWP_BF16;
      const int64_t rpt = (int64_t)(kWave >> d.lpr_log2) * kLowpItems;
      tasks += (std::min<int64_t>(h.capacity, h.rows) + rpt - 1) / rpt;
      ++k;
    }
    if (k == 0) continue;
    a.n_cols = k;
    const int64_t want = (tasks + kLowpWaves - 1) / kLowpWaves;
    const unsigned blocks =
        (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus() * kLowpBlocksPerCU));
    launch(a, blocks, stream);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

int lowp_apply_slices(int32_t n_cols, const hbk_lowp_slices_column_t* cols, int32_t apply, float* const* slot0,
                      float* const* slot1, const void* params, float lr, const hbk_lowp_rounding_t* rounding,
                      hbk_stream_t stream_) {
  static const char* kWho = "lowp_apply_slices_n";
  constexpr float kMax = 3.402823466e38f;
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", kWho, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", kWho);
  HBK_REQUIRE(apply == HBK_APPLY_SGD || apply == HBK_APPLY_ADAGRAD || apply == HBK_APPLY_LAZY_ADAM ||
                  apply == HBK_APPLY_FTRL || apply == HBK_APPLY_ROWWISE_ADAGRAD,
              "%s: apply must be HBK_APPLY_SGD, _ADAGRAD, _LAZY_ADAM, _FTRL or _ROWWISE_ADAGRAD, got %d", kWho,
              apply);
  const int32_t mode = rounding != nullptr ? rounding->mode : HBK_LOWP_ROUND_NEAREST;
  HBK_REQUIRE(mode == HBK_LOWP_ROUND_NEAREST || mode == HBK_LOWP_ROUND_STOCHASTIC,
              "%s: rounding mode must be HBK_LOWP_ROUND_NEAREST or HBK_LOWP_ROUND_STOCHASTIC, got %d", kWho, mode);
  const bool stochastic = mode == HBK_LOWP_ROUND_STOCHASTIC;
  HBK_REQUIRE(!stochastic || (rounding->step != nullptr && ((uintptr_t)rounding->step & 3) == 0),
              "%s: stochastic rounding needs a device uint32 [1] step counter", kWho);
  // the rule's slots: how many table-shaped ones (they enter the row shape's alignment), and the row-wise one
  const int n_slots = apply == HBK_APPLY_ADAGRAD ? 1 : (apply == HBK_APPLY_LAZY_ADAM || apply == HBK_APPLY_FTRL) ? 2 : 0;
  const bool rowwise = apply == HBK_APPLY_ROWWISE_ADAGRAD;
  const char* n0 = apply == HBK_APPLY_LAZY_ADAM ? "m" : apply == HBK_APPLY_FTRL ? "accum" : "the accumulator";
  const char* n1 = apply == HBK_APPLY_LAZY_ADAM ? "v" : "linear";
  // the hyperparameters and the lr, as the rule's own entry refuses them
  int rc = HBK_OK;
  if (apply == HBK_APPLY_LAZY_ADAM) {
    if ((rc = adam_check(static_cast<const hbk_adam_t*>(params), lr, kWho)) != HBK_OK) return rc;
  } else if (apply == HBK_APPLY_FTRL) {
    if ((rc = ftrl_check(static_cast<const hbk_ftrl_t*>(params), lr, kWho)) != HBK_OK) return rc;
  } else if (rowwise) {
    if ((rc = rowwise_adagrad_check(static_cast<const hbk_rowwise_adagrad_t*>(params), lr, kWho)) != HBK_OK) return rc;
  } else {
    HBK_REQUIRE(lr != 0.0f && lr >= -kMax && lr <= kMax, "%s: lr must be finite and != 0, got %g", kWho, (double)lr);
  }
  HBK_REQUIRE(n_cols == 0 || (n_slots < 1 && !rowwise) || slot0 != nullptr, "%s: the %s array (slot0) is NULL", kWho, n0);
  HBK_REQUIRE(n_cols == 0 || n_slots < 2 || slot1 != nullptr, "%s: the %s array (slot1) is NULL", kWho, n1);
  std::vector<RowShape> shapes((size_t)n_cols, RowShape{});
  std::vector<uintptr_t> seen;
  seen.reserve((size_t)n_cols * 3);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_lowp_slices_column_t& s = cols[c];
    HBK_REQUIRE(dtype_ok(s.table_dtype), "%s: column %d: table_dtype must be HBK_LOWP_BF16 or HBK_LOWP_FP16, got %d",
                kWho, c, s.table_dtype);
    HBK_REQUIRE(!stochastic || s.table_dtype == HBK_LOWP_BF16,
                "%s: column %d: stochastic rounding is defined for bf16 tables only", kWho, c);
    HBK_REQUIRE(s.capacity >= 0 && s.capacity < (1ll << 30), "%s: column %d: capacity %lld must be in [0, 2^30)",
                kWho, c, (long long)s.capacity);
    HBK_REQUIRE(s.rows >= 0, "%s: column %d: rows must be >= 0, got %lld", kWho, c, (long long)s.rows);
    HBK_REQUIRE(s.dim >= 1, "%s: column %d: dim must be >= 1", kWho, c);
    HBK_REQUIRE(((uintptr_t)s.table & 1) == 0, "%s: column %d: table must be 2-byte aligned", kWho, c);
    float* const a0 = (n_slots >= 1 || rowwise) ? slot0[c] : nullptr;
    float* const a1 = n_slots >= 2 ? slot1[c] : nullptr;
    HBK_REQUIRE(!(n_slots >= 1 || rowwise) || (a0 != nullptr && ((uintptr_t)a0 & 3) == 0),
                "%s: column %d: %s must be a device fp32 buffer", kWho, c, n0);
    HBK_REQUIRE(n_slots < 2 || (a1 != nullptr && ((uintptr_t)a1 & 3) == 0),
                "%s: column %d: %s must be a device fp32 buffer", kWho, c, n1);
    if (s.capacity > 0) {
      HBK_REQUIRE(s.table != nullptr, "%s: column %d: table is NULL", kWho, c);
      HBK_REQUIRE(s.unique_rows != nullptr && ((uintptr_t)s.unique_rows & 7) == 0,
                  "%s: column %d: unique_rows must be a device int64 [capacity]", kWho, c);
      HBK_REQUIRE(s.grad_rows != nullptr && ((uintptr_t)s.grad_rows & 3) == 0,
                  "%s: column %d: grad_rows must be a device fp32 [capacity, dim]", kWho, c);
      HBK_REQUIRE(s.n_unique != nullptr && ((uintptr_t)s.n_unique & 3) == 0,
                  "%s: column %d: n_unique must be a device int32 [1]", kWho, c);
      // the row shape of the fp32 entry: the table's bytes count twice (an 8-byte chunk where fp32 has 16), the
      // row-wise word does not enter
      const uintptr_t bits = ((uintptr_t)s.table * 2) | (uintptr_t)s.grad_rows |
                             (n_slots >= 1 ? (uintptr_t)a0 : 0) | (uintptr_t)a1;
      HBK_REQUIRE(make_rowshape(s.dim, bits, &shapes[(size_t)c]),
                  "%s: column %d: dim %d: at most 256 when dim %% 4 == 0, the table is 8-byte and the slots and "
                  "grad_rows are 16-byte aligned, 64 otherwise", kWho, c, s.dim);
    }
    if (s.table != nullptr) seen.push_back((uintptr_t)s.table);
    if (a0 != nullptr) seen.push_back((uintptr_t)a0);
    if (a1 != nullptr) seen.push_back((uintptr_t)a1);
  }
  std::sort(seen.begin(), seen.end());
  HBK_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(),
              "%s: two columns name the same table or slot (a row stepped twice in one call would race)", kWho);

  hipStream_t stream = as_stream(stream_);
  const LowpRound round = {stochastic ? rounding->step : nullptr, stochastic ? rounding->seed : 0u};
  if (apply == HBK_APPLY_SGD) {
    rc = launch_lowp<LrParams>(n_cols, cols, shapes, nullptr, nullptr, round, stream,
                               [&](LowpArgs<LrParams>& a, unsigned blocks, hipStream_t s) {
                                 a.p = LrParams{lr};
                                 hipLaunchKernelGGL(lowp_apply_kernel<SgdRule>, dim3(blocks), dim3(kLowpBlock), 0, s, a);
                               });
  } else if (apply == HBK_APPLY_ADAGRAD) {
    rc = launch_lowp<LrParams>(n_cols, cols, shapes, slot0, nullptr, round, stream,
                               [&](LowpArgs<LrParams>& a, unsigned blocks, hipStream_t s) {
                                 a.p = LrParams{lr};
                                 hipLaunchKernelGGL(lowp_apply_kernel<AdagradRule>, dim3(blocks), dim3(kLowpBlock), 0,
                                                    s, a);
                               });
  } else if (apply == HBK_APPLY_LAZY_ADAM) {
    const hbk_adam_t* adam = static_cast<const hbk_adam_t*>(params);
    rc = launch_lowp<AdamParams>(n_cols, cols, shapes, slot0, slot1, round, stream,
                                 [&](LowpArgs<AdamParams>& a, unsigned blocks, hipStream_t s) {
                                   a.p = AdamParams{adam->beta_powers, lr, adam->beta1, adam->beta2, adam->epsilon};
                                   hipLaunchKernelGGL(lowp_apply_kernel<AdamRule>, dim3(blocks), dim3(kLowpBlock), 0,
                                                      s, a);
                                 });
    if (rc == HBK_OK && adam->finish) {
      hipLaunchKernelGGL(lowp_adam_finish_kernel, dim3(1), dim3(kWave), 0, stream, adam->beta_powers, adam->beta1,
                         adam->beta2);
      HBK_HIP_OK(hipGetLastError());
    }
  } else if (apply == HBK_APPLY_FTRL) {
    const hbk_ftrl_t* ftrl = static_cast<const hbk_ftrl_t*>(params);
    rc = launch_lowp<FtrlParams>(
        n_cols, cols, shapes, slot0, slot1, round, stream,
        [&](LowpArgs<FtrlParams>& a, unsigned blocks, hipStream_t s) {
          a.p = FtrlParams{lr, ftrl->l1, 2.0f * ftrl->l2, 2.0f * ftrl->l2_shrinkage, -ftrl->lr_power};
          // lr_power = -0.5 (TF's default) takes the sqrtf instantiation, any other the powf one
          if (ftrl->lr_power != -0.5f) {
            hipLaunchKernelGGL(lowp_apply_kernel<FtrlRule<true>>, dim3(blocks), dim3(kLowpBlock), 0, s, a);
          } else {
            hipLaunchKernelGGL(lowp_apply_kernel<FtrlRule<false>>, dim3(blocks), dim3(kLowpBlock), 0, s, a);
          }
        });
  } else {
    const hbk_rowwise_adagrad_t* opt = static_cast<const hbk_rowwise_adagrad_t*>(params);
    rc = launch_lowp<RowwiseParams>(n_cols, cols, shapes, slot0, nullptr, round, stream,
                                    [&](LowpArgs<RowwiseParams>& a, unsigned blocks, hipStream_t s) {
                                      a.p = RowwiseParams{lr, opt->epsilon};
                                      hipLaunchKernelGGL(lowp_apply_kernel<RowwiseAdagradRule>, dim3(blocks),
                                                         dim3(kLowpBlock), 0, s, a);
                                    });
  }
  if (rc != HBK_OK) return rc;
  if (stochastic && rounding->advance != 0) {
    hipLaunchKernelGGL(lowp_advance_kernel, dim3(1), dim3(kWave), 0, stream, rounding->step);
    HBK_HIP_OK(hipGetLastError());
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

extern "C" int hbk_lowp_apply_slices_n(int32_t n_cols, const hbk_lowp_slices_column_t* cols, int32_t apply,
                                       float* const* slot0, float* const* slot1, const void* params, float lr,
                                       const hbk_lowp_rounding_t* rounding, hbk_stream_t stream) {
  return hbk::lowp_apply_slices(n_cols, cols, apply, slot0, slot1, params, lr, rounding, stream);
}
