// Gradient of the group lookup with respect to the per-id weights (sp_weights):
// hbk_group_lookup_bwd_weights, and the requester side of hbk_sharded_lookup_bwd_weights.
//
// A grouped gather shaped like the forward (lookup_fwd.hip): one launch for all columns of the call, a
// row of `dim` floats owned by LPR = pow2(chunks) adjacent lanes, every id's row loaded once, clipped in
// registers as the clipped forward clips it, and dotted with the gradient row G_s of its segment:
//     d_j = <G_s, e_j>     A_s = sum w_i d_i     W_s = sum w_i     Q_s = sum w_i w_i
//     dw_j = d_j                                              (sum)
//          = (d_j - A_s / W_s) / W_s                          (mean)
//          = d_j / sqrtf(Q_s) - (w_j * A_s) / (Q_s * sqrtf(Q_s))   (sqrtn)
// The order of every fp32 operation is fixed by the row shape alone (include/hbk.h): the lane's chunk in
// element order, the group's lanes in a butterfly (both lanes of a pair add the same two values), the
// segment's ids in id order.  No atomics, no workspace.
//   * ragged columns: a lane group owns a segment whatever its length and walks its ids LPR at a time
//     (lane `sub` of the group owns id j0 + sub: ids, weights and results move as one coalesced access
//     per group).  A segment of at most LPR ids keeps its d_j in registers and writes dw once; one of up
//     to 8 LPR ids parks d_j, w_j and the validity in LDS until A_s is known (379 us against 473 for the
//     sweep on config 2 ragged: profiles/weight_grad.txt; option bwd_weights_lds); a longer one writes
//     d_j to dw first and fixes the values up in a second sweep over its own n floats.  Either way a
//     lane re-reads only what it wrote itself: no barrier, no fence;
//   * one id per segment (row_splits == NULL): no segment walk -- a wave takes 64 ids, one per lane,
//     every lane group dots one (row, G) pair per step, the result goes back to the id's lane.
#include <string.h>

#include <vector>

#include "lookup_common.h"

namespace hbk {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kMaxWCols = 64;     // WArgs travels by value (kernarg)
constexpr int kSegIters = 4;      // segments per lane group and wave (ragged)
constexpr int kRowPasses = 2;     // passes of 64 ids per wave (one id per segment)
constexpr int kLdsIds = 2048;     // ids a workgroup's lane groups park in LDS (9 bytes each: 18 KB), shared evenly:
                                  // 8 x LPR per lane group (32 ids for a row of 16 floats)

struct WCol {
  const float* table;       // rows of `pitch` floats (HALF: halves)
  const void* ids;
  const int32_t* splits;    // NULL: one id per segment
  const float* weights;
  const float* grad_out;
  float* dw;                // [n_ids]
  const int64_t* run_start; // RUNS: the table is n_runs runs of rows (the sharded step's received rows)
  const int64_t* run_base;
  IdMap map;
  int64_t n_seg;
  int32_t n_ids;
  int32_t pitch;
  int32_t grad_stride;
  int32_t chunks;
  int32_t n_runs;
  float max_norm;           // 0: not clipped
  uint8_t lpr_log2, ids64, combiner, vec4;
};

struct WArgs {
  int32_t n_cols;
  int32_t lds;   // != 0: segments of up to 8 x LPR ids park d_j in LDS (option bwd_weights_lds)
  int32_t tile0[kMaxWCols];
  WCol col[kMaxWCols];
};
static_assert(sizeof(WArgs) <= 16384, "kernarg budget");
static_assert(kMaxWCols <= kWave, "one lane's worth of columns in the tile search");
static_assert(kLdsIds == 8 * kBlock, "8 x LPR LDS entries per lane group");

template <bool RUNS>
__device__ inline uint64_t wrow_offset(const WCol& c, uint64_t r) {
  if (!RUNS) return r * (uint64_t)c.pitch;
  int k = 0;
  while (k + 1 < c.n_runs && (uint64_t)c.run_start[k + 1] <= r) ++k;
  return (uint64_t)c.run_base[k] + (r - (uint64_t)c.run_start[k]) * (uint64_t)c.pitch;
}

__device__ inline float chunk_dot(float g, float e) { return g * e; }
__device__ inline float chunk_dot(f32x4 g, f32x4 e) {
  return ((g.x * e.x + g.y * e.y) + g.z * e.z) + g.w * e.w;
}

// d = <G, e> over the lanes of a group: every lane ends with the same bits
template <typename V>
__device__ inline float group_dot(V g, V e, int lpr_log2) {
  float s = chunk_dot(g, e);
  for (int o = 1; o < (1 << lpr_log2); o <<= 1) s = s + __shfl_xor(s, o, kWave);
  return s;
}

__device__ inline float wgrad_final(int combiner, bool valid, float d, float w, float A, float W,
                                    float Q) {
  if (!valid) return 0.f;
  if (combiner == HBK_COMBINER_SUM) return d;
  if (combiner == HBK_COMBINER_MEAN) return W != 0.f ? (d - A / W) / W : 0.f;
  const float r = sqrtf(Q);
  return r != 0.f ? d / r - (w * A) / (Q * r) : 0.f;
}

// ---- ragged segments ---------------------------------------------------------------------------------
// lds_d / lds_w / lds_ok: this lane group's `cap` LDS entries (cap = 0: none).  A lane reads back only the
// entries it wrote itself -- entry e belongs to lane e % LPR in both sweeps -- so no barrier is needed.
template <typename V, bool RUNS, int HALF>
__device__ inline void wgrad_segments(const WCol& c, int64_t wave_seg0, float* lds_d, float* lds_w,
                                      uint8_t* lds_ok, int cap) {
  constexpr int VE = sizeof(V) / 4;
  const int lane = lane_id();
  const int lpr_log2 = c.lpr_log2;
  const int lpr = 1 << lpr_log2;
  const int rpi = kWave >> lpr_log2;
  const int sub = lane & (lpr - 1);
  const int grp = lane >> lpr_log2;
  const int grp_lane0 = grp << lpr_log2;
  const bool live = sub < c.chunks;
  const bool clip = c.max_norm > 0.f;
  const int combiner = c.combiner;

  for (int it = 0; it < kSegIters; ++it) {
    const int64_t s = wave_seg0 + (int64_t)it * rpi + grp;
    int32_t beg = 0, end = 0;
    if (s < c.n_seg) {
      beg = c.splits[s];
      end = c.splits[s + 1];
      beg = beg < 0 ? 0 : beg;                  // (never outside the column's [0, n_ids))
      end = end > c.n_ids ? c.n_ids : end;
    }
    V g = zero_v<V>();
    if (live && end > beg) {
      g = __builtin_nontemporal_load(
          reinterpret_cast<const V*>(c.grad_out + s * (int64_t)c.grad_stride + (int64_t)sub * VE));
    }
    const bool two_sweeps = combiner != HBK_COMBINER_SUM && end - beg > lpr;
    const bool parked = two_sweeps && end - beg <= cap;   // d_j, w_j and validity wait in LDS, not in dw
    float A = 0.f, W = 0.f, Q = 0.f;
    float myd = 0.f, myw = 0.f;
    uint64_t myrow = kNoRow;
    int32_t j0 = beg;
    if (j0 + sub < end) {
      myrow = id_to_row(c.map, load_id(c.ids, c.ids64, j0 + sub));
      myw = __builtin_nontemporal_load(c.weights + j0 + sub);
    }
    while (__any(j0 < end)) {
      // the next LPR ids while this chunk's rows are in flight
      uint64_t nextrow = kNoRow;
      float nextw = 0.f;
      const int32_t j1 = j0 + lpr;
      if (j1 + sub < end) {
        nextrow = id_to_row(c.map, load_id(c.ids, c.ids64, j1 + sub));
        nextw = __builtin_nontemporal_load(c.weights + j1 + sub);
      }
      const int32_t cnt = end - j0;   // ids of this group still to do (may be <= 0)
      for (int t0 = 0; t0 < lpr; t0 += 4) {
        V v[4];
        bool p[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int tt = t0 + t;
          const uint64_t r = shfl_u64(myrow, grp_lane0 + (tt & (lpr - 1)));
          p[t] = tt < lpr && tt < cnt && r != kNoRow;
          v[t] = zero_v<V>();
          if (p[t] && live) {
            v[t] = load_row_chunk<V, HALF>(c.table, wrow_offset<RUNS>(c, r) + (uint64_t)sub * VE);
          }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int tt = t0 + t;
          if (clip) v[t] = clip_row<V>(v[t], c.max_norm, lpr_log2);
          const float d = group_dot<V>(g, v[t], lpr_log2);
          const float w = __shfl(myw, grp_lane0 + (tt & (lpr - 1)), kWave);
          if (p[t]) {   // an invalid row adds neither term nor weight (as in the forward)
            A = A + w * d;
            W = W + w;
            Q = Q + w * w;
          }
          if (tt < lpr && tt < cnt && sub == tt) myd = p[t] ? d : 0.f;
        }
      }
      if (j0 + sub < end) {
        if (combiner == HBK_COMBINER_SUM) {
          __builtin_nontemporal_store(myd, c.dw + j0 + sub);
        } else if (parked) {
          const int e = j0 - beg + sub;
          lds_d[e] = myd;
          lds_w[e] = myw;
          lds_ok[e] = myrow != kNoRow;
        } else if (two_sweeps) {
          c.dw[j0 + sub] = myd;   // d_j (0 for an invalid row): fixed up below
        }
      }
      if (j1 < end || two_sweeps) {   // (a one-chunk segment keeps its registers for the write below)
        myrow = nextrow;
        myw = nextw;
      }
      j0 = j1;
    }
    if (combiner == HBK_COMBINER_SUM) continue;
    if (!two_sweeps) {
      if (beg + sub < end) {
        __builtin_nontemporal_store(wgrad_final(combiner, myrow != kNoRow, myd, myw, A, W, Q),
                                    c.dw + beg + sub);
      }
    } else if (parked) {
      for (int32_t j = beg + sub; j < end; j += lpr) {
        const int e = j - beg;   // this lane's own entry
        __builtin_nontemporal_store(wgrad_final(combiner, lds_ok[e] != 0, lds_d[e], lds_w[e], A, W, Q),
                                    c.dw + j);
      }
    } else {
      for (int32_t j = beg + sub; j < end; j += lpr) {
        const bool valid = id_to_row(c.map, load_id(c.ids, c.ids64, j)) != kNoRow;
        const float w = c.weights[j];
        const float d = c.dw[j];   // this lane's own store
        c.dw[j] = wgrad_final(combiner, valid, d, w, A, W, Q);
      }
    }
  }
}

// ---- one id per segment ------------------------------------------------------------------------------
template <typename V, bool RUNS, int HALF>
__device__ inline void wgrad_rows(const WCol& c, int64_t wave_row0) {
  constexpr int VE = sizeof(V) / 4;
  const int lane = lane_id();
  const int lpr_log2 = c.lpr_log2;
  const int lpr = 1 << lpr_log2;
  const int rpi = kWave >> lpr_log2;
  const int sub = lane & (lpr - 1);
  const int grp = lane >> lpr_log2;
  const bool live = sub < c.chunks;
  const bool clip = c.max_norm > 0.f;
  const int my_step = lane >> (6 - lpr_log2);          // the step in which this lane's id is dotted
  const int my_src = (lane & (rpi - 1)) << lpr_log2;   // first lane of the group that dots it

  for (int pass = 0; pass < kRowPasses; ++pass) {
    const int64_t base = wave_row0 + (int64_t)pass * kWave;
    if (base >= c.n_seg) break;   // uniform
    const int64_t s = base + lane;
    uint64_t myrow = kNoRow;
    float myw = 0.f, myd = 0.f;
    if (s < c.n_seg) {
      myrow = id_to_row(c.map, load_id(c.ids, c.ids64, s));
      myw = __builtin_nontemporal_load(c.weights + s);
    }
    for (int u0 = 0; u0 < lpr; u0 += 4) {
      V v[4], g[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int u = u0 + t;
        const int q = (u * rpi + grp) & (kWave - 1);   // the id of this group in step u
        const uint64_t r = shfl_u64(myrow, q);
        v[t] = zero_v<V>();
        g[t] = zero_v<V>();
        if (u < lpr && r != kNoRow && live) {
          v[t] = load_row_chunk<V, HALF>(c.table, wrow_offset<RUNS>(c, r) + (uint64_t)sub * VE);
          g[t] = __builtin_nontemporal_load(reinterpret_cast<const V*>(
              c.grad_out + (base + q) * (int64_t)c.grad_stride + (int64_t)sub * VE));
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int u = u0 + t;
        if (clip) v[t] = clip_row<V>(v[t], c.max_norm, lpr_log2);
        const float d = group_dot<V>(g[t], v[t], lpr_log2);
        const float got = __shfl(d, my_src, kWave);
        if (my_step == u) myd = got;
      }
    }
    if (s < c.n_seg) {
      // the segment is the id alone: A = w d, W = w, Q = w w
      __builtin_nontemporal_store(
          wgrad_final(c.combiner, myrow != kNoRow, myd, myw, myw * myd, myw, myw * myw), c.dw + s);
    }
  }
}

template <bool CSR, typename V, bool RUNS, int HALF>
__global__ __launch_bounds__(kBlock) void group_lookup_bwd_weights_kernel(const WArgs a) {
  const int l = lane_id();
  const int t0 = l < a.n_cols ? a.tile0[l] : 0x7fffffff;
  int ci = (int)__builtin_popcountll(__ballot(t0 <= (int)blockIdx.x)) - 1;
  ci = __builtin_amdgcn_readfirstlane(ci);
  const WCol& c = a.col[ci];
  const int64_t tile = (int)blockIdx.x - a.tile0[ci];
  const int wave = (int)(threadIdx.x >> 6);
  if (!CSR) {
    const int64_t row0 = (tile * kWavesPerBlock + wave) * (int64_t)(kRowPasses * kWave);
    if (row0 >= c.n_seg) return;
    wgrad_rows<V, RUNS, HALF>(c, row0);
  } else {
    if (tile == 0) {
      // ids in no segment (before the first split, behind the last): every position is written
      const int32_t first = c.splits[0] < c.n_ids ? c.splits[0] : c.n_ids;
      const int32_t last = c.splits[c.n_seg] > 0 ? c.splits[c.n_seg] : 0;
      for (int32_t j = (int32_t)threadIdx.x; j < first; j += kBlock) c.dw[j] = 0.f;
      for (int32_t j = last + (int32_t)threadIdx.x; j < c.n_ids; j += kBlock) c.dw[j] = 0.f;
    }
    const int rpi = kWave >> c.lpr_log2;
    const int64_t seg0 = (tile * kWavesPerBlock + wave) * (int64_t)(kSegIters * rpi);
    if (seg0 >= c.n_seg) return;
    __shared__ float lds_d[kLdsIds];
    __shared__ float lds_w[kLdsIds];
    __shared__ uint8_t lds_ok[kLdsIds];
    const int cap = a.lds != 0 ? 8 << c.lpr_log2 : 0;   // kLdsIds over the kBlock >> lpr_log2 lane groups
    const int at = (int)(threadIdx.x >> c.lpr_log2) * (8 << c.lpr_log2);
    wgrad_segments<V, RUNS, HALF>(c, seg0, lds_d + at, lds_w + at, lds_ok + at, cap);
  }
}

template <bool CSR, typename V>
void launch_table(int table_kind, const WArgs& args, unsigned tiles, hipStream_t stream) {
  switch (table_kind) {
    case 0:
      hipLaunchKernelGGL((group_lookup_bwd_weights_kernel<CSR, V, false, 0>), dim3(tiles), dim3(kBlock), 0,
                         stream, args);
      return;
    case 1:
      hipLaunchKernelGGL((group_lookup_bwd_weights_kernel<CSR, V, true, 0>), dim3(tiles), dim3(kBlock), 0,
                         stream, args);
      return;
    default:
      hipLaunchKernelGGL((group_lookup_bwd_weights_kernel<CSR, V, true, 2>), dim3(tiles), dim3(kBlock), 0,
                         stream, args);
      return;
  }
}

// kind: bit 0 ragged, bit 1 scalar chunks, bits 2.. the table (0 plain, 1 runs, 2 runs of fp16 rows)
void launch_kind(int kind, const WArgs& args, unsigned tiles, hipStream_t stream) {
  switch (kind & 3) {
    case 0: launch_table<false, f32x4>(kind >> 2, args, tiles, stream); return;
    case 1: launch_table<true, f32x4>(kind >> 2, args, tiles, stream); return;
    case 2: launch_table<false, float>(kind >> 2, args, tiles, stream); return;
    default: launch_table<true, float>(kind >> 2, args, tiles, stream); return;
  }
}
constexpr int kWKinds = 12;

}  // namespace

// Checks every column, then launches; a refused call has launched nothing.
int group_lookup_bwd_weights(int32_t n_cols, const WeightGradColumn* cols, hipStream_t stream) {
  HBK_REQUIRE(n_cols >= 0, "group_lookup_bwd_weights: n_cols must be >= 0, got %d", n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "group_lookup_bwd_weights: cols is NULL");
  struct Classified {
    RowShape shape;
    int kind;   // -1: nothing to launch
  };
  std::vector<Classified> cls((size_t)(n_cols > 0 ? n_cols : 1));
  bool present[kWKinds] = {};
  for (int32_t c = 0; c < n_cols; ++c) {
    const WeightGradColumn& h = cols[c];
    cls[c].kind = -1;
    if (h.grad_weights == nullptr) continue;
    HBK_REQUIRE(h.id_weights != nullptr,
                "group_lookup_bwd_weights: column %d: a weight gradient is wanted but the column has no "
                "id_weights", c);
    HBK_REQUIRE(h.dim >= 1 && h.dim <= 1024, "group_lookup_bwd_weights: column %d: dim %d outside 1 .. 1024",
                c, h.dim);
    HBK_REQUIRE(h.rows >= 0 && h.n_ids >= 0 && h.n_segments >= 0,
                "group_lookup_bwd_weights: column %d: negative size", c);
    HBK_REQUIRE(h.n_ids < (1ll << 30) && h.n_segments < (1ll << 30),
                "group_lookup_bwd_weights: column %d: more than 2^30-1 ids / segments", c);
    HBK_REQUIRE(h.ids_dtype == HBK_INT32 || h.ids_dtype == HBK_INT64,
                "group_lookup_bwd_weights: column %d: ids must be int32 or int64", c);
    HBK_REQUIRE(h.bucket >= 0 && h.divisor >= 1, "group_lookup_bwd_weights: column %d: bad bucket/divisor", c);
    HBK_REQUIRE(h.combiner >= HBK_COMBINER_SUM && h.combiner <= HBK_COMBINER_SQRTN,
                "group_lookup_bwd_weights: column %d: unknown combiner %d", c, h.combiner);
    HBK_REQUIRE(h.row_splits != nullptr || h.n_segments == h.n_ids,
                "group_lookup_bwd_weights: column %d: n_segments must equal n_ids when row_splits is NULL",
                c);
    HBK_REQUIRE(h.n_ids == 0 || (h.ids && h.grad_out && (h.table || h.rows == 0)),
                "group_lookup_bwd_weights: column %d: NULL buffer", c);
    HBK_REQUIRE(h.table_pitch == 0 || h.table_pitch >= h.dim,
                "group_lookup_bwd_weights: column %d: table_pitch %d is smaller than dim %d", c,
                h.table_pitch, h.dim);
    HBK_REQUIRE(h.grad_stride == 0 || h.grad_stride >= h.dim,
                "group_lookup_bwd_weights: column %d: grad_stride %d is smaller than dim %d", c,
                h.grad_stride, h.dim);
    HBK_REQUIRE(h.n_runs >= 0 && (h.n_runs == 0 || (h.run_start && h.run_base)),
                "group_lookup_bwd_weights: column %d: bad segmented-table description", c);
    HBK_REQUIRE(h.max_norm >= 0.0f && h.max_norm <= 3.402823466e38f,
                "group_lookup_bwd_weights: column %d: max_norm must be 0 (no clip) or finite and > 0, got %g",
                c, (double)h.max_norm);
    HBK_REQUIRE(!h.table_half || (h.n_runs > 0 && h.max_norm == 0.0f),
                "group_lookup_bwd_weights: column %d: fp16 rows need a segmented table and no clip", c);
    if (h.n_ids == 0) continue;
    const int32_t pitch = h.table_pitch > 0 ? h.table_pitch : h.dim;
    const int32_t gstride = h.grad_stride > 0 ? h.grad_stride : h.dim;
    // (a half buffer is held to 8 bytes where an fp32 one is held to 16, as in the forward)
    const uintptr_t bits = (uintptr_t)h.table * (h.table_half ? 2 : 1) | (uintptr_t)h.grad_out |
                           ((uintptr_t)(uint32_t)pitch * 4) | ((uintptr_t)(uint32_t)gstride * 4);
    HBK_REQUIRE(make_rowshape(h.dim, bits, &cls[c].shape),
                "group_lookup_bwd_weights: column %d: dim %d needs more than 64 lanes per row (unaligned or "
                "dim %% 4 != 0 with dim > 64 is unsupported)", c, h.dim);
    cls[c].kind = (h.row_splits != nullptr ? 1 : 0) | (cls[c].shape.vec4 ? 0 : 2) |
                  (h.n_runs > 0 ? (h.table_half ? 8 : 4) : 0);
    if (h.n_segments > 0) present[cls[c].kind] = true;
  }
  {
    const int rc = sync_check("group_lookup_bwd_weights", stream);
    if (rc != HBK_OK) return rc;
  }
  // ids in no segment at all (a column without segments): zeros
  for (int32_t c = 0; c < n_cols; ++c) {
    if (cls[c].kind >= 0 && cols[c].n_segments == 0) {
      HBK_HIP_OK(hipMemsetAsync(cols[c].grad_weights, 0, (size_t)cols[c].n_ids * 4, stream));
    }
  }
  for (int kind = 0; kind < kWKinds; ++kind) {
    if (!present[kind]) continue;
    int32_t c0 = 0;
    while (c0 < n_cols) {
      WArgs args;
      args.lds = options().bwd_weights_lds;
      int32_t k = 0;
      int64_t tiles = 0;
      while (c0 < n_cols && k < kMaxWCols) {
        const int32_t ci = c0++;
        const WeightGradColumn& h = cols[ci];
        if (cls[ci].kind != kind || h.n_segments == 0) continue;
        WCol& d = args.col[k];
        d.table = h.table;
        d.ids = h.ids;
        d.splits = h.row_splits;
        d.weights = h.id_weights;
        d.grad_out = h.grad_out;
        d.dw = h.grad_weights;
        d.run_start = h.run_start;
        d.run_base = h.run_base;
        d.map = make_idmap(h.bucket, h.divisor, h.rows);
        d.n_seg = h.n_segments;
        d.n_ids = (int32_t)h.n_ids;
        d.pitch = h.table_pitch > 0 ? h.table_pitch : h.dim;
        d.grad_stride = h.grad_stride > 0 ? h.grad_stride : h.dim;
        d.chunks = cls[ci].shape.chunks;
        d.n_runs = h.n_runs;
        d.max_norm = h.max_norm;
        d.lpr_log2 = cls[ci].shape.lpr_log2;
        d.ids64 = h.ids_dtype == HBK_INT64;
        d.combiner = (uint8_t)h.combiner;
        d.vec4 = cls[ci].shape.vec4;
        const int64_t per_block =
            h.row_splits != nullptr ? kWavesPerBlock * kSegIters * (int64_t)(kWave >> d.lpr_log2)
                                    : kWavesPerBlock * kRowPasses * (int64_t)kWave;
        args.tile0[k] = (int32_t)tiles;
        tiles += (h.n_segments + per_block - 1) / per_block;
        HBK_REQUIRE(tiles < (1ll << 31), "group_lookup_bwd_weights: grid too large");
        ++k;
      }
      if (k == 0) continue;
      args.n_cols = k;
      launch_kind(kind, args, (unsigned)tiles, stream);
      HBK_HIP_OK(hipGetLastError());
    }
  }
  return HBK_OK;
}

}  // namespace hbk

extern "C" int hbk_group_lookup_bwd_weights(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                            const float* max_norms, float* const* grad_weights,
                                            hbk_stream_t stream) {
  using namespace hbk;
  HBK_REQUIRE(n_cols >= 0, "group_lookup_bwd_weights: n_cols must be >= 0, got %d", n_cols);
  HBK_REQUIRE(n_cols == 0 || (cols != nullptr && grad_weights != nullptr),
              "group_lookup_bwd_weights: NULL argument array");
  std::vector<WeightGradColumn> v((size_t)n_cols);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_lookup_grad_column_t& h = cols[c];
    memset(&v[c], 0, sizeof(v[c]));
    if (grad_weights[c] == nullptr) continue;   // not wanted: the column is skipped, unread
    HBK_REQUIRE(h.n_runs == 0,
                "group_lookup_bwd_weights: column %d: segmented inputs (n_runs > 0) are not supported", c);
    const float mn = max_norms != nullptr ? max_norms[c] : 0.0f;
    HBK_REQUIRE(mn >= 0.0f && mn <= 3.402823466e38f,
                "group_lookup_bwd_weights: column %d: max_norm must be 0 (no clip) or finite and > 0, got %g",
                c, (double)mn);
    WeightGradColumn& d = v[c];
    d.table = h.table;
    d.rows = h.rows;
    d.dim = h.dim;
    d.table_pitch = h.table_pitch;
    d.ids_dtype = h.ids_dtype;
    d.ids = h.ids;
    d.n_ids = h.n_ids;
    d.row_splits = h.row_splits;
    d.n_segments = h.n_segments;
    d.bucket = h.bucket;
    d.divisor = h.divisor;
    d.combiner = h.combiner;
    d.grad_out = h.grad_out;
    d.grad_stride = h.grad_stride;
    d.id_weights = h.id_weights;
    d.max_norm = mn;
    d.grad_weights = grad_weights[c];
  }
  return group_lookup_bwd_weights(n_cols, v.data(), as_stream(stream));
}
