// Sequence lookups (hbk_group_lookup_fwd_sequence, hbk_sequence_row_grid_n, hbk_sequence_id_grid_n): a ragged id list WITHOUT a
// combiner -- the first T ids of every sample gathered into padded [B, T, dim] rows, with the lengths and
// the bucketized id grid the backward reduces (include/hbk.h; replaces tf.sparse.slice +
// tf.sparse.to_dense + FloorMod + GatherV2 of docs/tutorial/ranking/data.py:195-224).
//
// The conventions of lookup_fwd.hip: one launch for the columns of a kind, found by a ballot over the tile
// prefix in the kernel arguments; a row is owned by 1 << lpr_log2 adjacent lanes that move one chunk each
// (16 bytes, or 4 bytes for odd dims / unaligned buffers); ids are read once per wave, one per lane,
// coalesced and non-temporal, and handed to the row's lanes by shuffle; kU row loads in flight per lane;
// non-temporal stores.  One unit of work is a RUN OF CONSECUTIVE POSITIONS p = b * T + t of the flattened
// grid: the rows of a sample are contiguous in `out`, so neighbouring lane groups write neighbouring rows
// (dim 16: a wave instruction stores 16 rows = 1 KB in one piece, whole 128-byte lines -- DESIGN.md 4.1 on
// what half-line requests cost).  b = p / T by FastDiv; a sample's two row splits are read by the first
// of its lanes in the wave and taken by the others with a shuffle: no search over row_splits.
#include <string.h>

#include <vector>

#include "lookup_common.h"

namespace hbk {
namespace {

constexpr int kBlock = 256;           // 4 waves
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kMaxColsPerLaunch = 64; // one ballot finds the column; SeqArgs travels by value
constexpr int kU = 2;                 // independent row loads per lane, as the forward's gather

struct SeqCol {
  const float* table;
  const void* ids;
  const int32_t* splits;   // NULL: one id per sample
  float* out;
  int64_t* grid;           // NULL: not wanted
  int32_t* lengths;        // NULL: not wanted
  int64_t n_pos;           // B * T
  int64_t n_ids;
  IdMap map;
  FastDiv max_len;         // T
  uint64_t pad_row;        // what a padding position looks up (kNoRow: nothing, a zero row)
  int64_t pad_grid;        // and its grid word (-1: nothing)
  int64_t out_stride;      // floats between samples (>= T * dim)
  int32_t dim;
  int32_t chunks;
  float max_norm;          // the clipped instantiations
  uint8_t lpr_log2;
  uint8_t ids64;
};

struct SeqArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  SeqCol col[kMaxColsPerLaunch];
};
static_assert(sizeof(SeqArgs) <= 24576, "kernarg budget");

// id -> (table row, grid word): id_to_row (lookup_common.h) with the bucketized id kept.  The grid word is
// what the backward's id_to_row, with bucket 0, maps to the same row: -1 where nothing is looked up.
__host__ __device__ inline uint64_t seq_map(const IdMap& m, int64_t id, int64_t* grid) {
  uint64_t r;
  if (m.bucket.d != 0) {
    r = floormod_i64(id, m.bucket);
  } else {
    if (id < 0) {
      *grid = -1;
      return kNoRow;
    }
    r = (uint64_t)id;
  }
  *grid = (int64_t)r;
  r = fastdiv(r, m.div);
  return r < m.rows ? r : kNoRow;
}

// The sample side of position p: t = p - b * T, the index of the sample's first id and L_b = min(len_b, T),
// the sample's length written by its first position.  False for a lane without a position.  The lanes of a
// wave hold CONSECUTIVE positions (lane l: p - l is lane 0's), valid ones first; every lane of the wave calls
// this.  The first lane of each sample inside the wave (t == 0, or lane 0) reads the sample's two row splits,
// the sample's other lanes take them by shuffle.
__device__ inline bool seq_sample(const SeqCol& c, int64_t p, bool valid, int64_t* t_out, int32_t* beg_out,
                                  int64_t* len_out) {
  const int lane = lane_id();
  const int64_t T = (int64_t)c.max_len.d;
  int64_t b = 0, t = 0;
  if (valid) {
    b = (int64_t)fastdiv((uint64_t)p, c.max_len);
    t = p - b * T;
  }
  int32_t beg = 0, end = 0;
  if (valid && (t == 0 || lane == 0)) {
    if (c.splits != nullptr) {
      beg = c.splits[b];
      end = c.splits[b + 1];
    } else {
      beg = (int32_t)b;
      end = (int32_t)b + 1;
    }
  }
  const int src = lane - (int)(t < lane ? t : lane);
  beg = __shfl(beg, src, kWave);
  end = __shfl(end, src, kWave);
  if (!valid) return false;
  int64_t len = (int64_t)end - (int64_t)beg;
  len = len < 0 ? 0 : (len > T ? T : len);
  if (t == 0 && c.lengths != nullptr) c.lengths[b] = (int32_t)len;
  *t_out = t;
  *beg_out = beg;
  *len_out = len;
  return true;
}

// Position p of the column's grid -> its row, and the grid word written (every lane of the wave calls this)
__device__ inline uint64_t seq_position(const SeqCol& c, int64_t p, bool valid) {
  int64_t t, len;
  int32_t beg;
  if (!seq_sample(c, p, valid, &t, &beg, &len)) return kNoRow;
  uint64_t row = c.pad_row;
  int64_t g = c.pad_grid;
  if (t < len) {
    const int64_t j = (int64_t)beg + t;
    row = kNoRow;
    g = -1;
    // (row splits that point outside the ids look nothing up)
    if ((uint64_t)j < (uint64_t)c.n_ids) row = seq_map(c.map, load_id(c.ids, c.ids64, j), &g);
  }
  if (c.grid != nullptr) __builtin_nontemporal_store(g, c.grid + p);
  return row;
}

// kU * rpi consecutive positions per wave: slot q lives in register q >> 6 of lane q & 63
template <typename V, bool CLIP>
__global__ __launch_bounds__(kBlock) void sequence_lookup_fwd_kernel(const SeqArgs a) {
  constexpr int VE = sizeof(V) / 4;
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const SeqCol& c = a.col[ci];
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int lpr_log2 = c.lpr_log2;
  const int rpi = kWave >> lpr_log2;  // rows per wave instruction
  const int sub = lane & ((1 << lpr_log2) - 1);
  const int grp = lane >> lpr_log2;
  const int n_slots = kU * rpi;
  const int64_t pos0 = ((int64_t)(b - a.tile_start[ci]) * kWavesPerBlock + wave) * (int64_t)n_slots;
  if (pos0 >= c.n_pos) return;   // (wave-uniform)

  uint64_t rowreg[kU];
#pragma unroll
  for (int k = 0; k < kU; ++k) {
    const int q = k * kWave + lane;
    const int64_t p = pos0 + q;
    rowreg[k] = seq_position(c, p, q < n_slots && p < c.n_pos);
  }

  V v[kU];
  const bool live = sub < c.chunks;
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int q0 = u * rpi;  // a multiple of rpi (a power of two <= 64): q0 >> 6 is uniform
    const int k = q0 >> 6;
    uint64_t src = rowreg[0];
#pragma unroll
    for (int kk = 1; kk < kU; ++kk) src = (k == kk) ? rowreg[kk] : src;
    const uint64_t r = shfl_u64(src, (q0 & (kWave - 1)) + grp);
    v[u] = zero_v<V>();
    if (live && r != kNoRow) {
      v[u] = load_row_chunk<V, 0>(c.table, r * (uint64_t)c.dim + (uint64_t)sub * VE);
    }
    if (CLIP) v[u] = clip_row<V>(v[u], c.max_norm, lpr_log2);
  }
  const int64_t T = (int64_t)c.max_len.d;
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int64_t p = pos0 + u * rpi + grp;
    if (live && p < c.n_pos) {
      const int64_t s = (int64_t)fastdiv((uint64_t)p, c.max_len);
      const int64_t off = s * c.out_stride + (p - s * T) * (int64_t)c.dim + (int64_t)sub * VE;
      __builtin_nontemporal_store(v[u], reinterpret_cast<V*>(c.out + off));
    }
  }
}

// the grid and the lengths alone: one thread per position
__global__ __launch_bounds__(kBlock) void sequence_row_grid_kernel(const SeqArgs a) {
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const SeqCol& c = a.col[ci];
  const int64_t p = (int64_t)(b - a.tile_start[ci]) * kBlock + (int64_t)threadIdx.x;
  seq_position(c, p, p < c.n_pos);
}

// the RAW-id grid (hbk_sequence_id_grid_n): the same position arithmetic, the effective ids themselves -- never
// bucketized, negative ones kept, pad_grid (= pad_id) past a sample's length.  One thread per position: a wave
// stores 64 consecutive words, 512 bytes in whole lines; the ids of a sample are consecutive too.
__global__ __launch_bounds__(kBlock) void sequence_id_grid_kernel(const SeqArgs a) {
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const SeqCol& c = a.col[ci];
  const int64_t p = (int64_t)(b - a.tile_start[ci]) * kBlock + (int64_t)threadIdx.x;
  int64_t t, len;
  int32_t beg;
  if (!seq_sample(c, p, p < c.n_pos, &t, &beg, &len)) return;
  int64_t g = c.pad_grid;
  if (t < len) {
    const int64_t j = (int64_t)beg + t;
    // (row splits that point outside the ids read nothing: such a position holds the pad id)
    if ((uint64_t)j < (uint64_t)c.n_ids) g = load_id(c.ids, c.ids64, j);
  }
  __builtin_nontemporal_store(g, c.grid + p);
}

template <typename V, bool CLIP>
void launch_sequence(const SeqArgs& args, unsigned tiles, hipStream_t stream) {
  hipLaunchKernelGGL((sequence_lookup_fwd_kernel<V, CLIP>), dim3(tiles), dim3(kBlock), 0, stream, args);
}

constexpr int kGridKind = 4;   // kinds 0..3: bit 0 4-byte chunks, bit 1 clipped; 4: grid only

// both entries: `gather` false = hbk_sequence_row_grid_n (no table, no output, no row shape)
int sequence_fwd(const char* who, bool gather, int32_t n_cols, const hbk_lookup_column_t* cols,
                 const hbk_sequence_t* seq, const float* max_norms, hbk_stream_t stream) {
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(n_cols == 0 || seq != nullptr, "%s: seq is NULL", who);
  struct Classified {
    RowShape shape;
    int kind;   // -1: nothing to do (no samples)
  };
  std::vector<Classified> cls((size_t)(n_cols > 0 ? n_cols : 1));
  bool kinds_present[kGridKind + 1] = {};
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_lookup_column_t& h = cols[c];
    const hbk_sequence_t& q = seq[c];
    HBK_REQUIRE(q.max_len >= 1, "%s: column %d: max_len must be >= 1, got %d", who, c, q.max_len);
    HBK_REQUIRE(h.id_weights == nullptr, "%s: column %d: id_weights are not supported on sequence columns",
                who, c);
    HBK_REQUIRE(h.out_slots == nullptr, "%s: column %d: out_slots are not supported on sequence columns",
                who, c);
    HBK_REQUIRE(h.half_io == 0, "%s: column %d: half_io %d: sequence columns read and write fp32 rows", who,
                c, h.half_io);
    HBK_REQUIRE(h.n_runs == 0, "%s: column %d: n_runs %d: sequence columns take a plain table", who, c,
                h.n_runs);
    HBK_REQUIRE(h.rows >= 0 && h.n_ids >= 0 && h.n_segments >= 0, "%s: column %d: negative size", who, c);
    HBK_REQUIRE(h.ids_dtype == HBK_INT32 || h.ids_dtype == HBK_INT64,
                "%s: column %d: ids must be int32 or int64", who, c);
    HBK_REQUIRE(h.bucket >= 0, "%s: column %d: bucket must be >= 0", who, c);
    HBK_REQUIRE(h.divisor >= 1, "%s: column %d: divisor must be >= 1", who, c);
    HBK_REQUIRE(h.row_splits != nullptr || h.n_segments == h.n_ids,
                "%s: column %d: n_segments (%lld) must equal n_ids (%lld) when row_splits is NULL", who, c,
                (long long)h.n_segments, (long long)h.n_ids);
    HBK_REQUIRE(h.n_ids < (1ll << 31), "%s: column %d: more than 2^31-1 ids", who, c);
    HBK_REQUIRE(h.n_segments < (1ll << 31) && h.n_segments * (int64_t)q.max_len < (1ll << 31),
                "%s: column %d: B * T = %lld x %d positions, must stay below 2^31", who, c,
                (long long)h.n_segments, q.max_len);
    if (gather) {
      HBK_REQUIRE(h.dim >= 1 && h.dim <= 1024, "%s: column %d: dim must be in [1, 1024], got %d", who, c,
                  h.dim);
      const float x = max_norms != nullptr ? max_norms[c] : 0.0f;
      HBK_REQUIRE(x >= 0.0f && x <= 3.402823466e38f,
                  "%s: column %d: max_norm must be 0 (no clip) or finite and > 0, got %g", who, c, (double)x);
    }
    cls[c].kind = -1;
    if (h.n_segments == 0) continue;
    HBK_REQUIRE(h.ids != nullptr || h.n_ids == 0, "%s: column %d: NULL buffer", who, c);
    if (!gather) {
      cls[c].kind = kGridKind;
      kinds_present[kGridKind] = true;
      continue;
    }
    HBK_REQUIRE((h.table != nullptr || h.rows == 0) && h.out != nullptr, "%s: column %d: NULL buffer", who, c);
    const int64_t sample = (int64_t)q.max_len * h.dim;
    HBK_REQUIRE(sample < (1ll << 31) && (h.out_stride == 0 || h.out_stride >= sample),
                "%s: column %d: out_stride %d is smaller than max_len * dim = %lld floats (or that exceeds "
                "2^31-1)", who, c, h.out_stride, (long long)sample);
    const uintptr_t bits = (uintptr_t)h.table | (uintptr_t)h.out | ((uintptr_t)(uint32_t)h.out_stride * 4);
    HBK_REQUIRE(make_rowshape(h.dim, bits, &cls[c].shape),
                "%s: column %d: dim %d needs more than 64 lanes per row (unaligned or dim %% 4 != 0 with "
                "dim > 64 is unsupported)", who, c, h.dim);
    cls[c].kind = (cls[c].shape.vec4 ? 0 : 1) | (max_norms != nullptr && max_norms[c] != 0.0f ? 2 : 0);
    kinds_present[cls[c].kind] = true;
  }
  for (int kind = 0; kind <= kGridKind; ++kind) {
    if (!kinds_present[kind]) continue;
    int32_t c0 = 0;
    while (c0 < n_cols) {
      SeqArgs args;
      int32_t k = 0;
      int64_t tiles = 0;
      args.tile_start[0] = 0;
      while (c0 < n_cols && k < kMaxColsPerLaunch) {
        const int32_t ci = c0++;
        if (cls[ci].kind != kind) continue;
        const hbk_lookup_column_t& h = cols[ci];
        const hbk_sequence_t& q = seq[ci];
        SeqCol& d = args.col[k];
        d.table = h.table;
        d.ids = h.ids;
        d.splits = h.row_splits;
        d.out = h.out;
        d.grid = q.row_grid;
        d.lengths = q.lengths;
        d.n_pos = h.n_segments * (int64_t)q.max_len;
        d.n_ids = h.n_ids;
        d.map = make_idmap(h.bucket, h.divisor, h.rows);
        d.max_len = make_fastdiv((uint64_t)q.max_len);
        d.pad_row = kNoRow;
        d.pad_grid = -1;
        if (q.has_pad != 0) d.pad_row = seq_map(d.map, q.pad_id, &d.pad_grid);
        d.out_stride = h.out_stride > 0 ? h.out_stride : (int64_t)q.max_len * h.dim;
        d.dim = h.dim;
        d.chunks = gather ? cls[ci].shape.chunks : 0;
        d.lpr_log2 = gather ? cls[ci].shape.lpr_log2 : 0;
        d.max_norm = (kind & 2) != 0 && gather ? max_norms[ci] : 0.0f;
        d.ids64 = h.ids_dtype == HBK_INT64;
        const int64_t per_block =
            gather ? (int64_t)kWavesPerBlock * (kWave >> d.lpr_log2) * kU : (int64_t)kBlock;
        tiles += (d.n_pos + per_block - 1) / per_block;
        HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
        ++k;
        args.tile_start[k] = (int32_t)tiles;
      }
      if (k == 0) continue;
      args.n_cols = k;
      hipStream_t s = as_stream(stream);
      switch (kind) {
        case 0: launch_sequence<f32x4, false>(args, (unsigned)tiles, s); break;
        case 1: launch_sequence<float, false>(args, (unsigned)tiles, s); break;
        case 2: launch_sequence<f32x4, true>(args, (unsigned)tiles, s); break;
        case 3: launch_sequence<float, true>(args, (unsigned)tiles, s); break;
        default:
          hipLaunchKernelGGL(sequence_row_grid_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, s, args);
          break;
      }
      HBK_HIP_OK(hipGetLastError());
    }
  }
  return HBK_OK;
}

// hbk_sequence_id_grid_n: one launch per kMaxColsPerLaunch columns, tiled as the row-grid kernel tiles
int sequence_id_grid(int32_t n_cols, const hbk_lookup_column_t* cols, const hbk_sequence_t* seq,
                     hbk_stream_t stream) {
  const char* who = "sequence_id_grid_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(n_cols == 0 || seq != nullptr, "%s: seq is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_lookup_column_t& h = cols[c];
    const hbk_sequence_t& q = seq[c];
    HBK_REQUIRE(q.max_len >= 1, "%s: column %d: max_len must be >= 1, got %d", who, c, q.max_len);
    HBK_REQUIRE(q.has_pad != 0, "%s: column %d: has_pad is 0: every int64 is an id, so a raw-id grid has no value "
                "for a position that holds nothing -- give a pad_id", who, c);
    HBK_REQUIRE(q.row_grid != nullptr, "%s: column %d: row_grid is NULL", who, c);
    HBK_REQUIRE(h.n_ids >= 0 && h.n_segments >= 0, "%s: column %d: negative size", who, c);
    HBK_REQUIRE(h.ids_dtype == HBK_INT32 || h.ids_dtype == HBK_INT64,
                "%s: column %d: ids must be int32 or int64", who, c);
    HBK_REQUIRE(h.row_splits != nullptr || h.n_segments == h.n_ids,
                "%s: column %d: n_segments (%lld) must equal n_ids (%lld) when row_splits is NULL", who, c,
                (long long)h.n_segments, (long long)h.n_ids);
    HBK_REQUIRE(h.n_ids < (1ll << 31), "%s: column %d: more than 2^31-1 ids", who, c);
    HBK_REQUIRE(h.n_segments < (1ll << 31) && h.n_segments * (int64_t)q.max_len < (1ll << 31),
                "%s: column %d: B * T = %lld x %d positions, must stay below 2^31", who, c,
                (long long)h.n_segments, q.max_len);
    HBK_REQUIRE(h.n_segments == 0 || h.ids != nullptr || h.n_ids == 0, "%s: column %d: NULL buffer", who, c);
  }
  int32_t c0 = 0;
  while (c0 < n_cols) {
    SeqArgs args;
    int32_t k = 0;
    int64_t tiles = 0;
    args.tile_start[0] = 0;
    while (c0 < n_cols && k < kMaxColsPerLaunch) {
      const int32_t ci = c0++;
      const hbk_lookup_column_t& h = cols[ci];
      const hbk_sequence_t& q = seq[ci];
      if (h.n_segments == 0) continue;
      SeqCol& d = args.col[k];
      memset(&d, 0, sizeof(d));
      d.ids = h.ids;
      d.splits = h.row_splits;
      d.grid = q.row_grid;
      d.lengths = q.lengths;
      d.n_pos = h.n_segments * (int64_t)q.max_len;
      d.n_ids = h.n_ids;
      d.max_len = make_fastdiv((uint64_t)q.max_len);
      d.pad_grid = q.pad_id;
      d.ids64 = h.ids_dtype == HBK_INT64;
      tiles += (d.n_pos + kBlock - 1) / kBlock;
      HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
      ++k;
      args.tile_start[k] = (int32_t)tiles;
    }
    if (k == 0) continue;
    args.n_cols = k;
    hipLaunchKernelGGL(sequence_id_grid_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, as_stream(stream), args);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_sequence_id_grid_n(int32_t n_cols, const hbk_lookup_column_t* cols,
                                      const hbk_sequence_t* seq, hbk_stream_t stream) {
  return hbk::sequence_id_grid(n_cols, cols, seq, stream);
}

extern "C" int hbk_group_lookup_fwd_sequence(int32_t n_cols, const hbk_lookup_column_t* cols,
                                             const hbk_sequence_t* seq, const float* max_norms,
                                             hbk_stream_t stream) {
  return hbk::sequence_fwd("group_lookup_fwd_sequence", true, n_cols, cols, seq, max_norms, stream);
}

extern "C" int hbk_sequence_row_grid_n(int32_t n_cols, const hbk_lookup_column_t* cols,
                                       const hbk_sequence_t* seq, hbk_stream_t stream) {
  return hbk::sequence_fwd("sequence_row_grid_n", false, n_cols, cols, seq, nullptr, stream);
}
