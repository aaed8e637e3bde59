// hbk_sequence_pack_n: the PACKED form of a zero-padded sequence column (include/hbk.h) -- the first
// min(len, T) ids of every sample back to back, and the position-level row splits that make the column a
// ragged one of B * T segments holding one id or none: what a sharded sequence column without a pad id hands
// the sharded step, whose combiner 'sum' turns an empty segment into a zero row that reaches no gradient.
//
// Three launches per launch group of up to kMaxColsPerLaunch columns (the by-value argument struct and the
// ballot over the tile prefix of lookup_sequence.hip), ordered by the stream alone -- no tile waits for
// another one inside a launch, so nothing here depends on dispatch order or on what another CU's L1 holds:
//   count   one workgroup per tile of kTile samples: the tile's clamped lengths summed into the workspace
//   scan    one workgroup per column: the exclusive scan of its tile sums, in passes of kBlock; total
//   write   ceil(T / kU) workgroups per tile: each scans the tile's samples again (257 row splits, L2 hits), the
//           first of them writes lengths and sample_splits, and each covers kU * kBlock of the tile's positions,
//           kU per thread -- their id loads issued together, then pos_splits and packed stored
// Plain loads and stores, no atomics; every workspace word is written by `count` before `scan` reads it, so
// no scratch needs clearing and a captured call replays.  A wave stores 64 consecutive pos_splits words and,
// inside a sample, consecutive 8-byte packed words (consecutive samples continue each other in packed).
#include <vector>

#include "lookup_common.h"

namespace hbk {
namespace {

constexpr int kBlock = 256;            // 4 waves
constexpr int kTile = kBlock;          // samples per tile: one per thread
constexpr int kWaves = kBlock / kWave;
constexpr int kU = 4;                  // positions per thread of the write launch: independent id loads in flight
constexpr int kMaxColsPerLaunch = 64;  // one ballot finds the column; PackArgs travels by value

struct PackCol {
  const void* ids;
  const int32_t* splits;    // NULL: one id per sample
  int32_t* lengths;
  int32_t* sample_splits;
  int32_t* pos_splits;
  int64_t* packed;
  int32_t* total;
  int32_t* tile_sums;       // workspace: one word per tile of samples
  int64_t capacity;         // of packed
  int64_t n_ids;
  int64_t n_pos;            // B * T
  FastDiv max_len;          // T
  int32_t n_samples;        // B
  int32_t n_tiles;          // ceil(B / kTile)
  int32_t parts;            // workgroups of the write launch per tile: ceil(T / kU)
  int32_t ids64;
};

struct PackArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  PackCol col[kMaxColsPerLaunch];
};
static_assert(sizeof(PackArgs) <= 24576, "kernarg budget");

// l_b = min(max(len_b, 0), T) and the index of the sample's first id; 0 for a thread without a sample
__device__ inline int32_t clamped_len(const PackCol& c, int64_t b, int32_t* beg_out) {
  if (b >= (int64_t)c.n_samples) {
    *beg_out = 0;
    return 0;
  }
  int32_t beg = (int32_t)b, end = (int32_t)b + 1;
  if (c.splits != nullptr) {
    beg = c.splits[b];
    end = c.splits[b + 1];
  }
  int64_t len = (int64_t)end - (int64_t)beg;
  const int64_t T = (int64_t)c.max_len.d;
  len = len < 0 ? 0 : (len > T ? T : len);
  *beg_out = beg;
  return (int32_t)len;
}

// exclusive scan of one value per thread over the workgroup; *sum: the workgroup's total.  `lds`: kWaves
// words; the barrier in front lets a caller's loop reuse them.
__device__ inline int32_t block_exclusive_scan(int32_t v, int32_t* lds, int32_t* sum) {
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  int32_t inc = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int32_t x = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += x;
  }
  __syncthreads();
  if (lane == kWave - 1) lds[wave] = inc;
  __syncthreads();
  int32_t base = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int32_t x = lds[w];
    if (w < wave) base += x;
    all += x;
  }
  *sum = all;
  return base + inc - v;
}

__global__ __launch_bounds__(kBlock) void sequence_pack_count_kernel(const PackArgs a) {
  __shared__ int32_t lds[kWaves];
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const PackCol& c = a.col[ci];
  const int tile = b - a.tile_start[ci];
  int32_t beg, sum;
  const int32_t l = clamped_len(c, (int64_t)tile * kTile + (int64_t)threadIdx.x, &beg);
  block_exclusive_scan(l, lds, &sum);
  if (threadIdx.x == 0) c.tile_sums[tile] = sum;
}

// tile sums -> their exclusive prefix, in place; the column's total and the closing words of both splits
__global__ __launch_bounds__(kBlock) void sequence_pack_scan_kernel(const PackArgs a) {
  __shared__ int32_t lds[kWaves];
  const PackCol& c = a.col[blockIdx.x];
  int32_t carry = 0;
  for (int32_t i0 = 0; i0 < c.n_tiles; i0 += kBlock) {
    const int32_t i = i0 + (int32_t)threadIdx.x;
    const int32_t v = i < c.n_tiles ? c.tile_sums[i] : 0;
    int32_t sum;
    const int32_t ex = block_exclusive_scan(v, lds, &sum);
    if (i < c.n_tiles) c.tile_sums[i] = carry + ex;
    carry += sum;
  }
  if (threadIdx.x == 0) {
    c.total[0] = carry;
    c.sample_splits[c.n_samples] = carry;
    c.pos_splits[c.n_pos] = carry;
  }
}

__global__ __launch_bounds__(kBlock) void sequence_pack_write_kernel(const PackArgs a) {
  __shared__ int32_t lds[kWaves];
  __shared__ int32_t s_start[kTile], s_len[kTile], s_beg[kTile];
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const PackCol& c = a.col[ci];
  const int local = b - a.tile_start[ci];
  const int tile = local / c.parts, part = local - tile * c.parts;
  const int64_t b0 = (int64_t)tile * kTile;
  const int64_t sample = b0 + (int64_t)threadIdx.x;
  int32_t beg, sum;
  const int32_t l = clamped_len(c, sample, &beg);
  const int32_t start = c.tile_sums[tile] + block_exclusive_scan(l, lds, &sum);
  s_start[threadIdx.x] = start;
  s_len[threadIdx.x] = l;
  s_beg[threadIdx.x] = beg;
  if (part == 0 && sample < (int64_t)c.n_samples) {
    c.lengths[sample] = l;
    c.sample_splits[sample] = start;
  }
  __syncthreads();
  const int64_t T = (int64_t)c.max_len.d;
  const int64_t left = (int64_t)c.n_samples - b0;
  const int64_t n_q = (left < kTile ? left : (int64_t)kTile) * T;   // positions of this tile
  const int64_t p0 = b0 * T;
  const int64_t q0 = (int64_t)part * (kU * kBlock) + (int64_t)threadIdx.x;
  int64_t at[kU], id[kU];
  bool holds[kU];
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int64_t q = q0 + u * kBlock;
    at[u] = 0;
    id[u] = 0;
    holds[u] = false;
    if (q < n_q) {
      const int64_t s = (int64_t)fastdiv((uint64_t)q, c.max_len);
      const int64_t t = q - s * T;
      const int64_t len = (int64_t)s_len[s];
      at[u] = (int64_t)s_start[s] + (t < len ? t : len);
      // (`at` reaches the capacity only with row splits that are no CSR of the ids)
      holds[u] = t < len && at[u] < c.capacity;
      // (row splits that point outside the ids read nothing: such an element holds 0)
      const int64_t j = (int64_t)s_beg[s] + t;
      if (holds[u] && (uint64_t)j < (uint64_t)c.n_ids) id[u] = load_id(c.ids, c.ids64 != 0, j);
    }
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int64_t q = q0 + u * kBlock;
    if (q < n_q) c.pos_splits[p0 + q] = (int32_t)at[u];
    if (holds[u]) c.packed[at[u]] = id[u];
  }
}

inline int64_t tiles_of(int64_t samples) { return (samples + kTile - 1) / kTile; }

int sequence_pack(int32_t n_cols, const hbk_lookup_column_t* cols, const hbk_sequence_t* seq,
                  const hbk_sequence_pack_t* pack, void* workspace, size_t workspace_bytes,
                  hbk_stream_t stream) {
  const char* who = "sequence_pack_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(n_cols == 0 || seq != nullptr, "%s: seq is NULL", who);
  HBK_REQUIRE(n_cols == 0 || pack != nullptr, "%s: pack is NULL", who);
  int64_t words = 0;
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_lookup_column_t& h = cols[c];
    const hbk_sequence_t& q = seq[c];
    const hbk_sequence_pack_t& k = pack[c];
    HBK_REQUIRE(q.max_len >= 1, "%s: column %d: max_len must be >= 1, got %d", who, c, q.max_len);
    HBK_REQUIRE(q.has_pad == 0, "%s: column %d: has_pad is %d: a pad id belongs to the grid ops "
                "(hbk_sequence_row_grid_n, hbk_sequence_id_grid_n); the packed form holds no padding at all", who,
                c, q.has_pad);
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
    HBK_REQUIRE(q.lengths != nullptr && k.packed != nullptr && k.pos_splits != nullptr &&
                k.sample_splits != nullptr && k.total != nullptr,
                "%s: column %d: NULL output (lengths, packed, pos_splits, sample_splits and total are all "
                "written, also with B == 0)", who, c);
    const int64_t n_pos = h.n_segments * (int64_t)q.max_len;
    const int64_t need = h.n_ids < n_pos ? h.n_ids : n_pos;
    HBK_REQUIRE(k.packed_capacity >= need, "%s: column %d: packed_capacity %lld is smaller than "
                "min(n_ids, B * T) = %lld", who, c, (long long)k.packed_capacity, (long long)need);
    words += tiles_of(h.n_segments);
    HBK_REQUIRE((size_t)words * sizeof(int32_t) <= workspace_bytes && (words == 0 || workspace != nullptr),
                "%s: column %d: a workspace of %zu bytes is too small: %zu bytes are needed "
                "(hbk_sequence_pack_workspace_bytes)", who, c, workspace != nullptr ? workspace_bytes : (size_t)0,
                hbk_sequence_pack_workspace_bytes(n_cols, cols));
  }
  int32_t* ws = static_cast<int32_t*>(workspace);
  hipStream_t s = as_stream(stream);
  for (int32_t c0 = 0; c0 < n_cols; c0 += kMaxColsPerLaunch) {
    PackArgs args;
    const int32_t k = n_cols - c0 < kMaxColsPerLaunch ? n_cols - c0 : kMaxColsPerLaunch;
    int64_t tiles = 0;
    args.n_cols = k;
    args.tile_start[0] = 0;
    for (int32_t i = 0; i < k; ++i) {
      const hbk_lookup_column_t& h = cols[c0 + i];
      const hbk_sequence_t& q = seq[c0 + i];
      const hbk_sequence_pack_t& p = pack[c0 + i];
      PackCol& d = args.col[i];
      d.ids = h.ids;
      d.splits = h.row_splits;
      d.lengths = q.lengths;
      d.sample_splits = p.sample_splits;
      d.pos_splits = p.pos_splits;
      d.packed = p.packed;
      d.total = p.total;
      d.tile_sums = ws;
      d.capacity = p.packed_capacity;
      d.n_ids = h.n_ids;
      d.n_pos = h.n_segments * (int64_t)q.max_len;
      d.max_len = make_fastdiv((uint64_t)q.max_len);
      d.n_samples = (int32_t)h.n_segments;
      d.n_tiles = (int32_t)tiles_of(h.n_segments);
      d.parts = (int32_t)(((int64_t)q.max_len + kU - 1) / kU);
      d.ids64 = h.ids_dtype == HBK_INT64;
      ws += d.n_tiles;
      tiles += d.n_tiles;
      args.tile_start[i + 1] = (int32_t)tiles;
    }
    if (tiles > 0) {
      hipLaunchKernelGGL(sequence_pack_count_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, s, args);
      HBK_HIP_OK(hipGetLastError());
    }
    hipLaunchKernelGGL(sequence_pack_scan_kernel, dim3((unsigned)k), dim3(kBlock), 0, s, args);
    HBK_HIP_OK(hipGetLastError());
    if (tiles > 0) {
      // the write launch deals `parts` workgroups to every tile of a column: its tile prefix counts those
      // (below 2^31: a workgroup per kU * kBlock positions and at most one short one per tile)
      int64_t groups = 0;
      for (int32_t i = 0; i < k; ++i) {
        groups += (int64_t)args.col[i].n_tiles * args.col[i].parts;
        HBK_REQUIRE(groups < (1ll << 31), "%s: grid too large", who);
        args.tile_start[i + 1] = (int32_t)groups;
      }
      hipLaunchKernelGGL(sequence_pack_write_kernel, dim3((unsigned)groups), dim3(kBlock), 0, s, args);
      HBK_HIP_OK(hipGetLastError());
    }
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" size_t hbk_sequence_pack_workspace_bytes(int32_t n_cols, const hbk_lookup_column_t* cols) {
  if (n_cols <= 0 || cols == nullptr) return 0;
  int64_t words = 0;
  for (int32_t c = 0; c < n_cols; ++c) {
    if (cols[c].n_segments > 0) words += hbk::tiles_of(cols[c].n_segments);
  }
  return (size_t)words * sizeof(int32_t);
}

extern "C" int hbk_sequence_pack_n(int32_t n_cols, const hbk_lookup_column_t* cols, const hbk_sequence_t* seq,
                                   const hbk_sequence_pack_t* pack, void* workspace, size_t workspace_bytes,
                                   hbk_stream_t stream) {
  return hbk::sequence_pack(n_cols, cols, seq, pack, workspace, workspace_bytes, stream);
}
