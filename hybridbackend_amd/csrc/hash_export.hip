// Hash tables leaving and entering the device whole (hbk_hash_export_n, hbk_hash_store_rows_n).
//
// Export: a stream compaction of N tables per call.  A slot is exported iff it holds a key (not EMPTY; not
// TOMBSTONE when `expiring` is set) and, with since > 0, last_seen[slot] >= since.  The exported keys appear in
// ASCENDING SOURCE-SLOT ORDER, packed from position 0, and every per-slot array named as a move (the embedding
// row, the optimizer slots, last_seen, freq) is copied bit for bit from the source slot to the key's position.
// The output is a function of the table's arrays alone: no ticket atomic (its order differs from run to run)
// and no look-back between tiles (no workgroup waits for another).  Instead, "output ranges from a count
// launch" as the deterministic backward has them -- three launches on the call's stream:
//   1. count   a 256-slot tile (one 64-slot chunk per wave) counts its matches into the workspace;
//   2. scan    one workgroup per column turns the tile counts into exclusive offsets in place and writes the
//              total to `count`;
//   3. write   every tile evaluates the SAME predicate again (nobody may write the table during the call) and
//              places lane's key at  tile offset + matches of the earlier waves of the tile + rank_below(ballot).
// The live lanes' numbers are gathered into the low lanes with one ds_permute (hash_common.h: compact_lanes)
// and lane groups copy the rows, r-th live slot -> r-th position of the wave's range: a wave's output rows are
// contiguous.  Nothing is written at positions >= out_capacity; `count` still receives the total.
//
// Store (hbk_hash_store_rows_n): the other half of an import.  The keys were placed by the table's own translate
// entry; this launch is dst[slots[i] * dst_pitch + j] = src[i * src_pitch + j] for every move of every column,
// one lane group per row, slots[i] outside [0, dst_rows) skipped.
//
// Memory rules: plain loads and plain vector stores only; no atomics anywhere in this file.  The tables are
// quiescent during either call, and the kernel boundaries order the three launches of an export.
//
// Rows travel as 4-byte words.  A move whose two bases, two pitches and width are all multiples of 16 bytes is
// copied with 16-byte accesses (hash_common.h: Move); the lane group of a move is pow2(accesses per row).
//
// The three launches of the export are hash_pack.h's, shared with hbk_hash_spill_n (hash_spill.hip): the kernels are
// templates over the argument struct, whose columns bring the selection.
#include "hash_pack.h"

namespace hbk {
namespace {

using namespace pack;   // kBlock, kSlotsPerTile, kMaxColsPerLaunch, tiles_of, the three kernels

struct ExportCol {
  const long long* keys;
  const int32_t* last_seen;   // read only when since > 0
  long long* out_keys;
  int64_t* out_slots;         // or NULL
  int64_t* count;
  int64_t* tiles;             // workspace [n_tiles]: counts after launch 1, exclusive offsets after launch 2
  int64_t capacity;
  int64_t out_capacity;
  int64_t n_tiles;
  int32_t since;
  int32_t expiring;
  int32_t n_moves;
  int32_t pad_;
  Move move[HBK_HASH_MAX_MOVES];

  // the selection: the one predicate of the count and the write launch
  __device__ bool selected(int64_t slot) const {
    if (slot >= capacity) return false;
    const long long key = keys[slot];
    if (!holds_key(key, expiring != 0)) return false;
    return since <= 0 || last_seen[slot] >= since;
  }
  __device__ void scanned() const {}
};

struct ExportArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  ExportCol col[kMaxColsPerLaunch];
};
static_assert(sizeof(ExportArgs) <= 24576, "kernarg budget");

struct StoreCol {
  const int64_t* slots;
  int64_t n;
  int64_t dst_rows;
  int32_t n_moves;
  int32_t pad_;
  Move move[HBK_HASH_MAX_MOVES];
};

struct StoreArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  StoreCol col[kMaxColsPerLaunch];
};
static_assert(sizeof(StoreArgs) <= 24576, "kernarg budget");

__global__ __launch_bounds__(kBlock) void hash_store_rows_kernel(const StoreArgs a) {
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const StoreCol& c = a.col[ci];
  const int64_t first = (int64_t)(b - a.tile_start[ci]) * kSlotsPerTile + (int64_t)wave * kWave;
  if (first >= c.n) return;   // (wave-uniform)
  int64_t my_slot = -1;
  if (first + lane < c.n) my_slot = c.slots[first + lane];
  if (my_slot >= c.dst_rows) my_slot = -1;   // (a slot outside the destination is skipped, never written)
  if (__ballot(my_slot >= 0) == 0ull) return;   // (wave-uniform)
  for (int m = 0; m < c.n_moves; ++m) {
    const Move& mv = c.move[m];
    const int lanes_log2 = mv.lanes_log2;
    const int sub = lane & ((1 << lanes_log2) - 1);
    for (int r0 = 0; r0 < kWave; r0 += kWave >> lanes_log2) {
      const int r = r0 + (lane >> lanes_log2);
      const int64_t to = (int64_t)__shfl((long long)my_slot, r & (kWave - 1), kWave);   // (every lane takes the shuffle)
      if (to >= 0) copy_row(mv, mv.src + (first + r) * mv.src_pitch, mv.dst + to * mv.dst_pitch, sub, 1 << mv.lanes_log2);
    }
  }
}

int check_export(const char* who, int32_t n_cols, const hbk_hash_export_column_t* cols, bool outputs) {
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_export_column_t& h = cols[c];
    if (int rc = check_geometry(who, c, "", "keys", h.keys, h.slab_count, h.slab_size)) return rc;
    if (!outputs) continue;
    HBK_REQUIRE(h.since <= 0 || h.last_seen != nullptr, "%s: column %d: since = %d needs last_seen, which is NULL",
                who, c, h.since);
    if (int rc = check_moves(who, c, h.n_moves, h.moves)) return rc;
    HBK_REQUIRE(h.count != nullptr, "%s: column %d: count is NULL", who, c);
    HBK_REQUIRE(h.out_capacity >= 0, "%s: column %d: out_capacity must be >= 0, got %lld", who, c,
                (long long)h.out_capacity);
    HBK_REQUIRE(h.out_capacity == 0 || h.out_keys != nullptr, "%s: column %d: out_keys is NULL with out_capacity %lld",
                who, c, (long long)h.out_capacity);
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_hash_export_workspace_bytes(int32_t n_cols, const hbk_hash_export_column_t* cols, size_t* bytes) {
  using namespace hbk;
  const char* who = "hash_export_workspace_bytes";
  HBK_REQUIRE(bytes != nullptr, "%s: bytes is NULL", who);
  *bytes = 0;
  if (int rc = check_export(who, n_cols, cols, false)) return rc;
  int64_t tiles = 0;
  for (int32_t c = 0; c < n_cols; ++c) tiles += tiles_of(cols[c].slab_count * cols[c].slab_size);
  *bytes = (size_t)tiles * sizeof(int64_t);
  return HBK_OK;
}

extern "C" int hbk_hash_export_n(int32_t n_cols, const hbk_hash_export_column_t* cols, void* workspace,
                                 hbk_stream_t stream) {
  using namespace hbk;
  const char* who = "hash_export_n";
  if (int rc = check_export(who, n_cols, cols, true)) return rc;
  if (n_cols == 0) return HBK_OK;
  HBK_REQUIRE(workspace != nullptr, "%s: workspace is NULL (hbk_hash_export_workspace_bytes says how large)", who);
  HBK_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  int64_t* ws = static_cast<int64_t*>(workspace);
  int32_t c0 = 0;
  while (c0 < n_cols) {
    ExportArgs args;
    int32_t k = 0;
    int64_t tiles = 0;
    args.tile_start[0] = 0;
    while (c0 < n_cols && k < kMaxColsPerLaunch) {
      const hbk_hash_export_column_t& h = cols[c0++];
      ExportCol& d = args.col[k];
      d.keys = reinterpret_cast<const long long*>(h.keys);
      d.last_seen = h.last_seen;
      d.out_keys = reinterpret_cast<long long*>(h.out_keys);
      d.out_slots = h.out_slots;
      d.count = h.count;
      d.tiles = ws;
      d.capacity = h.slab_count * h.slab_size;
      d.out_capacity = h.out_capacity;
      d.n_tiles = tiles_of(d.capacity);
      d.since = h.since;
      d.expiring = h.expiring;
      d.n_moves = h.n_moves;
      d.pad_ = 0;
      describe_moves(h.n_moves, h.moves, d.move);
      ws += d.n_tiles;
      tiles += d.n_tiles;
      HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
      ++k;
      args.tile_start[k] = (int32_t)tiles;
    }
    args.n_cols = k;
    if (int rc = launch_pack(args, tiles, as_stream(stream))) return rc;
  }
  return HBK_OK;
}

extern "C" int hbk_hash_store_rows_n(int32_t n_cols, const hbk_hash_store_column_t* cols, hbk_stream_t stream) {
  using namespace hbk;
  const char* who = "hash_store_rows_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_store_column_t& h = cols[c];
    HBK_REQUIRE(h.n >= 0, "%s: column %d: n must be >= 0, got %lld", who, c, (long long)h.n);
    HBK_REQUIRE(h.n == 0 || h.slots != nullptr, "%s: column %d: slots is NULL with n = %lld", who, c, (long long)h.n);
    HBK_REQUIRE(((uintptr_t)h.slots & 7) == 0, "%s: column %d: slots must be 8-byte aligned", who, c);
    HBK_REQUIRE(h.dst_rows >= 0, "%s: column %d: dst_rows must be >= 0, got %lld", who, c, (long long)h.dst_rows);
    if (int rc = check_moves(who, c, h.n_moves, h.moves)) return rc;
  }
  int32_t c0 = 0;
  while (c0 < n_cols) {
    StoreArgs args;
    int32_t k = 0;
    int64_t tiles = 0;
    args.tile_start[0] = 0;
    while (c0 < n_cols && k < kMaxColsPerLaunch) {
      const hbk_hash_store_column_t& h = cols[c0++];
      if (h.n == 0 || h.n_moves == 0 || h.dst_rows == 0) continue;   // nothing to store
      StoreCol& d = args.col[k];
      d.slots = h.slots;
      d.n = h.n;
      d.dst_rows = h.dst_rows;
      d.n_moves = h.n_moves;
      d.pad_ = 0;
      describe_moves(h.n_moves, h.moves, d.move);
      tiles += tiles_of(h.n);
      HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
      ++k;
      args.tile_start[k] = (int32_t)tiles;
    }
    if (k == 0) continue;
    args.n_cols = k;
    hipLaunchKernelGGL(hash_store_rows_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, as_stream(stream), args);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}
