// Spilling (hbk_hash_spill_n, hbk_hash_spill_lfu_n): export exactly the keys an eviction removes, then remove them.
// include/hbk.h has the semantics.  The selection was made by the order's select entry (hash_evict_to.hip) and is
// READ FROM DEVICE MEMORY by every launch: selection = that order's report (hash_order.h) -- {live_before, need, cut,
// n_selected} for LRU, {live_before, need, cut_freq, cut_last_seen, n_selected, ...} for LFU -- and a slot is
// selected iff it holds a key, is not protected by keep_freq, need > 0 and its key is at or below the cut: last_seen
// <= cut (signed), or the pair (freq, last_seen) against (cut_freq, cut_last_seen).  No host read anywhere.
//
// Four launches per 32 tables on the call's stream:
//   1-3. count, scan, write   hash_pack.h's stream compaction (the export's kernels, instantiated with this
//                             selection): keys, source slots and every move in ascending slot order, packed from 0,
//                             nothing behind out_capacity, *count = the total.  Plain loads and stores.  The
//                             scan's thread 0 also zeroes n_evicted, so a captured call replays.
//   4.   sweep                hash_common.h's sweep_wave with the same predicate, tiled as the compaction:
//                             TOMBSTONE, last_seen = freq = 0, companions filled, stats[0] and n_evicted added to
//                             (integer atomics: order-independent sums).  A table whose *count exceeds its
//                             out_capacity is left untouched: nothing leaves that was not exported in full.
// The kernel boundary between 3 and 4 orders the copies before the resets.
#include "hash_order.h"
#include "hash_pack.h"

namespace hbk {
namespace {

using namespace pack;

// the selection as both halves read it (selection: the order's report, hash_order.h)
template <class Order>
__device__ inline bool spilled(const int32_t* selection, int32_t keep_freq, long long key, int32_t seen,
                               int32_t freq) {
  return holds_key(key, true) && (keep_freq == 0 || freq < keep_freq) && Order::selected(selection, freq, seen);
}

template <class Order>
struct SpillCol {
  long long* keys;
  const int32_t* last_seen;
  const int32_t* freq;
  const int32_t* selection;
  long long* out_keys;
  int64_t* out_slots;         // or NULL
  int64_t* count;
  int64_t* tiles;             // workspace [n_tiles]: counts after launch 1, exclusive offsets after launch 2
  int32_t* n_evicted;         // or NULL
  int64_t capacity;
  int64_t out_capacity;
  int64_t n_tiles;
  int32_t keep_freq;
  int32_t n_moves;
  Move move[HBK_HASH_MAX_MOVES];

  __device__ bool selected(int64_t slot) const {
    if (slot >= capacity) return false;
    return spilled<Order>(selection, keep_freq, keys[slot], last_seen[slot], freq[slot]);
  }
  __device__ void scanned() const {
    if (n_evicted != nullptr) *n_evicted = 0;
  }
};

template <class Order>
struct SpillArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  SpillCol<Order> col[kMaxColsPerLaunch];
};
static_assert(sizeof(SpillArgs<LruOrder>) <= 24576 && sizeof(SpillArgs<LfuOrder>) <= 24576, "kernarg budget");

struct SweepCol {
  long long* keys;
  int32_t* last_seen;
  int32_t* freq;
  int32_t* stats;             // {n_evicted, n_reused} or NULL
  const int32_t* selection;
  const int64_t* count;       // written by the scan launch
  int32_t* n_evicted;         // or NULL
  int64_t capacity;
  int64_t out_capacity;
  int32_t keep_freq;
  int32_t n_fills;
  Fill fill[HBK_HASH_MAX_FILLS];
};

struct SweepArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  SweepCol col[kMaxColsPerLaunch];
};
static_assert(sizeof(SweepArgs) <= 24576, "kernarg budget");

template <class Order>
__global__ __launch_bounds__(kBlock) void hash_spill_sweep_kernel(const SweepArgs a) {
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const SweepCol& c = a.col[ci];
  const int32_t* selection = c.selection;
  if (selection[1] <= 0) return;            // inside the bound: nothing is written
  if (*c.count > c.out_capacity) return;    // not exported in full: the table stays as it is
  const int64_t capacity = c.capacity;
  const int32_t keep_freq = c.keep_freq;
  const int64_t first = (int64_t)(b - a.tile_start[ci]) * kSlotsPerTile + (int64_t)wave * kWave;
  if (first >= capacity) return;   // (wave-uniform)
  const int32_t n = sweep_wave(c.keys, c.last_seen, c.freq, capacity, first, lane, c.n_fills, c.fill,
                               [&](long long key, int32_t seen, int32_t freq) {
                                 return spilled<Order>(selection, keep_freq, key, seen, freq);
                               });
  if (lane == 0 && n != 0) {
    if (c.stats != nullptr) atomicAdd(c.stats, n);
    if (c.n_evicted != nullptr) atomicAdd(c.n_evicted, n);
  }
}

int check_spill(const char* who, int32_t n_cols, const hbk_hash_spill_column_t* cols, bool outputs) {
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_spill_column_t& h = cols[c];
    if (int rc = check_geometry(who, c, "", "keys_cache", h.keys_cache, h.slab_count, h.slab_size)) return rc;
    HBK_REQUIRE(h.slab_count * h.slab_size < (1ll << 31),
                "%s: column %d: slab_count * slab_size = %lld slots, must be below 2^31 (the counters are int32)", who,
                c, (long long)(h.slab_count * h.slab_size));
    if (!outputs) continue;
    HBK_REQUIRE(h.exp.last_seen != nullptr, "%s: column %d: last_seen is NULL", who, c);
    HBK_REQUIRE(h.exp.freq != nullptr, "%s: column %d: freq is NULL", who, c);
    HBK_REQUIRE(h.selection != nullptr, "%s: column %d: selection is NULL", who, c);
    HBK_REQUIRE(((uintptr_t)h.selection & 3) == 0, "%s: column %d: selection must be 4-byte aligned", who, c);
    HBK_REQUIRE(h.keep_freq >= 0, "%s: column %d: keep_freq must be >= 0, got %d", who, c, h.keep_freq);
    if (int rc = check_moves(who, c, h.n_moves, h.moves)) return rc;
    if (int rc = check_fills(who, c, h.n_fills, h.fills)) return rc;
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

extern "C" int hbk_hash_spill_workspace_bytes(int32_t n_cols, const hbk_hash_spill_column_t* cols, size_t* bytes) {
  using namespace hbk;
  const char* who = "hash_spill_workspace_bytes";
  HBK_REQUIRE(bytes != nullptr, "%s: bytes is NULL", who);
  *bytes = 0;
  if (int rc = check_spill(who, n_cols, cols, false)) return rc;
  int64_t tiles = 0;
  for (int32_t c = 0; c < n_cols; ++c) tiles += tiles_of(cols[c].slab_count * cols[c].slab_size);
  *bytes = (size_t)tiles * sizeof(int64_t);
  return HBK_OK;
}

namespace hbk {
namespace {

// both entries, after check_spill: the compaction and the sweep with the order's selection
template <class Order>
int spill(const char* who, int32_t n_cols, const hbk_hash_spill_column_t* cols, void* workspace, hbk_stream_t stream) {
  if (int rc = check_spill(who, n_cols, cols, true)) return rc;
  if (n_cols == 0) return HBK_OK;
  HBK_REQUIRE(workspace != nullptr, "%s: workspace is NULL (hbk_hash_spill_workspace_bytes says how large)", who);
  HBK_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  int64_t* ws = static_cast<int64_t*>(workspace);
  for (int32_t c0 = 0; c0 < n_cols; c0 += kMaxColsPerLaunch) {
    SpillArgs<Order> args;
    SweepArgs sweep;
    const int32_t k = n_cols - c0 < kMaxColsPerLaunch ? n_cols - c0 : kMaxColsPerLaunch;
    int64_t tiles = 0;
    args.tile_start[0] = sweep.tile_start[0] = 0;
    for (int32_t i = 0; i < k; ++i) {
      const hbk_hash_spill_column_t& h = cols[c0 + i];
      SpillCol<Order>& d = args.col[i];
      d.keys = reinterpret_cast<long long*>(h.keys_cache);
      d.last_seen = h.exp.last_seen;
      d.freq = h.exp.freq;
      d.selection = h.selection;
      d.out_keys = reinterpret_cast<long long*>(h.out_keys);
      d.out_slots = h.out_slots;
      d.count = h.count;
      d.tiles = ws;
      d.n_evicted = h.n_evicted;
      d.capacity = h.slab_count * h.slab_size;
      d.out_capacity = h.out_capacity;
      d.n_tiles = tiles_of(d.capacity);
      d.keep_freq = h.keep_freq;
      d.n_moves = h.n_moves;
      describe_moves(h.n_moves, h.moves, d.move);
      SweepCol& w = sweep.col[i];
      w.keys = d.keys;
      w.last_seen = h.exp.last_seen;
      w.freq = h.exp.freq;
      w.stats = h.exp.stats;
      w.selection = h.selection;
      w.count = h.count;
      w.n_evicted = h.n_evicted;
      w.capacity = d.capacity;
      w.out_capacity = h.out_capacity;
      w.keep_freq = h.keep_freq;
      w.n_fills = h.n_fills;
      describe_fills(h.n_fills, h.fills, w.fill);
      ws += d.n_tiles;
      tiles += d.n_tiles;   // (< 2^23 per table: 32 of them fit a grid)
      args.tile_start[i + 1] = sweep.tile_start[i + 1] = (int32_t)tiles;
    }
    args.n_cols = sweep.n_cols = k;
    if (int rc = launch_pack(args, tiles, as_stream(stream))) return rc;
    hipLaunchKernelGGL(hash_spill_sweep_kernel<Order>, dim3((unsigned)tiles), dim3(kBlock), 0, as_stream(stream),
                       sweep);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_hash_spill_n(int32_t n_cols, const hbk_hash_spill_column_t* cols, void* workspace,
                                hbk_stream_t stream) {
  return hbk::spill<hbk::LruOrder>("hash_spill_n", n_cols, cols, workspace, stream);
}

extern "C" int hbk_hash_spill_lfu_n(int32_t n_cols, const hbk_hash_spill_column_t* cols, void* workspace,
                                    hbk_stream_t stream) {
  return hbk::spill<hbk::LfuOrder>("hash_spill_lfu_n", n_cols, cols, workspace, stream);
}
