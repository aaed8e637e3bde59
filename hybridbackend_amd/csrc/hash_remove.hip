// Expiring hash tables (hbk_hash_remove_n): the keys a caller names leave N tables exactly as the sweeps make a
// key leave -- key -> TOMBSTONE (never EMPTY: hash_insert.hip, the probe's invariant), last_seen = freq = 0, the
// rows of the companion arrays filled with their value, the embedding row left for the next inserter -- and
// slots[i] answers the slot keys[i] held BEFORE the call, for every occurrence, duplicates included.
//
// Two launches per 32 columns, on the call's stream:
//   find   the pure find of the expiring table kind (hbk_hash_insert_expiring_n with insert == 0: plain loads, no
//          counter, no metadata), called as it is.  It writes slots.
//   erase  tiled over the OCCURRENCES of all columns; a lane owns one.  With s = slots[i] >= 0 the lane swaps
//          keys[s]: id -> TOMBSTONE with a 64-bit agent-scope compare-and-swap.  Of the occurrences of one id
//          exactly one finds the id still there: the winner.  It stores the metadata zeros; the wave ballots its
//          winners, gathers their lane numbers into the low lanes with one permute (compact_lanes) and fills their
//          companion rows with groups of pow2(dim) lanes, 64 / pow2(dim) rows per pass: hash_common.h's fill_rows,
//          the loop of sweep_wave -- the row's slot number arrives by a shuffle from the winner's lane, where the
//          sweep has first + lane.  One atomic per wave and counter.
//
// Why two kernels.  In one fused kernel a duplicate that walks after the winner's swap would find a TOMBSTONE and
// answer -1: slots would depend on which wave runs first.  The kernel boundary puts every read of the key array
// before every write of it, so slots, the arrays and both counters are functions of the inputs alone.  Which of an
// id's occurrences wins the swap is NOT fixed, and nothing that is written depends on it.
//
// Launch groups.  More than 32 columns with keys go in groups of 32, each group's find and erase before the next
// group's: the groups touch different columns, so the order between them does not matter.  Every refusal comes
// before the first launch, the grids included: the find's tiles of every group are summed in the validation, where
// the find entry itself would notice a grid of 2^31 tiles only at that group's turn.  A column of 2^30 keys or more
// goes through the find in up to three parts, the find entry's own limit per column (no test runs that path: it
// needs 8 GB of ids; the parts are consecutive ranges of the same keys and slots).
//
// Memory rules.  The find reads the key array with plain loads: nothing writes it beside it (the call is
// stream-ordered against translates, sweeps and backwards of its tables, never beside one).  The erase kernel's
// only access to the key array is the swap, served by the device's L2 whatever CU issues it; the other stores are
// plain -- one winner per slot -- and the kernel boundary makes them visible to the next launch.  No loop waits
// for anything: a lane does one swap.
#include "hash_common.h"

namespace hbk {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kChunks = 4;                              // 64-occurrence chunks per wave
constexpr int kKeysPerBlock = kBlock * kChunks;
constexpr int kMaxColsPerLaunch = 32;                   // RemoveArgs travels by value

struct RemoveCol {
  long long* keys;        // the table's key array
  const int64_t* ids;
  const int64_t* slots;   // the find's answers
  int32_t* last_seen;
  int32_t* freq;
  int32_t* stats;         // {n_evicted, n_reused} or NULL
  int32_t* n_removed;     // or NULL
  int64_t capacity;
  int64_t n_keys;
  int32_t n_fills;
  int32_t pad_;
};

struct RemoveArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  RemoveCol col[kMaxColsPerLaunch];
  Fill fill[kMaxColsPerLaunch][HBK_HASH_MAX_FILLS];
};
static_assert(sizeof(RemoveArgs) <= 24576, "kernarg budget");

__global__ __launch_bounds__(kBlock) void hash_remove_erase_kernel(const RemoveArgs a) {
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const RemoveCol& c = a.col[ci];
  const Fill* fills = a.fill[ci];
  const int64_t n_keys = c.n_keys;
  const int64_t capacity = c.capacity;
  const int64_t block_first = (int64_t)(b - a.tile_start[ci]) * kKeysPerBlock;
  int32_t n_won = 0;
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int64_t first = block_first + (int64_t)(u * kWavesPerBlock + wave) * kWave;
    if (first >= n_keys) break;   // (wave-uniform)
    const int64_t i = first + lane;
    bool won = false;
    int32_t slot = 0;             // (capacity < 2^31 was checked)
    if (i < n_keys) {
      const long long id = (long long)c.ids[i];
      const int64_t s = c.slots[i];
      // (the find answers -1 to both sentinels and a slot below the capacity: the rules, written out)
      if (s >= 0 && s < capacity && holds_key(id, true)) {
        long long expected = id;
        won = __hip_atomic_compare_exchange_strong(c.keys + s, &expected, kTombstoneKey, __ATOMIC_RELAXED,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        slot = (int32_t)s;
      }
    }
    const unsigned long long mask = __ballot(won);
    if (mask == 0ull) continue;   // (wave-uniform)
    const int n = (int)__builtin_popcountll(mask);
    n_won += n;
    if (won) {
      c.last_seen[slot] = 0;
      c.freq[slot] = 0;
    }
    if (c.n_fills == 0) continue;
    const int won_lane = compact_lanes(mask, won, lane);     // lane r < n: the lane of the r-th winner
    const int32_t won_slot = __shfl(slot, won_lane, kWave);  // lane r < n: its slot
    fill_rows(c.n_fills, fills, n, lane, [&](int r) { return (int64_t)__shfl(won_slot, r, kWave); });
  }
  if (lane == 0 && n_won != 0) {
    if (c.stats != nullptr) atomicAdd(c.stats, n_won);
    if (c.n_removed != nullptr) atomicAdd(c.n_removed, n_won);
  }
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_hash_remove_n(int32_t n_cols, const hbk_hash_remove_column_t* cols, hbk_stream_t stream) {
  using namespace hbk;
  const char* who = "hash_remove_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_remove_column_t& h = cols[c];
    if (int rc = check_geometry(who, c, "", "keys_cache", h.keys_cache, h.slab_count, h.slab_size)) return rc;
    HBK_REQUIRE(h.slab_count * h.slab_size < (1ll << 31),
                "%s: column %d: slab_count * slab_size = %lld slots, must be below 2^31 (the counters are int32)", who,
                c, (long long)(h.slab_count * h.slab_size));
    HBK_REQUIRE(h.exp.last_seen != nullptr, "%s: column %d: last_seen is NULL", who, c);
    HBK_REQUIRE(h.exp.freq != nullptr, "%s: column %d: freq is NULL", who, c);
    HBK_REQUIRE(h.n_keys >= 0 && h.n_keys < (1ll << 31), "%s: column %d: n_keys must be in [0, 2^31), got %lld", who,
                c, (long long)h.n_keys);
    HBK_REQUIRE(h.n_keys == 0 || h.keys != nullptr, "%s: column %d: keys is NULL with n_keys = %lld", who, c,
                (long long)h.n_keys);
    HBK_REQUIRE(h.n_keys == 0 || h.slots != nullptr, "%s: column %d: slots is NULL with n_keys = %lld", who, c,
                (long long)h.n_keys);
    if (int rc = check_fills(who, c, h.n_fills, h.fills)) return rc;
  }
  // the grids of every launch group, before the first launch: the find entry would refuse a grid of 2^31 tiles
  // only when its group's turn came, behind the erase of the groups before it (the erase's own grid is smaller:
  // 1024 occurrences per tile)
  if (int rc = check_find_grids(who, n_cols, kMaxColsPerLaunch, [&](int32_t c, int32_t* slab_size) {
        *slab_size = cols[c].slab_size;
        return cols[c].n_keys;
      })) {
    return rc;
  }
  int32_t c0 = 0;
  while (c0 < n_cols) {
    RemoveArgs args;
    hbk_hash_column_t find_cols[kMaxColsPerLaunch * kFindParts];
    hbk_hash_expiry_t find_exp[kMaxColsPerLaunch * kFindParts];
    int32_t k = 0, n_find = 0;
    int64_t tiles = 0;
    args.tile_start[0] = 0;
    while (c0 < n_cols && k < kMaxColsPerLaunch) {
      const hbk_hash_remove_column_t& h = cols[c0++];
      if (h.n_keys == 0) continue;
      n_find += describe_find_parts(h, find_cols + n_find, find_exp + n_find);
      RemoveCol& d = args.col[k];
      d.keys = reinterpret_cast<long long*>(h.keys_cache);
      d.ids = h.keys;
      d.slots = h.slots;
      d.last_seen = h.exp.last_seen;
      d.freq = h.exp.freq;
      d.stats = h.exp.stats;
      d.n_removed = h.n_removed;
      d.capacity = h.slab_count * h.slab_size;
      d.n_keys = h.n_keys;
      d.n_fills = h.n_fills;
      d.pad_ = 0;
      describe_fills(h.n_fills, h.fills, args.fill[k]);
      tiles += (h.n_keys + kKeysPerBlock - 1) / kKeysPerBlock;   // (< 2^21 per column: 32 of them fit a grid)
      ++k;
      args.tile_start[k] = (int32_t)tiles;
    }
    if (k == 0) continue;
    args.n_cols = k;
    if (int rc = hbk_hash_insert_expiring_n(n_find, find_cols, find_exp, 0, stream)) return rc;
    hipLaunchKernelGGL(hash_remove_erase_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, as_stream(stream), args);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}
