// Expiring hash tables (hbk_hash_missing_runs_n): hbk_hash_missing_n over ids that arrive as runs -- on the owner of
// a sharded hash table a column's ids are W arrays, one per requester, each with its own place for the find's
// answers (hbk_hash_translate_runs_n).  The id list E of a column is the concatenation of its runs in run order;
// the call reports the distinct ids of E that the table does not hold, in the order of their first occurrence in
// E.  include/hbk.h has the contract.  The table is not written.
//
// Positions.  Every run is padded up to whole 256-position tiles: run r of a column starts at position
// 256 * (tiles of the column's earlier runs), and the positions behind its n_keys hold nothing.  No tile straddles
// a run, positions stay monotone in E-order, and so atomicMin(first[cell], p) and the compaction in position order
// give first-occurrence order exactly as hash_missing.hip's flat positions do.  Empty runs take no tile.
//
// One clear launch per call, then per launch group -- up to 32 columns and HBK_HASH_MAX_RUNS_PER_LAUNCH non-empty
// runs, a column's runs never split -- five launches, all on the call's stream:
//   clear  every cell of the call's scratch sets = EMPTY, every first[] = INT32_MAX (plain stores).  The call
//          clears its own workspace, so it asks nothing of what the workspace held and can be captured and replayed.
//   find   hbk_hash_translate_runs_n with insert == 0, called as it is: ONE launch for the group.  It writes the
//          runs' slots.
//   claim  a workgroup takes up to 1024 positions of ONE run (four tiles; a wave walks four 64-position chunks in
//          order, as hash_missing.hip's claim does), a lane owns one position of a chunk.  The workgroup finds its
//          RUN as the runs translate does -- up to four 64-wide ballots over the runs' first claim tiles, the run
//          tables in the kernarg -- and the run names its column.  It records the run of each of its tiles in the
//          column's tile_run[] (workspace): count and write, whose lanes meet the position under divergence, read
//          it from there with a plain load after the kernel boundary.  A position inside the run with slots < 0 and
//          an id that is no sentinel goes into the column's scratch set (hash_miss_set.h: claim_cell, the set
//          hash_missing.hip fills).  A wave without a miss leaves after reading slots: a batch of resident ids
//          issues no atomic.
//   count, scan, write
//          hash_pack.h's stream compaction over the padded positions with the selection "p lies in its run, missed
//          and first[cell(id)] == p": exactly one position per distinct missed id, the first.  Ids only: no moves.
//
// The scratch set, why no lane waits for another and the memory rules: hash_miss_set.h.  The find reads the key
// array with plain loads, as hash_missing.hip's; the kernel boundary that publishes the set and first[] to count and
// write publishes tile_run[] too.
#include <vector>

#include "hash_miss_set.h"

namespace hbk {
namespace {

using namespace miss_set;

constexpr int kMaxRunsPerLaunch = HBK_HASH_MAX_RUNS_PER_LAUNCH;
static_assert(kMaxRunsPerLaunch % kWave == 0, "one ballot per 64 runs");
constexpr int64_t kKeyLimit = 1ll << 30;                // the runs translate of an expiring table takes fewer per column

// one non-empty run of the launch
struct Run {
  const int64_t* keys;
  const int64_t* slots;   // the find's answers
  int64_t n_keys;
  int32_t col;            // of the launch
  int32_t first_tile;     // of the launch: the run's first 256-position tile
};

// one column of the launch: what hash_pack.h's kernels read of a column, and where the column's tiles and runs
// lie in the launch
struct ColRec {
  long long* set;             // workspace [cell_mask + 1]
  int32_t* first;             // workspace [cell_mask + 1]: the smallest position that missed with the cell's id
  long long* out_keys;
  int64_t* count;
  int64_t* tiles;             // workspace [n_tiles]: the compaction's tile counts
  int32_t* tile_run;          // workspace [n_tiles]: the run (of the launch) a tile belongs to; written by the claim
  int64_t out_capacity;
  int64_t n_tiles;
  uint64_t cell_mask;         // S - 1
  int32_t tile_first;         // of the launch: tile_start of this column
  int32_t pad_;
};

// The columns of a launch as hash_pack.h's kernels index them: col[ci] is a VIEW of column ci that can see the
// launch's run table, so that "the id at position p" is answered through the tile's run.
struct ColTable;

// the ids by position (hash_pack.h's write kernel reads the key of a selected position as keys[p])
struct RunIds {
  const ColTable* tab;
  const int32_t* tile_run;
  int32_t tile_first;
  __device__ inline const Run& run_of(int64_t p, int64_t* off) const;
  __device__ inline long long operator[](int64_t p) const {
    int64_t off;
    const Run& r = run_of(p, &off);
    return (long long)r.keys[off];
  }
};

struct ColView {
  RunIds keys;
  const long long* set;
  const int32_t* first;
  long long* out_keys;
  int64_t* out_slots;         // NULL: not wanted
  int64_t* count;
  int64_t* tiles;
  int64_t capacity;           // the padded positions: n_tiles * 256
  int64_t out_capacity;
  int64_t n_tiles;
  uint64_t cell_mask;
  int32_t n_moves;            // 0: ids only
  const Move* move;           // (never read)

  // position p missed: it lies inside its run, holds an id the table could hold and the find did not see it
  __device__ inline bool missed(int64_t p, long long* id) const {
    int64_t off;
    const Run& r = keys.run_of(p, &off);
    if (off >= r.n_keys || r.slots[off] >= 0) return false;
    *id = (long long)r.keys[off];
    return holds_key(*id, true);
  }
  __device__ inline bool selected(int64_t p) const {
    if (p >= capacity) return false;
    long long id;
    if (!missed(p, &id)) return false;
    return first_position(set, first, cell_mask, id) == (int32_t)p;
  }
  __device__ void scanned() const {}
};

struct ColTable {
  ColRec rec[kMaxColsPerLaunch];
  int32_t n_runs;
  int32_t pad_;
  int32_t run_claim_start[kMaxRunsPerLaunch];  // the runs' first CLAIM tiles (1024 positions), one per lane of a ballot
  Run run[kMaxRunsPerLaunch];

  __device__ inline ColView operator[](int ci) const {
    const ColRec& c = rec[ci];
    return ColView{RunIds{this, c.tile_run, c.tile_first}, c.set, c.first, c.out_keys, nullptr, c.count, c.tiles,
                   c.n_tiles * kSlotsPerTile, c.out_capacity, c.n_tiles, c.cell_mask, 0, nullptr};
  }
};

// the run of position p of the column, recorded by the claim, and p's place in it.  The 64 positions of a wave
// lie in one tile: the run is wave-uniform.
__device__ inline const Run& RunIds::run_of(int64_t p, int64_t* off) const {
  const int64_t tile = p / kSlotsPerTile;
  const int ri = __builtin_amdgcn_readfirstlane(tile_run[tile]);
  const Run& r = tab->run[ri];
  *off = p - (int64_t)(r.first_tile - tile_first) * kSlotsPerTile;
  return r;
}

struct MissRunsArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];    // 256 positions per tile: count and write
  ColTable col;
};
static_assert(sizeof(MissRunsArgs) <= 24576, "kernarg budget");

// last run whose first claim tile is <= b (hash_insert.hip's find_run): up to four 64-wide ballots; every lane calls
__device__ inline int find_run(const ColTable& t, int b) {
  const int lane = lane_id();
  int below = 0;
#pragma unroll
  for (int k = 0; k < kMaxRunsPerLaunch / kWave; ++k) {
    if (k * kWave >= t.n_runs) break;   // (uniform)
    const int i = k * kWave + lane;
    const int t0 = i < t.n_runs ? t.run_claim_start[i] : 0x7fffffff;
    below += (int)__builtin_popcountll(__ballot(t0 <= b));
  }
  return __builtin_amdgcn_readfirstlane(below - 1);
}

// A claim workgroup takes up to 1024 consecutive positions of ONE run -- four 256-position tiles -- and a wave walks
// its four 64-position chunks in position order, as hash_missing.hip's claim does: the early occurrences of a hot
// missed id have lowered first[] before the later ones read it.
__global__ __launch_bounds__(kBlock) void hash_missing_runs_claim_kernel(const MissRunsArgs a) {
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ri = find_run(a.col, b);
  const Run& r = a.col.run[ri];
  const ColRec& c = a.col.rec[r.col];
  const int64_t n_keys = r.n_keys;
  const int64_t block_first = (int64_t)(b - a.col.run_claim_start[ri]) * kClaimPerBlock;   // in the run; < n_keys
  const int64_t run_first = (int64_t)(r.first_tile - c.tile_first) * kSlotsPerTile;        // the run's first position
  // the run of every 256-position tile this workgroup covers, for count and write: thread j records tile j
  if (threadIdx.x < kChunks && block_first + (int64_t)threadIdx.x * kSlotsPerTile < n_keys) {
    c.tile_run[(run_first + block_first) / kSlotsPerTile + threadIdx.x] = ri;
  }
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int64_t first = block_first + (int64_t)(u * kWavesPerBlock + wave) * kWave;
    if (first >= n_keys) break;   // (wave-uniform)
    const int64_t off = first + lane;
    long long id = kEmptyKey;
    bool miss = false;
    if (off < n_keys && r.slots[off] < 0) {
      id = (long long)r.keys[off];
      miss = holds_key(id, true);
    }
    if (__ballot(miss) == 0ull) continue;   // (wave-uniform) every id of the chunk is resident: no atomic
    if (miss) claim_cell(c.set, c.first, c.cell_mask, id, (int32_t)(run_first + off));   // (positions < 2^31: checked)
  }
}

// What the call reads of a column before any launch: its ids, its non-empty runs, its padded tiles and the tiles
// of its find.  Negative: the column is out of range (the call refuses it; the workspace size counts nothing).
struct Extent {
  int64_t ids;
  int64_t tiles;
  int64_t find_tiles;
  int32_t runs;
};

// (slab_size: checked, or 1 where the find's tiles are not read)
inline bool extent_of(int32_t slab_size, int32_t n_runs, const hbk_hash_run_t* runs, Extent* e) {
  *e = Extent{0, 0, 0, 0};
  if (n_runs < 0 || (n_runs > 0 && runs == nullptr)) return false;
  for (int32_t r = 0; r < n_runs; ++r) {
    const int64_t n = runs[r].n_keys;
    if (n < 0 || n >= (1ll << 31)) return false;
    if (n == 0) continue;
    e->ids += n;
    e->tiles += tiles_of(n);
    e->find_tiles += find_tiles_of(n, slab_size);   // (a run is one part: the ids of a column stay below kKeyLimit)
    ++e->runs;
  }
  return e->ids < kKeyLimit && e->tiles * kSlotsPerTile < (1ll << 31) && e->runs <= kMaxRunsPerLaunch;
}

// the workspace: hash_miss_set.h's, then tile_run[] of all columns
constexpr size_t kTileRunBytes = sizeof(int32_t);

inline Layout layout_of(int32_t n_cols, const int32_t* n_runs, const hbk_hash_run_t* const* runs) {
  Layout l = {0, 0};
  if (n_runs == nullptr || runs == nullptr) return l;
  for (int32_t c = 0; c < n_cols; ++c) {
    Extent e;
    if (!extent_of(1, n_runs[c], runs[c], &e) || e.ids == 0) continue;
    l.cells += cells_of(e.ids);
    l.tiles += e.tiles;
  }
  return l;
}

// the columns [c0, end) of the launch group that starts at c0: up to 32 columns with ids whose non-empty runs
// number at most kMaxRunsPerLaunch together (extents: checked, so one column alone always fits)
inline int32_t group_end(int32_t n_cols, const Extent* extents, int32_t c0) {
  int32_t k = 0, nr = 0, c = c0;
  for (; c < n_cols; ++c) {
    if (extents[c].ids == 0) continue;
    if (k == kMaxColsPerLaunch || nr + extents[c].runs > kMaxRunsPerLaunch) break;
    ++k;
    nr += extents[c].runs;
  }
  return c;
}

}  // namespace
}  // namespace hbk

extern "C" size_t hbk_hash_missing_runs_workspace_bytes(int32_t n_cols, const int32_t* n_runs,
                                                        const hbk_hash_run_t* const* runs) {
  return hbk::layout_of(n_cols, n_runs, runs).bytes(hbk::kTileRunBytes);
}

extern "C" int hbk_hash_missing_runs_n(int32_t n_cols, const hbk_hash_missing_runs_column_t* cols,
                                       const int32_t* n_runs, const hbk_hash_run_t* const* runs, void* workspace,
                                       size_t workspace_bytes, hbk_stream_t stream_) {
  using namespace hbk;
  const char* who = "hash_missing_runs_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(n_cols == 0 || (n_runs != nullptr && runs != nullptr), "%s: n_runs or runs is NULL", who);
  std::vector<Extent> extents((size_t)n_cols);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_missing_runs_column_t& h = cols[c];
    if (int rc = check_geometry(who, c, "", "keys_cache", h.keys_cache, h.slab_count, h.slab_size)) return rc;
    if (int rc = check_column(who, c, h.exp, h.count, h.out_capacity, h.out_ids)) return rc;
    // the rules of hbk_hash_translate_runs_n for an expiring table's runs
    HBK_REQUIRE(n_runs[c] >= 0, "%s: column %d: n_runs must be >= 0, got %d", who, c, n_runs[c]);
    HBK_REQUIRE(n_runs[c] == 0 || runs[c] != nullptr, "%s: column %d: runs is NULL with n_runs = %d", who, c,
                n_runs[c]);
    for (int32_t r = 0; r < n_runs[c]; ++r) {
      const hbk_hash_run_t& run = runs[c][r];
      HBK_REQUIRE(run.n_keys >= 0 && run.n_keys < (1ll << 31),
                  "%s: column %d: run %d: n_keys must be in [0, 2^31), got %lld", who, c, r, (long long)run.n_keys);
      HBK_REQUIRE(run.n_keys == 0 || (run.keys != nullptr && run.slots != nullptr),
                  "%s: column %d: run %d: NULL buffer (keys and slots are needed with n_keys > 0)", who, c, r);
    }
    Extent& e = extents[(size_t)c];
    (void)extent_of(h.slab_size, n_runs[c], runs[c], &e);
    HBK_REQUIRE(e.ids < kKeyLimit, "%s: column %d: the runs sum to %lld keys or more: must stay below 2^30 (the find "
                "of an expiring table takes no more)", who, c, (long long)e.ids);
    HBK_REQUIRE(e.tiles * kSlotsPerTile < (1ll << 31),
                "%s: column %d: n_keys: the runs, each padded to whole tiles of %d, take %lld positions: must stay "
                "below 2^31", who, c, kSlotsPerTile, (long long)(e.tiles * kSlotsPerTile));
    HBK_REQUIRE(e.runs <= kMaxRunsPerLaunch, "%s: column %d: n_runs: %d non-empty runs, a launch takes at most %d",
                who, c, e.runs, kMaxRunsPerLaunch);
  }
  // the find's grid of every launch group, before the first launch
  for (int32_t c0 = 0; c0 < n_cols;) {
    const int32_t c1 = group_end(n_cols, extents.data(), c0);
    int64_t find_tiles = 0;
    for (int32_t c = c0; c < c1; ++c) {
      find_tiles += extents[(size_t)c].find_tiles;
      HBK_REQUIRE(find_tiles < (1ll << 31),
                  "%s: column %d: n_keys: the find of its launch group needs %lld tiles or more, a grid takes fewer "
                  "than 2^31: name fewer ids per call", who, c, (long long)find_tiles);
    }
    c0 = c1;
  }
  const Layout layout = layout_of(n_cols, n_runs, runs);
  hipStream_t stream = as_stream(stream_);
  Workspace ws;
  if (int rc = open_workspace(who, "hbk_hash_missing_runs_workspace_bytes", workspace, workspace_bytes,
                              layout.bytes(kTileRunBytes), layout, stream, &ws)) {
    return rc;
  }
  int32_t* tile_runs = reinterpret_cast<int32_t*>(ws.tiles + layout.tiles);
  for (int32_t c0 = 0; c0 < n_cols;) {
    const int32_t c1 = group_end(n_cols, extents.data(), c0);
    MissRunsArgs args;
    hbk_hash_column_t find_cols[kMaxColsPerLaunch];
    hbk_hash_expiry_t find_exp[kMaxColsPerLaunch];
    int32_t find_n_runs[kMaxColsPerLaunch];
    const hbk_hash_run_t* find_runs[kMaxColsPerLaunch];
    int32_t k = 0, nr = 0;
    int64_t tiles = 0, claim_tiles = 0;
    args.tile_start[0] = 0;
    for (int32_t c = c0; c < c1; ++c) {
      const hbk_hash_missing_runs_column_t& h = cols[c];
      const Extent& e = extents[(size_t)c];
      if (e.ids == 0) {   // an empty id list misses nothing
        HBK_HIP_OK(hipMemsetAsync(h.count, 0, sizeof(int64_t), stream));
        continue;
      }
      describe_find(h, nullptr, nullptr, 0, find_cols + k, find_exp + k);   // (the ids: the runs)
      find_n_runs[k] = n_runs[c];
      find_runs[k] = runs[c];
      const int64_t cells = cells_of(e.ids);
      ColRec& d = args.col.rec[k];
      d.set = ws.set;
      d.first = ws.first;
      d.out_keys = reinterpret_cast<long long*>(h.out_ids);
      d.count = h.count;
      d.tiles = ws.tiles;
      d.tile_run = tile_runs;
      d.out_capacity = h.out_capacity;
      d.n_tiles = e.tiles;
      d.cell_mask = (uint64_t)cells - 1;
      d.tile_first = (int32_t)tiles;
      d.pad_ = 0;
      ws.take(cells, e.tiles);
      tile_runs += e.tiles;
      for (int32_t r = 0; r < n_runs[c]; ++r) {
        const hbk_hash_run_t& run = runs[c][r];
        if (run.n_keys == 0) continue;
        Run& o = args.col.run[nr];
        o.keys = run.keys;
        o.slots = run.slots;
        o.n_keys = run.n_keys;
        o.col = k;
        o.first_tile = (int32_t)tiles;
        args.col.run_claim_start[nr] = (int32_t)claim_tiles;
        tiles += tiles_of(run.n_keys);                                   // (< 2^23 per column: 32 of them fit a grid)
        claim_tiles += (run.n_keys + kClaimPerBlock - 1) / kClaimPerBlock;
        ++nr;
      }
      ++k;
      args.tile_start[k] = (int32_t)tiles;
    }
    c0 = c1;
    if (k == 0) continue;
    args.n_cols = k;
    args.col.n_runs = nr;
    args.col.pad_ = 0;
    if (int rc = hbk_hash_translate_runs_n(k, find_cols, find_exp, nullptr, find_n_runs, find_runs, 0, stream_)) {
      return rc;
    }
    hipLaunchKernelGGL(hash_missing_runs_claim_kernel, dim3((unsigned)claim_tiles), dim3(kBlock), 0, stream, args);
    HBK_HIP_OK(hipGetLastError());
    if (int rc = launch_pack(args, tiles, stream)) return rc;
  }
  return HBK_OK;
}
