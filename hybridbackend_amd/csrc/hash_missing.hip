// Expiring hash tables (hbk_hash_missing_n): the distinct ids of N id lists that their tables do not hold, in the
// order of their first occurrence -- what a fault-in asks the host tier for.  include/hbk.h has the contract.  The
// id list of a column is flat, or (with `seq`) the EFFECTIVE ID LIST of hbk_hash_translate_sequence_n: per sample
// its first min(len, T) ids, then the pad id; ids past T are never read.  The table is not written.
//
// One clear launch per call, then five launches per 32 columns, all on the call's stream:
//   clear  every cell of the call's scratch sets = EMPTY, every first[] = INT32_MAX (plain stores).  The call
//          clears its own workspace, so it asks nothing of what the workspace held and can be captured and replayed.
//   find   the pure find of the expiring table kind, called as it is: hbk_hash_insert_expiring_n with insert == 0,
//          or hbk_hash_translate_sequence_n with insert == 0.  It writes slots.
//   claim  tiled over the POSITIONS, 1024 per tile, a lane owns one.  A position that holds an id (flat: always;
//          sequence: recomputed by position as the sequence translate does, b = p / T by FastDiv and two row_splits
//          reads) with slots[p] < 0 and an id that is no sentinel puts the id into the column's scratch set: open
//          addressing over S = pow2 >= 2 * positions cells (at least 64), home cell = murmur3_i64(id) & (S - 1),
//          linear probing; an EMPTY cell is claimed with a 64-bit agent-scope compare-and-swap.  At the id's cell the
//          lane does atomicMin(first[cell], p).  A lane that finds its id already there does only the atomicMin,
//          and not even that when the first[cell] it reads is already below p (first[] only falls; on a Zipf(1.2)
//          batch the claim and compaction took 285 us with every occurrence's atomic and 185 us with the load:
//          profiles/hash_fault_in.txt).  A wave without a miss leaves after reading slots: a batch of resident ids
//          issues no atomic.
//   count, scan, write
//          hash_pack.h's stream compaction over the positions with the selection "p missed and first[cell(id)] ==
//          p": exactly one position per distinct missed id, the first, so the output is in first-occurrence order
//          and a function of the inputs alone.  Ids only: no moves.
//
// No lane waits for another.  The claim's probe reads at most S cells, the bound written out in the loop: a cell
// only ever goes EMPTY -> id, the distinct ids are at most S / 2, so a lane that loses a swap to ANOTHER id steps to
// the next cell and a lane that loses to its own id is done.  No spin, no retry of a cell.
//
// Memory rules.  The find reads the key array with plain loads: nothing writes it beside it (the call is
// stream-ordered against the translates, sweeps and backwards of its tables, never beside one).  The claim reads
// the set with relaxed agent-scope atomic loads and writes it with the swap and the atomicMin, all served by the
// device's L2 whatever CU issues them; a stale EMPTY read only costs a failed swap, whose returned value is the
// cell's.  The kernel boundary publishes the set: count and write read it (and first[]) with plain loads, as
// hash_insert.hip's find reads a key array nobody writes.
//
// hash_missing_runs.hip (hbk_hash_missing_runs_n) holds a copy of the scratch set -- kMinCells, kNoPosition, cells_of,
// claim_cell, the clear kernel and the walk of selected() -- for ids that arrive as runs: a change of the set's rules
// here is a change there.
#include "hash_pack.h"

namespace hbk {
namespace {

using namespace pack;

constexpr int kChunks = 4;                              // 64-position chunks per wave of the claim
constexpr int kClaimPerBlock = kBlock * kChunks;
constexpr int64_t kFindKeys = (1ll << 30) - 1;          // the find entry takes fewer than 2^30 keys per column
constexpr int kFindParts = 3;                           // n_keys < 2^31: at most three such parts
constexpr int kFindKeysPerGroup = 8;                    // hash_insert.hip's kKeys: a find tile takes (256 / G) * 8 keys
constexpr int64_t kMinCells = 64;
constexpr int32_t kNoPosition = 0x7fffffff;             // first[] of a cell nobody claimed
constexpr int kClearBlocks = 4096;                      // the clear's grid at the most: it strides

// The id list by position.  Flat: position p holds ids[p].  Sequence: hash_insert.hip's seq_key, restated -- the
// sample's t-th id when t < min(len_b, T), else the pad id, else nothing.
struct PosIds {
  const int64_t* ids;
  const int32_t* row_splits;   // [B + 1], or NULL: one id per sample
  int64_t pad_id;
  int64_t n_ids;
  FastDiv len_div;             // .d = T
  int32_t seq;                 // 0: flat
  int32_t has_pad;

  __device__ long long at(int64_t p, bool* there) const {
    *there = true;
    if (seq == 0) return (long long)ids[p];
    const int64_t T = (int64_t)len_div.d;
    const int64_t b = (int64_t)fastdiv((uint64_t)p, len_div);
    const int64_t t = p - b * T;
    int64_t start = b, len = 1;
    if (row_splits != nullptr) {
      start = row_splits[b];
      len = (int64_t)row_splits[b + 1] - start;
    }
    const int64_t L = len < 0 ? 0 : (len < T ? len : T);
    if (t < L && (uint64_t)(start + t) < (uint64_t)n_ids) return (long long)ids[start + t];
    if (has_pad != 0) return (long long)pad_id;
    *there = false;
    return kEmptyKey;
  }
  // (hash_pack.h's write kernel reads the key of a selected slot as keys[slot]: a selected position holds an id)
  __device__ long long operator[](int64_t p) const {
    bool there;
    return at(p, &there);
  }
};

struct MissCol {
  PosIds keys;                // the ids by position
  const int64_t* slots;       // the find's answers
  long long* set;             // workspace [cell_mask + 1]
  int32_t* first;             // workspace [cell_mask + 1]: the smallest position that missed with the cell's id
  long long* out_keys;
  int64_t* out_slots;         // NULL: not wanted
  int64_t* count;
  int64_t* tiles;             // workspace [n_tiles]
  int64_t capacity;           // the positions
  int64_t out_capacity;
  int64_t n_tiles;
  uint64_t cell_mask;         // S - 1
  int32_t n_moves;            // 0: ids only
  int32_t pad_;
  Move move[1];               // (never read)

  // position p missed: it holds an id the table could hold and the find did not see it
  __device__ bool missed(int64_t p, long long* id) const {
    if (slots[p] >= 0) return false;
    bool there;
    *id = keys.at(p, &there);
    return there && holds_key(*id, true);
  }
  __device__ bool selected(int64_t p) const {
    if (p >= capacity) return false;
    long long id;
    if (!missed(p, &id)) return false;
    uint64_t cell = (uint64_t)murmur3_i64((int64_t)id) & cell_mask;
    for (uint64_t k = 0; k <= cell_mask; ++k) {   // (the claim's walk; it ends at the id: every missed id is in the set)
      const long long cur = set[cell];
      if (cur == id) return first[cell] == (int32_t)p;
      if (cur == kEmptyKey) return false;
      cell = (cell + 1) & cell_mask;
    }
    return false;
  }
  __device__ void scanned() const {}
};

struct MissArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];    // 256 positions per tile: count and write
  int32_t claim_start[kMaxColsPerLaunch + 1];   // 1024 positions per tile: the claim
  MissCol col[kMaxColsPerLaunch];
};
static_assert(sizeof(MissArgs) <= 24576, "kernarg budget");

// 16-byte stores: the cells of a call are a multiple of 64 and both arrays start 16-byte aligned
__global__ __launch_bounds__(kBlock) void hash_missing_clear_kernel(longlong2* set, int4* first, int64_t cells) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < (cells >> 1); i += stride) {
    set[i] = make_longlong2(kEmptyKey, kEmptyKey);
    if (i < (cells >> 2)) first[i] = make_int4(kNoPosition, kNoPosition, kNoPosition, kNoPosition);
  }
}

// the id of a missed position into the column's set, its position into first[]: at most S cells are read
__device__ inline void claim_cell(const MissCol& c, long long id, int32_t p) {
  const uint64_t mask = c.cell_mask;
  uint64_t cell = (uint64_t)murmur3_i64((int64_t)id) & mask;
  for (uint64_t k = 0; k <= mask; ++k) {
    long long cur = __hip_atomic_load(c.set + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEmptyKey) {
      long long expected = kEmptyKey;
      const bool won = __hip_atomic_compare_exchange_strong(c.set + cell, &expected, id, __ATOMIC_RELAXED,
                                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      cur = won ? id : expected;   // (lost: the cell's key now, ours or another's)
    }
    if (cur == id) {
      // (first[] only falls: a position not below the value read changes nothing, and a stale read only costs the
      // atomic -- the load spares a hot id's later occurrences their turn at one address)
      if (__hip_atomic_load(c.first + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > p) {
        __hip_atomic_fetch_min(c.first + cell, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      return;
    }
    cell = (cell + 1) & mask;
  }
}

__global__ __launch_bounds__(kBlock) void hash_missing_claim_kernel(const MissArgs a) {
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ci = column_of(a.claim_start, a.n_cols, b, lane);
  const MissCol& c = a.col[ci];
  const int64_t positions = c.capacity;
  const int64_t block_first = (int64_t)(b - a.claim_start[ci]) * kClaimPerBlock;
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int64_t first = block_first + (int64_t)(u * kWavesPerBlock + wave) * kWave;
    if (first >= positions) break;   // (wave-uniform)
    const int64_t p = first + lane;
    long long id = kEmptyKey;
    const bool miss = p < positions && c.missed(p, &id);
    if (__ballot(miss) == 0ull) continue;   // (wave-uniform) every id of the chunk is resident: no atomic
    if (miss) claim_cell(c, id, (int32_t)p);   // (positions < 2^31 was checked)
  }
}

inline int64_t cells_of(int64_t positions) {
  int64_t s = kMinCells;
  while (s < 2 * positions) s <<= 1;
  return s;
}

// the positions of a column whose counts are in range, else -1
inline int64_t positions_of(const hbk_hash_missing_column_t& h, const hbk_hash_sequence_t* q) {
  if (q == nullptr) return h.n_keys >= 0 && h.n_keys < (1ll << 31) ? h.n_keys : -1;
  if (q->max_len < 1 || q->n_segments < 0 || q->n_segments >= (1ll << 31)) return -1;
  const int64_t positions = q->n_segments * (int64_t)q->max_len;
  return positions < (1ll << 31) ? positions : -1;
}

// the workspace: the sets of all columns, first[] of all columns, then the tile counts of all columns
struct Layout {
  int64_t cells;
  int64_t tiles;
  size_t bytes() const { return (size_t)cells * (sizeof(long long) + sizeof(int32_t)) + (size_t)tiles * sizeof(int64_t); }
};

inline Layout layout_of(int32_t n_cols, const hbk_hash_missing_column_t* cols, const hbk_hash_sequence_t* seq) {
  Layout l = {0, 0};
  if (cols == nullptr) return l;
  for (int32_t c = 0; c < n_cols; ++c) {
    const int64_t positions = positions_of(cols[c], seq != nullptr ? seq + c : nullptr);
    if (positions <= 0) continue;
    l.cells += cells_of(positions);
    l.tiles += tiles_of(positions);
  }
  return l;
}

}  // namespace
}  // namespace hbk

extern "C" size_t hbk_hash_missing_workspace_bytes(int32_t n_cols, const hbk_hash_missing_column_t* cols,
                                                   const hbk_hash_sequence_t* seq) {
  return hbk::layout_of(n_cols, cols, seq).bytes();
}

extern "C" int hbk_hash_missing_n(int32_t n_cols, const hbk_hash_missing_column_t* cols,
                                  const hbk_hash_sequence_t* seq, void* workspace, size_t workspace_bytes,
                                  hbk_stream_t stream_) {
  using namespace hbk;
  const char* who = "hash_missing_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_missing_column_t& h = cols[c];
    if (int rc = check_geometry(who, c, "", "keys_cache", h.keys_cache, h.slab_count, h.slab_size)) return rc;
    HBK_REQUIRE(h.exp.last_seen != nullptr, "%s: column %d: last_seen is NULL (expiring tables only)", who, c);
    HBK_REQUIRE(h.exp.freq != nullptr, "%s: column %d: freq is NULL (expiring tables only)", who, c);
    HBK_REQUIRE(h.count != nullptr, "%s: column %d: count is NULL", who, c);
    HBK_REQUIRE(h.out_capacity >= 0, "%s: column %d: out_capacity must be >= 0, got %lld", who, c,
                (long long)h.out_capacity);
    HBK_REQUIRE(h.out_capacity == 0 || h.out_ids != nullptr, "%s: column %d: out_ids is NULL with out_capacity %lld",
                who, c, (long long)h.out_capacity);
    HBK_REQUIRE(h.n_keys >= 0 && h.n_keys < (1ll << 31), "%s: column %d: n_keys must be in [0, 2^31), got %lld", who,
                c, (long long)h.n_keys);
    HBK_REQUIRE(h.n_keys == 0 || h.keys != nullptr, "%s: column %d: keys is NULL with n_keys = %lld", who, c,
                (long long)h.n_keys);
    if (seq == nullptr) {
      HBK_REQUIRE(h.n_keys == 0 || h.slots != nullptr, "%s: column %d: slots is NULL with n_keys = %lld", who, c,
                  (long long)h.n_keys);
      continue;
    }
    // the rules of hbk_hash_translate_sequence_n for an expiring table
    const hbk_hash_sequence_t& q = seq[c];
    HBK_REQUIRE(q.max_len >= 1, "%s: column %d: max_len must be >= 1, got %d", who, c, q.max_len);
    HBK_REQUIRE(q.n_segments >= 0, "%s: column %d: n_segments must be >= 0, got %lld", who, c,
                (long long)q.n_segments);
    HBK_REQUIRE(q.n_segments < (1ll << 30) && q.n_segments * (int64_t)q.max_len < (1ll << 30),
                "%s: column %d: %lld samples x max_len %d positions: must stay below 2^30 (the find of an expiring "
                "table takes no more)", who, c, (long long)q.n_segments, q.max_len);
    HBK_REQUIRE(q.n_segments == 0 || h.slots != nullptr,
                "%s: column %d: slots is NULL (the grid is needed with B * T > 0)", who, c);
    HBK_REQUIRE(q.row_splits != nullptr || h.n_keys == q.n_segments,
                "%s: column %d: row_splits is NULL (one id per sample) but n_keys %lld != n_segments %lld", who, c,
                (long long)h.n_keys, (long long)q.n_segments);
    if (q.has_pad != 0) {
      HBK_REQUIRE(q.pad_id != (int64_t)kEmptyKey, "%s: column %d: pad_id INT64_MIN (EMPTY) is never stored", who, c);
      HBK_REQUIRE(q.pad_id != (int64_t)kTombstoneKey,
                  "%s: column %d: pad_id INT64_MIN + 1 (TOMBSTONE) is never stored in an expiring table", who, c);
    }
  }
  // the find's grid of every launch group, before the first launch (hash_remove.hip: the find entry would notice a
  // grid of 2^31 tiles only at that group's turn)
  {
    int32_t k = 0;
    int64_t find_tiles = 0;
    for (int32_t c = 0; c < n_cols; ++c) {
      const int64_t positions = positions_of(cols[c], seq != nullptr ? seq + c : nullptr);
      if (positions == 0) continue;
      const int64_t per_tile = (int64_t)(kBlock >> pow2_log2(cols[c].slab_size)) * kFindKeysPerGroup;
      for (int64_t at = 0; at < positions; at += kFindKeys) {
        const int64_t part = positions - at < kFindKeys ? positions - at : kFindKeys;
        find_tiles += (part + per_tile - 1) / per_tile;
      }
      HBK_REQUIRE(find_tiles < (1ll << 31),
                  "%s: column %d: n_keys: the find of its launch group (32 columns) needs %lld tiles or more, a grid "
                  "takes fewer than 2^31: name fewer ids per call", who, c, (long long)find_tiles);
      if (++k == kMaxColsPerLaunch) {
        k = 0;
        find_tiles = 0;
      }
    }
  }
  const Layout layout = layout_of(n_cols, cols, seq);
  const size_t need = layout.bytes();
  if (need != 0) {
    HBK_REQUIRE(workspace != nullptr, "%s: workspace is NULL (hbk_hash_missing_workspace_bytes says how large: %zu "
                "bytes)", who, need);
    HBK_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    HBK_REQUIRE(workspace_bytes >= need, "%s: workspace_bytes %zu is too small: %zu bytes are needed", who,
                workspace_bytes, need);
  }
  hipStream_t stream = as_stream(stream_);
  long long* sets = static_cast<long long*>(workspace);
  int32_t* firsts = reinterpret_cast<int32_t*>(sets + layout.cells);      // (cells: a multiple of 64)
  int64_t* tile_ws = reinterpret_cast<int64_t*>(firsts + layout.cells);
  if (layout.cells != 0) {
    const int64_t blocks = ((layout.cells >> 1) + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(hash_missing_clear_kernel, dim3((unsigned)(blocks < kClearBlocks ? blocks : kClearBlocks)),
                       dim3(kBlock), 0, stream, reinterpret_cast<longlong2*>(sets), reinterpret_cast<int4*>(firsts),
                       layout.cells);
    HBK_HIP_OK(hipGetLastError());
  }
  int32_t c0 = 0;
  while (c0 < n_cols) {
    MissArgs args;
    hbk_hash_column_t find_cols[kMaxColsPerLaunch * kFindParts];
    hbk_hash_expiry_t find_exp[kMaxColsPerLaunch * kFindParts];
    hbk_hash_sequence_t find_seq[kMaxColsPerLaunch];
    int32_t k = 0, n_find = 0;
    int64_t tiles = 0, claim_tiles = 0;
    args.tile_start[0] = args.claim_start[0] = 0;
    while (c0 < n_cols && k < kMaxColsPerLaunch) {
      const int32_t c = c0++;
      const hbk_hash_missing_column_t& h = cols[c];
      const hbk_hash_sequence_t* q = seq != nullptr ? seq + c : nullptr;
      const int64_t positions = positions_of(h, q);
      if (positions == 0) {   // an empty id list misses nothing
        HBK_HIP_OK(hipMemsetAsync(h.count, 0, sizeof(int64_t), stream));
        continue;
      }
      // the find's columns: the table as a translate sees it, no table rows, no counters; a flat column of 2^30
      // keys or more goes in parts (the entry's own limit)
      for (int64_t at = 0; at < (q != nullptr ? 1 : positions); at += kFindKeys) {
        hbk_hash_column_t& f = find_cols[n_find];
        f.keys_cache = const_cast<int64_t*>(h.keys_cache);
        f.slab_count = h.slab_count;
        f.slab_size = h.slab_size;
        f.keys = q != nullptr ? h.keys : h.keys + at;
        f.n_keys = q != nullptr ? h.n_keys : (positions - at < kFindKeys ? positions - at : kFindKeys);
        f.slots = q != nullptr ? h.slots : h.slots + at;
        f.counts = nullptr;
        f.table = nullptr;
        f.dim = 0;
        f.table_pitch = 0;
        f.init_scale = 0.0f;
        f.seed = 0;
        hbk_hash_expiry_t& x = find_exp[n_find++];
        x.last_seen = h.exp.last_seen;
        x.freq = h.exp.freq;
        x.step = h.exp.step != nullptr ? h.exp.step : h.exp.last_seen;   // (a find reads no step; its check asks for an address)
        x.stats = nullptr;
      }
      if (q != nullptr) find_seq[k] = *q;
      MissCol& d = args.col[k];
      d.keys.ids = h.keys;
      d.keys.row_splits = q != nullptr ? q->row_splits : nullptr;
      d.keys.pad_id = q != nullptr ? q->pad_id : 0;
      d.keys.n_ids = h.n_keys;
      d.keys.len_div = make_fastdiv((uint64_t)(q != nullptr ? q->max_len : 1));
      d.keys.len_div.d = (uint64_t)(q != nullptr ? q->max_len : 1);
      d.keys.seq = q != nullptr ? 1 : 0;
      d.keys.has_pad = q != nullptr && q->has_pad != 0 ? 1 : 0;
      d.slots = h.slots;
      const int64_t cells = cells_of(positions);
      d.set = sets;
      d.first = firsts;
      d.out_keys = reinterpret_cast<long long*>(h.out_ids);
      d.out_slots = nullptr;
      d.count = h.count;
      d.tiles = tile_ws;
      d.capacity = positions;
      d.out_capacity = h.out_capacity;
      d.n_tiles = tiles_of(positions);
      d.cell_mask = (uint64_t)cells - 1;
      d.n_moves = 0;
      d.pad_ = 0;
      d.move[0] = Move{nullptr, nullptr, 0, 0, 0, 0, 0};
      sets += cells;
      firsts += cells;
      tile_ws += d.n_tiles;
      tiles += d.n_tiles;                                              // (< 2^23 per column: 32 of them fit a grid)
      claim_tiles += (positions + kClaimPerBlock - 1) / kClaimPerBlock;
      ++k;
      args.tile_start[k] = (int32_t)tiles;
      args.claim_start[k] = (int32_t)claim_tiles;
    }
    if (k == 0) continue;
    args.n_cols = k;
    if (seq != nullptr) {
      if (int rc = hbk_hash_translate_sequence_n(k, find_cols, find_exp, nullptr, find_seq, 0, stream_)) return rc;
    } else {
      if (int rc = hbk_hash_insert_expiring_n(n_find, find_cols, find_exp, 0, stream_)) return rc;
    }
    hipLaunchKernelGGL(hash_missing_claim_kernel, dim3((unsigned)claim_tiles), dim3(kBlock), 0, stream, args);
    HBK_HIP_OK(hipGetLastError());
    if (int rc = launch_pack(args, tiles, stream)) return rc;
  }
  return HBK_OK;
}
