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
//          reads) with slots[p] < 0 and an id that is no sentinel puts the id into the column's scratch set and
//          its position into first[] of the id's cell (hash_miss_set.h: claim_cell).  A wave without a miss leaves
//          after reading slots: a batch of resident ids issues no atomic.
//   count, scan, write
//          hash_pack.h's stream compaction over the positions with the selection "p missed and first[cell(id)] ==
//          p": exactly one position per distinct missed id, the first, so the output is in first-occurrence order
//          and a function of the inputs alone.  Ids only: no moves.
//
// The scratch set -- its invariants, why no lane waits for another, its memory rules and the workspace -- is
// hash_miss_set.h's, shared with hash_missing_runs.hip (ids that arrive as runs).  The find reads the key array with
// plain loads: nothing writes it beside it (the call is stream-ordered against the translates, sweeps and backwards
// of its tables, never beside one).
#include "hash_miss_set.h"

namespace hbk {
namespace {

using namespace miss_set;

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
    return first_position(set, first, cell_mask, id) == (int32_t)p;
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
    if (miss) claim_cell(c.set, c.first, c.cell_mask, id, (int32_t)p);   // (positions < 2^31 was checked)
  }
}

// the positions of a column whose counts are in range, else -1
inline int64_t positions_of(const hbk_hash_missing_column_t& h, const hbk_hash_sequence_t* q) {
  if (q == nullptr) return h.n_keys >= 0 && h.n_keys < (1ll << 31) ? h.n_keys : -1;
  if (q->max_len < 1 || q->n_segments < 0 || q->n_segments >= (1ll << 31)) return -1;
  const int64_t positions = q->n_segments * (int64_t)q->max_len;
  return positions < (1ll << 31) ? positions : -1;
}

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
    if (int rc = check_column(who, c, h.exp, h.count, h.out_capacity, h.out_ids)) return rc;
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
  // the find's grid of every launch group, before the first launch
  if (int rc = check_find_grids(who, n_cols, kMaxColsPerLaunch, [&](int32_t c, int32_t* slab_size) {
        *slab_size = cols[c].slab_size;
        return positions_of(cols[c], seq != nullptr ? seq + c : nullptr);
      })) {
    return rc;
  }
  const Layout layout = layout_of(n_cols, cols, seq);
  hipStream_t stream = as_stream(stream_);
  Workspace ws;
  if (int rc = open_workspace(who, "hbk_hash_missing_workspace_bytes", workspace, workspace_bytes, layout.bytes(),
                              layout, stream, &ws)) {
    return rc;
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
      // the find's columns: a sequence column as it is (with every id, also behind T), a flat one in parts
      if (q != nullptr) {
        describe_find(h, h.keys, h.slots, h.n_keys, find_cols + k, find_exp + k);
        find_seq[k] = *q;
      } else {
        n_find += describe_find_parts(h, find_cols + n_find, find_exp + n_find);
      }
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
      d.set = ws.set;
      d.first = ws.first;
      d.out_keys = reinterpret_cast<long long*>(h.out_ids);
      d.out_slots = nullptr;
      d.count = h.count;
      d.tiles = ws.tiles;
      d.capacity = positions;
      d.out_capacity = h.out_capacity;
      d.n_tiles = tiles_of(positions);
      d.cell_mask = (uint64_t)cells - 1;
      d.n_moves = 0;
      d.pad_ = 0;
      d.move[0] = Move{nullptr, nullptr, 0, 0, 0, 0, 0};
      ws.take(cells, d.n_tiles);
      tiles += d.n_tiles;                                             // (< 2^23 per column: 32 of them fit a grid)
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
