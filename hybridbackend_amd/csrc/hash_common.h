// The hash tables' contract, once: what probe.hip, hash_insert.hip, hash_evict.hip, hash_rehash.hip and
// hash_export.hip must agree on to read each other's tables -- the sentinels, the placement hash, which slots
// hold a key, the host checks of a table's geometry -- and the pieces their sweeps share: the wave compaction,
// the eviction sweep's body and fills (hash_evict.hip, hash_evict_to.hip, hash_spill.hip; the fills also
// hash_remove.hip's), and the per-slot row moves.  Last, the pure find as a pre-pass of hash_remove.hip,
// hash_missing.hip and hash_missing_runs.hip: its tile size, its grid check and its columns.  (The miss lists'
// scratch set is hash_miss_set.h's.)  Plain constants, structs and inline functions; internal to libhbk_core.so.
#ifndef HBK_CSRC_HASH_COMMON_H_
#define HBK_CSRC_HASH_COMMON_H_

#include <math.h>

#include "common.h"

namespace hbk {

constexpr long long kEmptyKey = (long long)0x8000000000000000ull;   // INT64_MIN: the slot was never taken
constexpr long long kTombstoneKey = kEmptyKey + 1;                   // expiring tables only: the sweep took the slot back

__host__ __device__ inline uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// murmur3_hash32<int64, seed 0> (hybridbackend/common/murmur3.cu.h:32-77): two 4-byte blocks, no tail, len = 8.
// THE placement hash: home slab = murmur3_i64(key) % slab_count for the probe, both translate kernels and the
// rehash, and the mix behind the initial rows and the sketch cells.  hbk_murmur3_hash32 returns this function,
// so the tests that pin that entry to the reference's header pin every placement.
__host__ __device__ inline uint32_t murmur3_i64(int64_t key) {
  const uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
  uint32_t h1 = 0;
  const uint32_t blocks[2] = {(uint32_t)((uint64_t)key & 0xffffffffu), (uint32_t)((uint64_t)key >> 32)};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    uint32_t k1 = blocks[i];
    k1 *= c1;
    k1 = rotl32(k1, 15);
    k1 *= c2;
    h1 ^= k1;
    h1 = rotl32(h1, 13);
    h1 = h1 * 5 + 0xe6546b64u;
  }
  h1 ^= 8u;
  h1 ^= h1 >> 16;
  h1 *= 0x85ebca6bu;
  h1 ^= h1 >> 13;
  h1 *= 0xc2b2ae35u;
  h1 ^= h1 >> 16;
  return h1;
}

// the slot holds a key: not EMPTY, and not TOMBSTONE in a table that has tombstones
__host__ __device__ inline bool holds_key(long long key, bool expiring) {
  return key != kEmptyKey && !(expiring && key == kTombstoneKey);
}

// smallest x with 2^x >= n, at most `cap`: the lanes of the group that owns a slab (slab_size <= 64 was checked)
// or moves a row (cap 6: a wave at the most)
inline int32_t pow2_log2(int32_t n, int32_t cap = 30) {
  int32_t x = 0;
  while (x < cap && (1 << x) < n) ++x;
  return x;
}

// Wave compaction: lane r < popcount(mask) receives the lane number of the r-th flagged lane; the other lanes
// take what is left, so the permute is a bijection of the wave.  mask = __ballot(flagged); every lane calls.
__device__ inline int compact_lanes(unsigned long long mask, bool flagged, int lane) {
  const int below = rank_below(mask);
  const int dest = flagged ? below : (int)__builtin_popcountll(mask) + lane - below;
  return __builtin_amdgcn_ds_permute(dest << 2, lane);
}

// One companion array of a sweep (hbk_hash_fill_t as the kernels take it): the rows of the evicted slots are
// filled with `value`; the padding between dim and pitch is not written.
struct Fill {
  float* base;
  int64_t pitch;        // floats between rows
  int32_t dim;
  int32_t lanes_log2;   // lanes per row of a pass: pow2(dim), at most 64
  float value;
  int32_t pad_;
};

// The companion rows of the n slots a wave has just freed (a sweep's evicted slots, hash_remove.hip's winners),
// filled by all lanes: groups of pow2(dim) lanes, 64 / pow2(dim) rows per pass.  row_of(r), r < 64, is the slot of
// the r-th of them; it may shuffle, so every lane calls it, also for an r it will not fill.
template <class RowOf>
__device__ inline void fill_rows(int n_fills, const Fill* fills, int n, int lane, RowOf row_of) {
  for (int f = 0; f < n_fills; ++f) {
    const Fill& fl = fills[f];
    const int rows_log2 = 6 - fl.lanes_log2;                 // rows per pass
    const int j0 = lane & ((1 << fl.lanes_log2) - 1);
    for (int r0 = 0; r0 < n; r0 += 1 << rows_log2) {
      const int r = r0 + (lane >> fl.lanes_log2);
      const int64_t slot = row_of(r & (kWave - 1));
      if (r < n) {
        float* row = fl.base + slot * fl.pitch;
        for (int j = j0; j < fl.dim; j += 1 << fl.lanes_log2) row[j] = fl.value;
      }
    }
  }
}

// The sweeps' body (hash_evict.hip, hash_evict_to.hip): a wave decides the 64 consecutive slots from `first`
// (wave-uniform, < capacity) with coalesced loads, 16 bytes per slot -- doomed(key, last_seen, freq) is the
// sweep's predicate -- ballots the evicted ones, writes key = TOMBSTONE, last_seen = freq = 0, gathers their lane
// numbers into the low lanes with one permute and fills their companion rows with all lanes: 64 / pow2(dim)
// rows per pass.  Returns the slots evicted (wave-uniform); every lane of the wave calls.
template <class Doomed>
__device__ inline int sweep_wave(long long* keys, int32_t* last_seen, int32_t* freqs, int64_t capacity, int64_t first,
                                 int lane, int n_fills, const Fill* fills, Doomed doomed) {
  const int64_t slot = first + lane;
  bool evict = false;
  if (slot < capacity) {
    const long long key = keys[slot];
    const int32_t seen = last_seen[slot];
    const int32_t freq = freqs[slot];
    evict = doomed(key, seen, freq);
  }
  const unsigned long long mask = __ballot(evict);
  if (mask == 0ull) return 0;   // (wave-uniform)
  const int n = (int)__builtin_popcountll(mask);
  if (evict) {
    keys[slot] = kTombstoneKey;
    last_seen[slot] = 0;
    freqs[slot] = 0;
  }
  if (n_fills == 0) return n;
  const int evicted_lane = compact_lanes(mask, evict, lane);   // lane r < n: the lane of the r-th evicted slot
  fill_rows(n_fills, fills, n, lane, [&](int r) { return first + __shfl(evicted_lane, r, kWave); });
  return n;
}

// the checks of a column's fills: HBK_OK or HBK_INVALID_ARGUMENT
inline int check_fills(const char* who, int32_t c, int32_t n_fills, const hbk_hash_fill_t* fills) {
  HBK_REQUIRE(n_fills >= 0 && n_fills <= HBK_HASH_MAX_FILLS, "%s: column %d: n_fills must be in [0, %d], got %d", who,
              c, HBK_HASH_MAX_FILLS, n_fills);
  for (int32_t f = 0; f < n_fills; ++f) {
    const hbk_hash_fill_t& fl = fills[f];
    HBK_REQUIRE(fl.base != nullptr, "%s: column %d: fill %d: base is NULL", who, c, f);
    HBK_REQUIRE(fl.dim >= 1, "%s: column %d: fill %d: dim must be >= 1, got %d", who, c, f, fl.dim);
    HBK_REQUIRE(fl.pitch == 0 || fl.pitch >= fl.dim, "%s: column %d: fill %d: pitch %d is smaller than dim %d", who,
                c, f, fl.pitch, fl.dim);
    HBK_REQUIRE(isfinite(fl.value), "%s: column %d: fill %d: value must be finite, got %g", who, c, f,
                (double)fl.value);
  }
  return HBK_OK;
}

// checked fills as the kernels take them
inline void describe_fills(int32_t n_fills, const hbk_hash_fill_t* fills, Fill* out) {
  for (int32_t f = 0; f < n_fills; ++f) {
    Fill& fl = out[f];
    fl.base = fills[f].base;
    fl.pitch = fills[f].pitch > 0 ? fills[f].pitch : fills[f].dim;
    fl.dim = fills[f].dim;
    fl.lanes_log2 = pow2_log2(fl.dim, 6);
    fl.value = fills[f].value;
    fl.pad_ = 0;
  }
}

// One per-slot array that travels with the keys (hbk_hash_move_t as the kernels take it).  Rows travel as 4-byte
// words, bit for bit; a move whose two bases, two pitches and width are all multiples of 16 bytes is copied with
// 16-byte accesses.
struct Move {
  const uint32_t* src;
  uint32_t* dst;
  int64_t src_pitch;    // words between rows
  int64_t dst_pitch;
  int32_t words;
  int16_t vec16;        // != 0: bases, pitches and words are multiples of 16 bytes
  int16_t lanes_log2;   // lanes per row of a pass: pow2(accesses per row), at most 64
};

// one row: `words` 4-byte words by the `step` lanes of a group (sub = the lane's place in it); the padding up
// to the pitch is not written
__device__ inline void copy_row(const Move& mv, const uint32_t* s, uint32_t* d, int sub, int step) {
  if (mv.vec16 != 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(s);
    uint4* d4 = reinterpret_cast<uint4*>(d);
    for (int j = sub; j < (mv.words >> 2); j += step) d4[j] = s4[j];
    return;
  }
  for (int j = sub; j < mv.words; j += step) d[j] = s[j];
}

// the checks of a column's moves: HBK_OK or HBK_INVALID_ARGUMENT
inline int check_moves(const char* who, int32_t c, int32_t n_moves, const hbk_hash_move_t* moves) {
  HBK_REQUIRE(n_moves >= 0 && n_moves <= HBK_HASH_MAX_MOVES, "%s: column %d: n_moves must be in [0, %d], got %d", who,
              c, HBK_HASH_MAX_MOVES, n_moves);
  for (int32_t m = 0; m < n_moves; ++m) {
    const hbk_hash_move_t& mv = moves[m];
    HBK_REQUIRE(mv.words >= 1, "%s: column %d: move %d: words must be >= 1, got %d", who, c, m, mv.words);
    HBK_REQUIRE(mv.src_pitch == 0 || mv.src_pitch >= mv.words,
                "%s: column %d: move %d: src_pitch %d is smaller than words %d", who, c, m, mv.src_pitch, mv.words);
    HBK_REQUIRE(mv.dst_pitch == 0 || mv.dst_pitch >= mv.words,
                "%s: column %d: move %d: dst_pitch %d is smaller than words %d", who, c, m, mv.dst_pitch, mv.words);
    HBK_REQUIRE(mv.src != nullptr && mv.dst != nullptr, "%s: column %d: move %d: NULL src or dst", who, c, m);
    HBK_REQUIRE((((uintptr_t)mv.src | (uintptr_t)mv.dst) & 3) == 0,
                "%s: column %d: move %d: src and dst must be 4-byte aligned", who, c, m);
    HBK_REQUIRE(mv.src != mv.dst, "%s: column %d: move %d: src and dst are the same array", who, c, m);
  }
  return HBK_OK;
}

// checked moves as the kernels take them
inline void describe_moves(int32_t n_moves, const hbk_hash_move_t* moves, Move* out) {
  for (int32_t m = 0; m < n_moves; ++m) {
    const hbk_hash_move_t& mv = moves[m];
    Move& o = out[m];
    o.src = static_cast<const uint32_t*>(mv.src);
    o.dst = static_cast<uint32_t*>(mv.dst);
    o.src_pitch = mv.src_pitch > 0 ? mv.src_pitch : mv.words;
    o.dst_pitch = mv.dst_pitch > 0 ? mv.dst_pitch : mv.words;
    o.words = mv.words;
    o.vec16 = (((uintptr_t)mv.src | (uintptr_t)mv.dst) & 15) == 0 &&
              ((o.src_pitch | o.dst_pitch | (int64_t)mv.words) & 3) == 0;
    o.lanes_log2 = (int16_t)pow2_log2(o.vec16 != 0 ? mv.words >> 2 : mv.words, 6);
  }
}

// The checks of a table's geometry.  `prefix` goes before the field names in the messages ("", "src_", "dst_").
// check_slabs: slab size and slab count alone, for the entries with a rule of their own for the key array.
inline int check_slabs(const char* who, int32_t c, const char* prefix, int64_t slab_count, int32_t slab_size) {
  HBK_REQUIRE(slab_size >= 1 && slab_size <= kWave, "%s: column %d: %sslab_size must be in [1, 64], got %d", who, c,
              prefix, slab_size);
  HBK_REQUIRE(slab_count >= 1, "%s: column %d: %sslab_count must be >= 1, got %lld", who, c, prefix,
              (long long)slab_count);
  HBK_REQUIRE(slab_count <= ((1ll << 62) / kWave), "%s: column %d: %sslab_count %lld is out of range", who, c, prefix,
              (long long)slab_count);
  return HBK_OK;
}
// ... and the key array, under the name the entry's struct gives it ("keys", "keys_cache")
inline int check_geometry(const char* who, int32_t c, const char* prefix, const char* keys_name, const void* keys,
                          int64_t slab_count, int32_t slab_size) {
  if (int rc = check_slabs(who, c, prefix, slab_count, slab_size)) return rc;
  HBK_REQUIRE(keys != nullptr, "%s: column %d: %s%s is NULL", who, c, prefix, keys_name);
  HBK_REQUIRE(((uintptr_t)keys & 7) == 0, "%s: column %d: %s%s must be 8-byte aligned", who, c, prefix, keys_name);
  return HBK_OK;
}

// The pure find as a pre-pass (hash_remove.hip, hash_missing.hip, hash_missing_runs.hip): the translate entries of
// hash_insert.hip with insert == 0, called as they are on columns built here.
constexpr int kFindKeysPerGroup = 8;                    // keys per lane group of a translate tile, first reads all in
                                                        // flight (probe.hip): a tile takes (256 / G) * 8 keys
constexpr int64_t kFindKeys = (1ll << 30) - 1;          // the find entry takes fewer than 2^30 keys per column
constexpr int kFindParts = 3;                           // n_keys < 2^31: at most three such parts

// the find's tiles of n keys at this slab size (checked), taken in parts of kFindKeys
inline int64_t find_tiles_of(int64_t n, int32_t slab_size) {
  const int64_t per_tile = (int64_t)(256 >> pow2_log2(slab_size)) * kFindKeysPerGroup;
  int64_t tiles = 0;
  for (int64_t at = 0; at < n; at += kFindKeys) {
    const int64_t part = n - at < kFindKeys ? n - at : kFindKeys;
    tiles += (part + per_tile - 1) / per_tile;
  }
  return tiles;
}

// The find's grid of every launch group -- `group` consecutive columns with keys -- before the first launch: the
// find entry would notice a grid of 2^31 tiles only at that group's turn.  keys_of(c, &slab_size) is the number of
// keys of column c.
template <class KeysOf>
inline int check_find_grids(const char* who, int32_t n_cols, int32_t group, KeysOf keys_of) {
  int32_t k = 0;
  int64_t find_tiles = 0;
  for (int32_t c = 0; c < n_cols; ++c) {
    int32_t slab_size;
    const int64_t n = keys_of(c, &slab_size);
    if (n == 0) continue;
    find_tiles += find_tiles_of(n, slab_size);
    HBK_REQUIRE(find_tiles < (1ll << 31),
                "%s: column %d: n_keys: the find of its launch group (%d columns) needs %lld tiles or more, a grid "
                "takes fewer than 2^31: name fewer ids per call", who, c, group, (long long)find_tiles);
    if (++k == group) {
      k = 0;
      find_tiles = 0;
    }
  }
  return HBK_OK;
}

// The find's column of a table and, with n > 0, n of its ids: the table as a translate sees it, no table rows, no
// counters.  Col: any entry's column struct with keys_cache, slab_count, slab_size and exp.
template <class Col>
inline void describe_find(const Col& h, const int64_t* keys, int64_t* slots, int64_t n, hbk_hash_column_t* f,
                          hbk_hash_expiry_t* x) {
  f->keys_cache = const_cast<int64_t*>(h.keys_cache);   // (a find writes no key)
  f->slab_count = h.slab_count;
  f->slab_size = h.slab_size;
  f->keys = keys;
  f->n_keys = n;
  f->slots = slots;
  f->counts = nullptr;
  f->table = nullptr;
  f->dim = 0;
  f->table_pitch = 0;
  f->init_scale = 0.0f;
  f->seed = 0;
  x->last_seen = h.exp.last_seen;
  x->freq = h.exp.freq;
  x->step = h.exp.step != nullptr ? h.exp.step : h.exp.last_seen;   // (a find reads no step; its check asks for an address)
  x->stats = nullptr;
}

// ... of a flat column (keys, n_keys < 2^31 and slots are h's): 2^30 keys or more go in parts, consecutive ranges of
// the same keys and slots (the entry's own limit).  Returns the parts written, at most kFindParts.
template <class Col>
inline int32_t describe_find_parts(const Col& h, hbk_hash_column_t* f, hbk_hash_expiry_t* x) {
  int32_t parts = 0;
  for (int64_t at = 0; at < h.n_keys; at += kFindKeys, ++parts) {
    describe_find(h, h.keys + at, h.slots + at, h.n_keys - at < kFindKeys ? h.n_keys - at : kFindKeys, f + parts,
                  x + parts);
  }
  return parts;
}

}  // namespace hbk

#endif  // HBK_CSRC_HASH_COMMON_H_
