// Hash tables (hbk_hash_rehash_n): growth and tombstone compaction on the device.  One streaming pass over the
// key array of N tables per launch; every key a source slot holds is placed into a fresh, all-EMPTY destination
// key array of any geometry, and its row of every per-slot array named in the call (the embedding row, the
// optimizer slots, last_seen, freq) moves from the source slot to the destination slot in the same launch.
//
// Source sweep (hash_evict.hip's): a wave reads 64 consecutive source slots with coalesced plain loads --
// nobody writes the source during the call -- ballots the slots that hold a key (not EMPTY; not TOMBSTONE when
// `expiring` is set), gathers their lane numbers into the low lanes with rank_below and one ds_permute, and
// lane groups of G = pow2(dst_slab_size) lanes take the live keys in turn, 64 / G per pass.
//
// Placement (hash_insert.hip's plain rule, bit for bit): home slab = murmur3_hash32(key) % dst_slab_count, the
// key takes the slab's FIRST EMPTY slot by a 64-bit agent-scope CAS, a full slab sends it to the next slab,
// wrapping.  The destination never holds a tombstone, so one rule serves both table kinds, and every key is
// found afterwards by hbk_cache_probe and by both translate kernels.  Source keys are distinct, so there is no
// match to look for and a lost CAS always means ANOTHER key took the slot: the same slab is read again.
//
// Memory rules (hash_insert.hip's): every read of dst_keys is a relaxed agent-scope 8-byte atomic load, every
// write of dst_keys the CAS; no fences, no plain stores to the key array.  Rows are copied with plain loads and
// stores by the one group whose CAS won the slot: nobody else knows the slot, and the kernel boundary makes the
// rows visible to the next launch.
//
// Bounded loops: slots only go EMPTY -> key, so at most dst_slab_size lost CASes per slab (`tries`) and at most
// dst_slab_count slabs per key (`probed`), both written out; nothing spins on another workgroup.
//
// Rows travel as 4-byte words, bit for bit.  A move whose two bases, two pitches and width are all multiples
// of 16 bytes is copied with 16-byte accesses.  HBK_REHASH_VEC16=0 builds the 4-byte form alone, for the A/B of
// tools/bench_hash_rehash.py --ab-lib: 494 against 676 us for growth, 517 against 728 us for compaction on 26
// tables x 131 072 slots with five moves (profiles/hash_rehash.txt, "rehash_kernel" against
// "rehash_kernel_ab_lib"), hence 1.
//
// One 64-slot chunk per wave, 64 / G keys per pass, one dependent load -> CAS -> copy chain per key: the launch
// reaches 1.7 TB/s of its byte model, a fifth of the HBM rate (same profile).  It is latency, hidden only by
// occupancy; several keys in flight per lane group, as hash_insert.hip's kKeys, is the open improvement.
#include "common.h"

#ifndef HBK_REHASH_VEC16
#define HBK_REHASH_VEC16 1
#endif

namespace hbk {
namespace {

__host__ __device__ inline uint32_t rotl32_(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// murmur3_hash32<int64, seed 0> as probe.hip and hash_insert.hip: the placement must be theirs, bit for bit
__host__ __device__ inline uint32_t murmur3_i64(int64_t key) {
  const uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
  uint32_t h1 = 0;
  const uint32_t blocks[2] = {(uint32_t)((uint64_t)key & 0xffffffffu), (uint32_t)((uint64_t)key >> 32)};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    uint32_t k1 = blocks[i];
    k1 *= c1;
    k1 = rotl32_(k1, 15);
    k1 *= c2;
    h1 ^= k1;
    h1 = rotl32_(h1, 13);
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

constexpr int kBlock = 256;
constexpr int kSlotsPerBlock = kBlock;                  // one 64-slot chunk per wave: the placement is the work
constexpr int kMaxColsPerLaunch = 32;                   // RehashArgs travels by value
constexpr long long kEmptyKey = (long long)0x8000000000000000ull;
constexpr long long kTombstoneKey = kEmptyKey + 1;

struct Move {
  const uint32_t* src;
  uint32_t* dst;
  int64_t src_pitch;    // words between rows
  int64_t dst_pitch;
  int32_t words;
  int32_t vec16;        // != 0: bases, pitches and words are multiples of 16 bytes
};

struct RehashCol {
  const long long* src_keys;
  long long* dst_keys;
  int64_t* new_slots;   // or NULL
  int32_t* counts;      // {n_moved, n_failed} or NULL
  int64_t src_capacity;
  FastDiv dst_div;      // .d = dst_slab_count
  int32_t dst_slab_size;
  int32_t group_log2;   // pow2(dst_slab_size) lanes per key
  int32_t expiring;
  int32_t n_moves;
  Move move[HBK_HASH_MAX_MOVES];
};

struct RehashArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  RehashCol col[kMaxColsPerLaunch];
};
static_assert(sizeof(RehashArgs) <= 24576, "kernarg budget");

__global__ __launch_bounds__(kBlock) void hash_rehash_kernel(const RehashArgs a) {
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  // last column whose first tile is <= b: one entry per lane, one ballot (hash_insert.hip)
  const int t0 = lane < a.n_cols ? a.tile_start[lane] : 0x7fffffff;
  const int ci = __builtin_amdgcn_readfirstlane((int)__builtin_popcountll(__ballot(t0 <= b)) - 1);
  const RehashCol& c = a.col[ci];
  const int64_t src_capacity = c.src_capacity;
  const int64_t first = (int64_t)(b - a.tile_start[ci]) * kSlotsPerBlock + (int64_t)wave * kWave;
  if (first >= src_capacity) return;   // (wave-uniform)
  const int64_t slot = first + lane;
  const bool in_table = slot < src_capacity;
  long long my_key = kEmptyKey;
  if (in_table) my_key = c.src_keys[slot];
  const bool holds = my_key != kEmptyKey && !(c.expiring != 0 && my_key == kTombstoneKey);
  if (c.new_slots != nullptr && in_table && !holds) c.new_slots[slot] = -1;   // no key there
  const unsigned long long mask = __ballot(holds);
  if (mask == 0ull) return;   // (wave-uniform)
  const int n = (int)__builtin_popcountll(mask);
  // lane r < n receives the lane number of the r-th live slot; the other lanes take what is left, so the
  // permute is a bijection of the wave (hash_evict.hip)
  const int below = rank_below(mask);
  const int dest = holds ? below : n + lane - below;
  const int live_lane = __builtin_amdgcn_ds_permute(dest << 2, lane);

  const int group_log2 = c.group_log2;
  const int gsize = 1 << group_log2;
  const int sub = lane & (gsize - 1);
  const int grp = lane >> group_log2;
  const int gbase = grp << group_log2;
  const int groups_per_wave = kWave >> group_log2;
  const unsigned long long group_mask = (gsize == 64 ? ~0ull : ((1ull << gsize) - 1ull)) << gbase;
  const int32_t slab_size = c.dst_slab_size;
  const int64_t slab_count = (int64_t)c.dst_div.d;
  const bool in_slab = sub < slab_size;
  long long* const cache = c.dst_keys;

  int32_t n_moved = 0, n_failed = 0;
  for (int r0 = 0; r0 < n; r0 += groups_per_wave) {   // (wave-uniform bounds)
    const int r = r0 + grp;
    // (every lane of the wave takes the shuffles)
    const int from = __shfl(live_lane, r & (kWave - 1), kWave);
    const long long key = __shfl(my_key, from, kWave);
    bool active = r < n;
    int64_t slab = (int64_t)fastmod((uint64_t)murmur3_i64((int64_t)key), c.dst_div);
    int64_t result = -1;
    int64_t probed = 0;     // slabs found full: < slab_count
    int32_t tries = 0;      // CASes lost in this slab: <= slab_size (each one a slot somebody else filled)
    long long rk = 0;
    if (active && in_slab) {
      rk = __hip_atomic_load(cache + slab * slab_size + sub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (;;) {
      const unsigned long long empty = __ballot(active && in_slab && rk == kEmptyKey) & group_mask;
      bool advance = false, cas = false;
      int first_empty = 0;
      if (active) {
        if (empty != 0ull) {
          first_empty = __builtin_ctzll(empty) - gbase;
          cas = true;
        } else {
          advance = true;
        }
      }
      // (every lane of the wave takes the shuffle; the CAS is the first EMPTY slot's lane alone)
      long long old = 0;
      if (cas && sub == first_empty) {
        long long expected = kEmptyKey;
        __hip_atomic_compare_exchange_strong(cache + slab * slab_size + first_empty, &expected, key,
                                             __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        old = expected;   // what the slot held: EMPTY when the exchange was made
      }
      old = __shfl(old, gbase + first_empty, kWave);
      if (cas) {
        if (old == kEmptyKey) {
          result = slab * slab_size + first_empty;
          active = false;
        } else if (++tries > slab_size) {
          advance = true;   // (unreachable while slots only go EMPTY -> key: the bound, written out)
        }
        // else: another key took the slot (source keys are distinct) -- re-read the SAME slab
      }
      if (advance) {
        ++probed;
        tries = 0;
        slab = slab + 1 == slab_count ? 0 : slab + 1;
        if (probed >= slab_count) active = false;   // every slab full: -1
      }
      if (!__any(active)) break;
      rk = 0;
      if (active && in_slab) {
        rk = __hip_atomic_load(cache + slab * slab_size + sub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (r < n) {
      const int64_t src_slot = first + from;
      if (result >= 0) {
        // the group that won the slot moves the key's rows; the padding up to the pitch is not written
        for (int m = 0; m < c.n_moves; ++m) {
          const Move& mv = c.move[m];
          const uint32_t* s = mv.src + src_slot * mv.src_pitch;
          uint32_t* d = mv.dst + result * mv.dst_pitch;
#if HBK_REHASH_VEC16
          if (mv.vec16 != 0) {
            const uint4* s4 = reinterpret_cast<const uint4*>(s);
            uint4* d4 = reinterpret_cast<uint4*>(d);
            for (int j = sub; j < (mv.words >> 2); j += gsize) d4[j] = s4[j];
            continue;
          }
#endif
          for (int j = sub; j < mv.words; j += gsize) d[j] = s[j];
        }
      }
      if (sub == 0) {
        if (c.new_slots != nullptr) c.new_slots[src_slot] = result;
        n_moved += result >= 0 ? 1 : 0;
        n_failed += result < 0 ? 1 : 0;
      }
    }
  }
  if (c.counts != nullptr) {
    // one atomic per wave and counter: the lanes' counts summed across the wave
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      n_moved += __shfl_xor(n_moved, off, kWave);
      n_failed += __shfl_xor(n_failed, off, kWave);
    }
    if (lane == 0 && n_moved != 0) atomicAdd(c.counts, n_moved);
    if (lane == 0 && n_failed != 0) atomicAdd(c.counts + 1, n_failed);
  }
}

// the checks of one side's geometry (hash_insert.hip: check_column)
int check_geometry(const char* who, int32_t c, const char* side, const void* keys, int64_t slab_count,
                   int32_t slab_size) {
  HBK_REQUIRE(slab_size >= 1 && slab_size <= kWave, "%s: column %d: %s_slab_size must be in [1, 64], got %d", who, c,
              side, slab_size);
  HBK_REQUIRE(slab_count >= 1, "%s: column %d: %s_slab_count must be >= 1, got %lld", who, c, side,
              (long long)slab_count);
  HBK_REQUIRE(slab_count <= ((1ll << 62) / kWave), "%s: column %d: %s_slab_count %lld is out of range", who, c, side,
              (long long)slab_count);
  HBK_REQUIRE(keys != nullptr, "%s: column %d: %s_keys is NULL", who, c, side);
  HBK_REQUIRE(((uintptr_t)keys & 7) == 0, "%s: column %d: %s_keys must be 8-byte aligned", who, c, side);
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_hash_rehash_n(int32_t n_cols, const hbk_hash_rehash_column_t* cols, hbk_stream_t stream) {
  using namespace hbk;
  const char* who = "hash_rehash_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_rehash_column_t& h = cols[c];
    if (int rc = check_geometry(who, c, "src", h.src_keys, h.src_slab_count, h.src_slab_size)) return rc;
    if (int rc = check_geometry(who, c, "dst", h.dst_keys, h.dst_slab_count, h.dst_slab_size)) return rc;
    HBK_REQUIRE(h.src_keys != h.dst_keys, "%s: column %d: src_keys and dst_keys are the same array (a rehash is "
                "never in place)", who, c);
    HBK_REQUIRE(h.n_moves >= 0 && h.n_moves <= HBK_HASH_MAX_MOVES, "%s: column %d: n_moves must be in [0, %d], got %d",
                who, c, HBK_HASH_MAX_MOVES, h.n_moves);
    for (int32_t m = 0; m < h.n_moves; ++m) {
      const hbk_hash_move_t& mv = h.moves[m];
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
  }
  int32_t c0 = 0;
  while (c0 < n_cols) {
    RehashArgs args;
    int32_t k = 0;
    int64_t tiles = 0;
    args.tile_start[0] = 0;
    while (c0 < n_cols && k < kMaxColsPerLaunch) {
      const hbk_hash_rehash_column_t& h = cols[c0++];
      RehashCol& d = args.col[k];
      d.src_keys = reinterpret_cast<const long long*>(h.src_keys);
      d.dst_keys = reinterpret_cast<long long*>(h.dst_keys);
      d.new_slots = h.new_slots;
      d.counts = h.counts;
      d.src_capacity = h.src_slab_count * h.src_slab_size;
      d.dst_div = make_fastdiv((uint64_t)h.dst_slab_count);
      d.dst_div.d = (uint64_t)h.dst_slab_count;
      d.dst_slab_size = h.dst_slab_size;
      d.group_log2 = 0;
      while ((1 << d.group_log2) < h.dst_slab_size) ++d.group_log2;
      d.expiring = h.expiring;
      d.n_moves = h.n_moves;
      for (int32_t m = 0; m < h.n_moves; ++m) {
        const hbk_hash_move_t& mv = h.moves[m];
        Move& o = d.move[m];
        o.src = static_cast<const uint32_t*>(mv.src);
        o.dst = static_cast<uint32_t*>(mv.dst);
        o.src_pitch = mv.src_pitch > 0 ? mv.src_pitch : mv.words;
        o.dst_pitch = mv.dst_pitch > 0 ? mv.dst_pitch : mv.words;
        o.words = mv.words;
        o.vec16 = (((uintptr_t)mv.src | (uintptr_t)mv.dst) & 15) == 0 &&
                  ((o.src_pitch | o.dst_pitch | (int64_t)mv.words) & 3) == 0;
      }
      tiles += (d.src_capacity + kSlotsPerBlock - 1) / kSlotsPerBlock;
      HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
      ++k;
      args.tile_start[k] = (int32_t)tiles;
    }
    args.n_cols = k;
    hipLaunchKernelGGL(hash_rehash_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, as_stream(stream), args);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}
