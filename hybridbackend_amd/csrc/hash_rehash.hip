// Hash tables (hbk_hash_rehash_n): growth and tombstone compaction on the device.  One streaming pass over the
// key array of N tables per launch; every key a source slot holds is placed into a fresh, all-EMPTY destination
// key array of any geometry, and its row of every per-slot array named in the call (the embedding row, the
// optimizer slots, last_seen, freq) moves from the source slot to the destination slot in the same launch.
//
// Source sweep (hash_evict.hip's): a wave reads 64 consecutive source slots with coalesced plain loads --
// nobody writes the source during the call -- ballots the slots that hold a key (not EMPTY; not TOMBSTONE when
// `expiring` is set), gathers their lane numbers into the low lanes (hash_common.h: compact_lanes), and
// lane groups of G = pow2(dst_slab_size) lanes take the live keys in turn, 64 / G per pass.
//
// Placement (hash_insert.hip's plain rule; the hash is hash_common.h's): home slab = murmur3_i64(key) % dst_slab_count, the
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
// Rows travel as 4-byte words, bit for bit (hash_common.h: Move, copy_row).  A move whose two bases, two pitches
// and width are all multiples of 16 bytes is copied with 16-byte accesses.
//
// One 64-slot chunk per wave, 64 / G keys per pass, one dependent load -> CAS -> copy chain per key: the launch
// reaches 1.7 TB/s of its byte model, a fifth of the HBM rate (same profile).  It is latency, hidden only by
// occupancy; several keys in flight per lane group, as hash_insert.hip's kKeys, is the open improvement.
#include "hash_common.h"

namespace hbk {
namespace {

constexpr int kBlock = 256;
constexpr int kSlotsPerBlock = kBlock;                  // one 64-slot chunk per wave: the placement is the work
constexpr int kMaxColsPerLaunch = 32;                   // RehashArgs travels by value

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
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const RehashCol& c = a.col[ci];
  const int64_t src_capacity = c.src_capacity;
  const int64_t first = (int64_t)(b - a.tile_start[ci]) * kSlotsPerBlock + (int64_t)wave * kWave;
  if (first >= src_capacity) return;   // (wave-uniform)
  const int64_t slot = first + lane;
  const bool in_table = slot < src_capacity;
  long long my_key = kEmptyKey;
  if (in_table) my_key = c.src_keys[slot];
  const bool holds = holds_key(my_key, c.expiring != 0);
  if (c.new_slots != nullptr && in_table && !holds) c.new_slots[slot] = -1;   // no key there
  const unsigned long long mask = __ballot(holds);
  if (mask == 0ull) return;   // (wave-uniform)
  const int n = (int)__builtin_popcountll(mask);
  const int live_lane = compact_lanes(mask, holds, lane);   // lane r < n: the lane of the r-th live slot

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
          copy_row(mv, mv.src + src_slot * mv.src_pitch, mv.dst + result * mv.dst_pitch, sub, gsize);
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

}  // namespace
}  // namespace hbk

extern "C" int hbk_hash_rehash_n(int32_t n_cols, const hbk_hash_rehash_column_t* cols, hbk_stream_t stream) {
  using namespace hbk;
  const char* who = "hash_rehash_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_rehash_column_t& h = cols[c];
    if (int rc = check_geometry(who, c, "src_", "keys", h.src_keys, h.src_slab_count, h.src_slab_size)) return rc;
    if (int rc = check_geometry(who, c, "dst_", "keys", h.dst_keys, h.dst_slab_count, h.dst_slab_size)) return rc;
    HBK_REQUIRE(h.src_keys != h.dst_keys, "%s: column %d: src_keys and dst_keys are the same array (a rehash is "
                "never in place)", who, c);
    if (int rc = check_moves(who, c, h.n_moves, h.moves)) return rc;
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
      d.group_log2 = pow2_log2(h.dst_slab_size);
      d.expiring = h.expiring;
      d.n_moves = h.n_moves;
      describe_moves(h.n_moves, h.moves, d.move);
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
