// Expiring hash tables (hbk_hash_evict_n): the eviction sweep.  One streaming pass over the slots of N
// tables per launch.  A slot whose key is neither EMPTY nor TOMBSTONE is evicted iff
//     steps_to_live > 0  and  (int64)*step - last_seen[slot] >= steps_to_live      (idle long enough)
//     and (keep_freq == 0  or  freq[slot] < keep_freq)                             (not seen often enough to stay)
// An evicted slot's key becomes TOMBSTONE (never EMPTY: hash_insert.hip, the probe's invariant), its freq and
// last_seen become 0 and its row of every companion array named in the call (the optimizer slots) is filled
// with that array's value; the padding between dim and pitch is not written.  The embedding row is left: the
// next key to take the slot writes it.
//
// The sweep is a kernel of its own, stream-ordered against the translate launches and never beside one, so
// the key array is read and written with plain vector loads and stores: nobody else touches it meanwhile, and
// a kernel boundary makes the stores visible to the next launch.
//
// A wave decides 64 consecutive slots with coalesced loads (16 bytes per slot), ballots the evicted ones,
// gathers their lane numbers into the low lanes with one permute, and fills their companion rows with all
// lanes: 64 / pow2(dim) rows per pass (hash_common.h: sweep_wave, the body hash_evict_to.hip's sweep shares).
// n_evicted: one atomic per wave.
#include "hash_common.h"

namespace hbk {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kChunks = 4;                              // 64-slot chunks per wave
constexpr int kSlotsPerBlock = kBlock * kChunks;
constexpr int kMaxColsPerLaunch = 32;                   // EvictArgs travels by value

struct EvictCol {
  long long* keys;
  int32_t* last_seen;
  int32_t* freq;
  const int32_t* step;
  int32_t* stats;         // {n_evicted, n_reused} or NULL
  int64_t capacity;
  int64_t steps_to_live;
  int32_t keep_freq;
  int32_t n_fills;
  Fill fill[HBK_HASH_MAX_FILLS];
};

struct EvictArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  EvictCol col[kMaxColsPerLaunch];
};
static_assert(sizeof(EvictArgs) <= 24576, "kernarg budget");

__global__ __launch_bounds__(kBlock) void hash_evict_kernel(const EvictArgs a) {
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const EvictCol& c = a.col[ci];
  const int64_t capacity = c.capacity;
  const int64_t ttl = c.steps_to_live;
  const int32_t keep_freq = c.keep_freq;
  const int64_t block_first = (int64_t)(b - a.tile_start[ci]) * kSlotsPerBlock;
  if (ttl <= 0) return;   // nothing expires (the host launches nothing for such a column; the rule, written out)
  const int64_t now = (int64_t)*c.step;
  int32_t n_evicted = 0;
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int64_t first = block_first + (int64_t)(u * kWavesPerBlock + wave) * kWave;
    if (first >= capacity) break;   // (wave-uniform)
    n_evicted += sweep_wave(c.keys, c.last_seen, c.freq, capacity, first, lane, c.n_fills, c.fill,
                            [&](long long key, int32_t seen, int32_t freq) {
                              return holds_key(key, true) && now - (int64_t)seen >= ttl &&
                                     (keep_freq == 0 || freq < keep_freq);
                            });
  }
  if (c.stats != nullptr && lane == 0 && n_evicted != 0) atomicAdd(c.stats, n_evicted);
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_hash_evict_n(int32_t n_cols, const hbk_hash_evict_column_t* cols, hbk_stream_t stream) {
  using namespace hbk;
  const char* who = "hash_evict_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_evict_column_t& h = cols[c];
    if (int rc = check_geometry(who, c, "", "keys_cache", h.keys_cache, h.slab_count, h.slab_size)) return rc;
    HBK_REQUIRE(h.exp.last_seen != nullptr && h.exp.freq != nullptr && h.exp.step != nullptr,
                "%s: column %d: NULL expiry buffer (last_seen, freq and step are needed)", who, c);
    HBK_REQUIRE(h.steps_to_live >= 0, "%s: column %d: steps_to_live must be >= 0, got %lld", who, c,
                (long long)h.steps_to_live);
    HBK_REQUIRE(h.keep_freq >= 0, "%s: column %d: keep_freq must be >= 0, got %d", who, c, h.keep_freq);
    if (int rc = check_fills(who, c, h.n_fills, h.fills)) return rc;
  }
  int32_t c0 = 0;
  while (c0 < n_cols) {
    EvictArgs args;
    int32_t k = 0;
    int64_t tiles = 0;
    args.tile_start[0] = 0;
    while (c0 < n_cols && k < kMaxColsPerLaunch) {
      const hbk_hash_evict_column_t& h = cols[c0++];
      if (h.steps_to_live == 0) continue;   // nothing expires
      EvictCol& d = args.col[k];
      d.keys = reinterpret_cast<long long*>(h.keys_cache);
      d.last_seen = h.exp.last_seen;
      d.freq = h.exp.freq;
      d.step = h.exp.step;
      d.stats = h.exp.stats;
      d.capacity = h.slab_count * h.slab_size;
      d.steps_to_live = h.steps_to_live;
      d.keep_freq = h.keep_freq;
      d.n_fills = h.n_fills;
      describe_fills(h.n_fills, h.fills, d.fill);
      tiles += (d.capacity + kSlotsPerBlock - 1) / kSlotsPerBlock;
      HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
      ++k;
      args.tile_start[k] = (int32_t)tiles;
    }
    if (k == 0) continue;
    args.n_cols = k;
    hipLaunchKernelGGL(hash_evict_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, as_stream(stream), args);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}
