// Bounded hash tables in LFU order (hbk_hash_evict_to_lfu_n, hbk_hash_evict_to_lfu_select_n, hbk_hash_spill_lfu_n):
// the least frequently used keys of N expiring tables leave down to a size bound, the oldest first among equally
// frequent ones, the threshold found on the device.  include/hbk.h has the semantics: the order is the pair
// (freq, last_seen), both signed, as ONE 64-bit key
//     k(slot) = ((uint64)(freq ^ 0x80000000) << 32) | (uint32)(last_seen ^ 0x80000000)
// need = live - max_size, cut = the smallest k at or below which at least `need` evictable slots lie, and every
// evictable slot with k <= cut leaves -- whole (freq, last_seen) classes together, no tie-break.
//
// The selection is hash_evict_to.hip's radix select carried over 64 bits: six digits, most significant first,
// 11 / 11 / 10 bits over the freq half, then 11 / 11 / 10 over the last_seen half.  Per digit two kernels, for up
// to 32 tables per launch:
//   hist  a streaming pass tiled over the slots of all tables as the sweep tiles them: a wave reads 64 consecutive
//         slots with coalesced loads (16 bytes per slot) and counts, in a per-workgroup LDS histogram of 2048 bins,
//         the evictable slots whose higher digits equal the prefix chosen so far (two state words: the freq half
//         and the last_seen half).  Real freq values pile up on 1 and 2, real steps on a few values: in most
//         digits every lane of every wave hits ONE bin.  So the wave's lanes that share the leading lane's bin are
//         found with one ballot and added once, as their popcount; only the lanes left over add one by one.  The
//         non-zero bins are then added to the table's histogram with integer atomics: an order-independent sum.
//         The first pass also counts the live slots.
//   pick  one workgroup per table scans the 2048 bins, finds the bin the remaining need falls into, extends the
//         prefix of its half, writes the need that remains inside that bin, and zeroes the bins for the next pass.
// Then the sweep (hash_common.h: sweep_wave) with the predicate "need > 0, evictable and k <= cut", need and cut
// read from the state.  Every pass after the first leaves at once for a table with need <= 0 or whose evictable
// slots all go.
//
// State per table in the workspace, int32 words: kState words, then the 2048 bins.  The entry clears it on the
// stream, so a captured call replays.  No host read anywhere.
//
// The report is int32[8]: {live_before, need, cut_freq, cut_last_seen, n_evicted (n_selected), 0, 0, 0}.  The select
// entry is the same call without the sweep, its last pick also writing the number of slots the sweep would evict.
//
// hbk_hash_spill_lfu_n is hash_spill.hip's call with this order: hash_pack.h's count, scan and write instantiated
// with the composite predicate read from the LFU report, then the guarded sweep.
#include "hash_pack.h"

namespace hbk {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kChunks = 4;                              // 64-slot chunks per wave
constexpr int kSlotsPerBlock = kBlock * kChunks;
constexpr int kMaxColsPerLaunch = 32;                   // the argument structs travel by value
constexpr int kBins = 2048;                             // 11 bits: 8 KB of LDS
constexpr int kBinsPerThread = kBins / kBlock;
constexpr int kDigits = 6;
constexpr int kReportWords = 8;

// the state words of a table
constexpr int kLive = 0;        // live slots (hist pass 0)
constexpr int kNeed = 1;        // live - max_size (pick 0); <= 0: the table is left alone
constexpr int kRemain = 2;      // the need that falls into the chosen bin
constexpr int kPrefixHi = 3;    // the digits chosen so far of the freq half, right-aligned; whole after digit 2
constexpr int kPrefixLo = 4;    // ... of the last_seen half (digits 3..5)
constexpr int kAll = 5;         // != 0: fewer evictable slots than need, all of them go (both cuts = INT32_MAX)
constexpr int kCutHi = 6;       // the cut's freq half as u = freq ^ 0x80000000 (pick 5, or pick 0 with kAll)
constexpr int kCutLo = 7;       // the cut's last_seen half as u = last_seen ^ 0x80000000
constexpr int kState = 8;
constexpr int kWordsPerTable = kState + kBins;

// a digit inside its 32-bit half: digits 0..2 cut the freq half, 3..5 the last_seen half
__host__ __device__ constexpr int digit_shift(int digit) { return digit % 3 == 0 ? 21 : digit % 3 == 1 ? 10 : 0; }
__host__ __device__ constexpr int digit_bits(int digit) { return digit % 3 == 2 ? 10 : 11; }

__device__ inline uint32_t order_half(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
__device__ inline uint64_t order_key(int32_t freq, int32_t seen) {
  return ((uint64_t)order_half(freq) << 32) | (uint64_t)order_half(seen);
}

struct LfuCol {
  long long* keys;
  int32_t* last_seen;
  int32_t* freq;
  int32_t* stats;         // {n_evicted, n_reused} or NULL
  int32_t* report;        // int32[8] or NULL
  int32_t* state;         // kWordsPerTable words of the workspace
  int64_t capacity;
  int64_t max_size;
  int32_t keep_freq;
  int32_t n_fills;
};

struct LfuHistArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  LfuCol col[kMaxColsPerLaunch];
};

struct LfuSweepArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  LfuCol col[kMaxColsPerLaunch];
  Fill fill[kMaxColsPerLaunch][HBK_HASH_MAX_FILLS];
};
static_assert(sizeof(LfuSweepArgs) <= 24576, "kernarg budget");

// the table's state says there is nothing (more) to select
__device__ inline bool settled(const int32_t* state) { return state[kNeed] <= 0 || state[kAll] != 0; }

template <int DIGIT>
__global__ __launch_bounds__(kBlock) void hash_evict_lfu_hist_kernel(const LfuHistArgs a) {
  __shared__ int32_t bins[kBins];
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const LfuCol& c = a.col[ci];
  uint32_t prefix_hi = 0, prefix_lo = 0;
  if (DIGIT > 0) {
    if (settled(c.state)) return;   // (workgroup-uniform)
    prefix_hi = (uint32_t)c.state[kPrefixHi];
    prefix_lo = (uint32_t)c.state[kPrefixLo];
  }
  for (int i = (int)threadIdx.x; i < kBins; i += kBlock) bins[i] = 0;
  __syncthreads();
  const int64_t capacity = c.capacity;
  const int32_t keep_freq = c.keep_freq;
  const int64_t block_first = (int64_t)(b - a.tile_start[ci]) * kSlotsPerBlock;
  int32_t n_live = 0;
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int64_t first = block_first + (int64_t)(u * kWavesPerBlock + wave) * kWave;
    if (first >= capacity) break;   // (wave-uniform)
    const int64_t slot = first + lane;
    bool live = false, counted = false;
    int bin = 0;
    if (slot < capacity) {
      const long long key = c.keys[slot];
      const int32_t seen = c.last_seen[slot];
      const int32_t freq = c.freq[slot];
      live = holds_key(key, true);
      const uint32_t hi = order_half(freq), lo = order_half(seen);
      counted = live && (keep_freq == 0 || freq < keep_freq);
      // the higher digits equal the prefix: of the freq half alone, or the whole freq half and the last_seen
      // half's digits so far
      if (DIGIT == 1 || DIGIT == 2) counted = counted && (hi >> (digit_shift(DIGIT) + digit_bits(DIGIT))) == prefix_hi;
      if (DIGIT >= 3) counted = counted && hi == prefix_hi;
      if (DIGIT >= 4) counted = counted && (lo >> (digit_shift(DIGIT) + digit_bits(DIGIT))) == prefix_lo;
      const uint32_t half = DIGIT < 3 ? hi : lo;
      bin = (int)((half >> digit_shift(DIGIT)) & ((1u << digit_bits(DIGIT)) - 1u));
    }
    if (DIGIT == 0) n_live += (int)__builtin_popcountll(__ballot(live));
    const unsigned long long mask = __ballot(counted);
    if (mask == 0ull) continue;   // (wave-uniform)
    // the lanes that share the leading lane's bin: one add of their number
    const int leader = (int)__builtin_ctzll(mask);
    const int lead_bin = __shfl(bin, leader, kWave);
    const unsigned long long same = __ballot(counted && bin == lead_bin);
    if (lane == leader) atomicAdd(&bins[lead_bin], (int32_t)__builtin_popcountll(same));
    if (counted && bin != lead_bin) atomicAdd(&bins[bin], 1);
  }
  if (DIGIT == 0 && lane == 0 && n_live != 0) atomicAdd(&c.state[kLive], n_live);
  __syncthreads();
  int32_t* hist = c.state + kState;
  for (int i = (int)threadIdx.x; i < kBins; i += kBlock) {
    const int32_t v = bins[i];
    if (v != 0) atomicAdd(&hist[i], v);
  }
}

struct LfuPickArgs {
  LfuCol col[kMaxColsPerLaunch];
};

// One workgroup per table.  Thread t owns the bins [8 t, 8 t + 8); a scan over the threads' sums finds the one
// thread whose bins the remaining need falls into.
// SELECT: report[4] = the slots a sweep with this cut evicts (hbk_hash_evict_to_lfu_select_n; the report is not NULL)
template <int DIGIT, bool SELECT>
__global__ __launch_bounds__(kBlock) void hash_evict_lfu_pick_kernel(const LfuPickArgs a) {
  __shared__ int32_t sums[kBlock];
  const LfuCol& c = a.col[blockIdx.x];
  int32_t* state = c.state;
  int32_t* hist = state + kState;
  const int t = (int)threadIdx.x;
  int32_t need;
  if (DIGIT == 0) {
    const int32_t live = state[kLive];
    const int64_t wanted = (int64_t)live - c.max_size;   // (live < 2^31, max_size >= 0: fits an int32 once clamped)
    need = wanted < -0x7fffffffll ? -0x7fffffff : (int32_t)wanted;
    if (t == 0) state[kNeed] = need;
    if (c.report != nullptr && t < kReportWords) c.report[t] = t == 0 ? live : t == 1 ? need : 0;
  } else {
    if (settled(state)) return;   // (workgroup-uniform; the bins were not written by the pass before)
    need = state[kRemain];
  }
  int32_t v[kBinsPerThread];
  int32_t sum = 0;
#pragma unroll
  for (int j = 0; j < kBinsPerThread; ++j) {
    v[j] = hist[t * kBinsPerThread + j];
    hist[t * kBinsPerThread + j] = 0;   // for the next digit's pass
    sum += v[j];
  }
  if (DIGIT == 0 && need <= 0) return;   // (workgroup-uniform)
  sums[t] = sum;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {   // inclusive scan
    const int32_t x = t >= d ? sums[t - d] : 0;
    __syncthreads();
    sums[t] += x;
    __syncthreads();
  }
  const int32_t upto = sums[t], before = upto - sum;
  if (DIGIT == 0 && sums[kBlock - 1] < need) {   // (workgroup-uniform) not enough evictable slots: all of them go
    if (t == 0) {
      state[kAll] = 1;
      state[kCutHi] = (int32_t)0xffffffffu;
      state[kCutLo] = (int32_t)0xffffffffu;
      if (c.report != nullptr) {
        c.report[2] = 0x7fffffff;
        c.report[3] = 0x7fffffff;
      }
      if (SELECT) c.report[4] = sums[kBlock - 1];
    }
    return;
  }
  // (digits 1 to 5: the chosen bin of the digit before holds at least `need` slots, so one thread matches)
  if (before < need && need <= upto) {
    int32_t run = before;
    int j = 0;
    while (run + v[j] < need) run += v[j++];
    constexpr int kWord = DIGIT < 3 ? kPrefixHi : kPrefixLo;
    const uint32_t prefix = ((DIGIT % 3 == 0 ? 0u : (uint32_t)state[kWord]) << digit_bits(DIGIT)) |
                            (uint32_t)(t * kBinsPerThread + j);
    state[kWord] = (int32_t)prefix;
    state[kRemain] = need - run;
    if (DIGIT == kDigits - 1) {
      const uint32_t hi = (uint32_t)state[kPrefixHi];
      state[kCutHi] = (int32_t)hi;
      state[kCutLo] = (int32_t)prefix;
      if (c.report != nullptr) {
        c.report[2] = (int32_t)(hi ^ 0x80000000u);
        c.report[3] = (int32_t)(prefix ^ 0x80000000u);
      }
      // `need - run` of the whole need is still open in front of the chosen bin: the rest was consumed by the
      // bins below it, over all six digits; the chosen bin -- one (freq, last_seen) class -- leaves whole
      if (SELECT) c.report[4] = state[kNeed] - (need - run) + v[j];
    }
  }
}

__global__ __launch_bounds__(kBlock) void hash_evict_lfu_sweep_kernel(const LfuSweepArgs a) {
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const LfuCol& c = a.col[ci];
  if (c.state[kNeed] <= 0) return;   // inside the bound: nothing is written
  const uint64_t cut = ((uint64_t)(uint32_t)c.state[kCutHi] << 32) | (uint64_t)(uint32_t)c.state[kCutLo];
  const int64_t capacity = c.capacity;
  const int32_t keep_freq = c.keep_freq;
  const int64_t block_first = (int64_t)(b - a.tile_start[ci]) * kSlotsPerBlock;
  int32_t n_evicted = 0;
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int64_t first = block_first + (int64_t)(u * kWavesPerBlock + wave) * kWave;
    if (first >= capacity) break;   // (wave-uniform)
    n_evicted += sweep_wave(c.keys, c.last_seen, c.freq, capacity, first, lane, c.n_fills, a.fill[ci],
                            [&](long long key, int32_t seen, int32_t freq) {
                              return holds_key(key, true) && (keep_freq == 0 || freq < keep_freq) &&
                                     order_key(freq, seen) <= cut;
                            });
  }
  if (lane == 0 && n_evicted != 0) {
    if (c.stats != nullptr) atomicAdd(c.stats, n_evicted);
    if (c.report != nullptr) atomicAdd(c.report + 4, n_evicted);
  }
}

// the call's first launch: every table's state and bins start at zero (a kernel, not a memset: it is captured
// into a graph as what it is)
__global__ __launch_bounds__(kBlock) void hash_evict_lfu_clear_kernel(int32_t* words, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) words[i] = 0;
}

template <int DIGIT, bool SELECT>
int launch_digit(const LfuHistArgs& hist, const LfuPickArgs& pick, int64_t tiles, hipStream_t stream) {
  hipLaunchKernelGGL(hash_evict_lfu_hist_kernel<DIGIT>, dim3((unsigned)tiles), dim3(kBlock), 0, stream, hist);
  HBK_HIP_OK(hipGetLastError());
  hipLaunchKernelGGL((hash_evict_lfu_pick_kernel<DIGIT, SELECT>), dim3((unsigned)hist.n_cols), dim3(kBlock), 0,
                     stream, pick);
  HBK_HIP_OK(hipGetLastError());
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" size_t hbk_hash_evict_to_lfu_workspace_bytes(int32_t n_cols) {
  return n_cols <= 0 ? 0 : (size_t)n_cols * hbk::kWordsPerTable * sizeof(int32_t);
}

namespace hbk {
namespace {

// both entries: SELECT = the selection alone, no sweep
template <bool SELECT>
int evict_to_lfu(const char* who, int32_t n_cols, const hbk_hash_evict_to_column_t* cols, void* workspace,
                 size_t workspace_bytes, hbk_stream_t stream) {
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_evict_to_column_t& h = cols[c];
    if (int rc = check_geometry(who, c, "", "keys_cache", h.keys_cache, h.slab_count, h.slab_size)) return rc;
    HBK_REQUIRE(h.slab_count * h.slab_size < (1ll << 31),
                "%s: column %d: slab_count * slab_size = %lld slots, must be below 2^31 (the counters are int32)", who,
                c, (long long)(h.slab_count * h.slab_size));
    HBK_REQUIRE(h.exp.last_seen != nullptr, "%s: column %d: last_seen is NULL", who, c);
    HBK_REQUIRE(h.exp.freq != nullptr, "%s: column %d: freq is NULL", who, c);
    HBK_REQUIRE(h.max_size >= 0, "%s: column %d: max_size must be >= 0, got %lld", who, c, (long long)h.max_size);
    HBK_REQUIRE(h.keep_freq >= 0, "%s: column %d: keep_freq must be >= 0, got %d", who, c, h.keep_freq);
    if (int rc = check_fills(who, c, h.n_fills, h.fills)) return rc;
    HBK_REQUIRE(!SELECT || h.report != nullptr, "%s: column %d: report is NULL", who, c);
  }
  if (n_cols == 0) return HBK_OK;
  const size_t needed = hbk_hash_evict_to_lfu_workspace_bytes(n_cols);
  HBK_REQUIRE(workspace != nullptr, "%s: workspace is NULL (%zu bytes are needed)", who, needed);
  HBK_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: workspace must be 4-byte aligned", who);
  HBK_REQUIRE(workspace_bytes >= needed, "%s: workspace of %zu bytes is too small: %zu are needed", who,
              workspace_bytes, needed);
  hipStream_t s = as_stream(stream);
  int32_t* words = static_cast<int32_t*>(workspace);
  const int64_t n_words = (int64_t)n_cols * kWordsPerTable;
  const int64_t clear_blocks = (n_words + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(hash_evict_lfu_clear_kernel, dim3((unsigned)(clear_blocks < 1024 ? clear_blocks : 1024)),
                     dim3(kBlock), 0, s, words, n_words);
  HBK_HIP_OK(hipGetLastError());
  for (int32_t c0 = 0; c0 < n_cols; c0 += kMaxColsPerLaunch) {
    LfuSweepArgs sweep;
    LfuHistArgs hist;
    LfuPickArgs pick;
    const int32_t k = n_cols - c0 < kMaxColsPerLaunch ? n_cols - c0 : kMaxColsPerLaunch;
    int64_t tiles = 0;
    sweep.tile_start[0] = 0;
    for (int32_t i = 0; i < k; ++i) {
      const hbk_hash_evict_to_column_t& h = cols[c0 + i];
      LfuCol& d = sweep.col[i];
      d.keys = reinterpret_cast<long long*>(h.keys_cache);
      d.last_seen = h.exp.last_seen;
      d.freq = h.exp.freq;
      d.stats = h.exp.stats;
      d.report = h.report;
      d.state = words + (int64_t)(c0 + i) * kWordsPerTable;
      d.capacity = h.slab_count * h.slab_size;
      d.max_size = h.max_size;
      d.keep_freq = h.keep_freq;
      d.n_fills = h.n_fills;
      describe_fills(h.n_fills, h.fills, sweep.fill[i]);
      tiles += (d.capacity + kSlotsPerBlock - 1) / kSlotsPerBlock;   // (< 2^21 per table: 32 of them fit a grid)
      sweep.tile_start[i + 1] = (int32_t)tiles;
      hist.col[i] = d;
      pick.col[i] = d;
    }
    sweep.n_cols = hist.n_cols = k;
    for (int32_t i = 0; i <= k; ++i) hist.tile_start[i] = sweep.tile_start[i];
    if (int rc = launch_digit<0, SELECT>(hist, pick, tiles, s)) return rc;
    if (int rc = launch_digit<1, SELECT>(hist, pick, tiles, s)) return rc;
    if (int rc = launch_digit<2, SELECT>(hist, pick, tiles, s)) return rc;
    if (int rc = launch_digit<3, SELECT>(hist, pick, tiles, s)) return rc;
    if (int rc = launch_digit<4, SELECT>(hist, pick, tiles, s)) return rc;
    if (int rc = launch_digit<5, SELECT>(hist, pick, tiles, s)) return rc;
    if (SELECT) continue;
    hipLaunchKernelGGL(hash_evict_lfu_sweep_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, s, sweep);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_hash_evict_to_lfu_n(int32_t n_cols, const hbk_hash_evict_to_column_t* cols, void* workspace,
                                       size_t workspace_bytes, hbk_stream_t stream) {
  return hbk::evict_to_lfu<false>("hash_evict_to_lfu_n", n_cols, cols, workspace, workspace_bytes, stream);
}

extern "C" int hbk_hash_evict_to_lfu_select_n(int32_t n_cols, const hbk_hash_evict_to_column_t* cols, void* workspace,
                                              size_t workspace_bytes, hbk_stream_t stream) {
  return hbk::evict_to_lfu<true>("hash_evict_to_lfu_select_n", n_cols, cols, workspace, workspace_bytes, stream);
}

// ---- spilling in LFU order ---------------------------------------------------------------------------------------
// hash_spill.hip's four launches with the composite predicate.  selection = the LFU report
// {live_before, need, cut_freq, cut_last_seen, n_selected, ...}, READ FROM DEVICE MEMORY by every launch.
namespace hbk {
namespace {

__device__ inline bool spilled_lfu(const int32_t* selection, int32_t keep_freq, long long key, int32_t seen,
                                   int32_t freq) {
  return holds_key(key, true) && (keep_freq == 0 || freq < keep_freq) && selection[1] > 0 &&
         order_key(freq, seen) <= order_key(selection[2], selection[3]);
}

struct LfuSpillCol {
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
    return spilled_lfu(selection, keep_freq, keys[slot], last_seen[slot], freq[slot]);
  }
  __device__ void scanned() const {
    if (n_evicted != nullptr) *n_evicted = 0;
  }
};

struct LfuSpillArgs {
  int32_t n_cols;
  int32_t tile_start[pack::kMaxColsPerLaunch + 1];
  LfuSpillCol col[pack::kMaxColsPerLaunch];
};
static_assert(sizeof(LfuSpillArgs) <= 24576, "kernarg budget");

struct LfuSpillSweepCol {
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

struct LfuSpillSweepArgs {
  int32_t n_cols;
  int32_t tile_start[pack::kMaxColsPerLaunch + 1];
  LfuSpillSweepCol col[pack::kMaxColsPerLaunch];
};
static_assert(sizeof(LfuSpillSweepArgs) <= 24576, "kernarg budget");

__global__ __launch_bounds__(pack::kBlock) void hash_spill_lfu_sweep_kernel(const LfuSpillSweepArgs a) {
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const LfuSpillSweepCol& c = a.col[ci];
  const int32_t* selection = c.selection;
  if (selection[1] <= 0) return;            // inside the bound: nothing is written
  if (*c.count > c.out_capacity) return;    // not exported in full: the table stays as it is
  const int64_t capacity = c.capacity;
  const int32_t keep_freq = c.keep_freq;
  const int64_t first = (int64_t)(b - a.tile_start[ci]) * pack::kSlotsPerTile + (int64_t)wave * kWave;
  if (first >= capacity) return;   // (wave-uniform)
  const int32_t n = sweep_wave(c.keys, c.last_seen, c.freq, capacity, first, lane, c.n_fills, c.fill,
                               [&](long long key, int32_t seen, int32_t freq) {
                                 return spilled_lfu(selection, keep_freq, key, seen, freq);
                               });
  if (lane == 0 && n != 0) {
    if (c.stats != nullptr) atomicAdd(c.stats, n);
    if (c.n_evicted != nullptr) atomicAdd(c.n_evicted, n);
  }
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_hash_spill_lfu_n(int32_t n_cols, const hbk_hash_spill_column_t* cols, void* workspace,
                                    hbk_stream_t stream) {
  using namespace hbk;
  const char* who = "hash_spill_lfu_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_spill_column_t& h = cols[c];
    if (int rc = check_geometry(who, c, "", "keys_cache", h.keys_cache, h.slab_count, h.slab_size)) return rc;
    HBK_REQUIRE(h.slab_count * h.slab_size < (1ll << 31),
                "%s: column %d: slab_count * slab_size = %lld slots, must be below 2^31 (the counters are int32)", who,
                c, (long long)(h.slab_count * h.slab_size));
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
  if (n_cols == 0) return HBK_OK;
  HBK_REQUIRE(workspace != nullptr, "%s: workspace is NULL (hbk_hash_spill_workspace_bytes says how large)", who);
  HBK_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  int64_t* ws = static_cast<int64_t*>(workspace);
  for (int32_t c0 = 0; c0 < n_cols; c0 += pack::kMaxColsPerLaunch) {
    LfuSpillArgs args;
    LfuSpillSweepArgs sweep;
    const int32_t k = n_cols - c0 < pack::kMaxColsPerLaunch ? n_cols - c0 : pack::kMaxColsPerLaunch;
    int64_t tiles = 0;
    args.tile_start[0] = sweep.tile_start[0] = 0;
    for (int32_t i = 0; i < k; ++i) {
      const hbk_hash_spill_column_t& h = cols[c0 + i];
      LfuSpillCol& d = args.col[i];
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
      d.n_tiles = pack::tiles_of(d.capacity);
      d.keep_freq = h.keep_freq;
      d.n_moves = h.n_moves;
      describe_moves(h.n_moves, h.moves, d.move);
      LfuSpillSweepCol& w = sweep.col[i];
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
    if (int rc = pack::launch_pack(args, tiles, as_stream(stream))) return rc;
    hipLaunchKernelGGL(hash_spill_lfu_sweep_kernel, dim3((unsigned)tiles), dim3(pack::kBlock), 0, as_stream(stream),
                       sweep);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}
