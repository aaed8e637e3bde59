// Bounded hash tables (hbk_hash_evict_to_n, hbk_hash_evict_to_lfu_n and their select entries): evict keys of N
// expiring tables down to a size bound, the threshold found on the device.  include/hbk.h has the semantics, and
// hash_order.h the orders: need = live - max_size, cut = the smallest key of the order at or below which at least
// `need` evictable slots lie, and every evictable slot with key <= cut leaves -- whole classes of equal keys
// together, no tie-break.  LruOrder's key is last_seen, LfuOrder's the pair (freq, last_seen) as one 64-bit word.
// Everything below is written once, over the order.
//
// The selection is a radix select over the order's 32-bit halves, each as u = value ^ 0x80000000 (signed order as
// unsigned), most significant digit first, 11 / 11 / 10 bits per half: three digits for LRU, six for LFU.  Per
// digit two kernels, for up to 32 tables per launch:
//   hist  a streaming pass tiled over the slots of all tables as the sweep tiles them: a wave reads 64 consecutive
//         slots with coalesced loads (16 bytes per slot) and counts, in a per-workgroup LDS histogram of 2048 bins,
//         the evictable slots whose higher digits equal the prefix chosen so far (one state word per half: every
//         earlier half whole, and this half's digits so far).  Real last_seen values are small and close together,
//         real freq values pile up on 1 and 2: in most digits every lane of every wave hits ONE bin.  So the
//         wave's lanes that share the leading lane's bin are found with one ballot and added once, as their
//         popcount; only the lanes left over add one by one.  The non-zero bins are then added to the table's
//         histogram with integer atomics: an order-independent sum.  The first pass also counts the live slots.
//   pick  one workgroup per table scans the 2048 bins, finds the bin the remaining need falls into, extends the
//         prefix of its half, writes the need that remains inside that bin, and zeroes the bins for the next pass.
// Then the sweep (hash_common.h: sweep_wave, hash_evict.hip's body) with the predicate "evictable and key <= cut",
// need and cut read from the state.  Every pass after the first leaves at once for a table with need <= 0 or
// whose evictable slots all go.
//
// State per table in the workspace, int32 words: kState words (hash_order.h), then the 2048 bins.  The entry clears
// it on the stream, so a captured call replays.  No host read anywhere.
//
// The select entries are the same call without the sweep: the clear launch and the digit passes, the pick kernels
// instantiated with SELECT, which also write the number of slots the sweep would evict to the report's n_evicted
// word -- the need consumed before the last chosen bin plus that bin's count, or the scan total when all evictable
// slots go.  Nothing of the table is written.
#include "hash_order.h"

namespace hbk {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kChunks = 4;                              // 64-slot chunks per wave
constexpr int kSlotsPerBlock = kBlock * kChunks;
constexpr int kMaxColsPerLaunch = 32;                   // the argument structs travel by value
constexpr int kBins = 2048;                             // 11 bits: 8 KB of LDS
constexpr int kBinsPerThread = kBins / kBlock;
constexpr int kWordsPerTable = kState + kBins;         // (hash_order.h: the state words)

struct ToCol {
  long long* keys;
  int32_t* last_seen;
  int32_t* freq;
  int32_t* stats;         // {n_evicted, n_reused} or NULL
  int32_t* report;        // int32[Order::kReportWords] or NULL
  int32_t* state;         // kWordsPerTable words of the workspace
  int64_t capacity;
  int64_t max_size;
  int32_t keep_freq;
  int32_t n_fills;
};

struct HistArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  ToCol col[kMaxColsPerLaunch];
};

struct SweepArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  ToCol col[kMaxColsPerLaunch];
  Fill fill[kMaxColsPerLaunch][HBK_HASH_MAX_FILLS];
};
static_assert(sizeof(SweepArgs) <= 24576, "kernarg budget");

// the table's state says there is nothing (more) to select
template <class Order>
__device__ inline bool settled(const int32_t* state) { return state[kNeed] <= 0 || state[Order::kAll] != 0; }

// The two walks over an order's halves.  (Functions: written as loops inside the hist kernel they change how its
// unrolled chunk loop is numbered, and with that a handful of its constants.)
// counted, and halves [0, n) of the slot's key equal their finished prefixes
template <class Order>
__device__ inline bool halves_match(bool counted, int n, int32_t freq, int32_t seen, const uint32_t* prefix) {
#pragma unroll
  for (int h = 0; h < n; ++h) counted = counted && Order::half(h, freq, seen) == prefix[h];
  return counted;
}

// the prefix words of the state
template <class Order>
__device__ inline void load_prefix(const int32_t* state, uint32_t* prefix) {
#pragma unroll
  for (int h = 0; h < Order::kHalves; ++h) prefix[h] = (uint32_t)state[Order::kPrefix + h];
}

template <class Order, int DIGIT>
__global__ __launch_bounds__(kBlock) void hash_evict_to_hist_kernel(const HistArgs a) {
  constexpr int kHalf = DIGIT / 3;   // the half this digit cuts
  __shared__ int32_t bins[kBins];
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const ToCol& c = a.col[ci];
  uint32_t prefix[Order::kHalves] = {};
  if (DIGIT > 0) {
    if (settled<Order>(c.state)) return;   // (workgroup-uniform)
    load_prefix<Order>(c.state, prefix);
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
      const uint32_t k = Order::half(kHalf, freq, seen);
      counted = live && (keep_freq == 0 || freq < keep_freq);
      // the higher digits equal the prefix: every earlier half whole, and this half's digits so far
      if constexpr (kHalf > 0) counted = halves_match<Order>(counted, kHalf, freq, seen, prefix);
      if constexpr (DIGIT % 3 != 0) {
        counted = counted && (k >> (digit_shift(DIGIT) + digit_bits(DIGIT))) == prefix[kHalf];
      }
      bin = (int)((k >> digit_shift(DIGIT)) & ((1u << digit_bits(DIGIT)) - 1u));
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

struct PickArgs {
  ToCol col[kMaxColsPerLaunch];
};

// One workgroup per table.  Thread t owns the bins [8 t, 8 t + 8); a scan over the threads' sums finds the one
// thread whose bins the remaining need falls into.
// SELECT: report[kReportEvicted] = the slots a sweep with this cut evicts (the select entries; report is not NULL)
template <class Order, int DIGIT, bool SELECT>
__global__ __launch_bounds__(kBlock) void hash_evict_to_pick_kernel(const PickArgs a) {
  __shared__ int32_t sums[kBlock];
  const ToCol& c = a.col[blockIdx.x];
  int32_t* state = c.state;
  int32_t* hist = state + kState;
  const int t = (int)threadIdx.x;
  int32_t need;
  if (DIGIT == 0) {
    const int32_t live = state[kLive];
    const int64_t wanted = (int64_t)live - c.max_size;   // (live < 2^31, max_size >= 0: fits an int32 once clamped)
    need = wanted < -0x7fffffffll ? -0x7fffffff : (int32_t)wanted;
    // the report opens with zeros behind live and need.  (One thread writes the four words of LruOrder's, eight
    // threads a word each of LfuOrder's: the two forms these kernels had before they were one, kept so that their
    // instructions stay what was measured.)
    if constexpr (Order::kReportWords == 4) {
      if (t == 0) {
        state[kNeed] = need;
        if (c.report != nullptr) {
          c.report[0] = live;
          c.report[1] = need;
          c.report[2] = 0;
          c.report[3] = 0;
        }
      }
    } else {
      if (t == 0) state[kNeed] = need;
      if (c.report != nullptr && t < Order::kReportWords) c.report[t] = t == 0 ? live : t == 1 ? need : 0;
    }
  } else {
    if (settled<Order>(state)) return;   // (workgroup-uniform; the bins were not written by the pass before)
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
      state[Order::kAll] = 1;
#pragma unroll
      for (int h = 0; h < Order::kHalves; ++h) state[Order::kCut + h] = (int32_t)0xffffffffu;
      if (c.report != nullptr) {
#pragma unroll
        for (int h = 0; h < Order::kHalves; ++h) c.report[Order::kReportCut + h] = 0x7fffffff;
      }
      if (SELECT) c.report[Order::kReportEvicted] = sums[kBlock - 1];
    }
    return;
  }
  // (later digits: the chosen bin of the digit before holds at least `need` slots, so one thread matches)
  if (before < need && need <= upto) {
    int32_t run = before;
    int j = 0;
    while (run + v[j] < need) run += v[j++];
    constexpr int kWord = Order::kPrefix + DIGIT / 3;   // the prefix of this digit's half
    const uint32_t prefix = ((DIGIT % 3 == 0 ? 0u : (uint32_t)state[kWord]) << digit_bits(DIGIT)) |
                            (uint32_t)(t * kBinsPerThread + j);
    state[kWord] = (int32_t)prefix;
    state[kRemain] = need - run;
    if (DIGIT == Order::kDigits - 1) {
      uint32_t cut[Order::kHalves];   // the earlier halves' finished prefixes, then this one
#pragma unroll
      for (int h = 0; h < Order::kHalves - 1; ++h) cut[h] = (uint32_t)state[Order::kPrefix + h];
      cut[Order::kHalves - 1] = prefix;
#pragma unroll
      for (int h = 0; h < Order::kHalves; ++h) state[Order::kCut + h] = (int32_t)cut[h];
      if (c.report != nullptr) {
#pragma unroll
        for (int h = 0; h < Order::kHalves; ++h) c.report[Order::kReportCut + h] = (int32_t)(cut[h] ^ 0x80000000u);
      }
      // `need - run` of the whole need is still open in front of the chosen bin: the rest was consumed by the
      // bins below it, over all digits; the chosen bin -- one class of equal keys -- leaves whole
      if (SELECT) c.report[Order::kReportEvicted] = state[kNeed] - (need - run) + v[j];
    }
  }
}

template <class Order>
__global__ __launch_bounds__(kBlock) void hash_evict_to_sweep_kernel(const SweepArgs a) {
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const ToCol& c = a.col[ci];
  if (c.state[kNeed] <= 0) return;   // inside the bound: nothing is written
  const typename Order::Key cut = Order::cut(c.state);
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
                                     Order::key(freq, seen) <= cut;
                            });
  }
  if (lane == 0 && n_evicted != 0) {
    if (c.stats != nullptr) atomicAdd(c.stats, n_evicted);
    if (c.report != nullptr) atomicAdd(c.report + Order::kReportEvicted, n_evicted);
  }
}

// the call's first launch: every table's state and bins start at zero (a kernel, not a memset: it is captured
// into a graph as what it is)
__global__ __launch_bounds__(kBlock) void hash_evict_to_clear_kernel(int32_t* words, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) words[i] = 0;
}

template <class Order, int DIGIT, bool SELECT>
int launch_digit(const HistArgs& hist, const PickArgs& pick, int64_t tiles, hipStream_t stream) {
  hipLaunchKernelGGL((hash_evict_to_hist_kernel<Order, DIGIT>), dim3((unsigned)tiles), dim3(kBlock), 0, stream, hist);
  HBK_HIP_OK(hipGetLastError());
  hipLaunchKernelGGL((hash_evict_to_pick_kernel<Order, DIGIT, SELECT>), dim3((unsigned)hist.n_cols), dim3(kBlock), 0,
                     stream, pick);
  HBK_HIP_OK(hipGetLastError());
  return HBK_OK;
}

// the passes of digit DIGIT and every digit after it
template <class Order, bool SELECT, int DIGIT = 0>
int launch_digits(const HistArgs& hist, const PickArgs& pick, int64_t tiles, hipStream_t stream) {
  if (int rc = launch_digit<Order, DIGIT, SELECT>(hist, pick, tiles, stream)) return rc;
  if constexpr (DIGIT + 1 < Order::kDigits) return launch_digits<Order, SELECT, DIGIT + 1>(hist, pick, tiles, stream);
  return HBK_OK;
}

// the same for every order: kState words and the bins per table
size_t select_workspace_bytes(int32_t n_cols) {
  return n_cols <= 0 ? 0 : (size_t)n_cols * kWordsPerTable * sizeof(int32_t);
}

// every entry: SELECT = the selection alone, no sweep
template <class Order, bool SELECT>
int evict_to(const char* who, int32_t n_cols, const hbk_hash_evict_to_column_t* cols, void* workspace,
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
  const size_t needed = select_workspace_bytes(n_cols);
  HBK_REQUIRE(workspace != nullptr, "%s: workspace is NULL (%zu bytes are needed)", who, needed);
  HBK_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: workspace must be 4-byte aligned", who);
  HBK_REQUIRE(workspace_bytes >= needed, "%s: workspace of %zu bytes is too small: %zu are needed", who,
              workspace_bytes, needed);
  hipStream_t s = as_stream(stream);
  int32_t* words = static_cast<int32_t*>(workspace);
  const int64_t n_words = (int64_t)n_cols * kWordsPerTable;
  const int64_t clear_blocks = (n_words + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(hash_evict_to_clear_kernel, dim3((unsigned)(clear_blocks < 1024 ? clear_blocks : 1024)),
                     dim3(kBlock), 0, s, words, n_words);
  HBK_HIP_OK(hipGetLastError());
  for (int32_t c0 = 0; c0 < n_cols; c0 += kMaxColsPerLaunch) {
    SweepArgs sweep;
    HistArgs hist;
    PickArgs pick;
    const int32_t k = n_cols - c0 < kMaxColsPerLaunch ? n_cols - c0 : kMaxColsPerLaunch;
    int64_t tiles = 0;
    sweep.tile_start[0] = 0;
    for (int32_t i = 0; i < k; ++i) {
      const hbk_hash_evict_to_column_t& h = cols[c0 + i];
      ToCol& d = sweep.col[i];
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
    if (int rc = launch_digits<Order, SELECT>(hist, pick, tiles, s)) return rc;
    if (SELECT) continue;
    hipLaunchKernelGGL(hash_evict_to_sweep_kernel<Order>, dim3((unsigned)tiles), dim3(kBlock), 0, s, sweep);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" size_t hbk_hash_evict_to_workspace_bytes(int32_t n_cols) { return hbk::select_workspace_bytes(n_cols); }

extern "C" size_t hbk_hash_evict_to_lfu_workspace_bytes(int32_t n_cols) {
  return hbk::select_workspace_bytes(n_cols);
}

extern "C" int hbk_hash_evict_to_n(int32_t n_cols, const hbk_hash_evict_to_column_t* cols, void* workspace,
                                   size_t workspace_bytes, hbk_stream_t stream) {
  return hbk::evict_to<hbk::LruOrder, false>("hash_evict_to_n", n_cols, cols, workspace, workspace_bytes, stream);
}

extern "C" int hbk_hash_evict_to_select_n(int32_t n_cols, const hbk_hash_evict_to_column_t* cols, void* workspace,
                                          size_t workspace_bytes, hbk_stream_t stream) {
  return hbk::evict_to<hbk::LruOrder, true>("hash_evict_to_select_n", n_cols, cols, workspace, workspace_bytes, stream);
}

extern "C" int hbk_hash_evict_to_lfu_n(int32_t n_cols, const hbk_hash_evict_to_column_t* cols, void* workspace,
                                       size_t workspace_bytes, hbk_stream_t stream) {
  return hbk::evict_to<hbk::LfuOrder, false>("hash_evict_to_lfu_n", n_cols, cols, workspace, workspace_bytes, stream);
}

extern "C" int hbk_hash_evict_to_lfu_select_n(int32_t n_cols, const hbk_hash_evict_to_column_t* cols, void* workspace,
                                              size_t workspace_bytes, hbk_stream_t stream) {
  return hbk::evict_to<hbk::LfuOrder, true>("hash_evict_to_lfu_select_n", n_cols, cols, workspace, workspace_bytes,
                                            stream);
}
