// Hash-keyed tables (hbk_hash_insert_n): the WRITER of the slab key cache that probe.hip reads.  Raw
// int64 ids -> row numbers of a fixed-capacity table by find-or-insert, N columns per launch:
//   slab = murmur3_hash32(key) % slab_count
//   the key is in the slab                  -> its slot
//   else the slab has EMPTY slots           -> the FIRST of them is claimed by a 64-bit agent-scope CAS
//   else (the slab is full)                 -> the next slab, wrapping; slab_count full slabs: -1
// so a key never sits behind a slab that still has an EMPTY slot, which is all cache_probe_kernel needs
// to find it.  The reference places missed keys at where(cache_keys == EMPTY)[:n_miss]
// (hbtf/embedding/service.py:212-218): not where its own probe looks.
//
// Lane mapping as cache_probe_kernel: a group of G = pow2(slab_size) adjacent lanes owns one key and
// reads one slab per step; kKeys keys per group with all first reads in flight at once.
//
// Memory rules (per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by
// another CU's stores): inside the inserting kernel EVERY read of the key array is a relaxed agent-scope
// 8-byte atomic load and EVERY write the CAS; no fences, no plain stores to the key array.  A plain load
// could be served from a stale L1 line and make the retry see the same EMPTY slot again.
//
// Bounded loops: slots only ever go EMPTY -> key, so a lost CAS means a slot of the slab was filled by
// somebody else: at most slab_size lost CASes per slab, at most slab_count slabs per key.  Both bounds
// are written out (`tries`, `probed`); nothing spins on another workgroup's progress.
//
// The group whose CAS returned EMPTY is the key's ONE inserter and writes the new row's initial values
// itself: a function of (key, seed, j) alone (include/hbk.h), never of the slot the key happened to get.
//
// Expiring tables (hbk_hash_insert_expiring_n, hash_insert_expiring_kernel below; the kernel above is not
// touched by them).  A second sentinel, TOMBSTONE = INT64_MIN + 1, marks a slot the eviction sweep
// (hash_evict.hip) took back: key -> TOMBSTONE, never -> EMPTY, so a slab without an EMPTY slot stays without
// one and every live key is still found by the probe's walk.  The insert reuses such slots:
//   walk the slabs from the home slab, wrapping, at most slab_count of them:
//       the slab holds the key            -> hit
//       remember the FIRST TOMBSTONE slot of the walk (slab order, then slot order)
//       the slab has an EMPTY slot        -> stop walking
//   claim the remembered TOMBSTONE (CAS TOMBSTONE -> key) if there is one, else the stopping slab's first
//   EMPTY slot (CAS EMPTY -> key), else -1; a claim lost to the same key is a hit on that slot, a claim lost
//   to another key starts the walk again at the home slab.
// The walk goes on PAST a tombstone to the stopping slab before anything is claimed: a key that spilled into
// slab h+1 while h was full is still there after a slot of h was evicted, and claiming the tombstone in h at
// first sight would store that key twice.
//
// One key, concurrent inserters, one slot.  Inside this kernel slots only go free -> key (free = EMPTY or
// TOMBSTONE; the sweep is a kernel of its own, stream-ordered against every translate launch, never beside
// one) and every read is an agent-scope atomic load.  A CAS that succeeds on slot s therefore takes the first
// free slot of the key's walk at that moment: every slot before s was read as filled and stays filled.  A
// second inserter of the same key whose walk covers s reads s either as free -- then s is its own first free
// slot or behind it; its CAS on s loses to the same key, a hit; a CAS on an earlier free slot cannot succeed,
// the first inserter read that slot as filled by another key -- or as the key, a hit.  It cannot read s as
// foreign.
//
// Bounded loops, expiring form: a walk reads at most slab_count slabs (`probed`); a walk is started again
// only after a lost CAS, and each lost CAS is a free slot somebody else filled, of which the table has at most
// slab_count * slab_size (`restarts`, written out).  Nothing waits on another workgroup.
//
// Metadata (insert != 0 only; an occurrence answered -1 touches nothing): every occurrence that resolved to a
// slot stores last_seen[slot] = *step -- all writers of a launch store the same value, plain stores -- and
// adds 1 to freq[slot] with a relaxed agent-scope atomic unless the value it read is already >= 2^30; with
// n_keys < 2^30 per column the counter cannot wrap.
//
// Admission filter (hbk_hash_insert_admit_n, hbk_hash_insert_expiring_admit_n): count, then admit -- the two
// kernels above again, with PHASE 1 and 2.  Phase 1 writes no key, so its walk uses plain loads; its only
// writes besides slots (and an expiring table's metadata of the hits) are relaxed agent-scope adds to the
// sketch, skipped from 2^30 on.  Phase 2 reads slots and the sketch with plain loads -- phase 1 ended at a
// kernel boundary -- and reads the key array as the inserting kernel does, atomically.  A wave of phase 2 whose
// keys were all resolved returns after one coalesced read of slots.  The loops are the ones above, with their
// bounds; the sketch loops run `depth` <= 8 times.  The provisional -2 in slots is overwritten by phase 2 for
// every occurrence that carries it.
//
// Runs (hbk_hash_translate_runs_n): the same kernels with Args = RunsArgs<the entry's Args>.  Only how a tile finds
// its work differs -- its run, by up to four ballots, and through the run its column; everything after that is
// the body above, so the memory rules, the bounds and the one-inserter argument hold unchanged: occurrences of a
// key in different runs of a column are occurrences of that key in one launch.  The instantiations without runs
// are the kernels they were, instruction for instruction.
//
// Sequences (hbk_hash_translate_sequence_n): the same kernels with Args = SeqArgs<the entry's Args>, a third source
// of work, indexed by POSITION of the [B * T] slot grid.  A tile covers positions of one column (found as a
// column's keys are: the column's n_keys is B * T, its slots the grid); a position finds its sample by a FastDiv
// by T, reads the two row_splits entries and takes its key, the pad id or NOTHING.  Nothing is a state of its own
// (`there`), not the EMPTY sentinel by value: a position with nothing is not walked, exactly as a lane past n_keys,
// its slot is written -1 and it counts nowhere, while an id INT64_MIN in the data is -1 counted as failed, as
// everywhere.  The walk is the body above, every lane of the wave in every ballot and shuffle as before.
// Everything new is behind `if constexpr (kSeq)`.
//
// 16-bit tables (hbk_hash_insert_lowp_n): the same kernels with LOWP = true, for the launches that insert.  The walk,
// the claims, the metadata and the counters are the body above; the one difference is init_row, the two kernels' one
// row initialisation: the winning group rounds the fp32 start values to the column's 16 bits (lowp_elems.h, the
// rounding of the apply) and stores whole 4-byte words of two elements.  HashCol has no spare field, so the element
// code rides in the bits of group_log2 above kElemShift, which only the LOWP instantiations mask: the others are
// the kernels they were, instruction for instruction.  A launch that writes no row -- a find, the counting phase of a
// filtered table -- is the fp32 kernel as it is.  hbk_hash_translate_runs_lowp_n and hbk_hash_translate_sequence_lowp_n
// are the same step for the other two sources of work: LOWP = true over RunsArgs / SeqArgs, inserting launches only.
#include <math.h>

#include "hash_common.h"
#include "lowp_elems.h"

namespace hbk {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kMaxColsPerLaunch = 64;   // one ballot finds the column; HashArgs travels by value
constexpr int kKeys = kFindKeysPerGroup;   // keys per lane group, first reads all in flight (probe.hip)

struct HashCol {
  long long* cache;
  const int64_t* keys;
  int64_t* slots;
  int32_t* counts;      // {n_inserted, n_failed} or NULL
  float* table;         // NULL: no row is written (16-bit kernels: 2-byte elements behind it)
  int64_t n_keys;
  FastDiv slab_div;     // .d = slab_count
  int64_t pitch;        // elements between rows
  uint64_t seed;
  float init_scale;
  int32_t slab_size;
  int32_t dim;
  int32_t group_log2;   // 16-bit kernels: bits 0-7; the element code (HBK_LOWP_*) from kElemShift up
};
static_assert(sizeof(HashCol) == 104, "HashCol has no spare field: SeqArgs<ExpiringAdmitArgs> exactly fits 64 columns");

struct HashArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  HashCol col[kMaxColsPerLaunch];
};
static_assert(sizeof(HashArgs) <= 24576, "kernarg budget");

// Keys that arrive as runs (hbk_hash_translate_runs_n): a column's keys are several arrays, each with its own
// slots.  The launch is tiled over the RUNS; a run names its column, whose HashCol.keys / slots / n_keys and
// the tile_start of the base arguments are not read.
constexpr int kMaxRunsPerLaunch = HBK_HASH_MAX_RUNS_PER_LAUNCH;
static_assert(kMaxRunsPerLaunch % kWave == 0, "one ballot per 64 runs");

struct Run {
  const int64_t* keys;
  int64_t* slots;
  int64_t n_keys;
  int32_t col;          // of the launch
  int32_t pad_;
};

template <class Base>
struct RunsArgs : Base {
  int32_t n_runs;
  int32_t run_tile_start[kMaxRunsPerLaunch + 1];
  Run run[kMaxRunsPerLaunch];
};

// What a tile works on -- its run (0 without runs), its column, its place in the column's or run's keys, and
// those keys and their slots -- by the kind of arguments: the column's own for the entries without runs, read
// where the kernels always read them.
template <class Args>
__device__ inline int find_run(const Args&, int) { return 0; }
template <class Args>
__device__ inline int work_column(const Args&, const HashArgs& a, int, int b) {
  return column_of(a.tile_start, a.n_cols, b, lane_id());
}
template <class Args>
__device__ inline int work_tile(const Args&, const HashArgs& a, int, int ci, int b) { return b - a.tile_start[ci]; }
template <class Args>
__device__ inline const int64_t* work_keys(const Args&, const HashCol& c, int) { return c.keys; }
template <class Args>
__device__ inline int64_t* work_slots(const Args&, const HashCol& c, int) { return c.slots; }
template <class Args>
__device__ inline int64_t work_n_keys(const Args&, const HashCol& c, int) { return c.n_keys; }

// last run whose first tile is <= b: column_of (common.h) over up to four 64-wide ballots
template <class Base>
__device__ inline int find_run(const RunsArgs<Base>& r, int b) {
  const int lane = (int)threadIdx.x & (kWave - 1);
  int below = 0;
#pragma unroll
  for (int k = 0; k < kMaxRunsPerLaunch / kWave; ++k) {
    if (k * kWave >= r.n_runs) break;   // (uniform)
    const int i = k * kWave + lane;
    const int t0 = i < r.n_runs ? r.run_tile_start[i] : 0x7fffffff;
    below += (int)__builtin_popcountll(__ballot(t0 <= b));
  }
  return __builtin_amdgcn_readfirstlane(below - 1);
}
template <class Base>
__device__ inline int work_column(const RunsArgs<Base>& r, const HashArgs&, int ri, int) { return r.run[ri].col; }
template <class Base>
__device__ inline int work_tile(const RunsArgs<Base>& r, const HashArgs&, int ri, int, int b) {
  return b - r.run_tile_start[ri];
}
template <class Base>
__device__ inline const int64_t* work_keys(const RunsArgs<Base>& r, const HashCol&, int ri) { return r.run[ri].keys; }
template <class Base>
__device__ inline int64_t* work_slots(const RunsArgs<Base>& r, const HashCol&, int ri) { return r.run[ri].slots; }
template <class Base>
__device__ inline int64_t work_n_keys(const RunsArgs<Base>& r, const HashCol&, int ri) { return r.run[ri].n_keys; }

// Keys that arrive as ragged sequences (hbk_hash_translate_sequence_n): HashCol.n_keys is the POSITIONS of the
// column, B * T, HashCol.slots its slot grid and tile_start tiles the positions; HashCol.keys are the flat ids.
struct SeqCol {
  const int32_t* row_splits;   // [B + 1], or NULL: one id per sample
  int32_t* lengths;            // [B] or NULL
  int64_t pad_id;
  int64_t n_ids;
  FastDiv len_div;             // .d = T
  int32_t has_pad;
  int32_t pad_;
};

template <class Base>
struct SeqArgs : Base {
  SeqCol s[kMaxColsPerLaunch];
};

template <class Args>
struct IsSeq { static constexpr bool value = false; };
template <class Base>
struct IsSeq<SeqArgs<Base>> { static constexpr bool value = true; };

// The id of position p = b * T + t: the sample's t-th id when t < min(len_b, T), else the pad id, else nothing
// (*there = false; the value returned is then not looked at as a key).  Ids at t >= T are never read; row_splits
// that point outside the ids name no id.  The lane that is told to also stores lengths[b] (the one of t == 0).
__device__ inline long long seq_key(const SeqCol& s, const int64_t* ids, int64_t p, bool write_length, bool* there) {
  const int64_t T = (int64_t)s.len_div.d;
  const int64_t b = (int64_t)fastdiv((uint64_t)p, s.len_div);
  const int64_t t = p - b * T;
  int64_t start = b, len = 1;
  if (s.row_splits != nullptr) {
    start = s.row_splits[b];
    len = (int64_t)s.row_splits[b + 1] - start;
  }
  const int64_t L = len < 0 ? 0 : (len < T ? len : T);
  if (write_length && t == 0 && s.lengths != nullptr) s.lengths[b] = (int32_t)L;
  *there = true;
  if (t < L && (uint64_t)(start + t) < (uint64_t)s.n_ids) return (long long)ids[start + t];
  if (s.has_pad != 0) return (long long)s.pad_id;
  *there = false;
  return kEmptyKey;
}

// float j of the initial row of `key` (include/hbk.h): exact in fp32 up to the final multiply
__host__ __device__ inline float init_value(int64_t key, uint64_t seed, int j, float scale) {
  const uint64_t mix = (seed + (uint64_t)j + 1ull) * 0x9E3779B97F4A7C15ull;
  const uint32_t r = murmur3_i64(key ^ (int64_t)mix);
  const float unit = (float)(r >> 8) * 1.1920928955078125e-07f - 1.0f;   // 2^-23: [-1, 1)
  return unit * scale;
}

// The 16-bit kernels (LOWP; hbk_hash_insert_lowp_n) carry the column's element code in the spare bits of
// HashCol.group_log2; the fp32 kernels read the field whole, as they always did.
constexpr int kElemShift = 8;
template <bool LOWP>
__device__ inline int lane_group_log2(const HashCol& c) {
  if constexpr (LOWP) return c.group_log2 & ((1 << kElemShift) - 1);
  return c.group_log2;
}

// The new row of `key` at `slot`, written by the lane group that won the slot (sub = the lane's place in it).
// fp32: one element per lane and pass.  LOWP: the fp32 value rounded to nearest even by lowp_elems.h, whole 4-byte
// words -- word w = elements 2w (low half) and 2w + 1 (high half); dim and the pitch are even and the table 4-byte
// aligned (checked), so no lane writes a partial dword and nothing outside [row, row + dim) is written.
template <bool LOWP>
__device__ inline void init_row(const HashCol& c, long long key, int64_t slot, int sub, int gsize) {
  if constexpr (LOWP) {
    const bool bf16 = (c.group_log2 >> kElemShift) == HBK_LOWP_BF16;
    uint32_t* row = reinterpret_cast<uint32_t*>(reinterpret_cast<uint16_t*>(c.table) + slot * c.pitch);
    for (int w = sub; w < (c.dim >> 1); w += gsize) {
      uint32_t word = 0u;
      if (c.init_scale != 0.0f) {
        const float lo = init_value(key, c.seed, 2 * w, c.init_scale);
        const float hi = init_value(key, c.seed, 2 * w + 1, c.init_scale);
        word = bf16 ? bf16_nearest(lo) | (bf16_nearest(hi) << 16) : fp16_nearest(lo) | (fp16_nearest(hi) << 16);
      }
      row[w] = word;
    }
  } else {
    float* row = c.table + slot * c.pitch;
    for (int j = sub; j < c.dim; j += gsize) {
      row[j] = c.init_scale == 0.0f ? 0.0f : init_value(key, c.seed, j, c.init_scale);
    }
  }
}

constexpr int32_t kFreqCeiling = 1 << 30;   // of freq and of the sketch's counters
constexpr int64_t kPending = -2;            // slots[i] between the two phases of an admitting call: not resolved yet

// The admission filter of one column (hbk_hash_admission_t): a count-min sketch, row r at sketch + r * width.
struct AdmitCol {
  int32_t* sketch;
  int32_t* filtered;    // or NULL
  FastDiv width_div;    // .d = width
  uint64_t seed;
  int32_t depth;
  int32_t min_freq;
};

struct AdmitArgs {
  HashArgs h;
  AdmitCol f[kMaxColsPerLaunch];
};
static_assert(sizeof(AdmitArgs) <= 24576, "kernarg budget");

__device__ inline const HashArgs& hash_args(const HashArgs& a) { return a; }
__device__ inline const HashArgs& hash_args(const AdmitArgs& a) { return a.h; }

// the cell of `key` in row r of the sketch: the mix of init_value
__device__ inline int32_t* sketch_cell(const AdmitCol& f, long long key, int r) {
  const uint64_t mix = (f.seed + (uint64_t)r + 1ull) * 0x9E3779B97F4A7C15ull;
  const uint64_t cell = fastmod((uint64_t)murmur3_i64((int64_t)key ^ (int64_t)mix), f.width_div);
  return f.sketch + (uint64_t)r * f.width_div.d + cell;
}

// Phase 1 of an admitting call, for a key its walk did not find: 1 to each of its cells, the lanes of the
// group taking the rows in turn; skipped at the ceiling (the rule of freq).
__device__ inline void sketch_count(const AdmitCol& f, long long key, int sub, int gsize) {
  for (int r = sub; r < f.depth; r += gsize) {
    int32_t* cell = sketch_cell(f, key, r);
    if (*cell < kFreqCeiling) __hip_atomic_fetch_add(cell, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Phase 2: min over the key's cells, plain loads (phase 1 ended at a kernel boundary).  Every lane of the wave
// takes the shuffles; the lanes of a group whose key is not `wanted` read nothing.
__device__ inline int32_t sketch_estimate(const AdmitCol& f, long long key, bool wanted, int sub, int gsize) {
  int32_t est = 0x7fffffff;
  if (wanted) {
    for (int r = sub; r < f.depth; r += gsize) est = min(est, *sketch_cell(f, key, r));
  }
  for (int off = 1; off < gsize; off <<= 1) est = min(est, __shfl_xor(est, off, kWave));
  return est;
}

template <bool INSERT>
__device__ inline long long read_slot(const long long* p) {
  if (INSERT) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}

// PHASE 0: the entries without a filter (Args = HashArgs).  PHASE 1 / 2 (Args = AdmitArgs): the two launches of
// an admitting call -- 1 = the find walk, the sketch adds of its misses, kPending into their slots; 2 = the
// find-or-insert of the pending occurrences whose estimate reaches min_freq, -1 for the others.  Everything the
// phases add is behind `if constexpr`: the PHASE 0 instantiations are the kernels they were.
template <bool INSERT, int PHASE = 0, class Args = HashArgs, bool LOWP = false>
__global__ __launch_bounds__(kBlock) void hash_insert_kernel(const Args args) {
  static_assert(PHASE == 0 || INSERT == (PHASE == 2), "phase 1 finds, phase 2 inserts");
  static_assert(INSERT || !LOWP, "only an inserting launch writes rows: a find of a 16-bit table is the fp32 find");
  constexpr bool kSeq = IsSeq<Args>::value;
  const HashArgs& a = hash_args(args);
  const int b = (int)blockIdx.x;
  const int ri = find_run(args, b);
  const int ci = work_column(args, a, ri, b);
  const HashCol& c = a.col[ci];
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int group_log2 = lane_group_log2<LOWP>(c);
  const int gsize = 1 << group_log2;
  const int sub = lane & (gsize - 1);
  const int grp = lane >> group_log2;
  const int gbase = grp << group_log2;
  const int groups_per_wave = kWave >> group_log2;
  const int64_t wave_in_col = (int64_t)work_tile(args, a, ri, ci, b) * kWavesPerBlock + wave;
  const int64_t first_key = wave_in_col * groups_per_wave * kKeys;
  const int64_t n_keys = work_n_keys(args, c, ri);
  if (first_key >= n_keys) return;   // (wave-uniform)
  const int64_t i0 = first_key + grp;   // + u * groups_per_wave
  const unsigned long long group_mask = (gsize == 64 ? ~0ull : ((1ull << gsize) - 1ull)) << gbase;
  const int32_t slab_size = c.slab_size;
  const int64_t slab_count = (int64_t)c.slab_div.d;
  const bool in_slab = sub < slab_size;
  long long* const cache = c.cache;

  long long key[kKeys], read_key[kKeys];
  int64_t slab[kKeys];
  [[maybe_unused]] bool pending[kKeys], admitted[kKeys];   // (PHASE 2)
  [[maybe_unused]] bool there[kKeys];                      // (sequences) the position holds an id: a key or the pad id
  if constexpr (PHASE == 2) {
    // one coalesced read of the answers of phase 1: a wave with nothing pending leaves here
    bool any = false;
#pragma unroll
    for (int u = 0; u < kKeys; ++u) {
      const int64_t i = i0 + (int64_t)u * groups_per_wave;
      pending[u] = i < n_keys && work_slots(args, c, ri)[i] == kPending;
      any |= pending[u];
    }
    if (!__any(any)) return;
  }
#pragma unroll
  for (int u = 0; u < kKeys; ++u) {
    const int64_t i = i0 + (int64_t)u * groups_per_wave;
    if constexpr (kSeq) {
      // (phase 2 reads what phase 1 read; the lengths were written by phase 1)
      const bool wanted = PHASE == 2 ? pending[u] : i < n_keys;
      there[u] = false;
      key[u] = kEmptyKey;
      if (wanted) key[u] = seq_key(args.s[ci], c.keys, i, PHASE != 2 && sub == 0, &there[u]);
    } else if constexpr (PHASE == 2) {
      key[u] = pending[u] ? (long long)work_keys(args, c, ri)[i] : kEmptyKey;
    } else {
      key[u] = i < n_keys ? (long long)work_keys(args, c, ri)[i] : kEmptyKey;
    }
  }
  if constexpr (PHASE == 2) {
#pragma unroll
    for (int u = 0; u < kKeys; ++u) {
      admitted[u] = sketch_estimate(args.f[ci], key[u], pending[u], sub, gsize) >= args.f[ci].min_freq && pending[u];
      if (!admitted[u]) key[u] = kEmptyKey;   // not walked: -1, counted in `filtered`
    }
  }
#pragma unroll
  for (int u = 0; u < kKeys; ++u) {
    slab[u] = (int64_t)fastmod((uint64_t)murmur3_i64(key[u]), c.slab_div);
    read_key[u] = 0;
    // (EMPTY is never looked for: the lanes past n_keys hold it too)
    if (key[u] != kEmptyKey && in_slab) read_key[u] = read_slot<INSERT>(cache + slab[u] * slab_size + sub);
  }
  int32_t n_inserted = 0, n_failed = 0, n_filtered = 0;
#pragma unroll
  for (int u = 0; u < kKeys; ++u) {
    const int64_t i = i0 + (int64_t)u * groups_per_wave;
    bool active = key[u] != kEmptyKey;
    bool won = false;
    int64_t result = -1;
    int64_t probed = 0;     // slabs found full: < slab_count
    int32_t tries = 0;      // CASes lost in this slab: <= slab_size (each one a slot somebody else filled)
    long long rk = read_key[u];
    for (;;) {
      const bool live = active && in_slab;
      const unsigned long long match = __ballot(live && rk == key[u]) & group_mask;
      const unsigned long long empty = __ballot(live && rk == kEmptyKey) & group_mask;
      bool advance = false, cas = false;
      int first = 0;
      if (active) {
        if (match != 0ull) {
          result = slab[u] * slab_size + (__builtin_ctzll(match) - gbase);
          active = false;
        } else if (empty != 0ull) {
          first = __builtin_ctzll(empty) - gbase;
          if (INSERT) cas = true; else active = false;
        } else {
          advance = true;
        }
      }
      if (INSERT) {
        // (every lane of the wave takes the shuffle; the CAS is the first EMPTY slot's lane alone)
        long long old = 0;
        if (cas && sub == first) {
          long long expected = kEmptyKey;
          __hip_atomic_compare_exchange_strong(cache + slab[u] * slab_size + first, &expected, key[u],
                                               __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          old = expected;   // what the slot held: EMPTY when the exchange was made
        }
        old = __shfl(old, gbase + first, kWave);
        if (cas) {
          if (old == kEmptyKey || old == key[u]) {
            // inserted, or a concurrent duplicate of the key won this slot: a hit on it
            won = old == kEmptyKey;
            result = slab[u] * slab_size + first;
            active = false;
          } else if (++tries > slab_size) {
            advance = true;   // (unreachable while slots only go EMPTY -> key: the bound, written out)
          }
          // else: re-read the SAME slab -- a match first, then its first EMPTY slot
        }
      }
      if (advance) {
        ++probed;
        tries = 0;
        slab[u] = slab[u] + 1 == slab_count ? 0 : slab[u] + 1;
        if (probed >= slab_count) active = false;
      }
      if (!__any(active)) break;
      rk = 0;
      if (active && in_slab) rk = read_slot<INSERT>(cache + slab[u] * slab_size + sub);
    }
    if (INSERT && won && c.table != nullptr) init_row<LOWP>(c, key[u], result, sub, gsize);
    if constexpr (PHASE == 1) {
      // not found and not the sentinel (which stays -1, counted as failed): counted, decided in phase 2
      if (result < 0 && key[u] != kEmptyKey) {
        sketch_count(args.f[ci], key[u], sub, gsize);
        result = kPending;
      }
    }
    if constexpr (PHASE == 2) {
      if (pending[u] && sub == 0) {
        work_slots(args, c, ri)[i] = result;
        n_inserted += won ? 1 : 0;
        n_failed += admitted[u] && result < 0 ? 1 : 0;
        n_filtered += admitted[u] ? 0 : 1;
      }
    } else if (i < n_keys && sub == 0) {
      work_slots(args, c, ri)[i] = result;
      n_inserted += won ? 1 : 0;
      if constexpr (kSeq) {
        n_failed += there[u] && (PHASE == 1 ? result == -1 : result < 0) ? 1 : 0;   // nothing here: not a failure
      } else {
        n_failed += (PHASE == 1 ? result == -1 : result < 0) ? 1 : 0;
      }
    }
  }
  if (c.counts != nullptr) {
    // one atomic per wave and counter: the lanes' counts summed across the wave
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      n_inserted += __shfl_xor(n_inserted, off, kWave);
      n_failed += __shfl_xor(n_failed, off, kWave);
    }
    if (lane == 0 && n_inserted != 0) atomicAdd(c.counts, n_inserted);
    if (lane == 0 && n_failed != 0) atomicAdd(c.counts + 1, n_failed);
  }
  if constexpr (PHASE == 2) {
    if (args.f[ci].filtered != nullptr) {
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) n_filtered += __shfl_xor(n_filtered, off, kWave);
      if (lane == 0 && n_filtered != 0) atomicAdd(args.f[ci].filtered, n_filtered);
    }
  }
}

struct ExpiryCol {
  int32_t* last_seen;
  int32_t* freq;
  const int32_t* step;
  int32_t* stats;       // {n_evicted, n_reused} or NULL
};

struct ExpiringArgs {
  HashArgs h;
  ExpiryCol e[kMaxColsPerLaunch];
};
static_assert(sizeof(ExpiringArgs) <= 24576, "kernarg budget");

struct ExpiringAdmitArgs {
  ExpiringArgs x;
  AdmitCol f[kMaxColsPerLaunch];
};
static_assert(sizeof(ExpiringAdmitArgs) <= 24576, "kernarg budget");

__device__ inline const ExpiringArgs& expiring_args(const ExpiringArgs& x) { return x; }
__device__ inline const ExpiringArgs& expiring_args(const ExpiringAdmitArgs& x) { return x.x; }

// The sibling of hash_insert_kernel for expiring tables: same lane mapping and first reads, the placement
// rule with tombstones of the header comment.  PHASE as in hash_insert_kernel (Args = ExpiringAdmitArgs for 1 and
// 2); the metadata of an occurrence is written by the phase that resolved it to a slot.
template <bool INSERT, int PHASE = 0, class Args = ExpiringArgs, bool LOWP = false>
__global__ __launch_bounds__(kBlock) void hash_insert_expiring_kernel(const Args args) {
  static_assert(PHASE == 0 || INSERT == (PHASE == 2), "phase 1 finds, phase 2 inserts");
  static_assert(INSERT || !LOWP, "only an inserting launch writes rows: a find of a 16-bit table is the fp32 find");
  constexpr bool kMetadata = INSERT || PHASE == 1;
  constexpr bool kSeq = IsSeq<Args>::value;
  const ExpiringArgs& x = expiring_args(args);
  const HashArgs& a = x.h;
  const int b = (int)blockIdx.x;
  const int ri = find_run(args, b);
  const int ci = work_column(args, a, ri, b);
  const HashCol& c = a.col[ci];
  const ExpiryCol& e = x.e[ci];
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int group_log2 = lane_group_log2<LOWP>(c);
  const int gsize = 1 << group_log2;
  const int sub = lane & (gsize - 1);
  const int grp = lane >> group_log2;
  const int gbase = grp << group_log2;
  const int groups_per_wave = kWave >> group_log2;
  const int64_t wave_in_col = (int64_t)work_tile(args, a, ri, ci, b) * kWavesPerBlock + wave;
  const int64_t first_key = wave_in_col * groups_per_wave * kKeys;
  const int64_t n_keys = work_n_keys(args, c, ri);
  if (first_key >= n_keys) return;   // (wave-uniform)
  const int64_t i0 = first_key + grp;   // + u * groups_per_wave
  const unsigned long long group_mask = (gsize == 64 ? ~0ull : ((1ull << gsize) - 1ull)) << gbase;
  const int32_t slab_size = c.slab_size;
  const int64_t slab_count = (int64_t)c.slab_div.d;
  const int64_t capacity = slab_count * slab_size;
  const bool in_slab = sub < slab_size;
  long long* const cache = c.cache;
  long long key[kKeys], read_key[kKeys];
  int64_t home[kKeys];
  [[maybe_unused]] bool pending[kKeys], admitted[kKeys];   // (PHASE 2)
  [[maybe_unused]] bool there[kKeys];                      // (sequences) the position holds an id: a key or the pad id
  if constexpr (PHASE == 2) {
    // one coalesced read of the answers of phase 1: a wave with nothing pending leaves here
    bool any = false;
#pragma unroll
    for (int u = 0; u < kKeys; ++u) {
      const int64_t i = i0 + (int64_t)u * groups_per_wave;
      pending[u] = i < n_keys && work_slots(args, c, ri)[i] == kPending;
      any |= pending[u];
    }
    if (!__any(any)) return;
  }
  const int32_t step = kMetadata ? *e.step : 0;
#pragma unroll
  for (int u = 0; u < kKeys; ++u) {
    const int64_t i = i0 + (int64_t)u * groups_per_wave;
    if constexpr (kSeq) {
      // (phase 2 reads what phase 1 read; the lengths were written by phase 1)
      const bool wanted = PHASE == 2 ? pending[u] : i < n_keys;
      there[u] = false;
      key[u] = kEmptyKey;
      if (wanted) key[u] = seq_key(args.s[ci], c.keys, i, PHASE != 2 && sub == 0, &there[u]);
    } else if constexpr (PHASE == 2) {
      key[u] = pending[u] ? (long long)work_keys(args, c, ri)[i] : kEmptyKey;
    } else {
      key[u] = i < n_keys ? (long long)work_keys(args, c, ri)[i] : kEmptyKey;
    }
    if (key[u] == kTombstoneKey) key[u] = kEmptyKey;   // neither sentinel is ever stored: -1, counted as failed
  }
  if constexpr (PHASE == 2) {
#pragma unroll
    for (int u = 0; u < kKeys; ++u) {
      admitted[u] = sketch_estimate(args.f[ci], key[u], pending[u], sub, gsize) >= args.f[ci].min_freq && pending[u];
      if (!admitted[u]) key[u] = kEmptyKey;   // not walked: -1, counted in `filtered`
    }
  }
#pragma unroll
  for (int u = 0; u < kKeys; ++u) {
    home[u] = (int64_t)fastmod((uint64_t)murmur3_i64(key[u]), c.slab_div);
    read_key[u] = 0;
    if (key[u] != kEmptyKey && in_slab) read_key[u] = read_slot<INSERT>(cache + home[u] * slab_size + sub);
  }
  int32_t n_inserted = 0, n_failed = 0, n_reused = 0, n_filtered = 0;
  int64_t seen_slot[kKeys];   // the slot of every occurrence this lane answers for, or -1
#pragma unroll
  for (int u = 0; u < kKeys; ++u) {
    const int64_t i = i0 + (int64_t)u * groups_per_wave;
    bool active = key[u] != kEmptyKey;
    bool won = false, reused = false;
    int64_t result = -1;
    int64_t slab = home[u];
    int64_t probed = 0;      // slabs of this walk read without an EMPTY slot: <= slab_count
    int64_t tomb = -1;       // the first TOMBSTONE slot of this walk
    int64_t restarts = 0;    // CASes lost to another key: <= capacity (each one a free slot somebody else filled)
    long long rk = read_key[u];
    for (;;) {
      const bool live = active && in_slab;
      const unsigned long long match = __ballot(live && rk == key[u]) & group_mask;
      const unsigned long long empty = __ballot(live && rk == kEmptyKey) & group_mask;
      const unsigned long long dead = __ballot(live && rk == kTombstoneKey) & group_mask;
      bool claim = false;
      int64_t target = -1;
      if (active) {
        if (match != 0ull) {
          result = slab * slab_size + (__builtin_ctzll(match) - gbase);
          active = false;
        } else {
          if (tomb < 0 && dead != 0ull) tomb = slab * slab_size + (__builtin_ctzll(dead) - gbase);
          if (empty != 0ull) {
            claim = true;   // the stopping slab: the key is nowhere behind it
            target = tomb >= 0 ? tomb : slab * slab_size + (__builtin_ctzll(empty) - gbase);
          } else {
            slab = slab + 1 == slab_count ? 0 : slab + 1;
            if (++probed >= slab_count) {
              claim = true;   // every slab read, none with an EMPTY slot
              target = tomb;
            }
          }
        }
      }
      if (INSERT) {
        // (every lane of the wave takes the shuffle; the CAS is the group's first lane alone)
        const bool cas = claim && target >= 0;
        const long long free_key = target == tomb ? kTombstoneKey : kEmptyKey;
        long long old = 0;
        if (cas && sub == 0) {
          long long expected = free_key;
          __hip_atomic_compare_exchange_strong(cache + target, &expected, key[u], __ATOMIC_RELAXED,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          old = expected;   // what the slot held: free_key when the exchange was made
        }
        old = __shfl(old, gbase, kWave);
        if (claim) {
          if (!cas) {
            active = false;   // no free slot on the whole walk: -1
          } else if (old == free_key || old == key[u]) {
            // stored, or a concurrent duplicate of the key won this slot: a hit on it
            won = old == free_key;
            reused = won && free_key == kTombstoneKey;
            result = target;
            active = false;
          } else {
            // lost to another key: the walk again from the home slab
            slab = home[u];
            probed = 0;
            tomb = -1;
            if (++restarts > capacity) active = false;   // (unreachable: the bound, written out)
          }
        }
      } else if (claim) {
        active = false;   // a find stops where an insert would claim: not stored
      }
      if (!__any(active)) break;
      rk = 0;
      if (active && in_slab) rk = read_slot<INSERT>(cache + slab * slab_size + sub);
    }
    if (INSERT && won && c.table != nullptr) init_row<LOWP>(c, key[u], result, sub, gsize);
    if constexpr (PHASE == 1) {
      // not found and not a sentinel (which stays -1, counted as failed): counted, decided in phase 2
      if (result < 0 && key[u] != kEmptyKey) {
        sketch_count(args.f[ci], key[u], sub, gsize);
        result = kPending;
      }
    }
    if constexpr (PHASE == 2) {
      if (pending[u] && sub == 0) {
        work_slots(args, c, ri)[i] = result;
        n_inserted += won ? 1 : 0;
        n_reused += reused ? 1 : 0;
        n_failed += admitted[u] && result < 0 ? 1 : 0;
        n_filtered += admitted[u] ? 0 : 1;
      }
      seen_slot[u] = pending[u] && sub == 0 ? result : -1;
    } else {
      if (i < n_keys && sub == 0) {
        work_slots(args, c, ri)[i] = result;
        n_inserted += won ? 1 : 0;
        n_reused += reused ? 1 : 0;
        if constexpr (kSeq) {
          n_failed += there[u] && (PHASE == 1 ? result == -1 : result < 0) ? 1 : 0;   // nothing here: not a failure
        } else {
          n_failed += (PHASE == 1 ? result == -1 : result < 0) ? 1 : 0;
        }
      }
      seen_slot[u] = i < n_keys && sub == 0 ? result : -1;   // (kPending is no slot either)
    }
  }
  if (kMetadata) {
    // the metadata of the wave's keys together, reads first: 8 independent loads, then 8 independent adds.
    // The read is a plain load (it only decides whether the counter is at its ceiling; a value as old as the
    // launch's start keeps the bound: below 2^30 then, plus fewer than 2^30 occurrences).
    int32_t seen_freq[kKeys];
#pragma unroll
    for (int u = 0; u < kKeys; ++u) {
      seen_freq[u] = kFreqCeiling;
      if (seen_slot[u] >= 0) {
        e.last_seen[seen_slot[u]] = step;
        seen_freq[u] = e.freq[seen_slot[u]];
      }
    }
#pragma unroll
    for (int u = 0; u < kKeys; ++u) {
      if (seen_freq[u] < kFreqCeiling) {
        __hip_atomic_fetch_add(e.freq + seen_slot[u], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  // one atomic per wave and counter: the lanes' counts summed across the wave
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    n_inserted += __shfl_xor(n_inserted, off, kWave);
    n_failed += __shfl_xor(n_failed, off, kWave);
    n_reused += __shfl_xor(n_reused, off, kWave);
  }
  if (c.counts != nullptr) {
    if (lane == 0 && n_inserted != 0) atomicAdd(c.counts, n_inserted);
    if (lane == 0 && n_failed != 0) atomicAdd(c.counts + 1, n_failed);
  }
  if (e.stats != nullptr && lane == 0 && n_reused != 0) atomicAdd(e.stats + 1, n_reused);
  if constexpr (PHASE == 2) {
    if (args.f[ci].filtered != nullptr) {
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) n_filtered += __shfl_xor(n_filtered, off, kWave);
      if (lane == 0 && n_filtered != 0) atomicAdd(args.f[ci].filtered, n_filtered);
    }
  }
}

}  // namespace
}  // namespace hbk

namespace hbk {
namespace {

// the host checks both entries make of one column: HBK_OK or HBK_INVALID_ARGUMENT
int check_column(const char* who, int32_t c, const hbk_hash_column_t& h) {
  if (int rc = check_slabs(who, c, "", h.slab_count, h.slab_size)) return rc;
  HBK_REQUIRE(h.n_keys >= 0 && h.n_keys < (1ll << 31), "%s: column %d: n_keys must be in [0, 2^31), got %lld",
              who, c, (long long)h.n_keys);
  HBK_REQUIRE(h.n_keys == 0 || (h.keys_cache != nullptr && h.keys != nullptr && h.slots != nullptr),
              "%s: column %d: NULL buffer (keys_cache, keys and slots are needed with n_keys > 0)", who, c);
  HBK_REQUIRE(((uintptr_t)h.keys_cache & 7) == 0, "%s: column %d: keys_cache must be 8-byte aligned", who, c);
  if (h.table != nullptr) {
    HBK_REQUIRE(h.dim >= 1, "%s: column %d: dim must be >= 1 with a table, got %d", who, c, h.dim);
    HBK_REQUIRE(h.table_pitch == 0 || h.table_pitch >= h.dim,
                "%s: column %d: table_pitch %d is smaller than dim %d", who, c, h.table_pitch, h.dim);
  }
  HBK_REQUIRE(h.init_scale >= 0.0f && h.init_scale <= 3.402823466e38f,
              "%s: column %d: init_scale must be finite and >= 0, got %g", who, c, (double)h.init_scale);
  return HBK_OK;
}

// what the 16-bit entries add to check_column for one column: its element code and the layout of whole 4-byte words
int check_lowp_column(const char* who, int32_t c, const hbk_hash_column_t& h, int32_t code) {
  HBK_REQUIRE(code == HBK_LOWP_BF16 || code == HBK_LOWP_FP16,
              "%s: column %d: table_dtypes must be HBK_LOWP_BF16 (%d) or HBK_LOWP_FP16 (%d), got %d", who, c,
              HBK_LOWP_BF16, HBK_LOWP_FP16, code);
  if (h.table != nullptr) {
    HBK_REQUIRE((h.dim & 1) == 0, "%s: column %d: dim must be even on a 16-bit table (rows are written as 4-byte "
                "words), got %d", who, c, h.dim);
    HBK_REQUIRE((h.table_pitch & 1) == 0, "%s: column %d: table_pitch must be even on a 16-bit table, got %d", who, c,
                h.table_pitch);
    HBK_REQUIRE(((uintptr_t)h.table & 3) == 0, "%s: column %d: table must be 4-byte aligned", who, c);
  }
  HBK_REQUIRE(code != HBK_LOWP_FP16 || h.init_scale <= 65504.0f,
              "%s: column %d: init_scale %g is above 65504, the largest fp16: a start value would round to infinity",
              who, c, (double)h.init_scale);
  return HBK_OK;
}

// the kernel's view of one column; returns its tiles.  elem: 0, or the element code of a 16-bit table for a LOWP
// kernel (which alone looks at it)
int64_t describe_column(const hbk_hash_column_t& h, int32_t insert, HashCol* out, int32_t elem = 0) {
  HashCol& d = *out;
  d.cache = reinterpret_cast<long long*>(h.keys_cache);
  d.keys = h.keys;
  d.slots = h.slots;
  d.counts = h.counts;
  d.table = insert != 0 ? h.table : nullptr;
  d.n_keys = h.n_keys;
  d.slab_div = make_fastdiv((uint64_t)h.slab_count);
  d.slab_div.d = (uint64_t)h.slab_count;
  d.pitch = h.table_pitch > 0 ? h.table_pitch : h.dim;
  d.seed = (uint64_t)h.seed;
  d.init_scale = h.init_scale;
  d.slab_size = h.slab_size;
  d.dim = h.dim;
  const int32_t group_log2 = pow2_log2(h.slab_size);
  d.group_log2 = group_log2 | (elem << kElemShift);
  const int64_t keys_per_block = (int64_t)(kBlock >> group_log2) * kKeys;
  return (h.n_keys + keys_per_block - 1) / keys_per_block;
}

// the checks both admitting entries make of one column's filter
int check_admission(const char* who, int32_t c, const hbk_hash_column_t& h, const hbk_hash_admission_t& f) {
  HBK_REQUIRE(h.n_keys < (1ll << 30), "%s: column %d: n_keys must be below 2^30 (a counter must not wrap), got %lld",
              who, c, (long long)h.n_keys);
  HBK_REQUIRE(f.width >= 1 && f.width < (1ll << 31), "%s: column %d: sketch width must be in [1, 2^31), got %lld",
              who, c, (long long)f.width);
  HBK_REQUIRE(f.depth >= 1 && f.depth <= HBK_HASH_MAX_SKETCH_DEPTH,
              "%s: column %d: sketch depth must be in [1, %d], got %d", who, c, HBK_HASH_MAX_SKETCH_DEPTH, f.depth);
  HBK_REQUIRE(f.min_freq >= 1 && f.min_freq <= kFreqCeiling,
              "%s: column %d: min_freq must be in [1, 2^30], got %d", who, c, f.min_freq);
  HBK_REQUIRE(h.n_keys == 0 || f.sketch != nullptr,
              "%s: column %d: NULL sketch (needed with n_keys > 0)", who, c);
  HBK_REQUIRE(((uintptr_t)f.sketch & 3) == 0, "%s: column %d: sketch must be 4-byte aligned", who, c);
  return HBK_OK;
}

void describe_admission(const hbk_hash_admission_t& f, AdmitCol* out) {
  AdmitCol& d = *out;
  d.sketch = f.sketch;
  d.filtered = f.filtered;
  d.width_div = make_fastdiv((uint64_t)f.width);
  d.width_div.d = (uint64_t)f.width;
  d.seed = (uint64_t)f.seed;
  d.depth = f.depth;
  d.min_freq = f.min_freq;
}

void describe_expiry(const hbk_hash_expiry_t& x, ExpiryCol* out) {
  out->last_seen = x.last_seen;
  out->freq = x.freq;
  out->step = x.step;
  out->stats = x.stats;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_hash_insert_n(int32_t n_cols, const hbk_hash_column_t* cols, int32_t insert,
                                 hbk_stream_t stream) {
  using namespace hbk;
  const char* who = "hash_insert_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    if (int rc = check_column(who, c, cols[c])) return rc;
  }
  int32_t c0 = 0;
  while (c0 < n_cols) {
    HashArgs args;
    int32_t k = 0;
    int64_t tiles = 0;
    args.tile_start[0] = 0;
    while (c0 < n_cols && k < kMaxColsPerLaunch) {
      const hbk_hash_column_t& h = cols[c0++];
      if (h.n_keys == 0) continue;
      tiles += describe_column(h, insert, &args.col[k]);
      HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
      ++k;
      args.tile_start[k] = (int32_t)tiles;
    }
    if (k == 0) continue;
    args.n_cols = k;
    if (insert != 0) {
      hipLaunchKernelGGL(hash_insert_kernel<true>, dim3((unsigned)tiles), dim3(kBlock), 0, as_stream(stream),
                         args);
    } else {
      hipLaunchKernelGGL(hash_insert_kernel<false>, dim3((unsigned)tiles), dim3(kBlock), 0, as_stream(stream),
                         args);
    }
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

extern "C" int hbk_hash_insert_expiring_n(int32_t n_cols, const hbk_hash_column_t* cols,
                                          const hbk_hash_expiry_t* exp, int32_t insert, hbk_stream_t stream) {
  using namespace hbk;
  const char* who = "hash_insert_expiring_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(n_cols == 0 || exp != nullptr, "%s: exp is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    if (int rc = check_column(who, c, cols[c])) return rc;
    HBK_REQUIRE(cols[c].n_keys < (1ll << 30), "%s: column %d: n_keys must be below 2^30 (freq must not wrap), got %lld",
                who, c, (long long)cols[c].n_keys);
    HBK_REQUIRE(cols[c].n_keys == 0 ||
                    (exp[c].last_seen != nullptr && exp[c].freq != nullptr && exp[c].step != nullptr),
                "%s: column %d: NULL expiry buffer (last_seen, freq and step are needed with n_keys > 0)", who, c);
  }
  int32_t c0 = 0;
  while (c0 < n_cols) {
    ExpiringArgs args;
    int32_t k = 0;
    int64_t tiles = 0;
    args.h.tile_start[0] = 0;
    while (c0 < n_cols && k < kMaxColsPerLaunch) {
      const hbk_hash_column_t& h = cols[c0];
      const hbk_hash_expiry_t& x = exp[c0++];
      if (h.n_keys == 0) continue;
      tiles += describe_column(h, insert, &args.h.col[k]);
      HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
      describe_expiry(x, &args.e[k]);
      ++k;
      args.h.tile_start[k] = (int32_t)tiles;
    }
    if (k == 0) continue;
    args.h.n_cols = k;
    if (insert != 0) {
      hipLaunchKernelGGL(hash_insert_expiring_kernel<true>, dim3((unsigned)tiles), dim3(kBlock), 0,
                         as_stream(stream), args);
    } else {
      hipLaunchKernelGGL(hash_insert_expiring_kernel<false>, dim3((unsigned)tiles), dim3(kBlock), 0,
                         as_stream(stream), args);
    }
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

// Count, then admit: every counting launch of the call before any admitting one, on one stream.
extern "C" int hbk_hash_insert_admit_n(int32_t n_cols, const hbk_hash_column_t* cols,
                                       const hbk_hash_admission_t* adm, int32_t insert, hbk_stream_t stream) {
  using namespace hbk;
  const char* who = "hash_insert_admit_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(n_cols == 0 || adm != nullptr, "%s: adm is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    if (int rc = check_column(who, c, cols[c])) return rc;
    if (int rc = check_admission(who, c, cols[c], adm[c])) return rc;
  }
  if (insert == 0) return hbk_hash_insert_n(n_cols, cols, 0, stream);   // a find: the sketch is not touched
  for (int phase = 1; phase <= 2; ++phase) {
    int32_t c0 = 0;
    while (c0 < n_cols) {
      AdmitArgs args;
      int32_t k = 0;
      int64_t tiles = 0;
      args.h.tile_start[0] = 0;
      while (c0 < n_cols && k < kMaxColsPerLaunch) {
        const hbk_hash_column_t& h = cols[c0];
        const hbk_hash_admission_t& f = adm[c0++];
        if (h.n_keys == 0) continue;
        tiles += describe_column(h, insert, &args.h.col[k]);
        HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
        describe_admission(f, &args.f[k]);
        ++k;
        args.h.tile_start[k] = (int32_t)tiles;
      }
      if (k == 0) continue;
      args.h.n_cols = k;
      if (phase == 1) {
        hipLaunchKernelGGL((hash_insert_kernel<false, 1, AdmitArgs>), dim3((unsigned)tiles), dim3(kBlock), 0,
                           as_stream(stream), args);
      } else {
        hipLaunchKernelGGL((hash_insert_kernel<true, 2, AdmitArgs>), dim3((unsigned)tiles), dim3(kBlock), 0,
                           as_stream(stream), args);
      }
      HBK_HIP_OK(hipGetLastError());
    }
  }
  return HBK_OK;
}

extern "C" int hbk_hash_insert_expiring_admit_n(int32_t n_cols, const hbk_hash_column_t* cols,
                                                const hbk_hash_expiry_t* exp, const hbk_hash_admission_t* adm,
                                                int32_t insert, hbk_stream_t stream) {
  using namespace hbk;
  const char* who = "hash_insert_expiring_admit_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(n_cols == 0 || exp != nullptr, "%s: exp is NULL", who);
  HBK_REQUIRE(n_cols == 0 || adm != nullptr, "%s: adm is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    if (int rc = check_column(who, c, cols[c])) return rc;
    if (int rc = check_admission(who, c, cols[c], adm[c])) return rc;
    HBK_REQUIRE(cols[c].n_keys == 0 ||
                    (exp[c].last_seen != nullptr && exp[c].freq != nullptr && exp[c].step != nullptr),
                "%s: column %d: NULL expiry buffer (last_seen, freq and step are needed with n_keys > 0)", who, c);
  }
  if (insert == 0) return hbk_hash_insert_expiring_n(n_cols, cols, exp, 0, stream);   // a find
  for (int phase = 1; phase <= 2; ++phase) {
    int32_t c0 = 0;
    while (c0 < n_cols) {
      ExpiringAdmitArgs args;
      int32_t k = 0;
      int64_t tiles = 0;
      args.x.h.tile_start[0] = 0;
      while (c0 < n_cols && k < kMaxColsPerLaunch) {
        const hbk_hash_column_t& h = cols[c0];
        const hbk_hash_expiry_t& x = exp[c0];
        const hbk_hash_admission_t& f = adm[c0++];
        if (h.n_keys == 0) continue;
        tiles += describe_column(h, insert, &args.x.h.col[k]);
        HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
        describe_expiry(x, &args.x.e[k]);
        describe_admission(f, &args.f[k]);
        ++k;
        args.x.h.tile_start[k] = (int32_t)tiles;
      }
      if (k == 0) continue;
      args.x.h.n_cols = k;
      if (phase == 1) {
        hipLaunchKernelGGL((hash_insert_expiring_kernel<false, 1, ExpiringAdmitArgs>), dim3((unsigned)tiles),
                           dim3(kBlock), 0, as_stream(stream), args);
      } else {
        hipLaunchKernelGGL((hash_insert_expiring_kernel<true, 2, ExpiringAdmitArgs>), dim3((unsigned)tiles),
                           dim3(kBlock), 0, as_stream(stream), args);
      }
      HBK_HIP_OK(hipGetLastError());
    }
  }
  return HBK_OK;
}

// ---- keys that arrive as runs ---------------------------------------------------------------------------
namespace hbk {
namespace {

static_assert(sizeof(RunsArgs<HashArgs>) <= 24576, "kernarg budget");
static_assert(sizeof(RunsArgs<ExpiringAdmitArgs>) <= 24576, "kernarg budget");

// the parts of the base arguments a column is described into (nullptr: the table kind has none)
inline HashArgs& hash_part(HashArgs& a) { return a; }
inline HashArgs& hash_part(AdmitArgs& a) { return a.h; }
inline HashArgs& hash_part(ExpiringArgs& a) { return a.h; }
inline HashArgs& hash_part(ExpiringAdmitArgs& a) { return a.x.h; }
inline ExpiryCol* expiry_part(HashArgs&) { return nullptr; }
inline ExpiryCol* expiry_part(AdmitArgs&) { return nullptr; }
inline ExpiryCol* expiry_part(ExpiringArgs& a) { return a.e; }
inline ExpiryCol* expiry_part(ExpiringAdmitArgs& a) { return a.x.e; }
inline AdmitCol* admit_part(HashArgs&) { return nullptr; }
inline AdmitCol* admit_part(AdmitArgs& a) { return a.f; }
inline AdmitCol* admit_part(ExpiringArgs&) { return nullptr; }
inline AdmitCol* admit_part(ExpiringAdmitArgs& a) { return a.f; }

// One pass over all runs of all columns with `kernel`: a launch takes up to kMaxRunsPerLaunch non-empty runs of
// up to kMaxColsPerLaunch columns (a column whose runs straddle two launches is described in both).  dtypes: the
// element codes for a LOWP kernel, or NULL for every other kernel (launch_columns below).
template <class Base>
int launch_runs(const char* who, int32_t n_cols, const hbk_hash_column_t* cols, const hbk_hash_expiry_t* exp,
                const hbk_hash_admission_t* adm, const int32_t* dtypes, const int32_t* n_runs,
                const hbk_hash_run_t* const* runs, int32_t insert, void (*kernel)(const RunsArgs<Base>),
                hipStream_t stream) {
  int32_t c = 0, r = 0;   // the next run to place
  while (c < n_cols) {
    RunsArgs<Base> args;
    HashArgs& h = hash_part(static_cast<Base&>(args));
    int32_t k = 0, nr = 0, described = -1;
    int64_t tiles = 0, keys_per_block = 0;   // keys_per_block: of the column described last
    h.tile_start[0] = 0;
    args.run_tile_start[0] = 0;
    while (c < n_cols && nr < kMaxRunsPerLaunch) {
      if (r >= n_runs[c]) {
        ++c;
        r = 0;
        continue;
      }
      const hbk_hash_run_t& run = runs[c][r];
      if (run.n_keys == 0) {
        ++r;
        continue;
      }
      if (described != c) {
        if (k == kMaxColsPerLaunch) break;
        hbk_hash_column_t col = cols[c];   // (its keys / slots / n_keys are the runs')
        col.keys = nullptr;
        col.slots = nullptr;
        col.n_keys = 0;
        (void)describe_column(col, insert, &h.col[k], dtypes != nullptr ? dtypes[c] : 0);
        if (ExpiryCol* e = expiry_part(static_cast<Base&>(args))) describe_expiry(exp[c], e + k);
        if (AdmitCol* f = admit_part(static_cast<Base&>(args))) describe_admission(adm[c], f + k);
        keys_per_block = (int64_t)(kBlock >> pow2_log2(col.slab_size)) * kKeys;   // (describe_column's tiling)
        described = c;
        ++k;
      }
      tiles += (run.n_keys + keys_per_block - 1) / keys_per_block;
      HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
      args.run[nr].keys = run.keys;
      args.run[nr].slots = run.slots;
      args.run[nr].n_keys = run.n_keys;
      args.run[nr].col = k - 1;
      args.run[nr].pad_ = 0;
      ++nr;
      args.run_tile_start[nr] = (int32_t)tiles;
      ++r;
    }
    if (nr == 0) continue;   // (only when every column is through)
    h.n_cols = k;
    args.n_runs = nr;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(kBlock), 0, stream, args);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

// The four translate entries over keys that arrive as runs: one launch (two for filtered tables: every counting
// launch of the call before any admitting one) while the non-empty runs stay within
// HBK_HASH_MAX_RUNS_PER_LAUNCH and the columns within 64.
//
// translate_runs is both entries: `lowp` is the 16-bit one (hbk_hash_translate_runs_lowp_n), whose checks come after
// the fp32 entry's for every column and whose INSERTING launches are the LOWP instantiations with the element codes;
// a find and the counting phase of a filtered table write no row and are the fp32 launches as they are.
namespace hbk {
namespace {

int translate_runs(const char* who, bool lowp, int32_t n_cols, const hbk_hash_column_t* cols,
                   const hbk_hash_expiry_t* exp, const hbk_hash_admission_t* adm, const int32_t* table_dtypes,
                   const int32_t* n_runs, const hbk_hash_run_t* const* runs, int32_t insert, hbk_stream_t stream_) {
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  if (lowp && n_cols == 0) return HBK_OK;
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(!lowp || table_dtypes != nullptr, "%s: table_dtypes is NULL", who);
  HBK_REQUIRE(n_cols == 0 || (n_runs != nullptr && runs != nullptr), "%s: n_runs or runs is NULL", who);
  const int64_t key_limit = exp != nullptr || adm != nullptr ? (1ll << 30) : (1ll << 31);
  for (int32_t c = 0; c < n_cols; ++c) {
    HBK_REQUIRE(n_runs[c] >= 0, "%s: column %d: n_runs must be >= 0, got %d", who, c, n_runs[c]);
    HBK_REQUIRE(n_runs[c] == 0 || runs[c] != nullptr, "%s: column %d: runs is NULL with n_runs = %d", who, c,
                n_runs[c]);
    int64_t total = 0;
    const hbk_hash_run_t* first = nullptr;
    for (int32_t r = 0; r < n_runs[c]; ++r) {
      const hbk_hash_run_t& run = runs[c][r];
      HBK_REQUIRE(run.n_keys >= 0 && run.n_keys < (1ll << 31),
                  "%s: column %d: run %d: n_keys must be in [0, 2^31), got %lld", who, c, r, (long long)run.n_keys);
      HBK_REQUIRE(run.n_keys == 0 || (run.keys != nullptr && run.slots != nullptr),
                  "%s: column %d: run %d: NULL buffer (keys and slots are needed with n_keys > 0)", who, c, r);
      if (run.n_keys > 0 && first == nullptr) first = &run;
      total += run.n_keys;
      HBK_REQUIRE(total < key_limit, "%s: column %d: the runs sum to %lld keys or more: must stay below 2^%d%s", who,
                  c, (long long)total, key_limit == (1ll << 30) ? 30 : 31,
                  key_limit == (1ll << 30) ? " (a counter must not wrap)" : "");
    }
    // the column as the matching entry would see it: the concatenation of its runs
    hbk_hash_column_t whole = cols[c];
    whole.n_keys = total;
    whole.keys = first != nullptr ? first->keys : nullptr;
    whole.slots = first != nullptr ? first->slots : nullptr;
    if (int rc = check_column(who, c, whole)) return rc;
    if (adm != nullptr) {
      if (int rc = check_admission(who, c, whole, adm[c])) return rc;
    }
    HBK_REQUIRE(exp == nullptr || total == 0 ||
                    (exp[c].last_seen != nullptr && exp[c].freq != nullptr && exp[c].step != nullptr),
                "%s: column %d: NULL expiry buffer (last_seen, freq and step are needed with keys)", who, c);
    if (lowp) {
      if (int rc = check_lowp_column(who, c, whole, table_dtypes[c])) return rc;
    }
  }
  hipStream_t stream = as_stream(stream_);
  const int32_t* const no_dtypes = nullptr;
  if (adm != nullptr && insert != 0) {   // count, then admit
    if (exp != nullptr) {
      if (int rc = launch_runs<ExpiringAdmitArgs>(
              who, n_cols, cols, exp, adm, no_dtypes, n_runs, runs, insert,
              hash_insert_expiring_kernel<false, 1, RunsArgs<ExpiringAdmitArgs>>, stream)) {
        return rc;
      }
      return launch_runs<ExpiringAdmitArgs>(
          who, n_cols, cols, exp, adm, table_dtypes, n_runs, runs, insert,
          lowp ? hash_insert_expiring_kernel<true, 2, RunsArgs<ExpiringAdmitArgs>, true>
               : hash_insert_expiring_kernel<true, 2, RunsArgs<ExpiringAdmitArgs>>,
          stream);
    }
    if (int rc = launch_runs<AdmitArgs>(who, n_cols, cols, exp, adm, no_dtypes, n_runs, runs, insert,
                                        hash_insert_kernel<false, 1, RunsArgs<AdmitArgs>>, stream)) {
      return rc;
    }
    return launch_runs<AdmitArgs>(who, n_cols, cols, exp, adm, table_dtypes, n_runs, runs, insert,
                                  lowp ? hash_insert_kernel<true, 2, RunsArgs<AdmitArgs>, true>
                                       : hash_insert_kernel<true, 2, RunsArgs<AdmitArgs>>,
                                  stream);
  }
  // no filter, or a find (which never touches the sketch)
  if (insert == 0) {
    if (exp != nullptr) {
      return launch_runs<ExpiringArgs>(who, n_cols, cols, exp, nullptr, no_dtypes, n_runs, runs, insert,
                                       hash_insert_expiring_kernel<false, 0, RunsArgs<ExpiringArgs>>, stream);
    }
    return launch_runs<HashArgs>(who, n_cols, cols, nullptr, nullptr, no_dtypes, n_runs, runs, insert,
                                 hash_insert_kernel<false, 0, RunsArgs<HashArgs>>, stream);
  }
  if (exp != nullptr) {
    return launch_runs<ExpiringArgs>(who, n_cols, cols, exp, nullptr, table_dtypes, n_runs, runs, insert,
                                     lowp ? hash_insert_expiring_kernel<true, 0, RunsArgs<ExpiringArgs>, true>
                                          : hash_insert_expiring_kernel<true, 0, RunsArgs<ExpiringArgs>>,
                                     stream);
  }
  return launch_runs<HashArgs>(who, n_cols, cols, nullptr, nullptr, table_dtypes, n_runs, runs, insert,
                               lowp ? hash_insert_kernel<true, 0, RunsArgs<HashArgs>, true>
                                    : hash_insert_kernel<true, 0, RunsArgs<HashArgs>>,
                               stream);
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_hash_translate_runs_n(int32_t n_cols, const hbk_hash_column_t* cols,
                                         const hbk_hash_expiry_t* exp, const hbk_hash_admission_t* adm,
                                         const int32_t* n_runs, const hbk_hash_run_t* const* runs,
                                         int32_t insert, hbk_stream_t stream) {
  return hbk::translate_runs("hash_translate_runs_n", false, n_cols, cols, exp, adm, nullptr, n_runs, runs, insert,
                             stream);
}

extern "C" int hbk_hash_translate_runs_lowp_n(int32_t n_cols, const hbk_hash_column_t* cols,
                                              const hbk_hash_expiry_t* exp, const hbk_hash_admission_t* adm,
                                              const int32_t* table_dtypes, const int32_t* n_runs,
                                              const hbk_hash_run_t* const* runs, int32_t insert,
                                              hbk_stream_t stream) {
  return hbk::translate_runs("hash_translate_runs_lowp_n", true, n_cols, cols, exp, adm, table_dtypes, n_runs, runs,
                             insert, stream);
}

// ---- 16-bit tables --------------------------------------------------------------------------------------
namespace hbk {
namespace {

// One pass over all columns with `kernel`, 64 columns with keys per launch: the loop of the four entries above, for
// any kind of arguments.  dtypes: the element codes for a LOWP kernel, or NULL for a kernel that writes no row (the
// counting phase of a filtered table).
template <class Base>
int launch_columns(const char* who, int32_t n_cols, const hbk_hash_column_t* cols, const hbk_hash_expiry_t* exp,
                   const hbk_hash_admission_t* adm, const int32_t* dtypes, int32_t insert,
                   void (*kernel)(const Base), hipStream_t stream) {
  int32_t c0 = 0;
  while (c0 < n_cols) {
    Base args;
    HashArgs& h = hash_part(args);
    int32_t k = 0;
    int64_t tiles = 0;
    h.tile_start[0] = 0;
    while (c0 < n_cols && k < kMaxColsPerLaunch) {
      const int32_t c = c0++;
      if (cols[c].n_keys == 0) continue;
      tiles += describe_column(cols[c], insert, &h.col[k], dtypes != nullptr ? dtypes[c] : 0);
      HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
      if (ExpiryCol* e = expiry_part(args)) describe_expiry(exp[c], e + k);
      if (AdmitCol* f = admit_part(args)) describe_admission(adm[c], f + k);
      ++k;
      h.tile_start[k] = (int32_t)tiles;
    }
    if (k == 0) continue;
    h.n_cols = k;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(kBlock), 0, stream, args);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_hash_insert_lowp_n(int32_t n_cols, const hbk_hash_column_t* cols, const hbk_hash_expiry_t* exp,
                                      const hbk_hash_admission_t* adm, const int32_t* table_dtypes, int32_t insert,
                                      hbk_stream_t stream_) {
  using namespace hbk;
  const char* who = "hash_insert_lowp_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  if (n_cols == 0) return HBK_OK;
  HBK_REQUIRE(cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(table_dtypes != nullptr, "%s: table_dtypes is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_column_t& h = cols[c];
    if (int rc = check_column(who, c, h)) return rc;
    if (exp != nullptr) {
      HBK_REQUIRE(h.n_keys < (1ll << 30), "%s: column %d: n_keys must be below 2^30 (freq must not wrap), got %lld",
                  who, c, (long long)h.n_keys);
      HBK_REQUIRE(h.n_keys == 0 || (exp[c].last_seen != nullptr && exp[c].freq != nullptr && exp[c].step != nullptr),
                  "%s: column %d: NULL expiry buffer (last_seen, freq and step are needed with n_keys > 0)", who, c);
    }
    if (adm != nullptr) {
      if (int rc = check_admission(who, c, h, adm[c])) return rc;
    }
    if (int rc = check_lowp_column(who, c, h, table_dtypes[c])) return rc;
  }
  if (insert == 0) {
    // a find writes no row and touches no sketch: the find of the fp32 entry, as it is
    return exp != nullptr ? hbk_hash_insert_expiring_n(n_cols, cols, exp, 0, stream_)
                          : hbk_hash_insert_n(n_cols, cols, 0, stream_);
  }
  hipStream_t stream = as_stream(stream_);
  if (adm != nullptr) {   // count (no row is written: the fp32 kernel), then admit
    if (exp != nullptr) {
      if (int rc = launch_columns<ExpiringAdmitArgs>(
              who, n_cols, cols, exp, adm, nullptr, insert, hash_insert_expiring_kernel<false, 1, ExpiringAdmitArgs>,
              stream)) {
        return rc;
      }
      return launch_columns<ExpiringAdmitArgs>(who, n_cols, cols, exp, adm, table_dtypes, insert,
                                               hash_insert_expiring_kernel<true, 2, ExpiringAdmitArgs, true>, stream);
    }
    if (int rc = launch_columns<AdmitArgs>(who, n_cols, cols, nullptr, adm, nullptr, insert,
                                           hash_insert_kernel<false, 1, AdmitArgs>, stream)) {
      return rc;
    }
    return launch_columns<AdmitArgs>(who, n_cols, cols, nullptr, adm, table_dtypes, insert,
                                     hash_insert_kernel<true, 2, AdmitArgs, true>, stream);
  }
  if (exp != nullptr) {
    return launch_columns<ExpiringArgs>(who, n_cols, cols, exp, nullptr, table_dtypes, insert,
                                        hash_insert_expiring_kernel<true, 0, ExpiringArgs, true>, stream);
  }
  return launch_columns<HashArgs>(who, n_cols, cols, nullptr, nullptr, table_dtypes, insert,
                                  hash_insert_kernel<true, 0, HashArgs, true>, stream);
}

// ---- keys that arrive as ragged sequences ---------------------------------------------------------------
namespace hbk {
namespace {

static_assert(sizeof(SeqArgs<HashArgs>) <= 24576, "kernarg budget");
static_assert(sizeof(SeqArgs<ExpiringAdmitArgs>) <= 24576, "kernarg budget");   // (64 columns fit: no smaller chunk)

// One pass over the positions of all columns with `kernel`: up to kMaxColsPerLaunch columns with positions per
// launch.  dtypes as for launch_runs.
template <class Base>
int launch_sequences(const char* who, int32_t n_cols, const hbk_hash_column_t* cols, const hbk_hash_expiry_t* exp,
                     const hbk_hash_admission_t* adm, const int32_t* dtypes, const hbk_hash_sequence_t* seq,
                     int32_t insert, void (*kernel)(const SeqArgs<Base>), hipStream_t stream) {
  int32_t c0 = 0;
  while (c0 < n_cols) {
    SeqArgs<Base> args;
    HashArgs& h = hash_part(static_cast<Base&>(args));
    int32_t k = 0;
    int64_t tiles = 0;
    h.tile_start[0] = 0;
    while (c0 < n_cols && k < kMaxColsPerLaunch) {
      const int32_t c = c0++;
      const hbk_hash_sequence_t& q = seq[c];
      const int64_t positions = q.n_segments * (int64_t)q.max_len;
      if (positions == 0) continue;
      hbk_hash_column_t col = cols[c];   // (the kernel's n_keys: the positions; its keys: the flat ids)
      col.n_keys = positions;
      tiles += describe_column(col, insert, &h.col[k], dtypes != nullptr ? dtypes[c] : 0);
      HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", who);
      if (ExpiryCol* e = expiry_part(static_cast<Base&>(args))) describe_expiry(exp[c], e + k);
      if (AdmitCol* f = admit_part(static_cast<Base&>(args))) describe_admission(adm[c], f + k);
      SeqCol& s = args.s[k];
      s.row_splits = q.row_splits;
      s.lengths = q.lengths;
      s.pad_id = q.pad_id;
      s.n_ids = cols[c].n_keys;
      s.len_div = make_fastdiv((uint64_t)q.max_len);
      s.len_div.d = (uint64_t)q.max_len;
      s.has_pad = q.has_pad != 0 ? 1 : 0;
      s.pad_ = 0;
      ++k;
      h.tile_start[k] = (int32_t)tiles;
    }
    if (k == 0) continue;
    h.n_cols = k;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(kBlock), 0, stream, args);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

// The four translate entries over the first T ids of every sample, answers into a [B * T] slot grid: one launch
// (two for filtered tables: every counting launch of the call before any admitting one) per 64 columns.
//
// translate_sequence is both entries, as translate_runs above: `lowp` is hbk_hash_translate_sequence_lowp_n.
namespace hbk {
namespace {

int translate_sequence(const char* who, bool lowp, int32_t n_cols, const hbk_hash_column_t* cols,
                       const hbk_hash_expiry_t* exp, const hbk_hash_admission_t* adm, const int32_t* table_dtypes,
                       const hbk_hash_sequence_t* seq, int32_t insert, hbk_stream_t stream_) {
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  if (lowp && n_cols == 0) return HBK_OK;
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(!lowp || table_dtypes != nullptr, "%s: table_dtypes is NULL", who);
  HBK_REQUIRE(n_cols == 0 || seq != nullptr, "%s: seq is NULL", who);
  const int64_t limit = exp != nullptr || adm != nullptr ? (1ll << 30) : (1ll << 31);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_hash_column_t& h = cols[c];
    const hbk_hash_sequence_t& q = seq[c];
    HBK_REQUIRE(q.max_len >= 1, "%s: column %d: max_len must be >= 1, got %d", who, c, q.max_len);
    HBK_REQUIRE(q.n_segments >= 0, "%s: column %d: n_segments must be >= 0, got %lld", who, c,
                (long long)q.n_segments);
    HBK_REQUIRE(q.n_segments < limit && q.n_segments * (int64_t)q.max_len < limit,
                "%s: column %d: %lld samples x max_len %d positions: must stay below 2^%d%s", who, c,
                (long long)q.n_segments, q.max_len, limit == (1ll << 30) ? 30 : 31,
                limit == (1ll << 30) ? " (a counter must not wrap)" : "");
    const int64_t positions = q.n_segments * (int64_t)q.max_len;
    HBK_REQUIRE(positions == 0 || h.slots != nullptr, "%s: column %d: NULL slots (the grid is needed with B * T > 0)",
                who, c);
    HBK_REQUIRE(h.n_keys >= 0 && h.n_keys < (1ll << 31), "%s: column %d: n_keys must be in [0, 2^31), got %lld", who,
                c, (long long)h.n_keys);
    HBK_REQUIRE(h.n_keys == 0 || h.keys != nullptr, "%s: column %d: NULL keys with n_keys = %lld", who, c,
                (long long)h.n_keys);
    HBK_REQUIRE(q.row_splits != nullptr || h.n_keys == q.n_segments,
                "%s: column %d: row_splits is NULL (one id per sample) but n_keys %lld != n_segments %lld", who, c,
                (long long)h.n_keys, (long long)q.n_segments);
    if (q.has_pad != 0) {
      HBK_REQUIRE(q.pad_id != (int64_t)kEmptyKey, "%s: column %d: pad_id INT64_MIN (EMPTY) is never stored", who, c);
      HBK_REQUIRE(exp == nullptr || q.pad_id != (int64_t)kTombstoneKey,
                  "%s: column %d: pad_id INT64_MIN + 1 (TOMBSTONE) is never stored in an expiring table", who, c);
    }
    // the column as the matching entry would see it: one key per position (a column without ids has no keys to
    // show: the grid stands in, the check only asks for an address)
    hbk_hash_column_t whole = h;
    whole.n_keys = positions;
    if (whole.keys == nullptr) whole.keys = h.slots;
    if (int rc = check_column(who, c, whole)) return rc;
    if (adm != nullptr) {
      if (int rc = check_admission(who, c, whole, adm[c])) return rc;
    }
    HBK_REQUIRE(exp == nullptr || positions == 0 ||
                    (exp[c].last_seen != nullptr && exp[c].freq != nullptr && exp[c].step != nullptr),
                "%s: column %d: NULL expiry buffer (last_seen, freq and step are needed with B * T > 0)", who, c);
    if (lowp) {
      if (int rc = check_lowp_column(who, c, whole, table_dtypes[c])) return rc;
    }
  }
  hipStream_t stream = as_stream(stream_);
  const int32_t* const no_dtypes = nullptr;
  if (adm != nullptr && insert != 0) {   // count, then admit
    if (exp != nullptr) {
      if (int rc = launch_sequences<ExpiringAdmitArgs>(
              who, n_cols, cols, exp, adm, no_dtypes, seq, insert,
              hash_insert_expiring_kernel<false, 1, SeqArgs<ExpiringAdmitArgs>>, stream)) {
        return rc;
      }
      return launch_sequences<ExpiringAdmitArgs>(
          who, n_cols, cols, exp, adm, table_dtypes, seq, insert,
          lowp ? hash_insert_expiring_kernel<true, 2, SeqArgs<ExpiringAdmitArgs>, true>
               : hash_insert_expiring_kernel<true, 2, SeqArgs<ExpiringAdmitArgs>>,
          stream);
    }
    if (int rc = launch_sequences<AdmitArgs>(who, n_cols, cols, exp, adm, no_dtypes, seq, insert,
                                             hash_insert_kernel<false, 1, SeqArgs<AdmitArgs>>, stream)) {
      return rc;
    }
    return launch_sequences<AdmitArgs>(who, n_cols, cols, exp, adm, table_dtypes, seq, insert,
                                       lowp ? hash_insert_kernel<true, 2, SeqArgs<AdmitArgs>, true>
                                            : hash_insert_kernel<true, 2, SeqArgs<AdmitArgs>>,
                                       stream);
  }
  // no filter, or a find (which never touches the sketch)
  if (insert == 0) {
    if (exp != nullptr) {
      return launch_sequences<ExpiringArgs>(who, n_cols, cols, exp, nullptr, no_dtypes, seq, insert,
                                            hash_insert_expiring_kernel<false, 0, SeqArgs<ExpiringArgs>>, stream);
    }
    return launch_sequences<HashArgs>(who, n_cols, cols, nullptr, nullptr, no_dtypes, seq, insert,
                                      hash_insert_kernel<false, 0, SeqArgs<HashArgs>>, stream);
  }
  if (exp != nullptr) {
    return launch_sequences<ExpiringArgs>(who, n_cols, cols, exp, nullptr, table_dtypes, seq, insert,
                                          lowp ? hash_insert_expiring_kernel<true, 0, SeqArgs<ExpiringArgs>, true>
                                               : hash_insert_expiring_kernel<true, 0, SeqArgs<ExpiringArgs>>,
                                          stream);
  }
  return launch_sequences<HashArgs>(who, n_cols, cols, nullptr, nullptr, table_dtypes, seq, insert,
                                    lowp ? hash_insert_kernel<true, 0, SeqArgs<HashArgs>, true>
                                         : hash_insert_kernel<true, 0, SeqArgs<HashArgs>>,
                                    stream);
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_hash_translate_sequence_n(int32_t n_cols, const hbk_hash_column_t* cols,
                                             const hbk_hash_expiry_t* exp, const hbk_hash_admission_t* adm,
                                             const hbk_hash_sequence_t* seq, int32_t insert,
                                             hbk_stream_t stream) {
  return hbk::translate_sequence("hash_translate_sequence_n", false, n_cols, cols, exp, adm, nullptr, seq, insert,
                                 stream);
}

extern "C" int hbk_hash_translate_sequence_lowp_n(int32_t n_cols, const hbk_hash_column_t* cols,
                                                  const hbk_hash_expiry_t* exp, const hbk_hash_admission_t* adm,
                                                  const int32_t* table_dtypes, const hbk_hash_sequence_t* seq,
                                                  int32_t insert, hbk_stream_t stream) {
  return hbk::translate_sequence("hash_translate_sequence_lowp_n", true, n_cols, cols, exp, adm, table_dtypes, seq,
                                 insert, stream);
}
