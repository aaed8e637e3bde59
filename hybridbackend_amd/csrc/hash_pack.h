// The deterministic stream compaction of hash_export.hip, once, for every selection: hbk_hash_export_n ("holds a
// key, seen since") and hbk_hash_spill_n ("an eviction's selection", hash_spill.hip) run the same three launches --
//   1. count   a 256-slot tile (one 64-slot chunk per wave) counts its matches into the workspace;
//   2. scan    one workgroup per column turns the tile counts into exclusive offsets in place and writes the
//              total to `count`;
//   3. write   every tile evaluates the SAME predicate again and places lane's key at  tile offset + matches of
//              the earlier waves of the tile + rank_below(ballot), the rows copied by lane groups.
// The kernels are templates over the launch's argument struct:
//   Args  { int32_t n_cols; int32_t tile_start[kMaxColsPerLaunch + 1]; Col col[kMaxColsPerLaunch]; }
//   Col   keys, out_keys, out_slots (or NULL), count, tiles, capacity, out_capacity, n_tiles, n_moves, move[],
//         bool selected(int64_t slot) const   the selection: false for slot >= capacity; a function of arrays
//                                             nobody writes during the three launches
//         void scanned() const                what thread 0 of the column's scan workgroup does besides
// Plain loads and plain vector stores only; no atomics anywhere in this file.  Internal to libhbk_core.so.
#ifndef HBK_CSRC_HASH_PACK_H_
#define HBK_CSRC_HASH_PACK_H_

#include "hash_common.h"

namespace hbk {
namespace pack {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kSlotsPerTile = kBlock;                   // one 64-slot chunk per wave
constexpr int kScanPerThread = 8;                       // tile counts a thread of the scan takes per pass
constexpr int kMaxColsPerLaunch = 32;                   // the argument structs travel by value

inline int64_t tiles_of(int64_t n) { return (n + kSlotsPerTile - 1) / kSlotsPerTile; }

template <class Args>
__global__ __launch_bounds__(kBlock) void hash_pack_count_kernel(const Args a) {
  __shared__ int32_t wave_n[kWavesPerBlock];
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const auto& c = a.col[ci];
  const int64_t tile = (int64_t)(b - a.tile_start[ci]);
  const int64_t slot = tile * kSlotsPerTile + (int64_t)wave * kWave + lane;
  const unsigned long long mask = __ballot(c.selected(slot));
  if (lane == 0) wave_n[wave] = (int32_t)__builtin_popcountll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t n = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) n += wave_n[w];
    c.tiles[tile] = (int64_t)n;
  }
}

// one workgroup per column: counts -> exclusive offsets in place, the total -> *count
template <class Args>
__global__ __launch_bounds__(kBlock) void hash_pack_scan_kernel(const Args a) {
  __shared__ int64_t wave_sum[kWavesPerBlock];
  const auto& c = a.col[blockIdx.x];
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  int64_t carry = 0;   // matches of the tiles before this pass (block-uniform)
  for (int64_t t0 = 0; t0 < c.n_tiles; t0 += (int64_t)kBlock * kScanPerThread) {   // (block-uniform bounds)
    const int64_t first = t0 + (int64_t)threadIdx.x * kScanPerThread;
    int64_t v[kScanPerThread];
    int64_t mine = 0;
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k) {
      v[k] = first + k < c.n_tiles ? c.tiles[first + k] : 0;
      mine += v[k];
    }
    // inclusive scan of `mine` across the wave, then across the four waves through LDS
    int64_t incl = mine;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int64_t up = (int64_t)__shfl_up((long long)incl, off, kWave);
      if (lane >= off) incl += up;
    }
    if (lane == kWave - 1) wave_sum[wave] = incl;
    __syncthreads();
    int64_t before = carry, total = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) {
      if (w < wave) before += wave_sum[w];
      total += wave_sum[w];
    }
    __syncthreads();   // (wave_sum is written again by the next pass)
    int64_t run = before + incl - mine;
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k) {
      if (first + k < c.n_tiles) c.tiles[first + k] = run;
      run += v[k];
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    *c.count = carry;
    c.scanned();
  }
}

template <class Args>
__global__ __launch_bounds__(kBlock) void hash_pack_write_kernel(const Args a) {
  __shared__ int32_t wave_n[kWavesPerBlock];
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const auto& c = a.col[ci];
  const int64_t tile = (int64_t)(b - a.tile_start[ci]);
  const int64_t first = tile * kSlotsPerTile + (int64_t)wave * kWave;
  const int64_t slot = first + lane;
  const bool take = c.selected(slot);
  const unsigned long long mask = __ballot(take);
  const int n = (int)__builtin_popcountll(mask);
  if (lane == 0) wave_n[wave] = n;
  __syncthreads();   // (every wave of the tile is here: nothing above returns)
  if (mask == 0ull) return;   // (wave-uniform)
  int64_t base = c.tiles[tile];
  for (int w = 0; w < wave; ++w) base += wave_n[w];
  const int64_t out_capacity = c.out_capacity;
  if (base >= out_capacity) return;   // (wave-uniform) the whole range lies behind the output
  const int below = rank_below(mask);
  if (take && base + below < out_capacity) {
    c.out_keys[base + below] = c.keys[slot];
    if (c.out_slots != nullptr) c.out_slots[base + below] = slot;
  }
  if (c.n_moves == 0) return;
  const int live_lane = compact_lanes(mask, take, lane);   // lane r < n: the lane of the r-th live slot
  for (int m = 0; m < c.n_moves; ++m) {
    const Move& mv = c.move[m];
    const int lanes_log2 = mv.lanes_log2;
    const int sub = lane & ((1 << lanes_log2) - 1);
    for (int r0 = 0; r0 < n; r0 += kWave >> lanes_log2) {   // (wave-uniform bounds)
      const int r = r0 + (lane >> lanes_log2);
      const int from = __shfl(live_lane, r & (kWave - 1), kWave);   // (every lane takes the shuffle)
      if (r < n && base + r < out_capacity) {
        copy_row(mv, mv.src + (first + from) * mv.src_pitch, mv.dst + (base + r) * mv.dst_pitch, sub,
                 1 << mv.lanes_log2);
      }
    }
  }
}

// the three launches of one argument struct: `tiles` = a.tile_start[a.n_cols]
template <class Args>
int launch_pack(const Args& a, int64_t tiles, hipStream_t stream) {
  hipLaunchKernelGGL(hash_pack_count_kernel<Args>, dim3((unsigned)tiles), dim3(kBlock), 0, stream, a);
  HBK_HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(hash_pack_scan_kernel<Args>, dim3((unsigned)a.n_cols), dim3(kBlock), 0, stream, a);
  HBK_HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(hash_pack_write_kernel<Args>, dim3((unsigned)tiles), dim3(kBlock), 0, stream, a);
  HBK_HIP_OK(hipGetLastError());
  return HBK_OK;
}

}  // namespace pack
}  // namespace hbk

#endif  // HBK_CSRC_HASH_PACK_H_
