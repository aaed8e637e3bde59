// The scratch set of the miss lists (hash_missing.hip, hash_missing_runs.hip), once: the distinct missed ids of a
// column and, beside every id, the smallest position that missed with it.  Both entries claim into it from their own
// claim kernel -- they find their positions differently -- and select from it in hash_pack.h's count and write.
//
// The set.  Open addressing over S = pow2 >= 2 * positions cells (at least 64), home cell = murmur3_i64(id) & (S - 1),
// linear probing, EMPTY = INT64_MIN; first[cell] is INT32_MAX until a position claims the cell's id.  Invariants:
//   a cell only ever goes EMPTY -> id, claimed with a 64-bit agent-scope compare-and-swap;
//   first[] only falls: atomicMin(first[cell], p), and not even that when the first[cell] a lane reads is already
//     below p (on a Zipf(1.2) batch the claim and compaction took 285 us with every occurrence's atomic and 185 us
//     with the load: profiles/hash_fault_in.txt);
//   a probe reads at most S cells, the bound written out in both walks: the distinct ids are at most S / 2, so a
//     lane that loses a swap to ANOTHER id steps to the next cell and a lane that loses to its own id is done.  No
//     lane waits for another: no spin, no retry of a cell.
//
// Memory rules.  The claim reads the set with relaxed agent-scope atomic loads and writes it with the swap and the
// atomicMin, all served by the device's L2 whatever CU issues them; a stale EMPTY read only costs a failed swap,
// whose returned value is the cell's.  The kernel boundary publishes the set and first[]: count and write read them
// with plain loads (first_position), as hash_insert.hip's find reads a key array nobody writes.
//
// The workspace of a call: the sets of all columns, first[] of all columns, the compaction's tile counts of all
// columns, then what the entry adds.  The call clears its own sets (plain stores), so it asks nothing of what the
// workspace held and can be captured and replayed.  Internal to libhbk_core.so.
#ifndef HBK_CSRC_HASH_MISS_SET_H_
#define HBK_CSRC_HASH_MISS_SET_H_

#include "hash_pack.h"

namespace hbk {
namespace miss_set {

using namespace pack;

constexpr int kChunks = 4;                              // 64-position chunks per wave of a claim
constexpr int kClaimPerBlock = kBlock * kChunks;        // a whole number of 256-position tiles
constexpr int64_t kMinCells = 64;
constexpr int32_t kNoPosition = 0x7fffffff;             // first[] of a cell nobody claimed
constexpr int kClearBlocks = 4096;                      // the clear's grid at the most: it strides

// the cells of a column of `positions` positions: at most half of them are ever taken
inline int64_t cells_of(int64_t positions) {
  int64_t s = kMinCells;
  while (s < 2 * positions) s <<= 1;
  return s;
}

// 16-byte stores: the cells of a call are a multiple of 64 and both arrays start 16-byte aligned
static __global__ __launch_bounds__(kBlock) void hash_miss_set_clear_kernel(longlong2* set, int4* first,
                                                                            int64_t cells) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < (cells >> 1); i += stride) {
    set[i] = make_longlong2(kEmptyKey, kEmptyKey);
    if (i < (cells >> 2)) first[i] = make_int4(kNoPosition, kNoPosition, kNoPosition, kNoPosition);
  }
}

// the id of a missed position into the set, its position into first[]: at most S = mask + 1 cells are read
__device__ inline void claim_cell(long long* set, int32_t* first, uint64_t mask, long long id, int32_t p) {
  uint64_t cell = (uint64_t)murmur3_i64((int64_t)id) & mask;
  for (uint64_t k = 0; k <= mask; ++k) {
    long long cur = __hip_atomic_load(set + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEmptyKey) {
      long long expected = kEmptyKey;
      const bool won = __hip_atomic_compare_exchange_strong(set + cell, &expected, id, __ATOMIC_RELAXED,
                                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      cur = won ? id : expected;   // (lost: the cell's key now, ours or another's)
    }
    if (cur == id) {
      // (first[] only falls: a position not below the value read changes nothing, and a stale read only costs the
      // atomic -- the load spares a hot id's later occurrences their turn at one address)
      if (__hip_atomic_load(first + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > p) {
        __hip_atomic_fetch_min(first + cell, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      return;
    }
    cell = (cell + 1) & mask;
  }
}

// after the claim's kernel boundary: the first position that missed with `id`, or kNoPosition when the set does
// not hold it (the claim's walk; it ends at the id or at an EMPTY cell)
__device__ inline int32_t first_position(const long long* set, const int32_t* first, uint64_t mask, long long id) {
  uint64_t cell = (uint64_t)murmur3_i64((int64_t)id) & mask;
  for (uint64_t k = 0; k <= mask; ++k) {
    const long long cur = set[cell];
    if (cur == id) return first[cell];
    if (cur == kEmptyKey) return kNoPosition;
    cell = (cell + 1) & mask;
  }
  return kNoPosition;
}

// what both miss lists ask of a column besides its ids: an expiring table, and where the answer goes
inline int check_column(const char* who, int32_t c, const hbk_hash_expiry_t& exp, const int64_t* count,
                        int64_t out_capacity, const int64_t* out_ids) {
  HBK_REQUIRE(exp.last_seen != nullptr, "%s: column %d: last_seen is NULL (expiring tables only)", who, c);
  HBK_REQUIRE(exp.freq != nullptr, "%s: column %d: freq is NULL (expiring tables only)", who, c);
  HBK_REQUIRE(count != nullptr, "%s: column %d: count is NULL", who, c);
  HBK_REQUIRE(out_capacity >= 0, "%s: column %d: out_capacity must be >= 0, got %lld", who, c,
              (long long)out_capacity);
  HBK_REQUIRE(out_capacity == 0 || out_ids != nullptr, "%s: column %d: out_ids is NULL with out_capacity %lld", who,
              c, (long long)out_capacity);
  return HBK_OK;
}

// the cells and tiles of all columns of a call, and the bytes they take; an entry may add bytes per tile
struct Layout {
  int64_t cells;
  int64_t tiles;
  size_t bytes(size_t more_per_tile = 0) const {
    return (size_t)cells * (sizeof(long long) + sizeof(int32_t)) + (size_t)tiles * (sizeof(int64_t) + more_per_tile);
  }
};

// The workspace as the columns of a call take it, one after the other: a column reads set, first and tiles, then
// steps them by its cells and tiles.
struct Workspace {
  long long* set;
  int32_t* first;
  int64_t* tiles;
  void take(int64_t cells, int64_t n_tiles) {
    set += cells;
    first += cells;
    tiles += n_tiles;
  }
};

// Checks the caller's workspace against the `need` bytes that `sizer` (the entry's own) reports, carves it -- the
// sets, first[], the tile counts; what an entry adds lies behind the l.tiles tile counts -- and launches the clear.
inline int open_workspace(const char* who, const char* sizer, void* workspace, size_t workspace_bytes, size_t need,
                          const Layout& l, hipStream_t stream, Workspace* w) {
  if (need != 0) {
    HBK_REQUIRE(workspace != nullptr, "%s: workspace is NULL (%s says how large: %zu bytes)", who, sizer, need);
    HBK_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    HBK_REQUIRE(workspace_bytes >= need, "%s: workspace_bytes %zu is too small: %zu bytes are needed", who,
                workspace_bytes, need);
  }
  w->set = static_cast<long long*>(workspace);
  w->first = reinterpret_cast<int32_t*>(w->set + l.cells);      // (cells: a multiple of 64)
  w->tiles = reinterpret_cast<int64_t*>(w->first + l.cells);
  if (l.cells != 0) {
    const int64_t blocks = ((l.cells >> 1) + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(hash_miss_set_clear_kernel, dim3((unsigned)(blocks < kClearBlocks ? blocks : kClearBlocks)),
                       dim3(kBlock), 0, stream, reinterpret_cast<longlong2*>(w->set), reinterpret_cast<int4*>(w->first),
                       l.cells);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

}  // namespace miss_set
}  // namespace hbk

#endif  // HBK_CSRC_HASH_MISS_SET_H_
