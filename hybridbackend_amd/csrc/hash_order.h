// The orders in which a bounded hash table gives up its keys (hash_evict_to.hip selects, hash_spill.hip exports):
// an order is a list of kHalves signed 32-bit values of a slot, most significant first, each compared as
// u = value ^ 0x80000000 (signed order as unsigned):
//   LruOrder  {last_seen}         the oldest keys leave first
//   LfuOrder  {freq, last_seen}   the least frequently used, the oldest first among equally frequent ones: ONE 64-bit
//                                 key  k(slot) = ((uint64)(freq ^ 0x80000000) << 32) | (uint32)(last_seen ^ 0x80000000)
// need = live - max_size, cut = the smallest key at or below which at least `need` evictable slots lie, and every
// evictable slot with key <= cut leaves -- whole classes of equal keys together, no tie-break.
//
// The radix select takes three digits per half, 11 / 11 / 10 bits, most significant first: digit d cuts half d / 3.
// A table's state in the workspace, int32 words:
//   kLive, kNeed, kRemain, kPrefix + h (one per half), kAll, kCut + h (one per half); kState words in all
// and the report a call leaves, int32[kReportWords]:
//   {live_before, need, cut[0 .. kHalves), n_evicted (the select entries: n_selected), zeros}
// that is {live_before, need, cut, n_evicted} for LRU and {live_before, need, cut_freq, cut_last_seen, n_evicted,
// 0, 0, 0} for LFU.  Constants and device-inline functions only; internal to libhbk_core.so.
#ifndef HBK_CSRC_HASH_ORDER_H_
#define HBK_CSRC_HASH_ORDER_H_

#include "hash_common.h"

namespace hbk {

// a digit inside its 32-bit half
__host__ __device__ constexpr int digit_shift(int digit) { return digit % 3 == 0 ? 21 : digit % 3 == 1 ? 10 : 0; }
__host__ __device__ constexpr int digit_bits(int digit) { return digit % 3 == 2 ? 10 : 11; }

__device__ inline uint32_t order_half(int32_t v) { return (uint32_t)v ^ 0x80000000u; }

// the state words of a table
constexpr int kLive = 0;      // live slots (hist pass 0)
constexpr int kNeed = 1;      // live - max_size (pick 0); <= 0: the table is left alone
constexpr int kRemain = 2;    // the need that falls into the chosen bin
constexpr int kState = 8;

template <int HALVES>
struct OrderWords {
  static constexpr int kHalves = HALVES;
  static constexpr int kDigits = 3 * HALVES;
  static constexpr int kPrefix = 3;               // + h: the digits chosen so far of half h, right-aligned; whole
                                                  // once the half's three digits are through
  static constexpr int kAll = 3 + HALVES;         // != 0: fewer evictable slots than need, all go (cuts = INT32_MAX)
  static constexpr int kCut = 4 + HALVES;         // + h: the cut's half h as u (the last pick, or pick 0 with kAll)
  static constexpr int kReportWords = 4 * HALVES;
  static constexpr int kReportCut = 2;            // + h
  static constexpr int kReportEvicted = 2 + HALVES;
  static_assert(kCut + HALVES <= kState, "the state words");
};

struct LruOrder : OrderWords<1> {
  typedef uint32_t Key;
  static __device__ inline uint32_t half(int, int32_t, int32_t seen) { return order_half(seen); }
  static __device__ inline Key key(int32_t, int32_t seen) { return order_half(seen); }
  static __device__ inline Key cut(const int32_t* state) { return (uint32_t)state[kCut]; }
  // the spill: a finished report selects the slot
  static __device__ inline bool selected(const int32_t* report, int32_t, int32_t seen) {
    return report[1] > 0 && seen <= report[2];
  }
};

struct LfuOrder : OrderWords<2> {
  typedef uint64_t Key;
  static __device__ inline uint32_t half(int h, int32_t freq, int32_t seen) { return order_half(h == 0 ? freq : seen); }
  static __device__ inline Key key(int32_t freq, int32_t seen) {
    return ((uint64_t)order_half(freq) << 32) | (uint64_t)order_half(seen);
  }
  static __device__ inline Key cut(const int32_t* state) {
    return ((uint64_t)(uint32_t)state[kCut] << 32) | (uint64_t)(uint32_t)state[kCut + 1];
  }
  static __device__ inline bool selected(const int32_t* report, int32_t freq, int32_t seen) {
    return report[1] > 0 && key(freq, seen) <= key(report[2], report[3]);
  }
};

}  // namespace hbk

#endif  // HBK_CSRC_HASH_ORDER_H_
