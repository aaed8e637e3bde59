// The position side of a sequence lookup (include/hbk.h, "Sequence lookups"): position p of the flattened [B * T]
// grid -> its sample, its id, its table row and its grid word.  Shared by lookup_sequence.hip (fp32 tables) and
// lookup_sequence_lowbit.hip (16-bit and 8-bit tables), so that both forwards and the grid kernels place, pad,
// truncate and bucketize with ONE piece of code.  Col is the launch's column record; what is read of it:
//   ids, ids64, n_ids, splits (NULL: one id per sample), max_len (FastDiv of T), map (IdMap), pad_row, pad_grid,
//   grid (NULL: not wanted), lengths (NULL: not wanted).
#ifndef HBK_CSRC_SEQUENCE_POSITION_H_
#define HBK_CSRC_SEQUENCE_POSITION_H_

#include "lookup_common.h"

namespace hbk {
namespace {

// id -> (table row, grid word): id_to_row (lookup_common.h) with the bucketized id kept.  The grid word is
// what the backward's id_to_row, with bucket 0, maps to the same row: -1 where nothing is looked up.
__host__ __device__ inline uint64_t seq_map(const IdMap& m, int64_t id, int64_t* grid) {
  uint64_t r;
  if (m.bucket.d != 0) {
    r = floormod_i64(id, m.bucket);
  } else {
    if (id < 0) {
      *grid = -1;
      return kNoRow;
    }
    r = (uint64_t)id;
  }
  *grid = (int64_t)r;
  r = fastdiv(r, m.div);
  return r < m.rows ? r : kNoRow;
}

// The sample side of position p: t = p - b * T, the index of the sample's first id and L_b = min(len_b, T),
// the sample's length written by its first position.  False for a lane without a position.  The lanes of a
// wave hold CONSECUTIVE positions (lane l: p - l is lane 0's), valid ones first; every lane of the wave calls
// this.  The first lane of each sample inside the wave (t == 0, or lane 0) reads the sample's two row splits,
// the sample's other lanes take them by shuffle.
template <typename Col>
__device__ inline bool seq_sample(const Col& c, int64_t p, bool valid, int64_t* t_out, int32_t* beg_out,
                                  int64_t* len_out) {
  const int lane = lane_id();
  const int64_t T = (int64_t)c.max_len.d;
  int64_t b = 0, t = 0;
  if (valid) {
    b = (int64_t)fastdiv((uint64_t)p, c.max_len);
    t = p - b * T;
  }
  int32_t beg = 0, end = 0;
  if (valid && (t == 0 || lane == 0)) {
    if (c.splits != nullptr) {
      beg = c.splits[b];
      end = c.splits[b + 1];
    } else {
      beg = (int32_t)b;
      end = (int32_t)b + 1;
    }
  }
  const int src = lane - (int)(t < lane ? t : lane);
  beg = __shfl(beg, src, kWave);
  end = __shfl(end, src, kWave);
  if (!valid) return false;
  int64_t len = (int64_t)end - (int64_t)beg;
  len = len < 0 ? 0 : (len > T ? T : len);
  if (t == 0 && c.lengths != nullptr) c.lengths[b] = (int32_t)len;
  *t_out = t;
  *beg_out = beg;
  *len_out = len;
  return true;
}

// Position p of the column's grid -> its row, and the grid word written (every lane of the wave calls this)
template <typename Col>
__device__ inline uint64_t seq_position(const Col& c, int64_t p, bool valid) {
  int64_t t, len;
  int32_t beg;
  if (!seq_sample(c, p, valid, &t, &beg, &len)) return kNoRow;
  uint64_t row = c.pad_row;
  int64_t g = c.pad_grid;
  if (t < len) {
    const int64_t j = (int64_t)beg + t;
    row = kNoRow;
    g = -1;
    // (row splits that point outside the ids look nothing up)
    if ((uint64_t)j < (uint64_t)c.n_ids) row = seq_map(c.map, load_id(c.ids, c.ids64, j), &g);
  }
  if (c.grid != nullptr) __builtin_nontemporal_store(g, c.grid + p);
  return row;
}

}  // namespace
}  // namespace hbk

#endif  // HBK_CSRC_SEQUENCE_POSITION_H_
