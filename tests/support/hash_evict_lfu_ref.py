"""Plain numpy restatement of hbk_hash_evict_to_lfu_n (include/hbk.h, "Bounded tables in LFU order") for
tests/test_hash_evict_lfu_abi.py and tests/test_gpu_hash_evict_lfu.py, on top of tests/support/hash_evict_to_ref.py.

* `order_key`: k(slot) = ((freq ^ 0x80000000) << 32) | (last_seen ^ 0x80000000), as Python-exact uint64.
* `cut_of`: live, need and the cut -- the evictable slots sorted by (freq, last_seen), both signed; the cut is the
  need-th smallest pair; (INT32_MAX, INT32_MAX) when there are fewer evictable slots than that.
* `evict_to`: what the call does to the arrays, in place, and its report
  {live_before, need, cut_freq, cut_last_seen, n_evicted, 0, 0, 0}.
* `select`: the report of the select entry (n_selected in the place of n_evicted); nothing is written.
* `mask_of`: the predicate of hbk_hash_spill_lfu_n, from a selection: holds a key, not kept by keep_freq, need > 0
  and (freq, last_seen) <= (cut_freq, cut_last_seen).
* `spill`: (export arrays in ascending slot order, arrays after, n_evicted, count), the capacity guard included.
"""
import numpy as np

from tests.support import hash_evict_to_ref as tref

EMPTY, TOMBSTONE = tref.EMPTY, tref.TOMBSTONE
INT32_MAX = tref.INT32_MAX
evictable_mask = tref.evictable_mask


def order_key(freq, last_seen):
  hi = (freq.astype(np.int64) + 2 ** 31).astype(np.uint64)      # x ^ 0x80000000 of a signed int32, as unsigned
  lo = (last_seen.astype(np.int64) + 2 ** 31).astype(np.uint64)
  return (hi << np.uint64(32)) | lo


def cut_of(cache, last_seen, freq, max_size, keep_freq=0):
  """(live, need, cut_freq, cut_last_seen); both cuts are 0 when need <= 0."""
  live = int(((cache != EMPTY) & (cache != TOMBSTONE)).sum())
  need = live - int(max_size)
  if need <= 0:
    return live, need, 0, 0
  ev = evictable_mask(cache, freq, keep_freq)
  if int(ev.sum()) < need:
    return live, need, INT32_MAX, INT32_MAX
  f, s = freq[ev].astype(np.int64), last_seen[ev].astype(np.int64)
  order = np.lexsort((s, f))                                      # by freq, then by last_seen
  at = order[need - 1]                                            # the need-th smallest pair
  return live, need, int(f[at]), int(s[at])


def selected_mask(cache, last_seen, freq, max_size, keep_freq=0):
  live, need, cut_f, cut_s = cut_of(cache, last_seen, freq, max_size, keep_freq)
  mask = np.zeros(cache.shape, bool)
  if need > 0:
    f, s = freq.astype(np.int64), last_seen.astype(np.int64)
    mask = evictable_mask(cache, freq, keep_freq) & ((f < cut_f) | ((f == cut_f) & (s <= cut_s)))
  return (live, need, cut_f, cut_s), mask


def select(cache, last_seen, freq, max_size, keep_freq=0):
  """The select entry's report, int32 [8]; and the mask of the selected slots."""
  head, mask = selected_mask(cache, last_seen, freq, max_size, keep_freq)
  return np.array(list(head) + [int(mask.sum()), 0, 0, 0], np.int32), mask


def evict_to(cache, last_seen, freq, max_size, keep_freq=0, companions=()):
  """The call, in place; `companions`: (array [capacity, >= dim], dim, value).  Returns (report, evicted mask);
  report = int32 [8] {live_before, need, cut_freq, cut_last_seen, n_evicted, 0, 0, 0}."""
  report, mask = select(cache, last_seen, freq, max_size, keep_freq)
  cache[mask] = TOMBSTONE
  last_seen[mask] = 0
  freq[mask] = 0
  for array, dim, value in companions:
    array[mask, :dim] = value
  return report, mask


def mask_of(cache, last_seen, freq, selection, keep_freq=0):
  if int(selection[1]) <= 0:
    return np.zeros(cache.shape, bool)
  f, s = freq.astype(np.int64), last_seen.astype(np.int64)
  cut_f, cut_s = int(selection[2]), int(selection[3])
  return evictable_mask(cache, freq, keep_freq) & ((f < cut_f) | ((f == cut_f) & (s <= cut_s)))


def spill(cache, last_seen, freq, selection, keep_freq=0, moves=(), companions=(), out_capacity=None):
  """`moves`: per-slot arrays ([capacity] or [capacity, >= words]) with their widths, (array, words); `companions`:
  (array [capacity, >= dim], dim, value).  Nothing is modified.  Returns (export, after, n_evicted, count): export =
  dict(keys, src_slots, moves=[...]) of the first min(count, out_capacity) selected slots in ascending slot order;
  after = dict(cache, last_seen, freq, companions=[...]); with count > out_capacity the table stays as it is."""
  mask = mask_of(cache, last_seen, freq, selection, keep_freq)
  where = np.flatnonzero(mask)
  count = int(where.size)
  out_capacity = count if out_capacity is None else int(out_capacity)
  kept = where[:out_capacity]
  export = dict(keys=cache[kept].copy(), src_slots=kept.astype(np.int64),
                moves=[(a[kept] if a.ndim == 1 else a[kept, :w]).copy() for a, w in moves])
  after = dict(cache=cache.copy(), last_seen=last_seen.copy(), freq=freq.copy(),
               companions=[a.copy() for a, _, _ in companions])
  n_evicted = 0
  if count <= out_capacity:                                               # all or nothing
    n_evicted = count
    after['cache'][mask] = TOMBSTONE
    after['last_seen'][mask] = 0
    after['freq'][mask] = 0
    for a, (_, dim, value) in zip(after['companions'], companions):
      a[mask, :dim] = value
  return export, after, n_evicted, count
