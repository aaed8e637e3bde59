"""Plain numpy restatement of hbk_hash_evict_to_select_n and hbk_hash_spill_n (include/hbk.h, "Spilling") for
tests/test_hash_spill_abi.py and tests/test_gpu_hash_spill.py, on top of tests/support/hash_evict_to_ref.py.

* `select`: the report {live_before, need, cut, n_selected}; nothing is written.
* `selected_mask`: the predicate of the spill, from a selection: holds a key, not kept by keep_freq, need > 0 and
  last_seen <= cut (signed).
* `spill`: (export arrays in ascending slot order, arrays after, n_evicted), the capacity guard included: with more
  selected slots than `out_capacity` the export is cut at the capacity and the table stays as it is.
"""
import numpy as np

from tests.support import hash_evict_to_ref as tref

EMPTY, TOMBSTONE, INT32_MAX = tref.EMPTY, tref.TOMBSTONE, tref.INT32_MAX


def select(cache, last_seen, freq, max_size, keep_freq=0):
  """int32 [4] {live_before, need, cut, n_selected}."""
  live, need, cut = tref.cut_of(cache, last_seen, freq, max_size, keep_freq)
  n = 0
  if need > 0:
    n = int((tref.evictable_mask(cache, freq, keep_freq) & (last_seen.astype(np.int64) <= cut)).sum())
  return np.array([live, need, cut, n], np.int32)


def selected_mask(cache, last_seen, freq, selection, keep_freq=0):
  if int(selection[1]) <= 0:
    return np.zeros(cache.shape, bool)
  return tref.evictable_mask(cache, freq, keep_freq) & (last_seen.astype(np.int64) <= int(selection[2]))


def spill(cache, last_seen, freq, selection, keep_freq=0, moves=(), companions=(), out_capacity=None):
  """`moves`: per-slot arrays ([capacity] or [capacity, >= words]) with their widths, (array, words); `companions`:
  (array [capacity, >= dim], dim, value) as tref.evict_to takes them.  Nothing is modified.  Returns
  (export, after, n_evicted, count): export = dict(keys, src_slots, moves=[...]) of the first min(count,
  out_capacity) selected slots in ascending slot order; after = dict(cache, last_seen, freq, companions=[...])."""
  mask = selected_mask(cache, last_seen, freq, selection, keep_freq)
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
