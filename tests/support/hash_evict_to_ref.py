"""Plain numpy restatement of hbk_hash_evict_to_n (include/hbk.h, "Bounded tables") for
tests/test_hash_evict_to_abi.py and tests/test_gpu_hash_evict_to.py, on top of tests/support/hash_expiry_ref.py.

* `cut_of`: live, need and the cut -- the smallest last_seen value (signed) at or below which at least `need`
  evictable slots lie; INT32_MAX when there are fewer evictable slots than that.
* `evict_to`: what the call does to the arrays, in place, and its report {live_before, need, cut, n_evicted}.
"""
import numpy as np

from tests.support import hash_expiry_ref as xref

EMPTY, TOMBSTONE = xref.EMPTY, xref.TOMBSTONE
INT32_MAX = 2 ** 31 - 1


def evictable_mask(cache, freq, keep_freq=0):
  live = (cache != EMPTY) & (cache != TOMBSTONE)
  return live if keep_freq == 0 else live & (freq < keep_freq)


def cut_of(cache, last_seen, freq, max_size, keep_freq=0):
  """(live, need, cut); cut is 0 when need <= 0."""
  live = int(((cache != EMPTY) & (cache != TOMBSTONE)).sum())
  need = live - int(max_size)
  if need <= 0:
    return live, need, 0
  ages = np.sort(last_seen[evictable_mask(cache, freq, keep_freq)].astype(np.int64))
  if ages.size < need:
    return live, need, INT32_MAX
  return live, need, int(ages[need - 1])   # the need-th oldest: the smallest v with #{<= v} >= need


def evict_to(cache, last_seen, freq, max_size, keep_freq=0, companions=()):
  """The call, in place; `companions`: (array [capacity, >= dim], dim, value).  Returns (report, evicted mask);
  report = int32 [4] {live_before, need, cut, n_evicted}."""
  live, need, cut = cut_of(cache, last_seen, freq, max_size, keep_freq)
  mask = np.zeros(cache.shape, bool)
  if need > 0:
    mask = evictable_mask(cache, freq, keep_freq) & (last_seen.astype(np.int64) <= cut)
    cache[mask] = TOMBSTONE
    last_seen[mask] = 0
    freq[mask] = 0
    for array, dim, value in companions:
      array[mask, :dim] = value
  return np.array([live, need, cut, int(mask.sum())], np.int32), mask
