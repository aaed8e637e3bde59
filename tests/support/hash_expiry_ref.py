"""Plain sequential restatement of the expiring hash table (include/hbk.h, hbk_hash_insert_expiring_n and
hbk_hash_evict_n) for tests/test_hash_expiry_abi.py and tests/test_gpu_hash_expiry.py.

* `insert`: the placement rule with tombstones, keys taken one at a time: walk from the home slab to the
  first slab with an EMPTY slot, remember the first TOMBSTONE on the way, then take that tombstone, else the
  stopping slab's first EMPTY slot.  With `last_seen` / `freq` it also keeps the per-slot metadata.
* `evict_mask` / `evict`: the sweep's predicate and what it does to the arrays.
"""
import numpy as np

from tests.support import hash_ref

EMPTY = hash_ref.EMPTY
TOMBSTONE = EMPTY + 1
FREQ_CEILING = 2 ** 30


def find(cache, slab_size, key):
  """Slot of `key` by the probe's walk (stop at the first slab with an EMPTY slot), or -1."""
  slab_count = cache.size // slab_size
  if key in (EMPTY, TOMBSTONE):
    return -1
  slab = hash_ref.home_slab(key, slab_count)
  for _ in range(slab_count):
    s = cache[slab * slab_size:(slab + 1) * slab_size]
    hit = np.where(s == key)[0]
    if hit.size:
      return slab * slab_size + int(hit[0])
    if (s == EMPTY).any():
      return -1
    slab = (slab + 1) % slab_count
  return -1


def insert(cache, slab_size, keys, last_seen=None, freq=None, step=0):
  """Insert `keys` one at a time into `cache` (modified in place).  Returns (slots, n_inserted, n_reused,
  n_failed); -1 for EMPTY, TOMBSTONE and keys for which the walk met no free slot."""
  slab_count = cache.size // slab_size
  slots = np.full(len(keys), -1, np.int64)
  n_inserted = n_reused = 0
  for n, k in enumerate(np.asarray(keys, np.int64).tolist()):
    if k in (EMPTY, TOMBSTONE):
      continue
    slab = hash_ref.home_slab(k, slab_count)
    tomb, at = -1, -1
    for _ in range(slab_count):
      s = cache[slab * slab_size:(slab + 1) * slab_size]
      hit = np.where(s == k)[0]
      if hit.size:
        at = slab * slab_size + int(hit[0])
        break
      dead = np.where(s == TOMBSTONE)[0]
      if tomb < 0 and dead.size:
        tomb = slab * slab_size + int(dead[0])
      free = np.where(s == EMPTY)[0]
      if free.size:
        at = tomb if tomb >= 0 else slab * slab_size + int(free[0])
        break
      slab = (slab + 1) % slab_count
    else:
      at = tomb
    if at >= 0 and cache[at] != k:
      n_inserted += 1
      n_reused += int(cache[at] == TOMBSTONE)
      cache[at] = k
    slots[n] = at
    if at >= 0 and last_seen is not None:
      last_seen[at] = step
      if freq[at] < FREQ_CEILING:
        freq[at] += 1
  return slots, n_inserted, n_reused, int((slots < 0).sum())


def evict_mask(cache, last_seen, freq, step, steps_to_live, keep_freq=0):
  """The slots the sweep evicts."""
  live = (cache != EMPTY) & (cache != TOMBSTONE)
  if steps_to_live <= 0:
    return np.zeros(cache.shape, bool)
  idle = np.int64(step) - last_seen.astype(np.int64) >= steps_to_live
  rare = np.ones(cache.shape, bool) if keep_freq == 0 else freq < keep_freq
  return live & idle & rare


def evict(cache, last_seen, freq, step, steps_to_live, keep_freq=0, companions=()):
  """The sweep, in place; `companions`: (array [capacity, >= dim], dim, value).  Returns the evicted mask."""
  mask = evict_mask(cache, last_seen, freq, step, steps_to_live, keep_freq)
  cache[mask] = TOMBSTONE
  last_seen[mask] = 0
  freq[mask] = 0
  for array, dim, value in companions:
    array[mask, :dim] = value
  return mask
