"""Plain sequential restatement of the admission filter (include/hbk.h, hbk_hash_insert_admit_n and
hbk_hash_insert_expiring_admit_n) for tests/test_hash_admission_abi.py and tests/test_gpu_hash_admission.py.

* `cells`: the cell of every key in every row of the count-min sketch.
* `translate`: one call with insert != 0, count then admit: phase 1 over ALL keys (the table's own find; the
  misses add 1 to their cells, with the ceiling), then phase 2 in key order through `hash_ref.fill` /
  `hash_expiry_ref.insert` for the occurrences whose estimate reaches `min_freq`.  Which ids are admitted, the
  sketch and the counters are what the device must give; slot numbers only where the order cannot matter.
"""
import numpy as np

from tests.support import hash_expiry_ref as xref
from tests.support import hash_ref

EMPTY = hash_ref.EMPTY
TOMBSTONE = xref.TOMBSTONE
CEILING = 2 ** 30


def cells(keys, depth, width, seed=0):
  """int64 [depth, n]: murmur3_hash32(key ^ (int64)((uint64)(seed + r + 1) * golden ratio)) % width."""
  keys = np.asarray(keys, np.int64)
  out = np.zeros((depth, keys.size), np.int64)
  for r in range(depth):
    mix = ((int(seed) + r + 1) * hash_ref.GOLDEN_RATIO) & 0xffffffffffffffff
    x = keys.astype(np.uint64) ^ np.uint64(mix)
    out[r] = hash_ref.murmur3_np(x.astype(np.int64)).astype(np.int64) % width
  return out


def estimate(sketch, keys, seed=0):
  """min over the rows of every key's cell."""
  depth, width = sketch.shape
  at = cells(keys, depth, width, seed)
  return sketch[np.arange(depth)[:, None], at].min(axis=0)


def find_plain(cache, slab_size, key):
  """Slot of `key` by the plain rule's walk (a key never sits behind a slab with an EMPTY slot), or -1."""
  slab_count = cache.size // slab_size
  if key == EMPTY:
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


def translate(cache, slab_size, keys, sketch, min_freq, expiring=False, seed=0, last_seen=None, freq=None, step=0):
  """One admitting call; `cache`, `sketch` (and `last_seen` / `freq` of an expiring table) are modified in
  place.  Returns (admitted, slots, counters): `admitted` the mask of the occurrences phase 2 sent to the
  find-or-insert, `counters` a dict of what the call adds to n_inserted / n_failed / n_reused / filtered."""
  keys = np.asarray(keys, np.int64)
  depth, width = sketch.shape
  sentinels = (EMPTY, TOMBSTONE) if expiring else (EMPTY,)
  at = cells(keys, depth, width, seed)
  slots = np.full(keys.size, -1, np.int64)
  pending = np.zeros(keys.size, bool)
  n_failed = 0
  # phase 1: count
  for n, k in enumerate(keys.tolist()):
    if k in sentinels:
      n_failed += 1
      continue
    s = xref.find(cache, slab_size, k) if expiring else find_plain(cache, slab_size, k)
    if s >= 0:
      slots[n] = s
      if expiring:
        last_seen[s] = step
        if freq[s] < CEILING:
          freq[s] += 1
      continue
    pending[n] = True
    for r in range(depth):
      if sketch[r, at[r, n]] < CEILING:
        sketch[r, at[r, n]] += 1
  # phase 2: admit, in key order
  admitted = pending & (sketch[np.arange(depth)[:, None], at].min(axis=0) >= min_freq)
  n_inserted = n_reused = 0
  chosen = keys[admitted]
  if expiring:
    got, n_inserted, n_reused, _ = xref.insert(cache, slab_size, chosen, last_seen, freq, step)
  else:
    before = int((cache != EMPTY).sum())
    got = hash_ref.fill(cache, slab_size, chosen)
    n_inserted = int((cache != EMPTY).sum()) - before
  slots[admitted] = got
  n_failed += int((got < 0).sum())
  counters = {'inserted': n_inserted, 'failed': n_failed, 'reused': n_reused,
              'filtered': int((pending & ~admitted).sum())}
  return admitted, slots, counters
