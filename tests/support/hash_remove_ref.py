"""Numpy restatement of hbk_hash_remove_n's effect on a table's arrays (include/hbk.h), independent of the walk: the
slot of a key is where(cache == key).  What the GPU tests compare with, bit for bit."""
import numpy as np

from tests.support import hash_expiry_ref as xref

EMPTY = xref.EMPTY
TOMBSTONE = xref.TOMBSTONE


def slots_of(cache, ids):
  """The slot every id holds, or -1; the sentinels hold none."""
  cache = np.asarray(cache, np.int64)
  ids = np.asarray(ids, np.int64)
  out = np.full(ids.shape, -1, np.int64)
  where = {int(k): s for s, k in enumerate(cache.tolist()) if k not in (EMPTY, TOMBSTONE)}
  assert len(where) == int(((cache != EMPTY) & (cache != TOMBSTONE)).sum()), 'a key is stored twice'
  for i, k in enumerate(ids.tolist()):
    out[i] = where.get(k, -1)
  return out


def remove(cache, last_seen, freq, ids, companions=()):
  """The removal, in place; `companions`: (array [capacity, >= dim], dim, value).  Returns (slots, n_removed): the
  slot of every occurrence before the call, and the distinct ids removed."""
  slots = slots_of(cache, ids)
  mask = np.zeros(cache.shape, bool)
  mask[slots[slots >= 0]] = True
  cache[mask] = TOMBSTONE
  last_seen[mask] = 0
  freq[mask] = 0
  for array, dim, value in companions:
    array[mask, :dim] = value
  return slots, int(mask.sum())
