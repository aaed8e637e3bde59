"""Numpy restatement of hbk_hash_missing_n (include/hbk.h), independent of the walk and of the scratch set: the
effective id list of a column, the keys a table's arrays hold, the slot of every position and the distinct missed ids
in the order of their first occurrence.  What the GPU tests compare with, bit for bit, order included."""
import numpy as np

from tests.support import hash_expiry_ref as xref

EMPTY = xref.EMPTY
TOMBSTONE = xref.TOMBSTONE


def effective(ids, row_splits=None, max_len=None, pad_id=None):
  """``(ids_by_position, there)``: the id list as the call reads it.  Flat (``max_len`` None): the ids, all there.
  Sequence: position ``b * T + t`` holds the sample's t-th id for ``t < min(len_b, T)``, then the pad id -- or
  nothing (``there`` False) without one.  A row_splits entry pointing outside the ids names no id."""
  ids = np.asarray(ids, np.int64)
  if max_len is None:
    return ids.copy(), np.ones(ids.shape, bool)
  T = int(max_len)
  splits = np.arange(ids.size + 1, dtype=np.int64) if row_splits is None else np.asarray(row_splits, np.int64)
  B = splits.size - 1
  out = np.full(B * T, EMPTY, np.int64)
  there = np.zeros(B * T, bool)
  for b in range(B):
    start, length = int(splits[b]), int(splits[b + 1] - splits[b])
    L = min(max(length, 0), T)
    for t in range(T):
      p = b * T + t
      if t < L and 0 <= start + t < ids.size:
        out[p], there[p] = ids[start + t], True
      elif pad_id is not None:
        out[p], there[p] = pad_id, True
  return out, there


def held(cache):
  """key -> slot of the keys the key array holds: a TOMBSTONE and an EMPTY slot hold none."""
  cache = np.asarray(cache, np.int64)
  where = {int(k): s for s, k in enumerate(cache.tolist()) if k not in (EMPTY, TOMBSTONE)}
  assert len(where) == int(((cache != EMPTY) & (cache != TOMBSTONE)).sum()), 'a key is stored twice'
  return where


def missing(cache, ids, row_splits=None, max_len=None, pad_id=None):
  """``(slots, missed)``: the pure find's answer per position (-1 where nothing is there) and the distinct ids of the
  effective list the table does not hold, first occurrence first; the sentinels are never reported."""
  e, there = effective(ids, row_splits, max_len, pad_id)
  where = held(cache)
  slots = np.full(e.shape, -1, np.int64)
  missed, seen = [], set()
  for p, (k, here) in enumerate(zip(e.tolist(), there.tolist())):
    if not here:
      continue
    slots[p] = where.get(k, -1)
    if slots[p] < 0 and k not in (EMPTY, TOMBSTONE) and k not in seen:
      seen.add(k)
      missed.append(k)
  return slots, np.asarray(missed, np.int64)
