"""hbk_hash_export_n and an import restated on the host: the selection, the order and the moves in numpy, and
the upsert as a dict by key.  The export is a function of the table's arrays alone, so the GPU tests compare bit
for bit."""
import numpy as np

EMPTY = np.int64(-2 ** 63)
TOMBSTONE = np.int64(-2 ** 63 + 1)


def live_mask(keys, expiring):
  """Slots that hold a key: not EMPTY, and not TOMBSTONE on an expiring table."""
  live = keys != EMPTY
  return live & (keys != TOMBSTONE) if expiring else live


def select(keys, expiring, last_seen=None, since=0):
  """The exported source slots, ascending."""
  take = live_mask(keys, expiring)
  if since > 0:
    take = take & (last_seen >= since)
  return np.nonzero(take)[0].astype(np.int64)


def export(keys, expiring, arrays, last_seen=None, since=0, out_capacity=None):
  """(count, out_keys, out_slots, [packed array per move]): the first min(count, out_capacity) matches in slot
  order; count is always the total."""
  slots = select(keys, expiring, last_seen, since)
  count = slots.size
  if out_capacity is not None:
    slots = slots[:out_capacity]
  return count, keys[slots], slots, [np.ascontiguousarray(a[slots]) for a in arrays]


def as_map(keys, *arrays):
  """key -> tuple of the bytes of its row in every array: two tables hold the same state iff their maps are equal."""
  assert np.unique(keys).size == keys.size
  return {int(k): tuple(a[i].tobytes() for a in arrays) for i, k in enumerate(keys.tolist())}


def upsert(state, keys, *arrays):
  """The import as a dict: a key the state holds takes the imported payload, a new key is added."""
  out = dict(state)
  out.update(as_map(keys, *arrays))
  return out
