"""Sequential restatement of hbk_hash_rehash_n (include/hbk.h) for tests/test_hash_rehash_abi.py and
tests/test_gpu_hash_rehash.py: the source slots taken in order, each live key into the first EMPTY slot of its
hashed destination slab, else of the next slab (wrapping) -- hash_ref.fill over the live keys.  The device
places concurrently, so slot numbers may differ; what must agree is stated where the tests compare."""
import numpy as np

from tests.support import hash_ref as ref

EMPTY = ref.EMPTY
TOMBSTONE = EMPTY + 1


def live_mask(keys, expiring):
  """The source slots that hold a key: not EMPTY, and not TOMBSTONE in an expiring table."""
  keys = np.asarray(keys, np.int64)
  live = keys != EMPTY
  return live & (keys != TOMBSTONE) if expiring else live


def rehash(src_keys, dst_slab_size, dst_slab_count, expiring, moves=()):
  """Returns (dst_keys, new_slots, n_moved, n_failed).  `moves`: (src, dst) numpy arrays with one row per slot;
  dst is modified in place: row new_slots[s] = row s of src for every key that was placed."""
  src_keys = np.asarray(src_keys, np.int64)
  dst = np.full(dst_slab_size * dst_slab_count, EMPTY, np.int64)
  live = live_mask(src_keys, expiring)
  new_slots = np.full(src_keys.size, -1, np.int64)
  new_slots[live] = ref.fill(dst, dst_slab_size, src_keys[live])
  placed = new_slots >= 0
  for src, out in moves:
    out[new_slots[placed]] = src[placed]
  return dst, new_slots, int(placed.sum()), int((live & ~placed).sum())
