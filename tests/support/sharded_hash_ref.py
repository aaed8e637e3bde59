"""The numpy model of sharded hash tables: one dict-by-raw-id table per column for the WHOLE world (the Model of
tests/test_gpu_hash.py restated), plus who owns what.  A row's start depends on (key, seed, j) alone
(hash_ref.init_rows), so the forward of any sharding is checkable bit for bit."""
import numpy as np

from tests.support import hash_ref as ref


def owner(keys, world):
  """floormod(key, world): numpy's % on int64 is floormod."""
  return np.asarray(keys, np.int64) % world


class Model:
  """One column: every distinct raw id of the world has a row (its initial row to start with); ids are renamed
  to their rank among the distinct ids, which the restatements of tests/support/reference.py treat as rows."""

  def __init__(self, ids_of_all_ranks, dim, seed, scale):
    self.uniq = np.unique(np.concatenate([np.asarray(i, np.int64) for i in ids_of_all_ranks]))
    self.w = ref.init_rows(self.uniq, dim, seed, scale)

  def index(self, ids):
    at = np.searchsorted(self.uniq, ids)
    assert (self.uniq[at] == ids).all()
    return at.astype(np.int64)

  def owned(self, world, rank):
    """Positions in `uniq` of the keys `rank` owns."""
    return np.nonzero(owner(self.uniq, world) == rank)[0]


def keys_without_overflow(rng, n, slab_count, slab_size, extra=()):
  """n distinct int64 keys (never a sentinel), `extra` first, at most slab_size - 1 of them per home slab: no slab
  overflows into its neighbour, so the key set of every slab is reproducible."""
  per_slab, out, seen = {}, [], set()
  cand = list(extra) + rng.randint(-2 ** 62, 2 ** 62, size=8 * n + 64, dtype=np.int64).tolist()
  for k in cand:
    h = ref.home_slab(k, slab_count)
    if k in seen or per_slab.get(h, 0) >= slab_size - 1:
      continue
    seen.add(k)
    per_slab[h] = per_slab.get(h, 0) + 1
    out.append(k)
    if len(out) == n:
      break
  assert len(out) == n
  return np.array(out, np.int64)
