"""A plain restatement of the stable partition (HbPartitionByModulo / HbPartitionByDualModuloStage{One,Two})
and the case lists of tests/test_partition_ref.py (CPU) and tests/test_gpu_partition_edges.py (GPU).

numpy only: nothing here comes from oracle/ or from the library.  tests/test_partition_ref.py holds the
restatement to the C oracle, to the reference's own cases and to the library's host entries, and holds every
list to the property its name states.

  shard(ids, P, M, stage)             the shard of every id
  partition(ids, P, M, stage, bucket) (output, sizes, indices) of one column
  assert_partition(got, want, ...)    exact comparison that says WHERE and WHAT KIND of error
"""
import numpy as np

TILE = 1024    # ids of one wave
CHUNK = 64     # ids of one ballot

DTYPES = {'int32': np.int32, 'int64': np.int64, 'uint32': np.uint32, 'uint64': np.uint64}

P_EDGES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000, 4095, 4096,
           4097, 16383, 16384)
# the chunk, the tile and the four-tile workgroup
LEN_EDGES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5000)
# (P, M): every P * M is below 2^31
DUAL_EDGES = ((1, 1), (1, 7), (7, 1), (8, 8), (9, 5), (64, 3), (65, 2), (3, 65), (16384, 131071),
              (2, (1 << 30) - 1))
COLUMN_COUNTS = (64, 65, 127, 128, 129, 257)
PATTERN_LEN = 5000


def _floormod(ids, d):
  """ids mod d in [0, d) as int64, d < 2^31."""
  ids = np.asarray(ids)
  d = int(d)
  assert 1 <= d < (1 << 31), d
  if ids.dtype.kind == 'i':
    return np.mod(ids, ids.dtype.type(d)).astype(np.int64)      # np.mod of signed integers is a floor-mod
  assert ids.dtype.kind == 'u', ids.dtype
  return (ids.astype(np.uint64) % np.uint64(d)).astype(np.int64)   # a remainder cannot wrap


def shard(ids, P, M=1, stage=0):
  """Shard of every id.  stage 0: v mod P.  Dual modulo: pre = v mod (P * M); stage 1: pre mod P, stage 2:
  pre div M (all floor forms)."""
  assert stage in (0, 1, 2), stage
  if stage == 0:
    return _floormod(ids, P)
  pre = _floormod(ids, int(P) * int(M))
  return pre % int(P) if stage == 1 else pre // int(M)


def partition(ids, P, M=1, stage=0, bucket=0):
  """(output, sizes, indices): ids grouped by shard, input order kept inside a shard; output[indices] == ids.
  bucket > 0: the ids are floor-modded by it first and the output holds those."""
  ids = np.ascontiguousarray(ids)
  if bucket:
    ids = _floormod(ids, bucket).astype(ids.dtype)
  s = shard(ids, P, M, stage)
  order = np.argsort(s, kind='stable')
  indices = np.empty(ids.size, np.int32)
  indices[order] = np.arange(ids.size, dtype=np.int32)
  sizes = np.bincount(s, minlength=int(P)).astype(np.int32)
  return ids[order], sizes, indices


def _kind_of_error(got_out, want_out, P, M, stage):
  """'stability' when got is the same ids still grouped by shard (the order inside a shard is wrong), 'base'
  otherwise (an id sits in another shard's run, or is not there at all)."""
  same_ids = got_out.shape == want_out.shape and np.array_equal(np.sort(got_out), np.sort(want_out))
  if same_ids and np.array_equal(shard(got_out, P, M, stage), shard(want_out, P, M, stage)):
    return 'stability'
  return 'base'


def assert_partition(got, want, what, P, M=1, stage=0, column=None):
  """got == want, (output, sizes, indices) each.  On a mismatch the AssertionError names the column, P, the
  first differing position with its tile (1024 ids) and chunk (64 ids), and the kind of error: `stability
  lost` (got is still a permutation grouped by shard) or `wrong base`."""
  g_out, g_sizes, g_idx = (np.asarray(x) for x in got)
  w_out, w_sizes, w_idx = (np.asarray(x) for x in want)
  where = '%s: column %s, P = %d' % (what, column, P) + (', M = %d, stage %d' % (M, stage) if stage else '')
  assert g_out.dtype == w_out.dtype and g_out.shape == w_out.shape, (where, g_out.dtype, g_out.shape,
                                                                     w_out.dtype, w_out.shape)
  assert g_sizes.shape == w_sizes.shape and g_idx.shape == w_idx.shape, (where, g_sizes.shape, g_idx.shape)

  def place(pos):
    return 'position %d (tile %d, chunk %d of the column)' % (pos, pos // TILE, pos // CHUNK)
  bad = np.flatnonzero(g_out != w_out)
  if bad.size:
    kind = _kind_of_error(g_out, w_out, P, M, stage)
    story = {'stability': 'stability lost: the ids are grouped by shard but not in input order',
             'base': 'wrong base: not a permutation grouped by shard'}[kind]
    pos = int(bad[0])
    raise AssertionError('%s: output differs at %s, %d positions in all; %s; got %r, want %r; sizes %s' % (
      where, place(pos), bad.size, story, g_out[pos], w_out[pos],
      'equal' if np.array_equal(g_sizes, w_sizes) else 'differ too'))
  bad = np.flatnonzero(g_idx != w_idx)
  if bad.size:
    pos = int(bad[0])
    raise AssertionError('%s: indices differ at input %s, %d in all (the output is right); got %d, want %d' % (
      where, place(pos), bad.size, g_idx[pos], w_idx[pos]))
  bad = np.flatnonzero(g_sizes != w_sizes)
  if bad.size:
    p = int(bad[0])
    raise AssertionError('%s: sizes differ at shard %d, %d in all (output and indices are right); got %d, '
                         'want %d' % (where, p, bad.size, g_sizes[p], w_sizes[p]))


# ---- ids ---------------------------------------------------------------------------------------------------
def _rng(*key):
  return np.random.default_rng([int(k) & 0xffffffff for k in key])


def edge_ids(dtype, P, M=1):
  """The ids at which a shard computation goes wrong: the ends of the type, the ids around zero, around
  multiples of d = P * M (the first ones, those next to 2^31, 2^32 and 2^62, the largest and the smallest that
  fit) and around 2^32; for the unsigned types also 2^63 and 2^64 - 1.  Distinct, in a fixed order."""
  info = np.iinfo(dtype)
  lo, hi = int(info.min), int(info.max)
  d = int(P) * int(M)
  vals = [lo, hi, 0, 1, -1, 2, -2]
  ks = [0, 1, -1]
  for big in (1 << 31, 1 << 32, 1 << 62):
    ks += [big // d, -(big // d), big // d + 1]          # the multiples of d next to 2^31, 2^32, 2^62
    ks += [big, -big]                                    # and d times them, where that fits
  ks += [hi // d, -((-lo) // d)]
  for k in ks:
    vals += [k * d - 1, k * d, k * d + 1]
  for big in (1 << 31, 1 << 32):
    vals += [big - 1, big, big + 1, -big - 1, -big, -big + 1]
  if lo == 0:
    vals += [(1 << 32) - 1, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1]
  seen, out = set(), []
  for v in vals:
    if lo <= v <= hi and v not in seen:
      seen.add(v)
      out.append(v)
  return np.array(out, dtype=dtype)


def uniform_ids(n, dtype, *key):
  """n ids drawn over the whole range of the type."""
  info = np.iinfo(dtype)
  return _rng(*key).integers(info.min, info.max, size=int(n), dtype=dtype, endpoint=True)


def ids_with_shards(s, P, dtype, *key):
  """Ids v = q * P + s[i] whose floor-mod by P is s[i], q drawn over everything that fits the type."""
  s = np.asarray(s, np.int64)
  info = np.iinfo(dtype)
  lo, hi, P = int(info.min), int(info.max), int(P)
  q_lo, q_hi = -((-lo) // P), (hi - (P - 1)) // P             # q_lo * P >= lo, q_hi * P + P - 1 <= hi
  wide = np.uint64 if lo == 0 else np.int64
  q = _rng(*key).integers(q_lo, q_hi, size=s.size, dtype=wide, endpoint=True)
  return (q * wide(P) + s.astype(wide)).astype(dtype)


def pattern_shards(n, P, seed=0):
  """name -> the shard of every position, for the patterns whose name states one."""
  n, P = int(n), int(P)
  pos = np.arange(n, dtype=np.int64)
  pats = {
    'shard0': np.zeros(n, np.int64),
    'shard_last': np.full(n, P - 1, np.int64),
    'alternating': np.where(pos % 2 == 0, P - 1, 0).astype(np.int64),     # the last and the first shard
    'descending': (P - 1 - (pos * P) // max(n, 1)).astype(np.int64),      # every shard, last first
    'position': pos % P,
  }
  if n <= P:
    pats['distinct'] = _rng(seed, n, P, 77).permutation(P)[:n].astype(np.int64)
  return pats


def patterns(n, P, dtype, seed=0):
  """name -> n ids: uniform over the range; one shard only (the first, the last); two alternating shards;
  shards descending (the worst case for stability: every id moves in front of all before it that differ);
  shard = position mod P; one distinct shard per id (only where n <= P); the edge ids tiled to n."""
  out = {'uniform': uniform_ids(n, dtype, seed, n, P, 1)}
  for k, (name, s) in enumerate(sorted(pattern_shards(n, P, seed).items())):
    out[name] = ids_with_shards(s, P, dtype, seed, n, P, 10 + k)
  out['edges'] = np.resize(edge_ids(dtype, P), int(n))
  return out


# ---- many columns ------------------------------------------------------------------------------------------
def uniform_tiles_of(n_cols):
  """Tiles per column of column_sets('uniform')."""
  return 1 + n_cols % 3


def column_sets(kind, seed=0):
  """n_cols -> the lengths of that many columns, for 64, 65, 127, 128, 129 and 257 columns (one launch group
  holds 128).  'uniform': every column has the same number of 1024-id tiles (uniform_tiles_of: one to three) but
  not the same length (three tiles: 2049 to 3072 ids).  'ragged': 0 to 3 tiles, with an empty column first, last and at 127 and 128."""
  assert kind in ('uniform', 'ragged'), kind
  sets = {}
  for n_cols in COLUMN_COUNTS:
    rng = _rng(seed, n_cols, kind == 'uniform')
    if kind == 'uniform':
      t = uniform_tiles_of(n_cols)
      lens = rng.integers((t - 1) * TILE + 1, t * TILE, size=n_cols, endpoint=True)
      lens[0], lens[-1] = (t - 1) * TILE + 1, t * TILE       # both ends of the range occur
    else:
      lens = rng.integers(0, 3 * TILE, size=n_cols, endpoint=True)
      for k in (0, 127, 128, n_cols - 1):
        if k < n_cols:
          lens[k] = 0
      lens[1], lens[2] = 3 * TILE, 1
    sets[n_cols] = [int(x) for x in lens]
  return sets
