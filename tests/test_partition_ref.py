"""tests/support/partition_ref.py held to everything that states the partition independently of it, without
a GPU: the C oracle (oracle/hbk_oracle.c, the reference's CPU functor restated), the reference's own cases
(tests/golden/partition.json) and the library's host entries (csrc/partition_host.cpp); the checker
assert_partition held to two planted errors; and the case lists held to what their names state.

One place where the oracle is not asked in its own type: the reference's functor computes
`(v % d + d) % d` in the type of the ids, and for int32 ids `v % d + d` leaves int32 once d = P * M exceeds
2^30 (two DUAL_EDGES pairs).  That is undefined in C, so there the int64 functor is asked with the same ids
widened -- the value the int32 one states wherever it is defined.
"""
import json
import os

import numpy as np
import pytest

import oracle
from tests.support import partition_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPE_NAMES = tuple(ref.DTYPES)
P_SMALL = tuple(P for P in ref.P_EDGES if P <= 129)
DUAL_LEN = 3000
SHORT = 300          # patterns again at a length below one tile (and 'distinct' wherever P allows)


def _oracle(ids, P, M=1, stage=0):
  if stage == 0:
    return oracle.partition_by_modulo(ids, P)
  if ids.dtype == np.int32 and P * M > (1 << 30):
    out, sizes, idx = oracle.partition_by_dual_modulo(ids.astype(np.int64), P, M, stage)
    assert np.array_equal(out.astype(np.int32).astype(np.int64), out)
    return out.astype(np.int32), sizes, idx
  return oracle.partition_by_dual_modulo(ids, P, M, stage)


def _modulo_columns(dtype, P):
  """(name, ids) of every patterns / edge_ids column the CPU checks use for one (dtype, P)."""
  cols = [('edge_ids', ref.edge_ids(dtype, P))]
  for n in (ref.PATTERN_LEN, SHORT, min(P, 64), 0):
    cols += [('%s[%d]' % (name, n), x) for name, x in ref.patterns(n, P, dtype, seed=3).items()]
  return cols


def _dual_columns(dtype, P, M):
  return [('edge_ids', np.resize(ref.edge_ids(dtype, P, M), DUAL_LEN)),
          ('uniform', ref.uniform_ids(DUAL_LEN, dtype, 5, P, M))]


# ---- the restatement against the oracle -------------------------------------------------------------------
@pytest.mark.parametrize('dtype_name', DTYPE_NAMES)
def test_restatement_equals_the_oracle_modulo(dtype_name):
  dtype = ref.DTYPES[dtype_name]
  for P in P_SMALL:
    for name, ids in _modulo_columns(dtype, P):
      ref.assert_partition(ref.partition(ids, P), _oracle(ids, P), '%s %s' % (dtype_name, name), P)


@pytest.mark.parametrize('dtype_name', DTYPE_NAMES)
@pytest.mark.parametrize('stage', [1, 2])
def test_restatement_equals_the_oracle_dual_modulo(dtype_name, stage):
  dtype = ref.DTYPES[dtype_name]
  for P, M in ref.DUAL_EDGES:
    assert P * M < (1 << 31)
    for name, ids in _dual_columns(dtype, P, M):
      ref.assert_partition(ref.partition(ids, P, M, stage), _oracle(ids, P, M, stage),
                           '%s %s' % (dtype_name, name), P, M, stage)


def test_restatement_equals_the_reference_cases():
  g = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'partition.json')))
  assert g['modulo'] and g['dual'] and g['property']
  for k in g['modulo']:
    want = (np.array(k['output'], np.int64), np.array(k['sizes'], np.int32), np.array(k['indices'], np.int32))
    ref.assert_partition(ref.partition(np.array(k['input'], np.int64), k['num_partitions']), want,
                         'golden modulo', k['num_partitions'])
  for k in g['dual']:
    want = (np.array(k['output'], np.int64), np.array(k['sizes'], np.int32), np.array(k['indices'], np.int32))
    got = ref.partition(np.array(k['input'], np.int64), k['num_partitions'], k['modulus'], k['stage'])
    ref.assert_partition(got, want, 'golden dual', k['num_partitions'], k['modulus'], k['stage'])
  for k in g['property']:                               # partition_test.py:40-65: x == take(y, idx)
    np.random.seed(k['seed'])
    for _ in range(k['columns']):
      x = np.random.randint(low=k['low'], high=k['high'], size=k['size'], dtype=k['dtype'])
      y, sizes, idx = ref.partition(x, k['num_partitions'])
      assert len(sizes) == k['num_partitions'] and int(sizes.sum()) == x.size
      np.testing.assert_array_equal(np.take(y, idx), x)


def test_shard_of_values_beyond_int64_by_python_integers():
  # the unsigned path of shard() against Python's own integers, which cannot wrap
  for P, M in ref.DUAL_EDGES + ((3, 1), (1000, 1), (16384, 1)):
    for name in ('uint32', 'uint64', 'int32', 'int64'):
      ids = ref.edge_ids(ref.DTYPES[name], P, M)
      for stage in (0, 1, 2):
        pre = [int(v) % (P * M) for v in ids]
        want = [int(v) % P for v in ids] if stage == 0 else [p % P for p in pre] if stage == 1 else \
            [p // M for p in pre]
        assert ref.shard(ids, P, M, stage).tolist() == want, (name, P, M, stage)


# ---- the library's host entries ---------------------------------------------------------------------------
def _host_partition(cols, code, P, M=1, stage=0):
  from hybridbackend_amd import _lib  # pylint: disable=import-outside-toplevel
  try:
    lib = _lib.lib()
  except (ImportError, OSError) as e:
    pytest.skip('the library cannot be loaded on this machine: %s' % e)
  outs = [np.full(c.size, 0x5a, c.dtype) for c in cols]
  sizes = [np.full(P, -7, np.int32) for _ in cols]
  idx = [np.full(c.size, -7, np.int32) for c in cols]
  ptrs = lambda arrs: _lib.ptr_array([a.ctypes.data for a in arrs])   # noqa: E731
  lens = _lib.i64_array([c.size for c in cols])
  if stage == 0:
    rc = lib.hbk_partition_by_modulo_host(len(cols), code, P, ptrs(cols), lens, ptrs(outs), ptrs(sizes),
                                          ptrs(idx))
  else:
    rc = lib.hbk_partition_by_dual_modulo_host(len(cols), code, P, M, stage, ptrs(cols), lens, ptrs(outs),
                                               ptrs(sizes), ptrs(idx))
  _lib.check(rc)
  return list(zip(outs, sizes, idx))


def _code(dtype_name):
  from hybridbackend_amd import _lib  # pylint: disable=import-outside-toplevel
  return {'int32': _lib.INT32, 'int64': _lib.INT64, 'uint32': _lib.UINT32, 'uint64': _lib.UINT64}[dtype_name]


@pytest.mark.parametrize('dtype_name', DTYPE_NAMES)
def test_host_entries_equal_the_restatement_modulo(dtype_name):
  dtype = ref.DTYPES[dtype_name]
  for P in ref.P_EDGES:                                 # the host entries take every P the device takes
    named = _modulo_columns(dtype, P) if P <= 129 else \
        [('edge_ids', ref.edge_ids(dtype, P))] + list(ref.patterns(ref.PATTERN_LEN, P, dtype, seed=3).items())
    cols = [np.ascontiguousarray(x) for _, x in named]
    for (name, x), got in zip(named, _host_partition(cols, _code(dtype_name), P)):
      ref.assert_partition(got, ref.partition(x, P), 'host %s %s' % (dtype_name, name), P)


@pytest.mark.parametrize('dtype_name', DTYPE_NAMES)
@pytest.mark.parametrize('stage', [1, 2])
def test_host_entries_equal_the_restatement_dual_modulo(dtype_name, stage):
  dtype = ref.DTYPES[dtype_name]
  for P, M in ref.DUAL_EDGES:
    named = _dual_columns(dtype, P, M)
    cols = [np.ascontiguousarray(x) for _, x in named]
    for (name, x), got in zip(named, _host_partition(cols, _code(dtype_name), P, M, stage)):
      ref.assert_partition(got, ref.partition(x, P, M, stage), 'host %s %s' % (dtype_name, name), P, M, stage)


# ---- the checker ------------------------------------------------------------------------------------------
def _checker_case():
  P = 5
  ids = ref.patterns(3000, P, np.int64, seed=9)['uniform']
  want = ref.partition(ids, P)
  starts = np.concatenate([[0], np.cumsum(want[1])])
  assert want[1].min() > 2
  return P, ids, want, starts


def test_checker_names_a_loss_of_stability():
  P, _, want, starts = _checker_case()
  out = want[0].copy()
  a = int(starts[2]) + 1                                # two ids of shard 2 change places
  assert out[a] != out[a + 1]
  out[a], out[a + 1] = out[a + 1], out[a]
  with pytest.raises(AssertionError) as e:
    ref.assert_partition((out, want[1], want[2]), want, 'planted', P, column=4)
  msg = str(e.value)
  assert 'stability lost' in msg and 'wrong base' not in msg, msg
  assert 'column 4' in msg and 'P = 5' in msg, msg
  assert 'position %d (tile %d, chunk %d' % (a, a // 1024, a // 64) in msg, msg


def test_checker_names_a_wrong_base():
  P, _, want, starts = _checker_case()
  out = want[0].copy()
  lo, hi = int(starts[2]), int(starts[3])               # the run of shard 2 written one place too far on: it
  out[lo:hi + 1] = np.roll(out[lo:hi + 1], 1)           # rotates over the first id of shard 3
  with pytest.raises(AssertionError) as e:
    ref.assert_partition((out, want[1], want[2]), want, 'planted', P, column=0)
  msg = str(e.value)
  assert 'wrong base' in msg and 'stability lost' not in msg, msg
  assert 'position %d (tile %d, chunk %d' % (lo, lo // 1024, lo // 64) in msg, msg


def test_checker_passes_what_is_equal_and_sees_indices_and_sizes():
  P, _, want, _ = _checker_case()
  ref.assert_partition(tuple(x.copy() for x in want), want, 'equal', P)
  idx = want[2].copy()
  idx[7] ^= 1
  with pytest.raises(AssertionError, match='indices differ'):
    ref.assert_partition((want[0], want[1], idx), want, 'planted', P)
  sizes = want[1].copy()
  sizes[1] += 1
  with pytest.raises(AssertionError, match='sizes differ at shard 1'):
    ref.assert_partition((want[0], sizes, want[2]), want, 'planted', P)


# ---- the lists --------------------------------------------------------------------------------------------
def test_constants_are_the_boundaries_of_the_kernel_paths():
  assert set(ref.P_EDGES) >= {1, 8, 9, 32, 33, 64, 65, 16384} and max(ref.P_EDGES) == 16384
  assert set(ref.LEN_EDGES) >= {0, 1, ref.CHUNK, ref.TILE, ref.TILE + 1, 4 * ref.TILE + 1}
  assert all(P * M < (1 << 31) for P, M in ref.DUAL_EDGES)
  assert max(P * M for P, M in ref.DUAL_EDGES) == (1 << 31) - 2


@pytest.mark.parametrize('dtype_name', DTYPE_NAMES)
def test_edge_ids_hold_what_they_claim(dtype_name):
  dtype = ref.DTYPES[dtype_name]
  lo, hi = int(np.iinfo(dtype).min), int(np.iinfo(dtype).max)
  fits = lambda xs: {x for x in xs if lo <= x <= hi}   # noqa: E731
  around = lambda m: fits([m - 1, m, m + 1])           # noqa: E731
  for P, M in [(P, 1) for P in ref.P_EDGES] + list(ref.DUAL_EDGES):
    d = P * M
    ids = ref.edge_ids(dtype, P, M)
    vals = set(int(v) for v in ids)
    assert ids.dtype == dtype and len(vals) == ids.size                      # distinct
    assert fits([lo, hi, 0, 1, -1, 2, -2]) <= vals
    for k in (0, 1, -1):
      assert around(k * d) <= vals, (P, M, k)
    for big in (1 << 31, 1 << 32, 1 << 62):                                  # the multiple next to it
      assert around(big // d * d) | around(-(big // d * d)) <= vals, (P, M, big)
      if lo <= big * d - 1 and big * d + 1 <= hi:                            # d times it
        assert around(big * d) <= vals, (P, M, big)
      assert around(big) | around(-big) <= vals or big == 1 << 62
    top, low = hi // d * d, -((-lo) // d * d)                                # the last multiples that fit
    assert around(top) | around(low) <= vals and top + d > hi and low - d < lo
    if lo == 0:
      assert fits([(1 << 32) - 1, (1 << 32) + 1, 1 << 63, (1 << 64) - 1]) <= vals
    # either side of a multiple: the last shard, then the first
    assert ref.shard(np.array([top - 1, top], dtype), P * M).tolist() == ([d - 1, 0] if d > 1 else [0, 0])


@pytest.mark.parametrize('dtype_name', DTYPE_NAMES)
def test_patterns_hold_what_their_names_state(dtype_name):
  dtype = ref.DTYPES[dtype_name]
  info = np.iinfo(dtype)
  # (seeds 1, 5 and 6 at 5000 ids and at P ids: what tests/test_gpu_partition_edges.py draws)
  for P in ref.P_EDGES:
    for n, seed in [(ref.PATTERN_LEN, s) for s in (1, 3, 5, 6)] + [(P, 6), (SHORT, 3), (min(P, 64), 3), (0, 3)]:
      pats = ref.patterns(n, P, dtype, seed=seed)
      assert ('distinct' in pats) == (n <= P)
      assert set(pats) - {'distinct'} == {'uniform', 'shard0', 'shard_last', 'alternating', 'descending',
                                          'position', 'edges'}
      for name, x in pats.items():
        assert x.dtype == dtype and x.shape == (n,), (name, P, n)
      s = {name: ref.shard(x, P) for name, x in pats.items()}
      pos = np.arange(n)
      assert (s['shard0'] == 0).all() and (s['shard_last'] == P - 1).all()
      assert (s['alternating'][0::2] == P - 1).all() and (s['alternating'][1::2] == 0).all()
      assert (s['descending'][:-1] >= s['descending'][1:]).all()
      assert (s['position'] == pos % P).all()
      if n >= P:
        assert np.unique(s['descending']).size == P     # every shard occurs
      if n:
        assert s['descending'][0] == P - 1
      if 'distinct' in pats:
        assert np.unique(s['distinct']).size == n
      if n == ref.PATTERN_LEN:
        # over the full range: both halves of the type, and the ids of a one-shard column are not one value
        assert int(pats['uniform'].max()) > info.max // 2 and int(pats['uniform'].min()) < info.min // 2 + \
            info.max // 4
        assert np.unique(pats['shard0']).size > 1 or P > info.max // 2
        if P <= 129:
          assert np.unique(s['uniform']).size == P
        assert set(ref.edge_ids(dtype, P).tolist()) == set(pats['edges'].tolist())


def test_column_sets_hold_what_they_claim():
  for kind in ('uniform', 'ragged'):
    sets = ref.column_sets(kind, seed=1)
    assert tuple(sets) == ref.COLUMN_COUNTS == (64, 65, 127, 128, 129, 257)
    for n_cols, lens in sets.items():
      assert len(lens) == n_cols
      tiles = [-(-n // ref.TILE) for n in lens]
      if kind == 'uniform':
        assert set(tiles) == {ref.uniform_tiles_of(n_cols)} and len(set(lens)) > 1
        assert min(lens) % ref.TILE == 1 and max(lens) % ref.TILE == 0
      else:
        assert set(tiles) == {0, 1, 2, 3}
        for k in (0, 127, 128, n_cols - 1):
          assert k >= n_cols or lens[k] == 0
  assert {ref.uniform_tiles_of(n) for n in ref.COLUMN_COUNTS} == {1, 2, 3}
