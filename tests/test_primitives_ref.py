"""The numpy / Python restatements of the id and wire primitives (tests/support/primitives_ref.py) against
the C oracle, on every input tests/test_gpu_primitive_edges.py feeds the kernels.  Two implementations
that share no code have to agree before the kernels are held to either.

Two rules of the cache probe are not spelled out where the kernel states its rule; the oracle (the
restated reference functor) decides them and the restatement follows:
  * a query equal to EMPTY_KEY is a hit, on the first EMPTY slot of its hashed slab (a match is looked
    for before EMPTY slots are);
  * a key stored behind an EMPTY slot of its own slab is found (the whole slab is compared, not the slots
    up to the first EMPTY one).
"""
import numpy as np
import pytest

import oracle
from tests.support import primitives_ref as ref


def test_numpy_casts_round_to_nearest_even():
  for x, bits in ref.cast_rounding_examples():
    got = ref.cast_f32_to_f16(np.array([x], np.float32)).view(np.uint16)[0]
    assert got == bits, (x, hex(got), hex(bits))


def test_cast_restatement_matches_oracle():
  x = ref.f32_rounding_edges()
  assert x.size == 6 * 31744 + 17
  ref.assert_same_bits(oracle.cast_f32_to_f16(x), ref.cast_f32_to_f16(x), 'f32 -> f16')
  h = ref.f16_all_bit_patterns()
  ref.assert_same_bits(oracle.cast_f16_to_f32(h), ref.cast_f16_to_f32(h), 'f16 -> f32')
  for k, (n, _, _) in enumerate(ref.cast_layout_product()):
    v = ref.cast_layout_values(k, n)
    ref.assert_same_bits(oracle.cast_f32_to_f16(v), ref.cast_f32_to_f16(v))
    back = ref.cast_f32_to_f16(v)
    ref.assert_same_bits(oracle.cast_f16_to_f32(back), ref.cast_f16_to_f32(back))


@pytest.mark.parametrize('dtype', [np.int64, np.int32])
def test_floormod_restatement_matches_oracle(dtype):
  cols = ref.floormod_columns(dtype)
  assert len(cols) == 130 and [c for c, (x, _) in enumerate(cols) if x.size == 0] == [0, 127, 128]
  for x, d in cols:
    want = ref.floormod(x, d)
    assert want.dtype == dtype and ((want >= 0) & (want < d)).all()
    np.testing.assert_array_equal(oracle.floormod(x, d), want)


def _check_unique(x):
  u, idx = ref.unique_first_occurrence(x)
  ou, oidx = oracle.unique(x)
  np.testing.assert_array_equal(u, ou)
  np.testing.assert_array_equal(idx, oidx)
  assert idx.dtype == np.int32


def test_unique_restatement_matches_oracle():
  for _, x in ref.unique_boundary_columns():
    _check_unique(x)
  for n_cols in (96, 97, 200):
    cols = ref.unique_many_columns(n_cols, n_cols)
    assert len(cols) == n_cols and all(cols[c].size == 0 for c in (95, n_cols - 1))
    for x in cols:
      _check_unique(x)
  assert all(x.size == 0 for x in ref.unique_many_columns(97, 1, all_empty=True))
  for log2p in ref.UNIQUE_BUCKETS_LOG2:
    for x in ref.unique_bucket_option_columns(log2p):
      _check_unique(x)
  for n_keys in ref.UNIQUE_SKEW_KEYS:
    _check_unique(ref.unique_skew_column(n_keys))


def test_skewed_keys_share_one_bucket():
  # mix64 itself: two values worked out by hand from the constants, then the property the inputs need
  assert int(ref.mix64(np.array([0], np.int64))[0]) == 0
  k = 1
  for mul in (0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53):
    k ^= k >> 33
    k = (k * mul) & ((1 << 64) - 1)
  k ^= k >> 33
  assert int(ref.mix64(np.array([1], np.int64))[0]) == k
  for n_keys in ref.UNIQUE_SKEW_KEYS:
    keys = ref.keys_of_one_bucket(n_keys, 7)
    assert np.unique(keys).size == n_keys
    assert np.unique(ref.mix64(keys) >> np.uint64(51)).size == 1
    x = ref.unique_skew_column(n_keys)
    top = ref.mix64(x) >> np.uint64(51)
    vals, counts = np.unique(top, return_counts=True)
    assert counts.max() == 2 * n_keys                     # the bucket the column was built around
    # ... holds exactly n_keys distinct keys at the column's default bucket count (512 ids per bucket)
    # and at every larger one: the other ids differ from them in the top bit of the mix
    assert 512 << 4 >= x.size > 512 << 3
    in_bucket = (ref.mix64(x) >> np.uint64(60)) == (vals[counts.argmax()] >> np.uint64(9))
    assert np.unique(x[in_bucket]).size == n_keys and in_bucket.sum() == 2 * n_keys


def test_murmur3_restatement_matches_oracle():
  rng = np.random.RandomState(2)
  keys = np.concatenate([rng.randint(-2**63, 2**63 - 1, size=20000, dtype=np.int64),
                         np.array([0, -1, 1, ref.EMPTY_KEY, ref.EMPTY_KEY + 1, ref.INT64_MAX], np.int64)])
  np.testing.assert_array_equal(ref.murmur3_hash32(keys), oracle.murmur3_hash32(keys))


def test_probe_rules_decided_by_the_oracle():
  slab_size, slab_count = 4, 3
  # a query equal to EMPTY_KEY: the first EMPTY slot of its slab answers
  home = int(ref.home_slab(np.array([ref.EMPTY_KEY], np.int64), slab_count)[0])
  cache = np.full(slab_size * slab_count, ref.EMPTY_KEY, np.int64)
  cache[home * slab_size] = 11
  got = oracle.cache_probe(cache, slab_size, np.array([ref.EMPTY_KEY], np.int64))
  assert got.tolist() == [home * slab_size + 1]
  np.testing.assert_array_equal(ref.cache_probe(cache, slab_size, [ref.EMPTY_KEY]), got)
  cache[:] = np.arange(1, cache.size + 1)                 # no EMPTY slot at all: a miss
  got = oracle.cache_probe(cache, slab_size, np.array([ref.EMPTY_KEY], np.int64))
  assert got.tolist() == [-1]
  np.testing.assert_array_equal(ref.cache_probe(cache, slab_size, [ref.EMPTY_KEY]), got)
  # a key stored behind an EMPTY slot of its slab: found
  key = 77
  home = int(ref.home_slab(np.array([key], np.int64), slab_count)[0])
  cache = np.full(slab_size * slab_count, ref.EMPTY_KEY, np.int64)
  cache[home * slab_size + 2] = key
  got = oracle.cache_probe(cache, slab_size, np.array([key], np.int64))
  assert got.tolist() == [home * slab_size + 2]
  np.testing.assert_array_equal(ref.cache_probe(cache, slab_size, [key]), got)


@pytest.mark.parametrize('slab_size', ref.PROBE_SLAB_SIZES)
def test_cache_probe_restatement_matches_oracle(slab_size):
  names = set()
  for slab_count in ref.PROBE_SLAB_COUNTS:
    for name, cache, must in ref.probe_tables(slab_size, slab_count):
      names.add(name)
      keys = ref.probe_universe(cache, must, 5)
      assert keys.size == ref.PROBE_UNIVERSE
      want = ref.cache_probe(cache, slab_size, keys)
      np.testing.assert_array_equal(want, oracle.cache_probe(cache, slab_size, keys), err_msg=name)
      # what each table was built to show is in the queries
      if name == 'full':
        assert (cache != ref.EMPTY_KEY).all()
        assert (want[keys < -1] == -1).all()                       # absent keys: every slab probed, a miss
        assert (want[np.isin(keys, must)] >= 0).all() and (must.size > 0) == (slab_count > 1)
        if slab_count > 1:
          assert (want[np.isin(keys, must)] < slab_size).any()     # found in slab 0 after the wrap
      if name == 'behind_empty':
        found = want[keys == must[0]]
        assert (found >= 0).all() and (cache[:found[0]][-(slab_size - 1):] == ref.EMPTY_KEY).all()
        if must.size > 1:
          assert (want[keys == must[1]] == -1).all()               # stored past a slab with room: unreachable
      if name == 'twice_in_slab':
        found = want[keys == must[0]]
        assert (found % slab_size == 0).all() and cache[found[0] + slab_size - 1] == must[0]
      if name == 'empty':
        assert ((want >= 0) == (keys == ref.EMPTY_KEY)).all()
      lists = ref.cache_lists(want, keys)
      assert lists[4].tolist() == [int((want >= 0).sum()), int((want < 0).sum())]
      sel = ref.probe_selections(want, slab_size)
      k = ref.probe_keys_per_block(slab_size)
      assert {0, 1, 1023, 1024, 1025, 5000, k - 1, k, k + 1} <= {v.size for v in sel.values()}
  assert {'empty', 'half', 'full'} <= names
  if slab_size >= 2:
    assert {'behind_empty', 'twice_in_slab', 'twice_in_two_slabs'} <= names


def test_probe_keys_per_block():
  assert [ref.probe_keys_per_block(s) for s in ref.PROBE_SLAB_SIZES] == [2048, 1024, 512, 256, 256, 32, 32, 32]


@pytest.mark.parametrize('world', ref.ALLTOALLV_WORLDS)
def test_alltoallv_restatement_matches_oracle(world):
  sizes = ref.alltoallv_sizes(world, 4, 3)
  assert sizes.shape == (4, world, world) and sizes.min() >= 0 and sizes.max() <= 41
  assert sizes[1].sum() == 0 and sizes[[0, 3], world - 1].sum() == 0
  assert sizes[2].sum() == sizes[2, 0, 1] + sizes[2, 1, 0] and sizes[2, 0, 1] > 0 and sizes[2, 1, 0] > 0
  for c, common in enumerate(ref.ALLTOALLV_COMMON):
    for kind in ('f32', 'i64', 'i32'):
      vals = [ref.alltoallv_values(kind, int(sizes[c, r].sum()) * common, 100 * c + r)
              for r in range(world)]
      outs, out_sizes = ref.alltoallv(vals, sizes[c], common)
      want, want_sizes = oracle.alltoallv_sim([v.reshape(-1, common) for v in vals],
                                              sizes[c].astype(np.int32))
      for r in range(world):
        ref.assert_same_bits(outs[r], want[r].reshape(-1), kind)
        np.testing.assert_array_equal(out_sizes[r], want_sizes[r])
