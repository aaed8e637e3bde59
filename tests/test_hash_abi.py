"""Hash-keyed tables at the C ABI and in Python's argument handling, without a GPU: the entry exists beside
unchanged structs and version, every refused argument is refused before any device work with the reason
named, and the numpy restatement the GPU tests compare with (tests/support/hash_ref.py) is checked against
the C oracle's probe and against hand-computed initial values built from the golden murmur3 hashes."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
import oracle
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import hashtable as _ht
from tests.support import hash_ref as ref

FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
FAKE2 = 0x7f0000101000
FAKE3 = 0x7f0000201000
FAKE4 = 0x7f0000301000


def test_symbol_version_and_struct_layouts():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_hash_insert_n')
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  assert hb.__version__ == '0.2.0'
  assert C.sizeof(_lib.LookupColumn) == 128
  assert C.sizeof(_lib.LookupGradColumn) == 160
  assert C.sizeof(_lib.Sequence) == 32
  # hbk_hash_column_t: pointer, int64, int32 (+4), pointer, int64, two pointers, pointer, three 4-byte
  # fields (+4), int64
  assert C.sizeof(_lib.HashColumn) == 88
  assert _lib.HashColumn.keys.offset == 24 and _lib.HashColumn.table.offset == 56
  assert _lib.HashColumn.init_scale.offset == 72 and _lib.HashColumn.seed.offset == 80
  assert hb.embedding.HashTable is _ht.HashTable and hb.embedding.HashGroupLookup is _ht.HashGroupLookup
  assert hb.embedding.hash_translate is _ht.hash_translate


def test_header_declares_the_struct_as_mirrored():
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'hbk.h')).read()
  end = text.index('} hbk_hash_column_t;')
  body = text[text.rindex('typedef struct {', 0, end):end]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  assert re.findall(r'(\w+);', body) == [n for n, _ in _lib.HashColumn._fields_]


def _col(**kw):
  col = _lib.HashColumn()
  col.keys_cache, col.slab_count, col.slab_size = FAKE, 8, 16
  col.keys, col.n_keys, col.slots, col.counts = FAKE2, 100, FAKE3, FAKE4
  col.table, col.dim, col.table_pitch, col.init_scale, col.seed = FAKE4 + 4096, 16, 0, 1e-3, 0
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _refused(cols, *words):
  lib = _lib.lib()
  arr = (_lib.HashColumn * len(cols))(*cols)
  for insert in (1, 0):
    rc = lib.hbk_hash_insert_n(len(cols), arr, insert, None)
    msg = lib.hbk_last_error().decode()
    assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
    for w in ('hash_insert_n',) + words:
      assert w in msg, msg


@pytest.mark.parametrize('bad', [0, -1, 65, 128])
def test_refuses_slab_size_outside_1_to_64(bad):
  _refused([_col(), _col(slab_size=bad)], 'column 1', 'slab_size')


@pytest.mark.parametrize('bad', [0, -5])
def test_refuses_slab_count_below_one(bad):
  _refused([_col(slab_count=bad)], 'column 0', 'slab_count')


@pytest.mark.parametrize('field', ['keys_cache', 'keys', 'slots'])
def test_refuses_null_buffers_with_keys(field):
  _refused([_col(), _col(), _col(**{field: None})], 'column 2', 'NULL')


@pytest.mark.parametrize('bad', [0, -16])
def test_refuses_dim_below_one_with_a_table(bad):
  _refused([_col(dim=bad)], 'column 0', 'dim')


def test_refuses_a_pitch_below_dim():
  _refused([_col(dim=16, table_pitch=15)], 'column 0', 'table_pitch')


@pytest.mark.parametrize('bad', [-1e-3, float('nan'), float('inf'), -float('inf')])
def test_refuses_bad_init_scale(bad):
  _refused([_col(init_scale=bad)], 'column 0', 'init_scale')


def test_refuses_bad_counts_of_things():
  lib = _lib.lib()
  assert lib.hbk_hash_insert_n(-1, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode()
  arr = (_lib.HashColumn * 1)(_col())
  assert lib.hbk_hash_insert_n(1, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  _refused([_col(n_keys=-1)], 'n_keys')
  _refused([_col(n_keys=1 << 31)], 'n_keys')
  del arr


def test_nothing_to_do_is_ok():
  lib = _lib.lib()
  assert lib.hbk_hash_insert_n(0, None, 1, None) == _lib.OK
  # no keys: NULL buffers are fine, nothing is launched; dim is not looked at without a table
  arr = (_lib.HashColumn * 2)(_col(n_keys=0, keys=None, slots=None, keys_cache=None),
                              _col(n_keys=0, table=None, dim=0))
  assert lib.hbk_hash_insert_n(2, arr, 1, None) == _lib.OK
  assert lib.hbk_hash_insert_n(2, arr, 0, None) == _lib.OK


# ---- Python argument handling ---------------------------------------------------------------------------
def test_hashtable_geometry_and_refusals():
  assert hb.embedding.HashTable(100, 8, 'cpu').slab_size == 8        # the measured best (profiles/hash_insert.txt)
  t = hb.embedding.HashTable(100, 8, 'cpu', slab_size=16)
  assert (t.slab_count, t.capacity, t.slab_size, t.dim) == (6, 96, 16, 8)     # rounded down to whole slabs
  assert t.keys.dtype == torch.int64 and t.keys.shape == (96,) and bool((t.keys == -2 ** 63).all())
  assert t.table.dtype == torch.float32 and t.table.shape == (96, 8) and not t.table.any()
  assert t.counts.dtype == torch.int32 and t.counts.tolist() == [0, 0]
  assert sorted(t.variables('user')) == ['user/embedding_weights', 'user/keys']
  assert t.variables('user')['user/keys'] is t.keys and t.variables('user')['user/embedding_weights'] is t.table
  for kw in (dict(capacity=15), dict(capacity=0), dict(slab_size=0), dict(slab_size=65), dict(dim=0),
             dict(init_scale=-1.0), dict(init_scale=float('nan')), dict(init_scale=float('inf')),
             dict(init_scale=1e39)):
    args = dict(capacity=64, dim=8, device='cpu', slab_size=16)
    args.update(kw)
    with pytest.raises(_lib.InvalidArgumentError):
      hb.embedding.HashTable(**args)


def test_python_refuses_ids_that_are_not_int64_device_vectors():
  t = hb.embedding.HashTable(64, 4, 'cpu')
  with pytest.raises(_lib.InvalidArgumentError, match='int64'):
    hb.embedding.hash_translate([t], [torch.zeros(4, dtype=torch.int32)])
  with pytest.raises(_lib.InvalidArgumentError, match='int64'):
    hb.embedding.hash_translate([t], [torch.zeros((2, 2), dtype=torch.int64)])
  with pytest.raises(_lib.InvalidArgumentError, match='int64'):
    t.find([1, 2, 3])
  with pytest.raises(_lib.HbkError, match='HBM'):                     # a host tensor: there is no CPU path
    t.lookup_or_insert(torch.zeros(4, dtype=torch.int64))
  with pytest.raises(_lib.InvalidArgumentError, match='expected 1 id tensors'):
    hb.embedding.hash_translate([t], [])
  with pytest.raises(_lib.InvalidArgumentError, match='HashTable'):
    hb.embedding.hash_translate([t.table], [torch.zeros(4, dtype=torch.int64)])


def test_python_refuses_tables_of_different_devices():
  a = hb.embedding.HashTable(64, 4, 'cpu')
  b = hb.embedding.HashTable(64, 4, 'meta')
  with pytest.raises(_lib.InvalidArgumentError, match='one device'):
    hb.embedding.HashGroupLookup([a, b])
  with pytest.raises(_lib.InvalidArgumentError, match='one device'):
    hb.embedding.hash_translate([a, b], [torch.zeros(1, dtype=torch.int64)] * 2)


# ---- the restatement -----------------------------------------------------------------------------------
def _golden():
  root = os.path.dirname(os.path.abspath(__file__))
  with open(os.path.join(root, 'golden', 'murmur3.json')) as f:
    return json.load(f)


def test_restatement_hash_is_the_golden_hash():
  g = _golden()
  assert [ref.murmur3(k) for k in g['keys']] == g['hash32']
  assert ref.murmur3_np(np.array(g['keys'], np.int64)).tolist() == g['hash32']
  rng = np.random.RandomState(3)
  keys = rng.randint(-2 ** 63, 2 ** 63 - 1, size=500, dtype=np.int64)
  np.testing.assert_array_equal(ref.murmur3_np(keys), oracle.murmur3_hash32(keys))


@pytest.mark.parametrize('slab_size,slab_count', [(5, 3), (16, 257), (64, 1), (1, 7)])
def test_oracle_probe_finds_every_filled_key_where_the_fill_put_it(slab_size, slab_count):
  rng = np.random.RandomState(slab_size * 1000 + slab_count)
  cap = slab_size * slab_count
  keys = rng.randint(-2 ** 63, 2 ** 63 - 1, size=cap + 9, dtype=np.int64)
  keys[:3] = [ref.EMPTY + 1, -1, 0]
  keys = np.concatenate([keys, keys[:10], [ref.EMPTY]])               # duplicates, and the key never stored
  cache = np.full(cap, ref.EMPTY, np.int64)
  slots = ref.fill(cache, slab_size, keys)
  assert int((cache != ref.EMPTY).sum()) == cap                       # cap + 9 distinct keys: it filled up
  assert slots[-1] == -1 and ref.EMPTY not in keys[:-1]
  placed = slots >= 0
  np.testing.assert_array_equal(cache[slots[placed]], keys[placed])
  assert len(set(keys[~placed].tolist()) - {ref.EMPTY}) == 9         # exactly the 9 that cannot fit
  assert not set(keys[~placed].tolist()) & set(keys[placed].tolist())
  np.testing.assert_array_equal(oracle.cache_probe(cache, slab_size, keys[:-1]), slots[:-1])
  # half full: nothing fails; keys never inserted are misses
  cache = np.full(cap, ref.EMPTY, np.int64)
  half = keys[:max(cap // 2, 1)]
  slots = ref.fill(cache, slab_size, half)
  assert (slots >= 0).all() and int((cache != ref.EMPTY).sum()) == half.size
  np.testing.assert_array_equal(oracle.cache_probe(cache, slab_size, half), slots)
  rest = keys[half.size:cap + 9]
  assert (oracle.cache_probe(cache, slab_size, rest) == -1).all()
  assert sorted(k for s in ref.slab_sets(cache, slab_size) for k in s) == sorted(half.tolist())


def test_init_values_built_from_the_golden_hashes():
  """init(key, j, seed) hashes key ^ ((seed + j + 1) * 0x9E3779B97F4A7C15): with key = golden ^ that word the
  hash is the golden one, and the value follows by hand: ((h >> 8) / 2^23 - 1) * scale, one fp32 rounding."""
  g = _golden()
  triples = [(0, 0, 0), (1, 3, 7), (4, 19, 12345), (5, 127, 2 ** 40 + 1), (8, 1, -3)]
  for n, j, seed in triples:
    word = ((seed + j + 1) & (2 ** 64 - 1)) * ref.GOLDEN_RATIO & (2 ** 64 - 1)
    key = (g['keys'][n] & (2 ** 64 - 1)) ^ word
    key = key - 2 ** 64 if key >> 63 else key
    assert ref.init_mix(key, j, seed) == g['keys'][n]
    h = g['hash32'][n]
    unit = (h >> 8) / 2.0 ** 23 - 1.0                                  # exact in float64, and in fp32
    assert -1.0 <= unit < 1.0 and float(np.float32(unit)) == unit
    for scale in (1e-3, 1.0, 0.25):
      want = np.float32(unit) * np.float32(scale)
      assert ref.init_value(key, j, seed, scale) == want
      row = ref.init_row(key, j + 1, seed, scale)
      assert row.dtype == np.float32 and row[j] == want
      np.testing.assert_array_equal(ref.init_rows([key, key + 1], j + 1, seed, scale)[0], row)
  # hand-computed: key 0 at j = 0, seed 0 hashes the word 0x9E3779B97F4A7C15 itself
  assert ref.init_mix(0, 0, 0) == 0x9E3779B97F4A7C15 - 2 ** 64
  assert not ref.init_row(5, 4, 0, 0.0).any() and not np.signbit(ref.init_row(5, 4, 0, 0.0)).any()


def test_init_rows_vectorised_equals_scalar():
  rng = np.random.RandomState(11)
  keys = rng.randint(-2 ** 63, 2 ** 63 - 1, size=40, dtype=np.int64)
  for dim, seed, scale in ((1, 0, 1e-3), (20, 9, 0.5), (16, -1, 1.0)):
    want = np.stack([ref.init_row(k, dim, seed, scale) for k in keys.tolist()])
    np.testing.assert_array_equal(ref.init_rows(keys, dim, seed, scale), want)
    assert (np.abs(want) <= np.float32(scale)).all()
