"""The admission filter at the C ABI and in Python's argument handling, without a GPU: the two entries exist
beside unchanged structs and version, hbk_hash_admission_t mirrors the header, every refused argument is
refused before any device work with the reason named, and the sequential restatement the GPU tests compare with
(tests/support/hash_admission_ref.py) holds what a count-min sketch must: min_freq 1 is the plain fill, the
estimate is never below the true count, and one cell counts everything."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import hashtable as _ht
from tests.support import hash_admission_ref as aref
from tests.support import hash_expiry_ref as xref
from tests.support import hash_ref as ref

FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('hash_insert_admit_n', 'hash_insert_expiring_admit_n')


def fake(n):
  return FAKE + n * 0x100000


def _header():
  return open(os.path.join(ROOT, 'include', 'hbk.h')).read()


def _struct_fields(name):
  text = _header()
  end = text.index('} %s;' % name)
  body = text[text.rindex('typedef struct {', 0, end):end]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return re.findall(r'(\w+)(?:\[\w+\])?;', body)


def test_symbols_version_and_struct_layout():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_hash_insert_admit_n') and hasattr(lib, 'hbk_hash_insert_expiring_admit_n')
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  A = _lib.HashAdmission
  assert C.sizeof(A) == 40
  assert [A.sketch.offset, A.width.offset, A.depth.offset, A.min_freq.offset, A.seed.offset, A.filtered.offset] == \
      [0, 8, 16, 20, 24, 32]
  assert C.sizeof(_lib.HashColumn) == 88 and C.sizeof(_lib.HashExpiry) == 32
  assert _lib.HASH_MAX_SKETCH_DEPTH == 8
  assert hb.embedding.sketch_cells is _ht.sketch_cells


def test_header_declares_the_struct_as_mirrored_and_the_rule():
  assert _struct_fields('hbk_hash_admission_t') == [n for n, _ in _lib.HashAdmission._fields_]
  assert _struct_fields('hbk_hash_column_t') == [n for n, _ in _lib.HashColumn._fields_]
  assert _struct_fields('hbk_hash_expiry_t') == [n for n, _ in _lib.HashExpiry._fields_]
  text = _header()
  assert '#define HBK_HASH_MAX_SKETCH_DEPTH 8' in text
  for name in ENTRIES:
    assert re.search(r'\bint hbk_%s\(' % name, text), name
  for word in ('count-min sketch', '(seed + r + 1) * 0x9E3779B97F4A7C15', '% width', 'min_freq', 'filtered',
               'never decremented', 'early, never late', 'default-value row'):
    assert word in text, word


# ---- refusals --------------------------------------------------------------------------------------------
def _col(**kw):
  col = _lib.HashColumn()
  col.keys_cache, col.slab_count, col.slab_size = fake(0), 8, 16
  col.keys, col.n_keys, col.slots, col.counts = fake(1), 100, fake(2), fake(3)
  col.table, col.dim, col.table_pitch, col.init_scale, col.seed = fake(4), 16, 0, 1e-3, 0
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _exp(**kw):
  e = _lib.HashExpiry()
  e.last_seen, e.freq, e.step, e.stats = fake(5), fake(6), fake(7), fake(8)
  for k, v in kw.items():
    setattr(e, k, v)
  return e


def _adm(**kw):
  a = _lib.HashAdmission()
  a.sketch, a.width, a.depth, a.min_freq, a.seed, a.filtered = fake(9), 128, 4, 2, 0, fake(10)
  for k, v in kw.items():
    setattr(a, k, v)
  return a


def _call(name, cols, exps, adms, insert):
  lib = _lib.lib()
  arr = (_lib.HashColumn * len(cols))(*cols) if cols is not None else None
  ex = (_lib.HashExpiry * len(exps))(*exps) if exps is not None else None
  ad = (_lib.HashAdmission * len(adms))(*adms) if adms is not None else None
  n = len(cols) if cols is not None else 1
  if name == 'hash_insert_admit_n':
    rc = lib.hbk_hash_insert_admit_n(n, arr, ad, insert, None)
  else:
    rc = lib.hbk_hash_insert_expiring_admit_n(n, arr, ex, ad, insert, None)
  return rc, lib.hbk_last_error().decode()


def _refused(cols, exps, adms, *words):
  for name in ENTRIES:
    for insert in (1, 0):
      rc, msg = _call(name, cols, exps, adms, insert)
      assert rc == _lib.INVALID_ARGUMENT, (name, rc, msg)
      for w in (name,) + words:
        assert w in msg, msg


@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)),
  (dict(slab_count=0), ('slab_count',)),
  (dict(keys_cache=None), ('NULL',)), (dict(keys=None), ('NULL',)), (dict(slots=None), ('NULL',)),
  (dict(dim=0), ('dim',)), (dict(dim=16, table_pitch=15), ('table_pitch',)),
  (dict(init_scale=-1e-3), ('init_scale',)), (dict(init_scale=float('nan')), ('init_scale',)),
  (dict(init_scale=float('inf')), ('init_scale',)),
  (dict(n_keys=-1), ('n_keys',)), (dict(n_keys=1 << 31), ('n_keys',)),
  (dict(n_keys=1 << 30), ('n_keys', '2^30')),
])
def test_refuses_what_the_entries_without_a_filter_refuse_and_2_to_30_keys(kw, words):
  _refused([_col(), _col(**kw)], [_exp(), _exp()], [_adm(), _adm()], 'column 1', *words)


@pytest.mark.parametrize('kw,words', [
  (dict(sketch=None), ('NULL', 'sketch')),
  (dict(sketch=fake(9) + 2), ('sketch', 'aligned')),
  (dict(width=0), ('width',)), (dict(width=1 << 31), ('width',)), (dict(width=-5), ('width',)),
  (dict(depth=0), ('depth',)), (dict(depth=9), ('depth',)),
  (dict(min_freq=0), ('min_freq',)), (dict(min_freq=(1 << 30) + 1), ('min_freq',)), (dict(min_freq=-1), ('min_freq',)),
])
def test_refuses_a_bad_admission_record(kw, words):
  _refused([_col(), _col(), _col()], [_exp()] * 3, [_adm(), _adm(), _adm(**kw)], 'column 2', *words)


@pytest.mark.parametrize('field', ['last_seen', 'freq', 'step'])
def test_expiring_entry_refuses_null_expiry_buffers(field):
  for insert in (1, 0):
    rc, msg = _call(ENTRIES[1], [_col(), _col()], [_exp(), _exp(**{field: None})], [_adm(), _adm()], insert)
    assert rc == _lib.INVALID_ARGUMENT and 'column 1' in msg and 'NULL' in msg and 'expiry' in msg, msg


def test_counts_of_things_and_nothing_to_do():
  lib = _lib.lib()
  assert lib.hbk_hash_insert_admit_n(-1, None, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_insert_expiring_admit_n(-1, None, None, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode()
  for name in ENTRIES:
    rc, msg = _call(name, None, [_exp()], [_adm()], 1)
    assert rc == _lib.INVALID_ARGUMENT and 'cols is NULL' in msg
    rc, msg = _call(name, [_col()], [_exp()], None, 1)
    assert rc == _lib.INVALID_ARGUMENT and 'adm is NULL' in msg
  rc, msg = _call(ENTRIES[1], [_col()], None, [_adm()], 1)
  assert rc == _lib.INVALID_ARGUMENT and 'exp is NULL' in msg
  assert lib.hbk_hash_insert_admit_n(0, None, None, 1, None) == _lib.OK
  assert lib.hbk_hash_insert_expiring_admit_n(0, None, None, None, 1, None) == _lib.OK
  # no keys: NULL buffers are fine (the sketch and the counter too), nothing is launched
  cols = [_col(n_keys=0, keys=None, slots=None, keys_cache=None), _col(n_keys=0, table=None, dim=0)]
  exps = [_exp(last_seen=None, freq=None, step=None, stats=None), _exp(stats=None)]
  adms = [_adm(sketch=None, filtered=None), _adm(filtered=None)]
  for name in ENTRIES:
    for insert in (1, 0):
      assert _call(name, cols, exps, adms, insert)[0] == _lib.OK


# ---- Python argument handling ---------------------------------------------------------------------------
def test_filtered_table_state_and_unfiltered_table_unchanged():
  plain = hb.embedding.HashTable(96, 8, 'cpu', slab_size=16)
  assert plain.min_freq == 0 and not hasattr(plain, 'sketch') and not hasattr(plain, 'filter_counts')
  assert sorted(plain.variables('u')) == ['u/embedding_weights', 'u/keys']
  for call in (plain.filtered, plain.clear_filter, plain.age_filter, lambda: plain.estimate(torch.zeros(1, dtype=torch.int64))):
    with pytest.raises(_lib.InvalidArgumentError, match='min_freq'):
      call()
  t = hb.embedding.HashTable(100, 8, 'cpu', slab_size=16, min_freq=3)
  assert t.min_freq == 3 and t.capacity == 96 and not t.expiring
  assert t.sketch.dtype == torch.int32 and tuple(t.sketch.shape) == (4, 96) and not t.sketch.any()
  assert t.filter_counts.dtype == torch.int32 and tuple(t.filter_counts.shape) == (1,) and t.filtered() == 0
  v = t.variables('u')
  assert sorted(v) == ['u/admission_sketch', 'u/embedding_weights', 'u/keys'] and v['u/admission_sketch'] is t.sketch
  x = hb.embedding.HashTable(96, 8, 'cpu', slab_size=16, expiring=True, min_freq=1, sketch_depth=2, sketch_width=7,
                             sketch_seed=-3)
  assert tuple(x.sketch.shape) == (2, 7) and x.sketch_seed == -3
  assert sorted(x.variables('u')) == ['u/admission_sketch', 'u/embedding_weights', 'u/freq', 'u/keys', 'u/last_seen']
  # the descriptor is the struct's
  adm = _lib.HashAdmission()
  x._describe_admission(adm)
  assert (adm.sketch, adm.width, adm.depth, adm.min_freq, adm.seed, adm.filtered) == \
      (x.sketch.data_ptr(), 7, 2, 1, -3, x.filter_counts.data_ptr())
  # estimate is the min over the restatement's cells; clear / age / recount
  keys = np.random.RandomState(3).randint(-2 ** 63, 2 ** 63 - 1, size=300, dtype=np.int64)
  keys[:2] = [ref.EMPTY, 2 ** 63 - 1]
  for table, seed in ((t, 0), (x, -3)):
    depth, width = table.sketch.shape
    at = aref.cells(keys, depth, width, seed)
    np.testing.assert_array_equal(_ht.sketch_cells(torch.from_numpy(keys), depth, width, seed).numpy(), at)
    for r in range(depth):
      for j in (0, 1, 17):
        assert at[r, j] == ref.murmur3(ref.init_mix(int(keys[j]), r, seed)) % width     # the mix of init_value
    table.sketch.copy_(torch.from_numpy(np.random.RandomState(4).randint(0, 2 ** 31 - 1, size=(depth, width)).astype(np.int32)))
    was = table.sketch.numpy().copy()
    np.testing.assert_array_equal(table.estimate(torch.from_numpy(keys)).numpy(), aref.estimate(was, keys, seed))
    table.age_filter()
    np.testing.assert_array_equal(table.sketch.numpy(), was >> 1)
    table.filter_counts[0] = 5
    table.recount()
    assert table.filtered() == 0
    table.clear_filter()
    assert not table.sketch.any()


@pytest.mark.parametrize('kw,word', [
  (dict(min_freq=-1), 'min_freq'), (dict(min_freq=2 ** 30 + 1), 'min_freq'),
  (dict(min_freq=2, sketch_depth=0), 'sketch_depth'), (dict(min_freq=2, sketch_depth=9), 'sketch_depth'),
  (dict(min_freq=2, sketch_width=0), 'sketch_width'), (dict(min_freq=2, sketch_width=2 ** 31), 'sketch_width'),
  (dict(min_freq=2, sketch_seed=2 ** 63), 'sketch_seed'),
])
def test_constructor_refusals(kw, word):
  with pytest.raises(_lib.InvalidArgumentError, match=word):
    hb.embedding.HashTable(64, 4, 'cpu', **kw)


def test_plan_groups_tables_by_entry_and_load_bypasses_the_filter():
  kinds = [(False, 0), (True, 2), (False, 2), (True, 0), (False, 2)]
  tables = [hb.embedding.HashTable(64, 4, 'cpu', expiring=e, min_freq=f) for e, f in kinds]
  plan = _ht._Plan(tables)
  assert [(e, f, len(cols)) for e, f, cols, _, _ in plan.groups] == \
      [(False, False, 1), (False, True, 2), (True, False, 1), (True, True, 1)]
  assert all(c is not None for c in plan.cols)
  for e, f, cols, expiry, adm in plan.groups:
    assert (expiry is not None) == e and (adm is not None) == f
  plan = _ht._Plan(tables, admit=False)
  assert [(e, f, len(cols)) for e, f, cols, _, _ in plan.groups] == [(False, False, 3), (True, False, 2)]


# ---- the restatement against itself ----------------------------------------------------------------------
@pytest.mark.parametrize('slab_size,slab_count', [(5, 3), (16, 257), (64, 1), (1, 7)])
@pytest.mark.parametrize('expiring', [False, True])
def test_min_freq_1_is_the_plain_fill(slab_size, slab_count, expiring):
  rng = np.random.RandomState(slab_size * 1000 + slab_count)
  cap = slab_size * slab_count
  keys = rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=cap + 9, dtype=np.int64)
  keys = np.concatenate([keys, keys[:10], [ref.EMPTY]])
  a, b = np.full(cap, ref.EMPTY, np.int64), np.full(cap, ref.EMPTY, np.int64)
  want = ref.fill(a, slab_size, keys)
  sketch = np.zeros((3, 11), np.int32)
  seen, freq = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
  admitted, slots, n = aref.translate(b, slab_size, keys, sketch, 1, expiring, last_seen=seen, freq=freq, step=7)
  np.testing.assert_array_equal(slots, want)
  np.testing.assert_array_equal(a, b)
  assert admitted[:-1].all() and not admitted[-1]                          # every key but the sentinel
  assert n == {'inserted': int((a != ref.EMPTY).sum()), 'failed': int((want < 0).sum()), 'reused': 0, 'filtered': 0}
  assert int(sketch.sum()) == 3 * (keys.size - 1)                          # nothing was resident: every occurrence counted
  if expiring:
    np.testing.assert_array_equal(freq, np.bincount(slots[slots >= 0], minlength=cap))


@pytest.mark.parametrize('depth,width', [(1, 1), (2, 2), (4, 64), (8, 1000)])
def test_estimate_is_never_below_the_true_count(depth, width):
  rng = np.random.RandomState(depth * 31 + width)
  slab_size, slab_count, F = 8, 64, 3
  cache = np.full(slab_size * slab_count, ref.EMPTY, np.int64)
  sketch = np.zeros((depth, width), np.int32)
  pool = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=150, dtype=np.int64))
  counted = {}
  for _ in range(4):
    keys = pool[rng.randint(0, pool.size, size=120)]
    resident = np.array([aref.find_plain(cache, slab_size, int(k)) >= 0 for k in keys])
    for k in keys[~resident]:
      counted[int(k)] = counted.get(int(k), 0) + 1
    total = int(sketch[0].sum()) + int((~resident).sum())
    admitted, slots, n = aref.translate(cache, slab_size, keys, sketch, F, seed=5)
    assert int(sketch[0].sum()) == total                                    # every non-resident occurrence, once per row
    est = aref.estimate(sketch, pool, seed=5)
    assert (est >= [counted.get(int(k), 0) for k in pool]).all()
    # admitted early, never late: an id counted F times is in; every occurrence of an id has one answer
    for k in np.unique(keys[~resident]):
      mine = admitted[keys == k]
      assert mine.all() or not mine.any()
      if counted[int(k)] >= F:
        assert mine.all()
    assert (slots[admitted] >= 0).all() and (slots[~admitted & ~resident] == -1).all()
    assert n['filtered'] == int((~admitted & ~resident).sum()) and n['failed'] == 0
    if width == 1:
      np.testing.assert_array_equal(sketch, np.full((depth, 1), total))       # one cell: the total count


def test_expiring_restatement_counts_no_sentinel_and_writes_metadata_of_hits_only():
  slab_size, cap = 4, 32
  cache = np.full(cap, ref.EMPTY, np.int64)
  seen, freq = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
  sketch = np.zeros((2, 16), np.int32)
  keys = np.array([5, 6, 5, ref.EMPTY, xref.TOMBSTONE, 7], np.int64)
  admitted, slots, n = aref.translate(cache, slab_size, keys, sketch, 2, True, last_seen=seen, freq=freq, step=3)
  assert admitted.tolist() == [True, False, True, False, False, False]
  assert slots[0] == slots[2] >= 0 and slots[[1, 3, 4, 5]].tolist() == [-1] * 4
  assert n == {'inserted': 1, 'failed': 2, 'reused': 0, 'filtered': 2}
  assert int(sketch.sum()) == 2 * 4 and int(freq.sum()) == 2 and seen[slots[0]] == 3
  # the resident id counts nothing more; the plain table counts INT64_MIN + 1 as a key
  before = sketch.copy()
  aref.translate(cache, slab_size, np.array([5, 5], np.int64), sketch, 2, True, last_seen=seen, freq=freq, step=4)
  np.testing.assert_array_equal(sketch, before)
  assert freq[slots[0]] == 4 and seen[slots[0]] == 4
  plain = np.full(cap, ref.EMPTY, np.int64)
  admitted, slots, n = aref.translate(plain, slab_size, np.array([xref.TOMBSTONE] * 2, np.int64), np.zeros((1, 4), np.int32), 2)
  assert admitted.all() and slots[0] == slots[1] >= 0 and n['inserted'] == 1
