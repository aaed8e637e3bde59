"""Expiring hash tables at the C ABI and in Python's argument handling, without a GPU: the two entries exist
beside unchanged structs and version, their structs mirror the header, every refused argument is refused
before any device work with the reason named, and the sequential restatement the GPU tests compare with
(tests/support/hash_expiry_ref.py) agrees with hash_ref.fill without tombstones and with the C oracle's probe
with them."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
import oracle
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import hashtable as _ht
from tests.support import hash_expiry_ref as xref
from tests.support import hash_ref as ref

FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fake(n):
  return FAKE + n * 0x100000


def _struct_fields(name):
  text = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
  end = text.index('} %s;' % name)
  body = text[text.rindex('typedef struct {', 0, end):end]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return re.findall(r'(\w+)(?:\[\w+\])?;', body)


def test_symbols_version_and_struct_layouts():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_hash_insert_expiring_n') and hasattr(lib, 'hbk_hash_evict_n')
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  assert C.sizeof(_lib.HashColumn) == 88
  assert _lib.HashColumn.keys.offset == 24 and _lib.HashColumn.table.offset == 56
  assert _lib.HashColumn.init_scale.offset == 72 and _lib.HashColumn.seed.offset == 80
  # four pointers
  assert C.sizeof(_lib.HashExpiry) == 32
  assert [_lib.HashExpiry.last_seen.offset, _lib.HashExpiry.freq.offset, _lib.HashExpiry.step.offset,
          _lib.HashExpiry.stats.offset] == [0, 8, 16, 24]
  # pointer, three 4-byte fields (+4)
  assert C.sizeof(_lib.HashFill) == 24 and _lib.HashFill.value.offset == 16
  # pointer, int64, int32 (+4), the expiry record, int64, two int32, four fills
  E = _lib.HashEvictColumn
  assert C.sizeof(E) == 24 + 32 + 16 + 4 * 24 == 168
  assert [E.exp.offset, E.steps_to_live.offset, E.keep_freq.offset, E.n_fills.offset, E.fills.offset] == \
      [24, 56, 64, 68, 72]
  assert _lib.HASH_MAX_FILLS == 4
  assert hb.embedding.hash_evict is _ht.hash_evict


def test_header_declares_the_structs_as_mirrored():
  assert _struct_fields('hbk_hash_expiry_t') == [n for n, _ in _lib.HashExpiry._fields_]
  assert _struct_fields('hbk_hash_fill_t') == [n for n, _ in _lib.HashFill._fields_]
  assert _struct_fields('hbk_hash_evict_column_t') == [n for n, _ in _lib.HashEvictColumn._fields_]
  assert _struct_fields('hbk_hash_column_t') == [n for n, _ in _lib.HashColumn._fields_]
  text = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
  assert '#define HBK_HASH_MAX_FILLS 4' in text
  for word in ('TOMBSTONE = INT64_MIN + 1', 'steps_to_live', 'keep_freq', '2^30', 'n_reused', 'n_evicted'):
    assert word in text, word


# ---- refusals of the expiring insert ----------------------------------------------------------------------
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


def _insert_refused(cols, exps, *words):
  lib = _lib.lib()
  arr = (_lib.HashColumn * len(cols))(*cols)
  ex = (_lib.HashExpiry * len(exps))(*exps)
  for insert in (1, 0):
    rc = lib.hbk_hash_insert_expiring_n(len(cols), arr, ex, insert, None)
    msg = lib.hbk_last_error().decode()
    assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
    for w in ('hash_insert_expiring_n',) + words:
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
def test_expiring_insert_refuses_what_the_plain_insert_refuses_and_2_to_30_keys(kw, words):
  _insert_refused([_col(), _col(**kw)], [_exp(), _exp()], 'column 1', *words)


@pytest.mark.parametrize('field', ['last_seen', 'freq', 'step'])
def test_expiring_insert_refuses_null_expiry_buffers_with_keys(field):
  _insert_refused([_col(), _col(), _col()], [_exp(), _exp(), _exp(**{field: None})], 'column 2', 'NULL', 'expiry')


def test_expiring_insert_counts_of_things_and_nothing_to_do():
  lib = _lib.lib()
  assert lib.hbk_hash_insert_expiring_n(-1, None, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode()
  arr, ex = (_lib.HashColumn * 1)(_col()), (_lib.HashExpiry * 1)(_exp())
  assert lib.hbk_hash_insert_expiring_n(1, None, ex, 1, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_insert_expiring_n(1, arr, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'exp is NULL' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_insert_expiring_n(0, None, None, 1, None) == _lib.OK
  # no keys: NULL buffers are fine (the expiry's too), nothing is launched; stats may always be NULL
  arr = (_lib.HashColumn * 2)(_col(n_keys=0, keys=None, slots=None, keys_cache=None), _col(n_keys=0, table=None, dim=0))
  ex = (_lib.HashExpiry * 2)(_exp(last_seen=None, freq=None, step=None, stats=None), _exp(stats=None))
  for insert in (1, 0):
    assert lib.hbk_hash_insert_expiring_n(2, arr, ex, insert, None) == _lib.OK


# ---- refusals of the sweep -------------------------------------------------------------------------------
def _ecol(fills=(), **kw):
  col = _lib.HashEvictColumn()
  col.keys_cache, col.slab_count, col.slab_size = fake(0), 8, 16
  col.exp = _exp()
  col.steps_to_live, col.keep_freq = 3, 0
  col.n_fills = len(fills)
  for f, (base, pitch, dim, value) in enumerate(fills):
    col.fills[f].base, col.fills[f].pitch, col.fills[f].dim, col.fills[f].value = base, pitch, dim, value
  for k, v in kw.items():
    if k in ('last_seen', 'freq', 'step', 'stats'):
      setattr(col.exp, k, v)
    else:
      setattr(col, k, v)
  return col


def _evict_refused(cols, *words):
  lib = _lib.lib()
  arr = (_lib.HashEvictColumn * len(cols))(*cols)
  rc = lib.hbk_hash_evict_n(len(cols), arr, None)
  msg = lib.hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_evict_n',) + words:
    assert w in msg, msg


GOOD_FILL = (fake(9), 0, 16, 0.1)


@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)),
  (dict(slab_count=0), ('slab_count',)), (dict(keys_cache=None), ('keys_cache',)),
  (dict(last_seen=None), ('NULL', 'expiry')), (dict(freq=None), ('NULL', 'expiry')),
  (dict(step=None), ('NULL', 'expiry')),
  (dict(steps_to_live=-1), ('steps_to_live',)), (dict(keep_freq=-1), ('keep_freq',)),
  (dict(n_fills=-1), ('n_fills',)), (dict(n_fills=5), ('n_fills',)),
  (dict(fills=[GOOD_FILL, (None, 0, 16, 0.0)]), ('fill 1', 'base')),
  (dict(fills=[(fake(9), 0, 0, 0.0)]), ('fill 0', 'dim')),
  (dict(fills=[(fake(9), 15, 16, 0.0)]), ('fill 0', 'pitch')),
  (dict(fills=[(fake(9), 16, 16, float('nan'))]), ('fill 0', 'value')),
  (dict(fills=[GOOD_FILL] * 3 + [(fake(9), 16, 16, float('inf'))]), ('fill 3', 'value')),
])
def test_sweep_refusals(kw, words):
  _evict_refused([_ecol(), _ecol(**kw)], 'column 1', *words)


def test_sweep_counts_of_things_and_nothing_to_do():
  lib = _lib.lib()
  assert lib.hbk_hash_evict_n(-1, None, None) == _lib.INVALID_ARGUMENT and 'n_cols' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_evict_n(1, None, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_evict_n(0, None, None) == _lib.OK
  # steps_to_live == 0 evicts nothing: nothing is launched (the addresses are not real)
  arr = (_lib.HashEvictColumn * 2)(_ecol(steps_to_live=0), _ecol(steps_to_live=0, stats=None, fills=[GOOD_FILL] * 4))
  assert lib.hbk_hash_evict_n(2, arr, None) == _lib.OK


# ---- Python argument handling ---------------------------------------------------------------------------
def test_expiring_table_state_and_plain_table_unchanged():
  plain = hb.embedding.HashTable(96, 8, 'cpu', slab_size=16)
  assert plain.expiring is False and not hasattr(plain, 'last_seen') and not hasattr(plain, 'step')
  assert sorted(plain.variables('u')) == ['u/embedding_weights', 'u/keys']
  t = hb.embedding.HashTable(100, 8, 'cpu', slab_size=16, expiring=True)
  assert t.expiring and t.capacity == 96
  for x, shape in ((t.last_seen, (96,)), (t.freq, (96,)), (t.step, (1,)), (t.stats, (2,))):
    assert x.dtype == torch.int32 and tuple(x.shape) == shape and not x.any()
  v = t.variables('u')
  assert sorted(v) == ['u/embedding_weights', 'u/freq', 'u/keys', 'u/last_seen']
  assert v['u/last_seen'] is t.last_seen and v['u/freq'] is t.freq
  t.set_step(41)
  assert t.step.tolist() == [41]
  assert (t.size(), t.evicted(), t.reused(), t.tombstones()) == (0, 0, 0, 0)
  assert _ht.TOMBSTONE_KEY == -2 ** 63 + 1 == xref.TOMBSTONE
  # items / recount leave tombstones out (of an expiring table only)
  t.keys[:4] = torch.tensor([5, _ht.TOMBSTONE_KEY, 7, _ht.TOMBSTONE_KEY])
  plain.keys[:4] = t.keys[:4]
  assert t.items()[0].tolist() == [5, 7] and t.tombstones() == 2
  assert plain.items()[0].tolist() == [_ht.TOMBSTONE_KEY, _ht.TOMBSTONE_KEY, 5, 7]
  t.stats[0] = 9
  t.recount()
  plain.recount()
  assert t.size() == 2 and t.evicted() == 0 and plain.size() == 4


def test_python_refusals():
  plain = hb.embedding.HashTable(64, 4, 'cpu')
  t = hb.embedding.HashTable(64, 4, 'cpu', expiring=True)
  for call in (lambda: plain.set_step(1), lambda: plain.evict(3), plain.evicted, plain.reused, plain.tombstones,
               plain.compact, lambda: hb.embedding.hash_evict([t, plain], 3)):
    with pytest.raises(_lib.InvalidArgumentError, match='expiring=True'):
      call()
  good = torch.zeros(64, 4)
  for bad in ([good], [(good,)], [(good.double(), 0.0)], [(torch.zeros(63, 4), 0.0)], [(torch.zeros(64), 0.0)],
              [(good, float('nan'))], [(good, 1e39)], [(good.t().contiguous().t(), 0.0)], [(good, 0.0)] * 5):
    with pytest.raises(_lib.InvalidArgumentError, match='slots|companion'):
      t.evict(3, slots=bad)
  with pytest.raises(_lib.InvalidArgumentError, match='>= 0'):
    t.evict(-1)
  with pytest.raises(_lib.InvalidArgumentError, match='>= 0'):
    t.evict(3, keep_freq=-2)
  with pytest.raises(_lib.InvalidArgumentError, match='lists of companion'):
    hb.embedding.hash_evict([t], 3, slots=[[], []])
  with pytest.raises(_lib.HbkError, match='HBM'):                     # a host table: there is no CPU path
    t.evict(3)


# ---- the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize('slab_size,slab_count', [(5, 3), (16, 257), (64, 1), (1, 7)])
def test_restatement_without_tombstones_is_the_plain_fill(slab_size, slab_count):
  rng = np.random.RandomState(slab_size * 1000 + slab_count)
  cap = slab_size * slab_count
  keys = rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=cap + 9, dtype=np.int64)
  keys = np.concatenate([keys, keys[:10], [ref.EMPTY]])
  a, b = np.full(cap, ref.EMPTY, np.int64), np.full(cap, ref.EMPTY, np.int64)
  seen, freq = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
  want = ref.fill(a, slab_size, keys)
  slots, n_inserted, n_reused, n_failed = xref.insert(b, slab_size, keys, seen, freq, step=7)
  np.testing.assert_array_equal(slots, want)
  np.testing.assert_array_equal(a, b)
  assert (n_inserted, n_reused, n_failed) == (int((a != ref.EMPTY).sum()), 0, int((want < 0).sum()))
  placed = slots[slots >= 0]
  np.testing.assert_array_equal(freq, np.bincount(placed, minlength=cap))
  np.testing.assert_array_equal(seen, np.where(freq > 0, 7, 0))
  for n in (0, 5, len(keys) - 1):
    assert xref.find(b, slab_size, int(keys[n])) == slots[n]


@pytest.mark.parametrize('slab_size,slab_count', [(5, 3), (16, 257), (64, 1), (4, 8)])
def test_oracle_probe_finds_every_live_key_of_an_array_with_tombstones(slab_size, slab_count):
  rng = np.random.RandomState(slab_size * 77 + slab_count)
  cap = slab_size * slab_count
  n = max(3 * cap // 4, 2)
  pool = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=3 * cap, dtype=np.int64))
  rng.shuffle(pool)
  old, young, later = pool[:n // 2], pool[n // 2:n], pool[n:n + cap // 2]
  cache = np.full(cap, ref.EMPTY, np.int64)
  seen, freq = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
  s_old = xref.insert(cache, slab_size, old, seen, freq, step=1)[0]
  s_young = xref.insert(cache, slab_size, young, seen, freq, step=5)[0]
  assert (s_old >= 0).all() and (s_young >= 0).all()
  empties = int((cache == ref.EMPTY).sum())
  mask = xref.evict(cache, seen, freq, step=6, steps_to_live=3)
  np.testing.assert_array_equal(np.sort(np.where(mask)[0]), np.sort(s_old))
  assert (cache[s_old] == xref.TOMBSTONE).all() and int((cache == ref.EMPTY).sum()) == empties
  # a tombstone is to the probe a key nobody asks for: the young keys are where they were, the old ones gone
  np.testing.assert_array_equal(oracle.cache_probe(cache, slab_size, young), s_young)
  assert (oracle.cache_probe(cache, slab_size, old) == -1).all()
  # new keys reuse the tombstones; every live key is found where the restatement put it, once
  mixed = np.concatenate([later, young, later[:5]])
  slots, n_inserted, n_reused, n_failed = xref.insert(cache, slab_size, mixed, seen, freq, step=7)
  placed = slots >= 0
  assert n_inserted == np.unique(mixed[placed]).size - young.size and 0 < n_reused <= old.size
  np.testing.assert_array_equal(slots[later.size:later.size + young.size], s_young)
  np.testing.assert_array_equal(oracle.cache_probe(cache, slab_size, mixed), slots)
  live = cache[(cache != ref.EMPTY) & (cache != xref.TOMBSTONE)]
  assert np.unique(live).size == live.size


def test_restatement_keeps_walking_past_a_tombstone_to_the_spilled_key():
  slab_size, slab_count = 4, 8
  homed, k = [], 1
  while len(homed) < 6:
    if ref.home_slab(k, slab_count) == 2:
      homed.append(k)
    k += 1
  cache = np.full(slab_size * slab_count, ref.EMPTY, np.int64)
  seen, freq = np.zeros(cache.size, np.int32), np.zeros(cache.size, np.int32)
  assert xref.insert(cache, slab_size, homed[:4], seen, freq, 1)[0].tolist() == [8, 9, 10, 11]
  assert xref.insert(cache, slab_size, homed[4:5], seen, freq, 5)[0].tolist() == [12]
  assert np.where(xref.evict(cache, seen, freq, 6, 3))[0].tolist() == [8, 9, 10, 11]
  slots, n_inserted, n_reused, _ = xref.insert(cache, slab_size, homed[4:5], seen, freq, 6)
  assert (slots.tolist(), n_inserted, n_reused) == ([12], 0, 0)
  slots, n_inserted, n_reused, _ = xref.insert(cache, slab_size, homed[5:6], seen, freq, 6)
  assert (slots.tolist(), n_inserted, n_reused) == ([8], 1, 1)
  # the predicate's edges: age == ttl goes, ttl - 1 stays; freq == keep_freq stays; ttl 0 evicts nothing
  cache = np.array([1, 2, 3, 4, ref.EMPTY, xref.TOMBSTONE], np.int64)
  seen = np.array([7, 8, 7, 7, 0, 0], np.int32)
  freq = np.array([1, 1, 5, 4, 0, 0], np.int32)
  assert xref.evict_mask(cache, seen, freq, 10, 3).tolist() == [True, False, True, True, False, False]
  assert xref.evict_mask(cache, seen, freq, 10, 3, keep_freq=5).tolist() == [True, False, False, True, False, False]
  assert not xref.evict_mask(cache, seen, freq, 10, 0).any()
