"""Bounded hash tables in LFU order (hbk_hash_evict_to_lfu_n, hbk_hash_evict_to_lfu_select_n, hbk_hash_spill_lfu_n)
at the C ABI and in Python's argument handling, without a GPU: the entries exist and are declared, every refused
argument is refused before any device work with the entry, the column and the field named, ``order=`` is checked by
name on every wrapper, ``age_freq`` checks its shift, and the numpy restatement the GPU tests compare with
(tests/support/hash_evict_lfu_ref.py) agrees with a brute-force O(n^2) statement of the header's definition."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import hashtable as _ht
from tests.support import hash_evict_lfu_ref as lref

FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def fake(n):
  return FAKE + n * 0x100000


def test_symbols_and_declarations():
  lib = _lib.lib()
  for name in ('hbk_hash_evict_to_lfu_workspace_bytes', 'hbk_hash_evict_to_lfu_n', 'hbk_hash_evict_to_lfu_select_n',
               'hbk_hash_spill_lfu_n'):
    assert hasattr(lib, name), name
  assert 'size_t hbk_hash_evict_to_lfu_workspace_bytes(int32_t n_cols);' in HEADER
  for name in ('hbk_hash_evict_to_lfu_n', 'hbk_hash_evict_to_lfu_select_n'):
    assert re.search(r'int %s\(int32_t n_cols, const hbk_hash_evict_to_column_t\* cols, void\* workspace,\s+'
                     r'size_t workspace_bytes, hbk_stream_t stream\);' % name, HEADER), name
    assert getattr(lib, name).argtypes == [C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
  assert re.search(r'int hbk_hash_spill_lfu_n\(int32_t n_cols, const hbk_hash_spill_column_t\* cols, '
                   r'void\* workspace, hbk_stream_t stream\);', HEADER)
  assert lib.hbk_hash_spill_lfu_n.argtypes == [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
  assert lib.hbk_hash_evict_to_lfu_workspace_bytes.restype is C.c_size_t
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'                  # new symbols, the same version
  for word in ('WHOLE CLASSES LEAVE TOGETHER', 'no tie-break by slot', 'freq ^ 0x80000000',
               '{live_before, need, cut_freq, cut_last_seen, n_evicted, 0, 0, 0}', 'age_freq'):
    assert word in HEADER, word
  assert 'not an LFU order' not in HEADER


# ---- the evicting entry and the select ---------------------------------------------------------------------
def _col(fills=(), **kw):
  col = _lib.HashEvictToColumn()
  col.keys_cache, col.slab_count, col.slab_size = fake(0), 8, 16
  col.exp.last_seen, col.exp.freq, col.exp.step, col.exp.stats = fake(5), fake(6), fake(7), fake(8)
  col.max_size, col.keep_freq, col.report = 10, 0, fake(10)
  col.n_fills = len(fills)
  for f, (base, pitch, dim, value) in enumerate(fills):
    col.fills[f].base, col.fills[f].pitch, col.fills[f].dim, col.fills[f].value = base, pitch, dim, value
  for k, v in kw.items():
    if k in ('last_seen', 'freq', 'step', 'stats'):
      setattr(col.exp, k, v)
    else:
      setattr(col, k, v)
  return col


ENTRIES = ['hbk_hash_evict_to_lfu_n', 'hbk_hash_evict_to_lfu_select_n']


def _refused(entry, cols, workspace, nbytes, *words):
  lib = _lib.lib()
  arr = (_lib.HashEvictToColumn * len(cols))(*cols)
  rc = getattr(lib, entry)(len(cols), arr, workspace, nbytes, None)
  msg = lib.hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in (entry[len('hbk_'):] + ':',) + words:
    assert w in msg, msg


GOOD_FILL = (fake(9), 0, 16, 0.1)


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)),
  (dict(slab_count=0), ('slab_count',)), (dict(keys_cache=None), ('keys_cache',)),
  (dict(keys_cache=fake(0) + 4), ('keys_cache', 'aligned')),
  (dict(last_seen=None), ('last_seen', 'NULL')), (dict(freq=None), ('freq', 'NULL')),
  (dict(max_size=-1), ('max_size',)), (dict(keep_freq=-1), ('keep_freq',)),
  (dict(n_fills=-1), ('n_fills',)), (dict(n_fills=5), ('n_fills',)),
  (dict(fills=[GOOD_FILL, (None, 0, 16, 0.0)]), ('fill 1', 'base')),
  (dict(fills=[(fake(9), 0, 0, 0.0)]), ('fill 0', 'dim')),
  (dict(fills=[(fake(9), 15, 16, 0.0)]), ('fill 0', 'pitch')),
  (dict(fills=[(fake(9), 16, 16, float('nan'))]), ('fill 0', 'value')),
  (dict(slab_count=1 << 25, slab_size=64), ('2^31', 'slab_count')),          # exactly 2^31 slots
])
def test_refusals_name_the_entry_the_column_and_the_field(entry, kw, words):
  nbytes = _lib.lib().hbk_hash_evict_to_lfu_workspace_bytes(2)
  _refused(entry, [_col(), _col(**kw)], fake(11), nbytes, 'column 1', *words)


@pytest.mark.parametrize('entry', ENTRIES)
def test_workspace_and_counts_of_things(entry):
  lib = _lib.lib()
  size = lib.hbk_hash_evict_to_lfu_workspace_bytes
  sizes = [size(n) for n in (0, 1, 2, 32, 33)]
  assert sizes[0] == 0 and size(-3) == 0 and sizes[1] >= 4 * 2048          # a table's histogram of 11-bit digits
  assert [s // sizes[1] for s in sizes] == [0, 1, 2, 32, 33]
  cols = [_col(), _col(fills=[GOOD_FILL] * 4, stats=None, step=None)]
  _refused(entry, cols, None, sizes[2], 'workspace', 'NULL')
  _refused(entry, cols, fake(11), sizes[2] - 1, 'workspace', 'too small')
  _refused(entry, cols, fake(11) + 2, sizes[2], 'workspace', 'aligned')
  call = getattr(lib, entry)
  assert call(-1, None, None, 0, None) == _lib.INVALID_ARGUMENT and 'n_cols' in lib.hbk_last_error().decode()
  assert call(1, None, fake(11), sizes[1], None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  assert call(0, None, None, 0, None) == _lib.OK                           # nothing to do, no workspace needed


def test_the_report_may_be_null_for_the_sweep_and_not_for_the_select():
  nbytes = _lib.lib().hbk_hash_evict_to_lfu_workspace_bytes(2)
  _refused('hbk_hash_evict_to_lfu_select_n', [_col(), _col(report=None)], fake(11), nbytes, 'column 1', 'report')
  # the sweep takes a NULL report: it goes on to the workspace checks
  _refused('hbk_hash_evict_to_lfu_n', [_col(), _col(report=None)], None, nbytes, 'workspace', 'NULL')


# ---- the spill ---------------------------------------------------------------------------------------------
def _spill_col(**kw):
  col = _lib.HashSpillColumn()
  col.keys_cache, col.slab_count, col.slab_size = fake(0), 8, 16
  col.exp.last_seen, col.exp.freq, col.exp.step, col.exp.stats = fake(5), fake(6), fake(7), fake(8)
  col.selection, col.keep_freq = fake(10), 0
  col.n_moves = 1
  col.moves[0].src, col.moves[0].dst, col.moves[0].words = fake(12), fake(13), 4
  col.n_fills = 1
  col.fills[0].base, col.fills[0].pitch, col.fills[0].dim, col.fills[0].value = GOOD_FILL
  col.out_keys, col.out_slots, col.out_capacity = fake(14), fake(15), 16
  col.count, col.n_evicted = fake(16), fake(17)
  for k, v in kw.items():
    if k in ('last_seen', 'freq'):
      setattr(col.exp, k, v)
    elif k.startswith('move_'):
      setattr(col.moves[0], k[5:], v)
    elif k.startswith('fill_'):
      setattr(col.fills[0], k[5:], v)
    else:
      setattr(col, k, v)
  return col


@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_count=0), ('slab_count',)), (dict(keys_cache=None), ('keys_cache',)),
  (dict(slab_count=1 << 25, slab_size=64), ('2^31',)),
  (dict(last_seen=None), ('last_seen', 'NULL')), (dict(freq=None), ('freq', 'NULL')),
  (dict(selection=None), ('selection', 'NULL')), (dict(selection=fake(10) + 2), ('selection', 'aligned')),
  (dict(keep_freq=-1), ('keep_freq',)), (dict(n_moves=9), ('n_moves',)), (dict(n_fills=5), ('n_fills',)),
  (dict(move_words=0), ('move 0', 'words')), (dict(move_src=None), ('move 0', 'NULL')),
  (dict(move_dst=fake(12)), ('move 0', 'same array')), (dict(move_src_pitch=3), ('move 0', 'src_pitch')),
  (dict(fill_dim=0), ('fill 0', 'dim')), (dict(fill_value=float('inf')), ('fill 0', 'value')),
  (dict(count=None), ('count', 'NULL')), (dict(out_capacity=-1), ('out_capacity',)),
  (dict(out_keys=None), ('out_keys', 'NULL')),
])
def test_spill_refusals_name_the_entry_the_column_and_the_field(kw, words):
  lib = _lib.lib()
  arr = (_lib.HashSpillColumn * 2)(_spill_col(), _spill_col(**kw))
  rc = lib.hbk_hash_spill_lfu_n(2, arr, fake(20), None)
  msg = lib.hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_spill_lfu_n:', 'column 1') + words:
    assert w in msg, msg


def test_spill_workspace_and_counts_of_things():
  lib = _lib.lib()
  arr = (_lib.HashSpillColumn * 1)(_spill_col())
  for workspace, word in ((None, 'NULL'), (fake(20) + 4, 'aligned')):
    assert lib.hbk_hash_spill_lfu_n(1, arr, workspace, None) == _lib.INVALID_ARGUMENT
    msg = lib.hbk_last_error().decode()
    assert 'hash_spill_lfu_n' in msg and 'workspace' in msg and word in msg, msg
  assert lib.hbk_hash_spill_lfu_n(-1, None, None, None) == _lib.INVALID_ARGUMENT
  assert lib.hbk_hash_spill_lfu_n(1, None, fake(20), None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_spill_lfu_n(0, None, None, None) == _lib.OK
  # an out_capacity of 0 needs no out_keys: refused only at the workspace
  arr = (_lib.HashSpillColumn * 1)(_spill_col(out_capacity=0, out_keys=None))
  assert lib.hbk_hash_spill_lfu_n(1, arr, None, None) == _lib.INVALID_ARGUMENT
  assert 'workspace' in lib.hbk_last_error().decode()


# ---- Python ------------------------------------------------------------------------------------------------
def test_order_is_checked_by_name_on_every_wrapper():
  t = hb.embedding.HashTable(64, 4, 'cpu', expiring=True)
  store = hb.embedding.HashSpillStore(4)
  E = hb.embedding
  calls = [lambda o: t.evict_to(3, order=o), lambda o: t.spill_to(3, order=o), lambda o: t.maybe_evict(order=o),
           lambda o: t.maybe_evict(spill=store, order=o),
           lambda o: E.hash_evict_to([t], 3, order=o), lambda o: E.hash_evict_to_select([t], 3, order=o),
           lambda o: E.hash_spill([t], 3, order=o), lambda o: E.hash_evict_to([], 3, order=o),
           lambda o: _ht.evict_tables(None, [t], 0.75, 0.5, 0, None, order=o)]
  for call in calls:
    for bad in ('mru', 'LFU', '', None, 0):
      with pytest.raises(_lib.InvalidArgumentError, match=r"order must be 'lru' or 'lfu'"):
        call(bad)
  with pytest.raises(_lib.InvalidArgumentError, match=r"got 'fifo'"):
    t.evict_to(3, order='fifo')
  for fn in (E.HashTable.evict_to, E.HashTable.spill_to, E.HashTable.maybe_evict, E.hash_evict_to,
             E.hash_evict_to_select, E.hash_spill, E.HashGroupLookup.maybe_evict, E.HashSequenceLookup.maybe_evict,
             E.ShardedHashGroupLookup.maybe_evict):
    assert inspect.signature(fn).parameters['order'].default == 'lru', fn
  # an empty table is below any max_load: nothing to do in either order, and the empty call returns nothing
  assert t.maybe_evict(order='lfu') is None and E.hash_evict_to([], 3, order='lfu') == []
  assert E.hash_evict_to_select([], 3, order='lfu') == [] and E.hash_spill([], 3, order='lfu') == []


def test_python_refusals_of_the_lfu_calls():
  plain = hb.embedding.HashTable(64, 4, 'cpu')
  t = hb.embedding.HashTable(64, 4, 'cpu', expiring=True)
  for call in (lambda: plain.evict_to(3, order='lfu'), lambda: plain.maybe_evict(order='lfu'),
               lambda: plain.spill_to(3, order='lfu'), lambda: hb.embedding.hash_evict_to([t, plain], 3, order='lfu'),
               plain.age_freq):
    with pytest.raises(_lib.InvalidArgumentError, match='expiring=True'):
      call()
  with pytest.raises(_lib.InvalidArgumentError, match='>= 0'):
    t.evict_to(-1, order='lfu')
  with pytest.raises(_lib.InvalidArgumentError, match='>= 0'):
    t.evict_to(3, keep_freq=-2, order='lfu')
  # the report of the LFU order has eight words; the LRU one keeps four
  with pytest.raises(_lib.InvalidArgumentError, match=r'reports\[0\] must be a contiguous int32 \[8\]'):
    t.evict_to(3, report=torch.zeros(4, dtype=torch.int32), order='lfu')
  with pytest.raises(_lib.InvalidArgumentError, match=r'reports\[0\] must be a contiguous int32 \[8\]'):
    t.evict_to(3, report=torch.zeros(8, dtype=torch.int64), order='lfu')
  with pytest.raises(_lib.InvalidArgumentError, match=r'reports\[0\] must be a contiguous int32 \[4\]'):
    t.evict_to(3, report=torch.zeros(8, dtype=torch.int32))
  with pytest.raises(_lib.HbkError, match='HBM'):                          # a host table: there is no CPU path
    t.evict_to(3, report=torch.zeros(8, dtype=torch.int32), order='lfu')
  with pytest.raises(_lib.HbkError, match='HBM'):
    t.spill_to(3, order='lfu')


def test_age_freq_checks_its_shift_and_shifts():
  t = hb.embedding.HashTable(64, 4, 'cpu', expiring=True)
  for bad in (0, -1, 31, 64):
    with pytest.raises(_lib.InvalidArgumentError, match=r'shift must be in \[1, 30\]'):
      t.age_freq(bad)
  t.freq.copy_(torch.arange(64, dtype=torch.int32))
  t.freq[63] = 2 ** 30
  t.last_seen.fill_(7)
  keys = t.keys.clone()
  t.age_freq()
  assert t.freq[:63].tolist() == [v // 2 for v in range(63)] and int(t.freq[63]) == 2 ** 29
  t.age_freq(3)
  assert t.freq[:63].tolist() == [v // 16 for v in range(63)] and int(t.freq[63]) == 2 ** 26
  t.age_freq(30)
  assert not t.freq.any()
  assert torch.equal(t.keys, keys) and (t.last_seen == 7).all()


# ---- the restatement against the definition ----------------------------------------------------------------
def _brute(cache, last_seen, freq, max_size, keep_freq):
  """The header's definition, literally and in O(n^2): k as a Python int; cut = the smallest k of an evictable slot
  with #{evictable : k(slot) <= cut} >= need."""
  n = cache.size
  live = [i for i in range(n) if cache[i] not in (lref.EMPTY, lref.TOMBSTONE)]
  need = len(live) - max_size
  if need <= 0:
    return [len(live), need, 0, 0], set()
  ev = [i for i in live if keep_freq == 0 or freq[i] < keep_freq]
  k = {i: (((int(freq[i]) & 0xffffffff) ^ 0x80000000) << 32) | ((int(last_seen[i]) & 0xffffffff) ^ 0x80000000)
       for i in ev}
  cut = None
  for i in ev:
    if sum(1 for j in ev if k[j] <= k[i]) >= need and (cut is None or k[i] < cut):
      cut = k[i]
  if cut is None:
    return [len(live), need, INT32_MAX, INT32_MAX], set(ev)

  def signed(u):
    u ^= 0x80000000
    return u - 2 ** 32 if u >= 2 ** 31 else u
  return [len(live), need, signed(cut >> 32), signed(cut & 0xffffffff)], {i for i in ev if k[i] <= cut}


@pytest.mark.parametrize('span', ['small', 'signed', 'one_class'])
@pytest.mark.parametrize('keep_freq', [0, 3])
def test_restatement_against_the_brute_force_definition(span, keep_freq):
  rng = np.random.RandomState(41 + keep_freq)
  for trial in range(25):
    cap = int(rng.randint(1, 70))
    cache = np.full(cap, lref.EMPTY, np.int64)
    kind = rng.randint(0, 10, size=cap)
    cache[kind < 6] = rng.randint(1, 2 ** 40, size=int((kind < 6).sum()))
    cache[kind == 6] = lref.TOMBSTONE
    if span == 'small':
      freq, last_seen = rng.randint(1, 5, size=cap), rng.randint(1, 5, size=cap)
    elif span == 'signed':
      edge = np.array([INT32_MIN, -1, 0, 1, 2 ** 30, INT32_MAX])
      freq, last_seen = edge[rng.randint(0, 6, size=cap)], edge[rng.randint(0, 6, size=cap)]
    else:
      freq, last_seen = np.full(cap, 2), np.full(cap, 9)
    freq, last_seen = freq.astype(np.int32), last_seen.astype(np.int32)
    live = int(((cache != lref.EMPTY) & (cache != lref.TOMBSTONE)).sum())
    max_size = int(rng.randint(0, live + 3))
    want_report, want_set = _brute(cache, last_seen, freq, max_size, keep_freq)
    sel, mask = lref.select(cache, last_seen, freq, max_size, keep_freq)
    assert sel.tolist() == want_report + [len(want_set), 0, 0, 0], (span, trial)
    assert set(np.flatnonzero(mask).tolist()) == want_set
    np.testing.assert_array_equal(lref.mask_of(cache, last_seen, freq, sel, keep_freq), mask)
    # order_key is the header's k
    ev = lref.evictable_mask(cache, freq, keep_freq)
    if want_report[1] > 0 and want_set and len(want_set) >= want_report[1]:
      k = lref.order_key(freq, last_seen)
      cut = lref.order_key(np.array([sel[2]], np.int32), np.array([sel[3]], np.int32))[0]
      np.testing.assert_array_equal(ev & (k <= cut), mask)
    # the call: what leaves is reset, nothing else changes, the padding stays
    comp = rng.rand(cap, 6).astype(np.float32)
    before = [x.copy() for x in (cache, last_seen, freq, comp)]
    report, mask2 = lref.evict_to(cache, last_seen, freq, max_size, keep_freq, [(comp, 5, 0.25)])
    np.testing.assert_array_equal(report, sel)
    np.testing.assert_array_equal(mask2, mask)
    for x, y in zip((cache, last_seen, freq, comp), before):
      np.testing.assert_array_equal(x[~mask], y[~mask])
    assert (cache[mask] == lref.TOMBSTONE).all() and not last_seen[mask].any() and not freq[mask].any()
    assert (comp[mask, :5] == np.float32(0.25)).all()
    np.testing.assert_array_equal(comp[:, 5], before[3][:, 5])
    after = live - int(mask.sum())
    if want_report[1] > 0 and sel[2:4].tolist() != [INT32_MAX, INT32_MAX]:
      at_cut = int((mask & (before[2] == sel[2]) & (before[1] == sel[3])).sum())
      assert after <= max_size < after + at_cut                             # undershoot: less than the cut's class
