"""Bounded hash tables (hbk_hash_evict_to_n) at the C ABI and in Python's argument handling, without a GPU: the
two entries exist and are declared, the struct mirrors the header, every refused argument is refused before any
device work with the column and the field named, the workspace size grows with the tables and one byte short is
refused, and the numpy restatement the GPU tests compare with (tests/support/hash_evict_to_ref.py) has the
properties the header states."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import hashtable as _ht
from tests.support import hash_evict_to_ref as tref

FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()


def fake(n):
  return FAKE + n * 0x100000


def _struct_fields(name):
  end = HEADER.index('} %s;' % name)
  body = HEADER[HEADER.rindex('typedef struct {', 0, end):end]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return re.findall(r'(\w+)(?:\[\w+\])?;', body)


def test_symbols_declarations_and_struct_layout():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_hash_evict_to_n') and hasattr(lib, 'hbk_hash_evict_to_workspace_bytes')
  assert 'size_t hbk_hash_evict_to_workspace_bytes(int32_t n_cols);' in HEADER
  assert re.search(r'int hbk_hash_evict_to_n\(int32_t n_cols, const hbk_hash_evict_to_column_t\* cols, '
                   r'void\* workspace,\s+size_t workspace_bytes, hbk_stream_t stream\);', HEADER)
  assert lib.hbk_hash_evict_to_n.argtypes == [C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
  assert lib.hbk_hash_evict_to_workspace_bytes.restype is C.c_size_t
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  # hbk_hash_evict_column_t with max_size in the place of steps_to_live, and a report pointer behind the fills
  T, E = _lib.HashEvictToColumn, _lib.HashEvictColumn
  assert _struct_fields('hbk_hash_evict_to_column_t') == [n for n, _ in T._fields_]
  assert [n for n, _ in T._fields_] == \
      [n.replace('steps_to_live', 'max_size') for n, _ in E._fields_] + ['report']
  assert C.sizeof(T) == C.sizeof(E) + 8 == 176
  assert [T.exp.offset, T.max_size.offset, T.keep_freq.offset, T.n_fills.offset, T.fills.offset, T.report.offset] == \
      [24, 56, 64, 68, 72, 168]
  assert hb.embedding.hash_evict_to is _ht.hash_evict_to
  for word in ('WHOLE STEPS LEAVE TOGETHER', 'no tie-break', 'INT32_MAX', 'live_before, need, cut, n_evicted'):
    assert word in HEADER, word


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


def _refused(cols, workspace, nbytes, *words):
  lib = _lib.lib()
  arr = (_lib.HashEvictToColumn * len(cols))(*cols)
  rc = lib.hbk_hash_evict_to_n(len(cols), arr, workspace, nbytes, None)
  msg = lib.hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_evict_to_n',) + words:
    assert w in msg, msg


GOOD_FILL = (fake(9), 0, 16, 0.1)


@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)),
  (dict(slab_count=0), ('slab_count',)), (dict(keys_cache=None), ('keys_cache',)),
  (dict(last_seen=None), ('last_seen', 'NULL')), (dict(freq=None), ('freq', 'NULL')),
  (dict(max_size=-1), ('max_size',)), (dict(keep_freq=-1), ('keep_freq',)),
  (dict(n_fills=-1), ('n_fills',)), (dict(n_fills=5), ('n_fills',)),
  (dict(fills=[GOOD_FILL, (None, 0, 16, 0.0)]), ('fill 1', 'base')),
  (dict(fills=[(fake(9), 0, 0, 0.0)]), ('fill 0', 'dim')),
  (dict(fills=[(fake(9), 15, 16, 0.0)]), ('fill 0', 'pitch')),
  (dict(fills=[(fake(9), 16, 16, float('nan'))]), ('fill 0', 'value')),
  (dict(fills=[GOOD_FILL] * 3 + [(fake(9), 16, 16, float('inf'))]), ('fill 3', 'value')),
  (dict(slab_count=1 << 25, slab_size=64), ('2^31', 'slab_count')),          # exactly 2^31 slots
  (dict(slab_count=(1 << 31) + 1, slab_size=1), ('2^31', 'slab_count')),
])
def test_refusals_name_the_column_and_the_field(kw, words):
  nbytes = _lib.lib().hbk_hash_evict_to_workspace_bytes(2)
  _refused([_col(), _col(**kw)], fake(11), nbytes, 'column 1', *words)


def test_workspace_and_counts_of_things():
  lib = _lib.lib()
  size = lib.hbk_hash_evict_to_workspace_bytes
  sizes = [size(n) for n in (0, 1, 2, 32, 33, 35)]
  assert sizes[0] == 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
  assert sizes[1] >= 4 * 2048                                              # a table's histogram of 11-bit digits
  assert sizes[2] == 2 * sizes[1] and sizes[5] == 35 * sizes[1]
  cols = [_col(), _col(fills=[GOOD_FILL] * 4, stats=None, step=None, report=None)]
  _refused(cols, None, sizes[2], 'workspace', 'NULL')
  _refused(cols, fake(11), sizes[2] - 1, 'workspace', 'too small')
  _refused(cols, fake(11), 0, 'workspace', 'too small')
  _refused(cols, fake(11) + 2, sizes[2], 'workspace', 'aligned')
  assert lib.hbk_hash_evict_to_n(-1, None, None, 0, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_evict_to_n(1, None, fake(11), sizes[1], None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_evict_to_n(0, None, None, 0, None) == _lib.OK        # nothing to do, no workspace needed


def test_python_refusals():
  plain = hb.embedding.HashTable(64, 4, 'cpu')
  t = hb.embedding.HashTable(64, 4, 'cpu', expiring=True)
  for call in (lambda: plain.evict_to(3), plain.maybe_evict, lambda: hb.embedding.hash_evict_to([t, plain], 3)):
    with pytest.raises(_lib.InvalidArgumentError, match='expiring=True'):
      call()
  with pytest.raises(_lib.InvalidArgumentError, match='>= 0'):
    t.evict_to(-1)
  with pytest.raises(_lib.InvalidArgumentError, match='>= 0'):
    t.evict_to(3, keep_freq=-2)
  with pytest.raises(_lib.InvalidArgumentError, match='>= 0'):
    t.maybe_evict(keep_freq=-1)
  with pytest.raises(_lib.InvalidArgumentError, match='max_sizes'):
    hb.embedding.hash_evict_to([t], [3, 4])
  with pytest.raises(_lib.InvalidArgumentError, match='lists of companion'):
    hb.embedding.hash_evict_to([t], 3, slots=[[], []])
  with pytest.raises(_lib.InvalidArgumentError, match='reports'):
    t.evict_to(3, report=torch.zeros(4, dtype=torch.int64))
  good = torch.zeros(64, 4)
  for bad in ([good], [(good.double(), 0.0)], [(torch.zeros(63, 4), 0.0)], [(good, float('nan'))], [(good, 0.0)] * 5):
    with pytest.raises(_lib.InvalidArgumentError, match='slots|companion'):
      t.evict_to(3, slots=bad)
  for loads in (dict(max_load=0.5, target_load=0.75), dict(target_load=0.0), dict(max_load=1.5),
                dict(target_load=float('nan'))):
    with pytest.raises(_lib.InvalidArgumentError, match='target_load'):
      t.maybe_evict(**loads)
    with pytest.raises(_lib.InvalidArgumentError, match='target_load'):   # what the lookups' maybe_evict calls
      _ht.evict_tables(None, [t], loads.get('max_load', 0.75), loads.get('target_load', 0.5), 0, None)
  for cls in (hb.embedding.HashGroupLookup, hb.embedding.HashSequenceLookup, hb.embedding.ShardedHashGroupLookup):
    assert callable(cls.maybe_evict)
  assert t.maybe_evict() is None and t.maybe_evict(1.0, 1.0) is None       # an empty table: below any max_load
  with pytest.raises(_lib.HbkError, match='HBM'):                          # a host table: there is no CPU path
    t.evict_to(3)
  assert hb.embedding.hash_evict_to([], 3) == []


# ---- the restatement's own properties -------------------------------------------------------------------
def _random_table(rng, cap, steps):
  cache = np.full(cap, tref.EMPTY, np.int64)
  kind = rng.randint(0, 10, size=cap)
  cache[kind < 6] = rng.randint(1, 2 ** 40, size=int((kind < 6).sum()))
  cache[kind == 6] = tref.TOMBSTONE
  last_seen = rng.randint(steps[0], steps[1], size=cap).astype(np.int32)
  freq = rng.randint(1, 6, size=cap).astype(np.int32)
  return cache, last_seen, freq


@pytest.mark.parametrize('steps', [(1, 7), (-2 ** 31, 2 ** 31 - 1), (5, 6)])
@pytest.mark.parametrize('keep_freq', [0, 3])
def test_reference_bounds_the_size_and_touches_nothing_younger_than_the_cut(steps, keep_freq):
  rng = np.random.RandomState(7 + keep_freq)
  for trial in range(20):
    cache, last_seen, freq = _random_table(rng, 200, steps)
    live = int(((cache != tref.EMPTY) & (cache != tref.TOMBSTONE)).sum())
    max_size = int(rng.randint(0, live + 3))
    comp = rng.rand(200, 6).astype(np.float32)
    before = [x.copy() for x in (cache, last_seen, freq, comp)]
    l0, need0, cut0 = tref.cut_of(cache, last_seen, freq, max_size, keep_freq)
    report, mask = tref.evict_to(cache, last_seen, freq, max_size, keep_freq, [(comp, 5, 0.25)])
    assert report.tolist() == [live, live - max_size, cut0, int(mask.sum())] and (l0, need0) == (live, live - max_size)
    after = int(((cache != tref.EMPTY) & (cache != tref.TOMBSTONE)).sum())
    assert after == live - int(mask.sum())
    if need0 <= 0:
      assert not mask.any()
      for x, y in zip((cache, last_seen, freq, comp), before):
        np.testing.assert_array_equal(x, y)
      continue
    # inside the bound, or every evictable slot is gone
    assert after <= max_size or not tref.evictable_mask(cache, freq, keep_freq).any()
    if after > max_size:
      assert cut0 == tref.INT32_MAX and report[3] < report[1]
    else:
      # the undershoot is less than the keys of one step: without the cut's own step the bound would not hold
      at_cut = int((mask & (before[1] == cut0)).sum())
      assert after + at_cut > max_size
    # no slot younger than the cut, no protected slot and no free slot is touched
    spared = (before[1].astype(np.int64) > cut0) | ~tref.evictable_mask(before[0], before[2], keep_freq)
    assert not (mask & spared).any()
    for x, y in zip((cache, last_seen, freq, comp), before):
      np.testing.assert_array_equal(x[~mask], y[~mask])
    assert (cache[mask] == tref.TOMBSTONE).all() and not last_seen[mask].any() and not freq[mask].any()
    assert (comp[mask, :5] == np.float32(0.25)).all()
    np.testing.assert_array_equal(comp[:, 5], before[3][:, 5])            # the padding stays
