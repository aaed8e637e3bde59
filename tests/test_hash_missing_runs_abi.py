"""The miss list over runs and the forward in three parts at the C ABI and in Python's argument handling, without a
GPU: hbk_hash_missing_runs_n, hbk_sharded_lookup_fwd_ids / _gather and hbk_sharded_hash_missing exist and are declared,
the new struct mirrors the header beside unchanged existing structs, every refused argument is refused before any
device work with the column and the field named, the state rules of the three-part forward name the call, and the
numpy restatement the GPU tests compare with gives a hand-written case on the concatenation of the runs."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import HashSpillStore, HashTable, ShardedHashGroupLookup
from tests.support import hash_missing_ref as mref

FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
FLAT = re.sub(r'/\*.*?\*/', '', HEADER, flags=re.S)
EMPTY, TOMBSTONE = mref.EMPTY, mref.TOMBSTONE


def fake(n):
  return FAKE + n * 0x100000


def _struct_fields(name):
  end = HEADER.index('} %s;' % name)
  body = HEADER[HEADER.rindex('typedef struct {', 0, end):end]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return re.findall(r'(\w+)(?:\[\w+\])?;', body)


def _proto(ret, name):
  return ' '.join(re.search(r'%s %s\((.*?)\);' % (ret, name), FLAT, flags=re.S).group(1).split())


# ---- ABI --------------------------------------------------------------------------------------------------
def test_symbols_declarations_and_struct_layout():
  lib = _lib.lib()
  vp = C.c_void_p
  assert _proto('int', 'hbk_hash_missing_runs_n') == (
    'int32_t n_cols, const hbk_hash_missing_runs_column_t* cols, const int32_t* n_runs, '
    'const hbk_hash_run_t* const* runs, void* workspace, size_t workspace_bytes, hbk_stream_t stream')
  assert _proto('size_t', 'hbk_hash_missing_runs_workspace_bytes') == (
    'int32_t n_cols, const int32_t* n_runs, const hbk_hash_run_t* const* runs')
  assert lib.hbk_hash_missing_runs_n.argtypes == [C.c_int32, vp, vp, vp, vp, C.c_size_t, vp]
  assert lib.hbk_hash_missing_runs_n.restype is C.c_int
  assert lib.hbk_hash_missing_runs_workspace_bytes.argtypes == [C.c_int32, vp, vp]
  assert lib.hbk_hash_missing_runs_workspace_bytes.restype == C.c_size_t
  assert _proto('int', 'hbk_sharded_lookup_fwd_ids') == (
    'hbk_sharded_t plan, const int64_t* const* ids, const int64_t* n_ids, const int32_t* const* row_splits, '
    'const int64_t* n_segments, hbk_stream_t stream')
  assert _proto('int', 'hbk_sharded_lookup_fwd_gather') == 'hbk_sharded_t plan, hbk_stream_t stream'
  assert _proto('int', 'hbk_sharded_hash_missing') == (
    'hbk_sharded_t plan, const uint8_t* want , int64_t* const* out_ids, const int64_t* out_capacity, '
    'int64_t* counts , hbk_stream_t stream')
  assert lib.hbk_sharded_lookup_fwd_ids.argtypes == [vp] * 6
  assert lib.hbk_sharded_lookup_fwd_gather.argtypes == [vp] * 2
  assert lib.hbk_sharded_hash_missing.argtypes == [vp] * 6
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  T = _lib.HashMissingRunsColumn
  names = [n for n, _ in T._fields_]
  assert _struct_fields('hbk_hash_missing_runs_column_t') == names
  assert names == ['keys_cache', 'slab_count', 'slab_size', 'exp', 'out_ids', 'out_capacity', 'count']
  assert C.sizeof(T) == 24 + 32 + 3 * 8 == 80                 # geometry, expiry, three 8-byte fields
  assert [getattr(T, n).offset for n in names] == [0, 8, 16, 24, 56, 64, 72]
  assert C.sizeof(_lib.HashRun) == 24 and _struct_fields('hbk_hash_run_t') == ['keys', 'slots', 'n_keys']
  # the existing structs are what they were
  sizes = {'HashColumn': 88, 'HashExpiry': 32, 'HashAdmission': 40, 'HashFill': 24, 'HashMove': 32,
           'HashSequence': 40, 'HashMissingColumn': 104, 'HashRemoveColumn': 192, 'HashSpillColumn': 472,
           'ShardedHash': 128}
  for name, size in sizes.items():
    assert C.sizeof(getattr(_lib, name)) == size, name
  for word in ('FIRST OCCURRENCE in E_c', 'at its earlier run', 'padded up to whole tiles of 256', 'a column\'s runs '
               'never split', 'valid only between the two', 'drops an open step'):
    assert word in HEADER, word


def _col(**kw):
  col = _lib.HashMissingRunsColumn()
  col.keys_cache, col.slab_count, col.slab_size = fake(0), 8, 16
  col.exp.last_seen, col.exp.freq, col.exp.step, col.exp.stats = fake(5), fake(6), None, None
  col.out_ids, col.out_capacity, col.count = fake(3), 7, fake(4)
  for k, v in kw.items():
    if k in ('last_seen', 'freq'):
      setattr(col.exp, k, v)
    else:
      setattr(col, k, v)
  return col


def _run(n_keys=7, keys=fake(1), slots=fake(2)):
  r = _lib.HashRun()
  r.keys, r.slots, r.n_keys = keys, slots, n_keys
  return r


class Args:
  """cols and runs[c] (lists of HashRun, or None for a NULL runs[c]) marshalled for the two entries."""

  def __init__(self, cols, runs, n_runs=None):
    n = len(cols)
    self.n = n
    self.cols = (_lib.HashMissingRunsColumn * max(n, 1))(*cols)
    self.keep = [(_lib.HashRun * max(len(r), 1))(*r) if r is not None else None for r in runs]
    self.n_runs = (C.c_int32 * max(n, 1))(*(n_runs or [len(r) if r is not None else 0 for r in runs]))
    self.runs = (C.c_void_p * max(n, 1))(*[C.addressof(a) if a is not None else None for a in self.keep])

  def need(self):
    return _lib.lib().hbk_hash_missing_runs_workspace_bytes(self.n, self.n_runs, self.runs)


def _refused(cols, runs, words, n_runs=None, workspace=fake(10), nbytes=1 << 40):
  lib = _lib.lib()
  a = Args(cols, runs, n_runs)
  rc = lib.hbk_hash_missing_runs_n(a.n, a.cols, a.n_runs, a.runs, workspace, nbytes, None)
  msg = lib.hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_missing_runs_n',) + tuple(words):
    assert w in msg, msg


@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)),
  (dict(slab_count=0), ('slab_count',)), (dict(slab_count=1 << 60), ('slab_count',)),
  (dict(keys_cache=None), ('keys_cache', 'NULL')),
  (dict(keys_cache=fake(0) + 4), ('keys_cache', 'aligned')),
  (dict(last_seen=None), ('last_seen', 'NULL')), (dict(freq=None), ('freq', 'NULL')),
  (dict(out_ids=None), ('out_ids', 'NULL', 'out_capacity')),
  (dict(out_capacity=-1), ('out_capacity',)),
  (dict(count=None), ('count', 'NULL')),
])
def test_table_refusals_name_the_column_and_the_field(kw, words):
  """Column 0 is fine; column 1 carries the fault; both have ids waiting at fake addresses: nothing may be
  launched."""
  _refused([_col(), _col(**kw)], [[_run()], [_run(), _run()]], ('column 1',) + words)


@pytest.mark.parametrize('runs,n_runs,words', [
  ([_run()], [-1], ('n_runs', '>= 0')),
  (None, [2], ('runs is NULL', 'n_runs = 2')),
  ([_run(), _run(n_keys=-1)], None, ('run 1', 'n_keys')),
  ([_run(), _run(n_keys=1 << 31)], None, ('run 1', 'n_keys', '2^31')),
  ([_run(keys=None)], None, ('run 0', 'NULL buffer')),
  ([_run(), _run(), _run(slots=None)], None, ('run 2', 'NULL buffer')),
  ([_run(n_keys=1 << 29), _run(n_keys=1 << 29)], None, ('runs sum to', '2^30')),
  ([_run(n_keys=1)] * 257, None, ('n_runs', '257', '256')),
])
def test_run_refusals_name_the_column_and_the_run(runs, n_runs, words):
  _refused([_col(), _col()], [[_run()], runs], ('column 1',) + words, n_runs=None if n_runs is None else [1] + n_runs)


def test_null_run_arrays_and_counts_of_things():
  lib = _lib.lib()
  f = lib.hbk_hash_missing_runs_n
  assert f(-1, None, None, None, None, 0, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode()
  assert f(1, None, None, None, None, 0, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  a = Args([_col()], [[_run()]])
  assert f(1, a.cols, None, a.runs, fake(10), 1 << 30, None) == _lib.INVALID_ARGUMENT
  assert 'n_runs or runs is NULL' in lib.hbk_last_error().decode()
  assert f(1, a.cols, a.n_runs, None, fake(10), 1 << 30, None) == _lib.INVALID_ARGUMENT
  # zero columns, and columns without ids (no runs, empty runs with NULL buffers): fine, nothing to launch
  assert f(0, None, None, None, None, 0, None) == _lib.OK
  assert lib.hbk_hash_missing_runs_workspace_bytes(0, None, None) == 0
  assert Args([_col()], [[_run(0, None, None)] * 3]).need() == 0


def test_workspace_refusals_name_the_size():
  cols = [_col(), _col()]
  runs = [[_run(7)], [_run(1025), _run(0, None, None), _run(1)]]
  # 7 ids: 64 cells, 1 tile; 1026 ids in runs of 1025 and 1: 4096 cells, 5 + 1 tiles; 12 bytes per cell and per tile
  need = (64 + 4096) * 12 + (1 + 6) * 12
  assert Args(cols, runs).need() == need
  _refused(cols, runs, ('workspace', 'NULL', str(need)), workspace=None)
  _refused(cols, runs, ('workspace', 'too small', str(need)), nbytes=need - 1)
  _refused(cols, runs, ('workspace', 'aligned'), workspace=fake(10) + 8)
  # a column whose counts are out of range adds nothing to the size; the call refuses it
  assert Args(cols, [runs[0], [_run(-1)]]).need() == 64 * 12 + 12


def test_the_largest_columns_pass_every_check_of_sizes():
  """Three columns of 2^30 - 1 ids at slab 64: below the key limit, their padded positions below 2^31 and their
  launch group's find below 2^31 tiles.  The one thing left to refuse, before any device work, is the workspace."""
  cols = [_col(slab_size=64) for _ in range(3)]
  big = [_run(n_keys=(1 << 30) - 1)]
  _refused(cols, [big, big, big], ('workspace is NULL',), workspace=None, nbytes=0)


# ---- the three-part forward's state rules ------------------------------------------------------------------------
def test_three_part_state_refusals_name_the_call():
  lib = _lib.lib()
  for call, who in ((lambda: lib.hbk_sharded_lookup_fwd_gather(None, None), 'sharded_lookup_fwd_gather'),
                    (lambda: lib.hbk_sharded_lookup_fwd_ids(None, None, None, None, None, None),
                     'sharded_lookup_fwd_ids'),
                    (lambda: lib.hbk_sharded_hash_missing(None, None, None, None, None, None),
                     'sharded_hash_missing')):
    assert call() == _lib.INVALID_ARGUMENT
    assert who in lib.hbk_last_error().decode() and 'plan is NULL' in lib.hbk_last_error().decode()


# ---- Python argument handling ---------------------------------------------------------------------------------
def _driver(tables, stores, accums=None):
  """A ShardedHashGroupLookup as its constructor leaves it before the stores are checked: the constructor itself
  needs tables in HBM."""
  drv = ShardedHashGroupLookup.__new__(ShardedHashGroupLookup)
  drv.tables, drv.stores, drv.accums = list(tables), stores, accums
  drv.moments = drv.ftrl_slots = drv.row_accums = None
  drv.initial_accumulator_value = 0.1
  drv._rows = [t.table for t in tables]
  return drv


def test_python_refusals():
  plain = HashTable(64, 4, 'cpu')
  t = HashTable(64, 4, 'cpu', expiring=True)
  store = HashSpillStore(4, pin_memory=False)
  accum = torch.zeros(64, 4)
  with pytest.raises(_lib.InvalidArgumentError, match='expiring=True'):
    _driver([plain], [store])._check_stores()                                # a store on a plain table
  with pytest.raises(_lib.InvalidArgumentError, match='one spill store'):
    _driver([t], [store, store])._check_stores()                             # stores of the wrong length
  with pytest.raises(_lib.InvalidArgumentError, match='store'):
    _driver([t], [HashSpillStore(5, pin_memory=False)])._check_stores()      # wrong row dim
  with pytest.raises(_lib.InvalidArgumentError, match='companions of widths'):
    _driver([t], [store], accums=[accum])._check_stores()                    # the bound slot is not in the store
  with pytest.raises(_lib.InvalidArgumentError, match='companions of widths'):
    _driver([t], [HashSpillStore(4, [3], pin_memory=False)], accums=[accum])._check_stores()   # wrong slot dim
  with pytest.raises(_lib.InvalidArgumentError, match='HashSpillStore'):
    _driver([t], [object()])._check_stores()
  _driver([t, plain], [HashSpillStore(4, [4], pin_memory=False), None], accums=[accum, accum.clone()])._check_stores()
  with pytest.raises(_lib.HbkError, match='launch_begin'):                   # the one-call first half would translate
    _driver([t], [store]).launch_begin(None)                                 # before anything could come back
  bare = _driver([t], None)
  bare._check_stores()
  with pytest.raises(_lib.InvalidArgumentError, match='without stores'):
    bare.spill_to(8)
  with pytest.raises(_lib.InvalidArgumentError, match='spill=True'):
    bare.maybe_evict(spill=True)
  assert bare.fault_in_received() == [0] and bare.last_restored == [0]       # no store: nothing to ask, no plan made


# ---- the restatement on the concatenation of the runs -----------------------------------------------------------
def test_reference_on_the_concatenation_by_hand():
  cache = np.array([10, EMPTY, TOMBSTONE, -1, 30, EMPTY], np.int64)
  runs = [np.array([7, 10, 7], np.int64), np.zeros(0, np.int64), np.array([EMPTY, 99, -1, TOMBSTONE], np.int64),
          np.array([99, 5, 30, 7], np.int64)]
  slots, missed = mref.missing(cache, np.concatenate(runs))
  per_run = np.split(slots, np.cumsum([r.size for r in runs])[:-1])
  assert [s.tolist() for s in per_run] == [[-1, 0, -1], [], [-1, -1, 3, -1], [-1, -1, 4, -1]]
  assert missed.tolist() == [7, 99, 5]          # 7 and 99 at their earlier runs; the sentinels never
  # the runs in another order: the earlier run still decides
  assert mref.missing(cache, np.concatenate(runs[::-1]))[1].tolist() == [99, 5, 7]
