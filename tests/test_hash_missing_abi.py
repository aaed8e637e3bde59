"""The device-side miss list (hbk_hash_missing_n, hash_missing / hash_missing_sequence / hash_fault_in) at the C ABI
and in Python's argument handling, without a GPU: the entries exist and are declared, the struct mirrors the header
beside unchanged existing structs, every refused argument is refused before any device work with the column and the
field named, and the numpy restatement the GPU tests compare with (tests/support/hash_missing_ref.py) gives a
hand-written case."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import HashSpillStore, HashTable
from hybridbackend_amd.embedding import hash_sequence as _hs
from hybridbackend_amd.embedding import hashtable as _ht
from tests.support import hash_missing_ref as mref

FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
EMPTY, TOMBSTONE = mref.EMPTY, mref.TOMBSTONE


def fake(n):
  return FAKE + n * 0x100000


def _struct_fields(name):
  end = HEADER.index('} %s;' % name)
  body = HEADER[HEADER.rindex('typedef struct {', 0, end):end]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return re.findall(r'(\w+)(?:\[\w+\])?;', body)


# ---- ABI --------------------------------------------------------------------------------------------------
def test_symbols_declaration_and_struct_layout():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_hash_missing_n') and hasattr(lib, 'hbk_hash_missing_workspace_bytes')
  flat = re.sub(r'/\*.*?\*/', '', HEADER, flags=re.S)
  proto = ' '.join(re.search(r'int hbk_hash_missing_n\((.*?)\);', flat, flags=re.S).group(1).split())
  assert proto == ('int32_t n_cols, const hbk_hash_missing_column_t* cols, const hbk_hash_sequence_t* seq, '
                   'void* workspace, size_t workspace_bytes, hbk_stream_t stream')
  proto = ' '.join(re.search(r'size_t hbk_hash_missing_workspace_bytes\((.*?)\);', flat, flags=re.S).group(1).split())
  assert proto == 'int32_t n_cols, const hbk_hash_missing_column_t* cols, const hbk_hash_sequence_t* seq'
  assert lib.hbk_hash_missing_n.argtypes == [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
  assert lib.hbk_hash_missing_workspace_bytes.argtypes == [C.c_int32, C.c_void_p, C.c_void_p]
  assert lib.hbk_hash_missing_workspace_bytes.restype == C.c_size_t
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  T = _lib.HashMissingColumn
  names = [n for n, _ in T._fields_]
  assert _struct_fields('hbk_hash_missing_column_t') == names
  assert names == ['keys_cache', 'slab_count', 'slab_size', 'exp', 'keys', 'n_keys', 'slots', 'out_ids',
                   'out_capacity', 'count']
  # 24 geometry + 32 expiry + six 8-byte fields
  assert C.sizeof(T) == 24 + 32 + 6 * 8 == 104
  assert [getattr(T, n).offset for n in names] == [0, 8, 16, 24, 56, 64, 72, 80, 88, 96]
  assert [getattr(T, n).size for n in names] == [8, 8, 4, 32, 8, 8, 8, 8, 8, 8]
  # the existing structs are what they were
  sizes = {'HashColumn': 88, 'HashExpiry': 32, 'HashAdmission': 40, 'HashFill': 24, 'HashMove': 32,
           'HashSequence': 40, 'HashEvictColumn': 168, 'HashEvictToColumn': 176, 'HashRemoveColumn': 192,
           'HashRehashColumn': 328, 'HashExportColumn': 328, 'HashStoreColumn': 288, 'HashSpillColumn': 472,
           'ShardedHash': 128}
  for name, size in sizes.items():
    assert C.sizeof(getattr(_lib, name)) == size, name
  assert hb.embedding.hash_missing is _ht.hash_missing
  assert hb.embedding.hash_fault_in is _ht.hash_fault_in
  assert hb.embedding.hash_missing_sequence is _hs.hash_missing_sequence
  assert callable(HashTable.missing) and callable(hb.embedding.HashSequenceLookup.fault_in)
  for word in ('FIRST OCCURRENCE', 'never reported', 'NOT written', 'functions of the inputs alone', 'no spin loop',
               'atomicMin(first[cell], p)', 'groups of 32'):
    assert word in HEADER, word


def _col(**kw):
  col = _lib.HashMissingColumn()
  col.keys_cache, col.slab_count, col.slab_size = fake(0), 8, 16
  col.exp.last_seen, col.exp.freq, col.exp.step, col.exp.stats = fake(5), fake(6), None, None
  col.keys, col.n_keys, col.slots = fake(1), 7, fake(2)
  col.out_ids, col.out_capacity, col.count = fake(3), 7, fake(4)
  for k, v in kw.items():
    if k in ('last_seen', 'freq', 'step', 'stats'):
      setattr(col.exp, k, v)
    else:
      setattr(col, k, v)
  return col


def _seq(**kw):
  q = _lib.HashSequence()
  q.row_splits, q.n_segments, q.max_len, q.has_pad, q.pad_id, q.lengths = fake(7), 3, 4, 0, 0, None
  for k, v in kw.items():
    setattr(q, k, v)
  return q


def _refused(cols, seqs, words, workspace=fake(10), nbytes=1 << 20):
  lib = _lib.lib()
  arr = (_lib.HashMissingColumn * len(cols))(*cols)
  sarr = (_lib.HashSequence * len(seqs))(*seqs) if seqs is not None else None
  rc = lib.hbk_hash_missing_n(len(cols), arr, sarr, workspace, nbytes, None)
  msg = lib.hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_missing_n',) + tuple(words):
    assert w in msg, msg


@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)),
  (dict(slab_count=0), ('slab_count',)), (dict(slab_count=1 << 60), ('slab_count',)),
  (dict(keys_cache=None), ('keys_cache', 'NULL')),
  (dict(keys_cache=fake(0) + 4), ('keys_cache', 'aligned')),
  (dict(last_seen=None), ('last_seen', 'NULL')), (dict(freq=None), ('freq', 'NULL')),
  (dict(keys=None), ('keys', 'NULL')), (dict(slots=None), ('slots', 'NULL')),
  (dict(n_keys=-1), ('n_keys',)), (dict(n_keys=1 << 31), ('n_keys', '2^31')),
  (dict(out_ids=None), ('out_ids', 'NULL', 'out_capacity')),
  (dict(out_capacity=-1), ('out_capacity',)),
  (dict(count=None), ('count', 'NULL')),
])
def test_flat_refusals_name_the_column_and_the_field(kw, words):
  """Column 0 is fine; column 1 carries the fault; both have ids waiting at fake addresses: nothing may be
  launched."""
  _refused([_col(), _col(**kw)], None, ('column 1',) + words)


@pytest.mark.parametrize('ckw,qkw,words', [
  ({}, dict(max_len=0), ('max_len',)),
  ({}, dict(n_segments=-1), ('n_segments',)),
  ({}, dict(n_segments=1 << 28, max_len=4), ('2^30',)),
  ({}, dict(n_segments=1 << 31, max_len=1), ('2^30',)),
  (dict(slots=None), {}, ('slots', 'NULL')),
  (dict(n_keys=1 << 31), {}, ('n_keys', '2^31')),
  (dict(keys=None), {}, ('keys', 'NULL')),
  ({}, dict(row_splits=None), ('row_splits', 'n_keys 7', 'n_segments 3')),
  ({}, dict(has_pad=1, pad_id=EMPTY), ('pad_id', 'EMPTY')),
  ({}, dict(has_pad=1, pad_id=TOMBSTONE), ('pad_id', 'TOMBSTONE')),
  (dict(count=None), {}, ('count', 'NULL')),
  (dict(out_ids=None), {}, ('out_ids', 'NULL')),
  (dict(last_seen=None), {}, ('last_seen', 'NULL')),
])
def test_sequence_refusals_name_the_column_and_the_field(ckw, qkw, words):
  _refused([_col(out_capacity=12), _col(out_capacity=12, **ckw)], [_seq(), _seq(**qkw)], ('column 1',) + words)


def test_workspace_refusals_name_the_size():
  lib = _lib.lib()
  cols = [_col(), _col(n_keys=1025)]
  arr = (_lib.HashMissingColumn * 2)(*cols)
  # 7 ids: 64 cells, 1 tile; 1025 ids: 4096 cells, 5 tiles; 12 bytes per cell, 8 per tile
  need = (64 + 4096) * 12 + (1 + 5) * 8
  assert lib.hbk_hash_missing_workspace_bytes(2, arr, None) == need
  _refused(cols, None, ('workspace', 'NULL', str(need)), workspace=None)
  _refused(cols, None, ('workspace', 'too small', str(need)), nbytes=need - 1)
  _refused(cols, None, ('workspace', 'aligned'), workspace=fake(10) + 4)
  # the sequence form sizes by B * T, whatever the ids' number; an empty column needs nothing
  sarr = (_lib.HashSequence * 2)(_seq(), _seq(n_segments=0))
  assert lib.hbk_hash_missing_workspace_bytes(2, arr, sarr) == 64 * 12 + 8
  _refused(cols, [_seq(), _seq(n_segments=300)], ('workspace', 'too small'), nbytes=(64 + 4096) * 12 + 6 * 8 - 1)
  assert lib.hbk_hash_missing_workspace_bytes(0, None, None) == 0


def test_a_find_grid_too_large_is_refused_before_the_first_group_runs():
  """33 columns of 2^31 - 1 ids at slab 64: the second launch group is fine, the first needs 32 x (2^26 + 1) find
  tiles.  Refused at the column that crosses 2^31, before anything is launched on the fake addresses."""
  cols = [_col(n_keys=(1 << 31) - 1, slab_size=64) for _ in range(33)]
  _refused(cols, None, ('column 31', 'n_keys', '2^31', 'tiles'), nbytes=1 << 62)


def test_counts_of_things():
  lib = _lib.lib()
  assert lib.hbk_hash_missing_n(-1, None, None, None, 0, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_missing_n(1, None, None, None, 0, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_missing_n(0, None, None, None, 0, None) == _lib.OK


# ---- Python argument handling ---------------------------------------------------------------------------------
def test_python_refusals():
  plain = HashTable(64, 4, 'cpu')
  t = HashTable(64, 4, 'cpu', expiring=True)
  ids = torch.arange(5, dtype=torch.int64)
  store = HashSpillStore(4, pin_memory=False)
  # a plain table: refused with the reason
  for call in (lambda: plain.missing(ids), lambda: hb.embedding.hash_missing([t, plain], [ids, ids]),
               lambda: hb.embedding.hash_missing_sequence([plain], [ids], max_lens=4),
               lambda: hb.embedding.hash_fault_in([plain], [ids], [store])):
    with pytest.raises(_lib.InvalidArgumentError, match='expiring=True'):
      call()
  # list lengths
  with pytest.raises(_lib.InvalidArgumentError, match='id tensors'):
    hb.embedding.hash_missing([t], [ids, ids])
  with pytest.raises(_lib.InvalidArgumentError, match='id tensors'):
    hb.embedding.hash_fault_in([t], [ids, ids], [store])
  with pytest.raises(_lib.InvalidArgumentError, match='spill stores'):
    hb.embedding.hash_fault_in([t], [ids], [store, store])
  with pytest.raises(_lib.InvalidArgumentError, match='lists of companion'):
    hb.embedding.hash_fault_in([t], [ids], [store], slots=[[], []])
  with pytest.raises(_lib.InvalidArgumentError, match='row_splits'):
    hb.embedding.hash_fault_in([t], [ids], [store], row_splits=[None, None], max_lens=4)
  with pytest.raises(_lib.InvalidArgumentError, match='row_splits'):
    hb.embedding.hash_missing_sequence([t], [ids], row_splits=[None, None], max_lens=4)
  with pytest.raises(_lib.InvalidArgumentError, match='max_lens'):
    hb.embedding.hash_missing_sequence([t], [ids])
  with pytest.raises(_lib.InvalidArgumentError, match='max_lens'):
    hb.embedding.hash_fault_in([t], [ids], [store], pad_ids=3)
  with pytest.raises(_lib.InvalidArgumentError, match='sentinel'):
    hb.embedding.hash_missing_sequence([t], [ids], max_lens=4, pad_ids=TOMBSTONE)
  # a store of the wrong widths, or no store
  comp = torch.zeros(64, 2)
  for wrong, slots in ((HashSpillStore(5, pin_memory=False), ()), (HashSpillStore(4, [4], pin_memory=False), [comp]),
                       (store, [comp]), (None, ()), (object(), ())):
    with pytest.raises(_lib.InvalidArgumentError, match='store'):
      hb.embedding.hash_fault_in([t], [ids], [wrong], slots=[slots])
  # ids that are no int64 vector
  for bad in (ids.int(), ids.float(), ids.reshape(5, 1), ids.tolist()):
    with pytest.raises(_lib.InvalidArgumentError, match='int64'):
      t.missing(bad)
  with pytest.raises(_lib.HbkError, match='HBM'):                          # a host table: there is no CPU path
    t.missing(ids)
  with pytest.raises(_lib.HbkError, match='HBM'):
    hb.embedding.hash_fault_in([t], [ids], [store])
  # no table: nothing to do
  assert hb.embedding.hash_missing([], []) == []
  assert hb.embedding.hash_missing_sequence([], [], max_lens=3) == []
  assert hb.embedding.hash_fault_in([], [], []) == []


# ---- the restatement against a hand-written case ----------------------------------------------------------------
def test_reference_by_hand():
  cache = np.array([10, EMPTY, TOMBSTONE, -1, 30, EMPTY], np.int64)
  ids = np.array([7, 10, 7, EMPTY, 99, -1, TOMBSTONE, 99, 5, 30], np.int64)
  slots, missed = mref.missing(cache, ids)
  assert slots.tolist() == [-1, 0, -1, -1, -1, 3, -1, -1, -1, 4]
  assert missed.tolist() == [7, 99, 5]
  # samples of lengths 0, 1, 4 and 5 at T = 3, without a pad id: the ids past T (30 of sample 2, 5 and 8 of
  # sample 3) are not read
  splits = np.array([0, 0, 1, 5, 10], np.int32)
  e, there = mref.effective(ids, splits, 3)
  assert e.tolist() == [EMPTY] * 3 + [7, EMPTY, EMPTY] + [10, 7, EMPTY] + [-1, TOMBSTONE, 99]
  assert there.tolist() == [False] * 3 + [True, False, False] + [True] * 6
  slots, missed = mref.missing(cache, ids, splits, 3)
  assert slots.tolist() == [-1, -1, -1, -1, -1, -1, 0, -1, -1, 3, -1, -1]
  assert missed.tolist() == [7, 99]
  # with a pad id the table does not hold: reported once, where the padding first stands (position 0)
  slots, missed = mref.missing(cache, ids, splits, 3, pad_id=44)
  assert missed.tolist() == [44, 7, 99]
  # a pad id the table holds is found, not reported
  slots, missed = mref.missing(cache, ids, splits, 3, pad_id=30)
  assert slots.tolist() == [4, 4, 4, -1, 4, 4, 0, -1, -1, 3, -1, -1] and missed.tolist() == [7, 99]
  # one id per sample (row_splits None); a row_splits entry outside the ids names no id
  assert mref.missing(cache, ids[:3], None, 2)[1].tolist() == [7]
  assert mref.effective(ids[:3], None, 2)[1].tolist() == [True, False] * 3
  assert mref.effective(ids[:3], np.array([0, 2, 9], np.int32), 4)[1].tolist() == [True, True, False, False,
                                                                                   True, False, False, False]
  assert mref.missing(np.full(4, EMPTY, np.int64), np.zeros(0, np.int64))[1].size == 0
