"""hbk_hash_export_n / hbk_hash_store_rows_n at the C ABI and in Python's argument handling, without a GPU: the
entries exist beside an unchanged version, the structs mirror the header, every refused argument is refused
before any device work with the reason named, HashExport passes through the Saver, and the restatement the GPU
tests compare with (tests/support/hash_export_ref.py) says what the header says."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import HashExport, HashTable, hash_export
from hybridbackend_amd.embedding import hashtable as _ht
from hybridbackend_amd.training.saver import Saver
from tests.support import hash_export_ref as xref

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


def test_symbols_prototypes_version_and_struct_layouts():
  lib = _lib.lib()
  vp, i32 = C.c_void_p, C.c_int32
  for name, args in (('hbk_hash_export_workspace_bytes', [i32, vp, vp]), ('hbk_hash_export_n', [i32, vp, vp, vp]),
                     ('hbk_hash_store_rows_n', [i32, vp, vp])):
    assert hasattr(lib, name)
    assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes == args
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  protos = {
    'hbk_hash_export_workspace_bytes': 'int32_t n_cols, const hbk_hash_export_column_t* cols, size_t* bytes',
    'hbk_hash_export_n': 'int32_t n_cols, const hbk_hash_export_column_t* cols, void* workspace, hbk_stream_t stream',
    'hbk_hash_store_rows_n': 'int32_t n_cols, const hbk_hash_store_column_t* cols, hbk_stream_t stream'}
  for name, want in protos.items():
    proto = re.search(r'int %s\(([^)]*)\);' % name, HEADER).group(1)
    assert re.sub(r'\s+', ' ', proto) == want
  # pointer, int64, two int32; pointer, two int32; eight moves of 32 bytes; two pointers, int64, pointer
  E = _lib.HashExportColumn
  assert C.sizeof(E) == 24 + 16 + 8 * 32 + 32 == 328
  assert [E.keys.offset, E.slab_count.offset, E.slab_size.offset, E.expiring.offset, E.last_seen.offset,
          E.since.offset, E.n_moves.offset, E.moves.offset, E.out_keys.offset, E.out_slots.offset,
          E.out_capacity.offset, E.count.offset] == [0, 8, 16, 20, 24, 32, 36, 40, 296, 304, 312, 320]
  # pointer, two int64, int32 (+4); eight moves
  S = _lib.HashStoreColumn
  assert C.sizeof(S) == 32 + 8 * 32 == 288
  assert [S.slots.offset, S.n.offset, S.dst_rows.offset, S.n_moves.offset, S.moves.offset] == [0, 8, 16, 24, 32]
  assert hb.embedding.hash_export is _ht.hash_export and hb.embedding.HashExport is _ht.HashExport
  # the structs that were there are what they were
  assert C.sizeof(_lib.HashMove) == 32 and C.sizeof(_lib.HashRehashColumn) == 328
  assert C.sizeof(_lib.HashColumn) == 88 and C.sizeof(_lib.HashEvictColumn) == 168


def test_header_declares_the_structs_as_mirrored():
  assert _struct_fields('hbk_hash_export_column_t') == [n for n, _ in _lib.HashExportColumn._fields_]
  assert _struct_fields('hbk_hash_store_column_t') == [n for n, _ in _lib.HashStoreColumn._fields_]
  for word in ('ASCENDING SOURCE-SLOT ORDER', 'last_seen[s] >= since', 'no workgroup waits for another',
               'ALWAYS receives the total', 'nothing is written at positions >=', 'An import is an upsert',
               'keeps its age and count'):
    assert word in HEADER, word


GOOD_MOVE = (fake(4), fake(5), 16, 0, 0)


def _moves(col, moves):
  col.n_moves = len(moves)
  for m, (src, dst, words, src_pitch, dst_pitch) in enumerate(moves):
    mv = col.moves[m]
    mv.src, mv.dst, mv.words, mv.src_pitch, mv.dst_pitch = src, dst, words, src_pitch, dst_pitch


def _ecol(moves=(GOOD_MOVE,), **kw):
  col = _lib.HashExportColumn()
  col.keys, col.slab_count, col.slab_size, col.expiring = fake(0), 8, 16, 1
  col.last_seen, col.since = fake(1), 3
  _moves(col, moves)
  col.out_keys, col.out_slots, col.out_capacity, col.count = fake(2), fake(3), 100, fake(6)
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _scol(moves=(GOOD_MOVE,), **kw):
  col = _lib.HashStoreColumn()
  col.slots, col.n, col.dst_rows = fake(0), 100, 128
  _moves(col, moves)
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _export_refused(cols, workspace, *words):
  lib = _lib.lib()
  arr = (_lib.HashExportColumn * len(cols))(*cols)
  rc = lib.hbk_hash_export_n(len(cols), arr, workspace, None)
  msg = lib.hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_export_n',) + words:
    assert w in msg, msg


BAD_MOVES = [
  (dict(n_moves=-1), ('n_moves',)), (dict(n_moves=9), ('n_moves',)),
  (dict(moves=[GOOD_MOVE, (fake(4), fake(5), 0, 0, 0)]), ('move 1', 'words')),
  (dict(moves=[(fake(4), fake(5), 16, 15, 0)]), ('move 0', 'src_pitch')),
  (dict(moves=[(fake(4), fake(5), 16, 0, 15)]), ('move 0', 'dst_pitch')),
  (dict(moves=[(None, fake(5), 16, 0, 0)]), ('move 0', 'NULL')),
  (dict(moves=[GOOD_MOVE] * 7 + [(fake(4), None, 16, 0, 0)]), ('move 7', 'NULL')),
  (dict(moves=[(fake(4) + 2, fake(5), 16, 0, 0)]), ('move 0', 'aligned')),
  (dict(moves=[(fake(4), fake(4), 16, 0, 0)]), ('move 0', 'same array')),
]


def _apply(make, kw):
  kw = dict(kw)
  moves = kw.pop('moves', None)
  return make(**kw) if moves is None else make(moves=moves, **kw)


@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)), (dict(slab_count=0), ('slab_count',)),
  (dict(slab_count=(1 << 56) + 1), ('slab_count', 'range')),
  (dict(keys=None), ('keys', 'NULL')), (dict(keys=fake(0) + 4), ('keys', 'aligned')),
  (dict(count=None), ('count', 'NULL')),
  (dict(out_keys=None), ('out_keys', 'NULL')),
  (dict(out_capacity=-1), ('out_capacity',)),
  (dict(last_seen=None), ('since', 'last_seen')),
] + BAD_MOVES)
def test_export_refusals(kw, words):
  _export_refused([_ecol(), _apply(_ecol, kw)], fake(7), 'column 1', *words)


def test_export_workspace_counts_of_things_and_nothing_to_do():
  lib = _lib.lib()
  nbytes = C.c_size_t(77)
  # 128 slots: one tile; 259 slots: two; 512: two; 513: three -- 8 bytes each
  cols = [_ecol(), _ecol(slab_count=37, slab_size=7), _ecol(slab_count=8, slab_size=64), _ecol(slab_count=513, slab_size=1)]
  arr = (_lib.HashExportColumn * 4)(*cols)
  assert lib.hbk_hash_export_workspace_bytes(4, arr, C.byref(nbytes)) == _lib.OK and nbytes.value == 8 * 8
  assert lib.hbk_hash_export_workspace_bytes(0, None, C.byref(nbytes)) == _lib.OK and nbytes.value == 0
  assert lib.hbk_hash_export_workspace_bytes(1, arr, None) == _lib.INVALID_ARGUMENT
  assert 'bytes is NULL' in lib.hbk_last_error().decode()
  bad = (_lib.HashExportColumn * 1)(_ecol(slab_size=0))
  assert lib.hbk_hash_export_workspace_bytes(1, bad, C.byref(nbytes)) == _lib.INVALID_ARGUMENT
  assert 'slab_size' in lib.hbk_last_error().decode()
  # the query says a workspace is needed: NULL is refused, and so is one that is not 8-byte aligned
  _export_refused([_ecol()], None, 'workspace', 'NULL')
  _export_refused([_ecol()], fake(7) + 4, 'workspace', 'aligned')
  # a NULL out_keys is fine with nothing to write, a NULL last_seen with nothing to compare: the next check speaks
  _export_refused([_ecol(out_keys=None, out_capacity=0, last_seen=None, since=0)], None, 'workspace')
  _export_refused([_ecol(last_seen=None, since=-1)], None, 'workspace')
  assert lib.hbk_hash_export_n(-1, None, None, None) == _lib.INVALID_ARGUMENT and 'n_cols' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_export_n(1, None, fake(7), None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_export_n(0, None, None, None) == _lib.OK
  assert lib.hbk_hash_export_n(0, arr, None, None) == _lib.OK


@pytest.mark.parametrize('kw,words', [
  (dict(n=-1), ('n must',)), (dict(slots=None), ('slots', 'NULL')), (dict(slots=fake(0) + 4), ('slots', 'aligned')),
  (dict(dst_rows=-1), ('dst_rows',)),
] + BAD_MOVES)
def test_store_refusals_and_nothing_to_do(kw, words):
  lib = _lib.lib()
  arr = (_lib.HashStoreColumn * 2)(_scol(), _apply(_scol, kw))
  rc = lib.hbk_hash_store_rows_n(2, arr, None)
  msg = lib.hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_store_rows_n', 'column 1') + words:
    assert w in msg, msg
  assert lib.hbk_hash_store_rows_n(-1, None, None) == _lib.INVALID_ARGUMENT
  assert lib.hbk_hash_store_rows_n(1, None, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_store_rows_n(0, None, None) == _lib.OK
  # columns with nothing to store launch nothing
  empty = (_lib.HashStoreColumn * 3)(_scol(n=0, slots=None), _scol(moves=()), _scol(dst_rows=0))
  assert lib.hbk_hash_store_rows_n(3, empty, None) == _lib.OK


# ---- Python argument handling ---------------------------------------------------------------------------
def _export_of(n, dim=4, expiring=True, slot_dims=(3,), seed=0):
  rng = np.random.RandomState(seed)
  e = HashExport.empty(n, dim, expiring, slot_dims)
  e.keys = torch.from_numpy(rng.permutation(10 * n)[:n].astype(np.int64) - 3 * n)
  e.rows = torch.from_numpy(rng.randn(n, dim).astype(np.float32))
  if expiring:
    e.last_seen = torch.from_numpy(rng.randint(1, 9, size=n).astype(np.int32))
    e.freq = torch.from_numpy(rng.randint(1, 99, size=n).astype(np.int32))
  e.slots = [torch.from_numpy(rng.randn(n, d).astype(np.float32)) for d in slot_dims]
  e.src_slots = torch.arange(n, dtype=torch.int64) * 2
  e.since = 5
  return e


def test_python_refusals_come_before_any_device_work():
  plain, exp = HashTable(64, 4, 'cpu'), HashTable(64, 4, 'cpu', expiring=True)
  with pytest.raises(_lib.InvalidArgumentError, match='since needs a table built with expiring'):
    plain.export_items(since=3)
  with pytest.raises(_lib.InvalidArgumentError, match='table 1: since'):
    hash_export([exp, plain], sinces=[None, 0])
  with pytest.raises(_lib.InvalidArgumentError, match='expected 2'):
    hash_export([exp, plain], sinces=[None])
  good = torch.zeros(64, 3)
  for bad in ([good.double()], [torch.zeros(63, 3)], [good[:, ::2]], [good] * 5, [(good, 0.0)]):
    with pytest.raises(_lib.InvalidArgumentError, match='slots|companion'):
      exp.export_items(slots=bad)
  with pytest.raises(_lib.HbkError, match='HBM'):                     # a host table: there is no CPU path
    exp.export_items(slots=[good])
  assert hash_export([]) == []
  # import: companions that do not match the export's in number or width
  e = _export_of(10)
  with pytest.raises(_lib.InvalidArgumentError, match='carries 1 companion tensors, slots names 0'):
    exp.import_items(e)
  with pytest.raises(_lib.InvalidArgumentError, match='carries 1 companion tensors, slots names 2'):
    exp.import_items(e, slots=[good, good.clone()])
  with pytest.raises(_lib.InvalidArgumentError, match=r'exp.slots\[0\] must be fp32 \[10, 5\]'):
    exp.import_items(e, slots=[torch.zeros(64, 5)])
  with pytest.raises(_lib.InvalidArgumentError, match='exp.rows'):
    HashTable(64, 8, 'cpu').import_items(_export_of(10, slot_dims=()))
  with pytest.raises(_lib.InvalidArgumentError, match='world and rank'):
    exp.import_items(e, slots=[good], world=2)
  with pytest.raises(_lib.InvalidArgumentError, match='HashExport'):
    exp.import_items((e.keys, e.rows))
  # duplicate keys are refused (after the ownership mask: the duplicate is even, rank 1 of 2 never sees it)
  e.keys[7] = 2 * (int(e.keys[2]) // 2)
  e.keys[2] = e.keys[7]
  for kw in (dict(), dict(world=2, rank=0)):
    with pytest.raises(_lib.InvalidArgumentError, match='not distinct'):
      exp.import_items(e, slots=[good], **kw)
  with pytest.raises(_lib.HbkError, match='HBM'):                     # distinct for rank 1: on to the device
    exp.import_items(e, slots=[good], world=2, rank=1)
  with pytest.raises(_lib.HbkError, match='HBM'):
    exp.import_items(e, slots=[good], assume_distinct=True)
  # nothing owned: nothing to do, no device needed
  assert exp.import_items(_export_of(0), slots=[good]).numel() == 0
  assert int(exp.counts[0]) == 0 and bool((exp.keys == _ht.EMPTY_KEY).all())


@pytest.mark.parametrize('expiring,slot_dims', [(True, (3, 16)), (False, ())])
def test_export_round_trips_through_the_saver(tmp_path, expiring, slot_dims):
  e = _export_of(37, 5, expiring, slot_dims, seed=3)
  saved = e.variables('emb/t0')
  assert set(saved) == {'emb/t0/items/' + k for k in ['keys', 'rows', 'since', 'src_slots'] +
                        (['last_seen', 'freq'] if expiring else []) + [f'slot{k}' for k in range(len(slot_dims))]}
  prefix = str(tmp_path / 'ckpt')
  Saver().save(prefix, saved)
  into = HashExport.empty(37, 5, expiring, slot_dims).variables('emb/t0')
  Saver().restore(prefix, into)
  back = HashExport.from_variables('emb/t0', into)
  assert back.since == 5 and len(back) == 37 and len(back.slots) == len(slot_dims)
  assert (back.last_seen is None) == (not expiring) and (back.freq is None) == (not expiring)
  for name in ['keys', 'rows', 'src_slots'] + (['last_seen', 'freq'] if expiring else []):
    a, b = getattr(e, name), getattr(back, name)
    assert a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes(), name
  for a, b in zip(e.slots, back.slots):
    assert a.numpy().tobytes() == b.numpy().tobytes()
  with pytest.raises(_lib.InvalidArgumentError, match='keys and'):
    HashExport.from_variables('emb/t1', into)


def test_cat_concatenates_in_order_and_keeps_metadata_only_when_all_have_it():
  a, b = _export_of(5, seed=1), _export_of(7, seed=2)
  b.since = 2
  c = HashExport.cat([a, b])
  assert len(c) == 12 and c.since == 2
  for name in ('keys', 'rows', 'last_seen', 'freq', 'src_slots'):
    assert torch.equal(getattr(c, name), torch.cat([getattr(a, name), getattr(b, name)]))
  assert torch.equal(c.slots[0], torch.cat([a.slots[0], b.slots[0]]))
  b.last_seen = None
  c = HashExport.cat([a, b])
  assert c.last_seen is None and c.freq is None and len(c) == 12
  with pytest.raises(_lib.InvalidArgumentError, match='companion'):
    HashExport.cat([a, _export_of(3, slot_dims=())])
  with pytest.raises(_lib.InvalidArgumentError, match='no exports'):
    HashExport.cat([])


# ---- the restatement -----------------------------------------------------------------------------------
def test_restatement_selects_orders_and_truncates_as_the_header_says():
  keys = np.array([5, xref.EMPTY, xref.TOMBSTONE, -9, 7, xref.EMPTY, 11], np.int64)
  seen = np.array([3, 0, 0, 2, 5, 0, 3], np.int32)
  rows = np.arange(14, dtype=np.float32).reshape(7, 2)
  count, k, s, (r, ls) = xref.export(keys, True, [rows, seen])
  assert count == 4 and s.tolist() == [0, 3, 4, 6] and k.tolist() == [5, -9, 7, 11]
  assert r.tolist() == rows[[0, 3, 4, 6]].tolist() and ls.tolist() == [3, 2, 5, 3]
  assert xref.export(keys, False, [])[2].tolist() == [0, 2, 3, 4, 6]          # a plain table: TOMBSTONE is a key
  assert xref.select(keys, True, seen, 3).tolist() == [0, 4, 6]               # step 3 is in, step 2 is out
  assert xref.select(keys, True, seen, 6).size == 0
  assert xref.select(keys, True, seen, 0).tolist() == xref.select(keys, True, seen, -1).tolist() == [0, 3, 4, 6]
  count, k, s, _ = xref.export(keys, True, [], out_capacity=3)
  assert count == 4 and s.tolist() == [0, 3, 4]
  state = xref.as_map(k, rows[s])
  state = xref.upsert(state, np.array([7, 13], np.int64), np.array([[1, 1], [2, 2]], np.float32))
  assert sorted(state) == [-9, 5, 7, 13] and state[7] == (np.array([1, 1], np.float32).tobytes(),)
