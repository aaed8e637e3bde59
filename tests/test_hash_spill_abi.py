"""Spilling to a host tier (hbk_hash_evict_to_select_n, hbk_hash_spill_n, HashSpillStore, spill_to / fault_in) at
the C ABI and in Python's argument handling, without a GPU: the three entries exist and are declared, the struct
mirrors the header, every refused argument is refused before any device work with the column and the field named,
the host store upserts, takes and peeks bit for bit, and the numpy restatement the GPU tests compare with
(tests/support/hash_spill_ref.py) agrees with the eviction's."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import HashExport, HashSpillStore, HashTable
from hybridbackend_amd.embedding import hashtable as _ht
from tests.support import hash_evict_to_ref as tref
from tests.support import hash_spill_ref as sref

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


# ---- ABI --------------------------------------------------------------------------------------------------
def test_symbols_declarations_and_struct_layout():
  lib = _lib.lib()
  for name in ('hbk_hash_evict_to_select_n', 'hbk_hash_spill_n', 'hbk_hash_spill_workspace_bytes'):
    assert hasattr(lib, name), name
  assert re.search(r'int hbk_hash_evict_to_select_n\(int32_t n_cols, const hbk_hash_evict_to_column_t\* cols, '
                   r'void\* workspace,\s+size_t workspace_bytes, hbk_stream_t stream\);', HEADER)
  assert ('int hbk_hash_spill_workspace_bytes(int32_t n_cols, const hbk_hash_spill_column_t* cols, size_t* bytes);'
          in HEADER)
  assert ('int hbk_hash_spill_n(int32_t n_cols, const hbk_hash_spill_column_t* cols, void* workspace, '
          'hbk_stream_t stream);' in HEADER)
  assert lib.hbk_hash_evict_to_select_n.argtypes == lib.hbk_hash_evict_to_n.argtypes
  assert lib.hbk_hash_spill_n.argtypes == [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  T = _lib.HashSpillColumn
  names = [n for n, _ in T._fields_]
  assert _struct_fields('hbk_hash_spill_column_t') == names
  for needed in ('keys_cache', 'slab_count', 'slab_size', 'exp', 'selection', 'keep_freq', 'n_moves', 'moves',
                 'n_fills', 'fills', 'out_keys', 'out_slots', 'out_capacity', 'count', 'n_evicted'):
    assert needed in names, needed
  # 24 geometry + 32 expiry + 8 selection + 8 (keep_freq, n_moves) + 8 x 32 moves (28 padded to the pointers)
  # + 4 n_fills + 4 x 20 fills (pointer-aligned: 8 + 96) + 5 x 8 outputs
  assert C.sizeof(_lib.HashMove) == 32 and C.sizeof(_lib.HashFill) == 24
  assert C.sizeof(T) == 24 + 32 + 8 + 8 + 8 * 32 + 8 + 4 * 24 + 5 * 8 == 472
  assert [T.exp.offset, T.selection.offset, T.keep_freq.offset, T.moves.offset, T.n_fills.offset, T.fills.offset,
          T.out_keys.offset, T.n_evicted.offset] == [24, 56, 64, 72, 328, 336, 432, 464]
  # the existing structs are what they were
  assert C.sizeof(_lib.HashEvictToColumn) == 176 and C.sizeof(_lib.HashExportColumn) == 328
  for fn in ('hash_evict_to_select', 'hash_spill', 'HashSpillStore'):
    assert getattr(hb.embedding, fn) is getattr(_ht, fn)
  for word in ('n_selected', 'ALL OR NOTHING', 'READ FROM DEVICE MEMORY', 'no host read anywhere', 'selection[1] > 0'):
    assert word in HEADER, word


GOOD_FILL = (fake(9), 0, 16, 0.1)
GOOD_MOVE = (fake(20), fake(21), 16, 0, 0)


def _col(fills=(), moves=(GOOD_MOVE,), **kw):
  col = _lib.HashSpillColumn()
  col.keys_cache, col.slab_count, col.slab_size = fake(0), 8, 16
  col.exp.last_seen, col.exp.freq, col.exp.step, col.exp.stats = fake(5), fake(6), None, fake(8)
  col.selection, col.keep_freq = fake(10), 0
  col.out_keys, col.out_slots, col.out_capacity = fake(12), fake(13), 7
  col.count, col.n_evicted = fake(14), fake(15)
  col.n_fills = len(fills)
  for f, (base, pitch, dim, value) in enumerate(fills):
    col.fills[f].base, col.fills[f].pitch, col.fills[f].dim, col.fills[f].value = base, pitch, dim, value
  col.n_moves = len(moves)
  for m, (src, dst, words, sp, dp) in enumerate(moves):
    mv = col.moves[m]
    mv.src, mv.dst, mv.words, mv.src_pitch, mv.dst_pitch = src, dst, words, sp, dp
  for k, v in kw.items():
    if k in ('last_seen', 'freq', 'step', 'stats'):
      setattr(col.exp, k, v)
    else:
      setattr(col, k, v)
  return col


def _refused(cols, workspace, *words):
  lib = _lib.lib()
  arr = (_lib.HashSpillColumn * len(cols))(*cols)
  rc = lib.hbk_hash_spill_n(len(cols), arr, workspace, None)
  msg = lib.hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_spill_n',) + words:
    assert w in msg, msg


@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)),
  (dict(slab_count=0), ('slab_count',)), (dict(keys_cache=None), ('keys_cache',)),
  (dict(keys_cache=fake(0) + 4), ('keys_cache', 'aligned')),
  (dict(slab_count=1 << 25, slab_size=64), ('2^31', 'slab_count')),          # exactly 2^31 slots
  (dict(slab_count=(1 << 31) + 1, slab_size=1), ('2^31', 'slab_count')),
  (dict(last_seen=None), ('last_seen', 'NULL')), (dict(freq=None), ('freq', 'NULL')),
  (dict(selection=None), ('selection', 'NULL')), (dict(count=None), ('count', 'NULL')),
  (dict(keep_freq=-1), ('keep_freq',)),
  (dict(n_moves=-1), ('n_moves',)), (dict(n_moves=9), ('n_moves',)),
  (dict(moves=[GOOD_MOVE, (fake(20), fake(21), 0, 0, 0)]), ('move 1', 'words')),
  (dict(moves=[(fake(20), fake(21), 16, 15, 0)]), ('move 0', 'src_pitch')),
  (dict(moves=[(fake(20), fake(21), 16, 0, 15)]), ('move 0', 'dst_pitch')),
  (dict(moves=[(None, fake(21), 16, 0, 0)]), ('move 0', 'NULL')),
  (dict(moves=[(fake(20), fake(21) + 2, 16, 0, 0)]), ('move 0', 'aligned')),
  (dict(moves=[(fake(20), fake(20), 16, 0, 0)]), ('move 0', 'same')),
  (dict(n_fills=-1), ('n_fills',)), (dict(n_fills=5), ('n_fills',)),
  (dict(fills=[GOOD_FILL, (None, 0, 16, 0.0)]), ('fill 1', 'base')),
  (dict(fills=[(fake(9), 0, 0, 0.0)]), ('fill 0', 'dim')),
  (dict(fills=[(fake(9), 15, 16, 0.0)]), ('fill 0', 'pitch')),
  (dict(fills=[(fake(9), 16, 16, float('nan'))]), ('fill 0', 'value')),
  (dict(out_capacity=-1), ('out_capacity',)),
  (dict(out_keys=None), ('out_keys', 'NULL')),
])
def test_spill_refusals_name_the_column_and_the_field(kw, words):
  _refused([_col(), _col(**kw)], fake(11), 'column 1', *words)


def test_spill_workspace_and_counts_of_things():
  lib = _lib.lib()
  nbytes = C.c_size_t(99)
  cols = (_lib.HashSpillColumn * 2)(_col(), _col(slab_count=37, slab_size=3, stats=None, out_slots=None,
                                                 n_evicted=None, out_keys=None, out_capacity=0))
  assert lib.hbk_hash_spill_workspace_bytes(2, cols, C.byref(nbytes)) == _lib.OK
  assert nbytes.value == 8 * (1 + 1)                                       # 8 bytes per 256 slots, per table
  _refused(list(cols), None, 'workspace', 'NULL')
  _refused(list(cols), fake(11) + 4, 'workspace', 'aligned')
  assert lib.hbk_hash_spill_workspace_bytes(1, cols, None) == _lib.INVALID_ARGUMENT
  bad = (_lib.HashSpillColumn * 1)(_col(slab_size=0))
  assert lib.hbk_hash_spill_workspace_bytes(1, bad, C.byref(nbytes)) == _lib.INVALID_ARGUMENT
  assert 'slab_size' in lib.hbk_last_error().decode() and nbytes.value == 0
  assert lib.hbk_hash_spill_n(-1, None, None, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_spill_n(1, None, fake(11), None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_spill_n(0, None, None, None) == _lib.OK              # nothing to do, no workspace needed
  assert lib.hbk_hash_spill_workspace_bytes(0, None, C.byref(nbytes)) == _lib.OK and nbytes.value == 0


def _select_col(**kw):
  col = _lib.HashEvictToColumn()
  col.keys_cache, col.slab_count, col.slab_size = fake(0), 8, 16
  col.exp.last_seen, col.exp.freq, col.exp.step, col.exp.stats = fake(5), fake(6), None, None
  col.max_size, col.keep_freq, col.report = 10, 0, fake(10)
  fills = kw.pop('fills', ())
  col.n_fills = len(fills)
  for f, (base, pitch, dim, value) in enumerate(fills):
    col.fills[f].base, col.fills[f].pitch, col.fills[f].dim, col.fills[f].value = base, pitch, dim, value
  for k, v in kw.items():
    if k in ('last_seen', 'freq'):
      setattr(col.exp, k, v)
    else:
      setattr(col, k, v)
  return col


@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)),
  (dict(slab_count=0), ('slab_count',)), (dict(keys_cache=None), ('keys_cache',)),
  (dict(last_seen=None), ('last_seen', 'NULL')), (dict(freq=None), ('freq', 'NULL')),
  (dict(max_size=-1), ('max_size',)), (dict(keep_freq=-1), ('keep_freq',)),
  (dict(n_fills=5), ('n_fills',)),
  (dict(fills=[GOOD_FILL, (None, 0, 16, 0.0)]), ('fill 1', 'base')),         # checked, though not used
  (dict(slab_count=1 << 25, slab_size=64), ('2^31', 'slab_count')),
  (dict(report=None), ('report', 'NULL')),                                  # required here
])
def test_select_refusals_carry_its_own_name(kw, words):
  lib = _lib.lib()
  nbytes = lib.hbk_hash_evict_to_workspace_bytes(2)
  arr = (_lib.HashEvictToColumn * 2)(_select_col(), _select_col(**kw))
  rc = lib.hbk_hash_evict_to_select_n(2, arr, fake(11), nbytes, None)
  msg = lib.hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_evict_to_select_n', 'column 1') + words:
    assert w in msg, msg


def test_select_workspace_and_counts_of_things():
  lib = _lib.lib()
  nbytes = lib.hbk_hash_evict_to_workspace_bytes(1)
  arr = (_lib.HashEvictToColumn * 1)(_select_col())
  for ws, size, word in ((None, nbytes, 'NULL'), (fake(11), nbytes - 1, 'too small'), (fake(11) + 2, nbytes, 'aligned')):
    assert lib.hbk_hash_evict_to_select_n(1, arr, ws, size, None) == _lib.INVALID_ARGUMENT
    msg = lib.hbk_last_error().decode()
    assert 'hash_evict_to_select_n' in msg and 'workspace' in msg and word in msg, msg
  assert lib.hbk_hash_evict_to_select_n(0, None, None, 0, None) == _lib.OK
  # the evicting entry still takes a NULL report
  arr[0].report = None
  assert lib.hbk_hash_evict_to_n(1, arr, None, nbytes, None) == _lib.INVALID_ARGUMENT
  assert 'workspace is NULL' in lib.hbk_last_error().decode()


# ---- Python refusals ----------------------------------------------------------------------------------------
def test_python_refusals():
  plain = HashTable(64, 4, 'cpu')
  t = HashTable(64, 4, 'cpu', expiring=True)
  store = HashSpillStore(4)
  ids = torch.arange(5, dtype=torch.int64)
  for call in (lambda: plain.spill_to(3), lambda: plain.spill_to(3, store), lambda: plain.fault_in(ids, store),
               lambda: hb.embedding.hash_spill([t, plain], 3), lambda: hb.embedding.hash_evict_to_select([plain], 3),
               lambda: plain.maybe_evict(spill=store)):
    with pytest.raises(_lib.InvalidArgumentError, match='expiring=True'):
      call()
  with pytest.raises(_lib.InvalidArgumentError, match='>= 0'):
    t.spill_to(-1)
  with pytest.raises(_lib.InvalidArgumentError, match='>= 0'):
    t.spill_to(3, keep_freq=-2)
  with pytest.raises(_lib.InvalidArgumentError, match='max_sizes'):
    hb.embedding.hash_spill([t], [3, 4])
  with pytest.raises(_lib.InvalidArgumentError, match='max_sizes'):
    hb.embedding.hash_evict_to_select([t], [3, 4])
  with pytest.raises(_lib.InvalidArgumentError, match='lists of companion'):
    hb.embedding.hash_spill([t], 3, slots=[[], []])
  with pytest.raises(_lib.InvalidArgumentError, match='reports'):
    hb.embedding.hash_evict_to_select([t], 3, reports=[torch.zeros(4, dtype=torch.int64)])
  good = torch.zeros(64, 4)
  for bad in ([good], [(good.double(), 0.0)], [(torch.zeros(63, 4), 0.0)], [(good, float('nan'))], [(good, 0.0)] * 5):
    with pytest.raises(_lib.InvalidArgumentError, match='slots|companion'):
      t.spill_to(3, slots=bad)
  # a store of the wrong dim or slot widths: refused before anything could leave the table
  for wrong, slots in ((HashSpillStore(5), ()), (HashSpillStore(4, [4]), ()), (HashSpillStore(4), [(good, 0.0)]),
                       (HashSpillStore(4, [3]), [(good, 0.0)]), (object(), ())):
    with pytest.raises(_lib.InvalidArgumentError, match='store'):
      t.spill_to(3, wrong, slots=slots)
    with pytest.raises(_lib.InvalidArgumentError, match='store'):
      t.fault_in(ids, wrong, slots=[x for x, _ in slots])
    with pytest.raises(_lib.InvalidArgumentError, match='store'):
      t.maybe_evict(spill=wrong, slots=slots)
  with pytest.raises(_lib.InvalidArgumentError, match='spill stores'):
    _ht.evict_tables(None, [t], 0.75, 0.5, 0, None, [store, store])
  assert t.maybe_evict(spill=store) is None                                # an empty table: below any max_load
  assert _ht.evict_tables(None, [t], 0.75, 0.5, 0, None, store) == [None]
  with pytest.raises(_lib.HbkError, match='HBM'):                          # a host table: there is no CPU path
    t.spill_to(3)
  with pytest.raises(_lib.HbkError, match='HBM'):
    t.spill_to(3, store)
  with pytest.raises(_lib.HbkError, match='HBM'):
    hb.embedding.hash_evict_to_select([t], 3)
  with pytest.raises(_lib.HbkError, match='HBM'):
    t.fault_in(ids, store)
  assert hb.embedding.hash_spill([], 3) == [] and hb.embedding.hash_evict_to_select([], 3) == []
  assert callable(hb.embedding.HashGroupLookup.fault_in)
  with pytest.raises(_lib.InvalidArgumentError, match='>= 1'):
    HashSpillStore(0)


# ---- the host store -------------------------------------------------------------------------------------------
def _export(rng, keys, dim=3, slot_dims=(2, 5)):
  n = len(keys)
  return HashExport(torch.tensor(keys, dtype=torch.int64), torch.from_numpy(rng.rand(n, dim).astype(np.float32)),
                    torch.from_numpy(rng.randint(-2 ** 31, 2 ** 31 - 1, size=n).astype(np.int32)),
                    torch.from_numpy(rng.randint(1, 100, size=n).astype(np.int32)),
                    [torch.from_numpy(rng.rand(n, d).astype(np.float32)) for d in slot_dims])


def _rows_of(exp, keys):
  """{key: every payload array's row, as bytes}"""
  arrays = [exp.rows, exp.last_seen, exp.freq] + list(exp.slots)
  return {int(k): tuple(a[i].numpy().tobytes() for a in arrays) for i, k in enumerate(exp.keys.tolist()) if k in keys}


def test_store_put_take_peek_upsert():
  rng = np.random.RandomState(3)
  store = HashSpillStore(3, (2, 5), pin_memory=False)
  assert len(store) == 0 and store.keys().numel() == 0
  empty = store.take(torch.tensor([1, 2, 3], dtype=torch.int64))
  assert len(empty) == 0 and tuple(empty.rows.shape) == (0, 3) and [tuple(x.shape) for x in empty.slots] == [(0, 2), (0, 5)]
  store.put(_export(rng, []))
  assert len(store) == 0
  first = _export(rng, [40, -7, 2 ** 62, 13, -2 ** 63 + 5])
  store.put(first)
  assert len(store) == 5 and store.keys().tolist() == sorted(first.keys.tolist())
  # peek: ascending key order, duplicates once, absent keys simply not returned, nothing removed
  got = store.peek(torch.tensor([13, 99, 40, 13, -7], dtype=torch.int64))
  assert got.keys.tolist() == [-7, 13, 40] and len(store) == 5
  assert _rows_of(got, {-7, 13, 40}) == _rows_of(first, {-7, 13, 40})     # bit for bit
  assert got.src_slots is None and got.last_seen.dtype == torch.int32
  # a later put wins, key by key
  second = _export(rng, [13, 77, 40])
  store.put(second)
  assert len(store) == 6
  got = store.take(torch.tensor([77, 40, 13, 2 ** 62, 5], dtype=torch.int64))
  assert got.keys.tolist() == [13, 40, 77, 2 ** 62]
  want = {**_rows_of(first, {2 ** 62}), **_rows_of(second, {13, 40, 77})}
  assert _rows_of(got, set(want)) == want
  # take removed them; the rest is untouched
  assert store.keys().tolist() == [-2 ** 63 + 5, -7] and len(store) == 2
  assert len(store.take(torch.tensor([13, 40], dtype=torch.int64))) == 0
  rest = store.peek(store.keys())
  assert _rows_of(rest, {-7, -2 ** 63 + 5}) == _rows_of(first, {-7, -2 ** 63 + 5})
  # of two equal keys of one export the later stays
  twice = _export(rng, [5, 5])
  store.put(twice)
  got = store.peek(torch.tensor([5], dtype=torch.int64))
  assert got.rows[0].tolist() == twice.rows[1].tolist() and len(store) == 3
  store.clear()
  assert len(store) == 0 and len(store.peek(torch.tensor([5], dtype=torch.int64))) == 0


def test_store_refuses_what_does_not_match():
  rng = np.random.RandomState(4)
  store = HashSpillStore(3, (2, 5), pin_memory=False)
  good = _export(rng, [1, 2])
  for bad, word in ((_export(rng, [1, 2], dim=4), 'rows'), (_export(rng, [1, 2], slot_dims=(2,)), 'companion'),
                    (_export(rng, [1, 2], slot_dims=(2, 4)), r'slots\[1\]'),
                    (HashExport(good.keys, good.rows, None, None, good.slots), 'last_seen'),
                    (HashExport(good.keys, good.rows, good.last_seen.long(), good.freq, good.slots), 'last_seen'),
                    (HashExport(good.keys.int(), good.rows, good.last_seen, good.freq, good.slots), 'keys'),
                    ((good.keys, good.rows), 'HashExport')):
    with pytest.raises(_lib.InvalidArgumentError, match=word):
      store.put(bad)
  assert len(store) == 0
  with pytest.raises(_lib.InvalidArgumentError, match='int64'):
    store.take(torch.tensor([1.0]))


def test_store_round_trip_through_variables():
  rng = np.random.RandomState(5)
  store = HashSpillStore(3, (2, 5), pin_memory=False)
  exp = _export(rng, list(range(100, 0, -3)))
  store.put(exp)
  d = store.variables('emb0/spill')
  assert 'emb0/spill/items/keys' in d and 'emb0/spill/items/slot1' in d and 'emb0/spill/items/last_seen' in d
  again = HashSpillStore.from_variables('emb0/spill', {k: v.clone() for k, v in d.items()}, pin_memory=False)
  assert again.dim == 3 and again.slot_dims == (2, 5) and again.keys().tolist() == store.keys().tolist()
  keys = set(exp.keys.tolist())
  assert _rows_of(again.take(again.keys()), keys) == _rows_of(exp, keys) and len(again) == 0
  none = HashSpillStore.from_variables('x', HashSpillStore(2, (), pin_memory=False).variables('x'), pin_memory=False)
  assert len(none) == 0 and none.dim == 2 and none.slot_dims == ()


# ---- the restatement's own properties -------------------------------------------------------------------
def _random_table(rng, cap, steps):
  cache = np.full(cap, tref.EMPTY, np.int64)
  kind = rng.randint(0, 10, size=cap)
  cache[kind < 6] = rng.randint(1, 2 ** 40, size=int((kind < 6).sum()))
  cache[kind == 6] = tref.TOMBSTONE
  last_seen = rng.randint(steps[0], steps[1], size=cap).astype(np.int32)
  freq = rng.randint(1, 6, size=cap).astype(np.int32)
  return cache, last_seen, freq


@pytest.mark.parametrize('steps', [(1, 7), (-2 ** 31, 2 ** 31 - 1), (-3, 1)])
@pytest.mark.parametrize('keep_freq', [0, 3])
def test_reference_selects_what_the_eviction_evicts(steps, keep_freq):
  rng = np.random.RandomState(21 + keep_freq)
  for trial in range(20):
    cache, last_seen, freq = _random_table(rng, 200, steps)
    live = int(((cache != tref.EMPTY) & (cache != tref.TOMBSTONE)).sum())
    max_size = int(rng.randint(0, live + 3))
    comp = rng.rand(200, 6).astype(np.float32)
    rows = rng.rand(200, 4).astype(np.float32)
    before = [x.copy() for x in (cache, last_seen, freq, comp)]
    sel = sref.select(cache, last_seen, freq, max_size, keep_freq)
    moves = [(rows, 4), (last_seen, 1), (freq, 1), (comp, 5)]
    export, after, n_evicted, count = sref.spill(cache, last_seen, freq, sel, keep_freq, moves, [(comp, 5, 0.25)])
    for x, y in zip((cache, last_seen, freq, comp), before):               # the restatement modifies nothing
      np.testing.assert_array_equal(x, y)
    e = [x.copy() for x in before]
    report, mask = tref.evict_to(e[0], e[1], e[2], max_size, keep_freq, [(e[3], 5, 0.25)])
    assert sel.tolist() == report.tolist() and sel[3] == mask.sum() == count == n_evicted
    assert (need_le_0 := sel[1] <= 0) == (sel[2] == 0 and sel[1] <= 0) and (not need_le_0 or count == 0)
    np.testing.assert_array_equal(sref.selected_mask(cache, last_seen, freq, sel, keep_freq), mask)
    # the table afterwards is the eviction's
    for x, y in zip((after['cache'], after['last_seen'], after['freq'], after['companions'][0]), e):
      np.testing.assert_array_equal(x, y)
    # the export is before[mask], in ascending slot order
    where = np.flatnonzero(mask)
    np.testing.assert_array_equal(export['src_slots'], where)
    np.testing.assert_array_equal(export['keys'], before[0][where])
    for got, want in zip(export['moves'], (rows[where], before[1][where], before[2][where], before[3][where, :5])):
      np.testing.assert_array_equal(got, want)
    if count == 0:
      continue
    # one row short: the count is still the total, the export is cut, and nothing changes
    export, after, n_evicted, total = sref.spill(cache, last_seen, freq, sel, keep_freq, moves, [(comp, 5, 0.25)],
                                                 out_capacity=count - 1)
    assert total == count and n_evicted == 0 and export['keys'].size == count - 1
    np.testing.assert_array_equal(export['src_slots'], where[:-1])
    for x, y in zip((after['cache'], after['last_seen'], after['freq'], after['companions'][0]), before):
      np.testing.assert_array_equal(x, y)


def test_reference_needs_the_need_and_not_only_the_cut():
  """need <= 0 reports cut = 0, and last_seen <= 0 is an ordinary value: a predicate on the cut alone would evict."""
  cache = np.arange(1, 9, dtype=np.int64)
  last_seen = np.array([-5, -1, 0, 0, 3, 4, -2 ** 31, 7], np.int32)
  freq = np.ones(8, np.int32)
  sel = sref.select(cache, last_seen, freq, 8)
  assert sel.tolist() == [8, 0, 0, 0] and (last_seen <= sel[2]).sum() == 5
  assert not sref.selected_mask(cache, last_seen, freq, sel).any()
  _, after, n_evicted, count = sref.spill(cache, last_seen, freq, sel)
  assert (n_evicted, count) == (0, 0) and (after['cache'] == cache).all()
  assert sref.select(cache, last_seen, freq, 7).tolist() == [8, 1, -2 ** 31, 1]
