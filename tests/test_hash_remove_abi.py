"""Removal by id (hbk_hash_remove_n, HashTable.remove, removal tracking, HashExport.removed) at the C ABI and in
Python's argument handling, without a GPU: the entry exists and is declared, the struct mirrors the header, every
refused argument is refused before any device work with the column and the field named, the export's new field
round-trips, the host store discards, and the numpy restatement the GPU tests compare with
(tests/support/hash_remove_ref.py) agrees with the eviction's."""
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
from tests.support import hash_expiry_ref as xref
from tests.support import hash_remove_ref as rref

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
def test_symbol_declaration_and_struct_layout():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_hash_remove_n')
  assert ('int hbk_hash_remove_n(int32_t n_cols, const hbk_hash_remove_column_t* cols, hbk_stream_t stream);'
          in HEADER)
  assert lib.hbk_hash_remove_n.argtypes == [C.c_int32, C.c_void_p, C.c_void_p]
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  T = _lib.HashRemoveColumn
  names = [n for n, _ in T._fields_]
  assert _struct_fields('hbk_hash_remove_column_t') == names
  assert names == ['keys_cache', 'slab_count', 'slab_size', 'exp', 'keys', 'n_keys', 'slots', 'n_removed', 'n_fills',
                   'fills']
  # 24 geometry + 32 expiry + 8 keys + 8 n_keys + 8 slots + 8 n_removed + 4 n_fills (padded to the pointers: 8)
  # + 4 x 24 fills
  assert C.sizeof(T) == 24 + 32 + 4 * 8 + 8 + 4 * 24 == 192
  assert [getattr(T, n).offset for n in names] == [0, 8, 16, 24, 56, 64, 72, 80, 88, 96]
  assert [getattr(T, n).size for n in names] == [8, 8, 4, 32, 8, 8, 8, 8, 4, 96]
  # the existing structs are what they were
  sizes = {'HashColumn': 88, 'HashExpiry': 32, 'HashAdmission': 40, 'HashFill': 24, 'HashMove': 32,
           'HashEvictColumn': 168, 'HashEvictToColumn': 176, 'HashRehashColumn': 328, 'HashExportColumn': 328,
           'HashStoreColumn': 288, 'HashSpillColumn': 472, 'ShardedHash': 128}
  for name, size in sizes.items():
    assert C.sizeof(getattr(_lib, name)) == size, name
  assert hb.embedding.hash_remove is _ht.hash_remove
  for cls in (hb.embedding.HashGroupLookup, hb.embedding.HashSequenceLookup, hb.embedding.ShardedHashGroupLookup,
              HashTable):
    assert callable(cls.remove)
  for word in ('BEFORE the call', 'never\n *     EMPTY', 'DISTINCT ids removed', 'kernel boundary',
               'functions of the inputs alone', 'step is not'):
    assert word in HEADER, word


GOOD_FILL = (fake(9), 0, 16, 0.1)


def _col(fills=(), **kw):
  col = _lib.HashRemoveColumn()
  col.keys_cache, col.slab_count, col.slab_size = fake(0), 8, 16
  col.exp.last_seen, col.exp.freq, col.exp.step, col.exp.stats = fake(5), fake(6), None, fake(8)
  col.keys, col.n_keys, col.slots, col.n_removed = fake(1), 0, fake(2), None
  col.n_fills = len(fills)
  for f, (base, pitch, dim, value) in enumerate(fills):
    col.fills[f].base, col.fills[f].pitch, col.fills[f].dim, col.fills[f].value = base, pitch, dim, value
  for k, v in kw.items():
    if k in ('last_seen', 'freq', 'step', 'stats'):
      setattr(col.exp, k, v)
    else:
      setattr(col, k, v)
  return col


@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)),
  (dict(slab_count=0), ('slab_count',)), (dict(slab_count=1 << 60), ('slab_count',)),
  (dict(keys_cache=None), ('keys_cache', 'NULL')),
  (dict(keys_cache=fake(0) + 4), ('keys_cache', 'aligned')),
  (dict(slab_count=1 << 25, slab_size=64), ('2^31', 'slab_count')),          # exactly 2^31 slots
  (dict(slab_count=(1 << 31) + 1, slab_size=1), ('2^31', 'slab_count')),
  (dict(last_seen=None), ('last_seen', 'NULL')), (dict(freq=None), ('freq', 'NULL')),
  (dict(n_keys=5, keys=None), ('keys', 'NULL')), (dict(n_keys=5, slots=None), ('slots', 'NULL')),
  (dict(n_keys=-1), ('n_keys',)), (dict(n_keys=1 << 31), ('n_keys', '2^31')),
  (dict(n_fills=-1), ('n_fills',)), (dict(n_fills=5), ('n_fills',)),
  (dict(fills=[GOOD_FILL, (None, 0, 16, 0.0)]), ('fill 1', 'base')),
  (dict(fills=[(fake(9), 0, 0, 0.0)]), ('fill 0', 'dim')),
  (dict(fills=[(fake(9), 15, 16, 0.0)]), ('fill 0', 'pitch')),
  (dict(fills=[(fake(9), 16, 16, float('nan'))]), ('fill 0', 'value')),
  (dict(fills=[(fake(9), 16, 16, float('inf'))]), ('fill 0', 'value')),
])
def test_refusals_name_the_column_and_the_field(kw, words):
  """Column 0 is fine and has no keys; column 1 carries the fault, with keys waiting at fake addresses: nothing may
  be launched."""
  lib = _lib.lib()
  bad = dict(n_keys=7)
  bad.update(kw)
  arr = (_lib.HashRemoveColumn * 2)(_col(), _col(**bad))
  rc = lib.hbk_hash_remove_n(2, arr, None)
  msg = lib.hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_remove_n', 'column 1') + words:
    assert w in msg, msg


def test_a_find_grid_too_large_is_refused_before_the_first_group_runs():
  """33 columns of 2^31 - 1 ids at slab 64: the second launch group is fine, the first needs 32 x (2^26 + 1) find
  tiles.  Refused at the column that crosses 2^31, before anything is launched on the fake addresses."""
  lib = _lib.lib()
  cols = [_col(n_keys=(1 << 31) - 1, slab_size=64) for _ in range(33)]
  arr = (_lib.HashRemoveColumn * 33)(*cols)
  assert lib.hbk_hash_remove_n(33, arr, None) == _lib.INVALID_ARGUMENT
  msg = lib.hbk_last_error().decode()
  for w in ('hash_remove_n', 'column 31', 'n_keys', '2^31', 'tiles'):
    assert w in msg, msg


def test_counts_of_things_and_what_is_not_refused():
  lib = _lib.lib()
  assert lib.hbk_hash_remove_n(-1, None, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_remove_n(1, None, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_remove_n(0, None, None) == _lib.OK
  # columns without keys: checked, nothing launched -- NULL keys / slots / step / stats / n_removed are fine there
  arr = (_lib.HashRemoveColumn * 2)(_col(keys=None, slots=None, stats=None), _col(fills=[GOOD_FILL] * 4))
  assert lib.hbk_hash_remove_n(2, arr, None) == _lib.OK


# ---- Python argument handling ---------------------------------------------------------------------------------
def test_python_refusals():
  plain = HashTable(64, 4, 'cpu')
  t = HashTable(64, 4, 'cpu', expiring=True)
  ids = torch.arange(5, dtype=torch.int64)
  good = torch.zeros(64, 4)
  # a plain table: refused with the reason
  for call in (lambda: plain.remove(ids), lambda: hb.embedding.hash_remove([t, plain], [ids, ids]),
               lambda: _ht.remove_tables([plain], [ids], None, None)):     # (what the lookup objects call)
    with pytest.raises(_lib.InvalidArgumentError, match='expiring=True.*TOMBSTONE'):
      call()
  with pytest.raises(_lib.InvalidArgumentError, match='expiring=True'):
    plain.track_removals()
  for call in (t.removed_keys, t.clear_removals):
    with pytest.raises(_lib.InvalidArgumentError, match='track_removals'):
      call()
  # more than 4 companions, and the other shapes of a bad companion
  for bad in ([(good, 0.0)] * 5, [good], [(good.double(), 0.0)], [(torch.zeros(63, 4), 0.0)], [(good, float('nan'))]):
    with pytest.raises(_lib.InvalidArgumentError, match='slots|companion'):
      t.remove(ids, slots=bad)
  # ids that are no int64 vector
  for bad in (ids.int(), ids.float(), ids.reshape(5, 1), ids.tolist()):
    with pytest.raises(_lib.InvalidArgumentError, match='int64'):
      t.remove(bad)
  with pytest.raises(_lib.InvalidArgumentError, match='id tensors'):
    hb.embedding.hash_remove([t], [ids, ids])
  with pytest.raises(_lib.InvalidArgumentError, match='lists of companion'):
    hb.embedding.hash_remove([t], [ids], slots=[[], []])
  with pytest.raises(_lib.InvalidArgumentError, match='outputs'):
    hb.embedding.hash_remove([t], [ids], outs=[None, None])
  for wrong, slots in ((HashSpillStore(5), ()), (HashSpillStore(4, [4]), ()), (object(), ())):
    with pytest.raises(_lib.InvalidArgumentError, match='store'):
      t.remove(ids, slots=slots, store=wrong)
  with pytest.raises(_lib.InvalidArgumentError, match='spill stores'):
    _ht.remove_tables([t], [ids], None, [HashSpillStore(4), HashSpillStore(4)])
  with pytest.raises(_lib.HbkError, match='HBM'):                          # a host table: there is no CPU path
    t.remove(ids)
  assert hb.embedding.hash_remove([], []) == []
  # tracking is a host-side switch
  t.track_removals()
  assert t.removed_keys().numel() == 0 and t.removed_keys().dtype == torch.int64
  t.clear_removals()
  t.track_removals(False)
  with pytest.raises(_lib.InvalidArgumentError, match='track_removals'):
    t.removed_keys()


def _export(n=3, removed=None, slot_dims=(2,)):
  return HashExport(torch.arange(n, dtype=torch.int64), torch.zeros(n, 4), torch.ones(n, dtype=torch.int32),
                    torch.ones(n, dtype=torch.int32), [torch.zeros(n, d) for d in slot_dims], None, 3, removed)


def test_import_of_removals_needs_fill_values():
  t = HashTable(64, 4, 'cpu', expiring=True)
  plain = HashTable(64, 4, 'cpu')
  comp = torch.zeros(64, 2)
  gone = torch.tensor([7, 9], dtype=torch.int64)
  # removals and bare companion tensors: refused, the reason named, before anything is touched
  with pytest.raises(_lib.InvalidArgumentError, match='removed keys.*fill_value.*bare'):
    t.import_items(_export(removed=gone), [comp])
  with pytest.raises(_lib.InvalidArgumentError, match='removed keys.*expiring=True'):
    plain.import_items(_export(removed=gone), [(comp, 0.0)])
  with pytest.raises(_lib.InvalidArgumentError, match='removed must be an int64'):
    t.import_items(_export(removed=gone.int()), [(comp, 0.0)])
  # pairs pass the argument checks (and then meet the host table: there is no CPU path); so do bare tensors when
  # nothing was removed, as before
  for exp, slots in ((_export(removed=gone), [(comp, 0.5)]), (_export(removed=gone[:0]), [comp]),
                     (_export(removed=None), [comp]), (_export(removed=None), [(comp, 0.5)])):
    with pytest.raises(_lib.HbkError, match='HBM'):
      t.import_items(exp, slots)
  with pytest.raises(_lib.InvalidArgumentError, match='companion'):
    t.import_items(_export(removed=gone), [(comp, 0.5), (comp, 0.5)])


# ---- the export's new field -------------------------------------------------------------------------------------
def test_export_variables_without_removed_are_what_they_were():
  exp = _export(removed=None)
  exp.src_slots = torch.arange(3, dtype=torch.int64)
  assert exp.removed is None
  assert sorted(exp.variables('t')) == sorted('t/items/' + k for k in ('keys', 'rows', 'since', 'last_seen', 'freq',
                                                                      'src_slots', 'slot0'))
  plain = HashExport(torch.arange(2, dtype=torch.int64), torch.zeros(2, 4))
  assert sorted(plain.variables('t')) == ['t/items/keys', 't/items/rows', 't/items/since'] and plain.removed is None
  assert HashExport.from_variables('t', exp.variables('t')).removed is None
  assert HashExport.empty(3, 4, True, (2,)).removed is None
  assert HashExport.cat([exp, exp]).removed is None


def test_export_removed_round_trips():
  gone = torch.tensor([-5, 2, 2 ** 62], dtype=torch.int64)
  exp = _export(removed=gone)
  d = exp.variables('t')
  assert 't/items/removed' in d and d['t/items/removed'] is gone
  back = HashExport.from_variables('t', d)
  assert back.removed.tolist() == gone.tolist() and back.since == 3 and back.keys.tolist() == [0, 1, 2]
  # empty(): the tensors a restore is read into
  blank = HashExport.empty(3, 4, True, (2,), n_removed=3)
  assert blank.removed.dtype == torch.int64 and tuple(blank.removed.shape) == (3,)
  assert sorted(blank.variables('t')) == sorted(list(d) + ['t/items/src_slots'])
  for k, v in d.items():
    blank.variables('t')[k].copy_(v)
  assert blank.removed.tolist() == gone.tolist()
  assert HashExport.empty(0, 4, n_removed=0).removed.numel() == 0
  # cat keeps it when every part has it: one ascending distinct list
  other = _export(removed=torch.tensor([2, -9], dtype=torch.int64))
  assert HashExport.cat([exp, other]).removed.tolist() == [-9, -5, 2, 2 ** 62]
  assert HashExport.cat([exp, _export(removed=gone[:0])]).removed.tolist() == gone.tolist()
  assert HashExport.cat([exp, _export(removed=None)]).removed is None


# ---- the host store ---------------------------------------------------------------------------------------------
def test_store_discard():
  rng = np.random.RandomState(3)
  keys = [40, -7, 2 ** 62, 13, -2 ** 63 + 5]
  n = len(keys)
  exp = HashExport(torch.tensor(keys, dtype=torch.int64), torch.from_numpy(rng.rand(n, 3).astype(np.float32)),
                   torch.arange(n, dtype=torch.int32), torch.ones(n, dtype=torch.int32),
                   [torch.from_numpy(rng.rand(n, 2).astype(np.float32))])
  store = HashSpillStore(3, (2,), pin_memory=False)
  assert store.discard(torch.tensor([1, 2], dtype=torch.int64)) == 0         # an empty store
  store.put(exp)
  kept = store.peek(torch.tensor([-7, 2 ** 62, -2 ** 63 + 5], dtype=torch.int64))
  # duplicates count once, absent keys are not there to leave
  assert store.discard(torch.tensor([13, 99, 40, 13], dtype=torch.int64)) == 2
  assert store.keys().tolist() == [-2 ** 63 + 5, -7, 2 ** 62] and len(store) == 3
  rest = store.peek(store.keys())
  for a, b in zip(_ht.HashSpillStore._arrays(rest), _ht.HashSpillStore._arrays(kept)):   # the others: bit for bit
    assert a.numpy().tobytes() == b.numpy().tobytes()
  assert store.discard(torch.tensor([13, 40], dtype=torch.int64)) == 0
  assert store.discard(torch.zeros(0, dtype=torch.int64)) == 0
  with pytest.raises(_lib.InvalidArgumentError, match='int64'):
    store.discard(torch.tensor([1.0]))
  assert store.discard(store.keys()) == 3 and len(store) == 0
  # take is what it was
  store.put(exp)
  assert store.take(torch.tensor([13, 5], dtype=torch.int64)).keys.tolist() == [13] and len(store) == 4


# ---- the restatement's own properties -------------------------------------------------------------------------
def _random_table(rng, cap):
  cache = np.full(cap, xref.EMPTY, np.int64)
  kind = rng.randint(0, 10, size=cap)
  n = int((kind < 6).sum())
  cache[kind < 6] = rng.choice(2 ** 20, size=n, replace=False).astype(np.int64) - 2 ** 19
  cache[kind == 6] = xref.TOMBSTONE
  return cache, rng.randint(0, 9, size=cap).astype(np.int32), rng.randint(1, 6, size=cap).astype(np.int32)


@pytest.mark.parametrize('keep_freq', [0, 3])
def test_reference_removing_what_a_sweep_evicts_is_the_sweep(keep_freq):
  rng = np.random.RandomState(5 + keep_freq)
  for trial in range(20):
    cache, last_seen, freq = _random_table(rng, 200)
    comp = rng.rand(200, 6).astype(np.float32)
    swept = [x.copy() for x in (cache, last_seen, freq, comp)]
    mask = xref.evict(swept[0], swept[1], swept[2], 9, 4, keep_freq, [(swept[3], 5, 0.25)])
    ids = cache[mask]
    ids = np.concatenate([ids, ids[::2], [xref.EMPTY, xref.TOMBSTONE, 2 ** 40]])   # duplicates, sentinels, an absent id
    rng.shuffle(ids)
    mine = [x.copy() for x in (cache, last_seen, freq, comp)]
    slots, n_removed = rref.remove(mine[0], mine[1], mine[2], ids, [(mine[3], 5, 0.25)])
    assert n_removed == int(mask.sum())
    for x, y in zip(mine, swept):
      np.testing.assert_array_equal(x, y)
    found = slots >= 0
    np.testing.assert_array_equal(cache[slots[found]], ids[found])          # the slots are those before the call
    assert set(ids[~found].tolist()) <= {xref.EMPTY, xref.TOMBSTONE, 2 ** 40}
    np.testing.assert_array_equal(comp[:, 5], mine[3][:, 5])                # the padding is not written
    # a second removal of the same ids finds nothing and changes nothing
    again = [x.copy() for x in mine]
    slots, n_removed = rref.remove(again[0], again[1], again[2], ids, [(again[3], 5, 0.25)])
    assert n_removed == 0 and (slots == -1).all()
    for x, y in zip(again, mine):
      np.testing.assert_array_equal(x, y)
