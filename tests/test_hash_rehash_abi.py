"""hbk_hash_rehash_n at the C ABI and in Python's argument handling, without a GPU: the entry exists beside an
unchanged version, its structs mirror the header, every refused argument is refused before any device work
with the reason named, and the sequential restatement the GPU tests compare with
(tests/support/hash_rehash_ref.py) agrees with hash_ref.fill and the C oracle's probe."""
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
from tests.support import hash_ref as ref
from tests.support import hash_rehash_ref as rref

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


def test_symbol_prototype_version_and_struct_layouts():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_hash_rehash_n')
  assert lib.hbk_hash_rehash_n.restype is C.c_int
  assert lib.hbk_hash_rehash_n.argtypes == [C.c_int32, C.c_void_p, C.c_void_p]
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  proto = re.search(r'int hbk_hash_rehash_n\(([^)]*)\);', HEADER).group(1)
  assert re.sub(r'\s+', ' ', proto) == 'int32_t n_cols, const hbk_hash_rehash_column_t* cols, hbk_stream_t stream'
  assert '#define HBK_HASH_MAX_MOVES 8' in HEADER and _lib.HASH_MAX_MOVES == 8
  # two pointers, three int32 (+4)
  M = _lib.HashMove
  assert C.sizeof(M) == 32
  assert [M.src.offset, M.dst.offset, M.words.offset, M.src_pitch.offset, M.dst_pitch.offset] == [0, 8, 16, 20, 24]
  # pointer, int64, int32 (+4); pointer, int64, three int32 (+4); eight moves; two pointers
  R = _lib.HashRehashColumn
  assert C.sizeof(R) == 24 + 32 + 8 * 32 + 16 == 328
  assert [R.src_keys.offset, R.src_slab_count.offset, R.src_slab_size.offset, R.dst_keys.offset,
          R.dst_slab_count.offset, R.dst_slab_size.offset, R.expiring.offset, R.n_moves.offset, R.moves.offset,
          R.new_slots.offset, R.counts.offset] == [0, 8, 16, 24, 32, 40, 44, 48, 56, 312, 320]
  assert hb.embedding.hash_rehash is _ht.hash_rehash
  # the structs that were there are what they were
  assert C.sizeof(_lib.HashColumn) == 88 and C.sizeof(_lib.HashEvictColumn) == 168


def test_header_declares_the_structs_as_mirrored():
  assert _struct_fields('hbk_hash_move_t') == [n for n, _ in _lib.HashMove._fields_]
  assert _struct_fields('hbk_hash_rehash_column_t') == [n for n, _ in _lib.HashRehashColumn._fields_]
  for word in ('all EMPTY on entry', 'relaxed agent-scope 8-byte atomic load', 'dst_slab_size per slab',
               'n_moved, n_failed', 'captured graphs'):
    assert word in HEADER, word


GOOD_MOVE = (fake(4), fake(5), 16, 0, 0)


def _rcol(moves=(GOOD_MOVE,), **kw):
  col = _lib.HashRehashColumn()
  col.src_keys, col.src_slab_count, col.src_slab_size = fake(0), 8, 16
  col.dst_keys, col.dst_slab_count, col.dst_slab_size = fake(1), 32, 8
  col.expiring = 0
  col.n_moves = len(moves)
  for m, (src, dst, words, src_pitch, dst_pitch) in enumerate(moves):
    mv = col.moves[m]
    mv.src, mv.dst, mv.words, mv.src_pitch, mv.dst_pitch = src, dst, words, src_pitch, dst_pitch
  col.new_slots, col.counts = fake(2), fake(3)
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _refused(cols, *words):
  lib = _lib.lib()
  arr = (_lib.HashRehashColumn * len(cols))(*cols)
  rc = lib.hbk_hash_rehash_n(len(cols), arr, None)
  msg = lib.hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_rehash_n',) + words:
    assert w in msg, msg


@pytest.mark.parametrize('kw,words', [
  (dict(src_slab_size=0), ('src_slab_size',)), (dict(src_slab_size=65), ('src_slab_size',)),
  (dict(dst_slab_size=0), ('dst_slab_size',)), (dict(dst_slab_size=65), ('dst_slab_size',)),
  (dict(src_slab_count=0), ('src_slab_count',)), (dict(dst_slab_count=0), ('dst_slab_count',)),
  (dict(src_slab_count=(1 << 56) + 1), ('src_slab_count', 'range')),
  (dict(dst_slab_count=(1 << 56) + 1), ('dst_slab_count', 'range')),
  (dict(src_keys=None), ('src_keys', 'NULL')), (dict(dst_keys=None), ('dst_keys', 'NULL')),
  (dict(src_keys=fake(0) + 4), ('src_keys', 'aligned')), (dict(dst_keys=fake(1) + 4), ('dst_keys', 'aligned')),
  (dict(dst_keys=fake(0)), ('same array',)),
  (dict(n_moves=-1), ('n_moves',)), (dict(n_moves=9), ('n_moves',)),
  (dict(moves=[GOOD_MOVE, (fake(4), fake(5), 0, 0, 0)]), ('move 1', 'words')),
  (dict(moves=[(fake(4), fake(5), 16, 15, 0)]), ('move 0', 'src_pitch')),
  (dict(moves=[(fake(4), fake(5), 16, 0, 15)]), ('move 0', 'dst_pitch')),
  (dict(moves=[(None, fake(5), 16, 0, 0)]), ('move 0', 'NULL')),
  (dict(moves=[GOOD_MOVE] * 7 + [(fake(4), None, 16, 0, 0)]), ('move 7', 'NULL')),
  (dict(moves=[(fake(4), fake(4), 16, 0, 0)]), ('move 0', 'same array')),
])
def test_refusals(kw, words):
  _refused([_rcol(), _rcol(**kw)], 'column 1', *words)


def test_counts_of_things_and_nothing_to_do():
  lib = _lib.lib()
  assert lib.hbk_hash_rehash_n(-1, None, None) == _lib.INVALID_ARGUMENT and 'n_cols' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_rehash_n(1, None, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_rehash_n(0, None, None) == _lib.OK
  arr = (_lib.HashRehashColumn * 1)(_rcol())
  assert lib.hbk_hash_rehash_n(0, arr, None) == _lib.OK


# ---- Python argument handling ---------------------------------------------------------------------------
def test_python_refusals_leave_the_table_alone():
  t = hb.embedding.HashTable(64, 4, 'cpu', expiring=True)
  before = (t.keys, t.table, t.last_seen, t.freq, t.capacity, t.slab_count, t.slab_size)
  good = torch.zeros(64, 4)
  for kw in (dict(slab_size=0), dict(slab_size=65), dict(capacity=7), dict(capacity=16, slab_size=32)):
    with pytest.raises(_lib.InvalidArgumentError, match='slab'):
      t.rehash(**kw)
  for bad in ([good], [(good.double(), 0.0)], [(torch.zeros(63, 4), 0.0)], [(good, float('nan'))], [(good, 0.0)] * 5):
    with pytest.raises(_lib.InvalidArgumentError, match='slots|companion'):
      t.rehash(slots=bad)
  with pytest.raises(_lib.InvalidArgumentError, match='expected 1'):
    hb.embedding.hash_rehash([t], capacities=[64, 64])
  with pytest.raises(_lib.InvalidArgumentError, match='twice'):
    hb.embedding.hash_rehash([t, t])
  for kw in (dict(max_load=0.0), dict(max_load=1.5), dict(factor=1.0), dict(factor=float('inf'))):
    with pytest.raises(_lib.InvalidArgumentError, match='max_load|factor'):
      t.maybe_grow(**kw)
  with pytest.raises(_lib.HbkError, match='HBM'):                     # a host table: there is no CPU path
    t.rehash()
  now = (t.keys, t.table, t.last_seen, t.freq, t.capacity, t.slab_count, t.slab_size)
  assert all(a is b for a, b in zip(before, now))
  assert hb.embedding.hash_rehash([]) == []


def test_maybe_grow_below_the_load_reads_the_counters_and_does_nothing():
  t = hb.embedding.HashTable(64, 4, 'cpu', expiring=True)
  t.counts[0] = 48                                                     # 48 / 64 == max_load: not above it
  assert t.maybe_grow(0.75) is None
  t.stats[1] = 1                                                       # one of them went into a reused slot
  t.counts[0] = 49
  assert t.maybe_grow(0.75) is None
  plain = hb.embedding.HashTable(64, 4, 'cpu')
  plain.counts[0] = 48
  assert plain.maybe_grow() is None


# ---- the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize('src,dst', [((5, 3), (8, 7)), ((16, 257), (8, 1031)), ((64, 1), (64, 2)), ((8, 64), (5, 40))])
def test_restatement_places_as_the_plain_fill_and_the_oracle_probe_finds_every_key(src, dst):
  rng = np.random.RandomState(src[0] * 100 + dst[1])
  cap = src[0] * src[1]
  n = cap // 4
  keys = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n, dtype=np.int64))
  rng.shuffle(keys)
  old = np.full(cap, ref.EMPTY, np.int64)
  assert (ref.fill(old, src[0], keys) >= 0).all()
  old[np.where(old == ref.EMPTY)[0][:3]] = rref.TOMBSTONE
  for expiring in (True, False):
    new, new_slots, n_moved, n_failed = rref.rehash(old, dst[0], dst[1], expiring)
    live = rref.live_mask(old, expiring)
    assert (n_moved, n_failed) == (int(live.sum()), 0)
    assert (new_slots[~live] == -1).all()
    np.testing.assert_array_equal(new[new_slots[live]], old[live])
    want = np.full(dst[0] * dst[1], ref.EMPTY, np.int64)
    ref.fill(want, dst[0], old[live])                                  # source-slot order, one key at a time
    np.testing.assert_array_equal(new, want)
    np.testing.assert_array_equal(oracle.cache_probe(new, dst[0], old[live]), new_slots[live])
  # a destination too small: the keys that found every slab full are -1 and counted
  new, new_slots, n_moved, n_failed = rref.rehash(old, 1, 2, True)
  assert (n_moved, n_failed) == (2, keys.size - 2) and int((new_slots >= 0).sum()) == 2
