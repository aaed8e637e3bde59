"""hbk_hash_translate_runs_lowp_n and hbk_hash_translate_sequence_lowp_n on the GPU, the two C entries directly.
Each IS the matching fp32 entry except for the row the inserting launch writes, so every case has a twin: table A
(16-bit, the new entry) and table B (fp32, the fp32 entry) are offered the same ids.  Slot numbers are run-dependent;
compared PER KEY: the key set of every slab, the counters, last_seen, freq and the sketch equal the twin's; the new
rows equal torch's cast of the fp32 start rows, bit for bit; every row no key took is still zero; the padding up to
the pitch keeps what it held."""
import ctypes as C

import numpy as np
import pytest
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import HashTable
from hybridbackend_amd.embedding.hashtable import LOWP_DTYPES
from tests.support import hash_ref as ref
from tests.support.hash_lowp import bits16, cast_rows, dev, host, translate_runs, translate_sequence

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LOWP = [torch.bfloat16, torch.float16]
IDS = ['bf16', 'fp16']
KINDS = {'plain': {}, 'expiring': dict(expiring=True), 'filtered': dict(min_freq=2),
         'both': dict(expiring=True, min_freq=2)}
MAX_RUNS = _lib.HASH_MAX_RUNS_PER_LAUNCH


def per_key(table, array, keys):
  slots = host(table.find(dev(keys)))
  assert (slots >= 0).all()
  return host(array)[slots], slots


def assert_twin(a, b, stored, what=''):
  """a: the 16-bit table, b: its fp32 twin; stored: the distinct keys both hold."""
  np.testing.assert_array_equal(np.sort(host(a.keys)), np.sort(host(b.keys)), what)
  assert host(a.counts).tolist() == host(b.counts).tolist(), what
  rows_b, _ = per_key(b, b.table, stored)
  np.testing.assert_array_equal(rows_b, ref.init_rows(stored, b.dim, b.seed, b.init_scale), what)
  got = bits16(a.table)
  _, slots = per_key(a, a.keys, stored)
  np.testing.assert_array_equal(got[slots], cast_rows(stored, a.dim, a.seed, a.init_scale, a.dtype), what)
  np.testing.assert_array_equal(
    got[slots], torch.from_numpy(rows_b).to(a.dtype).view(torch.int16).numpy().view(np.uint16), what)
  free = np.ones(a.capacity, bool)
  free[slots] = False
  assert not got[free].any(), f'{what}: a row no key took was written'
  if a.expiring:
    assert host(a.stats).tolist() == host(b.stats).tolist(), what
    np.testing.assert_array_equal(per_key(a, a.freq, stored)[0], per_key(b, b.freq, stored)[0], what)
    np.testing.assert_array_equal(per_key(a, a.last_seen, stored)[0], per_key(b, b.last_seen, stored)[0], what)
  if a.min_freq:
    np.testing.assert_array_equal(host(a.sketch), host(b.sketch), what)
    assert host(a.filter_counts).tolist() == host(b.filter_counts).tolist(), what


def twins(kind, dtype, slab_size, dim, capacity=1024, seed=0x5EED, scale=1.0):
  kw = dict(slab_size=slab_size, init_scale=scale, seed=seed + dim, sketch_width=4096, **KINDS[kind])
  a, b = HashTable(capacity, dim, DEV, dtype=dtype, **kw), HashTable(capacity, dim, DEV, **kw)
  for t in (a, b):
    if t.expiring:
      t.set_step(3)
  return a, b


def three_runs(rng):
  """300 ids from a pool of 200 in W = 3 runs of unequal length, one of them empty: duplicates across runs."""
  pool = rng.randint(-2 ** 62, 2 ** 62, size=200, dtype=np.int64)
  ids = pool[rng.randint(0, 200, size=300)]
  ids[:200] = pool
  ids = rng.permutation(ids)
  return [ids[:170], ids[:0], ids[170:]], ids


# ---- runs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
@pytest.mark.parametrize('slab_size,dim', [(1, 2), (8, 6), (8, 16), (64, 64), (8, 130)])
@pytest.mark.parametrize('kind', list(KINDS))
def test_runs_entry_writes_the_cast_start_rows_and_is_the_fp32_entry_otherwise(kind, slab_size, dim, dtype):
  rng = np.random.RandomState(slab_size * 1000 + dim)
  runs, ids = three_runs(rng)
  a, b = twins(kind, dtype, slab_size, dim)
  d_runs = [[dev(r) for r in runs]]
  got_a, got_b = translate_runs([a], d_runs), translate_runs([b], d_runs)
  sa = np.concatenate([host(x) for x in got_a[0]])
  sb = np.concatenate([host(x) for x in got_b[0]])
  stored = sa >= 0
  np.testing.assert_array_equal(stored, sb >= 0)             # the filter's decision is the twin's
  np.testing.assert_array_equal(host(a.keys)[sa[stored]], ids[stored])
  assert stored.any() and a.failed() == 0
  if 'min_freq' not in KINDS[kind]:
    assert stored.all() and a.size() == 200
  assert_twin(a, b, np.unique(ids[stored]), kind)
  # a second call meets its keys: nothing is initialised again, the metadata moves as the twin's
  a.table.view(torch.int16)[int(sa[stored][0])] = 0x1234
  before = bits16(a.table)
  for t in (a, b):
    if t.expiring:
      t.set_step(5)
  translate_runs([a], d_runs)
  translate_runs([b], d_runs)
  uniq = np.unique(ids)
  _, slots = per_key(a, a.keys, uniq)                        # (the second call admits every id seen twice)
  np.testing.assert_array_equal(bits16(a.table)[sa[stored]], before[sa[stored]])
  fresh = np.setdiff1d(uniq, np.unique(ids[stored]))
  if fresh.size:
    np.testing.assert_array_equal(bits16(a.table)[per_key(a, a.keys, fresh)[1]],
                                  cast_rows(fresh, dim, a.seed, a.init_scale, dtype))
  np.testing.assert_array_equal(np.sort(host(a.keys)), np.sort(host(b.keys)))
  assert host(a.counts).tolist() == host(b.counts).tolist()
  if a.expiring:
    np.testing.assert_array_equal(per_key(a, a.freq, uniq)[0], per_key(b, b.freq, uniq)[0])
    assert (per_key(a, a.last_seen, uniq)[0] == 5).all()


@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
@pytest.mark.parametrize('kind', list(KINDS))
def test_runs_insert_0_writes_nothing(kind, dtype):
  rng = np.random.RandomState(9)
  runs, ids = three_runs(rng)
  a, _ = twins(kind, dtype, 8, 16)
  d_runs = [[dev(r) for r in runs]]
  before = (host(a.keys), bits16(a.table), host(a.counts))
  got = translate_runs([a], d_runs, insert=False)
  assert all((host(s) == -1).all() for s in got[0])
  for x, y in zip(before, (host(a.keys), bits16(a.table), host(a.counts))):
    np.testing.assert_array_equal(x, y)
  if a.min_freq:
    assert not host(a.sketch).any()
  first = translate_runs([a], d_runs)
  translate_runs([a], d_runs)                                 # (a filtered table admits on the second sight)
  rows = bits16(a.table)
  again = translate_runs([a], d_runs, insert=False)
  np.testing.assert_array_equal(bits16(a.table), rows)
  found = np.concatenate([host(x) for x in again[0]])
  assert (found >= 0).all()
  np.testing.assert_array_equal(host(a.keys)[found], ids)
  del first


@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
def test_runs_keep_the_padding_up_to_the_pitch(dtype):
  rng = np.random.RandomState(77)
  dim, pitch, slab_size, slab_count = 6, 8, 8, 64
  cap = slab_size * slab_count
  runs, ids = three_runs(rng)
  d_runs = [dev(r) for r in runs]
  keys = torch.full((cap,), -2 ** 63, dtype=torch.int64, device=DEV)
  buf = torch.full((cap, pitch), 0x7FFF, dtype=torch.int16, device=DEV)
  outs = [torch.empty(r.size, dtype=torch.int64, device=DEV) for r in runs]
  counts = torch.zeros(2, dtype=torch.int32, device=DEV)
  col = (_lib.HashColumn * 1)()
  col[0].keys_cache, col[0].slab_count, col[0].slab_size = keys.data_ptr(), slab_count, slab_size
  col[0].counts = counts.data_ptr()
  col[0].table, col[0].dim, col[0].table_pitch, col[0].init_scale, col[0].seed = buf.data_ptr(), dim, pitch, 1.0, 11
  r = (_lib.HashRun * 3)()
  for k in range(3):
    r[k].keys, r[k].slots, r[k].n_keys = (d_runs[k].data_ptr(), outs[k].data_ptr(), runs[k].size) if runs[k].size \
        else (None, None, 0)
  _lib.check(_lib.lib().hbk_hash_translate_runs_lowp_n(
    1, col, None, None, (C.c_int32 * 1)(LOWP_DTYPES[dtype]), _lib.i32_array([3]),
    _lib.ptr_array([C.cast(r, C.c_void_p).value]), 1, _lib.current_stream(torch.device(DEV))))
  torch.cuda.synchronize()
  s = np.concatenate([host(o) for o in outs])
  assert (s >= 0).all() and counts.tolist() == [200, 0]
  got = buf.cpu().numpy().view(np.uint16)
  np.testing.assert_array_equal(got[s, :dim], cast_rows(ids, dim, 11, 1.0, dtype))
  assert (got[:, dim:] == 0x7FFF).all(), 'the padding was written'
  free = np.ones(cap, bool)
  free[s] = False
  assert (got[free] == 0x7FFF).all(), 'a row no key took was written'


@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
def test_65_tiny_columns_cross_the_64_column_launch_boundary(dtype):
  rng = np.random.RandomState(65)
  A = [HashTable(64, 2, DEV, slab_size=8, init_scale=1.0, seed=c, dtype=dtype) for c in range(65)]
  ids = [rng.randint(-2 ** 62, 2 ** 62, size=5, dtype=np.int64) for _ in range(65)]
  got = translate_runs(A, [[dev(i[:2]), dev(i[2:])] for i in ids])
  for c, t in enumerate(A):
    s = np.concatenate([host(x) for x in got[c]])
    assert (s >= 0).all() and t.size() == 5, c
    np.testing.assert_array_equal(host(t.keys)[s], ids[c])
    np.testing.assert_array_equal(bits16(t.table)[s], cast_rows(ids[c], 2, c, 1.0, dtype))
    assert int((bits16(t.table) != 0).any(axis=1).sum()) <= 5


@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
@pytest.mark.parametrize('kind', ['plain', 'both'])
def test_more_non_empty_runs_than_one_launch_takes(kind, dtype):
  rng = np.random.RandomState(MAX_RUNS)
  n_runs = MAX_RUNS + 9
  a, b = twins(kind, dtype, 8, 6, capacity=4096)
  pool = rng.randint(-2 ** 62, 2 ** 62, size=400, dtype=np.int64)
  runs = [pool[rng.randint(0, 400, size=3)] for _ in range(n_runs)]
  # two tables, so that a column's runs straddle the launches and the second column starts in the second launch
  a2, b2 = twins(kind, dtype, 8, 6, capacity=4096, seed=99)
  d_runs = [[dev(r) for r in runs], [dev(r) for r in runs[:20]]]
  for _ in range(2):                                          # (twice: a filtered table admits on the second sight)
    got = translate_runs([a, a2], d_runs)
    translate_runs([b, b2], d_runs)
  for t, u, rr, g in ((a, b, runs, got[0]), (a2, b2, runs[:20], got[1])):
    ids = np.concatenate(rr)
    s = np.concatenate([host(x) for x in g])
    assert (s >= 0).all()
    np.testing.assert_array_equal(host(t.keys)[s], ids)
    assert_twin(t, u, np.unique(ids), kind)


# ---- sequences ------------------------------------------------------------------------------------------------
def sequences(rng, pool):
  """B = 7, T = 4, lengths 0 .. 6: the ids past T of the long samples are ids nobody else holds."""
  lens = np.array([0, 1, 2, 3, 4, 5, 6])
  splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  ids = pool[rng.randint(0, 10, size=int(splits[-1]))]
  past = []
  for b in range(7):
    for t in range(4, lens[b]):
      ids[splits[b] + t] = pool[20 + len(past)]               # distinct ids, only ever past T
      past.append(ids[splits[b] + t])
  return ids, splits, lens, np.array(past, np.int64)


@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
@pytest.mark.parametrize('pad_id', [None, -1], ids=['nopad', 'pad'])
@pytest.mark.parametrize('kind', list(KINDS))
def test_sequence_entry_writes_the_cast_start_rows_and_is_the_fp32_entry_otherwise(kind, pad_id, dtype):
  rng = np.random.RandomState(len(kind) + 7)
  T = 4
  pool = rng.randint(-2 ** 62, 2 ** 62, size=40, dtype=np.int64)
  ids, splits, lens, past = sequences(rng, pool)
  a, b = twins(kind, dtype, 8, 16, capacity=256)
  d_ids, d_splits = [dev(ids)], [dev(splits)]
  for step in (3, 5):                                         # (twice: a filtered table admits on the second sight)
    for t in (a, b):
      if t.expiring:
        t.set_step(step)
    ga, la = translate_sequence([a], d_ids, d_splits, T, pad_id)
    gb, lb = translate_sequence([b], d_ids, d_splits, T, pad_id)
  np.testing.assert_array_equal(host(la[0]), np.minimum(lens, T))
  np.testing.assert_array_equal(host(lb[0]), np.minimum(lens, T))
  grid = host(ga[0]).reshape(7, T)
  effective = []
  for s in range(7):
    for t in range(T):
      if t < min(lens[s], T):
        assert grid[s, t] >= 0 and host(a.keys)[grid[s, t]] == ids[splits[s] + t]
        effective.append(ids[splits[s] + t])
      elif pad_id is None:
        assert grid[s, t] == -1
      else:
        assert grid[s, t] >= 0 and host(a.keys)[grid[s, t]] == pad_id
        effective.append(pad_id)
  np.testing.assert_array_equal(host(ga[0]) >= 0, host(gb[0]) >= 0)
  stored = np.unique(np.array(effective, np.int64))
  assert a.size() == stored.size and a.failed() == 0
  assert_twin(a, b, stored, kind)
  # the ids past T are in no table afterwards
  assert (host(a.find(dev(past))) == -1).all() and (host(b.find(dev(past))) == -1).all()
  # insert == 0 writes nothing and answers the same grid
  before = (host(a.keys), bits16(a.table), host(a.counts))
  found, _ = translate_sequence([a], d_ids, d_splits, T, pad_id, insert=False)
  np.testing.assert_array_equal(host(found[0]), host(ga[0]))
  for x, y in zip(before, (host(a.keys), bits16(a.table), host(a.counts))):
    np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
def test_sequence_insert_0_on_an_empty_table_writes_nothing(dtype):
  rng = np.random.RandomState(3)
  pool = rng.randint(-2 ** 62, 2 ** 62, size=40, dtype=np.int64)
  ids, splits, _, _ = sequences(rng, pool)
  a, _ = twins('expiring', dtype, 8, 16, capacity=256)
  before = (host(a.keys), bits16(a.table), host(a.counts), host(a.freq))
  grids, _ = translate_sequence([a], [dev(ids)], [dev(splits)], 4, -1, insert=False)
  assert (host(grids[0]) == -1).all()
  for x, y in zip(before, (host(a.keys), bits16(a.table), host(a.counts), host(a.freq))):
    np.testing.assert_array_equal(x, y)
