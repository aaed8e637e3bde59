"""Removal by id on the device (hbk_hash_remove_n, HashTable.remove / hash_remove, removal tracking and exact
deltas) against the numpy restatement tests/support/hash_remove_ref.py.  Every comparison is bit for bit: nothing
here is summed in floating point.  The shapes are the smallest at which the kernel can go wrong: a batch that is no
multiple of a wave with duplicates that cross waves (test 1: one workgroup), columns of several 1024-occurrence
tiles beside each other with one id in every workgroup of its column, companions of a width that is no power of two
and of a pitch above their width, a slab that spilled into its neighbour, more tables than one launch takes."""
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (GroupLookupGrad, HashExport, HashGroupLookup, HashSpillStore, HashTable,
                                         ShardedHashGroupLookup, hash_remove)
from tests.support import hash_expiry_ref as xref
from tests.support import hash_ref as ref
from tests.support import hash_remove_ref as rref
from tests.support import reference as model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
EMPTY, TOMB = xref.EMPTY, xref.TOMBSTONE


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def distinct_keys(rng, n):
  """n distinct int64 keys over the full range, neither sentinel nor -1 among them."""
  k = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=2 * n + 8, dtype=np.int64))
  k = k[k != -1]
  rng.shuffle(k)
  return k[:n]


def run_world(world, fn):
  """fn(rank, comm) on `world` host threads over the in-process world, each on a stream of its own; returns the
  per-rank results."""
  comms = hb.distribute.Collective.local_world(world)
  results, errors = [None] * world, []

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        results[r] = fn(r, comms[r])
        torch.cuda.current_stream().synchronize()
    except Exception as e:  # pylint: disable=broad-except
      import traceback
      errors.append((r, repr(e), traceback.format_exc()))

  threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=45)
  for cm in comms:
    cm.close()
  assert not errors, errors
  assert all(x is not None for x in results)
  return results


def homed_in(slab, slab_count, n, start=1):
  out, k = [], start
  while len(out) < n:
    if ref.home_slab(k, slab_count) == slab:
      out.append(k)
    k += 1
  return np.array(out, np.int64)


def table_from_ref(rng, keys, cap, slab_size, dim):
  """An expiring table whose arrays are the restatement's sequential placement of `keys`: the same bits however
  often it is built.  Returns the table and its host arrays."""
  cache = np.full(cap, EMPTY, np.int64)
  last_seen, freq = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
  for step, part in enumerate(np.array_split(keys, 3), 1):
    slots, _, _, n_failed = xref.insert(cache, slab_size, part, last_seen, freq, step)
    assert n_failed == 0
  rows = rng.rand(cap, dim).astype(F32)
  t = HashTable(cap, dim, DEV, slab_size=slab_size, expiring=True)
  t.keys.copy_(dev(cache))
  t.last_seen.copy_(dev(last_seen))
  t.freq.copy_(dev(freq))
  t.table.copy_(dev(rows))
  t.recount()
  return t, dict(cache=cache, last_seen=last_seen, freq=freq, rows=rows)


# ---- 1. one table, at the C level -----------------------------------------------------------------------------
def _case_one():
  rng = np.random.RandomState(11)
  keys = np.concatenate([distinct_keys(rng, 149), [-1]])                    # -1 is an ordinary key
  rng.shuffle(keys)
  t, arrays = table_from_ref(rng, keys, 256, 8, 4)
  comps = [rng.rand(256, 3).astype(F32), rng.rand(256, 16).astype(F32), rng.rand(256, 8).astype(F32)]
  dims, values = [3, 16, 5], [0.25, 0.1, -2.0]                              # the third: pitch 8 > dim 5
  present = np.concatenate([keys[keys != -1][:11], [-1]])
  hot = present[0]
  absent = distinct_keys(np.random.RandomState(12), 400)
  absent = absent[~np.isin(absent, keys)][:5]
  ids = np.concatenate([np.repeat(hot, 299), present, present[1:], [EMPTY, TOMB], absent, absent[:4]])
  assert ids.size == 333 and (np.bincount(np.searchsorted(np.sort(present), ids[np.isin(ids, present)])) >= 2).all()
  rng.shuffle(ids)
  return t, arrays, comps, dims, values, ids


def _c_remove(t, d_ids, d_comps, dims, values, beside_empty=True):
  """hbk_hash_remove_n on one table (and a column without keys beside it); returns (slots, n_removed) tensors."""
  n = d_ids.numel()
  slots = torch.full((n,), -7, dtype=torch.int64, device=DEV)
  n_removed = torch.zeros(2, dtype=torch.int32, device=DEV)
  cols = (_lib.HashRemoveColumn * 2)()
  for c, count in enumerate((n, 0)):
    col = cols[c]
    col.keys_cache, col.slab_count, col.slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
    col.exp.last_seen, col.exp.freq, col.exp.step = t.last_seen.data_ptr(), t.freq.data_ptr(), None
    col.exp.stats = t.stats.data_ptr()
    col.keys, col.n_keys, col.slots = d_ids.data_ptr(), count, slots.data_ptr()
    col.n_removed = n_removed.data_ptr() + 4 * c
    col.n_fills = len(d_comps)
    for f, (x, dim, value) in enumerate(zip(d_comps, dims, values)):
      col.fills[f].base, col.fills[f].pitch, col.fills[f].dim, col.fills[f].value = x.data_ptr(), x.stride(0), dim, value
  _lib.check(_lib.lib().hbk_hash_remove_n(2 if beside_empty else 1, cols, _lib.current_stream(torch.device(DEV))))
  return slots, n_removed


def _run_case_one():
  t, arrays, comps, dims, values, ids = _case_one()
  d_ids, d_comps = dev(ids), [dev(x) for x in comps]
  t.stats.copy_(dev(np.array([0, 5], np.int32)))                            # stats[1] is somebody else's
  counts_before = host(t.counts)
  found_before = host(t.find(d_ids))
  slots, n_removed = _c_remove(t, d_ids, d_comps, dims, values)
  torch.cuda.synchronize()
  want = {k: v.copy() for k, v in arrays.items()}
  want_comps = [x.copy() for x in comps]
  want_slots, want_n = rref.remove(want['cache'], want['last_seen'], want['freq'], ids,
                                   list(zip(want_comps, dims, values)))
  got = dict(slots=host(slots), n_removed=host(n_removed), keys=host(t.keys), last_seen=host(t.last_seen),
             freq=host(t.freq), rows=host(t.table), stats=host(t.stats), counts=host(t.counts),
             comps=[host(x) for x in d_comps])
  np.testing.assert_array_equal(got['slots'], found_before)                 # every occurrence: the slot before the call
  np.testing.assert_array_equal(got['slots'], want_slots)
  assert want_n == 12 and got['n_removed'].tolist() == [12, 0] and got['stats'].tolist() == [12, 5]
  np.testing.assert_array_equal(got['keys'], want['cache'])
  np.testing.assert_array_equal(got['last_seen'], want['last_seen'])
  np.testing.assert_array_equal(got['freq'], want['freq'])
  for x, y in zip(got['comps'], want_comps):
    np.testing.assert_array_equal(x, y)                                     # (the padding of the third among it)
  np.testing.assert_array_equal(got['rows'], arrays['rows'])                # the embedding rows are left
  np.testing.assert_array_equal(got['counts'], counts_before)
  assert (got['keys'] == TOMB).sum() == 12 and (got['keys'] == EMPTY).sum() == (arrays['cache'] == EMPTY).sum()
  assert t.size() == 150 - 12 and t.evicted() == 12
  # a second removal of the same ids: all -1, nothing changes
  slots2, n2 = _c_remove(t, d_ids, d_comps, dims, values, beside_empty=False)
  assert (host(slots2) == -1).all() and host(n2).tolist() == [0, 0]
  for name, x in (('keys', t.keys), ('last_seen', t.last_seen), ('freq', t.freq), ('stats', t.stats)):
    np.testing.assert_array_equal(host(x), got[name])
  for x, y in zip(d_comps, got['comps']):
    np.testing.assert_array_equal(host(x), y)
  return got


def test_one_table_against_the_restatement_and_twice_the_same_bits():
  first, second = _run_case_one(), _run_case_one()
  for name in first:
    if name == 'comps':
      for x, y in zip(first[name], second[name]):
        assert x.tobytes() == y.tobytes()
    else:
      assert first[name].tobytes() == second[name].tobytes(), name


# ---- 2. the probe invariant -----------------------------------------------------------------------------------
def test_a_removed_key_leaves_a_tombstone_the_spilled_key_is_still_found():
  slab_size, slab_count, dim, seed, scale = 2, 8, 4, 9, 0.05
  k = homed_in(2, slab_count, 3)
  t = HashTable(slab_size * slab_count, dim, DEV, slab_size=slab_size, init_scale=scale, seed=seed, expiring=True)
  acc = torch.full((t.capacity, 3), 0.1, device=DEV)
  t.set_step(1)
  assert sorted(host(t.lookup_or_insert(dev(k[:2]))).tolist()) == [4, 5]    # the home slab is full
  assert host(t.lookup_or_insert(dev(k[2:]))).tolist() == [6]               # ... so the third spills into slab 3
  s0 = int(host(t.find(dev(k[:1])))[0])
  t.table[s0] = 7.0                                                         # a trained row and accumulator
  acc[s0] = 3.0
  got = t.remove(dev(k[:1]), slots=[(acc, 0.1)])
  assert host(got).tolist() == [s0]
  cache = host(t.keys)
  assert cache[s0] == TOMB and (cache == EMPTY).sum() == 16 - 3             # never EMPTY: slab 2 stays full
  assert host(t.find(dev(k))).tolist() == [-1, 9 - s0, 6]
  hit, n_miss = hb.embedding.cache.probe(t.keys, dev(k[1:]), slab_size)
  assert host(hit).tolist() == [9 - s0, 6] and int(n_miss.item()) == 0
  assert (host(acc)[s0] == F32(0.1)).all() and (host(t.table)[s0] == 7.0).all()
  assert (t.size(), t.evicted(), t.reused()) == (2, 1, 0)
  # the removed id comes back: it takes the tombstone, once, and starts again
  t.set_step(2)
  assert host(t.lookup_or_insert(dev(np.repeat(k[:1], 70)))).tolist() == [s0] * 70
  cache = host(t.keys)
  assert (cache == k[0]).sum() == 1 and (t.size(), t.reused()) == (3, 1) and (cache == TOMB).sum() == 0
  np.testing.assert_array_equal(host(t.table)[s0], ref.init_rows(k[:1], dim, seed, scale)[0])
  assert (host(acc) == F32(0.1)).all()
  assert host(t.find(dev(k))).tolist() == [s0, 9 - s0, 6]


# ---- 3. more tables than one launch takes -----------------------------------------------------------------------
def test_33_tables_in_one_call():
  rng = np.random.RandomState(33)
  tables, arrays, accs, ids = [], [], [], []
  for c in range(33):
    keys = distinct_keys(rng, 9)
    t, a = table_from_ref(rng, keys, 16, 4, 2)
    tables.append(t)
    arrays.append(a)
    accs.append(rng.rand(16, 2).astype(F32))
    i = np.concatenate([keys[:c % 5], keys[:c % 3], distinct_keys(rng, 2)])  # table 0 (and 15, 30): absent ids only
    rng.shuffle(i)
    ids.append(i)
  d_accs = [dev(a) for a in accs]
  got = hash_remove(tables, [dev(i) for i in ids], [[(a, 0.5)] for a in d_accs])
  torch.cuda.synchronize()
  counters = hb.embedding.hashtable._read_counters(tables)
  for c, t in enumerate(tables):
    want, acc = {k: v.copy() for k, v in arrays[c].items()}, accs[c].copy()
    slots, n = rref.remove(want['cache'], want['last_seen'], want['freq'], ids[c], [(acc, 2, 0.5)])
    assert n == max(c % 5, c % 3)
    np.testing.assert_array_equal(host(got[c]), slots)
    np.testing.assert_array_equal(host(t.keys), want['cache'])
    np.testing.assert_array_equal(host(t.last_seen), want['last_seen'])
    np.testing.assert_array_equal(host(t.freq), want['freq'])
    np.testing.assert_array_equal(host(d_accs[c]), acc)
    assert counters[c] == (9, 0, n, 0)


def test_columns_of_several_tiles_and_duplicates_across_workgroups():
  """An erase tile takes 1024 occurrences.  Three columns in one call: 40, 2500 and 1100 occurrences -- 1, 3 and 2
  tiles, so the columns' first tiles are 0, 1 and 4 and the last tile of each is partly filled (2500 and 1100 are no
  multiples of 64 either).  In the second column one id is named 1100 times, shuffled over the whole batch: its
  occurrences sit in all three workgroups, and one of them wins."""
  rng = np.random.RandomState(35)
  tables, arrays, comps, ids = [], [], [], []
  for c, (n, n_hot) in enumerate(((40, 0), (2500, 1100), (1100, 300))):
    keys = distinct_keys(rng, 500)
    t, a = table_from_ref(rng, keys, 1024, 8, 2)
    tables.append(t)
    arrays.append(a)
    comps.append([rng.rand(1024, 3).astype(F32), rng.rand(1024, 16).astype(F32)])
    present = keys[:(n - n_hot) // 3]
    absent = distinct_keys(rng, 2000)
    absent = absent[~np.isin(absent, keys)]
    i = np.concatenate([np.repeat(keys[-1], n_hot), present, present, [EMPTY, TOMB]])
    i = np.concatenate([i, absent[:n - i.size]])
    assert i.size == n
    rng.shuffle(i)
    if n_hot:
      at = np.flatnonzero(i == keys[-1])
      assert at.min() < 1024 and at.max() >= 1024 * ((n - 1) // 1024)      # in the first and in the last tile
    ids.append(i)
  d_comps = [[dev(x) for x in cs] for cs in comps]
  d_ids = [dev(i) for i in ids]
  found = [host(t.find(i)) for t, i in zip(tables, d_ids)]
  got = hash_remove(tables, d_ids, [[(cs[0], 0.25), (cs[1], -1.5)] for cs in d_comps])
  torch.cuda.synchronize()
  for c, t in enumerate(tables):
    want = {k: v.copy() for k, v in arrays[c].items()}
    want_comps = [x.copy() for x in comps[c]]
    slots, n = rref.remove(want['cache'], want['last_seen'], want['freq'], ids[c],
                           [(want_comps[0], 3, 0.25), (want_comps[1], 16, -1.5)])
    live = arrays[c]['cache'][(arrays[c]['cache'] != EMPTY) & (arrays[c]['cache'] != TOMB)]
    assert n == np.unique(ids[c][np.isin(ids[c], live)]).size > 10
    np.testing.assert_array_equal(host(got[c]), found[c])
    np.testing.assert_array_equal(host(got[c]), slots)
    np.testing.assert_array_equal(host(t.keys), want['cache'])
    np.testing.assert_array_equal(host(t.last_seen), want['last_seen'])
    np.testing.assert_array_equal(host(t.freq), want['freq'])
    for x, y in zip(d_comps[c], want_comps):
      np.testing.assert_array_equal(host(x), y)
    np.testing.assert_array_equal(host(t.table), arrays[c]['rows'])
    assert (t.size(), t.evicted()) == (500 - n, n)


# ---- 4. a captured removal --------------------------------------------------------------------------------------
def test_captured_removal_takes_out_what_the_buffer_holds_at_the_replay():
  rng = np.random.RandomState(44)
  pools = [distinct_keys(rng, 120) for _ in range(2)]
  tables = [HashTable(256, 4, DEV, slab_size=ss, expiring=True) for ss in (8, 5)]
  accs = [torch.full((t.capacity, 4), 2.0, device=DEV) for t in tables]
  for t, p in zip(tables, pools):
    t.set_step(1)
    assert (host(t.lookup_or_insert(dev(p))) >= 0).all()
  parts = [[p[:40], p[40:80], p[80:]] for p in pools]
  bufs = [dev(x[0]) for x in parts]
  outs = [torch.full((40,), -7, dtype=torch.int64, device=DEV) for _ in range(2)]
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):                                # (one branch: two launches in a row)
      hash_remove(tables, bufs, [[(a, 0.5)] for a in accs], outs)
  torch.cuda.synchronize()
  for t in tables:
    assert t.size() == 120                                                 # captured, not run
  for round_, which in enumerate((1, 2), 1):
    for b, x in zip(bufs, parts):
      b.copy_(dev(x[which]))
    where = [host(t.find(b)) for t, b in zip(tables, bufs)]
    graph.replay()
    torch.cuda.synchronize()
    for c, t in enumerate(tables):
      np.testing.assert_array_equal(host(outs[c]), where[c])
      assert (where[c] >= 0).all() and (host(t.find(bufs[c])) == -1).all()
      assert (host(t.find(dev(parts[c][0]))) >= 0).all()                   # the ids of the capture itself: still there
      assert (t.size(), t.evicted()) == (120 - 40 * round_, 40 * round_)
      gone = host(t.keys) == TOMB
      assert gone.sum() == 40 * round_ and (host(accs[c])[gone] == 0.5).all() and (host(accs[c])[~gone] == 2.0).all()


# ---- 5. training across a removal -------------------------------------------------------------------------------
def test_a_removed_id_trains_again_as_in_a_fresh_table():
  rng = np.random.RandomState(55)
  B, dim, lr, scale, acc0 = 96, 16, 0.1, 0.05, 0.1
  seeds = [3, 4]
  tables = [HashTable(256, dim, DEV, slab_size=ss, init_scale=scale, seed=seeds[c], expiring=True)
            for c, ss in enumerate((16, 5))]
  accums = [torch.full_like(t.table, acc0) for t in tables]
  hgl = HashGroupLookup(tables, combiners='sum')
  grad = GroupLookupGrad(hgl.lookup, accums=accums, deterministic=True)
  pools = [distinct_keys(rng, 50) for _ in range(2)]
  uniq = [np.sort(p) for p in pools]
  W = [ref.init_rows(uniq[c], dim, seeds[c], scale) for c in range(2)]
  A = [np.full_like(W[c], F32(acc0)) for c in range(2)]

  def train(step):
    ids = [np.concatenate([p, p[rng.randint(0, p.size, size=B - p.size)]]) for p in pools]
    grads = [rng.randn(B, dim).astype(F32) for _ in range(2)]
    for t in tables:
      t.set_step(step)
    outs = hgl([dev(i) for i in ids], [None, None])
    index = [np.searchsorted(uniq[c], ids[c]) for c in range(2)]
    for c in range(2):
      np.testing.assert_array_equal(host(outs[c]), W[c][index[c]])
    grad(hgl.slots, [dev(g) for g in grads], [None, None], apply_lr=lr, optimizer='adagrad')
    for c in range(2):
      terms, r, valid = model.terms32(uniq[c].size, index[c], None, None, 'sum', grads[c])
      u, sums = model.seq_row_sums(terms, r, valid)
      model.adagrad_step(W[c], A[c], u, sums, lr)

  def check():
    for c in range(2):
      slots = host(tables[c].find(dev(uniq[c])))
      assert (slots >= 0).all()
      np.testing.assert_array_equal(host(tables[c].table)[slots], W[c])
      np.testing.assert_array_equal(host(accums[c])[slots], A[c])

  train(1)
  train(2)
  check()
  gone = [p[:17] for p in pools]
  old = hgl.remove([dev(np.concatenate([g, g[:5]])) for g in gone], [[(a, acc0)] for a in accums])
  for c in range(2):
    assert (host(old[c]) >= 0).all() and (tables[c].size(), tables[c].evicted()) == (33, 17)
    assert (host(tables[c].find(dev(gone[c]))) == -1).all()
    # the model forgets the removed ids: they start again as fresh ids do
    at = np.searchsorted(uniq[c], gone[c])
    W[c][at] = ref.init_rows(gone[c], dim, seeds[c], scale)
    A[c][at] = F32(acc0)
  train(3)                                                                  # train() checks the forward rows
  check()
  train(4)
  check()
  for c in range(2):
    assert tables[c].size() == 50 and tables[c].failed() == 0 and tables[c].reused() > 0


# ---- 6. exact deltas ----------------------------------------------------------------------------------------------
def _by_key(t, acc):
  """{key: (row, last_seen, freq, companion row) as bytes} of the live keys."""
  cache = host(t.keys)
  live = np.flatnonzero((cache != EMPTY) & (cache != TOMB))
  arrays = [host(t.table), host(t.last_seen), host(t.freq), host(acc)]
  return {int(cache[s]): tuple(a[s].tobytes() for a in arrays) for s in live}


def test_base_and_delta_of_a_tracked_table_restore_exactly_the_table():
  rng = np.random.RandomState(66)
  dim, seed, scale, acc0 = 4, 3, 0.05, 0.1
  t = HashTable(512, dim, DEV, slab_size=8, init_scale=scale, seed=seed, expiring=True)
  acc = torch.full((512, dim), acc0, device=DEV)
  store = HashSpillStore(dim, [dim])
  pool = distinct_keys(rng, 240)
  a, b, c, d = pool[:100], pool[100:160], pool[160:200], pool[200:230]
  t.track_removals()

  def touch(step, keys):
    t.set_step(step)
    slots = torch.unique(t.lookup_or_insert(dev(keys)))
    assert int(slots.min().item()) >= 0
    t.table[slots] += 0.01 * step                                           # "training": rows and accumulators move
    acc[slots] += 0.5
  touch(1, a)
  touch(2, b)
  s0 = 2
  base = t.export_items(slots=[acc])
  assert base.removed is not None and base.removed.numel() == 0 and len(base) == 160
  t.clear_removals()
  touch(3, np.concatenate([c, b[:25]]))                                     # new keys, and some of b again
  t.set_step(4)
  t.evict(3, slots=[(acc, acc0)])                                           # last seen at step 1: all of a
  assert t.evicted() == 100
  touch(5, np.concatenate([d, a[:5]]))                                      # new keys; five evicted ones come back
  n = t.size()
  t.evict_to(n - 20, slots=[(acc, acc0)])                                   # the oldest step leaves whole: b's rest
  assert t.size() == n - 35
  again = c[0]
  old = t.remove(dev(np.concatenate([c[:10], c[:3], pool[230:]])), slots=[(acc, acc0)])
  assert (host(old)[:13] >= 0).all() and (host(old)[13:] == -1).all()
  touch(6, np.array([again]))                                               # removed and inserted again
  n = t.size()
  spilled = t.spill_to(n - 10, store, slots=[(acc, acc0)])                   # step 3 leaves for the host tier
  assert len(spilled) == 30 + 25 and len(store) == len(spilled)             # c's rest and the b of step 3
  delta = t.export_items(since=s0 + 1, slots=[acc])
  live = _by_key(t, acc)
  assert sorted(live) == sorted(np.concatenate([d, a[:5], [again]]).tolist())
  # what the delta says
  gone = host(delta.removed)
  assert (np.diff(gone) > 0).all() and again not in gone and not np.isin(gone, list(live)).any()
  assert not np.isin(a[:5], gone).any()
  assert sorted(gone.tolist()) == sorted(np.concatenate([a[5:], b, c[1:]]).tolist())
  assert 'x/items/removed' in delta.variables('x')

  def restore(delta):
    t2 = HashTable(1024, dim, DEV, slab_size=16, init_scale=scale, seed=seed, expiring=True)
    acc2 = torch.full((1024, dim), acc0, device=DEV)
    t2.import_items(base, [acc2])
    t2.import_items(delta, [(acc2, acc0)])
    return t2, acc2
  t2, acc2 = restore(delta)
  got = _by_key(t2, acc2)
  assert sorted(got) == sorted(live)                                        # the key set is the live table's
  assert got == live                                                        # rows, last_seen, freq, companions
  # the base keys that left were taken out (the delta's new keys then reused some of their slots), and no slot
  # without a key keeps a companion row of the key it held
  cache2 = host(t2.keys)
  assert t2.evicted() == 160 - 5 and (cache2 == TOMB).sum() == 160 - 5 - t2.reused() > 0
  assert (host(acc2)[(cache2 == TOMB) | (cache2 == EMPTY)] == F32(acc0)).all()
  assert t2.size() == len(live)
  # bare companion tensors cannot be reset: refused, the reason named
  with pytest.raises(_lib.InvalidArgumentError, match='removed keys.*fill_value'):
    t2.import_items(delta, [acc2])
  # an import refused for its keys has removed nothing: the table is as it was
  k0 = torch.tensor(sorted(live)[:1] * 2, dtype=torch.int64)
  twice = HashExport(k0, torch.zeros(2, dim), torch.zeros(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32),
                     [torch.zeros(2, dim)], None, 3, torch.tensor(sorted(live)[1:9], dtype=torch.int64))
  state = [host(x) for x in (t2.keys, t2.last_seen, t2.freq, t2.stats, acc2)]
  with pytest.raises(_lib.InvalidArgumentError, match='not distinct'):
    t2.import_items(twice, [(acc2, acc0)])
  for x, y in zip((t2.keys, t2.last_seen, t2.freq, t2.stats, acc2), state):
    np.testing.assert_array_equal(host(x), y)
  # the same delta without the field restores a strict superset: what the field is for
  loose = HashExport(delta.keys, delta.rows, delta.last_seen, delta.freq, delta.slots, delta.src_slots, delta.since)
  t3, acc3 = restore(loose)
  stale = _by_key(t3, acc3)
  assert set(stale) > set(live) and len(stale) == len(live) + 160 - 5
  assert all(stale[k] == live[k] for k in live)


def test_tracking_records_the_same_keys_for_every_way_out_and_an_untracked_table_has_no_log():
  rng = np.random.RandomState(67)
  pool = distinct_keys(rng, 90)
  t = HashTable(256, 4, DEV, slab_size=8, expiring=True)
  u = HashTable(256, 4, DEV, slab_size=8, expiring=True)
  for x in (t, u):
    for step, part in enumerate(np.array_split(pool, 3), 1):
      x.set_step(step)
      x.lookup_or_insert(dev(part))
    x.set_step(4)
  t.track_removals()
  p1, p2, p3 = np.array_split(pool, 3)
  for x in (t, u):
    hb.embedding.hash_evict([x], 3)                                         # step 1 leaves
    x.remove(dev(np.concatenate([p2[:7], p2[:7], [EMPTY, TOMB, 12345]])))
    assert x.maybe_evict(max_load=0.2, target_load=0.15) is not None        # evict_to 38 keys, then a rehash
  assert u._removals is None

  def live(x):
    cache = host(x.keys)
    return np.sort(cache[(cache != EMPTY) & (cache != TOMB)])
  np.testing.assert_array_equal(live(t), live(u))                           # tracking changes nothing of the table
  want = np.sort(pool[host(u.find(dev(pool))) < 0])
  np.testing.assert_array_equal(host(t.removed_keys()), want)
  assert np.isin(p1, want).all() and np.isin(p2[:7], want).all() and t.size() == pool.size - want.size
  # a key that comes back is no longer removed; clearing forgets the rest
  t.lookup_or_insert(dev(p1[:4]))
  np.testing.assert_array_equal(host(t.removed_keys()), np.sort(want[~np.isin(want, p1[:4])]))
  t.clear_removals()
  assert t.removed_keys().numel() == 0


# ---- 7. sharded -------------------------------------------------------------------------------------------------
S_DIMS, S_SEEDS, S_SCALE, S_ACC0 = [8, 6], [3, 4], 0.05, 0.1


def _sharded_scenario(world, pools):
  """Every rank: insert the pools (each rank asks for all ids), a base export, remove ids on every rank (the same
  list everywhere), touch some keys, a delta.  Returns per rank its exports, what remove answered and what was
  there."""
  gone = [np.concatenate([p[:30], p[:4], [EMPTY, TOMB]]) for p in pools]

  def rank(r, comm):
    tables = [HashTable(512, S_DIMS[c], DEV, slab_size=(16, 5)[c], init_scale=S_SCALE, seed=S_SEEDS[c], expiring=True)
              for c in range(2)]
    accums = [torch.full_like(t.table, S_ACC0) for t in tables]
    drv = ShardedHashGroupLookup(tables, comm, combiners=['sum', 'sum'], accums=accums,
                                 initial_accumulator_value=S_ACC0)
    drv.track_removals()
    for t in tables:
      t.set_step(1)
    drv([dev(p) for p in pools], [None, None])
    drv.backward([dev(np.ones((p.size, S_DIMS[c]), F32)) for c, p in enumerate(pools)], apply_lr=0.5, emit=False,
                 optimizer='adagrad')
    base = drv.export_items()
    found = [host(t.find(dev(g))) for t, g in zip(tables, gone)]
    keys_before = [host(t.keys) for t in tables]
    old = drv.remove([dev(g) for g in gone])
    for t in tables:
      t.set_step(3)
    drv([dev(p[100:]) for p in pools], [None, None])                        # the last keys are seen again
    delta = drv.export_items(since=2)
    res = dict(base=base, delta=delta, old=[host(o) for o in old], found=found, keys_before=keys_before,
               keys=[host(t.keys) for t in tables], accums=[host(x) for x in accums],
               sizes=[t.size() for t in tables], evicted=[t.evicted() for t in tables])
    drv.close()
    return res
  return gone, rank


def _check_sharded(world, pools, gone, res):
  for c in range(2):
    for r in range(world):
      x = res[r]
      mine = hb.embedding.hash_owner(torch.from_numpy(gone[c]), world).numpy() == r
      real = (gone[c] != EMPTY) & (gone[c] != TOMB)
      np.testing.assert_array_equal(x['old'][c], x['found'][c])             # the slots before the call
      np.testing.assert_array_equal(x['old'][c] >= 0, mine & real)          # the owned ids only: no exchange
      want = x['keys_before'][c].copy()
      slots, n = rref.remove(want, np.zeros(want.size, np.int32), np.zeros(want.size, np.int32), gone[c])
      np.testing.assert_array_equal(x['keys'][c], want)
      assert x['evicted'][c] == n == np.unique(gone[c][mine & real]).size
      assert (x['accums'][c][want == TOMB] == F32(S_ACC0)).all()            # the driver's own fill value
      assert (x['accums'][c][(want != TOMB) & (want != EMPTY)] != F32(S_ACC0)).all()
      np.testing.assert_array_equal(np.sort(host(x['delta'][c].removed)), np.unique(gone[c][mine & real]))
    assert sum(res[r]['sizes'][c] for r in range(world)) == pools[c].size - 30


def test_sharded_remove_on_a_real_communicator():
  rng = np.random.RandomState(77)
  pools = [distinct_keys(rng, 150) for _ in range(2)]
  gone, rank = _sharded_scenario(1, pools)
  coll = hb.distribute.Collective(world_size=1, rank=0)
  with torch.cuda.stream(torch.cuda.Stream()):
    res = [rank(0, coll)]
    torch.cuda.current_stream().synchronize()
  coll.close()
  _check_sharded(1, pools, gone, res)


def test_sharded_remove_is_local_and_two_ranks_restore_onto_one_exactly():
  rng = np.random.RandomState(78)
  pools = [distinct_keys(rng, 150) for _ in range(2)]
  gone, rank = _sharded_scenario(2, pools)
  res = run_world(2, rank)
  _check_sharded(2, pools, gone, res)
  for c in range(2):
    for r in range(2):
      assert 0 < res[r]['evicted'][c] < 30                                  # both ranks owned some of the ids

  def restore(r, comm):
    tables = [HashTable(1024, S_DIMS[c], DEV, slab_size=8, init_scale=S_SCALE, seed=S_SEEDS[c], expiring=True)
              for c in range(2)]
    accums = [torch.full_like(t.table, S_ACC0) for t in tables]
    drv = ShardedHashGroupLookup(tables, comm, combiners=['sum', 'sum'], accums=accums,
                                 initial_accumulator_value=S_ACC0)
    drv.import_items([HashExport.cat([res[k]['base'][c] for k in range(2)]) for c in range(2)])
    sizes = [t.size() for t in tables]
    drv.import_items([HashExport.cat([res[k]['delta'][c] for k in range(2)]) for c in range(2)])
    out = dict(keys=[host(t.keys) for t in tables], rows=[host(t.table) for t in tables],
               accums=[host(x) for x in accums], sizes=sizes)
    drv.close()
    return out
  one = run_world(1, restore)[0]
  for c in range(2):
    assert one['sizes'][c] == 150
    cache = one['keys'][c]
    live = np.sort(cache[(cache != EMPTY) & (cache != TOMB)])
    np.testing.assert_array_equal(live, np.sort(pools[c][30:]))             # the same key set as the two ranks hold
    both = np.concatenate([res[r]['keys'][c] for r in range(2)])
    np.testing.assert_array_equal(live, np.sort(both[(both != EMPTY) & (both != TOMB)]))
    assert (one['accums'][c][cache == TOMB] == F32(S_ACC0)).all() and (cache == TOMB).sum() == 30
