"""Expiring hash tables on the GPU (hbk_hash_insert_expiring_n, hbk_hash_evict_n, HashTable(expiring=True)):
the insert that reuses tombstones against the placement rule's invariants, the existing probe (C oracle and
device) and the sequential restatement where the two must agree; the sweep against numpy's predicate, bit for
bit; the metadata the translate launch writes; and a sequential numpy model keyed by raw id for the training
steps around an eviction.

Slot numbers depend on which workgroup claims first; they are compared with a host order only where the order
cannot matter (one key at a time, or every key's walk being the same single slab)."""
import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
import oracle
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import GroupLookupGrad, HashGroupLookup, HashTable, hash_evict, hash_translate
from hybridbackend_amd.training.saver import Saver
from tests.support import hash_expiry_ref as xref
from tests.support import hash_ref as ref
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
  """n distinct int64 keys over the full range, neither sentinel among them."""
  k = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=2 * n + 8, dtype=np.int64))
  rng.shuffle(k)
  return k[:n]


def with_duplicates(rng, keys, n):
  """n draws (n >= len(keys)) that name every key at least once."""
  out = np.concatenate([keys, keys[rng.randint(0, keys.size, size=n - keys.size)]])
  rng.shuffle(out)
  return out


def homed_in(slab, slab_count, n, start=1):
  """The first n positive keys from `start` whose home slab is `slab`."""
  out, k = [], start
  while len(out) < n:
    if ref.home_slab(k, slab_count) == slab:
      out.append(k)
    k += 1
  return np.array(out, np.int64)


def insert_at(t, step, keys):
  t.set_step(step)
  return host(t.lookup_or_insert(dev(keys)))


def check_live(t, keys, slots):
  """What must hold of ANY correct concurrent insert, tombstones or not: every slot holds its key, no key is
  stored twice, and the probes -- which stop at the first slab with an EMPTY slot -- find every key there."""
  cache = host(t.keys)
  assert (slots >= 0).all() and (slots < t.capacity).all()
  np.testing.assert_array_equal(cache[slots], keys)
  live = cache[(cache != EMPTY) & (cache != TOMB)]
  assert np.unique(live).size == live.size
  assert np.unique(slots).size == np.unique(keys).size
  np.testing.assert_array_equal(oracle.cache_probe(cache, t.slab_size, keys), slots)
  hit, n_miss = hb.embedding.cache.probe(t.keys, dev(keys), t.slab_size)
  np.testing.assert_array_equal(host(hit), slots)
  assert int(n_miss.item()) == 0
  np.testing.assert_array_equal(host(t.find(dev(keys))), slots)
  np.testing.assert_array_equal(host(t.keys), cache)                       # a find writes nothing


# ---- 1. invariants with tombstones ----------------------------------------------------------------------
@pytest.mark.parametrize('slab_count', [1, 3, 257])
@pytest.mark.parametrize('slab_size', [5, 16, 64])
def test_invariants_with_tombstones(slab_size, slab_count):
  rng = np.random.RandomState(100 * slab_size + slab_count)
  cap = slab_size * slab_count
  n = max(3 * cap // 4, 2)
  pool = distinct_keys(rng, 2 * cap)
  g1, g2 = pool[:n // 2], pool[n // 2:n]
  t = HashTable(cap, 4, DEV, slab_size=slab_size, expiring=True)
  k1 = with_duplicates(rng, g1, min(20000, 2 * g1.size + 3))
  s1 = insert_at(t, 1, k1)
  s2 = insert_at(t, 5, g2)
  assert (s1 >= 0).all() and (s2 >= 0).all() and t.size() == n and t.failed() == 0
  before = host(t.keys)
  empties = int((before == EMPTY).sum())
  assert empties == cap - n
  t.set_step(6)
  t.evict(steps_to_live=3)
  after = host(t.keys)
  old = np.unique(s1)
  assert (after[old] == TOMB).all()
  rest = np.setdiff1d(np.arange(cap), old)
  np.testing.assert_array_equal(after[rest], before[rest])                 # group 2 bit for bit
  assert (t.evicted(), t.tombstones(), t.size(), t.reused()) == (g1.size, g1.size, g2.size, 0)
  assert int((after == EMPTY).sum()) == empties
  assert (host(t.find(dev(g1))) == -1).all()
  check_live(t, g2, s2)
  assert not host(t.last_seen)[old].any() and not host(t.freq)[old].any()
  # new keys and group 2, with duplicates
  n_new = g1.size if slab_count == 1 else g1.size + (cap - n) // 2
  new = pool[n:n + n_new]
  both = np.concatenate([new, g2])
  keys = with_duplicates(rng, both, min(20000, 3 * both.size + 5))
  slots = insert_at(t, 7, keys)
  check_live(t, keys, slots)
  np.testing.assert_array_equal(host(t.find(dev(g2))), s2)                 # group 2 stayed where it was
  assert t.size() == g2.size + n_new and t.failed() == 0
  assert 0 < t.reused() <= g1.size
  if slab_count == 1:
    # one slab, one walk: every new key takes a tombstone
    assert t.reused() == n_new and int((host(t.keys) == EMPTY).sum()) == empties
  else:
    assert int((host(t.keys) == EMPTY).sum()) == cap - (g2.size + n_new) - t.tombstones()


# ---- 2. the spilled key ---------------------------------------------------------------------------------
def test_the_spilled_key_is_found_behind_a_tombstone_not_stored_twice():
  slab_size, slab_count = 4, 8
  k = homed_in(2, slab_count, 6)
  t = HashTable(slab_size * slab_count, 4, DEV, slab_size=slab_size, expiring=True)
  assert sorted(insert_at(t, 1, k[:4]).tolist()) == [8, 9, 10, 11]
  assert insert_at(t, 5, k[4:5]).tolist() == [12]                          # slab 2 is full: it spills into slab 3
  t.set_step(6)
  t.evict(3)
  cache = host(t.keys)
  assert (cache[8:12] == TOMB).all() and cache[12] == k[4] and t.evicted() == 4
  assert insert_at(t, 6, k[4:5]).tolist() == [12]
  np.testing.assert_array_equal(host(t.keys), cache)
  assert (t.size(), t.reused()) == (1, 0)
  assert insert_at(t, 6, k[5:6]).tolist() == [8]                           # the first tombstone of its walk
  assert (t.size(), t.reused()) == (2, 1)
  want = cache.copy()
  want[8] = k[5]
  np.testing.assert_array_equal(host(t.keys), want)
  # the restatement tells the same story
  c = np.full(32, EMPTY, np.int64)
  xref.insert(c, slab_size, k[:4])
  xref.insert(c, slab_size, k[4:5])
  c[8:12] = TOMB
  assert xref.insert(c, slab_size, k[4:6])[0].tolist() == [12, 8]


# ---- 3. one key, many writers ---------------------------------------------------------------------------
def test_one_key_4096_times_into_a_slab_of_tombstones():
  slab_size, slab_count, dim = 16, 64, 8
  t = HashTable(slab_size * slab_count, dim, DEV, slab_size=slab_size, init_scale=0.5, seed=3, expiring=True)
  k = homed_in(9, slab_count, 17)
  assert sorted(insert_at(t, 1, k[:16]).tolist()) == list(range(9 * 16, 10 * 16))
  t.set_step(4)
  t.evict(3)
  assert t.tombstones() == 16 and t.size() == 0
  slots = insert_at(t, 4, np.full(4096, k[16], np.int64))
  assert (slots == 9 * 16).all()                                           # slot 0 of the home slab
  cache = host(t.keys)
  assert int((cache == k[16]).sum()) == 1 and int((cache == TOMB).sum()) == 15
  assert (t.size(), t.reused(), t.failed()) == (1, 1, 0)
  np.testing.assert_array_equal(host(t.table)[9 * 16], ref.init_row(int(k[16]), dim, 3, 0.5))
  assert int(t.freq[9 * 16].item()) == 4096 and int(t.last_seen[9 * 16].item()) == 4
  assert int(t.freq.sum().item()) == 4096


def test_20000_draws_of_300_values_into_a_half_tombstoned_table():
  rng = np.random.RandomState(31)
  slab_size, slab_count = 16, 64
  pool = distinct_keys(rng, 512 + 256 + 300)
  t = HashTable(slab_size * slab_count, 4, DEV, slab_size=slab_size, expiring=True)
  insert_at(t, 1, pool[:512])
  s_live = insert_at(t, 5, pool[512:768])
  t.set_step(6)
  t.evict(3)
  assert (t.tombstones(), t.size()) == (512, 256)
  values = pool[768:]
  keys = values[rng.randint(0, 300, size=20000)]
  assert np.unique(keys).size == 300
  slots = insert_at(t, 7, keys)
  check_live(t, keys, slots)
  assert t.size() == 556 and t.failed() == 0
  np.testing.assert_array_equal(host(t.find(dev(pool[512:768]))), s_live)
  values, counts = np.unique(keys, return_counts=True)
  np.testing.assert_array_equal(host(t.freq)[host(t.find(dev(values)))], counts)


# ---- 4. metadata ----------------------------------------------------------------------------------------
def test_freq_and_last_seen_follow_the_calls():
  rng = np.random.RandomState(41)
  t = HashTable(16 * 24, 4, DEV, slab_size=16, expiring=True)
  pool = distinct_keys(rng, 200)
  calls = [(2, pool[:120]), (4, pool[60:160]), (9, pool[100:200])]
  count, last = {}, {}
  for step, part in calls:
    keys = with_duplicates(rng, part, 5 * part.size)
    insert_at(t, step, keys)
    for k, c in zip(*np.unique(keys, return_counts=True)):
      count[int(k)] = count.get(int(k), 0) + int(c)
      last[int(k)] = step
  slots = host(t.find(dev(pool)))
  assert (slots >= 0).all()
  freq, seen = host(t.freq), host(t.last_seen)
  np.testing.assert_array_equal(freq[slots], [count[int(k)] for k in pool])
  np.testing.assert_array_equal(seen[slots], [last[int(k)] for k in pool])
  free = np.setdiff1d(np.arange(t.capacity), slots)
  assert not freq[free].any() and not seen[free].any()
  # a find touches neither array, whatever the step
  t.set_step(50)
  t.find(dev(with_duplicates(rng, pool, 700)))
  hash_translate([t], [dev(pool)], insert=False)
  np.testing.assert_array_equal(host(t.freq), freq)
  np.testing.assert_array_equal(host(t.last_seen), seen)


def test_a_refused_occurrence_touches_nothing_and_the_counter_saturates():
  t = HashTable(5, 4, DEV, slab_size=5, expiring=True)
  keys = np.array([11, 12, 13, 14, 15], np.int64)
  slots = insert_at(t, 3, keys)
  assert sorted(slots.tolist()) == [0, 1, 2, 3, 4]
  freq, seen = host(t.freq), host(t.last_seen)
  got = insert_at(t, 8, np.array([16, 16, EMPTY, TOMB, 17], np.int64))     # full; neither sentinel is ever stored
  assert (got == -1).all() and t.failed() == 5 and t.size() == 5
  np.testing.assert_array_equal(host(t.freq), freq)
  np.testing.assert_array_equal(host(t.last_seen), seen)
  np.testing.assert_array_equal(np.sort(host(t.keys)), keys)
  # 2^30 stays 2^30; one below it takes its last increment
  t.freq[int(slots[0])] = 2 ** 30
  t.freq[int(slots[1])] = 2 ** 30 - 1
  insert_at(t, 9, np.array([11, 12, 11, 13], np.int64))
  freq = host(t.freq)
  assert freq[slots[0]] == 2 ** 30 and freq[slots[1]] == 2 ** 30 and freq[slots[2]] == 2
  assert host(t.last_seen)[slots].tolist() == [9, 9, 9, 3, 3]


# ---- 5. the predicate, exact ----------------------------------------------------------------------------
FILL_SETS = [
  [],
  [(1, 1, 0.5), (16, 20, 0.1), (67, 67, -2.0), (16, 16, 0.0)],
  [(1, 3, 7.0), (67, 70, 0.25)],
]


@pytest.mark.parametrize('keep_freq', [0, 3])
@pytest.mark.parametrize('slab_count', [3, 257])
def test_sweep_equals_numpys_predicate_bit_for_bit(slab_count, keep_freq):
  rng = np.random.RandomState(500 + slab_count + keep_freq)
  slab_size, step, ttl = 5, 100, 10
  cap = slab_size * slab_count
  keys = distinct_keys(rng, cap)
  kind = rng.randint(0, 6, size=cap)
  keys[kind == 0] = EMPTY
  keys[kind == 1] = TOMB
  seen = rng.choice(np.array([89, 90, 91, 100, 0, 101], np.int32), size=cap)     # age 11, ttl, ttl - 1, 0, 100, -1
  freq = rng.choice(np.array([0, 2, 3, 4, 2 ** 30], np.int32), size=cap)          # keep_freq - 1, keep_freq, above
  if slab_count == 3:
    # every side of every boundary by hand: (last_seen, freq)
    keys[:6] = np.arange(1, 7)
    seen[:6] = [90, 91, 90, 90, 89, 91]
    freq[:6] = [2, 2, 3, 4, 2, 3]
  for fills in FILL_SETS:
    t = HashTable(cap, 4, DEV, slab_size=slab_size, expiring=True)
    t.keys.copy_(dev(keys))
    t.last_seen.copy_(dev(seen))
    t.freq.copy_(dev(freq))
    t.set_step(step)
    bases = [rng.randn(cap, pitch).astype(F32) for _, pitch, _ in fills]
    d_bases = [dev(b) for b in bases]
    comp = [(d[:, :dim], value) for d, (dim, _, value) in zip(d_bases, fills)]
    # steps_to_live == 0 evicts nothing
    t.evict(0, keep_freq, slots=comp)
    np.testing.assert_array_equal(host(t.keys), keys)
    assert t.evicted() == 0
    t.evict(ttl, keep_freq, slots=comp)
    c, s, f = keys.copy(), seen.copy(), freq.copy()
    want = [b.copy() for b in bases]
    mask = xref.evict(c, s, f, step, ttl, keep_freq,
                      [(w, dim, F32(value)) for w, (dim, _, value) in zip(want, fills)])
    assert 0 < int(mask.sum()) < int(((keys != EMPTY) & (keys != TOMB)).sum())
    if slab_count == 3:
      assert mask[:6].tolist() == [True, False, keep_freq == 0, keep_freq == 0, True, False]
    np.testing.assert_array_equal(host(t.keys), c)
    np.testing.assert_array_equal(host(t.last_seen), s)
    np.testing.assert_array_equal(host(t.freq), f)
    assert t.evicted() == int(mask.sum())                                   # EMPTY and TOMBSTONE never count
    for d, w in zip(d_bases, want):
      assert host(d).tobytes() == w.tobytes()                               # rows filled; padding and the rest untouched
    # a second sweep finds nothing left
    t.evict(ttl, keep_freq, slots=comp)
    assert t.evicted() == int(mask.sum())
    np.testing.assert_array_equal(host(t.keys), c)


def test_hash_evict_sweeps_n_tables_in_one_call():
  rng = np.random.RandomState(57)
  tables = [HashTable(cap, 4, DEV, slab_size=ss, expiring=True) for cap, ss in ((160, 16), (1000, 8), (64, 64))]
  accums = [torch.full((t.capacity, 16), 0.5, device=DEV) for t in tables]
  olds = []
  for t in tables:
    keys = distinct_keys(rng, t.capacity // 2)
    insert_at(t, 1, keys[:keys.size // 2])
    insert_at(t, 7, keys[keys.size // 2:])
    t.set_step(8)
    olds.append(host(t.find(dev(keys[:keys.size // 2]))))
  hash_evict(tables, 5, slots=[[(a, 0.1)] for a in accums])
  for t, a, old in zip(tables, accums, olds):
    assert t.evicted() == old.size == t.tombstones()
    want = np.full((t.capacity, 16), F32(0.5))
    want[old] = F32(0.1)
    np.testing.assert_array_equal(host(a), want)


# ---- 6. end to end against a sequential model keyed by raw id -----------------------------------------------
def test_training_across_an_eviction_equals_the_sequential_model():
  rng = np.random.RandomState(60)
  B, dim, lr, scale, acc0 = 96, 16, 0.1, 0.05, 0.1
  seeds = [3, 4]
  tables = [HashTable(256, dim, DEV, slab_size=ss, init_scale=scale, seed=seeds[c], expiring=True)
            for c, ss in enumerate((16, 5))]
  accums = [torch.full_like(t.table, acc0) for t in tables]
  hgl = HashGroupLookup(tables, combiners='sum')
  grad = GroupLookupGrad(hgl.lookup, accums=accums, deterministic=True)
  pools = [distinct_keys(rng, 70) for _ in range(2)]
  old = [p[:30] for p in pools]
  kept = [p[30:50] for p in pools]
  fresh = [p[50:] for p in pools]
  uniq = [np.sort(p) for p in pools]
  W = [ref.init_rows(uniq[c], dim, seeds[c], scale) for c in range(2)]
  A = [np.full_like(W[c], F32(acc0)) for c in range(2)]

  def train(step, parts):
    ids = [with_duplicates(rng, parts[c], B) for c in range(2)]
    grads = [rng.randn(B, dim).astype(F32) for _ in range(2)]
    for t in tables:
      t.set_step(step)
    outs = hgl([dev(i) for i in ids], [None, None])
    index = [np.searchsorted(uniq[c], ids[c]) for c in range(2)]
    for c in range(2):
      np.testing.assert_array_equal(host(outs[c]), W[c][index[c]])         # one id per sample, summed: the row
    grad(hgl.slots, [dev(g) for g in grads], [None, None], apply_lr=lr, optimizer='adagrad')
    for c in range(2):
      terms, r, valid = model.terms32(uniq[c].size, index[c], None, None, 'sum', grads[c])
      u, sums = model.seq_row_sums(terms, r, valid)
      model.adagrad_step(W[c], A[c], u, sums, lr)

  def check(c, keys):
    slots = host(tables[c].find(dev(keys)))
    assert (slots >= 0).all()
    at = np.searchsorted(uniq[c], keys)
    np.testing.assert_array_equal(host(tables[c].table)[slots], W[c][at])
    np.testing.assert_array_equal(host(accums[c])[slots], A[c][at])

  for step in (1, 2):
    train(step, [np.concatenate([old[c], kept[c]]) for c in range(2)])
  for step in (3, 4, 5):
    train(step, kept)
  for t in tables:
    t.set_step(6)
  hash_evict(tables, 3, slots=[[(a, acc0)] for a in accums])
  for c in range(2):
    assert (tables[c].evicted(), tables[c].size()) == (30, 20)
    assert (host(tables[c].find(dev(old[c]))) == -1).all()
    check(c, kept[c])                                                      # a kept id is unaffected
    # the model forgets the evicted ids: they start again as fresh ids do
    at = np.searchsorted(uniq[c], old[c])
    W[c][at] = ref.init_rows(old[c], dim, seeds[c], scale)
    A[c][at] = F32(acc0)
    assert (host(accums[c])[host(tables[c].keys) == TOMB] == F32(acc0)).all()
  # inference after the eviction: an evicted id reads as a zero row and nothing is inserted
  state = [(host(t.keys), host(t.freq), host(t.last_seen), host(t.counts)) for t in tables]
  ids = [np.concatenate([old[c][:8], kept[c][:8]]) for c in range(2)]
  outs = HashGroupLookup(tables, combiners='sum', train=False)([dev(i) for i in ids], [None, None])
  for c in range(2):
    got = host(outs[c])
    assert not got[:8].any()
    np.testing.assert_array_equal(got[8:], W[c][np.searchsorted(uniq[c], kept[c][:8])])
    for now, was in zip((host(tables[c].keys), host(tables[c].freq), host(tables[c].last_seen),
                         host(tables[c].counts)), state[c]):
      np.testing.assert_array_equal(now, was)
  # evicted ids come back beside fresh and kept ones: train() checks the forward rows (init_row again) and
  # steps the model, in which an evicted id and a fresh id are the same thing
  parts = [np.concatenate([old[c][:12], fresh[c], kept[c]]) for c in range(2)]
  train(7, parts)
  for c in range(2):
    check(c, parts[c])
    assert tables[c].size() == 20 + 12 + 20 and tables[c].reused() > 0 and tables[c].failed() == 0
  train(8, parts)
  for c in range(2):
    check(c, parts[c])


# ---- 7. captured launches -------------------------------------------------------------------------------
def test_captured_launch_follows_the_step_and_a_captured_sweep_evicts():
  rng = np.random.RandomState(90)
  B, dim = 200, 16
  tables = [HashTable(1024, dim, DEV, slab_size=ss, expiring=True) for ss in (8, 16)]
  hgl = HashGroupLookup(tables, combiners='sum')
  pools = [distinct_keys(rng, 300) for _ in range(2)]

  def batch(lo, hi):
    return [p[lo:hi][rng.randint(0, hi - lo, size=B)] for p in pools]
  first = batch(0, 100)
  bufs = [dev(i) for i in first]
  outs = [torch.empty((B, dim), dtype=torch.float32, device=DEV) for _ in range(2)]
  for t in tables:
    t.set_step(1)
  hgl(bufs, [None, None], outs)                 # warm-up outside the capture: descriptors and slot buffers exist
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph, sweep = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      hgl.launch()
    with torch.cuda.graph(sweep, stream=s):
      hash_evict(tables, 4)
  torch.cuda.synchronize()
  last = [{int(k): 1 for k in np.unique(i)} for i in first]
  for step, (lo, hi) in ((3, (50, 150)), (6, (120, 220))):
    new = batch(lo, hi)
    for b, i in zip(bufs, new):
      b.copy_(dev(i))
    for t in tables:
      t.set_step(step)
    graph.replay()
    torch.cuda.synchronize()
    for c in range(2):
      last[c].update({int(k): step for k in np.unique(new[c])})
      slots = host(hgl.slots[c])
      np.testing.assert_array_equal(host(tables[c].keys)[slots], new[c])
      assert (host(tables[c].last_seen)[slots] == step).all()
      assert tables[c].size() == len(last[c])
      np.testing.assert_array_equal(host(outs[c]), ref.init_rows(new[c], dim, 0, 1e-3))
  for t in tables:
    t.set_step(7)
  sweep.replay()                                 # ages: step 1 -> 6, step 3 -> 4, step 6 -> 1
  torch.cuda.synchronize()
  for c in range(2):
    keys = np.array(sorted(last[c]), np.int64)
    gone = np.array([7 - last[c][int(k)] >= 4 for k in keys])
    slots = host(tables[c].find(dev(keys)))
    assert ((slots == -1) == gone).all() and gone.any() and not gone.all()
    assert tables[c].evicted() == int(gone.sum())


# ---- 8. compact, items, load, checkpoint ------------------------------------------------------------------
def test_compact_items_load_and_checkpoint(tmp_path):
  rng = np.random.RandomState(80)
  slab_size, slab_count, dim = 16, 32, 8
  cap = slab_size * slab_count
  t = HashTable(cap, dim, DEV, slab_size=slab_size, expiring=True)
  accum = torch.full((cap, dim), 0.1, device=DEV)
  pool = distinct_keys(rng, 460)
  insert_at(t, 1, pool[:250])
  insert_at(t, 5, with_duplicates(rng, pool[250:400], 400))
  t.set_step(6)
  t.evict(3, slots=[(accum, 0.1)])
  insert_at(t, 7, pool[400:460])
  live = np.sort(pool[250:460])
  slots = host(t.find(dev(live)))
  assert (slots >= 0).all() and t.size() == live.size and t.tombstones() == 250 - t.reused() > 0
  # rows and accumulators that are no longer their start
  t.table[dev(slots)] = dev(rng.randn(live.size, dim).astype(F32))
  accum[dev(slots)] = dev(rng.rand(live.size, dim).astype(F32) + F32(1))
  rows, acc = host(t.table)[slots], host(accum)[slots]
  freq, seen = host(t.freq)[slots], host(t.last_seen)[slots]
  keys, item_rows = t.items()                                              # tombstones are not items
  np.testing.assert_array_equal(host(keys), live)
  np.testing.assert_array_equal(host(item_rows), rows)
  failed = t.failed()
  t.compact(slots=[(accum, 0.1)])
  assert (t.tombstones(), t.evicted(), t.reused(), t.size(), t.failed()) == (0, 0, 0, live.size, failed)
  cache = host(t.keys)
  assert int((cache == EMPTY).sum()) == cap - live.size
  new = host(t.find(dev(live)))
  check_live(t, live, new)
  np.testing.assert_array_equal(host(t.table)[new], rows)
  np.testing.assert_array_equal(host(accum)[new], acc)
  np.testing.assert_array_equal(host(t.freq)[new], freq)
  np.testing.assert_array_equal(host(t.last_seen)[new], seen)
  free = np.setdiff1d(np.arange(cap), new)
  assert (host(accum)[free] == F32(0.1)).all() and not host(t.freq)[free].any() and not host(t.last_seen)[free].any()
  # a table with tombstones through a checkpoint of the raw arrays
  insert_at(t, 9, pool[:40])
  t.set_step(12)
  t.evict(3, keep_freq=2)                                                  # the ids seen once at step 9 or before
  assert t.tombstones() > 0
  prefix = str(tmp_path / 'ckpt')
  Saver().save(prefix, t.variables('user'))
  other = HashTable(cap, dim, DEV, slab_size=slab_size, expiring=True)
  Saver().restore(prefix, other.variables('user'))
  other.recount()
  assert other.size() == t.size() and other.tombstones() == t.tombstones() and other.evicted() == 0
  for a, b in zip(t.items(), other.items()):
    np.testing.assert_array_equal(host(a), host(b))
  np.testing.assert_array_equal(host(other.freq), host(t.freq))
  np.testing.assert_array_equal(host(other.last_seen), host(t.last_seen))
  # items / load into another geometry leaves the tombstones behind
  bigger = HashTable(2 * cap, dim, DEV, slab_size=8, expiring=True)
  bigger.load(*t.items())
  assert bigger.size() == t.size() and bigger.tombstones() == 0
  for a, b in zip(t.items(), bigger.items()):
    np.testing.assert_array_equal(host(a), host(b))


# ---- 9. plain tables are unchanged ------------------------------------------------------------------------
def test_mixed_translate_gives_the_plain_column_the_plain_entrys_results():
  rng = np.random.RandomState(95)
  slab_size, slab_count, dim = 16, 257, 8
  cap = slab_size * slab_count
  keys = distinct_keys(rng, cap // 8)
  keys[:2] = [TOMB, -1]                                                    # INT64_MIN + 1 is an ordinary key there
  draws = with_duplicates(rng, keys, 3 * keys.size)
  want_cache = np.full(cap, EMPTY, np.int64)
  ref.fill(want_cache, slab_size, keys)
  assert max(len(s) for s in ref.slab_sets(want_cache, slab_size)) < slab_size     # no slab overflows
  # the plain entry alone, on a fresh cache
  alone = HashTable(cap, dim, DEV, slab_size=slab_size, init_scale=0.5, seed=5)
  cols = (_lib.HashColumn * 1)()
  alone._describe(cols[0])
  d_draws = dev(draws)
  s_alone = torch.empty(draws.size, dtype=torch.int64, device=DEV)
  cols[0].keys, cols[0].n_keys, cols[0].slots = d_draws.data_ptr(), draws.size, s_alone.data_ptr()
  _lib.check(_lib.lib().hbk_hash_insert_n(1, cols, 1, _lib.current_stream(torch.device(DEV))))
  # the same keys through a mixed call
  plain = HashTable(cap, dim, DEV, slab_size=slab_size, init_scale=0.5, seed=5)
  a, b = (HashTable(cap, dim, DEV, slab_size=slab_size, expiring=True) for _ in range(2))
  for t in (a, b):
    t.set_step(2)
  got = hash_translate([a, plain, b], [d_draws, d_draws, d_draws])
  assert ref.slab_sets(host(plain.keys), slab_size) == ref.slab_sets(host(alone.keys), slab_size) == \
      ref.slab_sets(want_cache, slab_size)
  assert host(plain.counts).tolist() == host(alone.counts).tolist() == [keys.size, 0]
  for t, s in ((plain, got[1]), (alone, s_alone)):
    s = host(s)
    np.testing.assert_array_equal(host(t.keys)[s], draws)
    assert int((host(t.keys) == TOMB).sum()) == 1
    np.testing.assert_array_equal(host(t.table)[s], ref.init_rows(draws, dim, 5, 0.5))
  # the expiring columns of the same call refuse the sentinel and match the plain placement otherwise
  for t, s in ((a, got[0]), (b, got[2])):
    s = host(s)
    assert (s[draws == TOMB] == -1).all() and (s[draws != TOMB] >= 0).all()
    assert t.size() == keys.size - 1 and t.failed() == int((draws == TOMB).sum())
    sets = ref.slab_sets(want_cache, slab_size)
    assert ref.slab_sets(host(t.keys), slab_size) == [[k for k in one if k != TOMB] for one in sets]
    assert (host(t.last_seen)[s[s >= 0]] == 2).all()
  # a mixed find, and a mixed HashGroupLookup
  found = hash_translate([a, plain], [d_draws, d_draws], insert=False)
  np.testing.assert_array_equal(host(found[0]), host(got[0]))
  np.testing.assert_array_equal(host(found[1]), host(got[1]))
  hgl = HashGroupLookup([plain, a], combiners='sum')
  outs = hgl([d_draws, d_draws], [None, None])
  np.testing.assert_array_equal(host(hgl.slots[0]), host(got[1]))
  np.testing.assert_array_equal(host(hgl.slots[1]), host(got[0]))
  np.testing.assert_array_equal(host(outs[0]), ref.init_rows(draws, dim, 5, 0.5))
  hgl.launch()
  torch.cuda.synchronize()
  np.testing.assert_array_equal(host(hgl.slots[0]), host(got[1]))
  np.testing.assert_array_equal(host(hgl.slots[1]), host(got[0]))
