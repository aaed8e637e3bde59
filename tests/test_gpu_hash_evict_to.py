"""Bounded hash tables on the GPU (hbk_hash_evict_to_n, HashTable.evict_to / maybe_evict and the lookups'
maybe_evict) against the numpy restatement of tests/support/hash_evict_to_ref.py.  Everything is integer and
compared bit for bit; the evicted set is a function of the arrays alone, so slot numbers never matter."""
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (HashGroupLookup, HashSequenceLookup, HashTable, ShardedHashGroupLookup,
                                         hash_evict_to)
from tests.support import hash_evict_to_ref as tref
from tests.support import hash_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
EMPTY, TOMB = tref.EMPTY, tref.TOMBSTONE
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def distinct_keys(rng, n):
  k = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=2 * n + 8, dtype=np.int64))
  rng.shuffle(k)
  return k[:n]


def padded(rng, cap, dim, pitch):
  """A companion of `dim` floats per row inside rows of `pitch`: (the view the call takes, the whole buffer)."""
  whole = dev(rng.rand(cap, pitch).astype(F32))
  return whole[:, :dim], whole


class State:
  """Host copies of everything a call may write."""

  def __init__(self, t, wholes=()):
    self.keys, self.last_seen, self.freq = host(t.keys), host(t.last_seen), host(t.freq)
    self.stats, self.counts = host(t.stats), host(t.counts)
    self.wholes = [host(w) for w in wholes]

  def live(self):
    return int(((self.keys != EMPTY) & (self.keys != TOMB)).sum())

  def restore(self, t, wholes=()):
    for name in ('keys', 'last_seen', 'freq', 'stats', 'counts'):
      getattr(t, name).copy_(dev(getattr(self, name)))
    for w, saved in zip(wholes, self.wholes):
      w.copy_(dev(saved))

  def apply(self, max_size, keep_freq=0, fills=()):
    """The reference's call on these copies; fills: (dim, value) per whole buffer.  Returns the report."""
    report, mask = tref.evict_to(self.keys, self.last_seen, self.freq, max_size, keep_freq,
                                 [(w, d, F32(v)) for w, (d, v) in zip(self.wholes, fills)])
    self.stats[0] += int(mask.sum())
    return report

  def check(self, t, wholes=()):
    for name in ('keys', 'last_seen', 'freq', 'stats', 'counts'):
      np.testing.assert_array_equal(host(getattr(t, name)), getattr(self, name), err_msg=name)
    for w, want in zip(wholes, self.wholes):
      np.testing.assert_array_equal(host(w), want)


def fill_over_steps(t, rng, groups, first_step=1):
  """Insert `groups` (arrays of keys) at consecutive steps, each step also touching a few keys of the step before.
  Returns the keys that got a slot."""
  held, prev = [], np.zeros(0, np.int64)
  for n, g in enumerate(groups):
    t.set_step(first_step + n)
    batch = np.concatenate([g, prev[:max(prev.size // 4, 0)]])
    slots = host(t.lookup_or_insert(dev(batch)))
    held.append(batch[slots >= 0])
    prev = g
  return np.unique(np.concatenate(held))


# ---- 1. bit for bit against the reference ---------------------------------------------------------------
@pytest.fixture(scope='module')
def filled_pair():
  """A table of 64 slabs x 8 and one of 37 x 3 (111 slots: a ragged last wave, a tile tail), filled over steps
  1..6, with a dim-5 and a dim-16 companion of pitch > dim each; their saved states."""
  rng = np.random.RandomState(11)
  out = []
  for slab_count, slab_size, per_step in ((64, 8, 55), (37, 3, 12)):
    cap = slab_count * slab_size
    t = HashTable(cap, 4, DEV, slab_size=slab_size, expiring=True)
    pool = distinct_keys(rng, 6 * per_step)
    fill_over_steps(t, rng, [pool[s * per_step:(s + 1) * per_step] for s in range(6)])
    (v5, w5), (v16, w16) = padded(rng, cap, 5, 8), padded(rng, cap, 16, 20)
    out.append((t, [(v5, 0.1), (v16, 0.0)], [w5, w16], State(t, [w5, w16])))
  return out


def _group_sizes(st):
  live = (st.keys != EMPTY) & (st.keys != TOMB)
  steps, sizes = np.unique(st.last_seen[live], return_counts=True)
  return steps, sizes


@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('case', ['above', 'exact', 'one', 'mid_group', 'boundary', 'zero'])
def test_bit_for_bit_against_the_reference(filled_pair, which, case):
  t, slots, wholes, saved = filled_pair[which]
  saved.restore(t, wholes)
  st = State(t, wholes)
  live = st.live()
  steps, sizes = _group_sizes(st)
  assert steps.size >= 3 and sizes[1] >= 2 and live > 0.5 * t.capacity
  max_size = {'above': live + 3, 'exact': live, 'one': live - 1, 'mid_group': live - int(sizes[0] + sizes[1] // 2),
              'boundary': live - int(sizes[0] + sizes[1]), 'zero': 0}[case]
  report = t.evict_to(max_size, slots=slots)
  want = st.apply(max_size, 0, [(5, 0.1), (16, 0.0)])
  np.testing.assert_array_equal(host(report), want)
  st.check(t, wholes)
  if case in ('above', 'exact'):
    saved.check(t, wholes)                                               # nothing at all was written
    assert want[3] == 0
  elif case == 'one':
    assert want.tolist() == [live, 1, int(steps[0]), int(sizes[0])]      # the whole oldest step leaves
  elif case in ('mid_group', 'boundary'):
    assert want[2] == steps[1] and want[3] == sizes[0] + sizes[1]
    assert (want[3] == want[1]) == (case == 'boundary')
  else:
    assert want[3] == live and t.size() == 0
  assert t.size() == live - int(want[3]) and (want[1] <= 0 or t.size() <= max_size)
  saved.restore(t, wholes)


# ---- 2. every digit and the sign ------------------------------------------------------------------------
def test_every_digit_and_the_sign():
  values = sorted([2 ** k for k in range(31)] + [0, -1, INT32_MIN, INT32_MAX])
  assert len(values) == 35 and values[0] == INT32_MIN and values[-1] == INT32_MAX
  rng = np.random.RandomState(12)
  t = HashTable(128, 4, DEV, slab_size=8, expiring=True)
  per_key = np.concatenate([[v] * (1 + k % 3) for k, v in enumerate(values)]).astype(np.int32)
  keys = distinct_keys(rng, per_key.size)
  slots = host(t.lookup_or_insert(dev(keys)))
  assert (slots >= 0).all()
  order = rng.permutation(per_key.size)
  t.last_seen[dev(slots[order])] = dev(per_key)                           # the values, spread over the slots
  st = State(t)
  for k, v in enumerate(values):
    live = st.live()
    max_size = 0 if k == len(values) - 1 else live - (1 + k % 3)          # down to the next boundary
    report = host(t.evict_to(max_size))
    want = st.apply(max_size)
    np.testing.assert_array_equal(report, want)
    assert want[2] == v and want[3] == 1 + k % 3, (k, v, want)
    st.check(t)
  assert t.size() == 0


# ---- 3. one hot bin, and none ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def wide_table():
  rng = np.random.RandomState(13)
  t = HashTable(8192, 4, DEV, slab_size=8, expiring=True)                 # 8 workgroups of 4 waves
  t.set_step(5)
  keys = distinct_keys(rng, 4900)
  slots = host(t.lookup_or_insert(dev(keys)))
  assert (slots >= 0).all()
  return t, State(t), rng


def test_one_hot_bin(wide_table):
  t, saved, _ = wide_table
  saved.restore(t)
  st = State(t)
  live = st.live()
  assert live == 4900 and (st.last_seen[st.keys != EMPTY] == 5).all()
  report = host(t.evict_to(live - 1))
  want = st.apply(live - 1)
  assert want.tolist() == [live, 1, 5, live]
  np.testing.assert_array_equal(report, want)
  st.check(t)
  assert t.size() == 0 and t.tombstones() == live


def test_no_hot_bin(wide_table):
  t, saved, rng = wide_table
  saved.restore(t)
  t.last_seen.copy_(dev(rng.randint(INT32_MIN, INT32_MAX + 1, size=t.capacity, dtype=np.int64).astype(np.int32)))
  st = State(t)
  live = st.live()
  for max_size in (live // 3, 7):
    report = host(t.evict_to(max_size))
    want = st.apply(max_size)
    np.testing.assert_array_equal(report, want)
    st.check(t)
    assert want[3] == want[1] and t.size() == max_size                    # distinct ages: the bound is met exactly


# ---- 4. keep_freq ----------------------------------------------------------------------------------------
def test_protected_keys_alone_exceed_the_bound():
  rng = np.random.RandomState(14)
  t = HashTable(512, 4, DEV, slab_size=8, expiring=True)
  keys = distinct_keys(rng, 300)
  often, rare = keys[:120], keys[120:]
  for step in (1, 2, 3):
    t.set_step(step)
    t.lookup_or_insert(dev(np.concatenate([often, rare[(step - 1) * 60:step * 60]])))
  view, whole = padded(rng, 512, 7, 8)
  st = State(t, [whole])
  report = host(t.evict_to(100, keep_freq=3, slots=[(view, 0.5)]))
  want = st.apply(100, 3, [(7, 0.5)])
  np.testing.assert_array_equal(report, want)
  assert want.tolist() == [300, 200, INT32_MAX, 180] and want[3] < want[1]
  st.check(t, [whole])
  assert (host(t.find(dev(often))) >= 0).all() and (host(t.find(dev(rare))) == -1).all()
  assert t.size() == 120 > 100


# ---- 5. N tables in one call -----------------------------------------------------------------------------
def test_35_tables_in_one_call():
  rng = np.random.RandomState(15)
  tables, states, wholes, slots, max_sizes = [], [], [], [], []
  for c in range(35):
    slab_size = int(rng.choice([1, 3, 8, 16, 64]))
    cap = slab_size * int(rng.randint(2, 40))
    t = HashTable(cap, 4, DEV, slab_size=slab_size, expiring=True)
    n = int(cap * rng.uniform(0.2, 0.7))
    pool = distinct_keys(rng, max(n, 4))
    fill_over_steps(t, rng, np.array_split(pool, 4), first_step=1 + c)
    view, whole = padded(rng, cap, 3, 4)
    tables.append(t)
    wholes.append(whole)
    slots.append([(view, 0.25)] if c % 2 else [])
    states.append(State(t, [whole] if c % 2 else []))
    live = states[-1].live()
    max_sizes.append(0 if c == 33 else live + c % 2 if c % 5 == 0 else int(rng.randint(0, live + 1)))
  before = [State(t, [w]) for t, w in zip(tables, wholes)]
  reports = hash_evict_to(tables, max_sizes, slots=slots)
  assert len(reports) == 35
  evicting = 0
  for c, t in enumerate(tables):
    want = states[c].apply(max_sizes[c], 0, [(3, 0.25)])
    np.testing.assert_array_equal(host(reports[c]), want, err_msg=str(c))
    states[c].check(t, [wholes[c]] if c % 2 else [])
    if want[1] <= 0:
      before[c].check(t, [wholes[c]])                                     # inside the bound: untouched
    else:
      evicting += 1
    np.testing.assert_array_equal(host(wholes[c])[:, 3], before[c].wholes[0][:, 3])
  assert evicting >= 20 and t.size() >= 0 and tables[33].size() == 0 and tables[34].size() <= max_sizes[34]


# ---- 6. the walk survives --------------------------------------------------------------------------------
def test_survivors_are_found_and_tombstones_reused():
  rng = np.random.RandomState(16)
  t = HashTable(256, 4, DEV, slab_size=2, expiring=True)
  pool = distinct_keys(rng, 330)
  held = fill_over_steps(t, rng, np.array_split(pool[:230], 6))           # load 0.9: keys spill past their slab
  st = State(t)
  live = st.live()
  assert live == held.size == 230 and t.failed() == 0
  home = np.array([ref.home_slab(int(k), t.slab_count) for k in held])
  where = host(t.find(dev(held)))
  assert (where >= 0).all() and (where // 2 != home).any()                # some do live outside their home slab
  t.evict_to(live // 2)
  want = st.apply(live // 2)
  st.check(t)
  gone = np.isin(held, st.keys, invert=True)
  assert gone.sum() == want[3] >= live - live // 2
  after = host(t.find(dev(held)))
  np.testing.assert_array_equal(after[~gone], where[~gone])
  assert (after[gone] == -1).all()
  t.set_step(9)
  new = pool[230:]
  slots = host(t.lookup_or_insert(dev(np.concatenate([new, held[~gone], new]))))
  assert (slots >= 0).all() and t.reused() > 0
  cache = host(t.keys)
  stored = cache[(cache != EMPTY) & (cache != TOMB)]
  assert np.unique(stored).size == stored.size == t.size() == int((~gone).sum()) + new.size
  np.testing.assert_array_equal(host(t.find(dev(held[~gone]))), where[~gone])


# ---- 7. captured graph -----------------------------------------------------------------------------------
def test_captured_call_replays_on_the_state_of_the_moment():
  rng = np.random.RandomState(17)
  t = HashTable(512, 4, DEV, slab_size=8, expiring=True)
  pool = distinct_keys(rng, 400)
  fill_over_steps(t, rng, np.array_split(pool[:150], 3))
  view, whole = padded(rng, 512, 5, 8)
  report = torch.zeros(4, dtype=torch.int32, device=DEV)
  t.evict_to(10 ** 6, slots=[(view, 0.1)], report=report)                 # outside the capture: the scratch exists
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      t.evict_to(120, slots=[(view, 0.1)], report=report)
  torch.cuda.synchronize()
  assert t.size() == 150                                                  # a capture runs nothing
  lo = 150
  for first_step, n in ((4, 90), (6, 70), (8, 0)):
    if n:
      fill_over_steps(t, rng, np.array_split(pool[lo:lo + n], 2), first_step=first_step)
      lo += n
    torch.cuda.synchronize()
    st = State(t, [whole])
    graph.replay()
    torch.cuda.synchronize()
    want = st.apply(120, 0, [(5, 0.1)])
    np.testing.assert_array_equal(host(report), want)
    st.check(t, [whole])
    assert (want[1] > 0) == (n > 0) and t.size() <= 120


# ---- 8. policy -------------------------------------------------------------------------------------------
def key_rows(keys, dim):
  """A row per key that names it: what a companion holds so that it can be followed through a rehash."""
  return ((keys % 1000).astype(F32)[:, None] + np.arange(dim, dtype=F32)[None, :] / 16).astype(F32)


def test_maybe_evict_bounds_the_table_and_moves_the_companions():
  rng = np.random.RandomState(18)
  t = HashTable(256, 4, DEV, slab_size=8, expiring=True)
  accum = torch.full((256, 4), 0.1, device=DEV)
  pool = distinct_keys(rng, 210)
  fill_over_steps(t, rng, np.array_split(pool[:100], 3))
  keys0, table0 = t.keys, t.table
  assert t.maybe_evict(0.75, 0.5, slots=[(accum, 0.1)]) is None and t.keys is keys0 and t.table is table0
  held = np.unique(np.concatenate([pool[:100], fill_over_steps(t, rng, np.array_split(pool[100:], 4), first_step=4)]))
  assert held.size == 210 > 0.75 * 256
  slots = host(t.find(dev(held)))
  accum[dev(slots)] = dev(key_rows(held, 4))
  rows_before = host(t.table)[slots]
  st = State(t)
  out = t.maybe_evict(0.75, 0.5, slots=[(accum, 0.1)])
  assert out is not None and len(out) == 1 and out[0] is not accum
  st.apply(128)
  survivors = held[np.isin(held, st.keys)]
  assert t.capacity == 256 and t.tombstones() == 0 and t.size() == survivors.size <= 128
  assert survivors.size > 128 - 70                                        # less than one step's keys below the bound
  now = host(t.find(dev(held)))
  assert ((now >= 0) == np.isin(held, survivors)).all()
  kept = now >= 0
  np.testing.assert_array_equal(host(out[0])[now[kept]], key_rows(held[kept], 4))
  np.testing.assert_array_equal(host(t.table)[now[kept]], rows_before[kept])
  free = np.setdiff1d(np.arange(256), now[kept])
  assert (host(out[0])[free] == F32(0.1)).all()
  # metadata moved with the keys too
  np.testing.assert_array_equal(host(t.last_seen)[now[kept]], st.last_seen[slots[kept]])
  # tombstones were the load: the rehash alone, nobody leaves
  t.evict(1)                                                              # step 7: everything not seen at 7 leaves
  size, dead = t.size(), t.tombstones()
  assert 0 < size <= 0.3 * 256 < size + dead
  assert t.maybe_evict(0.3, 0.3) is not None and t.tombstones() == 0 and t.size() == size and t.capacity == 256
  assert sorted(host(t.last_seen)[host(t.keys) != EMPTY].tolist()) == [7] * size


@pytest.mark.parametrize('kind', ['group', 'sequence'])
def test_lookups_rebind_and_an_evicted_id_starts_afresh(kind):
  rng = np.random.RandomState(19)
  dims, seeds, scale = [16, 6], [3, 4], 0.05
  tables = [HashTable(128, dims[c], DEV, slab_size=8, init_scale=scale, seed=seeds[c], expiring=True)
            for c in range(2)]
  look = HashGroupLookup(tables) if kind == 'group' else HashSequenceLookup(tables, 1)
  pools = [distinct_keys(rng, 110), distinct_keys(rng, 40)]               # table 0 passes 0.75, table 1 does not

  def forward(ids):
    out = look([dev(i) for i in ids], [None, None])
    return [host(o) for o in out] if kind == 'group' else [host(o)[:, 0, :] for o in out[0]]
  for step, part in enumerate(np.array_split(np.arange(110), 5), start=1):
    for t in tables:
      t.set_step(step)
    forward([pools[0][part], pools[1][part % 40]])
  accums = [torch.full_like(t.table, 0.1) for t in tables]
  for t, a in zip(tables, accums):                                        # trained rows, used slots
    t.table.add_(1.0)
    a.add_(2.0)
  for t in tables:
    t.set_step(6)
  oldest, newest = pools[0][:22], pools[0][88:]
  before = [host(tables[0].table)[host(tables[0].find(dev(newest)))], host(tables[1].table).copy()]
  rows1 = tables[1].table
  res = look.maybe_evict(0.75, 0.5, slots=[[(a, 0.1)] for a in accums])
  assert res[0] is not None and res[1] is None and tables[1].table is rows1
  assert tables[0].size() <= 64 and tables[0].capacity == 128 and tables[0].tombstones() == 0
  with pytest.raises(_lib.HbkError, match='launch'):                      # rebound: as a fresh object
    look.launch()
  assert (host(tables[0].find(dev(oldest))) == -1).all()
  got = forward([newest, pools[1][:22]])
  np.testing.assert_array_equal(got[0], before[0])                        # the survivors' rows, bit for bit
  np.testing.assert_array_equal(got[1], before[1][host(tables[1].find(dev(pools[1][:22])))])
  back = forward([oldest, pools[1][:22]])
  np.testing.assert_array_equal(back[0], ref.init_rows(oldest, dims[0], seeds[0], scale))
  where = host(tables[0].find(dev(oldest)))
  assert (where >= 0).all() and (host(res[0][0])[where] == F32(0.1)).all()
  assert (host(tables[0].last_seen)[where] == 6).all() and (host(tables[0].freq)[where] == 1).all()


# ---- 9. sharded -------------------------------------------------------------------------------------------
def run_world(world, fn):
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
  for th in threads:
    th.start()
  for th in threads:
    th.join(timeout=45)
  for cm in comms:
    cm.close()
  assert not errors, errors
  assert all(x is not None for x in results)
  return results


def test_sharded_maybe_evict_is_local_to_the_rank():
  dim, seed, scale, acc0 = 8, 5, 0.05, 0.1
  # rank 0 owns the even ids, rank 1 the odd ones: 110 against 30 keys in tables of 128 slots
  groups = [np.concatenate([np.arange(0, 44, 2) + 1000 * s, np.arange(1, 13, 2) + 1000 * s]).astype(np.int64)
            for s in range(1, 6)]

  def rank(r, comm):
    tables = [HashTable(128, dim, DEV, slab_size=8, init_scale=scale, seed=seed, expiring=True)]
    accums = [torch.full_like(tables[0].table, acc0)]
    drv = ShardedHashGroupLookup(tables, comm, combiners=['sum'], accums=accums, initial_accumulator_value=acc0)
    for step, g in enumerate(groups, start=1):
      tables[0].set_step(step)
      ids = dev(g[r::2].copy())                                           # each rank asks for half of the step's ids
      drv([ids], [None])
      drv.backward([torch.ones((ids.numel(), dim), device=DEV)], apply_lr=0.5, optimizer='adagrad', emit=False)
    size = tables[0].size()
    tables[0].set_step(6)
    rows = tables[0].table
    evicted = drv.maybe_evict(0.75, 0.5)                                  # rank 0 evicts and rebinds, rank 1 does nothing
    after, dead, moved = tables[0].size(), tables[0].tombstones(), tables[0].table is not rows
    ask = dev(np.concatenate([groups[0], groups[4]])[r::2].copy())        # the oldest and the newest step
    out = host(drv([ask], [None])[0])
    where = host(tables[0].find(dev(groups[0][groups[0] % 2 == r])))
    accum = host(drv.accums[0])[where]
    # a rehash behind the object's back on one rank: that rank is refused until it has rebound, then the step runs
    stale = None
    if r == 0:
      new = tables[0].rehash(slots=[(drv.accums[0], acc0)])
      try:
        drv._current()                                                    # pylint: disable=protected-access
      except _lib.InvalidArgumentError as e:
        stale = str(e)
      drv.rebind(accums=new)
    again = host(drv([ask], [None])[0])
    res = dict(size=size, after=after, moved=moved, evicted=evicted, stale=stale, out=out, again=again, ask=host(ask),
               accum=accum, tombstones=dead, capacity=tables[0].capacity)
    drv.close()
    return res

  res = run_world(2, rank)
  assert [x['size'] for x in res] == [110, 30]
  assert [x['evicted'] for x in res] == [[True], [False]] and [x['moved'] for x in res] == [True, False]
  assert [x['after'] for x in res] == [44, 30]                            # 110 -> 64 needs 46: three steps of 22
  assert [x['capacity'] for x in res] == [128, 128] and [x['tombstones'] for x in res] == [0, 0]
  assert res[0]['stale'] is not None and 'rebind' in res[0]['stale']
  for r in range(2):
    ask, out = res[r]['ask'], res[r]['out']
    fresh = ref.init_rows(ask, dim, seed, scale)
    old_even = (ask < 2000) & (ask % 2 == 0)                              # step 1's keys of rank 0: evicted, back afresh
    assert old_even.any() and not old_even.all()
    np.testing.assert_array_equal(out[old_even], fresh[old_even])
    assert (out[~old_even] != fresh[~old_even]).any(axis=1).all()         # every other key kept its trained row
    np.testing.assert_array_equal(res[r]['again'], out)
  assert (res[0]['accum'] == F32(acc0)).all()                             # ... and a fresh accumulator
  assert (res[1]['accum'] > F32(acc0)).all()


# ---- 10. model fuzz, keyed by id ---------------------------------------------------------------------------
def test_model_fuzz_keyed_by_id():
  rng = np.random.RandomState(20)
  tables = [HashTable(64, 4, DEV, slab_size=4, expiring=True), HashTable(96, 4, DEV, slab_size=8, expiring=True)]
  pools = [distinct_keys(rng, 48), distinct_keys(rng, 70)]                # below the capacity: no id is ever refused
  models = [{}, {}]
  step, n_evict_to, n_left = 1, 0, 0
  for x in tables:
    x.set_step(step)

  def read(t):
    keys, seen, freq = host(t.keys), host(t.last_seen), host(t.freq)
    live = (keys != EMPTY) & (keys != TOMB)
    assert np.unique(keys[live]).size == int(live.sum())
    return {int(k): (int(s), int(f)) for k, s, f in zip(keys[live], seen[live], freq[live])}
  for _ in range(300):
    c = int(rng.randint(2))
    t, m = tables[c], models[c]
    op = rng.choice(['translate', 'translate', 'step', 'evict_to', 'evict_to', 'evict', 'rehash'])
    if op == 'translate':
      ids = pools[c][rng.randint(0, pools[c].size, size=int(rng.randint(1, 40)))]
      slots = host(t.lookup_or_insert(dev(ids)))
      assert (slots >= 0).all()
      for k in ids.tolist():
        m[k] = (step, m.get(k, (0, 0))[1] + 1)
    elif op == 'step':
      step += int(rng.randint(1, 4))
      for x in tables:
        x.set_step(step)
    elif op == 'evict_to':
      max_size = int(rng.randint(0, len(m) + 3))
      keep = int(rng.choice([0, 0, 3]))
      report = host(t.evict_to(max_size, keep_freq=keep))
      need = len(m) - max_size
      gone = []
      if need > 0:
        ages = sorted(s for s, f in m.values() if keep == 0 or f < keep)
        cut = ages[need - 1] if len(ages) >= need else INT32_MAX
        gone = [k for k, (s, f) in m.items() if (keep == 0 or f < keep) and s <= cut]
        assert report.tolist() == [len(m), need, cut, len(gone)]
      else:
        assert report.tolist() == [len(m), need, 0, 0]
      for k in gone:
        del m[k]
      n_evict_to += 1
      n_left += len(gone)
      assert read(t) == m
      assert len(m) <= max_size or all(f >= keep for _, f in m.values())
    elif op == 'evict':
      ttl, keep = int(rng.randint(1, 6)), int(rng.choice([0, 4]))
      t.evict(ttl, keep_freq=keep)
      for k in [k for k, (s, f) in m.items() if step - s >= ttl and (keep == 0 or f < keep)]:
        del m[k]
    else:
      t.rehash()
  assert n_evict_to > 50 and n_left > 50
  for t, m in zip(tables, models):
    assert read(t) == m and t.size() == len(m)
