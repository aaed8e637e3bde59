"""Bounded hash tables in LFU order on the GPU (hbk_hash_evict_to_lfu_n, hbk_hash_evict_to_lfu_select_n,
hbk_hash_spill_lfu_n; ``order='lfu'`` on HashTable.evict_to / spill_to / maybe_evict, the N-table functions and the
lookups' maybe_evict; HashTable.age_freq) against the numpy restatement of tests/support/hash_evict_lfu_ref.py.
Everything is integer or a copy and compared bit for bit: keys, last_seen, freq, companions, stats and the report.
The evicted set is a function of the arrays alone, so most tables are written directly: neither call looks at where
a key hashes to."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (GroupLookupGrad, HashGroupLookup, HashSpillStore, HashTable,
                                         ShardedHashGroupLookup, hash_evict_to, hash_evict_to_select, hash_spill)
from hybridbackend_amd.embedding import hashtable as _ht
from tests.support import hash_evict_lfu_ref as lref
from tests.support import hash_evict_to_ref as tref
from tests.support import hash_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
EMPTY, TOMB = lref.EMPTY, lref.TOMBSTONE
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
NAMES = ('keys', 'last_seen', 'freq', 'stats', 'counts', 'table')


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
  """Host copies of everything a call may write (and of the rows, which no call here may write)."""

  def __init__(self, t, wholes=()):
    for name in NAMES:
      setattr(self, name, host(getattr(t, name)))
    self.wholes = [host(w) for w in wholes]

  def live(self):
    return int(((self.keys != EMPTY) & (self.keys != TOMB)).sum())

  def restore(self, t, wholes=()):
    for name in NAMES:
      getattr(t, name).copy_(dev(getattr(self, name)))
    for w, saved in zip(wholes, self.wholes):
      w.copy_(dev(saved))

  def apply(self, max_size, keep_freq=0, fills=()):
    """The restatement's evict_to on these copies; fills: (dim, value) per whole buffer.  Returns (report, mask)."""
    report, mask = lref.evict_to(self.keys, self.last_seen, self.freq, max_size, keep_freq,
                                 [(w, d, F32(v)) for w, (d, v) in zip(self.wholes, fills)])
    self.stats[0] += int(mask.sum())
    return report, mask

  def spill(self, selection, keep_freq, dims_values, out_capacity=None):
    """The restatement's spill of this state: (export, the State afterwards, n_evicted, count)."""
    moves = [(self.table, self.table.shape[1]), (self.last_seen, 1), (self.freq, 1)]
    moves += [(w, d) for w, (d, _) in zip(self.wholes, dims_values)]
    comps = [(w, d, F32(v)) for w, (d, v) in zip(self.wholes, dims_values)]
    export, after, n_evicted, count = lref.spill(self.keys, self.last_seen, self.freq, selection, keep_freq, moves,
                                                 comps, out_capacity)
    st = State.__new__(State)
    st.keys, st.last_seen, st.freq = after['cache'], after['last_seen'], after['freq']
    st.stats, st.counts, st.table, st.wholes = self.stats.copy(), self.counts, self.table, after['companions']
    st.stats[0] += n_evicted
    return export, st, n_evicted, count

  def check(self, t, wholes=()):
    for name in NAMES:
      np.testing.assert_array_equal(host(getattr(t, name)), getattr(self, name), err_msg=name)
    for w, want in zip(wholes, self.wholes):
      np.testing.assert_array_equal(host(w), want)


def written_table(rng, cap, slab_size, freq, seen, dim=4, tombstones=3):
  """A table whose arrays are written directly: freq.size keys at random slots with these freq / last_seen values
  (any int32), a few tombstones, random rows.  The counters are set from the arrays."""
  t = HashTable(cap, dim, DEV, slab_size=slab_size, expiring=True)
  assert t.capacity == cap
  freq, seen = np.asarray(freq, np.int64).astype(np.int32), np.asarray(seen, np.int64).astype(np.int32)
  n = freq.size
  tombstones = min(tombstones, cap - n)
  where = rng.permutation(cap)[:n + tombstones]
  t.keys[dev(where[:n])] = dev(distinct_keys(rng, n))
  t.last_seen[dev(where[:n])] = dev(seen)
  t.freq[dev(where[:n])] = dev(freq)
  if tombstones:
    t.keys[dev(where[n:])] = TOMB
  t.table.copy_(dev(rng.rand(cap, dim).astype(F32)))
  t.recount()
  return t


FILLS = [(5, 0.1), (16, 0.0)]


def companions(rng, cap):
  (v5, w5), (v16, w16) = padded(rng, cap, 5, 8), padded(rng, cap, 16, 20)
  return [(v5, 0.1), (v16, 0.0)], [w5, w16]


def evict_and_check(t, st, max_size, keep_freq=0, slots=(), wholes=(), fills=()):
  """One evict_to(order='lfu') against the restatement: the report and every array.  Returns (report, mask)."""
  report = host(t.evict_to(max_size, keep_freq, slots, order='lfu'))
  want, mask = st.apply(max_size, keep_freq, fills)
  assert report.dtype == np.int32 and report.shape == (8,)
  np.testing.assert_array_equal(report, want)
  st.check(t, wholes)
  return want, mask


# ---- 1. every digit, the sign, the ceiling ------------------------------------------------------------------
@pytest.mark.parametrize('digit', range(6))
def test_the_need_is_decided_inside_each_digit(digit):
  """Classes whose keys differ in ONE digit of k only (11 / 11 / 10 bits over freq, then over last_seen), every
  other bit equal: the five digits around it see one bin, this one decides.  The top digit of a half holds the sign."""
  shift, bits = [21, 10, 0][digit % 3], [11, 11, 10][digit % 3]
  base = 0x2aaaaaaa & ~(((1 << bits) - 1) << shift)                       # the other digits: a fixed pattern
  bins = sorted({0, 1, 2, (1 << bits) // 2 - 1, (1 << bits) // 2, (1 << bits) // 2 + 1, (1 << bits) - 2, (1 << bits) - 1})
  values = np.array([base | (b << shift) for b in bins], np.int64)
  values = np.sort(np.where(values >= 2 ** 31, values - 2 ** 32, values))   # as signed int32, ascending
  assert values.size == 8 and (digit % 3 != 0 or (values < 0).sum() == 4)
  rng = np.random.RandomState(100 + digit)
  per_key = np.concatenate([[v] * (1 + k % 3) for k, v in enumerate(values)])
  other = np.full(per_key.size, 7 if digit < 3 else 3)
  freq, seen = (per_key, other) if digit < 3 else (other, per_key)
  slab_size = [1, 8, 64][digit % 3]
  t = written_table(rng, 128, slab_size, freq, seen)
  slots, wholes = companions(rng, 128)
  st = State(t, wholes)
  for k, v in enumerate(values):
    live = st.live()
    max_size = 0 if k == len(values) - 1 else live - (1 + k % 3)          # down to the next boundary
    want, _ = evict_and_check(t, st, max_size, 0, slots, wholes, FILLS)
    cut = (int(v), 7) if digit < 3 else (3, int(v))
    assert want.tolist() == [live, live - max_size, cut[0], cut[1], 1 + k % 3, 0, 0, 0], (k, v)
  assert t.size() == 0


def test_the_ceiling_negative_counts_and_the_ends_of_the_range():
  """freq = 2^30 (where the count saturates), negative freq (an import may carry any value), and negative,
  INT32_MIN and INT32_MAX last_seen: every (freq, last_seen) pair is a class, and they leave in the order of the
  signed pair, class by class."""
  freqs = [INT32_MIN, -5, 0, 1, 2, 2 ** 30, INT32_MAX]
  seens = [INT32_MIN, -1, 0, 3, INT32_MAX]
  classes = [(f, s) for f in freqs for s in seens]                        # ascending in the LFU order
  rng = np.random.RandomState(106)
  mult = [1 + k % 3 for k in range(len(classes))]
  freq = np.concatenate([[f] * m for (f, _), m in zip(classes, mult)])
  seen = np.concatenate([[s] * m for (_, s), m in zip(classes, mult)])
  t = written_table(rng, 192, 8, freq, seen)
  st = State(t)
  for k, (f, s) in enumerate(classes):
    live = st.live()
    max_size = live - 1 if k % 2 else live - mult[k]                      # one key of the class is enough to take it whole
    want, _ = evict_and_check(t, st, max_size)
    assert want.tolist() == [live, live - max_size, f, s, mult[k], 0, 0, 0], (k, f, s)
  assert t.size() == 0 and t.tombstones() == freq.size + 3


# ---- 2. a freq class that straddles the need -----------------------------------------------------------------
def test_last_seen_decides_inside_a_freq_class_and_a_class_leaves_whole():
  rng = np.random.RandomState(107)
  # 10 keys seen once; 30 seen twice, six at each of the steps 1..5; 20 seen three times
  freq = np.concatenate([np.full(10, 1), np.full(30, 2), np.full(20, 3)])
  seen = np.concatenate([rng.randint(1, 9, size=10), np.repeat(np.arange(1, 6), 6), rng.randint(1, 9, size=20)])
  order = rng.permutation(60)
  t = written_table(rng, 256, 8, freq[order], seen[order])
  slots, wholes = companions(rng, 256)
  st = State(t, wholes)
  need = 10 + 6 + 6 + 2                                                   # two keys into the class (2, 3)
  want, mask = evict_and_check(t, st, 60 - need, 0, slots, wholes, FILLS)
  assert want.tolist() == [60, need, 2, 3, 28, 0, 0, 0]
  class_size, still_needed = 6, 2
  assert t.size() == 60 - need - (class_size - still_needed)              # the undershoot: the class less what was needed
  left = State(t)
  live = (left.keys != EMPTY) & (left.keys != TOMB)
  assert sorted(zip(left.freq[live].tolist(), left.last_seen[live].tolist()))[0] == (2, 4)


# ---- 3. edges ------------------------------------------------------------------------------------------------
def zipf_table(rng, cap, slab_size, load=0.7, steps=6, dim=4):
  """Counts as a click log leaves them (most keys seen once or twice, a few often) over a few steps."""
  n = max(int(cap * load), 1)
  freq = np.minimum(rng.zipf(1.6, size=n), 2 ** 30)
  seen = rng.randint(1, steps + 1, size=n)
  return written_table(rng, cap, slab_size, freq, seen, dim=dim)


EDGE_TABLES = {'one_slab': (64, 64), 'tile_tail': (1096, 8), 'below_a_wave': (40, 8), 'slab_1': (200, 1)}


@pytest.mark.parametrize('shape', sorted(EDGE_TABLES))
def test_edges_of_the_need_the_guard_and_the_geometry(shape):
  cap, slab_size = EDGE_TABLES[shape]
  rng = np.random.RandomState(108 + cap)
  t = zipf_table(rng, cap, slab_size)
  t.last_seen[::7] = -2                                                   # values at or below a cut of 0, too
  slots, wholes = companions(rng, cap)
  saved = State(t, wholes)
  live = saved.live()
  often = int((tref.evictable_mask(saved.keys, saved.freq, 3) == 0).sum() - (cap - live))
  assert live >= 20 and 0 < often < live
  # need <= 0: every array is bit-identical
  for max_size in (live, live + 5, 10 ** 9):
    st = State(t, wholes)
    want, mask = evict_and_check(t, st, max_size, 0, slots, wholes, FILLS)
    assert want.tolist() == [live, live - max_size, 0, 0, 0, 0, 0, 0] and not mask.any()
    saved.check(t, wholes)
  # the keep_freq guard with enough evictable keys: no key seen three times or more leaves
  st = State(t, wholes)
  want, mask = evict_and_check(t, st, live - 5, 3, slots, wholes, FILLS)
  assert want[4] >= 5 and want[2] < 3 and (saved.freq[mask] < 3).all()
  saved.restore(t, wholes)
  # fewer evictable keys than the need: all of them go, both cuts say INT32_MAX, the table stays above the bound
  st = State(t, wholes)
  want, mask = evict_and_check(t, st, often - 1, 3, slots, wholes, FILLS)
  assert want.tolist() == [live, live - often + 1, INT32_MAX, INT32_MAX, live - often, 0, 0, 0]
  assert t.size() == often > often - 1
  saved.restore(t, wholes)
  # max_size = 0: everything leaves
  st = State(t, wholes)
  want, mask = evict_and_check(t, st, 0, 0, slots, wholes, FILLS)
  assert want[4] == live and t.size() == 0
  assert want[2] == saved.freq[mask].max()
  saved.restore(t, wholes)
  # a bound in the middle
  st = State(t, wholes)
  want, mask = evict_and_check(t, st, live // 2, 0, slots, wholes, FILLS)
  assert want[4] >= want[1] == live - live // 2 and t.size() <= live // 2


# ---- 4. N tables in one call ----------------------------------------------------------------------------------
def test_33_tables_in_one_call():
  rng = np.random.RandomState(110)
  tables, states, wholes, slots, max_sizes = [], [], [], [], []
  for c in range(33):
    slab_size = int(rng.choice([1, 8, 64]))
    cap = slab_size * int(rng.randint(max(64 // slab_size, 1), 2048 // slab_size + 1))
    t = zipf_table(rng, cap, slab_size, load=rng.uniform(0.2, 0.8))
    view, whole = padded(rng, cap, 3, 4)
    tables.append(t)
    wholes.append([whole] if c % 2 else [])
    slots.append([(view, 0.25)] if c % 2 else [])
    states.append(State(t, wholes[-1]))
    live = states[-1].live()
    max_sizes.append(0 if c == 31 else live + c % 2 if c % 5 == 0 else int(rng.randint(0, live + 1)))
  max_sizes[32] = states[32].live() // 3                                  # the table behind the launch boundary evicts
  before = [State(t, w) for t, w in zip(tables, wholes)]
  reports = hash_evict_to(tables, max_sizes, slots=slots, order='lfu')
  assert len(reports) == 33
  evicting = idle = 0
  for c, t in enumerate(tables):
    want, _ = states[c].apply(max_sizes[c], 0, [(3, 0.25)] * len(wholes[c]))
    np.testing.assert_array_equal(host(reports[c]), want, err_msg=str(c))
    states[c].check(t, wholes[c])
    if want[1] <= 0:
      before[c].check(t, wholes[c])                                       # inside the bound: untouched
      idle += 1
    else:
      evicting += 1
  assert evicting >= 20 and idle >= 3 and tables[31].size() == 0 and 0 < tables[32].size() <= max_sizes[32]


# ---- 5. the order is not LRU's --------------------------------------------------------------------------------
def test_a_hot_key_that_is_old_survives_lfu_and_leaves_under_lru():
  rng = np.random.RandomState(111)
  t = HashTable(256, 4, DEV, slab_size=8, expiring=True)
  pool = distinct_keys(rng, 121)
  hot, rest = pool[:1], pool[1:]
  t.set_step(1)
  for _ in range(5):
    t.lookup_or_insert(dev(hot))                                          # seen five times at step 1, never again
  for step, part in enumerate(np.array_split(rest, 4), start=2):
    t.set_step(step)
    t.lookup_or_insert(dev(part))                                         # everything else: once, later
  at = int(t.find(dev(hot)).item())
  assert int(t.freq[at].item()) == 5 and int(t.last_seen[at].item()) == 1
  saved = State(t)
  want, _ = evict_and_check(t, State(t), 60)
  assert want[2] == 1 and int(t.find(dev(hot)).item()) == at              # the cut lies among the keys seen once
  assert t.size() <= 60
  saved.restore(t)
  report = host(t.evict_to(60))                                           # order='lru': the same table, the other choice
  assert report.shape == (4,) and report[2] >= 1 and int(t.find(dev(hot)).item()) == -1


# ---- 6. the select and the spill ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def spill_table():
  """1096 slots in slabs of 8 (five 256-slot tiles, the last one ragged), counts as a click log leaves them, a
  dim-5 companion at pitch 8 and a dim-16 one at pitch 20 (the 4-byte and the 16-byte copy path)."""
  rng = np.random.RandomState(112)
  t = zipf_table(rng, 1096, 8, load=0.7)
  slots, wholes = companions(rng, 1096)
  return t, slots, wholes, State(t, wholes)


@pytest.mark.parametrize('keep_freq', [0, 3])
def test_select_writes_nothing_and_counts_what_the_sweep_evicts(spill_table, keep_freq):
  t, slots, wholes, saved = spill_table
  saved.restore(t, wholes)
  live = saved.live()
  for max_size in (live + 1, live, live - 1, live // 2, 17, 0):
    st = State(t, wholes)
    report = hash_evict_to_select([t], [max_size], keep_freq, order='lfu')[0]
    want, mask = lref.select(st.keys, st.last_seen, st.freq, max_size, keep_freq)
    np.testing.assert_array_equal(host(report), want)
    st.check(t, wholes)                                                   # no array of the table changed
    swept, swept_mask = evict_and_check(t, st, max_size, keep_freq, slots, wholes, FILLS)
    np.testing.assert_array_equal(swept, want)                            # n_selected = what the sweep evicts
    assert want[4] == mask.sum() == swept_mask.sum() and (want[4] > 0) == (max_size < live)
    saved.restore(t, wholes)


def check_export(exp, export):
  np.testing.assert_array_equal(host(exp.keys), export['keys'])
  np.testing.assert_array_equal(host(exp.src_slots), export['src_slots'])
  got = [exp.rows, exp.last_seen, exp.freq] + list(exp.slots)
  assert len(got) == len(export['moves'])
  for x, want in zip(got, export['moves']):
    np.testing.assert_array_equal(host(x), want)


@pytest.mark.parametrize('keep_freq', [0, 3])
def test_spill_exports_exactly_what_evict_to_evicts(spill_table, keep_freq):
  t, slots, wholes, saved = spill_table
  live = saved.live()
  for max_size in (live + 1, live - 1, live // 2, 0):
    saved.restore(t, wholes)
    st = State(t, wholes)
    exp = hash_spill([t], [max_size], keep_freq, [slots], order='lfu')[0]
    sel, mask = lref.select(st.keys, st.last_seen, st.freq, max_size, keep_freq)
    export, after, n_evicted, count = st.spill(sel, keep_freq, FILLS)
    assert len(exp) == count == n_evicted == sel[4] == mask.sum()
    check_export(exp, export)                                             # before[mask], ascending slot order
    np.testing.assert_array_equal(export['src_slots'], np.flatnonzero(mask))
    after.check(t, wholes)
    left = State(t, wholes)
    st.restore(t, wholes)                                                 # ... and evict_to leaves the same table
    t.evict_to(max_size, keep_freq, slots, order='lfu')
    left.check(t, wholes)
  saved.restore(t, wholes)


POISON = -1234567


def _spill_raw(t, selection, keep_freq, pairs, out_rows, out_capacity):
  """hbk_hash_spill_lfu_n on one table at the C level, into poisoned outputs of `out_rows` rows.  Returns (outputs,
  count, n_evicted)."""
  out = [torch.full((out_rows,), POISON, dtype=torch.int64, device=DEV),
         torch.full((out_rows,), POISON, dtype=torch.int64, device=DEV),
         torch.full((out_rows, t.dim), float(POISON), device=DEV),
         torch.full((out_rows,), POISON, dtype=torch.int32, device=DEV),
         torch.full((out_rows,), POISON, dtype=torch.int32, device=DEV)]
  out += [torch.full((out_rows, x.shape[1]), float(POISON), device=DEV) for x, _ in pairs]
  col = (_lib.HashSpillColumn * 1)()
  _ht._describe_sweep(col[0], t, keep_freq, pairs)
  col[0].selection = selection.data_ptr()
  moves = [(t.table, out[2]), (t.last_seen, out[3]), (t.freq, out[4])] + [(x, y) for (x, _), y in zip(pairs, out[5:])]
  col[0].n_moves = len(moves)
  for m, (x, y) in enumerate(moves):
    _ht._describe_move(col[0].moves[m], per_slot=x, packed=y, to_packed=True)
  col[0].out_keys, col[0].out_slots, col[0].out_capacity = out[0].data_ptr(), out[1].data_ptr(), out_capacity
  count = torch.full((1,), POISON, dtype=torch.int64, device=DEV)
  n_evicted = torch.full((1,), POISON, dtype=torch.int32, device=DEV)
  col[0].count, col[0].n_evicted = count.data_ptr(), n_evicted.data_ptr()
  lib = _lib.lib()
  nbytes = C.c_size_t()
  _lib.check(lib.hbk_hash_spill_workspace_bytes(1, col, C.byref(nbytes)))
  workspace = torch.empty(max(nbytes.value // 8, 1), dtype=torch.int64, device=DEV)
  _lib.check(lib.hbk_hash_spill_lfu_n(1, col, workspace.data_ptr(), _lib.current_stream(torch.device(DEV))))
  return out, int(count.item()), int(n_evicted.item())


def test_an_output_one_row_short_leaves_the_table_untouched(spill_table):
  t, slots, wholes, saved = spill_table
  saved.restore(t, wholes)
  st = State(t, wholes)
  max_size = st.live() // 2
  selection = hash_evict_to_select([t], [max_size], order='lfu')[0]
  sel = host(selection)
  n = int(sel[4])
  assert n >= 3
  out, count, n_evicted = _spill_raw(t, selection, 0, slots, out_rows=n, out_capacity=n - 1)
  assert (count, n_evicted) == (n, 0)                                     # the total, and nothing was evicted
  st.check(t, wholes)                                                     # every array is as before
  export, _, _, _ = st.spill(sel, 0, FILLS, out_capacity=n - 1)
  for x, w in zip(out, [export['keys'], export['src_slots']] + export['moves']):
    np.testing.assert_array_equal(host(x)[:n - 1], w)                     # what fits is the export's front
    assert (host(x)[n - 1:] == POISON).all()                              # nothing behind out_capacity
  # with room for all of them the same call evicts: the guard and nothing else held it back
  out, count, n_evicted = _spill_raw(t, selection, 0, slots, out_rows=n + 1, out_capacity=n)
  assert (count, n_evicted) == (n, n) and (host(out[0])[n:] == POISON).all()
  _, after, _, _ = st.spill(sel, 0, FILLS)
  after.check(t, wholes)
  saved.restore(t, wholes)


def test_spilled_keys_come_back_as_they_left():
  rng = np.random.RandomState(113)
  t = HashTable(512, 4, DEV, slab_size=8, init_scale=0.05, expiring=True)
  (v5, w5), (v16, w16) = padded(rng, 512, 5, 8), padded(rng, 512, 16, 20)
  held = distinct_keys(rng, 300)
  for step in range(1, 7):                                                # a key of rank r is seen at 1 + r % 6 steps
    t.set_step(step)
    t.lookup_or_insert(dev(held[np.arange(300) % 6 >= step - 1]))
  store = HashSpillStore(4, (5, 16))
  where = host(t.find(dev(held)))
  assert (where >= 0).all()
  st = State(t, [w5, w16])
  exp = t.spill_to(150, store, slots=[(v5, 0.1), (v16, 0.0)], order='lfu')
  sel, mask = lref.select(st.keys, st.last_seen, st.freq, 150)
  gone = host(t.find(dev(held))) < 0
  np.testing.assert_array_equal(np.sort(held[gone]), np.sort(st.keys[mask]))
  assert gone.sum() == len(exp) == len(store) == sel[4] == 150 and sel[2:4].tolist() == [3, 3]   # freq 1..3 left
  np.testing.assert_array_equal(np.sort(held[gone]), host(store.keys()))
  back = held[gone][::2]
  batch = np.concatenate([back, back[:7], held[~gone][:40]])
  t.set_step(9)
  assert t.fault_in(dev(batch), store, slots=[v5, v16]) == back.size
  now = host(t.find(dev(held)))
  came = np.isin(held, back)
  assert ((now >= 0) == (~gone | came)).all() and t.size() + len(store) == 300
  for got, before in ((host(t.table), st.table), (host(t.last_seen), st.last_seen), (host(t.freq), st.freq),
                      (host(w5)[:, :5], st.wholes[0][:, :5]), (host(w16)[:, :16], st.wholes[1][:, :16])):
    np.testing.assert_array_equal(got[now[came]], before[where[came]])    # bit-equal to before the eviction
  np.testing.assert_array_equal(host(w5)[:, 5:], st.wholes[0][:, 5:])     # the padding never moved


# ---- 7. captured graph ----------------------------------------------------------------------------------------
def test_captured_call_replays_on_the_arrays_of_the_moment():
  rng = np.random.RandomState(114)
  t = zipf_table(rng, 1096, 8, load=0.3)
  view, whole = padded(rng, 1096, 5, 8)
  report = torch.zeros(8, dtype=torch.int32, device=DEV)
  t.evict_to(10 ** 6, slots=[(view, 0.1)], report=report, order='lfu')    # outside the capture: the scratch exists
  torch.cuda.synchronize()
  size = t.size()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      t.evict_to(200, slots=[(view, 0.1)], report=report, order='lfu')
  torch.cuda.synchronize()
  assert t.size() == size                                                 # a capture runs nothing
  for n_new, evicts in ((0, True), (150, True), (90, True), (0, False)):
    if n_new:                                                             # other arrays behind the same addresses
      free = np.flatnonzero(host(t.keys) == EMPTY)[:n_new]
      t.keys[dev(free)] = dev(distinct_keys(rng, n_new))
      t.freq[dev(free)] = dev(np.minimum(rng.zipf(1.6, size=n_new), 2 ** 30).astype(np.int32))
      t.last_seen[dev(free)] = dev(rng.randint(1, 9, size=n_new).astype(np.int32))
      t.counts[0] += n_new
      t.freq[::5] += 1
    torch.cuda.synchronize()
    st = State(t, [whole])
    graph.replay()
    torch.cuda.synchronize()
    want, _ = st.apply(200, 0, [(5, 0.1)])
    np.testing.assert_array_equal(host(report), want)
    st.check(t, [whole])
    assert t.size() <= 200 and (want[1] > 0) == evicts and (want[4] > 0) == evicts


# ---- 8. age_freq ----------------------------------------------------------------------------------------------
def test_age_freq_halves_the_counts_and_changes_the_choice():
  rng = np.random.RandomState(115)
  # 40 keys seen 2 or 3 times long ago, 40 keys seen once just now: once the old counts have faded to the new
  # keys' the age decides, and the old keys are the ones to leave
  freq = np.concatenate([rng.randint(2, 4, size=40), np.full(40, 1), [2 ** 30, -7]])
  seen = np.concatenate([np.full(40, 1), np.full(40, 9), [1, 1]])
  t = written_table(rng, 128, 8, freq, seen)
  saved = State(t)
  want, mask = evict_and_check(t, State(t), 50)
  assert (saved.last_seen[mask] == 9).sum() == 40                         # as counted: the new keys leave (and freq -7)
  saved.restore(t)
  t.age_freq()
  st = State(t)
  np.testing.assert_array_equal(st.freq, saved.freq >> 1)                 # halved (an arithmetic shift: -7 -> -4)
  np.testing.assert_array_equal(st.keys, saved.keys)
  np.testing.assert_array_equal(st.last_seen, saved.last_seen)
  assert st.freq.max() == 2 ** 29
  t.age_freq()                                                            # 2 or 3 -> 0, as the keys seen once
  st = State(t)
  np.testing.assert_array_equal(st.freq, saved.freq >> 2)
  want, mask = evict_and_check(t, st, 50)
  assert (saved.last_seen[mask] == 9).sum() == 0 and mask.sum() >= 32     # now the old keys leave, as the restatement says
  t.age_freq(30)
  live = (host(t.keys) != EMPTY) & (host(t.keys) != TOMB)
  assert set(host(t.freq)[live].tolist()) <= {0, -1}


# ---- 9. wrappers ----------------------------------------------------------------------------------------------
def _by_key(t, acc):
  """{key: (row, last_seen, freq, companion row) as bytes} of the live keys."""
  cache = host(t.keys)
  live = np.flatnonzero((cache != EMPTY) & (cache != TOMB))
  arrays = [host(t.table), host(t.last_seen), host(t.freq), host(acc)]
  return {int(cache[s]): tuple(a[s].tobytes() for a in arrays) for s in live}


def test_tracked_lfu_evictions_travel_in_a_delta():
  rng = np.random.RandomState(116)
  dim, seed, scale, acc0 = 4, 3, 0.05, 0.1
  t = HashTable(512, dim, DEV, slab_size=8, init_scale=scale, seed=seed, expiring=True)
  acc = torch.full((512, dim), acc0, device=DEV)
  store = HashSpillStore(dim, [dim])
  pool = distinct_keys(rng, 200)
  t.track_removals()

  def touch(step, keys):
    t.set_step(step)
    slots = torch.unique(t.lookup_or_insert(dev(keys)))
    assert int(slots.min().item()) >= 0
    t.table[slots] += 0.01 * step
    acc[slots] += 0.5
  touch(1, pool[:120])
  touch(2, pool[:60])                                                     # the first 60: seen twice
  base = t.export_items(slots=[acc])
  assert len(base) == 120 and base.removed.numel() == 0
  t.clear_removals()
  touch(3, np.concatenate([pool[120:], pool[:20]]))                       # 80 new keys; 20 seen a third time
  st = State(t)
  report = host(t.evict_to(150, slots=[(acc, acc0)], order='lfu'))       # a tracked sweep: the keys seen once at step 1
  _, mask = lref.select(st.keys, st.last_seen, st.freq, 150)
  assert report.tolist() == [200, 50, 1, 1, 60, 0, 0, 0]
  np.testing.assert_array_equal(np.sort(st.keys[mask]), np.sort(pool[60:120]))
  np.testing.assert_array_equal(host(t.removed_keys()), np.sort(pool[60:120]))
  st = State(t)
  spilled = t.spill_to(100, store, slots=[(acc, acc0)], order='lfu')      # a tracked spill: the keys seen once at step 3
  _, mask = lref.select(st.keys, st.last_seen, st.freq, 100)
  np.testing.assert_array_equal(np.sort(host(spilled.keys)), np.sort(st.keys[mask]))
  np.testing.assert_array_equal(np.sort(host(spilled.keys)), np.sort(pool[120:]))
  delta = t.export_items(since=3, slots=[acc])
  np.testing.assert_array_equal(host(delta.removed), np.sort(pool[60:]))
  live = _by_key(t, acc)
  assert sorted(live) == sorted(pool[:60].tolist())
  t2 = HashTable(1024, dim, DEV, slab_size=16, init_scale=scale, seed=seed, expiring=True)
  acc2 = torch.full((1024, dim), acc0, device=DEV)
  t2.import_items(base, [acc2])
  t2.import_items(delta, [(acc2, acc0)])
  assert _by_key(t2, acc2) == live                                        # base + delta: the table that was saved


def key_rows(keys, dim):
  return ((keys % 1000).astype(F32)[:, None] + np.arange(dim, dtype=F32)[None, :] / 16).astype(F32)


def test_group_lookup_maybe_evict_in_lfu_order_evicts_spills_and_rebinds():
  rng = np.random.RandomState(117)
  tables = [HashTable(256, d, DEV, slab_size=8, init_scale=0.05, seed=3 + c, expiring=True)
            for c, d in enumerate((4, 6))]
  look = HashGroupLookup(tables)
  pools = [distinct_keys(rng, 210), distinct_keys(rng, 60)]               # table 0 passes 0.75, table 1 does not
  for step in range(1, 5):
    for t in tables:
      t.set_step(step)
    # table 0: the first 70 keys at every step, 35 new ones per step besides
    look([dev(np.concatenate([pools[0][:70], pools[0][70 + 35 * (step - 1):70 + 35 * step]])),
          dev(pools[1][:15 * step])], [None, None])
  accums = [torch.full_like(t.table, 0.1) for t in tables]
  slots0 = host(tables[0].find(dev(pools[0])))
  assert (slots0 >= 0).all() and tables[0].size() == 210
  accums[0][dev(slots0)] = dev(key_rows(pools[0], 4))
  st = State(tables[0])
  rows1 = tables[1].table
  with pytest.raises(_lib.InvalidArgumentError, match="order must be 'lru' or 'lfu'"):
    look.maybe_evict(0.75, 0.5, slots=[[(a, 0.1)] for a in accums], order='fifo')
  res = look.maybe_evict(0.75, 0.5, slots=[[(a, 0.1)] for a in accums], order='lfu')
  assert res[0] is not None and res[1] is None and tables[1].table is rows1
  sel, mask = lref.select(st.keys, st.last_seen, st.freq, 128)
  assert sel.tolist() == [210, 82, 1, 3, 105, 0, 0, 0]                    # the keys seen once at the steps 1 to 3
  left = st.keys[mask]
  now = host(tables[0].find(dev(pools[0])))
  assert ((now < 0) == np.isin(pools[0], left)).all() and (now[:70] >= 0).all()
  assert tables[0].size() == 105 and tables[0].tombstones() == 0 and tables[0].capacity == 256
  kept = now >= 0
  np.testing.assert_array_equal(host(res[0][0])[now[kept]], key_rows(pools[0][kept], 4))
  np.testing.assert_array_equal(host(tables[0].table)[now[kept]], st.table[slots0[kept]])
  np.testing.assert_array_equal(host(tables[0].freq)[now[kept]], st.freq[slots0[kept]])
  with pytest.raises(_lib.HbkError, match='launch'):                      # rebound: as a fresh object
    look.launch()
  # with a store: what leaves in LFU order is in the store
  store = HashSpillStore(4, (4,))
  tables[0].set_step(5)
  look([dev(distinct_keys(rng, 95)), dev(pools[1][:5])], [None, None])
  st = State(tables[0])
  res = look.maybe_evict(0.75, 0.5, slots=[[(res[0][0], 0.1)], [(accums[1], 0.1)]], spill=[store, None], order='lfu')
  _, mask = lref.select(st.keys, st.last_seen, st.freq, 128)
  assert res[0] is not None and mask.sum() > 0
  np.testing.assert_array_equal(host(store.keys()), np.sort(st.keys[mask]))
  assert tables[0].size() == 200 - mask.sum() <= 128


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


def test_sharded_maybe_evict_in_lfu_order():
  dim, seed, scale, acc0 = 8, 5, 0.05, 0.1
  often = np.arange(40, dtype=np.int64) + 7000                            # asked for at every step
  once = [np.arange(14, dtype=np.int64) + 1000 * s for s in range(1, 6)]  # 14 new ids per step

  def rank(r, comm):
    tables = [HashTable(128, dim, DEV, slab_size=8, init_scale=scale, seed=seed, expiring=True)]
    accums = [torch.full_like(tables[0].table, acc0)]
    drv = ShardedHashGroupLookup(tables, comm, combiners=['sum'], accums=accums, initial_accumulator_value=acc0)
    for step, g in enumerate(once, start=1):
      tables[0].set_step(step)
      ids = dev(np.concatenate([often, g]))
      drv([ids], [None])
      drv.backward([torch.ones((ids.numel(), dim), device=DEV)], apply_lr=0.5, optimizer='adagrad', emit=False)
    torch.cuda.current_stream().synchronize()
    before = [host(x).copy() for x in (tables[0].keys, tables[0].last_seen, tables[0].freq)]
    size = tables[0].size()
    rows = tables[0].table
    tables[0].set_step(6)
    evicted = drv.maybe_evict(0.75, 0.5, order='lfu')
    ask = np.concatenate([often, once[0], once[4]])
    out = host(drv([dev(ask)], [None])[0])
    where = host(tables[0].find(dev(once[0])))
    res = dict(size=size, after=tables[0].size(), moved=tables[0].table is not rows, evicted=evicted, before=before,
               out=out, accum=host(drv.accums[0])[where], tombstones=tables[0].tombstones())
    drv.close()
    return res

  res = run_world(1, rank)[0]
  keys, seen, freq = res['before']
  sel, mask = lref.select(keys, seen, freq, 64)
  assert res['size'] == 110 and sel.tolist() == [110, 46, 1, 4, 56, 0, 0, 0]   # the ids seen once at the steps 1..4
  assert res['evicted'] == [True] and res['moved'] and res['tombstones'] == 0
  # the lookup behind the eviction inserted step 1's ids again: 110 - 56 + 14
  assert res['after'] == 68
  ask = np.concatenate([often, once[0], once[4]])
  fresh = ref.init_rows(ask, dim, seed, scale)
  back = np.isin(ask, once[0])
  np.testing.assert_array_equal(res['out'][back], fresh[back])            # evicted and back afresh ...
  assert (res['out'][~back] != fresh[~back]).any(axis=1).all()            # ... every other id kept its trained row
  assert (res['accum'] == F32(acc0)).all()                                # and a fresh accumulator


# ---- 10. training under a bound --------------------------------------------------------------------------------
def test_tiered_lfu_training_equals_unbounded_training():
  rng = np.random.RandomState(118)
  dims, lr, acc0, n_steps = [4, 16], 0.1, 0.1, 8
  # per column and step 64 ids: new ids alone for four steps (256 keys: the bound), then 24 new ones, 32 of those
  # used four and more steps back and 8 of the 56 twice
  batches, used = [], [[], []]
  for s in range(n_steps):
    ids = []
    for c in range(2):
      batch = distinct_keys(rng, 64)
      if s >= 4:
        old = np.concatenate(used[c][:s - 3])
        batch = np.concatenate([batch[:24], old[rng.permutation(old.size)[:32]]])
        batch = np.concatenate([batch, batch[rng.permutation(56)[:8]]])
      used[c].append(np.unique(batch))
      ids.append(batch[rng.permutation(64)])
    batches.append((ids, [rng.randn(64, d).astype(F32) for d in dims]))

  def run(bound):
    tables = [HashTable(2048, dims[c], DEV, slab_size=8, init_scale=0.05, seed=3 + c, expiring=True) for c in range(2)]
    accums = [torch.full_like(t.table, acc0) for t in tables]
    stores = [HashSpillStore(d, (d,)) for d in dims]
    hgl = HashGroupLookup(tables, combiners='sum')
    grad = GroupLookupGrad(hgl.lookup, accums=accums, deterministic=True)
    restored = 0
    for s, (ids, grads) in enumerate(batches, start=1):
      for t in tables:
        t.set_step(s)
      d_ids = [dev(i) for i in ids]
      if bound:
        restored += sum(hgl.fault_in(d_ids, stores, [[a] for a in accums]))
      hgl(d_ids)
      assert all(bool((x >= 0).all().item()) for x in hgl.slots)
      grad(hgl.slots, [dev(g) for g in grads], apply_lr=lr, optimizer='adagrad')
      if bound:
        for t, a, st in zip(tables, accums, stores):
          t.spill_to(bound, st, slots=[(a, acc0)], order='lfu')
          assert t.size() <= bound
    return tables, accums, stores, restored

  tiered, accums, stores, restored = run(256)
  whole, whole_accums, _, _ = run(0)
  assert restored >= 20                                                   # keys did leave and come back
  for c in range(2):
    seen = np.unique(np.concatenate([ids[c] for ids, _ in batches]))
    at, ref_at = host(tiered[c].find(dev(seen))), host(whole[c].find(dev(seen)))
    spilled = stores[c].peek(torch.from_numpy(seen))
    in_store = np.isin(seen, spilled.keys.numpy())
    assert ((at >= 0) ^ in_store).all() and in_store.any() and (ref_at >= 0).all()
    assert tiered[c].failed() == 0 and whole[c].failed() == 0
    for on_device, in_host, ref_array in ((tiered[c].table, spilled.rows, whole[c].table),
                                          (accums[c], spilled.slots[0], whole_accums[c]),
                                          (tiered[c].freq[:, None], spilled.freq[:, None], whole[c].freq[:, None])):
      got = np.empty((seen.size, ref_array.shape[1]), host(ref_array).dtype)
      got[at >= 0] = host(on_device)[at[at >= 0]]
      got[in_store] = in_host.numpy()
      np.testing.assert_array_equal(got, host(ref_array)[ref_at])         # rows, accumulators and counts, bit for bit
