"""Spilling to a host tier on the GPU (hbk_hash_evict_to_select_n, hbk_hash_spill_n, HashTable.spill_to / fault_in,
HashSpillStore, maybe_evict(spill=...)) against the numpy restatement of tests/support/hash_spill_ref.py.
Everything is compared bit for bit: the selection and the export are functions of the table's arrays alone, and
a key that left and came back carries the bits it left with."""
import ctypes as C

import numpy as np
import pytest
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (GroupLookupGrad, HashGroupLookup, HashSpillStore, HashTable,
                                         hash_evict_to_select, hash_spill)
from hybridbackend_amd.embedding import hashtable as _ht
from tests.support import hash_evict_to_ref as tref
from tests.support import hash_spill_ref as sref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
EMPTY, TOMB = tref.EMPTY, tref.TOMBSTONE
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
CASES = ['above', 'exact', 'one', 'mid_group', 'boundary', 'zero']


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


NAMES = ('keys', 'last_seen', 'freq', 'stats', 'counts', 'table')


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

  def check(self, t, wholes=()):
    for name in NAMES:
      np.testing.assert_array_equal(host(getattr(t, name)), getattr(self, name), err_msg=name)
    for w, want in zip(wholes, self.wholes):
      np.testing.assert_array_equal(host(w), want)

  def same(self, other):
    for name in NAMES:
      np.testing.assert_array_equal(getattr(self, name), getattr(other, name), err_msg=name)
    for a, b in zip(self.wholes, other.wholes):
      np.testing.assert_array_equal(a, b)

  def spill(self, selection, keep_freq, dims_values, out_capacity=None):
    """The restatement's spill of this state: (export, the State afterwards, n_evicted, count)."""
    moves = [(self.table, self.table.shape[1]), (self.last_seen, 1), (self.freq, 1)]
    moves += [(w, d) for w, (d, _) in zip(self.wholes, dims_values)]
    comps = [(w, d, F32(v)) for w, (d, v) in zip(self.wholes, dims_values)]
    export, after, n_evicted, count = sref.spill(self.keys, self.last_seen, self.freq, selection, keep_freq, moves,
                                                 comps, out_capacity)
    st = State.__new__(State)
    st.keys, st.last_seen, st.freq = after['cache'], after['last_seen'], after['freq']
    st.stats, st.counts, st.table, st.wholes = self.stats.copy(), self.counts, self.table, after['companions']
    st.stats[0] += n_evicted
    return export, st, n_evicted, count


def check_export(exp, export):
  """A HashExport against the restatement's export: keys, source slots, rows, last_seen, freq, companions."""
  np.testing.assert_array_equal(host(exp.keys), export['keys'])
  np.testing.assert_array_equal(host(exp.src_slots), export['src_slots'])
  got = [exp.rows, exp.last_seen, exp.freq] + list(exp.slots)
  assert len(got) == len(export['moves'])
  for x, want in zip(got, export['moves']):
    np.testing.assert_array_equal(host(x), want)
  assert exp.since == 0


def fill_over_steps(t, rng, groups, first_step=1):
  """Insert `groups` (arrays of keys) at consecutive steps, each step also touching a few keys of the step before."""
  prev = np.zeros(0, np.int64)
  for n, g in enumerate(groups):
    t.set_step(first_step + n)
    t.lookup_or_insert(dev(np.concatenate([g, prev[:max(prev.size // 4, 0)]])))
    prev = g


@pytest.fixture(scope='module')
def filled_pair():
  """A table of 64 slabs x 8 (two 256-slot tiles) and one of 37 x 3 (111 slots: a ragged last wave), filled over
  steps 1..6, with a dim-5 companion at pitch 8 and a dim-16 one at pitch 20 (the 4-byte and the 16-byte copy path,
  padding that must stay); their saved states."""
  rng = np.random.RandomState(31)
  out = []
  for slab_count, slab_size, per_step in ((64, 8, 55), (37, 3, 12)):
    cap = slab_count * slab_size
    t = HashTable(cap, 4, DEV, slab_size=slab_size, init_scale=0.05, expiring=True)
    pool = distinct_keys(rng, 6 * per_step)
    fill_over_steps(t, rng, [pool[s * per_step:(s + 1) * per_step] for s in range(6)])
    (v5, w5), (v16, w16) = padded(rng, cap, 5, 8), padded(rng, cap, 16, 20)
    out.append((t, [(v5, 0.1), (v16, 0.0)], [w5, w16], State(t, [w5, w16])))
  return out


FILLS = [(5, 0.1), (16, 0.0)]


def _prepare(filled, case, keep_freq):
  """The saved state restored, every third live slot seen often when keep_freq is set; (st, max_size)."""
  t, _, wholes, saved = filled
  saved.restore(t, wholes)
  if keep_freq:
    often = np.flatnonzero((saved.keys != EMPTY) & (saved.keys != TOMB))[::3]
    t.freq[dev(often)] = keep_freq + 2
  st = State(t, wholes)
  live = st.live()
  evictable = tref.evictable_mask(st.keys, st.freq, keep_freq)
  steps, sizes = np.unique(st.last_seen[evictable], return_counts=True)
  assert steps.size >= 3 and sizes[1] >= 2 and live > 0.5 * t.capacity   # the cases are what their names say
  max_size = {'above': live + 3, 'exact': live, 'one': live - 1, 'mid_group': live - int(sizes[0] + sizes[1] // 2),
              'boundary': live - int(sizes[0] + sizes[1]), 'zero': 0}[case]
  return st, max_size


# ---- 1. the select ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('keep_freq', [0, 3])
def test_select_reports_what_the_sweep_would_evict_and_writes_nothing(filled_pair, which, keep_freq):
  t, slots, wholes, saved = filled_pair[which]
  for case in CASES:
    st, max_size = _prepare(filled_pair[which], case, keep_freq)
    report = hash_evict_to_select([t], [max_size], keep_freq)[0]
    want = sref.select(st.keys, st.last_seen, st.freq, max_size, keep_freq)
    np.testing.assert_array_equal(host(report), want, err_msg=case)
    st.check(t, wholes)                                                   # no array of the table changed
    assert (want[3] == 0) == (case in ('above', 'exact')) and (case != 'boundary' or want[3] == want[1])
    if case == 'zero' and keep_freq:
      assert want[2] == INT32_MAX and 0 < want[3] < want[1]              # the protected keys alone exceed the bound
    # and the evicting entry agrees: its own fourth word is the sweep's count
    swept = host(t.evict_to(max_size, keep_freq, slots))
    np.testing.assert_array_equal(swept, want, err_msg=case)
  saved.restore(t, wholes)


def test_select_every_digit_the_sign_and_a_need_that_is_not_positive():
  values = sorted([2 ** k for k in range(0, 31, 3)] + [0, -1, -2 ** 20, INT32_MIN, INT32_MAX])
  rng = np.random.RandomState(32)
  t = HashTable(128, 4, DEV, slab_size=8, expiring=True)
  per_key = np.concatenate([[v] * (1 + k % 3) for k, v in enumerate(values)]).astype(np.int32)
  keys = distinct_keys(rng, per_key.size)
  slots = host(t.lookup_or_insert(dev(keys)))
  assert (slots >= 0).all()
  t.last_seen[dev(slots[rng.permutation(per_key.size)])] = dev(per_key)   # the values, spread over the slots
  st = State(t)
  live, below = st.live(), 0
  sizes = [live - n for n in np.cumsum([1 + k % 3 for k in range(len(values))])]
  reports = hash_evict_to_select([t] * len(sizes), sizes)                 # one call, the same table at every bound
  for k, v in enumerate(values):
    below += 1 + k % 3
    want = sref.select(st.keys, st.last_seen, st.freq, sizes[k])
    assert want.tolist() == [live, below, v, below]
    np.testing.assert_array_equal(host(reports[k]), want)
  st.check(t)
  # need <= 0 with last_seen values <= 0 = the reported cut: nothing is selected, nothing leaves
  for max_size in (live, live + 5):
    exp = t.spill_to(max_size)
    assert len(exp) == 0 and (st.last_seen[st.keys != EMPTY] <= 0).sum() >= 4
    st.check(t)
  sel = dev(np.array([live, 0, 0, 0], np.int32))
  count, n_evicted = _spill_raw(t, sel, 0, [], out_rows=4)[2:]
  assert (count, n_evicted) == (0, 0)
  st.check(t)


# ---- 2. the spill ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('keep_freq', [0, 3])
def test_spill_exports_what_it_evicts_and_evicts_as_evict_to(filled_pair, which, keep_freq):
  t, slots, wholes, saved = filled_pair[which]
  for case in CASES:
    st, max_size = _prepare(filled_pair[which], case, keep_freq)
    exp = t.spill_to(max_size, keep_freq=keep_freq, slots=slots)
    sel = sref.select(st.keys, st.last_seen, st.freq, max_size, keep_freq)
    export, after, n_evicted, count = st.spill(sel, keep_freq, FILLS)
    assert len(exp) == count == n_evicted == sel[3], case
    check_export(exp, export)                                             # before[mask], ascending slot order
    assert exp.keys.device.type == 'cuda' and (np.diff(export['src_slots']) > 0).all()
    after.check(t, wholes)
    left = State(t, wholes)
    # what evict_to leaves on a restored copy of the same state: every array, the padding included
    st.restore(t, wholes)
    t.evict_to(max_size, keep_freq, slots)
    left.check(t, wholes)
    assert t.size() == st.live() - count
  saved.restore(t, wholes)


# ---- 3. the guard ----------------------------------------------------------------------------------------
POISON = -1234567


def _spill_raw(t, selection, keep_freq, pairs, out_rows, out_capacity=None):
  """hbk_hash_spill_n on one table at the C level, into poisoned outputs of `out_rows` rows.  Returns (outputs,
  companions' outputs, count, n_evicted)."""
  out = {'keys': torch.full((out_rows,), POISON, dtype=torch.int64, device=DEV),
         'src_slots': torch.full((out_rows,), POISON, dtype=torch.int64, device=DEV),
         'rows': torch.full((out_rows, t.dim), float(POISON), device=DEV),
         'last_seen': torch.full((out_rows,), POISON, dtype=torch.int32, device=DEV),
         'freq': torch.full((out_rows,), POISON, dtype=torch.int32, device=DEV)}
  comps = [torch.full((out_rows, x.shape[1]), float(POISON), device=DEV) for x, _ in pairs]
  col = (_lib.HashSpillColumn * 1)()
  _ht._describe_sweep(col[0], t, keep_freq, pairs)
  col[0].selection = selection.data_ptr()
  moves = [(t.table, out['rows']), (t.last_seen, out['last_seen']), (t.freq, out['freq'])]
  moves += [(x, y) for (x, _), y in zip(pairs, comps)]
  col[0].n_moves = len(moves)
  for m, (x, y) in enumerate(moves):
    _ht._describe_move(col[0].moves[m], per_slot=x, packed=y, to_packed=True)
  col[0].out_keys, col[0].out_slots = out['keys'].data_ptr(), out['src_slots'].data_ptr()
  col[0].out_capacity = out_rows if out_capacity is None else out_capacity
  count = torch.full((1,), POISON, dtype=torch.int64, device=DEV)
  n_evicted = torch.full((1,), POISON, dtype=torch.int32, device=DEV)
  col[0].count, col[0].n_evicted = count.data_ptr(), n_evicted.data_ptr()
  lib = _lib.lib()
  nbytes = C.c_size_t()
  _lib.check(lib.hbk_hash_spill_workspace_bytes(1, col, C.byref(nbytes)))
  workspace = torch.empty(max(nbytes.value // 8, 1), dtype=torch.int64, device=DEV)
  _lib.check(lib.hbk_hash_spill_n(1, col, workspace.data_ptr(), _lib.current_stream(torch.device(DEV))))
  return out, comps, int(count.item()), int(n_evicted.item())


@pytest.mark.parametrize('which', [0, 1])
def test_guard_one_row_short_nothing_leaves_and_nothing_lies_behind_the_output(filled_pair, which):
  t, slots, wholes, saved = filled_pair[which]
  st, max_size = _prepare(filled_pair[which], 'mid_group', 0)
  selection = hash_evict_to_select([t], [max_size])[0]
  sel = host(selection)
  n = int(sel[3])
  assert n >= 3
  out, comps, count, n_evicted = _spill_raw(t, selection, 0, slots, out_rows=n, out_capacity=n - 1)
  assert (count, n_evicted) == (n, 0)                                     # the total, and nothing was evicted
  st.check(t, wholes)                                                     # every array is as before
  export, _, _, _ = st.spill(sel, 0, FILLS, out_capacity=n - 1)
  got = [out['keys'], out['src_slots'], out['rows'], out['last_seen'], out['freq']] + comps
  want = [export['keys'], export['src_slots']] + export['moves']
  for x, w in zip(got, want):
    np.testing.assert_array_equal(host(x)[:n - 1], w)                     # what fits is the export's front
    assert (host(x)[n - 1:] == POISON).all()                              # nothing behind out_capacity
  # with room for all of them the same call evicts: the guard and nothing else held it back
  out, comps, count, n_evicted = _spill_raw(t, selection, 0, slots, out_rows=n + 1, out_capacity=n)
  assert (count, n_evicted) == (n, n) and (host(out['keys'])[n:] == POISON).all()
  _, after, _, _ = st.spill(sel, 0, FILLS)
  after.check(t, wholes)
  saved.restore(t, wholes)


# ---- 4. many tables in one call ----------------------------------------------------------------------------
def test_33_tables_in_one_call_and_a_scan_of_two_passes():
  rng = np.random.RandomState(33)
  tables, states, wholes, slots, max_sizes = [], [], [], [], []
  for c in range(32):
    slab_size = int(rng.choice([1, 3, 8, 16, 64]))
    cap = slab_size * int(rng.randint(2, 40))
    t = HashTable(cap, 4, DEV, slab_size=slab_size, init_scale=0.05, expiring=True)
    pool = distinct_keys(rng, max(int(cap * rng.uniform(0.2, 0.7)), 4))
    fill_over_steps(t, rng, np.array_split(pool, 4), first_step=1 + c)
    view, whole = padded(rng, cap, 3, 4)
    tables.append(t)
    wholes.append([whole] if c % 2 else [])
    slots.append([(view, 0.25)] if c % 2 else [])
    states.append(State(t, wholes[-1]))
    live = states[-1].live()
    max_sizes.append(0 if c == 30 else live + c % 2 if c % 5 == 0 else int(rng.randint(0, live + 1)))
  # a dim-1 table of 2049 tiles: the scan's second pass (2048 tiles per pass) carries the first one's total.  The
  # arrays are written directly -- neither call looks at where a key hashes to
  cap = 524544
  big = HashTable(cap, 1, DEV, slab_size=64, expiring=True)
  ends = np.array([0, 255, 256, 524287, 524288, 524300, cap - 1])        # both ends of both passes: among the oldest
  where = np.unique(np.concatenate([rng.randint(0, cap, size=3000), ends]))
  big.keys[dev(where)] = dev(distinct_keys(rng, where.size))
  big.last_seen[dev(where)] = dev(rng.randint(1, 9, size=where.size).astype(np.int32))
  big.last_seen[dev(ends)] = 1
  big.freq[dev(where)] = 1
  big.table.copy_(dev(rng.rand(cap, 1).astype(F32)))
  big.recount()
  tables.append(big)
  wholes.append([])
  slots.append([])
  states.append(State(big))
  max_sizes.append(where.size // 2)
  exports = hash_spill(tables, max_sizes, slots=slots)
  assert len(exports) == 33
  evicting = idle = 0
  for c, t in enumerate(tables):
    st = states[c]
    sel = sref.select(st.keys, st.last_seen, st.freq, max_sizes[c])
    export, after, n_evicted, count = st.spill(sel, 0, [(3, 0.25)] * len(wholes[c]))
    assert len(exports[c]) == count == n_evicted, c
    check_export(exports[c], export)
    after.check(t, wholes[c])
    if sel[1] <= 0:
      st.check(t, wholes[c])                                              # inside the bound: untouched
      idle += 1
    else:
      evicting += 1
  assert evicting >= 20 and idle >= 3 and tables[30].size() == 0
  last = host(exports[32].src_slots)
  assert np.isin(ends, last).all() and big.size() <= max_sizes[32]


# ---- 5. round trip -----------------------------------------------------------------------------------------
def key_rows(keys, dim, step=0):
  """A row per (key, step) that names both."""
  return ((keys % 1000).astype(F32)[:, None] + np.arange(dim, dtype=F32)[None, :] / 16 + F32(step) * 1000).astype(F32)


def test_spilled_keys_come_back_as_they_left():
  rng = np.random.RandomState(34)
  t = HashTable(512, 4, DEV, slab_size=8, init_scale=0.05, expiring=True)
  (v5, w5), (v16, w16) = padded(rng, 512, 5, 8), padded(rng, 512, 16, 20)
  pool = distinct_keys(rng, 340)
  held, never = pool[:300], pool[300:]
  fill_over_steps(t, rng, np.array_split(held, 6))
  store = HashSpillStore(4, (5, 16))
  where = host(t.find(dev(held)))
  assert (where >= 0).all()
  st = State(t, [w5, w16])
  exp = t.spill_to(150, store, slots=[(v5, 0.1), (v16, 0.0)])
  gone = host(t.find(dev(held))) < 0
  assert gone.sum() == len(exp) == len(store) >= 150 >= 50 and t.size() + len(store) == 300   # >= a step's keys left
  np.testing.assert_array_equal(np.sort(held[gone]), host(store.keys()))
  # a batch of spilled keys (some twice), resident keys and keys never seen
  back = held[gone][::2]
  assert back.size >= 2
  batch = np.concatenate([back, back[:7], held[~gone][:40], never])
  rng.shuffle(batch)
  t.set_step(9)
  restored = t.fault_in(dev(batch), store, slots=[v5, v16])
  assert restored == back.size
  now = host(t.find(dev(held)))
  assert ((now >= 0) == (~gone | np.isin(held, back))).all()
  assert (host(t.find(dev(never))) == -1).all() and len(store.peek(torch.from_numpy(never))) == 0   # in neither tier
  assert not np.isin(back, host(store.keys())).any()                      # the store no longer holds them
  assert t.size() + len(store) == 300 and len(store) == gone.sum() - back.size and t.failed() == 0
  sel = np.isin(held, back)
  for got, before in ((host(t.table), st.table), (host(t.last_seen), st.last_seen), (host(t.freq), st.freq),
                      (host(w5)[:, :5], st.wholes[0][:, :5]), (host(w16)[:, :16], st.wholes[1][:, :16])):
    np.testing.assert_array_equal(got[now[sel]], before[where[sel]])      # bit-equal to before the eviction
  np.testing.assert_array_equal(host(w5)[:, 5:], st.wholes[0][:, 5:])     # the padding never moved
  assert t.fault_in(dev(batch), store, slots=[v5, v16]) == 0              # nothing more to bring
  # too full for what is taken: the keys that do not fit go back into the store, none is lost
  small = HashTable(8, 4, DEV, slab_size=8, expiring=True)
  (s5, _), (s16, _) = padded(rng, 8, 5, 8), padded(rng, 8, 16, 20)
  rest = host(store.keys())
  with pytest.raises(_lib.InvalidArgumentError, match='do not fit'):
    small.fault_in(dev(rest), store, slots=[s5, s16])
  inside = host(small.find(dev(rest))) >= 0
  assert inside.sum() == small.size() == 8 and len(store) == rest.size - 8
  np.testing.assert_array_equal(host(store.keys()), rest[~inside])


# ---- 6. tiered against unbounded, table level --------------------------------------------------------------
def test_tiered_table_equals_the_unbounded_one():
  rng = np.random.RandomState(35)
  pool = distinct_keys(rng, 400)
  steps = [np.unique(pool[rng.randint(0, 400, size=64)]) for _ in range(12)]
  # on the CPU: with these parameters the tiered table stays below load 0.75 at every step, even if no tombstone
  # is ever reused between two rehashes
  model, ever, dead, comebacks = {}, set(), 0, 0
  for s, ids in enumerate(steps, start=1):
    comebacks += sum(1 for k in ids.tolist() if k not in model and k in ever)
    ever.update(ids.tolist())
    for k in ids.tolist():
      model[k] = s
    assert len(model) + dead <= 0.75 * 512
    keys = np.array(list(model), np.int64)
    seen = np.array([model[k] for k in keys.tolist()], np.int32)
    sel = sref.select(keys, seen, np.ones(keys.size, np.int32), 128)
    for k in keys[sref.selected_mask(keys, seen, np.ones(keys.size, np.int32), sel)].tolist():
      del model[k]
    dead = 0 if s % 4 == 0 else dead + int(sel[3])
    assert len(model) <= 128
  assert comebacks >= 20                                                  # ids do recur after they left

  def run(capacity, bound):
    t = HashTable(capacity, 4, DEV, slab_size=8, init_scale=0.05, seed=7, expiring=True)
    acc = torch.full((capacity, 4), 0.1, device=DEV)
    store = HashSpillStore(4, (4,))
    for s, ids in enumerate(steps, start=1):
      t.set_step(s)
      d_ids = dev(ids)
      if bound:
        t.fault_in(d_ids, store, slots=[acc])
      slots = t.lookup_or_insert(d_ids)
      assert bool((slots >= 0).all().item())
      t.table[slots] = t.table[slots] * 0.5 + dev(key_rows(ids, 4, s))
      acc[slots] = acc[slots] + dev(key_rows(ids, 4, s) * F32(0.25))
      if bound:
        t.spill_to(bound, store, slots=[(acc, 0.1)])
        assert t.size() <= bound
        if s % 4 == 0:
          acc = t.rehash(slots=[(acc, 0.1)])[0]
    return t, acc, store

  tiered, acc, store = run(512, 128)
  whole, whole_acc, _ = run(2048, 0)
  assert tiered.failed() == 0 and whole.failed() == 0 and len(store) > 0
  seen = np.unique(np.concatenate(steps))
  at = host(tiered.find(dev(seen)))
  spilled = store.peek(torch.from_numpy(seen))
  in_store = np.isin(seen, spilled.keys.numpy())
  assert ((at >= 0) ^ in_store).all() and tiered.size() + len(store) == seen.size == whole.size()
  ref_at = host(whole.find(dev(seen)))
  want = [host(whole.table)[ref_at], host(whole_acc)[ref_at], host(whole.freq)[ref_at], host(whole.last_seen)[ref_at]]
  got = [np.empty_like(w) for w in want]
  for g, on_device, in_host in zip(got, (tiered.table, acc, tiered.freq, tiered.last_seen),
                                   (spilled.rows, spilled.slots[0], spilled.freq, spilled.last_seen)):
    g[at >= 0] = host(on_device)[at[at >= 0]]
    g[in_store] = in_host.numpy()                                         # (both in ascending key order)
  for g, w in zip(got, want):
    np.testing.assert_array_equal(g, w)


# ---- 7. tiered against unbounded, through the optimizer ----------------------------------------------------
def test_tiered_training_equals_unbounded_training():
  rng = np.random.RandomState(36)
  dims, lr, acc0, n_steps = [4, 16], 0.1, 0.1, 8
  # per column and step 64 ids: new ids alone for four steps (256 keys: the bound), then 24 new ones, 32 of those
  # used four and more steps back -- the oldest, which the bound pushes into the store -- and 8 of the 56 twice
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
          t.spill_to(bound, st, slots=[(a, acc0)])
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
                                          (accums[c], spilled.slots[0], whole_accums[c])):
      got = np.empty((seen.size, dims[c]), F32)
      got[at >= 0] = host(on_device)[at[at >= 0]]
      got[in_store] = in_host.numpy()
      np.testing.assert_array_equal(got, host(ref_array)[ref_at])         # rows and accumulators, bit for bit


# ---- 8. policy ---------------------------------------------------------------------------------------------
def test_maybe_evict_spills_what_leaves():
  rng = np.random.RandomState(37)
  t = HashTable(256, 4, DEV, slab_size=8, init_scale=0.05, expiring=True)
  accum = torch.full((256, 4), 0.1, device=DEV)
  store = HashSpillStore(4, (4,))
  pool = distinct_keys(rng, 210)
  fill_over_steps(t, rng, np.array_split(pool[:100], 3))
  assert t.maybe_evict(0.75, 0.5, slots=[(accum, 0.1)], spill=store) is None and len(store) == 0
  fill_over_steps(t, rng, np.array_split(pool[100:], 4), first_step=4)
  slots = host(t.find(dev(pool)))
  assert (slots >= 0).all() and t.size() == 210 > 0.75 * 256
  accum[dev(slots)] = dev(key_rows(pool, 4))
  st = State(t)
  out = t.maybe_evict(0.75, 0.5, slots=[(accum, 0.1)], spill=store)
  assert out is not None and len(out) == 1 and out[0] is not accum
  sel = sref.select(st.keys, st.last_seen, st.freq, 128)
  left = np.sort(st.keys[sref.selected_mask(st.keys, st.last_seen, st.freq, sel)])
  assert t.capacity == 256 and t.tombstones() == 0 and t.size() == 210 - left.size <= 128   # bounded and rehashed
  np.testing.assert_array_equal(host(store.keys()), left)                 # the store holds exactly the keys that left
  now = host(t.find(dev(pool)))
  kept = now >= 0
  assert (kept == ~np.isin(pool, left)).all()
  np.testing.assert_array_equal(host(out[0])[now[kept]], key_rows(pool[kept], 4))          # the survivors' companions
  np.testing.assert_array_equal(host(t.table)[now[kept]], st.table[slots[kept]])
  # ... and what left is in the store with the payload it had
  gone = store.peek(torch.from_numpy(pool))
  order = np.argsort(pool[~kept])
  np.testing.assert_array_equal(gone.keys.numpy(), pool[~kept][order])
  np.testing.assert_array_equal(gone.rows.numpy(), st.table[slots[~kept]][order])
  np.testing.assert_array_equal(gone.slots[0].numpy(), key_rows(pool[~kept], 4)[order])
  np.testing.assert_array_equal(gone.last_seen.numpy(), st.last_seen[slots[~kept]][order])
  # through a lookup: the list form, and the rebind
  look = HashGroupLookup([t])
  t.set_step(9)
  look([dev(distinct_keys(rng, 90))], [None])
  res = look.maybe_evict(0.75, 0.5, slots=[[(out[0], 0.1)]], spill=[store])
  assert res[0] is not None and t.size() <= 128 and t.size() + len(store) == 300 and t.tombstones() == 0
