"""The device-side miss list on the GPU (hbk_hash_missing_n, hash_missing / hash_missing_sequence, hash_fault_in,
HashGroupLookup.fault_in through it, HashSequenceLookup.fault_in) against the numpy restatement of
tests/support/hash_missing_ref.py.  Everything is compared bit for bit, the order of the missed ids included: slots,
the ids and their count are functions of the inputs alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (HashGroupLookup, HashSequenceLookup, HashSpillStore, HashTable,
                                         SequenceLookupGrad, hash_fault_in, hash_missing, hash_missing_sequence,
                                         hash_translate_sequence)
from tests.support import hash_missing_ref as mref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
EMPTY, TOMB = mref.EMPTY, mref.TOMBSTONE
GUARD = -0x5a5a5a5a5a5a5a5a      # what the outputs hold before the call


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def distinct_keys(rng, n):
  k = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=2 * n + 8, dtype=np.int64))
  rng.shuffle(k)
  return k[:n]


def table_with(keys, capacity=256, slab=8, dim=4, **kw):
  t = HashTable(capacity, dim, DEV, slab_size=slab, expiring=True, **kw)
  t.set_step(1)
  if len(keys):
    got = t.lookup_or_insert(dev(np.asarray(keys, np.int64)))
    assert bool((got >= 0).all().item())
  return t


class Call:
  """One hbk_hash_missing_n call over prepared buffers: slots pre-set to -7, outputs and the guard word behind them
  to GUARD, counts to -5, the workspace to garbage (the call clears what it uses)."""

  def __init__(self, tables, ids, seqs=None, caps=None):
    n = len(tables)
    self.n = n
    self.cols = (_lib.HashMissingColumn * n)()
    self.seqs = (_lib.HashSequence * n)() if seqs is not None else None
    self.ids = [i if isinstance(i, torch.Tensor) else dev(np.asarray(i, np.int64)) for i in ids]
    self.splits, self.slots, self.outs, self.caps = [], [], [], []
    self.counts = torch.full((n,), -5, dtype=torch.int64, device=DEV)
    for c, (t, i) in enumerate(zip(tables, self.ids)):
      positions = i.numel()
      if seqs is not None:
        splits, T, pad = seqs[c]
        s = None if splits is None else dev(np.asarray(splits, np.int32))
        self.splits.append(s)
        B = i.numel() if s is None else s.numel() - 1
        q = self.seqs[c]
        q.row_splits, q.n_segments, q.max_len = (s.data_ptr() if s is not None else None), B, T
        q.has_pad, q.pad_id, q.lengths = (0 if pad is None else 1), (pad or 0), None
        positions = B * T
      cap = positions if caps is None else caps[c]
      self.caps.append(cap)
      self.slots.append(torch.full((max(positions, 1),), -7, dtype=torch.int64, device=DEV)[:positions])
      self.outs.append(torch.full((cap + 1,), GUARD, dtype=torch.int64, device=DEV))
      col = self.cols[c]
      col.keys_cache, col.slab_count, col.slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
      t._describe_expiry(col.exp)
      col.keys, col.n_keys = (i.data_ptr() if i.numel() else None), i.numel()
      col.slots = self.slots[c].data_ptr() if positions else None
      col.out_ids, col.out_capacity = self.outs[c].data_ptr(), cap
      col.count = self.counts.data_ptr() + 8 * c
    lib = _lib.lib()
    self.nbytes = lib.hbk_hash_missing_workspace_bytes(n, self.cols, self.seqs)
    self.workspace = torch.randint(-2 ** 62, 2 ** 62, (self.nbytes // 8 + 1,), dtype=torch.int64, device=DEV)

  def launch(self, stream=None):
    s = _lib.current_stream(torch.device(DEV)) if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(_lib.lib().hbk_hash_missing_n(self.n, self.cols, self.seqs, self.workspace.data_ptr(), self.nbytes, s))

  def results(self):
    torch.cuda.synchronize()
    return [(host(s), host(o), int(k)) for s, o, k in zip(self.slots, self.outs, self.counts.tolist())]


def check_column(got, want_slots, want_missed, cap=None):
  """One column of Call.results() against the restatement: slots, the count, the ids in order, and everything from
  min(count, capacity) on -- the guard word included -- untouched."""
  slots, out, count = got
  np.testing.assert_array_equal(slots, want_slots)
  assert count == want_missed.size
  cap = out.size - 1 if cap is None else cap
  k = min(count, cap)
  np.testing.assert_array_equal(out[:k], want_missed[:k])
  assert (out[k:] == GUARD).all()


POOL = distinct_keys(np.random.RandomState(50), 40)
POOL[:4] = [-1, -2 ** 40, 0, 2 ** 62]          # negatives and zero are ordinary ids


# ---- 1. flat id lists ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1025, 5000])
def test_flat_against_the_reference(n):
  """n crosses lane, wave, 256-position (count / write) and 1024-position (claim) tile boundaries; ids from 40
  values, so duplicates dominate.  Per slab size: every id resident, an empty table, half resident."""
  rng = np.random.RandomState(100 + n)
  ids = POOL[rng.randint(0, POOL.size, size=n)]
  for slab in (4, 8, 32):
    for resident in (POOL, POOL[:0], POOL[::2]):
      t = table_with(resident, slab=slab)
      call = Call([t], [ids])
      call.launch()
      want_slots, want = mref.missing(host(t.keys), ids)
      got = call.results()[0]
      check_column(got, want_slots, want)
      if resident.size == POOL.size:
        assert got[2] == 0 and (got[1] == GUARD).all()                    # count 0, out_ids untouched
      if resident.size == 0:
        assert (got[0] == -1).all() and got[2] == np.unique(ids).size
      # the Python form: the same ids, narrowed to the count
      np.testing.assert_array_equal(host(t.missing(dev(ids))), want)
  assert host(hash_missing([t, t], [dev(ids), dev(ids[:0])])[1]).size == 0


def test_first_occurrence_decides_the_order_across_tiles():
  """One id at positions 0 and 1030 (another claim tile) and nowhere else is reported once, first; an id that
  stands only at the end comes last."""
  rng = np.random.RandomState(7)
  t = table_with(POOL[:20])
  ids = POOL[20 + rng.randint(0, 10, size=1200)]          # POOL[20:30]: all missing
  lone, last = np.int64(77), np.int64(-78)
  ids[0] = ids[1030] = lone
  ids[1199] = last
  call = Call([t], [ids])
  call.launch()
  want_slots, want = mref.missing(host(t.keys), ids)
  assert want[0] == lone and want[-1] == last and (want == lone).sum() == 1
  check_column(call.results()[0], want_slots, want)


def test_one_cell_contention():
  t = table_with(POOL[:20])
  ids = np.full(2000, 123456789, np.int64)
  call = Call([t], [ids])
  call.launch()
  slots, out, count = call.results()[0]
  assert count == 1 and out[0] == 123456789 and (out[1:] == GUARD).all() and (slots == -1).all()


def test_sentinels_are_never_reported_and_negatives_are_ordinary():
  rng = np.random.RandomState(8)
  t = table_with([-1, -5, 9])
  ids = np.array([EMPTY, TOMB, -1, -7, EMPTY, -2 ** 62, TOMB, -7, 9, TOMB + 1, -5, 2 ** 63 - 1], np.int64)
  ids = np.concatenate([ids, ids[rng.permutation(ids.size)]])
  call = Call([t], [ids])
  call.launch()
  want_slots, want = mref.missing(host(t.keys), ids)
  assert want.tolist()[:4] == [-7, -2 ** 62, TOMB + 1, 2 ** 63 - 1] and want.size == 4
  check_column(call.results()[0], want_slots, want)
  only = np.array([EMPTY, TOMB] * 40, np.int64)           # a batch of sentinels alone: nothing, and no id behind it
  call = Call([t], [only])
  call.launch()
  check_column(call.results()[0], np.full(80, -1, np.int64), np.zeros(0, np.int64))


def test_evicted_keys_are_reported():
  t = table_with(POOL[:30])
  t.set_step(5)
  t.lookup_or_insert(dev(POOL[:10]))
  t.evict(3)                                              # the keys last seen at step 1 leave
  assert t.tombstones() == 20
  rng = np.random.RandomState(9)
  ids = POOL[rng.randint(0, 30, size=300)]
  call = Call([t], [ids])
  call.launch()
  want_slots, want = mref.missing(host(t.keys), ids)
  assert set(want.tolist()) == set(POOL[10:30].tolist()) & set(ids.tolist()) and want.size > 10
  check_column(call.results()[0], want_slots, want)


def test_the_table_is_not_written_and_two_runs_agree():
  rng = np.random.RandomState(10)
  t = table_with(POOL[::2], min_freq=1, sketch_depth=2)   # a filtered expiring table: the sketch is watched too
  t.set_step(4)
  t.lookup_or_insert(dev(POOL[:6]))
  t.evict(2)
  names = ('keys', 'table', 'last_seen', 'freq', 'counts', 'stats', 'step', 'sketch', 'filter_counts')
  before = {k: host(getattr(t, k)).copy() for k in names}
  ids = np.concatenate([POOL[rng.randint(0, POOL.size, size=700)], [EMPTY, TOMB]])
  runs = []
  for _ in range(2):
    call = Call([t], [ids])
    call.launch()
    runs.append(call.results()[0])
    for k in names:
      assert host(getattr(t, k)).tobytes() == before[k].tobytes(), k
  for a, b in zip(runs[0], runs[1]):
    np.testing.assert_array_equal(a, b)
  want_slots, want = mref.missing(before['keys'], ids)
  check_column(runs[0], want_slots, want)
  # the Python forms leave it alone as well
  t.missing(dev(ids))
  hash_missing_sequence([t], [dev(ids)], None, 3, 5)
  for k in names:
    assert host(getattr(t, k)).tobytes() == before[k].tobytes(), k


def test_output_smaller_than_the_count():
  rng = np.random.RandomState(11)
  t = table_with(POOL[:5])
  ids = POOL[rng.randint(0, POOL.size, size=900)]
  want_slots, want = mref.missing(host(t.keys), ids)
  assert want.size > 20
  for cap in (0, 1, 7, want.size - 1, want.size):
    call = Call([t], [ids], caps=[cap])
    call.launch()
    got = call.results()[0]
    assert got[2] == want.size                                            # the count is exact
    check_column(got, want_slots, want, cap)                              # the prefix, and nothing behind it


def test_several_tables_in_one_call():
  rng = np.random.RandomState(12)
  tables = [table_with(POOL[:25], capacity=256, slab=4), table_with(POOL[10:], capacity=512, slab=16, dim=8),
            table_with(POOL[:0], capacity=64, slab=32), table_with(POOL[:3], capacity=64, slab=8)]
  ids = [POOL[rng.randint(0, POOL.size, size=n)] for n in (1500, 333, 0, 64)]
  call = Call(tables, ids)
  call.launch()
  for t, i, got in zip(tables, ids, call.results()):
    check_column(got, *mref.missing(host(t.keys), i))
  for t, i, m in zip(tables, ids, hash_missing(tables, [dev(i) for i in ids])):
    np.testing.assert_array_equal(host(m), mref.missing(host(t.keys), i)[1])


def test_more_tables_than_a_launch_group():
  rng = np.random.RandomState(13)
  tables = [table_with(POOL[rng.permutation(POOL.size)[:c % 7 * 5]], capacity=64) for c in range(34)]
  ids = [POOL[rng.randint(0, POOL.size, size=0 if c == 5 else 70)] for c in range(34)]
  call = Call(tables, ids)
  call.launch()
  for t, i, got in zip(tables, ids, call.results()):
    check_column(got, *mref.missing(host(t.keys), i))


# ---- 2. sequences ----------------------------------------------------------------------------------------------
def _sequences(rng, past):
  """Samples of lengths 0, 1, 4 and 9 (twice over, shuffled) at T = 4; `past` stands only behind position T."""
  lens = np.array([0, 1, 4, 9, 9, 4, 1, 0, 9])[rng.permutation(9)]
  splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  ids = POOL[rng.randint(0, 30, size=int(splits[-1]))]
  for b in np.flatnonzero(lens == 9):
    ids[splits[b] + 4 + rng.randint(0, 5)] = past
  return ids, splits


@pytest.mark.parametrize('pad', [None, 'missing', 'resident'])
def test_sequences_against_the_reference(pad):
  rng = np.random.RandomState(14)
  T, past = 4, np.int64(987654321)
  t = table_with(POOL[:15], slab=4)
  ids, splits = _sequences(rng, past)
  single = POOL[rng.randint(0, 30, size=9)]               # one id per sample: row_splits None
  pad_id = {None: None, 'missing': 4242, 'resident': int(POOL[3])}[pad]
  columns = [(ids, splits), (single, None)]
  call = Call([t, t], [ids, single], seqs=[(splits, T, pad_id), (None, T, pad_id)])
  call.launch()
  want = [mref.missing(host(t.keys), i, s, T, pad_id) for i, s in columns]
  assert past in ids.tolist()
  for got, (want_slots, want_missed), (i, s) in zip(call.results(), want, columns):
    check_column(got, want_slots, want_missed)
    assert past not in want_missed.tolist()                               # an id only past T is not reported
    if pad == 'missing':                                                  # once, where the padding first stands
      e, _ = mref.effective(i, s, T, pad_id)
      order = [int(np.flatnonzero(e == k)[0]) for k in want_missed.tolist()]
      assert order == sorted(order) and int(np.flatnonzero(e == pad_id)[0]) in order
      assert (want_missed == pad_id).sum() == 1
  # the grid is the pure find's
  d_ids, d_splits = [dev(ids), dev(single)], [dev(splits), None]
  grids, _ = hash_translate_sequence([t, t], d_ids, d_splits, T, pad_id, insert=False)
  for got, g in zip(call.results(), grids):
    np.testing.assert_array_equal(got[0], host(g))
  # the Python form
  for m, (_, want_missed) in zip(hash_missing_sequence([t, t], d_ids, d_splits, T, pad_id), want):
    np.testing.assert_array_equal(host(m), want_missed)


def test_sequence_fault_in_respects_T_and_brings_the_pad_id_back():
  a, b, c, pad, new = 11, 22, 33, 44, 55
  source = table_with([a, b, c, pad])
  store = HashSpillStore(4)
  source.spill_to(0, store)
  assert store.keys().tolist() == [a, b, c, pad]
  t = table_with([])
  hsl = HashSequenceLookup([t], 2, pad_ids=pad)
  # sample 0: a, new and -- past T -- b; sample 1: c and one padding position
  ids, splits = dev(np.array([a, new, b, c], np.int64)), dev(np.array([0, 3, 4], np.int32))
  assert hsl.fault_in([ids], [splits], [store]) == [3]
  assert store.keys().tolist() == [b]                                      # only past T: it stays in the store
  assert (host(t.find(dev(np.array([a, c, pad, b, new], np.int64)))) >= 0).tolist() == [True, True, True, False, False]
  assert hsl.fault_in([ids], [splits], [store]) == [0]


def test_empty_sequences():
  t = table_with(POOL[:5])
  none = np.zeros(0, np.int64)
  call = Call([t, t, t], [none, none, POOL[:3]],
              seqs=[(np.zeros(1, np.int32), 4, None), (np.zeros(6, np.int32), 4, None), (np.zeros(4, np.int32), 4, 7)])
  call.launch()
  got = call.results()
  assert got[0][2] == 0 and got[0][0].size == 0                           # B == 0
  check_column(got[1], np.full(20, -1, np.int64), none)                   # only empty samples, no pad: nothing
  check_column(got[2], np.full(12, -1, np.int64), np.array([7], np.int64))   # only empty samples, a missing pad id


# ---- 3. a captured call ------------------------------------------------------------------------------------------
def test_captured_call_replays_on_refilled_ids():
  rng = np.random.RandomState(15)
  t = table_with(POOL[:20])
  batches = [POOL[rng.randint(0, POOL.size, size=777)] for _ in range(3)]
  buf = dev(batches[0])
  call = Call([t], [buf])
  call.launch()                                           # warm-up outside the capture
  torch.cuda.synchronize()
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(side):
    with torch.cuda.graph(graph, stream=side):
      call.launch(side)
  torch.cuda.synchronize()
  for ids in batches[1:]:
    buf.copy_(dev(ids))
    call.outs[0].fill_(GUARD)
    graph.replay()
    check_column(call.results()[0], *mref.missing(host(t.keys), ids))


# ---- 4. the fault-in through the batched path ------------------------------------------------------------------
def _spilled_fleet(seed):
  """Three tables of different geometry with one companion each; keys inserted over four steps, the older half
  spilled into the stores of tables 0 and 2 (table 1 spills nothing: its store stays empty)."""
  rng = np.random.RandomState(seed)
  dims = [4, 8, 5]
  tables = [HashTable(cap, d, DEV, slab_size=s, init_scale=0.05, seed=c, expiring=True)
            for c, (cap, d, s) in enumerate(zip([256, 512, 128], dims, [8, 16, 4]))]
  comps = [dev(rng.rand(t.capacity, d).astype(F32)) for t, d in zip(tables, dims)]
  stores = [HashSpillStore(d, (d,)) for d in dims]
  pools = [distinct_keys(rng, 80) for _ in tables]
  for step in range(4):
    for t, pool in zip(tables, pools):
      t.set_step(step + 1)
      t.lookup_or_insert(dev(pool[step * 20:step * 20 + 20]))
  for c in (0, 2):
    tables[c].spill_to(40, stores[c], slots=[(comps[c], 0.25)])
    assert len(stores[c]) == 40
  batch = [np.concatenate([pool[rng.randint(0, 80, size=150)], distinct_keys(rng, 10), [EMPTY, TOMB]])
           for pool in pools]
  return tables, comps, stores, [dev(b) for b in batch]


def _snapshot(tables, comps, stores):
  out = []
  for t, a, st in zip(tables, comps, stores):
    exp = t.export_items(slots=[a])
    order = np.argsort(host(exp.keys))
    out.append([host(x)[order] for x in (exp.keys, exp.rows, exp.last_seen, exp.freq, exp.slots[0])] +
               [st.keys().numpy()] + [x.numpy().copy() for x in st.peek(st.keys()).slots])
  return out


def test_group_fault_in_equals_the_per_table_loop():
  A, B = _spilled_fleet(16), _spilled_fleet(16)
  for x, y in zip(_snapshot(*A[:3]), _snapshot(*B[:3])):
    for a, b in zip(x, y):
      np.testing.assert_array_equal(a, b)
  tables, comps, stores, batch = A
  got = HashGroupLookup(tables).fault_in(batch, stores, [[a] for a in comps])
  tables_b, comps_b, stores_b, batch_b = B
  want = [t.fault_in(i, st, [a]) for t, i, st, a in zip(tables_b, batch_b, stores_b, comps_b)]
  assert got == want and got[1] == 0 and got[0] > 10 and got[2] > 10
  for x, y in zip(_snapshot(*A[:3]), _snapshot(*B[:3])):
    for a, b in zip(x, y):
      assert a.tobytes() == b.tobytes()
  # nothing more to bring; only empty stores: no call at all
  assert hash_fault_in(tables, batch, stores, [[a] for a in comps]) == [0, 0, 0]
  empty = [HashSpillStore(t.dim) for t in tables]
  assert hash_fault_in(tables, batch, empty) == [0, 0, 0]


def test_too_full_table_puts_its_keys_back_and_later_tables_are_untouched():
  rng = np.random.RandomState(17)
  keys = [distinct_keys(rng, 12) for _ in range(3)]
  source = [table_with(k, capacity=64) for k in keys]
  stores = [HashSpillStore(4) for _ in keys]
  for t, st in zip(source, stores):
    t.spill_to(0, st)
    assert len(st) == 12
  tables = [table_with([], capacity=64), table_with([], capacity=8), table_with([], capacity=64)]
  with pytest.raises(_lib.InvalidArgumentError, match='do not fit'):
    hash_fault_in(tables, [dev(k) for k in keys], stores)
  assert tables[0].size() == 12 and len(stores[0]) == 0                   # the table before it was served
  inside = host(tables[1].find(dev(keys[1]))) >= 0
  assert inside.sum() == tables[1].size() == 8 and len(stores[1]) == 4    # what did not fit is back in the store
  assert set(stores[1].keys().tolist()) == set(keys[1][~inside].tolist())
  assert tables[2].size() == 0 and len(stores[2]) == 12                   # the table after it was not taken from


# ---- 5. tiered sequence training ---------------------------------------------------------------------------------
def test_tiered_sequence_training_equals_unbounded_training():
  rng = np.random.RandomState(18)
  T, B, dim, lr, acc0, n_steps, bound, pad_id = 4, 16, 4, 0.1, 0.1, 12, 64, 31337
  pool = distinct_keys(rng, 150)
  lone = np.int64(555555)                                 # read at step 1, afterwards only past T
  batches = []
  for s in range(n_steps):
    lens = rng.randint(0, 8, size=B)
    lens[0] = 7
    splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids = pool[rng.randint(0, pool.size, size=int(splits[-1]))]
    if s == 0:
      ids[0] = lone
    elif s >= n_steps - 3:
      ids[T + 1] = lone                                   # sample 0, position 5: never read
    batches.append((ids, splits, rng.randn(B, T, dim).astype(F32)))

  def run(capacity, tiered):
    t = HashTable(capacity, dim, DEV, slab_size=8, init_scale=0.05, seed=5, expiring=True)
    acc = torch.full_like(t.table, acc0)
    store = HashSpillStore(dim, (dim,))
    hsl = HashSequenceLookup([t], T, pad_ids=pad_id)
    grad = SequenceLookupGrad(hsl, accums=[acc])
    restored, lone_spilled_at = 0, None
    for s, (ids, splits, g) in enumerate(batches, start=1):
      t.set_step(s)
      d_ids, d_splits = dev(ids), dev(splits)
      if tiered:
        restored += hsl.fault_in([d_ids], [d_splits], [store], [[acc]])[0]
      hsl([d_ids], [d_splits])
      grid = host(hsl.grids[0])
      assert (grid >= 0).all()                            # (every position holds an id or the pad id)
      grad([dev(g)], apply_lr=lr, optimizer='adagrad', deterministic=True)
      if tiered:
        t.spill_to(bound, store, slots=[(acc, acc0)])
        assert t.size() <= bound
        if lone_spilled_at is None and lone in store.keys().tolist():
          lone_spilled_at = s
    return t, acc, store, restored, lone_spilled_at

  tiered, acc, store, restored, lone_spilled_at = run(512, True)
  whole, whole_acc, _, _, _ = run(2048, False)
  assert restored >= 20 and tiered.failed() == 0 and whole.failed() == 0   # keys did leave and come back
  # spilled before it stood past T, and still in the store: the fault-in never asked for it
  assert lone_spilled_at is not None and lone_spilled_at < n_steps - 3
  assert lone in store.keys().tolist() and int(tiered.find(dev(np.array([lone])))[0].item()) < 0
  seen = np.unique(np.concatenate([mref.effective(i, s, T, pad_id)[0] for i, s, _ in batches]))
  at, ref_at = host(tiered.find(dev(seen))), host(whole.find(dev(seen)))
  spilled = store.peek(torch.from_numpy(seen))
  in_store = np.isin(seen, spilled.keys.numpy())
  assert ((at >= 0) ^ in_store).all() and in_store.any() and (ref_at >= 0).all()
  for on_device, in_host, ref_array in ((tiered.table, spilled.rows, whole.table),
                                        (acc, spilled.slots[0], whole_acc)):
    got = np.empty((seen.size, dim), F32)
    got[at >= 0] = host(on_device)[at[at >= 0]]
    got[in_store] = in_host.numpy()
    np.testing.assert_array_equal(got, host(ref_array)[ref_at])           # rows and accumulators, bit for bit
