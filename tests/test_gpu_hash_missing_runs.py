"""hbk_hash_missing_runs_n on the GPU: the miss list over ids that arrive as runs.  Every case is compared bit for bit
-- the runs' slots, out_ids in order, count, the words behind the output and every array of the table -- with the
numpy restatement (tests/support/hash_missing_ref.py) applied to the concatenation of the column's runs, and with
hbk_hash_missing_n run on the device over the same ids concatenated."""
import ctypes as C

import numpy as np
import pytest
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import HashTable
from tests.support import hash_missing_ref as mref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EMPTY, TOMB = mref.EMPTY, mref.TOMBSTONE
GUARD = -0x5a5a5a5a5a5a5a5a      # what the outputs hold before the call
TABLE_ARRAYS = ('keys', 'table', 'last_seen', 'freq', 'counts', 'stats', 'step')


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def distinct_keys(rng, n):
  k = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=2 * n + 8, dtype=np.int64))
  rng.shuffle(k)
  return k[:n]


def table_with(keys, capacity=256, slab=8, dim=16):
  t = HashTable(capacity, dim, DEV, slab_size=slab, expiring=True)
  t.set_step(1)
  if len(keys):
    got = t.lookup_or_insert(dev(np.asarray(keys, np.int64)))
    assert bool((got >= 0).all().item())
  return t


def snapshot(t):
  return {k: host(getattr(t, k)).tobytes() for k in TABLE_ARRAYS}


def describe_table(col, t):
  col.keys_cache, col.slab_count, col.slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
  t._describe_expiry(col.exp)


class RunsCall:
  """One hbk_hash_missing_runs_n call over prepared buffers: every run's slots pre-set to -7, outputs and the guard
  word behind them to GUARD, counts to -5, the workspace to garbage (the call clears what it uses).  A run of
  length 0 has NULL buffers."""

  def __init__(self, tables, runs, caps=None):
    n = len(tables)
    self.n = n
    self.cols = (_lib.HashMissingRunsColumn * n)()
    self.n_runs = (C.c_int32 * n)(*[len(r) for r in runs])
    self.run_arrays = [(_lib.HashRun * max(len(r), 1))() for r in runs]
    self.run_ptrs = (C.c_void_p * n)(*[C.addressof(a) if len(r) else None for a, r in zip(self.run_arrays, runs)])
    self.ids = [[dev(np.asarray(i, np.int64)) for i in r] for r in runs]
    self.slots = [[torch.full((max(i.numel(), 1),), -7, dtype=torch.int64, device=DEV)[:i.numel()] for i in r]
                  for r in self.ids]
    self.counts = torch.full((max(n, 1),), -5, dtype=torch.int64, device=DEV)
    self.outs, self.caps = [], []
    for c, t in enumerate(tables):
      total = sum(i.numel() for i in self.ids[c])
      cap = total if caps is None else caps[c]
      self.caps.append(cap)
      self.outs.append(torch.full((cap + 1,), GUARD, dtype=torch.int64, device=DEV))
      col = self.cols[c]
      describe_table(col, t)
      col.out_ids, col.out_capacity = self.outs[c].data_ptr(), cap
      col.count = self.counts.data_ptr() + 8 * c
      for q, (i, s) in enumerate(zip(self.ids[c], self.slots[c])):
        r = self.run_arrays[c][q]
        r.keys, r.slots, r.n_keys = (i.data_ptr(), s.data_ptr(), i.numel()) if i.numel() else (None, None, 0)
    self.nbytes = _lib.lib().hbk_hash_missing_runs_workspace_bytes(n, self.n_runs, self.run_ptrs)
    self.workspace = torch.randint(-2 ** 62, 2 ** 62, (self.nbytes // 8 + 2,), dtype=torch.int64, device=DEV)

  def launch(self, stream=None):
    s = _lib.current_stream(torch.device(DEV)) if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(_lib.lib().hbk_hash_missing_runs_n(self.n, self.cols, self.n_runs, self.run_ptrs,
                                                  self.workspace.data_ptr(), self.nbytes, s))

  def results(self):
    """Per column: (the runs' slots concatenated, the output with its guard word, the count)."""
    torch.cuda.synchronize()
    counts = self.counts.tolist()
    return [(np.concatenate([host(s) for s in self.slots[c]] + [np.zeros(0, np.int64)]), host(self.outs[c]),
             int(counts[c])) for c in range(self.n)]


def flat_on_device(tables, ids, caps):
  """hbk_hash_missing_n over the concatenated ids: per column (slots, output with its guard word, count)."""
  n = len(tables)
  cols = (_lib.HashMissingColumn * n)()
  d_ids = [dev(i) for i in ids]
  slots = [torch.full((max(i.size, 1),), -7, dtype=torch.int64, device=DEV)[:i.size] for i in ids]
  outs = [torch.full((cap + 1,), GUARD, dtype=torch.int64, device=DEV) for cap in caps]
  counts = torch.full((max(n, 1),), -5, dtype=torch.int64, device=DEV)
  for c, t in enumerate(tables):
    col = cols[c]
    describe_table(col, t)
    col.keys, col.n_keys = (d_ids[c].data_ptr() if ids[c].size else None), ids[c].size
    col.slots = slots[c].data_ptr() if ids[c].size else None
    col.out_ids, col.out_capacity, col.count = outs[c].data_ptr(), caps[c], counts.data_ptr() + 8 * c
  lib = _lib.lib()
  nbytes = lib.hbk_hash_missing_workspace_bytes(n, cols, None)
  workspace = torch.zeros(nbytes // 8 + 2, dtype=torch.int64, device=DEV)
  _lib.check(lib.hbk_hash_missing_n(n, cols, None, workspace.data_ptr(), nbytes, _lib.current_stream(torch.device(DEV))))
  torch.cuda.synchronize()
  return [(host(s), host(o), int(k)) for s, o, k in zip(slots, outs, counts.tolist())]


def check(tables, runs, caps=None, call=None):
  """The runs call against the restatement and against the flat call on the device; the tables are not written.
  Returns the restatement's missed ids per column."""
  before = [snapshot(t) for t in tables]
  if call is None:
    call = RunsCall(tables, runs, caps)
    call.launch()
  got = call.results()
  after_runs = [snapshot(t) for t in tables]
  concat = [np.concatenate([np.asarray(i, np.int64) for i in r] + [np.zeros(0, np.int64)]) for r in runs]
  flat = flat_on_device(tables, concat, call.caps)
  wants = []
  for c, t in enumerate(tables):
    want_slots, want = mref.missing(host(t.keys), concat[c])
    slots, out, count = got[c]
    np.testing.assert_array_equal(slots, want_slots, err_msg=f'column {c}')
    assert count == want.size, (c, count, want.size)
    k = min(count, call.caps[c])
    np.testing.assert_array_equal(out[:k], want[:k], err_msg=f'column {c}')
    assert (out[k:] == GUARD).all(), f'column {c}: written behind min(count, out_capacity)'
    for a, b in zip(got[c][:2], flat[c][:2]):
      assert a.tobytes() == b.tobytes(), f'column {c}: differs from hbk_hash_missing_n on the concatenation'
    assert flat[c][2] == count
    assert after_runs[c] == before[c], f'column {c}: the table was written'
    wants.append(want)
  return wants


POOL = distinct_keys(np.random.RandomState(60), 48)
POOL[:4] = [-1, -2 ** 40, 0, 2 ** 62]          # negatives and zero are ordinary ids
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)


@pytest.fixture(scope='module')
def half():
  """512 slots in slabs of 8, dim 16: every second id of the pool is resident."""
  return table_with(POOL[::2], capacity=512, slab=8, dim=16)


@pytest.fixture(scope='module')
def odd():
  """320 slots in slabs of 5, dim 6: the first third of the pool is resident."""
  return table_with(POOL[:16], capacity=320, slab=5, dim=6)


def draw(rng, n, pool=POOL):
  return pool[rng.randint(0, pool.size, size=n)]


# ---- run counts and run lengths -----------------------------------------------------------------------------------
@pytest.mark.parametrize('n_runs', [0, 1, 3, 8])
def test_run_counts(half, odd, n_runs):
  rng = np.random.RandomState(200 + n_runs)
  for lengths in ([300, 65, 1025, 1, 64, 257, 63, 256][:n_runs], [7] * n_runs):
    runs = [[draw(rng, n) for n in lengths], [draw(rng, n) for n in lengths[::-1]]]
    wants = check([half, odd], runs)
    assert n_runs == 0 or all(w.size > 0 for w in wants)


@pytest.mark.parametrize('n', LENGTHS)
def test_run_lengths_with_empty_runs_first_in_the_middle_and_last(half, odd, n):
  """Every length stands first, in the middle and last among runs of the other lengths, and beside empty runs at
  the three places; the lengths cross lane, wave and tile boundaries."""
  rng = np.random.RandomState(300 + n)
  others = [m for m in LENGTHS if m != n][:3]
  for lengths in ([n] + others, others[:1] + [n] + others[1:], others + [n],
                  [0, n, 0, 0, others[0], 0], [0, 0, n], [n, 0, 0]):
    check([half, odd], [[draw(rng, m) for m in lengths], [draw(rng, m) for m in lengths]])


# ---- one id list, cut into runs: the flat call's answer, bit for bit -------------------------------------------------
WIDE = distinct_keys(np.random.RandomState(61), 1200)


@pytest.fixture(scope='module')
def wide():
  """2048 slots in slabs of 8: every second id of the wide pool is resident."""
  return table_with(WIDE[::2], capacity=2048, slab=8, dim=4)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_one_list_cut_into_runs_answers_as_the_flat_call(wide, n):
  """Both entries claim into one scratch set (csrc/hash_miss_set.h): over the same ids E -- about half of them
  resident, one missed id at both ends, so in the first and in the last run -- hbk_hash_missing_n on E and
  hbk_hash_missing_runs_n on E cut into runs report the same count and the same ids in the same order.  The lengths
  are the edges of a wave (64), of a compaction tile (256) and of a claim tile (1024)."""
  rng = np.random.RandomState(400 + n)
  ids = draw(rng, n, WIDE)
  ids[0] = ids[-1] = WIDE[1]
  flat_slots, flat_out, flat_count = flat_on_device([wide], [ids], [n])[0]
  assert 0 < flat_count <= n and (n == 1 or bool((flat_slots >= 0).any()))
  assert flat_out[0] == WIDE[1] and (flat_out[:flat_count] == WIDE[1]).sum() == 1
  cuts = ([ids], [ids[:1], ids[1:]], [ids[:n - 1], ids[n - 1:]], [ids[:n // 2], ids[:0], ids[n // 2:]])
  for runs in cuts:
    call = RunsCall([wide], [runs])
    call.launch()
    slots, out, count = call.results()[0]
    assert count == flat_count, [r.size for r in runs]
    assert out.tobytes() == flat_out.tobytes(), [r.size for r in runs]
    assert slots.tobytes() == flat_slots.tobytes(), [r.size for r in runs]


# ---- order across runs ---------------------------------------------------------------------------------------------
def test_an_id_in_two_runs_is_reported_once_at_its_earlier_run(half):
  rng = np.random.RandomState(21)
  missing = POOL[1::2]
  lone, late = np.int64(777), np.int64(-778)
  runs = [draw(rng, 70, missing[:5]), draw(rng, 300, missing[5:12]), draw(rng, 64, missing[:5])]
  runs[0][69] = lone            # the last id of run 0 ...
  runs[2][0] = lone             # ... again at the start of run 2
  runs[2][63] = late            # only here
  runs[1][:] = np.where(runs[1] == missing[5], missing[6], runs[1])
  runs[1][299] = missing[5]     # missed once at the end of run 1 ...
  runs.append(np.full(500, missing[5], np.int64))   # ... and five hundred times in run 3
  want = check([half], [runs])[0]
  assert (want == lone).sum() == 1 and (want == late).sum() == 1 and (want == missing[5]).sum() == 1
  order = want.tolist()
  assert order.index(lone) < order.index(missing[5]) < order.index(late)
  # the same runs in another order: the earlier run still decides
  want = check([half], [runs[::-1]])[0]
  assert want[0] == missing[5]


def test_one_id_everywhere(half):
  check([half], [[np.full(n, 123456789, np.int64) for n in (257, 1, 1025, 64)]])


# ---- all resident, all missing -------------------------------------------------------------------------------------
def test_all_resident_and_all_missing(half, odd):
  rng = np.random.RandomState(22)
  resident = [[draw(rng, n, POOL[::2]) for n in (65, 0, 256, 300)], [draw(rng, n, POOL[:16]) for n in (1025, 1)]]
  wants = check([half, odd], resident)
  assert all(w.size == 0 for w in wants)
  absent = [[draw(rng, n, POOL[1::2]) for n in (65, 0, 256, 300)], [draw(rng, n, POOL[16:]) for n in (1025, 1)]]
  wants = check([half, odd], absent)
  assert wants[0].size == np.unique(np.concatenate(absent[0])).size
  empty = table_with(POOL[:0], capacity=64, slab=8, dim=16)
  check([empty], [[draw(rng, 257), draw(rng, 64)]])


# ---- tombstones and sentinels ----------------------------------------------------------------------------------------
def test_tombstoned_ids_are_reported():
  t = table_with(POOL[:30], capacity=256, slab=5, dim=6)
  t.set_step(5)
  t.lookup_or_insert(dev(POOL[:10]))
  t.evict(3)                                              # the keys last seen at step 1 leave
  assert t.tombstones() == 20
  rng = np.random.RandomState(23)
  runs = [draw(rng, n, POOL[:30]) for n in (100, 257, 64)]
  want = check([t], [runs])[0]
  assert set(want.tolist()) == set(POOL[10:30].tolist()) & set(np.concatenate(runs).tolist()) and want.size > 10


def test_sentinels_are_never_reported(half):
  rng = np.random.RandomState(24)
  ids = np.array([EMPTY, TOMB, -1, -7, EMPTY, -2 ** 62, TOMB, -7, POOL[2], TOMB + 1, POOL[1], 2 ** 63 - 1], np.int64)
  runs = [ids, ids[rng.permutation(ids.size)], np.array([EMPTY, TOMB] * 40, np.int64), ids[::-1].copy()]
  want = check([half], [runs])[0]
  assert EMPTY not in want.tolist() and TOMB not in want.tolist() and TOMB + 1 in want.tolist()
  check([half], [[np.array([EMPTY, TOMB] * 40, np.int64), np.array([TOMB], np.int64)]])   # sentinels alone: nothing


# ---- a short output --------------------------------------------------------------------------------------------------
def test_out_capacity_one_short_of_the_count(half, odd):
  rng = np.random.RandomState(25)
  runs = [[draw(rng, n) for n in (300, 65, 257)], [draw(rng, n) for n in (64, 1025)]]
  wants = check([half, odd], runs)
  assert all(w.size > 10 for w in wants)
  for caps in ([w.size - 1 for w in wants], [0, wants[1].size], [1, 7]):
    check([half, odd], runs, caps=caps)                   # the exact count, the prefix, the canary untouched


# ---- more than one launch group ----------------------------------------------------------------------------------------
def test_33_columns_of_8_runs():
  """33 columns x 8 runs: more columns than a launch group takes (32) and more runs (264 > 256); a column without
  ids and a column with empty runs among them."""
  rng = np.random.RandomState(26)
  tables = [table_with(POOL[rng.permutation(POOL.size)[:c % 7 * 5]], capacity=64, slab=(8, 5)[c % 2],
                       dim=(16, 6)[c % 2]) for c in range(33)]
  runs = [[draw(rng, 0 if c == 5 or (c == 9 and q % 2) else (3, 70, 257)[(c + q) % 3]) for q in range(8)]
          for c in range(33)]
  wants = check(tables, runs)
  assert wants[5].size == 0 and sum(w.size > 0 for w in wants) >= 30


# ---- capture -------------------------------------------------------------------------------------------------------------
def test_a_captured_call_replays_on_refilled_id_buffers(half, odd):
  rng = np.random.RandomState(27)
  lengths = (257, 64, 0, 300)
  runs = [[draw(rng, n, POOL[:24]) for n in lengths], [draw(rng, n, POOL[:24]) for n in lengths]]
  call = RunsCall([half, odd], runs)
  stream = torch.cuda.Stream(DEV)
  stream.wait_stream(torch.cuda.current_stream(DEV))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(stream):
    call.launch(stream)                                   # (warm-up outside the capture)
    stream.synchronize()
    with torch.cuda.graph(graph, stream=stream):
      call.launch(stream)
  graph.replay()
  check([half, odd], runs, call=call)
  # other ids in the same buffers, the outputs reset: the replay reads what the buffers now hold
  runs = [[draw(rng, n, POOL[20:]) for n in lengths], [draw(rng, n, POOL[20:]) for n in lengths]]
  for c in range(2):
    for q, i in enumerate(runs[c]):
      call.ids[c][q].copy_(dev(i))
      call.slots[c][q].fill_(-7)
    call.outs[c].fill_(GUARD)
  call.counts.fill_(-5)
  call.workspace.random_(-2 ** 62, 2 ** 62)
  torch.cuda.synchronize()
  graph.replay()
  check([half, odd], runs, call=call)
