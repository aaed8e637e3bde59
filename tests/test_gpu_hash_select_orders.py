"""The two orders of a bounded table are one select and one spill (csrc/hash_order.h): LFU's key is the pair
(freq, last_seen), LRU's is last_seen alone, so LFU over keys of ONE freq class must be LRU -- the same need, the
same cut, the same slots, the same export -- and LFU over keys of ONE age must not be: LRU then has a single class,
which leaves whole or stays, and LFU cuts inside it.

One expiring table asked for with 1100 slots in slabs of 8 (1096 slots: more than one 1024-slot tile of the select
with a ragged last wave, five 256-slot tiles of the spill with a ragged last one), dim 4, one companion of dim 3 with
a non-zero fill, 700 live keys at scattered slots and a few tombstones between them.  `ages`: every key has freq 2
and last_seen spread over negative and positive values, some fifty keys per value, so every cut has ties.  `counts`
is the mirror: every key has last_seen 5 and freq takes those values.

Cases: max_size in {0, 1, 350, 699, 700, 5000}; keep_freq 0 and 3 protect nobody of `ages`, keep_freq 2 protects
everybody, which with need > 0 is the branch "fewer evictable slots than need: all of them go" with none to go.

The first two tests need no GPU: they assert the same equalities between the numpy restatements
(tests/support/hash_evict_to_ref.py, hash_spill_ref.py, hash_evict_lfu_ref.py), so the shapes are known to reach
what they are meant to reach before a GPU sees them.  Everything is integer or a copy and compared bit for bit."""
import numpy as np
import pytest
import torch

from hybridbackend_amd.embedding import HashTable, hash_evict_to, hash_evict_to_select, hash_spill
from tests.support import hash_evict_lfu_ref as lref
from tests.support import hash_evict_to_ref as tref
from tests.support import hash_spill_ref as sref

DEV = 'cuda:0'
F32 = np.float32
EMPTY, TOMB = tref.EMPTY, tref.TOMBSTONE
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
ASKED, SLAB, DIM, COMP_DIM, FILL = 1100, 8, 4, 3, 0.25
CAP = ASKED // SLAB * SLAB
N_LIVE, N_TOMB = 700, 6
MAX_SIZES = (0, 1, 350, 699, 700, 5000)
KEEP_FREQS = (0, 3, 2)
LRU_WORDS = [0, 1, 3, 4]                        # where LRU's {live_before, need, cut, n_evicted} lie in LFU's report


def arrays(kind):
  """The table's arrays on the host: dict(keys, last_seen, freq, table, comp)."""
  rng = np.random.RandomState(120)
  where = rng.permutation(CAP)[:N_LIVE + N_TOMB]
  live = where[:N_LIVE]
  keys = np.full(CAP, EMPTY, np.int64)
  keys[live] = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=4 * N_LIVE, dtype=np.int64))[:N_LIVE]
  keys[where[N_LIVE:]] = TOMB
  spread = rng.randint(-6, 7, size=N_LIVE)                                # 13 values: ties at every cut
  spread[:3], spread[3:6] = INT32_MIN, INT32_MAX - 1                      # (INT32_MAX is left to "all of them go")
  one, other = np.zeros(CAP, np.int32), np.zeros(CAP, np.int32)
  one[live], other[live] = spread, 2 if kind == 'ages' else 5
  seen, freq = (one, other) if kind == 'ages' else (other, one)
  return dict(keys=keys, last_seen=seen, freq=freq, table=rng.rand(CAP, DIM).astype(F32),
              comp=rng.rand(CAP, COMP_DIM).astype(F32))


def copy_of(a):
  return {k: v.copy() for k, v in a.items()}


def moves_of(a):
  return [(a['table'], DIM), (a['last_seen'], 1), (a['freq'], 1), (a['comp'], COMP_DIM)]


def ref_evict(mod, a, max_size, keep_freq):
  """mod.evict_to on a copy: (report, mask, arrays after)."""
  a = copy_of(a)
  report, mask = mod.evict_to(a['keys'], a['last_seen'], a['freq'], max_size, keep_freq,
                              [(a['comp'], COMP_DIM, F32(FILL))])
  return report, mask, a


def ref_spill(mod, a, selection, keep_freq):
  """mod.spill: (export, arrays after)."""
  export, after, n_evicted, count = mod.spill(a['keys'], a['last_seen'], a['freq'], selection, keep_freq, moves_of(a),
                                              [(a['comp'], COMP_DIM, F32(FILL))])
  assert n_evicted == count == export['keys'].size
  return export, dict(keys=after['cache'], last_seen=after['last_seen'], freq=after['freq'], table=a['table'],
                      comp=after['companions'][0])


def same_arrays(a, b):
  for name in ('keys', 'last_seen', 'freq', 'table', 'comp'):
    np.testing.assert_array_equal(a[name], b[name], err_msg=name)


def same_export(a, b):
  np.testing.assert_array_equal(a['keys'], b['keys'])
  np.testing.assert_array_equal(a['src_slots'], b['src_slots'])
  assert len(a['moves']) == len(b['moves']) == 4
  for x, y in zip(a['moves'], b['moves']):
    np.testing.assert_array_equal(x, y)


def expected_cut_freq(need, n_evictable):
  """cut_freq of the LFU report over `ages`: 0 inside the bound, INT32_MAX where all go, else the one class."""
  return 0 if need <= 0 else INT32_MAX if n_evictable < need else 2


def check_lfu_is_lru(lfu, lru, n_evictable):
  """The LFU report of `ages` against the LRU report, word for word."""
  lfu, lru = np.asarray(lfu), np.asarray(lru)
  assert lfu.dtype == lru.dtype == np.int32 and lfu.shape == (8,) and lru.shape == (4,)
  np.testing.assert_array_equal(lfu[LRU_WORDS], lru)
  assert lfu[2] == expected_cut_freq(int(lru[1]), n_evictable)
  assert (lfu[2] == INT32_MAX) == (lru[2] == INT32_MAX)
  assert lfu[5:].tolist() == [0, 0, 0]


# ---- without a GPU: the restatements --------------------------------------------------------------------------
@pytest.mark.parametrize('keep_freq', KEEP_FREQS)
def test_restatements_one_freq_class_is_lru(keep_freq):
  a = arrays('ages')
  n_evictable = int(tref.evictable_mask(a['keys'], a['freq'], keep_freq).sum())
  assert n_evictable == (0 if keep_freq == 2 else N_LIVE)
  evicted = []
  for max_size in MAX_SIZES:
    lru, lru_mask, lru_after = ref_evict(tref, a, max_size, keep_freq)
    lfu, lfu_mask, lfu_after = ref_evict(lref, a, max_size, keep_freq)
    check_lfu_is_lru(lfu, lru, n_evictable)
    np.testing.assert_array_equal(lfu_mask, lru_mask)
    same_arrays(lfu_after, lru_after)
    lru_sel = sref.select(a['keys'], a['last_seen'], a['freq'], max_size, keep_freq)
    lfu_sel, _ = lref.select(a['keys'], a['last_seen'], a['freq'], max_size, keep_freq)
    np.testing.assert_array_equal(lru_sel, lru)
    np.testing.assert_array_equal(lfu_sel, lfu)
    lru_export, lru_left = ref_spill(sref, a, lru_sel, keep_freq)
    lfu_export, lfu_left = ref_spill(lref, a, lfu_sel, keep_freq)
    same_export(lfu_export, lru_export)
    same_arrays(lfu_left, lru_left)
    same_arrays(lfu_left, lfu_after)
    assert lru[0] == N_LIVE and lru[1] == N_LIVE - max_size
    evicted.append(int(lru[3]))
  if keep_freq == 2:
    assert evicted == [0] * 6                                             # all of them go, and there are none
  else:
    assert evicted[:2] == [N_LIVE, N_LIVE] and evicted[4:] == [0, 0]      # max_size 1: the 3 newest keys are one class
    assert evicted[2] > 350 and evicted[3] == 3                           # ties at the cut leave together


@pytest.mark.parametrize('keep_freq', KEEP_FREQS)
def test_restatements_one_age_class_is_not_lru(keep_freq):
  a = arrays('counts')
  n_evictable = int(tref.evictable_mask(a['keys'], a['freq'], keep_freq).sum())
  assert 300 < n_evictable <= N_LIVE and (n_evictable == N_LIVE) == (keep_freq == 0)
  cuts_inside = 0
  for max_size in MAX_SIZES:
    lru, lru_mask, _ = ref_evict(tref, a, max_size, keep_freq)
    lfu, lfu_mask, _ = ref_evict(lref, a, max_size, keep_freq)
    need = N_LIVE - max_size
    assert lru[1] == lfu[1] == need
    assert lru[3] == (n_evictable if need > 0 else 0)                     # LRU: one class, whole or not at all
    assert not (lfu_mask & ~lru_mask).any() and min(max(need, 0), n_evictable) <= lfu[4] <= lru[3]
    cuts_inside += int(lfu[4] < lru[3])
  assert cuts_inside >= 2                                                 # max_size 350 and 699 at the least


# ---- on the GPU ---------------------------------------------------------------------------------------------------
def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


class Table:
  """A device table holding `arrays(kind)` and its companion; `put` writes the arrays again, `get` reads them."""

  def __init__(self, a):
    self.t = HashTable(ASKED, DIM, DEV, slab_size=SLAB, expiring=True)
    assert self.t.capacity == CAP
    self.comp = torch.empty((CAP, COMP_DIM), device=DEV)
    self.slots = [(self.comp, FILL)]
    self.put(a)

  def put(self, a):
    t = self.t
    for x, name in ((t.keys, 'keys'), (t.last_seen, 'last_seen'), (t.freq, 'freq'), (t.table, 'table'),
                    (self.comp, 'comp')):
      x.copy_(dev(a[name]))
    t.recount()

  def get(self):
    t = self.t
    return dict(keys=host(t.keys), last_seen=host(t.last_seen), freq=host(t.freq), table=host(t.table),
                comp=host(self.comp))


def export_of(exp):
  return dict(keys=host(exp.keys), src_slots=host(exp.src_slots),
              moves=[host(exp.rows), host(exp.last_seen), host(exp.freq)] + [host(x) for x in exp.slots])


@pytest.fixture(scope='module')
def tables():
  """kind -> (the arrays, a table for the LRU calls, an identically built one for the LFU calls)."""
  out = {}
  for kind in ('ages', 'counts'):
    a = arrays(kind)
    out[kind] = (a, Table(a), Table(a))
  return out


def run(table, a, what, max_size, keep_freq, order):
  """One call on the arrays `a`: (report or None, export or None, arrays after)."""
  table.put(a)
  report = export = None
  if what == 'select':
    report = host(hash_evict_to_select([table.t], [max_size], keep_freq, order=order)[0])
  elif what == 'evict_to':
    report = host(hash_evict_to([table.t], [max_size], keep_freq, [table.slots], order=order)[0])
  else:
    export = export_of(hash_spill([table.t], [max_size], keep_freq, [table.slots], order=order)[0])
  return report, export, table.get()


@pytest.mark.gpu
@pytest.mark.parametrize('keep_freq', KEEP_FREQS)
def test_lfu_over_one_freq_class_is_lru(tables, keep_freq):
  a, lru_table, lfu_table = tables['ages']
  n_evictable = 0 if keep_freq == 2 else N_LIVE
  for max_size in MAX_SIZES:
    want, _, want_after = ref_evict(tref, a, max_size, keep_freq)
    # the select: the reports, and nothing of either table written
    lru, _, lru_after = run(lru_table, a, 'select', max_size, keep_freq, 'lru')
    lfu, _, lfu_after = run(lfu_table, a, 'select', max_size, keep_freq, 'lfu')
    np.testing.assert_array_equal(lru, want)
    check_lfu_is_lru(lfu, lru, n_evictable)
    same_arrays(lru_after, a)
    same_arrays(lfu_after, a)
    # the eviction: the reports and every array
    lru, _, lru_after = run(lru_table, a, 'evict_to', max_size, keep_freq, 'lru')
    lfu, _, lfu_after = run(lfu_table, a, 'evict_to', max_size, keep_freq, 'lfu')
    np.testing.assert_array_equal(lru, want)
    check_lfu_is_lru(lfu, lru, n_evictable)
    same_arrays(lru_after, want_after)
    same_arrays(lfu_after, lru_after)
    assert host(lfu_table.t.stats).tolist() == host(lru_table.t.stats).tolist()
    # the spill: the exports field for field, and the tables it leaves
    _, lru_export, lru_after = run(lru_table, a, 'spill', max_size, keep_freq, 'lru')
    _, lfu_export, lfu_after = run(lfu_table, a, 'spill', max_size, keep_freq, 'lfu')
    want_export, _ = ref_spill(sref, a, want, keep_freq)
    same_export(lru_export, want_export)
    same_export(lfu_export, lru_export)
    same_arrays(lru_after, want_after)
    same_arrays(lfu_after, lru_after)
    assert lru_export['keys'].size == want[3]


@pytest.mark.gpu
@pytest.mark.parametrize('keep_freq', KEEP_FREQS)
def test_lfu_over_one_age_class_is_not_lru(tables, keep_freq):
  a, lru_table, lfu_table = tables['counts']
  n_evictable = int(tref.evictable_mask(a['keys'], a['freq'], keep_freq).sum())
  for max_size in MAX_SIZES:
    want, _, want_after = ref_evict(lref, a, max_size, keep_freq)
    lru_want, _, lru_want_after = ref_evict(tref, a, max_size, keep_freq)
    lfu, _, lfu_after = run(lfu_table, a, 'select', max_size, keep_freq, 'lfu')
    np.testing.assert_array_equal(lfu, want)
    same_arrays(lfu_after, a)
    lru, _, lru_after = run(lru_table, a, 'evict_to', max_size, keep_freq, 'lru')
    lfu, _, lfu_after = run(lfu_table, a, 'evict_to', max_size, keep_freq, 'lfu')
    np.testing.assert_array_equal(lru, lru_want)
    np.testing.assert_array_equal(lfu, want)
    same_arrays(lru_after, lru_want_after)
    same_arrays(lfu_after, want_after)
    assert lru[3] == (n_evictable if lru[1] > 0 else 0)                   # LRU: the one class whole, or nothing
    if max_size in (350, 699):
      assert 0 < lfu[4] < lru[3] and lfu[3] == 5                          # LFU cuts inside it
    _, lfu_export, lfu_after = run(lfu_table, a, 'spill', max_size, keep_freq, 'lfu')
    want_export, _ = ref_spill(lref, a, want, keep_freq)
    same_export(lfu_export, want_export)
    same_arrays(lfu_after, want_after)
