"""A model of one ``HashTable`` across its whole life, a checker that compares a table with it, and the seeded
generator of operation sequences that tests/test_gpu_hash_lifecycle.py (the device) and
tests/test_hash_lifecycle_model.py (a numpy device built from the sequential restatements) drive side by side.

The model knows no slot numbers: a dict ``key -> Record(row, last_seen, freq, companion rows)``, the sketch as an
array, and the counters.  Every operation is written from include/hbk.h and the docstrings of
hybridbackend_amd/embedding/hashtable.py, not from the kernels.

What the model may predict.  The device inserts concurrently, so the model predicts only what cannot depend on the
order in which the occurrences of a call are taken.  Two facts about an inserting launch carry the argument:

  (a) inside a launch a slot only goes from free to key (free = EMPTY, or TOMBSTONE on an expiring table); the sweep,
      the rehash and the sketch's aging are launches of their own, stream-ordered against it;
  (b) a walk that fails (-1 for an id that was sent to the find-or-insert) has read EVERY slab as full -- no EMPTY
      slot, and on an expiring table no TOMBSTONE on the way -- and by (a) a slab read as full stays full.

Let D be the distinct ids of a call that are not stored and that the call sends to the find-or-insert (all misses of
a table without a filter; of a filtered table the misses whose estimate after ALL of phase 1 reaches min_freq -- the
sketch after phase 1 is a sum, so it does not depend on order either), and F the free slots before the call.

  * D <= F (D == F included): no walk fails.  A failing walk of id k ends, by (b), with the table full and k not in
    it (k cannot be stored later: no free slot is left, and it was not stored before: the walk would have hit it).
    Full means F ids were stored by the call, all of them candidates other than k, so F <= D - 1: a contradiction.
    Hence every candidate is stored, once (the one-inserter argument of csrc/hash_insert.hip), and the key set, every
    counter but ``reused``, and every per-key value are exact.
  * F == 0: nothing can be stored; every candidate occurrence fails.  Exact as well.
  * 0 < F < D: some walk fails, so by (b) the table ends full: exactly F candidates are stored.  An id's occurrences
    all get one answer only when it is stored (they then share its slot); which F ids are stored is the device's
    choice.  ``Model.translate`` verifies these constraints on the answers and adopts the device's subset; n_failed
    is then the occurrences of the ids left out (plus the sentinels).  The generator lets this happen only on the
    one over-full table of a fleet.
  * ``reused`` (stats[1]) is never predicted: which of several free slots a key takes is order-dependent.  It is
    checked through an identity -- TOMBSTONE slots now == evicted since the last rehash / compact - reused since --
    and it may never decrease between two rebuilds.

Per-key values are order-free: a new row is a function of (key, seed, column); ``last_seen`` is the step of the call
for every id the call resolved; ``freq`` grows by the id's occurrences (an atomic add per occurrence; the ceiling of
2^30 is out of reach here).

The size bound, the host tier, export / import and the sequence translate are order-free as well: the selection
of ``evict_to`` / ``spill_to`` is a function of the per-key ``last_seen`` and ``freq``; an export is a function of the
table's arrays (its ``src_slots`` are not predicted, only checked against the key array); a ``fault_in`` and an
import go through the insert without the filter, so the D / F argument above holds for them with D = the distinct
keys not stored; a sequence translate is a translate of its effective id list.  ``Model.store`` is what the table's
``HashSpillStore`` holds.

Events (``Events``) are computed from the model and the geometry alone -- pigeonhole bounds where a layout fact is
wanted: more stored keys homing to one slab than it has slots means one of them overflowed; more new keys than the
table can still have EMPTY slots means a tombstone was reused.  The one exception is "an id found behind a
tombstone", which only a layout can tell: it is read off the key array of the side that is driven (the sequential
restatement in the model test).
"""
import ctypes as C

import numpy as np

from tests.support import hash_admission_ref as aref
from tests.support import hash_evict_to_ref as tref
from tests.support import hash_expiry_ref as xref
from tests.support import hash_export_ref as pref
from tests.support import hash_ref as ref
from tests.support import hash_rehash_ref as rref
from tests.support import hash_spill_ref as sref

EMPTY = ref.EMPTY
TOMBSTONE = EMPTY + 1
KINDS = ('plain', 'expiring', 'admit', 'expiring_admit')
SLAB_SIZES = (1, 5, 8, 16, 33, 64)
SLAB_COUNTS = (1, 3, 20, 257)
MAX_CAPACITY = 1300
INT32_MAX = tref.INT32_MAX
SEEDS = tuple(range(10))   # chosen so that the conditions of tests/test_hash_lifecycle_model.py hold
TIER_SEEDS = (11, 18, 21, 22, 26, 49, 54)   # the same, for the sequences that also draw the later operations;
# none of them is one of SEEDS: a seed fixes its fleet, so these put the later operations on seven further fleets
BASE_EVENTS = ('overflow', 'eviction', 'reused', 'behind_tombstone', 'exact_admission', 'early_admission', 'growth',
               'rehash_sheds_tombstones', 'fills_last_slot', 'empty_run')
# the size bound, the host tier, export / import and the sequence translate (drawn only by the TIER_SEEDS)
TIER_EVENTS = ('cut_inside_a_step', 'keep_freq_holds_the_bound', 'bound_already_met', 'spill', 'fault_in',
               'fault_in_onto_tombstone', 'respill', 'fresh_over_store', 'delta_is_a_proper_subset',
               'export_after_rehash', 'import_overwrites_stored', 'import_inserts', 'import_by_owner',
               'sequence_truncates', 'sequence_pads', 'sequence_on_tombstones')
EVENTS = BASE_EVENTS + TIER_EVENTS
_EXPIRING_EVENTS = ('eviction', 'reused', 'behind_tombstone', 'rehash_sheds_tombstones', 'cut_inside_a_step',
                    'keep_freq_holds_the_bound', 'bound_already_met', 'spill', 'fault_in', 'fault_in_onto_tombstone',
                    'respill', 'fresh_over_store', 'delta_is_a_proper_subset', 'sequence_on_tombstones',
                    'import_inserts')   # (no key ever leaves a table that does not expire: its snapshots hold nothing new)
_FILTER_EVENTS = ('exact_admission', 'early_admission')


def applies(event, kind):
  if event in _EXPIRING_EVENTS:
    return 'expiring' in kind
  if event in _FILTER_EVENTS:
    return 'admit' in kind
  return True


def host(x):
  """A numpy copy of a tensor or an array."""
  return np.array(x.cpu().numpy() if hasattr(x, 'cpu') else x)


def bits(a):
  """fp32 / int32 values as their 32-bit patterns: comparisons are bit for bit (-0.0 is not +0.0)."""
  return np.ascontiguousarray(a).view(np.uint32)


def keys_per_block(slab_size):
  """Keys one 256-thread block of the translate kernels takes: 8 per lane group of pow2(slab_size) lanes."""
  group_log2 = 0
  while (1 << group_log2) < slab_size:
    group_log2 += 1
  return (256 >> group_log2) * 8


def translate_runs(tables, runs, insert=True):
  """The runs entry (``hbk_hash_translate_runs_n``) on device tables of ONE kind: runs[c] = list of id tensors;
  returns the slot tensors in the same shape."""
  import torch
  from hybridbackend_amd import _lib
  n = len(tables)
  device = tables[0].keys.device if n else torch.device('cuda:0')
  kinds = {(t.expiring, bool(t.min_freq)) for t in tables}
  assert len(kinds) <= 1
  expiring, filtered = kinds.pop() if kinds else (False, False)
  cols = (_lib.HashColumn * max(n, 1))()
  exp = (_lib.HashExpiry * max(n, 1))() if expiring else None
  adm = (_lib.HashAdmission * max(n, 1))() if filtered else None
  keep, ptrs, slots = [], [], []
  for c, t in enumerate(tables):
    t._describe(cols[c], init=insert, count=bool(insert))
    cols[c].keys, cols[c].slots, cols[c].n_keys = None, None, -3          # ignored
    if expiring:
      t._describe_expiry(exp[c])
    if filtered:
      t._describe_admission(adm[c])
    r = (_lib.HashRun * max(len(runs[c]), 1))()
    out = [torch.full((i.numel(),), -7, dtype=torch.int64, device=device) for i in runs[c]]
    for k, (i, o) in enumerate(zip(runs[c], out)):
      r[k].keys, r[k].slots, r[k].n_keys = (i.data_ptr(), o.data_ptr(), i.numel()) if i.numel() else (None, None, 0)
    keep.append(r)
    ptrs.append(C.cast(r, C.c_void_p).value)
    slots.append(out)
  _lib.check(_lib.lib().hbk_hash_translate_runs_n(
    n, cols, exp, adm, _lib.i32_array([len(r) for r in runs]), _lib.ptr_array(ptrs), 1 if insert else 0,
    _lib.current_stream(device)))
  return slots


# ---- what a table is made from ------------------------------------------------------------------------------
class Spec:
  """The making of one table and the ids it is offered."""

  def __init__(self, kind, slab_size, slab_count, dim, comps=(), regime='roomy', pool=(), min_freq=2, depth=4,
               width=None, seed=0, sketch_seed=0, init_scale=0.05):
    self.kind, self.slab_size, self.slab_count, self.dim = kind, int(slab_size), int(slab_count), int(dim)
    self.comps = [(int(w), float(v)) for w, v in comps]   # (width, fill value)
    self.regime = regime
    self.pool = np.asarray(pool, np.int64)
    self.expiring, self.filtered = 'expiring' in kind, 'admit' in kind
    self.min_freq = int(min_freq) if self.filtered else 0
    self.depth, self.width = int(depth), int(width if width is not None else slab_size * slab_count)
    self.seed, self.sketch_seed, self.init_scale = int(seed), int(sketch_seed), float(init_scale)

  @property
  def capacity(self):
    return self.slab_size * self.slab_count


def written_rows(keys, op, width, salt=0):
  """The values a test writes into the rows of `keys` after operation `op`: a function of (key, op, column), exact
  in fp32 -- the stand-in for an optimizer step."""
  keys = np.asarray(keys, np.int64)
  base = (keys & 0xfff) * 3 + op * 17 + salt * 5
  return (((base[:, None] + np.arange(width, dtype=np.int64)[None, :]) % 4096).astype(np.float32) / np.float32(16) -
          np.float32(100))


class Record:
  __slots__ = ('row', 'last_seen', 'freq', 'comps')

  def __init__(self, row, last_seen, freq, comps):
    self.row, self.last_seen, self.freq, self.comps = row, last_seen, freq, comps

  def copy(self):
    return Record(np.array(self.row, np.float32), self.last_seen, self.freq,
                  [np.array(c, np.float32) for c in self.comps])


class Model:
  """One table, free of slot numbers (the module docstring says what it may predict)."""

  def __init__(self, spec):
    self.kind, self.expiring, self.min_freq = spec.kind, spec.expiring, spec.min_freq
    self.regime, self.pool = spec.regime, spec.pool
    self.dim, self.seed, self.init_scale = spec.dim, spec.seed, spec.init_scale
    self.slab_size, self.slab_count = spec.slab_size, spec.slab_count
    self.comp_specs = list(spec.comps)
    self.stored = {}
    self.sketch = np.zeros((spec.depth, spec.width), np.int32) if self.min_freq else None
    self.sketch_seed = spec.sketch_seed
    self.counts = [0, 0]          # inserted (moved, after a rehash) / occurrences refused
    self.evicted = 0              # stats[0]
    self.filtered = 0
    self.step = 0
    self.reused_seen = 0          # the device's stats[1] at the last check: never predicted, only bounded
    # bookkeeping of the events (bounds that hold for every order)
    self.nonempty_lb = 0          # slots that are certainly not EMPTY
    self.tomb_lb = 0              # tombstones the table certainly holds
    self.own = {}                 # id -> its own sightings the sketch carries
    # the host tier, the snapshots and what their events need
    self.store = {}               # key -> Record: what a HashSpillStore of this table holds (put is an upsert)
    self.returned = set()         # keys a fault_in brought back
    self.snapshots = []           # (version when taken, {key: Record}) per export, in order
    self.version = 0              # state-changing operations so far (kept by the Runner: `fingerprint`)
    self.rehashed = False         # a rehash or compact ran since the last export

  @property
  def capacity(self):
    return self.slab_size * self.slab_count

  def free(self):
    return self.capacity - len(self.stored)

  def sentinel_mask(self, ids):
    ids = np.asarray(ids, np.int64)
    return (ids == EMPTY) | (ids == TOMBSTONE) if self.expiring else ids == EMPTY

  def _new_record(self, key, row, freq):
    comps = [np.full(w, v, np.float32) for w, v in self.comp_specs]
    return Record(np.array(row, np.float32), self.step if self.expiring else 0, freq if self.expiring else 0, comps)

  def _candidates(self, uniq, cnt, sketch):
    """The distinct ids a call sends to the find-or-insert, with their occurrences; the occurrences the filter
    answers -1; `sketch` (None without a filter) is counted into."""
    resident = np.array([k in self.stored for k in uniq.tolist()], bool)
    miss, c = uniq[~resident], cnt[~resident]
    if sketch is None:
      return resident, miss, c, 0, None
    depth, width = sketch.shape
    at = aref.cells(miss, depth, width, self.sketch_seed)
    for r in range(depth):
      np.add.at(sketch[r], at[r], c.astype(np.int32))
    assert sketch.size == 0 or int(sketch.max()) < aref.CEILING   # the ceiling is out of reach of these sequences
    est = sketch[np.arange(depth)[:, None], at].min(axis=0) if miss.size else np.zeros(0, np.int32)
    admit = est >= self.min_freq
    return resident, miss[admit], c[admit], int(c[~admit].sum()), (miss, c, est, admit)

  def preview(self, ids):
    """(D, F, occurrences of the D candidates) of a translate with insert=True, changing nothing."""
    ids = np.asarray(ids, np.int64)
    uniq, cnt = np.unique(ids[~self.sentinel_mask(ids)], return_counts=True)
    sketch = None if self.sketch is None else self.sketch.copy()
    _, cand, occ, _, _ = self._candidates(uniq, cnt, sketch)
    return int(cand.size), self.free(), int(occ.sum())

  def translate(self, ids, slots=None):
    """One call with insert=True.  `slots`: the device's answers, read only when 0 < F < D (the subset is then
    the device's choice, verified here and adopted).  Returns (stored mask per occurrence, events, adopted)."""
    ids = np.asarray(ids, np.int64)
    sent = self.sentinel_mask(ids)
    uniq, cnt = np.unique(ids[~sent], return_counts=True)
    events = set()
    resident, cand, cand_cnt, n_filtered, filt = self._candidates(uniq, cnt, self.sketch)
    self.filtered += n_filtered
    if filt is not None:
      miss, c, est, admit = filt
      for k, n, e, a in zip(miss.tolist(), c.tolist(), est.tolist(), admit.tolist()):
        before = self.own.get(k, 0)
        self.own[k] = before + n
        if a and before + n < self.min_freq:
          events.add('early_admission')
        if a and before < self.min_freq and before + n == self.min_freq and e == before + n:
          events.add('exact_admission')
    D, F = int(cand.size), self.free()
    adopted = False
    if D <= F:
      chosen = np.ones(D, bool)
    elif F == 0:
      chosen = np.zeros(D, bool)
    else:
      assert slots is not None, 'the subset of an over-full call is the device\'s: its answers are needed'
      slots = np.asarray(slots, np.int64)
      chosen = np.zeros(D, bool)
      for n, k in enumerate(cand.tolist()):
        s = slots[ids == k]
        assert (s >= 0).all() or (s == -1).all(), f'occurrences of id {k} got different answers: {s.tolist()}'
        chosen[n] = s[0] >= 0
      assert int(chosen.sum()) == F, f'{D} candidates, {F} free slots: {int(chosen.sum())} were stored, not {F}'
      adopted = True
    if self.expiring:
      for k, n in zip(uniq[resident].tolist(), cnt[resident].tolist()):
        rec = self.stored[k]
        rec.last_seen, rec.freq = self.step, rec.freq + n
    new = cand[chosen]
    rows = ref.init_rows(new, self.dim, self.seed, self.init_scale)
    for k, n, row in zip(new.tolist(), cand_cnt[chosen].tolist(), rows):
      self.stored[k] = self._new_record(k, row, n)
    self.counts[0] += int(new.size)
    self.counts[1] += int(sent.sum()) + int(cand_cnt[~chosen].sum())
    # events, from bounds that hold whatever the order
    if new.size:
      homes = ref.murmur3_np(np.fromiter(self.stored, np.int64, len(self.stored))).astype(np.int64) % self.slab_count
      crowded = np.bincount(homes, minlength=self.slab_count) > self.slab_size
      if crowded[ref.murmur3_np(new).astype(np.int64) % self.slab_count].any():
        events.add('overflow')
      if self.expiring and new.size > self.capacity - self.nonempty_lb:
        events.add('reused')
      if D == F:
        events.add('fills_last_slot')
    self.nonempty_lb = max(self.nonempty_lb, len(self.stored))
    self.tomb_lb = max(0, self.tomb_lb - int(new.size))
    keys_now = self.stored
    stored = np.array([(not s) and (k in keys_now) for k, s in zip(ids.tolist(), sent.tolist())], bool)
    return stored, events, adopted

  def find(self, ids):
    """insert=False: the mask of the occurrences that are stored; nothing changes."""
    ids = np.asarray(ids, np.int64)
    sent = self.sentinel_mask(ids)
    return np.array([(not s) and (k in self.stored) for k, s in zip(ids.tolist(), sent.tolist())], bool)

  def set_step(self, n):
    self.step = int(n)

  def evict(self, steps_to_live, keep_freq):
    keys = np.fromiter(self.stored, np.int64, len(self.stored))
    seen = np.array([self.stored[k].last_seen for k in keys.tolist()], np.int32)
    freq = np.array([self.stored[k].freq for k in keys.tolist()], np.int32)
    mask = xref.evict_mask(keys, seen, freq, self.step, steps_to_live, keep_freq)
    for k in keys[mask].tolist():
      del self.stored[k]       # its metadata and companion rows go with it: the slot's are zeroed / filled
    self.returned -= set(keys[mask].tolist())
    n = int(mask.sum())
    self.evicted += n
    self.tomb_lb += n
    return n

  def fits(self, slab_size, slab_count):
    """Whether a rehash into this geometry is accepted: a table that does not shrink always is."""
    capacity = slab_size * slab_count
    return capacity >= self.capacity or len(self.stored) <= capacity

  def rehash(self, slab_size, slab_count):
    """counts[0] = keys moved, counts[1] kept, stats zeroed, no tombstone left; the sketch, filter_counts and
    every stored key's rows, metadata and companions unchanged."""
    assert self.fits(slab_size, slab_count)
    self.slab_size, self.slab_count = int(slab_size), int(slab_count)
    self.counts[0] = len(self.stored)
    self.evicted = self.reused_seen = 0
    self.nonempty_lb, self.tomb_lb = len(self.stored), 0
    self.rehashed = True

  def compact(self):
    """The host path: the same table in the same geometry, tombstones gone, stats reset, size() and failed() kept."""
    self.rehash(self.slab_size, self.slab_count)

  def load(self, keys, rows):
    """``load``: the keys go through the table's insert entry WITHOUT its filter and without row initialisation,
    then the rows are stored.  On an expiring table that entry is the expiring insert with insert != 0, so every
    key -- new or already stored -- gets last_seen = step and freq + 1.  Distinct keys that fit, no sentinel."""
    new = 0
    for k, row in zip(np.asarray(keys, np.int64).tolist(), np.asarray(rows, np.float32)):
      rec = self.stored.get(k)
      if rec is None:
        self.stored[k] = self._new_record(k, row, 1)
        new += 1
      else:
        rec.row = np.array(row, np.float32)
        if self.expiring:
          rec.last_seen, rec.freq = self.step, rec.freq + 1
    assert len(self.stored) <= self.capacity
    self.counts[0] += new
    self.nonempty_lb = max(self.nonempty_lb, len(self.stored))
    self.tomb_lb = max(0, self.tomb_lb - new)

  def age_filter(self):
    self.sketch >>= 1
    self.own = {k: v >> 1 for k, v in self.own.items()}   # (a cell is at least the halved own count)

  def clear_filter(self):
    self.sketch[:] = 0
    self.own = {}

  def write(self, keys, rows, comp_rows):
    for n, k in enumerate(np.asarray(keys, np.int64).tolist()):
      rec = self.stored[k]
      rec.row = np.array(rows[n], np.float32)
      rec.comps = [np.array(c[n], np.float32) for c in comp_rows]

  # ---- the size bound and the host tier ----------------------------------------------------------------------
  def select(self, max_size, keep_freq):
    """(report without its last word, the keys that leave) of ``evict_to`` / ``spill_to``: ``need = size() -
    max_size``; the cut is the need-th smallest last_seen among the keys seen fewer than keep_freq times (all of
    them with keep_freq 0), INT32_MAX when they are fewer than need; every such key at or below the cut leaves."""
    assert self.expiring
    live = len(self.stored)
    need = live - int(max_size)
    if need <= 0:
      return [live, need, 0], []
    able = [(rec.last_seen, k) for k, rec in self.stored.items() if keep_freq == 0 or rec.freq < keep_freq]
    cut = sorted(a for a, _ in able)[need - 1] if len(able) >= need else INT32_MAX
    return [live, need, cut], [k for a, k in able if a <= cut]

  def _bound_events(self, report, max_size):
    live, need, cut, n = report
    events = set()
    if need <= 0:
      events.add('bound_already_met')
    else:
      if live - n < max_size:
        events.add('cut_inside_a_step')
      if cut == INT32_MAX or live - n > max_size:
        events.add('keep_freq_holds_the_bound')
    return events

  def evict_to(self, max_size, keep_freq):
    """Returns (report {live_before, need, cut, n_evicted}, events); the bookkeeping is ``evict``'s."""
    head, leaving = self.select(max_size, keep_freq)
    for k in leaving:
      del self.stored[k]
    self.returned -= set(leaving)
    self.evicted += len(leaving)
    self.tomb_lb += len(leaving)
    report = head + [len(leaving)]
    return report, self._bound_events(report, max_size)

  def spill(self, max_size, keep_freq):
    """``evict_to`` whose keys leave with their records into the store.  Returns ({key: Record} of the export,
    events)."""
    head, leaving = self.select(max_size, keep_freq)
    events = self._bound_events(head + [len(leaving)], max_size)
    out = {}
    for k in leaving:
      out[k] = self.stored.pop(k)
      if k in self.returned:
        events.add('respill')
      if k in self.store:           # it came back fresh, by a translate, a load or an import: the store upserts
        events.add('fresh_over_store')
      self.store[k] = out[k].copy()
    self.returned -= set(leaving)
    self.evicted += len(leaving)
    self.tomb_lb += len(leaving)
    if leaving:
      events.add('spill')
    return out, events

  def wanted(self, ids):
    """The keys a ``fault_in(ids)`` asks the store for and gets: distinct, no sentinel, not stored, in the store."""
    ids = np.asarray(ids, np.int64)
    uniq = np.unique(ids[~self.sentinel_mask(ids)])
    return [k for k in uniq.tolist() if k not in self.stored and k in self.store]

  def fault_in(self, ids, now=None):
    """The wanted keys come back with their whole record and leave the store; nothing is stamped, the filter and
    the sketch are not touched.  With more of them than free slots the call raises after storing exactly F of
    them -- which F is the device's choice: `now`, the device's key array afterwards, is then read and the subset
    adopted; the others stay in the store and each counts as one failed occurrence.  Returns (keys restored,
    whether the call raises, events)."""
    want = self.wanted(ids)
    F = self.free()
    came = want
    if len(want) > F:
      assert now is not None, 'which keys of a fault_in that does not fit came in is the device\'s choice'
      held = set(np.asarray(now, np.int64).tolist())
      came = [k for k in want if k in held]
      assert len(came) == F, f'{len(want)} keys wanted, {F} free slots: {len(came)} came in, not {F}'
    events = set()
    for k in came:
      self.stored[k] = self.store.pop(k)
    self.returned |= set(came)
    self.counts[0] += len(came)
    self.counts[1] += len(want) - len(came)
    if came:
      events.add('fault_in')
      if len(came) > self.capacity - self.nonempty_lb:
        events.add('fault_in_onto_tombstone')
    self.nonempty_lb = max(self.nonempty_lb, len(self.stored))
    self.tomb_lb = max(0, self.tomb_lb - len(came))
    return len(came), len(want) > F, events

  # ---- export and import ---------------------------------------------------------------------------------
  def export(self, since=None):
    """{key: Record} of every key (since None), or of the keys with last_seen >= since (expiring kinds); the
    table does not change.  The snapshot is kept.  Returns (snapshot, events)."""
    assert since is None or self.expiring
    take = {k: r.copy() for k, r in self.stored.items() if since is None or r.last_seen >= since}
    events = set()
    if since is not None and 0 < len(take) < len(self.stored):
      events.add('delta_is_a_proper_subset')
    if self.rehashed and take:
      events.add('export_after_rehash')
    self.rehashed = False
    self.snapshots.append((self.version, take))
    return take, events

  def owned(self, keys, world, rank):
    keys = np.asarray(keys, np.int64)
    return np.ones(keys.size, bool) if world is None else np.mod(keys, world) == rank   # (numpy's % is a floormod)

  def import_(self, snapshot, world=None, rank=None, with_meta=True):
    """An upsert of {key: Record}: a stored key takes row and companions; on an expiring table last_seen and freq
    come from the snapshot with `with_meta`, else the key counts as seen now (last_seen = step; freq + 1, or 1
    when new).  A plain kind has no metadata.  Returns (the keys imported, events)."""
    keys = np.array(sorted(snapshot), np.int64)
    mine = keys[self.owned(keys, world, rank)]
    events = set()
    new = 0
    for k in mine.tolist():
      src, rec = snapshot[k], self.stored.get(k)
      if rec is None:
        rec = self.stored[k] = self._new_record(k, src.row, 1)
        new += 1
        events.add('import_inserts')
      else:
        events.add('import_overwrites_stored')
        rec.row = np.array(src.row, np.float32)
        if self.expiring:
          rec.last_seen, rec.freq = self.step, rec.freq + 1
      rec.comps = [np.array(c, np.float32) for c in src.comps]
      if self.expiring and with_meta:
        rec.last_seen, rec.freq = src.last_seen, src.freq
    assert len(self.stored) <= self.capacity
    if world is not None and 0 < mine.size < keys.size:
      events.add('import_by_owner')
    self.counts[0] += new
    self.nonempty_lb = max(self.nonempty_lb, len(self.stored))
    self.tomb_lb = max(0, self.tomb_lb - new)
    return mine, events

  def fingerprint(self):
    """Everything an export of the table could tell, and its geometry."""
    out = [np.array([self.slab_size, self.slab_count], np.int64).tobytes()]
    for k in sorted(self.stored):
      r = self.stored[k]
      out.append(np.array([k, r.last_seen, r.freq], np.int64).tobytes() + r.row.tobytes() +
                 b''.join(c.tobytes() for c in r.comps))
    return hash(b''.join(out))


def effective_ids(ids, row_splits, max_len, pad_id):
  """What a sequence translate looks up: per sample its first min(len, T) ids, then T - len pad ids when a pad id
  is given.  Returns (the ids, their positions b * T + t in the grid, lengths = min(len, T))."""
  ids = np.asarray(ids, np.int64)
  splits = np.arange(ids.size + 1) if row_splits is None else np.asarray(row_splits, np.int64)
  lens = np.minimum(np.diff(splits), max_len).astype(np.int64)
  out, at = [], []
  for b, (start, n) in enumerate(zip(splits[:-1].tolist(), lens.tolist())):
    out.append(ids[start:start + n])
    at.append(b * max_len + np.arange(n))
    if pad_id is not None and n < max_len:
      out.append(np.full(max_len - n, pad_id, np.int64))
      at.append(b * max_len + np.arange(n, max_len))
  cat = lambda x, t: np.concatenate(x).astype(t) if x else np.zeros(0, t)
  return cat(out, np.int64), cat(at, np.int64), lens.astype(np.int32)


# ---- the numpy device: the sequential restatements behind the attributes of a HashTable -----------------------
class NumpyTable:
  """A table held in numpy arrays and driven by the sequential restatements (hash_ref.fill,
  hash_expiry_ref.insert / evict, hash_admission_ref.translate, hash_rehash_ref's placement), behind the attribute
  and method names of ``HashTable`` that the checker reads.  `order`: None, or a RandomState that permutes the
  order in which every call's keys are taken."""

  def __init__(self, spec, order=None):
    self.slab_size, self.slab_count, self.capacity = spec.slab_size, spec.slab_count, spec.capacity
    self.dim, self.seed, self.init_scale = spec.dim, spec.seed, spec.init_scale
    self.expiring, self.min_freq, self.sketch_seed = spec.expiring, spec.min_freq, spec.sketch_seed
    self.keys = np.full(self.capacity, EMPTY, np.int64)
    self.table = np.zeros((self.capacity, self.dim), np.float32)
    self.counts = np.zeros(2, np.int32)
    self.last_seen = np.zeros(self.capacity, np.int32)   # (unused on a table that does not expire)
    self.freq = np.zeros(self.capacity, np.int32)
    self.stats = np.zeros(2, np.int32)
    self.step = 0
    if self.min_freq:
      self.sketch = np.zeros((spec.depth, spec.width), np.int32)
      self.filter_counts = np.zeros(1, np.int32)
    self.order = order

  def _perm(self, n):
    return np.arange(n) if self.order is None else self.order.permutation(n)

  def _live(self):
    return rref.live_mask(self.keys, self.expiring)

  def _insert(self, ids, admit=True, init=True):
    ids = np.asarray(ids, np.int64)
    perm = self._perm(ids.size)
    taken = ids[perm]
    before = self.keys.copy()
    if self.min_freq and admit:
      _, got, c = aref.translate(self.keys, self.slab_size, taken, self.sketch, self.min_freq, self.expiring,
                                 self.sketch_seed, self.last_seen, self.freq, self.step)
      self.counts += np.array([c['inserted'], c['failed']], np.int32)
      self.stats[1] += c['reused']
      self.filter_counts[0] += c['filtered']
    elif self.expiring:
      got, n_inserted, n_reused, n_failed = xref.insert(self.keys, self.slab_size, taken, self.last_seen, self.freq,
                                                        self.step)
      self.counts += np.array([n_inserted, n_failed], np.int32)
      self.stats[1] += n_reused
    else:
      got = ref.fill(self.keys, self.slab_size, taken)
      self.counts += np.array([int((self.keys != before).sum()), int((got < 0).sum())], np.int32)
    fresh = np.nonzero(self.keys != before)[0]
    if init and fresh.size:
      self.table[fresh] = ref.init_rows(self.keys[fresh], self.dim, self.seed, self.init_scale)
    slots = np.empty(ids.size, np.int64)
    slots[perm] = got
    return slots

  def lookup_or_insert(self, ids):
    return self._insert(ids)

  def find(self, ids):
    """The probe's walk for every id at once: its slot when no slab from its home slab up to the one it sits in
    has an EMPTY slot, else -1; never a sentinel of this table kind."""
    ids = np.asarray(ids, np.int64)
    out = np.full(ids.size, -1, np.int64)
    live = np.nonzero(self._live())[0]
    where = dict(zip(self.keys[live].tolist(), live.tolist()))
    at = np.array([where.get(k, -1) for k in ids.tolist()], np.int64)
    ok = at >= 0
    if ok.any():
      reach = reachable(self.keys, self.slab_size, ids[ok], at[ok])
      out[np.nonzero(ok)[0][reach]] = at[ok][reach]
    return out

  probe = find

  def size(self):
    return int(self.counts[0]) - (int(self.stats[0]) if self.expiring else 0)

  def failed(self):
    return int(self.counts[1])

  def evicted(self):
    return int(self.stats[0])

  def tombstones(self):
    return int((self.keys == TOMBSTONE).sum())

  def filtered(self):
    return int(self.filter_counts[0])

  def set_step(self, n):
    self.step = int(n)

  def evict(self, steps_to_live, keep_freq, companions):
    mask = xref.evict(self.keys, self.last_seen, self.freq, self.step, steps_to_live, keep_freq,
                      [(a, a.shape[1], v) for a, v in companions])
    self.stats[0] += int(mask.sum())

  def rehash(self, slab_size, slab_count, companions):
    """The live keys, in source order (or permuted), each into the first EMPTY slot of its hashed slab, else of
    the next; rows, metadata and companions moving along.  Returns the new companions, or None when refused."""
    capacity = slab_size * slab_count
    if capacity < self.capacity and self.size() > capacity:
      return None
    live = np.nonzero(self._live())[0]
    live = live[self._perm(live.size)]
    keys = np.full(capacity, EMPTY, np.int64)
    new = ref.fill(keys, slab_size, self.keys[live])
    assert (new >= 0).all()
    table = np.zeros((capacity, self.dim), np.float32)
    last_seen, freq = np.zeros(capacity, np.int32), np.zeros(capacity, np.int32)
    out = [np.full((capacity, a.shape[1]), v, np.float32) for a, v in companions]
    for src, dst in [(self.table, table), (self.last_seen, last_seen), (self.freq, freq)] + \
        [(a, o) for (a, _), o in zip(companions, out)]:
      dst[new] = src[live]
    self.keys, self.table, self.last_seen, self.freq = keys, table, last_seen, freq
    self.counts = np.array([live.size, self.counts[1]], np.int32)
    self.stats = np.zeros(2, np.int32)
    self.slab_size, self.slab_count, self.capacity = slab_size, slab_count, capacity
    return out

  def load(self, keys, rows):
    keys, rows = np.asarray(keys, np.int64), np.asarray(rows, np.float32)
    slots = self._insert(keys, admit=False, init=False)
    assert (slots >= 0).all()
    self.table[slots] = rows
    return slots

  def age_filter(self):
    self.sketch >>= 1

  def clear_filter(self):
    self.sketch[:] = 0

  def evict_to(self, max_size, keep_freq, companions):
    report, _ = tref.evict_to(self.keys, self.last_seen, self.freq, max_size, keep_freq,
                              [(a, a.shape[1], v) for a, v in companions])
    self.stats[0] += int(report[3])
    return report

  def spill(self, max_size, keep_freq, companions):
    """The select, then the spill of exactly the selected keys: the export, in ascending slot order."""
    selection = sref.select(self.keys, self.last_seen, self.freq, max_size, keep_freq)
    moves = [(self.table, self.dim), (self.last_seen, 1), (self.freq, 1)] + [(a, a.shape[1]) for a, _ in companions]
    exp, after, n_evicted, count = sref.spill(self.keys, self.last_seen, self.freq, selection, keep_freq, moves,
                                              [(a, a.shape[1], v) for a, v in companions], int(selection[3]))
    assert n_evicted == count == int(selection[3])
    self.keys[:], self.last_seen[:], self.freq[:] = after['cache'], after['last_seen'], after['freq']
    for (a, _), b in zip(companions, after['companions']):
      a[:] = b
    self.stats[0] += n_evicted
    return {'keys': exp['keys'], 'src_slots': exp['src_slots'], 'rows': exp['moves'][0], 'last_seen': exp['moves'][1],
            'freq': exp['moves'][2], 'comps': exp['moves'][3:]}

  def export(self, since, companions):
    arrays = [self.table] + ([self.last_seen, self.freq] if self.expiring else []) + [a for a, _ in companions]
    _, keys, slots, packed = pref.export(self.keys, self.expiring, arrays, self.last_seen,
                                         0 if since is None else max(int(since), 0))
    meta = packed[1:3] if self.expiring else [None, None]
    return {'keys': keys, 'src_slots': slots, 'rows': packed[0], 'last_seen': meta[0], 'freq': meta[1],
            'comps': packed[3:] if self.expiring else packed[1:]}

  def store_items(self, exp, companions, meta):
    """What ``import_items`` does with keys that passed its checks: the insert without the filter and without row
    initialisation, then the stores at the slots that were found.  Returns the slots."""
    slots = self._insert(exp['keys'], admit=False, init=False)
    ok = slots >= 0
    self.table[slots[ok]] = exp['rows'][ok]
    if meta and self.expiring:
      self.last_seen[slots[ok]], self.freq[slots[ok]] = exp['last_seen'][ok], exp['freq'][ok]
    for (a, _), rows in zip(companions, exp['comps']):
      a[slots[ok]] = rows[ok]
    return slots


def reachable(keys, slab_size, wanted, slots):
  """For keys `wanted` sitting in `slots` of the key array: whether no slab on the walk from the key's home slab
  up to (not including) the slab it sits in has an EMPTY slot -- what every reader's walk needs to arrive."""
  keys = np.asarray(keys, np.int64)
  slab_count = keys.size // slab_size
  has_empty = (keys.reshape(slab_count, slab_size) == EMPTY).any(axis=1)
  cum = np.concatenate([[0], np.cumsum(np.tile(has_empty, 2))])
  home = ref.murmur3_np(wanted).astype(np.int64) % slab_count
  dist = (np.asarray(slots, np.int64) // slab_size - home) % slab_count
  return cum[home + dist] - cum[home] == 0


def passes_tombstone(keys, slab_size, wanted, slots):
  """Whether the walk to each stored key meets a TOMBSTONE before the key: in a slab in front of its own, or in an
  earlier slot of its own slab."""
  keys = np.asarray(keys, np.int64)
  slab_count = keys.size // slab_size
  dead = keys == TOMBSTONE
  per_slab = dead.reshape(slab_count, slab_size).any(axis=1)
  cum = np.concatenate([[0], np.cumsum(np.tile(per_slab, 2))])
  slots = np.asarray(slots, np.int64)
  home = ref.murmur3_np(wanted).astype(np.int64) % slab_count
  dist = (slots // slab_size - home) % slab_count
  before = cum[home + dist] - cum[home] > 0
  inside = np.concatenate([[0], np.cumsum(dead)])
  return before | (inside[slots] - inside[slots // slab_size * slab_size] > 0)


# ---- the checker ------------------------------------------------------------------------------------------
def _state(table, companions):
  """Every array and counter of the table, read once."""
  s = {'keys': host(table.keys), 'table': host(table.table), 'counts': host(table.counts)}
  if table.expiring:
    s.update(last_seen=host(table.last_seen), freq=host(table.freq), stats=host(table.stats))
  if table.min_freq:
    s.update(sketch=host(table.sketch), filter_counts=host(table.filter_counts))
  for n, c in enumerate(companions):
    s[f'companion{n}'] = host(c)
  return s


def _like(table, a):
  """`a` where the table's arrays live."""
  if isinstance(table.keys, np.ndarray):
    return a
  import torch
  return torch.from_numpy(np.ascontiguousarray(a)).to(table.keys.device)


def _probe(table, ids):
  if hasattr(table, 'probe'):
    return table.probe(ids)
  from hybridbackend_amd.embedding import cache
  return host(cache.probe(table.keys, _like(table, ids), table.slab_size)[0])


def same_state(before, after, what):
  """Two readings of ``_state``: bit for bit the same."""
  assert before.keys() == after.keys()
  for name, a in before.items():
    np.testing.assert_array_equal(bits(a) if a.dtype == np.float32 else a,
                                  bits(after[name]) if a.dtype == np.float32 else after[name],
                                  err_msg=f'{what} changed {name}')


def export_arrays(exp):
  """A ``HashExport`` as a dict of numpy arrays."""
  return {'keys': host(exp.keys), 'src_slots': None if exp.src_slots is None else host(exp.src_slots),
          'rows': host(exp.rows), 'last_seen': None if exp.last_seen is None else host(exp.last_seen),
          'freq': None if exp.freq is None else host(exp.freq), 'comps': [host(x) for x in exp.slots]}


def as_export(arrays, device='cpu', meta=True, take=None):
  """The ``HashExport`` of such a dict (its rows `take`; without last_seen / freq when not `meta`)."""
  import torch
  from hybridbackend_amd.embedding.hashtable import HashExport

  def t(a):
    return torch.from_numpy(np.ascontiguousarray(a if take is None else a[take])).to(device)
  meta = meta and arrays['last_seen'] is not None
  return HashExport(t(arrays['keys']), t(arrays['rows']), t(arrays['last_seen']) if meta else None,
                    t(arrays['freq']) if meta else None, [t(c) for c in arrays['comps']])


def check_payload(model, got, want, what):
  """The arrays of an export (or of a store's ``peek``) against {key: Record}: the same key set, and per key the
  row, last_seen, freq and every companion row bit for bit."""
  keys = got['keys']
  assert keys.dtype == np.int64 and keys.ndim == 1
  assert np.unique(keys).size == keys.size, f'{what}: a key twice'
  np.testing.assert_array_equal(np.sort(keys), np.array(sorted(want), np.int64), err_msg=f'{what}: the keys')
  recs = [want[k] for k in keys.tolist()]
  assert got['rows'].dtype == np.float32 and got['rows'].shape == (keys.size, model.dim)
  np.testing.assert_array_equal(bits(got['rows']),
                                bits(np.array([r.row for r in recs], np.float32).reshape(keys.size, model.dim)),
                                err_msg=f'{what}: rows')
  if model.expiring:
    for name in ('last_seen', 'freq'):
      assert got[name].dtype == np.int32 and got[name].shape == (keys.size,)
      np.testing.assert_array_equal(got[name], np.array([getattr(r, name) for r in recs], np.int32),
                                    err_msg=f'{what}: {name}')
  else:
    assert got['last_seen'] is None and got['freq'] is None
  assert len(got['comps']) == len(model.comp_specs)
  for n, (w, _) in enumerate(model.comp_specs):
    assert got['comps'][n].dtype == np.float32 and got['comps'][n].shape == (keys.size, w)
    np.testing.assert_array_equal(bits(got['comps'][n]),
                                  bits(np.array([r.comps[n] for r in recs], np.float32).reshape(keys.size, w)),
                                  err_msg=f'{what}: companion {n}')


def check_export(model, got, want, keys_before, what):
  """An export or a spill: ``check_payload``, and src_slots -- not predicted, but strictly ascending, and the key
  array before the call held exactly these keys at these slots."""
  check_payload(model, got, want, what)
  src = got['src_slots']
  assert src.dtype == np.int64 and src.shape == got['keys'].shape
  assert (np.diff(src) > 0).all(), f'{what}: src_slots are not strictly ascending'
  assert src.size == 0 or (0 <= src[0] and src[-1] < keys_before.size)
  np.testing.assert_array_equal(keys_before[src], got['keys'], err_msg=f'{what}: the keys were not at src_slots')


def check_report(got, want, what):
  """{live_before, need, cut, n_evicted}, exactly."""
  got = np.asarray(got)
  assert got.dtype == np.int32 and got.shape == (4,)
  assert got.tolist() == list(want), f'{what}: the report is {got.tolist()}, not {list(want)}'


def check_store(store, model):
  """A ``HashSpillStore`` against ``Model.store``: the same keys, ascending, the payload bit for bit through
  ``peek`` -- and the peek changed nothing."""
  import torch
  assert model.expiring
  want = np.array(sorted(model.store), np.int64)
  before = {k: host(v) for k, v in store.variables('s').items()}
  assert len(store) == want.size, f'the store holds {len(store)} keys, the model\'s {want.size}'
  np.testing.assert_array_equal(host(store.keys()), want, err_msg='the store\'s keys')
  wanted = np.concatenate([want[::-1], want[:3]])   # (any order, duplicates: peek answers ascending, once each)
  got = export_arrays(store.peek(torch.from_numpy(wanted)))
  np.testing.assert_array_equal(got['keys'], want, err_msg='peek\'s keys')
  check_payload(model, got, model.store, 'the store')
  same_state(before, {k: host(v) for k, v in store.variables('s').items()}, 'a peek')


def check(table, model, companions, store=None):
  """The table (a ``HashTable`` or a ``NumpyTable``) and its companion arrays against the model: keys, reachability
  by every reader, per-key and per-free-slot values bit for bit, the counters and the sketch; that the finds it
  makes change nothing; and the table's ``HashSpillStore`` against the model's."""
  s = _state(table, companions)
  keys, ss, sc = s['keys'], table.slab_size, table.slab_count
  assert (ss, sc, keys.size) == (model.slab_size, model.slab_count, model.capacity)
  assert table.capacity == model.capacity
  live = rref.live_mask(keys, model.expiring)
  if not model.expiring:
    # INT64_MIN + 1 is an ordinary key here: it is there only as a key the model holds
    assert not (keys == TOMBSTONE).any() or TOMBSTONE in model.stored
  at = np.nonzero(live)[0]
  order = np.argsort(keys[at], kind='stable')
  got, slot_of = keys[at][order], at[order]
  want = np.array(sorted(model.stored), np.int64)
  assert (np.diff(got) != 0).all(), 'a key is stored twice'
  np.testing.assert_array_equal(got, want, err_msg='the stored keys are not the model\'s')
  # every reader's walk arrives
  assert reachable(keys, ss, want, slot_of).all(), 'a key sits behind a slab with an EMPTY slot'
  np.testing.assert_array_equal(host(table.find(_like(table, want))), slot_of)
  absent = model.pool[~model.sentinel_mask(model.pool) & (model.pool != TOMBSTONE)]
  absent = np.array([k for k in absent.tolist() if k not in model.stored][:64], np.int64)
  hit = _probe(table, np.concatenate([want, absent]))
  np.testing.assert_array_equal(hit[:want.size], slot_of)
  assert (hit[want.size:] == -1).all()
  assert (host(table.find(_like(table, absent))) == -1).all()
  # per key, bit for bit
  recs = [model.stored[k] for k in want.tolist()]
  rows = np.array([r.row for r in recs], np.float32).reshape(want.size, model.dim)
  np.testing.assert_array_equal(bits(s['table'][slot_of]), bits(rows), err_msg='rows')
  free = ~live
  if model.expiring:
    np.testing.assert_array_equal(s['last_seen'][slot_of], np.array([r.last_seen for r in recs], np.int32),
                                  err_msg='last_seen')
    np.testing.assert_array_equal(s['freq'][slot_of], np.array([r.freq for r in recs], np.int32), err_msg='freq')
    assert not s['last_seen'][free].any() and not s['freq'][free].any(), 'metadata in a slot without a key'
  for n, (w, value) in enumerate(model.comp_specs):
    c = s[f'companion{n}']
    assert c.shape == (model.capacity, w)
    held = np.array([r.comps[n] for r in recs], np.float32).reshape(want.size, w)
    np.testing.assert_array_equal(bits(c[slot_of]), bits(held), err_msg=f'companion {n}')
    # a slot without a key: never used (made with the fill value), evicted (filled by the sweep) or left free
    # by a compact / rehash (filled by it)
    np.testing.assert_array_equal(bits(c[free]), bits(np.full((int(free.sum()), w), value, np.float32)),
                                  err_msg=f'companion {n} of the slots without a key')
  # scalars
  assert s['counts'].tolist() == model.counts, (s['counts'].tolist(), model.counts)
  assert table.size() == len(model.stored) and table.failed() == model.counts[1]
  if model.expiring:
    evicted, reused = s['stats'].tolist()
    assert evicted == model.evicted
    assert reused >= model.reused_seen, 'reused went down'
    assert int((keys == TOMBSTONE).sum()) == model.evicted - reused, 'tombstones != evicted - reused'
    model.reused_seen = reused
    assert table.evicted() == model.evicted and table.tombstones() == model.evicted - reused
  if model.min_freq:
    np.testing.assert_array_equal(s['sketch'], model.sketch)
    assert s['filter_counts'].tolist() == [model.filtered]
    assert table.filtered() == model.filtered
  # the finds above changed nothing
  same_state(s, _state(table, companions), 'a find')
  if store is not None:
    check_store(store, model)
  return s


def check_slots(ids, slots, stored, keys):
  """The answers of one translate: >= 0 exactly where the model says the id is stored, the slot holds the id,
  occurrences of one id share it, everything else is -1 (no provisional -2 escapes)."""
  ids, slots = np.asarray(ids, np.int64), np.asarray(slots, np.int64)
  assert slots.shape == ids.shape
  np.testing.assert_array_equal(slots >= 0, stored)
  assert (slots[~stored] == -1).all(), sorted(set(slots[~stored].tolist()))
  assert (slots[stored] < keys.size).all()
  np.testing.assert_array_equal(keys[slots[stored]], ids[stored])
  # (equal ids answered by slots that hold the id, in an array without duplicates, share the slot)


# ---- fleets: the two sides behind one set of operations ---------------------------------------------------------
def make_stores(specs, pin_memory):
  """One real ``HashSpillStore`` per expiring table, None for the others."""
  from hybridbackend_amd.embedding.hashtable import HashSpillStore
  return [HashSpillStore(s.dim, [w for w, _ in s.comps], pin_memory=pin_memory) if s.expiring else None
          for s in specs]


class NumpyFleet:
  def __init__(self, specs, order=None):
    self.tables = [NumpyTable(s, order) for s in specs]
    self.comps = [[np.full((s.capacity, w), v, np.float32) for w, v in s.comps] for s in specs]
    self.fills = [[v for _, v in s.comps] for s in specs]
    self.stores = make_stores(specs, pin_memory=False)

  def pairs(self, i):
    return list(zip(self.comps[i], self.fills[i]))

  def keys(self, i):
    return self.tables[i].keys.copy()

  def translate(self, idx, ids, insert, route, cuts):   # (a restatement has no runs: an id's occurrences are one call's)
    return [self.tables[i]._insert(x) if insert else self.tables[i].find(x) for i, x in zip(idx, ids)]

  def set_step(self, i, n):
    self.tables[i].set_step(n)

  def evict(self, idx, steps_to_live, keep_freq):
    for i in idx:
      self.tables[i].evict(steps_to_live, keep_freq, self.pairs(i))

  def rehash(self, idx, geometry):
    if any(self.tables[i].size() > ss * sc and ss * sc < self.tables[i].capacity for i, (ss, sc) in zip(idx, geometry)):
      return False   # refused before anything changes
    for i, (ss, sc) in zip(idx, geometry):
      self.comps[i] = self.tables[i].rehash(ss, sc, self.pairs(i))
    return True

  def compact(self, i):
    t = self.tables[i]
    self.comps[i] = t.rehash(t.slab_size, t.slab_count, self.pairs(i))

  def load(self, i, keys, rows):
    self.tables[i].load(keys, rows)

  def age_filter(self, i):
    self.tables[i].age_filter()

  def clear_filter(self, i):
    self.tables[i].clear_filter()

  def write(self, i, slots, rows, comp_rows):
    self.tables[i].table[slots] = rows
    for c, r in zip(self.comps[i], comp_rows):
      c[slots] = r

  def evict_to(self, idx, max_sizes, keep_freq):
    return [self.tables[i].evict_to(m, keep_freq, self.pairs(i)) for i, m in zip(idx, max_sizes)]

  def spill(self, idx, max_sizes, keep_freq):
    out = []
    for i, m in zip(idx, max_sizes):
      exp = self.tables[i].spill(m, keep_freq, self.pairs(i))
      if exp['keys'].size:
        self.stores[i].put(as_export(exp))
      out.append(exp)
    return out

  def fault_in(self, i, ids):
    """``HashTable.fault_in`` restated: a find, the distinct misses, ``store.take``, the import; what did not fit
    goes back into the store.  Returns (keys restored, whether the call raises)."""
    import torch
    t, store = self.tables[i], self.stores[i]
    ids = np.asarray(ids, np.int64)
    missed = np.unique(ids[t.find(ids) < 0])
    if missed.size == 0 or len(store) == 0:
      return 0, False
    exp = export_arrays(store.take(torch.from_numpy(missed)))
    if exp['keys'].size == 0:
      return 0, False
    slots = t.store_items(exp, self.pairs(i), meta=True)
    lost = np.nonzero(slots < 0)[0]
    if lost.size:
      store.put(as_export(exp, take=lost))
      return None, True
    return int(exp['keys'].size), False

  def export(self, idx, sinces):
    return [self.tables[i].export(since, self.pairs(i)) for i, since in zip(idx, sinces)]

  def import_(self, i, exp, take, world, rank, with_meta):
    exp = {k: (None if v is None else [c[take] for c in v] if k == 'comps' else v[take]) for k, v in exp.items()}
    mine = np.ones(exp['keys'].size, bool) if world is None else np.mod(exp['keys'], world) == rank
    exp = {k: (None if v is None else [c[mine] for c in v] if k == 'comps' else v[mine]) for k, v in exp.items()}
    slots = self.tables[i].store_items(exp, self.pairs(i), meta=with_meta)
    assert (slots >= 0).all()
    return slots

  def translate_sequence(self, idx, ids, row_splits, max_lens, pad_ids, insert):
    """Through the effective id list: (grids, lengths)."""
    grids, lengths = [], []
    for i, x, s, T, pad in zip(idx, ids, row_splits, max_lens, pad_ids):
      eff, at, lens = effective_ids(x, s, T, pad)
      grid = np.full(lens.size * T, -1, np.int64)
      grid[at] = self.tables[i]._insert(eff) if insert else self.tables[i].find(eff)
      grids.append(grid)
      lengths.append(lens)
    return grids, lengths


class DeviceFleet:
  """``HashTable``s on the GPU; fleet-wide calls go through hash_translate (or the runs entry) / hash_evict /
  hash_rehash / hash_evict_to / hash_spill / hash_export / hash_translate_sequence, several tables of mixed kinds
  per call; fault_in and import_items are per-table entries and are called per table."""

  def __init__(self, specs, device='cuda:0'):
    import torch
    from hybridbackend_amd.embedding import HashTable
    self.torch, self.device = torch, device
    self.tables = [HashTable(s.capacity, s.dim, device, slab_size=s.slab_size, init_scale=s.init_scale, seed=s.seed,
                             expiring=s.expiring, min_freq=s.min_freq, sketch_depth=s.depth, sketch_width=s.width,
                             sketch_seed=s.sketch_seed) for s in specs]
    self.comps = [[torch.full((s.capacity, w), v, dtype=torch.float32, device=device) for w, v in s.comps]
                  for s in specs]
    self.fills = [[v for _, v in s.comps] for s in specs]
    self.stores = make_stores(specs, pin_memory=True)

  def dev(self, a):
    return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

  def pairs(self, i):
    return list(zip(self.comps[i], self.fills[i]))

  def keys(self, i):
    return host(self.tables[i].keys)

  def translate(self, idx, ids, insert, route, cuts):
    from hybridbackend_amd.embedding import hashtable as ht
    tables = [self.tables[i] for i in idx]
    if route == 'plain':
      return [host(s) for s in ht.hash_translate(tables, [self.dev(x) for x in ids], insert=insert)]
    out = [None] * len(idx)
    kinds = {}
    for n, t in enumerate(tables):
      kinds.setdefault((t.expiring, bool(t.min_freq)), []).append(n)
    for members in kinds.values():   # the runs entry takes tables of one kind
      runs = [[self.dev(r) for r in np.split(ids[n], cuts[n])] for n in members]
      got = translate_runs([tables[n] for n in members], runs, insert=insert)
      for n, g in zip(members, got):
        out[n] = np.concatenate([host(x) for x in g]) if g else np.zeros(0, np.int64)
    return out

  def set_step(self, i, n):
    self.tables[i].set_step(n)

  def evict(self, idx, steps_to_live, keep_freq):
    from hybridbackend_amd.embedding import hashtable as ht
    ht.hash_evict([self.tables[i] for i in idx], steps_to_live, keep_freq, [self.pairs(i) for i in idx])

  def rehash(self, idx, geometry):
    from hybridbackend_amd import _lib
    from hybridbackend_amd.embedding import hashtable as ht
    try:
      new = ht.hash_rehash([self.tables[i] for i in idx], [ss * sc for ss, sc in geometry],
                           [ss for ss, _ in geometry], [self.pairs(i) for i in idx])
    except _lib.InvalidArgumentError:
      return False
    for i, comps in zip(idx, new):
      self.comps[i] = comps
    return True

  def compact(self, i):
    self.tables[i].compact(self.pairs(i))

  def load(self, i, keys, rows):
    self.tables[i].load(self.dev(keys), self.dev(rows))

  def age_filter(self, i):
    self.tables[i].age_filter()

  def clear_filter(self, i):
    self.tables[i].clear_filter()

  def write(self, i, slots, rows, comp_rows):
    at = self.dev(slots)
    self.tables[i].table[at] = self.dev(rows)
    for c, r in zip(self.comps[i], comp_rows):
      c[at] = self.dev(r)

  def evict_to(self, idx, max_sizes, keep_freq):
    from hybridbackend_amd.embedding import hashtable as ht
    reports = ht.hash_evict_to([self.tables[i] for i in idx], list(max_sizes), keep_freq, [self.pairs(i) for i in idx])
    return [host(r) for r in reports]

  def spill(self, idx, max_sizes, keep_freq):
    from hybridbackend_amd.embedding import hashtable as ht
    exps = ht.hash_spill([self.tables[i] for i in idx], list(max_sizes), keep_freq, [self.pairs(i) for i in idx])
    for i, exp in zip(idx, exps):
      if len(exp):
        self.stores[i].put(exp)
    return [export_arrays(e) for e in exps]

  def fault_in(self, i, ids):
    from hybridbackend_amd import _lib
    try:
      return self.tables[i].fault_in(self.dev(ids), self.stores[i], self.comps[i]), False
    except _lib.InvalidArgumentError as e:
      if 'do not fit' not in str(e):   # (any other refusal is not the one a full table earns)
        raise
      return None, True

  def export(self, idx, sinces):
    from hybridbackend_amd.embedding import hashtable as ht
    exps = ht.hash_export([self.tables[i] for i in idx], list(sinces), [self.comps[i] for i in idx])
    return [export_arrays(e) for e in exps]

  def import_(self, i, exp, take, world, rank, with_meta):
    got = self.tables[i].import_items(as_export(exp, self.device, with_meta, take), self.comps[i], world, rank)
    return host(got)

  def translate_sequence(self, idx, ids, row_splits, max_lens, pad_ids, insert):
    from hybridbackend_amd.embedding import hash_sequence as hs
    splits = [None if s is None else self.dev(np.asarray(s, np.int32)) for s in row_splits]
    grids, lengths = hs.hash_translate_sequence([self.tables[i] for i in idx], [self.dev(x) for x in ids], splits,
                                                list(max_lens), list(pad_ids), insert=insert)
    return [host(g) for g in grids], [host(n) for n in lengths]


# ---- the generator ------------------------------------------------------------------------------------------
def _geometries():
  return [(ss, sc) for ss in SLAB_SIZES for sc in SLAB_COUNTS if 5 <= ss * sc <= MAX_CAPACITY]


def make_pool(rng, n, expiring):
  """n ids that can be keys -- negative ones, pairs that differ only in the high word, small ones; on a table that
  does not expire INT64_MIN + 1 among them -- and the sentinels behind them."""
  out = set()
  if not expiring:
    out.add(TOMBSTONE)
  for k in (0, -1, 2 ** 63 - 1, 7, 7 + (1 << 32), 7 + (5 << 32), -7, -7 - (1 << 32))[:max(n - len(out), 0)]:
    out.add(k)
  while len(out) < n:
    k = int(rng.randint(-2 ** 62, 2 ** 62, dtype=np.int64))
    out.add(k)
    if len(out) < n and rng.rand() < 0.2:
      out.add(k ^ (int(rng.randint(1, 1 << 20)) << 32))   # the same low word
  keys = np.array(sorted(out), np.int64)
  rng.shuffle(keys)
  sentinels = [EMPTY, TOMBSTONE] if expiring else [EMPTY]
  return np.concatenate([keys, np.array(sentinels, np.int64)])


def make_fleet(rng):
  """4-6 specs: every kind, one table of one slab, one of one-slot slabs, at most one over-full."""
  n = int(rng.randint(4, 7))
  kinds = list(KINDS) + [KINDS[int(rng.randint(4))] for _ in range(n - 4)]
  rng.shuffle(kinds)
  geo = _geometries()
  over = int(rng.randint(n)) if rng.rand() < 0.8 else -1
  specs = []
  for c, kind in enumerate(kinds):
    regime = 'over' if c == over else ('tight' if rng.rand() < 0.5 else 'roomy')
    if regime == 'roomy' and c == 0:
      choice = [g for g in geo if g[1] == 1]
    elif regime == 'roomy' and c == 1:
      choice = [g for g in geo if g[0] == 1]
    elif regime == 'tight':
      choice = [g for g in geo if g[1] in (3, 20)]
    elif regime == 'over':
      choice = [g for g in geo if g[1] <= 20]
    else:
      choice = geo
    ss, sc = choice[int(rng.randint(len(choice)))]
    capacity = ss * sc
    expiring = 'expiring' in kind
    if regime == 'roomy':
      n_pool = max(1, int(capacity * rng.uniform(0.2, 0.5)))
    elif regime == 'tight':
      n_pool = max(1, int(round(capacity * (0.9 if rng.rand() < 0.4 else 1.0))))
    else:
      n_pool = capacity + 3 + int(capacity * rng.uniform(0.1, 0.4))
    comps = [((1, 4, 8)[int(rng.randint(3))], (0.0, 0.1, -2.5)[int(rng.randint(3))]) for _ in range(int(rng.randint(3)))]
    specs.append(Spec(kind, ss, sc, (1, 4, 19, 20)[int(rng.randint(4))], comps, regime,
                      make_pool(rng, n_pool, expiring), min_freq=(1, 2, 3)[int(rng.randint(3))],
                      depth=(1, 4)[int(rng.randint(2))], width=(1, 7, capacity)[int(rng.randint(3))],
                      seed=int(rng.randint(100)), sketch_seed=int(rng.randint(-50, 50))))
  # the two geometries every fleet has
  if not any(s.slab_count == 1 for s in specs):
    s = specs[0]
    specs[0] = Spec(s.kind, 5, 1, s.dim, s.comps, 'roomy', make_pool(rng, 2, s.expiring), s.min_freq, s.depth, 5, s.seed,
                    s.sketch_seed)
  if not any(s.slab_size == 1 for s in specs):
    s = specs[1]
    specs[1] = Spec(s.kind, 1, 20, s.dim, s.comps, 'roomy', make_pool(rng, 9, s.expiring), s.min_freq, s.depth, 7, s.seed,
                    s.sketch_seed)
  return specs


class Generator:
  """The next operation of a sequence, drawn from `rng` and the models' state (never from a device)."""

  def __init__(self, rng, specs, n_ops=40, tier=False):
    self.rng, self.specs, self.n_ops = rng, specs, n_ops
    self.tier, self.pending = tier, []   # tier: also draw the operations of ``tier_op``
    self.many_runs_at = int(rng.randint(n_ops // 4, n_ops))
    self.expiring = [c for c, s in enumerate(specs) if s.expiring]
    self.filtered = [c for c, s in enumerate(specs) if s.filtered]

  def subset(self, of):
    of = list(of)
    if len(of) <= 1 or self.rng.rand() < 0.4:
      return of
    k = int(self.rng.randint(1, len(of) + 1))
    return sorted(self.rng.choice(of, size=k, replace=False).tolist())

  def draw_ids(self, model, n):
    rng, pool = self.rng, model.pool
    if n == 0:
      return np.zeros(0, np.int64)
    if rng.rand() < 0.6:   # skewed: many duplicates of a few ids
      p = 1.0 / (1.0 + rng.permutation(pool.size))
      return pool[rng.choice(pool.size, size=n, p=p / p.sum())]
    return pool[rng.randint(0, pool.size, size=n)]

  def to_drop(self, model, ids):
    """Outside the over-full table no call may offer more new ids than there are free slots (0 < F < D is the
    device's choice): candidates are named until D <= F.  And a call that must fail walks every slab per failing
    occurrence: those are kept to a number the sequential restatement gets through quickly.  Decided by the model
    alone.  None: the ids may stay as they are."""
    D, F, occurrences = model.preview(ids)
    absent = [k for k in np.unique(ids).tolist() if k not in model.stored and not model.sentinel_mask([k])[0]]
    if model.regime != 'over' and 0 < F < D:
      return absent[:max(1, D - F)]
    if D > F and occurrences * model.slab_count > 20000:
      return absent[:len(absent) // 2 + 1]
    return None

  def fit(self, model, ids):
    """The ids without the occurrences of what ``to_drop`` names, until it names nothing."""
    while True:
      drop = self.to_drop(model, ids)
      if drop is None:
        return ids
      ids = ids[~np.isin(ids, drop)]

  def cuts(self, n):
    """1-4 runs at random places, empty runs among them."""
    return sorted(self.rng.randint(0, n + 1, size=int(self.rng.randint(0, 4))).tolist())

  def translate(self, models, idx, insert=True):
    rng = self.rng
    ids = []
    for i in idx:
      K = keys_per_block(models[i].slab_size)
      n = (0, 1, 7, K - 1, K, K + 1, 3 * K + 5)[int(rng.randint(7))]
      x = self.draw_ids(models[i], n)
      ids.append(self.fit(models[i], x) if insert else x)
    route = 'runs' if rng.rand() < 0.5 else 'plain'
    return {'op': 'translate', 'tables': idx, 'ids': ids, 'insert': insert, 'route': route,
            'cuts': [self.cuts(x.size) for x in ids], 'write': bool(rng.rand() < 0.6)}

  def fill_exactly(self, models, only=None):
    """A call that offers one table exactly as many new ids as it has free slots, each often enough to pass its
    filter, among resident ids."""
    rng = self.rng
    order = rng.permutation(len(models)).tolist() if only is None else only
    for i in order:
      m = models[i]
      absent = [k for k in m.pool.tolist() if k not in m.stored and not m.sentinel_mask([k])[0]]
      F = m.free()
      if 0 < F <= len(absent):
        new = np.array(absent[:F], np.int64)
        ids = np.concatenate([np.repeat(new, max(m.min_freq, 1)), self.draw_ids(m, 7)])
        ids = ids[np.isin(ids, new) | np.array([k in m.stored for k in ids.tolist()], bool) | m.sentinel_mask(ids)]
        rng.shuffle(ids)
        if m.preview(ids)[:2] == (F, F):
          return {'op': 'translate', 'tables': [i], 'ids': [ids], 'insert': True,
                  'route': 'runs' if rng.rand() < 0.5 else 'plain', 'cuts': [self.cuts(ids.size)], 'write': True}
    return self.translate(models, self.subset(range(len(models)))) if only is None else None

  def many_runs(self, models):
    """More than 64 non-empty runs for one table: 65 runs of 1-3 ids, the second ballot of the run search."""
    rng = self.rng
    i = int(rng.randint(len(models)))
    sizes = rng.randint(1, 4, size=65)
    ids = self.draw_ids(models[i], int(sizes.sum()))
    kept = self.fit(models[i], ids)
    if kept.size != ids.size:   # (new ids had to go: the runs keep their sizes, filled from what the table holds)
      allowed = np.array(sorted(models[i].stored) + [EMPTY], np.int64)
      ids = allowed[rng.randint(0, allowed.size, size=ids.size)]
    return {'op': 'translate', 'tables': [i], 'ids': [ids], 'insert': True, 'route': 'runs',
            'cuts': [np.cumsum(sizes)[:-1].tolist()], 'write': True}

  def rehash(self, models):
    rng = self.rng
    idx = self.subset(range(len(models)))
    geometry = []
    for i in idx:
      m = models[i]
      mode = ('same', 'x2', 'x1.5', 'slab', 'fit')[int(rng.randint(5))]
      if m.tomb_lb > 0 and rng.rand() < 0.5:
        mode = 'same'
      ss, sc, size = m.slab_size, m.slab_count, len(m.stored)
      if mode == 'x2' and 2 * m.capacity <= 2 * MAX_CAPACITY:
        sc = 2 * sc
      elif mode == 'x1.5' and m.capacity * 1.5 <= 2 * MAX_CAPACITY and int(m.capacity * 1.5) // ss > sc:
        sc = int(np.ceil(m.capacity * 1.5)) // ss
      elif mode == 'slab':
        other = [s for s in SLAB_SIZES if s != ss and m.capacity // s >= 1 and m.capacity // s * s >= size]
        if other:
          ss = other[int(rng.randint(len(other)))]
          sc = m.capacity // ss
      elif mode == 'fit':
        sc = max(1, -(-size // ss))
      geometry.append((ss, sc))
    return {'op': 'rehash', 'tables': idx, 'geometry': geometry}

  def refused_shrink(self, models):
    for i in self.rng.permutation(len(models)).tolist():
      m = models[i]
      sc = -(-len(m.stored) // m.slab_size) - 1
      if sc >= 1:
        return {'op': 'rehash', 'tables': [i], 'geometry': [(m.slab_size, sc)], 'refused': True}
    return None

  # ---- the size bound, the host tier, export / import, the sequence translate (tier=True only) ---------------
  def draw_bound(self, m, keep):
    """A max_size around the live size: 0, one below it, inside a last_seen group, at a group boundary, above it."""
    rng, live = self.rng, len(m.stored)
    ages = [r.last_seen for r in m.stored.values() if keep == 0 or r.freq < keep]
    mode = int(rng.randint(5))
    if mode == 0:
      return 0
    if mode == 1:
      return max(live - 1, 0)
    if mode == 4 or not ages:
      return live + int(rng.randint(0, 3))
    _, counts = np.unique(ages, return_counts=True)
    upto = np.cumsum(counts)
    wide = np.nonzero(counts > 1)[0]
    if mode == 2 and wide.size:
      g = int(wide[rng.randint(wide.size)])
      return live - (int(upto[g] - counts[g]) + int(rng.randint(1, counts[g])))
    return live - int(upto[rng.randint(upto.size)])

  def fill_spill_return(self, models):
    """An expiring table is filled to its last slot, spilled without a rehash, and asked for everything its store
    holds: the keys come back onto tombstones, in front of and behind what stayed."""
    order = self.rng.permutation(self.expiring).tolist()
    op = self.fill_exactly(models, [i for i in order if models[i].regime != 'over'])
    if op is not None:
      i = op['tables'][0]
      self.pending.append(lambda models: self.bound(models, [i], again=False, rehash=False, spill=True))
      self.pending.append(lambda models: self.fault_in(models, i, everything=True))
    return op

  def bound(self, models, idx=None, again=True, rehash=None, spill=None):
    """A spill or an evict_to; about half of the time the same-capacity rehash of ``maybe_evict`` follows, else
    the tombstones stay for what comes next: often a fault_in, a translate or a sequence translate of one of the
    tables, and then sometimes a second spill (of keys that came back, or came back fresh over the store)."""
    rng = self.rng
    if idx is None:
      idx = self.subset([i for i in self.expiring if models[i].stored] or self.expiring)
    keep = (0, 2)[int(rng.randint(2))]
    op = {'op': 'spill' if (rng.rand() < 0.65 if spill is None else spill) else 'evict_to', 'tables': idx,
          'keep': keep, 'max_sizes': [self.draw_bound(models[i], keep) for i in idx]}
    if rng.rand() < 0.5 if rehash is None else rehash:
      self.pending.append(lambda models: {'op': 'rehash', 'tables': idx,
                                          'geometry': [(models[i].slab_size, models[i].slab_count) for i in idx]})
    if again and rng.rand() < 0.7:
      i = idx[int(rng.randint(len(idx)))]
      r = rng.rand()
      if r < 0.4:
        self.pending.append(lambda models: self.fault_in(models, i))
      elif r < 0.6:
        self.pending.append(lambda models: self.translate(models, [i]))
      elif r < 0.75:
        self.pending.append(lambda models: self.translate_sequence(models, [i]))
      else:   # (a snapshot from before the bound brings back what has just left)
        self.pending.append(lambda models: self.import_(models, i))
      if rng.rand() < 0.6:
        self.pending.append(lambda models: self.bound(models, [i], again=False))
    return op

  def fault_in(self, models, i=None, everything=False):
    """Ids of one table: some of what its store holds or all of it (some twice), ids of the pool, the sentinels
    that come with them; stored keys are dropped until the rest fits."""
    rng = self.rng
    if i is None:
      having = [i for i in self.expiring if models[i].store]
      if not having:
        return None
      i = having[int(rng.randint(len(having)))]
    m = models[i]
    if not m.store:
      return None
    held = np.array(sorted(m.store), np.int64)
    n = held.size if everything or rng.rand() < 0.5 else int(rng.randint(1, held.size + 1))
    some = held[rng.permutation(held.size)[:n]]
    ids = np.concatenate([some, some[:int(rng.randint(0, some.size + 1))], self.draw_ids(m, int(rng.randint(0, 9)))])
    rng.shuffle(ids)
    ids = ids[~np.isin(ids, m.wanted(ids)[m.free():])]
    return {'op': 'fault_in', 'table': i, 'ids': ids}

  def export(self, models):
    rng = self.rng
    idx = self.subset(range(len(models)))
    sinces = [max(models[i].step - int(rng.randint(0, 3)), 0) if models[i].expiring and rng.rand() < 0.6 else None
              for i in idx]
    return {'op': 'export', 'tables': idx, 'sinces': sinces}

  def import_(self, models, only=None):
    """One of a table's last three snapshots that is at least one state-changing operation old, all of it or
    what one rank of 2 or 3 owns, with or without its metadata; new keys are dropped until the rest fits."""
    rng = self.rng
    old = [(i, n) for i, m in enumerate(models) for n, (version, _) in enumerate(m.snapshots)
           if n >= len(m.snapshots) - 3 and version < m.version and only in (None, i)]
    if not old:
      return None
    i, n = old[int(rng.randint(len(old)))]
    m = models[i]
    world = (None, 2, 3)[int(rng.randint(3))]
    rank = None if world is None else int(rng.randint(world))
    keys = np.array(sorted(m.snapshots[n][1]), np.int64)
    new = [k for k in keys[m.owned(keys, world, rank)].tolist() if k not in m.stored]
    return {'op': 'import', 'table': i, 'snapshot': n, 'world': world, 'rank': rank,
            'with_meta': bool(rng.rand() < 0.5), 'drop': new[m.free():]}

  def translate_sequence(self, models, idx=None):
    rng = self.rng
    idx = self.subset(range(len(models))) if idx is None else idx
    op = {'op': 'translate_sequence', 'tables': idx, 'ids': [], 'row_splits': [], 'max_lens': [], 'pad_ids': [],
          'insert': bool(rng.rand() < 0.85), 'write': bool(rng.rand() < 0.6),
          'by': [int(rng.randint(1, 3)) if models[i].expiring and rng.rand() < 0.5 else 0 for i in idx]}
    for i in idx:
      m = models[i]
      K = keys_per_block(m.slab_size)
      T = (1, 2, 5)[int(rng.randint(3))]
      B = (0, 1, 7, K // T, K // T + 1)[int(rng.randint(5))]
      ragged = rng.rand() < 0.7   # else no row_splits: one id per sample
      lens = rng.randint(0, 2 * T + 1, size=B) if ragged else np.ones(B, np.int64)
      flat = self.draw_ids(m, int(lens.sum()))
      samples = np.split(flat, np.cumsum(lens)[:-1]) if B else []
      plain = m.pool[~m.sentinel_mask(m.pool)]
      pad = int(plain[rng.randint(plain.size)]) if rng.rand() < 0.5 else None
      while op['insert']:   # (Generator.fit, on the effective ids)
        lens = np.array([x.size for x in samples], np.int64)
        eff, _, _ = effective_ids(np.concatenate(samples) if samples else flat[:0],
                                  np.concatenate([[0], np.cumsum(lens)]), T, pad)
        drop = self.to_drop(m, eff)
        if drop is None:
          break
        if pad in drop:
          pad = None
        samples = [x[~np.isin(x, drop)] for x in samples]
      if not ragged:
        samples = [x for x in samples if x.size]
      lens = np.array([x.size for x in samples], np.int64)
      op['ids'].append(np.concatenate(samples) if samples else flat[:0])
      op['row_splits'].append(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32) if ragged else None)
      op['max_lens'].append(T)
      op['pad_ids'].append(pad)
    return op

  def tier_op(self, models):
    r = self.rng.rand()
    if r < 0.08 and self.expiring:
      return self.fill_spill_return(models)
    if r < 0.25 and self.expiring:
      return self.bound(models)
    if r < 0.37 and self.expiring:
      return self.fault_in(models)
    if r < 0.50:
      return self.export(models)
    if r < 0.75:
      return self.import_(models) or self.export(models)
    return self.translate_sequence(models)

  def next(self, models, index):
    rng = self.rng
    while self.tier and self.pending:   # (what a bound queued: made from the models as they are now)
      op = self.pending.pop(0)(models)
      if op is not None:
        return op
    if index == self.many_runs_at:
      return self.many_runs(models)
    if self.tier and rng.rand() < 0.6:
      op = self.tier_op(models)
      if op is not None:
        return op
    everyone = range(len(models))
    r = rng.rand()
    if r < 0.30:
      return self.translate(models, self.subset(everyone))
    if r < 0.35:
      return self.translate(models, self.subset(everyone), insert=False)
    if r < 0.43:
      return self.fill_exactly(models)
    if r < 0.53 and self.expiring:
      idx = self.subset(self.expiring)
      return {'op': 'step', 'tables': idx, 'by': [int(rng.randint(1, 4)) for _ in idx]}
    if r < 0.68 and self.expiring:   # a sweep, half of the time after the steps moved on
      idx = self.subset(self.expiring)
      return {'op': 'evict', 'tables': idx, 'ttl': (0, 1, 2, 4)[int(rng.randint(4))], 'keep': (0, 2)[int(rng.randint(2))],
              'by': [int(rng.randint(1, 4)) if rng.rand() < 0.5 else 0 for _ in idx]}
    if r < 0.80:
      return self.rehash(models)
    if r < 0.83:
      op = self.refused_shrink(models)
      if op is not None:
        return op
    if r < 0.86 and self.expiring:
      return {'op': 'compact', 'table': self.expiring[int(rng.randint(len(self.expiring)))]}
    if r < 0.91:
      i = int(rng.randint(len(models)))
      m = models[i]
      pool = m.pool[~m.sentinel_mask(m.pool)]
      keys = np.unique(pool[rng.randint(0, pool.size, size=int(rng.randint(0, 9)))])
      absent = [k for k in keys.tolist() if k not in m.stored]
      drop = absent[m.free():]   # only keys that fit
      return {'op': 'load', 'table': i, 'keys': keys[~np.isin(keys, drop)]}
    if r < 0.97 and self.filtered:
      return {'op': 'age' if r < 0.95 else 'clear', 'table': self.filtered[int(rng.randint(len(self.filtered)))]}
    return self.translate(models, self.subset(everyone))


# ---- the driver ---------------------------------------------------------------------------------------------
class Events:
  """Event counts per (event, table kind), and the share of translate calls whose subset was adopted."""

  def __init__(self, names=EVENTS):
    self.names = tuple(names)     # the events a list of seeds answers for
    self.counts = {}
    self.translates = self.adopted = 0

  def add(self, event, kind):
    self.counts[(event, kind)] = self.counts.get((event, kind), 0) + 1

  def missing(self):
    return [(e, k) for e in self.names for k in KINDS if applies(e, k) and not self.counts.get((e, k))]

  def report(self):
    lines = [f'{e:24s} ' + ' '.join(f'{k}={self.counts.get((e, k), 0)}' for k in KINDS if applies(e, k))
             for e in self.names]
    share = self.adopted / max(self.translates, 1)
    return '\n'.join(lines + [f'subset adopted in {self.adopted} of {self.translates} translate calls ({share:.1%})'])


class Runner:
  """Applies operations to a fleet and its models and checks every table after each."""

  def __init__(self, fleet, specs, events=None):
    self.fleet, self.specs = fleet, specs
    self.models = [Model(s) for s in specs]
    self.events = events if events is not None else Events()

    self.snapshots = [[] for _ in specs]   # the exports of every table, as arrays: beside Model.snapshots
    self.prints = [m.fingerprint() for m in self.models]

  def check_all(self):
    for t, m, c, s in zip(self.fleet.tables, self.models, self.fleet.comps, self.fleet.stores):
      check(t, m, c, s)
    for n, m in enumerate(self.models):   # (what an import may call an older state)
      now = m.fingerprint()
      m.version += int(now != self.prints[n])
      self.prints[n] = now

  def answered(self, i, ids, slots, before, op, index):
    """The answers `slots` of table i to the ids of one translate (of a sequence translate: its effective ids),
    against the model; then the row writes."""
    m, ev, fleet = self.models[i], self.events, self.fleet
    if op['insert']:
      if m.expiring and ids.size:   # resident ids whose walk passes a tombstone: a fact of the layout
        res = np.unique([k for k in ids.tolist() if k in m.stored])
        if res.size:
          order = np.argsort(before, kind='stable')
          at = order[np.searchsorted(before[order], res)]
          if passes_tombstone(before, m.slab_size, res, at).any():
            ev.add('behind_tombstone', m.kind)
      stored, events, adopted = m.translate(ids, slots)
      assert not adopted or m.regime == 'over', 'a subset was the device\'s choice outside the over-full table'
      ev.translates += 1
      ev.adopted += int(adopted)
      for e in events:
        ev.add(e, m.kind)
    else:
      stored = m.find(ids)
    keys = fleet.keys(i)
    check_slots(ids, slots, stored, keys)
    if op['write'] and stored.any():
      k, first = np.unique(ids[stored], return_index=True)
      at = slots[stored][first]
      rows = written_rows(k, index, m.dim)
      comp_rows = [written_rows(k, index, w, salt=c + 1) for c, (w, _) in enumerate(m.comp_specs)]
      fleet.write(i, at, rows, comp_rows)
      m.write(k, rows, comp_rows)

  def advance(self, op):
    for i, by in zip(op['tables'], op.get('by', ())):
      if by:
        self.models[i].set_step(self.models[i].step + by)
        self.fleet.set_step(i, self.models[i].step)

  def apply(self, op, index):
    fleet, models, ev = self.fleet, self.models, self.events
    what = op['op']
    if what == 'translate':
      idx, ids = op['tables'], op['ids']
      before = [fleet.keys(i) for i in idx] if op['insert'] else [None] * len(idx)
      slots = fleet.translate(idx, ids, op['insert'], op['route'], op['cuts'])
      for n, i in enumerate(idx):
        self.answered(i, ids[n], slots[n], before[n], op, index)
        if op['insert'] and op['route'] == 'runs' and any(a.size == 0 for a in np.split(ids[n], op['cuts'][n])):
          ev.add('empty_run', models[i].kind)
    elif what == 'translate_sequence':
      idx, ids = op['tables'], op['ids']
      self.advance(op)
      before = [fleet.keys(i) for i in idx] if op['insert'] else [None] * len(idx)
      grids, lengths = fleet.translate_sequence(idx, ids, op['row_splits'], op['max_lens'], op['pad_ids'], op['insert'])
      for n, i in enumerate(idx):
        m, T, pad = models[i], op['max_lens'][n], op['pad_ids'][n]
        eff, at, lens = effective_ids(ids[n], op['row_splits'][n], T, pad)
        assert lengths[n].dtype == np.int32
        np.testing.assert_array_equal(lengths[n], lens, err_msg='lengths')
        assert grids[n].shape == (lens.size * T,)
        rest = np.ones(grids[n].size, bool)
        rest[at] = False
        assert (grids[n][rest] == -1).all(), 'a position past a sample\'s length, without a pad id, is not -1'
        full = np.diff(np.arange(ids[n].size + 1) if op['row_splits'][n] is None else op['row_splits'][n])
        if (full > T).any():
          ev.add('sequence_truncates', m.kind)
        if pad is not None and (full < T).any():
          ev.add('sequence_pads', m.kind)
        if m.expiring and m.tomb_lb > 0 and eff.size:
          ev.add('sequence_on_tombstones', m.kind)
        self.answered(i, eff, grids[n][at], before[n], op, index)
    elif what in ('evict_to', 'spill'):
      idx, sizes, keep = op['tables'], op['max_sizes'], op['keep']
      before = [fleet.keys(i) for i in idx]
      got = (fleet.evict_to if what == 'evict_to' else fleet.spill)(idx, sizes, keep)
      for n, i in enumerate(idx):
        m = models[i]
        if what == 'evict_to':
          report, events = m.evict_to(sizes[n], keep)
          check_report(got[n], report, f'table {i}')
        else:
          want, events = m.spill(sizes[n], keep)
          check_export(m, got[n], want, before[n], f'the spill of table {i}')
        for e in events:
          ev.add(e, m.kind)
    elif what == 'fault_in':
      i, ids = op['table'], op['ids']
      m = models[i]
      before = set(m.stored) | set(m.store)
      n, raised = fleet.fault_in(i, ids)
      want, raises, events = m.fault_in(ids, fleet.keys(i))
      assert raised == raises == bool(op.get('raises')), 'a fault_in that fits raised' if raised else \
          'a fault_in that does not fit did not raise'
      assert raised or n == want, f'fault_in returned {n}, {want} keys came back'
      assert set(m.stored) | set(m.store) == before   # (and check_all: no key is lost, none is in both)
      for e in events:
        ev.add(e, m.kind)
    elif what == 'export':
      idx, sinces = op['tables'], op['sinces']
      state = [_state(fleet.tables[i], fleet.comps[i]) for i in idx]
      got = fleet.export(idx, sinces)
      for n, i in enumerate(idx):
        m = models[i]
        want, events = m.export(sinces[n])
        check_export(m, got[n], want, state[n]['keys'], f'the export of table {i}')
        same_state(state[n], _state(fleet.tables[i], fleet.comps[i]), 'an export')
        self.snapshots[i].append(got[n])
        for e in events:
          ev.add(e, m.kind)
    elif what == 'import':
      i, m = op['table'], models[op['table']]
      arrays, (_, snapshot) = self.snapshots[i][op['snapshot']], m.snapshots[op['snapshot']]
      take = np.nonzero(~np.isin(arrays['keys'], np.asarray(op.get('drop', ()), np.int64)))[0]
      kept = {k: snapshot[k] for k in arrays['keys'][take].tolist()}
      slots = fleet.import_(i, arrays, take, op.get('world'), op.get('rank'), op['with_meta'])
      mine, events = m.import_(kept, op.get('world'), op.get('rank'), op['with_meta'])
      own = m.owned(arrays['keys'][take], op.get('world'), op.get('rank'))
      assert slots.shape == (int(own.sum()),)
      np.testing.assert_array_equal(fleet.keys(i)[slots], arrays['keys'][take][own],
                                    err_msg='the returned slots do not hold the imported keys')
      for e in events:
        ev.add(e, m.kind)
    elif what == 'step':
      for i, by in zip(op['tables'], op['by']):
        models[i].set_step(models[i].step + by)
        fleet.set_step(i, models[i].step)
    elif what == 'evict':
      for i, by in zip(op['tables'], op.get('by', ())):
        if by:
          models[i].set_step(models[i].step + by)
          fleet.set_step(i, models[i].step)
      fleet.evict(op['tables'], op['ttl'], op['keep'])
      for i in op['tables']:
        if models[i].evict(op['ttl'], op['keep']):
          ev.add('eviction', models[i].kind)
    elif what == 'rehash':
      idx, geometry = op['tables'], op['geometry']
      fits = all(models[i].fits(ss, sc) for i, (ss, sc) in zip(idx, geometry))
      assert fits != bool(op.get('refused'))
      before = [(fleet.tables[i].keys, fleet.tables[i].table) for i in idx]
      done = fleet.rehash(idx, geometry)
      assert done == fits, 'a rehash was refused that fits' if fits else 'a shrink below size() was accepted'
      if not fits:   # nothing changed: the same arrays, and check_all compares their contents
        assert all(fleet.tables[i].keys is k and fleet.tables[i].table is t for i, (k, t) in zip(idx, before))
      else:
        for i, (ss, sc) in zip(idx, geometry):
          m = models[i]
          if ss * sc > m.capacity:
            ev.add('growth', m.kind)
          if ss * sc == m.capacity and m.tomb_lb > 0:
            ev.add('rehash_sheds_tombstones', m.kind)
          m.rehash(ss, sc)
    elif what == 'compact':
      fleet.compact(op['table'])
      models[op['table']].compact()
    elif what == 'load':
      i, keys = op['table'], op['keys']
      rows = written_rows(keys, index, models[i].dim, salt=9)
      fleet.load(i, keys, rows)
      models[i].load(keys, rows)
    elif what == 'age':
      fleet.age_filter(op['table'])
      models[op['table']].age_filter()
    elif what == 'clear':
      fleet.clear_filter(op['table'])
      models[op['table']].clear_filter()
    else:
      raise AssertionError(what)
    self.check_all()


def run_seed(seed, make, events=None, n_ops=40, tier=False):
  """One seeded sequence; `make(specs)` builds the fleet to drive.  `tier`: with the operations of
  ``Generator.tier_op`` (the TIER_SEEDS)."""
  rng = np.random.RandomState(1000 + seed)
  specs = make_fleet(rng)
  runner = Runner(make(specs), specs, events)
  runner.check_all()
  gen = Generator(rng, specs, n_ops, tier)
  for index in range(n_ops):
    op = gen.next(runner.models, index)
    try:
      runner.apply(op, index)
    except AssertionError as e:
      raise AssertionError(f'seed {seed}, operation {index}: {describe(op)}\n{e}') from e
  return runner


def describe(op):
  out = {k: v for k, v in op.items() if k not in ('ids', 'cuts', 'keys', 'row_splits', 'drop')}
  if 'ids' in op:
    out['n_ids'] = [int(x.size) for x in op['ids']] if isinstance(op['ids'], list) else int(op['ids'].size)
  if 'cuts' in op:
    out['n_runs'] = [len(c) + 1 for c in op['cuts']]
  if 'drop' in op:
    out['n_dropped'] = len(op['drop'])
  return str(out)


# ---- sequences written out by hand ------------------------------------------------------------------------
def _homing(slab_count, slab, n, start=1):
  """The first n positive ids from `start` on whose home slab is `slab`."""
  out, k = [], start
  while len(out) < n:
    if ref.home_slab(k, slab_count) == slab:
      out.append(k)
    k += 1
  return np.array(out, np.int64)


def _call(i, ids, insert=True, route='plain', cuts=(), write=False):
  return {'op': 'translate', 'tables': [i], 'ids': [np.asarray(ids, np.int64)], 'insert': insert, 'route': route,
          'cuts': [list(cuts)], 'write': write}


def fixed_refill_of_tombstones():
  """A 3 x 5 expiring table filled to the last slot by ids that all home into slab 1 (ten of them spill), everything
  evicted -- fifteen tombstones, no EMPTY slot -- then ONE call with every old id twice: each must land on a
  tombstone once, whichever occurrence is first, and start from its initial row.  Then five ids are evicted while
  ten stay, most of them spilled behind the new tombstones: they must be found there, not stored a second time in
  the first tombstone of their walk, and the five come back onto the tombstones."""
  old = _homing(3, 1, 15)
  spec = Spec('expiring', 5, 3, 4, [(4, 0.1)], 'tight', np.concatenate([old, [EMPTY, TOMBSTONE]]), seed=3)
  twice = np.concatenate([old, old[::-1]])
  sweep = {'op': 'evict', 'tables': [0], 'ttl': 1, 'keep': 0}
  ops = [_call(0, old, write=True), {'op': 'step', 'tables': [0], 'by': [2]}, dict(sweep), _call(0, twice, write=True),
         _call(0, twice, route='runs', cuts=(7, 7, 19)),
         {'op': 'step', 'tables': [0], 'by': [2]}, _call(0, old[5:]), dict(sweep), _call(0, old[5:], write=True),
         _call(0, old[5:][::-1], route='runs', cuts=(3,)), _call(0, twice), _call(0, old, insert=False)]
  return [spec], ops


def fixed_sighting_across_evict_and_rehash():
  """A filtered expiring table (min_freq 3): an id is seen twice, then the table is swept and rehashed, then the id
  is seen a third time: the sketch survives both, so the third sighting admits it."""
  late = np.array([-5, 5 + (1 << 32)], np.int64)
  early = _homing(3, 0, 7, start=100)
  spec = Spec('expiring_admit', 5, 3, 4, [(1, -2.5)], 'roomy', np.concatenate([late, early, [EMPTY, TOMBSTONE]]),
              min_freq=3, depth=4, width=64, seed=1, sketch_seed=2)
  ops = [_call(0, np.repeat(early, 3), write=True), _call(0, late), {'op': 'step', 'tables': [0], 'by': [1]},
         _call(0, np.concatenate([late, early[:3]])), {'op': 'step', 'tables': [0], 'by': [2]},
         {'op': 'evict', 'tables': [0], 'ttl': 2, 'keep': 0},
         {'op': 'rehash', 'tables': [0], 'geometry': [(8, 2)]},
         _call(0, np.concatenate([late, early]), route='runs', cuts=(1, 1), write=True),
         _call(0, np.concatenate([late, early]), insert=False)]
  return [spec], ops


def fixed_two_rehashes_around_a_write():
  """dim 19 (4-byte moves) with a width-4 companion (16-byte moves): growth, a row write, another slab size; the rows
  written between the two rehashes must arrive."""
  pool = np.concatenate([_homing(20, 2, 9), np.arange(-30, 30, dtype=np.int64) * 977, [EMPTY]])
  spec = Spec('plain', 5, 20, 19, [(4, 0.1)], 'roomy', pool, seed=5)
  keys = pool[:-1]
  ops = [_call(0, keys, write=True), {'op': 'rehash', 'tables': [0], 'geometry': [(5, 40)]},
         _call(0, keys[::2], insert=False, write=True), {'op': 'rehash', 'tables': [0], 'geometry': [(33, 6)]},
         _call(0, keys, insert=False)]
  return [spec], ops


def _step(by=1):
  return {'op': 'step', 'tables': [0], 'by': [by]}


def fixed_spill_chain_and_return():
  """A 3 x 5 filtered expiring table filled to the last slot by ids that all home into slab 1, with a width-4 and a
  width-1 companion, rows written, in three age groups of five.  A spill to a bound inside the middle group takes
  the two older groups: ten tombstones in front of and among the five keys that stay.  ONE fault_in then asks for
  six spilled ids twice each, the resident ids (behind the tombstones now), ids never seen and both sentinels: the
  six come back as they left, nothing else appears.  A translate stamps two of them and brings two ids back FRESH
  while the store still holds them; a second spill takes returned keys again and the two fresh ones (the store
  upserts); the table is rehashed to 8 x 2 and everything left comes back."""
  old = _homing(3, 1, 15)
  never = _homing(3, 1, 4, start=int(old[-1]) + 1)
  spec = Spec('expiring_admit', 5, 3, 4, [(4, 0.1), (1, -2.5)], 'tight',
              np.concatenate([old, never, [EMPTY, TOMBSTONE]]), min_freq=2, depth=4, width=64, seed=7, sketch_seed=3)
  back = old[[0, 2, 4, 5, 7, 9]]
  asked = np.concatenate([back, old[10:], never, [EMPTY, TOMBSTONE], back[::-1], never[:2]])
  spill = {'op': 'spill', 'tables': [0], 'keep': 0}
  ops = [_call(0, np.repeat(old, 2), write=True), _step(), _call(0, old[5:], write=True), _step(),
         _call(0, old[10:], route='runs', cuts=(2,), write=True),
         dict(spill, max_sizes=[8]),                                    # need 7, the cut inside the group of step 1
         {'op': 'fault_in', 'table': 0, 'ids': asked},
         _call(0, np.concatenate([old[[1, 3]], back[:2], old[10:11]]), write=True),   # 1, 3: fresh over the store
         _step(), _call(0, np.concatenate([old[11:14], back[2:3]])),
         dict(spill, max_sizes=[5]),                                    # 13 keys, four of step 3: nine leave
         {'op': 'rehash', 'tables': [0], 'geometry': [(8, 2)]},
         {'op': 'fault_in', 'table': 0, 'ids': np.concatenate([old, old])},
         _call(0, old, insert=False)]
  return [spec], ops


def fixed_fault_in_that_does_not_fit():
  """A full 3 x 5 expiring table spills ten keys, six new ids take six of the tombstones, and a fault_in asks for
  all ten: four fit.  The call must raise; afterwards the four are in the table as they left, the six are in the
  store again, nothing is lost and nothing is in both.  Which four is the device's choice.  After a rehash to
  24 slots the six follow."""
  old = _homing(3, 1, 15)
  new = _homing(3, 2, 6, start=1000)
  spec = Spec('expiring', 5, 3, 4, [(4, 0.1)], 'tight', np.concatenate([old, new, [EMPTY, TOMBSTONE]]), seed=11)
  ops = [_call(0, old, write=True), _step(), _call(0, old[10:], write=True),
         {'op': 'spill', 'tables': [0], 'keep': 0, 'max_sizes': [5]},
         _call(0, new, write=True),
         {'op': 'fault_in', 'table': 0, 'ids': np.concatenate([old, old[:10]]), 'raises': True},
         {'op': 'rehash', 'tables': [0], 'geometry': [(8, 3)]},
         {'op': 'fault_in', 'table': 0, 'ids': old},
         _call(0, np.concatenate([old, new]), insert=False)]
  return [spec], ops


def fixed_snapshot_over_a_moved_table():
  """dim 19 with a width-4 companion, expiring: a full export; then a sweep evicts a third of the keys, rows are
  written, the table moves to another slab size and takes new keys -- and the old snapshot is imported with its
  metadata: evicted keys return as they were, written rows are overwritten, the new keys stay.  Then a delta
  export of that second state; an evict_to takes seven of its nine keys and the table moves again; the delta is
  imported without metadata: seven keys are new, two are overwritten, all nine count as seen now."""
  first = np.concatenate([_homing(20, 2, 9), np.arange(-20, 20, dtype=np.int64) * 977])
  later = np.arange(1, 13, dtype=np.int64) * 7919 + (1 << 32)
  spec = Spec('expiring', 5, 20, 19, [(4, 0.1)], 'roomy', np.concatenate([first, later, [EMPTY, TOMBSTONE]]), seed=5)
  ops = [_call(0, first, write=True), _step(), _call(0, first[::3], write=True), _step(), _call(0, first[1::3]),
         {'op': 'export', 'tables': [0], 'sinces': [None]},
         _step(), {'op': 'evict', 'tables': [0], 'ttl': 3, 'keep': 0},           # first[2::3], last seen at step 0
         _call(0, first[::3], insert=False, write=True),
         {'op': 'rehash', 'tables': [0], 'geometry': [(33, 3)]},
         _call(0, later, write=True),
         {'op': 'import', 'table': 0, 'snapshot': 0, 'with_meta': True},
         _step(), _call(0, np.concatenate([later[:5], first[2::3][:4]]), write=True),
         {'op': 'export', 'tables': [0], 'sinces': [4]},                         # the nine keys of step 4
         _step(), _call(0, np.concatenate([first[::3], later[:2]])),
         {'op': 'evict_to', 'tables': [0], 'keep': 0, 'max_sizes': [20]},        # all of step 4 and before: 42 keys
         {'op': 'rehash', 'tables': [0], 'geometry': [(8, 12)]},
         _call(0, later[:2], insert=False, write=True), _step(2),
         {'op': 'import', 'table': 0, 'snapshot': 1, 'with_meta': False},
         _call(0, np.concatenate([first, later]), insert=False)]
  return [spec], ops


FIXED = {'refill_of_tombstones': fixed_refill_of_tombstones,
         'sighting_across_evict_and_rehash': fixed_sighting_across_evict_and_rehash,
         'two_rehashes_around_a_write': fixed_two_rehashes_around_a_write,
         'spill_chain_and_return': fixed_spill_chain_and_return,
         'fault_in_that_does_not_fit': fixed_fault_in_that_does_not_fit,
         'snapshot_over_a_moved_table': fixed_snapshot_over_a_moved_table}


def run_fixed(name, make, events=None):
  specs, ops = FIXED[name]()
  runner = Runner(make(specs), specs, events)
  runner.check_all()
  for index, op in enumerate(ops):
    try:
      runner.apply(op, index)
    except AssertionError as e:
      raise AssertionError(f'{name}, operation {index}: {describe(op)}\n{e}') from e
  return runner
