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

Events (``Events``) are computed from the model and the geometry alone -- pigeonhole bounds where a layout fact is
wanted: more stored keys homing to one slab than it has slots means one of them overflowed; more new keys than the
table can still have EMPTY slots means a tombstone was reused.  The one exception is "an id found behind a
tombstone", which only a layout can tell: it is read off the key array of the side that is driven (the sequential
restatement in the model test).
"""
import ctypes as C

import numpy as np

from tests.support import hash_admission_ref as aref
from tests.support import hash_expiry_ref as xref
from tests.support import hash_ref as ref
from tests.support import hash_rehash_ref as rref

EMPTY = ref.EMPTY
TOMBSTONE = EMPTY + 1
KINDS = ('plain', 'expiring', 'admit', 'expiring_admit')
SLAB_SIZES = (1, 5, 8, 16, 33, 64)
SLAB_COUNTS = (1, 3, 20, 257)
MAX_CAPACITY = 1300
SEEDS = tuple(range(10))   # chosen so that the conditions of tests/test_hash_lifecycle_model.py hold
EVENTS = ('overflow', 'eviction', 'reused', 'behind_tombstone', 'exact_admission', 'early_admission', 'growth',
          'rehash_sheds_tombstones', 'fills_last_slot', 'empty_run')
_EXPIRING_EVENTS = ('eviction', 'reused', 'behind_tombstone', 'rehash_sheds_tombstones')
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


def check(table, model, companions):
  """The table (a ``HashTable`` or a ``NumpyTable``) and its companion arrays against the model: keys, reachability
  by every reader, per-key and per-free-slot values bit for bit, the counters and the sketch; and that the finds it
  makes change nothing."""
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
    np.testing.assert_array_equal(s['last_seen'][slot_of], np.array([r.last_seen for r in recs], np.int32))
    np.testing.assert_array_equal(s['freq'][slot_of], np.array([r.freq for r in recs], np.int32))
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
  again = _state(table, companions)
  for name, a in s.items():
    np.testing.assert_array_equal(bits(a) if a.dtype == np.float32 else a,
                                  bits(again[name]) if a.dtype == np.float32 else again[name],
                                  err_msg=f'a find changed {name}')
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
class NumpyFleet:
  def __init__(self, specs, order=None):
    self.tables = [NumpyTable(s, order) for s in specs]
    self.comps = [[np.full((s.capacity, w), v, np.float32) for w, v in s.comps] for s in specs]
    self.fills = [[v for _, v in s.comps] for s in specs]

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


class DeviceFleet:
  """``HashTable``s on the GPU; fleet-wide calls go through hash_translate / hash_evict / hash_rehash."""

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

  def __init__(self, rng, specs, n_ops=40):
    self.rng, self.specs, self.n_ops = rng, specs, n_ops
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

  def fit(self, model, ids):
    """Outside the over-full table no call may offer more new ids than there are free slots (0 < F < D is the
    device's choice): occurrences of candidates are dropped until D <= F.  And a call that must fail walks every
    slab per failing occurrence: those are kept to a number the sequential restatement gets through quickly.
    Decided by the model alone."""
    while True:
      D, F, occurrences = model.preview(ids)
      absent = [k for k in np.unique(ids).tolist() if k not in model.stored and not model.sentinel_mask([k])[0]]
      if model.regime != 'over' and 0 < F < D:
        ids = ids[~np.isin(ids, absent[:max(1, D - F)])]
      elif D > F and occurrences * model.slab_count > 20000:
        ids = ids[~np.isin(ids, absent[:len(absent) // 2 + 1])]
      else:
        return ids

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

  def fill_exactly(self, models):
    """A call that offers one table exactly as many new ids as it has free slots, each often enough to pass its
    filter, among resident ids."""
    rng = self.rng
    order = rng.permutation(len(models)).tolist()
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
    return self.translate(models, self.subset(range(len(models))))

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

  def next(self, models, index):
    rng = self.rng
    if index == self.many_runs_at:
      return self.many_runs(models)
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

  def __init__(self):
    self.counts = {}
    self.translates = self.adopted = 0

  def add(self, event, kind):
    self.counts[(event, kind)] = self.counts.get((event, kind), 0) + 1

  def missing(self):
    return [(e, k) for e in EVENTS for k in KINDS if applies(e, k) and not self.counts.get((e, k))]

  def report(self):
    lines = [f'{e:24s} ' + ' '.join(f'{k}={self.counts.get((e, k), 0)}' for k in KINDS if applies(e, k))
             for e in EVENTS]
    share = self.adopted / max(self.translates, 1)
    return '\n'.join(lines + [f'subset adopted in {self.adopted} of {self.translates} translate calls ({share:.1%})'])


class Runner:
  """Applies operations to a fleet and its models and checks every table after each."""

  def __init__(self, fleet, specs, events=None):
    self.fleet, self.specs = fleet, specs
    self.models = [Model(s) for s in specs]
    self.events = events if events is not None else Events()

  def check_all(self):
    for t, m, c in zip(self.fleet.tables, self.models, self.fleet.comps):
      check(t, m, c)

  def apply(self, op, index):
    fleet, models, ev = self.fleet, self.models, self.events
    what = op['op']
    if what == 'translate':
      idx, ids = op['tables'], op['ids']
      before = [fleet.keys(i) for i in idx] if op['insert'] else None
      slots = fleet.translate(idx, ids, op['insert'], op['route'], op['cuts'])
      for n, i in enumerate(idx):
        m = models[i]
        if op['insert']:
          if m.expiring and ids[n].size:   # resident ids whose walk passes a tombstone: a fact of the layout
            res = np.unique([k for k in ids[n].tolist() if k in m.stored])
            if res.size:
              order = np.argsort(before[n], kind='stable')
              at = order[np.searchsorted(before[n][order], res)]
              if passes_tombstone(before[n], m.slab_size, res, at).any():
                ev.add('behind_tombstone', m.kind)
          stored, events, adopted = m.translate(ids[n], slots[n])
          assert not adopted or m.regime == 'over', 'a subset was the device\'s choice outside the over-full table'
          ev.translates += 1
          ev.adopted += int(adopted)
          for e in events:
            ev.add(e, m.kind)
          if op['route'] == 'runs' and any(a.size == 0 for a in np.split(ids[n], op['cuts'][n])):
            ev.add('empty_run', m.kind)
        else:
          stored = m.find(ids[n])
        keys = fleet.keys(i)
        check_slots(ids[n], slots[n], stored, keys)
        if op['write'] and stored.any():
          k, first = np.unique(ids[n][stored], return_index=True)
          at = slots[n][stored][first]
          rows = written_rows(k, index, m.dim)
          comp_rows = [written_rows(k, index, w, salt=c + 1) for c, (w, _) in enumerate(m.comp_specs)]
          fleet.write(i, at, rows, comp_rows)
          m.write(k, rows, comp_rows)
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


def run_seed(seed, make, events=None, n_ops=40):
  """One seeded sequence; `make(specs)` builds the fleet to drive."""
  rng = np.random.RandomState(1000 + seed)
  specs = make_fleet(rng)
  runner = Runner(make(specs), specs, events)
  runner.check_all()
  gen = Generator(rng, specs, n_ops)
  for index in range(n_ops):
    op = gen.next(runner.models, index)
    try:
      runner.apply(op, index)
    except AssertionError as e:
      raise AssertionError(f'seed {seed}, operation {index}: {describe(op)}\n{e}') from e
  return runner


def describe(op):
  out = {k: v for k, v in op.items() if k not in ('ids', 'cuts', 'keys')}
  if 'ids' in op:
    out['n_ids'] = [int(x.size) for x in op['ids']]
    out['n_runs'] = [len(c) + 1 for c in op['cuts']]
  return str(out)


# ---- three sequences written out by hand ------------------------------------------------------------------------
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


FIXED = {'refill_of_tombstones': fixed_refill_of_tombstones,
         'sighting_across_evict_and_rehash': fixed_sighting_across_evict_and_rehash,
         'two_rehashes_around_a_write': fixed_two_rehashes_around_a_write}


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
