"""Hash-keyed embedding tables: rows addressed by the RAW int64 id instead of ``floormod(id, num_buckets)``,
so two ids never share a row, its gradient and its optimizer slots (DeepRec's EmbeddingVariable; the
reference's ``EmbeddingService``, hybridbackend/tensorflow/embedding/service.py:153-283, in miniature).
Host side of ``hbk_hash_insert_n`` (include/hbk.h): a device find-or-insert that turns ids into row numbers
of a fixed-capacity table whose key array is exactly the slab cache ``hb.embedding.cache.probe`` reads.

The row numbers then feed the existing lookups with ``bucket = 0``: :class:`HashGroupLookup` is one
translate launch in front of a :class:`GroupLookup`, and ``GroupLookupGrad(hgl.lookup, ...)`` called on
``hgl.slots`` is its backward and optimizer step -- every reduce plan, ``deterministic=True``, max_norm,
weights, SGD, Adagrad, Lazy Adam and FTRL unchanged.

Expiring tables (``HashTable(..., expiring=True)``; ``hbk_hash_insert_expiring_n`` / ``hbk_hash_evict_n``):
every slot carries the step it was last seen at and how often it was seen, both written by the translate
launch; :meth:`HashTable.evict` turns idle slots into TOMBSTONEs (``INT64_MIN + 1``) and resets their
optimizer slots, later inserts reuse them, :meth:`HashTable.compact` turns tombstones back into EMPTY slots.

Admission filter (``HashTable(..., min_freq=F)``; ``hbk_hash_insert_admit_n`` /
``hbk_hash_insert_expiring_admit_n``; DeepRec's CounterFilter / CBFFilter): an id gets a row once a count-min
sketch of the table has seen it ``F`` times; until then it translates to -1 -- a zero row, no gradient, no
optimizer slot (DeepRec reads its default-value row there).

Growth and compaction (``hbk_hash_rehash_n``): :meth:`HashTable.rehash` / :func:`hash_rehash` move every live
key of N tables into fresh arrays of any geometry in ONE launch -- rows, ``last_seen``, ``freq`` and the optimizer
slots moving along, no host round trip when the table does not shrink; ``t.rehash()`` is a device-side
``compact()``.  :meth:`HashTable.maybe_grow` / :meth:`HashGroupLookup.maybe_grow` decide from the counters (one
host read) whether a table must grow or shed its tombstones.  A rehash changes slot numbers and tensor
addresses: :meth:`HashGroupLookup.rebind`, a new ``GroupLookupGrad`` over the new slot tensors, a new capture
of any captured graph.

Bounded tables (``hbk_hash_evict_to_n``): :meth:`HashTable.evict_to` / :func:`hash_evict_to` evict the oldest keys
down to a size bound, the cut found on the device (whole steps leave together: no exact size, no tie-break);
:meth:`HashTable.maybe_evict` / :meth:`HashGroupLookup.maybe_evict` are ``maybe_grow`` for a fixed memory budget.
``order='lfu'`` (``hbk_hash_evict_to_lfu_n``) on any of them picks the least frequently used keys instead, the oldest
first among equally frequent ones; :meth:`HashTable.age_freq` lets old popularity fade.

Spilling to a host tier (``hbk_hash_evict_to_select_n`` / ``hbk_hash_spill_n``): :meth:`HashTable.spill_to` /
:func:`hash_spill` export exactly the keys an ``evict_to`` would remove -- rows, ``last_seen``, ``freq`` and the
optimizer slots -- and then remove them; a :class:`HashSpillStore` keeps them on the host, and
:meth:`HashTable.fault_in` / :meth:`HashGroupLookup.fault_in` bring a batch's spilled keys back as they left before
the translate.  ``maybe_evict(..., spill=store)`` spills where it evicted.  :func:`hash_missing`
(``hbk_hash_missing_n``) reports, for N tables in one C call, the distinct ids the tables do not hold, in
first-occurrence order and without writing a table; :func:`hash_fault_in` asks the stores of N tables for them after
one such call, and with ``max_lens`` reads the ids as a sequence lookup does (``HashSequenceLookup.fault_in``).

Removal by id (``hbk_hash_remove_n``): :meth:`HashTable.remove` / :func:`hash_remove` take the keys the caller
names out of N expiring tables -- a find and an erase launch, the old slots returned, the companions reset as a sweep
resets them.  :meth:`HashTable.track_removals` records every key that leaves (removed, evicted or spilled), and a
delta export of a tracking table carries them (``HashExport.removed``), so base + deltas restore the table that was
saved, not a superset of it.

Sharded hash tables: :class:`hybridbackend_amd.embedding.ShardedHashGroupLookup` (sharded_hash.py) puts tables of
W ranks behind the sharded lookup step, owner = :func:`hash_owner`; :meth:`HashTable.load_owned` restores
``items()`` of W ranks onto W' ranks.

Export and import (``hbk_hash_export_n`` / ``hbk_hash_store_rows_n``): :meth:`HashTable.export_items` /
:func:`hash_export` pack the keys of N tables -- all, or those seen since a step: an incremental checkpoint --
with rows, ``last_seen``, ``freq`` and the optimizer slots into a :class:`HashExport`, in ascending slot order;
:meth:`HashTable.import_items` upserts one into a table of any geometry or, with ``world`` / ``rank``, onto any
number of ranks.  ``items()`` / ``load()`` / ``load_owned()`` / ``variables()`` are what they were.

16-bit rows (``HashTable(..., dtype=torch.bfloat16 / torch.float16)``; ``hbk_hash_insert_lowp_n``): the inserting
launch rounds a new row to the table's 16 bits, every move carries rows as 4-byte words whatever they hold, and
:class:`HashGroupLookup` puts a ``LowpGroupLookup`` behind the translate; ``LowpLookupGrad`` is the step.

Not provided: 16-bit tables behind sequence lookups, sharded tables and the feature columns; growth from inside a
translate launch (a full table answers -1 until ``maybe_grow`` ran), a
compaction that keeps the tensors' addresses, the TF shim op.  (As feature columns: ``feature_column.
HashEmbeddingColumn`` / ``HashSequenceEmbeddingColumn``.)
"""
import ctypes as C
import math
import threading

import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding.cache import EMPTY_KEY
from hybridbackend_amd.embedding.lookup import GroupLookup

TOMBSTONE_KEY = EMPTY_KEY + 1   # expiring tables only: a slot the eviction sweep took back
LOWP_DTYPES = {torch.bfloat16: _lib.LOWP_BF16, torch.float16: _lib.LOWP_FP16}   # HashTable(dtype=): 16-bit rows


def _bad(msg):
  return _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, msg)


def _per_table(n, *named):
  """Per-table argument lists: ``(name, value, default)`` each -- None becomes ``n`` defaults, anything else a list;
  all of them must then hold exactly ``n`` entries.  Returns the lists in order."""
  lists = [[default] * n if value is None else list(value) for _, value, default in named]
  if any(len(x) != n for x in lists):
    def listed(words):
      words = [str(w) for w in words]
      return words[0] if len(words) == 1 else ', '.join(words[:-1]) + ' and ' + words[-1]
    raise _bad(f'expected {n} {listed(name for name, _, _ in named)}, got {listed(len(x) for x in lists)}')
  return lists


def _check_geometry(capacity, slab_size, where=''):
  if not 1 <= slab_size <= 64:
    raise _bad(f'{where}slab_size must be in [1, 64], got {slab_size}')
  if capacity < slab_size:
    raise _bad(f'{where}capacity {capacity} is below one slab of {slab_size} slots')


def _read_counters(tables):
  """``(inserted, failed, evicted, reused)`` of every table -- 0 evicted and reused for one that is not expiring --
  from ONE host read for all of them."""
  parts = [x for t in tables for x in ((t.counts, t.stats) if t.expiring else (t.counts,))]
  words = iter((parts[0] if len(parts) == 1 else torch.cat(parts)).tolist())
  return [(next(words), next(words)) + ((next(words), next(words)) if t.expiring else (0, 0)) for t in tables]


class HashTable:
  """A fixed-capacity table keyed by raw int64 ids.

  Args:
    capacity: rows; rounded DOWN to whole slabs (``self.capacity``); below one slab is refused.
    dim: floats per row.
    device: where ``keys`` / ``table`` live.
    slab_size: slots per slab, 1..64: a key lives in slab ``murmur3_hash32(id) % slab_count`` or, when that
      one is full, in the next.  The default, 8 (one 64-byte request per key), is the fastest of 8 / 16 / 32 /
      64 in every case of profiles/hash_insert.txt; the time grows with the bytes read per key.
    init_scale: a new row starts uniform in ``[-init_scale, init_scale)``, a function of (id, seed, column)
      alone (include/hbk.h): the same id starts from the same row whatever slot it gets; 0: zeros.
    seed: of the row initialisation.
    expiring: False -- nothing below is allocated and nothing changes.  True -- the table can forget: see
      :meth:`set_step`, :meth:`evict` and :meth:`compact`.  The ids ``INT64_MIN`` and ``INT64_MIN + 1``
      (TOMBSTONE) are then never stored.
    min_freq: 0 -- no filter: nothing below is allocated and nothing changes.  F >= 1 -- an id is stored by the
      translate call (``insert=True``) after whose counting phase its estimate reaches F; before that it
      translates to -1, counted in :meth:`filtered`.  Ids the table holds are not counted.
    sketch_depth / sketch_width / sketch_seed: the count-min sketch, ``depth`` rows (1..8) of ``width`` int32
      counters (None: ``capacity``); an id's cell in row r is ``sketch_cells``'s.  Collisions only add: an id
      may be admitted early, never late.
    dtype: ``torch.float32`` -- nothing changes -- or ``torch.bfloat16`` / ``torch.float16``: ``table`` holds
      16-bit rows (``dim`` even; fp16: ``init_scale <= 65504``), a new row is the fp32 start value rounded to
      nearest even by the inserting launch (``hbk_hash_insert_lowp_n``), and every row-carrying call -- ``items``,
      ``load``, ``export_items`` / ``import_items``, the spill store, ``variables`` -- carries rows of this dtype
      bit for bit and refuses another.  The metadata and the companions (optimizer slots) stay what they were,
      fp32.  Look up through :class:`HashGroupLookup`, step with ``LowpLookupGrad``; sequence lookups, sharded
      tables and the feature-column layers take fp32 tables only.

  Attributes of a filtered table: ``sketch`` int32 ``[depth, width]``, ``filter_counts`` int32 ``[1]`` = id
  occurrences the filter answered -1.  The sketch is never decremented, so an id evicted from an expiring table
  is admitted again at once unless :meth:`clear_filter` or :meth:`age_filter` ran.

  Attributes of an expiring table: ``last_seen`` / ``freq`` int32 ``[capacity]`` (the step of a slot's last
  translate with ``insert=True`` and its occurrences so far, saturating at 2^30; :meth:`age_freq` lets them
  fade), ``step`` int32 ``[1]`` on the device (:meth:`set_step`), ``stats`` int32 ``[2]`` = keys evicted / keys
  stored into a reused slot.

  Attributes: ``keys`` int64 ``[slab_count * slab_size]`` (EMPTY = INT64_MIN), ``table`` ``dtype``
  ``[capacity, dim]``, ``counts`` int32 ``[2]`` = keys inserted (since the last rehash or compact: the keys it
  moved count as inserted) / id occurrences answered -1 by inserting calls (table full, or a sentinel id) so far.
  """

  def __init__(self, capacity, dim, device, slab_size=8, init_scale=1e-3, seed=0, expiring=False, min_freq=0,
               sketch_depth=4, sketch_width=None, sketch_seed=0, dtype=torch.float32):
    slab_size, capacity, dim = int(slab_size), int(capacity), int(dim)
    _check_geometry(capacity, slab_size)
    if dim < 1:
      raise _bad(f'dim must be >= 1, got {dim}')
    init_scale = float(init_scale)
    if not math.isfinite(init_scale) or init_scale < 0 or not math.isfinite(C.c_float(init_scale).value):
      raise _bad(f'init_scale must be finite and >= 0, got {init_scale!r}')
    if dtype != torch.float32 and dtype not in LOWP_DTYPES:
      raise _bad(f'dtype must be torch.float32, torch.bfloat16 or torch.float16, got {dtype!r}')
    if dtype in LOWP_DTYPES and dim % 2:
      raise _bad(f'dim must be even on a {dtype} table (a 16-bit row is written and moved as 4-byte words), got {dim}')
    if dtype == torch.float16 and init_scale > 65504.0:
      raise _bad(f'init_scale {init_scale!r} is above 65504, the largest torch.float16: a start value would round to '
                 'infinity')
    self.dtype = dtype
    self.slab_size = slab_size
    self.slab_count = capacity // slab_size
    self.capacity = self.slab_count * slab_size
    self.dim = dim
    self.init_scale = init_scale
    self.seed = int(seed)
    self.device = torch.device(device)
    self.keys = torch.full((self.capacity,), EMPTY_KEY, dtype=torch.int64, device=self.device)
    self.table = torch.zeros((self.capacity, dim), dtype=dtype, device=self.device)
    self.counts = torch.zeros(2, dtype=torch.int32, device=self.device)
    self.expiring = bool(expiring)
    self._removals = None   # track_removals(): the keys that left, as device tensors
    if self.expiring:
      self.last_seen = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
      self.freq = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
      self.step = torch.zeros(1, dtype=torch.int32, device=self.device)
      self.stats = torch.zeros(2, dtype=torch.int32, device=self.device)
    self.min_freq = int(min_freq)
    if not 0 <= self.min_freq <= 2 ** 30:
      raise _bad(f'min_freq must be in [0, 2^30], got {min_freq}')
    if self.min_freq:
      depth = int(sketch_depth)
      width = self.capacity if sketch_width is None else int(sketch_width)
      if not 1 <= depth <= _lib.HASH_MAX_SKETCH_DEPTH:
        raise _bad(f'sketch_depth must be in [1, {_lib.HASH_MAX_SKETCH_DEPTH}], got {sketch_depth}')
      if not 1 <= width < 2 ** 31:
        raise _bad(f'sketch_width must be in [1, 2^31), got {sketch_width}')
      if not -2 ** 63 <= int(sketch_seed) < 2 ** 63:
        raise _bad(f'sketch_seed must be an int64, got {sketch_seed}')
      self.sketch_seed = int(sketch_seed)
      self.sketch = torch.zeros((depth, width), dtype=torch.int32, device=self.device)
      self.filter_counts = torch.zeros(1, dtype=torch.int32, device=self.device)

  def _describe(self, col, init=True, count=True):
    """The table side of a descriptor."""
    col.keys_cache = self.keys.data_ptr()
    col.slab_count = self.slab_count
    col.slab_size = self.slab_size
    col.counts = self.counts.data_ptr() if count else None
    col.table = self.table.data_ptr() if init else None
    col.dim = self.dim
    col.table_pitch = 0
    col.init_scale = self.init_scale
    col.seed = self.seed

  def _describe_expiry(self, exp):
    exp.last_seen = self.last_seen.data_ptr()
    exp.freq = self.freq.data_ptr()
    exp.step = self.step.data_ptr()
    exp.stats = self.stats.data_ptr()

  def _describe_admission(self, adm):
    adm.sketch = self.sketch.data_ptr()
    adm.depth, adm.width = self.sketch.shape
    adm.min_freq = self.min_freq
    adm.seed = self.sketch_seed
    adm.filtered = self.filter_counts.data_ptr()

  def _need_filter(self, what):
    if not self.min_freq:
      raise _bad(f'{what} needs a table built with min_freq >= 1')

  def _need_expiring(self, what):
    if not self.expiring:
      raise _bad(f'{what} needs a table built with expiring=True')

  def _live(self):
    """Mask of the slots that hold a key."""
    live = self.keys != EMPTY_KEY
    return live & (self.keys != TOMBSTONE_KEY) if self.expiring else live

  def _check_rows_dtype(self, rows):
    """The dtype check of :meth:`load` and :meth:`load_owned`, made before anything else is looked at: rows of
    another dtype are refused, never cast."""
    if isinstance(rows, torch.Tensor) and rows.dtype != self.dtype:
      raise _bad(f'load: rows must be {_dtype_name(self.dtype)}, the table\'s own dtype (nothing is cast: a round '
                 f'trip is bit-exact), got {rows.dtype}')

  def lookup_or_insert(self, ids):
    """Row number of every id, int64 ``[n]``; ids never seen are inserted and their rows initialised; -1
    where the table is full, for id == INT64_MIN and, on an expiring table, for id == INT64_MIN + 1 (these count
    in :meth:`failed` too), and for ids a filter has not admitted yet (counted in :meth:`filtered`)."""
    return hash_translate([self], [ids], insert=True)[0]

  def find(self, ids):
    """Row number of every id or -1; nothing is inserted."""
    return hash_translate([self], [ids], insert=False)[0]

  def size(self):
    """Keys the table holds: inserted so far, less evicted (syncs the host).  After ``keys`` was written from
    outside (a restored checkpoint) call :meth:`recount` first."""
    n = int(self.counts[0].item())
    return n - int(self.stats[0].item()) if self.expiring else n

  def _counters(self):
    """``(inserted, failed, evicted, reused)`` in ONE host read."""
    return _read_counters([self])[0]

  def _live_count(self):
    """:meth:`size` in ONE host read."""
    inserted, _, evicted, _ = self._counters()
    return inserted - evicted

  def failed(self):
    """Id occurrences answered -1 by an inserting call so far because the table was full or the id is a sentinel
    (INT64_MIN; INT64_MIN + 1 on an expiring table); kept by a rehash and by :meth:`compact` (syncs the host)."""
    return int(self.counts[1].item())

  def recount(self):
    """Set the inserted counter from ``keys`` (after a restore of the raw arrays) and clear the failures
    (and, of an expiring table, the evicted / reused counters: ``size()`` is the live keys again)."""
    self.counts[0] = self._live().sum().to(torch.int32)
    self.counts[1] = 0
    if self.expiring:
      self.stats.zero_()
    if self.min_freq:
      self.filter_counts.zero_()

  def items(self):
    """``(keys, rows)`` of the occupied slots, sorted by key: the geometry-free form of the table."""
    occupied = self._live()
    keys = self.keys[occupied]
    order = torch.argsort(keys)
    return keys[order], self.table[occupied][order]

  def load(self, keys, rows):
    """Insert ``keys`` (without initialising) and store ``rows`` as their rows: ``load(*other.items())``
    moves a table into one of any capacity or slab size.  Refuses when a key does not fit.  The admission
    filter is bypassed and the sketch left alone: these are keys a table already admitted.  On an expiring table
    the keys go through the expiring insert, so a loaded key counts as seen now: ``last_seen`` = the current step
    and ``freq`` + 1, for keys the table already held as well (a key loaded with ``last_seen`` 0 would leave with
    the next sweep); ``items()`` does not carry the metadata of the table it came from."""
    self._check_rows_dtype(rows)
    check_ids([keys], [self])
    if tuple(rows.shape) != (keys.numel(), self.dim) or rows.device != self.table.device:
      raise _bad(f'rows must be {_dtype_name(self.dtype)} [{keys.numel()}, {self.dim}] on {self.table.device}')
    slots = _translate([self], [keys], True, None, init=False, plan=_Plan([self], admit=False))[0]
    ok = slots >= 0
    if not bool(ok.all().item()):
      raise _bad(f'load: {int((~ok).sum().item())} of {keys.numel()} keys do not fit: the table is full')
    self.table[slots] = rows
    return slots

  def load_owned(self, keys, rows, world, rank):
    """:meth:`load` of the keys rank ``rank`` of ``world`` owns (:func:`hash_owner`) and their rows: handed the
    concatenated ``items()`` of W ranks on each of W' ranks, the tables are resharded.  Returns the slots of the
    keys loaded."""
    self._check_rows_dtype(rows)   # (as load: before the ids are looked at; load sees the filtered rows)
    check_ids([keys], [self])
    mine = hash_owner(keys, world) == int(rank)
    return self.load(keys[mine], rows[mine])

  def variables(self, name):
    """The raw arrays for ``training.saver.Saver``: they restore into a table of the SAME geometry
    (capacity, slab_size); then :meth:`recount`.  ``items()`` / ``load()`` is the geometry-free form."""
    out = {name + '/keys': self.keys, name + '/embedding_weights': self.table}
    if self.expiring:
      out[name + '/last_seen'] = self.last_seen
      out[name + '/freq'] = self.freq
    if self.min_freq:
      out[name + '/admission_sketch'] = self.sketch
    return out

  # ---- admission filter -------------------------------------------------------------------------------------
  def filtered(self):
    """Id occurrences the filter answered -1 so far (syncs the host)."""
    self._need_filter('filtered')
    return int(self.filter_counts[0].item())

  def estimate(self, ids):
    """The sketch's count of every id, int32 ``[n]``: the min over its cells, restated in torch ops (a test
    and debugging aid, not the hot path).  At least the times the id was counted; ids the table holds are not
    counted."""
    self._need_filter('estimate')
    depth, width = self.sketch.shape
    cells = sketch_cells(ids.to(self.sketch.device), depth, width, self.sketch_seed)
    return torch.gather(self.sketch, 1, cells).min(dim=0).values

  def clear_filter(self):
    """Zero the sketch in place: every id not in the table needs ``min_freq`` sightings again."""
    self._need_filter('clear_filter')
    self.sketch.zero_()

  def age_filter(self):
    """Halve every counter in place (``>>= 1``): old sightings fade.  (:meth:`age_freq` does the same to the
    per-slot ``freq`` of an expiring table.)"""
    self._need_filter('age_filter')
    self.sketch.bitwise_right_shift_(1)

  # ---- expiry -------------------------------------------------------------------------------------------
  def set_step(self, n):
    """The current step, on the device: an in-place fill (capturable; replayed launches see it)."""
    self._need_expiring('set_step')
    self.step.fill_(int(n))

  def age_freq(self, shift=1):
    """Shift every slot's ``freq`` right in place (``>>= shift``; 1 halves it): old popularity fades, as
    :meth:`age_filter` lets old sightings fade in the sketch.  The count saturates at 2^30 and otherwise never
    forgets, so a table bounded with ``order='lfu'`` calls this now and then -- else an id that was hot long ago
    outlives everything newer.  Stream-ordered, no host read (capturable); keys and ``last_seen`` are not touched.
    ``shift`` must be in [1, 30]."""
    self._need_expiring('age_freq')
    shift = int(shift)
    if not 1 <= shift <= 30:
      raise _bad(f'age_freq: shift must be in [1, 30], got {shift}')
    self.freq.bitwise_right_shift_(shift)

  def evict(self, steps_to_live, keep_freq=0, slots=()):
    """One sweep launch (``hbk_hash_evict_n``): a key whose slot was last seen ``steps_to_live`` or more steps
    ago -- and, with ``keep_freq > 0``, was seen fewer than ``keep_freq`` times -- leaves the table; its slot
    becomes a TOMBSTONE that later inserts reuse.  ``slots``: up to 4 ``(tensor, fill_value)`` pairs, the
    optimizer slots (fp32 ``[capacity, d]``), whose rows of the evicted slots are set to ``fill_value``
    (Adagrad: ``initial_accumulator_value``).  Must not run beside a translate of the table on another
    stream.  Returns nothing and does not sync -- unless the table tracks its removals (:meth:`track_removals`):
    the call then copies the key array, compares after the sweep and synchronises the host once, and is refused
    inside a stream capture."""
    hash_evict([self], steps_to_live, keep_freq, [slots])

  def evicted(self):
    """Keys evicted so far (syncs the host)."""
    self._need_expiring('evicted')
    return int(self.stats[0].item())

  def reused(self):
    """Keys stored into a slot an eviction had freed, so far (syncs the host)."""
    self._need_expiring('reused')
    return int(self.stats[1].item())

  def tombstones(self):
    """Slots that hold a TOMBSTONE now (syncs the host)."""
    self._need_expiring('tombstones')
    return int((self.keys == TOMBSTONE_KEY).sum().item())

  # ---- removal by id ------------------------------------------------------------------------------------
  def remove(self, ids, slots=(), store=None):
    """The keys of ``ids`` leave the table (``hbk_hash_remove_n``: a find and an erase launch) exactly as
    :meth:`evict` makes a key leave: the slot becomes a TOMBSTONE that later inserts reuse, ``last_seen`` and
    ``freq`` become 0, the rows of the companions ``slots`` (``(tensor, fill_value)`` pairs as in :meth:`evict`)
    are set to their fill value, the embedding row is left for the next key.  Returns the slot every id held
    before the call, int64 ``[n]`` on the device, -1 for ids the table did not hold -- for every occurrence,
    duplicates included.  ``evicted()`` counts the distinct ids removed and ``size()`` stays right.  Does not
    sync.  Slots handed out earlier for the removed ids are void.  Needs ``expiring=True``: a removed key leaves
    a TOMBSTONE behind, and a plain table has none.

    ``store``: a :class:`HashSpillStore` -- the ids it holds leave it too (``store.discard``); this costs one
    device-to-host copy of the distinct ids, and only in this case.  Must not run beside a translate, a sweep or
    a backward of the table on another stream."""
    if store is not None:
      _check_store(store, self, slots)
    out = hash_remove([self], [ids], [slots])[0]
    if store is not None and len(store):
      store.discard(torch.unique(ids).cpu())
    return out

  def track_removals(self, on=True):
    """Start (or, ``on=False``, stop and forget) recording the keys that leave the table: every call that writes
    TOMBSTONEs -- :meth:`remove`, :meth:`evict`, :meth:`evict_to`, :meth:`spill_to`, :meth:`maybe_evict` and the
    N-table functions behind them -- then adds the keys it took out to a log of device int64 tensors, which
    :meth:`removed_keys` reads and a delta export carries (``HashExport.removed``).  The cost: ``remove`` and
    ``spill_to`` record the keys they already hold; a tracked SWEEP (``evict``, ``evict_to``) copies the key
    array before the call (8 B/slot) and compares after it, with one host synchronisation.  An untracked table
    issues exactly the calls it issued before.  ``rehash``, ``compact`` and ``maybe_grow`` do not touch the log.
    A captured ``remove`` records when it is captured, not when it is replayed; a tracked sweep needs the host and
    is refused inside a stream capture."""
    self._need_expiring('track_removals')
    if not on:
      self._removals = None
    elif self._removals is None:
      self._removals = []

  def removed_keys(self):
    """The sorted distinct keys recorded since :meth:`track_removals` / :meth:`clear_removals` that :meth:`find`
    does not see now, int64 on the device: a key that left and came back is not removed.  Syncs the host."""
    if self._removals is None:
      raise _bad('removed_keys needs track_removals() first')
    dev = self.keys.device
    if not self._removals:
      return torch.zeros(0, dtype=torch.int64, device=dev)
    keys = torch.unique(torch.cat(self._removals))
    keys = keys[(keys != TOMBSTONE_KEY) & (keys != EMPTY_KEY)]
    self._removals = [keys]   # (the log stays as long as its distinct keys)
    if keys.numel() == 0:
      return keys
    return keys[self.find(keys.contiguous()) < 0]

  def clear_removals(self):
    """Forget the recorded keys (after the delta that carried them was saved); tracking stays on."""
    if self._removals is None:
      raise _bad('clear_removals needs track_removals() first')
    self._removals = []

  def compact(self, slots=()):
    """Rebuild the table in place: every live key is inserted again into an all-EMPTY key array, so every
    TOMBSTONE becomes EMPTY and probes get short again.  Rows, ``last_seen``, ``freq`` and the rows of the
    given companion tensors (``(tensor, fill_value)`` pairs as in :meth:`evict`; the rows no key holds
    afterwards are set to ``fill_value``) move with their keys; ``stats`` is reset and ``size()`` stays.
    Slot numbers change.  A rare operation: torch ops and one :meth:`load`, host synchronisations included."""
    self._need_expiring('compact')
    pairs = _companions(self, slots)
    live = self._live().nonzero().flatten()
    keys, rows = self.keys[live], self.table[live]
    seen, freq = self.last_seen[live], self.freq[live]
    moved = [t[live] for t, _ in pairs]
    failed = self.counts[1].clone()
    self.keys.fill_(EMPTY_KEY)
    self.last_seen.zero_()
    self.freq.zero_()
    self.counts.zero_()
    self.stats.zero_()
    for t, value in pairs:
      t.fill_(value)
    new = self.load(keys, rows)
    self.last_seen[new] = seen
    self.freq[new] = freq
    for (t, _), m in zip(pairs, moved):
      t[new] = m
    self.counts[1] = failed

  # ---- growth and device-side compaction -------------------------------------------------------------------
  def rehash(self, capacity=None, slab_size=None, slots=()):
    """Move the table into fresh arrays of ``capacity`` rows in slabs of ``slab_size`` (None: as now) in one
    launch (``hbk_hash_rehash_n``): see :func:`hash_rehash`.  ``t.rehash()`` is :meth:`compact` on the device.
    ``slots``: up to 4 ``(tensor, fill_value)`` companions as in :meth:`evict`.  Returns the new companion
    tensors in order.  Slot numbers and tensor addresses change."""
    return hash_rehash([self], [capacity], [slab_size], [slots])[0]

  def maybe_grow(self, max_load=0.75, factor=2.0, slots=()):
    """Rehash when more than ``max_load`` of the slots are occupied (keys and tombstones: inserted - reused),
    decided from ONE host read of ``counts`` and ``stats``: to the same capacity when the live keys (inserted -
    evicted) are at most ``max_load * capacity / 2`` -- tombstones were the load -- else to ``ceil(capacity *
    factor)``.  Returns None when nothing was done, else the new companion tensors of ``slots`` (see
    :meth:`rehash` for what a rehash invalidates)."""
    max_load, factor = float(max_load), float(factor)
    if not 0.0 < max_load <= 1.0:
      raise _bad(f'max_load must be in (0, 1], got {max_load!r}')
    if not (math.isfinite(factor) and factor > 1.0):
      raise _bad(f'factor must be finite and > 1, got {factor!r}')
    inserted, _, evicted, reused = self._counters()
    occupied, live = inserted - reused, inserted - evicted
    if occupied <= max_load * self.capacity:
      return None
    if live <= max_load * self.capacity / 2:
      return self.rehash(slots=slots)
    return self.rehash(capacity=int(math.ceil(self.capacity * factor)), slots=slots)

  # ---- a size bound ---------------------------------------------------------------------------------------
  def evict_to(self, max_size, keep_freq=0, slots=(), report=None, order='lru'):
    """The oldest keys leave until at most ``max_size`` stay (``hbk_hash_evict_to_n``): with ``need = size() -
    max_size > 0``, every key whose ``last_seen`` is at or below the smallest step that covers ``need`` keys is
    evicted as :meth:`evict` evicts.  Whole steps leave together -- keys last seen at the same step are equally
    old -- so the size afterwards is ``<= max_size`` and undershoots it by less than the keys of one step; there
    is no tie-break and no exact size.  ``keep_freq > 0``: keys seen that often stay whatever their age (the
    table may then stay above the bound).  ``slots``: as in :meth:`evict`.  The step counter is not read.
    Returns the report, int32 ``[4]`` on the device: ``{live_before, need, cut, n_evicted}`` (``report``: a
    preallocated one, for a captured call).  No host read, no sync -- unless the table tracks its removals
    (:meth:`track_removals`): one key-array copy and one host synchronisation then, and no capture.

    ``order='lfu'`` (``hbk_hash_evict_to_lfu_n``): the LEAST FREQUENTLY USED keys leave instead -- the order is the
    pair (``freq``, ``last_seen``), least frequent first, the oldest first among equally frequent keys; keys with
    equal (``freq``, ``last_seen``) leave together, so the undershoot is less than one such class.  The report is
    then int32 ``[8]``: ``{live_before, need, cut_freq, cut_last_seen, n_evicted, 0, 0, 0}``.  See
    :meth:`age_freq`."""
    return hash_evict_to([self], [max_size], keep_freq, [slots], [report], order=order)[0]

  def maybe_evict(self, max_load=0.75, target_load=0.5, keep_freq=0, slots=(), spill=None, order='lru'):
    """The bounded-memory twin of :meth:`maybe_grow`: the capacity never changes.  Decided from ONE host read of
    ``counts`` and ``stats``: nothing (None) while at most ``max_load`` of the slots are occupied (keys and
    tombstones); else, when the live keys exceed ``target_load * capacity``, :meth:`evict_to`
    ``floor(target_load * capacity)`` and ALWAYS a :meth:`rehash` to the same capacity -- the eviction has just
    turned up to ``max_load - target_load`` of the slots into tombstones, and a table full of them translates
    slowly; else (tombstones were the load) the rehash alone.  Returns the new companion tensors of ``slots``
    (see :meth:`rehash` for what a rehash invalidates).  ``spill``: a :class:`HashSpillStore` -- when the call
    evicts it uses :meth:`spill_to` where it used :meth:`evict_to`: the keys that leave go to the store.
    ``order``: ``'lru'`` or ``'lfu'``, which keys leave when it evicts or spills (:meth:`evict_to`)."""
    self._need_expiring('maybe_evict')
    order = _check_order(order)
    max_load, target_load = _check_loads(max_load, target_load)
    if int(keep_freq) < 0:
      raise _bad(f'keep_freq must be >= 0, got {keep_freq}')
    if spill is not None:
      _check_store(spill, self, slots)
    inserted, _, evicted, reused = self._counters()
    occupied, live = inserted - reused, inserted - evicted
    if occupied <= max_load * self.capacity:
      return None
    if live > target_load * self.capacity:
      bound = int(math.floor(target_load * self.capacity))
      if spill is None:
        self.evict_to(bound, keep_freq, slots, order=order)
      else:
        self.spill_to(bound, spill, keep_freq, slots, order=order)
    return self.rehash(slots=slots)

  # ---- a host tier behind the bound -----------------------------------------------------------------------
  def spill_to(self, max_size, store=None, keep_freq=0, slots=(), order='lru'):
    """:meth:`evict_to` that keeps what it evicts (``hbk_hash_evict_to_select_n`` / ``hbk_hash_spill_n``): the
    keys an ``evict_to(max_size, keep_freq)`` would remove are exported -- row, ``last_seen``, ``freq`` and the rows
    of the companions -- and then evicted as :meth:`evict_to` evicts.  ``slots``: ``(tensor, fill_value)`` pairs
    as in :meth:`evict`: the tensor is exported, then reset to the value.  ``store``: a :class:`HashSpillStore`
    that takes the export (``store.put``).  Returns the :class:`HashExport`, on the device, in ascending slot
    order.  Two host reads (the selection's size, the export's count): see :func:`hash_spill`.  ``order``:
    ``'lru'`` or ``'lfu'`` as in :meth:`evict_to` (``hbk_hash_evict_to_lfu_select_n`` / ``hbk_hash_spill_lfu_n``)."""
    self._need_expiring('spill_to')
    order = _check_order(order)
    if store is not None:
      _check_store(store, self, slots)   # (before anything leaves the table)
    exp = hash_spill([self], [max_size], keep_freq, [slots], order=order)[0]
    if store is not None and len(exp):
      store.put(exp)
    return exp

  def fault_in(self, ids, store, slots=()):
    """Bring the keys of ``ids`` that ``store`` holds back into the table, before the translate of the step: a
    :meth:`find`, the distinct missed ids (``torch.unique`` on the device), one device-to-host copy of them,
    ``store.take`` and, if it returned anything, :meth:`import_items` -- rows, ``last_seen``, ``freq`` and the
    companions ``slots`` (the destination tensors, as for :meth:`import_items`) come back as they left.  Nothing
    the store does not hold is inserted: ids never seen are left to the translate that follows, and so is the
    ``last_seen`` stamp (``find`` does not stamp).  The admission filter is bypassed, as by :meth:`import_items`.
    No key is lost: when the table is too full for some of the taken keys they go back into the store before
    the error is raised.  Returns the number of keys restored."""
    self._need_expiring('fault_in')
    _check_store(store, self, [(x, 0.0) for x in slots])
    check_ids([ids], [self])
    found = self.find(ids)
    missed = torch.unique(ids[found < 0]).cpu()
    if missed.numel() == 0 or len(store) == 0:
      return 0
    return _restore(self, store, missed, slots)

  def missing(self, ids):
    """The distinct ids of ``ids`` the table does not hold, a device int64 tensor in the order of their first
    occurrence (:func:`hash_missing` for one table).  The table is not written."""
    return hash_missing([self], [ids])[0]

  # ---- export and import ----------------------------------------------------------------------------------
  def export_items(self, since=None, slots=()):
    """The table in its geometry-free form WITH its state (``hbk_hash_export_n``): a :class:`HashExport` of the
    keys, their rows, an expiring table's ``last_seen`` and ``freq``, and the rows of the companion tensors
    ``slots`` (fp32 ``[capacity, d]`` tensors: the optimizer slots), in ascending slot order.  ``since`` (expiring
    tables only): the keys with ``last_seen >= since`` -- a delta.  See :func:`hash_export`."""
    return hash_export([self], [since], [slots])[0]

  def import_items(self, exp, slots=(), world=None, rank=None, assume_distinct=False):
    """Upsert a :class:`HashExport`: a key the table holds keeps its slot and takes the imported payload, a new
    key is inserted by the table's own rule (the filter bypassed and the sketch left alone, tombstones of an
    expiring table reused, as :meth:`load`), then rows, metadata and companions are stored in ONE launch
    (``hbk_hash_store_rows_n``).  Returns the slots of the keys imported.

    ``slots``: the destination companions, fp32 ``[capacity, d]``, matching ``exp.slots`` in number and width;
    each entry a tensor or a ``(tensor, fill_value)`` pair.  An export with a non-empty ``removed`` (a delta of a
    tracking table) first removes those keys (:meth:`remove`; owner-filtered under ``world`` / ``rank``), then
    upserts: a removal resets the companion rows of the slots it frees, so such an import needs the pairs and is
    refused with bare tensors.
    ``world`` / ``rank``: only the keys rank ``rank`` of ``world`` owns are imported (:func:`hash_owner`).
    An export with metadata restores ``last_seen`` and ``freq`` on an expiring table (the key keeps its age and
    count); one without leaves :meth:`load`'s "seen now" stamp; a plain table drops the metadata.  The keys must
    be distinct: checked by a sort and a neighbour compare (one host read) unless ``assume_distinct``.  When some
    keys do not fit, the keys that did are stored completely and then the call raises, naming the count."""
    if not isinstance(exp, HashExport):
      raise _bad('import_items needs a HashExport')
    dev = self.keys.device
    removed = getattr(exp, 'removed', None)
    if removed is not None and (not isinstance(removed, torch.Tensor) or removed.dtype != torch.int64 or
                                removed.dim() != 1):
      raise _bad('import_items: exp.removed must be an int64 vector')
    removing = removed is not None and removed.numel() > 0
    slots = list(slots)
    paired = [isinstance(p, (tuple, list)) for p in slots]
    if removing:
      if not self.expiring:
        raise _bad('import_items: the export names removed keys, and removing needs a table built with '
                   'expiring=True')
      if not all(paired):
        raise _bad('import_items: the export names removed keys, and a removal resets the companion rows of the '
                   'slots it frees: slots must be (tensor, fill_value) pairs, got bare tensors')
    pairs = _companions(self, [p if is_pair else (p, 0.0) for p, is_pair in zip(slots, paired)])
    dst_slots = [t for t, _ in pairs]
    if len(dst_slots) != len(exp.slots):
      raise _bad(f'import_items: the export carries {len(exp.slots)} companion tensors, slots names {len(dst_slots)}')
    n = exp.keys.numel()
    if exp.keys.dtype != torch.int64 or exp.keys.dim() != 1:
      raise _bad('import_items: exp.keys must be an int64 vector')
    if exp.rows.dtype != self.dtype or tuple(exp.rows.shape) != (n, self.dim):
      raise _bad(f'import_items: exp.rows must be {_dtype_name(self.dtype)} [{n}, {self.dim}], the table\'s own '
                 f'dtype (nothing is cast), got {exp.rows.dtype} {tuple(exp.rows.shape)}')
    for k, (x, y) in enumerate(zip(exp.slots, dst_slots)):
      if x.dtype != torch.float32 or x.dim() != 2 or tuple(x.shape) != (n, y.shape[1]):
        raise _bad(f'import_items: exp.slots[{k}] must be fp32 [{n}, {y.shape[1]}], got {tuple(x.shape)}')
    meta = self.expiring and exp.last_seen is not None and exp.freq is not None
    if meta:
      for name in ('last_seen', 'freq'):
        x = getattr(exp, name)
        if x.dtype != torch.int32 or tuple(x.shape) != (n,):
          raise _bad(f'import_items: exp.{name} must be int32 [{n}]')
    if (world is None) != (rank is None):
      raise _bad('import_items: world and rank come together')
    src = [exp.rows] + ([exp.last_seen, exp.freq] if meta else []) + list(exp.slots)
    dst = [self.table] + ([self.last_seen, self.freq] if meta else []) + dst_slots
    keys = exp.keys.to(dev)
    src = [x.to(dev) for x in src]
    if world is not None:
      mine = (hash_owner(keys, world) == int(rank)).nonzero().flatten()
      keys = keys[mine]
      src = [x[mine] for x in src]
    keys = keys.contiguous()
    if keys.numel():   # (the checks of the upsert, before anything is removed: a refusal leaves the table as it was)
      if not assume_distinct:
        ordered = torch.sort(keys).values
        if bool((ordered[1:] == ordered[:-1]).any().item()):
          raise _bad('import_items: the keys are not distinct')
      check_ids([keys], [self])
      for x in src:
        if x.stride(-1) != 1:
          raise _bad('import_items: the export\'s rows must be contiguous')
    if removing:
      # every argument is checked: what left the saved table since its base leaves this one first (the owned keys;
      # the others are not here)
      gone = removed.to(dev)
      if world is not None:
        gone = gone[hash_owner(gone, world) == int(rank)]
      if gone.numel():
        hash_remove([self], [gone.contiguous()], [pairs])
    if keys.numel() == 0:
      return keys.new_empty(0)
    got = _translate([self], [keys], True, None, init=False, plan=_Plan([self], admit=False))[0]
    col = (_lib.HashStoreColumn * 1)()
    col[0].slots, col[0].n, col[0].dst_rows = got.data_ptr(), keys.numel(), self.capacity
    col[0].n_moves = len(src)
    for m, (x, y) in enumerate(zip(src, dst)):
      _describe_move(col[0].moves[m], per_slot=y, packed=x, to_packed=False)
    _lib.check(_lib.lib().hbk_hash_store_rows_n(1, col, _lib.current_stream(dev)))
    missing = int((got < 0).sum().item())
    if missing:
      raise _bad(f'import_items: {missing} of {keys.numel()} keys do not fit: the table is full (the others are '
                 'stored)')
    return got


def _companions(table, slots):
  """Checked ``(tensor, fill_value)`` pairs of one table."""
  pairs = [tuple(p) for p in slots]
  if len(pairs) > _lib.HASH_MAX_FILLS:
    raise _bad(f'at most {_lib.HASH_MAX_FILLS} companion tensors per table, got {len(pairs)}')
  out = []
  for n, p in enumerate(pairs):
    if len(p) != 2 or not isinstance(p[0], torch.Tensor):
      raise _bad(f'slots[{n}] must be a (tensor, fill_value) pair')
    t, value = p[0], float(p[1])
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != table.capacity or t.shape[1] < 1 or \
        t.device != table.keys.device:
      raise _bad(f'slots[{n}]: the tensor must be fp32 [{table.capacity}, d] on {table.keys.device}')
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
      raise _bad(f'slots[{n}]: the tensor\'s rows must be contiguous')
    if not math.isfinite(value) or not math.isfinite(C.c_float(value).value):
      raise _bad(f'slots[{n}]: fill_value must be finite, got {p[1]!r}')
    out.append((t, value))
  return out


def _plain_companions(table, slots):
  """Checked companion tensors of one table, without fill values (an export and an import fill nothing)."""
  return [t for t, _ in _companions(table, [(x, 0.0) for x in slots])]


def _dtype_name(dtype):
  return 'fp32' if dtype == torch.float32 else str(dtype)


def _words(x, elements):
  """``elements`` elements of ``x`` in 4-byte words: rows travel as words, bit for bit, whatever they hold (a 16-bit
  row of even dim is dim / 2 words; its pitch is even too)."""
  nbytes = elements * x.element_size()
  if nbytes % 4:
    raise _bad(f'a row of {elements} {x.dtype} elements is no whole number of 4-byte words')
  return nbytes // 4


def _describe_move(mv, per_slot, packed, to_packed):
  """One hbk_hash_move_t between a per-slot array of a table and a packed array of an export: a vector of 4-byte
  elements, or a matrix of any element size described in 4-byte words."""
  src, dst = (per_slot, packed) if to_packed else (packed, per_slot)
  mv.src, mv.dst = src.data_ptr(), dst.data_ptr()
  mv.words = 1 if per_slot.dim() == 1 else _words(per_slot, per_slot.shape[1])
  mv.src_pitch = 1 if src.dim() == 1 else _words(src, src.stride(0))
  mv.dst_pitch = 1 if dst.dim() == 1 else _words(dst, dst.stride(0))


class HashExport:
  """What :meth:`HashTable.export_items` returns and :meth:`HashTable.import_items` takes: the keys of a table
  (all of them, or a delta) with everything that belongs to them, independent of the table's geometry.

  Attributes: ``keys`` int64 ``[n]``; ``rows`` ``[n, dim]`` in the table's dtype; ``last_seen`` / ``freq`` int32 ``[n]``
  (None
  for a table that is not expiring); ``slots``: a list of fp32 ``[n, d]`` tensors, one per companion; ``src_slots``
  int64 ``[n]``: the slot every key had in the table it came from (ascending: the order of the export); ``since``:
  the ``since`` of the export, 0 for a full one; ``removed``: int64 ``[m]`` ascending, the keys that left the
  table since tracking began or was cleared and are not in it now (a table with :meth:`HashTable.track_removals`
  on: :meth:`HashTable.removed_keys` for a delta, empty for a full export), or None for a table that does not
  track."""

  def __init__(self, keys, rows, last_seen=None, freq=None, slots=(), src_slots=None, since=0, removed=None):
    self.keys, self.rows, self.last_seen, self.freq = keys, rows, last_seen, freq
    self.slots = list(slots)
    self.src_slots = src_slots
    self.since = int(since)
    self.removed = removed

  def __len__(self):
    return self.keys.numel()

  def variables(self, name):
    """The flat ``{name + '/items/...': tensor}`` dict ``training.saver.Saver.save`` takes (``since`` as an int64
    ``[1]`` tensor)."""
    base = name + '/items/'
    out = {base + 'keys': self.keys, base + 'rows': self.rows,
           base + 'since': torch.tensor([self.since], dtype=torch.int64)}
    if self.last_seen is not None and self.freq is not None:
      out[base + 'last_seen'] = self.last_seen
      out[base + 'freq'] = self.freq
    if self.src_slots is not None:
      out[base + 'src_slots'] = self.src_slots
    for k, x in enumerate(self.slots):
      out[base + f'slot{k}'] = x
    if self.removed is not None:
      out[base + 'removed'] = self.removed
    return out

  @classmethod
  def from_variables(cls, name, d):
    """The export a :meth:`variables` dict describes (the tensors themselves, not copies: restore into them with
    ``Saver.restore`` first, or hand over the dict that was saved)."""
    base = name + '/items/'
    if base + 'keys' not in d or base + 'rows' not in d:
      raise _bad(f'from_variables: {base}keys and {base}rows are needed')
    slots = []
    while base + f'slot{len(slots)}' in d:
      slots.append(d[base + f'slot{len(slots)}'])
    since = d.get(base + 'since')
    return cls(d[base + 'keys'], d[base + 'rows'], d.get(base + 'last_seen'), d.get(base + 'freq'), slots,
               d.get(base + 'src_slots'), 0 if since is None else int(since.reshape(-1)[0].item()),
               d.get(base + 'removed'))

  @classmethod
  def empty(cls, n, dim, expiring=False, slot_dims=(), device='cpu', n_removed=None, dtype=torch.float32):
    """An export of ``n`` zero keys: the tensors a ``Saver.restore`` of a saved export is read into.  ``n_removed``:
    None, or the length of ``removed``.  ``dtype``: of ``rows``, the table's."""
    n = int(n)
    meta = [torch.zeros(n, dtype=torch.int32, device=device) for _ in range(2)] if expiring else [None, None]
    return cls(torch.zeros(n, dtype=torch.int64, device=device),
               torch.zeros((n, int(dim)), dtype=dtype, device=device),
               meta[0], meta[1], [torch.zeros((n, int(d)), device=device) for d in slot_dims],
               torch.zeros(n, dtype=torch.int64, device=device), 0,
               None if n_removed is None else torch.zeros(int(n_removed), dtype=torch.int64, device=device))

  @classmethod
  def cat(cls, exports):
    """The exports of several ranks (or a table's parts) as one: concatenated in order.  The metadata stays only
    when every part has it, and so does ``removed`` (the parts' keys as one ascending distinct list); ``since`` is
    the smallest of the parts'."""
    exports = list(exports)
    if not exports:
      raise _bad('cat: no exports')
    if len(set(len(e.slots) for e in exports)) != 1:
      raise _bad('cat: the exports differ in their number of companion tensors')
    meta = all(e.last_seen is not None and e.freq is not None for e in exports)
    src = all(e.src_slots is not None for e in exports)
    gone = all(e.removed is not None for e in exports)
    return cls(torch.cat([e.keys for e in exports]), torch.cat([e.rows for e in exports]),
               torch.cat([e.last_seen for e in exports]) if meta else None,
               torch.cat([e.freq for e in exports]) if meta else None,
               [torch.cat([e.slots[k] for e in exports]) for k in range(len(exports[0].slots))],
               torch.cat([e.src_slots for e in exports]) if src else None, min(e.since for e in exports),
               torch.unique(torch.cat([e.removed for e in exports])) if gone else None)


def hash_export(tables, sinces=None, slots=None):
  """:meth:`HashTable.export_items` for N tables of any kinds in ONE C call (``hbk_hash_export_n``: a count, a
  scan and a write launch per 32 tables, no atomics, the keys in ascending slot order -- the result is a function
  of the tables' arrays alone).

  ``sinces[c]``: None for every key of table c, else an int: the keys with ``last_seen >= since`` (refused on a
  table that is not expiring).  ``slots[c]``: its companion tensors, fp32 ``[capacity, d]`` (the optimizer slots;
  no fill value is needed here).  Returns one :class:`HashExport` per table.

  The outputs are allocated from ONE host read of the counters (the live keys: an upper bound for a delta), the
  launches run, ONE host read of the counts follows and the outputs are narrowed to views.  More matches than the
  counters promised is refused: the counters are stale after a restore of the raw arrays -- :meth:`recount`.
  A table that tracks its removals (:meth:`HashTable.track_removals`) also gets ``removed``:
  :meth:`HashTable.removed_keys` for a delta (a find and one more host read), an empty tensor for a full export.
  Must not run beside a translate, a sweep or a backward of the same tables on another stream."""
  tables = list(tables)
  same_device(tables)
  n = len(tables)
  sinces, slots = _per_table(n, ('since values', sinces, None), ('lists of companion tensors', slots, ()))
  if n == 0:
    _lib.check(_lib.lib().hbk_hash_export_n(0, None, None, None))
    return []
  checked = []
  for c, t in enumerate(tables):
    if sinces[c] is not None:
      if not t.expiring:
        raise _bad(f'table {c}: since needs a table built with expiring=True (last_seen is the dirty mark)')
      if not -2 ** 31 <= int(sinces[c]) < 2 ** 31:
        raise _bad(f'table {c}: since must be an int32, got {sinces[c]}')
    checked.append(_plain_companions(t, slots[c]))
  for t in tables:
    _lib.require_device_tensor(t.keys, 'keys')
  dev = tables[0].keys.device
  # the live keys of every table in one host read
  counters = _read_counters(tables)
  cols = (_lib.HashExportColumn * n)()
  counts = torch.zeros(n, dtype=torch.int64, device=dev)
  outs = []
  for c, t in enumerate(tables):
    inserted, _, evicted, _ = counters[c]
    live = inserted - evicted
    cap = min(max(live, 0), t.capacity)
    rows = max(cap, 1)   # (never an empty allocation: a move needs an address)
    out = {'keys': torch.empty(rows, dtype=torch.int64, device=dev),
           'src_slots': torch.empty(rows, dtype=torch.int64, device=dev),
           'rows': torch.empty((rows, t.dim), dtype=t.dtype, device=dev)}
    moves = [(t.table, out['rows'])]
    if t.expiring:
      for name in ('last_seen', 'freq'):
        out[name] = torch.empty(rows, dtype=torch.int32, device=dev)
        moves.append((getattr(t, name), out[name]))
    out['slots'] = [torch.empty((rows, x.shape[1]), dtype=torch.float32, device=dev) for x in checked[c]]
    moves += list(zip(checked[c], out['slots']))
    col = cols[c]
    col.keys, col.slab_count, col.slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
    col.expiring = 1 if t.expiring else 0
    col.last_seen = t.last_seen.data_ptr() if t.expiring else None
    col.since = 0 if sinces[c] is None else max(int(sinces[c]), 0)
    col.n_moves = len(moves)
    for m, (x, y) in enumerate(moves):
      _describe_move(col.moves[m], per_slot=x, packed=y, to_packed=True)
    col.out_keys, col.out_slots, col.out_capacity = out['keys'].data_ptr(), out['src_slots'].data_ptr(), cap
    col.count = counts.data_ptr() + 8 * c
    outs.append((out, cap))
  lib = _lib.lib()
  nbytes = C.c_size_t()
  _lib.check(lib.hbk_hash_export_workspace_bytes(n, cols, C.byref(nbytes)))
  workspace = torch.empty(max(nbytes.value // 8, 1), dtype=torch.int64, device=dev)
  _lib.check(lib.hbk_hash_export_n(n, cols, workspace.data_ptr(), _lib.current_stream(dev)))
  result = []
  for c, (k, (out, cap)) in enumerate(zip(counts.tolist(), outs)):
    if k > cap:
      raise _bad(f'table {c}: {k} keys match but the counters promise {cap}: they are stale (a restore of the raw '
                 'arrays?) -- call recount() first')
    result.append(HashExport(out['keys'][:k], out['rows'][:k], out['last_seen'][:k] if tables[c].expiring else None,
                             out['freq'][:k] if tables[c].expiring else None, [x[:k] for x in out['slots']],
                             out['src_slots'][:k], 0 if sinces[c] is None else max(int(sinces[c]), 0)))
  for c, t in enumerate(tables):
    if t._removals is not None:
      result[c].removed = t.removed_keys() if sinces[c] is not None else torch.zeros(0, dtype=torch.int64, device=dev)
  return result


def hash_owner(ids, world):
  """The rank that owns every id of a sharded hash table: ``floormod(id, world)`` (what the sharded step's
  partition computes: negative ids have an owner), as a tensor op."""
  world = int(world)
  if world < 1:
    raise _bad(f'world must be >= 1, got {world}')
  return torch.remainder(ids, world)


def hash_rehash(tables, capacities=None, slab_sizes=None, slots=None):
  """Growth and compaction of N tables (plain, expiring and filtered ones may be mixed) in ONE launch
  (``hbk_hash_rehash_n``): every live key is placed into a fresh all-EMPTY key array by the plain placement rule
  and its rows move with it -- ``table``, an expiring table's ``last_seen`` and ``freq``, and the companions.

  ``capacities[c]`` / ``slab_sizes[c]``: the new geometry of table c (None: as now; the capacity is rounded down
  to whole slabs); ``slots[c]``: its ``(tensor, fill_value)`` companions as in :meth:`HashTable.evict`.  The call
  allocates the new arrays (``keys`` all EMPTY, ``table`` zeros, ``last_seen`` / ``freq`` zeros, one ``[capacity,
  d]`` tensor per companion filled with its ``fill_value``), launches, and replaces the tables' attributes;
  ``capacity``, ``slab_count`` and ``slab_size`` follow.  Returns, per table, the list of its new companion
  tensors in order.

  Counters (new tensors too, swapped in with the arrays, so a refused call leaves the table and its counters as
  they were): ``counts[0]`` becomes the keys moved, ``counts[1]`` (failed) is kept; an expiring table's ``stats``
  is zeroed (``tombstones()``, ``evicted()`` and ``reused()`` read 0, ``size()`` is unchanged), ``step`` is kept;
  a filtered table's sketch, ``filter_counts``, ``min_freq`` and seeds are untouched.

  No host synchronisation when no table shrinks (every live key then fits: the walk covers all slabs).  A
  smaller capacity reads ``size()`` -- one sync -- and is refused before anything changes when the keys do not
  fit.

  Slot numbers and tensor addresses change: slots handed out before are void, a :class:`HashGroupLookup` over
  the tables needs :meth:`HashGroupLookup.rebind`, a ``GroupLookupGrad`` built on the old ``hgl.lookup`` must be
  rebuilt with the new slot tensors, and a captured graph must be captured again.  Must not run beside a
  translate or a sweep of the same tables on another stream."""
  tables = list(tables)
  same_device(tables)
  n = len(tables)
  capacities, slab_sizes, slots = _per_table(n, ('capacities', capacities, None), ('slab sizes', slab_sizes, None),
                                             ('lists of companion tensors', slots, ()))
  if len(set(id(t) for t in tables)) != n:
    raise _bad('a table is named twice')
  if n == 0:
    _lib.check(_lib.lib().hbk_hash_rehash_n(0, None, None))
    return []
  geometry, checked = [], []
  for c, t in enumerate(tables):
    slab_size = t.slab_size if slab_sizes[c] is None else int(slab_sizes[c])
    capacity = t.capacity if capacities[c] is None else int(capacities[c])
    _check_geometry(capacity, slab_size, f'table {c}: ')
    geometry.append((capacity // slab_size, slab_size))
    checked.append(_companions(t, slots[c]))
  for c, t in enumerate(tables):
    _lib.require_device_tensor(t.keys, 'keys')
    capacity = geometry[c][0] * geometry[c][1]
    if capacity < t.capacity:
      live = t._live_count()   # (the one sync of a shrink)
      if live > capacity:
        raise _bad(f'table {c}: {live} keys do not fit into {capacity} slots')
  cols = (_lib.HashRehashColumn * n)()
  fresh = []
  for c, t in enumerate(tables):
    slab_count, slab_size = geometry[c]
    capacity, dev = slab_count * slab_size, t.keys.device
    new = {'keys': torch.full((capacity,), EMPTY_KEY, dtype=torch.int64, device=dev),
           'table': torch.zeros((capacity, t.dim), dtype=t.dtype, device=dev)}
    moves = [(t.table, new['table'])]
    if t.expiring:
      for name in ('last_seen', 'freq'):
        new[name] = torch.zeros(capacity, dtype=torch.int32, device=dev)
        moves.append((getattr(t, name), new[name]))
    companions = [torch.full((capacity, x.shape[1]), value, dtype=torch.float32, device=dev) for x, value in checked[c]]
    moves += [(x, y) for (x, _), y in zip(checked[c], companions)]
    col = cols[c]
    col.src_keys, col.src_slab_count, col.src_slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
    col.dst_keys, col.dst_slab_count, col.dst_slab_size = new['keys'].data_ptr(), slab_count, slab_size
    col.expiring = 1 if t.expiring else 0
    col.n_moves = len(moves)
    for m, (src, dst) in enumerate(moves):
      _describe_move(col.moves[m], per_slot=src, packed=dst, to_packed=True)
    col.new_slots = None
    # a fresh counter pair: {0, the failures so far}; the kernel adds the keys it moved.  It is swapped in with
    # the other new arrays, so a refused launch leaves the table and its counters as they were
    new['counts'] = t.counts.clone()
    new['counts'][:1].zero_()
    col.counts = new['counts'].data_ptr()
    if t.expiring:
      new['stats'] = torch.zeros(2, dtype=torch.int32, device=dev)
    fresh.append((new, companions))
  _lib.check(_lib.lib().hbk_hash_rehash_n(n, cols, _lib.current_stream(tables[0].keys.device)))
  for t, (slab_count, slab_size), (new, _) in zip(tables, geometry, fresh):
    for name, x in new.items():
      setattr(t, name, x)
    t.slab_count, t.slab_size, t.capacity = slab_count, slab_size, slab_count * slab_size
  return [companions for _, companions in fresh]


def hash_evict(tables, steps_to_live, keep_freq=0, slots=None):
  """:meth:`HashTable.evict` for N expiring tables in ONE launch.  ``slots[c]``: the ``(tensor, fill_value)``
  pairs of table ``c`` (None: no table has any).  Does not sync, unless a table tracks its removals
  (:meth:`HashTable.track_removals`): see :meth:`HashTable.evict`."""
  tables = list(tables)
  cols, _ = _evict_columns(tables, steps_to_live, keep_freq, slots)
  dev = tables[0].keys.device if tables else None
  before = _keys_before(tables)
  _lib.check(_lib.lib().hbk_hash_evict_n(len(tables), cols, _lib.current_stream(dev)))
  _record_swept(tables, before)


def _keys_before(tables):
  """The snapshot a tracked sweep needs (:meth:`HashTable.track_removals`): a copy of the key array of every
  tracking table, None for the others -- and None altogether when no table tracks."""
  if not any(t._removals is not None for t in tables):
    return None
  if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
    raise _bad('a sweep of a table that tracks its removals reads the host (the key array is compared after the '
               'call): it cannot be captured -- track_removals(False) first, or sweep outside the capture')
  return [t.keys.clone() if t._removals is not None else None for t in tables]


def _record_swept(tables, before):
  """The keys a sweep turned into TOMBSTONEs, into the log of every tracking table (one host synchronisation)."""
  if before is None:
    return
  for t, b in zip(tables, before):
    if b is not None:
      t._removals.append(b[(t.keys == TOMBSTONE_KEY) & (b != TOMBSTONE_KEY)])


def _evict_columns(tables, steps_to_live, keep_freq, slots):
  """The checked descriptors of one sweep call (and the tensors they point into)."""
  same_device(tables)
  steps_to_live, keep_freq = int(steps_to_live), int(keep_freq)
  if steps_to_live < 0 or keep_freq < 0:
    raise _bad(f'steps_to_live and keep_freq must be >= 0, got {steps_to_live} and {keep_freq}')
  slots, = _per_table(len(tables), ('lists of companion tensors', slots, ()))
  for t in tables:
    t._need_expiring('evict')
  checked = [_companions(t, slots[c]) for c, t in enumerate(tables)]
  cols = (_lib.HashEvictColumn * len(tables))()
  for c, t in enumerate(tables):
    _lib.require_device_tensor(t.keys, 'keys')
    _describe_sweep(cols[c], t, keep_freq, checked[c])
    cols[c].steps_to_live = steps_to_live
  return cols, checked


def _describe_sweep(col, t, keep_freq, pairs):
  """What the descriptors of both sweeps share: the table, its expiry record, the guard and the fills."""
  col.keys_cache, col.slab_count, col.slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
  t._describe_expiry(col.exp)
  col.keep_freq = keep_freq
  col.n_fills = len(pairs)
  for f, (x, value) in enumerate(pairs):
    col.fills[f].base, col.fills[f].pitch, col.fills[f].dim = x.data_ptr(), x.stride(0), x.shape[1]
    col.fills[f].value = value


_EVICT_TO_WORKSPACES = {}   # (device, n_tables) -> int32 scratch: the same address at every call, so a captured call replays
_EVICT_TO_LFU_WORKSPACES = {}   # the same for order='lfu'
_MAX_SELECT_WORKSPACES = 64     # entries of either: (device, tables, stream) -> scratch, the least recently used leaves
_SELECT_LOCK = threading.Lock()

# order -> (words of a report, the C entries of the sweep, of the select and of the workspace size, the scratch)
_EVICT_TO_ORDERS = {
  'lru': (4, 'hbk_hash_evict_to_n', 'hbk_hash_evict_to_select_n', 'hbk_hash_evict_to_workspace_bytes',
          _EVICT_TO_WORKSPACES),
  'lfu': (8, 'hbk_hash_evict_to_lfu_n', 'hbk_hash_evict_to_lfu_select_n', 'hbk_hash_evict_to_lfu_workspace_bytes',
          _EVICT_TO_LFU_WORKSPACES),
}


def _check_order(order):
  """``'lru'`` or ``'lfu'``; anything else is refused by name."""
  if not isinstance(order, str) or order not in _EVICT_TO_ORDERS:
    raise _bad(f"order must be 'lru' or 'lfu', got {order!r}")
  return order


def hash_evict_to(tables, max_sizes, keep_freq=0, slots=None, reports=None, order='lru'):
  """:meth:`HashTable.evict_to` for N expiring tables in ONE C call (``hbk_hash_evict_to_n``): per table the
  oldest keys leave until at most ``max_sizes[c]`` stay -- the cut is found on the device, three histogram passes
  over ``last_seen`` and a sweep, no host read.  ``max_sizes``: one int for all tables or one per table.
  ``slots[c]``: the ``(tensor, fill_value)`` pairs of table ``c`` as in :func:`hash_evict`.  ``reports[c]``: an
  int32 ``[4]`` device tensor or None (allocated): ``{live_before, need, cut, n_evicted}`` of table c after the
  call.  Returns the list of reports; does not sync.  The scratch tensor is kept per (device, number of tables),
  so a captured call replays.  With a table that tracks its removals (:meth:`HashTable.track_removals`) the call
  copies that table's key array first, compares after the sweep with one host synchronisation, and is refused inside
  a stream capture.

  ``order='lfu'`` (``hbk_hash_evict_to_lfu_n``): the least frequently used keys leave, the oldest first among
  equally frequent ones -- six histogram passes over (``freq``, ``last_seen``) and a sweep.  ``reports[c]`` is then
  int32 ``[8]``: ``{live_before, need, cut_freq, cut_last_seen, n_evicted, 0, 0, 0}``."""
  return _evict_to(tables, max_sizes, keep_freq, slots, reports, 'evict_to', _check_order(order))


def hash_evict_to_select(tables, max_sizes, keep_freq=0, reports=None, order='lru'):
  """The selection of :func:`hash_evict_to` without its sweep (``hbk_hash_evict_to_select_n``): nothing of the
  tables is written.  Returns the reports, int32 ``[4]`` on the device: ``{live_before, need, cut, n_selected}`` --
  ``n_selected`` is the exact number of keys ``hash_evict_to`` with the same arguments would evict.  ``reports``:
  preallocated ones.  No host read, no sync.  ``order='lfu'`` (``hbk_hash_evict_to_lfu_select_n``): int32 ``[8]``,
  ``{live_before, need, cut_freq, cut_last_seen, n_selected, 0, 0, 0}``."""
  return _evict_to(tables, max_sizes, keep_freq, None, reports, 'evict_to_select', _check_order(order))


def _evict_to(tables, max_sizes, keep_freq, slots, reports, what, order):
  """Both entries of the select, in either order: ``what`` names the call in a refusal and picks the C entry."""
  words, sweep_entry, select_entry, size_entry, workspaces = _EVICT_TO_ORDERS[order]
  entry = sweep_entry if what == 'evict_to' else select_entry
  tables = list(tables)
  same_device(tables)
  n = len(tables)
  keep_freq = int(keep_freq)
  if not isinstance(max_sizes, (list, tuple)):
    max_sizes = [max_sizes] * n
  max_sizes, slots, reports = _per_table(n, ('max_sizes', max_sizes, 0), ('lists of companion tensors', slots, ()),
                                         ('reports', reports, None))
  max_sizes = [int(m) for m in max_sizes]
  if any(m < 0 for m in max_sizes) or keep_freq < 0:
    raise _bad(f'max_size and keep_freq must be >= 0, got {min(max_sizes + [0])} and {keep_freq}')
  for t in tables:
    t._need_expiring(what)
  checked = [_companions(t, slots[c]) for c, t in enumerate(tables)]
  lib = _lib.lib()
  call = getattr(lib, entry)
  if n == 0:
    _lib.check(call(0, None, None, 0, None))
    return []
  dev = tables[0].keys.device
  cols = (_lib.HashEvictToColumn * n)()
  for c, r in enumerate(reports):
    if r is not None and (not isinstance(r, torch.Tensor) or r.dtype != torch.int32 or tuple(r.shape) != (words,) or
                          r.device != dev or not r.is_contiguous()):
      raise _bad(f'reports[{c}] must be a contiguous int32 [{words}] tensor on {dev}')
  for c, t in enumerate(tables):
    _lib.require_device_tensor(t.keys, 'keys')
    if reports[c] is None:
      reports[c] = torch.zeros(words, dtype=torch.int32, device=dev)
    _describe_sweep(cols[c], t, keep_freq, checked[c])
    cols[c].max_size = max_sizes[c]
    cols[c].report = reports[c].data_ptr()
  nbytes = getattr(lib, size_entry)(n)
  # (kept per stream: two streams of one process -- the ranks of an in-process world -- select side by side; at
  # most _MAX_SELECT_WORKSPACES entries, the oldest leaves: a process that makes streams as it goes does not grow it)
  slot = (dev, n, torch.cuda.current_stream(dev).cuda_stream)
  with _SELECT_LOCK:
    workspace = workspaces.pop(slot, None)
    if workspace is None or workspace.numel() * 4 < nbytes:
      workspace = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
    workspaces[slot] = workspace                 # (the newest entry: dicts keep insertion order)
    while len(workspaces) > _MAX_SELECT_WORKSPACES:
      workspaces.pop(next(iter(workspaces)))
  before = _keys_before(tables) if what == 'evict_to' else None   # (the select writes nothing)
  _lib.check(call(n, cols, workspace.data_ptr(), workspace.numel() * 4, _lib.current_stream(dev)))
  _record_swept(tables, before)
  return reports


def hash_spill(tables, max_sizes, keep_freq=0, slots=None, order='lru'):
  """:meth:`HashTable.spill_to` for N expiring tables: the keys :func:`hash_evict_to` with the same arguments would
  evict leave the tables WITH their payload.  Returns one :class:`HashExport` per table, on the device, in ascending
  slot order: keys, rows, ``last_seen``, ``freq`` and the rows of the companions as they were before the call.

  ``slots[c]``: the ``(tensor, fill_value)`` pairs of table c as in :func:`hash_evict`: the tensor is exported,
  then its evicted rows are reset to the value.

  The steps: the select (:func:`hash_evict_to_select`); ONE host read of all reports; outputs allocated for exactly
  ``n_selected`` keys per table; ``hbk_hash_spill_n`` -- count, scan and write of the export with the eviction's
  predicate, then the sweep, which leaves a table alone whose selected keys do not all fit the output; ONE host
  read of the counts, and a count that differs from its ``n_selected`` is refused (somebody wrote the table between
  the two calls; a table with more keys than promised was not touched).  Must not run beside a translate, a sweep
  or a backward of the same tables on another stream.

  ``order='lfu'``: the keys ``hash_evict_to(..., order='lfu')`` would evict -- the select and the spill are then
  ``hbk_hash_evict_to_lfu_select_n`` and ``hbk_hash_spill_lfu_n``; the steps and the host reads are the same."""
  order = _check_order(order)
  lfu = order == 'lfu'
  tables = list(tables)
  same_device(tables)
  n = len(tables)
  keep_freq = int(keep_freq)
  slots, = _per_table(n, ('lists of companion tensors', slots, ()))
  for t in tables:
    t._need_expiring('spill_to')
  checked = [_companions(t, slots[c]) for c, t in enumerate(tables)]
  reports = hash_evict_to_select(tables, max_sizes, keep_freq, order=order)
  lib = _lib.lib()
  spill = lib.hbk_hash_spill_lfu_n if lfu else lib.hbk_hash_spill_n
  if n == 0:
    _lib.check(spill(0, None, None, None))
    return []
  dev = tables[0].keys.device
  selected = [r[4 if lfu else 3] for r in torch.stack(reports).tolist()]   # the one host read of the selection
  cols = (_lib.HashSpillColumn * n)()
  counts = torch.zeros(n, dtype=torch.int64, device=dev)
  n_evicted = torch.zeros(n, dtype=torch.int32, device=dev)
  outs = []
  for c, t in enumerate(tables):
    cap = selected[c]
    rows = max(cap, 1)   # (never an empty allocation: a move needs an address)
    out = {'keys': torch.empty(rows, dtype=torch.int64, device=dev),
           'src_slots': torch.empty(rows, dtype=torch.int64, device=dev),
           'rows': torch.empty((rows, t.dim), dtype=t.dtype, device=dev),
           'last_seen': torch.empty(rows, dtype=torch.int32, device=dev),
           'freq': torch.empty(rows, dtype=torch.int32, device=dev),
           'slots': [torch.empty((rows, x.shape[1]), dtype=torch.float32, device=dev) for x, _ in checked[c]]}
    moves = [(t.table, out['rows']), (t.last_seen, out['last_seen']), (t.freq, out['freq'])]
    moves += [(x, y) for (x, _), y in zip(checked[c], out['slots'])]
    col = cols[c]
    _describe_sweep(col, t, keep_freq, checked[c])
    col.selection = reports[c].data_ptr()
    col.n_moves = len(moves)
    for m, (x, y) in enumerate(moves):
      _describe_move(col.moves[m], per_slot=x, packed=y, to_packed=True)
    col.out_keys, col.out_slots, col.out_capacity = out['keys'].data_ptr(), out['src_slots'].data_ptr(), cap
    col.count = counts.data_ptr() + 8 * c
    col.n_evicted = n_evicted.data_ptr() + 4 * c
    outs.append(out)
  nbytes = C.c_size_t()
  _lib.check(lib.hbk_hash_spill_workspace_bytes(n, cols, C.byref(nbytes)))
  workspace = torch.empty(max(nbytes.value // 8, 1), dtype=torch.int64, device=dev)
  _lib.check(spill(n, cols, workspace.data_ptr(), _lib.current_stream(dev)))
  result = []
  for c, (k, out) in enumerate(zip(counts.tolist(), outs)):
    if k != selected[c]:
      raise _bad(f'table {c}: the select promised {selected[c]} keys and the spill counted {k}: the table was '
                 'written between the two' + (' (it was left untouched)' if k > selected[c] else ''))
    result.append(HashExport(out['keys'][:k], out['rows'][:k], out['last_seen'][:k], out['freq'][:k],
                             [x[:k] for x in out['slots']], out['src_slots'][:k], 0))
  for t, exp in zip(tables, result):
    if t._removals is not None and len(exp):
      t._removals.append(exp.keys.clone())   # what left is what was exported
  return result


def hash_remove(tables, ids_list, slots=None, outs=None):
  """:meth:`HashTable.remove` for N expiring tables in ONE C call (``hbk_hash_remove_n``: a find and an erase
  launch per 32 tables).  ``ids_list[c]``: the int64 ids to take out of table c (duplicates, absent ids and the
  sentinels are fine); ``slots[c]``: its ``(tensor, fill_value)`` companions as in :func:`hash_evict`; ``outs[c]``:
  a preallocated int64 ``[n_ids]`` tensor or None.  Returns, per table, the slot every id held before the call or
  -1.  The tables' arrays, their counters and the answers are functions of the inputs alone.  No workspace, no host
  read, no sync: capturable -- a captured call removes, at every replay, whatever the id buffers then hold."""
  tables = list(tables)
  same_device(tables)
  n = len(tables)
  ids_list = list(ids_list)
  slots, outs = _per_table(n, ('lists of companion tensors', slots, ()), ('outputs', outs, None))
  for c, t in enumerate(tables):
    if not t.expiring:
      raise _bad(f'table {c}: remove needs a table built with expiring=True: a removed key leaves a TOMBSTONE '
                 'behind, and a plain table has none (INT64_MIN + 1 is an ordinary key there)')
  checked = [_companions(t, slots[c]) for c, t in enumerate(tables)]
  check_ids(ids_list, tables)
  if n == 0:
    _lib.check(_lib.lib().hbk_hash_remove_n(0, None, None))
    return []
  dev = tables[0].keys.device
  cols = (_lib.HashRemoveColumn * n)()
  for c, (t, i) in enumerate(zip(tables, ids_list)):
    _lib.require_device_tensor(t.keys, 'keys')
    if outs[c] is None:
      outs[c] = torch.empty(i.numel(), dtype=torch.int64, device=dev)
    o = outs[c]
    if not isinstance(o, torch.Tensor) or o.dtype != torch.int64 or tuple(o.shape) != (i.numel(),) or \
        o.device != i.device or not o.is_contiguous():
      raise _bad(f'output {c} must be a contiguous int64 [{i.numel()}] tensor on {i.device}')
    col = cols[c]
    col.keys_cache, col.slab_count, col.slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
    t._describe_expiry(col.exp)
    col.keys, col.n_keys, col.slots = i.data_ptr(), i.numel(), o.data_ptr()
    col.n_removed = None
    col.n_fills = len(checked[c])
    for f, (x, value) in enumerate(checked[c]):
      col.fills[f].base, col.fills[f].pitch, col.fills[f].dim = x.data_ptr(), x.stride(0), x.shape[1]
      col.fills[f].value = value
  _lib.check(_lib.lib().hbk_hash_remove_n(n, cols, _lib.current_stream(dev)))
  for t, i, o in zip(tables, ids_list, outs):
    if t._removals is not None and i.numel():
      t._removals.append(torch.where(o >= 0, i, TOMBSTONE_KEY))   # (no sync; removed_keys drops the sentinel)
  return outs


def remove_tables(tables, ids_list, slots, stores):
  """:func:`hash_remove` over the tables of a lookup object, and ``stores[c].discard`` where a store is named."""
  if isinstance(stores, HashSpillStore):
    stores = [stores]
  ids_list = list(ids_list)
  slots, stores = _per_table(len(tables), ('lists of companion tensors', slots, ()), ('spill stores', stores, None))
  for c, (t, st) in enumerate(zip(tables, stores)):
    if st is not None:
      _check_store(st, t, slots[c])
  out = hash_remove(tables, ids_list, slots)
  for i, st in zip(ids_list, stores):
    if st is not None and len(st):
      st.discard(torch.unique(i).cpu())
  return out


def _check_store(store, table, slots):
  """Refuses a store that cannot take what ``table`` with the companions ``slots`` spills."""
  if not isinstance(store, HashSpillStore):
    raise _bad('the store must be a HashSpillStore')
  widths = tuple(int(p[0].shape[1]) if isinstance(p, (tuple, list)) and len(p) == 2 and
                 isinstance(p[0], torch.Tensor) and p[0].dim() == 2 else -1 for p in slots)
  if store.dim != table.dim or store.slot_dims != widths:
    raise _bad(f'the store holds rows of dim {store.dim} with companions of widths {list(store.slot_dims)}, the '
               f'table has dim {table.dim} and companions of widths {list(widths)}')
  if store.dtype != table.dtype:
    raise _bad(f'the store holds {_dtype_name(store.dtype)} rows, the table {_dtype_name(table.dtype)} rows: build '
               'HashSpillStore(..., dtype=table.dtype) (nothing is cast)')


class HashSpillStore:
  """The host tier of ONE bounded table: the keys :meth:`HashTable.spill_to` evicted, with their rows, ``last_seen``,
  ``freq`` and companion rows, in host memory, sorted by key.  A key lives in the store or in the table, not in
  both: :meth:`take` removes what it returns.

  Args:
    dim: floats per row of the table.
    slot_dims: the widths of the companion tensors, in the order of the ``slots`` of ``spill_to`` / ``fault_in``.
    pin_memory: keep the arrays in page-locked memory when a GPU is present (copies from and to the device run
      at the link's speed).
    dtype: of the table's rows (``HashTable(dtype=)``): the store keeps them as they are, bit for bit, and takes
      no other.

  Everything is vectorised torch (sort, ``searchsorted``, masks): no per-key Python loop; the results are a
  function of the calls alone."""

  def __init__(self, dim, slot_dims=(), pin_memory=True, dtype=torch.float32):
    self.dim = int(dim)
    if dtype != torch.float32 and dtype not in LOWP_DTYPES:
      raise _bad(f'dtype must be torch.float32, torch.bfloat16 or torch.float16, got {dtype!r}')
    self.dtype = dtype
    self.slot_dims = tuple(int(d) for d in slot_dims)
    if self.dim < 1 or any(d < 1 for d in self.slot_dims):
      raise _bad(f'dim and slot_dims must be >= 1, got {dim} and {list(slot_dims)}')
    self._pin = bool(pin_memory) and torch.cuda.is_available()
    self.clear()

  def clear(self):
    """Forget everything."""
    self._data = self._arrays(HashExport.empty(0, self.dim, True, self.slot_dims, dtype=self.dtype))

  @staticmethod
  def _arrays(exp):
    return [exp.keys, exp.rows, exp.last_seen, exp.freq] + list(exp.slots)

  def _export(self, arrays):
    return HashExport(arrays[0], arrays[1], arrays[2], arrays[3], arrays[4:])

  def _host(self, shape, dtype):
    return torch.empty(shape, dtype=dtype, pin_memory=self._pin)

  def __len__(self):
    return self._data[0].numel()

  def keys(self):
    """The keys the store holds, ascending (a copy)."""
    return self._data[0].clone()

  def _check(self, exp):
    if not isinstance(exp, HashExport):
      raise _bad('put needs a HashExport')
    n = exp.keys.numel()
    if exp.keys.dtype != torch.int64 or exp.keys.dim() != 1:
      raise _bad('put: exp.keys must be an int64 vector')
    if exp.rows.dtype != self.dtype or tuple(exp.rows.shape) != (n, self.dim):
      raise _bad(f'put: exp.rows must be {_dtype_name(self.dtype)} [{n}, {self.dim}], the store\'s own dtype (nothing '
                 f'is cast), got {exp.rows.dtype} {tuple(exp.rows.shape)}')
    if exp.last_seen is None or exp.freq is None:
      raise _bad('put: the export carries no last_seen / freq: a store keeps the keys of an expiring table')
    for name in ('last_seen', 'freq'):
      x = getattr(exp, name)
      if x.dtype != torch.int32 or tuple(x.shape) != (n,):
        raise _bad(f'put: exp.{name} must be int32 [{n}]')
    if len(exp.slots) != len(self.slot_dims):
      raise _bad(f'put: the export carries {len(exp.slots)} companion tensors, the store keeps {len(self.slot_dims)}')
    for k, (x, d) in enumerate(zip(exp.slots, self.slot_dims)):
      if x.dtype != torch.float32 or tuple(x.shape) != (n, d):
        raise _bad(f'put: exp.slots[{k}] must be fp32 [{n}, {d}], got {tuple(x.shape)}')

  def put(self, exp):
    """Copy a :class:`HashExport` (of any device) to the host and upsert it by key: a key the store already holds
    takes the new payload, as does the later of two equal keys of one export.  Widths or metadata that do not
    match the store are refused."""
    self._check(exp)
    if len(exp) == 0:
      return
    new = []
    for x in self._arrays(exp):
      if x.device.type == 'cpu':
        new.append(x)
      else:
        y = self._host(tuple(x.shape), x.dtype)
        y.copy_(x, non_blocking=True)
        new.append(y)
    if exp.keys.device.type != 'cpu':
      torch.cuda.current_stream(exp.keys.device).synchronize()
    keys = torch.cat([self._data[0], new[0]])
    order = torch.argsort(keys, stable=True)            # equal keys: the earlier entry first
    ordered = keys[order]
    last = torch.ones(ordered.numel(), dtype=torch.bool)
    last[:-1] = ordered[1:] != ordered[:-1]             # the last of every run of equal keys stays
    pick = order[last]
    self._data = [self._gather(torch.cat([a, b]), pick) for a, b in zip(self._data, new)]

  def _gather(self, x, index):
    out = self._host((index.numel(),) + tuple(x.shape[1:]), x.dtype)
    return torch.index_select(x, 0, index, out=out)

  def _locate(self, keys):
    """Positions in the store of the distinct requested keys it holds, ascending."""
    if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64 or keys.dim() != 1:
      raise _bad('keys must be an int64 vector')
    held = self._data[0]
    if held.numel() == 0 or keys.numel() == 0:
      return torch.zeros(0, dtype=torch.int64)
    wanted = torch.unique(keys.cpu())
    pos = torch.searchsorted(held, wanted).clamp_(max=held.numel() - 1)
    return pos[held[pos] == wanted]

  def peek(self, keys):
    """A CPU :class:`HashExport` of the requested keys the store holds, in ascending key order (duplicates in
    ``keys`` count once; keys the store does not hold are simply not returned).  The store keeps them."""
    pos = self._locate(keys)
    return self._export([self._gather(x, pos) for x in self._data])

  def take(self, keys):
    """:meth:`peek`, and the returned keys leave the store."""
    pos = self._locate(keys)
    out = self._export([self._gather(x, pos) for x in self._data])
    self._drop(pos)
    return out

  def discard(self, keys):
    """:meth:`take` without building the export: the requested keys the store holds leave it.  Returns their
    number."""
    pos = self._locate(keys)
    self._drop(pos)
    return int(pos.numel())

  def _drop(self, pos):
    if pos.numel():
      keep = torch.ones(len(self), dtype=torch.bool)
      keep[pos] = False
      rest = keep.nonzero().flatten()
      self._data = [self._gather(x, rest) for x in self._data]

  def variables(self, name):
    """The store's content as the flat dict ``training.saver.Saver.save`` takes (:meth:`HashExport.variables`)."""
    return self._export(self._data).variables(name)

  @classmethod
  def from_variables(cls, name, d, pin_memory=True):
    """The store a :meth:`variables` dict describes (:meth:`HashExport.from_variables`): dim and slot widths are
    read from the tensors."""
    exp = HashExport.from_variables(name, d)
    if exp.rows.dim() != 2 or any(x.dim() != 2 for x in exp.slots):
      raise _bad('from_variables: rows and companions must be matrices')
    store = cls(exp.rows.shape[1], [x.shape[1] for x in exp.slots], pin_memory, dtype=exp.rows.dtype)
    store.put(exp)
    return store


def _missing(tables, ids_list, seq=None):
  """``hbk_hash_missing_n`` over checked arguments: ONE C call for all tables, its outputs and workspace allocated
  once, ONE host read (all counts).  ``seq``: None, or the checked ``(row_splits, max_lens, pad_ids)`` lists of the
  sequence form.  Returns ``(missed, slots)``: per table the distinct missed ids (views of one buffer, narrowed to
  their counts) and the find's answers per position."""
  n = len(tables)
  for c, t in enumerate(tables):
    if not isinstance(t, HashTable):
      raise _bad(f'table {c} must be a HashTable')
    if not t.expiring:
      raise _bad(f'table {c}: missing needs a table built with expiring=True, as fault_in does (on a plain table '
                 'INT64_MIN + 1 is an ordinary key)')
  check_ids(ids_list, tables)
  lib = _lib.lib()
  if n == 0:
    _lib.check(lib.hbk_hash_missing_n(0, None, None, None, 0, None))
    return [], []
  dev = tables[0].keys.device
  cols = (_lib.HashMissingColumn * n)()
  seqs = (_lib.HashSequence * n)() if seq is not None else None
  positions = []
  for c, i in enumerate(ids_list):
    if seq is None:
      positions.append(i.numel())
      continue
    s, t_max = seq[0][c], seq[1][c]
    if s is not None:
      _lib.require_device_tensor(s, 'row_splits')
      if s.dtype != torch.int32 or s.dim() != 1 or s.numel() < 1 or s.device != i.device:
        raise _bad(f'row_splits of column {c} must be an int32 vector [samples+1] on {i.device}')
    b = i.numel() if s is None else s.numel() - 1
    if b * t_max >= 2 ** 30:
      raise _bad(f'column {c}: {b} samples x max_len {t_max} positions, must stay below 2^30')
    q = seqs[c]
    q.row_splits = s.data_ptr() if s is not None else None
    q.n_segments, q.max_len = b, t_max
    q.has_pad = 0 if seq[2][c] is None else 1
    q.pad_id = seq[2][c] or 0
    q.lengths = None
    positions.append(b * t_max)
  total = sum(positions)
  slots = torch.split(torch.empty(total, dtype=torch.int64, device=dev), positions)
  outs = torch.split(torch.empty(total, dtype=torch.int64, device=dev), positions)
  counts = torch.empty(n, dtype=torch.int64, device=dev)
  for c, (t, i) in enumerate(zip(tables, ids_list)):
    _lib.require_device_tensor(t.keys, 'keys')
    col = cols[c]
    col.keys_cache, col.slab_count, col.slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
    t._describe_expiry(col.exp)
    col.keys, col.n_keys = (i.data_ptr() if i.numel() else None), i.numel()
    col.slots = slots[c].data_ptr() if positions[c] else None
    col.out_ids, col.out_capacity = (outs[c].data_ptr() if positions[c] else None), positions[c]
    col.count = counts.data_ptr() + 8 * c
  nbytes = lib.hbk_hash_missing_workspace_bytes(n, cols, seqs)
  workspace = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
  _lib.check(lib.hbk_hash_missing_n(n, cols, seqs, workspace.data_ptr(), nbytes, _lib.current_stream(dev)))
  return [o[:k] for o, k in zip(outs, counts.tolist())], list(slots)   # the one host read


def hash_missing(tables, ids_list):
  """The distinct ids of ``ids_list[c]`` that expiring table c does not hold, per table a device int64 tensor in the
  order of the ids' FIRST occurrence (``hbk_hash_missing_n``): what :func:`hash_fault_in` asks the stores for.  ONE C
  call for all tables -- a find, a claim into a scratch set and a stream compaction per 32 tables -- with outputs
  and workspace allocated once, and ONE host read (all counts) whatever N.  ``INT64_MIN`` and ``INT64_MIN + 1`` are
  never reported; an evicted id (a TOMBSTONE) is.  The tables are not written: nothing is inserted, no
  ``last_seen`` is stamped."""
  tables = list(tables)
  same_device(tables)
  return _missing(tables, list(ids_list))[0]


def _restore(table, store, missed, slots):
  """The host half of a fault-in: ``store.take`` of the missed ids (a CPU int64 vector) and, if it returned anything,
  ``import_items``; what does not fit goes back into the store before the error is raised.  Returns the keys
  restored."""
  exp = store.take(missed)
  if len(exp) == 0:
    return 0
  try:
    table.import_items(exp, slots, assume_distinct=True)
  except Exception:
    # whatever is not in the table now goes back where it came from
    lost = (table.find(exp.keys.to(table.keys.device)) < 0).cpu().nonzero().flatten()
    store.put(HashExport(exp.keys[lost], exp.rows[lost], exp.last_seen[lost], exp.freq[lost],
                         [x[lost] for x in exp.slots]))
    raise
  return len(exp)


def hash_fault_in(tables, ids_list, stores, slots=None, row_splits=None, max_lens=None, pad_ids=None):
  """:meth:`HashTable.fault_in` for N expiring tables: the keys of ``ids_list[c]`` that ``stores[c]`` holds come back
  into table c as they left.  Tables whose store is empty are left out entirely; the others go through ONE
  :func:`hash_missing` call (one host read of the counts), their distinct missed ids reach the host in ONE copy, and
  then, per table in order, ``stores[c].take`` and -- if anything came back -- :meth:`HashTable.import_items` with
  the companions ``slots[c]``.  ``take`` returns ascending key order and counts duplicates once, so tables, stores
  and the return value are what the per-table loop produces, bit for bit.

  ``max_lens`` (with ``row_splits`` and ``pad_ids``, as for ``hash_translate_sequence``): the ids are read the way
  :class:`hybridbackend_amd.embedding.HashSequenceLookup` reads them (:func:`hash_missing_sequence`): an id that
  occurs only past ``T`` stays in its store, a pad id the store holds comes back.

  When a table is too full for some of the taken keys they go back into its store before the error is raised; the
  tables after it have not been taken from.  Returns the keys restored per table."""
  tables = list(tables)
  same_device(tables)
  n = len(tables)
  ids_list, stores, slots = _per_table(n, ('id tensors', ids_list, None), ('spill stores', stores, None),
                                       ('lists of companion tensors', slots, ()))
  for c, t in enumerate(tables):
    t._need_expiring('fault_in')
    _check_store(stores[c], t, [(x, 0.0) for x in slots[c]])
  seq = None
  if max_lens is not None:
    from hybridbackend_amd.embedding.hash_sequence import check_hash_sequence_args   # pylint: disable=import-outside-toplevel
    max_lens, pad_ids = check_hash_sequence_args(tables, max_lens, pad_ids)
    row_splits, = _per_table(n, ('row_splits', row_splits, None))
    seq = (row_splits, max_lens, pad_ids)
  elif row_splits is not None or pad_ids is not None:
    raise _bad('row_splits and pad_ids come with max_lens: the sequence form')
  check_ids(ids_list, tables)
  restored = [0] * n
  live = [c for c in range(n) if len(stores[c])]
  if not live:
    return restored
  missed, _ = _missing([tables[c] for c in live], [ids_list[c] for c in live],
                       None if seq is None else tuple([x[c] for c in live] for x in seq))
  if sum(m.numel() for m in missed) == 0:
    return restored
  for c, m in zip(live, missed_to_host(missed)):
    if m.numel():
      restored[c] = _restore(tables[c], stores[c], m, slots[c])
  return restored


def missed_to_host(missed):
  """The missed ids of several tables (device vectors) as CPU vectors, each ascending, in ONE copy: ordered per
  table before they leave the device (two stable sorts over all tables' ids at once) -- ``take`` orders its keys on
  the host, where an ordered list is the cheaper one (profiles/hash_fault_in.txt: 29.4 -> 25.7 ms at 10 %
  missed)."""
  sizes = [m.numel() for m in missed]
  flat = missed[0] if len(missed) == 1 else torch.cat(missed)
  order = torch.argsort(flat, stable=True)
  if len(missed) > 1:
    owner = torch.repeat_interleave(torch.arange(len(missed), device=flat.device),
                                    torch.tensor(sizes, device=flat.device), output_size=flat.numel())
    order = order[torch.argsort(owner[order], stable=True)]
  return torch.split(flat[order].cpu(), sizes)   # the one copy


def _check_loads(max_load, target_load):
  max_load, target_load = float(max_load), float(target_load)
  if not 0.0 < target_load <= max_load <= 1.0:
    raise _bad(f'0 < target_load <= max_load <= 1 is needed, got target_load {target_load!r} and max_load '
               f'{max_load!r}')
  return max_load, target_load


def check_ids(ids_list, tables):
  if len(ids_list) != len(tables):
    raise _bad(f'expected {len(tables)} id tensors, got {len(ids_list)}')
  for c, (i, t) in enumerate(zip(ids_list, tables)):
    if not isinstance(t, HashTable):
      raise _bad(f'table {c} must be a HashTable')
    if not isinstance(i, torch.Tensor) or i.dtype != torch.int64 or i.dim() != 1:
      raise _bad(f'ids of column {c} must be an int64 device vector')
    _lib.require_device_tensor(i, 'ids')
    if i.device != t.keys.device:
      raise _bad(f'ids of column {c} are on {i.device}, the table on {t.keys.device}')


class _Plan:
  """The descriptors of N tables, split by entry: the plain tables' columns for ``hbk_hash_insert_n``, the
  expiring ones' (with their expiry records) for ``hbk_hash_insert_expiring_n``, and the filtered tables of
  either kind (with their admission records) for ``hbk_hash_insert_admit_n`` /
  ``hbk_hash_insert_expiring_admit_n``.  ``cols[c]`` is table c's.  ``admit=False``: no table is taken as
  filtered (:meth:`HashTable.load`).  The 16-bit tables of each kind form groups of their own, after the fp32
  ones, and go through ``hbk_hash_insert_lowp_n``: ``dtypes[g]`` is group g's element codes, None for an fp32
  group, whose calls are what they were."""

  def __init__(self, tables, admit=True):
    groups = {}
    for c, t in enumerate(tables):
      groups.setdefault((t.dtype in LOWP_DTYPES, t.expiring, bool(admit and t.min_freq)), []).append(c)
    self.cols = [None] * len(tables)
    self.groups = []   # (expiring, filtered, columns, expiry records, admission records)
    self.dtypes = []   # per group: None, or the int32 element codes of its 16-bit tables
    for (lowp, expiring, filtered), members in sorted(groups.items()):
      cols = (_lib.HashColumn * len(members))()
      expiry = (_lib.HashExpiry * len(members))() if expiring else None
      adm = (_lib.HashAdmission * len(members))() if filtered else None
      for k, c in enumerate(members):
        self.cols[c] = cols[k]
        if expiring:
          tables[c]._describe_expiry(expiry[k])
        if filtered:
          tables[c]._describe_admission(adm[k])
      self.groups.append((expiring, filtered, cols, expiry, adm))
      codes = [LOWP_DTYPES[tables[c].dtype] for c in members] if lowp else None
      self.dtypes.append((C.c_int32 * len(members))(*codes) if lowp else None)

  def launch(self, insert, stream):
    insert = 1 if insert else 0
    lib = _lib.lib()
    if not self.groups:
      _lib.check(lib.hbk_hash_insert_n(0, None, insert, stream))
    for (expiring, filtered, cols, expiry, adm), dtypes in zip(self.groups, self.dtypes):
      n = len(cols)
      if dtypes is not None:
        _lib.check(lib.hbk_hash_insert_lowp_n(n, cols, expiry, adm, dtypes, insert, stream))
      elif expiring and filtered:
        _lib.check(lib.hbk_hash_insert_expiring_admit_n(n, cols, expiry, adm, insert, stream))
      elif expiring:
        _lib.check(lib.hbk_hash_insert_expiring_n(n, cols, expiry, insert, stream))
      elif filtered:
        _lib.check(lib.hbk_hash_insert_admit_n(n, cols, adm, insert, stream))
      else:
        _lib.check(lib.hbk_hash_insert_n(n, cols, insert, stream))


def _translate(tables, ids_list, insert, outs, init=True, plan=None):
  n = len(tables)
  check_ids(ids_list, tables)
  outs = [None] * n if outs is None else list(outs)
  if len(outs) != n:
    raise _bad(f'expected {n} outputs, got {len(outs)}')
  plan = _Plan(tables) if plan is None else plan
  cols = plan.cols
  for c in range(n):
    i, t = ids_list[c], tables[c]
    if outs[c] is None:
      outs[c] = torch.empty(i.numel(), dtype=torch.int64, device=i.device)
    o = outs[c]
    if not isinstance(o, torch.Tensor) or o.dtype != torch.int64 or tuple(o.shape) != (i.numel(),) or \
        o.device != i.device or not o.is_contiguous():
      raise _bad(f'output {c} must be a contiguous int64 [{i.numel()}] tensor on {i.device}')
    # a find counts nothing: `counts` is the table's record of what was inserted and refused
    t._describe(cols[c], init=init and insert, count=bool(insert))
    cols[c].keys = i.data_ptr()
    cols[c].n_keys = i.numel()
    cols[c].slots = o.data_ptr()
  dev = tables[0].keys.device if n else None
  plan.launch(insert, _lib.current_stream(dev))
  return outs


def hash_translate(tables, ids_list, insert=True, outs=None):
  """ids -> row numbers for N columns in ONE launch (``hbk_hash_insert_n``; plain, expiring and filtered tables
  may be mixed: each kind goes through its own entry, the filtered ones in two launches, count then admit).
  ``insert=False``: a pure find (-1 for ids never seen; no sketch is touched).  ``outs``: preallocated int64
  ``[n_ids]`` tensors.  Returns the list of slots."""
  tables = list(tables)
  same_device(tables)
  return _translate(tables, list(ids_list), insert, outs)


def sketch_cells(ids, depth, width, seed=0):
  """int64 ``[depth, n]``: the cell of every id in every row of a ``[depth, width]`` admission sketch,
  ``murmur3_hash32(id ^ (int64)((uint64)(seed + r + 1) * 0x9E3779B97F4A7C15)) % width`` (include/hbk.h), in
  torch ops on the ids' device."""
  m = 0xffffffff

  def rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & m
  rows = []
  for r in range(int(depth)):
    mix = ((int(seed) + r + 1) * 0x9E3779B97F4A7C15) & 0xffffffffffffffff
    x = ids ^ (mix - (1 << 64) if mix >> 63 else mix)
    h = torch.zeros_like(x)
    for k in (x & m, (x >> 32) & m):
      k = (k * 0xcc9e2d51) & m
      k = (rotl(k, 15) * 0x1b873593) & m
      h = rotl(h ^ k, 13)
      h = (h * 5 + 0xe6546b64) & m
    h = h ^ 8
    h = ((h ^ (h >> 16)) * 0x85ebca6b) & m
    h = ((h ^ (h >> 13)) * 0xc2b2ae35) & m
    h = h ^ (h >> 16)
    rows.append(h % int(width))
  return torch.stack(rows) if rows else ids.new_zeros((0, ids.numel()))


def same_device(tables):
  for c, t in enumerate(tables):
    if not isinstance(t, HashTable):
      raise _bad(f'table {c} must be a HashTable')
    if t.keys.device != tables[0].keys.device:
      raise _bad(f'tables must live on one device: table {c} is on {t.keys.device}, table 0 on '
                 f'{tables[0].keys.device}')


def require_fp32_tables(tables, what, why):
  """Refuses, by name, a 16-bit :class:`HashTable` where only fp32 rows are served."""
  for c, t in enumerate(tables):
    if isinstance(t, HashTable) and t.dtype != torch.float32:
      raise _bad(f'{what}: table {c} is a {t.dtype} HashTable; {why}')


def check_current(tables, rows):
  """Refuses when ``rows``, the ``table`` tensors an object was built over, are no longer the tables' own."""
  if any(t.table is not r for t, r in zip(tables, rows)):
    raise _bad('a table was rehashed: rebind() first')


def check_bound(lookup, tables, rows):
  """The guard of a ``launch()``: a call bound the tensors, and no table was rehashed since."""
  if not lookup._bound:   # pylint: disable=protected-access
    raise _lib.HbkError(_lib.INTERNAL, 'launch() needs a call that bound the tensors first')
  check_current(tables, rows)


def grow_tables(lookup, tables, max_load, factor, slots):
  """:meth:`HashTable.maybe_grow` on every table, then ``lookup.rebind()`` if any was rehashed."""
  slots, = _per_table(len(tables), ('lists of companion tensors', slots, ()))
  out = [t.maybe_grow(max_load, factor, slots[c]) for c, t in enumerate(tables)]
  if any(o is not None for o in out):
    lookup.rebind()
  return out


def evict_tables(lookup, tables, max_load, target_load, keep_freq, slots, spill=None, order='lru'):
  """:meth:`HashTable.maybe_evict` on every table, then ``lookup.rebind()`` if any was rehashed.  ``spill``: one
  :class:`HashSpillStore` per table (a single store for a single table), or None.  ``order``: ``'lru'`` or ``'lfu'``,
  for every table."""
  order = _check_order(order)
  if isinstance(spill, HashSpillStore):
    spill = [spill]
  slots, spill = _per_table(len(tables), ('lists of companion tensors', slots, ()), ('spill stores', spill, None))
  _check_loads(max_load, target_load)
  out = [t.maybe_evict(max_load, target_load, keep_freq, slots[c], spill[c], order) for c, t in enumerate(tables)]
  if any(o is not None for o in out):
    lookup.rebind()
  return out


class HashGroupLookup:
  """N hash-keyed columns: one translate launch, then a :class:`GroupLookup` over ``[t.table ...]`` with
  buckets 0 on the row numbers.

  Args:
    tables: list of :class:`HashTable` on one device.
    combiners / max_norms: GroupLookup's.
    train: True -- ids never seen are inserted; False -- they translate to -1 and read as rows outside a
      table do, as zeros (they still count in a mean's divisor, as invalid ids do everywhere).

  After a call ``self.slots`` holds the row numbers per column and ``self.lookup`` the GroupLookup:
  ``GroupLookupGrad(hgl.lookup, ...)(hgl.slots, grads, row_splits, ...)`` is the backward / optimizer step.

  16-bit tables (``HashTable(..., dtype=torch.bfloat16 / torch.float16)``): all tables of one object are fp32 or all
  are 16-bit -- a mix is refused; ``hash_translate`` takes all kinds in one call, the lookups are two groups.  Over
  16-bit tables ``self.lookup`` is a :class:`hybridbackend_amd.embedding.LowpGroupLookup` with buckets 0 (a ``-1``
  slot reads a zero row; ``max_norms`` is refused), and the step is ``LowpLookupGrad`` where it was
  ``GroupLookupGrad``::

      step = LowpLookupGrad(hgl.lookup, row_accums=accums, rounding='stochastic', seed=7)
      step(hgl.slots, grads, row_splits, apply_lr=lr, optimizer='rowwise_adagrad')

  rebuilt after a rehash exactly as a ``GroupLookupGrad`` is.  The optimizer slots stay fp32.  Never hand
  ``hgl.lookup`` over 16-bit tables to a bare ``GroupLookupGrad`` with a non-zero ``apply_lr`` (see
  ``LowpLookupGrad``).
  """

  def __init__(self, tables, combiners='sum', max_norms=None, train=True):
    self.tables = list(tables)
    same_device(self.tables)
    self.train = bool(train)
    self._combiners, self._max_norms = combiners, max_norms
    self.rebind()

  def rebind(self):
    """After a rehash of a table (:func:`hash_rehash`, :meth:`HashTable.maybe_grow`): ``self.lookup`` is built
    again over the tables' current ``table`` tensors with the same combiners and max_norms, and the bound state
    is dropped -- :meth:`launch` refuses until the next call, as on a fresh object.  Slot numbers and tensor
    addresses changed: a ``GroupLookupGrad`` built on the old ``hgl.lookup`` must be rebuilt with the new slot
    tensors (the companions the rehash returned), and a captured graph must be captured again."""
    lowp = [t.dtype in LOWP_DTYPES for t in self.tables]
    if any(lowp) and not all(lowp):
      mixed = ', '.join(f'table {c}: {_dtype_name(t.dtype)}' for c, t in enumerate(self.tables))
      raise _bad(f'HashGroupLookup: fp32 and 16-bit tables cannot share one lookup ({mixed}): translate them together '
                 'with hash_translate, then look them up in two groups -- or build one HashGroupLookup per kind')
    if any(lowp):
      # (a clip is refused there, by name: it reads and the clipped step writes fp32 rows)
      from hybridbackend_amd.embedding.lowp import LowpGroupLookup   # pylint: disable=import-outside-toplevel
      self.lookup = LowpGroupLookup([t.table for t in self.tables], buckets=None, combiners=self._combiners,
                                    max_norms=self._max_norms, wide_rows=True)
    else:
      self.lookup = GroupLookup([t.table for t in self.tables], buckets=None, combiners=self._combiners,
                                max_norms=self._max_norms)
    self._plan = _Plan(self.tables)
    self._rows = [t.table for t in self.tables]
    self.slots = None
    self._keep = None
    self._bound = False

  def maybe_grow(self, max_load=0.75, factor=2.0, slots=None):
    """:meth:`HashTable.maybe_grow` on every table (``slots[c]``: the companions of table c), then
    :meth:`rebind` if any table was rehashed.  Returns the per-table results: None, or the new companion
    tensors.  See :meth:`rebind` for what must be rebuilt afterwards."""
    return grow_tables(self, self.tables, max_load, factor, slots)

  def maybe_evict(self, max_load=0.75, target_load=0.5, keep_freq=0, slots=None, spill=None, order='lru'):
    """:meth:`HashTable.maybe_evict` on every table (``slots[c]``: the companions of table c; ``spill``: one
    :class:`HashSpillStore` per table, or None; ``order``: ``'lru'`` or ``'lfu'``), then :meth:`rebind` if any table
    was rehashed.  Returns the per-table results: None, or the new companion tensors.  See :meth:`rebind` for what
    must be rebuilt afterwards."""
    return evict_tables(self, self.tables, max_load, target_load, keep_freq, slots, spill, order)

  def fault_in(self, ids, stores, slots=None):
    """:meth:`HashTable.fault_in` on every table, before the call of the step (:func:`hash_fault_in`: one
    ``hbk_hash_missing_n`` call for all tables that have anything spilled): ``ids[c]`` the raw ids of column c,
    ``stores[c]`` its :class:`HashSpillStore`, ``slots[c]`` its companion tensors.  The row tensors do not move, so
    no :meth:`rebind` is needed.  Returns the keys restored per table."""
    return hash_fault_in(self.tables, ids, stores, slots)

  def remove(self, ids_list, slots=None, stores=None):
    """:meth:`HashTable.remove` on every table in one call (:func:`hash_remove`): ``ids_list[c]`` the raw ids to take
    out of column c, ``slots[c]`` its ``(tensor, fill_value)`` companions, ``stores[c]`` its
    :class:`HashSpillStore` or None.  The row tensors do not move, so no :meth:`rebind` is needed; slots handed out
    earlier for the removed ids are void.  Returns the old slots per table."""
    return remove_tables(self.tables, ids_list, slots, stores)

  def __len__(self):
    return len(self.tables)

  def __call__(self, ids, row_splits=None, outs=None, sp_weights=None):
    """ids[c]: int64 raw ids, row_splits[c]: int32 ``[segments + 1]`` or None.  Returns GroupLookup's outputs."""
    self._translate_step(ids)
    return self.lookup(self.slots, row_splits, outs, sp_weights=sp_weights)

  def call_block(self, ids, row_splits, block, offsets, outs, sp_weights=None):
    """The call with every column's output a column block of ONE ``[segments, pitch]`` fp32 tensor (column c starts
    at float ``offsets[c]`` of every row: ``GroupLookup.bind_block``, what ``DenseFeatures`` writes): no per-column
    views are made.  ``outs``: a callable that gives the per-column views, asked only when the block needs the
    detailed checks of the ordinary call."""
    self._translate_step(ids)
    if self.lookup.bind_block(self.slots, row_splits, block, offsets, sp_weights=sp_weights):
      self.lookup.launch()
    else:
      self.lookup(self.slots, row_splits, outs(), sp_weights=sp_weights)

  def _translate_step(self, ids):
    """The translate launch of a call: ``self.slots`` holds the row numbers afterwards."""
    ids = list(ids)
    check_current(self.tables, self._rows)
    # the slot buffers of the call before serve again while the id counts stay (a resident loop; a
    # captured launch() needs them to stay where they are)
    keep = self.slots
    if keep is not None and (len(keep) != len(ids) or any(
        not isinstance(i, torch.Tensor) or s.numel() != i.numel() for s, i in zip(keep, ids))):
      keep = None
    self.slots = _translate(self.tables, ids, self.train, keep, plan=self._plan)
    self._keep = ids
    self._bound = True

  def launch(self, stream=None):
    """Both launches of the LAST call again on its tensors (id buffers refilled in place; captured graphs):
    two foreign calls, no allocation."""
    check_bound(self, self.tables, self._rows)
    dev = self.tables[0].keys.device if self.tables else None
    s = _lib.current_stream(dev) if stream is None else C.c_void_p(stream.cuda_stream)
    self._plan.launch(self.train, s)
    self.lookup.launch(stream)
