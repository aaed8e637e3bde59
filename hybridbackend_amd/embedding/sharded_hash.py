"""Sharded hash tables: hash-keyed columns behind the sharded lookup step (``hbk_sharded_set_hash_tables``,
include/hbk.h; DeepRec partitions its EmbeddingVariable the same way, the reference's ``EmbeddingService`` sits
behind its sharded lookup).

Every rank holds one :class:`HashTable` per column.  An id belongs to rank ``floormod(id, W)``
(:func:`hash_owner`); the step brings each owner the raw int64 ids it owns, the owner translates them into row
numbers of its table (one ``hbk_hash_translate_runs_n`` call per table kind, over the W runs where they lie),
gathers those rows, and in the backward reduces and steps them -- everything else of the step is
:class:`ShardedGroupLookup`'s, unchanged.

A bounded table keeps its state in a host tier (``stores``): the forward then runs in three parts, and between the id
exchange and the owner's translate the keys this rank received and spilled earlier come back from their stores
(``hbk_sharded_hash_missing``, :meth:`ShardedHashGroupLookup.fault_in_received`).
"""
import ctypes as C

import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import hashtable as _ht
from hybridbackend_amd.embedding import lowp as _lowp
from hybridbackend_amd.embedding import optimizer as _opt
from hybridbackend_amd.embedding.sharded import ShardedGroupLookup


def slot_kinds(owner, accum_fill):
  """The optimizer slots ``owner`` holds (``accums``, ``moments``, ``ftrl_slots`` with ``ftrl``, ``row_accums``
  with ``rowwise_adagrad``) as (attribute, index in a pair or None, fill value), in the ONE order every call that
  moves them with a hash table uses -- ``accums``; ``moments`` m, v; ``ftrl_slots`` accum, linear; ``row_accums``
  (``[capacity, 1]``: a companion of one word) -- and with the value a row that no key holds is set to:
  ``accum_fill`` for Adagrad's accumulator, 0 for Adam's m / v, FTRL's accum its ``initial_accumulator_value`` and
  linear 0, row-wise Adagrad's its ``initial_accumulator_value``.  The sharded driver and the feature-column
  layers share it."""
  kinds = []
  if owner.accums is not None:
    kinds.append(('accums', None, float(accum_fill)))
  if owner.moments is not None:
    kinds += [('moments', 0, 0.0), ('moments', 1, 0.0)]
  if owner.ftrl_slots is not None:
    kinds += [('ftrl_slots', 0, float(owner.ftrl.initial_accumulator_value)), ('ftrl_slots', 1, 0.0)]
  if getattr(owner, 'row_accums', None) is not None:
    kinds.append(('row_accums', None, float(owner.rowwise_adagrad.initial_accumulator_value)))
  return kinds


def slot_companions(owner, kinds, c):
  """The slots of table c as ``(tensor, fill_value)`` pairs, in the order of ``kinds``."""
  return [(getattr(owner, name)[c] if k is None else getattr(owner, name)[c][k], fill) for name, k, fill in kinds]


class ShardedHashGroupLookup(ShardedGroupLookup):
  """N hash-keyed columns, each sharded over the ranks by ``floormod(id, W)``.

  Args:
    tables: this rank's :class:`HashTable` per column (plain, expiring and filtered ones may be mixed; ranks
      may differ in capacity and geometry, not in dim).
    coll, combiners, wire_dtype, dedup, max_norms, hot_rows, world_size: :class:`ShardedGroupLookup`'s.
    train: True -- ids the owner never saw are inserted (a filtered table: once admitted); False -- a pure find:
      they read as zero rows, and neither ``size()`` nor ``counts`` moves.
    accums / moments, adam / ftrl_slots, ftrl: the optimizer slots of the tables, ``[capacity, dim]`` each, as for
      :class:`ShardedGroupLookup`; row_accums, rowwise_adagrad: row-wise Adagrad's, ``[capacity, 1]`` each.
    initial_accumulator_value: what :meth:`maybe_grow` fills the rows of a grown Adagrad accumulator with that no
      key holds (FTRL's comes from ``ftrl``).
    stores: None, or per column a :class:`HashSpillStore` or None -- the host tier of this rank's table (an
      expiring one), of the table's dim and the widths of the bound optimizer slots in the order of ``slot_kinds``.
      With stores a forward (``__call__`` / ``launch``) is :meth:`launch_ids`, :meth:`fault_in_received`,
      :meth:`launch_gather`, :meth:`launch_end`: the keys this rank receives come back from their stores with rows,
      metadata and optimizer slots before the translate could insert fresh rows for them, with ``train=False`` as
      well (nothing is inserted that a store does not hold).  :meth:`spill_to` bounds the tables into the stores.
      Such a forward reads the host (the counts of the missed ids), so it is NOT capturable: ``launch`` raises while
      the current stream is capturing.  ``stores=None`` issues exactly the calls of a driver without a host tier.

  ``__call__``, ``bind``, ``launch``, ``backward``, ``prefetch`` and ``close`` are inherited; in the slices
  ``backward`` returns, ``unique_rows`` are slot numbers of this rank's tables (``tables[c].keys[unique_rows]``
  names the ids).  ``sp_weights`` and ``p2p_bind`` are refused by the library; ``PipelinedLookup`` refuses
  objects of this class.  Eviction, ``set_step`` and filter maintenance are the tables' own methods: they move
  no tensor, so the plan stays valid.  A rehash of a table does: :meth:`rebind` (or :meth:`maybe_grow` and
  :meth:`maybe_evict`, which do both)."""

  def __init__(self, tables, coll, combiners='sum', wire_dtype=None, dedup=False, max_norms=None, train=True,
               accums=None, moments=None, adam=None, ftrl_slots=None, ftrl=None, hot_rows=False, world_size=None,
               initial_accumulator_value=0.1, row_accums=None, rowwise_adagrad=None, stores=None):
    self.tables = list(tables)
    _ht.same_device(self.tables)
    _ht.require_fp32_tables(self.tables, 'ShardedHashGroupLookup',
                            'the owner-side translate, gather and step read and write fp32 rows of 4 * dim bytes: '
                            'sharded hash tables are fp32 (HashGroupLookup serves 16-bit ones)')
    self.train = bool(train)
    self.initial_accumulator_value = float(initial_accumulator_value)
    self._rows = [t.table for t in self.tables]
    super().__init__(self._rows, coll, buckets=None, combiners=combiners, wire_dtype=wire_dtype,
                     world_size=world_size, accums=accums, hot_rows=hot_rows, dedup=dedup, moments=moments, adam=adam,
                     ftrl_slots=ftrl_slots, ftrl=ftrl, max_norms=max_norms, row_accums=row_accums,
                     rowwise_adagrad=rowwise_adagrad)
    self._init_stores(stores)

  def _init_stores(self, stores):
    """The last part of construction, shared with the subclasses: the host tier and its checks."""
    self.stores = None if stores is None else list(stores)
    self.last_restored = [0] * len(self.tables)
    try:
      self._check_stores()
    except _lib.HbkError:
      self.close()
      raise

  def _check_stores(self):
    """Every store fits its table and the bound optimizer slots (in the one order of ``slot_kinds``)."""
    if self.stores is None:
      return
    if len(self.stores) != len(self.tables):
      raise _ht._bad(f'stores: expected one spill store (or None) per table, {len(self.tables)}, got '   # pylint: disable=protected-access
                     f'{len(self.stores)}')
    for c, (t, st) in enumerate(zip(self.tables, self.stores)):
      if st is None:
        continue
      if not t.expiring:
        raise _ht._bad(f'stores[{c}]: a spill store needs a table built with expiring=True (what leaves a plain '   # pylint: disable=protected-access
                       'table leaves no TOMBSTONE behind)')
      _ht._check_store(st, t, self._companions(c))   # pylint: disable=protected-access

  def _current(self):
    _ht.check_current(self.tables, self._rows)

  def _plan(self):
    self._current()
    return super()._plan()

  def _hash_descriptors(self):
    """The ``hbk_sharded_hash_t`` of every table, as the plan's setters take them."""
    n = len(self.tables)
    arr = (_lib.ShardedHash * n)()
    for c, t in enumerate(self.tables):
      _lib.require_device_tensor(t.keys, 'keys')
      h = arr[c]
      h.keys_cache, h.slab_count, h.slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
      # a find counts nothing: `counts` is the table's record of what was inserted and refused
      h.counts = t.counts.data_ptr() if self.train else None
      h.init_scale, h.seed = t.init_scale, t.seed
      if t.expiring:
        t._describe_expiry(h.exp)        # pylint: disable=protected-access
      if t.min_freq:
        t._describe_admission(h.adm)     # pylint: disable=protected-access
      h.insert = 1 if self.train else 0
    return arr

  def _set_hash_tables(self, arr):
    return self._lib.hbk_sharded_set_hash_tables(self._plan_handle, arr)

  def _plan_created(self):
    """The tables' descriptors, right after the plan's creation; a refusal leaves no plan behind."""
    try:
      _lib.check(self._set_hash_tables(self._hash_descriptors()))
    except _lib.HbkError:
      self.close()
      raise

  def p2p_bind(self, outs):
    """Refused (``hbk_sharded_p2p_bind``: the p2p form has no owner-side translate)."""
    n = len(self.shards)
    _lib.check(self._lib.hbk_sharded_p2p_bind(
      self._plan(), _lib.ptr_array([o.data_ptr() for o in outs]), (C.c_int32 * n)(),
      _lib.i64_array([int(o.shape[0]) for o in outs]), _lib.current_stream(self.device)))
    raise _lib.HbkError(_lib.INTERNAL, 'p2p_bind: a plan with hash columns was bound')

  def rebind(self, accums=None, moments=None, ftrl_slots=None, row_accums=None):
    """After a rehash of any table (``hash_rehash``, ``HashTable.maybe_grow``): the plan is closed and the
    owner-side state built again over the tables' current tensors and the given slot tensors (the companions the
    rehash returned; None: the ones bound now, which must still have the tables' shapes).  Until then every call
    on the object is refused.  Local to the rank: no exchange."""
    self.close()
    rows = [t.table for t in self.tables]
    if accums is None:
      accums = self.accums
    if accums is not None:
      accums = list(accums)
      if len(accums) != len(rows) or any(tuple(a.shape) != tuple(r.shape) for a, r in zip(accums, rows)):
        raise _ht._bad('rebind: accums must be one fp32 [capacity, dim] tensor per table')   # pylint: disable=protected-access
    given = dict(moments=moments, ftrl_slots=ftrl_slots, row_accums=row_accums)
    for cls in _opt.TWO_SLOT.values():   # (None: the slots bound now; the optimizer objects stay)
      if given[cls.slot_kw] is None:
        given[cls.slot_kw] = getattr(self, cls.slot_kw)
      given[cls.name] = getattr(self, cls.name)
    # (checked into a scratch holder first: a refusal leaves this object's slots as they were)
    new = type('_Bound', (), {})()
    _opt.bind_all(new, given, rows, 'ShardedHashGroupLookup.rebind')
    self.shards, self._rows, self.accums = rows, rows, accums
    for cls in _opt.TWO_SLOT.values():
      setattr(self, cls.slot_kw, getattr(new, cls.slot_kw))
      setattr(self, cls.name, getattr(new, cls.name))
    self._call_cache = self._keep = self._auto_state = None
    self._setup()
    self._check_stores()

  def _slot_kinds(self):
    """The bound optimizer slots as (attribute, index in a pair or None, fill value), in the order every method
    that moves them uses: ``accums``; ``moments`` m, v; ``ftrl_slots`` accum, linear; ``row_accums``."""
    return slot_kinds(self, self.initial_accumulator_value)

  def _slot_tensors(self, c):
    return [getattr(self, name)[c] if k is None else getattr(self, name)[c][k] for name, k, _ in self._slot_kinds()]

  def export_items(self, since=None):
    """:func:`hash_export` of this rank's tables in one call, the bound optimizer slots travelling as companions
    in the order Adagrad's ``accums``; Lazy Adam's ``moments`` m, v; FTRL's ``ftrl_slots`` accum, linear;
    row-wise Adagrad's ``row_accums`` (those that are bound).  ``since``: None, or the step of a delta -- every table must then be expiring; with
    :meth:`track_removals` on, the delta names the keys that left (``HashExport.removed``).  Returns one
    :class:`HashExport` per table.  Local to the rank: no exchange, and ranks need not agree."""
    self._current()
    n = len(self.tables)
    return _ht.hash_export(self.tables, [since] * n, [self._slot_tensors(c) for c in range(n)])

  def import_items(self, exports):
    """``exports[c]``: a :class:`HashExport` of column c -- typically ``HashExport.cat`` of what every rank of the
    saving job exported, at whatever world size that was.  Each table upserts the keys THIS rank owns
    (``hash_owner(keys, world_size) == rank``) with rows, metadata and the bound optimizer slots (the order of
    :meth:`export_items`), after the owned keys of ``removed`` left with the fill values of :meth:`maybe_grow`; the
    tensors stay where they are, so the plan stays valid.  Returns the slots per table.  Local to the rank: no
    exchange, and ranks need not agree."""
    self._current()
    exports = list(exports)
    if len(exports) != len(self.tables):
      raise _ht._bad(f'expected {len(self.tables)} exports, got {len(exports)}')   # pylint: disable=protected-access
    return [t.import_items(e, self._companions(c), world=self.world_size, rank=self.coll.rank)
            for c, (t, e) in enumerate(zip(self.tables, exports))]

  def _companions(self, c):
    """The bound optimizer slots of table c as ``(tensor, fill_value)`` pairs, the fill values of
    :meth:`maybe_grow`."""
    return slot_companions(self, self._slot_kinds(), c)

  def remove(self, ids_list):
    """:func:`hash_remove` on this rank's tables: the ids of ``ids_list[c]`` this rank's table c holds leave it,
    the bound optimizer slots reset as companions with the fill values of :meth:`maybe_grow`; with ``stores`` they
    are discarded from the stores too.  Local to the rank: ids the rank does not own are simply not found, there is
    no exchange, and ranks need not agree.  The tensors stay where they are, so the plan stays valid.  Returns the
    old slots per table."""
    self._current()
    companions = [self._companions(c) for c in range(len(self.tables))]
    if self.stores is None:
      return _ht.hash_remove(self.tables, ids_list, companions)
    return _ht.remove_tables(self.tables, ids_list, companions, self.stores)

  # ---- the host tier inside the step ------------------------------------------------------------------------
  def _tiered(self):
    """The columns that have a store."""
    return [c for c, st in enumerate(self.stores or ()) if st is not None]

  def launch(self, bound):
    """Enqueue a bound step on the current stream; returns its outputs.  With ``stores``: :meth:`launch_ids`,
    :meth:`fault_in_received`, :meth:`launch_gather`, ``launch_end`` -- not capturable.  No rank leaves a
    collective half-made: when a table is too full for the keys its store gave back, they return to the store, the
    step is finished as every other rank finishes it, and only then the error is raised (that refusal alone is
    deferred: any other error of the fault-in leaves at once)."""
    if self.stores is None:
      return super().launch(bound)
    if torch.cuda.is_current_stream_capturing():
      raise _lib.HbkError(_lib.INTERNAL, 'launch: a forward with spill stores reads the host (the counts of the '
                          'missed ids): it cannot be captured into a graph')
    self._refresh_hot_rows()
    self.launch_ids(bound)
    error = None
    try:
      self.fault_in_received()
    except _lib.InvalidArgumentError as e:   # (a table too full: every other error leaves at once)
      error = e
    self.launch_gather(bound)
    outs = self.launch_end(bound)
    if error is not None:
      raise error
    return outs

  def launch_begin(self, bound):
    """``ShardedGroupLookup.launch_begin``; refused on a driver with stores: the one-call first half translates
    before anything could come back from a store, and a spilled key would get a fresh row beside its stored one.
    Use :meth:`launch_ids`, :meth:`fault_in_received`, :meth:`launch_gather`."""
    if self.stores is not None:
      raise _lib.HbkError(_lib.UNIMPLEMENTED, 'launch_begin: a driver with spill stores runs its first half as '
                          'launch_ids, fault_in_received, launch_gather')
    super().launch_begin(bound)

  def fault_in_received(self):
    """Between :meth:`launch_ids` and :meth:`launch_gather`: the keys among the ids this rank received that its
    stores hold come back into the tables -- rows, ``last_seen``, ``freq`` and the bound optimizer slots as they
    left -- so that the translate finds them.  Columns whose store is empty are not asked; when none is left there
    is no launch and no host read.  Otherwise ONE ``hbk_sharded_hash_missing`` call, ONE host read of the counts,
    the missed ids ordered per column on the device and copied to the host in ONE copy (as :func:`hash_fault_in`),
    then per column ``store.take`` and ``import_items(..., assume_distinct=True)``.  When a table is too full for
    the taken keys they go back into its store before the error is raised; the columns after it have not been
    taken from.  Local to the rank: no exchange, and ranks need not agree on whether anything was missed.  Returns
    the keys restored per column (also ``last_restored``)."""
    n = len(self.tables)
    self.last_restored = restored = [0] * n
    live = [c for c in self._tiered() if len(self.stores[c])]
    if not live:
      return restored
    self._current()
    plan = self._plan()
    caps = [0] * n
    for c in live:
      caps[c] = max(int(self._lib.hbk_sharded_owned_ids(plan, c)), 0)
    outs = torch.split(torch.empty(max(sum(caps), 1), dtype=torch.int64, device=self.device)[:sum(caps)], caps)
    counts = torch.zeros(n, dtype=torch.int64, device=self.device)
    want = (C.c_uint8 * n)(*[1 if caps[c] else 0 for c in range(n)])
    _lib.check(self._lib.hbk_sharded_hash_missing(
      plan, want, _lib.ptr_array([o.data_ptr() if k else None for o, k in zip(outs, caps)]), _lib.i64_array(caps),
      counts.data_ptr(), _lib.current_stream(self.device)))
    found = counts.tolist()   # the one host read
    live = [c for c in live if found[c]]
    if not live:
      return restored
    for c, m in zip(live, _ht.missed_to_host([outs[c][:found[c]] for c in live])):
      restored[c] = _ht._restore(self.tables[c], self.stores[c], m, self._companions(c))   # pylint: disable=protected-access
    return restored

  def spill_to(self, max_sizes, keep_freq=0, order='lru'):
    """:func:`hash_spill` on the columns that have a store: the keys ``evict_to(max_sizes[c])`` would evict leave
    table c WITH their rows, metadata and the bound optimizer slots (companions with the fill values of
    :meth:`maybe_grow`) and go into ``stores[c]``.  ``max_sizes``: one bound for all columns or one per column.  It
    moves no tensor, so the plan stays valid.  Local to the rank: no exchange, and ranks need not agree.  Returns
    the keys spilled per column."""
    self._current()
    n = len(self.tables)
    if self.stores is None:
      raise _ht._bad('spill_to: the driver was built without stores')   # pylint: disable=protected-access
    if isinstance(max_sizes, int):
      max_sizes = [max_sizes] * n
    max_sizes = list(max_sizes)
    if len(max_sizes) != n:
      raise _ht._bad(f'spill_to: expected {n} max_sizes, got {len(max_sizes)}')   # pylint: disable=protected-access
    live = self._tiered()
    spilled = [0] * n
    exports = _ht.hash_spill([self.tables[c] for c in live], [max_sizes[c] for c in live], keep_freq,
                             [self._companions(c) for c in live], order=order)
    for c, exp in zip(live, exports):
      if len(exp):
        self.stores[c].put(exp)
      spilled[c] = len(exp)
    return spilled

  def track_removals(self, on=True):
    """:meth:`HashTable.track_removals` on every table of this rank (all must be expiring): what :meth:`remove`,
    :meth:`maybe_evict` and the tables' own sweeps take out is recorded, and a delta :meth:`export_items` carries
    it."""
    for t in self.tables:
      t.track_removals(on)

  def maybe_grow(self, max_load=0.75, factor=2.0):
    """:meth:`HashTable.maybe_grow` on every table of this rank, the bound optimizer slots moving along as
    companions (the rows no key holds afterwards: Adagrad's accumulator ``initial_accumulator_value``, Adam's m /
    v 0, FTRL's accum its ``initial_accumulator_value`` and linear 0), then :meth:`rebind` with the new tensors
    if any table was rehashed.  Local to the rank: no exchange, and ranks need not agree.  Returns per table
    whether it was rehashed."""
    return self._maybe(lambda c, t, comp: t.maybe_grow(max_load, factor, comp))

  def maybe_evict(self, max_load=0.75, target_load=0.5, keep_freq=0, order='lru', spill=False):
    """:meth:`HashTable.maybe_evict` on every table of this rank -- the capacity stays, the oldest keys leave
    (``order='lfu'``: the least frequently used ones) --
    with the bound optimizer slots as companions and the fill values of :meth:`maybe_grow`, then :meth:`rebind`
    with the new tensors if any table was rehashed.  ``spill=True``: a column that has a store spills where it
    evicted -- what leaves goes into ``stores[c]`` (:meth:`HashTable.spill_to`).  Local to the rank: no exchange,
    and ranks need not agree.  Returns per table whether it was rehashed."""
    _ht._check_loads(max_load, target_load)   # pylint: disable=protected-access
    _ht._check_order(order)   # pylint: disable=protected-access
    if spill and self.stores is None:
      raise _ht._bad('maybe_evict: spill=True needs a driver built with stores')   # pylint: disable=protected-access
    stores = self.stores if spill else [None] * len(self.tables)
    return self._maybe(lambda c, t, comp: t.maybe_evict(max_load, target_load, keep_freq, comp, spill=stores[c],
                                                        order=order))

  def _maybe(self, policy):
    """``policy(c, table, companions)`` -> None or the new companions, on every table; the rebind that follows."""
    kinds = self._slot_kinds()
    new = {name: [list(x) if k is not None else x for x in getattr(self, name)]
           for name, k, _ in kinds}
    grown = []
    for c, t in enumerate(self.tables):
      out = policy(c, t, self._companions(c))
      grown.append(out is not None)
      for (name, k, _), x in zip(kinds, out or ()):
        if k is None:
          new[name][c] = x
        else:
          new[name][c][k] = x
    if any(grown):
      paired = {name for name, k, _ in kinds if k is not None}
      self.rebind(**{name: [tuple(p) for p in xs] if name in paired else xs for name, xs in new.items()})
    return grown


class LowpShardedHashGroupLookup(ShardedHashGroupLookup):
  """N hash-keyed columns over 16-bit tables (``HashTable(..., dtype=torch.bfloat16 / torch.float16)``), each sharded
  over the ranks by ``floormod(id, W)``: :class:`ShardedHashGroupLookup`'s forward and lifecycle over
  ``hbk_sharded_set_lowp_hash_tables``, ``LowpShardedGroupLookup``'s backward and step.

  Args:
    tables16: this rank's :class:`HashTable` per column, every one of them 16-bit (bf16 and fp16 may be mixed; plain,
      expiring and filtered ones too).
    coll, combiners, dedup, train, stores, initial_accumulator_value: :class:`ShardedHashGroupLookup`'s.  Stores come
      from ``HashSpillStore(dtype=)`` of the table's dtype.
    wire: ``'table'`` (the default) -- the owner's rows cross the link in the table's own 16 bits, half the bytes of
      fp32 and nothing rounded -- or ``'float'``: the owner upcasts.  Both give, bit for bit,
      :class:`ShardedHashGroupLookup` over fp32 tables holding the upcast rows of the same keys.
    accums / moments, adam / ftrl_slots, ftrl / row_accums, rowwise_adagrad: FP32 slots of the tables' shapes
      (``[capacity, dim]``; row-wise Adagrad ``[capacity, 1]``) and the optimizer objects.  They are the companions
      every lifecycle method moves with the keys.
    rounding, seed: as ``LowpSparseApply``; rank k steps with ``rank_seed(seed, k)``, the noise keyed by the SLOT.

  The owner's translate is ``hbk_hash_translate_runs_lowp_n``: a new row is the fp32 start row rounded to nearest
  even.  ``backward(grads, apply_lr=, optimizer=, emit=, finish=)`` is the plan's emit backward -- slot numbers,
  nothing sent for a ``-1`` -- followed by ``LowpSparseApply`` on ``tables[c].table``; with ``emit=False`` the slices
  go into buffers this object owns.  ``rebind``, ``maybe_grow``, ``maybe_evict``, ``remove``, ``export_items`` /
  ``import_items``, ``track_removals``, ``spill_to`` and ``fault_in_received`` are the base class's: rows travel in
  the table's dtype, nothing is cast.  The rounding's step counter survives a :meth:`rebind`.

  Refused by name: fp32 tables and a mix of fp32 and 16-bit tables, ``max_norms``, ``weight_grads``, ``wire_dtype``,
  ``hot_rows``, ``p2p_bind``; ``sp_weights`` by the library (a weighted column needs a bucket); a ``dim`` the plan
  refuses (odd, or wider than 64 with ``dim % 4 != 0``); ``PipelinedLookup`` over objects of this class."""

  def __init__(self, tables16, coll, combiners='sum', wire='table', dedup=False, train=True, accums=None,   # pylint: disable=super-init-not-called
               moments=None, adam=None, ftrl_slots=None, ftrl=None, row_accums=None, rowwise_adagrad=None,
               rounding='nearest', seed=0, stores=None, initial_accumulator_value=0.1, max_norms=None,
               weight_grads=False, wire_dtype=None, hot_rows=False):
    what = 'LowpShardedHashGroupLookup'
    self.tables = list(tables16)
    _ht.same_device(self.tables)
    if any(t.dtype not in _ht.LOWP_DTYPES for t in self.tables):
      named = ', '.join(f'table {c}: {_ht._dtype_name(t.dtype)}' for c, t in enumerate(self.tables))   # pylint: disable=protected-access
      raise _ht._bad(f'{what}: every table must be a 16-bit HashTable (dtype=torch.bfloat16 / torch.float16), got '   # pylint: disable=protected-access
                     f'{named}: fp32 tables go through ShardedHashGroupLookup, a mix through two drivers')
    # (the four arguments below exist to be refused by name: only their defaults pass)
    if max_norms is not None:
      raise _ht._bad(f'{what}: max_norms is not supported for 16-bit tables (the clip reads and the clipped step '   # pylint: disable=protected-access
                     'writes fp32 rows)')
    if weight_grads is not False and weight_grads is not None:
      raise _ht._bad(f'{what}: weight_grads is not supported for 16-bit tables (the received rows are 16-bit)')   # pylint: disable=protected-access
    if wire_dtype is not None:
      raise _ht._bad(f"{what}: wire_dtype is not supported: a 16-bit plan names its wire with wire='table' | "   # pylint: disable=protected-access
                     "'float' (the fp16 wire rounds what it sends)")
    if hot_rows is not False and hot_rows is not None:
      raise _ht._bad(f'{what}: hot_rows is not supported for 16-bit tables (the low-precision gathers stage '   # pylint: disable=protected-access
                     'nothing)')
    if wire not in _lowp._WIRES:   # pylint: disable=protected-access
      raise _ht._bad(f"{what}: wire must be 'table' or 'float', got {wire!r}")   # pylint: disable=protected-access
    _lowp.check_rounding(rounding, seed, [t.dtype for t in self.tables], what)
    for c, t in enumerate(self.tables):
      if t.dim > 64 and t.dim % 4:
        raise _ht._bad(f'{what}: table {c}: dim {t.dim}: a sharded 16-bit hash table wider than 64 needs '   # pylint: disable=protected-access
                       'dim % 4 == 0 (the bound of the 16-bit gathers of the plan)')
    self.wire, self.rounding = wire, rounding
    self.seed = int(seed)
    self.rank_seed = _lowp.rank_seed(seed, int(getattr(coll, 'rank', 0)))
    self.train = bool(train)
    self.initial_accumulator_value = float(initial_accumulator_value)
    self._rows = [t.table for t in self.tables]
    self._apply = None
    self._own = None   # emit=False: per column (unique_rows, grad_rows, n_unique) this object owns
    ShardedGroupLookup.__init__(self, self._rows, coll, buckets=None, combiners=combiners, accums=accums, dedup=dedup,
                                moments=moments, adam=adam, ftrl_slots=ftrl_slots, ftrl=ftrl, row_accums=row_accums,
                                rowwise_adagrad=rowwise_adagrad)
    self._init_stores(stores)

  def _setup(self):
    """The step of the tables as they are now: a ``LowpSparseApply`` over the current row and slot tensors (built
    again by every :meth:`rebind`; the rounding's step counter carries over)."""
    self._lib = _lib.lib()
    old = self._apply
    self._apply = _lowp.LowpSparseApply(self.shards, accums=self.accums, rounding=self.rounding, seed=self.rank_seed,
                                        **_opt.slot_kwargs(self))
    if old is not None:
      self._apply.step_counter.copy_(old.step_counter)
    self._own = None

  def _create_plan(self):
    # the slots live with the apply: a 16-bit plan takes none (its stepping entries are refused)
    held = {cls.slot_kw: getattr(self, cls.slot_kw) for cls in _opt.TWO_SLOT.values()}
    for kw in held:
      setattr(self, kw, None)
    try:
      super()._create_plan()
    finally:
      for kw, slots in held.items():
        setattr(self, kw, slots)

  def _set_hash_tables(self, arr):
    n = len(self.tables)
    return self._lib.hbk_sharded_set_lowp_hash_tables(
      self._plan_handle, arr, (C.c_int32 * n)(*[_ht.LOWP_DTYPES[t.dtype] for t in self.tables]),
      _lowp._WIRES[self.wire])   # pylint: disable=protected-access

  @property
  def step_counter(self):
    return self._apply.step_counter

  def p2p_bind(self, outs):   # pylint: disable=unused-argument
    raise _lib.HbkError(_lib.UNIMPLEMENTED, 'LowpShardedHashGroupLookup: p2p_bind is not supported (the p2p form '
                        'has no owner-side translate and its owner gather stores fp32 rows)')

  def _phase(self, *args, **kwargs):   # pylint: disable=unused-argument
    raise _lib.HbkError(_lib.UNIMPLEMENTED, 'LowpShardedHashGroupLookup has no separate phase methods: the step runs '
                        'inside the plan (__call__ / launch / backward)')

  partition = owner_gather = stitch = stitch_bwd = owner_bwd = _phase

  _own_slices = _lowp.LowpShardedGroupLookup._own_slices     # pylint: disable=protected-access
  _apply_views = _lowp.LowpShardedGroupLookup._apply_views   # pylint: disable=protected-access

  def backward(self, grads, apply_lr=0.0, outs=None, optimizer='sgd', emit=True, finish=True, weight_grads=None):
    """Backward of the LAST forward step and, with ``apply_lr``, the optimizer step on the 16-bit tables.  Returns
    per column the IndexedSlices of this rank's table ``(unique_rows, grad_rows, n_unique)`` -- ``unique_rows`` are
    slot numbers -- equal to the fp32 driver's; ``emit=False`` (with ``apply_lr``): the slices go into buffers this
    object owns and the triples are ``(None, None, n_unique)``.  ``optimizer``: 'sgd', 'adagrad', 'adam', 'ftrl' or
    'rowwise_adagrad' (the slots given to the constructor); ``finish=True`` advances Adam's beta powers and the
    rounding's step counter once, behind the step.  ``weight_grads`` is refused."""
    if weight_grads is not False and weight_grads is not None:
      raise _ht._bad('LowpShardedHashGroupLookup: weight_grads is not supported for 16-bit tables (the received rows '   # pylint: disable=protected-access
                     'are 16-bit)')
    self._current()
    return _lowp.LowpShardedGroupLookup.backward(self, grads, apply_lr=apply_lr, outs=outs, optimizer=optimizer,
                                                 emit=emit, finish=finish)
