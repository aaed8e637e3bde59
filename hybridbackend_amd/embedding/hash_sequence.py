"""Hash-keyed sequence lookups: the behaviour histories of DIN / DIEN / BST (item and shop ids: an open
vocabulary that never stops growing) looked up through :class:`HashTable` rows instead of
``floormod(id, bucket)``.  Host side of ``hbk_hash_translate_sequence_n`` (include/hbk.h): a translate that reads
ids the way :class:`SequenceLookup` does -- the first ``T`` ids of every sample, a pad id or nothing past a
sample's length -- and leaves a ``[B * T]`` SLOT GRID on the device.

The existing calls do not compose.  ``sequence_row_grid(..., buckets=0)`` maps negative ids to ``-1`` and writes
``-1`` at padding positions, and ``-1`` is an ordinary key of a hash table; translating the whole ragged list
inserts the ids past ``T``, which would claim a key slot, a row and its optimizer slots for ever (and stay fresh in
an expiring table without ever being trained); padding with ``INT64_MIN`` counts every padding position in
``failed()``.

The gather over the slot grid and the whole backward already exist: :class:`HashSequenceLookup` is the translate
launch in front of the plain :class:`GroupLookup` (buckets 0) over the grid viewed as one id per position, and
``SequenceLookupGrad(hsl, ...)`` is its backward and optimizer step.

16-bit tables (``HashTable(..., dtype=torch.bfloat16 / torch.float16)``): a list that is 16-bit THROUGHOUT goes through
``hbk_hash_translate_sequence_lowp_n`` -- the same translate, whose inserting launch rounds the start row to the
table's 16 bits -- and :class:`HashSequenceLookup` gathers with a ``LowpGroupLookup`` (fp32 outputs, the rows upcast
exactly); :class:`LowpSequenceLookupGrad` is the step.  A list that mixes fp32 and 16-bit tables is refused by name.

Tiered tables: :meth:`HashSequenceLookup.fault_in` brings back, before the call of a step, the spilled keys among
the ids the call will read -- the first ``T`` ids of every sample and the pad id, never an id past ``T``
(:func:`hash_missing_sequence`, ``hbk_hash_missing_n``).

As a column of a layer, and sharded over W ranks: ``feature_column.HashSequenceEmbeddingColumn`` in
``SequenceFeatures`` (the sharded form goes through ``ShardedHashGroupLookup`` over ``sequence_id_grid``).

Not provided: per-id weights, fp16 outputs, the TF shim op.
"""
import ctypes as C

import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding.cache import EMPTY_KEY
from hybridbackend_amd.embedding.hashtable import LOWP_DTYPES
from hybridbackend_amd.embedding.hashtable import TOMBSTONE_KEY
from hybridbackend_amd.embedding.hashtable import _Plan
from hybridbackend_amd.embedding.hashtable import _missing
from hybridbackend_amd.embedding.hashtable import hash_fault_in
from hybridbackend_amd.embedding.hashtable import check_bound
from hybridbackend_amd.embedding.hashtable import check_current
from hybridbackend_amd.embedding.hashtable import require_fp32_tables
from hybridbackend_amd.embedding.hashtable import check_ids
from hybridbackend_amd.embedding.hashtable import evict_tables
from hybridbackend_amd.embedding.hashtable import grow_tables
from hybridbackend_amd.embedding.hashtable import remove_tables
from hybridbackend_amd.embedding.hashtable import same_device
from hybridbackend_amd.embedding.lookup import GroupLookup
from hybridbackend_amd.embedding.lookup import max_norm_list
from hybridbackend_amd.embedding.sequence import SequenceLookupGrad
from hybridbackend_amd.embedding.sequence import per_column


def _bad(msg):
  return _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, msg)


_ONE_DTYPE = ('one translate call writes new rows, and one gather reads them, as fp32 rows or as 16-bit rows: a '
              'hash-keyed sequence lookup takes tables that are fp32 throughout or 16-bit throughout (two objects serve '
              'a mix)')


def _all_lowp(tables, what):
  """True when every table has 16-bit rows, False when every table is fp32; a mix is refused, naming the first 16-bit
  table."""
  lowp = [t.dtype in LOWP_DTYPES for t in tables]
  if lowp and all(lowp):
    return True
  require_fp32_tables(tables, what, _ONE_DTYPE)
  return False


def check_hash_sequence_args(tables, max_lens, pad_ids):
  """The per-column ``(max_lens, pad_ids)`` lists: ``max_len >= 1``; a ``pad_id`` is a RAW id, any int64 the
  table can store (not ``INT64_MIN``; on an expiring table not ``INT64_MIN + 1`` either)."""
  n = len(tables)
  if max_lens is None:
    raise _bad('max_lens is required: the padded length of every column')
  max_lens = per_column(max_lens, n, 'max_lens')
  pad_ids = per_column(pad_ids, n, 'pad_ids', none_ok=True)
  for c in range(n):
    if not 1 <= max_lens[c] < 2 ** 31:
      raise _bad(f'max_len of column {c} must be in [1, 2^31), got {max_lens[c]}')
    p = pad_ids[c]
    if p is None:
      continue
    if not -2 ** 63 <= p < 2 ** 63:
      raise _bad(f'pad_id of column {c} must be an int64, got {p}')
    if p == EMPTY_KEY or (tables[c].expiring and p == TOMBSTONE_KEY):
      raise _bad(f'pad_id of column {c} is a sentinel of the table ({p}): it is never stored')
  return max_lens, pad_ids


class _SeqPlan(_Plan):
  """:class:`_Plan` with one ``hbk_hash_sequence_t`` per column, grouped with the columns: ``seqs[c]`` is column
  c's record.  One ``hbk_hash_translate_sequence_n`` call per table kind; the groups of 16-bit tables (``dtypes[g]``
  their element codes) go through ``hbk_hash_translate_sequence_lowp_n``."""

  def __init__(self, tables):
    super().__init__(tables)
    self.seqs = [None] * len(tables)
    self._seq_groups = []
    at = {C.addressof(col): c for c, col in enumerate(self.cols)}
    for _, _, cols, _, _ in self.groups:
      seqs = (_lib.HashSequence * len(cols))()
      for k in range(len(cols)):
        self.seqs[at[C.addressof(cols[k])]] = seqs[k]
      self._seq_groups.append(seqs)

  def launch(self, insert, stream):
    insert = 1 if insert else 0
    f = _lib.lib().hbk_hash_translate_sequence_n
    if not self.groups:
      _lib.check(f(0, None, None, None, None, insert, stream))
    for (_, _, cols, expiry, adm), dtypes, seqs in zip(self.groups, self.dtypes, self._seq_groups):
      if dtypes is not None:
        _lib.check(_lib.lib().hbk_hash_translate_sequence_lowp_n(len(cols), cols, expiry, adm, dtypes, seqs, insert,
                                                                 stream))
      else:
        _lib.check(f(len(cols), cols, expiry, adm, seqs, insert, stream))


def _bind(plan, tables, ids, row_splits, max_lens, pad_ids, insert, outs, lengths=None):
  """Point the descriptors of ``plan`` at one step's tensors; returns ``(grids, lengths)`` (allocated where not
  given)."""
  n = len(tables)
  check_ids(ids, tables)
  row_splits = [None] * n if row_splits is None else list(row_splits)
  if len(row_splits) != n:
    raise _bad(f'expected {n} row_splits, got {len(row_splits)}')
  outs = [None] * n if outs is None else list(outs)
  if len(outs) != n:
    raise _bad(f'expected {n} outputs, got {len(outs)}')
  batch = []
  for c in range(n):
    s = row_splits[c]
    if s is not None:
      _lib.require_device_tensor(s, 'row_splits')
      if s.dtype != torch.int32 or s.dim() != 1 or s.numel() < 1 or s.device != ids[c].device:
        raise _bad(f'row_splits of column {c} must be an int32 vector [samples+1] on {ids[c].device}')
    b = ids[c].numel() if s is None else s.numel() - 1
    if b * max_lens[c] >= 2 ** 31:
      raise _bad(f'column {c}: {b} samples x max_len {max_lens[c]} positions, must stay below 2^31')
    batch.append(b)
  dev = tables[0].keys.device if n else None
  if lengths is None:
    flat = torch.empty(sum(batch), dtype=torch.int32, device=dev)
    lengths = list(torch.split(flat, batch)) if batch else []
  for c in range(n):
    i, t, q = ids[c], tables[c], plan.seqs[c]
    positions = batch[c] * max_lens[c]
    if outs[c] is None:
      outs[c] = torch.empty(positions, dtype=torch.int64, device=dev)
    o = outs[c]
    if not isinstance(o, torch.Tensor) or o.dtype != torch.int64 or tuple(o.shape) != (positions,) or \
        o.device != i.device or not o.is_contiguous():
      raise _bad(f'output {c} must be a contiguous int64 [{positions}] tensor on {i.device}')
    # a find counts nothing: `counts` is the table's record of what was inserted and refused
    t._describe(plan.cols[c], init=bool(insert), count=bool(insert))
    plan.cols[c].keys = i.data_ptr() if i.numel() else None
    plan.cols[c].n_keys = i.numel()
    plan.cols[c].slots = o.data_ptr() if positions else None
    q.row_splits = row_splits[c].data_ptr() if row_splits[c] is not None else None
    q.n_segments = batch[c]
    q.max_len = max_lens[c]
    q.has_pad = 0 if pad_ids[c] is None else 1
    q.pad_id = pad_ids[c] or 0
    q.lengths = lengths[c].data_ptr() if batch[c] else None
  return outs, lengths, row_splits


def hash_translate_sequence(tables, ids, row_splits=None, max_lens=None, pad_ids=None, insert=True, outs=None):
  """The first ``T_c`` ids of every sample -> row numbers, for N columns (``hbk_hash_translate_sequence_n``; plain,
  expiring and filtered tables may be mixed: one entry call per kind, the filtered ones in two launches).  The
  tables are fp32 throughout or 16-bit throughout (``hbk_hash_translate_sequence_lowp_n``: a new row is the fp32
  start row rounded to nearest even).

  ids[c]: int64 raw ids, row_splits[c]: int32 ``[B + 1]`` or None (one id per sample).  ``pad_ids``: None --
  positions past a sample's length are ``-1`` in the grid and touch nothing -- or the RAW id such positions look
  up, inserted and counted like any id of the data.  Ids past ``T_c`` are never read.  ``insert=False``: a pure
  find.  ``outs``: preallocated int64 ``[B * T_c]`` grids.

  Returns ``(slot_grids, lengths)``: per column int64 ``[B * T_c]`` (position ``b * T_c + t``) and int32 ``[B]``
  ``min(len, T_c)``.  The table, its counters and metadata and the sketch change exactly as ``hash_translate``
  on the effective id list (per sample its first ``min(len, T)`` ids, then the pad ids) would change them."""
  tables, ids = list(tables), list(ids)
  same_device(tables)
  _all_lowp(tables, 'hash_translate_sequence')
  max_lens, pad_ids = check_hash_sequence_args(tables, max_lens, pad_ids)
  plan = _SeqPlan(tables)
  grids, lengths, _ = _bind(plan, tables, ids, row_splits, max_lens, pad_ids, insert, outs)
  dev = tables[0].keys.device if tables else None
  plan.launch(insert, _lib.current_stream(dev))
  return grids, lengths


def hash_missing_sequence(tables, ids, row_splits=None, max_lens=None, pad_ids=None):
  """:func:`hybridbackend_amd.embedding.hash_missing` on the EFFECTIVE id lists (``hbk_hash_missing_n`` with a
  sequence record per column): per expiring table the distinct ids among the first ``T_c`` ids of every sample --
  and the pad id, where a sample is shorter than ``T_c`` and ``pad_ids[c]`` is given -- that the table does not hold,
  a device int64 tensor in the order of their first occurrence by position ``b * T_c + t``.  Ids past ``T_c`` are
  never read.  The arguments are those of :func:`hash_translate_sequence`.  One C call, one host read (all
  counts); the tables are not written."""
  tables, ids = list(tables), list(ids)
  same_device(tables)
  max_lens, pad_ids = check_hash_sequence_args(tables, max_lens, pad_ids)
  row_splits = [None] * len(tables) if row_splits is None else list(row_splits)
  if len(row_splits) != len(tables):
    raise _bad(f'expected {len(tables)} row_splits, got {len(row_splits)}')
  return _missing(tables, ids, (row_splits, max_lens, pad_ids))[0]


class HashSequenceLookup:
  """N hash-keyed sequence columns: one translate launch (``hbk_hash_translate_sequence_n``), then the plain
  :class:`GroupLookup` with buckets 0 over the slot grid viewed as one id per position, so a ``-1`` reads a zero
  row.

  Two launches, not one: a concurrent duplicate of a new id can hit the freshly claimed slot before the winner
  has written its row, so the row write and the gather need a kernel boundary between them.

  Args:
    tables: list of :class:`HashTable` on one device.
    max_lens: the padded length T of every column (one value for all, or one per column): a sample's first T
      ids are looked up, later ones are never read -- they are not inserted, not counted, not kept fresh.
    pad_ids: None -- positions past a sample's length are ZERO rows and take part in nothing -- or the RAW id
      such positions look up (any int64 the table can store): its row collects the gradient of every padding
      position.  One for all columns or one per column.
    max_norms: TF's ``max_norm``: every looked-up row, pad rows included, is clipped as in :class:`GroupLookup`.
    train: True -- ids never seen are inserted; False -- nothing is inserted, they read as zero rows.

  After a call: ``grids`` (the slot grids, int64 ``[B * T_c]``), ``lengths``, and with ``tables`` (the ROW
  tensors), ``dims`` and :meth:`plain_lookup` what ``SequenceLookupGrad(hsl, accums=..., ...)`` reads of a
  lookup: the backward and optimizer step, every reduce plan, ``deterministic=True``, the clip, SGD, Adagrad,
  Lazy Adam and FTRL unchanged.  ``hash_tables`` are the :class:`HashTable` objects.

  16-bit tables (all of them: a mix with fp32 tables is refused by name): the translate is
  ``hbk_hash_translate_sequence_lowp_n``, :meth:`plain_lookup` a ``LowpGroupLookup`` with buckets 0 and
  ``wide_rows=True`` -- outputs stay fp32, bit for bit those of the fp32 object over the upcast tables -- and the
  step is :class:`LowpSequenceLookupGrad`.  ``max_norms`` is refused there by name; ``launch()``, captured graphs,
  ``maybe_grow``, ``maybe_evict``, ``remove`` and ``fault_in`` are what they are on fp32 tables.
  """

  def __init__(self, tables, max_lens, pad_ids=None, max_norms=None, train=True):
    self.hash_tables = list(tables)
    same_device(self.hash_tables)
    self.lowp = _all_lowp(self.hash_tables, 'HashSequenceLookup')
    self.max_lens, self.pad_ids = check_hash_sequence_args(self.hash_tables, max_lens, pad_ids)
    self.max_norms = max_norm_list(max_norms, len(self.hash_tables))
    if self.lowp and any(self.max_norms):
      raise _bad('HashSequenceLookup: max_norms is not supported for 16-bit tables (the clip reads and the clipped '
                 'step writes fp32 rows)')
    self.train = bool(train)
    self.dims = [t.dim for t in self.hash_tables]
    self.rebind()

  def rebind(self):
    """After a rehash of a table (``hash_rehash``, :meth:`HashTable.maybe_grow`): the plain lookup is built again
    over the tables' current row tensors and the bound state is dropped -- :meth:`launch` refuses until the next
    call.  Slot numbers and tensor addresses changed: a ``SequenceLookupGrad`` built on this lookup before must
    be rebuilt (with the companions the rehash returned), and a captured graph captured again."""
    self.tables = [t.table for t in self.hash_tables]
    if self.lowp:
      from hybridbackend_amd.embedding.lowp import LowpGroupLookup   # pylint: disable=import-outside-toplevel
      self._plain = LowpGroupLookup(self.tables, buckets=None, combiners='sum', wide_rows=True)
    else:
      self._plain = GroupLookup(self.tables, buckets=None, combiners='sum',
                                max_norms=[m or None for m in self.max_norms])
    self._plan = _SeqPlan(self.hash_tables)
    self.grids = None
    self.lengths = None
    self._keep = None
    self._bound = False

  def maybe_grow(self, max_load=0.75, factor=2.0, slots=None):
    """:meth:`HashTable.maybe_grow` on every table (``slots[c]``: the companions of table c), then
    :meth:`rebind` if any table was rehashed.  Returns the per-table results: None, or the new companion
    tensors."""
    return grow_tables(self, self.hash_tables, max_load, factor, slots)

  def maybe_evict(self, max_load=0.75, target_load=0.5, keep_freq=0, slots=None, order='lru'):
    """:meth:`HashTable.maybe_evict` on every table (``slots[c]``: the companions of table c; ``order``: ``'lru'``
    or ``'lfu'``), then
    :meth:`rebind` if any table was rehashed.  Returns the per-table results: None, or the new companion
    tensors."""
    return evict_tables(self, self.hash_tables, max_load, target_load, keep_freq, slots, order=order)

  def remove(self, ids_list, slots=None, stores=None):
    """:meth:`HashGroupLookup.remove`: the ids of ``ids_list[c]`` leave table c (``slots[c]``: its ``(tensor,
    fill_value)`` companions, ``stores[c]``: its spill store or None).  The row tensors do not move, so no
    :meth:`rebind` is needed; slots handed out earlier for the removed ids are void.  Returns the old slots per
    table."""
    return remove_tables(self.hash_tables, ids_list, slots, stores)

  def fault_in(self, ids, row_splits, stores, slots=None):
    """:meth:`HashGroupLookup.fault_in` for sequence columns, before the call of the step (:func:`hash_fault_in`
    with this object's ``max_lens`` and ``pad_ids``): of ``ids[c]`` / ``row_splits[c]`` only what the call will
    read is asked of ``stores[c]`` -- the first ``T_c`` ids of every sample and, where a sample is shorter, the pad
    id.  An id that occurs only past ``T_c`` stays in the store; a pad id the store holds comes back.  ``slots[c]``:
    the companion tensors of table c.  The row tensors do not move, so no :meth:`rebind` is needed.  Returns the
    keys restored per table."""
    return hash_fault_in(self.hash_tables, ids, stores, slots, row_splits, self.max_lens, self.pad_ids)

  def __len__(self):
    return len(self.hash_tables)

  def plain_lookup(self):
    """The lookup over a slot grid: the tables' rows as one-id-per-position columns, buckets 0.  What the second
    launch gathers with and the backward differentiates."""
    return self._plain

  def __call__(self, ids, row_splits=None, outs=None):
    """ids[c]: int64 raw ids, row_splits[c]: int32 ``[B + 1]`` or None (one id per sample).  Returns
    ``(outs, lengths)``: per column fp32 ``[B, T_c, dim_c]`` (or the caller's contiguous ``outs[c]`` of that
    shape) and int32 ``[B]`` ``min(len, T_c)``."""
    ids = list(ids)
    check_current(self.hash_tables, self.tables)
    n = len(self.hash_tables)
    # the grids of the call before serve again while the shapes stay (a resident loop; a captured launch()
    # needs them to stay where they are)
    keep = self.grids
    if keep is not None:
      splits = [None] * n if row_splits is None else list(row_splits)
      if len(ids) != n or len(splits) != n or any(
          not isinstance(i, torch.Tensor) or not isinstance(s, (torch.Tensor, type(None))) or
          k.numel() != (i.numel() if s is None else s.numel() - 1) * t
          for k, i, s, t in zip(keep, ids, splits, self.max_lens)):
        keep = None
    grids, lengths, row_splits = _bind(self._plan, self.hash_tables, ids, row_splits, self.max_lens, self.pad_ids,
                                       self.train, keep)
    dev = self.hash_tables[0].keys.device if n else None
    outs = [None] * n if outs is None else list(outs)
    if len(outs) != n:
      raise _bad(f'expected {n} outputs, got {len(outs)}')
    views = []
    for c in range(n):
      shape = (lengths[c].numel(), self.max_lens[c], self.dims[c])
      if outs[c] is None:
        outs[c] = torch.empty(shape, dtype=torch.float32, device=dev)
      o = outs[c]
      if not isinstance(o, torch.Tensor) or not o.is_cuda or o.dtype != torch.float32 or \
          tuple(o.shape) != shape or not o.is_contiguous():
        raise _bad(f'output {c} must be a contiguous fp32 device tensor {list(shape)}')
      views.append(o.view(shape[0] * shape[1], shape[2]))
    self._plain.bind(grids, None, views)
    self._keep = (ids, row_splits, outs, views)
    self.grids, self.lengths = grids, lengths
    self._bound = True
    self._launch(None)
    return outs, lengths

  def _launch(self, stream):
    dev = self.hash_tables[0].keys.device if self.hash_tables else None
    s = _lib.current_stream(dev) if stream is None else C.c_void_p(stream.cuda_stream)
    self._plan.launch(self.train, s)
    self._plain.launch(stream)

  def launch(self, stream=None):
    """Both launches of the LAST call again on its tensors (ids and row_splits refilled in place; captured
    graphs): two foreign calls (three with filtered tables of both kinds), no allocation."""
    check_bound(self, self.hash_tables, self.tables)
    self._launch(stream)


class LowpSequenceLookupGrad:
  """Backward and optimizer step of a :class:`HashSequenceLookup` over 16-bit tables, the named form of
  ``LowpLookupGrad(hsl.plain_lookup(), ...)`` over ``hsl.grids`` with the ``[B, T, dim]`` gradients viewed
  ``[B * T, dim]`` -- what :class:`SequenceLookupGrad` is to the fp32 object.  The slots (``accums`` / ``moments`` /
  ``adam`` / ``ftrl_slots`` / ``ftrl`` / ``row_accums`` / ``rowwise_adagrad``) are fp32 and have the tables' shapes;
  ``deterministic``, ``rounding`` and ``seed`` are ``LowpLookupGrad``'s.  Truncated ids and zero padding are not in
  the grid: they reach no gradient row and no slot; with ``pad_ids`` the pad row collects the gradient of every
  padding position.  Rebuilt after a rehash, with the companions the rehash returned, as a ``SequenceLookupGrad``
  is."""

  def __init__(self, lookup, accums=None, moments=None, adam=None, ftrl_slots=None, ftrl=None, row_accums=None,
               rowwise_adagrad=None, deterministic=False, rounding='nearest', seed=0):
    if not isinstance(lookup, HashSequenceLookup) or not lookup.lowp:
      raise _bad('LowpSequenceLookupGrad needs a HashSequenceLookup over 16-bit tables (fp32 tables go through '
                 'SequenceLookupGrad)')
    from hybridbackend_amd.embedding.lowp import LowpLookupGrad   # pylint: disable=import-outside-toplevel
    self.lookup = lookup
    self.inner = LowpLookupGrad(lookup.plain_lookup(), accums=accums, moments=moments, adam=adam,
                                ftrl_slots=ftrl_slots, ftrl=ftrl, row_accums=row_accums,
                                rowwise_adagrad=rowwise_adagrad, deterministic=deterministic, rounding=rounding,
                                seed=seed)

  @property
  def step_counter(self):
    return self.inner.step_counter

  _rows_view = SequenceLookupGrad._rows_view   # pylint: disable=protected-access

  def __call__(self, grads, apply_lr=0.0, optimizer='sgd', emit=True, finish=True, grids=None):
    """grads[c]: the gradient of the last forward's ``outs[c]``.  Returns what ``LowpLookupGrad`` returns: per column
    ``(unique_rows, grad_rows, n_unique)`` (capacity ``B * T``; slot numbers).  ``grids``: explicit slot grids for a
    backward without a forward."""
    check_current(self.lookup.hash_tables, self.inner.lookup.tables)
    grids = self.lookup.grids if grids is None else list(grids)
    if grids is None:
      raise _bad('LowpSequenceLookupGrad: the lookup kept no grids: call it first, or pass grids=')
    n = len(self.lookup)
    if len(grads) != n or len(grids) != n:
      raise _bad(f'expected {n} gradients and grids, got {len(grads)} and {len(grids)}')
    rows = [self._rows_view(c, grads[c], int(grids[c].numel())) for c in range(n)]
    return self.inner(grids, rows, None, apply_lr=apply_lr, optimizer=optimizer, emit=emit, finish=finish)
