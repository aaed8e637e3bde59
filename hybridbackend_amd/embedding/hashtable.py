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

Not provided: admission filters / automatic growth (a full table answers -1; ``items()`` / ``load()`` into a
larger table is the way to grow), sharded hash tables, feature-column integration, the TF shim op.
"""
import ctypes as C
import math

import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding.cache import EMPTY_KEY
from hybridbackend_amd.embedding.lookup import GroupLookup

TOMBSTONE_KEY = EMPTY_KEY + 1   # expiring tables only: a slot the eviction sweep took back


def _bad(msg):
  return _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, msg)


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

  Attributes of an expiring table: ``last_seen`` / ``freq`` int32 ``[capacity]`` (the step of a slot's last
  translate with ``insert=True`` and its occurrences so far, saturating at 2^30), ``step`` int32 ``[1]`` on
  the device (:meth:`set_step`), ``stats`` int32 ``[2]`` = keys evicted / keys stored into a reused slot.

  Attributes: ``keys`` int64 ``[slab_count * slab_size]`` (EMPTY = INT64_MIN), ``table`` fp32
  ``[capacity, dim]``, ``counts`` int32 ``[2]`` = keys inserted / id occurrences refused (table full) so far.
  """

  def __init__(self, capacity, dim, device, slab_size=8, init_scale=1e-3, seed=0, expiring=False):
    slab_size, capacity, dim = int(slab_size), int(capacity), int(dim)
    if not 1 <= slab_size <= 64:
      raise _bad(f'slab_size must be in [1, 64], got {slab_size}')
    if capacity < slab_size:
      raise _bad(f'capacity {capacity} is below one slab of {slab_size} slots')
    if dim < 1:
      raise _bad(f'dim must be >= 1, got {dim}')
    init_scale = float(init_scale)
    if not math.isfinite(init_scale) or init_scale < 0 or not math.isfinite(C.c_float(init_scale).value):
      raise _bad(f'init_scale must be finite and >= 0, got {init_scale!r}')
    self.slab_size = slab_size
    self.slab_count = capacity // slab_size
    self.capacity = self.slab_count * slab_size
    self.dim = dim
    self.init_scale = init_scale
    self.seed = int(seed)
    self.device = torch.device(device)
    self.keys = torch.full((self.capacity,), EMPTY_KEY, dtype=torch.int64, device=self.device)
    self.table = torch.zeros((self.capacity, dim), dtype=torch.float32, device=self.device)
    self.counts = torch.zeros(2, dtype=torch.int32, device=self.device)
    self.expiring = bool(expiring)
    if self.expiring:
      self.last_seen = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
      self.freq = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
      self.step = torch.zeros(1, dtype=torch.int32, device=self.device)
      self.stats = torch.zeros(2, dtype=torch.int32, device=self.device)

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

  def _need_expiring(self, what):
    if not self.expiring:
      raise _bad(f'{what} needs a table built with expiring=True')

  def _live(self):
    """Mask of the slots that hold a key."""
    live = self.keys != EMPTY_KEY
    return live & (self.keys != TOMBSTONE_KEY) if self.expiring else live

  def lookup_or_insert(self, ids):
    """Row number of every id, int64 ``[n]``; ids never seen are inserted and their rows initialised; -1
    where the table is full (and for id == INT64_MIN)."""
    return hash_translate([self], [ids], insert=True)[0]

  def find(self, ids):
    """Row number of every id or -1; nothing is inserted."""
    return hash_translate([self], [ids], insert=False)[0]

  def size(self):
    """Keys the table holds: inserted so far, less evicted (syncs the host).  After ``keys`` was written from
    outside (a restored checkpoint) call :meth:`recount` first."""
    n = int(self.counts[0].item())
    return n - int(self.stats[0].item()) if self.expiring else n

  def failed(self):
    """Id occurrences refused so far because the table was full (syncs the host)."""
    return int(self.counts[1].item())

  def recount(self):
    """Set the inserted counter from ``keys`` (after a restore of the raw arrays) and clear the failures
    (and, of an expiring table, the evicted / reused counters: ``size()`` is the live keys again)."""
    self.counts[0] = self._live().sum().to(torch.int32)
    self.counts[1] = 0
    if self.expiring:
      self.stats.zero_()

  def items(self):
    """``(keys, rows)`` of the occupied slots, sorted by key: the geometry-free form of the table."""
    occupied = self._live()
    keys = self.keys[occupied]
    order = torch.argsort(keys)
    return keys[order], self.table[occupied][order]

  def load(self, keys, rows):
    """Insert ``keys`` (without initialising) and store ``rows`` as their rows: ``load(*other.items())``
    moves a table into one of any capacity or slab size.  Refuses when a key does not fit."""
    check_ids([keys], [self])
    if rows.dtype != torch.float32 or tuple(rows.shape) != (keys.numel(), self.dim) or \
        rows.device != self.table.device:
      raise _bad(f'rows must be fp32 [{keys.numel()}, {self.dim}] on {self.table.device}')
    slots = _translate([self], [keys], True, None, init=False)[0]
    ok = slots >= 0
    if not bool(ok.all().item()):
      raise _bad(f'load: {int((~ok).sum().item())} of {keys.numel()} keys do not fit: the table is full')
    self.table[slots] = rows
    return slots

  def variables(self, name):
    """The raw arrays for ``training.saver.Saver``: they restore into a table of the SAME geometry
    (capacity, slab_size); then :meth:`recount`.  ``items()`` / ``load()`` is the geometry-free form."""
    out = {name + '/keys': self.keys, name + '/embedding_weights': self.table}
    if self.expiring:
      out[name + '/last_seen'] = self.last_seen
      out[name + '/freq'] = self.freq
    return out

  # ---- expiry -------------------------------------------------------------------------------------------
  def set_step(self, n):
    """The current step, on the device: an in-place fill (capturable; replayed launches see it)."""
    self._need_expiring('set_step')
    self.step.fill_(int(n))

  def evict(self, steps_to_live, keep_freq=0, slots=()):
    """One sweep launch (``hbk_hash_evict_n``): a key whose slot was last seen ``steps_to_live`` or more steps
    ago -- and, with ``keep_freq > 0``, was seen fewer than ``keep_freq`` times -- leaves the table; its slot
    becomes a TOMBSTONE that later inserts reuse.  ``slots``: up to 4 ``(tensor, fill_value)`` pairs, the
    optimizer slots (fp32 ``[capacity, d]``), whose rows of the evicted slots are set to ``fill_value``
    (Adagrad: ``initial_accumulator_value``).  Must not run beside a translate of the table on another
    stream.  Returns nothing and does not sync."""
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


def hash_evict(tables, steps_to_live, keep_freq=0, slots=None):
  """:meth:`HashTable.evict` for N expiring tables in ONE launch.  ``slots[c]``: the ``(tensor, fill_value)``
  pairs of table ``c`` (None: no table has any)."""
  tables = list(tables)
  cols, _ = _evict_columns(tables, steps_to_live, keep_freq, slots)
  dev = tables[0].keys.device if tables else None
  _lib.check(_lib.lib().hbk_hash_evict_n(len(tables), cols, _lib.current_stream(dev)))


def _evict_columns(tables, steps_to_live, keep_freq, slots):
  """The checked descriptors of one sweep call (and the tensors they point into)."""
  same_device(tables)
  steps_to_live, keep_freq = int(steps_to_live), int(keep_freq)
  if steps_to_live < 0 or keep_freq < 0:
    raise _bad(f'steps_to_live and keep_freq must be >= 0, got {steps_to_live} and {keep_freq}')
  slots = [()] * len(tables) if slots is None else list(slots)
  if len(slots) != len(tables):
    raise _bad(f'expected {len(tables)} lists of companion tensors, got {len(slots)}')
  for t in tables:
    t._need_expiring('evict')
  checked = [_companions(t, slots[c]) for c, t in enumerate(tables)]
  cols = (_lib.HashEvictColumn * len(tables))()
  for c, t in enumerate(tables):
    _lib.require_device_tensor(t.keys, 'keys')
    col = cols[c]
    col.keys_cache, col.slab_count, col.slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
    t._describe_expiry(col.exp)
    col.steps_to_live, col.keep_freq = steps_to_live, keep_freq
    pairs = checked[c]
    col.n_fills = len(pairs)
    for f, (x, value) in enumerate(pairs):
      col.fills[f].base, col.fills[f].pitch, col.fills[f].dim = x.data_ptr(), x.stride(0), x.shape[1]
      col.fills[f].value = value
  return cols, checked


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
  expiring ones' (with their expiry records) for ``hbk_hash_insert_expiring_n``.  ``cols[c]`` is table c's."""

  def __init__(self, tables):
    plain = [c for c, t in enumerate(tables) if not t.expiring]
    expiring = [c for c, t in enumerate(tables) if t.expiring]
    self.plain = (_lib.HashColumn * len(plain))()
    self.expiring = (_lib.HashColumn * len(expiring))()
    self.expiry = (_lib.HashExpiry * len(expiring))()
    self.cols = [None] * len(tables)
    for k, c in enumerate(plain):
      self.cols[c] = self.plain[k]
    for k, c in enumerate(expiring):
      self.cols[c] = self.expiring[k]
      tables[c]._describe_expiry(self.expiry[k])

  def launch(self, insert, stream):
    insert = 1 if insert else 0
    if len(self.plain) or not len(self.expiring):
      _lib.check(_lib.lib().hbk_hash_insert_n(len(self.plain), self.plain, insert, stream))
    if len(self.expiring):
      _lib.check(_lib.lib().hbk_hash_insert_expiring_n(len(self.expiring), self.expiring, self.expiry, insert,
                                                       stream))


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
  """ids -> row numbers for N columns in ONE launch (``hbk_hash_insert_n``; plain and expiring tables may be
  mixed: the expiring ones go through ``hbk_hash_insert_expiring_n`` in a second launch).  ``insert=False``:
  a pure find (-1 for ids never seen).  ``outs``: preallocated int64 ``[n_ids]`` tensors.  Returns the list
  of slots."""
  tables = list(tables)
  same_device(tables)
  return _translate(tables, list(ids_list), insert, outs)


def same_device(tables):
  for c, t in enumerate(tables):
    if not isinstance(t, HashTable):
      raise _bad(f'table {c} must be a HashTable')
    if t.keys.device != tables[0].keys.device:
      raise _bad(f'tables must live on one device: table {c} is on {t.keys.device}, table 0 on '
                 f'{tables[0].keys.device}')


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
  """

  def __init__(self, tables, combiners='sum', max_norms=None, train=True):
    self.tables = list(tables)
    same_device(self.tables)
    self.train = bool(train)
    self.lookup = GroupLookup([t.table for t in self.tables], buckets=None, combiners=combiners,
                              max_norms=max_norms)
    self._plan = _Plan(self.tables)
    self.slots = None
    self._bound = False

  def __len__(self):
    return len(self.tables)

  def __call__(self, ids, row_splits=None, outs=None, sp_weights=None):
    """ids[c]: int64 raw ids, row_splits[c]: int32 ``[segments + 1]`` or None.  Returns GroupLookup's outputs."""
    ids = list(ids)
    # the slot buffers of the call before serve again while the id counts stay (a resident loop; a
    # captured launch() needs them to stay where they are)
    keep = self.slots
    if keep is not None and (len(keep) != len(ids) or any(
        not isinstance(i, torch.Tensor) or s.numel() != i.numel() for s, i in zip(keep, ids))):
      keep = None
    self.slots = _translate(self.tables, ids, self.train, keep, plan=self._plan)
    self._keep = ids
    self._bound = True
    return self.lookup(self.slots, row_splits, outs, sp_weights=sp_weights)

  def launch(self, stream=None):
    """Both launches of the LAST call again on its tensors (id buffers refilled in place; captured graphs):
    two foreign calls, no allocation."""
    if not self._bound:
      raise _lib.HbkError(_lib.INTERNAL, 'launch() needs a call that bound the tensors first')
    dev = self.tables[0].keys.device if self.tables else None
    s = _lib.current_stream(dev) if stream is None else C.c_void_p(stream.cuda_stream)
    self._plan.launch(self.train, s)
    self.lookup.launch(stream)
