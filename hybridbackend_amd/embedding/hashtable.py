"""Hash-keyed embedding tables: rows addressed by the RAW int64 id instead of ``floormod(id, num_buckets)``,
so two ids never share a row, its gradient and its optimizer slots (DeepRec's EmbeddingVariable; the
reference's ``EmbeddingService``, hybridbackend/tensorflow/embedding/service.py:153-283, in miniature).
Host side of ``hbk_hash_insert_n`` (include/hbk.h): a device find-or-insert that turns ids into row numbers
of a fixed-capacity table whose key array is exactly the slab cache ``hb.embedding.cache.probe`` reads.

The row numbers then feed the existing lookups with ``bucket = 0``: :class:`HashGroupLookup` is one
translate launch in front of a :class:`GroupLookup`, and ``GroupLookupGrad(hgl.lookup, ...)`` called on
``hgl.slots`` is its backward and optimizer step -- every reduce plan, ``deterministic=True``, max_norm,
weights, SGD, Adagrad, Lazy Adam and FTRL unchanged.

Not provided: admission / eviction / automatic growth (a full table answers -1; ``items()`` / ``load()``
into a larger table is the way to grow), sharded hash tables, feature-column integration, the TF shim op.
"""
import ctypes as C
import math

import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding.cache import EMPTY_KEY
from hybridbackend_amd.embedding.lookup import GroupLookup


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

  Attributes: ``keys`` int64 ``[slab_count * slab_size]`` (EMPTY = INT64_MIN), ``table`` fp32
  ``[capacity, dim]``, ``counts`` int32 ``[2]`` = keys inserted / id occurrences refused (table full) so far.
  """

  def __init__(self, capacity, dim, device, slab_size=8, init_scale=1e-3, seed=0):
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

  def lookup_or_insert(self, ids):
    """Row number of every id, int64 ``[n]``; ids never seen are inserted and their rows initialised; -1
    where the table is full (and for id == INT64_MIN)."""
    return hash_translate([self], [ids], insert=True)[0]

  def find(self, ids):
    """Row number of every id or -1; nothing is inserted."""
    return hash_translate([self], [ids], insert=False)[0]

  def size(self):
    """Keys inserted so far (syncs the host).  After ``keys`` was written from outside (a restored
    checkpoint) call :meth:`recount` first."""
    return int(self.counts[0].item())

  def failed(self):
    """Id occurrences refused so far because the table was full (syncs the host)."""
    return int(self.counts[1].item())

  def recount(self):
    """Set the inserted counter from ``keys`` (after a restore of the raw arrays) and clear the failures."""
    self.counts[0] = (self.keys != EMPTY_KEY).sum().to(torch.int32)
    self.counts[1] = 0

  def items(self):
    """``(keys, rows)`` of the occupied slots, sorted by key: the geometry-free form of the table."""
    occupied = self.keys != EMPTY_KEY
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
    return {name + '/keys': self.keys, name + '/embedding_weights': self.table}


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


def _translate(tables, ids_list, insert, outs, init=True, cols=None):
  n = len(tables)
  check_ids(ids_list, tables)
  outs = [None] * n if outs is None else list(outs)
  if len(outs) != n:
    raise _bad(f'expected {n} outputs, got {len(outs)}')
  cols = (_lib.HashColumn * n)() if cols is None else cols
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
  _lib.check(_lib.lib().hbk_hash_insert_n(n, cols, 1 if insert else 0, _lib.current_stream(dev)))
  return outs


def hash_translate(tables, ids_list, insert=True, outs=None):
  """ids -> row numbers for N columns in ONE launch (``hbk_hash_insert_n``).  ``insert=False``: a pure find
  (-1 for ids never seen).  ``outs``: preallocated int64 ``[n_ids]`` tensors.  Returns the list of slots."""
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
    self._cols = (_lib.HashColumn * len(self.tables))()
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
    self.slots = _translate(self.tables, ids, self.train, keep, cols=self._cols)
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
    _lib.check(_lib.lib().hbk_hash_insert_n(len(self.tables), self._cols, 1 if self.train else 0, s))
    self.lookup.launch(stream)
