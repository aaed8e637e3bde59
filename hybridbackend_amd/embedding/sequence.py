"""SequenceLookup: ragged id lists looked up WITHOUT a combiner -- the padded ``[batch, max_len, dim]``
rows an attention layer reads (DIN / DIEN / BST).  Host side of ``hbk_group_lookup_fwd_sequence`` and
``hbk_sequence_row_grid_n`` (include/hbk.h), which replace, for N columns at once, what the reference's
Taobao DIN tutorial builds per history field out of stock TF ops
(docs/tutorial/ranking/data.py:195-224, ``transform_categorical_non_pooling``):

  ``tf.sparse.slice(x, [0, 0], [batch, max_varlength])`` -> ``tf.sparse.to_dense(default_value=)``
  -> ``% embedding_size`` -> ``tf.nn.embedding_lookup``

and TF's ``sequence_categorical_column_*`` + ``embedding_column`` + ``SequenceFeatures`` (zero rows past
a sample's length and a ``sequence_length`` vector): that is the form without ``pad_ids``.

The forward leaves the bucketized id grid (``-1`` where nothing was looked up) on the device; the
backward hands it to :class:`GroupLookupGrad` as a column of one id per position, so every reduce plan,
the deterministic modes, the clip and every optimizer apply unchanged, and truncated ids or zero padding
reach no gradient row and no optimizer slot.
"""
import ctypes as C
import numbers

import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import optimizer as _opt
from hybridbackend_amd.embedding.lookup import GroupLookup
from hybridbackend_amd.embedding.lookup import GroupLookupGrad
from hybridbackend_amd.embedding.lookup import max_norm_list


def _bad(msg):
  return _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, msg)


def per_column(values, n, what, none_ok=False):
  """``values`` (one for all columns, or one per column) as a list of n ints (None kept when allowed)."""
  if values is None or isinstance(values, numbers.Integral):
    values = [values] * n
  try:
    values = list(values)
  except TypeError:
    raise _bad(f'{what} must be one integer or one per column, got {values!r}') from None
  if len(values) != n:
    raise _bad(f'expected {n} {what}, got {len(values)}')
  out = []
  for c, v in enumerate(values):
    if v is None and none_ok:
      out.append(None)
      continue
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
      raise _bad(f'{what} of column {c} must be an integer' + (' or None' if none_ok else '') + f', got {v!r}')
    out.append(int(v))
  return out


def check_sequence_args(n, buckets, max_lens, pad_ids, rows=None):
  """The per-column ``(buckets, max_lens, pad_ids)`` lists of a sequence lookup: ``max_len >= 1``; a
  ``pad_id`` must be a row the column can name -- ``0 <= pad_id < bucket`` with a bucket, else
  ``0 <= pad_id < rows`` (``rows`` None: not known, only the sign is checked)."""
  buckets = [0] * n if buckets is None else [int(b or 0) for b in buckets]
  if len(buckets) != n:
    raise _bad(f'expected {n} buckets, got {len(buckets)}')
  if max_lens is None:
    raise _bad('max_lens is required: the padded length of every column')
  max_lens = per_column(max_lens, n, 'max_lens')
  pad_ids = per_column(pad_ids, n, 'pad_ids', none_ok=True)
  for c in range(n):
    if max_lens[c] < 1:
      raise _bad(f'max_len of column {c} must be >= 1, got {max_lens[c]}')
    if buckets[c] < 0:
      raise _bad(f'bucket of column {c} must be >= 0, got {buckets[c]}')
    p = pad_ids[c]
    if p is None:
      continue
    limit = buckets[c] if buckets[c] > 0 else (None if rows is None else rows[c])
    if p < 0 or (limit is not None and p >= limit):
      raise _bad(f'pad_id of column {c} must be in [0, {limit if limit is not None else "rows"}), got {p}')
  return buckets, max_lens, pad_ids


def _bind_ids(cols, seqs, ids, row_splits, max_lens, pad_ids):
  """The id side of the descriptors; returns the samples per column."""
  n = len(max_lens)
  if len(ids) != n:
    raise _bad(f'expected {n} id tensors, got {len(ids)}')
  if row_splits is None:
    row_splits = [None] * n
  if len(row_splits) != n:
    raise _bad(f'expected {n} row_splits, got {len(row_splits)}')
  batch = []
  for c in range(n):
    i, s = ids[c], row_splits[c]
    _lib.require_device_tensor(i, 'ids')
    if i.dtype not in (torch.int32, torch.int64) or i.dim() != 1:
      raise _bad('ids must be an int32/int64 vector')
    if s is not None:
      _lib.require_device_tensor(s, 'row_splits')
      if s.dtype != torch.int32 or s.dim() != 1 or s.numel() < 1:
        raise _bad('row_splits must be an int32 vector [samples+1]')
    b = i.numel() if s is None else s.numel() - 1
    if b * max_lens[c] >= 2 ** 31:
      raise _bad(f'column {c}: {b} samples x max_len {max_lens[c]} positions, must stay below 2^31')
    col, q = cols[c], seqs[c]
    col.ids_dtype = _lib.INT64 if i.dtype == torch.int64 else _lib.INT32
    col.ids = i.data_ptr()
    col.n_ids = i.numel()
    col.row_splits = s.data_ptr() if s is not None else None
    col.n_segments = b
    q.max_len = max_lens[c]
    q.has_pad = 0 if pad_ids[c] is None else 1
    q.pad_id = pad_ids[c] or 0
    batch.append(b)
  return batch, list(row_splits)


def _alloc_side(batch, max_lens, device, grids):
  """lengths (one allocation, a view per column) and, when wanted, the grids."""
  flat = torch.empty(sum(batch), dtype=torch.int32, device=device)
  lengths = list(torch.split(flat, batch)) if batch else []
  gs = None
  if grids:
    gs = [torch.empty(b * t, dtype=torch.int64, device=device) for b, t in zip(batch, max_lens)]
  return lengths, gs


class SequenceLookup:
  """A group of N sequence columns looked up with one launch per kind of column.

  Args:
    tables: list of fp32 ``[rows, dim]`` device tensors.
    buckets: per-column ``embedding_size`` for the fused bucketize, or None/0.
    max_lens: the padded length T of every column (one value for all, or one per column): a sample's
      first T ids are looked up, later ones are never read.
    pad_ids: None -- positions past a sample's length are ZERO rows and take part in nothing (TF's
      ``SequenceFeatures``) -- or the id such positions look up (``to_dense(default_value=)`` followed by
      the lookup: the gradient that arrives there flows into that row); one for all columns or one per
      column.  ``0 <= pad_id < bucket`` with a bucket, else ``0 <= pad_id < rows``.
    divisor: ``row = id // divisor`` after the bucketize (a table sharded by modulo); 1 for a whole table.
    max_norms: TF's ``max_norm``: every looked-up row, pad rows included, is clipped as in
      :class:`GroupLookup`.
    fused: True -- one launch gathers the rows and writes grid and lengths
      (``hbk_group_lookup_fwd_sequence``); False -- ``hbk_sequence_row_grid_n`` followed by the plain
      gather over the grid (the same bits; outputs with a sample stride of their own still take the fused
      entry).  The default is the form that measured faster (profiles/sequence_lookup.txt).
  """

  def __init__(self, tables, buckets=None, max_lens=None, pad_ids=None, divisor=1, max_norms=None,
               fused=True):
    self._lib = _lib.lib()
    self.tables = list(tables)
    n = len(self.tables)
    for t in self.tables:
      _lib.require_device_tensor(t, 'embedding weights')
      if t.dtype != torch.float32 or t.dim() != 2:
        raise _bad('embedding weights must be fp32 [rows, dim]')
    self.buckets, self.max_lens, self.pad_ids = check_sequence_args(
      n, buckets, max_lens, pad_ids, rows=[int(t.shape[0]) for t in self.tables])
    self.divisor = int(divisor)
    self.max_norms = max_norm_list(max_norms, n)
    self.max_norms_c = (C.c_float * n)(*self.max_norms) if any(self.max_norms) else None
    self.fused = bool(fused)
    self.dims = [int(t.shape[1]) for t in self.tables]
    self._cols = (_lib.LookupColumn * n)()
    self._seqs = (_lib.Sequence * n)()
    for c, t in enumerate(self.tables):
      col = self._cols[c]
      col.table = t.data_ptr()
      col.rows = t.shape[0]
      col.dim = t.shape[1]
      col.bucket = self.buckets[c]
      col.divisor = self.divisor
    self._plain = None       # the two-launch form's gather over the grid
    self.grids = None        # the last forward's grids (None after an inference call)
    self.lengths = None

  def __len__(self):
    return len(self.tables)

  def plain_lookup(self):
    """The lookup over a grid: the same tables as one-id-per-position columns without a bucketize (the
    grid is bucketized already).  What the two-launch form gathers with and the backward differentiates."""
    if self._plain is None:
      self._plain = GroupLookup(self.tables, buckets=None, combiners='sum', divisor=self.divisor,
                                max_norms=[m or None for m in self.max_norms])
    return self._plain

  def __call__(self, ids, row_splits=None, outs=None, grids=True):
    """ids[c]: int32/int64 values, row_splits[c]: int32 ``[B+1]`` or None (one id per sample).  Returns
    ``(outs, lengths)``: per column fp32 ``[B, T_c, dim_c]`` -- or the caller's ``outs[c]`` of that shape,
    whose samples may lie a uniform stride apart (a block of a wider tensor) -- and int32 ``[B]``
    ``min(len, T_c)``.  ``grids=True`` keeps the id grid of every column (``self.grids``) for
    :class:`SequenceLookupGrad`; ``grids=False`` is the inference form: no grid is allocated or written."""
    n = len(self.tables)
    batch, row_splits = _bind_ids(self._cols, self._seqs, ids, row_splits, self.max_lens, self.pad_ids)
    dev = self.tables[0].device if n else None
    outs = [None] * n if outs is None else list(outs)
    if len(outs) != n:
      raise _bad(f'expected {n} outputs, got {len(outs)}')
    contiguous = True
    for c in range(n):
      shape = (batch[c], self.max_lens[c], self.dims[c])
      if outs[c] is None:
        outs[c] = torch.empty(shape, dtype=torch.float32, device=dev)
      o = outs[c]
      if not o.is_cuda or o.dtype != torch.float32 or tuple(o.shape) != shape:
        raise _bad(f'output {c} must be an fp32 device tensor {list(shape)}')
      stride = 0
      if not o.is_contiguous():
        if (shape[2] > 1 and o.stride(2) != 1) or (shape[1] > 1 and o.stride(1) != shape[2]) or \
            o.stride(0) < shape[1] * shape[2]:
          raise _bad(f'output {c}: the rows of a sample must be contiguous and the samples a uniform '
                     f'stride of at least {shape[1] * shape[2]} floats apart')
        stride = int(o.stride(0))
        contiguous = False
      self._cols[c].out = o.data_ptr()
      self._cols[c].out_stride = stride
    fused = self.fused or not contiguous
    lengths, gs = _alloc_side(batch, self.max_lens, dev, grids or not fused)
    for c in range(n):
      self._seqs[c].lengths = lengths[c].data_ptr()
      self._seqs[c].row_grid = gs[c].data_ptr() if gs is not None else None
    stream = _lib.current_stream(dev)
    if fused:
      _lib.check(self._lib.hbk_group_lookup_fwd_sequence(n, self._cols, self._seqs, self.max_norms_c, stream))
    else:
      _lib.check(self._lib.hbk_sequence_row_grid_n(n, self._cols, self._seqs, stream))
      self.plain_lookup()(gs, None, [o.view(g.numel(), d) for o, g, d in zip(outs, gs, self.dims)])
    self._keep = (list(ids), row_splits, outs)
    self.grids = gs if grids else None
    self.lengths = lengths
    return outs, lengths


class SequenceLookupGrad:
  """Backward of :class:`SequenceLookup`: a :class:`GroupLookupGrad` over the same tables, handed the
  last forward's grids as one-id-per-position columns and the ``[B, T, dim]`` gradients viewed
  ``[B * T, dim]`` in place.  ``accums`` / ``moments`` / ``adam`` / ``ftrl_slots`` / ``ftrl`` /
  ``row_accums`` / ``rowwise_adagrad`` are GroupLookupGrad's.  Truncated ids and zero padding are not in
  the grid: they reach no gradient row and no optimizer slot; with ``pad_ids`` the pad row collects the gradient of every padding position."""

  def __init__(self, lookup, accums=None, moments=None, adam=None, ftrl_slots=None, ftrl=None, row_accums=None,
               rowwise_adagrad=None):
    self.lookup = lookup
    self.inner = lookup.plain_lookup()
    # ONE optimizer object behind both drivers (the beta powers advance once per step)
    _opt.bind_all(self, dict(moments=moments, adam=adam, ftrl_slots=ftrl_slots, ftrl=ftrl, row_accums=row_accums,
                             rowwise_adagrad=rowwise_adagrad), lookup.tables, 'SequenceLookupGrad')
    self.accums = list(accums) if accums is not None else None
    self._drivers = {}

  def driver(self, deterministic=False):
    """The GroupLookupGrad of one summation mode (made when first asked for; both share a workspace)."""
    d = self._drivers.get(bool(deterministic))
    if d is None:
      other = next(iter(self._drivers.values()), None)
      d = GroupLookupGrad(self.inner, accums=self.accums, workspace_of=other,
                          deterministic=bool(deterministic), **_opt.slot_kwargs(self))
      self._drivers[bool(deterministic)] = d
    return d

  def _rows_view(self, c, g, n_pos):
    """grads[c] ``[B, T, dim]`` (or ``[B * T, dim]``) as ``[B * T, dim]`` rows a uniform stride apart: in
    place when the strides allow it with rows on 4-float boundaries, else one contiguous copy."""
    dim = self.lookup.dims[c]
    if g.dtype != torch.float32 or not g.is_cuda:
      raise _bad(f'grad {c} must be an fp32 device tensor')
    if g.dim() == 2 and tuple(g.shape) == (n_pos, dim):
      return g if g.is_contiguous() or (g.stride(1) == 1 and g.stride(0) % 4 == 0 and g.stride(0) >= dim) \
          else g.contiguous()
    if g.dim() != 3 or g.shape[2] != dim or g.shape[0] * g.shape[1] != n_pos:
      raise _bad(f'grad {c} must be fp32 [B, T, {dim}] with B * T = {n_pos}')
    if g.is_contiguous():
      return g.view(n_pos, dim)
    B, T = int(g.shape[0]), int(g.shape[1])
    row = g.stride(1) if T > 1 else (g.stride(0) if B > 1 else dim)
    if (dim == 1 or g.stride(2) == 1) and row >= dim and row % 4 == 0 and \
        (B <= 1 or T <= 1 or g.stride(0) == T * row):
      return g.as_strided((n_pos, dim), (row, 1))
    return g.contiguous().view(n_pos, dim)

  def __call__(self, grads, apply_lr=0.0, optimizer='sgd', emit=True, deterministic=False, finish=True,
               grids=None):
    """grads[c]: the gradient of the last forward's ``outs[c]``.  Returns what GroupLookupGrad returns:
    per column ``(unique_rows, grad_rows, n_unique)`` (capacity ``B * T``; table rows, after
    ``// divisor``).  ``deterministic=True``: every row's terms are summed in position order (b-major),
    rows ascending.  ``grids``: explicit grids (``sequence_row_grid``) for a backward without a forward."""
    grids = self.lookup.grids if grids is None else list(grids)
    if grids is None:
      raise _bad('the last forward kept no grids (grids=False): pass grids= or look up with grids=True')
    n = len(self.lookup)
    if len(grads) != n or len(grids) != n:
      raise _bad(f'expected {n} gradients and grids, got {len(grads)} and {len(grids)}')
    rows = [self._rows_view(c, grads[c], int(grids[c].numel())) for c in range(n)]
    return self.driver(deterministic)(grids, rows, None, apply_lr=apply_lr, optimizer=optimizer, emit=emit,
                                      finish=finish)


def sequence_row_grid(ids, row_splits=None, buckets=None, max_lens=None, pad_ids=None):
  """The grid op alone (``hbk_sequence_row_grid_n``): per column the int64 ``[B * T]`` bucketized ids of
  the first ``T`` ids of every sample -- ``pad_id`` (bucketized) or ``-1`` past a sample's length, ``-1``
  for a negative id without a bucket -- and the int32 ``[B]`` lengths.  Returns ``(grids, lengths)``.
  What a sharded sequence column feeds ``ShardedGroupLookup`` as ``B * T`` ids of one sample each."""
  n = len(ids)
  buckets, max_lens, pad_ids = check_sequence_args(n, buckets, max_lens, pad_ids)
  cols = (_lib.LookupColumn * n)()
  seqs = (_lib.Sequence * n)()
  for c in range(n):
    cols[c].bucket = buckets[c]
    cols[c].divisor = 1
  batch, _ = _bind_ids(cols, seqs, ids, row_splits, max_lens, pad_ids)
  dev = ids[0].device if n else None
  lengths, grids = _alloc_side(batch, max_lens, dev, True)
  for c in range(n):
    seqs[c].lengths = lengths[c].data_ptr()
    seqs[c].row_grid = grids[c].data_ptr()
  _lib.check(_lib.lib().hbk_sequence_row_grid_n(n, cols, seqs, _lib.current_stream(dev)))
  return grids, lengths


def sequence_id_grid(ids, row_splits=None, max_lens=None, pad_ids=None):
  """The RAW-id grid (``hbk_sequence_id_grid_n``): per column the int64 ``[B * T]`` effective ids -- the first
  ``T`` ids of every sample as they are (sign-extended from int32, never bucketized, negative ids kept), then
  ``pad_id`` -- and the int32 ``[B]`` lengths.  Returns ``(grids, lengths)``.  ``pad_ids`` are RAW ids, any int64,
  and every column needs one: among raw ids no value means "nothing".  What a sharded hash-keyed sequence column
  feeds ``ShardedHashGroupLookup`` as ``B * T`` ids of one sample each; ids past ``T`` are never read."""
  n = len(ids)
  if max_lens is None:
    raise _bad('max_lens is required: the padded length of every column')
  max_lens = per_column(max_lens, n, 'max_lens')
  pad_ids = per_column(pad_ids, n, 'pad_ids', none_ok=True)
  for c in range(n):
    if not 1 <= max_lens[c] < 2 ** 31:
      raise _bad(f'max_len of column {c} must be in [1, 2^31), got {max_lens[c]}')
    if pad_ids[c] is None:
      raise _bad(f'pad_id of column {c} is required: every int64 is an id, so a raw-id grid has no value for a '
                 'position that holds nothing')
    if not -2 ** 63 <= pad_ids[c] < 2 ** 63:
      raise _bad(f'pad_id of column {c} must be an int64, got {pad_ids[c]}')
  cols = (_lib.LookupColumn * n)()
  seqs = (_lib.Sequence * n)()
  batch, _ = _bind_ids(cols, seqs, ids, row_splits, max_lens, pad_ids)
  for c in range(n):
    seqs[c].pad_id = pad_ids[c]
  dev = ids[0].device if n else None
  lengths, _ = _alloc_side(batch, max_lens, dev, False)
  # (the entry refuses a NULL grid whatever the batch: a column without samples gets a view of one word)
  bufs = [torch.empty(max(b * t, 1), dtype=torch.int64, device=dev) for b, t in zip(batch, max_lens)]
  grids = [x[:b * t] for x, b, t in zip(bufs, batch, max_lens)]
  for c in range(n):
    seqs[c].lengths = lengths[c].data_ptr()
    seqs[c].row_grid = bufs[c].data_ptr()
  _lib.check(_lib.lib().hbk_sequence_id_grid_n(n, cols, seqs, _lib.current_stream(dev)))
  return grids, lengths


def sequence_pack(ids, row_splits=None, max_lens=None):
  """The PACKED form of zero-padded sequence columns (``hbk_sequence_pack_n``): per column the first
  ``min(len, T)`` ids of every sample back to back -- raw: sign-extended from int32, never bucketized, negative
  ids kept -- and the row splits that make them a ragged column of ``B * T`` segments, one per position,
  holding one id or none.  Returns ``(packed_ids, pos_splits, lengths, sample_splits)``, each a list with one
  entry per column: int64 ``[total]``, int32 ``[B * T + 1]``, int32 ``[B]`` and int32 ``[B + 1]`` (the CSR of
  the packed ids by sample).  There is no pad id: padding is in no list.  What a sharded sequence column
  without a pad id feeds ``ShardedGroupLookup`` / ``ShardedHashGroupLookup`` with combiner ``'sum'`` (an empty
  segment is a zero row that reaches no gradient); ids past ``T`` are never read.

  One C call, then ONE device-to-host copy, of the N totals (this call waits for the device there), to narrow
  every ``packed_ids[c]`` to a view of its ``total`` elements.  The sharded step that follows waits on the host
  once per forward itself (for the sizes of its id exchange)."""
  n = len(ids)
  if max_lens is None:
    raise _bad('max_lens is required: the padded length of every column')
  max_lens = per_column(max_lens, n, 'max_lens')
  for c in range(n):
    if not 1 <= max_lens[c] < 2 ** 31:
      raise _bad(f'max_len of column {c} must be in [1, 2^31), got {max_lens[c]}')
  cols = (_lib.LookupColumn * n)()
  seqs = (_lib.Sequence * n)()
  packs = (_lib.SequencePack * n)()
  batch, _ = _bind_ids(cols, seqs, ids, row_splits, max_lens, [None] * n)
  if n == 0:
    return [], [], [], []
  dev = ids[0].device
  lengths, _ = _alloc_side(batch, max_lens, dev, False)
  caps = [min(int(ids[c].numel()), batch[c] * max_lens[c]) for c in range(n)]
  # (the entry refuses a NULL output whatever the batch: an empty column gets a view of one word)
  bufs = [torch.empty(max(k, 1), dtype=torch.int64, device=dev) for k in caps]
  pos = [torch.empty(b * t + 1, dtype=torch.int32, device=dev) for b, t in zip(batch, max_lens)]
  samp = [torch.empty(b + 1, dtype=torch.int32, device=dev) for b in batch]
  totals = torch.empty(n, dtype=torch.int32, device=dev)
  for c in range(n):
    seqs[c].lengths = lengths[c].data_ptr() if batch[c] else totals.data_ptr()   # (no sample: nothing is written)
    packs[c].packed = bufs[c].data_ptr()
    packs[c].packed_capacity = caps[c]
    packs[c].pos_splits = pos[c].data_ptr()
    packs[c].sample_splits = samp[c].data_ptr()
    packs[c].total = totals.data_ptr() + 4 * c
  lib = _lib.lib()
  need = int(lib.hbk_sequence_pack_workspace_bytes(n, cols))
  work = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
  _lib.check(lib.hbk_sequence_pack_n(n, cols, seqs, packs, work.data_ptr(), need, _lib.current_stream(dev)))
  host = totals.cpu().tolist()
  for c in range(n):
    if host[c] > caps[c]:
      raise _bad(f'column {c}: row_splits name {host[c]} ids within max_len, the column holds {caps[c]}: '
                 'the row splits are no CSR of the ids')
  packed = [bufs[c][:host[c]] for c in range(n)]
  return packed, pos, lengths, samp


class ShardedSequenceLookup:
  """Zero-padded sequence lookups on SHARDED tables: a thin wrapper that packs (:func:`sequence_pack`) and hands
  the packed ids and the position-level row splits to a sharded driver.

  Args:
    driver: a ``ShardedGroupLookup`` or ``ShardedHashGroupLookup`` built with combiner ``'sum'``: ``dedup``, the
      fp16 wire, ``max_norms``, ``hot_rows``, every optimizer and ``maybe_grow`` / ``maybe_evict`` stay the
      driver's own.
    max_lens: the padded length T of every column (one value for all, or one per column).

  Positions past a sample's length are zero rows that take part in nothing (TF's ``SequenceFeatures``): they are
  in no id list, so they cross no wire, are looked up on no rank and reach no gradient row or optimizer slot;
  ids past T are never read, inserted, counted or kept fresh.  One host read per forward (the totals) beside
  the driver's own.  ``sp_weights``, the p2p form (``p2p_bind``) and ``PipelinedLookup`` are not offered through
  this wrapper."""

  def __init__(self, driver, max_lens):
    from hybridbackend_amd.embedding.lookup import _combiner_code
    self.driver = driver
    n = len(driver.shards)
    combs = driver.combiners
    if isinstance(combs, (str, int)) or combs is None:
      combs = [combs] * n
    if any(_combiner_code(k) != _lib.COMBINER_SUM for k in combs):
      raise _bad("ShardedSequenceLookup: the driver must be built with combiner 'sum' (an empty segment is "
                 'then a zero row)')
    self.max_lens = per_column(max_lens, n, 'max_lens')
    for c, t in enumerate(self.max_lens):
      if t < 1:
        raise _bad(f'max_len of column {c} must be >= 1, got {t}')
    self.dims = list(driver.dims)
    self.lengths = None
    self.sample_splits = None

  def __len__(self):
    return len(self.max_lens)

  def __call__(self, ids, row_splits=None, outs=None):
    """ids[c]: int32/int64 values, row_splits[c]: int32 ``[B+1]`` or None (one id per sample).  Returns
    ``(outs, lengths)``: per column fp32 ``[B, T_c, dim_c]`` (the caller's contiguous ``outs[c]`` of that shape,
    written in place) and int32 ``[B]`` ``min(len, T_c)``.  A collective when the driver's world is."""
    n = len(self.max_lens)
    if getattr(self.driver, '_p2p_keep', None) is not None:
      raise _lib.HbkError(_lib.UNIMPLEMENTED, 'ShardedSequenceLookup: the p2p form takes one id per segment; '
                          'p2p_unbind first')
    packed, pos, lengths, samp = sequence_pack(ids, row_splits, self.max_lens)
    flat = None
    if outs is not None:
      if len(outs) != n:
        raise _bad(f'expected {n} outputs, got {len(outs)}')
      flat = []
      for c, o in enumerate(outs):
        shape = (lengths[c].numel(), self.max_lens[c], self.dims[c])
        if not o.is_cuda or o.dtype != torch.float32 or tuple(o.shape) != shape or not o.is_contiguous():
          raise _bad(f'output {c} must be a contiguous fp32 device tensor {list(shape)}')
        flat.append(o.view(shape[0] * shape[1], shape[2]))
    rows = self.driver(packed, pos, outs=flat)
    self.lengths, self.sample_splits = lengths, samp
    return [o.view(ln.numel(), t, d) for o, ln, t, d in zip(rows, lengths, self.max_lens, self.dims)], lengths

  def backward(self, grads, **kw):
    """grads[c]: the gradient of the last forward's ``outs[c]``, ``[B, T, dim]`` (or ``[B * T, dim]``).  The
    driver's ``backward`` with its keywords and its result: it differentiates the last forward and the row
    splits that forward kept, so padding positions send no gradient row."""
    flat = [g.contiguous().view(-1, d) for g, d in zip(grads, self.dims)]
    return self.driver.backward(flat, **kw)
