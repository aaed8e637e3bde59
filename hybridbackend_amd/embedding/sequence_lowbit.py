"""Sequence lookups over low-bit tables: the padded ``[batch, max_len, dim]`` rows of :class:`SequenceLookup` read
from ``torch.bfloat16`` / ``torch.float16`` tables or from 8-bit tables (``torch.uint8`` ``[rows, pitch]``, embedding/
quant8.py), written as fp32, bf16 or fp16 by ONE launch that also leaves the id grid and the lengths
(``hbk_sequence_lookup_fwd_lowbit``, include/hbk.h).

  :class:`LowbitSequenceLookup`      the forward: bit for bit ``deq[row]`` per position -- ``deq = table.float()`` or
                                     ``dequantize_rows8(...)`` -- zeros where nothing is looked up, cast once to
                                     ``out_dtype``.  A lookup sums nothing, so there is nothing else to round.
  :class:`LowbitSequenceLookupGrad`  the backward and the step: the unmodified ``LowpLookupGrad`` /
                                     ``Quant8LookupGrad`` over the grid the forward left, as one id per position.
"""
import ctypes as C

import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding.lowp import LowpGroupLookup, LowpLookupGrad
from hybridbackend_amd.embedding.quant8 import Quant8GroupLookup, Quant8LookupGrad, _require_tables8
from hybridbackend_amd.embedding.sequence import SequenceLookupGrad, _alloc_side, _bind_ids, check_sequence_args

_ROW_FORMATS = {torch.bfloat16: _lib.LOWP_BF16, torch.float16: _lib.LOWP_FP16, torch.uint8: _lib.ROWS_INT8}
_OUT_DTYPES = {torch.float32: _lib.QUANT8_OUT_FP32, torch.bfloat16: _lib.LOWP_BF16, torch.float16: _lib.LOWP_FP16}


def _bad(msg):
  return _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, msg)


def check_dim(dim, what):
  """The dims the forward serves and both apply kernels step: 1..256, or 1..64 when ``dim % 4 != 0``."""
  if not 1 <= dim <= 256 or (dim % 4 != 0 and dim > 64):
    raise _bad(f'{what}: dim {dim} is beyond what the low-bit sequence forward and the step take (at most 256 when a '
               'multiple of 4, 64 otherwise)')


class LowbitSequenceLookup:
  """A group of N sequence columns over low-bit tables, one launch per 64 columns and kind.

  Args:
    tables: ALL ``torch.bfloat16`` / ``torch.float16`` ``[rows, dim]`` device tensors (a call may mix the two), or
      ALL ``torch.uint8`` ``[rows, pitch]`` 8-bit tables (``quantize_rows8``) with ``dims``.  fp32 tables, or a mix of
      16-bit and 8-bit ones, are refused by name: fp32 tables have :class:`SequenceLookup`.
    dims: the dims of 8-bit tables (they cannot be read off the tensors); None for 16-bit tables.
    buckets, max_lens, pad_ids, divisor: as :class:`SequenceLookup`.
    out_dtype: ``torch.float32``, ``torch.bfloat16`` or ``torch.float16``: the element type of every output.

  ``__call__``, ``grids`` and ``lengths`` are :class:`SequenceLookup`'s; outputs may be sample-strided blocks of a
  wider tensor.  ``lane_elems_used`` lists the elements a lane moves in every bound column (8, 4 or 1): a pure speed
  matter, no bit depends on it.  ``max_norms`` does not exist here."""

  def __init__(self, tables, dims=None, buckets=None, max_lens=None, pad_ids=None, divisor=1,
               out_dtype=torch.float32):
    what = 'LowbitSequenceLookup'
    if out_dtype not in _OUT_DTYPES:
      raise _bad(f'{what}: out_dtype must be torch.float32, torch.bfloat16 or torch.float16, got {out_dtype!r}')
    self.out_dtype = out_dtype
    tables = list(tables)
    kinds = set()
    for c, t in enumerate(tables):
      if not isinstance(t, torch.Tensor) or t.dtype not in _ROW_FORMATS or t.dim() != 2:
        raise _bad(f'{what}: table {c} must be a torch.bfloat16 / torch.float16 [rows, dim] or a torch.uint8 '
                   f'[rows, pitch] tensor, got {getattr(t, "dtype", type(t).__name__)} (fp32 tables go through '
                   'SequenceLookup)')
      kinds.add(t.dtype == torch.uint8)
    if len(kinds) > 1:
      raise _bad(f'{what}: the tables mix 16-bit and 8-bit rows; build one lookup per kind (fp32 tables go through '
                 'SequenceLookup)')
    self.int8 = kinds == {True}
    if self.int8:
      if dims is None:
        raise _bad(f'{what}: 8-bit tables need dims (a [rows, pitch] tensor does not name its dim)')
      self.tables, self.dims = _require_tables8(tables, dims, what)
    else:
      if dims is not None and [int(d) for d in dims] != [int(t.shape[1]) for t in tables]:
        raise _bad(f'{what}: dims {list(dims)} do not match the 16-bit tables\' {[int(t.shape[1]) for t in tables]}')
      for t in tables:
        _lib.require_device_tensor(t, 'embedding weights')
      self.tables, self.dims = tables, [int(t.shape[1]) for t in tables]
    n = len(self.tables)
    for c, d in enumerate(self.dims):
      check_dim(d, f'{what}: table {c}')
    self.buckets, self.max_lens, self.pad_ids = check_sequence_args(
      n, buckets, max_lens, pad_ids, rows=[int(t.shape[0]) for t in self.tables])
    self.divisor = int(divisor)
    self._lib = _lib.lib()
    self._cols = (_lib.SequenceLowbitColumn * n)()
    self._seqs = (_lib.Sequence * n)()
    for c, t in enumerate(self.tables):
      col = self._cols[c]
      col.table = t.data_ptr()
      col.pitch = t.shape[1] if self.int8 else 0
      col.rows = t.shape[0]
      col.dim = self.dims[c]
      col.row_format = _ROW_FORMATS[t.dtype]
      col.out_dtype = _OUT_DTYPES[out_dtype]
      col.bucket = self.buckets[c]
      col.divisor = self.divisor
    self._plain = None
    self._keep = None
    self.grids = None        # the last forward's grids (None after an inference call)
    self.lengths = None

  def __len__(self):
    return len(self.tables)

  def plain_lookup(self):
    """The lookup over a grid: the same tables as one-id-per-position columns without a bucketize (the grid is
    bucketized already).  What the backward differentiates."""
    if self._plain is None:
      if self.int8:
        self._plain = Quant8GroupLookup(self.tables, self.dims, buckets=None, combiners='sum', divisor=self.divisor)
      else:
        self._plain = LowpGroupLookup(self.tables, buckets=None, combiners='sum', divisor=self.divisor,
                                      wide_rows=True)
    return self._plain

  @property
  def lane_elems_used(self):
    """The elements per lane of every bound column (``hbk_sequence_lowbit_lane_elems``): 8, 4 or 1."""
    return [int(self._lib.hbk_sequence_lowbit_lane_elems(C.byref(self._cols[c]))) for c in range(len(self.tables))]

  def __call__(self, ids, row_splits=None, outs=None, grids=True):
    """ids[c]: int32/int64 values, row_splits[c]: int32 ``[B+1]`` or None (one id per sample).  Returns
    ``(outs, lengths)``: per column ``[B, T_c, dim_c]`` of ``out_dtype`` -- or the caller's ``outs[c]`` of that shape,
    whose samples may lie a uniform stride apart -- and int32 ``[B]`` ``min(len, T_c)``.  ``grids=True`` keeps the id
    grid of every column (``self.grids``) for :class:`LowbitSequenceLookupGrad`; ``grids=False`` is the inference
    form: no grid is allocated or written."""
    n = len(self.tables)
    batch, row_splits = _bind_ids(self._cols, self._seqs, ids, row_splits, self.max_lens, self.pad_ids)
    dev = self.tables[0].device if n else None
    outs = [None] * n if outs is None else list(outs)
    if len(outs) != n:
      raise _bad(f'expected {n} outputs, got {len(outs)}')
    for c in range(n):
      shape = (batch[c], self.max_lens[c], self.dims[c])
      if outs[c] is None:
        outs[c] = torch.empty(shape, dtype=self.out_dtype, device=dev)
      o = outs[c]
      if not isinstance(o, torch.Tensor) or not o.is_cuda or o.dtype != self.out_dtype or tuple(o.shape) != shape:
        raise _bad(f'output {c} must be a {self.out_dtype} (out_dtype) device tensor {list(shape)}')
      stride = 0
      if not o.is_contiguous():
        if (shape[2] > 1 and o.stride(2) != 1) or (shape[1] > 1 and o.stride(1) != shape[2]) or \
            o.stride(0) < shape[1] * shape[2]:
          raise _bad(f'output {c}: the rows of a sample must be contiguous and the samples a uniform stride of at '
                     f'least {shape[1] * shape[2]} elements apart')
        stride = int(o.stride(0))
      self._cols[c].out = o.data_ptr()
      self._cols[c].out_stride = stride
    lengths, gs = _alloc_side(batch, self.max_lens, dev, grids)
    for c in range(n):
      self._seqs[c].lengths = lengths[c].data_ptr()
      self._seqs[c].row_grid = gs[c].data_ptr() if gs is not None else None
    self._keep = (list(ids), row_splits, outs, lengths, gs)
    self.launch()
    self.grids = gs if grids else None
    self.lengths = lengths
    return outs, lengths

  def launch(self, stream=None):
    """The bound call again on its tensors (ids and row_splits refilled in place; captured graphs): one foreign call,
    no allocation."""
    if self._keep is None:
      raise _bad('LowbitSequenceLookup.launch: nothing is bound: call the lookup first')
    n = len(self.tables)
    if stream is None:
      s = _lib.current_stream(self.tables[0].device if n else None)
    else:
      s = C.c_void_p(stream.cuda_stream)
    _lib.check(self._lib.hbk_sequence_lookup_fwd_lowbit(n, self._cols, self._seqs, s))


class LowbitSequenceLookupGrad:
  """Backward and optimizer step of a :class:`LowbitSequenceLookup`: ``LowpLookupGrad`` (16-bit tables) or
  ``Quant8LookupGrad`` (8-bit tables), unmodified, over ``lookup.plain_lookup()``, handed the last forward's grids as
  one-id-per-position columns and the ``[B, T, dim]`` gradients viewed ``[B * T, dim]`` -- what
  :class:`SequenceLookupGrad` is to the fp32 object.  There is no backward kernel of its own: the reduce never reads
  the table, and both applies exist.  The slots (``accums`` / ``moments`` / ``adam`` / ``ftrl_slots`` / ``ftrl`` /
  ``row_accums`` / ``rowwise_adagrad``) are fp32 ``[rows, dim]``; ``deterministic``, ``rounding`` and ``seed`` are
  ``LowpLookupGrad``'s.  Truncated ids and zero padding are not in the grid: they reach no gradient row and no slot;
  with ``pad_ids`` the pad row collects the gradient of every padding position."""

  def __init__(self, lookup, accums=None, moments=None, adam=None, ftrl_slots=None, ftrl=None, row_accums=None,
               rowwise_adagrad=None, deterministic=False, rounding='nearest', seed=0):
    if not isinstance(lookup, LowbitSequenceLookup):
      raise _bad('LowbitSequenceLookupGrad needs a LowbitSequenceLookup (fp32 tables go through SequenceLookupGrad)')
    self.lookup = lookup
    cls = Quant8LookupGrad if lookup.int8 else LowpLookupGrad
    self.inner = cls(lookup.plain_lookup(), accums=accums, moments=moments, adam=adam, ftrl_slots=ftrl_slots,
                     ftrl=ftrl, row_accums=row_accums, rowwise_adagrad=rowwise_adagrad, deterministic=deterministic,
                     rounding=rounding, seed=seed)

  @property
  def step_counter(self):
    return self.inner.step_counter

  _rows_view = SequenceLookupGrad._rows_view   # pylint: disable=protected-access

  def __call__(self, grads, apply_lr=0.0, optimizer='sgd', emit=True, finish=True, grids=None):
    """grads[c]: the fp32 gradient of the last forward's ``outs[c]``.  Returns what ``LowpLookupGrad`` returns: per
    column ``(unique_rows, grad_rows, n_unique)`` (capacity ``B * T``; table rows, after ``// divisor``).  ``grids``:
    explicit grids (``sequence_row_grid``) for a backward without a forward."""
    grids = self.lookup.grids if grids is None else list(grids)
    if grids is None:
      raise _bad('LowbitSequenceLookupGrad: the last forward kept no grids (grids=False): pass grids= or look up '
                 'with grids=True')
    n = len(self.lookup)
    if len(grads) != n or len(grids) != n:
      raise _bad(f'expected {n} gradients and grids, got {len(grads)} and {len(grids)}')
    rows = [self._rows_view(c, grads[c], int(grids[c].numel())) for c in range(n)]
    return self.inner(grids, rows, None, apply_lr=apply_lr, optimizer=optimizer, emit=emit, finish=finish)
