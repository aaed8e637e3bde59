"""16-bit outputs: the group lookup's forward writing ``torch.bfloat16`` / ``torch.float16`` rows over fp32, bf16 or
fp16 tables (include/hbk.h, "16-bit outputs").

  :class:`Out16GroupLookup`  the forward (``hbk_group_lookup_fwd_out16``): the fp32 sums of ``GroupLookup`` (fp32
                             tables) or ``LowpGroupLookup`` (16-bit tables), rounded once per element to nearest even
                             where they are stored -- bit for bit the fp32-output lookup followed by
                             ``.to(out_dtype)``, without that second launch and without the fp32 block.
"""
import ctypes as C

import numpy as np
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding.lookup import GroupLookup, _combiner_code

_OUT_DTYPES = {torch.bfloat16: _lib.LOWP_BF16, torch.float16: _lib.LOWP_FP16}
_TABLE_DTYPES = {torch.float32: _lib.OUT16_TABLE_FP32, torch.bfloat16: _lib.LOWP_BF16, torch.float16: _lib.LOWP_FP16}


def _bad(msg):
  return _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, msg)


def check_out_dtype(out_dtype, what):
  if out_dtype not in _OUT_DTYPES:
    raise _bad(f'{what}: out_dtype must be torch.bfloat16 or torch.float16, got {out_dtype!r}')
  return out_dtype


class Out16GroupLookup(GroupLookup):
  """A group of N embedding columns looked up into 16-bit outputs, one launch per 64 columns, kind and lane width.

  Args:
    tables: list of ``torch.float32`` / ``torch.bfloat16`` / ``torch.float16`` ``[rows, dim]`` device tensors (a list
      may mix them).
    buckets, combiners, divisor: as :class:`GroupLookup`.
    out_dtype: ``torch.bfloat16`` or ``torch.float16``: the element type of every output.
    chunk_elems: None (the default lane width: 8 from dim 64 on, else 4), 4 or 8: elements a lane moves where the
      column allows it (8: ``dim % 8 == 0``, table and output rows 16-byte aligned).  A pure speed choice: the result
      does not depend on it.

  The calling convention is :class:`GroupLookup`'s -- ``bind``, ``__call__(ids, row_splits=None, outs=None,
  sp_weights=None)``, ``launch()``, ``bind_block``, outputs as column blocks of a wider tensor -- with outputs of
  ``out_dtype`` (an ``outs`` tensor of another dtype is refused), and the result is, bit for bit, the fp32-output
  lookup over ``[t.float() for t in tables]`` with the same arguments followed by ``.to(out_dtype)``.  ``max_norms``
  and ``hot_rows`` do not exist here and are refused; the attributes a ``GroupLookupGrad`` / ``LowpLookupGrad`` reads
  of its lookup say "none", so either is built on this object as on its own lookup (the gradient they take is fp32)."""

  def __init__(self, tables, buckets=None, combiners='sum', divisor=1, out_dtype=torch.bfloat16,   # pylint: disable=super-init-not-called
               chunk_elems=None, max_norms=None, hot_rows=False):
    what = 'Out16GroupLookup'
    if max_norms is not None and not (isinstance(max_norms, (list, tuple)) and all(x is None for x in max_norms)):
      raise _bad(f'{what}: max_norms is not supported with 16-bit outputs (the clip is part of the fp32-output forward)')
    if hot_rows is not False and hot_rows is not None and not (
        isinstance(hot_rows, (list, tuple)) and not any(hot_rows)):
      raise _bad(f'{what}: hot_rows is not supported with 16-bit outputs (this forward stages nothing)')
    if chunk_elems not in (None, 4, 8):
      raise _bad(f'{what}: chunk_elems must be None, 4 or 8, got {chunk_elems!r}')
    self.out_dtype = check_out_dtype(out_dtype, what)
    self.tables = list(tables)
    for c, t in enumerate(self.tables):
      if not isinstance(t, torch.Tensor) or t.dtype not in _TABLE_DTYPES or t.dim() != 2:
        raise _bad(f'{what}: table {c} must be a torch.float32, torch.bfloat16 or torch.float16 [rows, dim] tensor, '
                   f'got {getattr(t, "dtype", type(t).__name__)}')
      _lib.require_device_tensor(t, 'embedding weights')
    self._lib = _lib.lib()
    n = len(self.tables)
    if buckets is None:
      buckets = [0] * n
    if isinstance(combiners, (str, int)) or combiners is None:
      combiners = [combiners] * n
    self.buckets = [int(b or 0) for b in buckets]
    self.combiners = [_combiner_code(c) for c in combiners]
    self.divisor = int(divisor)
    # what GroupLookupGrad reads of its lookup: no clip, no hot-row bookkeeping
    self.max_norms = [0.0] * n
    self.max_norms_c = None
    self._auto_hot = []
    self._auto_state = None
    self._cols = (_lib.Out16LookupColumn * n)()
    self._cols_np = np.frombuffer(self._cols, dtype=np.dtype(_lib.Out16LookupColumn)) if n else None
    self._dims = [int(t.shape[1]) for t in self.tables]
    for c, t in enumerate(self.tables):
      col = self._cols[c]
      col.table = t.data_ptr()
      col.table_dtype = _TABLE_DTYPES[t.dtype]
      col.rows = t.shape[0]
      col.dim = t.shape[1]
      col.bucket = self.buckets[c]
      col.divisor = self.divisor
      col.combiner = self.combiners[c]
      col.out_dtype = _OUT_DTYPES[self.out_dtype]
      col.chunk_elems = chunk_elems or 0

  def _check_out(self, c, o, n_seg):
    if not isinstance(o, torch.Tensor) or o.dtype != self.out_dtype:
      raise _bad(f'Out16GroupLookup: output {c} must be a {self.out_dtype} tensor (out_dtype), got '
                 f'{getattr(o, "dtype", type(o).__name__)}')
    _lib.require_device_tensor(o, 'output', row_strided=True)
    if tuple(o.shape) != (n_seg, self._dims[c]):
      raise _bad(f'output {c} must be {self.out_dtype} [{n_seg}, {self._dims[c]}]')

  def bind(self, ids, row_splits=None, outs=None, lazy=False, sp_weights=None):   # pylint: disable=unused-argument
    """Point the column descriptors at this step's inputs/outputs; returns outs, the list of the per-column
    ``[segments, dim]`` tensors of ``out_dtype`` (allocated here when ``outs`` is None: one allocation, every column's
    block on a 16-byte boundary)."""
    self._call_key = None
    n = len(self.tables)
    if len(ids) != n:
      raise _bad(f'expected {n} id tensors, got {len(ids)}')
    row_splits = [None] * n if row_splits is None else list(row_splits)
    given = outs is not None
    outs = list(outs) if given else [None] * n
    if len(row_splits) != n or len(outs) != n:
      raise _bad(f'expected {n} row_splits and outputs, got {len(row_splits)} and {len(outs)}')
    for c in range(n):   # (the dtype first: an fp32 output is refused by name wherever it lives)
      if outs[c] is not None and (not isinstance(outs[c], torch.Tensor) or outs[c].dtype != self.out_dtype):
        self._check_out(c, outs[c], 0)
    n_seg = []
    for c in range(n):
      i, s = ids[c], row_splits[c]
      _lib.require_device_tensor(i, 'ids')
      if i.dtype not in (torch.int32, torch.int64) or i.dim() != 1:
        raise _bad('ids must be an int32/int64 vector')
      if s is not None:
        _lib.require_device_tensor(s, 'row_splits')
        if s.dtype != torch.int32 or s.dim() != 1 or s.numel() < 1:
          raise _bad('row_splits must be an int32 vector [segments+1]')
      n_seg.append(i.numel() if s is None else s.numel() - 1)
    self._bind_weights(ids, sp_weights)
    if not given and n:
      pad = [(n_seg[c] * self._dims[c] + 7) // 8 * 8 for c in range(n)]
      flat = torch.empty(sum(pad) + 8, dtype=self.out_dtype, device=self.tables[0].device)
      outs = [p[:r * d].view(r, d) for p, r, d in zip(torch.split(flat[:sum(pad)], pad), n_seg, self._dims)]
    for c in range(n):
      i, s, o = ids[c], row_splits[c], outs[c]
      self._check_out(c, o, n_seg[c])
      col = self._cols[c]
      col.ids_dtype = _lib.INT64 if i.dtype == torch.int64 else _lib.INT32
      col.ids = i.data_ptr()
      col.n_ids = i.numel()
      col.row_splits = s.data_ptr() if s is not None else None
      col.n_segments = n_seg[c]
      col.out = o.data_ptr()
      col.out_stride = 0 if o.is_contiguous() else int(o.stride(0))
    self._keep = (list(ids), row_splits, outs)
    return outs

  def bind_block(self, ids, row_splits, block, offsets, sp_weights=None):
    """bind() with every column's output a column block of ONE ``[segments, pitch]`` tensor of ``out_dtype``
    (``block``; column c starts at element ``offsets[c]`` of every row): what DenseFeatures writes.  Returns False
    when the inputs need bind()'s detailed checks (the caller then makes views and calls bind)."""
    n = len(self.tables)
    if (n == 0 or len(ids) != n or len(offsets) != n or not isinstance(block, torch.Tensor) or
        block.dtype != self.out_dtype or not block.is_cuda or block.dim() != 2 or block.stride(1) != 1 or
        any(offsets[c] < 0 or offsets[c] + self._dims[c] > block.shape[1] for c in range(n))):
      return False
    views = [block[:, o:o + d] for o, d in zip(offsets, self._dims)]
    self.bind(ids, row_splits, views, sp_weights=sp_weights)
    return True

  def launch(self, stream=None):
    """Enqueue the bound lookup on `stream` (a torch stream; default: current)."""
    if stream is None:
      s = _lib.current_stream(self.tables[0].device if self.tables else None)
    else:
      s = C.c_void_p(stream.cuda_stream)
    _lib.check(self._lib.hbk_group_lookup_fwd_out16(len(self.tables), self._cols, s))
