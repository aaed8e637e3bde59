"""8-bit embedding tables: rows of int8 codes with one fp32 scale per row, every sum and every optimizer slot fp32
(include/hbk.h, "8-bit tables").

A table is a ``torch.uint8`` ``[rows, pitch]`` device tensor: bytes ``0 .. dim-1`` of a row are codes in offset
binary (``q = code - 128``), the fp32 row scale sits at byte ``round_up(dim, 4)``, an element is ``q * scale``.
``dim`` cannot be read off such a tensor, so every class below takes ``dims``.

  :func:`quantize_rows8` / :func:`dequantize_rows8`   fp32 / bf16 / fp16 ``[rows, dim]`` -> table and back.
  :class:`Quant8GroupLookup`   the forward (``hbk_quant8_lookup_fwd``): bit for bit ``GroupLookup`` over the
                               dequantised tables, into fp32, bf16 or fp16 outputs.
  :class:`Quant8SparseApply`   the optimizer step on IndexedSlices (``hbk_quant8_apply_slices_n``): dequantise a
                               row, step it with the arithmetic of ``SparseApply``, requantise it -- to nearest, or
                               stochastically, without which a step below half a code is rounded away every time.
  :class:`Quant8LookupGrad`    the backward and the step: an unmodified ``GroupLookupGrad`` in its emit form (which
                               never reads the table), then ``Quant8SparseApply`` on the slices it returned.
"""
import ctypes as C

import numpy as np
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding.lookup import GroupLookup, GroupLookupGrad, _combiner_code
from hybridbackend_amd.embedding.lowp import LowpLookupGrad, check_rounding
from hybridbackend_amd.embedding.sparse_apply import SparseApply

_SRC_DTYPES = {torch.float32: _lib.QUANT8_OUT_FP32, torch.bfloat16: _lib.LOWP_BF16, torch.float16: _lib.LOWP_FP16}
_OUT_DTYPES = _SRC_DTYPES
MAX_DIM = 256


def _bad(msg):
  return _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, msg)


class Quant8Rows:
  """The row format's arithmetic."""

  @staticmethod
  def dim4(dim):
    return (int(dim) + 3) // 4 * 4

  @staticmethod
  def pitch_for(dim, align=4):
    """The smallest pitch of a ``dim``-wide row in bytes that is a multiple of ``align`` (4, 8 or 16): the codes
    rounded up to 4, then the scale, then padding.  ``align=4`` is the default pitch; 8 / 16 is what lets a lane of 8 /
    16 codes read its codes in one load (``Quant8GroupLookup(lane_codes=)``)."""
    if align not in (4, 8, 16):
      raise _bad(f'Quant8Rows.pitch_for: align must be 4, 8 or 16, got {align!r}')
    return (Quant8Rows.dim4(dim) + 4 + align - 1) // align * align


# 'auto': (ragged, 16-bit outputs, first dim, last dim) -> lane_codes.  Only what two runs of
# tools/bench_quant8_tables.py both showed faster than 4 codes per lane with the ranges apart
# (profiles/quant8_tables.txt; dims 16, 64 and 128 with one id per segment, 16 and 64 ragged); every other column keeps
# the narrow forward.
AUTO_LANE_CODES = (
  (False, True, 16, 128, 8),    # one id per segment, 16-bit outputs: 6 % faster at dim 16, 17 % at 64, 18 - 19 % at 128
  (False, False, 16, 16, 8),    # one id per segment, fp32 outputs: 3.5 % at dim 16; 11 - 16 % SLOWER at 64 and 128
  (True, True, 64, 64, 16),     # ragged, 16-bit outputs, dim 64: 27 % (8 codes: 9 %); dim 16: every width loses
  (True, False, 64, 64, 8),     # ragged, fp32 outputs, dim 64: 10 %
)


def auto_lane_codes(dim, out_dtype, ragged):
  """The width ``lane_codes='auto'`` gives a column: 8, 16, or 0 for the narrow forward."""
  o16 = out_dtype != torch.float32
  for r, o, lo, hi, w in AUTO_LANE_CODES:
    if r == bool(ragged) and o == o16 and lo <= dim <= hi and dim % w == 0:
      return w
  return 0


def _require_tables8(tables8, dims, what):
  """``tables8`` as a list of uint8 ``[rows, pitch]`` device tensors whose pitch holds a ``dims[c]``-wide row."""
  tables8, dims = list(tables8), [int(d) for d in dims]
  if len(dims) != len(tables8):
    raise _bad(f'{what}: {len(dims)} dims for {len(tables8)} tables')
  for c, (t, d) in enumerate(zip(tables8, dims)):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2:
      raise _bad(f'{what}: table {c} must be a torch.uint8 [rows, pitch] tensor, got '
                 f'{getattr(t, "dtype", type(t).__name__)} (fp32 and 16-bit tables have lookups of their own)')
    if not 1 <= d <= MAX_DIM:
      raise _bad(f'{what}: table {c}: dim must be in [1, {MAX_DIM}], got {d}')
    pitch = int(t.shape[1])
    if pitch % 4 != 0 or pitch < Quant8Rows.pitch_for(d):
      raise _bad(f'{what}: table {c}: pitch {pitch} must be a multiple of 4 and >= {Quant8Rows.pitch_for(d)} for '
                 f'dim {d}')
    _lib.require_device_tensor(t, 'embedding weights')
    if t.data_ptr() % 4 != 0:
      raise _bad(f'{what}: table {c} must be 4-byte aligned')
  return tables8, dims


def _rows_call(entry, tables8, dims, rows_f, rounding_c=None):
  n = len(tables8)
  cols = (_lib.Quant8RowsColumn * n)()
  for c in range(n):
    col = cols[c]
    col.table = tables8[c].data_ptr()
    col.rows_f = rows_f[c].data_ptr()
    col.rows = tables8[c].shape[0]
    col.dim = dims[c]
    col.pitch = tables8[c].shape[1]
    col.src_dtype = _SRC_DTYPES[rows_f[c].dtype]
  s = _lib.current_stream(tables8[0].device if n else None)
  lib = _lib.lib()
  if rounding_c is None:
    _lib.check(getattr(lib, entry)(n, cols, s))
  else:
    _lib.check(getattr(lib, entry)(n, cols, C.byref(rounding_c), s))


def quantize_rows8(tables, pitch=None, rounding='nearest', seed=0, step_counter=None):
  """fp32 / bf16 / fp16 ``[rows, dim]`` device tensors -> new uint8 ``[rows, pitch]`` tables, one launch per 64.

  pitch: None (``Quant8Rows.pitch_for(dim)``), one number for all tables or one per table (None: the default).
  rounding, seed: ``'nearest'`` or ``'stochastic'`` (include/hbk.h); the stochastic noise is keyed by ``seed``, the
  word in ``step_counter`` (a device int32 [1]; a zero when omitted; not advanced), the table's index and the row."""
  tables = list(tables)
  n = len(tables)
  mode, seed = check_rounding(rounding, seed, [], 'quantize_rows8')
  pitches = list(pitch) if isinstance(pitch, (list, tuple)) else [pitch] * n
  if len(pitches) != n:
    raise _bad(f'quantize_rows8: {len(pitches)} pitches for {n} tables')
  srcs, dims, out = [], [], []
  for c, t in enumerate(tables):
    if not isinstance(t, torch.Tensor) or t.dtype not in _SRC_DTYPES or t.dim() != 2:
      raise _bad(f'quantize_rows8: table {c} must be a torch.float32, torch.bfloat16 or torch.float16 [rows, dim] '
                 f'tensor, got {getattr(t, "dtype", type(t).__name__)}')
    _lib.require_device_tensor(t, 'embedding weights')
    d = int(t.shape[1])
    if not 1 <= d <= MAX_DIM:
      raise _bad(f'quantize_rows8: table {c}: dim must be in [1, {MAX_DIM}], got {d}')
    p = Quant8Rows.pitch_for(d) if pitches[c] is None else int(pitches[c])
    if p % 4 != 0 or p < Quant8Rows.pitch_for(d):
      raise _bad(f'quantize_rows8: table {c}: pitch {p} must be a multiple of 4 and >= {Quant8Rows.pitch_for(d)} for '
                 f'dim {d}')
    srcs.append(t.contiguous())
    dims.append(d)
    out.append(torch.empty((t.shape[0], p), dtype=torch.uint8, device=t.device))
  if not n:
    return out
  if mode == _lib.LOWP_ROUND_STOCHASTIC and step_counter is None:
    step_counter = torch.zeros(1, dtype=torch.int32, device=out[0].device)
  step = step_counter.data_ptr() if step_counter is not None else None
  _rows_call('hbk_quant8_rows_n', out, dims, srcs, _lib.LowpRounding(mode, seed, step, 0, 0))
  return out


def dequantize_rows8(tables8, dims):
  """uint8 ``[rows, pitch]`` tables -> new fp32 ``[rows, dim]`` tensors, one launch per 64."""
  tables8, dims = _require_tables8(tables8, dims, 'dequantize_rows8')
  out = [torch.empty((t.shape[0], d), dtype=torch.float32, device=t.device) for t, d in zip(tables8, dims)]
  if tables8:
    _rows_call('hbk_dequant8_rows_n', tables8, dims, out)
  return out


class Quant8GroupLookup(GroupLookup):
  """A group of N embedding columns over 8-bit tables, one launch per 64 columns, kind, lane width and output size.

  Args:
    tables8: list of ``torch.uint8`` ``[rows, pitch]`` device tensors (:func:`quantize_rows8`).
    dims: the tables' dims.
    buckets, combiners, divisor: as :class:`GroupLookup`.
    out_dtype: ``torch.float32``, ``torch.bfloat16`` or ``torch.float16``: the element type of every output.
    chunk_elems: None (the default lane width) or 4: codes a lane moves where the column allows it, in
      ``hbk_quant8_lookup_fwd``.  A pure speed choice: the result does not depend on it.
    lane_codes: None (``hbk_quant8_lookup_fwd``, unchanged), 8 or 16 (``hbk_quant8_lookup_fwd_wide``: lanes of that
      many codes wherever a column allows it -- ``dim % lane_codes == 0`` and the output block and its stride on a
      16-byte boundary -- and the narrow forward, in the same call, where not), or ``'auto'``: per column and bound
      kind, the width :data:`AUTO_LANE_CODES` names.  A pure speed choice too.  ``lane_codes_used`` lists the width
      every bound column gets.

  The calling convention is :class:`GroupLookup`'s -- ``bind``, ``__call__(ids, row_splits=None, outs=None,
  sp_weights=None)``, ``launch()``, ``bind_block``, outputs as column blocks of a wider tensor -- and the result is,
  bit for bit, ``GroupLookup`` over ``dequantize_rows8(tables8, dims)`` with the same arguments, followed by
  ``.to(out_dtype)``.  ``max_norms`` and ``hot_rows`` do not exist here and are refused; the attributes a
  ``GroupLookupGrad`` reads of its lookup say "none"."""

  def __init__(self, tables8, dims, buckets=None, combiners='sum', divisor=1, out_dtype=torch.float32,   # pylint: disable=super-init-not-called
               chunk_elems=None, max_norms=None, hot_rows=False, lane_codes=None):
    what = 'Quant8GroupLookup'
    if lane_codes not in (None, 8, 16, 'auto'):
      raise _bad(f"{what}: lane_codes must be None, 8, 16 or 'auto', got {lane_codes!r}")
    if lane_codes is not None and chunk_elems is not None:
      raise _bad(f'{what}: lane_codes={lane_codes!r} cannot be given together with chunk_elems={chunk_elems!r} '
                 '(chunk_elems is the narrow forward\'s width)')
    self.lane_codes = lane_codes
    if max_norms is not None and not (isinstance(max_norms, (list, tuple)) and all(x is None for x in max_norms)):
      raise _bad(f'{what}: max_norms is not supported for 8-bit tables (the clip reads and the clipped step writes '
                 'fp32 rows)')
    if hot_rows is not False and hot_rows is not None and not (
        isinstance(hot_rows, (list, tuple)) and not any(hot_rows)):
      raise _bad(f'{what}: hot_rows is not supported for 8-bit tables (this forward stages nothing)')
    if chunk_elems not in (None, 4):
      raise _bad(f'{what}: chunk_elems must be None or 4, got {chunk_elems!r}')
    if out_dtype not in _OUT_DTYPES:
      raise _bad(f'{what}: out_dtype must be torch.float32, torch.bfloat16 or torch.float16, got {out_dtype!r}')
    self.out_dtype = out_dtype
    self.tables, self._dims = _require_tables8(tables8, dims, what)
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
    self._cols = (_lib.Quant8LookupColumn * n)()
    self._cols_np = np.frombuffer(self._cols, dtype=np.dtype(_lib.Quant8LookupColumn)) if n else None
    for c, t in enumerate(self.tables):
      col = self._cols[c]
      col.table = t.data_ptr()
      col.pitch = t.shape[1]
      col.rows = t.shape[0]
      col.dim = self._dims[c]
      col.bucket = self.buckets[c]
      col.divisor = self.divisor
      col.combiner = self.combiners[c]
      col.out_dtype = _OUT_DTYPES[out_dtype]
      col.chunk_elems = chunk_elems or 0
    self._plan_calls()

  @property
  def dims(self):
    return list(self._dims)

  def _check_out(self, c, o, n_seg):
    if not isinstance(o, torch.Tensor) or o.dtype != self.out_dtype:
      raise _bad(f'Quant8GroupLookup: output {c} must be a {self.out_dtype} tensor (out_dtype), got '
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
      per16 = 16 // torch.empty((), dtype=self.out_dtype).element_size()
      pad = [(n_seg[c] * self._dims[c] + per16 - 1) // per16 * per16 for c in range(n)]
      flat = torch.empty(sum(pad) + per16, dtype=self.out_dtype, device=self.tables[0].device)
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
    self._plan_calls()
    return outs

  def _plan_calls(self):
    """The calls of a launch: [(lane_codes or 0, n, column array)].  One call over the bound array, except under
    ``'auto'`` when the rule gives the columns different widths: then one call, over a copy of its columns, per
    width."""
    n = len(self.tables)
    if self.lane_codes == 'auto':
      self._want = [auto_lane_codes(self._dims[c], self.out_dtype, bool(self._cols[c].row_splits)) for c in range(n)]
    else:
      self._want = [self.lane_codes or 0] * n
    self._calls = []
    for w in sorted(set(self._want)):
      idx = [c for c in range(n) if self._want[c] == w]
      cols = self._cols if len(idx) == n else (_lib.Quant8LookupColumn * len(idx))(*[self._cols[c] for c in idx])
      self._calls.append((w, len(idx), cols))

  @property
  def lane_codes_used(self):
    """The codes per lane of every bound column (``hbk_quant8_lookup_lane_codes``): 16, 8, 4 or 1."""
    return [int(self._lib.hbk_quant8_lookup_lane_codes(C.byref(self._cols[c]), w)) for c, w in enumerate(self._want)]

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
    for w, n, cols in self._calls:
      if w:
        _lib.check(self._lib.hbk_quant8_lookup_fwd_wide(n, cols, w, s))
      else:
        _lib.check(self._lib.hbk_quant8_lookup_fwd(n, cols, s))


class Quant8SparseApply(SparseApply):
  """The sparse optimizer step of N 8-bit tables from caller-held IndexedSlices, one launch per 64 tables.

  Args:
    tables8, dims: the ``torch.uint8`` ``[rows, pitch]`` tables, stepped in place, and their dims.
    accums / moments, adam / ftrl_slots, ftrl / row_accums, rowwise_adagrad: the optimizer slots and objects, as
      :class:`SparseApply` takes them.  Slots are FP32 ``[rows, dim]`` (row-wise Adagrad: ``[rows, 1]``).
    rounding: ``'nearest'`` (ties to even) or ``'stochastic'`` (``floor(t + u * 2^-16)``, unbiased, with noise that
      is a pure function of ``(seed, step counter, column, row, element)``; include/hbk.h).
    seed: the noise's seed, an integer in [0, 2^32).

  A stepped row is ``quantise(rule(dequantise(row), slots, g))`` with the formulas, rounding and operation order of
  :class:`SparseApply`; with ``'nearest'`` the slots equal ``SparseApply``'s on the dequantised table bit for bit and
  the table equals its result, quantised.  All five optimizers.  The object owns the device step counter
  (``step_counter``): a call with ``finish=True`` advances it once, behind the apply in stream order, so replays of a
  captured graph draw fresh noise; ``'nearest'`` never touches it.  ``__call__``, ``bind`` and ``launch`` are
  :class:`SparseApply`'s.  ``tables`` holds fp32 stand-ins of the rows' shape (one word each) for the slot checks;
  the 8-bit tensors are ``tables8``."""

  _NAME = 'Quant8SparseApply'
  _NEEDS = 'Quant8SparseApply(tables8, dims, {slots})'
  _COLUMN = _lib.Quant8SlicesColumn

  def __init__(self, tables8, dims, accums=None, moments=None, adam=None, ftrl_slots=None, ftrl=None, row_accums=None,
               rowwise_adagrad=None, rounding='nearest', seed=0):
    self.tables8, self.dims = _require_tables8(tables8, dims, self._NAME)
    self._mode, self.seed = check_rounding(rounding, seed, [], self._NAME)
    self.rounding = rounding
    super().__init__(self.tables8, accums=accums, moments=moments, adam=adam, ftrl_slots=ftrl_slots, ftrl=ftrl,
                     row_accums=row_accums, rowwise_adagrad=rowwise_adagrad)
    for c, t in enumerate(self.tables8):
      col = self._cols[c]
      col.table = t.data_ptr()
      col.pitch = t.shape[1]
    dev = self.tables8[0].device if self.tables8 else torch.device('cuda', torch.cuda.current_device())
    self.step_counter = torch.zeros(1, dtype=torch.int32, device=dev)
    # the hbk_lowp_rounding_t of a call with / without the advance (kept alive by this object)
    self._rounding_c = {f: _lib.LowpRounding(self._mode, self.seed, self.step_counter.data_ptr(), 1 if f else 0, 0)
                        for f in (False, True)}

  def _require_tables(self, tables):
    # what the base class reads of a table is its shape and device: fp32 stand-ins of the rows' shape
    return [torch.empty((), dtype=torch.float32, device=t.device).expand(t.shape[0], d)
            for t, d in zip(tables, self.dims)]

  def _foreign_call(self, apply, s0, s1, params, lr, finish, stream):
    return self._lib.hbk_quant8_apply_slices_n(len(self.tables), self._cols, apply, s0, s1, params, lr,
                                               C.byref(self._rounding_c[finish]), stream)


class Quant8LookupGrad(LowpLookupGrad):
  """Backward and optimizer step of a :class:`Quant8GroupLookup`, with :class:`LowpLookupGrad`'s calling convention:
  an UNMODIFIED ``GroupLookupGrad`` over the lookup, always asked to emit (the reduce never reads the table), then a
  :class:`Quant8SparseApply` on the slices it returned.  Never give a bare ``GroupLookupGrad`` a lookup over 8-bit
  tables and a non-zero ``apply_lr``: its fused step reads and writes fp32 rows.

  Args: ``lookup``, then the slots, ``deterministic``, ``rounding`` and ``seed`` of :class:`LowpLookupGrad`."""

  def __init__(self, lookup, accums=None, moments=None, adam=None, ftrl_slots=None, ftrl=None, row_accums=None,   # pylint: disable=super-init-not-called
               rowwise_adagrad=None, deterministic=False, rounding='nearest', seed=0):
    if not isinstance(lookup, Quant8GroupLookup):
      raise _bad('Quant8LookupGrad needs a Quant8GroupLookup (fp32 tables go through GroupLookupGrad, 16-bit tables '
                 'through LowpLookupGrad)')
    self.lookup = lookup
    self._apply = Quant8SparseApply(lookup.tables, lookup.dims, accums=accums, moments=moments, adam=adam,
                                    ftrl_slots=ftrl_slots, ftrl=ftrl, row_accums=row_accums,
                                    rowwise_adagrad=rowwise_adagrad, rounding=rounding, seed=seed)
    # no slots, no accumulators: this object can only emit.  The reduce reads a lookup's tables for their shapes:
    # it is given the rows' fp32 stand-ins
    self._reduce = GroupLookupGrad(_ReduceView(lookup, self._apply.tables), deterministic=deterministic)
    self._last_emit = True

  @staticmethod
  def _refuse_weight_grads(weight_grads):
    if weight_grads is not False and weight_grads is not None:
      raise _bad('Quant8LookupGrad: weight_grads is not supported for 8-bit tables (hbk_group_lookup_bwd_weights '
                 'reads fp32 rows)')


class _ReduceView:
  """A Quant8GroupLookup as the emit-form reduce reads its lookup: every attribute the lookup's own, ``tables`` the
  fp32 stand-ins of the rows' shape (the reduce takes dims from them and never touches their memory)."""

  def __init__(self, lookup, like):
    self._lookup = lookup
    self.tables = like

  def __getattr__(self, name):
    return getattr(self._lookup, name)

  def __len__(self):
    return len(self.tables)
