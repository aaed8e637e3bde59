"""SparseApply: the optimizer step on IndexedSlices the CALLER holds (``hbk_sparse_apply_slices_n``,
include/hbk.h) -- the apply launch of :class:`GroupLookupGrad` without the reduce in front of it.  What a
trainer needs after it has aggregated the gradients of replicated tables across ranks
(``hb.distribute.ReplicatedGradients``): the five optimizers, with the formulas, rounding and operation
order of ``GroupLookupGrad``'s step, on rows that are distinct and may have holes (``-1``)."""
import ctypes as C

import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import optimizer as _opt

_APPLY = {'sgd': _lib.APPLY_SGD, 'adagrad': _lib.APPLY_ADAGRAD, 'adam': _lib.APPLY_LAZY_ADAM,
          'ftrl': _lib.APPLY_FTRL, 'rowwise_adagrad': _lib.APPLY_ROWWISE_ADAGRAD}


def _bad(msg):
  return _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, msg)


class SparseApply:
  """The sparse optimizer step of N tables from caller-held IndexedSlices, one launch per 64 tables.

  Args:
    tables: list of fp32 ``[rows, dim]`` device tensors, stepped in place.
    accums / moments, adam / ftrl_slots, ftrl / row_accums, rowwise_adagrad: the optimizer slots and objects,
      as :class:`GroupLookupGrad` takes them.

  No workspace and no host read: a call can be captured in a graph, and ``launch()`` repeats it."""

  # what a subclass over another kind of table (embedding/lowp.py) replaces: the name its refusals use, the
  # descriptor, and _require_tables / _fill_table / _foreign_call / _launchable below
  _NAME = 'SparseApply'
  _NEEDS = 'SparseApply(tables, {slots})'
  _COLUMN = _lib.SlicesColumn

  def __init__(self, tables, accums=None, moments=None, adam=None, ftrl_slots=None, ftrl=None, row_accums=None,
               rowwise_adagrad=None):
    self.tables = self._require_tables(tables)
    self._lib = _lib.lib()
    n = len(self.tables)
    _opt.bind_all(self, dict(moments=moments, adam=adam, ftrl_slots=ftrl_slots, ftrl=ftrl, row_accums=row_accums,
                             rowwise_adagrad=rowwise_adagrad), self.tables, self._NAME)
    self._slot_ptrs = {opt.name: opt.ptr_arrays(slots) for opt, slots in _opt.bound(self)}
    self.accums = list(accums) if accums is not None else None
    self._accum_ptrs = None
    if self.accums is not None:
      if len(self.accums) != n:
        raise _bad(f'{self._NAME}: {len(self.accums)} accumulators for {n} tables')
      for c, (a, t) in enumerate(zip(self.accums, self.tables)):
        _lib.require_device_tensor(a, 'accumulator')
        if a.dtype != torch.float32 or a.shape != t.shape:
          raise _bad(f'accumulator {c} must be fp32 {tuple(t.shape)}')
      self._accum_ptrs = _lib.ptr_array([a.data_ptr() for a in self.accums])
    self._cols = (self._COLUMN * n)()
    for c, t in enumerate(self.tables):
      col = self._cols[c]
      col.table = t.data_ptr()
      col.rows = t.shape[0]
      col.dim = t.shape[1]
      self._fill_table(col, t)
    self._bound = None

  def _require_tables(self, tables):
    tables = list(tables)
    for t in tables:
      _lib.require_device_tensor(t, 'embedding weights')
      if t.dtype != torch.float32 or t.dim() != 2:
        raise _bad('embedding weights must be fp32 [rows, dim]')
    return tables

  def _fill_table(self, col, table):
    """What the descriptor holds of its table besides the address and the shape."""

  def _foreign_call(self, apply, s0, s1, params, lr, finish, stream):   # pylint: disable=unused-argument
    return self._lib.hbk_sparse_apply_slices_n(len(self.tables), self._cols, apply, s0, s1, params, lr, stream)

  def _launchable(self, explicit):   # pylint: disable=unused-argument
    """Whether ``launch()`` has what it repeats (explicit: the caller gave lr, optimizer and finish)."""
    return self._bound is not None

  def __len__(self):
    return len(self.tables)

  def _check(self, lr, optimizer):
    two_slot = _opt.two_slot_class(optimizer, self, self._NEEDS)
    if lr == 0.0:
      raise _bad(f'{self._NAME}: lr must be != 0')
    if optimizer == 'adagrad' and self.accums is None:
      raise _bad(f"optimizer='adagrad' needs {self._NAME}(tables, accums=...)")
    return two_slot

  def __call__(self, slices, lr, optimizer='sgd', finish=True):
    """slices[c] = ``(unique_rows int64 [capacity], grad_rows fp32 [capacity, dim], n_unique int32 [1])`` on the
    device.  The first ``n_unique`` entries are read (on the device, clamped to the capacity); an entry outside
    ``[0, rows)`` -- ``-1`` -- touches nothing.  Rows must be DISTINCT (not checked: no step but SGD's is
    additive).  ``optimizer`` and ``finish`` as in :class:`GroupLookupGrad`; the gradient is not clipped."""
    two_slot = self._check(lr, optimizer)
    self.bind(slices)
    self._bound = (float(lr), optimizer, bool(finish))
    self._step(two_slot, float(lr), optimizer, finish)

  def bind(self, slices):
    """Point the descriptors at ``slices`` (checked) without stepping."""
    n = len(self.tables)
    slices = list(slices)
    if len(slices) != n:
      raise _bad(f'{self._NAME}: {len(slices)} slices for {n} tables')
    keep = []
    for c, (s, t) in enumerate(zip(slices, self.tables)):
      if len(s) != 3:
        raise _bad(f'slices[{c}] must be (unique_rows, grad_rows, n_unique)')
      urows, grows, nu = s
      for x, what in ((urows, 'unique_rows'), (grows, 'grad_rows'), (nu, 'n_unique')):
        if not isinstance(x, torch.Tensor):
          raise _bad(f'slices[{c}].{what} must be a device tensor')
        _lib.require_device_tensor(x, f'slices[{c}].{what}')
      if urows.dtype != torch.int64 or urows.dim() != 1:
        raise _bad(f'slices[{c}].unique_rows must be an int64 vector')
      cap, dim = int(urows.shape[0]), int(t.shape[1])
      if grows.dtype != torch.float32 or tuple(grows.shape) != (cap, dim):
        raise _bad(f'slices[{c}].grad_rows must be fp32 [{cap}, {dim}]')
      if nu.dtype != torch.int32 or nu.numel() != 1:
        raise _bad(f'slices[{c}].n_unique must be an int32 device tensor of one element')
      col = self._cols[c]
      col.unique_rows = urows.data_ptr()
      col.grad_rows = grows.data_ptr()
      col.n_unique = nu.data_ptr()
      col.capacity = cap
      keep.append((urows, grows, nu))
    self._keep = keep

  def _step(self, two_slot, lr, optimizer, finish):
    n = len(self.tables)
    dev = self.tables[0].device if n else None
    s0 = s1 = params = None
    if two_slot is not None:
      ptrs = self._slot_ptrs[two_slot.name]
      s0 = ptrs[0]
      s1 = ptrs[1] if len(ptrs) > 1 else None
      params = C.byref(getattr(self, two_slot.name).params(finish))
    elif optimizer == 'adagrad':
      s0 = self._accum_ptrs
    _lib.check(self._foreign_call(_APPLY[optimizer], s0, s1, params, C.c_float(lr), bool(finish),
                                  _lib.current_stream(dev)))

  def launch(self, lr=None, optimizer=None, finish=None):
    """The last call again on the same tensors (refilled in place): one foreign call.  ``lr``, ``optimizer``
    and ``finish`` default to that call's."""
    if not self._launchable(None not in (lr, optimizer, finish)):
      raise _lib.HbkError(_lib.INTERNAL, 'launch() needs a call that bound the slices first')
    lr = self._bound[0] if lr is None else float(lr)
    optimizer = self._bound[1] if optimizer is None else optimizer
    finish = self._bound[2] if finish is None else bool(finish)
    self._step(self._check(lr, optimizer), lr, optimizer, finish)
