"""The slot optimizers that step after the emit-form reduce: Lazy Adam (``tf.contrib.opt.LazyAdamOptimizer``,
TF 1.15) -- the hyperparameters and the device-side beta powers --, FTRL-Proximal
(``tf.train.FtrlOptimizer``, TF 1.15) -- the hyperparameters only -- and row-wise Adagrad (one
accumulator per row).  Each class also carries what ``GroupLookupGrad``,
``ShardedGroupLookup`` and ``DenseFeatures`` need to know of it: its ``optimizer=`` name, the keyword
of its slots (pairs of table-shaped tensors, or one ``[rows, 1]`` tensor per table), fresh slots, its
checkpoint names and its C entry points.  ``TWO_SLOT`` lists them (one or two slots each); adding one
here is all those drivers need."""
import math
import ctypes as C

import torch

from hybridbackend_amd import _lib


class _TwoSlot:
  """What the drivers use of a slot optimizer.  A subclass sets ``name`` (``optimizer=``, and the
  drivers' attribute holding the object), ``slot_kw`` (the drivers' keyword and attribute of the
  slots), ``slot_names`` (two names: every table's entry is a pair of tensors; one name: it is the one
  tensor itself), ``tf_suffixes`` (checkpoint names of the slots), and implements
  ``params(finish)`` (the C parameter struct), ``slots_like(table)``, ``_c(lib)`` (its C entry
  points: group step, workspace query, sharded slot registration, sharded step) and ``_c_clipped(lib)``
  (the max_norm forms of the group step and its workspace query).  ``slot_shape(table)``: the shape of
  every slot of ``table`` (the table's own unless overridden)."""

  @staticmethod
  def slot_shape(table):
    return tuple(table.shape)

  @classmethod
  def slot_tensors(cls, entry):
    """One table's entry of the slot list as a tuple of tensors, in the order of ``slot_names``."""
    return (entry,) if len(cls.slot_names) == 1 else tuple(entry)

  @classmethod
  def ptr_arrays(cls, slots):
    """The C pointer arrays of a slot list: one per slot name, each with one pointer per table."""
    return tuple(_lib.ptr_array([cls.slot_tensors(e)[k].data_ptr() for e in slots])
                 for k in range(len(cls.slot_names)))

  @classmethod
  def needs_text(cls):
    """``kw=[...]`` as the refusals spell it."""
    if len(cls.slot_names) == 1:
      return f'{cls.slot_kw}=[{cls.slot_names[0]}, ...]'
    return f'{cls.slot_kw}=[({cls.slot_names[0]}, {cls.slot_names[1]}), ...]'

  def tf_variables(self):
    """Checkpoint variables besides the slots: ``{name: tensor}``."""
    return {}

  @classmethod
  def workspace_bytes(cls, n, cols, max_norms=None):
    if max_norms is not None:
      return cls._c_clipped(_lib.lib())[1](n, cols, max_norms)
    return cls._c(_lib.lib())[1](n, cols)

  def group_step(self, n, cols, slot_ptrs, lr, ws, stream, finish=True, max_norms=None):
    """The step of ``GroupLookupGrad``: the emit-form reduce and the apply on ``n`` descriptors;
    ``slot_ptrs``: :meth:`ptr_arrays` of the slots; ``max_norms`` (a ctypes float array, or None): the
    clipped form."""
    lib = _lib.lib()
    head = (n, cols) if max_norms is None else (n, cols, max_norms)
    fn = self._c(lib)[0] if max_norms is None else self._c_clipped(lib)[0]
    _lib.check(fn(*head, *slot_ptrs, C.byref(self.params(finish)), C.c_float(lr),
                  C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()), stream))

  def set_sharded_slots(self, plan, slots):
    """Every column's slot shards, registered with a sharded plan."""
    _lib.check(self._c(_lib.lib())[2](plan, *self.ptr_arrays(slots)))

  def sharded_step(self, plan, grads, strides, lr, unique_rows, grad_rows, n_unique, stream,
                   finish=True):
    """The step of ``ShardedGroupLookup.backward`` (pointer arrays; unique_rows / grad_rows None: step
    only)."""
    _lib.check(self._c(_lib.lib())[3](plan, grads, strides, C.byref(self.params(finish)),
                                      C.c_float(lr), unique_rows, grad_rows, n_unique, stream))


class LazyAdam(_TwoSlot):
  """The sparse Adam step of ``GroupLookupGrad`` / ``ShardedGroupLookup`` / ``DenseFeatures`` with
  ``optimizer='adam'``: for every distinct row r of a step, with its deduplicated gradient g, in fp32::

      lr_t = (lr * sqrt(1 - beta2_power)) / (1 - beta1_power)
      m[r] = beta1 * m[r] + (1 - beta1) * g
      v[r] = beta2 * v[r] + (1 - beta2) * g * g
      w[r] = w[r] - (lr_t * m[r]) / (sqrt(v[r]) + epsilon)

  Rows that do not occur in the step are not touched at all (that is what makes it lazy;
  ``tf.train.AdamOptimizer``'s sparse path decays and moves every row, a full-table pass this library
  does not provide).  ``beta_powers`` lives on the device ([beta1^t, beta2^t], starting at
  [beta1, beta2]) and is advanced after the step by the step itself (TF's ``_finish``), so a captured
  graph replayed K times makes K correct steps.  Share ONE object between everything one optimizer
  steps, as TF does; when one optimizer step spans several calls, pass ``finish=False`` to all but the
  last."""
  name, slot_kw, slot_names = 'adam', 'moments', ('m', 'v')
  tf_suffixes = ('/Adam', '/Adam_1')

  def __init__(self, beta1=0.9, beta2=0.999, epsilon=1e-8, device=None):
    for name, b in (('beta1', beta1), ('beta2', beta2)):
      if not 0.0 <= float(b) < 1.0:
        raise _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, f'{name} must be in [0, 1), got {b}')
    if not 0.0 <= float(epsilon) < float('inf'):
      raise _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT,
                                      f'epsilon must be finite and >= 0, got {epsilon}')
    self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
    if device is None:
      device = torch.device('cuda', torch.cuda.current_device())
    self.beta_powers = torch.tensor([self.beta1, self.beta2], dtype=torch.float32, device=device)
    self._params = {}

  @property
  def device(self):
    return self.beta_powers.device

  def params(self, finish=True):
    """The ``hbk_adam_t`` of a call (kept alive by this object)."""
    key = bool(finish)
    p = self._params.get(key)
    if p is None or p.beta_powers != self.beta_powers.data_ptr():
      p = _lib.AdamParams(C.c_float(self.beta1), C.c_float(self.beta2), C.c_float(self.epsilon),
                          self.beta_powers.data_ptr(), 1 if finish else 0)
      self._params[key] = p
    return p

  @classmethod
  def default(cls, device):
    return cls(device=device)

  def slots_like(self, table):
    """A new ``(m, v)`` pair for ``table``: zeros."""
    return (torch.zeros_like(table), torch.zeros_like(table))

  def tf_variables(self):
    # (0-d views of the device pair: a restore writes into it)
    return {'beta1_power': self.beta_powers[0], 'beta2_power': self.beta_powers[1]}

  @staticmethod
  def _c(lib):
    return (lib.hbk_group_lookup_bwd_adam, lib.hbk_group_lookup_bwd_adam_workspace_bytes,
            lib.hbk_sharded_set_adam_slots, lib.hbk_sharded_lookup_bwd_adam)

  @staticmethod
  def _c_clipped(lib):
    return (lib.hbk_group_lookup_bwd_adam_clipped, lib.hbk_group_lookup_bwd_adam_clipped_workspace_bytes)


class Ftrl(_TwoSlot):
  """The sparse FTRL-Proximal step of ``GroupLookupGrad`` / ``ShardedGroupLookup`` / ``DenseFeatures``
  with ``optimizer='ftrl'`` (TF 1.15 ``SparseApplyFtrl`` / ``SparseApplyFtrlV2``, the sparse apply of
  ``tf.train.FtrlOptimizer``): for every distinct row r of a step, with its deduplicated gradient g,
  in fp32, a = accum[r], z = linear[r], w = weights[r]::

      gs = g if l2_shrinkage == 0 else g + (2 * l2_shrinkage) * w
      na = a + g * g
      p(x) = sqrt(x) if lr_power == -0.5 else x ** -lr_power
      z  = z + (gs - ((p(na) - p(a)) / lr) * w)
      w  = (clip(z, -l1, l1) - z) / (p(na) / lr + 2 * l2)
      a  = na

  Rows that do not occur in the step are not touched, as in TF's sparse apply.  The slots are the
  accumulator (filled with ``initial_accumulator_value``) and the linear term (zeros).  There is no
  device state: one object may serve any number of calls."""
  name, slot_kw, slot_names = 'ftrl', 'ftrl_slots', ('accum', 'linear')
  tf_suffixes = ('/Ftrl', '/Ftrl_1')

  def __init__(self, l1=0.0, l2=0.0, l2_shrinkage=0.0, lr_power=-0.5, initial_accumulator_value=0.1):
    # tf.train.FtrlOptimizer.__init__ and the SparseApplyFtrl kernel refuse the same
    for name, x in (('l1', l1), ('l2', l2), ('l2_shrinkage', l2_shrinkage)):
      if not (math.isfinite(float(x)) and float(x) >= 0.0):
        raise _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, f'{name} must be finite and >= 0, got {x}')
    if not (math.isfinite(float(lr_power)) and float(lr_power) <= 0.0):
      raise _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT,
                                      f'lr_power must be finite and <= 0, got {lr_power}')
    if not float(initial_accumulator_value) >= 0.0:
      raise _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, 'initial_accumulator_value must be >= 0, '
                                      f'got {initial_accumulator_value}')
    self.l1, self.l2, self.l2_shrinkage = float(l1), float(l2), float(l2_shrinkage)
    self.lr_power = float(lr_power)
    self.initial_accumulator_value = float(initial_accumulator_value)
    self._params = _lib.FtrlParams(C.c_float(self.l1), C.c_float(self.l2),
                                   C.c_float(self.l2_shrinkage), C.c_float(self.lr_power))

  def params(self, finish=True):   # pylint: disable=unused-argument
    """The ``hbk_ftrl_t`` of a call (kept alive by this object; ``finish`` is Adam's)."""
    return self._params

  @classmethod
  def default(cls, device):   # pylint: disable=unused-argument
    return cls()

  def slots_like(self, table):
    """A new ``(accum, linear)`` pair for ``table``: TF's initial values."""
    return (torch.full_like(table, self.initial_accumulator_value), torch.zeros_like(table))

  @staticmethod
  def _c(lib):
    return (lib.hbk_group_lookup_bwd_ftrl, lib.hbk_group_lookup_bwd_ftrl_workspace_bytes,
            lib.hbk_sharded_set_ftrl_slots, lib.hbk_sharded_lookup_bwd_ftrl)

  @staticmethod
  def _c_clipped(lib):
    return (lib.hbk_group_lookup_bwd_ftrl_clipped, lib.hbk_group_lookup_bwd_ftrl_clipped_workspace_bytes)


class RowwiseAdagrad(_TwoSlot):
  """Row-wise Adagrad, the step of ``GroupLookupGrad`` / ``ShardedGroupLookup`` / ``DenseFeatures`` with
  ``optimizer='rowwise_adagrad'``: ONE fp32 accumulator per row.  For every distinct row r of a step, with
  its deduplicated gradient g (after a ``max_norm`` clip: g'), in fp32::

      s    = sum_k g[k] * g[k]
      a[r] = a[r] + s / dim
      w[r] = w[r] - (lr / (sqrt(a[r]) + epsilon)) * g

  (``include/hbk.h``, ``hbk_group_lookup_bwd_rowwise_adagrad``, fixes the rounding and the order of s).
  Rows that do not occur in the step are not touched.  The slot is ``row_accums``: per table one fp32
  ``[rows, 1]`` tensor filled with ``initial_accumulator_value`` -- 4 bytes of optimizer state per row
  instead of Adagrad's ``4 * dim``.  There is no device state: one object may serve any number of calls."""
  name, slot_kw, slot_names = 'rowwise_adagrad', 'row_accums', ('accum',)
  tf_suffixes = ('/RowwiseAdagrad',)

  def __init__(self, epsilon=1e-8, initial_accumulator_value=0.0):
    for name, x in (('epsilon', epsilon), ('initial_accumulator_value', initial_accumulator_value)):
      if not (math.isfinite(float(x)) and float(x) >= 0.0):
        raise _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, f'{name} must be finite and >= 0, got {x}')
    if float(epsilon) == 0.0 and float(initial_accumulator_value) == 0.0:
      raise _lib.InvalidArgumentError(
        _lib.INVALID_ARGUMENT, 'epsilon and initial_accumulator_value must not both be 0 (a row whose gradient '
        'is all zero would compute 0 / 0)')
    self.epsilon = float(epsilon)
    self.initial_accumulator_value = float(initial_accumulator_value)
    self._params = _lib.RowwiseAdagradParams(C.c_float(self.epsilon))

  def params(self, finish=True):   # pylint: disable=unused-argument
    """The ``hbk_rowwise_adagrad_t`` of a call (kept alive by this object; ``finish`` is Adam's)."""
    return self._params

  @classmethod
  def default(cls, device):   # pylint: disable=unused-argument
    return cls()

  @staticmethod
  def slot_shape(table):
    return (int(table.shape[0]), 1)

  def slots_like(self, table):
    """A new ``[rows, 1]`` accumulator for ``table``, filled with ``initial_accumulator_value``."""
    return torch.full((int(table.shape[0]), 1), self.initial_accumulator_value, dtype=torch.float32,
                      device=table.device)

  @staticmethod
  def _c(lib):
    return (lib.hbk_group_lookup_bwd_rowwise_adagrad, lib.hbk_group_lookup_bwd_rowwise_adagrad_workspace_bytes,
            lib.hbk_sharded_set_rowwise_adagrad_slots, lib.hbk_sharded_lookup_bwd_rowwise_adagrad)

  @staticmethod
  def _c_clipped(lib):
    return (lib.hbk_group_lookup_bwd_rowwise_adagrad_clipped,
            lib.hbk_group_lookup_bwd_rowwise_adagrad_clipped_workspace_bytes)


# the slot optimizers (one or two slots per table) by their optimizer= name; 'sgd' and 'adagrad' are fused
# into the reduce
TWO_SLOT = {c.name: c for c in (LazyAdam, Ftrl, RowwiseAdagrad)}
_NAMES = ['sgd', 'adagrad'] + list(TWO_SLOT)


def two_slot_class(optimizer, owner=None, needs=''):
  """The slot-optimizer class ``optimizer`` names, or None for a fused step ('sgd', 'adagrad').  Refuses
  other names and -- with an ``owner`` -- a slot optimizer whose slots the owner does not hold;
  ``needs``: how to build one that does (formatted with the class's ``name``, ``kw``, ``s0``, ``s1``
  and ``slots``, the whole ``kw=[...]`` argument as :meth:`_TwoSlot.needs_text` spells it)."""
  if optimizer in ('sgd', 'adagrad'):
    return None
  cls = TWO_SLOT.get(optimizer)
  if cls is None:
    raise _lib.InvalidArgumentError(
      _lib.INVALID_ARGUMENT,
      'optimizer must be ' + ', '.join(repr(n) for n in _NAMES[:-1]) + f' or {_NAMES[-1]!r}')
  if owner is not None and getattr(owner, cls.slot_kw, None) is None:
    raise _lib.InvalidArgumentError(
      _lib.INVALID_ARGUMENT, f"optimizer='{cls.name}' needs " + needs.format(
        name=cls.name, kw=cls.slot_kw, s0=cls.slot_names[0], s1=cls.slot_names[-1], slots=cls.needs_text()))
  return cls


def bind_slots(cls, pairs, opt, tables, what):
  """A driver's ``(slots, optimizer)`` of one slot-optimizer class from its keyword arguments: the
  slots (pairs, or one tensor per table) checked against ``tables`` (None when not given) and, with
  slots, an optimizer with the class's defaults when ``opt`` is None."""
  if pairs is None:
    return None, opt
  pairs = _lib.require_slot_pairs(pairs, tables, what, cls.slot_kw, cls.slot_names, cls.slot_shape)
  return pairs, opt if opt is not None else cls.default(tables[0].device if tables else None)


def bind_all(owner, given, tables, what):
  """``bind_slots`` for every class of ``TWO_SLOT``: ``given`` maps the drivers' keywords (every ``slot_kw``
  and ``name``; absent = None) to what the caller passed, and the results become ``owner``'s attributes of
  the same names."""
  for cls in TWO_SLOT.values():
    slots, opt = bind_slots(cls, given.get(cls.slot_kw), given.get(cls.name), tables, what)
    setattr(owner, cls.slot_kw, slots)
    setattr(owner, cls.name, opt)


def bound(owner):
  """``(optimizer object, slot list)`` of every class whose slots ``owner`` holds."""
  return [(getattr(owner, cls.name), getattr(owner, cls.slot_kw)) for cls in TWO_SLOT.values()
          if getattr(owner, cls.slot_kw, None) is not None]


def slot_kwargs(owner, idx=None):
  """The drivers' keyword arguments of every class from ``owner``'s attributes (tables ``idx``, or all)."""
  kw = {}
  for cls in TWO_SLOT.values():
    slots = getattr(owner, cls.slot_kw, None)
    kw[cls.slot_kw] = slots if slots is None or idx is None else [slots[c] for c in idx]
    kw[cls.name] = getattr(owner, cls.name, None)
  return kw
