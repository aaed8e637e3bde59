"""The two-slot sparse optimizers' shared state: Lazy Adam (``tf.contrib.opt.LazyAdamOptimizer``,
TF 1.15) -- the hyperparameters and the device-side beta powers -- and FTRL-Proximal
(``tf.train.FtrlOptimizer``, TF 1.15) -- the hyperparameters only."""
import math
import ctypes as C

import torch

from hybridbackend_amd import _lib


class LazyAdam:
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


class Ftrl:
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

  def params(self):
    """The ``hbk_ftrl_t`` of a call (kept alive by this object)."""
    return self._params

  def slots_like(self, table):
    """A new ``(accum, linear)`` pair for ``table``: TF's initial values."""
    return (torch.full_like(table, self.initial_accumulator_value), torch.zeros_like(table))
