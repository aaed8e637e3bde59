"""Lazy Adam (``tf.contrib.opt.LazyAdamOptimizer``, TF 1.15): the state every step of one optimizer
shares -- the hyperparameters and the device-side beta powers."""
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
