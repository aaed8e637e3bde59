"""Lazy Adam at the C ABI, without a GPU: the new symbols exist, every refused combination is refused
before any device work with the field named, and the step-only workspace holds the emit form's plus
the per-column IndexedSlices."""
import ctypes as C

import pytest

from hybridbackend_amd import _lib

FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it
M, V, T2, M2, V2, POW = (FAKE + k * 0x100000 for k in range(1, 7))


def test_new_symbols_and_unchanged_version():
  lib = _lib.lib()
  for name in ('hbk_group_lookup_bwd_adam_workspace_bytes', 'hbk_group_lookup_bwd_adam',
               'hbk_sharded_set_adam_slots', 'hbk_sharded_lookup_bwd_adam'):
    assert hasattr(lib, name), name
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  assert _lib.LookupGradColumn._fields_[-1][0] == 'id_weights'
  assert [f[0] for f in _lib.AdamParams._fields_] == ['beta1', 'beta2', 'epsilon', 'beta_powers', 'finish']


def _col(**kw):
  col = _lib.LookupGradColumn()
  col.table, col.rows, col.dim = FAKE, 100, 16
  col.ids_dtype, col.ids, col.n_ids, col.n_segments = _lib.INT64, FAKE, 8, 8
  col.divisor, col.combiner, col.grad_out = 1, _lib.COMBINER_SUM, FAKE
  col.unique_rows, col.grad_rows, col.n_unique = FAKE, FAKE, FAKE
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _adam(**kw):
  a = _lib.AdamParams(0.9, 0.999, 1e-8, POW, 1)
  for k, v in kw.items():
    setattr(a, k, v)
  return a


def _call(cols, m, v, adam=None, lr=0.01):
  lib = _lib.lib()
  n = len(cols)
  arr = (_lib.LookupGradColumn * n)(*cols)
  return lib.hbk_group_lookup_bwd_adam(n, arr, _lib.ptr_array(m), _lib.ptr_array(v),
                                       C.byref(adam if adam is not None else _adam()), C.c_float(lr),
                                       C.c_void_p(FAKE), C.c_size_t(1 << 40), None)


def _refused(rc, *words):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in words:
    assert w in msg, msg


@pytest.mark.parametrize('case', [
  'm_null', 'v_null', 'm_is_v', 'm_is_table', 'v_is_table', 'accum', 'beta1_high', 'beta1_neg',
  'beta2_one', 'eps_neg', 'eps_inf', 'eps_nan', 'powers_null', 'lr_zero', 'same_table',
  'same_slot', 'slot_is_other_table'])
def test_refusals(case):
  c0, m, v, adam, lr = _col(), [M], [V], _adam(), 0.01
  cols = [c0]
  words = ()
  if case == 'm_null':
    m, words = [None], ('m is NULL',)
  elif case == 'v_null':
    v, words = [None], ('v is NULL',)
  elif case == 'm_is_v':
    v, words = [M], ('m and v',)
  elif case == 'm_is_table':
    m, words = [FAKE], ('m is the table',)
  elif case == 'v_is_table':
    v, words = [FAKE], ('v is the table',)
  elif case == 'accum':
    cols, words = [_col(accum=FAKE + 0x800000)], ('accum',)
  elif case == 'beta1_high':
    adam, words = _adam(beta1=1.0), ('beta1',)
  elif case == 'beta1_neg':
    adam, words = _adam(beta1=-0.1), ('beta1',)
  elif case == 'beta2_one':
    adam, words = _adam(beta2=1.0), ('beta2',)
  elif case == 'eps_neg':
    adam, words = _adam(epsilon=-1e-8), ('epsilon',)
  elif case == 'eps_inf':
    adam, words = _adam(epsilon=float('inf')), ('epsilon',)
  elif case == 'eps_nan':
    adam, words = _adam(epsilon=float('nan')), ('epsilon',)
  elif case == 'powers_null':
    adam, words = _adam(beta_powers=None), ('beta_powers',)
  elif case == 'lr_zero':
    lr, words = 0.0, ('lr',)
  elif case == 'same_table':
    cols, m, v, words = [c0, _col()], [M, M2], [V, V2], ('same table',)
  elif case == 'same_slot':
    cols, m, v, words = [c0, _col(table=T2)], [M, M], [V, V2], ('same table, m or v',)
  elif case == 'slot_is_other_table':
    cols, m, v, words = [c0, _col(table=T2)], [M, M2], [T2, V2], ('same table, m or v',)
  _refused(_call(cols, m, v, adam, lr), *words)


def test_refusals_without_arrays_or_params():
  lib = _lib.lib()
  arr = (_lib.LookupGradColumn * 1)(_col())
  _refused(lib.hbk_group_lookup_bwd_adam(1, arr, None, None, C.byref(_adam()), C.c_float(0.1),
                                         C.c_void_p(FAKE), C.c_size_t(1 << 40), None), 'm / v')
  _refused(lib.hbk_group_lookup_bwd_adam(1, arr, _lib.ptr_array([M]), _lib.ptr_array([V]), None,
                                         C.c_float(0.1), C.c_void_p(FAKE), C.c_size_t(1 << 40), None),
           'adam')


def test_sharded_refusals_without_a_plan():
  lib = _lib.lib()
  _refused(lib.hbk_sharded_set_adam_slots(None, _lib.ptr_array([M]), _lib.ptr_array([V])), 'plan')
  _refused(lib.hbk_sharded_lookup_bwd_adam(None, None, None, C.byref(_adam()), C.c_float(0.1),
                                           None, None, None, None), 'plan')


def test_step_only_workspace_holds_the_emit_form_and_the_slices():
  lib = _lib.lib()
  col = _col(rows=1000, dim=12, n_ids=777, n_segments=300, row_splits=FAKE,
             combiner=_lib.COMBINER_MEAN)
  emit = lib.hbk_group_lookup_bwd_adam_workspace_bytes(1, (_lib.LookupGradColumn * 1)(col))
  plain = lib.hbk_group_lookup_bwd_workspace_bytes(1, (_lib.LookupGradColumn * 1)(col))
  assert emit >= plain > 0
  col.unique_rows, col.grad_rows = None, None
  step = lib.hbk_group_lookup_bwd_adam_workspace_bytes(1, (_lib.LookupGradColumn * 1)(col))
  assert step >= emit + 777 * 8 + 777 * 12 * 4


def test_python_refusals_without_a_gpu():
  from hybridbackend_amd.embedding import GroupLookupGrad, LazyAdam
  with pytest.raises(_lib.InvalidArgumentError, match='beta1'):
    LazyAdam(beta1=1.0, device='cpu')
  with pytest.raises(_lib.InvalidArgumentError, match='epsilon'):
    LazyAdam(epsilon=-1.0, device='cpu')
  grad = GroupLookupGrad.__new__(GroupLookupGrad)
  grad.moments = None
  with pytest.raises(_lib.InvalidArgumentError, match='moments'):
    grad([], [], apply_lr=0.1, optimizer='adam')
  with pytest.raises(_lib.InvalidArgumentError, match='adam'):
    grad([], [], apply_lr=0.1, optimizer='rmsprop')


def test_saver_keeps_0d_tensors_and_restores_shards_whole(tmp_path):
  """Adam's beta1_power / beta2_power are 0-d; a table sharded at W = 2 restores whole at W = 1."""
  import numpy as np
  import torch
  from hybridbackend_amd.training.saver import Saver, ShardedSlice
  powers = torch.tensor([0.729, 0.997003])
  full = torch.arange(30, dtype=torch.float32).view(10, 3)
  prefix = str(tmp_path / 'ck')
  import threading
  barrier = threading.Barrier(2)

  def save(r):
    Saver(r, 2, barrier.wait).save(prefix, {'beta1_power': powers[0], 'beta2_power': powers[1],
                                            't': ShardedSlice(full[r::2].clone(), 10, 2, r)})
  threads = [threading.Thread(target=save, args=(r,)) for r in range(2)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=30)
  got, whole = torch.zeros(2), torch.zeros(10, 3)
  Saver().restore(prefix, {'beta1_power': got[0], 'beta2_power': got[1], 't': whole})
  np.testing.assert_array_equal(got.numpy(), powers.numpy())
  np.testing.assert_array_equal(whole.numpy(), full.numpy())
