"""The weight-gradient entries without a device: the symbols and their prototypes, the struct sizes
they must not have changed, the refusals made before any launch, the Python layer's own refusals, and
the float64 restatement the GPU tests compare with against torch autograd."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd import _marshal
from tests.support import weight_grad_ref as ref

FAKE = 0x7f0000001000
FAKE2 = 0x7f0000101000
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'hbk.h')


def _refused(rc, *words, code=None):
  assert rc == (_lib.INVALID_ARGUMENT if code is None else code), rc
  msg = _lib.lib().hbk_last_error().decode()
  for w in words:
    assert w in msg, (w, msg)


def _grad_col(**kw):
  col = _lib.LookupGradColumn()
  col.table, col.rows, col.dim = FAKE, 100, 16
  col.ids_dtype, col.ids, col.n_ids, col.n_segments = _lib.INT64, FAKE, 8, 8
  col.divisor, col.combiner, col.grad_out = 1, _lib.COMBINER_MEAN, FAKE
  col.id_weights = FAKE2
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def test_symbols_and_prototypes():
  lib = _lib.lib()
  vp, i32 = C.c_void_p, C.c_int32
  assert lib.hbk_group_lookup_bwd_weights.argtypes == [i32, vp, vp, vp, vp]
  assert lib.hbk_group_lookup_bwd_weights.restype is C.c_int
  assert lib.hbk_sharded_lookup_bwd_weights.argtypes == [vp, vp, vp, vp, vp]
  assert lib.hbk_sharded_lookup_bwd_weights.restype is C.c_int
  text = open(HEADER).read()
  flat = re.sub(r'\s+', ' ', text)
  assert ('int hbk_group_lookup_bwd_weights(int32_t n_cols, const hbk_lookup_grad_column_t* cols, '
          'const float* max_norms, float* const* grad_weights, hbk_stream_t stream);') in flat
  assert ('int hbk_sharded_lookup_bwd_weights(hbk_sharded_t plan, const float* const* grads, '
          'const int32_t* grad_strides, float* const* grad_weights, hbk_stream_t stream);') in flat
  assert 'No gradient for the weights themselves' not in text


def test_version_and_struct_sizes_unchanged():
  assert _lib.lib().hbk_version().decode().startswith('hbk 0.2.0')
  # the sizes the 0.2.0 ABI tests pin (tests/test_abi.py, tests/test_weighted_abi.py)
  assert C.sizeof(_lib.LookupGradColumn) == 160
  assert C.sizeof(_lib.LookupColumn) == 128
  assert C.sizeof(_lib.StitchGradColumn) == 88


def test_nothing_wanted_is_a_no_op():
  lib = _lib.lib()
  cols = (_lib.LookupGradColumn * 2)(_grad_col(), _grad_col(id_weights=None))
  assert lib.hbk_group_lookup_bwd_weights(2, cols, None, _lib.ptr_array([0, 0]), None) == _lib.OK
  assert lib.hbk_group_lookup_bwd_weights(0, None, None, None, None) == _lib.OK


def test_an_unwanted_column_is_skipped_unread():
  # (segmented inputs and a bad max_norm are refused on the columns whose gradient is wanted only)
  cols = (_lib.LookupGradColumn * 2)(_grad_col(n_runs=2, run_start=FAKE, run_ids=FAKE, run_grads=FAKE),
                                     _grad_col(dim=0))
  norms = (C.c_float * 2)(float('nan'), -1.0)
  assert _lib.lib().hbk_group_lookup_bwd_weights(2, cols, norms, _lib.ptr_array([0, 0]), None) == _lib.OK


def test_refuses_a_column_without_weights():
  cols = (_lib.LookupGradColumn * 2)(_grad_col(), _grad_col(id_weights=None))
  rc = _lib.lib().hbk_group_lookup_bwd_weights(2, cols, None, _lib.ptr_array([FAKE, FAKE2]), None)
  _refused(rc, 'column 1', 'id_weights')


def test_refuses_segmented_inputs():
  cols = (_lib.LookupGradColumn * 1)(_grad_col(n_runs=2, run_start=FAKE, run_ids=FAKE, run_grads=FAKE))
  rc = _lib.lib().hbk_group_lookup_bwd_weights(1, cols, None, _lib.ptr_array([FAKE]), None)
  _refused(rc, 'column 0', 'n_runs')


@pytest.mark.parametrize('bad', [-1.0, float('nan'), float('inf')])
def test_refuses_bad_max_norm(bad):
  cols = (_lib.LookupGradColumn * 2)(_grad_col(), _grad_col())
  norms = (C.c_float * 2)(1.0, bad)
  rc = _lib.lib().hbk_group_lookup_bwd_weights(2, cols, norms, _lib.ptr_array([FAKE, FAKE2]), None)
  _refused(rc, 'column 1', 'max_norm')


def test_refuses_bad_columns_before_any_launch():
  lib = _lib.lib()
  out = _lib.ptr_array([FAKE])
  for kw, word in ((dict(dim=0), 'dim'), (dict(combiner=7), 'combiner'), (dict(n_segments=3), 'n_segments'),
                   (dict(ids=None), 'NULL buffer'), (dict(table_pitch=8), 'table_pitch'),
                   (dict(grad_stride=8), 'grad_stride'), (dict(dim=65, table=FAKE + 4), '64 lanes'),
                   (dict(dim=260), '64 lanes')):
    cols = (_lib.LookupGradColumn * 1)(_grad_col(**kw))
    _refused(lib.hbk_group_lookup_bwd_weights(1, cols, None, out, None), word)
  _refused(lib.hbk_group_lookup_bwd_weights(1, None, None, out, None), 'NULL')


def test_sharded_entry_refuses_a_null_plan():
  rc = _lib.lib().hbk_sharded_lookup_bwd_weights(None, _lib.ptr_array([FAKE]), None, _lib.ptr_array([FAKE]),
                                                 None)
  _refused(rc, 'plan is NULL')


def test_python_request():
  w = torch.zeros(4)
  req = _marshal.weight_grad_request
  assert req(False, [w, None], 2) is None
  assert req(None, None, 2) is None
  assert req(True, [w, None], 2) == [True, None]
  assert req([None, None], [w, None], 2) is None
  out = torch.zeros(4)
  got = req([out, None], [w, None], 2)
  assert got[0] is out and got[1] is None
  for flag, sp in ((True, None), (True, [None, None]), ([None, True], [w, None]), ([True], [w, None]),
                   ([3.0, None], [w, None]), (7, [w, None]), (True, [w])):
    with pytest.raises(_lib.InvalidArgumentError):
      req(flag, sp, 2)


def test_python_outputs_are_checked():
  ids = [torch.zeros(5, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)]
  outs = _marshal.weight_grad_outputs([True, None], ids, 'cpu')
  assert outs[1] is None and tuple(outs[0].shape) == (5,) and outs[0].dtype is torch.float32
  both = _marshal.weight_grad_outputs([True, True], ids, 'cpu')
  assert [tuple(o.shape) for o in both] == [(5,), (3,)]
  assert both[1].data_ptr() % 16 == both[0].data_ptr() % 16


@pytest.mark.parametrize('comb', ['sum', 'mean', 'sqrtn'])
@pytest.mark.parametrize('clip', [None, 0.75])
def test_restatement_equals_autograd(comb, clip):
  rng = np.random.RandomState(5)
  rows, dim, S = 37, 6, 11
  table = rng.uniform(-1, 1, size=(rows, dim))
  sp = np.concatenate([[0], np.cumsum(rng.randint(0, 5, size=S))])
  n = int(sp[-1])
  ids = rng.randint(-3, rows + 3, size=n)
  w = rng.uniform(0.2, 2, size=n)
  G = rng.randn(S, dim)
  r, valid = ref.rows_of(ids, rows)
  t = torch.tensor(table, dtype=torch.float64)
  if clip:
    t = t * clip / torch.clamp(t.norm(dim=1, keepdim=True), min=clip)
  wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
  loss = 0
  for s in range(S):
    j = [k for k in range(sp[s], sp[s + 1]) if valid[k]]
    if not j:
      continue
    num = (wt[j][:, None] * t[r[j]]).sum(0)
    den = 1.0 if comb == 'sum' else wt[j].sum() if comb == 'mean' else (wt[j] ** 2).sum().sqrt()
    loss = loss + (torch.tensor(G[s]) * (num / den)).sum()
  loss.backward()
  dw, mag, _ = ref.weight_grad(table, ids, sp, w, comb, G, max_norm=clip)
  np.testing.assert_allclose(dw, wt.grad.numpy(), rtol=0, atol=1e-13)
  assert (np.abs(dw) <= mag + 1e-15).all() and (dw[~valid] == 0).all()
  out, _ = ref.forward(table, ids, sp, w, comb, max_norm=clip)
  assert abs(float((out * G).sum()) - float(loss.detach())) < 1e-12
