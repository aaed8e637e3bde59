"""max_norm (TF's embedding_lookup[_sparse](..., max_norm=)) at the C ABI, without a GPU: the clipped
entry points exist beside unchanged structs and version, and every refused argument is refused before
any device work, with the reason named."""
import ctypes as C
import math

import pytest

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import lookup as _lookup

FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it
FAKE2 = 0x7f0000101000

_SYMBOLS = ('hbk_group_lookup_fwd_clipped',
            'hbk_group_lookup_bwd_apply_clipped_workspace_bytes', 'hbk_group_lookup_bwd_apply_clipped',
            'hbk_group_lookup_bwd_adam_clipped_workspace_bytes', 'hbk_group_lookup_bwd_adam_clipped',
            'hbk_group_lookup_bwd_ftrl_clipped_workspace_bytes', 'hbk_group_lookup_bwd_ftrl_clipped')


def test_symbols_version_and_struct_layouts_unchanged():
  import hybridbackend_amd
  lib = _lib.lib()
  for name in _SYMBOLS:
    assert hasattr(lib, name), name
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  assert hybridbackend_amd.__version__ == '0.2.0'
  for cls in (_lib.LookupColumn, _lib.LookupGradColumn, _lib.StitchGradColumn):
    assert cls._fields_[-1][0] == 'id_weights', cls
  # the 0.2.0 sizes (x86-64): nothing was added to the column structs
  assert C.sizeof(_lib.LookupColumn) == 128
  assert C.sizeof(_lib.LookupGradColumn) == 160
  assert C.sizeof(_lib.StitchGradColumn) == 88


def _norms(*xs):
  return (C.c_float * len(xs))(*xs)


def _refused(rc, *words, code=_lib.INVALID_ARGUMENT):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == code, (rc, msg)
  for w in words:
    assert w in msg, msg


def _fwd_col(**kw):
  col = _lib.LookupColumn()
  col.table, col.rows, col.dim = FAKE, 100, 16
  col.ids_dtype, col.ids, col.n_ids, col.n_segments = _lib.INT64, FAKE, 8, 8
  col.divisor, col.combiner, col.out = 1, _lib.COMBINER_SUM, FAKE
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _grad_col(table=FAKE, accum=None, **kw):
  col = _lib.LookupGradColumn()
  col.table, col.rows, col.dim = table, 100, 16
  col.ids_dtype, col.ids, col.n_ids, col.n_segments = _lib.INT64, FAKE, 8, 8
  col.divisor, col.combiner, col.grad_out = 1, _lib.COMBINER_SUM, FAKE
  col.unique_rows, col.grad_rows, col.n_unique = FAKE, FAKE, FAKE
  col.accum = accum
  for k, v in kw.items():
    setattr(col, k, v)
  return col


@pytest.mark.parametrize('bad', [-1.0, float('nan'), float('inf'), -float('inf')])
def test_forward_refuses_bad_max_norms(bad):
  cols = (_lib.LookupColumn * 2)(_fwd_col(), _fwd_col())
  rc = _lib.lib().hbk_group_lookup_fwd_clipped(2, cols, _norms(1.0, bad), None)
  _refused(rc, 'column 1', 'max_norm')


def test_forward_refuses_null_max_norms():
  cols = (_lib.LookupColumn * 1)(_fwd_col())
  _refused(_lib.lib().hbk_group_lookup_fwd_clipped(1, cols, None, None), 'max_norms is NULL')


def test_forward_refuses_half_table_and_out_slots_on_clipped_columns():
  lib = _lib.lib()
  runs = dict(n_runs=1, run_start=FAKE, run_base=FAKE2, half_io=2)   # HBK_LOOKUP_TABLE_HALF
  cols = (_lib.LookupColumn * 2)(_fwd_col(), _fwd_col(**runs))
  _refused(lib.hbk_group_lookup_fwd_clipped(2, cols, _norms(0.0, 2.0), None), 'column 1',
           'HBK_LOOKUP_TABLE_HALF')
  cols = (_lib.LookupColumn * 1)(_fwd_col(out_slots=FAKE2))
  _refused(lib.hbk_group_lookup_fwd_clipped(1, cols, _norms(2.0), None), 'out_slots')


@pytest.mark.parametrize('bad', [-0.5, float('nan'), float('inf')])
def test_backward_entries_refuse_bad_max_norms(bad):
  lib = _lib.lib()
  cols = (_lib.LookupGradColumn * 2)(_grad_col(), _grad_col(table=FAKE2))
  ws = C.c_void_p(FAKE)
  _refused(lib.hbk_group_lookup_bwd_apply_clipped(2, cols, _norms(bad, 1.0), _lib.APPLY_SGD,
                                                  C.c_float(0.1), ws, C.c_size_t(1 << 30), None),
           'column 0', 'max_norm')
  ptrs = _lib.ptr_array([FAKE + 4096, FAKE2 + 4096])
  ptrs2 = _lib.ptr_array([FAKE + 8192, FAKE2 + 8192])
  adam = _lib.AdamParams(C.c_float(0.9), C.c_float(0.999), C.c_float(1e-8), FAKE, 1)
  _refused(lib.hbk_group_lookup_bwd_adam_clipped(2, cols, _norms(1.0, bad), ptrs, ptrs2, C.byref(adam),
                                                 C.c_float(0.1), ws, C.c_size_t(1 << 30), None),
           'column 1', 'max_norm')
  ftrl = _lib.FtrlParams(C.c_float(0.0), C.c_float(0.0), C.c_float(0.0), C.c_float(-0.5))
  _refused(lib.hbk_group_lookup_bwd_ftrl_clipped(2, cols, _norms(bad, 0.0), ptrs, ptrs2, C.byref(ftrl),
                                                 C.c_float(0.1), ws, C.c_size_t(1 << 30), None),
           'column 0', 'max_norm')


@pytest.mark.parametrize('apply', [_lib.APPLY_SGD, _lib.APPLY_ADAGRAD])
def test_stepping_call_refuses_a_clipped_table_named_twice(apply):
  lib = _lib.lib()
  acc = FAKE + (1 << 20) if apply == _lib.APPLY_ADAGRAD else None
  acc2 = FAKE2 + (1 << 20) if apply == _lib.APPLY_ADAGRAD else None
  # the same table in a clipped and an unclipped column
  cols = (_lib.LookupGradColumn * 2)(_grad_col(accum=acc), _grad_col(accum=acc2))
  rc = lib.hbk_group_lookup_bwd_apply_clipped(2, cols, _norms(1.0, 0.0), apply, C.c_float(0.1),
                                              C.c_void_p(FAKE), C.c_size_t(1 << 30), None)
  _refused(rc, 'share a table', 'clipped')
  # another column stepping the clipped column's table as its accumulator
  if apply == _lib.APPLY_ADAGRAD:
    cols = (_lib.LookupGradColumn * 2)(_grad_col(accum=acc), _grad_col(table=FAKE2, accum=FAKE))
    rc = lib.hbk_group_lookup_bwd_apply_clipped(2, cols, _norms(1.0, 0.0), apply, C.c_float(0.1),
                                                C.c_void_p(FAKE), C.c_size_t(1 << 30), None)
    _refused(rc, 'share a table')


def test_clipped_column_needs_its_table_and_the_workspace():
  lib = _lib.lib()
  cols = (_lib.LookupGradColumn * 1)(_grad_col(table=None))
  rc = lib.hbk_group_lookup_bwd_apply_clipped(1, cols, _norms(1.0), _lib.APPLY_SGD, C.c_float(0.0),
                                              C.c_void_p(FAKE), C.c_size_t(1 << 30), None)
  _refused(rc, 'table is NULL')
  cols = (_lib.LookupGradColumn * 1)(_grad_col())
  need = lib.hbk_group_lookup_bwd_apply_clipped_workspace_bytes(1, cols, _norms(1.0))
  assert need > 0
  rc = lib.hbk_group_lookup_bwd_apply_clipped(1, cols, _norms(1.0), _lib.APPLY_SGD, C.c_float(0.0),
                                              C.c_void_p(FAKE), C.c_size_t(need - 1), None)
  _refused(rc, 'workspace too small')


def test_workspace_queries():
  lib = _lib.lib()
  cols = (_lib.LookupGradColumn * 2)(_grad_col(), _grad_col(table=FAKE2))
  plain = lib.hbk_group_lookup_bwd_workspace_bytes(2, cols)
  # no column clipped: the unclipped query
  assert lib.hbk_group_lookup_bwd_apply_clipped_workspace_bytes(2, cols, _norms(0.0, 0.0)) == plain
  # one clipped: the plain column's reduce plus the clipped column's emit form
  assert lib.hbk_group_lookup_bwd_apply_clipped_workspace_bytes(2, cols, _norms(0.0, 3.0)) > 0
  assert (lib.hbk_group_lookup_bwd_adam_clipped_workspace_bytes(2, cols, _norms(0.0, 3.0)) ==
          lib.hbk_group_lookup_bwd_adam_workspace_bytes(2, cols))
  assert (lib.hbk_group_lookup_bwd_ftrl_clipped_workspace_bytes(2, cols, _norms(1.0, 3.0)) ==
          lib.hbk_group_lookup_bwd_ftrl_workspace_bytes(2, cols))


def test_python_max_norm_list():
  assert _lookup.max_norm_list(None, 3) == [0.0, 0.0, 0.0]
  assert _lookup.max_norm_list(2, 2) == [2.0, 2.0]
  assert _lookup.max_norm_list([None, 0.5], 2) == [0.0, 0.5]
  for bad in (0, 0.0, -1.0, float('nan'), float('inf'), 1e-50, 1e39, True, '1'):
    with pytest.raises(_lib.InvalidArgumentError):
      _lookup.max_norm_list([1.0, bad], 2)
  with pytest.raises(_lib.InvalidArgumentError):
    _lookup.max_norm_list([1.0], 2)
  assert math.isfinite(_lookup.max_norm_list([3.4e38], 1)[0])


def test_python_max_norm_list_takes_numpy_scalars():
  import numpy as np
  assert _lookup.max_norm_list(np.float32(0.5), 2) == [0.5, 0.5]
  assert _lookup.max_norm_list([np.float64(2.0), None], 2) == [2.0, 0.0]
  for bad in (np.float32(0.0), np.float32('nan'), np.bool_(True), [np.bool_(True)], object()):
    with pytest.raises(_lib.InvalidArgumentError):
      _lookup.max_norm_list(bad, 1)


def test_sharded_setter_refuses_bad_values():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_sharded_set_max_norms')
  _refused(lib.hbk_sharded_set_max_norms(None, _norms(1.0)), 'plan is NULL')
