"""FTRL-Proximal at the C ABI and in Python, without a GPU: the new symbols exist, every refused
combination is refused before any device work with the field named, the workspace query is Lazy
Adam's, and the Python layers refuse what TF's FtrlOptimizer refuses and name the slots as TF does."""
import ctypes as C

import pytest

from hybridbackend_amd import _lib

FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it
A, Z, T2, A2, Z2 = (FAKE + k * 0x100000 for k in range(1, 6))
INF, NAN = float('inf'), float('nan')


def test_new_symbols_and_unchanged_abi():
  lib = _lib.lib()
  for name in ('hbk_group_lookup_bwd_ftrl_workspace_bytes', 'hbk_group_lookup_bwd_ftrl',
               'hbk_sharded_set_ftrl_slots', 'hbk_sharded_lookup_bwd_ftrl'):
    assert hasattr(lib, name), name
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  assert [f[0] for f in _lib.FtrlParams._fields_] == ['l1', 'l2', 'l2_shrinkage', 'lr_power']
  assert C.sizeof(_lib.FtrlParams) == 16
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


def _ftrl(**kw):
  f = _lib.FtrlParams(2.0, 1e-5, 0.0, -0.5)
  for k, v in kw.items():
    setattr(f, k, v)
  return f


def _call(cols, acc, lin, ftrl=None, lr=0.1):
  lib = _lib.lib()
  n = len(cols)
  arr = (_lib.LookupGradColumn * n)(*cols)
  return lib.hbk_group_lookup_bwd_ftrl(n, arr, _lib.ptr_array(acc), _lib.ptr_array(lin),
                                       C.byref(ftrl if ftrl is not None else _ftrl()), C.c_float(lr),
                                       C.c_void_p(FAKE), C.c_size_t(1 << 40), None)


def _refused(rc, *words):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in words:
    assert w in msg, msg


@pytest.mark.parametrize('case', [
  'accum_null', 'linear_null', 'accum_is_linear', 'accum_is_table', 'linear_is_table', 'col_accum',
  'lr_zero', 'lr_neg', 'lr_inf', 'lr_nan', 'l1_neg', 'l1_inf', 'l1_nan', 'l2_neg', 'l2_inf', 'l2_nan',
  'shrinkage_neg', 'shrinkage_inf', 'shrinkage_nan', 'lr_power_pos', 'lr_power_inf', 'lr_power_nan',
  'same_table', 'same_slot', 'slot_is_other_table', 'dim_vec4_too_wide', 'dim_scalar_too_wide'])
def test_refusals(case):
  c0, acc, lin, ftrl, lr = _col(), [A], [Z], _ftrl(), 0.1
  cols = [c0]
  words = ()
  if case == 'accum_null':
    acc, words = [None], ('accum is NULL',)
  elif case == 'linear_null':
    lin, words = [None], ('linear is NULL',)
  elif case == 'accum_is_linear':
    lin, words = [A], ('accum and linear',)
  elif case == 'accum_is_table':
    acc, words = [FAKE], ('accum is the table',)
  elif case == 'linear_is_table':
    lin, words = [FAKE], ('linear is the table',)
  elif case == 'col_accum':
    cols, words = [_col(accum=FAKE + 0x800000)], ('accum must be NULL',)
  elif case.startswith('lr_') and not case.startswith('lr_power'):
    lr, words = {'lr_zero': 0.0, 'lr_neg': -0.1, 'lr_inf': INF, 'lr_nan': NAN}[case], ('lr must',)
  elif case.startswith(('l1_', 'l2_', 'shrinkage_', 'lr_power_')):
    field = {'l1': 'l1', 'l2': 'l2', 'shrinkage': 'l2_shrinkage', 'lr': 'lr_power'}[case.split('_')[0]]
    bad = {'neg': -1e-3, 'pos': 0.1, 'inf': INF, 'nan': NAN}[case.split('_')[-1]]
    if field == 'lr_power' and bad == INF:
      bad = -INF
    ftrl, words = _ftrl(**{field: bad}), (f'{field} must',)
  elif case == 'same_table':
    cols, acc, lin, words = [c0, _col()], [A, A2], [Z, Z2], ('same table',)
  elif case == 'same_slot':
    cols, acc, lin, words = [c0, _col(table=T2)], [A, A], [Z, Z2], ('same table, accum or linear',)
  elif case == 'slot_is_other_table':
    cols, acc, lin, words = [c0, _col(table=T2)], [A, A2], [T2, Z2], ('same table, accum or linear',)
  elif case == 'dim_vec4_too_wide':   # 16-byte aligned f32x4 rows: at most 256
    cols, words = [_col(dim=260)], ('64 lanes', 'accum / linear')
  elif case == 'dim_scalar_too_wide':   # dim % 4 != 0: scalar rows, at most 64
    cols, words = [_col(dim=66)], ('64 lanes',)
  _refused(_call(cols, acc, lin, ftrl, lr), *words)


def test_widest_accepted_dims_pass_the_host_checks():
  """dim 256 aligned and dim 63 scalar are not refused by the row-shape check (the call then fails
  later only because nothing here is a device buffer -- so it is stopped at the workspace check)."""
  lib = _lib.lib()
  for dim in (256, 63):
    arr = (_lib.LookupGradColumn * 1)(_col(dim=dim))
    rc = lib.hbk_group_lookup_bwd_ftrl(1, arr, _lib.ptr_array([A]), _lib.ptr_array([Z]),
                                       C.byref(_ftrl()), C.c_float(0.1), None, C.c_size_t(0), None)
    _refused(rc, 'workspace too small')


def test_refusals_without_arrays_or_params():
  lib = _lib.lib()
  arr = (_lib.LookupGradColumn * 1)(_col())
  _refused(lib.hbk_group_lookup_bwd_ftrl(1, arr, None, None, C.byref(_ftrl()), C.c_float(0.1),
                                         C.c_void_p(FAKE), C.c_size_t(1 << 40), None), 'accum / linear')
  _refused(lib.hbk_group_lookup_bwd_ftrl(1, arr, _lib.ptr_array([A]), _lib.ptr_array([Z]), None,
                                         C.c_float(0.1), C.c_void_p(FAKE), C.c_size_t(1 << 40), None),
           'ftrl')


def test_sharded_refusals_without_a_plan():
  lib = _lib.lib()
  _refused(lib.hbk_sharded_set_ftrl_slots(None, _lib.ptr_array([A]), _lib.ptr_array([Z])), 'plan')
  _refused(lib.hbk_sharded_lookup_bwd_ftrl(None, None, None, C.byref(_ftrl()), C.c_float(0.1),
                                           None, None, None, None), 'plan')


@pytest.mark.parametrize('step_only', [False, True])
def test_workspace_query_matches_adam(step_only):
  lib = _lib.lib()
  cols = [_col(rows=1000, dim=12, n_ids=777, n_segments=300, row_splits=FAKE,
               combiner=_lib.COMBINER_MEAN),
          _col(table=T2, rows=5000, dim=64, n_ids=4096, n_segments=4096)]
  if step_only:
    for c in cols:
      c.unique_rows, c.grad_rows = None, None
  arr = (_lib.LookupGradColumn * 2)(*cols)
  ftrl = lib.hbk_group_lookup_bwd_ftrl_workspace_bytes(2, arr)
  assert ftrl == lib.hbk_group_lookup_bwd_adam_workspace_bytes(2, arr)
  assert ftrl >= lib.hbk_group_lookup_bwd_workspace_bytes(2, arr) > 0
  if step_only:
    assert ftrl >= 777 * 8 + 777 * 12 * 4 + 4096 * 8 + 4096 * 64 * 4


@pytest.mark.parametrize('kw, word', [
  ({'l1': -1.0}, 'l1'), ({'l1': INF}, 'l1'), ({'l2': NAN}, 'l2'), ({'l2': -1e-9}, 'l2'),
  ({'l2_shrinkage': -0.1}, 'l2_shrinkage'), ({'l2_shrinkage': INF}, 'l2_shrinkage'),
  ({'lr_power': 0.1}, 'lr_power'), ({'lr_power': NAN}, 'lr_power'), ({'lr_power': -INF}, 'lr_power'),
  ({'initial_accumulator_value': -0.1}, 'initial_accumulator_value')])
def test_python_ftrl_refusals(kw, word):
  from hybridbackend_amd.embedding import Ftrl
  with pytest.raises(_lib.InvalidArgumentError, match=word):
    Ftrl(**kw)


def test_python_ftrl_defaults_are_tfs():
  from hybridbackend_amd.embedding import Ftrl
  f = Ftrl()
  assert (f.l1, f.l2, f.l2_shrinkage, f.lr_power, f.initial_accumulator_value) == (0, 0, 0, -0.5, 0.1)
  p = Ftrl(l1=2.0, l2=1e-5, l2_shrinkage=0.01, lr_power=-0.3).params()
  assert (p.l1, p.lr_power) == (2.0, pytest.approx(-0.3))
  Ftrl(lr_power=0.0, initial_accumulator_value=0.0)   # TF accepts both


def test_python_optimizer_refusals_without_a_gpu():
  from hybridbackend_amd.embedding import GroupLookupGrad
  grad = GroupLookupGrad.__new__(GroupLookupGrad)
  grad.moments = None
  grad.ftrl_slots = None
  with pytest.raises(_lib.InvalidArgumentError, match='ftrl_slots'):
    grad([], [], apply_lr=0.1, optimizer='ftrl')
  with pytest.raises(_lib.InvalidArgumentError, match="'ftrl'"):
    grad([], [], apply_lr=0.1, optimizer='rmsprop')
  grad._bound_call = (True, [])
  with pytest.raises(_lib.InvalidArgumentError, match='ftrl_slots'):
    grad.launch(0.1, optimizer='ftrl')


def test_dense_features_refuses_ftrl_without_slots_and_unknown_optimizers():
  import hybridbackend_amd as hb
  cols = [hb.feature_column.EmbeddingColumn('a', 100, 4, 'sum')]
  with pytest.raises(_lib.InvalidArgumentError, match="'ftrl'"):
    hb.feature_column.DenseFeatures(cols, 'cpu', optimizer='rmsprop')
  layer = hb.feature_column.DenseFeatures.__new__(hb.feature_column.DenseFeatures)
  layer.moments, layer.ftrl_slots = None, None
  with pytest.raises(_lib.InvalidArgumentError, match="optimizer='ftrl'"):
    layer.backward(None, apply_lr=0.1, optimizer='ftrl')


def test_dense_features_ftrl_variable_names_follow_tf():
  """tf.train.FtrlOptimizer's slots: <var>/Ftrl (accum) and <var>/Ftrl_1 (linear), sharded as the
  weights (the layer's variables() without a GPU: its tensors are set by hand)."""
  import torch
  import hybridbackend_amd as hb
  from hybridbackend_amd.embedding import Ftrl
  from hybridbackend_amd.training.saver import ShardedSlice
  cols = [hb.feature_column.EmbeddingColumn('a', 100, 4, 'sum'),
          hb.feature_column.EmbeddingColumn('b', 8, 2, 'mean')]
  layer = hb.feature_column.DenseFeatures.__new__(hb.feature_column.DenseFeatures)
  import types
  layer.columns, layer.sharded = cols, [True, False]
  layer.coll = types.SimpleNamespace(world_size=2, rank=0)   # (rank 0 of 2: 'a' is sharded)
  layer.weights = [torch.zeros(50, 4), torch.zeros(8, 2)]
  layer.accums, layer.moments, layer.adam = None, None, None
  layer.ftrl = Ftrl(initial_accumulator_value=0.25)
  layer.ftrl_slots = [layer.ftrl.slots_like(w) for w in layer.weights]
  v = layer.variables()
  assert sorted(v) == ['a_embedding/embedding_weights', 'a_embedding/embedding_weights/Ftrl',
                       'a_embedding/embedding_weights/Ftrl_1', 'b_embedding/embedding_weights',
                       'b_embedding/embedding_weights/Ftrl', 'b_embedding/embedding_weights/Ftrl_1']
  assert isinstance(v['a_embedding/embedding_weights/Ftrl'], ShardedSlice)
  assert v['b_embedding/embedding_weights/Ftrl'] is layer.ftrl_slots[1][0]
  assert v['b_embedding/embedding_weights/Ftrl_1'] is layer.ftrl_slots[1][1]
  assert float(layer.ftrl_slots[0][0].min()) == float(layer.ftrl_slots[0][0].max()) == 0.25
  assert float(layer.ftrl_slots[0][1].abs().max()) == 0.0
