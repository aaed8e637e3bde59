"""Row-wise Adagrad at the C ABI and in Python, without a GPU: the new symbols are declared in the header,
exported by the library and bound by the ctypes layer; every refused combination is refused before any
device work with the field named; the workspace query is Lazy Adam's; the class refuses what the issue
lists; the numpy restatement sums in the documented order."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hybridbackend_amd import _lib
from tests.support import rowwise_adagrad_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it
A, T2, A2 = (FAKE + k * 0x100000 for k in range(1, 4))
INF, NAN = float('inf'), float('nan')
NEW = ('hbk_group_lookup_bwd_rowwise_adagrad_workspace_bytes', 'hbk_group_lookup_bwd_rowwise_adagrad',
       'hbk_group_lookup_bwd_rowwise_adagrad_clipped_workspace_bytes',
       'hbk_group_lookup_bwd_rowwise_adagrad_clipped', 'hbk_sharded_set_rowwise_adagrad_slots',
       'hbk_sharded_lookup_bwd_rowwise_adagrad')


def test_new_symbols_declared_exported_and_bound():
  lib = _lib.lib()
  declared = set(re.findall(r'\b(hbk_\w*rowwise_adagrad\w*)\s*\(', HEADER))
  out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True)
  exported = {name for name in (line.split()[-1] for line in out.stdout.splitlines())
              if name.startswith('hbk_') and 'rowwise_adagrad' in name}
  assert declared == set(NEW) == exported
  for name in NEW:
    assert getattr(lib, name).argtypes is not None, name
  assert 'hbk_rowwise_adagrad_t' in HEADER
  assert [f[0] for f in _lib.RowwiseAdagradParams._fields_] == ['epsilon']
  assert C.sizeof(_lib.RowwiseAdagradParams) == 4
  # the structs the other entries share did not move
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


def _call(cols, acc, eps=1e-8, lr=0.1, clip=None, ws=FAKE, ws_bytes=1 << 40):
  lib = _lib.lib()
  n = len(cols)
  arr = (_lib.LookupGradColumn * n)(*cols)
  p = _lib.RowwiseAdagradParams(eps)
  tail = (_lib.ptr_array(acc), C.byref(p), C.c_float(lr), C.c_void_p(ws), C.c_size_t(ws_bytes), None)
  if clip is not None:
    return lib.hbk_group_lookup_bwd_rowwise_adagrad_clipped(n, arr, (C.c_float * n)(*clip), *tail)
  return lib.hbk_group_lookup_bwd_rowwise_adagrad(n, arr, *tail)


def _refused(rc, *words):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in words:
    assert w in msg, msg


@pytest.mark.parametrize('clipped', [False, True])
@pytest.mark.parametrize('case', [
  'accum_null', 'accum_misaligned', 'accum_is_table', 'col_accum', 'same_table', 'same_accum',
  'accum_is_other_table', 'dim_vec4_too_wide', 'dim_scalar_too_wide', 'lr_zero', 'lr_inf', 'lr_nan',
  'eps_neg', 'eps_inf', 'eps_nan'])
def test_refusals(case, clipped):
  cols, acc, eps, lr, words = [_col()], [A], 1e-8, 0.1, ()
  if case == 'accum_null':
    acc, words = [None], ('accum is NULL',)
  elif case == 'accum_misaligned':
    acc, words = [A + 2], ('4-byte aligned',)
  elif case == 'accum_is_table':
    acc, words = [FAKE], ('accum is the table',)
  elif case == 'col_accum':
    cols, words = [_col(accum=FAKE + 0x800000)], ('accum must be NULL',)
  elif case == 'same_table':
    cols, acc, words = [_col(), _col()], [A, A2], ('same table or accum',)
  elif case == 'same_accum':
    cols, acc, words = [_col(), _col(table=T2)], [A, A], ('same table or accum',)
  elif case == 'accum_is_other_table':
    cols, acc, words = [_col(), _col(table=T2)], [T2, A2], ('same table or accum',)
  elif case == 'dim_vec4_too_wide':
    cols, words = [_col(dim=260)], ('64 lanes',)
  elif case == 'dim_scalar_too_wide':
    cols, words = [_col(dim=66)], ('64 lanes',)
  elif case.startswith('lr_'):
    lr, words = {'lr_zero': 0.0, 'lr_inf': INF, 'lr_nan': NAN}[case], ('lr must',)
  elif case.startswith('eps_'):
    eps, words = {'eps_neg': -1e-9, 'eps_inf': INF, 'eps_nan': NAN}[case], ('epsilon must',)
  _refused(_call(cols, acc, eps, lr, clip=[1.0] * len(cols) if clipped else None), *words)


def test_refused_max_norms_and_missing_arguments():
  lib = _lib.lib()
  for bad in (-1.0, INF, NAN):
    _refused(_call([_col()], [A], clip=[bad]), 'max_norm')
  arr = (_lib.LookupGradColumn * 1)(_col())
  p = _lib.RowwiseAdagradParams(1e-8)
  _refused(lib.hbk_group_lookup_bwd_rowwise_adagrad(1, arr, None, C.byref(p), C.c_float(0.1), C.c_void_p(FAKE),
                                                    C.c_size_t(1 << 40), None), 'accum array is NULL')
  _refused(lib.hbk_group_lookup_bwd_rowwise_adagrad(1, arr, _lib.ptr_array([A]), None, C.c_float(0.1),
                                                    C.c_void_p(FAKE), C.c_size_t(1 << 40), None), 'rowwise_adagrad is NULL')
  _refused(lib.hbk_group_lookup_bwd_rowwise_adagrad(-1, arr, _lib.ptr_array([A]), C.byref(p), C.c_float(0.1),
                                                    C.c_void_p(FAKE), C.c_size_t(1 << 40), None), 'n_cols')


def test_the_accumulator_does_not_decide_the_row_shape():
  """dim 256 on a 16-byte aligned table passes the row-shape check whatever the accumulator's alignment (a
  4-byte-aligned accumulator in the alignment bits would send it to the scalar path, where 256 is refused);
  dim 63 passes on the scalar path.  Both calls stop at the workspace check: nothing here is a device buffer."""
  for dim, acc in ((256, A + 4), (256, A), (63, A + 12)):
    _refused(_call([_col(dim=dim)], [acc], ws=None, ws_bytes=0), 'workspace too small')
  _refused(_call([_col(dim=256, table=FAKE + 4)], [A], ws=None, ws_bytes=0), '64 lanes')


def test_sharded_refusals_without_a_plan():
  lib = _lib.lib()
  p = _lib.RowwiseAdagradParams(1e-8)
  _refused(lib.hbk_sharded_set_rowwise_adagrad_slots(None, _lib.ptr_array([A])), 'plan')
  _refused(lib.hbk_sharded_lookup_bwd_rowwise_adagrad(None, None, None, C.byref(p), C.c_float(0.1), None, None, None,
                                                      None), 'plan')


@pytest.mark.parametrize('step_only', [False, True])
def test_workspace_query_matches_adam(step_only):
  lib = _lib.lib()
  cols = [_col(rows=1000, dim=12, n_ids=777, n_segments=300, row_splits=FAKE, combiner=_lib.COMBINER_MEAN),
          _col(table=T2, rows=5000, dim=64, n_ids=4096, n_segments=4096)]
  if step_only:
    for c in cols:
      c.unique_rows, c.grad_rows = None, None
  arr = (_lib.LookupGradColumn * 2)(*cols)
  need = lib.hbk_group_lookup_bwd_rowwise_adagrad_workspace_bytes(2, arr)
  assert need == lib.hbk_group_lookup_bwd_adam_workspace_bytes(2, arr)
  assert need == lib.hbk_group_lookup_bwd_rowwise_adagrad_clipped_workspace_bytes(2, arr, (C.c_float * 2)(1.0, 0.0))
  assert need >= lib.hbk_group_lookup_bwd_workspace_bytes(2, arr) > 0
  if step_only:
    assert need >= 777 * 8 + 777 * 12 * 4 + 4096 * 8 + 4096 * 64 * 4
  assert lib.hbk_group_lookup_bwd_rowwise_adagrad_workspace_bytes(0, None) == 0


@pytest.mark.parametrize('kw, word', [
  ({'epsilon': -1e-9}, 'epsilon'), ({'epsilon': INF}, 'epsilon'), ({'epsilon': NAN}, 'epsilon'),
  ({'initial_accumulator_value': -0.1}, 'initial_accumulator_value'),
  ({'initial_accumulator_value': INF}, 'initial_accumulator_value'),
  ({'initial_accumulator_value': NAN}, 'initial_accumulator_value'),
  ({'epsilon': 0.0, 'initial_accumulator_value': 0.0}, 'both')])
def test_python_class_refusals(kw, word):
  from hybridbackend_amd.embedding import RowwiseAdagrad
  with pytest.raises(_lib.InvalidArgumentError, match=word):
    RowwiseAdagrad(**kw)


def test_python_class_defaults_and_registry():
  import torch
  from hybridbackend_amd.embedding import RowwiseAdagrad, optimizer as _opt
  r = RowwiseAdagrad()
  assert (r.epsilon, r.initial_accumulator_value) == (1e-8, 0.0)
  assert (r.name, r.slot_kw, r.tf_suffixes) == ('rowwise_adagrad', 'row_accums', ('/RowwiseAdagrad',))
  assert r.params().epsilon == pytest.approx(1e-8)
  RowwiseAdagrad(epsilon=0.0, initial_accumulator_value=0.1)   # one of the two may be 0
  RowwiseAdagrad(epsilon=1e-8, initial_accumulator_value=0.0)
  a = RowwiseAdagrad(initial_accumulator_value=0.25).slots_like(torch.zeros(7, 5))
  assert tuple(a.shape) == (7, 1) and a.dtype == torch.float32 and float(a.min()) == float(a.max()) == 0.25
  assert list(_opt.TWO_SLOT) == ['adam', 'ftrl', 'rowwise_adagrad']
  assert _opt.two_slot_class('rowwise_adagrad') is RowwiseAdagrad
  assert _opt.two_slot_class('sgd') is None and _opt.two_slot_class('adagrad') is None


def test_python_optimizer_refusals_without_a_gpu():
  from hybridbackend_amd.embedding import GroupLookupGrad
  grad = GroupLookupGrad.__new__(GroupLookupGrad)
  grad.moments = grad.ftrl_slots = grad.row_accums = None
  with pytest.raises(_lib.InvalidArgumentError, match=r'row_accums=\[accum, \.\.\.\]'):
    grad([], [], apply_lr=0.1, optimizer='rowwise_adagrad')
  with pytest.raises(_lib.InvalidArgumentError, match="'rowwise_adagrad'"):
    grad([], [], apply_lr=0.1, optimizer='rmsprop')
  # the texts of the four existing optimizers stay as they were
  with pytest.raises(_lib.InvalidArgumentError, match=r'GroupLookupGrad\(lookup, moments=\[\(m, v\), \.\.\.\]\)'):
    grad([], [], apply_lr=0.1, optimizer='adam')
  with pytest.raises(_lib.InvalidArgumentError, match=r'ftrl_slots=\[\(accum, linear\), \.\.\.\]'):
    grad([], [], apply_lr=0.1, optimizer='ftrl')


def test_slot_checks_without_a_gpu():
  """require_slot_pairs on one-slot entries: the count, the [rows, 1] shape, distinct buffers -- checked after
  the device check, so with CPU tensors only the device refusal can be reached; the shape rule is the class's."""
  import torch
  from hybridbackend_amd.embedding import RowwiseAdagrad
  t = torch.zeros(6, 4)
  assert RowwiseAdagrad.slot_shape(t) == (6, 1)
  assert RowwiseAdagrad.slot_tensors(t) == (t,)
  with pytest.raises(_lib.InvalidArgumentError, match='2 accum tensors for 1 tables'):
    _lib.require_slot_pairs([t, t], [t], 'X', 'row_accums', ('accum',), RowwiseAdagrad.slot_shape)
  with pytest.raises(_lib.HbkError, match='must live in HBM'):
    _lib.require_slot_pairs([torch.zeros(6, 1)], [t], 'X', 'row_accums', ('accum',), RowwiseAdagrad.slot_shape)


def test_dense_features_variable_names_and_slot_kinds():
  import types
  import torch
  import hybridbackend_amd as hb
  from hybridbackend_amd.embedding import RowwiseAdagrad
  from hybridbackend_amd.embedding.sharded_hash import slot_kinds
  from hybridbackend_amd.training.saver import ShardedSlice
  cols = [hb.feature_column.EmbeddingColumn('a', 100, 4, 'sum'), hb.feature_column.EmbeddingColumn('b', 8, 2, 'mean')]
  with pytest.raises(_lib.InvalidArgumentError, match="'rowwise_adagrad'"):
    hb.feature_column.DenseFeatures(cols, 'cpu', optimizer='rmsprop')
  layer = hb.feature_column.DenseFeatures.__new__(hb.feature_column.DenseFeatures)
  layer.moments = layer.ftrl_slots = layer.row_accums = None
  with pytest.raises(_lib.InvalidArgumentError, match="optimizer='rowwise_adagrad'"):
    layer.backward(None, apply_lr=0.1, optimizer='rowwise_adagrad')
  layer.columns, layer.sharded = cols, [True, False]
  layer.coll = types.SimpleNamespace(world_size=2, rank=0)
  layer.weights = [torch.zeros(50, 4), torch.zeros(8, 2)]
  layer.accums = layer.adam = layer.ftrl = None
  layer.rowwise_adagrad = RowwiseAdagrad(initial_accumulator_value=0.25)
  layer.row_accums = [layer.rowwise_adagrad.slots_like(w) for w in layer.weights]
  v = layer.variables()
  assert sorted(v) == ['a_embedding/embedding_weights', 'a_embedding/embedding_weights/RowwiseAdagrad',
                       'b_embedding/embedding_weights', 'b_embedding/embedding_weights/RowwiseAdagrad']
  assert isinstance(v['a_embedding/embedding_weights/RowwiseAdagrad'], ShardedSlice)
  assert v['b_embedding/embedding_weights/RowwiseAdagrad'] is layer.row_accums[1]
  assert slot_kinds(layer, 0.0) == [('row_accums', None, 0.25)]
  # the one order: accums; m, v; accum, linear; row_accums
  layer.accums, layer.moments = [None], [None]
  layer.ftrl_slots, layer.ftrl = [None], hb.embedding.Ftrl(initial_accumulator_value=0.5)
  assert slot_kinds(layer, 0.1) == [('accums', None, 0.1), ('moments', 0, 0.0), ('moments', 1, 0.0),
                                    ('ftrl_slots', 0, 0.5), ('ftrl_slots', 1, 0.0), ('row_accums', None, 0.25)]


@pytest.mark.parametrize('dim, vec4', [(1, False), (3, False), (4, False), (4, True), (20, False), (20, True),
                                       (64, True), (256, True)])
def test_restatement_sums_in_the_documented_order(dim, vec4):
  """row_sum_sq against a lane-by-lane scalar walk of the same order, and -- on a grid where every order is
  exact -- against float64."""
  rng = np.random.RandomState(dim + vec4)
  g = rng.randn(5, dim).astype(np.float32)
  got = ref.row_sum_sq(g, vec4)
  W = 4 if vec4 else 1
  chunks = dim // W
  lanes = 1 << max(0, int(np.ceil(np.log2(chunks))))
  for r in range(g.shape[0]):
    p = [np.float32(0)] * lanes
    for i in range(chunks):
      acc = np.float32(g[r, i * W] * g[r, i * W])
      for k in range(1, W):
        acc = np.float32(acc + np.float32(g[r, i * W + k] * g[r, i * W + k]))
      p[i] = acc
    o = 1
    while o < lanes:
      p = [np.float32(p[i] + p[i ^ o]) for i in range(lanes)]
      o *= 2
    assert len({x.tobytes() for x in p}) == 1   # every lane ends with the same bits
    assert got[r].tobytes() == p[0].tobytes()
  exact = (rng.randint(-15, 16, size=(5, dim)) / 4.0).astype(np.float32)
  np.testing.assert_array_equal(ref.row_sum_sq(exact, vec4).astype(np.float64),
                                (exact.astype(np.float64) ** 2).sum(axis=1))
