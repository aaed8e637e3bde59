"""Aggregated replicated gradients at the C ABI and in Python, without a GPU: the three new symbols are declared
in the header, exported by the library and bound by the ctypes layer; every refusal precedes any device work
(the addresses here are no device buffers); the numpy restatement agrees with a float64 dense scatter-add."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hybridbackend_amd import _lib
from tests.support import exact
from tests.support import replica_grads_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it
T2, S0, S1, S2, S3 = (FAKE + k * 0x100000 for k in range(1, 6))
BUCKET = FAKE + 0x4000000
INF, NAN = float('inf'), float('nan')
NEW = ('hbk_sparse_apply_slices_n', 'hbk_replica_grads_pack_n', 'hbk_replica_grads_rows_n')
SGD, ADAGRAD, ADAM, FTRL, ROWWISE = (_lib.APPLY_SGD, _lib.APPLY_ADAGRAD, _lib.APPLY_LAZY_ADAM, _lib.APPLY_FTRL,
                                     _lib.APPLY_ROWWISE_ADAGRAD)


def test_new_symbols_declared_exported_and_bound():
  lib = _lib.lib()
  out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True)
  exported = {line.split()[-1] for line in out.stdout.splitlines()}
  for name in NEW:
    assert re.search(r'\b' + name + r'\s*\(', HEADER), name
    assert name in exported, name
    assert getattr(lib, name).argtypes is not None, name
  assert 'hbk_slices_column_t' in HEADER and 'hbk_replica_column_t' in HEADER
  assert (C.sizeof(_lib.SlicesColumn), C.sizeof(_lib.ReplicaColumn)) == (56, 72)
  assert (ADAM, FTRL, ROWWISE) == tuple(int(re.search(r'#define HBK_APPLY_' + k + r' (\d+)', HEADER).group(1))
                                       for k in ('LAZY_ADAM', 'FTRL', 'ROWWISE_ADAGRAD'))
  # the structs and the version the other entries share did not move
  assert C.sizeof(_lib.LookupGradColumn) == 160 and C.sizeof(_lib.AdamParams) == 32
  assert '0.2.0' in lib.hbk_version().decode()


def _refused(rc, *words):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in words:
    assert w in msg, msg


# ---- hbk_sparse_apply_slices_n ---------------------------------------------------------------------------
def _scol(**kw):
  col = _lib.SlicesColumn()
  col.table, col.rows, col.dim = FAKE, 100, 16
  col.unique_rows, col.grad_rows, col.n_unique, col.capacity = FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, 8
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _apply(cols, apply, s0=None, s1=None, params=None, lr=0.1):
  n = len(cols)
  arr = (_lib.SlicesColumn * n)(*cols)
  return _lib.lib().hbk_sparse_apply_slices_n(
    n, arr, apply, None if s0 is None else _lib.ptr_array(s0), None if s1 is None else _lib.ptr_array(s1),
    None if params is None else C.byref(params), C.c_float(lr), None)


def _adam(**kw):
  p = dict(beta1=0.9, beta2=0.999, epsilon=1e-8, beta_powers=FAKE + 0x9000, finish=1)
  p.update(kw)
  return _lib.AdamParams(p['beta1'], p['beta2'], p['epsilon'], p['beta_powers'], p['finish'])


RULES = {
  SGD: lambda n: dict(),
  ADAGRAD: lambda n: dict(s0=[S0 + 0x10000 * c for c in range(n)]),
  ADAM: lambda n: dict(s0=[S0 + 0x10000 * c for c in range(n)], s1=[S1 + 0x10000 * c for c in range(n)],
                       params=_adam()),
  FTRL: lambda n: dict(s0=[S0 + 0x10000 * c for c in range(n)], s1=[S1 + 0x10000 * c for c in range(n)],
                       params=_lib.FtrlParams(0.0, 0.0, 0.0, -0.5)),
  ROWWISE: lambda n: dict(s0=[S0 + 0x10000 * c for c in range(n)], params=_lib.RowwiseAdagradParams(1e-8)),
}


COMMON = ['dim_vec4_too_wide', 'dim_scalar_too_wide', 'dim_unaligned_too_wide', 'dim_zero', 'same_table',
          'table_null', 'urows_null', 'grows_null', 'nu_null', 'capacity_neg', 'capacity_big', 'pitch_small', 'lr_zero',
          'lr_nan', 'lr_inf']
# (Lazy Adam takes any lr but 0, as hbk_group_lookup_bwd_adam does)
CASES = [(a, k) for a in sorted(RULES) for k in COMMON if not (a == ADAM and k in ('lr_nan', 'lr_inf'))]


@pytest.mark.parametrize('apply, case', CASES)
def test_apply_refusals_common_to_every_rule(apply, case):
  cols, lr, words = [_scol()], 0.1, ()
  if case == 'dim_vec4_too_wide':
    cols, words = [_scol(dim=260)], ('64 lanes',)
  elif case == 'dim_scalar_too_wide':
    cols, words = [_scol(dim=65)], ('64 lanes',)
  elif case == 'dim_unaligned_too_wide':
    cols, words = [_scol(dim=128, grad_rows=FAKE + 0x2004)], ('64 lanes',)
  elif case == 'dim_zero':
    cols, words = [_scol(dim=0)], ('dim must be >= 1',)
  elif case == 'same_table':
    cols, words = [_scol(), _scol()], ('same table',)
  elif case == 'table_null':
    cols, words = [_scol(table=None)], ('table',)
  elif case == 'urows_null':
    cols, words = [_scol(unique_rows=None)], ('unique_rows',)
  elif case == 'grows_null':
    cols, words = [_scol(grad_rows=None)], ('grad_rows',)
  elif case == 'nu_null':
    cols, words = [_scol(n_unique=None)], ('n_unique',)
  elif case == 'capacity_neg':
    cols, words = [_scol(capacity=-1)], ('capacity',)
  elif case == 'capacity_big':
    cols, words = [_scol(capacity=1 << 30)], ('capacity',)
  elif case == 'pitch_small':
    cols, words = [_scol(table_pitch=8)], ('table_pitch',)
  else:
    lr, words = {'lr_zero': 0.0, 'lr_nan': NAN, 'lr_inf': INF}[case], ('lr must',)
  _refused(_apply(cols, apply, lr=lr, **RULES[apply](len(cols))), *words)


def test_apply_refusals_of_the_slots_and_hyperparameters():
  one = [_scol()]
  _refused(_apply(one, 1), 'apply must be')
  _refused(_apply(one, 6), 'apply must be')
  _refused(_apply(one, ADAGRAD), 'slot0')
  _refused(_apply(one, ADAGRAD, s0=[None]), 'accumulator is NULL')
  _refused(_apply(one, ADAGRAD, s0=[FAKE]), 'accumulator is the table')
  _refused(_apply([_scol(), _scol(table=T2)], ADAGRAD, s0=[S0, S0]), 'same table or accumulator')
  _refused(_apply([_scol(), _scol(table=T2)], ADAGRAD, s0=[T2, S0]), 'same table or accumulator')
  two = dict(s0=[S0], s1=[S1])
  _refused(_apply(one, ADAM, **two), 'adam is NULL')
  _refused(_apply(one, ADAM, params=_adam(beta1=1.0), **two), 'beta1')
  _refused(_apply(one, ADAM, params=_adam(beta_powers=None), **two), 'beta_powers')
  _refused(_apply(one, ADAM, params=_adam(), s0=[S0], s1=[S0]), 'same buffer')
  _refused(_apply(one, ADAM, params=_adam(), s0=[S0], s1=[None]), 'v is NULL')
  _refused(_apply(one, ADAM, params=_adam(), s0=[S0]), 'arrays are NULL')
  _refused(_apply([_scol(), _scol(table=T2)], ADAM, params=_adam(), s0=[S0, S2], s1=[S1, S0]), 'same table, m or v')
  _refused(_apply(one, FTRL, **two), 'ftrl is NULL')
  _refused(_apply(one, FTRL, params=_lib.FtrlParams(-1.0, 0.0, 0.0, -0.5), **two), 'l1')
  _refused(_apply(one, FTRL, params=_lib.FtrlParams(0.0, 0.0, 0.0, 0.5), **two), 'lr_power')
  _refused(_apply(one, FTRL, params=_lib.FtrlParams(0.0, 0.0, 0.0, -0.5), lr=-0.1, **two), 'lr must')
  _refused(_apply(one, ROWWISE, s0=[S0]), 'rowwise_adagrad is NULL')
  _refused(_apply(one, ROWWISE, s0=[S0], params=_lib.RowwiseAdagradParams(-1.0)), 'epsilon')
  _refused(_apply(one, ROWWISE, s0=[S0 + 2], params=_lib.RowwiseAdagradParams(1e-8)), '4-byte aligned')
  _refused(_lib.lib().hbk_sparse_apply_slices_n(-1, None, SGD, None, None, None, C.c_float(0.1), None), 'n_cols')
  _refused(_lib.lib().hbk_sparse_apply_slices_n(1, None, SGD, None, None, None, C.c_float(0.1), None), 'cols is NULL')


def test_apply_row_shape_follows_the_alignment_of_what_the_rule_reads():
  """dim 256 needs 16-byte lanes: refused when a table-shaped slot is only 4-byte aligned, but row-wise Adagrad's
  one word per row does not decide the row shape.  (The accepted calls would launch: only refusals are made.)"""
  wide = [_scol(dim=256)]
  _refused(_apply(wide, ADAGRAD, s0=[S0 + 4]), '64 lanes')
  _refused(_apply(wide, ADAM, params=_adam(), s0=[S0], s1=[S1 + 8]), '64 lanes')
  _refused(_apply([_scol(dim=256, table=FAKE + 4)], ROWWISE, s0=[S0], params=_lib.RowwiseAdagradParams(1e-8)),
           '64 lanes')
  _refused(_apply([_scol(dim=256, table_pitch=258)], SGD), '64 lanes')


# ---- hbk_replica_grads_pack_n / hbk_replica_grads_rows_n ---------------------------------------------------------------
def _rcol(**kw):
  col = _lib.ReplicaColumn()
  col.unique_rows, col.grad_rows, col.n_unique, col.capacity = FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, 8
  col.rows, col.dim = 10, 4
  col.block, col.touched, col.urows = BUCKET, BUCKET + 40 * 4, FAKE + 0x5000
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _pack(cols, bucket=BUCKET, floats=50):
  n = len(cols)
  return _lib.lib().hbk_replica_grads_pack_n(n, (_lib.ReplicaColumn * n)(*cols), bucket, floats, None)


@pytest.mark.parametrize('kw, call, words', [
  (dict(unique_rows=None), {}, ('unique_rows',)),
  (dict(grad_rows=None), {}, ('grad_rows',)),
  (dict(n_unique=None), {}, ('n_unique',)),
  (dict(block=None), {}, ('block',)),
  (dict(touched=None), {}, ('touched',)),
  (dict(unique_rows=FAKE + 0x1004), {}, ('unique_rows',)),
  ({}, dict(bucket=None), ('bucket',)),
  (dict(dim=65, block=BUCKET, touched=BUCKET + 650 * 4), dict(floats=660), ('64 lanes',)),
  (dict(dim=260, block=BUCKET, touched=BUCKET + 2600 * 4), dict(floats=2610), ('64 lanes',)),
  (dict(dim=128, block=BUCKET + 4, touched=BUCKET + 1284 * 4), dict(floats=1300), ('64 lanes',)),
  (dict(dim=0), {}, ('dim must be >= 1',)),
  (dict(capacity=-1), {}, ('capacity',)),
  (dict(capacity=1 << 30), {}, ('capacity',)),
  (dict(rows=-1), {}, ('rows',)),
  (dict(rows=1 << 31), dict(floats=(1 << 31) - 1), ('rows',)),
  ({}, dict(floats=49), ('too small', 'touched words')),
  ({}, dict(floats=39), ('too small', 'block')),
  (dict(block=BUCKET - 16), {}, ('too small', 'block')),
  ({}, dict(floats=0), ('bucket_floats',)),
  ({}, dict(floats=1 << 31), ('bucket_floats',)),
  (dict(touched=BUCKET + 36 * 4), {}, ('overlap',)),
])
def test_pack_refusals(kw, call, words):
  _refused(_pack([_rcol(**kw)], **call), *words)


def test_pack_and_rows_refusals_over_columns():
  lib = _lib.lib()
  # two tables in one block
  _refused(_pack([_rcol(), _rcol(touched=BUCKET + 50 * 4)], floats=60), 'overlap')
  _refused(lib.hbk_replica_grads_pack_n(-1, None, BUCKET, 50, None), 'n_cols')
  _refused(lib.hbk_replica_grads_pack_n(1, None, BUCKET, 50, None), 'cols is NULL')
  arr = lambda *cols: (_lib.ReplicaColumn * len(cols))(*cols)   # noqa: E731
  _refused(lib.hbk_replica_grads_rows_n(1, arr(_rcol(touched=None)), None), 'touched')
  _refused(lib.hbk_replica_grads_rows_n(1, arr(_rcol(urows=None)), None), 'urows')
  _refused(lib.hbk_replica_grads_rows_n(1, arr(_rcol(urows=FAKE + 0x5004)), None), 'urows')
  _refused(lib.hbk_replica_grads_rows_n(1, arr(_rcol(rows=-1)), None), 'rows')
  _refused(lib.hbk_replica_grads_rows_n(-1, None, None), 'n_cols')
  # nothing to do is no error and touches nothing
  assert lib.hbk_replica_grads_rows_n(0, None, None) == _lib.OK
  assert lib.hbk_replica_grads_rows_n(1, arr(_rcol(rows=0, touched=None, urows=None)), None) == _lib.OK
  assert lib.hbk_sparse_apply_slices_n(0, None, SGD, None, None, None, C.c_float(0.1), None) == _lib.OK


# ---- Python ----------------------------------------------------------------------------------------------------------------
def test_python_refusals_without_a_gpu():
  import torch
  import hybridbackend_amd as hb
  from hybridbackend_amd.embedding import SparseApply
  app = SparseApply.__new__(SparseApply)
  app.moments = app.ftrl_slots = app.row_accums = app.accums = None
  with pytest.raises(_lib.InvalidArgumentError, match=r'SparseApply\(tables, moments=\[\(m, v\), \.\.\.\]\)'):
    app([], 0.1, optimizer='adam')
  with pytest.raises(_lib.InvalidArgumentError, match=r'row_accums=\[accum, \.\.\.\]'):
    app([], 0.1, optimizer='rowwise_adagrad')
  with pytest.raises(_lib.InvalidArgumentError, match="'rowwise_adagrad'"):
    app([], 0.1, optimizer='rmsprop')
  with pytest.raises(_lib.InvalidArgumentError, match='accums='):
    app([], 0.1, optimizer='adagrad')
  with pytest.raises(_lib.InvalidArgumentError, match='lr must be != 0'):
    app([], 0.0)
  with pytest.raises(_lib.HbkError, match='launch'):
    app._bound = None
    app.launch()
  with pytest.raises(_lib.HbkError, match='must live in HBM'):
    SparseApply([torch.zeros(4, 4)])
  RG = hb.distribute.ReplicatedGradients
  for shapes, word in (([(4, 0)], 'dim'), ([(4, 65)], 'beyond'), ([(4, 260)], 'beyond'), ([(-1, 4)], 'rows')):
    with pytest.raises(_lib.InvalidArgumentError, match=word):
      RG(shapes, None, device='cpu')
  for scale in (INF, NAN, 0.0, 0.5):     # (0.5: one rank has no allreduce to apply it)
    with pytest.raises(_lib.InvalidArgumentError, match='scale'):
      RG([(4, 4)], None, scale=scale, device='cpu')
  assert hb.distribute.replica_bucket_layout([(7, 4), (40, 8), (48, 3)]) == ref.layout([(7, 4), (40, 8), (48, 3)])
  assert ref.layout([(3, 3), (2, 5)]) == ([0, 12], [24, 27], 29)


# ---- the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('world, scale', [(1, 1.0), (2, 0.5), (3, 1.0 / 3), (4, 0.25), (3, 1.0), (2, -2.0)])
def test_restatement_agrees_with_a_float64_dense_scatter_add(world, scale):
  """On the exact grid of tests/support/exact.py the fp32 sum over ranks is exact in any order: pack + reduce must
  EQUAL float64(scatter-add of every rank's slices) * float64(fp32(scale)) rounded once -- and the holes, the
  stale tail and the out-of-range entries must reach neither the blocks nor the touched words."""
  rng = np.random.RandomState(world * 10 + 1)
  shapes = [(7, 4), (40, 8), (48, 3), (1, 1)]
  lay = ref.layout(shapes)
  per_rank, dense, touched = [], [np.zeros(s, np.float64) for s in shapes], [np.zeros(s[0], bool) for s in shapes]
  for _ in range(world):
    slices = []
    for c, (rows, dim) in enumerate(shapes):
      cap = rows + 5
      k = int(rng.randint(0, rows + 1))
      urows = np.full(cap, -1, np.int64)
      urows[:k] = rng.permutation(rows)[:k]
      n = k + 2
      urows[k], urows[k + 1] = -1, rows           # inside n_unique, outside the table
      urows[n:] = rng.randint(0, rows, size=cap - n)   # a stale tail of valid-looking rows
      g = exact.exact_grads(rng, (cap, dim), 8)
      g[n:] = np.nan
      slices.append((urows, g, n))
      dense[c][urows[:k]] += g[:k].astype(np.float64)
      touched[c][urows[:k]] = True
    per_rank.append(slices)
  bucket = ref.reduce([ref.pack(shapes, s, lay, fill=np.nan) for s in per_rank], scale)
  assert np.isfinite(bucket).all()
  for c, (urows, block) in enumerate(ref.unpack(shapes, bucket, lay)):
    want = (dense[c] * np.float64(np.float32(scale))).astype(np.float32)
    exact.assert_bits_equal(block, want, f'table {c}')
    np.testing.assert_array_equal(urows, np.where(touched[c], np.arange(shapes[c][0]), -1))
    assert (block[~touched[c]] == 0).all()
