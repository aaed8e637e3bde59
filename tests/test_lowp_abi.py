"""Low-precision tables at the C ABI and in Python, without a GPU: the two new symbols are declared in the header,
exported by the library and bound by the ctypes layer; every refusal precedes any device work (the addresses here
are no device buffers); the numpy restatement of the rounding agrees with torch's cast on every pattern class."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from hybridbackend_amd import _lib
from tests.support import lowp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it
T2, S0, S1, S2 = (FAKE + k * 0x100000 for k in range(1, 5))
STEP = FAKE + 0x800000
INF, NAN = float('inf'), float('nan')
NEW = ('hbk_lowp_lookup_fwd', 'hbk_lowp_apply_slices_n')
SGD, ADAGRAD, ADAM, FTRL, ROWWISE = (_lib.APPLY_SGD, _lib.APPLY_ADAGRAD, _lib.APPLY_LAZY_ADAM, _lib.APPLY_FTRL,
                                     _lib.APPLY_ROWWISE_ADAGRAD)
BF16, FP16 = _lib.LOWP_BF16, _lib.LOWP_FP16


def test_new_symbols_declared_exported_and_bound():
  lib = _lib.lib()
  out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True)
  exported = {line.split()[-1] for line in out.stdout.splitlines()}
  for name in NEW:
    assert re.search(r'\b' + name + r'\s*\(', HEADER), name
    assert name in exported, name
    assert getattr(lib, name).argtypes is not None, name
  for struct in ('hbk_lowp_lookup_column_t', 'hbk_lowp_slices_column_t', 'hbk_lowp_rounding_t'):
    assert struct in HEADER
  assert (C.sizeof(_lib.LowpLookupColumn), C.sizeof(_lib.LowpSlicesColumn), C.sizeof(_lib.LowpRounding)) == (104, 56, 24)
  codes = {k: int(re.search(r'#define HBK_LOWP_' + k + r' (\d+)', HEADER).group(1))
           for k in ('BF16', 'FP16', 'ROUND_NEAREST', 'ROUND_STOCHASTIC')}
  assert codes == dict(BF16=BF16, FP16=FP16, ROUND_NEAREST=_lib.LOWP_ROUND_NEAREST,
                       ROUND_STOCHASTIC=_lib.LOWP_ROUND_STOCHASTIC)
  # the structs and the version the other entries share did not move
  assert C.sizeof(_lib.LookupColumn) == 128 and C.sizeof(_lib.LookupGradColumn) == 160
  assert C.sizeof(_lib.SlicesColumn) == 56 and C.sizeof(_lib.AdamParams) == 32
  assert '0.2.0' in lib.hbk_version().decode()


def _refused(rc, *words):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in words:
    assert w in msg, msg


# ---- hbk_lowp_lookup_fwd ----------------------------------------------------------------------------------------
def _fcol(**kw):
  col = _lib.LowpLookupColumn()
  col.table, col.table_dtype, col.rows, col.dim = FAKE, BF16, 100, 16
  col.ids, col.ids_dtype, col.n_ids, col.n_segments = FAKE + 0x1000, _lib.INT64, 8, 8
  col.divisor, col.combiner, col.out = 1, _lib.COMBINER_SUM, FAKE + 0x2000
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _fwd(cols):
  n = len(cols)
  return _lib.lib().hbk_lowp_lookup_fwd(n, (_lib.LowpLookupColumn * n)(*cols), None)


@pytest.mark.parametrize('kw, words', [
  (dict(table_dtype=0), ('column 0', 'table_dtype')),
  (dict(table_dtype=3), ('table_dtype',)),
  (dict(table_dtype=_lib.HALF), ('table_dtype',)),
  (dict(dim=0), ('dim must be >= 1',)),
  (dict(dim=65), ('column 0', 'dim 65', '64 otherwise')),
  (dict(dim=257), ('dim 257',)),
  (dict(dim=260), ('dim 260', 'at most 256')),
  (dict(dim=128, table=FAKE + 2), ('dim 128', '64 otherwise')),       # one element per lane holds 64
  (dict(dim=128, out=FAKE + 0x2004), ('dim 128',)),
  (dict(dim=128, out_stride=130), ('dim 128',)),
  (dict(table=FAKE + 1), ('2-byte aligned',)),
  (dict(out=FAKE + 0x2002), ('4-byte aligned',)),
  (dict(table=None), ('table is NULL',)),
  (dict(ids=None), ('ids is NULL',)),
  (dict(out=None), ('out is NULL',)),
  (dict(ids_dtype=_lib.FLOAT), ('int32 or int64',)),
  (dict(combiner=3), ('combiner',)),
  (dict(bucket=-1), ('bucket',)),
  (dict(divisor=0), ('divisor',)),
  (dict(n_segments=7), ('n_segments',)),
  (dict(n_ids=-1, n_segments=-1), ('negative',)),
  (dict(n_ids=1 << 31, n_segments=1 << 31), ('2^31',)),
  (dict(out_stride=8), ('out_stride',)),
  (dict(chunk_elems=16), ('chunk_elems',)),
])
def test_forward_refusals(kw, words):
  _refused(_fwd([_fcol(**kw)]), *words)


def test_forward_refusals_name_the_column_and_nothing_to_do_is_ok():
  lib = _lib.lib()
  _refused(_fwd([_fcol(n_segments=0, n_ids=0), _fcol(dim=260, out=FAKE + 0x9000)]), 'column 1')
  _refused(lib.hbk_lowp_lookup_fwd(-1, None, None), 'n_cols')
  _refused(lib.hbk_lowp_lookup_fwd(1, None, None), 'cols is NULL')
  assert lib.hbk_lowp_lookup_fwd(0, None, None) == _lib.OK
  # a column without segments launches nothing, whatever its buffers
  assert _fwd([_fcol(n_segments=0, n_ids=0, table=None, ids=None, out=None)]) == _lib.OK


# ---- hbk_lowp_apply_slices_n -----------------------------------------------------------------------------------
def _scol(**kw):
  col = _lib.LowpSlicesColumn()
  col.table, col.table_dtype, col.rows, col.dim = FAKE, BF16, 100, 16
  col.unique_rows, col.grad_rows, col.n_unique, col.capacity = FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, 8
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _round(mode=0, seed=0, step=STEP, advance=1):
  return _lib.LowpRounding(mode, seed, step, advance, 0)


def _apply(cols, apply, s0=None, s1=None, params=None, lr=0.1, rounding=None):
  n = len(cols)
  arr = (_lib.LowpSlicesColumn * n)(*cols)
  return _lib.lib().hbk_lowp_apply_slices_n(
    n, arr, apply, None if s0 is None else _lib.ptr_array(s0), None if s1 is None else _lib.ptr_array(s1),
    None if params is None else C.byref(params), C.c_float(lr), None if rounding is None else C.byref(rounding), None)


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

COMMON = ['dtype_zero', 'dtype_three', 'dim_vec4_too_wide', 'dim_257', 'dim_scalar_too_wide', 'dim_unaligned_too_wide',
          'dim_zero', 'same_table', 'table_odd', 'table_null', 'urows_null', 'grows_null', 'nu_null', 'capacity_neg',
          'capacity_big', 'lr_zero', 'round_mode', 'stochastic_fp16', 'stochastic_null_step']
CASES = [(a, k) for a in sorted(RULES) for k in COMMON]


@pytest.mark.parametrize('apply, case', CASES)
def test_apply_refusals_common_to_every_rule(apply, case):
  cols, lr, words, rounding = [_scol()], 0.1, (), None
  if case == 'dtype_zero':
    cols, words = [_scol(table_dtype=0)], ('table_dtype',)
  elif case == 'dtype_three':
    cols, words = [_scol(table_dtype=3)], ('table_dtype',)
  elif case == 'dim_vec4_too_wide':
    cols, words = [_scol(dim=260)], ('dim 260', 'at most 256')
  elif case == 'dim_257':
    cols, words = [_scol(dim=257)], ('dim 257',)
  elif case == 'dim_scalar_too_wide':
    cols, words = [_scol(dim=65)], ('dim 65', '64 otherwise')
  elif case == 'dim_unaligned_too_wide':
    cols, words = [_scol(dim=128, table=FAKE + 4)], ('dim 128',)     # 4-byte aligned: one element per lane
  elif case == 'dim_zero':
    cols, words = [_scol(dim=0)], ('dim must be >= 1',)
  elif case == 'same_table':
    cols, words = [_scol(), _scol()], ('same table',)
  elif case == 'table_odd':
    cols, words = [_scol(table=FAKE + 1)], ('2-byte aligned',)
  elif case == 'table_null':
    cols, words = [_scol(table=None)], ('table is NULL',)
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
  elif case == 'lr_zero':
    lr, words = 0.0, ('lr must',)
  elif case == 'round_mode':
    rounding, words = _round(mode=2), ('rounding mode',)
  elif case == 'stochastic_fp16':
    cols, rounding, words = [_scol(table_dtype=FP16)], _round(mode=1), ('column 0', 'bf16 tables only')
  else:
    rounding, words = _round(mode=1, step=None), ('step counter',)
  kw = RULES[apply](len(cols))
  if case == 'same_table' and 's0' in kw:   # (distinct slots: the table is what is named twice)
    kw = RULES[apply](2)
  _refused(_apply(cols, apply, lr=lr, rounding=rounding, **kw), *words)


def test_apply_refusals_of_the_slots_and_hyperparameters():
  one = [_scol()]
  _refused(_apply(one, 1), 'apply must be')
  _refused(_apply(one, 6), 'apply must be')
  _refused(_apply(one, SGD, lr=NAN), 'lr must')
  _refused(_apply(one, ADAGRAD, lr=INF, s0=[S0]), 'lr must')
  _refused(_apply(one, ADAGRAD), 'slot0')
  _refused(_apply(one, ADAGRAD, s0=[None]), 'accumulator must be')
  _refused(_apply(one, ADAGRAD, s0=[FAKE]), 'same table or slot')
  _refused(_apply([_scol(), _scol(table=T2)], ADAGRAD, s0=[S0, S0]), 'same table or slot')
  two = dict(s0=[S0], s1=[S1])
  _refused(_apply(one, ADAM, **two), 'adam is NULL')
  _refused(_apply(one, ADAM, params=_adam(beta1=1.0), **two), 'beta1')
  _refused(_apply(one, ADAM, params=_adam(beta_powers=None), **two), 'beta_powers')
  _refused(_apply(one, ADAM, params=_adam(), s0=[S0], s1=[S0]), 'same table or slot')
  _refused(_apply(one, ADAM, params=_adam(), s0=[S0], s1=[None]), 'v must be')
  _refused(_apply(one, ADAM, params=_adam(), s0=[S0]), 'slot1')
  _refused(_apply(one, FTRL, **two), 'ftrl is NULL')
  _refused(_apply(one, FTRL, params=_lib.FtrlParams(-1.0, 0.0, 0.0, -0.5), **two), 'l1')
  _refused(_apply(one, FTRL, params=_lib.FtrlParams(0.0, 0.0, 0.0, 0.5), **two), 'lr_power')
  _refused(_apply(one, FTRL, params=_lib.FtrlParams(0.0, 0.0, 0.0, -0.5), lr=-0.1, **two), 'lr must')
  _refused(_apply(one, ROWWISE, s0=[S0]), 'rowwise_adagrad is NULL')
  _refused(_apply(one, ROWWISE, s0=[S0], params=_lib.RowwiseAdagradParams(-1.0)), 'epsilon')
  _refused(_apply(one, ROWWISE, s0=[S0 + 2], params=_lib.RowwiseAdagradParams(1e-8)), 'accumulator must be')
  _refused(_apply(one, ROWWISE, params=_lib.RowwiseAdagradParams(1e-8)), 'slot0')
  # dim 256 needs 4 elements per lane: a table-shaped slot that is only 4-byte aligned refuses it, row-wise
  # Adagrad's one word per row does not decide the row shape, the table's 8-byte alignment does
  wide = [_scol(dim=256)]
  _refused(_apply(wide, ADAGRAD, s0=[S0 + 4]), 'dim 256')
  _refused(_apply(wide, ADAM, params=_adam(), s0=[S0], s1=[S1 + 8]), 'dim 256')
  _refused(_apply([_scol(dim=256, table=FAKE + 4)], ROWWISE, s0=[S0], params=_lib.RowwiseAdagradParams(1e-8)),
           'dim 256')
  _refused(_apply([_scol(dim=256, grad_rows=FAKE + 0x2004)], SGD), 'dim 256')
  lib = _lib.lib()
  _refused(lib.hbk_lowp_apply_slices_n(-1, None, SGD, None, None, None, C.c_float(0.1), None, None), 'n_cols')
  _refused(lib.hbk_lowp_apply_slices_n(1, None, SGD, None, None, None, C.c_float(0.1), None, None), 'cols is NULL')
  # nothing to do is no error and touches nothing (nearest: the counter is never read)
  assert lib.hbk_lowp_apply_slices_n(0, None, SGD, None, None, None, C.c_float(0.1), None, None) == _lib.OK
  assert lib.hbk_lowp_apply_slices_n(0, None, SGD, None, None, None, C.c_float(0.1), C.byref(_round(step=None)),
                                     None) == _lib.OK


# ---- the restatement of the rounding -------------------------------------------------------------------------------
LOWS = (0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def test_nearest_restatement_equals_torchs_cast_on_every_pattern_class():
  """Every fp32 pattern (h << 16) | low: h over all 65 536 upper halves, low over the six values that decide a
  rounding -- NaNs excepted (a NaN must stay a NaN; its payload is not specified)."""
  h = np.arange(1 << 16, dtype=np.uint32)
  for low in LOWS:
    u = (h << np.uint32(16)) | np.uint32(low)
    got = ref.bf16_nearest(u)
    want = torch.from_numpy(u.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = ref.is_nan(u)
    np.testing.assert_array_equal(got[~nan], want[~nan], err_msg=f'low half 0x{low:04x}')
    up = ref.bf16_up(got[nan])
    assert np.isnan(up).all() and np.isnan(ref.bf16_up(want[nan])).all()


def test_stochastic_restatement_rounds_up_exactly_above_its_threshold():
  rng = np.random.RandomState(7)
  highs = np.concatenate([rng.randint(0, 1 << 16, size=300), [0x0000, 0x8000, 0x3F80, 0xBF80, 0x7F7F, 0xFF7F, 0x0001]])
  highs = highs[(highs & 0x7F80) != 0x7F80].astype(np.uint32)          # (exponent all ones: nearest, below)
  lows = np.concatenate([rng.randint(0, 1 << 16, size=40), LOWS]).astype(np.uint32)
  n16 = np.concatenate([rng.randint(0, 1 << 16, size=60), [0, 1, 0x7FFF, 0x8000, 0xFFFF]]).astype(np.uint32)
  u = ((highs[:, None, None] << np.uint32(16)) | lows[None, :, None]) + np.zeros((1, 1, n16.size), np.uint32)
  lo = np.broadcast_to(lows[None, :, None], u.shape)
  nz = np.broadcast_to(n16[None, None, :], u.shape)
  # the upper 16 bits of the noise word are ignored
  got = ref.bf16_stochastic(u, nz | np.uint32(0xABCD0000))
  up = nz >= (np.uint32(0x10000) - lo)
  want = (np.broadcast_to(highs[:, None, None], u.shape) + up).astype(np.uint16)
  np.testing.assert_array_equal(got, want)
  assert not up[lo == 0].any()                        # an exact value never moves
  # magnitude rounding: the result is u's neighbour away from zero or u truncated, for both signs
  assert (np.abs(ref.bf16_up(got).astype(np.float64)) >= np.abs(ref.bf16_up((u >> 16).astype(np.uint16)))).all()
  # the carry out of the largest finite value is infinity
  assert ref.bf16_stochastic(np.uint32(0x7F7FFFFF), np.uint32(1)) == 0x7F80
  assert ref.bf16_stochastic(np.uint32(0xFF7F8000), np.uint32(0x8000)) == 0xFF80
  # exponent all ones: infinities stay, NaNs stay NaNs, whatever the noise
  assert ref.bf16_stochastic(np.uint32(0x7F800000), np.uint32(0xFFFF)) == 0x7F80
  assert ref.bf16_stochastic(np.uint32(0xFF800000), np.uint32(0xFFFF)) == 0xFF80
  assert np.isnan(ref.bf16_up(ref.bf16_stochastic(np.uint32(0x7F800001), np.uint32(0xFFFF))))


def test_noise_is_a_function_of_every_argument():
  rows = np.array([0, 1, 5, (1 << 32) + 5, -1 & 0x7FFFFFFFFFFFFFFF], np.int64)
  base = ref.noise(3, 9, 0, rows, 8)
  assert base.shape == (5, 8) and base.dtype == np.uint32
  np.testing.assert_array_equal(base, ref.noise(3, 9, 0, rows, 8))
  for other in (ref.noise(4, 9, 0, rows, 8), ref.noise(3, 10, 0, rows, 8), ref.noise(3, 9, 1, rows, 8)):
    assert (other != base).mean() > 0.99
  assert len(np.unique(base)) == base.size          # rows (their upper halves too) and elements all differ
  # fixed points of the definition (murmur3's finalizer)
  assert int(ref.fmix32(np.uint32(0))) == 0 and int(ref.fmix32(np.uint32(1))) == 0x514E28B7


# ---- Python ----------------------------------------------------------------------------------------------------------
class _TwoRanks:
  world_size, rank = 2, 0


def test_python_refusals_without_a_gpu():
  import hybridbackend_amd as hb
  from hybridbackend_amd.embedding import LowpGroupLookup, LowpLookupGrad, LowpSparseApply
  from hybridbackend_amd.embedding.lowp import check_rounding
  bad = _lib.InvalidArgumentError
  for cls in (LowpGroupLookup, LowpSparseApply):
    with pytest.raises(bad, match='bfloat16 or torch.float16'):
      cls([torch.zeros(4, 4)])                                   # an fp32 table, wherever it lives
    with pytest.raises(bad, match='bfloat16 or torch.float16'):
      cls([torch.zeros(4, dtype=torch.bfloat16)])
    with pytest.raises(_lib.HbkError, match='must live in HBM'):
      cls([torch.zeros(4, 4, dtype=torch.bfloat16)])
  with pytest.raises(bad, match='max_norms is not supported'):
    LowpGroupLookup([], max_norms=1.0)
  with pytest.raises(bad, match='max_norms is not supported'):
    LowpGroupLookup([], max_norms=[None, 2.0])
  with pytest.raises(bad, match='chunk_elems'):
    LowpGroupLookup([], chunk_elems=16)
  with pytest.raises(bad, match='needs a LowpGroupLookup'):
    LowpLookupGrad(object())
  grad = LowpLookupGrad.__new__(LowpLookupGrad)
  with pytest.raises(bad, match='weight_grads is not supported'):
    grad([], [], weight_grads=True)
  with pytest.raises(bad, match='weight_grads is not supported'):
    grad([], [], weight_grads=[None])
  with pytest.raises(bad, match="'nearest' or 'stochastic'"):
    check_rounding('up', 0, [torch.bfloat16], 'x')
  with pytest.raises(bad, match='bfloat16 tables only'):
    check_rounding('stochastic', 0, [torch.bfloat16, torch.float16], 'x')
  for seed in (-1, 1 << 32, 0.5, True):
    with pytest.raises(bad, match='seed'):
      check_rounding('nearest', seed, [torch.bfloat16], 'x')
  assert check_rounding('stochastic', 7, [torch.bfloat16], 'x') == (_lib.LOWP_ROUND_STOCHASTIC, 7)
  app = LowpSparseApply.__new__(LowpSparseApply)
  app.moments = app.ftrl_slots = app.row_accums = app.accums = None
  app.tables, app._slices_key, app._bound = [], None, None
  with pytest.raises(bad, match=r'LowpSparseApply\(tables, moments=\[\(m, v\), \.\.\.\]\)'):
    app([], 0.1, optimizer='adam')
  with pytest.raises(bad, match='accums='):
    app([], 0.1, optimizer='adagrad')
  with pytest.raises(bad, match='lr must be != 0'):
    app([], 0.0)
  with pytest.raises(_lib.HbkError, match='launch'):
    app.launch()
  # the layer: everything table_dtype refuses, before any table is allocated
  EC, DF = hb.feature_column.EmbeddingColumn, hb.feature_column.DenseFeatures
  cols = [EC('a', 100, 8), EC('b', 100, 16)]
  with pytest.raises(bad, match='table_dtype'):
    DF(cols, 'cpu', table_dtype=torch.float32)
  with pytest.raises(bad, match='one rank only'):
    DF(cols, 'cpu', coll=_TwoRanks(), table_dtype=torch.bfloat16)
  with pytest.raises(bad, match="'h' is hash-keyed"):
    DF(cols + [hb.feature_column.HashEmbeddingColumn('h', 64, 8)], 'cpu', table_dtype=torch.bfloat16)
  with pytest.raises(bad, match="'c' has max_norm"):
    DF(cols + [EC('c', 100, 8, max_norm=1.0)], 'cpu', table_dtype=torch.float16)
  with pytest.raises(bad, match="'w'.*cannot be addressed in place"):
    DF([EC('a', 100, 3), EC('w', 100, 128)], 'cpu', table_dtype=torch.bfloat16)
  with pytest.raises(bad, match='bfloat16 tables only'):
    DF(cols, 'cpu', table_dtype=torch.float16, table_rounding='stochastic')
  with pytest.raises(bad, match='seed'):
    DF(cols, 'cpu', table_dtype=torch.bfloat16, table_seed=-1)
