"""8-bit tables at the C ABI and in Python, without a GPU: the new symbols and their prototypes; every refusal of the
four entries precedes any device work (the addresses here are no device buffers) and names what it refuses; the
Python classes and the layer refuse what they do not serve, by name."""
import ctypes as C

import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib

FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it
LOOKUP, SLICES, ROWS = _lib.Quant8LookupColumn, _lib.Quant8SlicesColumn, _lib.Quant8RowsColumn


def _make(struct, base, kw):
  col = struct()
  for k, v in {**base, **kw}.items():
    setattr(col, k, v)
  return col


def _lookup(**kw):
  return _make(LOOKUP, dict(table=FAKE, rows=100, dim=16, ids=FAKE + 0x1000, ids_dtype=_lib.INT64, n_ids=8,
                            n_segments=8, divisor=1, combiner=_lib.COMBINER_SUM, out=FAKE + 0x2000), kw)


def _slices(**kw):
  return _make(SLICES, dict(table=FAKE, rows=100, dim=16, unique_rows=FAKE + 0x1000, grad_rows=FAKE + 0x2000,
                            n_unique=FAKE + 0x3000, capacity=8), kw)


def _rows(**kw):
  return _make(ROWS, dict(table=FAKE, rows_f=FAKE + 0x1000, rows=8, dim=16), kw)


def _refused(rc, *words):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in words:
    assert w in msg, msg


def _fwd(cols):
  return _lib.lib().hbk_quant8_lookup_fwd(len(cols), (LOOKUP * len(cols))(*cols), None)


def _apply(cols, apply=_lib.APPLY_SGD, s0=None, s1=None, params=None, lr=0.1, rounding=None):
  ptrs = lambda x: None if x is None else (C.c_void_p * len(cols))(*x)   # noqa: E731
  return _lib.lib().hbk_quant8_apply_slices_n(len(cols), (SLICES * len(cols))(*cols), apply, ptrs(s0), ptrs(s1),
                                              params, C.c_float(lr), rounding, None)


def test_symbols_prototypes_and_nothing_to_do():
  lib = _lib.lib()
  assert '0.2.0' in lib.hbk_version().decode()
  assert (C.sizeof(LOOKUP), C.sizeof(SLICES), C.sizeof(ROWS)) == (104, 56, 40)
  vp, i32 = C.c_void_p, C.c_int32
  for name, args in (('hbk_quant8_rows_n', [i32, vp, vp, vp]), ('hbk_dequant8_rows_n', [i32, vp, vp]),
                     ('hbk_quant8_lookup_fwd', [i32, vp, vp]),
                     ('hbk_quant8_apply_slices_n', [i32, vp, i32, vp, vp, vp, C.c_float, vp, vp])):
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == args, name
  assert lib.hbk_quant8_lookup_fwd(0, None, None) == _lib.OK
  assert lib.hbk_quant8_rows_n(0, None, None, None) == _lib.OK and lib.hbk_dequant8_rows_n(0, None, None) == _lib.OK
  _refused(lib.hbk_quant8_lookup_fwd(-1, None, None), 'n_cols')
  _refused(lib.hbk_quant8_lookup_fwd(1, None, None), 'cols is NULL')
  # a column without segments or rows launches nothing, whatever its buffers
  assert _fwd([_lookup(n_segments=0, n_ids=0, table=None, ids=None, out=None)]) == _lib.OK
  assert lib.hbk_dequant8_rows_n(1, (ROWS * 1)(_rows(rows=0, table=None, rows_f=None)), None) == _lib.OK


@pytest.mark.parametrize('kw, words', [
  (dict(dim=0), ('dim must be in [1, 256]',)),
  (dict(dim=260, pitch=264), ('dim must be in [1, 256]',)),
  (dict(pitch=18), ('pitch 18', 'multiple of 4')),
  (dict(pitch=16), ('pitch 16', '>= round_up(dim, 4) + 4 = 20')),
  (dict(dim=3, pitch=4), ('pitch 4',)),
  (dict(table=FAKE + 2), ('table must be 4-byte aligned',)),
  (dict(out_dtype=3), ('out_dtype',)),
  (dict(out_dtype=-1), ('out_dtype',)),
  (dict(out=FAKE + 0x2002), ('out must be aligned to its element',)),
  (dict(out=FAKE + 0x2001, out_dtype=_lib.LOWP_BF16), ('out must be aligned to its element',)),
  (dict(chunk_elems=8), ('chunk_elems must be 0 or 4',)),
  (dict(dim=65, pitch=72), ('dim 65', '64 otherwise')),
  (dict(dim=128, out=FAKE + 0x2004), ('dim 128', '64 otherwise')),            # one code per lane holds 64
  (dict(dim=128, out=FAKE + 0x2004, out_dtype=_lib.LOWP_FP16), ('dim 128',)),
  (dict(dim=128, out_stride=130), ('dim 128',)),
  (dict(ids_dtype=_lib.FLOAT), ('int32 or int64',)),
  (dict(combiner=3), ('combiner',)),
  (dict(table=None), ('table is NULL',)),
  (dict(ids=None), ('ids is NULL',)),
  (dict(out=None), ('out is NULL',)),
  (dict(n_ids=-1, n_segments=-1), ('negative',)),
  (dict(n_ids=1 << 31, n_segments=1 << 31), ('2^31',)),
  (dict(bucket=-1), ('bucket',)),
  (dict(divisor=0), ('divisor',)),
  (dict(out_stride=8), ('out_stride',)),
  (dict(n_segments=7), ('n_segments',)),
])
def test_forward_refusals_name_the_column(kw, words):
  _refused(_fwd([_lookup(n_segments=0, n_ids=0), _lookup(**kw)]), 'column 1', *words)


def test_step_refusals():
  _refused(_apply([_slices()], apply=1), 'apply must be')
  _refused(_apply([_slices()], lr=0.0), 'lr must be finite and != 0')
  _refused(_apply([_slices(pitch=22)]), 'column 0', 'pitch 22')
  _refused(_apply([_slices(dim=300, pitch=304)]), 'dim must be in [1, 256]')
  _refused(_apply([_slices(table=FAKE + 1)]), 'table must be 4-byte aligned')
  _refused(_apply([_slices(dim=68, pitch=72, grad_rows=FAKE + 0x2004)]), 'dim 68', '64 otherwise')
  _refused(_apply([_slices(capacity=-1)]), 'capacity')
  _refused(_apply([_slices(table=None)]), 'table is NULL')
  _refused(_apply([_slices(unique_rows=None)]), 'unique_rows')
  _refused(_apply([_slices(grad_rows=None)]), 'grad_rows')
  _refused(_apply([_slices(n_unique=None)]), 'n_unique')
  _refused(_apply([_slices(), _slices()]), 'two columns name the same table')
  _refused(_apply([_slices()], apply=_lib.APPLY_ADAGRAD), 'the accumulator array (slot0) is NULL')
  _refused(_apply([_slices()], apply=_lib.APPLY_ADAGRAD, s0=[None]), 'the accumulator must be a device fp32 buffer')
  _refused(_apply([_slices()], apply=_lib.APPLY_LAZY_ADAM), 'adam is NULL')
  _refused(_apply([_slices()], apply=_lib.APPLY_FTRL), 'ftrl is NULL')
  _refused(_apply([_slices()], apply=_lib.APPLY_ROWWISE_ADAGRAD), 'rowwise_adagrad is NULL')
  bad_mode = _lib.LowpRounding(7, 0, None, 0, 0)
  _refused(_apply([_slices()], rounding=C.byref(bad_mode)), 'rounding mode')
  no_step = _lib.LowpRounding(_lib.LOWP_ROUND_STOCHASTIC, 0, None, 1, 0)
  _refused(_apply([_slices()], rounding=C.byref(no_step)), 'step counter')


def test_quantise_and_dequantise_refusals():
  lib = _lib.lib()
  q = lambda col, r=None: lib.hbk_quant8_rows_n(1, (ROWS * 1)(col), r, None)   # noqa: E731
  d = lambda col: lib.hbk_dequant8_rows_n(1, (ROWS * 1)(col), None)   # noqa: E731
  _refused(q(_rows(dim=257, pitch=264)), 'column 0', 'dim must be in [1, 256]')
  _refused(q(_rows(pitch=21)), 'pitch 21')
  _refused(q(_rows(table=FAKE + 2)), '4-byte aligned')
  _refused(q(_rows(src_dtype=3)), 'src_dtype')
  _refused(q(_rows(rows_f=FAKE + 0x1002)), 'rows_f must be aligned')
  _refused(q(_rows(rows_f=FAKE + 0x1001, src_dtype=_lib.LOWP_BF16)), 'rows_f must be aligned')
  _refused(q(_rows(rows_f=None)), 'is NULL')
  _refused(q(_rows(rows=-1)), 'rows must be in')
  _refused(q(_rows(reserved=1)), 'reserved')
  _refused(q(_rows(), C.byref(_lib.LowpRounding(_lib.LOWP_ROUND_STOCHASTIC, 0, None, 0, 0))), 'step counter')
  _refused(d(_rows(src_dtype=_lib.LOWP_FP16)), 'src_dtype must be 0')
  _refused(d(_rows(pitch=16)), 'pitch 16')


class _TwoRanks:
  world_size, rank = 2, 0


def test_python_refusals_without_a_gpu():
  E = hb.embedding
  bad = _lib.InvalidArgumentError
  assert E.Quant8Rows.pitch_for(1) == 8 and E.Quant8Rows.pitch_for(64) == 68 and E.Quant8Rows.pitch_for(130) == 136
  with pytest.raises(bad, match='max_norms is not supported'):
    E.Quant8GroupLookup([], [], max_norms=1.0)
  with pytest.raises(bad, match='hot_rows is not supported'):
    E.Quant8GroupLookup([], [], hot_rows='auto')
  with pytest.raises(bad, match='chunk_elems must be None or 4'):
    E.Quant8GroupLookup([], [], chunk_elems=8)
  with pytest.raises(bad, match='out_dtype must be'):
    E.Quant8GroupLookup([], [], out_dtype=torch.int8)
  with pytest.raises(bad, match='table 0 must be a torch.uint8'):
    E.Quant8GroupLookup([torch.zeros(4, 8)], [4])
  with pytest.raises(bad, match='1 dims for 0 tables'):
    E.Quant8GroupLookup([], [4])
  with pytest.raises(bad, match='pitch 6 must be a multiple of 4'):
    E.Quant8GroupLookup([torch.zeros(4, 6, dtype=torch.uint8)], [2])
  with pytest.raises(bad, match=r'pitch 16 must be .* >= 20 for dim 16'):
    E.dequantize_rows8([torch.zeros(4, 16, dtype=torch.uint8)], [16])
  with pytest.raises(bad, match=r'dim must be in \[1, 256\]'):
    E.Quant8SparseApply([torch.zeros(4, 264, dtype=torch.uint8)], [260])
  with pytest.raises(_lib.HbkError, match='must live in HBM'):
    E.Quant8GroupLookup([torch.zeros(4, 8, dtype=torch.uint8)], [4])
  with pytest.raises(bad, match="rounding must be 'nearest' or 'stochastic'"):
    E.Quant8SparseApply([], [], rounding='up')
  with pytest.raises(bad, match='seed must be an integer'):
    E.quantize_rows8([], seed=-1)
  with pytest.raises(bad, match='table 0 must be a torch.float32, torch.bfloat16 or torch.float16'):
    E.quantize_rows8([torch.zeros(4, 4, dtype=torch.float64)])
  with pytest.raises(bad, match='needs a Quant8GroupLookup'):
    E.Quant8LookupGrad(object())
  with pytest.raises(bad, match='weight_grads is not supported for 8-bit tables'):
    E.Quant8LookupGrad._refuse_weight_grads(True)
  # the layer: everything table_dtype='int8' refuses, before any table is allocated
  EC, DF = hb.feature_column.EmbeddingColumn, hb.feature_column.DenseFeatures
  cols = [EC('a', 100, 8), EC('b', 100, 16)]
  with pytest.raises(bad, match="torch.float16 or 'int8', got 'int4'"):
    DF(cols, 'cpu', table_dtype='int4')
  with pytest.raises(bad, match='8-bit tables are kept on one rank only'):
    DF(cols, 'cpu', coll=_TwoRanks(), table_dtype='int8', lowp_sharded=True)
  with pytest.raises(bad, match="'h' is hash-keyed"):
    DF(cols + [hb.feature_column.HashEmbeddingColumn('h', 64, 8)], 'cpu', table_dtype='int8')
  with pytest.raises(bad, match="'c' has max_norm"):
    DF(cols + [EC('c', 100, 8, max_norm=1.0)], 'cpu', table_dtype='int8')
  with pytest.raises(bad, match="'w'.*cannot be addressed in place"):
    DF([EC('a', 100, 3), EC('w', 100, 128)], 'cpu', table_dtype='int8')
  with pytest.raises(bad, match="'w': dimension 66 is beyond what the 8-bit step takes"):
    DF([EC('a', 100, 4), EC('w', 100, 66)], 'cpu', table_dtype='int8')
  with pytest.raises(bad, match="rounding must be"):
    DF(cols, 'cpu', table_dtype='int8', table_rounding='up')
