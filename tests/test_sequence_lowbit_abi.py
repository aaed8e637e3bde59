"""Sequence lookups over low-bit tables at the C ABI and in Python, without a GPU: the two symbols, the descriptor's
size, every refusal before any device work (the addresses here are no device buffers) with the column named, the lane
query on fake pointers, the Python refusals."""
import ctypes as C

import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib

FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it
COLUMN = _lib.SequenceLowbitColumn
BF16, FP16, INT8, FP32 = _lib.LOWP_BF16, _lib.LOWP_FP16, _lib.ROWS_INT8, _lib.QUANT8_OUT_FP32


def _column(**kw):
  col = COLUMN()
  for k, v in {**dict(table=FAKE, rows=100, dim=16, ids=FAKE + 0x1000, ids_dtype=_lib.INT64, n_ids=8, n_segments=8,
                      divisor=1, row_format=INT8, out=FAKE + 0x2000), **kw}.items():
    setattr(col, k, v)
  return col


def _fwd(cols, max_len=5):
  seqs = (_lib.Sequence * len(cols))()
  for q in seqs:
    q.max_len = max_len
  return _lib.lib().hbk_sequence_lookup_fwd_lowbit(len(cols), (COLUMN * len(cols))(*cols), seqs, None)


def _refused(rc, *words):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in words:
    assert w in msg, msg


def test_symbols_prototypes_and_nothing_to_do():
  lib = _lib.lib()
  vp, i32 = C.c_void_p, C.c_int32
  assert C.sizeof(COLUMN) == 96 and INT8 == 3
  assert lib.hbk_sequence_lookup_fwd_lowbit.restype is C.c_int
  assert list(lib.hbk_sequence_lookup_fwd_lowbit.argtypes) == [i32, vp, vp, vp]
  assert lib.hbk_sequence_lowbit_lane_elems.restype is i32
  assert list(lib.hbk_sequence_lowbit_lane_elems.argtypes) == [vp]
  assert lib.hbk_sequence_lookup_fwd_lowbit(0, None, None, None) == _lib.OK
  # a column without samples launches nothing, whatever its buffers
  for fmt in (BF16, FP16, INT8):
    assert _fwd([_column(row_format=fmt, n_segments=0, n_ids=0, table=None, ids=None, out=None)]) == _lib.OK
  _refused(lib.hbk_sequence_lookup_fwd_lowbit(-1, None, None, None), 'n_cols')
  _refused(lib.hbk_sequence_lookup_fwd_lowbit(1, None, None, None), 'cols is NULL')
  _refused(lib.hbk_sequence_lookup_fwd_lowbit(1, (COLUMN * 1)(_column()), None, None), 'seq is NULL')


@pytest.mark.parametrize('kw, words', [
  (dict(row_format=0), ('row_format must be', 'got 0')),
  (dict(row_format=4), ('row_format must be', 'got 4')),
  (dict(out_dtype=3), ('out_dtype must be', 'got 3')),
  (dict(pitch=18), ('pitch 18', 'multiple of 4')),
  (dict(pitch=16), ('pitch 16', '>= round_up(dim, 4) + 4 = 20')),
  (dict(row_format=BF16, pitch=30), ('pitch 30', '>= 2 * dim = 32')),
  (dict(row_format=FP16, pitch=33), ('pitch 33', 'even')),
  (dict(table=FAKE + 2), ('8-bit table must be 4-byte aligned',)),
  (dict(row_format=BF16, table=FAKE + 1), ('16-bit table must be 2-byte aligned',)),
  (dict(dim=0), ('dim must be in [1, 256]',)),
  (dict(dim=260, pitch=264), ('dim must be in [1, 256]',)),
  (dict(dim=65, pitch=72), ('dim 65', '64 otherwise')),
  (dict(dim=128, out=FAKE + 0x2004), ('dim 128', '64 otherwise')),   # falls to one element per lane, which holds 64
  (dict(out_stride=79), ('out_stride 79', 'max_len * dim = 80')),
  (dict(out=FAKE + 0x2002), ('out must be aligned to its element',)),
  (dict(out=FAKE + 0x2001, out_dtype=BF16), ('out must be aligned to its element',)),
  (dict(ids_dtype=_lib.FLOAT), ('int32 or int64',)),
  (dict(table=None), ('table is NULL',)),
  (dict(ids=None), ('ids is NULL',)),
  (dict(out=None), ('out is NULL',)),
  (dict(n_ids=-1, n_segments=-1), ('negative',)),
  (dict(n_ids=1 << 29, n_segments=1 << 29), ('B * T', '2^31')),
  (dict(bucket=-1), ('bucket',)),
  (dict(divisor=0), ('divisor',)),
  (dict(n_segments=7), ('n_segments',)),
])
def test_refusals_name_the_column(kw, words):
  _refused(_fwd([_column(n_segments=0, n_ids=0), _column(**kw)]), 'sequence_lookup_fwd_lowbit', 'column 1', *words)


def test_max_len_is_refused():
  _refused(_fwd([_column()], max_len=0), 'column 0', 'max_len must be >= 1, got 0')


@pytest.mark.parametrize('kw, width', [
  (dict(out_dtype=BF16), 8), (dict(out_dtype=FP16, dim=256, pitch=260), 8), (dict(out_dtype=BF16, dim=24), 8),
  (dict(out_dtype=FP32), 4), (dict(out_dtype=FP32, dim=12), 4), (dict(out_dtype=FP32, dim=256, pitch=260), 4),
  (dict(out_dtype=BF16, dim=12), 4), (dict(out_dtype=BF16, out=FAKE + 0x2008), 4),      # 16-bit: 8 bytes carry 4
  (dict(out_dtype=BF16, out_stride=84), 4), (dict(out_dtype=BF16, out_stride=82), 1),     # the sample stride
  (dict(out_dtype=BF16, dim=7), 1), (dict(out_dtype=FP32, dim=63), 1), (dict(out_dtype=FP32, out=FAKE + 0x2008), 1),
  (dict(out_dtype=BF16, out=FAKE + 0x2004), 1), (dict(out_dtype=FP32, out_stride=82), 1),
  (dict(row_format=BF16, out_dtype=BF16), 8), (dict(row_format=FP16, out_dtype=FP32), 4),
  (dict(row_format=BF16, out_dtype=BF16, table=FAKE + 8), 8),                             # two 8-byte loads
  (dict(row_format=BF16, out_dtype=FP32, dim=12, table=FAKE + 24), 4),                    # a view from row 1
  (dict(row_format=BF16, out_dtype=BF16, table=FAKE + 4), 1), (dict(row_format=FP16, out_dtype=FP32, pitch=36), 1),
  (dict(row_format=0), 0), (dict(out_dtype=7), 0), (dict(dim=0), 0),
])
def test_lane_query(kw, width):
  lib = _lib.lib()
  assert lib.hbk_sequence_lowbit_lane_elems(C.byref(_column(**kw))) == width
  assert lib.hbk_sequence_lowbit_lane_elems(None) == 0


def test_python_refusals():
  E, bad = hb.embedding, _lib.InvalidArgumentError
  bf, u8, f32 = (torch.zeros(4, 8, dtype=d) for d in (torch.bfloat16, torch.uint8, torch.float32))
  with pytest.raises(bad, match='mix 16-bit and 8-bit rows.*SequenceLookup'):
    E.LowbitSequenceLookup([bf, u8], dims=[8, 4], max_lens=3)
  with pytest.raises(bad, match='table 1 must be .*torch.float32.*fp32 tables go through SequenceLookup'):
    E.LowbitSequenceLookup([bf, f32], max_lens=3)
  with pytest.raises(bad, match='out_dtype must be torch.float32, torch.bfloat16 or torch.float16'):
    E.LowbitSequenceLookup([], max_lens=3, out_dtype=torch.float64)
  with pytest.raises(bad, match='2 dims for 1 tables'):
    E.LowbitSequenceLookup([u8], dims=[4, 4], max_lens=3)
  with pytest.raises(bad, match='8-bit tables need dims'):
    E.LowbitSequenceLookup([u8], max_lens=3)
  with pytest.raises(bad, match=r'dims \[4\] do not match'):
    E.LowbitSequenceLookup([bf], dims=[4], max_lens=3)
  with pytest.raises(bad, match='needs a LowbitSequenceLookup'):
    E.LowbitSequenceLookupGrad(object())
  assert not hasattr(E.LowbitSequenceLookup([], max_lens=3), 'max_norms')
  SF, SC = hb.feature_column.SequenceFeatures, hb.feature_column.SequenceEmbeddingColumn
  with pytest.raises(bad, match=r'output_dtype=torch.bfloat16\) needs table_dtype.*SequenceLookup\(out_dtype=\)'):
    SF([SC('a', 100, 8, max_len=4)], 'cpu', output_dtype=torch.bfloat16)
  with pytest.raises(bad, match="table_dtype=\\): None, torch.bfloat16, torch.float16 or 'int8', got torch.float32"):
    SF([SC('a', 100, 8, max_len=4)], 'cpu', table_dtype=torch.float32)
  with pytest.raises(bad, match="column 'a' has max_norm"):
    SF([SC('a', 100, 8, max_len=4, max_norm=1.0)], 'cpu', table_dtype='int8')
  with pytest.raises(bad, match="column 'b': dimension 66 is beyond"):
    SF([SC('a', 100, 68, max_len=4), SC('b', 100, 66, max_len=4)], 'cpu', table_dtype=torch.float16)
  with pytest.raises(bad, match='kept on one rank only, the layer spans 2'):
    SF([SC('a', 100, 8, max_len=4)], 'cpu', coll=type('Coll', (), dict(world_size=2, rank=0))(), table_dtype='int8')
  with pytest.raises(bad, match="column 'h' is hash-keyed"):
    SF([hb.feature_column.HashSequenceEmbeddingColumn('h', 64, 8, max_len=4)], 'cpu', table_dtype='int8')
