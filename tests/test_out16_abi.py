"""16-bit outputs at the C ABI and in Python, without a GPU: every refusal of hbk_group_lookup_fwd_out16 precedes any
device work (the addresses here are no device buffers) and names its column; the Python class and the layer refuse
what they do not serve, by name."""
import ctypes as C

import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib

FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it
BF16, FP16 = _lib.LOWP_BF16, _lib.LOWP_FP16


def _col(**kw):
  col = _lib.Out16LookupColumn()
  col.table, col.table_dtype, col.rows, col.dim = FAKE, _lib.OUT16_TABLE_FP32, 100, 16
  col.ids, col.ids_dtype, col.n_ids, col.n_segments = FAKE + 0x1000, _lib.INT64, 8, 8
  col.divisor, col.combiner, col.out, col.out_dtype = 1, _lib.COMBINER_SUM, FAKE + 0x2000, BF16
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _fwd(cols):
  n = len(cols)
  return _lib.lib().hbk_group_lookup_fwd_out16(n, (_lib.Out16LookupColumn * n)(*cols), None)


def _refused(rc, *words):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in words:
    assert w in msg, msg


@pytest.mark.parametrize('kw, words', [
  (dict(table_dtype=3), ('table_dtype',)),
  (dict(table_dtype=-1), ('table_dtype',)),
  (dict(out_dtype=0), ('out_dtype',)),
  (dict(out_dtype=3), ('out_dtype',)),
  (dict(ids_dtype=_lib.FLOAT), ('int32 or int64',)),
  (dict(combiner=3), ('combiner',)),
  (dict(chunk_elems=16), ('chunk_elems',)),
  (dict(reserved=1), ('reserved',)),
  (dict(dim=0), ('dim must be >= 1',)),
  (dict(dim=65), ('dim 65', '64 otherwise')),
  (dict(dim=260), ('dim 260', 'at most 256')),
  (dict(dim=128, out=FAKE + 0x2002), ('dim 128', '64 otherwise')),              # one element per lane holds 64
  (dict(dim=128, out_stride=130), ('dim 128',)),
  (dict(dim=128, table=FAKE + 8), ('dim 128',)),                                # an fp32 table needs 16 bytes
  (dict(dim=128, table=FAKE + 4, table_dtype=BF16), ('dim 128',)),              # a 16-bit table 8
  (dict(out=FAKE + 0x2001), ('2-byte aligned',)),
  (dict(table=FAKE + 2), ('aligned to its element',)),
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
def test_refusals_name_the_column(kw, words):
  _refused(_fwd([_col(n_segments=0, n_ids=0), _col(**kw)]), 'column 1', *words)


def test_struct_and_nothing_to_do():
  lib = _lib.lib()
  assert C.sizeof(_lib.Out16LookupColumn) == 112 and '0.2.0' in lib.hbk_version().decode()
  _refused(lib.hbk_group_lookup_fwd_out16(-1, None, None), 'n_cols')
  _refused(lib.hbk_group_lookup_fwd_out16(1, None, None), 'cols is NULL')
  assert lib.hbk_group_lookup_fwd_out16(0, None, None) == _lib.OK
  # a column without segments launches nothing, whatever its buffers
  assert _fwd([_col(n_segments=0, n_ids=0, table=None, ids=None, out=None)]) == _lib.OK


class _TwoRanks:
  world_size, rank = 2, 0


def test_python_refusals_without_a_gpu():
  from hybridbackend_amd.embedding import Out16GroupLookup, SequenceLookup
  bad = _lib.InvalidArgumentError
  with pytest.raises(bad, match='max_norms is not supported'):
    Out16GroupLookup([], max_norms=1.0)
  with pytest.raises(bad, match='hot_rows is not supported'):
    Out16GroupLookup([], hot_rows='auto')
  with pytest.raises(bad, match='chunk_elems'):
    Out16GroupLookup([], chunk_elems=16)
  with pytest.raises(bad, match='out_dtype must be'):
    Out16GroupLookup([], out_dtype=torch.float32)
  with pytest.raises(bad, match='table 0 must be'):
    Out16GroupLookup([torch.zeros(4, 4, dtype=torch.float64)])
  with pytest.raises(_lib.HbkError, match='must live in HBM'):
    Out16GroupLookup([torch.zeros(4, 4)])
  one = Out16GroupLookup.__new__(Out16GroupLookup)
  one.tables, one.out_dtype, one._dims = [None], torch.bfloat16, [4]
  with pytest.raises(bad, match=r'output 0 must be a torch.bfloat16 tensor \(out_dtype\), got torch.float32'):
    one.bind([torch.zeros(2, dtype=torch.int64)], None, [torch.zeros(2, 4)])
  with pytest.raises(bad, match='max_norms is not supported with out_dtype'):
    SequenceLookup([], max_lens=4, max_norms=1.0, out_dtype=torch.float16)
  with pytest.raises(bad, match='out_dtype must be'):
    SequenceLookup([], max_lens=4, out_dtype=torch.int16)
  # the layer: everything output_dtype refuses, before any table is allocated
  EC, DF = hb.feature_column.EmbeddingColumn, hb.feature_column.DenseFeatures
  cols = [EC('a', 100, 8), EC('b', 100, 16)]
  with pytest.raises(bad, match='output_dtype'):
    DF(cols, 'cpu', output_dtype=torch.float32)
  with pytest.raises(bad, match='one rank only'):
    DF(cols, 'cpu', coll=_TwoRanks(), output_dtype=torch.bfloat16)
  with pytest.raises(bad, match="'h' is hash-keyed"):
    DF(cols + [hb.feature_column.HashEmbeddingColumn('h', 64, 8)], 'cpu', output_dtype=torch.bfloat16)
  with pytest.raises(bad, match="'c' has max_norm"):
    DF(cols + [EC('c', 100, 8, max_norm=1.0)], 'cpu', output_dtype=torch.float16)
  with pytest.raises(bad, match="'w'.*staged through a tensor of its own"):
    DF([EC('a', 100, 3), EC('w', 100, 128)], 'cpu', output_dtype=torch.bfloat16)
