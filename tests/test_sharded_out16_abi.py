"""The 16-bit stitch and the sharded 16-bit forward without a GPU: the symbols exist, every refusal of
hbk_lookup_fwd_runs_out16 precedes any device work and names its column, the Python classes refuse by name."""
import ctypes as C

import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import LowpShardedGroupLookup, ShardedGroupLookup
from tests.test_out16_abi import BF16, FAKE, FP16, _refused, _TwoRanks


def _col(runs=None, **kw):
  r = _lib.Out16RunsColumn()
  col = r.col
  col.table, col.table_dtype, col.rows, col.dim = FAKE, _lib.OUT16_TABLE_FP32, 100, 16
  col.ids, col.ids_dtype, col.n_ids, col.n_segments = FAKE + 0x1000, _lib.INT32, 8, 8
  col.divisor, col.combiner, col.out, col.out_dtype = 1, _lib.COMBINER_SUM, FAKE + 0x2000, BF16
  r.run_start, r.run_base, r.n_runs = FAKE + 0x3000, FAKE + 0x4000, 3
  for k, v in kw.items():
    setattr(col, k, v)
  for k, v in (runs or {}).items():
    setattr(r, k, v)
  return r


def _fwd(cols):
  return _lib.lib().hbk_lookup_fwd_runs_out16(len(cols), (_lib.Out16RunsColumn * len(cols))(*cols), None)


@pytest.mark.parametrize('kw, runs, words', [
  (dict(table_dtype=3), None, ('table_dtype',)), (dict(out_dtype=0), None, ('out_dtype',)),
  (dict(combiner=3), None, ('combiner',)), (dict(ids_dtype=_lib.FLOAT), None, ('int32 or int64',)),
  (dict(dim=0), None, ('dim must be >= 1',)), (dict(dim=65), None, ('dim 65', '64 otherwise')),
  (dict(dim=260), None, ('dim 260', 'at most 256')), (dict(dim=128, out_stride=130), None, ('dim 128',)),
  (dict(dim=128, table=FAKE + 8), None, ('dim 128',)),
  (dict(dim=128, table=FAKE + 4, table_dtype=BF16), None, ('dim 128',)),
  ({}, dict(n_runs=0), ('segmented-table',)), ({}, dict(run_start=None), ('segmented-table',)),
  ({}, dict(run_base=None), ('segmented-table',)), (dict(out=FAKE + 0x2001), None, ('2-byte aligned',)),
  (dict(table=FAKE + 2), None, ('aligned to its element',)), (dict(n_ids=-1, n_segments=-1), None, ('negative',)),
  (dict(out_stride=8), None, ('out_stride',)), (dict(n_segments=7), None, ('n_segments',)),
  (dict(reserved=1), None, ('reserved',)), ({}, dict(reserved=1), ('reserved',)),
  (dict(chunk_elems=16), None, ('chunk_elems',)), (dict(bucket=7), None, ('bucket must be 0',)),
  (dict(divisor=2), None, ('divisor 1',)),
])
def test_refusals_name_the_column(kw, runs, words):
  _refused(_fwd([_col(n_segments=0, n_ids=0), _col(runs, **kw)]), 'column 1', *words)


def test_symbols_struct_and_nothing_to_do():
  lib = _lib.lib()
  assert lib.hbk_sharded_lookup_fwd_weighted_out16 is not None   # (the other three are called below)
  assert C.sizeof(_lib.Out16RunsColumn) == 136 and '0.2.0' in lib.hbk_version().decode()
  _refused(lib.hbk_lookup_fwd_runs_out16(-1, None, None), 'n_cols')
  _refused(lib.hbk_lookup_fwd_runs_out16(1, None, None), 'cols is NULL')
  assert lib.hbk_lookup_fwd_runs_out16(0, None, None) == _lib.OK
  assert _fwd([_col(n_segments=0, n_ids=0, table=None, ids=None, out=None)]) == _lib.OK   # (nothing to launch)
  _refused(lib.hbk_sharded_lookup_fwd_end_out16(None, None, None, BF16, None), 'NULL')
  _refused(lib.hbk_sharded_lookup_fwd_out16(None, None, None, None, None, None, None, FP16, None), 'NULL')


def test_python_refusals_without_a_gpu():
  bad = _lib.InvalidArgumentError
  with pytest.raises(bad, match='ShardedGroupLookup: out_dtype must be None, torch.bfloat16 or torch.float16'):
    ShardedGroupLookup([], _TwoRanks(), out_dtype=torch.float32)
  with pytest.raises(bad, match='LowpShardedGroupLookup: out_dtype must be'):
    LowpShardedGroupLookup([], _TwoRanks(), out_dtype=torch.int16)
  one = ShardedGroupLookup.__new__(ShardedGroupLookup)
  one.shards, one.dims, one.out_dtype = [None], [4], torch.float16
  with pytest.raises(_lib.HbkError, match='p2p_bind: not with out_dtype=torch.float16.*no stitch to round in'):
    one.p2p_bind([torch.zeros(2, 4)])
  # the layer spans more than one rank with out16_sharded; what it still refuses, it refuses by name
  EC, DF = hb.feature_column.EmbeddingColumn, hb.feature_column.DenseFeatures
  cols = [EC('a', 100, 8), EC('b', 100, 16)]
  kw = dict(coll=_TwoRanks(), out16_sharded=True)
  with pytest.raises(bad, match='one rank only.*out16_sharded=True'):
    DF(cols, 'cpu', coll=_TwoRanks(), output_dtype=torch.bfloat16)
  DF._check_out16(cols, _TwoRanks(), torch.bfloat16, True)   # pylint: disable=protected-access
  with pytest.raises(bad, match="'h' is hash-keyed"):
    DF(cols + [hb.feature_column.HashEmbeddingColumn('h', 64, 8)], 'cpu', output_dtype=torch.bfloat16, **kw)
  with pytest.raises(bad, match="'c' has max_norm"):
    DF(cols + [EC('c', 100, 8, max_norm=1.0)], 'cpu', output_dtype=torch.float16, **kw)
