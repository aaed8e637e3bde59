"""Low-precision sharded tables at the C ABI and in Python, without a GPU: the three new symbols are declared in the
header, exported by the library and bound by the ctypes layer; the two kernel entries refuse before any device work
(the addresses here are no device buffers); the driver and the layer name what they refuse."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it
NEW = ('hbk_lowp_gather_rows_n', 'hbk_lowp_lookup_fwd_runs', 'hbk_sharded_set_table_dtypes')


def test_new_symbols_declared_exported_and_bound():
  lib = _lib.lib()
  out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True)
  exported = {line.split()[-1] for line in out.stdout.splitlines()}
  for name in NEW:
    assert re.search(r'\b' + name + r'\s*\(', HEADER), name
    assert name in exported, name
    assert getattr(lib, name).argtypes is not None, name
  for struct in ('hbk_lowp_gather_column_t', 'hbk_lowp_lookup_runs_column_t'):
    assert struct in HEADER
  assert (C.sizeof(_lib.LowpGatherColumn), C.sizeof(_lib.LowpLookupRunsColumn)) == (64, 128)
  codes = {k: int(re.search(r'#define HBK_LOWP_WIRE_' + k + r' (\d+)', HEADER).group(1)) for k in ('TABLE', 'FLOAT')}
  assert codes == dict(TABLE=_lib.LOWP_WIRE_TABLE, FLOAT=_lib.LOWP_WIRE_FLOAT)
  # the structs and the version the other entries share did not move
  assert (C.sizeof(_lib.LowpLookupColumn), C.sizeof(_lib.LowpSlicesColumn), C.sizeof(_lib.LowpRounding)) == (104, 56, 24)
  assert C.sizeof(_lib.LookupColumn) == 128 and C.sizeof(_lib.LookupGradColumn) == 160
  assert C.sizeof(_lib.ShardedColumn) == 48
  assert '0.2.0' in lib.hbk_version().decode()


def _refused(rc, *words):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in words:
    assert w in msg, msg


def _gcol(**kw):
  col = _lib.LowpGatherColumn()
  col.table, col.rows, col.dim = FAKE, 100, 16
  col.ids, col.ids_dtype, col.n_ids = FAKE + 0x1000, _lib.INT64, 8
  col.divisor, col.out = 1, FAKE + 0x2000
  for k, v in kw.items():
    setattr(col, k, v)
  return col


@pytest.mark.parametrize('kw,words', [
  (dict(dim=0), ('column 0', 'dim')),
  (dict(dim=260), ('dim 260',)),
  (dict(dim=72, table=FAKE + 2), ('dim 72', '64 otherwise')),
  (dict(dim=72, out=FAKE + 0x2002), ('dim 72',)),
  (dict(dim=72, out_stride=73), ('dim 72',)),
  (dict(ids_dtype=_lib.FLOAT), ('int32 or int64',)),
  (dict(rows=-1), ('negative',)),
  (dict(n_ids=-1), ('negative',)),
  (dict(n_ids=1 << 31), ('2^31',)),
  (dict(bucket=-1), ('bucket',)),
  (dict(divisor=0), ('divisor',)),
  (dict(out_stride=8), ('out_stride',)),
  (dict(table=FAKE + 1), ('2-byte aligned',)),
  (dict(out=FAKE + 0x2001), ('2-byte aligned',)),
  (dict(table=0), ('table is NULL',)),
  (dict(out=0), ('out is NULL',)),
  (dict(ids=0), ('ids is NULL',)),
])
def test_gather_rows_refusals_precede_any_launch(kw, words):
  cols = (_lib.LowpGatherColumn * 2)(_gcol(n_ids=0), _gcol(**kw))
  rc = _lib.lib().hbk_lowp_gather_rows_n(2, cols, None)
  _refused(rc, 'lowp_gather_rows_n', 'column 1', *[w for w in words if w != 'column 0'])


def test_gather_rows_trivial_calls():
  lib = _lib.lib()
  assert lib.hbk_lowp_gather_rows_n(0, None, None) == _lib.OK
  _refused(lib.hbk_lowp_gather_rows_n(-1, None, None), 'n_cols')
  _refused(lib.hbk_lowp_gather_rows_n(1, None, None), 'cols is NULL')
  # a column without ids needs no buffers
  cols = (_lib.LowpGatherColumn * 1)(_gcol(n_ids=0, table=0, out=0, ids=0))
  assert lib.hbk_lowp_gather_rows_n(1, cols, None) == _lib.OK


def _rcol(**kw):
  col = _lib.LowpLookupRunsColumn()
  c = col.col
  c.table, c.table_dtype, c.rows, c.dim = FAKE, _lib.LOWP_BF16, 100, 16
  c.ids, c.ids_dtype, c.n_ids, c.n_segments = FAKE + 0x1000, _lib.INT32, 8, 8
  c.divisor, c.combiner, c.out = 1, _lib.COMBINER_SUM, FAKE + 0x2000
  col.run_start, col.run_base, col.n_runs = FAKE + 0x3000, FAKE + 0x4000, 2
  for k, v in kw.items():
    setattr(col if k in ('run_start', 'run_base', 'n_runs') else c, k, v)
  return col


@pytest.mark.parametrize('kw,words', [
  (dict(n_runs=0), ('segmented-table',)),
  (dict(run_start=0), ('segmented-table',)),
  (dict(run_base=0), ('segmented-table',)),
  (dict(table_dtype=0), ('table_dtype',)),
  (dict(table_dtype=_lib.HALF), ('table_dtype',)),
  (dict(dim=0), ('dim',)),
  (dict(dim=260), ('dim 260',)),
  (dict(dim=72, table=FAKE + 2), ('dim 72',)),
  (dict(combiner=5), ('combiner',)),
  (dict(chunk_elems=3), ('chunk_elems',)),
  (dict(n_segments=9), ('n_segments',)),
  (dict(out_stride=8), ('out_stride',)),
  (dict(divisor=0), ('divisor',)),
  (dict(out=0), ('out is NULL',)),
])
def test_lookup_fwd_runs_refusals_precede_any_launch(kw, words):
  cols = (_lib.LowpLookupRunsColumn * 1)(_rcol(**kw))
  _refused(_lib.lib().hbk_lowp_lookup_fwd_runs(1, cols, None), 'lowp_lookup_fwd_runs', 'column 0', *words)
  assert _lib.lib().hbk_lowp_lookup_fwd_runs(0, None, None) == _lib.OK


def test_set_table_dtypes_needs_a_plan():
  _refused(_lib.lib().hbk_sharded_set_table_dtypes(None, None, 0), 'sharded_set_table_dtypes', 'plan is NULL')


# ---- Python ----------------------------------------------------------------------------------------------------------
class _TwoRanks:
  world_size, rank = 2, 1


def test_driver_refusals_without_a_gpu():
  from hybridbackend_amd.embedding import LowpShardedGroupLookup
  from hybridbackend_amd.embedding.lowp import rank_seed
  bad = _lib.InvalidArgumentError
  with pytest.raises(bad, match='bfloat16 or torch.float16'):
    LowpShardedGroupLookup([torch.zeros(4, 4)], _TwoRanks())                      # fp32 shards, wherever they live
  with pytest.raises(_lib.HbkError, match='must live in HBM'):
    LowpShardedGroupLookup([torch.zeros(4, 4, dtype=torch.bfloat16)], _TwoRanks())
  for kw, word in ((dict(max_norms=[1.0]), 'max_norms is not supported'),
                   (dict(max_norms=2.0), 'max_norms is not supported'),
                   (dict(weight_grads=True), 'weight_grads is not supported'),
                   (dict(wire_dtype=torch.float16), 'wire_dtype is not supported'),
                   (dict(hot_rows=True), 'hot_rows is not supported'),
                   (dict(hot_rows='auto'), 'hot_rows is not supported'),
                   (dict(wire='half'), "wire must be 'table' or 'float'"),
                   (dict(rounding='up'), "'nearest' or 'stochastic'"),
                   (dict(seed=-1), 'seed')):
    with pytest.raises(bad, match=word):
      LowpShardedGroupLookup([], _TwoRanks(), **kw)
  drv = LowpShardedGroupLookup.__new__(LowpShardedGroupLookup)
  with pytest.raises(_lib.HbkError, match='p2p_bind is not supported'):
    drv.p2p_bind([])
  with pytest.raises(bad, match='weight_grads is not supported'):
    drv.backward([], weight_grads=True)
  with pytest.raises(bad, match='weight_grads is not supported'):
    drv.backward([], weight_grads=[True])
  with pytest.raises(bad, match='emit=False needs apply_lr'):
    drv.backward([], emit=False)
  with pytest.raises(_lib.HbkError, match='no separate phase methods'):
    drv.partition([])
  # rank k rounds with (seed + 0x9E3779B9 * k) mod 2^32
  assert rank_seed(7, 0) == 7 and rank_seed(7, 1) == 7 + 0x9E3779B9
  assert rank_seed(0xFFFFFFFF, 3) == (0xFFFFFFFF + 3 * 0x9E3779B9) % (1 << 32)
  assert '0x9E3779B9' in LowpShardedGroupLookup.__doc__ and '0x9E3779B9 * k' in HEADER
  assert hb.embedding.LowpShardedGroupLookup is LowpShardedGroupLookup


def test_layer_refusals_without_a_gpu():
  bad = _lib.InvalidArgumentError
  EC, DF = hb.feature_column.EmbeddingColumn, hb.feature_column.DenseFeatures
  cols = [EC('a', 100, 8), EC('b', 100, 16)]
  # without lowp_sharded the refusal stands, word for word
  with pytest.raises(bad, match='16-bit tables are kept on one rank only, the layer spans 2 '
                                r'\(sharded and replicated-at-W>1 tables stay fp32\)'):
    DF(cols, 'cpu', coll=_TwoRanks(), table_dtype=torch.bfloat16)
  with pytest.raises(bad, match='one rank only'):
    DF(cols, 'cpu', coll=_TwoRanks(), table_dtype=torch.bfloat16, lowp_sharded=False)
  # with it, what 16-bit tables cannot do is still named
  kw = dict(coll=_TwoRanks(), table_dtype=torch.bfloat16, lowp_sharded=True)
  with pytest.raises(bad, match="'h' is hash-keyed"):
    DF(cols + [hb.feature_column.HashEmbeddingColumn('h', 64, 8)], 'cpu', **kw)
  with pytest.raises(bad, match="'c' has max_norm"):
    DF(cols + [EC('c', 100, 8, max_norm=1.0)], 'cpu', **kw)
  with pytest.raises(bad, match="'w'.*cannot be addressed in place"):
    DF([EC('a', 100, 3), EC('w', 100, 128)], 'cpu', **kw)
  with pytest.raises(bad, match='bfloat16 tables only'):
    DF(cols, 'cpu', coll=_TwoRanks(), table_dtype=torch.float16, table_rounding='stochastic', lowp_sharded=True)
  with pytest.raises(bad, match='table_dtype'):
    DF(cols, 'cpu', coll=_TwoRanks(), table_dtype=torch.float32, lowp_sharded=True)
