"""Sequence lookups at the C ABI and in Python's argument handling, without a GPU: the two entries exist
beside unchanged structs and version, every refused argument is refused before any device work with the
reason named, and the numpy restatement the GPU tests compare with reproduces the hand-derived golden
case."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import sequence as _seq
from tests.support import sequence_ref as ref

FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it
FAKE2 = 0x7f0000101000


def test_symbols_version_and_struct_layouts_unchanged():
  lib = _lib.lib()
  for name in ('hbk_group_lookup_fwd_sequence', 'hbk_sequence_row_grid_n'):
    assert hasattr(lib, name), name
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  assert hb.__version__ == '0.2.0'
  assert C.sizeof(_lib.LookupColumn) == 128
  assert C.sizeof(_lib.LookupGradColumn) == 160
  assert C.sizeof(_lib.StitchGradColumn) == 88
  assert C.sizeof(_lib.Sequence) == 32      # hbk_sequence_t: two int32, an int64, two pointers


def _col(**kw):
  col = _lib.LookupColumn()
  col.table, col.rows, col.dim = FAKE, 100, 16
  col.ids_dtype, col.ids, col.n_ids, col.n_segments = _lib.INT64, FAKE, 8, 8
  col.divisor, col.combiner, col.out = 1, _lib.COMBINER_SUM, FAKE2
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _seqs(*max_lens, **kw):
  arr = (_lib.Sequence * len(max_lens))()
  for q, t in zip(arr, max_lens):
    q.max_len, q.lengths, q.row_grid = t, FAKE, FAKE2
    for k, v in kw.items():
      setattr(q, k, v)
  return arr


def _refused(rc, *words):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in words:
    assert w in msg, msg


def _both(cols, seqs, *words):
  """The fused entry and the grid entry refuse alike."""
  lib = _lib.lib()
  n = len(cols)
  _refused(lib.hbk_group_lookup_fwd_sequence(n, cols, seqs, None, None), 'group_lookup_fwd_sequence', *words)
  _refused(lib.hbk_sequence_row_grid_n(n, cols, seqs, None), 'sequence_row_grid_n', *words)


@pytest.mark.parametrize('bad', [0, -3])
def test_refuses_max_len_below_one(bad):
  cols = (_lib.LookupColumn * 2)(_col(), _col())
  _both(cols, _seqs(4, bad), 'column 1', 'max_len')


def test_refuses_null_seq():
  cols = (_lib.LookupColumn * 1)(_col())
  _both(cols, None, 'seq is NULL')


@pytest.mark.parametrize('field,kw', [('id_weights', dict(id_weights=FAKE)),
                                      ('out_slots', dict(out_slots=FAKE)),
                                      ('half_io', dict(half_io=1)),
                                      ('n_runs', dict(n_runs=1, run_start=FAKE, run_base=FAKE2))])
def test_refuses_what_sequence_columns_do_not_take(field, kw):
  cols = (_lib.LookupColumn * 2)(_col(), _col(**kw))
  _both(cols, _seqs(4, 4), 'column 1', field)


@pytest.mark.parametrize('bad', [-1.0, float('nan'), float('inf')])
def test_refuses_bad_max_norms(bad):
  cols = (_lib.LookupColumn * 2)(_col(), _col())
  norms = (C.c_float * 2)(1.0, bad)
  _refused(_lib.lib().hbk_group_lookup_fwd_sequence(2, cols, _seqs(4, 4), norms, None), 'column 1', 'max_norm')


def test_refuses_a_wide_row_at_a_misaligned_output():
  lib = _lib.lib()
  cols = (_lib.LookupColumn * 1)(_col(dim=65))
  _refused(lib.hbk_group_lookup_fwd_sequence(1, cols, _seqs(4), None, None), 'dim 65', '64 lanes')
  cols = (_lib.LookupColumn * 1)(_col(dim=128, out=FAKE2 + 4))
  _refused(lib.hbk_group_lookup_fwd_sequence(1, cols, _seqs(4), None, None), 'dim 128', '64 lanes')
  # a sample stride below max_len * dim
  cols = (_lib.LookupColumn * 1)(_col(out_stride=63))
  _refused(lib.hbk_group_lookup_fwd_sequence(1, cols, _seqs(4), None, None), 'out_stride')


def test_refuses_two_to_the_31_positions():
  b = 1 << 20
  cols = (_lib.LookupColumn * 1)(_col(n_ids=b, n_segments=b))
  _both(cols, _seqs(1 << 11), 'column 0', '2^31')


def test_no_columns_is_ok():
  lib = _lib.lib()
  assert lib.hbk_group_lookup_fwd_sequence(0, None, None, None, None) == _lib.OK
  assert lib.hbk_sequence_row_grid_n(0, None, None, None) == _lib.OK


# ---- Python argument handling ---------------------------------------------------------------------------
def test_per_column_values():
  assert _seq.check_sequence_args(2, None, 5, None) == ([0, 0], [5, 5], [None, None])
  assert _seq.check_sequence_args(2, [7, 0], [5, 3], [6, None], rows=[7, 9]) == ([7, 0], [5, 3], [6, None])
  assert _seq.check_sequence_args(2, [7, 0], 4, 6, rows=[7, 9]) == ([7, 0], [4, 4], [6, 6])
  for kw in (dict(max_lens=[5]), dict(max_lens=[5, 3, 1]), dict(max_lens=5, pad_ids=[1]),
             dict(max_lens=5, pad_ids=[1, 2, 3]), dict(max_lens=None), dict(max_lens=0), dict(max_lens=[5, 0]),
             dict(max_lens=2.5), dict(max_lens=True), dict(max_lens=5, pad_ids=1.0)):
    with pytest.raises(_lib.InvalidArgumentError):
      _seq.check_sequence_args(2, [7, 0], kw.get('max_lens'), kw.get('pad_ids'), rows=[7, 9])
  with pytest.raises(_lib.InvalidArgumentError):
    _seq.check_sequence_args(2, [7], 5, None)


@pytest.mark.parametrize('buckets,rows,pad', [([7], [100], 7), ([7], [100], -1), ([0], [9], 9), ([0], [9], -2),
                                              ([7], None, 7), ([0], None, -1)])
def test_pad_id_out_of_range(buckets, rows, pad):
  with pytest.raises(_lib.InvalidArgumentError, match='pad_id'):
    _seq.check_sequence_args(1, buckets, 4, pad, rows=rows)


def test_pad_id_in_range():
  assert _seq.check_sequence_args(1, [7], 4, 6, rows=[100])[2] == [6]
  assert _seq.check_sequence_args(1, [0], 4, 8, rows=[9])[2] == [8]
  assert _seq.check_sequence_args(1, [0], 4, 10 ** 12)[2] == [10 ** 12]   # rows not known: the sign only


def test_sequence_column_arguments():
  fc = hb.feature_column
  col = fc.SequenceEmbeddingColumn('hist', 1000, 16, 50, pad_id=0, max_norm=2.0, dedup=True)
  assert (col.key, col.num_buckets, col.dimension, col.max_len, col.pad_id, col.max_norm, col.dedup) == \
      ('hist', 1000, 16, 50, 0, 2.0, True)
  for kw in (dict(max_len=0), dict(max_len=5, pad_id=1000), dict(max_len=5, pad_id=-1),
             dict(max_len=5, max_norm=-1.0)):
    with pytest.raises(_lib.InvalidArgumentError):
      fc.SequenceEmbeddingColumn('hist', 1000, 16, **kw)
  with pytest.raises(_lib.InvalidArgumentError):
    fc.SequenceEmbeddingColumn('hist', 0, 16, 5)


class _World:
  """What SequenceFeatures reads of a communicator before it builds anything on it."""
  world_size, rank = 3, 0


def test_sharded_sequence_column_requires_a_pad_id():
  fc = hb.feature_column
  made = []

  def init(col, rows, dev):
    import torch
    made.append((col.key, rows))
    return torch.zeros(rows, col.dimension)
  big = fc.SequenceEmbeddingColumn('big', 30000, 8, 5)                # sharded at W = 3, no pad_id
  small = fc.SequenceEmbeddingColumn('small', 2, 8, 5)                # replicated: zero padding is fine
  with pytest.raises(_lib.InvalidArgumentError, match='requires a pad_id') as e:
    fc.SequenceFeatures([small, big], 'cpu', coll=_World(), batch_size=4, init=init)
  assert "'big'" in str(e.value) and 'sharded' in str(e.value)
  assert made == [('small', 2), ('big', 10000)]                        # (the rule did shard it)


# ---- the restatement and the golden case ---------------------------------------------------------------
def _golden():
  root = os.path.dirname(os.path.abspath(__file__))
  with open(os.path.join(root, 'golden', 'sequence_lookup.json')) as f:
    return json.load(f)


@pytest.mark.parametrize('case', ['no_pad', 'pad'])
def test_restatement_reproduces_the_golden_case(case):
  g = _golden()
  assert 'hand-derived' in g['source']
  want = g[case]
  for dtype in (np.int32, np.int64):
    grid, lengths = ref.grid_ref(np.asarray(g['ids'], dtype), np.asarray(g['row_splits'], np.int32),
                                 g['bucket'], g['max_len'], want['pad_id'])
    assert grid.dtype == np.int64 and lengths.dtype == np.int32
    assert grid.tolist() == want['grid']
    assert lengths.tolist() == g['lengths']
    assert ref.rows_ref(grid, g['rows']).tolist() == want['gathered_rows']
  table = np.arange(g['rows'] * 3, dtype=np.float32).reshape(g['rows'], 3) + 1
  out = ref.forward_ref(table, grid, g['max_len'])
  assert out.shape == (5, 3, 3) and out.dtype == np.float32
  for p, r in enumerate(want['gathered_rows']):
    np.testing.assert_array_equal(out.reshape(-1, 3)[p], table[r] if r >= 0 else np.zeros(3, np.float32))
  # the gradient: ones scattered over the grid count every row's positions
  u, s, mag = ref.grad_ref(grid, np.ones((5, 3, 3)), g['rows'])
  rows = [r for r in want['gathered_rows'] if r >= 0]
  assert u.tolist() == sorted(set(rows))
  assert s[:, 0].tolist() == [rows.count(r) for r in u.tolist()]
  np.testing.assert_array_equal(s, mag)
  u32, s32 = ref.grad_seq32(grid, np.ones((5, 3, 3), np.float32), g['rows'])
  assert u32.tolist() == u.tolist()
  np.testing.assert_array_equal(s32, s.astype(np.float32))
  # row 2 is named by a truncated id only: present with pad_id = 2 alone
  assert (2 in u.tolist()) == (case == 'pad')


def test_restatement_edge_cases():
  # no bucket: ids >= rows stay in the grid (a zero row), negative ones are -1
  grid, lengths = ref.grid_ref(np.array([5, -1, 12, 3]), None, 0, 2)
  assert grid.tolist() == [5, -1, -1, -1, 12, -1, 3, -1] and lengths.tolist() == [1, 1, 1, 1]
  assert ref.rows_ref(grid, 10).tolist() == [5, -1, -1, -1, -1, -1, 3, -1]
  # no ids at all, three samples
  grid, lengths = ref.grid_ref(np.zeros(0, np.int64), np.zeros(4, np.int32), 7, 2, pad_id=9)
  assert grid.tolist() == [2] * 6 and lengths.tolist() == [0, 0, 0]
  # a divisor: row = grid // divisor
  assert ref.rows_ref(np.array([7, 8, -1, 30]), 4, divisor=3).tolist() == [2, 2, -1, -1]
