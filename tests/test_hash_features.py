"""Hash-keyed feature columns without a GPU: what the columns refuse, the raw-id grid entry at the C ABI
(hbk_sequence_id_grid_n: present beside an unchanged version, every refusal made before any device work), the
PerRank wrapper of the saver, and the variables() of a layer without hash columns."""
import ctypes as C
import os
import re
import threading

import pytest
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd import feature_column as fc
from hybridbackend_amd.training.saver import PerRank, Saver, load_full

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
INT64_MIN = -2 ** 63


# ---- columns ----------------------------------------------------------------------------------------------
def test_hash_column_keeps_its_arguments():
  col = fc.HashEmbeddingColumn('item', 1000, 16, combiner='sum', max_norm=2.0, dedup=True, slab_size=16, seed=7,
                               expiring=True, min_freq=2)
  assert (col.key, col.capacity, col.dimension, col.combiner, col.dedup) == ('item', 1000, 16, 'sum', True)
  assert col.max_norm == 2.0 and col.expiring and col.weight_feature_key is None
  assert col.table_args['slab_size'] == 16 and col.table_args['seed'] == 7 and col.table_args['min_freq'] == 2
  # one rank: the capacity as given; W ranks: ceil(capacity / W) rounded up to whole slabs
  assert col.local_capacity(1) == 1000
  assert col.local_capacity(2) == 512 and col.local_capacity(3) == 336 and col.local_capacity(7) == 144


@pytest.mark.parametrize('kw,text', [
  (dict(capacity=4), 'below one slab'),
  (dict(slab_size=65), 'slab_size must be in [1, 64]'),
  (dict(dimension=0), 'dim must be >= 1'),
  (dict(init_scale=float('inf')), 'init_scale must be finite'),
  (dict(min_freq=-1), 'min_freq must be in'),
  (dict(min_freq=2, sketch_depth=9), 'sketch_depth must be in'),
  (dict(min_freq=2, sketch_width=0), 'sketch_width must be in'),
  (dict(combiner='max'), 'combiner must be one of'),
  (dict(max_norm=-1.0), 'max_norm'),
])
def test_hash_column_refusals_are_the_tables(kw, text):
  args = dict(key='k', capacity=64, dimension=4)
  args.update(kw)
  with pytest.raises(_lib.InvalidArgumentError) as e:
    fc.HashEmbeddingColumn(**args)
  assert text in str(e.value)


def test_hash_sequence_column_pad_id_is_a_raw_id():
  col = fc.HashSequenceEmbeddingColumn('h', 64, 4, max_len=5, pad_id=-7)
  assert (col.max_len, col.pad_id) == (5, -7)
  assert fc.HashSequenceEmbeddingColumn('h', 64, 4, 5, pad_id=INT64_MIN + 1).pad_id == INT64_MIN + 1
  assert fc.HashSequenceEmbeddingColumn('h', 64, 4, 5).pad_id is None
  for kw, text in [(dict(max_len=0), 'max_len of column 0 must be in [1, 2^31)'),
                   (dict(max_len=3, pad_id=INT64_MIN), 'sentinel of the table'),
                   (dict(max_len=3, pad_id=INT64_MIN + 1, expiring=True), 'sentinel of the table'),
                   (dict(max_len=3, pad_id=2 ** 63), 'must be an int64'),
                   (dict(max_len=3, capacity=4), 'below one slab')]:
    args = dict(key='h', capacity=64, dimension=4)
    args.update(kw)
    with pytest.raises(_lib.InvalidArgumentError) as e:
      fc.HashSequenceEmbeddingColumn(**args)
    assert text in str(e.value)


class _World:
  """What a layer reads of a communicator before it builds a sharded plan."""

  def __init__(self, world_size, rank=0):
    self.world_size, self.rank = world_size, rank


def test_layers_refuse_by_name_what_a_sharded_hash_column_cannot_do():
  # (both refusals come before any table or plan is asked of the device... the tables are made first, so the
  # layer is built on the CPU device here: a HashTable's tensors are plain torch tensors)
  col = fc.HashEmbeddingColumn('item', 64, 4, weight_feature_key='item_w')
  with pytest.raises(_lib.InvalidArgumentError) as e:
    fc.DenseFeatures([col], 'cpu', coll=_World(2))
  assert "'item'" in str(e.value) and "'item_w'" in str(e.value) and 'refuses weights' in str(e.value)
  seq = fc.HashSequenceEmbeddingColumn('hist', 64, 4, max_len=3)
  with pytest.raises(_lib.InvalidArgumentError) as e:
    fc.SequenceFeatures([seq], 'cpu', coll=_World(2))
  assert "'hist'" in str(e.value) and 'requires a pad_id' in str(e.value) and 'every int64 is a key' in str(e.value)


# ---- the new entry at the C ABI ---------------------------------------------------------------------------
def test_symbol_header_prototype_and_version():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_sequence_id_grid_n')
  f = lib.hbk_sequence_id_grid_n
  assert f.restype is C.c_int and f.argtypes == [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  proto = re.search(r'int hbk_sequence_id_grid_n\((.*?)\);', HEADER, flags=re.S).group(1)
  assert re.sub(r'\s+', ' ', proto) == ('int32_t n_cols, const hbk_lookup_column_t* cols, '
                                        'const hbk_sequence_t* seq, hbk_stream_t stream')
  assert C.sizeof(_lib.Sequence) == 32   # the struct is the one of hbk_sequence_row_grid_n
  from hybridbackend_amd import embedding
  assert embedding.sequence_id_grid is embedding.sequence.sequence_id_grid


def _grid_call(null_seq=False, **kw):
  col = (_lib.LookupColumn * 1)()
  seq = (_lib.Sequence * 1)()
  col[0].ids, col[0].ids_dtype, col[0].n_ids = FAKE, _lib.INT64, 100
  col[0].row_splits, col[0].n_segments = FAKE + 0x10000, 37
  seq[0].max_len, seq[0].has_pad, seq[0].pad_id = 7, 1, -5
  seq[0].lengths, seq[0].row_grid = FAKE + 0x20000, FAKE + 0x30000
  for k, v in kw.items():
    setattr(col[0] if hasattr(col[0], k) else seq[0], k, v)
  status = _lib.lib().hbk_sequence_id_grid_n(1, col, None if null_seq else seq, None)
  return status, _lib.lib().hbk_last_error().decode()


@pytest.mark.parametrize('kw,text', [
  (dict(null_seq=True), 'seq is NULL'),
  (dict(has_pad=0), 'has_pad is 0'),
  (dict(row_grid=None), 'row_grid is NULL'),
  (dict(row_grid=None, n_segments=0), 'row_grid is NULL'),      # whatever the batch
  (dict(max_len=0), 'max_len must be >= 1'),
  (dict(n_segments=2 ** 28, max_len=8), 'must stay below 2^31'),
])
def test_refusals_come_before_any_device_work(kw, text):
  status, msg = _grid_call(**kw)
  assert status == _lib.INVALID_ARGUMENT and text in msg and 'sequence_id_grid_n' in msg


def test_no_columns_is_no_work():
  assert _lib.lib().hbk_sequence_id_grid_n(0, None, None, None) == _lib.OK


def test_python_wrapper_requires_a_pad_id_per_column():
  from hybridbackend_amd.embedding import sequence_id_grid
  ids = [torch.zeros(3, dtype=torch.int64)]
  for kw, text in [(dict(max_lens=2, pad_ids=None), 'pad_id of column 0 is required'),
                   (dict(max_lens=None, pad_ids=1), 'max_lens is required'),
                   (dict(max_lens=0, pad_ids=1), 'max_len of column 0 must be in'),
                   (dict(max_lens=2, pad_ids=2 ** 63), 'must be an int64')]:
    with pytest.raises(_lib.InvalidArgumentError) as e:
      sequence_id_grid(ids, None, **kw)
    assert text in str(e.value)


# ---- PerRank through the Saver ----------------------------------------------------------------------------
def test_per_rank_round_trips_with_two_in_process_ranks(tmp_path):
  prefix = str(tmp_path / 'ckpt')
  world = 2
  barrier = threading.Barrier(world)
  own = [torch.arange(3 + r, dtype=torch.int64) * (r + 1) - 2 ** 40 for r in range(world)]
  rows = [torch.full((3 + r, 2), float(r + 1)) for r in range(world)]
  plain = torch.tensor([1.0, 2.0])
  errors = []

  def rank(r):
    try:
      Saver(r, world, barrier.wait).save(prefix, {
        f't/part_{r}_of_{world}/items/keys': PerRank(own[r]),
        f't/part_{r}_of_{world}/items/rows': PerRank(rows[r]),
        'plain': plain if r == 0 else torch.zeros(2)})   # (a plain tensor: rank 0's alone, as before)
    except Exception as e:  # pylint: disable=broad-except
      errors.append(repr(e))
      barrier.abort()

  threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=30)
  assert not errors, errors
  for r in range(world):
    assert load_full(prefix, f't/part_{r}_of_{world}/items/keys').tolist() == own[r].tolist()
    assert load_full(prefix, f't/part_{r}_of_{world}/items/rows').tolist() == rows[r].tolist()
  assert load_full(prefix, 'plain').tolist() == [1.0, 2.0]
  # restored whole by the name it was saved under, at any world size
  got = {f't/part_1_of_{world}/items/keys': PerRank(torch.zeros(4, dtype=torch.int64)), 'plain': torch.zeros(2)}
  Saver().restore(prefix, got)
  assert got[f't/part_1_of_{world}/items/keys'].tensor.tolist() == own[1].tolist()
  assert got['plain'].tolist() == [1.0, 2.0]


def test_restore_refuses_an_incomplete_part_set_before_any_import(tmp_path):
  prefix = str(tmp_path / 'ckpt')
  base = 'h_embedding/embedding_weights/part_0_of_2/items/'
  Saver().save(prefix, {base + 'keys': torch.arange(3, dtype=torch.int64), base + 'rows': torch.ones(3, 4)})
  layer = fc.DenseFeatures.__new__(fc.DenseFeatures)
  layer._init_tables([fc.HashEmbeddingColumn('h', 64, 4)], 'cpu', None, 0, None, None, None, None, None)   # pylint: disable=protected-access
  with pytest.raises(_lib.InvalidArgumentError) as e:
    layer.restore(prefix)
  assert 'parts 0 .. W-1 of one world size' in str(e.value) and '/part_0_of_2' in str(e.value)
  with pytest.raises(ValueError):
    layer.restore(prefix, layout='diagonal')


# ---- a layer without hash columns is what it was ----------------------------------------------------------
def test_variables_of_a_hash_free_layer_has_exactly_todays_keys():
  cols = [fc.EmbeddingColumn('a', 10, 4), fc.EmbeddingColumn('b', 7, 3)]
  layer = fc.DenseFeatures.__new__(fc.DenseFeatures)
  layer._init_tables(cols, 'cpu', None, 0, None, 0.1, 'adam', None, None)   # pylint: disable=protected-access
  assert layer.hash_tables == [None, None]
  assert sorted(layer.variables()) == sorted(
    [f'{k}_embedding/embedding_weights{s}' for k in 'ab' for s in ('', '/Adagrad', '/Adam', '/Adam_1')] +
    ['beta1_power', 'beta2_power'])
  # and with a hash column beside them, the hash column is in none of the names
  mixed = fc.DenseFeatures.__new__(fc.DenseFeatures)
  mixed._init_tables(cols + [fc.HashEmbeddingColumn('h', 64, 4)], 'cpu', None, 0, None, 0.1, None, None, None)   # pylint: disable=protected-access
  assert sorted(mixed.variables()) == sorted(
    f'{k}_embedding/embedding_weights{s}' for k in 'ab' for s in ('', '/Adagrad'))
  # a checkpoint that holds a bucketed variable under a hash column's name is refused by name
  import tempfile
  with tempfile.TemporaryDirectory() as d:
    prefix = os.path.join(d, 'ckpt')
    layer.save(prefix)
    other = fc.DenseFeatures.__new__(fc.DenseFeatures)
    other._init_tables([fc.HashEmbeddingColumn('a', 64, 4), cols[1]], 'cpu', None, 0, None, 0.1, None, None, None)   # pylint: disable=protected-access
    with pytest.raises(_lib.InvalidArgumentError) as e:
      other.restore(prefix)
    assert 'a_embedding/embedding_weights' in str(e.value) and 'holds a bucketed variable' in str(e.value)
  assert mixed.hash_tables[2].capacity == 64 and mixed.weights[2] is mixed.hash_tables[2].table
  assert tuple(mixed.accums[2].shape) == (64, 4) and float(mixed.accums[2][0, 0]) == pytest.approx(0.1)
