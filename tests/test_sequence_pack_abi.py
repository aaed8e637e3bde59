"""hbk_sequence_pack_n without a GPU: the two symbols exist beside an unchanged version and unchanged structs,
every refused argument is refused before any device work with the column named, the workspace query grows
with B, the numpy restatement the GPU tests compare with reproduces hand-written cases, and SequenceFeatures
with the default argument refuses a sharded column without a pad id exactly as before."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from tests.support import sequence_pack_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
FAKE2 = 0x7f0000101000
WS = 1 << 20


def test_symbols_prototypes_structs_and_version():
  lib = _lib.lib()
  f = lib.hbk_sequence_pack_n
  assert f.restype is C.c_int
  assert f.argtypes == [C.c_int32] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]
  w = lib.hbk_sequence_pack_workspace_bytes
  assert w.restype is C.c_size_t and w.argtypes == [C.c_int32, C.c_void_p]
  proto = re.search(r'int hbk_sequence_pack_n\((.*?)\);', HEADER, flags=re.S).group(1)
  assert len(proto.split(',')) == 7
  assert re.search(r'size_t hbk_sequence_pack_workspace_bytes\(int32_t n_cols, const hbk_lookup_column_t\* cols\);',
                   HEADER)
  body = re.search(r'typedef struct \{([^}]*)\} hbk_sequence_pack_t;', HEADER).group(1)
  fields = re.findall(r'(\w+);', body)
  assert fields == [name for name, _ in _lib.SequencePack._fields_]
  assert C.sizeof(_lib.SequencePack) == 40
  # new symbols only: the version and the existing structs are those of 0.2.0
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  assert C.sizeof(_lib.LookupColumn) == 128 and C.sizeof(_lib.Sequence) == 32
  assert callable(hb.embedding.sequence_pack) and callable(hb.embedding.ShardedSequenceLookup)
  # the header carries the formulas and the bounds rule
  for text in ('pos_splits[b * T + t] = sample_splits[b] + min(t, l_b)', 'a negative value counts as 0',
               'outside [0, n_ids)', 'at or past total'):
    assert text in HEADER, text


def _col(**kw):
  col = _lib.LookupColumn()
  col.ids_dtype, col.ids, col.n_ids, col.n_segments = _lib.INT64, FAKE, 8, 8
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _seq(max_len=4, **kw):
  q = _lib.Sequence()
  q.max_len, q.lengths = max_len, FAKE
  for k, v in kw.items():
    setattr(q, k, v)
  return q


def _pack(**kw):
  p = _lib.SequencePack()
  p.packed, p.packed_capacity, p.pos_splits, p.sample_splits, p.total = FAKE2, 1 << 20, FAKE2, FAKE2, FAKE2
  for k, v in kw.items():
    setattr(p, k, v)
  return p


def _call(col=None, seq=None, pack=None, workspace=FAKE, workspace_bytes=WS):
  """Two columns, the first in order, the second as given: the refusal must name column 1."""
  cols = (_lib.LookupColumn * 2)(_col(), col if col is not None else _col())
  seqs = (_lib.Sequence * 2)(_seq(), seq if seq is not None else _seq())
  packs = (_lib.SequencePack * 2)(_pack(), pack if pack is not None else _pack())
  rc = _lib.lib().hbk_sequence_pack_n(2, cols, seqs, packs, workspace, workspace_bytes, None)
  return rc, _lib.lib().hbk_last_error().decode()


def _refused(words, **kw):
  rc, msg = _call(**kw)
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('sequence_pack_n', 'column 1') + tuple(words):
    assert w in msg, msg


@pytest.mark.parametrize('bad', [0, -3])
def test_refuses_max_len_below_one(bad):
  _refused(['max_len'], seq=_seq(bad))


def test_refuses_two_to_the_31_positions_or_ids():
  b = 1 << 20
  _refused(['2^31'], col=_col(n_ids=b, n_segments=b), seq=_seq(1 << 11))
  _refused(['2^31'], col=_col(n_ids=1 << 31, n_segments=4, row_splits=FAKE))


def test_refuses_segments_that_are_not_the_ids_without_row_splits():
  _refused(['n_segments', 'row_splits is NULL'], col=_col(n_ids=8, n_segments=7))


@pytest.mark.parametrize('which', ['lengths', 'packed', 'pos_splits', 'sample_splits', 'total'])
def test_refuses_a_null_output(which):
  if which == 'lengths':
    _refused(['NULL output'], seq=_seq(lengths=None))
  else:
    _refused(['NULL output'], pack=_pack(**{which: None}))
  # also with B == 0: all five are written or named
  if which != 'lengths':
    _refused(['NULL output'], col=_col(n_ids=0, n_segments=0), pack=_pack(**{which: None}))


def test_refuses_a_packed_capacity_below_its_bound():
  # min(n_ids, B * T): 8 ids in 3 samples of T = 2 -> 6; 8 ids, one per sample, T = 4 -> 8
  _refused(['packed_capacity 5', '= 6'], col=_col(n_ids=8, n_segments=3, row_splits=FAKE), seq=_seq(2),
           pack=_pack(packed_capacity=5))
  _refused(['packed_capacity 7', '= 8'], pack=_pack(packed_capacity=7))
  rc, msg = _call(col=_col(n_ids=8, n_segments=3, row_splits=FAKE), seq=_seq(2), pack=_pack(packed_capacity=6),
                  workspace_bytes=4)
  assert rc == _lib.INVALID_ARGUMENT and 'workspace' in msg     # (the capacity passed: the next check speaks)


def test_refuses_a_pad_id():
  _refused(['has_pad', 'a pad id belongs to the grid ops'], seq=_seq(has_pad=1, pad_id=3))


def test_refuses_a_small_workspace_and_states_the_size():
  cols = (_lib.LookupColumn * 2)(_col(), _col(n_ids=600, n_segments=600))
  need = _lib.lib().hbk_sequence_pack_workspace_bytes(2, cols)
  assert need == 4 * (1 + 3)
  _refused([f'{need} bytes are needed'], col=_col(n_ids=600, n_segments=600), workspace_bytes=need - 1)
  rc, msg = _call(col=_col(n_ids=600, n_segments=600), workspace=None, workspace_bytes=need)   # (NULL: column 0's)
  assert rc == _lib.INVALID_ARGUMENT and 'column 0' in msg and f'{need} bytes are needed' in msg


def test_refuses_bad_id_sides():
  _refused(['int32 or int64'], col=_col(ids_dtype=_lib.FLOAT))
  _refused(['NULL buffer'], col=_col(ids=None))
  _refused(['negative size'], col=_col(n_ids=-1, n_segments=-1))
  lib = _lib.lib()
  assert lib.hbk_sequence_pack_n(1, None, None, None, None, 0, None) == _lib.INVALID_ARGUMENT
  assert lib.hbk_sequence_pack_n(-1, None, None, None, None, 0, None) == _lib.INVALID_ARGUMENT


def test_no_columns_is_ok():
  lib = _lib.lib()
  assert lib.hbk_sequence_pack_n(0, None, None, None, None, 0, None) == _lib.OK
  assert lib.hbk_sequence_pack_workspace_bytes(0, None) == 0


def test_workspace_query_is_monotone_in_the_batch():
  lib = _lib.lib()
  last = 0
  for b in (0, 1, 255, 256, 257, 512, 513, 70001, 1 << 20, (1 << 31) - 1):
    cols = (_lib.LookupColumn * 1)(_col(n_ids=b, n_segments=b))
    need = lib.hbk_sequence_pack_workspace_bytes(1, cols)
    assert need >= last, (b, need, last)
    last = need
  assert lib.hbk_sequence_pack_workspace_bytes(1, (_lib.LookupColumn * 1)(_col(n_ids=0, n_segments=0))) == 0
  two = (_lib.LookupColumn * 2)(_col(n_ids=300, n_segments=300), _col(n_ids=300, n_segments=300))
  one = (_lib.LookupColumn * 1)(_col(n_ids=300, n_segments=300))
  assert lib.hbk_sequence_pack_workspace_bytes(2, two) == 2 * lib.hbk_sequence_pack_workspace_bytes(1, one)


def test_python_argument_handling():
  with pytest.raises(_lib.InvalidArgumentError, match='max_lens is required'):
    hb.embedding.sequence_pack([], None, None)
  assert hb.embedding.sequence_pack([], None, 3) == ([], [], [], [])
  import torch
  with pytest.raises(_lib.InvalidArgumentError, match='max_len of column 0'):
    hb.embedding.sequence_pack([torch.zeros(3, dtype=torch.int64)], None, 0)
  with pytest.raises(_lib.HbkError, match='HBM'):     # no CPU fallback
    hb.embedding.sequence_pack([torch.zeros(3, dtype=torch.int64)], None, 2)


# ---- the restatement against hand-written cases -----------------------------------------------------------
def _check(ids, splits, T, packed, pos, lengths, samp):
  for dtype in (np.int32, np.int64):
    got = ref.pack_ref(np.asarray(ids, dtype), None if splits is None else np.asarray(splits, np.int32), T)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int32 and \
        got[3].dtype == np.int32
    assert got[0].tolist() == packed
    assert got[1].tolist() == pos
    assert got[2].tolist() == lengths
    assert got[3].tolist() == samp
    assert got[4] == samp[-1] == pos[-1] == len(packed)


def test_restatement_max_len_one():
  # T = 1: a position per sample; lengths 2, 0, 1 -> one id, none, one id
  _check([10, 11, 12], [0, 2, 2, 3], 1, packed=[10, 12], pos=[0, 1, 1, 2], lengths=[1, 0, 1], samp=[0, 1, 1, 2])


def test_restatement_an_empty_sample_and_one_longer_than_max_len():
  # lengths 2, 0, 5, 1 at T = 3 -> 2, 0, 3, 1; ids 7 and 8 (positions 3, 4 of sample 2) are never read
  ids = [1, -2, 3, 4, 5, 7, 8, 9]
  _check(ids, [0, 2, 2, 7, 8], 3, packed=[1, -2, 3, 4, 5, 9],
         pos=[0, 1, 2, 2, 2, 2, 2, 3, 4, 5, 6, 6, 6], lengths=[2, 0, 3, 1], samp=[0, 2, 2, 5, 6])


def test_restatement_all_samples_empty():
  _check([], [0, 0, 0, 0], 2, packed=[], pos=[0] * 7, lengths=[0, 0, 0], samp=[0, 0, 0, 0])
  _check([], [0], 2, packed=[], pos=[0], lengths=[], samp=[0])


def test_restatement_without_row_splits():
  # one id per sample: the first position of every sample holds it
  _check([5, -6, 7], None, 2, packed=[5, -6, 7], pos=[0, 1, 1, 2, 2, 3, 3], lengths=[1, 1, 1], samp=[0, 1, 2, 3])
  _check([5, -6], None, 1, packed=[5, -6], pos=[0, 1, 2], lengths=[1, 1], samp=[0, 1, 2])


def test_restatement_bounds_rule_and_negative_lengths():
  # row splits that point outside the ids: not read, the element holds 0; a negative length counts as 0
  got = ref.pack_ref(np.asarray([1, 2, 3], np.int64), np.asarray([2, 5, 4, 4], np.int32), 2)
  assert got[0].tolist() == [3, 0] and got[2].tolist() == [2, 0, 0] and got[3].tolist() == [0, 2, 2, 2]
  assert got[1].tolist() == [0, 1, 2, 2, 2, 2, 2]
  # int32 ids are sign-extended
  got = ref.pack_ref(np.asarray([-1, -(2 ** 31)], np.int32), None, 1)
  assert got[0].tolist() == [-1, -(2 ** 31)]


# ---- the layer: the default argument refuses as before ------------------------------------------------------
class _World:
  """What SequenceFeatures reads of a communicator before it builds anything on it."""

  def __init__(self, world_size=3, rank=0):
    self.world_size, self.rank = world_size, rank


def _init(col, rows, dev):
  import torch
  return torch.zeros(rows, col.dimension)


_BUCKETED = ("sequence column 'big': its table is sharded over 3 ranks, and a sharded sequence column requires a "
             'pad_id (the sharded step bucketizes the id grid again, which would turn the -1 of a zero-padded '
             'position into a row; zero padding is for replicated tables)')
_HASHED = ("hash sequence column 'hist': its table is sharded over 2 ranks, and a sharded sequence column requires "
           'a pad_id (the sharded step takes one raw id per position, and among raw ids no value means "nothing": '
           'every int64 is a key; zero padding is for one rank)')


@pytest.mark.parametrize('kw', [dict(), dict(sharded_zero_padding=False)])
def test_default_argument_refuses_a_sharded_column_without_a_pad_id_as_before(kw):
  fc = hb.feature_column
  big = fc.SequenceEmbeddingColumn('big', 30000, 8, 5)
  small = fc.SequenceEmbeddingColumn('small', 2, 8, 5)
  with pytest.raises(_lib.InvalidArgumentError) as e:
    fc.SequenceFeatures([small, big], 'cpu', coll=_World(3), batch_size=4, init=_init, **kw)
  # what it raised before, then the sentence that names the new argument
  assert _BUCKETED in str(e.value)
  assert str(e.value).split(_BUCKETED)[1].startswith('.  SequenceFeatures(..., sharded_zero_padding=True)')
  seq = fc.HashSequenceEmbeddingColumn('hist', 64, 4, max_len=3)
  with pytest.raises(_lib.InvalidArgumentError) as e:
    fc.SequenceFeatures([seq], 'cpu', coll=_World(2), **kw)
  assert _HASHED in str(e.value)
  assert 'sharded_zero_padding=True' in str(e.value).split(_HASHED)[1]


def test_the_argument_is_kept_and_documented():
  fc = hb.feature_column
  assert 'sharded_zero_padding' in fc.SequenceFeatures.__doc__ and 'host read' in fc.SequenceFeatures.__doc__
  assert 'waits on the host once per forward' in ' '.join(hb.embedding.sequence_pack.__doc__.split())
  for word in ('sp_weights', 'p2p_bind', 'PipelinedLookup'):
    assert word in hb.embedding.ShardedSequenceLookup.__doc__
