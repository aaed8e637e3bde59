"""Key-deduplicated features without a GPU: the four symbols exist beside an unchanged version and unchanged
structs, every refused argument is refused before any device work with the column named, the workspace query grows
with the batch, the Python argument handling refuses what it must, and the numpy restatement the GPU tests compare
with reproduces hand-written cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from tests.support import expand_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
FAKE2 = 0x7f0000101000
FAKE3 = 0x7f0000201000
WS = 1 << 20


def test_symbols_prototypes_structs_and_version():
  lib = _lib.lib()
  vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
  f = lib.hbk_expand_rows_n
  assert f.restype is C.c_int and f.argtypes == [i32, vp, vp, i32, i64, i64, vp]
  g = lib.hbk_expand_rows_grad_n
  assert g.restype is C.c_int and g.argtypes == [i32, vp, vp, vp, i64, i64, vp]
  w = lib.hbk_expand_index_workspace_bytes
  assert w.restype is C.c_size_t and w.argtypes == [i64, i64]
  b = lib.hbk_expand_index_build
  assert b.restype is C.c_int and b.argtypes == [vp, i32, i64, i64, vp, vp, vp, vp, C.c_size_t, vp]
  for name, n_args in (('int hbk_expand_rows_n', 7), ('int hbk_expand_rows_grad_n', 7),
                       ('size_t hbk_expand_index_workspace_bytes', 2), ('int hbk_expand_index_build', 10)):
    proto = re.search(re.escape(name) + r'\((.*?)\);', HEADER, flags=re.S).group(1)
    assert len(proto.split(',')) == n_args, name
  body = re.search(r'typedef struct \{([^}]*)\} hbk_expand_column_t;', HEADER).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  assert re.findall(r'(\w+);', body) == [name for name, _ in _lib.ExpandColumn._fields_]
  assert C.sizeof(_lib.ExpandColumn) == 40
  # new symbols only: the version and the existing structs are those of 0.2.0
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  assert C.sizeof(_lib.LookupColumn) == 128 and C.sizeof(_lib.Sequence) == 32 and C.sizeof(_lib.SequencePack) == 40
  assert callable(hb.embedding.expand_rows) and callable(hb.embedding.expand_rows_grad)
  assert callable(hb.embedding.ExpandIndex) and callable(hb.feature_column.DeduplicatedFeatures)
  # the header carries the formulas
  for text in ('out[b, :] = src[idx[b], :]', 'if 0 <= idx[b] < n_keys', 'in ASCENDING b',
               'out[u, :] = src[order[splits[u]], :] + src[order[splits[u] + 1], :] + ...',
               'STARTS FROM ITS FIRST TERM', 'idx == NULL is the identity'):
    assert text in HEADER, text


def _col(**kw):
  col = _lib.ExpandColumn()
  col.src, col.out, col.width = FAKE, FAKE2, 16
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _two(col):
  """Two columns, the first in order, the second as given: the refusal must name column 1."""
  return (_lib.ExpandColumn * 2)(_col(), col if col is not None else _col(out=FAKE3))


def _fwd(col=None, idx=FAKE, idx_dtype=_lib.INT64, n_samples=8, n_keys=4):
  rc = _lib.lib().hbk_expand_rows_n(2, _two(col), idx, idx_dtype, n_samples, n_keys, None)
  return rc, _lib.lib().hbk_last_error().decode()


def _grad(col=None, order=FAKE, splits=FAKE, n_samples=8, n_keys=4):
  rc = _lib.lib().hbk_expand_rows_grad_n(2, _two(col), order, splits, n_samples, n_keys, None)
  return rc, _lib.lib().hbk_last_error().decode()


def _refused(call, who, words, **kw):
  rc, msg = call(**kw)
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in (who,) + tuple(words):
    assert w in msg, msg


BOTH = [(_fwd, 'expand_rows_n'), (_grad, 'expand_rows_grad_n')]


@pytest.mark.parametrize('call,who', BOTH)
def test_refuses_a_null_buffer_with_rows_to_move(call, who):
  _refused(call, who, ['column 1', 'src is NULL'], col=_col(src=None, out=FAKE3))
  _refused(call, who, ['column 1', 'out is NULL'], col=_col(out=None))


@pytest.mark.parametrize('call,who', BOTH)
@pytest.mark.parametrize('bad', [0, -5])
def test_refuses_a_width_below_one(call, who, bad):
  _refused(call, who, ['column 1', 'width'], col=_col(width=bad, out=FAKE3))


@pytest.mark.parametrize('call,who', BOTH)
def test_refuses_a_stride_below_the_width(call, who):
  _refused(call, who, ['column 1', 'src_stride 15', 'width 16'], col=_col(src_stride=15, out=FAKE3))
  _refused(call, who, ['column 1', 'out_stride 3', 'width 16'], col=_col(out_stride=3, out=FAKE3))
  _refused(call, who, ['column 1', 'out_stride -1'], col=_col(out_stride=-1, out=FAKE3))


@pytest.mark.parametrize('call,who', BOTH)
def test_refuses_sizes_outside_31_bits(call, who):
  for kw in (dict(n_samples=-1), dict(n_keys=-1), dict(n_samples=1 << 31), dict(n_keys=1 << 31)):
    _refused(call, who, ['2^31'], **kw)
  lib = _lib.lib()
  for kw in (dict(n_samples=-1, n_keys=4), dict(n_samples=4, n_keys=-1), dict(n_samples=1 << 31, n_keys=4),
             dict(n_samples=4, n_keys=1 << 31)):
    rc = lib.hbk_expand_index_build(FAKE, _lib.INT64, kw['n_samples'], kw['n_keys'], FAKE2, FAKE2, FAKE2, FAKE3,
                                    WS, None)
    assert rc == _lib.INVALID_ARGUMENT and '2^31' in lib.hbk_last_error().decode()
    assert lib.hbk_expand_index_workspace_bytes(kw['n_samples'], kw['n_keys']) == 0


def test_refuses_an_id_dtype_that_is_neither_int32_nor_int64():
  lib = _lib.lib()
  for dtype in (_lib.FLOAT, _lib.UINT64, _lib.INT8, 77):
    rc, msg = _fwd(idx_dtype=dtype)
    assert rc == _lib.INVALID_ARGUMENT and 'int32 or int64' in msg, msg
    rc = lib.hbk_expand_index_build(FAKE, dtype, 8, 4, FAKE2, FAKE2, FAKE2, FAKE3, WS, None)
    assert rc == _lib.INVALID_ARGUMENT and 'int32 or int64' in lib.hbk_last_error().decode()


@pytest.mark.parametrize('call,who', BOTH)
def test_refuses_two_columns_naming_the_same_out(call, who):
  _refused(call, who, ['column 1', 'same out', 'column 0'], col=_col())


def test_refuses_a_small_workspace_and_states_the_size():
  lib = _lib.lib()
  need = lib.hbk_expand_index_workspace_bytes(600, 37)
  assert need >= 600 * (8 + 8 + 4)
  for ws, n in ((FAKE3, need - 1), (None, need), (FAKE3, 0)):
    rc = lib.hbk_expand_index_build(FAKE, _lib.INT32, 600, 37, FAKE2, FAKE2, FAKE2, ws, n, None)
    msg = lib.hbk_last_error().decode()
    assert rc == _lib.INVALID_ARGUMENT and 'expand_index_build' in msg and f'{need} bytes are needed' in msg, msg
  rc = lib.hbk_expand_index_build(None, _lib.INT32, 600, 37, FAKE2, FAKE2, FAKE2, FAKE3, need, None)
  assert rc == _lib.INVALID_ARGUMENT and 'idx is NULL' in lib.hbk_last_error().decode()
  rc = lib.hbk_expand_index_build(FAKE, _lib.INT32, 600, 37, FAKE2, None, FAKE2, FAKE3, need, None)
  assert rc == _lib.INVALID_ARGUMENT and 'splits' in lib.hbk_last_error().decode()
  rc, msg = _grad(splits=None)
  assert rc == _lib.INVALID_ARGUMENT and 'splits is NULL' in msg
  rc, msg = _grad(order=None)
  assert rc == _lib.INVALID_ARGUMENT and 'order is NULL' in msg


def test_nothing_to_do_is_ok():
  lib = _lib.lib()
  assert lib.hbk_expand_rows_n(0, None, None, _lib.INT64, 0, 0, None) == _lib.OK
  assert lib.hbk_expand_rows_n(0, None, FAKE, _lib.INT64, 100, 10, None) == _lib.OK
  assert lib.hbk_expand_rows_grad_n(0, None, FAKE, FAKE, 100, 10, None) == _lib.OK
  # no samples: nothing is read or written, NULL buffers included
  cols = (_lib.ExpandColumn * 1)(_col(src=None, out=None))
  assert lib.hbk_expand_rows_n(1, cols, None, _lib.INT64, 0, 5, None) == _lib.OK
  # no keys: the transpose writes no row
  assert lib.hbk_expand_rows_grad_n(1, cols, None, None, 0, 0, None) == _lib.OK
  assert lib.hbk_expand_rows_n(-1, None, None, _lib.INT64, 0, 0, None) == _lib.INVALID_ARGUMENT
  assert lib.hbk_expand_rows_n(1, None, None, _lib.INT64, 0, 0, None) == _lib.INVALID_ARGUMENT
  assert lib.hbk_expand_index_workspace_bytes(0, 0) == 0
  assert lib.hbk_expand_index_workspace_bytes(0, 1000) == 0


def test_workspace_query_is_monotone_in_the_batch():
  lib = _lib.lib()
  for n_keys in (0, 1, 37, 70001, (1 << 31) - 1):
    last = 0
    for b in (0, 1, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097, 70001, 1 << 20, (1 << 20) + 1, 1 << 24,
              (1 << 31) - 1):
      need = lib.hbk_expand_index_workspace_bytes(b, n_keys)
      assert need >= last and need >= b * 20, (b, n_keys, need, last)
      last = need


def test_python_argument_handling():
  e = hb.embedding
  idx = torch.zeros(3, dtype=torch.int64)
  with pytest.raises(_lib.HbkError, match='HBM'):                 # no CPU fallback
    e.expand_rows(idx, [torch.zeros(2, 4)])
  with pytest.raises(_lib.HbkError, match='HBM'):
    e.ExpandIndex(idx, 2)
  with pytest.raises(_lib.InvalidArgumentError, match='int32 or int64 vector'):
    e.ExpandIndex(torch.zeros(3), 2)
  with pytest.raises(_lib.InvalidArgumentError, match='int32 or int64 vector'):
    e.expand_rows(torch.zeros(3, 2, dtype=torch.int64), [torch.zeros(2, 4)])
  with pytest.raises(_lib.InvalidArgumentError, match='must be an ExpandIndex'):
    e.expand_rows_grad(idx, [torch.zeros(3, 4)])
  assert e.expand_rows(None, []) == []
  meta = torch.zeros(3, dtype=torch.int64, device='meta')   # a device the package has no path for either
  with pytest.raises(_lib.HbkError):
    e.expand_rows(meta, [torch.zeros(2, 4)])


# ---- the restatement against hand-written cases -----------------------------------------------------------
def test_restatement_the_reference_tests_case():
  # key_idx [[0, 1, 0, 1], [0, 0, 1, 1]] of two row groups of two keys each, flattened to global row numbers
  idx = [0, 1, 0, 1, 2, 2, 3, 3]
  src = np.arange(8, dtype=np.float32).reshape(4, 2)
  for dtype in (np.int32, np.int64):
    got = ref.expand_ref(src, np.asarray(idx, dtype))
    assert got.tolist() == [[0, 1], [2, 3], [0, 1], [2, 3], [4, 5], [4, 5], [6, 7], [6, 7]]
    order, splits, invalid = ref.index_ref(np.asarray(idx, dtype), 4)
    assert order.tolist() == [0, 2, 1, 3, 4, 5, 6, 7] and splits.tolist() == [0, 2, 4, 6, 8] and invalid == 0
    assert order.dtype == np.int32 and splits.dtype == np.int32
  g = np.asarray([[1], [2], [4], [8], [16], [32], [64], [128]], np.float32)
  assert ref.grad_ref(g, idx, 4).tolist() == [[5], [10], [48], [192]]


def test_restatement_an_empty_batch():
  src = np.ones((3, 2), np.float32)
  assert ref.expand_ref(src, np.zeros(0, np.int64)).shape == (0, 2)
  order, splits, invalid = ref.index_ref(np.zeros(0, np.int32), 3)
  assert order.tolist() == [] and splits.tolist() == [0, 0, 0, 0] and invalid == 0
  assert ref.grad_ref(np.zeros((0, 2), np.float32), np.zeros(0, np.int64), 3).tolist() == [[0, 0]] * 3
  order, splits, invalid = ref.index_ref(np.zeros(0, np.int32), 0)
  assert order.tolist() == [] and splits.tolist() == [0] and invalid == 0


def test_restatement_a_key_nobody_names():
  idx = [2, 0, 2]
  order, splits, invalid = ref.index_ref(idx, 4)
  assert order.tolist() == [1, 0, 2] and splits.tolist() == [0, 1, 1, 3, 3] and invalid == 0
  g = np.asarray([[1, -1], [2, -2], [3, -3]], np.float32)
  assert ref.grad_ref(g, idx, 4).tolist() == [[2, -2], [0, 0], [4, -4], [0, 0]]


def test_restatement_an_out_of_range_index():
  idx = np.asarray([1, -1, 3, 2 ** 40, 0, 1], np.int64)
  src = np.asarray([[1, 2], [3, 4], [5, 6]], np.int32)
  assert ref.expand_ref(src, idx).tolist() == [[3, 4], [0, 0], [0, 0], [0, 0], [1, 2], [3, 4]]
  order, splits, invalid = ref.index_ref(idx, 3)
  assert order.tolist() == [4, 0, 5, 1, 2, 3] and splits.tolist() == [0, 1, 3, 3] and invalid == 3
  g = np.arange(6, dtype=np.float32).reshape(6, 1) + 1
  assert ref.grad_ref(g, idx, 3).tolist() == [[5], [7], [0]]
  # no keys at all: every forward row is zero, every sample is in no list
  assert ref.expand_ref(np.zeros((0, 2), np.float32), [0, 1]).tolist() == [[0, 0], [0, 0]]
  assert ref.index_ref([0, 1], 0)[2] == 2


def test_restatement_sums_in_order_from_the_first_term():
  # 1e8 + 1 - 1e8 in fp32: in order 0, the other way round 1; and a lone -0 stays -0 (0 + -0 would be +0)
  g = np.asarray([[1e8], [1.0], [-1e8], [-0.0]], np.float32)
  got = ref.grad_ref(g, [0, 0, 0, 1], 2)
  assert got[0, 0] == 0.0 and np.signbit(got[1, 0])
  assert ref.grad_ref(g[[1, 0, 2, 3]], [0, 0, 0, 1], 2)[0, 0] == 0.0
  assert ref.grad_ref(g[[0, 2, 1, 3]], [0, 0, 0, 1], 2)[0, 0] == 1.0
