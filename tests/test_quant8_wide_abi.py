"""8-bit tables, lanes of 8 and 16 codes at the C ABI and in Python, without a GPU: the two symbols, every refusal
before any device work (the addresses here are no device buffers) with the column named, the width query on fake
pointers, the Python refusals."""
import ctypes as C

import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib

FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it
LOOKUP = _lib.Quant8LookupColumn


def _lookup(**kw):
  col = LOOKUP()
  for k, v in {**dict(table=FAKE, rows=100, dim=16, ids=FAKE + 0x1000, ids_dtype=_lib.INT64, n_ids=8, n_segments=8,
                      divisor=1, combiner=_lib.COMBINER_SUM, out=FAKE + 0x2000), **kw}.items():
    setattr(col, k, v)
  return col


def _wide(cols, lane_codes=8):
  return _lib.lib().hbk_quant8_lookup_fwd_wide(len(cols), (LOOKUP * len(cols))(*cols), lane_codes, None)


def _refused(rc, *words):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in words:
    assert w in msg, msg


def test_symbols_prototypes_and_nothing_to_do():
  lib = _lib.lib()
  assert '0.2.0' in lib.hbk_version().decode() and C.sizeof(LOOKUP) == 104
  vp, i32 = C.c_void_p, C.c_int32
  assert lib.hbk_quant8_lookup_fwd_wide.restype is C.c_int
  assert list(lib.hbk_quant8_lookup_fwd_wide.argtypes) == [i32, vp, i32, vp]
  assert lib.hbk_quant8_lookup_lane_codes.restype is i32
  assert list(lib.hbk_quant8_lookup_lane_codes.argtypes) == [vp, i32]
  for lane_codes in (8, 16):
    assert lib.hbk_quant8_lookup_fwd_wide(0, None, lane_codes, None) == _lib.OK
    # a column without segments launches nothing, whatever its buffers
    assert _wide([_lookup(n_segments=0, n_ids=0, table=None, ids=None, out=None)], lane_codes) == _lib.OK
  _refused(lib.hbk_quant8_lookup_fwd_wide(-1, None, 8, None), 'n_cols')
  _refused(lib.hbk_quant8_lookup_fwd_wide(1, None, 8, None), 'cols is NULL')
  for lane_codes in (0, 4, 12, 32):
    _refused(_wide([_lookup()], lane_codes), f'lane_codes must be 8 or 16, got {lane_codes}')


@pytest.mark.parametrize('kw, words', [
  (dict(chunk_elems=4), ('chunk_elems must be 0',)),
  (dict(chunk_elems=8), ('chunk_elems must be 0',)),
  (dict(dim=0), ('dim must be in [1, 256]',)),
  (dict(dim=264, pitch=268), ('dim must be in [1, 256]',)),
  (dict(pitch=18), ('pitch 18', 'multiple of 4')),
  (dict(pitch=16), ('pitch 16', '>= round_up(dim, 4) + 4 = 20')),
  (dict(table=FAKE + 2), ('table must be 4-byte aligned',)),
  (dict(out_dtype=3), ('out_dtype',)),
  (dict(out=FAKE + 0x2002), ('out must be aligned to its element',)),
  (dict(out=FAKE + 0x2001, out_dtype=_lib.LOWP_BF16), ('out must be aligned to its element',)),
  (dict(dim=65, pitch=72), ('dim 65', '64 otherwise')),
  (dict(dim=128, out=FAKE + 0x2004), ('dim 128', '64 otherwise')),   # falls to one code per lane, which holds 64
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
@pytest.mark.parametrize('lane_codes', (8, 16))
def test_refusals_name_the_column(lane_codes, kw, words):
  _refused(_wide([_lookup(n_segments=0, n_ids=0), _lookup(**kw)], lane_codes), 'quant8_lookup_fwd_wide', 'column 1',
           *words)


@pytest.mark.parametrize('kw, lane_codes, width', [
  (dict(dim=8), 8, 8), (dict(dim=8), 16, 4), (dict(dim=16), 16, 16), (dict(dim=16), 8, 8), (dict(dim=256), 16, 16),
  (dict(dim=24), 8, 8), (dict(dim=24), 16, 4), (dict(dim=48), 16, 16),
  (dict(dim=64, out_dtype=_lib.LOWP_BF16), 16, 16), (dict(dim=64, out_stride=72, out_dtype=_lib.LOWP_FP16), 8, 8),
  (dict(dim=20), 8, 4), (dict(dim=18), 8, 1), (dict(dim=17), 16, 1),                    # dim % L != 0
  (dict(dim=64, out=FAKE + 0x2008), 8, 1),                                              # fp32 out off 16 bytes
  (dict(dim=64, out=FAKE + 0x2008, out_dtype=_lib.LOWP_BF16), 16, 4),                   # 16-bit: 8 bytes carry 4 codes
  (dict(dim=64, out=FAKE + 0x2004, out_dtype=_lib.LOWP_BF16), 16, 1),
  (dict(dim=64, out_stride=66), 8, 1), (dict(dim=64, out_stride=68, out_dtype=_lib.LOWP_BF16), 8, 4),   # the stride
  (dict(dim=64), 0, 4), (dict(dim=64), 4, 4), (dict(dim=3), 0, 1),                      # the narrow forward's rule
  (dict(dim=64), 12, 0), (dict(dim=64), -8, 0),                                         # no such width
])
def test_width_query(kw, lane_codes, width):
  lib = _lib.lib()
  col = _lookup(**kw)
  assert lib.hbk_quant8_lookup_lane_codes(C.byref(col), lane_codes) == width
  assert lib.hbk_quant8_lookup_lane_codes(None, 8) == 0


def test_python_refusals_and_the_pitch_helper():
  E = hb.embedding
  bad = _lib.InvalidArgumentError
  for lane_codes in (4, 12, 32, 'wide', True):
    with pytest.raises(bad, match="lane_codes must be None, 8, 16 or 'auto'"):
      E.Quant8GroupLookup([], [], lane_codes=lane_codes)
  with pytest.raises(bad, match='lane_codes=8 cannot be given together with chunk_elems=4'):
    E.Quant8GroupLookup([], [], lane_codes=8, chunk_elems=4)
  with pytest.raises(bad, match="lane_codes='auto' cannot be given together with chunk_elems=4"):
    E.Quant8GroupLookup([], [], lane_codes='auto', chunk_elems=4)
  for lane_codes in (None, 8, 16, 'auto'):
    look = E.Quant8GroupLookup([], [], lane_codes=lane_codes)
    assert look.lane_codes == lane_codes and look.lane_codes_used == []
  P = E.Quant8Rows.pitch_for
  assert [P(64), P(64, 4), P(64, 8), P(64, 16)] == [68, 68, 72, 80]
  assert [P(8, 8), P(12, 16), P(60, 16), P(256, 16), P(1, 8)] == [16, 16, 64, 272, 8]
  with pytest.raises(bad, match='align must be 4, 8 or 16'):
    P(64, 32)
  # 'auto' names a width only where the measured rule does; elsewhere, and where dim % width != 0, the narrow forward
  assert E.quant8.auto_lane_codes(20, torch.float32, False) == 0
  for ragged, o16, lo, hi, w in E.quant8.AUTO_LANE_CODES:
    assert w in (8, 16) and 1 <= lo <= hi <= 256
  DF, EC = hb.feature_column.DenseFeatures, hb.feature_column.EmbeddingColumn
  with pytest.raises(bad, match="table_lane_codes=\\) applies to table_dtype='int8' only"):
    DF([EC('a', 100, 8)], 'cpu', table_lane_codes=8)
  with pytest.raises(bad, match="table_lane_codes=\\): None, 8, 16 or 'auto', got 12"):
    DF([EC('a', 100, 8)], 'cpu', table_dtype='int8', table_lane_codes=12)
