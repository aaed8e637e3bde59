"""hbk_hash_translate_sequence_n at the C ABI without a GPU: the entry exists beside an unchanged version, its
struct mirrors the header, and every refused argument is refused before any device work with the reason named."""
import ctypes as C
import os
import re

import pytest

from hybridbackend_amd import _lib

FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
KINDS = ['plain', 'expiring', 'admit', 'expiring_admit']
INT64_MIN = -2 ** 63


def fake(n):
  return FAKE + n * 0x100000


def _struct_fields(name):
  end = HEADER.index('} %s;' % name)
  body = HEADER[HEADER.rindex('typedef struct {', 0, end):end]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return re.findall(r'(\w+)(?:\[\w+\])?;', body)


def test_symbol_prototype_version_and_struct_layout():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_hash_translate_sequence_n')
  f = lib.hbk_hash_translate_sequence_n
  assert f.restype is C.c_int
  assert f.argtypes == [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  proto = re.search(r'int hbk_hash_translate_sequence_n\((.*?)\);', HEADER, flags=re.S).group(1)
  proto = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', proto))
  assert proto == ('int32_t n_cols, const hbk_hash_column_t* cols, const hbk_hash_expiry_t* exp, '
                   'const hbk_hash_admission_t* adm, const hbk_hash_sequence_t* seq, '
                   'int32_t insert, hbk_stream_t stream')
  S = _lib.HashSequence
  assert _struct_fields('hbk_hash_sequence_t') == [n for n, _ in S._fields_]
  assert C.sizeof(S) == 40
  assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16, 20, 24, 32]
  # the structs that were there are what they were
  assert C.sizeof(_lib.HashColumn) == 88 and C.sizeof(_lib.HashExpiry) == 32 and C.sizeof(_lib.HashAdmission) == 40
  assert C.sizeof(_lib.Sequence) == 32
  assert _struct_fields('hbk_sequence_t') == [n for n, _ in _lib.Sequence._fields_]


def _col(**kw):
  col = _lib.HashColumn()
  col.keys_cache, col.slab_count, col.slab_size = fake(0), 8, 16
  col.keys, col.n_keys, col.slots = fake(9), 100, fake(10)
  col.counts, col.table, col.dim, col.table_pitch = fake(1), fake(2), 4, 0
  col.init_scale, col.seed = 0.5, 1
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _exp(**kw):
  e = _lib.HashExpiry()
  e.last_seen, e.freq, e.step, e.stats = fake(3), fake(4), fake(5), fake(6)
  for k, v in kw.items():
    setattr(e, k, v)
  return e


def _adm(**kw):
  a = _lib.HashAdmission()
  a.sketch, a.width, a.depth, a.min_freq, a.seed, a.filtered = fake(7), 64, 4, 2, 0, fake(8)
  for k, v in kw.items():
    setattr(a, k, v)
  return a


def _seq(**kw):
  q = _lib.HashSequence()
  q.row_splits, q.n_segments, q.max_len, q.has_pad, q.pad_id, q.lengths = fake(11), 37, 7, 0, 0, fake(12)
  for k, v in kw.items():
    setattr(q, k, v)
  return q


def _call(kind, cols, seqs, exp=None, adm=None, insert=1, null_seq=False):
  n = len(cols)
  if exp is None and 'expiring' in kind:
    exp = [_exp() for _ in range(n)]
  if adm is None and 'admit' in kind:
    adm = [_adm() for _ in range(n)]
  lib = _lib.lib()
  rc = lib.hbk_hash_translate_sequence_n(
    n, (_lib.HashColumn * n)(*cols), (_lib.HashExpiry * n)(*exp) if exp else None,
    (_lib.HashAdmission * n)(*adm) if adm else None,
    None if null_seq else (_lib.HashSequence * n)(*seqs), insert, None)
  return rc, lib.hbk_last_error().decode()


def _refused(words, *args, **kw):
  rc, msg = _call(*args, **kw)
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_translate_sequence_n',) + tuple(words):
    assert w in msg, msg


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)), (dict(slab_count=0), ('slab_count',)),
  (dict(slab_count=(1 << 56) + 1), ('slab_count', 'range')), (dict(keys_cache=None), ('NULL',)),
  (dict(keys_cache=fake(0) + 4), ('aligned',)), (dict(dim=0), ('dim',)), (dict(table_pitch=3), ('table_pitch',)),
  (dict(init_scale=-1.0), ('init_scale',)), (dict(init_scale=float('inf')), ('init_scale',)),
  (dict(init_scale=float('nan')), ('init_scale',)),
])
def test_what_the_matching_entry_refuses_of_a_column(kind, kw, words):
  _refused(('column 1',) + words, kind, [_col(), _col(**kw)], [_seq(), _seq()])


def test_what_the_matching_entries_refuse_of_expiry_and_admission():
  cols, seqs = [_col(), _col()], [_seq(), _seq()]
  for bad in (dict(last_seen=None), dict(freq=None), dict(step=None)):
    _refused(('column 1', 'expiry'), 'expiring', cols, seqs, exp=[_exp(), _exp(**bad)])
    _refused(('column 1', 'expiry'), 'expiring_admit', cols, seqs, exp=[_exp(), _exp(**bad)])
  for bad, word in ((dict(width=0), 'width'), (dict(width=1 << 31), 'width'), (dict(depth=0), 'depth'),
                    (dict(depth=9), 'depth'), (dict(min_freq=0), 'min_freq'), (dict(min_freq=(1 << 30) + 1), 'min_freq'),
                    (dict(sketch=None), 'sketch'), (dict(sketch=fake(7) + 2), 'aligned')):
    _refused(('column 1', word), 'admit', cols, seqs, adm=[_adm(), _adm(**bad)])
    _refused(('column 1', word), 'expiring_admit', cols, seqs, adm=[_adm(), _adm(**bad)])
  # neither an expiry buffer nor a sketch is needed where there is no position
  none = [_col(keys=None, n_keys=0, slots=None)], [_seq(n_segments=0)]
  assert _call('expiring', *none, exp=[_exp(last_seen=None)])[0] == _lib.OK
  assert _call('admit', *none, adm=[_adm(sketch=None)])[0] == _lib.OK


@pytest.mark.parametrize('kind', KINDS)
def test_refusals_of_the_sequence(kind):
  cols, good = [_col(), _col()], _seq()
  _refused(('seq is NULL',), kind, cols, [good, good], null_seq=True)
  _refused(('column 1', 'max_len'), kind, cols, [good, _seq(max_len=0)])
  _refused(('column 1', 'max_len'), kind, cols, [good, _seq(max_len=-3)])
  _refused(('column 1', 'n_segments'), kind, cols, [good, _seq(n_segments=-1)])
  # B * T: below 2^31, below 2^30 where a counter must not wrap
  counted = kind != 'plain'
  limit, word = (1 << 30, '2^30') if counted else (1 << 31, '2^31')
  _refused(('column 1', word), kind, cols, [good, _seq(n_segments=limit // 8, max_len=8)])
  _refused(('column 1', word), kind, cols, [good, _seq(n_segments=limit, max_len=1)])
  _refused(('column 1', word), kind, cols, [good, _seq(n_segments=3, max_len=(1 << 31) - 1)])
  _refused(('column 1', word), kind, cols, [good, _seq(n_segments=1 << 40, max_len=1 << 30)])
  if counted:
    _refused(('column 1', 'wrap'), kind, cols, [good, _seq(n_segments=limit // 8, max_len=8)])
  # buffers
  _refused(('column 1', 'NULL slots'), kind, [_col(), _col(slots=None)], [good, good])
  _refused(('column 1', 'NULL keys'), kind, [_col(), _col(keys=None)], [good, good])
  _refused(('column 1', 'n_keys'), kind, [_col(), _col(n_keys=-1)], [good, good])
  _refused(('column 1', 'n_keys'), kind, [_col(), _col(n_keys=1 << 31)], [good, good])
  _refused(('column 1', 'row_splits is NULL', 'n_segments'), kind, cols, [good, _seq(row_splits=None)])
  # the pad id is a raw id the table can store
  _refused(('column 1', 'pad_id', 'INT64_MIN'), kind, cols, [good, _seq(has_pad=1, pad_id=INT64_MIN)])
  if 'expiring' in kind:
    _refused(('column 1', 'pad_id', 'INT64_MIN + 1'), kind, cols, [good, _seq(has_pad=1, pad_id=INT64_MIN + 1)])


def test_counts_of_things():
  lib = _lib.lib()
  f = lib.hbk_hash_translate_sequence_n
  assert f(-1, None, None, None, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode()
  assert f(1, None, None, None, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()


@pytest.mark.parametrize('kind', KINDS)
def test_nothing_to_do_is_accepted(kind):
  f = _lib.lib().hbk_hash_translate_sequence_n
  for insert in (0, 1):
    assert f(0, None, None, None, None, insert, None) == _lib.OK
    # no samples: nothing to launch, no device is touched, no buffer is needed -- with and without a pad id, with
    # row_splits (of one entry) and without
    empty = _col(keys=None, n_keys=0, slots=None)
    for q in (_seq(n_segments=0, lengths=None), _seq(n_segments=0, row_splits=None, lengths=None),
              _seq(n_segments=0, has_pad=1, pad_id=-1)):
      rc, msg = _call(kind, [empty, empty], [q, q], insert=insert)
      assert rc == _lib.OK, msg
    # a sentinel pad id that is not in use is not looked at
    rc, msg = _call(kind, [empty], [_seq(n_segments=0, has_pad=0, pad_id=INT64_MIN)], insert=insert)
    assert rc == _lib.OK, msg
