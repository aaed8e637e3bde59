"""hbk_hash_translate_runs_n at the C ABI without a GPU: the entry exists beside an unchanged version, its struct
mirrors the header, and every refused argument is refused before any device work with the reason named."""
import ctypes as C
import os
import re

import pytest

from hybridbackend_amd import _lib

FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()


def fake(n):
  return FAKE + n * 0x100000


def _struct_fields(name):
  end = HEADER.index('} %s;' % name)
  body = HEADER[HEADER.rindex('typedef struct {', 0, end):end]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return re.findall(r'(\w+)(?:\[\w+\])?;', body)


def test_symbol_prototype_version_and_struct_layout():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_hash_translate_runs_n')
  assert lib.hbk_hash_translate_runs_n.restype is C.c_int
  assert lib.hbk_hash_translate_runs_n.argtypes == [C.c_int32] + [C.c_void_p] * 5 + [C.c_int32, C.c_void_p]
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  proto = re.search(r'int hbk_hash_translate_runs_n\((.*?)\);', HEADER, flags=re.S).group(1)
  proto = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', proto))
  assert proto == ('int32_t n_cols, const hbk_hash_column_t* cols, const hbk_hash_expiry_t* exp, '
                   'const hbk_hash_admission_t* adm, const int32_t* n_runs, const hbk_hash_run_t* const* runs, '
                   'int32_t insert, hbk_stream_t stream')
  # two pointers and an int64
  R = _lib.HashRun
  assert C.sizeof(R) == 24 and [R.keys.offset, R.slots.offset, R.n_keys.offset] == [0, 8, 16]
  assert _struct_fields('hbk_hash_run_t') == [n for n, _ in R._fields_]
  # the limit the header states covers 26 columns x 8 runs
  limit = int(re.search(r'#define HBK_HASH_MAX_RUNS_PER_LAUNCH (\d+)', HEADER).group(1))
  assert limit == _lib.HASH_MAX_RUNS_PER_LAUNCH and limit >= 26 * 8
  # the structs that were there are what they were
  assert C.sizeof(_lib.HashColumn) == 88 and C.sizeof(_lib.HashExpiry) == 32 and C.sizeof(_lib.HashAdmission) == 40


def _col(**kw):
  col = _lib.HashColumn()
  col.keys_cache, col.slab_count, col.slab_size = fake(0), 8, 16
  col.keys, col.n_keys, col.slots = None, -5, None          # ignored by the entry
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


GOOD_RUNS = [(fake(9), fake(10), 100), (None, None, 0), (fake(11), fake(12), 7)]


def _call(cols, runs_per_col, exp=None, adm=None, n_runs=None, insert=1, null_runs=False, null_n_runs=False):
  """runs_per_col[c]: list of (keys, slots, n_keys), or None for a NULL run array."""
  n = len(cols)
  arr = (_lib.HashColumn * n)(*cols)
  keep, ptrs = [], []
  for runs in runs_per_col:
    if runs is None:
      ptrs.append(None)
      continue
    r = (_lib.HashRun * max(len(runs), 1))()
    for k, (keys, slots, nk) in enumerate(runs):
      r[k].keys, r[k].slots, r[k].n_keys = keys, slots, nk
    keep.append(r)
    ptrs.append(C.cast(r, C.c_void_p).value)
  counts = n_runs if n_runs is not None else [0 if r is None else len(r) for r in runs_per_col]
  lib = _lib.lib()
  rc = lib.hbk_hash_translate_runs_n(
    n, arr, (_lib.HashExpiry * n)(*exp) if exp else None, (_lib.HashAdmission * n)(*adm) if adm else None,
    None if null_n_runs else _lib.i32_array(counts), None if null_runs else _lib.ptr_array(ptrs), insert, None)
  return rc, lib.hbk_last_error().decode()


def _refused(words, *args, **kw):
  rc, msg = _call(*args, **kw)
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in ('hash_translate_runs_n',) + tuple(words):
    assert w in msg, msg


@pytest.mark.parametrize('kind', ['plain', 'expiring', 'admit', 'expiring_admit'])
@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)), (dict(slab_count=0), ('slab_count',)),
  (dict(slab_count=(1 << 56) + 1), ('slab_count', 'range')), (dict(keys_cache=None), ('NULL',)),
  (dict(keys_cache=fake(0) + 4), ('aligned',)), (dict(dim=0), ('dim',)), (dict(table_pitch=3), ('table_pitch',)),
  (dict(init_scale=-1.0), ('init_scale',)), (dict(init_scale=float('inf')), ('init_scale',)),
  (dict(init_scale=float('nan')), ('init_scale',)),
])
def test_what_the_matching_entry_refuses_of_a_column(kind, kw, words):
  exp = [_exp(), _exp()] if 'expiring' in kind else None
  adm = [_adm(), _adm()] if 'admit' in kind else None
  _refused(('column 1',) + words, [_col(), _col(**kw)], [GOOD_RUNS, GOOD_RUNS], exp=exp, adm=adm)


def test_what_the_matching_entries_refuse_of_expiry_and_admission():
  cols, runs = [_col(), _col()], [GOOD_RUNS, GOOD_RUNS]
  for bad in (dict(last_seen=None), dict(freq=None), dict(step=None)):
    _refused(('column 1', 'expiry'), cols, runs, exp=[_exp(), _exp(**bad)])
    _refused(('column 1', 'expiry'), cols, runs, exp=[_exp(), _exp(**bad)], adm=[_adm(), _adm()])
  for bad, word in ((dict(width=0), 'width'), (dict(width=1 << 31), 'width'), (dict(depth=0), 'depth'),
                    (dict(depth=9), 'depth'), (dict(min_freq=0), 'min_freq'), (dict(min_freq=(1 << 30) + 1), 'min_freq'),
                    (dict(sketch=None), 'sketch'), (dict(sketch=fake(7) + 2), 'aligned')):
    _refused(('column 1', word), cols, runs, adm=[_adm(), _adm(**bad)])
    _refused(('column 1', word), cols, runs, exp=[_exp(), _exp()], adm=[_adm(), _adm(**bad)])
  # an expiry buffer is not needed where there is no key
  rc, msg = _call([_col()], [[(None, None, 0)]], exp=[_exp(last_seen=None)])
  assert rc == _lib.OK, msg


def test_refusals_of_the_runs():
  cols = [_col(), _col()]
  _refused(('n_runs or runs is NULL',), cols, [GOOD_RUNS, GOOD_RUNS], null_runs=True)
  _refused(('n_runs or runs is NULL',), cols, [GOOD_RUNS, GOOD_RUNS], null_n_runs=True)
  _refused(('column 1', 'n_runs'), cols, [GOOD_RUNS, GOOD_RUNS], n_runs=[3, -1])
  _refused(('column 1', 'runs is NULL'), cols, [GOOD_RUNS, None], n_runs=[3, 2])
  _refused(('column 1', 'run 2', 'NULL'), cols, [GOOD_RUNS, GOOD_RUNS[:2] + [(None, fake(12), 7)]])
  _refused(('column 1', 'run 0', 'NULL'), cols, [GOOD_RUNS, [(fake(9), None, 1)]])
  _refused(('column 1', 'run 1', 'n_keys'), cols, [GOOD_RUNS, [GOOD_RUNS[0], (fake(9), fake(10), -1)]])
  big = (1 << 30)
  half = [(fake(9), fake(10), big), (fake(11), fake(12), big)]         # 2^31 in all
  _refused(('column 1', '2^31'), cols, [GOOD_RUNS, half])
  quarter = [(fake(9), fake(10), big // 2), (fake(11), fake(12), big // 2)]   # 2^30 in all
  _refused(('column 1', '2^30'), cols, [GOOD_RUNS, quarter], exp=[_exp(), _exp()])
  _refused(('column 1', '2^30'), cols, [GOOD_RUNS, quarter], adm=[_adm(), _adm()])


def test_counts_of_things_and_nothing_to_do():
  lib = _lib.lib()
  f = lib.hbk_hash_translate_runs_n
  assert f(-1, None, None, None, None, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode()
  assert f(1, None, None, None, None, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  for insert in (0, 1):
    assert f(0, None, None, None, None, None, insert, None) == _lib.OK
    # zero runs, and runs of zero keys: nothing to launch, no device is touched
    assert _call([_col(), _col()], [[], [(None, None, 0), (fake(9), fake(10), 0)]], insert=insert)[0] == _lib.OK
    assert _call([_col()], [None], n_runs=[0], exp=[_exp()], adm=[_adm()], insert=insert)[0] == _lib.OK
