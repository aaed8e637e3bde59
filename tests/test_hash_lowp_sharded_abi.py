"""16-bit hash tables behind runs, sequences and the sharded plan, at the C ABI and in Python's argument handling,
without a GPU: hbk_hash_translate_runs_lowp_n, hbk_hash_translate_sequence_lowp_n and hbk_sharded_set_lowp_hash_tables
exist beside unchanged structs and version and are declared as documented; the two translate entries refuse every bad
argument before any device work (fake pointers) with the entry, the column and the field named; the Python objects
over them refuse what is not built; and the messages older tests pin for mixed lists still read as they did."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib

FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()
KINDS = ['plain', 'expiring', 'admit', 'expiring_admit']
BF16, FP16 = _lib.LOWP_BF16, _lib.LOWP_FP16
LOWP = [torch.bfloat16, torch.float16]
RUNS, SEQ = 'hash_translate_runs_lowp_n', 'hash_translate_sequence_lowp_n'
INT64_MIN = -2 ** 63


def fake(n):
  return FAKE + n * 0x100000


def _params(name):
  m = re.search(r'int %s\((.*?)\);' % name, HEADER, flags=re.S)
  assert m is not None, name
  return [' '.join(p.split()) for p in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')], m.start()


def test_symbols_version_and_structs_are_those_of_0_2_0():
  lib = _lib.lib()
  out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True)
  for name in ('hbk_hash_translate_runs_lowp_n', 'hbk_hash_translate_sequence_lowp_n',
               'hbk_sharded_set_lowp_hash_tables'):
    assert hasattr(lib, name), name
    assert re.search(r'\bT %s\b' % name, out.stdout), name
  vp, i32 = C.c_void_p, C.c_int32
  assert lib.hbk_hash_translate_runs_lowp_n.argtypes == [i32] + [vp] * 6 + [i32, vp]
  assert lib.hbk_hash_translate_sequence_lowp_n.argtypes == [i32] + [vp] * 5 + [i32, vp]
  assert lib.hbk_sharded_set_lowp_hash_tables.argtypes == [vp, vp, vp, i32]
  assert all(getattr(lib, n).restype is C.c_int for n in ('hbk_hash_translate_runs_lowp_n',
                                                          'hbk_hash_translate_sequence_lowp_n',
                                                          'hbk_sharded_set_lowp_hash_tables'))
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950' and hb.__version__ == '0.2.0'
  assert C.sizeof(_lib.HashColumn) == 88 and C.sizeof(_lib.HashExpiry) == 32 and C.sizeof(_lib.HashAdmission) == 40
  assert C.sizeof(_lib.HashRun) == 24 and C.sizeof(_lib.HashSequence) == 40


def test_header_declares_the_entries_as_documented():
  got, at = _params('hbk_hash_translate_runs_lowp_n')
  assert got == ['int32_t n_cols', 'const hbk_hash_column_t* cols', 'const hbk_hash_expiry_t* exp',
                 'const hbk_hash_admission_t* adm', 'const int32_t* table_dtypes', 'const int32_t* n_runs',
                 'const hbk_hash_run_t* const* runs', 'int32_t insert', 'hbk_stream_t stream']
  assert HEADER.index('} hbk_hash_run_t;') < at and HEADER.index('#define HBK_LOWP_FP16') < at
  got, at = _params('hbk_hash_translate_sequence_lowp_n')
  assert got == ['int32_t n_cols', 'const hbk_hash_column_t* cols', 'const hbk_hash_expiry_t* exp',
                 'const hbk_hash_admission_t* adm', 'const int32_t* table_dtypes', 'const hbk_hash_sequence_t* seq',
                 'int32_t insert', 'hbk_stream_t stream']
  assert HEADER.index('} hbk_hash_sequence_t;') < at
  got, at = _params('hbk_sharded_set_lowp_hash_tables')
  assert got == ['hbk_sharded_t plan', 'const hbk_sharded_hash_t* tables', 'const int32_t* dtypes', 'int32_t wire']
  assert HEADER.index('} hbk_sharded_hash_t;') < at and HEADER.index('#define HBK_LOWP_WIRE_FLOAT') < at
  # the fp32 entries are declared as they were
  assert _params('hbk_hash_translate_runs_n')[0][4] == 'const int32_t* n_runs'
  assert _params('hbk_hash_translate_sequence_n')[0][4] == 'const hbk_hash_sequence_t* seq'


# ---- the two translate entries ----------------------------------------------------------------------------------
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


GOOD_RUNS = [(fake(9), fake(10), 100), (None, None, 0), (fake(11), fake(12), 7)]
NO_CODES = object()


def _kind_records(kind, n, exp, adm):
  if exp is None and 'expiring' in kind:
    exp = [_exp() for _ in range(n)]
  if adm is None and 'admit' in kind:
    adm = [_adm() for _ in range(n)]
  return ((_lib.HashExpiry * n)(*exp) if exp else None, (_lib.HashAdmission * n)(*adm) if adm else None)


def _call_runs(kind, cols, runs_per_col=None, codes=None, exp=None, adm=None, insert=1, n_runs=None, null_runs=False):
  n = len(cols)
  runs_per_col = [GOOD_RUNS] * n if runs_per_col is None else runs_per_col
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
  e, a = _kind_records(kind, n, exp, adm)
  dt = None if codes is NO_CODES else (C.c_int32 * n)(*(codes or [BF16] * n))
  lib = _lib.lib()
  rc = lib.hbk_hash_translate_runs_lowp_n(n, (_lib.HashColumn * n)(*cols), e, a, dt, _lib.i32_array(counts),
                                          None if null_runs else _lib.ptr_array(ptrs), insert, None)
  return rc, lib.hbk_last_error().decode()


def _call_seq(kind, cols, seqs=None, codes=None, exp=None, adm=None, insert=1, null_seq=False):
  n = len(cols)
  seqs = [_seq() for _ in range(n)] if seqs is None else seqs
  e, a = _kind_records(kind, n, exp, adm)
  dt = None if codes is NO_CODES else (C.c_int32 * n)(*(codes or [BF16] * n))
  lib = _lib.lib()
  rc = lib.hbk_hash_translate_sequence_lowp_n(n, (_lib.HashColumn * n)(*cols), e, a, dt,
                                              None if null_seq else (_lib.HashSequence * n)(*seqs), insert, None)
  return rc, lib.hbk_last_error().decode()


ENTRIES = [(RUNS, _call_runs), (SEQ, _call_seq)]


def _refused(words, cols, kinds=KINDS, **kw):
  """Both entries, every table kind, insert and find: refused with the entry and `words` in the message."""
  for entry, call in ENTRIES:
    for kind in kinds:
      for insert in (1, 0):
        rc, msg = call(kind, cols, insert=insert, **kw)
        assert rc == _lib.INVALID_ARGUMENT, (entry, kind, insert, rc, msg)
        for w in (entry,) + tuple(words):
          assert w in msg, (entry, kind, msg)


def test_n_cols_0_is_ok_and_touches_nothing():
  lib = _lib.lib()
  for insert in (0, 1):
    assert lib.hbk_hash_translate_runs_lowp_n(0, None, None, None, None, None, None, insert, None) == _lib.OK
    assert lib.hbk_hash_translate_sequence_lowp_n(0, None, None, None, None, None, insert, None) == _lib.OK
  assert lib.hbk_hash_translate_runs_lowp_n(-1, None, None, None, None, None, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode() and RUNS in lib.hbk_last_error().decode()
  assert lib.hbk_hash_translate_sequence_lowp_n(-1, None, None, None, None, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode() and SEQ in lib.hbk_last_error().decode()
  dt = (C.c_int32 * 1)(BF16)
  assert lib.hbk_hash_translate_runs_lowp_n(1, None, None, None, dt, None, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  assert lib.hbk_hash_translate_sequence_lowp_n(1, None, None, None, dt, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  # nothing to launch: no keys, no positions -- no device is touched, for every kind
  for kind in KINDS:
    for insert in (0, 1):
      rc, msg = _call_runs(kind, [_col(), _col()], [[], [(None, None, 0), (fake(9), fake(10), 0)]], [BF16, FP16],
                           insert=insert)
      assert rc == _lib.OK, msg
      empty = _col(keys=None, n_keys=0, slots=None)
      rc, msg = _call_seq(kind, [empty, empty], [_seq(n_segments=0, lengths=None)] * 2, [FP16, BF16], insert=insert)
      assert rc == _lib.OK, msg


@pytest.mark.parametrize('kw,words', [
  (dict(slab_size=0), ('slab_size',)), (dict(slab_size=65), ('slab_size',)), (dict(slab_count=0), ('slab_count',)),
  (dict(keys_cache=None), ('NULL',)), (dict(keys_cache=fake(0) + 4), ('aligned',)), (dict(dim=0), ('dim',)),
  (dict(dim=4, table_pitch=2), ('table_pitch',)), (dict(init_scale=-1.0), ('init_scale',)),
  (dict(init_scale=float('inf')), ('init_scale',)), (dict(init_scale=float('nan')), ('init_scale',)),
])
def test_what_the_fp32_entries_refuse_of_a_column(kw, words):
  _refused(('column 1',) + words, [_col(), _col(**kw)])


def test_what_the_fp32_entries_refuse_of_expiry_and_admission():
  cols = [_col(), _col()]
  for bad in (dict(last_seen=None), dict(freq=None), dict(step=None)):
    _refused(('column 1', 'expiry'), cols, kinds=['expiring', 'expiring_admit'], exp=[_exp(), _exp(**bad)])
  for bad, word in ((dict(width=0), 'width'), (dict(depth=9), 'depth'), (dict(min_freq=0), 'min_freq'),
                    (dict(sketch=None), 'sketch'), (dict(sketch=fake(7) + 2), 'aligned')):
    _refused(('column 1', word), cols, kinds=['admit', 'expiring_admit'], adm=[_adm(), _adm(**bad)])


def test_what_the_fp32_entries_refuse_of_runs_and_sequences():
  cols = [_col(), _col()]
  for kind in KINDS:
    for rc, msg in (_call_runs(kind, cols, null_runs=True), ):
      assert rc == _lib.INVALID_ARGUMENT and RUNS in msg and 'n_runs or runs is NULL' in msg, msg
    rc, msg = _call_runs(kind, cols, [GOOD_RUNS, GOOD_RUNS], n_runs=[3, -1])
    assert rc == _lib.INVALID_ARGUMENT and 'column 1' in msg and 'n_runs' in msg, msg
    rc, msg = _call_runs(kind, cols, [GOOD_RUNS, None], n_runs=[3, 2])
    assert rc == _lib.INVALID_ARGUMENT and 'column 1' in msg and 'runs is NULL' in msg, msg
    rc, msg = _call_runs(kind, cols, [GOOD_RUNS, [GOOD_RUNS[0], (fake(9), None, 1)]])
    assert rc == _lib.INVALID_ARGUMENT and 'column 1' in msg and 'run 1' in msg and 'NULL' in msg, msg
    rc, msg = _call_runs(kind, cols, [GOOD_RUNS, [(fake(9), fake(10), -1)]])
    assert rc == _lib.INVALID_ARGUMENT and 'run 0' in msg and 'n_keys' in msg, msg
    big = 1 << 30
    word = '2^31' if kind == 'plain' else '2^30'
    rc, msg = _call_runs(kind, cols, [GOOD_RUNS, [(fake(9), fake(10), big), (fake(11), fake(12), big)]])
    assert rc == _lib.INVALID_ARGUMENT and 'column 1' in msg and word in msg, msg
    # sequences
    good = _seq()
    rc, msg = _call_seq(kind, cols, null_seq=True)
    assert rc == _lib.INVALID_ARGUMENT and SEQ in msg and 'seq is NULL' in msg, msg
    for bad, words in ((_seq(max_len=0), ('max_len',)), (_seq(n_segments=-1), ('n_segments',)),
                       (_seq(n_segments=big, max_len=2), (word,)), (_seq(row_splits=None), ('row_splits is NULL',)),
                       (_seq(has_pad=1, pad_id=INT64_MIN), ('pad_id', 'INT64_MIN'))):
      rc, msg = _call_seq(kind, cols, [good, bad])
      assert rc == _lib.INVALID_ARGUMENT and SEQ in msg and 'column 1' in msg, msg
      for w in words:
        assert w in msg, msg
    if 'expiring' in kind:
      rc, msg = _call_seq(kind, cols, [good, _seq(has_pad=1, pad_id=INT64_MIN + 1)])
      assert rc == _lib.INVALID_ARGUMENT and 'INT64_MIN + 1' in msg, msg
    rc, msg = _call_seq(kind, [_col(), _col(slots=None)])
    assert rc == _lib.INVALID_ARGUMENT and 'column 1' in msg and 'NULL slots' in msg, msg
    rc, msg = _call_seq(kind, [_col(), _col(keys=None)])
    assert rc == _lib.INVALID_ARGUMENT and 'column 1' in msg and 'NULL keys' in msg, msg


# ---- what only the 16-bit entries refuse -----------------------------------------------------------------------------
def test_refuses_null_table_dtypes():
  _refused(('table_dtypes',), [_col()], codes=NO_CODES)


@pytest.mark.parametrize('bad', [0, 3, -1, 16])
def test_refuses_an_unknown_element_code(bad):
  _refused(('column 1', 'table_dtypes'), [_col(), _col()], codes=[FP16, bad])


@pytest.mark.parametrize('code', [BF16, FP16])
def test_refuses_rows_that_are_no_whole_words(code):
  _refused(('column 1', 'dim'), [_col(), _col(dim=15)], codes=[code] * 2)
  _refused(('column 0', 'dim'), [_col(dim=1)], codes=[code])
  _refused(('column 0', 'table_pitch'), [_col(dim=16, table_pitch=17)], codes=[code])
  _refused(('column 0', 'table', 'aligned'), [_col(table=fake(2) + 2)], codes=[code])


def test_refuses_an_fp16_scale_that_rounds_to_infinity():
  _refused(('column 1', 'init_scale', '65504'), [_col(), _col(init_scale=65505.0)], codes=[FP16, FP16])
  # bf16 has fp32's range; fp16 takes its largest finite value (nothing to launch: no device is touched)
  for code, scale in ((BF16, 65505.0), (BF16, 1e30), (FP16, 65504.0)):
    rc, msg = _call_runs('plain', [_col(init_scale=scale)], [[]], [code])
    assert rc == _lib.OK, (code, scale, msg)
    rc, msg = _call_seq('plain', [_col(init_scale=scale, keys=None, n_keys=0, slots=None)], [_seq(n_segments=0)],
                        [code])
    assert rc == _lib.OK, (code, scale, msg)


def test_a_column_without_a_table_may_have_any_dim():
  rc, msg = _call_runs('plain', [_col(table=None, dim=15)], [[]], [BF16])
  assert rc == _lib.OK, msg


def test_the_sharded_setter_needs_a_plan():
  lib = _lib.lib()
  assert lib.hbk_sharded_set_lowp_hash_tables(None, None, None, 0) == _lib.INVALID_ARGUMENT
  msg = lib.hbk_last_error().decode()
  assert 'sharded_set_lowp_hash_tables' in msg and 'plan is NULL' in msg


# ---- Python -----------------------------------------------------------------------------------------------------
class _TwoRanks:
  world_size, rank = 2, 1


def _tables(*dtypes, dim=8, **kw):
  return [hb.embedding.HashTable(64, dim, 'meta', dtype=d, **kw) for d in dtypes]


@pytest.mark.parametrize('dtype', LOWP)
def test_the_sharded_driver_refuses_by_name(dtype):
  bad = _lib.InvalidArgumentError
  D = hb.embedding.LowpShardedHashGroupLookup
  with pytest.raises(bad, match='LowpShardedHashGroupLookup: every table must be a 16-bit HashTable.*table 0: fp32'):
    D(_tables(torch.float32), _TwoRanks())
  with pytest.raises(bad, match='table 0: ' + str(dtype) + ', table 1: fp32.*a mix through two drivers'):
    D(_tables(dtype, torch.float32), _TwoRanks())
  for kw, word in ((dict(max_norms=[1.0]), 'max_norms is not supported'),
                   (dict(max_norms=2.0), 'max_norms is not supported'),
                   (dict(weight_grads=True), 'weight_grads is not supported'),
                   (dict(wire_dtype=torch.float16), 'wire_dtype is not supported'),
                   (dict(hot_rows=True), 'hot_rows is not supported'),
                   (dict(hot_rows='auto'), 'hot_rows is not supported'),
                   (dict(wire='half'), "wire must be 'table' or 'float'"),
                   (dict(rounding='up'), "'nearest' or 'stochastic'"),
                   (dict(seed=-1), 'seed')):
    with pytest.raises(bad, match='LowpShardedHashGroupLookup: .*' + word):
      D(_tables(dtype), _TwoRanks(), **kw)
  with pytest.raises(bad, match='table 1: dim 130.*dim % 4 == 0'):
    D(_tables(dtype) + _tables(dtype, dim=130), _TwoRanks())
  if dtype == torch.float16:
    with pytest.raises(bad, match='bfloat16 tables only'):
      D(_tables(dtype), _TwoRanks(), rounding='stochastic')
  drv = D.__new__(D)
  with pytest.raises(_lib.HbkError, match='LowpShardedHashGroupLookup: p2p_bind is not supported'):
    drv.p2p_bind([])
  with pytest.raises(bad, match='LowpShardedHashGroupLookup: weight_grads is not supported'):
    drv.backward([], weight_grads=True)
  with pytest.raises(_lib.HbkError, match='no separate phase methods'):
    drv.partition([])
  # PipelinedLookup refuses every driver over hash tables, this one included
  drv.tables = []
  with pytest.raises(_lib.HbkError, match='PipelinedLookup over hash columns'):
    hb.embedding.PipelinedLookup([drv, drv])
  assert issubclass(D, hb.embedding.ShardedHashGroupLookup)


@pytest.mark.parametrize('dtype', LOWP)
def test_a_16_bit_sequence_lookup_refuses_max_norms_by_name(dtype):
  with pytest.raises(_lib.InvalidArgumentError, match='HashSequenceLookup: max_norms is not supported for 16-bit'):
    hb.embedding.HashSequenceLookup(_tables(dtype, dtype), max_lens=4, max_norms=[None, 1.0])
  with pytest.raises(_lib.InvalidArgumentError, match='LowpSequenceLookupGrad needs a HashSequenceLookup over 16-bit'):
    hb.embedding.LowpSequenceLookupGrad(object())


@pytest.mark.parametrize('dtype', LOWP)
def test_mixed_lists_are_refused_in_the_words_older_tests_pin(dtype):
  a, = _tables(torch.float32)
  t, = _tables(dtype)
  with pytest.raises(_lib.InvalidArgumentError, match='HashSequenceLookup: table 1 is a ' + str(dtype)):
    hb.embedding.HashSequenceLookup([a, t], max_lens=4)
  with pytest.raises(_lib.InvalidArgumentError, match='HashSequenceLookup: table 0 is a ' + str(dtype)):
    hb.embedding.HashSequenceLookup([t, a, t], max_lens=4)
  ids = [torch.zeros(4, dtype=torch.int64, device='meta')] * 2
  with pytest.raises(_lib.InvalidArgumentError, match='hash_translate_sequence: table 1 is a ' + str(dtype)):
    hb.embedding.hash_translate_sequence([a, t], ids, max_lens=4)
  # ShardedHashGroupLookup stays fp32-only: a list that is 16-bit throughout is refused there too
  with pytest.raises(_lib.InvalidArgumentError, match='ShardedHashGroupLookup: table 0 is a ' + str(dtype)):
    hb.embedding.ShardedHashGroupLookup([t, a], None)
  with pytest.raises(_lib.InvalidArgumentError, match='ShardedHashGroupLookup: table 0 is a ' + str(dtype)):
    hb.embedding.ShardedHashGroupLookup([t, t], None)


# ---- the feature-column layers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', LOWP)
def test_hash_columns_take_a_dtype_and_check_the_tables_refusals_when_made(dtype):
  fc = hb.feature_column
  bad = _lib.InvalidArgumentError
  for make in (lambda **kw: fc.HashEmbeddingColumn('h', 64, kw.pop('dim', 8), **kw),
               lambda **kw: fc.HashSequenceEmbeddingColumn('h', 64, kw.pop('dim', 8), 4, **kw)):
    assert make().dtype == torch.float32 and 'dtype' not in make().table_args     # the default changes nothing
    col = make(dtype=dtype)
    assert col.dtype == dtype and col.make_table('meta', 1).dtype == dtype
    with pytest.raises(bad, match='dim must be even'):
      make(dim=7, dtype=dtype)
    with pytest.raises(bad, match='dtype'):
      make(dtype=torch.float64)
    with pytest.raises(bad, match='65504'):
      make(dtype=torch.float16, init_scale=65505.0)
    make(dim=7)                                                                     # odd dims stay fine in fp32


@pytest.mark.parametrize('dtype', LOWP)
def test_the_layers_refuse_by_name(dtype):
  fc = hb.feature_column
  bad = _lib.InvalidArgumentError
  H, S = fc.HashEmbeddingColumn, fc.HashSequenceEmbeddingColumn
  other = torch.float16 if dtype == torch.bfloat16 else torch.float32
  # a mix of hash dtypes in one layer: at construction, before any table is made
  with pytest.raises(bad, match="DenseFeatures: the hash columns of one layer share one dtype.*'a'.*'b'.*two layers"):
    fc.DenseFeatures([H('a', 64, 8), fc.EmbeddingColumn('e', 100, 8), H('b', 64, 8, dtype=dtype)], 'cpu')
  with pytest.raises(bad, match='SequenceFeatures: the hash columns of one layer share one dtype.*two layers'):
    fc.SequenceFeatures([S('a', 64, 8, 4, dtype=other), S('b', 64, 8, 4, dtype=dtype)], 'cpu')
  with pytest.raises(bad, match="hash column 'h' is a " + str(dtype) + ' column with max_norm'):
    fc.DenseFeatures([H('h', 64, 8, dtype=dtype, max_norm=1.0)], 'cpu')
  with pytest.raises(bad, match="hash column 's' is a " + str(dtype) + ' column with max_norm'):
    fc.SequenceFeatures([S('s', 64, 8, 4, dtype=dtype, max_norm=1.0)], 'cpu')
  with pytest.raises(bad, match="hash column 'h' is a " + str(dtype) + " column with weight_feature_key 'w'"):
    fc.DenseFeatures([H('h', 64, 8, dtype=dtype, weight_feature_key='w')], 'cpu')
  with pytest.raises(bad, match="'nearest' or 'stochastic'"):
    fc.DenseFeatures([H('h', 64, 8, dtype=dtype)], 'cpu', table_rounding='up')
  if dtype == torch.float16:
    with pytest.raises(bad, match='bfloat16 tables only'):
      fc.SequenceFeatures([S('s', 64, 8, 4, dtype=dtype)], 'cpu', table_rounding='stochastic')
  # table_dtype stays the bucketed tables' argument and still refuses a hash column, of any dtype
  with pytest.raises(bad, match="'h' is hash-keyed"):
    fc.DenseFeatures([fc.EmbeddingColumn('e', 100, 8), H('h', 64, 8, dtype=dtype)], 'cpu', table_dtype=torch.bfloat16)
  # backward(weight_grads=True) on a layer with 16-bit hash columns
  layer = fc.DenseFeatures.__new__(fc.DenseFeatures)
  layer._hash, layer.hash_dtype = [0], dtype   # pylint: disable=protected-access
  with pytest.raises(bad, match=r'backward\(weight_grads=True\).*16-bit'):
    layer._refuse_weight_grads('DenseFeatures', True)   # pylint: disable=protected-access
  layer._refuse_weight_grads('DenseFeatures', False)   # pylint: disable=protected-access
