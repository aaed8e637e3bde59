"""Hash-keyed 16-bit tables at the C ABI and in Python's argument handling, without a GPU: hbk_hash_insert_lowp_n
exists beside unchanged structs and version, is declared as documented, refuses every bad argument before any device
work with the entry, the column and the field named; HashTable(dtype=) and the objects over it refuse what is not
built; and the oracle of the GPU tests -- the fp32 start values of tests/support/hash_ref.py rounded by
tests/support/lowp_ref.py -- is torch's own cast, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import hashtable as _ht
from tests.support import hash_ref
from tests.support import lowp_ref

FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them
FAKE2 = 0x7f0000101000
FAKE3 = 0x7f0000201000
FAKE4 = 0x7f0000301000
ENTRY = 'hash_insert_lowp_n'
BF16, FP16 = _lib.LOWP_BF16, _lib.LOWP_FP16
LOWP = [torch.bfloat16, torch.float16]


def test_symbol_version_and_structs_are_those_of_0_2_0():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_hash_insert_lowp_n')
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  assert hb.__version__ == '0.2.0'
  assert C.sizeof(_lib.HashColumn) == 88 and C.sizeof(_lib.HashExpiry) == 32 and C.sizeof(_lib.HashAdmission) == 40
  assert (BF16, FP16) == (1, 2)


def test_header_declares_the_entry_as_documented():
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'include', 'hbk.h')).read()
  m = re.search(r'int hbk_hash_insert_lowp_n\((.*?)\);', text, flags=re.S)
  assert m is not None
  params = [' '.join(p.split()) for p in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')]
  assert params == ['int32_t n_cols', 'const hbk_hash_column_t* cols', 'const hbk_hash_expiry_t* exp',
                    'const hbk_hash_admission_t* adm', 'const int32_t* table_dtypes', 'int32_t insert',
                    'hbk_stream_t stream']
  # the records it takes are declared before it
  for name in ('} hbk_hash_column_t;', '} hbk_hash_expiry_t;', '} hbk_hash_admission_t;', '#define HBK_LOWP_FP16'):
    assert text.index(name) < m.start(), name


def _col(**kw):
  col = _lib.HashColumn()
  col.keys_cache, col.slab_count, col.slab_size = FAKE, 8, 16
  col.keys, col.n_keys, col.slots, col.counts = FAKE2, 100, FAKE3, FAKE4
  col.table, col.dim, col.table_pitch, col.init_scale, col.seed = FAKE4 + 4096, 16, 0, 1e-3, 0
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _exp(**kw):
  x = _lib.HashExpiry()
  x.last_seen, x.freq, x.step, x.stats = FAKE, FAKE2, FAKE3, FAKE4
  for k, v in kw.items():
    setattr(x, k, v)
  return x


def _adm(**kw):
  f = _lib.HashAdmission()
  f.sketch, f.width, f.depth, f.min_freq, f.seed, f.filtered = FAKE, 64, 4, 2, 0, FAKE2
  for k, v in kw.items():
    setattr(f, k, v)
  return f


KINDS = ['plain', 'expiring', 'admit', 'expiring_admit']


def _call(cols, kind, codes, insert, exps=None, adms=None):
  lib = _lib.lib()
  n = len(cols)
  arr = (_lib.HashColumn * n)(*cols)
  exp = (_lib.HashExpiry * n)(*(exps or [_exp() for _ in cols])) if 'expiring' in kind else None
  adm = (_lib.HashAdmission * n)(*(adms or [_adm() for _ in cols])) if 'admit' in kind else None
  dtypes = (C.c_int32 * n)(*codes) if codes is not None else None
  rc = lib.hbk_hash_insert_lowp_n(n, arr, exp, adm, dtypes, insert, None)
  return rc, lib.hbk_last_error().decode()


def _refused(cols, *words, kinds=KINDS, codes=None, exps=None, adms=None, null_dtypes=False):
  for kind in kinds:
    for insert in (1, 0):
      given = None if null_dtypes else (codes or [BF16] * len(cols))
      rc, msg = _call(cols, kind, given, insert, exps, adms)
      assert rc == _lib.INVALID_ARGUMENT, (kind, insert, rc, msg)
      for w in (ENTRY,) + words:
        assert w in msg, (kind, msg)


# ---- everything the matching fp32 entry refuses ----------------------------------------------------------------
@pytest.mark.parametrize('bad', [0, -1, 65])
def test_refuses_slab_size_outside_1_to_64(bad):
  _refused([_col(), _col(slab_size=bad)], 'column 1', 'slab_size')


def test_refuses_slab_count_below_one():
  _refused([_col(slab_count=0)], 'column 0', 'slab_count')


@pytest.mark.parametrize('field', ['keys_cache', 'keys', 'slots'])
def test_refuses_null_buffers_with_keys(field):
  _refused([_col(), _col(), _col(**{field: None})], 'column 2', 'NULL')


def test_refuses_dim_pitch_and_init_scale_as_the_fp32_entry():
  _refused([_col(dim=0)], 'column 0', 'dim')
  _refused([_col(dim=16, table_pitch=14)], 'column 0', 'table_pitch')
  for bad in (-1e-3, float('nan'), float('inf')):
    _refused([_col(init_scale=bad)], 'column 0', 'init_scale')


def test_refuses_bad_counts_of_things():
  lib = _lib.lib()
  dt = (C.c_int32 * 1)(BF16)
  assert lib.hbk_hash_insert_lowp_n(-1, None, None, None, None, 1, None) == _lib.INVALID_ARGUMENT
  assert 'n_cols' in lib.hbk_last_error().decode() and ENTRY in lib.hbk_last_error().decode()
  assert lib.hbk_hash_insert_lowp_n(1, None, None, None, dt, 1, None) == _lib.INVALID_ARGUMENT
  assert 'cols is NULL' in lib.hbk_last_error().decode()
  _refused([_col(n_keys=-1)], 'column 0', 'n_keys')
  _refused([_col(n_keys=1 << 31)], 'column 0', 'n_keys')
  # the expiring and the filtered kinds count in int32 words that must not wrap
  _refused([_col(n_keys=1 << 30)], 'column 0', 'n_keys', kinds=KINDS[1:])


@pytest.mark.parametrize('field', ['last_seen', 'freq', 'step'])
def test_refuses_null_expiry_buffers(field):
  _refused([_col(), _col()], 'column 1', 'NULL expiry', kinds=['expiring', 'expiring_admit'],
           exps=[_exp(), _exp(**{field: None})])


def test_refuses_a_bad_filter():
  kinds = ['admit', 'expiring_admit']
  _refused([_col()], 'column 0', 'width', kinds=kinds, adms=[_adm(width=0)])
  _refused([_col()], 'column 0', 'depth', kinds=kinds, adms=[_adm(depth=9)])
  _refused([_col()], 'column 0', 'min_freq', kinds=kinds, adms=[_adm(min_freq=0)])
  _refused([_col()], 'column 0', 'sketch', kinds=kinds, adms=[_adm(sketch=None)])
  _refused([_col()], 'column 0', 'sketch', kinds=kinds, adms=[_adm(sketch=FAKE + 2)])


# ---- what only the 16-bit entry refuses -------------------------------------------------------------------------
def test_refuses_null_table_dtypes():
  _refused([_col()], 'table_dtypes', null_dtypes=True)


@pytest.mark.parametrize('bad', [0, 3, -1, 16])
def test_refuses_an_unknown_element_code(bad):
  _refused([_col(), _col()], 'column 1', 'table_dtypes', codes=[FP16, bad])


@pytest.mark.parametrize('code', [BF16, FP16])
def test_refuses_rows_that_are_no_whole_words(code):
  _refused([_col(), _col(dim=15)], 'column 1', 'dim', codes=[code] * 2)
  _refused([_col(dim=1)], 'column 0', 'dim', codes=[code])
  _refused([_col(dim=16, table_pitch=17)], 'column 0', 'table_pitch', codes=[code])
  _refused([_col(table=FAKE4 + 4098)], 'column 0', 'table', 'aligned', codes=[code])


def test_a_column_without_a_table_may_have_any_dim():
  # (no row is written: the shape of a row is not looked at -- but nothing is launched on a fake address either)
  rc, msg = _call([_col(n_keys=0, table=None, dim=15, table_pitch=0)], 'plain', [BF16], 1)
  assert rc == _lib.OK, msg


def test_refuses_an_fp16_scale_that_rounds_to_infinity():
  _refused([_col(), _col(init_scale=65505.0)], 'column 1', 'init_scale', '65504', codes=[FP16, FP16])
  # bf16 has fp32's range; fp16 takes its largest finite value
  for code, scale in ((BF16, 65505.0), (BF16, 1e30), (FP16, 65504.0)):
    rc, msg = _call([_col(n_keys=0, init_scale=scale)], 'plain', [code], 1)
    assert rc == _lib.OK, (code, scale, msg)


def test_nothing_to_do_is_ok():
  lib = _lib.lib()
  for insert in (1, 0):
    assert lib.hbk_hash_insert_lowp_n(0, None, None, None, None, insert, None) == _lib.OK
  # no keys: NULL buffers are fine and nothing is launched, for every kind
  cols = [_col(n_keys=0, keys=None, slots=None, keys_cache=None), _col(n_keys=0, table=None, dim=0)]
  for kind in KINDS:
    for insert in (1, 0):
      exps = [_exp(last_seen=None, freq=None, step=None) for _ in cols]
      adms = [_adm(sketch=None) for _ in cols]
      rc, msg = _call(cols, kind, [BF16, FP16], insert, exps, adms)
      assert rc == _lib.OK, (kind, msg)


# ---- Python argument handling ---------------------------------------------------------------------------------
@pytest.mark.parametrize('device', ['cpu', 'meta'])
def test_hashtable_dtype_and_its_refusals(device):
  t = hb.embedding.HashTable(64, 8, device)
  assert t.dtype == torch.float32 and t.table.dtype == torch.float32            # the default: nothing changes
  for dtype in LOWP:
    t = hb.embedding.HashTable(100, 6, device, slab_size=16, dtype=dtype, expiring=True, min_freq=2)
    assert t.dtype == dtype and t.table.dtype == dtype and tuple(t.table.shape) == (96, 6)
    assert t.variables('u')['u/embedding_weights'] is t.table
    assert t.last_seen.dtype == torch.int32 and t.sketch.dtype == torch.int32
  for dtype in (torch.float64, torch.int16, torch.float8_e4m3fn, None, 'bfloat16'):
    with pytest.raises(_lib.InvalidArgumentError, match='dtype'):
      hb.embedding.HashTable(64, 8, device, dtype=dtype)
  for dtype in LOWP:
    with pytest.raises(_lib.InvalidArgumentError, match='dim must be even'):
      hb.embedding.HashTable(64, 7, device, dtype=dtype)
  with pytest.raises(_lib.InvalidArgumentError, match='65504'):
    hb.embedding.HashTable(64, 8, device, dtype=torch.float16, init_scale=65505.0)
  hb.embedding.HashTable(64, 8, device, dtype=torch.float16, init_scale=65504.0)
  hb.embedding.HashTable(64, 8, device, dtype=torch.bfloat16, init_scale=1e30)
  hb.embedding.HashTable(64, 7, device, dtype=torch.float32)                    # odd dims stay fine in fp32


def test_the_plan_groups_by_kind_and_element_size():
  mk = hb.embedding.HashTable
  tables = [mk(64, 8, 'meta'), mk(64, 8, 'meta', dtype=torch.bfloat16), mk(64, 8, 'meta', expiring=True),
            mk(64, 8, 'meta', dtype=torch.float16, expiring=True), mk(64, 8, 'meta', dtype=torch.float16),
            mk(64, 8, 'meta', dtype=torch.bfloat16, min_freq=2)]
  plan = _ht._Plan(tables)
  kinds = [(g[0], g[1], None if d is None else list(d)) for g, d in zip(plan.groups, plan.dtypes)]
  assert kinds == [(False, False, None), (True, False, None), (False, False, [BF16, FP16]), (False, True, [BF16]),
                   (True, False, [FP16])]
  assert all(c is not None for c in plan.cols)
  # fp32 tables alone: the groups the plan always made, no element codes
  plain = _ht._Plan(tables[::2][:2])
  assert [g[:2] for g in plain.groups] == [(False, False), (True, False)] and plain.dtypes == [None, None]
  # load() and import_items() bypass the filter
  assert [(g[1], list(d)) for g, d in zip(*(lambda p: (p.groups, p.dtypes))(_ht._Plan(tables[5:], admit=False)))] == \
      [(False, [BF16])]


def test_moves_are_described_in_words():
  mv = _lib.HashMove()
  for dtype, dim, words in ((torch.float32, 6, 6), (torch.bfloat16, 6, 3), (torch.float16, 16, 8)):
    a, b = torch.zeros((4, dim), dtype=dtype), torch.zeros((9, dim + 2), dtype=dtype)[:, :dim]
    _ht._describe_move(mv, per_slot=a, packed=b, to_packed=True)
    assert (mv.words, mv.src_pitch, mv.dst_pitch) == (words, words, words + (2 if dtype == torch.float32 else 1))
  a, b = torch.zeros(4, dtype=torch.int32), torch.zeros(9, dtype=torch.int32)
  _ht._describe_move(mv, per_slot=a, packed=b, to_packed=False)
  assert (mv.words, mv.src_pitch, mv.dst_pitch) == (1, 1, 1)
  with pytest.raises(_lib.InvalidArgumentError, match='4-byte words'):
    _ht._describe_move(mv, per_slot=torch.zeros((4, 3), dtype=torch.bfloat16),
                       packed=torch.zeros((4, 3), dtype=torch.bfloat16), to_packed=True)


def test_a_mixed_group_lookup_is_refused_by_name():
  a = hb.embedding.HashTable(64, 8, 'meta')
  b = hb.embedding.HashTable(64, 8, 'meta', dtype=torch.bfloat16)
  with pytest.raises(_lib.InvalidArgumentError, match='hash_translate') as e:
    hb.embedding.HashGroupLookup([a, b])
  assert 'table 0: fp32' in str(e.value) and 'table 1: torch.bfloat16' in str(e.value)


@pytest.mark.parametrize('dtype', LOWP)
def test_max_norms_on_a_16_bit_group_is_refused(dtype):
  t = hb.embedding.HashTable(64, 8, 'meta', dtype=dtype)
  with pytest.raises(_lib.InvalidArgumentError, match='max_norms is not supported for 16-bit tables'):
    hb.embedding.HashGroupLookup([t], max_norms=[1.0])


@pytest.mark.parametrize('dtype', LOWP)
def test_sequence_and_sharded_lookups_refuse_16_bit_tables(dtype):
  a = hb.embedding.HashTable(64, 8, 'meta')
  t = hb.embedding.HashTable(64, 8, 'meta', dtype=dtype)
  with pytest.raises(_lib.InvalidArgumentError, match='HashSequenceLookup: table 1 is a ' + str(dtype)):
    hb.embedding.HashSequenceLookup([a, t], max_lens=4)
  ids = [torch.zeros(4, dtype=torch.int64, device='meta')] * 2
  with pytest.raises(_lib.InvalidArgumentError, match='hash_translate_sequence: table 1 is a ' + str(dtype)):
    hb.embedding.hash_translate_sequence([a, t], ids, max_lens=4)
  with pytest.raises(_lib.InvalidArgumentError, match='ShardedHashGroupLookup: table 0 is a ' + str(dtype)):
    hb.embedding.ShardedHashGroupLookup([t, a], None)


@pytest.mark.parametrize('table_dtype,rows_dtype', [(torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16),
                                                    (torch.float16, torch.bfloat16), (torch.float16, torch.float32),
                                                    (torch.float32, torch.float16)])
def test_rows_of_another_dtype_are_refused_not_cast(table_dtype, rows_dtype):
  t = hb.embedding.HashTable(64, 8, 'meta', dtype=table_dtype, expiring=True)
  keys = torch.zeros(3, dtype=torch.int64, device='meta')
  rows = torch.zeros((3, 8), dtype=rows_dtype, device='meta')
  with pytest.raises(_lib.InvalidArgumentError, match='load: rows must be .*nothing is cast'):
    t.load(keys, rows)
  with pytest.raises(_lib.InvalidArgumentError, match='load: rows must be'):
    t.load_owned(keys, rows, 2, 0)
  with pytest.raises(_lib.InvalidArgumentError, match='import_items: exp.rows must be .*nothing is cast'):
    t.import_items(hb.embedding.HashExport(keys, rows))
  # the host tier: a store keeps one dtype and serves the table of that dtype
  store = hb.embedding.HashSpillStore(8, pin_memory=False, dtype=rows_dtype)
  with pytest.raises(_lib.InvalidArgumentError, match='nothing is cast'):
    t.spill_to(10, store)
  meta = torch.zeros(3, dtype=torch.int32)
  other = hb.embedding.HashSpillStore(8, pin_memory=False, dtype=table_dtype)
  with pytest.raises(_lib.InvalidArgumentError, match='put: exp.rows must be'):
    other.put(hb.embedding.HashExport(torch.arange(3), torch.zeros((3, 8), dtype=rows_dtype), meta, meta))


@pytest.mark.parametrize('dtype', LOWP)
def test_the_store_keeps_16_bit_rows_bit_for_bit(dtype):
  store = hb.embedding.HashSpillStore(4, slot_dims=(1,), pin_memory=False, dtype=dtype)
  rows = torch.arange(-6, 6, dtype=torch.float32).reshape(3, 4).mul(0.37).to(dtype)
  meta = torch.tensor([1, 2, 3], dtype=torch.int32)
  store.put(hb.embedding.HashExport(torch.tensor([30, 10, 20]), rows, meta, meta, [torch.ones((3, 1))]))
  got = store.take(torch.tensor([10, 30]))
  assert got.rows.dtype == dtype and got.keys.tolist() == [10, 30]
  assert torch.equal(got.rows.view(torch.int16), rows[[1, 0]].view(torch.int16))
  again = hb.embedding.HashSpillStore.from_variables('s', store.variables('s'), pin_memory=False)
  assert again.dtype == dtype and again.keys().tolist() == [20]
  assert hb.embedding.HashExport.empty(2, 4, dtype=dtype).rows.dtype == dtype


# ---- the oracle of the GPU tests ------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dtype', [(lowp_ref.BF16, torch.bfloat16), (lowp_ref.FP16, torch.float16)])
@pytest.mark.parametrize('scale', [1.0, 1e-3])
def test_the_oracle_is_torchs_cast_bit_for_bit(name, dtype, scale):
  rng = np.random.RandomState(5)
  keys = rng.randint(-2 ** 63, 2 ** 63 - 1, size=400, dtype=np.int64)
  for dim, seed in ((2, 0), (16, 9), (130, -3)):
    rows = hash_ref.init_rows(keys, dim, seed, scale)
    want = lowp_ref.round_nearest(lowp_ref.bits32(rows), name)
    assert want.dtype == np.uint16 and want.shape == (400, dim)
    cast = torch.from_numpy(rows).to(dtype).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(want, cast)
    assert len(np.unique(want)) > 100                                  # (not a table of zeros)
  zeros = hash_ref.init_rows(keys, 4, 7, 0.0)
  assert not lowp_ref.round_nearest(lowp_ref.bits32(zeros), name).any()   # init_scale 0: 0x0000


# ---- the forward's wide rows (hbk_lowp_lookup_column_t.wide_rows, the field that was reserved) -------------------
def test_wide_rows_is_the_reserved_word_and_takes_0_or_1():
  assert C.sizeof(_lib.LowpLookupColumn) == 104 and _lib.LowpLookupColumn.wide_rows.offset == 100
  assert _lib.LowpLookupColumn.wide_rows.offset == _lib.LowpLookupColumn.chunk_elems.offset + 4
  lib = _lib.lib()
  for bad in (2, -1):
    col = (_lib.LowpLookupColumn * 1)()
    col[0].table, col[0].table_dtype, col[0].dim, col[0].rows = FAKE, BF16, 130, 10
    col[0].ids, col[0].ids_dtype, col[0].n_ids, col[0].n_segments = FAKE2, _lib.INT64, 4, 4
    col[0].divisor, col[0].out, col[0].wide_rows = 1, FAKE3, bad
    assert lib.hbk_lowp_lookup_fwd(1, col, None) == _lib.INVALID_ARGUMENT
    msg = lib.hbk_last_error().decode()
    assert 'column 0' in msg and 'wide_rows' in msg, msg
  # 0, the value every caller passed so far, keeps the bound
  col[0].wide_rows = 0
  assert lib.hbk_lowp_lookup_fwd(1, col, None) == _lib.INVALID_ARGUMENT
  assert 'dim 130' in lib.hbk_last_error().decode() and '64 otherwise' in lib.hbk_last_error().decode()
  # with 1, a row beyond 256 elements is still refused
  col[0].wide_rows, col[0].dim = 1, 258
  assert lib.hbk_lowp_lookup_fwd(1, col, None) == _lib.INVALID_ARGUMENT
  assert 'dim 258' in lib.hbk_last_error().decode()
