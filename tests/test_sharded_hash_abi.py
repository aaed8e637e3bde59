"""hbk_sharded_set_hash_tables at the C ABI and the Python names of sharded hash tables, without a GPU: the
symbol, the struct as the header declares it, the exports.  Refusals that need a plan are in
tests/test_gpu_sharded_hash.py."""
import ctypes as C
import os
import re

import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'hbk.h')).read()


def _struct_fields(name):
  end = HEADER.index('} %s;' % name)
  body = HEADER[HEADER.rindex('typedef struct {', 0, end):end]
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return re.findall(r'(\w+)(?:\[\w+\])?;', body)


def test_symbol_prototype_and_struct_layout():
  lib = _lib.lib()
  assert hasattr(lib, 'hbk_sharded_set_hash_tables')
  assert lib.hbk_sharded_set_hash_tables.restype is C.c_int
  assert lib.hbk_sharded_set_hash_tables.argtypes == [C.c_void_p, C.c_void_p]
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  proto = re.search(r'int hbk_sharded_set_hash_tables\((.*?)\);', HEADER, flags=re.S).group(1)
  assert re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', proto)).strip() == \
      'hbk_sharded_t plan, const hbk_sharded_hash_t* tables'
  # pointer, int64, int32 (+4), pointer, float (+4), int64, the expiry record (4 pointers), the admission record
  # (pointer, int64, 2 int32, int64, pointer), int32 (+4)
  H = _lib.ShardedHash
  assert C.sizeof(_lib.HashExpiry) == 32 and C.sizeof(_lib.HashAdmission) == 40
  assert C.sizeof(H) == 48 + 32 + 40 + 8 == 128
  assert [H.keys_cache.offset, H.slab_count.offset, H.slab_size.offset, H.counts.offset, H.init_scale.offset,
          H.seed.offset, H.exp.offset, H.adm.offset, H.insert.offset] == [0, 8, 16, 24, 32, 40, 48, 80, 120]
  assert _struct_fields('hbk_sharded_hash_t') == [n for n, _ in H._fields_]
  # the sharded column is what it was
  assert C.sizeof(_lib.ShardedColumn) == 48


def test_null_plan_is_refused():
  lib = _lib.lib()
  assert lib.hbk_sharded_set_hash_tables(None, None) == _lib.INVALID_ARGUMENT
  assert 'sharded_set_hash_tables' in lib.hbk_last_error().decode()


def test_python_names():
  from hybridbackend_amd.embedding import sharded_hash
  assert hb.embedding.ShardedHashGroupLookup is sharded_hash.ShardedHashGroupLookup
  assert issubclass(hb.embedding.ShardedHashGroupLookup, hb.embedding.ShardedGroupLookup)
  for name in ('rebind', 'maybe_grow', 'p2p_bind'):
    assert name in vars(hb.embedding.ShardedHashGroupLookup)
  assert hasattr(hb.embedding.HashTable, 'load_owned')


def test_hash_owner_is_floormod():
  ids = torch.tensor([-7, -1, 0, 1, 5, 2 ** 40 + 3, -2 ** 63 + 1, 2 ** 63 - 1], dtype=torch.int64)
  for world in (1, 2, 3, 8):
    got = hb.embedding.hash_owner(ids, world).tolist()
    assert got == [int(i) % world for i in ids.tolist()]              # Python's % is floormod
    assert got == [_lib.lib().hbk_host_floormod_i64(int(i), world) for i in ids.tolist()]
  with pytest.raises(_lib.InvalidArgumentError, match='world'):
    hb.embedding.hash_owner(ids, 0)
