"""hbk_hash_insert_quant8_n at the C ABI, without a GPU: the symbol, and every refusal before any device work."""
import ctypes as C

import pytest

from hybridbackend_amd import _lib

FAKE = 0x7f0000001000      # device-looking addresses: validation must refuse before touching them


def _call(pitches, insert=1, **bad):
  """Two columns, the second with `bad`; returns (status, message)."""
  cols = (_lib.HashColumn * 2)()
  for k, col in enumerate(cols):
    col.keys_cache, col.slab_count, col.slab_size = FAKE, 8, 16
    col.keys, col.n_keys, col.slots, col.counts = FAKE + 0x100000, 100, FAKE + 0x200000, FAKE + 0x300000
    col.table, col.dim, col.table_pitch, col.init_scale, col.seed = FAKE + 0x400000, 16, 0, 1e-3, 0
    for name, v in (bad.items() if k else ()):
      setattr(col, name, v)
  lib = _lib.lib()
  p = (C.c_int32 * 2)(*pitches) if pitches is not None else None
  return lib.hbk_hash_insert_quant8_n(2, cols, None, None, p, insert, None), lib.hbk_last_error().decode()


@pytest.mark.parametrize('bad,pitch,word', [
  (dict(dim=0), 0, 'dim'), (dict(dim=257), 0, 'dim 257'), (dict(dim=260), 0, 'dim 260'), (dict(dim=66), 0, 'dim 66'),
  (dict(dim=6), 10, 'pitch 10'), (dict(dim=6), 8, 'pitch 8'), (dict(dim=16), 16, 'pitch 16'),
  (dict(table=FAKE + 0x400002), 0, 'aligned'), (dict(slab_size=65), 0, 'slab_size'), (dict(n_keys=-1), 0, 'n_keys')])
def test_refusals_name_the_entry_and_the_column(bad, pitch, word):
  for insert in (1, 0):
    rc, msg = _call([0, pitch], insert, **bad)
    assert rc == _lib.INVALID_ARGUMENT and 'hash_insert_quant8_n' in msg and 'column 1' in msg and word in msg, msg


def test_the_symbol_is_new_null_pitches_are_refused_and_nothing_to_do_is_ok():
  lib = _lib.lib()
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950' and C.sizeof(_lib.HashColumn) == 88
  rc, msg = _call(None)
  assert rc == _lib.INVALID_ARGUMENT and 'hash_insert_quant8_n: pitches is NULL' in msg
  assert lib.hbk_hash_insert_quant8_n(0, None, None, None, None, 1, None) == _lib.OK
