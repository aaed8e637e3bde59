"""The wide-offset case of the kernels that write 16-bit rows through the runs and the sequence entry
(hbk_hash_translate_runs_lowp_n, hbk_hash_translate_sequence_lowp_n), with the helpers of
tests/support/wide_offsets.py: a bf16 table of dim 256 and 2^23 + 1024 slots, whose row array crosses byte offset
2^31 at slot 2^22 and byte offset 2^32 at slot 2^23.  Keys are picked on the host (tests/support/hash_ref.py) so that
their home slabs lie below, between and past the two thresholds.  The table's rows are looked after by a WideTable:
random rows are planted at every alias row -- where a row address truncated to 31 or 32 bits would land -- and at the
slots the keys will take; afterwards the written rows must be the cast start rows, the alias rows what was planted,
and the whole rest of the 4 GiB array zero (scanned on the device: the array is never copied to the host)."""
import numpy as np
import pytest
import torch

from hybridbackend_amd.embedding import HashTable
from tests.support import hash_ref
from tests.support import wide_offsets as wo
from tests.support.hash_lowp import cast_rows, dev, host, translate_runs, translate_sequence

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DIM, SLAB, ES = 256, 8, 2
FAR = 1 << 23                                   # the first slot whose row starts at or past byte 2^32
MID = 1 << 22                                   # ... at or past byte 2^31
CAPACITY = FAR + 1024
SLABS = CAPACITY // SLAB
GEOM = wo.Geometry('hash16', DIM, DIM, CAPACITY)


def pick_keys():
  """6 keys whose home slab lies past byte 2^32, 4 past byte 2^31 and 4 below it (slabs 4096 .. 4223, away from every
  alias), at most one per slab: a key's slot is then the first of its home slab."""
  cand = np.arange(1, 1 + (1 << 22), dtype=np.int64) * np.int64(0x1E3779B97F4A7C15)
  home = hash_ref.murmur3_np(cand).astype(np.int64) % SLABS
  keys = []
  for lo, n in ((FAR // SLAB, 6), (MID // SLAB, 4), (4096, 4)):
    hit = np.nonzero((home >= lo) & (home < lo + 128))[0]
    _, first = np.unique(home[hit], return_index=True)
    assert first.size >= n, 'too few candidates: widen the search'
    keys.append(cand[hit[first[:n]]])
  return np.concatenate(keys)


@pytest.mark.parametrize('entry', ['runs', 'sequence'])
def test_rows_past_byte_offset_2_31_and_2_32_are_written_where_they_belong(entry):
  keys = pick_keys()
  probes = (hash_ref.murmur3_np(keys).astype(np.int64) % SLABS * SLAB).tolist()
  assert sum(s >= FAR for s in probes) == 6 and sum(MID <= s < FAR for s in probes) == 4
  aliases = sorted({a for s in probes for a in wo.alias_rows_of(GEOM, ES, s)} - set(probes))
  assert aliases and all(wo.mutant_can_differ(m, GEOM, ES) for m in ('byte_u32', 'byte_i32'))
  t = HashTable(CAPACITY, DIM, DEV, slab_size=SLAB, init_scale=1.0, seed=5, dtype=torch.bfloat16)
  assert t.capacity == CAPACITY and t.table.numel() * ES > wo.M32
  rng = np.random.RandomState(7)
  wt = wo.WideTable(GEOM, torch.bfloat16, DEV, over=t.table).plant(
    probes, aliases, rng.randint(1, 0x7F00, size=(len(probes) + len(aliases), DIM)).astype(np.uint16))
  if entry == 'runs':
    got = translate_runs([t], [[dev(keys[:5]), dev(keys[:0]), dev(keys[5:])]])
    slots = np.concatenate([host(x) for x in got[0]])
  else:
    # B = 4 samples of 5, 2, 4 and 5 ids with T = 4: the fifth ids are never read
    lens = np.array([5, 2, 4, 5])
    splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    extra = np.array([12345, 67890], np.int64)
    ids = np.concatenate([keys[:4], extra[:1], keys[4:6], keys[6:10], keys[10:14], extra[1:]])
    grids, _ = translate_sequence([t], [dev(ids)], [dev(splits)], 4, None)
    grid = host(grids[0]).reshape(4, 4)
    assert (grid[1, 2:] == -1).all()
    slots = np.concatenate([grid[0], grid[1, :2], grid[2], grid[3]])
    assert (host(t.find(dev(extra))) == -1).all()
  np.testing.assert_array_equal(slots, np.array(probes))     # the first slot of the home slab
  np.testing.assert_array_equal(host(t.keys[dev(slots)]), keys)
  assert t.size() == keys.size
  np.testing.assert_array_equal(wt.rows(slots), cast_rows(keys, DIM, 5, 1.0, torch.bfloat16))
  wt.assert_rest_untouched(slots.tolist(), entry)
