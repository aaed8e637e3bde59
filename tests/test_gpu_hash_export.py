"""Export and import of hash tables on the GPU (hbk_hash_export_n, hbk_hash_store_rows_n, HashTable.export_items /
import_items, hash_export, ShardedHashGroupLookup.export_items / import_items).

The export is a function of the table's arrays alone (ascending slot order, no atomics), so it is compared BIT FOR
BIT with the numpy restatement of tests/support/hash_export_ref.py computed from the arrays read back after
filling.  Round trips are compared as key -> payload maps: slot numbers are the destination table's own."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (GroupLookupGrad, HashExport, HashGroupLookup, HashTable,
                                         ShardedHashGroupLookup, hash_export)
from tests.support import hash_export_ref as xref
from tests.support import hash_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
EMPTY, TOMB = xref.EMPTY, xref.TOMBSTONE
SENT32, SENT64, GUARD = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a, 4


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def distinct_keys(rng, n):
  """n distinct int64 keys over the full range, neither sentinel among them."""
  k = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=2 * n + 8, dtype=np.int64))
  rng.shuffle(k)
  return k[:n]


def fill(t, rng, n, keys=None):
  """n keys into t -- on an expiring table spread over steps 1..5, some seen twice -- and EVERY row of the table
  random (the rows no key holds too: an export must not pick them up).  Returns the keys."""
  keys = distinct_keys(rng, n) if keys is None else keys
  if t.expiring:
    for s, part in enumerate(np.array_split(keys, 5)):
      t.set_step(s + 1)
      if part.size == 0:
        continue
      got = t.lookup_or_insert(dev(np.concatenate([part, part[:part.size // 3]])))
      assert bool((got >= 0).all().item())
  elif keys.size:
    assert bool((t.lookup_or_insert(dev(keys)) >= 0).all().item())
  t.table.copy_(dev(rng.randn(t.capacity, t.dim).astype(F32)))
  return keys


def companions(t, rng, dims=(3, 16)):
  """Companions whose widths differ from the table's: the first a strided view (rows at a pitch of d + 2)."""
  out = []
  for n, d in enumerate(dims):
    x = dev(rng.randn(t.capacity, d + (2 if n == 0 else 0)).astype(F32))
    out.append(x[:, :d] if n == 0 else x)
  return out


def arrays_of(t, comps=()):
  return [t.table] + ([t.last_seen, t.freq] if t.expiring else []) + list(comps)


def restate(t, comps=(), since=0, out_capacity=None):
  """(count, keys, slots, packed arrays) of the table as it is now."""
  return xref.export(host(t.keys), t.expiring, [host(x) for x in arrays_of(t, comps)],
                     host(t.last_seen) if t.expiring else None, since, out_capacity)


def words_of(x):
  return 1 if x.dim() == 1 else x.shape[1]


class Raw:
  """One column of hbk_hash_export_n by hand: every output buffer has GUARD rows of a sentinel pattern behind its
  out_capacity rows, and the first move's destination a pitch wider than its words."""

  def __init__(self, t, arrays, since, out_capacity):
    rows = out_capacity + GUARD
    self.n_out = out_capacity
    self.keys = torch.full((rows,), SENT64, dtype=torch.int64, device=DEV)
    self.slots = torch.full((rows,), SENT64, dtype=torch.int64, device=DEV)
    self.count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    self.col = (_lib.HashExportColumn * 1)()
    col = self.col[0]
    col.keys, col.slab_count, col.slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
    col.expiring = 1 if t.expiring else 0
    col.last_seen = t.last_seen.data_ptr() if t.expiring else None
    col.since, col.n_moves = since, len(arrays)
    self.bufs, self.words = [], []
    for m, x in enumerate(arrays):
      w = words_of(x)
      pad = (4 if w % 4 == 0 else 2) if m == 0 else 0
      buf = torch.full((rows, w + pad), SENT32, dtype=torch.int32, device=DEV)
      mv = col.moves[m]
      mv.src, mv.dst, mv.words = x.data_ptr(), buf.data_ptr(), w
      mv.src_pitch, mv.dst_pitch = (1 if x.dim() == 1 else x.stride(0)), w + pad
      self.bufs.append(buf)
      self.words.append(w)
    col.out_keys, col.out_slots, col.out_capacity = self.keys.data_ptr(), self.slots.data_ptr(), out_capacity
    col.count = self.count.data_ptr()
    nbytes = C.c_size_t()
    _lib.check(_lib.lib().hbk_hash_export_workspace_bytes(1, self.col, C.byref(nbytes)))
    assert nbytes.value == 8 * ((t.capacity + 255) // 256)
    self.workspace = torch.empty(nbytes.value // 8, dtype=torch.int64, device=DEV)

  def launch(self):
    _lib.check(_lib.lib().hbk_hash_export_n(1, self.col, self.workspace.data_ptr(),
                                            _lib.current_stream(torch.device(DEV))))

  def check(self, want):
    count, keys, slots, packed = want
    n = min(count, self.n_out)
    assert int(self.count.item()) == count
    assert keys.size == n
    got_keys, got_slots = host(self.keys), host(self.slots)
    np.testing.assert_array_equal(got_slots[:n], slots)
    assert (np.diff(got_slots[:n]) > 0).all()                                # strictly ascending
    np.testing.assert_array_equal(got_keys[:n], keys)
    assert (got_keys[n:] == SENT64).all() and (got_slots[n:] == SENT64).all()     # the guard rows
    for buf, w, p in zip(self.bufs, self.words, packed):
      got = host(buf)
      assert got[:n, :w].tobytes() == np.ascontiguousarray(p).view(np.int32).reshape(n, w).tobytes()
      assert (got[n:] == SENT32).all() and (got[:, w:] == SENT32).all()      # guard rows and padding


def check_raw(t, comps=(), since=0, out_capacity=None):
  """The C entry against the restatement, buffers sized to the matches (or to out_capacity), guards behind them."""
  want = restate(t, comps, since, out_capacity)
  raw = Raw(t, arrays_of(t, comps), since, want[0] if out_capacity is None else out_capacity)
  raw.launch()
  raw.check(want)
  return want


def check_export(e, t, want, since=0):
  """A HashExport against the restatement, bit for bit."""
  count, keys, slots, packed = want
  assert len(e) == count and e.since == max(since, 0)
  np.testing.assert_array_equal(host(e.keys), keys)
  np.testing.assert_array_equal(host(e.src_slots), slots)
  got = [e.rows] + ([e.last_seen, e.freq] if t.expiring else []) + e.slots
  assert (e.last_seen is None) == (not t.expiring) and (e.freq is None) == (not t.expiring)
  assert len(got) == len(packed)
  for g, p in zip(got, packed):
    assert host(g).dtype == p.dtype and host(g).shape == p.shape and host(g).tobytes() == p.tobytes()


def state_map(t, comps=()):
  """key -> payload bytes of the table as it is now, read through the restatement."""
  _, keys, _, packed = restate(t, comps)
  return xref.as_map(keys, *packed)


def export_map(e):
  meta = [e.last_seen, e.freq] if e.last_seen is not None else []
  return xref.as_map(host(e.keys), *[host(x) for x in [e.rows] + meta + e.slots])


# ---- 1. bit equality across geometries ------------------------------------------------------------------
@pytest.mark.parametrize('dim', [4, 19])
@pytest.mark.parametrize('capacity', [259, 512, 1000])
@pytest.mark.parametrize('slab_size', [1, 7, 8, 64])
def test_export_equals_the_restatement_across_geometries(slab_size, capacity, dim):
  rng = np.random.RandomState(1000 * slab_size + capacity + dim)
  t = HashTable(capacity, dim, DEV, slab_size=slab_size, expiring=True)
  fill(t, rng, 3 * t.capacity // 5)
  comps = companions(t, rng)
  want = check_raw(t, comps)
  assert want[0] == t.size() == 3 * t.capacity // 5
  check_export(t.export_items(slots=comps), t, want)
  check_export(t.export_items(), t, restate(t))
  # a delta through both ways: the keys of steps 3, 4 and 5
  delta = check_raw(t, comps, since=3)
  assert 0 < delta[0] < want[0]
  check_export(t.export_items(since=3, slots=comps), t, delta, since=3)


# ---- 2. occupancy ---------------------------------------------------------------------------------------
def test_an_empty_table_a_full_table_and_whole_empty_tiles():
  rng = np.random.RandomState(2)
  empty = HashTable(512, 4, DEV)
  want = check_raw(empty)
  assert want[0] == 0
  assert len(empty.export_items()) == 0
  # filled to the last slot
  full = HashTable(1000, 4, DEV, slab_size=8)
  fill(full, rng, 1000)
  assert int((full.keys == int(EMPTY)).sum().item()) == 0
  want = check_raw(full)
  assert want[0] == 1000 and want[2].tolist() == list(range(1000))
  check_export(full.export_items(), full, want)
  # keys homed in two far-apart slabs: the tiles between them count nothing
  far = HashTable(2048, 4, DEV, slab_size=8)
  pool = distinct_keys(rng, 6000)
  home = ref.murmur3_np(pool).astype(np.int64) % far.slab_count
  keys = np.concatenate([pool[home == 3][:6], pool[home == 200][:6]])
  assert keys.size == 12
  fill(far, rng, 12, keys=keys)
  want = check_raw(far)
  assert want[0] == 12 and sorted(set((want[2] // 256).tolist())) == [0, 6]
  check_export(far.export_items(), far, want)


def test_no_tombstone_is_exported_and_a_plain_table_exports_the_tombstone_key():
  rng = np.random.RandomState(3)
  t = HashTable(1000, 4, DEV, slab_size=8, expiring=True)
  keys = distinct_keys(rng, 400)
  t.set_step(1)
  t.lookup_or_insert(dev(keys[:100]))
  t.set_step(5)
  t.lookup_or_insert(dev(keys[100:]))
  t.set_step(6)
  accum = dev(rng.randn(1000, 4).astype(F32))
  t.evict(3, slots=[(accum, 0.1)])
  assert (t.tombstones(), t.size()) == (100, 300)
  want = check_raw(t, [accum])
  assert want[0] == 300 and not np.isin(want[1], [EMPTY, TOMB]).any()
  np.testing.assert_array_equal(np.sort(want[1]), np.sort(keys[100:]))
  check_export(t.export_items(slots=[accum]), t, want)
  plain = HashTable(259, 4, DEV, slab_size=7)
  fill(plain, rng, 21, keys=np.concatenate([keys[:20], [TOMB]]))
  want = check_raw(plain)
  assert want[0] == 21 and int(TOMB) in want[1].tolist()
  check_export(plain.export_items(), plain, want)


# ---- 3. deltas -----------------------------------------------------------------------------------------
def test_deltas_take_exactly_the_keys_seen_since_a_step():
  rng = np.random.RandomState(4)
  t = HashTable(1000, 19, DEV, slab_size=8, expiring=True)
  keys = fill(t, rng, 500)
  comps = companions(t, rng)
  by_step = np.array_split(keys, 5)                                          # step s + 1 saw by_step[s]
  since3 = check_raw(t, comps, since=3)
  assert since3[0] == 300
  np.testing.assert_array_equal(np.sort(since3[1]), np.sort(np.concatenate(by_step[2:])))
  assert np.isin(by_step[2], since3[1]).all() and not np.isin(by_step[1], since3[1]).any()
  check_export(t.export_items(since=3, slots=comps), t, since3, since=3)
  for since in (0, -1):
    assert check_raw(t, comps, since=since)[0] == 500
    check_export(t.export_items(since=since, slots=comps), t, restate(t, comps), since=since)
  assert check_raw(t, comps, since=6)[0] == 0
  assert len(t.export_items(since=6, slots=comps)) == 0


# ---- 4. truncation --------------------------------------------------------------------------------------
def test_an_output_too_small_gets_the_first_keys_in_slot_order_and_the_total_count():
  rng = np.random.RandomState(5)
  t = HashTable(1000, 4, DEV, slab_size=8, expiring=True)
  fill(t, rng, 600)
  comps = companions(t, rng)
  for out_capacity in (0, 1, 63, 64, 257, 599):
    want = check_raw(t, comps, out_capacity=out_capacity)
    assert want[0] == 600 and want[1].size == out_capacity
  assert check_raw(t, comps, since=3, out_capacity=100)[0] == 360
  # stale counters (a restore of the raw arrays): more matches than promised is refused, recount() cures it
  t.counts[0] = 100
  with pytest.raises(_lib.InvalidArgumentError, match=r'600 keys match but the counters promise 100.*recount\(\)'):
    t.export_items()
  t.recount()
  check_export(t.export_items(slots=comps), t, restate(t, comps))


# ---- 5. many tables, one call ---------------------------------------------------------------------------
def test_40_tables_of_mixed_kinds_geometries_and_since_values_in_one_call():
  rng = np.random.RandomState(6)
  tables, comps, sinces = [], [], []
  for c in range(40):
    slab_size = (5, 8, 16, 64)[c % 4]
    kind = c % 4                                                             # plain, expiring, filtered, both
    t = HashTable(slab_size * (3 + c % 11), (4, 19, 16)[c % 3], DEV, slab_size=slab_size, expiring=kind in (1, 3),
                  min_freq=1 if kind >= 2 else 0, sketch_width=1 << 10)
    fill(t, rng, (t.capacity * (c % 5)) // 5)                               # some of them empty
    tables.append(t)
    comps.append(companions(t, rng, dims=(3, 16)[:c % 3]))
    sinces.append(None if not t.expiring else 6 if c % 8 == 1 else (None, 3, 0, 5)[(c // 4) % 4])
  got = hash_export(tables, sinces, comps)
  assert len(got) == 40
  for c, (t, e) in enumerate(zip(tables, got)):
    since = sinces[c] or 0
    check_export(e, t, restate(t, comps[c], since), since=since)


# ---- 6. round trips -------------------------------------------------------------------------------------
def test_a_change_of_geometry_keeps_every_keys_payload_and_leaves_the_sketch_alone():
  rng = np.random.RandomState(7)
  src = HashTable(512, 19, DEV, slab_size=8, expiring=True)
  keys = fill(src, rng, 300)
  comps = companions(src, rng)
  e = src.export_items(slots=comps)
  dst = HashTable(1000, 19, DEV, slab_size=5, expiring=True, min_freq=2, sketch_width=1 << 10)
  dst.set_step(9)
  dst_comps = [torch.full((dst.capacity, 3), 0.5, device=DEV), torch.full((dst.capacity, 16), 0.25, device=DEV)]
  slots = dst.import_items(e, slots=dst_comps)
  np.testing.assert_array_equal(host(dst.find(dev(host(e.keys)))), host(slots))
  found = host(dst.find(dev(keys)))
  assert (found >= 0).all() and np.unique(found).size == keys.size
  assert state_map(dst, dst_comps) == state_map(src, comps) == export_map(e)
  assert dst.size() == src.size() == 300
  assert not host(dst.sketch).any() and dst.filtered() == 0
  free = np.setdiff1d(np.arange(dst.capacity), found)
  assert (host(dst_comps[0])[free] == F32(0.5)).all() and (host(dst_comps[1])[free] == F32(0.25)).all()
  # an export WITHOUT metadata into an expiring table leaves load()'s stamp; one WITH metadata into a plain table
  # drops it
  bare = HashExport(e.keys, e.rows)
  stamped = HashTable(512, 19, DEV, expiring=True)
  stamped.set_step(9)
  s = host(stamped.import_items(bare))
  assert (host(stamped.last_seen)[s] == 9).all() and (host(stamped.freq)[s] == 1).all()
  plain = HashTable(512, 19, DEV)
  plain.import_items(HashExport(e.keys, e.rows, e.last_seen, e.freq))
  assert state_map(plain) == xref.as_map(host(e.keys), host(e.rows))


def test_an_import_is_an_upsert_that_reuses_tombstones():
  rng = np.random.RandomState(8)
  src = HashTable(512, 4, DEV, slab_size=8, expiring=True)
  keys = fill(src, rng, 300)
  comps = companions(src, rng)
  e = src.export_items(slots=comps)
  dst = HashTable(504, 4, DEV, slab_size=7, expiring=True)
  held, doomed = keys[:150], distinct_keys(np.random.RandomState(80), 600)
  doomed = doomed[~np.isin(doomed, keys)][:200]
  dst.set_step(1)
  assert bool((dst.lookup_or_insert(dev(doomed)) >= 0).all().item())
  dst.set_step(5)
  held_slots = host(dst.lookup_or_insert(dev(held)))
  dst.table.copy_(dev(rng.randn(dst.capacity, 4).astype(F32)))               # rows that are not the export's
  dst_comps = [torch.full((dst.capacity, 3), 0.5, device=DEV), torch.full((dst.capacity, 16), 0.25, device=DEV)]
  dst.set_step(6)
  dst.evict(3)
  assert (dst.tombstones(), dst.size(), dst.reused()) == (200, 150, 0)
  inserted = int(dst.counts[0].item())
  dst.import_items(e, slots=dst_comps)
  np.testing.assert_array_equal(host(dst.find(dev(held))), held_slots)       # the held keys keep their slots
  assert int(dst.counts[0].item()) == inserted + 150                         # the new keys only
  assert dst.size() == 300 and dst.reused() > 0 and dst.failed() == 0
  assert state_map(dst, dst_comps) == export_map(e)
  # importing the same export again changes nothing
  dst.import_items(e, slots=dst_comps, assume_distinct=True)
  assert dst.size() == 300 and state_map(dst, dst_comps) == export_map(e)


def test_a_destination_too_small_stores_what_fits_completely_and_names_the_count():
  rng = np.random.RandomState(9)
  src = HashTable(512, 19, DEV, slab_size=8, expiring=True)
  fill(src, rng, 200)
  comps = companions(src, rng)
  e = src.export_items(slots=comps)
  dst = HashTable(64, 19, DEV, slab_size=8, expiring=True)
  dst_comps = [torch.zeros((64, 3), device=DEV), torch.zeros((64, 16), device=DEV)]
  with pytest.raises(_lib.InvalidArgumentError, match='136 of 200 keys do not fit'):
    dst.import_items(e, slots=dst_comps)
  assert dst.size() == 64
  got, want = state_map(dst, dst_comps), export_map(e)
  assert len(got) == 64 and all(want[k] == v for k, v in got.items())        # every key found has its full payload


# ---- 7. training across a checkpoint ------------------------------------------------------------------
def test_training_across_a_checkpoint_equals_uninterrupted_training():
  rng = np.random.RandomState(10)
  dim, lr, acc0, n_ids, k, fresh = 8, 0.1, 0.1, 64, 4, 20
  splits = [None, dev(np.arange(0, n_ids + 1, 2, dtype=np.int32))]
  pools = [distinct_keys(rng, 2 * k * fresh) for _ in range(2)]
  batches = []
  for s in range(2 * k):
    ids = []
    for p in pools:
      new, seen = p[s * fresh:(s + 1) * fresh], p[:(s + 1) * fresh]
      one = np.concatenate([new, seen[rng.randint(0, seen.size, size=n_ids - fresh)]])
      rng.shuffle(one)
      ids.append(one)
    batches.append((ids, [rng.randn(n_ids, dim).astype(F32), rng.randn(n_ids // 2, dim).astype(F32)]))

  def make(capacities, slab_sizes):
    tables = [HashTable(capacities[c], dim, DEV, slab_size=slab_sizes[c], init_scale=0.05, seed=3 + c) for c in range(2)]
    return tables, [torch.full_like(t.table, acc0) for t in tables]

  def train(tables, accums, steps):
    hgl = HashGroupLookup(tables, combiners=['sum', 'mean'], max_norms=[0.1, None])
    grad = GroupLookupGrad(hgl.lookup, accums=accums, deterministic=True)
    for ids, grads in steps:
      hgl([dev(i) for i in ids], splits)
      assert all(bool((s >= 0).all().item()) for s in hgl.slots)
      grad(hgl.slots, [dev(g) for g in grads], splits, apply_lr=lr, optimizer='adagrad')

  whole, whole_accums = make([512, 500], [8, 5])
  train(whole, whole_accums, batches)
  first, first_accums = make([512, 500], [8, 5])
  train(first, first_accums, batches[:k])
  exports = hash_export(first, slots=[[a] for a in first_accums])
  items = [t.items() for t in first]
  # through export / import, into tables of another geometry
  second, second_accums = make([640, 400], [16, 8])
  for t, a, e in zip(second, second_accums, exports):
    t.import_items(e, slots=[a])
  train(second, second_accums, batches[k:])
  # through items() / load(): the accumulators start again
  lossy, lossy_accums = make([640, 400], [16, 8])
  for t, (keys, rows) in zip(lossy, items):
    t.load(keys, rows)
  train(lossy, lossy_accums, batches[k:])
  for c in range(2):
    assert whole[c].size() == second[c].size() == 2 * k * fresh
    assert state_map(second[c], [second_accums[c]]) == state_map(whole[c], [whole_accums[c]])
    assert state_map(lossy[c], [lossy_accums[c]]) != state_map(whole[c], [whole_accums[c]])   # the gap this closes


# ---- 8. base plus delta ---------------------------------------------------------------------------------
def test_a_base_and_a_delta_restore_the_trained_table():
  rng = np.random.RandomState(11)
  t = HashTable(1000, 8, DEV, slab_size=8, expiring=True)
  accum = torch.full((1000, 8), 0.1, device=DEV)
  pool = distinct_keys(rng, 500)

  def step(s, ids):
    """What a training step does to the table: the translate stamps the slots, the backward writes their rows."""
    t.set_step(s)
    slots = torch.unique(t.lookup_or_insert(dev(ids)))
    assert bool((slots >= 0).all().item())
    t.table[slots] += dev(rng.randn(slots.numel(), 8).astype(F32))
    accum[slots] += dev(rng.rand(slots.numel(), 8).astype(F32))

  for s in (1, 2, 3):
    step(s, pool[rng.randint(0, 300, size=200)])
  s0 = 3
  base = t.export_items(slots=[accum])
  for s in (4, 5, 6):                                                        # old keys and new ones; no eviction
    step(s, np.concatenate([pool[rng.randint(0, 300, size=40)], pool[300 + (s - 4) * 60:300 + (s - 3) * 60]]))
  delta = t.export_items(since=s0 + 1, slots=[accum])
  full = t.export_items(slots=[accum])
  assert 0 < len(delta) < len(full) and len(full) > len(base)
  assert int(delta.last_seen.min().item()) > s0 and delta.since == s0 + 1
  untouched = ~np.isin(host(full.keys), host(delta.keys))
  assert (host(full.last_seen)[untouched] <= s0).all()
  fresh = HashTable(640, 8, DEV, slab_size=5, expiring=True)
  fresh_accum = torch.full((640, 8), 0.1, device=DEV)
  fresh.import_items(base, slots=[fresh_accum])
  assert state_map(fresh, [fresh_accum]) == export_map(base)
  fresh.import_items(delta, slots=[fresh_accum])
  assert state_map(fresh, [fresh_accum]) == export_map(full) == state_map(t, [accum])
  assert fresh.size() == t.size() == len(full)
  assert xref.upsert(export_map(base), host(delta.keys), host(delta.rows), host(delta.last_seen), host(delta.freq),
                     host(delta.slots[0])) == export_map(full)


# ---- 9. resharding --------------------------------------------------------------------------------------
DIMS, COMB, SEEDS, SCALE, SLAB, CAP = [16, 6], ['mean', 'sum'], [3, 4], 0.05, [16, 5], [512, 500]


def run_world(world, fn):
  """fn(rank, comm) on `world` host threads, each on a stream of its own; returns the per-rank results."""
  comms = hb.distribute.Collective.local_world(world)
  results, errors = [None] * world, []

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        results[r] = fn(r, comms[r])
        torch.cuda.current_stream().synchronize()
    except Exception as e:  # pylint: disable=broad-except
      import traceback
      errors.append((r, repr(e), traceback.format_exc()))

  threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=45)
  for cm in comms:
    cm.close()
  assert not errors, errors
  assert all(x is not None for x in results)
  return results


def test_exports_of_two_ranks_restore_onto_three_with_their_optimizer_state():
  rng = np.random.RandomState(12)
  n, lr = 300, 0.5
  pools = [np.unique(np.concatenate([rng.randint(-2 ** 62, 0, size=60, dtype=np.int64),
                                     rng.randint(0, 1000, size=60, dtype=np.int64),
                                     rng.randint(2 ** 40, 2 ** 62, size=80, dtype=np.int64)])) for _ in range(2)]
  ids = [[p[rng.randint(0, p.size, size=n)] for p in pools] for _ in range(2)]
  grads = [[rng.randn(n, d).astype(F32) for d in DIMS] for _ in range(2)]

  def make():
    tables = [HashTable(CAP[c], DIMS[c], DEV, slab_size=SLAB[c], init_scale=SCALE, seed=SEEDS[c], expiring=True)
              for c in range(2)]
    return tables, [torch.full_like(t.table, 0.1) for t in tables]

  def rank_a(r, comm):
    tables, accums = make()
    drv = ShardedHashGroupLookup(tables, comm, combiners=COMB, accums=accums)
    for s in (1, 2):
      for t in tables:
        t.set_step(s)
      drv([dev(i) for i in ids[r]], [None, None])
      drv.backward([dev(g) for g in grads[r]], apply_lr=lr, optimizer='adagrad', emit=False)
    for t in tables:
      t.set_step(3)
    outs = [host(o) for o in drv([dev(i) for i in ids[r]], [None, None])]
    exports = drv.export_items()
    assert all(len(e.slots) == 1 for e in exports)
    res = dict(outs=outs, exports=[HashExport(*[x.cpu() for x in (e.keys, e.rows, e.last_seen, e.freq)],
                                              [e.slots[0].cpu()], e.src_slots.cpu(), e.since) for e in exports])
    drv.close()
    return res

  two = run_world(2, rank_a)
  merged = [HashExport.cat([two[r]['exports'][c] for r in range(2)]) for c in range(2)]
  want = [export_map(m) for m in merged]
  for c in range(2):
    assert (np.mod(host(two[0]['exports'][c].keys), 2) == 0).all()
    assert len(want[c]) == np.unique(np.concatenate([ids[0][c], ids[1][c]])).size

  def rank_b(r, comm):
    tables, accums = make()
    drv = ShardedHashGroupLookup(tables, comm, combiners=COMB, accums=accums)
    drv.import_items(merged)
    state = [state_map(t, [a]) for t, a in zip(tables, accums)]
    for t in tables:
      t.set_step(3)
    q = r % 2                                                # ranks 0 and 1 repeat the 2-rank batches, rank 2 rank 0's
    outs = [host(o) for o in drv([dev(i) for i in ids[q]], [None, None])]
    res = dict(outs=outs, state=state, sizes=[t.size() for t in tables])
    drv.close()
    return res

  three = run_world(3, rank_b)
  for c in range(2):
    together = {}
    for r in range(3):
      assert all(k % 3 == r for k in three[r]['state'][c])                   # floormod(id, 3): Python's % on ints
      assert three[r]['sizes'][c] == len(three[r]['state'][c])
      together.update(three[r]['state'][c])
      np.testing.assert_array_equal(three[r]['outs'][c], two[r % 2]['outs'][c])
    assert sum(len(three[r]['state'][c]) for r in range(3)) == len(want[c])
    assert together == want[c]                                               # row, last_seen, freq, accumulator


# ---- 10. a captured graph -------------------------------------------------------------------------------
def test_a_captured_export_replays_on_the_tables_new_contents():
  rng = np.random.RandomState(13)
  t = HashTable(1000, 4, DEV, slab_size=8, expiring=True)
  keys = distinct_keys(rng, 500)
  fill(t, rng, 200, keys=keys[:200])
  comps = companions(t, rng)
  raw = Raw(t, arrays_of(t, comps), 0, 600)
  stream = torch.cuda.Stream()
  stream.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(stream):
    raw.launch()                                                             # warm up outside the capture
  torch.cuda.current_stream().wait_stream(stream)
  raw.check(restate(t, comps, 0, 600))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    raw.launch()
  t.set_step(7)
  assert bool((t.lookup_or_insert(dev(keys[200:])) >= 0).all().item())       # the table changes: same tensors
  t.table.copy_(dev(rng.randn(t.capacity, 4).astype(F32)))
  comps[1].copy_(dev(rng.randn(t.capacity, 16).astype(F32)))
  graph.replay()
  torch.cuda.synchronize()
  want = restate(t, comps, 0, 600)
  assert want[0] == 500
  raw.check(want)
