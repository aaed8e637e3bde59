"""Growth and compaction of hash tables on the GPU (hbk_hash_rehash_n, HashTable.rehash / maybe_grow,
HashGroupLookup.rebind / maybe_grow): the rehashed table against the placement rule's invariants, the existing
probes (C oracle and device), the host path (items / load, compact) and a twin that never had to grow.

Slot numbers depend on which workgroup claims first; they are compared with a host order only where the order
cannot matter (no destination slab overflowing: the key SET of every slab)."""
import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
import oracle
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import GroupLookupGrad, HashGroupLookup, HashTable, hash_rehash
from tests.support import hash_ref as ref
from tests.support import hash_rehash_ref as rref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
EMPTY, TOMB = rref.EMPTY, rref.TOMBSTONE


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def distinct_keys(rng, n):
  """n distinct int64 keys over the full range, neither sentinel among them."""
  k = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=2 * n + 8, dtype=np.int64))
  rng.shuffle(k)
  return k[:n]


def homed_in(slab, slab_count, n, pool):
  """The first n keys of `pool` whose home slab is `slab` (vectorised)."""
  out = pool[ref.murmur3_np(pool).astype(np.int64) % slab_count == slab][:n]
  assert out.size == n
  return out


def check_live(t, keys, slots):
  """What must hold of ANY correct concurrent placement: every slot holds its key, no key is stored twice, and
  the probes -- which stop at the first slab with an EMPTY slot -- find every key there."""
  cache = host(t.keys)
  assert (slots >= 0).all() and (slots < t.capacity).all()
  np.testing.assert_array_equal(cache[slots], keys)
  live = cache[(cache != EMPTY) & (cache != TOMB)] if t.expiring else cache[cache != EMPTY]
  assert np.unique(live).size == live.size == keys.size
  np.testing.assert_array_equal(oracle.cache_probe(cache, t.slab_size, keys), slots)
  hit, n_miss = hb.embedding.cache.probe(t.keys, dev(keys), t.slab_size)
  np.testing.assert_array_equal(host(hit), slots)
  assert int(n_miss.item()) == 0
  assert int((cache == EMPTY).sum()) == t.capacity - keys.size


def identifying_rows(keys, dim, salt):
  """fp32 [n, dim] whose every row names its key (and the array: `salt`)."""
  low = (keys & 0xffff).astype(F32)
  return (low[:, None] * F32(8) + np.arange(dim, dtype=F32)[None, :] + F32(salt) / F32(4)).astype(F32)


def fill_table(t, rng, n, salt=0):
  """n keys into t, rows overwritten with values that identify their key.  Returns the keys, sorted."""
  keys = np.sort(distinct_keys(rng, n))
  slots = t.lookup_or_insert(dev(keys))
  assert bool((slots >= 0).all().item())
  t.table[slots] = dev(identifying_rows(keys, t.dim, salt))
  return keys


def companions_of(t, keys):
  """One companion of dim 3 with pitch 5 (a strided view) and one of dim 16, rows naming their keys."""
  slots = t.find(dev(keys))
  wide = torch.full((t.capacity, 5), -7.0, device=DEV)
  a = wide[:, :3]
  b = torch.full((t.capacity, 16), 0.25, device=DEV)
  a[slots] = dev(identifying_rows(keys, 3, 1))
  b[slots] = dev(identifying_rows(keys, 16, 2))
  return [(a, 0.5), (b, 0.25)]


def check_table(t, keys, comps, fills=(0.5, 0.25)):
  """Table t holds exactly `keys` (sorted), rows and companion rows following their keys bit for bit, the rows
  no key holds equal to the companion's fill value."""
  got_keys, got_rows = t.items()
  np.testing.assert_array_equal(host(got_keys), keys)
  assert host(got_rows).tobytes() == identifying_rows(keys, t.dim, 0).tobytes()
  slots = host(t.find(dev(keys)))
  check_live(t, keys, slots)
  free = np.setdiff1d(np.arange(t.capacity), slots)
  for n, (x, fill) in enumerate(zip(comps, fills)):
    assert tuple(x.shape) == (t.capacity, (3, 16)[n]) and x.is_contiguous()
    got = host(x)
    assert got[slots].tobytes() == identifying_rows(keys, x.shape[1], n + 1).tobytes()
    assert (got[free] == F32(fill)).all()


# ---- 1. invariants across geometries --------------------------------------------------------------------
GEOMETRIES = [((5, 3), (8, 7), 3), ((16, 257), (8, 1031), 3), ((64, 1), (64, 2), 3), ((8, 257), (8, 257), 3),
              ((8, 64), (5, 40), 1)]


@pytest.mark.parametrize('dim', [4, 19])
@pytest.mark.parametrize('src,dst,quarters', GEOMETRIES)
def test_invariants_across_geometries(src, dst, quarters, dim):
  rng = np.random.RandomState(1000 * src[0] + dst[1] + dim)
  cap = src[0] * src[1]
  n = max(quarters * cap // 4, 2)
  t = HashTable(cap, dim, DEV, slab_size=src[0])
  keys = fill_table(t, rng, n)
  comps = companions_of(t, keys)
  # a failure on record: it must be kept
  t.counts[1] = 3
  old_keys, old_table = t.keys, t.table
  old_cache = host(old_keys)
  before = [host(x) for x in t.items()]
  # the C entry once by hand, with new_slots, into arrays of its own
  d_keys = torch.full((dst[0] * dst[1],), EMPTY, dtype=torch.int64, device=DEV)
  d_wide = torch.full((dst[0] * dst[1], dim + 2), -3.0, device=DEV)     # rows at a pitch of dim + 2 words
  d_table = d_wide[:, :dim]
  new_slots = torch.full((cap,), -5, dtype=torch.int64, device=DEV)
  counts = torch.zeros(2, dtype=torch.int32, device=DEV)
  col = (_lib.HashRehashColumn * 1)()
  col[0].src_keys, col[0].src_slab_count, col[0].src_slab_size = old_keys.data_ptr(), src[1], src[0]
  col[0].dst_keys, col[0].dst_slab_count, col[0].dst_slab_size = d_keys.data_ptr(), dst[1], dst[0]
  col[0].expiring, col[0].n_moves = 0, 1
  col[0].moves[0].src, col[0].moves[0].dst, col[0].moves[0].words = old_table.data_ptr(), d_table.data_ptr(), dim
  col[0].moves[0].dst_pitch = dim + 2
  col[0].new_slots, col[0].counts = new_slots.data_ptr(), counts.data_ptr()
  _lib.check(_lib.lib().hbk_hash_rehash_n(1, col, _lib.current_stream(torch.device(DEV))))
  got_slots, got_cache = host(new_slots), host(d_keys)
  live = old_cache != EMPTY
  assert (got_slots[~live] == -1).all() and (got_slots[live] >= 0).all()
  np.testing.assert_array_equal(got_cache[got_slots[live]], old_cache[live])
  assert np.unique(got_slots[live]).size == n and host(counts).tolist() == [n, 0]
  assert host(d_table)[got_slots[live]].tobytes() == host(old_table)[live].tobytes()
  rest = np.setdiff1d(np.arange(dst[0] * dst[1]), got_slots[live])
  assert (host(d_wide)[:, dim:] == F32(-3)).all() and (host(d_wide)[rest] == F32(-3)).all()   # padding, free rows
  np.testing.assert_array_equal(host(old_keys), old_cache)                  # the source is only read
  # the method
  new = t.rehash(capacity=dst[0] * dst[1], slab_size=dst[0], slots=comps)
  assert (t.capacity, t.slab_count, t.slab_size) == (dst[0] * dst[1], dst[1], dst[0])
  assert t.keys is not old_keys and t.table is not old_table and tuple(t.table.shape) == (t.capacity, dim)
  assert (t.size(), t.failed()) == (n, 3)
  for a, b in zip(before, t.items()):
    assert a.tobytes() == host(b).tobytes()
  check_table(t, keys, new)


# ---- 2. contention and a full destination ---------------------------------------------------------------
def test_100_keys_homed_in_one_slab_and_a_destination_filled_to_the_last_slot():
  rng = np.random.RandomState(2)
  pool = distinct_keys(rng, 4000)
  keys = np.sort(homed_in(11, 16, 100, pool))
  t = HashTable(1024, 4, DEV, slab_size=64)
  assert bool((t.lookup_or_insert(dev(keys)) >= 0).all().item())
  t.table[t.find(dev(keys))] = dev(identifying_rows(keys, 4, 0))
  t.rehash(capacity=128, slab_size=8)
  slots = host(t.find(dev(keys)))
  check_live(t, keys, slots)
  assert host(t.table)[slots].tobytes() == identifying_rows(keys, 4, 0).tobytes()
  # 100 keys from slab 11 on, wrapping: 12 full slabs and 4 keys in the 13th
  used = np.unique(slots // 8)
  np.testing.assert_array_equal(used, np.sort((11 + np.arange(13)) % 16))
  per_slab = np.bincount(slots // 8, minlength=16)
  assert sorted(per_slab[used].tolist()) == [4] + [8] * 12
  assert (t.size(), t.failed()) == (100, 0)
  # live count == destination capacity: every slot is taken, nothing fails
  full = HashTable(16 * 40, 4, DEV, slab_size=16)
  keys = np.sort(distinct_keys(rng, 35 * 8))
  assert bool((full.lookup_or_insert(dev(keys)) >= 0).all().item())
  full.table[full.find(dev(keys))] = dev(identifying_rows(keys, 4, 0))
  full.rehash(capacity=35 * 8, slab_size=8)
  assert full.capacity == keys.size and int((full.keys == EMPTY).sum().item()) == 0
  slots = host(full.find(dev(keys)))
  check_live(full, keys, slots)
  assert (full.size(), full.failed()) == (keys.size, 0)
  assert host(full.table)[slots].tobytes() == identifying_rows(keys, 4, 0).tobytes()


# ---- 3. expiring tables ---------------------------------------------------------------------------------
def test_expiring_rehash_equals_compact_and_a_plain_table_keeps_the_tombstone_key():
  rng = np.random.RandomState(3)
  pool = distinct_keys(rng, 700)
  g1, g2, later = pool[:250], pool[250:500], pool[500:700]
  pair = []
  for _ in range(2):
    t = HashTable(16 * 40, 8, DEV, slab_size=16, expiring=True)
    accum = torch.full((t.capacity, 8), 0.1, device=DEV)
    t.set_step(1)
    t.lookup_or_insert(dev(g1))
    t.set_step(5)
    t.lookup_or_insert(dev(np.concatenate([g2, g2[:77], g2[:9]])))
    t.set_step(6)
    t.evict(3, slots=[(accum, 0.1)])
    where = t.find(dev(g2))
    t.table[where] = dev(identifying_rows(g2, 8, 0))
    accum[where] = dev(identifying_rows(g2, 8, 1))
    assert (t.tombstones(), t.size()) == (250, 250)
    pair.append((t, accum))
  (t, accum), (twin, twin_accum) = pair
  step = host(t.step).copy()
  accum, = t.rehash(slots=[(accum, 0.1)])
  twin.compact(slots=[(twin_accum, 0.1)])
  assert (t.tombstones(), t.evicted(), t.reused(), t.size(), t.failed()) == (0, 0, 0, 250, 0)
  np.testing.assert_array_equal(host(t.step), step)
  for a, b in zip(t.items(), twin.items()):
    assert host(a).tobytes() == host(b).tobytes()
  keys = np.sort(g2)
  s, s_twin = host(t.find(dev(keys))), host(twin.find(dev(keys)))
  check_live(t, keys, s)
  for mine, theirs in ((t.last_seen, twin.last_seen), (t.freq, twin.freq), (accum, twin_accum)):
    assert host(mine)[s].tobytes() == host(theirs)[s_twin].tobytes()
  free = np.setdiff1d(np.arange(t.capacity), s)
  assert not host(t.last_seen)[free].any() and not host(t.freq)[free].any() and (host(accum)[free] == F32(0.1)).all()
  # new keys find EMPTY slots and reuse nothing
  t.set_step(7)
  assert bool((t.lookup_or_insert(dev(later)) >= 0).all().item())
  assert (t.reused(), t.size(), t.tombstones()) == (0, 450, 0)
  assert int((t.keys == EMPTY).sum().item()) == t.capacity - 450
  # a plain table: INT64_MIN + 1 is an ordinary key
  plain = HashTable(64, 4, DEV, slab_size=8)
  keys = np.sort(np.concatenate([g1[:20], [TOMB]]))
  plain.lookup_or_insert(dev(keys))
  plain.rehash(capacity=128)
  np.testing.assert_array_equal(host(plain.items()[0]), keys)
  assert plain.size() == 21 and int(plain.find(dev(np.array([TOMB])))[0].item()) >= 0


# ---- 4. the same result as the host path ----------------------------------------------------------------
def test_slab_sets_equal_those_of_load_items_when_no_slab_overflows():
  rng = np.random.RandomState(4)
  t = HashTable(16 * 64, 4, DEV, slab_size=16)
  keys = fill_table(t, rng, 256)
  other = HashTable(8 * 257, 4, DEV, slab_size=8)
  other.load(*t.items())
  t.rehash(capacity=8 * 257, slab_size=8)
  sets = ref.slab_sets(host(other.keys), 8)
  assert max(len(s) for s in sets) < 8                                      # no slab overflows
  assert ref.slab_sets(host(t.keys), 8) == sets
  want, _, n_moved, n_failed = rref.rehash(np.sort(keys), 8, 257, False)
  assert ref.slab_sets(want, 8) == sets and (n_moved, n_failed) == (256, 0)
  for a, b in zip(t.items(), other.items()):
    assert host(a).tobytes() == host(b).tobytes()


# ---- 5. training across growth --------------------------------------------------------------------------
def test_training_across_growth_equals_tables_that_never_grew():
  rng = np.random.RandomState(5)
  dim, lr, acc0, n_ids, steps, fresh = 8, 0.1, 0.1, 64, 8, 20
  splits = [None, dev(np.arange(0, n_ids + 1, 2, dtype=np.int32))]
  pools = [distinct_keys(rng, steps * fresh) for _ in range(2)]
  batches = []
  for s in range(steps):
    ids = []
    for p in pools:
      new, seen = p[s * fresh:(s + 1) * fresh], p[:(s + 1) * fresh]
      one = np.concatenate([new, seen[rng.randint(0, seen.size, size=n_ids - fresh)]])
      rng.shuffle(one)
      ids.append(one)
    batches.append((ids, [rng.randn(n_ids, dim).astype(F32), rng.randn(n_ids // 2, dim).astype(F32)]))

  def run(capacities, grow):
    tables = [HashTable(capacities[c], dim, DEV, slab_size=(8, 5)[c], init_scale=0.05, seed=3 + c) for c in range(2)]
    accums = [torch.full_like(t.table, acc0) for t in tables]
    hgl = HashGroupLookup(tables, combiners=['sum', 'mean'], max_norms=[0.1, None])
    grad = GroupLookupGrad(hgl.lookup, accums=accums, deterministic=True)
    outs, grown = [], 0
    for ids, grads in batches:
      out = hgl([dev(i) for i in ids], splits)
      assert all(bool((s >= 0).all().item()) for s in hgl.slots)          # no id ever translates to -1
      outs.append([host(o) for o in out])
      grad(hgl.slots, [dev(g) for g in grads], splits, apply_lr=lr, optimizer='adagrad')
      if grow:
        old_lookup = hgl.lookup
        res = hgl.maybe_grow(0.75, 2.0, slots=[[(a, acc0)] for a in accums])
        if any(r is not None for r in res):
          grown += 1
          assert hgl.lookup is not old_lookup and hgl.slots is None
          with pytest.raises(_lib.HbkError, match='launch'):
            hgl.launch()                                                   # right after rebind(): nothing is bound
          accums = [a if r is None else r[0] for a, r in zip(accums, res)]
          grad = GroupLookupGrad(hgl.lookup, accums=accums, deterministic=True)
    return tables, accums, outs, grown

  tables, accums, outs, grown = run([64, 60], True)
  assert grown >= 2 and all(t.capacity > 64 for t in tables) and all(t.failed() == 0 for t in tables)
  twins, twin_accums, twin_outs, _ = run([t.capacity for t in tables], False)
  for s in range(steps):
    for c in range(2):
      assert outs[s][c].tobytes() == twin_outs[s][c].tobytes(), (s, c)
  for c in range(2):
    keys = np.sort(pools[c])
    for a, b in zip(tables[c].items(), twins[c].items()):
      assert host(a).tobytes() == host(b).tobytes()
    np.testing.assert_array_equal(host(tables[c].items()[0]), keys)
    s, s_twin = host(tables[c].find(dev(keys))), host(twins[c].find(dev(keys)))
    assert host(accums[c])[s].tobytes() == host(twin_accums[c])[s_twin].tobytes()
    assert tables[c].size() == keys.size


def test_a_call_on_a_rehashed_table_without_rebind_is_refused():
  t = HashTable(64, 4, DEV)
  hgl = HashGroupLookup([t])
  ids = dev(np.arange(1, 9, dtype=np.int64))
  hgl([ids], [None])
  t.rehash(capacity=128)
  with pytest.raises(_lib.InvalidArgumentError, match='rebind'):
    hgl([ids], [None])
  with pytest.raises(_lib.InvalidArgumentError, match='rebind'):
    hgl.launch()
  hgl.rebind()
  out = hgl([ids], [None])
  np.testing.assert_array_equal(host(out[0]), ref.init_rows(host(ids), 4, 0, 1e-3))
  assert t.size() == 8


# ---- 6. filtered tables ---------------------------------------------------------------------------------
def test_a_filtered_tables_sketch_and_admissions_are_untouched():
  rng = np.random.RandomState(6)
  pool = distinct_keys(rng, 300)
  first = np.concatenate([pool[:200], pool[:100]])                          # 100 ids twice, 100 once
  pair = [HashTable(512, 4, DEV, slab_size=8, min_freq=2, sketch_width=1 << 12, sketch_seed=9) for _ in range(2)]
  for t in pair:
    got = host(t.lookup_or_insert(dev(first)))
    assert ((got >= 0) == np.isin(first, pool[:100])).all()
  t, twin = pair
  sketch, filtered, width = host(t.sketch).copy(), t.filtered(), t.sketch
  t.rehash(capacity=1024, slab_size=16)
  assert t.sketch is width and host(t.sketch).tobytes() == sketch.tobytes() and t.filtered() == filtered
  assert (t.min_freq, t.sketch_seed, t.size()) == (2, 9, 100)
  nxt = np.concatenate([pool[100:250], pool[:50]])                          # second sightings, first sightings, residents
  got, want = host(t.lookup_or_insert(dev(nxt))), host(twin.lookup_or_insert(dev(nxt)))
  np.testing.assert_array_equal(got >= 0, want >= 0)
  assert (got[:100] >= 0).all() and (got[100:150] == -1).all() and (got[150:] >= 0).all()
  assert host(t.sketch).tobytes() == host(twin.sketch).tobytes() and t.filtered() == twin.filtered()
  assert t.size() == twin.size() == 200


# ---- 7. many tables, one call ---------------------------------------------------------------------------
def test_70_tables_of_mixed_kinds_and_geometries_in_one_call():
  rng = np.random.RandomState(7)
  tables, keys, comps, caps, sizes = [], [], [], [], []
  for c in range(70):
    slab_size = (5, 8, 16)[c % 3]
    slab_count = 3 + c % 5
    kind = c % 4                                                            # plain, expiring, filtered, both
    t = HashTable(slab_size * slab_count, 4, DEV, slab_size=slab_size, expiring=kind in (1, 3),
                  min_freq=1 if kind >= 2 else 0, sketch_width=1 << 10)
    if t.expiring:
      t.set_step(c)
    k = fill_table(t, rng, t.capacity // 2)
    tables.append(t)
    keys.append(k)
    comps.append(companions_of(t, k))
    new_size = (8, 5, 16, None)[c % 4]
    sizes.append(new_size)
    caps.append(None if c % 7 == 0 else (new_size or slab_size) * (2 * slab_count + c % 3))
  geometry = [(t.capacity, t.slab_size) for t in tables]
  new = hash_rehash(tables, caps, sizes, comps)
  assert len(new) == 70
  for c, t in enumerate(tables):
    want_size = sizes[c] or geometry[c][1]
    want_cap = geometry[c][0] if caps[c] is None else caps[c]
    assert (t.slab_size, t.capacity) == (want_size, want_cap // want_size * want_size), c
    check_table(t, keys[c], new[c])
    assert (t.size(), t.failed()) == (keys[c].size, 0)
    if t.expiring:
      s = host(t.find(dev(keys[c])))
      assert (host(t.last_seen)[s] == c).all() and (host(t.freq)[s] == 1).all()
      assert int(t.last_seen.sum().item()) == c * keys[c].size and int(t.freq.sum().item()) == keys[c].size


# ---- 8. a refused shrink --------------------------------------------------------------------------------
def test_a_shrink_below_size_is_refused_and_changes_nothing():
  rng = np.random.RandomState(8)
  t = HashTable(256, 4, DEV, slab_size=8, expiring=True)
  t.set_step(2)
  keys = fill_table(t, rng, 100)
  state = (t.keys, t.table, t.last_seen, t.freq, t.counts, t.stats)
  contents = [host(x).copy() for x in state]
  with pytest.raises(_lib.InvalidArgumentError, match='do not fit'):
    t.rehash(capacity=96)
  now = (t.keys, t.table, t.last_seen, t.freq, t.counts, t.stats)
  assert all(a is b for a, b in zip(state, now)) and (t.capacity, t.slab_count, t.slab_size) == (256, 32, 8)
  for x, was in zip(now, contents):
    assert host(x).tobytes() == was.tobytes()
  t.rehash(capacity=104)                                                    # 100 keys into 104 slots: fits
  assert t.capacity == 104 and t.size() == 100
  check_live(t, keys, host(t.find(dev(keys))))
