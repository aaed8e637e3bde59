"""Hash-keyed tables on the GPU (hbk_hash_insert_n, HashTable, HashGroupLookup): the device find-or-insert
against the placement rule's invariants, the existing probe (C oracle and device), the sequential host fill
where the two must agree, and a numpy dict model keyed by raw id for the lookups and optimizer steps behind it.

Slot numbers depend on which workgroup claims first; nothing below compares them with a host order except
where the order cannot matter (every key alone in its slab).  Row contents depend on the key alone, so they
are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
import oracle
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import GroupLookup, GroupLookupGrad, HashGroupLookup, HashTable, hash_translate
from tests.support import hash_ref as ref
from tests.support import reference as model
from tests.support.tolerance import assert_sums_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
EMPTY = ref.EMPTY
SPECIAL = np.array([EMPTY + 1, -1, 0, 2 ** 63 - 1], np.int64)


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def distinct_keys(rng, n, specials=True):
  """n distinct int64 keys over the full range (never EMPTY), the special ones first."""
  k = rng.randint(-2 ** 63 + 1, 2 ** 63 - 1, size=2 * n + 8, dtype=np.int64)
  pool = np.concatenate([SPECIAL, k]) if specials else k
  _, first = np.unique(pool, return_index=True)
  return pool[np.sort(first)][:n]


def with_duplicates(rng, keys, n):
  """n draws (n >= len(keys)) that name every key at least once."""
  extra = keys[rng.randint(0, keys.size, size=n - keys.size)]
  out = np.concatenate([keys, extra])
  rng.shuffle(out)
  return out


def raw_insert(cache, slab_size, keys, table=None, dim=0, pitch=0, scale=1e-3, seed=0, insert=1):
  """One column through the C entry: (slots, counts) device tensors; `cache` / `table` are written in place."""
  slots = torch.full((keys.numel(),), -7, dtype=torch.int64, device=DEV)
  counts = torch.zeros(2, dtype=torch.int32, device=DEV)
  col = _lib.HashColumn()
  col.keys_cache, col.slab_count, col.slab_size = cache.data_ptr(), cache.numel() // slab_size, slab_size
  col.keys, col.n_keys, col.slots, col.counts = keys.data_ptr(), keys.numel(), slots.data_ptr(), counts.data_ptr()
  col.table = table.data_ptr() if table is not None else None
  col.dim, col.table_pitch, col.init_scale, col.seed = dim, pitch, scale, seed
  arr = (_lib.HashColumn * 1)(col)
  _lib.check(_lib.lib().hbk_hash_insert_n(1, arr, insert, _lib.current_stream(torch.device(DEV))))
  return slots, counts


def empty_cache(slab_size, slab_count):
  return torch.full((slab_size * slab_count,), EMPTY, dtype=torch.int64, device=DEV)


def check_placement(cache_np, slab_size, keys, slots, d_cache=None):
  """What must hold of ANY correct concurrent insert: every slot holds its key, and the probe -- which stops
  at the first slab with an EMPTY slot -- finds every key exactly there."""
  placed = slots >= 0
  np.testing.assert_array_equal(cache_np[slots[placed]], keys[placed])
  np.testing.assert_array_equal(oracle.cache_probe(cache_np, slab_size, keys), slots)
  if d_cache is not None:
    hit, n_miss = hb.embedding.cache.probe(d_cache, dev(keys), slab_size)
    np.testing.assert_array_equal(host(hit), slots)
    assert int(n_miss.item()) == int((~placed).sum())
    found, counts = raw_insert(d_cache, slab_size, dev(keys), insert=0)      # the N-ary find
    np.testing.assert_array_equal(host(found), slots)
    assert host(counts).tolist() == [0, int((~placed).sum())]
    np.testing.assert_array_equal(host(d_cache), cache_np)                   # a find writes nothing


# ---- 1. invariants on random keys -----------------------------------------------------------------------
@pytest.mark.parametrize('slab_count', [1, 3, 257])
@pytest.mark.parametrize('slab_size', [5, 16, 64])
def test_invariants_empty_then_half_full(slab_size, slab_count):
  rng = np.random.RandomState(100 * slab_size + slab_count)
  cap = slab_size * slab_count
  pool = distinct_keys(rng, cap)
  d1 = max(cap // 2, 1)
  first = pool[:d1]
  second = np.concatenate([pool[d1:d1 + (cap - d1) // 2 + 1], first[:max(d1 // 3, 1)]])   # new keys and old ones
  cache = empty_cache(slab_size, slab_count)
  total = 0
  for batch_keys in (first, second):
    keys = with_duplicates(rng, batch_keys, min(20000, 3 * batch_keys.size + 5))
    before = host(cache)
    new = np.setdiff1d(batch_keys, before)
    slots, counts = raw_insert(cache, slab_size, dev(keys))
    slots, after = host(slots), host(cache)
    total += new.size
    # capacity >= the distinct keys so far: nothing can fail (a derived condition)
    assert total <= cap
    assert host(counts).tolist() == [new.size, 0]
    assert (slots >= 0).all() and (slots < cap).all()
    assert int((after != EMPTY).sum()) == total
    np.testing.assert_array_equal(after[before != EMPTY], before[before != EMPTY])   # slots only go EMPTY -> key
    check_placement(after, slab_size, keys, slots, cache)
    # one slot per distinct key
    assert np.unique(slots).size == np.unique(keys).size


# ---- 2. exact cases -------------------------------------------------------------------------------------
def test_keys_alone_in_their_slabs_equal_the_host_fill_bit_for_bit():
  rng = np.random.RandomState(21)
  slab_size, slab_count = 16, 257
  chosen, homes = [], set()
  for k in distinct_keys(rng, 2000).tolist():
    h = ref.home_slab(k, slab_count)
    if h not in homes and len(chosen) < 120:
      homes.add(h)
      chosen.append(k)
  keys = with_duplicates(rng, np.array(chosen, np.int64), 1000)
  want = np.full(slab_size * slab_count, EMPTY, np.int64)
  want_slots = ref.fill(want, slab_size, keys)
  assert (want_slots % slab_size == 0).all()                      # every key lands in slot 0 of its own slab
  cache = empty_cache(slab_size, slab_count)
  slots, counts = raw_insert(cache, slab_size, dev(keys))
  np.testing.assert_array_equal(host(cache), want)
  np.testing.assert_array_equal(host(slots), want_slots)
  assert host(counts).tolist() == [len(chosen), 0]


@pytest.mark.parametrize('slab_size,slab_count', [(5, 257), (16, 3), (64, 3)])
def test_no_overflow_gives_the_host_fills_slab_sets(slab_size, slab_count):
  rng = np.random.RandomState(22 + slab_size)
  # keys kept only while their home slab has room: by construction no slab overflows
  room = [slab_size] * slab_count
  chosen = []
  for k in distinct_keys(rng, 3 * slab_size * slab_count).tolist():
    h = ref.home_slab(k, slab_count)
    if room[h] > 0 and len(chosen) < (3 * slab_size * slab_count) // 4:
      room[h] -= 1
      chosen.append(k)
  keys = with_duplicates(rng, np.array(chosen, np.int64), 3 * len(chosen))
  want = np.full(slab_size * slab_count, EMPTY, np.int64)
  want_slots = ref.fill(want, slab_size, keys)
  assert (want_slots // slab_size == [ref.home_slab(k, slab_count) for k in keys.tolist()]).all()
  cache = empty_cache(slab_size, slab_count)
  slots, counts = raw_insert(cache, slab_size, dev(keys))
  got = host(cache)
  assert ref.slab_sets(got, slab_size) == ref.slab_sets(want, slab_size)
  # and inside a slab the occupied slots are its first ones (always the FIRST EMPTY slot is claimed)
  for s, w in zip(got.reshape(-1, slab_size), want.reshape(-1, slab_size)):
    np.testing.assert_array_equal(s != EMPTY, w != EMPTY)
  check_placement(got, slab_size, keys, host(slots))
  assert host(counts).tolist() == [len(chosen), 0]


# ---- 3. contention --------------------------------------------------------------------------------------
def test_one_key_4096_times():
  cache = empty_cache(16, 3)
  keys = np.full(4096, 1234567890123, np.int64)
  slots, counts = raw_insert(cache, 16, dev(keys))
  slots, after = host(slots), host(cache)
  assert int((after != EMPTY).sum()) == 1 and host(counts).tolist() == [1, 0]
  assert (slots == slots[0]).all() and after[slots[0]] == keys[0]
  assert slots[0] == ref.home_slab(int(keys[0]), 3) * 16        # the first EMPTY slot of its slab


def test_20000_keys_of_300_values():
  rng = np.random.RandomState(31)
  slab_size, slab_count = 16, 257
  values = distinct_keys(rng, 300)
  keys = with_duplicates(rng, values, 20000)
  cache = empty_cache(slab_size, slab_count)
  table = torch.zeros((slab_size * slab_count, 16), dtype=torch.float32, device=DEV)
  slots, counts = raw_insert(cache, slab_size, dev(keys), table=table, dim=16)
  slots, after = host(slots), host(cache)
  assert host(counts).tolist() == [300, 0] and int((after != EMPTY).sum()) == 300
  assert np.unique(slots).size == 300
  check_placement(after, slab_size, keys, slots, cache)
  # every row was written by exactly one winner, whole
  np.testing.assert_array_equal(host(table)[slots], ref.init_rows(keys, 16))


# ---- 4. idempotence -------------------------------------------------------------------------------------
def test_second_call_changes_nothing():
  rng = np.random.RandomState(41)
  t = HashTable(16 * 257, 20, DEV, slab_size=16, seed=5)
  keys = dev(with_duplicates(rng, distinct_keys(rng, 1500), 6000))
  s1 = host(t.lookup_or_insert(keys))
  cache1, rows1, n1 = host(t.keys), host(t.table), t.size()
  s2 = host(t.lookup_or_insert(keys))
  np.testing.assert_array_equal(s2, s1)
  np.testing.assert_array_equal(host(t.keys), cache1)
  np.testing.assert_array_equal(host(t.table), rows1)
  assert t.size() == n1 == 1500 and t.failed() == 0
  np.testing.assert_array_equal(host(t.find(keys)), s1)


# ---- 5. a table that fills up ---------------------------------------------------------------------------
@pytest.mark.parametrize('slab_size', [5, 16])
def test_full_table(slab_size):
  rng = np.random.RandomState(50 + slab_size)
  slab_count = 3
  cap = slab_size * slab_count
  values = distinct_keys(rng, cap + 7)
  keys = np.concatenate([with_duplicates(rng, values, 4 * values.size), [EMPTY, EMPTY]])
  rng.shuffle(keys)
  cache = empty_cache(slab_size, slab_count)
  slots, counts = raw_insert(cache, slab_size, dev(keys))
  slots, after = host(slots), host(cache)
  assert int((after != EMPTY).sum()) == cap                      # exactly capacity slots are occupied
  assert EMPTY not in after.tolist()
  assert (slots[keys == EMPTY] == -1).all()
  real = keys != EMPTY
  failed = np.unique(keys[real & (slots < 0)])
  assert failed.size == 7                                        # exactly 7 distinct keys found no room
  assert (slots[np.isin(keys, failed)] == -1).all()              # at every occurrence
  assert host(counts).tolist() == [cap, int((slots < 0).sum())]
  placed = slots >= 0
  np.testing.assert_array_equal(after[slots[placed]], keys[placed])
  assert sorted(after.tolist()) == sorted(np.setdiff1d(values, failed).tolist())
  # everything already present still translates, by insert and by find; nothing moves
  again, counts2 = raw_insert(cache, slab_size, dev(keys))
  np.testing.assert_array_equal(host(again), slots)
  assert host(counts2).tolist() == [0, int((slots < 0).sum())]
  np.testing.assert_array_equal(host(cache), after)
  hit, _ = hb.embedding.cache.probe(cache, dev(keys[real]), slab_size)
  np.testing.assert_array_equal(host(hit), slots[real])


# ---- 6. row initialisation ------------------------------------------------------------------------------
@pytest.mark.parametrize('dim,pitch', [(1, 0), (16, 0), (20, 0), (128, 0), (20, 24), (1, 3)])
@pytest.mark.parametrize('slab_size', [5, 64])
def test_row_init_depends_on_the_key_alone(dim, pitch, slab_size):
  rng = np.random.RandomState(60 + dim + pitch)
  slab_count, seed, scale = 3, 77, 0.25
  cap = slab_size * slab_count
  values = distinct_keys(rng, cap // 2)
  keys = with_duplicates(rng, values, 3 * values.size)
  cache = empty_cache(slab_size, slab_count)
  width = pitch or dim
  table = torch.full((cap, width), 9.0, dtype=torch.float32, device=DEV)
  slots, _ = raw_insert(cache, slab_size, dev(keys), table=table, dim=dim, pitch=pitch, scale=scale, seed=seed)
  slots, rows = host(slots), host(table)
  np.testing.assert_array_equal(rows[slots][:, :dim], ref.init_rows(keys, dim, seed, scale))
  assert (rows[:, dim:] == 9.0).all()                            # the floats between rows are not touched
  free = np.setdiff1d(np.arange(cap), slots)
  assert (rows[free] == 9.0).all()                               # nor the rows of slots nobody took
  # rows of keys already present are untouched: poison them, insert old and new keys
  table.fill_(-5.0)
  more = distinct_keys(rng, cap // 4 + 1, specials=False)
  more = more[~np.isin(more, values)]
  keys2 = with_duplicates(rng, np.concatenate([values, more]), 4 * values.size)
  slots2, counts2 = raw_insert(cache, slab_size, dev(keys2), table=table, dim=dim, pitch=pitch, scale=scale,
                               seed=seed)
  slots2, rows2 = host(slots2), host(table)
  assert host(counts2).tolist() == [more.size, 0]
  old = np.isin(keys2, values)
  assert (rows2[slots2[old]] == -5.0).all()
  np.testing.assert_array_equal(rows2[slots2[~old]][:, :dim], ref.init_rows(keys2[~old], dim, seed, scale))


def test_row_init_scale_zero_and_no_table():
  rng = np.random.RandomState(66)
  keys = with_duplicates(rng, distinct_keys(rng, 40), 100)
  cache = empty_cache(16, 5)
  table = torch.full((80, 8), 3.0, dtype=torch.float32, device=DEV)
  slots, counts = raw_insert(cache, 16, dev(keys), table=table, dim=8, scale=0.0)
  rows = host(table)
  got = rows[host(slots)]
  assert not got.any() and not np.signbit(got).any()             # +0.0
  assert int((rows == 3.0).all(axis=1).sum()) == 80 - 40
  # table == NULL: keys are placed, no row is written anywhere
  cache2 = empty_cache(16, 5)
  slots2, counts2 = raw_insert(cache2, 16, dev(keys), table=None, dim=0)
  assert host(counts2).tolist() == [40, 0] == host(counts).tolist()
  check_placement(host(cache2), 16, keys, host(slots2))
  # HashTable(init_scale=0) starts rows at zero; a seed changes nonzero starts
  a, b = HashTable(64, 4, DEV, seed=1), HashTable(64, 4, DEV, seed=2)
  ka = dev(keys[:10])
  ra, rb = host(a.table[a.lookup_or_insert(ka)]), host(b.table[b.lookup_or_insert(ka)])
  np.testing.assert_array_equal(ra, ref.init_rows(keys[:10], 4, 1, 1e-3))
  np.testing.assert_array_equal(rb, ref.init_rows(keys[:10], 4, 2, 1e-3))
  assert (ra != rb).any()


# ---- 7. end to end against a dict model keyed by raw id ---------------------------------------------------
class Model:
  """One column of the numpy model: every distinct raw id has a row (its initial row to start with); ids
  are renamed to their rank among the column's distinct ids, which the restatement then treats as rows."""

  def __init__(self, ids, dim, seed, scale):
    self.uniq, self.index = np.unique(ids, return_inverse=True)
    self.w = ref.init_rows(self.uniq, dim, seed, scale)


@pytest.fixture(scope='module')
def e2e():
  """Two columns: a ragged mean (dim 16) and one id per sample summed (dim 8); the batch, its model and the
  gradients are made once and shared."""
  rng = np.random.RandomState(70)
  B = 700
  lens = rng.poisson(3, size=B).clip(0, 9)
  sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  pool0, pool1 = distinct_keys(rng, 400), distinct_keys(rng, 250)
  ids0 = pool0[rng.zipf(1.3, size=int(sp[-1])) % pool0.size]
  ids1 = pool1[rng.randint(0, pool1.size, size=B)]
  return dict(B=B, ids=[ids0, ids1], sp=[sp, None], comb=['mean', 'sum'], dims=[16, 8], seeds=[3, 4],
              scale=0.05, grads=[rng.randn(B, 16).astype(F32), rng.randn(B, 8).astype(F32)],
              grads2=[rng.randn(B, 16).astype(F32), rng.randn(B, 8).astype(F32)])


def make_tables(e, capacity=(1024, 512), slab_size=(16, 5)):
  return [HashTable(capacity[c], e['dims'][c], DEV, slab_size=slab_size[c], init_scale=e['scale'],
                    seed=e['seeds'][c]) for c in range(2)]


def d_splits(e):
  return [None if s is None else dev(s) for s in e['sp']]


def rows_by_key(table, uniq):
  """The rows of `uniq` read through find."""
  slots = host(table.find(dev(uniq)))
  assert (slots >= 0).all()
  return host(table.table)[slots]


def test_forward_equals_the_model(e2e):
  e = e2e
  tables = make_tables(e)
  hgl = HashGroupLookup(tables, combiners=e['comb'])
  outs = hgl([dev(i) for i in e['ids']], d_splits(e))
  for c in range(2):
    m = Model(e['ids'][c], e['dims'][c], e['seeds'][c], e['scale'])
    assert tables[c].size() == m.uniq.size and tables[c].failed() == 0
    slots = host(hgl.slots[c])
    np.testing.assert_array_equal(host(tables[c].keys)[slots], e['ids'][c])
    # the combiner over the rows init_row(key): the fp32 oracle bit for bit, the float64 restatement within
    # the bound for fp32 sums
    want = oracle.group_lookup_fwd([m.w], [m.index.astype(np.int64)], [e['sp'][c]], [m.uniq.size], [e['comb'][c]])[0]
    np.testing.assert_array_equal(host(outs[c]), want)
    w64, mag = model.forward64(m.w, m.index, e['sp'][c], None, e['comb'][c])
    assert_sums_close(host(outs[c]), w64, mag, err_msg=f'forward column {c}')


def test_deterministic_sgd_then_adagrad_equal_the_sequential_sums(e2e):
  e = e2e
  tables = make_tables(e)
  hgl = HashGroupLookup(tables, combiners=e['comb'])
  hgl([dev(i) for i in e['ids']], d_splits(e))
  accums = [torch.full_like(t.table, 0.1) for t in tables]
  grad = GroupLookupGrad(hgl.lookup, accums=accums, deterministic=True)
  lr = 0.1
  grad(hgl.slots, [dev(g) for g in e['grads']], d_splits(e), apply_lr=lr, optimizer='sgd')
  models = [Model(e['ids'][c], e['dims'][c], e['seeds'][c], e['scale']) for c in range(2)]
  for c, m in enumerate(models):
    t, r, valid = model.terms32(m.uniq.size, m.index, e['sp'][c], None, e['comb'][c], e['grads'][c])
    u, sums = model.seq_row_sums(t, r, valid)
    model.sgd_step(m.w, u, sums, lr)
    np.testing.assert_array_equal(rows_by_key(tables[c], m.uniq), m.w)
  grad(hgl.slots, [dev(g) for g in e['grads2']], d_splits(e), apply_lr=lr, optimizer='adagrad')
  for c, m in enumerate(models):
    a = np.full_like(m.w, F32(0.1))
    t, r, valid = model.terms32(m.uniq.size, m.index, e['sp'][c], None, e['comb'][c], e['grads2'][c])
    u, sums = model.seq_row_sums(t, r, valid)
    model.adagrad_step(m.w, a, u, sums, lr)
    slots = host(tables[c].find(dev(m.uniq)))
    np.testing.assert_array_equal(host(tables[c].table)[slots], m.w)
    np.testing.assert_array_equal(host(accums[c])[slots], a)
    # rows no key owns were never stepped
    free = np.setdiff1d(np.arange(tables[c].capacity), slots)
    assert not host(tables[c].table)[free].any() and (host(accums[c])[free] == F32(0.1)).all()


def test_default_step_is_close_to_the_float64_model(e2e):
  e = e2e
  tables = make_tables(e)
  hgl = HashGroupLookup(tables, combiners=e['comb'])
  hgl([dev(i) for i in e['ids']], d_splits(e))
  lr = 0.1
  GroupLookupGrad(hgl.lookup)(hgl.slots, [dev(g) for g in e['grads']], d_splits(e), apply_lr=lr)
  for c in range(2):
    m = Model(e['ids'][c], e['dims'][c], e['seeds'][c], e['scale'])
    u, g64, gmag = model.backward64(m.w, m.index, e['sp'][c], None, e['comb'][c], e['grads'][c])
    want = m.w.astype(np.float64)
    mag = np.abs(want)
    want[u] -= lr * g64
    mag[u] += lr * gmag
    assert_sums_close(rows_by_key(tables[c], m.uniq), want, mag, err_msg=f'sgd step column {c}')


def test_ids_that_collide_under_a_bucket_get_rows_of_their_own():
  cap, dim = 512, 8
  t = HashTable(cap, dim, DEV, init_scale=0.5)
  a = 123456789
  ids = dev(np.array([a, a + cap, a + 7 * cap], np.int64))     # one row under floormod(id, 512)
  bucketed = GroupLookup([t.table], buckets=[cap], combiners='sum')
  hashed = HashGroupLookup([t], combiners='sum')
  out = host(hashed([ids])[0])
  slots = host(hashed.slots[0])
  assert np.unique(slots).size == 3
  np.testing.assert_array_equal(out, ref.init_rows(host(ids), dim, 0, 0.5))
  assert (out[0] != out[1]).any() and (out[1] != out[2]).any()
  shared = host(bucketed([ids])[0])
  np.testing.assert_array_equal(shared[0], shared[1])
  np.testing.assert_array_equal(shared[0], shared[2])


# ---- 8. inference ---------------------------------------------------------------------------------------
def test_inference_inserts_nothing(e2e):
  e = e2e
  tables = make_tables(e)
  HashGroupLookup(tables, combiners=e['comb'])([dev(i) for i in e['ids']], d_splits(e))
  rng = np.random.RandomState(80)
  ids = [i.copy() for i in e['ids']]
  unseen = []
  for c in range(2):
    new = distinct_keys(rng, 50, specials=False)
    new = new[~np.isin(new, e['ids'][c])]
    at = rng.choice(ids[c].size, size=new.size, replace=False)
    ids[c][at] = new
    unseen.append(at)
  before = [(host(t.keys), host(t.table), host(t.counts)) for t in tables]
  hgl = HashGroupLookup(tables, combiners=e['comb'], train=False)
  outs = hgl([dev(i) for i in ids], d_splits(e))
  plain = GroupLookup([t.table for t in tables], combiners=e['comb'])(hgl.slots, d_splits(e))
  for c in range(2):
    slots = host(hgl.slots[c])
    assert (slots[unseen[c]] == -1).all() and int((slots < 0).sum()) == unseen[c].size
    np.testing.assert_array_equal(host(outs[c]), host(plain[c]))
    for got, want in zip((host(tables[c].keys), host(tables[c].table), host(tables[c].counts)), before[c]):
      np.testing.assert_array_equal(got, want)
  # an unseen id reads as a zero row: the one-id column's outputs there are zeros
  assert not host(outs[1])[unseen[1]].any()
  # both columns were translated by one call of the N-ary find
  found = hash_translate(tables, [dev(i) for i in ids], insert=False)
  for c in range(2):
    np.testing.assert_array_equal(host(found[c]), host(hgl.slots[c]))


# ---- 9. items / load ------------------------------------------------------------------------------------
def test_items_load_into_another_geometry(e2e):
  e = e2e
  tables = make_tables(e)
  hgl = HashGroupLookup(tables, combiners=e['comb'])
  d_ids = [dev(i) for i in e['ids']]
  hgl(d_ids, d_splits(e))
  GroupLookupGrad(hgl.lookup, deterministic=True)(hgl.slots, [dev(g) for g in e['grads']], d_splits(e),
                                                   apply_lr=0.1)          # rows that are no longer their init
  outs = [host(o) for o in hgl(d_ids, d_splits(e))]
  bigger = make_tables(e, capacity=(2048, 1024), slab_size=(64, 16))
  for old, new in zip(tables, bigger):
    keys, rows = old.items()
    assert keys.numel() == old.size() and bool((keys[1:] > keys[:-1]).all())
    new.load(keys, rows)
    assert new.size() == old.size() and new.failed() == 0
    k2, r2 = new.items()
    np.testing.assert_array_equal(host(k2), host(keys))
    np.testing.assert_array_equal(host(r2), host(rows))
    np.testing.assert_array_equal(rows_by_key(new, host(keys)), rows_by_key(old, host(keys)))
  outs2 = HashGroupLookup(bigger, combiners=e['comb'], train=False)(d_ids, d_splits(e))
  for a, b in zip(outs, outs2):
    np.testing.assert_array_equal(host(b), a)
  # a table too small refuses the load instead of dropping keys
  small = HashTable(32, e['dims'][0], DEV, slab_size=16)
  with pytest.raises(_lib.InvalidArgumentError, match='do not fit'):
    small.load(*tables[0].items())


# ---- 10. captured graph ---------------------------------------------------------------------------------
def test_captured_launch_inserts_the_replays_keys():
  rng = np.random.RandomState(90)
  B, dims, scale = 300, [16, 8], 0.05
  lens = rng.poisson(2, size=B).clip(0, 6)
  sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  n = [int(sp[-1]), B]
  combs = ['mean', 'sum']
  tables = [HashTable(2048, d, DEV, init_scale=scale, seed=c) for c, d in enumerate(dims)]
  hgl = HashGroupLookup(tables, combiners=combs)

  def batch():
    return [distinct_keys(rng, 200, specials=False)[rng.randint(0, 200, size=k)] for k in n]
  first = batch()
  bufs = [dev(i) for i in first]
  splits = [dev(sp), None]
  outs = [torch.empty((B, d), dtype=torch.float32, device=DEV) for d in dims]
  hgl(bufs, splits, outs)                       # warm-up outside the capture: descriptors and slot buffers exist
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      hgl.launch()
  torch.cuda.synchronize()
  seen = [set(i.tolist()) for i in first]
  for _ in range(2):
    new = batch()
    for b, i in zip(bufs, new):
      b.copy_(dev(i))
    for o in outs:
      o.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    for c in range(2):
      seen[c] |= set(new[c].tolist())
      assert tables[c].size() == len(seen[c]) and tables[c].failed() == 0
      np.testing.assert_array_equal(host(tables[c].keys)[host(hgl.slots[c])], new[c])
      m = Model(new[c], dims[c], c, scale)
      want = oracle.group_lookup_fwd([m.w], [m.index.astype(np.int64)], [[sp, None][c]], [m.uniq.size],
                                     [combs[c]])[0]
      np.testing.assert_array_equal(host(outs[c]), want)
