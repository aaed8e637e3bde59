"""The admission filter on the GPU (hbk_hash_insert_admit_n, hbk_hash_insert_expiring_admit_n,
HashTable(min_freq=F)): which ids a call admits, the sketch and the counters against the sequential restatement
(tests/support/hash_admission_ref.py), bit for bit; the admitted keys against the placement rule's invariants
and the existing probes; the filter across calls, under collisions, beside a full table, with expiry, in mixed
plans, through training steps, and through load / compact / a checkpoint.

Slot numbers depend on which workgroup claims first: they are compared with the restatement's nowhere, only
with themselves (every slot holds its key; the same id, the same slot)."""
import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
import oracle
from hybridbackend_amd.embedding import GroupLookupGrad, HashGroupLookup, HashTable, hash_translate
from hybridbackend_amd.training.saver import Saver
from tests.support import hash_admission_ref as aref
from tests.support import hash_ref as ref
from tests.support import reference as model
from tests.support.tolerance import assert_sums_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
EMPTY, TOMB = aref.EMPTY, aref.TOMBSTONE


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def distinct_keys(rng, n):
  """n distinct int64 keys over the full range, neither sentinel among them."""
  k = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=2 * n + 8, dtype=np.int64))
  rng.shuffle(k)
  return k[:n]


def call(t, keys, step=None):
  if step is not None:
    t.set_step(step)
  return host(t.lookup_or_insert(dev(keys)))


def check_live(t, keys, slots):
  """What must hold of any correct concurrent insert: every slot holds its key, no key is stored twice, and the
  probes find every key where the insert put it."""
  cache = host(t.keys)
  assert (slots >= 0).all() and (slots < t.capacity).all()
  np.testing.assert_array_equal(cache[slots], keys)
  live = cache[(cache != EMPTY) & (cache != TOMB)] if t.expiring else cache[cache != EMPTY]
  assert np.unique(live).size == live.size
  assert np.unique(slots).size == np.unique(keys).size
  np.testing.assert_array_equal(oracle.cache_probe(cache, t.slab_size, keys), slots)
  hit, n_miss = hb.embedding.cache.probe(t.keys, dev(keys), t.slab_size)
  np.testing.assert_array_equal(host(hit), slots)
  assert int(n_miss.item()) == 0
  np.testing.assert_array_equal(host(t.find(dev(keys))), slots)
  np.testing.assert_array_equal(host(t.keys), cache)                       # a find writes nothing


class Twin:
  """The restatement's arrays of one table, stepped beside it."""

  def __init__(self, t):
    self.t = t
    self.cache = np.full(t.capacity, EMPTY, np.int64)
    self.sketch = np.zeros(tuple(t.sketch.shape), np.int32)
    self.seen, self.freq = np.zeros(t.capacity, np.int32), np.zeros(t.capacity, np.int32)
    self.n = {'inserted': 0, 'failed': 0, 'reused': 0, 'filtered': 0}

  def call(self, keys, step=0):
    admitted, slots, n = aref.translate(self.cache, self.t.slab_size, keys, self.sketch, self.t.min_freq,
                                        self.t.expiring, self.t.sketch_seed, self.seen, self.freq, step)
    for k, v in n.items():
      self.n[k] += v
    return admitted, slots

  def check(self):
    """The sketch bit for bit, the counters, the stored key SET."""
    t = self.t
    np.testing.assert_array_equal(host(t.sketch), self.sketch)
    assert (t.filtered(), int(t.counts[0].item()), t.failed()) == \
        (self.n['filtered'], self.n['inserted'], self.n['failed'])
    live = lambda c: np.sort(c[(c != EMPTY) & (c != TOMB)] if t.expiring else c[c != EMPTY])   # noqa: E731
    np.testing.assert_array_equal(live(host(t.keys)), live(self.cache))


def same_answer_per_id(keys, slots):
  order = np.argsort(keys, kind='stable')
  k, s = keys[order], slots[order]
  same = k[1:] == k[:-1]
  assert (s[1:][same] == s[:-1][same]).all()


# ---- 1. exact against the restatement, within one call -------------------------------------------------------
@pytest.mark.parametrize('slab_count', [1, 3, 257])
@pytest.mark.parametrize('slab_size', [5, 16, 64])
def test_one_call_equals_the_restatement(slab_size, slab_count):
  rng = np.random.RandomState(100 * slab_size + slab_count)
  cap, dim = slab_size * slab_count, 4
  pool = distinct_keys(rng, max(cap // 2, 1))
  keys = np.repeat(pool, 1 + np.arange(pool.size) % 5)
  rng.shuffle(keys)
  t = HashTable(cap, dim, DEV, slab_size=slab_size, init_scale=0.5, seed=3, min_freq=3)
  assert tuple(t.sketch.shape) == (4, cap)
  twin = Twin(t)
  slots = call(t, keys)
  admitted, _ = twin.call(keys)
  np.testing.assert_array_equal(slots >= 0, admitted)                      # the admitted id set, per occurrence
  assert (slots[~admitted] == -1).all()
  same_answer_per_id(keys, slots)
  twin.check()
  assert t.failed() == 0 and t.size() == np.unique(keys[admitted]).size and t.filtered() == int((~admitted).sum())
  # every id seen 3 times or more is in (early, never late); the rest only by collision, as the restatement has it
  times = dict(zip(*np.unique(keys, return_counts=True)))
  assert all(admitted[n] for n, k in enumerate(keys.tolist()) if times[k] >= 3)
  table = host(t.table)
  if admitted.any():
    check_live(t, keys[admitted], slots[admitted])
    np.testing.assert_array_equal(table[slots[admitted]], ref.init_rows(keys[admitted], dim, 3, 0.5))
  free = np.setdiff1d(np.arange(cap), slots[admitted])
  assert not table[free].any() and (host(t.keys)[free] == EMPTY).all()


# ---- 2. across calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('expiring', [False, True])
def test_the_third_sighting_admits_and_residents_count_nothing(expiring):
  rng = np.random.RandomState(21)
  n = 1500
  keys = distinct_keys(rng, n)
  # (a sketch with room: no two of the ids share all four cells, so nothing is admitted early here)
  t = HashTable(4096, 4, DEV, slab_size=8, min_freq=3, sketch_width=1 << 16, expiring=expiring)
  twin = Twin(t)
  for k in (1, 2):
    assert (call(t, keys, k if expiring else None) == -1).all()
    twin.call(keys, k)
    assert (host(t.keys) == EMPTY).all() and t.size() == 0 and t.filtered() == k * n
    assert not host(t.table).any()
    twin.check()
  assert (host(t.estimate(dev(keys))) == 2).all()
  slots = call(t, keys, 3 if expiring else None)
  admitted, _ = twin.call(keys, 3)
  assert admitted.all()
  check_live(t, keys, slots)
  twin.check()
  assert t.size() == n and t.filtered() == 2 * n
  sketch = host(t.sketch)
  np.testing.assert_array_equal(call(t, keys, 4 if expiring else None), slots)
  twin.call(keys, 4)
  twin.check()
  np.testing.assert_array_equal(host(t.sketch), sketch)                    # residents count nothing
  assert t.filtered() == 2 * n and t.size() == n
  # find and train=False never change the sketch, for resident and unseen ids alike
  unseen = distinct_keys(np.random.RandomState(22), 300)
  both = np.concatenate([unseen, keys[:300]])
  got = host(t.find(dev(both)))
  assert (got[:300] == -1).all() and (got[300:] == slots[:300]).all()
  HashGroupLookup([t], combiners='sum', train=False)([dev(both)], [None])
  hash_translate([t], [dev(both)], insert=False)
  np.testing.assert_array_equal(host(t.sketch), sketch)
  assert t.filtered() == 2 * n and t.size() == n
  if expiring:
    assert (host(t.freq)[slots] == 2).all() and (host(t.last_seen)[slots] == 4).all()


# ---- 3. collisions ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth,width', [(1, 1), (2, 2)])
def test_collisions_admit_early_never_late(depth, width):
  rng = np.random.RandomState(30 + width)
  F = 4
  t = HashTable(1024, 4, DEV, slab_size=8, min_freq=F, sketch_depth=depth, sketch_width=width, sketch_seed=9)
  twin = Twin(t)
  pool = distinct_keys(rng, 200)
  seen = {}
  for n_call in range(3):
    keys = pool[n_call * 40:n_call * 40 + 80][rng.randint(0, 80, size=150)] if n_call else pool[:F]
    resident = host(t.find(dev(keys))) >= 0
    slots = call(t, keys)
    admitted, _ = twin.call(keys)
    np.testing.assert_array_equal(slots[~resident] >= 0, admitted[~resident])
    assert (slots[resident] >= 0).all()
    twin.check()
    same_answer_per_id(keys, slots)
    for k in keys[~resident].tolist():
      seen[k] = seen.get(k, 0) + 1
    assert all(slots[n] >= 0 for n, k in enumerate(keys.tolist()) if seen.get(k, 0) >= F)    # never late
    if n_call == 0 and width == 1:
      assert (slots >= 0).all() and t.size() == F                          # F distinct new ids, one cell: all in
  if width == 1:
    assert int(t.sketch.item()) == sum(seen.values())


# ---- 4. partial waves and many columns ----------------------------------------------------------------------
@pytest.mark.parametrize('slab_size', [5, 64])
@pytest.mark.parametrize('n_keys', [1, 7, 'block + 1'])
def test_partial_waves(slab_size, n_keys):
  group = 8 if slab_size == 5 else 64
  n = (256 // group) * 8 + 1 if n_keys == 'block + 1' else n_keys
  rng = np.random.RandomState(40 + n)
  keys = distinct_keys(rng, n)
  t = HashTable(slab_size * 120, 4, DEV, slab_size=slab_size, min_freq=2, sketch_width=1 << 14)
  twin = Twin(t)
  out = torch.full((n + 3,), 77, dtype=torch.int64, device=DEV)            # nothing is written past n_keys
  hash_translate([t], [dev(keys)], outs=[out[:n]])
  twin.call(keys)
  assert (host(out[:n]) == -1).all() and (host(out[n:]) == 77).all()
  twin.check()
  slots = host(hash_translate([t], [dev(keys)], outs=[out[:n]])[0])
  admitted, _ = twin.call(keys)
  assert admitted.all() and (host(out[n:]) == 77).all()
  check_live(t, keys, slots)
  twin.check()


@pytest.mark.parametrize('expiring', [False, True])
def test_65_columns_and_two_columns_naming_one_table(expiring):
  rng = np.random.RandomState(45)
  tables = [HashTable(16, 4, DEV, slab_size=8, min_freq=2, sketch_width=1024, expiring=expiring) for c in range(65)]
  tables[64] = tables[0]                                                   # the second launch's only column
  pool = distinct_keys(rng, 65 * 3).reshape(65, 3)
  ids = [np.array([p[0], p[1], p[0]], np.int64) for p in pool]
  shared = distinct_keys(rng, 3)
  ids[0] = np.array([shared[0], shared[1]], np.int64)
  ids[64] = np.array([shared[0], shared[2]], np.int64)
  slots = [host(s) for s in hash_translate(tables, [dev(i) for i in ids])]
  for c in range(1, 64):
    assert slots[c][0] == slots[c][2] >= 0 and slots[c][1] == -1
    assert (tables[c].size(), tables[c].filtered(), tables[c].failed()) == (1, 1, 0)
    assert host(tables[c].keys)[slots[c][0]] == pool[c][0]
  # both columns' counts were in the sketch before either launch admitted: the shared id is in, in one slot
  assert slots[0][0] == slots[64][0] >= 0 and slots[0][1] == -1 and slots[64][1] == -1
  assert (tables[0].size(), tables[0].filtered()) == (1, 2)
  assert host(tables[0].estimate(dev(shared))).tolist() == [2, 1, 1]


# ---- 5. a full table ----------------------------------------------------------------------------------------
def test_admitted_ids_that_find_the_table_full_count_as_failed():
  F = 3
  t = HashTable(5, 4, DEV, slab_size=5, min_freq=F)
  keys = np.repeat(np.arange(101, 109, dtype=np.int64), F)
  np.random.RandomState(50).shuffle(keys)
  slots = call(t, keys)
  same_answer_per_id(keys, slots)
  stored = np.unique(keys[slots >= 0])
  assert stored.size == 5 and sorted(np.unique(slots[slots >= 0]).tolist()) == [0, 1, 2, 3, 4]
  assert (t.size(), t.failed(), t.filtered()) == (5, 3 * F, 0)
  np.testing.assert_array_equal(np.sort(host(t.keys)), stored)


# ---- 6. expiring + filter -----------------------------------------------------------------------------------
def test_expiring_filtered_table():
  rng = np.random.RandomState(60)
  F = 3
  t = HashTable(16 * 24, 4, DEV, slab_size=16, expiring=True, min_freq=F, sketch_width=1 << 15)
  twin = Twin(t)
  old, young, new = np.split(distinct_keys(rng, 300), [120, 200])
  keys = np.concatenate([old, old, [EMPTY, TOMB]])
  assert (call(t, keys, 1) == -1).all()
  twin.call(keys, 1)
  twin.check()
  # filtered occurrences wrote no metadata; the sentinels count in failed and nowhere in the sketch
  assert not host(t.last_seen).any() and not host(t.freq).any() and t.failed() == 2 and t.filtered() == 2 * old.size
  assert int(t.sketch.sum().item()) == 4 * 2 * old.size
  # the admitting call: freq = that call's occurrences, last_seen = its step
  keys = np.concatenate([old, old[:50], old[:10]])
  rng.shuffle(keys)
  slots = call(t, keys, 2)
  twin.call(keys, 2)
  twin.check()
  check_live(t, keys, slots)
  where = host(t.find(dev(old)))
  np.testing.assert_array_equal(host(t.freq)[where], np.r_[np.full(10, 3), np.full(40, 2), np.full(70, 1)])
  assert (host(t.last_seen)[where] == 2).all() and int(t.freq.sum().item()) == keys.size
  # (per key the restatement's too; slot numbers are the device's own)
  twin_where = np.array([aref.xref.find(twin.cache, 16, int(k)) for k in old])
  np.testing.assert_array_equal(host(t.freq)[where], twin.freq[twin_where])
  # young ids come in at step 6 (three sightings in one call), old ones are evicted at step 7
  keys = np.tile(young, 3)
  call(t, keys, 6)
  twin.call(keys, 6)
  t.set_step(7)
  t.evict(steps_to_live=3)
  twin.cache[twin_where] = TOMB
  twin.seen[twin_where] = 0
  twin.freq[twin_where] = 0
  assert (t.evicted(), t.tombstones(), t.size()) == (old.size, old.size, young.size)
  twin.check()
  # admitted new ids reuse tombstones; an evicted id comes back in ONE call while the sketch stands
  keys = np.concatenate([np.tile(new, 3), old[:30], young])
  rng.shuffle(keys)
  slots = call(t, keys, 8)
  twin.call(keys, 8)
  assert (slots >= 0).all()
  check_live(t, keys, slots)
  twin.check()
  assert 0 < t.reused() <= old.size and t.size() == young.size + new.size + 30
  # after clear_filter an evicted id needs F sightings again
  t.set_step(20)
  t.evict(steps_to_live=3)
  assert t.size() == 0
  t.clear_filter()
  assert not host(t.sketch).any()
  back = old[:40]
  for k in range(F - 1):
    assert (call(t, back, 21 + k) == -1).all()
  assert (call(t, back, 23) >= 0).all() and t.size() == 40
  # age_filter halves the sketch exactly
  call(t, np.tile(new[:20], 5), 24)                                        # not resident any more: counted
  before = host(t.sketch)
  assert before.max() >= 5
  t.age_filter()
  np.testing.assert_array_equal(host(t.sketch), before >> 1)


# ---- 7. mixed plans -----------------------------------------------------------------------------------------
def test_mixed_plan_leaves_the_unfiltered_tables_results_as_they_were():
  rng = np.random.RandomState(70)
  cap, dim, ss = 16 * 64, 8, 16

  def make():
    return [HashTable(cap, dim, DEV, slab_size=ss, init_scale=0.5, seed=5),
            HashTable(cap, dim, DEV, slab_size=ss, init_scale=0.5, seed=5, min_freq=2, sketch_width=1 << 16),
            HashTable(cap, dim, DEV, slab_size=ss, init_scale=0.5, seed=5, expiring=True),
            HashTable(cap, dim, DEV, slab_size=ss, init_scale=0.5, seed=5, expiring=True, min_freq=2,
                      sketch_width=1 << 16)]
  pool = distinct_keys(rng, cap // 8)
  want_cache = np.full(cap, EMPTY, np.int64)
  ref.fill(want_cache, ss, pool)
  assert max(len(s) for s in ref.slab_sets(want_cache, ss)) < ss            # no slab overflows: slab sets are fixed
  once, twice = pool[:60], pool[60:]
  draws = np.concatenate([once, twice, twice])
  rng.shuffle(draws)
  d = dev(draws)
  mixed, alone = make(), make()
  for t in mixed + alone:
    if t.expiring:
      t.set_step(2)
  got = [host(s) for s in hash_translate(mixed, [d] * 4)]
  base = [host(s) for s in hash_translate([alone[0], alone[2]], [d] * 2)]
  for m, a, g, b in ((mixed[0], alone[0], got[0], base[0]), (mixed[2], alone[2], got[2], base[1])):
    assert ref.slab_sets(host(m.keys), ss) == ref.slab_sets(host(a.keys), ss) == ref.slab_sets(want_cache, ss)
    assert host(m.counts).tolist() == host(a.counts).tolist() == [pool.size, 0]
    np.testing.assert_array_equal(host(m.keys)[g], draws)
    np.testing.assert_array_equal(host(m.table)[g], host(a.table)[b])
  for t, g in ((mixed[1], got[1]), (mixed[3], got[3])):
    assert ((g >= 0) == np.isin(draws, twice)).all()
    assert (t.size(), t.filtered(), t.failed()) == (twice.size, once.size, 0)
    check_live(t, draws[g >= 0], g[g >= 0])
  assert (host(mixed[3].freq)[got[3][got[3] >= 0]] == 2).all()
  # one HashGroupLookup over the four, and its launch() again
  hgl = HashGroupLookup(mixed, combiners='sum')
  outs = hgl([d] * 4, [None] * 4)
  rows = ref.init_rows(draws, dim, 5, 0.5)
  for c in range(4):
    slots = host(hgl.slots[c])
    assert (slots >= 0).all()                                              # the second sighting of `once`
    np.testing.assert_array_equal(slots[got[c] >= 0], got[c][got[c] >= 0])
    np.testing.assert_array_equal(host(outs[c]), rows)
  before = [host(s) for s in hgl.slots]
  hgl.launch()
  torch.cuda.synchronize()
  for c in range(4):
    np.testing.assert_array_equal(host(hgl.slots[c]), before[c])
  # a mixed find
  found = hash_translate(mixed, [d] * 4, insert=False)
  for c in range(4):
    np.testing.assert_array_equal(host(found[c]), before[c])


# ---- 8. training through it ---------------------------------------------------------------------------------
@pytest.mark.parametrize('optimizer', ['sgd', 'adagrad'])
def test_training_moves_exactly_the_admitted_rows(optimizer):
  rng = np.random.RandomState(80)
  B, dim, lr, scale, acc0, F = 120, 8, 0.1, 0.05, 0.1, 3
  lens = rng.poisson(3, size=B).clip(0, 7)
  sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  n_ids = int(sp[-1])
  pool = distinct_keys(rng, 90)
  often, rare, once = pool[:30], pool[30:60], pool[60:]
  # `often` three times each, `rare` once each, the rest of the batch drawn from `often`
  ids = np.concatenate([np.tile(often, 3), rare, often[rng.randint(0, 30, size=n_ids - 120)]])
  rng.shuffle(ids)
  t = HashTable(512, dim, DEV, slab_size=5, init_scale=scale, seed=3, min_freq=F, sketch_width=1 << 15)
  accum = torch.full_like(t.table, acc0)
  hgl = HashGroupLookup([t], combiners='mean')
  grad = GroupLookupGrad(hgl.lookup, accums=[accum], deterministic=optimizer == 'adagrad')
  uniq = np.sort(pool)
  W = ref.init_rows(uniq, dim, 3, scale)
  A = np.full_like(W, F32(acc0))

  def step(ids, admitted_keys):
    """One training step on the device and in the model keyed by raw id: an id that is not admitted is row -1."""
    g = rng.randn(B, dim).astype(F32)
    out = host(hgl([dev(ids)], [dev(sp)])[0])
    index = np.where(np.isin(ids, admitted_keys), np.searchsorted(uniq, ids), -1)
    assert ((host(hgl.slots[0]) >= 0) == (index >= 0)).all()
    w64, mag = model.forward64(W, index, sp, None, 'mean')                 # (-1 counts in the divisor, adds zero)
    assert_sums_close(out, w64, mag, err_msg='forward')
    grad(hgl.slots, [dev(g)], [dev(sp)], apply_lr=lr, optimizer=optimizer)
    want, mag = W.astype(np.float64), np.abs(W).astype(np.float64)
    if optimizer == 'sgd':
      u, g64, gmag = model.backward64(W, index, sp, None, 'mean', g)
      want[u] -= lr * g64
      mag[u] += lr * gmag
      W[u] = want[u].astype(F32)
    else:
      terms, r, valid = model.terms32(uniq.size, index, sp, None, 'mean', g)
      u, sums = model.seq_row_sums(terms, r, valid)
      model.adagrad_step(W, A, u, sums, lr)
      want = W.astype(np.float64)
    slots = host(t.find(dev(uniq)))
    assert ((slots >= 0) == np.isin(uniq, admitted_keys)).all()
    on = slots >= 0
    assert_sums_close(host(t.table)[slots[on]], want[on], mag[on], err_msg='stepped rows')
    if optimizer == 'adagrad':
      assert_sums_close(host(accum)[slots[on]], A[on].astype(np.float64), np.abs(A[on]), err_msg='accumulators')
    W[on] = host(t.table)[slots[on]]                                        # the next step starts from the device's rows
    # the rows no key holds: never written, never stepped
    free = np.setdiff1d(np.arange(t.capacity), slots[on])
    assert not host(t.table)[free].any() and (host(accum)[free] == F32(acc0)).all()
    return u

  moved = step(ids, often)
  np.testing.assert_array_equal(uniq[moved], np.sort(often))                 # exactly the admitted rows moved
  assert t.size() == 30 and t.filtered() == 30
  # `rare` for the second time: still row -1, table and accumulator of nothing but `often` move
  step(ids, often)
  assert t.size() == 30 and t.filtered() == 60
  # the third sighting admits them: this step moves their rows too
  moved = step(ids, np.concatenate([often, rare]))
  np.testing.assert_array_equal(uniq[moved], np.sort(np.concatenate([often, rare])))
  assert t.size() == 60 and t.filtered() == 60
  # launch() continues the count: ids with one occurrence per launch appear on the third
  ids2 = ids.copy()
  ids2[np.isin(ids, rare)] = once
  buf = dev(ids2)
  hgl([buf], [dev(sp)])
  at = np.isin(ids2, once)
  assert (host(hgl.slots[0])[at] == -1).all()
  hgl.launch()
  torch.cuda.synchronize()
  assert (host(hgl.slots[0])[at] == -1).all() and t.size() == 60
  hgl.launch()
  torch.cuda.synchronize()
  assert (host(hgl.slots[0]) >= 0).all() and t.size() == 90 and t.filtered() == 60 + 2 * 30


# ---- 9. moving tables ---------------------------------------------------------------------------------------
def test_load_compact_and_checkpoint(tmp_path):
  rng = np.random.RandomState(90)
  dim, F = 8, 2
  t = HashTable(16 * 32, dim, DEV, slab_size=16, expiring=True, min_freq=F, sketch_width=1 << 15)
  pool = distinct_keys(rng, 300)
  call(t, np.tile(pool[:200], 2), 1)
  call(t, pool[200:260], 2)                                                # seen once: in the sketch, not in the table
  assert t.size() == 200 and t.filtered() == 60
  # load(*items()) into a filtered table of another capacity: every key at once, its sketch untouched
  other = HashTable(1000, dim, DEV, slab_size=8, min_freq=5)
  other.load(*t.items())
  assert other.size() == 200 and other.filtered() == 0 and not host(other.sketch).any()
  for a, b in zip(t.items(), other.items()):
    np.testing.assert_array_equal(host(a), host(b))
  # compact keeps the sketch
  t.set_step(9)
  t.evict(steps_to_live=8)                                                 # the 200 of step 1
  call(t, np.tile(pool[260:300], 2), 9)
  sketch, filtered = host(t.sketch), t.filtered()
  t.compact()
  np.testing.assert_array_equal(host(t.sketch), sketch)
  assert (t.tombstones(), t.size(), t.filtered()) == (0, 40, filtered)
  # a checkpoint of the raw arrays restores the sketch: the next call decides as the unrestored table does
  prefix = str(tmp_path / 'ckpt')
  assert 'user/admission_sketch' in t.variables('user')
  Saver().save(prefix, t.variables('user'))
  back = HashTable(16 * 32, dim, DEV, slab_size=16, expiring=True, min_freq=F, sketch_width=1 << 15)
  Saver().restore(prefix, back.variables('user'))
  back.recount()
  np.testing.assert_array_equal(host(back.sketch), sketch)
  assert back.size() == 40 and back.filtered() == 0
  nxt = np.concatenate([pool[200:260], pool[260:300], distinct_keys(np.random.RandomState(91), 50)])
  a, b = call(t, nxt, 10), call(back, nxt, 10)
  np.testing.assert_array_equal(a >= 0, b >= 0)
  assert (a[:100] >= 0).all() and (a[100:] == -1).sum() > 0                 # the second sighting; new ids wait
  np.testing.assert_array_equal(host(back.sketch), host(t.sketch))
