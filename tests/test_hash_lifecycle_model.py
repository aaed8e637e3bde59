"""The model of tests/support/hash_lifecycle.py against a numpy device built from the sequential restatements
(hash_ref.fill, hash_expiry_ref.insert / evict, hash_admission_ref.translate, hash_rehash_ref's placement,
hash_evict_to_ref.evict_to, hash_spill_ref.select / spill, hash_export_ref.export, and a real HashSpillStore): the
generator, seeds, fixed sequences and checker of tests/test_gpu_hash_lifecycle.py, without a GPU.

Every sequence runs twice; the second time the restatement takes the keys of each call in a permuted order.  Both
pass only if the model predicts nothing that depends on order.  The conditions on the seeds -- how often a subset
is the device's choice, and that every event of the list occurs for every table kind it applies to -- are asserted
here, from the model's own bookkeeping, under both orders: for SEEDS the events of hl.BASE_EVENTS, for TIER_SEEDS
(which also draw evict_to, spill, fault_in, export, import and the sequence translate) those of hl.TIER_EVENTS."""
import numpy as np
import pytest

from tests.support import hash_lifecycle as hl

SEEDS = hl.SEEDS
TIER_SEEDS = hl.TIER_SEEDS


def make(order):
  return lambda specs: hl.NumpyFleet(specs, order)


@pytest.fixture(scope='module')
def both_orders():
  """Every seeded sequence under both key orders: {order name: Events}."""
  out = {}
  for name in ('in order', 'permuted'):
    events = hl.Events(hl.BASE_EVENTS)
    for seed in SEEDS:
      order = None if name == 'in order' else np.random.RandomState(77 + seed)
      hl.run_seed(seed, make(order), events)
    out[name] = events
  return out


@pytest.fixture(scope='module')
def tier_both_orders():
  """The same for the TIER_SEEDS."""
  out = {}
  for name in ('in order', 'permuted'):
    events = hl.Events(hl.TIER_EVENTS)
    for seed in TIER_SEEDS:
      order = None if name == 'in order' else np.random.RandomState(77 + seed)
      hl.run_seed(seed, make(order), events, tier=True)
    out[name] = events
  return out


def test_seeded_sequences_pass_in_both_key_orders_and_meet_the_conditions(both_orders):
  for name, events in both_orders.items():
    print(f'--- keys taken {name}: {len(SEEDS)} seeds\n{events.report()}')
  for name, events in both_orders.items():
    assert events.translates > 0
    # (outside the over-full table an adopted subset fails the sequence itself: Runner.apply)
    assert events.adopted <= 0.10 * events.translates, (name, events.adopted, events.translates)
    assert not events.missing(), (name, events.missing())


def test_tier_sequences_pass_in_both_key_orders_and_meet_the_conditions(tier_both_orders):
  for name, events in tier_both_orders.items():
    print(f'--- keys taken {name}: {len(TIER_SEEDS)} tier seeds\n{events.report()}')
  for name, events in tier_both_orders.items():
    assert events.translates > 0
    assert events.adopted <= 0.10 * events.translates, (name, events.adopted, events.translates)
    assert not events.missing(), (name, events.missing())
  # (the two orders need not count alike: after an adopted subset the models differ, and the generator draws from them)


@pytest.mark.parametrize('name', sorted(hl.FIXED))
def test_fixed_sequences_pass_in_both_key_orders(name):
  for order in (None, np.random.RandomState(5)):
    hl.run_fixed(name, make(order))


def test_fixed_sequences_do_what_their_names_say():
  r = hl.run_fixed('refill_of_tombstones', make(None))
  assert r.events.counts.get(('fills_last_slot', 'expiring')) == 3 and r.events.counts.get(('reused', 'expiring'))
  assert r.events.counts.get(('behind_tombstone', 'expiring'))
  assert r.events.counts.get(('overflow', 'expiring')) and r.events.counts.get(('eviction', 'expiring'))
  assert r.fleet.tables[0].tombstones() == 0 and r.fleet.tables[0].size() == 15
  r = hl.run_fixed('sighting_across_evict_and_rehash', make(None))
  assert r.events.counts.get(('exact_admission', 'expiring_admit')) and {-5, 5 + (1 << 32)} <= set(r.models[0].stored)
  r = hl.run_fixed('two_rehashes_around_a_write', make(None))
  assert (r.models[0].slab_size, r.models[0].slab_count) == (33, 6)
  r = hl.run_fixed('spill_chain_and_return', make(None))
  kind = 'expiring_admit'
  assert r.events.counts.get(('fills_last_slot', kind)) == 1 and r.events.counts.get(('overflow', kind))
  assert r.events.counts.get(('spill', kind)) == 2 and r.events.counts.get(('cut_inside_a_step', kind)) == 2
  assert r.events.counts.get(('fault_in', kind)) == 2 and r.events.counts.get(('fault_in_onto_tombstone', kind)) == 1
  assert r.events.counts.get(('respill', kind)) == 1 and r.events.counts.get(('fresh_over_store', kind)) == 1
  assert len(r.models[0].stored) == 15 and not r.models[0].store and len(r.fleet.stores[0]) == 0
  assert (r.models[0].slab_size, r.models[0].slab_count) == (8, 2)
  r = hl.run_fixed('fault_in_that_does_not_fit', make(None))
  assert r.events.counts.get(('fault_in', 'expiring')) == 2 and r.fleet.tables[0].failed() == 6
  assert len(r.models[0].stored) == 21 and len(r.fleet.stores[0]) == 0
  r = hl.run_fixed('snapshot_over_a_moved_table', make(None))
  for event, n in (('import_inserts', 2), ('import_overwrites_stored', 2), ('delta_is_a_proper_subset', 1),
                   ('export_after_rehash', 1), ('eviction', 1), ('cut_inside_a_step', 1)):
    assert r.events.counts.get((event, 'expiring')) == n, event
  assert [len(s) for _, s in r.models[0].snapshots] == [49, 9] and len(r.models[0].stored) == 26


def test_the_checker_sees_a_wrong_table():
  """The checker itself: each of these damages to a correct numpy table must fail it."""
  specs, ops = hl.FIXED['refill_of_tombstones']()

  def damaged(damage):
    r = hl.Runner(hl.NumpyFleet(specs), specs)
    for index, op in enumerate(ops[:3]):
      r.apply(op, index)
    r.apply(hl._call(0, specs[0].pool[:6]), 3)
    damage(r.fleet.tables[0], r.fleet.comps[0])
    with pytest.raises(AssertionError):
      r.check_all()

  def twice(t, c):
    t.keys[np.nonzero(t.keys == hl.TOMBSTONE)[0][0]] = t.keys[np.nonzero(t._live())[0][0]]

  def freq(t, c):
    t.freq[np.nonzero(t.keys == hl.TOMBSTONE)[0][0]] = 1

  def row(t, c):
    t.table[np.nonzero(t._live())[0][0], 3] = -0.0 if t.table[np.nonzero(t._live())[0][0], 3] == 0 else 0.0

  def companion(t, c):
    c[0][np.nonzero(t.keys == hl.TOMBSTONE)[0][0], 1] = 7.0

  def counter(t, c):
    t.stats[1] += 1

  def hidden(t, c):
    t.keys[t.keys == hl.TOMBSTONE] = hl.EMPTY   # EMPTY slots in front of keys that spilled

  for damage in (twice, freq, row, companion, counter, hidden):
    damaged(damage)
  the_tier_checks_see_their_damages()


class Lying(hl.NumpyFleet):
  """A numpy fleet whose answers -- an export, a spill's export, an evict_to report -- pass through `lie` first."""
  lie = None

  def _told(self, out):
    if self.lie is not None:
      self.lie(out[0])
    return out

  def export(self, idx, sinces):
    return self._told(super().export(idx, sinces))

  def spill(self, idx, max_sizes, keep_freq):
    return self._told(super().spill(idx, max_sizes, keep_freq))

  def evict_to(self, idx, max_sizes, keep_freq):
    return self._told(super().evict_to(idx, max_sizes, keep_freq))


def the_tier_checks_see_their_damages():
  """The checks of the bound, the host tier and the export: each of these damages must fail, and none of them
  fails undamaged.  A 3 x 5 expiring table whose rows start as zeros (init_scale 0); eight keys keep them, four are
  written; the older eight are spilled, three come back two steps later."""
  old = hl._homing(3, 1, 12)
  spec = hl.Spec('expiring', 5, 3, 4, [(4, 0.1)], 'tight', np.concatenate([old, [hl.EMPTY, hl.TOMBSTONE]]), seed=3,
                 init_scale=0.0)
  start = [hl._call(0, old[:8]), hl._step(), hl._call(0, old[8:], write=True)]
  export = {'op': 'export', 'tables': [0], 'sinces': [None]}
  spill = {'op': 'spill', 'tables': [0], 'keep': 0, 'max_sizes': [4]}
  evict_to = {'op': 'evict_to', 'tables': [0], 'keep': 0, 'max_sizes': [4]}
  back = [hl._step(2), {'op': 'fault_in', 'table': 0, 'ids': old[:3]}]

  def run(ops, lie=None, damage=None):
    """`ops`, the last of them answered through `lie`; then `damage` to the table and its store, and a check."""
    r = hl.Runner(Lying([spec]), [spec])
    for index, op in enumerate(ops):
      r.fleet.lie = lie if index == len(ops) - 1 else None
      r.apply(op, index)
    if damage is not None:
      damage(r.fleet.tables[0], r.fleet.stores[0], r.models[0])
      r.check_all()

  def minus_zero(exp):
    a = np.nonzero((exp['rows'][:, 0] == 0) & ~np.signbit(exp['rows'][:, 0]))[0][0]
    exp['rows'][a, 0] = -0.0

  def swapped(exp):
    a, b = np.nonzero(exp['rows'][:, 0] == 0)[0][0], np.nonzero(exp['rows'][:, 0] != 0)[0][0]
    exp['rows'][[a, b]] = exp['rows'][[b, a]]

  def off_by_one(report):
    report[3] += 1

  def lacks_a_key(t, store, m):
    import torch
    assert len(store.take(torch.tensor(sorted(m.store)[:1]))) == 1

  def stale_freq(t, store, m):
    store._data[3][1] += 1

  def stamped(t, store, m):
    slot = int(np.nonzero(t.keys == old[1])[0][0])
    assert t.last_seen[slot] == 0 and t.step == 3
    t.last_seen[slot] = t.step

  # (operations, lie, damage, what the failing check must name)
  for ops, lie, damage, names in (
      (start + [export], minus_zero, None, 'the export of table 0: rows'),
      (start + [export], swapped, None, 'the export of table 0: rows'),
      (start + [spill], minus_zero, None, 'the spill of table 0: rows'),
      (start + [dict(spill, max_sizes=[0])], swapped, None, 'the spill of table 0: rows'),
      (start + [evict_to], off_by_one, None, 'the report is [12, 8, 0, 9], not [12, 8, 0, 8]'),
      (start + [spill], None, lacks_a_key, 'the store holds 7 keys, the model\'s 8'),
      (start + [spill], None, stale_freq, 'the store: freq'),
      (start + [spill] + back, None, stamped, 'last_seen')):
    run(ops)
    with pytest.raises(AssertionError) as caught:
      run(ops, lie, damage)
    assert names in str(caught.value), ((lie or damage).__name__, str(caught.value))
