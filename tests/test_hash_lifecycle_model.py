"""The model of tests/support/hash_lifecycle.py against a numpy device built from the sequential restatements
(hash_ref.fill, hash_expiry_ref.insert / evict, hash_admission_ref.translate, hash_rehash_ref's placement): the
generator, seeds, fixed sequences and checker of tests/test_gpu_hash_lifecycle.py, without a GPU.

Every sequence runs twice; the second time the restatement takes the keys of each call in a permuted order.  Both
pass only if the model predicts nothing that depends on order.  The conditions on the seeds -- how often a subset
is the device's choice, and that every event of the list occurs for every table kind it applies to -- are asserted
here, from the model's own bookkeeping, under both orders."""
import numpy as np
import pytest

from tests.support import hash_lifecycle as hl

SEEDS = hl.SEEDS


def make(order):
  return lambda specs: hl.NumpyFleet(specs, order)


@pytest.fixture(scope='module')
def both_orders():
  """Every seeded sequence under both key orders: {order name: Events}."""
  out = {}
  for name in ('in order', 'permuted'):
    events = hl.Events()
    for seed in SEEDS:
      order = None if name == 'in order' else np.random.RandomState(77 + seed)
      hl.run_seed(seed, make(order), events)
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
