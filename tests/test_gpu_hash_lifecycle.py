"""Hash tables across their whole life on the GPU: seeded sequences of about 40 operations -- translate through
hash_translate and through the runs entry, finds, sweeps, rehashes of every shape, compact, load, filter aging,
row writes -- on a fleet of 4-6 tables of all four kinds, called fleet-wide, every table checked against the model
of tests/support/hash_lifecycle.py after every operation.  tests/test_hash_lifecycle_model.py drives the same
sequences against the sequential restatements and asserts what the seeds must cover.

Geometries: slab_size in {1, 5, 8, 16, 33, 64}, slab_count in {1, 3, 20, 257}, 5 to about 1300 slots; dim in
{1, 4, 19, 20} with 0-2 companions of width {1, 4, 8}, so rehashes mix 16-byte and 4-byte moves; tables run roomy,
tight (slabs overflow, walks pass tombstones) and, one per fleet, over-full.

The TIER_SEEDS run the same fleets through the later operations as well, about 60 % of their draws: evict_to and
spill_to through hash_evict_to / hash_spill (reports and exports predicted, a real HashSpillStore per expiring table
compared with the model's after every operation), HashTable.fault_in, hash_export over mixed kinds and sinces (the
tables bit-identical afterwards), import_items of older snapshots (whole, by owner, with and without metadata), and
hash_translate_sequence over mixed kinds (truncation, pad ids, tombstones).

Times of one run on an MI355X, per case: the ten SEEDS 0.19-0.43 s (0 2.68 -- the first test of the process,
with its start-up -- 1 0.28, 2 0.25, 3 0.24, 4 0.34, 5 0.24, 6 0.22, 7 0.43, 8 0.22, 9 0.19); the TIER_SEEDS
0.20-0.43 s (11 0.35, 18 0.43, 21 0.31, 22 0.20, 26 0.38, 49 0.27, 54 0.33); the fixed sequences 0.01-0.03 s each.
No tier case takes twice the slowest old seed, so they keep their 40 operations."""
import pytest

from tests.support import hash_lifecycle as hl

pytestmark = pytest.mark.gpu


def make(specs):
  return hl.DeviceFleet(specs, 'cuda:0')


@pytest.mark.parametrize('seed', hl.SEEDS)
def test_seeded_lifecycle(seed):
  hl.run_seed(seed, make)


@pytest.mark.parametrize('seed', hl.TIER_SEEDS)
def test_seeded_tier_lifecycle(seed):
  hl.run_seed(seed, make, tier=True)


@pytest.mark.parametrize('name', sorted(hl.FIXED))
def test_fixed_lifecycle(name):
  hl.run_fixed(name, make)
