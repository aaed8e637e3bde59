"""Hash tables across their whole life on the GPU: seeded sequences of about 40 operations -- translate through
hash_translate and through the runs entry, finds, sweeps, rehashes of every shape, compact, load, filter aging,
row writes -- on a fleet of 4-6 tables of all four kinds, called fleet-wide, every table checked against the model
of tests/support/hash_lifecycle.py after every operation.  tests/test_hash_lifecycle_model.py drives the same
sequences against the sequential restatements and asserts what the seeds must cover.

Geometries: slab_size in {1, 5, 8, 16, 33, 64}, slab_count in {1, 3, 20, 257}, 5 to about 1300 slots; dim in
{1, 4, 19, 20} with 0-2 companions of width {1, 4, 8}, so rehashes mix 16-byte and 4-byte moves; tables run roomy,
tight (slabs overflow, walks pass tombstones) and, one per fleet, over-full."""
import pytest

from tests.support import hash_lifecycle as hl

pytestmark = pytest.mark.gpu


def make(specs):
  return hl.DeviceFleet(specs, 'cuda:0')


@pytest.mark.parametrize('seed', hl.SEEDS)
def test_seeded_lifecycle(seed):
  hl.run_seed(seed, make)


@pytest.mark.parametrize('name', sorted(hl.FIXED))
def test_fixed_lifecycle(name):
  hl.run_fixed(name, make)
