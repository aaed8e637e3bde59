"""tests/support/wide_offsets.py held to its purpose without a GPU: on a sparse-memory model of a gather and of a
row step, every 32-bit mutant of ``base + row * pitch`` that can differ from the true address on a geometry is
noticed by that geometry's probes -- a mismatching probe row, an access outside the array, or a failing
assert_rest_untouched -- and the true address passes.  A condition, not a measurement."""
import numpy as np
import pytest

from tests.support import lowp_ref
from tests.support import wide_offsets as wo

ELEM_SIZES = (4, 2)
CASES = [(g, es) for g in wo.GEOMETRIES.values() for es in ELEM_SIZES]
IDS = [f'{g.name}-es{es}' for g, es in CASES]


def test_thresholds_are_the_four_of_the_issue():
  assert wo.thresholds(4) == [1 << 29, 1 << 30, 1 << 31, 1 << 32]
  assert wo.thresholds(2) == [1 << 30, 1 << 31, 1 << 32]          # byte 2^32 and element 2^31 coincide


def test_geometries_cross_what_they_are_for():
  g = wo.GEOMETRIES
  assert g['E'].dim == 256 and g['E'].rows == (1 << 24) + 1024 and wo.extent(g['E']) > wo.M32
  assert g['E100'].rows == -(-wo.M32 // 100) + 1024
  for t in wo.thresholds(4):
    assert t % 100 and (t - 1) // 100 == t // 100                   # every threshold inside a row
  assert g['P'].rows == 4200 and 4096 * g['P'].pitch > wo.M32 > 4095 * g['P'].pitch
  assert g['R'].dim == 1 and g['R'].rows == wo.M32 + 1024
  for name in ('E', 'E100', 'R'):                                   # 16 GiB in fp32, 8 GiB in 16 bits (+ the margin)
    assert 16 << 30 <= wo.extent(g[name]) * 4 < (16 << 30) + (2 << 20)


@pytest.mark.parametrize('geom,es', CASES, ids=IDS)
def test_probes_sit_on_both_sides_of_every_threshold(geom, es):
  probes, aliases = wo.probe_rows(geom, es)
  assert probes == sorted(set(probes)) and all(0 <= r < geom.rows for r in probes + aliases)
  assert len(probes) <= 4 * 4 + 2
  for t in wo.thresholds(es):
    if t > wo.extent(geom) - 1:
      continue
    hi = t // geom.pitch
    # a probe whose every element lies below T and one at or above it, both within 64 rows of it; the first row at
    # or past T is itself a probe (probe_rows moves rows away from a threshold only below it, see there)
    below = [r for r in probes if r * geom.pitch + geom.dim - 1 < t and r >= hi - 64]
    above = [r for r in probes if r * geom.pitch >= t and r <= hi + 64]
    assert below and above, (geom.name, es, t)
    first_past = hi if hi * geom.pitch >= t else hi + 1
    assert first_past in probes, (geom.name, es, t)
  assert min(probes) <= 64 and max(probes) >= geom.rows - 64        # row 0 and the last row (or what they moved to)
  if geom.name == 'R':
    assert any(r >= wo.M32 for r in probes) and any(wo.M31 <= r < wo.M32 for r in probes)


@pytest.mark.parametrize('geom,es', CASES, ids=IDS)
def test_alias_rows_are_distinct_from_probe_rows(geom, es):
  probes, aliases = wo.probe_rows(geom, es)
  assert not set(probes) & set(aliases)
  for r in probes:
    mine = wo.alias_rows_of(geom, es, r)
    assert set(mine) <= set(aliases) and r not in mine
  # every row a mutant lands on from a probe row is planted: a probe itself (unchanged address) or an alias row
  planted = set(probes) | set(aliases)
  for name, addr in wo.MUTANTS.items():
    for r in probes:
      for k in (0, geom.dim - 1):
        o = addr(geom, es, r, k)
        if 0 <= o < wo.extent(geom):
          assert o // geom.pitch in planted, (name, r, k)


@pytest.mark.parametrize('geom,es', CASES, ids=IDS)
def test_true_address_passes(geom, es):
  assert not wo.model_detects(geom, es, wo.true_offset)


@pytest.mark.parametrize('name', list(wo.MUTANTS))
@pytest.mark.parametrize('geom,es', CASES, ids=IDS)
def test_every_mutant_that_can_differ_is_caught(geom, es, name):
  can = wo.mutant_can_differ(name, geom, es)
  seen = wo.model_detects(geom, es, wo.MUTANTS[name])
  assert seen == can, f'{name} on {geom.name}, {es}-byte elements: can differ {can}, noticed {seen}'


def test_every_mutant_differs_on_some_geometry():
  for name in wo.MUTANTS:
    assert any(wo.mutant_can_differ(name, g, es) for g, es in CASES), name
  # the geometries are the smallest: E and E100 never reach a row number of 2^31, P not even 2^13
  assert not wo.mutant_can_differ('row_i32', wo.GEOMETRIES['E'], 4)
  assert wo.mutant_can_differ('row_u32', wo.GEOMETRIES['R'], 2)
  assert wo.mutant_can_differ('pitch_mul_32', wo.GEOMETRIES['P'], 4)


def test_a_mutant_that_lands_on_zeros_or_outside_is_caught_too():
  """The model's three ways of noticing, one at a time."""
  geom, es = wo.GEOMETRIES['P'], 4
  probes, aliases = wo.probe_rows(geom, es)
  mem = wo.SparseMemory(geom, es, probes, aliases)
  far = next(r for r in probes if wo.M31 <= r * geom.pitch < wo.M32)
  assert mem.gather(wo.MUTANTS['elem_i32'], far)[0] is None and mem.caught        # a negative offset
  mem = wo.SparseMemory(geom, es, probes, aliases)
  mem.step(lambda g, e, r, k: wo.true_offset(g, e, r, k) + g.dim, probes[0])       # into the pitch's padding
  assert not mem.caught and not mem.rest_untouched()
  mem = wo.SparseMemory(geom, es, probes, aliases)
  mem.step(wo.true_offset, probes[0])
  assert mem.rest_untouched() and mem.gather(wo.true_offset, probes[0]) == mem.want_row(probes[0], 0.5)


# ---- WideTable itself, on a small array in host memory -------------------------------------------------------------
@pytest.mark.parametrize('dtype_name', ['float32', 'bfloat16'])
def test_wide_table_plants_gathers_and_notices_stray_writes(dtype_name):
  import torch
  dtype = getattr(torch, dtype_name)
  geom = wo.Geometry('small', 3, 5, 40)
  probes, aliases = [0, 7, 39], [3, 20]
  rng = np.random.RandomState(0)
  if dtype is torch.float32:
    values = rng.uniform(1, 2, size=(5, 3)).astype(np.float32)
  else:
    values = lowp_ref.bf16_nearest(lowp_ref.bits32(rng.uniform(1, 2, size=(5, 3))))
  old_chunk, wo.SCAN_CHUNK = wo.SCAN_CHUNK, 16          # several chunks, the last one short
  try:
    wt = wo.WideTable(geom, dtype, 'cpu').plant(probes, aliases, values)
    assert wt.table.shape == (40, 3) and wt.t.shape == (40, 5)
    np.testing.assert_array_equal(wt.planted, [0, 3, 7, 20, 39])
    np.testing.assert_array_equal(wt.rows([7, 3]), values[[2, 1]])
    np.testing.assert_array_equal(wt.compact_of([39, 0]), [4, 0])
    wt.table[7] += 1                                     # a probe row that was stepped
    wt.assert_rest_untouched([7], 'stepped')
    assert not wt.t.any() and wt.planted.size == 0       # left all zero for the next plant
    wt.plant(probes, aliases, values)
    wt.table[7] += 1
    with pytest.raises(AssertionError, match='changed'):
      wt.assert_rest_untouched([], 'a probe changed that was not to')
    wt = wo.WideTable(geom, dtype, 'cpu').plant(probes, aliases, values)
    wt.table[20] *= 2                                    # an alias row: where a truncating step lands
    with pytest.raises(AssertionError, match=r'rows \[20\]'):
      wt.assert_rest_untouched(probes, 'alias')
    wt = wo.WideTable(geom, dtype, 'cpu').plant(probes, aliases, values)
    wt.t[31, 4] = -0.0 if dtype is torch.float32 else 1.0   # the padding of a row nobody planted (fp32: a bit, not a value)
    with pytest.raises(AssertionError, match='element 159 .row 31, lane 4'):
      wt.assert_rest_untouched(probes, 'padding')
    # keep=True: the stepped row becomes what is planted, the array is left as it was found
    wt = wo.WideTable(geom, dtype, 'cpu').plant(probes, aliases, values)
    wt.table[7] += 1
    before = wt.t.clone()
    wt.assert_rest_untouched([7], 'kept', keep=True)
    assert torch.equal(wt.t, before) and wt.planted.size == 5
    wt.assert_rest_untouched([], 'nothing changed since')
    # over= and adopt(): an array somebody else allocated and wrote two rows of
    own = torch.zeros((40, 5), dtype=dtype)
    wt = wo.WideTable(geom, dtype, 'cpu', over=own)
    wt.write_rows([9, 4], values[:2])
    wt.adopt([9, 4], values[:2]).assert_rest_untouched((), 'adopted')
    assert not own.any()
    wt.write_rows([9, 4], values[:2])
    with pytest.raises(AssertionError, match='changed'):
      wt.adopt([9, 4], values[1:3]).assert_rest_untouched((), 'adopted, other values')
    with pytest.raises(AssertionError, match='only probe rows'):
      wo.WideTable(geom, dtype, 'cpu').plant(probes, aliases, values).assert_rest_untouched([3], 'an alias may not change')
  finally:
    wo.SCAN_CHUNK = old_chunk


def test_slab_pool_reuses_and_zeroes():
  import torch
  geom, small = wo.Geometry('small', 3, 5, 40), wo.Geometry('smaller', 2, 2, 7)
  pool = wo.SlabPool(40 * 5 * 4, 'cpu')
  assert pool.reserve(2, extra=100) == 2 * 800 + 100
  a, b = pool.take(geom, torch.float32), pool.take(small, torch.bfloat16)
  assert a.t.shape == (40, 5) and b.t.shape == (7, 2) and b.t.dtype is torch.bfloat16
  with pytest.raises(AssertionError, match='reserved'):
    pool.take(geom, torch.float32)
  a.t.fill_(3.0)
  slabs = {x.data_ptr() for x in pool.busy}
  pool.release()
  pool.reserve(1)
  c = pool.take(geom, torch.float32)
  assert c.t.data_ptr() in slabs and not c.t.any()         # the same memory, zero again
  pool.release()
  assert len(pool.idle) == 2
  pool.reserve(0, extra=wo.LIMIT_BYTES - (1 << 30))        # no room is left for idle slabs
  assert not pool.idle
  with pytest.raises(AssertionError, match='72 GiB'):
    pool.reserve(1, extra=wo.LIMIT_BYTES)
  with pytest.raises(AssertionError, match='do not fit'):
    pool.reserve(1)
    pool.take(wo.Geometry('big', 3, 5, 41), torch.float32)


# ---- noise_row's high word ---------------------------------------------------------------------------------------
def test_noise_row_without_its_high_word_is_caught_on_R():
  """The stochastic rounding's noise is keyed by the 64-bit row number (lowp_ref.noise).  A device function that
  dropped the upper 32 bits would round row 2^32 + k with the noise of row k: on geometry R's probes at and above
  2^32 the stored bf16 bits of an SGD step differ, below 2^32 they cannot."""
  geom = wo.GEOMETRIES['R']
  probes, _ = wo.probe_rows(geom, 2)
  rows = np.array(probes, np.int64)
  high = rows >= wo.M32
  assert high.sum() >= 2 and (~high).sum() >= 2
  rng = np.random.RandomState(5)
  n = rows.size
  bits = lowp_ref.bf16_nearest(lowp_ref.bits32(rng.uniform(-1, 1, size=(n, geom.dim))))
  g = rng.uniform(-1, 1, size=(n, geom.dim)).astype(np.float32)
  idx = np.arange(n)

  def stepped(noise_rows, seed):
    return lowp_ref.apply_step(bits, 'bf16', [], idx, g, 'sgd', 2.0 ** -9, rounding='stochastic', seed=seed,
                               step=3, col=0, noise_rows=noise_rows)[0]
  differs = np.zeros(n, bool)
  for seed in range(8):     # (one element per row: a single draw agrees by chance half the time)
    true, mutant = stepped(rows, seed), stepped(rows & 0xFFFFFFFF, seed)
    differs |= (true != mutant).any(axis=1)
    # noise_rows defaults to rows: the compact copy with its own numbers is NOT the table's noise
    assert (lowp_ref.noise(seed, 3, 0, rows[high], 4) != lowp_ref.noise(seed, 3, 0, rows[high] & 0xFFFFFFFF, 4)).any()
  assert not differs[~high].any()
  assert differs[high].all(), 'a probe row at or above 2^32 whose bits do not depend on the high word'
