"""Every row-addressing kernel past 2^32 elements and 2^32 rows (tests/support/wide_offsets.py).

A kernel that forms ``base + row * pitch`` is right only if the product is carried in 64 bits on every path.  Each
test here runs one op on a table whose probe rows sit on both sides of the four thresholds of its element size --
byte offset 2^31 and 2^32, element offset 2^31 and 2^32 -- and compares the HIP path with the host reference the
small-shape test of the same op uses, on a compact copy of the planted rows, with that test's comparison (bit for
bit wherever that one is).  Gradients come from tests/support/exact.py: fp32 sums are exact in any order, so a
repeated row compares bit for bit under every reduce plan.  A step is followed by assert_rest_untouched: the alias
rows a truncating kernel would land on hold what was planted, and nothing else in the array is non-zero.

The tables are never on the host.  Every test states the HBM it needs (its docstring and POOL.reserve: slabs of 17
GiB that the wide arrays are views of, and the bytes something else allocates) and skips when that does not fit
with 4 GiB to spare; none holds more than 72 GiB, idle slabs kept for the next test included (wide_offsets.SlabPool
says why they are kept).  The file name sorts last on purpose (tests/conftest.py)."""
import ctypes as C
import gc
import time

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
import oracle
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (GroupLookup, GroupLookupGrad, LazyAdam, Ftrl, RowwiseAdagrad)
from hybridbackend_amd.embedding.expand import ExpandIndex, expand_rows, expand_rows_grad
from hybridbackend_amd.embedding.lowp import (LowpGroupLookup, LowpLookupGrad, LowpSparseApply,
                                              LowpShardedGroupLookup)
from hybridbackend_amd.embedding.sequence import SequenceLookup, SequenceLookupGrad
from hybridbackend_amd.embedding.sharded import ShardedGroupLookup
from hybridbackend_amd.embedding.sparse_apply import SparseApply
from tests.support import exact, expand_ref, lowp_ref, reference, rowwise_adagrad_ref, sequence_ref, weight_grad_ref
from tests.support import wide_offsets as wo
from tests.support.tolerance import assert_sums_close

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32 = np.float32
GiB = 1 << 30
TORCH = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
LR = exact.EXACT_LR
BLOCK_ROWS, BLOCK_PITCH = (1 << 16) + 8, (1 << 16) + 4     # a block whose last rows start past 2^32 floats
HASH_CAP, HASH_CAP2, HASH_DIM, HASH_SLAB = (1 << 24) + (1 << 20), (1 << 24) + (1 << 21), 256, 8
# one slab holds the largest array a test plants: a companion of the hash table's value array (17 GiB; the pitched
# geometry P takes 16.4 GiB, E, E100, R and the blocks 16 GiB in fp32)
POOL = wo.SlabPool(HASH_CAP * HASH_DIM * 4, DEV)


@pytest.fixture(autouse=True)
def _cost(record_property):
  """Wall time and peak HBM of every test (the junit properties and the captured output); 72 GiB is the limit.  The
  slabs of the test go back to the pool."""
  if torch.cuda.memory_allocated() > GiB:   # (what a test before left in a cycle or a traceback)
    gc.collect()
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  t0 = time.perf_counter()
  yield
  torch.cuda.synchronize()
  POOL.release()
  peak, dt = torch.cuda.max_memory_allocated(), time.perf_counter() - t0
  record_property('wall_s', round(dt, 2))
  record_property('peak_GiB', round(peak / GiB, 2))
  print(f'wide-offsets cost: {dt:.2f} s, peak {peak / GiB:.2f} GiB')
  assert peak <= 72 * GiB, 'a wide-offsets test may not hold more than 72 GiB'


def dev(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
  return t.detach().cpu().numpy()


def grid_rows(rng, n, dim):
  """fp32 [n, dim] on the exact grid 2^-4, |w| <= 4, no zero element (a planted row is non-zero everywhere: a
  gather that lands on unplanted memory differs in every lane)."""
  v = exact.exact_tables(rng, n, dim)
  v[v == 0] = F32(0.0625)
  return v


class Case:
  """One geometry with its probe and alias rows, the planted table and planted fp32 slot arrays."""

  def __init__(self, geom, dtype='fp32', seed=0, slots32=False):
    self.geom = wo.GEOMETRIES[geom] if isinstance(geom, str) else geom
    self.dtype = dtype
    es = 4 if dtype == 'fp32' else 2
    # fp32 slot arrays of a 16-bit table cross their thresholds at other rows: the union of both
    self.es = (2, 4) if (slots32 and es == 2) else es
    self.probes, self.aliases = wo.probe_rows(self.geom, self.es)
    self.planted = np.array(sorted(self.probes + self.aliases), np.int64)
    self.rng = np.random.RandomState(seed)
    self.n, self.dim = self.planted.size, self.geom.dim
    self.p = np.array(self.probes, np.int64)
    self.cp = wo.compact(self.planted, self.p)       # the probes' numbers in the compact copy

  def table(self, into=None):
    """A new planted table, or fresh values planted into the all-zero `into` (same tensor, same address)."""
    v = grid_rows(self.rng, self.n, self.dim)
    if self.dtype != 'fp32':
      v = lowp_ref.round_nearest(lowp_ref.bits32(v), self.dtype)       # (the grid is exact in both 16-bit types)
    wt = POOL.take(self.geom, TORCH[self.dtype]) if into is None else into
    return wt.plant(self.probes, self.aliases, v)

  def ragged(self, n_ids):
    """int32 row_splits over exactly n_ids ids with lengths 0, 1, 2 and 4 (a mean over them is exact)."""
    lens, left = [], int(n_ids)
    while left:
      k = int(self.rng.choice([0, 1, 2, 4]))
      lens.append(k if k <= left else 1)
      left -= lens[-1]
    return exact.splits_of(np.array(lens + [0], np.int64))

  def slot(self, lo, hi, rowwise=False):
    """An fp32 array of the table's shape (rowwise: [rows, 1]) planted with uniform(lo, hi) at the same rows."""
    geom = wo.Geometry(self.geom.name + '/row', 1, 1, self.geom.rows) if rowwise else self.geom
    v = self.rng.uniform(lo, hi, size=(self.n, geom.dim)).astype(F32)
    return POOL.take(geom, torch.float32).plant(self.probes, self.aliases, v)

  def compact(self, rows):
    return wo.compact(self.planted, np.asarray(rows, np.int64))

  def ids(self, id_dtype=np.int64, unbucketized=False):
    return wo.draw_ids(self.rng, self.probes, id_dtype, self.geom.rows, unbucketized)

  def slices(self, grads=None):
    """Caller-held IndexedSlices over the probe rows: shuffled, -1 holes in between, stale entries past n_unique.
    Returns ((unique_rows, grad_rows, n_unique) on the device, the probe rows in slice order, their fp32 gradient)."""
    k = self.p.size
    order = self.rng.permutation(k)
    rows = self.p[order]
    g = self.rng.uniform(-1, 1, size=(k, self.dim)).astype(F32) if grads is None else grads[order]
    cap = 2 * k + 5
    urows, gs = np.full(cap, -1, np.int64), np.full((cap, self.dim), np.nan, F32)
    urows[0:2 * k:2], gs[0:2 * k:2] = rows, g
    gs[1:2 * k:2] = 1e30
    urows[2 * k:] = self.p[:5]
    return (dev(urows), dev(gs), torch.tensor([2 * k], dtype=torch.int32, device=DEV)), rows, g


# ---- a. fp32 forward ---------------------------------------------------------------------------------------------------------
FWD_CASES = [('E', np.int32, 0), ('E', np.int64, 0), ('E', np.int32, 1), ('E', np.int64, 1),
             ('E100', np.int32, 0), ('E100', np.int64, 0), ('R', np.int64, 1)]


@pytest.mark.parametrize('geom,id_dtype,hot', FWD_CASES,
                         ids=[f'{g}-{np.dtype(d).name}-hot{h}' for g, d, h in FWD_CASES])
def test_fp32_forward(hbk_option, geom, id_dtype, hot):
  """GroupLookup: one id per sample with a bucket, ragged mean, weighted ragged sum and the max_norm clip; with
  fwd_hot_rows 0 and 1 on E; on R (ids un-bucketized, row + k * rows: the floor-mod's divisor is above 2^32) the
  column is served with the hot-row hint set.  HBM: one fp32 table, 16 GiB."""
  c = Case(geom, 'fp32', seed=11)
  POOL.reserve(1)
  hbk_option('fwd_hot_rows', hot)
  wt = c.table()
  rows_n = c.geom.rows
  i64 = id_dtype == np.int64
  what = f'{geom} {np.dtype(id_dtype).name} hot {hot}'
  # one id per sample, bucketized by the kernel
  ids, r = c.ids(id_dtype, unbucketized=i64)
  np.testing.assert_array_equal(oracle.floormod(ids.astype(np.int64), rows_n), r)
  lookup = GroupLookup([wt.table], buckets=[rows_n], combiners='sum', hot_rows=bool(hot))
  out = lookup([dev(ids)])[0]
  want = oracle.group_lookup_fwd([wt.values], [c.compact(r)], [None], None, ['sum'])[0]
  exact.assert_bits_equal(host(out), want, f'{what}: one id per sample')
  # ragged mean (lengths 1, 2, 4: exact on the grid, and the oracle's sequential fp32 sum)
  ids, r = c.ids(id_dtype, unbucketized=i64)
  splits = c.ragged(r.size)
  n_ids = r.size
  out = GroupLookup([wt.table], buckets=[rows_n], combiners='mean')([dev(ids)], [dev(splits)])[0]
  want = oracle.group_lookup_fwd([wt.values], [c.compact(r)], [splits], None, ['mean'])[0]
  exact.assert_bits_equal(host(out), want, f'{what}: ragged mean')
  # weighted ragged sum (weights and rows on grids: every fp32 sum is exact, so float64's bits)
  w = exact.exact_weights(c.rng, splits, n_ids, 'sum')
  out = GroupLookup([wt.table], buckets=[rows_n], combiners='sum')([dev(ids)], [dev(splits)], sp_weights=[dev(w)])[0]
  want64, _ = reference.forward64(wt.values, c.compact(r), splits, w, 'sum')
  np.testing.assert_array_equal(host(out), want64.astype(F32), err_msg=f'{what}: weighted sum')
  assert (want64.astype(F32).astype(np.float64) == want64).all()
  # max_norm: some rows inside the ball, some outside (the small-shape test's bound)
  norms = np.sqrt((wt.values.astype(np.float64) ** 2).sum(1))
  clip = float(F32(np.median(norms[c.cp])))
  out = GroupLookup([wt.table], buckets=[rows_n], combiners='sum', max_norms=clip)([dev(ids)], [dev(splits)])[0]
  want64, mag = reference.forward64(wt.values, c.compact(r), splits, None, 'sum', max_norm=clip)
  assert_sums_close(host(out), want64, mag, err_msg=f'{what}: max_norm {clip}')
  torch.cuda.synchronize()
  wt.assert_rest_untouched((), what)       # a forward writes no table


def test_fp32_forward_into_a_block_past_2_32_floats():
  """Output into a block [2^16 + 8, 2^16 + 4]: the last segments' output offsets pass 2^32 floats; every segment is
  compared with torch's own gather, the probe segments of the block with the oracle, and the block's padding stays
  zero.  HBM: an fp32 table (16 GiB) and the block (16 GiB)."""
  c = Case('E', 'fp32', seed=12)
  block_geom = wo.Geometry('block', c.dim, BLOCK_PITCH, BLOCK_ROWS)
  POOL.reserve(2, GiB)
  wt = c.table()
  off = 1 << 12
  block = POOL.take(block_geom, torch.float32)
  r = c.p[c.rng.randint(0, c.p.size, size=BLOCK_ROWS)]
  d_ids = dev(r)
  lookup = GroupLookup([wt.table], buckets=[c.geom.rows], combiners='sum')
  assert lookup.bind_block([d_ids], None, block.t, [off])
  lookup.launch()
  torch.cuda.synchronize()
  col = block.t[:, off:off + c.dim]
  at = torch.from_numpy(c.compact(r)).to(DEV)
  assert torch.equal(col, dev(wt.values)[at]), 'a segment of the block differs from its row'
  segs, _ = wo.probe_rows(block_geom, 4)
  want = oracle.group_lookup_fwd([wt.values], [c.compact(r[segs])], [None], None, ['sum'])[0]
  got = host(torch.cat([block.t.narrow(0, s, 1)[:, off:off + c.dim] for s in segs]))
  exact.assert_bits_equal(got, want, 'probe segments of the block')
  col.zero_()
  block.assert_rest_untouched((), 'the block around its column')


# ---- b. fp32 backward and fused step ---------------------------------------------------------------------------------------
def _exact_backward_inputs(c, unbucketized, id_dtype=np.int64):
  ids, r = c.ids(id_dtype, unbucketized)
  bits = exact.exact_terms_budget(r, 0, c.geom.name)
  g = exact.exact_grads(c.rng, (r.size, c.dim), min(bits, 6))
  return ids, r, g


def _check_emitted(c, res, r, g, det, what, sums=None):
  urows, grows, nu = res
  k = int(nu.item())
  if sums is None:
    sums = exact.exact_dense((c.n, c.dim), c.compact(r), g, case=what)
  got_u = host(urows)[:k]
  order = np.argsort(got_u, kind='stable')
  np.testing.assert_array_equal(got_u[order], c.planted[sums.rows], err_msg=f'{what}: rows')
  if det:
    assert (np.diff(got_u) > 0).all(), f'{what}: a deterministic plan emits rows ascending'
  exact.assert_bits_equal(host(grows)[:k][order], sums.sums(), f'{what}: sums', unit=sums.unit[sums.rows],
                          rows=c.planted[sums.rows])
  return sums, got_u


BWD_CASES = [('E', np.int64), ('E', np.int32), ('R', np.int64)]


@pytest.mark.parametrize('det', [0, 1, 2])
@pytest.mark.parametrize('geom,id_dtype', BWD_CASES, ids=[f'{g}-{np.dtype(d).name}' for g, d in BWD_CASES])
def test_fp32_backward_emit_sgd_adagrad(hbk_option, record_property, geom, id_dtype, det):
  """GroupLookupGrad: emit, apply_lr with SGD, and Adagrad, under bwd_deterministic 0, 1 and 2; the table and the
  accumulator through assert_rest_untouched.  int32 and int64 ids on E; on R the ids arrive un-bucketized.  HBM: fp32
  table and accumulator, 32 GiB."""
  c = Case(geom, 'fp32', seed=20 + det)
  POOL.reserve(2)
  hbk_option('bwd_deterministic', det)
  what = f'{geom} {np.dtype(id_dtype).name} det {det}'
  wt = c.table()
  acc = POOL.take(c.geom, torch.float32)
  lookup = GroupLookup([wt.table], buckets=[c.geom.rows], combiners='sum')
  grad = GroupLookupGrad(lookup, accums=[acc.table])
  ids, r, g = _exact_backward_inputs(c, geom == 'R', id_dtype)
  d_ids, d_g = dev(ids), dev(g)
  # emit
  res = grad([d_ids], [d_g])[0]
  torch.cuda.synchronize()
  sums, got_u = _check_emitted(c, res, r, g, det, f'{what} emit')
  if geom == 'R' and det == 0:
    # no plan is asked for: what the library picks on its own for 2^32 + 1024 rows shows in the order the rows
    # leave in (the row-sorted plans, which the host keeps to tables below 2^32 rows, emit ascending)
    ascending = bool((np.diff(got_u) > 0).all())
    record_property('rows_emitted_ascending', ascending)
    print(f'{what}: rows emitted ascending: {ascending} (the row-sorted plans are kept to tables of fewer than 2^32 rows)')
  wt.assert_rest_untouched((), f'{what} emit')
  # SGD
  wt = c.table(into=wt)
  res = grad([d_ids], [d_g], apply_lr=LR)[0]
  torch.cuda.synchronize()
  _check_emitted(c, res, r, g, det, f'{what} sgd', sums)
  want = exact.exact_sgd(wt.values, sums, LR, what)
  exact.assert_bits_equal(wt.rows(c.p), want[c.cp], f'{what}: stepped rows', rows=c.p)
  wt.assert_rest_untouched(c.probes, f'{what} sgd')
  # Adagrad
  wt = c.table(into=wt)
  acc = acc.plant(c.probes, c.aliases, c.rng.uniform(0.1, 0.5, size=(c.n, c.dim)).astype(F32))
  res = grad([d_ids], [d_g], apply_lr=0.05, optimizer='adagrad')[0]
  torch.cuda.synchronize()
  _check_emitted(c, res, r, g, det, f'{what} adagrad', sums)
  want_t, want_a = wt.values.copy(), acc.values.copy()
  oracle.sparse_adagrad_apply(want_t, want_a, sums.rows, sums.sums(), 0.05)
  exact.assert_bits_equal(wt.rows(c.p), want_t[c.cp], f'{what}: Adagrad rows', rows=c.p)
  exact.assert_bits_equal(acc.rows(c.p), want_a[c.cp], f'{what}: accumulator rows', rows=c.p)
  wt.assert_rest_untouched(c.probes, f'{what} adagrad table')
  acc.assert_rest_untouched(c.probes, f'{what} adagrad accumulator')


@pytest.mark.parametrize('det', [0, 1, 2])
def test_fp32_backward_gradients_from_a_block_past_2_32_floats(hbk_option, det):
  """Gradients read from a block with grad_stride 2^16 + 4 over 2^16 + 8 segments (the last segments' gradient rows
  start past 2^32 floats): emit and the SGD step.  HBM: fp32 table (16 GiB) and the gradient block (16 GiB)."""
  c = Case('E', 'fp32', seed=30 + det)
  block_geom = wo.Geometry('block', c.dim, BLOCK_PITCH, BLOCK_ROWS)
  POOL.reserve(2, GiB)
  hbk_option('bwd_deterministic', det)
  what = f'grad block det {det}'
  wt = c.table()
  off = 1 << 12
  block = POOL.take(block_geom, torch.float32).t
  gen = torch.Generator(device=DEV)
  gen.manual_seed(30 + det)
  # exact grid: integers in [-16, 16] / 16; at most 2^16 + 8 terms in a row: 5 + 17 bits
  block[:, off:off + c.dim] = torch.randint(-16, 17, (BLOCK_ROWS, c.dim), device=DEV, generator=gen).float() / 16
  g = host(block[:, off:off + c.dim])
  r = c.p[c.rng.randint(0, c.p.size, size=BLOCK_ROWS)]
  d_ids = dev(r)
  lookup = GroupLookup([wt.table], buckets=[c.geom.rows], combiners='sum')
  grad = GroupLookupGrad(lookup)
  res = grad([d_ids], None, grad_block=(block, [off]))[0]
  torch.cuda.synchronize()
  sums, _ = _check_emitted(c, res, r, g, det, f'{what} emit')
  res = grad([d_ids], None, grad_block=(block, [off]), apply_lr=LR)[0]
  torch.cuda.synchronize()
  _check_emitted(c, res, r, g, det, f'{what} sgd', sums)
  want = exact.exact_sgd(wt.values, sums, LR, what)
  exact.assert_bits_equal(wt.rows(c.p), want[c.cp], f'{what}: stepped rows', rows=c.p)
  wt.assert_rest_untouched(c.probes, what)


@pytest.mark.parametrize('optimizer', ['sgd', 'adagrad'])
def test_fp32_backward_table_pitch(optimizer):
  """table_pitch on P (20 floats every 2^20 + 4: row 4096 starts past 2^32 floats): the fused SGD and Adagrad steps
  through the descriptor's pitch, table and accumulator -- padding included -- through assert_rest_untouched.
  HBM: two pitched fp32 arrays, 33 GiB."""
  c = Case('P', 'fp32', seed=40)
  POOL.reserve(2, GiB)
  wt = c.table()
  acc = c.slot(0.1, 0.5)
  # the Python wrapper takes contiguous tables: a stand-in gives the shapes, the descriptor the real addresses
  stand_in = torch.zeros((c.geom.rows, c.dim), dtype=torch.float32, device=DEV)
  grad = GroupLookupGrad(GroupLookup([stand_in], buckets=[c.geom.rows], combiners='sum'),
                         accums=[torch.zeros_like(stand_in)])
  col = grad._cols[0]
  col.table, col.accum, col.table_pitch = wt.t.data_ptr(), acc.t.data_ptr(), c.geom.pitch
  ids, r, g = _exact_backward_inputs(c, False)
  lr = LR if optimizer == 'sgd' else 0.05
  res = grad([dev(ids)], [dev(g)], apply_lr=lr, optimizer=optimizer)[0]
  torch.cuda.synchronize()
  sums, _ = _check_emitted(c, res, r, g, 0, f'P {optimizer}')
  assert not stand_in.any()
  if optimizer == 'sgd':
    want = exact.exact_sgd(wt.values, sums, lr, 'P')
    exact.assert_bits_equal(wt.rows(c.p), want[c.cp], 'P: stepped rows', rows=c.p)
    acc.assert_rest_untouched((), 'P sgd accumulator')
  else:
    want_t, want_a = wt.values.copy(), acc.values.copy()
    oracle.sparse_adagrad_apply(want_t, want_a, sums.rows, sums.sums(), lr)
    exact.assert_bits_equal(wt.rows(c.p), want_t[c.cp], 'P: Adagrad rows', rows=c.p)
    exact.assert_bits_equal(acc.rows(c.p), want_a[c.cp], 'P: accumulator rows', rows=c.p)
    acc.assert_rest_untouched(c.probes, 'P adagrad accumulator')
  wt.assert_rest_untouched(c.probes, f'P {optimizer} table')


# ---- c. sparse apply ---------------------------------------------------------------------------------------------------------
FTRL = dict(l1=0.01, l2=0.02, l2_shrinkage=0.03, lr_power=-0.5)
ROWWISE_EPS = 1e-8


def _apply_reference(optimizer, w, slots, rows, g, lr, vec4=True):
  """The step of tests/support/reference.py / rowwise_adagrad_ref.py on compact fp32 arrays, in place."""
  if optimizer == 'sgd':
    reference.sgd_step(w, rows, g, lr)
  elif optimizer == 'adagrad':
    reference.adagrad_step(w, slots[0], rows, g, lr)
  elif optimizer == 'adam':
    reference.adam_step(w, slots[0], slots[1], rows, g, lr, reference.ADAM_DEFAULTS[:2])
  elif optimizer == 'ftrl':
    reference.ftrl_step(w, slots[0], slots[1], rows, g, lr, **FTRL)
  else:
    rowwise_adagrad_ref.step(w, slots[0], rows, g, lr, ROWWISE_EPS, vec4)


def _slot_arrays(c, optimizer):
  """(the planted slot WideTables, the constructor keywords of SparseApply / LowpSparseApply over them)."""
  if optimizer == 'adagrad':
    s = [c.slot(0.1, 0.5)]
    return s, dict(accums=[s[0].table])
  if optimizer == 'adam':
    s = [c.slot(-0.1, 0.1), c.slot(0.001, 0.1)]
    return s, dict(moments=[(s[0].table, s[1].table)], adam=LazyAdam())
  if optimizer == 'ftrl':
    s = [c.slot(0.1, 0.5), c.slot(-0.1, 0.1)]
    return s, dict(ftrl_slots=[(s[0].table, s[1].table)], ftrl=Ftrl(**FTRL))
  if optimizer == 'rowwise_adagrad':
    s = [c.slot(0.1, 0.5, rowwise=True)]
    return s, dict(row_accums=[s[0].table], rowwise_adagrad=RowwiseAdagrad(epsilon=ROWWISE_EPS))
  return [], {}


SLOT_ARRAYS = {'sgd': 0, 'adagrad': 1, 'adam': 2, 'ftrl': 2, 'rowwise_adagrad': 1}
APPLY_CASES = [('E', 'adam'), ('E', 'ftrl'), ('E', 'rowwise_adagrad'), ('R', 'rowwise_adagrad')]


@pytest.mark.parametrize('geom,optimizer', APPLY_CASES, ids=[f'{g}-{o}' for g, o in APPLY_CASES])
def test_sparse_apply(geom, optimizer):
  """SparseApply on caller-held slices over the probe rows: Lazy Adam (both moments), FTRL (both slots, lr_power
  -0.5) and row-wise Adagrad on E; row-wise Adagrad also on R, where the accumulator is indexed by the row number.
  Every slot array is checked like the table.  HBM: the fp32 table and up to two fp32 slot arrays, 48 GiB (R: 32)."""
  c = Case(geom, 'fp32', seed=50)
  POOL.reserve(1 + SLOT_ARRAYS[optimizer], GiB)
  what = f'{geom} {optimizer}'
  wt = c.table()
  slots, kw = _slot_arrays(c, optimizer)
  slices, rows, g = c.slices()
  SparseApply([wt.table], **kw)([slices], 0.05, optimizer)
  torch.cuda.synchronize()
  w, s = wt.values.copy(), [x.values.copy() for x in slots]
  _apply_reference(optimizer, w, s, c.compact(rows), g, 0.05, vec4=c.dim % 4 == 0)
  exact.assert_bits_equal(wt.rows(c.p), w[c.cp], f'{what}: table rows', rows=c.p)
  wt.assert_rest_untouched(c.probes, f'{what}: table')
  for k, (x, want) in enumerate(zip(slots, s)):
    exact.assert_bits_equal(x.rows(c.p), want[c.cp], f'{what}: slot {k} rows', rows=c.p)
    x.assert_rest_untouched(c.probes, f'{what}: slot {k}')
  if optimizer == 'adam':
    exact.assert_bits_equal(host(kw['adam'].beta_powers),
                            np.array(reference.adam_finish(reference.ADAM_DEFAULTS[:2]), F32), 'beta powers')


@pytest.mark.parametrize('optimizer', ['adam', 'ftrl', 'rowwise_adagrad', 'sgd'])
def test_sparse_apply_table_pitch(optimizer):
  """hbk_sparse_apply_slices_n with table_pitch on P, through the C ABI (the wrapper takes contiguous tables): the
  slots of Adam and FTRL lie at the table's pitch.  HBM: up to three pitched fp32 arrays, 50 GiB."""
  c = Case('P', 'fp32', seed=51)
  POOL.reserve(1 + SLOT_ARRAYS[optimizer], GiB)
  what = f'P {optimizer}'
  wt = c.table()
  if optimizer == 'adam':
    slots, opt = [c.slot(-0.1, 0.1), c.slot(0.001, 0.1)], LazyAdam()
  elif optimizer == 'ftrl':
    slots, opt = [c.slot(0.1, 0.5), c.slot(-0.1, 0.1)], Ftrl(**FTRL)
  elif optimizer == 'rowwise_adagrad':
    slots, opt = [c.slot(0.1, 0.5, rowwise=True)], RowwiseAdagrad(epsilon=ROWWISE_EPS)
  else:
    slots, opt = [], None
  slices, rows, g = c.slices()
  col = (_lib.SlicesColumn * 1)()
  col[0].table, col[0].rows, col[0].dim, col[0].table_pitch = wt.t.data_ptr(), c.geom.rows, c.dim, c.geom.pitch
  col[0].unique_rows, col[0].grad_rows, col[0].n_unique = (x.data_ptr() for x in slices)
  col[0].capacity = slices[0].numel()
  from hybridbackend_amd.embedding.sparse_apply import _APPLY
  s0 = _lib.ptr_array([slots[0].t.data_ptr()]) if slots else None
  s1 = _lib.ptr_array([slots[1].t.data_ptr()]) if len(slots) > 1 else None
  params = C.byref(opt.params(True)) if opt is not None else None
  _lib.check(_lib.lib().hbk_sparse_apply_slices_n(1, col, _APPLY[optimizer], s0, s1, params, C.c_float(0.05),
                                                  _lib.current_stream(torch.device(DEV))))
  torch.cuda.synchronize()
  w, s = wt.values.copy(), [x.values.copy() for x in slots]
  # (a pitch of 2^20 + 4 floats keeps rows 16-byte aligned: the row-wise sum takes 4-float chunks)
  _apply_reference(optimizer, w, s, c.compact(rows), g, 0.05, vec4=True)
  exact.assert_bits_equal(wt.rows(c.p), w[c.cp], f'{what}: table rows', rows=c.p)
  wt.assert_rest_untouched(c.probes, f'{what}: table')
  for k, (x, want) in enumerate(zip(slots, s)):
    exact.assert_bits_equal(x.rows(c.p), want[c.cp], f'{what}: slot {k} rows', rows=c.p)
    x.assert_rest_untouched(c.probes, f'{what}: slot {k}')


def test_clipped_sgd_step():
  """SGD with the clip pass of the apply (GroupLookupGrad over a lookup with max_norms) on E: the stepped rows against
  the float64 clip Jacobian with the small-shape test's bound; the rest of the table untouched.  HBM: 16 GiB."""
  c = Case('E', 'fp32', seed=52)
  POOL.reserve(1, GiB)
  wt = c.table()
  norms = np.sqrt((wt.values.astype(np.float64) ** 2).sum(1))
  clip = float(F32(np.median(norms[c.cp])))
  ids, r, g = _exact_backward_inputs(c, False)
  lookup = GroupLookup([wt.table], buckets=[c.geom.rows], combiners='sum', max_norms=clip)
  res = GroupLookupGrad(lookup)([dev(ids)], [dev(g)], apply_lr=0.05)[0]
  torch.cuda.synchronize()
  u, gp, gm = reference.backward64(wt.values, c.compact(r), None, None, 'sum', g, max_norm=clip)
  np.testing.assert_array_equal(c.planted[u], c.p)
  k = int(res[2].item())
  got_u = host(res[0])[:k]
  order = np.argsort(got_u)
  np.testing.assert_array_equal(got_u[order], c.p)
  assert_sums_close(host(res[1])[:k][order], gp, gm, err_msg='clipped gradient rows')
  pre = wt.values[c.cp].astype(np.float64)
  assert_sums_close(wt.rows(c.p), pre - 0.05 * gp, np.abs(pre) + 0.05 * gm, err_msg='clipped SGD rows')
  wt.assert_rest_untouched(c.probes, 'clipped SGD')


# ---- d. sp_weights gradient --------------------------------------------------------------------------------------------------
def test_weight_gradient():
  """hbk_group_lookup_bwd_weights on E, ragged weighted mean: rows, gradients and weights on grids on which every
  dot product and every quotient is exact, so the fp32 result equals weight_grad_ref's float64 one.  HBM: 16 GiB."""
  c = Case('E', 'fp32', seed=60)
  POOL.reserve(1, GiB)
  wt = c.table()
  ids, r = c.ids(np.int64, unbucketized=True)
  splits = c.ragged(r.size)
  n_ids, lens = r.size, np.diff(splits)
  w = exact.exact_weights(c.rng, splits, n_ids, 'mean')
  g = exact.exact_grads(c.rng, (lens.size, c.dim), 4)                    # |e| <= 2^6, |g| <= 2^4 grids, 256 lanes, 4 ids
  lookup = GroupLookup([wt.table], buckets=[c.geom.rows], combiners='mean')
  _, wg = GroupLookupGrad(lookup)([dev(ids)], [dev(g)], [dev(splits)], sp_weights=[dev(w)], weight_grads=True)
  torch.cuda.synchronize()
  want, _, _ = weight_grad_ref.weight_grad(wt.values, c.compact(r), splits, w, 'mean', g)
  assert (want.astype(F32).astype(np.float64) == want).all(), 'the reference is not exact in fp32: shrink the grids'
  np.testing.assert_array_equal(host(wg[0]), want.astype(F32))
  assert np.count_nonzero(want) > n_ids // 4
  wt.assert_rest_untouched((), 'weight gradient')


# ---- e. sequence lookup and backward ---------------------------------------------------------------------------------------
def test_sequence_lookup_and_backward():
  """SequenceLookup on E with max_len 4 and a pad id, the output through out_stride 2^16 + 4 over 2^16 + 8 samples
  (the last samples' rows start past 2^32 floats); then the backward's SGD step.  HBM: table and output block,
  32 GiB."""
  c = Case('E', 'fp32', seed=70)
  T, B = 4, BLOCK_ROWS
  assert T * c.dim <= BLOCK_PITCH
  block_geom = wo.Geometry('samples', T * c.dim, BLOCK_PITCH, B)
  POOL.reserve(2, 2 * GiB)
  wt = c.table()
  pad_row = int(c.p[1])
  lens = c.rng.randint(0, 7, size=B)                   # some longer than max_len, some empty
  splits = exact.splits_of(lens)
  r = c.p[c.rng.randint(0, c.p.size, size=int(splits[-1]))]
  block = POOL.take(block_geom, torch.float32)
  out = block.t.as_strided((B, T, c.dim), (BLOCK_PITCH, c.dim, 1))
  seq = SequenceLookup([wt.table], buckets=[c.geom.rows], max_lens=T, pad_ids=pad_row)
  outs, lengths = seq([dev(r)], [dev(splits)], outs=[out])
  torch.cuda.synchronize()
  grid, want_len = sequence_ref.grid_ref(r, splits, c.geom.rows, T, pad_row)
  np.testing.assert_array_equal(host(lengths[0]), want_len)
  np.testing.assert_array_equal(host(seq.grids[0]).reshape(-1), grid)
  cgrid = c.compact(grid)                             # (with a pad id every position looks a row up)
  samples, _ = wo.probe_rows(block_geom, 4)
  want = sequence_ref.forward_ref(wt.values, cgrid.reshape(B, T)[samples].reshape(-1), T)
  got = host(torch.cat([block.t.narrow(0, s, 1)[:, :T * c.dim] for s in samples])).reshape(-1, T, c.dim)
  exact.assert_bits_equal(got, want, 'probe samples of the sequence output')
  flat = block.t[:, :T * c.dim]
  assert torch.equal(flat, dev(wt.values)[torch.from_numpy(cgrid).to(DEV)].view(B, T * c.dim)), 'a sample differs'
  flat.zero_()
  block.assert_rest_untouched((), 'the padding between samples')
  # backward + SGD of a second, small forward of the same object (the table's rows are what is far away here; the
  # [B, T, dim] gradient of 2^16 + 8 samples would cost a 0.5 GB float64 reference): 2048 samples, contiguous
  B = 2048
  lens = c.rng.randint(0, 7, size=B)
  splits = exact.splits_of(lens)
  r = c.p[c.rng.randint(0, c.p.size, size=int(splits[-1]))]
  seq([dev(r)], [dev(splits)])
  grid, _ = sequence_ref.grid_ref(r, splits, c.geom.rows, T, pad_row)
  cgrid = c.compact(grid)
  g = exact.exact_grads(c.rng, (B, T, c.dim), 4)       # at most 4 * 2048 terms in a row (13 bits) and 5 value bits
  res = SequenceLookupGrad(seq)([dev(g)], apply_lr=LR)[0]
  torch.cuda.synchronize()
  sums = exact.exact_dense((c.n, c.dim), cgrid, g.reshape(B * T, c.dim), case='sequence')
  k = int(res[2].item())
  got_u = host(res[0])[:k]
  order = np.argsort(got_u)
  np.testing.assert_array_equal(got_u[order], c.planted[sums.rows])
  exact.assert_bits_equal(host(res[1])[:k][order], sums.sums(), 'sequence gradient rows')
  want_t = exact.exact_sgd(wt.values, sums, LR, 'sequence')
  exact.assert_bits_equal(wt.rows(c.p), want_t[c.cp], 'sequence: stepped rows', rows=c.p)
  wt.assert_rest_untouched(c.probes, 'sequence SGD')


# ---- f. expand_rows and its gradient ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', [20, 256])
def test_expand_rows_and_gradient(width):
  """expand_rows / expand_rows_grad with 2^16 + 8 samples and keys, src_stride and out_stride 2^16 + 4 elements:
  the last keys' and samples' rows start past 2^32 floats.  Bit for bit expand_ref on the column blocks; the
  padding of every block stays zero.  HBM: two blocks of 16 GiB at a time (three allocated in all: 48 GiB)."""
  geom = wo.Geometry('expand', width, BLOCK_PITCH, BLOCK_ROWS)
  POOL.reserve(3, GiB)
  rng = np.random.RandomState(80 + width)
  n = BLOCK_ROWS
  probes, _ = wo.probe_rows(geom, 4)
  src, out, back = (POOL.take(geom, torch.float32) for _ in range(3))
  gen = torch.Generator(device=DEV)
  gen.manual_seed(width)
  # integers / 16 in [-1, 1]: a key's gradient sums at most 2^16 + 8 samples of 5 bits exactly
  src.table.copy_(torch.randint(-16, 17, (n, width), device=DEV, generator=gen).float() / 16)
  idx = rng.randint(0, n, size=n).astype(np.int64)
  idx[probes] = np.array(probes)[::-1]                # far samples read near keys and the reverse
  idx[5] = n                                          # outside: a zero row
  idx[7] = -1
  d_idx = dev(idx)
  expand_rows(d_idx, [src.table], outs=[out.table], n_keys=n)
  torch.cuda.synchronize()
  h_src = host(src.table)
  want = expand_ref.expand_ref(h_src, idx, n)
  exact.assert_bits_equal(host(out.table), want, f'expand_rows width {width}')
  index = ExpandIndex(d_idx, n).build()
  expand_rows_grad(index, [out.table], outs=[back.table])
  torch.cuda.synchronize()
  counts = np.bincount(idx[(idx >= 0) & (idx < n)], minlength=n).astype(np.float64)
  want_back = (h_src.astype(np.float64) * counts[:, None] + 0.0).astype(F32)   # (exact: see above; no -0.0)
  exact.assert_bits_equal(host(back.table), want_back, f'expand_rows_grad width {width}')
  at = np.array(probes)
  exact.assert_bits_equal(host(back.table)[at], expand_ref.grad_ref(want, idx, n)[at], 'probe keys against grad_ref')
  for blk, what in ((src, 'source'), (out, 'output'), (back, 'gradient')):
    blk.table.zero_()
    blk.assert_rest_untouched((), f'expand {what} block padding')


# ---- g. 16-bit tables ------------------------------------------------------------------------------------------------------------
LOWP_STEPS = [('sgd', 'nearest'), ('adagrad', 'nearest'), ('adam', 'nearest'), ('ftrl', 'nearest'),
              ('rowwise_adagrad', 'nearest'), ('sgd', 'stochastic'), ('adam', 'stochastic')]
SEED = 0x5EED1234


def _lowp_hyper(optimizer):
  return {'adam': {'powers': reference.ADAM_DEFAULTS[:2]}, 'ftrl': FTRL,
          'rowwise_adagrad': {'epsilon': ROWWISE_EPS}}.get(optimizer)


LOWP_CASES = [(g, d, o, r) for g in ('E', 'E100', 'R') for d in ('bf16', 'fp16') for o, r in LOWP_STEPS
              if r == 'nearest' or d == 'bf16']


@pytest.mark.parametrize('geom', ['E', 'E100', 'R'])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_lowp_forward(geom, dtype):
  """LowpGroupLookup's forward, one id per sample and ragged mean (int64 and int32 ids; on R un-bucketized int64
  ones), bit for bit lowp_ref.forward_rows on the compact copy.  HBM: one 16-bit table, 8 GiB."""
  c = Case(geom, dtype, seed=90)
  POOL.reserve(1, GiB)
  what = f'{geom} {dtype}'
  wt = c.table()
  for id_dtype in (np.int64,) if geom == 'R' else (np.int64, np.int32):
    ids, r = c.ids(id_dtype, unbucketized=geom == 'R')
    out = LowpGroupLookup([wt.table], buckets=[c.geom.rows], combiners='sum')([dev(ids)])[0]
    want = lowp_ref.forward_rows(wt.values, dtype, c.compact(r))
    exact.assert_bits_equal(host(out), want, f'{what} {np.dtype(id_dtype).name}: forward')
    splits = c.ragged(r.size)
    out = LowpGroupLookup([wt.table], buckets=[c.geom.rows], combiners='mean')([dev(ids)], [dev(splits)])[0]
    want = lowp_ref.forward_rows(wt.values, dtype, c.compact(r), splits, None, 'mean')
    exact.assert_bits_equal(host(out), want, f'{what} {np.dtype(id_dtype).name}: ragged mean')
  torch.cuda.synchronize()
  wt.assert_rest_untouched((), f'{what}: forward')


@pytest.mark.parametrize('geom,dtype,optimizer,rounding', LOWP_CASES, ids=['-'.join(x) for x in LOWP_CASES])
def test_lowp_step(geom, dtype, optimizer, rounding):
  """One step of each of the five optimizers with nearest rounding and, on bf16, of SGD and Adam with stochastic
  rounding, through LowpLookupGrad (the backward's emit, then LowpSparseApply): the stored bits against
  lowp_ref.apply_step on the compact copy, the noise keyed by the TABLE's row numbers -- on R the rows at and above
  2^32 carry a non-zero high word (noise_row).  The probes are those of the 16-bit table and of its fp32 slot
  arrays together.  HBM: the 16-bit table (8 GiB) and up to two fp32 slot arrays of its shape (32 GiB)."""
  c = Case(geom, dtype, seed=92 + len(optimizer), slots32=True)
  POOL.reserve(1 + SLOT_ARRAYS[optimizer], GiB)
  what = f'{geom} {dtype} {optimizer} {rounding}'
  wt = c.table()
  lookup = LowpGroupLookup([wt.table], buckets=[c.geom.rows], combiners='sum')
  slots, kw = _slot_arrays(c, optimizer)
  # (the fp16 cases of E and E100 take int32 ids, the others int64)
  ids, r, g = _exact_backward_inputs(c, geom == 'R', np.int32 if dtype == 'fp16' and geom != 'R' else np.int64)
  grad = LowpLookupGrad(lookup, rounding=rounding, seed=SEED, **kw)
  step_no = 0
  if rounding == 'stochastic':
    step_no = 0x80000001 if optimizer == 'adam' else 5
    grad.step_counter.fill_(step_no - (1 << 32) if step_no >= 1 << 31 else step_no)
  # (SGD to nearest: steps of several ulps, or dim-1 rows would mostly stay; stochastic: steps around one bf16 ulp)
  lr = 0.05 if optimizer != 'sgd' else 0.125 if rounding == 'nearest' else 2.0 ** -6
  res = grad([dev(ids)], [dev(g)], apply_lr=lr, optimizer=optimizer)[0]
  torch.cuda.synchronize()
  sums, _ = _check_emitted(c, res, r, g, 0, what)
  want_bits, want_slots = lowp_ref.apply_step(
    wt.values, dtype, [x.values for x in slots], sums.rows, sums.sums(), optimizer, lr, _lowp_hyper(optimizer),
    rounding, SEED, step_no, 0, vec4=c.dim % 4 == 0, noise_rows=c.planted[sums.rows])
  np.testing.assert_array_equal(wt.rows(c.p), want_bits[c.cp], err_msg=f'{what}: stored bits')
  assert (want_bits[c.cp] != wt.values[c.cp]).any(axis=1).sum() >= c.p.size // 2, 'the step moved too few rows'
  if rounding == 'stochastic':
    assert int(grad.step_counter.item()) & 0xFFFFFFFF == (step_no + 1) & 0xFFFFFFFF
  if geom == 'R':
    assert (c.p >= wo.M32).sum() >= 2           # rows at and above 2^32 are among those compared above
  wt.assert_rest_untouched(c.probes, f'{what}: table')
  for k, (x, w_slot) in enumerate(zip(slots, want_slots)):
    exact.assert_bits_equal(x.rows(c.p), w_slot[c.cp], f'{what}: slot {k} rows', rows=c.p)
    x.assert_rest_untouched(c.probes, f'{what}: slot {k}')


def high_word_case(c, seed):
  """Slices over R's probe rows whose SGD step (lr 2^-9) lands every row exactly on a bf16 tie -- the fp32 pattern's
  low half is 0x8000, so the stochastic rounding goes up on half of all noise words -- with the bf16 bits
  lowp_ref.apply_step stores under the noise of the 64-bit row number and under that of its low word alone.
  Returns (table bits [n, 1], rows, g, want, low_word); reference only, no device."""
  bits = lowp_ref.round_nearest(lowp_ref.bits32(grid_rows(c.rng, c.n, c.dim)), 'bf16')
  rows = c.p[c.rng.permutation(c.p.size)]
  w = lowp_ref.upcast(bits, 'bf16')[c.compact(rows)]
  _, e = np.frexp(w)                                  # |w| = m 2^e, m in [0.5, 1): half a bf16 ulp is 2^(e - 9)
  g = (-np.sign(w) * np.ldexp(1.0, e - 9) * 2.0 ** 9).astype(F32)
  args = (bits, 'bf16', [], c.compact(rows), g, 'sgd', 2.0 ** -9, None, 'stochastic', seed, 7, 0)
  want, _ = lowp_ref.apply_step(*args, noise_rows=rows)
  low_word, _ = lowp_ref.apply_step(*args, noise_rows=rows & 0xFFFFFFFF)
  return bits, rows, g, want, low_word


HIGH_WORD_SEEDS = 16


def test_lowp_apply_stochastic_on_rows_past_2_32():
  """LowpSparseApply alone on R with stochastic rounding, every stepped row on a tie: the stored bf16 bits equal
  lowp_ref.apply_step with the noise of the 64-bit row number -- which, for every row at and above 2^32, differ from
  those under the noise of the row's low word in at least one of the seeds, so the device reads the high word
  (noise_row).  HBM: one bf16 table, 8 GiB."""
  c = Case('R', 'bf16', seed=91)
  POOL.reserve(1, GiB)
  high = c.p >= wo.M32
  differs = np.zeros(c.p.size, bool)
  wt = POOL.take(c.geom, torch.bfloat16)
  for seed in range(HIGH_WORD_SEEDS):
    bits, rows, g, want, low_word = high_word_case(c, seed)
    assert ((lowp_ref.bits32(lowp_ref.upcast(bits, 'bf16')[c.compact(rows)] - F32(2.0 ** -9) * g) & 0xFFFF) == 0x8000).all()
    wt.plant(c.probes, c.aliases, bits)
    slices = (dev(rows), dev(g), torch.tensor([rows.size], dtype=torch.int32, device=DEV))
    app = LowpSparseApply([wt.table], rounding='stochastic', seed=seed)
    app.step_counter.fill_(7)
    app([slices], 2.0 ** -9, 'sgd')
    torch.cuda.synchronize()
    np.testing.assert_array_equal(wt.rows(c.p), want[c.cp], err_msg=f'seed {seed}')
    differs |= (want[c.cp] != low_word[c.cp]).any(axis=1)
    wt.assert_rest_untouched(c.probes, f'stochastic SGD seed {seed}')
  assert high.sum() >= 2 and differs[high].all() and not differs[~high].any()


# ---- h. sharded owner gather -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_sharded_owner_gather_one_shard(dtype):
  """ShardedGroupLookup / LowpShardedGroupLookup over Collective.local_world(1) with one E shard: forward, backward and
  the SGD step against the unsharded reference on the compact copy.  HBM: one shard, 16 GiB (bf16: 8)."""
  c = Case('E', dtype, seed=100)
  POOL.reserve(1, 2 * GiB)
  wt = c.table()
  comms = hb.distribute.Collective.local_world(1)
  try:
    if dtype == 'fp32':
      drv = ShardedGroupLookup([wt.table], comms[0], buckets=[c.geom.rows], combiners='sum')
    else:
      drv = LowpShardedGroupLookup([wt.table], comms[0], buckets=[c.geom.rows], combiners='sum')
    ids, r, g = _exact_backward_inputs(c, True)
    out = drv([dev(ids)])[0]
    torch.cuda.synchronize()
    if dtype == 'fp32':
      want = oracle.group_lookup_fwd([wt.values], [c.compact(r)], [None], None, ['sum'])[0]
    else:
      want = lowp_ref.forward_rows(wt.values, dtype, c.compact(r))
    exact.assert_bits_equal(host(out), want, f'sharded {dtype}: forward')
    lr = LR if dtype == 'fp32' else 2.0 ** -9
    res = drv.backward([dev(g)], apply_lr=lr)[0]
    torch.cuda.current_stream().synchronize()
    torch.cuda.synchronize()
    sums, _ = _check_emitted(c, res, r, g, 0, f'sharded {dtype}')
    if dtype == 'fp32':
      want_t = exact.exact_sgd(wt.values, sums, lr, 'sharded')
      exact.assert_bits_equal(wt.rows(c.p), want_t[c.cp], 'sharded: stepped rows', rows=c.p)
    else:
      want_bits, _ = lowp_ref.apply_step(wt.values, dtype, [], sums.rows, sums.sums(), 'sgd', lr)
      np.testing.assert_array_equal(wt.rows(c.p), want_bits[c.cp], err_msg='sharded bf16: stored bits')
    wt.assert_rest_untouched(c.probes, f'sharded {dtype}')
    drv.close()
  finally:
    for cm in comms:
      cm.close()


# ---- i. hash tables --------------------------------------------------------------------------------------------------------
HASH_SEED, HASH_SCALE = 3, 1e-3
_HASH_KEYS = {}


def slab_probes(capacity, dim=HASH_DIM, slab=HASH_SLAB):
  """(probe slabs, alias slabs) of a value array [capacity, dim]: probe_rows of the array seen as rows of one slab
  each, so the slots slab * 8 .. + 7 of the probe slabs sit on both sides of every threshold and no alias slab is a
  probe slab."""
  return wo.probe_rows(wo.Geometry('slabs', slab * dim, slab * dim, capacity // slab), 4)


def keys_with_home_slabs(slab_count, slabs, per_slab=2, allowed=None):
  """int64 keys, `per_slab` for every slab of `slabs`, whose home slab murmur3(key) % slab_count is that slab: found
  on the host with hash_ref.murmur3_np over a fixed sequence of candidates (the same keys on every run).  allowed:
  allowed(key, hash) says whether a candidate with the right home slab may be taken.  Returns {slab: [keys]}."""
  key = (slab_count, tuple(slabs), per_slab, allowed is not None)
  if key in _HASH_KEYS and allowed is None:
    return _HASH_KEYS[key]
  from tests.support import hash_ref
  want = np.zeros(slab_count, bool)
  want[list(slabs)] = True
  found = {int(s): [] for s in slabs}
  chunk = 1 << 21
  for c in range(64):
    cand = np.arange(1 + c * chunk, 1 + (c + 1) * chunk, dtype=np.int64) * np.int64(0x1E3779B97F4A7C15)
    h = hash_ref.murmur3_np(cand)
    home = h.astype(np.int64) % slab_count
    hit = want[home]
    for k, s, hk in zip(cand[hit].tolist(), home[hit].tolist(), h[hit].tolist()):
      if len(found[s]) < per_slab and (allowed is None or allowed(k, hk)):
        found[s].append(k)
    if all(len(v) == per_slab for v in found.values()):
      break
  else:
    raise AssertionError('no keys found for some slab')
  if allowed is None:
    _HASH_KEYS[key] = found
  return found


class HashCase:
  """An expiring HashTable(capacity 2^24 + 2^20, dim 256, slab_size 8) whose keys have their home slabs on both sides
  of every threshold of the value array, two per slab (no slab overflows: a key's slot is one of the first two of its
  home slab), the value array and an optional companion array looked after by a WideTable each: random rows planted
  at every slot of the alias slabs, and -- to be overwritten by the insert -- at the slots the keys will take."""

  def __init__(self, seed, comp_dim=None, capacity=HASH_CAP, new_capacity=None, table_seed=HASH_SEED):
    from tests.support import hash_ref
    self.hash_ref = hash_ref
    self.rng = np.random.RandomState(seed)
    self.ht = hb.embedding.HashTable(capacity, HASH_DIM, DEV, slab_size=HASH_SLAB, init_scale=HASH_SCALE,
                                     seed=table_seed, expiring=True)
    sc = self.ht.slab_count
    self.probe_slabs, self.alias_slabs = slab_probes(capacity)
    by_slab = keys_with_home_slabs(sc, self.probe_slabs)
    keys = [k for s in self.probe_slabs for k in by_slab[s]]
    slots = [s * HASH_SLAB + j for s in self.probe_slabs for j in range(len(by_slab[s]))]
    self.new_probe_keys = []
    if new_capacity is not None:
      # keys for the probe slabs of the table a rehash makes; here each takes the first slot of a slab of its own
      # that is neither a probe nor an alias slab
      sc2 = new_capacity // HASH_SLAB
      taken = np.zeros(sc, bool)
      taken[self.probe_slabs + self.alias_slabs] = True
      def allowed(k, h):                           # (one key per old slab)
        old = h % sc
        if taken[old]:
          return False
        taken[old] = True
        return True
      more = keys_with_home_slabs(sc2, slab_probes(new_capacity)[0], 2, allowed)
      for ks in more.values():
        for k in ks:
          keys.append(k)
          slots.append(int(hash_ref.murmur3_np(np.array([k]))[0]) % sc * HASH_SLAB)
          self.new_probe_keys.append(k)
    self.keys = np.array(keys, np.int64)
    self.home = hash_ref.murmur3_np(self.keys).astype(np.int64) % sc
    self.probe_slots = sorted(slots)
    self.alias_slots = [s * HASH_SLAB + j for s in self.alias_slabs for j in range(HASH_SLAB)]
    assert len(set(self.probe_slots)) == self.keys.size and not set(self.probe_slots) & set(self.alias_slots)
    n = len(self.probe_slots) + len(self.alias_slots)
    geom = wo.Geometry('hash', HASH_DIM, HASH_DIM, self.ht.capacity)
    self.wt = wo.WideTable(geom, torch.float32, DEV, over=self.ht.table).plant(
      self.probe_slots, self.alias_slots, self.rng.uniform(1, 2, size=(n, HASH_DIM)).astype(F32))
    self.comp = None
    if comp_dim:
      cg = wo.Geometry('companion', comp_dim, comp_dim, self.ht.capacity)
      # (a companion as wide as the rows is a slab of the pool; a narrow one is counted with the table's own arrays)
      comp = POOL.take(cg, torch.float32) if comp_dim == HASH_DIM else wo.WideTable(cg, torch.float32, DEV)
      self.comp = comp.plant(
        self.probe_slots, self.alias_slots, self.rng.uniform(1, 2, size=(n, comp_dim)).astype(F32))

  def insert(self, keys=None):
    """Insert the keys: the slots against the placement rule, the initial rows against hash_ref.init_rows, the rest
    of the value array untouched.  Returns the slots (host)."""
    keys = self.keys if keys is None else keys
    slots = host(self.ht.lookup_or_insert(dev(keys)))
    home = self.hash_ref.murmur3_np(keys).astype(np.int64) % self.ht.slab_count
    np.testing.assert_array_equal(slots // HASH_SLAB, home, err_msg='a key outside its home slab')
    assert set(slots.tolist()) <= set(self.probe_slots) and np.unique(slots).size == slots.size
    want = self.hash_ref.init_rows(keys, HASH_DIM, self.ht.seed, HASH_SCALE)
    exact.assert_bits_equal(self.wt.rows(slots), want, 'the initial rows', rows=slots)
    self.wt.assert_rest_untouched(slots, 'insert', keep=True)
    return slots

  def slots_by_key(self):
    slots = host(self.ht.find(dev(self.keys)))
    assert (slots >= 0).all()
    return slots


def _view(wt):
  """What _check_emitted reads of a Case, for a WideTable."""
  import types
  return types.SimpleNamespace(n=wt.planted.size, dim=wt.geom.dim, compact=wt.compact_of, planted=wt.planted)


def test_hash_insert_lookup_backward_step():
  """insert: the initial row at the slot equals hash_ref.init_rows; HashGroupLookup's forward, backward and SGD step
  equal the fp32 path on table[slots] (the oracle on the compact copy).  HBM: the value array, 17 GiB."""
  POOL.reserve(0, HASH_CAP * HASH_DIM * 4 + 2 * GiB)
  hc = HashCase(110)
  slots = hc.insert()
  at = {int(k): int(s) for k, s in zip(hc.keys, slots)}
  reps = hc.rng.randint(1, 4, size=hc.keys.size)
  ids = np.repeat(hc.keys, reps)
  hc.rng.shuffle(ids)
  r = np.array([at[int(k)] for k in ids], np.int64)
  hgl = hb.embedding.HashGroupLookup([hc.ht], combiners='sum')
  out = hgl([dev(ids)])[0]
  torch.cuda.synchronize()
  np.testing.assert_array_equal(host(hgl.slots[0]), r)
  assert hc.ht.size() == hc.keys.size
  want = oracle.group_lookup_fwd([hc.wt.values], [hc.wt.compact_of(r)], [None], None, ['sum'])[0]
  exact.assert_bits_equal(host(out), want, 'hash forward')
  g = exact.exact_grads(hc.rng, (ids.size, HASH_DIM), 6)
  res = GroupLookupGrad(hgl.lookup)(hgl.slots, [dev(g)], apply_lr=LR)[0]
  torch.cuda.synchronize()
  sums, _ = _check_emitted(_view(hc.wt), res, r, g, 0, 'hash backward')
  want_t = hc.wt.values.copy()
  oracle.sparse_sgd_apply(want_t, sums.rows, sums.sums(), LR)
  exact.assert_bits_equal(hc.wt.rows(slots), want_t[hc.wt.compact_of(slots)], 'hash SGD rows', rows=slots)
  hc.wt.assert_rest_untouched(slots, 'hash SGD')


def test_hash_remove():
  """hash_remove: the fill value lands at the slots the removed keys held, in a companion array of the value array's
  shape, and only there; the value array is left alone.  HBM: value array and companion, 34 GiB."""
  POOL.reserve(1, HASH_CAP * HASH_DIM * 4 + 2 * GiB)
  hc = HashCase(111, comp_dim=HASH_DIM)
  slots = hc.insert()
  gone = np.arange(hc.keys.size) % 2 == 0             # every other key: both sides of every threshold
  ids = np.concatenate([hc.keys[gone], hc.keys[gone][:3], [12345678901]]).astype(np.int64)
  old = host(hc.ht.remove(dev(ids), slots=[(hc.comp.table, 0.5)]))
  np.testing.assert_array_equal(old[:gone.sum()], slots[gone])
  assert old[-1] == -1
  after = host(hc.ht.find(dev(hc.keys)))
  np.testing.assert_array_equal(after, np.where(gone, -1, slots))
  got = hc.comp.rows(slots[gone])
  exact.assert_bits_equal(got, np.full_like(got, 0.5), 'the fill value at the removed slots', rows=slots[gone])
  hc.comp.assert_rest_untouched(slots[gone], 'remove: companion')
  hc.wt.assert_rest_untouched((), 'remove: value array')


def test_hash_export_import():
  """hash_export of the table (keys far and near, ascending slot order) with one companion array, and the import
  into a fresh table of the same capacity.  HBM: two value arrays and two companions of 64 floats, 43 GiB."""
  POOL.reserve(0, 2 * HASH_CAP * (HASH_DIM + 64) * 4 + 2 * GiB)
  hc = HashCase(112, comp_dim=64)
  slots = hc.insert()
  exp = hb.embedding.hash_export([hc.ht], slots=[[hc.comp.table]])[0]
  order = np.argsort(slots)
  np.testing.assert_array_equal(host(exp.src_slots), slots[order])
  np.testing.assert_array_equal(host(exp.keys), hc.keys[order])
  exact.assert_bits_equal(host(exp.rows), hc.wt.rows(slots[order]), 'exported rows')
  exact.assert_bits_equal(host(exp.slots[0]), hc.comp.rows(slots[order]), 'exported companion rows')
  hc.wt.assert_rest_untouched((), 'export: value array', keep=True)
  hc.comp.assert_rest_untouched((), 'export: companion', keep=True)
  into = HashCase(113, comp_dim=64, table_seed=HASH_SEED + 1)
  got = host(into.ht.import_items(exp, slots=[into.comp.table]))
  np.testing.assert_array_equal(got // HASH_SLAB, hc.home[order])
  assert set(got.tolist()) == set(into.probe_slots)
  exact.assert_bits_equal(into.wt.rows(got), host(exp.rows), 'imported rows', rows=got)
  exact.assert_bits_equal(into.comp.rows(got), host(exp.slots[0]), 'imported companion rows', rows=got)
  into.wt.assert_rest_untouched(got, 'import: value array')
  into.comp.assert_rest_untouched(got, 'import: companion')


def test_hash_rehash():
  """hash_rehash into capacity 2^24 + 2^21: the keys' rows and companion rows move to their new home slabs -- the
  keys include two for every probe slab of the NEW value array -- and nothing else of the new arrays is written; the
  old arrays are only read.  HBM: old and new value array and companions of 64 floats, 45 GiB."""
  POOL.reserve(0, (HASH_CAP + HASH_CAP2) * (HASH_DIM + 64) * 4 + 2 * GiB)
  hc = HashCase(114, comp_dim=64, new_capacity=HASH_CAP2)
  assert len(hc.new_probe_keys) >= 24
  slots = hc.insert()
  rows, comp_rows = hc.wt.rows(slots), hc.comp.rows(slots)
  new_comp = hc.ht.rehash(capacity=HASH_CAP2, slots=[(hc.comp.table, 0.0)])[0]
  assert hc.ht.capacity == HASH_CAP2 // HASH_SLAB * HASH_SLAB and tuple(new_comp.shape) == (hc.ht.capacity, 64)
  new = hc.slots_by_key()
  np.testing.assert_array_equal(new // HASH_SLAB, hc.hash_ref.murmur3_np(hc.keys).astype(np.int64) % hc.ht.slab_count)
  assert np.unique(new).size == new.size
  far = set((np.array(slab_probes(HASH_CAP2)[0]) * HASH_SLAB).tolist())
  assert len(far & set((new // HASH_SLAB * HASH_SLAB).tolist())) == len(far), 'a probe slab of the new array without a key'
  geom = wo.Geometry('rehashed', HASH_DIM, HASH_DIM, hc.ht.capacity)
  wo.WideTable(geom, torch.float32, DEV, over=hc.ht.table).adopt(new, rows).assert_rest_untouched((), 'rehash: new value array')
  cg = wo.Geometry('rehashed companion', 64, 64, hc.ht.capacity)
  wo.WideTable(cg, torch.float32, DEV, over=new_comp).adopt(new, comp_rows).assert_rest_untouched((), 'rehash: new companion')
  hc.wt.assert_rest_untouched((), 'rehash: old value array')
  hc.comp.assert_rest_untouched((), 'rehash: old companion')


def test_hash_spill_and_fault_in():
  """hash_spill of a handful of far keys (the oldest) into a HashSpillStore, and hash_fault_in of them: rows and
  companion rows leave and come back as they were, the companion rows are reset in between, nothing else is
  written.  HBM: value array and a companion of 64 floats, 22 GiB."""
  POOL.reserve(0, HASH_CAP * (HASH_DIM + 64) * 4 + 2 * GiB)
  hc = HashCase(115, comp_dim=64)
  top = sorted(hc.probe_slabs)[-6:]                    # the slabs around row 2^24 and the last one
  far = np.isin(hc.home, top)
  assert 6 <= far.sum() <= 12
  hc.ht.set_step(1)
  s_far = hc.insert(hc.keys[far])
  hc.ht.set_step(5)
  s_near = hc.insert(hc.keys[~far])
  rows, comp_rows = hc.wt.rows(s_far), hc.comp.rows(s_far)
  store = hb.embedding.HashSpillStore(HASH_DIM, [64])
  exp = hc.ht.spill_to(int((~far).sum()), store=store, slots=[(hc.comp.table, 0.0)])
  order = np.argsort(s_far)
  np.testing.assert_array_equal(host(exp.keys), hc.keys[far][order])
  np.testing.assert_array_equal(host(exp.src_slots), s_far[order])
  exact.assert_bits_equal(host(exp.rows), rows[order], 'spilled rows')
  exact.assert_bits_equal(host(exp.slots[0]), comp_rows[order], 'spilled companion rows')
  assert len(store) == far.sum() and (host(hc.ht.find(dev(hc.keys[far]))) == -1).all()
  np.testing.assert_array_equal(host(hc.ht.find(dev(hc.keys[~far]))), s_near)
  assert not hc.comp.rows(s_far).any(), 'the companion rows of the spilled keys are reset'
  hc.comp.assert_rest_untouched(s_far, 'spill: companion', keep=True)
  hc.wt.assert_rest_untouched((), 'spill: value array', keep=True)
  ids = np.concatenate([hc.keys[far], hc.keys[far][:2], hc.keys[~far][:2]])
  assert hb.embedding.hash_fault_in([hc.ht], [dev(ids)], [store], slots=[[hc.comp.table]]) == [int(far.sum())]
  back = host(hc.ht.find(dev(hc.keys[far])))
  assert set(back.tolist()) == set(s_far.tolist()) and len(store) == 0       # (the tombstones are reused)
  exact.assert_bits_equal(hc.wt.rows(back), rows, 'rows after the fault-in', rows=back)
  exact.assert_bits_equal(hc.comp.rows(back), comp_rows, 'companion rows after the fault-in', rows=back)
  hc.wt.assert_rest_untouched(back, 'fault-in: value array')
  hc.comp.assert_rest_untouched(back, 'fault-in: companion')


# a table of dim 20 whose value array has geometry P's pitch: the entries that take Move / Fill pitches directly
P_SLABS_FULL, P_SLABS_TWO = (63, 127, 255, 511), (0, 64, 128, 256, 512, 524)


def test_hash_value_array_with_a_pitch():
  """A HashTable(capacity 4200, dim 20) whose rows live in a [4200, 2^20 + 4] array (row 4096 starts past 2^32
  floats): the insert's table_pitch, hash_remove's Fill pitch, the Move pitches of export (source), import
  (destination), rehash and spill (source) and of the fault-in (destination).  The slabs below a threshold are full,
  so the slots just under 2^29, 2^30, 2^31 and 2^32 floats are taken.  HBM: two pitched arrays, 33 GiB."""
  from tests.support import hash_ref
  geom = wo.GEOMETRIES['P']
  POOL.reserve(2, GiB)
  rng = np.random.RandomState(116)
  wide = POOL.take(geom, torch.float32)

  class Pitched(hb.embedding.HashTable):
    """The value array of the insert is `wide` (hbk_hash_column_t.table_pitch); .table stays a stand-in."""

    def _describe(self, col, init=True, count=True):
      super()._describe(col, init, count)
      if init:
        col.table, col.table_pitch = wide.t.data_ptr(), geom.pitch

  ht = Pitched(geom.rows, geom.dim, DEV, slab_size=HASH_SLAB, init_scale=HASH_SCALE, seed=HASH_SEED, expiring=True)
  sc = ht.slab_count
  assert sc == 525
  by_slab = dict(keys_with_home_slabs(sc, P_SLABS_FULL, HASH_SLAB))
  by_slab.update(keys_with_home_slabs(sc, P_SLABS_TWO, 2))
  keys = np.array([k for s in sorted(by_slab) for k in by_slab[s]], np.int64)
  probe_slots = sorted(s * HASH_SLAB + j for s in by_slab for j in range(len(by_slab[s])))
  assert {511, 1023, 2047, 4095, 4096} <= set(probe_slots)
  aliases = sorted({a for r in probe_slots for a in wo.alias_rows_of(geom, 4, r)} - set(probe_slots))
  n = len(probe_slots) + len(aliases)
  wide.plant(probe_slots, aliases, rng.uniform(1, 2, size=(n, geom.dim)).astype(F32))
  view = wide.table                                   # [4200, 20] with a row stride of 2^20 + 4
  # insert
  slots = host(ht.lookup_or_insert(dev(keys)))
  np.testing.assert_array_equal(slots // HASH_SLAB, hash_ref.murmur3_np(keys).astype(np.int64) % sc)
  assert sorted(slots.tolist()) == probe_slots
  exact.assert_bits_equal(wide.rows(slots), hash_ref.init_rows(keys, geom.dim, HASH_SEED, HASH_SCALE), 'initial rows',
                          rows=slots)
  assert not ht.table.any()
  wide.assert_rest_untouched(slots, 'pitched insert', keep=True)
  # export (Move.src_pitch)
  order = np.argsort(slots)
  exp = hb.embedding.hash_export([ht], slots=[[view]])[0]
  np.testing.assert_array_equal(host(exp.src_slots), slots[order])
  exact.assert_bits_equal(host(exp.slots[0]), wide.rows(slots[order]), 'exported rows of the pitched array')
  # import into a second table with a second pitched array (Move.dst_pitch)
  wide2 = POOL.take(geom, torch.float32).plant(probe_slots, aliases, rng.uniform(1, 2, size=(n, geom.dim)).astype(F32))
  ht2 = hb.embedding.HashTable(geom.rows, geom.dim, DEV, slab_size=HASH_SLAB, expiring=True)
  got = host(ht2.import_items(exp, slots=[wide2.table]))
  assert sorted(got.tolist()) == probe_slots
  exact.assert_bits_equal(wide2.rows(got), host(exp.slots[0]), 'imported rows of the pitched array', rows=got)
  wide2.assert_rest_untouched(got, 'pitched import')
  del wide2, ht2
  # rehash to the same capacity (Move.src_pitch; the new companion is contiguous)
  before = wide.rows(slots)
  new_comp = ht.rehash(slots=[(view, 0.0)])[0]
  new = host(ht.find(dev(keys)))
  assert sorted(new.tolist()) == probe_slots
  exact.assert_bits_equal(host(new_comp)[new], before, 'rehashed rows')
  assert int(new_comp.count_nonzero().item()) == int(np.count_nonzero(before))
  wide.assert_rest_untouched((), 'pitched rehash: the source', keep=True)
  # the array keeps the rows at the slots of the FIRST placement: put them where the keys are now
  wide.write_rows(new, before)
  wide.refresh(probe_slots)
  # remove (Fill.pitch)
  gone = np.arange(keys.size) % 3 == 0
  old = host(ht.remove(dev(keys[gone]), slots=[(view, 0.5)]))
  np.testing.assert_array_equal(old, new[gone])
  filled = wide.rows(old)
  exact.assert_bits_equal(filled, np.full_like(filled, 0.5), 'the fill value in the pitched array', rows=old)
  wide.assert_rest_untouched(old, 'pitched remove', keep=True)
  # spill (Move.src_pitch and Fill.pitch) and fault-in (Move.dst_pitch) of the keys that stayed in the far slabs
  stay = ~gone
  far = stay & (new >= 4088)
  assert far.sum() >= 4
  ht.set_step(9)
  ht.lookup_or_insert(dev(keys[stay & ~far]))         # (seen now: the far keys are the oldest)
  rows = wide.rows(new[far])
  store = hb.embedding.HashSpillStore(geom.dim, [geom.dim])
  exp = ht.spill_to(int((stay & ~far).sum()), store=store, slots=[(view, 0.0)])
  np.testing.assert_array_equal(host(exp.keys), keys[far][np.argsort(new[far])])
  exact.assert_bits_equal(host(exp.slots[0]), rows[np.argsort(new[far])], 'spilled rows')
  assert not wide.rows(new[far]).any()
  wide.assert_rest_untouched(new[far], 'pitched spill', keep=True)
  assert ht.fault_in(dev(keys[far]), store, slots=[view]) == int(far.sum())
  back = host(ht.find(dev(keys[far])))
  # (a key comes back into the first free slot of its home slab: that of a removed key, or one of those spilled)
  np.testing.assert_array_equal(back // HASH_SLAB, new[far] // HASH_SLAB)
  assert np.unique(back).size == back.size and set(back.tolist()) <= set(probe_slots)
  exact.assert_bits_equal(wide.rows(back), rows, 'rows of the pitched array after the fault-in', rows=back)
  wide.assert_rest_untouched(back, 'pitched fault-in')
