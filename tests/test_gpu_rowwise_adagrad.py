"""Row-wise Adagrad on the GPU against tests/support/rowwise_adagrad_ref.py, the numpy fp32 restatement of
include/hbk.h's formula in its documented chunk and butterfly order: bit for bit on the exact grid under the
default reduce plans and on N(0,1) gradients under the deterministic ones, each distinct row stepped once
across two apply launches, through max_norm, launch() and a captured graph, sequence lookups, the sharded
step, hash tables and the feature-column layers with their checkpoints."""
import math
import threading

import numpy as np
import pytest
import torch

import oracle
import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (GroupLookup, GroupLookupGrad, RowwiseAdagrad, SequenceLookup,
                                         SequenceLookupGrad)
from hybridbackend_amd.embedding.sharded import ShardedGroupLookup
from tests.support import exact
from tests.support import rowwise_adagrad_ref as ref
from tests.support.tolerance import assert_sums_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
LR, EPS, A0 = 0.05, 1e-8, 0.1


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def dev_table(w, offset=False):
  """w on the device; offset: a contiguous view that starts 4 bytes past a 16-byte boundary (the scalar path
  for every dim)."""
  if not offset:
    return dev(w)
  flat = torch.zeros(w.size + 8, dtype=torch.float32, device=DEV)
  view = flat[1:1 + w.size].view(*w.shape)
  view.copy_(torch.from_numpy(w))
  assert view.data_ptr() % 16 == 4 and view.is_contiguous()
  return view


def emitted(res):
  u, g, k = res
  k = int(k.item())
  return host(u)[:k], host(g)[:k]


def dedup_in_order(rows, terms, n_rows):
  """The deterministic mode's sums: every row's fp32 terms added in id order.  Returns (distinct rows
  ascending, fp32 sums) of the rows inside the table."""
  rows = np.asarray(rows, np.int64)
  ok = (rows >= 0) & (rows < n_rows)
  uniq = np.unique(rows[ok])
  sums = oracle.unsorted_segment_sum(np.ascontiguousarray(terms[ok]),
                                     np.searchsorted(uniq, rows[ok]).astype(np.int32), uniq.size)
  return uniq, sums


# ---- 1. the exact grid under the default reduce plans ---------------------------------------------------
def value_budget(dim):
  """b of the issue: 2 b + ceil(log2 dim) <= 24."""
  return (exact.MANTISSA - int(math.ceil(math.log2(dim))) if dim > 1 else exact.MANTISSA) // 2


class ExactColumn:
  """One column on the exact grid: the deduplicated gradient of every row is a multiple of q below 2^b q, so
  s = sum g^2 is exact in ANY order -- asserted here, on the reference alone."""

  def __init__(self, name, dim, rows, ids, vec4, seed, comb='sum', splits=None):
    rng = np.random.RandomState(seed)
    self.name, self.dim, self.rows, self.comb, self.vec4 = name, dim, rows, comb, vec4
    self.ids = np.asarray(ids, np.int64)
    self.splits = None if splits is None else np.asarray(splits, np.int32)
    n_seg = self.ids.size if self.splits is None else self.splits.size - 1
    valid = (self.ids >= 0) & (self.ids < rows)
    b = value_budget(dim)
    count = int(np.unique(self.ids[valid], return_counts=True)[1].max(initial=1))
    count_bits = int(math.ceil(math.log2(count))) if count > 1 else 0
    longest = 1 if self.splits is None else int(np.diff(self.splits).max(initial=1))
    value_bits = b - count_bits - exact.factor_bits(comb, longest) - 1     # (-1: the range is closed)
    assert value_bits >= 1, f'{name}: {count} terms in a row leave {value_bits} value bits of {b}: shrink the case'
    self.grads = exact.exact_grads(rng, (n_seg, dim), value_bits, frac_bits=2)
    self.table = exact.exact_tables(rng, rows, dim)
    self.accum = rng.uniform(0.0, 2.0, size=(rows, 1)).astype(F32)
    terms = exact.id_terms(self.grads, self.splits, comb)
    self.want = exact.exact_dense((rows, dim), self.ids[valid], terms[valid], case=name)
    g = self.want.sums()
    # the budget, on the reference: |g| / q < 2^b and 2 b + ceil(log2 dim) <= 24, so s is exact
    assert 2 * b + (int(math.ceil(math.log2(dim))) if dim > 1 else 0) <= exact.MANTISSA
    assert np.abs(g.astype(np.float64) / self.want.q).max(initial=0.0) < 2.0 ** b, f'{name}: |g| / q reaches 2^{b}'
    s64 = (g.astype(np.float64) ** 2).sum(axis=1)
    for order in {False, dim % 4 == 0}:      # exact in either chunking, so in any order
      assert (ref.row_sum_sq(g, order).astype(np.float64) == s64).all(), f'{name}: s is not exact'
    self.w1, self.a1 = self.table.copy(), self.accum.copy()
    ref.step(self.w1, self.a1, self.want.rows, g, LR, EPS, vec4)


def exact_columns(dim, vec4):
  rng = np.random.RandomState(1000 + dim + vec4)
  lanes = 1 << max(0, int(math.ceil(math.log2(dim // 4 if vec4 else dim))))
  per_task = (64 // lanes) * 4
  n_odd = 3 * per_task + max(1, per_task // 2) + 1           # no multiple of (64 >> lpr_log2) * 4
  assert n_odd % per_task != 0
  rows = max(2 * n_odd, 64)
  hot = min(300, 1 << (value_budget(dim) - 2))             # (the budget bounds the duplicates: dim 256 -> 64)
  some = rng.permutation(rows)[:n_odd]
  cols = [
    ExactColumn('none', dim, 50, np.array([-1, 50, 77, -1], np.int64), vec4, 1),            # n_unique 0
    ExactColumn('one_hot', dim, 50, np.full(hot, 7, np.int64), vec4, 2),                    # n_unique 1
    ExactColumn('odd', dim, rows, np.concatenate([some, some[:5], [-1, rows, rows + 9]]), vec4, 3),
  ]
  assert cols[0].want.rows.size == 0 and cols[1].want.rows.size == 1 and cols[2].want.rows.size == n_odd
  sp = exact.exact_ragged(rng, 40, 'mean', 4)
  cols.append(ExactColumn('ragged_mean', dim, 97, rng.randint(-3, 100, size=int(sp[-1])), vec4, 4, 'mean', sp))
  return cols


@pytest.mark.parametrize('dim, vec4', [(1, False), (3, False), (4, False), (16, False), (20, False), (64, False),
                                       (64, True), (256, True)])
@pytest.mark.parametrize('emit', [True, False])
def test_exact_grid_default_plans_bit_for_bit(dim, vec4, emit):
  cols = exact_columns(dim, vec4)
  offset = not vec4 and dim % 4 == 0                   # dims 4, 16, 20, 64 reach the scalar path by their address
  tables = [dev_table(c.table, offset) for c in cols]
  accs = [dev(c.accum) for c in cols]
  lookup = GroupLookup(tables, combiners=[c.comb for c in cols])
  grad = GroupLookupGrad(lookup, row_accums=accs, rowwise_adagrad=RowwiseAdagrad(epsilon=EPS))
  res = grad([dev(c.ids) for c in cols], [dev(c.grads) for c in cols],
             [None if c.splits is None else dev(c.splits) for c in cols], apply_lr=LR,
             optimizer='rowwise_adagrad', emit=emit)
  torch.cuda.synchronize()
  for k, c in enumerate(cols):
    assert int(res[k][2].item()) == c.want.rows.size, c.name
    if emit:
      u, g = emitted(res[k])
      order = np.argsort(u)
      np.testing.assert_array_equal(u[order], c.want.rows, err_msg=c.name)
      exact.assert_bits_equal(g[order], c.want.sums(), c.name + ': deduplicated gradient')
    exact.assert_bits_equal(host(tables[k]), c.w1, f'{c.name}: weights')
    exact.assert_bits_equal(host(accs[k]), c.a1, f'{c.name}: accumulator')


# ---- 2. N(0,1) gradients, deterministic ------------------------------------------------------------------
def test_random_gradients_deterministic_steps_and_step_only():
  rng = np.random.RandomState(21)
  rows, dims, offsets, steps = [2003, 301, 499], [16, 5, 64], [False, False, True], 3
  n = len(rows)
  w0 = [rng.uniform(-1, 1, size=(rows[c], dims[c])).astype(F32) for c in range(n)]
  a0 = [rng.uniform(0, 0.5, size=(rows[c], 1)).astype(F32) for c in range(n)]
  runs = []
  for emit in (True, False):
    tables = [dev_table(w0[c], offsets[c]) for c in range(n)]
    accs = [dev(a) for a in a0]
    grad = GroupLookupGrad(GroupLookup(tables), row_accums=accs, deterministic=True)
    runs.append((tables, accs, grad, emit))
  w, a = [x.copy() for x in w0], [x.copy() for x in a0]
  touched = [np.zeros(r, bool) for r in rows]
  for s in range(steps):
    srng = np.random.RandomState(100 + s)
    ids = [((srng.zipf(1.3, size=1500) * 7) % rows[c] - (srng.rand(1500) < 0.02)).astype(np.int64)
           for c in range(n)]
    gs = [srng.randn(1500, dims[c]).astype(F32) for c in range(n)]
    for tables, accs, grad, emit in runs:
      grad([dev(i) for i in ids], [dev(g) for g in gs], apply_lr=LR, optimizer='rowwise_adagrad', emit=emit)
    for c in range(n):
      u, sums = dedup_in_order(ids[c], gs[c], rows[c])
      touched[c][u] = True
      ref.step(w[c], a[c], u, sums, LR, EPS, ref.is_vec4(dims[c], not offsets[c]))
  torch.cuda.synchronize()
  for tables, accs, _, emit in runs:
    for c in range(n):
      exact.assert_bits_equal(host(tables[c]), w[c], f'w {c} emit={emit}')
      exact.assert_bits_equal(host(accs[c]), a[c], f'a {c} emit={emit}')
  for c in range(n):   # rows that never occurred keep their bits (the reference copied them)
    assert not touched[c].all()
    exact.assert_bits_equal(w[c][~touched[c]], w0[c][~touched[c]])
    exact.assert_bits_equal(a[c][~touched[c]], a0[c][~touched[c]])


# ---- 3. each distinct row once, two apply launches --------------------------------------------------------
def test_each_row_stepped_exactly_once_across_two_apply_launches():
  rng = np.random.RandomState(3)
  n, rows = 65, 61
  dims = [(4, 3, 16, 1)[c % 4] for c in range(n)]
  w0 = [rng.uniform(-1, 1, size=(rows, d)).astype(F32) for d in dims]
  a0 = [rng.uniform(0, 0.5, size=(rows, 1)).astype(F32) for _ in dims]
  ids = [rng.randint(0, rows, size=int(rng.randint(1, 90))).astype(np.int64) for _ in dims]
  gs = [rng.randn(i.size, d).astype(F32) for i, d in zip(ids, dims)]
  tables, accs = [dev(x) for x in w0], [dev(x) for x in a0]
  grad = GroupLookupGrad(GroupLookup(tables), row_accums=accs, deterministic=True)
  res = grad([dev(i) for i in ids], [dev(g) for g in gs], apply_lr=LR, optimizer='rowwise_adagrad')
  torch.cuda.synchronize()
  for c in range(n):
    u, g = emitted(res[c])
    want_u, sums = dedup_in_order(ids[c], gs[c], rows)
    assert np.unique(u).size == u.size, f'column {c}: a row emitted twice'
    np.testing.assert_array_equal(u, want_u)
    exact.assert_bits_equal(g, sums, f'gradient of column {c}')
    w, a = w0[c].copy(), a0[c].copy()
    ref.step(w, a, want_u, sums, LR, EPS, ref.is_vec4(dims[c]))
    exact.assert_bits_equal(host(tables[c]), w, f'w of column {c}')      # (a neighbour's accumulator, or a
    exact.assert_bits_equal(host(accs[c]), a, f'a of column {c}')        # second step, changes bits)


# ---- 4. max_norm ----------------------------------------------------------------------------------------------
def _clip_case(rng, dims, rows):
  from tests.test_gpu_max_norm import _ids, _splits, _table
  tables = [_table(rng, rows, d) for d in dims]
  splits = [_splits(rng, 150) for _ in dims]
  ids = [_ids(rng, rows, int(s[-1]), rows, np.int64) for s in splits]
  grads = [rng.randn(len(s) - 1, d).astype(F32) for s, d in zip(splits, dims)]
  return tables, ids, splits, grads


@pytest.mark.parametrize('emit', [True, False])
def test_max_norm_steps_with_the_clipped_gradient(emit):
  from tests.test_gpu_max_norm import C, grad64
  rng = np.random.RandomState(44)
  dims, rows = [16, 3, 64], 211
  tables, ids, splits, grads = _clip_case(rng, dims, rows)
  a0 = [rng.uniform(0.05, 0.5, size=(rows, 1)).astype(F32) for _ in dims]

  def run(emit, lr):
    ts, accs = [dev(t) for t in tables], [dev(a) for a in a0]
    lookup = GroupLookup(ts, buckets=[rows] * 3, combiners='mean', max_norms=C)
    grad = GroupLookupGrad(lookup, row_accums=accs, deterministic=True)
    res = grad([dev(i) for i in ids], [dev(g) for g in grads], [dev(s) for s in splits], apply_lr=lr,
               optimizer='rowwise_adagrad', emit=emit)
    torch.cuda.synchronize()
    return res, ts, accs
  # g' as the emit form returns it, against the float64 Jacobian (rows inside and outside the ball)
  res, ts, accs = run(True, LR)
  if not emit:
    _, ts, accs = run(False, LR)
  for c, d in enumerate(dims):
    u, gp = emitted(res[c])
    want_u, want, gm = grad64(tables[c], ids[c], splits[c], None, 'mean', grads[c], C, bucket=rows)
    norms = np.linalg.norm(tables[c][want_u].astype(np.float64), axis=1)
    assert (norms < C).any() and (norms > C).any()
    order = np.argsort(u)
    np.testing.assert_array_equal(u[order], want_u)
    assert_sums_close(gp[order], want, gm, err_msg=f"g' of column {c}")
    # the step from THAT g': the accumulator grew by mean(g'^2), the row moved by one rate -- bit for bit
    w, a = tables[c].copy(), a0[c].copy()
    ref.step(w, a, u, gp, LR, EPS, ref.is_vec4(d))
    exact.assert_bits_equal(host(ts[c]), w, f'w of column {c}')
    exact.assert_bits_equal(host(accs[c]), a, f'a of column {c}')


@pytest.mark.parametrize('emit', [True, False])
def test_big_power_of_two_max_norm_changes_no_bit(emit):
  from tests.test_gpu_max_norm import BIG, _small_table
  rng = np.random.RandomState(45)
  dims, rows = [16, 3, 64, 256], 301
  tables = [_small_table(rng, rows, d) for d in dims]
  ids = [rng.randint(0, rows, size=500).astype(np.int64) for _ in dims]
  grads = [rng.randn(500, d).astype(F32) for d in dims]
  results = []
  for max_norms in (None, BIG):
    ts = [dev(t) for t in tables]
    accs = [torch.full((rows, 1), A0, dtype=torch.float32, device=DEV) for _ in dims]
    grad = GroupLookupGrad(GroupLookup(ts, max_norms=max_norms), row_accums=accs, deterministic=True)
    res = grad([dev(i) for i in ids], [dev(g) for g in grads], apply_lr=LR, optimizer='rowwise_adagrad', emit=emit)
    torch.cuda.synchronize()
    got = [host(t) for t in ts] + [host(a) for a in accs]
    if emit:
      for r in res:
        got += list(emitted(r))
    results.append(got)
  for x, y in zip(*results):
    np.testing.assert_array_equal(x, y)
  assert not np.array_equal(results[0][0], tables[0])


# ---- 5. launch() and a captured graph -----------------------------------------------------------------------------
def test_graph_replay_and_launch_equal_eager_steps():
  rng = np.random.RandomState(5)
  rows, dim, K = 2003, 16, 3
  w = rng.uniform(-1, 1, size=(rows, dim)).astype(F32)
  sp = np.concatenate([[0], np.cumsum(rng.poisson(3, size=400).clip(0, 12))]).astype(np.int32)
  d_ids = dev(rng.randint(0, rows, size=int(sp[-1])).astype(np.int64))
  d_sp, d_g = dev(sp), dev(rng.randn(sp.size - 1, dim).astype(F32))

  def make():
    tables = [dev(w)]
    accs = [torch.full((rows, 1), A0, dtype=torch.float32, device=DEV)]
    return tables, accs, GroupLookupGrad(GroupLookup(tables, combiners='mean'), row_accums=accs, deterministic=True)
  step = dict(apply_lr=LR, optimizer='rowwise_adagrad')
  eager = make()
  for _ in range(K):
    eager[2]([d_ids], [d_g], [d_sp], **step)
  launched = make()
  launched[2]([d_ids], [d_g], [d_sp], **step)
  for _ in range(K - 1):
    launched[2].launch(LR, optimizer='rowwise_adagrad')
  graphed = make()
  graphed[2]([d_ids], [d_g], [d_sp], **step)   # binds; step 1
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      graphed[2].launch(LR, optimizer='rowwise_adagrad')
  torch.cuda.synchronize()
  for _ in range(K - 1):                      # (the capture records a step without running it)
    graph.replay()
  torch.cuda.synchronize()
  for other in (launched, graphed):
    exact.assert_bits_equal(host(other[0][0]), host(eager[0][0]))
    exact.assert_bits_equal(host(other[1][0]), host(eager[1][0]))
  assert not np.array_equal(host(eager[0][0]), w)


# ---- 6. sequence lookups ----------------------------------------------------------------------------------------------
def test_sequence_lookup_pad_row_collects_the_padding_once():
  rng = np.random.RandomState(6)
  rows, dim, T, B, pad = 53, 8, 4, 40, 7
  w0 = rng.uniform(-1, 1, size=(rows, dim)).astype(F32)
  a0 = rng.uniform(0, 0.5, size=(rows, 1)).astype(F32)
  lens = rng.randint(0, 7, size=B)              # shorter than, equal to and longer than T
  sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  ids = rng.randint(0, 1 << 20, size=int(sp[-1])).astype(np.int64)
  g = rng.randn(B, T, dim).astype(F32)
  for emit in (True, False):
    tables, accs = [dev(w0)], [dev(a0)]
    lookup = SequenceLookup(tables, [rows], max_lens=[T], pad_ids=[pad])
    lookup([dev(ids)], [dev(sp)])
    grad = SequenceLookupGrad(lookup, row_accums=accs)
    res = grad([dev(g)], apply_lr=LR, optimizer='rowwise_adagrad', emit=emit, deterministic=True)
    torch.cuda.synchronize()
    grid = np.full((B, T), pad, np.int64)
    for b in range(B):
      k = min(int(lens[b]), T)
      grid[b, :k] = ids[sp[b]:sp[b] + k] % rows
    assert (lens < T).any() and (lens > T).any()
    u, sums = dedup_in_order(grid.reshape(-1), g.reshape(B * T, dim), rows)
    assert pad in u
    w, a = w0.copy(), a0.copy()
    ref.step(w, a, u, sums, LR, EPS, True)
    if emit:
      got_u, got_g = emitted(res[0])
      np.testing.assert_array_equal(got_u, u)
      exact.assert_bits_equal(got_g, sums)
    exact.assert_bits_equal(host(tables[0]), w, f'w emit={emit}')
    exact.assert_bits_equal(host(accs[0]), a, f'a emit={emit}')
    # the pad row's accumulator: one step with the sum over every padding position, not one per position
    k = int(np.searchsorted(u, pad))
    one = F32(a0[pad, 0] + ref.row_sum_sq(sums[k:k + 1], True)[0] / F32(dim))
    assert host(accs[0])[pad, 0] == one


# ---- 7. sharded ---------------------------------------------------------------------------------------------------------
def _sharded_case(rng, world):
  dims, rows = [16, 8, 3], [1999, 1013, 503]
  n = len(dims)
  host_w = [rng.uniform(-1, 1, size=(rows[c], dims[c])).astype(F32) for c in range(n)]
  host_a = [rng.uniform(0, 0.5, size=(rows[c], 1)).astype(F32) for c in range(n)]
  ids = [[rng.randint(0, 1 << 30, size=int(rng.randint(100, 900))).astype(np.int64) for c in range(n)]
         for _ in range(world)]
  grads = [[rng.randn(i.size, dims[c]).astype(F32) for c, i in enumerate(r)] for r in ids]
  return dims, rows, host_w, host_a, ids, grads


def _single_gpu(rows, host_w, host_a, ids, grads, emit):
  """The unsharded step on the logical tables: every rank's ids and gradients as one batch, in rank order."""
  n = len(rows)
  tables, accs = [dev(w) for w in host_w], [dev(a) for a in host_a]
  grad = GroupLookupGrad(GroupLookup(tables, buckets=rows), row_accums=accs, deterministic=True)
  grad([dev(np.concatenate([r[c] for r in ids])) for c in range(n)],
       [dev(np.concatenate([r[c] for r in grads])) for c in range(n)], apply_lr=LR, optimizer='rowwise_adagrad',
       emit=emit)
  torch.cuda.synchronize()
  return [host(t) for t in tables], [host(a) for a in accs]


def _run_world(comms, world, dims, rows, host_w, host_a, ids, grads, emit):
  n = len(dims)
  shards = [[(dev(host_w[c][r::world].copy()), dev(host_a[c][r::world].copy())) for c in range(n)]
            for r in range(world)]
  errors = []

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        drv = ShardedGroupLookup([s[0] for s in shards[r]], comms[r], buckets=rows,
                                 row_accums=[s[1] for s in shards[r]])
        drv([dev(i) for i in ids[r]])
        res = drv.backward([dev(g) for g in grads[r]], apply_lr=LR, optimizer='rowwise_adagrad', emit=emit)
        torch.cuda.current_stream().synchronize()
        if emit:
          for c in range(n):
            u, _ = emitted(res[c])
            assert np.unique(u).size == u.size
        drv.close()
    except Exception as e:  # pylint: disable=broad-except
      import traceback
      errors.append((r, repr(e), traceback.format_exc()))

  threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=60)
  assert not errors, errors
  logical = []
  for k in range(2):
    out = []
    for c in range(n):
      full = np.empty_like((host_w, host_a)[k][c])
      for r in range(world):
        full[r::world] = host(shards[r][c][k])
      out.append(full)
    logical.append(out)
  return logical


@pytest.mark.parametrize('world', [1, 2, 4])
@pytest.mark.parametrize('emit', [True, False])
def test_sharded_equals_single_gpu(hbk_option, world, emit):
  hbk_option('bwd_deterministic', 1)
  rng = np.random.RandomState(300 + world)
  dims, rows, host_w, host_a, ids, grads = _sharded_case(rng, world)
  comms = hb.distribute.Collective.local_world(world)
  try:
    logical = _run_world(comms, world, dims, rows, host_w, host_a, ids, grads, emit)
  finally:
    for cm in comms:
      cm.close()
  want = _single_gpu(rows, host_w, host_a, ids, grads, emit)
  for k, what in enumerate(('weights', 'accumulator')):
    for c in range(len(dims)):
      exact.assert_bits_equal(logical[k][c], want[k][c], f'{what} of column {c}')
      assert not np.array_equal(want[k][c], (host_w, host_a)[k][c])


@pytest.mark.parametrize('emit', [True, False])
def test_sharded_through_a_real_communicator_world1(hbk_option, emit):
  hbk_option('bwd_deterministic', 1)
  rng = np.random.RandomState(399)
  dims, rows, host_w, host_a, ids, grads = _sharded_case(rng, 1)
  coll = hb.distribute.Collective(world_size=1, rank=0)
  try:
    logical = _run_world([coll], 1, dims, rows, host_w, host_a, ids, grads, emit)
  finally:
    coll.close()
  want = _single_gpu(rows, host_w, host_a, ids, grads, emit)
  for k in range(2):
    for c in range(len(dims)):
      exact.assert_bits_equal(logical[k][c], want[k][c], f'slot {k} column {c}')


# ---- 8. hash tables ------------------------------------------------------------------------------------------------------
class _HashRun:
  """One expiring HashTable under HashGroupLookup + row-wise Adagrad, and a model of its accumulators by key: a
  key's accumulator starts at A0, grows by the step's mean(g^2) and goes back to A0 when the key leaves."""

  def __init__(self, capacity, dim, slab_size=8):
    from hybridbackend_amd.embedding import HashGroupLookup, HashTable
    self.dim = dim
    self.opt = RowwiseAdagrad(epsilon=EPS, initial_accumulator_value=A0)
    self.table = HashTable(capacity, dim, DEV, slab_size=slab_size, init_scale=0.05, seed=3, expiring=True)
    self.hgl = HashGroupLookup([self.table])
    self.acc = self.opt.slots_like(self.table.table)
    self.model = {}
    self._bind()

  def _bind(self):
    assert tuple(self.acc.shape) == (self.table.capacity, 1)
    self.grad = GroupLookupGrad(self.hgl.lookup, row_accums=[self.acc], rowwise_adagrad=self.opt, deterministic=True)

  def step(self, n, ids, g):
    """One training step, held to the restatement: rows read after the insert are the pre-step rows."""
    self.table.set_step(n)
    self.hgl([dev(ids)])
    keys = np.unique(ids)
    slots = host(self.table.find(dev(keys)))
    assert (slots >= 0).all() and self.table.failed() == 0
    w = host(self.table.table)[slots]
    a = np.array([[self.model.get(int(k), F32(A0))] for k in keys], F32)
    np.testing.assert_array_equal(host(self.acc)[slots], a)       # (a new or returning key starts at the fill)
    self.grad(self.hgl.slots, [dev(g)], apply_lr=LR, optimizer='rowwise_adagrad')
    u, sums = dedup_in_order(np.searchsorted(keys, ids), g, keys.size)
    ref.step(w, a, u, sums, LR, EPS, ref.is_vec4(self.dim))
    exact.assert_bits_equal(host(self.table.table)[slots], w, f'rows after step {n}')
    exact.assert_bits_equal(host(self.acc)[slots], a, f'accumulators after step {n}')
    for k, x in zip(keys, a[:, 0]):
      self.model[int(k)] = x

  def by_key(self):
    from tests.test_gpu_hash_features import by_key
    return by_key(self.table, [self.table.table, self.acc])

  def check_model(self, what):
    got = self.by_key()
    assert set(got) == set(self.model), what
    for k, (_, a) in got.items():
      assert a[0] == self.model[k], (what, k)
    # every slot no key holds carries the fill value
    keys = host(self.table.keys)
    free = (keys == -2 ** 63) | (keys == -2 ** 63 + 1)
    assert free.any() and (host(self.acc)[free, 0] == F32(A0)).all(), what


def test_hash_table_evict_grow_export_import_by_key():
  from hybridbackend_amd.embedding import HashTable
  from tests.test_gpu_hash_features import assert_same_by_key, wide_keys
  rng = np.random.RandomState(8)
  dim = 8
  pool = wide_keys(rng, 110)
  run = _HashRun(512, dim)
  old, rest = pool[:60], pool[60:]
  for n, part in ((1, old), (2, old), (3, rest), (4, rest)):
    ids = part[rng.randint(0, part.size, size=150)]
    run.step(n, ids, rng.randn(ids.size, dim).astype(F32))
  run.check_model('after training')
  # evict: keys last seen 8 or more steps before step 10 (the keys of steps 1 and 2 only) leave; the freed slots'
  # accumulators go back to the fill value
  gone = np.array(sorted(k for k in run.model if k in set(old.tolist())), np.int64)
  slots_gone = host(run.table.find(dev(gone)))
  assert (host(run.acc)[slots_gone, 0] != F32(A0)).all()
  run.table.set_step(10)
  run.table.evict(8, slots=[(run.acc, A0)])
  torch.cuda.synchronize()
  assert (host(run.table.find(dev(gone))) < 0).all() and run.table.evicted() == gone.size
  assert (host(run.acc)[slots_gone, 0] == F32(A0)).all()
  for k in gone:
    del run.model[int(k)]
  run.check_model('after evict')
  # the evicted ids come back: they train as new keys (step() checks the fill and the restatement)
  ids = np.concatenate([gone[:30], rest[:20], gone[:30]])
  run.step(11, ids, rng.randn(ids.size, dim).astype(F32))
  # maybe_grow: the [capacity, 1] companion moves with its keys
  before = run.by_key()
  out = run.hgl.maybe_grow(max_load=0.2, factor=2.0, slots=[[(run.acc, A0)]])
  assert out[0] is not None and run.table.capacity == 1024
  run.acc = out[0][0]
  run._bind()   # pylint: disable=protected-access
  assert_same_by_key(run.by_key(), before, 'maybe_grow')
  run.check_model('after maybe_grow')
  ids = pool[rng.randint(0, pool.size, size=200)]
  run.step(12, ids, rng.randn(ids.size, dim).astype(F32))
  # export / import into another capacity and slab size
  exp = run.table.export_items(slots=[run.acc])
  assert tuple(exp.slots[0].shape) == (len(run.model), 1)
  other = HashTable(768, dim, DEV, slab_size=4, init_scale=0.05, seed=3, expiring=True)
  acc2 = run.opt.slots_like(other.table)
  other.import_items(exp, [(acc2, A0)])
  from tests.test_gpu_hash_features import by_key
  assert_same_by_key(by_key(other, [other.table, acc2]), run.by_key(), 'import_items')
  run.check_model('at the end')


def test_hash_id_removed_and_seen_again_trains_as_in_a_fresh_table():
  from tests.test_gpu_hash_features import wide_keys
  rng = np.random.RandomState(9)
  dim = 8
  pool = wide_keys(rng, 60)
  run = _HashRun(512, dim)
  for n in (1, 2):
    ids = pool[rng.randint(0, pool.size, size=150)]
    run.step(n, ids, rng.randn(ids.size, dim).astype(F32))
  again = np.array(sorted(run.model), np.int64)[:25]
  slots = host(run.table.find(dev(again)))
  run.hgl.remove([dev(again)], slots=[[(run.acc, A0)]])
  torch.cuda.synchronize()
  assert (host(run.table.find(dev(again))) < 0).all()
  assert (host(run.acc)[slots, 0] == F32(A0)).all()
  for k in again:
    del run.model[int(k)]
  run.check_model('after remove')
  ids = again[rng.randint(0, again.size, size=90)]
  g = rng.randn(ids.size, dim).astype(F32)
  run.step(3, ids, g)
  fresh = _HashRun(256, dim, slab_size=4)
  fresh.step(3, ids, g)
  seen, new = run.by_key(), fresh.by_key()
  assert set(new) == set(np.unique(ids).tolist())
  for k, (row, a) in new.items():
    exact.assert_bits_equal(seen[k][0], row, f'row of key {k}')
    exact.assert_bits_equal(seen[k][1], a, f'accumulator of key {k}')


# ---- 9. feature columns ---------------------------------------------------------------------------------------------------
fc = hb.feature_column
NB, HD = 211, 16


def _fc_columns(cap=512, slab=8):
  return [fc.EmbeddingColumn('b', NB, 6, 'sum', hot_rows=False),
          fc.HashEmbeddingColumn('h', cap, HD, 'mean', init_scale=0.05, seed=4, expiring=True, slab_size=slab)]


def _fc_layer(dense, comm=None, r=0, world=1, fresh=False, **kw):
  def init(col, rows, d):
    return torch.zeros(rows, col.dimension, device=DEV) if fresh else dev(dense[r::world].copy())
  return fc.DenseFeatures(_fc_columns(**kw), DEV, coll=comm, init=init, optimizer='rowwise_adagrad',
                          rowwise_adagrad=RowwiseAdagrad(epsilon=EPS, initial_accumulator_value=A0))


def _fc_batches(rng, steps, world, B, pool):
  from tests.test_gpu_hash_features import ragged
  out = []
  for _ in range(steps):
    per_rank = []
    for _ in range(world):
      hi, hs = ragged(rng, pool, B)
      per_rank.append(dict(b=rng.randint(0, 10 ** 6, size=B).astype(np.int64), h=hi, hs=hs,
                           grad=rng.randn(B, 6 + HD).astype(F32)))
    out.append(per_rank)
  return out


def _fc_step(layer, n, b):
  layer.set_step(n)
  layer({'b': dev(b['b']), 'h': (dev(b['h']), dev(b['hs']))})
  return layer.backward(dev(b['grad']), apply_lr=LR, optimizer='rowwise_adagrad', emit=False)


def _fc_state(layer):
  from tests.test_gpu_hash_features import by_key
  t = layer.hash_tables[1]
  assert layer.weights[1] is t.table and tuple(layer.row_accums[1].shape) == (t.capacity, 1)
  assert tuple(layer.row_accums[0].shape) == (layer.weights[0].shape[0], 1)
  return dict(b=host(layer.weights[0]), b_acc=host(layer.row_accums[0]),
              h=by_key(t, [t.table, layer.row_accums[1], t.last_seen, t.freq]))


@pytest.fixture
def deterministic():
  old = _lib.set_option('bwd_deterministic', 1)
  yield
  _lib.set_option('bwd_deterministic', old)


def test_dense_features_equal_the_hand_composition(deterministic):   # pylint: disable=unused-argument,redefined-outer-name
  from hybridbackend_amd.embedding import HashGroupLookup, HashTable
  from tests.test_gpu_hash_features import assert_same_by_key, by_key, wide_keys
  rng = np.random.RandomState(91)
  dense = rng.uniform(-1, 1, size=(NB, 6)).astype(F32)
  batches = _fc_batches(rng, 3, 1, 48, wide_keys(rng, 70))
  layer = _fc_layer(dense)
  assert layer.accums is None and layer.moments is None and layer.ftrl_slots is None
  opt = RowwiseAdagrad(epsilon=EPS, initial_accumulator_value=A0)
  w = dev(dense)
  col = _fc_columns()[1]
  table = HashTable(col.capacity, col.dimension, DEV, **col.table_args)
  hgl = HashGroupLookup([table], combiners=['mean'])
  accs = [opt.slots_like(w), opt.slots_like(table.table)]
  g_b = GroupLookupGrad(GroupLookup([w], buckets=[NB], combiners='sum'), row_accums=accs[:1], rowwise_adagrad=opt)
  g_h = GroupLookupGrad(hgl.lookup, row_accums=accs[1:], rowwise_adagrad=opt)
  for n, (b,) in enumerate(batches):
    _fc_step(layer, n + 1, b)
    table.set_step(n + 1)
    hgl([dev(b['h'])], [dev(b['hs'])])
    g = dev(b['grad'])
    g_b([dev(b['b'])], [g[:, :6].contiguous()], apply_lr=LR, optimizer='rowwise_adagrad', emit=False)
    g_h(hgl.slots, [g[:, 6:].contiguous()], [dev(b['hs'])], apply_lr=LR, optimizer='rowwise_adagrad', emit=False)
  torch.cuda.synchronize()
  got = _fc_state(layer)
  exact.assert_bits_equal(got['b'], host(w), 'bucketed weights')
  exact.assert_bits_equal(got['b_acc'], host(accs[0]), 'bucketed accumulators')
  assert not np.array_equal(got['b'], dense) and (got['b_acc'] != F32(A0)).any()
  assert_same_by_key(got['h'], by_key(table, [table.table, accs[1], table.last_seen, table.freq]), 'hash column')
  assert sorted(layer.variables()) == ['b_embedding/embedding_weights', 'b_embedding/embedding_weights/RowwiseAdagrad']
  layer.close()


def test_dense_features_checkpoint_across_world_sizes(tmp_path, deterministic):   # pylint: disable=unused-argument,redefined-outer-name
  from tests.test_gpu_hash_features import assert_same_by_key, merged, run_world, wide_keys
  rng = np.random.RandomState(92)
  dense = rng.uniform(-1, 1, size=(NB, 6)).astype(F32)
  batches = _fc_batches(rng, 2, 2, 40, wide_keys(rng, 60))
  p2, p1 = str(tmp_path / 'w2'), str(tmp_path / 'w1')
  barrier = threading.Barrier(2)

  # saved at W = 2 (and, by the same ranks, a W = 1 checkpoint restored at W = 2 further down)
  def train2(r, comm):
    layer = _fc_layer(dense, comm, r, 2)
    assert layer.sharded == [True, True]
    for n in range(2):
      _fc_step(layer, n + 1, batches[n][r])
    layer.save(p2, barrier=barrier.wait)
    st = _fc_state(layer)
    layer.close()
    return st
  saved2 = run_world(2, train2)
  index = set(hb.training.saver._read_index(p2)['variables'])   # pylint: disable=protected-access
  assert 'b_embedding/embedding_weights/RowwiseAdagrad' in index
  assert 'h_embedding/embedding_weights/part_1_of_2/items/slot0' in index
  one = _fc_layer(dense, fresh=True, cap=768, slab=4)
  one.restore(p2)
  got = _fc_state(one)
  one.close()
  keys2 = merged([s['h'] for s in saved2])
  assert len(keys2) > 40 and any(v[1][0] != F32(A0) for v in keys2.values())
  assert_same_by_key(got['h'], keys2, 'W = 2 -> W = 1, hash column')
  for r in range(2):
    exact.assert_bits_equal(got['b'][r::2], saved2[r]['b'], f'weights of rank {r}')
    exact.assert_bits_equal(got['b_acc'][r::2], saved2[r]['b_acc'], f'accumulators of rank {r}')
    assert (saved2[r]['b_acc'] != F32(A0)).any()

  # the other way round: saved at W = 1, restored at W = 2
  layer = _fc_layer(dense)
  for n in range(2):
    _fc_step(layer, n + 1, batches[n][0])
  layer.save(p1)
  saved1 = _fc_state(layer)
  layer.close()

  def restore2(r, comm):
    fresh = _fc_layer(dense, comm, r, 2, fresh=True, cap=256, slab=16)
    fresh.restore(p1, barrier=barrier.wait)
    st = _fc_state(fresh)
    fresh.close()
    return st
  at2 = run_world(2, restore2)
  assert_same_by_key(merged([s['h'] for s in at2]), saved1['h'], 'W = 1 -> W = 2, hash column')
  for r in range(2):
    assert all(k % 2 == r for k in at2[r]['h'])
    exact.assert_bits_equal(at2[r]['b'], saved1['b'][r::2], f'weights of rank {r}')
    exact.assert_bits_equal(at2[r]['b_acc'], saved1['b_acc'][r::2], f'accumulators of rank {r}')
