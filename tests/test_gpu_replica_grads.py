"""Replicated tables at W > 1 on the GPU: the pack and rows kernels and the slice apply, bit for bit against the
numpy restatement (tests/support/replica_grads_ref.py); SparseApply against GroupLookupGrad(deterministic=True)
stepping the same distinct rows; and the layers' aggregated step on Collective.local_world, where the sum over
ranks runs in rank order and the gradients sit on the exact grid of tests/support/exact.py, so every rank's
replicated tables and slots must equal the restatement's bits."""
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import GroupLookup, GroupLookupGrad, SparseApply
from tests.support import exact
from tests.support import reference
from tests.support import replica_grads_ref as ref
from tests.support.tolerance import assert_sums_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
LR = exact.EXACT_LR
fc = hb.feature_column
OPTIMIZERS = ('sgd', 'adagrad', 'adam', 'ftrl', 'rowwise_adagrad')


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


# ---- slices with everything that must not reach the bucket ----------------------------------------------------------
def make_slices(rng, rows, dim, n_unique='some', extra=5):
  """(unique_rows [cap], grad_rows [cap, dim], n_unique as the device holds it): distinct rows in random order,
  a -1 and a `rows` inside n_unique, and past it a stale tail of valid-looking rows with NaN gradients."""
  cap = rows + extra
  urows = np.full(cap, -1, np.int64)
  k = {'some': int(rng.randint(0, rows + 1)), 'all': rows, 'none': 0}.get(n_unique, 0)
  urows[:k] = rng.permutation(rows)[:k]
  n = k + 2
  urows[k], urows[k + 1] = -1, rows
  if n_unique in ('some', 'all', 'none'):
    nu = n
  elif n_unique == 'zero':
    nu, n = 0, 0
  elif n_unique == 'one':
    urows[0], nu, n = rows // 2, 1, 1
  elif n_unique == 'capacity':
    urows[:] = -1
    urows[:rows] = rng.permutation(rows)
    nu, n = cap, cap
  elif n_unique == 'above':        # the device value is clamped to the capacity
    urows[:] = -1
    urows[1:rows + 1] = rng.permutation(rows)
    nu, n = cap + 1000, cap
  else:                            # 'negative': clamped to 0
    nu, n = -7, 0
  urows[n:] = rng.randint(0, rows, size=cap - n)
  g = exact.exact_grads(rng, (cap, dim), 8)
  g[n:] = np.nan
  return urows, g, nu


class Bucket:
  """A bucket laid out by hand (block c at `offsets[c]` floats), pre-filled with NaN, and its C descriptors."""

  def __init__(self, shapes, slices, block_offsets=None):
    blocks, touched, total = ref.layout(shapes)
    if block_offsets is not None:
      blocks = list(block_offsets)
      at = max(o + r * d for o, (r, d) in zip(blocks, shapes))
      touched = []
      for r, _ in shapes:
        touched.append(at)
        at += r
      total = at
    self.lay = (blocks, touched, total)
    self.shapes = shapes
    self.store = torch.full((total + 4,), float('nan'), dtype=torch.float32, device=DEV)
    self.bucket = self.store[:total]
    self.urows = [torch.full((r,), -99, dtype=torch.int64, device=DEV) for r, _ in shapes]
    self.dev = [(dev(u), dev(g), torch.tensor([nu], dtype=torch.int32, device=DEV)) for u, g, nu in slices]
    n = len(shapes)
    self.cols = (_lib.ReplicaColumn * n)()
    for c, (rows, dim) in enumerate(shapes):
      col, (u, g, nu) = self.cols[c], self.dev[c]
      col.unique_rows, col.grad_rows, col.n_unique, col.capacity = u.data_ptr(), g.data_ptr(), nu.data_ptr(), u.numel()
      col.rows, col.dim = rows, dim
      col.block = self.bucket.data_ptr() + 4 * blocks[c]
      col.touched = self.bucket.data_ptr() + 4 * touched[c]
      col.urows = self.urows[c].data_ptr()

  def pack(self):
    return _lib.lib().hbk_replica_grads_pack_n(len(self.shapes), self.cols, self.bucket.data_ptr(),
                                               self.bucket.numel(), _lib.current_stream(DEV))

  def rows(self):
    return _lib.lib().hbk_replica_grads_rows_n(len(self.shapes), self.cols, _lib.current_stream(DEV))


def check_pack_and_rows(shapes, slices, **kw):
  b = Bucket(shapes, slices, **kw)
  _lib.check(b.pack())
  _lib.check(b.rows())
  torch.cuda.synchronize()
  want = ref.pack(shapes, slices, b.lay, fill=np.nan)
  exact.assert_bits_equal(host(b.bucket), want, 'bucket')
  assert np.isnan(host(b.store)[b.bucket.numel():]).all(), 'a store past the bucket'
  for c, (rows, _) in enumerate(shapes):
    np.testing.assert_array_equal(host(b.urows[c]), ref.rows_of(want[b.lay[1][c]:b.lay[1][c] + rows]), f'urows {c}')
  return b


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [1, 3, 4, 20, 64, 256])
def test_pack_and_rows_every_dim_and_row_count(dim):
  rng = np.random.RandomState(dim)
  shapes = [(rows, dim) for rows in (1, 255, 256, 257, 1000)]
  slices = [make_slices(rng, rows, dim, how) for (rows, _), how in zip(shapes, ('all', 'some', 'all', 'some', 'some'))]
  b = check_pack_and_rows(shapes, slices)
  assert all(b.cols[c].block % 16 == 0 for c in range(len(shapes)))


@pytest.mark.parametrize('dim', [3, 4])
def test_n_unique_zero_one_capacity_above_and_negative(dim):
  rng = np.random.RandomState(10 + dim)
  hows = ('zero', 'one', 'capacity', 'above', 'negative')
  shapes = [(257, dim)] * len(hows)
  check_pack_and_rows(shapes, [make_slices(rng, 257, dim, how) for how in hows])


@pytest.mark.parametrize('dim', [3, 4, 64])
def test_block_at_a_4_byte_aligned_offset(dim):
  """The block starts 4 bytes past a 16-byte boundary: 4-byte lanes for every dim (64 is the widest they take)."""
  rng = np.random.RandomState(20 + dim)
  shapes = [(257, dim), (40, dim)]
  slices = [make_slices(rng, r, d) for r, d in shapes]
  b = check_pack_and_rows(shapes, slices, block_offsets=[1, 1 + 257 * dim + 2])
  assert b.cols[0].block % 16 == 4


def test_dim_65_is_refused_on_the_4_byte_path_before_any_store():
  rng = np.random.RandomState(3)
  shapes = [(10, 65)]
  b = Bucket(shapes, [make_slices(rng, 10, 65)])
  assert b.pack() == _lib.INVALID_ARGUMENT
  assert '64 lanes' in _lib.lib().hbk_last_error().decode()
  # 128 floats take 16-byte lanes, but not from a block that is only 4-byte aligned
  b2 = Bucket([(10, 128)], [make_slices(rng, 10, 128)], block_offsets=[1])
  assert b2.pack() == _lib.INVALID_ARGUMENT
  torch.cuda.synchronize()
  assert np.isnan(host(b.store)).all() and np.isnan(host(b2.store)).all()


def test_65_columns_in_one_call():
  rng = np.random.RandomState(4)
  shapes = [((5, 300, 64)[c % 3] + c, (4, 3, 8, 1)[c % 4]) for c in range(65)]
  check_pack_and_rows(shapes, [make_slices(rng, r, d) for r, d in shapes])


# ---- 2. SparseApply against GroupLookupGrad(deterministic=True) ---------------------------------------------------------------
def _slots(kind, tables):
  if kind == 'adagrad':
    return dict(accums=[torch.full_like(t, 0.1) for t in tables])
  if kind == 'adam':
    return dict(moments=[(torch.zeros_like(t), torch.zeros_like(t)) for t in tables], adam=hb.embedding.LazyAdam())
  if kind == 'ftrl':
    opt = hb.embedding.Ftrl(l1=0.01, l2=0.02, l2_shrinkage=0.03)
    return dict(ftrl_slots=[opt.slots_like(t) for t in tables], ftrl=opt)
  if kind == 'rowwise_adagrad':
    opt = hb.embedding.RowwiseAdagrad(initial_accumulator_value=0.25)
    return dict(row_accums=[opt.slots_like(t) for t in tables], rowwise_adagrad=opt)
  return {}


def _state(kind, tables, kw):
  out = [host(t) for t in tables]
  for key in ('accums', 'row_accums'):
    out += [host(a) for a in kw.get(key, [])]
  for key in ('moments', 'ftrl_slots'):
    out += [host(x) for pair in kw.get(key, []) for x in pair]
  if 'adam' in kw:
    out.append(host(kw['adam'].beta_powers))
  return out


@pytest.mark.parametrize('optimizer', OPTIMIZERS)
def test_sparse_apply_equals_group_lookup_grad_on_the_same_distinct_rows(optimizer):
  rng = np.random.RandomState(30)
  shapes = [(300, 4), (257, 3), (40, 20)]
  w0 = [rng.uniform(-1, 1, size=s).astype(F32) for s in shapes]
  a_tables, b_tables = [dev(w) for w in w0], [dev(w) for w in w0]
  a_kw, b_kw = _slots(optimizer, a_tables), _slots(optimizer, b_tables)
  grad = GroupLookupGrad(GroupLookup(a_tables, combiners='sum'), deterministic=True, **a_kw)
  app = SparseApply(b_tables, **b_kw)
  for step in range(2):
    ids, grads, slices = [], [], []
    for rows, dim in shapes:
      k = int(rng.randint(1, rows))
      r = rng.permutation(rows)[:k].astype(np.int64)
      g = rng.randn(k, dim).astype(F32)
      ids.append(dev(r))
      grads.append(dev(g))
      # the same rows as hand-made slices: another order, -1 holes in between, a stale NaN tail past n_unique
      order = rng.permutation(k)
      cap = 2 * k + 7
      urows, gs = np.full(cap, -1, np.int64), np.full((cap, dim), np.nan, F32)
      urows[0:2 * k:2], gs[0:2 * k:2] = r[order], g[order]
      gs[1:2 * k:2] = 1e30
      urows[2 * k:] = rng.randint(0, rows, size=7)
      slices.append((dev(urows), dev(gs), torch.tensor([2 * k], dtype=torch.int32, device=DEV)))
    grad(ids, grads, apply_lr=0.05, optimizer=optimizer, emit=False)
    app(slices, 0.05, optimizer=optimizer)
  torch.cuda.synchronize()
  for k, (got, want) in enumerate(zip(_state(optimizer, b_tables, b_kw), _state(optimizer, a_tables, a_kw))):
    exact.assert_bits_equal(got, want, f'{optimizer}: tensor {k}')
  assert all(not np.array_equal(host(t), w) for t, w in zip(b_tables, w0))


# ---- 3. a captured pack -> rows -> apply graph --------------------------------------------------------------------------------
@pytest.mark.parametrize('optimizer', ['adam', 'rowwise_adagrad'])
def test_captured_pack_rows_apply_graph_replayed_after_the_slices_changed(optimizer):
  rng = np.random.RandomState(40)
  shapes = [(257, 4), (40, 3)]
  w0 = [exact.exact_tables(rng, r, d) for r, d in shapes]
  tables = [dev(w) for w in w0]
  kw = _slots(optimizer, tables)
  app = SparseApply(tables, **kw)
  rg = hb.distribute.ReplicatedGradients(shapes, None, device=DEV)
  rg.bucket.fill_(float('nan'))
  steps = [[make_slices(rng, r, d) for r, d in shapes] for _ in range(3)]
  d_slices = [(dev(u), dev(g), torch.tensor([nu], dtype=torch.int32, device=DEV)) for u, g, nu in steps[0]]
  agg = rg.aggregate(d_slices)           # binds; step 1 eagerly
  app(agg, LR, optimizer=optimizer)
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      rg.launch_pack()
      rg.launch_rows()
      app.launch()
  torch.cuda.synchronize()
  for step in steps[1:]:                  # (the capture records a step without running it)
    for (du, dg, dn), (u, g, nu) in zip(d_slices, step):
      du.copy_(dev(u))
      dg.copy_(dev(g))
      dn.fill_(nu)
    graph.replay()
  torch.cuda.synchronize()
  # the restatement: three steps on one rank (scale 1)
  states, powers = [], reference.ADAM_DEFAULTS[:2]
  for w in w0:
    st = dict(w=w.copy())
    if optimizer == 'adam':
      st.update(m=np.zeros_like(w), v=np.zeros_like(w))
    else:
      st.update(a=np.full((w.shape[0], 1), 0.25, F32))
    states.append(st)
  for step in steps:
    ref.aggregated_step(optimizer, states, shapes, [step], 1.0, LR, powers=powers)
    powers = reference.adam_finish(powers)
  for c, st in enumerate(states):
    exact.assert_bits_equal(host(tables[c]), st['w'], f'table {c}')
    if optimizer == 'adam':
      exact.assert_bits_equal(host(kw['moments'][c][0]), st['m'], f'm {c}')
      exact.assert_bits_equal(host(kw['moments'][c][1]), st['v'], f'v {c}')
    else:
      exact.assert_bits_equal(host(kw['row_accums'][c]), st['a'], f'accumulator {c}')
  if optimizer == 'adam':
    exact.assert_bits_equal(host(kw['adam'].beta_powers), np.array(powers, F32), 'beta powers')


# ---- 4. the layers on Collective.local_world ----------------------------------------------------------------------------------
B = 48
REP = [('a', 7, 4), ('b', 40, 8), ('c', 48, 3)]
SHD = ('s', 1000, 8)
STEPS = 3


def run_world(world, body):
  """body(rank, comm) on one thread and one stream per rank; returns the per-rank results."""
  comms = hb.distribute.Collective.local_world(world)
  results, errors = [None] * world, []

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        results[r] = body(r, comms[r])
        torch.cuda.current_stream().synchronize()
    except Exception as e:  # pylint: disable=broad-except
      import traceback
      errors.append((r, repr(e), traceback.format_exc()))
  try:
    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
      t.start()
    for t in threads:
      t.join(timeout=120)
    assert not errors, errors
    assert not any(t.is_alive() for t in threads), 'a rank did not finish'
  finally:
    for cm in comms:
      cm.close()
  return results


def dense_columns(max_norm=None):
  cols = [fc.EmbeddingColumn(k, n, d, 'sum', hot_rows=False) for k, n, d in REP]
  if max_norm is not None:
    cols[1] = fc.EmbeddingColumn('b', 40, 8, 'sum', hot_rows=False, max_norm=max_norm)
  return cols + [fc.EmbeddingColumn(SHD[0], SHD[1], SHD[2], 'sum', hot_rows=False)]


def layer_kwargs(optimizer):
  if optimizer == 'adagrad':
    return dict(initial_accumulator_value=0.1)
  return {} if optimizer == 'sgd' else dict(optimizer=optimizer)


def initial_tables(rng, random=False):
  make = (lambda r, d: rng.uniform(-1, 1, size=(r, d)).astype(F32)) if random else \
      (lambda r, d: exact.exact_tables(rng, r, d))
  return {k: make(n, d) for k, n, d in REP + [SHD]}


def make_layer(tables, comm, r, world, optimizer, cols=None, **kw):
  def init(col, rows, d):
    t = tables[col.key]
    return dev(t[r::world].copy() if rows != t.shape[0] else t.copy())
  return fc.DenseFeatures(cols or dense_columns(), DEV, coll=comm, batch_size=B, init=init, **layer_kwargs(optimizer),
                          **kw)


def allowed_rows(n):
  """The rows the batches draw from: every fifth row is touched by no rank in any step."""
  return np.array([r for r in range(n) if r % 5 != 4], np.int64)


def make_batches(rng, world, steps=STEPS, random=False):
  """[step][rank] -> dict(ids per key, grad [B, width]).  Gradients on the exact grid: at most B * world terms of 8
  value bits and 4 fraction bits meet in one row, so every sum over ids and ranks is exact in any order."""
  width = sum(d for _, _, d in REP) + SHD[2]
  out = []
  for _ in range(steps):
    per_rank = []
    for _ in range(world):
      b = {k: rng.choice(allowed_rows(n), size=B) for k, n, _ in REP}
      b[SHD[0]] = rng.randint(0, SHD[1], size=B).astype(np.int64)
      b['grad'] = rng.randn(B, width).astype(F32) if random else exact.exact_grads(rng, (B, width), 8)
      per_rank.append(b)
    out.append(per_rank)
  return out


def local_slices(batch, key, n, dim, offset):
  """One rank's IndexedSlices of a replicated 'sum' column with one id per sample: distinct rows ascending and
  their exact sums."""
  sums = exact.exact_dense((n, dim), batch[key], batch['grad'][:, offset:offset + dim].astype(np.float64))
  return sums.rows, sums.sums(), sums.rows.size


def fresh_states(optimizer, tables):
  states = []
  for k, n, d in REP:
    st = dict(w=tables[k].copy())
    if optimizer == 'adagrad':
      st['a'] = np.full((n, d), 0.1, F32)
    elif optimizer == 'adam':
      st.update(m=np.zeros((n, d), F32), v=np.zeros((n, d), F32))
    elif optimizer == 'ftrl':
      st.update(a=np.full((n, d), 0.1, F32), z=np.zeros((n, d), F32))
    elif optimizer == 'rowwise_adagrad':
      st['a'] = np.zeros((n, 1), F32)
    states.append(st)
  return states


def restate(optimizer, tables, batches, world, scale):
  """The replicated tables and slots after every step of `batches`, and the beta powers."""
  states, powers = fresh_states(optimizer, tables), reference.ADAM_DEFAULTS[:2]
  shapes = [(n, d) for _, n, d in REP]
  for per_rank in batches:
    slices, off = [[] for _ in range(world)], 0
    for k, n, d in REP:
      for r in range(world):
        slices[r].append(local_slices(per_rank[r], k, n, d, off))
      off += d
    ref.aggregated_step(optimizer, states, shapes, slices, scale, LR, powers=powers)
    powers = reference.adam_finish(powers)
  return states, powers


def layer_state(layer, optimizer):
  """Per replicated table the dict the restatement keeps, from the layer's tensors."""
  out = []
  for c in layer._rep:
    st = dict(w=host(layer.weights[c]))
    if optimizer == 'adagrad':
      st['a'] = host(layer.accums[c])
    elif optimizer == 'adam':
      st.update(m=host(layer.moments[c][0]), v=host(layer.moments[c][1]))
    elif optimizer == 'ftrl':
      st.update(a=host(layer.ftrl_slots[c][0]), z=host(layer.ftrl_slots[c][1]))
    elif optimizer == 'rowwise_adagrad':
      st['a'] = host(layer.row_accums[c])
    out.append(st)
  return out


def features(b):
  return {k: dev(b[k]) for k in b if k != 'grad'}


def assert_states_equal(got, want, what):
  for c, (g, w) in enumerate(zip(got, want)):
    assert sorted(g) == sorted(w)
    for name in w:
      exact.assert_bits_equal(g[name], w[name], f'{what}: table {REP[c][0]}: {name}')


@pytest.mark.parametrize('world', [2, 3, 4])
@pytest.mark.parametrize('optimizer', OPTIMIZERS)
def test_layer_steps_replicated_tables_bit_equal_on_every_rank(world, optimizer):
  rng = np.random.RandomState(100 * world + OPTIMIZERS.index(optimizer))
  tables = initial_tables(rng)
  batches = make_batches(rng, world)

  def body(r, comm):
    agg = make_layer(tables, comm, r, world, optimizer, aggregate_replicated=True)
    plain = make_layer(tables, comm, r, world, optimizer)
    assert [agg.sharded[c] for c in range(4)] == [False, False, False, True]
    local = []
    for per_rank in batches:
      agg(features(per_rank[r]))
      res = agg.backward(dev(per_rank[r]['grad']), apply_lr=LR, optimizer=optimizer)
      local.append([(host(u)[:int(k)], host(g)[:int(k)]) for u, g, k in res[:3]])
      plain(features(per_rank[r]))
      plain.backward(dev(per_rank[r]['grad']), apply_lr=LR, optimizer=optimizer)
    drift = float(agg.replica_drift())
    out = dict(agg=layer_state(agg, optimizer), plain=layer_state(plain, optimizer), drift=drift, local=local,
               shard=(host(agg.weights[3]), host(plain.weights[3])),
               powers=host(agg.adam.beta_powers) if optimizer == 'adam' else None)
    agg.close()
    plain.close()
    return out
  results = run_world(world, body)
  want, powers = restate(optimizer, tables, batches, world, 1.0 / world)
  for r, res in enumerate(results):
    assert_states_equal(res['agg'], want, f'rank {r}')
    assert res['drift'] == 0.0
    # the sharded table is as without the argument; without it the replicated tables are not stepped at all
    exact.assert_bits_equal(res['shard'][0], res['shard'][1], f'rank {r}: the sharded table')
    assert not np.array_equal(res['shard'][0], tables['s'][r::world])
    for c, (k, _, _) in enumerate(REP):
      exact.assert_bits_equal(res['plain'][c]['w'], tables[k], f'rank {r}: {k} without the argument')
    if optimizer == 'adam':
      exact.assert_bits_equal(res['powers'], np.array(powers, F32), f'rank {r}: beta powers')
    # the return value stays this rank's LOCAL slices
    off = 0
    for c, (k, n, d) in enumerate(REP):
      u, g, _ = local_slices(batches[-1][r], k, n, d, off)
      got_u, got_g = res['local'][-1][c]
      order = np.argsort(got_u)
      np.testing.assert_array_equal(got_u[order], u)
      exact.assert_bits_equal(got_g[order], g, f'rank {r}: local slices of {k}')
      off += d
  # untouched rows and their slots keep their bits; touched ones moved
  first = fresh_states(optimizer, tables)
  for c, (k, n, _) in enumerate(REP):
    untouched = np.setdiff1d(np.arange(n), allowed_rows(n))
    assert untouched.size
    for name in want[c]:
      exact.assert_bits_equal(results[0]['agg'][c][name][untouched], first[c][name][untouched], f'{k}: {name}')
    assert not np.array_equal(results[0]['agg'][c]['w'], tables[k])


def test_adam_steps_a_row_one_rank_touched_and_a_row_whose_gradients_cancel():
  """Row 5 of table b is touched by rank 1 only: rank 0 steps it too, with the same bits.  Row 6 is touched by both
  ranks with opposite gradients in step 2: the sum is zero, and Lazy Adam still decays m and v and moves the row."""
  world, rng = 2, np.random.RandomState(7)
  tables = initial_tables(rng)
  batches = make_batches(rng, world, steps=2)
  off_b = REP[0][2]
  for step, per_rank in enumerate(batches):
    for r, b in enumerate(per_rank):
      b['b'] = np.where(np.isin(b['b'], (5, 6)), 7, b['b'])
      b['b'][0] = 6
    per_rank[1]['b'][1] = 5
    if step == 1:
      per_rank[1]['grad'][0, off_b:off_b + 8] = -per_rank[0]['grad'][0, off_b:off_b + 8]

  def body(r, comm):
    layer = make_layer(tables, comm, r, world, 'adam', aggregate_replicated=True)
    mid = None
    for per_rank in batches:
      mid = layer_state(layer, 'adam')
      layer(features(per_rank[r]))
      layer.backward(dev(per_rank[r]['grad']), apply_lr=LR, optimizer='adam', emit=False)
    out = (mid, layer_state(layer, 'adam'), float(layer.replica_drift()))
    layer.close()
    return out
  results = run_world(world, body)
  want, _ = restate('adam', tables, batches, world, 0.5)
  for r, (mid, end, drift) in enumerate(results):
    assert_states_equal(end, want, f'rank {r}')
    assert drift == 0.0
  mid, end, _ = results[0]
  b1, b2 = reference.ADAM_DEFAULTS[:2]
  assert (mid[1]['m'][6] != 0).any() and (mid[1]['v'][6] != 0).any()
  exact.assert_bits_equal(end[1]['m'][6], (b1 * mid[1]['m'][6]).astype(F32) + F32(0), 'm decays')
  exact.assert_bits_equal(end[1]['v'][6], (b2 * mid[1]['v'][6]).astype(F32) + F32(0), 'v decays')
  assert (end[1]['w'][6] != mid[1]['w'][6]).any(), 'the row moves with its decayed momentum'
  assert (end[1]['w'][5] != tables['b'][5]).any() and (end[1]['m'][5] != 0).any()


@pytest.mark.parametrize('world', [1, 2])
def test_emit_false_scale_one_and_world_one(world):
  """emit=False returns (None, None, n_unique) for the replicated columns and steps the same bits; scale 1.0 sums
  instead of averaging; at W = 1 the argument changes nothing."""
  rng = np.random.RandomState(50 + world)
  tables = initial_tables(rng)
  batches = make_batches(rng, world, steps=2)

  def body(r, comm):
    comm = comm if world > 1 else None
    kw = dict(aggregate_replicated=True, replicated_scale=1.0 if world > 1 else None)
    a = make_layer(tables, comm, r, world, 'adagrad', **kw)
    b = make_layer(tables, comm, r, world, 'adagrad', **(kw if world > 1 else {}))
    for per_rank in batches:
      a(features(per_rank[r]))
      res_a = a.backward(dev(per_rank[r]['grad']), apply_lr=LR, optimizer='adagrad', emit=False)
      b(features(per_rank[r]))
      res_b = b.backward(dev(per_rank[r]['grad']), apply_lr=LR, optimizer='adagrad', emit=True)
      assert all(x[0] is None and x[1] is None and int(x[2]) == int(y[2]) for x, y in zip(res_a[:3], res_b[:3]))
    out = (layer_state(a, 'adagrad'), layer_state(b, 'adagrad'), host(a.weights[3]), host(b.weights[3]))
    a.close()
    b.close()
    return out
  if world == 1:
    results = [body(0, None)]
    torch.cuda.synchronize()
  else:
    results = run_world(world, body)
  want, _ = restate('adagrad', tables, batches, world, 1.0)
  for r, (sa, sb, wa, wb) in enumerate(results):
    assert_states_equal(sa, want, f'rank {r}, emit=False')
    assert_states_equal(sb, want, f'rank {r}, emit=True')
    exact.assert_bits_equal(wa, wb, 'the fourth table')


def test_max_norm_column_and_random_gradients_against_float64():
  """N(0, 1) gradients and a clipped column: the ranks aggregate the g' of their local clip passes (taken at the
  pre-step rows, which are equal on every rank) and the aggregated step is not clipped again.  One SGD step, held
  to assert_sums_close against float64; the ranks agree bit for bit whatever the values."""
  world, rng, c_norm = 3, np.random.RandomState(60), 0.75
  tables = initial_tables(rng, random=True)
  tables['b'][::2] *= F32(0.2)        # rows inside the ball next to rows outside it
  batches = make_batches(rng, world, steps=1, random=True)

  def body(r, comm):
    layer = make_layer(tables, comm, r, world, 'sgd', cols=dense_columns(max_norm=c_norm), aggregate_replicated=True)
    layer(features(batches[0][r]))
    layer.backward(dev(batches[0][r]['grad']), apply_lr=LR)
    out = (layer_state(layer, 'sgd'), float(layer.replica_drift()))
    layer.close()
    return out
  results = run_world(world, body)
  off = 0
  for c, (k, n, d) in enumerate(REP):
    g64, mag = np.zeros((n, d)), np.zeros((n, d))
    for r in range(world):
      u, gp, gm = reference.backward64(tables[k], batches[0][r][k], None, None, 'sum',
                                       batches[0][r]['grad'][:, off:off + d], c_norm if k == 'b' else 0.0, bucket=n)
      g64[u] += gp
      mag[u] += gm
    want = tables[k].astype(np.float64) - LR * g64 / world
    for r, (state, drift) in enumerate(results):
      assert_sums_close(state[c]['w'], want, np.abs(tables[k]) + LR * mag / world, err_msg=f'rank {r}: table {k}')
      exact.assert_bits_equal(state[c]['w'], results[0][0][c]['w'], f'rank {r} against rank 0: table {k}')
      assert drift == 0.0
    off += d
  assert (np.linalg.norm(tables['b'], axis=1) > c_norm).any() and (np.linalg.norm(tables['b'], axis=1) < c_norm).any()


def test_replica_drift_returns_a_perturbation_made_by_hand():
  world, rng = 2, np.random.RandomState(70)
  tables = initial_tables(rng)

  def body(r, comm):
    layer = make_layer(tables, comm, r, world, 'sgd', aggregate_replicated=True)
    before = float(layer.replica_drift())
    if r == 1:
      layer.weights[1][3, 2] += 0.375
    after = float(layer.replica_drift())
    layer.close()
    return before, after
  assert run_world(world, body) == [(0.0, 0.375)] * world


def test_wide_replicated_column_is_refused_at_construction():
  """Refused before any lookup object is built or the collective is used (so a stand-in for it will do)."""
  import types
  coll = types.SimpleNamespace(world_size=2, rank=0)
  for dim in (260, 66):
    cols = [fc.EmbeddingColumn('w', 8, dim, 'sum', hot_rows=False)]
    with pytest.raises(_lib.InvalidArgumentError, match="replicated column 'w'"):
      fc.DenseFeatures(cols, DEV, coll=coll, batch_size=B, aggregate_replicated=True)
    seq = [fc.SequenceEmbeddingColumn('w', 8, dim, 4)]
    with pytest.raises(_lib.InvalidArgumentError, match="replicated column 'w'"):
      fc.SequenceFeatures(seq, DEV, coll=coll, batch_size=B, aggregate_replicated=True)


# ---- 5. SequenceFeatures ---------------------------------------------------------------------------------------------------------
def test_sequence_features_zero_padded_and_pad_id_columns():
  """Two replicated sequence columns at W = 2 under Lazy Adam: padding positions of the zero-padded column reach no
  row; those of the pad_id column collect in the pad row, on the rank that has them and, aggregated, on both."""
  world, rng, T = 2, np.random.RandomState(80), 4
  cols = lambda: [fc.SequenceEmbeddingColumn('z', 40, 4, T), fc.SequenceEmbeddingColumn('p', 30, 3, T, pad_id=2)]   # noqa: E731
  shapes = [(40, 4), (30, 3)]
  tables = {'z': exact.exact_tables(rng, 40, 4), 'p': exact.exact_tables(rng, 30, 3)}
  batches = []
  for _ in range(2):
    per_rank = []
    for _ in range(world):
      b = {}
      for key, n in (('z', 40), ('p', 30)):
        lens = rng.randint(0, 7, size=B)
        b[key] = (rng.choice(allowed_rows(n), size=int(lens.sum())), exact.splits_of(lens))
      b['grads'] = [exact.exact_grads(rng, (B, T, d), 6) for _, d in shapes]
      per_rank.append(b)
    batches.append(per_rank)

  def body(r, comm):
    layer = fc.SequenceFeatures(cols(), DEV, coll=comm, batch_size=B, optimizer='adam', aggregate_replicated=True,
                                init=lambda col, rows, d: dev(tables[col.key]))
    assert layer.sharded == [False, False]
    for per_rank in batches:
      b = per_rank[r]
      layer({k: (dev(b[k][0]), dev(b[k][1])) for k in ('z', 'p')})
      layer.backward([dev(g) for g in b['grads']], apply_lr=LR, optimizer='adam')
    out = ([dict(w=host(layer.weights[c]), m=host(layer.moments[c][0]), v=host(layer.moments[c][1])) for c in (0, 1)],
           float(layer.replica_drift()), host(layer.adam.beta_powers))
    layer.close()
    return out
  results = run_world(world, body)
  states = [dict(w=tables[k].copy(), m=np.zeros(s, F32), v=np.zeros(s, F32)) for k, s in zip(('z', 'p'), shapes)]
  powers = reference.ADAM_DEFAULTS[:2]
  for per_rank in batches:
    slices = []
    for b in per_rank:
      mine = []
      for c, (key, pad) in enumerate((('z', None), ('p', 2))):
        ids, sp = b[key]
        rows_, terms = [], []
        for s in range(B):
          k = min(int(sp[s + 1] - sp[s]), T)
          for t in range(T):
            if t < k:
              rows_.append(int(ids[sp[s] + t]))
            elif pad is not None:
              rows_.append(pad)
            else:
              continue
            terms.append(b['grads'][c][s, t])
        sums = exact.exact_dense(shapes[c], np.array(rows_, np.int64), np.array(terms, np.float64).reshape(-1, shapes[c][1]))
        mine.append((sums.rows, sums.sums(), sums.rows.size))
      slices.append(mine)
    ref.aggregated_step('adam', states, shapes, slices, 0.5, LR, powers=powers)
    powers = reference.adam_finish(powers)
  for r, (got, drift, got_powers) in enumerate(results):
    for c in (0, 1):
      for name in ('w', 'm', 'v'):
        exact.assert_bits_equal(got[c][name], states[c][name], f'rank {r}: column {c}: {name}')
    assert drift == 0.0
    exact.assert_bits_equal(got_powers, np.array(powers, F32), 'beta powers')
  assert (states[1]['m'][2] != 0).any(), 'the pad row collected gradient'
  untouched = np.setdiff1d(np.arange(40), allowed_rows(40))
  exact.assert_bits_equal(results[0][0][0]['w'][untouched], tables['z'][untouched], 'untouched rows')
