"""Lazy Adam (tf.contrib.opt.LazyAdamOptimizer's sparse apply) on the GPU: one step bit-equal to a numpy
fp32 restatement applied to the call's own IndexedSlices, every distinct row stepped exactly once,
deterministic multi-step runs bit-equal to a fully numpy reference, the interleaved [w|m|v|pad] row
pitch, captured-graph replay, and the sharded driver against the single-GPU step."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import oracle
import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import GroupLookup, GroupLookupGrad, LazyAdam
from hybridbackend_amd.embedding.sharded import ShardedGroupLookup

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
B1, B2, EPS = F32(0.9), F32(0.999), F32(1e-8)


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- numpy fp32 restatement of the step (every op a separately rounded fp32 op, in this order) ------
def np_adam(w, m, v, rows, g, lr, b1p, b2p, b1=B1, b2=B2, eps=EPS):
  lr, b1p, b2p = F32(lr), F32(b1p), F32(b2p)
  lr_t = F32(F32(lr * np.sqrt(F32(F32(1) - b2p))) / F32(F32(1) - b1p))
  g = g.astype(F32)
  mr = (b1 * m[rows]).astype(F32) + (F32(F32(1) - b1) * g).astype(F32)
  vr = (b2 * v[rows]).astype(F32) + (F32(F32(1) - b2) * (g * g)).astype(F32)
  m[rows] = mr
  v[rows] = vr
  w[rows] = w[rows] - (lr_t * mr) / (np.sqrt(vr) + eps)
  return F32(b1p * b1), F32(b2p * b2)


def ragged(rng, n_seg, lam=3, cap=12):
  lens = rng.poisson(lam, size=n_seg).clip(0, cap)
  return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def emitted(res):
  u, g, k = res
  k = int(k.item())
  return u.cpu().numpy()[:k], g.cpu().numpy()[:k]


def valid_rows(ids, rows, bucket=0, divisor=1):
  r = np.asarray(ids, np.int64)
  if bucket:
    r = r % bucket
  r = np.where(r >= 0, r // divisor, -1)
  return np.unique(r[(r >= 0) & (r < rows)])


def state(rng, rows, dim):
  w = rng.uniform(-1, 1, size=(rows, dim)).astype(F32)
  m = rng.uniform(-0.1, 0.1, size=(rows, dim)).astype(F32)
  v = rng.uniform(0, 0.01, size=(rows, dim)).astype(F32)
  return w, m, v


def check_one_step(tables, moms, res, host, lr, p0, powers):
  """w, m, v after ONE emit-mode step == numpy on the call's own slices; powers == fp32 products."""
  want_p = None
  for c in range(len(tables)):
    u, g = emitted(res[c])
    assert np.unique(u).size == u.size, f'column {c}: a row emitted twice'
    w, m, v = (x.copy() for x in host[c])
    want_p = np_adam(w, m, v, u, g, lr, p0[0], p0[1])
    np.testing.assert_array_equal(tables[c].cpu().numpy(), w, err_msg=f'w of column {c}')
    np.testing.assert_array_equal(moms[c][0].cpu().numpy(), m, err_msg=f'm of column {c}')
    np.testing.assert_array_equal(moms[c][1].cpu().numpy(), v, err_msg=f'v of column {c}')
  np.testing.assert_array_equal(powers.cpu().numpy(), np.array(want_p, F32))


# ---- 1. one step against the slices it emitted ----------------------------------------------------
@pytest.mark.parametrize('dim', [1, 3, 4, 8, 16, 64, 128, 256])
@pytest.mark.parametrize('id64', [False, True])
def test_one_step_bit_equal_to_its_own_slices(dim, id64):
  rng = np.random.RandomState(dim * 2 + id64)
  rows = [3001, 5003, 1009, 4099]
  combs = ['sum', 'mean', 'sqrtn', 'sum']
  n = len(rows)
  idt = np.int64 if id64 else np.int32
  # 0: one id per sample with a bucket; 1: ragged mean, divisor 2, some ids out of range;
  # 2: ragged sqrtn weighted; 3: one id per sample, Zipf, weighted
  splits = [None, ragged(rng, 700), ragged(rng, 500), None]
  ids = [rng.randint(0, 1 << 30, size=1500).astype(idt),
         rng.randint(-50, 2 * rows[1] + 400, size=int(splits[1][-1])).astype(idt),
         rng.randint(0, rows[2], size=int(splits[2][-1])).astype(idt),
         ((rng.zipf(1.3, size=1200) * 13) % rows[3]).astype(idt)]
  weights = [None, None, rng.uniform(-1, 2, size=ids[2].size).astype(F32),
             rng.uniform(0.5, 2, size=ids[3].size).astype(F32)]
  host = [state(rng, rows[c], dim) for c in range(n)]
  tables = [dev(h[0]) for h in host]
  moms = [(dev(h[1]), dev(h[2])) for h in host]
  lk = GroupLookup(tables, buckets=[rows[0], 0, 0, 0], combiners=combs, divisor=1)
  lk2 = GroupLookup(tables[1:2], combiners='mean', divisor=2)
  adam = LazyAdam(device=DEV)
  p0 = (F32(B1 ** 3), F32(B2 ** 3))
  adam.beta_powers.copy_(torch.tensor(p0, dtype=torch.float32))
  d_ids = [dev(i) for i in ids]
  d_sp = [None if s is None else dev(s) for s in splits]
  d_w = [None if w is None else dev(w) for w in weights]
  grads = [dev(rng.randn(ids[c].size if splits[c] is None else splits[c].size - 1, dim).astype(F32))
           for c in range(n)]
  lr = 0.05
  # column 1 uses divisor 2: its own object, with the same optimizer (finish=False: one step)
  g_main = GroupLookupGrad(lk, moments=[moms[0], (dev(np.zeros((rows[1], dim), F32)),
                                                   dev(np.zeros((rows[1], dim), F32))), moms[2], moms[3]],
                           adam=adam)
  g_div = GroupLookupGrad(lk2, moments=[moms[1]], adam=adam)
  res_div = g_div([d_ids[1]], [grads[1]], [d_sp[1]], apply_lr=lr, optimizer='adam', finish=False)
  # column 1 of the main object is an empty batch (nothing stepped, nothing emitted)
  empty = torch.zeros(0, dtype=d_ids[0].dtype, device=DEV)
  res = g_main([d_ids[0], empty, d_ids[2], d_ids[3]],
               [grads[0], torch.zeros((0, dim), dtype=torch.float32, device=DEV), grads[2], grads[3]],
               [None, None, d_sp[2], None], apply_lr=lr, optimizer='adam',
               sp_weights=[None, None, d_w[2], d_w[3]])
  torch.cuda.synchronize()
  assert int(res[1][2].item()) == 0
  res = [res[0], res_div[0], res[2], res[3]]
  for c, bucket, div in ((0, rows[0], 1), (1, 0, 2), (2, 0, 1), (3, 0, 1)):
    u, _ = emitted(res[c])
    np.testing.assert_array_equal(np.sort(u), valid_rows(ids[c], rows[c], bucket, div))
  check_one_step(tables, moms, res, host, lr, p0, adam.beta_powers)


def test_dim_the_backward_refuses_is_refused():
  rows, dim = 64, 1024
  lk = GroupLookup([dev(np.zeros((rows, dim), F32))])
  grad = GroupLookupGrad(lk, moments=[(dev(np.zeros((rows, dim), F32)), dev(np.zeros((rows, dim), F32)))])
  with pytest.raises(_lib.InvalidArgumentError, match='64 lanes'):
    grad([dev(np.arange(8, dtype=np.int64))], [dev(np.ones((8, dim), F32))], apply_lr=0.1,
         optimizer='adam')


# ---- 2. each row stepped exactly once ---------------------------------------------------------------
@pytest.mark.parametrize('hook', [None, 'one_bucket'])
def test_each_row_stepped_exactly_once(hbk_option, hook):
  if hook:
    hbk_option('bwd_buckets_log2', 0)     # one bucket: far more distinct rows than the LDS table
  rng = np.random.RandomState(7)
  dim = 16
  # column 0: Zipf (hot rows: split buckets); columns 1, 2: many distinct rows per bucket (several
  # passes over a bucket); columns 3..71: more than one launch group and more than one apply launch
  rows = [100003, 4000, 10000] + [2003] * 69
  n = len(rows)
  ids = [((rng.zipf(1.1, size=200000) * 7) % rows[0]).astype(np.int64),
         rng.randint(0, rows[1], size=20000).astype(np.int64),
         rng.randint(0, rows[2], size=3000).astype(np.int64)] + \
        [rng.randint(0, rows[c], size=int(rng.randint(1, 3000))).astype(np.int64) for c in range(3, n)]
  host = [state(rng, rows[c], dim) for c in range(n)]
  tables = [dev(h[0]) for h in host]
  moms = [(dev(h[1]), dev(h[2])) for h in host]
  adam = LazyAdam(device=DEV)
  grad = GroupLookupGrad(GroupLookup(tables), moments=moms, adam=adam)
  grads = [dev(rng.randn(i.size, dim).astype(F32)) for i in ids]
  res = grad([dev(i) for i in ids], grads, apply_lr=0.01, optimizer='adam')
  torch.cuda.synchronize()
  for c in range(n):
    u, _ = emitted(res[c])
    np.testing.assert_array_equal(np.sort(u), np.unique(ids[c]))
  check_one_step(tables, moms, res, host, 0.01, (B1, B2), adam.beta_powers)


# ---- 3. deterministic across steps ------------------------------------------------------------------
def test_deterministic_steps_equal_numpy_and_step_only_equals_emit():
  rng = np.random.RandomState(11)
  rows, dim, steps, lr = [20011, 3001], [16, 5], 5, 0.02
  n = len(rows)
  host = [state(rng, rows[c], dim[c]) for c in range(n)]
  runs = []
  for emit in (True, False):
    tables = [dev(h[0]) for h in host]
    moms = [(dev(h[1]), dev(h[2])) for h in host]
    adam = LazyAdam(device=DEV)
    grad = GroupLookupGrad(GroupLookup(tables), moments=moms, adam=adam, deterministic=True)
    runs.append((tables, moms, adam, grad, emit))
  ref = [[x.copy() for x in h] for h in host]
  p = (B1, B2)
  for step in range(steps):
    srng = np.random.RandomState(100 + step)
    ids = [((srng.zipf(1.2, size=4000) * 31) % rows[c]).astype(np.int64) for c in range(n)]
    gs = [srng.randn(4000, dim[c]).astype(F32) for c in range(n)]
    for tables, moms, adam, grad, emit in runs:
      grad([dev(i) for i in ids], [dev(g) for g in gs], apply_lr=lr, optimizer='adam', emit=emit)
    for c in range(n):
      uniq = np.unique(ids[c])
      sums = oracle.unsorted_segment_sum(gs[c], np.searchsorted(uniq, ids[c]).astype(np.int32), uniq.size)
      pc = np_adam(ref[c][0], ref[c][1], ref[c][2], uniq, sums, lr, p[0], p[1])
    p = pc
  torch.cuda.synchronize()
  for tables, moms, adam, _, emit in runs:
    for c in range(n):
      np.testing.assert_array_equal(tables[c].cpu().numpy(), ref[c][0], err_msg=f'w {c} emit={emit}')
      np.testing.assert_array_equal(moms[c][0].cpu().numpy(), ref[c][1], err_msg=f'm {c} emit={emit}')
      np.testing.assert_array_equal(moms[c][1].cpu().numpy(), ref[c][2], err_msg=f'v {c} emit={emit}')
    np.testing.assert_array_equal(adam.beta_powers.cpu().numpy(), np.array(p, F32))


# ---- 4. interleaved [w | m | v | pad] rows -----------------------------------------------------------
@pytest.mark.parametrize('dim', [16, 3])
def test_interleaved_row_pitch_equals_separate_tensors(dim):
  rng = np.random.RandomState(dim)
  rows, lr = 50021, 0.03
  w, m, v = state(rng, rows, dim)
  ids = rng.randint(0, rows, size=8192).astype(np.int64)
  g = rng.randn(ids.size, dim).astype(F32)
  tables, moms = [dev(w)], [(dev(m), dev(v))]
  adam = LazyAdam(device=DEV)
  grad = GroupLookupGrad(GroupLookup(tables), moments=moms, adam=adam, deterministic=True)
  grad([dev(ids)], [dev(g)], apply_lr=lr, optimizer='adam')
  # the same step at the C ABI on one [rows, 4 dim] buffer: w, m, v side by side, table_pitch = 4 dim
  buf = dev(np.concatenate([w, m, v, np.zeros_like(w)], axis=1))
  adam2 = LazyAdam(device=DEV)
  cols = type(grad._cols).from_buffer_copy(grad._cols)
  cols[0].table, cols[0].table_pitch = buf.data_ptr(), 4 * dim
  cols[0].unique_rows, cols[0].grad_rows = None, None          # step only
  n_unique = torch.zeros(1, dtype=torch.int32, device=DEV)
  cols[0].n_unique = n_unique.data_ptr()
  lib = _lib.lib()
  need = lib.hbk_group_lookup_bwd_adam_workspace_bytes(1, cols)
  ws = torch.empty(need, dtype=torch.uint8, device=DEV)
  _lib.check(lib.hbk_group_lookup_bwd_adam(
    1, cols, _lib.ptr_array([buf.data_ptr() + 4 * dim]), _lib.ptr_array([buf.data_ptr() + 8 * dim]),
    C.byref(adam2.params()), C.c_float(lr), C.c_void_p(ws.data_ptr()), C.c_size_t(need),
    _lib.current_stream(DEV)))
  torch.cuda.synchronize()
  out = buf.cpu().numpy()
  np.testing.assert_array_equal(out[:, :dim], tables[0].cpu().numpy())
  np.testing.assert_array_equal(out[:, dim:2 * dim], moms[0][0].cpu().numpy())
  np.testing.assert_array_equal(out[:, 2 * dim:3 * dim], moms[0][1].cpu().numpy())
  np.testing.assert_array_equal(out[:, 3 * dim:], 0)
  assert int(n_unique.item()) == np.unique(ids).size
  np.testing.assert_array_equal(adam2.beta_powers.cpu().numpy(), adam.beta_powers.cpu().numpy())


# ---- 5. captured graph replay and launch() ---------------------------------------------------------------
def test_graph_replay_and_launch_equal_eager_steps():
  rng = np.random.RandomState(5)
  rows, dim, K, lr = 10007, 16, 4, 0.05
  w, m, v = state(rng, rows, dim)
  sp = ragged(rng, 600)
  ids = rng.randint(0, rows, size=int(sp[-1])).astype(np.int64)
  g = rng.randn(sp.size - 1, dim).astype(F32)
  d_ids, d_sp, d_g = dev(ids), dev(sp), dev(g)

  def make():
    tables, moms = [dev(w)], [(dev(m), dev(v))]
    adam = LazyAdam(device=DEV)
    grad = GroupLookupGrad(GroupLookup(tables, combiners='mean'), moments=moms, adam=adam,
                           deterministic=True)
    return tables, moms, adam, grad

  def result(x):
    tables, moms, adam, _ = x
    return [tables[0].cpu().numpy(), moms[0][0].cpu().numpy(), moms[0][1].cpu().numpy(),
            adam.beta_powers.cpu().numpy()]

  eager = make()
  for _ in range(K):
    eager[3]([d_ids], [d_g], [d_sp], apply_lr=lr, optimizer='adam')
  launched = make()
  launched[3]([d_ids], [d_g], [d_sp], apply_lr=lr, optimizer='adam')
  for _ in range(K - 1):
    launched[3].launch(lr, optimizer='adam')
  graphed = make()
  graphed[3]([d_ids], [d_g], [d_sp], apply_lr=lr, optimizer='adam')   # binds; step 1
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      graphed[3].launch(lr, optimizer='adam')
  torch.cuda.synchronize()
  for _ in range(K - 1):
    graph.replay()
  torch.cuda.synchronize()
  want = result(eager)
  for other in (launched, graphed):
    for a, b in zip(result(other), want):
      np.testing.assert_array_equal(a, b)
  p = (B1, B2)
  for _ in range(K):
    p = (F32(p[0] * B1), F32(p[1] * B2))
  np.testing.assert_array_equal(want[3], np.array(p, F32))


# ---- 6. sharded ------------------------------------------------------------------------------------------
def _sharded_case(rng, world):
  dims, rows = [16, 8, 3], [4099, 1013, 2003]
  n = len(dims)
  host = [state(rng, rows[c], dims[c]) for c in range(n)]
  ids = [[rng.randint(0, 1 << 30, size=int(rng.randint(100, 1500))).astype(np.int64) for c in range(n)]
         for _ in range(world)]
  # gradients on a 1/16 grid with small magnitudes: every sum is exact in fp32, whatever its order
  grads = [[(rng.randint(-64, 65, size=(i.size, dims[c])) / 16.0).astype(F32) for c, i in enumerate(r)]
           for r in ids]
  return dims, rows, host, ids, grads


def _single_gpu_adam(rows, host, ids, grads, lr, emit):
  """The unsharded step on the logical tables: every rank's ids and gradients as one batch."""
  n = len(rows)
  tables = [dev(h[0]) for h in host]
  moms = [(dev(h[1]), dev(h[2])) for h in host]
  adam = LazyAdam(device=DEV)
  grad = GroupLookupGrad(GroupLookup(tables, buckets=rows), moments=moms, adam=adam, deterministic=True)
  cat_ids = [np.concatenate([r[c] for r in ids]) for c in range(n)]
  cat_g = [np.concatenate([r[c] for r in grads]) for c in range(n)]
  grad([dev(i) for i in cat_ids], [dev(g) for g in cat_g], apply_lr=lr, optimizer='adam', emit=emit)
  torch.cuda.synchronize()
  return ([t.cpu().numpy() for t in tables], [m.cpu().numpy() for m, _ in moms],
          [v.cpu().numpy() for _, v in moms], adam.beta_powers.cpu().numpy())


def _run_world(comms, world, dims, rows, host, ids, grads, lr, emit):
  n = len(dims)
  shards = [[[dev(x[r::world].copy()) for x in host[c]] for c in range(n)] for r in range(world)]
  errors, fwd = [], [None] * world
  adams = [LazyAdam(device=DEV) for _ in range(world)]

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        drv = ShardedGroupLookup([s[0] for s in shards[r]], comms[r], buckets=rows,
                                 moments=[(s[1], s[2]) for s in shards[r]], adam=adams[r])
        outs = drv([dev(i) for i in ids[r]])
        drv.backward([dev(g) for g in grads[r]], apply_lr=lr, optimizer='adam', emit=emit)
        torch.cuda.current_stream().synchronize()
        fwd[r] = [o.cpu().numpy() for o in outs]
        drv.close()
    except Exception as e:  # pylint: disable=broad-except
      errors.append((r, repr(e)))

  threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=120)
  assert not errors, errors
  logical = []
  for k in range(3):
    out = []
    for c in range(n):
      full = np.empty_like(host[c][k])
      for r in range(world):
        full[r::world] = shards[r][c][k].cpu().numpy()
      out.append(full)
    logical.append(out)
  return fwd, logical, [a.beta_powers.cpu().numpy() for a in adams]


@pytest.mark.parametrize('world', [1, 2, 4])
@pytest.mark.parametrize('emit', [True, False])
def test_sharded_equals_single_gpu(hbk_option, world, emit):
  hbk_option('bwd_deterministic', 1)
  rng = np.random.RandomState(300 + world)
  dims, rows, host, ids, grads = _sharded_case(rng, world)
  lr = 0.1
  comms = hb.distribute.Collective.local_world(world)
  fwd, logical, powers = _run_world(comms, world, dims, rows, host, ids, grads, lr, emit)
  for cm in comms:
    cm.close()
  want = _single_gpu_adam(rows, host, ids, grads, lr, emit)
  for r in range(world):
    for c in range(len(dims)):
      np.testing.assert_array_equal(fwd[r][c], host[c][0][ids[r][c] % rows[c]])
  for k in range(3):
    for c in range(len(dims)):
      np.testing.assert_array_equal(logical[k][c], want[k][c], err_msg=f'slot {k} column {c}')
  for p in powers:
    np.testing.assert_array_equal(p, want[3])


def test_sharded_through_rccl_world1():
  rng = np.random.RandomState(399)
  dims, rows, host, ids, grads = _sharded_case(rng, 1)
  coll = hb.distribute.Collective(world_size=1, rank=0)
  try:
    fwd, logical, powers = _run_world([coll], 1, dims, rows, host, ids, grads, 0.1, True)
  finally:
    coll.close()
  want = _single_gpu_adam(rows, host, ids, grads, 0.1, True)
  for k in range(3):
    for c in range(len(dims)):
      np.testing.assert_array_equal(logical[k][c], want[k][c])
  np.testing.assert_array_equal(powers[0], want[3])


# ---- 7. DenseFeatures with Lazy Adam ---------------------------------------------------------------------
def _df_case(world, steps, seed):
  """Columns: 'a' and 'c' sharded at W > 1, 'b' replicated (8 buckets <= batch); one id per sample;
  gradients on a 1/16 grid so every row sum is exact in fp32 whatever its order."""
  rng = np.random.RandomState(seed)
  spec = [('a', 50021, 16, 'sum'), ('b', 8, 8, 'mean'), ('c', 3001, 4, 'sum')]
  cols = [hb.feature_column.EmbeddingColumn(k, nb, d, comb, hot_rows=False) for k, nb, d, comb in spec]
  tables = [rng.uniform(-1, 1, size=(nb, d)).astype(F32) for _, nb, d, _ in spec]
  batch, width = 256, sum(d for _, _, d, _ in spec)
  data = [[({c.key: rng.randint(0, 1 << 40, size=batch).astype(np.int64) for c in cols},
            (rng.randint(-64, 65, size=(batch, width)) / 16.0).astype(F32))
           for _ in range(world)] for _ in range(steps)]
  return cols, tables, batch, data


def _df_reference(cols, tables, data, world, steps, lr):
  """numpy: the logical w, m, v and powers after `steps` steps of every rank's batches; replicated
  tables are not stepped at W > 1."""
  w = [t.copy() for t in tables]
  m = [np.zeros_like(t) for t in tables]
  v = [np.zeros_like(t) for t in tables]
  p = (B1, B2)
  for s in range(steps):
    off = 0
    for k, c in enumerate(cols):
      if world == 1 or c.num_buckets > 256:
        rows = np.concatenate([data[s][r][0][c.key] % c.num_buckets for r in range(world)])
        g = np.concatenate([data[s][r][1][:, off:off + c.dimension] for r in range(world)])
        uniq = np.unique(rows)
        sums = oracle.unsorted_segment_sum(g, np.searchsorted(uniq, rows).astype(np.int32), uniq.size)
        np_adam(w[k], m[k], v[k], uniq, sums, lr, p[0], p[1])
      off += c.dimension
    p = (F32(p[0] * B1), F32(p[1] * B2))
  return w, m, v, np.array(p, F32)


def _df_world(world, fn):
  comms = hb.distribute.Collective.local_world(world) if world > 1 else [None]
  barrier = threading.Barrier(world)
  results, errors = [None] * world, []

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        results[r] = fn(r, comms[r], barrier.wait)
        torch.cuda.current_stream().synchronize()
    except Exception as e:  # pylint: disable=broad-except
      import traceback
      errors.append((r, repr(e), traceback.format_exc()))
      barrier.abort()
  threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=90)
  for cm in comms:
    if cm is not None:
      cm.close()
  assert not errors, errors
  return results


def _df_layer(cols, tables, batch, r, world, coll, fresh=False):
  def init(c, rows, d):
    t = tables[cols.index(c)]
    if fresh:
      return torch.zeros(rows, c.dimension, device=DEV)
    return dev((t[r::world] if rows != c.num_buckets else t).copy())
  return hb.feature_column.DenseFeatures(cols, DEV, coll=coll, batch_size=batch, init=init,
                                         optimizer='adam')


def _df_steps(layer, data, r, steps, lr, first=0):
  for s in range(first, steps):
    feats, g = data[s][r]
    layer({k: dev(x) for k, x in feats.items()})
    layer.backward(dev(g), apply_lr=lr, optimizer='adam', emit=False)


def _df_logical(layer, cols, world, r, results_of_all):
  """(w, m, v) of every column as logical tables, from every rank's layer state."""
  out = []
  for k, c in enumerate(cols):
    trip = []
    for slot in range(3):
      parts = [res[slot][k] for res in results_of_all]
      if world == 1 or not results_of_all[0][3][k]:
        trip.append(parts[0])
      else:
        full = np.empty((c.num_buckets, c.dimension), F32)
        for q in range(world):
          full[q::world] = parts[q]
        trip.append(full)
    out.append(trip)
  return out


def _df_state(layer):
  return ([w.cpu().numpy() for w in layer.weights], [m.cpu().numpy() for m, _ in layer.moments],
          [v.cpu().numpy() for _, v in layer.moments], list(layer.sharded),
          layer.adam.beta_powers.cpu().numpy())


def _df_check(cols, results, world, want):
  logical = _df_logical(None, cols, world, 0, results)
  for k in range(len(cols)):
    for slot in range(3):
      np.testing.assert_array_equal(logical[k][slot], want[slot][k], err_msg=f'column {k} slot {slot}')
  for res in results:
    np.testing.assert_array_equal(res[4], want[3])


@pytest.mark.parametrize('world', [1, 2])
def test_dense_features_adam_steps(world):
  steps, lr = 3, 0.05
  cols, tables, batch, data = _df_case(world, steps, 700 + world)

  def fn(r, coll, barrier):
    layer = _df_layer(cols, tables, batch, r, world, coll)
    assert layer.sharded == [world > 1, False, world > 1]
    _df_steps(layer, data, r, steps, lr)
    st = _df_state(layer)
    layer.close()
    return st
  results = _df_world(world, fn)
  want = _df_reference(cols, tables, data, world, steps, lr)
  _df_check(cols, results, world, want)
  if world > 1:   # the replicated table: not stepped, its slots untouched
    for res in results:
      np.testing.assert_array_equal(res[0][1], tables[1])
      np.testing.assert_array_equal(res[1][1], 0)


def test_dense_features_adam_checkpoint_across_world_sizes(tmp_path):
  import json
  steps, lr = 3, 0.05
  cols, tables, batch, data = _df_case(2, steps, 801)
  prefix = str(tmp_path / 'w2.ckpt')

  def train_save(r, coll, barrier):   # W = 2: two steps, save, then keep going (the run that never stopped)
    layer = _df_layer(cols, tables, batch, r, 2, coll)
    _df_steps(layer, data, r, 2, lr)
    layer.save(prefix, barrier=barrier)
    _df_steps(layer, data, r, steps, lr, first=2)
    st = _df_state(layer)
    layer.close()
    return st
  unbroken = _df_world(2, train_save)
  _df_check(cols, unbroken, 2, _df_reference(cols, tables, data, 2, steps, lr))
  with open(prefix + '.index') as f:
    names = set(json.load(f)['variables'])
  for c in cols:
    for suffix in ('', '/Adam', '/Adam_1'):
      assert f'{c.key}_embedding/embedding_weights{suffix}' in names
  assert {'beta1_power', 'beta2_power'} <= names

  def restore_continue(r, coll, barrier):   # a fresh W = 2 layer: restore, the third step
    layer = _df_layer(cols, tables, batch, r, 2, coll, fresh=True)
    layer.restore(prefix, barrier=barrier)
    _df_steps(layer, data, r, steps, lr, first=2)
    st = _df_state(layer)
    layer.close()
    return st
  resumed = _df_world(2, restore_continue)
  for a, b in zip(resumed, unbroken):
    for x, y in zip(a[:3], b[:3]):
      for xx, yy in zip(x, y):
        np.testing.assert_array_equal(xx, yy)
    np.testing.assert_array_equal(a[4], b[4])

  # the W = 2 checkpoint at W = 1: every logical row of w, m, v and both powers
  after2 = _df_reference(cols, tables, data, 2, 2, lr)

  def restore_only(world):
    def fn(r, coll, barrier):
      layer = _df_layer(cols, tables, batch, r, world, coll, fresh=True)
      layer.restore(prefix if world == 1 else prefix1, barrier=barrier)
      st = _df_state(layer)
      layer.close()
      return st
    return fn
  prefix1 = None
  at1 = _df_world(1, restore_only(1))
  _df_check(cols, at1, 1, after2)

  # a W = 1 checkpoint at W = 2
  prefix1 = str(tmp_path / 'w1.ckpt')
  data1 = [[(feats, g)] for (feats, g), _ in data[:2]]

  def train_save1(r, coll, barrier):
    layer = _df_layer(cols, tables, batch, r, 1, coll)
    _df_steps(layer, data1, r, 2, lr)
    layer.save(prefix1, barrier=barrier)
    st = _df_state(layer)
    layer.close()
    return st
  w1 = _df_world(1, train_save1)
  at2 = _df_world(2, restore_only(2))
  want = (w1[0][0], w1[0][1], w1[0][2], w1[0][4])
  _df_check(cols, at2, 2, want)
