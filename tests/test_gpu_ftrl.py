"""FTRL-Proximal (TF 1.15 SparseApplyFtrl / SparseApplyFtrlV2, the sparse apply of
tf.train.FtrlOptimizer) on the GPU: one step bit-equal to a numpy fp32 restatement applied to the
call's own IndexedSlices for lr_power -0.5 and 0, the powf form within a few ulps of a float64
restatement, every distinct row stepped exactly once, deterministic multi-step runs, the interleaved
[w|accum|linear|pad] row pitch, captured-graph replay, the sharded driver against the single-GPU step,
DenseFeatures with checkpoints across world sizes, and the reference project's own configuration
against its closed form."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import oracle
import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import Ftrl, GroupLookup, GroupLookupGrad
from hybridbackend_amd.embedding.sharded import ShardedGroupLookup

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- numpy fp32 restatement of the step (every op a separately rounded fp32 op, in this order) ------
def np_ftrl(w, a, z, rows, g, lr, ftrl):
  lr, l1, l2 = F32(lr), F32(ftrl.l1), F32(ftrl.l2)
  shrink, lrp = F32(ftrl.l2_shrinkage), F32(ftrl.lr_power)
  g = g.astype(F32)
  wr, ar, zr = w[rows], a[rows], z[rows]
  gs = g if shrink == 0 else g + (F32(2) * shrink) * wr
  na = ar + g * g
  if lrp == F32(-0.5):
    pn, po = np.sqrt(na), np.sqrt(ar)
  else:
    pn, po = np.power(na, -lrp), np.power(ar, -lrp)
  zn = zr + (gs - ((pn - po) / lr) * wr)
  y = pn / lr + F32(2) * l2
  w[rows] = (np.maximum(np.minimum(zn, l1), -l1) - zn) / y
  a[rows] = na
  z[rows] = zn


def f64_ftrl(w, a, z, rows, g, lr, ftrl):
  """The same step in float64 from the same fp32 inputs; returns the magnitude of the terms that
  make up each new z (the scale its fp32 rounding errors are relative to) and y."""
  w, a, z, g = (x.astype(np.float64) for x in (w[rows], a[rows], z[rows], g))
  lr, lrp = float(F32(lr)), float(F32(ftrl.lr_power))
  shrink = float(F32(ftrl.l2_shrinkage))
  gs = g if shrink == 0 else g + 2 * shrink * w
  na = a + g * g
  pn, po = na ** -lrp, a ** -lrp
  zn = z + (gs - (pn - po) / lr * w)
  y = pn / lr + 2 * float(F32(ftrl.l2))
  l1 = float(F32(ftrl.l1))
  wn = (np.clip(zn, -l1, l1) - zn) / y
  # (p(na) and p(a) each carry an error relative to themselves, not to their difference)
  return wn, na, zn, np.abs(z) + np.abs(gs) + (pn + po) / lr * np.abs(w), y


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
  a = rng.uniform(0.1, 1, size=(rows, dim)).astype(F32)
  z = rng.uniform(-4, 4, size=(rows, dim)).astype(F32)
  return w, a, z


def check_one_step(tables, slots, res, host, lr, ftrl):
  """w, accum, linear after ONE emit-mode step == numpy on the call's own slices; rows absent from
  the batch bit-unchanged."""
  zeros = 0
  for c in range(len(tables)):
    u, g = emitted(res[c])
    assert np.unique(u).size == u.size, f'column {c}: a row emitted twice'
    w, a, z = (x.copy() for x in host[c])
    np_ftrl(w, a, z, u, g, lr, ftrl)
    got = (tables[c].cpu().numpy(), slots[c][0].cpu().numpy(), slots[c][1].cpu().numpy())
    for name, x, want in zip(('w', 'accum', 'linear'), got, (w, a, z)):
      np.testing.assert_array_equal(x, want, err_msg=f'{name} of column {c}')
    absent = np.ones(w.shape[0], bool)
    absent[u] = False
    for x, h in zip(got, host[c]):
      np.testing.assert_array_equal(x[absent], h[absent])
    zeros += int((got[0][u] == 0).sum())
  return zeros


CONFIGS = {   # (l1, l2, l2_shrinkage, lr_power)
  'default': Ftrl(),
  'l1_l2': Ftrl(l1=2.0, l2=1e-5),
  'shrinkage': Ftrl(l2=1e-5, l2_shrinkage=0.01),
  'l1_shrinkage_pow0': Ftrl(l1=2.0, l2_shrinkage=0.01, lr_power=0.0),
}


# ---- 1. one step against the slices it emitted ----------------------------------------------------
@pytest.mark.parametrize('config', sorted(CONFIGS))
@pytest.mark.parametrize('dim', [1, 3, 4, 8, 16, 64, 128, 256])
@pytest.mark.parametrize('id64', [False, True])
def test_one_step_bit_equal_to_its_own_slices(config, dim, id64):
  ftrl = CONFIGS[config]
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
  slots = [(dev(h[1]), dev(h[2])) for h in host]
  lk = GroupLookup(tables, buckets=[rows[0], 0, 0, 0], combiners=combs, divisor=1)
  lk2 = GroupLookup(tables[1:2], combiners='mean', divisor=2)
  d_ids = [dev(i) for i in ids]
  d_sp = [None if s is None else dev(s) for s in splits]
  d_w = [None if w is None else dev(w) for w in weights]
  grads = [dev(rng.randn(ids[c].size if splits[c] is None else splits[c].size - 1, dim).astype(F32))
           for c in range(n)]
  lr = 0.05
  # column 1 uses divisor 2: its own object
  g_main = GroupLookupGrad(lk, ftrl_slots=[slots[0], ftrl.slots_like(tables[1]), slots[2], slots[3]],
                           ftrl=ftrl)
  g_div = GroupLookupGrad(lk2, ftrl_slots=[slots[1]], ftrl=ftrl)
  res_div = g_div([d_ids[1]], [grads[1]], [d_sp[1]], apply_lr=lr, optimizer='ftrl')
  # column 1 of the main object is an empty batch (nothing stepped, nothing emitted)
  empty = torch.zeros(0, dtype=d_ids[0].dtype, device=DEV)
  res = g_main([d_ids[0], empty, d_ids[2], d_ids[3]],
               [grads[0], torch.zeros((0, dim), dtype=torch.float32, device=DEV), grads[2], grads[3]],
               [None, None, d_sp[2], None], apply_lr=lr, optimizer='ftrl',
               sp_weights=[None, None, d_w[2], d_w[3]])
  torch.cuda.synchronize()
  assert int(res[1][2].item()) == 0
  res = [res[0], res_div[0], res[2], res[3]]
  for c, bucket, div in ((0, rows[0], 1), (1, 0, 2), (2, 0, 1), (3, 0, 1)):
    u, _ = emitted(res[c])
    np.testing.assert_array_equal(np.sort(u), valid_rows(ids[c], rows[c], bucket, div))
  zeros = check_one_step(tables, slots, res, host, lr, ftrl)
  if ftrl.l1 > 0:
    assert zeros > 0, 'l1 = 2 should clip some stepped weights to exactly 0'


@pytest.mark.parametrize('lr_power', [-0.3, -1.0])
@pytest.mark.parametrize('dim', [3, 16])
def test_powf_form_within_a_few_ulps_of_float64(lr_power, dim):
  """lr_power not in {-0.5, 0}: powf is not correctly rounded, so w and linear are held to a bound --
  K fp32 ulps of the magnitude of the terms that make up each value -- and accum to its bits."""
  K = 8
  ftrl = Ftrl(l2=1e-5, l2_shrinkage=0.01, lr_power=lr_power)
  rng = np.random.RandomState(int(-lr_power * 10) + dim)
  rows = 20011
  w, a, z = state(rng, rows, dim)
  ids = ((rng.zipf(1.2, size=6000) * 7) % rows).astype(np.int64)
  g = rng.randn(ids.size, dim).astype(F32)
  tables, slots = [dev(w)], [(dev(a), dev(z))]
  grad = GroupLookupGrad(GroupLookup(tables), ftrl_slots=slots, ftrl=ftrl)
  res = grad([dev(ids)], [dev(g)], apply_lr=0.07, optimizer='ftrl')
  torch.cuda.synchronize()
  u, gr = emitted(res[0])
  want_w, want_a, want_z, zscale, y = f64_ftrl(w, a, z, u, gr, 0.07, ftrl)
  got_w, got_a, got_z = (x.cpu().numpy() for x in (tables[0], slots[0][0], slots[0][1]))
  aa = a.copy()
  aa[u] = a[u] + gr * gr                                   # accum: one fp32 add, bit-equal
  np.testing.assert_array_equal(got_a, aa)
  err_z = np.abs(got_z[u] - want_z) / (EPS32 * zscale)
  err_w = np.abs(got_w[u] - want_w) / (EPS32 * (np.abs(want_w) + zscale / y))
  print(f'lr_power {lr_power} dim {dim}: largest error {err_z.max():.2f} ulps (linear), '
        f'{err_w.max():.2f} ulps (w)')
  assert err_z.max() <= K and err_w.max() <= K, (err_z.max(), err_w.max())
  absent = np.ones(rows, bool)
  absent[u] = False
  for got, h in ((got_w, w), (got_a, a), (got_z, z)):
    np.testing.assert_array_equal(got[absent], h[absent])


def test_dim_the_backward_refuses_is_refused():
  rows, dim = 64, 1024
  lk = GroupLookup([dev(np.zeros((rows, dim), F32))])
  grad = GroupLookupGrad(lk, ftrl_slots=[Ftrl().slots_like(lk.tables[0])])
  with pytest.raises(_lib.InvalidArgumentError, match='64 lanes'):
    grad([dev(np.arange(8, dtype=np.int64))], [dev(np.ones((8, dim), F32))], apply_lr=0.1,
         optimizer='ftrl')


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
  slots = [(dev(h[1]), dev(h[2])) for h in host]
  ftrl = Ftrl(l1=0.5, l2=1e-5)
  grad = GroupLookupGrad(GroupLookup(tables), ftrl_slots=slots, ftrl=ftrl)
  grads = [dev(rng.randn(i.size, dim).astype(F32)) for i in ids]
  res = grad([dev(i) for i in ids], grads, apply_lr=0.01, optimizer='ftrl')
  torch.cuda.synchronize()
  for c in range(n):
    u, _ = emitted(res[c])
    np.testing.assert_array_equal(np.sort(u), np.unique(ids[c]))
  check_one_step(tables, slots, res, host, 0.01, ftrl)


# ---- 3. deterministic across steps ------------------------------------------------------------------
def test_deterministic_steps_equal_numpy_and_step_only_equals_emit(hbk_option):
  hbk_option('bwd_deterministic', 1)
  rng = np.random.RandomState(11)
  rows, dim, steps, lr = [20011, 3001], [16, 5], 5, 0.02
  ftrl = Ftrl(l1=2.0, l2=1e-5, l2_shrinkage=0.01)
  n = len(rows)
  host = [state(rng, rows[c], dim[c]) for c in range(n)]
  runs = []
  for emit in (True, True, False):   # emit twice: two runs of the same steps give the same bits
    tables = [dev(h[0]) for h in host]
    slots = [(dev(h[1]), dev(h[2])) for h in host]
    grad = GroupLookupGrad(GroupLookup(tables), ftrl_slots=slots, ftrl=ftrl)
    runs.append((tables, slots, grad, emit))
  ref = [[x.copy() for x in h] for h in host]
  for step in range(steps):
    srng = np.random.RandomState(100 + step)
    ids = [((srng.zipf(1.2, size=4000) * 31) % rows[c]).astype(np.int64) for c in range(n)]
    gs = [srng.randn(4000, dim[c]).astype(F32) for c in range(n)]
    for tables, slots, grad, emit in runs:
      grad([dev(i) for i in ids], [dev(g) for g in gs], apply_lr=lr, optimizer='ftrl', emit=emit)
    for c in range(n):
      uniq = np.unique(ids[c])
      sums = oracle.unsorted_segment_sum(gs[c], np.searchsorted(uniq, ids[c]).astype(np.int32), uniq.size)
      np_ftrl(ref[c][0], ref[c][1], ref[c][2], uniq, sums, lr, ftrl)
  torch.cuda.synchronize()
  for k, (tables, slots, _, emit) in enumerate(runs):
    for c in range(n):
      np.testing.assert_array_equal(tables[c].cpu().numpy(), ref[c][0], err_msg=f'w {c} run {k}')
      np.testing.assert_array_equal(slots[c][0].cpu().numpy(), ref[c][1], err_msg=f'accum {c} run {k}')
      np.testing.assert_array_equal(slots[c][1].cpu().numpy(), ref[c][2], err_msg=f'linear {c} run {k}')


# ---- 4. interleaved [w | accum | linear | pad] rows ------------------------------------------------
@pytest.mark.parametrize('lr_power', [-0.5, -0.3])
@pytest.mark.parametrize('dim', [16, 3])
def test_interleaved_row_pitch_equals_separate_tensors(dim, lr_power):
  rng = np.random.RandomState(dim)
  rows, lr = 50021, 0.03
  ftrl = Ftrl(l1=2.0, l2=1e-5, lr_power=lr_power)
  w, a, z = state(rng, rows, dim)
  ids = rng.randint(0, rows, size=8192).astype(np.int64)
  g = rng.randn(ids.size, dim).astype(F32)
  tables, slots = [dev(w)], [(dev(a), dev(z))]
  grad = GroupLookupGrad(GroupLookup(tables), ftrl_slots=slots, ftrl=ftrl, deterministic=True)
  grad([dev(ids)], [dev(g)], apply_lr=lr, optimizer='ftrl')
  # the same step at the C ABI on one [rows, 4 dim] buffer: w, accum, linear side by side
  buf = dev(np.concatenate([w, a, z, np.zeros_like(w)], axis=1))
  cols = type(grad._cols).from_buffer_copy(grad._cols)
  cols[0].table, cols[0].table_pitch = buf.data_ptr(), 4 * dim
  cols[0].unique_rows, cols[0].grad_rows = None, None          # step only
  n_unique = torch.zeros(1, dtype=torch.int32, device=DEV)
  cols[0].n_unique = n_unique.data_ptr()
  lib = _lib.lib()
  need = lib.hbk_group_lookup_bwd_ftrl_workspace_bytes(1, cols)
  ws = torch.empty(need, dtype=torch.uint8, device=DEV)
  _lib.check(lib.hbk_group_lookup_bwd_ftrl(
    1, cols, _lib.ptr_array([buf.data_ptr() + 4 * dim]), _lib.ptr_array([buf.data_ptr() + 8 * dim]),
    C.byref(ftrl.params()), C.c_float(lr), C.c_void_p(ws.data_ptr()), C.c_size_t(need),
    _lib.current_stream(DEV)))
  torch.cuda.synchronize()
  out = buf.cpu().numpy()
  np.testing.assert_array_equal(out[:, :dim], tables[0].cpu().numpy())
  np.testing.assert_array_equal(out[:, dim:2 * dim], slots[0][0].cpu().numpy())
  np.testing.assert_array_equal(out[:, 2 * dim:3 * dim], slots[0][1].cpu().numpy())
  np.testing.assert_array_equal(out[:, 3 * dim:], 0)
  assert int(n_unique.item()) == np.unique(ids).size


# ---- 5. captured graph replay and launch() ---------------------------------------------------------------
def test_graph_replay_and_launch_equal_eager_steps():
  rng = np.random.RandomState(5)
  rows, dim, K, lr = 10007, 16, 4, 0.05
  ftrl = Ftrl(l1=2.0, l2=1e-5, l2_shrinkage=0.01)
  w, a, z = state(rng, rows, dim)
  sp = ragged(rng, 600)
  ids = rng.randint(0, rows, size=int(sp[-1])).astype(np.int64)
  g = rng.randn(sp.size - 1, dim).astype(F32)
  d_ids, d_sp, d_g = dev(ids), dev(sp), dev(g)

  def make():
    tables, slots = [dev(w)], [(dev(a), dev(z))]
    grad = GroupLookupGrad(GroupLookup(tables, combiners='mean'), ftrl_slots=slots, ftrl=ftrl,
                           deterministic=True)
    return tables, slots, grad

  def result(x):
    tables, slots, _ = x
    return [tables[0].cpu().numpy(), slots[0][0].cpu().numpy(), slots[0][1].cpu().numpy()]

  eager = make()
  for _ in range(K):
    eager[2]([d_ids], [d_g], [d_sp], apply_lr=lr, optimizer='ftrl')
  launched = make()
  launched[2]([d_ids], [d_g], [d_sp], apply_lr=lr, optimizer='ftrl')
  for _ in range(K - 1):
    launched[2].launch(lr, optimizer='ftrl')
  graphed = make()
  graphed[2]([d_ids], [d_g], [d_sp], apply_lr=lr, optimizer='ftrl')   # binds; step 1
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      graphed[2].launch(lr, optimizer='ftrl')
  torch.cuda.synchronize()
  for _ in range(K - 1):
    graph.replay()
  torch.cuda.synchronize()
  want = result(eager)
  for other in (launched, graphed):
    for x, y in zip(result(other), want):
      np.testing.assert_array_equal(x, y)
  assert not np.array_equal(want[2], z)   # (the steps did step)


# ---- 6. sharded ------------------------------------------------------------------------------------------
SHARDED_FTRL = Ftrl(l1=2.0, l2=1e-5, l2_shrinkage=0.01)


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


def _single_gpu_ftrl(rows, host, ids, grads, lr, emit):
  """The unsharded step on the logical tables: every rank's ids and gradients as one batch."""
  n = len(rows)
  tables = [dev(h[0]) for h in host]
  slots = [(dev(h[1]), dev(h[2])) for h in host]
  grad = GroupLookupGrad(GroupLookup(tables, buckets=rows), ftrl_slots=slots, ftrl=SHARDED_FTRL,
                         deterministic=True)
  cat_ids = [np.concatenate([r[c] for r in ids]) for c in range(n)]
  cat_g = [np.concatenate([r[c] for r in grads]) for c in range(n)]
  grad([dev(i) for i in cat_ids], [dev(g) for g in cat_g], apply_lr=lr, optimizer='ftrl', emit=emit)
  torch.cuda.synchronize()
  return ([t.cpu().numpy() for t in tables], [a.cpu().numpy() for a, _ in slots],
          [z.cpu().numpy() for _, z in slots])


def _run_world(comms, world, dims, rows, host, ids, grads, lr, emit):
  n = len(dims)
  shards = [[[dev(x[r::world].copy()) for x in host[c]] for c in range(n)] for r in range(world)]
  errors, fwd = [], [None] * world

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        drv = ShardedGroupLookup([s[0] for s in shards[r]], comms[r], buckets=rows,
                                 ftrl_slots=[(s[1], s[2]) for s in shards[r]], ftrl=SHARDED_FTRL)
        outs = drv([dev(i) for i in ids[r]])
        drv.backward([dev(g) for g in grads[r]], apply_lr=lr, optimizer='ftrl', emit=emit)
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
  return fwd, logical


@pytest.mark.parametrize('world', [1, 2, 4])
@pytest.mark.parametrize('emit', [True, False])
def test_sharded_equals_single_gpu(hbk_option, world, emit):
  hbk_option('bwd_deterministic', 1)
  rng = np.random.RandomState(300 + world)
  dims, rows, host, ids, grads = _sharded_case(rng, world)
  lr = 0.1
  comms = hb.distribute.Collective.local_world(world)
  fwd, logical = _run_world(comms, world, dims, rows, host, ids, grads, lr, emit)
  for cm in comms:
    cm.close()
  want = _single_gpu_ftrl(rows, host, ids, grads, lr, emit)
  for r in range(world):
    for c in range(len(dims)):
      np.testing.assert_array_equal(fwd[r][c], host[c][0][ids[r][c] % rows[c]])
  for k in range(3):
    for c in range(len(dims)):
      np.testing.assert_array_equal(logical[k][c], want[k][c], err_msg=f'slot {k} column {c}')


def test_sharded_through_rccl_world1():
  rng = np.random.RandomState(399)
  dims, rows, host, ids, grads = _sharded_case(rng, 1)
  coll = hb.distribute.Collective(world_size=1, rank=0)
  try:
    _, logical = _run_world([coll], 1, dims, rows, host, ids, grads, 0.1, True)
  finally:
    coll.close()
  want = _single_gpu_ftrl(rows, host, ids, grads, 0.1, True)
  for k in range(3):
    for c in range(len(dims)):
      np.testing.assert_array_equal(logical[k][c], want[k][c])


# ---- 7. DenseFeatures with FTRL ----------------------------------------------------------------------
DF_FTRL = Ftrl(l1=0.5, l2=1e-5, initial_accumulator_value=0.1)


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
  """numpy: the logical w, accum, linear after `steps` steps of every rank's batches; replicated
  tables are not stepped at W > 1."""
  w = [t.copy() for t in tables]
  a = [np.full_like(t, F32(DF_FTRL.initial_accumulator_value)) for t in tables]
  z = [np.zeros_like(t) for t in tables]
  for s in range(steps):
    off = 0
    for k, c in enumerate(cols):
      if world == 1 or c.num_buckets > 256:
        rows = np.concatenate([data[s][r][0][c.key] % c.num_buckets for r in range(world)])
        g = np.concatenate([data[s][r][1][:, off:off + c.dimension] for r in range(world)])
        uniq = np.unique(rows)
        sums = oracle.unsorted_segment_sum(g, np.searchsorted(uniq, rows).astype(np.int32), uniq.size)
        np_ftrl(w[k], a[k], z[k], uniq, sums, lr, DF_FTRL)
      off += c.dimension
  return w, a, z


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
  layer = hb.feature_column.DenseFeatures(cols, DEV, coll=coll, batch_size=batch, init=init,
                                          optimizer='ftrl', ftrl=DF_FTRL)
  if fresh:   # (a restore must overwrite every slot: start them away from their initial values)
    for a, z in layer.ftrl_slots:
      a.fill_(7.0)
      z.fill_(-7.0)
  return layer


def _df_steps(layer, data, r, steps, lr, first=0):
  for s in range(first, steps):
    feats, g = data[s][r]
    layer({k: dev(x) for k, x in feats.items()})
    layer.backward(dev(g), apply_lr=lr, optimizer='ftrl', emit=False)


def _df_state(layer):
  return ([w.cpu().numpy() for w in layer.weights], [a.cpu().numpy() for a, _ in layer.ftrl_slots],
          [z.cpu().numpy() for _, z in layer.ftrl_slots], list(layer.sharded))


def _df_check(cols, results, world, want):
  for k, c in enumerate(cols):
    for slot in range(3):
      parts = [res[slot][k] for res in results]
      if world == 1 or not results[0][3][k]:
        got = parts[0]
      else:
        got = np.empty((c.num_buckets, c.dimension), F32)
        for q in range(world):
          got[q::world] = parts[q]
      np.testing.assert_array_equal(got, want[slot][k], err_msg=f'column {k} slot {slot}')


@pytest.mark.parametrize('world', [1, 2])
def test_dense_features_ftrl_steps(world):
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
      np.testing.assert_array_equal(res[1][1], F32(0.1))
      np.testing.assert_array_equal(res[2][1], 0)


def test_dense_features_ftrl_checkpoint_across_world_sizes(tmp_path):
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
    for suffix in ('', '/Ftrl', '/Ftrl_1'):
      assert f'{c.key}_embedding/embedding_weights{suffix}' in names

  def restore_continue(r, coll, barrier):   # a fresh W = 2 layer: restore, the third step
    layer = _df_layer(cols, tables, batch, r, 2, coll, fresh=True)
    layer.restore(prefix, barrier=barrier)
    _df_steps(layer, data, r, steps, lr, first=2)
    st = _df_state(layer)
    layer.close()
    return st
  resumed = _df_world(2, restore_continue)
  for x, y in zip(resumed, unbroken):
    for xs, ys in zip(x[:3], y[:3]):
      for xx, yy in zip(xs, ys):
        np.testing.assert_array_equal(xx, yy)

  # the W = 2 checkpoint at W = 1: every logical row of w, accum and linear
  after2 = _df_reference(cols, tables, data, 2, 2, lr)

  def restore_only(world, src):
    def fn(r, coll, barrier):
      layer = _df_layer(cols, tables, batch, r, world, coll, fresh=True)
      layer.restore(src, barrier=barrier)
      st = _df_state(layer)
      layer.close()
      return st
    return fn
  at1 = _df_world(1, restore_only(1, prefix))
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
  at2 = _df_world(2, restore_only(2, prefix1))
  _df_check(cols, at2, 2, (w1[0][0], w1[0][1], w1[0][2]))


# ---- 8. an independent anchor: the reference project's own configuration --------------------------------
def test_reference_configuration_against_its_closed_form():
  """tf.train.FtrlOptimizer(0.1, l1_regularization_strength=2.0, l2_regularization_strength=1e-5),
  accum 0.1, rows of ones, a gradient of 2 on every element of every stepped row: one step gives
  w = (-2 + 15.0862...) / 20.2485... = 0.6463... and accum 4.1 -- checked against the closed form in
  float64, not against the numpy restatement."""
  rows, dim, lr = 64, 8, 0.1
  ftrl = Ftrl(l1=2.0, l2=1e-5, initial_accumulator_value=0.1)
  table = dev(np.ones((rows, dim), F32))
  acc, lin = ftrl.slots_like(table)
  stepped = np.array([0, 3, 17, 40, 63], np.int64)
  grad = GroupLookupGrad(GroupLookup([table]), ftrl_slots=[(acc, lin)], ftrl=ftrl)
  grad([dev(stepped)], [dev(np.full((stepped.size, dim), 2.0, F32))], apply_lr=lr, optimizer='ftrl')
  torch.cuda.synchronize()
  a0, g = float(F32(0.1)), 2.0
  na = a0 + g * g
  z = g - (np.sqrt(na) - np.sqrt(a0)) / lr * 1.0
  y = np.sqrt(na) / lr + 2 * 1e-5
  w = (-2.0 - z) / y                          # z < -l1: clip(z) = -2
  assert abs(z + 15.0862) < 1e-4 and abs(y - 20.2485) < 1e-4 and abs(w - 0.6463) < 1e-4
  got_w, got_a, got_z = (x.cpu().numpy() for x in (table, acc, lin))
  np.testing.assert_allclose(got_w[stepped], w, rtol=16 * EPS32)
  np.testing.assert_allclose(got_z[stepped], z, rtol=16 * EPS32)
  np.testing.assert_array_equal(got_a[stepped], F32(4.1))
  others = np.setdiff1d(np.arange(rows), stepped)
  np.testing.assert_array_equal(got_w[others], 1.0)
  np.testing.assert_array_equal(got_a[others], F32(0.1))
  np.testing.assert_array_equal(got_z[others], 0.0)
