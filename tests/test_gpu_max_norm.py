"""max_norm (TF's embedding_lookup[_sparse](..., max_norm=)) on the GPU: the clipped forward and the
gradient through the clip against a float64 restatement of include/hbk.h's formulas (within
tests/support/tolerance.py's bound), the exact consequences (a power-of-two max_norm above every row
norm changes no bit; the tie row's radial component is exactly 0), reproducible deterministic modes, the
SGD / Adagrad / Lazy Adam / FTRL steps with the clipped gradient of the pre-step row, mixed calls,
captured graphs and the config-2 shape at full size."""
import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import GroupLookup, GroupLookupGrad
from tests.support.tolerance import assert_sums_close, dense_sums

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
F64 = np.float64
C = 0.5          # a power of two: the tie row [C, 0, ..] is exact
BIG = 4.0        # a power of two above every row norm of _table's rows


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the float64 restatement --------------------------------------------------------------------------
def clip64(x, c):
  x = np.asarray(x, F64)
  n = np.sqrt((x * x).sum(1))
  return x * c / np.maximum(n, c)[:, None]


def jac64(x, g, mag, c):
  """g' of every distinct row (x: its pre-step row, g: its summed gradient, mag: sum|terms| of g) and
  the bound's sum|terms| of g'."""
  x, g, mag = np.asarray(x, F64), np.asarray(g, F64), np.asarray(mag, F64)
  s = (x * x).sum(1)
  n = np.sqrt(s)
  m = np.maximum(n, c)
  radial = (s > 0) & (n >= c)
  d = (g * x).sum(1) * c / (m * m)
  ds = -0.5 * d / np.where(n > 0, n, 1.0)
  scale = (c / m)[:, None]
  gp = g * scale + np.where(radial[:, None], 2.0 * ds[:, None] * x, 0.0)
  nn = np.where(n > 0, n * n, 1.0)
  gmag = scale * (mag + np.where(radial[:, None], np.abs(x) * ((np.abs(x) * mag).sum(1) / nn)[:, None], 0.0))
  return gp, gmag


def rows_of(ids, rows, bucket):
  ids = np.asarray(ids, np.int64)
  return ids % bucket if bucket else ids.copy()


def seg_of(splits, n_ids):
  if splits is None:
    return np.arange(n_ids), np.ones(n_ids, np.int64)
  sp = np.asarray(splits, np.int64)
  lens = np.diff(sp)
  return np.repeat(np.arange(lens.size), lens), lens


def factors(splits, n_ids, w, comb):
  """Per id: the factor of its row in its segment's output (and of the segment's gradient in its
  term): w_j / W_s (mean), w_j / sqrt(Q_s) (sqrtn), w_j (sum); unweighted w = 1, W = count."""
  seg, lens = seg_of(splits, n_ids)
  w = np.ones(n_ids, F64) if w is None else np.asarray(w, F64)
  S = lens.size
  if comb == 'sum':
    div = np.ones(S)
  elif comb == 'mean':
    div = np.bincount(seg, weights=w, minlength=S)
  else:
    div = np.sqrt(np.bincount(seg, weights=w * w, minlength=S))
  safe = np.where(div != 0, div, 1.0)
  return seg, np.where(div[seg] != 0, w / safe[seg], 0.0), S


def fwd64(table, ids, splits, w, comb, c, bucket=0):
  r = rows_of(ids, table.shape[0], bucket)
  y = clip64(table[r], c) if c else np.asarray(table[r], F64)
  seg, f, S = factors(splits, len(ids), w, comb)
  return dense_sums((S, table.shape[1]), seg, y * f[:, None])


def grad64(table, ids, splits, w, comb, gout, c, bucket=0):
  """{row: (g', sum|terms| of g')} of every distinct row."""
  r = rows_of(ids, table.shape[0], bucket)
  seg, f, _ = factors(splits, len(ids), w, comb)
  u, inv = np.unique(r, return_inverse=True)
  G, M = dense_sums((u.size, table.shape[1]), inv, np.asarray(gout, F64)[seg] * f[:, None])
  gp, gm = jac64(table[u], G, M, c)
  return u, gp, gm


# ---- data ---------------------------------------------------------------------------------------------
def _table(rng, rows, dim, c=C):
  """Rows of norms between 0.2 c and 3 c, plus a zero row (0), a tie row [c, 0, ..] (1) and a row
  exactly on the ball in another direction (2, when dim > 1)."""
  t = rng.randn(rows, dim)
  t /= np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-30)
  t *= rng.uniform(0.2 * c, 3 * c, size=(rows, 1))
  t[0] = 0
  t[1] = 0
  t[1, 0] = c
  if dim > 1:
    t[2] = 0
    t[2, dim - 1] = -c
  return t.astype(F32)


def _small_table(rng, rows, dim):
  t = rng.uniform(-0.01, 0.01, size=(rows, dim)).astype(F32)
  t[0] = 0
  return t


def _ids(rng, rows, n, bucket, dtype):
  base = rng.randint(0, rows, size=n)
  base[:3] = [0, 1, 2 % rows]          # the zero row, the tie row and the other one on the ball
  ids = base + rows * rng.randint(0, 50, size=n) if bucket else base
  return ids.astype(dtype)


def _splits(rng, n_seg, max_len=6):
  lens = rng.randint(0, max_len + 1, size=n_seg)
  return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


# ---- 1. forward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [1, 3, 4, 16, 33, 64, 128, 256])
@pytest.mark.parametrize('csr', [False, True])
@pytest.mark.parametrize('weighted', [False, True])
def test_forward_against_f64(dim, csr, weighted):
  rng = np.random.RandomState(dim * 4 + 2 * csr + weighted)
  rows = 97
  table = _table(rng, rows, dim)
  for k, comb in enumerate(('sum', 'mean', 'sqrtn')):
    bucket = rows if (k + dim) % 2 else 0
    dtype = np.int64 if (k + csr) % 2 else np.int32
    splits = _splits(rng, 50) if csr else None
    n = int(splits[-1]) if csr else 200
    ids = _ids(rng, rows, n, bucket, dtype)
    w = rng.uniform(0.1, 2.0, size=n).astype(F32) if weighted else None
    want, mag = fwd64(table, ids, splits, w, comb, C, bucket)
    # aligned: a table of its own; unaligned: a table and an output one float into a buffer (4-byte
    # chunks; the gather refuses those above 64 floats)
    for unaligned in ((False, True) if dim <= 64 else (False,)):
      if unaligned:
        buf = torch.zeros(rows * dim + 1, device=DEV)
        buf[1:].copy_(dev(table).view(-1))
        t = buf[1:].view(rows, dim)
      else:
        t = dev(table)
      lookup = GroupLookup([t], buckets=[bucket], combiners=comb, max_norms=C)
      sp = [dev(splits)] if csr else None
      out = lookup([dev(ids)], sp, sp_weights=[dev(w)] if weighted else None)[0]
      assert_sums_close(out.cpu().numpy(), want, mag,
                        err_msg=f'dim {dim} csr {csr} w {weighted} {comb} unaligned {unaligned}')


def test_forward_mixed_columns_and_refusals():
  rng = np.random.RandomState(7)
  tables = [_table(rng, 61, 16), _table(rng, 61, 16)]
  ids = [_ids(rng, 61, 300, 0, np.int64) for _ in range(2)]
  d_ids = [dev(i) for i in ids]
  plain = GroupLookup([dev(t) for t in tables], combiners='sum')(d_ids)
  mixed = GroupLookup([dev(t) for t in tables], combiners='sum', max_norms=[None, C])(d_ids)
  np.testing.assert_array_equal(mixed[0].cpu().numpy(), plain[0].cpu().numpy())
  want, mag = fwd64(tables[1], ids[1], None, None, 'sum', C)
  assert_sums_close(mixed[1].cpu().numpy(), want, mag)
  for bad in (0.0, -1.0, float('nan'), float('inf')):
    with pytest.raises(_lib.InvalidArgumentError):
      GroupLookup([dev(t) for t in tables], max_norms=[C, bad])


# ---- 2. exactness -------------------------------------------------------------------------------------
def _pair(rng, dims, rows, n, csr):
  tables = [_small_table(rng, rows, d) for d in dims]
  ids = [_ids(rng, rows, n, 0, np.int64) for _ in dims]
  splits = [_splits(rng, n // 3) for _ in dims] if csr else None
  if csr:
    ids = [_ids(rng, rows, int(s[-1]), 0, np.int64) for s in splits]
  grads = [rng.randn((len(s) - 1) if csr else n, d).astype(F32) for s, d in
           zip(splits if csr else [None] * len(dims), dims)]
  return tables, ids, splits, grads


def _state(tables):
  return [dev(t) for t in tables]


@pytest.mark.parametrize('optimizer,emit', [('emit', True)] + [(o, e) for o in ('sgd', 'adagrad', 'adam', 'ftrl')
                                                                   for e in (True, False)])
def test_big_power_of_two_max_norm_changes_no_bit(optimizer, emit):
  rng = np.random.RandomState(11)
  dims = [16, 3, 64, 256]
  tables, ids, splits, grads = _pair(rng, dims, 301, 600, csr=True)
  results = []
  for max_norms in (None, BIG):
    ts = _state(tables)
    accums = [torch.full_like(t, 0.1) for t in ts]
    moments = [(torch.zeros_like(t), torch.zeros_like(t)) for t in ts]
    fslots = [hb.embedding.Ftrl().slots_like(t) for t in ts]
    lookup = GroupLookup(ts, combiners='mean', max_norms=max_norms)
    out = lookup([dev(i) for i in ids], [dev(s) for s in splits])
    grad = GroupLookupGrad(lookup, accums=accums, moments=moments, ftrl_slots=fslots, deterministic=True)
    res = grad([dev(i) for i in ids], [dev(g) for g in grads], [dev(s) for s in splits],
               apply_lr=0.0 if optimizer == 'emit' else 0.05,
               optimizer='sgd' if optimizer == 'emit' else optimizer, emit=emit)
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in out] + [t.cpu().numpy() for t in ts]
    got += [a.cpu().numpy() for a in accums] + [x.cpu().numpy() for p in moments + fslots for x in p]
    if emit:
      for urows, grows, nu in res:
        k = int(nu.item())
        got += [urows[:k].cpu().numpy(), grows[:k].cpu().numpy()]
    results.append(got)
  for a, b in zip(*results):
    np.testing.assert_array_equal(a, b)


def test_mixed_call_keeps_unclipped_columns_bits():
  rng = np.random.RandomState(12)
  dims = [16, 8, 16]
  tables, ids, splits, grads = _pair(rng, dims, 211, 500, csr=False)
  tables = [_table(rng, 211, d) for d in dims]
  for optimizer in ('sgd', 'adagrad'):
    res = []
    for max_norms in (None, [None, C, None]):
      ts = _state(tables)
      accums = [torch.full_like(t, 0.1) for t in ts]
      lookup = GroupLookup(ts, combiners='sum', max_norms=max_norms)
      grad = GroupLookupGrad(lookup, accums=accums, deterministic=True)
      grad([dev(i) for i in ids], [dev(g) for g in grads], apply_lr=0.1, optimizer=optimizer)
      torch.cuda.synchronize()
      res.append([t.cpu().numpy() for t in ts] + [a.cpu().numpy() for a in accums])
    for c in (0, 2):
      np.testing.assert_array_equal(res[1][c], res[0][c])
      np.testing.assert_array_equal(res[1][3 + c], res[0][3 + c])
    assert not np.array_equal(res[1][1], res[0][1])   # (the clipped column did step differently)


# ---- 3. backward emit ---------------------------------------------------------------------------------
def _emit(tables, ids, splits, grads, combs, max_norms, w=None, deterministic=True, bucket=None):
  ts = _state(tables)
  lookup = GroupLookup(ts, buckets=bucket, combiners=combs, max_norms=max_norms)
  grad = GroupLookupGrad(lookup, deterministic=deterministic)
  res = grad([dev(i) for i in ids], [dev(g) for g in grads],
             [None if s is None else dev(s) for s in splits] if splits else None,
             sp_weights=None if w is None else [None if x is None else dev(x) for x in w])
  torch.cuda.synchronize()
  out = []
  for urows, grows, nu in res:
    k = int(nu.item())
    u, g = urows[:k].cpu().numpy(), grows[:k].cpu().numpy()
    order = np.argsort(u)
    out.append((u[order], g[order]))
  return out


@pytest.mark.parametrize('dim', [1, 4, 16, 33, 128, 256])
@pytest.mark.parametrize('weighted', [False, True])
def test_emit_against_f64_jacobian(dim, weighted):
  rng = np.random.RandomState(100 + dim + weighted)
  rows = 89
  combs = ['sum', 'mean', 'sqrtn']
  tables = [_table(rng, rows, dim) for _ in combs]
  splits = [_splits(rng, 80) for _ in combs]
  ids = [_ids(rng, rows, int(s[-1]), 0, np.int64) for s in splits]
  grads = [rng.randn(len(s) - 1, dim).astype(F32) for s in splits]
  w = [rng.uniform(0.1, 2.0, size=len(i)).astype(F32) for i in ids] if weighted else None
  for det in (False, True):
    got = _emit(tables, ids, splits, grads, combs, C, w=w, deterministic=det)
    for c, comb in enumerate(combs):
      u, gp, gm = grad64(tables[c], ids[c], splits[c], None if w is None else w[c], comb, grads[c], C)
      np.testing.assert_array_equal(got[c][0], u)
      assert_sums_close(got[c][1], gp, gm, err_msg=f'{comb} det {det}')


def test_tie_and_zero_rows_exact():
  rng = np.random.RandomState(5)
  dim, rows = 16, 40
  table = _table(rng, rows, dim)
  ids = np.array([0, 1, 1, 0, 5, 1, 7], np.int64)
  grads = rng.randn(ids.size, dim).astype(F32)
  plain = _emit([table], [ids], None, [grads], 'sum', None)[0]
  clipped = _emit([table], [ids], None, [grads], 'sum', C)[0]
  np.testing.assert_array_equal(plain[0], clipped[0])
  G = dict(zip(plain[0].tolist(), plain[1]))
  gp = dict(zip(clipped[0].tolist(), clipped[1]))
  # zero row: g' = (G / c) * c
  np.testing.assert_array_equal(gp[0], (G[0] / F32(C)) * F32(C))
  # tie row x = [c, 0, ..]: the radial component is exactly 0, the others are G's
  assert gp[1][0] == 0.0
  np.testing.assert_array_equal(gp[1][1:], G[1][1:])


@pytest.mark.parametrize('mode', [1, 2])
def test_deterministic_modes_reproduce(hbk_option, mode):
  hbk_option('bwd_deterministic', mode)
  rng = np.random.RandomState(30 + mode)
  dims = [16, 33, 128]
  tables = [_table(rng, 4001, d) for d in dims]
  ids = [rng.randint(0, 4001, size=20000).astype(np.int64) for _ in dims]
  grads = [rng.randn(20000, d).astype(F32) for d in dims]
  a = _emit(tables, ids, None, grads, 'sum', C, deterministic=False)
  b = _emit(tables, ids, None, grads, 'sum', C, deterministic=False)
  for (ua, ga), (ub, gb) in zip(a, b):
    np.testing.assert_array_equal(ua, ub)
    np.testing.assert_array_equal(ga, gb)
  for c in range(len(dims)):
    u, gp, gm = grad64(tables[c], ids[c], None, None, 'sum', grads[c], C)
    assert_sums_close(a[c][1], gp, gm)


# ---- 4. steps -----------------------------------------------------------------------------------------
def _step_ref_fp32(optimizer, x, gp, slots, lr, state):
  """The fp32 step of include/hbk.h from g' (the emit form's clipped rows), op by op."""
  lr = F32(lr)
  if optimizer == 'sgd':
    return x - lr * gp, slots
  if optimizer == 'adagrad':
    acc = slots[0] + gp * gp
    return x - (lr * gp) * (F32(1.0) / np.sqrt(acc)), (acc,)
  if optimizer == 'adam':
    b1, b2, eps, p1, p2 = state
    lr_t = (lr * np.sqrt(F32(1) - p2)) / (F32(1) - p1)
    m = b1 * slots[0] + (F32(1) - b1) * gp
    v = b2 * slots[1] + (F32(1) - b2) * (gp * gp)
    return x - (lr_t * m) / (np.sqrt(v) + eps), (m, v)
  a, z = slots
  na = a + gp * gp
  pn, po = np.sqrt(na), np.sqrt(a)
  zn = z + (gp - ((pn - po) / lr) * x)
  y = pn / lr + F32(0.0)
  l1 = F32(0.001)
  return (np.clip(zn, -l1, l1) - zn) / y, (na, zn)


@pytest.mark.parametrize('optimizer', ['sgd', 'adagrad', 'adagrad_interleaved', 'adam', 'ftrl'])
@pytest.mark.parametrize('emit', [True, False])
def test_steps_with_the_clipped_gradient_of_the_pre_step_row(optimizer, emit):
  rng = np.random.RandomState(40)
  dims = [16, 3, 64]
  rows = 503
  tables = [_table(rng, rows, d) for d in dims]
  splits = [_splits(rng, 200) for _ in dims]
  ids = [_ids(rng, rows, int(s[-1]), rows, np.int64) for s in splits]
  grads = [rng.randn(len(s) - 1, d).astype(F32) for s, d in zip(splits, dims)]
  lr = 0.05
  gp = _emit(tables, ids, splits, grads, 'mean', C, bucket=[rows] * 3)
  # g' itself against float64
  for c in range(len(dims)):
    u, want, gm = grad64(tables[c], ids[c], splits[c], None, 'mean', grads[c], C, bucket=rows)
    assert_sums_close(gp[c][1], want, gm)
  ts = _state(tables)
  opt = optimizer
  kw = {}
  if optimizer == 'adagrad':
    kw['accums'] = [torch.full_like(t, 0.1) for t in ts]
  elif optimizer == 'adagrad_interleaved':
    opt = 'adagrad'
    kw['interleaved'] = [torch.cat([t, torch.full_like(t, 0.1)], 1).contiguous() for t in ts]
  elif optimizer == 'adam':
    kw['moments'] = [(torch.zeros_like(t), torch.zeros_like(t)) for t in ts]
    kw['adam'] = hb.embedding.LazyAdam(device=DEV)
  elif optimizer == 'ftrl':
    kw['ftrl'] = hb.embedding.Ftrl(l1=0.001)
    kw['ftrl_slots'] = [kw['ftrl'].slots_like(t) for t in ts]
  lookup = GroupLookup(ts, buckets=[rows] * 3, combiners='mean', max_norms=C)
  grad = GroupLookupGrad(lookup, deterministic=True, **kw)
  grad([dev(i) for i in ids], [dev(g) for g in grads], [dev(s) for s in splits], apply_lr=lr,
       optimizer=opt, emit=emit)
  torch.cuda.synchronize()
  for c in range(len(dims)):
    u, g = gp[c]
    x = tables[c][u]
    if optimizer == 'sgd':
      slots, got_slots = (), ()
      w_after = ts[c].cpu().numpy()
    elif optimizer == 'adagrad':
      slots = (np.full_like(x, F32(0.1)),)
      got_slots = (kw['accums'][c].cpu().numpy(),)
      w_after = ts[c].cpu().numpy()
    elif optimizer == 'adagrad_interleaved':
      slots = (np.full_like(x, F32(0.1)),)
      b = kw['interleaved'][c].cpu().numpy()
      w_after, got_slots = b[:, :dims[c]], (b[:, dims[c]:],)
    elif optimizer == 'adam':
      slots = (np.zeros_like(x), np.zeros_like(x))
      got_slots = tuple(s.cpu().numpy() for s in kw['moments'][c])
      w_after = ts[c].cpu().numpy()
    else:
      slots = (np.full_like(x, F32(0.1)), np.zeros_like(x))
      got_slots = tuple(s.cpu().numpy() for s in kw['ftrl_slots'][c])
      w_after = ts[c].cpu().numpy()
    state = (F32(0.9), F32(0.999), F32(1e-8), F32(0.9), F32(0.999))
    want_w, want_slots = _step_ref_fp32(optimizer.split('_')[0], x, g, slots, lr, state)
    np.testing.assert_array_equal(w_after[u], want_w, err_msg=f'{optimizer} column {c}')
    for a, b in zip(got_slots, want_slots):
      np.testing.assert_array_equal(a[u], b)
    untouched = np.setdiff1d(np.arange(rows), u)
    np.testing.assert_array_equal(w_after[untouched], tables[c][untouched])


# ---- 7. graph replay ----------------------------------------------------------------------------------
def test_captured_forward_backward_sgd_equals_direct_calls():
  rng = np.random.RandomState(70)
  dims, rows, K, lr = [16, 8], 1009, 4, 0.1
  tables = [_table(rng, rows, d) for d in dims]
  ids = [dev(_ids(rng, rows, 3000, 0, np.int64)) for _ in dims]
  grads = [dev(rng.randn(3000, d).astype(F32)) for d in dims]

  def make():
    ts = _state(tables)
    lookup = GroupLookup(ts, combiners='sum', max_norms=C)
    outs = [torch.empty(3000, d, device=DEV) for d in dims]
    return ts, lookup, GroupLookupGrad(lookup, deterministic=True), outs

  direct = make()
  for _ in range(K):
    direct[1](ids, outs=direct[3])
    direct[2](ids, grads, apply_lr=lr)
  graphed = make()
  graphed[1](ids, outs=graphed[3])
  graphed[2](ids, grads, apply_lr=lr)      # binds; step 1
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      graphed[1].launch()
      graphed[2].launch(apply_lr=lr)
  torch.cuda.synchronize()
  for _ in range(K - 1):
    graph.replay()
  torch.cuda.synchronize()
  for a, b in zip(direct[0] + direct[3], graphed[0] + graphed[3]):
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
  assert not np.array_equal(direct[0][0].cpu().numpy(), tables[0])


# ---- 8. config-2 shape at full size -------------------------------------------------------------------
def test_config2_shape_half_the_rows_clipped():
  cols, rows, dim, batch, lr = 26, 1_000_000, 16, 65536, 0.1
  gen = torch.Generator(device=DEV)
  gen.manual_seed(8)
  tables = [torch.empty(rows, dim, device=DEV).uniform_(-1e-3, 1e-3, generator=gen) for _ in range(cols)]
  ids = [torch.randint(0, 1 << 40, (batch,), device=DEV, dtype=torch.int64, generator=gen)
         for _ in range(cols)]
  grads = [torch.randn(batch, dim, device=DEV, generator=gen) for _ in range(cols)]
  sample = tables[0][:4096].cpu().numpy().astype(F64)
  c = float(np.median(np.linalg.norm(sample, axis=1)))
  lookup = GroupLookup(tables, buckets=[rows] * cols, combiners='sum', max_norms=c)
  outs = lookup(ids)
  pre = [t.cpu().numpy() for t in tables]
  grad = GroupLookupGrad(lookup)
  res = grad(ids, grads)          # emit: g'
  torch.cuda.synchronize()
  rs = np.random.RandomState(9)
  clipped_share = []
  for k in range(cols):
    r = ids[k].cpu().numpy() % rows
    s = rs.choice(batch, 2048, replace=False)
    want, mag = fwd64(pre[k], r[s], None, None, 'sum', c)
    assert_sums_close(outs[k].cpu().numpy()[s], want, mag, err_msg=f'forward column {k}')
    clipped_share.append(np.mean(np.linalg.norm(pre[k][r].astype(F64), axis=1) > c))
    urows, grows, nu = res[k]
    n = int(nu.item())
    got_u = urows[:n].cpu().numpy()
    order = np.argsort(got_u)
    u, gp, gm = grad64(pre[k], r, None, None, 'sum', grads[k].cpu().numpy(), c)
    np.testing.assert_array_equal(got_u[order], u)
    assert_sums_close(grows[:n].cpu().numpy()[order], gp, gm, err_msg=f'emit column {k}')
  assert 0.3 < np.mean(clipped_share) < 0.7
  # + SGD (step only) from the same tables: the stepped rows against float64
  grad2 = GroupLookupGrad(lookup)
  grad2(ids, grads, apply_lr=lr, emit=False)
  torch.cuda.synchronize()
  for k in range(0, cols, 5):
    r = ids[k].cpu().numpy() % rows
    u, gp, gm = grad64(pre[k], r, None, None, 'sum', grads[k].cpu().numpy(), c)
    got = tables[k].cpu().numpy()
    assert_sums_close(got[u], pre[k][u].astype(F64) - lr * gp, np.abs(pre[k][u]) + lr * gm,
                      err_msg=f'sgd column {k}')


# ---- 2b. mixed Adam / FTRL calls; the IndexedSlices of a stepping call -----------------------------
@pytest.mark.parametrize('optimizer', ['adam', 'ftrl'])
def test_mixed_two_slot_call_keeps_unclipped_columns_bits(optimizer):
  rng = np.random.RandomState(13)
  dims = [16, 8, 16]
  tables = [_table(rng, 211, d) for d in dims]
  ids = [_ids(rng, 211, 500, 0, np.int64) for _ in dims]
  grads = [rng.randn(500, d).astype(F32) for d in dims]
  res = []
  for max_norms in (None, [None, C, None]):
    ts = _state(tables)
    kw = {}
    if optimizer == 'adam':
      kw['moments'] = [(torch.zeros_like(t), torch.zeros_like(t)) for t in ts]
      kw['adam'] = hb.embedding.LazyAdam(device=DEV)
      slots = kw['moments']
    else:
      kw['ftrl'] = hb.embedding.Ftrl(l1=0.001)
      kw['ftrl_slots'] = [kw['ftrl'].slots_like(t) for t in ts]
      slots = kw['ftrl_slots']
    lookup = GroupLookup(ts, combiners='sum', max_norms=max_norms)
    grad = GroupLookupGrad(lookup, deterministic=True, **kw)
    out = grad([dev(i) for i in ids], [dev(g) for g in grads], apply_lr=0.05, optimizer=optimizer)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in ts] + [[x.cpu().numpy() for x in p] for p in slots]
    got.append([emitted_sorted(o) for o in out])
    res.append(got)
  for c in (0, 2):
    np.testing.assert_array_equal(res[1][c], res[0][c])
    for a, b in zip(res[1][3 + c], res[0][3 + c]):
      np.testing.assert_array_equal(a, b)
    for a, b in zip(res[1][6][c], res[0][6][c]):
      np.testing.assert_array_equal(a, b)
  assert not np.array_equal(res[1][1], res[0][1])


def emitted_sorted(res):
  urows, grows, nu = res
  k = int(nu.item())
  u, g = urows[:k].cpu().numpy(), grows[:k].cpu().numpy()
  order = np.argsort(u)
  return u[order], g[order]


@pytest.mark.parametrize('optimizer', ['sgd', 'adagrad', 'adam', 'ftrl'])
def test_stepping_call_returns_the_clipped_gradient(optimizer):
  """With a step the IndexedSlices of a clipped column are g', the gradient its rows were stepped with:
  the rows of the emit form, bit for bit."""
  rng = np.random.RandomState(14)
  dims = [16, 3]
  tables = [_table(rng, 307, d) for d in dims]
  ids = [_ids(rng, 307, 700, 0, np.int64) for _ in dims]
  grads = [rng.randn(700, d).astype(F32) for d in dims]
  want = _emit(tables, ids, None, grads, 'sum', C)
  ts = _state(tables)
  kw = {'accums': [torch.full_like(t, 0.1) for t in ts],
        'moments': [(torch.zeros_like(t), torch.zeros_like(t)) for t in ts],
        'ftrl_slots': [hb.embedding.Ftrl().slots_like(t) for t in ts]}
  lookup = GroupLookup(ts, combiners='sum', max_norms=C)
  grad = GroupLookupGrad(lookup, deterministic=True, **kw)
  out = grad([dev(i) for i in ids], [dev(g) for g in grads], apply_lr=0.05, optimizer=optimizer)
  torch.cuda.synchronize()
  for c in range(len(dims)):
    u, g = emitted_sorted(out[c])
    np.testing.assert_array_equal(u, want[c][0])
    np.testing.assert_array_equal(g, want[c][1])


# ---- 5. sharded ---------------------------------------------------------------------------------------
def _world_g64(tables_c, rows, ids_r, splits_r, w_r, comb, grads_r, c):
  """float64 g' over the logical table from every rank's batch: (rows touched, g', sum|terms|)."""
  dim = tables_c.shape[1]
  G, M = np.zeros((rows, dim)), np.zeros((rows, dim))
  for ids, sp, w, g in zip(ids_r, splits_r, w_r, grads_r):
    r = rows_of(ids, rows, rows)
    seg, f, _ = factors(sp, len(ids), w, comb)
    a, b = dense_sums((rows, dim), r, np.asarray(g, F64)[seg] * f[:, None])
    G += a
    M += b
  u = np.nonzero(M.sum(1) > 0)[0]
  gp, gm = jac64(tables_c[u], G[u], M[u], c)
  return u, gp, gm


@pytest.mark.parametrize('world', [1, 2, 4, 8])
@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
def test_sharded_against_f64(world, optimizer):
  import threading
  from hybridbackend_amd.embedding.sharded import ShardedGroupLookup
  from tests.support.tolerance import WIRE16_FLOOR, WIRE16_REL
  wire16 = world in (2, 8)
  dedup = world in (4, 8)
  weighted = world in (1, 4, 8)
  rng = np.random.RandomState(500 + world + (optimizer == 'adam'))
  dims, rows, combs = [16, 8, 33], [3001, 211, 1009], ['sum', 'mean', 'sqrtn']
  n = len(dims)
  max_norms = [C, C, None]
  tables = [_table(rng, rows[c], dims[c]) for c in range(n)]
  ids, splits, grads, ws = [], [], [], []
  for _ in range(world):
    rid, rsp, rg, rw = [], [], [], []
    for c in range(n):
      sp = None if c == 0 else _splits(rng, 200)
      k = 600 if sp is None else int(sp[-1])
      rsp.append(sp)
      rid.append(_ids(rng, rows[c], k, rows[c], np.int64))
      rw.append(rng.uniform(0.1, 2.0, size=k).astype(F32) if weighted else None)
      rg.append(rng.randn(k if sp is None else sp.size - 1, dims[c]).astype(F32))
    ids.append(rid)
    splits.append(rsp)
    grads.append(rg)
    ws.append(rw)
  comms = hb.distribute.Collective.local_world(world)
  shards = [[dev(t[r::world].copy()) for t in tables] for r in range(world)]
  adams = [hb.embedding.LazyAdam(device=DEV) for _ in range(world)]
  moments = [[(torch.zeros_like(s), torch.zeros_like(s)) for s in shards[r]] for r in range(world)]
  results, errors = [None] * world, []
  lr = 0.05

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        drv = ShardedGroupLookup(shards[r], comms[r], buckets=rows, combiners=combs, dedup=[dedup] * n,
                                 wire_dtype=torch.float16 if wire16 else None, max_norms=max_norms,
                                 moments=moments[r], adam=adams[r])
        d_ids = [dev(i) for i in ids[r]]
        d_sp = [None if s is None else dev(s) for s in splits[r]]
        d_w = [None if w is None else dev(w) for w in ws[r]] if weighted else None
        outs = drv(d_ids, d_sp, sp_weights=d_w)
        slices = drv.backward([dev(g) for g in grads[r]], apply_lr=0.0)
        torch.cuda.current_stream().synchronize()
        first = [o.cpu().numpy().copy() for o in outs]
        emit = [tuple(x.copy() for x in emitted_sorted(s)) for s in slices]
        drv(d_ids, d_sp, sp_weights=d_w)
        drv.backward([dev(g) for g in grads[r]], apply_lr=lr, optimizer=optimizer, emit=False)
        torch.cuda.current_stream().synchronize()
        results[r] = (first, emit)
        drv.close()
    except Exception as e:  # pylint: disable=broad-except
      errors.append((r, repr(e)))

  threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=120)
  assert not errors, errors
  assert all(x is not None for x in results)
  rel, floor = (WIRE16_REL, WIRE16_FLOOR) if wire16 else (1e-5, 1e-6)
  for r in range(world):
    for c in range(n):
      tab = tables[c]
      if max_norms[c]:
        y = clip64(tab, max_norms[c])
      else:
        y = tab.astype(F64)
      if wire16:          # the owner clips in fp32, then the rows travel as fp16
        y = y.astype(np.float16).astype(F64)
      want, mag = fwd64(y, ids[r][c], splits[r][c], None if ws[r][c] is None else ws[r][c], combs[c], None,
                        bucket=rows[c])
      assert_sums_close(results[r][0][c], want, mag, rel=rel, floor=floor, err_msg=f'fwd rank {r} col {c}')
  for c in range(n):
    cc = max_norms[c] or 1e30
    u, gp, gm = _world_g64(tables[c], rows[c], [ids[r][c] for r in range(world)],
                           [splits[r][c] for r in range(world)], [ws[r][c] for r in range(world)], combs[c],
                           [grads[r][c] for r in range(world)], cc)
    got = np.zeros((rows[c], dims[c]))
    seen = np.zeros(rows[c], bool)
    for r in range(world):
      lu, lg = results[r][1][c]
      got[lu * world + r] = lg
      seen[lu * world + r] = True
    np.testing.assert_array_equal(np.nonzero(seen)[0], u)
    assert_sums_close(got[u], gp, gm, rel=rel, floor=floor, err_msg=f'emit col {c}')
    after = np.zeros_like(tables[c])
    for r in range(world):
      after[r::world] = shards[r][c].cpu().numpy()
    x = tables[c][u].astype(F64)
    if optimizer == 'sgd':
      assert_sums_close(after[u], x - lr * gp, np.abs(x) + lr * gm, rel=rel, floor=floor, err_msg=f'sgd col {c}')
    else:
      b1, b2, eps = 0.9, 0.999, 1e-8
      lr_t = lr * np.sqrt(1 - b2) / (1 - b1)
      want = x - lr_t * ((1 - b1) * gp) / (np.sqrt((1 - b2) * gp * gp) + eps)
      # Adam's first step is ~lr * sign(g'): an element whose g' lies within the bound of its own
      # rounding (fp16 wire: 1e-3 relative) may take either sign; it moves by at most ~lr either way
      sure = np.abs(gp) > 4 * (rel * gm + floor)
      np.testing.assert_allclose(after[u][sure], want[sure], rtol=0, atol=lr * 2e-3, err_msg=f'adam col {c}')
      assert np.all(np.abs(after[u][~sure] - x[~sure]) <= 1.01 * lr_t * (1 - b1) / np.sqrt(1 - b2))
    untouched = np.setdiff1d(np.arange(rows[c]), u)
    np.testing.assert_array_equal(after[untouched], tables[c][untouched])
  for cm in comms:
    cm.close()


def test_sharded_p2p_bound_plan_refuses_a_clipped_forward(hbk_option):
  import threading
  from hybridbackend_amd.embedding.sharded import ShardedGroupLookup
  hbk_option('sharded_p2p', 1)
  world = 2
  comms = hb.distribute.Collective.local_world(world)
  codes, errors = [None] * world, []

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        drv = ShardedGroupLookup([dev(np.zeros((50, 16), F32))], comms[r], buckets=[100], max_norms=C)
        out = torch.zeros((8, 16), dtype=torch.float32, device=DEV)
        if not drv.p2p_bind([out]):
          codes[r] = 'unbound'
          return
        ids = dev(np.arange(8, dtype=np.int64))
        codes[r] = drv._lib.hbk_sharded_lookup_fwd(drv._plan(), _lib.ptr_array([ids.data_ptr()]),
                                                   _lib.i64_array([8]), None, _lib.i64_array([8]),
                                                   _lib.ptr_array([out.data_ptr()]), None,
                                                   _lib.current_stream(DEV))
        drv.p2p_unbind()
        drv.close()
    except Exception as e:  # pylint: disable=broad-except
      errors.append((r, repr(e)))

  threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=60)
  assert not errors, errors
  assert 'unbound' not in codes, 'peer memory could not be mapped'
  assert codes == [_lib.UNIMPLEMENTED] * world
  for cm in comms:
    cm.close()


# ---- 6. DenseFeatures ---------------------------------------------------------------------------------
@pytest.mark.parametrize('world', [1, 2])
def test_dense_features_max_norm_column(hbk_option, world):
  import threading
  hbk_option('bwd_deterministic', 1)
  rng = np.random.RandomState(90 + world)
  batch, lr = 256, 0.1
  nb = [1009, 977]
  tables = [_table(rng, nb[0], 16), _table(rng, nb[1], 8)]
  feats = []
  for _ in range(world):
    sp = _splits(rng, batch, 4)
    feats.append({'a': (rng.randint(0, 2**40, size=int(sp[-1])).astype(np.int64), sp),
                  'b': rng.randint(0, 2**40, size=batch).astype(np.int64)})
  grads = [rng.randn(batch, 24).astype(F32) for _ in range(world)]

  def layer_run(max_norm):
    comms = hb.distribute.Collective.local_world(world) if world > 1 else [None]
    results, errors = [None] * world, []
    cols = [hb.feature_column.EmbeddingColumn('a', nb[0], 16, 'mean', max_norm=max_norm),
            hb.feature_column.EmbeddingColumn('b', nb[1], 8, 'sum')]

    def run(r):
      try:
        with torch.cuda.stream(torch.cuda.Stream()):
          def init(col, rows, device):
            t = tables[cols.index(col)]
            return dev(t[r::world].copy() if rows != col.num_buckets else t).to(device)
          layer = hb.feature_column.DenseFeatures(cols, DEV, comms[r], batch_size=batch, init=init)
          assert layer.sharded == [world > 1] * 2
          f = {k: (tuple(dev(x) for x in v) if isinstance(v, tuple) else dev(v)) for k, v in feats[r].items()}
          out = layer(f)
          layer.backward(dev(grads[r]), apply_lr=lr)
          torch.cuda.current_stream().synchronize()
          results[r] = (out.cpu().numpy(), [t.cpu().numpy() for t in layer.weights])
          layer.close()
      except Exception as e:  # pylint: disable=broad-except
        errors.append((r, repr(e)))

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
      t.start()
    for t in threads:
      t.join(timeout=120)
    assert not errors, errors
    for cm in comms:
      if cm is not None:
        cm.close()
    return results

  plain = layer_run(None)
  clipped = layer_run(C)
  for r in range(world):
    ia, sp = feats[r]['a']
    want, mag = fwd64(tables[0], ia, sp, None, 'mean', C, bucket=nb[0])
    assert_sums_close(clipped[r][0][:, :16], want, mag)
    np.testing.assert_array_equal(clipped[r][0][:, 16:], plain[r][0][:, 16:])   # the unclipped column
    np.testing.assert_array_equal(clipped[r][1][1], plain[r][1][1])
  # the clipped column's table: SGD with g' of the pre-step rows, over every rank's batch
  u, gp, gm = _world_g64(tables[0], nb[0], [feats[r]['a'][0] for r in range(world)],
                         [feats[r]['a'][1] for r in range(world)], [None] * world, 'mean',
                         [grads[r][:, :16] for r in range(world)], C)
  after = np.zeros_like(tables[0])
  for r in range(world):
    if world > 1:
      after[r::world] = clipped[r][1][0]
    else:
      after = clipped[r][1][0]
  x = tables[0][u].astype(F64)
  assert_sums_close(after[u], x - lr * gp, np.abs(x) + lr * gm)
