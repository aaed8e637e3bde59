"""Weighted lookups (tf.nn.embedding_lookup_sparse with sp_weights) on the GPU: forward bit-equal to a
numpy sequential fp32 reference, backward against float64 within tests/support/tolerance.py's bound
(bit-equal in the deterministic mode), all-ones weights equal to the unweighted path bit for bit, the
sharded driver equal to the single-GPU weighted path, captured graphs."""
import threading

import numpy as np
import pytest
import torch

import oracle
import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import GroupLookup, GroupLookupGrad
from hybridbackend_amd.embedding.sharded import ShardedGroupLookup
from tests.support.tolerance import WIRE16_FLOOR, WIRE16_REL, assert_sums_close, dense_sums

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- numpy reference ----------------------------------------------------------------------------
def rows_of(ids, rows, bucket=0, divisor=1):
  ids = np.asarray(ids, np.int64)
  r = ids % bucket if bucket else ids.copy()
  r = np.where(r >= 0, r // divisor, -1)
  valid = (r >= 0) & (r < rows)
  return np.where(valid, r, 0), valid


def segments(splits, n_ids):
  return np.arange(n_ids + 1, dtype=np.int32) if splits is None else np.asarray(splits)


def ref_fwd(table, ids, splits, w, comb, bucket=0, divisor=1):
  """Sequential fp32: for each segment, in id order, acc += w_j * e_j over valid ids; divisor sum."""
  r, valid = rows_of(ids, table.shape[0], bucket, divisor)
  sp = segments(splits, len(ids))
  S, dim = sp.size - 1, table.shape[1]
  lens = np.diff(sp)
  acc = np.zeros((S, dim), F32)
  div = np.zeros(S, F32)
  w = np.asarray(w, F32)
  for k in range(int(lens.max()) if S else 0):
    seg = np.nonzero(lens > k)[0]
    j = sp[seg] + k
    keep = valid[j]
    seg, j = seg[keep], j[keep]
    acc[seg] = acc[seg] + table[r[j]] * w[j][:, None]
    div[seg] = div[seg] + (w[j] * w[j] if comb == 'sqrtn' else w[j])
  if comb == 'sum':
    return acc
  d = div if comb == 'mean' else np.sqrt(div)
  out = np.zeros_like(acc)
  nz = d != 0
  out[nz] = acc[nz] / d[nz][:, None]
  return out


def ref_terms(table_rows, ids, splits, w, comb, grad, bucket=0, divisor=1):
  """t_j = (g_s / W_s) * w_j (mean), (g_s / sqrtf(Q_s)) * w_j (sqrtn), g_s * w_j (sum), fp32; the
  rows and validity of the ids."""
  r, valid = rows_of(ids, table_rows, bucket, divisor)
  sp = segments(splits, len(ids))
  w = np.asarray(w, F32)
  seg = np.repeat(np.arange(sp.size - 1), np.diff(sp))
  g = grad[seg]
  if comb != 'sum':
    div = np.zeros(sp.size - 1, F32)
    lens = np.diff(sp)
    for k in range(int(lens.max()) if lens.size else 0):
      s = np.nonzero(lens > k)[0]
      j = sp[s] + k
      keep = valid[j]
      s, j = s[keep], j[keep]
      div[s] = div[s] + (w[j] * w[j] if comb == 'sqrtn' else w[j])
    d = (div if comb == 'mean' else np.sqrt(div))[seg]
    g = np.where((d != 0)[:, None], g / np.where(d != 0, d, 1)[:, None], F32(0)).astype(F32)
  return (g * w[:, None]).astype(F32), r, valid


def seq_row_sums(t, r, valid):
  """(ascending distinct rows, their sequential fp32 sums of t in id order)"""
  rr, tt = r[valid], t[valid]
  uniq = np.unique(rr)
  return uniq, oracle.unsorted_segment_sum(tt, np.searchsorted(uniq, rr).astype(np.int32), uniq.size)


def ragged(rng, n_seg, lam=3, cap=12, empty_ok=True):
  lens = rng.poisson(lam, size=n_seg).clip(0 if empty_ok else 1, cap)
  return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def emitted(res):
  u, g, k = res
  k = int(k.item())
  return u.cpu().numpy()[:k], g.cpu().numpy()[:k]


# ---- 1. TF's published example ------------------------------------------------------------------
@pytest.mark.parametrize('comb', ['sum', 'mean', 'sqrtn'])
def test_tf_docstring_example(comb):
  rng = np.random.RandomState(1)
  p = rng.randn(4, 8).astype(F32)
  ids = np.array([1, 3, 0, 1], np.int64)
  sp = np.array([0, 2, 3, 4], np.int32)
  w = np.array([2.0, 0.5, 1.0, 3.0], F32)
  got = hb.embedding.group_lookup([dev(p)], [dev(ids)], [dev(sp)], combiners=comb,
                                  sp_weights=[dev(w)])[0].cpu().numpy()
  np.testing.assert_array_equal(got, ref_fwd(p, ids, sp, w, comb))
  want0 = {'sum': 2 * p[1] + 0.5 * p[3], 'mean': (2 * p[1] + 0.5 * p[3]) / 2.5,
           'sqrtn': (2 * p[1] + 0.5 * p[3]) / np.sqrt(4.25)}[comb]
  np.testing.assert_allclose(got[0], want0, rtol=1e-6)
  np.testing.assert_allclose(got[1], p[0], rtol=1e-6)
  np.testing.assert_allclose(got[2], {'sum': 3 * p[1], 'mean': p[1], 'sqrtn': p[1]}[comb], rtol=1e-6)


# ---- 2. forward, bit-equal --------------------------------------------------------------------
@pytest.mark.parametrize('dim', [1, 3, 4, 8, 16, 32, 64, 128, 256])
@pytest.mark.parametrize('id32', [False, True])
def test_forward_bit_equal(dim, id32):
  rng = np.random.RandomState(dim + 7 * id32)
  rows, bucket, divisor = 3001, 6007, 2
  table = rng.randn(rows, dim).astype(F32)
  combs = ['sum', 'mean', 'sqrtn', 'mean', 'sum', 'sqrtn']
  ids, sps, ws = [], [], []
  for c, comb in enumerate(combs):
    sp = None if c < 3 else ragged(rng, 700)
    n = 1500 if sp is None else int(sp[-1])
    i = rng.randint(-50, 2 * rows, size=n)            # negative and out-of-range ids (no bucket: c even)
    if c % 2:
      i = rng.randint(0, 2**30 if id32 else 2**40, size=n)
    w = rng.uniform(-1, 2, size=n).astype(F32)
    w[rng.rand(n) < 0.05] = 0
    if sp is not None:                                 # segments whose weights cancel: zero divisor
      for s in range(0, sp.size - 1, 17):
        if sp[s + 1] - sp[s] == 2:
          w[sp[s] + 1] = -w[sp[s]]
    ids.append(i.astype(np.int32 if id32 else np.int64))
    sps.append(sp)
    ws.append(w)
  lk = GroupLookup([dev(table)] * len(combs), buckets=[0 if c % 2 == 0 else bucket for c in range(6)],
                   combiners=combs, divisor=divisor)
  outs = lk([dev(i) for i in ids], [None if s is None else dev(s) for s in sps],
            sp_weights=[dev(w) for w in ws])
  for c, comb in enumerate(combs):
    want = ref_fwd(table, ids[c], sps[c], ws[c], comb, 0 if c % 2 == 0 else bucket, divisor)
    np.testing.assert_array_equal(outs[c].cpu().numpy(), want, err_msg=f'col {c} {comb}')


def test_forward_mixed_strided_and_many_columns():
  rng = np.random.RandomState(5)
  n, rows, dim = 150, 997, 8                           # > 128 columns: more than one launch
  tables = [rng.randn(rows, dim).astype(F32) for _ in range(3)]
  combs = ['sum', 'mean', 'sqrtn']
  ids, sps, ws = [], [], []
  for c in range(n):
    sp = ragged(rng, 64) if c % 2 else None
    k = 64 if sp is None else int(sp[-1])
    ids.append(rng.randint(0, rows, size=k).astype(np.int64))
    sps.append(sp)
    ws.append(rng.uniform(0.1, 3, size=k).astype(F32) if c % 3 else None)
  d_tables = [dev(t) for t in tables]
  lk = GroupLookup([d_tables[c % 3] for c in range(n)], combiners=[combs[c % 3] for c in range(n)])
  block = torch.empty((64, n * dim + 4), dtype=torch.float32, device=DEV)   # out_stride blocks
  outs = [block[:, c * dim:(c + 1) * dim] for c in range(n)]
  d_ids = [dev(i) for i in ids]
  d_sp = [None if s is None else dev(s) for s in sps]
  lk(d_ids, d_sp, outs=outs, sp_weights=[None if w is None else dev(w) for w in ws])
  got = block.cpu().numpy()
  plain = GroupLookup([d_tables[c % 3] for c in range(n)], combiners=[combs[c % 3] for c in range(n)])
  unweighted = plain(d_ids, d_sp)
  for c in range(n):
    g = got[:, c * dim:(c + 1) * dim]
    if ws[c] is None:
      np.testing.assert_array_equal(g, unweighted[c].cpu().numpy())
    else:
      np.testing.assert_array_equal(g, ref_fwd(tables[c % 3], ids[c], sps[c], ws[c], combs[c % 3]))
  # the same tensors again without weights: the remembered call must not keep them
  lk(d_ids, d_sp, outs=outs)
  got = block.cpu().numpy()
  for c in range(n):
    np.testing.assert_array_equal(got[:, c * dim:(c + 1) * dim], unweighted[c].cpu().numpy())


# ---- 3. all-ones weights == unweighted ----------------------------------------------------------
@pytest.mark.parametrize('comb', ['sum', 'mean', 'sqrtn'])
def test_all_ones_equal_unweighted(comb):
  rng = np.random.RandomState(11)
  rows, dims = 5003, [16, 12, 64]
  tables = [rng.randn(rows, d).astype(F32) for d in dims]
  sps = [None, ragged(rng, 900), ragged(rng, 400, lam=6)]
  ids = [rng.zipf(1.2, size=900 if s is None else int(s[-1])) % rows for s in sps]
  ids = [i.astype(np.int64) for i in ids]
  ones = [dev(np.ones(i.size, F32)) for i in ids]
  d_ids = [dev(i) for i in ids]
  d_sp = [None if s is None else dev(s) for s in sps]
  grads = [dev(rng.randn(len(i) if s is None else s.size - 1, d).astype(F32))
           for i, s, d in zip(ids, sps, dims)]
  lk = GroupLookup([dev(t) for t in tables], combiners=comb)
  a = [o.cpu().numpy() for o in lk(d_ids, d_sp)]
  b = [o.cpu().numpy() for o in lk(d_ids, d_sp, sp_weights=ones)]
  for x, y in zip(a, b):
    np.testing.assert_array_equal(x, y)
  ga = [emitted(r) for r in GroupLookupGrad(lk, deterministic=True)(d_ids, grads, d_sp)]
  gb = [emitted(r) for r in GroupLookupGrad(lk, deterministic=True)(d_ids, grads, d_sp, sp_weights=ones)]
  for (ua, va), (ub, vb) in zip(ga, gb):
    np.testing.assert_array_equal(ua, ub)
    np.testing.assert_array_equal(va, vb)
  # stepped tables: SGD, Adagrad, the interleaved Adagrad layout
  for opt in ('sgd', 'adagrad', 'interleaved'):
    res = []
    for wts in (None, ones):
      tt = [dev(t) for t in tables]
      acc = [torch.full_like(t, 0.1) for t in tt]
      inter = [torch.cat([t, a_], 1).contiguous() for t, a_ in zip(tt, acc)]
      lk2 = GroupLookup(tt, combiners=comb)
      kw = dict(accums=acc) if opt == 'adagrad' else dict(interleaved=inter) if opt == 'interleaved' else {}
      GroupLookupGrad(lk2, deterministic=True, **kw)(
        d_ids, grads, d_sp, apply_lr=0.05, optimizer='sgd' if opt == 'sgd' else 'adagrad', sp_weights=wts)
      res.append([x.cpu().numpy() for x in (inter if opt == 'interleaved' else tt + acc)])
    for x, y in zip(*res):
      np.testing.assert_array_equal(x, y)


# ---- 4./5. backward emit with the plan switches; deterministic ---------------------------------
def _bwd_case(rng, zipf, rows=20011):
  dims = [16, 8, 3, 64]
  combs = ['mean', 'sqrtn', 'sum', 'mean']
  sps = [None, ragged(rng, 3000), ragged(rng, 2000, lam=8, cap=40), None]
  ids, ws, grads = [], [], []
  for c, s in enumerate(sps):
    k = 6000 if s is None else int(s[-1])
    i = (rng.zipf(1.2, size=k) * 7919) % (1 << 40) if zipf else rng.randint(0, 1 << 40, size=k)
    ids.append(i.astype(np.int64))
    w = rng.uniform(-0.5, 2, size=k).astype(F32)
    w[::97] = 0
    ws.append(w)
    grads.append(rng.randn(k if s is None else s.size - 1, dims[c]).astype(F32))
  tables = [rng.randn(rows, d).astype(F32) for d in dims]
  return dims, combs, sps, ids, ws, grads, tables, rows


SWITCHES = [('bwd_onepass', 0), ('bwd_onepass', 1), ('bwd_dense', 1), ('bwd_simple', 0), ('bwd_simple', 1),
            ('bwd_scale_fused', 0), ('bwd_scale_fused', 1), ('bwd_split_pairs', 64)]


@pytest.mark.parametrize('zipf', [False, True])
@pytest.mark.parametrize('switch', SWITCHES, ids=[f'{k}={v}' for k, v in SWITCHES])
def test_backward_emit_against_float64(hbk_option, switch, zipf):
  hbk_option(*switch)
  rng = np.random.RandomState(21 + zipf)
  dims, combs, sps, ids, ws, grads, tables, rows = _bwd_case(rng, zipf)
  lk = GroupLookup([dev(t) for t in tables], buckets=[rows] * 4, combiners=combs)
  res = GroupLookupGrad(lk)([dev(i) for i in ids], [dev(g) for g in grads],
                            [None if s is None else dev(s) for s in sps], sp_weights=[dev(w) for w in ws])
  for c in range(4):
    t, r, valid = ref_terms(rows, ids[c], sps[c], ws[c], combs[c], grads[c], bucket=rows)
    want, mag = dense_sums((rows, dims[c]), r[valid], t[valid])
    u, g = emitted(res[c])
    assert sorted(u.tolist()) == np.unique(r[valid]).tolist()
    assert_sums_close(g, want[u], mag[u], err_msg=f'col {c}')


@pytest.mark.parametrize('mode', [1, 2])
def test_deterministic_bit_equal(hbk_option, mode):
  hbk_option('bwd_deterministic', mode)
  rng = np.random.RandomState(31)
  dims, combs, sps, ids, ws, grads, tables, rows = _bwd_case(rng, True)
  lk = GroupLookup([dev(t) for t in tables], buckets=[rows] * 4, combiners=combs)
  args = ([dev(i) for i in ids], [dev(g) for g in grads], [None if s is None else dev(s) for s in sps])
  wts = [dev(w) for w in ws]
  runs = []
  for _ in range(2):
    runs.append([tuple(x.copy() for x in emitted(r)) for r in GroupLookupGrad(lk)(*args, sp_weights=wts)])
  for c in range(4):
    t, r, valid = ref_terms(rows, ids[c], sps[c], ws[c], combs[c], grads[c], bucket=rows)
    uniq, sums = seq_row_sums(t, r, valid)
    for run in runs:
      np.testing.assert_array_equal(run[c][0], uniq)
      np.testing.assert_array_equal(run[c][1], sums)


# ---- 6. fused steps -------------------------------------------------------------------------------
@pytest.mark.parametrize('opt', ['sgd', 'adagrad', 'step_only'])
def test_fused_steps(opt):
  rng = np.random.RandomState(41)
  dims, combs, sps, ids, ws, grads, tables, rows = _bwd_case(rng, True)
  tt = [dev(t) for t in tables]
  acc = [torch.full_like(t, 0.1) for t in tt]
  lk = GroupLookup(tt, buckets=[rows] * 4, combiners=combs)
  lr = 0.1
  GroupLookupGrad(lk, accums=acc)([dev(i) for i in ids], [dev(g) for g in grads],
                                  [None if s is None else dev(s) for s in sps], apply_lr=lr,
                                  optimizer='adagrad' if opt == 'adagrad' else 'sgd',
                                  emit=opt != 'step_only', sp_weights=[dev(w) for w in ws])
  for c in range(4):
    t, r, valid = ref_terms(rows, ids[c], sps[c], ws[c], combs[c], grads[c], bucket=rows)
    g, mag = dense_sums((rows, dims[c]), r[valid], t[valid])
    if opt == 'adagrad':
      a = 0.1 + g * g
      want = tables[c] - lr * g / np.sqrt(a)
      touched = np.zeros(rows, bool)
      touched[r[valid]] = True
      want[~touched] = tables[c][~touched]
      np.testing.assert_allclose(acc[c].cpu().numpy(), a, rtol=1e-4, atol=1e-5)
      np.testing.assert_allclose(tt[c].cpu().numpy(), want, rtol=1e-4, atol=1e-4)
    else:
      assert_sums_close(tt[c].cpu().numpy(), tables[c] - lr * g, np.abs(tables[c]) + lr * mag)


# ---- 7. torch's embedding_bag as a second implementation --------------------------------------------
def test_embedding_bag_sum():
  rng = np.random.RandomState(51)
  rows, dim = 10007, 32
  table = rng.randn(rows, dim).astype(F32)
  sp = ragged(rng, 2000, lam=5, cap=20)
  ids = rng.randint(0, rows, size=int(sp[-1])).astype(np.int64)
  w = rng.uniform(-1, 3, size=ids.size).astype(F32)
  got = hb.embedding.group_lookup([dev(table)], [dev(ids)], [dev(sp)], combiners='sum',
                                  sp_weights=[dev(w)])[0]
  want = torch.nn.functional.embedding_bag(dev(ids), dev(table), dev(sp[:-1].astype(np.int64)),
                                           mode='sum', per_sample_weights=dev(w))
  np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-5)


# ---- 8. sharded -------------------------------------------------------------------------------------
SHARDED = [(1, False, False, 1), (2, True, False, 1), (2, False, True, 0), (4, True, True, 1),
           (4, False, False, 0), (8, True, False, 0), (8, False, True, 1)]


@pytest.mark.parametrize('world,dedup,wire16,inline', SHARDED)
def test_sharded_equals_single_gpu(hbk_option, world, dedup, wire16, inline):
  hbk_option('sharded_inline', inline)
  rng = np.random.RandomState(600 + world)
  dims = [16, 8, 32, 4]
  rows = [50021, 211, 3000, 1009]
  combs = ['sum', 'mean', 'sqrtn', 'mean']
  n = len(dims)
  tables = [rng.uniform(-1, 1, size=(rows[c], dims[c])).astype(F32) for c in range(n)]
  ids, splits, grads, ws = [], [], [], []
  for _ in range(world):
    rid, rsp, rg, rw = [], [], [], []
    for c in range(n):
      sp = None if c % 2 == 0 else ragged(rng, int(rng.randint(1, 300)))
      k = int(rng.randint(0, 2000)) if sp is None else int(sp[-1])
      rsp.append(sp)
      rid.append(((rng.zipf(1.2, size=k) * 7919) % (1 << 40)).astype(np.int64))
      rw.append(rng.uniform(-0.5, 2, size=k).astype(F32))
      rg.append(rng.randn(k if sp is None else sp.size - 1, dims[c]).astype(F32))
    ids.append(rid)
    splits.append(rsp)
    grads.append(rg)
    ws.append(rw)
  comms = hb.distribute.Collective.local_world(world)
  shards = [[dev(t[r::world].copy()) for t in tables] for r in range(world)]
  results, errors = [None] * world, []
  lr = 0.25

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        drv = ShardedGroupLookup(shards[r], comms[r], buckets=rows, combiners=combs, dedup=[dedup] * n,
                                 wire_dtype=torch.float16 if wire16 else None)
        d_ids = [dev(i) for i in ids[r]]
        d_sp = [None if s is None else dev(s) for s in splits[r]]
        d_w = [dev(w) for w in ws[r]]
        outs = drv(d_ids, d_sp, sp_weights=d_w)
        slices = drv.backward([dev(g) for g in grads[r]], apply_lr=0.0)
        torch.cuda.current_stream().synchronize()
        first = [o.cpu().numpy().copy() for o in outs]
        emit = [tuple(x.copy() for x in emitted(s)) for s in slices]
        drv(d_ids, d_sp, sp_weights=d_w)
        drv.backward([dev(g) for g in grads[r]], apply_lr=lr, emit=False)
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
  eff = tables
  rel, floor = 1e-5, 1e-6
  if wire16:
    eff = [oracle.cast_f16_to_f32(oracle.cast_f32_to_f16(t)) for t in tables]
    rel, floor = WIRE16_REL, WIRE16_FLOOR
  for r in range(world):
    for c in range(n):
      np.testing.assert_array_equal(
        results[r][0][c], ref_fwd(eff[c], ids[r][c], splits[r][c], ws[r][c], combs[c], bucket=rows[c]))
  for c in range(n):
    want = np.zeros((rows[c], dims[c]))
    mag = np.zeros_like(want)
    for r in range(world):
      t, rr, valid = ref_terms(rows[c], ids[r][c], splits[r][c], ws[r][c], combs[c], grads[r][c],
                               bucket=rows[c])
      w_, m_ = dense_sums(want.shape, rr[valid], t[valid])
      want += w_
      mag += m_
    got = np.zeros_like(want)
    for r in range(world):
      lr_, g_ = results[r][1][c]
      assert len(set(lr_.tolist())) == len(lr_)
      got[lr_ * world + r] += g_
    assert_sums_close(got, want, mag, rel=rel, floor=floor, err_msg=f'col {c}')
    for r in range(world):
      assert_sums_close(shards[r][c].cpu().numpy(), tables[c][r::world].astype(np.float64) -
                        lr * want[r::world], (np.abs(tables[c]) + lr * mag)[r::world], rel=rel, floor=floor)
  for cm in comms:
    cm.close()


def test_sharded_p2p_bound_refuses_weights(hbk_option):
  hbk_option('sharded_p2p', 1)
  world = 2
  comms = hb.distribute.Collective.local_world(world)
  codes, errors = [None] * world, []

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        drv = ShardedGroupLookup([dev(np.zeros((50, 16), F32))], comms[r], buckets=[100])
        out = torch.zeros((8, 16), dtype=torch.float32, device=DEV)
        if not drv.p2p_bind([out]):
          codes[r] = 'unbound'
          return
        ids = dev(np.arange(8, dtype=np.int64))
        w = dev(np.ones(8, F32))
        a = (C_void_array([ids.data_ptr()]), _lib.i64_array([8]), C_void_array([None]),
             _lib.i64_array([8]), C_void_array([w.data_ptr()]), C_void_array([out.data_ptr()]))
        codes[r] = drv._lib.hbk_sharded_lookup_fwd_weighted(drv._plan(), a[0], a[1], a[2], a[3], a[4], a[5],
                                                            None, _lib.current_stream(DEV))
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
  if 'unbound' in codes:
    pytest.skip('peer memory could not be mapped: no p2p form to refuse in')
  assert codes == [_lib.UNIMPLEMENTED] * world
  for cm in comms:
    cm.close()


def C_void_array(ptrs):
  return _lib.ptr_array(ptrs)


# ---- 9. DenseFeatures -------------------------------------------------------------------------------
@pytest.mark.parametrize('world', [1, 2])
def test_dense_features_weighted_column(world):
  rng = np.random.RandomState(71)
  cols = [hb.feature_column.EmbeddingColumn('a', 5003, 16, 'mean', weight_feature_key='a_w'),
          hb.feature_column.EmbeddingColumn('b', 977, 8, 'sum')]
  batch = 256
  tables = [rng.uniform(-1, 1, size=(c.num_buckets, c.dimension)).astype(F32) for c in cols]
  feats = []
  for _ in range(world):
    sp = ragged(rng, batch)
    ia = rng.randint(0, 2**40, size=int(sp[-1])).astype(np.int64)
    feats.append({'a': (ia, sp), 'a_w': rng.uniform(0.1, 2, size=ia.size).astype(F32),
                  'b': rng.randint(0, 2**40, size=batch).astype(np.int64)})
  grads = [rng.randn(batch, 24).astype(F32) for _ in range(world)]
  comms = hb.distribute.Collective.local_world(world) if world > 1 else [None]
  results, errors = [None] * world, []
  lr = 0.1

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        def init(col, rows, device):
          t = tables[cols.index(col)]
          return dev(t[r::world].copy() if rows != col.num_buckets else t).to(device)
        layer = hb.feature_column.DenseFeatures(cols, DEV, comms[r], batch_size=batch, init=init,
                                                initial_accumulator_value=0.1)
        assert layer.sharded == [world > 1] * 2
        f = {k: (tuple(dev(x) for x in v) if isinstance(v, tuple) else dev(v)) for k, v in feats[r].items()}
        out = layer(f)
        layer.backward(dev(grads[r]), apply_lr=lr, optimizer='adagrad')
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
  for r in range(world):
    ia, sp = feats[r]['a']
    want_a = ref_fwd(tables[0], ia, sp, feats[r]['a_w'], 'mean', bucket=5003)
    want_b = oracle.group_lookup_fwd([tables[1]], [feats[r]['b']], [None], [977], ['sum'])[0]
    np.testing.assert_array_equal(results[r][0], np.concatenate([want_a, want_b], 1))
  # Adagrad on the weighted column's table
  g = np.zeros(tables[0].shape)
  mag = np.zeros_like(g)
  for r in range(world):
    ia, sp = feats[r]['a']
    t, rr, valid = ref_terms(5003, ia, sp, feats[r]['a_w'], 'mean',
                             np.ascontiguousarray(grads[r][:, :16]), bucket=5003)
    w_, m_ = dense_sums(g.shape, rr[valid], t[valid])
    g += w_
    mag += m_
  touched = mag.sum(1) > 0
  want = tables[0].astype(np.float64) - lr * g / np.sqrt(0.1 + g * g)
  want[~touched] = tables[0][~touched]
  got = np.zeros_like(want)
  for r in range(world):
    got[r::world] = results[r][1][0]
  np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)
  for cm in comms:
    if cm is not None:
      cm.close()


# ---- 10. captured graph -----------------------------------------------------------------------------
def test_weighted_inside_a_captured_graph():
  rng = np.random.RandomState(81)
  rows, dim = 4099, 16
  table = rng.randn(rows, dim).astype(F32)
  sp = ragged(rng, 512)
  ids = rng.randint(0, rows, size=int(sp[-1])).astype(np.int64)
  w = rng.uniform(-1, 2, size=ids.size).astype(F32)
  g = rng.randn(sp.size - 1, dim).astype(F32)
  d_ids, d_sp, d_w, d_g = dev(ids), dev(sp), dev(w), dev(g)
  lk = GroupLookup([dev(table)], combiners='mean')
  grad = GroupLookupGrad(lk, deterministic=True)
  out = torch.empty((sp.size - 1, dim), dtype=torch.float32, device=DEV)
  # warm-up outside the capture: descriptors, workspace and result buffers exist before it
  lk([d_ids], [d_sp], outs=[out], sp_weights=[d_w])
  res = grad([d_ids], [d_g], [d_sp], sp_weights=[d_w])
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      lk.launch()
      grad.launch()
  torch.cuda.synchronize()
  want = ref_fwd(table, ids, sp, w, 'mean')
  t, r, valid = ref_terms(rows, ids, sp, w, 'mean', g)
  uniq, sums = seq_row_sums(t, r, valid)
  for _ in range(3):
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    u, gr = emitted(res[0])
    np.testing.assert_array_equal(u, uniq)
    np.testing.assert_array_equal(gr, sums)


# ---- 11. full size ------------------------------------------------------------------------------------
def test_config2_weighted_full_size():
  rng = np.random.RandomState(91)
  n, rows, dim, batch = 26, 1 << 20, 16, 65536
  tables = [dev(rng.uniform(-1e-3, 1e-3, size=(rows, dim)).astype(F32)) for _ in range(n)]
  ids = [rng.randint(0, 2**40, size=batch).astype(np.int64) for _ in range(n)]
  ws = [rng.uniform(0.5, 2, size=batch).astype(F32) for _ in range(n)]
  grads = [rng.randn(batch, dim).astype(F32) for _ in range(n)]
  lk = GroupLookup(tables, buckets=[rows] * n, combiners='sum')
  d_ids = [dev(i) for i in ids]
  d_w = [dev(w) for w in ws]
  outs = lk(d_ids, sp_weights=d_w)
  for c in (0, 13, 25):
    np.testing.assert_array_equal(outs[c].cpu().numpy(),
                                  ref_fwd(tables[c].cpu().numpy(), ids[c], None, ws[c], 'sum', bucket=rows))
  before = [tables[c].cpu().numpy() for c in (0, 25)]
  lr = 0.5
  res = GroupLookupGrad(lk)(d_ids, [dev(g) for g in grads], apply_lr=lr, sp_weights=d_w)
  for k, c in enumerate((0, 25)):
    t, r, valid = ref_terms(rows, ids[c], None, ws[c], 'sum', grads[c], bucket=rows)
    g, mag = dense_sums((rows, dim), r[valid], t[valid])
    u, gr = emitted(res[c])
    assert_sums_close(gr, g[u], mag[u])
    assert_sums_close(tables[c].cpu().numpy(), before[k] - lr * g, np.abs(before[k]) + lr * mag)


# ---- launch batching: more weighted columns than one launch of each kernel holds -------------------
def test_many_weighted_columns_forward_backward_stitch():
  rng = np.random.RandomState(101)
  n, rows, dim = 140, 509, 8                     # > 128 weighted one-id columns: two forward launches
  table = rng.randn(rows, dim).astype(F32)
  d_table = dev(table)
  sps = [ragged(rng, 40) if c % 5 == 0 else None for c in range(n)]
  ids = [rng.randint(-3, rows + 3, size=40 if s is None else int(s[-1])).astype(np.int64) for s in sps]
  ws = [rng.uniform(-0.5, 2, size=i.size).astype(F32) for i in ids]
  grads = [rng.randn(i.size if s is None else s.size - 1, dim).astype(F32) for i, s in zip(ids, sps)]
  combs = [['sum', 'mean', 'sqrtn'][c % 3] for c in range(n)]
  d_ids = [dev(i) for i in ids]
  d_sp = [None if s is None else dev(s) for s in sps]
  d_w = [dev(w) for w in ws]
  lk = GroupLookup([d_table] * n, combiners=combs)
  outs = lk(d_ids, d_sp, sp_weights=d_w)
  for c in range(n):
    np.testing.assert_array_equal(outs[c].cpu().numpy(), ref_fwd(table, ids[c], sps[c], ws[c], combs[c]))
  # > 64 weighted gradient columns: several launches of the term pass; deterministic, bit-equal
  res = GroupLookupGrad(lk, deterministic=True)(d_ids, [dev(g) for g in grads], d_sp, sp_weights=d_w)
  for c in range(n):
    t, r, valid = ref_terms(rows, ids[c], sps[c], ws[c], combs[c], grads[c])
    uniq, sums = seq_row_sums(t, r, valid)
    u, g = emitted(res[c])
    np.testing.assert_array_equal(u, uniq)
    np.testing.assert_array_equal(g, sums)
  # hbk_group_stitch_bwd with > 128 weighted columns: grad_rows[index[j]] = t_j
  lib = _lib.lib()
  cols = (_lib.StitchGradColumn * n)()
  keep, outs = [], []
  for c in range(n):
    perm = rng.permutation(ids[c].size).astype(np.int32)
    d_perm, d_g = dev(perm), dev(grads[c])
    o = torch.full((ids[c].size, dim), float('nan'), device=DEV)
    keep += [d_perm, d_g]
    outs.append((perm, o))
    col = cols[c]
    col.dim, col.combiner, col.n_ids = dim, _lib.COMBINER_SUM + c % 3, ids[c].size
    col.index, col.row_splits = d_perm.data_ptr(), None if sps[c] is None else d_sp[c].data_ptr()
    col.n_segments = ids[c].size if sps[c] is None else sps[c].size - 1
    col.grad_out, col.grad_rows, col.id_weights = d_g.data_ptr(), o.data_ptr(), d_w[c].data_ptr()
  _lib.check(lib.hbk_group_stitch_bwd(n, cols, _lib.current_stream(DEV)))
  for c in range(n):
    # the stitch sees no owner range check: every id of a segment counts in its divisor
    t, _, _ = ref_terms(1 << 40, np.zeros(ids[c].size, np.int64), sps[c], ws[c], combs[c], grads[c])
    perm, o = outs[c]
    want = np.empty_like(t)
    want[perm] = t
    np.testing.assert_array_equal(o.cpu().numpy(), want, err_msg=f'col {c}')


def test_sharded_weighted_column_needs_a_bucket():
  comms = hb.distribute.Collective.local_world(1)
  drv = ShardedGroupLookup([dev(np.zeros((50, 16), F32))], comms[0])    # no bucket
  ids = dev(np.arange(8, dtype=np.int64))
  with pytest.raises(_lib.InvalidArgumentError, match='bucket'):
    drv([ids], sp_weights=[dev(np.ones(8, F32))])
  drv([ids])                                          # unweighted: as before
  torch.cuda.synchronize()
  drv.close()
  for cm in comms:
    cm.close()


def test_sharded_weighted_call_reuses_its_binding():
  comms = hb.distribute.Collective.local_world(1)
  rng = np.random.RandomState(111)
  table = rng.randn(1000, 16).astype(F32)
  drv = ShardedGroupLookup([dev(table)], comms[0], buckets=[1000], combiners='mean')
  sp = ragged(rng, 100)
  ids = rng.randint(0, 1 << 40, size=int(sp[-1])).astype(np.int64)
  d_ids, d_sp = dev(ids), dev(sp)
  out = torch.empty((100, 16), device=DEV)
  w1, w2 = dev(rng.uniform(0.5, 2, size=ids.size).astype(F32)), dev(rng.uniform(0.5, 2, size=ids.size).astype(F32))
  drv([d_ids], [d_sp], [out], sp_weights=[w1])
  bound = drv._call_cache[1]
  drv([d_ids], [d_sp], [out], sp_weights=[w1])
  assert drv._call_cache[1] is bound                  # same tensors, same weights: no rebind
  np.testing.assert_array_equal(out.cpu().numpy(), ref_fwd(table, ids, sp, w1.cpu().numpy(), 'mean', bucket=1000))
  drv([d_ids], [d_sp], [out], sp_weights=[w2])        # other weights: a new binding
  assert drv._call_cache[1] is not bound
  np.testing.assert_array_equal(out.cpu().numpy(), ref_fwd(table, ids, sp, w2.cpu().numpy(), 'mean', bucket=1000))
  drv([d_ids], [d_sp], [out])                         # unweighted again
  want = oracle.group_lookup_fwd([table], [ids], [sp], [1000], ['mean'])[0]
  np.testing.assert_array_equal(out.cpu().numpy(), want)
  drv.close()
  for cm in comms:
    cm.close()
