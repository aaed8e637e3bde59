"""tests/support/reference.py against the C oracle, a float64 central difference and the fp32 step
restatements of the feature tests (CPU only: runs without a GPU)."""
import numpy as np
import pytest

import oracle
from tests.support import reference as ref

F32, F64 = np.float32, np.float64


def _ragged(rng, n_seg, max_len=7):
  lens = rng.randint(0, max_len + 1, size=n_seg)
  return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


@pytest.mark.parametrize('comb', ref.COMBINERS)
@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('bucket', [0, 1])
def test_unweighted_unclipped_against_oracle(comb, ragged, bucket):
  rng = np.random.RandomState(ref.COMBINERS.index(comb) * 4 + 2 * ragged + bucket)
  rows, dim = 97, 5
  table = rng.uniform(-1, 1, size=(rows, dim)).astype(F32)
  sp = _ragged(rng, 300) if ragged else None
  n = int(sp[-1]) if ragged else 400
  if bucket:
    ids = rng.randint(-2**40, 2**40, size=n).astype(np.int64)
    bucket = rows
  else:   # ids as rows, some negative or past the table: they add zero rows and no gradient
    ids = rng.randint(-20, rows + 20, size=n).astype(np.int64)
  want = oracle.group_lookup_fwd([table], [ids], [sp], [bucket], [comb])[0]
  got, mag = ref.forward64(table, ids, sp, None, comb, bucket=bucket)
  np.testing.assert_allclose(got, want, rtol=0, atol=1e-6 * (1 + mag.max()))
  assert np.all(mag >= np.abs(got))
  g_out = rng.randn(n if sp is None else sp.size - 1, dim).astype(F32)
  splits = sp if sp is not None else np.arange(n + 1, dtype=np.int32)
  g_id = oracle.segment_combine_grad(g_out, splits, comb)
  terms, r, valid = ref.terms32(rows, ids, sp, None, comb, g_out, bucket)
  np.testing.assert_array_equal(terms, g_id)             # the fp32 terms, bit for bit
  u, seq = ref.seq_row_sums(terms, r, valid)
  want_u = np.unique(r[valid])
  np.testing.assert_array_equal(u, want_u)
  np.testing.assert_array_equal(
    seq, oracle.unsorted_segment_sum(g_id[valid], np.searchsorted(want_u, r[valid]).astype(np.int32), u.size))
  u64, gp, gm = ref.backward64(table, ids, sp, None, comb, g_out, bucket=bucket)
  np.testing.assert_array_equal(u64, want_u)
  want64 = oracle.unsorted_segment_sum(g_id[valid], np.searchsorted(want_u, r[valid]).astype(np.int32),
                                       u.size, f64=True)
  np.testing.assert_allclose(gp, want64, rtol=0, atol=1e-6 * (1 + gm.max()))


@pytest.mark.parametrize('comb', ref.COMBINERS)
def test_weighted_terms_sum_to_the_float64_backward(comb):
  rng = np.random.RandomState(40 + ref.COMBINERS.index(comb))
  rows, dim = 31, 3
  table = rng.uniform(-1, 1, size=(rows, dim)).astype(F32)
  sp = _ragged(rng, 200)
  n = int(sp[-1])
  ids = rng.randint(-5, rows + 5, size=n).astype(np.int64)
  w = rng.uniform(-1, 2, size=n).astype(F32)
  w[sp[3]:sp[4]] = 0                                     # a segment of zero weight: a zero row
  g_out = rng.randn(sp.size - 1, dim).astype(F32)
  terms, r, valid = ref.terms32(rows, ids, sp, w, comb, g_out)
  u, seq = ref.seq_row_sums(terms, r, valid)
  u64, gp, gm = ref.backward64(table, ids, sp, w, comb, g_out)
  np.testing.assert_array_equal(u, u64)
  assert np.all(np.abs(seq - gp) <= 1e-5 * gm + 1e-6)
  out, _ = ref.forward64(table, ids, sp, w, comb)
  np.testing.assert_array_equal(out[3], 0)


@pytest.mark.parametrize('dim', [1, 2, 5, 16])
def test_clip_jacobian_against_central_difference(dim):
  """g' = J(x)^T G with J = d clip(x) / dx, for rows inside, on and outside the ball."""
  rng = np.random.RandomState(dim)
  c = 0.5
  for scale in (0.3, 0.9, 1.7, 4.0):
    x = rng.randn(dim)
    x *= scale * c / np.linalg.norm(x)
    G = rng.randn(dim)
    h = 1e-6
    J = np.zeros((dim, dim))
    for k in range(dim):
      e = np.zeros(dim)
      e[k] = h
      J[:, k] = (ref.clip64((x + e)[None], c)[0] - ref.clip64((x - e)[None], c)[0]) / (2 * h)
    gp, gm = ref.clip_jacobian64(x[None], G[None], np.abs(G)[None], c)
    np.testing.assert_allclose(gp[0], J.T @ G, rtol=1e-6, atol=1e-8)
    assert np.all(gm[0] >= np.abs(gp[0]) * (1 - 1e-12))
  # the tie [c, 0, ..]: the one-sided derivative of TF's max (gradient to the norm at equality)
  x = np.zeros(dim)
  x[0] = c
  G = rng.randn(dim)
  gp, _ = ref.clip_jacobian64(x[None], G[None], np.abs(G)[None], c)
  want = G.copy()
  want[0] = 0.0
  np.testing.assert_allclose(gp[0], want, atol=1e-15)
  # the zero row and no clip
  gp, _ = ref.clip_jacobian64(np.zeros((1, dim)), G[None], np.abs(G)[None], c)
  np.testing.assert_array_equal(gp[0], G)
  gp, _ = ref.clip_jacobian64(x[None] * 3, G[None], np.abs(G)[None], 0.0)
  np.testing.assert_array_equal(gp[0], G)


def _state(rng, rows, dim):
  w = rng.uniform(-1, 1, size=(rows, dim)).astype(F32)
  s0 = rng.uniform(0.1, 1, size=(rows, dim)).astype(F32)
  s1 = rng.uniform(-0.5, 0.5, size=(rows, dim)).astype(F32)
  return w, s0, s1


@pytest.mark.parametrize('seed', range(4))
def test_sgd_and_adagrad_bit_equal_to_the_oracle(seed):
  rng = np.random.RandomState(seed)
  w, a, _ = _state(rng, 300, 7)
  rows = rng.choice(300, size=120, replace=False).astype(np.int64)
  g = (rng.randn(120, 7) * 10 ** rng.uniform(-3, 2)).astype(F32)
  w1, w2 = w.copy(), w.copy()
  ref.sgd_step(w1, rows, g, 0.03)
  oracle.sparse_sgd_apply(w2, rows, g, 0.03)
  np.testing.assert_array_equal(w1, w2)
  (w1, a1), (w2, a2) = (w.copy(), a.copy()), (w.copy(), a.copy())
  ref.adagrad_step(w1, a1, rows, g, 0.03)
  oracle.sparse_adagrad_apply(w2, a2, rows, g, 0.03)
  np.testing.assert_array_equal(w1, w2)
  np.testing.assert_array_equal(a1, a2)


def _feature_module(name):
  """The restatements of an existing GPU feature test, loaded without running its module-level GPU
  marks (the helpers themselves are plain numpy)."""
  import importlib
  pytest.importorskip('torch')
  return importlib.import_module(f'tests.{name}')


@pytest.mark.parametrize('seed', range(4))
def test_adam_bit_equal_to_the_adam_tests_restatement(seed):
  mod = _feature_module('test_gpu_adam')
  rng = np.random.RandomState(10 + seed)
  w, _, _ = _state(rng, 200, 9)
  m = rng.uniform(-0.1, 0.1, size=w.shape).astype(F32)
  v = rng.uniform(0, 0.01, size=w.shape).astype(F32)
  rows = rng.choice(200, size=80, replace=False).astype(np.int64)
  g = rng.randn(80, 9).astype(F32)
  powers = (F32(0.9 ** (seed + 1)), F32(0.999 ** (seed + 1)))
  a, b = [x.copy() for x in (w, m, v)], [x.copy() for x in (w, m, v)]
  p1 = ref.adam_step(*a, rows, g, 0.05, powers)
  p2 = mod.np_adam(*b, rows, g, 0.05, powers[0], powers[1])
  for x, y in zip(a, b):
    np.testing.assert_array_equal(x, y)
  assert p1 == p2


@pytest.mark.parametrize('cfg', [(0.0, 0.0, 0.0, -0.5), (2.0, 1e-5, 0.0, -0.5), (0.0, 1e-5, 0.01, -0.5),
                                 (2.0, 0.0, 0.01, 0.0), (0.5, 1e-3, 0.02, -0.3), (0.0, 0.0, 0.0, -1.0)])
def test_ftrl_bit_equal_to_the_ftrl_tests_restatement(cfg):
  mod = _feature_module('test_gpu_ftrl')
  from hybridbackend_amd.embedding.optimizer import Ftrl
  l1, l2, shrink, lrp = cfg
  rng = np.random.RandomState(int(1000 * (l1 + l2 + shrink - lrp)))
  w, a, _ = _state(rng, 200, 6)
  z = rng.uniform(-4, 4, size=w.shape).astype(F32)
  rows = rng.choice(200, size=90, replace=False).astype(np.int64)
  g = rng.randn(90, 6).astype(F32)
  x, y = [t.copy() for t in (w, a, z)], [t.copy() for t in (w, a, z)]
  ref.ftrl_step(*x, rows, g, 0.07, l1, l2, shrink, lrp)
  mod.np_ftrl(*y, rows, g, 0.07, Ftrl(l1=l1, l2=l2, l2_shrinkage=shrink, lr_power=lrp))
  for p, q in zip(x, y):
    np.testing.assert_array_equal(p, q)
  # numpy's pow is within the powf bound of the float64 step too
  ref.assert_ftrl_powf_close(x[0][rows], x[2][rows], w, a, z, rows, g, 0.07, l1, l2, shrink, lrp)
