"""tests/support/exact.py pinned on the CPU: the budget rule, that fp32 sums of the generated data equal
float64 in every order, that ONE dropped or doubled term always changes bits, and -- the reason the helper
exists -- that the 1e-5 * sum|terms| bound of tests/support/tolerance.py lets dropped terms of a 50 000-term
row pass while the exact check lets none."""
import numpy as np
import pytest

from tests.support import exact
from tests.support.tolerance import assert_sums_close

F32 = np.float32


def _seq32(x):
  """The sequential fp32 sum of x [n, dim] along axis 0 (every add rounded to fp32)."""
  return np.cumsum(x, axis=0, dtype=F32)[-1]


def _pairwise32(x):
  return np.add.reduce(x, axis=0, dtype=F32)


def _chunked32(x, chunk=2048):
  """Chunks of 2048 terms summed one after the other, the chunk sums then merged."""
  parts = [_seq32(x[a:a + chunk]) for a in range(0, x.shape[0], chunk)]
  return _seq32(np.stack(parts))


ORDERS = {'sequential': _seq32, 'pairwise': _pairwise32, 'chunks of 2048, merged': _chunked32}


def test_budget_rule():
  one_row = np.zeros(50000, np.int64)                       # 50 000 terms: 16 bits
  assert exact.exact_terms_budget(one_row, 0) == 8
  assert exact.exact_terms_budget(one_row, 2) == 6          # mean over up to 4
  assert exact.exact_terms_budget(one_row, 5) == 3          # mean over up to 32: the last case that fits
  assert exact.exact_terms_budget(np.arange(100), 5) == 19  # every row once
  assert exact.exact_terms_budget(np.zeros(2048, np.int64), 0) == 13   # a power of two costs its log2
  assert exact.exact_terms_budget(np.zeros(2049, np.int64), 0) == 12
  assert exact.exact_terms_budget(np.zeros(0, np.int64), 5) == 19      # an empty column
  assert exact.exact_terms_budget(np.array([5, 1 << 40, 5]), 0) == 23  # row numbers of any size
  with pytest.raises(AssertionError, match='zipf head.*shrink'):
    exact.exact_terms_budget(np.zeros(70000, np.int64), 5, case='zipf head')
  assert exact.factor_bits('sum', 9) == 0 and exact.factor_bits('sum', 9, weighted=True) == 3
  assert exact.factor_bits('mean', 32) == 5 and exact.factor_bits('mean', 9) == 3
  assert exact.factor_bits('sqrtn', 32) == 2 and exact.factor_bits('sqrtn', 9) == 1
  assert exact.factor_bits('mean', 0) == 0


def test_generators_keep_their_promises():
  rng = np.random.RandomState(1)
  g = exact.exact_grads(rng, (40, 3), 5, frac_bits=4)
  assert g.dtype == F32 and (g == 0).any() and (g > 0).any() and (g < 0).any()
  assert np.abs(g).max() == 2.0 and (g * 16 == np.rint(g * 16)).all()
  for comb, allowed in (('mean', exact.MEAN_LENGTHS), ('sqrtn', exact.SQRTN_LENGTHS)):
    sp = exact.exact_ragged(rng, 500, comb, 32)
    lens = np.diff(sp)
    assert sp.dtype == np.int32 and sp[0] == 0 and set(lens.tolist()) == set(allowed)
    assert set(np.diff(exact.exact_ragged(rng, 300, comb, 9)).tolist()) == {x for x in allowed if x <= 9}
    np.testing.assert_array_equal(exact.snap_lengths(np.arange(40), comb),
                                  [max(x for x in allowed if x <= n) for n in range(40)])
    w = exact.exact_weights(rng, sp, int(sp[-1]), comb)
    f = exact.id_factors(sp, int(sp[-1]), comb, w)
    seg_len = np.repeat(lens, lens)
    want = 1.0 / seg_len if comb == 'mean' else 1.0 / np.sqrt(seg_len)
    np.testing.assert_array_equal(f, want)                   # the weights cancel: 1/len, 1/sqrt(len)
    assert set(np.unique(w).tolist()) == set(exact.SEGMENT_WEIGHTS)
  assert set(np.diff(exact.exact_ragged(rng, 300, 'sum', 5)).tolist()) == set(range(6))
  np.testing.assert_array_equal(exact.snap_lengths(np.arange(7), 'sum'), np.arange(7))
  w = exact.exact_weights(rng, None, 4000, 'sum')
  assert w.dtype == F32 and set(np.unique(w).tolist()) == set(exact.SUM_WEIGHTS)
  t = exact.exact_tables(rng, 50, 7)
  assert t.dtype == F32 and t.shape == (50, 7) and (t * 16 == np.rint(t * 16)).all()
  assert t.min() == -4.0 and t.max() == 63 / 16 and (t == 0).any()


def _hot_rows(rng, n, comb, max_len, dim=3, weighted=False):
  """One column whose first row receives ~n terms (three more rows share a few): ids, splits, weights,
  gradients by the budget, the terms per id."""
  sp = None if max_len is None else exact.exact_ragged(rng, n // max(max_len // 4, 1), comb, max_len)
  n_ids = n if sp is None else int(sp[-1])
  rows = np.where(rng.rand(n_ids) < 0.97, 0, rng.randint(1, 4, size=n_ids)).astype(np.int64)
  w = exact.exact_weights(rng, sp, n_ids, comb) if weighted else None
  bits = exact.exact_terms_budget(rows, exact.factor_bits(comb, max_len or 1, weighted), case=f'{comb} {n}')
  n_seg = n_ids if sp is None else sp.size - 1
  g = exact.exact_grads(rng, (n_seg, dim), bits)
  return rows, exact.id_terms(g, sp, comb, w)


@pytest.mark.parametrize('n,comb,max_len,weighted', [
  (100, 'sum', None, False), (8000, 'sum', None, True), (16000, 'mean', 32, False),
  (40000, 'mean', 4, True), (40000, 'sqrtn', 16, False), (30000, 'sqrtn', 16, True),
  (6161, 'sum', 9, False)])
def test_fp32_sums_in_any_order_equal_float64(n, comb, max_len, weighted):
  rng = np.random.RandomState(n)
  rows, terms = _hot_rows(rng, n, comb, max_len, weighted=weighted)
  want = exact.exact_dense((4, 3), rows, terms, case=f'{comb} {n}')
  assert want.counts[0] > 0.9 * rows.size and want.rows.tolist() == [0, 1, 2, 3]
  t32 = terms.astype(F32)
  assert (t32.astype(np.float64) == terms).all()
  for trial in range(3):
    perm = rng.permutation(rows.size)
    for name, order in ORDERS.items():
      got = np.stack([order(t32[perm][rows[perm] == r]) for r in range(4)])
      exact.assert_bits_equal(got, want.sums(), f'{name}, trial {trial}', unit=want.unit)


def test_exact_dense_refuses_inputs_that_are_not_exact():
  rng = np.random.RandomState(2)
  rows = np.zeros(5000, np.int64)
  g = exact.exact_grads(rng, (5000, 2), 8).astype(np.float64)
  exact.exact_dense((1, 2), rows, g)
  with pytest.raises(AssertionError, match='not below 2\\^24'):
    exact.exact_dense((1, 2), rows, g * 4096 + 2.0 ** -4, case='too many bits')
  with pytest.raises(AssertionError, match='no multiple of the grid'):
    exact.exact_dense((1, 2), rows, g / 3.0, q=2.0 ** -4)
  with pytest.raises(AssertionError, match='not below 2\\^24'):
    exact.exact_dense((1, 2), rows, rng.randn(5000, 2))      # N(0,1): the grid is 2^-50 or so
  with pytest.raises(AssertionError, match='outside the table'):
    exact.exact_dense((1, 2), rows + 1, g)
  with pytest.raises(AssertionError, match='fp16'):
    exact.exact_dense((1, 2), rows, g * 2.0 ** -4 + 2.0 ** -12, fp16=True)
  exact.exact_dense((1, 2), rows[:40], exact.exact_grads(rng, (40, 2), 6), fp16=True)
  empty = exact.exact_dense((3, 2), np.zeros(0, np.int64), np.zeros((0, 2)))
  assert empty.rows.size == 0 and not empty.dense.any()
  # a scatter-add INTO zeros: terms of -0.0 (a zero gradient under a negative weight) sum to +0.0
  zeros = exact.exact_dense((3, 2), np.array([1, 1, 2]), np.array([[-0.0, 1.0], [-0.0, -1.0], [-0.0, -0.0]]))
  assert zeros.rows.tolist() == [1, 2] and not zeros.dense.view(np.uint32).any()


def test_exact_sgd_checks_the_step_on_the_reference():
  rng = np.random.RandomState(3)
  rows = rng.randint(0, 5, size=3000)
  sums = exact.exact_dense((6, 4), rows, exact.exact_grads(rng, (3000, 4), 6))
  table = exact.exact_tables(rng, 6, 4)
  want = exact.exact_sgd(table, sums)
  # the same bits from separately rounded fp32 operations, whatever their association
  np.testing.assert_array_equal(want, table - F32(exact.EXACT_LR) * sums.dense)
  np.testing.assert_array_equal(want[5], table[5])           # no term: untouched
  with pytest.raises(AssertionError, match='power of two'):
    exact.exact_sgd(table, sums, lr=0.03)
  with pytest.raises(AssertionError, match='2\\^24'):
    exact.exact_sgd(table * F32(2.0 ** 20) + F32(1 / 16), sums)


def test_one_dropped_or_doubled_term_always_changes_bits():
  rng = np.random.RandomState(4)
  rows, terms = _hot_rows(rng, 20000, 'mean', 32)
  want = exact.exact_dense((4, 3), rows, terms)
  t32 = terms.astype(F32)
  hot = np.nonzero(rows == 0)[0]
  mag = np.abs(terms[hot])
  smallest = hot[np.argmin(np.where(mag > 0, mag, np.inf).min(axis=1))]
  low = np.abs(terms[smallest])
  assert low[low > 0].min() == want.unit[0] == 2.0 ** -9     # one gradient step of 1/16, mean over 32
  victims = [smallest] + [k for k in hot[rng.permutation(hot.size)] if terms[k].any()][:150]
  for name, order in ORDERS.items():
    for k in victims:
      perm = rng.permutation(hot.size)
      kept = hot[perm][hot[perm] != k]
      for what, sel in (('dropped', kept), ('doubled', np.concatenate([hot[perm], [k]]))):
        got = want.sums().copy()
        got[0] = order(t32[sel])
        with pytest.raises(AssertionError, match='x the smallest term of that row'):
          exact.assert_bits_equal(got, want.sums(), f'{name}: term {k} {what}', unit=want.unit, rows=want.rows)
  # the message names the place and the size of the damage
  got = want.sums().copy()
  got[0] = _pairwise32(t32[hot[hot != smallest]])
  lane = int(np.argmax(terms[smallest] != 0))
  sign = -np.sign(terms[smallest][lane]) * abs(terms[smallest][lane]) / want.unit[0]
  with pytest.raises(AssertionError, match=f'first at \\(0, {lane}\\) \\(row 0 \\(table row 0\\)\\).* = {sign:g} x the smallest'):
    exact.assert_bits_equal(got, want.sums(), 'smallest term dropped', unit=want.unit, rows=want.rows)


def test_assert_bits_equal_sees_signed_zero_and_nan():
  a = np.array([[0.0, 1.0]], F32)
  exact.assert_bits_equal(a, a.copy())
  with pytest.raises(AssertionError, match='0x80000000'):
    exact.assert_bits_equal(np.array([[-0.0, 1.0]], F32), a)          # == says equal; the bits do not
  nan = np.array([[np.nan, 1.0]], F32)
  exact.assert_bits_equal(nan, nan.copy())                            # the same NaN: the same bits
  other = nan.copy()
  other.view(np.uint32)[0, 0] ^= 1
  with pytest.raises(AssertionError, match='differ in their bits'):
    exact.assert_bits_equal(other, nan)
  with pytest.raises(AssertionError, match='differ in their bits'):
    exact.assert_bits_equal(nan, a)
  with pytest.raises(AssertionError, match='shape'):
    exact.assert_bits_equal(a, a[:, :1])
  with pytest.raises(AssertionError, match='not fp32'):
    exact.assert_bits_equal(a.astype(np.float64), a)


def test_the_loose_bound_misses_dropped_terms_of_a_hot_row_and_the_exact_check_misses_none():
  """A row of 50 000 N(0,1) terms (the Zipf head of a big fuzz column), ONE term dropped, the rest summed
  in fp32 in random order, 200 times: 1e-5 * sum|terms| + 1e-6 is ~0.40 there, so every dropped term
  smaller than that passes assert_sums_close (about a quarter of them).  The same experiment on the exact
  grid: assert_bits_equal fails every time."""
  rng = np.random.RandomState(0)
  n, trials = 50000, 200
  t = rng.randn(n, 1).astype(F32)
  want = t.astype(np.float64).sum(axis=0)
  mag = np.abs(t.astype(np.float64)).sum(axis=0)
  assert 0.35 < 1e-5 * mag[0] < 0.45
  passed = 0
  for k in range(trials):
    got = _pairwise32(np.delete(t, k, axis=0)[rng.permutation(n - 1)])
    try:
      assert_sums_close(got, want, mag, err_msg=f'term {k} dropped')
      passed += 1
    except AssertionError:
      pass
  print(f'loose bound: {passed} of {trials} dropped terms not noticed')
  assert passed >= trials // 10, passed         # measured: about a quarter; P(|N(0,1)| < 0.4) = 0.31
  # the exact grid at the same row size: 16 bits of count leave 8 value bits
  rows = np.zeros(n, np.int64)
  g = exact.exact_grads(rng, (n, 1), exact.exact_terms_budget(rows, 0))
  sums = exact.exact_dense((1, 1), rows, g)
  victims = np.nonzero(g[:, 0] != 0)[0][:trials]             # (a zero term adds nothing, lost or not)
  missed = 0
  for k in victims:
    got = _pairwise32(np.delete(g, k, axis=0)[rng.permutation(n - 1)])[None, :]
    try:
      exact.assert_bits_equal(got, sums.sums(), f'term {k} dropped', unit=sums.unit)
      missed += 1
    except AssertionError:
      pass
  assert victims.size == trials and missed == 0, missed
