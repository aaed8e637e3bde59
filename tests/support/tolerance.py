"""The ONE bound for comparing fp32 sums (deduplicated gradients, stepped tables) with a float64
reference.

An fp32 sum of n terms taken in ANY order differs from the exact sum by at most
(n - 1) * 2^-24 * sum|terms| -- a bound on the MAGNITUDE OF THE TERMS, not of the result.  A row
that sums 500 N(0,1) gradients to ~0.004 carries the rounding of the whole sum: holding it to
`rtol * |result| + fixed atol` fails on a run whose summation order differs (the backward takes
pair slots inside a row's run by LDS ticket atomics, so the order IS run-dependent; the reference's
TF path, `tf.math.unsorted_segment_sum` on a GPU, is not reproducible either).  BASELINE.json's
"within 1e-5 relative for the fp32 combiner" is therefore read as

    |got - want_f64| <= rel * sum|terms| + floor          (rel = 1e-5, floor = 1e-6)

everywhere a test compares such sums (VERDICT r05 "next round" 1a).  With sequential fp32 rounding
the actual error is ~0.5 * 2^-24 * sum|terms| ~ 3e-8 * sum|terms|: the bound leaves a factor of
> 100 and still catches one missing or doubled term of ordinary size (a term is ~1/n of
sum|terms|; 1e-5 * n < 1 for every n < 100 000).

What the bound cannot see: a missing or doubled term SMALLER than rel * sum|terms|, and on a hot row
that is a sizeable share of them.  Measured in numpy (tests/test_exact_support.py repeats the second
line as an assertion) -- fp32 sums in random order with ONE term of the row dropped, 200 trials:

    terms in the row                          term size    bound     dropped terms not noticed
    6 300   (skew='one' in the fuzz)          N(0,1)       0.050       6 of 200
    50 000  (Zipf head of a big fuzz column)  N(0,1)       0.40       54 of 200
    50 000  (mean over 4 ids)                 N(0,1)/4     0.099      57 of 200
    4 000   (mean over 32 ids)                N(0,1)/32    0.00099     9 of 200

Hot rows are where the reduce plans' special paths live (runs that cross shares, jobs of several chunks,
split buckets and their merge), and the step-only optimizer modes are compared through this bound on
every row that occurs more than once.  Those are pinned elsewhere, bit for bit: tests/support/exact.py
makes inputs whose fp32 sums are exact in any order, and tests/test_gpu_backward_exact.py and
test_group_lookup_random_plans_exact (tests/test_gpu_fuzz.py) hold every plan, the hot-row paths, the
step-only modes, the sequence pad row and the sharded owner reduce to the float64 result's bits.  This
bound stays for what the exact grid cannot express: arbitrary lengths and N(0,1) values.
"""
import os

import numpy as np

REL = 1e-5      # north_star: "within 1e-5 relative for the fp32 combiner"
FLOOR = 1e-6


def dense_sums(shape, index, terms):
  """float64 scatter-add of `terms` and of |terms| into zeros(shape) at rows `index`:
  (sum, abs_sum).  `terms` are the per-id gradient rows AFTER the combiner's factor."""
  t = np.asarray(terms, dtype=np.float64)
  want = np.zeros(shape, np.float64)
  mag = np.zeros(shape, np.float64)
  if t.size:
    np.add.at(want, index, t)
    np.add.at(mag, index, np.abs(t))
  return want, mag


def assert_sums_close(got, want_f64, abs_sum, rel=REL, floor=FLOOR, err_msg=''):
  """|got - want_f64| <= rel * abs_sum + floor, elementwise.  `abs_sum` = the float64 sum of the
  absolute values of everything that was added into the element (same shape as `want_f64`, or
  broadcastable); for a stepped table: |table| + lr * sum|gradient terms|."""
  got = np.asarray(got, dtype=np.float64)
  want = np.asarray(want_f64, dtype=np.float64)
  assert got.shape == want.shape, f'{err_msg}: shape {got.shape} vs {want.shape}'
  bound = rel * np.broadcast_to(np.asarray(abs_sum, np.float64), want.shape) + floor
  diff = np.abs(got - want)
  log = os.environ.get('HBK_TEST_RATIO_LOG')   # evidence runs: the worst |diff| / sum|terms| per check
  if log and diff.size:
    mag = np.broadcast_to(np.asarray(abs_sum, np.float64), want.shape)
    ratio = np.where(mag > 0, diff / np.maximum(mag, 1e-300), 0.0)
    w = np.unravel_index(np.argmax(ratio), ratio.shape)
    with open(log, 'a') as f:
      f.write(f'{os.getpid()} {err_msg!r} worst_ratio={ratio[w]:.3e} diff={diff[w]:.3e} '
              f'sum_abs={mag[w]:.4g} want={want[w]:.6g} n={diff.size}\n')
  bad = ~(diff <= bound)          # NaN-safe: a NaN anywhere is a failure
  if bad.any():
    worst = np.unravel_index(np.argmax(np.where(bad, diff / bound, 0.0)), diff.shape)
    raise AssertionError(
      f'{err_msg}: {int(bad.sum())} of {bad.size} elements outside {rel:g} * sum|terms| + '
      f'{floor:g}; worst at {tuple(int(i) for i in worst)}: got {got[worst]!r}, want '
      f'{want[worst]!r}, |diff| {diff[worst]:.3e} = {diff[worst] / max(np.broadcast_to(abs_sum, want.shape)[worst], 1e-300):.3e}'
      f' x sum|terms| ({np.broadcast_to(abs_sum, want.shape)[worst]:.4g}), bound {bound[worst]:.3e}')


def world_grad_sums(rows, dim, contributions, bucket=None):
  """The dense gradient of one table summed over every rank's batch, in float64, with the
  magnitude next to it: `contributions` = iterable of (ids, grad_out, row_splits | None, combiner),
  one per rank; d(combiner) per id follows oracle.segment_combine_grad (collective.py:334-347 is
  the exchange's gradient, the combiner's comes from TF).  Rows = ids mod `bucket` (default `rows`).
  Returns (sum, abs_sum), both [rows, dim]."""
  import oracle
  want = np.zeros((rows, dim), np.float64)
  mag = np.zeros((rows, dim), np.float64)
  for ids, grad_out, splits, combiner in contributions:
    sp = splits if splits is not None else np.arange(ids.size + 1, dtype=np.int32)
    g_id = oracle.segment_combine_grad(grad_out, sp, combiner).astype(np.float64)
    r = ids % (bucket or rows)
    np.add.at(want, r, g_id)
    np.add.at(mag, r, np.abs(g_id))
  return want, mag


WIRE16_REL = 2e-3   # fp16 wire: every contribution is rounded to 11 bits (2^-11 = 4.9e-4 of its own
                    # magnitude) by its sender, rows once more by their owner: <= 1e-3 * sum|terms|
WIRE16_FLOOR = 1e-5  # terms below the fp16 normal range (6e-5) carry one denormal step (6e-8) each
