"""Inputs whose fp32 sums are exact in ANY order, and the check that they are.

tests/support/tolerance.py bounds a run-dependent fp32 sum by 1e-5 * sum|terms|: on a row of many terms
that bound is wider than one term, so one pair lost or added twice at a chunk, share or merge boundary
can pass.  Here every per-id term is a multiple of one grid `q`, and for every output element
sum|terms| / q < 2^24.  Every partial sum -- in registers, in LDS, across chunks, in a merge, in any order
and association -- is then an integer multiple of q below 2^24 * q, which fp32 holds exactly.  The fp32
result must EQUAL the float64 one; a lost, doubled or misrouted term of any size changes bits.

The budget:  value_bits + factor_bits + ceil(log2(max terms per row)) <= 24

  value_bits   gradient values are integers in [-2^value_bits, 2^value_bits] times a power of two
  factor_bits  what the combiner adds: 1/len for a mean over len in {1, 2, 4, 8, 16, 32} (up to 5 bits),
               1/sqrt(len) for sqrtn over len in {1, 4, 16} (up to 2), the weights of exact_weights (3)

Everything is asserted on the REFERENCE (exact_dense, exact_sgd): a test whose inputs break the budget
fails loudly before any kernel result is looked at.  Pure numpy."""
import math

import numpy as np

MANTISSA = 24                       # fp32: integers up to 2^24 are exact
MIN_VALUE_BITS = 3
MEAN_LENGTHS = (0, 1, 2, 4, 8, 16, 32)   # 1/len is a power of two
SQRTN_LENGTHS = (0, 1, 4, 16)            # sqrt(len) is an integer power of two
SUM_WEIGHTS = (-2.0, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 2.0)
SEGMENT_WEIGHTS = (0.25, 0.5, 1.0, 2.0)  # positive: sum w and sqrt(sum w^2) over a set length are exact
WEIGHT_BITS = 3                          # SUM_WEIGHTS: two fraction bits (0.25) and one of magnitude (2)


def factor_bits(combiner, max_len, weighted=False):
  """The bits the combiner's factor costs for segments of up to `max_len` ids."""
  longest = max([x for x in lengths_of(combiner, max_len)] + [1])
  if combiner == 'sum':
    return WEIGHT_BITS if weighted else 0
  if combiner == 'mean':
    return int(math.log2(longest))          # w / (len * w) = 1 / len, weighted or not
  return int(math.log2(longest)) // 2       # sqrtn: w / (w * sqrt(len))


def lengths_of(combiner, max_len):
  """The segment lengths a combiner may see, up to max_len (sum: every length)."""
  if combiner == 'sum':
    return tuple(range(0, int(max_len) + 1))
  allowed = MEAN_LENGTHS if combiner in ('mean', None) else SQRTN_LENGTHS
  return tuple(x for x in allowed if x <= max_len)


def exact_terms_budget(ids_rows, factor_bits, case=''):  # pylint: disable=redefined-outer-name
  """How many bits remain for gradient values when the valid row numbers `ids_rows` (one per term)
  are summed per row after a combiner that costs `factor_bits`.  Fewer than 3: AssertionError naming
  `case` -- the case generator must shrink, a test never skips."""
  rows = np.asarray(ids_rows).reshape(-1)
  max_count = int(np.unique(rows, return_counts=True)[1].max()) if rows.size else 1
  count_bits = int(math.ceil(math.log2(max_count))) if max_count > 1 else 0
  value_bits = MANTISSA - int(factor_bits) - count_bits
  assert value_bits >= MIN_VALUE_BITS, (
    f'{case}: {max_count} terms in one row ({count_bits} bits) and {factor_bits} factor bits leave '
    f'{value_bits} value bits, fewer than {MIN_VALUE_BITS}: shrink the case')
  return value_bits


def exact_grads(rng, shape, value_bits, frac_bits=4):
  """fp32 integers in [-2^value_bits, 2^value_bits] times 2^-frac_bits.  Zero, the largest value and
  the smallest negative one are planted, so zeros and both signs occur whenever there are 3 values."""
  k = int(value_bits)
  ints = rng.randint(-(1 << k), (1 << k) + 1, size=shape).astype(np.int64)
  flat = ints.reshape(-1)
  if flat.size >= 3:
    flat[:3] = (0, 1 << k, -1)
  return (ints * 2.0 ** -int(frac_bits)).astype(np.float32)


def snap_lengths(lens, combiner):
  """Every length moved down to the nearest one the combiner's factor is exact for."""
  lens = np.asarray(lens, np.int64)
  if combiner == 'sum':
    return lens
  allowed = np.array(MEAN_LENGTHS if combiner in ('mean', None) else SQRTN_LENGTHS, np.int64)
  return allowed[np.searchsorted(allowed, np.minimum(lens, allowed[-1]), side='right') - 1]


def splits_of(lens):
  return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def exact_ragged(rng, n_seg, combiner, max_len):
  """int32 row_splits [n_seg + 1] with lengths from the combiner's set (lengths_of)."""
  allowed = np.array(lengths_of(combiner, max_len), np.int64)
  return splits_of(rng.choice(allowed, size=int(n_seg)))


def exact_weights(rng, row_splits, n_ids, combiner):
  """fp32 [n_ids] sp_weights.  sum: any of SUM_WEIGHTS per id.  mean / sqrtn: one of SEGMENT_WEIGHTS
  per SEGMENT (row_splits with lengths from the combiner's set), so that sum w = len * w and
  sqrt(sum w^2) = sqrt(len) * w are exact and the factor of every id is 1/len or 1/sqrt(len)."""
  if combiner == 'sum':
    return rng.choice(np.array(SUM_WEIGHTS, np.float32), size=int(n_ids))
  lens = np.diff(np.asarray(row_splits, np.int64))
  assert int(lens.sum()) == n_ids
  ok = np.isin(lens, MEAN_LENGTHS if combiner in ('mean', None) else SQRTN_LENGTHS)
  assert ok.all(), f'{combiner}: a segment length outside the exact set'
  per_seg = rng.choice(np.array(SEGMENT_WEIGHTS, np.float32), size=lens.size)
  return np.repeat(per_seg, lens).astype(np.float32)


def id_factors(row_splits, n_ids, combiner, weights=None):
  """float64 [n_ids]: d(combined row) / d(looked-up row) of every id -- w for sum, w / sum w for mean,
  w / sqrt(sum w^2) for sqrtn (w = 1 without weights; a segment whose divisor is 0 gives 0)."""
  w = np.ones(int(n_ids), np.float64) if weights is None else np.asarray(weights, np.float64)
  if combiner == 'sum':
    return w
  lens = np.diff(np.asarray(row_splits, np.int64)) if row_splits is not None else np.ones(int(n_ids), np.int64)
  seg = np.repeat(np.arange(lens.size), lens)
  if combiner in ('mean', None):
    div = np.bincount(seg, weights=w, minlength=lens.size)
  else:
    div = np.sqrt(np.bincount(seg, weights=w * w, minlength=lens.size))
  div = div.astype(np.float64)                  # (bincount of nothing counts in int64)
  inv = np.divide(1.0, div, out=np.zeros_like(div), where=div != 0)
  return w * inv[seg]


def id_terms(grads, row_splits, combiner, weights=None):
  """float64 [n_ids, dim]: the gradient term of every id (its segment's gradient row times its factor)."""
  g = np.asarray(grads, np.float64)
  if row_splits is None:
    n_ids, seg = g.shape[0], slice(None)
  else:
    lens = np.diff(np.asarray(row_splits, np.int64))
    n_ids, seg = int(lens.sum()), np.repeat(np.arange(lens.size), lens)
  return g[seg] * id_factors(row_splits, n_ids, combiner, weights)[:, None]


def _grid(values):
  """The largest power of two every value is a multiple of (1.0 when all are zero)."""
  v = np.asarray(values, np.float64).reshape(-1)
  v = v[v != 0]
  if not v.size:
    return 1.0
  assert np.isfinite(v).all(), 'a term is not finite'
  m, e = np.frexp(np.abs(v))
  x = (m * 2.0 ** 53).astype(np.int64)         # 53-bit integer mantissas
  low = x & -x                                  # lowest set bit
  return float(2.0 ** int((e - 53 + np.log2(low.astype(np.float64)).astype(np.int64)).min()))


class ExactSums:
  """What exact_dense returns: `rows` the distinct row numbers ascending, sums() fp32 [len(rows), dim]
  their sums, `dense` the same scattered into zeros [rows of the table, dim] (made when first asked for),
  `q` the grid, `unit` float64 [rows of the table] the smallest non-zero |term| added into each row (0
  where none) and `counts` the number of terms per row."""
  __slots__ = ('shape', 'rows', 'q', 'unit', 'counts', '_sums', '_dense')

  def sums(self):
    return self._sums

  @property
  def dense(self):
    if self._dense is None:
      self._dense = np.zeros(self.shape, np.float32)
      self._dense[self.rows] = self._sums
    return self._dense


def exact_dense(shape, rows, terms, q=None, fp16=False, case=''):
  """The float64 scatter-add of `terms` [n, dim] into zeros(shape) at `rows` [n] (all valid), plus the
  proof obligation, asserted on the reference alone: every term is a multiple of the grid q (derived
  when not given), sum|terms| / q < 2^24 for every element, and the float64 sums survive the cast to
  fp32.  fp16=True additionally asserts that every term round-trips through fp16 (a 16-bit wire)."""
  t = np.asarray(terms, np.float64)
  rows = np.asarray(rows, np.int64).reshape(-1)
  assert t.ndim == 2 and t.shape == (rows.size, shape[1]), f'{case}: terms {t.shape} for {rows.size} rows'
  assert not rows.size or (rows.min() >= 0 and rows.max() < shape[0]), f'{case}: a row outside the table'
  q = _grid(t) if q is None else float(q)
  scaled = t / q
  assert (scaled == np.rint(scaled)).all(), f'{case}: a term is no multiple of the grid {q!r}'
  if fp16:
    assert (t.astype(np.float16).astype(np.float64) == t).all(), f'{case}: a term does not survive fp16'
  out = ExactSums()
  out.shape, out.q, out._dense = tuple(shape), q, None
  out.unit = np.zeros(shape[0], np.float64)
  out.counts = np.bincount(rows, minlength=shape[0]) if rows.size else np.zeros(shape[0], np.int64)
  if not rows.size:
    out.rows, out._sums = np.zeros(0, np.int64), np.zeros((0, shape[1]), np.float32)
    return out
  order = np.argsort(rows, kind='stable')
  out.rows, starts = np.unique(rows[order], return_index=True)
  s = scaled[order]
  # integers < 2^53: exact in float64.  Added INTO zeros, as a scatter-add is: a row whose terms are all
  # -0.0 (a zero gradient under a negative weight) sums to +0.0
  want = np.add.reduceat(s, starts, axis=0) + 0.0
  mag = np.add.reduceat(np.abs(s), starts, axis=0)
  assert mag.max() < 2.0 ** MANTISSA, (
    f'{case}: sum|terms| / q reaches 2^{math.log2(mag.max()):.2f}, not below 2^{MANTISSA}')
  a = np.abs(t[order])
  a[a == 0] = np.inf
  unit = np.minimum.reduceat(a.min(axis=1), starts)
  out.unit[out.rows] = np.where(np.isfinite(unit), unit, 0.0)
  want *= q
  out._sums = want.astype(np.float32)
  assert (out._sums.astype(np.float64) == want).all(), f'{case}: a float64 sum is no fp32 value'
  return out


def exact_tables(rng, rows, dim, value_bits=6, frac_bits=4):
  """fp32 [rows, dim] on the grid 2^-frac_bits, integers in [-2^value_bits, 2^value_bits) times it
  (|w| <= 4.0 by default).  From the generator's bytes: tables of 10^7 values in a blink."""
  k = int(value_bits)
  assert 0 <= k <= 7
  ints = np.frombuffer(rng.bytes(int(rows) * int(dim)), np.int8) >> (7 - k)     # (arithmetic shift)
  return ints.reshape(int(rows), int(dim)).astype(np.float32) * np.float32(2.0 ** -int(frac_bits))


EXACT_LR = 0.125   # a power of two: lr * sum is exact, so w - lr * sum is the same with or without an FMA


def exact_sgd(table, sums, lr=EXACT_LR, case=''):
  """exact_dense's sibling for a stepped table: w - lr * sums in float64 with, asserted on the reference,
  lr a power of two, every w and every lr * sum a multiple of one grid and |w|, |lr * sum| and
  |w - lr * sum| all below 2^24 grids.  `sums`: an ExactSums.  Returns the fp32 table."""
  m, _ = math.frexp(lr)
  assert m == 0.5, f'{case}: lr {lr!r} is no power of two'
  table = np.asarray(table)
  assert table.dtype == np.float32
  w = table[sums.rows].astype(np.float64)        # (rows without a term are copied: nothing to prove)
  step = lr * sums.sums().astype(np.float64)
  grid = min(_grid(w), lr * sums.q)
  want = w - step
  for name, x in (('w', w), ('lr * sum', step), ('w - lr * sum', want)):
    s = x / grid
    assert (s == np.rint(s)).all(), f'{case}: {name} off the grid {grid!r}'
    assert np.abs(s).max(initial=0.0) < 2.0 ** MANTISSA, f'{case}: |{name}| / grid reaches 2^24'
  out = table.copy()
  out[sums.rows] = want.astype(np.float32)
  assert (out[sums.rows].astype(np.float64) == want).all(), f'{case}: a stepped weight is no fp32 value'
  return out


def assert_bits_equal(got, want, err_msg='', unit=None, rows=None):
  """got and want (fp32, same shape) compared as uint32: -0.0 / +0.0 differ, a NaN equals only the
  same NaN.  On a mismatch: the first differing (row, lane), both values and -- with `unit` [rows of
  got], the smallest term of each row -- the difference in multiples of that term (1: a pair lost or
  added twice; a large multiple: a pair from another row).  `rows`: the table row of each row of got."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == np.float32 and want.dtype == np.float32, f'{err_msg}: {got.dtype} vs {want.dtype}, not fp32'
  assert got.shape == want.shape, f'{err_msg}: shape {got.shape} vs {want.shape}'
  g = np.ascontiguousarray(got).view(np.uint32)
  w = np.ascontiguousarray(want).view(np.uint32)
  bad = g != w
  if not bad.any():
    return
  at = tuple(int(i) for i in np.argwhere(bad)[0])
  diff = float(got[at]) - float(want[at])
  where = f'row {at[0]}' if rows is None or not at else f'row {at[0]} (table row {int(np.asarray(rows)[at[0]])})'
  msg = (f'{err_msg}: {int(bad.sum())} of {bad.size} elements differ in their bits; first at {at} ({where}): '
         f'got {got[at]!r} (0x{int(g[at]):08x}), want {want[at]!r} (0x{int(w[at]):08x}), difference {diff!r}')
  if unit is not None and at:
    u = float(np.asarray(unit)[at[0]])
    if u > 0:
      msg += f' = {diff / u:g} x the smallest term of that row ({u!r})'
  raise AssertionError(msg)
