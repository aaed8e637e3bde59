"""One plain restatement of the lookup, its backward and the optimizer steps, for the randomised feature
suite (tests/test_gpu_fuzz_features.py).

* float64 forward: ids -> rows (floormod by `bucket`, or with bucket 0 the ids themselves, dropped when
  negative or >= rows), TF's clip ``x * c / max(|x|, c)``, the per-id weight, the sum / mean / sqrtn
  combine; a segment whose divisor is 0 gives a zero row.  Returns (value, sum|terms|) for
  tolerance.assert_sums_close.
* float64 backward: per-id terms (weights and combiner factors) summed per distinct row, then, once per
  distinct row, the clip Jacobian at the pre-step row:
  ``g' = (c/n) (G - x (x.G) / n^2)`` outside the ball (n >= c, n > 0), ``G`` inside.
* fp32 step rules in include/hbk.h's operation order (every op a separately rounded fp32 op), so that a
  step can be compared bit for bit with the rule applied to the call's own IndexedSlices.  FTRL with
  lr_power not in {-0.5, 0} goes through powf, which is not correctly rounded: `ftrl_f64` gives the
  float64 step and the scales its ulp bound is taken against.

Divisors: an unweighted column divides by the segment's id count (invalid ids add zero rows, TF's GPU
gather), a weighted one by the weights of its VALID ids only (include/hbk.h, hbk_lookup_column_t).
"""
import numpy as np

F32 = np.float32
F64 = np.float64
COMBINERS = ('sum', 'mean', 'sqrtn')


# ---- ids, segments, factors ---------------------------------------------------------------------------
def rows_of(ids, rows, bucket=0):
  """(row of every id, valid mask): floormod by bucket, or the id itself when bucket == 0."""
  r = np.asarray(ids, np.int64)
  r = np.mod(r, bucket) if bucket else r.copy()
  valid = (r >= 0) & (r < rows)
  return np.where(valid, r, 0), valid


def segments_of(splits, n_ids):
  """(segment of every id, segment lengths); splits None = one id per segment."""
  if splits is None:
    return np.arange(n_ids), np.ones(n_ids, np.int64)
  lens = np.diff(np.asarray(splits, np.int64))
  return np.repeat(np.arange(lens.size), lens), lens


def factors64(splits, n_ids, weights, comb, valid):
  """(segment of every id, float64 factor of every id in its segment's output, number of segments,
  condition of every id's factor).  The factor is 0 for an invalid id and for every id of a segment
  whose divisor is 0.

  The condition: the kernels sum a weighted mean's divisor W_s over the segment's k valid ids in fp32,
  which is off by at most (k - 1) 2^-24 sum|w| -- relative to W_s, (k - 1) 2^-24 kappa with kappa =
  sum|w| / |W_s|, unbounded when signed weights cancel.  A term's error is then at most
  2^-24 |term| (k kappa + 2), inside tolerance.REL * |term| * cond with cond = 1 + k kappa (REL > 2^-23):
  the magnitude of a term is taken as |term| * cond.  Counts are exact and sqrtn's sum of squares has no
  cancellation (kappa = 1)."""
  seg, lens = segments_of(splits, n_ids)
  S = lens.size
  if weights is None:
    w = valid.astype(F64)
    cnt = lens.astype(F64)                      # (invalid ids count: they add zero rows)
    div = {'sum': np.ones(S), 'mean': cnt, 'sqrtn': np.sqrt(cnt)}[comb]
  else:
    w = np.where(valid, np.asarray(weights, F64), 0.0)
    if comb == 'sum':
      div = np.ones(S)
    elif comb == 'mean':
      div = np.bincount(seg, weights=w, minlength=S)
    else:
      div = np.sqrt(np.bincount(seg, weights=w * w, minlength=S))
  d = div[seg] if seg.size else np.zeros(0)
  f = np.where(d != 0, w / np.where(d != 0, d, 1.0), 0.0)
  cond = np.ones(seg.size)
  if weights is not None and comb != 'sum':
    k = np.bincount(seg, weights=valid.astype(F64), minlength=S)
    if comb == 'mean':
      absw = np.bincount(seg, weights=np.abs(w), minlength=S)
      kappa = np.where(div != 0, absw / np.where(div != 0, np.abs(div), 1.0), 0.0)
    else:
      kappa = np.ones(S)
    cond = 1.0 + (k * kappa)[seg]
  return seg, f, S, cond


# ---- float64 forward and backward ---------------------------------------------------------------------
def clip64(x, c):
  x = np.asarray(x, F64)
  if not c:
    return x
  n = np.sqrt((x * x).sum(1))
  return x * c / np.maximum(n, c)[:, None]


def forward64(table, ids, splits, weights, comb, max_norm=0.0, bucket=0):
  """The combined rows [segments, dim] in float64 and the sum of |terms| of every element."""
  r, valid = rows_of(ids, table.shape[0], bucket)
  seg, f, S, cond = factors64(splits, len(ids), weights, comb, valid)
  y = clip64(np.asarray(table, F64)[r], max_norm) * f[:, None]
  out = np.zeros((S, table.shape[1]))
  mag = np.zeros((S, table.shape[1]))
  if seg.size:
    np.add.at(out, seg, y)
    np.add.at(mag, seg, np.abs(y) * cond[:, None])
  return out, mag


def clip_jacobian64(x, G, M, c):
  """g' = J(x)^T G of every distinct row (x its pre-step row, G its summed gradient, M = sum|terms| of
  G) and the bound's sum|terms| of g'.  c = 0: no clip (G, M)."""
  x, G, M = np.asarray(x, F64), np.asarray(G, F64), np.asarray(M, F64)
  if not c:
    return G.copy(), M.copy()
  s = (x * x).sum(1)
  n = np.sqrt(s)
  m = np.maximum(n, c)
  out = (s > 0) & (n >= c)                       # (the tie n == c takes the radial term, as TF's max does)
  nn = np.where(s > 0, s, 1.0)
  scale = (c / m)[:, None]
  radial = x * ((x * G).sum(1) / nn)[:, None]
  gp = scale * (G - np.where(out[:, None], radial, 0.0))
  gm = scale * (M + np.where(out[:, None], np.abs(x) * ((np.abs(x) * M).sum(1) / nn)[:, None], 0.0))
  return gp, gm


def backward64(table, ids, splits, weights, comb, grad_out, max_norm=0.0, bucket=0):
  """(ascending distinct valid rows, g' [k, dim] float64, sum|terms| bound of g')."""
  r, valid = rows_of(ids, table.shape[0], bucket)
  seg, f, _, cond = factors64(splits, len(ids), weights, comb, valid)
  rr = r[valid]
  u, inv = np.unique(rr, return_inverse=True)
  terms = np.asarray(grad_out, F64)[seg[valid]] * f[valid][:, None]
  G = np.zeros((u.size, table.shape[1]))
  M = np.zeros((u.size, table.shape[1]))
  if u.size:
    np.add.at(G, inv, terms)
    np.add.at(M, inv, np.abs(terms) * cond[valid][:, None])
  gp, gm = clip_jacobian64(np.asarray(table, F64)[u], G, M, max_norm)
  return u, gp, gm


# ---- fp32 terms in id order (the deterministic modes' sums) --------------------------------------------
def terms32(table_rows, ids, splits, weights, comb, grad_out, bucket=0):
  """fp32 gradient term of every id as the kernels form it -- unweighted: g_s / count (mean),
  g_s / sqrtf(count) (sqrtn); weighted: (g_s / W_s) * w_j, (g_s / sqrtf(Q_s)) * w_j, g_s * w_j with W_s, Q_s
  summed in id order over the valid ids -- with the rows and validity of the ids."""
  r, valid = rows_of(ids, table_rows, bucket)
  seg, lens = segments_of(splits, len(ids))
  g = np.asarray(grad_out, F32)[seg]
  if weights is None:
    if comb != 'sum':
      d = lens.astype(F32) if comb == 'mean' else np.sqrt(lens.astype(F32))
      g = (g / d[seg][:, None]).astype(F32)
    return g, r, valid
  w = np.asarray(weights, F32)
  if comb != 'sum':
    S = lens.size
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    div = np.zeros(S, F32)
    for k in range(int(lens.max()) if lens.size else 0):
      s = np.nonzero(lens > k)[0]
      j = starts[s] + k
      keep = valid[j]
      s, j = s[keep], j[keep]
      div[s] = div[s] + (w[j] * w[j] if comb == 'sqrtn' else w[j])
    d = (div if comb == 'mean' else np.sqrt(div))[seg]
    g = np.where((d != 0)[:, None], g / np.where(d != 0, d, F32(1))[:, None], F32(0)).astype(F32)
  return (g * w[:, None]).astype(F32), r, valid


def seq_row_sums(terms, r, valid):
  """(ascending distinct valid rows, their sequential fp32 sums of `terms` in id order)."""
  rr, tt = r[valid], np.asarray(terms, F32)[valid]
  u, inv = np.unique(rr, return_inverse=True)
  out = np.zeros((u.size, tt.shape[1]), F32)
  for j in range(rr.size):          # (np.add.at on fp32 adds in index order, one rounding per add)
    out[inv[j]] = out[inv[j]] + tt[j]
  return u, out


# ---- fp32 step rules (include/hbk.h; sparse_apply.hip / lookup_bwd.hip) --------------------------------
def sgd_step(w, rows, g, lr):
  w[rows] = w[rows] - F32(lr) * np.asarray(g, F32)


def adagrad_step(w, a, rows, g, lr):
  g = np.asarray(g, F32)
  acc = a[rows] + g * g
  a[rows] = acc
  w[rows] = w[rows] - (F32(lr) * g) * (F32(1) / np.sqrt(acc))


ADAM_DEFAULTS = (F32(0.9), F32(0.999), F32(1e-8))


def adam_lr_t(lr, powers):
  b1p, b2p = F32(powers[0]), F32(powers[1])
  return F32(F32(F32(lr) * np.sqrt(F32(F32(1) - b2p))) / F32(F32(1) - b1p))


def adam_step(w, m, v, rows, g, lr, powers, b1=ADAM_DEFAULTS[0], b2=ADAM_DEFAULTS[1], eps=ADAM_DEFAULTS[2]):
  """Lazy Adam on the rows with the powers of this call; returns the powers after TF's _finish."""
  b1, b2, eps = F32(b1), F32(b2), F32(eps)
  lr_t = adam_lr_t(lr, powers)
  g = np.asarray(g, F32)
  mr = (b1 * m[rows]).astype(F32) + (F32(F32(1) - b1) * g).astype(F32)
  vr = (b2 * v[rows]).astype(F32) + (F32(F32(1) - b2) * (g * g)).astype(F32)
  m[rows] = mr
  v[rows] = vr
  w[rows] = w[rows] - (lr_t * mr) / (np.sqrt(vr) + eps)
  return adam_finish(powers, b1, b2)


def adam_finish(powers, b1=ADAM_DEFAULTS[0], b2=ADAM_DEFAULTS[1]):
  """TF's _finish: one fp32 product per power."""
  return F32(F32(powers[0]) * F32(b1)), F32(F32(powers[1]) * F32(b2))


def ftrl_exact(lr_power):
  """lr_power -0.5 (sqrtf) and 0 (powf(x, 0) = 1 exactly) are correctly rounded: bit-equal."""
  return F32(lr_power) in (F32(-0.5), F32(0))


def ftrl_step(w, a, z, rows, g, lr, l1, l2, l2_shrinkage, lr_power):
  lr, l1, l2 = F32(lr), F32(l1), F32(l2)
  shrink, lrp = F32(l2_shrinkage), F32(lr_power)
  g = np.asarray(g, F32)
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


def ftrl_f64(w, a, z, rows, g, lr, l1, l2, l2_shrinkage, lr_power):
  """The FTRL step in float64 from the same fp32 inputs: (w, accum, linear, scale of linear's terms,
  y) of the rows.  A powf-form step is held to K fp32 ulps of `scale` (linear) and of
  |w| + scale / y (w); accum is one fp32 add and stays bit-equal."""
  w, a, z, g = (np.asarray(x, F64) for x in (w[rows], a[rows], z[rows], g))
  lr, lrp = float(F32(lr)), float(F32(lr_power))
  shrink = float(F32(l2_shrinkage))
  gs = g if shrink == 0 else g + 2 * shrink * w
  na = a + g * g
  pn, po = na ** -lrp, a ** -lrp
  zn = z + (gs - (pn - po) / lr * w)
  y = pn / lr + 2 * float(F32(l2))
  l1 = float(F32(l1))
  wn = (np.clip(zn, -l1, l1) - zn) / y
  return wn, na, zn, np.abs(z) + np.abs(gs) + (pn + po) / lr * np.abs(w), y


FTRL_POWF_ULPS = 8     # test_gpu_ftrl.py::test_powf_form_within_a_few_ulps_of_float64
EPS32 = float(np.finfo(np.float32).eps)


def assert_ftrl_powf_close(got_w, got_z, w, a, z, rows, g, lr, l1, l2, l2_shrinkage, lr_power, err_msg=''):
  want_w, _, want_z, zscale, y = ftrl_f64(w, a, z, rows, g, lr, l1, l2, l2_shrinkage, lr_power)
  err_z = np.abs(np.asarray(got_z, F64) - want_z) / (EPS32 * np.maximum(zscale, 1e-300))
  err_w = np.abs(np.asarray(got_w, F64) - want_w) / (EPS32 * np.maximum(np.abs(want_w) + zscale / y, 1e-300))
  assert (err_z.size == 0 or err_z.max() <= FTRL_POWF_ULPS) and (err_w.size == 0 or err_w.max() <= FTRL_POWF_ULPS), \
      f'{err_msg}: powf FTRL {err_z.max():.2f} ulps (linear), {err_w.max():.2f} ulps (w)'
