"""float64 restatement of the gradient of a weighted sparse lookup with respect to its per-id weights
(include/hbk.h, hbk_group_lookup_bwd_weights), with the magnitude of everything summed into each
element next to it -- what tests/support/tolerance.assert_sums_close needs.

Per id j of segment s: e_j the looked-up row after the column's clip, d_j = <G_s, e_j>,
A_s = sum w_i d_i, W_s = sum w_i, Q_s = sum w_i^2 over the segment's ids that map inside the table:

  sum    dw_j = d_j
  mean   dw_j = (d_j - A_s / W_s) / W_s
  sqrtn  dw_j = d_j / sqrt(Q_s) - w_j A_s / (Q_s sqrt(Q_s))

A zero divisor, an id outside the table and an id in no segment give 0."""
import numpy as np


def rows_of(ids, rows, bucket=0, divisor=1):
  ids = np.asarray(ids, np.int64)
  r = ids % bucket if bucket else ids.copy()
  r = np.where(r >= 0, r // divisor, -1)
  valid = (r >= 0) & (r < rows)
  return np.where(valid, r, 0), valid


def clipped_rows(table, max_norm):
  """x * c / max(|x|, c) of every row, in float64."""
  t = np.asarray(table, np.float64)
  if not max_norm:
    return t
  n = np.sqrt((t * t).sum(1, keepdims=True))
  return t * max_norm / np.maximum(n, max_norm)


def weight_grad(table, ids, splits, w, comb, grad, bucket=0, divisor=1, max_norm=None):
  """(dw, abs_sum, cancel): float64 [n_ids] gradient, the float64 sum of the absolute values of
  everything added into it, and per id the segment's |divisor| / sum|w| (mean) or 1 (else): how far
  the segment's divisor is from cancelling."""
  table = np.asarray(table)
  n = len(ids)
  r, valid = rows_of(ids, table.shape[0], bucket, divisor)
  sp = np.arange(n + 1) if splits is None else np.asarray(splits, np.int64)
  seg = np.full(n, -1, np.int64)
  for s in range(sp.size - 1):
    seg[sp[s]:sp[s + 1]] = s
  valid = valid & (seg >= 0)
  S = sp.size - 1
  e = clipped_rows(table, max_norm)[r]
  G = np.asarray(grad, np.float64)[np.maximum(seg, 0)]
  w = np.asarray(w, np.float64)
  d = np.where(valid, (G * e).sum(1), 0.0)
  ad = np.where(valid, np.abs(G * e).sum(1), 0.0)
  wv = np.where(valid, w, 0.0)
  sv = np.maximum(seg, 0)
  A = np.bincount(sv, wv * d, S)
  aA = np.bincount(sv, np.abs(wv) * ad, S)
  W = np.bincount(sv, wv, S)
  aW = np.bincount(sv, np.abs(wv), S)
  Q = np.bincount(sv, wv * wv, S)
  dw = np.zeros(n)
  mag = np.zeros(n)
  cancel = np.ones(n)
  if comb == 'sum':
    dw, mag = d.copy(), ad.copy()
  elif comb == 'mean':
    Wj, ok = W[sv], valid & (W[sv] != 0)
    with np.errstate(all='ignore'):
      dw = np.where(ok, (d - A[sv] / Wj) / Wj, 0.0)
      mag = np.where(ok, ad / np.abs(Wj) + aA[sv] / (Wj * Wj), 0.0)
      cancel = np.where(ok, np.abs(Wj) / np.maximum(aW[sv], 1e-300), 1.0)
  else:
    Qj, ok = Q[sv], valid & (Q[sv] != 0)
    with np.errstate(all='ignore'):
      rt = np.sqrt(Qj)
      dw = np.where(ok, d / rt - w * A[sv] / (Qj * rt), 0.0)
      mag = np.where(ok, ad / rt + np.abs(w) * aA[sv] / (Qj * rt), 0.0)
  dw[~valid] = 0.0
  mag[~valid] = 0.0
  return dw, mag, cancel


def forward(table, ids, splits, w, comb, bucket=0, divisor=1, max_norm=None):
  """The weighted lookup itself in float64: (out [segments, dim], abs_sum of the same shape: the
  magnitude of the terms of every element after the combiner's divisor)."""
  table = np.asarray(table)
  n = len(ids)
  r, valid = rows_of(ids, table.shape[0], bucket, divisor)
  sp = np.arange(n + 1) if splits is None else np.asarray(splits, np.int64)
  S = sp.size - 1
  e = clipped_rows(table, max_norm)[r]
  w = np.asarray(w, np.float64)
  out = np.zeros((S, table.shape[1]))
  mag = np.zeros_like(out)
  for s in range(S):
    j = np.arange(sp[s], sp[s + 1])
    j = j[valid[j]]
    if j.size == 0:
      continue
    div = 1.0 if comb == 'sum' else w[j].sum() if comb == 'mean' else np.sqrt((w[j] ** 2).sum())
    if div == 0:
      continue
    out[s] = (w[j][:, None] * e[j]).sum(0) / div
    mag[s] = np.abs(w[j][:, None] * e[j]).sum(0) / abs(div)
  return out, mag
