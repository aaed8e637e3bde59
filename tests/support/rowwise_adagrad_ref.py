"""Row-wise Adagrad restated in numpy fp32 (include/hbk.h, hbk_group_lookup_bwd_rowwise_adagrad): from the
deduplicated gradient g of every distinct row, each operation a separately rounded fp32 operation,

    s    = sum_k g_k * g_k          the row split into lane chunks, then a butterfly (row_sum_sq)
    a'   = a + s / (float)dim
    m    = lr / (sqrtf(a') + epsilon)
    w_k  = w_k - m * g_k
    a    = a'

The order of s depends on (dim, vec4) only: vec4 -- dim % 4 == 0 and table, grad_rows and the pitch 16-byte
aligned -- sums chunks of 4 floats ((x0 + x1) + x2) + x3 per lane, the scalar path has one float per lane;
the L = 2^ceil(log2(chunks)) partial sums (lanes past dim give +0.0) meet in p[i] = p[i] + p[i ^ o] for
o = 1, 2, 4, .. < L.  Pure numpy; float64 twins for the tolerance-bound tests."""
import numpy as np

F32 = np.float32


def is_vec4(dim, aligned=True):
  """The row shape the kernels take: 4-float chunks need dim % 4 == 0 and 16-byte aligned rows."""
  return bool(aligned) and dim % 4 == 0


def row_sum_sq(g, vec4):
  """fp32 [n]: s of every row of g fp32 [n, dim], in the documented order."""
  g = np.asarray(g)
  assert g.dtype == F32 and g.ndim == 2
  n, dim = g.shape
  sq = (g * g).astype(F32)
  if vec4:
    assert dim % 4 == 0
    p = ((sq[:, 0::4] + sq[:, 1::4]).astype(F32) + sq[:, 2::4]).astype(F32) + sq[:, 3::4]
    p = p.astype(F32)
  else:
    p = sq
  chunks = p.shape[1]
  lanes = 1
  while lanes < chunks:
    lanes *= 2
  full = np.zeros((n, lanes), F32)
  full[:, :chunks] = p
  lane = np.arange(lanes)
  o = 1
  while o < lanes:
    full = (full + full[:, lane ^ o]).astype(F32)
    o *= 2
  return full[:, 0].copy()


def step(w, a, rows, g, lr, eps, vec4):
  """One step in place: w fp32 [R, dim], a fp32 [R, 1], rows int64 [n] distinct, g fp32 [n, dim]."""
  rows = np.asarray(rows, np.int64)
  assert np.unique(rows).size == rows.size, 'a row twice: the step is not additive'
  g = np.asarray(g, F32)
  dim = w.shape[1]
  s = row_sum_sq(g, vec4)
  na = (a[rows, 0] + (s / F32(dim)).astype(F32)).astype(F32)
  m = (F32(lr) / (np.sqrt(na).astype(F32) + F32(eps)).astype(F32)).astype(F32)
  w[rows] = (w[rows] - (m[:, None] * g).astype(F32)).astype(F32)
  a[rows, 0] = na


def step64(w, a, rows, g, lr, eps):
  """The same formula in float64 (no order: the tolerance tests' reference).  Returns (w rows, a rows)."""
  g = np.asarray(g, np.float64)
  dim = w.shape[1]
  na = a[rows, 0].astype(np.float64) + (g * g).sum(axis=1) / dim
  m = float(lr) / (np.sqrt(na) + float(eps))
  return w[rows].astype(np.float64) - m[:, None] * g, na
