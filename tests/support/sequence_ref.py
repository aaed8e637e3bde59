"""A numpy restatement of the sequence lookup (include/hbk.h, hbk_group_lookup_fwd_sequence): the id
grid, the lengths, the output by plain indexing -- no arithmetic besides the clip, in float64 -- and the
gradient as a float64 scatter over the grid."""
import numpy as np


def grid_ref(ids, row_splits, bucket, max_len, pad_id=None):
  """(grid int64 [B * T], lengths int32 [B]).  A sample's first T ids, floor-mod `bucket` (Python's %)
  when bucket > 0, else kept (a negative one: -1); past the sample's length: pad_id mapped the same way,
  or -1."""
  ids = np.asarray(ids).astype(np.int64)
  T = int(max_len)
  if row_splits is None:
    splits = np.arange(ids.size + 1, dtype=np.int64)
  else:
    splits = np.asarray(row_splits).astype(np.int64)
  B = splits.size - 1
  lengths = np.minimum(np.diff(splits), T)
  t = np.arange(T)[None, :]
  valid = t < lengths[:, None]
  src = np.where(valid, splits[:-1, None] + t, 0)
  padded = np.concatenate([ids, [0]])          # (ids may be empty)
  pad = -1 if pad_id is None else int(pad_id)
  raw = np.where(valid, padded[src], pad)
  looked = valid | (pad_id is not None)
  if bucket:
    g = np.where(looked, raw % int(bucket), -1)
  else:
    g = np.where(looked & (raw >= 0), raw, -1)
  return g.reshape(B * T).astype(np.int64), lengths.astype(np.int32)


def rows_ref(grid, rows, divisor=1):
  """The table row of every position, -1 where nothing is read (a zero row)."""
  grid = np.asarray(grid, np.int64)
  r = grid // int(divisor)
  return np.where((grid >= 0) & (r < rows), r, -1)


def forward_ref(table, grid, max_len, divisor=1, max_norm=None):
  """out [B, T, dim]: fp32 by plain indexing; with max_norm the float64 clip x * c / max(|x|, c) of
  every looked-up row, and next to it the |terms| of tests/support/tolerance.py's bound."""
  table = np.asarray(table)
  r = rows_ref(grid, table.shape[0], divisor)
  dim = table.shape[1]
  if not max_norm:
    out = np.zeros((r.size, dim), np.float32)
    out[r >= 0] = table[r[r >= 0]]
    return out.reshape(-1, int(max_len), dim)
  x = np.zeros((r.size, dim), np.float64)
  x[r >= 0] = table[r[r >= 0]].astype(np.float64)
  n = np.sqrt((x * x).sum(1))
  y = x * max_norm / np.maximum(n, max_norm)[:, None]
  return y.reshape(-1, int(max_len), dim), np.abs(y).reshape(-1, int(max_len), dim)


def grad_ref(grid, grad_out, rows, divisor=1):
  """(unique rows ascending, float64 sums [u, dim], float64 sums of |terms|) of the [B, T, dim]
  gradient scattered over the grid's rows."""
  g = np.asarray(grad_out, np.float64)
  g = g.reshape(-1, g.shape[-1])
  r = rows_ref(grid, rows, divisor)
  keep = r >= 0
  u, inv = np.unique(r[keep], return_inverse=True)
  want = np.zeros((u.size, g.shape[1]), np.float64)
  mag = np.zeros_like(want)
  np.add.at(want, inv, g[keep])
  np.add.at(mag, inv, np.abs(g[keep]))
  return u, want, mag


def grad_seq32(grid, grad_out, rows, divisor=1):
  """The same sums in fp32, every row's terms added one by one in position order (what the
  deterministic backward must reproduce bit for bit)."""
  g = np.asarray(grad_out, np.float32)
  g = g.reshape(-1, g.shape[-1])
  r = rows_ref(grid, rows, divisor)
  u = np.unique(r[r >= 0])
  slot = {int(x): k for k, x in enumerate(u)}
  out = np.zeros((u.size, g.shape[1]), np.float32)
  for p in np.nonzero(r >= 0)[0]:
    k = slot[int(r[p])]
    out[k] = out[k] + g[p]
  return u, out
