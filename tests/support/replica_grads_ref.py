"""The aggregated step of replicated tables restated in numpy fp32 (include/hbk.h: hbk_replica_grads_pack_n,
hbk_replica_grads_rows_n, hbk_sparse_apply_slices_n):

    pack    bucket = +0.0 everywhere; for u < clamp(n_unique, 0, capacity) with r = unique_rows[u] in [0, rows):
            block[r, :] = grad_rows[u, :] (a bit copy), touched[r] = 1.0
    reduce  the ranks' buckets summed in RANK ORDER in fp32 (acc = b_0; acc = acc + b_r), then ONE multiply by
            fp32(scale) -- what Collective.local_world computes by construction and what the layer asks of
            any transport
    rows    urows[r] = r where touched[r] != 0, else -1
    step    the optimizer's rule (tests/support/reference.py, rowwise_adagrad_ref.py: include/hbk.h's operation
            order, every op a separately rounded fp32 op) on the rows urows names, with g = block[r]

Pure numpy."""
import numpy as np

from tests.support import reference
from tests.support import rowwise_adagrad_ref

F32 = np.float32


def layout(shapes):
  """(block offsets, touched offsets, floats) of the bucket of tables shapes[c] = (rows, dim): every block starts
  on a 16-byte boundary, the touched words follow the last block."""
  blocks, at = [], 0
  for rows, dim in shapes:
    blocks.append(at)
    at += (rows * dim + 3) // 4 * 4
  touched = []
  for rows, _ in shapes:
    touched.append(at)
    at += rows
  return blocks, touched, at


def pack(shapes, slices, lay=None, fill=None):
  """One rank's bucket: slices[c] = (unique_rows [cap], grad_rows [cap, dim], n_unique).  `fill`: what the bucket
  held before the call (it must not matter)."""
  blocks, touched, total = lay if lay is not None else layout(shapes)
  bucket = np.zeros(total, F32)
  if fill is not None:
    bucket[:] = fill
    bucket[:] = 0.0          # the call clears all of it
  for c, ((rows, dim), (urows, grows, nu)) in enumerate(zip(shapes, slices)):
    urows = np.asarray(urows, np.int64)
    grows = np.asarray(grows, F32).reshape(urows.size, dim)
    n = min(max(int(nu), 0), urows.size)
    block = bucket[blocks[c]:blocks[c] + rows * dim].reshape(rows, dim)
    for u in range(n):
      r = int(urows[u])
      if 0 <= r < rows:
        block[r] = grows[u]
        bucket[touched[c] + r] = 1.0
  return bucket


def reduce(buckets, scale):
  """fp32 sum in rank order, then one multiply by fp32(scale)."""
  acc = np.array(buckets[0], F32, copy=True)
  for b in buckets[1:]:
    acc = (acc + np.asarray(b, F32)).astype(F32)
  if F32(scale) != F32(1):
    acc = (acc * F32(scale)).astype(F32)
  return acc


def rows_of(touched):
  t = np.asarray(touched, F32)
  return np.where(t != 0, np.arange(t.size, dtype=np.int64), np.int64(-1))


def unpack(shapes, bucket, lay=None):
  """Per table (urows int64 [rows], block fp32 [rows, dim]) of a reduced bucket: the slices with holes."""
  blocks, touched, _ = lay if lay is not None else layout(shapes)
  out = []
  for c, (rows, dim) in enumerate(shapes):
    out.append((rows_of(bucket[touched[c]:touched[c] + rows]),
                bucket[blocks[c]:blocks[c] + rows * dim].reshape(rows, dim).copy()))
  return out


ADAM = dict(b1=reference.ADAM_DEFAULTS[0], b2=reference.ADAM_DEFAULTS[1], eps=reference.ADAM_DEFAULTS[2])
FTRL = dict(l1=0.0, l2=0.0, l2_shrinkage=0.0, lr_power=-0.5)
ROWWISE = dict(eps=1e-8)


def apply_slices(optimizer, state, urows, grows, lr, n_unique=None, powers=None, hyper=None, vec4=None):
  """The optimizer step on slices with holes, in place.  state: dict(w=, and the optimizer's slots: a (adagrad,
  rowwise_adagrad [rows, 1]); m, v (adam); a, z (ftrl)).  Entries at or after n_unique and rows outside the table
  touch nothing.  Rows must be distinct.  Adam: `powers` (b1^t, b2^t) of this step; the caller advances them."""
  w = state['w']
  urows = np.asarray(urows, np.int64)
  n = urows.size if n_unique is None else min(max(int(n_unique), 0), urows.size)
  keep = np.flatnonzero((urows[:n] >= 0) & (urows[:n] < w.shape[0]))
  rows = urows[keep]
  assert np.unique(rows).size == rows.size, 'a row twice: the step is not additive'
  g = np.asarray(grows, F32).reshape(urows.size, w.shape[1])[keep]
  hyper = dict(hyper or {})
  if optimizer == 'sgd':
    reference.sgd_step(w, rows, g, lr)
  elif optimizer == 'adagrad':
    reference.adagrad_step(w, state['a'], rows, g, lr)
  elif optimizer == 'adam':
    h = dict(ADAM, **hyper)
    reference.adam_step(w, state['m'], state['v'], rows, g, lr, powers, h['b1'], h['b2'], h['eps'])
  elif optimizer == 'ftrl':
    h = dict(FTRL, **hyper)
    reference.ftrl_step(w, state['a'], state['z'], rows, g, lr, h['l1'], h['l2'], h['l2_shrinkage'], h['lr_power'])
  elif optimizer == 'rowwise_adagrad':
    h = dict(ROWWISE, **hyper)
    v4 = rowwise_adagrad_ref.is_vec4(w.shape[1]) if vec4 is None else vec4
    rowwise_adagrad_ref.step(w, state['a'], rows, g, lr, h['eps'], v4)
  else:
    raise ValueError(optimizer)


def aggregated_step(optimizer, states, shapes, per_rank_slices, scale, lr, powers=None, hyper=None):
  """One aggregated step of the tables `states` (one dict per table; every rank holds the same): pack per rank,
  reduce, rows, apply.  Returns the reduced slices [(urows, block), ...]."""
  lay = layout(shapes)
  bucket = reduce([pack(shapes, s, lay) for s in per_rank_slices], scale)
  agg = unpack(shapes, bucket, lay)
  for state, (urows, block) in zip(states, agg):
    apply_slices(optimizer, state, urows, block, lr, powers=powers, hyper=hyper)
  return agg
