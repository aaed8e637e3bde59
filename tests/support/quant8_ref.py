"""8-bit tables restated in numpy (include/hbk.h, "8-bit tables"): the quantiser and the decode in np.float32
operations, one at a time; the noise is lowp_ref's restatement of the 16-bit step's.  Nothing here imports the
library."""
import numpy as np

from tests.support import lowp_ref

F32 = np.float32
TINY = F32(2.0 ** -100)


def pitch_for(dim):
  return (dim + 3) // 4 * 4 + 4


def quantise(v, pitch=None, rounding='nearest', seed=0, step=0, col=0, rows=None):
  """uint8 [R, pitch]: the table of the fp32 rows `v` [R, dim]; `rows`: the row numbers the noise is keyed by
  (default 0 .. R-1)."""
  v = np.ascontiguousarray(v, F32)
  R, dim = v.shape
  dim4 = (dim + 3) // 4 * 4
  pitch = pitch_for(dim) if pitch is None else pitch
  amax = np.abs(v).max(axis=1) if dim else np.zeros(R, F32)
  zero = amax < TINY
  with np.errstate(all='ignore'):
    scale = np.where(zero, F32(0), amax / F32(127.0)).astype(F32)
    t = (v / np.where(zero, F32(1), scale)[:, None]).astype(F32)
    if rounding == 'stochastic':
      rows = np.arange(R, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
      u = (lowp_ref.noise(seed, step, col, rows, dim) & np.uint32(0xFFFF)).astype(F32)
      q = np.floor((t + (u * F32(2.0 ** -16)).astype(F32)).astype(F32))
    else:
      q = np.rint(t)
  q = np.clip(q, -127, 127).astype(np.int32)
  out = np.zeros((R, pitch), np.uint8)
  out[:, :dim] = np.where(zero[:, None], 128, q + 128).astype(np.uint8)
  out[:, dim4:dim4 + 4] = scale.view(np.uint8).reshape(R, 4)
  return out


def scales(table8, dim):
  dim4 = (dim + 3) // 4 * 4
  return np.ascontiguousarray(table8[:, dim4:dim4 + 4]).view(F32).reshape(-1)


def dequantise(table8, dim):
  """fp32 [R, dim]: (code - 128) * scale, one fp32 multiply."""
  q = table8[:, :dim].astype(np.int32) - 128
  return (q.astype(F32) * scales(table8, dim)[:, None]).astype(F32)


def special_rows(rng, rows, dim):
  """fp32 [rows, dim] N(0, 1) rows with the four rows every table of the tests holds: an all-zero row, a row whose
  amax is below 2^-100, a row with a single non-zero element, a row holding +amax and -amax."""
  v = rng.standard_normal((rows, dim)).astype(F32)
  v[0] = 0
  v[1] = F32(1e-33) * v[1]
  v[2] = 0
  v[2, dim // 2] = F32(-0.75)
  v[3] = np.clip(v[3], -3, 3)
  v[3, 0] = F32(4.0)
  v[3, dim - 1] = F32(-4.0) if dim > 1 else F32(4.0)
  return v
