"""Low-precision tables restated in numpy (include/hbk.h, "Low-precision tables"): fp32 -> bf16 to nearest even and
stochastically, the noise function, fp32 <-> fp16 through numpy's IEEE float16, the fp32 patterns that exercise every
rounding decision (boundary_patterns), the forward in separately rounded fp32 operations (forward_rows) and the
optimizer step round(rule(upcast(row), slots, g)) (apply_step, over the rule restatements of reference.py and
rowwise_adagrad_ref.py).  The roundings work on uint32 / uint16 bit patterns; nothing here imports the library.
tests/test_lowp_ref.py holds all of it to a second authority."""
import numpy as np

GOLDEN = np.uint32(0x9E3779B9)


def fmix32(h):
  """murmur3's finalizer on uint32 arrays (arithmetic modulo 2^32)."""
  h = np.asarray(h, np.uint32).copy()
  with np.errstate(over='ignore'):
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
  return h


def noise(seed, step, col, rows, dim):
  """uint32 [len(rows), dim]: noise_k of every element k of every row r of column `col` of a call."""
  rows = np.asarray(rows, np.int64)
  with np.errstate(over='ignore'):
    base = fmix32(np.uint32(seed) ^ fmix32(np.uint32(step & 0xFFFFFFFF) + GOLDEN * np.uint32(col + 1)))
    lo = (rows.view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (rows.view(np.uint64) >> np.uint64(32)).astype(np.uint32)
    rowh = fmix32(fmix32(base ^ lo) ^ hi)
    k = np.arange(dim, dtype=np.uint32)
    return fmix32(rowh[:, None] + GOLDEN * (k[None, :] + np.uint32(1)))


def is_nan(u):
  u = np.asarray(u, np.uint32)
  return (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def bf16_nearest(u):
  """uint16 bf16 patterns of the fp32 patterns `u`: round to nearest, ties to even; a NaN gives 0x7FC0."""
  u = np.asarray(u, np.uint32)
  r = ((u.astype(np.uint64) + 0x7FFF + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)).astype(np.uint16)
  return np.where(is_nan(u), np.uint16(0x7FC0), r)


def bf16_stochastic(u, n):
  """uint16 bf16 patterns of the fp32 patterns `u` with the noise words `n`: exponent all ones -> nearest, else
  (u + (n & 0xFFFF)) >> 16."""
  u = np.asarray(u, np.uint32)
  n = np.asarray(n, np.uint32)
  r = ((u.astype(np.uint64) + (n & np.uint32(0xFFFF))) >> np.uint64(16)).astype(np.uint16)
  special = (u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
  return np.where(special, bf16_nearest(u), r)


def bf16_up(h):
  """fp32 values of uint16 bf16 patterns (exact)."""
  return (np.asarray(h, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_rows(w32, rows, seed, step, col):
  """The bf16 patterns [len(rows), dim] of fp32 rows `w32` [len(rows), dim] stepped at table rows `rows`."""
  w32 = np.ascontiguousarray(w32, np.float32)
  return bf16_stochastic(w32.view(np.uint32), noise(seed, step, col, rows, w32.shape[1]))


# ---- both 16-bit types on bit patterns -------------------------------------------------------------------------
BF16, FP16 = 'bf16', 'fp16'
F32 = np.float32


def is_nan16(h, dtype):
  """NaN-ness of uint16 patterns of `dtype`: exponent all ones and a non-zero fraction."""
  h = np.asarray(h, np.uint16)
  return (h & np.uint16(0x7FFF)) > np.uint16(0x7F80 if dtype == BF16 else 0x7C00)


def fp16_up(h):
  """fp32 values of uint16 fp16 patterns (exact, subnormals included): numpy's float16 -> float32."""
  return np.ascontiguousarray(h, np.uint16).view(np.float16).astype(F32)


def fp16_nearest(u):
  """uint16 fp16 patterns of the fp32 patterns `u`: numpy's float32 -> float16, IEEE round to nearest, ties to even
  (a NaN gives a NaN; its payload is not specified)."""
  with np.errstate(all='ignore'):
    return np.ascontiguousarray(u, np.uint32).view(F32).astype(np.float16).view(np.uint16)


def upcast(bits, dtype):
  """fp32 values of uint16 patterns of `dtype` ('bf16' | 'fp16')."""
  assert dtype in (BF16, FP16), dtype
  return bf16_up(bits) if dtype == BF16 else fp16_up(bits)


def round_nearest(u, dtype):
  """uint16 patterns of `dtype` of the fp32 patterns `u`, to nearest even."""
  assert dtype in (BF16, FP16), dtype
  return bf16_nearest(u) if dtype == BF16 else fp16_nearest(u)


def bits32(x):
  """uint32 patterns of fp32 values."""
  return np.ascontiguousarray(x, F32).view(np.uint32)


BF16_LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)
FP16_EXTRA = (0x7F800000, 0xFF800000,                            # +-inf
              0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001,    # a quiet and a signalling NaN of each sign
              0x7F7FFFFF, 0xFF7FFFFF,                            # +-FLT_MAX
              0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF)    # the smallest and the largest fp32 subnormal


def boundary_patterns(dtype):
  """uint32 [n]: the fp32 patterns that exercise every rounding decision of fp32 -> `dtype`, generated from the
  16-bit side.

  bf16: every upper half with the low halves BF16_LOW_HALVES (exact, just above, just below the tie, the tie, just
  above it, just below the next value): 6 * 2^16 patterns, infinities, NaNs, both zeros and subnormals among them.
  fp16: for every finite pattern h of either sign, with a = up(h), b = up(the next pattern away from zero) -- 65536
  above the largest finite value -- and m their exact midpoint: a, the fp32 value after a, the one before m, m, the
  one after m, the one before b (positive fp32 patterns are ordered as their values, so "after" is + 1 on the
  pattern); then FP16_EXTRA."""
  if dtype == BF16:
    h = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
    return (h[:, None] | np.array(BF16_LOW_HALVES, np.uint32)[None, :]).reshape(-1)
  assert dtype == FP16, dtype
  h = np.arange(0x7C00, dtype=np.uint16)                       # the finite magnitudes
  a = fp16_up(h).astype(np.float64)
  b = np.append(a[1:], 65536.0)
  m = (a + b) / 2
  au, mu, bu = (bits32(x.astype(F32)).astype(np.uint32) for x in (a, m, b))
  assert (au.view(F32) == a).all() and (mu.view(F32) == m).all() and (bu.view(F32) == b).all()   # all exact in fp32
  one = np.uint32(1)
  mag = np.stack([au, au + one, mu - one, mu, mu + one, bu - one], axis=1).reshape(-1)
  return np.concatenate([mag, mag | np.uint32(0x80000000), np.array(FP16_EXTRA, np.uint32)])


# ---- the forward --------------------------------------------------------------------------------------------------
def _rows_of(ids, rows, bucket, divisor):
  r = np.asarray(ids).astype(np.int64)
  if bucket:
    r = np.mod(r, bucket)                                       # (floor-mod: never negative)
  valid = r >= 0
  r = r // divisor
  valid &= r < rows
  return np.where(valid, r, 0), valid


def forward_rows(bits, dtype, ids, splits=None, weights=None, combiner='sum', bucket=0, divisor=1):
  """fp32 [segments, dim]: the forward of include/hbk.h ("Low-precision tables", FORWARD) on upcast(bits, dtype) in
  plain np.float32 operations, one at a time and in id order: acc = +0, every product and every sum separately
  rounded, the division by float32(n), sqrt(float32(n)), W or sqrt(Q); invalid rows and zero divisors give zeros."""
  table = upcast(bits, dtype)
  dim = table.shape[1]
  r, valid = _rows_of(ids, table.shape[0], bucket, divisor)
  n_ids = r.size
  w = None if weights is None else np.asarray(weights, F32)
  with np.errstate(all='ignore'):
    e = table[r] if n_ids else np.zeros((0, dim), F32)
    e = np.where(valid[:, None], e, F32(0))
    if splits is None:
      if w is None:
        return e
      div = {'sum': np.ones(n_ids, F32), 'mean': w, 'sqrtn': np.sqrt(w * w)}[combiner]
      out = e * w[:, None]
      if combiner != 'sum':
        out = out / div[:, None]
      return np.where((valid & (div != 0))[:, None], out, F32(0)).astype(F32)
    splits = np.asarray(splits, np.int64)
    lens = np.diff(splits)
    S = lens.size
    acc = np.zeros((S, dim), F32)
    wsum = np.zeros(S, F32)
    for k in range(int(lens.max()) if S else 0):
      s = np.nonzero(lens > k)[0]
      j = splits[s] + k
      if w is None:
        acc[s] = acc[s] + e[j]                                  # (an invalid row adds a row of +0)
      else:
        keep = valid[j]                                         # (an invalid row adds neither term nor weight)
        s, j = s[keep], j[keep]
        acc[s] = acc[s] + e[j] * w[j][:, None]
        wsum[s] = wsum[s] + (w[j] * w[j] if combiner == 'sqrtn' else w[j])
    if combiner == 'sum':
      return acc
    if w is None:
      fn = lens.astype(F32)
      div = fn if combiner == 'mean' else np.sqrt(fn)
      return np.where((lens > 0)[:, None], acc / np.where(lens > 0, div, F32(1))[:, None], acc).astype(F32)
    div = wsum if combiner == 'mean' else np.sqrt(wsum)
    return np.where((div != 0)[:, None], acc / div[:, None], F32(0)).astype(F32)


# ---- the apply ----------------------------------------------------------------------------------------------------
def apply_step(bits, dtype, slots, rows, g, optimizer, lr, hyper=None, rounding='nearest', seed=0, step=0, col=0,
               vec4=None, noise_rows=None):
  """One optimizer step of hbk_lowp_apply_slices_n restated: a stepped row is round(rule(upcast(row), slots, g)).

  bits uint16 [R, dim]; slots: the fp32 slot arrays of the rule (sgd: none; adagrad: accum; adam: m, v; ftrl: accum,
  linear; rowwise_adagrad: accum [R, 1]); rows int64 [n] (entries outside [0, R) touch nothing), g fp32 [n, dim].
  hyper: adam {'powers': (b1^t, b2^t)[, 'beta1', 'beta2', 'epsilon']}, ftrl {'l1', 'l2', 'l2_shrinkage', 'lr_power'},
  rowwise_adagrad {'epsilon'}.  vec4: the row-wise sum's lane layout (default: dim % 4 == 0).  noise_rows int64 [n]: the
  row numbers the stochastic noise is keyed by when `bits` is a compact copy of a few rows of a table too large for
  the host and `rows` number that copy (default: `rows`).  The rules are the
  project's restatements (tests/support/reference.py, rowwise_adagrad_ref.py).  Returns (new bits, new slots); the
  arguments are left alone."""
  from tests.support import reference, rowwise_adagrad_ref
  hyper = hyper or {}
  bits = np.array(bits, np.uint16)
  slots = [np.array(s, F32) for s in slots]
  rows = np.asarray(rows, np.int64)
  g = np.asarray(g, F32)
  keep = (rows >= 0) & (rows < bits.shape[0])
  noise_rows = rows if noise_rows is None else np.asarray(noise_rows, np.int64)
  rows, g, noise_rows = rows[keep], g[keep], noise_rows[keep]
  assert np.unique(rows).size == rows.size, 'a row twice: the step is not additive'
  dim = bits.shape[1]
  w = upcast(bits, dtype).copy()
  with np.errstate(all='ignore'):
    if optimizer == 'sgd':
      reference.sgd_step(w, rows, g, lr)
    elif optimizer == 'adagrad':
      reference.adagrad_step(w, slots[0], rows, g, lr)
    elif optimizer == 'adam':
      b = [hyper.get(k, d) for k, d in zip(('beta1', 'beta2', 'epsilon'), reference.ADAM_DEFAULTS)]
      reference.adam_step(w, slots[0], slots[1], rows, g, lr, hyper['powers'], *b)
    elif optimizer == 'ftrl':
      reference.ftrl_step(w, slots[0], slots[1], rows, g, lr, hyper['l1'], hyper['l2'], hyper['l2_shrinkage'],
                          hyper['lr_power'])
    elif optimizer == 'rowwise_adagrad':
      v4 = (dim % 4 == 0) if vec4 is None else bool(vec4)
      rowwise_adagrad_ref.step(w, slots[0], rows, g, lr, hyper['epsilon'], v4)
    else:
      raise ValueError(optimizer)
  u = bits32(w[rows])
  if rounding == 'stochastic':
    assert dtype == BF16
    bits[rows] = bf16_stochastic(u, noise(seed, step, col, noise_rows, dim))
  else:
    bits[rows] = round_nearest(u, dtype)
  return bits, slots
