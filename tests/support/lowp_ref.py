"""The rounding of low-precision tables restated in numpy (include/hbk.h, "Low-precision tables"): fp32 -> bf16 to
nearest even and stochastically, and the noise function.  Everything works on uint32 bit patterns; nothing here
imports the library."""
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
