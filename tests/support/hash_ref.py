"""Plain restatement of the hash table's placement rule and row initialisation (include/hbk.h,
hbk_hash_insert_n) for tests/test_hash_abi.py and tests/test_gpu_hash.py.

* `fill`: the SEQUENTIAL form of the placement: keys taken one at a time, each into the first EMPTY slot of
  its hashed slab, else of the next slab (wrapping).  The device inserts concurrently, so slot numbers may
  differ from this order; what must agree is stated where the tests compare (the key set of every slab when
  no slab overflows; the whole array when every key has a slab of its own).
* `init_row`: the initial row of a key, a function of (key, seed, j) alone.
"""
import numpy as np

EMPTY = -2 ** 63
_M32 = 0xffffffff
_M64 = 0xffffffffffffffff
GOLDEN_RATIO = 0x9E3779B97F4A7C15


def _rotl(x, r):
  return ((x << r) | (x >> (32 - r))) & _M32


def murmur3(key):
  """murmur3_hash32<int64, seed 0> of one Python int (hybridbackend/common/murmur3.cu.h:32-77)."""
  u = int(key) & _M64
  h = 0
  for k in (u & _M32, u >> 32):
    k = (k * 0xcc9e2d51) & _M32
    k = _rotl(k, 15)
    k = (k * 0x1b873593) & _M32
    h ^= k
    h = _rotl(h, 13)
    h = (h * 5 + 0xe6546b64) & _M32
  h ^= 8
  h ^= h >> 16
  h = (h * 0x85ebca6b) & _M32
  h ^= h >> 13
  h = (h * 0xc2b2ae35) & _M32
  h ^= h >> 16
  return h


def home_slab(key, slab_count):
  return murmur3(key) % slab_count


def fill(cache, slab_size, keys):
  """Insert `keys` one at a time into `cache` (int64 [slab_count * slab_size], modified in place); returns
  the slot of every key, -1 where no slab had room (or key == EMPTY)."""
  slab_count = cache.size // slab_size
  slots = np.full(len(keys), -1, np.int64)
  for n, k in enumerate(np.asarray(keys, np.int64).tolist()):
    if k == EMPTY:
      continue
    slab = home_slab(k, slab_count)
    for _ in range(slab_count):
      s = cache[slab * slab_size:(slab + 1) * slab_size]
      hit = np.where(s == k)[0]
      if hit.size:
        slots[n] = slab * slab_size + hit[0]
        break
      free = np.where(s == EMPTY)[0]
      if free.size:
        s[free[0]] = k
        slots[n] = slab * slab_size + free[0]
        break
      slab = (slab + 1) % slab_count
  return slots


def init_mix(key, j, seed):
  """The int64 whose hash starts float j of the row of `key`."""
  x = (int(key) & _M64) ^ (((int(seed) + j + 1) & _M64) * GOLDEN_RATIO & _M64)
  return x - (1 << 64) if x >> 63 else x


def init_value(key, j, seed, scale):
  r = murmur3(init_mix(key, j, seed))
  unit = np.float32(r >> 8) * np.float32(2.0 ** -23) - np.float32(1.0)   # exact: 24 bits, a power of two, [-1, 1)
  return np.float32(unit) * np.float32(scale)


def init_row(key, dim, seed=0, scale=1e-3):
  """fp32 [dim]: the row a key starts from; scale 0: zeros (+0.0)."""
  if np.float32(scale) == 0:
    return np.zeros(dim, np.float32)
  return np.array([init_value(key, j, seed, scale) for j in range(dim)], np.float32)


def murmur3_np(keys):
  """`murmur3` of an int64 array at once (uint32 lanes kept in uint64, masked after every product)."""
  u = np.asarray(keys, np.int64).astype(np.uint64)
  m = np.uint64(_M32)
  h = np.zeros(u.shape, np.uint64)
  rot = lambda x, r: ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & m   # noqa: E731
  for k in (u & m, u >> np.uint64(32)):
    k = (k * np.uint64(0xcc9e2d51)) & m
    k = rot(k, 15)
    k = (k * np.uint64(0x1b873593)) & m
    h = rot(h ^ k, 13)
    h = (h * np.uint64(5) + np.uint64(0xe6546b64)) & m
  h ^= np.uint64(8)
  h ^= h >> np.uint64(16)
  h = (h * np.uint64(0x85ebca6b)) & m
  h ^= h >> np.uint64(13)
  h = (h * np.uint64(0xc2b2ae35)) & m
  h ^= h >> np.uint64(16)
  return h.astype(np.uint32)


def init_rows(keys, dim, seed=0, scale=1e-3):
  """`init_row` of every key at once: fp32 [len(keys), dim] (checked against the scalar form)."""
  keys = np.asarray(keys, np.int64)
  if np.float32(scale) == 0:
    return np.zeros((keys.size, dim), np.float32)
  with np.errstate(over='ignore'):
    mix = (np.arange(dim, dtype=np.uint64) + np.uint64((int(seed) + 1) & _M64)) * np.uint64(GOLDEN_RATIO)
    x = keys.astype(np.uint64)[:, None] ^ mix[None, :]
  r = murmur3_np(x.astype(np.int64))
  unit = (r >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
  return (unit * np.float32(scale)).astype(np.float32)


def slab_sets(cache, slab_size):
  """Sorted keys of every slab (EMPTY slots dropped)."""
  return [sorted(int(k) for k in s if k != EMPTY) for s in np.asarray(cache).reshape(-1, slab_size)]
