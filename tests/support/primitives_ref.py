"""Plain restatements of the id and wire primitives (hbk_cast_n, hbk_floormod_n, hbk_unique_n,
hbk_cache_probe / hbk_cache_lookup, hbk_alltoallv_n) in numpy and Python integers, and the inputs that
drive them to the boundaries of their kernels, for tests/test_primitives_ref.py (the restatements against
the C oracle, on the CPU) and tests/test_gpu_primitive_edges.py (the kernels against the restatements).

Nothing here goes through ctypes: a restatement shares no code with what it checks.
"""
import numpy as np

from hybridbackend_amd.distribute.collective import alltoallv_offsets

EMPTY_KEY = -2 ** 63   # csrc/probe.hip: an EMPTY slot
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1


# ---------------------------------------------------------------------------------------------------
# wire casts
def cast_f32_to_f16(x):
  """IEEE round to nearest even (numpy's conversion; pinned by cast_rounding_examples)."""
  with np.errstate(over='ignore', invalid='ignore'):
    return np.asarray(x, np.float32).astype(np.float16)


def cast_f16_to_f32(h):
  with np.errstate(invalid='ignore'):
    return np.asarray(h, np.float16).astype(np.float32)


def assert_same_bits(got, want, what=''):
  """Bit for bit; where `want` is a NaN, `got` must be a NaN of the same sign (payload free)."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape,
                                                               want.shape)
  if got.dtype.kind != 'f':
    np.testing.assert_array_equal(got, want, err_msg=what)
    return
  bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
  nan = np.isnan(want)
  g, w = got.view(bits), want.view(bits)
  np.testing.assert_array_equal(g[~nan], w[~nan], err_msg=what)
  assert np.isnan(got[nan]).all(), what
  np.testing.assert_array_equal(np.signbit(got[nan]), np.signbit(want[nan]), err_msg=what)


def f16_all_bit_patterns():
  return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)


def f32_rounding_edges():
  """Every place fp32 -> fp16 has to decide: the midpoint between each finite non-negative fp16 value and
  its successor (65520 above 65504), the fp32 values next to it on either side, all with both signs
  (6 * 31744 = 190464 values), and the special values."""
  h = np.arange(0x7c00, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float64)
  succ = np.concatenate([h[1:], [65536.0]])
  mid = ((h + succ) / 2).astype(np.float32)
  assert (mid.astype(np.float64) * 2 == h + succ).all()           # the midpoints are exact in fp32
  below = np.nextafter(mid, np.float32(-np.inf))
  above = np.nextafter(mid, np.float32(np.inf))
  pos = np.concatenate([mid, below, above])
  bits = [0x00000000, 0x80000000,            # +-0
          0x7f800000, 0xff800000,            # +-inf
          0x7fc00000, 0x7f800001,            # quiet NaN, signalling NaN
          0xffc12345, 0x7f812345,            # NaNs with a payload (one negative)
          0x00000001, 0x007fffff,            # smallest and largest fp32 denormal
          0x80000001, 0x807fffff,
          0x7f7fffff, 0xff7fffff,            # +-FLT_MAX
          0x33000000, 0x32ffffff, 0x33000001]   # 2^-25 (half the smallest fp16 denormal) and its neighbours
  special = np.array(bits, np.uint32).view(np.float32)
  return np.concatenate([pos, -pos, special])


def cast_rounding_examples():
  """(fp32 value, fp16 bits) pairs that say what "nearest even" means at the places the set above probes;
  any conversion used as the expectation has to give these."""
  u = 2.0 ** -24   # the fp16 denormal unit
  return [(0.5 * u, 0x0000), (1.5 * u, 0x0002), (2.5 * u, 0x0002), (3.5 * u, 0x0004),
          (65520.0, 0x7c00), (float(np.nextafter(np.float32(65520.0), np.float32(0))), 0x7bff),
          (-65520.0, 0xfc00), (1.0 + 2.0 ** -11, 0x3c00), (1.0 + 3 * 2.0 ** -11, 0x3c02)]


CAST_LENGTHS = (0, 1, 7, 8, 9, 2047, 2048, 2049, 4101)
CAST_F32_OFFSETS = (0, 1, 2, 3)   # elements on the fp32 side
CAST_F16_OFFSETS = (0, 1, 4, 7)   # elements on the fp16 side


def cast_layout_product():
  """[(len, fp32 offset, fp16 offset)]: the full product, 144 tensors = two launches of a cast call."""
  return [(n, a, b) for n in CAST_LENGTHS for a in CAST_F32_OFFSETS for b in CAST_F16_OFFSETS]


def cast_layout_values(seed, n):
  """n finite fp32 values over the fp16 range (some beyond it)."""
  rng = np.random.RandomState(seed)
  return (rng.randn(n) * 10.0 ** rng.uniform(-9, 5.3, size=n)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# floormod
FLOORMOD_DIVISORS = [1, 2, 3, 5, 7, 8, 10, 1000, 1 << 20, 1000000, 1000003, 100000000,
                     (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) + 15, (1 << 40) - 87,
                     (1 << 62) + 1, (1 << 63) - 1]     # tests/test_abi.py test_host_floormod_matches_python
FLOORMOD_EDGES = [0, 1, -1, 2, -2, (1 << 63) - 1, -(1 << 63), (1 << 62), -(1 << 62), (1 << 32),
                  -(1 << 32), (1 << 32) - 1]
FLOORMOD_LENGTHS = (2047, 2048, 2049)


def floormod(x, d):
  """TF FloorMod for a positive divisor: Python's %."""
  x = np.asarray(x)
  return np.array([int(v) % int(d) for v in x.tolist()], dtype=x.dtype)


def floormod_columns(dtype, n_cols=130, empty=(0, 127, 128), seed=41):
  """[(values, divisor)] for one hbk_floormod_n call: every column its own divisor, the edge values, the
  values around its divisor, random fill to a length around the 2048-element tile."""
  info = np.iinfo(dtype)
  rng = np.random.RandomState(seed)
  divisors = [d for d in FLOORMOD_DIVISORS if d <= info.max and (dtype == np.int64 or d < (1 << 31))]
  cols = []
  for c in range(n_cols):
    d = divisors[c % len(divisors)]
    if c in empty:
      cols.append((np.zeros(0, dtype), d))
      continue
    n = FLOORMOD_LENGTHS[(c // len(divisors) + c) % len(FLOORMOD_LENGTHS)]
    head = [v for v in FLOORMOD_EDGES + [d - 1, d, d + 1, -d, -d - 1] if info.min <= v <= info.max]
    fill = rng.randint(info.min, info.max, size=n - len(head), dtype=dtype)
    cols.append((np.concatenate([np.array(head, dtype), fill]), d))
  return cols


# ---------------------------------------------------------------------------------------------------
# unique
def unique_first_occurrence(x):
  """(unique, index): the distinct values in order of first occurrence, and for every input its place in
  that list (TF Unique)."""
  x = np.asarray(x, np.int64)
  if x.size == 0:
    return np.zeros(0, np.int64), np.zeros(0, np.int32)
  vals, first, inv = np.unique(x, return_index=True, return_inverse=True)
  order = np.argsort(first, kind='stable')           # sorted-unique number -> first-occurrence order
  place = np.empty(order.size, np.int64)
  place[order] = np.arange(order.size)
  return vals[order], place[inv.reshape(-1)].astype(np.int32)


def mix64(keys):
  """The 64-bit mix csrc/unique.hip derives buckets (top bits) and LDS slots (low bits) from."""
  k = np.asarray(keys).astype(np.int64).view(np.uint64).copy()
  with np.errstate(over='ignore'):
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> np.uint64(33)
  return k


def _unmix64(h):
  """Inverse of mix64 (each of its steps is a bijection of the 64-bit words)."""
  k = np.asarray(h, np.uint64).copy()
  inv2 = np.uint64(pow(0xc4ceb9fe1a85ec53, -1, 1 << 64))
  inv1 = np.uint64(pow(0xff51afd7ed558ccd, -1, 1 << 64))
  with np.errstate(over='ignore'):
    k ^= k >> np.uint64(33)
    k *= inv2
    k ^= k >> np.uint64(33)
    k *= inv1
    k ^= k >> np.uint64(33)
  return k.view(np.int64)


def keys_of_one_bucket(n, seed, top13=0x0a5b):
  """n distinct keys whose mix64 has the same top 13 bits: one bucket at any bucket count."""
  rng = np.random.RandomState(seed)
  low = np.unique(rng.randint(0, 1 << 51, size=2 * n + 64, dtype=np.int64))
  low = rng.permutation(low)[:n].astype(np.uint64)
  keys = _unmix64((np.uint64(top13) << np.uint64(51)) | low)
  keys = keys[keys != -1]
  assert keys.size == n and np.unique(keys).size == n
  return keys


UNIQUE_LENGTHS = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 6143, 6144, 6145)


def unique_patterns(n, seed):
  """{name: ids} of length n: the layouts that put repeats, first occurrences and the key -1 on the edges
  of the 1024-id and 2048-id tiles."""
  rng = np.random.RandomState(seed)
  i = np.arange(n, dtype=np.int64)
  distinct = rng.permutation(n).astype(np.int64) * 7919 - 5
  back1024 = np.resize(distinct[:1024], n)   # the first tile over and over (all distinct up to 1024 ids)
  back2048 = np.resize(distinct[:2048], n)
  mixed = np.array([-1, 0, INT64_MIN, INT64_MAX], np.int64)[rng.randint(0, 4, size=n)]
  return {
    'all_equal': np.full(n, 123456789012, np.int64),
    'all_distinct': distinct,
    'repeat_1024_back': back1024,          # ids[i] = ids[i - 1024]
    'repeat_2048_back': back2048,          # ids[i] = ids[i - 2048]
    'new_at_tile_end': (i + 1) // 1024,    # a new value only at the last position of each 1024-tile
    'all_minus_one': np.full(n, -1, np.int64),
    'minus_one_mixed': mixed,
  }


def unique_boundary_columns(seed=51):
  """[(name, ids)]: every pattern at every boundary length, 77 columns = one launch group."""
  cols = []
  for k, n in enumerate(UNIQUE_LENGTHS):
    for name, ids in unique_patterns(n, seed + k).items():
      cols.append(('%s/%d' % (name, n), ids))
  return cols


def unique_many_columns(n_cols, seed, all_empty=False):
  """n_cols columns of 0 to 3000 ids; zero-length columns at 95, 96 and the last position."""
  rng = np.random.RandomState(seed)
  cols = []
  for c in range(n_cols):
    n = 0 if all_empty or c in (95, 96, n_cols - 1) else int(rng.randint(0, 3001))
    hi = (8, 700, 1 << 40)[c % 3]
    ids = rng.randint(-3, hi, size=n).astype(np.int64)
    cols.append(ids)
  return cols


UNIQUE_BUCKETS_LOG2 = (0, 1, 9, 10, 13)   # 9: the last count the one-launch grouping takes; 10: falls back


def unique_bucket_option_columns(log2p, seed=61):
  """Columns for a forced bucket count at lengths 5000 and 70000: one of many repeats and one of many
  distinct ids.  The second goes with every count at 5000 (in one bucket: ~2400 keys for 2048 slots, the
  overflowing ones repeated) but only with the larger counts at 70000, and the first has 1500 distinct
  ids where all 70000 share one bucket, 2100 elsewhere: 70000 ids probing a FULL 2048-slot table walk
  about a thousand slots each, and every overflowing id scans the whole bucket -- seconds of time, no
  further path."""
  rng = np.random.RandomState(seed + log2p)
  cols = []
  for n in (5000, 70000):
    distinct = 1500 if (n == 70000 and log2p == 0) else 2100
    cols.append(rng.randint(0, distinct, size=n).astype(np.int64))
    if n == 5000:      # ~2400 distinct ids, most of them more than once: in one bucket the overflowing keys
      cols.append(rng.randint(0, 3000, size=n).astype(np.int64) * 1000003 - 2 ** 40)   # have repeats to find
    elif log2p >= 9:
      cols.append(rng.randint(-2 ** 40, 2 ** 40, size=n).astype(np.int64))
  return cols


UNIQUE_SKEW_KEYS = (2047, 2048, 2049, 3000)


def unique_skew_column(n_keys, seed=71, total=8000):
  """About `total` ids under the default options: n_keys distinct keys of ONE bucket, each twice, in
  shuffled order among ids of other buckets (the top bit of their mix differs, so they share a bucket
  with the keys at no bucket count above one) -- 2047 keys leave the bucket's LDS table one free slot,
  2048 fill it exactly, 2049 overflow it by one key."""
  rng = np.random.RandomState(seed + n_keys)
  keys = keys_of_one_bucket(n_keys, seed + n_keys)
  other = rng.randint(0, 1 << 62, size=max(total - 2 * n_keys, 0), dtype=np.int64).astype(np.uint64)
  rest = _unmix64(other | (np.uint64(1) << np.uint64(63)))
  return rng.permutation(np.concatenate([keys, keys, rest]))


# ---------------------------------------------------------------------------------------------------
# cache probe
def murmur3_hash32(keys):
  """murmur3_hash32<int64, seed 0>: MurmurHash3_x86_32 over the 8 key bytes, as uint32."""
  u = np.asarray(keys).astype(np.int64).view(np.uint64)
  m32 = np.uint64(0xffffffff)

  def rotl(x, r):
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & m32

  h = np.zeros(u.shape, np.uint64)
  for k in (u & m32, u >> np.uint64(32)):
    k = (k * np.uint64(0xcc9e2d51)) & m32
    k = rotl(k, 15)
    k = (k * np.uint64(0x1b873593)) & m32
    h = h ^ k
    h = rotl(h, 13)
    h = (h * np.uint64(5) + np.uint64(0xe6546b64)) & m32
  h = h ^ np.uint64(8)
  h = h ^ (h >> np.uint64(16))
  h = (h * np.uint64(0x85ebca6b)) & m32
  h = h ^ (h >> np.uint64(13))
  h = (h * np.uint64(0xc2b2ae35)) & m32
  h = h ^ (h >> np.uint64(16))
  return h.astype(np.uint32)


def home_slab(keys, slab_count):
  return (murmur3_hash32(keys).astype(np.int64) % slab_count).astype(np.int64)


def cache_probe(cache, slab_size, keys):
  """hit_slot per key, the rule at the top of csrc/probe.hip: start at the hashed slab; the first slot of
  the slab that holds the key is a hit (before anything else is asked of the slab: a key behind an EMPTY
  slot is found, and a query equal to EMPTY_KEY "hits" the first EMPTY slot); otherwise an EMPTY slot
  anywhere in the slab is a miss; otherwise the next slab, wrapping, until every slab was probed."""
  cache = np.asarray(cache, np.int64)
  keys = np.asarray(keys, np.int64)
  slab_count = cache.size // slab_size
  slabs = cache.reshape(slab_count, slab_size)
  slab_has_empty = (slabs == EMPTY_KEY).any(axis=1)
  result = np.full(keys.size, -1, np.int64)
  active = np.arange(keys.size)
  slab = home_slab(keys, slab_count)
  for _ in range(slab_count):
    if active.size == 0:
      break
    s = slab[active]
    match = slabs[s] == keys[active, None]
    found = match.any(axis=1)
    result[active[found]] = s[found] * slab_size + match[found].argmax(axis=1)
    go_on = ~found & ~slab_has_empty[s]
    active = active[go_on]
    slab[active] = (slab[active] + 1) % slab_count
  return result


def cache_lists(want, keys):
  """The four lists of hbk_cache_lookup, key order kept, and counts = (hits, misses)."""
  want, keys = np.asarray(want, np.int64), np.asarray(keys, np.int64)
  hit = want >= 0
  return (np.where(hit)[0].astype(np.int32), want[hit], np.where(~hit)[0].astype(np.int32), keys[~hit],
          np.array([hit.sum(), (~hit).sum()], np.int32))


PROBE_SLAB_SIZES = (1, 2, 3, 7, 8, 33, 63, 64)
PROBE_SLAB_COUNTS = (1, 2, 257)
PROBE_UNIVERSE = 5000


def probe_keys_per_block(slab_size):
  """Keys one workgroup of cache_probe_kernel takes: (256 >> group_log2) * 8."""
  g = 0
  while (1 << g) < slab_size:
    g += 1
  return (256 >> g) * 8


def _fill(cache, slab_size, keys):
  """The way a slab hash fills: first free slot of the hashed slab, else of the next slab."""
  slab_count = cache.size // slab_size
  for k, home in zip(keys.tolist(), home_slab(keys, slab_count).tolist()):
    slab = home
    for _ in range(slab_count):
      s = cache[slab * slab_size:(slab + 1) * slab_size]
      if (s == k).any():
        break
      free = np.where(s == EMPTY_KEY)[0]
      if free.size:
        s[free[0]] = k
        break
      slab = (slab + 1) % slab_count


def _pool_by_home(rng, slab_count, n=1 << 16):
  """Random distinct keys and their home slabs."""
  keys = np.unique(rng.randint(1, 1 << 44, size=n).astype(np.int64))
  keys = rng.permutation(keys)
  return keys, home_slab(keys, slab_count)


def probe_tables(slab_size, slab_count, seed=81):
  """[(name, cache, must)]: the tables of one geometry; `must` = keys the queries have to contain (what
  the table was built to show).  Tables a geometry cannot hold are left out (no second slot, no second slab)."""
  rng = np.random.RandomState(seed + 1000 * slab_size + slab_count)
  cap = slab_size * slab_count
  pool, home = _pool_by_home(rng, slab_count)
  by_home = lambda s: pool[home == s]   # noqa: E731
  last = slab_count - 1
  tables = [('empty', np.full(cap, EMPTY_KEY, np.int64), np.zeros(0, np.int64))]

  half = np.full(cap, EMPTY_KEY, np.int64)
  _fill(half, slab_size, pool[:(cap + 1) // 2])
  tables.append(('half', half, np.zeros(0, np.int64)))

  # full: no EMPTY slot anywhere, so any slot is reachable from any home slab, after up to slab_count
  # probes; keys of the last slab's home sit in slab 0 (the wrap), keys of slab 1's home sit in slab 0
  # too (found by the very last probe)
  full = pool[:cap].copy()
  must = []
  if slab_count > 1:
    wrap = by_home(last)[-min(slab_size, 2):]
    full[:wrap.size] = wrap
    must += wrap.tolist()
    if slab_size >= 3 and slab_count > 2:   # (with two slabs the wrap is that last probe)
      far = by_home(1)[-1:]
      full[2:3] = far
      must += far.tolist()
  assert np.unique(full).size == cap
  tables.append(('full', full, np.array(must, np.int64)))

  if slab_size >= 2:
    # a key stored behind an EMPTY slot of its own slab; and a key stored in the slab AFTER its home
    # slab while the home slab has room (what a probe may not reach)
    t = half.copy()
    s = int(rng.randint(0, slab_count))
    k = by_home(s)[-3:]
    t[s * slab_size:(s + 1) * slab_size] = EMPTY_KEY
    t[s * slab_size + slab_size - 1] = k[0]
    must = [k[0]]
    if slab_count > 1:
      nxt = (s + 1) % slab_count
      t[nxt * slab_size] = k[1]
      must.append(k[1])
    tables.append(('behind_empty', t, np.array(must, np.int64)))

    # the same key twice in one slab (the lower slot answers); the slab is otherwise full
    t = full.copy()
    s = int(rng.randint(0, slab_count))
    k = by_home(s)[-4]
    t[s * slab_size] = k
    t[s * slab_size + slab_size - 1] = k
    tables.append(('twice_in_slab', t, np.array([k], np.int64)))

  if slab_count > 1:
    # the same key in two slabs: in its home slab and the next (home answers), and -- from three slabs
    # on -- in the two slabs after a full home slab (the nearer answers)
    t = full.copy()
    s = int(rng.randint(0, slab_count))
    k = by_home(s)[-6:-4]
    t[s * slab_size] = k[0]
    t[((s + 1) % slab_count) * slab_size + slab_size - 1] = k[0]
    must = [k[0]]
    if slab_count > 2 and (t[s * slab_size:(s + 1) * slab_size] != k[1]).all():
      t[((s + 1) % slab_count) * slab_size] = k[1]
      t[((s + 2) % slab_count) * slab_size] = k[1]
      must.append(k[1])
    tables.append(('twice_in_two_slabs', t, np.array(must, np.int64)))
  return tables


def probe_universe(cache, must, seed):
  """PROBE_UNIVERSE query keys for one table: stored keys, absent keys, repeats of both, the special
  values, what the table was built to show; shuffled.  Every query of the tests is a selection from it,
  so one restated probe serves them all."""
  rng = np.random.RandomState(seed)
  stored = cache[cache != EMPTY_KEY]
  present = stored[rng.randint(0, stored.size, size=2000)] if stored.size else np.zeros(0, np.int64)
  absent = -rng.randint(2, 1 << 44, size=1500).astype(np.int64)   # (stored keys are positive)
  special = np.array([EMPTY_KEY, EMPTY_KEY + 1, -1, 0], np.int64)
  base = np.concatenate([present, absent, special, special, must, must])
  again = base[rng.randint(0, base.size, size=PROBE_UNIVERSE - base.size)]
  return rng.permutation(np.concatenate([base, again]))


def probe_key_counts(slab_size):
  k = probe_keys_per_block(slab_size)
  return sorted(set([0, 1, 1023, 1024, 1025, PROBE_UNIVERSE, k - 1, k, k + 1]))


def probe_selections(want, slab_size):
  """{name: indices into the universe}: a prefix for every key count, and all hits / all misses /
  strictly alternating (1025 keys: more than a compaction tile), where the table allows."""
  sel = {'first_%d' % n: np.arange(n) for n in probe_key_counts(slab_size)}
  hits, misses = np.where(want >= 0)[0], np.where(want < 0)[0]
  if hits.size:
    sel['all_hits'] = np.resize(hits, 1025)
  if misses.size:
    sel['all_misses'] = np.resize(misses, 1025)
  if hits.size and misses.size:
    alt = np.empty(2050, np.int64)
    alt[0::2] = np.resize(hits, 1025)
    alt[1::2] = np.resize(misses, 1025)
    sel['alternating'] = alt
  return sel


# ---------------------------------------------------------------------------------------------------
# alltoallv
def alltoallv(values_by_rank, sizes_by_rank, common):
  """One column over W ranks.  values_by_rank[r]: flat array of sum(sizes_by_rank[r]) * common elements,
  the chunks for ranks 0 .. W-1 in order; sizes_by_rank[r][d]: rows rank r sends to rank d.  Returns
  (received flat arrays, received sizes) per rank: rank d gets the chunks in order of the sender."""
  world = len(values_by_rank)
  outs, out_sizes = [], []
  for d in range(world):
    parts = []
    for r in range(world):
      off, _ = alltoallv_offsets(sizes_by_rank[r], common)
      parts.append(np.asarray(values_by_rank[r])[off[d]:off[d] + int(sizes_by_rank[r][d]) * common])
    outs.append(np.concatenate(parts))
    out_sizes.append(np.array([sizes_by_rank[r][d] for r in range(world)], np.int32))
  return outs, out_sizes


ALLTOALLV_WORLDS = (2, 3, 5)
ALLTOALLV_COMMON = (1, 3, 4, 16)


def alltoallv_sizes(world, n_cols, seed):
  """sizes[c][r][d] in [0, 40]; forced: the last rank sends nothing, column 1 is empty everywhere, in
  column 2 only ranks 0 and 1 exchange, and only with each other (in a world of two that pair includes
  the last rank: there it is silent in the calls of one and two columns and in every other column)."""
  rng = np.random.RandomState(seed + 10 * world + n_cols)
  sizes = rng.randint(0, 41, size=(n_cols, world, world))
  sizes[:, world - 1, :] = 0
  if n_cols > 1:
    sizes[1] = 0
  if n_cols > 2:
    pair = np.zeros((world, world), np.int64)
    pair[0, 1], pair[1, 0] = sizes[2, 0, 1] + 1, sizes[2, 1, 0] + 1
    sizes[2] = pair
  return sizes


def alltoallv_values(kind, n, seed):
  """n elements to send: 'f32' / 'f16wire' floats across the fp16 range (ties, +-65504, beyond), 'i64', 'i32'."""
  rng = np.random.RandomState(seed)
  if kind == 'i64':
    return rng.randint(INT64_MIN, INT64_MAX, size=n, dtype=np.int64)
  if kind == 'i32':
    return rng.randint(-2 ** 31, 2 ** 31 - 1, size=n, dtype=np.int32)
  x = (rng.randn(n) * 10.0 ** rng.uniform(-9, 5.5, size=n)).astype(np.float32)
  edge = np.array([65504, 65519.996, 65520, -65520, 1e5, 2.0 ** -25, 1.5 * 2.0 ** -24, 1 + 2.0 ** -11,
                   1 + 3 * 2.0 ** -11, 0.0, -0.0], np.float32)
  k = min(n, edge.size)
  x[rng.permutation(n)[:k]] = edge[:k]
  return x
