"""Row arrays past 2^32 elements and 2^32 rows: geometry, probe rows, alias rows, and a device table that is
never on the host (tests/test_gpu_wide_offsets.py; held to its purpose on the CPU by
tests/test_wide_offsets_support.py).

Every kernel that forms ``base + row * pitch`` is right only if that product is carried in 64 bits.  The four
THRESHOLDS of a row array with element size `es` are the element offsets at which a 32-bit quantity wraps: byte
offset 2^31 and 2^32, element offset 2^31 and 2^32.  A GEOMETRY is the smallest shape at which one kind of
overflow can occur.  PROBE rows sit on both sides of every threshold; the ALIAS rows of a probe are the rows a
kernel that truncates some part of the address would land on.  A WideTable is zeros on the device with distinct
random rows planted at the probe and at the alias rows: a gather that truncates returns another row's values, a
step that truncates leaves its probe row unstepped and changes an alias row or a zero.

The geometry part is pure numpy / Python integers; torch is imported by WideTable alone."""
import collections

import numpy as np

M31, M32 = 1 << 31, 1 << 32

Geometry = collections.namedtuple('Geometry', 'name dim pitch rows')

GEOMETRIES = {
  # dim 256 is the largest a row shape allows: all four thresholds at the fewest rows
  'E': Geometry('E', 256, 256, (1 << 24) + 1024),
  # dim 100: every threshold falls inside a row
  'E100': Geometry('E100', 100, 100, -(-M32 // 100) + 1024),
  # a row pitch: row 4096 starts past element offset 2^32 with 4200 rows in all
  'P': Geometry('P', 20, (1 << 20) + 4, 4200),
  # dim 1: row NUMBERS 2^31 and 2^32
  'R': Geometry('R', 1, 1, M32 + 1024),
}


def extent(geom):
  """Elements from the first of row 0 to one past the last of the last row."""
  return (geom.rows - 1) * geom.pitch + geom.dim


def _sizes(es):
  return (es,) if isinstance(es, int) else tuple(es)


def thresholds(es):
  """The four thresholds of an array of `es`-byte elements as element offsets, ascending, without repeats.  `es`
  may be a tuple -- a 16-bit table stepped together with fp32 slot arrays of its shape, (2, 4) -- for the union."""
  return sorted({t for e in _sizes(es) for t in (M31 // e, M32 // e, M31, M32)})


# ---- the address and its 32-bit mutants --------------------------------------------------------------------------
def _u32(x):
  return x & 0xFFFFFFFF


def _i32(x):
  x &= 0xFFFFFFFF
  return x - M32 if x >= M31 else x


def true_offset(geom, es, row, k):   # pylint: disable=unused-argument
  """The element offset of element k of row `row`."""
  return row * geom.pitch + k


# name -> element offset of (row, k) as a kernel with that 32-bit quantity would form it.  A byte offset that is no
# multiple of es cannot occur: es divides 2^31 and 2^32.
MUTANTS = collections.OrderedDict([
  ('elem_u32', lambda g, es, r, k: _u32(r * g.pitch + k)),
  ('elem_i32', lambda g, es, r, k: _i32(r * g.pitch + k)),
  ('byte_u32', lambda g, es, r, k: _u32((r * g.pitch + k) * es) // es),
  ('byte_i32', lambda g, es, r, k: _i32((r * g.pitch + k) * es) // es),
  ('row_u32', lambda g, es, r, k: _u32(r) * g.pitch + k),
  ('row_i32', lambda g, es, r, k: _i32(r) * g.pitch + k),
  ('pitch_mul_32', lambda g, es, r, k: _i32(r * g.pitch) + k),   # row * (int32)pitch evaluated in 32 bits
])


def mutant_can_differ(name, geom, es):
  """Whether the mutant's address differs from the true one anywhere in the array -- from the array's size alone
  (never from the probes): the largest value of the quantity it truncates against the width it keeps."""
  last = extent(geom) - 1
  return {
    'elem_u32': last >= M32, 'elem_i32': last >= M31,
    'byte_u32': last * es >= M32, 'byte_i32': last * es >= M31,
    'row_u32': geom.rows - 1 >= M32, 'row_i32': geom.rows - 1 >= M31,
    'pitch_mul_32': (geom.rows - 1) * geom.pitch >= M31,
  }[name]


# ---- probe and alias rows ------------------------------------------------------------------------------------------
def alias_rows_of(geom, es, row):
  """The rows a truncating kernel lands on instead of `row`: those that hold the element offsets o mod 2^31,
  o mod 2^32, (o es mod 2^31) / es and (o es mod 2^32) / es for o the offset of the row's first and of its last
  element (a wrapped offset need not start a row: both rows it spans), and the rows `row` mod 2^31 and mod 2^32.
  Only what lies inside the array and is not `row` itself."""
  out = set()
  for k in (0, geom.dim - 1):
    o = row * geom.pitch + k
    for e in _sizes(es):
      for a in (o % M31, o % M32, (o * e % M31) // e, (o * e % M32) // e):
        out.add(a // geom.pitch)
  out.update((row % M31, row % M32))
  return sorted(r for r in out if r != row and 0 <= r < geom.rows)


def probe_rows(geom, es):
  """(probe rows, alias rows), both ascending lists of Python ints, disjoint.

  The candidates: for every threshold T inside the array the rows that hold element offsets T - 1 and T and the
  rows just before and after those two; row 0 and the last row.

  No alias row may be a probe row (a step that truncates must hit a row nobody expects to change).  The arithmetic
  makes that impossible for the plain candidates: with a power-of-two pitch the rows around 2^32 wrap onto the rows
  around 2^31 (mod 2^31), which wrap onto row 0, 1, ...; so candidates are taken from the highest threshold down
  and a candidate that is an alias of an accepted probe, or whose own alias is an accepted probe, is moved one row
  at a time AWAY from its threshold (row 0 upwards, the last row downwards) until neither holds.  It stays on its
  side of its threshold; the row it left is planted as an alias row and so is still looked at."""
  last = extent(geom) - 1
  cands = []   # (row, direction to move in)
  for t in reversed(thresholds(es)):
    if t > last:
      continue
    lo, hi = (t - 1) // geom.pitch, t // geom.pitch
    # (T inside a row: that one row holds T - 1 and T)
    cands += [(hi, 1), (lo, -1)] if hi != lo else [(hi, 1)]
    cands += [(hi + 1, 1), (lo - 1, -1)]
  cands += [(geom.rows - 1, -1), (0, 1)]
  probes, aliases = set(), set()
  for r, step in cands:
    r = min(max(r, 0), geom.rows - 1)
    for _ in range(64):
      mine = alias_rows_of(geom, es, r)
      if r not in probes and r not in aliases and not probes.intersection(mine):
        break
      r += step
      assert 0 <= r < geom.rows, f'{geom.name}: a probe left the array'
    else:
      raise AssertionError(f'{geom.name}: no free row within 64 of a candidate')
    probes.add(r)
    aliases.update(mine)
  assert not probes & aliases
  return sorted(probes), sorted(aliases)


def draw_ids(rng, probes, id_dtype=np.int64, rows=None, unbucketized=False):
  """Ids in which every probe row occurs one to three times, shuffled.  unbucketized (int64 only): some arrive as
  row + k * rows, so the fused floor-mod runs with divisor `rows`.  Returns (ids, the row of every id)."""
  reps = rng.randint(1, 4, size=len(probes))
  r = np.repeat(np.asarray(probes, np.int64), reps)
  rng.shuffle(r)
  ids = r.copy()
  if unbucketized:
    assert id_dtype == np.int64 and rows
    k = rng.randint(0, 1 << 20, size=r.size).astype(np.int64)
    k[::3] = 0
    ids = r + k * np.int64(rows)
  assert ids.max() <= np.iinfo(id_dtype).max
  return ids.astype(id_dtype), r


def compact(planted, rows):
  """The numbers 0..n-1 of `rows` in the compact copy whose row i is planted row planted[i]."""
  planted = np.asarray(planted, np.int64)
  at = np.searchsorted(planted, rows)
  assert (planted[at] == rows).all(), 'a row that was not planted'
  return at


# ---- the sparse-memory model (CPU) ---------------------------------------------------------------------------------
class SparseMemory:
  """A row array as a dict from element offset to value; everything else inside [0, extent) reads 0, an access
  outside is CAUGHT (on the device: a fault, or a neighbour's memory).  `addr(geom, es, row, k)` is the address
  computation under test."""

  def __init__(self, geom, es, probes, aliases):
    self.geom, self.es, self.probes, self.aliases = geom, es, list(probes), list(aliases)
    self.mem = {}
    for r in self.probes + self.aliases:
      for k in range(geom.dim):
        o = true_offset(geom, es, r, k)
        self.mem[o] = float(1 + o % 1000003)        # non-zero, and distinct across the planted rows
    self.planted = dict(self.mem)
    self.caught = False

  def _at(self, addr, row, k):
    o = addr(self.geom, self.es, row, k)
    if not 0 <= o < extent(self.geom):
      self.caught = True
      return None
    return o

  def gather(self, addr, row):
    out = []
    for k in range(self.geom.dim):
      o = self._at(addr, row, k)
      out.append(None if o is None else self.mem.get(o, 0.0))
    return out

  def step(self, addr, row, g=0.5):
    for k in range(self.geom.dim):
      o = self._at(addr, row, k)
      if o is not None:
        self.mem[o] = self.mem.get(o, 0.0) - g

  def want_row(self, row, stepped=0.0):
    return [self.planted[true_offset(self.geom, self.es, row, k)] - stepped for k in range(self.geom.dim)]

  def rest_untouched(self):
    """WideTable.assert_rest_untouched on the model: the alias rows as planted, and, the probe and alias rows set
    aside, nothing non-zero."""
    probe_offs = {true_offset(self.geom, self.es, r, k) for r in self.probes for k in range(self.geom.dim)}
    for o, v in self.mem.items():
      if o in probe_offs:
        continue
      if v != self.planted.get(o, 0.0):
        return False
    return True


def model_detects(geom, es, addr, probes=None, aliases=None):
  """Whether a gather and a row step over every probe row through `addr` are noticed: a probe row that reads or
  ends up different from the true address's result, an access outside the array, or a failing rest_untouched."""
  if probes is None:
    probes, aliases = probe_rows(geom, es)
  mem = SparseMemory(geom, es, probes, aliases)
  seen = False
  for r in probes:
    if mem.gather(addr, r) != mem.want_row(r):
      seen = True
  for r in probes:
    mem.step(addr, r)
  for r in probes:
    if [mem.mem[true_offset(geom, es, r, k)] for k in range(geom.dim)] != mem.want_row(r, 0.5):
      seen = True
  return seen or mem.caught or not mem.rest_untouched()


# ---- the device table ----------------------------------------------------------------------------------------------
SCAN_CHUNK = 1 << 28     # elements per chunk of the zero scan


class WideTable:
  """A [rows, pitch] array of zeros on the device (the table: its first `dim` columns) with rows planted.

  `planted` (ascending int64) are the probe and alias rows, `values` [len(planted), dim] what was planted there
  (numpy, of the array's host dtype: fp32, or uint16 bit patterns for the 16-bit types).  Nothing of full size is
  ever copied to, or allocated on, the host."""

  def __init__(self, geom, dtype, device='cuda:0', over=None):
    """over: an existing [rows, pitch] tensor (all zero, or holding only what `adopt` is then told of) to look
    after instead of a new one -- the arrays a hash table allocates itself."""
    import torch
    self.torch = torch
    self.geom, self.dtype = geom, dtype
    self.es = torch.empty(0, dtype=dtype).element_size()
    if over is not None:
      assert over.dtype == dtype and tuple(over.shape) == (geom.rows, geom.pitch) and over.is_contiguous()
    self.t = torch.zeros((geom.rows, geom.pitch), dtype=dtype, device=device) if over is None else over
    self.planted = np.zeros(0, np.int64)
    self.values = None
    self.probes = self.aliases = ()

  @property
  def table(self):
    """The [rows, dim] table (a view; contiguous unless the geometry has a pitch)."""
    return self.t if self.geom.pitch == self.geom.dim else self.t[:, :self.geom.dim]

  @property
  def nbytes(self):
    return self.t.numel() * self.es

  def _bits(self, x):
    """A tensor of this array's dtype seen as integers of its width (the zero scan and the 16-bit planting are on
    bits: -0.0 is not zero)."""
    return x.view(self.torch.int32 if self.es == 4 else self.torch.int16)

  def _to_device(self, values):
    v = np.ascontiguousarray(values)
    if self.es == 2:
      assert v.dtype == np.uint16
      return self.torch.from_numpy(v.view(np.int16)).to(self.t.device).view(self.dtype)
    assert v.dtype == np.float32
    return self.torch.from_numpy(v).to(self.t.device)

  def write_rows(self, idx, values):
    d = self._to_device(values)
    for i, r in enumerate(idx):
      self.t.narrow(0, int(r), 1)[:, :self.geom.dim].copy_(d[i:i + 1])

  def plant(self, probes, aliases, values):
    """Plant `values` (one row per planted row, probes and aliases merged ascending) into an all-zero array."""
    self.probes, self.aliases = list(probes), list(aliases)
    self.planted = np.array(sorted(set(self.probes) | set(self.aliases)), np.int64)
    assert self.planted.size == len(self.probes) + len(self.aliases)
    values = np.ascontiguousarray(values)
    assert values.shape == (self.planted.size, self.geom.dim)
    self.values = values.copy()
    self.write_rows(self.planted, values)
    return self

  def adopt(self, probes, values):
    """Rows a kernel wrote into an array nothing was planted in (the arrays a rehash allocates): `values` is what they
    must hold; assert_rest_untouched(()) then compares them and finds everything else zero."""
    assert not self.planted.size
    self.probes, self.aliases = sorted(int(r) for r in probes), []
    self.planted = np.array(self.probes, np.int64)
    order = np.argsort(np.asarray(probes, np.int64), kind='stable')
    self.values = np.ascontiguousarray(values)[order].copy()
    assert np.unique(self.planted).size == self.planted.size
    return self

  def refresh(self, rows):
    """The rows `rows` (probe rows an op was meant to change, and was checked to have changed rightly) as they are on
    the device now become what was planted there."""
    rows = [int(r) for r in rows]
    if rows:
      self.values[self.compact_of(rows)] = self.rows(rows)

  def rows(self, idx):
    """The rows `idx` on the host (fp32, or uint16 patterns)."""
    idx = [int(r) for r in idx]
    if not idx:
      return np.zeros((0, self.geom.dim), np.float32 if self.es == 4 else np.uint16)
    got = self.torch.cat([self.t.narrow(0, r, 1)[:, :self.geom.dim] for r in idx])
    if self.es == 2:
      return self._bits(got.contiguous()).cpu().numpy().view(np.uint16)
    return got.cpu().numpy()

  def compact_of(self, rows):
    return compact(self.planted, np.asarray(rows, np.int64))

  def assert_rest_untouched(self, changed_rows=(), what='', keep=False):
    """The alias rows (and every planted row not in `changed_rows`) hold what was planted; then the planted rows are
    zeroed on the device and the whole array -- padding of a pitch included -- must hold no non-zero bit, scanned
    in chunks of at most 2^28 elements.  Leaves the array all zero, ready for the next plant -- or, with `keep`,
    puts the planted rows back as they were found (the changed ones as they are now) for the next op on it."""
    torch = self.torch
    if keep:
      self.refresh(changed_rows)
      changed_rows = ()
      saved = torch.cat([self.t.narrow(0, int(r), 1)[:, :self.geom.dim] for r in self.planted.tolist()]) \
          if self.planted.size else None
    changed = set(int(r) for r in changed_rows)
    assert changed <= set(self.probes), f'{what}: only probe rows may change'
    same = np.array([r for r in self.planted.tolist() if r not in changed], np.int64)
    got = self.rows(same)
    want = self.values[self.compact_of(same)] if same.size else got
    bad = np.nonzero((got.view(np.uint32 if self.es == 4 else np.uint16) !=
                      want.view(np.uint32 if self.es == 4 else np.uint16)).any(axis=1))[0]
    assert not bad.size, f'{what}: rows {same[bad].tolist()[:8]} of geometry {self.geom.name} changed (planted, not stepped)'
    for r in self.planted.tolist():
      self.t.narrow(0, r, 1)[:, :self.geom.dim].zero_()
    flat = self._bits(self.t.view(-1))
    flags = []
    for off in range(0, flat.numel(), SCAN_CHUNK):
      flags.append(flat.narrow(0, off, min(SCAN_CHUNK, flat.numel() - off)).any())
    hit = torch.stack(flags).cpu().numpy()
    if hit.any():
      c = int(np.nonzero(hit)[0][0])
      chunk = flat.narrow(0, c * SCAN_CHUNK, min(SCAN_CHUNK, flat.numel() - c * SCAN_CHUNK))
      first = c * SCAN_CHUNK + int(torch.nonzero(chunk)[0].item())
      raise AssertionError(f'{what}: element {first} (row {first // self.geom.pitch}, lane {first % self.geom.pitch}) of '
                           f'geometry {self.geom.name} is non-zero: written by a row that is not there')
    if keep:
      for i, r in enumerate(self.planted.tolist()):
        self.t.narrow(0, r, 1)[:, :self.geom.dim].copy_(saved[i:i + 1])
      return
    self.planted, self.values, self.probes, self.aliases = np.zeros(0, np.int64), None, (), ()


LIMIT_BYTES = 72 << 30     # no test may hold more
MARGIN_BYTES = 4 << 30     # free HBM a test leaves to others


class SlabPool:
  """The device memory of the wide arrays, allocated once and handed from test to test.

  Freeing a 16 GiB allocation and making another of a different size costs the driver 0.5 - 2.5 s now and then (a
  fresh mapping), which is a hundred times what a test does with it; so the arrays are views of SLABS of one size
  (the largest array any test plants), made with torch.zeros when first needed, zeroed again when reused, and kept
  between tests as long as the next test's own needs leave room for them below 72 GiB.

  reserve(n, extra) is a test's statement of the HBM it needs -- n slabs and `extra` bytes that something else
  allocates (a hash table's own arrays, outputs): idle slabs the statement leaves no room for are released,
  torch.cuda.empty_cache() runs, and the test is skipped unless what must still be allocated fits into the free
  memory with 4 GiB to spare.  take(geom, dtype) gives a zeroed [rows, pitch] view of a reserved slab; release()
  (the test's tear-down) makes every slab idle again."""

  def __init__(self, slab_bytes, device='cuda:0'):
    self.slab_bytes, self.device = int(slab_bytes), device
    self.idle, self.busy, self.reserved = [], [], 0

  def need(self, n_slabs, extra=0):
    return n_slabs * self.slab_bytes + int(extra)

  def reserve(self, n_slabs, extra=0):
    import pytest
    import torch
    need = self.need(n_slabs, extra)
    assert need <= LIMIT_BYTES, 'no test may hold more than 72 GiB'
    assert not self.busy, 'reserve() comes first'
    room = max(n_slabs, (LIMIT_BYTES - int(extra) - (1 << 30)) // self.slab_bytes)
    del self.idle[room:]
    self.reserved = n_slabs
    if not torch.cuda.is_available():
      return need
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    still = max(0, n_slabs - len(self.idle)) * self.slab_bytes + int(extra)
    if free < still + MARGIN_BYTES:
      pytest.skip(f'needs {need / 2**30:.1f} GiB of HBM + 4 GiB: {still / 2**30:.1f} GiB are still to be allocated, '
                  f'{free / 2**30:.1f} GiB are free')
    return need

  def take(self, geom, dtype):
    """A WideTable over a zeroed [rows, pitch] view of one reserved slab."""
    import torch
    assert len(self.busy) < self.reserved, 'more arrays than the test reserved slabs for'
    es = torch.empty(0, dtype=dtype).element_size()
    nbytes = geom.rows * geom.pitch * es
    assert nbytes <= self.slab_bytes, f'{geom.name}: {nbytes} bytes do not fit a slab'
    if self.idle:
      slab = self.idle.pop()
      view = slab[:nbytes].view(dtype).view(geom.rows, geom.pitch)
      view.zero_()             # (whatever the test before left, a failed one included)
    else:
      slab = torch.zeros(self.slab_bytes, dtype=torch.uint8, device=self.device)
      view = slab[:nbytes].view(dtype).view(geom.rows, geom.pitch)
    self.busy.append(slab)
    return WideTable(geom, dtype, self.device, over=view)

  def release(self):
    self.idle += self.busy
    self.busy = []
    self.reserved = 0
