"""Low-precision tables on the GPU against the host restatement alone (tests/support/lowp_ref.py, itself held to torch's
CPU casts, an integer restatement and the binomial by tests/test_lowp_ref.py) -- no comparison here goes through the
GPU's own casts or through the fp32 kernels:

1. every rounding decision through the apply's rounder.  LowpSparseApply with SGD pushes any fp32 pattern x through
   it: with a table of -0, lr = 1 and grad_rows = -x the stepped value is -0 - (1 * -x) = x exactly, for every x
   (a table of +0 would turn x = -0 into +0: +0 - +0; from -0 both zeros keep their sign).  The patterns are
   lowp_ref.boundary_patterns: every tie, the fp16 subnormal range, 65520 -> inf, the carry out of the largest finite
   bf16 value, fp32 subnormals, infinities, NaNs;
2. the identity: a zero gradient leaves each of the 65 536 patterns of a type alone;
3. the upcast of each of the 65 536 patterns through the forward, and non-finite rows in real sums;
4. the noise's column index with skipped columns and a second launch, the apply's and the forward's alignment classes,
   refusals that leave the state alone, and the row bound (a spare row behind every table and slot, which an
   off-by-one in the bound check would step).

Known and left out: noise_row's use of the upper 32 bits of the row number is not exercised on the device -- it would
need a table of more than 2^32 rows; tests/test_lowp_ref.py covers the formula."""
import numpy as np
import pytest
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import Ftrl, LazyAdam, LowpGroupLookup, LowpSparseApply, RowwiseAdagrad
from tests.support import lowp_ref as ref
from tests.support import reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
BF, HF = torch.bfloat16, torch.float16
NAME = {BF: 'bf16', HF: 'fp16'}
OPTIMIZERS = ('sgd', 'adagrad', 'adam', 'ftrl', 'rowwise_adagrad')
SEED = 0x9E3779B1
STEPS = (0, 1, 2 ** 32 - 1)
FTRL_HYPER = dict(l1=0.05, l2=1e-5, l2_shrinkage=0.01, lr_power=-0.5)
# what the spare rows behind tables and slots hold: ordinary values (fp32 0.5), so that a step of them shows in the bits
SPARE16, SPARE32 = 0x3C3C, 0x3F000000


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.detach().cpu().numpy().copy()


def bits16(t):
  """uint16 patterns of a 16-bit tensor, on the host."""
  return host(t.contiguous().view(torch.int16)).view(np.uint16)


def bits32_of(t):
  """uint32 patterns of an fp32 tensor, on the host."""
  return host(t.contiguous().view(torch.int32)).view(np.uint32)


def at_offset(shape, dtype, byte_off=0, spare_rows=0):
  """(a contiguous [rows, dim] view `byte_off` bytes into a fresh 16-byte aligned buffer, the `spare_rows` rows behind
  it in the same buffer).  Everything is zero."""
  item = torch.empty(0, dtype=dtype).element_size()
  assert byte_off % item == 0
  rows, dim = shape
  k, n, extra = byte_off // item, rows * dim, spare_rows * dim
  buf = torch.zeros(k + n + extra + 16, dtype=dtype, device=DEV)
  assert buf.data_ptr() % 16 == 0
  view = buf[k:k + n].view(rows, dim)
  assert view.data_ptr() % 16 == byte_off % 16 and view.is_contiguous()
  return view, buf[k + n:k + n + extra].view(spare_rows, dim)


def fill16(t, bits):
  t.view(torch.int16).copy_(dev(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(t.shape))


def fill32(t, bits):
  t.view(torch.int32).copy_(dev(np.ascontiguousarray(bits, np.uint32).view(np.int32)).view(t.shape))


def set_step(app, step):
  app.step_counter.fill_(step - 2 ** 32 if step >= 2 ** 31 else step)


def step_of(app):
  return int(app.step_counter.item()) & 0xFFFFFFFF


def same_where_not_nan(got, want, nan, what):
  """uint patterns: equal where `nan` is False."""
  bad = (got != want) & ~nan
  if bad.any():
    i = tuple(np.argwhere(bad)[0])
    raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} patterns differ, first at {i}: got '
                         f'{int(got[i]):#x}, want {int(want[i]):#x}')


# ---- 1. every rounding decision ---------------------------------------------------------------------------------------
LAYOUTS = {'dim256': (256, 0), 'dim3': (3, 0), 'dim64_two_bytes_in': (64, 2)}   # 4 elements per lane, one, one


def push_through_rounder(x, dtype, layout, rounding='nearest', step=0):
  """The table's patterns after the SGD step that computes exactly the fp32 patterns `x` (padded with +0 to whole
  rows), and x as laid out: (uint16 [rows, dim], uint32 [rows, dim])."""
  dim, off = LAYOUTS[layout]
  rows = -(-x.size // dim)
  xs = np.zeros(rows * dim, np.uint32)
  xs[:x.size] = x
  xs = xs.reshape(rows, dim)
  table, _ = at_offset((rows, dim), dtype, off)
  fill16(table, np.full((rows, dim), 0x8000, np.uint16))
  grows = torch.empty(rows, dim, dtype=torch.float32, device=DEV)
  fill32(grows, xs ^ np.uint32(0x80000000))                    # -x, whatever x is
  slices = (torch.arange(rows, dtype=torch.int64, device=DEV), grows,
            torch.tensor([rows], dtype=torch.int32, device=DEV))
  app = LowpSparseApply([table], rounding=rounding, seed=SEED)
  set_step(app, step)
  app([slices], 1.0, 'sgd')
  torch.cuda.synchronize()
  if rounding == 'stochastic':
    assert step_of(app) == (step + 1) & 0xFFFFFFFF
  return bits16(table), xs


@pytest.fixture(scope='module')
def patterns():
  return {d: ref.boundary_patterns(NAME[d]) for d in (BF, HF)}


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('dtype', [BF, HF], ids=['bf16', 'fp16'])
def test_nearest_on_every_boundary_pattern(patterns, dtype, layout):
  """Ties to even, fp32-subnormal inputs, fp16-subnormal results, 65520 -> inf, the carry out of the largest finite
  value, both zeros, infinities: the bits of the restatement.  A NaN stays a NaN (bf16: 0x7FC0)."""
  got, xs = push_through_rounder(patterns[dtype], dtype, layout)
  nan = ref.is_nan(xs)
  same_where_not_nan(got, ref.round_nearest(xs, NAME[dtype]), nan, f'{NAME[dtype]} {layout}')
  assert ref.is_nan16(got[nan], NAME[dtype]).all(), 'a NaN became a number'
  assert not ref.is_nan16(got[~nan], NAME[dtype]).any(), 'a number became a NaN'
  if dtype is BF:
    assert (got[nan] == 0x7FC0).all()


@pytest.mark.parametrize('step', STEPS)
@pytest.mark.parametrize('layout', list(LAYOUTS))
def test_stochastic_on_every_boundary_pattern(patterns, layout, step):
  got, xs = push_through_rounder(patterns[BF], BF, layout, 'stochastic', step)
  rows, dim = xs.shape
  want = ref.round_rows(xs.view(F32), np.arange(rows), SEED, step, 0)
  np.testing.assert_array_equal(got, want, f'{layout} step {step:#x}')
  # independently of the noise function
  g, down, low = got.astype(np.int64), (xs >> 16).astype(np.int64), xs & 0xFFFF
  special = (xs & 0x7F800000) == 0x7F800000
  assert ((g == down) | (g == down + 1))[~special].all()
  assert (g == down)[~special & (low == 0)].all()
  np.testing.assert_array_equal(got[special], ref.bf16_nearest(xs[special]))    # inf stays inf, NaN a NaN
  live = ~special
  live.reshape(-1)[patterns[BF].size:] = False                                 # (not the padding)
  for L in ref.BF16_LOW_HALVES[1:]:
    at = live & (low == L)
    n, up = int(at.sum()), int((g == down + 1)[at].sum())
    assert n == 65536 - 256
    if L == 1:
      assert up <= 12, (L, up)                                                 # Poisson, mean 1
    elif L == 0xFFFF:
      assert up >= n - 12, (L, up)
    else:
      p = L / 65536.0
      sd = np.sqrt(p * (1 - p) / n)
      assert abs(up / n - p) <= 6 * sd, f'L = {L:#x}: {up / n:.5f}, expected {p:.5f} +- {6 * sd:.5f}'


# ---- 2. the identity -----------------------------------------------------------------------------------------------------
ALL16 = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16).reshape(256, 256)


@pytest.mark.parametrize('optimizer', ['sgd', 'adagrad', 'rowwise_adagrad'])
@pytest.mark.parametrize('dtype,rounding', [(BF, 'nearest'), (HF, 'nearest'), (BF, 'stochastic')],
                         ids=['bf16-nearest', 'fp16-nearest', 'bf16-stochastic'])
def test_a_zero_gradient_moves_no_pattern(dtype, rounding, optimizer):
  """All 65 536 patterns of the type, -0, subnormals and infinities among them: w - rate * 0 = w.  The slots equal the
  restatement (Adagrad: 0.1 + 0 * 0; row-wise: 0.1 + 0 / dim)."""
  table, _ = at_offset((256, 256), dtype)
  fill16(table, ALL16)
  acc0 = np.full((256, 1 if optimizer == 'rowwise_adagrad' else 256), 0.1, F32)
  acc = dev(acc0)
  kw = {'adagrad': dict(accums=[acc]), 'rowwise_adagrad': dict(row_accums=[acc], rowwise_adagrad=RowwiseAdagrad())
        }.get(optimizer, {})
  app = LowpSparseApply([table], rounding=rounding, seed=SEED, **kw)
  urows = np.random.RandomState(1).permutation(256)
  slices = (dev(urows.astype(np.int64)), torch.zeros(256, 256, dtype=torch.float32, device=DEV),
            torch.tensor([256], dtype=torch.int32, device=DEV))
  app([slices], 1.0, optimizer)
  torch.cuda.synchronize()
  got = bits16(table)
  nan = ref.is_nan16(ALL16, NAME[dtype])
  same_where_not_nan(got, ALL16, nan, f'{NAME[dtype]} {rounding} {optimizer}')
  assert ref.is_nan16(got[nan], NAME[dtype]).all()
  if optimizer != 'sgd':
    _, (want_acc,) = ref.apply_step(ALL16, NAME[dtype], [acc0], urows, np.zeros((256, 256), F32), optimizer, 1.0,
                                    {'epsilon': 1e-8}, rounding, SEED, 0, 0)
    np.testing.assert_array_equal(bits32_of(acc), ref.bits32(want_acc))


# ---- 3. the upcast through the forward, and non-finite rows in sums ------------------------------------------------------
def assert_rows_equal(got, want, payloads, what):
  """fp32 outputs: bit for bit where `want` is not NaN, NaN-ness where it is (payloads: bit for bit everywhere)."""
  g, w = ref.bits32(got), ref.bits32(want)
  assert g.shape == w.shape, (what, g.shape, w.shape)
  nan = np.zeros(w.shape, bool) if payloads else ref.is_nan(w)
  same_where_not_nan(g, w, nan, what)
  assert ref.is_nan(g[nan]).all(), f'{what}: a NaN became a number'


@pytest.mark.parametrize('dtype', [BF, HF], ids=['bf16', 'fp16'])
def test_forward_upcasts_every_pattern_exactly(dtype):
  name = NAME[dtype]
  table, _ = at_offset((256, 256), dtype)
  fill16(table, ALL16)
  ids = torch.arange(256, dtype=torch.int64, device=DEV)
  want = ref.upcast(ALL16, name)
  for chunk in (None, 4, 8):
    out = LowpGroupLookup([table], chunk_elems=chunk)([ids])[0]
    torch.cuda.synchronize()
    assert_rows_equal(host(out), want, dtype is BF, f'{name} chunk {chunk}')
  # one element per lane: a view two bytes into its buffer
  narrow, _ = at_offset((1024, 64), dtype, 2)
  fill16(narrow, ALL16.reshape(1024, 64))
  ids = torch.arange(1024, dtype=torch.int32, device=DEV)
  out = LowpGroupLookup([narrow])([ids])[0]
  torch.cuda.synchronize()
  assert_rows_equal(host(out), want.reshape(1024, 64), dtype is BF, f'{name} one element per lane')
  # ragged sum, segments of one id: +0 + e (so -0 comes out as +0 and a NaN's payload is not kept: the restatement)
  ids = torch.arange(256, dtype=torch.int64, device=DEV)
  splits = torch.arange(257, dtype=torch.int32, device=DEV)
  want = ref.forward_rows(ALL16, name, np.arange(256), np.arange(257), None, 'sum')
  assert not np.signbit(want[ALL16 == 0x8000]).any()
  for chunk in (None, 4):
    out = LowpGroupLookup([table], chunk_elems=chunk)([ids], [splits])[0]
    torch.cuda.synchronize()
    assert_rows_equal(host(out), want, False, f'{name} ragged chunk {chunk}')


SPECIAL16 = {BF: (0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7F7F, 0xFF7F, 0x0001, 0x8001, 0x007F, 0x0080, 0x8000, 0x0000),
             HF: (0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x03FF, 0x0400, 0x8000, 0x0000)}
# zero, negative, ordinary; 2^-110 (fp32-subnormal products of fp16 subnormals), 2^112 (fp16's largest values overflow)
SPECIAL_WEIGHTS = (0.0, -1.0, -0.5, 0.25, 1.0, 3.0, 2.0 ** -110, 2.0 ** 112)


@pytest.mark.parametrize('combiner', ['sum', 'mean', 'sqrtn'])
@pytest.mark.parametrize('dtype', [BF, HF], ids=['bf16', 'fp16'])
def test_forward_sums_with_non_finite_and_extreme_rows(dtype, combiner):
  rng = np.random.RandomState(3)
  name, rows = NAME[dtype], 40
  tables, bits = [], []
  for dim in (3, 8, 64):
    b = ref.round_nearest(ref.bits32(rng.uniform(-2, 2, size=(rows, dim)).astype(F32)), name)
    plant = rng.rand(rows, dim) < 0.3
    b[plant] = rng.choice(np.array(SPECIAL16[dtype], np.uint16), size=int(plant.sum()))
    t, _ = at_offset((rows, dim), dtype)
    fill16(t, b)
    tables.append(t)
    bits.append(b)
  lens = rng.randint(0, 7, size=30)
  lens[7] = 70
  sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  for splits, n in ((sp, int(sp[-1])), (None, 50)):
    ids = [rng.randint(-2, rows + 2, size=n).astype(np.int64) for _ in tables]
    for weighted in (True, False):
      w = [rng.choice(np.array(SPECIAL_WEIGHTS, F32), size=n) for _ in tables] if weighted else None
      low = LowpGroupLookup(tables, combiners=combiner)
      outs = low([dev(i) for i in ids], None if splits is None else [dev(splits) for _ in tables],
                 sp_weights=None if w is None else [dev(x) for x in w])
      torch.cuda.synchronize()
      seen_nan = seen_inf = False
      for c, b in enumerate(bits):
        want = ref.forward_rows(b, name, ids[c], splits, None if w is None else w[c], combiner)
        assert_rows_equal(host(outs[c]), want, False,
                          f'{name} {combiner} dim {b.shape[1]} ragged {splits is not None} weighted {weighted}')
        seen_nan |= bool(np.isnan(want).any())
        seen_inf |= bool(np.isinf(want).any())
      assert seen_nan and seen_inf            # (the case does what it is for)


# ---- 4. columns of the apply: a host mirror per column ------------------------------------------------------------------
class Column:
  """One table with its fp32 slots and IndexedSlices on the device, each at a chosen byte offset into its buffer and
  with ONE SPARE ROW behind it in the same buffer (a sentinel the step must not touch: the slices name row `rows`),
  and host copies that follow the restatement."""

  def __init__(self, rng, rows, dim, dtype, optimizer, table_off=0, slot_off=0, grad_off=0, how='some'):
    self.rows, self.dim, self.dtype, self.name, self.optimizer = rows, dim, dtype, NAME[dtype], optimizer
    self.bits = ref.round_nearest(ref.bits32(rng.uniform(-2, 2, size=(rows, dim)).astype(F32)), self.name)
    self.table, self.table_spare = at_offset((rows, dim), dtype, table_off, 1)
    fill16(self.table, self.bits)
    fill16(self.table_spare, np.full((1, dim), SPARE16, np.uint16))
    shapes = {'sgd': [], 'adagrad': [dim], 'adam': [dim, dim], 'ftrl': [dim, dim], 'rowwise_adagrad': [1]}[optimizer]
    ranges = {'adagrad': [(0.1, 0.9)], 'adam': [(-0.1, 0.1), (0.01, 0.1)], 'ftrl': [(0.1, 0.9), (-1, 1)],
              'rowwise_adagrad': [(0.1, 0.9)]}.get(optimizer, [])
    self.slots_h, self.slots, self.slot_spares = [], [], []
    for k, (width, (lo, hi)) in enumerate(zip(shapes, ranges)):
      h = rng.uniform(lo, hi, size=(rows, width)).astype(F32)
      t, spare = at_offset((rows, width), torch.float32, slot_off if k == 0 else 0, 1)
      t.copy_(dev(h))
      fill32(spare, np.full((1, width), SPARE32, np.uint32))
      self.slots_h.append(h)
      self.slots.append(t)
      self.slot_spares.append(spare)
    self.grad_off = grad_off
    self.new_slices(rng, how)

  def new_slices(self, rng, how='some'):
    """Distinct rows in random order with a -1 and a `rows` among them, a stale tail (NaN gradients, live row numbers)
    past n_unique.  how: 'some' | 'empty' (capacity 0) | 'zero' (n_unique = 0 on the device)."""
    rows, dim = self.rows, self.dim
    if how == 'empty':
      self.urows_h, self.g_h, self.n = np.zeros(0, np.int64), np.zeros((0, dim), F32), 0
      self.slices = (dev(self.urows_h), torch.zeros(0, dim, dtype=torch.float32, device=DEV),
                     torch.zeros(1, dtype=torch.int32, device=DEV))
      return
    k = int(rng.randint(1, rows + 1))
    u = np.concatenate([rng.permutation(rows)[:k], [-1, rows]])
    u = u[rng.permutation(u.size)]
    n, cap = u.size, u.size + 3
    self.urows_h = np.concatenate([u, rng.randint(0, rows, size=cap - n)]).astype(np.int64)
    self.g_h = rng.randn(cap, dim).astype(F32)
    self.g_h[n:] = np.nan
    self.n = 0 if how == 'zero' else n
    g, _ = at_offset((cap, dim), torch.float32, self.grad_off)
    g.copy_(dev(self.g_h))
    self.slices = (dev(self.urows_h), g, torch.tensor([self.n], dtype=torch.int32, device=DEV))

  def check(self, c, lr, hyper, rounding, step, vec4, what):
    """Table and slots equal the restatement's step from the host copies, which then move on; the spare rows keep
    their sentinel."""
    want, slots = ref.apply_step(self.bits, self.name, self.slots_h, self.urows_h[:self.n], self.g_h[:self.n],
                                 self.optimizer, lr, hyper, rounding, SEED, step, c, vec4)
    what = f'{what}: column {c} ({self.name}, dim {self.dim}, {self.optimizer}, {rounding})'
    got = bits16(self.table)
    bad = got != want
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {bad.size} patterns differ, first at '
                           f'{tuple(np.argwhere(bad)[0])}')
    for k, (t, w) in enumerate(zip(self.slots, slots)):
      np.testing.assert_array_equal(bits32_of(t), ref.bits32(w), f'{what}: slot {k}')
    self.check_spares(what)
    self.bits, self.slots_h = want, slots

  def check_spares(self, what):
    assert (bits16(self.table_spare) == SPARE16).all(), f'{what}: the row behind the table was written'
    for k, s in enumerate(self.slot_spares):
      assert (bits32_of(s) == SPARE32).all(), f'{what}: the row behind slot {k} was written'

  def unchanged(self, what):
    np.testing.assert_array_equal(bits16(self.table), self.bits, what)
    for k, (t, w) in enumerate(zip(self.slots, self.slots_h)):
      np.testing.assert_array_equal(bits32_of(t), ref.bits32(w), f'{what}: slot {k}')
    self.check_spares(what)


def make_apply(cols, optimizer, rounding):
  kw = {}
  if optimizer == 'adagrad':
    kw = dict(accums=[c.slots[0] for c in cols])
  elif optimizer == 'adam':
    kw = dict(moments=[tuple(c.slots) for c in cols], adam=LazyAdam(device=DEV))
  elif optimizer == 'ftrl':
    kw = dict(ftrl_slots=[tuple(c.slots) for c in cols], ftrl=Ftrl(**FTRL_HYPER))
  elif optimizer == 'rowwise_adagrad':
    kw = dict(row_accums=[c.slots[0] for c in cols], rowwise_adagrad=RowwiseAdagrad())
  return LowpSparseApply([c.table for c in cols], rounding=rounding, seed=SEED, **kw)


def hyper_of(app, optimizer):
  """The rule's hyperparameters as the restatement takes them; Adam's powers are read from the device NOW."""
  if optimizer == 'adam':
    a = app.adam
    return dict(powers=tuple(host(a.beta_powers)), beta1=a.beta1, beta2=a.beta2, epsilon=a.epsilon)
  if optimizer == 'ftrl':
    return dict(FTRL_HYPER)
  if optimizer == 'rowwise_adagrad':
    return dict(epsilon=app.rowwise_adagrad.epsilon)
  return {}


MANY_DIMS = (1, 3, 4, 16, 20, 64)


@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
def test_seventy_columns_key_the_noise_by_the_index_in_the_call(optimizer):
  """70 bf16 columns in one stochastic call: two launches.  Column 5 has capacity 0, column 9's descriptor says 0 rows
  (both are left out of their launch), column 20 has n_unique = 0 on the device: every later column's index in its
  LAUNCH differs from its index in the CALL, which is what keys the noise.  Adam's powers and the step counter
  advance once per call, not once per launch."""
  rng = np.random.RandomState(70)
  cols = [Column(rng, 11, MANY_DIMS[c % len(MANY_DIMS)], BF, optimizer,
                 how={5: 'empty', 20: 'zero'}.get(c, 'some')) for c in range(70)]
  app = make_apply(cols, optimizer, 'stochastic')
  app._cols[9].rows = 0          # a table of no rows with live slices: nothing of it may be read or written
  cols[9].n = 0
  set_step(app, 41)
  powers = (F32(0.9), F32(0.999))
  for step in (41, 42):
    hyper = hyper_of(app, optimizer)
    if optimizer == 'adam':
      np.testing.assert_array_equal(np.array(hyper['powers'], F32), np.array(powers, F32), f'step {step}: powers')
      powers = reference.adam_finish(powers)
    app([c.slices for c in cols], 0.05, optimizer)
    torch.cuda.synchronize()
    assert step_of(app) == step + 1
    for c, col in enumerate(cols):
      col.check(c, 0.05, hyper, 'stochastic', step, None, f'step {step}')
  assert sum(col.n > 0 for col in cols[64:]) == 6 and all(col.n == 0 for col in (cols[5], cols[9], cols[20]))
  if optimizer == 'adam':
    np.testing.assert_array_equal(host(app.adam.beta_powers), np.array(powers, F32))


def alignment_columns(rng, optimizer, dtypes):
  """(column, vec4) of every alignment class the rule has."""
  dt = lambda: dtypes[len(out) % len(dtypes)]   # noqa: E731
  out = []
  for dim in (4, 16, 64):                      # (a) the table two bytes in: one element per lane
    out.append((Column(rng, 9, dim, dt(), optimizer, table_off=2), False))
  for dim in (16, 128, 256):                   # (b) the table 8 bytes in: still four elements per lane
    out.append((Column(rng, 9, dim, dt(), optimizer, table_off=8), True))
  for dim in (4, 64):                          # (c) grad_rows, or a slot, 4 bytes in: one element per lane
    out.append((Column(rng, 9, dim, dt(), optimizer, grad_off=4), False))
    if optimizer in ('adagrad', 'adam', 'ftrl'):
      out.append((Column(rng, 9, dim, dt(), optimizer, slot_off=4), False))
  if optimizer == 'rowwise_adagrad':           # (e) the row-wise word does not enter the row shape
    out.append((Column(rng, 9, 128, dt(), optimizer, slot_off=4), True))
    out.append((Column(rng, 9, 256, dt(), optimizer, slot_off=4, table_off=8), True))
  return out


@pytest.mark.parametrize('rounding', ['nearest', 'stochastic'])
@pytest.mark.parametrize('optimizer', OPTIMIZERS)
def test_apply_alignment_classes(optimizer, rounding):
  rng = np.random.RandomState(len(optimizer) + len(rounding))
  cols = alignment_columns(rng, optimizer, (BF,) if rounding == 'stochastic' else (BF, HF))
  assert cols[3][0].table.data_ptr() % 16 == 8 and cols[0][0].table.data_ptr() % 4 == 2
  app = make_apply([c for c, _ in cols], optimizer, rounding)
  set_step(app, 7)
  for step in (7, 8):
    hyper = hyper_of(app, optimizer)
    app([c.slices for c, _ in cols], 0.05, optimizer)
    torch.cuda.synchronize()
    for k, (col, vec4) in enumerate(cols):
      col.check(k, 0.05, hyper, rounding, step, vec4, f'step {step}')
    for col, _ in cols:
      col.new_slices(rng)


@pytest.mark.parametrize('misaligned', ['table', 'slot', 'grad_rows'])
@pytest.mark.parametrize('optimizer', ['adagrad', 'adam'])
def test_misaligned_dim_68_is_refused_by_name_and_nothing_moves(optimizer, misaligned):
  """One element per lane holds at most 64: the column is named, and tables, slots, beta powers and the step counter
  keep their bits."""
  rng = np.random.RandomState(68)
  off = {'table': dict(table_off=2), 'slot': dict(slot_off=4), 'grad_rows': dict(grad_off=4)}[misaligned]
  cols = [Column(rng, 9, 68, BF, optimizer), Column(rng, 9, 68, BF, optimizer, **off)]
  app = make_apply(cols, optimizer, 'stochastic')
  set_step(app, 5)
  powers = host(app.adam.beta_powers) if optimizer == 'adam' else None
  with pytest.raises(_lib.InvalidArgumentError, match='column 1'):
    app([c.slices for c in cols], 0.05, optimizer)
  torch.cuda.synchronize()
  for c, col in enumerate(cols):
    col.unchanged(f'column {c}')
  assert step_of(app) == 5
  if optimizer == 'adam':
    np.testing.assert_array_equal(host(app.adam.beta_powers), powers)
  # the same columns, aligned, are taken (dim 68 = 17 chunks of 4)
  cols = [Column(rng, 9, 68, BF, optimizer) for _ in range(2)]
  app = make_apply(cols, optimizer, 'stochastic')
  hyper = hyper_of(app, optimizer)
  app([c.slices for c in cols], 0.05, optimizer)
  torch.cuda.synchronize()
  for c, col in enumerate(cols):
    col.check(c, 0.05, hyper, 'stochastic', 0, True, 'aligned')


@pytest.mark.parametrize('chunk', [None, 8])
@pytest.mark.parametrize('dtype', [BF, HF], ids=['bf16', 'fp16'])
def test_forward_of_a_table_eight_bytes_into_its_buffer(dtype, chunk):
  """8-byte but not 16-byte aligned: the forward falls from eight to four elements per lane (a 16-byte load would
  straddle).  The result does not depend on the lane layout; this holds the layout to the restatement."""
  rng = np.random.RandomState(8)
  name, rows = NAME[dtype], 37
  tables, bits = [], []
  for dim in (64, 128, 256):
    b = ref.round_nearest(ref.bits32(rng.uniform(-2, 2, size=(rows, dim)).astype(F32)), name)
    t, _ = at_offset((rows, dim), dtype, 8)
    assert t.data_ptr() % 16 == 8
    fill16(t, b)
    tables.append(t)
    bits.append(b)
  lens = rng.randint(0, 9, size=70)
  lens[3] = 40
  sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  for splits, n in ((None, 130), (sp, int(sp[-1]))):
    ids = [rng.randint(-3, rows + 3, size=n).astype(np.int64) for _ in tables]
    w = [rng.uniform(-1, 2, size=n).astype(F32) for _ in tables]
    for weights in (None, w):
      low = LowpGroupLookup(tables, combiners='mean', chunk_elems=chunk)
      outs = low([dev(i) for i in ids], None if splits is None else [dev(splits) for _ in tables],
                 sp_weights=None if weights is None else [dev(x) for x in weights])
      torch.cuda.synchronize()
      for c, b in enumerate(bits):
        want = ref.forward_rows(b, name, ids[c], splits, None if weights is None else weights[c], 'mean')
        assert_rows_equal(host(outs[c]), want, False, f'{name} dim {b.shape[1]} chunk {chunk} ragged {splits is not None}')
