"""The host restatement of the low-precision tables (tests/support/lowp_ref.py) held to a second authority, so that
the GPU tests which compare the kernels with it (tests/test_gpu_lowp_rounding.py, tests/test_gpu_lowp_fuzz.py) do not
rest on one implementation: torch's CPU casts, an integer restatement of round-to-nearest-even written here, the
binomial for the noise, and the float64 reference of tests/support/reference.py for the sums.

Known and left out: noise_row's use of the upper 32 bits of the row number is covered here as a formula only (rows
2^32 and above are fed to the restatement); no device test can reach it without a table of more than 2^32 rows."""
import numpy as np
import pytest
import torch

from tests.support import lowp_ref as ref
from tests.support import reference
from tests.support.tolerance import FLOOR, REL, assert_sums_close

F32 = np.float32
TORCH = {'bf16': torch.bfloat16, 'fp16': torch.float16}
SEED = 0x9E3779B1
NOISE_STEPS = (0, 1, 2 ** 32 - 1)
NOISE_COLS = (0, 1, 69)


def torch_nearest(u, dtype):
  """torch's CPU float32 -> 16-bit cast of the fp32 patterns `u`, as uint16 patterns."""
  x = torch.from_numpy(np.ascontiguousarray(u, np.uint32).view(np.int32).copy()).view(torch.float32)
  return x.to(TORCH[dtype]).view(torch.int16).numpy().view(np.uint16)


def torch_up(h, dtype):
  """torch's CPU 16-bit -> float32 cast of uint16 patterns, as uint32 patterns."""
  x = torch.from_numpy(np.ascontiguousarray(h, np.uint16).view(np.int16).copy()).view(TORCH[dtype])
  return x.float().view(torch.int32).numpy().view(np.uint32)


def rne_fp16_integers(u):
  """fp32 patterns -> fp16 patterns of the non-NaN inputs in integer arithmetic.  |x| = M * 2^E (M the 24-bit
  significand); fp16's grid at that magnitude has the step 2^(E + shift).  Pick the lower neighbour, compare the
  remainder with half a step, break ties on the low bit; the biased exponent eh of the step (1 for subnormals) and
  the count q of steps give the pattern (eh - 1) * 1024 + q, carries into the exponent and into infinity included."""
  u = np.asarray(u, np.uint32).astype(np.int64)
  sign, e, frac = (u >> 31) << 15, (u >> 23) & 0xFF, u & 0x7FFFFF
  M = np.where(e > 0, frac | (1 << 23), frac)
  eh = np.maximum(e - 112, 1)                      # fp16's biased exponent of the interval that holds |x|
  shift = np.minimum(13 + eh - (np.maximum(e, 1) - 112), 40)
  lower, rem, half = M >> shift, M & ((1 << shift) - 1), 1 << (shift - 1)
  q = lower + ((rem > half) | ((rem == half) & (lower & 1 == 1)))
  out = np.where((e == 255) | (eh > 30), 0x7C00, np.minimum((eh - 1) * 1024 + q, 0x7C00))
  return (sign | out).astype(np.uint16)


# ---- the patterns themselves ---------------------------------------------------------------------------------------
def test_boundary_patterns_cover_what_they_claim():
  b = ref.boundary_patterns('bf16')
  assert b.dtype == np.uint32 and b.size == 6 * 65536 == 393216 and np.unique(b).size == b.size
  assert ref.is_nan(b).sum() == 6 * 2 * 128 - 2          # (the low half 0 of 0x7F80 / 0xFF80 is an infinity)
  for u in (0, 0x80000000, 0x7F800000, 0xFF800000, 0x00010000, 0x7F7F8000, 0x7F7FFFFF, 0x3F808000, 0x3F818000):
    assert u in b, hex(u)
  f = ref.boundary_patterns('fp16')
  assert f.dtype == np.uint32 and f.size == 2 * 6 * 0x7C00 + 12
  x = f.view(F32)
  for v in (65520.0, -65520.0, 2.0 ** -25, -2.0 ** -25, 65504.0, 2.0 ** -24, 2.0 ** -14, 0.0):
    assert (x == F32(v)).any(), v
  assert (f == 0x80000000).any() and (f == 0x33000001).any() and (f == 0x32FFFFFF).any()   # -0, 2^-25's neighbours
  # every interval: a < a+ <= m- < m < m+ <= b-, and m halfway
  six = f[:6 * 0x7C00].reshape(-1, 6).astype(np.int64)
  assert (np.diff(six, axis=1) >= 0).all() and (six[:, 3] - six[:, 0] >= 2).all()
  v = six.astype(np.uint32).view(F32).astype(np.float64)
  nxt = np.append(v[1:, 0], 65536.0)
  assert ((v[:, 0] + nxt) / 2 == v[:, 3]).all()


# ---- round to nearest ------------------------------------------------------------------------------------------------
def test_bf16_nearest_equals_torch_on_every_boundary_pattern():
  u = ref.boundary_patterns('bf16')
  got, want = ref.bf16_nearest(u), torch_nearest(u, 'bf16')
  nan = ref.is_nan(u)
  np.testing.assert_array_equal(got[~nan], want[~nan])
  assert ref.is_nan16(got[nan], 'bf16').all() and ref.is_nan16(want[nan], 'bf16').all()
  assert (got[nan] == 0x7FC0).all()
  assert not ref.is_nan16(got[~nan], 'bf16').any()
  # the decisions by name: ties go to even, the largest finite value carries into infinity
  assert ref.bf16_nearest(np.uint32(0x3F808000)) == 0x3F80 and ref.bf16_nearest(np.uint32(0x3F818000)) == 0x3F82
  assert ref.bf16_nearest(np.uint32(0x7F7F8000)) == 0x7F80 and ref.bf16_nearest(np.uint32(0xFF7FFFFF)) == 0xFF80
  assert ref.bf16_nearest(np.uint32(0x80000000)) == 0x8000 and ref.bf16_nearest(np.uint32(0x00008000)) == 0x0000


def test_fp16_nearest_equals_torch_and_the_integer_restatement():
  u = ref.boundary_patterns('fp16')
  got, want = ref.fp16_nearest(u), torch_nearest(u, 'fp16')
  nan = ref.is_nan(u)
  assert nan.sum() == 4
  np.testing.assert_array_equal(got[~nan], want[~nan])
  assert ref.is_nan16(got[nan], 'fp16').all() and ref.is_nan16(want[nan], 'fp16').all()
  np.testing.assert_array_equal(got[~nan], rne_fp16_integers(u[~nan]))
  # the integer restatement on the bf16 side's patterns too (every fp32 exponent, both signs)
  b = ref.boundary_patterns('bf16')
  b = b[~ref.is_nan(b)]
  np.testing.assert_array_equal(ref.fp16_nearest(b), rne_fp16_integers(b))
  one = lambda x: int(ref.fp16_nearest(ref.bits32(F32(x))).reshape(-1)[0])   # noqa: E731
  assert one(65520.0) == 0x7C00 and one(-65520.0) == 0xFC00 and one(np.nextafter(F32(65520), F32(0))) == 0x7BFF
  assert one(2.0 ** -25) == 0 and one(np.nextafter(F32(2.0 ** -25), F32(1))) == 1 and one(-2.0 ** -25) == 0x8000
  assert one(1.5 * 2.0 ** -24) == 2 and one(2.5 * 2.0 ** -24) == 2           # subnormal ties, to even
  assert one(1.0 + 2.0 ** -11) == 0x3C00 and one(1.0 + 3 * 2.0 ** -11) == 0x3C02


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_upcasts_are_exact_on_every_pattern(dtype):
  h = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
  up = ref.upcast(h, dtype)
  assert up.dtype == F32
  nan = ref.is_nan16(h, dtype)
  assert nan.sum() == (2 * 127 if dtype == 'bf16' else 2 * 1023)
  np.testing.assert_array_equal(np.isnan(up), nan)
  np.testing.assert_array_equal(ref.bits32(up)[~nan], torch_up(h, dtype)[~nan])
  if dtype == 'bf16':
    np.testing.assert_array_equal(ref.bits32(up), h.astype(np.uint32) << 16)      # payloads included
  else:    # the value from the fields, in float64 (exact)
    s, e, m = h >> 15, (h >> 10) & 0x1F, (h & 0x3FF).astype(np.float64)
    val = np.where(e == 0, m * 2.0 ** -24, (1024 + m) * 2.0 ** (e.astype(np.float64) - 25))
    val = np.where(s == 1, -val, val)
    fin = e != 31
    np.testing.assert_array_equal(up[fin].astype(np.float64), val[fin])
    np.testing.assert_array_equal(np.signbit(up[fin]), s[fin] == 1)
    assert up[0x7C00] == np.inf and up[0xFC00] == -np.inf
  np.testing.assert_array_equal(ref.round_nearest(ref.bits32(up), dtype)[~nan], h[~nan])


# ---- the noise -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def noise_cases():
  rows = np.arange(1024)
  return {(s, c): ref.noise(SEED, s, c, rows, 64) & np.uint32(0xFFFF) for s in NOISE_STEPS for c in NOISE_COLS}


def within_six_sd(share, p, n, what):
  sd = np.sqrt(p * (1 - p) / n)
  assert abs(share - p) <= 6 * sd, f'{what}: {share:.5f}, expected {p:.5f} +- {6 * sd:.5f} ({(share - p) / sd:+.2f} sd)'


def check_noise_shares(n16, what):
  """The bounds on 16 noise bits of N elements: the share that carries for an increment L."""
  n16 = np.asarray(n16, np.int64).reshape(-1)
  N = n16.size
  for L in (0x4000, 0x8000, 0xC000):
    within_six_sd(float((n16 + L >= 65536).mean()), L / 65536.0, N, f'{what}: L = {L:#x}')
  assert int((n16 + 1 >= 65536).sum()) <= 12, f'{what}: L = 1'                 # Poisson, mean N / 65536
  assert int((n16 + 0xFFFF >= 65536).sum()) >= N - int(round(12 * N / 65536.0)), f'{what}: L = 0xFFFF'


def test_noise_shares_per_increment(noise_cases):
  for (s, c), n16 in noise_cases.items():
    assert n16.size == 65536
    check_noise_shares(n16, f'step {s} column {c}')


def test_noise_is_independent_along_rows_steps_and_columns(noise_cases):
  up = {k: v >= 0x8000 for k, v in noise_cases.items()}
  for (s, c), b in up.items():
    within_six_sd(float((b[:, 1:] == b[:, :-1]).mean()), 0.5, b[:, 1:].size, f'step {s} column {c}: along a row')
    within_six_sd(float((b[1:] == b[:-1]).mean()), 0.5, b[1:].size, f'step {s} column {c}: neighbouring rows')
  for c in NOISE_COLS:
    for s0, s1 in ((0, 1), (1, 2 ** 32 - 1), (2 ** 32 - 1, 0)):
      within_six_sd(float((up[s0, c] == up[s1, c]).mean()), 0.5, 65536, f'column {c}: steps {s0} and {s1}')
  for s in NOISE_STEPS:
    for c0, c1 in ((0, 1), (1, 69), (69, 0)):
      within_six_sd(float((up[s, c0] == up[s, c1]).mean()), 0.5, 65536, f'step {s}: columns {c0} and {c1}')


def test_noise_formula_by_hand_and_the_upper_row_word():
  def fmix(h):
    h ^= h >> 16
    h = h * 0x85EBCA6B & 0xFFFFFFFF
    h ^= h >> 13
    h = h * 0xC2B2AE35 & 0xFFFFFFFF
    return h ^ h >> 16

  def one(seed, step, c, r, k):
    base = fmix(seed ^ fmix((step + 0x9E3779B9 * (c + 1)) & 0xFFFFFFFF))
    rowh = fmix(fmix(base ^ (r & 0xFFFFFFFF)) ^ (r >> 32))
    return fmix((rowh + 0x9E3779B9 * (k + 1)) & 0xFFFFFFFF)

  rows = np.array([0, 1, 1023, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 7], np.int64)
  for step in NOISE_STEPS:
    for c in NOISE_COLS:
      got = ref.noise(SEED, step, c, rows, 5)
      want = [[one(SEED, step, c, int(r), k) for k in range(5)] for r in rows]
      np.testing.assert_array_equal(got, np.array(want, np.uint32))
  lo = ref.noise(SEED, 0, 0, np.array([1], np.int64), 64)
  hi = ref.noise(SEED, 0, 0, np.array([2 ** 32 + 1], np.int64), 64)
  assert (lo != hi).mean() > 0.9                                    # the upper word enters


def test_stochastic_restatement_properties_on_every_boundary_pattern():
  u = ref.boundary_patterns('bf16')
  n = ref.noise(SEED, 1, 0, np.arange(u.size // 256), 256).reshape(-1)
  got = ref.bf16_stochastic(u, n).astype(np.int64)
  special = (u & 0x7F800000) == 0x7F800000
  down = (u >> 16).astype(np.int64)
  assert ((got == down) | (got == down + 1))[~special].all()
  assert (got == down)[~special & ((u & 0xFFFF) == 0)].all()
  np.testing.assert_array_equal(got[special], ref.bf16_nearest(u[special]))


# ---- the sums against the float64 reference ---------------------------------------------------------------------------
def small_column(rng, dtype, rows, dim):
  return ref.round_nearest(ref.bits32(rng.uniform(-2, 2, size=(rows, dim)).astype(F32)), dtype)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('combiner', ['sum', 'mean', 'sqrtn'])
def test_forward_rows_within_the_bound_of_the_float64_forward(combiner, dtype):
  rng = np.random.RandomState(5)
  for rows, dim, bucket in ((7, 3, 0), (64, 16, 64), (13, 20, 0)):
    bits = small_column(rng, dtype, rows, dim)
    t32 = ref.upcast(bits, dtype)
    lens = rng.randint(0, 7, size=40)
    splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    for sp, n in ((None, 40), (splits, int(splits[-1]))):
      ids = rng.randint(-3, rows + 3, size=n) if not bucket else rng.randint(-1000, 1000, size=n)
      for w in (None, rng.uniform(0.1, 2, size=n).astype(F32)):
        got = ref.forward_rows(bits, dtype, ids, sp, w, combiner, bucket)
        comb = combiner if (sp is not None or w is not None) else 'sum'   # (one id, unweighted: the row itself)
        want, mag = reference.forward64(t32, ids, sp, w, comb, 0.0, bucket)
        assert got.dtype == F32
        assert_sums_close(got, want, mag, err_msg=f'{dtype} {combiner} rows {rows} ragged {sp is not None}')


def test_forward_rows_edges_by_hand():
  bits = ref.round_nearest(ref.bits32(np.array([[1.0, -2.0], [0.5, 4.0], [-0.0, 3.0]], F32)), 'fp16')
  ids = np.array([0, 2, -1, 1, 3, 1])
  sp = np.array([0, 2, 2, 5, 6])
  out = ref.forward_rows(bits, 'fp16', ids, sp, None, 'mean')
  np.testing.assert_array_equal(out, np.array([[0.5, 0.5], [0, 0], [F32(0.5) / F32(3), F32(4) / F32(3)], [0.5, 4.0]], F32))
  w = np.array([2.0, -2.0, 5.0, 0.0, 1.0, 0.0], F32)
  out = ref.forward_rows(bits, 'fp16', ids, sp, w, 'mean')      # segment 0: W = 0; segment 2: only id 1 (w = 0) is valid
  np.testing.assert_array_equal(out, np.array([[0, 0], [0, 0], [0, 0], [0, 0]], F32))
  out = ref.forward_rows(bits, 'fp16', ids, None, w, 'sqrtn')
  np.testing.assert_array_equal(out, np.array([[1, -2], [0, -3], [0, 0], [0, 0], [0, 0], [0, 0]], F32))
  assert np.signbit(out[1, 0]) == np.signbit(F32(-0.0) * F32(-2.0) / F32(2.0))
  assert ref.forward_rows(bits, 'fp16', ids[:0], None, None).shape == (0, 2)
  # divisor: row = floormod(id, bucket) // divisor
  out = ref.forward_rows(bits, 'fp16', np.array([-1, 4]), None, None, bucket=7, divisor=3)
  np.testing.assert_array_equal(out, ref.upcast(bits, 'fp16')[[2, 1]])


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('optimizer', ['sgd', 'adagrad', 'rowwise_adagrad'])
def test_apply_step_within_half_an_ulp_of_the_float64_step(optimizer, dtype):
  """round(rule(...)) lies within half an ulp of the 16-bit type (2^-8 / 2^-11 relative; values stay in the normal
  range) plus the fp32 bound of the float64 step."""
  rng = np.random.RandomState(6)
  half_ulp = 2.0 ** (-8 if dtype == 'bf16' else -11)
  lr = 0.05
  for rows, dim in ((7, 3), (40, 16)):
    bits = small_column(rng, dtype, rows, dim)
    w = ref.upcast(bits, dtype).astype(np.float64)
    urows = np.concatenate([rng.permutation(rows)[:rows // 2 + 1], [-1, rows]])
    g = rng.randn(urows.size, dim).astype(F32)
    acc = rng.uniform(0.1, 0.9, size=(rows, 1 if optimizer == 'rowwise_adagrad' else dim)).astype(F32)
    slots = [] if optimizer == 'sgd' else [acc]
    new_bits, new_slots = ref.apply_step(bits, dtype, slots, urows, g, optimizer, lr, {'epsilon': 1e-8})
    st, g64 = urows[:-2], g[:-2].astype(np.float64)
    want = w.copy()
    if optimizer == 'sgd':
      want[st] -= lr * g64
    elif optimizer == 'adagrad':
      a = acc[st] + g64 * g64
      want[st] -= lr * g64 / np.sqrt(a)
      assert_sums_close(new_slots[0][st], a, a, err_msg='accumulator')
    else:
      a = acc[st, 0] + (g64 * g64).sum(1) / dim
      want[st] -= (lr / (np.sqrt(a) + 1e-8))[:, None] * g64
      assert_sums_close(new_slots[0][st, 0], a, a, err_msg='row accumulator')
    got = ref.upcast(new_bits, dtype).astype(np.float64)
    mag = np.abs(w) + np.abs(want - w)
    assert (np.abs(got - want) <= half_ulp * np.abs(want) + REL * mag + FLOOR).all()
    outside = np.setdiff1d(np.arange(rows), st)
    np.testing.assert_array_equal(new_bits[outside], bits[outside])
    assert (new_bits[st] != bits[st]).any()
    if slots:
      np.testing.assert_array_equal(new_slots[0][outside], acc[outside])
      np.testing.assert_array_equal(slots[0], acc)                # the arguments are left alone


def test_apply_step_adam_and_ftrl_are_the_rules_then_the_rounding():
  rng = np.random.RandomState(7)
  rows, dim = 9, 4
  bits = small_column(rng, 'bf16', rows, dim)
  st = np.array([3, 0, 8])
  g = rng.randn(3, dim).astype(F32)
  m, v = rng.uniform(-0.1, 0.1, size=(rows, dim)).astype(F32), np.full((rows, dim), 0.01, F32)
  for rounding in ('nearest', 'stochastic'):
    nb, (nm, nv) = ref.apply_step(bits, 'bf16', [m, v], st, g, 'adam', 0.05, {'powers': (F32(0.9), F32(0.999))},
                                  rounding=rounding, seed=SEED, step=3, col=2)
    w32, m2, v2 = ref.upcast(bits, 'bf16').copy(), m.copy(), v.copy()
    reference.adam_step(w32, m2, v2, st, g, 0.05, (F32(0.9), F32(0.999)))
    want = bits.copy()
    want[st] = ref.bf16_nearest(ref.bits32(w32[st])) if rounding == 'nearest' else ref.round_rows(w32[st], st, SEED, 3, 2)
    np.testing.assert_array_equal(nb, want)
    np.testing.assert_array_equal(nm, m2)
    np.testing.assert_array_equal(nv, v2)
  a, z = np.full((rows, dim), 0.1, F32), rng.uniform(-1, 1, size=(rows, dim)).astype(F32)
  hyper = dict(l1=0.05, l2=1e-5, l2_shrinkage=0.01, lr_power=-0.5)
  nb, (na, nz) = ref.apply_step(bits, 'bf16', [a, z], st, g, 'ftrl', 0.05, hyper)
  w32, a2, z2 = ref.upcast(bits, 'bf16').copy(), a.copy(), z.copy()
  reference.ftrl_step(w32, a2, z2, st, g, 0.05, **hyper)
  want = bits.copy()
  want[st] = ref.bf16_nearest(ref.bits32(w32[st]))
  np.testing.assert_array_equal(nb, want)
  np.testing.assert_array_equal(na, a2)
  np.testing.assert_array_equal(nz, z2)
