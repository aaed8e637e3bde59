"""The stable partition (csrc/partition.hip) at the boundaries of its kernel paths, bit for bit against the
plain restatement of tests/support/partition_ref.py (which tests/test_partition_ref.py holds to the C oracle,
to the reference's cases and to the library's host entries).  The C ABI is called directly: inputs, outputs,
indices and sizes are windows of sentinel-filled flat buffers with 16 guard elements around each, the workspace
has a guard behind it, and after every call nothing outside the windows may have changed.  Unsigned columns
travel as int32 / int64 tensors holding the bit patterns.  Nothing here has a tolerance.

  every P regime        P_EDGES x four dtypes: byte counters and bit ballots (P <= 8), one ballot per bit
                        (<= 64), LDS counters and the match-any loop (up to 16384: 64 KB of dynamic LDS, which
                        a gfx950 workgroup may ask for without a function attribute -- its limit is the CU's
                        160 KB), the mask shortcut for powers of two; every refusal by name
  launch groups         64 .. 257 columns: tile / uniform_tiles and the two-ballot search of find_col, the
                        second and third launch group with hist += tiles * P, in both forms
  one-launch limits     3072 / 3073 tiles in a call, 262144 / 262145 ids in a column
  dual modulo           P * M up to 2^31 - 2, both stages, four dtypes (the only callers of the unsigned
                        fastmod and of fastdiv by M)
  the two options       partition_sub_tiles (the sb loops, the workspace size) and partition_fixed_max (the
                        runtime-loop forms of count_shards / place)
  sync-word handover    csrc/sync.hip: a call's first kernel clears what the call before left in the other
                        half -- small after large, one kernel family after another, a replaced buffer
  repetition            the same call three times over refilled outputs
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import GroupLookup, GroupLookupGrad
from tests.support import exact
from tests.support import partition_ref as ref
from tests.support import primitives_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CODES = {'int32': _lib.INT32, 'int64': _lib.INT64, 'uint32': _lib.UINT32, 'uint64': _lib.UINT64}
CARRIER = {'int32': np.int32, 'uint32': np.int32, 'int64': np.int64, 'uint64': np.int64}
DTYPE_NAMES = tuple(CODES)
GUARD = 16
SENTINEL = {np.dtype(np.int32): -0x5a5a5a5b, np.dtype(np.int64): -0x5a5a5a5a5a5a5a5b}
WS_GUARD = 256           # bytes behind the workspace
WS_FILL = 0x5a
K_MAX_PARTITIONS = 16384


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.detach().cpu().numpy()


def _layout(lens):
  """Windows inside one flat buffer, GUARD elements in front of the first and behind each."""
  starts, pos = [], GUARD
  for n in lens:
    starts.append(pos)
    pos += int(n) + GUARD
  return starts, pos


class Call:
  """One partition call of the C ABI over windows of sentinel-filled buffers."""

  def __init__(self, dtype_name, cols, P, M=1, stage=0, want=None):
    self.dtype_name, self.dtype, self.carrier = dtype_name, ref.DTYPES[dtype_name], CARRIER[dtype_name]
    self.cols = [np.ascontiguousarray(c) for c in cols]
    assert all(c.dtype == self.dtype and c.ndim == 1 for c in self.cols)
    self.P, self.M, self.stage, self.want = P, M, stage, want
    self.lens = [int(c.size) for c in self.cols]
    self.starts, total = _layout(self.lens)
    self.size_starts, size_total = _layout([P] * len(cols))
    self.sent = SENTINEL[np.dtype(self.carrier)]
    self.h_in = np.full(total, self.sent, self.carrier)
    for c, s in zip(self.cols, self.starts):
      self.h_in[s:s + c.size] = c.view(self.carrier)
    self.d_in = dev(self.h_in)
    self.d_out = torch.empty(total, dtype=self.d_in.dtype, device=DEV)
    self.d_idx = torch.empty(total, dtype=torch.int32, device=DEV)
    self.d_sizes = torch.empty(size_total, dtype=torch.int32, device=DEV)
    self.refill()
    self.set_workspace(self.workspace_bytes())

  def refill(self):
    self.d_out.fill_(self.sent)
    self.d_idx.fill_(SENTINEL[np.dtype(np.int32)])
    self.d_sizes.fill_(SENTINEL[np.dtype(np.int32)])

  def workspace_bytes(self):
    return int(_lib.lib().hbk_partition_workspace_bytes(len(self.cols), _lib.i64_array(self.lens), self.P))

  def set_workspace(self, n_bytes):
    self.ws_bytes = int(n_bytes)
    self.d_ws = torch.full((self.ws_bytes + WS_GUARD,), WS_FILL, dtype=torch.uint8, device=DEV)

  def run(self):
    """The call on the current stream; returns its status."""
    isz = np.dtype(self.carrier).itemsize
    lib, n = _lib.lib(), len(self.cols)
    args = (_lib.ptr_array([self.d_in.data_ptr() + s * isz for s in self.starts]), _lib.i64_array(self.lens),
            _lib.ptr_array([self.d_out.data_ptr() + s * isz for s in self.starts]),
            _lib.ptr_array([self.d_sizes.data_ptr() + s * 4 for s in self.size_starts]),
            _lib.ptr_array([self.d_idx.data_ptr() + s * 4 for s in self.starts]),
            C.c_void_p(self.d_ws.data_ptr()), C.c_size_t(self.ws_bytes), _lib.current_stream())
    code = CODES[self.dtype_name]
    if self.stage == 0:
      return lib.hbk_partition_by_modulo_n(n, code, self.P, *args)
    return lib.hbk_partition_by_dual_modulo_n(n, code, self.P, self.M, self.stage, *args)

  def issue(self):
    _lib.check(self.run())

  def _outside(self, flat, starts, lens, what):
    outside = np.ones(flat.size, bool)
    for n, s in zip(lens, starts):
      outside[s:s + n] = False
    sent = SENTINEL[flat.dtype]
    touched = np.flatnonzero(outside & (flat != sent))
    assert touched.size == 0, ('%s: written outside the windows' % what, touched[:8].tolist(), starts[:4])

  def check(self, what):
    """Every column equals the restatement; inputs, guards and the bytes behind the workspace are as before."""
    out, idx, sizes = host(self.d_out), host(self.d_idx), host(self.d_sizes)
    np.testing.assert_array_equal(host(self.d_in), self.h_in, err_msg='%s: the inputs changed' % what)
    self._outside(out, self.starts, self.lens, what + ' output')
    self._outside(idx, self.starts, self.lens, what + ' indices')
    self._outside(sizes, self.size_starts, [self.P] * len(self.cols), what + ' sizes')
    tail = host(self.d_ws[self.ws_bytes:])
    assert (tail == WS_FILL).all(), '%s: written behind the workspace' % what
    want = self.want or [ref.partition(c, self.P, self.M, self.stage) for c in self.cols]
    for k, (n, s, zs) in enumerate(zip(self.lens, self.starts, self.size_starts)):
      got = (out[s:s + n].view(self.dtype), sizes[zs:zs + self.P], idx[s:s + n])
      ref.assert_partition(got, want[k], '%s %s' % (what, self.dtype_name), self.P, self.M, self.stage, column=k)

  def check_untouched(self, what):
    """A refused call: every output element still holds its sentinel."""
    for t in (self.d_out, self.d_idx, self.d_sizes):
      a = host(t)
      assert (a == SENTINEL[a.dtype]).all(), '%s: a refused call wrote something' % what
    assert (host(self.d_ws) == WS_FILL).all(), '%s: a refused call wrote to the workspace' % what


def _refused(call, word, what):
  rc = call.run()
  msg = _lib.lib().hbk_last_error().decode()
  torch.cuda.synchronize()
  assert rc == _lib.INVALID_ARGUMENT and word in msg, (what, rc, msg)
  call.check_untouched(what)


def _run_and_check(call, what):
  call.issue()
  torch.cuda.synchronize()
  call.check(what)


# ----------------------------------------------------------------------------------------------
# 1. every P regime
@functools.lru_cache(maxsize=4)
def _regime_case(dtype_name, P):
  """(column names, columns, expected results): LEN_EDGES columns of uniform ids and every pattern at 5000
  ids; at P = 16384 (5 tiles x 16384 words of workspace per column) eight columns."""
  dtype = ref.DTYPES[dtype_name]
  pats = ref.patterns(ref.PATTERN_LEN, P, dtype, seed=1)
  if P == K_MAX_PARTITIONS:
    named = [('uniform[%d]' % n, ref.uniform_ids(n, dtype, 11, n, P)) for n in (0, 1, 1025, 4097)]
    named += [(k, pats[k]) for k in ('shard0', 'alternating', 'descending', 'distinct')]
    assert len(named) == 8
  else:
    named = [('uniform[%d]' % n, ref.uniform_ids(n, dtype, 11, n, P)) for n in ref.LEN_EDGES]
    named += sorted(pats.items())
  cols = [x for _, x in named]
  return [k for k, _ in named], cols, [ref.partition(x, P) for x in cols]


@pytest.mark.parametrize('onepass', [1, 0])
@pytest.mark.parametrize('P', ref.P_EDGES)
@pytest.mark.parametrize('dtype_name', DTYPE_NAMES)
def test_every_partition_count_regime(hbk_option, onepass, P, dtype_name):
  hbk_option('partition_onepass', onepass)
  names, cols, want = _regime_case(dtype_name, P)
  _run_and_check(Call(dtype_name, cols, P, want=want), 'P regime (%s)' % ', '.join(names))


@pytest.mark.parametrize('onepass', [1, 0])
def test_refusals_by_name_leave_every_sentinel(hbk_option, onepass):
  hbk_option('partition_onepass', onepass)
  cols = [ref.uniform_ids(n, np.int64, 12, n) for n in (5, 1025)]
  P_ws = 4                                                # (the workspace of a call that would be accepted)
  for P, M, stage, word in ((0, 1, 0, 'num_partitions'), (K_MAX_PARTITIONS + 1, 1, 0, 'num_partitions'),
                            (0, 2, 1, 'num_partitions'), (K_MAX_PARTITIONS + 1, 2, 2, 'num_partitions'),
                            (4, 0, 1, 'modulus'), (4, 0, 2, 'modulus'), (4, -1, 1, 'modulus'),
                            (2, 1 << 30, 1, 'num_partitions * modulus'),
                            (2, 1 << 30, 2, 'num_partitions * modulus'),
                            (K_MAX_PARTITIONS, 1 << 17, 1, 'num_partitions * modulus')):
    call = Call('int64', cols, P_ws)
    call.P, call.M, call.stage = P, M, stage              # (windows and workspace stay those of P_ws)
    _refused(call, word, 'P = %d, M = %d, stage %d' % (P, M, stage))
  lib = _lib.lib()
  for stage in (0, 3):                                    # a dual-modulo call must name its stage
    call = Call('int64', cols, P_ws)
    isz = 8
    rc = lib.hbk_partition_by_dual_modulo_n(
      2, _lib.INT64, 4, 2, stage, _lib.ptr_array([call.d_in.data_ptr() + s * isz for s in call.starts]),
      _lib.i64_array(call.lens), _lib.ptr_array([call.d_out.data_ptr() + s * isz for s in call.starts]),
      _lib.ptr_array([call.d_sizes.data_ptr() + s * 4 for s in call.size_starts]),
      _lib.ptr_array([call.d_idx.data_ptr() + s * 4 for s in call.starts]),
      C.c_void_p(call.d_ws.data_ptr()), C.c_size_t(call.ws_bytes), _lib.current_stream())
    msg = lib.hbk_last_error().decode()
    torch.cuda.synchronize()
    assert rc == _lib.INVALID_ARGUMENT and 'stage' in msg, (stage, rc, msg)
    call.check_untouched('stage %d' % stage)
  # and the library still answers: the limit itself is accepted
  _run_and_check(Call('int64', cols, K_MAX_PARTITIONS), 'P at the limit after the refusals')


# ----------------------------------------------------------------------------------------------
# 2. launch groups and find_col
_FORMS = [(8, 1, 'int64'), (8, 0, 'int64'), (13, 0, 'uint32'), (65, 0, 'int64'), (100, 0, 'int32')]


@functools.lru_cache(maxsize=2)
def _columns_case(kind, n_cols, dtype_name, P):
  lens = ref.column_sets(kind, seed=2)[n_cols]
  cols = [ref.uniform_ids(n, ref.DTYPES[dtype_name], 21, k, n_cols) for k, n in enumerate(lens)]
  return cols, [ref.partition(x, P) for x in cols]


@pytest.mark.parametrize('P,onepass,dtype_name', _FORMS, ids=['P8_one', 'P8_three', 'P13', 'P65', 'P100'])
@pytest.mark.parametrize('n_cols', ref.COLUMN_COUNTS)
@pytest.mark.parametrize('kind', ['uniform', 'ragged'])
def test_launch_groups_and_find_col(hbk_option, P, onepass, dtype_name, n_cols, kind):
  hbk_option('partition_onepass', onepass)
  cols, want = _columns_case(kind, n_cols, dtype_name, P)
  _run_and_check(Call(dtype_name, cols, P, want=want), '%d %s columns' % (n_cols, kind))


@pytest.mark.parametrize('onepass', [1, 0])
@pytest.mark.parametrize('P', [8, 65])
def test_129_empty_columns(hbk_option, onepass, P):
  hbk_option('partition_onepass', onepass)
  call = Call('int64', [np.zeros(0, np.int64)] * 129, P)
  assert call.workspace_bytes() == 0
  _run_and_check(call, '129 empty columns')


@pytest.mark.parametrize('onepass', [1, 0])
@pytest.mark.parametrize('P', [8, 65])
def test_first_launch_group_empty(hbk_option, onepass, P):
  # 128 empty columns, then two with ids: the first group has no tile, the second clears and publishes
  hbk_option('partition_onepass', onepass)
  cols = [np.zeros(0, np.int64)] * 128 + [ref.uniform_ids(n, np.int64, 22, n) for n in (2049, 70)]
  for rep in range(2):
    _run_and_check(Call('int64', cols, P), '128 empty columns in front, call %d' % rep)


# ----------------------------------------------------------------------------------------------
# 3. the one-launch limits: kOneMaxGrid = 3072 tiles in a call, kOneMaxTiles = 256 tiles in a column
_LIMITS = {'3072_tiles': [262144] * 12, '3073_tiles': [262144] * 12 + [1],
           'column_of_262145': [5, 262145, 1000, 0, 70]}


@functools.lru_cache(maxsize=1)
def _limit_case(which):
  cols = [ref.uniform_ids(n, np.int32, 31, k) for k, n in enumerate(_LIMITS[which])]
  return cols, [ref.partition(x, 8) for x in cols]


@pytest.mark.parametrize('onepass', [1, 0])
@pytest.mark.parametrize('which', list(_LIMITS))
def test_one_launch_limits(hbk_option, onepass, which):
  hbk_option('partition_onepass', onepass)
  cols, want = _limit_case(which)
  tiles = sum(-(-c.size // ref.TILE) for c in cols)
  assert tiles == {'3072_tiles': 3072, '3073_tiles': 3073}.get(which, tiles)
  _run_and_check(Call('int32', cols, 8, want=want), which)


# ----------------------------------------------------------------------------------------------
# 4. dual modulo
@pytest.mark.parametrize('onepass', [1, 0])
@pytest.mark.parametrize('stage', [1, 2])
@pytest.mark.parametrize('P,M', ref.DUAL_EDGES)
@pytest.mark.parametrize('dtype_name', DTYPE_NAMES)
def test_dual_modulo_edges(hbk_option, onepass, stage, P, M, dtype_name):
  hbk_option('partition_onepass', onepass)
  dtype = ref.DTYPES[dtype_name]
  cols = [np.resize(ref.edge_ids(dtype, P, M), 3000), ref.uniform_ids(3000, dtype, 41, P, M)]
  _run_and_check(Call(dtype_name, cols, P, M, stage), 'dual modulo (edge ids, uniform)')


# ----------------------------------------------------------------------------------------------
# 5. the two options
@pytest.mark.parametrize('onepass', [1, 0])
@pytest.mark.parametrize('P', [3, 8, 9, 64, 65])
@pytest.mark.parametrize('sub', [2, 3, 8, 9])
def test_option_sub_tiles(hbk_option, onepass, P, sub):
  hbk_option('partition_onepass', onepass)
  hbk_option('partition_sub_tiles', sub)
  eff = min(sub, 8)                                       # the option is clamped to 8 passes per wave
  lens = [eff * ref.TILE - 1, eff * ref.TILE, eff * ref.TILE + 1, 2 * eff * ref.TILE + 1]
  cols = [ref.uniform_ids(n, np.int64, 51, n) for n in lens]
  cols.append(ref.patterns(lens[2], P, np.int64, seed=5)['descending'])
  call = Call('int64', cols, P)
  tiles = sum(-(-c.size // (eff * ref.TILE)) for c in cols)
  assert call.workspace_bytes() == tiles * P * 4, 'the workspace size must follow partition_sub_tiles'
  _run_and_check(call, 'partition_sub_tiles = %d' % sub)


@pytest.mark.parametrize('onepass', [1, 0])
@pytest.mark.parametrize('P', [3, 8, 9, 64, 65])
def test_workspace_sized_for_another_option_is_refused(hbk_option, onepass, P):
  hbk_option('partition_onepass', onepass)
  cols = [ref.uniform_ids(n, np.int64, 52, n) for n in (8 * ref.TILE + 1, 16 * ref.TILE)]
  hbk_option('partition_sub_tiles', 8)
  small = Call('int64', cols, P).workspace_bytes()
  assert small == (2 + 2) * P * 4
  hbk_option('partition_sub_tiles', 1)
  call = Call('int64', cols, P)
  assert call.workspace_bytes() == (9 + 16) * P * 4
  call.set_workspace(small)
  _refused(call, 'workspace too small', 'workspace of sub_tiles = 8 under sub_tiles = 1')
  call.set_workspace(call.workspace_bytes())
  _run_and_check(call, 'the same call with its own workspace')


@functools.lru_cache(maxsize=2)
def _fixed_case(P):
  pats = ref.patterns(ref.PATTERN_LEN, P, np.int64, seed=6)
  named = sorted(pats.items()) + [('distinct[%d]' % P, ref.patterns(P, P, np.int64, seed=6)['distinct'])]
  cols = [x for _, x in named]
  return cols, [ref.partition(x, P) for x in cols]


# (past 64 the lane-per-shard counters of the one-ballot-per-shard forms do not exist: the option stops there)
@pytest.mark.parametrize('onepass', [1, 0])
@pytest.mark.parametrize('fixed_max,P', [(f, P) for f in (4, 16, 64) for P in (4, 5, 8, 9, 16, 17, 64)] +
                         [(f, P) for f in (65, 100, 16384) for P in (64, 65, 100)])
def test_option_fixed_max(hbk_option, onepass, fixed_max, P):
  hbk_option('partition_onepass', onepass)
  hbk_option('partition_fixed_max', fixed_max)
  cols, want = _fixed_case(P)
  _run_and_check(Call('int64', cols, P, want=want), 'partition_fixed_max = %d' % fixed_max)


# ----------------------------------------------------------------------------------------------
# 6. the sync-word handover (default options; every call of a sequence on one fresh stream, one synchronise)
class UniqueStep:
  def __init__(self, lens, seed):
    rng = np.random.RandomState(seed)
    self.cols = [rng.randint(-20000, 20000, size=n).astype(np.int64) for n in lens]
    self.d_cols = [dev(x) for x in self.cols]

  def issue(self):
    self.res = hb.embedding.unique_n(self.d_cols)

  def check(self, what):
    for c, ((u, idx, nu), x) in enumerate(zip(self.res, self.cols)):
      wu, widx = primitives_ref.unique_first_occurrence(x)
      assert int(nu.item()) == wu.size, (what, c, int(nu.item()), wu.size)
      np.testing.assert_array_equal(host(u)[:wu.size], wu, err_msg='%s column %d: unique' % (what, c))
      np.testing.assert_array_equal(host(idx), widx, err_msg='%s column %d: index' % (what, c))


class BackwardStep:
  """A GroupLookupGrad emit backward of one column with one id: its grouping launch takes sync words too.
  With ONE column the launch group stays on the calling stream whatever bwd_streams says (helper streams are
  for calls of more than 64 or of mixed columns); the test sets bwd_streams = 0 and bwd_deterministic = 0 all
  the same, so that the words are the calling stream's by the options alone.  Values from the exact grid:
  the sum of one term is that term."""
  ROWS, DIM = 50, 8

  def __init__(self, seed):
    rng = np.random.RandomState(seed)
    self.row = int(rng.randint(0, self.ROWS))
    self.grads = exact.exact_grads(rng, (1, self.DIM), 12)
    self.table = exact.exact_tables(rng, self.ROWS, self.DIM)
    self.d_table, self.d_ids = dev(self.table), dev(np.array([self.row], np.int64))
    self.d_grads = dev(self.grads)
    self.grad = GroupLookupGrad(GroupLookup([self.d_table], None, ['sum']))

  def issue(self):
    self.res = self.grad([self.d_ids], [self.d_grads], [None], apply_lr=0.0, optimizer='sgd', emit=True)

  def check(self, what):
    (u, g, nu), = self.res
    assert int(nu.item()) == 1, (what, int(nu.item()))
    assert host(u)[:1].tolist() == [self.row], what
    exact.assert_bits_equal(host(g)[:1], self.grads, '%s: the gradient row' % what)
    exact.assert_bits_equal(host(self.d_table), self.table, '%s: the table of a call without a step' % what)


def _part_step(lens, seed, dtype_name='int64'):
  dtype = ref.DTYPES[dtype_name]
  return Call(dtype_name, [ref.uniform_ids(n, dtype, 61, seed, k) for k, n in enumerate(lens)], 8)


_LARGE, _ONE_ID, _GROWN = [65536] * 4, [1], [262144] * 12    # 2048, 8 and 24576 sync words at P = 8


def _sequence(name):
  """The steps of one sequence, fresh values in every step; large, small, large, large: the second large call
  takes the half the small one cleared, the third the other one."""
  if name == 'partition_clears_partition':
    return [_part_step(_LARGE, 1), _part_step(_ONE_ID, 2), _part_step(_LARGE, 3), _part_step(_LARGE, 4)]
  if name == 'unique_clears_partition':
    return [_part_step(_LARGE, 1), UniqueStep([3], 2), _part_step(_LARGE, 3), _part_step(_LARGE, 4)]
  if name == 'partition_clears_unique':
    return [UniqueStep([200000] * 2, 1), _part_step(_ONE_ID, 2), UniqueStep([200000] * 2, 3),
            UniqueStep([200000] * 2, 4)]
  if name == 'backward_clears_partition':
    return [_part_step(_LARGE, 1), BackwardStep(2), _part_step(_LARGE, 3), _part_step(_LARGE, 4)]
  assert name == 'growth'                                 # the second call replaces the stream's buffer
  return [_part_step(_ONE_ID, 1, 'int32'), _part_step(_GROWN, 2, 'int32'), _part_step(_ONE_ID, 3, 'int32'),
          _part_step(_GROWN, 4, 'int32')]


@pytest.mark.parametrize('name', ['partition_clears_partition', 'unique_clears_partition',
                                  'partition_clears_unique', 'backward_clears_partition', 'growth'])
def test_sync_words_handed_from_call_to_call(hbk_option, name):
  hbk_option('bwd_streams', 0)
  hbk_option('bwd_deterministic', 0)
  assert _lib.get_option('partition_onepass') == 1 and _lib.get_option('unique_onepass') == 1
  stream = torch.cuda.Stream()
  with torch.cuda.stream(stream):
    steps = _sequence(name)
    stream.synchronize()                                  # (the inputs are there; from here on no host wait)
    for step in steps:
      step.issue()
    stream.synchronize()
    for k, step in enumerate(steps):
      step.check('%s, call %d' % (name, k))
  assert _lib.get_option('sync_onepass_off') == 0, 'a wait between tiles ran out'


# ----------------------------------------------------------------------------------------------
# 7. repetition inside one process
@pytest.mark.parametrize('onepass', [1, 0])
@pytest.mark.parametrize('P', [8, 65])
@pytest.mark.parametrize('dtype_name', DTYPE_NAMES)
def test_three_calls_over_the_same_buffers(hbk_option, onepass, P, dtype_name):
  hbk_option('partition_onepass', onepass)
  _, cols, want = _regime_case(dtype_name, P)
  call = Call(dtype_name, cols, P, want=want)
  for rep in range(3):
    call.refill()
    _run_and_check(call, 'call %d of three' % rep)
