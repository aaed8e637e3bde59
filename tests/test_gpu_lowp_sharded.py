"""Low-precision sharded tables on the GPU.  Every comparison is bit for bit.

1. hbk_lowp_gather_rows_n against numpy on the bit patterns.
2. hbk_lowp_lookup_fwd_runs against hbk_group_lookup_fwd over the same runs of the upcast fp32 buffer and against
   tests/support/lowp_ref.forward_rows.
3. LowpShardedGroupLookup's forward: both wires equal each other and ShardedGroupLookup over ``shard.float()``.
4. Its backward and step: shards and slots equal lowp_ref.apply_step on the exact per-owner sums.
5. Stochastic rounding with the per-rank seed.
6. The plan's refusals at the ABI: no stepping entry touches a 2-byte shard.
7. DenseFeatures(lowp_sharded=True) on two ranks.

W = 1 runs on the real communicator, W > 1 on Collective.local_world (ranks as host threads of one process)."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (Ftrl, LazyAdam, LowpShardedGroupLookup, RowwiseAdagrad, ShardedGroupLookup)
from tests.support import exact
from tests.support import lowp_ref as ref
from tests.support import reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
BF, HF = torch.bfloat16, torch.float16
NAME = {BF: ref.BF16, HF: ref.FP16}
CODE = {BF: _lib.LOWP_BF16, HF: _lib.LOWP_FP16}
OPTIMIZERS = ('sgd', 'adagrad', 'adam', 'ftrl', 'rowwise_adagrad')
GATHER_DIMS = (1, 3, 4, 8, 12, 16, 64, 72, 128, 256)
FTRL_HYPER = dict(l1=0.01, l2=0.02, l2_shrinkage=0.0, lr_power=-0.5)
LR = 0.05
fc = hb.feature_column


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def bits16(t):
  return host(t.contiguous().view(torch.int16)).view(np.uint16)


def from_bits16(bits, dtype):
  return dev(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(dtype)


def bits32(t):
  return host(t.contiguous().view(torch.int32))


def same_bits(got, want, what=''):
  g, w = bits32(got), bits32(want)
  assert g.shape == w.shape, (what, g.shape, w.shape)
  bad = g != w
  assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} words differ, first at {tuple(np.argwhere(bad)[0])}'


def same_as_restatement(got, want, what=''):
  """fp32 `got` against the numpy restatement: the same bits, except that a NaN need only be a NaN where the
  restatement has one -- numpy's float16 -> float32 keeps a signalling NaN's quiet bit clear where the device's
  conversion sets it, and neither the header nor IEEE 754 pins the payload a NaN carries through arithmetic.  (The
  comparisons against the fp32 kernels on the upcast data stay bit for bit, NaNs included.)"""
  got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  nan = np.isnan(want)
  np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what + ': NaN positions')
  np.testing.assert_array_equal(np.where(nan, np.uint32(0), got.view(np.uint32)),
                                np.where(nan, np.uint32(0), want.view(np.uint32)), err_msg=what)


@functools.lru_cache(maxsize=None)
def pattern_pool(dtype):
  """16-bit patterns of every class: the upper halves and the rounded values of lowp_ref.boundary_patterns, with NaN
  payloads, infinities, subnormals and -0 of the type planted in front."""
  p = ref.boundary_patterns(NAME[dtype])
  special = {BF: (0x0000, 0x8000, 0x7F80, 0xFF80, 0x7F81, 0xFFC1, 0x7FFF, 0x0001, 0x807F),
             HF: (0x0000, 0x8000, 0x7C00, 0xFC00, 0x7C01, 0xFE01, 0x7FFF, 0x0001, 0x83FF)}[dtype]
  return np.concatenate([np.array(special, np.uint16), (p >> np.uint32(16)).astype(np.uint16),
                         ref.round_nearest(p, NAME[dtype])])


def pattern_table(rng, rows, dim, dtype, finite=False):
  """finite: no NaN and no infinity among the patterns -- for the tables a test ADDS rows of: which payload the sum
  of two different NaNs carries depends on the operand order the compiler chose for the add, in either kernel, and is
  nobody's contract (a NaN the arithmetic generates itself, inf - inf, is the canonical one everywhere)."""
  pool = pattern_pool(dtype)
  if finite:
    exp = np.uint16(0x7F80 if dtype is BF else 0x7C00)
    pool = pool[(pool & exp) != exp]
  b = pool[rng.randint(0, pool.size, size=rows * dim)]
  k = min(9, b.size)
  b[rng.permutation(b.size)[:k]] = pool[:k]          # the planted patterns are really there
  return b.reshape(rows, dim).astype(np.uint16)


def run_threads(world, fn, timeout=60):
  errors = []

  def wrap(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        fn(r)
        torch.cuda.current_stream().synchronize()
    except Exception as e:  # pylint: disable=broad-except
      import traceback
      errors.append((r, repr(e), traceback.format_exc()))
  threads = [threading.Thread(target=wrap, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=timeout)
  assert not errors, errors


def make_comms(world):
  if world == 1:
    return [hb.distribute.Collective(world_size=1, rank=0)]
  return hb.distribute.Collective.local_world(world)


# ---- 1. the owner gather ----------------------------------------------------------------------------------------------
def gather_width(dim, aligned=True):
  """Elements per lane by the header's rule (aligned: table, out and stride 16-byte aligned)."""
  if aligned and dim % 8 == 0:
    return 8
  if aligned and dim % 4 == 0:
    return 4
  return 1


def gather_block_rows(dim, aligned=True):
  """Rows of one 256-thread block: 4 waves x rows per wave instruction x 4 loads per lane."""
  chunks = dim // gather_width(dim, aligned)
  lpr = 1
  while lpr < chunks:
    lpr *= 2
  return 4 * (64 // lpr) * 4


def call_gather(tables, ids, outs, buckets=None, divisor=1, strides=None):
  n = len(tables)
  cols = (_lib.LowpGatherColumn * n)()
  for c in range(n):
    col = cols[c]
    col.table, col.dim, col.rows = tables[c].data_ptr(), tables[c].shape[1], tables[c].shape[0]
    col.ids, col.n_ids = ids[c].data_ptr(), ids[c].numel()
    col.ids_dtype = _lib.INT64 if ids[c].dtype == torch.int64 else _lib.INT32
    col.bucket = buckets[c] if buckets else 0
    col.divisor = divisor
    col.out = outs[c].data_ptr()
    col.out_stride = strides[c] if strides else 0
  return _lib.lib().hbk_lowp_gather_rows_n(n, cols, _lib.current_stream(torch.device(DEV)))


def want_gather(table_bits, ids, bucket, divisor):
  r, valid = ref._rows_of(ids, table_bits.shape[0], bucket, divisor)   # pylint: disable=protected-access
  return np.where(valid[:, None], table_bits[r], np.uint16(0))


@pytest.mark.parametrize('id_dtype', [np.int32, np.int64])
@pytest.mark.parametrize('dtype', [BF, HF], ids=['bf16', 'fp16'])
def test_gather_rows_every_dim_and_block_boundary(dtype, id_dtype):
  rng = np.random.RandomState(11)
  rows = 37
  bits = [pattern_table(rng, rows, d, dtype) for d in GATHER_DIMS]
  tables = [from_bits16(b, dtype) for b in bits]
  for delta in ('none', 'one', -1, 0, 1):
    # n = 0, n = 1, then one below, at and one above every column's own block row count
    if delta in ('none', 'one'):
      ns = [0 if delta == 'none' else 1] * len(GATHER_DIMS)
    else:
      ns = [gather_block_rows(d) + delta for d in GATHER_DIMS]
    ids = [rng.randint(-6, rows + 6, size=n).astype(id_dtype) for n in ns]
    outs = [torch.full((n, d), 0x5555, dtype=torch.int16, device=DEV) for n, d in zip(ns, GATHER_DIMS)]
    _lib.check(call_gather(tables, [dev(i) for i in ids], outs))
    torch.cuda.synchronize()
    for c, d in enumerate(GATHER_DIMS):
      np.testing.assert_array_equal(host(outs[c]).view(np.uint16), want_gather(bits[c], ids[c], 0, 1),
                                    err_msg=f'dim {d} n {ns[c]}')


@pytest.mark.parametrize('divisor,bucketed', [(1, False), (2, False), (3, False), (3, True), (1, True)])
def test_gather_rows_divisor_bucket_and_65_columns(divisor, bucketed):
  """65 columns: the second launch.  Negative and too-large ids give zero rows; a bucket takes the floor-mod."""
  rng = np.random.RandomState(12)
  n_cols, rows = 65, 13
  dims = [GATHER_DIMS[c % 7] for c in range(n_cols)]
  dtypes = [(BF, HF)[c % 2] for c in range(n_cols)]
  bits = [pattern_table(rng, rows, d, t) for d, t in zip(dims, dtypes)]
  tables = [from_bits16(b, t) for b, t in zip(bits, dtypes)]
  buckets = [37 + c % 3 if bucketed else 0 for c in range(n_cols)]
  ids = [rng.randint(-1000, 1000, size=70).astype(np.int64 if c % 2 else np.int32) for c in range(n_cols)]
  outs = [torch.full((70, d), 0x5555, dtype=torch.int16, device=DEV) for d in dims]
  _lib.check(call_gather(tables, [dev(i) for i in ids], outs, buckets, divisor))
  torch.cuda.synchronize()
  some_zero = False
  for c in range(n_cols):
    want = want_gather(bits[c], ids[c], buckets[c], divisor)
    some_zero = some_zero or not want.any(axis=1).all()
    np.testing.assert_array_equal(host(outs[c]).view(np.uint16), want, err_msg=f'column {c}')
  assert some_zero


def test_gather_rows_one_element_path_strided_blocks_and_refusals():
  rng = np.random.RandomState(13)
  rows, n = 37, 300
  # a table and an output one element into their buffers: one element per lane
  dims = (4, 16, 64)
  bits = [pattern_table(rng, rows, d, BF) for d in dims]
  tables, outs = [], []
  for b, d in zip(bits, dims):
    buf = torch.empty(rows * d + 1, dtype=BF, device=DEV)
    buf[1:].view(rows, d).copy_(from_bits16(b, BF))
    tables.append(buf[1:].view(rows, d))
    obuf = torch.full((n * d + 1,), 0x5555, dtype=torch.int16, device=DEV)
    outs.append(obuf[1:].view(n, d))
    assert tables[-1].data_ptr() % 4 == 2 and outs[-1].data_ptr() % 4 == 2
  ids = [rng.randint(-3, rows + 3, size=n).astype(np.int64) for _ in dims]
  _lib.check(call_gather(tables, [dev(i) for i in ids], outs))
  torch.cuda.synchronize()
  for c in range(len(dims)):
    np.testing.assert_array_equal(host(outs[c]).view(np.uint16), want_gather(bits[c], ids[c], 0, 1))
  # dim 72 on the one-element path is refused, before anything runs
  buf = torch.empty(rows * 72 + 1, dtype=BF, device=DEV)
  t72 = buf[1:].view(rows, 72)
  o72 = torch.zeros((4, 72), dtype=torch.int16, device=DEV)
  rc = call_gather([t72], [dev(np.zeros(4, np.int64))], [o72])
  assert rc == _lib.INVALID_ARGUMENT and 'dim 72' in _lib.lib().hbk_last_error().decode()
  # column blocks of a wider tensor: out_stride counts elements; what lies between the blocks stays
  dims = (8, 3, 16, 4)
  offsets, width = (0, 8, 16, 36), 40
  bits = [pattern_table(rng, rows, d, HF) for d in dims]
  tables = [from_bits16(b, HF) for b in bits]
  wide = torch.full((n, width), 0x5555, dtype=torch.int16, device=DEV)
  outs = [wide[:, o:o + d] for o, d in zip(offsets, dims)]
  _lib.check(call_gather(tables, [dev(i) for i in ids] + [dev(ids[0])], outs, strides=[width] * 4))
  torch.cuda.synchronize()
  want = np.full((n, width), 0x5555, np.uint16)
  for c, (o, d) in enumerate(zip(offsets, dims)):
    want[:, o:o + d] = want_gather(bits[c], (ids + [ids[0]])[c], 0, 1)
  np.testing.assert_array_equal(host(wide).view(np.uint16), want)
  rc = call_gather(tables[:1], [dev(ids[0])], outs[:1], strides=[4])
  assert rc == _lib.INVALID_ARGUMENT and 'out_stride' in _lib.lib().hbk_last_error().decode()


# ---- 2. the requester's stitch ------------------------------------------------------------------------------------------
class RunsColumn:
  """A column over n_runs runs of one 16-bit buffer (one run empty when there are several), its upcast fp32 twin and
  the logical table the runs spell."""

  def __init__(self, rng, dim, dtype, n_runs, total, finite=False):
    cuts = np.sort(rng.randint(0, total + 1, size=n_runs - 1)) if n_runs > 1 else np.zeros(0, np.int64)
    if n_runs > 1:
      cuts[0] = cuts[min(1, n_runs - 2)] if n_runs > 2 else cuts[0]     # (three runs: the second is empty)
    start = np.concatenate([[0], cuts]).astype(np.int64)
    counts = np.diff(np.concatenate([start, [total]]))
    if n_runs == 2:
      start = np.array([0, 0], np.int64)                                  # (two runs: the first is empty)
      counts = np.array([0, total], np.int64)
    self.dim, self.dtype, self.total, self.n_runs = dim, dtype, total, n_runs
    self.logical = pattern_table(rng, total, dim, dtype, finite)
    pad = 4 if dim % 4 == 0 else 1
    base, at = [], 8
    for k in reversed(range(n_runs)):                                     # (later runs first: bases not ascending)
      base.append(at)
      at += int(counts[k]) * dim + 5 * pad
      at = (at + pad - 1) // pad * pad
    base = np.array(base[::-1], np.int64)
    buf = np.full(at + 8, 0x7FC1 if dtype is BF else 0x7E01, np.uint16)   # NaN between the runs
    for k in range(n_runs):
      lo = int(start[k])
      buf[base[k]:base[k] + int(counts[k]) * dim] = self.logical[lo:lo + int(counts[k])].reshape(-1)
    self.buf16 = from_bits16(buf, dtype)
    self.buf32 = self.buf16.float()
    self.start, self.base = dev(start), dev(base)


def stitch_case(rng, combiner, weighted, ragged):
  dims = (3, 4, 8, 16, 64, 128)
  cols = [RunsColumn(rng, d, (BF, HF)[c % 2], 1 + c % 3, 41, finite=ragged) for c, d in enumerate(dims)]
  ids, splits, weights = [], [], []
  for c, col in enumerate(cols):
    if ragged:
      lens = rng.choice([0, 0, 1, 2, 3, 5, 9, 17], size=70)
      lens[0], lens[1], lens[5] = 0, 2, 2
      sp = exact.splits_of(lens)
      k = int(sp[-1])
    else:
      sp, k = None, 70
    i = rng.randint(-3, col.total + 3, size=k).astype(np.int32 if c % 2 else np.int64)
    w = None
    if weighted:
      w = rng.choice([-2.0, -0.5, 0.0, 0.25, 1.0, 1.5], size=k).astype(F32)
      if ragged:                                   # a zero-divisor segment: weights that cancel / are all zero
        i[sp[1]:sp[2]] = (1, 2)
        w[sp[1]:sp[2]] = (0.0, 0.0) if combiner == 'sqrtn' else (1.0, -1.0)
    ids.append(i)
    splits.append(sp)
    weights.append(w)
  return cols, ids, splits, weights


@pytest.mark.parametrize('ragged', [False, True], ids=['one_id', 'ragged'])
@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('combiner', ['sum', 'mean', 'sqrtn'])
def test_lookup_fwd_runs_equals_the_fp32_stitch_and_the_restatement(combiner, weighted, ragged):
  rng = np.random.RandomState(21)
  cols, ids, splits, weights = stitch_case(rng, combiner, weighted, ragged)
  n = len(cols)
  comb = {'sum': _lib.COMBINER_SUM, 'mean': _lib.COMBINER_MEAN, 'sqrtn': _lib.COMBINER_SQRTN}[combiner]
  d_ids = [dev(i) for i in ids]
  d_sp = [None if s is None else dev(s) for s in splits]
  d_w = [None if w is None else dev(w) for w in weights]
  n_seg = [ids[c].size if splits[c] is None else splits[c].size - 1 for c in range(n)]
  # out_stride > dim for every second column: blocks of a wider tensor
  strides = [cols[c].dim + 4 if c % 2 else 0 for c in range(n)]
  outs = [[torch.full((n_seg[c], strides[c] or cols[c].dim), -7.0, dtype=torch.float32, device=DEV) for c in range(n)]
          for _ in range(2)]
  low = (_lib.LowpLookupRunsColumn * n)()
  f32 = (_lib.LookupColumn * n)()
  for c, col in enumerate(cols):
    for dst, table, out in ((low[c].col, col.buf16, outs[0][c]), (f32[c], col.buf32, outs[1][c])):
      dst.table, dst.rows, dst.dim = table.data_ptr(), col.total, col.dim
      dst.ids, dst.n_ids = d_ids[c].data_ptr(), ids[c].size
      dst.ids_dtype = _lib.INT64 if ids[c].dtype == np.int64 else _lib.INT32
      dst.row_splits = None if d_sp[c] is None else d_sp[c].data_ptr()
      dst.n_segments, dst.divisor, dst.combiner = n_seg[c], 1, comb
      dst.out, dst.out_stride = out.data_ptr(), strides[c]
      dst.id_weights = None if d_w[c] is None else d_w[c].data_ptr()
    low[c].col.table_dtype = CODE[col.dtype]
    for dst in (low[c], f32[c]):
      dst.run_start, dst.run_base, dst.n_runs = col.start.data_ptr(), col.base.data_ptr(), col.n_runs
  stream = _lib.current_stream(torch.device(DEV))
  _lib.check(_lib.lib().hbk_lowp_lookup_fwd_runs(n, low, stream))
  _lib.check(_lib.lib().hbk_group_lookup_fwd(n, f32, stream))
  torch.cuda.synchronize()
  for c, col in enumerate(cols):
    what = f'column {c} dim {col.dim} runs {col.n_runs}'
    same_bits(outs[0][c], outs[1][c], what)
    want = ref.forward_rows(col.logical, NAME[col.dtype], ids[c], splits[c], weights[c], combiner)
    same_as_restatement(host(outs[0][c])[:, :col.dim], want, what)
    if strides[c]:
      assert (host(outs[0][c])[:, col.dim:] == -7.0).all(), what


def test_lookup_fwd_runs_refuses_a_column_without_runs():
  col = (_lib.LowpLookupRunsColumn * 1)()
  t = torch.zeros((4, 4), dtype=BF, device=DEV)
  o = torch.zeros((2, 4), dtype=torch.float32, device=DEV)
  i = dev(np.zeros(2, np.int32))
  c = col[0].col
  c.table, c.table_dtype, c.rows, c.dim = t.data_ptr(), _lib.LOWP_BF16, 4, 4
  c.ids, c.ids_dtype, c.n_ids, c.n_segments, c.divisor, c.out = i.data_ptr(), _lib.INT32, 2, 2, 1, o.data_ptr()
  rc = _lib.lib().hbk_lowp_lookup_fwd_runs(1, col, None)
  assert rc == _lib.INVALID_ARGUMENT and 'segmented-table' in _lib.lib().hbk_last_error().decode()


# ---- 3. the driver's forward --------------------------------------------------------------------------------------------
class World:
  """The columns of the driver tests: 1000 x 8 (plain ids, some outside the table), 1000 x 16 (bucketed int64 ids up
  to 2^40, ragged, weighted), 37 x 3 (bucketed) and 2 x 4 (a rank beyond the second owns nothing; rank 0 has no ids
  for it: an empty column).  Batch 48."""
  ROWS = (1000, 1000, 37, 2)
  DIMS = (8, 16, 3, 4)
  DTYPES = (BF, HF, BF, HF)
  BUCKETS = (0, 1000, 37, 0)
  COMBINERS = ('sum', 'mean', 'sum', 'sum')
  BATCH = 48

  def __init__(self, seed, world, dtypes=None, finite=False):
    rng = self.rng = np.random.RandomState(seed)
    self.world = world
    self.dtypes = dtypes or self.DTYPES
    self.n = len(self.ROWS)
    self.ids, self.splits, self.weights = [], [], []
    for r in range(world):
      sp1 = exact.exact_ragged(rng, self.BATCH, 'mean', 8)
      ids = [np.concatenate([rng.randint(0, 1000, size=self.BATCH - 3), [-5, 1000, 1003]]).astype(np.int64),
             rng.randint(0, 2 ** 40, size=int(sp1[-1])).astype(np.int64),
             rng.randint(-100, 2 ** 40, size=self.BATCH).astype(np.int64),
             rng.randint(0, 2, size=0 if r == 0 else 5).astype(np.int64)]
      self.ids.append(ids)
      self.splits.append([None, sp1, None, None])
      self.weights.append([None, exact.exact_weights(rng, sp1, int(sp1[-1]), 'mean'), None, None])
    touched = self.touched_rows()
    self.bits = []
    for c in range(self.n):
      b = pattern_table(rng, self.ROWS[c], self.DIMS[c], self.dtypes[c], finite=self.COMBINERS[c] == 'mean')   # (the ragged column)
      if finite:     # finite values in the rows a step reads, arbitrary patterns (NaNs among them) elsewhere
        fin = torch.from_numpy(rng.uniform(-2, 2, size=(touched[c].size, self.DIMS[c])).astype(F32)).to(self.dtypes[c])
        b[touched[c]] = fin.view(torch.int16).numpy().view(np.uint16)
      self.bits.append(b)

  def global_rows(self, r, c):
    """The logical row of every id of rank r's column c, and whether it names one."""
    i = self.ids[r][c]
    g = np.mod(i, self.BUCKETS[c]) if self.BUCKETS[c] else i
    return g, (g >= 0) & (g < self.ROWS[c])

  def touched_rows(self):
    out = []
    for c in range(self.n):
      rows = [self.global_rows(r, c) for r in range(self.world)]
      out.append(np.unique(np.concatenate([g[v] for g, v in rows])))
    return out

  def shard_bits(self, r, c):
    return self.bits[c][r::self.world].copy()

  def shards(self, r):
    return [from_bits16(self.shard_bits(r, c), self.dtypes[c]) for c in range(self.n)]

  def step_inputs(self, r):
    return ([dev(i) for i in self.ids[r]], [None if s is None else dev(s) for s in self.splits[r]],
            [None if w is None else dev(w) for w in self.weights[r]])

  def want_forward(self, r, c):
    return ref.forward_rows(self.bits[c], NAME[self.dtypes[c]], self.ids[r][c], self.splits[r][c], self.weights[r][c],
                            self.COMBINERS[c], bucket=self.BUCKETS[c])


@pytest.mark.parametrize('world,dedup,groups,inline', [
    (1, False, 0, 1), (1, True, 2, 0), (1, False, 0, 0), (2, False, 0, 1), (2, True, 2, 0), (3, False, 2, 0),
    (3, True, 0, 1), (4, False, 0, 0), (4, True, 2, 1)])
def test_driver_forward_both_wires_equal_the_fp32_driver(hbk_option, world, dedup, groups, inline):
  hbk_option('sharded_groups', groups)
  hbk_option('sharded_inline', inline)
  if inline and world == 1:
    hbk_option('sharded_copy_self', 1)   # (the own slice really goes through the exchange)
  w = World(300 + world, world)
  comms = make_comms(world)
  results = [None] * world

  def run(r):
    shards = w.shards(r)
    ids, sp, wt = w.step_inputs(r)
    kw = dict(buckets=list(w.BUCKETS), combiners=list(w.COMBINERS), dedup=dedup)
    drivers = [LowpShardedGroupLookup(shards, comms[r], wire='table', **kw),
               LowpShardedGroupLookup(shards, comms[r], wire='float', **kw),
               ShardedGroupLookup([s.float() for s in shards], comms[r], **kw)]
    outs = []
    for drv in drivers:
      for _ in range(2):   # (the second step reuses the grown buffers)
        o = drv(ids, sp, sp_weights=wt)
      torch.cuda.current_stream().synchronize()
      outs.append([x.clone() for x in o])
    results[r] = outs
    for drv in drivers:
      drv.close()

  run_threads(world, run)
  for r in range(world):
    table, flt, f32 = results[r]
    for c in range(w.n):
      what = f'rank {r} column {c}'
      same_bits(table[c], f32[c], what + ': 16-bit wire against the fp32 driver')
      same_bits(flt[c], f32[c], what + ': float wire against the fp32 driver')
      same_as_restatement(host(table[c]), w.want_forward(r, c), what)
  for cm in comms:
    cm.close()


# ---- 4. backward and step -----------------------------------------------------------------------------------------------
def initial_slots(rng, optimizer, shape):
  rows, dim = shape
  if optimizer == 'adagrad':
    return [rng.uniform(0.1, 0.9, size=(rows, dim)).astype(F32)]
  if optimizer in ('adam', 'ftrl'):
    return [rng.uniform(0.1, 0.9, size=(rows, dim)).astype(F32) for _ in range(2)]
  if optimizer == 'rowwise_adagrad':
    return [rng.uniform(0.1, 0.9, size=(rows, 1)).astype(F32)]
  return []


def slot_kwargs(optimizer, slots):
  if optimizer == 'adagrad':
    return dict(accums=[s[0] for s in slots])
  if optimizer == 'adam':
    return dict(moments=[tuple(s) for s in slots], adam=LazyAdam(device=DEV))
  if optimizer == 'ftrl':
    return dict(ftrl_slots=[tuple(s) for s in slots], ftrl=Ftrl(**FTRL_HYPER))
  if optimizer == 'rowwise_adagrad':
    return dict(row_accums=[s[0] for s in slots], rowwise_adagrad=RowwiseAdagrad())
  return {}


def owner_sums(w, grads, c):
  """Per owner rank: (local rows ascending, exact fp32 gradient sums) of column c over every rank's batch."""
  terms, rows = [], []
  for r in range(w.world):
    g, valid = w.global_rows(r, c)
    t = exact.id_terms(grads[r][c], w.splits[r][c], w.COMBINERS[c], w.weights[r][c])
    terms.append(t[valid])
    rows.append(g[valid])
  rows = np.concatenate(rows)
  terms = np.concatenate(terms)
  uniq, inv = np.unique(rows, return_inverse=True)
  sums = np.zeros((uniq.size, w.DIMS[c]), np.float64)
  np.add.at(sums, inv, terms)
  assert (sums.astype(F32).astype(np.float64) == sums).all(), 'the sums are not exact in fp32: shrink the case'
  out = []
  for r in range(w.world):
    mine = uniq % w.world == r
    out.append((uniq[mine] // w.world, sums[mine].astype(F32)))
  return out


def restated_steps(w, grads_per_step, optimizer, slots0, rounding='nearest', seeds=None):
  """Every rank's shards and slots after the steps: lowp_ref.apply_step on the exact per-owner sums."""
  state = [[(w.shard_bits(r, c), [s.copy() for s in slots0[r][c]]) for c in range(w.n)] for r in range(w.world)]
  powers = reference.ADAM_DEFAULTS[:2]
  hyper0 = {'ftrl': FTRL_HYPER, 'rowwise_adagrad': dict(epsilon=1e-8)}.get(optimizer, {})
  for step, grads in enumerate(grads_per_step):
    hyper = dict(hyper0)
    if optimizer == 'adam':
      hyper['powers'] = powers
    for c in range(w.n):
      per_owner = owner_sums(w, grads, c)
      for r in range(w.world):
        rows, g = per_owner[r]
        b, s = state[r][c]
        state[r][c] = ref.apply_step(b, NAME[w.dtypes[c]], s, rows, g, optimizer, LR, hyper, rounding=rounding,
                                     seed=seeds[r] if seeds else 0, step=step, col=c)
    powers = reference.adam_finish(powers)
  return state, powers


@pytest.mark.parametrize('world', [1, 3])
@pytest.mark.parametrize('optimizer', OPTIMIZERS)
def test_driver_backward_and_step_equal_the_restatement(optimizer, world):
  w = World(400 + world, world, finite=True)
  rng = w.rng
  steps = 3
  grads = [[[exact.exact_grads(rng, (w.BATCH if c < 3 else w.ids[r][c].size, w.DIMS[c]), 8) for c in range(w.n)]
            for r in range(world)] for _ in range(steps)]
  slots0 = [[initial_slots(rng, optimizer, (w.shard_bits(r, c).shape[0], w.DIMS[c])) for c in range(w.n)]
            for r in range(world)]
  want, want_powers = restated_steps(w, grads, optimizer, slots0)
  comms = make_comms(world)
  results = [None] * world

  def run(r):
    ids, sp, wt = w.step_inputs(r)
    kw = dict(buckets=list(w.BUCKETS), combiners=list(w.COMBINERS))
    twins = []
    for emit in (True, False):
      shards = w.shards(r)
      slots = [[dev(s) for s in ss] for ss in slots0[r]]
      okw = slot_kwargs(optimizer, slots)
      twins.append((LowpShardedGroupLookup(shards, comms[r], wire='table', **kw, **okw), shards, slots, okw, emit))
    f32 = ShardedGroupLookup([s.float() for s in w.shards(r)], comms[r], **kw)
    slices_equal = True
    for step in range(steps):
      g = [dev(x) for x in grads[step][r]]
      f32(ids, sp, sp_weights=wt)
      ref_slices = f32.backward(g, apply_lr=0.0)
      for drv, _, _, _, emit in twins:
        drv(ids, sp, sp_weights=wt)
        res = drv.backward(g, apply_lr=LR, optimizer=optimizer, emit=emit)
        torch.cuda.current_stream().synchronize()
        if not emit:
          assert all(u is None and x is None for u, x, _ in res)
          continue
        for (u, x, k), (ru, rx, rk) in zip(res, ref_slices):
          n_u = int(k.item())
          assert n_u == int(rk.item())
          a, b = np.argsort(host(u)[:n_u]), np.argsort(host(ru)[:n_u])
          slices_equal = slices_equal and (host(u)[:n_u][a] == host(ru)[:n_u][b]).all() and \
              (host(x)[:n_u][a].view(np.uint32) == host(rx)[:n_u][b].view(np.uint32)).all()
    results[r] = dict(
      twins=[([bits16(s) for s in shards], [[host(x) for x in ss] for ss in slots],
              host(okw['adam'].beta_powers) if optimizer == 'adam' else None) for _, shards, slots, okw, _ in twins],
      slices_equal=slices_equal)
    for drv, *_ in twins:
      drv.close()
    f32.close()

  run_threads(world, run, timeout=90)
  for r in range(world):
    assert results[r]['slices_equal'], f'rank {r}: emit=True slices differ from the fp32 driver\'s'
    for which, (bits, slots, powers) in zip(('emit=True', 'emit=False'), results[r]['twins']):
      for c in range(w.n):
        what = f'{which} rank {r} column {c}'
        np.testing.assert_array_equal(bits[c], want[r][c][0], err_msg=what + ': shard')
        for k, s in enumerate(slots[c]):
          np.testing.assert_array_equal(s.view(np.uint32), want[r][c][1][k].view(np.uint32),
                                        err_msg=f'{what}: slot {k}')
      if optimizer == 'adam':   # one advance per finishing call
        np.testing.assert_array_equal(powers, np.array(want_powers, F32), err_msg=which)
  for cm in comms:
    cm.close()


# ---- 5. stochastic rounding -----------------------------------------------------------------------------------------------
def test_driver_stochastic_rounding_uses_a_seed_per_rank():
  world, seed = 2, 12345
  w = World(500, world, dtypes=(BF, BF, BF, BF), finite=True)
  rng = w.rng
  steps = 2
  grads = [[[exact.exact_grads(rng, (w.BATCH if c < 3 else w.ids[r][c].size, w.DIMS[c]), 8) for c in range(w.n)]
            for r in range(world)] for _ in range(steps)]
  seeds = [(seed + 0x9E3779B9 * r) % (1 << 32) for r in range(world)]
  slots0 = [[[] for _ in range(w.n)] for _ in range(world)]
  want, _ = restated_steps(w, grads, 'sgd', slots0, rounding='stochastic', seeds=seeds)
  comms = make_comms(world)
  results = [None] * world
  # two ranks stepping the SAME local row with the same gradient: a one-column plan of its own, after the steps above
  same_row = exact.exact_grads(np.random.RandomState(5), (1, 64), 8) * F32(2.0 ** -9)
  start = np.full((8, 64), 0x3F80, np.uint16)     # 1.0; the steps are no multiples of its ulp

  def run(r):
    ids, sp, wt = w.step_inputs(r)
    shards = w.shards(r)
    drv = LowpShardedGroupLookup(shards, comms[r], buckets=list(w.BUCKETS), combiners=list(w.COMBINERS),
                                 rounding='stochastic', seed=seed)
    assert drv.rank_seed == seeds[r]
    counters = [int(drv.step_counter.item())]
    for step in range(steps):
      drv(ids, sp, sp_weights=wt)
      drv.backward([dev(x) for x in grads[step][r]], apply_lr=LR, emit=bool(step % 2))
      torch.cuda.current_stream().synchronize()
      counters.append(int(drv.step_counter.item()))
    drv(ids, sp, sp_weights=wt)
    drv.backward([dev(x) for x in grads[0][r]], apply_lr=0.0)      # no step: no advance
    torch.cuda.current_stream().synchronize()
    counters.append(int(drv.step_counter.item()))
    drv.close()
    one = from_bits16(start, BF)
    drv1 = LowpShardedGroupLookup([one], comms[r], rounding='stochastic', seed=seed)
    drv1([dev(np.array([2 * world + r], np.int64))])                # local row 2 on every rank
    drv1.backward([dev(same_row)], apply_lr=1.0)
    torch.cuda.current_stream().synchronize()
    drv1.close()
    results[r] = ([bits16(s) for s in shards], counters, bits16(one))

  run_threads(world, run)
  for r in range(world):
    bits, counters, _ = results[r]
    assert counters == [0, 1, 2, 2], counters
    for c in range(w.n):
      np.testing.assert_array_equal(bits[c], want[r][c][0], err_msg=f'rank {r} column {c}')
  a, b = results[0][2], results[1][2]
  assert (a[[0, 1, 3, 4, 5, 6, 7]] == 0x3F80).all() and (b[[0, 1, 3, 4, 5, 6, 7]] == 0x3F80).all()
  assert (a[2] != b[2]).any(), 'two ranks rounded the same local row alike over 64 elements'
  for r, got in enumerate((a, b)):
    stepped = ref.apply_step(start, ref.BF16, [], np.array([2]), same_row, 'sgd', 1.0, rounding='stochastic',
                             seed=seeds[r], step=0, col=0)[0]
    np.testing.assert_array_equal(got, stepped)
  for cm in comms:
    cm.close()


# ---- 6. the plan's refusals -------------------------------------------------------------------------------------------------
def _last():
  return _lib.lib().hbk_last_error().decode()


def test_plan_refuses_every_step_on_a_16_bit_shard_and_returns_to_fp32():
  lib = _lib.lib()
  rows, dim, n = 64, 8, 32
  coll = hb.distribute.Collective(world_size=1, rank=0)
  stream = _lib.current_stream(torch.device(DEV))
  rng = np.random.RandomState(61)
  # the shard's 2-byte rows with a guard region behind them, in ONE allocation large enough for fp32 rows too
  buf = torch.full((rows * dim * 2 + 1024,), 0x5A5A, dtype=torch.int16, device=DEV)
  shard_bits = pattern_table(rng, rows, dim, BF)
  buf[:rows * dim].copy_(dev(shard_bits.view(np.int16).reshape(-1)))
  before = host(buf).copy()
  slot = [torch.zeros((rows, dim), dtype=torch.float32, device=DEV) for _ in range(3)]
  col = (_lib.ShardedColumn * 1)()
  col[0].shard, col[0].rows_local, col[0].dim, col[0].bucket = buf.data_ptr(), rows, dim, rows
  col[0].combiner = _lib.COMBINER_SUM
  plan = C.c_void_p()
  _lib.check(lib.hbk_sharded_create(C.byref(plan), coll._handle, 1, col, _lib.FLOAT))
  bf = (C.c_int32 * 1)(_lib.LOWP_BF16)
  try:
    assert lib.hbk_sharded_set_table_dtypes(plan, (C.c_int32 * 1)(7), 0) == _lib.INVALID_ARGUMENT
    assert lib.hbk_sharded_set_table_dtypes(plan, bf, 5) == _lib.INVALID_ARGUMENT
    _lib.check(lib.hbk_sharded_set_table_dtypes(plan, bf, _lib.LOWP_WIRE_TABLE))
    ids = dev(rng.randint(0, 10 ** 6, size=n).astype(np.int64))
    out = torch.zeros((n, dim), dtype=torch.float32, device=DEV)
    fwd = (_lib.ptr_array([ids.data_ptr()]), _lib.i64_array([n]), None, None, _lib.ptr_array([out.data_ptr()]), None)
    _lib.check(lib.hbk_sharded_lookup_fwd(plan, *fwd, stream))
    torch.cuda.synchronize()
    want = ref.forward_rows(shard_bits, ref.BF16, host(ids), bucket=rows)
    same_as_restatement(host(out), want, 'the forward of a 16-bit plan')
    g = dev(exact.exact_grads(rng, (n, dim), 8))
    urows = torch.zeros(n, dtype=torch.int64, device=DEV)
    grows = torch.zeros((n, dim), dtype=torch.float32, device=DEV)
    nu = torch.zeros(1, dtype=torch.int32, device=DEV)
    bwd = (_lib.ptr_array([g.data_ptr()]), None)
    tail = (_lib.ptr_array([urows.data_ptr()]), _lib.ptr_array([grows.data_ptr()]), _lib.ptr_array([nu.data_ptr()]),
            stream)
    one = lambda t: _lib.ptr_array([t.data_ptr()])   # noqa: E731
    adam = _lib.AdamParams(0.9, 0.999, 1e-8, slot[2].data_ptr(), 1)
    ftrl = _lib.FtrlParams(0.0, 0.0, 0.0, -0.5)
    rowwise = _lib.RowwiseAdagradParams(1e-8)
    refused = {
      'bwd apply_lr != 0': lambda: lib.hbk_sharded_lookup_bwd(plan, *bwd, C.c_float(0.1), *tail),
      'bwd_apply sgd': lambda: lib.hbk_sharded_lookup_bwd_apply(plan, *bwd, _lib.APPLY_SGD, C.c_float(0.1), *tail),
      'bwd_apply adagrad': lambda: lib.hbk_sharded_lookup_bwd_apply(plan, *bwd, _lib.APPLY_ADAGRAD, C.c_float(0.1),
                                                                    *tail),
      'bwd_apply step only': lambda: lib.hbk_sharded_lookup_bwd_apply(plan, *bwd, _lib.APPLY_SGD, C.c_float(0.1), None,
                                                                      None, tail[2], stream),
      'set_adam_slots': lambda: lib.hbk_sharded_set_adam_slots(plan, one(slot[0]), one(slot[1])),
      'set_ftrl_slots': lambda: lib.hbk_sharded_set_ftrl_slots(plan, one(slot[0]), one(slot[1])),
      'set_rowwise_adagrad_slots': lambda: lib.hbk_sharded_set_rowwise_adagrad_slots(plan, one(slot[0])),
      'bwd_adam': lambda: lib.hbk_sharded_lookup_bwd_adam(plan, *bwd, C.byref(adam), C.c_float(0.1), *tail),
      'bwd_ftrl': lambda: lib.hbk_sharded_lookup_bwd_ftrl(plan, *bwd, C.byref(ftrl), C.c_float(0.1), *tail),
      'bwd_rowwise_adagrad': lambda: lib.hbk_sharded_lookup_bwd_rowwise_adagrad(plan, *bwd, C.byref(rowwise),
                                                                                C.c_float(0.1), *tail),
      'set_max_norms': lambda: lib.hbk_sharded_set_max_norms(plan, (C.c_float * 1)(1.0)),
      'p2p_bind': lambda: lib.hbk_sharded_p2p_bind(plan, one(out), None, _lib.i64_array([n]), stream),
      'bwd_weights': lambda: lib.hbk_sharded_lookup_bwd_weights(plan, bwd[0], None, one(grows), stream),
    }
    hash_t = (_lib.ShardedHash * 1)()
    hash_t[0].keys_cache, hash_t[0].slab_count, hash_t[0].slab_size = urows.data_ptr(), rows // 8, 8
    refused['set_hash_tables'] = lambda: lib.hbk_sharded_set_hash_tables(plan, hash_t)
    for name, call in refused.items():
      rc = call()
      assert rc == _lib.UNIMPLEMENTED, (name, rc, _last())
      assert '16-bit' in _last(), (name, _last())
      torch.cuda.synchronize()
      np.testing.assert_array_equal(host(buf), before, err_msg=f'{name}: the shard or its guard region changed')
    # a zero max_norm and a table list without a hash column are no refusals
    _lib.check(lib.hbk_sharded_set_max_norms(plan, (C.c_float * 1)(0.0)))
    _lib.check(lib.hbk_sharded_set_hash_tables(plan, None))   # (drops the step: tables may have changed)
    _lib.check(lib.hbk_sharded_lookup_fwd(plan, *fwd, stream))
    # the emit form works and returns LOCAL rows
    _lib.check(lib.hbk_sharded_lookup_bwd(plan, *bwd, C.c_float(0.0), *tail))
    torch.cuda.synchronize()
    k = int(nu.item())
    assert sorted(host(urows)[:k].tolist()) == sorted(np.unique(host(ids) % rows).tolist())
    np.testing.assert_array_equal(host(buf), before)
    # NULL: an fp32 plan again, equal to a fresh one over the same buffer read as fp32 rows
    _lib.check(lib.hbk_sharded_set_table_dtypes(plan, None, 0))
    buf.view(torch.float32)[:rows * dim].copy_(dev(rng.uniform(-1, 1, size=rows * dim).astype(F32)))
    fresh = C.c_void_p()
    _lib.check(lib.hbk_sharded_create(C.byref(fresh), coll._handle, 1, col, _lib.FLOAT))
    outs = []
    for p in (plan, fresh):
      o = torch.zeros((n, dim), dtype=torch.float32, device=DEV)
      a = fwd[:4] + (_lib.ptr_array([o.data_ptr()]), None)
      _lib.check(lib.hbk_sharded_lookup_fwd(p, *a, stream))
      nu.zero_()
      _lib.check(lib.hbk_sharded_lookup_bwd(p, *bwd, C.c_float(0.0), *tail))
      torch.cuda.synchronize()
      k = int(nu.item())
      order = np.argsort(host(urows)[:k])
      outs.append((host(o).copy(), host(urows)[:k][order].copy(), host(grows)[:k][order].copy()))
    for x, y in zip(*outs):
      assert x.shape == y.shape and x.tobytes() == y.tobytes()
    table = host(buf.view(torch.float32)[:rows * dim]).reshape(rows, dim)
    np.testing.assert_array_equal(outs[0][0], table[host(ids) % rows])
    _lib.check(lib.hbk_sharded_lookup_bwd(plan, *bwd, C.c_float(0.1), *tail))     # the fused step is back
    torch.cuda.synchronize()
    lib.hbk_sharded_destroy(fresh)
    # a plan created with the fp16 wire, a clipped plan: the setter refuses
    half = C.c_void_p()
    _lib.check(lib.hbk_sharded_create(C.byref(half), coll._handle, 1, col, _lib.HALF))
    assert lib.hbk_sharded_set_table_dtypes(half, bf, 0) == _lib.UNIMPLEMENTED and 'HBK_HALF' in _last()
    lib.hbk_sharded_destroy(half)
    clipped = C.c_void_p()
    _lib.check(lib.hbk_sharded_create(C.byref(clipped), coll._handle, 1, col, _lib.FLOAT))
    _lib.check(lib.hbk_sharded_set_max_norms(clipped, (C.c_float * 1)(2.0)))
    assert lib.hbk_sharded_set_table_dtypes(clipped, bf, 0) == _lib.UNIMPLEMENTED and 'max_norm' in _last()
    lib.hbk_sharded_destroy(clipped)
  finally:
    lib.hbk_sharded_destroy(plan)
    coll.close()


# ---- 7. the layer ---------------------------------------------------------------------------------------------------------
B = 48
REP = [('a', 7, 4), ('b', 40, 8), ('c', 48, 3)]     # replicated at batch 48: they stay fp32
SHD = ('s', 1000, 8)                                # sharded: bf16 shards
WIDTH = sum(d for _, _, d in REP) + SHD[2]


def layer_columns():
  return [fc.EmbeddingColumn(k, n, d, 'sum', hot_rows=False) for k, n, d in REP + [SHD]]


def layer_kwargs(optimizer):
  return {} if optimizer == 'sgd' else dict(optimizer=optimizer)


def world_run(world, fn, timeout=90):
  comms = make_comms(world)
  barrier = threading.Barrier(world)
  results = [None] * world

  def run(r):
    try:
      results[r] = fn(r, comms[r], barrier.wait)
    except Exception:
      barrier.abort()
      raise
  try:
    run_threads(world, run, timeout)
  finally:
    for cm in comms:
      cm.close()
  return results


@pytest.mark.parametrize('optimizer', ['sgd', 'rowwise_adagrad'])
def test_layer_lowp_sharded_two_ranks_steps_and_reshards(tmp_path, optimizer):
  world, steps = 2, 3
  rng = np.random.RandomState(700 + len(optimizer))
  tables = {k: rng.uniform(-1, 1, size=(n, d)).astype(F32) for k, n, d in REP + [SHD]}
  batches = [[dict({k: rng.randint(0, n, size=B).astype(np.int64) for k, n, _ in REP + [SHD]},
                   grad=exact.exact_grads(rng, (B, WIDTH), 8)) for _ in range(world)] for _ in range(steps)]
  prefix2, prefix1 = str(tmp_path / 'w2.ckpt'), str(tmp_path / 'w1.ckpt')

  def init_for(r, w_):
    def init(col, rows, d):   # pylint: disable=unused-argument
      t = tables[col.key]
      return dev(t[r::w_].copy() if rows != t.shape[0] else t.copy())
    return init

  def feats(b):
    return {k: dev(b[k]) for k in b if k != 'grad'}

  def train(r, coll, barrier):
    kw = dict(coll=coll, batch_size=B, init=init_for(r, world), aggregate_replicated=True, **layer_kwargs(optimizer))
    low = fc.DenseFeatures(layer_columns(), DEV, table_dtype=BF, lowp_sharded=True, **kw)
    f32 = fc.DenseFeatures(layer_columns(), DEV, **kw)
    assert low.sharded == [False, False, False, True] and low.weights[3].dtype == BF
    assert all(low.weights[c].dtype == torch.float32 for c in range(3))
    for step in range(steps):
      for layer in (low, f32):
        layer(feats(batches[step][r]))
        layer.backward(dev(batches[step][r]['grad']), apply_lr=LR, optimizer=optimizer, emit=bool(step % 2))
    out = low(feats(batches[0][r])).clone()
    torch.cuda.current_stream().synchronize()
    res = dict(shard=bits16(low.weights[3]), rep=[host(low.weights[c]) for c in range(3)],
               rep32=[host(f32.weights[c]) for c in range(3)], out=host(out),
               slot=host(low.row_accums[3]) if optimizer == 'rowwise_adagrad' else None)
    low.save(prefix2, barrier=barrier)
    low.close()
    f32.close()
    return res

  got = world_run(world, train)
  # the sharded table: the numpy restatement on the exact per-owner sums
  off = WIDTH - SHD[2]
  hyper = dict(epsilon=1e-8) if optimizer == 'rowwise_adagrad' else {}
  state = []
  for r in range(world):
    bits = ref.bf16_nearest(ref.bits32(tables['s'][r::world]))
    slots = [np.zeros((bits.shape[0], 1), F32)] if optimizer == 'rowwise_adagrad' else []
    state.append((bits, slots))
  for step in range(steps):
    ids = np.concatenate([batches[step][r]['s'] for r in range(world)])
    g = np.concatenate([batches[step][r]['grad'][:, off:] for r in range(world)]).astype(np.float64)
    uniq, inv = np.unique(ids, return_inverse=True)
    sums = np.zeros((uniq.size, SHD[2]), np.float64)
    np.add.at(sums, inv, g)
    assert (sums.astype(F32).astype(np.float64) == sums).all()
    for r in range(world):
      mine = uniq % world == r
      state[r] = ref.apply_step(state[r][0], ref.BF16, state[r][1], uniq[mine] // world, sums[mine].astype(F32),
                                optimizer, LR, hyper)
  for r in range(world):
    np.testing.assert_array_equal(got[r]['shard'], state[r][0], err_msg=f'rank {r}: the bf16 shard')
    if optimizer == 'rowwise_adagrad':
      np.testing.assert_array_equal(got[r]['slot'].view(np.uint32), state[r][1][0].view(np.uint32))
    for c in range(3):   # the replicated tables are fp32 and equal the fp32 layer's
      np.testing.assert_array_equal(got[r]['rep'][c].view(np.uint32), got[r]['rep32'][c].view(np.uint32),
                                    err_msg=f'rank {r}: replicated table {c}')
      assert not np.array_equal(got[r]['rep'][c], tables[REP[c][0]])     # (they were stepped)

  # saved at W = 2, restored into W = 1 (an fp32 layer: the upcast is exact): the same forward
  def restore_one(r, coll, barrier):   # pylint: disable=unused-argument
    layer = fc.DenseFeatures(layer_columns(), DEV, batch_size=B, **layer_kwargs(optimizer))
    layer.restore(prefix2)
    outs = [host(layer(feats(batches[0][q])).clone()) for q in range(world)]
    # ... and a 16-bit layer of one rank, saved for the way back
    one = fc.DenseFeatures(layer_columns(), DEV, batch_size=B, init=init_for(0, 1), table_dtype=BF,
                           **layer_kwargs(optimizer))
    one.save(prefix1)
    return outs, [bits16(w) for w in one.weights]

  outs, one_bits = world_run(1, restore_one)[0]
  for q in range(world):
    np.testing.assert_array_equal(outs[q].view(np.uint32), got[q]['out'].view(np.uint32), err_msg=f'batch of rank {q}')

  # saved at W = 1, restored into W = 2: the same shards
  def restore_two(r, coll, barrier):
    layer = fc.DenseFeatures(layer_columns(), DEV, coll=coll, batch_size=B, table_dtype=BF, lowp_sharded=True,
                             **layer_kwargs(optimizer))
    layer.restore(prefix1, barrier=barrier)
    res = (bits16(layer.weights[3]), [host(layer.weights[c]) for c in range(3)])
    layer.close()
    return res

  back = world_run(world, restore_two)
  for r in range(world):
    np.testing.assert_array_equal(back[r][0], one_bits[3][r::world], err_msg=f'rank {r}: shard')
    for c in range(3):
      np.testing.assert_array_equal(back[r][1][c], ref.bf16_up(one_bits[c]))
