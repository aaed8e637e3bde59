"""Sharded lookups with 16-bit outputs on the GPU, bit for bit: the stitch hbk_lookup_fwd_runs_out16 against a numpy
restatement, the driver against the fp32 driver followed by torch's cast, the layer against the fp32-output layer."""
import functools

import numpy as np
import pytest
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (HashTable, LowpShardedGroupLookup, LowpShardedHashGroupLookup,
                                         ShardedGroupLookup, ShardedHashGroupLookup)
from tests.support import exact
from tests.support import lowp_ref as ref
from tests.test_gpu_lowp_sharded import (B, BF, CODE, DEV, F32, HF, NAME, REP, SHD, WIDTH, World, bits16, dev, fc,
                                         from_bits16, host, layer_columns, make_comms, pattern_table, world_run)

pytestmark = pytest.mark.gpu
DIMS, ROWS, SEGS = (1, 3, 4, 12, 16, 40, 64, 72, 128, 256), 200, 70
KINDS = {'fp32': None, 'wire_half': HF, 'bf16': BF, 'fp16': HF}
COMB = {'sum': _lib.COMBINER_SUM, 'mean': _lib.COMBINER_MEAN, 'sqrtn': _lib.COMBINER_SQRTN}


def restate(table, ids, sp, w, combiner):
  """include/hbk.h, "16-bit outputs", in plain float32 operations, one id at a time."""
  n_seg = ids.size if sp is None else sp.size - 1
  out = np.zeros((n_seg, table.shape[1]), F32)
  ok = (ids >= 0) & (ids < table.shape[0])
  with np.errstate(all='ignore'):
    for s in range(n_seg):
      if sp is None:
        div = F32(1) if w is None or combiner == 'sum' else w[s] if combiner == 'mean' else np.sqrt(w[s] * w[s])
        if ok[s] and div != 0:
          e = table[ids[s]] if w is None else table[ids[s]] * w[s]
          out[s] = e if w is None or combiner == 'sum' else e / div
        continue
      acc, wsum = np.zeros(table.shape[1], F32), F32(0)
      for j in range(sp[s], sp[s + 1]):
        if ok[j]:
          acc = acc + (table[ids[j]] if w is None else table[ids[j]] * w[j])
          wsum = wsum + (0 if w is None else w[j] * w[j] if combiner == 'sqrtn' else w[j])
      div = F32(sp[s + 1] - sp[s]) if w is None else wsum
      div = div if combiner == 'mean' else np.sqrt(div)
      out[s] = acc if combiner == 'sum' or (w is None and div == 0) else acc / div if div != 0 else 0
  return out


class Col:
  """One column: `rows` logical rows in runs at `start`, laid into a buffer so that the table pointer sits P elements
  in: run 0 at base 4 (a multiple of 4, not of 8), the last run below the pointer (a negative base), the others
  empty."""

  def __init__(self, rng, dim, kind, start, finite):
    dt = KINDS[kind]
    if dt is None:   # fp32 rows: the patterns that decide every rounding of either output type
      pool = np.concatenate([ref.boundary_patterns(ref.BF16)[::97], ref.boundary_patterns(ref.FP16)[::53]])
      if finite:
        pool = pool[(pool & 0x7F800000) != 0x7F800000]
      self.logical = pool[rng.randint(0, pool.size, size=(ROWS, dim))].view(F32)
      bits = self.logical
    else:
      bits = pattern_table(rng, ROWS, dim, dt, finite)
      self.logical = ref.upcast(bits, NAME[dt])
    if finite:       # ... but one row of +inf and one of -inf: a sum may meet them, and each other
      bits[7], bits[8] = {None: (np.inf, -np.inf), BF: (0x7F80, 0xFF80), HF: (0x7C00, 0xFC00)}[dt]
      self.logical = bits if dt is None else ref.upcast(bits, NAME[dt])
    start = np.asarray(start, np.int64)
    cnt = np.diff(np.append(start, ROWS))
    if start.size == 3:
      P = (int(cnt[-1]) * dim + 15) // 8 * 8
      base = np.array((4, 12344, 4 - P), np.int64)
    else:            # many runs: the logical order with 4 elements between runs
      P, base = 0, start * dim + 4 * np.arange(start.size)
    buf = np.full(P + int(base[np.nonzero(cnt)[0]].max()) + int(cnt.max()) * dim + 8, 0x7FC1, bits.dtype)
    for k in np.nonzero(cnt)[0]:
      buf[P + base[k]:P + base[k] + cnt[k] * dim] = bits[start[k]:start[k] + cnt[k]].reshape(-1)
    self.buf = dev(buf) if dt is None else from_bits16(buf, dt)
    self.ptr = self.buf.data_ptr() + P * self.buf.element_size()
    self.code = _lib.OUT16_TABLE_FP32 if dt is None else CODE[dt]
    self.start, self.base, self.dim = dev(start), dev(base), dim


@functools.lru_cache(maxsize=None)
def case(kind, combiner, weighted, ragged, dims=DIMS, start=(0, 80, 80)):
  """The columns, their inputs and the restated fp32 rows: computed once per kind and arguments, never changed."""
  rng = np.random.RandomState(31)
  cols, inputs, want = [], [], []
  for c, d in enumerate(dims):
    col = Col(rng, d, kind, start, finite=ragged)
    sp = None
    if ragged:
      lens = rng.choice([0, 0, 1, 2, 3, 5, 9], size=SEGS)
      lens[0], lens[1], lens[5], lens[9] = 0, 2, 2, 67            # empty, the zero-divisor one, one longer than a wave
      sp = exact.splits_of(lens)
    k = SEGS if sp is None else int(sp[-1])
    ids = rng.randint(-3, ROWS + 3, size=k).astype(np.int32 if c % 2 else np.int64)
    w = None
    if weighted:
      w = rng.choice([-2.0, -0.5, 0.0, 0.25, 1.0, 1.5], size=k).astype(F32)
      if ragged:
        ids[sp[1]:sp[2]] = (1, 2)
        w[sp[1]:sp[2]] = (0.0, 0.0) if combiner == 'sqrtn' else (1.0, -1.0)
    cols.append(col)
    inputs.append((dev(ids), None if sp is None else dev(sp), None if w is None else dev(w)))
    want.append(torch.from_numpy(restate(col.logical, ids, sp, w, combiner)))
  return cols, inputs, want


def run_stitch(cols, inputs, outs, out_dtype, combiner, chunk=0, strides=None):
  n = len(cols)
  a = (_lib.Out16RunsColumn * n)()
  for c, (col, (ids, sp, w)) in enumerate(zip(cols, inputs)):
    h = a[c].col
    h.table, h.table_dtype, h.rows, h.dim = col.ptr, col.code, ROWS, col.dim
    h.ids, h.n_ids, h.ids_dtype = ids.data_ptr(), ids.numel(), _lib.torch_dtype_code(ids.dtype)
    h.row_splits = None if sp is None else sp.data_ptr()
    h.n_segments = ids.numel() if sp is None else sp.numel() - 1
    h.divisor, h.combiner, h.out, h.out_dtype = 1, COMB[combiner], outs[c].data_ptr(), CODE[out_dtype]
    h.chunk_elems = chunk
    h.out_stride = strides[c] if strides else 0
    h.id_weights = None if w is None else w.data_ptr()
    a[c].run_start, a[c].run_base, a[c].n_runs = col.start.data_ptr(), col.base.data_ptr(), col.start.numel()
  _lib.check(_lib.lib().hbk_lookup_fwd_runs_out16(n, a, _lib.current_stream(torch.device(DEV))))
  torch.cuda.synchronize()


def same16(got, want, what):
  """Bit for bit; where the reference has a NaN a NaN (IEEE 754 pins no payload through arithmetic or a conversion)."""
  g, w = bits16(got), bits16(want)
  nan = host(torch.isnan(want.float()))
  assert g.shape == w.shape and (host(torch.isnan(got.float())) == nan).all(), what
  bad = (g != w) & ~nan
  assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}'


@pytest.mark.parametrize('chunk', [0, 4, 8])
@pytest.mark.parametrize('ragged', [False, True], ids=['one_id', 'ragged'])
@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('combiner', ['sum', 'mean', 'sqrtn'])
@pytest.mark.parametrize('out_dtype', [BF, HF], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('kind', list(KINDS))
def test_stitch_equals_the_restatement(kind, out_dtype, combiner, weighted, ragged, chunk, **kw):
  cols, inputs, want = case(kind, combiner, weighted, ragged, **kw)
  outs = [torch.full(tuple(w.shape), -7.0, dtype=out_dtype, device=DEV) for w in want]
  run_stitch(cols, inputs, outs, out_dtype, combiner, chunk)
  for col, o, w in zip(cols, outs, want):
    same16(o, w.to(out_dtype), f'dim {col.dim}')


@pytest.mark.parametrize('kind', ['fp32', 'bf16'])
def test_stitch_walks_more_than_64_runs(kind):
  start = tuple(min(3 * k, 150) for k in range(65))               # 3-row runs; runs 50 .. 63 are empty
  test_stitch_equals_the_restatement(kind, BF, 'mean', True, True, 0, dims=(3, 16, 72), start=start)


@pytest.mark.parametrize('pitch', [400, 397])
def test_blocks_of_a_wider_tensor_keep_what_lies_between(pitch):
  offsets = (5, 16, 40, 120) if pitch % 8 == 0 else (5, 16)   # (an odd pitch: one element per lane, dim <= 64)
  cols, inputs, want = case('bf16', 'sum', False, True, dims=(3, 16, 72, 128)[:len(offsets)])
  wide = torch.full((SEGS, pitch), -7.0, dtype=HF, device=DEV)
  expect = wide.clone()
  for o, w in zip(offsets, want):
    expect[:, o:o + w.shape[1]] = w.to(HF).to(DEV)
  run_stitch(cols, inputs, [wide[:, o:] for o in offsets], HF, 'sum', strides=[pitch] * len(cols))
  same16(wide, expect, f'pitch {pitch}')


class Wide(World):   # the 72-wide ragged, weighted column behind the 4-wide one: bases at odd multiples of 4
  DIMS = (4, 72, 16, 4)


@pytest.mark.parametrize('kind,dedup', [('fp32', False), ('fp32', True), ('wire16', False), ('wire16', True),
                                        ('table', True), ('float', False)])
@pytest.mark.parametrize('world', [1, 3])
def test_driver_equals_the_fp32_driver_cast(world, kind, dedup):
  """Two launches with refilled ids, then backward + SGD, against the same driver without out_dtype."""
  w = Wide(500 + world, world, finite=True)
  if world > 1:   # (some base of the 72-wide column is a multiple of 4 and not of 8)
    assert any(n % 2 for r in range(world) for n in np.bincount(np.mod(w.ids[r][0], world)))

  def run(r, comm, barrier):   # pylint: disable=unused-argument
    ids, sp, wt = w.step_inputs(r)
    kw = dict(buckets=list(w.BUCKETS), combiners=list(w.COMBINERS), dedup=dedup)
    res = []
    for od in (HF, None):
      shards = w.shards(r)
      if kind in ('table', 'float'):
        drv = LowpShardedGroupLookup(shards, comm, wire=kind, out_dtype=od, **kw)
      else:
        drv = ShardedGroupLookup([s.float() for s in shards], comm, out_dtype=od,
                                 wire_dtype=torch.float16 if kind == 'wire16' else None, **kw)
      bound = drv.bind(ids, sp, sp_weights=wt)
      first = [o.clone() for o in drv.launch(bound)]
      ids[0].copy_(ids[0].flip(0))
      outs = drv.launch(bound)
      assert all(o.dtype == (od or torch.float32) for o in outs)
      drv.backward([torch.ones_like(o, dtype=torch.float32) for o in outs], apply_lr=0.5)
      torch.cuda.current_stream().synchronize()
      ids[0].copy_(ids[0].flip(0))
      res.append([o.to(HF) for o in first + outs] + [s.clone() for s in drv.shards])
      drv.close()
    return res

  for r, res in enumerate(world_run(world, run)):
    for c, (x, y) in enumerate(zip(*res)):
      ints = torch.int16 if x.element_size() == 2 else torch.int32
      assert x.dtype == y.dtype and torch.equal(x.view(ints), y.view(ints)), (r, c)


@pytest.mark.parametrize('dtype', [torch.float32, BF])
def test_driver_hash_columns_three_ranks(dtype):
  rng = np.random.RandomState(8)
  keys = [[dev(rng.randint(0, 2 ** 40, size=64).astype(np.int64)) for _ in range(2)] for _ in range(3)]

  def run(r, comm, barrier):   # pylint: disable=unused-argument
    res = []
    for od in (BF, None):
      tables = [HashTable(256, d, DEV, init_scale=0.5, seed=3 + d, dtype=dtype) for d in (4, 72)]
      cls = ShardedHashGroupLookup if dtype is torch.float32 else LowpShardedHashGroupLookup
      drv = cls(tables, comm, out_dtype=od)
      res.append([o.to(BF) for o in drv(keys[r])])
      torch.cuda.current_stream().synchronize()
      drv.close()
    return res

  for r, res in enumerate(world_run(3, run)):
    for x, y in zip(*res):
      assert torch.equal(x.view(torch.int16), y.view(torch.int16)), r


def test_driver_split_forward_and_graph_replay():
  rng = np.random.RandomState(9)
  comm = make_comms(1)[0]
  shards = [dev(rng.uniform(-2, 2, size=(300, d)).astype(F32)) for d in (4, 16, 72)]
  ids = [dev(rng.randint(-5, 305, size=64).astype(np.int64)) for _ in shards]
  new, old = ShardedGroupLookup(shards, comm, out_dtype=BF), ShardedGroupLookup(shards, comm)
  bound = new.bind(ids)
  graph = torch.cuda.CUDAGraph()
  for k in range(3):   # the second half -- the rows' way back and the 16-bit stitch -- eager, captured, replayed
    ids[k].copy_(ids[k].flip(0))
    for o in bound.outs:
      o.fill_(-1.0)
    new.launch_begin(bound)
    if k == 1:
      with torch.cuda.graph(graph):
        new.launch_end(bound)
    new.launch_end(bound) if k == 0 else graph.replay()   # pylint: disable=expression-not-assigned
    torch.cuda.synchronize()
    for x, y in zip(bound.outs, old(ids)):
      assert torch.equal(x.view(torch.int16), y.to(BF).view(torch.int16)), k
  with pytest.raises(_lib.InvalidArgumentError, match=r'torch.bfloat16.*\(out_dtype\), got torch.float32'):
    new.bind(ids, outs=[torch.zeros(64, d, device=DEV) for d in (4, 16, 72)])
  for x in (new, old, comm):
    x.close()


@pytest.mark.parametrize('table_dtype', [None, BF])
def test_layer_two_ranks_block_and_sgd_step_equal_the_fp32_output_layer(table_dtype):
  rng = np.random.RandomState(12)
  tables = {k: rng.uniform(-1, 1, size=(n, d)).astype(F32) for k, n, d in REP + [SHD]}
  feats = [{k: rng.randint(0, n, size=B).astype(np.int64) for k, n, _ in REP + [SHD]} for _ in range(2)]
  grad = exact.exact_grads(rng, (B, WIDTH), 5)

  def train(r, coll, barrier):   # pylint: disable=unused-argument
    def init(col, rows, d):   # pylint: disable=unused-argument
      t = tables[col.key]
      return dev(t[r::2].copy() if rows != t.shape[0] else t.copy())
    kw = dict(coll=coll, batch_size=B, init=init, table_dtype=table_dtype, lowp_sharded=table_dtype is not None)
    res = []
    for od in (BF, None):
      layer = fc.DenseFeatures(layer_columns(), DEV, output_dtype=od, out16_sharded=od is not None, **kw)
      out = layer({k: dev(v) for k, v in feats[r].items()})
      assert od is None or (out.dtype == BF and out.stride(0) % 8 == 0)
      layer.backward(dev(grad).to(od or torch.float32), apply_lr=0.25)
      torch.cuda.current_stream().synchronize()
      res.append([out.to(BF).clone()] + [w.clone() for w in layer.weights])
      layer.close()
    return res

  for r, (new, old) in enumerate(world_run(2, train)):
    for c, (x, y) in enumerate(zip(new, old)):
      assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (r, c)
