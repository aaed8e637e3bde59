"""8-bit tables on the GPU.  The quantiser and the decode against the numpy restatement (tests/support/quant8_ref.py),
byte for byte; the forward against GroupLookup over the dequantised table, bit for bit; the step against SparseApply
on the dequantised table, requantised by the restatement; the stochastic rounding against the restatement and the
binomial; Quant8LookupGrad and DenseFeatures(table_dtype='int8') against their hand compositions."""
import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd.embedding import (Ftrl, GroupLookup, GroupLookupGrad, LazyAdam, Quant8GroupLookup,
                                         Quant8LookupGrad, Quant8SparseApply, RowwiseAdagrad, SparseApply,
                                         dequantize_rows8, quantize_rows8)
from tests.support import quant8_ref as ref
from tests.support import tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
ROWS = 257
DIMS = (1, 3, 4, 16, 20, 60, 64, 128, 132, 256)
# (dim, pitch): the default pitch everywhere, one padded pitch for dims 16 and 128
SHAPES = [(d, None) for d in DIMS] + [(16, 32), (128, 144)]
OUTS = (torch.float32, torch.bfloat16, torch.float16)
OPTIMIZERS = ('sgd', 'adagrad', 'adam', 'ftrl', 'rowwise_adagrad')
_CACHE = {}


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def table_of(dim, pitch=None):
  """(fp32 rows, the restatement's table, the device table, the dequantised device table) of a shape, made once."""
  if (dim, pitch) not in _CACHE:
    v = ref.special_rows(np.random.RandomState(dim), ROWS, dim)
    t8 = ref.quantise(v, pitch)
    _CACHE[dim, pitch] = (v, t8, dev(t8), dev(ref.dequantise(t8, dim)))
  return _CACHE[dim, pitch]


def raw(x):
  """The bytes of a tensor or an array, on the host."""
  if isinstance(x, torch.Tensor):
    return host(x.contiguous().view(torch.uint8))
  return np.ascontiguousarray(x).view(np.uint8)


def same(got, want, what=''):
  """Equal shapes in bytes and equal bytes."""
  g, w = raw(got), raw(want)
  assert g.shape == w.shape, (what, g.shape, w.shape)
  bad = np.argwhere(g != w)
  assert not bad.size, f'{what}: {len(bad)} bytes differ, first at {bad[0]}'


def ragged(rng, segments, longest):
  lens = rng.randint(0, longest + 1, size=segments)
  lens[rng.randint(0, segments, size=segments // 4)] = 0
  return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def some_ids(rng, n, rows, dtype=np.int64):
  ids = rng.randint(0, rows, size=n).astype(dtype)
  if n > 4:
    ids[1], ids[n // 2] = -1, rows + 5   # an invalid and an out-of-range id
    ids[2:4] = (0, 1)                    # the zero rows
  return dev(ids)


@pytest.mark.parametrize('dim, pitch', SHAPES)
def test_quantise_and_dequantise_equal_the_restatement(dim, pitch):
  v, t8, d8, deq = table_of(dim, pitch)
  srcs = [dev(v), dev(v).to(torch.bfloat16), dev(v).to(torch.float16)]
  got = quantize_rows8(srcs, pitch=pitch)
  for g, s in zip(got, srcs):
    same(g, ref.quantise(host(s.float()), pitch), f'quantise from {s.dtype}')
  same(dequantize_rows8([d8], [dim])[0], ref.dequantise(t8, dim), 'dequantise')
  # half a code plus the two fp32 roundings at |t| <= 127; a row below 2^-100 is a zero row by definition (its scale
  # is 0: the bound does not speak of it) and decodes to +0
  err = np.abs(host(deq).astype(np.float64) - v)
  live = np.abs(v).max(axis=1) >= ref.TINY
  assert (err[live] <= 0.5001 * ref.scales(t8, dim)[live, None].astype(np.float64)).all(), err.max()
  assert not live[0] and not live[1] and live[2:].all()
  assert (t8[~live, :dim] == 128).all() and (ref.scales(t8, dim)[~live] == 0).all() and (host(deq)[~live] == 0).all()


@pytest.mark.parametrize('out_dtype', OUTS, ids=str)
@pytest.mark.parametrize('dim, pitch', SHAPES)
def test_forward_equals_group_lookup_over_the_dequantised_table(dim, pitch, out_dtype):
  _, t8, d8, deq = table_of(dim, pitch)
  rng = np.random.RandomState(dim)
  for combiner, weighted, idt in (('sum', True, np.int32), ('mean', True, np.int32), ('sqrtn', False, np.int32),
                                  ('sqrtn', True, np.int64), ('mean', False, np.int64), ('sum', False, np.int64)):
    splits = [None, dev(ragged(rng, 300, 9))]
    ids = [some_ids(rng, 300 if s is None else int(s[-1]), ROWS, idt) for s in splits]
    ws = [dev(rng.uniform(-1, 2, size=i.numel()).astype(F32)) for i in ids] if weighted else None
    if weighted:
      ws[0][5] = 0.0   # a zero divisor
    want = GroupLookup([deq, deq], combiners=combiner)(ids, splits, sp_weights=ws)
    for chunk in (None, 4):
      got = Quant8GroupLookup([d8, d8], [dim, dim], combiners=combiner, out_dtype=out_dtype, chunk_elems=chunk)(
        ids, splits, sp_weights=ws)
      for g, w in zip(got, want):
        same(g, w.to(out_dtype), f'{combiner} weighted={weighted} chunk_elems={chunk}')
  # the float64 sum of the dequantised rows, ragged and unweighted (the last call)
  if out_dtype == torch.float32:
    sp, r = host(splits[1]).astype(np.int64), host(ids[1]).astype(np.int64)
    rows = np.where((r >= 0) & (r < ROWS), host(deq).astype(np.float64)[np.clip(r, 0, ROWS - 1)].T, 0).T
    seg = np.repeat(np.arange(300), np.diff(sp))
    want64, mag = tolerance.dense_sums((300, dim), seg, rows)
    tolerance.assert_sums_close(host(got[1]), want64, mag, err_msg='float64 sum')


@pytest.mark.parametrize('n_cols', (1, 3, 65))
@pytest.mark.parametrize('out_dtype', (torch.float32, torch.bfloat16), ids=str)
def test_forward_columns_blocks_launch_and_graph(n_cols, out_dtype):
  """Mixed dims as aligned and unaligned column blocks of one wider tensor whose other bytes survive, bucket and
  divisor, a column without ids, launch() and a captured-graph replay."""
  rng = np.random.RandomState(n_cols)
  dims = [(16, 3, 64, 20, 128)[c % 5] for c in range(n_cols)]
  seg = 70
  t8 = [table_of(d)[2] for d in dims]
  deq = [table_of(d)[3] for d in dims]
  # blocks: 16-byte aligned offsets, except that every dim <= 64 column with an odd index starts one element late
  offsets, at = [], 0
  for c, d in enumerate(dims):
    at = (at + 7) // 8 * 8 + (1 if d <= 64 and c % 2 else 0)
    offsets.append(at)
    at += d
  width = (at + 8) // 8 * 8
  kw = dict(buckets=[ROWS - 7] * n_cols, combiners='mean', divisor=2)
  splits = [dev(ragged(rng, seg, 5)) if c % 3 == 1 else None for c in range(n_cols)]
  ids = [dev(rng.randint(-2 ** 40, 2 ** 40, size=seg if s is None else int(s[-1]))) for s in splits]
  want = GroupLookup(deq, **kw)(ids, splits)
  block = torch.full((seg, width), 7.0, dtype=out_dtype, device=DEV)
  look = Quant8GroupLookup(t8, dims, out_dtype=out_dtype, **kw)
  assert look.bind_block(ids, splits, block, offsets)
  expect = torch.full((seg, width), 7.0, dtype=out_dtype, device=DEV)
  for o, d, w in zip(offsets, dims, want):
    expect[:, o:o + d] = w.to(out_dtype)
  s = torch.cuda.Stream()
  graph = torch.cuda.CUDAGraph()
  look.launch()
  same(block, expect, 'launch')
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      look.launch()
  for replay in range(3):
    block.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    same(block, expect, f'graph replay {replay}')
  # no ids at all
  none = Quant8GroupLookup(t8[:1], dims[:1], out_dtype=out_dtype)([dev(np.zeros(0, np.int64))])
  assert tuple(none[0].shape) == (0, dims[0])


def slots_of(optimizer, dims):
  full = lambda d, x: torch.full((ROWS, d), x, dtype=torch.float32, device=DEV)   # noqa: E731
  if optimizer == 'adagrad':
    return dict(accums=[full(d, 0.1) for d in dims])
  if optimizer == 'adam':
    return dict(moments=[(full(d, 0.0), full(d, 0.0)) for d in dims], adam=LazyAdam(device=DEV))
  if optimizer == 'ftrl':
    return dict(ftrl_slots=[(full(d, 0.1), full(d, 0.0)) for d in dims], ftrl=Ftrl(l1=0.01, l2=0.02))
  if optimizer == 'rowwise_adagrad':
    return dict(row_accums=[full(1, 0.1) for _ in dims], rowwise_adagrad=RowwiseAdagrad())
  return {}


def slot_tensors(kw):
  out = []
  for v in kw.values():
    if isinstance(v, list):
      out += [t for e in v for t in (e if isinstance(e, tuple) else (e,))]
  return out


def some_slices(rng, dims, cap=90):
  """Distinct rows with -1 entries and an out-of-range row; n_unique below the capacity."""
  out = []
  for d in dims:
    perm = rng.permutation(ROWS).astype(np.int64)
    rows = perm[perm != 3][:cap]
    rows[3], rows[11], rows[0] = -1, ROWS + 2, 3   # (row 3: +amax and -amax)
    rows[20:22] = -1
    out.append((dev(rows), dev(rng.standard_normal((cap, d)).astype(F32)),
                dev(np.array([cap - 10], np.int32))))
  return out


STEP_DIMS = (1, 3, 16, 20, 64, 132, 256)


@pytest.mark.parametrize('optimizer', OPTIMIZERS)
def test_step_nearest_equals_sparse_apply_requantised(optimizer):
  rng = np.random.RandomState(3)
  t8 = [table_of(d)[2].clone() for d in STEP_DIMS]
  kw8, kw32 = slots_of(optimizer, STEP_DIMS), slots_of(optimizer, STEP_DIMS)
  step8 = Quant8SparseApply(t8, STEP_DIMS, **kw8)
  for step in range(3):
    slices = some_slices(rng, STEP_DIMS)
    before = [host(t) for t in t8]
    w32 = dequantize_rows8(t8, STEP_DIMS)
    SparseApply(w32, **kw32)(slices, 0.05, optimizer)
    step8(slices, 0.05, optimizer)
    for c, d in enumerate(STEP_DIMS):
      rows = host(slices[c][0])[:80]
      rows = rows[(rows >= 0) & (rows < ROWS)]
      want = before[c].copy()
      want[rows] = ref.quantise(host(w32[c])[rows])
      same(t8[c], want, f'{optimizer} step {step} dim {d}')
    for a, b in zip(slot_tensors(kw8), slot_tensors(kw32)):
      same(a, b, f'{optimizer} step {step}: slot')
  assert int(step8.step_counter.item()) == 0   # 'nearest' never touches the counter


def test_step_stochastic_equals_the_restatement_and_replays_draw_fresh_noise():
  rng = np.random.RandomState(5)
  dims = (3, 16, 132)
  t8 = [table_of(d)[2].clone() for d in dims]
  step8 = Quant8SparseApply(t8, dims, rounding='stochastic', seed=77)
  slices = some_slices(rng, dims)
  for step in range(2):
    before = [host(t) for t in t8]
    w32 = dequantize_rows8(t8, dims)
    SparseApply(w32)(slices, 0.3, 'sgd')
    step8(slices, 0.3, 'sgd')
    for c, d in enumerate(dims):
      rows = host(slices[c][0])[:80]
      rows = rows[(rows >= 0) & (rows < ROWS)]
      want = before[c].copy()
      want[rows] = ref.quantise(host(w32[c])[rows], rounding='stochastic', seed=77, step=step, col=c, rows=rows)
      same(t8[c], want, f'stochastic step {step} dim {d}')
  assert int(step8.step_counter.item()) == 2
  # replays of a captured graph: the counter advances on the device, so every replay equals the restatement at ITS step
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      step8.launch()
  for step in range(2, 5):
    before = host(t8[1])
    w32 = dequantize_rows8(t8, dims)
    SparseApply(w32)(slices, 0.3, 'sgd')
    graph.replay()
    torch.cuda.synchronize()
    rows = host(slices[1][0])[:80]
    rows = rows[(rows >= 0) & (rows < ROWS)]
    want = before.copy()
    want[rows] = ref.quantise(host(w32[1])[rows], rounding='stochastic', seed=77, step=step, col=1, rows=rows)
    same(t8[1], want, f'graph replay at step {step}')


@pytest.mark.parametrize('rounding', ('nearest', 'stochastic'))
def test_stochastic_rounding_is_unbiased_where_nearest_stalls(rounding):
  """16 384 rows of dim 16, element 0 pinned at 127.0 (scale == 1.0 exactly), the other 15 stepped 64 times by
  -lr * g = +0.25: to nearest no byte ever changes; stochastically every step is +1 with probability 1/4, so an element
  ends at Binomial(64, 1/4): mean 16, variance 12; the mean over 245 760 elements within 7 sigma = 7 sqrt(12 / 245760)
  = 0.049 < 0.05."""
  n = 16384
  v = np.zeros((n, 16), F32)
  v[:, 0] = 127.0
  t8 = quantize_rows8([dev(v)])
  start = host(t8[0])
  g = np.full((n, 16), -1.0, F32)
  g[:, 0] = 0.0
  slices = [(dev(np.arange(n, dtype=np.int64)), dev(g), dev(np.array([n], np.int32)))]
  step8 = Quant8SparseApply(t8, [16], rounding=rounding, seed=1)
  step8(slices, 0.25, 'sgd')
  for _ in range(63):
    step8.launch()
  if rounding == 'nearest':
    same(t8[0], start, 'nearest')
    return
  got = host(dequantize_rows8(t8, [16])[0])
  assert (got[:, 0] == 127.0).all()
  assert abs(got[:, 1:].astype(np.float64).mean() - 16.0) <= 0.05, got[:, 1:].mean()


def test_lookup_grad_equals_emit_then_apply():
  rng = np.random.RandomState(11)
  dims = (3, 16, 64)
  t8a, t8b = ([table_of(d)[2].clone() for d in dims] for _ in range(2))
  acc_a, acc_b = (slots_of('adagrad', dims)['accums'] for _ in range(2))
  look = Quant8GroupLookup(t8a, dims, combiners='mean')
  grad = Quant8LookupGrad(look, accums=acc_a, deterministic=True, rounding='stochastic', seed=4)
  emit = GroupLookupGrad(GroupLookup([torch.zeros(ROWS, d, device=DEV) for d in dims], combiners='mean'),
                         deterministic=True)
  hand = Quant8SparseApply(t8b, dims, accums=acc_b, rounding='stochastic', seed=4)
  for step in range(3):
    splits = [None, dev(ragged(rng, 120, 6)), None]
    ids = [some_ids(rng, 120 if s is None else int(s[-1]), ROWS) for s in splits]
    grads = [dev(rng.standard_normal((120, d)).astype(F32)) for d in dims]
    got = grad(ids, grads, splits, apply_lr=0.1, optimizer='adagrad')
    want = emit(ids, grads, splits)
    hand(want, 0.1, 'adagrad')
    for c in range(len(dims)):
      k = int(want[c][2].item())
      assert int(got[c][2].item()) == k
      same(got[c][0][:k], want[c][0][:k], 'unique_rows')
      same(got[c][1][:k], want[c][1][:k], 'grad_rows')
      same(t8a[c], t8b[c], f'table {c} step {step}')
      same(acc_a[c], acc_b[c], f'accum {c} step {step}')


@pytest.mark.parametrize('output_dtype', (None, torch.bfloat16), ids=str)
def test_layer_with_int8_tables(output_dtype, tmp_path):
  fc = hb.feature_column
  # (sum over ragged ids, sqrtn over one id and integer gradients: the reduce's sums are exact in any order)
  cols = [fc.EmbeddingColumn('a', ROWS, 16, combiner='sum'), fc.EmbeddingColumn('c', ROWS, 128, combiner='sqrtn'),
          fc.EmbeddingColumn('b', ROWS, 3, combiner='sum')]
  init = lambda col, rows, d: dev(ref.special_rows(np.random.RandomState(col.dimension), rows, col.dimension))   # noqa: E731
  layer = fc.DenseFeatures(cols, DEV, init=init, initial_accumulator_value=0.1, table_dtype='int8',
                           table_rounding='stochastic', table_seed=6, output_dtype=output_dtype)
  dims = [c.dimension for c in cols]
  for w, c in zip(layer.weights, cols):
    assert w.dtype == torch.uint8
    same(w, ref.quantise(ref.special_rows(np.random.RandomState(c.dimension), ROWS, c.dimension)), 'init')
  f32 = fc.DenseFeatures(cols, DEV, init=lambda col, rows, d: dequantize_rows8(
    [layer.weights[dims.index(col.dimension)]], [col.dimension])[0], output_dtype=output_dtype)
  t8 = [w.clone() for w in layer.weights]
  acc = [a.clone() for a in layer.accums]
  hand = Quant8SparseApply(t8, dims, accums=acc, rounding='stochastic', seed=6)
  emit = GroupLookupGrad(GroupLookup([torch.zeros(ROWS, d, device=DEV) for d in dims],
                                     [ROWS] * 3, [c.combiner for c in cols]))
  rng = np.random.RandomState(2)
  for step in range(5):
    sp = dev(ragged(rng, 96, 5))
    feats = {'a': (dev(rng.randint(0, 2 ** 40, size=int(sp[-1]))), sp), 'b': dev(rng.randint(0, 2 ** 40, size=96)),
             'c': dev(rng.randint(0, 2 ** 40, size=96))}
    out = layer(feats)
    if step == 0:
      same(out, f32(feats), 'forward')
    g = dev(rng.randint(-4, 5, size=(96, layer.width)).astype(F32))
    layer.backward(g, apply_lr=0.05, optimizer='adagrad')
    ids = [feats['a'][0], feats['c'], feats['b']]
    offs = np.cumsum([0] + dims)
    hand(emit(ids, [g[:, offs[c]:offs[c + 1]].contiguous() for c in range(3)], [sp, None, None]), 0.05, 'adagrad')
    for c in range(3):
      same(layer.weights[c], t8[c], f'layer step {step} table {c}')
      same(layer.accums[c], acc[c], f'layer step {step} accum {c}')
  path = str(tmp_path / 'ckpt')
  layer.save(path)
  saved = [host(w) for w in layer.weights]
  for w in layer.weights:
    w.zero_()
  layer.restore(path)
  for w, s in zip(layer.weights, saved):
    assert w.dtype == torch.uint8
    same(w, s, 'restore')
