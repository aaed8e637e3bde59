"""16-bit outputs on the GPU.  The oracle is always the existing fp32-output lookup over ``[t.float() for t in tables]``
with the same arguments followed by torch's ``.to(out_dtype)``, compared as bit patterns."""
import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd.embedding import GroupLookup, Out16GroupLookup, SequenceLookup
from tests.support import exact
from tests.test_gpu_lowp_tables import (BF, DIMS, F32, HF, ROWS, bits16, dev, host, layer_init, ragged, some_ids,
                                        sorted_slices, special_table)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
fc = hb.feature_column
KINDS = {'fp32': (F32,), 'bf16': (BF,), 'fp16': (HF,), 'mixed': (F32, BF, HF)}


def make_tables(rng, kind, dims, rows=ROWS):
  """fp32 tables carry full fp32 fractions (so the output rounding rounds), 16-bit tables their special patterns."""
  kinds = [KINDS[kind][c % len(KINDS[kind])] for c in range(len(dims))]
  return [dev(rng.uniform(-2, 2, size=(rows, d)).astype(F32)) if k is F32 else special_table(rng, rows, d, k)
          for d, k in zip(dims, kinds)]


def same16(got, want, what=''):
  g, w = bits16(got), bits16(want)
  assert g.shape == w.shape, (what, g.shape, w.shape)
  bad = g != w
  assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}'


def check(tables, ids, out_dtype, splits=None, weights=None, combiners='sum', buckets=None, divisor=1, chunk=None,
          what=''):
  new = Out16GroupLookup(tables, buckets, combiners, divisor, out_dtype=out_dtype, chunk_elems=chunk)
  old = GroupLookup([t.float() for t in tables], buckets, combiners, divisor)
  a = new(ids, splits, sp_weights=weights)
  b = old(ids, splits, sp_weights=weights)
  for c, (x, y) in enumerate(zip(a, b)):
    assert x.dtype == out_dtype
    same16(x, y.to(out_dtype), f'{what} column {c} dim {tables[c].shape[1]}')


@pytest.mark.parametrize('id_dtype', [np.int32, np.int64])
@pytest.mark.parametrize('chunk', [None, 4, 8])
@pytest.mark.parametrize('out_dtype', [BF, HF])
@pytest.mark.parametrize('kind', list(KINDS))
def test_one_id_per_segment(kind, out_dtype, chunk, id_dtype):
  rng = np.random.RandomState(1)
  tables = make_tables(rng, kind, DIMS)
  for n in (1, 257):
    check(tables, [some_ids(rng, n, ROWS, id_dtype) for _ in DIMS], out_dtype, chunk=chunk, what=f'n={n}')
  # floor-mod buckets with negative ids and divisor 3: rows 37 < ceil(113 / 3), some ids land past the table
  ids = [dev(rng.randint(-1000, 1000, size=70).astype(id_dtype)) for _ in DIMS]
  check(tables, ids, out_dtype, buckets=[113] * len(DIMS), divisor=3, chunk=chunk, what='bucket')


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('combiner', ['sum', 'mean', 'sqrtn'])
@pytest.mark.parametrize('chunk', [None, 4, 8])
@pytest.mark.parametrize('out_dtype', [BF, HF])
@pytest.mark.parametrize('kind', list(KINDS))
def test_ragged(kind, out_dtype, chunk, combiner, weighted):
  rng = np.random.RandomState(2)
  tables = make_tables(rng, kind, DIMS)
  splits = [dev(ragged(rng, 70)) for _ in DIMS]
  ids = [some_ids(rng, int(s[-1]), ROWS, (np.int32, np.int64)[c % 2]) for c, s in enumerate(splits)]
  weights = None
  if weighted:
    weights = []
    for s in splits:
      w = rng.choice([-1.0, 0.25, 0.5, 1.0, 3.0], size=int(s[-1])).astype(F32)
      sp = host(s)
      k = int(np.argmax(np.diff(sp) == 2))     # a zero-divisor segment: weights that cancel (mean), all zero
      if np.diff(sp)[k] == 2:
        w[sp[k]:sp[k + 1]] = (1.0, -1.0) if combiner == 'mean' else (0.0, 0.0)
      weights.append(dev(w))
  check(tables, ids, out_dtype, splits, weights, combiner, chunk=chunk, what=combiner)


def test_rounding_edges():
  """fp32 table, one id per segment: f[s] is the table value itself, so the oracle alone decides every bit."""
  u32 = lambda *p: np.array(p, np.uint32).view(F32)   # noqa: E731
  bf = u32(0x3F808000, 0x3F818000,        # exact ties, even and odd neighbour below
           0x3F807FFF, 0x3F808001,        # either side of a tie
           0x7F7F0000, 0x3FFFFFFF,        # the largest finite bf16; rounds up into the next binade
           0x7F7F7FFF)                    # the largest fp32 that stays finite in bf16
  hf = u32(0x3F801000, 0x3F803000,        # exact ties (fp16 keeps 10 fraction bits: bit 12 is the half)
           0x3F800FFF, 0x3F801001,
           0x477FE000, 0x3FFFF000,        # 65504, the largest finite fp16; rounds up into the next binade
           0x477FEFFF,                    # just below the tie at the top: stays 65504
           0x477FF000, 0x47800000, 0x7F7FFFFF,   # the tie at the top, 65536 and the largest fp32: +-inf
           0x33000000, 0x33000001,        # 2^-25: ties to zero; the smallest value that does not round to zero
           0x33800000, 0x387FC000, 0x38000000, 0x387FFFFF)   # subnormals: the smallest, the largest, a middle, just below normal
  for vals, out_dtype in ((bf, BF), (np.concatenate([bf, hf]), HF)):
    vals = np.concatenate([vals, -vals])
    n = (vals.size + 7) // 8 * 8
    table = dev(np.concatenate([vals, np.zeros(n - vals.size, F32)]).reshape(-1, 8))
    ids = [dev(np.arange(table.shape[0], dtype=np.int64))]
    check([table], ids, out_dtype, what=str(out_dtype))
    check([table.view(-1, 1)], [dev(np.arange(n, dtype=np.int64))], out_dtype, what=f'{out_dtype} one element per lane')


@pytest.mark.parametrize('out_dtype', [BF, HF])
def test_blocks_of_a_wider_tensor_keep_what_lies_between(out_dtype):
  rng = np.random.RandomState(4)
  dims, offsets, width = (3, 5, 16, 64), (1, 7, 20, 40), 112     # lane widths 1, 1, 4 (8-byte aligned only), 8
  tables = make_tables(rng, 'mixed', dims)
  splits = [None, dev(ragged(rng, 70)), None, dev(ragged(rng, 70))]
  ids = [some_ids(rng, 70 if s is None else int(s[-1]), ROWS) for s in splits]
  wide16 = torch.full((70, width), -7.0, dtype=out_dtype, device=DEV)
  wide32 = torch.full((70, width), -7.0, dtype=torch.float32, device=DEV)
  new = Out16GroupLookup(tables, combiners='mean', out_dtype=out_dtype)
  assert new.bind_block(ids, splits, wide16, list(offsets))
  new.launch()
  GroupLookup([t.float() for t in tables], combiners='mean')(
    ids, splits, [wide32[:, o:o + d] for o, d in zip(offsets, dims)])
  same16(wide16, wide32.to(out_dtype), 'the whole wide tensor')


def test_launch_and_graph_replay_after_new_ids():
  rng = np.random.RandomState(5)
  dims = (3, 16, 128)
  tables = make_tables(rng, 'mixed', dims)
  splits = [None, dev(ragged(rng, 64, longest=30)), None]
  ids = [some_ids(rng, 64 if s is None else int(s[-1]), ROWS) for s in splits]
  new = Out16GroupLookup(tables, combiners='mean', out_dtype=BF)
  old = GroupLookup([t.float() for t in tables], combiners='mean')
  outs = [torch.zeros(64, d, dtype=BF, device=DEV) for d in dims]
  new(ids, splits, outs)
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      new.launch()
  torch.cuda.synchronize()
  for again in (new.launch, graph.replay, graph.replay):
    for i in ids:
      i.copy_(some_ids(rng, i.numel(), ROWS))
    for o in outs:
      o.fill_(-1.0)
    again()
    torch.cuda.synchronize()
    for x, y in zip(outs, old(ids, splits)):
      same16(x, y.to(BF), again.__name__)


# ---- the layer ---------------------------------------------------------------------------------------------------
def layer_columns():
  return [fc.EmbeddingColumn('a', 50, 8, combiner='sum'),
          fc.EmbeddingColumn('bb', 60, 16, combiner='sum', weight_feature_key='bb_w'),
          fc.EmbeddingColumn('ccc', 70, 3, combiner='sum'), fc.EmbeddingColumn('dddd', 40, 64, combiner='sum')]


@pytest.mark.parametrize('table_dtype', [None, BF])
def test_layer_block_and_sgd_step_equal_the_fp32_output_layer(table_dtype):
  rng = np.random.RandomState(6)
  kw = dict(init=layer_init, table_dtype=table_dtype)
  new = fc.DenseFeatures(layer_columns(), DEV, output_dtype=BF, **kw)
  old = fc.DenseFeatures(layer_columns(), DEV, **kw)
  batch = 70
  f = {c.key: dev(rng.randint(-20, 200, size=batch).astype(np.int64)) for c in layer_columns()}
  sp = exact.exact_ragged(rng, batch, 'sum', 5)                 # 'bb': ragged and weighted
  f['bb'] = (dev(rng.randint(-20, 200, size=int(sp[-1])).astype(np.int64)), dev(sp))
  f['bb_w'] = dev(exact.exact_weights(rng, sp, int(sp[-1]), 'sum').astype(F32))
  out = new(f)
  assert out.dtype == BF and out.stride(0) == 96 and out.data_ptr() % 16 == 0
  same16(out, old(f).to(BF), 'block')
  grad = dev(exact.exact_grads(rng, tuple(out.shape), 5)).to(BF)     # (8 significant bits: bf16 holds them)
  a = new.backward(grad, apply_lr=0.25)
  b = old.backward(grad.float(), apply_lr=0.25)
  torch.cuda.synchronize()
  for c, ((ua, ga), (ub, gb)) in enumerate(zip(sorted_slices(a), sorted_slices(b))):
    np.testing.assert_array_equal(ua, ub, f'unique_rows {c}')
    exact.assert_bits_equal(ga, gb, f'grad_rows {c}')
  for c, (x, y) in enumerate(zip(new.weights, old.weights)):
    assert x.dtype == y.dtype
    assert torch.equal(x.view(torch.int16), y.view(torch.int16)), f'table {c}'


# ---- sequences ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad_id', [None, 3])
def test_sequence_outputs_lengths_and_grid(pad_id):
  rng = np.random.RandomState(7)
  dims, max_lens = (8, 20, 3), (4, 6, 1)
  tables = make_tables(rng, 'fp32', dims)
  lens = rng.choice([0, 1, 3, 4, 5, 9], size=33)                # shorter and longer than every T
  splits = [dev(exact.splits_of(lens)) for _ in dims]
  ids = [some_ids(rng, int(lens.sum()), ROWS) for _ in dims]
  kw = dict(buckets=None, max_lens=list(max_lens), pad_ids=pad_id)
  new, old = SequenceLookup(tables, out_dtype=HF, **kw), SequenceLookup(tables, **kw)
  (oa, la), (ob, lb) = new(ids, splits), old(ids, splits)
  for c in range(len(dims)):
    assert oa[c].dtype == HF and tuple(oa[c].shape) == (33, max_lens[c], dims[c])
    same16(oa[c], ob[c].to(HF), f'outputs {c}')
    assert torch.equal(la[c], lb[c]) and torch.equal(new.grids[c], old.grids[c])
