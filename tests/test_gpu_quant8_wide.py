"""8-bit tables, lanes of 8 and 16 codes (hbk_quant8_lookup_fwd_wide) on the GPU: bit for bit GroupLookup over the
dequantised tables, followed by the cast for 16-bit outputs -- at the smallest dims at which each lane geometry can go
wrong, both forms of the code load, views off the wide boundary, column blocks of a wider tensor."""
import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd.embedding import GroupLookup, Quant8GroupLookup, Quant8Rows, dequantize_rows8, quantize_rows8

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROWS = 257
OUTS = (torch.float32, torch.bfloat16, torch.float16)
# (lane_codes, dim): one lane per row, three live lanes of four, a full group, the most lanes a row takes
GEOMETRY = [(8, 8), (8, 24), (8, 64), (8, 256), (16, 16), (16, 48), (16, 64), (16, 256)]
# the code load: L / 4 loads of 4 bytes (the default pitch; also a view whose base is 4 mod 8) or one L-byte load (a
# pitch rounded up to 16; also a view that starts at row 1)
LAYOUTS = ('default', 'default_view', 'pitch16', 'pitch16_view')
_TABLES = {}


def table_of(dim, layout):
  """(the 8-bit table, its dequantised rows) of a dim and layout, made once."""
  key = (dim, layout.split('_')[0])
  if key not in _TABLES:
    gen = torch.Generator(device=DEV).manual_seed(dim)
    rows = torch.randn(ROWS + 1, dim, device=DEV, generator=gen)
    rows[3] = 0.0   # a zero row (scale 0)
    t8 = quantize_rows8([rows], pitch=Quant8Rows.pitch_for(dim, 16 if key[1] == 'pitch16' else 4))[0]
    _TABLES[key] = (t8, dequantize_rows8([t8], [dim])[0])
  t8, deq = _TABLES[key]
  first = 1 if layout.endswith('_view') else 0
  view = t8[first:first + ROWS]
  if layout == 'default_view' and dim % 8 == 0:
    assert view.data_ptr() % 8 == 4
  if layout.startswith('pitch16'):
    assert view.data_ptr() % 16 == 0 and view.shape[1] % 16 == 0
  return view, deq[first:first + ROWS].contiguous()


def bits(t):
  return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check(lane_codes, dim, layout, out_dtype, ids, splits, weights, combiner, bucket):
  """One column into a block of a wider, prefilled tensor: the width it reports, its bits, its neighbours."""
  t8, deq = table_of(dim, layout)
  want = GroupLookup([deq], [bucket], combiner)([ids], [splits], sp_weights=weights)[0].to(out_dtype)
  pad = 16 // want.element_size()
  block = torch.full((want.shape[0], dim + 2 * pad), 7.0, device=DEV, dtype=out_dtype)
  look = Quant8GroupLookup([t8], [dim], [bucket], combiner, out_dtype=out_dtype, lane_codes=lane_codes)
  look([ids], [splits], [block[:, pad:pad + dim]], sp_weights=weights)
  assert look.lane_codes_used == [lane_codes]
  what = f'{combiner} weighted={weights is not None} ids={ids.dtype}'
  assert torch.equal(bits(block[:, pad:pad + dim]), bits(want)), what
  assert (block[:, :pad] == 7.0).all() and (block[:, pad + dim:] == 7.0).all(), what


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('out_dtype', OUTS, ids=str)
@pytest.mark.parametrize('lane_codes, dim', GEOMETRY)
def test_one_id_per_segment(lane_codes, dim, out_dtype, layout):
  n = 2048 + 3   # no multiple of the rows of a wave instruction, more than one block at 64 rows per instruction
  rng = np.random.RandomState(dim)
  for idt, combiner, weighted, bucket in ((np.int32, 'sum', False, 0), (np.int64, 'sum', False, ROWS + 9),
                                          (np.int64, 'sum', True, 0), (np.int32, 'mean', True, ROWS + 9),
                                          (np.int64, 'sqrtn', True, 0)):
    ids = rng.randint(0, ROWS, size=n) if bucket == 0 else rng.randint(0, 1 << 30, size=n)
    ids[[1, n // 2, n - 1]] = (-1, ROWS + 5, ROWS)   # outside the table (bucketed: ROWS .. ROWS + 8 are)
    ids[2] = 3                                       # the zero row
    w = None
    if weighted:
      w = rng.uniform(-1, 2, size=n).astype(np.float32)
      w[[5, 64, n - 2]] = 0.0   # zero divisors under mean and sqrtn
      w = [torch.from_numpy(w).to(DEV)]
    check(lane_codes, dim, layout, out_dtype, torch.from_numpy(ids.astype(idt)).to(DEV), None, w, combiner, bucket)


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('out_dtype', OUTS, ids=str)
@pytest.mark.parametrize('lane_codes, dim', GEOMETRY)
def test_ragged(lane_codes, dim, out_dtype, layout):
  lpr = 1 << int(np.ceil(np.log2(dim // lane_codes)))
  lens = np.tile([0, 1, lpr, lpr + 1, 3 * lpr + 1, 40, 7, 9], 130)   # 1040 segments: more than one block
  splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  n = int(splits[-1])
  rng = np.random.RandomState(dim + 1)
  ids = rng.randint(0, ROWS, size=n)
  ids[splits[5] + 2] = -1             # an invalid id inside a segment of 40
  ids[splits[12] + 1] = ROWS + 5      # and inside one of 3 * lpr + 1
  w = rng.uniform(-1, 2, size=n).astype(np.float32)
  w[splits[13]:splits[14]] = 0.0      # a segment of 40 whose divisor is zero
  w[splits[2]] = 0.0                  # a zero weight at the head of a segment
  ids_d, splits_d, w_d = (torch.from_numpy(x).to(DEV) for x in (ids, splits, w))
  for combiner in ('sum', 'mean', 'sqrtn'):
    for weights in (None, [w_d]):
      check(lane_codes, dim, layout, out_dtype, ids_d, splits_d, weights, combiner, 0)


def test_columns_that_cannot_take_the_width_fall_back_and_replays_repeat_the_call():
  dims = (64, 20, 16, 24)
  tables = [table_of(d, 'default') for d in dims]
  n = 300
  rng = np.random.RandomState(7)
  splits = [None, None, None, torch.from_numpy(np.arange(0, 3 * n + 1, 3).astype(np.int32)).to(DEV)]
  ids = [torch.from_numpy(rng.randint(0, ROWS, size=n if s is None else 3 * n)).to(DEV) for s in splits]
  want = GroupLookup([t[1] for t in tables], combiners='mean')(ids, splits)
  block = torch.full((n, 160), 7.0, device=DEV)
  # dim 20 is no multiple of 8; the dim-16 block starts one element off its 16-byte boundary
  offsets = (0, 64, 89, 108)
  views = [block[:, o:o + d] for o, d in zip(offsets, dims)]
  look = Quant8GroupLookup([t[0] for t in tables], dims, combiners='mean', lane_codes=8)
  look(ids, splits, views)
  assert look.lane_codes_used == [8, 4, 1, 8]
  expect = torch.full_like(block, 7.0)
  for o, d, w in zip(offsets, dims, want):
    expect[:, o:o + d] = w
  assert torch.equal(bits(block), bits(expect))
  block.fill_(7.0)
  look.launch()
  assert torch.equal(bits(block), bits(expect)), 'launch()'
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      look.launch()
  for replay in range(3):
    block.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(block), bits(expect)), f'graph replay {replay}'
  # 'auto' splits the call by the width its rule names per column (here: the narrow forward, and 8 codes for the
  # dim-16 column, whose block then cannot take them)
  auto = Quant8GroupLookup([t[0] for t in tables], dims, combiners='mean', lane_codes='auto')
  block.fill_(7.0)
  auto(ids, splits, views)
  assert auto.lane_codes_used == [4, 4, 1, 4] and torch.equal(bits(block), bits(expect)), "'auto'"


def test_layer_passes_table_lane_codes_through():
  fc = hb.feature_column
  # (128 elements wide: every block's stride is a multiple of 16 bytes; the dim-20 blocks cannot take 8 codes)
  cols = [fc.EmbeddingColumn('a', ROWS, 64, combiner='mean'), fc.EmbeddingColumn('b', ROWS, 24, combiner='sum'),
          fc.EmbeddingColumn('c', ROWS, 20, combiner='sum'), fc.EmbeddingColumn('d', ROWS, 20, combiner='sqrtn')]
  init = lambda col, rows, device: torch.randn(   # noqa: E731
    rows, col.dimension, device=device, generator=torch.Generator(DEV).manual_seed(col.dimension))
  rng = np.random.RandomState(3)
  sp = torch.from_numpy(np.concatenate([[0], np.cumsum(rng.randint(0, 12, size=96))]).astype(np.int32)).to(DEV)
  feats = {'a': (torch.from_numpy(rng.randint(0, 1 << 40, size=int(sp[-1]))).to(DEV), sp),
           'b': torch.from_numpy(rng.randint(0, 1 << 40, size=96)).to(DEV),
           'c': torch.from_numpy(rng.randint(0, 1 << 40, size=96)).to(DEV),
           'd': torch.from_numpy(rng.randint(0, 1 << 40, size=96)).to(DEV)}
  outs = []
  for lane_codes in (None, 8):
    layer = fc.DenseFeatures(cols, DEV, init=init, train=False, table_dtype='int8', table_lane_codes=lane_codes,
                             output_dtype=torch.bfloat16)
    outs.append(layer(feats).clone())
    assert layer._lookup.lane_codes == lane_codes   # pylint: disable=protected-access
  assert outs[0].dtype == torch.bfloat16 and torch.equal(bits(outs[0]), bits(outs[1]))
  assert sorted(layer._lookup.lane_codes_used) == [4, 4, 8, 8]   # pylint: disable=protected-access
