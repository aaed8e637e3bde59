"""Sequence lookups over bf16 / fp16 / int8 tables (hbk_sequence_lookup_fwd_lowbit) against plain torch: per position
``deq[row]`` with ``deq = table.float()`` or ``dequantize_rows8``, zeros where nothing is looked up, one cast to the
output dtype.  A lookup sums nothing, so every comparison is bit for bit.  Then the backward and the step over the grid
the forward left, and the layer."""
import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd.embedding import (LowbitSequenceLookup, LowbitSequenceLookupGrad, LowpSparseApply,
                                         Quant8Rows, Quant8SparseApply, RowwiseAdagrad, SequenceLookup,
                                         SequenceLookupGrad, dequantize_rows8, quantize_rows8, sequence_row_grid)

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ROWS = 37
B = 411            # 2055 positions at T = 5: no multiple of a wave's slots, several blocks at 64 rows per instruction
FORMATS = ('bf16', 'fp16', 'int8')
OUTS = (torch.float32, torch.bfloat16, torch.float16)
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
# pad id, ids dtype, bucket, divisor, ragged
CONFIGS = {
  'nopad-int64-rows-div1': (None, torch.int64, 0, 1, True),
  'pad-int32-rows-div2': (3, torch.int32, 0, 2, True),
  'nopad-int32-bucket-div2': (None, torch.int32, ROWS + 9, 2, True),
  'pad-int64-bucket-div1': (3, torch.int64, ROWS + 9, 1, True),     # buckets past the table read zero rows
  'one-id-per-sample': (None, torch.int64, 0, 1, False),
}


def same(got, want, what=''):
  assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
  bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
  assert torch.equal(got.contiguous().view(bits), want.contiguous().view(bits)), what


def make_table(fmt, dim, rows=ROWS, pitch=None):
  """(table, its dequantised fp32 [rows, dim])"""
  src = torch.from_numpy(np.random.RandomState(dim).standard_normal((rows, dim)).astype(np.float32)).to(DEV)
  if fmt == 'int8':
    t = quantize_rows8([src], pitch=pitch)[0]
    return t, dequantize_rows8([t], [dim])[0]
  t = src.to(DTYPES[fmt])
  return t, t.float()


def make_ids(rng, n, dtype, bucket, divisor, rows=ROWS):
  if bucket:
    lim = 2 ** 30 if dtype == torch.int32 else 2 ** 40
    ids = rng.randint(-lim, lim, size=n)
  else:
    ids = rng.randint(0, rows * divisor, size=n)
    plant = rng.randint(0, n, size=max(n // 8, 1))
    ids[plant] = rng.choice([-1, rows * divisor, rows * divisor + 5], size=plant.size)
  return torch.from_numpy(ids).to(DEV).to(dtype)


def ragged(rng, T):
  """lengths 0 .. 2T: empty samples, truncated ones, samples that cross a wave's boundary"""
  return torch.from_numpy(np.concatenate([[0], np.cumsum(rng.randint(0, 2 * T + 1, size=B))]).astype(np.int32)).to(DEV)


def reference(deq, ids, splits, T, bucket, divisor, pad_id, out_dtype):
  """(rows [B, T, dim] of out_dtype, grid int64 [B * T], lengths int32 [B]) in plain torch"""
  n, rows = ids.numel(), deq.shape[0]
  if splits is None:
    splits = torch.arange(n + 1, device=DEV, dtype=torch.int32)
  beg = splits[:-1].long()
  lens = (splits[1:].long() - beg).clamp(0, T)
  t = torch.arange(T, device=DEV)
  valid = t[None, :] < lens[:, None]
  raw = ids.long()[(beg[:, None] + t[None, :]).clamp(0, n - 1)]
  raw = torch.where(valid, raw, torch.full_like(raw, -1 if pad_id is None else pad_id))
  has = valid if pad_id is None else torch.ones_like(valid)
  if bucket:
    g = torch.remainder(raw, bucket)
  else:
    g, has = raw, has & (raw >= 0)
  grid = torch.where(has, g, torch.full_like(g, -1))
  row = torch.div(grid, divisor, rounding_mode='floor')
  looked = (grid >= 0) & (row < rows)
  out = torch.where(looked[..., None], deq[row.clamp(0, rows - 1)], torch.zeros((), device=DEV))
  return out.to(out_dtype), grid.reshape(-1), lens.int()


@pytest.mark.parametrize('config', CONFIGS)
@pytest.mark.parametrize('T', (1, 5))
@pytest.mark.parametrize('out_dtype', OUTS, ids=str)
@pytest.mark.parametrize('fmt', FORMATS)
def test_forward_equals_the_dequantised_rows(fmt, out_dtype, T, config):
  pad, idt, bucket, div, is_ragged = CONFIGS[config]
  rng = np.random.RandomState(17 * T + len(config))
  wide = 4 if out_dtype == torch.float32 else 8
  dims = [wide, 3 * wide, 64, 256, 1, 3, 7, 63]   # lanes of `wide` elements, then one element per lane
  n = len(dims)
  tabs = [make_table(fmt, d) for d in dims]
  splits = ragged(rng, T) if is_ragged else None
  ids = make_ids(rng, int(splits[-1]) if is_ragged else B, idt, bucket, div)
  look = LowbitSequenceLookup([t for t, _ in tabs], dims if fmt == 'int8' else None, [bucket] * n, T, pad, div,
                              out_dtype)
  outs, lengths = look([ids] * n, [splits] * n if is_ragged else None)
  assert look.lane_elems_used == [wide] * 4 + [1] * 4
  grid_op = sequence_row_grid([ids], [splits] if is_ragged else None, [bucket], T, pad)[0][0]
  for c, (_, deq) in enumerate(tabs):
    want, grid, lens = reference(deq, ids, splits, T, bucket, div, pad, out_dtype)
    same(outs[c], want, f'rows, dim {dims[c]}')
    same(look.grids[c], grid, f'grid, dim {dims[c]}')
    same(look.grids[c], grid_op, 'sequence_row_grid')
    same(lengths[c], lens, 'lengths')


@pytest.mark.parametrize('out_dtype', OUTS, ids=str)
@pytest.mark.parametrize('fmt', FORMATS)
def test_layouts_blocks_inference_and_launch(fmt, out_dtype):
  T, rng = 5, np.random.RandomState(3)
  o16 = out_dtype != torch.float32
  if fmt == 'int8':
    src = torch.from_numpy(rng.standard_normal((ROWS + 1, 8)).astype(np.float32)).to(DEV)
    src[2] = 0                                                       # a zero row: scale 0
    a = quantize_rows8([src])[0]                                     # pitch 12: two 4-byte code loads at W = 8
    b = quantize_rows8([src], pitch=Quant8Rows.pitch_for(8, 16))[0]  # pitch 16: one 8-byte load
    tables, dims = [a[:ROWS], b[:ROWS], a[1:]], [8, 8, 8]            # a[1:]: a view from row 1, base 4 mod 8
    deqs = dequantize_rows8(tables, dims)
    lanes = [8 if o16 else 4] * 3
  else:
    a = torch.from_numpy(rng.standard_normal((ROWS + 1, 12)).astype(np.float32)).to(DEV).to(DTYPES[fmt])[1:]
    flat = torch.from_numpy(rng.standard_normal(ROWS * 8 + 4).astype(np.float32)).to(DEV).to(DTYPES[fmt])
    tables, dims = [a, flat[4:].view(ROWS, 8)], [12, 8]   # base 24 (off 16): W = 4; rows on 8 bytes: two 8-byte loads
    deqs = [t.float() for t in tables]
    lanes = [4, 8 if o16 else 4]
  n = len(tables)
  splits = ragged(rng, T)
  ids = make_ids(rng, int(splits[-1]), torch.int64, 0, 1)
  look = LowbitSequenceLookup(tables, dims if fmt == 'int8' else None, None, T, None, 1, out_dtype)
  wants = [reference(q, ids, splits, T, 0, 1, None, out_dtype)[0] for q in deqs]
  # blocks of a wider prefilled tensor: on the store's boundary, then one element off it (one element per lane)
  for off, lanes_want in ((8, lanes), (1, [1] * n)):
    wides = [torch.full((B, T * d + 16), 7.0, dtype=out_dtype, device=DEV) for d in dims]
    outs = [w[:, off:off + T * d].unflatten(1, (T, d)) for w, d in zip(wides, dims)]
    got, _ = look([ids] * n, [splits] * n, outs=outs, grids=False)
    assert look.lane_elems_used == lanes_want and look.grids is None
    for w, o, want, d in zip(wides, got, wants, dims):
      same(o, want, f'block at {off}, dim {d}')
      assert bool((w[:, :off] == 7).all()) and bool((w[:, off + T * d:] == 7).all()), 'neighbours'
  # launch() after refilling the ids in place
  ids.copy_(make_ids(rng, ids.numel(), torch.int64, 0, 1))
  look.launch()
  for o, q in zip(got, deqs):
    same(o, reference(q, ids, splits, T, 0, 1, None, out_dtype)[0], 'launch')


STEPS = [(f, o, r) for f in FORMATS for o in ('sgd', 'rowwise_adagrad') for r in ('nearest', 'stochastic')
         if (f, r) != ('fp16', 'stochastic')]   # (stochastic rounding is defined for bf16 and int8 tables)


@pytest.mark.parametrize('fmt, optimizer, rounding', STEPS)
def test_backward_and_step_equal_the_fp32_reduce_then_the_apply(fmt, optimizer, rounding):
  T, rows, dims, rng = 5, 4096, [16, 6], np.random.RandomState(9)
  tabs = [make_table(fmt, d, rows=rows) for d in dims]
  tables, deqs = [t for t, _ in tabs], [q for _, q in tabs]
  before, twins = [t.clone() for t in tables], [t.clone() for t in tables]

  def slots():
    if optimizer != 'rowwise_adagrad':
      return {}
    return dict(row_accums=[torch.full((rows, 1), 0.1, device=DEV) for _ in dims], rowwise_adagrad=RowwiseAdagrad())
  mine, theirs = slots(), slots()
  look = LowbitSequenceLookup(tables, dims if fmt == 'int8' else None, None, T)
  grad = LowbitSequenceLookupGrad(look, deterministic=True, rounding=rounding, seed=5, **mine)
  ref_look = SequenceLookup(deqs, None, T)
  if fmt == 'int8':
    hand = Quant8SparseApply(twins, dims, rounding=rounding, seed=5, **theirs)
  else:
    hand = LowpSparseApply(twins, rounding=rounding, seed=5, **theirs)
  splits = ragged(rng, T)
  ids = [make_ids(rng, int(splits[-1]), torch.int64, 0, 1, rows=rows) for _ in dims]
  look(ids, [splits] * 2)
  ref_look(ids, [splits] * 2)
  gs = [torch.from_numpy(rng.standard_normal((B, T, d)).astype(np.float32)).to(DEV) for d in dims]
  got = grad(gs, apply_lr=0.1, optimizer=optimizer)
  want = SequenceLookupGrad(ref_look)(gs, deterministic=True)
  hand(want, 0.1, optimizer)
  assert int(grad.step_counter.item()) == int(hand.step_counter.item()) == (1 if rounding == 'stochastic' else 0)
  for c in range(len(dims)):
    k = int(want[c][2].item())
    assert int(got[c][2].item()) == k
    same(got[c][0][:k], want[c][0][:k], 'unique_rows')
    same(got[c][1][:k], want[c][1][:k], 'grad_rows')
    same(tables[c], twins[c], 'stepped table')
    if mine:
      same(mine['row_accums'][c], theirs['row_accums'][c], 'slots')
    # padding without a pad id reaches no row: the rows the grid does not name keep their bits
    g = look.grids[c]
    named = torch.zeros(rows, dtype=torch.bool, device=DEV)
    named[g[(g >= 0) & (g < rows)]] = True   # (a grid word is the id: the planted ids past the table are in it)
    assert bool((g == -1).any()) and not bool(named.all()) and not torch.equal(tables[c], before[c])
    same(tables[c][~named], before[c][~named], 'rows outside the grid')


@pytest.mark.parametrize('table_dtype, output_dtype', (('int8', torch.bfloat16), (torch.bfloat16, None),
                                                      (torch.float16, torch.float16)), ids=str)
def test_layer(table_dtype, output_dtype, tmp_path):
  fc = hb.feature_column
  cols = [fc.SequenceEmbeddingColumn('a', ROWS, 16, max_len=5), fc.SequenceEmbeddingColumn('b', ROWS, 6, max_len=3, pad_id=2)]
  layer = fc.SequenceFeatures(cols, DEV, table_dtype=table_dtype, output_dtype=output_dtype)
  rng = np.random.RandomState(1)
  splits = ragged(rng, 5)
  ids = make_ids(rng, int(splits[-1]), torch.int64, ROWS, 1)
  outs, lengths = layer({'a': (ids, splits), 'b': (ids, splits)})
  look = LowbitSequenceLookup(layer.weights, [16, 6] if table_dtype == 'int8' else None, [ROWS, ROWS], [5, 3],
                              [None, 2], out_dtype=output_dtype or torch.float32)
  want, want_len = look([ids] * 2, [splits] * 2)
  for c in range(2):
    assert outs[c].dtype == (output_dtype or torch.float32)
    same(outs[c], want[c], 'layer forward')
    same(lengths[c], want_len[c], 'layer lengths')
  start = [w.clone() for w in layer.weights]
  layer.backward([torch.ones(o.shape, device=DEV) for o in outs], apply_lr=0.5)
  assert not any(torch.equal(w, s) for w, s in zip(layer.weights, start))
  path = str(tmp_path / 'ckpt')
  layer.save(path)
  saved = [w.clone() for w in layer.weights]
  for w in layer.weights:
    w.zero_()
  layer.restore(path)
  for w, s in zip(layer.weights, saved):
    assert w.dtype == s.dtype
    same(w, s, 'restore')
