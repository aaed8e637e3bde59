"""Key-deduplicated features on the GPU, the kernels: hbk_expand_rows_n, hbk_expand_index_build and
hbk_expand_rows_grad_n against their numpy restatement (tests/support/expand_ref.py), bit for bit -- the backward
against a literal fp32 loop in ascending sample order on N(0,1) gradients.  Widths across the lane-group sizes and
the wave tile, batch sizes around the workgroup's rows, every index pattern, indices outside [0, n_keys) (inputs
the kernels are specified to survive: compared with the range before any address is formed), column blocks of a
wider tensor between canary columns, more columns than one launch holds, a rerun and a captured graph."""
import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from tests.support import expand_ref as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
WIDTHS = [1, 3, 4, 16, 17, 64, 65, 256, 260, 416, 800]
SAMPLES = [0, 1, 63, 64, 65, 257]
CANARY = 0x7fc0dead          # a NaN's bits: a float compare would not see it change
LAYOUTS = [None, 0, 1, 4]    # contiguous, or a column block at this offset (floats) of a wider tensor


def _bits(x):
  return np.ascontiguousarray(x).view(np.uint32)


def _same_bits(got, want, what):
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
  bad = _bits(got) != _bits(want)
  assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0]}'


class Block:
  """``rows`` rows of ``width`` elements: contiguous, or a column block of a wider tensor whose other columns
  hold the canary."""

  def __init__(self, rows, width, layout, data=None, dtype=torch.float32):
    self.left = 0 if layout is None else layout
    total = width if layout is None else self.left + width + 3
    self.wide = torch.full((rows, total), CANARY, dtype=torch.int32, device=DEV).view(dtype)
    self.view = self.wide[:, self.left:self.left + width]
    self.width = width
    if data is not None:
      self.view.copy_(torch.from_numpy(np.ascontiguousarray(data)).to(DEV))

  def numpy(self):
    wide = self.wide.cpu().numpy()
    mask = np.ones(wide.shape[1], bool)
    mask[self.left:self.left + self.width] = False
    assert (_bits(wide)[:, mask] == CANARY).all(), 'a canary column changed'
    return wide[:, self.left:self.left + self.width]


def _patterns(rng, n, n_keys, dtype):
  """name -> idx: sorted, reversed, random (a permutation when n_keys == n), all equal, and one with -1, n_keys
  and the largest value of the dtype's test set planted."""
  if n_keys == 0:
    base = np.zeros(n, np.int64)
  elif n_keys == n:
    base = rng.permutation(n).astype(np.int64)
  else:
    base = rng.randint(0, n_keys, size=n).astype(np.int64)
  out = {'sorted': np.sort(base), 'reversed': np.sort(base)[::-1].copy(), 'random': base,
         'equal': np.full(n, max(n_keys - 1, 0), np.int64)}
  bad = base.copy()
  far = 2 ** 40 if dtype == np.int64 else 2 ** 31 - 1
  for k, v in enumerate((-1, n_keys, far, -2 ** 31)):
    bad[k::7][:max(1, n // 11)] = v
  out['invalid'] = bad
  return {k: v.astype(dtype) for k, v in out.items()}


def _run(rng, widths, layouts, idx, n_keys, outs_given=True):
  """Forward, index and transpose of the columns ``widths`` (column c laid out by layouts[c]) through the Python
  entries, each compared with the restatement."""
  n = idx.size
  d_idx = torch.from_numpy(idx).to(DEV)
  srcs = [rng.randn(n_keys, w).astype(np.float32) for w in widths]
  grads = [rng.randn(n, w).astype(np.float32) for w in widths]
  s_blocks = [Block(n_keys, w, lay, s) for w, lay, s in zip(widths, layouts, srcs)]
  o_blocks = [Block(n, w, lay) for w, lay in zip(widths, layouts)]
  got = hb.embedding.expand_rows(d_idx, [b.view for b in s_blocks],
                                 [b.view for b in o_blocks] if outs_given else None, n_keys=n_keys)
  for c, w in enumerate(widths):
    have = o_blocks[c].numpy() if outs_given else got[c].cpu().numpy()
    _same_bits(have, ref.expand_ref(srcs[c], idx, n_keys), f'forward column {c} width {w}')
    s_blocks[c].numpy()    # (the sources' canaries)
  index = hb.embedding.ExpandIndex(d_idx, n_keys).build()
  order, splits, invalid = ref.index_ref(idx, n_keys)
  assert index.order.cpu().numpy().tolist() == order.tolist()
  assert index.splits.cpu().numpy().tolist() == splits.tolist()
  assert index.invalid_count() == invalid
  g_blocks = [Block(n, w, lay, g) for w, lay, g in zip(widths, layouts, grads)]
  r_blocks = [Block(n_keys, w, lay) for w, lay in zip(widths, layouts)]
  got = hb.embedding.expand_rows_grad(index, [b.view for b in g_blocks],
                                      [b.view for b in r_blocks] if outs_given else None)
  for c, w in enumerate(widths):
    have = r_blocks[c].numpy() if outs_given else got[c].cpu().numpy()
    _same_bits(have, ref.grad_ref(grads[c], idx, n_keys), f'transpose column {c} width {w}')
  return index, g_blocks, r_blocks


@pytest.mark.parametrize('width', WIDTHS)
def test_every_width_in_every_layout(width):
  rng = np.random.RandomState(width)
  for k, layout in enumerate(LAYOUTS):
    dtype = (np.int32, np.int64)[k % 2]
    idx = _patterns(rng, 257, 37, dtype)['invalid' if k < 2 else 'random']
    _run(rng, [width], [layout], idx, 37)
  # a source and an output laid out differently, and the outputs the entry allocates itself
  idx = _patterns(rng, 65, 65, np.int64)['random']
  _run(rng, [width, width], [1, None], idx, 65, outs_given=False)


@pytest.mark.parametrize('n', SAMPLES)
def test_every_batch_size_key_count_and_index_pattern(n):
  rng = np.random.RandomState(100 + n)
  for n_keys in sorted({0, 1, n, n + 9}):
    for k, dtype in enumerate((np.int32, np.int64)):
      for name, idx in _patterns(rng, n, n_keys, dtype).items():
        if (name in ('sorted', 'reversed')) and k == 1:
          continue      # (the order patterns once per key count)
        _run(rng, [3, 16], [1, None], idx, n_keys)


def test_one_key_owning_more_samples_than_a_wave_is_still_the_sequential_sum():
  rng = np.random.RandomState(5)
  idx = np.full(257, 2, np.int32)
  _run(rng, [1, 17, 416], [None, 4, 0], idx, 4)
  # and the chain is the order-dependent one: 1e8 + 1 - 1e8 is 0 in sample order, 1 if the big terms met first
  g = np.zeros((257, 4), np.float32)
  g[0], g[1], g[2] = 1e8, 1.0, -1e8
  index = hb.embedding.ExpandIndex(torch.from_numpy(idx).to(DEV), 4).build()
  got = hb.embedding.expand_rows_grad(index, [torch.from_numpy(g).to(DEV)])[0].cpu().numpy()
  _same_bits(got, ref.grad_ref(g, idx, 4), 'cancellation')
  assert got[2, 0] == 0.0
  # a lone -0 stays -0: the chain starts from its first term, not from 0
  g = np.full((3, 5), -0.0, np.float32)
  index = hb.embedding.ExpandIndex(torch.tensor([1, 0, 5], device=DEV), 3).build()
  got = hb.embedding.expand_rows_grad(index, [torch.from_numpy(g).to(DEV)])[0].cpu().numpy()
  assert np.signbit(got[:2]).all() and not np.signbit(got[2]).any()


@pytest.mark.parametrize('n_cols', [1, 3, 65])
def test_columns_per_launch(n_cols):
  rng = np.random.RandomState(n_cols)
  widths = [WIDTHS[c % 8] for c in range(n_cols)]
  layouts = [LAYOUTS[(c + c // 4) % 4] for c in range(n_cols)]
  _run(rng, widths, layouts, _patterns(rng, 65, 17, np.int64)['invalid'], 17)


def test_int32_rows_pass_through_bit_for_bit_and_the_identity_places_a_block():
  rng = np.random.RandomState(9)
  lengths = rng.randint(-2 ** 31, 2 ** 31 - 1, size=(37,)).astype(np.int32)    # any bits, NaN patterns among them
  lengths[:3] = (0x7fc00001, -1, 0)
  rows = rng.randn(37, 4, 5).astype(np.float32)
  idx = _patterns(rng, 150, 37, np.int64)['invalid']
  got = hb.embedding.expand_rows(torch.from_numpy(idx).to(DEV),
                                 [torch.from_numpy(rows).to(DEV), torch.from_numpy(lengths).to(DEV)])
  assert got[0].shape == (150, 4, 5) and got[1].shape == (150,) and got[1].dtype == torch.int32
  _same_bits(got[0].cpu().numpy(), ref.expand_ref(rows, idx, 37), 'rows [U, T, dim]')
  assert got[1].cpu().numpy().tolist() == ref.expand_ref(lengths, idx, 37).tolist()
  # idx=None: out[b] = src[b], into a column block
  for width, layout in ((416, 4), (13, 1), (64, None)):
    src = rng.randn(150, width).astype(np.float32)
    out = Block(150, width, layout)
    hb.embedding.expand_rows(None, [torch.from_numpy(src).to(DEV)], [out.view])
    _same_bits(out.numpy(), src, f'identity width {width}')


def test_python_refusals_on_the_device():
  e = hb.embedding
  idx = torch.zeros(3, dtype=torch.int64, device=DEV)
  src = torch.zeros(2, 4, device=DEV)
  with pytest.raises(hb.InvalidArgumentError, match='not built'):
    e.expand_rows_grad(e.ExpandIndex(idx, 2), [torch.zeros(3, 4, device=DEV)])
  with pytest.raises(hb.InvalidArgumentError, match='expected 1 outputs'):
    e.expand_rows(idx, [src], [])
  with pytest.raises(hb.InvalidArgumentError, match='output 0 must be a float32 tensor'):
    e.expand_rows(idx, [src], [torch.zeros(3, 5, device=DEV)])
  with pytest.raises(hb.InvalidArgumentError, match='float32 or int32'):
    e.expand_rows(idx, [src.half()])
  with pytest.raises(hb.InvalidArgumentError, match='same out'):
    out = torch.zeros(3, 4, device=DEV)
    e.expand_rows(idx, [src, src], [out, out])
  with pytest.raises(hb.InvalidArgumentError, match='2 rows, expected 5'):
    e.expand_rows(idx, [src], n_keys=5)
  with pytest.raises(hb.HbkError, match='HBM'):
    e.expand_rows(idx, [src.cpu()])


def test_the_transpose_gives_the_same_bits_on_every_run():
  rng = np.random.RandomState(11)
  idx = np.concatenate([np.full(200, 3), rng.randint(0, 37, size=57)]).astype(np.int64)
  rng.shuffle(idx)
  index = hb.embedding.ExpandIndex(torch.from_numpy(idx).to(DEV), 37).build()
  g = torch.from_numpy(rng.randn(257, 416).astype(np.float32)).to(DEV)
  first = hb.embedding.expand_rows_grad(index, [g])[0].cpu().numpy()
  again = hb.embedding.expand_rows_grad(index, [g])[0].cpu().numpy()
  _same_bits(first, again, 'rerun')
  other = hb.embedding.ExpandIndex(torch.from_numpy(idx).to(DEV), 37).build()
  assert torch.equal(other.order, index.order) and torch.equal(other.splits, index.splits)


def test_a_captured_graph_of_expand_and_reduce_replays_on_refilled_buffers():
  rng = np.random.RandomState(13)
  n, n_keys, widths = 257, 37, [17, 416]
  idx = _patterns(rng, n, n_keys, np.int64)['invalid']
  d_idx = torch.from_numpy(idx).to(DEV)
  index = hb.embedding.ExpandIndex(d_idx, n_keys).build()     # (built outside the capture)
  srcs = [torch.zeros(n_keys, w, device=DEV) for w in widths]
  grads = [torch.zeros(n, w, device=DEV) for w in widths]
  outs = [torch.empty(n, w, device=DEV) for w in widths]
  sums = [torch.empty(n_keys, w, device=DEV) for w in widths]
  side = torch.cuda.Stream(DEV)
  side.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(side):                                # (a first run outside the capture)
    hb.embedding.expand_rows(index, srcs, outs)
    hb.embedding.expand_rows_grad(index, grads, sums)
  torch.cuda.current_stream(DEV).wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    hb.embedding.expand_rows(index, srcs, outs)
    hb.embedding.expand_rows_grad(index, grads, sums)
  for _ in range(2):
    new_s = [rng.randn(n_keys, w).astype(np.float32) for w in widths]
    new_g = [rng.randn(n, w).astype(np.float32) for w in widths]
    for t, x in zip(srcs + grads, new_s + new_g):
      t.copy_(torch.from_numpy(x))                             # refilled in place
    graph.replay()
    torch.cuda.synchronize()
    for c in range(len(widths)):
      _same_bits(outs[c].cpu().numpy(), ref.expand_ref(new_s[c], idx, n_keys), f'replayed forward {c}')
      _same_bits(sums[c].cpu().numpy(), ref.grad_ref(new_g[c], idx, n_keys), f'replayed transpose {c}')
