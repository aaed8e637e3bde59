"""Sequence lookups on the GPU (hbk_group_lookup_fwd_sequence, hbk_sequence_row_grid_n, SequenceLookup,
SequenceLookupGrad): outputs, id grids and lengths bit-equal to the numpy restatement
(tests/support/sequence_ref.py) over the row shapes, lengths and id kinds where the kernel takes
different paths; strided outputs; the fused and the two-launch forms; max_norm; the backward over the
grid in its emit, deterministic and stepping forms; and a captured graph."""
import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (GroupLookup, GroupLookupGrad, SequenceLookup, SequenceLookupGrad,
                                         sequence_row_grid)
from tests.support import sequence_ref as ref
from tests.support.tolerance import assert_sums_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def _lens(rng, B, T):
  """Lengths 0, < T, == T and > T in one batch (as far as B allows)."""
  lens = rng.randint(0, 2 * T + 2, size=B)
  fixed = [0, max(T - 1, 0), T, T + 3, 2 * T + 1]
  lens[:min(B, len(fixed))] = fixed[:B]
  return lens


def _ragged(rng, B, T, lo, hi, dtype):
  lens = _lens(rng, B, T)
  splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  ids = rng.randint(lo, hi, size=int(splits[-1])).astype(dtype)
  return ids, splits


def _check(table, ids, splits, bucket, T, pad, d_table=None, **kw):
  """One column through SequenceLookup against the restatement, bit for bit; returns the lookup."""
  t = dev(table) if d_table is None else d_table
  lookup = SequenceLookup([t], [bucket], max_lens=T, pad_ids=pad, **kw)
  outs, lengths = lookup([dev(ids)], None if splits is None else [dev(splits)])
  grid, lens = ref.grid_ref(ids, splits, bucket, T, pad)
  B = lens.size
  assert tuple(outs[0].shape) == (B, T, table.shape[1]) and outs[0].dtype == torch.float32
  assert lengths[0].dtype == torch.int32 and lookup.grids[0].dtype == torch.int64
  np.testing.assert_array_equal(host(lookup.grids[0]), grid)
  np.testing.assert_array_equal(host(lengths[0]), lens)
  np.testing.assert_array_equal(host(outs[0]), ref.forward_ref(table, grid, T))
  return lookup


# ---- 1. forward, exact ------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 5, 64])
@pytest.mark.parametrize('dim', [3, 6, 16, 64, 128, 256])
def test_forward_bit_equal_to_the_restatement(dim, T):
  rng = np.random.RandomState(dim * 100 + T)
  rows = 97
  table = rng.uniform(-1, 1, size=(rows, dim)).astype(F32)
  d_table = dev(table)
  for k, B in enumerate((0, 1, 63, 257)):
    dtype = np.int64 if k % 2 else np.int32
    other = np.int32 if k % 2 else np.int64
    # a bucket, ids of both signs and beyond it, with and without a pad id
    ids, splits = _ragged(rng, B, T, -5 * rows, 5 * rows, dtype)
    _check(table, ids, splits, rows, T, None, d_table)
    _check(table, ids, splits, rows, T, 11, d_table)
    # no bucket: ids >= rows read zeros and stay in the grid, negative ones are -1 there
    ids, splits = _ragged(rng, B, T, -3, rows + 20, other)
    lookup = _check(table, ids, splits, 0, T, None, d_table)
    _check(table, ids, splits, 0, T, rows - 1, d_table)
    if ids.size:
      g = host(lookup.grids[0])
      assert (g >= rows).any() and (g == -1).any()
    # one id per sample
    flat = rng.randint(-3, rows + 20, size=B).astype(dtype)
    _check(table, flat, None, 0, T, None, d_table)
    _check(table, flat, None, 13, T, 5, d_table)
    # samples without any id
    if B:
      _check(table, np.zeros(0, dtype), np.zeros(B + 1, np.int32), rows, T, None, d_table)
      _check(table, np.zeros(0, dtype), np.zeros(B + 1, np.int32), rows, T, 7, d_table)


def test_divisor_maps_the_grid_to_local_rows():
  rng = np.random.RandomState(3)
  bucket, W, dim, T = 1000, 4, 16, 5
  table = rng.uniform(-1, 1, size=(bucket // W, dim)).astype(F32)
  ids, splits = _ragged(rng, 70, T, 0, 1 << 40, np.int64)
  lookup = SequenceLookup([dev(table)], [bucket], max_lens=T, pad_ids=8, divisor=W)
  outs, _ = lookup([dev(ids)], [dev(splits)])
  grid, _ = ref.grid_ref(ids, splits, bucket, T, 8)
  np.testing.assert_array_equal(host(lookup.grids[0]), grid)        # before // divisor
  np.testing.assert_array_equal(host(outs[0]), ref.forward_ref(table, grid, T, divisor=W))


# ---- 2. strided outputs -----------------------------------------------------------------------------------
@pytest.mark.parametrize('dim,off,width', [(6, 2, 40), (16, 1, 100), (16, 4, 100), (128, 8, 700)])
def test_strided_output_keeps_its_neighbours(dim, off, width):
  """A [B, T, dim] block inside a wider tensor: (6, .) and (16, 1, .) take 4-byte chunks (odd dim / rows off
  the 16-byte grid), the others 16-byte chunks with a sample stride of their own."""
  rng = np.random.RandomState(dim + off)
  rows, T, B = 50, 5, 67
  table = rng.uniform(-1, 1, size=(rows, dim)).astype(F32)
  ids, splits = _ragged(rng, B, T, -100, 100, np.int64)
  for pad in (None, 4):
    wide = torch.full((B, width), float('nan'), device=DEV)
    wide.view(torch.int32).fill_(0x7fc0dead)                         # a sentinel NaN with its own bits
    out = wide.as_strided((B, T, dim), (width, dim, 1), off)
    lookup = SequenceLookup([dev(table)], [rows], max_lens=T, pad_ids=pad)
    outs, _ = lookup([dev(ids)], [dev(splits)], outs=[out])
    assert outs[0] is out
    grid, _ = ref.grid_ref(ids, splits, rows, T, pad)
    got = host(wide.view(torch.int32))
    want = np.full((B, width), 0x7fc0dead, np.int32)
    want[:, off:off + T * dim] = ref.forward_ref(table, grid, T).reshape(B, T * dim).view(np.int32)
    np.testing.assert_array_equal(got, want)


# ---- 3. mixed columns, inference form ---------------------------------------------------------------------
def _mixed(rng):
  dims, Ts, pads, buckets = [16, 6, 128], [5, 1, 64], [None, 3, 0], [61, 0, 40]
  rowsn = [61, 30, 40]
  tables = [rng.uniform(-1, 1, size=(r, d)).astype(F32) for r, d in zip(rowsn, dims)]
  B = 130
  data = [_ragged(rng, B, T, -200, 200, dt) for T, dt in zip(Ts, (np.int64, np.int32, np.int64))]
  return dims, Ts, pads, buckets, tables, [d[0] for d in data], [d[1] for d in data]


def test_mixed_columns_and_the_inference_form():
  rng = np.random.RandomState(21)
  dims, Ts, pads, buckets, tables, ids, splits = _mixed(rng)
  lookup = SequenceLookup([dev(t) for t in tables], buckets, max_lens=Ts, pad_ids=pads)
  d_ids, d_sp = [dev(i) for i in ids], [dev(s) for s in splits]
  outs, lengths = lookup(d_ids, d_sp)
  for c in range(3):
    grid, lens = ref.grid_ref(ids[c], splits[c], buckets[c], Ts[c], pads[c])
    np.testing.assert_array_equal(host(lookup.grids[c]), grid)
    np.testing.assert_array_equal(host(lengths[c]), lens)
    np.testing.assert_array_equal(host(outs[c]), ref.forward_ref(tables[c], grid, Ts[c]))
  # grids=False: the same outputs and lengths; the grids of the call before are not written again
  kept = lookup.grids
  for g in kept:
    g.fill_(-77)
  outs2, lengths2 = lookup(d_ids, d_sp, grids=False)
  assert lookup.grids is None
  for c in range(3):
    assert torch.equal(outs2[c], outs[c]) and torch.equal(lengths2[c], lengths[c])
    assert bool((kept[c] == -77).all())
  with pytest.raises(_lib.InvalidArgumentError, match='kept no grids'):
    SequenceLookupGrad(lookup)([torch.zeros_like(o) for o in outs])


# ---- 4. fused and two-launch forms ------------------------------------------------------------------------
def test_two_launch_form_equals_the_fused_one():
  rng = np.random.RandomState(22)
  dims, Ts, pads, buckets, tables, ids, splits = _mixed(rng)
  d_tables = [dev(t) for t in tables]
  d_ids, d_sp = [dev(i) for i in ids], [dev(s) for s in splits]
  fused = SequenceLookup(d_tables, buckets, max_lens=Ts, pad_ids=pads, fused=True)
  outs, lengths = fused(d_ids, d_sp)
  grids, lengths2 = sequence_row_grid(d_ids, d_sp, buckets, Ts, pads)
  plain = GroupLookup(d_tables, buckets=None, combiners='sum')(grids)
  two = SequenceLookup(d_tables, buckets, max_lens=Ts, pad_ids=pads, fused=False)
  outs3, lengths3 = two(d_ids, d_sp)
  for c in range(3):
    assert torch.equal(grids[c], fused.grids[c]) and torch.equal(two.grids[c], fused.grids[c])
    assert torch.equal(lengths2[c], lengths[c]) and torch.equal(lengths3[c], lengths[c])
    assert torch.equal(plain[c], outs[c].view(-1, dims[c]))
    assert torch.equal(outs3[c], outs[c])


# ---- 5. max_norm ------------------------------------------------------------------------------------------
def _normed_table(rng, rows, dim, c):
  t = rng.randn(rows, dim)
  t /= np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-30)
  t *= rng.uniform(0.2 * c, 3 * c, size=(rows, 1))
  t[0] = 0
  return t.astype(F32)


@pytest.mark.parametrize('dim', [3, 16, 128])
def test_max_norm_against_f64(dim):
  """The bound of test_gpu_max_norm.py's forward rows: tests/support/tolerance.py over |y|."""
  rng = np.random.RandomState(dim)
  rows, T, c, pad = 53, 5, 0.5, 9
  table = _normed_table(rng, rows, dim, c)
  table[pad] *= 3.0 * c / np.linalg.norm(table[pad])                 # the pad row lies outside the ball
  ids, splits = _ragged(rng, 90, T, -200, 200, np.int64)
  lookup = SequenceLookup([dev(table)], [rows], max_lens=T, pad_ids=pad, max_norms=c)
  outs, _ = lookup([dev(ids)], [dev(splits)])
  grid, lens = ref.grid_ref(ids, splits, rows, T, pad)
  want, mag = ref.forward_ref(table, grid, T, max_norm=c)
  got = host(outs[0])
  assert_sums_close(got, want, mag, err_msg=f'dim {dim}')
  # pad rows are clipped too
  at_pad = np.arange(T)[None, :] >= lens[:, None]
  assert at_pad.sum() > 50
  norms = np.linalg.norm(got.astype(np.float64), axis=2)
  np.testing.assert_allclose(norms[at_pad], c, rtol=1e-5)
  # the two-launch form clips alike, bit for bit
  two = SequenceLookup([dev(table)], [rows], max_lens=T, pad_ids=pad, max_norms=c, fused=False)
  assert torch.equal(two([dev(ids)], [dev(splits)])[0][0], outs[0])


def test_big_power_of_two_max_norm_changes_no_bit():
  rng = np.random.RandomState(5)
  dims, Ts, pads, buckets, tables, ids, splits = _mixed(rng)        # row norms < 16
  d_tables = [dev(t) for t in tables]
  d_ids, d_sp = [dev(i) for i in ids], [dev(s) for s in splits]
  plain = SequenceLookup(d_tables, buckets, max_lens=Ts, pad_ids=pads)(d_ids, d_sp)[0]
  clipped = SequenceLookup(d_tables, buckets, max_lens=Ts, pad_ids=pads, max_norms=[16.0, None, 16.0])(
    d_ids, d_sp)[0]
  for a, b in zip(plain, clipped):
    assert torch.equal(a, b)


# ---- 6. backward, emit form -------------------------------------------------------------------------------
def _bwd_case(rng, pad):
  """B = 64, T = 5; many short samples: with a pad id (31; real ids are < 30) its row collects > 100
  padding positions.  Row 33 is named at truncated positions only."""
  rows, dim, B, T = 37, 16, 64, 5
  lens = rng.choice([0, 1, 2, 7, 9], size=B)
  lens[:3] = [7, 9, 7]
  splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  ids = rng.randint(0, 30, size=int(splits[-1])).astype(np.int64)
  for b in range(B):                     # row 33: at truncated positions only
    if lens[b] > T:
      ids[splits[b] + T:splits[b + 1]] = 33
  table = rng.uniform(-1, 1, size=(rows, dim)).astype(F32)
  grads = rng.randn(B, T, dim).astype(F32)
  grid, ln = ref.grid_ref(ids, splits, rows, T, pad)
  return rows, dim, B, T, ids, splits, table, grads, grid, ln


def _slices(res):
  urows, grows, nu = res
  k = int(nu.item())
  return host(urows)[:k], host(grows)[:k]


@pytest.mark.parametrize('plan', ['default', 'split'])
@pytest.mark.parametrize('pad', [None, 31])
def test_backward_emit_against_the_f64_scatter(pad, plan, hbk_option):
  if plan == 'split':
    # one hashed bucket cut into workgroups of 64 pairs: the pad row's > 100 terms span several
    hbk_option('bwd_dense', 0)
    hbk_option('bwd_buckets_log2', 0)
    hbk_option('bwd_split_pairs', 64)
  rng = np.random.RandomState(8)
  rows, dim, B, T, ids, splits, table, grads, grid, ln = _bwd_case(rng, pad)
  lookup = SequenceLookup([dev(table)], [rows], max_lens=T, pad_ids=pad)
  lookup([dev(ids)], [dev(splits)])
  grad = SequenceLookupGrad(lookup)
  u, want, mag = ref.grad_ref(grid, grads, rows)
  got_rows, got = _slices(grad([dev(grads)])[0])
  order = np.argsort(got_rows)
  np.testing.assert_array_equal(got_rows[order], u)
  assert_sums_close(got[order], want, mag, err_msg=f'pad {pad} {plan}')
  assert 33 not in got_rows.tolist()                                 # truncated positions only
  n_padding = int((T - ln).sum())
  assert n_padding > 100
  if pad is None:
    assert 31 not in got_rows.tolist() and (grid == -1).sum() == n_padding
  else:
    # the pad row: every padding position (31 is no real id: ids < 30) -- more than 100 terms
    k = got_rows.tolist().index(31)
    at_pad = (np.arange(T)[None, :] >= ln[:, None]).reshape(-1)
    w = grads.reshape(-1, dim)[at_pad].astype(np.float64)
    assert_sums_close(got[k], w.sum(0), np.abs(w).sum(0), err_msg='pad row')
  # deterministic: rows ascending, bit-equal to the sequential fp32 sum in position order
  det_rows, det = _slices(grad([dev(grads)], deterministic=True)[0])
  u32, s32 = ref.grad_seq32(grid, grads, rows)
  np.testing.assert_array_equal(det_rows, u32)
  np.testing.assert_array_equal(det, s32)


def test_backward_takes_strided_gradients_and_explicit_grids():
  rng = np.random.RandomState(9)
  rows, dim, B, T, ids, splits, table, grads, grid, _ = _bwd_case(rng, 31)
  lookup = SequenceLookup([dev(table)], [rows], max_lens=T, pad_ids=31)
  grad = SequenceLookupGrad(lookup)
  u32, s32 = ref.grad_seq32(grid, grads, rows)
  d_grid = sequence_row_grid([dev(ids)], [dev(splits)], [rows], T, 31)[0]
  wide = torch.zeros(B, T, dim + 4, device=DEV)                      # rows a uniform 20 floats apart: in place
  wide[:, :, :dim] = dev(grads)
  odd = torch.zeros(B, T * dim + 3, device=DEV)                      # samples 83 floats apart: one copy
  odd[:, :T * dim] = dev(grads).view(B, -1)
  for g in (dev(grads), wide[:, :, :dim], odd[:, :T * dim].view(B, T, dim), dev(grads).view(B * T, dim)):
    r, s = _slices(grad([g], deterministic=True, grids=d_grid)[0])
    np.testing.assert_array_equal(r, u32)
    np.testing.assert_array_equal(s, s32)


# ---- 7. optimizers: the plumbing --------------------------------------------------------------------------
@pytest.mark.parametrize('optimizer', ['sgd', 'adagrad', 'adam', 'ftrl'])
def test_steps_equal_group_lookup_grad_on_the_restatements_grid(optimizer):
  rng = np.random.RandomState(12)
  rows, dim, B, T, ids, splits, table, grads, grid, _ = _bwd_case(rng, None)
  lr = 0.05

  def state():
    t = dev(table)
    return dict(t=t, acc=torch.full_like(t, 0.1), mom=(torch.zeros_like(t), torch.zeros_like(t)),
                fs=hb.embedding.Ftrl().slots_like(t), adam=hb.embedding.LazyAdam(device=DEV))

  def kw(s):
    return dict(accums=[s['acc']], moments=[s['mom']], adam=s['adam'], ftrl_slots=[s['fs']])

  a, b = state(), state()
  lookup = SequenceLookup([a['t']], [rows], max_lens=T)
  lookup([dev(ids)], [dev(splits)])
  seq = SequenceLookupGrad(lookup, **kw(a))
  direct = GroupLookupGrad(GroupLookup([b['t']], buckets=None, combiners='sum'), deterministic=True, **kw(b))
  d_grid, flat = dev(grid), dev(grads.reshape(B * T, dim))
  for _ in range(2):
    ra = seq([dev(grads)], apply_lr=lr, optimizer=optimizer, deterministic=True)
    rb = direct([d_grid], [flat], apply_lr=lr, optimizer=optimizer)
    for x, y in zip(_slices(ra[0]), _slices(rb[0])):
      np.testing.assert_array_equal(x, y)
  for k in ('t', 'acc'):
    assert torch.equal(a[k], b[k]), k
  for k in ('mom', 'fs'):
    assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]), k
  assert not torch.equal(a['t'], dev(table))
  # row 33 occurs at truncated positions only: weights and slots keep their bits
  np.testing.assert_array_equal(host(a['t'][33]), table[33])
  if optimizer == 'adam':
    assert not bool(a['mom'][0][33].any()) and not bool(a['mom'][1][33].any())
    assert bool(a['mom'][0][:30].any())
    # two steps advanced the powers twice
    p = (F32(0.9), F32(0.999))
    for _ in range(2):
      p = (F32(p[0] * F32(0.9)), F32(p[1] * F32(0.999)))
    np.testing.assert_array_equal(host(a['adam'].beta_powers), np.array(p, F32))
    np.testing.assert_array_equal(host(b['adam'].beta_powers), np.array(p, F32))
  else:
    np.testing.assert_array_equal(host(a['adam'].beta_powers), np.array([0.9, 0.999], F32))


# ---- 8. no host synchronisation: a captured graph ---------------------------------------------------------
def test_forward_and_backward_inside_a_captured_graph():
  rng = np.random.RandomState(14)
  rows, dim, B, T, pad, lr = 211, 16, 96, 5, 7, 0.05
  n_ids = 400
  table = rng.uniform(-1, 1, size=(rows, dim)).astype(F32)

  def batch():
    cut = np.sort(rng.randint(0, n_ids + 1, size=B - 1))
    splits = np.concatenate([[0], cut, [n_ids]]).astype(np.int32)   # (the same id count every step)
    return rng.randint(-1000, 1000, size=n_ids).astype(np.int64), splits, rng.randn(B, T, dim).astype(F32)

  d_ids = torch.zeros(n_ids, dtype=torch.int64, device=DEV)
  d_sp = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
  d_g = torch.zeros(B, T, dim, device=DEV)
  t_graph, t_eager = dev(table), dev(table)
  lookup = SequenceLookup([t_graph], [rows], max_lens=T, pad_ids=pad)
  grad = SequenceLookupGrad(lookup)

  def step():
    outs, lengths = lookup([d_ids], [d_sp])
    res = grad([d_g], apply_lr=lr, deterministic=True)
    return outs[0], lengths[0], res[0]

  side = torch.cuda.Stream()
  with torch.cuda.stream(side):       # warm-up on the capture stream (allocations, lazy set-up)
    step()
  torch.cuda.synchronize()
  t_graph.copy_(t_eager)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    out, lengths, (urows, grows, nu) = step()
  eager_lookup = SequenceLookup([t_eager], [rows], max_lens=T, pad_ids=pad)
  eager_grad = SequenceLookupGrad(eager_lookup)
  for _ in range(2):
    ids, splits, g = batch()
    d_ids.copy_(dev(ids))
    d_sp.copy_(dev(splits))
    d_g.copy_(dev(g))
    graph.replay()
    torch.cuda.synchronize()
    e_out, e_len = eager_lookup([dev(ids)], [dev(splits)])
    e_res = eager_grad([dev(g)], apply_lr=lr, deterministic=True)[0]
    torch.cuda.synchronize()
    assert torch.equal(out, e_out[0]) and torch.equal(lengths, e_len[0])
    k = int(nu.item())
    assert k == int(e_res[2].item())
    assert torch.equal(urows[:k], e_res[0][:k]) and torch.equal(grows[:k], e_res[1][:k])
    assert torch.equal(t_graph, t_eager)
    grid, lens = ref.grid_ref(ids, splits, rows, T, pad)
    np.testing.assert_array_equal(host(lengths), lens)
  assert not torch.equal(t_graph, dev(table))
