"""Hash-keyed feature columns on the GPU: the raw-id grid kernel against numpy, DenseFeatures and SequenceFeatures
with HashEmbeddingColumn / HashSequenceEmbeddingColumn against the hand composition (HashGroupLookup +
GroupLookupGrad, HashSequenceLookup), growth and eviction through the layer, W = 2 against W = 1 (ranks are host
threads over Collective.local_world), and checkpoints across world sizes.  A row's start depends on its key alone
(tests/support/hash_ref.py), so tables are compared BY KEY, whatever slot or rank a key got."""
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
import oracle
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (GroupLookupGrad, HashGroupLookup, HashSequenceLookup, HashTable, LazyAdam,
                                         Ftrl, SequenceLookupGrad, sequence_id_grid)
from tests.support import hash_ref as ref
from tests.support.sharded_hash_ref import Model, owner
from tests.support.tolerance import assert_sums_close, world_grad_sums

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
fc = hb.feature_column
EMPTY, TOMBSTONE = -2 ** 63, -2 ** 63 + 1
SCALE = 0.05


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


@pytest.fixture
def deterministic():
  old = _lib.set_option('bwd_deterministic', 1)
  yield
  _lib.set_option('bwd_deterministic', old)


def run_world(world, fn):
  """fn(rank, comm) on `world` host threads, each on a stream of its own; returns the per-rank results."""
  comms = hb.distribute.Collective.local_world(world)
  results, errors = [None] * world, []

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        results[r] = fn(r, comms[r])
        torch.cuda.current_stream().synchronize()
    except Exception as e:  # pylint: disable=broad-except
      import traceback
      errors.append((r, repr(e), traceback.format_exc()))

  threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=45)
  for cm in comms:
    cm.close()
  assert not errors, errors
  assert all(x is not None for x in results)
  return results


def by_key(table, tensors):
  """{key: tuple of that key's row in every tensor} of one HashTable (copies on the host)."""
  keys = host(table.keys)
  live = (keys != EMPTY) & ((keys != TOMBSTONE) | (not table.expiring))
  arrays = [host(x) for x in tensors]
  return {int(keys[s]): tuple(np.array(a[s]) for a in arrays) for s in np.nonzero(live)[0]}


def layer_state(layer, c):
  """Column c of a layer by key: (row, every optimizer slot..., last_seen, freq where the table expires)."""
  t = layer.hash_tables[c]
  assert layer.weights[c] is t.table
  tensors = [t.table] + [x for x, _ in layer._hash_companions(c)]   # pylint: disable=protected-access
  for x in tensors:
    assert tuple(x.shape) == (t.capacity, t.dim)
  if t.expiring:
    tensors += [t.last_seen, t.freq]
  return by_key(t, tensors)


def assert_same_by_key(got, want, what=''):
  assert set(got) == set(want), f'{what}: key sets differ ({len(got)} vs {len(want)})'
  for k, rows in want.items():
    for n, (a, b) in enumerate(zip(got[k], rows)):
      np.testing.assert_array_equal(a, b, err_msg=f'{what}: key {k}, tensor {n}')


def merged(states):
  out = {}
  for s in states:
    assert not set(s) & set(out)
    out.update(s)
  return out


def pick_keys(rng, n, stages, extra=(), keep=None):
  """n distinct keys, negative ones and ones above 2^40 among them, such that for every (first, slab_count) of
  `stages` no home slab of a table of slab_count slabs of 8 holds more than 8 of the first `first` keys: every key
  then lives in its home slab whatever the order of the inserts, and no insert fails."""
  cand = list(extra) + np.concatenate([rng.randint(-2 ** 62, 0, size=4 * n, dtype=np.int64),
                                       rng.randint(2 ** 40, 2 ** 62, size=4 * n, dtype=np.int64),
                                       rng.randint(0, 10 ** 6, size=4 * n, dtype=np.int64)])[rng.permutation(12 * n)].tolist()
  counts = [dict() for _ in stages]
  out, seen = [], set()
  for k in cand:
    if k in seen or (keep is not None and not keep(k)):
      continue
    homes =[(s, ref.home_slab(k, slabs)) for s, (first, slabs) in enumerate(stages) if len(out) < first]
    if any(counts[s].get(h, 0) >= 8 for s, h in homes):
      continue
    for s, h in homes:
      counts[s][h] = counts[s].get(h, 0) + 1
    seen.add(k)
    out.append(k)
    if len(out) == n:
      return np.array(out, np.int64)
  raise AssertionError('not enough candidates')


def ragged(rng, pool, n_samples, lam=3):
  lens = rng.poisson(lam, size=n_samples).clip(0, 9)
  splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  return pool[rng.randint(0, pool.size, size=int(splits[-1]))], splits


# ---- 1. the raw-id grid ------------------------------------------------------------------------------------
def id_grid_ref(ids, splits, T, pad):
  ids = np.asarray(ids).astype(np.int64)
  if splits is None:
    splits = np.arange(ids.size + 1)
  B = len(splits) - 1
  grid = np.full(B * T, pad, np.int64)
  lengths = np.zeros(B, np.int32)
  for b in range(B):
    L = min(int(splits[b + 1] - splits[b]), T)
    grid[b * T:b * T + L] = ids[splits[b]:splits[b] + L]
    lengths[b] = L
  return grid, lengths


POISON = 0x5A5A5A5A5A5A5A5A


def poisoned(ids):
  """`ids` as a view of a longer device buffer: what lies behind them is poison."""
  ids = np.asarray(ids)
  big = np.full(ids.size + 64, POISON if ids.dtype == np.int64 else 0x5A5A5A5A, ids.dtype)
  big[:ids.size] = ids
  return dev(big)[:ids.size]


def raw_grid(ids, splits, T, pad, want_lengths=True, has_pad=1):
  """hbk_sequence_id_grid_n on one column through the C ABI; returns (status, grid, lengths)."""
  col, seq = (_lib.LookupColumn * 1)(), (_lib.Sequence * 1)()
  B = ids.numel() if splits is None else splits.numel() - 1
  grid = torch.full((B * T,), 77, dtype=torch.int64, device=DEV)
  lengths = torch.full((B,), -7, dtype=torch.int32, device=DEV)
  col[0].ids, col[0].n_ids = ids.data_ptr(), ids.numel()
  col[0].ids_dtype = _lib.INT64 if ids.dtype == torch.int64 else _lib.INT32
  col[0].row_splits, col[0].n_segments = (splits.data_ptr() if splits is not None else None), B
  seq[0].max_len, seq[0].has_pad, seq[0].pad_id = T, has_pad, pad
  seq[0].lengths, seq[0].row_grid = (lengths.data_ptr() if want_lengths else None), grid.data_ptr()
  status = _lib.lib().hbk_sequence_id_grid_n(1, col, seq, _lib.current_stream(torch.device(DEV)))
  return status, grid, lengths


def test_id_grid_equals_numpy_bit_for_bit():
  lens = np.array([0, 1, 3, 4, 7, 4])
  splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  ids = np.arange(100, 100 + splits[-1]).astype(np.int64)
  ids[:4] = [-1, -2 ** 63 + 2, 2 ** 62, 0]
  late = ids[splits[4] + 4:splits[5]].copy()          # positions 4.. of the length-7 sample
  pad = -2 ** 40 - 5
  want, want_len = id_grid_ref(ids, splits, 4, pad)
  (got,), (got_len,) = sequence_id_grid([poisoned(ids)], [dev(splits)], 4, pad)
  np.testing.assert_array_equal(host(got), want)
  np.testing.assert_array_equal(host(got_len), want_len)
  assert got.dtype == torch.int64 and got_len.dtype == torch.int32
  assert not np.isin(late, host(got)).any() and not (host(got) == POISON).any()
  # T = 1; one id per sample (row_splits None); int32 ids are sign-extended; two columns of different T at once
  i32 = np.array([-1, 5, -2 ** 31, 2 ** 31 - 1, 0, 9, 3], np.int32)
  sp32 = np.array([0, 2, 2, 7], np.int32)
  grids, lengths = sequence_id_grid([poisoned(ids), poisoned(i32), poisoned(ids[:5]), poisoned(i32)],
                                    [dev(splits), dev(sp32), None, None], [1, 3, 2, 1], [pad, -9, 0, 2 ** 62])
  for k, (i, s, T, p) in enumerate([(ids, splits, 1, pad), (i32, sp32, 3, -9), (ids[:5], None, 2, 0),
                                    (i32, None, 1, 2 ** 62)]):
    w, wl = id_grid_ref(i, s, T, p)
    np.testing.assert_array_equal(host(grids[k]), w, err_msg=f'column {k}')
    np.testing.assert_array_equal(host(lengths[k]), wl, err_msg=f'column {k}')
  # B = 0: nothing is written, nothing fails
  (g0,), (l0,) = sequence_id_grid([dev(np.zeros(0, np.int64))], [dev(np.zeros(1, np.int32))], 4, pad)
  assert g0.numel() == 0 and l0.numel() == 0
  # lengths not wanted
  status, g, ln = raw_grid(poisoned(ids), dev(splits), 4, pad, want_lengths=False)
  assert status == _lib.OK
  np.testing.assert_array_equal(host(g), want)
  assert (host(ln) == -7).all()
  # more than one block, B * T no multiple of the block
  rng = np.random.RandomState(3)
  big_ids, big_sp = ragged(rng, rng.randint(-2 ** 62, 2 ** 62, size=500, dtype=np.int64), 301, lam=5)
  (g,), (ln,) = sequence_id_grid([poisoned(big_ids)], [dev(big_sp)], 7, -1)
  w, wl = id_grid_ref(big_ids, big_sp, 7, -1)
  np.testing.assert_array_equal(host(g), w)
  np.testing.assert_array_equal(host(ln), wl)


def test_id_grid_refusals_and_capture():
  ids, splits = dev(np.arange(10, dtype=np.int64)), dev(np.array([0, 3, 10], np.int32))
  for kw, text in [(dict(has_pad=0), 'has_pad is 0'), (dict(T=0), 'max_len must be >= 1')]:
    status, _, _ = raw_grid(ids, splits, kw.get('T', 4), -1, has_pad=kw.get('has_pad', 1))
    assert status == _lib.INVALID_ARGUMENT and text in _lib.lib().hbk_last_error().decode()
  col, seq = (_lib.LookupColumn * 1)(), (_lib.Sequence * 1)()
  col[0].ids, col[0].n_ids, col[0].ids_dtype, col[0].n_segments = ids.data_ptr(), 10, _lib.INT64, 10
  seq[0].max_len, seq[0].has_pad = 2, 1
  stream = _lib.current_stream(torch.device(DEV))
  assert _lib.lib().hbk_sequence_id_grid_n(1, col, seq, stream) == _lib.INVALID_ARGUMENT        # row_grid NULL
  assert 'row_grid is NULL' in _lib.lib().hbk_last_error().decode()
  assert _lib.lib().hbk_sequence_id_grid_n(1, col, None, stream) == _lib.INVALID_ARGUMENT       # seq NULL
  assert 'seq is NULL' in _lib.lib().hbk_last_error().decode()
  seq[0].row_grid, seq[0].max_len, col[0].n_segments, col[0].n_ids = ids.data_ptr(), 2 ** 30, 2, 2
  assert _lib.lib().hbk_sequence_id_grid_n(1, col, seq, stream) == _lib.INVALID_ARGUMENT        # B * T >= 2^31
  assert 'below 2^31' in _lib.lib().hbk_last_error().decode()
  # inside a captured graph: replays follow the id buffer
  buf = dev(np.arange(10, dtype=np.int64))
  out = {}

  def call():
    status, out['grid'], out['len'] = raw_grid(buf, splits, 4, -3)
    assert status == _lib.OK
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      call()
  torch.cuda.synchronize()
  fresh = np.arange(10, dtype=np.int64) * -1000 - 1
  buf.copy_(dev(fresh))
  graph.replay()
  torch.cuda.synchronize()
  w, wl = id_grid_ref(fresh, host(splits), 4, -3)
  np.testing.assert_array_equal(host(out['grid']), w)
  np.testing.assert_array_equal(host(out['len']), wl)


# ---- 2. DenseFeatures forward, a mixed layer on one GPU ----------------------------------------------------
def wide_keys(rng, n):
  return np.unique(np.concatenate([rng.randint(-2 ** 62, 0, size=n, dtype=np.int64),
                                   rng.randint(2 ** 40, 2 ** 62, size=n, dtype=np.int64), [-1, 0, 2 ** 63 - 1]]))


@pytest.mark.parametrize('staged', [False, True])
def test_dense_forward_mixed_layer(staged):
  rng = np.random.RandomState(11)
  B = 64
  b0, b1 = fc.EmbeddingColumn('b0', 1009, 16, 'mean'), fc.EmbeddingColumn('b1', 53, 6, 'sum')
  h0 = fc.HashEmbeddingColumn('h0', 1024, 6, 'mean', init_scale=SCALE, seed=3)
  h1 = fc.HashEmbeddingColumn('h1', 1024, 16, 'sum', init_scale=SCALE, seed=4, slab_size=16)
  h2 = fc.HashEmbeddingColumn('h2', 512, 72, 'sum', init_scale=SCALE, seed=5)
  cols = [b0, h0] + ([h2] if staged else []) + [b1, h1]      # h2: dimension 72 at offset 22, staged
  tables = {'b0': rng.uniform(-1, 1, size=(1009, 16)).astype(F32), 'b1': rng.uniform(-1, 1, size=(53, 6)).astype(F32)}
  init = lambda col, rows, d: dev(tables[col.key])   # noqa: E731
  pool = wide_keys(rng, 60)
  feats = {'b0': ragged(rng, rng.randint(-10 ** 6, 10 ** 6, size=300).astype(np.int64), B),
           'b1': (rng.randint(0, 10 ** 6, size=B).astype(np.int64), None),
           'h0': ragged(rng, pool, B), 'h1': (pool[rng.randint(0, pool.size, size=B)], None),
           'h2': (pool[rng.randint(0, pool.size, size=B)], None)}
  d_feats = {k: (dev(i), dev(s)) if s is not None else dev(i) for k, (i, s) in feats.items()}
  layer = fc.DenseFeatures(cols, DEV, init=init)
  assert layer.hash_tables[0] is None and [layer.hash_tables[c] is not None for c in range(len(cols))] == \
      [isinstance(c, fc.HashEmbeddingColumn) for c in cols]
  assert layer._staged == ({2} if staged else set())   # pylint: disable=protected-access
  views = {}
  out = layer(d_feats, cols_to_output_tensors=views)
  assert tuple(out.shape) == (B, sum(c.dimension for c in cols))
  plain = fc.DenseFeatures([b0, b1], DEV, init=init)
  plain_views = {}
  plain(d_feats, cols_to_output_tensors=plain_views)
  for col in (b0, b1):
    assert torch.equal(views[col], plain_views[col]), col.key
  for col in cols:
    if not isinstance(col, fc.HashEmbeddingColumn):
      continue
    ids, splits = feats[col.key]
    m = Model([ids], col.dimension, col.table_args['seed'], SCALE)
    want = oracle.group_lookup_fwd([m.w], [m.index(ids)], [splits], [m.uniq.size], [col.combiner])[0]
    np.testing.assert_array_equal(host(views[col]), want, err_msg=col.key)
    t = layer.hash_tables[cols.index(col)]
    assert t.size() == m.uniq.size and t.failed() == 0
  # the second call finds every key and gives the same block
  assert torch.equal(layer(d_feats), out)


# ---- 3. training equals the hand composition ---------------------------------------------------------------
def train_columns(cap0=1024, cap1=1024, **kw):
  return [fc.HashEmbeddingColumn('h0', cap0, 6, 'mean', init_scale=SCALE, seed=3, **kw),
          fc.HashEmbeddingColumn('h1', cap1, 16, 'sum', init_scale=SCALE, seed=4, **kw)]


def train_batches(rng, steps, B, pools):
  out = []
  for _ in range(steps):
    i0, s0 = ragged(rng, pools[0], B)
    out.append(dict(ids=[i0, pools[1][rng.randint(0, pools[1].size, size=B)]], splits=[s0, None],
                    grad=rng.randn(B, 22).astype(F32)))
  return out


def feats_of(b):
  return {'h0': (dev(b['ids'][0]), dev(b['splits'][0])), 'h1': dev(b['ids'][1])}


@pytest.mark.parametrize('optimizer', ['adagrad', 'adam', 'ftrl'])
def test_training_equals_the_hand_composition(optimizer, deterministic):   # pylint: disable=unused-argument,redefined-outer-name
  rng = np.random.RandomState(21)
  pools = [wide_keys(rng, 70), wide_keys(rng, 70)]
  batches = train_batches(rng, 3, 48, pools)
  lr = 0.1
  cols = train_columns(expiring=True)
  kw = dict(initial_accumulator_value=0.1) if optimizer == 'adagrad' else dict(optimizer=optimizer)
  layer = fc.DenseFeatures(cols, DEV, **kw)
  # by hand: the tables, the slots, the lookup and the grad object
  tables = [HashTable(c.capacity, c.dimension, DEV, **c.table_args) for c in cols]
  hgl = HashGroupLookup(tables, combiners=[c.combiner for c in cols])
  slots = {}
  if optimizer == 'adagrad':
    slots['accums'] = [torch.full_like(t.table, 0.1) for t in tables]
  elif optimizer == 'adam':
    slots['adam'] = LazyAdam.default(DEV)
    slots['moments'] = [slots['adam'].slots_like(t.table) for t in tables]
  else:
    slots['ftrl'] = Ftrl()
    slots['ftrl_slots'] = [slots['ftrl'].slots_like(t.table) for t in tables]
  grad = GroupLookupGrad(hgl.lookup, **slots)
  for n, b in enumerate(batches):
    layer.set_step(n + 5)
    for t in tables:
      t.set_step(n + 5)
    out = layer(feats_of(b))
    want = hgl([dev(i) for i in b['ids']], [dev(b['splits'][0]), None])
    assert torch.equal(out[:, :6], want[0]) and torch.equal(out[:, 6:], want[1])
    g = dev(b['grad'])
    res = layer.backward(g, apply_lr=lr, optimizer=optimizer)
    grad(hgl.slots, [g[:, :6].contiguous(), g[:, 6:].contiguous()], [dev(b['splits'][0]), None], apply_lr=lr,
         optimizer=optimizer)
    # the slices name slot numbers of the layer's tables
    for c in range(2):
      k = int(res[c][2].item())
      named = host(layer.hash_tables[c].keys)[host(res[c][0])[:k]]
      assert set(named.tolist()) == set(b['ids'][c].tolist())
  for c, t in enumerate(tables):
    hand = [t.table]
    hand += [slots['accums'][c]] if optimizer == 'adagrad' else list(slots['moments' if optimizer == 'adam' else 'ftrl_slots'][c])
    assert_same_by_key(layer_state(layer, c), by_key(t, hand + [t.last_seen, t.freq]), f'{optimizer} column {c}')
    seen = layer_state(layer, c)
    last = {k: int(v[-2]) for k, v in seen.items()}
    assert max(last.values()) == 7 and all(last[int(k)] == 7 for k in np.unique(batches[-1]['ids'][c]))
  if optimizer == 'adam':
    assert torch.equal(layer.adam.beta_powers, slots['adam'].beta_powers)


def test_weighted_hash_column_on_one_rank(deterministic):   # pylint: disable=unused-argument,redefined-outer-name
  rng = np.random.RandomState(22)
  ids, splits = ragged(rng, wide_keys(rng, 40), 48)
  w = rng.uniform(0.5, 2.0, size=ids.size).astype(F32)
  g = dev(rng.randn(48, 6).astype(F32))
  col = fc.HashEmbeddingColumn('h0', 1024, 6, 'mean', init_scale=SCALE, seed=3, weight_feature_key='w')
  layer = fc.DenseFeatures([col], DEV)
  out = layer({'h0': (dev(ids), dev(splits)), 'w': dev(w)})
  table = HashTable(1024, 6, DEV, init_scale=SCALE, seed=3)
  hgl = HashGroupLookup([table], combiners=['mean'])
  want = hgl([dev(ids)], [dev(splits)], sp_weights=[dev(w)])[0]
  assert torch.equal(out, want) and not torch.equal(out, hgl([dev(ids)], [dev(splits)])[0])
  hgl([dev(ids)], [dev(splits)], sp_weights=[dev(w)])
  _, wgrads = layer.backward(g, apply_lr=0.1, weight_grads=True)
  hand = GroupLookupGrad(hgl.lookup)(hgl.slots, [g], [dev(splits)], apply_lr=0.1, sp_weights=[dev(w)],
                                     weight_grads=[True])
  assert set(wgrads) == {'w'} and torch.equal(wgrads['w'], hand[1][0]) and host(wgrads['w']).any()
  assert_same_by_key(layer_state(layer, 0), by_key(table, [table.table]), 'weighted step')


# ---- 4. growth and eviction through the layer --------------------------------------------------------------
def test_maybe_grow_equals_a_layer_that_never_grows(deterministic):   # pylint: disable=unused-argument,redefined-outer-name
  rng = np.random.RandomState(31)
  new = [50, 47, 30, 25]        # 50 / 64 > 0.75: 128 slots; 97 / 128 > 0.75: 256 slots; 127, 152 of 256: stays
  stages = [(50, 8), (97, 16), (152, 32), (152, 128)]
  keys = [pick_keys(rng, 152, stages, extra=[-1, 2 ** 62]) for _ in range(2)]
  B, lr = 96, 0.1
  small = fc.DenseFeatures(train_columns(cap0=64, cap1=64), DEV, initial_accumulator_value=0.1)
  large = fc.DenseFeatures(train_columns(), DEV, initial_accumulator_value=0.1)
  seen, grown = 0, []
  for n, k in enumerate(new):
    fresh = [x[seen:seen + k] for x in keys]
    seen += k
    lens = rng.poisson(3, size=B).clip(0, 9)
    splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    i0 = keys[0][rng.randint(0, seen, size=int(splits[-1]))]
    i0[rng.permutation(i0.size)[:k]] = fresh[0]
    i1 = keys[1][rng.randint(0, seen, size=B)]
    i1[rng.permutation(B)[:k]] = fresh[1]
    b = dict(ids=[i0, i1], splits=[splits, None], grad=rng.randn(B, 22).astype(F32))
    for layer in (small, large):
      layer(feats_of(b))
      layer.backward(dev(b['grad']), apply_lr=lr, optimizer='adagrad', emit=False)
    before = [small.weights[c] for c in range(2)]
    grown.append(small.maybe_grow())
    assert large.maybe_grow() == []
    for c in range(2):
      t = small.hash_tables[c]
      assert small.weights[c] is t.table and (small.weights[c] is not before[c]) == (f'h{c}' in grown[-1])
      assert tuple(small.accums[c].shape) == (t.capacity, t.dim) and t.failed() == 0
  assert grown == [['h0', 'h1'], ['h0', 'h1'], [], []]
  assert [t.capacity for t in small.hash_tables] == [256, 256]
  for c in range(2):
    assert len(layer_state(small, c)) == 152
    assert_same_by_key(layer_state(small, c), layer_state(large, c), f'column {c}')


def test_maybe_evict_lfu_through_the_layer():
  rng = np.random.RandomState(32)
  keys = pick_keys(rng, 52, [(52, 8)])
  col = fc.HashEmbeddingColumn('h', 64, 6, 'sum', init_scale=SCALE, expiring=True)
  layer = fc.DenseFeatures([col], DEV, initial_accumulator_value=0.1)
  plain = fc.DenseFeatures([fc.HashEmbeddingColumn('p', 64, 6, 'sum')], DEV)
  with pytest.raises(_lib.InvalidArgumentError) as e:
    plain.maybe_evict()
  assert "'p'" in str(e.value) and 'not expiring' in str(e.value)
  for step, ids in enumerate([keys[:30], np.concatenate([keys[:10], keys[30:]])]):    # keys[:10] are seen twice
    layer.set_step(step + 1)
    layer({'h': dev(ids)})
    layer.backward(dev(rng.randn(ids.size, 6).astype(F32)), apply_lr=0.1, optimizer='adagrad', emit=False)
  t = layer.hash_tables[0]
  assert t.size() == 52
  assert layer.maybe_evict(order='lfu') == ['h']        # 52 / 64 > 0.75: down to <= 32 keys, the least used first
  assert t.size() <= 0.5 * t.capacity and layer.weights[0] is t.table and t.capacity == 64
  left = layer_state(layer, 0)
  assert set(keys[:10].tolist()) <= set(left)           # the keys seen twice are the most frequently used
  assert tuple(layer.accums[0].shape) == (64, 6)
  layer.set_step(3)
  out = layer({'h': dev(keys[:40])})
  layer.backward(torch.ones_like(out), apply_lr=0.1, optimizer='adagrad', emit=False)
  after = layer_state(layer, 0)
  assert set(keys[:40].tolist()) <= set(after) and t.failed() == 0
  for k in keys[:10].tolist():
    assert not np.array_equal(after[k][0], left[k][0]) and (after[k][1] > left[k][1]).all()


def test_maybe_grow_on_two_ranks(deterministic):   # pylint: disable=unused-argument,redefined-outer-name
  """The sharded driver's rebind with the layer's slots: every rank's 64-slot table takes 50 keys in the first step
  and grows; by key the layer equals one of 512 slots per rank that never grows."""
  rng = np.random.RandomState(33)
  world, B, lr = 2, 60, 0.1
  own = [pick_keys(rng, 50, [(50, 8), (50, 16), (50, 64)], keep=lambda k, r=r: k % world == r) for r in range(world)]
  pool = np.concatenate(own)[rng.permutation(100)]
  batches = [[dict(ids=np.concatenate([pool[r * 50:(r + 1) * 50], pool[rng.randint(0, 100, size=10)]]),
                   grad=rng.randn(B, 6).astype(F32)) for r in range(world)],
             [dict(ids=pool[rng.randint(0, 100, size=B)], grad=rng.randn(B, 6).astype(F32)) for r in range(world)]]
  column = lambda cap: fc.HashEmbeddingColumn('h', cap, 6, 'sum', init_scale=SCALE, seed=3)   # noqa: E731

  def rank(r, comm):
    small = fc.DenseFeatures([column(128)], DEV, coll=comm, initial_accumulator_value=0.1)
    large = fc.DenseFeatures([column(1024)], DEV, coll=comm, initial_accumulator_value=0.1)
    assert small.hash_tables[0].capacity == 64 and large.hash_tables[0].capacity == 512
    grown = []
    for per_rank in batches:
      for layer in (small, large):
        layer({'h': dev(per_rank[r]['ids'])})
        layer.backward(dev(per_rank[r]['grad']), apply_lr=lr, optimizer='adagrad', emit=False)
      grown.append((small.maybe_grow(), large.maybe_grow()))
    torch.cuda.current_stream().synchronize()
    t = small.hash_tables[0]
    res = dict(grown=grown, capacity=t.capacity, failed=t.failed(), accum=tuple(small.accums[0].shape),
               small=layer_state(small, 0), large=layer_state(large, 0))
    small.close()
    large.close()
    return res

  res = run_world(world, rank)
  for r, x in enumerate(res):
    assert x['grown'] == [(['h'], []), ([], [])] and x['capacity'] == 128 and x['accum'] == (128, 6)
    assert x['failed'] == 0 and set(x['small']) == set(own[r].tolist())
    assert_same_by_key(x['small'], x['large'], f'rank {r}')


# ---- 5. two ranks against one ------------------------------------------------------------------------------
def test_two_ranks_equal_one_rank():
  rng = np.random.RandomState(41)
  world, B, lr = 2, 40, 0.1
  pools = [wide_keys(rng, 60), wide_keys(rng, 60)]
  steps = [[train_batches(rng, 1, B, pools)[0] for _ in range(world)] for _ in range(2)]

  def whole(per_rank):
    sp = [per_rank[0]['splits'][0]] + [b['splits'][0][1:] + sum(int(x['splits'][0][-1]) for x in per_rank[:r])
                                      for r, b in enumerate(per_rank) if r > 0]
    return dict(ids=[np.concatenate([b['ids'][c] for b in per_rank]) for c in range(2)],
                splits=[np.concatenate(sp).astype(np.int32), None],
                grad=np.concatenate([b['grad'] for b in per_rank]))

  one = fc.DenseFeatures(train_columns(), DEV)
  first = None
  for per_rank in steps:
    g = whole(per_rank)
    out = one(feats_of(g))
    first = host(out) if first is None else first
    one.backward(dev(g['grad']), apply_lr=lr, emit=False)
  want = [layer_state(one, c) for c in range(2)]

  def rank(r, comm):
    layer = fc.DenseFeatures(train_columns(), DEV, coll=comm)
    assert layer.sharded == [True, True] and [t.capacity for t in layer.hash_tables] == [512, 512]
    outs = []
    for per_rank in steps:
      outs.append(host(layer(feats_of(per_rank[r]))))
      layer.backward(dev(per_rank[r]['grad']), apply_lr=lr, emit=False)
    torch.cuda.current_stream().synchronize()
    res = dict(first=outs[0], state=[layer_state(layer, c) for c in range(2)],
               failed=[t.failed() for t in layer.hash_tables])
    layer.close()
    return res

  res = run_world(world, rank)
  np.testing.assert_array_equal(np.concatenate([x['first'] for x in res]), first)
  for c in range(2):
    for r in range(world):
      assert all(owner(np.array([k]), world)[0] == r for k in res[r]['state'][c]) and res[r]['failed'][c] == 0
    got = merged([x['state'][c] for x in res])
    assert set(got) == set(want[c])
    m = Model([np.array(sorted(got), np.int64)], one.columns[c].dimension, 3 + c, SCALE)
    mag = np.zeros(m.w.shape, np.float64)
    for per_rank in steps:
      mag += world_grad_sums(m.uniq.size, m.w.shape[1], [
        (m.index(b['ids'][c]), b['grad'][:, :6] if c == 0 else b['grad'][:, 6:], b['splits'][c],
         one.columns[c].combiner) for b in per_rank])[1]
    assert_sums_close(np.stack([got[int(k)][0] for k in m.uniq]),
                      np.stack([want[c][int(k)][0] for k in m.uniq]).astype(np.float64),
                      np.abs(m.w) + lr * mag, err_msg=f'column {c}')


# ---- 6. a sharded hash sequence column ---------------------------------------------------------------------
def test_sharded_hash_sequence_column():
  rng = np.random.RandomState(51)
  world, B, T, dim, pad, lr = 2, 12, 4, 8, -3, 0.1
  pool = wide_keys(rng, 30)
  late = 424242                                  # occurs only past T
  batches = []
  for _ in range(world):
    lens = rng.randint(0, 7, size=B)
    lens[:3] = [0, T, 7]
    splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids = pool[rng.randint(0, pool.size, size=int(splits[-1]))]
    ids[splits[2] + 5] = late
    batches.append(dict(ids=ids, splits=splits, grad=rng.randn(B, T, dim).astype(F32)))
  make = lambda **kw: fc.HashSequenceEmbeddingColumn('hist', 512, dim, T, init_scale=SCALE, seed=9, **kw)   # noqa: E731
  all_ids = np.concatenate([b['ids'] for b in batches])
  all_sp = np.concatenate([batches[0]['splits'], batches[1]['splits'][1:] + batches[0]['splits'][-1]]).astype(np.int32)
  table = HashTable(512, dim, DEV, init_scale=SCALE, seed=9)
  hsl = HashSequenceLookup([table], T, pad_ids=pad)
  (want,), (want_len,) = hsl([dev(all_ids)], [dev(all_sp)])
  want, want_len = host(want), host(want_len)
  effective = np.unique(id_grid_ref(all_ids, all_sp, T, pad)[0])
  assert table.size() == effective.size and late not in effective and pad in effective

  def rank(r, comm):
    with pytest.raises(_lib.InvalidArgumentError) as e:
      fc.SequenceFeatures([make()], DEV, coll=comm)
    assert 'requires a pad_id' in str(e.value)
    layer = fc.SequenceFeatures([make(pad_id=pad)], DEV, coll=comm)
    b = batches[r]
    (out,), (ln,) = layer({'hist': (dev(b['ids']), dev(b['splits']))})
    assert tuple(out.shape) == (B, T, dim)
    out, ln = host(out), host(ln)
    t = layer.hash_tables[0]
    found = host(t.find(dev(np.array([late, pad], np.int64))))
    size = t.size()
    layer.backward([dev(b['grad'])], apply_lr=lr, emit=False)
    torch.cuda.current_stream().synchronize()
    res = dict(out=out, len=ln, found=found, size=size, state=layer_state(layer, 0), failed=t.failed())
    layer.close()
    return res

  res = run_world(world, rank)
  np.testing.assert_array_equal(np.concatenate([x['out'] for x in res]), want)
  np.testing.assert_array_equal(np.concatenate([x['len'] for x in res]), want_len)
  assert all(x['found'][0] == -1 and x['failed'] == 0 for x in res)
  assert sum(x['size'] for x in res) == effective.size
  assert res[pad % world]['found'][1] >= 0 and res[1 - pad % world]['found'][1] == -1
  got = merged([x['state'] for x in res])
  assert set(got) == set(effective.tolist())
  # the pad id's row collects the gradient of every padding position, of both ranks
  terms = np.concatenate([b['grad'][np.arange(T)[None, :] >= np.minimum(np.diff(b['splits']), T)[:, None]]
                          for b in batches]).astype(np.float64)
  terms = np.concatenate([terms] + [b['grad'].reshape(-1, dim)[id_grid_ref(b['ids'], b['splits'], T, 2 ** 62)[0] == pad]
                                    for b in batches])          # (the pad id among the data, if it is drawn)
  w0 = ref.init_rows([pad], dim, 9, SCALE)[0].astype(np.float64)
  assert terms.shape[0] > 10
  assert_sums_close(got[pad][0], w0 - lr * terms.sum(0), np.abs(w0) + lr * np.abs(terms).sum(0), err_msg='pad row')


def test_sequence_training_on_one_rank_equals_the_hand_composition(deterministic):   # pylint: disable=unused-argument,redefined-outer-name
  """SequenceFeatures with a hash column on one rank, in training: HashSequenceLookup + SequenceLookupGrad by hand on
  a table of 1024 slots against the layer's 64-slot table, which holds 50 keys after the first step (49 ids and the
  pad id) and grows: the grad object is rebuilt by the layer."""
  rng = np.random.RandomState(52)
  T, dim, pad, lr = 4, 8, -3, 0.1
  keys = pick_keys(rng, 60, [(50, 8), (60, 16), (60, 128)], extra=[pad])
  lens = np.array([4] * 12 + [0, 1, 3, 7] + [4] * 4)
  splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  n, B = int(splits[-1]), lens.size
  batches = [dict(ids=keys[1:50][np.arange(n) % 49], grad=rng.randn(B, T, dim).astype(F32)),
             dict(ids=keys[1:][(np.arange(n) * 7) % 59], grad=rng.randn(B, T, dim).astype(F32))]
  col = fc.HashSequenceEmbeddingColumn('hist', 64, dim, T, pad_id=pad, init_scale=SCALE, seed=9)
  layer = fc.SequenceFeatures([col], DEV, initial_accumulator_value=0.1)
  table = HashTable(1024, dim, DEV, init_scale=SCALE, seed=9)
  hsl = HashSequenceLookup([table], T, pad_ids=pad)
  accum = torch.full_like(table.table, 0.1)
  grad = SequenceLookupGrad(hsl, accums=[accum])
  grown = []
  for b in batches:
    (out,), (ln,) = layer({'hist': (dev(b['ids']), dev(splits))})
    (want,), (want_len,) = hsl([dev(b['ids'])], [dev(splits)])
    assert torch.equal(out, want) and torch.equal(ln, want_len) and tuple(out.shape) == (B, T, dim)
    res = layer.backward([dev(b['grad'])], apply_lr=lr, optimizer='adagrad')
    grad([dev(b['grad'])], apply_lr=lr, optimizer='adagrad')
    k = int(res[0][2].item())
    named = host(layer.hash_tables[0].keys)[host(res[0][0])[:k]]
    assert set(named.tolist()) == set(id_grid_ref(b['ids'], splits, T, pad)[0].tolist())
    grown.append(layer.maybe_grow())
  assert grown == [['hist'], []] and layer.hash_tables[0].capacity == 128 and layer.hash_tables[0].failed() == 0
  assert_same_by_key(layer_state(layer, 0), by_key(table, [table.table, accum]), 'sequence training')
  assert len(layer_state(layer, 0)) == table.size() > 50


# ---- 7. checkpoints across world sizes ---------------------------------------------------------------------
def ckpt_columns(cap=1024, slab=8):
  return [fc.EmbeddingColumn('b', 211, 6, 'sum'),
          fc.HashEmbeddingColumn('h0', cap, 6, 'mean', init_scale=SCALE, seed=3, expiring=True, slab_size=slab),
          fc.HashEmbeddingColumn('h1', cap, 16, 'sum', init_scale=SCALE, seed=4, expiring=True, slab_size=slab)]


def test_checkpoint_across_world_sizes(tmp_path, deterministic):   # pylint: disable=unused-argument,redefined-outer-name
  """Trained on 2 ranks, restored onto 1 rank and onto 2 ranks with other capacities and slab sizes.  The further
  step is compared bit for bit by key (row, accumulator, last_seen, freq) on both: the 2-rank restore against the
  layers that were saved, and the 1-rank restore, fed the ranks' batches concatenated in rank order, against the same
  -- with bwd_deterministic = 1 an owner sums requester 0's terms in id order, then requester 1's, which is the
  order of one table fed that concatenation (tests/test_gpu_sharded_hash.py holds the sharded step to it)."""
  rng = np.random.RandomState(61)
  world, B, lr = 2, 40, 0.1
  pools = [wide_keys(rng, 60), wide_keys(rng, 60)]
  steps = []
  for _ in range(3):
    per_rank = train_batches(rng, world, B, pools)
    for b in per_rank:
      b['b'] = rng.randint(0, 10 ** 6, size=B).astype(np.int64)
      b['grad'] = rng.randn(B, 28).astype(F32)
    steps.append(per_rank)
  prefix = str(tmp_path / 'ckpt')
  dense = rng.uniform(-1, 1, size=(211, 6)).astype(F32)

  def feats(b):
    return dict(feats_of(b), b=dev(b['b']))

  def state(layer):
    return dict(h=[layer_state(layer, c) for c in (1, 2)], b=host(layer.weights[0]), b_acc=host(layer.accums[0]))

  def step(layer, n, b):
    layer.set_step(n)
    layer(feats(b))
    layer.backward(dev(b['grad']), apply_lr=lr, optimizer='adagrad', emit=False)

  barrier = threading.Barrier(world)

  def train(r, comm):
    init = lambda col, rows, d: dev(dense[r::world].copy())   # noqa: E731
    layer = fc.DenseFeatures(ckpt_columns(), DEV, coll=comm, init=init, initial_accumulator_value=0.1)
    for n in (0, 1):
      step(layer, n + 1, steps[n][r])
    layer.save(prefix, barrier=barrier.wait)
    saved = state(layer)
    fresh = fc.DenseFeatures(ckpt_columns(cap=1500, slab=4), DEV, coll=comm, initial_accumulator_value=0.1)
    fresh.restore(prefix, barrier=barrier.wait)
    restored = state(fresh)
    for x in (layer, fresh):
      step(x, 3, steps[2][r])
    torch.cuda.current_stream().synchronize()
    res = dict(saved=saved, restored=restored, next=state(layer), next_restored=state(fresh))
    layer.close()
    fresh.close()
    return res

  res = run_world(world, train)
  index = set(hb.training.saver._read_index(prefix)['variables'])   # pylint: disable=protected-access
  assert 'h0_embedding/embedding_weights/part_1_of_2/items/keys' in index
  assert 'h1_embedding/embedding_weights/part_0_of_2/items/slot0' in index and 'b_embedding/embedding_weights' in index
  saved = [merged([x['saved']['h'][c] for x in res]) for c in range(2)]
  for c in range(2):
    assert len(saved[c]) > 50 and {len(v) for v in saved[c].values()} == {4}    # row, accum, last_seen, freq
    assert_same_by_key(merged([x['restored']['h'][c] for x in res]), saved[c], f'W = 2 restore, column {c}')
    assert_same_by_key(merged([x['next_restored']['h'][c] for x in res]), merged([x['next']['h'][c] for x in res]),
                       f'W = 2 further step, column {c}')
    for r in range(world):
      assert all(k % world == r for k in res[r]['restored']['h'][c])
      np.testing.assert_array_equal(res[r]['restored']['b'], res[r]['saved']['b'])
      np.testing.assert_array_equal(res[r]['restored']['b_acc'], res[r]['saved']['b_acc'])
      np.testing.assert_array_equal(res[r]['next_restored']['b'], res[r]['next']['b'])
  # one rank, another geometry again
  one = fc.DenseFeatures(ckpt_columns(cap=600, slab=16), DEV, initial_accumulator_value=0.1)
  one.restore(prefix)
  got = state(one)
  for c in range(2):
    assert_same_by_key(got['h'][c], saved[c], f'W = 1 restore, column {c}')
  for r in range(world):
    np.testing.assert_array_equal(got['b'][r::world], res[r]['saved']['b'])
    np.testing.assert_array_equal(got['b_acc'][r::world], res[r]['saved']['b_acc'])
  per_rank = steps[2]
  sp = np.concatenate([per_rank[0]['splits'][0], per_rank[1]['splits'][0][1:] + per_rank[0]['splits'][0][-1]])
  whole = dict(ids=[np.concatenate([b['ids'][c] for b in per_rank]) for c in range(2)], splits=[sp.astype(np.int32), None],
               b=np.concatenate([b['b'] for b in per_rank]), grad=np.concatenate([b['grad'] for b in per_rank]))
  step(one, 3, whole)
  after = state(one)
  for c in range(2):    # row, accumulator, last_seen and freq of every key
    assert_same_by_key(after['h'][c], merged([x['next']['h'][c] for x in res]), f'W = 1 further step, column {c}')
  # the other way round: a bucketed column of a hash column's name
  wrong = fc.DenseFeatures([fc.EmbeddingColumn('h0', 211, 6)], DEV)
  with pytest.raises(_lib.InvalidArgumentError) as e:
    wrong.restore(prefix)
  assert 'h0_embedding/embedding_weights' in str(e.value) and 'hash-keyed column' in str(e.value)
  # and a table too small for its keys raises import_items's own error
  tiny = fc.DenseFeatures(ckpt_columns(cap=32, slab=8), DEV, initial_accumulator_value=0.1)
  with pytest.raises(_lib.InvalidArgumentError) as e:
    tiny.restore(prefix)
  assert 'do not fit: the table is full' in str(e.value)


# ---- 8. train=False ----------------------------------------------------------------------------------------
def test_train_false_is_a_pure_find(tmp_path):
  rng = np.random.RandomState(71)
  pools = [wide_keys(rng, 40), wide_keys(rng, 40)]
  b = train_batches(rng, 1, 32, pools)[0]
  layer = fc.DenseFeatures(train_columns(), DEV, train=False)
  out = layer(feats_of(b))
  assert not host(out).any()
  assert [t.size() for t in layer.hash_tables] == [0, 0] and not any(host(t.counts).any() for t in layer.hash_tables)
  with pytest.raises(_lib.InvalidArgumentError) as e:
    layer.backward(torch.ones_like(out), apply_lr=0.1)
  assert 'train=False' in str(e.value)
  layer.save(str(tmp_path / 'empty'))           # tables without a key save and restore
  layer.restore(str(tmp_path / 'empty'))
  assert [t.size() for t in layer.hash_tables] == [0, 0]
  seq = fc.SequenceFeatures([fc.HashSequenceEmbeddingColumn('s', 64, 4, 3, pad_id=-1)], DEV, train=False)
  (o,), (ln,) = seq({'s': (dev(b['ids'][0]), dev(b['splits'][0]))})
  assert not host(o).any() and seq.hash_tables[0].size() == 0
  np.testing.assert_array_equal(host(ln), np.minimum(np.diff(b['splits'][0]), 3))
  with pytest.raises(_lib.InvalidArgumentError):
    seq.backward([torch.ones_like(o)], apply_lr=0.1)
