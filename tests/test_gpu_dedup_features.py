"""DeduplicatedFeatures on the GPU: a layer with one plain and one user group against ONE DenseFeatures over all
columns fed the RESTORED ids (what the reference's restore_deduplicated_to_sparse hands the lookup).  The expand
is a bit copy of the inner block; forward, IndexedSlices, stepped tables and optimizer slots equal the restored
layer's bit for bit on the exact grid of tests/support/exact.py (every optimizer, three steps, also under
deterministic=True), and within tests/support/tolerance.py's bound on N(0,1) gradients with a clipping max_norm.
SequenceFeatures and hash-keyed groups, two ranks with a sharded user table, restore indexes outside [0, U) --
inputs the kernels are specified to survive -- and train=False."""
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from tests.support import exact
from tests.support.tolerance import assert_sums_close, dense_sums

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
fc = hb.feature_column
BIG = 64.0         # a power-of-two max_norm above every row of an exact table: the clip changes no bit
CLIP = 0.004       # N(0,1) case: below the norm of most rows of a uniform(-1e-2, 1e-2) table
LR = exact.EXACT_LR
OPTIMIZERS = {'sgd': {}, 'adagrad': dict(initial_accumulator_value=0.1), 'adam': dict(optimizer='adam'),
              'ftrl': dict(optimizer='ftrl'), 'rowwise_adagrad': dict(optimizer='rowwise_adagrad')}


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


@pytest.fixture(params=[0, 1], ids=['default', 'deterministic'])
def deterministic(request):
  old = _lib.set_option('bwd_deterministic', request.param)
  yield request.param
  _lib.set_option('bwd_deterministic', old)


def plain_columns():
  return [fc.EmbeddingColumn('p0', 53, 8, 'sum'), fc.EmbeddingColumn('p1', 41, 5, 'mean')]


def user_columns(max_norm=BIG):
  return [fc.EmbeddingColumn('u_one', 47, 16, 'mean'), fc.EmbeddingColumn('u_sum', 43, 6, 'sum'),
          fc.EmbeddingColumn('u_mean', 37, 4, 'mean'), fc.EmbeddingColumn('u_sqrtn', 31, 8, 'sqrtn'),
          fc.EmbeddingColumn('u_clip', 29, 8, 'sum', max_norm=max_norm),
          fc.EmbeddingColumn('u_w', 23, 4, 'sum', weight_feature_key='u_w_weights')]


RAGGED = {'p1': 'mean', 'u_sum': 'sum', 'u_mean': 'mean', 'u_sqrtn': 'sqrtn', 'u_w': 'sum'}


def column_feature(rng, col, n):
  """(ids, splits | None, weights | None) of n segments: lengths up to 4 from the combiner's exact set."""
  if col.key not in RAGGED:
    return rng.randint(0, 2 ** 40, size=n).astype(np.int64), None, None
  lens = exact.snap_lengths(rng.randint(0, 5, size=n), RAGGED[col.key])
  splits = exact.splits_of(lens)
  ids = rng.randint(0, 2 ** 40, size=int(splits[-1])).astype(np.int64)
  w = exact.exact_weights(rng, splits, ids.size, 'sum') if col.weight_feature_key else None
  return ids, splits, w


def restore(feature, idx):
  """What the reference hands the lookup: every sample's copy of its key's segment."""
  ids, splits, w = feature
  if splits is None:
    return ids[idx], None, None
  parts = [np.arange(splits[u], splits[u + 1]) for u in idx]
  at = np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
  return ids[at], exact.splits_of(np.diff(splits)[idx]), None if w is None else w[at]


def covering_idx(rng, n, n_keys, dtype=np.int64):
  """Every key named at least once (a key nobody names is stepped with a zero gradient by the layer underneath,
  which a stateful optimizer notices and the restored layer cannot reproduce), the rest random, shuffled."""
  idx = np.concatenate([np.arange(n_keys), rng.randint(0, n_keys, size=n - n_keys)])
  rng.shuffle(idx)
  return idx.astype(dtype)


def as_features(cols, feats, out=None):
  out = {} if out is None else out
  for col in cols:
    ids, splits, w = feats[col.key]
    out[col.key] = dev(ids) if splits is None else (dev(ids), dev(splits))
    if w is not None:
      out[col.weight_feature_key] = dev(w)
  return out


class Batch:
  def __init__(self, rng, n, n_keys, idx_dtype=np.int64, idx=None):
    self.n, self.n_keys = n, n_keys
    self.idx = covering_idx(rng, n, n_keys, idx_dtype) if idx is None else idx
    self.plain = {c.key: column_feature(rng, c, n) for c in plain_columns()}
    self.user = {c.key: column_feature(rng, c, n_keys) for c in user_columns()}
    ok = (self.idx >= 0) & (self.idx < n_keys)
    assert ok.all() or idx is not None
    self.restored = dict(self.plain)
    if ok.all():
      self.restored.update({k: restore(f, self.idx) for k, f in self.user.items()})

  def dedup_features(self):
    f = as_features(plain_columns(), self.plain)
    as_features(user_columns(), self.user, f)
    f['user_idx'] = dev(self.idx)
    return f

  def restored_features(self):
    return as_features(plain_columns() + user_columns(), self.restored)

  def value_bits(self):
    """The budget, asserted on the RESTORED ids: the fewest bits any column leaves for gradient values."""
    bits = []
    for col in plain_columns() + user_columns():
      ids, splits, w = self.restored[col.key]
      comb = col.combiner
      factor = exact.factor_bits(comb, 4, weighted=w is not None)
      bits.append(exact.exact_terms_budget(ids % col.num_buckets, factor, case=col.key))
    return min(min(bits), 6)


def exact_init(seed):
  def init(col, rows, device):
    rng = np.random.RandomState(seed + sum(map(ord, col.key)))
    return dev(exact.exact_tables(rng, col.num_buckets, col.dimension)).to(device)
  return init


def uniform_init(seed):
  def init(col, rows, device):
    rng = np.random.RandomState(seed + sum(map(ord, col.key)))
    return dev(rng.uniform(-1e-2, 1e-2, size=(col.num_buckets, col.dimension)).astype(F32)).to(device)
  return init


def make_layers(init, okw, max_norm=BIG, train=True):
  dedup = fc.DeduplicatedFeatures(fc.DenseFeatures(plain_columns(), DEV, init=init, **okw),
                                  {'user_idx': fc.DenseFeatures(user_columns(max_norm), DEV, init=init, **okw)},
                                  train=train)
  restored = fc.DenseFeatures(plain_columns() + user_columns(max_norm), DEV, init=init, **okw)
  return dedup, restored


def state(layer, c):
  out = [layer.weights[c]]
  for name in ('accums', 'moments', 'ftrl_slots', 'row_accums'):
    slots = getattr(layer, name, None)
    if slots is not None:
      out += list(slots[c]) if isinstance(slots[c], (tuple, list)) else [slots[c]]
  return [host(x) for x in out]


def dedup_states(dedup):
  return [state(layer, c) for layer in dedup.layers for c in range(len(layer.columns))]


def dense_slices(slices, cols):
  out = []
  for (rows, grads, n), col in zip(slices, cols):
    k = int(n.item())
    d = np.zeros((col.num_buckets, col.dimension), F32)
    d[host(rows)[:k]] = host(grads)[:k]
    out.append(d)
  return out


def assert_states_equal(dedup, restored, what):
  got, n = dedup_states(dedup), len(restored.columns)
  assert len(got) == n
  for c in range(n):
    want = state(restored, c)
    assert len(got[c]) == len(want)
    for k, (a, b) in enumerate(zip(got[c], want)):
      exact.assert_bits_equal(a, b, f'{what}: column {restored.columns[c].key}, tensor {k}')


def assert_expand_is_a_copy(dedup, block, batch):
  """The block against the inner layers' own outputs of the same features, row for row."""
  plain, user = dedup.layers
  feats = batch.dedup_features()
  inner = host(user(feats))
  exact.assert_bits_equal(host(block[:, :plain.width]), host(plain(feats)), 'plain block')
  exact.assert_bits_equal(host(block[:, plain.width:]), inner[batch.idx], 'expanded block')
  assert block.shape == (batch.n, plain.width + user.width) and block.stride(0) % 4 == 0


# ---- forward and backward on the exact grid: bit for bit -------------------------------------------------------
@pytest.mark.parametrize('optimizer', list(OPTIMIZERS))
@pytest.mark.parametrize('n,n_keys', [(150, 37), (60, 60)])
def test_training_equals_the_restored_layer_bit_for_bit(optimizer, n, n_keys, deterministic):   # pylint: disable=unused-argument,redefined-outer-name
  rng = np.random.RandomState(n + len(optimizer))
  dedup, restored = make_layers(exact_init(7), OPTIMIZERS[optimizer])
  assert [c.key for c in dedup.columns] == [c.key for c in restored.columns]
  assert dedup.width == restored.width == 59 and dedup.offsets == {'user_idx': 13}   # (13: the 4-byte path)
  for step in range(3):
    batch = Batch(rng, n, n_keys, (np.int64, np.int32)[step % 2])
    block, sequences = dedup(batch.dedup_features())
    assert sequences == {}
    want = restored(batch.restored_features())
    if step == 0:
      assert_expand_is_a_copy(dedup, block, batch)
      dedup(batch.dedup_features())                       # (the copy check ran the inner layers: run the step's again)
      exact.assert_bits_equal(host(block), host(want), 'forward on exact tables')
    assert_sums_close(host(block), host(want).astype(np.float64), np.abs(host(want)), err_msg=f'forward {step}')
    grad = dev(exact.exact_grads(rng, (n, 59), batch.value_bits()))
    kw = dict(apply_lr=LR, optimizer=optimizer)
    got = dedup.backward(grad, **kw)
    ref = restored.backward(grad, **kw)
    for c, (a, b) in enumerate(zip(dense_slices(got, dedup.columns), dense_slices(ref, restored.columns))):
      exact.assert_bits_equal(a, b, f'step {step}: IndexedSlices of {restored.columns[c].key}')
    assert_states_equal(dedup, restored, f'{optimizer} step {step}')
    assert dedup.indexes['user_idx'].invalid_count() == 0


def test_normal_gradients_and_a_clipping_max_norm_within_the_bound():
  rng = np.random.RandomState(3)
  n, n_keys, lr = 150, 37, 0.1
  dedup, restored = make_layers(uniform_init(5), {}, max_norm=CLIP)
  before = [s[0].copy() for s in dedup_states(dedup)]
  batch = Batch(rng, n, n_keys)
  block, _ = dedup(batch.dedup_features())
  want = host(restored(batch.restored_features()))
  assert_expand_is_a_copy(dedup, block, batch)
  dedup(batch.dedup_features())
  assert_sums_close(host(block), want.astype(np.float64), np.abs(want), err_msg='forward')
  g = rng.randn(n, 59).astype(F32)
  got, wg = dedup.backward(dev(g), apply_lr=lr, weight_grads=True)
  ref, wr = restored.backward(dev(g), apply_lr=lr, weight_grads=True)
  a, b = dense_slices(got, dedup.columns), dense_slices(ref, restored.columns)
  after_d, after_r = [s[0] for s in dedup_states(dedup)], [state(restored, c)[0] for c in range(8)]
  for c, col in enumerate(restored.columns):
    # sum|terms| of a row: every sample's |gradient| that reaches it, through the restored ids
    ids, splits, w = batch.restored[col.key]
    off = restored.offsets[c]
    terms = np.abs(exact.id_terms(g[:, off:off + col.dimension], splits, col.combiner, w))
    if col.max_norm:
      # through the clip an element's term is bounded by the gradient row's NORM, not by its own element
      terms = np.broadcast_to(np.linalg.norm(terms, axis=1, keepdims=True), terms.shape)
    _, mag = dense_sums(a[c].shape, ids % col.num_buckets, terms)
    assert_sums_close(a[c], b[c].astype(np.float64), mag, err_msg=f'IndexedSlices of {col.key}')
    assert_sums_close(after_d[c], after_r[c].astype(np.float64), np.abs(before[c]) + lr * mag,
                      err_msg=f'stepped table of {col.key}')
    assert (after_d[c] != before[c]).any()
  # the weight gradient of a key's id is the sum of its copies'
  assert set(wg) == set(wr) == {'u_w_weights'}
  _, splits, _ = batch.user['u_w']
  copies = np.concatenate([np.arange(splits[u], splits[u + 1]) for u in batch.idx]).astype(np.int64)
  want_w, mag_w = dense_sums((int(splits[-1]),), copies, host(wr['u_w_weights']))
  assert_sums_close(host(wg['u_w_weights']), want_w, mag_w, err_msg='weight gradient')
  assert mag_w.any()


# ---- a SequenceFeatures group ------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad_id', [None, 0])
def test_a_sequence_group_equals_the_restored_sequence_features(pad_id, deterministic):   # pylint: disable=unused-argument,redefined-outer-name
  rng = np.random.RandomState(17)
  n, n_keys, T = 150, 37, 4
  cols = lambda: [fc.SequenceEmbeddingColumn('s0', 45, 6, T, pad_id=pad_id),   # noqa: E731
                  fc.SequenceEmbeddingColumn('s1', 33, 4, T, pad_id=pad_id)]
  init = exact_init(23)
  dedup = fc.DeduplicatedFeatures(None, {'user_idx': fc.SequenceFeatures(cols(), DEV, init=init)})
  restored = fc.SequenceFeatures(cols(), DEV, init=init)
  for step in range(2):
    idx = covering_idx(rng, n, n_keys)
    feats = {}
    for c in cols():
      splits = exact.splits_of(rng.randint(0, 7, size=n_keys))             # longer than T among them
      feats[c.key] = (rng.randint(0, 2 ** 40, size=int(splits[-1])).astype(np.int64), splits, None)
    rest = {k: restore(f, idx) for k, f in feats.items()}
    f = {k: (dev(v[0]), dev(v[1])) for k, v in feats.items()}
    f['user_idx'] = dev(idx)
    block, sequences = dedup(f)
    assert block is None and list(sequences) == ['user_idx']
    outs, lengths = sequences['user_idx']
    want_o, want_l = restored({k: (dev(v[0]), dev(v[1])) for k, v in rest.items()})
    grads = []
    for c, col in enumerate(cols()):
      assert outs[c].shape == (n, T, col.dimension) and lengths[c].dtype == torch.int32
      exact.assert_bits_equal(host(outs[c]), host(want_o[c]), f'outputs of {col.key}')
      assert host(lengths[c]).tolist() == host(want_l[c]).tolist()
      # the budget on the restored ids a position reads (with a pad id its row collects the padding too)
      ids, splits, _ = rest[col.key]
      read = np.concatenate([ids[splits[b]:splits[b] + T][:splits[b + 1] - splits[b]] for b in range(n)])
      pads = n * T - read.size if pad_id is not None else 0
      rows = np.concatenate([read % col.num_buckets, np.full(pads, pad_id or 0, np.int64)])
      grads.append(dev(exact.exact_grads(rng, (n, T, col.dimension), min(exact.exact_terms_budget(rows, 0), 6))))
    got = dedup.backward(None, {'user_idx': grads}, apply_lr=LR)
    ref = restored.backward(grads, apply_lr=LR)
    for c, (a, b) in enumerate(zip(dense_slices(got, dedup.columns), dense_slices(ref, restored.columns))):
      exact.assert_bits_equal(a, b, f'step {step}: IndexedSlices of column {c}')
    for c in range(2):
      exact.assert_bits_equal(host(dedup.layers[0].weights[c]), host(restored.weights[c]), f'stepped table {c}')


# ---- a hash-keyed group on one rank ------------------------------------------------------------------------------
def by_key(table):
  keys = host(table.keys)
  rows = host(table.table)
  live = keys > -2 ** 63 + 1            # (neither the empty nor the tombstone sentinel)
  return {int(k): rows[s].copy() for s, k in enumerate(keys) if live[s]}


def test_a_hash_keyed_group_on_one_rank():
  rng = np.random.RandomState(29)
  n, n_keys = 150, 37
  cols = lambda: [fc.HashEmbeddingColumn('h0', 1024, 6, 'mean', init_scale=0.05, seed=3),   # noqa: E731
                  fc.HashEmbeddingColumn('h1', 1024, 16, 'sum', init_scale=0.05, seed=4)]
  dedup = fc.DeduplicatedFeatures(None, {'user_idx': fc.DenseFeatures(cols(), DEV)})
  restored = fc.DenseFeatures(cols(), DEV)
  pool = rng.randint(-2 ** 62, 2 ** 62, size=90).astype(np.int64)
  for step in range(2):
    idx = covering_idx(rng, n, n_keys)
    lens = exact.snap_lengths(rng.randint(0, 5, size=n_keys), 'mean')
    feats = {'h0': (pool[rng.randint(0, 90, size=int(lens.sum()))], exact.splits_of(lens), None),
             'h1': (pool[rng.randint(0, 90, size=n_keys)], None, None)}
    rest = {k: restore(f, idx) for k, f in feats.items()}
    f = as_features(cols(), feats)
    f['user_idx'] = dev(idx)
    block, _ = dedup(f)
    want = host(restored(as_features(cols(), rest)))
    assert_sums_close(host(block), want.astype(np.float64), np.abs(want), err_msg='forward')
    bits = min(exact.exact_terms_budget(rest['h0'][0], exact.factor_bits('mean', 4)),
               exact.exact_terms_budget(rest['h1'][0], 0), 6)
    grad = dev(exact.exact_grads(rng, (n, 22), bits))
    dedup.backward(grad, apply_lr=LR)
    restored.backward(grad, apply_lr=LR)
    for c in range(2):
      got, ref = by_key(dedup.layers[0].hash_tables[c]), by_key(restored.hash_tables[c])
      assert set(got) == set(ref) and len(got) > 0
      for k in ref:
        exact.assert_bits_equal(got[k], ref[k], f'step {step}: column {c}, key {k}')


# ---- two ranks, one sharded user table ---------------------------------------------------------------------------
def run_world(world, fn):
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


def test_two_ranks_with_a_sharded_user_table():
  world, n, n_keys = 2, 150, 37
  p_cols = lambda: [fc.EmbeddingColumn('p0', 53, 8, 'sum')]   # noqa: E731
  u_cols = lambda: [fc.EmbeddingColumn('u_big', 1009, 16, 'mean'), fc.EmbeddingColumn('u_small', 31, 4, 'sum')]   # noqa: E731
  tables = {c.key: exact.exact_tables(np.random.RandomState(31 + k), c.num_buckets, c.dimension)
            for k, c in enumerate(p_cols() + u_cols())}
  rng = np.random.RandomState(37)
  batches = []
  for r in range(world):
    idx = covering_idx(rng, n, n_keys)
    lens = exact.snap_lengths(rng.randint(0, 5, size=n_keys), 'mean')
    user = {'u_big': (rng.randint(0, 2 ** 40, size=int(lens.sum())).astype(np.int64), exact.splits_of(lens), None),
            'u_small': (rng.randint(0, 2 ** 40, size=n_keys).astype(np.int64), None, None)}
    plain = {'p0': (rng.randint(0, 2 ** 40, size=n).astype(np.int64), None, None)}
    batches.append((idx, plain, user, {k: restore(f, idx) for k, f in user.items()}))
  # the budget over BOTH ranks' restored ids: the sharded table sums them all
  big = np.concatenate([b[3]['u_big'][0] for b in batches]) % 1009
  bits = min(exact.exact_terms_budget(big, exact.factor_bits('mean', 4)), 6)
  grads = [exact.exact_grads(rng, (n, 28), bits) for _ in range(world)]

  def run(which):
    def rank(r, comm):
      def init(col, rows, device):
        t = tables[col.key]
        return dev(t[r::world].copy() if rows != col.num_buckets else t).to(device)
      idx, plain, user, rest = batches[r]
      if which == 'dedup':
        layer = fc.DeduplicatedFeatures(
          fc.DenseFeatures(p_cols(), DEV, comm, batch_size=n, init=init),
          {'user_idx': fc.DenseFeatures(u_cols(), DEV, comm, batch_size=n, init=init)})
        assert layer.layers[1].sharded == [True, False]
        f = as_features(p_cols(), plain)
        as_features(u_cols(), user, f)
        f['user_idx'] = dev(idx)
        block, _ = layer(f)
        layer.backward(dev(grads[r]), apply_lr=LR)
        weights = [w for inner in layer.layers for w in inner.weights]
      else:
        layer = fc.DenseFeatures(p_cols() + u_cols(), DEV, comm, batch_size=n, init=init)
        assert layer.sharded == [False, True, False]
        f = as_features(p_cols(), plain)
        block = layer(as_features(u_cols(), rest, f))
        layer.backward(dev(grads[r]), apply_lr=LR)
        weights = layer.weights
      torch.cuda.current_stream().synchronize()
      out = (host(block), [host(w) for w in weights])
      layer.close()
      return out
    return run_world(world, rank)
  got, ref = run('dedup'), run('restored')
  for r in range(world):
    exact.assert_bits_equal(got[r][0], ref[r][0], f'rank {r}: forward')
    for c in range(3):
      exact.assert_bits_equal(got[r][1][c], ref[r][1][c], f'rank {r}: table {c}')
    assert (got[r][1][1] != tables['u_big'][r::world]).any()     # the sharded table was stepped


# ---- restore indexes outside [0, U), and train=False -------------------------------------------------------------
def test_an_out_of_range_restore_index_gives_a_zero_row_and_steps_nothing():
  rng = np.random.RandomState(41)
  n, n_keys = 150, 37
  dedup, _ = make_layers(exact_init(7), {})
  before = [s[0].copy() for s in dedup_states(dedup)]
  # every sample names no key: the user block is zero and the user tables do not move
  idx = np.resize(np.asarray([-1, n_keys, 2 ** 40, -2 ** 63], np.int64), n)
  batch = Batch(rng, n, n_keys, idx=idx)
  block, _ = dedup(batch.dedup_features())
  bits = lambda t: np.ascontiguousarray(host(t)).view(np.uint32)   # noqa: E731
  assert not bits(block[:, 13:]).any() and host(block[:, :13]).any()
  assert dedup.indexes['user_idx'].invalid_count() == n
  slices = dense_slices(dedup.backward(dev(exact.exact_grads(rng, (n, 59), 6)), apply_lr=LR), dedup.columns)
  after = [s[0] for s in dedup_states(dedup)]
  for c in range(2, 8):
    exact.assert_bits_equal(after[c], before[c], f'user table {c - 2}')
    assert not slices[c].any()
  assert (after[0] != before[0]).any()
  # some samples name no key: their rows are zero, the others are copies, and the gradient of the former is dropped
  idx = covering_idx(rng, n, n_keys)
  bad = rng.choice(n, size=20, replace=False)
  idx[bad] = np.resize(np.asarray([-1, n_keys, 2 ** 40], np.int64), 20)
  batch = Batch(rng, n, n_keys, idx=idx)
  feats = batch.dedup_features()
  block, _ = dedup(feats)
  assert dedup.indexes['user_idx'].invalid_count() == 20
  inner = host(dedup.layers[1](feats))
  ok = (idx >= 0) & (idx < n_keys)
  exact.assert_bits_equal(host(block[:, 13:])[ok], inner[idx[ok]], 'valid rows')
  assert not bits(block[:, 13:])[~ok].any()
  dedup(feats)
  g = exact.exact_grads(rng, (n, 59), 6)
  a = dense_slices(dedup.backward(dev(g)), dedup.columns)
  g[~ok, 13:] = 1e30                                         # what the dropped samples carry reaches nothing
  dedup(feats)
  b = dense_slices(dedup.backward(dev(g)), dedup.columns)
  for c in range(8):
    exact.assert_bits_equal(a[c], b[c], f'column {c}')
    assert a[c].any()


def test_train_false_builds_no_index():
  rng = np.random.RandomState(43)
  dedup, restored = make_layers(exact_init(7), {}, train=False)
  batch = Batch(rng, 60, 20)
  block, _ = dedup(batch.dedup_features())
  assert dedup.indexes == {}
  exact.assert_bits_equal(host(block), host(restored(batch.restored_features())), 'forward')
  with pytest.raises(hb.InvalidArgumentError, match='train=False'):
    dedup.backward(block)
  with pytest.raises(hb.InvalidArgumentError, match='DenseFeatures or a SequenceFeatures'):
    fc.DeduplicatedFeatures(None, {'user_idx': object()})
  trained, _ = make_layers(exact_init(7), {})
  with pytest.raises(hb.InvalidArgumentError, match='run the forward first'):
    trained.backward(block)
  with pytest.raises(hb.InvalidArgumentError, match='the plain columns hold 60 samples, the restore indexes 59'):
    f = batch.dedup_features()
    f['user_idx'] = f['user_idx'][:-1]
    trained(f)
