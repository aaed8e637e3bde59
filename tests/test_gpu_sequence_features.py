"""SequenceFeatures on the GPU: the layer against SequenceLookup / SequenceLookupGrad on one GPU, its
checkpoints, and in-process worlds of 1 and 3 ranks with one sharded column (with a pad id) and one
replicated column (zero padded)."""
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd.embedding import SequenceLookup, SequenceLookupGrad
from tests.support import sequence_ref as ref
from tests.support.tolerance import assert_sums_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
fc = hb.feature_column


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def _columns():
  return [fc.SequenceEmbeddingColumn('big', 3001, 16, 5, pad_id=2),
          fc.SequenceEmbeddingColumn('small', 40, 6, 3)]


def _batch(rng, cols, B):
  feats = {}
  for col in cols:
    lens = rng.randint(0, 2 * col.max_len + 2, size=B)
    lens[:3] = [0, col.max_len, col.max_len + 2]
    splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    feats[col.key] = (rng.randint(-10 ** 6, 10 ** 6, size=int(splits[-1])).astype(np.int64), splits)
  grads = [rng.randn(B, col.max_len, col.dimension).astype(F32) for col in cols]
  return feats, grads


def _dev_feats(feats):
  return {k: (dev(i), dev(s)) for k, (i, s) in feats.items()}


def _tables(rng, cols):
  return [rng.uniform(-1, 1, size=(c.num_buckets, c.dimension)).astype(F32) for c in cols]


def _init_from(cols, tables, world=1, rank=0):
  def init(c, rows, d):   # pylint: disable=unused-argument
    t = tables[cols.index(c)]
    return dev((t[rank::world] if rows != c.num_buckets else t).copy())
  return init


def _reference(cols, tables, feats):
  """SequenceLookup over the whole tables on one GPU."""
  lookup = SequenceLookup([dev(t) for t in tables], [c.num_buckets for c in cols],
                          max_lens=[c.max_len for c in cols], pad_ids=[c.pad_id for c in cols])
  f = _dev_feats(feats)
  outs, lengths = lookup([f[c.key][0] for c in cols], [f[c.key][1] for c in cols])
  return lookup, outs, lengths


def test_single_gpu_layer_equals_the_lookup_and_its_backward():
  rng = np.random.RandomState(1)
  cols = _columns()
  tables = _tables(rng, cols)
  feats, grads = _batch(rng, cols, 50)
  layer = fc.SequenceFeatures(cols, DEV, init=_init_from(cols, tables))
  assert layer.sharded == [False, False]
  outs, lengths = layer(_dev_feats(feats))
  lookup, want, want_len = _reference(cols, tables, feats)
  for c, col in enumerate(cols):
    assert tuple(outs[c].shape) == (50, col.max_len, col.dimension)
    assert torch.equal(outs[c], want[c]) and torch.equal(lengths[c], want_len[c])
  res = layer.backward([dev(g) for g in grads], apply_lr=0.1)
  ref_res = SequenceLookupGrad(lookup)([dev(g) for g in grads], apply_lr=0.1)
  for c, col in enumerate(cols):
    grid, _ = ref.grid_ref(*feats[col.key], col.num_buckets, col.max_len, col.pad_id)
    u, s, mag = ref.grad_ref(grid, grads[c], col.num_buckets)
    assert int(res[c][2].item()) == u.size == int(ref_res[c][2].item())
    want_t = tables[c].astype(np.float64)
    bound = np.abs(want_t)
    want_t[u] -= 0.1 * s
    bound[u] += 0.1 * mag
    assert_sums_close(host(layer.weights[c]), want_t, bound, err_msg=col.key)
    assert_sums_close(host(lookup.tables[c]), want_t, bound, err_msg=col.key + ' lookup')
    assert not np.array_equal(host(layer.weights[c]), tables[c])


def test_checkpoint_round_trip(tmp_path):
  rng = np.random.RandomState(2)
  cols = _columns()
  tables = _tables(rng, cols)
  feats, grads = _batch(rng, cols, 30)
  layer = fc.SequenceFeatures(cols, DEV, init=_init_from(cols, tables), initial_accumulator_value=0.1)
  layer(_dev_feats(feats))
  layer.backward([dev(g) for g in grads], apply_lr=0.1, optimizer='adagrad', emit=False)
  names = set(layer.variables())
  assert names == {f'{k}_embedding/embedding_weights{s}' for k in ('big', 'small') for s in ('', '/Adagrad')}
  prefix = str(tmp_path / 'ckpt')
  layer.save(prefix)
  other = fc.SequenceFeatures(cols, DEV, initial_accumulator_value=0.5)
  other.restore(prefix)
  for c in range(len(cols)):
    assert torch.equal(other.weights[c], layer.weights[c])
    assert torch.equal(other.accums[c], layer.accums[c])
    assert not torch.equal(layer.accums[c], torch.full_like(layer.accums[c], 0.1))


@pytest.mark.parametrize('world', [1, 3])
def test_sharded_and_replicated_columns_in_process_world(world):
  rng = np.random.RandomState(40 + world)
  cols = _columns()
  tables = _tables(rng, cols)
  B, lr = 48, 0.1
  data = [_batch(rng, cols, B) for _ in range(world)]
  comms = hb.distribute.Collective.local_world(world)
  results, errors = [None] * world, []

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        layer = fc.SequenceFeatures(cols, DEV, coll=comms[r], batch_size=B,
                                    init=_init_from(cols, tables, world, r))
        assert layer.sharded == [world > 1, False]
        outs, lengths = layer(_dev_feats(data[r][0]))
        res = layer.backward([dev(g) for g in data[r][1]], apply_lr=lr)
        torch.cuda.current_stream().synchronize()
        results[r] = ([host(o) for o in outs], [host(x) for x in lengths], [host(w) for w in layer.weights],
                      [(host(u)[:int(k.item())], host(g)[:int(k.item())]) for u, g, k in res])
        layer.close()
    except Exception as e:  # pylint: disable=broad-except
      errors.append((r, repr(e)))

  threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=45)
  assert not errors, errors
  # forward: every rank's outputs are the single-GPU result for its samples, bit for bit (fp32 wire)
  grids = []
  for r in range(world):
    _, want, want_len = _reference(cols, tables, data[r][0])
    for c in range(len(cols)):
      np.testing.assert_array_equal(results[r][0][c], host(want[c]))
      np.testing.assert_array_equal(results[r][1][c], host(want_len[c]))
    grids.append([ref.grid_ref(*data[r][0][col.key], col.num_buckets, col.max_len, col.pad_id)[0]
                  for col in cols])
  # the step: the whole world's batch on one GPU, and in float64
  for c, col in enumerate(cols):
    grid = np.concatenate([grids[r][c] for r in range(world)])
    g = np.concatenate([data[r][1][c] for r in range(world)])
    u, s, mag = ref.grad_ref(grid, g, col.num_buckets)
    want_t = tables[c].astype(np.float64)
    bound = np.abs(want_t)
    want_t[u] -= lr * s
    bound[u] += lr * mag
    if c == 0 or world == 1:
      # the (sharded) table was stepped: its shards, reassembled
      got = np.zeros_like(tables[c])
      if c == 0 and world > 1:
        for r in range(world):
          got[r::world] = results[r][2][c]
      else:
        got = results[0][2][c]
      assert_sums_close(got, want_t, bound, err_msg=f'{col.key} W {world}')
      assert not np.array_equal(got, tables[c])
      single = dev(tables[c])
      lookup = SequenceLookup([single], [col.num_buckets], max_lens=col.max_len, pad_ids=col.pad_id)
      SequenceLookupGrad(lookup)([dev(g)], apply_lr=lr, grids=[dev(grid)])
      assert_sums_close(host(single), want_t, bound, err_msg=f'{col.key} single GPU')
    else:
      # a replicated table at W > 1 is not stepped: every rank returns its IndexedSlices instead
      dense = np.zeros((col.num_buckets, col.dimension), np.float64)
      for r in range(world):
        np.testing.assert_array_equal(results[r][2][c], tables[c])
        rows, vals = results[r][3][c]
        np.add.at(dense, rows, vals.astype(np.float64))
      full = np.zeros_like(dense)
      full_mag = np.zeros_like(dense)
      full[u], full_mag[u] = s, mag
      assert_sums_close(dense, full, full_mag, err_msg=f'{col.key} slices')
  for cm in comms:
    cm.close()
