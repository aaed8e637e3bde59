"""16-bit hash columns in the feature-column layers on the GPU: DenseFeatures and SequenceFeatures over
HashEmbeddingColumn(dtype=) / HashSequenceEmbeddingColumn(dtype=) at W = 1 and W = 2 -- a forward, three stepping
backwards, maybe_grow, then save -> restore at the OTHER world size -- against the drivers built by hand
(HashGroupLookup + LowpLookupGrad, HashSequenceLookup + LowpSequenceLookupGrad, LowpShardedHashGroupLookup).
Everything is compared per key, bit for bit: slot numbers are not reproducible, gradients lie on the exact grid."""
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import feature_column as fc
from hybridbackend_amd.embedding import (HashGroupLookup, HashSequenceLookup, LowpLookupGrad, LowpSequenceLookupGrad,
                                         LowpShardedHashGroupLookup, ShardedSequenceLookup)
from tests.support import exact
from tests.support import hash_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
LOWP = [torch.bfloat16, torch.float16]
IDS = ['bf16', 'fp16']
DIMS, SEEDS, CAP, T = [6, 16], [3, 4], 256, [4, 3]
LR, ACC0 = 0.05, 0.1


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def bits16(t):
  return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def run_world(world, fn):
  if world == 1:
    return [fn(0, None)]
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
    t.join(timeout=60)
  for cm in comms:
    cm.close()
  assert not errors, errors
  return results


def by_key(tables, accums):
  """Per table {key: (row bits, accumulator row bits)}."""
  out = []
  for t, a in zip(tables, accums):
    keys = host(t.keys)
    live = np.nonzero(keys != hash_ref.EMPTY)[0]
    rows, acc = bits16(t.table), host(a).view(np.uint32)
    assert a.dtype == torch.float32 and t.table.dtype == t.dtype
    out.append({int(keys[s]): (rows[s].copy(), acc[s].copy()) for s in live})
  return out


def merged(states):
  out = [{} for _ in states[0]]
  for s in states:
    for c, d in enumerate(s):
      assert not set(d) & set(out[c])
      out[c].update(d)
  return out


def assert_same(got, want, what):
  for c, (g, w) in enumerate(zip(got, want)):
    assert set(g) == set(w) and len(w) > 10, f'{what}: column {c}: key sets differ ({len(g)} vs {len(w)})'
    for k in w:
      np.testing.assert_array_equal(g[k][0], w[k][0], err_msg=f'{what}: column {c} key {k}: row')
      np.testing.assert_array_equal(g[k][1], w[k][1], err_msg=f'{what}: column {c} key {k}: accumulator')


def batches(world, seed, B=24):
  rng = np.random.RandomState(seed)
  pools = [np.concatenate([rng.randint(-2 ** 62, 0, size=20, dtype=np.int64),
                           rng.randint(2 ** 40, 2 ** 62, size=20, dtype=np.int64)]) for _ in range(2)]
  out = []
  for _ in range(world):
    lens = rng.randint(0, 7, size=B)
    lens[:3] = (0, 4, 6)
    sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    out.append(dict(ids=[pools[0][rng.randint(0, 40, size=int(sp[-1]))], pools[1][rng.randint(0, 40, size=B)]], splits=sp))
  return out, rng


# ---- DenseFeatures ----------------------------------------------------------------------------------------------------
def dense_columns(dtype, cap=CAP):
  return [fc.HashEmbeddingColumn(f'h{c}', cap, DIMS[c], 'sum', init_scale=0.05, seed=SEEDS[c], dtype=dtype)
          for c in range(2)]


def dense_feats(b):
  return {'h0': (dev(b['ids'][0]), dev(b['splits'])), 'h1': dev(b['ids'][1])}


@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
@pytest.mark.parametrize('world', [1, 2])
def test_dense_features_equal_the_hand_built_drivers_and_restore_at_the_other_world_size(world, dtype, tmp_path):
  per_rank, rng = batches(world, 10 + world)
  B, width = 24, sum(DIMS)
  grads = [[exact.exact_grads(rng, (B, width), 6) for _ in range(world)] for _ in range(3)]
  prefix = str(tmp_path / 'ckpt')
  barrier = threading.Barrier(world)

  def rank(r, comm):
    layer = fc.DenseFeatures(dense_columns(dtype), DEV, coll=comm, initial_accumulator_value=ACC0)
    assert layer.hash_dtype == dtype and all(t.dtype == dtype for t in layer.hash_tables)
    assert all(a.dtype == torch.float32 for a in layer.accums)
    tables = [col.make_table(DEV, world) for col in dense_columns(dtype)]
    accums = [torch.full((t.capacity, t.dim), ACC0, dtype=torch.float32, device=DEV) for t in tables]
    b = per_rank[r]
    ids, sp = [dev(b['ids'][0]), dev(b['ids'][1])], [dev(b['splits']), None]
    if world == 1:
      assert isinstance(layer._hash_grad, LowpLookupGrad)   # pylint: disable=protected-access
      hgl = HashGroupLookup(tables, combiners='sum')
      step = LowpLookupGrad(hgl.lookup, accums)
    else:
      assert isinstance(layer._hash_sharded, LowpShardedHashGroupLookup)   # pylint: disable=protected-access
      drv = LowpShardedHashGroupLookup(tables, comm, combiners='sum', accums=accums, initial_accumulator_value=ACC0)

    def hand_forward():
      return torch.cat(list(hgl(ids, sp) if world == 1 else drv(ids, sp)), dim=1)

    same = True
    for k in range(3):
      got, want = layer(dense_feats(b)), hand_forward()
      same = same and torch.equal(got.view(torch.int32), want.view(torch.int32)) and bool(got.any())
      g = dev(grads[k][r])
      layer.backward(g, apply_lr=LR, optimizer='adagrad', emit=False)
      cols = [g[:, :DIMS[0]].contiguous(), g[:, DIMS[0]:].contiguous()]
      if world == 1:
        step(hgl.slots, cols, sp, apply_lr=LR, optimizer='adagrad')
      else:
        drv.backward(cols, apply_lr=LR, optimizer='adagrad')
    torch.cuda.current_stream().synchronize()
    stepped = (by_key(layer.hash_tables, layer.accums), by_key(tables, accums))
    # growth: the rows and the slots move with their keys, and the layer keeps working
    assert sorted(layer.maybe_grow(max_load=0.01)) == ['h0', 'h1']
    if world == 1:
      new = hgl.maybe_grow(max_load=0.01, slots=[[(a, ACC0)] for a in accums])
      accums = [n[0] for n in new]
    else:
      assert drv.maybe_grow(max_load=0.01) == [True, True]
      accums = list(drv.accums)
    got, want = layer(dense_feats(b)), hand_forward()
    same = same and torch.equal(got.view(torch.int32), want.view(torch.int32))
    grown = (by_key(layer.hash_tables, layer.accums), by_key(tables, accums))
    assert all(t.capacity > CAP // world for t in layer.hash_tables)
    layer.save(prefix, barrier=barrier.wait if world > 1 else None)
    layer.close()
    if world > 1:
      drv.close()
    return dict(same=same, stepped=stepped, grown=grown)

  res = run_world(world, rank)
  assert all(x['same'] for x in res), 'a forward differs from the hand-built driver'
  saved = merged([x['grown'][0] for x in res])
  assert_same(merged([x['stepped'][0] for x in res]), merged([x['stepped'][1] for x in res]), 'three steps')
  assert_same(saved, merged([x['grown'][1] for x in res]), 'after maybe_grow')
  assert_same(saved, merged([x['stepped'][0] for x in res]), 'maybe_grow moved a row or a slot')
  # restore at the other world size, into another geometry: nothing is cast, every key with its row and slot
  other = 3 - world
  barrier2 = threading.Barrier(other)

  def restore(r, comm):
    fresh = fc.DenseFeatures(dense_columns(dtype, cap=1024), DEV, coll=comm, initial_accumulator_value=ACC0)
    fresh.restore(prefix, barrier=barrier2.wait if other > 1 else None)
    state = by_key(fresh.hash_tables, fresh.accums)
    assert all(k % other == r for d in state for k in d)
    fresh.close()
    return state

  assert_same(merged(run_world(other, restore)), saved, f'restore onto {other} rank(s)')


# ---- SequenceFeatures -------------------------------------------------------------------------------------------------
def sequence_columns(dtype, pads, cap=CAP):
  return [fc.HashSequenceEmbeddingColumn(f's{c}', cap, DIMS[c], T[c], pad_id=pads[c], init_scale=0.05, seed=SEEDS[c],
                                         dtype=dtype) for c in range(2)]


def sequence_batches(world, seed, B=12):
  rng = np.random.RandomState(seed)
  pools = [np.concatenate([rng.randint(-2 ** 62, 0, size=15, dtype=np.int64),
                           rng.randint(2 ** 40, 2 ** 62, size=15, dtype=np.int64)]) for _ in range(2)]
  out = []
  for _ in range(world):
    ids, splits = [], []
    for c in range(2):
      lens = rng.randint(0, 7, size=B)
      lens[:3] = (0, T[c], 6)
      sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
      ids.append(pools[c][rng.randint(0, 30, size=int(sp[-1]))])
      splits.append(sp)
    out.append(dict(ids=ids, splits=splits))
  return out, rng


@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
@pytest.mark.parametrize('world', [1, 2])
def test_sequence_features_equal_the_hand_built_drivers_and_restore_at_the_other_world_size(world, dtype, tmp_path):
  per_rank, rng = sequence_batches(world, 30 + world)
  B = 12
  pads = [-1, None] if world == 1 else [None, None]       # W = 2: zero padding through the packed form
  grads = [[[exact.exact_grads(rng, (B, T[c], DIMS[c]), 6) for c in range(2)] for _ in range(world)] for _ in range(3)]
  prefix = str(tmp_path / 'ckpt')
  barrier = threading.Barrier(world)

  def rank(r, comm):
    layer = fc.SequenceFeatures(sequence_columns(dtype, pads), DEV, coll=comm, initial_accumulator_value=ACC0,
                                sharded_zero_padding=True)
    assert layer.hash_dtype == dtype and all(a.dtype == torch.float32 for a in layer.accums)
    tables = [col.make_table(DEV, world) for col in sequence_columns(dtype, pads)]
    accums = [torch.full((t.capacity, t.dim), ACC0, dtype=torch.float32, device=DEV) for t in tables]
    b = per_rank[r]
    ids, sp = [dev(i) for i in b['ids']], [dev(s) for s in b['splits']]
    feats = {f's{c}': (ids[c], sp[c]) for c in range(2)}
    if world == 1:
      assert isinstance(layer._hash_grad, LowpSequenceLookupGrad)   # pylint: disable=protected-access
      hsl = HashSequenceLookup(tables, T, pad_ids=pads)
      step = LowpSequenceLookupGrad(hsl, accums)
    else:
      assert isinstance(layer._hash_sharded, LowpShardedHashGroupLookup)   # pylint: disable=protected-access
      drv = LowpShardedHashGroupLookup(tables, comm, combiners='sum', accums=accums, initial_accumulator_value=ACC0)
      seq = ShardedSequenceLookup(drv, T)

    def hand_forward():
      return hsl(ids, sp) if world == 1 else seq(ids, sp)

    def forwards_agree():
      (got, glen), (want, wlen) = layer(feats), hand_forward()
      return all(torch.equal(a.view(torch.int32), x.view(torch.int32)) and torch.equal(p, q) and bool(a.any())
                 for a, x, p, q in zip(got, want, glen, wlen))

    same = True
    for k in range(3):
      same = same and forwards_agree()
      g = [dev(x) for x in grads[k][r]]
      layer.backward(g, apply_lr=LR, optimizer='adagrad', emit=False)
      if world == 1:
        step(g, apply_lr=LR, optimizer='adagrad')
      else:
        seq.backward(g, apply_lr=LR, optimizer='adagrad')
    torch.cuda.current_stream().synchronize()
    stepped = (by_key(layer.hash_tables, layer.accums), by_key(tables, accums))
    assert sorted(layer.maybe_grow(max_load=0.01)) == ['s0', 's1']
    if world == 1:
      new = hsl.maybe_grow(max_load=0.01, slots=[[(a, ACC0)] for a in accums])
      accums = [n[0] for n in new]
    else:
      assert drv.maybe_grow(max_load=0.01) == [True, True]
      accums = list(drv.accums)
    same = same and forwards_agree()
    grown = (by_key(layer.hash_tables, layer.accums), by_key(tables, accums))
    layer.save(prefix, barrier=barrier.wait if world > 1 else None)
    layer.close()
    if world > 1:
      drv.close()
    return dict(same=same, stepped=stepped, grown=grown)

  res = run_world(world, rank)
  assert all(x['same'] for x in res), 'a forward differs from the hand-built driver'
  saved = merged([x['grown'][0] for x in res])
  assert_same(merged([x['stepped'][0] for x in res]), merged([x['stepped'][1] for x in res]), 'three steps')
  assert_same(saved, merged([x['grown'][1] for x in res]), 'after maybe_grow')
  assert_same(saved, merged([x['stepped'][0] for x in res]), 'maybe_grow moved a row or a slot')
  other = 3 - world
  barrier2 = threading.Barrier(other)

  def restore(r, comm):
    fresh = fc.SequenceFeatures(sequence_columns(dtype, [None, None], cap=1024), DEV, coll=comm,
                                initial_accumulator_value=ACC0, sharded_zero_padding=True)
    fresh.restore(prefix, barrier=barrier2.wait if other > 1 else None)
    state = by_key(fresh.hash_tables, fresh.accums)
    assert all(k % other == r for d in state for k in d)
    fresh.close()
    return state

  assert_same(merged(run_world(other, restore)), saved, f'restore onto {other} rank(s)')
