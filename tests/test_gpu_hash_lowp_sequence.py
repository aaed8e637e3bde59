"""Hash-keyed sequence lookups over 16-bit tables on the GPU: HashSequenceLookup over tables that are 16-bit throughout
equals the fp32 object over the upcast twin, bit for bit; three steps of LowpSequenceLookupGrad equal
tests/support/lowp_ref.py applied per key to the exact sums (the pad id's row collects the gradient of every padding
position); launch() repeats the bits; ShardedSequenceLookup takes the sharded 16-bit driver unchanged, in the packed
form and over the pad-id grid."""
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (HashSequenceLookup, HashTable, LowpGroupLookup, LowpSequenceLookupGrad,
                                         LowpShardedHashGroupLookup, ShardedHashGroupLookup, ShardedSequenceLookup,
                                         sequence_id_grid)
from tests.support import exact
from tests.support import hash_ref
from tests.support import lowp_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
BF, HF = torch.bfloat16, torch.float16
NAME = {BF: ref.BF16, HF: ref.FP16}
DIMS, SEEDS, T = [16, 6], [3, 4], [4, 3]
LR = 0.05


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def bits16(t):
  return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def make_tables(dtypes, **kw):
  return [HashTable(256, DIMS[c], DEV, slab_size=8, init_scale=0.05, seed=SEEDS[c], dtype=d, **kw)
          for c, d in enumerate(dtypes)]


def batch(seed, B=9):
  """Two columns of B samples with lengths 0 .. 6 (T = 4 and 3: truncated, exact and short samples)."""
  rng = np.random.RandomState(seed)
  ids, splits = [], []
  for c in range(2):
    lens = rng.randint(0, 7, size=B)
    lens[:3] = (0, T[c], 6)
    sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    pool = rng.randint(-2 ** 62, 2 ** 62, size=25, dtype=np.int64)
    ids.append(pool[rng.randint(0, 25, size=int(sp[-1]))])
    splits.append(sp)
  return ids, splits, rng


def effective(ids, sp, t_max, pad_id):
  """Per position b * T + t: the key, or None where the position holds nothing."""
  out = []
  for b in range(sp.size - 1):
    n = min(int(sp[b + 1] - sp[b]), t_max)
    out += [int(x) for x in ids[sp[b]:sp[b] + n]] + [pad_id] * (t_max - n)
  return out


def upcast_twins(tables):
  twins = []
  for t in tables:
    u = HashTable(t.capacity, t.dim, DEV, slab_size=t.slab_size, init_scale=t.init_scale, seed=t.seed)
    keys, rows = t.items()
    u.load(keys, rows.float())
    twins.append(u)
  return twins


@pytest.mark.parametrize('pad_ids', [None, [-1, 7]], ids=['nopad', 'pad'])
@pytest.mark.parametrize('dtypes', [[BF, HF], [HF, BF]], ids=['bf16-fp16', 'fp16-bf16'])
def test_forward_equals_the_fp32_object_over_the_upcast_twin_and_launch_repeats_the_bits(dtypes, pad_ids):
  ids, splits, _ = batch(5)
  tables = make_tables(dtypes)
  hsl = HashSequenceLookup(tables, T, pad_ids=pad_ids)
  assert isinstance(hsl.plain_lookup(), LowpGroupLookup)
  d_ids, d_sp = [dev(i) for i in ids], [dev(s) for s in splits]
  outs, lengths = hsl(d_ids, d_sp)
  torch.cuda.synchronize()
  first = [host(o).copy() for o in outs]
  for c in range(2):
    assert outs[c].dtype == torch.float32 and tuple(outs[c].shape) == (9, T[c], DIMS[c])
    np.testing.assert_array_equal(host(lengths[c]), np.minimum(np.diff(splits[c]), T[c]))
    keys = effective(ids[c], splits[c], T[c], None if pad_ids is None else pad_ids[c])
    stored = np.unique(np.array([k for k in keys if k is not None], np.int64))
    assert tables[c].size() == stored.size and tables[c].failed() == 0
    # every position: the cast start row of its key, upcast; nothing: a zero row
    want = np.zeros((len(keys), DIMS[c]), F32)
    have = np.array([k is not None for k in keys])
    start = hash_ref.init_rows(np.array([k for k in keys if k is not None], np.int64), DIMS[c], SEEDS[c], 0.05)
    want[have] = torch.from_numpy(start).to(dtypes[c]).float().numpy()
    np.testing.assert_array_equal(first[c].reshape(-1, DIMS[c]).view(np.uint32), want.view(np.uint32))
    # the ids past T are in no table
    past = np.concatenate([ids[c][splits[c][b] + T[c]:splits[c][b + 1]] for b in range(9)])
    past = np.setdiff1d(past, stored)
    assert past.size, 'the batch has no id that occurs only past T: draw another'
    assert (host(tables[c].find(dev(past))) == -1).all()
  # the fp32 object over the upcast twin
  f32 = HashSequenceLookup(upcast_twins(tables), T, pad_ids=pad_ids, train=False)
  want, _ = f32(d_ids, d_sp)
  for c in range(2):
    np.testing.assert_array_equal(first[c].view(np.uint32), host(want[c]).view(np.uint32))
  # launch(): both launches again on the bound tensors, the same bits, nothing new in the tables
  sizes = [t.size() for t in tables]
  for o in outs:
    o.fill_(7.0)
  hsl.launch()
  torch.cuda.synchronize()
  for c in range(2):
    np.testing.assert_array_equal(host(outs[c]).view(np.uint32), first[c].view(np.uint32))
  assert [t.size() for t in tables] == sizes
  # a captured graph replays them
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  g = torch.cuda.CUDAGraph()
  with torch.cuda.stream(side):
    with torch.cuda.graph(g, stream=side):
      hsl.launch()
  torch.cuda.synchronize()
  for o in outs:
    o.fill_(7.0)
  g.replay()
  torch.cuda.synchronize()
  for c in range(2):
    np.testing.assert_array_equal(host(outs[c]).view(np.uint32), first[c].view(np.uint32))


@pytest.mark.parametrize('optimizer,rounding,dtypes', [('sgd', 'nearest', [BF, HF]), ('sgd', 'stochastic', [BF, BF]),
                                                       ('rowwise_adagrad', 'nearest', [HF, BF])])
def test_three_steps_equal_the_restatement_per_key(optimizer, rounding, dtypes):
  ids, splits, rng = batch(11)
  pad_ids = [-1, None]                                   # column 0 pads with an id, column 1 with nothing
  tables = make_tables(dtypes, expiring=True)
  for t in tables:
    t.set_step(1)
  hsl = HashSequenceLookup(tables, T, pad_ids=pad_ids)
  slots0 = [np.random.RandomState(3 + c).uniform(0.1, 0.9, size=(t.capacity, 1)).astype(F32)
            for c, t in enumerate(tables)] if optimizer == 'rowwise_adagrad' else None
  slots = [dev(s) for s in slots0] if slots0 else None
  kw = dict(row_accums=slots, rowwise_adagrad=hb.embedding.RowwiseAdagrad()) if slots0 else {}
  step = LowpSequenceLookupGrad(hsl, rounding=rounding, seed=99, **kw)
  d_ids, d_sp = [dev(i) for i in ids], [dev(s) for s in splits]
  hsl(d_ids, d_sp)
  torch.cuda.synchronize()
  want = [(bits16(t.table), [slots0[c].copy()] if slots0 else []) for c, t in enumerate(tables)]
  hyper = dict(epsilon=1e-8) if optimizer == 'rowwise_adagrad' else {}
  for k in range(3):
    hsl(d_ids, d_sp)
    grads = [exact.exact_grads(rng, (9, T[c], DIMS[c]), 6) for c in range(2)]
    res = step([dev(g) for g in grads], apply_lr=LR, optimizer=optimizer)
    torch.cuda.synchronize()
    for c, t in enumerate(tables):
      keys = effective(ids[c], splits[c], T[c], pad_ids[c])
      have = np.array([x is not None for x in keys])
      flat = grads[c].reshape(-1, DIMS[c])[have]
      uniq, inv = np.unique(np.array([x for x in keys if x is not None], np.int64), return_inverse=True)
      sums = np.zeros((uniq.size, DIMS[c]), np.float64)
      np.add.at(sums, inv, flat.astype(np.float64))
      assert (sums.astype(F32).astype(np.float64) == sums).all()
      rows = host(t.find(dev(uniq)))
      assert (rows >= 0).all()
      if pad_ids[c] is not None:
        # the pad id's row collects the gradient of every padding position
        pad_at = int(np.nonzero(uniq == pad_ids[c])[0][0])
        n_pad = int((np.array([x == pad_ids[c] for x in keys])).sum())
        assert n_pad > 1 and np.abs(sums[pad_at]).sum() > 0
      u, g, n_u = res[c]
      n_u = int(n_u.item())
      assert n_u == uniq.size
      a, o = np.argsort(host(u)[:n_u]), np.argsort(rows)
      np.testing.assert_array_equal(host(u)[:n_u][a], rows[o])
      np.testing.assert_array_equal(host(g)[:n_u][a].view(np.uint32), sums.astype(F32)[o].view(np.uint32))
      want[c] = ref.apply_step(want[c][0], NAME[dtypes[c]], want[c][1], rows, sums.astype(F32), optimizer, LR, hyper,
                               rounding=rounding, seed=99, step=k, col=c)
  for c, t in enumerate(tables):
    np.testing.assert_array_equal(bits16(t.table), want[c][0], err_msg=f'column {c}: rows')
    if slots0:
      np.testing.assert_array_equal(host(slots[c]).view(np.uint32), want[c][1][0].view(np.uint32))
  assert int(step.step_counter.item()) == (3 if rounding == 'stochastic' else 0)
  # a rehash moves the rows with their keys; the lookup is rebound and the step rebuilt, as on fp32 tables
  before = [(host(t.items()[0]), bits16(t.items()[1])) for t in tables]
  grown = hsl.maybe_grow(max_load=0.01, slots=[[(s, 0.0)] for s in slots] if slots else None)
  assert all(g is not None for g in grown)
  with pytest.raises(_lib.InvalidArgumentError, match='rebind'):
    step([dev(g) for g in grads], apply_lr=LR, optimizer=optimizer)
  outs, _ = hsl(d_ids, d_sp)
  for c, t in enumerate(tables):
    keys, rows = t.items()
    o, w = np.argsort(host(keys)), np.argsort(before[c][0])
    np.testing.assert_array_equal(host(keys)[o], before[c][0][w])
    np.testing.assert_array_equal(bits16(rows)[o], before[c][1][w])


# ---- sharded --------------------------------------------------------------------------------------------------------
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
  return results


@pytest.mark.parametrize('form', ['packed', 'pad_id'])
def test_sharded_sequence_lookup_over_the_16_bit_driver_at_two_ranks(form):
  world = 2
  batches = [batch(20 + r) for r in range(world)]
  dtypes = [BF, HF]
  pads = [-1, 7]

  def rank(r, comm):
    ids, splits, _ = batches[r]
    d_ids, d_sp = [dev(i) for i in ids], [dev(s) for s in splits]
    tables = make_tables(dtypes)
    drv = LowpShardedHashGroupLookup(tables, comm, combiners='sum', wire='table')
    if form == 'packed':
      outs, lengths = ShardedSequenceLookup(drv, T)(d_ids, d_sp)
      outs = [host(o) for o in outs]
    else:
      grids, lengths = sequence_id_grid(d_ids, d_sp, T, pads)
      outs = [host(o).reshape(9, T[c], DIMS[c]) for c, o in enumerate(drv(grids))]
    twins = upcast_twins(tables)
    f32 = ShardedHashGroupLookup(twins, comm, combiners='sum', train=False)
    if form == 'packed':
      want = [host(o) for o in ShardedSequenceLookup(f32, T)(d_ids, d_sp)[0]]
    else:
      want = [host(o).reshape(9, T[c], DIMS[c]) for c, o in enumerate(f32(grids))]
    res = dict(outs=outs, want=want, lengths=[host(x) for x in lengths], keys=[host(t.items()[0]) for t in tables])
    drv.close()
    f32.close()
    return res

  res = run_world(world, rank)
  for r in range(world):
    ids, splits, _ = batches[r]
    for c in range(2):
      np.testing.assert_array_equal(res[r]['outs'][c].view(np.uint32), res[r]['want'][c].view(np.uint32))
      np.testing.assert_array_equal(res[r]['lengths'][c], np.minimum(np.diff(splits[c]), T[c]))
      keys = effective(ids[c], splits[c], T[c], None if form == 'packed' else pads[c])
      want = np.zeros((len(keys), DIMS[c]), F32)
      have = np.array([k is not None for k in keys])
      start = hash_ref.init_rows(np.array([k for k in keys if k is not None], np.int64), DIMS[c], SEEDS[c], 0.05)
      want[have] = torch.from_numpy(start).to(dtypes[c]).float().numpy()
      np.testing.assert_array_equal(res[r]['outs'][c].reshape(-1, DIMS[c]).view(np.uint32), want.view(np.uint32))
  for c in range(2):
    stored = np.concatenate([res[r]['keys'][c] for r in range(world)])
    eff = [k for r in range(world)
           for k in effective(batches[r][0][c], batches[r][1][c], T[c], None if form == 'packed' else pads[c])
           if k is not None]
    np.testing.assert_array_equal(np.sort(stored), np.unique(np.array(eff, np.int64)))
