"""Sharded 16-bit hash tables on the GPU (hbk_sharded_set_lowp_hash_tables, LowpShardedHashGroupLookup): W ranks as
host threads of one process over Collective.local_world(W), every rank with its own 16-bit HashTable per column.

Every comparison is bit for bit.  Slot numbers are not reproducible under concurrent insertion, so rows, slots,
metadata and companions are compared PER KEY: the forward against ShardedHashGroupLookup over fp32 twin tables loaded
with the upcast rows of the same keys; the steps against tests/support/lowp_ref.py applied to the exact per-owner
gradient sums, each key's row addressed by the SLOT read back with find (the stochastic noise is keyed by the rank's
seed and that slot)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (HashExport, HashSpillStore, HashTable, LowpShardedGroupLookup,
                                         LowpShardedHashGroupLookup, RowwiseAdagrad, ShardedGroupLookup,
                                         ShardedHashGroupLookup)
from hybridbackend_amd.embedding.hashtable import LOWP_DTYPES
from hybridbackend_amd.embedding.lowp import rank_seed
from tests.support import exact
from tests.support import hash_ref
from tests.support import lowp_ref as ref
from tests.support.sharded_hash_ref import owner

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
BF, HF = torch.bfloat16, torch.float16
NAME = {BF: ref.BF16, HF: ref.FP16}
DIMS, COMB, SEEDS, SCALE = [16, 6], ['sum', 'sum'], [3, 4], 0.05
SLAB, CAP = [16, 5], [512, 500]
LR = 0.05


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def bits16(t):
  return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


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


def make_batches(world, seed=0, pool_size=120, n=90):
  """Per rank: column 0 ragged, column 1 one id per sample, drawn from ONE pool per column with negative keys and
  keys above 2^40, so ranks ask owners for the same keys; gradients on the exact grid."""
  rng = np.random.RandomState(900 + seed)
  pools = []
  for _ in range(2):
    k = np.concatenate([rng.randint(-2 ** 62, 0, size=pool_size // 3, dtype=np.int64),
                        rng.randint(0, 1000, size=pool_size // 3, dtype=np.int64),
                        rng.randint(2 ** 40, 2 ** 62, size=pool_size, dtype=np.int64), [-1, 0, 2 ** 63 - 1]])
    pools.append(np.unique(k)[rng.permutation(np.unique(k).size)][:pool_size])
  ids, splits = [], []
  for _ in range(world):
    lens = rng.poisson(3, size=n // 3).clip(0, 6)
    sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids.append([pools[0][rng.randint(0, pool_size, size=int(sp[-1]))], pools[1][rng.randint(0, pool_size, size=n)]])
    splits.append([sp, None])
  return dict(ids=ids, splits=splits, pools=pools, rng=rng, n=n)


def exact_grads(b, world, steps):
  return [[[exact.exact_grads(b['rng'], (b['splits'][r][c].size - 1 if b['splits'][r][c] is not None else b['n'],
                                         DIMS[c]), 6) for c in range(2)] for r in range(world)] for _ in range(steps)]


def make_tables(dtypes, cap=CAP, **kw):
  return [HashTable(cap[c], DIMS[c], DEV, slab_size=SLAB[c], init_scale=SCALE, seed=SEEDS[c], dtype=dtypes[c], **kw)
          for c in range(2)]


def d_step(b, r):
  return [dev(i) for i in b['ids'][r]], [None if s is None else dev(s) for s in b['splits'][r]]


def key_sums(b, grads, c, world):
  """(distinct keys of column c over every rank's batch, their exact fp32 gradient sums)."""
  keys = np.concatenate([b['ids'][r][c] for r in range(world)])
  terms = np.concatenate([exact.id_terms(grads[r][c], b['splits'][r][c], COMB[c]) for r in range(world)])
  uniq, inv = np.unique(keys, return_inverse=True)
  sums = np.zeros((uniq.size, DIMS[c]), np.float64)
  np.add.at(sums, inv, terms)
  assert (sums.astype(F32).astype(np.float64) == sums).all(), 'the sums are not exact in fp32: shrink the case'
  return uniq, sums.astype(F32)


def slots_of(table, keys):
  s = host(table.find(dev(keys)))
  assert (s >= 0).all()
  return s


def twin_forward(tables, comm, ids, sp, dedup):
  """ShardedHashGroupLookup over fp32 twins loaded with the upcast rows of the same keys; a pure find."""
  twins = []
  for t in tables:
    kw = dict(slab_size=t.slab_size, init_scale=t.init_scale, seed=t.seed, expiring=t.expiring)
    u = HashTable(t.capacity, t.dim, DEV, **kw)
    keys, rows = t.items()
    if keys.numel():
      u.load(keys, rows.float())
    twins.append(u)
  f32 = ShardedHashGroupLookup(twins, comm, combiners=COMB, dedup=dedup, train=False)
  outs = [host(o) for o in f32(ids, sp)]
  f32.close()
  return outs


# ---- forward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('world,wire,dedup', [(1, 'table', False), (1, 'float', True), (2, 'table', True),
                                              (2, 'float', False), (3, 'table', False), (3, 'float', True)])
def test_forward_equals_the_fp32_driver_over_the_upcast_twins(world, wire, dedup):
  b = make_batches(world, seed=world)
  dtypes = [BF, HF]

  def rank(r, comm):
    tables = make_tables(dtypes)
    drv = LowpShardedHashGroupLookup(tables, comm, combiners=COMB, wire=wire, dedup=dedup)
    ids, sp = d_step(b, r)
    for _ in range(2):     # the second step reuses the grown buffers and finds every key
      outs = [host(o) for o in drv(ids, sp)]
    want = twin_forward(tables, comm, ids, sp, dedup)
    res = dict(outs=outs, want=want, keys=[host(t.keys) for t in tables], rows=[bits16(t.table) for t in tables],
               size=[t.size() for t in tables], failed=[t.failed() for t in tables])
    drv.close()
    return res

  res = run_world(world, rank)
  for c in range(2):
    uniq = np.unique(np.concatenate([b['ids'][r][c] for r in range(world)]))
    total = 0
    for r in range(world):
      np.testing.assert_array_equal(res[r]['outs'][c].view(np.uint32), res[r]['want'][c].view(np.uint32))
      assert res[r]['outs'][c].any()
      keys = res[r]['keys'][c]
      live = keys != hash_ref.EMPTY
      assert (owner(keys[live], world) == r).all() and res[r]['failed'][c] == 0
      # every new row is the cast start row of its key, every other row still zero
      start = hash_ref.init_rows(keys[live], DIMS[c], SEEDS[c], SCALE)
      np.testing.assert_array_equal(res[r]['rows'][c][live],
                                    torch.from_numpy(start).to(dtypes[c]).view(torch.int16).numpy().view(np.uint16))
      assert not res[r]['rows'][c][~live].any()
      total += int(live.sum())
    assert total == uniq.size


@pytest.mark.parametrize('wire', ['table', 'float'])
def test_a_minus_one_slot_reads_a_zero_row(wire):
  """A full shard, train=False and a filtered id: all three answer -1, which is a zero row on both wires."""
  world = 2
  b = make_batches(world, seed=11, pool_size=60, n=40)

  def rank(r, comm):
    ids, sp = d_step(b, r)
    out = {}
    # train=False on empty tables: nothing is inserted, everything reads zero
    tables = make_tables([BF, HF])
    drv = LowpShardedHashGroupLookup(tables, comm, combiners=COMB, wire=wire, train=False)
    out['find'] = [host(o) for o in drv(ids, sp)]
    out['find_size'] = [t.size() for t in tables]
    drv.close()
    # a filtered table: an id seen once over all requesters of the step is not admitted
    tables = make_tables([BF, HF], min_freq=10 ** 6)
    drv = LowpShardedHashGroupLookup(tables, comm, combiners=COMB, wire=wire)
    out['filtered'] = [host(o) for o in drv(ids, sp)]
    out['filtered_size'] = [t.size() for t in tables]
    # nothing is sent back for a -1: the emit backward names no slot
    g = [dev(np.ones(o.shape, F32)) for o in out['filtered']]
    out['n_unique'] = [int(k.item()) for _, _, k in drv.backward(g)]
    drv.close()
    # a full shard: one slab per rank and column, far more keys
    tables = make_tables([BF, HF], cap=[16, 5])
    drv = LowpShardedHashGroupLookup(tables, comm, combiners=COMB, wire=wire)
    outs = [host(o) for o in drv(ids, sp)]
    out['full'] = outs
    out['full_state'] = [(host(t.keys), bits16(t.table), t.failed()) for t in tables]
    out['full_want'] = twin_forward(tables, comm, ids, sp, False)
    drv.close()
    return out

  res = run_world(world, rank)
  for r in range(world):
    assert res[r]['find_size'] == [0, 0] and res[r]['filtered_size'] == [0, 0] and res[r]['n_unique'] == [0, 0]
    for c in range(2):
      assert not res[r]['find'][c].view(np.uint32).any() and not res[r]['filtered'][c].view(np.uint32).any()
      keys, rows, failed = res[r]['full_state'][c]
      assert (keys != hash_ref.EMPTY).all() and failed > 0
      np.testing.assert_array_equal(res[r]['full'][c].view(np.uint32), res[r]['full_want'][c].view(np.uint32))
  assert any(res[r]['full'][1].any() for r in range(world))


# ---- backward and step ---------------------------------------------------------------------------------------------
def slot_arrays(optimizer, tables, rng):
  """fp32 optimizer slots of the tables' shapes as numpy arrays, per table a list."""
  if optimizer == 'adagrad':
    return [[rng.uniform(0.1, 0.9, size=(t.capacity, t.dim)).astype(F32)] for t in tables]
  if optimizer == 'rowwise_adagrad':
    return [[rng.uniform(0.1, 0.9, size=(t.capacity, 1)).astype(F32)] for t in tables]
  return [[] for _ in tables]


def slot_kwargs(optimizer, slots):
  if optimizer == 'adagrad':
    return dict(accums=[s[0] for s in slots])
  if optimizer == 'rowwise_adagrad':
    return dict(row_accums=[s[0] for s in slots], rowwise_adagrad=RowwiseAdagrad())
  return {}


@pytest.mark.parametrize('world,dtypes,rounding', [(1, [BF, HF], 'nearest'), (2, [HF, BF], 'nearest'),
                                                   (3, [BF, BF], 'stochastic')])
@pytest.mark.parametrize('optimizer', ['sgd', 'adagrad', 'rowwise_adagrad'])
def test_three_steps_equal_the_restatement_per_key(optimizer, world, dtypes, rounding):
  b = make_batches(world, seed=20 + world)
  steps, seed = 3, 4242
  grads = exact_grads(b, world, steps)
  hyper = dict(epsilon=1e-8) if optimizer == 'rowwise_adagrad' else {}

  def rank(r, comm):
    tables = make_tables(dtypes)
    slots0 = slot_arrays(optimizer, tables, np.random.RandomState(77 + r))
    slots = [[dev(s) for s in ss] for ss in slots0]
    drv = LowpShardedHashGroupLookup(tables, comm, combiners=COMB, wire='table', rounding=rounding, seed=seed,
                                     **slot_kwargs(optimizer, slots))
    assert drv.rank_seed == rank_seed(seed, r)
    ids, sp = d_step(b, r)
    drv(ids, sp)          # every key of the world is stored from here on: the slots stay
    torch.cuda.current_stream().synchronize()
    want = [(bits16(t.table), [s.copy() for s in slots0[c]]) for c, t in enumerate(tables)]
    for step in range(steps):
      drv(ids, sp)
      res = drv.backward([dev(g) for g in grads[step][r]], apply_lr=LR, optimizer=optimizer, emit=bool(step % 2))
      torch.cuda.current_stream().synchronize()
      for c, t in enumerate(tables):
        uniq, sums = key_sums(b, grads[step], c, world)
        mine = owner(uniq, world) == r
        rows = slots_of(t, uniq[mine])
        if step % 2:
          u, g, k = res[c]
          n_u = int(k.item())
          assert n_u == rows.size
          a, o = np.argsort(host(u)[:n_u]), np.argsort(rows)
          np.testing.assert_array_equal(host(u)[:n_u][a], rows[o])
          np.testing.assert_array_equal(host(g)[:n_u][a].view(np.uint32), sums[mine][o].view(np.uint32))
        else:
          assert res[c][0] is None and res[c][1] is None
        want[c] = ref.apply_step(want[c][0], NAME[dtypes[c]], want[c][1], rows, sums[mine], optimizer, LR, hyper,
                                 rounding=rounding, seed=rank_seed(seed, r), step=step, col=c)
    got = [(bits16(t.table), [host(s) for s in slots[c]]) for c, t in enumerate(tables)]
    counter = int(drv.step_counter.item())
    drv.close()
    return dict(got=got, want=want, counter=counter)

  res = run_world(world, rank)
  for r in range(world):
    assert res[r]['counter'] == (steps if rounding == 'stochastic' else 0)
    for c in range(2):
      what = f'rank {r} column {c}'
      np.testing.assert_array_equal(res[r]['got'][c][0], res[r]['want'][c][0], err_msg=what + ': rows')
      for k, s in enumerate(res[r]['got'][c][1]):
        np.testing.assert_array_equal(s.view(np.uint32), res[r]['want'][c][1][k].view(np.uint32),
                                      err_msg=f'{what}: slot {k}')


# ---- one case each ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wire', ['table', 'float'])
def test_a_plan_mixing_a_16_bit_hash_column_and_a_16_bit_bucketed_column(wire):
  world = 2
  b = make_batches(world, seed=7)
  rows = 211
  dense = np.random.RandomState(5).uniform(-1, 1, size=(rows, DIMS[1])).astype(F32)

  def rank(r, comm):
    t = make_tables([BF, HF])[0]
    shard = dev(dense[r::world].copy()).to(HF)
    drv = LowpShardedGroupLookup([t.table, shard], comm, buckets=[0, rows], combiners=COMB, wire=wire)
    h = (_lib.ShardedHash * 2)()
    h[0].keys_cache, h[0].slab_count, h[0].slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
    h[0].counts, h[0].init_scale, h[0].seed, h[0].insert = t.counts.data_ptr(), t.init_scale, t.seed, 1
    codes = (C.c_int32 * 2)(LOWP_DTYPES[BF], LOWP_DTYPES[HF])
    _lib.check(_lib.lib().hbk_sharded_set_lowp_hash_tables(drv._plan(), h, codes,
                                                           _lib.LOWP_WIRE_TABLE if wire == 'table' else
                                                           _lib.LOWP_WIRE_FLOAT))
    ids, sp = d_step(b, r)
    outs = [host(o) for o in drv(ids, sp)]
    # the twin: an fp32 plan with the same two columns, the hash table loaded with the upcast rows
    u = HashTable(t.capacity, t.dim, DEV, slab_size=t.slab_size, init_scale=t.init_scale, seed=t.seed)
    keys, stored = t.items()
    u.load(keys, stored.float())
    f32 = ShardedGroupLookup([u.table, shard.float()], comm, buckets=[0, rows], combiners=COMB)
    g = (_lib.ShardedHash * 2)()
    g[0].keys_cache, g[0].slab_count, g[0].slab_size = u.keys.data_ptr(), u.slab_count, u.slab_size
    g[0].init_scale, g[0].seed, g[0].insert = u.init_scale, u.seed, 0
    _lib.check(_lib.lib().hbk_sharded_set_hash_tables(f32._plan(), g))
    want = [host(o) for o in f32(ids, sp)]
    res = dict(outs=outs, want=want, size=t.size())
    drv.close()
    f32.close()
    return res

  res = run_world(world, rank)
  uniq = np.unique(np.concatenate([b['ids'][r][0] for r in range(world)]))
  assert sum(x['size'] for x in res) == uniq.size
  for r in range(world):
    for c in range(2):
      np.testing.assert_array_equal(res[r]['outs'][c].view(np.uint32), res[r]['want'][c].view(np.uint32))
      assert res[r]['outs'][c].any()


def test_maybe_grow_rebinds_and_the_slots_move_with_their_keys():
  world = 2
  b = make_batches(world, seed=31)
  grads = exact_grads(b, world, 2)

  def rank(r, comm):
    tables = make_tables([BF, HF], cap=[128, 125])
    accums = [torch.full((t.capacity, t.dim), 0.5, dtype=torch.float32, device=DEV) for t in tables]
    drv = LowpShardedHashGroupLookup(tables, comm, combiners=COMB, accums=accums, initial_accumulator_value=0.25)
    ids, sp = d_step(b, r)
    drv(ids, sp)
    drv.backward([dev(g) for g in grads[0][r]], apply_lr=LR, optimizer='adagrad')
    torch.cuda.current_stream().synchronize()
    before = []
    for c, t in enumerate(tables):
      keys, rows = t.items()
      before.append((host(keys), bits16(rows), host(drv.accums[c][t.find(keys)])))
    grown = drv.maybe_grow(max_load=0.05)
    assert grown == [True, True]
    after = []
    for c, t in enumerate(tables):
      keys = dev(before[c][0])
      s = t.find(keys)
      assert (s >= 0).all() and t.capacity > CAP[c] // 4 and tuple(drv.accums[c].shape) == (t.capacity, t.dim)
      free = torch.ones(t.capacity, dtype=torch.bool, device=DEV)
      free[s] = False
      assert not bits16(t.table[free]).any() and (drv.accums[c][free] == 0.25).all()
      after.append((bits16(t.table[s]), host(drv.accums[c][s])))
    # the rebuilt step works on the moved rows and slots
    drv(ids, sp)
    drv.backward([dev(g) for g in grads[1][r]], apply_lr=LR, optimizer='adagrad')
    torch.cuda.current_stream().synchronize()
    stepped = []
    for c, t in enumerate(tables):
      uniq, sums = key_sums(b, grads[1], c, world)
      mine = owner(uniq, world) == r
      keys = before[c][0]
      order = np.searchsorted(keys[np.argsort(keys)], uniq[mine])
      idx = np.argsort(keys)[order]
      want = ref.apply_step(after[c][0], NAME[t.dtype], [after[c][1]], idx, sums[mine], 'adagrad', LR)
      s = t.find(dev(keys))
      stepped.append((bits16(t.table[s]), host(drv.accums[c][s]), want))
    drv.close()
    return dict(before=before, after=after, stepped=stepped)

  res = run_world(world, rank)
  for r in range(world):
    for c in range(2):
      np.testing.assert_array_equal(res[r]['after'][c][0], res[r]['before'][c][1])
      np.testing.assert_array_equal(res[r]['after'][c][1].view(np.uint32), res[r]['before'][c][2].view(np.uint32))
      got_rows, got_acc, (want_rows, want_slots) = res[r]['stepped'][c]
      np.testing.assert_array_equal(got_rows, want_rows)
      np.testing.assert_array_equal(got_acc.view(np.uint32), want_slots[0].view(np.uint32))


def test_a_tiered_run_equals_an_unbounded_one():
  """stores=, the tables bounded to 64 of 512 slots after every step, against tables that keep everything."""
  world = 2
  batches = [make_batches(world, seed=40 + k, pool_size=150) for k in range(3)]
  for k in range(3):
    batches[k]['grads'] = exact_grads(batches[k], world, 1)[0]

  def rank(r, comm):
    out = {}
    for tiered in (False, True):
      tables = make_tables([BF, HF], cap=[512, 500], expiring=True)
      accums = [torch.full((t.capacity, t.dim), 0.5, dtype=torch.float32, device=DEV) for t in tables]
      stores = [HashSpillStore(t.dim, slot_dims=(t.dim,), pin_memory=False, dtype=t.dtype) for t in tables] \
          if tiered else None
      drv = LowpShardedHashGroupLookup(tables, comm, combiners=COMB, accums=accums, stores=stores,
                                       initial_accumulator_value=0.5)
      outs = []
      for step, b in enumerate(batches):
        for t in tables:
          t.set_step(step + 1)
        ids, sp = d_step(b, r)
        outs.append([host(o) for o in drv(ids, sp)])
        drv.backward([dev(g) for g in b['grads'][r]], apply_lr=LR, optimizer='adagrad')
        if tiered:
          drv.spill_to(64)
          assert all(t.size() <= 64 for t in tables)
      torch.cuda.current_stream().synchronize()
      state = []
      for c, t in enumerate(tables):
        exp = drv.export_items()[c]
        keys, rows, acc = host(exp.keys), bits16(exp.rows), host(exp.slots[0])
        if tiered and len(stores[c]):
          held = stores[c].peek(stores[c].keys())
          keys = np.concatenate([keys, host(held.keys)])
          rows = np.concatenate([rows, bits16(held.rows)])
          acc = np.concatenate([acc, host(held.slots[0])])
        o = np.argsort(keys)
        state.append((keys[o], rows[o], acc[o]))
      out[tiered] = dict(outs=outs, state=state)
      drv.close()
    return out

  res = run_world(world, rank)
  for r in range(world):
    for k in range(3):
      for c in range(2):
        np.testing.assert_array_equal(res[r][True]['outs'][k][c].view(np.uint32),
                                      res[r][False]['outs'][k][c].view(np.uint32), err_msg=f'step {k} column {c}')
    for c in range(2):
      for x, y in zip(res[r][True]['state'][c], res[r][False]['state'][c]):
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == F32 else x,
                                      y.view(np.uint32) if y.dtype == F32 else y)


def test_export_items_of_two_ranks_restore_onto_three():
  b2 = make_batches(2, seed=50)
  grads = exact_grads(b2, 2, 1)[0]

  def save(r, comm):
    tables = make_tables([BF, HF])
    accums = [torch.full((t.capacity, 1), 0.5, dtype=torch.float32, device=DEV) for t in tables]
    drv = LowpShardedHashGroupLookup(tables, comm, combiners=COMB, row_accums=accums,
                                     rowwise_adagrad=RowwiseAdagrad())
    ids, sp = d_step(b2, r)
    drv(ids, sp)
    drv.backward([dev(g) for g in grads[r]], apply_lr=LR, optimizer='rowwise_adagrad')
    exps = drv.export_items()
    assert all(e.rows.dtype == t.dtype for e, t in zip(exps, tables))
    out = [e.variables('x') for e in exps]
    out = [{k: v.cpu() for k, v in d.items()} for d in out]
    drv.close()
    return out

  saved = run_world(2, save)
  exports = [HashExport.cat([HashExport.from_variables('x', saved[r][c]) for r in range(2)]) for c in range(2)]
  b3 = make_batches(3, seed=51)

  def restore(r, comm):
    tables = make_tables([BF, HF])
    accums = [torch.full((t.capacity, 1), 0.5, dtype=torch.float32, device=DEV) for t in tables]
    drv = LowpShardedHashGroupLookup(tables, comm, combiners=COMB, row_accums=accums,
                                     rowwise_adagrad=RowwiseAdagrad(), train=False)
    on_dev = [HashExport(e.keys.to(DEV), e.rows.to(DEV), slots=[s.to(DEV) for s in e.slots]) for e in exports]
    drv.import_items(on_dev)
    state = []
    for c, t in enumerate(tables):
      keys, rows = t.items()
      state.append((host(keys), bits16(rows), host(accums[c][t.find(keys)])))
    ids, sp = d_step(b3, r)
    outs = [host(o) for o in drv(ids, sp)]      # a pure find over the restored tables: the plan stayed valid
    drv.close()
    return dict(state=state, outs=outs)

  res = run_world(3, restore)
  for c in range(2):
    keys = host(exports[c].keys)
    assert np.unique(keys).size == keys.size
    got_keys = np.concatenate([res[r]['state'][c][0] for r in range(3)])
    got_rows = np.concatenate([res[r]['state'][c][1] for r in range(3)])
    got_acc = np.concatenate([res[r]['state'][c][2] for r in range(3)])
    for r in range(3):
      assert (owner(res[r]['state'][c][0], 3) == r).all()
    o, w = np.argsort(got_keys), np.argsort(keys)
    np.testing.assert_array_equal(got_keys[o], keys[w])
    np.testing.assert_array_equal(got_rows[o], bits16(exports[c].rows)[w])
    np.testing.assert_array_equal(got_acc[o].view(np.uint32), host(exports[c].slots[0])[w].view(np.uint32))


# ---- the C-level refusals of the new setter ---------------------------------------------------------------------------
def _last():
  return _lib.lib().hbk_last_error().decode()


def _hash_of(t, **kw):
  h = (_lib.ShardedHash * 1)()
  h[0].keys_cache, h[0].slab_count, h[0].slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
  h[0].counts, h[0].init_scale, h[0].seed, h[0].insert = t.counts.data_ptr(), t.init_scale, t.seed, 1
  for k, v in kw.items():
    setattr(h[0], k, v)
  return h


def _code(dtype):
  return (C.c_int32 * 1)(LOWP_DTYPES.get(dtype, 7))


def test_the_setter_refuses_by_name_and_leaves_the_shard_alone():
  """The plans are made over the table's rows viewed as fp32 words ([capacity, dim / 2]): creation takes any shard, and
  what is looked at here is the setter."""
  lib = _lib.lib()
  comm = hb.distribute.Collective.local_world(1)[0]
  TABLE = _lib.LOWP_WIRE_TABLE

  def plan_over(t, **kw):
    return ShardedGroupLookup([t.table.view(torch.float32)], comm, **kw)

  def refused(drv, t, h, dt, wire, status, *words):
    before = (bits16(t.table), host(t.keys))
    rc = lib.hbk_sharded_set_lowp_hash_tables(drv._plan(), h, dt, wire)
    msg = _last()
    assert rc == status, (rc, msg)
    for w in ('sharded_set_lowp_hash_tables',) + words:
      assert w in msg, msg
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits16(t.table), before[0])
    np.testing.assert_array_equal(host(t.keys), before[1])

  try:
    t = HashTable(64, 8, DEV, slab_size=8, dtype=BF)
    t.table.view(torch.int16).fill_(0x1234)
    drv = plan_over(t)
    refused(drv, t, _hash_of(t), _code(None), TABLE, _lib.INVALID_ARGUMENT, 'column 0', 'dtype')
    refused(drv, t, _hash_of(t), _code(BF), 5, _lib.INVALID_ARGUMENT, 'wire')
    refused(drv, t, _hash_of(t, slab_size=65), _code(BF), TABLE, _lib.INVALID_ARGUMENT, 'column 0', 'slab_size')
    refused(drv, t, _hash_of(t, slab_count=3), _code(BF), TABLE, _lib.INVALID_ARGUMENT, 'column 0', 'capacity')
    refused(drv, t, _hash_of(t, init_scale=65505.0), _code(HF), TABLE, _lib.INVALID_ARGUMENT, 'column 0', '65504')
    h = _hash_of(t)
    h[0].exp.last_seen = t.keys.data_ptr()
    refused(drv, t, h, _code(BF), TABLE, _lib.INVALID_ARGUMENT, 'column 0', 'expiring')
    # accepted; then everything a 16-bit plan refuses stays refused, and NULL gives the fp32 plan back
    assert lib.hbk_sharded_set_lowp_hash_tables(drv._plan(), _hash_of(t), _code(BF), TABLE) == _lib.OK, _last()
    assert lib.hbk_sharded_set_max_norms(drv._plan(), (C.c_float * 1)(1.0)) == _lib.UNIMPLEMENTED
    assert '16-bit' in _last()
    assert lib.hbk_sharded_set_hash_tables(drv._plan(), _hash_of(t)) == _lib.UNIMPLEMENTED
    assert '16-bit' in _last()
    assert lib.hbk_sharded_set_lowp_hash_tables(drv._plan(), None, None, 0) == _lib.OK
    assert lib.hbk_sharded_set_max_norms(drv._plan(), (C.c_float * 1)(1.0)) == _lib.OK
    refused(drv, t, _hash_of(t), _code(BF), TABLE, _lib.UNIMPLEMENTED, 'column 0', 'max_norm')
    drv.close()
    # a bucketed column cannot be a hash column; a plan created for the fp16 wire cannot be a 16-bit plan
    drv = plan_over(t, buckets=[100])
    refused(drv, t, _hash_of(t), _code(BF), TABLE, _lib.INVALID_ARGUMENT, 'column 0', 'bucket')
    drv.close()
    drv = plan_over(t, wire_dtype=torch.float16)
    refused(drv, t, _hash_of(t), _code(BF), TABLE, _lib.UNIMPLEMENTED, 'HBK_HALF')
    drv.close()
    # dims the translate or the 16-bit gathers would refuse inside the step (the plan's dim is the view's)
    for dim, word in ((7, 'even'), (130, 'dim % 4')):
      u = HashTable(64, 2 * dim, DEV, slab_size=8, dtype=BF)
      drv = plan_over(u)
      refused(drv, u, _hash_of(u), _code(BF), TABLE, _lib.INVALID_ARGUMENT, 'column 0', word)
      drv.close()
  finally:
    comm.close()


def test_sp_weights_are_refused_by_the_library_before_anything_is_inserted():
  comm = hb.distribute.Collective.local_world(1)[0]
  try:
    b = make_batches(1, seed=3)
    tables = make_tables([BF, HF])
    drv = LowpShardedHashGroupLookup(tables, comm, combiners=COMB)
    ids, sp = d_step(b, 0)
    weights = [torch.ones(ids[0].numel(), dtype=torch.float32, device=DEV), None]
    with pytest.raises(_lib.HbkError, match='id_weights need a bucket'):
      drv(ids, sp, sp_weights=weights)
    torch.cuda.synchronize()
    assert [t.size() for t in tables] == [0, 0] and not any(bits16(t.table).any() for t in tables)
    drv.close()
  finally:
    comm.close()
