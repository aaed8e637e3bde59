"""Sharded hash tables on the GPU (hbk_sharded_set_hash_tables, ShardedHashGroupLookup): W ranks as host threads of
one process over Collective.local_world(W), every rank with its own HashTable per column, against the
dict-by-raw-id model of tests/support/sharded_hash_ref.py.  A row's start depends on its key alone, so the
forward is compared bit for bit whatever rank owns the key and whatever slot it got."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
import oracle
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import HashTable, ShardedGroupLookup, ShardedHashGroupLookup
from tests.support import hash_ref as ref
from tests.support import reference as model
from tests.support.sharded_hash_ref import Model, owner
from tests.support.tolerance import FLOOR, REL, WIRE16_FLOOR, WIRE16_REL, assert_sums_close, world_grad_sums

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
DIMS, COMB, SEEDS, SCALE = [16, 6], ['mean', 'sum'], [3, 4], 0.05
SLAB, CAP = [16, 5], [512, 500]


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


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


def make_batches(world, seed=0, pool_size=200, n=300):
  """Per rank: column 0 ragged (about n ids), column 1 one id per sample (n ids), drawn from ONE pool per column
  with negative keys and keys above 2^40, so ranks ask owners for the same keys."""
  rng = np.random.RandomState(900 + seed)
  pools = []
  for _ in range(2):
    k = np.concatenate([rng.randint(-2 ** 62, 0, size=pool_size // 3, dtype=np.int64),
                        rng.randint(0, 1000, size=pool_size // 3, dtype=np.int64),
                        rng.randint(2 ** 40, 2 ** 62, size=pool_size, dtype=np.int64), [-1, 0, 2 ** 63 - 1]])
    pools.append(np.unique(k)[rng.permutation(np.unique(k).size)][:pool_size])
  ids, splits, grads = [], [], []
  for _ in range(world):
    lens = rng.poisson(3, size=n // 3).clip(0, 9)
    sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids.append([pools[0][rng.randint(0, pool_size, size=int(sp[-1]))], pools[1][rng.randint(0, pool_size, size=n)]])
    splits.append([sp, None])
    grads.append([rng.randn(sp.size - 1, DIMS[0]).astype(F32), rng.randn(n, DIMS[1]).astype(F32)])
  return dict(ids=ids, splits=splits, grads=grads, pools=pools)


def make_tables(cap=CAP, **kw):
  return [HashTable(cap[c], DIMS[c], DEV, slab_size=SLAB[c], init_scale=SCALE, seed=SEEDS[c], **kw) for c in range(2)]


def d_step(b, r):
  return [dev(i) for i in b['ids'][r]], [None if s is None else dev(s) for s in b['splits'][r]]


def models_of(b):
  return [Model([i[c] for i in b['ids']], DIMS[c], SEEDS[c], SCALE) for c in range(2)]


def table_state(t):
  return dict(keys=host(t.keys), table=host(t.table), size=t.size(), failed=t.failed(), counts=host(t.counts))


def rows_by_key(states, c, uniq, world, what='table'):
  """The rows of `uniq` read on their owners (a key is found where the probe of its owner's key array finds it)."""
  out = np.zeros((uniq.size, states[0][c][what].shape[1]), F32)
  for r in range(world):
    mine = np.nonzero(owner(uniq, world) == r)[0]
    slots = oracle.cache_probe(states[r][c]['keys'], SLAB[c], uniq[mine])
    assert (slots >= 0).all()
    out[mine] = states[r][c][what][slots]
  return out


def check_forward(b, outs, world, wire16=False, models=None):
  models = models or models_of(b)
  for c, m in enumerate(models):
    eff = oracle.cast_f16_to_f32(oracle.cast_f32_to_f16(m.w)) if wire16 else m.w
    for r in range(world):
      want = oracle.group_lookup_fwd([eff], [m.index(b['ids'][r][c])], [b['splits'][r][c]], [m.uniq.size], [COMB[c]])[0]
      np.testing.assert_array_equal(outs[r][c], want)


def check_ownership(states, models, world):
  for c, m in enumerate(models):
    total = 0
    for r in range(world):
      keys = states[r][c]['keys']
      live = keys[keys != ref.EMPTY]
      assert (owner(live, world) == r).all()
      assert np.isin(live, m.uniq).all() and np.unique(live).size == live.size
      assert states[r][c]['size'] == live.size and states[r][c]['failed'] == 0
      total += live.size
    assert total == m.uniq.size


# ---- forward + SGD backward -------------------------------------------------------------------------------
@pytest.mark.parametrize('world,wire16,dedup', [(1, False, False), (2, False, False), (3, False, False),
                                                (2, True, False), (3, True, False), (3, False, True)])
def test_forward_and_sgd_step_equal_the_model(world, wire16, dedup):
  b = make_batches(world, seed=world)
  lr = 0.1

  def rank(r, comm):
    tables = make_tables()
    drv = ShardedHashGroupLookup(tables, comm, combiners=COMB, dedup=dedup,
                                 wire_dtype=torch.float16 if wire16 else None)
    ids, sp = d_step(b, r)
    for _ in range(2):     # the second step reuses the grown buffers and finds every key
      outs = drv(ids, sp)
    before = [table_state(t) for t in tables]
    slices = drv.backward([dev(g) for g in b['grads'][r]], apply_lr=lr)
    torch.cuda.current_stream().synchronize()
    res = dict(outs=[host(o) for o in outs], before=before, after=[table_state(t) for t in tables],
               slices=[(host(u)[:int(k.item())], host(g)[:int(k.item())]) for u, g, k in slices])
    drv.close()
    return res

  res = run_world(world, rank)
  models = models_of(b)
  check_forward(b, [x['outs'] for x in res], world, wire16, models)
  check_ownership([x['before'] for x in res], models, world)
  rel, floor = (WIRE16_REL, WIRE16_FLOOR) if wire16 else (REL, FLOOR)
  for c, m in enumerate(models):
    G, mag = world_grad_sums(m.uniq.size, DIMS[c], [(m.index(b['ids'][r][c]), b['grads'][r][c], b['splits'][r][c],
                                                     COMB[c]) for r in range(world)])
    # the stepped rows, read through find on their owners
    got = rows_by_key([x['after'] for x in res], c, m.uniq, world)
    assert_sums_close(got, m.w.astype(np.float64) - lr * G, np.abs(m.w) + lr * mag, rel=rel, floor=floor,
                      err_msg=f'sgd step column {c}')
    # the emitted slices: distinct slots, whose keys are ids this rank owns; their scatter is the dense sum
    dense = np.zeros_like(G)
    for r in range(world):
      u, g = res[r]['slices'][c]
      assert np.unique(u).size == u.size
      keys = res[r]['after'][c]['keys'][u]
      assert (keys != ref.EMPTY).all() and (owner(keys, world) == r).all()
      dense[m.index(keys)] += g
      # rows no key holds are untouched (the table starts as zeros)
      free = res[r]['after'][c]['keys'] == ref.EMPTY
      assert not res[r]['after'][c]['table'][free].any()
    assert_sums_close(dense, G, mag, rel=rel, floor=floor, err_msg=f'slices column {c}')


# ---- a mixed plan at the C level: one hash column beside one ordinary bucketed column -------------------------
def test_mixed_plan_hash_column_beside_a_bucketed_column():
  world = 2
  b = make_batches(world, seed=7)
  rows = 211
  rng = np.random.RandomState(5)
  dense = rng.uniform(-1, 1, size=(rows, DIMS[1])).astype(F32)

  def rank(r, comm):
    t = make_tables()[0]
    shard = dev(dense[r::world].copy())
    drv = ShardedGroupLookup([t.table, shard], comm, buckets=[0, rows], combiners=COMB)
    h = (_lib.ShardedHash * 2)()
    h[0].keys_cache, h[0].slab_count, h[0].slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
    h[0].counts, h[0].init_scale, h[0].seed, h[0].insert = t.counts.data_ptr(), t.init_scale, t.seed, 1
    _lib.check(_lib.lib().hbk_sharded_set_hash_tables(drv._plan(), h))
    ids, sp = d_step(b, r)
    outs = drv(ids, sp)
    res = dict(outs=[host(o) for o in outs], state=[table_state(t)])
    drv.close()
    return res

  res = run_world(world, rank)
  m = models_of(b)[0]
  check_forward(b, [x['outs'] for x in res], world, models=[m])
  check_ownership([x['state'] for x in res], [m], world)
  for r in range(world):
    want = oracle.group_lookup_fwd([dense], [b['ids'][r][1]], [None], [rows], [COMB[1]])[0]
    np.testing.assert_array_equal(res[r]['outs'][1], want)


# ---- Adagrad and Lazy Adam, [capacity, dim] slots ----------------------------------------------------------
def world_seq_sums(b, models, c, world):
  """(rows of the model, their fp32 sums in the order the owner sees the terms: requester 0's ids in id order,
  then requester 1's, ... -- the sharded step's deterministic order)."""
  m = models[c]
  t, idx = [], []
  for r in range(world):
    tr, rr, valid = model.terms32(m.uniq.size, m.index(b['ids'][r][c]), b['splits'][r][c], None, COMB[c],
                                  b['grads'][r][c])
    assert valid.all()
    t.append(tr)
    idx.append(rr)
  t, idx = np.concatenate(t), np.concatenate(idx)
  # every key has ONE owner, and the owner receives the requesters' terms in rank order
  return model.seq_row_sums(t, idx, np.ones(idx.size, bool))


@pytest.mark.parametrize('optimizer', ['adagrad', 'adam'])
def test_adagrad_and_lazy_adam_step_equal_the_sequential_model(hbk_option, optimizer):
  hbk_option('bwd_deterministic', 1)
  world, lr = 2, 0.05
  b = make_batches(world, seed=11)

  def rank(r, comm):
    tables = make_tables()
    kw = {}
    if optimizer == 'adagrad':
      kw['accums'] = [torch.full_like(t.table, 0.1) for t in tables]
      slots = [(a,) for a in kw['accums']]
    else:
      kw['adam'] = hb.embedding.LazyAdam(device=torch.device(DEV))
      kw['moments'] = [kw['adam'].slots_like(t.table) for t in tables]
      slots = kw['moments']
    drv = ShardedHashGroupLookup(tables, comm, combiners=COMB, **kw)
    ids, sp = d_step(b, r)
    drv(ids, sp)
    drv.backward([dev(g) for g in b['grads'][r]], apply_lr=lr, optimizer=optimizer, emit=False)
    torch.cuda.current_stream().synchronize()
    res = []
    for c, t in enumerate(tables):
      st = table_state(t)
      for k, x in enumerate(slots[c]):
        st[f'slot{k}'] = host(x)
      res.append(st)
    drv.close()
    return res

  res = run_world(world, rank)
  models = models_of(b)
  for c, m in enumerate(models):
    u, sums = world_seq_sums(b, models, c, world)
    w = m.w.copy()
    if optimizer == 'adagrad':
      a = np.full_like(w, F32(0.1))
      model.adagrad_step(w, a, u, sums, lr)
      want = [a]
      fill = [F32(0.1)]
    else:
      mm, vv = np.zeros_like(w), np.zeros_like(w)
      model.adam_step(w, mm, vv, u, sums, lr, model.ADAM_DEFAULTS[:2])
      want = [mm, vv]
      fill = [F32(0), F32(0)]
    np.testing.assert_array_equal(rows_by_key(res, c, m.uniq, world), w)
    for k, x in enumerate(want):
      np.testing.assert_array_equal(rows_by_key(res, c, m.uniq, world, f'slot{k}'), x)
      for r in range(world):      # slots of rows no key holds were never stepped
        free = res[r][c]['keys'] == ref.EMPTY
        assert (res[r][c][f'slot{k}'][free] == fill[k]).all()


# ---- inference ----------------------------------------------------------------------------------------------
def test_inference_reads_zero_rows_for_unseen_ids_and_inserts_nothing():
  world = 2
  b = make_batches(world, seed=13)
  rng = np.random.RandomState(14)
  b2 = dict(b, ids=[[i.copy() for i in ids] for ids in b['ids']])
  unseen = rng.randint(2 ** 62, 2 ** 63 - 1, size=40, dtype=np.int64)     # (outside the pools' range)
  for r in range(world):
    for c in range(2):
      at = rng.choice(b2['ids'][r][c].size, size=20, replace=False)
      b2['ids'][r][c][at] = unseen[rng.randint(0, unseen.size, size=20)]

  def rank(r, comm):
    tables = make_tables()
    train = ShardedHashGroupLookup(tables, comm, combiners=COMB)
    train(*d_step(b, r))
    before = [table_state(t) for t in tables]
    train.close()
    infer = ShardedHashGroupLookup(tables, comm, combiners=COMB, train=False)
    outs = infer(*d_step(b2, r))
    res = dict(outs=[host(o) for o in outs], before=before, after=[table_state(t) for t in tables])
    infer.close()
    return res

  res = run_world(world, rank)
  for r in range(world):
    for c in range(2):
      for k in ('keys', 'table', 'counts', 'size'):
        np.testing.assert_array_equal(res[r]['before'][c][k], res[r]['after'][c][k])
  # the model with zero rows for the unseen ids
  for c in range(2):
    m = Model([i[c] for i in b2['ids']], DIMS[c], SEEDS[c], SCALE)
    m.w[np.isin(m.uniq, unseen)] = 0
    for r in range(world):
      want = oracle.group_lookup_fwd([m.w], [m.index(b2['ids'][r][c])], [b2['splits'][r][c]], [m.uniq.size], [COMB[c]])[0]
      np.testing.assert_array_equal(res[r]['outs'][c], want)


# ---- a full shard -------------------------------------------------------------------------------------------
def test_a_full_shard_answers_zero_rows_and_keeps_gradients_off_foreign_rows():
  world, lr = 2, 0.5
  b = make_batches(world, seed=17)

  def rank(r, comm):
    # rank 0's table of column 1 is ONE slab: fewer slots than the keys it owns
    tables = make_tables(cap=[CAP[0], SLAB[1] if r == 0 else CAP[1]])
    drv = ShardedHashGroupLookup(tables, comm, combiners=COMB)
    outs = drv(*d_step(b, r))
    before = [table_state(t) for t in tables]
    drv.backward([dev(g) for g in b['grads'][r]], apply_lr=lr, emit=False)
    torch.cuda.current_stream().synchronize()
    res = dict(outs=[host(o) for o in outs], before=before, after=[table_state(t) for t in tables])
    drv.close()
    return res

  res = run_world(world, rank)
  m = models_of(b)[1]
  assert (owner(m.uniq, world) == 0).sum() > SLAB[1]
  zeros = 0
  for r in range(world):
    ids, out = b['ids'][r][1], res[r]['outs'][1]
    rows = m.w[m.index(ids)]
    is_row, is_zero = (out == rows).all(1), (out == 0).all(1)
    assert (is_row | is_zero).all() and not (rows == 0).all(1).any()
    assert (owner(ids[is_zero], world) == 0).all()          # only the full shard fails
    zeros += int(is_zero.sum())
  assert zeros == res[0]['before'][1]['failed'] > 0 and res[1]['before'][1]['failed'] == 0
  # the full shard's rows: a key's row moved by its own gradient only (float64 model over the ids it answered)
  keys = res[0]['after'][1]['keys']
  assert (keys != ref.EMPTY).all() and np.array_equal(keys, res[0]['before'][1]['keys'])
  G, mag = world_grad_sums(m.uniq.size, DIMS[1], [(m.index(b['ids'][r][1]), b['grads'][r][1], None, 'sum')
                                                  for r in range(world)])
  at = m.index(keys)
  assert_sums_close(res[0]['after'][1]['table'], m.w[at].astype(np.float64) - lr * G[at],
                    np.abs(m.w[at]) + lr * mag[at], err_msg='full shard')


# ---- expiring ----------------------------------------------------------------------------------------------
def test_expiring_tables_evict_on_each_rank_and_evicted_ids_come_back_with_their_initial_rows():
  world, lr = 2, 0.5
  b1, b2 = make_batches(world, seed=19), make_batches(world, seed=19)
  # step 2 asks for the first half of each pool only: the other keys go idle
  for r in range(world):
    for c in range(2):
      half = b1['pools'][c][:100]
      b2['ids'][r][c] = half[np.searchsorted(np.sort(half), b1['ids'][r][c]) % half.size]

  def rank(r, comm):
    tables = make_tables(expiring=True)
    drv = ShardedHashGroupLookup(tables, comm, combiners=COMB)
    for t in tables:
      t.set_step(1)
    drv(*d_step(b1, r))
    drv.backward([dev(g) for g in b1['grads'][r]], apply_lr=lr, emit=False)    # rows move away from their start
    for t in tables:
      t.set_step(2)
    drv(*d_step(b2, r))
    for t in tables:
      t.set_step(3)
      t.evict(2)                                                               # last seen at step 1: idle for 2
    mid = [dict(table_state(t), evicted=t.evicted()) for t in tables]
    outs = drv(*d_step(b1, r))                                                 # the evicted ids come back
    res = dict(outs=[host(o) for o in outs], mid=mid, after=[dict(table_state(t), reused=t.reused()) for t in tables])
    drv.close()
    return res

  res = run_world(world, rank)
  for c in range(2):
    m1 = Model([i[c] for i in b1['ids']], DIMS[c], SEEDS[c], SCALE)
    kept = np.unique(np.concatenate([i[c] for i in b2['ids']]))
    gone = np.setdiff1d(m1.uniq, kept)
    assert gone.size > 0
    assert sum(res[r]['mid'][c]['evicted'] for r in range(world)) == gone.size
    # (which free slot a returning key takes is run-dependent once slabs overflow: some are reused, not all need be)
    assert 0 < sum(res[r]['after'][c]['reused'] for r in range(world)) <= gone.size
    for r in range(world):
      live = res[r]['mid'][c]['keys']
      live = live[(live != ref.EMPTY) & (live != ref.EMPTY + 1)]
      assert not np.isin(live, gone).any() and (owner(live, world) == r).all()
    # after they came back: the evicted ids read their initial rows again, the others their stepped rows
    rows = rows_by_key([x['after'] for x in res], c, m1.uniq, world)
    np.testing.assert_array_equal(rows[np.isin(m1.uniq, gone)], m1.w[np.isin(m1.uniq, gone)])
    assert (rows[np.isin(m1.uniq, kept)] != m1.w[np.isin(m1.uniq, kept)]).any()
    for r in range(world):
      want = oracle.group_lookup_fwd([rows], [m1.index(b1['ids'][r][c])], [b1['splits'][r][c]], [m1.uniq.size], [COMB[c]])[0]
      np.testing.assert_array_equal(res[r]['outs'][c], want)


# ---- filtered ----------------------------------------------------------------------------------------------
def test_filtered_tables_count_an_id_over_all_requesters_of_a_step():
  world = 2
  # column 1 only matters: ids 10 and 11 are sent once by EACH rank (owners 0 and 1), 20 and 21 once in total
  ids = [[np.array([10, 11, 20], np.int64)], [np.array([11, 10, 21], np.int64)]]

  def rank(r, comm):
    t = HashTable(CAP[1], DIMS[1], DEV, slab_size=SLAB[1], init_scale=SCALE, seed=SEEDS[1], min_freq=2)
    drv = ShardedHashGroupLookup([t], comm, combiners='sum')
    first = host(drv([dev(ids[r][0])])[0])
    sizes = (t.size(), t.filtered())
    second = host(drv([dev(ids[r][0])])[0])
    res = dict(first=first, second=second, sizes=sizes, size2=t.size(), keys=host(t.keys))
    drv.close()
    return res

  res = run_world(world, rank)
  for r in range(world):
    rows = ref.init_rows(ids[r][0], DIMS[1], SEEDS[1], SCALE)
    np.testing.assert_array_equal(res[r]['first'][:2], rows[:2])       # admitted in the step that saw them twice
    assert not res[r]['first'][2].any()                                # seen once in total: a zero row
    np.testing.assert_array_equal(res[r]['second'], rows)              # ... and admitted by the next step
    assert res[r]['sizes'] == (1, 1) and res[r]['size2'] == 2
    live = res[r]['keys'][res[r]['keys'] != ref.EMPTY]
    assert sorted(live.tolist()) == [10 + r, 20 + r]


# ---- growth -------------------------------------------------------------------------------------------------
def test_maybe_grow_rebinds_and_the_slots_move_with_their_keys(hbk_option):
  hbk_option('bwd_deterministic', 1)
  world, lr = 2, 0.05
  b = make_batches(world, seed=23)
  small = [128, 125]                                                   # about 100 keys per rank: past 0.75

  def rank(r, comm):
    tables = make_tables(cap=small)
    accums = [torch.full_like(t.table, 0.1) for t in tables]
    drv = ShardedHashGroupLookup(tables, comm, combiners=COMB, accums=accums)
    ids, sp = d_step(b, r)
    grads = [dev(g) for g in b['grads'][r]]
    before = [host(o) for o in drv(ids, sp)]
    drv.backward(grads, apply_lr=lr, optimizer='adagrad', emit=False)
    stepped = [host(o) for o in drv(ids, sp)]
    # a rehash behind the object's back: the stale object refuses
    load = [t.size() / t.capacity for t in tables]
    tables[0].rehash(capacity=2 * tables[0].capacity, slots=[(accums[0], 0.1)])
    refused = None
    try:
      drv(ids, sp)
    except _lib.InvalidArgumentError as e:
      refused = str(e)
    try:
      drv.backward(grads, apply_lr=lr, optimizer='adagrad', emit=False)
      refused = None
    except _lib.InvalidArgumentError:
      pass
    drv.close()
    return dict(before=before, stepped=stepped, load=load, refused=refused)

  res = run_world(world, rank)
  for r in range(world):
    assert res[r]['refused'] is not None and 'rebind' in res[r]['refused']
    assert (res[r]['before'][0] != res[r]['stepped'][0]).any()

  def rank2(r, comm):
    tables = make_tables(cap=small)
    accums = [torch.full_like(t.table, 0.1) for t in tables]
    drv = ShardedHashGroupLookup(tables, comm, combiners=COMB, accums=accums)
    ids, sp = d_step(b, r)
    grads = [dev(g) for g in b['grads'][r]]
    drv(ids, sp)
    drv.backward(grads, apply_lr=lr, optimizer='adagrad', emit=False)
    stepped = [host(o) for o in drv(ids, sp)]
    load = [t.size() / t.capacity for t in tables]
    grown = drv.maybe_grow(max_load=0.5)
    caps = [t.capacity for t in tables]
    again = [host(o) for o in drv(ids, sp)]                                  # the rebound object serves
    drv.backward(grads, apply_lr=lr, optimizer='adagrad', emit=False)        # one more step on the moved slots
    torch.cuda.current_stream().synchronize()
    st = []
    for c, t in enumerate(tables):
      s = table_state(t)
      s['slot0'] = host(drv.accums[c])
      st.append(s)
    drv.close()
    return dict(stepped=stepped, again=again, load=load, grown=grown, caps=caps, state=st)

  res = run_world(world, rank2)
  models = models_of(b)
  for r in range(world):
    assert all(l > 0.5 for l in res[r]['load']) and res[r]['grown'] == [True, True]
    assert res[r]['caps'] == [2 * small[0], 2 * small[1]]
    for c in range(2):
      np.testing.assert_array_equal(res[r]['again'][c], res[r]['stepped'][c])
  for c, m in enumerate(models):
    u, sums = world_seq_sums(b, models, c, world)
    w, a = m.w.copy(), np.full_like(m.w, F32(0.1))
    for _ in range(2):
      model.adagrad_step(w, a, u, sums, lr)
    st = [x['state'] for x in res]
    np.testing.assert_array_equal(rows_by_key(st, c, m.uniq, world), w)
    np.testing.assert_array_equal(rows_by_key(st, c, m.uniq, world, 'slot0'), a)


# ---- reshard ------------------------------------------------------------------------------------------------
def test_items_of_two_ranks_restore_onto_three_through_load_owned():
  b = make_batches(3, seed=29)
  b2 = dict(b, ids=b['ids'][:2], splits=b['splits'][:2], grads=b['grads'][:2])

  def rank_a(r, comm):
    tables = make_tables()
    drv = ShardedHashGroupLookup(tables, comm, combiners=COMB)
    drv(*d_step(b2, r))
    drv.backward([dev(g) for g in b2['grads'][r]], apply_lr=0.5, emit=False)      # rows that are not initial rows
    outs = [host(o) for o in drv(*d_step(b2, r))]
    items = [tuple(host(x) for x in t.items()) for t in tables]
    drv.close()
    return dict(outs=outs, items=items)

  two = run_world(2, rank_a)
  keys = [np.concatenate([two[r]['items'][c][0] for r in range(2)]) for c in range(2)]
  rows = [np.concatenate([two[r]['items'][c][1] for r in range(2)]) for c in range(2)]

  def rank_b(r, comm):
    tables = make_tables()
    for c, t in enumerate(tables):
      t.load_owned(dev(keys[c]), dev(rows[c]), 3, r)
    drv = ShardedHashGroupLookup(tables, comm, combiners=COMB, train=False)
    q = r % 2                                                # ranks 0 and 1 repeat the 2-rank batches, rank 2 rank 0's
    outs = [host(o) for o in drv(*d_step(b2, q))]
    res = dict(outs=outs, state=[table_state(t) for t in tables])
    drv.close()
    return res

  three = run_world(3, rank_b)
  for r in range(3):
    for c in range(2):
      np.testing.assert_array_equal(three[r]['outs'][c], two[r % 2]['outs'][c])
      live = three[r]['state'][c]['keys']
      live = live[live != ref.EMPTY]
      assert (owner(live, 3) == r).all()
  for c in range(2):
    assert sum(three[r]['state'][c]['size'] for r in range(3)) == keys[c].size


# ---- refusals that need a plan --------------------------------------------------------------------------------
def test_refusals():
  b = make_batches(1, seed=31)

  def rank(r, comm):
    lib = _lib.lib()
    t = make_tables()[0]
    h = (_lib.ShardedHash * 1)()
    h[0].keys_cache, h[0].slab_count, h[0].slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
    h[0].counts, h[0].init_scale, h[0].seed, h[0].insert = t.counts.data_ptr(), t.init_scale, t.seed, 1
    msgs = {}
    # bucket != 0
    drv = ShardedGroupLookup([t.table], comm, buckets=[t.capacity], combiners='sum')
    assert lib.hbk_sharded_set_hash_tables(drv._plan(), h) == _lib.INVALID_ARGUMENT
    msgs['bucket'] = lib.hbk_last_error().decode()
    drv.close()
    # capacity mismatch
    drv = ShardedGroupLookup([t.table[:-1]], comm, combiners='sum')
    assert lib.hbk_sharded_set_hash_tables(drv._plan(), h) == _lib.INVALID_ARGUMENT
    msgs['capacity'] = lib.hbk_last_error().decode()
    # NULL / no hash column: accepted, the plan stays an ordinary one
    assert lib.hbk_sharded_set_hash_tables(drv._plan(), None) == _lib.OK
    assert lib.hbk_sharded_set_hash_tables(drv._plan(), (_lib.ShardedHash * 1)()) == _lib.OK
    drv.close()
    # p2p_bind on a hash plan, whatever the option says
    tables = make_tables()
    hd = ShardedHashGroupLookup(tables, comm, combiners=COMB)
    ids, sp = d_step(b, 0)
    outs = [torch.zeros(ids[c].numel(), DIMS[c], device=DEV) for c in range(2)]
    for opt in (0, 1):
      old = _lib.set_option('sharded_p2p', opt)
      try:
        hd.close()
        with pytest.raises(_lib.HbkError, match='hash column') as e:
          hd.p2p_bind(outs)
        assert e.value.code == _lib.UNIMPLEMENTED
      finally:
        _lib.set_option('sharded_p2p', old)
    # sp_weights: a weighted column needs a bucket, a hash column has none
    w = [torch.ones(i.numel(), device=DEV) for i in ids]
    with pytest.raises(_lib.InvalidArgumentError, match='bucket'):
      hd(ids, sp, sp_weights=w)
    assert all(x.size() == 0 for x in tables)                      # refused before anything was translated
    # PipelinedLookup
    hd2 = ShardedHashGroupLookup(make_tables(), comm, combiners=COMB)
    with pytest.raises(_lib.HbkError, match='PipelinedLookup') as e:
      hb.embedding.PipelinedLookup([hd, hd2])
    assert e.value.code == _lib.UNIMPLEMENTED
    hd.close()
    hd2.close()
    return msgs

  msgs = run_world(1, rank)[0]
  assert 'bucket' in msgs['bucket'] and 'sharded_set_hash_tables' in msgs['bucket']
  assert 'capacity' in msgs['capacity']
