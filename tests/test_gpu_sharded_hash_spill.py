"""Sharded hash tables with a host tier inside the step (ShardedHashGroupLookup(stores=...)): W ranks as host threads
over Collective.local_world(W).  A tiered world -- every rank's tables bounded to 64 keys through drv.spill_to, the
spilled keys coming back through fault_in_received between the id exchange and the translate -- must train bit for
bit like its unbounded twin.  Gradients lie on the exact grid of tests/support/exact.py (combiner sum, one id per
sample), so every per-key sum is the same whatever slot the key holds and in whatever order it is reduced."""
import numpy as np
import pytest
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (HashExport, HashGroupLookup, HashSpillStore, HashTable,
                                         ShardedHashGroupLookup, hash_fault_in)
from tests.support import exact
from tests.support.sharded_hash_ref import owner
from tests.test_gpu_sharded_hash import DEV, dev, host, run_world

pytestmark = pytest.mark.gpu
F32 = np.float32
DIMS, SLAB, CAP, SEEDS, SCALE = [16, 6], [8, 5], [512, 500], [3, 4], 0.05
STEPS, BOUND, LR, ACC0 = 12, 64, 0.125, 0.1
N_BLOCKS = 6                     # a block of keys returns after six steps: four and more


def make_tables(cap=CAP, **kw):
  return [HashTable(cap[c], DIMS[c], DEV, slab_size=SLAB[c], init_scale=SCALE, seed=SEEDS[c], expiring=True, **kw)
          for c in range(2)]


def make_accums(tables):
  return [torch.full((t.capacity, t.dim), ACC0, dtype=torch.float32, device=DEV) for t in tables]


def make_stores():
  return [HashSpillStore(d, [d]) for d in DIMS]


def make_steps(world, seed, n=48):
  """Per column a pool of 4 W hot keys and six blocks of 12 W keys; step s draws, on every rank, n ids from the hot
  keys and block s mod 6.  Gradients on the exact grid; the budget is asserted here, on the reference alone."""
  rng = np.random.RandomState(seed)
  pools = []
  for _ in range(2):
    k = np.unique(np.concatenate([rng.randint(-2 ** 62, 2 ** 62, size=(4 + 12 * N_BLOCKS) * world + 16, dtype=np.int64),
                                  [-1, 0]]))
    pools.append(k[rng.permutation(k.size)][:(4 + 12 * N_BLOCKS) * world])
  steps = []
  for s in range(STEPS):
    ids, grads = [[] for _ in range(world)], [[] for _ in range(world)]
    for c, pool in enumerate(pools):
      hot, block = pool[:4 * world], pool[4 * world:].reshape(N_BLOCKS, -1)[s % N_BLOCKS]
      cand = np.concatenate([hot, block])
      drawn = [cand[rng.randint(0, cand.size, size=n)] for _ in range(world)]
      rows = np.searchsorted(np.sort(pool), np.concatenate(drawn))
      bits = min(exact.exact_terms_budget(rows, 0, case=f'step {s} column {c}'), 6)
      g = [exact.exact_grads(rng, (n, DIMS[c]), bits) for _ in range(world)]
      exact.exact_dense((pool.size, DIMS[c]), rows, np.concatenate(g), case=f'step {s} column {c}')
      for r in range(world):
        ids[r].append(drawn[r])
        grads[r].append(g[r])
    steps.append((ids, grads))
  return steps, pools


def by_key(exports):
  """key -> the bytes of (row, accumulator row, last_seen, freq), from HashExports (of a table or of a store)."""
  out = {}
  for e in exports:
    keys = host(e.keys) if e.keys.is_cuda else e.keys.numpy()
    arrays = [x.cpu().numpy() for x in (e.rows, e.slots[0], e.last_seen, e.freq)]
    for i, k in enumerate(keys.tolist()):
      assert k not in out, f'key {k} lives twice'
      out[k] = tuple(a[i].tobytes() for a in arrays)
  return out


@pytest.mark.parametrize('world', [1, 2, 4])
def test_a_tiered_world_trains_like_its_unbounded_twin(world):
  steps, _ = make_steps(world, seed=70 + world)

  def rank(r, comm):
    twins = {}
    for name in ('unbounded', 'tiered'):
      tables = make_tables()
      twins[name] = ShardedHashGroupLookup(tables, comm, combiners='sum', accums=make_accums(tables),
                                           initial_accumulator_value=ACC0,
                                           stores=make_stores() if name == 'tiered' else None)
    tiered = twins['tiered']
    log = dict(equal=[], restored=[], stored=[], spilled=[], disjoint=True)
    for s, (ids, grads) in enumerate(steps):
      outs = {}
      for name, drv in twins.items():
        for t in drv.tables:
          t.set_step(s + 1)
        outs[name] = [host(o) for o in drv([dev(i) for i in ids[r]])]
        drv.backward([dev(g) for g in grads[r]], apply_lr=LR, optimizer='adagrad', emit=False)
      log['equal'].append(all(a.tobytes() == b.tobytes() for a, b in zip(outs['unbounded'], outs['tiered'])))
      log['restored'].append(list(tiered.last_restored))
      log['spilled'].append(tiered.spill_to(BOUND))
      log['stored'].append([len(st) for st in tiered.stores])
      for t, st in zip(tiered.tables, tiered.stores):
        both = int((t.find(st.keys().to(DEV)) >= 0).sum().item()) if len(st) else 0
        log['disjoint'] = log['disjoint'] and both == 0
    torch.cuda.current_stream().synchronize()
    log['failed'] = [t.failed() for drv in twins.values() for t in drv.tables]
    log['sizes'] = [t.size() for t in tiered.tables]
    log['unbounded'] = [by_key([e]) for e in twins['unbounded'].export_items()]
    log['tiered'] = [by_key([e, st.peek(st.keys())]) for e, st in zip(tiered.export_items(), tiered.stores)]
    for drv in twins.values():
      drv.close()
    return log

  for r, log in enumerate(run_world(world, rank)):
    assert all(log['equal']), f'rank {r}: outputs differ at steps {[s for s, e in enumerate(log["equal"]) if not e]}'
    assert log['failed'] == [0] * 4
    assert log['disjoint'], f'rank {r}: a key lives in its table and in its store'
    for c in range(2):
      assert sum(x[c] for x in log['restored']) > 0, f'rank {r} column {c}: nothing was ever restored'
      assert max(x[c] for x in log['stored']) > 0, f'rank {r} column {c}: the store was never used'
      assert log['sizes'][c] <= BOUND
      a, b = log['unbounded'][c], log['tiered'][c]
      assert sorted(a) == sorted(b), f'rank {r} column {c}: the twins hold different keys'
      assert all(owner(np.array([k], np.int64), world)[0] == r for k in a)
      bad = [k for k in a if a[k] != b[k]]
      assert not bad, f'rank {r} column {c}: {len(bad)} of {len(a)} keys differ in row, accumulator, last_seen or freq'
    # keys that came back after four and more steps: a block's keys are restored six steps after they were seen
    assert any(sum(x) > 0 for x in log['restored'][N_BLOCKS:])


def test_one_rank_equals_the_composition_by_hand():
  """W = 1: the driver with stores against hash_fault_in + HashGroupLookup + spill by hand -- the tables, the
  stores and the restored counts."""
  steps, _ = make_steps(1, seed=81)

  def rank(r, comm):
    tables, hand = make_tables(), make_tables()
    drv = ShardedHashGroupLookup(tables, comm, combiners='sum', accums=make_accums(tables),
                                 initial_accumulator_value=ACC0, stores=make_stores())
    hand_acc, hand_stores = make_accums(hand), make_stores()
    lookup = HashGroupLookup(hand, combiners='sum')
    same, counts = True, []
    for s, (ids, _) in enumerate(steps[:8]):
      d_ids = [dev(i) for i in ids[0]]
      for t in tables + hand:
        t.set_step(s + 1)
      outs = drv(d_ids)
      restored = hash_fault_in(hand, d_ids, hand_stores, [[a] for a in hand_acc])
      want = lookup(d_ids)
      counts.append((list(drv.last_restored), restored))
      same = same and all(host(a).tobytes() == host(b).tobytes() for a, b in zip(outs, want))
      spilled = drv.spill_to(BOUND // 2)
      for c, t in enumerate(hand):
        exp = t.spill_to(BOUND // 2, hand_stores[c], slots=[(hand_acc[c], ACC0)])
        same = same and len(exp) == spilled[c]
    torch.cuda.current_stream().synchronize()
    res = dict(same=same, counts=counts,
               driver=[by_key([e, st.peek(st.keys())]) for e, st in zip(drv.export_items(), drv.stores)],
               hand=[by_key([e, st.peek(st.keys())]) for e, st in
                     zip([t.export_items(slots=[a]) for t, a in zip(hand, hand_acc)], hand_stores)],
               stored=([len(st) for st in drv.stores], [len(st) for st in hand_stores]))
    drv.close()
    return res

  res = run_world(1, rank)[0]
  assert res['same']
  assert all(a == b for a, b in res['counts']) and sum(sum(a) for a, _ in res['counts']) > 0
  assert res['driver'] == res['hand'] and res['stored'][0] == res['stored'][1] and max(res['stored'][0]) > 0


def test_a_table_too_full_raises_after_every_rank_finished_the_step():
  """Rank 0's column 0 is a 16-slot table whose store holds 40 of its keys; the step asks for all of them.  Every
  rank finishes the step, rank 0 raises afterwards with its keys back in the store, the store of column 1 -- behind the failing
  one -- has not been taken from, and rank 1's outputs are what its own tables hold."""
  world = 2
  rng = np.random.RandomState(90)
  pool = np.unique(rng.randint(-2 ** 62, 2 ** 62, size=400, dtype=np.int64))
  mine = [pool[owner(pool, world) == r] for r in range(world)]
  spilled = mine[0][:40]
  ids = [[np.concatenate([spilled, mine[1][:20]]), mine[0][40:60]], [mine[1][:30], mine[1][30:60]]]

  def rank(r, comm):
    tables = make_tables(cap=[16, 500] if r == 0 else CAP)
    stores = [HashSpillStore(d) for d in DIMS]
    if r == 0:
      for c, keys in enumerate((spilled, mine[0][40:50])):
        n = keys.size
        stores[c].put(HashExport(torch.from_numpy(keys), torch.full((n, DIMS[c]), 2.5), torch.ones(n, dtype=torch.int32),
                                 torch.ones(n, dtype=torch.int32)))
    drv = ShardedHashGroupLookup(tables, comm, combiners='sum', stores=stores)
    for t in tables:
      t.set_step(2)
    error, outs = None, None
    try:
      outs = drv([dev(i) for i in ids[r]])
    except _lib.HbkError as e:
      error = str(e)
    torch.cuda.current_stream().synchronize()
    in_table = [int((t.find(dev(k)) >= 0).sum().item()) for t, k in zip(tables, (spilled, mine[0][40:50]))]
    res = dict(error=error, outs=None if outs is None else [host(o) for o in outs], stored=[len(st) for st in stores],
               in_table=in_table, rows=[host(t.table[t.find(dev(i)).clamp(min=0)]) for t, i in zip(tables, ids[r])])
    drv.close()
    return res

  r0, r1 = run_world(world, rank)
  assert r0['error'] is not None and 'do not fit' in r0['error'] and r0['outs'] is None
  assert r0['stored'][0] + r0['in_table'][0] == 40 and r0['in_table'][0] <= 16      # nothing lost, nothing twice
  assert r0['stored'][1] == 10                                                       # not taken from
  assert r1['error'] is None
  for c in range(2):
    assert r1['outs'][c].tobytes() == r1['rows'][c].tobytes() and r1['outs'][c].any()


class CountingLib:
  """The driver's C library with every call counted by name."""

  def __init__(self, lib):
    self._lib, self.calls = lib, []

  def __getattr__(self, name):
    fn = getattr(self._lib, name)

    def counted(*args):
      self.calls.append(name)
      return fn(*args)
    return counted


def test_all_stores_empty_makes_no_c_call_between_the_halves():
  """With every store empty fault_in_received returns before any tensor work: no C entry is called between
  launch_ids and launch_gather (the stub counts C entries; it cannot see a host read on its own)."""
  steps, _ = make_steps(1, seed=82)

  def rank(r, comm):
    tables = make_tables()
    drv = ShardedHashGroupLookup(tables, comm, combiners='sum', accums=make_accums(tables),
                                 initial_accumulator_value=ACC0, stores=make_stores())
    for t in tables:
      t.set_step(1)
    bound = drv.bind([dev(i) for i in steps[0][0][0]])
    drv._plan()
    drv._lib = counting = CountingLib(drv._lib)
    drv.launch_ids(bound)
    before = list(counting.calls)
    restored = drv.fault_in_received()
    between = counting.calls[len(before):]
    drv.launch_gather(bound)
    outs = drv.launch_end(bound)
    # a store with a key nobody asks for: one call, one read, nothing restored
    drv.stores[0].put(HashExport(torch.tensor([12345]), torch.ones(1, DIMS[0]), torch.ones(1, dtype=torch.int32),
                                 torch.ones(1, dtype=torch.int32), [torch.ones(1, DIMS[0])]))
    drv.launch_ids(bound)
    mark = len(counting.calls)
    again = drv.fault_in_received()
    asked = counting.calls[mark:]
    drv.launch_gather(bound)
    drv.launch_end(bound)
    torch.cuda.current_stream().synchronize()
    res = dict(before=before, between=between, restored=restored, again=again, asked=asked, any=bool(outs[0].any()),
               stored=len(drv.stores[0]))
    drv._lib = counting._lib
    drv.close()
    return res

  res = run_world(1, rank)[0]
  assert res['before'] == ['hbk_sharded_lookup_fwd_ids'] and res['between'] == [] and res['restored'] == [0, 0]
  assert res['asked'].count('hbk_sharded_hash_missing') == 1 and res['again'] == [0, 0] and res['stored'] == 1
  assert res['any']


@pytest.mark.parametrize('world', [1, 2])
def test_maybe_evict_with_spill_remove_and_a_find_only_driver(world):
  """maybe_evict(spill=True) keeps what it evicts and rebinds; remove discards from the stores too; a driver with
  train=False still brings back what its stores hold and inserts nothing else."""
  rng = np.random.RandomState(95 + world)
  pool = np.unique(rng.randint(-2 ** 62, 2 ** 62, size=300 * world, dtype=np.int64))
  mine = [pool[owner(pool, world) == r] for r in range(world)]
  assert min(m.size for m in mine) >= 120

  def rank(r, comm):
    tables = make_tables(cap=[128, 125])
    accums = make_accums(tables)
    stores = make_stores()
    drv = ShardedHashGroupLookup(tables, comm, combiners='sum', accums=accums, initial_accumulator_value=ACC0,
                                 stores=stores)
    keys = mine[r][:100]
    for s in range(4):      # 25 keys of this rank per step: 100 of 128 slots, above max_load 0.75
      for t in tables:
        t.set_step(s + 1)
      drv([dev(keys[25 * s:25 * s + 25])] * 2)
    trained = [host(t.table[t.find(dev(keys))]) for t in tables]
    grown = drv.maybe_evict(max_load=0.75, target_load=0.5, spill=True)
    sizes = [t.size() for t in drv.tables]
    stored = [len(st) for st in stores]
    # remove: ten keys of the stores and ten of the tables
    in_store = [st.keys().numpy()[:10] for st in stores]
    in_table = [host(t.keys[t._live()])[:10] for t in drv.tables]
    drv.remove([dev(np.concatenate([a, b])) for a, b in zip(in_store, in_table)])
    after_remove = [len(st) for st in stores]
    # a find-only driver over the same tables and stores: the spilled keys come back, an unknown key reads zero
    drv.close()
    finder = ShardedHashGroupLookup(drv.tables, comm, combiners='sum', accums=drv.accums, train=False,
                                    initial_accumulator_value=ACC0, stores=stores)
    for t in drv.tables:
      t.set_step(9)
    unknown = mine[r][110:115]
    asked = np.concatenate([keys, unknown])
    outs = finder([dev(asked)] * 2)
    torch.cuda.current_stream().synchronize()
    res = dict(grown=grown, sizes=sizes, stored=stored, after_remove=after_remove, restored=list(finder.last_restored),
               outs=[host(o) for o in outs], trained=trained, left=[len(st) for st in stores],
               removed=[np.isin(keys, np.concatenate([a, b])) for a, b in zip(in_store, in_table)],
               final=[t.size() for t in drv.tables])
    finder.close()
    return res

  for res in run_world(world, rank):
    assert res['grown'] == [True, True]
    for c in range(2):
      assert res['sizes'][c] <= 64 and res['stored'][c] > 0 and res['sizes'][c] + res['stored'][c] == 100
      assert res['after_remove'][c] == res['stored'][c] - 10
      assert res['restored'][c] == res['after_remove'][c] and res['left'][c] == 0
      assert res['final'][c] == 100 - 20                           # nothing inserted: the unknown keys stay unknown
      gone = res['removed'][c]
      out = res['outs'][c]
      assert out[:100][~gone].tobytes() == res['trained'][c][~gone].tobytes()    # rows as they were, spilled or not
      assert not out[:100][gone].any() and not out[100:].any()                   # removed and unknown keys: zero rows


def test_sequences_over_a_tiered_driver():
  """A ShardedSequenceLookup over a tiered driver, T = 4: the tiered twin equals the unbounded one step by step."""
  from hybridbackend_amd.embedding import ShardedSequenceLookup
  world, T = 2, 4
  steps, _ = make_steps(world, seed=99, n=80)
  rng = np.random.RandomState(5)
  lens = [rng.randint(0, 7, size=12) for _ in range(world)]
  splits = [np.concatenate([[0], np.cumsum(x)]).astype(np.int32) for x in lens]

  def rank(r, comm):
    n = int(splits[r][-1])
    twins = {}
    for name in ('unbounded', 'tiered'):
      tables = make_tables()
      drv = ShardedHashGroupLookup(tables, comm, combiners='sum', accums=make_accums(tables),
                                   initial_accumulator_value=ACC0, stores=make_stores() if name == 'tiered' else None)
      twins[name] = (drv, ShardedSequenceLookup(drv, T))
    equal, restored = [], 0
    for s, (ids, _) in enumerate(steps):
      got = {}
      for name, (drv, seq) in twins.items():
        for t in drv.tables:
          t.set_step(s + 1)
        outs, _ = seq([dev(i[:n]) for i in ids[r]], [dev(splits[r])] * 2)
        got[name] = [host(o) for o in outs]
      equal.append(all(a.tobytes() == b.tobytes() and a.shape == (12, T, d)
                       for a, b, d in zip(got['unbounded'], got['tiered'], DIMS)))
      restored += sum(twins['tiered'][0].last_restored)
      twins['tiered'][0].spill_to(16)
    torch.cuda.current_stream().synchronize()
    for drv, _ in twins.values():
      drv.close()
    return dict(equal=equal, restored=restored)

  for res in run_world(world, rank):
    assert all(res['equal']) and res['restored'] > 0
