"""The sharded forward in three parts on the GPU (hbk_sharded_lookup_fwd_ids / _gather, hbk_sharded_hash_missing;
ShardedGroupLookup.launch_ids / launch_gather): W ranks as host threads over Collective.local_world(W).  Every rank
runs the same steps twice over twin state -- once through the one-call forward, once through launch_ids +
launch_gather + launch_end -- and outputs, table state and the stepped tables must agree bit for bit (the backward
runs in its reproducible mode, so nothing depends on the run; hash tables are compared key by key).  Between the
halves hbk_sharded_hash_missing must report what hash_missing reports on the ids the rank owns, taken on the host
from all ranks' batches in peer order."""
import ctypes as C

import numpy as np
import pytest
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import HashTable, ShardedGroupLookup, ShardedHashGroupLookup, hash_missing
from tests.support import hash_missing_ref as mref
from tests.support.sharded_hash_ref import owner
from tests.test_gpu_sharded_hash import DEV, DIMS, COMB, d_step, dev, host, make_batches, run_world

pytestmark = pytest.mark.gpu
F32 = np.float32
SLAB, CAP, ROWS, LR = [8, 5], [512, 500], 211, 0.125


def make_tables():
  return [HashTable(CAP[c], DIMS[c], DEV, slab_size=SLAB[c], init_scale=0.05, seed=3 + c, expiring=True)
          for c in range(2)]


def table_arrays(t):
  """The table by key: which slot of its slab a key wins is decided by a compare-and-swap among the lanes that
  insert beside it, so twins agree on the keys and on everything a key holds, not on slot numbers."""
  keys = host(t.keys)
  live = np.flatnonzero((keys != mref.EMPTY) & (keys != mref.TOMBSTONE))
  order = live[np.argsort(keys[live], kind='stable')]
  return [keys[order]] + [host(x)[order] for x in (t.table, t.last_seen, t.freq)] + [host(t.counts), host(t.stats)]


def make_plan(kind, r, world, comm, wire16, dedup):
  """(driver, state()) of one twin: `state` reads every array the step may write."""
  wire = torch.float16 if wire16 else None
  dense = [np.random.RandomState(40 + c).uniform(-1, 1, size=(ROWS, DIMS[c])).astype(F32) for c in range(2)]
  if kind == 'bucketed':
    shards = [dev(d[r::world].copy()) for d in dense]
    drv = ShardedGroupLookup(shards, comm, buckets=[ROWS, ROWS], combiners=COMB, wire_dtype=wire, dedup=dedup)
    return drv, lambda: [host(s) for s in shards]
  tables = make_tables()
  if kind == 'hash':
    drv = ShardedHashGroupLookup(tables, comm, combiners=COMB, wire_dtype=wire, dedup=dedup)
    drv.tables_ = tables
    return drv, lambda: [a for t in tables for a in table_arrays(t)]
  # mixed: a hash column beside a bucketed column, the tables set at the C level
  t = tables[0]
  t.set_step(1)
  shard = dev(dense[1][r::world].copy())
  drv = ShardedGroupLookup([t.table, shard], comm, buckets=[0, ROWS], combiners=COMB, wire_dtype=wire, dedup=dedup)
  h = (_lib.ShardedHash * 2)()
  h[0].keys_cache, h[0].slab_count, h[0].slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
  h[0].counts, h[0].init_scale, h[0].seed, h[0].insert = t.counts.data_ptr(), t.init_scale, t.seed, 1
  t._describe_expiry(h[0].exp)
  _lib.check(_lib.lib().hbk_sharded_set_hash_tables(drv._plan(), h))
  drv.keep_ = (t, h)
  return drv, lambda: table_arrays(t) + [host(shard)]


def forward(drv, form, ids, sp):
  if form == 'one':
    return drv(ids, sp)
  bound = drv.bind(ids, sp)
  drv.launch_ids(bound)
  drv.launch_gather(bound)
  return drv.launch_end(bound)


@pytest.fixture
def reproducible_backward():
  old = _lib.set_option('bwd_deterministic', 1)
  yield
  _lib.set_option('bwd_deterministic', old)


@pytest.mark.parametrize('kind', ['bucketed', 'hash', 'mixed'])
@pytest.mark.parametrize('world,wire16,dedup', [(1, False, False), (2, False, False), (3, False, False),
                                                (2, True, False), (3, False, True)])
def test_three_parts_equal_the_one_call_forward(reproducible_backward, kind, world, wire16, dedup):
  b = make_batches(world, seed=10 + world)

  def rank(r, comm):
    res = {}
    for form in ('one', 'three'):
      drv, state = make_plan(kind, r, world, comm, wire16, dedup)
      ids, sp = d_step(b, r)
      for t in getattr(drv, 'tables_', ()):
        t.set_step(1)
      for _ in range(2):     # the second step reuses the grown buffers and finds every key
        outs = forward(drv, form, ids, sp)
      torch.cuda.current_stream().synchronize()
      outs, before = [host(o) for o in outs], state()
      slices = drv.backward([dev(g) for g in b['grads'][r]], apply_lr=LR)
      torch.cuda.current_stream().synchronize()
      res[form] = dict(outs=outs, before=before, after=state(),
                       slices=[(host(u)[:int(k.item())], host(g)[:int(k.item())]) for u, g, k in slices])
      drv.close()
    return res

  for r, res in enumerate(run_world(world, rank)):
    one, three = res['one'], res['three']
    for name in ('outs', 'before', 'after'):
      assert len(one[name]) == len(three[name])
      for k, (x, y) in enumerate(zip(one[name], three[name])):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f'rank {r}: {name}[{k}] differs'
    assert any(o.any() for o in one['outs'])
    assert any(x.tobytes() != y.tobytes() for x, y in zip(one['before'], one['after'])), 'the backward stepped nothing'
    for c, ((u1, g1), (u3, g3)) in enumerate(zip(one['slices'], three['slices'])):
      if kind == 'bucketed' or (kind == 'mixed' and c == 1):   # (row numbers; a hash column's are slot numbers)
        assert u1.tobytes() == u3.tobytes() and g1.tobytes() == g3.tobytes(), f'rank {r}: the emitted slices differ'
      else:
        assert u1.size == u3.size and np.sort(g1, axis=0).tobytes() == np.sort(g3, axis=0).tobytes()


@pytest.mark.parametrize('world,dedup', [(1, False), (2, False), (3, False), (3, True)])
def test_hash_missing_between_the_halves(world, dedup):
  """Step 1 inserts one batch; step 2 brings another whose pools overlap it.  Between launch_ids and launch_gather
  of step 2 the call must report, per column, the distinct ids this rank received that its table does not hold, in
  the order of the ids it owns: every requester's batch in peer order, each in batch order."""
  first, second = make_batches(world, seed=20 + world), make_batches(world, seed=20 + world, pool_size=260)
  assert any(np.setdiff1d(second['pools'][c], first['pools'][c]).size for c in range(2))

  def rank(r, comm):
    tables = make_tables()
    drv = ShardedHashGroupLookup(tables, comm, combiners=COMB, dedup=dedup)
    for t in tables:
      t.set_step(1)
    drv(*d_step(first, r))
    bound = drv.bind(*d_step(second, r))
    drv.launch_ids(bound)
    plan, lib = drv._plan(), _lib.lib()
    caps = [int(lib.hbk_sharded_owned_ids(plan, c)) for c in range(2)]
    outs = [torch.full((k + 1,), -77, dtype=torch.int64, device=DEV) for k in caps]
    counts = torch.full((2,), -5, dtype=torch.int64, device=DEV)
    _lib.check(lib.hbk_sharded_hash_missing(plan, (C.c_uint8 * 2)(1, 1), _lib.ptr_array([o.data_ptr() for o in outs]),
                                            _lib.i64_array(caps), counts.data_ptr(),
                                            _lib.current_stream(torch.device(DEV))))
    # one wanted column only: the other's count and output are not touched
    lone = torch.full((2,), -5, dtype=torch.int64, device=DEV)
    lone_out = torch.full((caps[1] + 1,), -77, dtype=torch.int64, device=DEV)
    _lib.check(lib.hbk_sharded_hash_missing(plan, (C.c_uint8 * 2)(0, 1), _lib.ptr_array([None, lone_out.data_ptr()]),
                                            _lib.i64_array([0, caps[1]]), lone.data_ptr(),
                                            _lib.current_stream(torch.device(DEV))))
    owned = [np.concatenate([second['ids'][q][c][owner(second['ids'][q][c], world) == r] for q in range(world)])
             for c in range(2)]
    want = [host(m) for m in hash_missing(tables, [dev(o) for o in owned])]
    keys_before = [host(t.keys) for t in tables]
    drv.launch_gather(bound)
    out = drv.launch_end(bound)
    torch.cuda.current_stream().synchronize()
    res = dict(caps=caps, owned=[o.size for o in owned], got=[host(o) for o in outs], counts=counts.tolist(),
               want=want, lone=lone.tolist(), lone_out=host(lone_out), keys_before=keys_before,
               sizes=[t.size() for t in tables], out=[host(o) for o in out])
    drv.close()
    return res

  missed_somewhere = 0
  for r, res in enumerate(run_world(world, rank)):
    for c in range(2):
      k = res['counts'][c]
      assert res['caps'][c] <= res['owned'][c] and (dedup or res['caps'][c] == res['owned'][c])
      assert k == res['want'][c].size, (r, c, k, res['want'][c].size)
      np.testing.assert_array_equal(res['got'][c][:k], res['want'][c])
      assert (res['got'][c][k:] == -77).all()
      missed_somewhere += k
    assert res['lone'] == [-5, res['counts'][1]]
    assert res['lone_out'].tobytes() == res['got'][1].tobytes()
  assert missed_somewhere > 0


def test_state_rules_name_the_call():
  """_gather and hbk_sharded_hash_missing need an open _ids step, _end comes after _gather, want[c] needs a hash
  column with an expiring table, a new _ids drops an open step, and a tiered driver refuses a capture."""
  from hybridbackend_amd.embedding import HashSpillStore
  b = make_batches(1, seed=31)

  def refused(call, *words):
    with pytest.raises(_lib.HbkError) as e:
      call()
    for w in words:
      assert w in str(e.value), str(e.value)
    return True

  def rank(r, comm):
    lib, stream = _lib.lib(), _lib.current_stream(torch.device(DEV))
    tables = make_tables()
    plain = HashTable(CAP[1], DIMS[1], DEV, slab_size=SLAB[1])
    drv = ShardedHashGroupLookup([tables[0], plain], comm, combiners=COMB)
    tables[0].set_step(1)
    bound = drv.bind(*d_step(b, r))
    plan = drv._plan()
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    out = torch.zeros(4096, dtype=torch.int64, device=DEV)

    def missing(want):
      _lib.check(lib.hbk_sharded_hash_missing(plan, (C.c_uint8 * 2)(*want), _lib.ptr_array([out.data_ptr()] * 2),
                                              _lib.i64_array([4096, 4096]), counts.data_ptr(), stream))
    ok = [refused(lambda: drv.launch_gather(bound), 'sharded_lookup_fwd_gather', 'no step is open'),
          refused(lambda: missing([1, 0]), 'sharded_hash_missing', 'no step is open'),
          refused(lambda: drv.launch_end(bound), 'sharded_lookup_fwd_end', 'no step is open')]
    drv.launch_ids(bound)
    ok += [refused(lambda: drv.launch_end(bound), 'sharded_lookup_fwd_end', 'hbk_sharded_lookup_fwd_gather'),
           refused(lambda: missing([1, 1]), 'sharded_hash_missing', 'column 1', 'expiring')]
    missing([0, 0])                      # nothing wanted: nothing to do
    missing([1, 0])
    drv.launch_ids(bound)                # a new _ids drops the open step and opens its own
    drv.launch_gather(bound)
    ok.append(refused(lambda: drv.launch_gather(bound), 'sharded_lookup_fwd_gather', 'no step is open'))
    ok.append(refused(lambda: missing([1, 0]), 'sharded_hash_missing', 'no step is open'))
    first = [host(o) for o in drv.launch_end(bound)]
    again = [host(o) for o in drv(*d_step(b, r))]     # the one-call forward after it: the same rows
    drv.close()
    # a driver with stores reads the host in its forward: refused while the stream captures
    tiered = ShardedHashGroupLookup([tables[0]], comm, combiners=COMB[:1], stores=[HashSpillStore(DIMS[0])])
    ids, sp = d_step(b, r)
    bound = tiered.bind(ids[:1], sp[:1])
    tiered.launch(bound)
    torch.cuda.current_stream().synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.current_stream()):
      ok.append(refused(lambda: tiered.launch(bound), 'cannot be captured'))
    tiered.close()
    return dict(ok=ok, same=all(x.tobytes() == y.tobytes() for x, y in zip(first, again)))

  res = run_world(1, rank)[0]
  assert all(res['ok']) and len(res['ok']) == 8 and res['same']


def test_p2p_bound_plan_is_unimplemented(hbk_option):
  """hbk_sharded_lookup_fwd_ids and hbk_sharded_hash_missing on a p2p-bound plan: HBK_UNIMPLEMENTED, the call named;
  the refused _ids drops the step an earlier _ids left open."""
  hbk_option('sharded_p2p', 1)
  world = 2

  def rank(r, comm):
    lib, stream = _lib.lib(), _lib.current_stream(torch.device(DEV))
    drv = ShardedGroupLookup([dev(np.zeros((50, 16), F32))], comm, buckets=[100])
    ids = dev(np.arange(8, dtype=np.int64) * 7 + r)
    out = torch.zeros((8, 16), dtype=torch.float32, device=DEV)
    bound = drv.bind([ids], None, [out])
    drv.launch_ids(bound)                                    # an open step of the exchange form
    if not drv.p2p_bind([out]):                              # (collective: every rank gets the same answer)
      drv.launch_gather(bound)
      drv.launch_end(bound)
      drv.close()
      return 'unbound'
    a = bound.args
    seen = []
    for call in (lambda: lib.hbk_sharded_lookup_fwd_ids(drv._plan(), a[0], a[1], a[2], a[3], stream),
                 lambda: lib.hbk_sharded_lookup_fwd_gather(drv._plan(), stream),
                 lambda: lib.hbk_sharded_hash_missing(drv._plan(), (C.c_uint8 * 1)(1), None, None, None, stream)):
      seen.append((call(), lib.hbk_last_error().decode()))
    with pytest.raises(_lib.HbkError, match='sharded_lookup_fwd_ids'):
      drv.launch_ids(bound)
    drv.p2p_unbind()
    drv.close()
    return seen

  res = run_world(world, rank)
  if 'unbound' in res:
    pytest.skip('peer memory could not be mapped: no p2p form to refuse in')
  for seen in res:
    (ids_rc, ids_msg), (gather_rc, gather_msg), (miss_rc, miss_msg) = seen
    assert ids_rc == _lib.UNIMPLEMENTED and 'sharded_lookup_fwd_ids' in ids_msg and 'p2p-bound' in ids_msg
    assert gather_rc == _lib.INVALID_ARGUMENT and 'no step is open' in gather_msg     # the refused _ids dropped it
    assert miss_rc == _lib.UNIMPLEMENTED and 'sharded_hash_missing' in miss_msg and 'p2p-bound' in miss_msg
