"""Hash-keyed 8-bit tables on the GPU (HashTable(dtype='int8'), hbk_hash_insert_quant8_n), everything bit for bit:
insert, lookup, step, the lifecycle moves, and the refusals of what is not built."""
import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd import feature_column as fc
from hybridbackend_amd.embedding import GroupLookup, GroupLookupGrad, Quant8GroupLookup, Quant8LookupGrad, Quant8Rows
from hybridbackend_amd.embedding import RowwiseAdagrad, SparseApply, dequantize_rows8, quantize_rows8
from tests.support import exact, hash_ref, quant8_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
KINDS = {'plain': {}, 'expiring': dict(expiring=True), 'filtered': dict(min_freq=2),
         'expiring-filtered': dict(expiring=True, min_freq=2)}


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def some_ids(rng, n=300, distinct=200):
  pool = rng.randint(-2 ** 62, 2 ** 62, size=distinct, dtype=np.int64)
  return rng.permutation(np.concatenate([pool, pool[rng.randint(0, distinct, size=n - distinct)]]))


def check_rows(t8, ids, scale, twin=None):
  """Every key's row, all pitch bytes, is the numpy restatement and quantize_rows8 of the fp32 twin's row."""
  s8 = t8.find(dev(ids))
  assert (s8 >= 0).all()
  got = t8.table[s8].cpu().numpy()
  np.testing.assert_array_equal(got, quant8_ref.quantise(hash_ref.init_rows(ids, t8.dim, t8.seed, scale), t8.pitch))
  if twin is not None:
    rows32 = twin.table[twin.find(dev(ids))]
    np.testing.assert_array_equal(got, quantize_rows8([rows32], t8.pitch)[0].cpu().numpy())
  if scale in (0.0, 1e-35):
    assert not quant8_ref.scales(got, t8.dim).any() and (got[:, :t8.dim] == 128).all()
  return s8


@pytest.mark.parametrize('dim,slab_size', [(4, 64), (6, 8), (20, 8), (64, 1), (64, 8), (256, 2)])
def test_insert_equals_the_format(dim, slab_size):
  ids = some_ids(np.random.RandomState(dim + slab_size))
  for align, scale in ((4, 1e-3), (16, 1e-3), (4, 0.0), (4, 1e-35)):
    kw = dict(slab_size=slab_size, seed=dim + 5, init_scale=scale)
    twin = hb.embedding.HashTable(512, dim, DEV, **kw)
    t8 = hb.embedding.HashTable(512, dim, DEV, dtype='int8', pitch=Quant8Rows.pitch_for(dim, align), **kw)
    assert t8.table.dtype == torch.uint8 and tuple(t8.table.shape) == (t8.capacity, t8.pitch) and t8.dim == dim
    twin.lookup_or_insert(dev(ids))
    assert (t8.lookup_or_insert(dev(ids)) >= 0).all() and t8.size() == 200
    s8 = check_rows(t8, ids, scale, twin)
    free = torch.ones(t8.capacity, dtype=torch.bool, device=DEV)
    free[s8] = False
    assert int(free.sum()) == t8.capacity - 200 and not t8.table[free].any()   # (a fresh table is all zero bytes)


@pytest.mark.parametrize('kind', list(KINDS))
def test_the_four_inserting_forms_and_a_reused_slot(kind):
  rng = np.random.RandomState(3)
  t8 = hb.embedding.HashTable(512, 20, DEV, dtype='int8', pitch=32, seed=9, **KINDS[kind])
  ids = some_ids(rng)
  for step in (1, 2):                        # (a filtered table admits at the second sighting)
    if t8.expiring:
      t8.set_step(step)
    t8.lookup_or_insert(dev(ids))
  assert t8.size() == 200
  check_rows(t8, ids, 1e-3)
  if t8.expiring:                            # every key leaves; the next keys take their slots, scribbled on in between
    t8.set_step(9)
    t8.evict(2)
    t8.table.fill_(0xFF)
    other = dev(some_ids(rng))
    t8.lookup_or_insert(other)
    t8.lookup_or_insert(other)
    assert t8.size() == 200 and t8.reused() > 0
    check_rows(t8, other.cpu().numpy(), 1e-3)


def test_lookup_is_grouplookup_over_the_dequantised_tables():
  rng = np.random.RandomState(5)
  dims, n_seg = [6, 64], 40
  tables = [hb.embedding.HashTable(256, d, DEV, dtype='int8', init_scale=1.0, seed=c) for c, d in enumerate(dims)]
  lens = rng.randint(0, 5, size=n_seg)
  splits = [dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)), None]
  counts = [int(lens.sum()), n_seg]
  weights = [dev(rng.uniform(-2, 2, size=counts[0]).astype(F32)), None]
  pools = [rng.randint(-2 ** 62, 2 ** 62, size=60, dtype=np.int64) for _ in dims]
  draw = lambda pools: [dev(p[rng.randint(0, p.size, size=n)]) for p, n in zip(pools, counts)]   # noqa: E731
  ids = draw(pools)

  def same(hgl, outs, what):
    deq = dequantize_rows8([t.table for t in hgl.tables], dims)
    want = GroupLookup(deq, combiners=['mean', 'sum'])(hgl.slots, splits, sp_weights=weights)
    bits = lambda x: x.view(torch.int16 if x.element_size() == 2 else torch.int32)   # noqa: E731
    for o, w in zip(outs, want):
      assert o.any() and torch.equal(bits(o), bits(w.to(o.dtype))), what

  hgl = hb.embedding.HashGroupLookup(tables, combiners=['mean', 'sum'])
  assert isinstance(hgl.lookup, Quant8GroupLookup) and hgl.lookup.buckets == [0, 0]
  outs = hgl(ids, splits, sp_weights=weights)
  same(hgl, outs, 'call')
  wide = hb.embedding.HashGroupLookup(tables, combiners=['mean', 'sum'], out_dtype=torch.bfloat16, lane_codes=8)
  same(wide, wide(ids, splits, sp_weights=weights), 'bf16 outputs, 8 codes per lane')
  for i, fresh in zip(ids, draw([np.concatenate([p, p + 1]) for p in pools])):   # launch(): both launches again
    i.copy_(fresh)
  hgl.launch()
  same(hgl, outs, 'launch')
  frozen = hb.embedding.HashGroupLookup(tables, combiners=['mean', 'sum'], train=False)
  outs = frozen(draw([np.concatenate([p, p + 7]) for p in pools]), splits, sp_weights=weights)
  assert all((s == -1).any() for s in frozen.slots)
  same(frozen, outs, 'train=False: unseen ids read as zero rows')


@pytest.mark.parametrize('optimizer', ['rowwise_adagrad', 'sgd'])
def test_three_steps_equal_sparse_apply_on_the_dequantised_table_requantised(optimizer):
  rng = np.random.RandomState(7)
  dim, n_seg, lr = 20, 48, 0.05
  t = hb.embedding.HashTable(512, dim, DEV, dtype='int8', init_scale=1.0, seed=3)
  acc = torch.full((t.capacity, 1), 0.1, device=DEV)
  slots_of = lambda a: dict(row_accums=[a], rowwise_adagrad=RowwiseAdagrad()) if optimizer != 'sgd' else {}   # noqa: E731
  hgl = hb.embedding.HashGroupLookup([t])
  step = Quant8LookupGrad(hgl.lookup, rounding='nearest', **slots_of(acc))
  pool = rng.randint(-2 ** 62, 2 ** 62, size=90, dtype=np.int64)
  hgl([dev(pool)])                                            # keys beyond every batch
  for _ in range(3):
    hgl([dev(pool[rng.randint(0, 60, size=n_seg)])])
    grads = [dev(exact.exact_grads(rng, (n_seg, dim), 6))]
    before, deq, acc32 = t.table.clone(), dequantize_rows8([t.table], [dim]), acc.clone()
    slices = GroupLookupGrad(GroupLookup(deq))(hgl.slots, grads)
    SparseApply(deq, **slots_of(acc32))(slices, lr, optimizer)
    step(hgl.slots, grads, apply_lr=lr, optimizer=optimizer)
    hit = torch.zeros(t.capacity, dtype=torch.bool, device=DEV)
    hit[hgl.slots[0]] = True
    assert torch.equal(t.table[hit], quantize_rows8(deq, t.pitch)[0][hit]) and not torch.equal(t.table[hit], before[hit])
    assert torch.equal(t.table[~hit], before[~hit]) and torch.equal(acc.view(torch.int32), acc32.view(torch.int32))


@pytest.mark.parametrize('op', ['rehash', 'maybe_grow', 'export_import', 'spill_fault_in', 'remove', 'evict_to'])
def test_lifecycle_carries_rows_and_companions_bit_for_bit(op):
  rng = np.random.RandomState(11)
  dim, pitch = 20, 32
  mk = lambda cap, slab: hb.embedding.HashTable(cap, dim, DEV, slab_size=slab, dtype='int8', pitch=pitch,   # noqa: E731
                                                init_scale=1.0, expiring=True)
  t, pool = mk(256, 8), rng.randint(-2 ** 62, 2 ** 62, size=150, dtype=np.int64)
  acc = torch.full((t.capacity, 1), 0.1, device=DEV)
  hgl = hb.embedding.HashGroupLookup([t], train=False)
  for step in (1, 2, 3):
    t.set_step(step)
    part = dev(pool[50 * (step - 1):50 * step])
    acc[t.lookup_or_insert(part)] = ((part % 1000).float() + step).unsqueeze(1)
  t.table[t.find(dev(pool)), dim + 4:] = 0xAB                 # (marks behind the scale word: they travel too)
  rows, accs = t.table[t.find(dev(pool))].clone(), acc[t.find(dev(pool))].clone()
  store = hb.embedding.HashSpillStore(dim, (1,), dtype='int8', pitch=pitch)
  if op == 'rehash':
    acc, = t.rehash(capacity=512, slots=[(acc, 0.1)])
  elif op == 'maybe_grow':
    acc, = hgl.maybe_grow(max_load=0.5, slots=[[(acc, 0.1)]])[0]
  elif op == 'export_import':
    exp = t.export_items(slots=[acc])
    assert exp.rows.dtype == torch.uint8 and tuple(exp.rows.shape) == (150, pitch)
    t, acc = mk(512, 16), torch.zeros((512, 1), device=DEV)
    t.import_items(exp, slots=[acc])
    hgl = hb.embedding.HashGroupLookup([t], train=False)
  elif op == 'spill_fault_in':
    t.spill_to(100, store, slots=[(acc, 0.1)])                 # (the 50 keys of step 1)
    assert len(store) == 50 == t.fault_in(dev(pool), store, slots=[acc])
  elif op == 'remove':                                        # 10 keys out of the store, 10 out of the table
    t.spill_to(100, store, slots=[(acc, 0.1)])
    t.remove(dev(np.concatenate([pool[:10], pool[140:]])), slots=[(acc, 0.1)], store=store)
    assert len(store) == 40
  else:
    t.evict_to(100, slots=[(acc, 0.1)])
  hgl.rebind()
  found = t.find(dev(pool))
  here = found >= 0                                           # (what was removed, evicted or spilled is not here)
  assert int(here.sum()) == {'remove': 90, 'evict_to': 100}.get(op, 150)
  assert torch.equal(t.table[found[here]], rows[here])
  assert torch.equal(acc[found[here]].view(torch.int32), accs[here].view(torch.int32))
  out = hgl([dev(pool)])[0]
  want = torch.where(here.unsqueeze(1), dev(quant8_ref.dequantise(rows.cpu().numpy(), dim)), torch.zeros((), device=DEV))
  assert torch.equal(out.view(torch.int32), want.view(torch.int32))


def test_refusals_name_what_they_refuse():
  def refused(match, call):
    with pytest.raises(_lib.InvalidArgumentError, match=match):
      call()
  mk, emb = hb.embedding.HashTable, hb.embedding
  t = mk(64, 8, DEV, dtype='int8', expiring=True)
  refused('cannot share one lookup.*table 1: int8', lambda: emb.HashGroupLookup([mk(64, 8, DEV), t]))
  refused('max_norms is not supported for 8-bit tables', lambda: emb.HashGroupLookup([t], max_norms=[1.0]))
  refused('pitch 16', lambda: t.spill_to(10, emb.HashSpillStore(8, dtype='int8', pitch=16)))
  keys, meta = torch.arange(3, device=DEV), torch.zeros(3, dtype=torch.int32)
  for rows in (torch.zeros((3, 8), device=DEV), torch.zeros((3, 16), dtype=torch.uint8, device=DEV)):   # dtype, pitch
    refused('load: rows must be uint8', lambda: t.load(keys, rows))
    refused('import_items: exp.rows must be uint8', lambda: t.import_items(emb.HashExport(keys, rows)))
    refused('put: exp.rows must be uint8',
            lambda: emb.HashSpillStore(8, dtype='int8').put(emb.HashExport(keys.cpu(), rows.cpu(), meta, meta)))
  refused("HashSequenceLookup: table 0 is an 'int8' HashTable", lambda: emb.HashSequenceLookup([t], max_lens=4))
  refused("ShardedHashGroupLookup: table 0 is an 'int8' HashTable", lambda: emb.ShardedHashGroupLookup([t], None))
  refused("column 'k': dtype='int8' is not served", lambda: fc.HashEmbeddingColumn('k', 64, 8, dtype='int8'))
  refused("column 'k': dtype='int8' is not served", lambda: fc.HashSequenceEmbeddingColumn('k', 64, 8, 4, dtype='int8'))
  for dim in (257, 66):
    refused(f'HashTable: dim {dim} is beyond', lambda: mk(64, dim, DEV, dtype='int8'))
