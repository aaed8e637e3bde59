"""Hash-keyed 16-bit tables on the GPU (HashTable(dtype=), hbk_hash_insert_lowp_n): the inserting launch writes the
rounded start row and nothing else, a mixed translate leaves the fp32 tables as they were, the forward is GroupLookup
over the upcast tables bit for bit, the step is lowp_ref.apply_step per key, and a whole life of a 16-bit table --
loads, sweeps, rehashes, the host tier, removal, export, import, the saver's variables -- is the life of its fp32
twin, cast."""
import ctypes as C

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import GroupLookup, LowpGroupLookup, LowpLookupGrad, RowwiseAdagrad
from tests.support import exact
from tests.support import hash_ref
from tests.support import lowp_ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32 = np.float32
NAMES = {torch.bfloat16: lowp_ref.BF16, torch.float16: lowp_ref.FP16}
LOWP = [torch.bfloat16, torch.float16]
IDS = ['bf16', 'fp16']
KINDS = {'plain': {}, 'expiring': dict(expiring=True), 'filtered': dict(min_freq=1),
         'expiring-filtered': dict(expiring=True, min_freq=1)}


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits16(t):
  return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def bits32(t):
  return t.detach().contiguous().view(torch.int32).cpu().numpy()


def oracle(keys, dim, seed, scale, dtype):
  """The uint16 patterns of the start rows of `keys`: the fp32 values of include/hbk.h, rounded to nearest even."""
  return lowp_ref.round_nearest(lowp_ref.bits32(hash_ref.init_rows(np.asarray(keys, np.int64), dim, seed, scale)),
                                NAMES[dtype])


def some_ids(rng, n=300, distinct=200):
  """n ids over `distinct` values of the whole int64 range, the sentinels left out: duplicates inside one call."""
  pool = rng.randint(-2 ** 62, 2 ** 62, size=distinct, dtype=np.int64)
  ids = pool[rng.randint(0, distinct, size=n)]
  ids[:distinct] = pool                      # every value occurs
  return rng.permutation(ids)


# ---- 1. the bits the inserting launch writes ---------------------------------------------------------------------
@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
@pytest.mark.parametrize('slab_size,dim', [(1, 2), (8, 6), (8, 16), (64, 2), (16, 130)])
@pytest.mark.parametrize('kind', list(KINDS))
def test_new_rows_are_the_rounded_start_values_and_nothing_else_is_written(kind, slab_size, dim, dtype):
  """dim / 2 words below, equal to and above the lane group (pow2 of the slab size), and not a power of two."""
  rng = np.random.RandomState(slab_size * 1000 + dim)
  ids = some_ids(rng)
  d_ids = dev(ids)
  for scale in (1.0, 1e-3, 0.0):
    t = hb.embedding.HashTable(1024, dim, DEV, slab_size=slab_size, init_scale=scale, seed=0x5EED + dim, dtype=dtype,
                               **KINDS[kind])
    assert t.table.dtype == dtype and t.capacity >= 4 * 200
    if t.expiring:
      t.set_step(3)
    slots = t.lookup_or_insert(d_ids)
    s = slots.cpu().numpy()
    assert (s >= 0).all() and t.size() == 200 and t.failed() == 0
    assert len(set(zip(ids.tolist(), s.tolist()))) == 200 and np.unique(s).size == 200     # one slot per key
    np.testing.assert_array_equal(t.keys[slots].cpu().numpy(), ids)
    got = bits16(t.table)
    want = oracle(ids, dim, t.seed, scale, dtype)
    np.testing.assert_array_equal(got[s], want, f'{kind} scale {scale}')
    if scale == 0.0:
      assert not got.any()                                                                # 0x0000, not -0
    # every row no key took is still 0x0000: a store of 4 * dim bytes or a wrong pitch would have reached one
    free = np.ones(t.capacity, bool)
    free[s] = False
    assert free.sum() == t.capacity - 200 and not got[free].any(), f'{kind} scale {scale}: a free row was written'
    # a present key's row is not initialised again
    t.table.view(torch.int16)[int(s[0])] = 0x1234
    before = bits16(t.table)
    again = t.lookup_or_insert(d_ids)
    np.testing.assert_array_equal(again.cpu().numpy(), s)
    np.testing.assert_array_equal(bits16(t.table), before)
    assert (before[s[0]] == 0x1234).all() and t.size() == 200
    # find writes nothing, for keys it finds and keys it does not
    keys_before = t.keys.clone()
    unseen = dev(np.concatenate([ids[:50], rng.randint(-2 ** 62, 2 ** 62, size=50, dtype=np.int64)]))
    found = t.find(unseen).cpu().numpy()
    np.testing.assert_array_equal(found[:50], s[:50])
    assert (found[50:] == -1).all()
    np.testing.assert_array_equal(bits16(t.table), before)
    assert torch.equal(t.keys, keys_before) and t.size() == 200


@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
def test_the_padding_between_dim_and_pitch_keeps_what_it_held(dtype):
  """The entry itself, with table_pitch = dim + 2 on a buffer full of 0x7FFF."""
  rng = np.random.RandomState(77)
  dim, pitch, slab_size, slab_count = 6, 8, 8, 64
  cap = slab_size * slab_count
  ids = some_ids(rng, 150, 100)
  d_ids = dev(ids)
  keys = torch.full((cap,), -2 ** 63, dtype=torch.int64, device=DEV)
  buf = torch.full((cap, pitch), 0x7FFF, dtype=torch.int16, device=DEV)
  slots = torch.empty(ids.size, dtype=torch.int64, device=DEV)
  counts = torch.zeros(2, dtype=torch.int32, device=DEV)
  col = (_lib.HashColumn * 1)()
  col[0].keys_cache, col[0].slab_count, col[0].slab_size = keys.data_ptr(), slab_count, slab_size
  col[0].keys, col[0].n_keys, col[0].slots = d_ids.data_ptr(), ids.size, slots.data_ptr()
  col[0].counts = counts.data_ptr()
  col[0].table, col[0].dim, col[0].table_pitch, col[0].init_scale, col[0].seed = buf.data_ptr(), dim, pitch, 1.0, 11
  codes = (C.c_int32 * 1)(hb.embedding.hashtable.LOWP_DTYPES[dtype])
  _lib.check(_lib.lib().hbk_hash_insert_lowp_n(1, col, None, None, codes, 1, _lib.current_stream(torch.device(DEV))))
  torch.cuda.synchronize()
  s = slots.cpu().numpy()
  assert (s >= 0).all() and counts.tolist() == [100, 0]
  got = buf.cpu().numpy().view(np.uint16)
  np.testing.assert_array_equal(got[s, :dim], oracle(ids, dim, 11, 1.0, dtype))
  assert (got[:, dim:] == 0x7FFF).all(), 'the padding was written'
  free = np.ones(cap, bool)
  free[s] = False
  assert (got[free] == 0x7FFF).all(), 'a row no key took was written'


def test_a_mixed_translate_leaves_the_fp32_table_as_it_is_alone():
  rng = np.random.RandomState(21)
  ids = some_ids(rng)
  d_ids = dev(ids)
  mk = lambda **kw: hb.embedding.HashTable(1024, 16, DEV, seed=9, init_scale=1.0, **kw)   # noqa: E731
  alone = mk()
  alone.lookup_or_insert(d_ids)
  tables = [mk(), mk(dtype=torch.bfloat16), mk(dtype=torch.float16, expiring=True)]
  tables[2].set_step(5)
  slots = hb.embedding.hash_translate(tables, [d_ids] * 3)
  keys, rows = tables[0].items()
  akeys, arows = alone.items()
  assert torch.equal(keys, akeys)
  np.testing.assert_array_equal(bits32(rows), bits32(arows))
  assert tables[0].counts.tolist() == alone.counts.tolist() == [200, 0]
  for t, s in zip(tables[1:], slots[1:]):
    assert (s >= 0).all() and t.size() == 200
    np.testing.assert_array_equal(bits16(t.table[s]), oracle(ids, 16, 9, 1.0, t.dtype))
    assert int((bits16(t.table) != 0).any(axis=1).sum()) <= 200
  assert (tables[2].last_seen[slots[2]] == 5).all()
  # a find over the same mix
  found = hb.embedding.hash_translate(tables, [d_ids] * 3, insert=False)
  for a, b in zip(found, slots):
    assert torch.equal(a, b)


def fp32_lookup(tables32, ids, splits, weights, combiners, buckets=None):
  """GroupLookup over fp32 tables, the reference of every forward here.  hbk_group_lookup_fwd itself takes a row wider
  than 64 floats only when dim % 4 == 0, so such a table (dim 130) is handed to it as contiguous column blocks of 64
  floats with the column's ids, splits, weights and combiner, and the outputs are joined again: every output element
  is a sum over the ids of its own column of the table, so this is the same kernel computing the same elements."""
  cols, owner = [], []
  for c, t in enumerate(tables32):
    wide = t.shape[1] > 64 and t.shape[1] % 4 != 0
    for first in (range(0, t.shape[1], 64) if wide else [0]):
      cols.append(t[:, first:first + 64].contiguous() if wide else t)
      owner.append(c)
  pick = lambda x: None if x is None else [x[c] for c in owner]   # noqa: E731
  outs = GroupLookup(cols, buckets=pick(buckets), combiners=pick(combiners))(pick(ids), pick(splits),
                                                                             sp_weights=pick(weights))
  return [torch.cat([o for o, k in zip(outs, owner) if k == c], dim=1) for c in range(len(tables32))]


# ---- 2. the forward ---------------------------------------------------------------------------------------------
def ragged(rng, n_seg, longest=5):
  lens = rng.randint(0, longest + 1, size=n_seg)
  lens[[1, n_seg - 1]] = 0                    # empty segments, the last one too
  return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def forward_is_grouplookup_over_the_upcast_tables(dtype, dims):
  """3 columns, sum / mean / sqrtn, ragged splits with empty segments, sp_weights on one column: the call, launch()
  on refilled id buffers, call_block and train=False, each bit for bit GroupLookup over the upcast tables."""
  rng = np.random.RandomState(31)
  combiners, n_seg = ['sum', 'mean', 'sqrtn'], 40
  tables = [hb.embedding.HashTable(512, d, DEV, init_scale=1.0, seed=c + 1, dtype=dtype, expiring=c == 1)
            for c, d in enumerate(dims)]
  pools = [rng.randint(-2 ** 62, 2 ** 62, size=60, dtype=np.int64) for _ in dims]
  splits = [ragged(rng, n_seg) for _ in dims]
  draw = lambda c, pool: dev(pool[rng.randint(0, pool.size, size=int(splits[c][-1]))])   # noqa: E731
  ids = [draw(c, pools[c]) for c in range(3)]
  d_splits = [dev(s) for s in splits]
  weights = [None, dev(rng.uniform(-2, 2, size=int(splits[1][-1])).astype(F32)), None]

  def same_as_fp32(hgl, outs, what):
    want = fp32_lookup([t.table.float() for t in hgl.tables], hgl.slots, d_splits, weights, combiners)
    for c, (o, w) in enumerate(zip(outs, want)):
      assert o.dtype == torch.float32 and tuple(o.shape) == (n_seg, dims[c])
      np.testing.assert_array_equal(bits32(o), bits32(w), f'{what}: column {c}')

  hgl = hb.embedding.HashGroupLookup(tables, combiners=combiners)
  assert isinstance(hgl.lookup, LowpGroupLookup) and hgl.lookup.buckets == [0, 0, 0]
  outs = hgl(ids, d_splits, sp_weights=weights)
  assert all((s >= 0).all() for s in hgl.slots) and any(o.any() for o in outs)
  same_as_fp32(hgl, outs, 'call')
  # launch() after the id buffers were refilled in place: both launches again, new ids inserted
  more = [np.concatenate([p, rng.randint(-2 ** 62, 2 ** 62, size=20, dtype=np.int64)]) for p in pools]
  sizes = [t.size() for t in tables]
  for c in range(3):
    ids[c].copy_(draw(c, more[c]))
  hgl.launch()
  assert all(t.size() > n for t, n in zip(tables, sizes))
  same_as_fp32(hgl, outs, 'launch')
  # call_block: the bits of __call__
  offsets = [0, 8, 24]
  block = torch.full((n_seg, 24 + dims[2] + 4), 7.0, device=DEV)
  hgl.call_block(ids, d_splits, block, offsets, lambda: [block[:, o:o + d] for o, d in zip(offsets, dims)],
                 sp_weights=weights)
  again = hgl(ids, d_splits, sp_weights=weights)
  for c, (o, d) in enumerate(zip(offsets, dims)):
    np.testing.assert_array_equal(bits32(block[:, o:o + d]), bits32(again[c]), f'call_block: column {c}')
  assert (block[:, 6:8] == 7.0).all() and (block[:, -4:] == 7.0).all()
  # train=False: ids never seen read as zero rows and nothing is inserted
  sizes = [t.size() for t in tables]
  frozen = hb.embedding.HashGroupLookup(tables, combiners=combiners, train=False)
  unseen = [np.concatenate([p, rng.randint(-2 ** 62, 2 ** 62, size=40, dtype=np.int64)]) for p in more]
  ids2 = [draw(c, unseen[c]) for c in range(3)]
  outs2 = frozen(ids2, d_splits, sp_weights=weights)
  assert all((s == -1).any() and (s >= 0).any() for s in frozen.slots)
  assert [t.size() for t in tables] == sizes
  same_as_fp32(frozen, outs2, 'train=False')
  one = hb.embedding.HashGroupLookup(tables[:1], train=False)
  alone = one([dev(np.array([unseen[0][-1], pools[0][0]]))])[0]
  assert not alone[0].any() and alone[1].any()                 # a -1 slot is a zero row


@pytest.mark.parametrize('dims', [(6, 16, 130), (6, 16, 128)], ids=['130', '128'])
@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
def test_forward_is_grouplookup_over_the_upcast_tables(dtype, dims):
  """Dims 6 / 16 / 130: one element per lane below and at a power of two, and a row wider than a wave that is no
  multiple of four (served in column blocks of 64 elements).  6 / 16 / 128: the widest kind of row, 4 and 8 elements
  per lane."""
  forward_is_grouplookup_over_the_upcast_tables(dtype, dims)


@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
def test_wide_rows_go_in_column_blocks_and_no_bit_depends_on_it(dtype):
  """LowpGroupLookup(wide_rows=True), what HashGroupLookup builds: rows of one element per lane wider than 64, one id
  per segment and ragged, weighted, and more blocks than one launch holds (20 columns of 4 blocks)."""
  rng = np.random.RandomState(61)
  rows, n_seg = 50, 70
  dims = [65, 130, 255, 64, 6] + [193] * 20
  tables = [dev(rng.uniform(-2, 2, size=(rows, d)).astype(F32)).to(dtype) for d in dims]
  for ragged_ids in (False, True):
    splits = [ragged(rng, n_seg) for _ in dims] if ragged_ids else None
    n_ids = [int(s[-1]) for s in splits] if ragged_ids else [n_seg] * len(dims)
    ids = [dev(rng.randint(-3, rows + 3, size=n).astype(np.int64)) for n in n_ids]       # (invalid rows too)
    d_splits = [dev(s) for s in splits] if ragged_ids else None
    weights = [dev(rng.uniform(-2, 2, size=n).astype(F32)) if c % 2 else None for c, n in enumerate(n_ids)]
    combiners = [('sum', 'mean', 'sqrtn')[c % 3] for c in range(len(dims))]
    got = LowpGroupLookup(tables, buckets=[rows] * len(dims), combiners=combiners, wide_rows=True)(
      ids, d_splits, sp_weights=weights)
    want = fp32_lookup([t.float() for t in tables], ids, d_splits, weights, combiners, [rows] * len(dims))
    for c, (g, w) in enumerate(zip(got, want)):
      assert tuple(g.shape) == (n_seg, dims[c]) and g.any()
      np.testing.assert_array_equal(bits32(g), bits32(w), f'ragged {ragged_ids}: column {c} dim {dims[c]}')
  # without the flag the bound of the 16-bit forward stands, by name
  with pytest.raises(_lib.InvalidArgumentError, match='column 1: dim 130'):
    LowpGroupLookup([tables[3], tables[1]])([ids[0][:4], ids[1][:4]])


# ---- 3. the step ------------------------------------------------------------------------------------------------
SEED = 0x9E3779B1


@pytest.mark.parametrize('dtype', LOWP, ids=IDS)
def test_the_step_of_a_wide_row_that_is_no_multiple_of_four_is_refused_by_name(dtype):
  """The forward takes dim 130 in column blocks; the backward and the 16-bit apply keep their bound (rows wider than
  64 elements move 4 per lane): the step says so before it writes a row."""
  rng = np.random.RandomState(43)
  t = hb.embedding.HashTable(256, 130, DEV, init_scale=1.0, seed=5, dtype=dtype)
  hgl = hb.embedding.HashGroupLookup([t])
  ids = dev(rng.randint(-2 ** 62, 2 ** 62, size=32, dtype=np.int64))
  out = hgl([ids])[0]
  assert tuple(out.shape) == (32, 130) and out.any()
  before = bits16(t.table)
  step = LowpLookupGrad(hgl.lookup)
  with pytest.raises(_lib.InvalidArgumentError, match='dim 130'):
    step(hgl.slots, [dev(exact.exact_grads(rng, (32, 130), 6))], apply_lr=0.05)
  torch.cuda.synchronize()
  np.testing.assert_array_equal(bits16(t.table), before)


@pytest.mark.parametrize('optimizer', ['rowwise_adagrad', 'sgd'])
@pytest.mark.parametrize('dtype,rounding', [(torch.bfloat16, 'nearest'), (torch.bfloat16, 'stochastic'),
                                            (torch.float16, 'nearest')], ids=['bf16', 'bf16-stochastic', 'fp16'])
def test_three_steps_equal_the_restatement_per_key(dtype, rounding, optimizer):
  """Column 1 is filled on purpose (one slab of 8 slots, 20 ids): its -1 slots reach no row and no slot."""
  rng = np.random.RandomState(41)
  dims, caps, n_seg, lr = (6, 16), (512, 8), 48, 0.05
  tables = [hb.embedding.HashTable(cap, d, DEV, init_scale=1.0, seed=3, dtype=dtype) for cap, d in zip(caps, dims)]
  accs = [torch.full((t.capacity, 1), 0.1, device=DEV) for t in tables]
  hgl = hb.embedding.HashGroupLookup(tables, combiners='sum')
  kw = dict(row_accums=accs, rowwise_adagrad=RowwiseAdagrad()) if optimizer == 'rowwise_adagrad' else {}
  step = LowpLookupGrad(hgl.lookup, rounding=rounding, seed=SEED, **kw)
  pools = [rng.randint(-2 ** 62, 2 ** 62, size=n, dtype=np.int64) for n in (70, 20)]
  for k in range(3):
    splits = [ragged(rng, n_seg, 4) for _ in dims]
    ids = [dev(p[rng.randint(0, p.size, size=int(s[-1]))]) for p, s in zip(pools, splits)]
    d_splits = [dev(s) for s in splits]
    hgl(ids, d_splits)
    grads = [exact.exact_grads(rng, (n_seg, d), 6) for d in dims]
    before = [bits16(t.table) for t in tables]
    acc_before = [a.cpu().numpy() for a in accs]
    step(hgl.slots, [dev(g) for g in grads], d_splits, apply_lr=lr, optimizer=optimizer)
    torch.cuda.synchronize()
    for c, t in enumerate(tables):
      slots = hgl.slots[c].cpu().numpy()
      if c == 1:
        assert (slots == -1).any() and (slots >= 0).any() and t.size() == 8
      else:
        assert (slots >= 0).all()
      seg = np.repeat(np.arange(n_seg), np.diff(splits[c]))
      valid = slots >= 0
      rows = np.unique(slots[valid])
      sums = np.zeros((rows.size, dims[c]), np.float64)
      np.add.at(sums, np.searchsorted(rows, slots[valid]), grads[c][seg[valid]].astype(np.float64))
      assert (sums.astype(F32).astype(np.float64) == sums).all()         # the grid: exact in any order
      want, want_slots = lowp_ref.apply_step(
        before[c], NAMES[dtype], [acc_before[c]] if kw else [], rows, sums.astype(F32), optimizer, lr,
        hyper={'epsilon': 1e-8}, rounding=rounding, seed=SEED, step=k, col=c)
      np.testing.assert_array_equal(bits16(t.table), want, f'step {k} column {c}: table')
      assert (want[rows] != before[c][rows]).any()
      if kw:
        np.testing.assert_array_equal(accs[c].cpu().numpy().view(np.int32), want_slots[0].view(np.int32),
                                      f'step {k} column {c}: accumulator')
      else:
        np.testing.assert_array_equal(accs[c].cpu().numpy(), acc_before[c])
  assert int(step.step_counter) == (3 if rounding == 'stochastic' else 0)


# ---- 4. a life, against an fp32 twin ----------------------------------------------------------------------------
class Life:
  """One expiring table with one fp32 [capacity, 1] companion, a host tier, and the operations of the sequence."""

  def __init__(self, dim, dtype, capacity=1024, slab_size=8):
    self.dim, self.dtype = dim, dtype
    self.t = hb.embedding.HashTable(capacity, dim, DEV, slab_size=slab_size, init_scale=1.0, seed=17, expiring=True,
                                    dtype=dtype)
    self.acc = torch.full((self.t.capacity, 1), 0.1, device=DEV)
    self.store = hb.embedding.HashSpillStore(dim, (1,), dtype=dtype)

  def batch(self, ids, step):
    self.t.set_step(step)
    slots = self.t.lookup_or_insert(ids)
    assert (slots >= 0).all()
    self.acc[slots] = ((ids % 1000).float() + step).unsqueeze(1)

  def state(self):
    """(keys, rows, companion per key, counters), the keys ascending."""
    keys, rows = self.t.items()
    acc = self.acc[self.t.find(keys.contiguous())]
    return keys.cpu().numpy(), rows, acc.cpu().numpy(), (self.t.size(), self.t.evicted(), self.t.tombstones())


def same_life(low, twin, what):
  keys, rows, acc, counters = low.state()
  tkeys, trows, tacc, tcounters = twin.state()
  assert rows.dtype == low.dtype and trows.dtype == torch.float32
  np.testing.assert_array_equal(keys, tkeys, f'{what}: keys')
  np.testing.assert_array_equal(bits16(rows), bits16(trows.to(low.dtype)), f'{what}: rows')
  np.testing.assert_array_equal(acc.view(np.int32), tacc.view(np.int32), f'{what}: companion')
  assert counters == tcounters, (what, counters, tcounters)
  return keys


@pytest.mark.parametrize('dim,dtype', [(4, torch.bfloat16), (6, torch.bfloat16), (16, torch.bfloat16),
                                       (6, torch.float16)], ids=['bf16-4', 'bf16-6', 'bf16-16', 'fp16-6'])
def test_a_16_bit_table_lives_the_life_of_its_fp32_twin(dim, dtype):
  """Every table stays roomy, so the set of stored keys is the header's own rule and both tables hold the same."""
  rng = np.random.RandomState(dim)
  pool = rng.randint(-2 ** 62, 2 ** 62, size=240, dtype=np.int64)
  low, twin = Life(dim, dtype), Life(dim, torch.float32)
  both = (low, twin)
  assert low.t.table.element_size() == 2 and low.t.table.shape == twin.t.table.shape
  for step, part in ((1, pool[:120]), (2, pool[60:180]), (3, pool[150:200])):
    ids = dev(part[rng.randint(0, part.size, size=200)])
    for x in both:
      x.batch(ids, step)
    same_life(low, twin, f'batch {step}')
  # load: rows exactly representable in 16 bits, for new keys and for keys the tables hold
  lkeys = dev(np.concatenate([pool[200:220], pool[:5]]))
  lrows = (torch.randint(-64, 65, (25, dim), generator=torch.Generator().manual_seed(dim)).float() / 16).to(DEV)
  for x in both:
    x.t.load(lkeys, lrows.to(x.dtype))
  keys = same_life(low, twin, 'load')
  held = low.t.find(lkeys)
  np.testing.assert_array_equal(bits16(low.t.table[held]), bits16(lrows.to(dtype)))
  n0 = keys.size
  for x in both:
    x.t.set_step(4)
    x.t.evict(3, slots=[(x.acc, 0.1)])              # last seen at step 1
  assert 0 < same_life(low, twin, 'evict').size < n0
  assert low.t.tombstones() > 0
  for x in both:
    x.acc = x.t.rehash(capacity=2304, slab_size=16, slots=[(x.acc, 0.1)])[0]
  same_life(low, twin, 'rehash (growth)')
  assert low.t.table.dtype == dtype and (low.t.capacity, low.t.slab_size) == (2304, 16)
  for x in both:
    x.t.set_step(5)
    x.t.evict(3, slots=[(x.acc, 0.1)])              # ... at step 2: tombstones again
  assert low.t.tombstones() > 0
  for x in both:
    x.acc = x.t.rehash(slots=[(x.acc, 0.1)])[0]
  same_life(low, twin, 'rehash (compaction)')
  assert low.t.tombstones() == 0
  # two more steps, so that the table holds three ages: whole steps leave together
  for step, part in ((6, pool[:80]), (7, pool[40:120])):
    ids = dev(part[rng.randint(0, part.size, size=200)])
    for x in both:
      x.batch(ids, step)
  bound = same_life(low, twin, 'batches 6 and 7').size - 10
  for x in both:
    x.t.evict_to(bound, slots=[(x.acc, 0.1)])       # the keys of step 3 leave
  n1 = same_life(low, twin, 'evict_to').size
  assert 0 < n1 <= bound
  exports = [x.t.spill_to(n1 - 15, x.store, slots=[(x.acc, 0.1)]) for x in both]     # ... those of step 6
  assert exports[0].rows.dtype == dtype and len(exports[0]) == len(exports[1]) == len(low.store) > 0
  np.testing.assert_array_equal(bits16(exports[0].rows), bits16(exports[1].rows.to(dtype)))
  assert 0 < same_life(low, twin, 'spill_to').size <= n1 - 15
  back = dev(np.concatenate([exports[1].keys.cpu().numpy()[::2], pool[100:130]]))
  restored = [x.t.fault_in(back, x.store, slots=[x.acc]) for x in both]
  assert restored[0] == restored[1] > 0 and len(low.store) == len(twin.store) > 0
  same_life(low, twin, 'fault_in')
  for x in both:
    x.t.track_removals()
    x.t.remove(dev(np.concatenate([pool[60:80], pool[230:]])), slots=[(x.acc, 0.1)])
  keys = same_life(low, twin, 'remove')
  # a delta, imported into a fresh table of another geometry
  fresh = []
  for x in both:
    exp = x.t.export_items(since=7, slots=[x.acc])
    assert exp.rows.dtype == x.dtype and 0 < len(exp) < keys.size and exp.removed.numel() > 0
    y = Life(dim, x.dtype, capacity=600, slab_size=4)
    y.t.set_step(9)
    y.t.import_items(exp, slots=[(y.acc, 0.1)])
    order = torch.argsort(exp.keys)
    np.testing.assert_array_equal(bits16(y.t.items()[1]) if x is low else bits32(y.t.items()[1]),
                                  bits16(exp.rows[order]) if x is low else bits32(exp.rows[order]))
    fresh.append(y)
  same_life(fresh[0], fresh[1], 'import_items')
  # the saver's variables, copied into a table of the same geometry
  for x in both:
    y = Life(dim, x.dtype, capacity=x.t.capacity, slab_size=x.t.slab_size)
    src, dst = x.t.variables('t'), y.t.variables('t')
    assert dst['t/embedding_weights'].dtype == x.dtype and sorted(src) == sorted(dst)
    for name, value in src.items():
      dst[name].copy_(value)
    y.acc.copy_(x.acc)
    y.t.recount()
    a, b = x.state(), y.state()
    np.testing.assert_array_equal(a[0], b[0])
    bits = bits16 if x is low else bits32
    np.testing.assert_array_equal(bits(a[1]), bits(b[1]))
    np.testing.assert_array_equal(a[2], b[2])
    assert y.t.size() == x.t.size() and y.t.tombstones() == x.t.tombstones()
    fresh.append(y)
  same_life(fresh[2], fresh[3], 'variables')
