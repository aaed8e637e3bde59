"""Zero-padded sequence lookups on sharded tables, on the GPU: hbk_sequence_pack_n against its numpy restatement
(tests/support/sequence_pack_ref.py) bit for bit, captured into a graph, and the packed form through the sharded
step -- ShardedSequenceLookup over bucketed and hash-keyed drivers at W = 1 (a real communicator), 2 and 3
(host threads over Collective.local_world) against the one-rank zero-padded lookups, and SequenceFeatures with
``sharded_zero_padding=True``.  Gradients are on the exact grid (tests/support/exact.py): every sum is exact in
any order, so stepped tables and accumulators are compared bit for bit."""
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import (HashSequenceLookup, HashTable, SequenceLookup, SequenceLookupGrad,
                                         ShardedGroupLookup, ShardedHashGroupLookup, ShardedSequenceLookup,
                                         sequence_pack)
from tests.support import exact
from tests.support import sequence_pack_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
fc = hb.feature_column
GUARD = 0x5A5A5A5A5A5A5A5A
N_GUARD = 8
EMPTY, TOMBSTONE = -2 ** 63, -2 ** 63 + 1
LR = exact.EXACT_LR


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def run_world(world, fn, real=False):
  """fn(rank, comm) on `world` host threads, each on a stream of its own (``real``: one rank on a communicator
  made the way a job makes it); returns the per-rank results."""
  comms = [hb.distribute.Collective(world_size=1, rank=0)] if real else hb.distribute.Collective.local_world(world)
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


WORLDS = [(1, True), (2, False), (3, False)]
WORLD_IDS = ['W1-real', 'W2', 'W3']


# ---- 1. the op against the restatement --------------------------------------------------------------------
class Packed:
  """hbk_sequence_pack_n on N columns through the C ABI: packed_capacity at its bound min(n_ids, B * T), a guard
  behind it, every output filled with a value the op never writes."""

  def __init__(self, columns):
    n = len(columns)
    self.columns = columns
    self.cols, self.seqs, self.packs = (_lib.LookupColumn * n)(), (_lib.Sequence * n)(), (_lib.SequencePack * n)()
    self.keep, self.out = [], []
    for c, (ids, splits, T) in enumerate(columns):
      d_ids = dev(ids)
      d_sp = dev(splits) if splits is not None else None
      B = ids.shape[0] if splits is None else splits.shape[0] - 1
      cap = min(ids.shape[0], B * T)
      o = dict(packed=torch.full((cap + N_GUARD,), GUARD, dtype=torch.int64, device=DEV),
               pos=torch.full((B * T + 1 + N_GUARD,), -7, dtype=torch.int32, device=DEV),
               lengths=torch.full((B + N_GUARD,), -7, dtype=torch.int32, device=DEV),
               samp=torch.full((B + 1 + N_GUARD,), -7, dtype=torch.int32, device=DEV),
               total=torch.full((1 + N_GUARD,), -7, dtype=torch.int32, device=DEV), B=B, T=T, cap=cap)
      col, q, p = self.cols[c], self.seqs[c], self.packs[c]
      col.ids, col.n_ids = d_ids.data_ptr(), ids.shape[0]
      col.ids_dtype = _lib.INT64 if ids.dtype == np.int64 else _lib.INT32
      col.row_splits, col.n_segments = (d_sp.data_ptr() if d_sp is not None else None), B
      q.max_len, q.lengths = T, o['lengths'].data_ptr()
      p.packed, p.packed_capacity = o['packed'].data_ptr(), cap
      p.pos_splits, p.sample_splits, p.total = o['pos'].data_ptr(), o['samp'].data_ptr(), o['total'].data_ptr()
      self.keep.append((d_ids, d_sp))
      self.out.append(o)
    self.need = int(_lib.lib().hbk_sequence_pack_workspace_bytes(n, self.cols))
    self.work = torch.full((self.need + 64,), 0x5A, dtype=torch.uint8, device=DEV)

  def __call__(self):
    n = len(self.columns)
    _lib.check(_lib.lib().hbk_sequence_pack_n(n, self.cols, self.seqs, self.packs, self.work.data_ptr(), self.need,
                                              _lib.current_stream(torch.device(DEV))))

  def check(self, columns=None):
    """Every output of every column against the restatement, bit for bit; what lies behind them is intact."""
    for c, (ids, splits, T) in enumerate(columns if columns is not None else self.columns):
      o = self.out[c]
      packed, pos, lengths, samp, total = ref.pack_ref(ids, splits, T)
      B = o['B']
      what = f'column {c} (B {B}, T {T})'
      got_total = host(o['total'])
      assert got_total[0] == total and (got_total[1:] == -7).all(), what
      for name, want, n in (('pos', pos, B * T + 1), ('lengths', lengths, B), ('samp', samp, B + 1)):
        got = host(o[name])
        np.testing.assert_array_equal(got[:n], want, err_msg=f'{what}: {name}')
        assert (got[n:] == -7).all(), f'{what}: {name} written past its end'
      got = host(o['packed'])
      np.testing.assert_array_equal(got[:total], packed, err_msg=f'{what}: packed')
      assert (got[total:] == GUARD).all(), f'{what}: packed written at or past total'
    assert (host(self.work)[self.need:] == 0x5A).all(), 'the workspace was written past its size'


def mixed_lengths(rng, B, T):
  """0, values in 1..T and values above T; a sample longer than T as the last of a tile and the first of the next."""
  lens = rng.choice(np.array([0, 0, 1, T, max(T - 1, 1), T + 1, T + 3, 2 * T + 1]), size=B)
  if B >= 3:
    lens[:3] = [0, T, T + 1]
  for b in (255, 256, 511, 512):
    if b < B:
      lens[b] = T + 2
  return lens


def column(rng, B, T, lens=None, dtype=np.int64, no_splits=False):
  if no_splits:
    return (ids_of(rng, B, dtype), None, T)
  lens = mixed_lengths(rng, B, T) if lens is None else np.asarray(lens)
  splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
  return (ids_of(rng, int(splits[-1]), dtype), splits, T)


def ids_of(rng, n, dtype):
  if dtype == np.int32:
    ids = rng.randint(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
    if n >= 2:
      ids[:2] = [-1, -2 ** 31]
    return ids
  ids = rng.randint(-2 ** 62, 2 ** 62, size=n, dtype=np.int64)
  if n >= 2:
    ids[:2] = [-1, 2 ** 62]
  return ids


@pytest.mark.parametrize('B,T', [(1, 1), (7, 3), (256, 4), (257, 4), (513, 1), (70001, 2)])
def test_pack_equals_the_restatement(B, T):
  rng = np.random.RandomState(B + T)
  cols = [column(rng, B, T)]
  lens = np.diff(cols[0][1])
  if B >= 7:
    assert (lens == 0).any() and (lens > T).any() and ((lens >= 1) & (lens <= T)).any()
  if B > 256:
    assert lens[255] > T and lens[256] > T
  p = Packed(cols)
  p()
  p.check()
  # more tile sums than one pass of the scan workgroup takes
  assert B != 70001 or p.need // 4 > 256


def test_pack_edge_cases():
  rng = np.random.RandomState(7)
  cols = [column(rng, 300, 3, lens=np.zeros(300, np.int64)),            # all samples empty
          column(rng, 300, 3, lens=np.full(300, 5)),                    # every sample longer than T
          column(rng, 300, 2, dtype=np.int32),                          # int32 ids, negative ones: sign extension
          column(rng, 300, 2, no_splits=True),                          # one id per sample
          column(rng, 300, 1, dtype=np.int32, no_splits=True),
          column(rng, 0, 4, lens=np.zeros(0, np.int64)),                # B = 0 beside columns of other B and T
          column(rng, 5, 9),
          column(rng, 1000, 1)]
  p = Packed(cols)
  p()
  p.check()
  # the Python entry: the same outputs, packed narrowed to total
  packed, pos, lengths, samp = sequence_pack([dev(i) for i, _, _ in cols],
                                             [dev(s) if s is not None else None for _, s, _ in cols],
                                             [t for _, _, t in cols])
  for c, (ids, splits, T) in enumerate(cols):
    want = ref.pack_ref(ids, splits, T)
    assert packed[c].dtype == torch.int64 and packed[c].numel() == want[4]
    for got, w in zip((packed[c], pos[c], lengths[c], samp[c]), want):
      np.testing.assert_array_equal(host(got), w, err_msg=f'column {c}')


def test_pack_one_more_column_than_a_launch_group():
  rng = np.random.RandomState(8)
  cols = [column(rng, 3 + 5 * c, 1 + c % 4) for c in range(65)]
  cols[64] = column(rng, 300, 2)
  cols[10] = column(rng, 0, 2, lens=np.zeros(0, np.int64))
  p = Packed(cols)
  p()
  p.check()


def test_pack_row_splits_that_are_no_csr_stay_in_bounds():
  """Row splits that point outside the ids are not read (the element holds 0), negative lengths count as 0."""
  ids = np.arange(1, 7, dtype=np.int64)
  splits = np.array([4, 9, 7, 7, 2, 6], np.int32)     # lengths 5 (-> 3, ids 5, 6, then outside), -2, 0, -5, 4 (-> 3)
  p = Packed([(ids, splits, 3)])
  assert p.out[0]['cap'] == 6
  p()
  p.check()
  assert host(p.out[0]['packed'])[:6].tolist() == [5, 6, 0, 3, 4, 5]


def test_pack_captured_into_a_graph_follows_refilled_inputs():
  rng = np.random.RandomState(9)
  first = [column(rng, 300, 3), column(rng, 40, 2, dtype=np.int32)]
  p = Packed(first)
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      p()
  torch.cuda.synchronize()
  graph.replay()
  torch.cuda.synchronize()
  p.check()
  # other lengths, the same number of ids and samples: ids and row_splits refilled in place
  fresh = []
  for c, (ids, splits, T) in enumerate(first):
    lens = rng.permutation(np.diff(splits))
    sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    fresh.append((ids_of(rng, ids.shape[0], ids.dtype.type), sp, T))
    assert not np.array_equal(sp, splits)
    p.keep[c][0].copy_(dev(fresh[c][0]))
    p.keep[c][1].copy_(dev(sp))
    for name in ('packed', 'pos', 'lengths', 'samp', 'total'):
      p.out[c][name].fill_(GUARD if name == 'packed' else -7)
  graph.replay()
  torch.cuda.synchronize()
  p.check(fresh)


# ---- 2. sharded, bucketed ---------------------------------------------------------------------------------
BUCKETS, DIMS, TS, B_RANK = 64, (16, 5), (3, 4), 9


def seq_batches(rng, world, pool_of):
  """Per rank and column (ids, splits): lengths 0, 1..T and above T; ``pool_of(c)``: the ids to draw from."""
  out = []
  for _ in range(world):
    cols = []
    for c, T in enumerate(TS):
      lens = rng.randint(0, 2 * T + 2, size=B_RANK)
      lens[:3] = [0, T, T + 2]
      splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
      pool = pool_of(c)
      cols.append((pool[rng.randint(0, pool.size, size=int(splits[-1]))], splits))
    out.append(cols)
  return out


def whole_batch(batches, c):
  """Column c of every rank's batch, concatenated in rank order."""
  ids = np.concatenate([b[c][0] for b in batches])
  sp, base = [np.zeros(1, np.int64)], 0
  for b in batches:
    sp.append(b[c][1][1:].astype(np.int64) + base)
    base += int(b[c][1][-1])
  return ids, np.concatenate(sp).astype(np.int32)


def unaligned(a):
  """A device copy of `a` that starts 4 bytes past a 16-byte boundary."""
  flat = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
  view = flat[1:].view(a.shape)
  view.copy_(dev(a))
  assert view.data_ptr() % 16 == 4
  return view


@pytest.mark.parametrize('optimizer', ['sgd', 'adagrad'])
@pytest.mark.parametrize('world,real', WORLDS, ids=WORLD_IDS)
def test_sharded_bucketed_equals_the_one_rank_zero_padded_lookup(world, real, optimizer):
  rng = np.random.RandomState(100 + world)
  tables = [exact.exact_tables(rng, BUCKETS, d) for d in DIMS]
  pool = rng.randint(-10 ** 6, 10 ** 6, size=40).astype(np.int64)
  batches = seq_batches(rng, world, lambda c: pool)
  rows = [np.concatenate([ref.pack_ref(b[c][0], b[c][1], TS[c])[0] for b in batches]) % BUCKETS for c in range(2)]
  bits = [exact.exact_terms_budget(rows[c], 0, f'column {c}') for c in range(2)]
  grads = [[exact.exact_grads(rng, (B_RANK, TS[c], DIMS[c]), min(bits[c], 6)) for c in range(2)]
           for _ in range(world)]
  totals = [[ref.pack_ref(b[c][0], b[c][1], TS[c])[4] for c in range(2)] for b in batches]

  def rank(r, comm):
    shards = [dev(tables[0][r::world].copy()), unaligned(tables[1][r::world])]
    accums = [torch.full_like(shards[0], 0.1), unaligned(np.full_like(tables[1][r::world], 0.1))]
    drv = ShardedGroupLookup(shards, comm, buckets=[BUCKETS] * 2, combiners='sum', accums=accums)
    look = ShardedSequenceLookup(drv, TS)
    outs, lengths = look([dev(i) for i, _ in batches[r]], [dev(s) for _, s in batches[r]])
    assert [tuple(o.shape) for o in outs] == [(B_RANK, TS[c], DIMS[c]) for c in range(2)]
    outs, lengths = [host(o) for o in outs], [host(x) for x in lengths]
    owned = [int(_lib.lib().hbk_sharded_owned_ids(drv._plan(), c)) for c in range(2)]   # pylint: disable=protected-access
    look.backward([dev(g) for g in grads[r]], apply_lr=LR, optimizer=optimizer, emit=False)
    torch.cuda.current_stream().synchronize()
    res = dict(outs=outs, lengths=lengths, owned=owned, shards=[host(s) for s in shards],
               accums=[host(a) for a in accums])
    drv.close()
    return res

  res = run_world(world, rank, real)
  for c in range(2):
    ids, sp = whole_batch(batches, c)
    table = dev(tables[c])
    accum = torch.full_like(table, 0.1)
    lookup = SequenceLookup([table], [BUCKETS], max_lens=TS[c])
    (want,), (want_len,) = lookup([dev(ids)], [dev(sp)])
    want, want_len = host(want), host(want_len)
    got = np.concatenate([x['outs'][c] for x in res])
    exact.assert_bits_equal(got, want, f'forward, column {c}')
    np.testing.assert_array_equal(np.concatenate([x['lengths'][c] for x in res]), want_len)
    padding = np.arange(TS[c])[None, :] >= want_len[:, None]
    assert padding.any() and (got[padding].view(np.uint32) == 0).all()      # exactly +0.0
    # the owners received the effective ids, not W * B * T positions
    assert sum(x['owned'][c] for x in res) == sum(t[c] for t in totals) < world * B_RANK * TS[c]
    SequenceLookupGrad(lookup, accums=[accum])([dev(np.concatenate([g[c] for g in grads]))], apply_lr=LR,
                                               optimizer=optimizer, emit=False)
    for name, one in (('shards', table), ('accums', accum)):
      stitched = np.empty((BUCKETS, DIMS[c]), F32)
      for r in range(world):
        stitched[r::world] = res[r][name][c]
      exact.assert_bits_equal(stitched, host(one), f'{optimizer}: {name} of column {c}')
    assert not np.array_equal(host(table), tables[c])
    assert (optimizer == 'adagrad') == bool((host(accum) != F32(0.1)).any())


# ---- 3. sharded, hash-keyed -------------------------------------------------------------------------------
def by_key(table, tensors):
  keys = host(table.keys)
  live = (keys != EMPTY) & ((keys != TOMBSTONE) | (not table.expiring))
  arrays = [host(x) for x in tensors]
  return {int(keys[s]): tuple(np.array(a[s]) for a in arrays) for s in np.nonzero(live)[0]}


LATE = 424242      # an id that occurs only past T


@pytest.mark.parametrize('world,real', WORLDS, ids=WORLD_IDS)
def test_sharded_hash_equals_the_one_rank_zero_padded_lookup_by_key(world, real):
  rng = np.random.RandomState(200 + world)
  pool = np.unique(np.concatenate([rng.randint(-2 ** 62, 0, size=15, dtype=np.int64),
                                   rng.randint(2 ** 40, 2 ** 62, size=15, dtype=np.int64), [-1, 0, 7]]))
  steps = []
  for _ in range(3):
    batches = seq_batches(rng, world, lambda c: pool)
    for b in batches:
      for c, T in enumerate(TS):
        b[c][0][b[c][1][2] + T] = LATE          # sample 2 holds T + 2 ids: its position T is past T
    steps.append(batches)
  effective = [np.unique(np.concatenate([ref.pack_ref(b[c][0], b[c][1], TS[c])[0] for bs in steps for b in bs]))
               for c in range(2)]
  per_step = [np.concatenate([ref.pack_ref(b[c][0], b[c][1], TS[c])[0] for b in steps[0]]) for c in range(2)]
  bits = [exact.exact_terms_budget(per_step[c], 0, f'column {c}') - 1 for c in range(2)]
  grads = [[[exact.exact_grads(rng, (B_RANK, TS[c], DIMS[c]), min(bits[c], 6)) for c in range(2)]
            for _ in range(world)] for _ in steps]
  make = lambda: [HashTable(256, d, DEV, init_scale=0.05, seed=11 + c, expiring=True)   # noqa: E731
                  for c, d in enumerate(DIMS)]

  def rank(r, comm):
    tables = make()
    accums = [torch.full_like(t.table, 0.1) for t in tables]
    drv = ShardedHashGroupLookup(tables, comm, combiners='sum', accums=accums)
    look = ShardedSequenceLookup(drv, TS)
    for n, batches in enumerate(steps):
      for t in tables:
        t.set_step(n + 1)
      look([dev(i) for i, _ in batches[r]], [dev(s) for _, s in batches[r]])
      look.backward([dev(g) for g in grads[n][r]], apply_lr=LR, optimizer='adagrad', emit=False)
    torch.cuda.current_stream().synchronize()
    res = dict(state=[by_key(t, [t.table, a]) for t, a in zip(tables, accums)],
               failed=[t.failed() for t in tables], size=[t.size() for t in tables])
    drv.close()
    return res

  res = run_world(world, rank, real)
  tables = make()
  accums = [torch.full_like(t.table, 0.1) for t in tables]
  hsl = HashSequenceLookup(tables, list(TS))
  grad = SequenceLookupGrad(hsl, accums=accums)
  for n, batches in enumerate(steps):
    for t in tables:
      t.set_step(n + 1)
    whole = [whole_batch(batches, c) for c in range(2)]
    hsl([dev(i) for i, _ in whole], [dev(s) for _, s in whole])
    grad([dev(np.concatenate([g[c] for g in grads[n]])) for c in range(2)], apply_lr=LR, optimizer='adagrad',
         emit=False)
  for c in range(2):
    want = by_key(tables[c], [tables[c].table, accums[c]])
    got = {}
    for r, x in enumerate(res):
      assert not set(x['state'][c]) & set(got)
      assert all(k % world == r for k in x['state'][c])
      got.update(x['state'][c])
    # the union of the ranks' keys is exactly the distinct effective ids; an id that occurs only past T is nowhere
    assert set(got) == set(effective[c].tolist()) == set(want) and LATE not in got
    for k, (row, acc) in want.items():
      exact.assert_bits_equal(got[k][0], row, f'column {c}, row of key {k}')
      exact.assert_bits_equal(got[k][1], acc, f'column {c}, accumulator of key {k}')
    assert any((acc != F32(0.1)).any() for _, acc in want.values())
    assert all(x['failed'][c] == 0 for x in res)
    assert sum(x['size'][c] for x in res) == tables[c].size() == effective[c].size


# ---- 4. the layer -----------------------------------------------------------------------------------------
def layer_columns(dedup=False):
  return [fc.SequenceEmbeddingColumn('rep', 8, 6, 3),                                     # replicated, zero padded
          fc.SequenceEmbeddingColumn('pad', 3001, 16, 5, pad_id=2),                       # sharded, grid form
          fc.SequenceEmbeddingColumn('zp', 3001, 5, 4, dedup=dedup),                      # sharded, packed form
          fc.HashSequenceEmbeddingColumn('hist', 512, 8, 3, init_scale=0.05, seed=9)]     # hash, packed form


def test_layer_with_sharded_zero_padding(tmp_path):
  rng = np.random.RandomState(300)
  world, B = 2, 12
  cols = layer_columns()
  tables = [exact.exact_tables(rng, c.num_buckets, c.dimension) for c in cols[:3]]
  pool = np.unique(rng.randint(-2 ** 40, 2 ** 40, size=30, dtype=np.int64))
  batches = []
  for _ in range(world):
    feats = {}
    for col in cols:
      lens = rng.randint(0, 2 * col.max_len + 2, size=B)
      lens[:3] = [0, col.max_len, col.max_len + 2]
      splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
      n = int(splits[-1])
      ids = pool[rng.randint(0, pool.size, size=n)] if col.key == 'hist' else \
          rng.randint(-10 ** 6, 10 ** 6, size=n).astype(np.int64)
      feats[col.key] = (ids, splits)
    batches.append(feats)
  # (3001 rows and 24 positions per rank: a row repeats a few times at most; the hash pool repeats more)
  grads = [[exact.exact_grads(rng, (B, col.max_len, col.dimension), 6) for col in cols] for _ in range(world)]
  prefix = str(tmp_path / 'ckpt')
  barrier = threading.Barrier(world)

  def init_for(r):
    def init(col, rows, d):   # pylint: disable=unused-argument
      t = tables[[x.key for x in cols].index(col.key)]
      return dev((t[r::world] if rows != col.num_buckets else t).copy())
    return init

  def d_feats(f):
    return {k: (dev(i), dev(s)) for k, (i, s) in f.items()}

  def rank(r, comm):
    with pytest.raises(_lib.InvalidArgumentError, match='requires a pad_id'):
      fc.SequenceFeatures(layer_columns(), DEV, coll=comm, batch_size=B, init=init_for(r))
    res = {}
    for dedup in (False, True):
      layer = fc.SequenceFeatures(layer_columns(dedup), DEV, coll=comm, batch_size=B, init=init_for(r),
                                  initial_accumulator_value=0.1, sharded_zero_padding=True)
      assert layer.sharded == [False, True, True, True]
      outs, lengths = layer(d_feats(batches[r]))
      first = ([host(o) for o in outs], [host(x) for x in lengths])
      layer.backward([dev(g) for g in grads[r]], apply_lr=LR, optimizer='adagrad', emit=False)
      outs, _ = layer(d_feats(batches[r]))
      again = [host(o) for o in outs]
      torch.cuda.current_stream().synchronize()
      res[dedup] = dict(first=first, again=again, zp=host(layer.weights[2]), zp_acc=host(layer.accums[2]))
      if not dedup:
        layer.save(prefix, barrier=barrier.wait)
      layer.close()
    return res

  res = run_world(world, rank)
  whole = {col.key: whole_batch([[b[col.key]] for b in batches], 0) for col in cols}
  # forward: every column against its one-rank lookup over the logical table
  lookup = SequenceLookup([dev(t) for t in tables], [c.num_buckets for c in cols[:3]],
                          max_lens=[c.max_len for c in cols[:3]], pad_ids=[c.pad_id for c in cols[:3]])
  want, want_len = lookup([dev(whole[c.key][0]) for c in cols[:3]], [dev(whole[c.key][1]) for c in cols[:3]])
  table = HashTable(512, 8, DEV, init_scale=0.05, seed=9)
  (h_want,), (h_len,) = HashSequenceLookup([table], 3)([dev(whole['hist'][0])], [dev(whole['hist'][1])])
  want, want_len = [host(x) for x in want] + [host(h_want)], [host(x) for x in want_len] + [host(h_len)]
  for c, col in enumerate(cols):
    got = np.concatenate([x[False]['first'][0][c] for x in res])
    exact.assert_bits_equal(got, want[c], f'forward of {col.key}')
    np.testing.assert_array_equal(np.concatenate([x[False]['first'][1][c] for x in res]), want_len[c])
    if col.pad_id is None:
      padding = np.arange(col.max_len)[None, :] >= want_len[c][:, None]
      assert padding.any() and (got[padding].view(np.uint32) == 0).all(), col.key
  # the Adagrad step of the zero-padded sharded column against SequenceLookupGrad on one rank, bit for bit
  zp = dev(tables[2])
  zp_acc = torch.full_like(zp, 0.1)
  one = SequenceLookup([zp], [3001], max_lens=4)
  one([dev(whole['zp'][0])], [dev(whole['zp'][1])])
  SequenceLookupGrad(one, accums=[zp_acc])([dev(np.concatenate([g[2] for g in grads]))], apply_lr=LR,
                                           optimizer='adagrad', emit=False)
  for name, w in (('zp', zp), ('zp_acc', zp_acc)):
    stitched = np.empty((3001, 5), F32)
    for r in range(world):
      stitched[r::world] = res[r][False][name]
    exact.assert_bits_equal(stitched, host(w), name)
  assert not np.array_equal(host(zp), tables[2])
  # dedup=True on the zero-padded column: the same bits, forward and step
  for r in range(world):
    for c in range(len(cols)):
      exact.assert_bits_equal(res[r][True]['first'][0][c], res[r][False]['first'][0][c], f'dedup forward {c}')
      exact.assert_bits_equal(res[r][True]['again'][c], res[r][False]['again'][c], f'dedup, after the step {c}')
    exact.assert_bits_equal(res[r][True]['zp'], res[r][False]['zp'], 'dedup: shard')
    exact.assert_bits_equal(res[r][True]['zp_acc'], res[r][False]['zp_acc'], 'dedup: accumulator')
  # saved at W = 2, restored at W = 1 into a layer with the default argument: the same outputs on the same batch
  single = fc.SequenceFeatures(layer_columns(), DEV, initial_accumulator_value=0.1)
  single.restore(prefix)
  for r in range(world):
    outs, lengths = single(d_feats(batches[r]))
    for c, col in enumerate(cols):
      exact.assert_bits_equal(host(outs[c]), res[r][False]['again'][c], f'W = 1 restore: {col.key}, rank {r}')
      np.testing.assert_array_equal(host(lengths[c]), res[r][False]['first'][1][c])
