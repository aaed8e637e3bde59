"""hbk_hash_translate_sequence_n and HashSequenceLookup on the GPU.  Twin tables, as in test_gpu_hash_runs.py: table
A goes through the new entry, table B through ``hash_translate`` on the host-built EFFECTIVE id list (per sample its
first min(len, T) ids, then T - min(len, T) pad ids when there is a pad id).  Slot numbers are run-dependent;
everything else -- the key set of every slab (no slab overflows here), counts, stats, freq and last_seen per key,
the sketch, filter_counts -- must be equal.  Then the forward, the backward through SequenceLookupGrad, launch(),
a captured graph and a rehash."""
import numpy as np
import pytest
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import HashSequenceLookup
from hybridbackend_amd.embedding import HashTable
from hybridbackend_amd.embedding import SequenceLookupGrad
from hybridbackend_amd.embedding import hash_translate
from hybridbackend_amd.embedding import hash_translate_sequence
from tests.support import hash_ref as ref
from tests.support import sequence_ref as sref
from tests.support.sharded_hash_ref import keys_without_overflow
from tests.support.tolerance import assert_sums_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
KINDS = ['plain', 'expiring', 'admit', 'expiring_admit']
INT64_MIN = -2 ** 63
EXTRA = (-1, 0, 2 ** 63 - 1)
# (slab_size, slab_count, dim), T, B, ragged.  B * T = 111 and 259: T no power of two, B * T no multiple of a
# wave's pass (8 keys x 64 / 8 or 16 lanes); 101 x 7 = 707 positions: tiles (256 and 128 keys) and blocks end inside
# samples; the last column has one id per sample: T - 1 padding positions each.
COLUMNS = [((5, 60, 4), 3, 37, True), ((16, 20, 6), 7, 37, True), ((5, 60, 4), 7, 101, True),
           ((16, 20, 6), 3, 37, False)]
PADS = [-1, 2 ** 63 - 1, 0, -1]     # raw ids: -1 is an ordinary key


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def make_tables(kind, min_freq=2, columns=COLUMNS):
  return [HashTable(ss * sc, dim, DEV, slab_size=ss, init_scale=0.05, seed=3 + c, expiring='expiring' in kind,
                    min_freq=min_freq if 'admit' in kind else 0, sketch_width=4096)
          for c, ((ss, sc, dim), _, _, _) in enumerate(columns)]


def make_pools(rng, n=150, n_trunc=40, columns=COLUMNS):
  """Per column (looked-up pool with -1, 0 and 2^63 - 1 in it, truncated pool): disjoint, and together without a
  slab that overflows."""
  out = []
  for (ss, sc, _), _, _, _ in columns:
    keys = keys_without_overflow(rng, n + n_trunc, sc, ss, extra=EXTRA)
    out.append((keys[:n], keys[n:]))
  return out


def draw_column(rng, pool, trunc, T, B, ragged):
  """(ids, row_splits or None): lengths 0, 1, T - 1, T, T + 1 and 3 T all occur; a sample's first T ids come from
  `pool`, the ids past T from `trunc`."""
  if not ragged:
    return pool[rng.randint(0, pool.size, size=B)], None
  choice = np.array([0, 1, T - 1, T, T + 1, 3 * T])
  lens = np.concatenate([choice, choice[rng.randint(0, choice.size, size=B - choice.size)]])
  rng.shuffle(lens)
  ids = []
  for n in lens:
    ids.append(pool[rng.randint(0, pool.size, size=min(n, T))])
    ids.append(trunc[rng.randint(0, trunc.size, size=max(n - T, 0))])
  return np.concatenate(ids).astype(np.int64), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def effective(ids, splits, T, pad):
  """(E int64, where int64 [B * T]: the index into E of every position or -1, lengths int32 [B])."""
  sp = np.arange(ids.size + 1) if splits is None else splits.astype(np.int64)
  E, where, lengths = [], [], []
  for b in range(sp.size - 1):
    L = min(int(sp[b + 1] - sp[b]), T)
    lengths.append(L)
    for t in range(T):
      if t < L or pad is not None:
        where.append(len(E))
        E.append(int(ids[sp[b] + t]) if t < L else pad)
      else:
        where.append(-1)
  return np.array(E, np.int64), np.array(where, np.int64), np.array(lengths, np.int32)


def d_opt(x):
  return None if x is None else dev(x)


def per_key(table, array, keys):
  slots = host(table.find(dev(keys)))
  assert (slots >= 0).all()
  return host(array)[slots]


def assert_twins_equal(a, b, keys):
  """Table a (sequence entry) against table b (the existing entry on the effective list); keys: those stored."""
  assert ref.slab_sets(host(a.keys), a.slab_size) == ref.slab_sets(host(b.keys), b.slab_size)
  assert host(a.counts).tolist() == host(b.counts).tolist()
  np.testing.assert_array_equal(per_key(a, a.table, keys), per_key(b, b.table, keys))
  np.testing.assert_array_equal(per_key(a, a.table, keys), ref.init_rows(keys, a.dim, a.seed, a.init_scale))
  if a.expiring:
    assert host(a.stats).tolist() == host(b.stats).tolist()
    np.testing.assert_array_equal(per_key(a, a.freq, keys), per_key(b, b.freq, keys))
    np.testing.assert_array_equal(per_key(a, a.last_seen, keys), per_key(b, b.last_seen, keys))
  if a.min_freq:
    np.testing.assert_array_equal(host(a.sketch), host(b.sketch))
    assert host(a.filter_counts).tolist() == host(b.filter_counts).tolist()


def snapshot(t):
  arrays = [t.keys, t.table, t.counts]
  if t.expiring:
    arrays += [t.last_seen, t.freq, t.stats]
  if t.min_freq:
    arrays += [t.sketch, t.filter_counts]
  return [host(x).copy() for x in arrays]


def assert_unchanged(t, before):
  for x, y in zip(before, snapshot(t)):
    np.testing.assert_array_equal(x, y)


# ---- 1. the translate against its twin --------------------------------------------------------------------
@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('kind', KINDS)
def test_sequence_entry_equals_the_matching_entry_on_the_effective_ids(kind, padded):
  rng = np.random.RandomState(len(kind) + 7 * padded)
  pools = make_pools(rng)
  pads = PADS if padded else [None] * len(COLUMNS)
  T = [c[1] for c in COLUMNS]
  A, B = make_tables(kind), make_tables(kind)
  distinct = [set() for _ in COLUMNS]
  for step, sub in ((3, slice(0, 100)), (5, slice(50, 150))):      # the second call meets old keys and new ones
    data = [draw_column(rng, p[sub], tr, t, b, ragged) for (p, tr), (_, t, b, ragged) in zip(pools, COLUMNS)]
    if 'expiring' in kind:
      for t in A + B:
        t.set_step(step)
    grids, lengths = hash_translate_sequence(A, [dev(i) for i, _ in data], [d_opt(s) for _, s in data],
                                             max_lens=T, pad_ids=pads)
    eff = [effective(i, s, t, p) for (i, s), t, p in zip(data, T, pads)]
    want = hash_translate(B, [dev(e) for e, _, _ in eff])
    for c, (E, where, ln) in enumerate(eff):
      g, w = host(grids[c]), host(want[c])
      assert g.shape == (COLUMNS[c][2] * T[c],)
      np.testing.assert_array_equal(host(lengths[c]), ln)
      there = where >= 0
      if not padded:
        assert (~there).any()
      # padding without a pad id is -1; every answer names a slot that holds its effective id; the same positions
      # are -1 as in the twin (the filter's decision is reproducible; nothing fails: capacity >= the distinct keys)
      assert (g[~there] == -1).all()
      stored = g >= 0
      np.testing.assert_array_equal(host(A[c].keys)[g[stored]], E[where[stored]])
      np.testing.assert_array_equal(stored[there], w[where[there]] >= 0)
      if 'admit' not in kind:
        assert stored[there].all()
      assert A[c].failed() == 0
      kept = np.unique(E[where[stored]])
      assert_twins_equal(A[c], B[c], kept)
      if 'expiring' in kind:
        assert (per_key(A[c], A[c].last_seen, kept) == step).all()
      # truncated ids (a pool of their own) were never read: not stored, not counted
      assert (host(A[c].find(dev(pools[c][1]))) == -1).all()
      distinct[c] |= set(E.tolist()) if 'admit' not in kind else set(kept.tolist())
      assert A[c].size() == len(distinct[c]) == B[c].size()
      if 'admit' in kind:
        assert (host(A[c].estimate(dev(pools[c][1]))) == host(B[c].estimate(dev(pools[c][1])))).all()


# ---- 2. sentinels in the data, padding only, a find -------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_a_sentinel_in_the_data_fails_once_and_padding_counts_nothing(kind):
  rng = np.random.RandomState(21)
  columns = COLUMNS[:2]
  pools = make_pools(rng, 60, 10, columns)
  A = make_tables(kind, min_freq=1, columns=columns)
  for t in A:
    if t.expiring:
      t.set_step(1)
  # column 0 (T = 3): INT64_MIN at a looked-up position and at a truncated one (never read); on an expiring table
  # INT64_MIN + 1 as well.  Column 1: samples without ids only.
  p = pools[0][0]
  samples = [[p[0], INT64_MIN, p[1], INT64_MIN, INT64_MIN + 1], [p[2]], [], [p[3], INT64_MIN + 1], [p[4], p[5], p[6]]]
  ids = np.array([k for s in samples for k in s], np.int64)
  sp = np.concatenate([[0], np.cumsum([len(s) for s in samples])]).astype(np.int32)
  empty_sp = np.zeros(12, np.int32)
  for pads in ([None, None], [int(p[7]), None]):
    before = A[1].size(), A[1].failed()
    f0 = A[0].failed()
    grids, lengths = hash_translate_sequence(A, [dev(ids), dev(np.zeros(0, np.int64))], [dev(sp), dev(empty_sp)],
                                             max_lens=[3, 7], pad_ids=pads)
    g = host(grids[0]).reshape(5, 3)
    tomb = 'expiring' in kind
    assert A[0].failed() - f0 == (2 if tomb else 1)
    assert g[0, 1] == -1 and (g[3, 1] == -1) == tomb
    E, where, ln = effective(ids, sp, 3, pads[0])
    np.testing.assert_array_equal(host(lengths[0]), ln)
    ok = (where >= 0) & (g.reshape(-1) >= 0)
    np.testing.assert_array_equal(host(A[0].keys)[g.reshape(-1)[ok]], E[where[ok]])
    assert ok.sum() == (where >= 0).sum() - (2 if tomb else 1)
    # a column of padding only: -1 everywhere, lengths 0, and nothing counted anywhere
    assert (host(grids[1]) == -1).all() and host(grids[1]).size == 77 and not host(lengths[1]).any()
    assert (A[1].size(), A[1].failed()) == before == (0, 0)
    assert (host(A[1].keys) == INT64_MIN).all() and not host(A[1].table).any()
    if A[1].min_freq:
      assert A[1].filtered() == 0 and not host(A[1].sketch).any()
    if A[1].expiring:
      assert not host(A[1].freq).any() and not host(A[1].last_seen).any()
  # ... while a pad id there is an id like any other: one key, seen at every position
  hash_translate_sequence(A[1:], [dev(np.zeros(0, np.int64))], [dev(empty_sp)], max_lens=[7], pad_ids=[-1])
  assert A[1].size() == 1 and A[1].failed() == 0
  if A[1].expiring:
    assert per_key(A[1], A[1].freq, np.array([-1], np.int64)).tolist() == [77]
  # B == 0 and no columns
  g, ln = hash_translate_sequence(A[:1], [dev(np.zeros(0, np.int64))], [dev(np.zeros(1, np.int32))], max_lens=4)
  assert g[0].numel() == 0 and ln[0].numel() == 0
  assert hash_translate_sequence([], [], max_lens=3) == ([], [])


@pytest.mark.parametrize('kind', KINDS)
def test_a_find_changes_no_array_of_the_table(kind):
  rng = np.random.RandomState(5)
  pools = make_pools(rng, 60, 10)
  T = [c[1] for c in COLUMNS]
  A = make_tables(kind, min_freq=1)
  for t in A:
    if t.expiring:
      t.set_step(2)
  data = [draw_column(rng, p, tr, t, b, ragged) for (p, tr), (_, t, b, ragged) in zip(pools, COLUMNS)]
  d_ids, d_sp = [dev(i) for i, _ in data], [d_opt(s) for _, s in data]
  before = [snapshot(t) for t in A]
  grids, _ = hash_translate_sequence(A, d_ids, d_sp, max_lens=T, pad_ids=PADS, insert=False)
  for c, t in enumerate(A):
    assert (host(grids[c]) == -1).all()
    assert_unchanged(t, before[c])
  # after an insert the find answers what the insert answered, through the function and through train=False
  first, ln = hash_translate_sequence(A, d_ids, d_sp, max_lens=T, pad_ids=PADS)
  first = [host(g).copy() for g in first]
  before = [snapshot(t) for t in A]
  again, ln2 = hash_translate_sequence(A, d_ids, d_sp, max_lens=T, pad_ids=PADS, insert=False)
  hsl = HashSequenceLookup(A, T, pad_ids=PADS, train=False)
  outs, ln3 = hsl(d_ids, d_sp)
  for c, t in enumerate(A):
    np.testing.assert_array_equal(host(again[c]), first[c])
    np.testing.assert_array_equal(host(hsl.grids[c]), first[c])
    np.testing.assert_array_equal(host(ln2[c]), host(ln[c]))
    np.testing.assert_array_equal(host(ln3[c]), host(ln[c]))
    assert_unchanged(t, before[c])
    want = sref.forward_ref(host(t.table), first[c], T[c])
    np.testing.assert_array_equal(host(outs[c]), want)


# ---- 3. the forward ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def case():
  """One batch of the four columns for the forward / backward tests, and its effective ids without and with pads."""
  rng = np.random.RandomState(33)
  pools = make_pools(rng, 100, 20)
  T = [c[1] for c in COLUMNS]
  data = [draw_column(rng, p, tr, t, b, ragged) for (p, tr), (_, t, b, ragged) in zip(pools, COLUMNS)]
  grads = [rng.randn(b, t, dim).astype(F32) for (_, _, dim), t, b, _ in COLUMNS]
  return dict(T=T, data=data, grads=grads, pools=pools,
              eff={False: [effective(i, s, t, None) for (i, s), t in zip(data, T)],
                   True: [effective(i, s, t, p) for (i, s), t, p in zip(data, T, PADS)]})


def call(hsl, case):
  return hsl([dev(i) for i, _ in case['data']], [d_opt(s) for _, s in case['data']])


@pytest.mark.parametrize('padded', [False, True])
def test_forward_rows_are_the_initial_rows_of_the_effective_ids(case, padded):
  tables = make_tables('plain')
  pads = PADS if padded else None
  hsl = HashSequenceLookup(tables, case['T'], pad_ids=pads)
  outs, lengths = call(hsl, case)
  for c, (E, where, ln) in enumerate(case['eff'][padded]):
    t = tables[c]
    B, T = COLUMNS[c][2], case['T'][c]
    assert tuple(outs[c].shape) == (B, T, t.dim)
    np.testing.assert_array_equal(host(lengths[c]), ln)
    o = host(outs[c]).reshape(B * T, t.dim)
    there = where >= 0
    np.testing.assert_array_equal(o[there], ref.init_rows(E[where[there]], t.dim, t.seed, t.init_scale))
    assert not o[~there].any()
    assert t.size() == np.unique(E).size and t.failed() == 0
    if padded:
      at_pad = (np.arange(T)[None, :] >= ln[:, None]).reshape(-1)
      assert at_pad.any()
      slot = int(t.find(dev(np.array([PADS[c]], np.int64))).item())
      assert slot >= 0 and (host(hsl.grids[c])[at_pad] == slot).all()
      np.testing.assert_array_equal(o[at_pad], np.broadcast_to(host(t.table)[slot], (int(at_pad.sum()), t.dim)))


def test_forward_max_norms_clip_every_looked_up_row(case):
  tables = make_tables('plain')
  norms = [0.04, None, 0.05, 0.05]     # rows are uniform in [-0.05, 0.05): most norms lie above
  hsl = HashSequenceLookup(tables, case['T'], pad_ids=PADS, max_norms=norms)
  outs, _ = call(hsl, case)
  for c, t in enumerate(tables):
    grid = host(hsl.grids[c])
    if norms[c] is None:
      np.testing.assert_array_equal(host(outs[c]), sref.forward_ref(host(t.table), grid, case['T'][c]))
      continue
    want, mag = sref.forward_ref(host(t.table), grid, case['T'][c], max_norm=norms[c])
    assert_sums_close(host(outs[c]), want, mag, err_msg=f'clipped column {c}')
    n = np.sqrt((host(outs[c]).astype(np.float64) ** 2).sum(-1))
    assert (n <= norms[c] * (1 + 1e-5)).all() and (n > norms[c] * 0.99).any()


# ---- 4. the backward through SequenceLookupGrad -----------------------------------------------------------
def _slices(res):
  urows, grows, nu = res
  k = int(nu.item())
  return host(urows)[:k], host(grows)[:k]


@pytest.mark.parametrize('padded', [False, True])
def test_backward_emit_against_the_f64_scatter_over_the_slot_grid(case, padded):
  tables = make_tables('plain')
  hsl = HashSequenceLookup(tables, case['T'], pad_ids=PADS if padded else None)
  call(hsl, case)
  grad = SequenceLookupGrad(hsl)
  d_grads = [dev(g) for g in case['grads']]
  res = [_slices(r) for r in grad(d_grads)]                         # (read before the next call: one workspace)
  det = [_slices(r) for r in grad(d_grads, deterministic=True)]
  for c, t in enumerate(tables):
    grid, g = host(hsl.grids[c]), case['grads'][c]
    u, want, mag = sref.grad_ref(grid, g, t.capacity)
    got_rows, got = res[c]
    assert (got_rows >= 0).all()                                    # no unique_rows entry is negative
    order = np.argsort(got_rows)
    np.testing.assert_array_equal(got_rows[order], u)
    assert_sums_close(got[order], want, mag, err_msg=f'emit column {c}')
    # the rows that collect a gradient are the slots of the effective ids: truncated ids and zero padding reach none
    E, where, ln = case['eff'][padded][c]
    np.testing.assert_array_equal(np.sort(host(t.keys)[u]), np.unique(E))
    det_rows, det_sums = det[c]
    u32, s32 = sref.grad_seq32(grid, g, t.capacity)
    np.testing.assert_array_equal(det_rows, u32)
    np.testing.assert_array_equal(det_sums, s32)
    if padded:
      # the pad id's slot: every padding position, beside the positions where the data names the same id
      slot = int(t.find(dev(np.array([PADS[c]], np.int64))).item())
      same = (E[where] == PADS[c])
      w = g.reshape(-1, t.dim)[same].astype(np.float64)
      at_pad = (np.arange(case['T'][c])[None, :] >= ln[:, None]).reshape(-1)
      assert at_pad.sum() > 0 and same[at_pad].all()
      k = got_rows.tolist().index(slot)
      assert_sums_close(got[k], w.sum(0), np.abs(w).sum(0), err_msg=f'pad row column {c}')


@pytest.mark.parametrize('optimizer', ['sgd', 'adagrad'])
def test_backward_steps_against_the_f64_scatter_over_the_slot_grid(case, optimizer):
  tables = make_tables('plain')
  hsl = HashSequenceLookup(tables, case['T'], pad_ids=PADS)
  call(hsl, case)
  acc0, lr = 0.1, 0.05
  accums = [torch.full_like(t.table, acc0) for t in tables]
  before = [host(t.table).copy() for t in tables]
  SequenceLookupGrad(hsl, accums=accums)([dev(g) for g in case['grads']], apply_lr=lr, optimizer=optimizer)
  for c, t in enumerate(tables):
    u, g64, gmag = sref.grad_ref(host(hsl.grids[c]), case['grads'][c], t.capacity)
    want = before[c].astype(np.float64)
    mag = np.abs(want)
    if optimizer == 'sgd':
      want[u] -= lr * g64
      mag[u] += lr * gmag
    else:
      # acc' = acc + g^2, w' = w - lr * g / sqrt(acc').  With |g32 - g64| <= e = rel * sum|terms|:
      # |g32^2 - g64^2| <= e * (2 |g| + e) <= 2 rel * sum|terms|^2 (+ e^2), and the update lr * g / sqrt(acc + g^2)
      # has slope lr * acc / (acc + g^2)^1.5 <= lr / sqrt(acc0) in g, so it moves by at most lr * e / sqrt(acc0);
      # its own roundings (a square root, a division, a product) are relative to |update| <= lr.
      a_want = np.full(before[c].shape, acc0, np.float64)
      a_mag = a_want.copy()
      a_want[u] += g64 * g64
      a_mag[u] += 2.0 * gmag * gmag
      assert_sums_close(host(accums[c]), a_want, a_mag, err_msg=f'accumulator column {c}')
      want[u] -= lr * g64 / np.sqrt(a_want[u])
      mag[u] += lr * (gmag / np.sqrt(acc0) + 1.0)
    assert_sums_close(host(t.table), want, mag, err_msg=f'{optimizer} step column {c}')
    # rows no effective id owns keep their bits
    free = np.setdiff1d(np.arange(t.capacity), u)
    np.testing.assert_array_equal(host(t.table)[free], before[c][free])
    assert (host(accums[c])[free] == F32(acc0)).all()
    assert not np.array_equal(host(t.table)[u], before[c][u])


# ---- 5. launch(), a captured graph, a rehash --------------------------------------------------------------
def _resident(kind, seed):
  """Two columns (one ragged with pads, one with one id per sample) on buffers that are refilled in place: the
  batches share their sizes, not their ids or lengths."""
  rng = np.random.RandomState(seed)
  columns = [COLUMNS[1], COLUMNS[3]]
  pools = make_pools(rng, 150, 20, columns)
  T, pads = [7, 3], [-1, None]
  lens0 = draw_column(rng, pools[0][0], pools[0][1], 7, 37, True)[1]
  lens0 = np.diff(lens0)

  def batch():
    lens = rng.permutation(lens0)
    ids = []
    for n in lens:
      ids.append(pools[0][0][rng.randint(0, 150, size=min(n, 7))])
      ids.append(pools[0][1][rng.randint(0, 20, size=max(n - 7, 0))])
    return [(np.concatenate(ids).astype(np.int64), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)),
            (pools[1][0][rng.randint(0, 150, size=37)], None)]
  return columns, T, pads, batch


def _check_resident(hsl, tables, outs, data, T, pads, columns, seen):
  """The bound buffers after a launch on `data`, against a fresh call on twin tables that saw the same batches."""
  for c, (i, s) in enumerate(data):
    E, where, ln = effective(i, s, T[c], pads[c])
    g = host(hsl.grids[c])
    there = where >= 0
    assert (g[~there] == -1).all() and (g[there] >= 0).all()
    np.testing.assert_array_equal(host(tables[c].keys)[g[there]], E[where[there]])
    np.testing.assert_array_equal(host(hsl.lengths[c]), ln)
    seen[c] |= set(E.tolist())
    assert tables[c].size() == len(seen[c]) and tables[c].failed() == 0
    o = host(outs[c]).reshape(-1, tables[c].dim)
    np.testing.assert_array_equal(o[there], ref.init_rows(E[where[there]], tables[c].dim, tables[c].seed, 0.05))
    assert not o[~there].any()


def test_launch_after_a_refill_in_place_equals_a_fresh_call_on_a_twin():
  columns, T, pads, batch = _resident('plain', 40)
  A, B = make_tables('plain', columns=columns), make_tables('plain', columns=columns)
  hsl, twin = HashSequenceLookup(A, T, pad_ids=pads), HashSequenceLookup(B, T, pad_ids=pads)
  with pytest.raises(_lib.HbkError, match='launch'):
    hsl.launch()
  first = batch()
  bufs = [(dev(i), d_opt(s)) for i, s in first]
  outs, _ = hsl([i for i, _ in bufs], [s for _, s in bufs])
  twin([dev(i) for i, _ in first], [d_opt(s) for _, s in first])
  seen = [set(), set()]
  _check_resident(hsl, A, outs, first, T, pads, columns, seen)
  grids = [g.data_ptr() for g in hsl.grids]
  for _ in range(2):
    new = batch()
    for (bi, bs), (i, s) in zip(bufs, new):
      bi.copy_(dev(i))
      if s is not None:
        bs.copy_(dev(s))
    for o in outs:
      o.fill_(float('nan'))
    hsl.launch()
    t_outs, t_len = twin([dev(i) for i, _ in new], [d_opt(s) for _, s in new])
    assert [g.data_ptr() for g in hsl.grids] == grids
    _check_resident(hsl, A, outs, new, T, pads, columns, seen)
    for c in range(2):
      np.testing.assert_array_equal(host(outs[c]), host(t_outs[c]))
      np.testing.assert_array_equal(host(hsl.lengths[c]), host(t_len[c]))
      assert ref.slab_sets(host(A[c].keys), A[c].slab_size) == ref.slab_sets(host(B[c].keys), B[c].slab_size)
      assert host(A[c].counts).tolist() == host(B[c].counts).tolist()
      np.testing.assert_array_equal(host(A[c].keys)[host(hsl.grids[c])], host(B[c].keys)[host(twin.grids[c])])


@pytest.mark.parametrize('kind', ['plain', 'expiring_admit'])
def test_captured_launch_translates_the_replays_ids(kind):
  columns, T, pads, batch = _resident(kind, 41)
  A = make_tables(kind, min_freq=1, columns=columns)
  for t in A:
    if t.expiring:
      t.set_step(1)
  hsl = HashSequenceLookup(A, T, pad_ids=pads)
  first = batch()
  bufs = [(dev(i), d_opt(s)) for i, s in first]
  outs, _ = hsl([i for i, _ in bufs], [s for _, s in bufs])   # warm-up outside the capture: the buffers exist
  torch.cuda.synchronize()
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(side):
    with torch.cuda.graph(graph, stream=side):
      hsl.launch()
  torch.cuda.synchronize()
  seen = [set(), set()]
  for c, (i, s) in enumerate(first):
    seen[c] |= set(effective(i, s, T[c], pads[c])[0].tolist())
  new = batch()
  for (bi, bs), (i, s) in zip(bufs, new):
    bi.copy_(dev(i))
    if s is not None:
      bs.copy_(dev(s))
  for o in outs:
    o.fill_(float('nan'))
  graph.replay()
  torch.cuda.synchronize()
  _check_resident(hsl, A, outs, new, T, pads, columns, seen)


def test_a_rehash_needs_a_rebind():
  rng = np.random.RandomState(50)
  table = HashTable(64, 4, DEV, slab_size=8, init_scale=0.05, seed=9)
  hsl = HashSequenceLookup([table], 3, pad_ids=7)
  # (56 distinct keys; not rng.choice(2 ** 40, replace=False), which permutes the whole range on the host)
  keys = rng.permutation(np.unique(rng.randint(100, 2 ** 40, size=64, dtype=np.int64)))[:56]
  assert keys.size == 56
  sp = dev(np.arange(0, 57, 4).astype(np.int32))          # 14 samples of 4 ids: T = 3 reads 42 of them
  hsl([dev(keys)], [sp])
  E, where, ln = effective(keys, host(sp), 3, 7)
  assert table.size() == np.unique(E).size == 42 and table.failed() == 0
  # nothing to do below the load: the lookup stays bound
  assert hsl.maybe_grow(max_load=0.75) == [None]
  hsl.launch()
  assert table.maybe_grow(max_load=0.5) is not None and table.capacity == 128
  with pytest.raises(_lib.InvalidArgumentError, match='rebind'):
    hsl([dev(keys)], [sp])
  with pytest.raises(_lib.InvalidArgumentError, match='rebind'):
    hsl.launch()
  hsl.rebind()
  with pytest.raises(_lib.HbkError, match='launch'):
    hsl.launch()
  outs, lengths = hsl([dev(keys)], [sp])
  g = host(hsl.grids[0])
  np.testing.assert_array_equal(host(table.keys)[g], E[where])
  np.testing.assert_array_equal(host(lengths[0]), ln)
  np.testing.assert_array_equal(host(outs[0]).reshape(-1, 4), ref.init_rows(E[where], 4, 9, 0.05))
  assert table.size() == 42 and hsl.tables[0] is table.table
  # through the lookup's own maybe_grow the rebind is made
  assert hsl.maybe_grow(max_load=0.25)[0] is not None and table.capacity == 256
  outs, _ = hsl([dev(keys)], [sp])
  np.testing.assert_array_equal(host(table.keys)[host(hsl.grids[0])], E[where])
  np.testing.assert_array_equal(host(outs[0]).reshape(-1, 4), ref.init_rows(E[where], 4, 9, 0.05))
