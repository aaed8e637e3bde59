"""The backward's reduce plans checked BIT FOR BIT (tests/support/exact.py): every gradient term lies on a
grid fine enough, and small enough, that fp32 sums are exact in any order -- so the default
(run-dependent) plans must give exactly the float64 scatter-add, and one pair lost, doubled or added to
the wrong row at a chunk, share, range or merge boundary changes bits.  The columns are the smallest that
reach each path: one hot row of one / exactly one / just over one / several chunks of 2048 pairs, tables
of a few rows, a Zipf head over wide rows, ids on either side of every multiple of 16384 rows, ragged mean
at the length limit, narrow and odd dims, ids outside the table, empty columns, a sparse batch over a
large table; over them the switches that choose or shape a plan.  With exact sums the optimizer steps
are bit-checkable against their references (oracle.sparse_sgd_apply / sparse_adagrad_apply, np_adam,
np_ftrl) in emit AND step-only mode, in every row.  Sequence columns (the pad row) and the sharded
owner reduce (in-process worlds) the same way.  max_norm is left out: the clip divides by a norm."""
import threading

import numpy as np
import pytest
import torch

import oracle
import hybridbackend_amd as hb
from hybridbackend_amd.embedding import (Ftrl, GroupLookup, GroupLookupGrad, LazyAdam, SequenceLookup,
                                         SequenceLookupGrad)
from hybridbackend_amd.embedding.sharded import ShardedGroupLookup
from tests.support import exact
from tests.support import sequence_ref
from tests.test_gpu_adam import B1, B2, np_adam
from tests.test_gpu_ftrl import np_ftrl

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
LR = exact.EXACT_LR
ACCUM0 = 0.1
FTRL = Ftrl(l1=2.0, l2=1e-5)               # lr_power -0.5: the form the FTRL tests pin bit for bit
K_SPAN = 16384                             # kRsSpan: rows per bucket range of the row-sorted reduce


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


# ---- columns and their exact references (computed once per session, never changed) -------------------
class Column:
  """One column: inputs on the exact grid and the float64 reference of its gradient sums."""

  def __init__(self, name, dim, rows, ids, comb='sum', splits=None, weights=None, seed=0, fp16=False):
    rng = np.random.RandomState(seed)
    self.name, self.dim, self.rows, self.comb = name, dim, rows, comb
    self.ids = np.asarray(ids, np.int64)
    self.splits = None if splits is None else np.asarray(splits, np.int32)
    self.weights = None if weights is None else np.asarray(weights, F32)
    n_seg = self.ids.size if self.splits is None else self.splits.size - 1
    valid = (self.ids >= 0) & (self.ids < rows)
    longest = 1 if self.splits is None else int(np.diff(self.splits).max(initial=0))
    bits = exact.exact_terms_budget(self.ids[valid], exact.factor_bits(comb, longest, weights is not None),
                                    case=name)
    # (an fp16 wire holds 11 significant bits: 7 of value, 3 of weights at the most)
    self.grads = exact.exact_grads(rng, (n_seg, dim), min(bits, 6 if fp16 else 12))
    self.table = exact.exact_tables(rng, rows, dim)
    terms = exact.id_terms(self.grads, self.splits, comb, self.weights)
    self.want = exact.exact_dense((rows, dim), self.ids[valid], terms[valid], fp16=fp16, case=name)
    self._steps = {}

  def stepped(self, optimizer):
    """(table, slot, slot, ...) after one step of `optimizer` on the EXACT sums, from state0()."""
    if optimizer not in self._steps:
      w, a, b = (x.copy() for x in self.state0(optimizer))
      u, g = self.want.rows, self.want.sums()
      if optimizer == 'sgd':
        w = exact.exact_sgd(self.table, self.want, LR, case=self.name)     # asserts the step is exact
        np.testing.assert_array_equal(oracle.sparse_sgd_apply(self.table.copy(), u, g, LR), w)
      elif optimizer == 'adagrad':
        oracle.sparse_adagrad_apply(w, a, u, g, LR)
      elif optimizer == 'adam':
        np_adam(w, a, b, u, g, LR, B1, B2)
      else:
        np_ftrl(w, a, b, u, g, LR, FTRL)
      self._steps[optimizer] = (w, a, b)
    return self._steps[optimizer]

  def state0(self, optimizer):
    """(table, slot a, slot b) before the step; unused slots are zeros."""
    rng = np.random.RandomState(len(self.name) + self.dim)
    z = np.zeros_like(self.table)
    if optimizer == 'adagrad':
      return self.table, np.full_like(self.table, ACCUM0), z
    if optimizer == 'adam':
      return (self.table, rng.uniform(-0.1, 0.1, size=z.shape).astype(F32),
              rng.uniform(0, 0.01, size=z.shape).astype(F32))
    if optimizer == 'ftrl':
      return (self.table, rng.uniform(0.1, 1, size=z.shape).astype(F32),
              rng.uniform(-4, 4, size=z.shape).astype(F32))
    return self.table, z, z


def _ragged_ids(rng, n_seg, comb, max_len, draw):
  sp = exact.exact_ragged(rng, n_seg, comb, max_len)
  return sp, draw(int(sp[-1]))


def _boundary_ids(rng, rows, n):
  """Mostly the rows on either side of every multiple of the bucket span, row 0 and the last row."""
  edges = [0, rows - 1]
  for m in range(K_SPAN, rows + 1, K_SPAN):
    edges += [r for r in (m - 2, m - 1, m, m + 1) if 0 <= r < rows]
  edges = np.unique(np.array(edges, np.int64))
  return np.where(rng.rand(n) < 0.7, rng.choice(edges, size=n), rng.randint(0, rows, size=n)).astype(np.int64)


_SUITES = {}


def suite(name):
  if name not in _SUITES:
    _SUITES[name] = {'plain': _plain_columns, 'ragged': _ragged_columns, 'weighted': _weighted_columns}[name]()
  return _SUITES[name]


def _plain_columns():
  """One id per sample, no weights: launch groups of plain columns only."""
  rng = np.random.RandomState(2024)
  cols = []
  # one hot row: a run that crosses every share; a job of one, exactly one, just over one, several chunks
  for dim in (16, 128):
    for n in (2047, 2048, 2049, 4096, 3 * 2048 + 17):
      cols.append(Column(f'hot{n}x{dim}', dim, 64, np.full(n, 5, np.int64), seed=n + dim))
  # Zipf head over wide rows: the head splits its bucket (ranges, then the merge of partial entries)
  cols.append(Column('zipf700x128', 128, 700, rng.zipf(1.2, size=20000) % 700, seed=1))
  # ids on either side of every bucket-range boundary
  for rows in (K_SPAN - 1, K_SPAN, K_SPAN + 1, 2 * K_SPAN + 1):
    cols.append(Column(f'edges{rows}', 8, rows, _boundary_ids(rng, rows, 9000), seed=rows))
  # narrow and odd dims, dim 256, the dim-16 instantiation: Zipf over 500 rows, more than one tile
  for dim in (1, 3, 6, 20, 16, 256):
    cols.append(Column(f'dim{dim}', dim, 500, rng.zipf(1.3, size=3000) % 500, seed=dim))
  # ids outside the table (no bucket): negative ones and ids >= rows reach no sum
  cols.append(Column('outside', 8, 1000, rng.randint(-1000, 3000, size=6000), seed=3))
  cols.append(Column('empty', 8, 10, np.zeros(0, np.int64), seed=4))
  # sparse over a large table: hashed buckets by the shipped policy (wide rows, rows > 8 x ids; with an
  # optimizer step the wide sorted walk), and row-range buckets with few repeated rows (narrow rows)
  cols.append(Column('sparse100k', 64, 100000, rng.randint(0, 100000, size=4000), seed=5))
  # (3000 ids: 7 buckets of < 16384 rows each, and rows > 32 x ids keeps the row-sorted jobs away)
  cols.append(Column('sparse100k_narrow', 8, 100000, rng.randint(0, 100000, size=3000), seed=6))
  return cols


def _ragged_columns():
  rng = np.random.RandomState(2025)
  cols = []
  # tables of a few rows: every lane group's run head crosses shares
  for rows in (2, 100):
    sp, ids = _ragged_ids(rng, 5700, 'sqrtn', 16, lambda n, r=rows: rng.randint(0, r, size=n))
    cols.append(Column(f'small{rows}', 4, rows, ids, 'sqrtn', sp, seed=rows))
  # ragged mean at the length limit: the rows the seg-of launch (or the histogram launch) scales
  sp, ids = _ragged_ids(rng, 6000, 'mean', 32, lambda n: rng.randint(0, 50000, size=n))
  cols.append(Column('mean32', 16, 50000, ids, 'mean', sp, seed=6))
  for dim, comb in ((3, 'mean'), (20, 'sqrtn'), (16, 'sum'), (128, 'mean')):
    sp, ids = _ragged_ids(rng, 900, comb, 8, lambda n: rng.zipf(1.3, size=n) % 300)
    cols.append(Column(f'ragged{dim}{comb}', dim, 300, ids, comb, sp, seed=dim))
  sp, ids = _ragged_ids(rng, 1500, 'mean', 8, lambda n: rng.randint(-300, 900, size=n))
  cols.append(Column('ragged_outside', 8, 300, ids, 'mean', sp, seed=7))
  # a column of empty segments only
  cols.append(Column('empty_segments', 8, 10, np.zeros(0, np.int64), 'mean', np.zeros(51, np.int32), seed=8))
  # one row hot through ragged segments
  sp, ids = _ragged_ids(rng, 1300, 'mean', 8, lambda n: np.full(n, 1, np.int64))
  cols.append(Column('ragged_hot', 16, 3, ids, 'mean', sp, seed=9))
  return cols


def _weighted_columns():
  rng = np.random.RandomState(2026)
  cols = []
  for comb in ('sum', 'mean', 'sqrtn'):
    for dim, rows, n_seg, hot in ((16, 400, 1500, False), (128, 50, 600, False), (6, 3, 900, True)):
      sp = exact.exact_ragged(rng, n_seg, comb, 16 if comb != 'sum' else 6)
      n = int(sp[-1])
      ids = np.where(rng.rand(n) < (0.8 if hot else 0.0), 1, rng.zipf(1.3, size=n) % rows)
      w = exact.exact_weights(rng, sp, n, comb)
      cols.append(Column(f'w{comb}{dim}', dim, rows, ids, comb, sp, w, seed=dim))
    # one id per sample with weights (sum only: a mean over one id has factor 1)
  n = 2 * 2048 + 5
  cols.append(Column('wsum_hot', 16, 8, np.full(n, 2, np.int64), 'sum', None,
                     exact.exact_weights(rng, None, n, 'sum'), seed=10))
  return cols


# ---- one backward call over a suite ---------------------------------------------------------------------
def run(cols, optimizer=None, emit=True, deterministic=False, interleaved=False):
  """The columns through one GroupLookupGrad call.  Returns (result triples, tables, slot pairs, adam)."""
  opt = optimizer or 'sgd'
  state = [c.state0(opt) for c in cols]
  kw, adam = {}, None
  if interleaved:
    inter = [dev(np.concatenate([s[0], s[1]], axis=1)) for s in state]
    tables = [t[:, :c.dim] for t, c in zip(inter, cols)]
    slots = [(t[:, c.dim:], None) for t, c in zip(inter, cols)]
    lookup = GroupLookup([dev(s[0]) for s in state], None, [c.comb for c in cols])
    kw['interleaved'] = inter
  else:
    tables = [dev(s[0]) for s in state]
    slots = [(dev(s[1]), dev(s[2])) for s in state]
    lookup = GroupLookup(tables, None, [c.comb for c in cols])
    if opt == 'adagrad':
      kw['accums'] = [s[0] for s in slots]
    elif opt == 'adam':
      adam = LazyAdam(device=DEV)
      kw.update(moments=slots, adam=adam)
    elif opt == 'ftrl':
      kw.update(ftrl_slots=slots, ftrl=FTRL)
  grad = GroupLookupGrad(lookup, deterministic=deterministic, **kw)
  weights = [None if c.weights is None else dev(c.weights) for c in cols]
  res = grad([dev(c.ids) for c in cols], [dev(c.grads) for c in cols],
             [None if c.splits is None else dev(c.splits) for c in cols],
             apply_lr=LR if optimizer else 0.0, optimizer=opt, emit=emit,
             sp_weights=weights if any(w is not None for w in weights) else None)
  torch.cuda.synchronize()
  return res, tables, slots, adam


def check_emitted(cols, res, label, ascending=False):
  """n_unique = the distinct valid rows; the emitted rows are distinct and exactly that set; every emitted
  gradient row has the bits of the exact sum."""
  for c, (u, g, nu) in zip(cols, res):
    want = c.want
    k = int(nu.item())
    assert k == want.rows.size, f'{label} {c.name}: n_unique {k}, {want.rows.size} distinct valid rows'
    rows = host(u[:k])
    order = np.arange(k) if ascending else np.argsort(rows, kind='stable')
    np.testing.assert_array_equal(rows[order], want.rows, err_msg=f'{label} {c.name}: emitted rows')
    exact.assert_bits_equal(host(g[:k])[order], want.sums(), f'{label} {c.name}: gradient sums',
                            unit=want.unit[want.rows], rows=want.rows)


def check_stepped(cols, optimizer, tables, slots, label, n_unique=None):
  """Tables and slots after the step == the reference applied to the EXACT sums, in every row (rows
  outside the batch untouched: the reference leaves them)."""
  used = {'sgd': 0, 'adagrad': 1, 'adam': 2, 'ftrl': 2}[optimizer]
  for k, c in enumerate(cols):
    want = c.stepped(optimizer)
    unit = c.want.unit
    exact.assert_bits_equal(host(tables[k]), want[0], f'{label} {c.name}: table', unit=LR * unit)
    for s in range(used):
      exact.assert_bits_equal(host(slots[k][s]), want[1 + s], f'{label} {c.name}: slot {s}')
    if n_unique is not None:
      assert int(n_unique[k][2].item()) == c.want.rows.size, f'{label} {c.name}: n_unique'


def check_table_untouched(cols, tables, label):
  for c, t in zip(cols, tables):
    exact.assert_bits_equal(host(t), c.table, f'{label} {c.name}: table after a call without a step')


def emit_and_sgd(cols, label):
  """What every plan must satisfy: assertions 1 and 3 of the issue."""
  res, tables, _, _ = run(cols)
  check_emitted(cols, res, f'{label} emit')
  check_table_untouched(cols, tables, label)
  ends = []
  for emit in (True, False):
    res, tables, slots, _ = run(cols, 'sgd', emit=emit)
    if emit:
      check_emitted(cols, res, f'{label} sgd emit')
    check_stepped(cols, 'sgd', tables, slots, f'{label} sgd emit={emit}', n_unique=res)
    ends.append([host(t) for t in tables])
  for c, a, b in zip(cols, *ends):                         # step only == emit, in EVERY row
    exact.assert_bits_equal(b, a, f'{label} {c.name}: step only against emit')


# ---- the plans --------------------------------------------------------------------------------------------
# bwd_dense x bwd_onepass, with ONE pass over the hooks' grid beside them (every value of every hook once or more)
_HOOKS = [{}, {'bwd_buckets_log2': 0, 'bwd_split_pairs': 96, 'bwd_bucket_pairs': 200},
          {'bwd_buckets_log2': 2, 'bwd_split_pairs': 700, 'bwd_bucket_pairs': 448},
          {'bwd_split_pairs': 96, 'bwd_bucket_pairs': 448}, {'bwd_buckets_log2': 0},
          {'bwd_buckets_log2': 2, 'bwd_split_pairs': 96}, {'bwd_split_pairs': 700, 'bwd_bucket_pairs': 200},
          {'bwd_buckets_log2': 0, 'bwd_split_pairs': 700}]
PLANS = {}
for _k, (_dense, _onepass) in enumerate((d, o) for d in (1, 0, 2, 3) for o in (1, 0)):
  _opts = dict(bwd_dense=_dense, bwd_onepass=_onepass, **_HOOKS[_k])
  PLANS['-'.join(f'{k[4:]}{v}' for k, v in _opts.items())] = _opts
# one-at-a-time flips off the default (the histogram launch's scale and the staged scatter exist in the
# three-launch grouping only: flipped there too)
for _name, _values in (('bwd_pairs_packed', (0,)), ('bwd_seg_inline', (0,)), ('bwd_scatter_staged', (0,)),
                       ('bwd_scale_fused', (0,)), ('bwd_wide', (0, 2)), ('bwd_simple', (0,)),
                       ('bwd_xcd', (0, 2, 4)), ('bwd_rowsort_ratio', (0, 64)), ('bwd_lds_pad', (14,)),
                       ('bwd_streams', (0,))):
  for _v in _values:
    PLANS[f'{_name[4:]}{_v}'] = {_name: _v}
for _name in ('bwd_scatter_staged', 'bwd_scale_fused', 'bwd_seg_inline'):
  PLANS[f'onepass0-{_name[4:]}0'] = {'bwd_onepass': 0, _name: 0}


@pytest.mark.parametrize('which', ['plain', 'ragged'])
@pytest.mark.parametrize('plan', sorted(PLANS))
def test_plans_emit_and_sgd_bit_equal_to_the_exact_sums(hbk_option, plan, which):
  for name, value in PLANS[plan].items():
    hbk_option(name, value)
  emit_and_sgd(suite(which), plan)


@pytest.mark.parametrize('which', ['plain', 'ragged', 'weighted'])
@pytest.mark.parametrize('det', [1, 2])
def test_deterministic_plans_give_the_bits_of_the_default_plan(hbk_option, det, which):
  """Exact sums have one value whatever the order: the in-order plans (rows ascending) and the default
  plan (checked against the same reference above) agree bit for bit."""
  cols = suite(which)
  hbk_option('bwd_deterministic', det)
  res, tables, _, _ = run(cols)
  check_emitted(cols, res, f'deterministic={det}', ascending=True)
  check_table_untouched(cols, tables, f'deterministic={det}')
  hbk_option('bwd_deterministic', 0)
  res, _, _, _ = run(cols, deterministic=True)            # the per-object flag
  check_emitted(cols, res, 'GroupLookupGrad(deterministic=True)', ascending=True)
  res, _, _, _ = run(cols)
  check_emitted(cols, res, 'default plan')


_STEP_HOOKS = {'default': {}, 'one_bucket': {'bwd_buckets_log2': 0},
               'split': {'bwd_split_pairs': 96, 'bwd_buckets_log2': 2}, 'hashed': {'bwd_dense': 0},
               'rowsorted': {'bwd_dense': 3}}


@pytest.mark.parametrize('which', ['plain', 'ragged'])
@pytest.mark.parametrize('hook', sorted(_STEP_HOOKS))
@pytest.mark.parametrize('optimizer', ['adagrad', 'adam', 'ftrl'])
def test_optimizer_steps_emit_and_step_only(hbk_option, optimizer, hook, which):
  """Adagrad, Lazy Adam and FTRL, emitting and step only (where rows span chunks or buckets are split the
  step-only form steps from scratch rows in the workspace): tables and slots bit-equal to the reference
  applied to the exact sums."""
  for name, value in _STEP_HOOKS[hook].items():
    hbk_option(name, value)
  cols = suite(which)
  for emit in (True, False):
    label = f'{optimizer} {hook} emit={emit}'
    res, tables, slots, adam = run(cols, optimizer, emit=emit)
    if emit:
      check_emitted(cols, res, label)
    check_stepped(cols, optimizer, tables, slots, label, n_unique=res)
    if adam is not None:
      np.testing.assert_array_equal(host(adam.beta_powers), np.array([F32(B1 * B1), F32(B2 * B2)], F32))


@pytest.mark.parametrize('emit', [True, False])
@pytest.mark.parametrize('optimizer', ['sgd', 'adagrad'])
def test_interleaved_weights_and_accumulator(optimizer, emit):
  """table_pitch = 2 dim: the step works on [w | accumulator] rows."""
  for which in ('plain', 'ragged'):
    cols = suite(which)
    res, tables, slots, _ = run(cols, optimizer, emit=emit, interleaved=True)
    if emit:
      check_emitted(cols, res, f'interleaved {optimizer}')
    for k, c in enumerate(cols):
      want = c.stepped(optimizer)
      exact.assert_bits_equal(host(tables[k]), want[0], f'interleaved {optimizer} emit={emit} {c.name}: weights')
      # (SGD leaves the accumulator half as it was)
      exact.assert_bits_equal(host(slots[k][0]), want[1], f'interleaved {optimizer} emit={emit} {c.name}: accumulator')


_WEIGHTED_PLANS = {'default': {}, 'dense0': {'bwd_dense': 0}, 'dense2': {'bwd_dense': 2},
                   'dense0-onepass0-split96': {'bwd_dense': 0, 'bwd_onepass': 0, 'bwd_split_pairs': 96},
                   'dense3-onepass0': {'bwd_dense': 3, 'bwd_onepass': 0},
                   'one_bucket-split96': {'bwd_buckets_log2': 0, 'bwd_split_pairs': 96}}


@pytest.mark.parametrize('plan', sorted(_WEIGHTED_PLANS))
def test_weighted_columns(hbk_option, plan):
  """sp_weights from exact_weights (sum: any of -2 ... 2 per id; mean / sqrtn: one positive power of two
  per segment): emitted sums and SGD steps as for the unweighted columns.  A zero gradient under a
  negative weight is a term of -0.0: a row that receives nothing else must still leave as +0.0, what the
  scatter-add into zeros gives (the hashed plans once stored such a row's one pair as it arrived)."""
  for name, value in _WEIGHTED_PLANS[plan].items():
    hbk_option(name, value)
  emit_and_sgd(suite('weighted'), f'weighted {plan}')


# ---- sequence columns: the pad row ------------------------------------------------------------------------
_SEQ = {}


def _sequence_case(B, pad):
  """B samples of T = 16 positions, about a quarter of them padding; ids past T in the longest samples."""
  key = (B, pad)
  if key in _SEQ:
    return _SEQ[key]
  rng = np.random.RandomState(B + (pad or 0))
  rows, dim, T = 211, 16, 16
  lens = rng.choice([2, 6, 8, 12, 14, 16, 16, 19, 24], size=B)       # mean min(len, T) / T = 0.74
  splits = exact.splits_of(lens)
  ids = rng.randint(0, 200, size=int(splits[-1])).astype(np.int64)   # (the pad id, 205, is no real id)
  for b in np.nonzero(lens > T)[0]:
    ids[splits[b] + T:splits[b + 1]] = 209                           # row 209: at truncated positions only
  grid, ln = sequence_ref.grid_ref(ids, splits, rows, T, pad)
  r = sequence_ref.rows_ref(grid, rows)
  keep = r >= 0
  bits = exact.exact_terms_budget(r[keep], 0, case=f'sequence B={B} pad={pad}')
  grads = exact.exact_grads(rng, (B, T, dim), min(bits, 12))
  col = Column.__new__(Column)
  col.name, col.dim, col.rows, col.comb = f'seq{B}pad{pad}', dim, rows, 'sum'
  col.table = exact.exact_tables(rng, rows, dim)
  col.want = exact.exact_dense((rows, dim), r[keep], grads.reshape(-1, dim).astype(np.float64)[keep], case=col.name)
  col._steps = {}
  n_padding = int((T - ln).sum())
  _SEQ[key] = (col, ids, splits, grads, T, n_padding)
  return _SEQ[key]


@pytest.mark.parametrize('B', [512, 2048])
@pytest.mark.parametrize('pad', [205, None])
def test_sequence_backward_pad_row(B, pad):
  """With a pad id its row collects every padding position's gradient (~2 000 terms at B = 512: about
  one chunk; ~8 000 at B = 2048: several); without one, padding reaches no row; ids past T reach nothing."""
  col, ids, splits, grads, T, n_padding = _sequence_case(B, pad)
  assert 0.2 < n_padding / (B * T) < 0.3
  assert 209 not in col.want.rows.tolist()
  if pad is None:
    assert int(col.want.counts.sum()) == B * T - n_padding
  else:
    assert col.want.counts[pad] == n_padding and col.want.rows.tolist().count(pad) == 1
    assert n_padding > (1800 if B == 512 else 3 * 2048)

  def backward(optimizer=None, deterministic=False, emit=True):
    w, a, _ = col.state0(optimizer or 'sgd')
    t, acc = dev(w), dev(a)
    lookup = SequenceLookup([t], [col.rows], max_lens=T, pad_ids=pad)
    lookup([dev(ids)], [dev(splits)])
    res = SequenceLookupGrad(lookup, accums=[acc])([dev(grads)], apply_lr=LR if optimizer else 0.0,
                                                  optimizer=optimizer or 'sgd', emit=emit,
                                                  deterministic=deterministic)
    torch.cuda.synchronize()
    return res, [t], [(acc, None)]

  res, t, _ = backward()
  check_emitted([col], res, 'sequence emit')
  check_table_untouched([col], t, 'sequence')
  res, _, _ = backward(deterministic=True)
  check_emitted([col], res, 'sequence deterministic', ascending=True)
  for optimizer in ('sgd', 'adagrad'):
    for emit in (True, False):
      res, t, slots = backward(optimizer, emit=emit)
      if emit:
        check_emitted([col], res, f'sequence {optimizer}')
      check_stepped([col], optimizer, t, slots, f'sequence {optimizer} emit={emit}', n_unique=res)


# ---- the sharded owner reduce, in-process worlds ----------------------------------------------------------
def _world(world, fn):
  """fn(rank, communicator) on `world` host threads over Collective.local_world; the results by rank."""
  comms = hb.distribute.Collective.local_world(world)
  results, errors = [None] * world, []

  def body(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        results[r] = fn(r, comms[r])
        torch.cuda.current_stream().synchronize()
    except Exception as e:  # pylint: disable=broad-except
      errors.append((r, repr(e)))

  threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=60)
  for cm in comms:
    cm.close()
  assert not errors, errors
  assert all(x is not None for x in results)
  return results


_SHARDED = {}


def _sharded_case(world, wire16):
  """4 columns, 256 samples per rank, sum and mean; the reference: ONE unsharded column over all ranks'
  batches.  Ids of few values in the first two columns (what dedup is for, and hot rows on the owner)."""
  key = (world, wire16)
  if key in _SHARDED:
    return _SHARDED[key]
  rng = np.random.RandomState(40 + world)
  dims, rows, combs = [16, 8, 128, 6], [40, 1000, 64, 5003], ['sum', 'mean', 'mean', 'sum']
  batch = 256
  ids, splits = [], []
  for r in range(world):
    ri, rs = [], []
    for c in range(4):
      sp = exact.exact_ragged(rng, batch, 'mean', 8) if combs[c] == 'mean' else None
      n = batch if sp is None else int(sp[-1])
      rs.append(sp)
      ri.append((rng.zipf(1.3, size=n) % rows[c]).astype(np.int64))
    ids.append(ri)
    splits.append(rs)
  cols = []
  for c in range(4):
    # the whole world's batch as one column: ranks one after the other
    all_ids = np.concatenate([ids[r][c] for r in range(world)])
    all_sp = None
    if combs[c] == 'mean':
      all_sp = exact.splits_of(np.concatenate([np.diff(splits[r][c]) for r in range(world)]))
    cols.append(Column(f'sharded{c}w{world}', dims[c], rows[c], all_ids, combs[c], all_sp, seed=c, fp16=wire16))
  _SHARDED[key] = (cols, ids, splits, batch)
  return _SHARDED[key]


@pytest.mark.parametrize('world,dedup,wire16', [(2, False, False), (2, True, False), (3, False, False),
                                                (3, True, False), (2, False, True)])
def test_sharded_owner_reduce_in_process_world(world, dedup, wire16):
  """The owner's emitted slices and stepped shards (SGD, Adagrad; emit and step only) bit-equal to the
  unsharded exact reference over all ranks' batches.  With requester-side dedup the partial sums that
  travel are exact too; on the fp16 wire every term is checked (on the reference) to survive fp16."""
  cols, ids, splits, batch = _sharded_case(world, wire16)
  n = len(cols)

  def step(optimizer, emit):
    def fn(r, comm):
      state = [c.state0(optimizer or 'sgd') for c in cols]
      shards = [dev(s[0][r::world].copy()) for s in state]
      accums = [dev(s[1][r::world].copy()) for s in state]
      drv = ShardedGroupLookup(shards, comm, buckets=[c.rows for c in cols], combiners=[c.comb for c in cols],
                               wire_dtype=torch.float16 if wire16 else None, dedup=dedup, accums=accums)
      drv([dev(i) for i in ids[r]], [None if s is None else dev(s) for s in splits[r]])
      grads = [dev(c.grads[r * batch:(r + 1) * batch]) for c in cols]
      res = drv.backward(grads, apply_lr=LR if optimizer else 0.0, optimizer=optimizer or 'sgd', emit=emit)
      torch.cuda.current_stream().synchronize()
      out = ([int(x[2].item()) for x in res],
             [None if x[0] is None else host(x[0][:int(x[2].item())]) for x in res],
             [None if x[1] is None else host(x[1][:int(x[2].item())]) for x in res],
             [host(t) for t in shards], [host(a) for a in accums])
      drv.close()
      return out
    return _world(world, fn)

  for optimizer, emit in ((None, True), ('sgd', True), ('sgd', False), ('adagrad', True), ('adagrad', False)):
    label = f'W={world} dedup={dedup} wire16={wire16} {optimizer} emit={emit}'
    results = step(optimizer, emit)
    for k, c in enumerate(cols):
      want = c.stepped(optimizer) if optimizer else (c.table, np.full_like(c.table, ACCUM0))
      for r in range(world):
        nu, urows, grows, shards, accums = (x[k] for x in results[r])
        mine = c.want.rows[c.want.rows % world == r]
        assert nu == mine.size, f'{label} {c.name} rank {r}: n_unique'
        if emit:
          order = np.argsort(urows, kind='stable')
          np.testing.assert_array_equal(urows[order] * world + r, mine, err_msg=f'{label} {c.name} rank {r}: rows')
          exact.assert_bits_equal(grows[order], c.want.dense[mine], f'{label} {c.name} rank {r}: gradient sums',
                                  unit=c.want.unit[mine], rows=mine)
        exact.assert_bits_equal(shards, want[0][r::world], f'{label} {c.name} rank {r}: shard')
        if optimizer == 'adagrad':
          exact.assert_bits_equal(accums, want[1][r::world], f'{label} {c.name} rank {r}: accumulator')
  assert n == 4
