"""Randomised parity of the features layered on the backward -- per-id weights, max_norm, Lazy Adam, FTRL
and the shared two-slot apply -- drawn together and under random plans, against the one float64 /
fp32 restatement of tests/support/reference.py:

1. grouped lookup + backward, two or three chained steps per draw: the forward within the float64
   bound (bit-equal to the oracle for plain columns), the emitted rows within the bound of g' (bit-equal
   to the in-order fp32 sums in the deterministic modes), every step bit-equal to its rule applied to the
   call's own slices (the powf FTRL form within its ulp bound), rows outside the batch untouched, Adam's
   powers advanced once per finished call, step-only calls equal to emitting ones;
2. more than 64 columns through the two-slot and clip launches (the per-64-column split);
3. every clipped / weighted forward kind of a segmented fp32 table through the C ABI;
4. a captured graph of a deterministic (sort path) Lazy Adam step with weights and clip;
5. refusals that leave every table, slot and power bit-identical;
6. the sharded backward with weights, clip and every optimizer in an in-process world.

The committed runs are deterministic; HBK_FUZZ_RANDOM=1 HBK_FUZZ_SCALE=10 hunts with fresh draws."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.support import reference as ref  # noqa: E402
from tests.support.tolerance import (FLOOR, REL, WIRE16_FLOOR, WIRE16_REL,  # noqa: E402
                                     assert_sums_close)

hypothesis = pytest.importorskip('hypothesis')
from hypothesis import example, given  # noqa: E402
from hypothesis import strategies as st  # noqa: E402

from tests.test_gpu_fuzz import _cfg, _ids, plan_options  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = np.float32, np.float64


def dev(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
  return t.detach().cpu().numpy().copy()


# ---- draws --------------------------------------------------------------------------------------------
feature_column = st.fixed_dictionaries({
  'dim': st.sampled_from([1, 3, 4, 6, 8, 16, 20, 32, 64, 128, 256]),
  'rows': st.sampled_from([1, 2, 7, 64, 1000, 20011]),
  'n_seg': st.one_of(st.just(0), st.integers(1, 600)),
  'ragged': st.booleans(),
  'max_len': st.integers(0, 9),
  'combiner': st.sampled_from(['sum', 'mean', 'sqrtn']),
  'skew': st.sampled_from(['uniform', 'zipf', 'one', 'negative']),
  'bucket0': st.booleans(),                    # ids as rows: negative and out-of-range ids are dropped
  'weights': st.sampled_from(['none', 'uniform', 'signed', 'zero_segment']),
  'clip': st.sampled_from(['none', 'half', 'big', 'ties']),
})
big_feature_column = st.fixed_dictionaries({
  'dim': st.sampled_from([4, 16, 32, 64]),
  'rows': st.sampled_from([200, 5000, 100000]),
  'n_seg': st.sampled_from([3000, 9000, 20000]),
  'ragged': st.booleans(),
  'max_len': st.integers(1, 4),
  'combiner': st.sampled_from(['sum', 'mean', 'sqrtn']),
  'skew': st.sampled_from(['uniform', 'zipf', 'negative']),
  'bucket0': st.just(False),
  'weights': st.sampled_from(['none', 'uniform', 'signed']),
  'clip': st.sampled_from(['none', 'half', 'ties']),
})
optimizer_draw = st.fixed_dictionaries({
  'name': st.sampled_from(['emit', 'sgd', 'adagrad', 'adam', 'ftrl']),
  'interleaved': st.booleans(),                # Adagrad: weights and accumulator side by side per row
  'emit': st.booleans(),
  'finish': st.booleans(),                     # Adam: advance the beta powers
  'lr_power': st.sampled_from([-0.5, 0.0, -0.3]),
  'l1': st.sampled_from([0.0, 0.05, 2.0]),
  'l2': st.sampled_from([0.0, 1e-5, 0.1]),
  'l2_shrinkage': st.sampled_from([0.0, 0.01]),
})
feature_plan = st.fixed_dictionaries({
  'bwd_deterministic': st.sampled_from([0, 1, 2]),
  'bwd_buckets_log2': st.sampled_from([-1, 0, 3]),
  'bwd_pairs_packed': st.sampled_from([0, 1]),
  'bwd_seg_inline': st.sampled_from([0, 1]),
  'bwd_scatter_staged': st.sampled_from([0, 1]),
  'bwd_scale_fused': st.sampled_from([0, 1]),
  'bwd_split_pairs': st.sampled_from([0, 64]),
})

ADAM_P0 = (F32(0.9), F32(0.999))   # LazyAdam's powers before its first step
CLIP_C = 0.5     # a power of two: the tie rows [c, 0, ..] and [0, .., -c] are exact


def _table(rng, c):
  rows, dim = c['rows'], c['dim']
  t = rng.uniform(-1, 1, size=(rows, dim))
  if c['clip'] in ('half', 'ties'):
    # norms between 0.2 c and 3 c: about half the rows outside the ball
    t /= np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-30)
    t *= rng.uniform(0.2 * CLIP_C, 3 * CLIP_C, size=(rows, 1))
  if c['clip'] == 'ties':
    t[0] = 0                                   # n = 0
    if rows > 1:
      t[1] = 0
      t[1, 0] = CLIP_C                         # n == c exactly
    if rows > 2:
      t[2] = 0
      t[2, dim - 1] = -CLIP_C
  return t.astype(F32)


def _max_norm(c, table):
  if c['clip'] in ('half', 'ties'):
    return CLIP_C
  if c['clip'] == 'big':   # a power of two above every row norm
    n = float(np.sqrt((table.astype(F64) ** 2).sum(1)).max()) if table.size else 1.0
    return float(2.0 ** np.ceil(np.log2(max(n, 1e-3)) + 1))
  return 0.0


def _batch(rng, c, id_dtype):
  """ids, row splits, bucket, weights of one step of column c."""
  rows = c['rows']
  if c['ragged']:
    lens = rng.randint(0, c['max_len'] + 1, size=c['n_seg'])
    sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n = int(sp[-1])
  else:
    sp, n = None, c['n_seg']
  if c['bucket0']:
    bucket = 0
    ids = rng.randint(-max(rows // 4, 2), rows + max(rows // 4, 2), size=n)
  else:
    bucket = rows
    ids = _ids(rng, n, rows, c['skew'])
  ids = np.asarray(ids, np.int64)
  if c['clip'] == 'ties' and n >= 3:
    ids[:3] = [0, 1 % rows, 2 % rows]          # the n = 0 and n == c rows take part
  if id_dtype == np.int32:   # (wrapped into int32's range, negatives kept)
    ids = ((ids + 2**31) % 2**32 - 2**31).astype(np.int32)
  w = None
  if c['weights'] == 'uniform':
    w = rng.uniform(0.1, 2, size=n).astype(F32)
  elif c['weights'] == 'signed':
    w = rng.uniform(-1, 2, size=n).astype(F32)
    w[rng.rand(n) < 0.2] = 0
  elif c['weights'] == 'zero_segment':
    w = rng.uniform(0.1, 2, size=n).astype(F32)
    spp = sp if sp is not None else np.arange(n + 1)
    nz = np.nonzero(np.diff(spp) > 0)[0]
    for s in nz[:2]:                           # whole segments of zero weight: zero rows
      w[spp[s]:spp[s + 1]] = 0
  return ids, sp, bucket, w


def _n_seg(ids, sp):
  return ids.size if sp is None else sp.size - 1


# ---- the grouped check ----------------------------------------------------------------------------------
class _State:
  """Tables and optimizer slots of one draw, on the device, and the objects that step them."""

  def __init__(self, tables, opt, cols, maxn):
    from hybridbackend_amd.embedding import Ftrl, GroupLookup, GroupLookupGrad, LazyAdam
    self.opt = opt
    self.name = opt['name']
    self.inter = self.name == 'adagrad' and opt['interleaved']
    self.tables = [dev(t) for t in tables]
    self.slots = None
    kw = {}
    if self.name == 'adagrad':
      acc = [np.full(t.shape, 0.1, F32) for t in tables]
      if self.inter:
        self.buf = [dev(np.concatenate([t, a], axis=1)) for t, a in zip(tables, acc)]
        kw['interleaved'] = self.buf
      else:
        self.slots = [(dev(a),) for a in acc]
        kw['accums'] = [s[0] for s in self.slots]
    elif self.name == 'adam':
      self.adam = LazyAdam(device=DEV)
      self.slots = [(dev(np.random.RandomState(7).uniform(-0.1, 0.1, size=t.shape).astype(F32)),
                     dev(np.full(t.shape, 0.01, F32))) for t in tables]
      kw.update(moments=self.slots, adam=self.adam)
    elif self.name == 'ftrl':
      self.ftrl = Ftrl(l1=opt['l1'], l2=opt['l2'], l2_shrinkage=opt['l2_shrinkage'],
                       lr_power=opt['lr_power'])
      self.slots = [(dev(np.full(t.shape, 0.1, F32)), dev(np.random.RandomState(8).uniform(
        -1, 1, size=t.shape).astype(F32))) for t in tables]
      kw.update(ftrl_slots=self.slots, ftrl=self.ftrl)
    self.lookup = GroupLookup(self.tables, [c['bucket'] for c in cols], [c['combiner'] for c in cols],
                              max_norms=[m or None for m in maxn])
    self.grad = GroupLookupGrad(self.lookup, **kw)

  def weights(self):
    """The weights as the step sees them."""
    if self.inter:
      return [b[:, :b.shape[1] // 2] for b in self.buf]
    return self.tables

  def snapshot(self):
    """fp32 host copies: per column [w, slot0, slot1] (absent slots None), and the powers."""
    out = []
    for c, w in enumerate(self.weights()):
      s = []
      if self.inter:
        s = [self.buf[c][:, self.buf[c].shape[1] // 2:]]
      elif self.slots is not None:
        s = list(self.slots[c])
      out.append([host(w)] + [host(x) for x in s] + [None] * (2 - len(s)))
    pw = host(self.adam.beta_powers) if self.name == 'adam' else None
    return out, pw

  def sync_forward_tables(self):
    if self.inter:   # the forward reads lookup.tables: a trainer with interleaved storage copies back
      for t, b in zip(self.tables, self.buf):
        t.copy_(b[:, :t.shape[1]])

  def call(self, d_ids, d_g, d_sp, d_w, lr, emit, finish=True):
    name = self.name
    if name == 'emit':
      return self.grad(d_ids, d_g, d_sp, sp_weights=d_w)
    return self.grad(d_ids, d_g, d_sp, apply_lr=lr, optimizer=name, emit=emit, sp_weights=d_w,
                     finish=finish)


def _apply_rule(st_, snap_c, rows, g, lr, powers):
  """The fp32 rule on host copies of one column: returns (w, s0, s1)."""
  w, s0, s1 = (None if x is None else x.copy() for x in snap_c)
  name = st_.name
  if name == 'sgd':
    ref.sgd_step(w, rows, g, lr)
  elif name == 'adagrad':
    ref.adagrad_step(w, s0, rows, g, lr)
  elif name == 'adam':
    ref.adam_step(w, s0, s1, rows, g, lr, powers)
  elif name == 'ftrl':
    f = st_.ftrl
    ref.ftrl_step(w, s0, s1, rows, g, lr, f.l1, f.l2, f.l2_shrinkage, f.lr_power)
  return w, s0, s1


def _check_stepped(st_, k, before, after, rows, g, lr, powers, err):
  """after == the rule on `before` with the slices (rows, g) bit for bit (powf FTRL: its ulp bound);
  rows outside the slices bit-unchanged."""
  want = _apply_rule(st_, before, rows, g, lr, powers)
  powf = st_.name == 'ftrl' and not ref.ftrl_exact(st_.ftrl.lr_power)
  for j, (got_x, want_x) in enumerate(zip(after, want)):
    if got_x is None:
      continue
    if powf and j in (0, 2):
      outside = np.ones(got_x.shape[0], bool)
      outside[rows] = False
      np.testing.assert_array_equal(got_x[outside], before[j][outside], err_msg=f'{err} slot {j}')
      continue
    np.testing.assert_array_equal(got_x, want_x, err_msg=f'{err}: {st_.name} state {j}')
  if powf:
    f = st_.ftrl
    ref.assert_ftrl_powf_close(after[0][rows], after[2][rows], before[0], before[1], before[2], rows, g, lr,
                               f.l1, f.l2, f.l2_shrinkage, f.lr_power, err_msg=err)


def _run_features(cols, opt, plan, steps, id32, seed):
  import oracle
  from hybridbackend_amd import _lib
  rng = np.random.RandomState(seed)
  cols = [dict(c) for c in cols]
  for c in cols:
    if c['dim'] % 4 != 0 and c['dim'] > 64:
      c['dim'] = 64
    c['bucket'] = 0 if c['bucket0'] else c['rows']
  tables = [_table(rng, c) for c in cols]
  maxn = [_max_norm(c, t) for c, t in zip(cols, tables)]
  name = opt['name']
  emit = opt['emit'] or name == 'emit'
  det = plan.get('bwd_deterministic', 0)
  if not emit and det == 0 and name != 'sgd':
    emit = True          # (step-only against an emitting call: bit-equal in modes 1, 2; SGD's bound in 0)
  lr = 0.05
  id_dtype = np.int32 if id32 else np.int64
  main = _State(tables, opt, cols, maxn)
  twin = _State(tables, opt, cols, maxn) if not emit else None   # the emitting call of a step-only one
  old = {k: _lib.set_option(k, v) for k, v in plan.items()}
  try:
    for step in range(steps):
      batch = [_batch(rng, c, id_dtype) for c in cols]
      grads = [rng.randn(_n_seg(b[0], b[1]), c['dim']).astype(F32) for b, c in zip(batch, cols)]
      d_ids = [dev(b[0]) for b in batch]
      d_sp = [None if b[1] is None else dev(b[1]) for b in batch]
      d_w = [None if b[3] is None else dev(b[3]) for b in batch]
      d_g = [dev(g) for g in grads]
      before, p0 = main.snapshot()
      w_fwd = [host(t) for t in main.tables]
      finish = opt['finish'] or name != 'adam'
      # forward
      outs = main.lookup(d_ids, d_sp, sp_weights=d_w)
      for k, c in enumerate(cols):
        ids, sp, bucket, w = batch[k]
        got = host(outs[k])
        if w is None and not maxn[k] and bucket:
          want = oracle.group_lookup_fwd([w_fwd[k]], [np.asarray(ids, np.int64)], [sp], [bucket],
                                         [c['combiner']])[0]
          np.testing.assert_array_equal(got, want, err_msg=f'step {step} forward column {k}')
        else:
          want, mag = ref.forward64(w_fwd[k], ids, sp, w, c['combiner'], maxn[k], bucket)
          assert_sums_close(got, want, mag, err_msg=f'step {step} forward column {k}')
      # backward (+ step); a step-only call is compared with an emitting call on a twin of the state
      if twin is not None:
        t_before, t_p0 = twin.snapshot()
        for a, b in zip(t_before, before):
          for x, y in zip(a, b):
            if x is not None:
              np.testing.assert_array_equal(x, y)
        res = twin.call(d_ids, d_g, d_sp, d_w, lr, True, finish)
        run, run_before, run_p0 = twin, t_before, t_p0
      else:
        res = main.call(d_ids, d_g, d_sp, d_w, lr, True, finish)
        run, run_before, run_p0 = main, before, p0
      torch.cuda.synchronize()
      after, p1 = run.snapshot()
      for k, c in enumerate(cols):
        ids, sp, bucket, w = batch[k]
        err = f'step {step} column {k} ({name}, clip {maxn[k]}, weights {c["weights"]}, det {det})'
        u, gp = host(res[k][0]), host(res[k][1])
        n = int(res[k][2].item())
        u, gp = u[:n], gp[:n]
        want_u, want_g, want_m = ref.backward64(run_before[k][0], ids, sp, w, c['combiner'], grads[k],
                                                maxn[k], bucket)
        assert np.unique(u).size == n, f'{err}: a row emitted twice'
        np.testing.assert_array_equal(np.sort(u), want_u, err_msg=err)
        order = np.argsort(u)
        assert_sums_close(gp[order], want_g, want_m, err_msg=err)
        if det:
          np.testing.assert_array_equal(u, want_u, err_msg=f'{err}: rows not ascending')
          if not maxn[k]:
            t32, r32, v32 = ref.terms32(c['rows'], ids, sp, w, c['combiner'], grads[k], bucket)
            _, seq = ref.seq_row_sums(t32, r32, v32)
            np.testing.assert_array_equal(gp, seq, err_msg=f'{err}: not the in-order fp32 sum')
        if name == 'emit':
          for x, y in zip(after[k], run_before[k]):
            if x is not None:
              np.testing.assert_array_equal(x, y, err_msg=f'{err}: emit changed the state')
        else:
          _check_stepped(run, k, run_before[k], after[k], u, gp, lr, run_p0, err)
      if name == 'adam':
        want_p = ref.adam_finish(run_p0) if finish else tuple(run_p0)
        np.testing.assert_array_equal(p1, np.array(want_p, F32), err_msg=f'step {step}: beta powers')
      if twin is not None:
        main.call(d_ids, d_g, d_sp, d_w, lr, False, finish)
        torch.cuda.synchronize()
        got_after, got_p = main.snapshot()
        for k in range(len(cols)):
          for j, (x, y) in enumerate(zip(got_after[k], after[k])):
            if x is None:
              continue
            if det:
              np.testing.assert_array_equal(x, y, err_msg=f'step {step} column {k}: step only != emit')
            else:   # SGD in mode 0: both within the bound of the float64 step from the same state
              ids, sp, bucket, w = batch[k]
              uu, g64, m64 = ref.backward64(before[k][0], ids, sp, w, cols[k]['combiner'], grads[k],
                                            maxn[k], bucket)
              want = before[k][0].astype(F64)
              mag = np.abs(want)
              want[uu] -= lr * g64
              mag[uu] += lr * m64
              assert_sums_close(x, want, mag, err_msg=f'step {step} column {k}: step only')
              untouched = np.setdiff1d(np.arange(x.shape[0]), uu)
              np.testing.assert_array_equal(x[untouched], before[k][0][untouched])
        if name == 'adam':
          np.testing.assert_array_equal(got_p, p1)
        if not det:   # (mode 0: the two states may differ in their last bits; go on from one of them)
          for k in range(len(cols)):
            twin.weights()[k].copy_(main.weights()[k])
            if twin.slots is not None:
              for a, b in zip(twin.slots[k], main.slots[k]):
                a.copy_(b)
      main.sync_forward_tables()
      if twin is not None:
        twin.sync_forward_tables()
  finally:
    for k, v in old.items():
      _lib.set_option(k, v)


@_cfg(200)
@given(cols=st.lists(feature_column, min_size=1, max_size=5), opt=optimizer_draw, plan=feature_plan,
       steps=st.integers(2, 3), id32=st.booleans(), seed=st.integers(0, 2**31 - 1))
@example(cols=[dict(dim=16, rows=64, n_seg=300, ragged=True, max_len=6, combiner='mean', skew='uniform',
                    bucket0=False, weights='signed', clip='ties')],
         opt=dict(name='adam', interleaved=False, emit=False, finish=True, lr_power=-0.5, l1=0.0, l2=0.0,
                  l2_shrinkage=0.0),
         plan=dict(bwd_deterministic=1, bwd_buckets_log2=-1, bwd_pairs_packed=1, bwd_seg_inline=1,
                   bwd_scatter_staged=1, bwd_scale_fused=1, bwd_split_pairs=0),
         steps=3, id32=False, seed=1)
def test_features_random(cols, opt, plan, steps, id32, seed):
  """Weights, clip and every optimizer drawn together with the deterministic modes and the grouping
  switches, over chained steps."""
  _run_features(cols, opt, plan, steps, id32, seed)


@_cfg(60)
@given(cols=st.lists(st.one_of(big_feature_column, feature_column), min_size=1, max_size=4),
       opt=optimizer_draw, plan=plan_options, det=st.sampled_from([0, 1, 2]),
       fwd=st.fixed_dictionaries({'fwd_hot_rows': st.sampled_from([0, 1]), 'fwd_d16': st.sampled_from([0, 1]),
                                  'fwd_xcd': st.sampled_from([0, 2]), 'fwd_interleave': st.sampled_from([0, 3])}),
       id32=st.booleans(), seed=st.integers(0, 2**31 - 1))
def test_features_random_plans(cols, opt, plan, det, fwd, id32, seed):
  """The same over large columns with the plan switches of test_gpu_fuzz.py drawn too."""
  p = dict(plan)
  p.update(fwd)
  p['bwd_deterministic'] = det
  _run_features(cols, opt, p, 2, id32, seed)


# ---- more than 64 columns -------------------------------------------------------------------------------
@pytest.mark.parametrize('n_cols', [65, 128, 130])
@pytest.mark.parametrize('optimizer', ['emit', 'sgd', 'adagrad', 'adam', 'ftrl'])
def test_many_columns(n_cols, optimizer):
  """The clip / two-slot launches split a call into launches of 64 columns and deal rows out per
  column; clipped, unclipped and empty columns mixed, dims 1 .. 256 within one launch."""
  rng = np.random.RandomState(n_cols * 7 + len(optimizer))
  dims = [1, 3, 4, 16, 20, 64, 128, 256, 8, 2]
  cols = []
  for k in range(n_cols):
    cols.append(dict(dim=dims[k % len(dims)], rows=int(rng.choice([7, 300, 2000])),
                     n_seg=0 if k % 9 == 4 else int(rng.randint(1, 120)), ragged=bool(k % 2),
                     max_len=4, combiner=('sum', 'mean', 'sqrtn')[k % 3], skew='uniform',
                     bucket0=k % 5 == 0, weights=('none', 'uniform', 'signed')[k % 3],
                     clip=('half', 'none', 'ties', 'big')[k % 4]))
  opt = dict(name=optimizer, interleaved=False, emit=True, finish=True, lr_power=-0.5, l1=0.05,
             l2=1e-5, l2_shrinkage=0.01)
  _run_features(cols, opt, {'bwd_deterministic': 1}, 2, False, n_cols)
  _run_features(cols[:n_cols // 2 + 1], opt, {'bwd_deterministic': 0}, 1, True, n_cols + 1)


# ---- every forward kind of a segmented table through the C ABI ----------------------------------------------
@pytest.mark.parametrize('dim', [3, 16, 64, 5])
@pytest.mark.parametrize('ragged', [False, True])
def test_segmented_table_forward_kinds(dim, ragged):
  """fp32 segmented tables (n_runs > 0, runs out of order in their buffer) plain, weighted, clipped and
  weighted + clipped (the clip kinds 64+4..7 and 64+36..39 of lookup_fwd.hip), vec4 and scalar dims."""
  from hybridbackend_amd import _lib
  lib = _lib.lib()
  rng = np.random.RandomState(dim * 2 + ragged)
  rows = 301
  table = _table(rng, dict(rows=rows, dim=dim, clip='ties'))
  lens = [120, 0, 101, 80]                       # logical rows of every run
  # runs stored in reverse order with gaps, each 16-byte aligned (the vec4 path) in a larger buffer
  bases, at = [0] * len(lens), 8
  for k in reversed(range(len(lens))):
    bases[k] = at
    at += (lens[k] * dim + 3) // 4 * 4 + 8
  buf = np.full(at, np.nan, F32)
  starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
  for k, ln in enumerate(lens):
    buf[bases[k]:bases[k] + ln * dim] = table[starts[k]:starts[k] + ln].reshape(-1)
  d_buf = dev(buf)
  d_start, d_base = dev(starts), dev(np.array(bases, np.int64))
  n_seg = 400
  if ragged:
    lens_s = rng.randint(0, 6, size=n_seg)
    sp = np.concatenate([[0], np.cumsum(lens_s)]).astype(np.int32)
  else:
    sp = None
  n = int(sp[-1]) if ragged else n_seg
  ids = rng.randint(-3, rows + 3, size=n).astype(np.int64)
  ids[:3] = [0, 1, 2]
  d_ids = dev(ids)
  d_sp = dev(sp) if ragged else None
  for weighted in (False, True):
    w = rng.uniform(-1, 2, size=n).astype(F32) if weighted else None
    d_w = dev(w) if weighted else None
    for clip in (0.0, CLIP_C):
      for comb_name, comb in (('sum', 0), ('mean', 1), ('sqrtn', 2)):
        if not ragged and comb:
          continue
        out = torch.full((n_seg, dim), float('nan'), device=DEV)
        cols = (_lib.LookupColumn * 1)()
        c = cols[0]
        c.table, c.rows, c.dim, c.ids_dtype = d_buf.data_ptr(), rows, dim, _lib.INT64
        c.ids, c.n_ids, c.n_segments, c.bucket, c.divisor = d_ids.data_ptr(), n, n_seg, 0, 1
        c.row_splits = d_sp.data_ptr() if ragged else None
        c.combiner, c.out = comb, out.data_ptr()
        c.run_start, c.run_base, c.n_runs = d_start.data_ptr(), d_base.data_ptr(), len(lens)
        c.id_weights = d_w.data_ptr() if weighted else None
        mn = (C.c_float * 1)(clip)
        _lib.check(lib.hbk_group_lookup_fwd_clipped(1, cols, mn, _lib.current_stream(DEV)))
        torch.cuda.synchronize()
        want, mag = ref.forward64(table, ids, sp, w, comb_name, clip)
        assert_sums_close(host(out), want, mag,
                          err_msg=f'dim {dim} ragged {ragged} weighted {weighted} clip {clip} {comb_name}')


# ---- captured graph on the sort path ------------------------------------------------------------------------
def test_graph_capture_deterministic_sort_path_adam(hbk_option):
  """bwd_deterministic = 2 (the sort for every column) under graph capture: weighted, clipped columns
  with a Lazy Adam step; K replays == K eager steps bit for bit, beta powers included."""
  from hybridbackend_amd.embedding import GroupLookup, GroupLookupGrad, LazyAdam
  hbk_option('bwd_deterministic', 2)
  rng = np.random.RandomState(3)
  K, lr = 4, 0.05
  specs = [dict(rows=3001, dim=16, clip='ties'), dict(rows=500, dim=3, clip='half'),
           dict(rows=2000, dim=64, clip='none')]
  tables = [_table(rng, s) for s in specs]
  sp = [np.concatenate([[0], np.cumsum(rng.randint(0, 6, size=700))]).astype(np.int32) for _ in specs]
  ids = [rng.randint(0, s['rows'], size=int(p[-1])).astype(np.int64) for s, p in zip(specs, sp)]
  for i in ids:
    i[:3] = [0, 1, 2]
  ws = [rng.uniform(0.1, 2, size=i.size).astype(F32) for i in ids]
  gs = [rng.randn(p.size - 1, s['dim']).astype(F32) for s, p in zip(specs, sp)]
  d = [[dev(x) for x in xs] for xs in (ids, sp, ws, gs)]

  def make():
    t = [dev(x) for x in tables]
    m = [(torch.zeros_like(x), torch.zeros_like(x)) for x in t]
    adam = LazyAdam(device=DEV)
    lk = GroupLookup(t, combiners=['sum', 'mean', 'sqrtn'], max_norms=[CLIP_C, CLIP_C, None])
    return t, m, adam, GroupLookupGrad(lk, moments=m, adam=adam)

  def result(x):
    t, m, adam, _ = x
    return [host(a) for a in t] + [host(a) for p in m for a in p] + [host(adam.beta_powers)]

  eager = make()
  for _ in range(K):
    eager[3](d[0], d[3], d[1], apply_lr=lr, optimizer='adam', sp_weights=d[2])
  graphed = make()
  graphed[3](d[0], d[3], d[1], apply_lr=lr, optimizer='adam', sp_weights=d[2])   # binds; step 1
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      graphed[3].launch(lr, optimizer='adam')
  torch.cuda.synchronize()
  for _ in range(K - 1):
    graph.replay()
  torch.cuda.synchronize()
  for a, b in zip(result(graphed), result(eager)):
    np.testing.assert_array_equal(a, b)
  p = (F32(0.9), F32(0.999))
  for _ in range(K):
    p = (F32(p[0] * F32(0.9)), F32(p[1] * F32(0.999)))
  np.testing.assert_array_equal(result(eager)[-1], np.array(p, F32))


# ---- refusals leave every state untouched -------------------------------------------------------------------
@pytest.mark.parametrize('case,optimizer',
                         [('clip_table_shared', o) for o in ('sgd', 'adagrad', 'adam', 'ftrl')] +
                         [('clip_table_is_accum', 'adagrad')] +
                         [(c, o) for c in ('two_slot_table_shared', 'two_slot_slot_shared') for o in ('adam', 'ftrl')])
def test_refusals_leave_state_bit_identical(case, optimizer):
  """A stepping call in which a clipped column's table is named by another column, and a two-slot call
  whose columns share a table or a slot, are refused; every table, slot and power keeps its bits."""
  from hybridbackend_amd import _lib
  from hybridbackend_amd.embedding import Ftrl, GroupLookup, GroupLookupGrad, LazyAdam
  rng = np.random.RandomState(len(case) + len(optimizer))
  rows, dim = 211, 16
  t0 = dev(_table(rng, dict(rows=rows, dim=dim, clip='half')))
  t1 = dev(_table(rng, dict(rows=rows, dim=dim, clip='half')))
  a0, a1 = torch.full_like(t0, 0.1), torch.full_like(t1, 0.1)
  s = [(dev(rng.uniform(0.1, 1, size=(rows, dim)).astype(F32)), dev(rng.uniform(-1, 1, size=(rows, dim)).astype(F32)))
       for _ in range(2)]
  adam = LazyAdam(device=DEV)
  ftrl = Ftrl(l1=0.05)
  if case == 'clip_table_shared':
    tabs, maxn, slots = [t0, t0], [CLIP_C, None], [s[0], s[1]]
  elif case == 'clip_table_is_accum':
    tabs, maxn, slots = [t0, t1], [CLIP_C, None], [s[0], s[1]]
  elif case == 'two_slot_table_shared':
    tabs, maxn, slots = [t0, t0], [None, None], [s[0], s[1]]
  else:
    tabs, maxn, slots = [t0, t1], [None, None], [s[0], (s[0][0], s[1][1])]
  accs = [a0, t0] if case == 'clip_table_is_accum' else [a0, a1]
  everything = [t0, t1, a0, a1, s[0][0], s[0][1], s[1][0], s[1][1], adam.beta_powers]
  before = [host(x) for x in everything]
  sp = np.arange(0, 301, 3).astype(np.int32)
  ids = [dev(rng.randint(0, rows, size=300).astype(np.int64)) for _ in range(2)]
  grads = [dev(rng.randn(100, dim).astype(F32)) for _ in range(2)]
  with pytest.raises(_lib.HbkError):
    lk = GroupLookup(tabs, combiners='mean', max_norms=maxn)
    kw = {'accums': accs}
    if optimizer == 'adam':
      kw = dict(moments=slots, adam=adam)
    elif optimizer == 'ftrl':
      kw = dict(ftrl_slots=slots, ftrl=ftrl)
    g = GroupLookupGrad(lk, **kw)
    g(ids, grads, [dev(sp), dev(sp)], apply_lr=0.05, optimizer=optimizer)
  torch.cuda.synchronize()
  for x, y in zip(everything, before):
    np.testing.assert_array_equal(host(x), y)


# ---- sharded backward ---------------------------------------------------------------------------------------
sharded_feature_column = st.fixed_dictionaries({
  'dim': st.sampled_from([4, 6, 8, 16, 20, 64]),
  'rows': st.sampled_from([3, 64, 1000, 50021]),
  'ragged': st.booleans(),
  'combiner': st.sampled_from(['sum', 'mean', 'sqrtn']),
  'weights': st.sampled_from(['none', 'uniform', 'signed']),
  'clip': st.sampled_from(['none', 'half', 'ties']),
})
sharded_plan = st.fixed_dictionaries({
  'bwd_deterministic': st.sampled_from([0, 1]),
  'sharded_inline': st.sampled_from([0, 1]),
  'sharded_pack_early': st.sampled_from([0, 1]),
  'sharded_wire_fused': st.sampled_from([0, 1]),
  'sharded_id64': st.sampled_from([0, 1]),
  'sharded_groups': st.sampled_from([0, 1, 3]),
})


@_cfg(60)
@given(world=st.sampled_from([2, 3, 5]), cols=st.lists(sharded_feature_column, min_size=1, max_size=4),
       wire16=st.booleans(), hot=st.booleans(), dedup=st.sampled_from(['none', 'all', 'mixed']),
       optimizer=st.sampled_from(['emit', 'sgd', 'adagrad', 'adam', 'ftrl']), plan=sharded_plan,
       seed=st.integers(0, 2**31 - 1))
def test_sharded_features_random_in_process_world(world, cols, wire16, hot, dedup, optimizer, plan, seed):
  """hbk_sharded_lookup_fwd/_bwd with weights, max_norm and every optimizer step in an in-process world:
  the forward within the float64 world forward (the owner clips in fp32, then the wire), the emitted
  slices within the bound of the float64 world g', every stepped shard row bit-equal to its rule on the
  slices the call returned, untouched shard rows bit-unchanged."""
  import hybridbackend_amd as hb
  from hybridbackend_amd import _lib
  from hybridbackend_amd.embedding import Ftrl, LazyAdam
  from hybridbackend_amd.embedding.sharded import ShardedGroupLookup
  rng = np.random.RandomState(seed)
  n = len(cols)
  dims = [c['dim'] for c in cols]
  rows = [max(c['rows'], world) for c in cols]
  combs = [c['combiner'] for c in cols]
  tables = [_table(rng, dict(c, rows=rows[k])) for k, c in enumerate(cols)]
  maxn = [CLIP_C if c['clip'] != 'none' else 0.0 for c in cols]
  ids, splits, grads, wts = [], [], [], []
  for r in range(world):
    ri, rs, rg, rw = [], [], [], []
    for k, c in enumerate(cols):
      n_seg = int(rng.choice([0, 1, 77, 600]))
      if c['ragged']:
        sp = np.concatenate([[0], np.cumsum(rng.randint(0, 6, size=n_seg))]).astype(np.int32)
        cnt = int(sp[-1])
      else:
        sp, cnt = None, n_seg
      hi = 2**40 if k % 2 == 0 else 40
      i = rng.randint(0, hi, size=cnt).astype(np.int64)
      if c['clip'] == 'ties' and cnt >= 3:
        i[:3] = [0, 1, 2]
      w = None
      if c['weights'] == 'uniform':
        w = rng.uniform(0.1, 2, size=cnt).astype(F32)
      elif c['weights'] == 'signed':
        w = rng.uniform(-1, 2, size=cnt).astype(F32)
        w[rng.rand(cnt) < 0.2] = 0
      ri.append(i)
      rs.append(sp)
      rg.append(rng.randn(n_seg, dims[k]).astype(F32))
      rw.append(w)
    ids.append(ri)
    splits.append(rs)
    grads.append(rg)
    wts.append(rw)
  comms = hb.distribute.Collective.local_world(world)
  shards = [[dev(t[r::world].copy()) for t in tables] for r in range(world)]
  kw = [{} for _ in range(world)]
  slots = [None] * world
  ftrl = Ftrl(l1=0.05, l2=1e-5, l2_shrinkage=0.01)
  for r in range(world):
    if optimizer == 'adagrad':
      slots[r] = [(torch.full_like(s, 0.1),) for s in shards[r]]
      kw[r] = dict(accums=[s[0] for s in slots[r]])
    elif optimizer == 'adam':
      slots[r] = [(torch.zeros_like(s), torch.zeros_like(s)) for s in shards[r]]
      kw[r] = dict(moments=slots[r], adam=LazyAdam(device=DEV))
    elif optimizer == 'ftrl':
      slots[r] = [(torch.full_like(s, 0.1), torch.zeros_like(s)) for s in shards[r]]
      kw[r] = dict(ftrl_slots=slots[r], ftrl=ftrl)
  before = [[[host(s)] + ([host(x) for x in slots[r][k]] if slots[r] else []) for k, s in enumerate(shards[r])]
            for r in range(world)]
  results, errors, done = [None] * world, [], [False] * world
  lr = 0.05

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        drv = ShardedGroupLookup(shards[r], comms[r], buckets=rows, combiners=combs,
                                 wire_dtype=torch.float16 if wire16 else None, hot_rows=hot,
                                 dedup=[dedup == 'all' or (dedup == 'mixed' and k % 2 == 1) for k in range(n)],
                                 max_norms=[m or None for m in maxn], **kw[r])
        d_w = [None if w is None else dev(w) for w in wts[r]]
        outs = drv([dev(i) for i in ids[r]], [None if s is None else dev(s) for s in splits[r]],
                   sp_weights=d_w if any(w is not None for w in wts[r]) else None)
        if optimizer == 'emit':
          sl = drv.backward([dev(g) for g in grads[r]])
        else:
          sl = drv.backward([dev(g) for g in grads[r]], apply_lr=lr, optimizer=optimizer)
        torch.cuda.current_stream().synchronize()
        results[r] = ([host(o) for o in outs],
                      [(host(u)[:int(q.item())], host(g)[:int(q.item())]) for u, g, q in sl],
                      kw[r].get('adam').beta_powers.cpu().numpy() if optimizer == 'adam' else None)
        drv.close()
        done[r] = True
    except Exception as e:  # pylint: disable=broad-except
      errors.append((r, repr(e)))

  old = {k: _lib.set_option(k, v) for k, v in plan.items()}
  try:
    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
      t.start()
    for t in threads:
      t.join(timeout=120)
    alive = [t.is_alive() for t in threads]
  finally:
    for k, v in old.items():
      _lib.set_option(k, v)
  for cm in comms:
    cm.close()
  assert not any(alive), f'worker threads still running: {alive}'
  assert not errors, errors
  assert all(done), done
  rel, floor = (WIRE16_REL, WIRE16_FLOOR) if wire16 else (REL, FLOOR)
  for r in range(world):
    for k in range(n):
      y = ref.clip64(tables[k], maxn[k])
      if wire16:          # the owner clips in fp32, then the rows travel as fp16
        y = ref.clip64(tables[k], maxn[k]).astype(F32).astype(np.float16).astype(F64)
      want, mag = ref.forward64(y, ids[r][k], splits[r][k], wts[r][k], combs[k], 0.0, rows[k])
      assert_sums_close(results[r][0][k], want, mag, rel=rel, floor=floor, err_msg=f'fwd rank {r} col {k}')
  for k in range(n):
    G = np.zeros((rows[k], dims[k]))
    M = np.zeros((rows[k], dims[k]))
    for r in range(world):
      rr, valid = ref.rows_of(ids[r][k], rows[k], rows[k])
      seg, f, _, cond = ref.factors64(splits[r][k], ids[r][k].size, wts[r][k], combs[k], valid)
      t = np.asarray(grads[r][k], F64)[seg] * f[:, None]
      np.add.at(G, rr, t)
      np.add.at(M, rr, np.abs(t) * cond[:, None])
    touched = np.unique(np.concatenate([ref.rows_of(ids[r][k], rows[k], rows[k])[0] for r in range(world)]))
    gp, gm = ref.clip_jacobian64(tables[k][touched], G[touched], M[touched], maxn[k])
    got = np.zeros((rows[k], dims[k]))
    seen = np.zeros(rows[k], bool)
    for r in range(world):
      lu, lg = results[r][1][k]
      assert np.unique(lu).size == lu.size, f'rank {r} col {k}: a row emitted twice'
      got[lu * world + r] = lg
      seen[lu * world + r] = True
    np.testing.assert_array_equal(np.nonzero(seen)[0], touched, err_msg=f'col {k}: emitted rows')
    assert_sums_close(got[touched], gp, gm, rel=rel, floor=floor, err_msg=f'emit col {k}')
    for r in range(world):
      lu, lg = results[r][1][k]
      b = before[r][k]
      w0 = b[0].copy()
      s0 = b[1].copy() if len(b) > 1 else None
      s1 = b[2].copy() if len(b) > 2 else None
      if optimizer == 'sgd':
        ref.sgd_step(w0, lu, lg, lr)
      elif optimizer == 'adagrad':
        ref.adagrad_step(w0, s0, lu, lg, lr)
      elif optimizer == 'adam':
        ref.adam_step(w0, s0, s1, lu, lg, lr, ADAM_P0)
      elif optimizer == 'ftrl':
        ref.ftrl_step(w0, s0, s1, lu, lg, lr, ftrl.l1, ftrl.l2, ftrl.l2_shrinkage, ftrl.lr_power)
      got_state = [host(shards[r][k])] + ([host(x) for x in slots[r][k]] if slots[r] else [])
      for j, (x, want) in enumerate(zip(got_state, [w0, s0, s1])):
        np.testing.assert_array_equal(x, want, err_msg=f'rank {r} col {k} state {j} ({optimizer})')
    if optimizer == 'adam':
      for r in range(world):
        np.testing.assert_array_equal(results[r][2], np.array(ref.adam_finish(ADAM_P0), F32))
