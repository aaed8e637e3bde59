"""Gradient with respect to sp_weights (hbk_group_lookup_bwd_weights, hbk_sharded_lookup_bwd_weights,
GroupLookupGrad / ShardedGroupLookup / DenseFeatures weight_grads=): against the float64 restatement in
tests/support/weight_grad_ref.py within the project's one bound (tests/support/tolerance), exact
checks, stepping calls, graph capture, the sharded step, DenseFeatures and a finite difference through
the shipped forward."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import GroupLookup, GroupLookupGrad
from hybridbackend_amd.embedding.sharded import ShardedGroupLookup
from tests.support import reference
from tests.support import weight_grad_ref as ref
from tests.support.tolerance import WIRE16_FLOOR, WIRE16_REL, assert_sums_close
from tests.test_gpu_row_layouts import placed

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
COMBS = ['sum', 'mean', 'sqrtn']


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.detach().cpu().numpy()


def splits_of(rng, layout, n_seg):
  if layout == 'h1':
    return None
  if layout == 'fixed':
    return (np.arange(n_seg + 1) * 3).astype(np.int32)
  lens = rng.choice([0, 0, 1, 2, 3, 5, 9, 17], size=n_seg)   # ragged, empty segments included
  return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def table_of(rng, rows, dim, clip):
  """Rows on both sides of the ball of radius `clip`: norms from 0.2 to 3 times it."""
  t = rng.uniform(-1, 1, size=(rows, dim))
  t /= np.maximum(np.sqrt((t * t).sum(1, keepdims=True)), 1e-6)
  t *= rng.uniform(0.2, 3.0, size=(rows, 1)) * (clip or 1.0)
  t[0] = 0.0
  return t.astype(F32)


def mixed_sign_weights(rng, sp, n):
  """Weights of both signs whose segment sums stay away from 0: |W_s| >= sum|w| / 4 (checked)."""
  w = rng.uniform(0.5, 2.0, size=n)
  sp = np.arange(n + 1) if sp is None else sp
  for s in range(sp.size - 1):
    j = np.arange(sp[s], sp[s + 1])
    if j.size == 0:
      continue
    flip = rng.rand(j.size) < 0.35
    if abs((w[j] * np.where(flip, -1, 1)).sum()) >= 0.25 * w[j].sum():
      w[j] = w[j] * np.where(flip, -1, 1)
    elif j.size == 1:
      w[j] = -w[j]
  return w.astype(F32)


def case(rng, comb, layout, dim, clip, n_seg=300, rows=1009, weights='positive', bucket=True):
  sp = splits_of(rng, layout, n_seg)
  n = n_seg if sp is None else int(sp[-1])
  ids = rng.randint(0, 1 << 40, size=n).astype(np.int64) if bucket else \
      rng.randint(-30, rows + 80, size=n).astype(np.int64)
  w = rng.uniform(0.25, 2.0, size=n).astype(F32) if weights == 'positive' else mixed_sign_weights(rng, sp, n)
  return dict(table=table_of(rng, rows, dim, clip), ids=ids, sp=sp, w=w, comb=comb, clip=clip,
              bucket=rows if bucket else 0, G=rng.randn(n_seg, dim).astype(F32))


def want_of(k):
  dw, mag, cancel = ref.weight_grad(k['table'], k['ids'], k['sp'], k['w'], k['comb'], k['G'],
                                    bucket=k['bucket'], max_norm=k['clip'])
  assert cancel.min() >= 0.2, 'the draw must keep every divisor away from cancelling'
  return dw, mag


def run_fused(cases, **kw):
  """The cases as the columns of ONE GroupLookupGrad call; returns (grad object, result, weight grads)."""
  lk = GroupLookup([dev(k['table']) for k in cases], buckets=[k['bucket'] for k in cases],
                   combiners=[k['comb'] for k in cases], max_norms=[k['clip'] for k in cases])
  grad = GroupLookupGrad(lk, **kw.pop('ctor', {}))
  res = grad([dev(k['ids']) for k in cases], [dev(k['G']) for k in cases],
             [None if k['sp'] is None else dev(k['sp']) for k in cases],
             sp_weights=[dev(k['w']) for k in cases], weight_grads=True, **kw)
  torch.cuda.synchronize()
  return grad, res[0], res[1]


# ---- 1. comparison with the float64 restatement -------------------------------------------------------
@pytest.mark.parametrize('clip', [None, 0.5])
@pytest.mark.parametrize('layout', ['h1', 'fixed', 'ragged'])
@pytest.mark.parametrize('comb', COMBS)
def test_fused_against_float64(comb, layout, clip):
  rng = np.random.RandomState(11)
  cases = [case(rng, comb, layout, d, clip, rows=1009 + 7 * d) for d in (1, 3, 16, 17, 128)]
  _, _, wg = run_fused(cases)
  for k, g in zip(cases, wg):
    dw, mag = want_of(k)
    assert g.dtype is torch.float32 and tuple(g.shape) == (k['ids'].size,)
    assert_sums_close(host(g), dw, mag, err_msg=f'{comb} {layout} dim {k["table"].shape[1]} clip {clip}')


@pytest.mark.parametrize('comb', ['mean', 'sqrtn'])
def test_parked_in_lds_or_swept_in_memory_same_bits(hbk_option, comb):
  """Segments of more than L and at most 8 L ids wait for A_s in LDS (option bwd_weights_lds, default 1)
  or in the output (0): the same arithmetic, so the same bits, and both within the bound."""
  rng = np.random.RandomState(22)
  got = {}
  for lds in (1, 0):
    hbk_option('bwd_weights_lds', lds)
    rng = np.random.RandomState(22)
    cases = [case(rng, comb, 'ragged', d, clip) for d, clip in ((16, None), (3, 0.5), (17, None), (64, 0.5))]
    lens = np.diff(cases[0]['sp'])
    assert ((lens > 4) & (lens <= 32)).any() and (lens <= 4).any()
    got[lds] = [host(g) for g in run_fused(cases)[2]]
  for k, a, b in zip(cases, got[1], got[0]):
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    dw, mag = want_of(k)
    assert_sums_close(a, dw, mag, err_msg=f'{comb} dim {k["table"].shape[1]}')


@pytest.mark.parametrize('comb', COMBS)
def test_negative_weights(comb):
  rng = np.random.RandomState(12)
  cases = [case(rng, comb, lay, d, clip, weights='mixed')
           for lay, d, clip in (('ragged', 16, None), ('fixed', 17, 0.5), ('h1', 16, None), ('ragged', 128, 2.0))]
  assert all((k['w'] < 0).any() and (k['w'] > 0).any() for k in cases)
  _, _, wg = run_fused(cases)
  for k, g in zip(cases, wg):
    dw, mag = want_of(k)
    assert_sums_close(host(g), dw, mag, err_msg=f'{comb} mixed signs')


@pytest.mark.parametrize('comb', COMBS)
def test_one_segment_much_longer_than_a_workgroup(comb):
  rng = np.random.RandomState(13)
  for dim, clip in ((16, None), (3, 0.5)):
    lens = rng.choice([0, 1, 2, 4], size=200)
    lens[57] = 20000     # a workgroup's share is 4 segments per lane group: far beyond it
    sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    k = case(rng, comb, 'h1', dim, clip, n_seg=200)
    n = int(sp[-1])
    k.update(sp=sp, ids=rng.randint(0, 1 << 40, size=n).astype(np.int64),
             w=rng.uniform(0.25, 2.0, size=n).astype(F32))
    _, _, wg = run_fused([k])
    dw, mag = want_of(k)
    assert_sums_close(host(wg[0]), dw, mag, err_msg=f'{comb} long segment dim {dim}')


@pytest.mark.parametrize('comb', COMBS)
@pytest.mark.parametrize('dim,shift,gap', [(16, 1, 0), (16, 0, 1), (5, 2, 3), (64, 3, 1)])
def test_unaligned_row_pitch(comb, dim, shift, gap):
  """The table placed `shift` floats into a sentinel arena with a row pitch of dim + gap (the C entry:
  hbk_lookup_grad_column_t.table_pitch), the gradient rows strided likewise."""
  rng = np.random.RandomState(14)
  k = case(rng, comb, 'ragged', dim, 0.5)
  rows = k['table'].shape[0]
  t, tcheck = placed((rows, dim), shift, dim + gap)
  t.copy_(dev(k['table']))
  g, gcheck = placed(k['G'].shape, shift, dim + gap + 4)
  g.copy_(dev(k['G']))
  ids, sp, w = dev(k['ids']), dev(k['sp']), dev(k['w'])
  out = torch.full((k['ids'].size,), float('nan'), dtype=torch.float32, device=DEV)
  col = _lib.LookupGradColumn()
  col.table, col.rows, col.dim, col.table_pitch = t.data_ptr(), rows, dim, dim + gap
  col.ids_dtype, col.ids, col.n_ids = _lib.INT64, ids.data_ptr(), ids.numel()
  col.row_splits, col.n_segments = sp.data_ptr(), sp.numel() - 1
  col.bucket, col.divisor = k['bucket'], 1
  col.combiner = {'sum': _lib.COMBINER_SUM, 'mean': _lib.COMBINER_MEAN, 'sqrtn': _lib.COMBINER_SQRTN}[comb]
  col.grad_out, col.grad_stride, col.id_weights = g.data_ptr(), dim + gap + 4, w.data_ptr()
  cols = (_lib.LookupGradColumn * 1)(col)
  _lib.check(_lib.lib().hbk_group_lookup_bwd_weights(1, cols, (C.c_float * 1)(0.5), _lib.ptr_array([out.data_ptr()]),
                                                     _lib.current_stream(DEV)))
  torch.cuda.synchronize()
  tcheck('table arena')
  gcheck('gradient arena')
  dw, mag = want_of(k)
  assert_sums_close(host(out), dw, mag, err_msg=f'{comb} dim {dim} shift {shift} gap {gap}')


# ---- 2. exact checks ------------------------------------------------------------------------------------
@pytest.mark.parametrize('comb', COMBS)
def test_one_id_per_segment_exact_checks(comb):
  """row_splits = None: zero weights (a zero divisor for mean and sqrtn), ids outside the table, a
  NaN-filled output, two runs."""
  rng = np.random.RandomState(21)
  k = case(rng, comb, 'h1', 16, 0.5, n_seg=1000, bucket=False)   # ids on both sides of [0, rows)
  zero = np.arange(0, 1000, 7)
  k['ids'][zero] = rng.randint(0, 1009, size=zero.size)
  k['w'][zero] = 0.0
  _, valid = ref.rows_of(k['ids'], 1009)
  assert (~valid).sum() > 10
  lk = GroupLookup([dev(k['table'])], combiners=comb, max_norms=[0.5])
  grad = GroupLookupGrad(lk)
  outs = [torch.full((1000,), float('nan'), dtype=torch.float32, device=DEV) for _ in range(2)]
  for o in outs:
    grad([dev(k['ids'])], [dev(k['G'])], sp_weights=[dev(k['w'])], weight_grads=[o])
  torch.cuda.synchronize()
  a, b = host(outs[0]), host(outs[1])
  assert not np.isnan(a).any(), 'every position of the output is written'
  np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
  assert (a[~valid] == 0).all()
  if comb != 'sum':
    assert (a[zero] == 0).all()
  dw, mag, _ = ref.weight_grad(k['table'], k['ids'], None, k['w'], comb, k['G'], max_norm=0.5)
  assert_sums_close(a, dw, mag, err_msg=f'{comb} one id per segment')


@pytest.mark.parametrize('comb', COMBS)
def test_zero_divisor_out_of_range_nan_prefill_and_bits(comb):
  rng = np.random.RandomState(15)
  k = case(rng, comb, 'ragged', 16, None, bucket=False)   # ids on both sides of [0, rows)
  sp = k['sp']
  lens = np.diff(sp)
  z = [s for s in range(lens.size) if lens[s] == 2][:5] + [s for s in range(lens.size) if lens[s] == 3][:3]
  assert len(z) >= 4
  zero_ids = []
  for s in z:
    j = np.arange(sp[s], sp[s + 1])
    k['ids'][j] = rng.randint(0, 1009, size=j.size)    # valid rows: the divisor is what is zero
    k['w'][j] = 0.0 if comb == 'sqrtn' or j.size == 3 else np.array([1.5, -1.5], F32)
    zero_ids.extend(j.tolist())
  _, valid = ref.rows_of(k['ids'], 1009)
  assert (~valid).sum() > 10
  lk = GroupLookup([dev(k['table'])], combiners=comb)
  grad = GroupLookupGrad(lk)
  outs = [torch.full((k['ids'].size,), float('nan'), dtype=torch.float32, device=DEV) for _ in range(2)]
  args = ([dev(k['ids'])], [dev(k['G'])], [dev(sp)])
  for o in outs:
    res = grad(*args, sp_weights=[dev(k['w'])], weight_grads=[o])
    assert res[1][0] is o
  torch.cuda.synchronize()
  a, b = host(outs[0]), host(outs[1])
  assert not np.isnan(a).any(), 'every position of the output is written'
  np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))   # run to run: the same bits
  assert (a[~valid] == 0).all()
  if comb != 'sum':
    assert (a[zero_ids] == 0).all()
  dw, mag, _ = ref.weight_grad(k['table'], k['ids'], sp, k['w'], comb, k['G'])
  assert_sums_close(a, dw, mag, err_msg=f'{comb} with zero divisors and invalid ids')


def test_flag_off_returns_what_it_returned_and_refusals():
  rng = np.random.RandomState(16)
  k = case(rng, 'mean', 'ragged', 16, None)
  lk = GroupLookup([dev(k['table'])] * 2, buckets=[k['bucket']] * 2, combiners='mean')
  grad = GroupLookupGrad(lk, deterministic=True)
  ids, G, sp, w = dev(k['ids']), dev(k['G']), dev(k['sp']), dev(k['w'])
  plain = grad([ids, ids], [G, G], [sp, sp], sp_weights=[w, None])
  assert isinstance(plain, list) and len(plain) == 2 and len(plain[0]) == 3
  res, wg = grad([ids, ids], [G, G], [sp, sp], sp_weights=[w, None], weight_grads=True)
  assert wg[1] is None and wg[0] is not None
  with pytest.raises(_lib.InvalidArgumentError):
    grad([ids, ids], [G, G], [sp, sp], sp_weights=[w, None], weight_grads=[None, True])
  with pytest.raises(_lib.InvalidArgumentError):
    grad([ids, ids], [G, G], [sp, sp], weight_grads=True)
  with pytest.raises(_lib.InvalidArgumentError):
    grad([ids, ids], [G, G], [sp, sp], sp_weights=[w, None], weight_grads=[torch.zeros(3, device=DEV), None])


# ---- 3. stepping calls -----------------------------------------------------------------------------------
LR = 0.05


def _stepper(opt, tables):
  """(GroupLookupGrad keyword arguments, numpy step over a pre-step table given the rows and their fp32
  gradient): the fp32 rules of include/hbk.h as tests/support/reference.py restates them."""
  if opt == 'sgd':
    return {}, lambda w, u, g: reference.sgd_step(w, u, g, LR)
  if opt == 'adagrad':
    return (dict(accums=[torch.full_like(t, 0.1) for t in tables]),
            lambda w, u, g: reference.adagrad_step(w, np.full_like(w, F32(0.1)), u, g, LR))
  if opt == 'adam':
    adam = hb.embedding.LazyAdam(device=DEV)
    return (dict(moments=[(torch.zeros_like(t), torch.zeros_like(t)) for t in tables], adam=adam),
            lambda w, u, g: reference.adam_step(w, np.zeros_like(w), np.zeros_like(w), u, g, LR,
                                                (F32(0.9), F32(0.999))))
  f = hb.embedding.Ftrl(l1=0.001)
  return (dict(ftrl_slots=[f.slots_like(t) for t in tables], ftrl=f),
          lambda w, u, g: reference.ftrl_step(w, np.full_like(w, F32(0.1)), np.zeros_like(w), u, g, LR,
                                              0.001, 0.0, 0.0, -0.5))


@pytest.mark.parametrize('clip', [None, 0.5])
@pytest.mark.parametrize('opt', ['sgd', 'adagrad', 'adam', 'ftrl'])
def test_stepping_calls_read_the_rows_before_the_step(opt, clip):
  """A stepping call with weight_grads=True returns the weight gradient of a call that does not step.  Its
  IndexedSlices are within the bound of the float64 gradient (through the clip: reference.backward64), and
  its stepped tables are the fp32 step rule applied to those very slices (the emitted rows are the g the
  step used: bit-equal, as tests/test_gpu_adam.py::test_one_step_bit_equal_to_its_own_slices holds every
  step to) -- in the reproducible mode, where tables and slices also equal bit for bit those of the same
  call without the flag, and in the run-dependent mode."""
  rng = np.random.RandomState(17)
  cases = [case(rng, 'mean', 'ragged', 16, clip), case(rng, 'sqrtn', 'h1', 8, clip),
           case(rng, 'sum', 'fixed', 32, clip)]
  d = dict(ids=[dev(k['ids']) for k in cases], G=[dev(k['G']) for k in cases],
           sp=[None if k['sp'] is None else dev(k['sp']) for k in cases], w=[dev(k['w']) for k in cases])
  np_step = [None]

  def run(flag, deterministic, step=True):
    tables = [dev(k['table']) for k in cases]
    lk = GroupLookup(tables, buckets=[k['bucket'] for k in cases], combiners=[k['comb'] for k in cases],
                     max_norms=[k['clip'] for k in cases])
    kw, np_step[0] = _stepper(opt, tables)
    grad = GroupLookupGrad(lk, deterministic=deterministic, **kw)
    r = grad(d['ids'], d['G'], d['sp'], apply_lr=LR if step else 0.0, optimizer=opt, sp_weights=d['w'],
             weight_grads=flag)
    torch.cuda.synchronize()
    res, wg = r if flag else (r, None)
    slices = []
    for u, g, nu in res:
      n = int(nu.item())
      order = np.argsort(host(u)[:n], kind='stable')
      slices.append((host(u)[:n][order], host(g)[:n][order]))
    return [host(t) for t in tables], slices, None if wg is None else [host(x) for x in wg]

  _, _, wg_plain = run(True, True, step=False)
  for deterministic in (True, False):
    t_on, s_on, wg_step = run(True, deterministic)
    t_off, s_off, _ = run(False, deterministic)
    for c, k in enumerate(cases):
      what = f'{opt} clip {clip} deterministic {deterministic} col {c}'
      # the same gradient as a call that does not step: the rows were read before the step
      np.testing.assert_array_equal(wg_step[c].view(np.uint32), wg_plain[c].view(np.uint32), err_msg=what)
      dw, mag = want_of(k)
      assert_sums_close(wg_step[c], dw, mag, err_msg=what)
      # IndexedSlices, with the flag and without: within the bound of the float64 gradient
      u, gp, gm = reference.backward64(k['table'], k['ids'], k['sp'], k['w'], k['comb'], k['G'],
                                       max_norm=k['clip'] or 0.0, bucket=k['bucket'])
      for rows_got, g_got in (s_on[c], s_off[c]):
        np.testing.assert_array_equal(rows_got, u, err_msg=what)
        assert_sums_close(g_got, gp, gm, err_msg='slices ' + what)
      # stepped tables: the fp32 step of the call's own slices on the pre-step table, nothing else moved
      for t_got, (rows_got, g_got) in ((t_on[c], s_on[c]), (t_off[c], s_off[c])):
        want = k['table'].copy()
        np_step[0](want, rows_got, g_got)
        assert not np.array_equal(want, k['table'])
        np.testing.assert_array_equal(t_got.view(np.uint32), want.view(np.uint32), err_msg='table ' + what)
      if deterministic:
        # reproducible mode: the flag changes no bit of the tables and the slices
        np.testing.assert_array_equal(t_on[c].view(np.uint32), t_off[c].view(np.uint32), err_msg=what)
        np.testing.assert_array_equal(s_on[c][1].view(np.uint32), s_off[c][1].view(np.uint32), err_msg=what)


# ---- 4. graph capture ------------------------------------------------------------------------------------
def test_launch_form_inside_a_captured_graph():
  rng = np.random.RandomState(18)
  cases = [case(rng, 'mean', 'ragged', 16, 0.5), case(rng, 'sqrtn', 'h1', 16, None)]
  lk = GroupLookup([dev(k['table']) for k in cases], buckets=[k['bucket'] for k in cases],
                   combiners=[k['comb'] for k in cases], max_norms=[k['clip'] for k in cases])
  grad = GroupLookupGrad(lk, deterministic=True)
  outs = [torch.zeros(k['ids'].size, dtype=torch.float32, device=DEV) for k in cases]
  args = ([dev(k['ids']) for k in cases], [dev(k['G']) for k in cases],
          [None if k['sp'] is None else dev(k['sp']) for k in cases])
  ws = [dev(k['w']) for k in cases]
  # warm-up outside the capture: descriptors, workspace and result buffers exist before it
  grad(*args, sp_weights=ws, weight_grads=outs)
  torch.cuda.synchronize()
  first = [host(o).copy() for o in outs]
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):
      res, wg = grad.launch()
  torch.cuda.synchronize()
  assert all(a is b for a, b in zip(wg, outs))
  for _ in range(3):
    for o in outs:
      o.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    for k, o, f in zip(cases, outs, first):
      np.testing.assert_array_equal(host(o).view(np.uint32), f.view(np.uint32))
      dw, mag = want_of(k)
      assert_sums_close(host(o), dw, mag, err_msg='replay')


# ---- 5. sharded ------------------------------------------------------------------------------------------
def _threads(world, run):
  errors = []

  def guarded(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        run(r)
    except Exception as e:  # pylint: disable=broad-except
      errors.append((r, repr(e)))
  ts = [threading.Thread(target=guarded, args=(r,)) for r in range(world)]
  for t in ts:
    t.start()
  for t in ts:
    t.join(timeout=120)
  assert not errors, errors


@pytest.mark.parametrize('world,dedup,wire16', [(2, False, False), (2, True, True), (4, True, False),
                                                (4, False, True)])
def test_sharded_equals_single_gpu(world, dedup, wire16):
  rng = np.random.RandomState(600 + world)
  spec = [('sum', 'h1', 16, None), ('mean', 'ragged', 8, 0.5), ('sqrtn', 'ragged', 32, None),
          ('mean', 'fixed', 4, None)]
  per_rank = [[case(rng, comb, lay, d, clip, n_seg=200, rows=997 + 4 * d) for comb, lay, d, clip in spec]
              for _ in range(world)]
  n = len(spec)
  for r in range(1, world):     # one logical table per column
    for c in range(n):
      per_rank[r][c]['table'] = per_rank[0][c]['table']
      # Zipf-like repeats so that dedup has duplicates to share rows between
      per_rank[r][c]['ids'] = (rng.zipf(1.3, size=per_rank[r][c]['ids'].size) * 7919).astype(np.int64)
  tables = [k['table'] for k in per_rank[0]]
  rows = [t.shape[0] for t in tables]
  comms = hb.distribute.Collective.local_world(world)
  got = [None] * world

  def run(r):
    ks = per_rank[r]
    drv = ShardedGroupLookup([dev(t[r::world].copy()) for t in tables], comms[r], buckets=rows,
                             combiners=[k['comb'] for k in ks], dedup=[dedup] * n,
                             wire_dtype=torch.float16 if wire16 else None,
                             max_norms=[k['clip'] for k in ks], weight_grads=True)
    ids = [dev(k['ids']) for k in ks]
    sps = [None if k['sp'] is None else dev(k['sp']) for k in ks]
    ws = [dev(k['w']) for k in ks]
    w3 = [ws[0], ws[1], ws[2], None]          # the last column unweighted
    gs = [dev(k['G']) for k in ks]
    drv(ids, sps, sp_weights=w3)
    res, wg = drv.backward(gs)
    torch.cuda.current_stream().synchronize()
    assert wg[3] is None and len(res) == n
    # the row backward has run: the received rows are gone, a second request is refused
    rc = drv._lib.hbk_sharded_lookup_bwd_weights(
      drv._plan(), _lib.ptr_array([g.data_ptr() for g in gs]), None,
      _lib.ptr_array([wg[0].data_ptr(), 0, 0, 0]), _lib.current_stream(DEV))
    assert rc == _lib.INVALID_ARGUMENT
    # a stepping backward returns the same weight gradient (rows before the step)
    drv(ids, sps, sp_weights=w3)
    _, wg2 = drv.backward(gs, apply_lr=0.1, emit=False)
    torch.cuda.current_stream().synchronize()
    got[r] = ([host(x) for x in wg[:3]], [host(x) for x in wg2[:3]])
    drv.close()

  _threads(world, run)
  rel, floor = (WIRE16_REL, WIRE16_FLOOR) if wire16 else (1e-5, 1e-6)
  for r in range(world):
    fused = run_fused(per_rank[r][:3])[2]
    for c in range(3):
      dw, mag = want_of(per_rank[r][c])
      assert_sums_close(host(fused[c]), dw, mag, err_msg=f'fused rank {r} col {c}')
      assert_sums_close(got[r][0][c], dw, mag, rel=rel, floor=floor, err_msg=f'sharded rank {r} col {c}')
      np.testing.assert_array_equal(got[r][0][c].view(np.uint32), got[r][1][c].view(np.uint32))
  for cm in comms:
    cm.close()


def test_sharded_refusals_on_every_rank():
  world = 2
  rng = np.random.RandomState(19)
  k = case(rng, 'mean', 'h1', 16, None, n_seg=64, rows=100)
  comms = hb.distribute.Collective.local_world(world)
  codes = [None] * world

  def run(r):
    drv = ShardedGroupLookup([dev(k['table'][r::world].copy())], comms[r], buckets=[100], combiners='mean')
    ids, w, G = dev(k['ids']), dev(k['w']), dev(k['G'])
    out = torch.zeros(64, dtype=torch.float32, device=DEV)
    call = lambda: drv._lib.hbk_sharded_lookup_bwd_weights(   # noqa: E731
      drv._plan(), _lib.ptr_array([G.data_ptr()]), None, _lib.ptr_array([out.data_ptr()]),
      _lib.current_stream(DEV))
    seen = [call()]                      # no forward before it
    drv([ids])
    seen.append(call())                  # the last forward gave the column no weights
    with pytest.raises(_lib.InvalidArgumentError):
      drv.backward([G], weight_grads=True)
    drv([ids], sp_weights=[w])
    seen.append(call())                  # legal: after the weighted forward, before the row backward
    drv.backward([G])
    seen.append(call())                  # the row backward has overwritten the received rows
    torch.cuda.current_stream().synchronize()
    codes[r] = seen
    drv.close()

  _threads(world, run)
  bad = _lib.INVALID_ARGUMENT
  assert codes == [[bad, bad, _lib.OK, bad]] * world
  for cm in comms:
    cm.close()


def test_sharded_p2p_bound_plan_is_unimplemented(hbk_option):
  hbk_option('sharded_p2p', 1)
  world = 2
  comms = hb.distribute.Collective.local_world(world)
  codes = [None] * world

  def run(r):
    drv = ShardedGroupLookup([dev(np.zeros((50, 16), F32))], comms[r], buckets=[100])
    out = torch.zeros((8, 16), dtype=torch.float32, device=DEV)
    if not drv.p2p_bind([out]):     # (collective: every rank gets the same answer)
      codes[r] = 'unbound'
      drv.close()
      return
    dw = torch.zeros(8, dtype=torch.float32, device=DEV)
    codes[r] = drv._lib.hbk_sharded_lookup_bwd_weights(
      drv._plan(), _lib.ptr_array([out.data_ptr()]), None, _lib.ptr_array([dw.data_ptr()]),
      _lib.current_stream(DEV))
    drv.p2p_unbind()
    drv.close()

  _threads(world, run)
  for cm in comms:
    cm.close()
  if 'unbound' in codes:
    pytest.skip('peer memory could not be mapped: no p2p form to refuse in')
  assert codes == [_lib.UNIMPLEMENTED] * world


# ---- 6. DenseFeatures ------------------------------------------------------------------------------------
@pytest.mark.parametrize('world', [1, 2])
def test_dense_features_weight_keys(hbk_option, world):
  # every reduce (replicated tables, the sharded tables' owner side) in its reproducible mode, so that the
  # IndexedSlices of the two layers compare bit for bit
  hbk_option('bwd_deterministic', 1)
  rng = np.random.RandomState(71)
  EC = hb.feature_column.EmbeddingColumn
  batch = 256
  # 'a' (200 buckets <= batch) stays replicated at any world size; 'b' and 'p' are sharded at W > 1
  cols = [EC('a', 200, 16, 'mean', weight_feature_key='a_w'),
          EC('b', 5003, 8, 'sqrtn', weight_feature_key='b_w', max_norm=0.5), EC('p', 6007, 8, 'sum')]
  tables = [table_of(rng, c.num_buckets, c.dimension, c.max_norm) for c in cols]
  feats, grads = [], []
  for _ in range(world):
    f = {}
    for key in ('a', 'b'):
      sp = splits_of(rng, 'ragged', batch)
      f[key] = (rng.randint(0, 2**40, size=int(sp[-1])).astype(np.int64), sp)
      f[key + '_w'] = rng.uniform(0.25, 2, size=int(sp[-1])).astype(F32)
    f['p'] = rng.randint(0, 2**40, size=batch).astype(np.int64)
    feats.append(f)
    grads.append(rng.randn(batch, 32).astype(F32))
  comms = hb.distribute.Collective.local_world(world) if world > 1 else [None]
  results = [None] * world

  def run(r):
    def init(col, rows, device):
      t = tables[cols.index(col)]
      return dev(t[r::world].copy() if rows != col.num_buckets else t).to(device)
    f = {k: (tuple(dev(x) for x in v) if isinstance(v, tuple) else dev(v)) for k, v in feats[r].items()}
    runs = []
    for flag in (False, True):
      layer = hb.feature_column.DenseFeatures(cols, DEV, comms[r], batch_size=batch, init=init)
      assert layer.sharded == [False, world > 1, world > 1]
      out = layer(f)
      res = layer.backward(dev(grads[r]), weight_grads=True) if flag else layer.backward(dev(grads[r]))
      torch.cuda.current_stream().synchronize()
      wg = None
      if flag:
        res, wg = res
        wg = {k: host(v) for k, v in wg.items()}
      slices = []
      for u, g, nu in res:
        n = int(nu.item())
        order = np.argsort(host(u)[:n], kind='stable')
        slices.append((host(u)[:n][order], host(g)[:n][order]))
      runs.append((host(out), slices, wg))
      layer.close()
    results[r] = runs

  _threads(world, run)
  for r in range(world):
    (out0, sl0, _), (out1, sl1, wg) = results[r]
    assert sorted(wg) == ['a_w', 'b_w']        # the weight keys only
    np.testing.assert_array_equal(out0.view(np.uint32), out1.view(np.uint32))
    for c in range(3):       # the row backward of every table, replicated or sharded: not a bit differs
      assert sl0[c][0].size > 0
      np.testing.assert_array_equal(sl0[c][0], sl1[c][0])
      np.testing.assert_array_equal(sl0[c][1].view(np.uint32), sl1[c][1].view(np.uint32))
    for c, key in ((0, 'a'), (1, 'b')):
      ids, sp = feats[r][key]
      o = sum(x.dimension for x in cols[:c])
      dw, mag, _ = ref.weight_grad(tables[c], ids, sp, feats[r][key + '_w'], cols[c].combiner,
                                   grads[r][:, o:o + cols[c].dimension], bucket=cols[c].num_buckets,
                                   max_norm=cols[c].max_norm)
      assert_sums_close(wg[key + '_w'], dw, mag, err_msg=f'rank {r} {key}_w')
  for cm in comms:
    if cm is not None:
      cm.close()


# ---- 7. finite difference through the shipped forward ---------------------------------------------------
@pytest.mark.parametrize('comb', COMBS)
def test_finite_difference_of_the_gpu_forward(comb):
  """Perturb one weight by +-h, run the GPU forward, compare the change of sum G * out with dw_j.
  Tolerance: the fp32 forward rounds every element of the perturbed segment within
  (n + 2) * 2^-24 * sum|terms| (n terms, the weight product and the division); the two evaluations err
  independently, other segments give identical bits and cancel: 2 * (n + 2) * 2^-24 * M_s / step with
  M_s = sum_k |G_sk| * sum|terms|_sk, plus the central difference's own truncation (float64 central
  difference of the restatement minus its derivative), plus the bound on dw_j itself."""
  rng = np.random.RandomState(20)
  k = case(rng, comb, 'ragged', 16, 0.5, n_seg=40, rows=211)
  sp, w = k['sp'], k['w']
  lk = GroupLookup([dev(k['table'])], buckets=[k['bucket']], combiners=comb, max_norms=[0.5])
  ids, dsp = dev(k['ids']), dev(sp)
  _, _, wg = run_fused([k])
  dw, mag = want_of(k)
  G64 = k['G'].astype(np.float64)
  h = 2.0 ** -5
  checked = 0
  for s in [s for s in range(sp.size - 1) if sp[s + 1] - sp[s] >= 3][:4]:
    j = int(sp[s]) + 1
    n = int(sp[s + 1] - sp[s])
    L, L64, M, at = [], [], 0.0, []
    for sign in (+1, -1):
      w2 = w.copy()
      w2[j] = F32(w[j] + sign * h)
      at.append(float(w2[j]))     # the fp32 weight both the GPU and the restatement are given
      out = host(lk([ids], [dsp], sp_weights=[dev(w2)])[0]).astype(np.float64)
      o64, m64 = ref.forward(k['table'], k['ids'], sp, w2, comb, bucket=k['bucket'], max_norm=0.5)
      # only segment s differs between the two runs: the others give identical bits and cancel
      L.append(float((G64[s] * out[s]).sum()))
      L64.append(float((G64[s] * o64[s]).sum()))
      M = max(M, float((np.abs(G64[s]) * m64[s]).sum()))
    step = at[0] - at[1]
    fd = (L[0] - L[1]) / step
    trunc = abs((L64[0] - L64[1]) / step - dw[j])
    tol = 2 * (n + 2) * 2.0 ** -24 * M / step + trunc + 1e-5 * mag[j] + 1e-6
    got = float(host(wg[0])[j])
    print(f'{comb} seg {s} id {j}: fd {fd:.7g} dw {got:.7g} f64 {dw[j]:.7g} tol {tol:.3g}')
    assert abs(fd - got) <= tol, (comb, s, fd, got, tol)
    checked += 1
  assert checked >= 3
