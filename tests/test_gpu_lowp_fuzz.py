"""Randomised parity of the low-precision tables -- LowpGroupLookup, LowpLookupGrad and DenseFeatures(table_dtype=) --
against the host restatement only (tests/support/lowp_ref.py; tests/test_lowp_ref.py holds it to torch's CPU casts, an
integer restatement and the float64 reference).  Nothing here is compared with the fp32 kernels or with a cast made on
the GPU.

1. grouped lookup + backward + step, two or three chained steps per draw: the forward bit-equal to
   lowp_ref.forward_rows (the header fixes every operation), the emitted rows as tests/test_gpu_fuzz_features.py
   checks them (bit-equal to the in-order fp32 sums in the deterministic mode, within tolerance.assert_sums_close
   otherwise), every table and slot bit-equal to lowp_ref.apply_step on the call's OWN emitted slices, rows outside
   the batch untouched, Adam's powers and the rounding's step counter advanced once per finished call, a step-only
   call equal to an emitting one;
2. DenseFeatures(table_dtype=) over weighted and ragged columns with each optimizer and rounding, then a save /
   restore round trip;
3. more than 64 columns of mixed types: the per-64-column split of the forward and of the apply in one case.

FTRL is drawn with lr_power = -0.5 only: the powf form is bounded in ulps of fp32 (tests/test_gpu_ftrl.py), and a
result that is a few fp32 ulps off cannot be held bit for bit behind a 16-bit rounding -- near a tie it rounds the
other way.  Its arithmetic is the fp32 entry's functor, which the fp32 fuzz holds to that bound.

noise_row's use of the upper 32 bits of the row number needs a table of more than 2^32 rows: that is
tests/test_gpu_wide_offsets.py (test_lowp_step on geometry R, test_lowp_apply_stochastic_on_rows_past_2_32).

The committed runs are deterministic; HBK_FUZZ_RANDOM=1 HBK_FUZZ_SCALE=10 hunts with fresh draws."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.support import lowp_ref as ref  # noqa: E402
from tests.support import reference  # noqa: E402
from tests.support.tolerance import assert_sums_close  # noqa: E402

hypothesis = pytest.importorskip('hypothesis')
from hypothesis import example, given  # noqa: E402
from hypothesis import strategies as st  # noqa: E402

from tests.test_gpu_fuzz import _cfg  # noqa: E402
from tests.test_gpu_fuzz_features import _batch, _n_seg  # noqa: E402
from tests.test_gpu_lowp_rounding import BF, HF, assert_rows_equal, bits16, bits32_of, dev, host, step_of  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
SEED = 0x9E3779B1
TORCH = {'bf16': BF, 'fp16': HF}
OPTIMIZERS = ('sgd', 'adagrad', 'adam', 'ftrl', 'rowwise_adagrad')
LR = 0.05

lowp_column = st.fixed_dictionaries({
  'dim': st.sampled_from([1, 3, 4, 6, 8, 16, 20, 32, 64, 100, 128, 256]),
  'rows': st.sampled_from([1, 2, 7, 64, 1000]),
  'n_seg': st.one_of(st.just(0), st.integers(1, 300)),
  'ragged': st.booleans(),
  'max_len': st.integers(0, 9),
  'combiner': st.sampled_from(['sum', 'mean', 'sqrtn']),
  'skew': st.sampled_from(['uniform', 'zipf', 'one', 'negative']),
  'bucket0': st.booleans(),
  'weights': st.sampled_from(['none', 'uniform', 'signed', 'zero_segment']),
  'dtype': st.sampled_from(['bf16', 'fp16']),
})
lowp_optimizer = st.fixed_dictionaries({
  'name': st.sampled_from(OPTIMIZERS),
  'emit': st.booleans(),
  'finish': st.booleans(),
  'l1': st.sampled_from([0.0, 0.05, 2.0]),
  'l2': st.sampled_from([0.0, 1e-5, 0.1]),
  'l2_shrinkage': st.sampled_from([0.0, 0.01]),
})
lowp_call = st.fixed_dictionaries({
  'chunk_elems': st.sampled_from([None, 4, 8]),
  'rounding': st.sampled_from(['nearest', 'stochastic']),
  'deterministic': st.booleans(),
  'grad_block': st.booleans(),
})


def table_bits(rng, rows, dim, name):
  return ref.round_nearest(ref.bits32(rng.uniform(-1, 1, size=(rows, dim)).astype(F32)), name)


def initial_slots(name, rows, dim):
  """Host fp32 slots of one table, as the fp32 fuzz starts them."""
  if name == 'adagrad':
    return [np.full((rows, dim), 0.1, F32)]
  if name == 'adam':
    return [np.random.RandomState(7).uniform(-0.1, 0.1, size=(rows, dim)).astype(F32), np.full((rows, dim), 0.01, F32)]
  if name == 'ftrl':
    return [np.full((rows, dim), 0.1, F32), np.random.RandomState(8).uniform(-1, 1, size=(rows, dim)).astype(F32)]
  if name == 'rowwise_adagrad':
    return [np.full((rows, 1), 0.1, F32)]
  return []


def slot_kwargs(name, slots, opt):
  """(keyword arguments of LowpSparseApply / LowpLookupGrad, the restatement's hyperparameters without Adam's powers)."""
  from hybridbackend_amd.embedding import Ftrl, LazyAdam, RowwiseAdagrad
  if name == 'adagrad':
    return dict(accums=[s[0] for s in slots]), {}
  if name == 'adam':
    return dict(moments=[tuple(s) for s in slots], adam=LazyAdam(device=DEV)), {}
  if name == 'ftrl':
    hyper = dict(l1=opt['l1'], l2=opt['l2'], l2_shrinkage=opt['l2_shrinkage'], lr_power=-0.5)
    return dict(ftrl_slots=[tuple(s) for s in slots], ftrl=Ftrl(**hyper)), hyper
  if name == 'rowwise_adagrad':
    return dict(row_accums=[s[0] for s in slots], rowwise_adagrad=RowwiseAdagrad()), dict(epsilon=1e-8)
  return {}, {}


class _State:
  """Tables and slots of one draw on the device, and the objects that look them up and step them."""

  def __init__(self, bits, cols, opt, call, rounding):
    from hybridbackend_amd.embedding import LowpGroupLookup, LowpLookupGrad
    self.name = opt['name']
    self.tables = [dev(b.view(np.int16)).view(TORCH[c['dtype']]) for b, c in zip(bits, cols)]
    self.slots = [[dev(s) for s in initial_slots(self.name, c['rows'], c['dim'])] for c in cols]
    kw, self.hyper = slot_kwargs(self.name, self.slots, opt)
    self.lookup = LowpGroupLookup(self.tables, [c['bucket'] for c in cols], [c['combiner'] for c in cols],
                                  chunk_elems=call['chunk_elems'])
    self.grad = LowpLookupGrad(self.lookup, deterministic=call['deterministic'], rounding=rounding, seed=SEED, **kw)

  def snapshot(self):
    """Host copies: per column (uint16 table, [fp32 slots]); Adam's powers; the step counter."""
    cols = [(bits16(t), [host(s) for s in ss]) for t, ss in zip(self.tables, self.slots)]
    powers = tuple(host(self.grad.adam.beta_powers)) if self.name == 'adam' else None
    return cols, powers, step_of(self.grad)

  def vec4(self, k, grad_rows):
    """The lane layout the apply takes for column k (include/hbk.h): it fixes the order of the row-wise sum."""
    t = self.tables[k]
    bits = (t.data_ptr() * 2) | grad_rows.data_ptr()
    if self.name != 'rowwise_adagrad':
      for s in self.slots[k]:
        bits |= s.data_ptr()
    return t.shape[1] % 4 == 0 and bits % 16 == 0


def assert_state_equal(a, b, what):
  (ca, pa, sa), (cb, pb, sb) = a, b
  for k, ((ta, la), (tb, lb)) in enumerate(zip(ca, cb)):
    np.testing.assert_array_equal(ta, tb, f'{what}: table {k}')
    for j, (x, y) in enumerate(zip(la, lb)):
      np.testing.assert_array_equal(ref.bits32(x), ref.bits32(y), f'{what}: slot {j} of table {k}')
  assert sa == sb, f'{what}: step counter {sa} vs {sb}'
  if pa is not None:
    np.testing.assert_array_equal(np.array(pa, F32), np.array(pb, F32), f'{what}: beta powers')


def _run_lowp(cols, opt, call, steps, id32, seed):
  rng = np.random.RandomState(seed)
  cols = [dict(c, clip='none') for c in cols]
  for c in cols:
    c['bucket'] = 0 if c['bucket0'] else c['rows']
  rounding = call['rounding']
  if rounding == 'stochastic':       # (defined for bf16 only: such a draw has bf16 columns; 'nearest' mixes the types)
    for c in cols:
      c['dtype'] = 'bf16'
  name, det = opt['name'], call['deterministic']
  emit = opt['emit'] or not det      # (a step-only call is compared bit for bit: the deterministic mode)
  finish = opt['finish']
  id_dtype = np.int32 if id32 else np.int64
  bits0 = [table_bits(rng, c['rows'], c['dim'], c['dtype']) for c in cols]
  main = _State(bits0, cols, opt, call, rounding)
  twin = _State(bits0, cols, opt, call, rounding) if not emit else None
  for step in range(steps):
    batch = [_batch(rng, c, id_dtype) for c in cols]
    grads = [rng.randn(_n_seg(b[0], b[1]), c['dim']).astype(F32) for b, c in zip(batch, cols)]
    d_ids = [dev(b[0]) for b in batch]
    d_sp = [None if b[1] is None else dev(b[1]) for b in batch]
    d_w = [None if b[3] is None else dev(b[3]) for b in batch]
    d_g, block = [dev(g) for g in grads], None
    if call['grad_block'] and len({g.shape[0] for g in grads}) == 1:
      # the gradients as column blocks of one wider tensor, every block on a 16-byte boundary of its row
      offsets, at = [], 0
      for c in cols:
        offsets.append(at)
        at += (c['dim'] + 3) // 4 * 4
      wide = torch.zeros(grads[0].shape[0], at + 4, dtype=torch.float32, device=DEV)
      for o, g in zip(offsets, d_g):
        wide[:, o:o + g.shape[1]] = g
      block = (wide, offsets)
    run = twin if twin is not None else main
    before = run.snapshot()
    if twin is not None:
      assert_state_equal(main.snapshot(), before, f'step {step}: main and twin before')
    # forward
    outs = run.lookup(d_ids, d_sp, sp_weights=d_w if any(w is not None for w in d_w) else None)
    torch.cuda.synchronize()
    for k, c in enumerate(cols):
      ids, sp, bucket, w = batch[k]
      want = ref.forward_rows(before[0][k][0], c['dtype'], ids, sp, w, c['combiner'], bucket)
      assert_rows_equal(host(outs[k]), want, False,
                        f'step {step} forward column {k} ({c["dtype"]}, dim {c["dim"]}, {c["combiner"]}, weights '
                        f'{c["weights"]}, ragged {c["ragged"]})')
    # backward and step
    kw = dict(apply_lr=LR, optimizer=name, sp_weights=d_w, finish=finish)
    if block is not None:
      res = run.grad(d_ids, None, d_sp, emit=True, grad_block=block, **kw)
    else:
      res = run.grad(d_ids, d_g, d_sp, emit=True, **kw)
    torch.cuda.synchronize()
    after = run.snapshot()
    hyper = dict(run.hyper)
    if name == 'adam':
      hyper['powers'] = before[1]
    for k, c in enumerate(cols):
      ids, sp, bucket, w = batch[k]
      err = f'step {step} column {k} ({name}, {c["dtype"]}, dim {c["dim"]}, {rounding}, det {det}, weights {c["weights"]})'
      n = int(res[k][2].item())
      u, gp = host(res[k][0])[:n], host(res[k][1])[:n]
      t32 = ref.upcast(before[0][k][0], c['dtype'])
      want_u, want_g, want_m = reference.backward64(t32, ids, sp, w, c['combiner'], grads[k], 0.0, bucket)
      assert np.unique(u).size == n, f'{err}: a row emitted twice'
      np.testing.assert_array_equal(np.sort(u), want_u, err_msg=err)
      assert_sums_close(gp[np.argsort(u)], want_g, want_m, err_msg=err)
      if det:
        np.testing.assert_array_equal(u, want_u, err_msg=f'{err}: rows not ascending')
        terms, r32, v32 = reference.terms32(c['rows'], ids, sp, w, c['combiner'], grads[k], bucket)
        _, seq = reference.seq_row_sums(terms, r32, v32)
        np.testing.assert_array_equal(ref.bits32(gp), ref.bits32(seq), err_msg=f'{err}: not the in-order fp32 sum')
      want_bits, want_slots = ref.apply_step(before[0][k][0], c['dtype'], before[0][k][1], u, gp, name, LR, hyper,
                                             rounding, SEED, before[2], k, run.vec4(k, res[k][1]))
      got_bits, got_slots = after[0][k]
      bad = got_bits != want_bits
      assert not bad.any(), f'{err}: {int(bad.sum())} patterns differ, first at {tuple(np.argwhere(bad)[0])}'
      for j, (x, y) in enumerate(zip(got_slots, want_slots)):
        np.testing.assert_array_equal(ref.bits32(x), ref.bits32(y), err_msg=f'{err}: slot {j}')
      outside = np.setdiff1d(np.arange(c['rows']), u)
      np.testing.assert_array_equal(got_bits[outside], before[0][k][0][outside], err_msg=f'{err}: outside the batch')
    if name == 'adam':
      want_p = reference.adam_finish(before[1]) if finish else before[1]
      np.testing.assert_array_equal(np.array(after[1], F32), np.array(want_p, F32), err_msg=f'step {step}: beta powers')
    want_step = (before[2] + 1) & 0xFFFFFFFF if (finish and rounding == 'stochastic') else before[2]
    assert after[2] == want_step, f'step {step}: step counter {after[2]}, want {want_step}'
    if twin is not None:         # the step-only call on the main state
      if block is not None:
        r = main.grad(d_ids, None, d_sp, emit=False, grad_block=block, **kw)
      else:
        r = main.grad(d_ids, d_g, d_sp, emit=False, **kw)
      torch.cuda.synchronize()
      assert all(t[0] is None and t[1] is None and int(t[2].item()) == int(s[2].item()) for t, s in zip(r, res))
      assert_state_equal(main.snapshot(), after, f'step {step}: step only != emit')


@_cfg(150)
@given(cols=st.lists(lowp_column, min_size=1, max_size=5), opt=lowp_optimizer, call=lowp_call,
       steps=st.integers(2, 3), id32=st.booleans(), seed=st.integers(0, 2**31 - 1))
@example(cols=[dict(dim=16, rows=64, n_seg=300, ragged=True, max_len=6, combiner='mean', skew='uniform',
                    bucket0=False, weights='signed', dtype='bf16'),
               dict(dim=100, rows=7, n_seg=300, ragged=False, max_len=0, combiner='sqrtn', skew='zipf',
                    bucket0=True, weights='zero_segment', dtype='bf16')],
         opt=dict(name='adam', emit=False, finish=True, l1=0.0, l2=0.0, l2_shrinkage=0.0),
         call=dict(chunk_elems=8, rounding='stochastic', deterministic=True, grad_block=True),
         steps=3, id32=False, seed=1)
@example(cols=[dict(dim=3, rows=1000, n_seg=77, ragged=True, max_len=9, combiner='sqrtn', skew='negative',
                    bucket0=False, weights='uniform', dtype='fp16'),
               dict(dim=256, rows=64, n_seg=77, ragged=False, max_len=0, combiner='mean', skew='uniform',
                    bucket0=False, weights='none', dtype='bf16')],
         opt=dict(name='rowwise_adagrad', emit=True, finish=False, l1=0.0, l2=0.0, l2_shrinkage=0.0),
         call=dict(chunk_elems=None, rounding='nearest', deterministic=False, grad_block=False),
         steps=2, id32=True, seed=2)
@example(cols=[dict(dim=20, rows=2, n_seg=150, ragged=True, max_len=4, combiner='sum', skew='one',
                    bucket0=True, weights='signed', dtype='fp16')],
         opt=dict(name='ftrl', emit=True, finish=True, l1=0.05, l2=1e-5, l2_shrinkage=0.01),
         call=dict(chunk_elems=4, rounding='nearest', deterministic=True, grad_block=False),
         steps=3, id32=False, seed=3)
def test_lowp_grouped_random(cols, opt, call, steps, id32, seed):
  _run_lowp(cols, opt, call, steps, id32, seed)


# ---- more than 64 columns ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('optimizer', ['adagrad', 'adam'])
def test_lowp_many_columns_mixed_types(optimizer):
  """67 columns, bf16 and fp16 alternating, rounded to nearest: the second launch of the forward (per kind and lane
  width) and of the apply in one case; dims 1 .. 256, empty columns among them."""
  dims = [1, 3, 4, 16, 20, 64, 128, 256, 8, 100]
  rng = np.random.RandomState(67)
  cols = []
  for k in range(67):
    cols.append(dict(dim=dims[k % len(dims)], rows=int(rng.choice([7, 64, 300])),
                     n_seg=0 if k % 9 == 4 else int(rng.randint(1, 60)), ragged=bool(k % 2), max_len=4,
                     combiner=('sum', 'mean', 'sqrtn')[k % 3], skew='uniform', bucket0=k % 5 == 0,
                     weights=('none', 'uniform', 'signed')[k % 3], dtype=('bf16', 'fp16')[k % 2]))
  opt = dict(name=optimizer, emit=True, finish=True, l1=0.05, l2=1e-5, l2_shrinkage=0.01)
  call = dict(chunk_elems=None, rounding='nearest', deterministic=True, grad_block=False)
  _run_lowp(cols, opt, call, 2, False, 67)


# ---- the layer -----------------------------------------------------------------------------------------------------------
layer_column = st.fixed_dictionaries({
  'dim': st.sampled_from([1, 3, 4, 8, 16, 20, 64, 128]),
  'rows': st.sampled_from([2, 7, 64, 1000]),
  'ragged': st.booleans(),
  'max_len': st.integers(0, 6),
  'combiner': st.sampled_from(['sum', 'mean', 'sqrtn']),
  'weighted': st.booleans(),
})


def _run_layer(cols, optimizer, rounding, dtype_name, batch, seed, tmp):
  import hybridbackend_amd as hb
  fc = hb.feature_column
  rng = np.random.RandomState(seed)
  cols = sorted(cols, key=lambda c: c['dim'] <= 64)     # (wide columns first: their blocks stay on 16-byte boundaries)
  dtype = TORCH[dtype_name]

  def columns():
    return [fc.EmbeddingColumn(f'c{k}', c['rows'], c['dim'], combiner=c['combiner'],
                               weight_feature_key=f'w{k}' if c['weighted'] else None) for k, c in enumerate(cols)]

  def init(col, rows, device):
    rs = np.random.RandomState(rows + col.dimension)
    return torch.from_numpy(rs.uniform(-1, 1, size=(rows, col.dimension)).astype(F32)).to(device)

  def build(init_):
    kw = dict(initial_accumulator_value=0.1) if optimizer == 'adagrad' else \
        dict(optimizer=optimizer) if optimizer != 'sgd' else {}
    if optimizer == 'rowwise_adagrad':
      kw['rowwise_adagrad'] = hb.embedding.RowwiseAdagrad(initial_accumulator_value=0.1)
    return fc.DenseFeatures(columns(), DEV, init=init_, table_dtype=dtype, table_rounding=rounding, table_seed=SEED,
                            **kw)

  def slots_of(layer, k):
    if optimizer == 'adagrad':
      return [layer.accums[k]]
    if optimizer == 'adam':
      return list(layer.moments[k])
    if optimizer == 'ftrl':
      return list(layer.ftrl_slots[k])
    if optimizer == 'rowwise_adagrad':
      return [layer.row_accums[k]]
    return []

  layer = build(init)
  hyper0 = {'ftrl': dict(l1=0.0, l2=0.0, l2_shrinkage=0.0, lr_power=-0.5), 'rowwise_adagrad': dict(epsilon=1e-8)
            }.get(optimizer, {})
  for k, c in enumerate(cols):     # the cast of init is to nearest
    want = ref.round_nearest(ref.bits32(host(init(layer.columns[k], c['rows'], 'cpu'))), dtype_name)
    np.testing.assert_array_equal(bits16(layer.weights[k]), want, f'initial table {k}')
  for step in range(3):
    feats, hostf = {}, []
    for k, c in enumerate(cols):
      if c['ragged']:
        lens = rng.randint(0, c['max_len'] + 1, size=batch)
        sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        n = int(sp[-1])
      else:
        sp, n = None, batch
      ids = rng.randint(-3 * c['rows'], 3 * c['rows'], size=n).astype(np.int64)
      w = rng.uniform(-1, 2, size=n).astype(F32) if c['weighted'] else None
      feats[f'c{k}'] = dev(ids) if sp is None else (dev(ids), dev(sp))
      if w is not None:
        feats[f'w{k}'] = dev(w)
      hostf.append((ids, sp, w))
    before = [(bits16(layer.weights[k]), [host(s) for s in slots_of(layer, k)]) for k in range(len(cols))]
    powers = tuple(host(layer.adam.beta_powers)) if optimizer == 'adam' else None
    counter = step_of(layer._grad)
    out = host(layer(feats))
    torch.cuda.synchronize()
    for k, c in enumerate(cols):
      ids, sp, w = hostf[k]
      want = ref.forward_rows(before[k][0], dtype_name, ids, sp, w, c['combiner'], c['rows'])
      assert_rows_equal(np.ascontiguousarray(out[:, layer.offsets[k]:layer.offsets[k] + c['dim']]), want, False,
                        f'step {step} forward column {k}')
    grad = rng.randn(batch, layer.width).astype(F32)
    res = layer.backward(dev(grad), apply_lr=LR, optimizer=optimizer)
    torch.cuda.synchronize()
    hyper = dict(hyper0)
    if optimizer == 'adam':
      hyper['powers'] = powers
    for k, c in enumerate(cols):
      n = int(res[k][2].item())
      u, gp = host(res[k][0])[:n], host(res[k][1])[:n]
      ids, sp, w = hostf[k]
      err = f'step {step} column {k} ({optimizer}, {dtype_name}, {rounding}, dim {c["dim"]})'
      g = grad[:, layer.offsets[k]:layer.offsets[k] + c['dim']]
      want_u, want_g, want_m = reference.backward64(ref.upcast(before[k][0], dtype_name), ids, sp, w, c['combiner'], g,
                                                    0.0, c['rows'])
      np.testing.assert_array_equal(np.sort(u), want_u, err_msg=err)
      assert_sums_close(gp[np.argsort(u)], want_g, want_m, err_msg=err)
      t = layer.weights[k]
      align = (t.data_ptr() * 2) | res[k][1].data_ptr()
      if optimizer != 'rowwise_adagrad':
        for s in slots_of(layer, k):
          align |= s.data_ptr()
      want_bits, want_slots = ref.apply_step(before[k][0], dtype_name, before[k][1], u, gp, optimizer, LR, hyper,
                                             rounding, SEED, counter, k, c['dim'] % 4 == 0 and align % 16 == 0)
      np.testing.assert_array_equal(bits16(t), want_bits, err_msg=err)
      for j, (s, y) in enumerate(zip(slots_of(layer, k), want_slots)):
        np.testing.assert_array_equal(bits32_of(s), ref.bits32(y), err_msg=f'{err}: slot {j}')
    assert step_of(layer._grad) == (counter + 1 if rounding == 'stochastic' else counter)
    if optimizer == 'adam':
      np.testing.assert_array_equal(host(layer.adam.beta_powers), np.array(reference.adam_finish(powers), F32))
  # save / restore: bits and dtype of tables and slots, Adam's powers
  prefix = os.path.join(tmp, 'ckpt')
  layer.save(prefix)
  other = build(lambda col, rows, device: torch.zeros(rows, col.dimension, device=device))
  other.restore(prefix)
  torch.cuda.synchronize()
  for k in range(len(cols)):
    assert other.weights[k].dtype == dtype
    np.testing.assert_array_equal(bits16(other.weights[k]), bits16(layer.weights[k]), f'restored table {k}')
    a, b = slots_of(layer, k), slots_of(other, k)
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
      assert y.dtype == torch.float32
      np.testing.assert_array_equal(bits32_of(y), bits32_of(x), f'restored slot {j} of table {k}')
  if optimizer == 'adam':
    np.testing.assert_array_equal(bits32_of(other.adam.beta_powers), bits32_of(layer.adam.beta_powers))


@_cfg(40)
@given(cols=st.lists(layer_column, min_size=1, max_size=4), optimizer=st.sampled_from(OPTIMIZERS),
       rounding=st.sampled_from(['nearest', 'stochastic']), dtype=st.sampled_from(['bf16', 'fp16']),
       batch=st.sampled_from([1, 64, 257]), seed=st.integers(0, 2**31 - 1))
@example(cols=[dict(dim=128, rows=64, ragged=False, max_len=0, combiner='mean', weighted=True),
               dict(dim=3, rows=1000, ragged=True, max_len=6, combiner='sqrtn', weighted=True),
               dict(dim=20, rows=7, ragged=True, max_len=3, combiner='sum', weighted=False)],
         optimizer='ftrl', rounding='stochastic', dtype='bf16', batch=64, seed=4)
@example(cols=[dict(dim=16, rows=2, ragged=False, max_len=0, combiner='sum', weighted=False),
               dict(dim=64, rows=64, ragged=True, max_len=5, combiner='mean', weighted=True)],
         optimizer='adam', rounding='nearest', dtype='fp16', batch=257, seed=5)
def test_lowp_layer_random(tmp_path_factory, cols, optimizer, rounding, dtype, batch, seed):
  if dtype == 'fp16':
    rounding = 'nearest'
  _run_layer(cols, optimizer, rounding, dtype, batch, seed, str(tmp_path_factory.mktemp('lowp')))
