"""The one sparse-apply walk under its two table policies: SparseApply (fp32 rows) and LowpSparseApply (bf16 / fp16
rows) driven through the SAME task-boundary cases and compared bit for bit with their numpy restatements
(tests/support/replica_grads_ref.py:apply_slices and tests/support/lowp_ref.py:apply_step).

One call steps three columns whose rows take 1, 8 and 16 lanes (dim 1, 20 and 64: 256, 32 and 16 rows per wave
task), so a workgroup's walk crosses column boundaries; the capacity of 37 leaves the last task of every column
partial; unique_rows holds the three kinds of hole; n_unique takes 0, 1, the capacity, a value above it (clamped on
the device) and a negative one."""
import numpy as np
import pytest
import torch

from hybridbackend_amd.embedding import Ftrl, LazyAdam, LowpSparseApply, RowwiseAdagrad, SparseApply
from tests.support import lowp_ref
from tests.support import replica_grads_ref

DEV = 'cuda:0'
F32 = np.float32
ROWS, CAP = 50, 37
DIMS = (1, 20, 64)
# position in unique_rows -> what stands there (the last one lies in every column's partial task)
HOLES = {3: -1, 17: ROWS, CAP - 1: ROWS + 7}
N_UNIQUE = (0, 1, CAP, 42, -3)
LR = 0.05
OPTIMIZERS = ('sgd', 'adagrad', 'adam', 'ftrl', 'rowwise_adagrad')
FTRL = dict(l1=0.01, l2=0.02, l2_shrinkage=0.03, lr_power=-0.5)
EPSILON = 1e-8                                    # row-wise Adagrad's
SLOTS = {'sgd': (), 'adagrad': ('a',), 'adam': ('m', 'v'), 'ftrl': ('a', 'z'), 'rowwise_adagrad': ('a',)}
TORCH = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}


def make_columns(kind, optimizer):
  """Per column the host state dict(w=fp32 values or uint16 patterns, and the rule's fp32 slots) and its slices
  (unique_rows with the holes, grad_rows finite everywhere: what n_unique leaves out must stay as it was)."""
  rng = np.random.RandomState(7)
  states, slices = [], []
  for dim in DIMS:
    w = rng.uniform(-2, 2, size=(ROWS, dim)).astype(F32)
    st = dict(w=w if kind == 'fp32' else lowp_ref.round_nearest(lowp_ref.bits32(w), kind))
    for name in SLOTS[optimizer]:
      shape = (ROWS, 1) if optimizer == 'rowwise_adagrad' else (ROWS, dim)
      lo, hi = (-0.1, 0.1) if name in ('m', 'z') else (0.1, 0.9)
      st[name] = rng.uniform(lo, hi, size=shape).astype(F32)
    urows = rng.permutation(ROWS)[:CAP].astype(np.int64)
    for at, hole in HOLES.items():
      urows[at] = hole
    states.append(st)
    slices.append((urows, rng.randn(CAP, dim).astype(F32)))
  return states, slices


def restate(kind, optimizer, st, urows, g, n_unique, powers, col):
  """One step of one column on the host, in place in `st`."""
  if kind == 'fp32':
    hyper = {'ftrl': FTRL, 'rowwise_adagrad': dict(eps=EPSILON)}.get(optimizer)
    replica_grads_ref.apply_slices(optimizer, st, urows, g, LR, n_unique=n_unique, powers=powers, hyper=hyper)
    return
  n = min(max(n_unique, 0), urows.size)
  hyper = {'adam': dict(powers=powers), 'ftrl': FTRL, 'rowwise_adagrad': dict(epsilon=EPSILON)}.get(optimizer)
  names = SLOTS[optimizer]
  st['w'], slots = lowp_ref.apply_step(st['w'], kind, [st[k] for k in names], urows[:n], g[:n], optimizer, LR, hyper,
                                       col=col)
  st.update(zip(names, slots))


def untouched_rows(urows, n_unique):
  n = min(max(n_unique, 0), urows.size)
  live = urows[:n]
  return np.setdiff1d(np.arange(ROWS), live[(live >= 0) & (live < ROWS)])


@pytest.mark.parametrize('optimizer', OPTIMIZERS)
@pytest.mark.parametrize('kind', ['fp32', 'bf16', 'fp16'])
def test_both_restatements_run_these_shapes(kind, optimizer):
  """No GPU: the restatements step exactly the live rows of every n_unique and leave the holes' neighbours, the
  rows past n_unique and every slot row of theirs alone."""
  states, slices = make_columns(kind, optimizer)
  powers = (F32(0.9), F32(0.999))
  for n_unique in N_UNIQUE:
    for c, (st, (urows, g)) in enumerate(zip(states, slices)):
      before = {k: v.copy() for k, v in st.items()}
      restate(kind, optimizer, st, urows, g, n_unique, powers, c)
      same = untouched_rows(urows, n_unique)
      assert same.size == ROWS - {0: 0, 1: 1, CAP: CAP - len(HOLES), 42: CAP - len(HOLES), -3: 0}[n_unique]
      for k in st:
        np.testing.assert_array_equal(st[k][same].view(np.uint8), before[k][same].view(np.uint8),
                                      f'{k} of column {c}')
        assert st[k].shape == before[k].shape and st[k].dtype == before[k].dtype
      if same.size < ROWS:
        stepped = np.setdiff1d(np.arange(ROWS), same)
        assert not np.array_equal(st['w'][stepped], before['w'][stepped])


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits_of(t):
  """The patterns of a device tensor of 2- or 4-byte elements."""
  t = t.contiguous()
  return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('optimizer', OPTIMIZERS)
@pytest.mark.parametrize('kind', ['fp32', 'bf16', 'fp16'])
def test_walk_crosses_columns_partial_tasks_holes_and_every_n_unique(kind, optimizer):
  states, slices = make_columns(kind, optimizer)
  if kind == 'fp32':
    tables = [dev(st['w']) for st in states]
  else:
    tables = [dev(st['w'].view(np.int16)).view(TORCH[kind]) for st in states]
  slots = [[dev(st[k]) for k in SLOTS[optimizer]] for st in states]
  kw = {}
  if optimizer == 'adagrad':
    kw = dict(accums=[s[0] for s in slots])
  elif optimizer == 'adam':
    kw = dict(moments=[tuple(s) for s in slots], adam=LazyAdam(device=DEV))
  elif optimizer == 'ftrl':
    kw = dict(ftrl_slots=[tuple(s) for s in slots], ftrl=Ftrl(**FTRL))
  elif optimizer == 'rowwise_adagrad':
    kw = dict(row_accums=[s[0] for s in slots], rowwise_adagrad=RowwiseAdagrad(epsilon=EPSILON))
  app = (SparseApply if kind == 'fp32' else LowpSparseApply)(tables, **kw)
  nu = [torch.zeros(1, dtype=torch.int32, device=DEV) for _ in DIMS]
  device_slices = [(dev(u), dev(g), n) for (u, g), n in zip(slices, nu)]
  for n_unique in N_UNIQUE:
    for n in nu:
      n.fill_(n_unique)
    powers = tuple(app.adam.beta_powers.cpu().numpy()) if optimizer == 'adam' else None   # (of THIS step)
    app(device_slices, LR, optimizer)
    torch.cuda.synchronize()
    for c, (st, (urows, g)) in enumerate(zip(states, slices)):
      restate(kind, optimizer, st, urows, g, n_unique, powers, c)
      what = f'{kind} {optimizer} n_unique {n_unique} column {c} (dim {DIMS[c]})'
      for name, t in zip(('w',) + SLOTS[optimizer], [tables[c]] + slots[c]):
        want = st[name].view(np.int16 if st[name].itemsize == 2 else np.int32)
        bad = bits_of(t) != want
        assert not bad.any(), (f'{what}: {name}: {int(bad.sum())} of {bad.size} patterns differ, first at '
                               f'{tuple(np.argwhere(bad)[0])}')
