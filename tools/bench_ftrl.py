"""FTRL-Proximal against SGD, Adagrad and Lazy Adam after the config-2 backward, in one process,
alternating:

  emit_{sgd,adagrad,adam,ftrl,ftrl_pow}   26 columns x 1M x 16, batch 65536, uniform ids, sum:
                            IndexedSlices + step; ftrl: lr_power = -0.5 (sqrtf form), ftrl_pow:
                            lr_power = -0.3 (powf form)
  step_{sgd,adagrad,adam,ftrl,ftrl_pow}   the same, step only (no IndexedSlices written)
  ftrl_separate / ftrl_interleaved   FTRL step only, w / accum / linear as three tensors against one
                            [rows, 64] tensor per column holding [w | accum | linear | pad]
                            (table_pitch 64, at the C ABI: hbk_group_lookup_bwd_ftrl)
  ragged_{sgd,ftrl}         26 columns x 65536 segments of Poisson(8) ids clipped to [0, 32], mean,
                            IndexedSlices + step

Timing follows tools/bench_weighted.py: resident id batches (a step reads another one), warm-up steps,
then `--steps` launches between HIP events; the forms of a group take turns for `--rounds` rounds and
the median per-step time of each is reported (with min / max).  Also reports the distinct rows of a
config-2 step (n_unique summed over the columns) and the request floor of the apply kernel: 3 random
loads + 3 random stores per row (separate slots) at 49 G requests/s.  Prints one JSON
line.

  python tools/bench_ftrl.py [--steps 20 --warmup 5 --rounds 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

REQ_PER_S = 49e9   # random requests per second


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--steps', type=int, default=20)
  p.add_argument('--warmup', type=int, default=5)
  p.add_argument('--rounds', type=int, default=5)
  p.add_argument('--batches', type=int, default=4)
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  dev = torch.device('cuda:0')
  cols, rows, dim, batch = 26, 1_000_000, 16, 65536
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)

  def table():
    return torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen)
  tables = [table() for _ in range(cols)]
  accums = [torch.full((rows, dim), 0.1, device=dev) for _ in range(cols)]
  moments = [(torch.zeros(rows, dim, device=dev), torch.zeros(rows, dim, device=dev)) for _ in range(cols)]
  ftrl = hb.embedding.Ftrl()
  ftrl_pow = hb.embedding.Ftrl(lr_power=-0.3)
  slots = [ftrl.slots_like(t) for t in tables]
  flat = [[torch.randint(0, 1 << 40, (batch,), device=dev, dtype=torch.int64, generator=gen)
           for _ in range(cols)] for _ in range(args.batches)]
  rng = np.random.RandomState(4242)
  splits = []
  for _ in range(cols):
    sp = np.concatenate([[0], np.cumsum(rng.poisson(8, size=batch).clip(0, 32))]).astype(np.int32)
    splits.append(torch.from_numpy(sp).to(dev))
  ragged = [[torch.randint(0, 1 << 40, (int(splits[c][-1]),), device=dev, dtype=torch.int64,
                           generator=gen) for c in range(cols)] for _ in range(args.batches)]
  grads = [torch.randn(batch, dim, device=dev, generator=gen) for _ in range(cols)]
  adam = hb.embedding.LazyAdam(device=dev)
  lib = _lib.lib()

  def bwd_case(optimizer, pool, sp, combiner, emit, lr=1e-4, params=ftrl):
    lookup = hb.embedding.GroupLookup(tables, buckets=[rows] * cols, combiners=combiner)
    objs = []
    for b in range(args.batches):
      g = hb.embedding.GroupLookupGrad(
        lookup, accums=accums if optimizer == 'adagrad' else None,
        moments=moments if optimizer == 'adam' else None, adam=adam,
        ftrl_slots=slots if optimizer == 'ftrl' else None, ftrl=params,
        workspace_of=objs[0] if objs else None)
      g(pool[b], grads, sp, apply_lr=lr, optimizer=optimizer, emit=emit)
      objs.append(g)
    return lambda i: objs[i % len(objs)].launch(apply_lr=lr, optimizer=optimizer)

  def interleaved_case(lr=1e-4):
    # [w | accum | linear | pad] per row, pitch 64 floats: a row is two whole 128-byte lines
    bufs = [torch.zeros(rows, 4 * dim, device=dev) for _ in range(cols)]
    for c in range(cols):
      bufs[c][:, :dim].copy_(tables[c])
      bufs[c][:, dim:2 * dim].fill_(ftrl.initial_accumulator_value)
    a_ptrs = _lib.ptr_array([b.data_ptr() + 4 * dim for b in bufs])
    z_ptrs = _lib.ptr_array([b.data_ptr() + 8 * dim for b in bufs])
    lookup = hb.embedding.GroupLookup(tables, buckets=[rows] * cols, combiners='sum')
    nu = torch.zeros(cols, dtype=torch.int32, device=dev)
    calls = []
    for b in range(args.batches):
      g = hb.embedding.GroupLookupGrad(lookup, ftrl_slots=slots, ftrl=ftrl)
      g(flat[b], grads, apply_lr=lr, optimizer='ftrl', emit=False)
      cd = type(g._cols).from_buffer_copy(g._cols)
      for c in range(cols):
        cd[c].table, cd[c].table_pitch = bufs[c].data_ptr(), 4 * dim
        cd[c].unique_rows = cd[c].grad_rows = None
        cd[c].n_unique = nu.data_ptr() + 4 * c
      need = lib.hbk_group_lookup_bwd_ftrl_workspace_bytes(cols, cd)
      ws = torch.empty(need, dtype=torch.uint8, device=dev)
      calls.append((cd, ws, g))
    params = ftrl.params()

    def step(i):
      cd, ws, _ = calls[i % len(calls)]
      _lib.check(lib.hbk_group_lookup_bwd_ftrl(
        cols, cd, a_ptrs, z_ptrs, C.byref(params), C.c_float(lr), C.c_void_p(ws.data_ptr()),
        C.c_size_t(ws.numel()), _lib.current_stream(dev)))
    step.keep = (bufs, calls)
    return step

  groups = [
    {'emit_sgd': lambda: bwd_case('sgd', flat, None, 'sum', True),
     'emit_adagrad': lambda: bwd_case('adagrad', flat, None, 'sum', True),
     'emit_adam': lambda: bwd_case('adam', flat, None, 'sum', True),
     'emit_ftrl': lambda: bwd_case('ftrl', flat, None, 'sum', True),
     'emit_ftrl_pow': lambda: bwd_case('ftrl', flat, None, 'sum', True, params=ftrl_pow)},
    {'step_sgd': lambda: bwd_case('sgd', flat, None, 'sum', False),
     'step_adagrad': lambda: bwd_case('adagrad', flat, None, 'sum', False),
     'step_adam': lambda: bwd_case('adam', flat, None, 'sum', False),
     'step_ftrl': lambda: bwd_case('ftrl', flat, None, 'sum', False),
     'step_ftrl_pow': lambda: bwd_case('ftrl', flat, None, 'sum', False, params=ftrl_pow)},
    {'ftrl_separate': lambda: bwd_case('ftrl', flat, None, 'sum', False),
     'ftrl_interleaved': interleaved_case},
    {'ragged_sgd': lambda: bwd_case('sgd', ragged, splits, 'mean', True),
     'ragged_ftrl': lambda: bwd_case('ftrl', ragged, splits, 'mean', True)},
  ]

  def timed(step):
    for i in range(args.warmup):
      step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(args.steps):
      step(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps   # us per step

  result = {}
  for group in groups:
    steps = {name: make() for name, make in group.items()}
    t = {name: [] for name in group}
    for _ in range(args.rounds):
      for name in group:   # alternating
        t[name].append(timed(steps[name]))
    for name in group:
      result[name] = {'us': round(float(np.median(t[name])), 2),
                      'min_max_us': [round(min(t[name]), 2), round(max(t[name]), 2)]}
    del steps
    torch.cuda.synchronize()
  # distinct rows of one config-2 step, and the apply kernel's request floor
  g = hb.embedding.GroupLookupGrad(hb.embedding.GroupLookup(tables, buckets=[rows] * cols))
  res = g(flat[0], grads)
  n_unique = int(sum(int(r[2].item()) for r in res))
  g = hb.embedding.GroupLookupGrad(hb.embedding.GroupLookup(tables, buckets=[rows] * cols,
                                                            combiners='mean'))
  res = g(ragged[0], grads, splits)
  n_unique_ragged = int(sum(int(r[2].item()) for r in res))
  result['n_unique'] = {'config2': n_unique, 'ragged': n_unique_ragged}
  result['apply_floor_us'] = {'separate': round(6 * n_unique / REQ_PER_S * 1e6, 2),
                              'ragged': round(6 * n_unique_ragged / REQ_PER_S * 1e6, 2)}
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  print(json.dumps(result))


if __name__ == '__main__':
  main()
