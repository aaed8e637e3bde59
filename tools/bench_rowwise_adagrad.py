"""Row-wise Adagrad against SGD, fused Adagrad and Lazy Adam after the grouped backward, in one process, the
forms taking turns:

  c2     config 2's shape: 26 columns x 1M x 16, batch 65536, uniform ids, sum
  d128   the same with dim 128 (8 columns: the four optimizers' state for 26 would not be measured any better)
  ragged 26 columns x 1M x 16, 65536 segments of Poisson(8) ids clipped to [0, 32], mean

  <case>_emit_none                  the emit-form reduce alone (apply_lr = 0): phase 1 of every slot optimizer
  <case>_{emit,step}_{sgd,adagrad,rowwise,adam}   IndexedSlices + step, and step only

Timing follows tools/bench_adam.py: resident id batches (a step reads another one), warm-up steps, then
`--steps` launches between HIP events; the forms of a case take turns for `--rounds` rounds (default 7) and the
median per-step time of each is reported with min / max.  The apply launch of a slot optimizer is not timed on
its own: `apply_us` is its emit form's median minus `emit_none`'s of the same case, and `apply_tb_s` that time
against the byte model per distinct row -- 8 B row number, 4 dim gradient, 2 * 4 dim weights, and 8 B
accumulator (row-wise) or 2 * 2 * 4 dim moments (Lazy Adam).  Also reports the optimizer state per row.  Prints
one JSON line.

  python tools/bench_rowwise_adagrad.py [--steps 20 --warmup 5 --rounds 7]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--steps', type=int, default=20)
  p.add_argument('--warmup', type=int, default=5)
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--batches', type=int, default=4)
  p.add_argument('--cases', default='c2,d128,ragged')
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  dev = torch.device('cuda:0')
  rows, batch = 1_000_000, 65536
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)
  rng = np.random.RandomState(4242)

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

  def run_case(name, cols, dim, is_ragged):
    tables = [torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen) for _ in range(cols)]
    accums = [torch.full((rows, dim), 0.1, device=dev) for _ in range(cols)]
    moments = [(torch.zeros(rows, dim, device=dev), torch.zeros(rows, dim, device=dev)) for _ in range(cols)]
    rowwise = hb.embedding.RowwiseAdagrad(initial_accumulator_value=0.1)
    row_accums = [rowwise.slots_like(t) for t in tables]
    adam = hb.embedding.LazyAdam(device=dev)
    splits, combiner = None, 'sum'
    if is_ragged:
      combiner = 'mean'
      splits = [torch.from_numpy(np.concatenate([[0], np.cumsum(rng.poisson(8, size=batch).clip(0, 32))])
                                 .astype(np.int32)).to(dev) for _ in range(cols)]
    n_ids = [batch if splits is None else int(s[-1]) for s in (splits or [None] * cols)]
    pool = [[torch.randint(0, 1 << 40, (n_ids[c],), device=dev, dtype=torch.int64, generator=gen)
             for c in range(cols)] for _ in range(args.batches)]
    grads = [torch.randn(batch, dim, device=dev, generator=gen) for _ in range(cols)]
    lookup = hb.embedding.GroupLookup(tables, buckets=[rows] * cols, combiners=combiner)
    kw = {'sgd': {}, 'adagrad': dict(accums=accums), 'adam': dict(moments=moments, adam=adam),
          'rowwise_adagrad': dict(row_accums=row_accums, rowwise_adagrad=rowwise)}

    def form(optimizer, emit, lr=1e-4):
      objs = []
      for b in range(args.batches):
        g = hb.embedding.GroupLookupGrad(lookup, workspace_of=objs[0] if objs else None, **kw[optimizer])
        g(pool[b], grads, splits, apply_lr=lr, optimizer=optimizer, emit=emit)
        objs.append(g)
      return lambda i: objs[i % len(objs)].launch(apply_lr=lr, optimizer=optimizer)

    short = {'sgd': 'sgd', 'adagrad': 'adagrad', 'rowwise_adagrad': 'rowwise', 'adam': 'adam'}
    out = {}
    for mode, emit in (('emit', True), ('step', False)):
      forms = {f'{mode}_{short[o]}': form(o, emit) for o in short}
      if emit:
        forms['emit_none'] = form('sgd', True, lr=0.0)
      t = {k: [] for k in forms}
      for _ in range(args.rounds):
        for k in forms:   # taking turns
          t[k].append(timed(forms[k]))
      for k in forms:
        out[k] = {'us': round(float(np.median(t[k])), 2), 'min_max_us': [round(min(t[k]), 2), round(max(t[k]), 2)]}
      del forms
      torch.cuda.synchronize()
    res = hb.embedding.GroupLookupGrad(lookup)(pool[0], grads, splits)
    n_unique = int(sum(int(r[2].item()) for r in res))
    out['n_unique'] = n_unique
    model = {'rowwise': 8 + 4 * dim + 2 * 4 * dim + 8, 'adam': 8 + 4 * dim + 3 * 2 * 4 * dim}
    for k, per_row in model.items():
      us = out[f'emit_{k}']['us'] - out['emit_none']['us']
      out[f'apply_{k}'] = {'us': round(us, 2), 'bytes_per_row': per_row,
                           'tb_s': round(n_unique * per_row / (us * 1e-6) / 1e12, 3) if us > 0 else None}
    out['state_bytes_per_row'] = {'adagrad': 4 * dim, 'rowwise': 4, 'adam': 8 * dim}
    return {f'{name}_{k}': v for k, v in out.items()}

  cases = {'c2': (26, 16, False), 'd128': (8, 128, False), 'ragged': (26, 16, True)}
  result = {}
  for name in args.cases.split(','):
    result.update(run_case(name, *cases[name]))
    torch.cuda.empty_cache()
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  print(json.dumps(result))


if __name__ == '__main__':
  main()
