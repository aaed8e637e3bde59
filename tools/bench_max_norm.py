"""max_norm against the unclipped paths on the config-2 shape, in one process, alternating:

  fwd_plain / fwd_clip            26 columns x 1M x 16, batch 65536, uniform ids, sum: the forward with
                                  no column / every column clipped
  emit_plain / emit_clip          the backward's IndexedSlices, unclipped / clipped (emit form + clip pass)
  sgd_plain / sgd_clip            the same + SGD (plain: the step fused into the reduce)
  adagrad_plain / adagrad_clip    the same + Adagrad
  adam_plain / adam_clip          the same + Lazy Adam

max_norm is the median row norm of the tables at the start (about half of the looked-up rows are
clipped then; the stepping cases move the shared tables, so later groups clip more rows).  Timing
follows tools/bench_adam.py: resident id batches (a step reads another one), warm-up steps, then
`--steps` launches between HIP events; the two forms of a group take turns for `--rounds` rounds and the
median per-step time of each is reported (with min / max).  Prints one JSON line.

  python tools/bench_max_norm.py [--steps 20 --warmup 5 --rounds 5]
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
  p.add_argument('--rounds', type=int, default=5)
  p.add_argument('--batches', type=int, default=4)
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  dev = torch.device('cuda:0')
  cols, rows, dim, batch = 26, 1_000_000, 16, 65536
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)
  tables = [torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen) for _ in range(cols)]
  accums = [torch.full((rows, dim), 0.1, device=dev) for _ in range(cols)]
  moments = [(torch.zeros(rows, dim, device=dev), torch.zeros(rows, dim, device=dev)) for _ in range(cols)]
  flat = [[torch.randint(0, 1 << 40, (batch,), device=dev, dtype=torch.int64, generator=gen)
           for _ in range(cols)] for _ in range(args.batches)]
  grads = [torch.randn(batch, dim, device=dev, generator=gen) for _ in range(cols)]
  c = float(tables[0][:65536].norm(dim=1).median().item())

  def clipped_share():
    looked_up = torch.cat([tables[k][flat[0][k] % rows] for k in range(cols)])
    return round(float((looked_up.norm(dim=1) > c).float().mean().item()), 3)
  result = {'max_norm': c, 'clipped_share_at_start': clipped_share()}
  adam = hb.embedding.LazyAdam(device=dev)

  def fwd_case(max_norms):
    lookup = hb.embedding.GroupLookup(tables, buckets=[rows] * cols, combiners='sum', max_norms=max_norms)
    outs = [torch.empty(batch, dim, device=dev) for _ in range(cols)]
    lookup(flat[0], outs=outs)

    def step(i):
      lookup(flat[i % len(flat)], outs=outs)
    step.keep = (lookup, outs)
    return step

  def bwd_case(optimizer, max_norms, lr):
    lookup = hb.embedding.GroupLookup(tables, buckets=[rows] * cols, combiners='sum', max_norms=max_norms)
    objs = []
    for b in range(args.batches):
      g = hb.embedding.GroupLookupGrad(
        lookup, accums=accums if optimizer == 'adagrad' else None,
        moments=moments if optimizer == 'adam' else None, adam=adam,
        workspace_of=objs[0] if objs else None)
      g(flat[b], grads, apply_lr=lr, optimizer=optimizer)
      objs.append(g)
    return lambda i: objs[i % len(objs)].launch(apply_lr=lr, optimizer=optimizer)

  groups = [
    {'fwd_plain': lambda: fwd_case(None), 'fwd_clip': lambda: fwd_case(c)},
    {'emit_plain': lambda: bwd_case('sgd', None, 0.0), 'emit_clip': lambda: bwd_case('sgd', c, 0.0)},
    {'sgd_plain': lambda: bwd_case('sgd', None, 1e-4), 'sgd_clip': lambda: bwd_case('sgd', c, 1e-4)},
    {'adagrad_plain': lambda: bwd_case('adagrad', None, 1e-4),
     'adagrad_clip': lambda: bwd_case('adagrad', c, 1e-4)},
    {'adam_plain': lambda: bwd_case('adam', None, 1e-4), 'adam_clip': lambda: bwd_case('adam', c, 1e-4)},
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
  # (the stepping cases move the shared tables: later groups see more rows outside the ball)
  result['clipped_share_at_end'] = clipped_share()
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  print(json.dumps(result))


if __name__ == '__main__':
  main()
