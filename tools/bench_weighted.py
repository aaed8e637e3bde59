"""Weighted (sp_weights) against unweighted lookups, in one process, alternating:

  fwd            config 2 forward: 26 columns x 1M x 16, batch 65536, one id per sample, sum
  bwd_emit       config 2 backward -> IndexedSlices
  bwd_sgd        the same + fused SGD
  bwd_step_only  the fused SGD step alone
  bwd_ragged     26 columns x 65536 segments of Poisson(8) ids clipped to [0, 32], mean, IndexedSlices

Timing follows bench.py: resident id batches (a step reads another one; nothing is served from the
Infinity Cache by repetition), warm-up steps, then `--steps` launches between HIP events; the two forms
take turns for `--rounds` rounds and the median per-step time of each is reported (with min / max).
Prints one JSON line.

  python tools/bench_weighted.py [--steps 20 --warmup 5 --rounds 5]
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
  flat = [[torch.randint(0, 1 << 40, (batch,), device=dev, dtype=torch.int64, generator=gen)
           for _ in range(cols)] for _ in range(args.batches)]
  rng = np.random.RandomState(4242)
  splits, counts = [], []
  for _ in range(cols):
    sp = np.concatenate([[0], np.cumsum(rng.poisson(8, size=batch).clip(0, 32))]).astype(np.int32)
    splits.append(torch.from_numpy(sp).to(dev))
    counts.append(int(sp[-1]))
  ragged = [[torch.randint(0, 1 << 40, (counts[c],), device=dev, dtype=torch.int64, generator=gen)
             for c in range(cols)] for _ in range(args.batches)]

  def weights(pool):
    return [[torch.empty(i.numel(), device=dev).uniform_(0.5, 2.0, generator=gen) for i in b] for b in pool]
  w_flat, w_ragged = weights(flat), weights(ragged)
  grads = [torch.randn(batch, dim, device=dev, generator=gen) for _ in range(cols)]
  out_block = [torch.empty(batch, dim, device=dev) for _ in range(cols)]

  def fwd_case(weighted):
    objs = []
    for b in range(args.batches):   # one bound lookup per resident batch: a step is one C-ABI call
      lk = hb.embedding.GroupLookup(tables, buckets=[rows] * cols, combiners='sum')
      lk(flat[b], outs=out_block, sp_weights=w_flat[b] if weighted else None)
      objs.append(lk)
    return lambda i: objs[i % len(objs)].launch()

  def bwd_case(weighted, pool, wpool, sp, combiner, lr, emit):
    lookup = hb.embedding.GroupLookup(tables, buckets=[rows] * cols, combiners=combiner)
    objs = []
    for b in range(args.batches):
      g = hb.embedding.GroupLookupGrad(lookup, workspace_of=objs[0] if objs else None)
      g(pool[b], grads, sp, apply_lr=lr, emit=emit, sp_weights=wpool[b] if weighted else None)
      objs.append(g)
    return lambda i: objs[i % len(objs)].launch(apply_lr=lr)

  cases = {
    'fwd': lambda w: fwd_case(w),
    'bwd_emit': lambda w: bwd_case(w, flat, w_flat, None, 'sum', 0.0, True),
    'bwd_sgd': lambda w: bwd_case(w, flat, w_flat, None, 'sum', 1e-4, True),
    'bwd_step_only': lambda w: bwd_case(w, flat, w_flat, None, 'sum', 1e-4, False),
    'bwd_ragged': lambda w: bwd_case(w, ragged, w_ragged, splits, 'mean', 0.0, True),
  }

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
  for name, make in cases.items():
    steps = {False: make(False), True: make(True)}
    t = {False: [], True: []}
    for _ in range(args.rounds):
      for w in (False, True):   # alternating
        t[w].append(timed(steps[w]))
    med = {w: float(np.median(t[w])) for w in t}
    result[name] = {'unweighted_us': round(med[False], 2), 'weighted_us': round(med[True], 2),
                    'ratio': round(med[True] / med[False], 3),
                    'unweighted_min_max_us': [round(min(t[False]), 2), round(max(t[False]), 2)],
                    'weighted_min_max_us': [round(min(t[True]), 2), round(max(t[True]), 2)]}
    del steps
    torch.cuda.synchronize()
  result['expansion_bytes'] = {'bwd_emit': cols * batch * dim * 4, 'bwd_ragged': sum(counts) * dim * 4}
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  print(json.dumps(result))


if __name__ == '__main__':
  main()
