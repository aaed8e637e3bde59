"""The forward with 16-bit outputs against what a user does today (fp32 outputs, then ``.to(bfloat16)``), in one
process, the forms taking turns; every launch a replay of a captured graph.

26 columns x 1M rows, batch 65536, outputs as column blocks of one tensor:

  c2      dim 16, one id per sample
  d64     dim 64, one id per sample
  d128    dim 128, one id per sample
  ragged  dim 16, Poisson(8) ids per sample clipped to [0, 32], mean

Forms:

  a       GroupLookup                                  (fp32 tables, fp32 block)
  b       a, then block.to(bfloat16)                   (the baseline of c)
  c4 c8   Out16GroupLookup over the fp32 tables, 4 / 8 elements per lane
  d       LowpGroupLookup                              (bf16 tables, fp32 block)
  e       d, then block.to(bfloat16)                   (the baseline of f)
  f4 f8   Out16GroupLookup over the bf16 tables, 4 / 8 elements per lane

c4 / c8 and f4 / f8 are the A/B behind the default lane width.  The forms take turns for `--rounds` rounds (default
7); per form the median time per launch with min and max, beside its byte model per row and column: 8 B id + table row
+ output row (+ the cast pass's read and write).  Appends its lines to `--out` (default profiles/out16_lookup.txt) and
prints one JSON line.

  python tools/bench_out16_lookup.py [--steps 20 --warmup 5 --rounds 7 --cases c2,d64,d128,ragged]
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
  p.add_argument('--cases', default='c2,d64,d128,ragged')
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'out16_lookup.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  E = hb.embedding
  dev = torch.device('cuda:0')
  cols, rows, batch = 26, 1_000_000, 65536
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)
  rng = np.random.RandomState(4242)
  lines = []

  def graphed(fn):
    """fn() once eagerly (binds, loads code), then captured: the returned callable replays it."""
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
      with torch.cuda.graph(g, stream=s):
        fn()
    torch.cuda.synchronize()
    return g.replay

  def timed(replay):
    for _ in range(args.warmup):
      replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
      replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps   # us per launch

  def case(name, dim, is_ragged):
    t32 = [torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen) for _ in range(cols)]
    t16 = [t.to(torch.bfloat16) for t in t32]
    splits, n_ids = None, [batch] * cols
    if is_ragged:
      splits = [torch.from_numpy(np.concatenate([[0], np.cumsum(rng.poisson(8, size=batch).clip(0, 32))])
                                 .astype(np.int32)).to(dev) for _ in range(cols)]
      n_ids = [int(s[-1]) for s in splits]
    ids = [torch.randint(0, 1 << 40, (k,), device=dev, dtype=torch.int64, generator=gen) for k in n_ids]
    combiner = 'mean' if is_ragged else 'sum'
    block32 = torch.empty(batch, cols * dim, device=dev)
    block16 = torch.empty(batch, cols * dim, device=dev, dtype=torch.bfloat16)
    outs32 = [block32[:, c * dim:(c + 1) * dim] for c in range(cols)]
    outs16 = [block16[:, c * dim:(c + 1) * dim] for c in range(cols)]
    buckets = [rows] * cols
    widths = (4, 8) if dim % 8 == 0 else (4,)
    looks = {'a': (E.GroupLookup(t32, buckets, combiner), outs32),
             'd': (E.LowpGroupLookup(t16, buckets, combiner), outs32)}
    for w in widths:
      looks[f'c{w}'] = (E.Out16GroupLookup(t32, buckets, combiner, chunk_elems=w), outs16)
      looks[f'f{w}'] = (E.Out16GroupLookup(t16, buckets, combiner, chunk_elems=w), outs16)
    forms = {}
    for k, (look, outs) in looks.items():
      look(ids, splits, outs)
      forms[k] = graphed(look.launch)
    for k, base in (('b', 'a'), ('e', 'd')):
      def with_cast(look=looks[base][0]):
        look.launch()
        block16.copy_(block32)
      forms[k] = graphed(with_cast)
    # bytes per output row and column: the ids of the row, the table rows they name, the output row, the cast pass
    per_row = float(np.mean(n_ids)) / batch
    model = {k: per_row * (8 + (4 if k[0] in 'abc' else 2) * dim) +
             (2 if k[0] in 'cf' else 4) * dim + (6 * dim if k[0] in 'be' else 0) for k in forms}
    t = {k: [] for k in sorted(forms)}
    for _ in range(args.rounds):
      for k in t:
        t[k].append(timed(forms[k]))
    out = {}
    for k in t:
      med = float(np.median(t[k]))
      out[f'{name}_{k}'] = {'us': round(med, 2), 'min_max_us': [round(min(t[k]), 2), round(max(t[k]), 2)],
                            'model_bytes': round(model[k], 1)}
      lines.append(f'{name:8s} {k:3s} {med:9.2f} us  (min {min(t[k]):.2f}, max {max(t[k]):.2f})   '
                   f'{model[k]:7.1f} B per row and column')
    return out

  result = {}
  shapes = {'c2': (16, False), 'd64': (64, False), 'd128': (128, False), 'ragged': (16, True)}
  for name in args.cases.split(','):
    result.update(case(name, *shapes[name]))
    torch.cuda.empty_cache()
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(f'# tools/bench_out16_lookup.py --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} '
            f'--cases {args.cases}: graph replays, medians of {args.rounds}\n')
    f.write('\n'.join(lines) + '\n')
  print(json.dumps(result))


if __name__ == '__main__':
  main()
