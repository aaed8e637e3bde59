"""Low-precision tables against fp32 ones, in one process, the forms taking turns; every launch a replay of a
captured graph.

Forward (hb.embedding.GroupLookup against LowpGroupLookup, bf16 rows; `bf16x4` / `bf16x8`: 4 / 8 elements per
lane, the A/B behind the default of 8 from dim 64 on), 26 columns x 1M rows, batch 65536:

  c2      dim 16, one id per sample (config 2's shape)
  d64     dim 64, one id per sample
  d128    dim 128, one id per sample
  ragged  dim 16, Poisson(8) ids per sample clipped to [0, 32], mean

Step, on c2's shape and the same ids and gradients, for SGD, Adagrad and row-wise Adagrad:

  fused32   GroupLookupGrad with apply_lr: the reduce and the step in one pass
  split32   GroupLookupGrad in its emit form, then SparseApply on the slices
  bf16_rn   LowpLookupGrad, rounding to nearest      (emit form, then LowpSparseApply)
  bf16_sr   LowpLookupGrad, stochastic rounding

The forms of a case take turns for `--rounds` rounds (default 7); per form the median time per launch with min and
max.  Beside every line: bytes per row of table plus optimizer state.  Appends its lines to `--out` (default
profiles/lowp_tables.txt) and prints one JSON line.

  python tools/bench_lowp_tables.py [--steps 20 --warmup 5 --rounds 7 --cases c2,d64,d128,ragged,step]
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
  p.add_argument('--cases', default='c2,d64,d128,ragged,step')
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lowp_tables.txt'))
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

  def take_turns(case, forms, row_bytes):
    t = {k: [] for k in forms}
    for _ in range(args.rounds):
      for k in forms:
        t[k].append(timed(forms[k]))
    out = {}
    for k in forms:
      med = float(np.median(t[k]))
      out[f'{case}_{k}'] = {'us': round(med, 2), 'min_max_us': [round(min(t[k]), 2), round(max(t[k]), 2)],
                            'row_bytes': row_bytes[k]}
      lines.append(f'{case:13s} {k:8s} {med:9.2f} us  (min {min(t[k]):.2f}, max {max(t[k]):.2f})   '
                   f'{row_bytes[k]:4d} B/row of table + state')
    return out

  def ids_of(is_ragged):
    if not is_ragged:
      return [torch.randint(0, 1 << 40, (batch,), device=dev, dtype=torch.int64, generator=gen)
              for _ in range(cols)], None
    splits = [torch.from_numpy(np.concatenate([[0], np.cumsum(rng.poisson(8, size=batch).clip(0, 32))])
                               .astype(np.int32)).to(dev) for _ in range(cols)]
    return [torch.randint(0, 1 << 40, (int(s[-1]),), device=dev, dtype=torch.int64, generator=gen)
            for s in splits], splits

  def forward_case(name, dim, is_ragged):
    t32 = [torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen) for _ in range(cols)]
    t16 = [t.to(torch.bfloat16) for t in t32]
    ids, splits = ids_of(is_ragged)
    combiner = 'mean' if is_ragged else 'sum'
    block = torch.empty(batch, cols * dim, device=dev)
    outs = [block[:, c * dim:(c + 1) * dim] for c in range(cols)]
    looks = {'fp32': E.GroupLookup(t32, [rows] * cols, combiner),
             'bf16x4': E.LowpGroupLookup(t16, [rows] * cols, combiner, chunk_elems=4)}
    if dim % 8 == 0:
      looks['bf16x8'] = E.LowpGroupLookup(t16, [rows] * cols, combiner, chunk_elems=8)
    forms = {}
    for k, look in looks.items():
      look(ids, splits, outs)
      forms[k] = graphed(look.launch)
    return take_turns(name, forms, {k: (4 if k == 'fp32' else 2) * dim for k in forms})

  def step_case(name, dim):
    ids, _ = ids_of(False)
    grads = [torch.randn(batch, dim, device=dev, generator=gen) for _ in range(cols)]
    out = {}
    for opt, state in (('sgd', 0), ('adagrad', 4 * dim), ('rowwise_adagrad', 4)):
      def fresh(dtype):
        tables = [torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen).to(dtype)
                  for _ in range(cols)]
        kw = {}
        if opt == 'adagrad':
          kw['accums'] = [torch.full((rows, dim), 0.1, device=dev) for _ in range(cols)]
        elif opt == 'rowwise_adagrad':
          kw['row_accums'] = [torch.full((rows, 1), 0.1, device=dev) for _ in range(cols)]
        return tables, kw
      forms, keep = {}, []
      tables, kw = fresh(torch.float32)
      fused = E.GroupLookupGrad(E.GroupLookup(tables, [rows] * cols, 'sum'), **kw)
      fused(ids, grads, None, apply_lr=1e-4, optimizer=opt)
      forms['fused32'] = graphed(lambda g=fused: g.launch(apply_lr=1e-4, optimizer=opt))
      tables, kw = fresh(torch.float32)
      emit = E.GroupLookupGrad(E.GroupLookup(tables, [rows] * cols, 'sum'))
      apply32 = E.SparseApply(tables, **kw)
      apply32(emit(ids, grads, None), 1e-4, opt)

      def split(e=emit, a=apply32):
        e.launch(0.0)
        a.launch()
      forms['split32'] = graphed(split)
      keep += [fused, emit, apply32]
      for k, rounding in (('bf16_rn', 'nearest'), ('bf16_sr', 'stochastic')):
        tables, kw = fresh(torch.bfloat16)
        low = E.LowpLookupGrad(E.LowpGroupLookup(tables, [rows] * cols, 'sum'), rounding=rounding, seed=1, **kw)
        low(ids, grads, None, apply_lr=1e-4, optimizer=opt)
        forms[k] = graphed(lambda g=low: g.launch(1e-4, opt))
        keep.append(low)
      bytes_of = {k: (4 if k.endswith('32') else 2) * dim + state for k in forms}
      out.update(take_turns(f'{name}_{opt.replace("rowwise_adagrad", "rowwise")}', forms, bytes_of))
      del forms, keep
      torch.cuda.empty_cache()
    return out

  result = {}
  fwd = {'c2': (16, False), 'd64': (64, False), 'd128': (128, False), 'ragged': (16, True)}
  for name in args.cases.split(','):
    result.update(step_case('step', 16) if name == 'step' else forward_case(name, *fwd[name]))
    torch.cuda.empty_cache()
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(f'# tools/bench_lowp_tables.py --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} '
            f'--cases {args.cases}: graph replays, medians of {args.rounds}\n')
    f.write('\n'.join(lines) + '\n')
  print(json.dumps(result))


if __name__ == '__main__':
  main()
