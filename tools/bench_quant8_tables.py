"""8-bit tables against fp32 and bf16 ones, in one process, the forms taking turns; every launch a replay of a
captured graph.

Forward, 26 columns x 1M rows, batch 65536, into fp32 and into bf16 outputs (`_o32` / `_o16`):

  c2      dim 16, one id per sample (config 2's shape)
  d64     dim 64, one id per sample
  d128    dim 128, one id per sample
  ragged  dim 16, Poisson(8) ids per sample clipped to [0, 32], mean
  ragged64  the same at dim 64

  fp32    hb.embedding.GroupLookup / Out16GroupLookup over fp32 tables
  bf16    LowpGroupLookup / Out16GroupLookup over bf16 tables (their default lane widths)
  int8    Quant8GroupLookup, 4 codes per lane (hbk_quant8_lookup_fwd: the baseline of the wide lanes)
  int8_L8 / int8_L16      lane_codes 8 / 16 over the same tables (default pitch dim + 4: L / 4 loads of 4 bytes)
  int8p / int8p_L8 / int8p_L16   4, 8 and 16 codes per lane over tables whose pitch is rounded up to 16 (one load)

Step, on c2's shape and the same ids and gradients, for SGD, Adagrad and row-wise Adagrad: the emit-form reduce
and the split apply, `bf16_rn` / `bf16_sr` (LowpLookupGrad) against `int8_rn` / `int8_sr` (Quant8LookupGrad).

The forms of a case take turns for `--rounds` rounds (default 7); per form the median time per launch with min and
max.  Beside every forward line: bytes per looked-up row by the README's model (8 B id + table row + output row);
beside every step line: bytes per row of table plus optimizer state.  Appends its lines to `--out` (default
profiles/quant8_tables.txt) and prints one JSON line.

  python tools/bench_quant8_tables.py [--steps 20 --warmup 5 --rounds 7 --cases c2,d64,d128,ragged,ragged64,step]
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
  p.add_argument('--cases', default='c2,d64,d128,ragged,ragged64,step')
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'quant8_tables.txt'))
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

  def take_turns(case, forms, row_bytes, what):
    t = {k: [] for k in forms}
    for _ in range(args.rounds):
      for k in forms:
        t[k].append(timed(forms[k]))
    out = {}
    for k in forms:
      med = float(np.median(t[k]))
      out[f'{case}_{k}'] = {'us': round(med, 2), 'min_max_us': [round(min(t[k]), 2), round(max(t[k]), 2)],
                            'row_bytes': row_bytes[k]}
      lines.append(f'{case:14s} {k:10s} {med:9.2f} us  (min {min(t[k]):.2f}, max {max(t[k]):.2f})   '
                   f'{row_bytes[k]:4d} {what}')
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
    t8 = E.quantize_rows8(t32)
    t8p = E.quantize_rows8(t32, pitch=E.Quant8Rows.pitch_for(dim, 16))
    ids, splits = ids_of(is_ragged)
    combiner = 'mean' if is_ragged else 'sum'
    buckets, dims = [rows] * cols, [dim] * cols
    out = {}
    for tag, odt, obytes in (('o32', torch.float32, 4), ('o16', torch.bfloat16, 2)):
      block = torch.empty(batch, cols * dim, device=dev, dtype=odt)
      outs = [block[:, c * dim:(c + 1) * dim] for c in range(cols)]
      if odt == torch.float32:
        looks = {'fp32': E.GroupLookup(t32, buckets, combiner), 'bf16': E.LowpGroupLookup(t16, buckets, combiner)}
      else:
        looks = {'fp32': E.Out16GroupLookup(t32, buckets, combiner, out_dtype=odt),
                 'bf16': E.Out16GroupLookup(t16, buckets, combiner, out_dtype=odt)}
      for k, t in (('int8', t8), ('int8p', t8p)):
        for lane_codes in (None, 8, 16):
          if lane_codes is None or dim % lane_codes == 0:
            looks[k + (f'_L{lane_codes}' if lane_codes else '')] = E.Quant8GroupLookup(
              t, dims, buckets, combiner, out_dtype=odt, lane_codes=lane_codes)
      forms = {}
      for k, look in looks.items():
        look(ids, splits, outs)
        if k.startswith('int8'):   # the form runs the path it names
          assert look.lane_codes_used == [int(k.split('_L')[1]) if '_L' in k else 4] * cols, (k, look.lane_codes_used)
        forms[k] = graphed(look.launch)
      table_bytes = {'fp32': 4 * dim, 'bf16': 2 * dim, 'int8': E.Quant8Rows.pitch_for(dim),
                     'int8p': E.Quant8Rows.pitch_for(dim, 16)}
      out.update(take_turns(f'{name}_{tag}', forms,
                            {k: 8 + table_bytes[k.split('_')[0]] + obytes * dim for k in forms},
                            'B per looked-up row (id + table row + output row)'))
    return out

  def step_case(name, dim):
    ids, _ = ids_of(False)
    grads = [torch.randn(batch, dim, device=dev, generator=gen) for _ in range(cols)]
    out = {}
    for opt, state in (('sgd', 0), ('adagrad', 4 * dim), ('rowwise_adagrad', 4)):
      def slots():
        if opt == 'adagrad':
          return dict(accums=[torch.full((rows, dim), 0.1, device=dev) for _ in range(cols)])
        if opt == 'rowwise_adagrad':
          return dict(row_accums=[torch.full((rows, 1), 0.1, device=dev) for _ in range(cols)])
        return {}
      forms, keep = {}, []
      for k, rounding in (('bf16_rn', 'nearest'), ('bf16_sr', 'stochastic'), ('int8_rn', 'nearest'),
                          ('int8_sr', 'stochastic')):
        t32 = [torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen) for _ in range(cols)]
        if k.startswith('bf16'):
          grad = E.LowpLookupGrad(E.LowpGroupLookup([t.to(torch.bfloat16) for t in t32], [rows] * cols, 'sum'),
                                  rounding=rounding, seed=1, **slots())
        else:
          grad = E.Quant8LookupGrad(E.Quant8GroupLookup(E.quantize_rows8(t32), [dim] * cols, [rows] * cols, 'sum'),
                                    rounding=rounding, seed=1, **slots())
        del t32
        grad(ids, grads, None, apply_lr=1e-4, optimizer=opt)
        forms[k] = graphed(lambda g=grad: g.launch(1e-4, opt))
        keep.append(grad)
      bytes_of = {k: (2 * dim if k.startswith('bf16') else E.Quant8Rows.pitch_for(dim)) + state for k in forms}
      out.update(take_turns(f'{name}_{opt.replace("rowwise_adagrad", "rowwise")}', forms, bytes_of,
                            'B/row of table + state'))
      del forms, keep
      torch.cuda.empty_cache()
    return out

  result = {}
  fwd = {'c2': (16, False), 'd64': (64, False), 'd128': (128, False), 'ragged': (16, True), 'ragged64': (64, True)}
  for name in args.cases.split(','):
    result.update(step_case('step', 16) if name == 'step' else forward_case(name, *fwd[name]))
    torch.cuda.empty_cache()
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(f'# tools/bench_quant8_tables.py --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} '
            f'--cases {args.cases}: graph replays, medians of {args.rounds}\n')
    f.write('\n'.join(lines) + '\n')
  print(json.dumps(result))


if __name__ == '__main__':
  main()
