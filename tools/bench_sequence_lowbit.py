"""The fused low-bit sequence lookup (hbk_sequence_lookup_fwd_lowbit) next to what it replaces, in one process, the
forms taking turns, on tools/bench_sequence.py's shape: 4 columns x 1M rows, B = 8192 samples, T = 50, lengths uniform
in [0, 2T], int64 ids, no pad id.  One cell per {bf16, int8 tables} x {fp32, bf16 outputs} x dim {16, 64, 128}:

  fused       (a) one launch: rows + grid + lengths (LowbitSequenceLookup)
  two_launch  (b) hbk_sequence_row_grid_n, then the one-id-per-position lookup over the grid: LowpGroupLookup /
                  Out16GroupLookup (bf16 tables) or Quant8GroupLookup(lane_codes='auto') (int8 tables)
  fp32        (c) the fp32 SequenceLookup with fp32 outputs: the traffic yardstick

Every step is the C-ABI calls alone on descriptors bound once (resident batches; a step reads another one).  Timing as
tools/bench_sequence.py: warm-up steps, `--steps` steps between HIP events, `--rounds` rounds with the forms taking
turns, the median per-step time of each with min / max.  Prints one JSON line and appends it to `--out` (default
profiles/sequence_lowbit.txt).  Run it in three fresh processes, then `--verdict` prints per cell the range of every
form over the processes and the verdict: (a) counts as faster than (b) only where it wins by more than the spread of
(b) over the processes.

  python tools/bench_sequence_lowbit.py [--steps 50 --warmup 10 --rounds 5]
  python tools/bench_sequence_lowbit.py --verdict
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

FORMS = ('fused', 'two_launch', 'fp32')


def verdict(path):
  runs = [json.loads(line) for line in open(path) if line.startswith('{')]
  cells = sorted({k for r in runs for k in r['cells']}, key=lambda k: (k.split('/')[0], k.split('/')[1], int(k.split('/')[2])))
  print(f'{len(runs)} processes; us per step, median of each process: min - max over the processes')
  print('%-18s %17s %17s %17s  %s' % ('tables/out/dim', 'fused (a)', 'two_launch (b)', 'fp32 (c)', 'verdict'))
  for cell in cells:
    t = {f: [r['cells'][cell][f + '_us'] for r in runs if cell in r['cells']] for f in FORMS}
    a, b = np.median(t['fused']), np.median(t['two_launch'])
    spread = max(t['two_launch']) - min(t['two_launch'])
    word = 'faster' if b - a > spread else ('slower' if a - b > spread else 'no difference')
    rng = lambda v: '%7.1f - %7.1f' % (min(v), max(v))   # noqa: E731
    print('%-18s %17s %17s %17s  (a) %s: %+.1f %% (spread of (b) %.1f us); %.2fx of fp32'
          % (cell, rng(t['fused']), rng(t['two_launch']), rng(t['fp32']), word, 100 * (a - b) / b, spread,
             a / np.median(t['fp32'])))


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--steps', type=int, default=50)
  p.add_argument('--warmup', type=int, default=10)
  p.add_argument('--rounds', type=int, default=5)
  p.add_argument('--batches', type=int, default=2)
  p.add_argument('--dims', default='16,64,128')
  p.add_argument('--verdict', action='store_true')
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_lowbit.txt'))
  args = p.parse_args()
  if args.verdict:
    return verdict(args.out)
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding import sequence as seq_mod   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_sequence_lowbit.py measures on a GPU: none found')
  E, lib = hb.embedding, _lib.lib()
  dev = torch.device('cuda:0')
  cols, rows, B, T = 4, 1_000_000, 8192, 50
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)
  rng = np.random.RandomState(4242)
  stream = _lib.current_stream(dev)
  batches = []
  for _ in range(args.batches):
    splits, ids = [], []
    for _ in range(cols):
      sp = np.concatenate([[0], np.cumsum(rng.randint(0, 2 * T + 1, size=B))]).astype(np.int32)
      splits.append(torch.from_numpy(sp).to(dev))
      ids.append(torch.randint(0, 1 << 40, (int(sp[-1]),), device=dev, dtype=torch.int64, generator=gen))
    batches.append((ids, splits))

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

  result = {'shape': {'cols': cols, 'rows': rows, 'B': B, 'T': T, 'positions': cols * B * T}, 'cells': {}}
  for dim in [int(d) for d in args.dims.split(',')]:
    f32 = [torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen) for _ in range(cols)]
    yard = []
    for ids, splits in batches:
      o = E.SequenceLookup(f32, [rows] * cols, T)
      o(ids, splits)
      yard.append(o)
    for fmt in ('bf16', 'int8'):
      tables = E.quantize_rows8(f32) if fmt == 'int8' else [t.to(torch.bfloat16) for t in f32]
      dims = [dim] * cols if fmt == 'int8' else None
      for out_dtype, out_name in ((torch.float32, 'fp32'), (torch.bfloat16, 'bf16')):
        fused, grid_side, plain = [], [], []
        for ids, splits in batches:
          a = E.LowbitSequenceLookup(tables, dims, [rows] * cols, T, out_dtype=out_dtype)
          got, _ = a(ids, splits)
          fused.append(a)
          # (b): the grid launch's descriptors, then the lookup over the grid as one id per position
          gc, gq = (_lib.LookupColumn * cols)(), (_lib.Sequence * cols)()
          for c in range(cols):
            gc[c].bucket, gc[c].divisor = rows, 1
          batch, _ = seq_mod._bind_ids(gc, gq, ids, splits, [T] * cols, [None] * cols)   # pylint: disable=protected-access
          lengths, grids = seq_mod._alloc_side(batch, [T] * cols, dev, True)   # pylint: disable=protected-access
          for c in range(cols):
            gq[c].lengths, gq[c].row_grid = lengths[c].data_ptr(), grids[c].data_ptr()
          _lib.check(lib.hbk_sequence_row_grid_n(cols, gc, gq, stream))
          if fmt == 'int8':
            b = E.Quant8GroupLookup(tables, dims, out_dtype=out_dtype, lane_codes='auto')
          elif out_dtype == torch.float32:
            b = E.LowpGroupLookup(tables)
          else:
            b = E.Out16GroupLookup(tables, out_dtype=out_dtype)
          outs = b(grids)
          for x, y in zip(got, outs):
            assert torch.equal(x.view(B * T, dim), y)   # the two forms give the same bits
          grid_side.append((gc, gq, ids, splits, lengths, grids))
          plain.append(b)

        def step_fused(i, fused=fused):
          o = fused[i % len(fused)]
          _lib.check(lib.hbk_sequence_lookup_fwd_lowbit(cols, o._cols, o._seqs, stream))

        def step_two(i, grid_side=grid_side, plain=plain):
          gc, gq = grid_side[i % len(plain)][:2]
          _lib.check(lib.hbk_sequence_row_grid_n(cols, gc, gq, stream))
          plain[i % len(plain)].launch()

        def step_fp32(i):
          o = yard[i % len(yard)]
          _lib.check(lib.hbk_group_lookup_fwd_sequence(cols, o._cols, o._seqs, None, stream))
        steps = {'fused': step_fused, 'two_launch': step_two, 'fp32': step_fp32}
        t = {k: [] for k in steps}
        for _ in range(args.rounds):
          for k in steps:   # taking turns
            t[k].append(timed(steps[k]))
        cell = {k + '_us': round(float(np.median(v)), 2) for k, v in t.items()}
        cell.update({k + '_min_max_us': [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})
        cell['lane_elems'] = fused[0].lane_elems_used[0]
        result['cells'][f'{fmt}/{out_name}/{dim}'] = cell
        del fused, grid_side, plain
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    del yard, f32
    torch.cuda.empty_cache()
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  line = json.dumps(result)
  print(line)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
