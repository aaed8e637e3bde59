"""The sequence lookup (hbk_group_lookup_fwd_sequence) next to its two-launch form and its backward, in
one process, alternating, on a DIN-like shape: 4 columns x 1M rows x dim 16, B = 8192 samples, T = 50,
lengths uniform in [0, 2T], int64 ids; once without and once with a pad id.

  fused_grid     (a) one launch: gather + pad + grid + lengths
  fused_nogrid   (b) the same without the grid (inference)
  two_launch     (c) hbk_sequence_row_grid_n, then hbk_group_lookup_fwd over the grid
  bwd_sgd        (d) the backward over the grid with the fused SGD step (step only)

Every step is the C-ABI calls alone on descriptors bound once (resident batches; a step reads another
one).  Timing follows tools/bench_weight_grad.py: warm-up steps, then `--steps` steps between HIP events,
`--rounds` rounds with the forms taking turns; the median per-step time of each is reported with min /
max.  Prints one JSON line and appends it to `--out` (default profiles/sequence_lookup.txt).  Run it in
several fresh processes to see the spread between processes.

  python tools/bench_sequence.py [--steps 50 --warmup 10 --rounds 5]
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
  p.add_argument('--steps', type=int, default=50)
  p.add_argument('--warmup', type=int, default=10)
  p.add_argument('--rounds', type=int, default=5)
  p.add_argument('--batches', type=int, default=4)
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_lookup.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_sequence.py measures on a GPU: none found')
  lib = _lib.lib()
  dev = torch.device('cuda:0')
  cols, rows, dim, B, T = 4, 1_000_000, 16, 8192, 50
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)
  rng = np.random.RandomState(4242)
  tables = [torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen) for _ in range(cols)]
  grads = [torch.randn(B, T, dim, device=dev, generator=gen) for _ in range(cols)]

  def make(pad):
    forms = {'fused_grid': [], 'fused_nogrid': [], 'two_launch': [], 'bwd_sgd': []}
    valid = 0
    for _ in range(args.batches):
      splits, ids = [], []
      for _ in range(cols):
        lens = rng.randint(0, 2 * T + 1, size=B)
        valid += int(np.minimum(lens, T).sum())
        sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        splits.append(torch.from_numpy(sp).to(dev))
        ids.append(torch.randint(0, 1 << 40, (int(sp[-1]),), device=dev, dtype=torch.int64, generator=gen))
      kw = dict(buckets=[rows] * cols, max_lens=T, pad_ids=pad)
      a = hb.embedding.SequenceLookup(tables, fused=True, **kw)
      a(ids, splits)
      b = hb.embedding.SequenceLookup(tables, fused=True, **kw)
      b(ids, splits, grids=False)
      c = hb.embedding.SequenceLookup(tables, fused=False, **kw)
      c(ids, splits)
      for x, y in zip(a(ids, splits)[0], c(ids, splits)[0]):
        assert torch.equal(x, y)                      # the two forms give the same bits
      g = hb.embedding.SequenceLookupGrad(a)
      g(grads, apply_lr=1e-6, emit=False)
      forms['fused_grid'].append(a)
      forms['fused_nogrid'].append(b)
      forms['two_launch'].append(c)
      forms['bwd_sgd'].append(g.driver(False))
    stream = _lib.current_stream(dev)

    def fused(objs):
      def step(i):
        o = objs[i % len(objs)]
        _lib.check(lib.hbk_group_lookup_fwd_sequence(cols, o._cols, o._seqs, None, stream))
      return step

    def two_launch(i):
      o = forms['two_launch'][i % args.batches]
      _lib.check(lib.hbk_sequence_row_grid_n(cols, o._cols, o._seqs, stream))
      o.plain_lookup().launch()

    def bwd(i):
      forms['bwd_sgd'][i % args.batches].launch(apply_lr=1e-6)
    # (the plain lookup of a two-launch object is bound to that object's last grids and outputs)
    return {'fused_grid': fused(forms['fused_grid']), 'fused_nogrid': fused(forms['fused_nogrid']),
            'two_launch': two_launch, 'bwd_sgd': bwd}, valid // args.batches

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

  result = {'shape': {'cols': cols, 'rows': rows, 'dim': dim, 'B': B, 'T': T, 'positions': cols * B * T}}
  for name, pad in (('no_pad', None), ('pad', 0)):
    steps, valid = make(pad)
    t = {k: [] for k in steps}
    for _ in range(args.rounds):
      for k in steps:   # alternating
        t[k].append(timed(steps[k]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    looked = cols * B * T if pad is not None else valid
    # bytes the fused form with the grid must move: ids of valid positions, a row read per looked-up
    # position, a row written and a grid word per position, lengths
    algo = valid * 8 + looked * dim * 4 + cols * B * T * (dim * 4 + 8) + cols * B * 8
    result[name] = {k + '_us': round(v, 2) for k, v in med.items()}
    result[name].update({k + '_min_max_us': [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})
    result[name]['valid_positions'] = valid
    result[name]['fused_grid_algorithmic_GBps'] = round(algo / med['fused_grid'] / 1e3, 1)
    result[name]['fused_over_two_launch'] = round(med['fused_grid'] / med['two_launch'], 4)
    del steps
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  line = json.dumps(result)
  print(line)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
