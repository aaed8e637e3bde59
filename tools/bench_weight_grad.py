"""The weight gradient (hbk_group_lookup_bwd_weights) next to the weighted forward, in one process,
alternating, every column weighted:

  h1          config 2: 26 columns x 1M x 16, batch 65536, one id per sample, sum
  h1_mean     the same, mean (the general formula on a segment of one id)
  ragged      26 columns x 65536 segments of Poisson(8) ids clipped to [0, 32], mean
  dim128      8 columns x 1M x 128, batch 65536, one id per sample, sum
  *_clip      the same with every column clipped (max_norm = the median row norm)

Per case the forward (GroupLookup.launch), the weight gradient (one hbk_group_lookup_bwd_weights call on
the same descriptors) and the weight gradient with option bwd_weights_lds = 0 (every segment longer than
the row's lanes takes the second sweep in memory instead of parking d_j in LDS) take turns.  Timing follows tools/bench_weighted.py: resident id batches (a
step reads another one), warm-up steps, then `--steps` launches between HIP events, `--rounds` rounds;
the median per-step time of each is reported with min / max.  Prints one JSON line.

  python tools/bench_weight_grad.py [--steps 20 --warmup 5 --rounds 5]
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
  rows, batch = 1_000_000, 65536
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)
  rng = np.random.RandomState(4242)

  def make(cols, dim, ragged, combiner, clip):
    tables = [torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen) for _ in range(cols)]
    max_norm = float(tables[0][:4096].norm(dim=1).median()) if clip else None
    splits, counts = None, [batch] * cols
    if ragged:
      splits, counts = [], []
      for _ in range(cols):
        sp = np.concatenate([[0], np.cumsum(rng.poisson(8, size=batch).clip(0, 32))]).astype(np.int32)
        splits.append(torch.from_numpy(sp).to(dev))
        counts.append(int(sp[-1]))
    grads = [torch.randn(batch, dim, device=dev, generator=gen) for _ in range(cols)]
    outs = [torch.empty(batch, dim, device=dev) for _ in range(cols)]
    fwd, bwd = [], []
    for _ in range(args.batches):   # one bound object per resident batch: a step is one C-ABI call
      ids = [torch.randint(0, 1 << 40, (k,), device=dev, dtype=torch.int64, generator=gen) for k in counts]
      w = [torch.empty(k, device=dev).uniform_(0.5, 2.0, generator=gen) for k in counts]
      lk = hb.embedding.GroupLookup(tables, buckets=[rows] * cols, combiners=combiner, max_norms=max_norm)
      lk(ids, splits, outs=outs, sp_weights=w)
      g = hb.embedding.GroupLookupGrad(lk)
      _, dw = g(ids, grads, splits, sp_weights=w, weight_grads=True)
      fwd.append(lk)
      bwd.append((g, dw))
    n = len(tables)

    def weight_grad(i):
      g, _ = bwd[i % len(bwd)]
      _lib.check(g._lib.hbk_group_lookup_bwd_weights(n, g._cols, g.lookup.max_norms_c, g._wg[1],
                                                     _lib.current_stream(dev)))
    return {'fwd': lambda i: fwd[i % len(fwd)].launch(), 'weight_grad': weight_grad,
            'weight_grad_sweep': weight_grad}, sum(counts)

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

  shapes = {'h1': (26, 16, False, 'sum'), 'h1_mean': (26, 16, False, 'mean'),
            'ragged': (26, 16, True, 'mean'), 'dim128': (8, 128, False, 'sum')}
  result = {}
  for name, (cols, dim, ragged, combiner) in shapes.items():
    for clip in (False, True):
      steps, n_ids = make(cols, dim, ragged, combiner, clip)
      t = {k: [] for k in steps}
      for _ in range(args.rounds):
        for k in steps:   # alternating
          old = _lib.set_option('bwd_weights_lds', 0 if k == 'weight_grad_sweep' else 1)
          t[k].append(timed(steps[k]))
          _lib.set_option('bwd_weights_lds', old)
      med = {k: float(np.median(v)) for k, v in t.items()}
      result[name + ('_clip' if clip else '')] = {
        'ids': n_ids, 'fwd_us': round(med['fwd'], 2), 'weight_grad_us': round(med['weight_grad'], 2),
        'ratio': round(med['weight_grad'] / med['fwd'], 3),
        'fwd_min_max_us': [round(min(t['fwd']), 2), round(max(t['fwd']), 2)],
        'weight_grad_min_max_us': [round(min(t['weight_grad']), 2), round(max(t['weight_grad']), 2)],
        'sweep_us': round(med['weight_grad_sweep'], 2),
        'sweep_min_max_us': [round(min(t['weight_grad_sweep']), 2), round(max(t['weight_grad_sweep']), 2)]}
      del steps
      torch.cuda.synchronize()
      torch.cuda.empty_cache()
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  print(json.dumps(result))


if __name__ == '__main__':
  main()
