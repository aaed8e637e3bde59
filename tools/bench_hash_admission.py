"""The admission filter (hbk_hash_insert_admit_n, hbk_hash_insert_expiring_admit_n) next to the entries without
one, in one process, forms alternating, on the shape of tools/bench_hash_insert.py: 26 columns x 65 536 one-id
int64 keys, dim 16, every table of capacity 131 072 (load factor 0.5 once the batch is resident), slab_size 8;
sketch depth 4, width = capacity, min_freq 2.

  hit / f_hit            every key of the batch is resident (steady state: warm-up, then --steps launches)
  new / f_new            the first batch of new distinct ids on empty tables and a zero sketch: the unfiltered
                         tables insert them all, the filtered ones only count (every id answered -1 but the few
                         whose cells all collide: `*_new_admitted_early`)
  again / f_again        the same batch again: the filtered tables admit every id now (the unfiltered form is
                         `new` once more: tables emptied, every id inserted)
  zipf / f_zipf          a Zipf(1.2) batch over the resident keys
  zipf_new / f_zipf_new  the same Zipf batch on empty tables and a zero sketch: its hot ids, not yet admitted,
                         send all their occurrences to `depth` counters
  x_* / xf_*             the same on expiring tables

Launches that need a prepared table are timed alone between their own events (median of 5), as `miss` is in
tools/bench_hash_expiry.py.  `--entries-only` measures hit and x_hit alone and uses nothing this filter added:
run from a checkout of the parent commit in the same visit, it is the comparison of the two existing entries.
Prints one JSON line and appends it to `--out` (default profiles/hash_admission.txt).

  python tools/bench_hash_admission.py [--steps 50 --warmup 10 --rounds 5] [--entries-only --label parent]
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
  p.add_argument('--slab-size', type=int, default=8)
  p.add_argument('--entries-only', action='store_true')
  p.add_argument('--label', default='')
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_admission.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding.cache import EMPTY_KEY   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_admission.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  cols, batch, dim, slab_size, min_freq = 26, 65536, 16, args.slab_size, 2
  capacity = 2 * batch
  rng = np.random.RandomState(777)

  def distinct(n):
    return torch.from_numpy(np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n + 64, dtype=np.int64))[:n]
                            .copy()).to(dev)
  resident = [distinct(batch)[torch.randperm(batch, device=dev)].contiguous() for _ in range(cols)]
  zipf = [r[torch.from_numpy((rng.zipf(1.2, size=batch) - 1) % batch).to(dev)] for r in resident]
  stream = _lib.current_stream(dev)

  def timed(step):
    for _ in range(args.warmup):
      step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
      step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps   # us per step

  def timed_alone(prepare, step, n=5):
    out = []
    for _ in range(n):
      prepare()
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      step()
      e1.record()
      e1.synchronize()
      out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out))

  def make(expiring, filtered):
    kw = dict(min_freq=min_freq, sketch_depth=4) if filtered else {}
    return [hb.embedding.HashTable(capacity, dim, dev, slab_size=slab_size, expiring=expiring, **kw)
            for _ in range(cols)]

  def empty(tables):
    for t in tables:
      t.keys.fill_(EMPTY_KEY)
      t.counts.zero_()
      if t.expiring:
        t.last_seen.zero_()
        t.freq.zero_()
        t.stats.zero_()
      if getattr(t, 'min_freq', 0):
        t.sketch.zero_()
        t.filter_counts.zero_()

  def launcher(hgl):
    return lambda: hgl._plan.launch(True, stream)

  t, early = {}, {}
  kinds = [('', False, False), ('x_', True, False)]
  if not args.entries_only:
    kinds += [('f_', False, True), ('xf_', True, True)]
  tables, hit, zf = {}, {}, {}
  for name, expiring, filtered in kinds:
    tables[name] = make(expiring, filtered)
    hit[name] = hb.embedding.HashGroupLookup(tables[name])
    for _ in range(min_freq if filtered else 1):
      hit[name](resident)
    assert all(x.size() == batch and x.failed() == 0 for x in tables[name])
    zf[name] = hb.embedding.HashGroupLookup(tables[name])
    zf[name](zipf)
  steady = {}
  for name, _, _ in kinds:
    steady[name + 'hit'] = launcher(hit[name])
    if not args.entries_only:
      steady[name + 'zipf'] = launcher(zf[name])
  for k in steady:
    t[k] = []
  for _ in range(args.rounds):
    for k in steady:   # alternating
      t[k].append(timed(steady[k]))
  if not args.entries_only:
    for name, _, filtered in kinds:
      x = tables[name]

      def counted(x=x, name=name):
        empty(x)
        hit[name]._plan.launch(True, stream)   # the first sighting: in the sketch, not in the table
      t[name + 'new'] = [timed_alone(lambda x=x: empty(x), launcher(hit[name])) for _ in range(args.rounds)]
      if filtered:
        # (width = capacity at this load: an id whose four cells all collide is admitted at first sight)
        assert all(y.size() + y.filtered() == batch for y in x)
        early[name + 'new_admitted_early'] = round(sum(y.size() for y in x) / (cols * batch), 4)
        t[name + 'again'] = [timed_alone(counted, launcher(hit[name])) for _ in range(args.rounds)]
      assert all(y.size() == batch and y.failed() == 0 for y in x)
      t[name + 'zipf_new'] = [timed_alone(lambda x=x: empty(x), launcher(zf[name])) for _ in range(args.rounds)]

  med = {k: float(np.median(v)) for k, v in t.items()}
  result = {'label': args.label, 'slab_size': slab_size,
            'shape': {'cols': cols, 'keys_per_col': batch, 'dim': dim, 'capacity': capacity, 'load': 0.5,
                      'sketch': [4, capacity], 'min_freq': min_freq}}
  result.update({k + '_us': round(v, 2) for k, v in med.items()})
  result.update({k + '_min_max_us': [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})
  if not args.entries_only:
    for pre, base in (('f_', ''), ('xf_', 'x_')):
      for k in ('hit', 'new', 'zipf', 'zipf_new'):
        result[f'{pre}{k}_over_{base}{k}'] = round(med[pre + k] / med[base + k], 4)
      result[f'{pre}again_over_{base}new'] = round(med[pre + 'again'] / med[base + 'new'], 4)
  result.update(early)
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  line = json.dumps(result)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
