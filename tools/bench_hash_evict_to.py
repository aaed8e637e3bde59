"""Bounded hash tables (hbk_hash_evict_to_n) in one process, the forms taking turns, on the shape of
tools/bench_hash_expiry.py and tools/bench_hash_rehash.py: 26 expiring tables x 131 072 slots, dim 16, slab_size 8,
65 536 keys each, two dim-16 companions per table; last_seen spread evenly over 64 steps.

Per target (75 % / 50 % / 10 % of the live keys stay), every call on freshly restored tables and timed between
its own events as a user makes it (the Python descriptors included, in every form), medians of 7:
  evict_to      hbk_hash_evict_to_n over the 26 tables: three histogram passes, their picks and the sweep
  floor         hbk_hash_evict_n with the steps_to_live that evicts the same keys: the sweep alone, the threshold
                known in advance
  torch         what a user writes without the entry: torch.kthvalue of last_seen[live] per table, ONE host read of
                the 26 thresholds, then hbk_hash_evict_n per threshold group
and once:
  first_pass    hbk_hash_evict_to_n with max_size = the live keys (need = 0): the first histogram pass and its pick;
                every later launch leaves at once.  us, and TB/s over its byte model, 16 B per slot.

Prints one JSON line and appends it to `--out` (default profiles/hash_evict_to.txt).

  python tools/bench_hash_evict_to.py [--repeats 7]
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
  p.add_argument('--repeats', type=int, default=7)
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_evict_to.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding import hash_evict, hash_evict_to   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_evict_to.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  cols, batch, dim, slab_size, n_steps = 26, 65536, 16, 8, 64
  capacity = 2 * batch
  rng = np.random.RandomState(778)
  tables = [hb.embedding.HashTable(capacity, dim, dev, slab_size=slab_size, expiring=True) for _ in range(cols)]
  for t in tables:
    keys = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=batch + 64, dtype=np.int64))[:batch]
    t.set_step(1)
    slots = t.lookup_or_insert(torch.from_numpy(keys.copy()).to(dev))
    assert t.size() == batch and t.failed() == 0
    # 1024 keys per step, steps 1..64
    t.last_seen[slots] = torch.from_numpy((rng.permutation(batch) % n_steps + 1).astype(np.int32)).to(dev)
    t.set_step(n_steps)
  comps = [[(torch.full((capacity, dim), 0.1, device=dev), 0.1), (torch.zeros((capacity, dim), device=dev), 0.0)]
           for _ in range(cols)]
  saved = [(t.keys.clone(), t.last_seen.clone(), t.freq.clone()) for t in tables]
  reports = [torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(cols)]

  def restore():
    for t, (k, s, f) in zip(tables, saved):
      t.keys.copy_(k)
      t.last_seen.copy_(s)
      t.freq.copy_(f)
      t.stats.zero_()

  def timed_alone(step):
    restore()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3

  def torch_form(max_size):
    # the threshold by a selection in torch, read on the host, then the sweep that exists
    cuts = []
    for t in tables:
      ages = t.last_seen[t._live()]   # pylint: disable=protected-access
      need = ages.numel() - max_size
      cuts.append(torch.kthvalue(ages, need).values if need > 0 else torch.full((), -1, dtype=torch.int32, device=dev))
    cuts = torch.stack(cuts).tolist()
    for cut in sorted(set(cuts)):
      if cut >= 0:
        group = [c for c in range(cols) if cuts[c] == cut]
        hash_evict([tables[c] for c in group], n_steps - cut, 0, [comps[c] for c in group])

  result = {'shape': {'cols': cols, 'keys_per_col': batch, 'dim': dim, 'capacity': capacity, 'slab_size': slab_size,
                      'steps': n_steps}, 'repeats': args.repeats}
  for pct in (75, 50, 10):
    max_size = batch * pct // 100
    cut = n_steps - n_steps * pct // 100          # the steps 1..cut leave: the first whole steps that cover the need
    forms = {'evict_to': lambda m=max_size: hash_evict_to(tables, m, 0, comps, reports),
             'floor': lambda c=cut: hash_evict(tables, n_steps - c, 0, comps),
             'torch': lambda m=max_size: torch_form(m)}
    for f in forms.values():   # warm-up: descriptors, scratch, kernels loaded
      timed_alone(f)
    us = {k: [] for k in forms}
    for _ in range(args.repeats):
      for k, f in forms.items():   # taking turns
        us[k].append(timed_alone(f))
        evicted = sum(t.evicted() for t in tables)
        assert evicted == cols * cut * (batch // n_steps), (pct, k, evicted)   # whole steps leave
    result[f'to_{pct}pct'] = {'max_size': max_size, 'evicted': cols * cut * (batch // n_steps)}
    for k, v in us.items():
      result[f'to_{pct}pct'][k + '_us'] = round(float(np.median(v)), 2)
      result[f'to_{pct}pct'][k + '_min_max_us'] = [round(min(v), 2), round(max(v), 2)]
  first = [timed_alone(lambda: hash_evict_to(tables, batch, 0, comps, reports)) for _ in range(args.repeats + 1)][1:]
  assert sum(t.evicted() for t in tables) == 0
  med = float(np.median(first))
  nbytes = cols * capacity * 16
  result['first_pass'] = {'us': round(med, 2), 'min_max_us': [round(min(first), 2), round(max(first), 2)],
                          'bytes': nbytes, 'TBps': round(nbytes / med * 1e-6, 3)}
  line = json.dumps(result)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
