"""Hash-keyed 16-bit tables (HashTable(dtype=), hbk_hash_insert_lowp_n) beside their fp32 twins, one process, the
forms taking turns, on the shape of profiles/hash_insert.txt: 26 columns x 65 536 one-id int64 keys, tables of
131 072 rows at load factor 0.5, slab_size 8.

  translate   dim 16, fp32 / bf16 / fp16:  hit (every key resident), miss (the first batch: tables emptied before every
              timed launch, so CAS + row initialisation), zipf (a Zipf(1.2) batch over the resident keys)
  forward     dim 16 / 64 / 128, fp32 / bf16 / fp16: translate (hit) + lookup, HashGroupLookup.launch()
  rehash      dim 16, fp32 / bf16: hash_rehash of the 26 tables to twice the capacity (allocation included: the call)
  bytes       per key with row-wise Adagrad: key 8 + row + last_seen 4 + accumulator 4

`--fp32-entries` measures only the four fp32 translate entries (plain, expiring, filtered, expiring + filtered), hit
and miss, and uses nothing a checkout without 16-bit hash tables lacks: run from two checkouts taking turns it is the
A/B that shows the fp32 translate did not get slower.

Timing follows tools/bench_hash_insert.py: warm-up steps, then `--steps` steps between HIP events, `--rounds` rounds
with the forms taking turns; medians with min / max.  Prints one JSON line and appends it to `--out`.

  python tools/bench_hash_lowp.py [--steps 30 --warmup 5 --rounds 7] [--fp32-entries] [--out profiles/hash_lowp.txt]
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

COLS, BATCH, SLAB = 26, 65536, 8
CAPACITY = 2 * BATCH
ENTRIES = {'plain': {}, 'expiring': dict(expiring=True), 'filtered': dict(min_freq=1),
           'expiring_filtered': dict(expiring=True, min_freq=1)}


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--steps', type=int, default=30)
  p.add_argument('--warmup', type=int, default=5)
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--fp32-entries', action='store_true')
  p.add_argument('--label', default='')
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_lowp.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding.cache import EMPTY_KEY   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_lowp.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  rng = np.random.RandomState(777)
  resident = [torch.from_numpy(np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=BATCH + 64,
                                                     dtype=np.int64))[:BATCH].copy()).to(dev) for _ in range(COLS)]
  resident = [r[torch.randperm(BATCH, device=dev)] for r in resident]
  zipf = [r[torch.from_numpy((rng.zipf(1.2, size=BATCH) - 1) % BATCH).to(dev)] for r in resident]
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
    """Median over n launches, each behind its own `prepare` and between its own events."""
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

  class Group:
    """26 tables of one kind, filled to load 0.5, with the translate of the resident and of the Zipf batch."""

    def __init__(self, dim, **kw):
      self.tables = [hb.embedding.HashTable(CAPACITY, dim, dev, slab_size=SLAB, **kw) for _ in range(COLS)]
      self.hit = hb.embedding.HashGroupLookup(self.tables)
      self.hit(resident)
      assert all(t.size() == BATCH and t.failed() == 0 for t in self.tables)
      self.zipf = hb.embedding.HashGroupLookup(self.tables)
      self.zipf(zipf)

    def empty(self):
      for t in self.tables:
        t.keys.fill_(EMPTY_KEY)
        t.counts.zero_()
        if t.expiring:
          t.stats.zero_()
        if t.min_freq:
          t.sketch.zero_()

    def steps(self, name):
      translate = lambda: self.hit._plan.launch(1, stream)   # noqa: E731
      return {name + '_hit': translate, name + '_zipf': lambda: self.zipf._plan.launch(1, stream)}, \
          {name + '_miss': (self.empty, translate)}

  def measure(turns, alone):
    t = {k: [] for k in list(turns) + list(alone)}
    for _ in range(args.rounds):
      for k, step in turns.items():   # taking turns
        t[k].append(timed(step))
      for k, (prepare, step) in alone.items():
        t[k].append(timed_alone(prepare, step))
    return t

  result = {'label': args.label, 'shape': {'cols': COLS, 'keys_per_col': BATCH, 'capacity': CAPACITY, 'load': 0.5,
                                           'slab_size': SLAB}}
  times = {}
  if args.fp32_entries:
    turns, alone = {}, {}
    groups = [Group(16, **kw) for kw in ENTRIES.values()]
    for name, g in zip(ENTRIES, groups):
      a, b = g.steps(name)
      a.pop(name + '_zipf')
      turns.update(a)
      alone.update(b)
    times.update(measure(turns, alone))
  else:
    dtypes = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
    turns, alone = {}, {}
    groups = {name: Group(16, dtype=d) for name, d in dtypes.items()}
    for name, g in groups.items():
      a, b = g.steps('translate_' + name)
      turns.update(a)
      alone.update(b)
    times.update(measure(turns, alone))
    for dim in (16, 64, 128):
      fwd = {name: (groups[name] if dim == 16 else Group(dim, dtype=d)) for name, d in dtypes.items()}
      for g in fwd.values():
        g.hit(resident)   # (resident again after the misses) binds the lookup
      times.update(measure({f'forward_dim{dim}_{name}': g.hit.launch for name, g in fwd.items()}, {}))
      del fwd
      torch.cuda.empty_cache()
    # growth: every round rehashes fresh tables of load 0.5 to twice the capacity
    del groups
    torch.cuda.empty_cache()
    for name in ('fp32', 'bf16'):
      times['rehash_' + name] = []
    for _ in range(args.rounds):
      for name in ('fp32', 'bf16'):
        g = Group(16, dtype=dtypes[name])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hb.embedding.hash_rehash(g.tables, [2 * CAPACITY] * COLS)
        e1.record()
        e1.synchronize()
        times['rehash_' + name].append(e0.elapsed_time(e1) * 1e3)
        assert all(t.size() == BATCH and t.capacity == 2 * CAPACITY for t in g.tables)
        del g
    result['bytes_per_key'] = {f'dim{d}': {'fp32': 8 + 4 * d + 4 + 4, '16-bit': 8 + 2 * d + 4 + 4}
                               for d in (16, 64, 128)}
  result.update({k + '_us': round(float(np.median(v)), 2) for k, v in times.items()})
  result.update({k + '_min_max_us': [round(min(v), 2), round(max(v), 2)] for k, v in times.items()})
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  line = json.dumps(result)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
