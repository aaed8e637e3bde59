"""Hash-keyed 8-bit tables (HashTable(dtype='int8'), hbk_hash_insert_quant8_n) beside fp32 and bf16 tables, one
process, the forms taking turns, on the shape of profiles/hash_lowp.txt: 26 columns x 65 536 one-id int64 keys, tables
of 131 072 rows at load factor 0.5, slab_size 8.  For dim 16 / 64 / 128 and fp32 / bf16 / int8:

  first     the first batch: the tables emptied before every timed launch, so every key is a CAS and a row
            initialisation (int8: the amax butterfly and a divide per element); eager, each launch between its own events
  steady    every key resident: the translate alone, replays of a captured graph
  forward   translate (steady) + lookup, HashGroupLookup.launch(), replays of a captured graph

`--unchanged` measures only the fp32 and bf16 inserting entries (plain and expiring, first and steady, dim 16) and uses
nothing a checkout without 8-bit hash tables lacks: run from two checkouts taking turns it is the A/B that shows the
paths this change does not touch did not get slower.

Medians over `--rounds` rounds (7) with min / max; a round times every form once.  Prints one JSON line and appends it
to `--out`.

  python tools/bench_hash_quant8.py [--steps 30 --warmup 5 --rounds 7] [--unchanged] [--out profiles/hash_quant8.txt]
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


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--steps', type=int, default=30)
  p.add_argument('--warmup', type=int, default=5)
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--unchanged', action='store_true')
  p.add_argument('--label', default='')
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_quant8.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding.cache import EMPTY_KEY   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_quant8.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  rng = np.random.RandomState(777)
  resident = [torch.from_numpy(np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=BATCH + 64,
                                                     dtype=np.int64))[:BATCH].copy()).to(dev) for _ in range(COLS)]
  resident = [r[torch.randperm(BATCH, device=dev)] for r in resident]

  graphs = {}

  def replays(name, step):
    """us per replay of `step`, captured once per form: warm-up replays, then `--steps` replays between two events."""
    if name not in graphs:
      graphs[name] = torch.cuda.CUDAGraph()
      with torch.cuda.graph(graphs[name]):
        step()
    graph = graphs[name]
    for _ in range(args.warmup):
      graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
      graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps

  def alone(prepare, step, n=5):
    """Median over n eager launches, each behind its own `prepare` and between its own events."""
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
    """26 tables of one kind, filled to load 0.5, behind one HashGroupLookup bound to the resident batch."""

    def __init__(self, dim, **kw):
      self.tables = [hb.embedding.HashTable(CAPACITY, dim, dev, slab_size=SLAB, **kw) for _ in range(COLS)]
      self.hgl = hb.embedding.HashGroupLookup(self.tables)
      self.hgl(resident)
      assert all(t.size() == BATCH and t.failed() == 0 for t in self.tables)

    def empty(self):
      for t in self.tables:
        t.keys.fill_(EMPTY_KEY)
        t.counts.zero_()
        if t.expiring:
          t.stats.zero_()

    def translate(self):
      self.hgl._plan.launch(1, _lib.current_stream(dev))   # pylint: disable=protected-access

    def forms(self, name, forward=True):
      out = {name + '_first': lambda: alone(self.empty, self.translate),
             name + '_steady': lambda: replays(name + '_steady', self.translate)}
      if forward:
        out[name + '_forward'] = lambda: replays(name + '_forward', self.hgl.launch)
      return out

  if args.unchanged:
    plans = [(16, {f'{d}_{k}': dict(dtype=dt, expiring=k == 'expiring')
                   for d, dt in (('fp32', torch.float32), ('bf16', torch.bfloat16)) for k in ('plain', 'expiring')})]
  else:
    plans = [(dim, {'fp32': dict(dtype=torch.float32), 'bf16': dict(dtype=torch.bfloat16), 'int8': dict(dtype='int8')})
             for dim in (16, 64, 128)]
  times = {}
  for dim, kinds in plans:
    forms = {}
    for name, kw in kinds.items():
      forms.update(Group(dim, **kw).forms(f'dim{dim}_{name}', forward=not args.unchanged))
    for k in forms:
      times[k] = []
    for _ in range(args.rounds):
      for k, form in forms.items():   # taking turns; `first` leaves the tables resident again
        times[k].append(form())
    del forms
    graphs.clear()
    torch.cuda.empty_cache()
  result = {'label': args.label, 'shape': {'cols': COLS, 'keys_per_col': BATCH, 'capacity': CAPACITY, 'load': 0.5,
                                           'slab_size': SLAB}}
  if not args.unchanged:
    result['bytes_per_key'] = {f'dim{d}': {'fp32': 8 + 4 * d + 4 + 4, 'bf16': 8 + 2 * d + 4 + 4,
                                           'int8': 8 + (d + 3) // 4 * 4 + 4 + 4 + 4} for d in (16, 64, 128)}
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
