"""The hash table's find-or-insert (hbk_hash_insert_n) in one process, forms alternating, on config 2's
shape: 26 columns x 65 536 one-id int64 keys, dim 16, every table at load factor 0.5 (65 536 resident keys
in 131 072 rows), for slab_size 8 / 16 / 32 / 64.

  hit            (a) the steady state: every key of the batch is resident (no CAS is issued)
  miss           (b) the first batch: every key is new (tables emptied before every timed launch)
  zipf           (c) a Zipf(1.2) batch over the resident keys (duplicates inside the batch)
  zipf_first     (c') the same batch into empty tables: inserts with duplicates racing
  find           insert = 0 on the batch of (a)
  hit_lookup     translate (a) + GroupLookup over the row numbers (HashGroupLookup.launch)
  bucketed       GroupLookup with buckets = capacity on the raw ids: the forward this one is set beside

and, as the yardstick of (a), on ONE table of 26 x 65 536 keys (the probe takes one column per launch):

  ab_probe       hbk_cache_probe on that table and its keys
  ab_hit         hbk_hash_insert_n, insert = 1, the same table and keys (all hits)
  ab_find        hbk_hash_insert_n, insert = 0

Timing follows tools/bench_sequence.py: warm-up steps, then `--steps` steps between HIP events, `--rounds`
rounds with the forms taking turns; medians with min / max.  `miss` and `zipf_first` empty the tables
before each launch, so each of their steps is timed alone between its own pair of events.  Prints one JSON
line per slab size and appends it to `--out` (default profiles/hash_insert.txt).

  python tools/bench_hash_insert.py [--steps 50 --warmup 10 --rounds 5]
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
  p.add_argument('--steps', type=int, default=50)
  p.add_argument('--warmup', type=int, default=10)
  p.add_argument('--rounds', type=int, default=5)
  p.add_argument('--slab-sizes', default='8,16,32,64')
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_insert.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding.cache import EMPTY_KEY   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_insert.py measures on a GPU: none found')
  lib = _lib.lib()
  dev = torch.device('cuda:0')
  cols, batch, dim = 26, 65536, 16
  capacity = 2 * batch
  rng = np.random.RandomState(777)
  # distinct resident keys per column; the Zipf batch names them by rank
  resident = [torch.from_numpy(np.unique(rng.randint(-2 ** 63 + 1, 2 ** 63 - 1, size=batch + 64,
                                                     dtype=np.int64))[:batch].copy()).to(dev)
              for _ in range(cols)]
  resident = [r[torch.randperm(batch, device=dev)] for r in resident]
  zipf = [r[torch.from_numpy((rng.zipf(1.2, size=batch) - 1) % batch).to(dev)] for r in resident]
  stream = _lib.current_stream(dev)

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

  def timed_alone(prepare, step, n):
    """Median over n launches, each behind its own `prepare` and between its own events."""
    out = []
    for _ in range(n):
      prepare()
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      step(0)
      e1.record()
      e1.synchronize()
      out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out))

  for slab_size in [int(x) for x in args.slab_sizes.split(',')]:
    tables = [hb.embedding.HashTable(capacity, dim, dev, slab_size=slab_size) for _ in range(cols)]

    def empty():
      for t in tables:
        t.keys.fill_(EMPTY_KEY)
        t.counts.zero_()
    hit = hb.embedding.HashGroupLookup(tables)
    outs = hit(resident)                                   # fills the tables: load factor 0.5
    assert all(t.size() == batch and t.failed() == 0 for t in tables)
    find = hb.embedding.HashGroupLookup(tables, train=False)
    find(resident)
    for a, b in zip(hit.slots, find.slots):
      assert torch.equal(a, b)
    zf = hb.embedding.HashGroupLookup(tables)
    zf(zipf)
    bucketed = hb.embedding.GroupLookup([t.table for t in tables], buckets=[capacity] * cols)
    bucketed(resident, None, [torch.empty_like(o) for o in outs])

    def translate(obj, insert):
      def step(i):   # pylint: disable=unused-argument
        obj._plan.launch(insert, stream)   # plain tables alone: one hbk_hash_insert_n
      return step
    steps = {'hit': translate(hit, 1), 'zipf': translate(zf, 1), 'find': translate(find, 0),
             'hit_lookup': lambda i: hit.launch(), 'bucketed': lambda i: bucketed.launch()}
    t = {k: [] for k in steps}
    for _ in range(args.rounds):
      for k in steps:   # alternating
        t[k].append(timed(steps[k]))
    t['miss'] = [timed_alone(empty, translate(hit, 1), 5) for _ in range(args.rounds)]
    assert all(x.size() == batch for x in tables)
    t['zipf_first'] = [timed_alone(empty, translate(zf, 1), 5) for _ in range(args.rounds)]
    empty()
    hit.launch()                                           # resident again for the A/B below
    del tables, hit, find, zf, bucketed, outs

    # the yardstick of (a): one table of cols * batch keys, probe / insert (all hits) / find taking turns
    n = cols * batch
    big = hb.embedding.HashTable(2 * n, dim, dev, slab_size=slab_size)
    keys = torch.cat(resident)
    slots = big.lookup_or_insert(keys)
    assert big.size() == torch.unique(keys).numel() and big.failed() == 0
    hit_slot = torch.empty_like(slots)
    col = (_lib.HashColumn * 1)()
    big._describe(col[0])
    col[0].keys, col[0].n_keys, col[0].slots = keys.data_ptr(), n, slots.data_ptr()

    def ab_probe(i):   # pylint: disable=unused-argument
      _lib.check(lib.hbk_cache_probe(C.c_void_p(big.keys.data_ptr()), C.c_int64(big.slab_count),
                                     C.c_int32(slab_size), C.c_void_p(keys.data_ptr()), C.c_int64(n),
                                     C.c_void_p(hit_slot.data_ptr()), None, stream))
    ab = {'ab_probe': ab_probe, 'ab_hit': lambda i: _lib.check(lib.hbk_hash_insert_n(1, col, 1, stream)),
          'ab_find': lambda i: _lib.check(lib.hbk_hash_insert_n(1, col, 0, stream))}
    ab_probe(0)
    ab['ab_hit'](0)
    assert torch.equal(hit_slot, slots)
    for k in ab:
      t[k] = []
    for _ in range(args.rounds):
      for k in ab:
        t[k].append(timed(ab[k]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    result = {'slab_size': slab_size,
              'shape': {'cols': cols, 'keys_per_col': batch, 'dim': dim, 'capacity': capacity, 'load': 0.5}}
    result.update({k + '_us': round(v, 2) for k, v in med.items()})
    result.update({k + '_min_max_us': [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})
    result['hit_lookup_over_bucketed'] = round(med['hit_lookup'] / med['bucketed'], 4)
    result['ab_hit_over_probe'] = round(med['ab_hit'] / med['ab_probe'], 4)
    result['ab_find_over_probe'] = round(med['ab_find'] / med['ab_probe'], 4)
    result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
      f.write(line + '\n')
    del big, keys, slots, hit_slot
    torch.cuda.empty_cache()


if __name__ == '__main__':
  main()
