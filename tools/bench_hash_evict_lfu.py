"""Bounded hash tables in LFU order (hbk_hash_evict_to_lfu_n / _select_n, hbk_hash_spill_lfu_n) in one process, the
forms taking turns, on the shape of profiles/hash_rehash.txt: 26 expiring tables x 131 072 slots, dim 16, slab_size 8,
load 0.75 (98 304 keys each), bound 0.5 x capacity, two dim-16 companions per table; freq Zipf-distributed (most
keys seen once or twice), last_seen spread over 64 steps.  The arrays are written directly: no call here looks at
where a key hashes to.

Every call on freshly restored tables and timed between its own events as a user makes it (the Python descriptors
included, in every form), medians of 7:
  evict_lfu     hash_evict_to(order='lfu'): the clear launch, six histogram passes, their picks and the sweep
  select_lfu    hash_evict_to_select(order='lfu'): the same without the sweep
  spill_lfu     hash_spill(order='lfu'): the select, a host read, the export's count / scan / write and the sweep
  evict_lru     hash_evict_to(order='lru') on the same state: three passes and the sweep
  select_lru    hash_evict_to_select(order='lru')
  spill_lru     hash_spill(order='lru')
  torch         what a user writes without the entry: per table a torch.sort of (freq << 32 | last_seen) over the
                live slots, ONE host read of the 26 cuts, then an indexing sweep (keys, last_seen, freq, companions)
With 26 tables the calls above are bound by the host (the descriptors of 26 tables in Python), so the device side is
timed on its own: the four capturable forms and, per order, first_pass -- the call with max_size = the live keys
(need = 0: the clear launch, the first histogram pass and its pick; every later launch leaves at once) -- are
captured into a graph each and the REPLAY is timed the same way (`graph` in the result).
Byte model: 16 B per slot per histogram pass (and per sweep).  TB/s figures, all from the replays and all whole-call
rates over the byte model, launch gaps included: first_pass over one pass; the select over its six (LFU) or three
(LRU) passes; the sweep as (evict - select) over one.  Per-kernel times come from a kernel trace, not from here.

Prints one JSON line and appends it to `--out` (default profiles/hash_evict_lfu.txt).

  python tools/bench_hash_evict_lfu.py [--repeats 7]
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
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_evict_lfu.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding import hash_evict_to, hash_evict_to_select, hash_spill   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding.hashtable import TOMBSTONE_KEY   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_evict_lfu.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  cols, capacity, dim, slab_size, n_steps = 26, 131072, 16, 8, 64
  n_keys, max_size = capacity * 3 // 4, capacity // 2
  rng = np.random.RandomState(779)
  tables = [hb.embedding.HashTable(capacity, dim, dev, slab_size=slab_size, expiring=True) for _ in range(cols)]
  for t in tables:
    where = torch.from_numpy(rng.permutation(capacity)[:n_keys]).to(dev)
    keys = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n_keys + 64, dtype=np.int64))[:n_keys]
    t.keys[where] = torch.from_numpy(keys.copy()).to(dev)
    t.freq[where] = torch.from_numpy(np.minimum(rng.zipf(1.6, size=n_keys), 2 ** 30).astype(np.int32)).to(dev)
    t.last_seen[where] = torch.from_numpy(rng.randint(1, n_steps + 1, size=n_keys).astype(np.int32)).to(dev)
    t.set_step(n_steps)
    t.recount()
  comps = [[(torch.full((capacity, dim), 0.1, device=dev), 0.1), (torch.zeros((capacity, dim), device=dev), 0.0)]
           for _ in range(cols)]
  saved = [(t.keys.clone(), t.last_seen.clone(), t.freq.clone()) for t in tables]
  reports = {'lfu': [torch.zeros(8, dtype=torch.int32, device=dev) for _ in range(cols)],
             'lru': [torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(cols)]}

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

  def torch_form():
    # the cut by a sort in torch, read on the host, then the sweep by indexing
    order, cuts = [], []
    for t in tables:
      k = (t.freq.to(torch.int64) << 32) | t.last_seen.to(torch.int64)   # (both >= 0 here)
      live = t._live()   # pylint: disable=protected-access
      ks = torch.sort(k[live]).values
      need = ks.numel() - max_size
      order.append((k, live))
      cuts.append(ks[need - 1] if need > 0 else torch.full((), -1, dtype=torch.int64, device=dev))
    cuts = torch.stack(cuts).tolist()
    for t, (k, live), cut, pairs in zip(tables, order, cuts, comps):
      mask = live & (k <= cut)
      t.stats[0] += mask.sum().to(torch.int32)
      t.keys[mask] = TOMBSTONE_KEY
      t.last_seen[mask] = 0
      t.freq[mask] = 0
      for x, value in pairs:
        x[mask] = value

  forms = {'evict_lfu': lambda: hash_evict_to(tables, max_size, 0, comps, reports['lfu'], order='lfu'),
           'select_lfu': lambda: hash_evict_to_select(tables, max_size, 0, reports['lfu'], order='lfu'),
           'spill_lfu': lambda: hash_spill(tables, max_size, 0, comps, order='lfu'),
           'evict_lru': lambda: hash_evict_to(tables, max_size, 0, comps, reports['lru'], order='lru'),
           'select_lru': lambda: hash_evict_to_select(tables, max_size, 0, reports['lru'], order='lru'),
           'spill_lru': lambda: hash_spill(tables, max_size, 0, comps, order='lru'),
           'torch': torch_form}
  evicted = {}
  for k, f in forms.items():   # warm-up: descriptors, scratch, kernels loaded
    timed_alone(f)
    evicted[k] = sum(t.evicted() for t in tables)
  # the LFU forms and the torch composition take out the same number of keys; the selects take out none
  assert evicted['evict_lfu'] == evicted['spill_lfu'] == evicted['torch'] >= cols * (n_keys - max_size), evicted
  assert evicted['select_lfu'] == evicted['select_lru'] == 0
  assert evicted['evict_lru'] == evicted['spill_lru'] >= cols * (n_keys - max_size), evicted
  us = {k: [] for k in forms}
  for _ in range(args.repeats):
    for k, f in forms.items():   # taking turns
      us[k].append(timed_alone(f))
  first = {}
  for order in ('lfu', 'lru'):
    runs = [timed_alone(lambda o=order: hash_evict_to(tables, n_keys, 0, comps, reports[o], order=o))
            for _ in range(args.repeats + 1)][1:]
    assert sum(t.evicted() for t in tables) == 0
    first[order] = runs
  # the device side alone: the capturable forms as graph replays
  def captured(step):
    restore()
    step()   # (outside the capture: the scratch exists)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
      with torch.cuda.graph(graph, stream=s):
        step()
    torch.cuda.synchronize()
    return graph
  graphs = {k: captured(forms[k]) for k in ('evict_lfu', 'select_lfu', 'evict_lru', 'select_lru')}
  for order in ('lfu', 'lru'):
    graphs['first_pass_' + order] = captured(
      lambda o=order: hash_evict_to(tables, n_keys, 0, comps, reports[o], order=o))
  for k, g in graphs.items():
    timed_alone(g.replay)
    assert sum(t.evicted() for t in tables) == evicted.get(k, 0), k   # a replay does what the call did
  graph_us = {k: [] for k in graphs}
  for _ in range(args.repeats):
    for k, g in graphs.items():   # taking turns
      graph_us[k].append(timed_alone(g.replay))
  pass_bytes = cols * capacity * 16
  med = {k: float(np.median(v)) for k, v in us.items()}
  fp = {k: float(np.median(v)) for k, v in first.items()}
  gmed = {k: float(np.median(v)) for k, v in graph_us.items()}

  def tbps(nbytes, t_us):
    return round(nbytes / t_us * 1e-6, 3) if t_us > 0 else None
  result = {'shape': {'cols': cols, 'slots_per_col': capacity, 'keys_per_col': n_keys, 'max_size': max_size,
                      'dim': dim, 'slab_size': slab_size, 'companions': 2, 'steps': n_steps, 'freq': 'zipf(1.6)'},
            'repeats': args.repeats, 'evicted': evicted, 'pass_bytes': pass_bytes}
  for k, v in us.items():
    result[k] = {'us': round(med[k], 2), 'min_max_us': [round(min(v), 2), round(max(v), 2)]}
  for order in ('lfu', 'lru'):
    result['first_pass_' + order] = {'us': round(fp[order], 2),
                                     'min_max_us': [round(min(first[order]), 2), round(max(first[order]), 2)]}
  result['evict_lfu_over_evict_lru'] = round(med['evict_lfu'] / med['evict_lru'], 3)
  result['torch_over_evict_lfu'] = round(med['torch'] / med['evict_lfu'], 2)
  graph = {}
  for k, v in graph_us.items():
    graph[k] = {'us': round(gmed[k], 2), 'min_max_us': [round(min(v), 2), round(max(v), 2)]}
  for order, passes in (('lfu', 6), ('lru', 3)):
    graph['first_pass_' + order]['TBps'] = tbps(pass_bytes, gmed['first_pass_' + order])
    graph['select_' + order].update(passes=passes, TBps=tbps(passes * pass_bytes, gmed['select_' + order]))
    sweep = gmed['evict_' + order] - gmed['select_' + order]
    graph['sweep_' + order] = {'us': round(sweep, 2), 'TBps': tbps(pass_bytes, sweep)}
  graph['select_lfu_over_select_lru'] = round(gmed['select_lfu'] / gmed['select_lru'], 3)
  graph['evict_lfu_over_evict_lru'] = round(gmed['evict_lfu'] / gmed['evict_lru'], 3)
  result['graph'] = graph
  line = json.dumps(result)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
