"""Removal by id (hbk_hash_remove_n) against what a caller had before it, in one process, on the shape of
tools/bench_hash_rehash.py: 26 expiring tables x 131 072 slots, slab_size 8, 65 536 resident keys each (load 0.5),
two dim-16 companions per table.

  cases   1 %, 10 % and 50 % of every table's keys named once each, and `10pct_x4`: the ids of the 10 % case, every
          one 4 times (shuffled)
  A       ONE hash_remove call over the 26 tables: a find and an erase launch
  find    the find launch alone (hash_translate with insert=False over the 26 tables): A's first launch
  graphs  A and the find alone, each captured into a graph and replayed: the same launches without the host's share
          (describing 26 tables in Python).  The erase launch cannot be launched alone -- the two are one C call --
          so its time is the replay of A less the replay of the find, medians of the rounds
  B       find (one launch for the 26 tables) plus torch indexing stores per table: TOMBSTONE into the keys, zeros
          into last_seen and freq, the fill values into the companion rows, at the found slots

Every timed region is one operation between its own HIP events with the tables restored before it; `--rounds`
rounds with the two forms taking turns; medians with min / max.  Bytes of A (the model of include/hbk.h): per
occurrence the 8 B id, a 64 B slab read and an 8 B slot store in the find, the 8 B id and the 8 B slot again in the
erase; per removed key the 8 B swap, 8 B of metadata and the fill bytes (2 x 64 B).  TB/s over the whole call, over
the find's own bytes for the find alone, and over the erase's own bytes for the difference of the replays.
Prints one JSON line and appends it to `--out` (default profiles/hash_remove.txt).

  python tools/bench_hash_remove.py [--rounds 7]
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
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--cols', type=int, default=26)
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_remove.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding.hashtable import TOMBSTONE_KEY   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_remove.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  cols, batch, dim, slab_size = args.cols, 65536, 16, 8
  capacity = 2 * batch
  rng = np.random.RandomState(779)

  def distinct(n):
    return torch.from_numpy(np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n + 64, dtype=np.int64))[:n]
                            .copy()).to(dev)
  resident = [distinct(batch)[torch.randperm(batch, device=dev)].contiguous() for _ in range(cols)]
  tables = [hb.embedding.HashTable(capacity, dim, dev, slab_size=slab_size, expiring=True) for _ in range(cols)]
  comps = []
  for x, r in zip(tables, resident):
    x.set_step(7)
    where = x.lookup_or_insert(r)
    assert x.size() == batch and x.failed() == 0
    a, b = torch.full((capacity, dim), 0.1, device=dev), torch.zeros((capacity, dim), device=dev)
    a[where] = torch.rand((batch, dim), device=dev) + 1
    b[where] = torch.randn((batch, dim), device=dev)
    comps.append([(a, 0.1), (b, 0.0)])
  NAMES = ('keys', 'last_seen', 'freq', 'stats')
  saved = [({n: getattr(x, n).clone() for n in NAMES}, [c.clone() for c, _ in cs]) for x, cs in zip(tables, comps)]

  def restore():
    for x, cs, (state, cc) in zip(tables, comps, saved):
      for n in NAMES:
        getattr(x, n).copy_(state[n])
      for (c, _), s in zip(cs, cc):
        c.copy_(s)

  def once(step):
    restore()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3

  def summary(us, nbytes=None):
    med = float(np.median(us))
    out = {'us': round(med, 2), 'min_max_us': [round(min(us), 2), round(max(us), 2)]}
    if nbytes is not None:
      out['TBps'] = round(nbytes / med * 1e-6, 3)
    return out

  result = {'shape': {'cols': cols, 'slots_per_col': capacity, 'keys_per_col': batch, 'slab_size': slab_size,
                      'companions': 2, 'companion_dim': dim}, 'rounds': args.rounds}
  for name, share, times in (('1pct', 0.01, 1), ('10pct', 0.10, 1), ('50pct', 0.50, 1), ('10pct_x4', 0.10, 4)):
    k = int(batch * share)
    ids = [r[:k].repeat(times)[torch.randperm(k * times, device=dev)].contiguous() for r in resident]
    outs = [torch.empty(k * times, dtype=torch.int64, device=dev) for _ in range(cols)]

    def form_a():
      hb.embedding.hash_remove(tables, ids, comps, outs)

    def form_b():
      slots = hb.embedding.hash_translate(tables, ids, insert=False, outs=outs)
      for x, s, cs in zip(tables, slots, comps):
        s = s[s >= 0]
        x.keys[s] = TOMBSTONE_KEY
        x.last_seen[s] = 0
        x.freq[s] = 0
        for c, v in cs:
          c[s] = v

    def find_alone():
      hb.embedding.hash_translate(tables, ids, insert=False, outs=outs)
    forms = {'A_hash_remove': form_a, 'find_alone': find_alone, 'B_find_and_torch_stores': form_b}
    for step in (form_a, find_alone):   # (before the captures: every allocation and first launch is behind us)
      once(step)
    graphs = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      for f, step in (('A_graph', form_a), ('find_graph', find_alone)):
        graphs[f] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[f], stream=side):
          step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    forms['A_graph'] = graphs['A_graph'].replay
    forms['find_graph'] = graphs['find_graph'].replay
    t = {f: [] for f in forms}
    for f, step in forms.items():   # one untimed pass of everything: allocator, first launches
      once(step)
    for _ in range(args.rounds):
      for f, step in forms.items():   # taking turns
        t[f].append(once(step))
    # every form leaves the same table behind
    after = {}
    for f, step in forms.items():
      if f in ('find_alone', 'find_graph'):
        continue
      once(step)
      after[f] = [x.keys.clone() for x in tables] + [x.freq.clone() for x in tables] + [c.clone() for cs in comps
                                                                                        for c, _ in cs]
      assert all(int((x.keys == TOMBSTONE_KEY).sum().item()) == k for x in tables)
    first = after['A_hash_remove']
    assert all(torch.equal(a, b) for other in after.values() for a, b in zip(first, other))
    occ, gone = cols * k * times, cols * k
    nbytes = occ * (8 + 64 + 8 + 8 + 8) + gone * (8 + 8 + 2 * 4 * dim)
    case = {'occurrences_per_col': k * times, 'removed_per_col': k, 'bytes_per_call': nbytes,
            'A_hash_remove': summary(t['A_hash_remove'], nbytes),
            'find_alone': summary(t['find_alone'], occ * (8 + 64 + 8)),
            'B_find_and_torch_stores': summary(t['B_find_and_torch_stores'])}
    erase_us = float(np.median(t['A_graph'])) - float(np.median(t['find_graph']))
    erase_bytes = occ * 16 + gone * (8 + 8 + 2 * 4 * dim)
    case['A_graph'] = summary(t['A_graph'], nbytes)
    case['find_graph'] = summary(t['find_graph'], occ * (8 + 64 + 8))
    case['erase_by_difference'] = {'us': round(erase_us, 2), 'bytes': erase_bytes,
                                   'TBps': round(erase_bytes / erase_us * 1e-6, 3) if erase_us > 0 else None}
    case['B_over_A'] = round(case['B_find_and_torch_stores']['us'] / case['A_hash_remove']['us'], 2)
    result[name] = case
  line = json.dumps(result)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
