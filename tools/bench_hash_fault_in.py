"""The batched fault-in (hash_fault_in over hbk_hash_missing_n) against the per-table HashTable.fault_in loop, in one
process, on the shape of tools/bench_hash_rehash.py: 26 expiring tables x 131 072 slots, slab_size 8, dim 16, two
dim-16 companions per table, 65 536 keys per table of which the older half was spilled into the table's
HashSpillStore; 65 536 ids per column and step.

  cases     0 %, 1 %, 10 % and 100 % of a column's id occurrences name spilled keys (the others resident ones), and
            `zipf`: ranks drawn Zipf(1.2) over the table's 65 536 keys in a random order (half of them spilled)
  batched   hash_fault_in(tables, ids, stores, companions): ONE hbk_hash_missing_n call, one read of the counts, one
            copy of the missed ids, then store.take / import_items per table
  loop      [t.fault_in(ids_c, store_c, companions_c) for every table]: a find, a boolean index, a torch.unique and
            a .cpu() per table, then the same take / import
  missing   hash_missing alone (the C call, the allocation of its outputs and the one host read)
  graphs    the hbk_hash_missing_n call and the find alone (hash_translate, insert=False), each captured into a graph
            and replayed: the launches without the host's share.  Claim and compaction = the difference of the medians.

batched / loop / missing are wall-clock times between two device synchronisations (the host tier is host work);
the replays are timed between HIP events.  Tables, companions and stores are restored before every timed run;
`--rounds` rounds with the forms taking turns; medians with min / max.

Byte model of the C call (include/hbk.h), stated, not compared with HBM: the find reads per position the 8 B id and
a 64 B slab and stores an 8 B slot; claim and compaction read the 8 B slot per position three times (claim, count,
write), and per missed occurrence the 8 B id three times, an 8 B cell three times and 4 B of first[] twice, plus one
4 B atomic; per distinct miss 8 B are written; the clear writes 12 B per cell.  TB/s over these bytes.
Prints one JSON line and appends it to `--out` (default profiles/hash_fault_in.txt).

  python tools/bench_hash_fault_in.py [--rounds 7]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--cols', type=int, default=26)
  p.add_argument('--cases', default='0pct,1pct,10pct,100pct,zipf')
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_fault_in.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_fault_in.py measures on a GPU: none found')
  E = hb.embedding
  dev = torch.device('cuda:0')
  cols, batch, dim, slab_size = args.cols, 65536, 16, 8
  capacity, half = 2 * batch, batch // 2
  rng = np.random.RandomState(781)

  def distinct(n):
    k = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n + 64, dtype=np.int64))
    rng.shuffle(k)
    return k[:n].copy()
  keys = [distinct(batch) for _ in range(cols)]           # [:half] spilled, [half:] resident
  tables = [E.HashTable(capacity, dim, dev, slab_size=slab_size, expiring=True) for _ in range(cols)]
  comps, stores = [], []
  for t, k in zip(tables, keys):
    for step, part in ((1, k[:half]), (2, k[half:])):
      t.set_step(step)
      where = t.lookup_or_insert(torch.from_numpy(part).to(dev))
    assert t.size() == batch and t.failed() == 0
    a, b = torch.full((capacity, dim), 0.1, device=dev), torch.zeros((capacity, dim), device=dev)
    a[where] = torch.rand((half, dim), device=dev) + 1
    b[where] = torch.randn((half, dim), device=dev)
    comps.append([a, b])
    store = E.HashSpillStore(dim, (dim, dim))
    t.spill_to(half, store, slots=[(a, 0.1), (b, 0.0)])
    assert len(store) == half and t.size() == half
    t.set_step(3)
    stores.append(store)
  NAMES = ('keys', 'table', 'last_seen', 'freq', 'stats', 'counts')
  saved = [({n: getattr(t, n).clone() for n in NAMES}, [c.clone() for c in cs], st.peek(st.keys()))
           for t, cs, st in zip(tables, comps, stores)]

  def restore():
    for t, cs, st, (state, cc, held) in zip(tables, comps, stores, saved):
      for n in NAMES:
        getattr(t, n).copy_(state[n])
      for c, s in zip(cs, cc):
        c.copy_(s)
      if len(st) != half:
        st.clear()
        st.put(held)

  def wall(step):
    restore()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6

  def events(step):
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

  def batch_of(name, k):
    if name == 'zipf':
      order = k[rng.permutation(batch)]
      return order[(rng.zipf(1.2, size=batch) - 1) % batch]
    share = {'0pct': 0.0, '1pct': 0.01, '10pct': 0.10, '100pct': 1.0}[name]
    n_miss = int(batch * share)
    ids = np.concatenate([k[:half][rng.permutation(n_miss) % half], k[half:][rng.randint(0, half, size=batch - n_miss)]])
    return ids[rng.permutation(batch)]

  lib = _lib.lib()
  result = {'shape': {'cols': cols, 'slots_per_col': capacity, 'resident_per_col': half, 'spilled_per_col': half,
                      'ids_per_col': batch, 'slab_size': slab_size, 'dim': dim, 'companions': 2},
            'rounds': args.rounds}
  for name in args.cases.split(','):
    host_ids = [batch_of(name, k) for k in keys]
    ids = [torch.from_numpy(i).to(dev) for i in host_ids]
    got = {}

    def batched():
      got['batched'] = E.hash_fault_in(tables, ids, stores, comps)

    def loop():
      got['loop'] = [t.fault_in(i, st, cs) for t, i, st, cs in zip(tables, ids, stores, comps)]

    def missing():
      got['missing'] = E.hash_missing(tables, ids)
    # the C call on buffers of its own, for the capture
    mcols = (_lib.HashMissingColumn * cols)()
    slots = torch.empty((cols, batch), dtype=torch.int64, device=dev)
    outs = torch.empty((cols, batch), dtype=torch.int64, device=dev)
    counts = torch.empty(cols, dtype=torch.int64, device=dev)
    for c, (t, i) in enumerate(zip(tables, ids)):
      col = mcols[c]
      col.keys_cache, col.slab_count, col.slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
      t._describe_expiry(col.exp)   # pylint: disable=protected-access
      col.keys, col.n_keys, col.slots = i.data_ptr(), batch, slots[c].data_ptr()
      col.out_ids, col.out_capacity, col.count = outs[c].data_ptr(), batch, counts.data_ptr() + 8 * c
    nbytes = lib.hbk_hash_missing_workspace_bytes(cols, mcols, None)
    workspace = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)
    find_outs = [torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(cols)]

    def c_call():
      s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
      _lib.check(lib.hbk_hash_missing_n(cols, mcols, None, workspace.data_ptr(), nbytes, s))

    def find_alone():
      E.hash_translate(tables, ids, insert=False, outs=find_outs)
    restore()
    for step in (c_call, find_alone):   # (before the captures: every first launch is behind us)
      events(step)
    graphs = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      for f, step in (('missing_graph', c_call), ('find_graph', find_alone)):
        graphs[f] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[f], stream=side):
          step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    walls = {'batched': batched, 'loop': loop, 'missing': missing}
    replays = {f: g.replay for f, g in graphs.items()}
    t = {f: [] for f in list(walls) + list(replays)}
    for f, step in walls.items():   # one untimed pass of everything: allocator, first launches
      wall(step)
    restore()
    for step in replays.values():
      events(step)
    for _ in range(args.rounds):   # taking turns
      for f, step in walls.items():
        t[f].append(wall(step))
      restore()
      for f, step in replays.items():
        t[f].append(events(step))
    # both forms restore the same keys and leave the same tables and stores behind
    after = {}
    for f in ('batched', 'loop'):
      wall(walls[f])
      exports = E.hash_export(tables, slots=comps)
      after[f] = [x[torch.argsort(e.keys)] for e in exports for x in [e.keys, e.rows, e.last_seen, e.freq] + e.slots]
      after[f] += [st.keys().to(dev) for st in stores]
    assert got['batched'] == got['loop'], (got['batched'], got['loop'])
    assert all(torch.equal(a, b) for a, b in zip(after['batched'], after['loop']))
    distinct_missed = int(sum(m.numel() for m in got['missing']))
    torch.cuda.synchronize()
    occ = cols * batch
    missed_occ = int(sum(int((s < 0).sum().item()) for s in slots))
    cells = cols * 2 * batch
    find_bytes = occ * (8 + 64 + 8)
    rest_bytes = occ * 3 * 8 + missed_occ * (3 * 8 + 3 * 8 + 2 * 4 + 4) + distinct_missed * 8 + cells * 12
    case = {'restored_per_col': int(np.mean(got['batched'])), 'missed_occurrences': missed_occ,
            'distinct_missed': distinct_missed, 'workspace_bytes': int(nbytes),
            'batched_hash_fault_in': summary(t['batched']), 'loop_of_fault_in': summary(t['loop']),
            'hash_missing_alone': summary(t['missing']),
            'missing_graph': summary(t['missing_graph'], find_bytes + rest_bytes),
            'find_graph': summary(t['find_graph'], find_bytes)}
    rest_us = float(np.median(t['missing_graph'])) - float(np.median(t['find_graph']))
    case['clear_claim_compact_by_difference'] = {
      'us': round(rest_us, 2), 'bytes': rest_bytes, 'TBps': round(rest_bytes / rest_us * 1e-6, 3) if rest_us > 0 else None}
    case['loop_over_batched'] = round(case['loop_of_fault_in']['us'] / case['batched_hash_fault_in']['us'], 2)
    case['batched_not_above_the_loops_slowest_round'] = bool(
      case['batched_hash_fault_in']['us'] <= case['loop_of_fault_in']['min_max_us'][1])
    result[name] = case
    print(name, json.dumps(case), file=sys.stderr, flush=True)
  line = json.dumps(result)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
