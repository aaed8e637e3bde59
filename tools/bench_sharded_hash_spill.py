"""Sharded hash tables with a host tier inside the step, in one process:

  (a) missing   hbk_hash_missing_runs_n beside hbk_hash_missing_n on the same ids concatenated: 26 expiring tables x
                131 072 slots, slab_size 8, 65 536 resident keys per table; per column 8 runs x 8 192 ids, as the owner
                of a sharded table receives them at W = 8.  Cases: 0 %, 1 %, 10 % and 100 % of a column's id
                occurrences name keys the table does not hold, and `zipf`: ranks drawn Zipf(1.2) over 131 072 keys in
                a random order, half of them resident.  Both calls captured into a graph; the replays are timed
                between HIP events.  The bytes are the same; the difference is the run lookup and the padded tiles
                (none here: 8 192 is a multiple of 256).  No ratio is promised.
  (b) step      a full step -- forward, backward with the SGD apply -- of ShardedHashGroupLookup over expiring
                tables, 26 columns x `--batch` ids per rank, dim 16, at W = 1 over a real communicator and at W = 8
                over Collective.local_world(8) (ranks as host threads on one GPU), in five forms:
                  no_stores      stores=None, every key resident: the one-call forward
                  empty_stores   the same tables, a store per column, all empty: the price of the split alone
                  stores_0pct / stores_1pct / stores_10pct
                                 the older half of every table's keys spilled into its store; that share of a rank's
                                 id occurrences names spilled keys (the others resident ones)
                Every timed step is ONE step on a host clock between two device synchronisations (the host tier is
                host work; W = 8: rank 0's clock behind a barrier); tables and stores are restored before it where the
                step before moved keys.  One warm step per form first.
  (c) --parent DIR   the regression check: `tools/bench_sharded_hash.py --regression` and `bench.py --gpus 1` run as
                child processes from DIR (a built checkout of the parent commit) and from this tree, (parent, this) x
                `--turns` taking turns; every median of this tree is set against the span of the parent's turns.

`--rounds` rounds with the forms taking turns; medians with min - max.  `--parts` picks among a, b, c.
Prints one JSON line and appends it to `--out` (default profiles/sharded_hash_spill.txt).

  python tools/bench_sharded_hash_spill.py [--rounds 7] [--parts a,b,c --parent ../parent]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import threading
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
  p.add_argument('--parts', default='a,b')
  p.add_argument('--batch', type=int, default=8192)
  p.add_argument('--parent', default=None)
  p.add_argument('--turns', type=int, default=3)
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sharded_hash_spill.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_sharded_hash_spill.py measures on a GPU: none found')
  lib = _lib.lib()
  dev = torch.device('cuda:0')
  cols, dim, slab_size = args.cols, 16, 8
  parts = args.parts.split(',')

  def summary(us):
    return {'us': round(float(np.median(us)), 2), 'min_max_us': [round(min(us), 2), round(max(us), 2)]}

  # ---- (a) the miss list over runs beside the flat form ---------------------------------------------------------
  def missing_runs():
    n_runs, run_len = 8, 8192
    batch = n_runs * run_len
    capacity = 2 * batch
    rng = np.random.RandomState(782)

    def distinct(n):
      k = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n + 64, dtype=np.int64))
      rng.shuffle(k)
      return k[:n].copy()
    keys = [distinct(2 * batch) for _ in range(cols)]        # [:batch] resident, [batch:] absent
    tables = [hb.embedding.HashTable(capacity, dim, dev, slab_size=slab_size, expiring=True) for _ in range(cols)]
    for t, k in zip(tables, keys):
      t.set_step(1)
      t.lookup_or_insert(torch.from_numpy(k[:batch]).to(dev))
      assert t.size() == batch and t.failed() == 0

    def batch_of(name, k):
      if name == 'zipf':
        order = rng.permutation(2 * batch)
        ranks = np.minimum(rng.zipf(1.2, size=batch), 2 * batch) - 1
        return k[order[ranks]]
      share = float(name[:-3]) / 100.0
      miss = rng.rand(batch) < share
      return np.where(miss, k[batch + rng.randint(0, batch, size=batch)], k[rng.randint(0, batch, size=batch)])

    ids = [torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(cols)]
    slots = [torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(cols)]
    outs = [torch.empty(batch, dtype=torch.int64, device=dev) for _ in range(cols)]
    counts = torch.zeros(cols, dtype=torch.int64, device=dev)
    rcols = (_lib.HashMissingRunsColumn * cols)()
    fcols = (_lib.HashMissingColumn * cols)()
    run_arrays = [(_lib.HashRun * n_runs)() for _ in range(cols)]
    for c, t in enumerate(tables):
      for col in (rcols[c], fcols[c]):
        col.keys_cache, col.slab_count, col.slab_size = t.keys.data_ptr(), t.slab_count, t.slab_size
        t._describe_expiry(col.exp)   # pylint: disable=protected-access
        col.out_ids, col.out_capacity, col.count = outs[c].data_ptr(), batch, counts.data_ptr() + 8 * c
      fcols[c].keys, fcols[c].n_keys, fcols[c].slots = ids[c].data_ptr(), batch, slots[c].data_ptr()
      for q in range(n_runs):   # the runs are the eighths of the same buffers
        r = run_arrays[c][q]
        r.keys, r.slots, r.n_keys = ids[c].data_ptr() + 8 * q * run_len, slots[c].data_ptr() + 8 * q * run_len, run_len
    n_runs_arr = (C.c_int32 * cols)(*[n_runs] * cols)
    run_ptrs = (C.c_void_p * cols)(*[C.addressof(a) for a in run_arrays])
    runs_bytes = lib.hbk_hash_missing_runs_workspace_bytes(cols, n_runs_arr, run_ptrs)
    flat_bytes = lib.hbk_hash_missing_workspace_bytes(cols, fcols, None)
    runs_ws = torch.empty(runs_bytes // 8 + 2, dtype=torch.int64, device=dev)
    flat_ws = torch.empty(flat_bytes // 8 + 2, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(dev)
    s = C.c_void_p(stream.cuda_stream)

    def call_runs():
      _lib.check(lib.hbk_hash_missing_runs_n(cols, rcols, n_runs_arr, run_ptrs, runs_ws.data_ptr(), runs_bytes, s))

    def call_flat():
      _lib.check(lib.hbk_hash_missing_n(cols, fcols, None, flat_ws.data_ptr(), flat_bytes, s))

    graphs = {}
    with torch.cuda.stream(stream):
      for name, call in (('runs', call_runs), ('flat', call_flat)):
        call()
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
          call()
        graphs[name] = g

    def replay_us(g):
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      g.replay()
      e1.record()
      e1.synchronize()
      return e0.elapsed_time(e1) * 1e3

    cases = {}
    for name in args.cases.split(','):
      for c in range(cols):
        ids[c].copy_(torch.from_numpy(batch_of(name, keys[c])))
      times = {'runs': [], 'flat': []}
      found = {}
      for form in ('runs', 'flat'):      # (one warm replay each; the two forms must agree)
        graphs[form].replay()
        torch.cuda.synchronize()
        k = counts.tolist()
        found[form] = (k, [outs[c][:k[c]].clone() for c in range(cols)], [x.clone() for x in slots])
      assert found['runs'][0] == found['flat'][0]
      assert all(torch.equal(a, b) for a, b in zip(found['runs'][1], found['flat'][1]))
      assert all(torch.equal(a, b) for a, b in zip(found['runs'][2], found['flat'][2]))
      for _ in range(args.rounds):
        for form in ('runs', 'flat'):
          times[form].append(replay_us(graphs[form]))
      cases[name] = {'distinct_missed_per_column': int(np.mean(found['runs'][0])),
                               'runs': summary(times['runs']), 'flat': summary(times['flat'])}
    return {'runs': n_runs, 'run_len': run_len, 'slots_per_table': capacity, 'cases': cases}

  # ---- (b) the step ---------------------------------------------------------------------------------------------
  FORMS = ('no_stores', 'empty_stores', 'stores_0pct', 'stores_1pct', 'stores_10pct')
  NAMES = ('keys', 'table', 'last_seen', 'freq', 'stats', 'counts')

  def make_rank(comm, world, r):
    """The five forms of one rank: {form: (restore, step)}.  Per column 2 * batch * world keys, the older half
    inserted at step 1, the newer at step 2, each on its owner; `full` tables hold all of them, `half` tables had the
    older half spilled into their stores."""
    E = hb.embedding
    rng = np.random.RandomState(900 + r)
    shared = np.random.RandomState(899)
    universe = []
    for _ in range(cols):
      k = np.unique(shared.randint(-2 ** 62, 2 ** 62, size=2 * args.batch * world + 64, dtype=np.int64))
      shared.shuffle(k)
      universe.append(k[:2 * args.batch * world])
    n_half = args.batch * world
    rows = 4 * args.batch

    def tables_with_all():
      tables = [E.HashTable(rows, dim, dev, slab_size=slab_size, expiring=True) for _ in range(cols)]
      for t, k in zip(tables, universe):
        for step, part in ((1, k[:n_half]), (2, k[n_half:])):
          t.set_step(step)
          mine = part[np.mod(part, world) == r]
          t.lookup_or_insert(torch.from_numpy(mine).to(dev))
        assert t.failed() == 0
        t.set_step(3)
      return tables
    full, half = tables_with_all(), tables_with_all()
    plain = E.ShardedHashGroupLookup(full, comm, combiners='sum')
    empty = E.ShardedHashGroupLookup(full, comm, combiners='sum', stores=[E.HashSpillStore(dim) for _ in range(cols)])
    tiered = E.ShardedHashGroupLookup(half, comm, combiners='sum', stores=[E.HashSpillStore(dim) for _ in range(cols)])
    newer = [int((np.mod(k[n_half:], world) == r).sum()) for k in universe]
    spilled = tiered.spill_to(newer)
    assert all(len(st) == n and n > 0 for st, n in zip(tiered.stores, spilled))
    saved = [({n: getattr(t, n).clone() for n in NAMES}, st.peek(st.keys())) for t, st in zip(half, tiered.stores)]

    def restore():
      for t, st, (state, held) in zip(half, tiered.stores, saved):
        if len(st) != len(held):
          for n in NAMES:
            getattr(t, n).copy_(state[n])
          st.clear()
          st.put(held)

    def batch_of(share):
      ids = []
      for k in universe:
        old = rng.rand(args.batch) < share
        ids.append(torch.from_numpy(np.where(old, k[rng.randint(0, n_half, size=args.batch)],
                                             k[n_half + rng.randint(0, n_half, size=args.batch)])).to(dev))
      return ids
    grads = [torch.randn(args.batch, dim, device=dev) for _ in range(cols)]
    outs = [torch.empty(args.batch, dim, device=dev) for _ in range(cols)]

    def form(drv, share, fix):
      bound = drv.bind(batch_of(share), None, outs)

      def step():
        drv.launch(bound)
        drv.backward(grads, apply_lr=0.01, emit=False)
      return fix, step
    forms = {'no_stores': form(plain, 0.0, None), 'empty_stores': form(empty, 0.0, None),
             'stores_0pct': form(tiered, 0.0, restore), 'stores_1pct': form(tiered, 0.01, restore),
             'stores_10pct': form(tiered, 0.10, restore)}
    return forms, (plain, empty, tiered)

  def step_world(world):
    real = world == 1
    comms = [hb.distribute.Collective(world_size=1, rank=0)] if real else hb.distribute.Collective.local_world(world)
    times, errors = {k: [] for k in FORMS}, []
    gate = threading.Barrier(world)

    def run(r):
      try:
        with torch.cuda.stream(torch.cuda.Stream()):
          forms, drivers = make_rank(comms[r], world, r)
          for rnd in range(args.rounds + 1):            # (round 0: one warm step per form, not recorded)
            for k in FORMS:
              fix, step = forms[k]
              if fix is not None:
                fix()
              torch.cuda.current_stream().synchronize()
              gate.wait(timeout=300)
              t0 = time.perf_counter()
              step()
              torch.cuda.current_stream().synchronize()
              if r == 0 and rnd > 0:
                times[k].append((time.perf_counter() - t0) * 1e6)
          for d in drivers:
            d.close()
      except Exception as e:  # pylint: disable=broad-except
        errors.append((r, repr(e)))
        gate.abort()
    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
      t.start()
    for t in threads:
      t.join(timeout=900)
    for c in comms:
      c.close()
    if errors:
      raise SystemExit(f'step at W = {world} failed: {errors}')
    return {k: summary(v) for k, v in times.items()}

  # ---- (c) the parent commit and this tree, taking turns --------------------------------------------------------
  def regression():
    trees = (('parent', os.path.abspath(args.parent)), ('this', ROOT))
    runs = {name: {'w1': [], 'w8_local_world': [], 'bench_ms_per_step': []} for name, _ in trees}
    for _ in range(args.turns):
      for name, root in trees:
        out = subprocess.run([sys.executable, os.path.join(root, 'tools', 'bench_sharded_hash.py'), '--regression'],
                             cwd=root, check=True, capture_output=True, text=True, timeout=600).stdout
        step = json.loads([x for x in out.splitlines() if x.startswith('{')][-1])['regression_bucketed_step']
        runs[name]['w1'].append(step['w1']['us'])
        runs[name]['w8_local_world'].append(step['w8_local_world']['us'])
        out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '50',
                              '--warmup', '10'], cwd=root, check=True, capture_output=True, text=True,
                             timeout=600).stdout
        runs[name]['bench_ms_per_step'].append(json.loads([x for x in out.splitlines() if x.startswith('{')][-1])
                                               ['ms_per_step'])
    outside = []
    for what, parent in runs['parent'].items():
      for turn, v in enumerate(runs['this'][what]):
        if not min(parent) <= v <= max(parent):
          outside.append({'what': what, 'turn': turn, 'this': v, 'parent_span': [min(parent), max(parent)]})
    return {'turns': args.turns, 'runs': runs, 'outside_the_parents_span': outside}

  result = {'tool': 'bench_sharded_hash_spill', 'cols': cols, 'rounds': args.rounds, 'batch_per_rank': args.batch,
            'missing_runs': missing_runs() if 'a' in parts else 'not measured'}
  torch.cuda.empty_cache()
  result['step_w1'] = step_world(1) if 'b' in parts else 'not measured'
  result['step_w8_local_world'] = step_world(8) if 'b' in parts else 'not measured'
  if 'c' in parts and args.parent is None:
    raise SystemExit('part c needs --parent DIR: a built checkout of the parent commit')
  result['regression_vs_parent'] = regression() if 'c' in parts else 'not measured'
  line = json.dumps(result)
  print(line)
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
