"""Sharded hash tables (hbk_hash_translate_runs_n, hbk_sharded_set_hash_tables), in one process:

  translate     the owner translate of 26 tables x 8 runs (the 65 536 ids per column of the other hash benches:
                8 runs of 8 192; every key resident; capacity 131 072, slab_size 8, dim 16), plain and expiring:
    runs                     hbk_hash_translate_runs_n: ONE launch
    virtual_columns          the existing entry over 26 x 8 = 208 virtual columns: 4 launches (what the parent
                             commit offers)
  step          a full sharded step, forward + backward with the SGD apply, 26 columns x `--batch` ids per rank,
                dim 16: ShardedHashGroupLookup (every key resident after the first step) against a bucketed
                ShardedGroupLookup of the same shapes; W = 1 over a real communicator and W = 8 over
                Collective.local_world(8) (ranks as host threads on one GPU: device copies instead of RCCL)
  --regression  ONLY the bucketed W = 1 and W = 8 steps, one JSON line on stdout and nothing else written: run
                from a checkout of the parent commit and from this one, taking turns, to show that an ordinary
                plan's step did not move

Every timed region is `--steps` operations between HIP events (translate, W = 1) or a host clock around work that
ends in a device synchronise (W = 8: rank 0's clock), after `--warmup`; `--rounds` rounds with the forms taking
turns; medians with min / max.  Prints one JSON line and appends it to `--out` (default
profiles/sharded_hash.txt).

  python tools/bench_sharded_hash.py [--rounds 7 --steps 50 --warmup 10]
"""
import argparse
import ctypes as C
import json
import os
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
  p.add_argument('--steps', type=int, default=50)
  p.add_argument('--warmup', type=int, default=10)
  p.add_argument('--cols', type=int, default=26)
  p.add_argument('--runs', type=int, default=8)
  p.add_argument('--batch', type=int, default=8192)
  p.add_argument('--regression', action='store_true')
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sharded_hash.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_sharded_hash.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  cols, dim, slab_size = args.cols, 16, 8
  rng = np.random.RandomState(779)
  lib = _lib.lib()

  def summary(us):
    med = float(np.median(us))
    return {'us': round(med, 2), 'min_max_us': [round(min(us), 2), round(max(us), 2)]}

  def timed_events(step):
    for _ in range(args.warmup):
      step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
      step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps

  def alternate(forms):
    t = {k: [] for k in forms}
    for _ in range(args.rounds):
      for k, step in forms.items():
        t[k].append(timed_events(step))
    return {k: summary(v) for k, v in t.items()}

  # ---- 1. the owner translate ----------------------------------------------------------------------------
  def translate(expiring):
    n_keys, n_runs = 65536, args.runs
    per_run = n_keys // n_runs
    stream = _lib.current_stream(dev)
    tables = [hb.embedding.HashTable(2 * n_keys, dim, dev, slab_size=slab_size, expiring=expiring) for _ in range(cols)]
    keys = [torch.from_numpy(np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n_keys + 64, dtype=np.int64))[:n_keys]
                             .copy()).to(dev) for _ in range(cols)]
    keys = [k[torch.randperm(n_keys, device=dev)].contiguous() for k in keys]
    for t, k in zip(tables, keys):
      t.lookup_or_insert(k)                                 # resident from here on
      assert t.size() == n_keys and t.failed() == 0
    slots = [torch.empty(n_keys, dtype=torch.int64, device=dev) for _ in range(cols)]
    slots_v = [torch.empty(n_keys, dtype=torch.int64, device=dev) for _ in range(cols)]
    col = (_lib.HashColumn * cols)()
    exp = (_lib.HashExpiry * cols)() if expiring else None
    vcol = (_lib.HashColumn * (cols * n_runs))()
    vexp = (_lib.HashExpiry * (cols * n_runs))() if expiring else None
    runs, ptrs = [], []
    for c, t in enumerate(tables):
      t._describe(col[c])
      if expiring:
        t._describe_expiry(exp[c])
      r = (_lib.HashRun * n_runs)()
      for q in range(n_runs):
        r[q].keys = keys[c].data_ptr() + 8 * q * per_run
        r[q].slots = slots[c].data_ptr() + 8 * q * per_run
        r[q].n_keys = per_run
        v = vcol[c * n_runs + q]
        t._describe(v)
        v.keys, v.slots, v.n_keys = r[q].keys, slots_v[c].data_ptr() + 8 * q * per_run, per_run
        if expiring:
          t._describe_expiry(vexp[c * n_runs + q])
      runs.append(r)
      ptrs.append(C.cast(r, C.c_void_p).value)
    n_runs_arr, run_ptrs = _lib.i32_array([n_runs] * cols), _lib.ptr_array(ptrs)

    def by_runs():
      _lib.check(lib.hbk_hash_translate_runs_n(cols, col, exp, None, n_runs_arr, run_ptrs, 1, stream))

    def by_virtual_columns():
      if expiring:
        _lib.check(lib.hbk_hash_insert_expiring_n(cols * n_runs, vcol, vexp, 1, stream))
      else:
        _lib.check(lib.hbk_hash_insert_n(cols * n_runs, vcol, 1, stream))
    by_runs()
    by_virtual_columns()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(slots, slots_v))          # resident keys: the same slots
    out = alternate({'runs': by_runs, 'virtual_columns': by_virtual_columns})
    out['launches'] = {'runs': 1, 'virtual_columns': -(-cols * n_runs // 64)}
    out['virtual_over_runs'] = round(out['virtual_columns']['us'] / out['runs']['us'], 3)
    return out

  # ---- 2. a full step -----------------------------------------------------------------------------------
  def make_step(kind, comm, world, r):
    """One rank's forward + backward-with-apply closure; ids drawn from a pool the whole world shares."""
    g = torch.Generator(device='cpu').manual_seed(1000 + r)
    pool = 4 * args.batch * world
    ids = [(torch.randint(0, pool, (args.batch,), generator=g, dtype=torch.int64) * 2654435761 - (1 << 40)).to(dev)
           for _ in range(cols)]
    grads = [torch.randn(args.batch, dim, device=dev) for _ in range(cols)]
    outs = [torch.empty(args.batch, dim, device=dev) for _ in range(cols)]
    rows = 2 * pool // world
    if kind == 'hash':
      tables = [hb.embedding.HashTable(rows, dim, dev, slab_size=slab_size) for _ in range(cols)]
      drv = hb.embedding.ShardedHashGroupLookup(tables, comm, combiners='sum')
    else:
      shards = [torch.zeros(rows, dim, device=dev) for _ in range(cols)]
      drv = hb.embedding.ShardedGroupLookup(shards, comm, buckets=[rows * world] * cols, combiners='sum')
    bound = drv.bind(ids, None, outs)

    def step():
      drv.launch(bound)
      drv.backward(grads, apply_lr=0.01, emit=False)
    return drv, step

  def step_w1(kinds):
    comm = hb.distribute.Collective(world_size=1, rank=0)
    made = {k: make_step(k, comm, 1, 0) for k in kinds}
    out = alternate({k: s for k, (_, s) in made.items()})
    for d, _ in made.values():
      d.close()
    comm.close()
    return out

  def step_w8(kinds, world=8):
    comms = hb.distribute.Collective.local_world(world)
    times, errors = {k: [] for k in kinds}, []
    gate = threading.Barrier(world)

    def run(r):
      try:
        with torch.cuda.stream(torch.cuda.Stream()):
          made = {k: make_step(k, comms[r], world, r) for k in kinds}
          for _ in range(args.rounds):
            for k in kinds:
              step = made[k][1]
              for _ in range(args.warmup):
                step()
              torch.cuda.current_stream().synchronize()
              gate.wait(timeout=120)
              t0 = time.perf_counter()
              for _ in range(args.steps):
                step()
              torch.cuda.current_stream().synchronize()
              if r == 0:
                times[k].append((time.perf_counter() - t0) * 1e6 / args.steps)
          for d, _ in made.values():
            d.close()
      except Exception as e:  # pylint: disable=broad-except
        errors.append((r, repr(e)))
        gate.abort()
    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
      t.start()
    for t in threads:
      t.join(timeout=600)
    for c in comms:
      c.close()
    if errors:
      raise SystemExit(f'step_w8 failed: {errors}')
    return {k: summary(v) for k, v in times.items()}

  shape = {'cols': cols, 'dim': dim, 'slab_size': slab_size, 'batch_per_rank': args.batch,
           'translate': {'runs_per_table': args.runs, 'keys_per_table': 65536, 'slots_per_table': 131072}}
  if args.regression:
    line = json.dumps({'regression_bucketed_step': {'w1': step_w1(['bucketed'])['bucketed'],
                                                    'w8_local_world': step_w8(['bucketed'])['bucketed']},
                       'shape': shape, 'rounds': args.rounds, 'steps': args.steps})
    print(line, flush=True)
    return
  result = {'shape': shape, 'rounds': args.rounds, 'steps': args.steps,
            'translate_plain': translate(False), 'translate_expiring': translate(True)}
  torch.cuda.empty_cache()
  for name, fn in (('step_w1', step_w1), ('step_w8_local_world', step_w8)):
    out = fn(['hash', 'bucketed'])
    out['hash_over_bucketed'] = round(out['hash']['us'] / out['bucketed']['us'], 3)
    result[name] = out
  line = json.dumps(result)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
