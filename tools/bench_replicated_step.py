"""What training replicated tables at W > 1 costs: the pack, rows and slice-apply launches alone against their
byte models, the same columns' fused direct step at W = 1 as the floor, and the layer's backward with
``aggregate_replicated=True`` against what the library offered before it.

Shape: 8 tables x 4096 rows x dim 16 fp32, B = 4096 int64 ids per table and rank of which 2048 are distinct (half
the rows touched).

  launch   hbk_replica_grads_pack_n, hbk_replica_grads_rows_n and hbk_sparse_apply_slices_n (SGD, Adagrad, Lazy Adam)
           alone, as replays of a captured graph (no Python per step), with their byte models:
             pack   4 * bucket floats (the clear) + touched * (8 + 4 dim [read] + 4 dim + 4 [written]) per table
             rows   rows * (4 + 8) per table
             apply  rows * 8 (urows) + touched * 4 dim * (1 gradient + 2 per table-shaped buffer stepped)
           and `fused_*`: GroupLookupGrad's direct step (reduce + step in one call, step only) of the same ids at
           W = 1 -- the floor a rank pays for these tables when nothing has to cross ranks
  layer    on Collective.local_world at W = 2 and 4 (the 8 replicated tables and one sharded table of 10^5 rows),
           SGD, the backward alone over one resident forward:
             aggregated   DenseFeatures(..., aggregate_replicated=True).backward(grad, apply_lr)
             by_hand      DenseFeatures(...).backward(grad, apply_lr), then n_unique to the host,
                          hb.distribute.aggregate_gradients over the 8 IndexedSlices (two allgathers each), then a
                          GroupLookupGrad over the gathered slices that dedups them again and steps
           The ranks of local_world are HOST THREADS ON ONE GPU that meet at host barriers inside every collective:
           these numbers are host-bound wall time per step (rank 0's clock) and say how many collectives and host
           waits a form makes, not what a link would carry.

Medians of `--rounds` rounds with min / max, the forms taking turns.  Prints one JSON line per part and appends it
to `--out` (default profiles/replicated_step.txt).

  python tools/bench_replicated_step.py [--steps 30 --warmup 5 --rounds 7]
"""
import argparse
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

N_TABLES, ROWS, DIM, B, TOUCHED = 8, 4096, 16, 4096, 2048
SHARDED_ROWS = 100000
LR = 1e-6


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--steps', type=int, default=30)
  p.add_argument('--warmup', type=int, default=5)
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--worlds', default='2,4')
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'replicated_step.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_replicated_step.py measures on a GPU: none found')
  fc, emb, dist = hb.feature_column, hb.embedding, hb.distribute
  dev = torch.device('cuda:0')

  def report(result):
    result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
      f.write(line + '\n')

  def summary(times):
    out = {k + '_us': round(float(np.median(v)), 2) for k, v in times.items()}
    out.update({k + '_min_max_us': [round(min(v), 2), round(max(v), 2)] for k, v in times.items()})
    return out

  def timed(step):
    for _ in range(args.warmup):
      step()
    torch.cuda.current_stream().synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
      step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps   # us per step

  def graph_of(fn):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
      fn()
    return g.replay

  def batch_ids(rng):
    """B ids per table: TOUCHED distinct rows, each named B / TOUCHED times."""
    return [torch.from_numpy(np.tile(rng.permutation(ROWS)[:TOUCHED], B // TOUCHED).astype(np.int64)).to(dev)
            for _ in range(N_TABLES)]

  # ---- the launches alone ---------------------------------------------------------------------------------------
  rng = np.random.RandomState(0)
  ids = batch_ids(rng)
  grads = [torch.randn(B, DIM, device=dev) for _ in range(N_TABLES)]
  new_tables = lambda: [torch.empty(ROWS, DIM, device=dev).uniform_(-1e-3, 1e-3) for _ in range(N_TABLES)]   # noqa: E731
  tables = new_tables()
  local = emb.GroupLookupGrad(emb.GroupLookup(tables, combiners='sum'))(ids, grads)     # this rank's slices
  rg = dist.ReplicatedGradients([(ROWS, DIM)] * N_TABLES, None, device=dev)
  holes = rg.aggregate(local)
  forms = {'pack': graph_of(rg.launch_pack), 'rows': graph_of(rg.launch_rows)}
  slot_kw = {'sgd': {}, 'adagrad': dict(accums=[torch.full_like(t, 0.1) for t in tables]),
             'adam': dict(moments=[(torch.zeros_like(t), torch.zeros_like(t)) for t in tables])}
  keep = []
  for opt, kw in slot_kw.items():
    app = emb.SparseApply(tables, **kw)
    app(holes, LR, optimizer=opt)
    keep.append(app)
    forms['apply_' + opt] = graph_of(app.launch)
    t2 = new_tables()
    kw2 = {k: ([torch.full_like(t, 0.1) for t in t2] if k == 'accums' else
               [(torch.zeros_like(t), torch.zeros_like(t)) for t in t2]) for k in kw}
    fused = emb.GroupLookupGrad(emb.GroupLookup(t2, combiners='sum'), **kw2)
    fused(ids, grads, apply_lr=LR, optimizer=opt, emit=False)
    keep.append(fused)
    forms['fused_' + opt] = graph_of(lambda f=fused, o=opt: f.launch(LR, optimizer=o))
  times = {k: [] for k in forms}
  for _ in range(args.rounds):
    for k, step in forms.items():
      times[k].append(timed(step))
  res = {'part': 'launch', 'tables': N_TABLES, 'rows': ROWS, 'dim': DIM, 'touched': TOUCHED, 'capacity': B}
  res.update(summary(times))
  model = {'pack': 4 * rg.bucket.numel() + N_TABLES * TOUCHED * (8 + 4 * DIM + 4 * DIM + 4),
           'rows': N_TABLES * ROWS * 12}
  for opt, bufs in (('sgd', 1), ('adagrad', 2), ('adam', 3)):
    model['apply_' + opt] = N_TABLES * (ROWS * 8 + TOUCHED * 4 * DIM * (1 + 2 * bufs))
  for k, nbytes in model.items():
    res[k + '_model_KB'] = round(nbytes / 1e3, 1)
    res[k + '_GBps'] = round(nbytes / res[k + '_us'] / 1e3, 1)
  report(res)

  # ---- the layer on the in-process world -------------------------------------------------------------------------
  def layer_part(world):
    comms = dist.Collective.local_world(world)
    names = ('aggregated', 'by_hand')
    times = {k: [] for k in names}
    gate = threading.Barrier(world)
    errors = []

    def run(r):
      try:
        with torch.cuda.stream(torch.cuda.Stream()):
          rng = np.random.RandomState(10 + r)
          cols = lambda: ([fc.EmbeddingColumn(f'c{c}', ROWS, DIM, 'sum', hot_rows=False)   # noqa: E731
                           for c in range(N_TABLES)] +
                          [fc.EmbeddingColumn('s', SHARDED_ROWS, DIM, 'sum', hot_rows=False)])
          # (the same replicas on every rank)
          init = lambda col, rows, d: torch.linspace(-1e-3, 1e-3, rows * col.dimension, device=d).view(   # noqa: E731
            rows, col.dimension)
          agg = fc.DenseFeatures(cols(), dev, coll=comms[r], batch_size=B, init=init, aggregate_replicated=True)
          plain = fc.DenseFeatures(cols(), dev, coll=comms[r], batch_size=B, init=init)
          assert agg.sharded == [False] * N_TABLES + [True]
          feats = {f'c{c}': i for c, i in enumerate(batch_ids(rng))}
          feats['s'] = torch.from_numpy(rng.randint(0, 2 ** 40, size=B).astype(np.int64)).to(dev)
          grad = torch.randn(B, (N_TABLES + 1) * DIM, device=dev)
          agg(feats)
          plain(feats)
          rep = [plain.weights[c] for c in range(N_TABLES)]
          again = emb.GroupLookupGrad(emb.GroupLookup(rep, combiners='sum'))

          def aggregated():
            agg.backward(grad, apply_lr=LR)

          def by_hand():
            res = plain.backward(grad, apply_lr=LR)[:N_TABLES]
            counts = torch.cat([k for _, _, k in res]).tolist()            # the one host read of the caller
            out = dist.aggregate_gradients([(g[:k], u[:k]) for (u, g, _), k in zip(res, counts)], comms[r])
            again([i for _, i in out], [v for v, _ in out], apply_lr=LR, emit=False)
          for _ in range(args.rounds):
            for name, step in (('aggregated', aggregated), ('by_hand', by_hand)):
              for _ in range(args.warmup):
                step()
              torch.cuda.current_stream().synchronize()
              gate.wait()
              t0 = time.perf_counter()
              for _ in range(args.steps):
                step()
              torch.cuda.current_stream().synchronize()
              dt = (time.perf_counter() - t0) * 1e6 / args.steps
              if r == 0:
                times[name].append(dt)
          drift = float(agg.replica_drift())
          assert drift == 0.0, drift
          agg.close()
          plain.close()
      except Exception as e:  # pylint: disable=broad-except
        import traceback
        errors.append((r, repr(e), traceback.format_exc()))
        gate.abort()
    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
      t.start()
    for t in threads:
      t.join()
    for cm in comms:
      cm.close()
    if errors:
      raise SystemExit(f'layer part at W = {world} failed: {errors}')
    res = {'part': 'layer', 'world': world, 'transport': 'local_world (host threads on one GPU: host-bound)',
           'tables': N_TABLES, 'rows': ROWS, 'dim': DIM, 'batch_per_rank': B, 'touched_per_rank': TOUCHED,
           'sharded_rows': SHARDED_ROWS, 'optimizer': 'sgd'}
    res.update(summary(times))
    res['by_hand_over_aggregated'] = round(res['by_hand_us'] / res['aggregated_us'], 3)
    report(res)

  for world in [int(w) for w in args.worlds.split(',') if w]:
    layer_part(world)


if __name__ == '__main__':
  main()
