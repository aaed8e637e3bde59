"""What zero-padded sequence lookups on SHARDED tables cost: the pack op alone, and the packed form of the step
against the pad-id grid form, in one process, the forms taking turns.

The shape of profiles/sequence_lookup.txt: 4 columns x 1M rows (or slots) x dim 16, B = 8192 per rank, T = 50,
Poisson(40) lengths, int64 ids.

  pack / row_grid / id_grid   hbk_sequence_pack_n, hbk_sequence_row_grid_n and hbk_sequence_id_grid_n alone, as
                              replays of a captured graph (no Python per step), with the pack's byte model: per
                              sample 4 B of row_splits read, 4 B of lengths and 4 B of sample_splits written; per
                              position 4 B of pos_splits written; per effective id 8 B read and 8 B written
  w1_*                        W = 1 on a real communicator, the drivers by hand (a layer shards nothing on one rank):
                              ShardedSequenceLookup (packed) against sequence_row_grid / sequence_id_grid +
                              the driver (pad id), forward and backward + SGD, a bucketed and a hash-keyed group
  w8_*                        W = 8 on Collective.local_world (ranks are host threads on ONE GPU, so the "wire" is
                              device copies), both forms through SequenceFeatures: sharded_zero_padding=True against
                              columns with a pad id; timed on rank 0 between HIP events, all ranks in step
  *_ids_sent                  the ids all ranks hand the step per step, in both forms

Timing follows tools/bench_hash_features.py: warm-up steps, then `--steps` steps between HIP events, `--rounds`
rounds with the forms taking turns; medians with min / max (the spread of each form).  Prints one JSON line and
appends it to `--out` (default profiles/sequence_pack.txt).

`--regression LABEL` measures only the pad-id forms at W = 8 through the layer and touches nothing this tool's
other forms need, so the same file also runs from a checkout of the parent commit: (parent, this) x 3 taking
turns shows whether the existing step moved.

  python tools/bench_sequence_pack.py [--steps 30 --warmup 5 --rounds 7] [--regression LABEL] [--world 8]
"""
import argparse
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_COLS, ROWS, DIM, B, T, LAM = 4, 1000000, 16, 8192, 50, 40
PAD = 0
LR = 1e-6


def batch_of(seed, dev):
  """Per column (ids, row_splits) on the device, and the effective ids of the batch."""
  rng = np.random.RandomState(seed)
  out, valid = [], 0
  for _ in range(N_COLS):
    lens = rng.poisson(LAM, size=B)
    valid += int(np.minimum(lens, T).sum())
    sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    # (a vocabulary of ROWS ids for both kinds of table: a hash table of 2 x ROWS slots stays half empty; the pad
    # id 0 is no data id)
    ids = rng.randint(1, ROWS, size=int(sp[-1])).astype(np.int64)
    out.append((torch.from_numpy(ids).to(dev), torch.from_numpy(sp).to(dev)))
  return out, valid


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--steps', type=int, default=30)
  p.add_argument('--warmup', type=int, default=5)
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--world', type=int, default=8)
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_pack.txt'))
  p.add_argument('--regression', default=None, metavar='LABEL',
                 help='only the pad-id forms at W = --world through the layer: the form that also runs from a '
                      'checkout of the parent commit (copy this file there); LABEL names the checkout')
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding import sequence as seq_mod   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_sequence_pack.py measures on a GPU: none found')
  fc = hb.feature_column
  dev = torch.device('cuda:0')
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)

  def timed(step, sync=None):
    for i in range(args.warmup):
      step(i)
    torch.cuda.current_stream().synchronize()
    if sync is not None:
      sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(args.steps):
      step(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps   # us per step

  def summary(t):
    out = {k + '_us': round(float(np.median(v)), 2) for k, v in t.items()}
    out.update({k + '_min_max_us': [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})
    return out

  def report(result):
    result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
      f.write(line + '\n')

  # ---- the step through the layer, W ranks as host threads ---------------------------------------------------
  def layer_columns(hashed, pad):
    kw = dict(pad_id=PAD) if pad else {}
    if hashed:
      return [fc.HashSequenceEmbeddingColumn(f'c{c}', 2 * ROWS, DIM, T, seed=c, **kw) for c in range(N_COLS)]
    return [fc.SequenceEmbeddingColumn(f'c{c}', ROWS, DIM, T, **kw) for c in range(N_COLS)]

  def world_forms(world, kinds):
    """{form: us per step, per round} of the layer forms `kinds` = [(name, hashed, pad)] at W = world."""
    comms = hb.distribute.Collective.local_world(world)
    barrier = threading.Barrier(world)
    times, errors = {}, []

    def rank(r):
      try:
        with torch.cuda.stream(torch.cuda.Stream()):
          forms = {}
          for name, hashed, pad in kinds:
            kw = {} if pad else dict(sharded_zero_padding=True)
            layer = fc.SequenceFeatures(layer_columns(hashed, pad), dev, coll=comms[r], batch_size=B, **kw)
            data, _ = batch_of(100 + r, dev)
            feats = {f'c{c}': data[c] for c in range(N_COLS)}
            grads = [torch.randn(B, T, DIM, device=dev) for _ in range(N_COLS)]
            outs, _ = layer(feats)
            layer.backward(grads, apply_lr=LR, emit=False)
            forms[name + '_fwd'] = lambda i, layer=layer, feats=feats: layer(feats)
            forms[name + '_bwd_sgd'] = lambda i, layer=layer, grads=grads: layer.backward(grads, apply_lr=LR, emit=False)
          t = {k: [] for k in forms}
          for _ in range(args.rounds):
            for k in forms:   # taking turns; every rank takes the same turn
              t[k].append(timed(forms[k], sync=barrier.wait))
          torch.cuda.current_stream().synchronize()
          if r == 0:
            times.update(t)
      except Exception as e:  # pylint: disable=broad-except
        import traceback
        errors.append((r, repr(e), traceback.format_exc()))
        barrier.abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for th in threads:
      th.start()
    for th in threads:
      th.join()
    for cm in comms:
      cm.close()
    if errors:
      raise SystemExit(f'a rank failed: {errors}')
    return times

  W = args.world
  if args.regression is not None:
    t = world_forms(W, [('bucketed_pad', False, True), ('hash_pad', True, True)])
    result = {'regression': args.regression, 'world': W}
    result.update(summary({f'w{W}_{k}': v for k, v in t.items()}))
    report(result)
    return

  # ---- the op alone ------------------------------------------------------------------------------------------
  data, valid = batch_of(7, dev)
  ids, splits = [d[0] for d in data], [d[1] for d in data]
  lib = _lib.lib()
  stream_of = lambda: _lib.current_stream(dev)   # noqa: E731

  def grid_call(fn, pad):
    cols, seqs = (_lib.LookupColumn * N_COLS)(), (_lib.Sequence * N_COLS)()
    for c in range(N_COLS):
      cols[c].bucket, cols[c].divisor = ROWS, 1
    counts, _ = seq_mod._bind_ids(cols, seqs, ids, splits, [T] * N_COLS, [pad] * N_COLS)   # pylint: disable=protected-access
    lengths, grids = seq_mod._alloc_side(counts, [T] * N_COLS, dev, True)   # pylint: disable=protected-access
    for c in range(N_COLS):
      seqs[c].lengths, seqs[c].row_grid = lengths[c].data_ptr(), grids[c].data_ptr()
    return (lambda: _lib.check(fn(N_COLS, cols, seqs, stream_of()))), (cols, seqs, lengths, grids)

  def pack_call():
    cols, seqs, packs = (_lib.LookupColumn * N_COLS)(), (_lib.Sequence * N_COLS)(), (_lib.SequencePack * N_COLS)()
    counts, _ = seq_mod._bind_ids(cols, seqs, ids, splits, [T] * N_COLS, [None] * N_COLS)   # pylint: disable=protected-access
    lengths, _ = seq_mod._alloc_side(counts, [T] * N_COLS, dev, False)   # pylint: disable=protected-access
    keep = [lengths]
    for c in range(N_COLS):
      cap = min(ids[c].numel(), B * T)
      bufs = (torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(B * T + 1, dtype=torch.int32, device=dev),
              torch.empty(B + 1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
      keep.append(bufs)
      seqs[c].lengths = lengths[c].data_ptr()
      packs[c].packed, packs[c].packed_capacity = bufs[0].data_ptr(), cap
      packs[c].pos_splits, packs[c].sample_splits, packs[c].total = (x.data_ptr() for x in bufs[1:])
    need = int(lib.hbk_sequence_pack_workspace_bytes(N_COLS, cols))
    work = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    keep.append(work)
    return (lambda: _lib.check(lib.hbk_sequence_pack_n(N_COLS, cols, seqs, packs, work.data_ptr(), need,
                                                       stream_of()))), (cols, seqs, packs, keep)

  def captured(fn):
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
      with torch.cuda.graph(graph, stream=s):
        fn()
    torch.cuda.synchronize()
    return graph

  calls = [pack_call(), grid_call(lib.hbk_sequence_row_grid_n, PAD), grid_call(lib.hbk_sequence_id_grid_n, PAD)]
  graphs = [captured(c[0]) for c in calls]
  pack_bytes = N_COLS * B * 12 + N_COLS * B * T * 4 + valid * 16

  # ---- W = 1 on a real communicator: the drivers by hand -----------------------------------------------------
  coll = hb.distribute.Collective(world_size=1, rank=0)
  w1 = {}
  for name, hashed in (('bucketed', False), ('hash', True)):
    d, _ = batch_of(100, dev)
    d_ids, d_sp = [x[0] for x in d], [x[1] for x in d]
    grads = [torch.randn(B, T, DIM, device=dev, generator=gen) for _ in range(N_COLS)]
    flat = [g.view(B * T, DIM) for g in grads]
    for pad in (False, True):
      if hashed:
        tables = [hb.embedding.HashTable(2 * ROWS, DIM, dev, seed=c) for c in range(N_COLS)]
        drv = hb.embedding.ShardedHashGroupLookup(tables, coll, combiners='sum')
      else:
        shards = [torch.empty(ROWS, DIM, device=dev).uniform_(-1e-3, 1e-3, generator=gen) for _ in range(N_COLS)]
        drv = hb.embedding.ShardedGroupLookup(shards, coll, buckets=[ROWS] * N_COLS, combiners='sum')
      if pad:
        def fwd(i, drv=drv, hashed=hashed, d_ids=d_ids, d_sp=d_sp):
          if hashed:
            grids, _ = hb.embedding.sequence_id_grid(d_ids, d_sp, T, PAD)
          else:
            grids, _ = hb.embedding.sequence_row_grid(d_ids, d_sp, [ROWS] * N_COLS, T, PAD)
          drv(grids)
        bwd = lambda i, drv=drv, flat=flat: drv.backward(flat, apply_lr=LR, emit=False)   # noqa: E731
      else:
        look = hb.embedding.ShardedSequenceLookup(drv, T)
        fwd = lambda i, look=look, d_ids=d_ids, d_sp=d_sp: look(d_ids, d_sp)   # noqa: E731
        bwd = lambda i, look=look, grads=grads: look.backward(grads, apply_lr=LR, emit=False)   # noqa: E731
      fwd(0)
      bwd(0)
      form = f'w1_{name}_{"pad" if pad else "packed"}'
      w1[form + '_fwd'], w1[form + '_bwd_sgd'] = fwd, bwd

  steps = {'pack': lambda i: graphs[0].replay(), 'row_grid': lambda i: graphs[1].replay(),
           'id_grid': lambda i: graphs[2].replay()}
  steps.update(w1)
  t = {k: [] for k in steps}
  for _ in range(args.rounds):
    for k in steps:   # taking turns
      t[k].append(timed(steps[k]))
  coll.close()
  result = {'shape': {'cols': N_COLS, 'rows': ROWS, 'dim': DIM, 'B': B, 'T': T, 'poisson': LAM,
                      'positions': N_COLS * B * T, 'effective_ids': valid, 'pack_bytes': pack_bytes}}
  result.update(summary(t))
  result['pack_gb_per_s'] = round(pack_bytes / float(np.median(t['pack'])) * 1e-3, 1)
  result['w1_ids_sent'] = {'pad': N_COLS * B * T, 'packed': batch_of(100, 'cpu')[1]}

  # ---- W = 8 through the layer -------------------------------------------------------------------------------
  tw = world_forms(W, [('bucketed_packed', False, False), ('bucketed_pad', False, True),
                       ('hash_packed', True, False), ('hash_pad', True, True)])
  result['world'] = W
  result.update(summary({f'w{W}_{k}': v for k, v in tw.items()}))
  result[f'w{W}_ids_sent'] = {'pad': W * N_COLS * B * T,
                              'packed': sum(batch_of(100 + r, 'cpu')[1] for r in range(W))}
  report(result)


if __name__ == '__main__':
  main()
