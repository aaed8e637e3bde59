"""16-bit hash tables behind runs, sequences and the sharded plan (hbk_hash_translate_runs_lowp_n,
hbk_hash_translate_sequence_lowp_n, LowpShardedHashGroupLookup), in one process, the forms taking turns:

  runs          the owner translate of 26 tables x 8 runs x 8 192 ids (capacity 131 072, slab 8, dim 16) through the
                runs entry, fp32 against bf16 against fp16: every id resident, and a first batch (the key arrays are
                emptied before every timed call; only the call is timed)
  sequence      the same through the sequence entry in the shape of profiles/hash_sequence.txt: 4 columns, B = 8192,
                T = 50, dim 16, Poisson(40) lengths, tables of 524 288 slots -- HashSequenceLookup's translate launch
                alone, bound once
  step          the W = 1 step on the real communicator, forward + backward with SGD and with row-wise Adagrad, 26
                columns x `--batch` ids, at dim 16 / 64 / 128: fp32 ShardedHashGroupLookup against
                LowpShardedHashGroupLookup (bf16) with wire='table' and wire='float'.  At W = 1 no row crosses a link:
                the halved wire traffic of wire='table' CANNOT be measured on one GPU, and is not
  --regression  ONLY the unchanged fp32 paths -- the fp32 runs entry (resident, first batch) and the fp32 sharded hash
                step at W = 1 -- one JSON line on stdout, nothing written, nothing imported that the parent commit
                lacks: run from a checkout of the parent and from this commit, taking turns

Timed regions: `--steps` operations between HIP events after `--warmup` (a first batch: one event pair per call, the
reset outside it); `--rounds` rounds; medians with min / max.  Prints one JSON line and appends it to `--out`.

  python tools/bench_hash_lowp_sharded.py [--rounds 7 --steps 50 --warmup 10]
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

EMPTY = -2 ** 63


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--steps', type=int, default=50)
  p.add_argument('--warmup', type=int, default=10)
  p.add_argument('--first-steps', type=int, default=10)
  p.add_argument('--cols', type=int, default=26)
  p.add_argument('--runs', type=int, default=8)
  p.add_argument('--batch', type=int, default=8192)
  p.add_argument('--regression', action='store_true')
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_lowp_sharded.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_lowp_sharded.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  cols, slab_size = args.cols, 8
  rng = np.random.RandomState(781)
  lib = _lib.lib()
  F32, BF16, FP16 = torch.float32, torch.bfloat16, torch.float16
  names = {F32: 'fp32', BF16: 'bf16', FP16: 'fp16'}

  def summary(us):
    return {'us': round(float(np.median(us)), 2), 'min_max_us': [round(min(us), 2), round(max(us), 2)]}

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

  def timed_first(reset, step):
    """A call on emptied tables: the reset outside the event pair."""
    total = 0.0
    for k in range(args.first_steps + 2):
      reset()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      step()
      e1.record()
      e1.synchronize()
      if k >= 2:
        total += e0.elapsed_time(e1) * 1e3
    return total / args.first_steps

  def alternate(forms, timer=timed_events):
    t = {k: [] for k in forms}
    for _ in range(args.rounds):
      for k, step in forms.items():
        t[k].append(timer(*step) if isinstance(step, tuple) else timer(step))
    return {k: summary(v) for k, v in t.items()}

  def table(capacity, dim, dtype, **kw):
    if dtype == F32:
      return hb.embedding.HashTable(capacity, dim, dev, slab_size=slab_size, **kw)
    return hb.embedding.HashTable(capacity, dim, dev, slab_size=slab_size, dtype=dtype, **kw)

  def emptier(tables):
    def reset():
      for t in tables:
        t.keys.fill_(EMPTY)
        t.counts.zero_()
    return reset

  # ---- 1. the runs entry ------------------------------------------------------------------------------------------
  def runs_forms(dtypes, dim=16):
    n_keys, n_runs = args.runs * args.batch, args.runs
    stream = _lib.current_stream(dev)
    keys = [torch.from_numpy(np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n_keys + 64, dtype=np.int64))[:n_keys]
                             .copy()).to(dev) for _ in range(cols)]
    keys = [k[torch.randperm(n_keys, device=dev)].contiguous() for k in keys]
    resident, first, keep = {}, {}, []
    for dtype in dtypes:
      tables = [table(2 * n_keys, dim, dtype) for _ in range(cols)]
      slots = [torch.empty(n_keys, dtype=torch.int64, device=dev) for _ in range(cols)]
      col = (_lib.HashColumn * cols)()
      runs, ptrs = [], []
      for c, t in enumerate(tables):
        t._describe(col[c])   # pylint: disable=protected-access
        r = (_lib.HashRun * n_runs)()
        for q in range(n_runs):
          r[q].keys = keys[c].data_ptr() + 8 * q * args.batch
          r[q].slots = slots[c].data_ptr() + 8 * q * args.batch
          r[q].n_keys = args.batch
        runs.append(r)
        ptrs.append(C.cast(r, C.c_void_p).value)
      n_runs_arr, run_ptrs = _lib.i32_array([n_runs] * cols), _lib.ptr_array(ptrs)
      codes = None if dtype == F32 else (C.c_int32 * cols)(*[hb.embedding.hashtable.LOWP_DTYPES[dtype]] * cols)
      keep.append((tables, slots, col, runs, n_runs_arr, run_ptrs, codes))

      def call(col=col, n_runs_arr=n_runs_arr, run_ptrs=run_ptrs, codes=codes):
        if codes is None:
          _lib.check(lib.hbk_hash_translate_runs_n(cols, col, None, None, n_runs_arr, run_ptrs, 1, stream))
        else:
          _lib.check(lib.hbk_hash_translate_runs_lowp_n(cols, col, None, None, codes, n_runs_arr, run_ptrs, 1, stream))
      call()
      torch.cuda.synchronize()
      assert all(t.size() == n_keys and t.failed() == 0 for t in tables)
      resident[names[dtype]] = call
      first[names[dtype]] = (emptier(tables), call)
    # the resident forms first (the tables are full), then the first-batch forms, which empty them
    out = {'resident': alternate(resident), 'first_batch': alternate(first, timed_first)}
    del keep
    return out

  # ---- 2. the sequence entry --------------------------------------------------------------------------------------
  def sequence_forms(dtypes, n_cols=4, B=8192, T=50, dim=16, n_ids=262144):
    stream = _lib.current_stream(dev)
    lens = [rng.poisson(40, size=B) for _ in range(n_cols)]
    splits = [torch.from_numpy(np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)).to(dev) for ln in lens]
    pools = [np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n_ids + 64, dtype=np.int64))[:n_ids] for _ in range(n_cols)]
    ids = [torch.from_numpy(pl[rng.randint(0, n_ids, size=int(ln.sum()))]).to(dev) for pl, ln in zip(pools, lens)]
    resident, first, keep = {}, {}, []
    for dtype in dtypes:
      tables = [table(2 * n_ids, dim, dtype) for _ in range(n_cols)]
      hsl = hb.embedding.HashSequenceLookup(tables, T)
      hsl(ids, splits)                                       # binds; every id of the batch resident from here on
      torch.cuda.synchronize()
      keep.append(hsl)

      def call(hsl=hsl):
        hsl._plan.launch(True, stream)   # pylint: disable=protected-access
      resident[names[dtype]] = call
      first[names[dtype]] = (emptier(tables), call)
    out = {'resident': alternate(resident), 'first_batch': alternate(first, timed_first),
           'positions': n_cols * B * T, 'positions_with_an_id': int(sum(np.minimum(ln, T).sum() for ln in lens))}
    del keep
    return out

  # ---- 3. the W = 1 step ------------------------------------------------------------------------------------------
  def make_step(form, comm, dim, optimizer):
    g = torch.Generator(device='cpu').manual_seed(1000)
    pool = 4 * args.batch
    ids = [(torch.randint(0, pool, (args.batch,), generator=g, dtype=torch.int64) * 2654435761 - (1 << 40)).to(dev)
           for _ in range(cols)]
    grads = [torch.randn(args.batch, dim, device=dev) for _ in range(cols)]
    outs = [torch.empty(args.batch, dim, device=dev) for _ in range(cols)]
    rows = 2 * pool
    dtype = F32 if form == 'fp32' else BF16
    tables = [table(rows, dim, dtype) for _ in range(cols)]
    kw = {}
    if optimizer == 'rowwise_adagrad':
      kw = dict(row_accums=[torch.full((t.capacity, 1), 0.1, device=dev) for t in tables],
                rowwise_adagrad=hb.embedding.RowwiseAdagrad())
    if form == 'fp32':
      drv = hb.embedding.ShardedHashGroupLookup(tables, comm, combiners='sum', **kw)
    else:
      drv = hb.embedding.LowpShardedHashGroupLookup(tables, comm, combiners='sum',
                                                    wire='table' if form == 'bf16_wire_table' else 'float', **kw)
    bound = drv.bind(ids, None, outs)

    def step():
      drv.launch(bound)
      drv.backward(grads, apply_lr=0.01, optimizer=optimizer, emit=False)
    return drv, step

  def step_w1(forms, dim, optimizer):
    comm = hb.distribute.Collective(world_size=1, rank=0)
    made = {k: make_step(k, comm, dim, optimizer) for k in forms}
    out = alternate({k: s for k, (_, s) in made.items()})
    for d, _ in made.values():
      d.close()
    comm.close()
    torch.cuda.empty_cache()
    return out

  shape = {'cols': cols, 'slab_size': slab_size, 'runs_per_table': args.runs, 'ids_per_run': args.batch,
           'slots_per_table': 2 * args.runs * args.batch, 'step_batch': args.batch}
  if args.regression:
    line = json.dumps({'regression_fp32': {'runs_entry': runs_forms([F32]),
                                           'sharded_hash_step_w1_sgd_dim16': step_w1(['fp32'], 16, 'sgd')['fp32']},
                       'shape': shape, 'rounds': args.rounds, 'steps': args.steps})
    print(line, flush=True)
    return
  result = {'shape': shape, 'rounds': args.rounds, 'steps': args.steps, 'first_steps': args.first_steps,
            'runs_entry_dim16': runs_forms([F32, BF16, FP16])}
  torch.cuda.empty_cache()
  result['sequence_entry'] = sequence_forms([F32, BF16, FP16])
  torch.cuda.empty_cache()
  result['step_w1'] = {}
  for dim in (16, 64, 128):
    for optimizer in ('sgd', 'rowwise_adagrad'):
      result['step_w1'][f'dim{dim}_{optimizer}'] = step_w1(['fp32', 'bf16_wire_table', 'bf16_wire_float'], dim, optimizer)
  result['not_measured'] = 'the halved wire traffic of wire=table: at W = 1 no row crosses a link'
  line = json.dumps(result)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
