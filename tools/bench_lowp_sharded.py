"""Low-precision sharded tables, measured in one process with the forms taking turns.

(a) `kernels`: the two new kernels alone, as replays of captured graphs -- 26 columns x 65536 ids, dim 16 / 64 / 128,
    1M-row tables:
      gather   hbk_lowp_gather_rows_n against hbk_lowp_lookup_fwd (bf16 rows in, fp32 rows out) and the fp32 gather
               with HBK_LOOKUP_OUT_HALF
      stitch   hbk_lowp_lookup_fwd_runs against the fp32 stitch and the HBK_LOOKUP_TABLE_HALF stitch, over 8 runs
    with GB/s of the byte model  ids + rows read + rows written  (ids 8 B for the gather, 4 B for the stitch).
(b) `step`: the W = 1 step on the real communicator, 26 columns x 1M rows x dim 16, batch 65536 -- the forward, and
    the backward + SGD step -- for fp32 shards on the fp32 wire, fp32 shards on the fp16 wire, bf16 shards with
    wire='float' and bf16 shards with wire='table'.  At W = 1 no row crosses a link: this times the kernels and the
    host path of the step, not the wire.
(c) `fp32step`: (b)'s first form alone, printed as one JSON line: what a job runs in turns from this tree and from a
    checkout of the parent (`--root`) to see that the fp32 step did not move.

Medians of `--rounds` (default 7) with min - max.  Appends to `--out` (default profiles/lowp_sharded.txt).

  python tools/bench_lowp_sharded.py [--cases kernels,step] [--steps 20 --warmup 5 --rounds 7] [--root DIR]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--steps', type=int, default=20)
  p.add_argument('--warmup', type=int, default=5)
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--cases', default='kernels,step')
  p.add_argument('--root', default=HERE, help='the tree whose package is measured')
  p.add_argument('--out', default=os.path.join(HERE, 'profiles', 'lowp_sharded.txt'))
  args = p.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  E = hb.embedding
  lib = _lib.lib()
  dev = torch.device('cuda:0')
  cols, rows, batch = 26, 1_000_000, 65536
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)
  lines, result = [], {}

  def graphed(fn):
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
      with torch.cuda.graph(g, stream=s):
        fn()
    torch.cuda.synchronize()
    return g.replay

  def timed(fn):
    for _ in range(args.warmup):
      fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
      fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps   # us per call

  def take_turns(case, forms, model_bytes=None):
    t = {k: [] for k in forms}
    for _ in range(args.rounds):
      for k in forms:
        t[k].append(timed(forms[k]))
    for k in forms:
      med = float(np.median(t[k]))
      entry = {'us': round(med, 2), 'min_max_us': [round(min(t[k]), 2), round(max(t[k]), 2)]}
      line = f'{case:16s} {k:14s} {med:9.2f} us  (min {min(t[k]):.2f} - max {max(t[k]):.2f})'
      if model_bytes is not None:
        entry['gb_s'] = round(model_bytes[k] / med / 1e3, 1)
        line += f'   {model_bytes[k] / 1e6:7.1f} MB  {entry["gb_s"]:7.1f} GB/s'
      result[f'{case}_{k}'] = entry
      lines.append(line)

  def stream():
    return _lib.current_stream(dev)

  # ---- (a) ---------------------------------------------------------------------------------------------------------
  def kernels_case(dim):
    t16 = [torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen).to(torch.bfloat16)
           for _ in range(cols)]
    t32 = [t.float() for t in t16]
    ids = [torch.randint(0, 1 << 40, (batch,), device=dev, dtype=torch.int64, generator=gen) for _ in range(cols)]
    out16 = [torch.empty(batch, dim, device=dev, dtype=torch.int16) for _ in range(cols)]
    out32 = [torch.empty(batch, dim, device=dev) for _ in range(cols)]
    g = (_lib.LowpGatherColumn * cols)()
    lf = (_lib.LowpLookupColumn * cols)()
    fh = (_lib.LookupColumn * cols)()
    for c in range(cols):
      g[c].table, g[c].dim, g[c].rows, g[c].ids, g[c].n_ids = t16[c].data_ptr(), dim, rows, ids[c].data_ptr(), batch
      g[c].ids_dtype, g[c].bucket, g[c].divisor, g[c].out = _lib.INT64, rows, 1, out16[c].data_ptr()
      lf[c].table, lf[c].table_dtype, lf[c].dim, lf[c].rows = t16[c].data_ptr(), _lib.LOWP_BF16, dim, rows
      lf[c].ids, lf[c].ids_dtype, lf[c].n_ids, lf[c].n_segments = ids[c].data_ptr(), _lib.INT64, batch, batch
      lf[c].bucket, lf[c].divisor, lf[c].out = rows, 1, out32[c].data_ptr()
      fh[c].table, fh[c].rows, fh[c].dim, fh[c].ids = t32[c].data_ptr(), rows, dim, ids[c].data_ptr()
      fh[c].ids_dtype, fh[c].n_ids, fh[c].n_segments, fh[c].bucket = _lib.INT64, batch, batch, rows
      fh[c].divisor, fh[c].out, fh[c].half_io = 1, out16[c].data_ptr(), 1

    forms = {'gather16': graphed(lambda: _lib.check(lib.hbk_lowp_gather_rows_n(cols, g, stream()))),
             'lowp_fwd_f32out': graphed(lambda: _lib.check(lib.hbk_lowp_lookup_fwd(cols, lf, stream()))),
             'fp32_out_half': graphed(lambda: _lib.check(lib.hbk_group_lookup_fwd(cols, fh, stream())))}
    n = cols * batch
    take_turns(f'gather_d{dim}', forms, {'gather16': n * (8 + 4 * dim),
                                         'lowp_fwd_f32out': n * (8 + 6 * dim), 'fp32_out_half': n * (8 + 6 * dim)})
    del forms, t32, t16
    torch.cuda.empty_cache()
    # the stitch: 65536 received rows per column in 8 runs of one buffer, read through a permutation
    n_runs = 8
    per_run = batch // n_runs
    buf16 = torch.empty(cols * batch * dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen).to(torch.bfloat16)
    bufh = buf16.to(torch.float16)
    buf32 = buf16.float()
    index = [torch.randperm(batch, device=dev, generator=gen).to(torch.int32) for _ in range(cols)]
    start = torch.arange(n_runs, device=dev, dtype=torch.int64) * per_run
    # peer-major: run k of column c sits behind run k of the columns before it
    bases = [(torch.arange(n_runs, device=dev, dtype=torch.int64) * cols + c) * per_run * dim for c in range(cols)]
    lr = (_lib.LowpLookupRunsColumn * cols)()
    f32 = (_lib.LookupColumn * cols)()
    f16 = (_lib.LookupColumn * cols)()
    for c in range(cols):
      d = lr[c].col
      d.table, d.table_dtype, d.dim, d.rows = buf16.data_ptr(), _lib.LOWP_BF16, dim, batch
      d.ids, d.ids_dtype, d.n_ids, d.n_segments, d.divisor = index[c].data_ptr(), _lib.INT32, batch, batch, 1
      d.out = out32[c].data_ptr()
      lr[c].run_start, lr[c].run_base, lr[c].n_runs = start.data_ptr(), bases[c].data_ptr(), n_runs
      for dst, table, half in ((f32[c], buf32, 0), (f16[c], bufh, 2)):
        dst.table, dst.rows, dst.dim, dst.ids = table.data_ptr(), batch, dim, index[c].data_ptr()
        dst.ids_dtype, dst.n_ids, dst.n_segments, dst.divisor = _lib.INT32, batch, batch, 1
        dst.out, dst.half_io = out32[c].data_ptr(), half
        dst.run_start, dst.run_base, dst.n_runs = start.data_ptr(), bases[c].data_ptr(), n_runs
    forms = {'stitch16_runs': graphed(lambda: _lib.check(lib.hbk_lowp_lookup_fwd_runs(cols, lr, stream()))),
             'fp32_stitch': graphed(lambda: _lib.check(lib.hbk_group_lookup_fwd(cols, f32, stream()))),
             'table_half': graphed(lambda: _lib.check(lib.hbk_group_lookup_fwd(cols, f16, stream())))}
    take_turns(f'stitch_d{dim}', forms, {'stitch16_runs': n * (4 + 6 * dim), 'fp32_stitch': n * (4 + 8 * dim),
                                         'table_half': n * (4 + 6 * dim)})
    del forms
    torch.cuda.empty_cache()

  # ---- (b), (c) ------------------------------------------------------------------------------------------------------
  def step_case(which):
    dim = 16
    coll = hb.distribute.Collective(world_size=1, rank=0)
    ids = [torch.randint(0, 1 << 40, (batch,), device=dev, dtype=torch.int64, generator=gen) for _ in range(cols)]
    grads = [torch.randn(batch, dim, device=dev, generator=gen) for _ in range(cols)]
    outs = [torch.empty(batch, dim, device=dev) for _ in range(cols)]

    def tables(dtype):
      return [torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen).to(dtype) for _ in range(cols)]
    drivers = {'fp32_fp32wire': E.ShardedGroupLookup(tables(torch.float32), coll, buckets=[rows] * cols)}
    if which == 'step':
      drivers['fp32_fp16wire'] = E.ShardedGroupLookup(tables(torch.float32), coll, buckets=[rows] * cols,
                                                      wire_dtype=torch.float16)
      drivers['bf16_float'] = E.LowpShardedGroupLookup(tables(torch.bfloat16), coll, buckets=[rows] * cols, wire='float')
      drivers['bf16_table'] = E.LowpShardedGroupLookup(tables(torch.bfloat16), coll, buckets=[rows] * cols, wire='table')
    fwd, bwd = {}, {}
    for k, drv in drivers.items():
      bound = drv.bind(ids, None, outs)
      fwd[k] = lambda d=drv, b=bound: d.launch(b)
      bwd[k] = lambda d=drv: d.backward(grads, apply_lr=1e-4, emit=False)
      fwd[k]()
      bwd[k]()
    take_turns('step_fwd', fwd)
    # (the backward differentiates the plan's last forward: every form ran one above)
    take_turns('step_bwd_sgd', bwd)
    for drv in drivers.values():
      drv.close()
    coll.close()

  for name in args.cases.split(','):
    if name == 'kernels':
      for dim in (16, 64, 128):
        kernels_case(dim)
    else:
      step_case(name)
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  if 'fp32step' not in args.cases:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
      f.write(f'# tools/bench_lowp_sharded.py --cases {args.cases} --steps {args.steps} --warmup {args.warmup} '
              f'--rounds {args.rounds}: one process, forms taking turns, medians of {args.rounds}\n')
      f.write('\n'.join(lines) + '\n')
  print(json.dumps(result))


if __name__ == '__main__':
  main()
