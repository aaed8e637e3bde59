"""Sharded lookups with 16-bit outputs, measured in one process with the forms taking turns.

(a) `stitch`: hbk_lookup_fwd_runs_out16 alone, as replays of captured graphs -- 26 columns x 65536 ids over 8 runs of
    one buffer whose bases are multiples of 4 and not of 8 elements, rows read through a permutation, dim 16 / 64 /
    128, and a ragged Poisson(8) dim-16 case -- with chunk_elems 4 and 8, over fp32 and bf16 rows, against
      f32            the fp32 stitch (hbk_group_lookup_fwd over the runs)
      f32+cast       the fp32 stitch followed by .to(bfloat16): what a user does without this entry
      lowp_runs      hbk_lowp_lookup_fwd_runs (bf16 rows in, fp32 rows out)
(b) `step`: the W = 1 forward on the real communicator, 26 columns x 1M rows x dim 16 and 64, batch 65536: fp32
    outputs, fp32 outputs + cast, out_dtype=bfloat16.  At W = 1 no row crosses a link: this times the kernels and the
    host path of the step, not the wire.
(c) `fp32step`: (b)'s first form alone, printed as one JSON line, for runs in turns against a checkout of the parent
    (`--root`).

Medians of `--rounds` (default 7) with min - max over windows of `--steps` calls (default 100; the numbers recorded
in the profile were taken with --steps 20, as their header line says).  Appends to `--out` (default profiles/sharded_out16.txt).
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
  p.add_argument('--steps', type=int, default=100)
  p.add_argument('--warmup', type=int, default=5)
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--cases', default='stitch,step')
  p.add_argument('--root', default=HERE, help='the tree whose package is measured')
  p.add_argument('--out', default=os.path.join(HERE, 'profiles', 'sharded_out16.txt'))
  args = p.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  lib = _lib.lib()
  dev = torch.device('cuda:0')
  cols, rows, batch, n_runs = 26, 1_000_000, 65536, 8
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

  def take_turns(case, forms):
    t = {k: [] for k in forms}
    for _ in range(args.rounds):
      for k in forms:
        t[k].append(timed(forms[k]))
    for k in forms:
      med = float(np.median(t[k]))
      result[f'{case}_{k}'] = {'us': round(med, 2), 'min_max_us': [round(min(t[k]), 2), round(max(t[k]), 2)]}
      lines.append(f'{case:16s} {k:14s} {med:9.2f} us  (min {min(t[k]):.2f} - max {max(t[k]):.2f})')

  def stream():
    return _lib.current_stream(dev)

  def stitch_case(dim, ragged):
    per_run = batch // n_runs
    buf16 = torch.empty(cols * batch * dim + 8, device=dev).uniform_(-1e-3, 1e-3, generator=gen).to(torch.bfloat16)
    buf32 = buf16.float()
    index = [torch.randperm(batch, device=dev, generator=gen).to(torch.int32) for _ in range(cols)]
    n_seg, splits = batch, None
    if ragged:
      n_seg = batch // 8
      lens = torch.poisson(torch.full((n_seg,), 8.0, device=dev), generator=gen).long()
      lens[-1] += batch - int(lens.sum()) if int(lens.sum()) <= batch else 0
      sp = torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)
      sp[1:] = torch.cumsum(lens, 0).clamp(max=batch)
      splits = sp.to(torch.int32)
    start = torch.arange(n_runs, device=dev, dtype=torch.int64) * per_run
    # peer-major: run k of column c sits behind run k of the columns before it; + 4: bases on 4, not on 8 elements
    bases = [(torch.arange(n_runs, device=dev, dtype=torch.int64) * cols + c) * per_run * dim + 4 for c in range(cols)]
    out16 = [torch.empty(n_seg, dim, device=dev, dtype=torch.bfloat16) for _ in range(cols)]
    out32 = [torch.empty(n_seg, dim, device=dev) for _ in range(cols)]
    n_ids = batch if not ragged else int(splits[-1])

    def runs_cols(table, code, chunk):
      a = (_lib.Out16RunsColumn * cols)()
      for c in range(cols):
        d = a[c].col
        d.table, d.table_dtype, d.dim, d.rows = table.data_ptr(), code, dim, batch
        d.ids, d.ids_dtype, d.n_ids, d.n_segments, d.divisor = index[c].data_ptr(), _lib.INT32, n_ids, n_seg, 1
        d.row_splits = None if splits is None else splits.data_ptr()
        d.out, d.out_dtype, d.chunk_elems = out16[c].data_ptr(), _lib.LOWP_BF16, chunk
        a[c].run_start, a[c].run_base, a[c].n_runs = start.data_ptr(), bases[c].data_ptr(), n_runs
      return a
    f32 = (_lib.LookupColumn * cols)()
    lr = (_lib.LowpLookupRunsColumn * cols)()
    for c in range(cols):
      for d, table in ((f32[c], buf32), (lr[c].col, buf16)):
        d.table, d.rows, d.dim, d.ids = table.data_ptr(), batch, dim, index[c].data_ptr()
        d.ids_dtype, d.n_ids, d.n_segments, d.divisor = _lib.INT32, n_ids, n_seg, 1
        d.row_splits = None if splits is None else splits.data_ptr()
        d.out = out32[c].data_ptr()
      lr[c].col.table_dtype = _lib.LOWP_BF16
      for d in (f32[c], lr[c]):
        d.run_start, d.run_base, d.n_runs = start.data_ptr(), bases[c].data_ptr(), n_runs
    keep = {k: runs_cols(t, code, w) for k, t, code, w in (
      ('f32_w4', buf32, _lib.OUT16_TABLE_FP32, 4), ('f32_w8', buf32, _lib.OUT16_TABLE_FP32, 8),
      ('bf16_w4', buf16, _lib.LOWP_BF16, 4), ('bf16_w8', buf16, _lib.LOWP_BF16, 8))}

    def fp32_cast():
      _lib.check(lib.hbk_group_lookup_fwd(cols, f32, stream()))
      for c in range(cols):
        out16[c].copy_(out32[c])
    forms = {k: graphed(lambda a=a: _lib.check(lib.hbk_lookup_fwd_runs_out16(cols, a, stream())))
             for k, a in keep.items()}
    forms['f32'] = graphed(lambda: _lib.check(lib.hbk_group_lookup_fwd(cols, f32, stream())))
    forms['f32+cast'] = graphed(fp32_cast)
    forms['lowp_runs'] = graphed(lambda: _lib.check(lib.hbk_lowp_lookup_fwd_runs(cols, lr, stream())))
    take_turns(f'stitch_d{dim}' + ('_ragged' if ragged else ''), forms)
    del forms
    torch.cuda.empty_cache()

  def step_case(which, dim):
    E = hb.embedding
    coll = hb.distribute.Collective(world_size=1, rank=0)
    ids = [torch.randint(0, 1 << 40, (batch,), device=dev, dtype=torch.int64, generator=gen) for _ in range(cols)]
    tables = [torch.empty(rows, dim, device=dev).uniform_(-1e-3, 1e-3, generator=gen) for _ in range(cols)]
    o32 = [torch.empty(batch, dim, device=dev) for _ in range(cols)]
    o16 = [torch.empty(batch, dim, device=dev, dtype=torch.bfloat16) for _ in range(cols)]
    f32 = E.ShardedGroupLookup(tables, coll, buckets=[rows] * cols)
    b32 = f32.bind(ids, None, o32)
    forms = {'fp32': lambda: f32.launch(b32)}
    drivers = [f32]
    if which == 'step':
      new = E.ShardedGroupLookup(tables, coll, buckets=[rows] * cols, out_dtype=torch.bfloat16)
      b16 = new.bind(ids, None, o16)
      drivers.append(new)

      def cast():
        f32.launch(b32)
        for c in range(cols):
          o16[c].copy_(o32[c])
      forms['fp32+cast'] = cast
      forms['out_bf16'] = lambda: new.launch(b16)
    take_turns(f'step_fwd_d{dim}', forms)
    for d in drivers:
      d.close()
    coll.close()

  for name in args.cases.split(','):
    if name == 'stitch':
      for dim, ragged in ((16, False), (64, False), (128, False), (16, True)):
        stitch_case(dim, ragged)
    else:
      for dim in (16, 64):
        step_case(name, dim)
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  if 'fp32step' not in args.cases:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
      f.write(f'# tools/bench_sharded_out16.py --cases {args.cases} --steps {args.steps} --warmup {args.warmup} '
              f'--rounds {args.rounds}: one process, forms taking turns, medians of {args.rounds}\n')
      f.write('\n'.join(lines) + '\n')
  print(json.dumps(result))


if __name__ == '__main__':
  main()
