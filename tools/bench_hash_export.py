"""Export and import of hash tables (hbk_hash_export_n, hbk_hash_store_rows_n) against the torch form, in one
process, on the shape of tools/bench_hash_rehash.py: 26 expiring tables x 131 072 slots, dim 16, slab_size 8,
65 536 resident keys each (load 0.5), two dim-16 companions per table.

  export        export_call      hash_export(tables, slots=companions): one host read, allocations, three launches,
                                 one host read
                export_launches  the entry alone (count, scan, write) into buffers prepared before the timed region
                torch            per table items() plus the indexing of last_seen, freq and the companions
  delta         1 %, 10 % and 100 % of the keys seen at the step of `since`: the call and the launches alone
  import        import_items     per table into fresh tables of twice the capacity (translate + one store launch)
                load             per table load(keys, rows) plus the indexing of last_seen, freq and the companions
                hash_rehash      growth of the source tables to twice the capacity: the device-side yardstick

Every timed region is one operation between its own HIP events; `--rounds` rounds with the forms taking turns;
medians with min / max.  Byte model of the three launches: per source slot 8 B of key (+ 4 B of last_seen for a
delta), each read twice; per exported key 8 B of key, 8 B of slot and twice the row bytes of every move; TB/s
against 8 TB/s.  Prints one JSON line and appends it to `--out` (default profiles/hash_export.txt).

  python tools/bench_hash_export.py [--rounds 7]
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


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--cols', type=int, default=26)
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_export.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_export.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  cols, batch, dim, slab_size = args.cols, 65536, 16, 8
  capacity = 2 * batch
  rng = np.random.RandomState(779)
  stream = _lib.current_stream(dev)
  lib = _lib.lib()
  HashTable = hb.embedding.HashTable

  def distinct(n):
    k = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n + 64, dtype=np.int64))[:n].copy()
    return torch.from_numpy(k).to(dev)[torch.randperm(n, device=dev)].contiguous()
  resident = [distinct(batch) for _ in range(cols)]

  def build():
    tables, comps = [], []
    for r in resident:
      x = HashTable(capacity, dim, dev, slab_size=slab_size, expiring=True)
      x.set_step(100)
      x.lookup_or_insert(r)
      assert x.size() == batch and x.failed() == 0
      tables.append(x)
      comps.append([torch.rand((capacity, dim), device=dev) + 1, torch.randn((capacity, dim), device=dev)])
    return tables, comps

  def once(prepare, step):
    prepare()
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
      out['bytes'] = nbytes
      out['TBps'] = round(nbytes / med * 1e-6, 3)
      out['of_8TBps'] = round(nbytes / med * 1e-6 / 8, 4)
    return out

  def run(forms, nbytes=None):
    t = {k: [] for k in forms}
    for k, (prep, step) in forms.items():   # one untimed pass of everything: allocator, first launches
      once(prep, step)
    for _ in range(args.rounds):
      for k, (prep, step) in forms.items():   # the forms take turns
        t[k].append(once(prep, step))
    return {k: summary(v, nbytes if k.endswith('launches') else None) for k, v in t.items()}

  row_bytes = 4 * (dim + 1 + 1 + 2 * dim)

  def model(n_keys, delta):
    return cols * (capacity * (8 + (4 if delta else 0)) * 2 + n_keys * (8 + 8 + 2 * row_bytes))

  def describe(tables, comps, since):
    """Output buffers and descriptors of the entry alone."""
    arr = (_lib.HashExportColumn * cols)()
    counts = torch.zeros(cols, dtype=torch.int64, device=dev)
    keep = []
    for c, (x, cs) in enumerate(zip(tables, comps)):
      outs = [torch.empty(batch, dtype=torch.int64, device=dev), torch.empty(batch, dtype=torch.int64, device=dev)]
      moves = [(x.table, torch.empty((batch, dim), device=dev), dim),
               (x.last_seen, torch.empty(batch, dtype=torch.int32, device=dev), 1),
               (x.freq, torch.empty(batch, dtype=torch.int32, device=dev), 1)]
      moves += [(s, torch.empty((batch, dim), device=dev), dim) for s in cs]
      col = arr[c]
      col.keys, col.slab_count, col.slab_size, col.expiring = x.keys.data_ptr(), x.slab_count, x.slab_size, 1
      col.last_seen, col.since, col.n_moves = x.last_seen.data_ptr(), since, len(moves)
      for m, (s, d, words) in enumerate(moves):
        col.moves[m].src, col.moves[m].dst, col.moves[m].words = s.data_ptr(), d.data_ptr(), words
      col.out_keys, col.out_slots, col.out_capacity = outs[0].data_ptr(), outs[1].data_ptr(), batch
      col.count = counts.data_ptr() + 8 * c
      keep.append((outs, moves))
    nbytes = C.c_size_t()
    _lib.check(lib.hbk_hash_export_workspace_bytes(cols, arr, C.byref(nbytes)))
    workspace = torch.empty(nbytes.value // 8, dtype=torch.int64, device=dev)
    return arr, workspace, counts, keep

  def torch_export(tables, comps):
    out = []
    for x, cs in zip(tables, comps):
      keys, rows = x.items()
      at = x.find(keys)
      out.append((keys, rows, x.last_seen[at], x.freq[at], [s[at] for s in cs]))
    return out

  nothing = lambda: None   # noqa: E731
  tables, comps = build()
  result = {'shape': {'cols': cols, 'slots_per_col': capacity, 'keys_per_col': batch, 'dim': dim, 'slab_size': slab_size,
                      'companions': 2, 'moves_per_table': 5, 'row_bytes_per_key': row_bytes}, 'rounds': args.rounds}

  # ---- full export
  arr, workspace, counts, keep = describe(tables, comps, 0)
  forms = {'export_call': (nothing, lambda: hb.embedding.hash_export(tables, slots=comps)),
           'export_launches': (nothing, lambda: _lib.check(lib.hbk_hash_export_n(cols, arr, workspace.data_ptr(), stream))),
           'torch': (nothing, lambda: torch_export(tables, comps))}
  out = run(forms, model(batch, False))
  assert counts.tolist() == [batch] * cols
  out['torch_over_export_call'] = round(out['torch']['us'] / out['export_call']['us'], 2)
  result['export'] = out
  exports = hb.embedding.hash_export(tables, slots=comps)
  del arr, workspace, counts, keep

  # ---- deltas: 1 %, 10 %, 100 % of the keys seen at step 200
  result['delta'] = {}
  for pct in (1, 10, 100):
    dirty = batch * pct // 100
    for x, r in zip(tables, resident):
      x.last_seen.fill_(100)
      x.set_step(200)
      x.lookup_or_insert(r[:dirty].contiguous())
    arr, workspace, counts, keep = describe(tables, comps, 200)
    forms = {'delta_call': (nothing, lambda: hb.embedding.hash_export(tables, [200] * cols, comps)),
             'delta_launches': (nothing, lambda: _lib.check(lib.hbk_hash_export_n(cols, arr, workspace.data_ptr(), stream)))}
    out = run(forms, model(dirty, True))
    assert counts.tolist() == [dirty] * cols
    result['delta'][f'{pct}pct'] = out
    del arr, workspace, counts, keep
  torch.cuda.empty_cache()

  # ---- import into fresh tables of twice the capacity
  state = {}

  def fresh():
    state['tables'] = [HashTable(2 * capacity, dim, dev, slab_size=slab_size, expiring=True) for _ in range(cols)]
    state['comps'] = [[torch.full((2 * capacity, dim), 0.1, device=dev), torch.zeros((2 * capacity, dim), device=dev)]
                      for _ in range(cols)]

  def import_step():
    for x, cs, e in zip(state['tables'], state['comps'], exports):
      x.import_items(e, slots=cs, assume_distinct=True)

  def load_step():
    for x, cs, e in zip(state['tables'], state['comps'], exports):
      to = x.load(e.keys, e.rows)
      x.last_seen[to] = e.last_seen
      x.freq[to] = e.freq
      for d, s in zip(cs, e.slots):
        d[to] = s

  NAMES = ('keys', 'table', 'last_seen', 'freq', 'counts', 'stats')
  saved = [{n: getattr(x, n) for n in NAMES} for x in tables]

  def restore():
    for x, s in zip(tables, saved):
      for n in NAMES:
        setattr(x, n, s[n])
      x.slab_size, x.slab_count, x.capacity = slab_size, capacity // slab_size, capacity

  pairs = [[(a, 0.1), (b, 0.0)] for a, b in comps]
  forms = {'import_items': (fresh, import_step), 'load': (fresh, load_step),
           'hash_rehash': (restore, lambda: hb.embedding.hash_rehash(tables, [2 * capacity] * cols, None, pairs))}
  out = run(forms)
  assert all(x.size() == batch for x in state['tables'])
  out['load_over_import_items'] = round(out['load']['us'] / out['import_items']['us'], 2)
  result['import'] = out

  line = json.dumps(result)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
