"""Spilling to a host tier (hbk_hash_evict_to_select_n / hbk_hash_spill_n, HashSpillStore, fault_in) in one
process, the forms taking turns, on the shape of tools/bench_hash_evict_to.py and profiles/hash_rehash.txt: 26
expiring tables x 131 072 slots, dim 16, slab_size 8, two dim-16 companions per table, filled to load 0.75 (98 304
keys each), last_seen spread evenly over 64 steps; the bound is 0.5 x capacity, so 22 whole steps (33 792 keys per
table) leave.

Every call runs on freshly restored tables.  Device forms are timed between their own events, host forms (the
copy into the store, fault_in) with the wall clock between two synchronisations; medians of 7:
  select        hash_evict_to_select over the 26 tables: the clear launch and the three digit passes, no sweep
  spill_n       hbk_hash_spill_n ALONE (descriptors, selection and outputs prepared): count, scan, write, sweep.
                us and TB/s of its byte model: per source slot 16 B read three times (count, write, sweep), per
                spilled key the export's bytes (row and companions read and written, key, slot, last_seen, freq
                written) plus the sweep's resets (key, last_seen, freq, companions)
  hash_spill    the whole Python call a user makes: select, one host read, allocation, hbk_hash_spill_n, one host read
  evict_to      hash_evict_to of the same state: the price of evicting without keeping anything
  export_mask   what could be written without the entries to keep the rows: a full hash_export of the tables,
                hash_evict_to with reports, one host read of the cuts, a torch mask last_seen <= cut over every export
  put           the exports of one hash_spill copied into 26 pinned HashSpillStores (device-to-host and the merge)
  fault_in      HashTable.fault_in of ONE table for a batch of 65 536 distinct ids of which 1 % / 10 % are in its
                store (the rest resident, and ids never seen where the table holds too few): find, unique, the copy of the
                missed ids, take, import_items

Prints one JSON line and appends it to `--out` (default profiles/hash_spill.txt).

  python tools/bench_hash_spill.py [--repeats 7]
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
  p.add_argument('--repeats', type=int, default=7)
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_spill.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding import hashtable as ht   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_spill.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  cols, capacity, dim, slab_size, n_steps, batch = 26, 131072, 16, 8, 64, 65536
  n_keys, bound = capacity * 3 // 4, capacity // 2
  per_step = n_keys // n_steps
  gone_steps = -(-(n_keys - bound) // per_step)             # whole steps leave
  n_gone = gone_steps * per_step
  rng = np.random.RandomState(779)
  tables = [hb.embedding.HashTable(capacity, dim, dev, slab_size=slab_size, expiring=True) for _ in range(cols)]
  for t in tables:
    keys = np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n_keys + 64, dtype=np.int64))[:n_keys]
    t.set_step(1)
    slots = t.lookup_or_insert(torch.from_numpy(keys.copy()).to(dev))
    assert t.size() == n_keys and t.failed() == 0
    t.last_seen[slots] = torch.from_numpy((rng.permutation(n_keys) % n_steps + 1).astype(np.int32)).to(dev)
    t.set_step(n_steps)
  comps = [[(torch.full((capacity, dim), 0.1, device=dev), 0.1), (torch.zeros((capacity, dim), device=dev), 0.0)]
           for _ in range(cols)]
  plain = [[x for x, _ in c] for c in comps]
  saved = [[x.clone() for x in (t.keys, t.last_seen, t.freq, t.counts, t.table, c[0][0], c[1][0])]
           for t, c in zip(tables, comps)]
  reports = [torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(cols)]

  def restore():
    for t, c, s in zip(tables, comps, saved):
      for x, y in zip((t.keys, t.last_seen, t.freq, t.counts, t.table, c[0][0], c[1][0]), s):
        x.copy_(y)
      t.stats.zero_()

  def on_device(step):
    restore()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3

  # hbk_hash_spill_n alone: the descriptors of hash_spill, built once
  selections = ht.hash_evict_to_select(tables, bound)
  assert all(r.tolist()[3] == n_gone for r in selections)
  raw = (_lib.HashSpillColumn * cols)()
  counts = torch.zeros(cols, dtype=torch.int64, device=dev)
  outs = []
  for c, t in enumerate(tables):
    out = [torch.empty(n_gone, dtype=torch.int64, device=dev), torch.empty(n_gone, dtype=torch.int64, device=dev),
           torch.empty((n_gone, dim), device=dev), torch.empty(n_gone, dtype=torch.int32, device=dev),
           torch.empty(n_gone, dtype=torch.int32, device=dev), torch.empty((n_gone, dim), device=dev),
           torch.empty((n_gone, dim), device=dev)]
    ht._describe_sweep(raw[c], t, 0, comps[c])   # pylint: disable=protected-access
    raw[c].selection = selections[c].data_ptr()
    moves = list(zip([t.table, t.last_seen, t.freq] + plain[c], out[2:]))
    raw[c].n_moves = len(moves)
    for m, (x, y) in enumerate(moves):
      ht._describe_move(raw[c].moves[m], per_slot=x, packed=y, to_packed=True)   # pylint: disable=protected-access
    raw[c].out_keys, raw[c].out_slots, raw[c].out_capacity = out[0].data_ptr(), out[1].data_ptr(), n_gone
    raw[c].count, raw[c].n_evicted = counts.data_ptr() + 8 * c, None
    outs.append(out)
  lib = _lib.lib()
  nbytes = C.c_size_t()
  _lib.check(lib.hbk_hash_spill_workspace_bytes(cols, raw, C.byref(nbytes)))
  workspace = torch.empty(nbytes.value // 8, dtype=torch.int64, device=dev)

  def export_mask():
    exports = ht.hash_export(tables, None, plain)
    ht.hash_evict_to(tables, bound, 0, comps, reports)
    kept = []
    for e, r in zip(exports, torch.stack(reports).tolist()):
      m = (e.last_seen <= r[2]).nonzero().flatten() if r[1] > 0 else e.keys.new_zeros(0)
      kept.append(ht.HashExport(e.keys[m], e.rows[m], e.last_seen[m], e.freq[m], [x[m] for x in e.slots]))
    return kept

  forms = {'select': lambda: ht.hash_evict_to_select(tables, bound, 0, reports),
           'spill_n': lambda: _lib.check(lib.hbk_hash_spill_n(cols, raw, workspace.data_ptr(), _lib.current_stream(dev))),
           'hash_spill': lambda: ht.hash_spill(tables, bound, 0, comps),
           'evict_to': lambda: ht.hash_evict_to(tables, bound, 0, comps, reports),
           'export_mask': export_mask}
  evicts = {'select': 0, 'spill_n': cols * n_gone, 'hash_spill': cols * n_gone, 'evict_to': cols * n_gone,
            'export_mask': cols * n_gone}
  for f in forms.values():   # warm-up: descriptors, scratch, kernels loaded
    on_device(f)
  us = {k: [] for k in forms}
  for _ in range(args.repeats):
    for k, f in forms.items():   # taking turns
      us[k].append(on_device(f))
      assert sum(t.evicted() for t in tables) == evicts[k], k
  assert counts.tolist() == [n_gone] * cols
  result = {'shape': {'cols': cols, 'capacity': capacity, 'keys_per_col': n_keys, 'dim': dim, 'slab_size': slab_size,
                      'companions': 2, 'steps': n_steps, 'bound': bound, 'spilled_per_col': n_gone},
            'repeats': args.repeats}
  for k, v in us.items():
    result[k + '_us'] = round(float(np.median(v)), 2)
    result[k + '_min_max_us'] = [round(min(v), 2), round(max(v), 2)]
  per_key = (3 * dim * 4) + (8 + 8 + 3 * dim * 4 + 4 + 4) + (8 + 4 + 4 + 2 * dim * 4)   # read, written, reset
  model = cols * (capacity * 16 * 3 + n_gone * per_key)
  result['spill_n_bytes'] = model
  result['spill_n_TBps'] = round(model / result['spill_n_us'] * 1e-6, 3)

  # host forms, with the wall clock
  def wall(step, before=None):
    if before is not None:
      before()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6

  restore()
  exports = ht.hash_spill(tables, bound, 0, comps)
  stores = [ht.HashSpillStore(dim, (dim, dim)) for _ in range(cols)]

  def put_all():
    for s, e in zip(stores, exports):
      s.put(e)

  def clear_all():
    for s in stores:
      s.clear()
  puts = [wall(put_all, clear_all) for _ in range(args.repeats + 1)][1:]
  nbytes_put = cols * n_gone * (8 + 3 * dim * 4 + 4 + 4)
  result['put'] = {'us': round(float(np.median(puts)), 2), 'min_max_us': [round(min(puts), 2), round(max(puts), 2)],
                   'bytes': nbytes_put, 'GBps': round(nbytes_put / float(np.median(puts)) * 1e-3, 2)}
  # fault_in of table 0: its state right after the spill, its store refilled before every call
  t0, store0, comps0 = tables[0], stores[0], plain[0]
  after = [x.clone() for x in (t0.keys, t0.last_seen, t0.freq, t0.counts, t0.stats, t0.table, comps0[0], comps0[1])]
  spilled = ht.HashExport(*[x.cpu() for x in (exports[0].keys, exports[0].rows, exports[0].last_seen, exports[0].freq)],
                          [x.cpu() for x in exports[0].slots])
  resident = t0.keys[t0._live()]   # pylint: disable=protected-access

  def refill():
    for x, y in zip((t0.keys, t0.last_seen, t0.freq, t0.counts, t0.stats, t0.table, comps0[0], comps0[1]), after):
      x.copy_(y)
    store0.clear()
    store0.put(spilled)
  for pct in (1, 10):
    n_back = batch * pct // 100
    n_resident = min(batch - n_back, resident.numel())   # (the table holds fewer keys than a batch has ids)
    unseen = np.arange(1, batch - n_back - n_resident + 1, dtype=np.int64) << 40
    ids = torch.cat([spilled.keys[torch.from_numpy(rng.permutation(n_gone)[:n_back])].to(dev),
                     resident[torch.from_numpy(rng.permutation(resident.numel())[:n_resident]).to(dev)],
                     torch.from_numpy(unseen).to(dev)])
    assert ids.numel() == batch
    ids = ids[torch.from_numpy(rng.permutation(batch)).to(dev)].contiguous()
    got = []
    times = [wall(lambda: got.append(t0.fault_in(ids, store0, comps0)), refill) for _ in range(args.repeats + 1)][1:]
    assert got == [n_back] * (args.repeats + 1)
    result[f'fault_in_{pct}pct'] = {'batch': batch, 'restored': n_back, 'us': round(float(np.median(times)), 2),
                                    'min_max_us': [round(min(times), 2), round(max(times), 2)]}
  line = json.dumps(result)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
