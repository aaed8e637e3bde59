"""Growth and compaction of hash tables (hbk_hash_rehash_n) against the host path, in one process, on the shape
of tools/bench_hash_expiry.py: 26 expiring tables x 131 072 slots, dim 16, slab_size 8, 65 536 resident keys each
(load 0.5), two dim-16 companions per table.

  growth        every table to 262 144 slots:
    rehash_call              hash_rehash(tables, capacities, slots=companions): allocations, fills, ONE launch
    rehash_kernel            the entry alone, into destination arrays prepared before the timed region
    host                     per table load(*items()) into a fresh table, last_seen / freq / companions moved by
                             indexing with the old and new slots of the keys
  compaction    the same geometry, 25 % of the SLOTS tombstoned (that many other keys inserted before the resident
                ones and evicted after them): rehash_call / rehash_kernel against compact(slots=...) per table
  translate     the resident translate (every key of the batch resident) of tables that never held a tombstone,
                of the tombstoned tables, and of those after the device-side rehash
  --ab-lib      a second build of the library (make OUT=... OBJDIR=..., of another commit or with other flags): the
                entry alone, the two builds taking turns on the same descriptors

Every timed region is one operation between its own HIP events, the tables restored before it; `--rounds`
rounds with the forms taking turns; medians with min / max.  Bytes per launch: 8 B per source slot, per live key
64 B of destination slab read + 8 B of compare-and-swap + 2 x the row bytes of every move; GB/s against 8 TB/s.
Prints one JSON line and appends it to `--out` (default profiles/hash_rehash.txt).

  python tools/bench_hash_rehash.py [--rounds 7 --steps 50 --warmup 10]
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
  p.add_argument('--steps', type=int, default=50)
  p.add_argument('--warmup', type=int, default=10)
  p.add_argument('--cols', type=int, default=26)
  p.add_argument('--ab-lib', default=None)
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_rehash.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding.cache import EMPTY_KEY   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_rehash.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  cols, batch, dim, slab_size = args.cols, 65536, 16, 8
  capacity = 2 * batch
  rng = np.random.RandomState(778)
  stream = _lib.current_stream(dev)
  lib = _lib.lib()
  other = None
  if args.ab_lib:
    other = C.CDLL(args.ab_lib, mode=C.RTLD_LOCAL)
    other.hbk_hash_rehash_n.restype = C.c_int
    other.hbk_hash_rehash_n.argtypes = [C.c_int32, C.c_void_p, C.c_void_p]

  def distinct(n):
    return torch.from_numpy(np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n + 64, dtype=np.int64))[:n]
                            .copy()).to(dev)
  pool = [distinct(2 * batch) for _ in range(cols)]
  pool = [r[torch.randperm(2 * batch, device=dev)] for r in pool]
  resident = [r[:batch].contiguous() for r in pool]
  others = [r[batch:].contiguous() for r in pool]

  def once(prepare, step):
    prepare()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3

  def resident_translate(tables):
    hit = hb.embedding.HashGroupLookup(tables)
    hit(resident)
    step = lambda: hit._plan.launch(True, stream)   # noqa: E731
    out = []
    for _ in range(args.rounds):
      for _ in range(args.warmup):
        step()
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(args.steps):
        step()
      e1.record()
      e1.synchronize()
      out.append(e0.elapsed_time(e1) * 1e3 / args.steps)
    return out

  def build(n_dead):
    tables = [hb.embedding.HashTable(capacity, dim, dev, slab_size=slab_size, expiring=True) for _ in range(cols)]
    for x, o, r in zip(tables, others, resident):
      x.set_step(0)
      if n_dead:
        x.lookup_or_insert(o[:n_dead])
      x.set_step(100)
      x.lookup_or_insert(r)
      x.evict(50)
      assert x.tombstones() == n_dead and x.size() == batch and x.failed() == 0
    comps = []
    for x, r in zip(tables, resident):
      a, b = torch.full((capacity, dim), 0.1, device=dev), torch.zeros((capacity, dim), device=dev)
      where = x.find(r)
      a[where] = torch.rand((batch, dim), device=dev) + 1
      b[where] = torch.randn((batch, dim), device=dev)
      comps.append([(a, 0.1), (b, 0.0)])
    return tables, comps

  NAMES = ('keys', 'table', 'last_seen', 'freq', 'counts', 'stats')

  def snapshot(tables, comps):
    return [({n: getattr(x, n).clone() for n in NAMES}, [c.clone() for c, _ in cs]) for x, cs in zip(tables, comps)]

  def restore(tables, comps, saved):
    """Fresh copies of the saved arrays as the tables' state (the host path writes in place, the device path
    replaces the tensors: both start from the same thing)."""
    out = []
    for x, cs, (state, cc) in zip(tables, comps, saved):
      for n in NAMES:
        setattr(x, n, state[n].clone())
      x.slab_size, x.slab_count, x.capacity = slab_size, capacity // slab_size, capacity
      out.append([(c.clone(), v) for c, (_, v) in zip(cc, cs)])
    return out

  def describe(tables, comps, new_capacity):
    """Destination arrays and descriptors of the entry alone."""
    arr = (_lib.HashRehashColumn * cols)()
    keep, dst_keys = [], []
    for c, (x, cs) in enumerate(zip(tables, comps)):
      k = torch.full((new_capacity,), EMPTY_KEY, dtype=torch.int64, device=dev)
      moves = [(x.table, torch.zeros((new_capacity, dim), device=dev), dim),
               (x.last_seen, torch.zeros(new_capacity, dtype=torch.int32, device=dev), 1),
               (x.freq, torch.zeros(new_capacity, dtype=torch.int32, device=dev), 1)]
      moves += [(s, torch.full((new_capacity, dim), v, device=dev), dim) for s, v in cs]
      col = arr[c]
      col.src_keys, col.src_slab_count, col.src_slab_size = x.keys.data_ptr(), x.slab_count, x.slab_size
      col.dst_keys, col.dst_slab_count, col.dst_slab_size = k.data_ptr(), new_capacity // slab_size, slab_size
      col.expiring, col.n_moves = 1, len(moves)
      for m, (s, d, words) in enumerate(moves):
        col.moves[m].src, col.moves[m].dst, col.moves[m].words = s.data_ptr(), d.data_ptr(), words
      dst_keys.append(k)
      keep.append(moves)
    return arr, dst_keys, keep

  def host_growth(tables, comps, new_capacity):
    for x, cs in zip(tables, comps):
      new = hb.embedding.HashTable(new_capacity, dim, dev, slab_size=slab_size, expiring=True)
      keys, rows = x.items()
      to = new.load(keys, rows)
      at = x.find(keys)
      new.last_seen[to] = x.last_seen[at]
      new.freq[to] = x.freq[at]
      for s, v in cs:
        d = torch.full((new_capacity, dim), v, device=dev)
        d[to] = s[at]

  row_bytes = 4 * (dim + 1 + 1 + 2 * dim)
  nbytes = cols * (capacity * 8 + batch * (64 + 8 + 2 * row_bytes))
  result = {'shape': {'cols': cols, 'slots_per_col': capacity, 'keys_per_col': batch, 'dim': dim, 'slab_size': slab_size,
                      'companions': 2, 'moves_per_table': 5, 'row_bytes_per_key': row_bytes},
            'bytes_per_launch': nbytes, 'rounds': args.rounds}

  def summary(us, with_bytes=False):
    med = float(np.median(us))
    out = {'us': round(med, 2), 'min_max_us': [round(min(us), 2), round(max(us), 2)]}
    if with_bytes:
      out['GBps'] = round(nbytes / med * 1e-3, 1)
      out['of_8TBps'] = round(nbytes / med * 1e-3 / 8000, 4)
    return out

  def case(n_dead, new_capacity, host_step):
    tables, comps = build(n_dead)
    saved = snapshot(tables, comps)
    state = {}

    def prepare():
      state['comps'] = restore(tables, comps, saved)

    def prepare_kernel():
      prepare()
      state['arr'], state['dst'], state['keep'] = describe(tables, state['comps'], new_capacity)

    forms = {
      'rehash_call': (prepare, lambda: hb.embedding.hash_rehash(tables, [new_capacity] * cols, None, state['comps'])),
      'rehash_kernel': (prepare_kernel, lambda: _lib.check(lib.hbk_hash_rehash_n(cols, state['arr'], stream))),
      'host': (prepare, lambda: host_step(tables, state['comps'])),
    }
    if other is not None:
      forms['rehash_kernel_ab_lib'] = (prepare_kernel,
                                       lambda: _lib.check(other.hbk_hash_rehash_n(cols, state['arr'], stream)))
    t = {k: [] for k in forms}
    for k, (prep, step) in forms.items():   # one untimed pass of everything: allocator, first launches
      once(prep, step)
    for _ in range(args.rounds):
      for k, (prep, step) in forms.items():   # alternating
        t[k].append(once(prep, step))
    out = {k: summary(v, with_bytes=k.startswith('rehash_kernel')) for k, v in t.items()}
    out['host_over_rehash_call'] = round(out['host']['us'] / out['rehash_call']['us'], 2)
    # leave the tables rehashed on the device, checked
    prepare()
    hb.embedding.hash_rehash(tables, [new_capacity] * cols, None, state['comps'])
    assert all(x.size() == batch and x.tombstones() == 0 and x.capacity == new_capacity for x in tables)
    return out, tables, saved, comps

  result['growth'], _, _, _ = case(0, 2 * capacity, lambda tables, comps: host_growth(tables, comps, 2 * capacity))
  torch.cuda.empty_cache()

  clean, _ = build(0)
  translate = {'untombstoned': summary(resident_translate(clean))}
  del clean
  n_dead = capacity // 4
  compaction, tables, saved, comps = case(
    n_dead, capacity, lambda tables, cs: [x.compact(slots=c) for x, c in zip(tables, cs)])
  result['compaction_25pct_tombstones'] = compaction
  translate['after_rehash'] = summary(resident_translate(tables))
  restore(tables, comps, saved)
  assert all(x.tombstones() == n_dead for x in tables)
  translate['tombstoned_25pct'] = summary(resident_translate(tables))
  result['resident_translate'] = translate

  line = json.dumps(result)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
