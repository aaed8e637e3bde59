"""Expiring hash tables (hbk_hash_insert_expiring_n, hbk_hash_evict_n) in one process, forms alternating, on
the shape of tools/bench_hash_insert.py: 26 columns x 65 536 one-id int64 keys, dim 16, every table at load
factor 0.5 (65 536 resident keys in 131 072 rows), slab_size 8.

  translate     plain (hbk_hash_insert_n) against expiring tables holding the same keys:
    hit / x_hit              every key of the batch is resident
    miss / x_miss            the first batch: every key is new (tables emptied before every timed launch)
    zipf / x_zipf            a Zipf(1.2) batch over the resident keys (duplicates inside the batch)
  sweep         hbk_hash_evict_n over the 26 expiring tables with two dim-16 companions each, 0 % / 10 % / 50 %
                of the resident keys evicted (the tables are restored before every timed launch): us, and
                GB/s over 16 B per slot + the bytes of the filled rows
  tombstones    x_hit with 0 % / 25 % / 50 % of the SLOTS tombstoned (that many other keys were inserted before
                the resident ones and evicted after them), and again after compact()

Timing follows tools/bench_hash_insert.py: warm-up steps, then `--steps` steps between HIP events, `--rounds`
rounds with the forms taking turns; medians with min / max; launches that need a prepared table are timed
alone between their own events.  Prints one JSON line and appends it to `--out` (default
profiles/hash_expiry.txt).

  python tools/bench_hash_expiry.py [--steps 50 --warmup 10 --rounds 5]
"""
import argparse
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
  p.add_argument('--steps', type=int, default=50)
  p.add_argument('--warmup', type=int, default=10)
  p.add_argument('--rounds', type=int, default=5)
  p.add_argument('--slab-size', type=int, default=8)
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_expiry.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding.cache import EMPTY_KEY   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_expiry.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  cols, batch, dim, slab_size = 26, 65536, 16, args.slab_size
  capacity = 2 * batch
  rng = np.random.RandomState(777)

  def distinct(n):
    return torch.from_numpy(np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=n + 64, dtype=np.int64))[:n]
                            .copy()).to(dev)
  pool = [distinct(2 * batch) for _ in range(cols)]
  pool = [r[torch.randperm(2 * batch, device=dev)] for r in pool]
  resident = [r[:batch].contiguous() for r in pool]
  others = [r[batch:].contiguous() for r in pool]
  zipf = [r[torch.from_numpy((rng.zipf(1.2, size=batch) - 1) % batch).to(dev)] for r in resident]
  stream = _lib.current_stream(dev)

  def timed(step):
    for _ in range(args.warmup):
      step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
      step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps   # us per step

  def timed_alone(prepare, step, n=5):
    out = []
    for _ in range(n):
      prepare()
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      step()
      e1.record()
      e1.synchronize()
      out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out))

  def make(expiring):
    return [hb.embedding.HashTable(capacity, dim, dev, slab_size=slab_size, expiring=expiring) for _ in range(cols)]

  def empty(tables):
    for t in tables:
      t.keys.fill_(EMPTY_KEY)
      t.counts.zero_()
      if t.expiring:
        t.last_seen.zero_()
        t.freq.zero_()
        t.stats.zero_()

  def launcher(hgl, insert=True):
    return lambda: hgl._plan.launch(insert, stream)

  t = {}
  # ---- translate: plain against expiring ------------------------------------------------------------------
  plain, exp = make(False), make(True)
  forms = {}
  for name, tables in (('', plain), ('x_', exp)):
    hit = hb.embedding.HashGroupLookup(tables)
    hit(resident)
    assert all(x.size() == batch and x.failed() == 0 for x in tables)
    zf = hb.embedding.HashGroupLookup(tables)
    zf(zipf)
    forms[name + 'hit'], forms[name + 'zipf'] = launcher(hit), launcher(zf)
  for k in forms:
    t[k] = []
  for _ in range(args.rounds):
    for k in forms:   # alternating
      t[k].append(timed(forms[k]))
  t['miss'] = [timed_alone(lambda: empty(plain), forms['hit']) for _ in range(args.rounds)]
  t['x_miss'] = [timed_alone(lambda: empty(exp), forms['x_hit']) for _ in range(args.rounds)]
  assert all(x.size() == batch for x in plain + exp)
  del plain

  # ---- sweep ------------------------------------------------------------------------------------------------
  comps = [[(torch.full((capacity, dim), 0.1, device=dev), 0.1), (torch.zeros((capacity, dim), device=dev), 0.0)]
           for _ in range(cols)]
  for x in exp:
    x.set_step(100)
  saved = [(x.keys.clone(), x.freq.clone()) for x in exp]
  where = [x.find(r) for x, r in zip(exp, resident)]
  # (the descriptors once: the timed region is the entry alone)
  from hybridbackend_amd.embedding.hashtable import _evict_columns   # pylint: disable=import-outside-toplevel
  lib = _lib.lib()
  evict_cols, _keep = _evict_columns(exp, 50, 0, comps)
  sweep = {}
  for pct in (0, 10, 50):
    # the first pct % of the resident keys were last seen at step 0, the others at step 100
    seen = []
    for w in where:
      s = torch.full((capacity,), 100, dtype=torch.int32, device=dev)
      s[w[:batch * pct // 100]] = 0
      seen.append(s)

    def restore():
      for x, (k, f), s in zip(exp, saved, seen):
        x.keys.copy_(k)
        x.freq.copy_(f)
        x.last_seen.copy_(s)
        x.stats.zero_()
    us = [timed_alone(restore, lambda: _lib.check(lib.hbk_hash_evict_n(cols, evict_cols, stream)))
          for _ in range(args.rounds)]
    n_evicted = sum(x.evicted() for x in exp)
    assert n_evicted == cols * (batch * pct // 100), (pct, n_evicted)
    nbytes = cols * capacity * 16 + n_evicted * (16 + 2 * dim * 4)
    med = float(np.median(us))
    sweep[f'{pct}pct'] = {'us': round(med, 2), 'min_max_us': [round(min(us), 2), round(max(us), 2)],
                          'evicted': n_evicted, 'bytes': nbytes, 'GBps': round(nbytes / med * 1e-3, 1)}
  del comps, saved

  # ---- tombstone load -----------------------------------------------------------------------------------------
  tomb = {}
  for pct in (0, 25, 50):
    empty(exp)
    n_dead = capacity * pct // 100
    # that many OTHER keys go in first (step 0), the resident keys behind them (step 100); the sweep then
    # takes the others: the resident keys stay where they were placed, tombstones before and between them
    for x, o in zip(exp, others):
      x.set_step(0)
      if n_dead:
        x.lookup_or_insert(o[:n_dead])
      x.set_step(100)
    hit = hb.embedding.HashGroupLookup(exp)
    hit(resident)
    for x in exp:
      x.evict(50)
      assert x.tombstones() == n_dead and x.size() == batch and x.failed() == 0
    left = sum(x.tombstones() for x in exp) / (cols * capacity)
    before = [timed(launcher(hit)) for _ in range(args.rounds)]
    for x in exp:
      x.compact()
    hit(resident)
    assert all(x.size() == batch and x.tombstones() == 0 for x in exp)
    after = [timed(launcher(hit)) for _ in range(args.rounds)]
    tomb[f'{pct}pct'] = {'tombstoned': round(left, 4),
                         'x_hit_us': round(float(np.median(before)), 2),
                         'x_hit_min_max_us': [round(min(before), 2), round(max(before), 2)],
                         'compacted_x_hit_us': round(float(np.median(after)), 2),
                         'compacted_min_max_us': [round(min(after), 2), round(max(after), 2)]}

  med = {k: float(np.median(v)) for k, v in t.items()}
  result = {'slab_size': slab_size,
            'shape': {'cols': cols, 'keys_per_col': batch, 'dim': dim, 'capacity': capacity, 'load': 0.5}}
  result.update({k + '_us': round(v, 2) for k, v in med.items()})
  result.update({k + '_min_max_us': [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})
  for k in ('hit', 'miss', 'zipf'):
    result[f'x_{k}_over_{k}'] = round(med['x_' + k] / med[k], 4)
  result['sweep'] = sweep
  result['tombstones'] = tomb
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  line = json.dumps(result)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
