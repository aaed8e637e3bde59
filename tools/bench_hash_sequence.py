"""The hash-keyed sequence lookup (hbk_hash_translate_sequence_n, HashSequenceLookup) next to the bucketed
SequenceLookup, in one process, the forms taking turns, on the shape of profiles/sequence_lookup.txt: 4 columns,
B = 8192 samples, T = 50, dim 16, int64 ids, Poisson(40) lengths (about one sample in twenty is truncated); every
table holds the column's vocabulary of 262 144 ids at load factor 0.5 (524 288 rows), slab_size 8.

  translate_hit     the translate alone, every id resident (no CAS is issued), no pad id
  translate_pad     the same with a pad id (every position is walked)
  translate_first   the first batch: the tables emptied before every timed launch
  hash_fwd          translate + gather over the slot grid (HashSequenceLookup.launch), no pad id
  hash_fwd_pad      the same with a pad id
  hash_bwd_sgd      SequenceLookupGrad over the slot grid with the fused SGD step (step only)
  bucketed_fwd      SequenceLookup (fused, buckets = the table's rows) on the same ids: the forward this is set beside
  bucketed_bwd_sgd  its backward with the fused SGD step

Timing follows tools/bench_sequence.py: warm-up steps, then `--steps` steps between HIP events, `--rounds` rounds
with the forms taking turns; medians with min / max.  `translate_first` empties the tables before each launch, so
each of its steps is timed alone between its own pair of events.  Prints one JSON line and appends it to `--out`
(default profiles/hash_sequence.txt).

  python tools/bench_hash_sequence.py [--steps 50 --warmup 10 --rounds 7]
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
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_sequence.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding.cache import EMPTY_KEY   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_sequence.py measures on a GPU: none found')
  dev = torch.device('cuda:0')
  cols, B, T, dim, vocab, slab_size = 4, 8192, 50, 16, 262144, 8
  capacity = 2 * vocab
  rng = np.random.RandomState(4242)
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)
  words = [torch.from_numpy(np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=vocab + 64,
                                                  dtype=np.int64))[:vocab].copy()).to(dev) for _ in range(cols)]
  words = [w[torch.randperm(vocab, device=dev)] for w in words]
  pad_ids = [int(w[0].item()) for w in words]
  splits, ids, valid = [], [], 0
  for c in range(cols):
    lens = rng.poisson(40, size=B)
    valid += int(np.minimum(lens, T).sum())
    sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    splits.append(torch.from_numpy(sp).to(dev))
    ids.append(words[c][torch.randint(0, vocab, (int(sp[-1]),), device=dev, generator=gen)])
  grads = [torch.randn(B, T, dim, device=dev, generator=gen) for _ in range(cols)]

  def make_tables():
    return [hb.embedding.HashTable(capacity, dim, dev, slab_size=slab_size, seed=c) for c in range(cols)]
  tables, first_tables = make_tables(), make_tables()
  for t, w in zip(tables, words):
    t.lookup_or_insert(w)
    assert t.size() == vocab and t.failed() == 0            # load factor 0.5
  hit = hb.embedding.HashSequenceLookup(tables, T)
  hit(ids, splits)
  pad = hb.embedding.HashSequenceLookup(tables, T, pad_ids=pad_ids)
  pad(ids, splits)
  assert all(t.size() == vocab and t.failed() == 0 for t in tables)
  first = hb.embedding.HashSequenceLookup(first_tables, T)
  first(ids, splits)
  hash_bwd = hb.embedding.SequenceLookupGrad(hit)
  hash_bwd(grads, apply_lr=1e-6, emit=False)
  bucketed = hb.embedding.SequenceLookup([t.table for t in tables], [capacity] * cols, max_lens=T, fused=True)
  bucketed(ids, splits)
  bucketed_bwd = hb.embedding.SequenceLookupGrad(bucketed)
  bucketed_bwd(grads, apply_lr=1e-6, emit=False)
  stream = _lib.current_stream(dev)
  lib = _lib.lib()

  def empty():
    for t in first_tables:
      t.keys.fill_(EMPTY_KEY)
      t.counts.zero_()

  def timed(step):
    for i in range(args.warmup):
      step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(args.steps):
      step(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps   # us per step

  def timed_alone(prepare, step, n):
    out = []
    for _ in range(n):
      prepare()
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      step(0)
      e1.record()
      e1.synchronize()
      out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out))

  steps = {
    'translate_hit': lambda i: hit._plan.launch(1, stream),
    'translate_pad': lambda i: pad._plan.launch(1, stream),
    'hash_fwd': lambda i: hit.launch(),
    'hash_fwd_pad': lambda i: pad.launch(),
    'hash_bwd_sgd': lambda i: hash_bwd.driver(False).launch(apply_lr=1e-6),
    'bucketed_fwd': lambda i: _lib.check(lib.hbk_group_lookup_fwd_sequence(cols, bucketed._cols, bucketed._seqs,
                                                                           None, stream)),
    'bucketed_bwd_sgd': lambda i: bucketed_bwd.driver(False).launch(apply_lr=1e-6),
  }
  t = {k: [] for k in steps}
  t['translate_first'] = []
  for _ in range(args.rounds):
    for k in steps:   # alternating
      t[k].append(timed(steps[k]))
    t['translate_first'].append(timed_alone(empty, lambda i: first._plan.launch(1, stream), 5))
  med = {k: float(np.median(v)) for k, v in t.items()}
  result = {'shape': {'cols': cols, 'B': B, 'T': T, 'dim': dim, 'positions': cols * B * T, 'valid_positions': valid,
                      'ids': int(sum(i.numel() for i in ids)), 'vocab': vocab, 'capacity': capacity, 'load': 0.5,
                      'slab_size': slab_size}}
  result.update({k + '_us': round(v, 2) for k, v in med.items()})
  result.update({k + '_min_max_us': [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})
  result['hash_fwd_over_bucketed_fwd'] = round(med['hash_fwd'] / med['bucketed_fwd'], 4)
  result['hash_bwd_over_bucketed_bwd'] = round(med['hash_bwd_sgd'] / med['bucketed_bwd_sgd'], 4)
  result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
  line = json.dumps(result)
  print(line)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
