"""What hash-keyed feature columns cost through the layer, in one process, the forms taking turns.

The shape of config 2 with every column hash-keyed: 26 columns x 131 072 slots, dim 16, batch 65 536, one id per
sample, every id resident (a vocabulary of 65 536 ids per column: load factor 0.5, slab_size 8).

  layer_fwd        DenseFeatures.__call__ over 26 HashEmbeddingColumn (the translate + the lookup into the block)
  hand_fwd         HashGroupLookup called by hand on the same ids, writing the same kind of block
  launch_fwd       the two launches of the forward alone, as replays of a captured graph (no Python per step)
  layer_bwd_sgd    DenseFeatures.backward with the fused SGD step (step only)
  hand_bwd_sgd     GroupLookupGrad(hgl.lookup) called by hand on hgl.slots
  launch_bwd_sgd   the backward's launches alone, as replays of a captured graph
  bucketed_fwd / bucketed_bwd_sgd   the same layer with 26 bucketed EmbeddingColumn of 131 072 rows: today's step

A step enqueues without waiting, so a form whose Python takes longer than its kernels is timed by its Python: the
difference between a layer form and its launch form is what the layer's host side costs.

  id_grid          hbk_sequence_id_grid_n alone at the sequence shape (4 columns, B = 8192, T = 50, Poisson(40)
                   lengths), with its byte model: 8 B stored per position, 8 B read per position that holds an id,
                   4 B per row split -- and the GB/s that gives

Timing follows tools/bench_hash_sequence.py: warm-up steps, then `--steps` steps between HIP events, `--rounds`
rounds with the forms taking turns; medians with min / max.  Prints one JSON line and appends it to `--out` (default
profiles/hash_features.txt).

`--regression LABEL` measures only the two bucketed forms and touches nothing of the hash-keyed columns, so the same
file also runs from a checkout of the parent commit: (parent, this) x 3 taking turns shows whether the bucketed step
moved.

  python tools/bench_hash_features.py [--steps 50 --warmup 10 --rounds 7] [--regression LABEL]
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
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hash_features.txt'))
  p.add_argument('--regression', default=None, metavar='LABEL',
                 help='only bucketed_fwd / bucketed_bwd_sgd, with nothing of the hash-keyed columns touched: the '
                      'form that also runs from a checkout of the parent commit (copy this file there); LABEL names '
                      'the checkout in the result')
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd import _lib   # pylint: disable=import-outside-toplevel
  from hybridbackend_amd.embedding import sequence as seq_mod   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_hash_features.py measures on a GPU: none found')
  fc = hb.feature_column
  dev = torch.device('cuda:0')
  n_cols, slots, dim, batch, vocab = 26, 131072, 16, 65536, 65536
  rng = np.random.RandomState(4242)
  gen = torch.Generator(device=dev)
  gen.manual_seed(1234)
  words = [torch.from_numpy(np.unique(rng.randint(-2 ** 63 + 2, 2 ** 63 - 1, size=vocab + 64,
                                                  dtype=np.int64))[:vocab].copy()).to(dev) for _ in range(n_cols)]
  ids = [w[torch.randint(0, vocab, (batch,), device=dev, generator=gen)] for w in words]
  feats = {f'c{c}': ids[c] for c in range(n_cols)}
  grad = torch.randn(batch, n_cols * dim, device=dev, generator=gen)
  lr = 1e-6

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

  def report(result):
    result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
      f.write(line + '\n')

  # today's step: the same layer with bucketed columns
  bucketed = fc.DenseFeatures([fc.EmbeddingColumn(f'c{c}', slots, dim, 'sum', hot_rows=False)
                               for c in range(n_cols)], dev)
  bucketed(feats)
  bucketed.backward(grad, apply_lr=lr, emit=False)
  if args.regression is not None:
    forms = {'bucketed_fwd': lambda i: bucketed(feats),
             'bucketed_bwd_sgd': lambda i: bucketed.backward(grad, apply_lr=lr, emit=False)}
    t = {k: [] for k in forms}
    for _ in range(args.rounds):
      for k in forms:
        t[k].append(timed(forms[k]))
    result = {'regression': args.regression}
    result.update({k + '_us': round(float(np.median(v)), 2) for k, v in t.items()})
    result.update({k + '_min_max_us': [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})
    report(result)
    return

  # through the layer
  layer = fc.DenseFeatures([fc.HashEmbeddingColumn(f'c{c}', slots, dim, 'sum', seed=c) for c in range(n_cols)], dev)
  for t, w in zip(layer.hash_tables, words):
    t.lookup_or_insert(w)
    assert t.size() == vocab and t.failed() == 0            # load factor 0.5
  layer(feats)
  layer.backward(grad, apply_lr=lr, emit=False)
  # by hand, on tables of the same arguments
  tables = [hb.embedding.HashTable(slots, dim, dev, seed=c) for c in range(n_cols)]
  for t, w in zip(tables, words):
    t.lookup_or_insert(w)
  hgl = hb.embedding.HashGroupLookup(tables, combiners='sum')
  block = torch.empty(batch, n_cols * dim, device=dev)
  views = [block[:, c * dim:(c + 1) * dim] for c in range(n_cols)]
  offsets = [c * dim for c in range(n_cols)]
  hgl(ids, None, views)
  hand_grad = hb.embedding.GroupLookupGrad(hgl.lookup)
  hand_grad(hgl.slots, None, None, apply_lr=lr, emit=False, grad_block=(grad, offsets))
  torch.cuda.synchronize()

  def captured(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
      with torch.cuda.graph(graph, stream=s):
        fn()
    torch.cuda.synchronize()
    return graph
  g_fwd = captured(hgl.launch)
  g_bwd = captured(lambda: hand_grad.launch(apply_lr=lr))

  # the raw-id grid alone
  s_cols, B, T = 4, 8192, 50
  s_ids, s_splits, valid = [], [], 0
  for _ in range(s_cols):
    lens = rng.poisson(40, size=B)
    valid += int(np.minimum(lens, T).sum())
    sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    s_splits.append(torch.from_numpy(sp).to(dev))
    s_ids.append(torch.randint(-2 ** 62, 2 ** 62, (int(sp[-1]),), device=dev, generator=gen))
  g_cols, g_seqs = (_lib.LookupColumn * s_cols)(), (_lib.Sequence * s_cols)()
  counts, _ = seq_mod._bind_ids(g_cols, g_seqs, s_ids, s_splits, [T] * s_cols, [-1] * s_cols)   # pylint: disable=protected-access
  lengths, grids = seq_mod._alloc_side(counts, [T] * s_cols, dev, True)   # pylint: disable=protected-access
  for c in range(s_cols):
    g_seqs[c].pad_id = -1
    g_seqs[c].lengths, g_seqs[c].row_grid = lengths[c].data_ptr(), grids[c].data_ptr()
  stream = _lib.current_stream(dev)
  lib = _lib.lib()
  grid_bytes = s_cols * B * T * 8 + valid * 8 + s_cols * (B + 1) * 4 + s_cols * B * 4

  steps = {
    'layer_fwd': lambda i: layer(feats),
    'hand_fwd': lambda i: hgl(ids, None, views),
    'launch_fwd': lambda i: g_fwd.replay(),
    'layer_bwd_sgd': lambda i: layer.backward(grad, apply_lr=lr, emit=False),
    'hand_bwd_sgd': lambda i: hand_grad(hgl.slots, None, None, apply_lr=lr, emit=False, grad_block=(grad, offsets)),
    'launch_bwd_sgd': lambda i: g_bwd.replay(),
    'bucketed_fwd': lambda i: bucketed(feats),
    'bucketed_bwd_sgd': lambda i: bucketed.backward(grad, apply_lr=lr, emit=False),
    'id_grid': lambda i: _lib.check(lib.hbk_sequence_id_grid_n(s_cols, g_cols, g_seqs, stream)),
  }
  t = {k: [] for k in steps}
  for _ in range(args.rounds):
    for k in steps:   # taking turns
      t[k].append(timed(steps[k]))
  med = {k: float(np.median(v)) for k, v in t.items()}
  result = {'shape': {'cols': n_cols, 'slots': slots, 'dim': dim, 'batch': batch, 'vocab': vocab, 'load': 0.5,
                      'slab_size': 8},
            'id_grid_shape': {'cols': s_cols, 'B': B, 'T': T, 'positions': s_cols * B * T, 'valid_positions': valid,
                              'bytes': grid_bytes}}
  result.update({k + '_us': round(v, 2) for k, v in med.items()})
  result.update({k + '_min_max_us': [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})
  result['layer_fwd_over_hand_fwd'] = round(med['layer_fwd'] / med['hand_fwd'], 4)
  result['layer_bwd_over_hand_bwd'] = round(med['layer_bwd_sgd'] / med['hand_bwd_sgd'], 4)
  result['id_grid_gb_per_s'] = round(grid_bytes / med['id_grid'] * 1e-3, 1)
  report(result)


if __name__ == '__main__':
  main()
