"""What key-deduplicated features cost and save: the expand and reduce launches alone, and DeduplicatedFeatures
against DenseFeatures over the restored ids, in one process, the forms taking turns.

Config 2's shape: 26 columns x 1M rows x dim 16 (one block of 416 floats), one int64 id per segment, B = 65 536
samples; U = B / ratio segments for ratio 1, 4 and 16, the restore index sorted (a reader that groups a user's
samples) and shuffled.

  launch_*   hbk_expand_rows_n and hbk_expand_rows_grad_n alone over a prebuilt index, as replays of a captured
             graph (no Python per step), with the byte model of include/hbk.h: forward 4 * width * (B + U) + 8 * B
             (int64 index), backward 4 * width * (B + U) + 4 * B + 4 * U; and hbk_expand_index_build (not captured)
  layer_*    forward and backward + SGD of DeduplicatedFeatures(None, {idx: DenseFeatures}) -- lookup of U segments,
             expand; index build (in the forward), reduce, backward of U segments -- against DenseFeatures fed the
             restored ids (ids[idx], made outside the timed region): what the parent commit offers.  At ratio 1 the
             feature can only cost.
  layer_pooled_*  the same two layers with Poisson(8) ids per segment (combiner mean), the restore index shuffled: the
             restored form gathers and reduces B * 8 table rows, the deduplicated one U * 8
  one_key    the degenerate batch in which one key owns every sample: the transpose is ONE sequential chain per
             element (long lists are not split)

Timing follows tools/bench_sequence_pack.py: warm-up steps, then `--steps` steps between HIP events, `--rounds`
rounds with the forms taking turns; medians with min / max.  Prints one JSON line per part and appends it to `--out`
(default profiles/expand_rows.txt).

  python tools/bench_expand_rows.py [--steps 30 --warmup 5 --rounds 7]
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

N_COLS, ROWS, DIM, B = 26, 1000000, 16, 65536
WIDTH = N_COLS * DIM
RATIOS = (1, 4, 16)
LAM = 8
LR = 1e-6


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--steps', type=int, default=30)
  p.add_argument('--warmup', type=int, default=5)
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'expand_rows.txt'))
  args = p.parse_args()
  import hybridbackend_amd as hb   # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_expand_rows.py measures on a GPU: none found')
  fc, emb = hb.feature_column, hb.embedding
  dev = torch.device('cuda:0')

  def timed(step):
    for _ in range(args.warmup):
      step()
    torch.cuda.current_stream().synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
      step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps   # us per step

  def turns(forms):
    t = {k: [] for k in forms}
    for _ in range(args.rounds):
      for k, step in forms.items():
        t[k].append(timed(step))
    out = {k + '_us': round(float(np.median(v)), 2) for k, v in t.items()}
    out.update({k + '_min_max_us': [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})
    return out

  def report(result):
    result['steps'], result['warmup'], result['rounds'] = args.steps, args.warmup, args.rounds
    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
      f.write(line + '\n')

  def restore_index(ratio, shuffled, seed=0):
    rng = np.random.RandomState(seed)
    u = B // ratio
    idx = np.repeat(np.arange(u), ratio)
    if shuffled:
      rng.shuffle(idx)
    return torch.from_numpy(idx.astype(np.int64)).to(dev), u

  def graph_of(fn):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
      fn()
    return g.replay

  # ---- the launches alone -------------------------------------------------------------------------------------
  def launches(idx, u, name):
    index = emb.ExpandIndex(idx, u).build()
    src = torch.randn(u, WIDTH, device=dev)
    out = torch.empty(B, WIDTH, device=dev)
    grad = torch.randn(B, WIDTH, device=dev)
    red = torch.empty(u, WIDTH, device=dev)
    forms = {'fwd': graph_of(lambda: emb.expand_rows(index, [src], [out])),
             'grad': graph_of(lambda: emb.expand_rows_grad(index, [grad], [red])),
             'index_build': index.build}
    res = {'part': 'launch', 'case': name, 'B': B, 'U': u, 'width': WIDTH}
    res.update(turns(forms))
    fwd_bytes = 4 * WIDTH * (B + u) + 8 * B
    grad_bytes = 4 * WIDTH * (B + u) + 4 * B + 4 * u
    res['fwd_model_MB'], res['grad_model_MB'] = round(fwd_bytes / 1e6, 1), round(grad_bytes / 1e6, 1)
    res['fwd_TBps'] = round(fwd_bytes / res['fwd_us'] / 1e6, 3)
    res['grad_TBps'] = round(grad_bytes / res['grad_us'] / 1e6, 3)
    report(res)

  for ratio in RATIOS:
    for shuffled in (False, True):
      idx, u = restore_index(ratio, shuffled)
      launches(idx, u, f'ratio{ratio}_{"shuffled" if shuffled else "sorted"}')
  launches(torch.zeros(B, dtype=torch.int64, device=dev), 1, 'one_key')

  # ---- the layer against DenseFeatures over the restored ids ----------------------------------------------------
  columns = lambda: [fc.EmbeddingColumn(f'c{c}', ROWS, DIM, 'mean') for c in range(N_COLS)]   # noqa: E731
  dedup = fc.DeduplicatedFeatures(None, {'idx': fc.DenseFeatures(columns(), dev)})
  restored = fc.DenseFeatures(columns(), dev)
  grad = torch.randn(B, WIDTH, device=dev)
  for ratio in RATIOS:
    for shuffled in (False, True):
      idx, u = restore_index(ratio, shuffled, seed=ratio)
      rng = np.random.RandomState(100 + ratio)
      ids = [torch.from_numpy(rng.randint(0, 2 ** 40, size=u).astype(np.int64)).to(dev) for _ in range(N_COLS)]
      feats = {f'c{c}': ids[c] for c in range(N_COLS)}
      feats['idx'] = idx
      rest = {f'c{c}': ids[c][idx].contiguous() for c in range(N_COLS)}   # (outside the timed region)

      def dedup_step():
        dedup(feats)
        dedup.backward(grad, apply_lr=LR, emit=False)

      def restored_step():
        restored(rest)
        restored.backward(grad, apply_lr=LR, emit=False)
      forms = {'dedup_fwd': lambda: dedup(feats), 'restored_fwd': lambda: restored(rest),
               'dedup_fwd_bwd_sgd': dedup_step, 'restored_fwd_bwd_sgd': restored_step}
      res = {'part': 'layer', 'case': f'ratio{ratio}_{"shuffled" if shuffled else "sorted"}', 'B': B, 'U': u,
             'columns': N_COLS, 'dim': DIM}
      res.update(turns(forms))
      res['fwd_speedup'] = round(res['restored_fwd_us'] / res['dedup_fwd_us'], 3)
      res['step_speedup'] = round(res['restored_fwd_bwd_sgd_us'] / res['dedup_fwd_bwd_sgd_us'], 3)
      report(res)

  # ---- the same with pooled columns: Poisson(LAM) ids per segment, combiner mean --------------------------------
  for ratio in RATIOS:
    idx, u = restore_index(ratio, True, seed=ratio)
    rng = np.random.RandomState(200 + ratio)
    feats, rest = {'idx': idx}, {}
    for c in range(N_COLS):
      lens = rng.poisson(LAM, size=u)
      splits = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(dev)
      ids = torch.from_numpy(rng.randint(0, 2 ** 40, size=int(lens.sum())).astype(np.int64)).to(dev)
      feats[f'c{c}'] = (ids, splits)
      # every sample's copy of its key's segment (outside the timed region)
      d_lens = torch.from_numpy(lens).to(dev)[idx]
      ends = torch.cumsum(d_lens, 0)
      at = (torch.repeat_interleave(splits[:-1].long()[idx] - (ends - d_lens), d_lens)
            + torch.arange(int(ends[-1]), device=dev))
      rest[f'c{c}'] = (ids[at].contiguous(), torch.cat([ends.new_zeros(1), ends]).int())

    def dedup_step():
      dedup(feats)
      dedup.backward(grad, apply_lr=LR, emit=False)

    def restored_step():
      restored(rest)
      restored.backward(grad, apply_lr=LR, emit=False)
    forms = {'dedup_fwd': lambda: dedup(feats), 'restored_fwd': lambda: restored(rest),
             'dedup_fwd_bwd_sgd': dedup_step, 'restored_fwd_bwd_sgd': restored_step}
    res = {'part': 'layer_pooled', 'case': f'ratio{ratio}_shuffled', 'B': B, 'U': u, 'columns': N_COLS, 'dim': DIM,
           'ids_per_segment': f'Poisson({LAM})'}
    res.update(turns(forms))
    res['fwd_speedup'] = round(res['restored_fwd_us'] / res['dedup_fwd_us'], 3)
    res['step_speedup'] = round(res['restored_fwd_bwd_sgd_us'] / res['dedup_fwd_bwd_sgd_us'], 3)
    report(res)


if __name__ == '__main__':
  main()
