"""Plain numpy restatement of hbk_sequence_pack_n (include/hbk.h, "The PACKED form"), written from the
header's formulas, one sample and one position at a time:

    len_b            = row_splits[b + 1] - row_splits[b]   (1 without row_splits; a negative value counts as 0)
    l_b              = min(len_b, T)
    sample_splits[b] = sum over b' < b of l_b'              sample_splits[B] = total
    lengths[b]       = l_b
    pos_splits[b * T + t] = sample_splits[b] + min(t, l_b)  pos_splits[B * T] = total
    packed[sample_splits[b] + t] = int64(ids[row_splits[b] + t])  for t < l_b
    total            = sample_splits[B]

Bounds rule (hbk_sequence_id_grid_n's): an id index outside [0, n_ids) is not read; the packed element, which has
no pad id to hold, holds 0."""
import numpy as np


def pack_ref(ids, row_splits, max_len):
  """Returns ``(packed int64 [total], pos_splits int32 [B*T+1], lengths int32 [B], sample_splits int32 [B+1],
  total int)`` of one column.  ``row_splits`` None: one id per sample."""
  ids = np.asarray(ids)
  n_ids = int(ids.shape[0])
  T = int(max_len)
  assert T >= 1
  if row_splits is None:
    B = n_ids
    begs = list(range(B))
    lens = [1] * B
  else:
    sp = [int(v) for v in np.asarray(row_splits).tolist()]
    B = len(sp) - 1
    begs = sp[:B]
    lens = [sp[b + 1] - sp[b] for b in range(B)]
  lengths = np.zeros(B, np.int32)
  sample_splits = np.zeros(B + 1, np.int32)
  pos_splits = np.zeros(B * T + 1, np.int32)
  packed = []
  total = 0
  for b in range(B):
    l = min(max(lens[b], 0), T)
    lengths[b] = l
    sample_splits[b] = total
    for t in range(T):
      pos_splits[b * T + t] = total + min(t, l)
    for t in range(l):
      j = begs[b] + t
      packed.append(int(ids[j]) if 0 <= j < n_ids else 0)
    total += l
  sample_splits[B] = total
  pos_splits[B * T] = total
  return np.asarray(packed, np.int64).reshape(-1), pos_splits, lengths, sample_splits, total

