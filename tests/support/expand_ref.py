"""Plain numpy restatement of the key-deduplicated feature ops (include/hbk.h, "Key-deduplicated features"),
written from the formulas there and from nothing of the kernels: what the GPU tests compare with bit for bit."""
import numpy as np


def valid(idx, n_keys):
  idx = np.asarray(idx).astype(np.int64)
  return (idx >= 0) & (idx < n_keys)


def expand_ref(src, idx, n_keys=None):
  """out[b] = src[idx[b]] where 0 <= idx[b] < n_keys, else a zero row; idx None: the identity."""
  src = np.asarray(src)
  if idx is None:
    return src.copy()
  n_keys = src.shape[0] if n_keys is None else n_keys
  idx = np.asarray(idx).astype(np.int64)
  out = np.zeros((idx.size,) + src.shape[1:], src.dtype)
  for b in range(idx.size):
    if 0 <= idx[b] < n_keys:
      out[b] = src[idx[b]]
  return out


def index_ref(idx, n_keys):
  """(order, splits, invalid): order[splits[u]:splits[u + 1]] = the samples with idx[b] == u, ascending b;
  behind splits[n_keys] the samples in no list, ascending b too."""
  idx = np.asarray(idx).astype(np.int64)
  lists = [[] for _ in range(n_keys + 1)]
  for b in range(idx.size):
    lists[int(idx[b]) if 0 <= idx[b] < n_keys else n_keys].append(b)
  order = np.asarray([b for l in lists for b in l], np.int32).reshape(-1)
  splits = np.zeros(n_keys + 1, np.int32)
  at = 0
  for u in range(n_keys + 1):
    splits[u] = at
    at += len(lists[u])
  return order, splits, len(lists[n_keys])


def grad_ref(grad, idx, n_keys):
  """out[u] = the fp32 sum of grad[b] over the samples with idx[b] == u: a literal loop in ascending b that
  starts from the first term (not from 0) and adds one term at a time in fp32; no sample: a zero row."""
  grad = np.asarray(grad, np.float32)
  idx = np.asarray(idx).astype(np.int64)
  out = np.zeros((n_keys,) + grad.shape[1:], np.float32)
  seen = np.zeros(n_keys, bool)
  for b in range(idx.size):
    u = int(idx[b])
    if not 0 <= u < n_keys:
      continue
    if seen[u]:
      out[u] = (out[u] + grad[b]).astype(np.float32)
    else:
      out[u] = grad[b]
      seen[u] = True
  return out
