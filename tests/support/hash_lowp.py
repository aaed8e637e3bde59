"""What the GPU tests of the 16-bit runs and sequence entries share (hbk_hash_translate_runs_lowp_n,
hbk_hash_translate_sequence_lowp_n): the records of a list of tables of one kind, the two calls -- a 16-bit table goes
through the 16-bit entry, an fp32 twin through the fp32 entry -- and the oracle of a new row, torch's own cast of the
fp32 start row."""
import ctypes as C

import numpy as np
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding.hashtable import LOWP_DTYPES
from tests.support import hash_ref as ref

DEV = 'cuda:0'


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def bits16(t):
  return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def cast_rows(keys, dim, seed, scale, dtype):
  """The uint16 patterns of torch.from_numpy(fp32 start row).to(dtype)."""
  rows = ref.init_rows(np.asarray(keys, np.int64), dim, seed, scale)
  return torch.from_numpy(rows).to(dtype).view(torch.int16).numpy().view(np.uint16)


def describe(tables, insert):
  """The column, expiry and admission records of tables of ONE kind."""
  n = len(tables)
  kinds = {(t.expiring, bool(t.min_freq)) for t in tables}
  assert len(kinds) == 1
  expiring, filtered = kinds.pop()
  cols = (_lib.HashColumn * n)()
  exp = (_lib.HashExpiry * n)() if expiring else None
  adm = (_lib.HashAdmission * n)() if filtered else None
  for c, t in enumerate(tables):
    t._describe(cols[c], init=bool(insert), count=bool(insert))
    if expiring:
      t._describe_expiry(exp[c])
    if filtered:
      t._describe_admission(adm[c])
  return cols, exp, adm


def codes_of(tables):
  return (C.c_int32 * len(tables))(*[LOWP_DTYPES[t.dtype] for t in tables])


def translate_runs(tables, runs, insert=True):
  """runs[c]: list of id tensors.  16-bit tables go through hbk_hash_translate_runs_lowp_n, fp32 ones through
  hbk_hash_translate_runs_n; returns the slot tensors in the same shape."""
  n = len(tables)
  cols, exp, adm = describe(tables, insert)
  keep, ptrs, slots = [], [], []
  for c in range(n):
    cols[c].keys, cols[c].slots, cols[c].n_keys = None, None, -3          # ignored
    r = (_lib.HashRun * max(len(runs[c]), 1))()
    out = [torch.full((i.numel(),), -7, dtype=torch.int64, device=DEV) for i in runs[c]]
    for k, (i, o) in enumerate(zip(runs[c], out)):
      r[k].keys, r[k].slots, r[k].n_keys = (i.data_ptr(), o.data_ptr(), i.numel()) if i.numel() else (None, None, 0)
    keep.append(r)
    ptrs.append(C.cast(r, C.c_void_p).value)
    slots.append(out)
  n_runs, run_ptrs = _lib.i32_array([len(r) for r in runs]), _lib.ptr_array(ptrs)
  stream = _lib.current_stream(torch.device(DEV))
  lib = _lib.lib()
  if tables[0].dtype == torch.float32:
    _lib.check(lib.hbk_hash_translate_runs_n(n, cols, exp, adm, n_runs, run_ptrs, 1 if insert else 0, stream))
  else:
    _lib.check(lib.hbk_hash_translate_runs_lowp_n(n, cols, exp, adm, codes_of(tables), n_runs, run_ptrs,
                                                  1 if insert else 0, stream))
  torch.cuda.synchronize()
  return slots


def translate_sequence(tables, ids, splits, max_len, pad_id, insert=True):
  """ids[c] / splits[c]: the flat ids and int32 row_splits of column c.  Returns (grids, lengths)."""
  n = len(tables)
  cols, exp, adm = describe(tables, insert)
  seqs = (_lib.HashSequence * n)()
  grids, lengths = [], []
  for c in range(n):
    b = splits[c].numel() - 1
    g = torch.full((b * max_len,), -7, dtype=torch.int64, device=DEV)
    ln = torch.full((b,), -7, dtype=torch.int32, device=DEV)
    cols[c].keys, cols[c].n_keys, cols[c].slots = ids[c].data_ptr(), ids[c].numel(), g.data_ptr()
    q = seqs[c]
    q.row_splits, q.n_segments, q.max_len = splits[c].data_ptr(), b, max_len
    q.has_pad, q.pad_id, q.lengths = (0, 0, ln.data_ptr()) if pad_id is None else (1, pad_id, ln.data_ptr())
    grids.append(g)
    lengths.append(ln)
  stream = _lib.current_stream(torch.device(DEV))
  lib = _lib.lib()
  if tables[0].dtype == torch.float32:
    _lib.check(lib.hbk_hash_translate_sequence_n(n, cols, exp, adm, seqs, 1 if insert else 0, stream))
  else:
    _lib.check(lib.hbk_hash_translate_sequence_lowp_n(n, cols, exp, adm, codes_of(tables), seqs, 1 if insert else 0,
                                                      stream))
  torch.cuda.synchronize()
  return grids, lengths
