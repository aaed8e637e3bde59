"""Key-deduplicated features: rows looked up once per distinct key, expanded to the batch on the device
(``hbk_expand_rows_n``), and the batch gradient reduced back to one row per key (``hbk_expand_rows_grad_n`` over
the inverse index ``hbk_expand_index_build`` makes) -- csrc/expand_rows.hip, include/hbk.h "Key-deduplicated
features".  The reference's ``hb.data.deduplicate`` (data/dataframe.py:301-392) restores the ids to batch length
before the lookup instead; here the lookup, its backward and its optimizer step see ``U`` segments and only the
pooled rows are restored.

There is no CPU fallback: host tensors are refused as everywhere in the package.
"""
import torch

from hybridbackend_amd import _lib


def _bad(msg):
  return _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, msg)


def _check_idx(idx, what):
  if not isinstance(idx, torch.Tensor) or idx.dim() != 1 or idx.dtype not in (torch.int32, torch.int64):
    raise _bad(f'{what}: idx must be an int32 or int64 vector, one row number per sample')
  _lib.require_device_tensor(idx, f'{what}: idx')


class ExpandIndex:
  """The inverse of a restore index ``idx`` (int32/int64 ``[B]``, row numbers into ``n_keys`` rows), built once
  per key field and step and shared by all of the key's columns: ``order`` (int32 ``[B]``) and ``splits`` (int32
  ``[n_keys + 1]``) list, per key, the samples that name it in ascending sample order; ``invalid`` (int32 ``[1]``)
  counts the samples whose index is outside ``[0, n_keys)`` -- they are in no list, read zero rows in the forward
  and send no gradient.  ``build()`` enqueues the build on the current stream (no host read, no allocation: the
  buffers and the workspace are made here); ``invalid_count()`` is the one place that reads the host."""

  def __init__(self, idx, n_keys):
    _check_idx(idx, 'ExpandIndex')
    n_keys = int(n_keys)
    if not 0 <= n_keys < 2 ** 31:
      raise _bad(f'ExpandIndex: n_keys must be in [0, 2^31), got {n_keys}')
    self.idx, self.n_keys, self.n_samples = idx, n_keys, int(idx.numel())
    dev = idx.device
    self.order = torch.empty(self.n_samples, dtype=torch.int32, device=dev)
    self.splits = torch.empty(n_keys + 1, dtype=torch.int32, device=dev)
    self.invalid = torch.empty(1, dtype=torch.int32, device=dev)
    self._need = int(_lib.lib().hbk_expand_index_workspace_bytes(self.n_samples, n_keys))
    self._work = torch.empty(max(self._need, 4), dtype=torch.uint8, device=dev)
    self.built = False

  def build(self):
    _lib.check(_lib.lib().hbk_expand_index_build(
      self.idx.data_ptr(), _lib.torch_dtype_code(self.idx.dtype), self.n_samples, self.n_keys,
      self.order.data_ptr(), self.splits.data_ptr(), self.invalid.data_ptr(), self._work.data_ptr(), self._need,
      _lib.current_stream(self.idx.device)))
    self.built = True
    return self

  def invalid_count(self):
    """The number of samples in no list (waits for the device)."""
    if not self.built:
      raise _bad('ExpandIndex.invalid_count: build() first')
    return int(self.invalid.item())


def _rows_of(t, rows, dtypes, what):
  """``t`` as ``rows`` rows of 4-byte elements: (row stride in elements, width)."""
  if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.dtype not in dtypes:
    raise _bad(f'{what} must be a {" or ".join(str(d).replace("torch.", "") for d in dtypes)} tensor of at '
               'least one dimension')
  _lib.require_device_tensor(t, what, row_strided=True)
  if t.shape[0] != rows:
    raise _bad(f'{what}: {t.shape[0]} rows, expected {rows}')
  width = 1
  for d in t.shape[1:]:
    width *= int(d)
  if width < 1:
    raise _bad(f'{what}: rows of {width} elements')
  stride = int(t.stride(0)) if t.dim() == 2 and not t.is_contiguous() else width
  return stride, width


def _columns(srcs, outs, rows_in, rows_out, dtypes, what):
  n = len(srcs)
  if outs is not None and len(outs) != n:
    raise _bad(f'{what}: expected {n} outputs, got {len(outs)}')
  cols = (_lib.ExpandColumn * n)()
  res = []
  for c, src in enumerate(srcs):
    stride, width = _rows_of(src, rows_in, dtypes, f'{what}: input {c}')
    shape = (rows_out,) + tuple(src.shape[1:])
    if outs is None:
      out = torch.empty(shape, dtype=src.dtype, device=src.device)
    else:
      out = outs[c]
      if not isinstance(out, torch.Tensor) or out.dtype != src.dtype or tuple(out.shape) != shape:
        raise _bad(f'{what}: output {c} must be a {str(src.dtype).replace("torch.", "")} tensor {list(shape)}')
    out_stride, _ = _rows_of(out, rows_out, (src.dtype,), f'{what}: output {c}')
    cols[c].src, cols[c].out = src.data_ptr(), out.data_ptr()
    cols[c].src_stride, cols[c].out_stride, cols[c].width = stride, out_stride, width
    res.append(out)
  return cols, res


def expand_rows(idx, srcs, outs=None, n_keys=None):
  """``outs[c][b] = srcs[c][idx[b]]``, a zero row where ``idx[b]`` is outside ``[0, n_keys)``: the forward over a
  list of ``[U, ...]`` tensors, each viewed as ``[U, width]`` (fp32, or int32 such as sequence lengths: the rows
  are copied bit for bit; contiguous, or 2-D column blocks of a wider tensor).  ``idx``: an int32/int64 ``[B]``
  device vector or an :class:`ExpandIndex` (its ``idx``; nothing built is read, so inference builds nothing);
  None: the identity ``outs[c][b] = srcs[c][b]``, which places a plain block with the same kind of launch.
  ``n_keys`` defaults to the index's, else to the rows of the inputs.  ``outs``: tensors of ``[B, ...]`` written
  in place (column blocks allowed), all distinct; default: new contiguous ones.  One launch per 64 columns, no
  host read: capturable.  Returns the outputs."""
  what = 'expand_rows'
  srcs = list(srcs)
  if isinstance(idx, ExpandIndex):
    n_keys = idx.n_keys if n_keys is None else n_keys
    idx = idx.idx
  if idx is not None:
    _check_idx(idx, what)
  if not srcs:
    if outs:
      raise _bad(f'{what}: expected 0 outputs, got {len(outs)}')
    return []
  if n_keys is None or idx is None:
    n_keys = int(srcs[0].shape[0]) if isinstance(srcs[0], torch.Tensor) and srcs[0].dim() >= 1 else 0
  n_keys = int(n_keys)
  n_samples = int(idx.numel()) if idx is not None else n_keys
  cols, res = _columns(srcs, outs, n_keys, n_samples, (torch.float32, torch.int32), what)
  dev = srcs[0].device
  _lib.check(_lib.lib().hbk_expand_rows_n(
    len(srcs), cols, None if idx is None else idx.data_ptr(),
    _lib.INT64 if idx is None else _lib.torch_dtype_code(idx.dtype), n_samples, n_keys, _lib.current_stream(dev)))
  return res


def expand_rows_grad(index, grads, outs=None):
  """The transpose of :func:`expand_rows` over a built :class:`ExpandIndex`: ``outs[c][u]`` is the fp32 sum of
  ``grads[c][b]`` over the samples ``b`` with ``idx[b] == u``, added one by one in ascending ``b`` starting from
  the first (one sequential chain per element: the same bits on every run, and those of a plain loop); a key
  nobody names gets a zero row, and every row of ``outs[c]`` is written.  ``grads[c]``: fp32 ``[B, ...]``,
  contiguous or a 2-D column block of the batch gradient; ``outs[c]``: ``[n_keys, ...]``.  No atomics, no host
  read: capturable over a prebuilt index.  Returns the outputs."""
  what = 'expand_rows_grad'
  if not isinstance(index, ExpandIndex):
    raise _bad(f'{what}: the first argument must be an ExpandIndex (the transpose needs the built inverse)')
  if not index.built:
    raise _bad(f'{what}: the ExpandIndex is not built: build() first')
  grads = list(grads)
  if not grads:
    if outs:
      raise _bad(f'{what}: expected 0 outputs, got {len(outs)}')
    return []
  cols, res = _columns(grads, outs, index.n_samples, index.n_keys, (torch.float32,), what)
  _lib.check(_lib.lib().hbk_expand_rows_grad_n(
    len(grads), cols, index.order.data_ptr(), index.splits.data_ptr(), index.n_samples, index.n_keys,
    _lib.current_stream(grads[0].device)))
  return res
