"""ReplicatedGradients: the gradients of small REPLICATED tables across ranks, in their dense form -- the
reference's ``TRAINABLE_REPLICATED_SMALL`` (hybridbackend/tensorflow/training/gradient.py:131-141: sparse
gradients of small replicated variables are made dense and allreduced, then averaged, ``_mean``, ``:77-99``).

A replicated table has at most ``max(batch, W)`` rows, so every rank scatters its IndexedSlices into one
bucket (``hbk_replica_grads_pack_n``), ONE packed allreduce sums the buckets of all ranks, and each table's
block of the bucket is handed back as IndexedSlices WITH HOLES (``hbk_replica_grads_rows_n``): rows no rank
touched read ``-1``, which ``hb.embedding.SparseApply`` skips.  No compaction, no copy, no host read besides
the collective's own."""
import math

import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.distribute.collective import Collective


def _bad(msg):
  return _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, msg)


def replica_bucket_layout(shapes):
  """The bucket of tables ``shapes[c] = (rows, dim)``: ``(block offsets, touched offsets, floats)``, all in
  floats.  Every block ``[rows, dim]`` starts on a 16-byte boundary; the ``touched`` words, one per row of
  every table, follow the last block."""
  blocks, at = [], 0
  for rows, dim in shapes:
    blocks.append(at)
    at += (int(rows) * int(dim) + 3) // 4 * 4
  touched = []
  for rows, _ in shapes:
    touched.append(at)
    at += int(rows)
  return blocks, touched, at


class ReplicatedGradients:
  """Owns the bucket, the ``urows`` tensors and the row counts of a group of replicated tables.

  Args:
    shapes: per table ``(rows, dim)``.
    coll: the :class:`Collective` (None or one rank: nothing is reduced).
    scale: multiplies the summed bucket in the allreduce's own pass.  None: ``1 / world_size``, the mean of the
      reference and of ``aggregate_gradients``.  Any finite value but 0 (negative ones included).
    device: where the bucket lives (default: the current GPU).

  A row counts as touched when ANY rank touched it: the ``touched`` words travel in the same allreduce."""

  def __init__(self, shapes, coll=None, scale=None, device=None):
    self._lib = _lib.lib()
    self.shapes = [(int(r), int(d)) for r, d in shapes]
    for c, (rows, dim) in enumerate(self.shapes):
      if rows < 0 or rows >= 2 ** 31 or dim < 1:
        raise _bad(f'ReplicatedGradients: table {c}: rows must be in [0, 2^31) and dim >= 1, got {(rows, dim)}')
      if dim > 256 or (dim % 4 != 0 and dim > 64):
        raise _bad(f'ReplicatedGradients: table {c}: dim {dim} is beyond what the sparse apply takes (at most 256 '
                   'with dim % 4 == 0, 64 otherwise)')
    self.coll = coll
    world = coll.world_size if coll is not None else 1
    self.scale = 1.0 / world if scale is None else float(scale)
    if not math.isfinite(self.scale) or self.scale == 0.0:
      raise _bad(f'ReplicatedGradients: scale must be finite and != 0 (the touched words travel in the same '
                 f'allreduce: a zero scale would erase them), got {scale!r}')
    if world <= 1 and self.scale != 1.0:
      raise _bad('ReplicatedGradients: a scale other than 1 needs a collective over more than one rank (the '
                 'allreduce applies it)')
    if device is None:
      device = torch.device('cuda', torch.cuda.current_device())
    self.device = torch.device(device)
    n = len(self.shapes)
    b_off, t_off, total = replica_bucket_layout(self.shapes)
    if total >= 2 ** 31:
      raise _bad(f'ReplicatedGradients: a bucket of {total} floats: must stay below 2^31')
    self.bucket = torch.zeros(max(total, 1), dtype=torch.float32, device=self.device)
    self.blocks = [self.bucket[o:o + r * d].view(r, d) for o, (r, d) in zip(b_off, self.shapes)]
    self.touched = [self.bucket[o:o + r] for o, (r, _) in zip(t_off, self.shapes)]
    flat = torch.empty(max(sum(r for r, _ in self.shapes), 1), dtype=torch.int64, device=self.device)
    self.urows = list(torch.split(flat[:sum(r for r, _ in self.shapes)], [r for r, _ in self.shapes])) if n else []
    self._counts = torch.tensor([r for r, _ in self.shapes] or [0], dtype=torch.int32, device=self.device)
    self.counts = [self._counts[c:c + 1] for c in range(n)]
    self._cols = (_lib.ReplicaColumn * n)()
    for c, (rows, dim) in enumerate(self.shapes):
      col = self._cols[c]
      col.rows, col.dim = rows, dim
      col.block = self.blocks[c].data_ptr()
      col.touched = self.touched[c].data_ptr()
      col.urows = self.urows[c].data_ptr()
    self._keep = None

  def __len__(self):
    return len(self.shapes)

  def slices(self):
    """Per table ``(urows int64 [rows], block fp32 [rows, dim], count int32 [1] = rows)``: the aggregated
    IndexedSlices with holes, views of this object's buffers (valid until the next :meth:`aggregate`)."""
    return [(self.urows[c], self.blocks[c], self.counts[c]) for c in range(len(self.shapes))]

  def pack(self, slices):
    """This rank's ``slices[c] = (unique_rows, grad_rows, n_unique)`` scattered into the cleared bucket."""
    n = len(self.shapes)
    slices = list(slices)
    if len(slices) != n:
      raise _bad(f'ReplicatedGradients: {len(slices)} slices for {n} tables')
    for c, s in enumerate(slices):
      if len(s) != 3:
        raise _bad(f'slices[{c}] must be (unique_rows, grad_rows, n_unique)')
      urows, grows, nu = s
      for x, what in ((urows, 'unique_rows'), (grows, 'grad_rows'), (nu, 'n_unique')):
        if not isinstance(x, torch.Tensor):
          raise _bad(f'slices[{c}].{what} must be a device tensor')
        _lib.require_device_tensor(x, f'slices[{c}].{what}')
      if urows.dtype != torch.int64 or urows.dim() != 1:
        raise _bad(f'slices[{c}].unique_rows must be an int64 vector')
      cap, dim = int(urows.shape[0]), self.shapes[c][1]
      if grows.dtype != torch.float32 or tuple(grows.shape) != (cap, dim):
        raise _bad(f'slices[{c}].grad_rows must be fp32 [{cap}, {dim}]')
      if nu.dtype != torch.int32 or nu.numel() != 1:
        raise _bad(f'slices[{c}].n_unique must be an int32 device tensor of one element')
      col = self._cols[c]
      col.unique_rows = urows.data_ptr()
      col.grad_rows = grows.data_ptr()
      col.n_unique = nu.data_ptr()
      col.capacity = cap
    self._keep = slices
    self.launch_pack()

  def launch_pack(self):
    """The pack of the last bound slices again (refilled in place): one foreign call, capturable."""
    _lib.check(self._lib.hbk_replica_grads_pack_n(len(self.shapes), self._cols, self.bucket.data_ptr(),
                                                  self.bucket.numel(), _lib.current_stream(self.device)))

  def launch_rows(self):
    """``urows`` from the bucket's touched words: one foreign call, capturable."""
    _lib.check(self._lib.hbk_replica_grads_rows_n(len(self.shapes), self._cols,
                                                  _lib.current_stream(self.device)))

  def aggregate(self, slices):
    """Pack, ONE allreduce of the whole bucket (SUM, times ``scale``, in place), rows.  Returns :meth:`slices`:
    every row any rank touched, with ``g = fp32(sum over ranks) * fp32(scale)``, rows nobody touched as ``-1``.
    A collective: every rank calls it at the same point of its step."""
    self.pack(slices)
    if self.coll is not None and self.coll.world_size > 1:
      self.coll.allreduce_n([self.bucket], Collective.SUM, self.scale, outs=[self.bucket])
    self.launch_rows()
    return self.slices()
