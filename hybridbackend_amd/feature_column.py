"""Embedding feature columns -> one dense block: host mirror of what the reference's users build
with ``tf.feature_column.embedding_column`` + ``tf.keras.layers.DenseFeatures`` /
``hb.keras.layers.dense_features`` (hybridbackend/tensorflow/keras/layers/__init__.py:29-46,
docs/tutorial/ranking/taobao/train_keras.py:60-75) under ``hb.scope(sharding=True)``
(hybridbackend/tensorflow/embedding/variables.py:77-146, sharding.py:171-205).

All columns are looked up by ONE fused launch (``hbk_group_lookup_fwd``) or one sharded step
(``hbk_sharded_lookup_fwd``), and every column writes its block of the concatenated
``[batch, sum of dims]`` tensor in place (``out_stride``): there is no per-column output and no
concat pass.  The backward reads the blocks of the incoming gradient in place the same way.
"""
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding.lookup import GroupLookup
from hybridbackend_amd.embedding.lookup import GroupLookupGrad
from hybridbackend_amd.embedding import optimizer as _opt
from hybridbackend_amd.embedding.sharded import ShardedGroupLookup
from hybridbackend_amd.embedding.variables import sharded_bucket_size


class EmbeddingColumn:
  """``embedding_column(categorical_column_with_identity/hash_bucket(key, num_buckets),
  dimension, combiner)``: ids are bucketized with floor-mod ``num_buckets``
  (docs/tutorial/ranking/data.py:179,186).  ``hot_rows``: the ids are skewed (Zipf heads) --
  a wide column (dimension >= 64, one id per sample) then fetches the rows repeated inside a
  256-sample tile once and serves the repeats from LDS (GroupLookup(hot_rows=)).  The default
  ``'auto'`` lets the layer decide per column from what the last backward saw (distinct rows <
  half the ids: on); True / False pin it.  ``dedup``: a sharded column sends every distinct id of
  a batch once (ShardedGroupLookup(dedup=); the tutorials' tf.unique in front of the lookup).
  ``weight_feature_key``: ``tf.feature_column.weighted_categorical_column``'s -- the features hold
  one fp32 weight per id under this key (the ``sp_weights`` of embedding_lookup_sparse: sum of
  ``w e``, mean divides by the sum of the weights, sqrtn by the root of the sum of their squares; a
  sample whose divisor is 0 gives a zero row).  Nothing is pruned: unlike TF's
  ``safe_embedding_lookup_sparse``, ids with weight <= 0 stay in the sums, so callers pass positive
  weights for that behaviour.  ``max_norm``: ``embedding_column(max_norm=)`` -- every looked-up row is
  clipped to an L2 norm of at most ``max_norm`` before its weight and the combine, and the gradient
  goes through the clip (GroupLookup(max_norms=), ShardedGroupLookup(max_norms=)); None: no clip."""

  def __init__(self, key, num_buckets, dimension, combiner='mean', hot_rows='auto', dedup=False,
               weight_feature_key=None, max_norm=None):
    if num_buckets < 1 or dimension < 1:
      raise _lib.InvalidArgumentError(
        _lib.INVALID_ARGUMENT, 'num_buckets and dimension must be >= 1')
    self.key, self.num_buckets, self.dimension = key, int(num_buckets), int(dimension)
    self.combiner = combiner
    self.hot_rows = 'auto' if hot_rows == 'auto' else bool(hot_rows)
    self.dedup = bool(dedup)
    self.weight_feature_key = weight_feature_key
    from hybridbackend_amd.embedding.lookup import max_norm_list
    self.max_norm = None if max_norm is None else max_norm_list([max_norm], 1)[0]


class _TableLayer:
  """What DenseFeatures and SequenceFeatures share: one table per column, replicated or sharded by the
  reference's rule, the optimizer slots, and the checkpoints."""

  def _init_tables(self, columns, device, coll, batch_size, init, initial_accumulator_value, optimizer,
                   adam, ftrl):
    self.columns = list(columns)
    self.device = torch.device(device)
    self.coll = coll
    world = coll.world_size if coll is not None else 1
    rank = coll.rank if coll is not None else 0
    if init is None:
      def init(col, rows, dev):
        return torch.empty(rows, col.dimension, device=dev).uniform_(-1e-3, 1e-3)
    self.sharded, self.weights = [], []
    for col in self.columns:
      is_sharded, rows, _ = sharded_bucket_size(col.num_buckets, world, rank, batch_size)
      is_sharded = is_sharded and world > 1
      self.sharded.append(is_sharded)
      self.weights.append(init(col, rows if is_sharded else col.num_buckets, self.device))
    # Adagrad accumulators (tf.train.AdagradOptimizer: initial_accumulator_value = 0.1)
    self.accums = None
    if initial_accumulator_value is not None:
      self.accums = [torch.full_like(w, float(initial_accumulator_value)) for w in self.weights]
    if optimizer is not None:
      _opt.two_slot_class(optimizer)   # (refuses unknown names)
    # two-slot optimizers: the optimizer named (TF's defaults) or passed, fresh slots for every table
    # (Lazy Adam: m = v = 0; FTRL: accum = initial_accumulator_value, linear = 0)
    self.moments = self.adam = self.ftrl_slots = self.ftrl = None
    for cls, opt in ((_opt.LazyAdam, adam), (_opt.Ftrl, ftrl)):
      if optimizer == cls.name or opt is not None:
        opt = opt if opt is not None else cls.default(self.device)
        setattr(self, cls.name, opt)
        setattr(self, cls.slot_kw, [opt.slots_like(w) for w in self.weights])
    self._rep = [c for c in range(len(self.columns)) if not self.sharded[c]]
    self._shd = [c for c in range(len(self.columns)) if self.sharded[c]]

  def _two_slot_kw(self, idx):
    """The drivers' keyword arguments of the two-slot optimizers, tables idx."""
    kw = {}
    for cls in _opt.TWO_SLOT.values():
      pairs = getattr(self, cls.slot_kw)
      kw[cls.slot_kw] = None if pairs is None else [pairs[c] for c in idx]
      kw[cls.name] = getattr(self, cls.name)
    return kw

  # ---- checkpoints (hybridbackend/tensorflow/training/saver.py:97-185) ----------------------------
  def variables(self):
    """``{name: tensor | ShardedSlice}`` of this rank: the embedding weights (TF naming:
    ``<key>_embedding/embedding_weights``; a sharded table is the slice ``part_<rank>`` of it,
    variables.py:112-141) and, when the layer keeps them, the Adagrad slots (``.../Adagrad``) or the
    Lazy Adam slots (``.../Adam`` = m, ``.../Adam_1`` = v, sharded as the weights) with the 0-d
    scalars ``beta1_power`` and ``beta2_power``, or the FTRL slots (``.../Ftrl`` = accum,
    ``.../Ftrl_1`` = linear, sharded as the weights)."""
    from hybridbackend_amd.training.saver import ShardedSlice
    world = self.coll.world_size if self.coll is not None else 1
    rank = self.coll.rank if self.coll is not None else 0
    per_table = [('', self.weights), ('/Adagrad', self.accums)]
    extra = {}
    for cls in _opt.TWO_SLOT.values():
      pairs = getattr(self, cls.slot_kw)
      if pairs is not None:
        per_table += [(cls.tf_suffixes[0], [a for a, _ in pairs]),
                      (cls.tf_suffixes[1], [b for _, b in pairs])]
        extra.update(getattr(self, cls.name).tf_variables())
    out = {}
    for c, col in enumerate(self.columns):
      name = f'{col.key}_embedding/embedding_weights'
      for suffix, tensors in per_table:
        if tensors is None:
          continue
        t = tensors[c]
        out[name + suffix] = (ShardedSlice(t, col.num_buckets, world, rank)
                              if self.sharded[c] else t)
    out.update(extra)
    return out

  def _saver(self, barrier):
    from hybridbackend_amd.training.saver import Saver
    world = self.coll.world_size if self.coll is not None else 1
    rank = self.coll.rank if self.coll is not None else 0
    if barrier is None and world > 1:
      import torch.distributed as dist   # pylint: disable=import-outside-toplevel
      if not dist.is_initialized():
        raise _lib.HbkError(_lib.INTERNAL, 'save/restore at W > 1 needs a barrier '
                                           '(torch.distributed is not initialized)')
      barrier = dist.barrier
    return Saver(rank, world, barrier)

  def save(self, prefix, barrier=None):
    """Every rank writes its shards, rank 0 also the replicated tables and the index; all ranks
    call this together.  The device work of the current stream is waited for first."""
    if self.device.type == 'cuda':
      torch.cuda.current_stream(self.device).synchronize()
    return self._saver(barrier).save(prefix, self.variables())

  def restore(self, prefix, barrier=None, layout='logical'):
    """Loads this rank's rows from a checkpoint written at ANY world size (``layout='reference'``:
    the reference's contiguous slicing instead, see training/saver.py)."""
    self._saver(barrier).restore(prefix, self.variables(), layout=layout)

  def restore_reference(self, prefix, names=None, barrier=None, layout='logical'):
    """Loads this rank's rows from a checkpoint the REFERENCE saved (TensorFlow tensor bundle,
    training/tf_bundle.py), written at any world size.  ``names``: ``{name here: tensor name in
    the checkpoint}`` for variables the model named differently (default: the TF names of
    ``variables()``).  layout: see ``Saver.restore_reference``."""
    self._saver(barrier).restore_reference(prefix, self.variables(), names=names, layout=layout)

  def close(self):
    if self._sharded is not None:
      self._sharded.close()


class DenseFeatures(_TableLayer):
  """N embedding columns -> ``[batch, sum of dims]``.

  Args:
    columns: list of :class:`EmbeddingColumn`.
    device: the GPU.
    coll: a ``hybridbackend_amd.distribute.Collective`` for sharded tables, or None.
    batch_size: local batch size used by the replicate-or-shard rule
      (``bucket_size <= num_shards or bucket_size <= batch_size`` keeps a table replicated,
      variables.py:93-104).
    init: ``init(column, rows, device) -> fp32 [rows, dim]`` for this rank's rows (rows
      ``rank, rank + W, ..`` of the logical table when sharded); default uniform(-1e-3, 1e-3)
      (docs/tutorial/ranking/criteo/train.py:84,91).
    initial_accumulator_value: keep Adagrad accumulators (``optimizer='adagrad'``).
    optimizer: ``'adam'`` keeps Lazy Adam slots -- zero ``m`` and ``v`` for every table -- for
      ``backward(optimizer='adam')``; ``adam`` is the :class:`LazyAdam` they step with (TF's
      defaults when omitted), whose beta powers advance once per stepped backward.  ``'ftrl'`` keeps
      FTRL slots -- accum filled with ``ftrl.initial_accumulator_value``, zero linear -- for
      ``backward(optimizer='ftrl')``; ``ftrl`` is the :class:`Ftrl` they step with (TF's defaults
      when omitted).
  """

  def __init__(self, columns, device, coll=None, batch_size=0, init=None,
               initial_accumulator_value=None, optimizer=None, adam=None, ftrl=None):
    self._init_tables(columns, device, coll, batch_size, init, initial_accumulator_value, optimizer,
                      adam, ftrl)
    self.offsets, off = [], 0
    for col in self.columns:
      self.offsets.append(off)
      off += col.dimension
    self.width = off
    # columns whose block the kernels cannot address: a row of more than 64 floats needs 16-byte
    # chunks, so it must start on a 16-byte boundary of the row.  Such a column is looked up into a
    # tensor of its own and copied into the block, and its gradient is handed over as a contiguous
    # copy of its block; every other column keeps the block's addresses.
    self._staged = {c for c, col in enumerate(self.columns)
                    if col.dimension > 64 and self.offsets[c] % 4 != 0}
    pick = lambda idx, xs: [xs[c] for c in idx]   # noqa: E731
    two_slot_kw = self._two_slot_kw
    self._lookup = self._grad = self._sharded = None
    if self._rep:
      self._lookup = GroupLookup(pick(self._rep, self.weights),
                                 [self.columns[c].num_buckets for c in self._rep],
                                 [self.columns[c].combiner for c in self._rep],
                                 hot_rows=[self.columns[c].hot_rows for c in self._rep],
                                 max_norms=[self.columns[c].max_norm for c in self._rep])
      self._grad = GroupLookupGrad(
        self._lookup, pick(self._rep, self.accums) if self.accums is not None else None,
        **two_slot_kw(self._rep))
    if self._shd:
      self._sharded = ShardedGroupLookup(pick(self._shd, self.weights), coll,
                                         buckets=[self.columns[c].num_buckets for c in self._shd],
                                         combiners=[self.columns[c].combiner for c in self._shd],
                                         hot_rows=[self.columns[c].hot_rows for c in self._shd],
                                         dedup=[self.columns[c].dedup for c in self._shd],
                                         max_norms=[self.columns[c].max_norm for c in self._shd],
                                         accums=(pick(self._shd, self.accums)
                                                 if self.accums is not None else None),
                                         **two_slot_kw(self._shd))

  def _weights(self, features):
    """Per column its fp32 per-id weights (weight_feature_key) or None; None when no column has any."""
    ws = [features[col.weight_feature_key] if col.weight_feature_key is not None else None
          for col in self.columns]
    return ws if any(w is not None for w in ws) else None

  def _split(self, features):
    ids, splits, batch = [], [], None
    for col in self.columns:
      f = features[col.key]
      i, s = f if isinstance(f, (tuple, list)) else (f, None)
      n = i.numel() if s is None else s.numel() - 1
      if batch is not None and n != batch:
        raise _lib.InvalidArgumentError(
          _lib.INVALID_ARGUMENT, f'feature {col.key}: {n} samples, expected {batch}')
      batch = n
      ids.append(i)
      splits.append(s)
    return ids, splits, batch

  def __call__(self, features, cols_to_output_tensors=None):
    """features[key] = int64 ids ``[batch]`` (one id per sample) or ``(values, row_splits)``
    (the values + row_splits layout of hybridbackend/tensorflow/data/dataframe.py:366-376).
    Returns the dense block; ``cols_to_output_tensors`` (a dict) receives each column's view."""
    ids, splits, batch = self._split(features)
    ws = self._weights(features)
    # rows start on 16-byte boundaries (row stride padded to 4 floats) so that columns whose
    # offset is a multiple of 4 floats keep 16-byte accesses
    pitch = (self.width + 3) // 4 * 4
    out = torch.empty((batch or 0, pitch), dtype=torch.float32, device=self.device)[:, :self.width]
    pick = lambda idx, xs: [xs[c] for c in idx]   # noqa: E731
    pick_w = lambda idx: None if ws is None else pick(idx, ws)   # noqa: E731
    views = None

    def col_views():
      return [out[:, self.offsets[c]:self.offsets[c] + self.columns[c].dimension]
              for c in range(len(self.columns))]
    # the kernels' outputs: the block's views, a tensor of its own for a staged column
    dests = None
    if self._staged:
      views = col_views()
      dests = [torch.empty((batch or 0, self.columns[c].dimension), dtype=torch.float32,
                           device=self.device) if c in self._staged else views[c]
               for c in range(len(self.columns))]
    if self._rep:
      # the blocks' addresses are arithmetic: no per-column views unless somebody asks for them
      # (26 views + their validation were ~100 us of Python per step)
      if (batch and dests is None and
          self._lookup.bind_block(pick(self._rep, ids), pick(self._rep, splits), out,
                                  pick(self._rep, self.offsets), sp_weights=pick_w(self._rep))):
        self._lookup.launch()
      else:
        views = views or col_views()
        self._lookup(pick(self._rep, ids), pick(self._rep, splits), pick(self._rep, dests or views),
                     sp_weights=pick_w(self._rep))
    if self._shd:
      views = views or col_views()
      self._sharded(pick(self._shd, ids), pick(self._shd, splits), pick(self._shd, dests or views),
                    sp_weights=pick_w(self._shd))
    for c in self._staged:
      views[c].copy_(dests[c])
    self._last = (ids, splits, ws)
    if cols_to_output_tensors is not None:
      views = views or col_views()
      for c, col in enumerate(self.columns):
        cols_to_output_tensors[col] = views[c]
    return out

  def prefetch(self, features, ids_ready=None):
    """The NEXT step's features, as soon as the loader has them on the device: the sharded
    columns' bucketize + partition + size exchange run on the plan's stream beside the step in
    flight (``ShardedGroupLookup.prefetch``); the forward over the same tensors picks them up.
    A no-op for a layer whose columns are all replicated.  All ranks prefetch the same steps."""
    if self._shd:
      ids, _, _ = self._split(features)
      self._sharded.prefetch([ids[c] for c in self._shd], ids_ready)

  def backward(self, grad, apply_lr=0.0, optimizer='sgd', emit=True, weight_grads=False):
    """grad: ``[batch, sum of dims]`` gradient of the last forward's output.  Returns per column
    the ``IndexedSlices`` ``(unique_rows, grad_rows, n_unique)`` of this rank's rows (local row
    numbers for sharded tables); with ``apply_lr`` the sparse optimizer step (``'sgd'``, or
    ``'adagrad'`` when the layer was built with ``initial_accumulator_value``) is applied in the
    same pass -- for the SHARDED tables.  Small tables are replicated on every rank: at W > 1
    their gradients must first be aggregated across ranks (``hb.distribute.aggregate_gradients``,
    hybridbackend/tensorflow/training/gradient.py:119-177) or the replicas diverge, so for them
    this method never applies the step at W > 1: it returns their IndexedSlices and the caller
    applies the aggregated gradient.  ``emit=False`` (with ``apply_lr``): the stepped tables
    write no IndexedSlices (step only; their entries are ``(None, None, n_unique)``).
    ``optimizer='adam'`` (layer built with ``optimizer='adam'``): the Lazy Adam step; the beta powers
    advance once per backward that steps any table.  ``optimizer='ftrl'`` (layer built with
    ``optimizer='ftrl'``): the FTRL-Proximal step.
    ``weight_grads=True``: returns ``(slices, {weight_feature_key: tensor})`` -- the gradient of every
    weighted column's per-id weights (fp32 ``[n_ids]``; replicated and sharded tables alike, taken at the
    rows as the forward read them), an empty dict for a layer without weighted columns."""
    _opt.two_slot_class(optimizer, self, "DenseFeatures(..., optimizer='{name}')")
    ids, splits, ws = self._last
    if grad.dim() != 2 or grad.shape[1] != self.width or grad.dtype != torch.float32:
      raise _lib.InvalidArgumentError(
        _lib.INVALID_ARGUMENT, f'grad must be fp32 [batch, {self.width}]')
    if grad.stride(1) != 1 or grad.stride(0) % 4 != 0:
      # same pitch as the forward's block: rows on 16-byte boundaries (one extra copy)
      pitch = (self.width + 3) // 4 * 4
      padded = torch.empty((grad.shape[0], pitch), dtype=torch.float32,
                           device=grad.device)[:, :self.width]
      padded.copy_(grad)
      grad = padded
    pick = lambda idx, xs: [xs[c] for c in idx]   # noqa: E731
    res = [None] * len(self.columns)
    wgrads = {}

    def want(idx):
      # the weighted columns among `idx` (False: none, and the callee is called as without the flag)
      if not weight_grads or ws is None:
        return False
      w = [True if ws[c] is not None else None for c in idx]
      return w if any(w) else False

    def take(idx, r):
      # a callee that was asked returns (slices, weight gradients)
      if not isinstance(r, tuple):
        return r
      for c, g in zip(idx, r[1]):
        if g is not None:
          wgrads[self.columns[c].weight_feature_key] = g
      return r[0]

    def col_grads():
      return [grad[:, self.offsets[c]:self.offsets[c] + self.columns[c].dimension]
              for c in range(len(self.columns))]
    if self._rep:
      rep_lr = apply_lr if (self.coll.world_size if self.coll is not None else 1) <= 1 else 0.0
      # the gradient's column blocks are addressed by arithmetic (no per-column views)
      # one optimizer step: the powers advance with the last call that steps (the sharded one)
      grads, grad_block = None, (grad, pick(self._rep, self.offsets))
      if any(c in self._staged for c in self._rep):
        views = col_grads()
        grads = [views[c].contiguous() for c in self._rep]
        grad_block = None
      r = self._grad(pick(self._rep, ids), grads, pick(self._rep, splits),
                     apply_lr=rep_lr, optimizer=optimizer, emit=emit or rep_lr == 0.0,
                     grad_block=grad_block,
                     sp_weights=None if ws is None else pick(self._rep, ws),
                     finish=not (self._shd and apply_lr != 0.0), weight_grads=want(self._rep))
      r = take(self._rep, r)
      for k, c in enumerate(self._rep):
        res[c] = r[k]
    if self._shd:
      views = [grad[:, self.offsets[c]:self.offsets[c] + self.columns[c].dimension]
               for c in self._shd]
      views = [v.contiguous() if c in self._staged else v for c, v in zip(self._shd, views)]
      r = self._sharded.backward(views, apply_lr=apply_lr, optimizer=optimizer,
                                 emit=emit, weight_grads=want(self._shd))
      r = take(self._shd, r)
      for k, c in enumerate(self._shd):
        res[c] = r[k]
    if weight_grads:
      return res, wgrads
    return res


def dense_features(features, layer):
  """``hb.keras.layers.dense_features``: the per-column tensors, in column order."""
  m = {}
  layer(features, cols_to_output_tensors=m)
  return [m[c] for c in layer.columns]


class SequenceEmbeddingColumn:
  """``embedding_column(sequence_categorical_column_with_identity/hash_bucket(key, num_buckets),
  dimension)`` -- or the DIN tutorial's ``transform_categorical_non_pooling``
  (docs/tutorial/ranking/data.py:195-224): a ragged id list looked up WITHOUT a combiner into
  ``[batch, max_len, dimension]``.  A sample's first ``max_len`` ids are looked up (``tf.sparse.slice``);
  ``pad_id`` None: the positions past a sample's length are zero rows that take part in nothing (TF's
  ``SequenceFeatures``); ``pad_id`` set (``0 <= pad_id < num_buckets``): they look that id up
  (``tf.sparse.to_dense(default_value=)``) and its row collects their gradient.  ``max_norm`` and
  ``dedup`` are EmbeddingColumn's.  A column whose table is sharded needs a ``pad_id``."""

  def __init__(self, key, num_buckets, dimension, max_len, pad_id=None, max_norm=None, dedup=False):
    from hybridbackend_amd.embedding.lookup import max_norm_list
    from hybridbackend_amd.embedding.sequence import check_sequence_args
    if num_buckets < 1 or dimension < 1:
      raise _lib.InvalidArgumentError(
        _lib.INVALID_ARGUMENT, 'num_buckets and dimension must be >= 1')
    self.key, self.num_buckets, self.dimension = key, int(num_buckets), int(dimension)
    _, (self.max_len,), (self.pad_id,) = check_sequence_args(1, [self.num_buckets], max_len, pad_id)
    self.max_norm = None if max_norm is None else max_norm_list([max_norm], 1)[0]
    self.dedup = bool(dedup)


class SequenceFeatures(_TableLayer):
  """N sequence columns -> per column ``[batch, max_len, dimension]`` rows and the int32 ``[batch]``
  lengths (``tf.keras.experimental.SequenceFeatures``; the columns may differ in ``max_len``, so there is
  no concatenated block).  Arguments, tables, optimizer slots, the replicate-or-shard rule and the
  checkpoint names are :class:`DenseFeatures`'.

  Replicated tables go through ``SequenceLookup`` / ``SequenceLookupGrad``.  A sharded table (W > 1) is
  looked up through ``ShardedGroupLookup`` as ``batch * max_len`` ids of one sample each, over the grid
  ``sequence_row_grid`` builds.  The sharded step bucketizes its ids again, which would carry the ``-1`` of
  a zero-padded position to row ``num_buckets - 1``: a sharded sequence column therefore requires a
  ``pad_id`` (zero-padded sequences on sharded tables are not provided)."""

  def __init__(self, columns, device, coll=None, batch_size=0, init=None,
               initial_accumulator_value=None, optimizer=None, adam=None, ftrl=None):
    from hybridbackend_amd.embedding.sequence import SequenceLookup, SequenceLookupGrad
    self._init_tables(columns, device, coll, batch_size, init, initial_accumulator_value, optimizer,
                      adam, ftrl)
    for c in self._shd:
      col = self.columns[c]
      if col.pad_id is None:
        raise _lib.InvalidArgumentError(
          _lib.INVALID_ARGUMENT,
          f'sequence column {col.key!r}: its table is sharded over {coll.world_size} ranks, and a sharded '
          'sequence column requires a pad_id (the sharded step bucketizes the id grid again, which would '
          'turn the -1 of a zero-padded position into a row; zero padding is for replicated tables)')
    pick = lambda idx, xs: [xs[c] for c in idx]   # noqa: E731
    attr = lambda idx, name: [getattr(self.columns[c], name) for c in idx]   # noqa: E731
    self._lookup = self._grad = self._sharded = None
    if self._rep:
      self._lookup = SequenceLookup(pick(self._rep, self.weights), attr(self._rep, 'num_buckets'),
                                    max_lens=attr(self._rep, 'max_len'), pad_ids=attr(self._rep, 'pad_id'),
                                    max_norms=attr(self._rep, 'max_norm'))
      self._grad = SequenceLookupGrad(
        self._lookup, pick(self._rep, self.accums) if self.accums is not None else None,
        **self._two_slot_kw(self._rep))
    if self._shd:
      self._sharded = ShardedGroupLookup(pick(self._shd, self.weights), coll,
                                         buckets=attr(self._shd, 'num_buckets'), combiners='sum',
                                         dedup=attr(self._shd, 'dedup'),
                                         max_norms=attr(self._shd, 'max_norm'),
                                         accums=(pick(self._shd, self.accums)
                                                 if self.accums is not None else None),
                                         **self._two_slot_kw(self._shd))

  def __call__(self, features):
    """features[key] = ``(values, row_splits)`` (int32/int64 ids, int32 ``[batch + 1]``), or an id vector
    (one id per sample).  Returns ``(outputs, lengths)``, two lists in column order."""
    from hybridbackend_amd.embedding.sequence import sequence_row_grid
    ids, splits, batch = [], [], None
    for col in self.columns:
      f = features[col.key]
      i, s = f if isinstance(f, (tuple, list)) else (f, None)
      n = i.numel() if s is None else s.numel() - 1
      if batch is not None and n != batch:
        raise _lib.InvalidArgumentError(
          _lib.INVALID_ARGUMENT, f'feature {col.key}: {n} samples, expected {batch}')
      batch = n
      ids.append(i)
      splits.append(s)
    pick = lambda idx, xs: [xs[c] for c in idx]   # noqa: E731
    outs, lengths = [None] * len(self.columns), [None] * len(self.columns)
    if self._rep:
      o, ln = self._lookup(pick(self._rep, ids), pick(self._rep, splits))
      for k, c in enumerate(self._rep):
        outs[c], lengths[c] = o[k], ln[k]
    if self._shd:
      cols = pick(self._shd, self.columns)
      grids, ln = sequence_row_grid(pick(self._shd, ids), pick(self._shd, splits),
                                    [col.num_buckets for col in cols], [col.max_len for col in cols],
                                    [col.pad_id for col in cols])
      o = self._sharded(grids)
      for k, c in enumerate(self._shd):
        outs[c] = o[k].view(batch or 0, cols[k].max_len, cols[k].dimension)
        lengths[c] = ln[k]
    return outs, lengths

  def backward(self, grads, apply_lr=0.0, optimizer='sgd', emit=True):
    """grads[c]: the gradient of the last forward's ``outputs[c]``.  Returns per column the
    ``IndexedSlices`` ``(unique_rows, grad_rows, n_unique)`` of this rank's rows, as
    ``DenseFeatures.backward`` does and with its rule for the step: the sharded tables are stepped in the
    same pass, replicated tables are stepped only at W = 1 (at W > 1 their gradients must be aggregated
    across ranks first; their IndexedSlices are returned)."""
    _opt.two_slot_class(optimizer, self, "SequenceFeatures(..., optimizer='{name}')")
    if len(grads) != len(self.columns):
      raise _lib.InvalidArgumentError(
        _lib.INVALID_ARGUMENT, f'expected {len(self.columns)} gradients, got {len(grads)}')
    res = [None] * len(self.columns)
    if self._rep:
      rep_lr = apply_lr if (self.coll.world_size if self.coll is not None else 1) <= 1 else 0.0
      # one optimizer step: the powers advance with the last call that steps (the sharded one)
      r = self._grad([grads[c] for c in self._rep], apply_lr=rep_lr, optimizer=optimizer,
                     emit=emit or rep_lr == 0.0, finish=not (self._shd and apply_lr != 0.0))
      for k, c in enumerate(self._rep):
        res[c] = r[k]
    if self._shd:
      flat = [grads[c].contiguous().view(grads[c].shape[0] * self.columns[c].max_len, self.columns[c].dimension)
              for c in self._shd]
      r = self._sharded.backward(flat, apply_lr=apply_lr, optimizer=optimizer, emit=emit)
      for k, c in enumerate(self._shd):
        res[c] = r[k]
    return res
