"""Embedding feature columns -> one dense block: host mirror of what the reference's users build
with ``tf.feature_column.embedding_column`` + ``tf.keras.layers.DenseFeatures`` /
``hb.keras.layers.dense_features`` (hybridbackend/tensorflow/keras/layers/__init__.py:29-46,
docs/tutorial/ranking/taobao/train_keras.py:60-75) under ``hb.scope(sharding=True)``
(hybridbackend/tensorflow/embedding/variables.py:77-146, sharding.py:171-205).

All columns are looked up by ONE fused launch (``hbk_group_lookup_fwd``) or one sharded step
(``hbk_sharded_lookup_fwd``), and every column writes its block of the concatenated
``[batch, sum of dims]`` tensor in place (``out_stride``): there is no per-column output and no
concat pass.  The backward reads the blocks of the incoming gradient in place the same way.

Hash-keyed columns (:class:`HashEmbeddingColumn`, :class:`HashSequenceEmbeddingColumn`) are what the
reference's users get from ``embedding_column`` under DeepRec (``embedding/deeprecev.py`` hooks
``get_embedding_variable`` into the sharded rewrite): the table is a :class:`HashTable` keyed by the raw ids.
The layers keep the tables, their optimizer slots and the lookup objects together, so the "void after a
rehash" rules of the hand composition stay inside ``maybe_grow`` / ``maybe_evict``.
"""
import re

import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding.hashtable import HashExport
from hybridbackend_amd.embedding.hashtable import HashGroupLookup
from hybridbackend_amd.embedding.hashtable import HashTable
from hybridbackend_amd.embedding.lookup import GroupLookup
from hybridbackend_amd.embedding.lookup import GroupLookupGrad
from hybridbackend_amd.embedding import optimizer as _opt
from hybridbackend_amd.embedding.sharded import ShardedGroupLookup
from hybridbackend_amd.embedding.sharded_hash import ShardedHashGroupLookup
from hybridbackend_amd.embedding.sharded_hash import slot_companions
from hybridbackend_amd.embedding.sharded_hash import slot_kinds
from hybridbackend_amd.embedding.variables import sharded_bucket_size


def _bad(msg):
  return _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, msg)


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


class _HashColumn:
  """What the hash-keyed columns share: the arguments of the column's :class:`HashTable`, checked when the
  column is made (a table on the ``meta`` device allocates nothing and refuses what every table refuses)."""

  def _init_table_args(self, key, capacity, dimension, max_norm, dedup, slab_size, init_scale, seed, expiring,
                       min_freq, sketch_depth, sketch_width, sketch_seed, dtype=torch.float32):
    from hybridbackend_amd.embedding.lookup import max_norm_list
    self.key, self.capacity, self.dimension = key, int(capacity), int(dimension)
    self.table_args = dict(slab_size=int(slab_size), init_scale=float(init_scale), seed=int(seed),
                           expiring=bool(expiring), min_freq=int(min_freq), sketch_depth=sketch_depth,
                           sketch_width=sketch_width, sketch_seed=sketch_seed)
    if dtype != torch.float32:
      # (the default adds no argument: an fp32 column builds the table it always built; HashTable refuses an
      # unknown dtype, an odd dim and an fp16 init_scale above 65504 when the probe below is made)
      self.table_args['dtype'] = dtype
    self.dtype = dtype
    self.expiring = bool(expiring)
    self._probe = HashTable(self.capacity, self.dimension, 'meta', **self.table_args)
    self.max_norm = None if max_norm is None else max_norm_list([max_norm], 1)[0]
    self.dedup = bool(dedup)

  def local_capacity(self, world):
    """The slots of one rank's table: ``capacity`` at W = 1 (whole slabs: HashTable rounds down), else
    ``ceil(capacity / W)`` rounded UP to whole slabs."""
    if world <= 1:
      return self.capacity
    slab = self.table_args['slab_size']
    return (-(-self.capacity // world) + slab - 1) // slab * slab

  def make_table(self, device, world):
    """This rank's table.  The seed is the column's on every rank: a key's first row does not depend on W."""
    return HashTable(self.local_capacity(world), self.dimension, device, **self.table_args)


class HashEmbeddingColumn(_HashColumn):
  """``embedding_column`` over a DeepRec EmbeddingVariable (``get_embedding_variable``): the rows are keyed by the
  RAW int64 ids -- no bucketize, an open vocabulary -- in a :class:`HashTable` of ``capacity`` slots in all
  (the logical total across ranks).  ``slab_size``, ``init_scale``, ``seed``, ``expiring``, ``min_freq`` and the
  ``sketch_*`` arguments are the table's, with its refusals.  ``combiner``, ``max_norm``, ``dedup`` and
  ``weight_feature_key`` are :class:`EmbeddingColumn`'s; per-id weights work on one rank only (the sharded step
  refuses weights on a column without a bucket, so a weighted hash column is refused when a layer is built over
  more than one rank).  ``dtype``: ``torch.float32`` (the default: nothing changes), ``torch.bfloat16`` or
  ``torch.float16`` -- the column's table is ``HashTable(dtype=)`` with 2-byte rows (``dimension`` even, fp16 takes
  ``init_scale <= 65504``; refused here, when the column is made) and fp32 optimizer slots.  All hash columns of one
  layer share one dtype; on a 16-bit column ``max_norm`` and ``weight_feature_key`` are refused by the layer."""

  def __init__(self, key, capacity, dimension, combiner='mean', max_norm=None, dedup=False,
               weight_feature_key=None, slab_size=8, init_scale=1e-3, seed=0, expiring=False, min_freq=0,
               sketch_depth=4, sketch_width=None, sketch_seed=0, dtype=torch.float32):
    from hybridbackend_amd.embedding.lookup import _combiner_code
    self._init_table_args(key, capacity, dimension, max_norm, dedup, slab_size, init_scale, seed, expiring,
                          min_freq, sketch_depth, sketch_width, sketch_seed, dtype)
    _combiner_code(combiner)   # (refuses unknown names)
    self.combiner = combiner
    self.weight_feature_key = weight_feature_key


class HashSequenceEmbeddingColumn(_HashColumn):
  """:class:`SequenceEmbeddingColumn` over a :class:`HashTable`: a sample's first ``max_len`` RAW ids looked up
  into ``[batch, max_len, dimension]``.  ``pad_id`` is a raw id, any int64 the table can store (not a sentinel
  of the table); None: the positions past a sample's length are zero rows.  A column on more than one rank
  needs a ``pad_id`` or ``SequenceFeatures(..., sharded_zero_padding=True)``.  The table arguments are
  :class:`HashEmbeddingColumn`'s, ``dtype`` included."""

  def __init__(self, key, capacity, dimension, max_len, pad_id=None, max_norm=None, dedup=False, slab_size=8,
               init_scale=1e-3, seed=0, expiring=False, min_freq=0, sketch_depth=4, sketch_width=None,
               sketch_seed=0, dtype=torch.float32):
    from hybridbackend_amd.embedding.hash_sequence import check_hash_sequence_args
    self._init_table_args(key, capacity, dimension, max_norm, dedup, slab_size, init_scale, seed, expiring,
                          min_freq, sketch_depth, sketch_width, sketch_seed, dtype)
    (self.max_len,), (self.pad_id,) = check_hash_sequence_args([self._probe], max_len, pad_id)


def _is_hash(col):
  return isinstance(col, _HashColumn)


class _TableLayer:
  """What DenseFeatures and SequenceFeatures share: one table per column, replicated or sharded by the
  reference's rule (a hash-keyed column: one :class:`HashTable`, sharded by ``floormod(id, W)`` whenever
  W > 1), the optimizer slots, and the checkpoints."""

  def _init_tables(self, columns, device, coll, batch_size, init, initial_accumulator_value, optimizer,
                   adam, ftrl, train=True, rowwise_adagrad=None, table_dtype=None, lowp_sharded=False,
                   table_rounding='nearest', table_seed=0, what='DenseFeatures'):
    self.columns = list(columns)
    self._check_hash_dtype(what, table_rounding, table_seed)
    self.device = torch.device(device)
    self.coll = coll
    self.train = bool(train)
    self._initial_accumulator_value = initial_accumulator_value
    world = coll.world_size if coll is not None else 1
    rank = coll.rank if coll is not None else 0
    if init is None:
      def init(col, rows, dev):
        return torch.empty(rows, col.dimension, device=dev).uniform_(-1e-3, 1e-3)
    self.sharded, self.weights, self.hash_tables = [], [], []
    for col in self.columns:
      if _is_hash(col):
        # never replicated: slot numbers differ per rank, and replicated tables are by default not stepped at W > 1
        table = col.make_table(self.device, world)
        self.hash_tables.append(table)
        self.sharded.append(world > 1)
        self.weights.append(table.table)
        continue
      self.hash_tables.append(None)
      is_sharded, rows, _ = sharded_bucket_size(col.num_buckets, world, rank, batch_size)
      is_sharded = is_sharded and world > 1
      self.sharded.append(is_sharded)
      self.weights.append(init(col, rows if is_sharded else col.num_buckets, self.device))
    # 16-bit tables (DenseFeatures(table_dtype=)): init's result rounded to nearest; every slot below stays
    # fp32 and is built from an fp32 stand-in of the table's shape (zero strides: it owns one word)
    # DenseFeatures(lowp_sharded=True) at W > 1: the SHARDED tables only; the replicated ones stay fp32
    like = self.weights
    if table_dtype is not None:
      low = [world <= 1 or (bool(lowp_sharded) and s and h is None) for s, h in zip(self.sharded, self.hash_tables)]
      self.weights = [w.to(table_dtype) if l else w for w, l in zip(self.weights, low)]
      like = [torch.empty((), dtype=torch.float32, device=self.device).expand(w.shape) if l else w
              for w, l in zip(self.weights, low)]
    elif self.hash_dtype != torch.float32:
      # 16-bit hash columns (HashEmbeddingColumn(dtype=)): their tables are built 16-bit, their slots stay fp32
      like = [torch.empty((), dtype=torch.float32, device=self.device).expand(w.shape) if h is not None else w
              for w, h in zip(self.weights, self.hash_tables)]
    # Adagrad accumulators (tf.train.AdagradOptimizer: initial_accumulator_value = 0.1)
    self.accums = None
    if initial_accumulator_value is not None:
      self.accums = [torch.full_like(w, float(initial_accumulator_value)) for w in like]
    if optimizer is not None:
      _opt.two_slot_class(optimizer)   # (refuses unknown names)
    # slot optimizers: the optimizer named (its defaults) or passed, fresh slots for every table
    # (Lazy Adam: m = v = 0; FTRL: accum = initial_accumulator_value, linear = 0; row-wise Adagrad: one
    # [rows, 1] accumulator = its initial_accumulator_value)
    given = dict(adam=adam, ftrl=ftrl, rowwise_adagrad=rowwise_adagrad)
    for cls in _opt.TWO_SLOT.values():
      setattr(self, cls.name, None)
      setattr(self, cls.slot_kw, None)
      opt = given[cls.name]
      if optimizer == cls.name or opt is not None:
        opt = opt if opt is not None else cls.default(self.device)
        setattr(self, cls.name, opt)
        setattr(self, cls.slot_kw, [opt.slots_like(w) for w in like])
    self._hash = [c for c in range(len(self.columns)) if self.hash_tables[c] is not None]
    self._rep = [c for c in range(len(self.columns)) if not self.sharded[c] and c not in self._hash]
    self._shd = [c for c in range(len(self.columns)) if self.sharded[c] and c not in self._hash]
    # the lookup objects of the hash group: one rank (_hash_lookup + _hash_grad) or the sharded step
    self._hash_lookup = self._hash_grad = self._hash_sharded = None

  def _two_slot_kw(self, idx):
    """The drivers' keyword arguments of the slot optimizers, tables idx."""
    return _opt.slot_kwargs(self, idx)

  # ---- replicated tables at W > 1: aggregate across ranks, then step (aggregate_replicated) ---------------
  def _init_replica(self, aggregate_replicated, replicated_scale, what):
    """The cross-rank step of the replicated group: a ``ReplicatedGradients`` over its tables and a
    ``SparseApply`` over the tables and the layer's slots.  Built only where it runs (the argument set,
    replicated columns, W > 1); refuses a replicated column whose dim the apply cannot take."""
    self.aggregate_replicated = bool(aggregate_replicated)
    self._replica = self._rep_apply = None
    if not (self.aggregate_replicated and self._rep and self._world() > 1):
      return
    from hybridbackend_amd.distribute.replicated import ReplicatedGradients   # pylint: disable=import-outside-toplevel
    from hybridbackend_amd.embedding.sparse_apply import SparseApply   # pylint: disable=import-outside-toplevel
    for c in self._rep:
      dim = self.columns[c].dimension
      if dim > 256 or (dim % 4 != 0 and dim > 64):
        raise _bad(f'{what}(..., aggregate_replicated=True): replicated column {self.columns[c].key!r}: dimension '
                   f'{dim} is beyond what the aggregated step takes (at most 256 when a multiple of 4, 64 otherwise)')
    tables = [self.weights[c] for c in self._rep]
    self._replica = ReplicatedGradients([tuple(t.shape) for t in tables], self.coll, scale=replicated_scale,
                                        device=self.device)
    self._rep_apply = SparseApply(tables, [self.accums[c] for c in self._rep] if self.accums is not None else None,
                                  **self._two_slot_kw(self._rep))

  def _rep_step(self, slices, apply_lr, optimizer, finish):
    """Stages 2 and 3 of the replicated group's aggregated step, behind the local emit-form reduce that wrote
    ``slices``: ONE allreduce of the packed dense gradients (every rank issues it here, before the sharded
    step's backward), then the optimizer step on every row any rank touched."""
    self._rep_apply(self._replica.aggregate(slices), apply_lr, optimizer, finish)

  def replica_drift(self):
    """``max(max over ranks - min over ranks)`` over every element of the replicated tables, as a device scalar:
    two packed allreduces (MAX and MIN).  A collective.  0.0 as long as the replicas agree -- forever under
    ``aggregate_replicated``, when the transport's allreduce leaves the same bits on every rank."""
    tables = [self.weights[c] for c in self._rep if self.weights[c].numel()]
    if not tables or self._world() <= 1:
      return torch.zeros((), dtype=torch.float32, device=self.device)
    hi = self.coll.allreduce_n(tables, self.coll.MAX)
    lo = self.coll.allreduce_n(tables, self.coll.MIN)
    return torch.stack([(h - l).max() for h, l in zip(hi, lo)]).max()

  # ---- hash-keyed columns: what moves with a table ------------------------------------------------------
  def _world(self):
    return self.coll.world_size if self.coll is not None else 1

  def _sharded_hash_lookup(self, combiners):
    """The sharded step of the hash group (W > 1)."""
    attr = lambda name: [getattr(self.columns[c], name) for c in self._hash]   # noqa: E731
    pick = lambda xs: [xs[c] for c in self._hash]   # noqa: E731
    # (the driver's own fill value: read only with accums, which the layer keeps only with a value of its own)
    kw = {} if self.accums is None else dict(accums=pick(self.accums),
                                             initial_accumulator_value=self._initial_accumulator_value)
    if self.hash_dtype != torch.float32:
      # 16-bit hash columns: the same forward and lifecycle, the step in the driver (fp32 slots, the layer's rounding)
      from hybridbackend_amd.embedding.sharded_hash import LowpShardedHashGroupLookup   # pylint: disable=import-outside-toplevel
      return LowpShardedHashGroupLookup(pick(self.hash_tables), self.coll, combiners=combiners, dedup=attr('dedup'),
                                        train=self.train, rounding=self._hash_rounding, seed=self._hash_seed, **kw,
                                        **self._two_slot_kw(self._hash))
    return ShardedHashGroupLookup(pick(self.hash_tables), self.coll, combiners=combiners, dedup=attr('dedup'),
                                  max_norms=attr('max_norm'), train=self.train, **kw,
                                  **self._two_slot_kw(self._hash))

  def _check_hash_dtype(self, what, rounding, seed):
    """The one dtype of the layer's hash columns (``hash_dtype``; fp32 without any) and everything a layer with
    16-bit hash columns refuses, before any table is allocated."""
    from hybridbackend_amd.embedding.lowp import check_rounding   # pylint: disable=import-outside-toplevel
    cols = [col for col in self.columns if _is_hash(col)]
    dtypes = {col.dtype for col in cols}
    if len(dtypes) > 1:
      named = ', '.join(f'{col.key!r}: {col.dtype}' for col in cols)
      raise _bad(f'{what}: the hash columns of one layer share one dtype, as one HashGroupLookup holds fp32 or '
                 f'16-bit tables ({named}): build two layers')
    self.hash_dtype = dtypes.pop() if dtypes else torch.float32
    self._hash_rounding, self._hash_seed = rounding, seed
    if self.hash_dtype == torch.float32:
      return
    check_rounding(rounding, seed, [self.hash_dtype], f'{what}(table_rounding=, table_seed=)')
    for col in cols:
      if col.max_norm is not None:
        raise _bad(f'{what}: hash column {col.key!r} is a {col.dtype} column with max_norm; the clip reads and the '
                   'clipped step writes fp32 rows')
      if getattr(col, 'weight_feature_key', None) is not None:
        raise _bad(f'{what}: hash column {col.key!r} is a {col.dtype} column with weight_feature_key '
                   f'{col.weight_feature_key!r}; per-id weights and their gradients read fp32 rows')

  def _refuse_weight_grads(self, what, weight_grads):
    if weight_grads and self._hash and self.hash_dtype != torch.float32:
      raise _bad(f'{what}.backward(weight_grads=True): the layer has {self.hash_dtype} hash columns; weight '
                 'gradients are not supported over 16-bit tables (hbk_group_lookup_bwd_weights reads fp32 rows)')

  def _hash_slot_kinds(self):
    """The layer's optimizer slots in the drivers' one order with their fill values (``sharded_hash.slot_kinds``):
    the fill value is what a row no key holds is set to -- what the slot was made with."""
    return slot_kinds(self, self._initial_accumulator_value if self.accums is not None else 0.0)

  def _hash_companions(self, c):
    """The slots of hash column c as ``(tensor, fill_value)`` pairs."""
    return slot_companions(self, self._hash_slot_kinds(), c)

  def _rebuild_hash_grad(self):
    """(W = 1) the backward object of the hash group over the lookup's current tables and the layer's slots."""
    raise NotImplementedError

  def _rehash_each(self, policy):
    """``policy(table, companions)`` -> None or the new companion tensors, on every hash table; the tensors that
    moved are stored back and the lookup objects rebuilt over them.  Returns the keys of the columns rehashed."""
    kinds = self._hash_slot_kinds()
    moved = []
    for c in self._hash:
      out = policy(self.hash_tables[c], self._hash_companions(c))
      if out is None:
        continue
      moved.append(self.columns[c].key)
      self.weights[c] = self.hash_tables[c].table
      for (name, k, _), x in zip(kinds, out):
        slots = getattr(self, name)
        if k is None:
          slots[c] = x
        else:
          pair = list(slots[c])
          pair[k] = x
          slots[c] = tuple(pair)
    if moved and self._hash_sharded is not None:
      pick = lambda xs: None if xs is None else [xs[c] for c in self._hash]   # noqa: E731
      self._hash_sharded.rebind(accums=pick(self.accums),
                                **{cls.slot_kw: pick(getattr(self, cls.slot_kw)) for cls in _opt.TWO_SLOT.values()})
    elif moved:
      self._hash_lookup.rebind()
      self._rebuild_hash_grad()
    return moved

  def set_step(self, n):
    """The step number of every expiring hash table (:meth:`HashTable.set_step`).  The layers do not advance it
    themselves: a captured graph follows the device scalar."""
    for t in self.hash_tables:
      if t is not None and t.expiring:
        t.set_step(n)

  def maybe_grow(self, max_load=0.75, factor=2.0):
    """:meth:`HashTable.maybe_grow` on every hash table, the layer's optimizer slots moving along as companions
    (rows no key holds: Adagrad's ``initial_accumulator_value``, Adam's 0, FTRL's accum its
    ``initial_accumulator_value`` and linear 0).  The new tensors are stored back into ``weights``, ``accums``,
    ``moments`` and ``ftrl_slots`` and the lookup objects rebuilt over them: afterwards ``layer.weights[c] is
    layer.hash_tables[c].table`` and the next forward and backward work as before; tensors taken from the layer
    earlier (and a captured graph) are void.  Local to the rank: no exchange, and ranks need not agree.  Returns
    the keys of the columns that were rehashed."""
    return self._rehash_each(lambda t, comp: t.maybe_grow(max_load, factor, comp))

  def maybe_evict(self, max_load=0.75, target_load=0.5, keep_freq=0, order='lru'):
    """:meth:`HashTable.maybe_evict` on every hash table -- the capacity stays, the oldest (``order='lfu'``:
    the least frequently used) keys leave -- with the companions and the bookkeeping of :meth:`maybe_grow`.
    Every hash column must be ``expiring``.  Returns the keys of the columns that were rehashed."""
    for c in self._hash:
      if not self.columns[c].expiring:
        raise _bad(f'maybe_evict: hash column {self.columns[c].key!r} is not expiring (build the column with '
                   'expiring=True)')
    return self._rehash_each(lambda t, comp: t.maybe_evict(max_load, target_load, keep_freq, comp, order=order))

  def _refuse_backward_of_a_find(self, what):
    if self._hash and not self.train:
      raise _bad(f'{what}.backward: the layer was built with train=False, its hash columns only find: there is '
                 'nothing to step')

  # ---- checkpoints (hybridbackend/tensorflow/training/saver.py:97-185) ----------------------------
  def variables(self):
    """``{name: tensor | ShardedSlice}`` of this rank: the embedding weights (TF naming:
    ``<key>_embedding/embedding_weights``; a sharded table is the slice ``part_<rank>`` of it,
    variables.py:112-141) and, when the layer keeps them, the Adagrad slots (``.../Adagrad``) or the
    Lazy Adam slots (``.../Adam`` = m, ``.../Adam_1`` = v, sharded as the weights) with the 0-d
    scalars ``beta1_power`` and ``beta2_power``, or the FTRL slots (``.../Ftrl`` = accum,
    ``.../Ftrl_1`` = linear, sharded as the weights), or the row-wise Adagrad accumulators
    (``.../RowwiseAdagrad``, ``[rows, 1]``, sharded as the weights).  Hash-keyed columns are not in it:
    they do not fit a mapping of preallocated tensors, ``save`` and ``restore`` handle them beside it."""
    from hybridbackend_amd.training.saver import ShardedSlice
    world = self.coll.world_size if self.coll is not None else 1
    rank = self.coll.rank if self.coll is not None else 0
    per_table = [('', self.weights), ('/Adagrad', self.accums)]
    extra = {}
    for cls in _opt.TWO_SLOT.values():
      pairs = getattr(self, cls.slot_kw, None)
      if pairs is not None:
        per_table += [(suffix, [cls.slot_tensors(e)[k] for e in pairs]) for k, suffix in enumerate(cls.tf_suffixes)]
        extra.update(getattr(self, cls.name).tf_variables())
    out = {}
    for c, col in enumerate(self.columns):
      if _is_hash(col):
        continue   # (the number of keys is the state: save / restore export and import them beside this dict)
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
    variables = self.variables()
    variables.update(self._hash_variables())
    return self._saver(barrier).save(prefix, variables)

  def _hash_variables(self):
    """The hash columns' state for a save: per column :meth:`HashTable.export_items` with the layer's slots as
    companions (the drivers' order: accums; m, v; accum, linear), named ``<key>_embedding/embedding_weights
    [/part_<rank>_of_<W>]/items/...``.  At W > 1 every rank writes its own part (``PerRank``)."""
    from hybridbackend_amd.training.saver import PerRank
    world = self._world()
    rank = self.coll.rank if self.coll is not None else 0
    out = {}
    for c in self._hash:
      exp = self.hash_tables[c].export_items(slots=[t for t, _ in self._hash_companions(c)])
      name = f'{self.columns[c].key}_embedding/embedding_weights'
      if world > 1:
        name += f'/part_{rank}_of_{world}'
      for k, v in exp.variables(name).items():
        out[k] = PerRank(v) if world > 1 else v
    return out

  def restore(self, prefix, barrier=None, layout='logical'):
    """Loads this rank's rows from a checkpoint written at ANY world size (``layout='reference'``:
    the reference's contiguous slicing instead, see training/saver.py).  A hash column imports, of the keys
    every rank of the saving job exported, those this rank owns (:meth:`HashTable.import_items` with ``world``
    and ``rank``: an upsert, with rows, ``last_seen`` / ``freq`` and the optimizer slots); a table too small
    for them raises ``import_items``'s error.  A column whose name the checkpoint holds as the other kind of
    variable (bucketed against hash-keyed) is refused by name."""
    if layout not in ('logical', 'reference'):
      raise ValueError("layout must be 'logical' or 'reference'")
    saver = self._saver(barrier)
    exports = self._load_hash_exports(prefix)   # (every name, kind and part set is checked before anything moves)
    for c, exp in exports:
      self.hash_tables[c].import_items(exp, self._hash_companions(c), world=saver.world_size, rank=saver.rank)
    saver.restore(prefix, self.variables(), layout=layout)

  def _load_hash_exports(self, prefix):
    """What a restore imports: ``[(column, HashExport)]`` of the hash columns the checkpoint holds, read to the
    host.  Everything that can be refused without touching a table is refused here, for ALL columns, before the
    first import: a name the checkpoint holds as the other kind of variable, parts that are not ``part_0 ..
    part_<W-1>_of_<W>`` of one W (or the one unsharded entry), an export whose companions are not the layer's
    slots.  (A table too small for its keys is found by ``import_items`` itself, which stores what fits.)"""
    import numpy as np   # pylint: disable=import-outside-toplevel
    from hybridbackend_amd.training.saver import _read_index, load_full
    names = set(_read_index(prefix)['variables'])
    found = []
    for c, col in enumerate(self.columns):
      name = f'{col.key}_embedding/embedding_weights'
      part = re.compile(re.escape(name) + r'(?:/part_(\d+)_of_(\d+))?/items/keys$')
      hits = sorted((m.group(1) is not None, int(m.group(2) or 1), int(m.group(1) or 0), n[:-len('/items/keys')])
                    for n, m in ((n, part.match(n)) for n in names) if m)
      if not _is_hash(col):
        if hits and name not in names:
          raise _bad(f'restore: {name}: the checkpoint holds the items of a hash-keyed column, the layer a '
                     'bucketed variable of this name')
        continue
      if name in names:
        raise _bad(f'restore: {name}: the checkpoint holds a bucketed variable, the layer a hash-keyed column of '
                   'this name')
      if not hits:
        continue   # (names missing from the checkpoint are left untouched)
      world = hits[0][1]
      if [(h[1], h[2]) for h in hits] != [(world, r) for r in range(world)] or len({h[0] for h in hits}) != 1:
        raise _bad(f'restore: {name}: the checkpoint does not hold the parts 0 .. W-1 of one world size (found '
                   f'{", ".join(h[3][len(name):] or "the unsharded entry" for h in hits)})')
      found.append((c, [h[3] for h in hits]))
    out = []
    for c, bases in found:
      parts = []
      for base in bases:
        d = {n: torch.from_numpy(np.array(load_full(prefix, n), copy=True))
             for n in names if n.startswith(base + '/items/')}
        rows = base + '/items/rows'
        if self.hash_tables[c].dtype == torch.bfloat16 and rows in d and d[rows].dtype == torch.int16:
          d[rows] = d[rows].view(torch.bfloat16)   # (the saver keeps bfloat16 as its bit patterns)
        parts.append(HashExport.from_variables(base, d))
      exp = HashExport.cat(parts)
      slots = self._hash_companions(c)
      if len(exp.slots) != len(slots) or exp.rows.shape[1:] != self.hash_tables[c].table.shape[1:]:
        raise _bad(f'restore: {self.columns[c].key}_embedding/embedding_weights: the checkpoint holds rows of '
                   f'{tuple(exp.rows.shape[1:])} floats with {len(exp.slots)} optimizer slot tensors, the layer '
                   f'rows of {tuple(self.hash_tables[c].table.shape[1:])} with {len(slots)}')
      out.append((c, exp))
    return out

  def restore_reference(self, prefix, names=None, barrier=None, layout='logical'):
    """Loads this rank's rows from a checkpoint the REFERENCE saved (TensorFlow tensor bundle,
    training/tf_bundle.py), written at any world size.  ``names``: ``{name here: tensor name in
    the checkpoint}`` for variables the model named differently (default: the TF names of
    ``variables()``).  layout: see ``Saver.restore_reference``."""
    self._saver(barrier).restore_reference(prefix, self.variables(), names=names, layout=layout)

  def close(self):
    if self._sharded is not None:
      self._sharded.close()
    if self._hash_sharded is not None:
      self._hash_sharded.close()


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
      when omitted).  ``'rowwise_adagrad'`` keeps one ``[rows, 1]`` accumulator per table (``row_accums``)
      for ``backward(optimizer='rowwise_adagrad')``; ``rowwise_adagrad`` is the :class:`RowwiseAdagrad` they
      step with (its defaults when omitted).
    train: False makes every hash-keyed column a pure find -- unseen ids read zero rows, ``size()`` and
      ``counts`` do not move, and ``backward`` is refused; bucketed columns ignore it.
    aggregate_replicated: True makes a stepping ``backward`` at W > 1 train the REPLICATED tables too: their
      gradients are aggregated across ranks as one packed dense allreduce (``hb.distribute.ReplicatedGradients``)
      and applied with the layer's optimizer and slots on every rank (``hb.embedding.SparseApply``), so the
      replicas stay bit-equal (``replica_drift()``).  False (the default): they are not stepped at W > 1 and the
      caller aggregates.  At W = 1 it changes nothing.  A replicated column wider than the apply takes (256
      floats, 64 when not a multiple of 4) is refused at construction.
    replicated_scale: what multiplies the summed gradients; None: ``1 / W``, the mean of the reference.
    table_dtype: None (fp32 tables: nothing below applies), ``torch.bfloat16`` or ``torch.float16``: the tables are
      stored in 16 bits -- ``init``'s result rounded to nearest -- with fp32 sums in the forward
      (``hb.embedding.LowpGroupLookup``) and fp32 accumulators and slots in the step
      (``hb.embedding.LowpLookupGrad``: the reduce's emit form, then an apply of its own).  ``weights[c]`` are the
      16-bit tensors, and ``variables()`` / ``save`` / ``restore`` carry them as they are.  One rank only (``coll``
      None or of one rank) unless ``lowp_sharded``; a hash-keyed column, a column with ``max_norm`` and a column
      wider than 64 whose block does not start on a multiple of 4 floats are refused by name;
      ``backward(weight_grads=True)`` is refused.
    lowp_sharded: True lets a layer with ``table_dtype`` span W > 1 ranks: its SHARDED tables are 16-bit shards
      looked up and stepped by ``hb.embedding.LowpShardedGroupLookup`` -- the rows cross the wire in the table's own
      16 bits, the slots are fp32, ``table_rounding`` / ``table_seed`` as above (rank k rounds with
      ``(table_seed + 0x9E3779B9 * k) mod 2^32``) -- and ``variables()`` / ``save`` / ``restore`` carry the 16-bit
      shards, resharding across world sizes as the fp32 ones do.  The REPLICATED tables stay fp32 (they hold at
      most ``max(batch, W)`` rows: capacity is not their problem) with every path they have today,
      ``aggregate_replicated`` included.  The refusals above stand.  At W = 1 the argument changes nothing.
    table_rounding: ``'nearest'``, or ``'stochastic'`` (bf16 only) -- what lets a bf16 table train on steps
      smaller than half an ulp; table_seed: the seed of its noise.

  Hash-keyed columns (:class:`HashEmbeddingColumn`) mix freely with bucketed ones; column order decides the
  block offsets.  ``hash_tables[c]`` is the column's :class:`HashTable` (None for a bucketed column) and
  ``weights[c]`` its ``table``; ``accums`` / ``moments`` / ``ftrl_slots`` of such a column are ``[capacity_local,
  dim]``.  On one rank the hash group goes through one :class:`HashGroupLookup` and one ``GroupLookupGrad``; on
  W > 1 ranks through one :class:`ShardedHashGroupLookup` (owner ``floormod(id, W)``), a step of its own beside
  the bucketed columns' -- and ``weight_feature_key`` on a hash column is then refused.  See ``set_step``,
  ``maybe_grow`` and ``maybe_evict``.  Spilling to a host tier, ``track_removals`` and delta exports are not
  driven by the layer: compose them on ``hash_tables``.

  16-bit hash columns (``HashEmbeddingColumn(dtype=torch.bfloat16 / torch.float16)``; all hash columns of a layer
  share one dtype, a mix is refused by name: two layers): the tables are ``HashTable(dtype=)``, the slots fp32, and
  ``table_rounding`` / ``table_seed`` -- without ``table_dtype``, which stays the bucketed tables' argument and still
  refuses a hash column -- are the rounding of the hash group's step.  On one rank the group goes through
  ``HashGroupLookup`` + ``LowpLookupGrad``, on W > 1 ranks through ``LowpShardedHashGroupLookup`` (``wire='table'``).
  ``set_step``, ``maybe_grow``, ``maybe_evict``, ``train=False``, ``save`` / ``restore`` (W ranks onto W') carry the
  16-bit rows through the same ``export_items`` / ``import_items`` path: nothing is cast.  Refused by name on such a
  layer: ``max_norm`` and ``weight_feature_key`` on a 16-bit hash column, ``backward(weight_grads=True)``.
  """

  def __init__(self, columns, device, coll=None, batch_size=0, init=None,
               initial_accumulator_value=None, optimizer=None, adam=None, ftrl=None, train=True,
               rowwise_adagrad=None, aggregate_replicated=False, replicated_scale=None, table_dtype=None,
               table_rounding='nearest', table_seed=0, lowp_sharded=False):
    self.table_dtype = table_dtype
    self.lowp_sharded = bool(lowp_sharded)
    if table_dtype is not None:
      self._check_lowp(columns, coll, table_dtype, table_rounding, table_seed, lowp_sharded)
    self._init_tables(columns, device, coll, batch_size, init, initial_accumulator_value, optimizer,
                      adam, ftrl, train, rowwise_adagrad, table_dtype, lowp_sharded, table_rounding, table_seed,
                      'DenseFeatures')
    self._init_replica(aggregate_replicated, replicated_scale, 'DenseFeatures')
    for c in self._hash:
      col = self.columns[c]
      if col.weight_feature_key is not None and self._world() > 1:
        raise _bad(f'hash column {col.key!r}: weight_feature_key {col.weight_feature_key!r} on a layer over '
                   f'{self._world()} ranks: the sharded step refuses weights on a column without a bucket '
                   '(weighted hash columns work on one rank)')
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
    if self._rep and table_dtype is not None and self._world() <= 1:
      # 16-bit tables: the same two roles, so that __call__ and backward do not fork
      from hybridbackend_amd.embedding.lowp import LowpGroupLookup, LowpLookupGrad   # pylint: disable=import-outside-toplevel
      self._lookup = LowpGroupLookup(pick(self._rep, self.weights),
                                     [self.columns[c].num_buckets for c in self._rep],
                                     [self.columns[c].combiner for c in self._rep])
      self._grad = LowpLookupGrad(
        self._lookup, pick(self._rep, self.accums) if self.accums is not None else None,
        rounding=table_rounding, seed=table_seed, **two_slot_kw(self._rep))
    elif self._rep:
      self._lookup = GroupLookup(pick(self._rep, self.weights),
                                 [self.columns[c].num_buckets for c in self._rep],
                                 [self.columns[c].combiner for c in self._rep],
                                 hot_rows=[self.columns[c].hot_rows for c in self._rep],
                                 max_norms=[self.columns[c].max_norm for c in self._rep])
      self._grad = GroupLookupGrad(
        self._lookup, pick(self._rep, self.accums) if self.accums is not None else None,
        **two_slot_kw(self._rep))
    if self._shd and table_dtype is not None:
      # lowp_sharded (else refused above): 16-bit shards on their own wire, fp32 slots, the step in the driver
      from hybridbackend_amd.embedding.lowp import LowpShardedGroupLookup   # pylint: disable=import-outside-toplevel
      self._sharded = LowpShardedGroupLookup(pick(self._shd, self.weights), coll,
                                             buckets=[self.columns[c].num_buckets for c in self._shd],
                                             combiners=[self.columns[c].combiner for c in self._shd],
                                             dedup=[self.columns[c].dedup for c in self._shd],
                                             accums=(pick(self._shd, self.accums)
                                                     if self.accums is not None else None),
                                             rounding=table_rounding, seed=table_seed, **two_slot_kw(self._shd))
    elif self._shd:
      self._sharded = ShardedGroupLookup(pick(self._shd, self.weights), coll,
                                         buckets=[self.columns[c].num_buckets for c in self._shd],
                                         combiners=[self.columns[c].combiner for c in self._shd],
                                         hot_rows=[self.columns[c].hot_rows for c in self._shd],
                                         dedup=[self.columns[c].dedup for c in self._shd],
                                         max_norms=[self.columns[c].max_norm for c in self._shd],
                                         accums=(pick(self._shd, self.accums)
                                                 if self.accums is not None else None),
                                         **two_slot_kw(self._shd))
    if self._hash:
      combiners = [self.columns[c].combiner for c in self._hash]
      if self._world() > 1:
        self._hash_sharded = self._sharded_hash_lookup(combiners)
      else:
        self._hash_lookup = HashGroupLookup(pick(self._hash, self.hash_tables), combiners=combiners,
                                            max_norms=[self.columns[c].max_norm for c in self._hash],
                                            train=self.train)
        self._rebuild_hash_grad()

  def _rebuild_hash_grad(self):
    accums = [self.accums[c] for c in self._hash] if self.accums is not None else None
    if self.hash_dtype != torch.float32:
      # 16-bit hash columns: HashGroupLookup put a LowpGroupLookup behind the translate; this is its step
      from hybridbackend_amd.embedding.lowp import LowpLookupGrad   # pylint: disable=import-outside-toplevel
      self._hash_grad = LowpLookupGrad(self._hash_lookup.lookup, accums, rounding=self._hash_rounding,
                                       seed=self._hash_seed, **self._two_slot_kw(self._hash))
      return
    self._hash_grad = GroupLookupGrad(self._hash_lookup.lookup, accums, **self._two_slot_kw(self._hash))

  @staticmethod
  def _check_lowp(columns, coll, table_dtype, table_rounding, table_seed, lowp_sharded=False):
    """Everything ``table_dtype`` refuses, before any table is allocated."""
    from hybridbackend_amd.embedding.lowp import check_rounding   # pylint: disable=import-outside-toplevel
    if table_dtype not in (torch.bfloat16, torch.float16):
      raise _bad(f'DenseFeatures(table_dtype=): None, torch.bfloat16 or torch.float16, got {table_dtype!r}')
    check_rounding(table_rounding, table_seed, [table_dtype], 'DenseFeatures(table_dtype=)')
    if coll is not None and coll.world_size > 1 and not lowp_sharded:
      raise _bad(f'DenseFeatures(table_dtype={table_dtype}): 16-bit tables are kept on one rank only, the layer '
                 f'spans {coll.world_size} (sharded and replicated-at-W>1 tables stay fp32)')
    off = 0
    for col in columns:
      if _is_hash(col):
        raise _bad(f'DenseFeatures(table_dtype={table_dtype}): column {col.key!r} is hash-keyed; hash tables '
                   'stay fp32')
      if col.max_norm is not None:
        raise _bad(f'DenseFeatures(table_dtype={table_dtype}): column {col.key!r} has max_norm; the clip reads '
                   'and the clipped step writes fp32 rows')
      if col.dimension > 64 and off % 4 != 0:
        raise _bad(f'DenseFeatures(table_dtype={table_dtype}): column {col.key!r} ({col.dimension} wide at float '
                   f'{off} of the block) cannot be addressed in place: a row of more than 64 elements must start '
                   'on a 16-byte boundary of the output row; reorder the columns')
      off += col.dimension

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
    if self._hash:
      # the hash columns write their blocks in place too: outs = the block's views (the translate's slot
      # buffers stay with the lookup object)
      if self._hash_lookup is not None and batch and dests is None:
        # (as for the replicated group: the blocks' addresses are arithmetic, views only when the checks need them)
        def hash_views():
          nonlocal views
          views = views or col_views()
          return pick(self._hash, views)
        self._hash_lookup.call_block(pick(self._hash, ids), pick(self._hash, splits), out,
                                     pick(self._hash, self.offsets), hash_views, sp_weights=pick_w(self._hash))
      else:
        views = views or col_views()
        look = self._hash_lookup if self._hash_lookup is not None else self._hash_sharded
        look(pick(self._hash, ids), pick(self._hash, splits), pick(self._hash, dests or views),
             sp_weights=pick_w(self._hash))
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
    this method by default never applies the step at W > 1: it returns their IndexedSlices and the caller
    applies the aggregated gradient.  A layer built with ``aggregate_replicated=True`` does both itself: behind
    the local reduce every rank issues ONE allreduce of the replicated group's packed dense gradients -- at this
    point of the method, before the sharded step's backward, so all ranks must call ``backward`` in step -- and
    then steps every row ANY rank touched with ``g = fp32(sum over ranks) * fp32(scale)`` on every rank, also
    where the sum is zero; rows nobody touched and their slots are not written.  A ``max_norm`` column
    aggregates the clipped gradients g' of the ranks' local clip passes; the aggregated step is not clipped
    again.  The return value stays this rank's LOCAL slices (``(None, None, n_unique)`` with ``emit=False``).
    ``emit=False`` (with ``apply_lr``): the stepped tables
    write no IndexedSlices (step only; their entries are ``(None, None, n_unique)``).
    ``optimizer='adam'`` (layer built with ``optimizer='adam'``): the Lazy Adam step; the beta powers
    advance once per backward that steps any table.  ``optimizer='ftrl'`` (layer built with
    ``optimizer='ftrl'``): the FTRL-Proximal step.
    ``weight_grads=True``: returns ``(slices, {weight_feature_key: tensor})`` -- the gradient of every
    weighted column's per-id weights (fp32 ``[n_ids]``; replicated and sharded tables alike, taken at the
    rows as the forward read them), an empty dict for a layer without weighted columns.
    A hash-keyed column is always stepped (it is never replicated), and the ``unique_rows`` of its
    IndexedSlices are SLOT NUMBERS of this rank's table: ``layer.hash_tables[c].keys[unique_rows]`` names the
    ids.  Refused after a forward of a layer built with ``train=False``."""
    _opt.two_slot_class(optimizer, self, "DenseFeatures(..., optimizer='{name}')")
    self._refuse_backward_of_a_find('DenseFeatures')
    self._refuse_weight_grads('DenseFeatures', weight_grads)
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
                     finish=not ((self._shd or self._hash) and apply_lr != 0.0),
                     weight_grads=want(self._rep))
      r = take(self._rep, r)
      if self._replica is not None and apply_lr != 0.0:
        # aggregate_replicated: the emit form above was stage 1; every rank issues the allreduce HERE, before
        # the sharded step's backward.  The return value stays this rank's LOCAL slices
        self._rep_step(r, apply_lr, optimizer, not ((self._shd or self._hash) and apply_lr != 0.0))
        if not emit:
          r = [(None, None, t[2]) for t in r]
      for k, c in enumerate(self._rep):
        res[c] = r[k]
    if self._shd:
      views = [grad[:, self.offsets[c]:self.offsets[c] + self.columns[c].dimension]
               for c in self._shd]
      views = [v.contiguous() if c in self._staged else v for c, v in zip(self._shd, views)]
      r = self._sharded.backward(views, apply_lr=apply_lr, optimizer=optimizer,
                                 emit=emit, finish=not (self._hash and apply_lr != 0.0),
                                 weight_grads=want(self._shd))
      r = take(self._shd, r)
      for k, c in enumerate(self._shd):
        res[c] = r[k]
    if self._hash_sharded is not None:
      views = [grad[:, self.offsets[c]:self.offsets[c] + self.columns[c].dimension]
               for c in self._hash]
      views = [v.contiguous() if c in self._staged else v for c, v in zip(self._hash, views)]
      r = self._hash_sharded.backward(views, apply_lr=apply_lr, optimizer=optimizer, emit=emit)
      for k, c in enumerate(self._hash):
        res[c] = r[k]
    elif self._hash:
      # the last forward's slot numbers are the ids of the backward: the tables are stepped at W = 1 only here
      grads, grad_block = None, (grad, pick(self._hash, self.offsets))
      if any(c in self._staged for c in self._hash):
        views = col_grads()
        grads = [views[c].contiguous() for c in self._hash]
        grad_block = None
      r = self._hash_grad(self._hash_lookup.slots, grads, pick(self._hash, splits), apply_lr=apply_lr,
                          optimizer=optimizer, emit=emit, grad_block=grad_block,
                          sp_weights=None if ws is None else pick(self._hash, ws),
                          weight_grads=want(self._hash))
      r = take(self._hash, r)
      for k, c in enumerate(self._hash):
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
  ``dedup`` are EmbeddingColumn's.  A column whose table is sharded needs a ``pad_id`` or
  ``SequenceFeatures(..., sharded_zero_padding=True)``."""

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
  ``pad_id`` -- unless the layer is built with ``sharded_zero_padding=True``: a sharded column without a ``pad_id``
  (bucketed or hash-keyed) then goes through the PACKED form (``sequence_pack``): the step is handed the first
  ``min(len, max_len)`` ids of every sample and ``batch * max_len`` segments holding one id or none, in the same
  step as the group's columns with a pad id.  Padding is in no id list: zero rows that cross no wire, reach no
  gradient row and keep no key fresh (TF's ``SequenceFeatures``), at the price of ONE more host read per forward
  and group (the packed totals) -- which is why the argument is opt-in.

  Hash-keyed columns (:class:`HashSequenceEmbeddingColumn`) mix freely with bucketed ones.  On one rank they go
  through ``HashSequenceLookup`` / ``SequenceLookupGrad``; on W > 1 ranks through ``ShardedHashGroupLookup``
  with combiner ``'sum'`` over the RAW-id grid ``sequence_id_grid`` builds (``batch * max_len`` ids of one sample
  each): ids past ``max_len`` are not in the grid, so they are not inserted, counted or kept fresh on any rank,
  and a pad id is required there too unless ``sharded_zero_padding`` is set (the packed ids are raw too).
  ``train``, ``hash_tables``, ``set_step``, ``maybe_grow`` and ``maybe_evict`` are :class:`DenseFeatures`'.

  16-bit hash columns (``HashSequenceEmbeddingColumn(dtype=)``, one dtype per layer): on one rank
  ``HashSequenceLookup`` + ``LowpSequenceLookupGrad``, on W > 1 ranks ``LowpShardedHashGroupLookup`` over the id grid
  or, with ``sharded_zero_padding``, the packed form; ``table_rounding`` / ``table_seed`` are the rounding of their
  step, and ``max_norm`` on such a column is refused by name."""

  def __init__(self, columns, device, coll=None, batch_size=0, init=None,
               initial_accumulator_value=None, optimizer=None, adam=None, ftrl=None, train=True,
               rowwise_adagrad=None, sharded_zero_padding=False, aggregate_replicated=False,
               replicated_scale=None, table_rounding='nearest', table_seed=0):
    from hybridbackend_amd.embedding.hash_sequence import HashSequenceLookup
    from hybridbackend_amd.embedding.sequence import SequenceLookup, SequenceLookupGrad
    self._init_tables(columns, device, coll, batch_size, init, initial_accumulator_value, optimizer,
                      adam, ftrl, train, rowwise_adagrad, table_rounding=table_rounding, table_seed=table_seed,
                      what='SequenceFeatures')
    self._init_replica(aggregate_replicated, replicated_scale, 'SequenceFeatures')
    self.sharded_zero_padding = bool(sharded_zero_padding)
    for c in self._hash:
      col = self.columns[c]
      if col.pad_id is None and self._world() > 1 and not self.sharded_zero_padding:
        raise _bad(f'hash sequence column {col.key!r}: its table is sharded over {self._world()} ranks, and a '
                   'sharded sequence column requires a pad_id (the sharded step takes one raw id per position, '
                   'and among raw ids no value means "nothing": every int64 is a key; zero padding is for one '
                   'rank).  SequenceFeatures(..., sharded_zero_padding=True) looks such a column up zero padded, '
                   'through the packed form, at the price of one more host read per forward')
    for c in self._shd:
      col = self.columns[c]
      if col.pad_id is None and not self.sharded_zero_padding:
        raise _lib.InvalidArgumentError(
          _lib.INVALID_ARGUMENT,
          f'sequence column {col.key!r}: its table is sharded over {coll.world_size} ranks, and a sharded '
          'sequence column requires a pad_id (the sharded step bucketizes the id grid again, which would '
          'turn the -1 of a zero-padded position into a row; zero padding is for replicated tables).  '
          'SequenceFeatures(..., sharded_zero_padding=True) looks such a column up zero padded, through the '
          'packed form, at the price of one more host read per forward')
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
    if self._hash and self._world() > 1:
      self._hash_sharded = self._sharded_hash_lookup('sum')
    elif self._hash:
      self._hash_lookup = HashSequenceLookup(pick(self._hash, self.hash_tables), attr(self._hash, 'max_len'),
                                             pad_ids=attr(self._hash, 'pad_id'),
                                             max_norms=attr(self._hash, 'max_norm'), train=self.train)
      self._rebuild_hash_grad()

  def _rebuild_hash_grad(self):
    from hybridbackend_amd.embedding.sequence import SequenceLookupGrad
    accums = [self.accums[c] for c in self._hash] if self.accums is not None else None
    if self.hash_dtype != torch.float32:
      from hybridbackend_amd.embedding.hash_sequence import LowpSequenceLookupGrad   # pylint: disable=import-outside-toplevel
      self._hash_grad = LowpSequenceLookupGrad(self._hash_lookup, accums, rounding=self._hash_rounding,
                                               seed=self._hash_seed, **self._two_slot_kw(self._hash))
      return
    self._hash_grad = SequenceLookupGrad(self._hash_lookup, accums, **self._two_slot_kw(self._hash))

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
      def row_grid(idx):
        cols = pick(idx, self.columns)
        return sequence_row_grid(pick(idx, ids), pick(idx, splits), [col.num_buckets for col in cols],
                                 [col.max_len for col in cols], [col.pad_id for col in cols])
      self._sharded_step(self._sharded, self._shd, ids, splits, row_grid, batch or 0, outs, lengths)
    if self._hash_sharded is not None:
      # the RAW-id grid: B * T ids of one sample each, the pad id past a sample's length; ids past T are not in
      # it, so they reach no owner
      def id_grid(idx):
        from hybridbackend_amd.embedding.sequence import sequence_id_grid
        cols = pick(idx, self.columns)
        return sequence_id_grid(pick(idx, ids), pick(idx, splits), [col.max_len for col in cols],
                                [col.pad_id for col in cols])
      self._sharded_step(self._hash_sharded, self._hash, ids, splits, id_grid, batch or 0, outs, lengths)
    elif self._hash:
      o, ln = self._hash_lookup(pick(self._hash, ids), pick(self._hash, splits))
      for k, c in enumerate(self._hash):
        outs[c], lengths[c] = o[k], ln[k]
    return outs, lengths

  def _sharded_step(self, driver, group, ids, splits, grid_of, batch, outs, lengths):
    """One step of a sharded driver over the columns ``group``: those with a pad id as ``batch * max_len`` ids of
    one sample each (``grid_of(columns)``: their grids and lengths), the zero-padded ones
    (``sharded_zero_padding``) in the packed form -- the first ``min(len, max_len)`` ids of every sample and
    ``batch * max_len`` segments of one id or none (``sequence_pack``: one call for the group, one host read).
    The step keeps the row splits, so the backward needs nothing else."""
    from hybridbackend_amd.embedding.sequence import sequence_pack
    packed = [c for c in group if self.columns[c].pad_id is None]
    gridded = [c for c in group if self.columns[c].pad_id is not None]
    step_ids, step_splits = {}, {}
    if gridded:
      grids, ln = grid_of(gridded)
      for k, c in enumerate(gridded):
        step_ids[c], step_splits[c], lengths[c] = grids[k], None, ln[k]
    if packed:
      p_ids, p_pos, ln, _ = sequence_pack([ids[c] for c in packed], [splits[c] for c in packed],
                                          [self.columns[c].max_len for c in packed])
      for k, c in enumerate(packed):
        step_ids[c], step_splits[c], lengths[c] = p_ids[k], p_pos[k], ln[k]
    o = driver([step_ids[c] for c in group], [step_splits[c] for c in group] if packed else None)
    for k, c in enumerate(group):
      outs[c] = o[k].view(batch, self.columns[c].max_len, self.columns[c].dimension)

  def backward(self, grads, apply_lr=0.0, optimizer='sgd', emit=True):
    """grads[c]: the gradient of the last forward's ``outputs[c]``.  Returns per column the
    ``IndexedSlices`` ``(unique_rows, grad_rows, n_unique)`` of this rank's rows, as
    ``DenseFeatures.backward`` does and with its rule for the step: the sharded tables are stepped in the
    same pass, replicated tables are by default stepped only at W = 1 (at W > 1 their gradients must be
    aggregated across ranks first; their IndexedSlices are returned) -- a layer built with
    ``aggregate_replicated=True`` aggregates and steps them itself, exactly as ``DenseFeatures.backward``
    describes (one allreduce, issued before the sharded step's backward).  A hash-keyed column is always stepped, and its
    ``unique_rows`` are slot numbers of this rank's table (``layer.hash_tables[c].keys[unique_rows]`` names the
    ids).  Refused after a forward of a layer built with ``train=False``."""
    _opt.two_slot_class(optimizer, self, "SequenceFeatures(..., optimizer='{name}')")
    self._refuse_backward_of_a_find('SequenceFeatures')
    if len(grads) != len(self.columns):
      raise _lib.InvalidArgumentError(
        _lib.INVALID_ARGUMENT, f'expected {len(self.columns)} gradients, got {len(grads)}')
    res = [None] * len(self.columns)
    if self._rep:
      rep_lr = apply_lr if (self.coll.world_size if self.coll is not None else 1) <= 1 else 0.0
      # one optimizer step: the powers advance with the last call that steps (the sharded one)
      r = self._grad([grads[c] for c in self._rep], apply_lr=rep_lr, optimizer=optimizer,
                     emit=emit or rep_lr == 0.0,
                     finish=not ((self._shd or self._hash) and apply_lr != 0.0))
      if self._replica is not None and apply_lr != 0.0:
        # aggregate_replicated, as in DenseFeatures.backward: the allreduce is issued here, before the sharded step
        self._rep_step(r, apply_lr, optimizer, not ((self._shd or self._hash) and apply_lr != 0.0))
        if not emit:
          r = [(None, None, t[2]) for t in r]
      for k, c in enumerate(self._rep):
        res[c] = r[k]
    flat = lambda c: grads[c].contiguous().view(   # noqa: E731
      grads[c].shape[0] * self.columns[c].max_len, self.columns[c].dimension)
    if self._shd:
      r = self._sharded.backward([flat(c) for c in self._shd], apply_lr=apply_lr, optimizer=optimizer, emit=emit,
                                 finish=not (self._hash and apply_lr != 0.0))
      for k, c in enumerate(self._shd):
        res[c] = r[k]
    if self._hash_sharded is not None:
      r = self._hash_sharded.backward([flat(c) for c in self._hash], apply_lr=apply_lr, optimizer=optimizer,
                                      emit=emit)
    elif self._hash:
      r = self._hash_grad([grads[c] for c in self._hash], apply_lr=apply_lr, optimizer=optimizer, emit=emit)
    for k, c in enumerate(self._hash):
      res[c] = r[k]
    return res


class DeduplicatedFeatures:
  """Key-deduplicated features: the layer side of the reference's ``hb.data.deduplicate(key_idx_field_names,
  value_field_names)`` (data/dataframe.py:301-392).  Features that are the same for many samples of a batch (the
  user side of a click log) arrive once per distinct key -- ``U`` segments for ``B`` samples -- beside a restore
  index per sample.  The reference restores the IDS to batch length before the lookup; this layer looks the ``U``
  segments up once and expands the pooled ROWS to the batch on the device (``hb.embedding.expand_rows``), and its
  backward reduces the batch gradient to ``U`` rows (``expand_rows_grad``: per key the fp32 sum of its samples'
  rows in ascending sample order, bit-identical from run to run) before the inner layer's backward runs on them.
  Lookup, reduce plan, optimizer step, sharded step and hash table underneath see ``U`` segments and are untouched.

  Args:
    plain: a :class:`DenseFeatures` over the per-sample columns, or None.
    groups: an ordered dict ``{key_idx_feature_name: DenseFeatures | SequenceFeatures}``: per key field the layer
      over its value columns.  Every inner layer is built as usual -- its own tables, optimizer slots and ``coll``
      -- and is reachable as ``layer.layers`` (plain first, then the groups in order); checkpoints, ``set_step``,
      ``maybe_grow`` and ``maybe_evict`` are the inner layers' own.
    train: False builds no inverse index in the forward (inference needs none); ``backward`` is then refused.

  Forward: ``features[key_idx_name]`` is the int32/int64 ``[B]`` restore index of a group, GLOBAL row numbers into
  the group's ``U`` segments (a reader that yields the reference's per-row-group local indices adds the offsets
  itself); the group's columns carry ``U`` segments, the plain columns ``B``.  Returns ``(block, sequences)``:
  ``block`` is ``[B, sum of widths]`` -- the plain block first, then the :class:`DenseFeatures` groups in order,
  adjacent, the row pitch padded to 4 floats as in :class:`DenseFeatures` (None without such layers) -- and
  ``sequences[key_idx_name] = (outputs, lengths)`` of every :class:`SequenceFeatures` group, ``[B, T, dim]`` rows
  and int32 ``[B]`` lengths per column, expanded by the same launch as rows of ``T * dim`` and of 1 element.  A
  restore index outside ``[0, U)`` reads zero rows (and a length of 0) and sends no gradient.  The plain block is
  placed by the identity form of the expand launch (``idx=None``); :class:`DenseFeatures` itself is unchanged.

  ``indexes[key_idx_name]``: the :class:`~hybridbackend_amd.embedding.ExpandIndex` the last forward built
  (``train``); its ``invalid_count()`` is the only host read."""

  def __init__(self, plain, groups, train=True):
    from hybridbackend_amd.embedding.expand import ExpandIndex, expand_rows, expand_rows_grad
    self._index_cls, self._expand, self._expand_grad = ExpandIndex, expand_rows, expand_rows_grad
    if plain is not None and not isinstance(plain, DenseFeatures):
      raise _bad('DeduplicatedFeatures: plain must be a DenseFeatures or None')
    self.plain = plain
    self.groups = dict(groups)
    for name, layer in self.groups.items():
      if not isinstance(layer, (DenseFeatures, SequenceFeatures)):
        raise _bad(f'DeduplicatedFeatures: group {name!r} must be a DenseFeatures or a SequenceFeatures')
    if plain is None and not self.groups:
      raise _bad('DeduplicatedFeatures: no layer at all')
    self.layers = ([plain] if plain is not None else []) + list(self.groups.values())
    self.columns = [col for layer in self.layers for col in layer.columns]
    self.device = self.layers[0].device
    self.train = bool(train)
    # the block: plain first, then the DenseFeatures groups in order, adjacent
    self.offsets, off = {}, plain.width if plain is not None else 0
    for name, layer in self.groups.items():
      if isinstance(layer, DenseFeatures):
        self.offsets[name] = off
        off += layer.width
    self.width = off
    self.indexes = {}

  def __call__(self, features):
    idxs = {name: features[name] for name in self.groups}
    batch = None
    for name, idx in idxs.items():
      if idx.dim() != 1 or (batch is not None and idx.numel() != batch):
        raise _bad(f'feature {name}: the restore index must be a vector of one row number per sample'
                   + ('' if batch is None else f' ({batch} samples)'))
      batch = idx.numel()
    block = None
    plain_block = self.plain(features) if self.plain is not None else None
    if plain_block is not None:
      if batch is not None and plain_block.shape[0] != batch:
        raise _bad(f'the plain columns hold {plain_block.shape[0]} samples, the restore indexes {batch}')
      batch = plain_block.shape[0]
    if self.width:
      pitch = (self.width + 3) // 4 * 4
      block = torch.empty((batch, pitch), dtype=torch.float32, device=self.device)[:, :self.width]
    if plain_block is not None:
      self._expand(None, [plain_block], [block[:, :self.plain.width]])
    sequences = {}
    self.indexes = {}
    for name, layer in self.groups.items():
      if isinstance(layer, DenseFeatures):
        rows = layer(features)
        n_keys, srcs = rows.shape[0], [rows]
        outs = [block[:, self.offsets[name]:self.offsets[name] + layer.width]]
      else:
        o, lengths = layer(features)
        n_keys, srcs, outs = lengths[0].numel(), list(o) + list(lengths), None
      if self.train:
        self.indexes[name] = self._index_cls(idxs[name], n_keys).build()
      outs = self._expand(idxs[name], srcs, outs, n_keys=n_keys)
      if not isinstance(layer, DenseFeatures):
        k = len(layer.columns)
        sequences[name] = (outs[:k], outs[k:])
    return block, sequences

  def backward(self, grad, seq_grads=None, **kw):
    """grad: the gradient of the last forward's block, fp32 ``[B, width]`` (None without one); ``seq_grads``:
    ``{key_idx_name: [gradient of outputs[c], ...]}`` for the :class:`SequenceFeatures` groups.  Every group's
    gradient is reduced to its ``U`` rows and handed to the inner layer's ``backward`` with the keywords
    (``apply_lr``, ``optimizer``, ``emit``; ``weight_grads`` for the :class:`DenseFeatures` layers) unchanged; the
    plain layer gets its block as the strided view it is.  Returns the inner layers' IndexedSlices as one list in
    ``layer.columns`` order -- with ``weight_grads=True`` ``(slices, {weight_feature_key: tensor})``, a group's
    weight gradients being those of its ``U`` segments' ids.  All ranks call the inner layers in the same order."""
    if not self.train:
      raise _bad('DeduplicatedFeatures.backward: the layer was built with train=False, its forward builds no index')
    for name in self.groups:
      if name not in self.indexes:
        raise _bad(f'DeduplicatedFeatures.backward: group {name!r} has no index: run the forward first')
    if self.width:
      if grad is None or grad.dim() != 2 or grad.shape[1] != self.width or grad.dtype != torch.float32:
        raise _bad(f'grad must be fp32 [batch, {self.width}]')
      if grad.stride(1) != 1:
        grad = grad.contiguous()
    seq_grads = seq_grads or {}
    want_w = bool(kw.get('weight_grads', False))
    seq_kw = {k: v for k, v in kw.items() if k != 'weight_grads'}
    res, wgrads = [], {}

    def take(r):
      if want_w:
        wgrads.update(r[1])
        r = r[0]
      res.extend(r)
    if self.plain is not None:
      take(self.plain.backward(grad[:, :self.plain.width], **kw))
    for name, layer in self.groups.items():
      index = self.indexes[name]
      if isinstance(layer, DenseFeatures):
        pitch = (layer.width + 3) // 4 * 4
        g_keys = torch.empty((index.n_keys, pitch), dtype=torch.float32, device=self.device)[:, :layer.width]
        off = self.offsets[name]
        self._expand_grad(index, [grad[:, off:off + layer.width]], [g_keys])
        take(layer.backward(g_keys, **kw))
      else:
        gs = seq_grads.get(name)
        if gs is None or len(gs) != len(layer.columns):
          raise _bad(f'seq_grads[{name!r}] must hold {len(layer.columns)} gradients, one per column of the group')
        res.extend(layer.backward(self._expand_grad(index, [g.contiguous() for g in gs]), **seq_kw))
    if want_w:
      return res, wgrads
    return res

  def close(self):
    for layer in self.layers:
      layer.close()
