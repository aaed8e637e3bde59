"""Low-precision embedding tables: rows stored as ``torch.bfloat16`` / ``torch.float16``, every sum and every
optimizer slot fp32 (include/hbk.h, "Low-precision tables").

Four classes with the calling conventions of their fp32 counterparts:

  :class:`LowpGroupLookup`   the forward (``hbk_lowp_lookup_fwd``): gathers 2-byte rows, upcasts them exactly and
                             combines in fp32 -- bit for bit ``GroupLookup`` over ``table.float()``.
  :class:`LowpSparseApply`   the optimizer step on IndexedSlices (``hbk_lowp_apply_slices_n``): upcast a row, step
                             it with the arithmetic of ``SparseApply``, round it back -- to nearest even, or
                             stochastically (bf16), without which a bf16 table does not train: an SGD step below
                             half an ulp (2^-8 relative) is rounded away every time.
  :class:`LowpLookupGrad`    the backward and the step: an unmodified ``GroupLookupGrad`` in its emit form (which
                             never reads the table), then ``LowpSparseApply`` on the slices it returned.
  :class:`LowpShardedGroupLookup`  the sharded step over 16-bit shards: rows cross the wire in the table's own 16
                             bits (or upcast by the owner), the plan's emit backward, ``LowpSparseApply`` on the shards.
"""
import ctypes as C
import numbers

import numpy as np
import torch

from hybridbackend_amd import _lib
from hybridbackend_amd.embedding import optimizer as _opt
from hybridbackend_amd.embedding.lookup import GroupLookup, GroupLookupGrad, _combiner_code
from hybridbackend_amd.embedding.sharded import ShardedGroupLookup
from hybridbackend_amd.embedding.sparse_apply import SparseApply

_DTYPES = {torch.bfloat16: _lib.LOWP_BF16, torch.float16: _lib.LOWP_FP16}
_ROUNDING = {'nearest': _lib.LOWP_ROUND_NEAREST, 'stochastic': _lib.LOWP_ROUND_STOCHASTIC}


def _bad(msg):
  return _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, msg)


def _require_lowp_tables(tables, what):
  """``tables`` as a list of bf16 / fp16 ``[rows, dim]`` device tensors (the dtype is looked at first: an fp32
  table is refused by name wherever it lives)."""
  tables = list(tables)
  for c, t in enumerate(tables):
    if not isinstance(t, torch.Tensor) or t.dtype not in _DTYPES or t.dim() != 2:
      raise _bad(f'{what}: table {c} must be a torch.bfloat16 or torch.float16 [rows, dim] tensor, got '
                 f'{getattr(t, "dtype", type(t).__name__)} (fp32 tables go through GroupLookup / SparseApply)')
    _lib.require_device_tensor(t, 'embedding weights')
  return tables


def check_rounding(rounding, seed, dtypes, what):
  """The rounding mode's code and the seed as a uint32; 'stochastic' is defined for bf16 tables only."""
  if rounding not in _ROUNDING:
    raise _bad(f"{what}: rounding must be 'nearest' or 'stochastic', got {rounding!r}")
  if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= int(seed) < 2 ** 32:
    raise _bad(f'{what}: seed must be an integer in [0, 2^32), got {seed!r}')
  if rounding == 'stochastic' and any(d != torch.bfloat16 for d in dtypes):
    raise _bad(f"{what}: rounding='stochastic' is defined for torch.bfloat16 tables only")
  return _ROUNDING[rounding], int(seed)


class LowpGroupLookup(GroupLookup):
  """A group of N embedding columns over 16-bit tables, looked up with one launch per 64 columns and kind.

  Args:
    tables: list of ``torch.bfloat16`` / ``torch.float16`` ``[rows, dim]`` device tensors (a call may mix them).
    buckets, combiners, divisor: as :class:`GroupLookup`.
    chunk_elems: None (the default lane width: 8 from dim 64 on, else 4), 4 or 8: elements a lane moves where the
      column allows it (8: ``dim % 8 == 0`` and a 16-byte aligned table).  A pure speed choice: the result does not
      depend on it.
    wide_rows: False -- a table whose rows cannot move 4 elements per lane (``dim % 4 != 0``, or an unaligned table or
      output) is served up to dim 64, as ever.  True -- up to dim 256: the launch takes such a row in column blocks of
      64 elements.  The forward only: the 16-bit apply keeps its bound.

  The calling convention is :class:`GroupLookup`'s -- ``bind``, ``__call__(ids, row_splits=None, outs=None,
  sp_weights=None)``, ``launch()``, outputs as column blocks of a wider tensor -- and the result is, bit for bit,
  ``GroupLookup`` over ``[t.float() for t in tables]`` with the same arguments.  ``max_norms`` and ``hot_rows`` do
  not exist here: a clip is refused, and the attributes a ``GroupLookupGrad`` reads of its lookup say "none"."""

  def __init__(self, tables, buckets=None, combiners='sum', divisor=1, max_norms=None,   # pylint: disable=super-init-not-called
               chunk_elems=None, wide_rows=False):
    if max_norms is not None and not (isinstance(max_norms, (list, tuple)) and all(x is None for x in max_norms)):
      raise _bad('LowpGroupLookup: max_norms is not supported for 16-bit tables (the clip reads and the clipped '
                 'step writes fp32 rows)')
    if chunk_elems not in (None, 4, 8):
      raise _bad(f'LowpGroupLookup: chunk_elems must be None, 4 or 8, got {chunk_elems!r}')
    self.tables = _require_lowp_tables(tables, 'LowpGroupLookup')
    self._lib = _lib.lib()
    n = len(self.tables)
    if buckets is None:
      buckets = [0] * n
    if isinstance(combiners, (str, int)) or combiners is None:
      combiners = [combiners] * n
    self.buckets = [int(b or 0) for b in buckets]
    self.combiners = [_combiner_code(c) for c in combiners]
    self.divisor = int(divisor)
    # what GroupLookupGrad reads of its lookup: no clip, no hot-row bookkeeping
    self.max_norms = [0.0] * n
    self.max_norms_c = None
    self._auto_hot = []
    self._auto_state = None
    self._cols = (_lib.LowpLookupColumn * n)()
    self._cols_np = np.frombuffer(self._cols, dtype=np.dtype(_lib.LowpLookupColumn)) if n else None
    self._dims = [int(t.shape[1]) for t in self.tables]
    for c, t in enumerate(self.tables):
      col = self._cols[c]
      col.table = t.data_ptr()
      col.table_dtype = _DTYPES[t.dtype]
      col.rows = t.shape[0]
      col.dim = t.shape[1]
      col.bucket = self.buckets[c]
      col.divisor = self.divisor
      col.combiner = self.combiners[c]
      col.chunk_elems = chunk_elems or 0
      col.wide_rows = 1 if wide_rows else 0

  def launch(self, stream=None):
    """Enqueue the bound lookup on `stream` (a torch stream; default: current)."""
    if stream is None:
      s = _lib.current_stream(self.tables[0].device if self.tables else None)
    else:
      s = C.c_void_p(stream.cuda_stream)
    _lib.check(self._lib.hbk_lowp_lookup_fwd(len(self.tables), self._cols, s))


class LowpSparseApply(SparseApply):
  """The sparse optimizer step of N 16-bit tables from caller-held IndexedSlices, one launch per 64 tables.

  Args:
    tables: list of ``torch.bfloat16`` / ``torch.float16`` ``[rows, dim]`` device tensors, stepped in place.
    accums / moments, adam / ftrl_slots, ftrl / row_accums, rowwise_adagrad: the optimizer slots and objects, as
      :class:`SparseApply` takes them.  Slots are FP32 and have the table's SHAPE (row-wise Adagrad: ``[rows, 1]``).
    rounding: ``'nearest'`` (ties to even; bf16: the bits of torch's ``float32 -> bfloat16`` cast) or
      ``'stochastic'`` (bf16 only): ``(u + 16 bits of noise) >> 16`` on the fp32 pattern, unbiased, with noise that
      is a pure function of ``(seed, step counter, column, row, element)`` (include/hbk.h).
    seed: the noise's seed, an integer in [0, 2^32).

  A stepped row is ``round(rule(upcast(row), slots, g))`` with the formulas, rounding and operation order of
  :class:`SparseApply`; with ``'nearest'`` table and slots equal ``SparseApply`` on ``table.float()``, cast, bit for
  bit.  The object owns the device step counter (``step_counter``, one int32 word read as uint32): a call with
  ``finish=True`` advances it once, behind the apply in stream order, so replays of a captured graph draw fresh
  noise; ``'nearest'`` never touches it.  ``__call__``, ``bind`` and ``launch`` are :class:`SparseApply`'s: the
  slices are those it takes, ``finish=True`` also advances the step counter, and ``launch()`` steps again on the
  bound slices (after a bare ``bind`` it needs ``lr``, ``optimizer`` and ``finish``)."""

  _NAME = 'LowpSparseApply'
  _NEEDS = 'LowpSparseApply(tables, {slots})'
  _COLUMN = _lib.LowpSlicesColumn

  def __init__(self, tables, accums=None, moments=None, adam=None, ftrl_slots=None, ftrl=None, row_accums=None,
               rowwise_adagrad=None, rounding='nearest', seed=0):
    self.rounding, self.seed = rounding, seed   # (checked with the tables, before anything is bound)
    super().__init__(tables, accums=accums, moments=moments, adam=adam, ftrl_slots=ftrl_slots, ftrl=ftrl,
                     row_accums=row_accums, rowwise_adagrad=rowwise_adagrad)
    dev = self.tables[0].device if self.tables else torch.device('cuda', torch.cuda.current_device())
    self.step_counter = torch.zeros(1, dtype=torch.int32, device=dev)
    # the hbk_lowp_rounding_t of a call with / without the advance (kept alive by this object)
    self._rounding_c = {f: _lib.LowpRounding(self._mode, self.seed, self.step_counter.data_ptr(), 1 if f else 0, 0)
                        for f in (False, True)}
    self._slices_key = None

  def _require_tables(self, tables):
    tables = _require_lowp_tables(tables, 'LowpSparseApply')
    self._mode, self.seed = check_rounding(self.rounding, self.seed, [t.dtype for t in tables], 'LowpSparseApply')
    return tables

  def _fill_table(self, col, table):
    col.table_dtype = _DTYPES[table.dtype]

  def _foreign_call(self, apply, s0, s1, params, lr, finish, stream):
    return self._lib.hbk_lowp_apply_slices_n(len(self.tables), self._cols, apply, s0, s1, params, lr,
                                             C.byref(self._rounding_c[finish]), stream)

  def _launchable(self, explicit):
    return self._slices_key is not None and (self._bound is not None or explicit)

  def bind(self, slices):
    """Point the descriptors at ``slices`` (checked) without stepping; the same tensors at the same addresses as
    the last time are not looked at again."""
    slices = list(slices)
    key = tuple(id(x) for s in slices for x in s) if len(slices) == len(self.tables) else None
    if key is not None and key == self._slices_key and all(
        x.data_ptr() == q for s, qs in zip(slices, self._slices_ptrs) for x, q in zip(s, qs)):
      return
    super().bind(slices)
    self._slices_key = key
    self._slices_ptrs = [tuple(x.data_ptr() for x in s) for s in self._keep]


class LowpLookupGrad:
  """Backward and optimizer step of a :class:`LowpGroupLookup`, with :class:`GroupLookupGrad`'s calling convention.

  Internally an UNMODIFIED ``GroupLookupGrad`` over the lookup, always called with ``apply_lr=0.0, emit=True`` --
  the reduce's emit form never reads the table, so every plan, ``deterministic=True`` and weighted columns work
  unchanged on a table of any element type -- and then a :class:`LowpSparseApply` on the slices it returned.  The
  split costs a launch and a round trip of ``grad_rows`` through memory that the fused fp32 step does not pay.

  Never give a bare ``GroupLookupGrad`` a lookup over 16-bit tables and a non-zero ``apply_lr``: its fused step
  (and the slot optimizers' apply) reads and writes ``table`` as fp32 rows of ``4 * dim`` bytes -- on a 16-bit
  table that corrupts two rows per step and runs past the end of the allocation.  This class is the way to step
  one, and it cannot reach the fused step: the inner object holds no slots and is only ever asked to emit.

  Args:
    lookup: the :class:`LowpGroupLookup`.
    accums / moments, adam / ftrl_slots, ftrl / row_accums, rowwise_adagrad: FP32 slots of the table's shape.
    deterministic: as :class:`GroupLookupGrad`.
    rounding, seed: as :class:`LowpSparseApply`."""

  def __init__(self, lookup, accums=None, moments=None, adam=None, ftrl_slots=None, ftrl=None, row_accums=None,
               rowwise_adagrad=None, deterministic=False, rounding='nearest', seed=0):
    if not isinstance(lookup, LowpGroupLookup):
      raise _bad('LowpLookupGrad needs a LowpGroupLookup (fp32 tables go through GroupLookupGrad)')
    self.lookup = lookup
    self._apply = LowpSparseApply(lookup.tables, accums=accums, moments=moments, adam=adam, ftrl_slots=ftrl_slots,
                                  ftrl=ftrl, row_accums=row_accums, rowwise_adagrad=rowwise_adagrad,
                                  rounding=rounding, seed=seed)
    # no slots, no accumulators: this object can only emit
    self._reduce = GroupLookupGrad(lookup, deterministic=deterministic)
    self._last_emit = True

  @property
  def step_counter(self):
    return self._apply.step_counter

  @property
  def accums(self):
    return self._apply.accums

  def __getattr__(self, name):
    # the slot lists and optimizer objects (moments / adam / ...) live with the apply
    if name in ('_apply', '_reduce'):
      raise AttributeError(name)
    for cls in _opt.TWO_SLOT.values():
      if name in (cls.name, cls.slot_kw):
        return getattr(self._apply, name)
    raise AttributeError(name)

  @staticmethod
  def _refuse_weight_grads(weight_grads):
    if weight_grads is not False and weight_grads is not None:
      raise _bad('LowpLookupGrad: weight_grads is not supported for 16-bit tables (hbk_group_lookup_bwd_weights '
                 'reads fp32 rows)')

  def __call__(self, ids, grads, row_splits=None, apply_lr=0.0, optimizer='sgd', emit=True, grad_block=None,
               sp_weights=None, finish=True, weight_grads=False):
    """As :meth:`GroupLookupGrad.__call__`; returns per column ``(unique_rows, grad_rows, n_unique)``, equal to the
    fp32 object's.  ``emit=False`` (with ``apply_lr``) is accepted: the slices are written all the same (the step
    reads them) and the returned triples are ``(None, None, n_unique)``.  ``weight_grads`` is refused."""
    self._refuse_weight_grads(weight_grads)
    if not emit and apply_lr == 0.0:
      raise _bad('emit=False needs apply_lr != 0')
    if apply_lr != 0.0:
      self._apply._check(apply_lr, optimizer)   # (before the reduce: a refused call writes nothing)
    else:
      _opt.two_slot_class(optimizer)
    r = self._reduce(ids, grads, row_splits, apply_lr=0.0, optimizer='sgd', emit=True, grad_block=grad_block,
                     sp_weights=sp_weights)
    if apply_lr != 0.0:
      self._apply(r, apply_lr, optimizer, finish)
    else:
      self._apply.bind(r)   # (a later launch() may step)
    self._last_emit = bool(emit)
    return r if emit else [(None, None, t[2]) for t in r]

  def launch(self, apply_lr=0.0, optimizer='sgd', finish=True):
    """The backward of the LAST call again on the same tensors, then the step when ``apply_lr`` != 0: two foreign
    calls.  Same emit mode as that call; returns the same result views."""
    if not self._last_emit and apply_lr == 0.0:
      raise _bad('emit=False needs apply_lr != 0')
    if apply_lr != 0.0:
      self._apply._check(apply_lr, optimizer)
    r = self._reduce.launch(0.0)
    if apply_lr != 0.0:
      self._apply.launch(apply_lr, optimizer, finish)
    return r if self._last_emit else [(None, None, t[2]) for t in r]


_WIRES = {'table': _lib.LOWP_WIRE_TABLE, 'float': _lib.LOWP_WIRE_FLOAT}


def rank_seed(seed, rank):
  """The seed rank ``rank`` steps its shards with: ``(seed + 0x9E3779B9 * rank) mod 2^32`` (include/hbk.h)."""
  return (int(seed) + 0x9E3779B9 * int(rank)) % (1 << 32)


class LowpShardedGroupLookup(ShardedGroupLookup):
  """N row-sharded 16-bit embedding tables looked up together: :class:`ShardedGroupLookup` over bf16 / fp16 shards.

  Args:
    shards16: this rank's local rows per column, ``torch.bfloat16`` / ``torch.float16`` ``[rows_local, dim]`` (a
      plan has 16-bit shards in every column; the two types may be mixed).
    coll, buckets, combiners, dedup: as :class:`ShardedGroupLookup`.
    wire: what crosses the link in the forward.  ``'table'`` (the default): the rows in the table's own 16 bits --
      the owner gather copies bits (``hbk_lowp_gather_rows_n``), the exchange moves 2-byte elements and the
      requester's stitch upcasts them (``hbk_lowp_lookup_fwd_runs``): half the wire bytes of fp32 and, unlike the
      fp16 wire, nothing is rounded.  ``'float'``: the owner upcasts (``hbk_lowp_lookup_fwd``) and everything behind
      it is the fp32 step -- the twin ``'table'`` is compared and timed against.  Both give, bit for bit,
      ``ShardedGroupLookup`` over ``[s.float() for s in shards16]`` on the fp32 wire.
    accums / moments, adam / ftrl_slots, ftrl / row_accums, rowwise_adagrad: FP32 slots of the shards' shapes
      (row-wise Adagrad: ``[rows_local, 1]``) and the optimizer objects, as :class:`LowpSparseApply` takes them.
    rounding, seed: as :class:`LowpSparseApply`.  The stochastic noise is keyed by the LOCAL row, so two ranks with
      one seed would round local row r alike: rank k steps with ``rank_seed = (seed + 0x9E3779B9 * k) mod 2^32``.

  ``__call__``, ``bind``, ``launch`` (weighted steps included), ``prefetch`` and the split forward are the base
  class's.  ``backward(grads, apply_lr=, optimizer=, emit=, finish=)`` is the plan's emit backward -- which never
  reads the shards and returns LOCAL row numbers, the gradient exchange in fp32 -- followed by a
  :class:`LowpSparseApply` on the shards; with ``emit=False`` the slices go into buffers this object owns.  All five
  optimizers.  The plan's own stepping entries read and write fp32 rows and are refused on a 16-bit plan at the ABI;
  this class never calls them.

  Refused by name: fp32 shards, ``max_norms``, ``weight_grads``, ``wire_dtype``, ``hot_rows`` and ``p2p_bind``."""

  def __init__(self, shards16, coll, buckets=None, combiners='sum', wire='table', dedup=False, accums=None,   # pylint: disable=super-init-not-called
               moments=None, adam=None, ftrl_slots=None, ftrl=None, row_accums=None, rowwise_adagrad=None,
               rounding='nearest', seed=0, max_norms=None, weight_grads=False, wire_dtype=None, hot_rows=False):
    what = 'LowpShardedGroupLookup'
    self.shards = _require_lowp_tables(shards16, what)
    if max_norms is not None and not (isinstance(max_norms, (list, tuple)) and all(x is None for x in max_norms)):
      raise _bad(f'{what}: max_norms is not supported for 16-bit shards (the clip reads and the clipped step writes '
                 'fp32 rows)')
    if weight_grads is not False and weight_grads is not None:
      raise _bad(f'{what}: weight_grads is not supported for 16-bit shards (the received rows are 16-bit)')
    if wire_dtype is not None:
      raise _bad(f"{what}: wire_dtype is not supported: a 16-bit plan names its wire with wire='table' | 'float' "
                 '(the fp16 wire rounds what it sends)')
    if hot_rows is not False and hot_rows is not None and hot_rows != [False] * len(self.shards):
      raise _bad(f'{what}: hot_rows is not supported for 16-bit shards (the low-precision gathers stage nothing)')
    if wire not in _WIRES:
      raise _bad(f"{what}: wire must be 'table' or 'float', got {wire!r}")
    check_rounding(rounding, seed, [t.dtype for t in self.shards], what)
    n = len(self.shards)
    self.wire = wire
    self.coll = coll
    self.world_size = int(coll.world_size)
    self.rank = int(getattr(coll, 'rank', 0))
    self.seed = int(seed)
    self.rank_seed = rank_seed(seed, self.rank)
    # a rank that owns no row of a table has an empty shard and empty slots, which have no address: the apply is
    # handed one-row stand-ins for them (never stepped: such a column's slices are empty), so that every column
    # keeps its index -- the stochastic noise is keyed by it
    empty = [c for c, t in enumerate(self.shards) if t.shape[0] == 0]

    def filled(tensors, pair=False):
      if tensors is None or not empty:
        return tensors
      tensors = list(tensors)
      for c in empty:
        one = lambda t: torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)   # noqa: E731
        tensors[c] = tuple(one(t) for t in tensors[c]) if pair else one(tensors[c])
      return tensors
    self._apply = LowpSparseApply(filled(self.shards), accums=filled(accums), moments=filled(moments, True), adam=adam,
                                  ftrl_slots=filled(ftrl_slots, True), ftrl=ftrl, row_accums=filled(row_accums),
                                  rowwise_adagrad=rowwise_adagrad, rounding=rounding, seed=self.rank_seed)
    # what the base class reads: no clip, no slots of the plan's own (they live with the apply), no hints
    self.weight_grads = False
    self.max_norms = [0.0] * n
    self.accums = None
    for cls in _opt.TWO_SLOT.values():
      setattr(self, cls.slot_kw, None)
      setattr(self, cls.name, None)
    self.buckets = [int(b or 0) for b in (buckets or [0] * n)]
    self.combiners = combiners
    self.wire_dtype = None
    self.device = self.shards[0].device if n else None
    self.dims = [int(t.shape[1]) for t in self.shards]
    self._auto_hot = []
    self._auto_state = None
    self.hot_rows = [False] * n
    self.dedup = [bool(dedup)] * n if isinstance(dedup, (bool, int)) else [bool(d) for d in dedup]
    self._own = None   # emit=False: per column (unique_rows, grad_rows, n_unique) this object owns
    self._setup()

  def _setup(self):
    self._lib = _lib.lib()

  def _plan_created(self):
    n = len(self.shards)
    _lib.check(self._lib.hbk_sharded_set_table_dtypes(
      self._plan_handle, (C.c_int32 * n)(*[_DTYPES[t.dtype] for t in self.shards]), _WIRES[self.wire]))

  @property
  def step_counter(self):
    return self._apply.step_counter

  def p2p_bind(self, outs):   # pylint: disable=unused-argument
    raise _lib.HbkError(_lib.UNIMPLEMENTED, 'LowpShardedGroupLookup: p2p_bind is not supported for 16-bit shards '
                        "(the p2p form's owner gather stores fp32 rows)")

  def _phase(self, *args, **kwargs):   # pylint: disable=unused-argument
    raise _lib.HbkError(_lib.UNIMPLEMENTED, 'LowpShardedGroupLookup has no separate phase methods: the step runs '
                        'inside the plan (__call__ / launch / backward)')

  partition = owner_gather = stitch = stitch_bwd = owner_bwd = _phase

  def _own_slices(self, plan):
    """Driver-owned IndexedSlices buffers with room for the rows this rank owns of the last forward."""
    n = len(self.shards)
    if self._own is None:
      self._own = [None] * n
    for c in range(n):
      k = int(self._lib.hbk_sharded_owned_ids(plan, c))
      if k < 0:
        raise _lib.HbkError(_lib.INTERNAL, 'backward() needs a forward step first')
      cur = self._own[c]
      if cur is None or cur[0].numel() < k:
        cap = max(k, 1) if cur is None else max(k, 2 * cur[0].numel())
        self._own[c] = (torch.empty(cap, dtype=torch.int64, device=self.device),
                        torch.empty((cap, self.dims[c]), dtype=torch.float32, device=self.device),
                        torch.zeros(1, dtype=torch.int32, device=self.device))
    return self._own

  def backward(self, grads, apply_lr=0.0, outs=None, optimizer='sgd', emit=True, finish=True, weight_grads=None):
    """Backward of the LAST forward step and, with ``apply_lr``, the optimizer step on the 16-bit shards.  Returns
    per column the IndexedSlices of the LOCAL shard ``(unique_rows, grad_rows, n_unique)``, equal to the fp32
    driver's; ``emit=False`` (with ``apply_lr``): the slices go into buffers this object owns and the triples are
    ``(None, None, n_unique)``.  ``optimizer``: 'sgd', 'adagrad', 'adam', 'ftrl' or 'rowwise_adagrad' (the slots
    given to the constructor); ``finish=True`` advances Adam's beta powers and the rounding's step counter once,
    behind the step.  ``weight_grads`` is refused."""
    if weight_grads is not False and weight_grads is not None:
      raise _bad('LowpShardedGroupLookup: weight_grads is not supported for 16-bit shards (the received rows are '
                 '16-bit)')
    if not emit and apply_lr == 0.0:
      raise _bad('emit=False needs apply_lr != 0')
    if apply_lr != 0.0:
      self._apply._check(apply_lr, optimizer)   # (before the exchange: a refused call moves nothing)
    else:
      _opt.two_slot_class(optimizer)
    if not emit and outs is None:
      outs = self._own_slices(self._plan())
    r = ShardedGroupLookup.backward(self, grads, apply_lr=0.0, outs=outs, optimizer='sgd', emit=True, weight_grads=False)
    if apply_lr != 0.0:
      self._apply(self._apply_views(r), apply_lr, optimizer, finish)
    return r if emit else [(None, None, t[2]) for t in r]

  def _apply_views(self, slices):
    """The slices as :class:`LowpSparseApply` takes them: ``grad_rows`` ``[capacity, dim]`` (caller-owned outputs
    may be larger than the rows they hold)."""
    out = []
    for c, (u, g, nu) in enumerate(slices):
      cap = int(u.shape[0])
      if g.dim() != 2 or tuple(g.shape) != (cap, self.dims[c]):
        g = g.reshape(-1)[:cap * self.dims[c]].view(cap, self.dims[c])
      out.append((u, g, nu))
    return out
