"""Unaligned row layouts: every row-moving kernel family picks 16-byte chunks only when the dim and
every operand address and row stride allow it, and moves the row as 4-byte chunks (one lane per
float, at most 64 floats) otherwise.  Tensors from the caching allocator are 256-byte aligned, so
the rest of the suite reaches the 4-byte form only at dims 1, 3 and 6.  Here every operand is placed
by hand (`placed`): shifted 1-3 floats into a buffer of NaN sentinels and given odd row pitches, at
dims 1-64 where lane masking goes wrong.  Results must equal the aligned run and the references,
and no float outside an operand may change.  Refused calls must refuse before any device work, and
DenseFeatures must accept any column dims."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from tests.support.tolerance import assert_sums_close
from tests.test_gpu_adam import np_adam, B1, B2, EPS
from tests.test_gpu_parity import _in_order_slices, RTOL
from tests.test_gpu_weighted import ref_fwd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
SENT32 = 0x7fc0dead            # a quiet NaN with a payload no kernel computes
SENT16 = 0x7dea                # an fp16 NaN, likewise
DIMS = [4, 8, 12, 16, 20, 28, 32, 36, 48, 60, 64, 1, 3]
# (shift in floats, pitch - dim): the aligned control first
LAYOUTS = [(0, 0), (1, 0), (2, 1), (3, 3), (0, 1), (2, 3), (1, 1), (3, 0)]
COMBS = {'sum': _lib.COMBINER_SUM, 'mean': _lib.COMBINER_MEAN, 'sqrtn': _lib.COMBINER_SQRTN}


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.detach().cpu().numpy()


def stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Arena:
  """A flat buffer of sentinel bits (256-byte aligned, from the caching allocator) that operands
  are carved from at any offset and row pitch; `check` asserts every element outside them kept
  the sentinel."""

  def __init__(self, n, half=False):
    self.half = half
    it = torch.int16 if half else torch.int32
    sent = SENT16 if half else SENT32
    self.bits = torch.full((n,), sent, dtype=it, device=DEV)
    self.buf = self.bits.view(torch.float16 if half else torch.float32)
    self.sent = sent
    self.regions = []

  def view(self, shape, at, pitch=None):
    rows, dim = shape
    pitch = dim if pitch is None else pitch
    assert at + (rows - 1) * pitch + dim <= self.buf.numel() if rows else True
    self.regions.append((at, rows, dim, pitch))
    return self.buf.as_strided((rows, dim), (pitch, 1), at)

  def check(self, what):
    bits = host(self.bits)
    outside = np.ones(bits.size, bool)
    for at, rows, dim, pitch in self.regions:
      if rows:
        idx = at + np.arange(rows)[:, None] * pitch + np.arange(dim)[None, :]
        outside[idx.ravel()] = False
    bad = np.nonzero(outside & (bits != self.sent))[0]
    assert bad.size == 0, f'{what}: {bad.size} sentinel elements overwritten, first at {bad[:8]}'


def placed(shape, shift, pitch=None, half=False):
  """`[rows, dim]` view that starts `shift` elements into a sentinel buffer, row stride `pitch`
  (default dim); returns (view, check)."""
  rows, dim = shape
  pitch = dim if pitch is None else pitch
  a = Arena(shift + max(rows - 1, 0) * pitch + dim + 16, half=half)
  v = a.view(shape, shift, pitch)
  return v, a.check


def ragged(rng, n_seg, lens=(0, 1, 2, 3, 5)):
  return np.concatenate([[0], np.cumsum(rng.choice(lens, size=n_seg))]).astype(np.int32)


def ptr(t):
  return None if t is None else t.data_ptr()


# ---- 1. forward ---------------------------------------------------------------------------------
def _fwd_cols(rng, id64):
  """One column per dim, kinds rotating: one id per sample with a bucket, ragged sum / mean with
  out-of-range ids, ragged sqrtn with a divisor, weighted ragged mean."""
  idt = np.int64 if id64 else np.int32
  spec = []
  for k, d in enumerate([3, 16, 20, 36, 6, 64] + DIMS):
    kind = k % 5
    rows = 2003 + 17 * k
    batch = 300
    splits = None if kind == 0 else ragged(rng, batch)
    n = batch if splits is None else int(splits[-1])
    if kind == 0:
      ids, bucket, div, comb = rng.randint(0, 1 << 30, size=n), rows, 1, 'sum'
    elif kind in (1, 2):
      ids, bucket, div, comb = rng.randint(-20, rows + 60, size=n), 0, 1, ('sum', 'mean')[kind - 1]
    elif kind == 3:
      ids, bucket, div, comb = rng.randint(0, 2 * rows, size=n), 0, 2, 'sqrtn'
    else:
      ids, bucket, div, comb = rng.randint(0, rows, size=n), 0, 1, 'mean'
    w = rng.uniform(0.25, 2, size=n).astype(F32) if kind == 4 else None
    spec.append(dict(dim=d, rows=rows, ids=ids.astype(idt), splits=splits, bucket=bucket, div=div,
                     comb=comb, w=w, table=rng.uniform(-1, 1, size=(rows, d)).astype(F32),
                     batch=batch))
  return spec


def _run_fwd(spec, shift, gap, t_shift):
  """The columns' outputs side by side in ONE [batch, pitch] block that starts `shift` floats into
  a sentinel arena, `gap` sentinel floats between blocks; tables `t_shift` floats in."""
  batch = spec[0]['batch']
  offs, o = [], 0
  for s in spec:
    offs.append(o)
    o += s['dim'] + gap
  pitch = o + gap
  arena = Arena(shift + batch * pitch + 16)
  block = arena.view((batch, pitch), shift)
  arena.regions.clear()
  outs = [arena.view((batch, s['dim']), shift + off, pitch) for s, off in zip(spec, offs)]
  keep, tchecks = [], []
  cols = (_lib.LookupColumn * len(spec))()
  for c, s in enumerate(spec):
    t, chk = placed(s['table'].shape, t_shift)
    t.copy_(dev(s['table']))
    tchecks.append(chk)
    ids = dev(s['ids'])
    sp = None if s['splits'] is None else dev(s['splits'])
    w = None if s['w'] is None else dev(s['w'])
    keep += [t, ids, sp, w]
    col = cols[c]
    col.table, col.rows, col.dim = t.data_ptr(), s['rows'], s['dim']
    col.ids_dtype = _lib.INT64 if s['ids'].dtype == np.int64 else _lib.INT32
    col.ids, col.n_ids = ids.data_ptr(), ids.numel()
    col.row_splits, col.n_segments = ptr(sp), batch
    col.bucket, col.divisor, col.combiner = s['bucket'], s['div'], COMBS[s['comb']]
    col.out, col.out_stride = outs[c].data_ptr(), pitch
    col.id_weights = ptr(w)
  _lib.check(_lib.lib().hbk_group_lookup_fwd(len(spec), cols, stream()))
  torch.cuda.synchronize()
  del block
  arena.check(f'forward block (shift {shift}, gap {gap})')
  for c, chk in enumerate(tchecks):
    chk(f'table {c}')
  return [host(o) for o in outs]


def _fwd_want(s):
  ids = s['ids'].astype(np.int64)
  if s['w'] is not None:
    return ref_fwd(s['table'], ids, s['splits'], s['w'], s['comb'], s['bucket'], s['div'])
  rows = np.where(ids >= 0, ids // s['div'], -1) if s['div'] > 1 else ids
  return oracle.group_lookup_fwd([s['table']], [rows], [s['splits']], [s['bucket']], [s['comb']])[0]


def _fwd_f64(s):
  """float64 embedding_bag of the column and the magnitudes of its terms."""
  ids = s['ids'].astype(np.int64)
  r = ids % s['bucket'] if s['bucket'] else ids
  r = np.where(r >= 0, r // s['div'], -1)
  ok = (r >= 0) & (r < s['rows'])
  sp = s['splits'] if s['splits'] is not None else np.arange(ids.size + 1, dtype=np.int32)
  seg = np.repeat(np.arange(sp.size - 1), np.diff(sp))
  w = np.ones(ids.size) if s['w'] is None else s['w'].astype(np.float64)
  want = np.zeros((sp.size - 1, s['dim']))
  mag = np.zeros_like(want)
  terms = s['table'][np.where(ok, r, 0)].astype(np.float64) * (w * ok)[:, None]
  np.add.at(want, seg, terms)
  np.add.at(mag, seg, np.abs(terms))
  # unweighted: mean / sqrtn count every id of the segment; weighted: ids outside the table add no
  # weight (include/hbk.h)
  den = np.zeros(sp.size - 1)
  np.add.at(den, seg, (w if s['comb'] == 'mean' else w * w) * (ok if s['w'] is not None else 1))
  if s['comb'] != 'sum':
    d = den if s['comb'] == 'mean' else np.sqrt(den)
    nz = d != 0
    want[nz] /= d[nz][:, None]
    mag[nz] /= d[nz][:, None]
  return want, mag


@pytest.mark.parametrize('opts', ['default', 'hot_d16'])
@pytest.mark.parametrize('id64', [False, True])
def test_forward_shared_block_every_phase(hbk_option, opts, id64):
  if opts == 'hot_d16':
    hbk_option('fwd_hot_rows', 1)
    hbk_option('fwd_d16', 1)
  rng = np.random.RandomState(100 + id64)
  spec = _fwd_cols(rng, id64)
  control = _run_fwd(spec, 0, 0, 0)
  for s, got in zip(spec, control):
    np.testing.assert_array_equal(got, _fwd_want(s), err_msg=f'aligned dim {s["dim"]} {s["comb"]}')
    want, mag = _fwd_f64(s)
    assert_sums_close(got, want, mag, err_msg=f'aligned dim {s["dim"]}')
  for shift, gap, t_shift in ((1, 0, 1), (2, 1, 3), (3, 3, 2), (0, 1, 0), (1, 3, 0)):
    outs = _run_fwd(spec, shift, gap, t_shift)
    for s, got, ref in zip(spec, outs, control):
      np.testing.assert_array_equal(got, ref, err_msg=f'dim {s["dim"]} {s["comb"]} at shift {shift} '
                                    f'gap {gap} table shift {t_shift}')


@pytest.mark.parametrize('dim', [4, 8, 16, 20, 36, 64, 3])
def test_forward_half_output_at_8_and_4_byte_alignment(dim):
  """HBK_LOOKUP_OUT_HALF: fp16 rows at offsets of 0-3 halves and an odd pitch; bits equal the fp32
  oracle rounded to nearest even."""
  rng = np.random.RandomState(dim)
  rows, batch = 1009, 400
  table = rng.uniform(-70000, 70000, size=(rows, dim)).astype(F32)
  ids = rng.randint(0, 1 << 30, size=batch).astype(np.int64)
  want = oracle.group_lookup_fwd([table], [ids], [None], [rows], ['sum'])[0].astype(np.float16)
  t = dev(table)
  d_ids = dev(ids)
  for shift, extra in ((0, 0), (1, 0), (2, 1), (3, 3), (4, 2)):
    out, chk = placed((batch, dim), shift, dim + extra, half=True)
    cols = (_lib.LookupColumn * 1)()
    col = cols[0]
    col.table, col.rows, col.dim, col.ids_dtype = t.data_ptr(), rows, dim, _lib.INT64
    col.ids, col.n_ids, col.n_segments, col.bucket, col.divisor = d_ids.data_ptr(), batch, batch, rows, 1
    col.out, col.out_stride, col.half_io = out.data_ptr(), dim + extra, 1
    _lib.check(_lib.lib().hbk_group_lookup_fwd(1, cols, stream()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(out).view(np.uint16), want.view(np.uint16),
                                  err_msg=f'dim {dim} shift {shift} pitch {dim + extra}')
    chk(f'half output dim {dim} shift {shift}')


# ---- 2. backward: emit, SGD, Adagrad ------------------------------------------------------------
class BwdCase:
  """Columns of one C-ABI backward call with every operand placed by hand."""

  def __init__(self, rng, dims, layouts, id64=True, n=1500, rows_of=None, combs=None, ragged_every=3):
    self.cols = []
    idt = np.int64 if id64 else np.int32
    for k, d in enumerate(dims):
      rows = rows_of(k) if rows_of else (400 + 31 * k if k % 2 else 20000 + 101 * k)
      comb = combs[k % len(combs)] if combs else ('sum', 'mean', 'sqrtn')[k % 3]
      splits = ragged(rng, n // 3) if k % ragged_every == 1 else None
      n_ids = n if splits is None else int(splits[-1])
      ids = rng.randint(0, 1 << 40, size=n_ids).astype(idt) if id64 else \
          rng.randint(0, 1 << 30, size=n_ids).astype(idt)
      n_seg = n_ids if splits is None else splits.size - 1
      self.cols.append(dict(dim=d, rows=rows, ids=ids, splits=splits, comb=comb if splits is not None
                            else 'sum', layout=layouts[k % len(layouts)], n_seg=n_seg,
                            grads=rng.randn(n_seg, d).astype(F32),
                            table=rng.uniform(-1, 1, size=(rows, d)).astype(F32),
                            accum=rng.uniform(0.1, 0.5, size=(rows, d)).astype(F32)))

  def rows(self, c):
    s = self.cols[c]
    return s['ids'].astype(np.int64) % s['rows']

  def run(self, lr=0.0, apply=_lib.APPLY_SGD, aligned=False, override=None):
    """One call; returns per column (unique_rows, grad_rows, table, accum) on the host and checks
    the sentinels.  override(c, col): last word on a column's descriptor."""
    n = len(self.cols)
    cols = (_lib.LookupGradColumn * n)()
    keep, checks, res = [], [], []
    for c, s in enumerate(self.cols):
      d, rows = s['dim'], s['rows']
      shift, extra = (0, 0) if aligned else s['layout']
      aligned_col = (shift, extra) == (0, 0)   # every operand of the column 16-byte aligned
      g, gchk = placed((s['n_seg'], d), shift, d + extra)
      g.copy_(dev(s['grads']))
      gr, grchk = placed((s['ids'].size, d), (shift + 1) % 4 if not aligned_col else 0)
      t, tchk = placed((rows, d), (shift + 2) % 4 if not aligned_col else 0, d + extra)
      t.copy_(dev(s['table']))
      a, achk = placed((rows, d), (shift + 3) % 4 if not aligned_col else 0, d + extra)
      a.copy_(dev(s['accum']))
      ids = dev(s['ids'])
      sp = None if s['splits'] is None else dev(s['splits'])
      ur = torch.empty(s['ids'].size, dtype=torch.int64, device=DEV)
      nu = torch.full((1,), -7, dtype=torch.int32, device=DEV)
      keep += [g, gr, t, a, ids, sp, ur, nu]
      checks += [(gchk, f'grad_out {c}'), (grchk, f'grad_rows {c}'), (tchk, f'table {c}'),
                 (achk, f'accum {c}')]
      col = cols[c]
      col.table, col.rows, col.dim = t.data_ptr(), rows, d
      col.ids_dtype = _lib.INT64 if s['ids'].dtype == np.int64 else _lib.INT32
      col.ids, col.n_ids = ids.data_ptr(), s['ids'].size
      col.row_splits, col.n_segments = ptr(sp), s['n_seg']
      col.bucket, col.divisor, col.combiner = rows, 1, COMBS[s['comb']]
      col.grad_out, col.grad_stride = g.data_ptr(), d + extra
      col.unique_rows, col.grad_rows, col.n_unique = ur.data_ptr(), gr.data_ptr(), nu.data_ptr()
      col.accum = a.data_ptr() if apply == _lib.APPLY_ADAGRAD else None
      col.table_pitch = d + extra
      if override is not None:
        override(c, col)
      res.append((ur, gr, nu, t, a))
    lib = _lib.lib()
    wsb = lib.hbk_group_lookup_bwd_workspace_bytes(n, cols)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=DEV)
    _lib.check(lib.hbk_group_lookup_bwd_apply(n, cols, apply, C.c_float(lr), ws.data_ptr(), wsb,
                                              stream()))
    torch.cuda.synchronize()
    for chk, what in checks:
      chk(what)
    out = []
    for ur, gr, nu, t, a in res:
      k = int(nu.item())
      out.append((host(ur)[:k], host(gr)[:k], host(t), host(a)))
    return out

  def check_emitted(self, out, det):
    for c, s in enumerate(self.cols):
      u, g = out[c][0], out[c][1]
      rows = self.rows(c)
      what = f'column {c} dim {s["dim"]} layout {s["layout"]}'
      if det:
        want_u, want_g = _in_order_slices(rows, s['grads'], s['splits'], s['comb'], s['rows'])
        np.testing.assert_array_equal(u, want_u, err_msg=what)
        np.testing.assert_array_equal(g, want_g, err_msg=what)
        continue
      ou, oinv = oracle.unique(rows)
      assert u.size == ou.size and set(u.tolist()) == set(ou.tolist()), what
      sp = s['splits'] if s['splits'] is not None else np.arange(rows.size + 1, dtype=np.int32)
      g_id = oracle.segment_combine_grad(s['grads'], sp, s['comb'])
      want64 = oracle.unsorted_segment_sum(g_id, oinv, ou.size, f64=True)
      abs64 = oracle.unsorted_segment_sum(np.abs(g_id), oinv, ou.size, f64=True)
      at = {int(r): i for i, r in enumerate(ou.tolist())}
      pos = np.array([at[int(r)] for r in u.tolist()], np.int64)
      assert_sums_close(g.astype(np.float64), want64[pos], abs64[pos], rel=RTOL, err_msg=what)

  def check_stepped(self, out, lr, apply):
    for c, s in enumerate(self.cols):
      u, g, t, a = out[c]
      want_t, want_a = s['table'].copy(), s['accum'].copy()
      if apply == _lib.APPLY_ADAGRAD:
        oracle.sparse_adagrad_apply(want_t, want_a, u, g, lr)
      else:
        oracle.sparse_sgd_apply(want_t, u, g, lr)
      what = f'column {c} dim {s["dim"]} layout {s["layout"]}'
      np.testing.assert_array_equal(t, want_t, err_msg='table of ' + what)
      np.testing.assert_array_equal(a, want_a, err_msg='accum of ' + what)


BWD_OPTS = [('bwd_dense', 0), ('bwd_dense', 1), ('bwd_dense', 2), ('bwd_dense', 3),
            ('bwd_onepass', 0), ('bwd_onepass', 1), ('bwd_wide', 0), ('bwd_wide', 1), ('bwd_wide', 2),
            ('bwd_simple', 1), ('bwd_group_cols', 1), ('bwd_deterministic', 1),
            ('bwd_deterministic', 2)]


@pytest.mark.parametrize('opt', BWD_OPTS, ids=[f'{k}={v}' for k, v in BWD_OPTS])
def test_backward_misaligned_every_dim(hbk_option, opt):
  """Every dim at a rotating layout, with an aligned dim-16 and dim-128 column in the same launch
  group (a deterministic group with one misaligned column runs all of it in 4-byte chunks): emit,
  SGD and Adagrad."""
  hbk_option(*opt)
  det = opt[0] == 'bwd_deterministic'
  rng = np.random.RandomState(BWD_OPTS.index(opt))
  dims = DIMS + [16, 128]
  layouts = LAYOUTS[1:] * 2
  layouts = layouts[:len(DIMS)] + [(0, 0), (0, 0)]
  case = BwdCase(rng, dims, layouts, id64=opt[1] % 2 == 0)
  out = case.run()
  case.check_emitted(out, det)
  if det:   # bit-equal to the aligned run
    ref = case.run(aligned=True)
    for c in range(len(dims)):
      np.testing.assert_array_equal(out[c][0], ref[c][0])
      np.testing.assert_array_equal(out[c][1], ref[c][1])
  for apply in (_lib.APPLY_SGD, _lib.APPLY_ADAGRAD):
    out = case.run(lr=0.05, apply=apply)
    case.check_emitted(out, det)
    case.check_stepped(out, 0.05, apply)


@pytest.mark.parametrize('det', [0, 1, 2])
def test_backward_more_than_64_columns(hbk_option, det):
  hbk_option('bwd_deterministic', det)
  rng = np.random.RandomState(70 + det)
  dims = [DIMS[k % len(DIMS)] for k in range(70)]
  case = BwdCase(rng, dims, LAYOUTS, n=200, rows_of=lambda k: 97 + 13 * k if k % 3 else 20000 + k)
  out = case.run(lr=0.05, apply=_lib.APPLY_ADAGRAD)
  case.check_emitted(out, det != 0)
  case.check_stepped(out, 0.05, _lib.APPLY_ADAGRAD)


def test_stitch_backward_misaligned_grad_stride():
  """hbk_group_stitch_bwd: per-id gradient rows of a misaligned, odd-strided grad_out, against
  float64."""
  rng = np.random.RandomState(5)
  lib = _lib.lib()
  for d in (4, 12, 20, 36, 64, 3):
    for shift, extra in ((0, 0), (1, 0), (3, 1), (2, 3)):
      n_seg = 300
      splits = ragged(rng, n_seg)
      n_ids = int(splits[-1])
      grads = rng.randn(n_seg, d).astype(F32)
      g, gchk = placed((n_seg, d), shift, d + extra)
      g.copy_(dev(grads))
      index = rng.permutation(n_ids).astype(np.int32)
      out, ochk = placed((n_ids, d), (shift + 1) % 4)
      sp = dev(splits)
      idx = dev(index)
      for comb in ('sum', 'mean', 'sqrtn'):
        cols = (_lib.StitchGradColumn * 1)()
        col = cols[0]
        col.dim, col.combiner, col.n_ids = d, COMBS[comb], n_ids
        col.index, col.row_splits, col.n_segments = idx.data_ptr(), sp.data_ptr(), n_seg
        col.grad_out, col.grad_rows, col.grad_stride = g.data_ptr(), out.data_ptr(), d + extra
        _lib.check(lib.hbk_group_stitch_bwd(1, cols, stream()))
        torch.cuda.synchronize()
        lens = np.diff(splits).astype(np.float64)
        scale = {'sum': np.ones_like(lens), 'mean': 1 / np.maximum(lens, 1),
                 'sqrtn': 1 / np.sqrt(np.maximum(lens, 1))}[comb]
        seg = np.repeat(np.arange(n_seg), np.diff(splits))
        want = np.zeros((n_ids, d))
        want[index] = grads[seg].astype(np.float64) * scale[seg][:, None]
        assert_sums_close(host(out), want, np.abs(want), err_msg=f'dim {d} shift {shift} {comb}')
        gchk(f'stitch grad_out dim {d}')
        ochk(f'stitch grad_rows dim {d}')


# ---- 3. Lazy Adam -------------------------------------------------------------------------------
def _adam_call(cols, n, m_ptrs, v_ptrs, powers, lr, finish=1):
  lib = _lib.lib()
  params = _lib.AdamParams(B1, B2, EPS, powers.data_ptr(), finish)
  wsb = lib.hbk_group_lookup_bwd_adam_workspace_bytes(n, cols)
  ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=DEV)
  mp = (C.c_void_p * n)(*m_ptrs)
  vp = (C.c_void_p * n)(*v_ptrs)
  return lib.hbk_group_lookup_bwd_adam(n, cols, mp, vp, C.byref(params), C.c_float(lr),
                                       ws.data_ptr(), wsb, stream())


@pytest.mark.parametrize('interleaved', [False, True])
def test_adam_misaligned_slots(hbk_option, interleaved):
  """m and v misaligned, or [w|m|v|pad] rows at a pitch of 4 dim + 1: one step bit-equal to numpy on
  the call's own slices, rows no id names untouched, sentinels intact."""
  rng = np.random.RandomState(9 + interleaved)
  dims = [4, 8, 12, 20, 36, 48, 64, 3, 16]
  n = len(dims)
  cols = (_lib.LookupGradColumn * n)()
  keep, host_state, dev_state, checks = [], [], [], []
  m_ptrs, v_ptrs = [], []
  p0 = (F32(B1 ** 2), F32(B2 ** 2))
  powers = dev(np.array(p0, F32))
  for c, d in enumerate(dims):
    rows = 3001 + c
    w0 = rng.uniform(-1, 1, size=(rows, d)).astype(F32)
    m0 = rng.uniform(-0.1, 0.1, size=(rows, d)).astype(F32)
    v0 = rng.uniform(0, 0.01, size=(rows, d)).astype(F32)
    shift = 1 + c % 3
    if interleaved:
      pitch = 4 * d + 1
      ar = Arena(shift + rows * pitch + 16)
      w = ar.view((rows, d), shift, pitch)
      m = ar.view((rows, d), shift + d, pitch)
      v = ar.view((rows, d), shift + 2 * d, pitch)
      checks.append((ar.check, f'interleaved rows of column {c}'))
    else:
      pitch = d
      w, chk = placed((rows, d), 0)
      m, chk_m = placed((rows, d), shift)
      v, chk_v = placed((rows, d), (shift + 1) % 4)
      checks += [(chk, f'w {c}'), (chk_m, f'm {c}'), (chk_v, f'v {c}')]
    for x, y in ((w, w0), (m, m0), (v, v0)):
      x.copy_(dev(y))
    ids = rng.randint(0, 1 << 40, size=800).astype(np.int64)
    g, gchk = placed((ids.size, d), (shift + 2) % 4, d + 1)
    g.copy_(dev(rng.randn(ids.size, d).astype(F32)))
    ur = torch.empty(ids.size, dtype=torch.int64, device=DEV)
    gr, grchk = placed((ids.size, d), shift)
    nu = torch.zeros(1, dtype=torch.int32, device=DEV)
    checks += [(gchk, f'grad_out {c}'), (grchk, f'grad_rows {c}')]
    d_ids = dev(ids)
    keep += [w, m, v, g, ur, gr, nu, d_ids]
    col = cols[c]
    col.table, col.rows, col.dim, col.ids_dtype = w.data_ptr(), rows, d, _lib.INT64
    col.ids, col.n_ids, col.n_segments, col.bucket, col.divisor = d_ids.data_ptr(), ids.size, ids.size, rows, 1
    col.grad_out, col.grad_stride, col.table_pitch = g.data_ptr(), d + 1, pitch
    col.unique_rows, col.grad_rows, col.n_unique = ur.data_ptr(), gr.data_ptr(), nu.data_ptr()
    m_ptrs.append(m.data_ptr())
    v_ptrs.append(v.data_ptr())
    host_state.append((w0, m0, v0))
    dev_state.append((w, m, v, ur, gr, nu))
  _lib.check(_adam_call(cols, n, m_ptrs, v_ptrs, powers, 0.01))
  torch.cuda.synchronize()
  for chk, what in checks:
    chk(what)
  for c in range(n):
    w, m, v, ur, gr, nu = dev_state[c]
    k = int(nu.item())
    u, g = host(ur)[:k], host(gr)[:k]
    assert np.unique(u).size == k
    ww, mm, vv = (x.copy() for x in host_state[c])
    want_p = np_adam(ww, mm, vv, u, g, 0.01, p0[0], p0[1])
    np.testing.assert_array_equal(host(w), ww, err_msg=f'w of column {c} dim {dims[c]}')
    np.testing.assert_array_equal(host(m), mm, err_msg=f'm of column {c} dim {dims[c]}')
    np.testing.assert_array_equal(host(v), vv, err_msg=f'v of column {c} dim {dims[c]}')
  np.testing.assert_array_equal(host(powers), np.array(want_p, F32))


# ---- 4. cast_n ----------------------------------------------------------------------------------
def test_cast_n_every_phase_and_rounding_boundaries():
  """fp32 -> fp16 with inputs and outputs 1-7 elements into their buffers and lengths that are not
  multiples of 8 (vector body and scalar tails at every phase), against numpy's round to nearest
  even; fp16 -> fp32 exact."""
  special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 65504, 65519, 65520, -65520, 2.0 ** -24,
                      2.0 ** -25, -(2.0 ** -25), 3 * 2.0 ** -26, 6.097555e-05, 6.1035156e-05,
                      1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65536.0, 1e-9], F32)
  rng = np.random.RandomState(3)
  lib = _lib.lib()
  ins, outs, lens, want, checks, keep = [], [], [], [], [], []
  for k, n in enumerate([1, 7, 9, 15, 17, 63, 65, 131, 1003, 4097]):
    for sh_in in range(1, 8):
      sh_out = (sh_in * 3 + k) % 8
      x = np.concatenate([special, rng.randn(n).astype(F32) * F32(10.0 ** rng.randint(-6, 5))])[:n]
      x = rng.permutation(np.concatenate([x, special]))[:max(n, 1)] if n >= special.size else x
      xi, ichk = placed((1, x.size), sh_in)
      xi.copy_(dev(x[None]))
      xo, ochk = placed((1, x.size), sh_out, half=True)
      ins.append(xi.data_ptr())
      outs.append(xo.data_ptr())
      lens.append(x.size)
      want.append(x.astype(np.float16))
      checks += [(ichk, 'input'), (ochk, f'output of {x.size} at phase {sh_out}')]
      keep.append((xi, xo))
  m = len(ins)
  _lib.check(lib.hbk_cast_n(m, _lib.FLOAT, _lib.HALF, (C.c_void_p * m)(*ins), (C.c_int64 * m)(*lens),
                            (C.c_void_p * m)(*outs), stream()))
  torch.cuda.synchronize()
  for chk, what in checks:
    chk(what)
  for (xi, xo), w in zip(keep, want):
    got = host(xo)[0]
    nan = np.isnan(w)
    assert (np.isnan(got) == nan).all()
    np.testing.assert_array_equal(got[~nan].view(np.uint16), w[~nan].view(np.uint16))
  # and back: fp16 -> fp32 is exact, at every phase
  backs, bchecks = [], []
  for (xi, xo), w, n in zip(keep, want, lens):
    b, chk = placed((1, n), (xo.storage_offset() + 5) % 8)
    backs.append(b)
    bchecks.append(chk)
  _lib.check(lib.hbk_cast_n(m, _lib.HALF, _lib.FLOAT, (C.c_void_p * m)(*outs), (C.c_int64 * m)(*lens),
                            (C.c_void_p * m)(*[b.data_ptr() for b in backs]), stream()))
  torch.cuda.synchronize()
  for b, chk, w in zip(backs, bchecks, want):
    chk('fp16 -> fp32 output')
    got = host(b)[0]
    nan = np.isnan(w)
    np.testing.assert_array_equal(got[~nan], w[~nan].astype(F32))
    assert np.isnan(got[nan]).all()


# ---- 5. refusals are all-or-nothing -------------------------------------------------------------
BIG_ROWS = 300_000_000   # more row-sorted buckets than the jobs take: the deterministic sort path


class RefusalCase:
  """Columns of one SGD call: `spec` = [(dim, rows, grad shift, grad stride or None)].  Tables of
  BIG_ROWS rows are zeros, and only the rows the ids name are read back."""

  def __init__(self, rng, spec, n=300):
    self.cols = []
    for d, rows, shift, stride in spec:
      ids = rng.randint(0, rows, size=n).astype(np.int64)
      ids[::10] = ids[5::10][:ids[::10].size]
      grads = rng.randn(n, d).astype(F32)
      big = rows == BIG_ROWS
      table0 = None if big else rng.uniform(-1, 1, size=(rows, d)).astype(F32)
      self.cols.append(dict(dim=d, rows=rows, ids=ids, grads=grads, shift=shift, stride=stride,
                            table0=table0, table=torch.zeros(rows, d, device=DEV) if big else dev(table0),
                            ur=torch.full((n,), -3, dtype=torch.int64, device=DEV),
                            gr=torch.full((n, d), 5.0, device=DEV),
                            nu=torch.full((1,), -7, dtype=torch.int32, device=DEV)))

  def watched(self):
    """What a refused call must leave alone: the rows the ids name, the emitted slices, n_unique."""
    out = []
    for s in self.cols:
      out.append([host(s['table'][dev(s['ids'])]), host(s['ur']), host(s['gr']), host(s['nu'])])
    return out

  def call(self, lr):
    n = len(self.cols)
    cols = (_lib.LookupGradColumn * n)()
    keep = []
    for c, s in enumerate(self.cols):
      d = s['dim']
      stride = s['stride'] or d
      gbuf = torch.zeros(s['shift'] + s['ids'].size * max(stride, d) + 8, device=DEV)
      g = gbuf.as_strided((s['ids'].size, d), (stride, 1), s['shift'])
      if stride >= d:
        g.copy_(dev(s['grads']))
      ids = dev(s['ids'])
      keep += [gbuf, ids]
      col = cols[c]
      col.table, col.rows, col.dim, col.ids_dtype = s['table'].data_ptr(), s['rows'], d, _lib.INT64
      col.ids, col.n_ids, col.n_segments = ids.data_ptr(), s['ids'].size, s['ids'].size
      col.bucket, col.divisor = 0, 1
      col.grad_out, col.grad_stride = g.data_ptr(), stride
      col.unique_rows, col.grad_rows, col.n_unique = s['ur'].data_ptr(), s['gr'].data_ptr(), s['nu'].data_ptr()
    lib = _lib.lib()
    wsb = lib.hbk_group_lookup_bwd_workspace_bytes(n, cols)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=DEV)
    rc = lib.hbk_group_lookup_bwd_apply(n, cols, _lib.APPLY_SGD, C.c_float(lr), ws.data_ptr(), wsb,
                                        stream())
    torch.cuda.synchronize()
    _lib.check(rc)

  def expect_refused(self, lr, match):
    torch.cuda.synchronize()
    before = self.watched()
    with pytest.raises(_lib.InvalidArgumentError, match=match):
      self.call(lr)
    after = self.watched()
    for c in range(len(self.cols)):
      for name, a, b in zip(('stepped rows', 'unique_rows', 'grad_rows', 'n_unique'), after[c], before[c]):
        np.testing.assert_array_equal(a, b, err_msg=f'{name} of column {c} after a refused call')

  def check_result(self, lr, det):
    for c, s in enumerate(self.cols):
      k = int(s['nu'].item())
      u, g = host(s['ur'])[:k], host(s['gr'])[:k]
      want_u, want_g = _in_order_slices(s['ids'], s['grads'], None, 'sum', s['rows'])
      what = f'column {c} dim {s["dim"]}'
      if det:
        np.testing.assert_array_equal(u, want_u, err_msg=what)
        np.testing.assert_array_equal(g, want_g, err_msg=what)
      else:
        assert k == want_u.size and set(u.tolist()) == set(want_u.tolist()), what
      if s['table0'] is not None:
        want = s['table0'].copy()
        oracle.sparse_sgd_apply(want, u, g, lr)
        np.testing.assert_array_equal(host(s['table']), want, err_msg='table of ' + what)
      else:
        want = np.zeros((k, s['dim']), F32)
        oracle.sparse_sgd_apply(want, np.arange(k), g, lr)
        np.testing.assert_array_equal(host(s['table'][torch.from_numpy(u).to(DEV)]), want,
                                      err_msg='table of ' + what)


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_refused_call_changes_nothing(hbk_option, mode):
  """dim 128 with grad_out 4 bytes off: 16-byte chunks are impossible and the 4-byte form holds at
  most 64 floats -- except on the deterministic sort path, which walks up to 256 floats as scalars.
  Over a small table the column takes the row-sorted jobs under mode 1, so modes 0 and 1 refuse it,
  alone and beside sort-path columns (which must not have been stepped); mode 2 sorts every column
  and accepts it.  A valid call on the same objects then gives the normal result."""
  hbk_option('bwd_deterministic', mode)
  rng = np.random.RandomState(31 + mode)
  lr = 0.05
  for spec in ([(128, 700, 1, None)],
               [(4, BIG_ROWS, 0, None), (128, 700, 1, None), (8, BIG_ROWS, 3, 9)]):
    case = RefusalCase(rng, spec)
    refused_col = [c for c, x in enumerate(spec) if x[0] == 128][0]
    if mode == 2:
      case.call(lr)
      case.check_result(lr, True)
      continue
    case.expect_refused(lr, f'column {refused_col}: dim 128 needs more than 64 lanes')
    case.cols[refused_col]['shift'] = 0
    case.call(lr)
    case.check_result(lr, mode != 0)


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_grad_stride_below_dim_is_refused_in_every_mode(hbk_option, mode):
  """grad_stride = dim - 1 (rows of grad_out that overlap) is refused on every path, the sort
  included, before the sort-path column beside it is stepped."""
  hbk_option('bwd_deterministic', mode)
  rng = np.random.RandomState(41)
  lr = 0.05
  case = RefusalCase(rng, [(4, BIG_ROWS, 0, None), (16, 800, 0, None), (32, 3000, 1, 31)])
  case.expect_refused(lr, 'column 2: grad_stride 31 is smaller than dim 32')
  case.cols[2]['stride'] = 33
  case.call(lr)
  case.check_result(lr, mode != 0)


@pytest.mark.parametrize('mode', [0, 1])
def test_adam_refusal_changes_nothing(hbk_option, mode):
  """Through the Adam entry: a dim-128 column with grad_out 4 bytes off beside a sort-path column
  (refused by the reduce of phase 1), and dim 68 with m 4 bytes off (refused by the apply's own
  check).  Nothing moves: w, m, v, n_unique, beta_powers; the realigned call then steps."""
  hbk_option('bwd_deterministic', mode)
  rng = np.random.RandomState(51)
  n = 300
  for dims, rows, g_shift, m_shift in (([4, 128], [BIG_ROWS, 700], 1, 0),
                                       ([4, 68], [BIG_ROWS, 900], 0, 1)):
    cols = (_lib.LookupGradColumn * 2)()
    state, m_ptrs, v_ptrs = [], [], []
    for c, d in enumerate(dims):
      w = torch.zeros(rows[c], d, device=DEV)
      mbuf = torch.zeros(rows[c] * d + 4, device=DEV)
      m = mbuf[m_shift if c == 1 else 0:][:rows[c] * d].view(rows[c], d)
      v = torch.zeros(rows[c], d, device=DEV)
      ids = dev(rng.randint(0, rows[c], size=n).astype(np.int64))
      gbuf = torch.zeros(n * d + 4, device=DEV)
      g = gbuf[g_shift if c == 1 else 0:][:n * d].view(n, d)
      g.copy_(dev(rng.randn(n, d).astype(F32)))
      nu = torch.full((1,), -7, dtype=torch.int32, device=DEV)
      state.append(dict(w=w, m=m, v=v, ids=ids, g=g, nu=nu, keep=(mbuf, gbuf)))
      col = cols[c]
      col.table, col.rows, col.dim, col.ids_dtype = w.data_ptr(), rows[c], d, _lib.INT64
      col.ids, col.n_ids, col.n_segments, col.bucket, col.divisor = ids.data_ptr(), n, n, 0, 1
      col.grad_out, col.n_unique = g.data_ptr(), nu.data_ptr()
      m_ptrs.append(m.data_ptr())
      v_ptrs.append(v.data_ptr())
    powers = dev(np.array([B1, B2], F32))

    def watched():
      return [[host(x[st['ids']]) for x in (st['w'], st['m'], st['v'])] + [host(st['nu'])]
              for st in state]
    torch.cuda.synchronize()
    before = watched()
    with pytest.raises(_lib.InvalidArgumentError, match=f'column 1: dim {dims[1]} needs more than 64'):
      _lib.check(_adam_call(cols, 2, m_ptrs, v_ptrs, powers, 0.01))
    torch.cuda.synchronize()
    for c, (a, b) in enumerate(zip(watched(), before)):
      for name, x, y in zip(('w', 'm', 'v', 'n_unique'), a, b):
        np.testing.assert_array_equal(x, y, err_msg=f'{name} of column {c} after a refused call')
    np.testing.assert_array_equal(host(powers), np.array([B1, B2], F32))
    # realigned: the call goes through and steps every named row once
    if dims[1] == 68:
      fresh = torch.zeros(rows[1], 68, device=DEV)
      m_ptrs[1] = fresh.data_ptr()
    else:
      fresh = state[1]['g'].clone()
      cols[1].grad_out = fresh.data_ptr()
    _lib.check(_adam_call(cols, 2, m_ptrs, v_ptrs, powers, 0.01))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(powers), np.array([B1 * B1, B2 * B2], F32))
    for st in state:
      assert int(st['nu'].item()) == np.unique(host(st['ids'])).size
      assert (host(st['w'][st['ids']]) != 0).any()


# ---- 6. DenseFeatures with any column dims ------------------------------------------------------
DF_SPEC = [('a', 5003, 3, 'sum', False), ('b', 8, 16, 'mean', True), ('c', 7001, 128, 'sqrtn', True),
           ('d', 6007, 6, 'mean', True), ('e', 4001, 64, 'sum', False), ('f', 12, 1, 'sum', False),
           ('g', 3001, 32, 'sqrtn', False)]


def _df_data(rng, world, steps, batch):
  """Per step and rank: features and a gradient on a 1/16 grid.  Ragged mean segments hold 0, 1, 2
  or 4 ids and sqrtn segments 0, 1 or 4, so every per-id term and every row sum is exact in fp32
  in any order: the reference is exact."""
  width = sum(d for _, _, d, _, _ in DF_SPEC)
  data = []
  for _ in range(steps):
    per_rank = []
    for _ in range(world):
      feats = {}
      for key, nb, _, comb, rag in DF_SPEC:
        if rag:
          sp = ragged(rng, batch, (0, 1, 2, 4) if comb == 'mean' else (0, 1, 4))
          feats[key] = (rng.randint(0, 1 << 40, size=int(sp[-1])).astype(np.int64), sp)
        else:
          feats[key] = rng.randint(0, 1 << 40, size=batch).astype(np.int64)
      per_rank.append((feats, (rng.randint(-64, 65, size=(batch, width)) / 16.0).astype(F32)))
    data.append(per_rank)
  return data


def _df_terms(key, comb, feats, g):
  f = feats[key]
  ids, sp = f if isinstance(f, tuple) else (f, np.arange(f.size + 1, dtype=np.int32))
  return ids, oracle.segment_combine_grad(g, sp, comb)


@pytest.mark.parametrize('world', [1, 2])
@pytest.mark.parametrize('optimizer', ['sgd', 'adagrad', 'adam'])
def test_dense_features_any_column_dims(world, optimizer):
  """Dims [3, 16, 128, 6, 64, 1, 32] in declaration order put the dim-128 column at float 19 and the
  dim-64 one at float 153 of the block: the forward equals float64 per column, and three steps
  equal the exact reference."""
  from tests.test_gpu_adam import _df_world
  steps, lr, batch = 3, 0.05, 256
  rng = np.random.RandomState(900 + world)
  cols = [hb.feature_column.EmbeddingColumn(k, nb, d, comb, hot_rows=False)
          for k, nb, d, comb, _ in DF_SPEC]
  tables = [rng.uniform(-1, 1, size=(nb, d)).astype(F32) for _, nb, d, _, _ in DF_SPEC]
  data = _df_data(rng, world, steps, batch)
  offs = np.concatenate([[0], np.cumsum([d for _, _, d, _, _ in DF_SPEC])])

  def fn(r, coll, barrier):
    def init(c, rows, d):
      t = tables[cols.index(c)]
      return dev((t[r::world] if rows != c.num_buckets else t).copy())
    layer = hb.feature_column.DenseFeatures(
      cols, DEV, coll=coll, batch_size=batch, init=init,
      initial_accumulator_value=0.1 if optimizer == 'adagrad' else None,
      optimizer='adam' if optimizer == 'adam' else None)
    fwd = []
    for s in range(steps):
      feats, g = data[s][r]
      d_feats = {k: (dev(v[0]), dev(v[1])) if isinstance(v, tuple) else dev(v) for k, v in feats.items()}
      out = layer(d_feats)
      fwd.append(host(out))
      layer.backward(dev(g), apply_lr=lr, optimizer=optimizer)
    st = ([host(w) for w in layer.weights], list(layer.sharded))
    layer.close()
    return fwd, st
  results = _df_world(world, fn)

  w = [t.copy() for t in tables]
  acc = [np.full_like(t, 0.1) for t in tables]
  m = [np.zeros_like(t) for t in tables]
  v = [np.zeros_like(t) for t in tables]
  p = (B1, B2)
  for s in range(steps):
    # forward of every rank against float64 of the tables before this step
    for r in range(world):
      got = results[r][0][s]
      assert got.shape == (batch, offs[-1])
      for k, (key, nb, d, comb, _) in enumerate(DF_SPEC):
        f = data[s][r][0][key]
        ids, sp = f if isinstance(f, tuple) else (f, None)
        spec = dict(ids=ids, splits=sp, bucket=nb, div=1, rows=nb, dim=d, comb=comb, w=None, table=w[k])
        want, mag = _fwd_f64(spec)
        assert_sums_close(got[:, offs[k]:offs[k + 1]], want, mag, err_msg=f'step {s} rank {r} {key}')
    for k, (key, nb, d, comb, _) in enumerate(DF_SPEC):
      if world > 1 and nb <= 256:
        continue   # replicated at W > 1: the caller aggregates and applies
      ids, terms = [], []
      for r in range(world):
        i, t = _df_terms(key, comb, data[s][r][0], data[s][r][1][:, offs[k]:offs[k + 1]])
        ids.append(i)
        terms.append(t)
      rows = np.concatenate(ids) % nb
      uniq = np.unique(rows)
      sums = oracle.unsorted_segment_sum(np.concatenate(terms), np.searchsorted(uniq, rows).astype(np.int32),
                                         uniq.size)
      if optimizer == 'sgd':
        oracle.sparse_sgd_apply(w[k], uniq, sums, lr)
      elif optimizer == 'adagrad':
        oracle.sparse_adagrad_apply(w[k], acc[k], uniq, sums, lr)
      else:
        np_adam(w[k], m[k], v[k], uniq, sums, lr, p[0], p[1])
    p = (F32(p[0] * B1), F32(p[1] * B2))
  for k, (key, nb, d, _, _) in enumerate(DF_SPEC):
    parts = [res[1][0][k] for res in results]
    if world > 1 and results[0][1][1][k]:
      got = np.empty((nb, d), F32)
      for q in range(world):
        got[q::world] = parts[q]
    else:
      got = parts[0]
    np.testing.assert_array_equal(got, w[k], err_msg=f'table {key} (dim {d}) after {steps} steps')
