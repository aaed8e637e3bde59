"""The id and wire primitives at the boundaries of their kernel paths, bit for bit against the plain
restatements of tests/support/primitives_ref.py (which tests/test_primitives_ref.py holds to the C oracle):

  hbk_cast_n        both kernels (16-byte aligned -> vector, anything else -> scalar) on every rounding
                    decision of fp32 -> fp16 and every fp16 bit pattern; lengths around the 8-element group and
                    the 2048-element tile at every misalignment, inside sentinel-filled buffers; more than
                    128 tensors (two launches)
  hbk_floormod_n    divisors up to 2^63 - 1 on the device, 130 columns in one call
  hbk_unique_n      more than 96 columns (second chunk), repeats and first occurrences across every tile edge,
                    forced bucket counts around the one-launch limit, an LDS table filled exactly / overflowing
                    under the default options
  cache probe       full tables, one slab, one slot, keys behind EMPTY slots, duplicates, all hits / all
                    misses, key counts at the compaction tile and at the keys-per-block edge
  hbk_alltoallv_n   W = 2, 3, 5 in-process ranks, several columns, zero sizes, fp16 wire on unaligned views

Where the expected value is a NaN the result must be a NaN of the same sign; everything else is exact.
"""
import functools
import threading

import numpy as np
import pytest
import torch

import hybridbackend_amd as hb
from hybridbackend_amd import _lib
from tests.support import primitives_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------
# casts
_BITS = {np.dtype(np.float32): (np.uint32, np.int32, 0xdeadbeef),
         np.dtype(np.float16): (np.uint16, np.int16, 0xbeef)}


def _layout(lens, offs):
  """Windows inside one buffer: window k starts `offs[k]` elements past a 64-element boundary (256 bytes of
  fp32, 128 of fp16) and is followed by at least 16 guard elements."""
  starts, pos = [], 64
  for n, o in zip(lens, offs):
    starts.append(pos + o)
    pos += -(-(o + n + 16) // 64) * 64
  return starts, pos


def _cast_call(to_half, arrays, in_offs, out_offs):
  """One hbk_cast_n call over windows of two flat buffers; every output element outside the windows must
  keep its sentinel.  Returns the output windows."""
  src_t, dst_t = (np.float32, np.float16) if to_half else (np.float16, np.float32)
  ubits_s, ibits_s, _ = _BITS[np.dtype(src_t)]
  ubits_d, ibits_d, sentinel = _BITS[np.dtype(dst_t)]
  lens = [int(a.size) for a in arrays]
  in_starts, in_total = _layout(lens, in_offs)
  out_starts, out_total = _layout(lens, out_offs)
  src = np.zeros(in_total, ubits_s)
  for a, s in zip(arrays, in_starts):
    assert a.dtype == src_t
    src[s:s + a.size] = a.view(ubits_s)
  d_src = dev(src.view(ibits_s))
  d_dst = dev(np.full(out_total, sentinel, ubits_d).view(ibits_d))
  assert d_src.data_ptr() % 256 == 0 and d_dst.data_ptr() % 256 == 0
  isz, osz = np.dtype(src_t).itemsize, np.dtype(dst_t).itemsize
  lib = _lib.lib()
  _lib.check(lib.hbk_cast_n(
    len(arrays), _lib.FLOAT if to_half else _lib.HALF, _lib.HALF if to_half else _lib.FLOAT,
    _lib.ptr_array([d_src.data_ptr() + s * isz for s in in_starts]), _lib.i64_array(lens),
    _lib.ptr_array([d_dst.data_ptr() + s * osz for s in out_starts]), _lib.current_stream()))
  out = host(d_dst).view(ubits_d)
  outside = np.ones(out_total, bool)
  for n, s in zip(lens, out_starts):
    outside[s:s + n] = False
  touched = np.where(outside & (out != sentinel))[0]
  assert touched.size == 0, ('written outside the windows', touched[:8].tolist(), out_starts[:4])
  return [out[s:s + n].view(dst_t) for n, s in zip(lens, out_starts)]


def _reference_cast(to_half, a):
  return ref.cast_f32_to_f16(a) if to_half else ref.cast_f16_to_f32(a)


@pytest.mark.parametrize('to_half', [True, False], ids=['f32_to_f16', 'f16_to_f32'])
def test_cast_values_through_both_kernels(to_half):
  x = ref.f32_rounding_edges() if to_half else ref.f16_all_bit_patterns()
  want = _reference_cast(to_half, x)
  vec = _cast_call(to_half, [x], [0], [0])[0]          # 16-byte aligned: cast_vec_kernel
  sca = _cast_call(to_half, [x], [1], [1])[0]          # from element 1 of a buffer: ew_kernel
  ref.assert_same_bits(vec, want, 'vector kernel')
  ref.assert_same_bits(sca, want, 'scalar kernel')
  ubits = _BITS[vec.dtype][0]
  np.testing.assert_array_equal(vec.view(ubits), sca.view(ubits))   # two expressions, one rounding


def _layout_arrays(to_half, lens, seed=0):
  arrays = []
  for k, n in enumerate(lens):
    v = ref.cast_layout_values(seed + k, n)
    arrays.append(v if to_half else ref.cast_f32_to_f16(v))
  return arrays


def _check_cast(to_half, arrays, f32_offs, f16_offs):
  in_offs, out_offs = (f32_offs, f16_offs) if to_half else (f16_offs, f32_offs)
  outs = _cast_call(to_half, arrays, in_offs, out_offs)
  for k, (a, o) in enumerate(zip(arrays, outs)):
    ref.assert_same_bits(o, _reference_cast(to_half, a), 'tensor %d of %d elements' % (k, a.size))


@pytest.mark.parametrize('to_half', [True, False], ids=['f32_to_f16', 'f16_to_f32'])
def test_cast_layout_every_length_at_every_misalignment(to_half):
  prod = ref.cast_layout_product()
  assert len(prod) == 144                               # two launches of 128 and 16 tensors
  _check_cast(to_half, _layout_arrays(to_half, [n for n, _, _ in prod]),
              [a for _, a, _ in prod], [b for _, _, b in prod])


@pytest.mark.parametrize('to_half', [True, False], ids=['f32_to_f16', 'f16_to_f32'])
@pytest.mark.parametrize('case', ['aligned', 'last_misaligned', 'empty_tensors'])
def test_cast_130_tensors_two_launches(to_half, case):
  nonzero = [n for n in ref.CAST_LENGTHS if n]
  lens = [nonzero[k % len(nonzero)] for k in range(130)]
  f32_offs, f16_offs = [0] * 130, [0] * 130
  if case == 'last_misaligned':                         # first launch vector, second scalar
    f32_offs[129], f16_offs[129] = 1, 4
  if case == 'empty_tensors':
    for k in (0, 127, 128, 129):
      lens[k] = 0
  _check_cast(to_half, _layout_arrays(to_half, lens, seed=1000), f32_offs, f16_offs)


# ----------------------------------------------------------------------------------------------
# floormod
@pytest.mark.parametrize('dtype,code', [(np.int64, _lib.INT64), (np.int32, _lib.INT32)], ids=['int64', 'int32'])
def test_floormod_n_wide_divisors_130_columns(dtype, code):
  cols = ref.floormod_columns(dtype)
  ins = [dev(x) for x, _ in cols]
  outs = [torch.full_like(t, -7) for t in ins]
  _lib.check(_lib.lib().hbk_floormod_n(
    len(cols), code, _lib.ptr_array([t.data_ptr() for t in ins]),
    _lib.i64_array([t.numel() for t in ins]), _lib.i64_array([d for _, d in cols]),
    _lib.ptr_array([t.data_ptr() for t in outs]), _lib.current_stream()))
  for c, ((x, d), o) in enumerate(zip(cols, outs)):
    np.testing.assert_array_equal(host(o), ref.floormod(x, d), err_msg='column %d, divisor %d' % (c, d))


# ----------------------------------------------------------------------------------------------
# unique
@functools.lru_cache(maxsize=None)
def _unique_expected(kind, arg=None):
  """(columns, expected (unique, index) per column) of one generated input, computed once."""
  if kind == 'many':
    cols = ref.unique_many_columns(arg, arg)
  elif kind == 'all_empty':
    cols = ref.unique_many_columns(97, 1, all_empty=True)
  elif kind == 'boundary':
    cols = [x for _, x in ref.unique_boundary_columns()]
  elif kind == 'buckets':
    cols = ref.unique_bucket_option_columns(arg)
  else:
    cols = [ref.unique_skew_column(n) for n in ref.UNIQUE_SKEW_KEYS]
  return cols, [ref.unique_first_occurrence(x) for x in cols]


def _check_unique(res, expected, what=''):
  counts = host(torch.cat([nu for _, _, nu in res])).tolist()
  for c, ((u, idx, _), (wu, widx)) in enumerate(zip(res, expected)):
    assert counts[c] == wu.size, (what, c, counts[c], wu.size)
    np.testing.assert_array_equal(host(u)[:wu.size], wu, err_msg='%s column %d: unique' % (what, c))
    np.testing.assert_array_equal(host(idx), widx, err_msg='%s column %d: index' % (what, c))


def _unique_three_calls(kind, arg=None):
  cols, expected = _unique_expected(kind, arg)
  d_cols = [dev(x) for x in cols]
  for rep in range(3):                                  # (the sync words of the one-launch form alternate)
    _check_unique(hb.embedding.unique_n(d_cols), expected, '%s call %d' % (kind, rep))


@pytest.mark.parametrize('onepass', [1, 0])
@pytest.mark.parametrize('n_cols', [96, 97, 200])
def test_unique_more_columns_than_one_launch(hbk_option, n_cols, onepass):
  hbk_option('unique_onepass', onepass)
  _unique_three_calls('many', n_cols)
  if n_cols == 97:
    _unique_three_calls('all_empty')


@pytest.mark.parametrize('onepass', [1, 0])
def test_unique_repeats_across_tile_edges(hbk_option, onepass):
  hbk_option('unique_onepass', onepass)
  _unique_three_calls('boundary')


@pytest.mark.parametrize('onepass', [1, 0])
@pytest.mark.parametrize('log2p', ref.UNIQUE_BUCKETS_LOG2)
def test_unique_forced_bucket_counts(hbk_option, log2p, onepass):
  hbk_option('unique_onepass', onepass)
  hbk_option('unique_buckets_log2', log2p)
  _unique_three_calls('buckets', log2p)


@pytest.mark.parametrize('onepass', [1, 0])
def test_unique_one_bucket_fills_and_overflows_the_lds_table(hbk_option, onepass):
  # default bucket count: the keys were chosen to share the top bits of the mix
  hbk_option('unique_onepass', onepass)
  _unique_three_calls('skew')


def test_unique_bound_plan_over_97_columns():
  cols, expected = _unique_expected('many', 97)
  d_cols = [dev(x) for x in cols]
  plan = hb.embedding.UniqueN()
  _check_unique(plan(d_cols), expected, 'bound')
  refill = ref.unique_many_columns(97, 4242)
  big = max(range(97), key=lambda c: cols[c].size)
  fresh = np.resize(np.concatenate([refill[c] for c in range(97)]), cols[big].size)
  d_cols[big].copy_(dev(fresh))                        # refilled in place: same binding, new answer
  expected = list(expected)
  expected[big] = ref.unique_first_occurrence(fresh)
  _check_unique(plan(d_cols), expected, 'bound, refilled')


# ----------------------------------------------------------------------------------------------
# cache probe
@pytest.mark.parametrize('slab_size', ref.PROBE_SLAB_SIZES)
def test_cache_probe_and_lookup_tables_and_key_counts(slab_size):
  for slab_count in ref.PROBE_SLAB_COUNTS:
    for name, cache, must in ref.probe_tables(slab_size, slab_count):
      universe = ref.probe_universe(cache, must, 5)
      want_all = ref.cache_probe(cache, slab_size, universe)
      d_cache = dev(cache)
      for sel_name, sel in ref.probe_selections(want_all, slab_size).items():
        what = '%s, %d slabs of %d, %s' % (name, slab_count, slab_size, sel_name)
        keys, want = universe[sel], want_all[sel]
        d_keys = dev(keys)
        hit_slot, n_miss = hb.embedding.cache.probe(d_cache, d_keys, slab_size)
        np.testing.assert_array_equal(host(hit_slot), want, err_msg=what)
        assert int(n_miss.item()) == int((want < 0).sum()), what
        got = hb.embedding.cache.lookup(d_cache, d_keys, slab_size)
        w_hk, w_hc, w_mk, w_mkeys, w_counts = ref.cache_lists(want, keys)
        assert [got[0].numel(), got[2].numel()] == w_counts.tolist(), what     # counts
        for g, w in zip(got, (w_hk, w_hc, w_mk, w_mkeys)):
          assert host(g).dtype == w.dtype, what
          np.testing.assert_array_equal(host(g), w, err_msg=what)


# ----------------------------------------------------------------------------------------------
# alltoallv over in-process ranks
def _run_ranks(world, fn):
  comms = hb.distribute.Collective.local_world(world)
  results, errors = [None] * world, []

  def run(r):
    try:
      with torch.cuda.stream(torch.cuda.Stream()):
        results[r] = fn(r, comms[r])
        torch.cuda.current_stream().synchronize()
    except Exception as e:  # pylint: disable=broad-except
      errors.append((r, repr(e)))

  threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=45)
  for c in comms:
    c.close()
  assert not errors, errors
  return results


_A2A = {'f32': (np.float32, None), 'f16wire': (np.float32, torch.float16), 'i64': (np.int64, None),
        'i32': (np.int32, None)}
_SEND_OFF, _RECV_OFF, _GUARD = 1, 3, 16     # views start 1 and 3 elements into their buffers


def _sentinel_like(dtype, n):
  if np.dtype(dtype).kind == 'f':
    return np.full(n, 0xdeadbeef, np.uint32).view(np.float32)
  return np.full(n, -0x5a5a5a5a, dtype)


def _bits(a):
  return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize('kind', ['f32', 'f16wire', 'i64', 'i32'])
@pytest.mark.parametrize('world', ref.ALLTOALLV_WORLDS)
def test_alltoallv_n_columns_sizes_and_wire(world, kind):
  dtype, wire = _A2A[kind]
  cases = []
  for n_cols in (1, 2, 3, 4):
    sizes = ref.alltoallv_sizes(world, n_cols, 7)
    commons = [ref.ALLTOALLV_COMMON[(c + n_cols) % 4] for c in range(n_cols)]
    vals = [[ref.alltoallv_values(kind, int(sizes[c, r].sum()) * commons[c], 1000 * n_cols + 10 * c + r)
             for r in range(world)] for c in range(n_cols)]
    want, want_sizes = [], []
    for c in range(n_cols):
      w, ws = ref.alltoallv(vals[c], sizes[c], commons[c])
      if wire is not None:
        w = [ref.cast_f16_to_f32(ref.cast_f32_to_f16(x)) for x in w]
      want.append(w)
      want_sizes.append(ws)
    cases.append((sizes, commons, vals, want, want_sizes))

  def fn(r, coll):
    got = []
    for sizes, commons, vals, want, want_sizes in cases:
      n_cols = len(commons)
      recv = coll.alltoall_n([dev(sizes[c, r].astype(np.int32)) for c in range(n_cols)])
      torch.cuda.current_stream().synchronize()
      recv = [host(x).tolist() for x in recv]
      assert recv == [want_sizes[c][r].tolist() for c in range(n_cols)], ('recv_sizes', r, recv)
      values, out_bufs, out_views = [], [], []
      for c in range(n_cols):
        send = _sentinel_like(dtype, _SEND_OFF + vals[c][r].size + _GUARD)
        send[_SEND_OFF:_SEND_OFF + vals[c][r].size] = vals[c][r]
        n = vals[c][r].size
        values.append(dev(send)[_SEND_OFF:_SEND_OFF + n].view(n // commons[c], commons[c]))
        m = want[c][r].size
        out_bufs.append(dev(_sentinel_like(dtype, _RECV_OFF + m + _GUARD)))
        out_views.append(out_bufs[c][_RECV_OFF:_RECV_OFF + m].view(m // commons[c], commons[c]))
      coll.alltoallv_n(values, [sizes[c, r].tolist() for c in range(n_cols)], recv, common_sizes=commons,
                       wire_dtype=wire, outs=out_views)
      torch.cuda.current_stream().synchronize()
      got.append([host(b) for b in out_bufs])
    return got

  res = _run_ranks(world, fn)
  for k, (sizes, commons, vals, want, want_sizes) in enumerate(cases):
    for r in range(world):
      for c in range(len(commons)):
        m = want[c][r].size
        expect = _sentinel_like(dtype, _RECV_OFF + m + _GUARD)
        expect[_RECV_OFF:_RECV_OFF + m] = want[c][r]
        np.testing.assert_array_equal(_bits(res[r][k][c]), _bits(expect),
                                      err_msg='%d columns, rank %d, column %d' % (len(commons), r, c))
