"""Weighted lookups (tf.nn.embedding_lookup_sparse's sp_weights) at the C ABI, without a GPU: the
structs end in id_weights with the C layout, the version says so, and every refused combination is
refused before any device work with the field named."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hybridbackend_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7f0000001000      # a device-looking address: validation must refuse before touching it

_PROBE = r'''
#include <stddef.h>
#include <stdio.h>
#include "hbk.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n",
         sizeof(hbk_lookup_column_t), offsetof(hbk_lookup_column_t, id_weights),
         sizeof(hbk_lookup_grad_column_t), offsetof(hbk_lookup_grad_column_t, id_weights),
         sizeof(hbk_stitch_grad_column_t), offsetof(hbk_stitch_grad_column_t, id_weights));
  return 0;
}
'''


def _c_layout(tmp_path):
  src = tmp_path / 'layout.c'
  src.write_text(_PROBE)
  exe = tmp_path / 'layout'
  for cc in ('cc', 'gcc', 'clang', '/opt/rocm/llvm/bin/clang'):
    try:
      subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
      break
    except (OSError, subprocess.CalledProcessError):
      continue
  else:
    pytest.skip('no C compiler')
  return [int(x) for x in subprocess.check_output([str(exe)]).split()]


def test_structs_end_in_id_weights_with_the_c_layout(tmp_path):
  sizes = _c_layout(tmp_path)
  for k, cls in enumerate((_lib.LookupColumn, _lib.LookupGradColumn, _lib.StitchGradColumn)):
    assert cls._fields_[-1][0] == 'id_weights'
    assert C.sizeof(cls) == sizes[2 * k], cls
    assert cls.id_weights.offset == sizes[2 * k + 1], cls
    assert cls().id_weights is None     # (ctypes zero-fills: unweighted unless set)


def test_version_and_new_symbols():
  import hybridbackend_amd
  lib = _lib.lib()
  assert lib.hbk_version().decode() == 'hbk 0.2.0 gfx950'
  assert hybridbackend_amd.__version__ == '0.2.0'
  assert hasattr(lib, 'hbk_sharded_lookup_fwd_weighted')


def _fwd_col(**kw):
  col = _lib.LookupColumn()
  col.table, col.rows, col.dim = FAKE, 100, 16
  col.ids_dtype, col.ids, col.n_ids, col.n_segments = _lib.INT64, FAKE, 8, 8
  col.divisor, col.combiner, col.out = 1, _lib.COMBINER_MEAN, FAKE
  col.id_weights = FAKE
  for k, v in kw.items():
    setattr(col, k, v)
  return col


def _refused(rc, *words):
  msg = _lib.lib().hbk_last_error().decode()
  assert rc == _lib.INVALID_ARGUMENT, (rc, msg)
  for w in words:
    assert w in msg, msg


def test_forward_refusals():
  lib = _lib.lib()
  cols = (_lib.LookupColumn * 1)(_fwd_col(out_slots=FAKE))
  _refused(lib.hbk_group_lookup_fwd(1, cols, None), 'id_weights', 'out_slots')
  cols = (_lib.LookupColumn * 1)(_fwd_col(half_io=1))
  _refused(lib.hbk_group_lookup_fwd(1, cols, None), 'id_weights', 'HBK_LOOKUP_OUT_HALF')
  # an unweighted column with the same settings passes validation (out_slots) -- the refusal is
  # about the weights; nothing launches: another column of the call is invalid
  cols = (_lib.LookupColumn * 2)(_fwd_col(out_slots=FAKE, id_weights=None), _fwd_col(dim=0))
  _refused(lib.hbk_group_lookup_fwd(2, cols, None), 'dim')


def test_backward_refusal_with_segmented_inputs():
  lib = _lib.lib()
  col = _lib.LookupGradColumn()
  col.table, col.rows, col.dim = FAKE, 100, 16
  col.ids_dtype, col.ids, col.n_ids, col.n_segments = _lib.INT64, FAKE, 8, 8
  col.divisor, col.combiner, col.grad_out = 1, _lib.COMBINER_SUM, FAKE
  col.unique_rows, col.grad_rows, col.n_unique = FAKE, FAKE, FAKE
  col.run_start, col.run_ids, col.run_grads, col.n_runs = FAKE, FAKE, FAKE, 2
  col.id_weights = FAKE
  cols = (_lib.LookupGradColumn * 1)(col)
  _refused(lib.hbk_group_lookup_bwd_apply(1, cols, _lib.APPLY_SGD, C.c_float(0.0), C.c_void_p(FAKE),
                                          C.c_size_t(1 << 30), None), 'id_weights', 'run_')


def test_backward_workspace_counts_the_term_buffers():
  lib = _lib.lib()
  col = _lib.LookupGradColumn()
  col.rows, col.dim, col.ids_dtype, col.n_ids, col.n_segments = 1000, 12, _lib.INT64, 777, 300
  col.row_splits, col.divisor, col.combiner = FAKE, 1, _lib.COMBINER_MEAN
  col.unique_rows, col.grad_rows, col.n_unique = FAKE, FAKE, FAKE
  plain = lib.hbk_group_lookup_bwd_workspace_bytes(1, (_lib.LookupGradColumn * 1)(col))
  col.id_weights = FAKE
  weighted = lib.hbk_group_lookup_bwd_workspace_bytes(1, (_lib.LookupGradColumn * 1)(col))
  # the weighted column is reduced as one of 777 one-id SUM segments behind its [777, 12] terms
  col2 = _lib.LookupGradColumn.from_buffer_copy(col)
  col2.id_weights, col2.row_splits, col2.n_segments, col2.combiner = None, None, 777, _lib.COMBINER_SUM
  as_sum = lib.hbk_group_lookup_bwd_workspace_bytes(1, (_lib.LookupGradColumn * 1)(col2))
  terms = (777 * 12 * 4 + 15) // 16 * 16 + 16
  assert weighted == terms + as_sum
  assert plain > 0


def test_python_refusals_without_a_gpu():
  from hybridbackend_amd.embedding import sharded
  bound = sharded._BoundStep()
  bound.weights = (None, [object()])
  with pytest.raises(_lib.InvalidArgumentError, match='sp_weights'):
    sharded.ShardedGroupLookup.launch_begin(None, bound)
  pipe = sharded.PipelinedLookup.__new__(sharded.PipelinedLookup)
  pipe.plans = [None]
  with pytest.raises(_lib.InvalidArgumentError, match='PipelinedLookup'):
    pipe.bind(0, [np.zeros(1)], sp_weights=[np.zeros(1)])
  # p2p-bound object: refused in Python before the driver (whose own refusal is HBK_UNIMPLEMENTED)
  drv = sharded.ShardedGroupLookup.__new__(sharded.ShardedGroupLookup)
  drv._p2p_keep = [object()]
  with pytest.raises(_lib.HbkError) as e:
    drv([np.zeros(1)], sp_weights=[np.zeros(1)])
  assert e.value.code == _lib.UNIMPLEMENTED
