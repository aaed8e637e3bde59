"""hbk_hash_translate_runs_n on the GPU: for plain, expiring and filtered tables the runs entry is compared with
the matching existing entry called once on the concatenation of the runs, on twin tables.  Slot numbers are
run-dependent; everything else -- the key set of every slab (no slab overflows here), counts, stats, freq and
last_seen per key, the sketch -- must be equal."""
import numpy as np
import pytest
import torch

from hybridbackend_amd.embedding import HashTable
from hybridbackend_amd.embedding import hashtable as _ht
from tests.support import hash_ref as ref
from tests.support.hash_lifecycle import translate_runs
from tests.support.sharded_hash_ref import keys_without_overflow

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GEOMETRY = [(5, 60, 4), (16, 20, 6)]      # (slab_size, slab_count, dim): 300 and 320 slots


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
  return t.cpu().numpy()


def make_tables(kind, min_freq=2):
  return [HashTable(ss * sc, dim, DEV, slab_size=ss, init_scale=0.05, seed=3 + c, expiring='expiring' in kind,
                    min_freq=min_freq if 'admit' in kind else 0, sketch_width=4096)
          for c, (ss, sc, dim) in enumerate(GEOMETRY)]


def draw_runs(rng, pools):
  """Three runs per table: 120 and 90 draws that share keys, an empty run between them."""
  return [[p[rng.randint(0, p.size, size=120)], np.zeros(0, np.int64), p[rng.randint(0, p.size, size=90)]]
          for p in pools]


def per_key(table, array, keys):
  slots = host(table.find(dev(keys)))
  assert (slots >= 0).all()
  return host(array)[slots]


def assert_twins_equal(a, b, keys):
  """Table a (runs entry) against table b (the existing entry on the concatenation); keys: those stored."""
  assert ref.slab_sets(host(a.keys), a.slab_size) == ref.slab_sets(host(b.keys), b.slab_size)
  assert host(a.counts).tolist() == host(b.counts).tolist()
  np.testing.assert_array_equal(per_key(a, a.table, keys), per_key(b, b.table, keys))
  np.testing.assert_array_equal(per_key(a, a.table, keys), ref.init_rows(keys, a.dim, a.seed, a.init_scale))
  if a.expiring:
    assert host(a.stats).tolist() == host(b.stats).tolist()
    np.testing.assert_array_equal(per_key(a, a.freq, keys), per_key(b, b.freq, keys))
    np.testing.assert_array_equal(per_key(a, a.last_seen, keys), per_key(b, b.last_seen, keys))
  if a.min_freq:
    np.testing.assert_array_equal(host(a.sketch), host(b.sketch))
    assert host(a.filter_counts).tolist() == host(b.filter_counts).tolist()


@pytest.mark.parametrize('kind', ['plain', 'expiring', 'admit', 'expiring_admit'])
def test_runs_entry_equals_the_matching_entry_on_the_concatenation(kind):
  rng = np.random.RandomState(len(kind))
  pools = [keys_without_overflow(rng, 150, sc, ss, extra=(-1, 0, 2 ** 63 - 1)) for ss, sc, _ in GEOMETRY]
  A, B = make_tables(kind), make_tables(kind)
  for step, sub in ((3, slice(0, 100)), (5, slice(50, 150))):      # the second call meets old keys and new ones
    runs = draw_runs(rng, [p[sub] for p in pools])
    if 'expiring' in kind:
      for t in A + B:
        t.set_step(step)
    got = translate_runs(A, [[dev(i) for i in r] for r in runs])
    whole = [np.concatenate(r) for r in runs]
    want = _ht.hash_translate(B, [dev(w) for w in whole])
    for c in range(2):
      s = np.concatenate([host(x) for x in got[c]])
      stored = s >= 0
      # every answer names a slot that holds its key; the same occurrences are answered -1 (the filter's
      # decision is reproducible, and nothing fails: capacity >= the distinct keys)
      np.testing.assert_array_equal(host(A[c].keys)[s[stored]], whole[c][stored])
      np.testing.assert_array_equal(stored, host(want[c]) >= 0)
      if 'admit' not in kind:
        assert stored.all()
      assert A[c].failed() == 0
      assert_twins_equal(A[c], B[c], np.unique(whole[c][stored]))
      if 'expiring' in kind:
        # freq per key = its occurrences so far that resolved to a slot; last_seen = this step
        k = np.unique(whole[c][stored])
        assert (per_key(A[c], A[c].last_seen, k) == step).all()


@pytest.mark.parametrize('kind', ['admit', 'expiring_admit'])
def test_an_id_once_in_each_of_two_runs_is_admitted_by_that_call(kind):
  rng = np.random.RandomState(11)
  pools = [keys_without_overflow(rng, 90, sc, ss) for ss, sc, _ in GEOMETRY]
  A = make_tables(kind, min_freq=2)
  for t in A:
    if t.expiring:
      t.set_step(1)
  runs, twice, once = [], [], []
  for p in pools:
    both, single = p[:40], p[40:]
    r0, r2 = np.concatenate([both, single[:25]]), np.concatenate([both, single[25:]])
    rng.shuffle(r0)
    rng.shuffle(r2)
    runs.append([r0, np.zeros(0, np.int64), r2])
    twice.append(both)
    once.append(single)
  got = translate_runs(A, [[dev(i) for i in r] for r in runs])
  for c in range(2):
    for k in (0, 2):
      s, ids = host(got[c][k]), runs[c][k]
      seen_twice = np.isin(ids, twice[c])
      assert (s[seen_twice] >= 0).all() and (s[~seen_twice] == -1).all()
      np.testing.assert_array_equal(host(A[c].keys)[s[seen_twice]], ids[seen_twice])
    assert A[c].size() == twice[c].size and A[c].filtered() == once[c].size and A[c].failed() == 0
    assert (host(A[c].estimate(dev(once[c]))) >= 1).all()


@pytest.mark.parametrize('kind', ['plain', 'expiring', 'admit', 'expiring_admit'])
def test_a_find_inserts_nothing_and_nothing_to_do_is_accepted(kind):
  rng = np.random.RandomState(5)
  pools = [keys_without_overflow(rng, 60, sc, ss) for ss, sc, _ in GEOMETRY]
  A = make_tables(kind, min_freq=1)
  runs = draw_runs(rng, pools)
  d_runs = [[dev(i) for i in r] for r in runs]
  before = [(host(t.keys), host(t.table), host(t.counts)) for t in A]
  got = translate_runs(A, d_runs, insert=False)
  for c, t in enumerate(A):
    assert all((host(s) == -1).all() for s in got[c])
    for x, y in zip(before[c], (host(t.keys), host(t.table), host(t.counts))):
      np.testing.assert_array_equal(x, y)
    if t.min_freq:
      assert not host(t.sketch).any()
  # after an insert the find answers what the insert answered
  first = translate_runs(A, d_runs)
  again = translate_runs(A, d_runs, insert=False)
  for c in range(2):
    for x, y in zip(first[c], again[c]):
      np.testing.assert_array_equal(host(x), host(y))
  # no runs, runs without keys, no columns
  size = [t.size() for t in A]
  assert translate_runs(A, [[], []]) == [[], []]
  translate_runs(A, [[dev(np.zeros(0, np.int64))] * 2, []])
  assert translate_runs([], []) == []
  assert [t.size() for t in A] == size
