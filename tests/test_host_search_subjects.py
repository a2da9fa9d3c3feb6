"""Host-side checks of the subject-labelled search (include/ffrnet.h: ffr_search_topk_subjects): the numpy restatement of
tests/search_subjects_ref.py against a second, naive per-probe loop, the shard argument on the restatement, subject_rates
against a naive CMC, and the Python surface that needs no device."""
import numpy as np
import pytest
import torch

import search_subjects_ref as ref
from ffrnet_amd import native, search


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
               for x, y in zip(a, b))


def _random_case(rng, Q, G, nsubj, removed, levels):
    """scores drawn from a few levels (so ties abound), subjects at random, a fraction removed"""
    S = rng.choice(np.linspace(-0.5, 0.9, levels).astype(np.float32), size=(Q, G))
    subj = rng.integers(0, nsubj, size=G).astype(np.int32)
    subj[rng.random(G) < removed] = -1
    return S, subj


def test_ref_equals_the_naive_loop_on_random_cases():
    rng = np.random.default_rng(1)
    for Q, G, nsubj, removed, levels in ((3, 40, 7, 0.0, 5), (4, 64, 20, 0.3, 9), (2, 17, 3, 0.5, 3), (5, 100, 100, 0.1, 50),
                                         (1, 1, 1, 0.0, 2), (2, 30, 4, 0.0, 1000)):
        S, subj = _random_case(rng, Q, G, nsubj, removed, levels)
        for k in (1, 5, 12):
            for distinct in (0, 1):
                for base in (0, 1000):
                    assert _same(ref.search_ref(S, subj, k, distinct, base), ref.search_naive(S, subj, k, distinct, base)), (
                        Q, G, k, distinct)


def test_ref_on_hand_made_cases():
    #            row:  0    1    2    3    4    5    6    7
    S = np.array([[0.5, 0.9, 0.9, 0.5, 0.9, 0.1, 0.5, 0.9]], dtype=np.float32)
    subj = np.array([4, 2, 2, 7, 3, 4, -1, 2], dtype=np.int32)
    # ties across subjects (rows 1, 4) and within one (rows 1, 2, 7): the smallest index speaks for a subject, tied subjects
    # order by that index; row 6 is removed
    s, i, u = ref.search_ref(S, subj, 3, 1)
    assert i.tolist() == [[1, 4, 0]] and u.tolist() == [[2, 3, 4]] and s.tolist() == [[np.float32(0.9), np.float32(0.9), 0.5]]
    s, i, u = ref.search_ref(S, subj, 8, 0, index_base=10)
    assert i.tolist() == [[11, 12, 14, 17, 10, 13, 15, -1]] and u.tolist() == [[2, 2, 3, 2, 4, 7, 4, -1]]
    assert s[0, 7] == -np.inf
    # fewer live subjects than k: padding
    s, i, u = ref.search_ref(S, subj, 6, 1)
    assert i.tolist() == [[1, 4, 0, 3, -1, -1]] and u.tolist() == [[2, 3, 4, 7, -1, -1]] and np.all(s[0, 4:] == -np.inf)
    # everything removed
    for distinct in (0, 1):
        s, i, u = ref.search_ref(S, np.full(8, -1, dtype=np.int32), 4, distinct)
        assert np.all(i == -1) and np.all(u == -1) and np.all(s == -np.inf)
        assert _same((s, i, u), ref.search_naive(S, np.full(8, -1), 4, distinct))
    # no removed row, row mode: the plain top-k
    s, i, u = ref.search_ref(S, np.arange(8), 4, 0)
    assert i.tolist() == [[1, 2, 4, 7]] and u.tolist() == [[1, 2, 4, 7]]
    assert s.dtype == np.float32 and i.dtype == np.int64 and u.dtype == np.int32


def test_merging_shard_lists_equals_one_search_on_the_ref():
    """The shard argument of the header: split G at arbitrary points, list every shard, merge the lists."""
    rng = np.random.default_rng(2)
    for trial in range(30):
        Q, G = 3, int(rng.integers(1, 90))
        S, subj = _random_case(rng, Q, G, int(rng.integers(1, 12)), float(rng.choice([0.0, 0.3])), int(rng.integers(2, 12)))
        k = int(rng.integers(1, 9))
        cuts = sorted(set([0, G] + [int(c) for c in rng.integers(0, G + 1, size=int(rng.integers(0, 5)))]))
        cuts = cuts + [G]                      # and an empty shard at the end
        for distinct in (0, 1):
            parts = [ref.search_ref(S[:, lo:hi], subj[lo:hi], k, distinct, index_base=lo)
                     for lo, hi in zip(cuts[:-1], cuts[1:])]
            merged = ref.merge_ref(*[np.stack([p[j] for p in parts]) for j in range(3)], distinct)
            assert _same(merged, ref.search_ref(S, subj, k, distinct)), (trial, distinct, cuts)


def test_subject_rates_against_a_naive_cmc():
    rng = np.random.default_rng(3)
    subj = rng.integers(-1, 6, size=(50, 10)).astype(np.int32)
    labels = rng.integers(0, 6, size=50)
    got = search.subject_rates(torch.from_numpy(subj), torch.from_numpy(labels), ranks=(1, 3, 10))
    want = ref.cmc_naive(subj, labels, (1, 3, 10))
    assert got == pytest.approx(want, abs=1e-12) and set(got) == {1, 3, 10}
    # padding never hits, not even a label of -1
    pad = torch.full((4, 5), -1, dtype=torch.int32)
    assert search.subject_rates(pad, torch.full((4,), -1), ranks=(1, 5)) == {1: 0.0, 5: 0.0}
    assert search.subject_rates(torch.empty((0, 5), dtype=torch.int32), torch.empty((0,), dtype=torch.int64)) == {
        1: 0.0, 5: 0.0, 10: 0.0}


def test_python_surface():
    names = {n for n, _, _ in native.SYMBOLS}
    assert {'ffr_search_topk_subjects', 'ffr_topk_merge_subjects'} <= names
    for fn in ('search_subjects', 'topk_merge_subjects'):
        assert callable(getattr(native.Engine, fn))
    for fn in ('search_subjects', 'remove', 'compact', 'subjects'):
        assert hasattr(search.Gallery, fn)
    import inspect
    assert list(inspect.signature(search.search_sharded).parameters) == ['gallery_shard', 'query', 'k', 'group', 'distinct']
    assert list(inspect.signature(search.Gallery.__init__).parameters) == ['self', 'engine', 'capacity', 'coarse', 'subjects']
