"""Host-side checks of the filtered search (include/ffrnet.h: ffr_search_topk_filtered): the numpy restatement of
tests/search_filtered_ref.py against a naive per-probe loop, hand-made cases, the shard argument on the restatement, and
the Python surface that needs no device."""
import inspect

import numpy as np
import pytest
import torch

import search_filtered_ref as fref
import search_subjects_ref as sref
from ffrnet_amd import native, search


def _same(a, b, planes=3):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
               for x, y in list(zip(a, b))[:planes])


def _random_case(rng, Q, G, nsubj, removed, levels, bits):
    """scores from a few levels (ties abound), sparse tags and masks over `bits` bits, bit 31 among them, some words zero"""
    S = rng.choice(np.linspace(-0.5, 0.9, levels).astype(np.float32), size=(Q, G))
    subj = rng.integers(0, nsubj, size=G).astype(np.int32)
    subj[rng.random(G) < removed] = -1
    pool = np.array([0, 1, 5, 9, 17, 30, 31][:bits], dtype=np.int64)

    def draw(n):
        w = np.zeros(n, dtype=np.int64)
        for b in pool:
            w |= (rng.random(n) < 0.3).astype(np.int64) << b
        return w
    return S, subj, draw(G), draw(Q)


def test_ref_equals_the_naive_loop_on_random_cases():
    rng = np.random.default_rng(11)
    for Q, G, nsubj, removed, levels, bits in ((3, 40, 7, 0.0, 5, 3), (4, 64, 20, 0.3, 9, 7), (2, 17, 3, 0.5, 3, 2),
                                               (5, 100, 100, 0.1, 50, 7), (1, 1, 1, 0.0, 2, 1), (2, 30, 4, 0.0, 1000, 4)):
        S, subj, tag, mask = _random_case(rng, Q, G, nsubj, removed, levels, bits)
        for k in (1, 5, 12):
            for base in (0, 1000):
                for distinct in (0, 1):
                    assert _same(fref.search_ref(S, tag, mask, k, subj, distinct, base),
                                 fref.search_naive(S, tag, mask, k, subj, distinct, base)), (Q, G, k, distinct)
                assert _same(fref.search_ref(S, tag, mask, k, None, 0, base), fref.search_naive(S, tag, mask, k, None, 0, base),
                             planes=2), (Q, G, k)


def test_ref_on_hand_made_cases():
    #            row:  0    1    2    3    4    5    6    7
    S = np.array([[0.5, 0.9, 0.9, 0.5, 0.9, 0.1, 0.5, 0.9]] * 5, dtype=np.float32)
    B31 = 0x80000000
    tag = np.array([1, B31, 2, B31 | 1, 0, 4, 1, 2], dtype=np.int64)
    subj = np.array([4, 2, 2, 7, 3, 4, -1, 2], dtype=np.int32)
    #                bit 31   nothing  all        bit 1   bit 0
    mask = np.array([B31,     0,       0xFFFFFFFF, 2,      1], dtype=np.int64)
    s, i, u = fref.search_ref(S, tag, mask, 4, index_base=10)
    # bit 31 only: rows 1 and 3, a bit like any other; fewer admissible rows than k pads
    assert i[0].tolist() == [11, 13, -1, -1] and s[0, :2].tolist() == [np.float32(0.9), 0.5] and np.all(s[0, 2:] == -np.inf)
    assert i[1].tolist() == [-1] * 4 and np.all(s[1] == -np.inf)                   # mask 0: padding
    assert i[2].tolist() == [11, 12, 17, 10]                                         # row 4 has tag 0: admissible for nobody
    assert i[3].tolist() == [12, 17, -1, -1] and i[4].tolist() == [10, 13, 16, -1]
    # the same words as int32 bit patterns
    assert _same(fref.search_ref(S, tag.astype(np.uint32).view(np.int32), mask.astype(np.uint32).view(np.int32), 4, index_base=10),
                 (s, i, u))
    # with subjects: row 6 is removed; identity mode lists a subject by its best ADMISSIBLE row
    s, i, u = fref.search_ref(S, tag, mask, 4, subj, 1)
    assert i[0].tolist() == [1, 3, -1, -1] and u[0].tolist() == [2, 7, -1, -1]
    assert i[2].tolist() == [1, 0, 3, -1] and u[2].tolist() == [2, 4, 7, -1]
    assert i[3].tolist() == [2, -1, -1, -1] and u[3].tolist() == [2, -1, -1, -1]      # subject 2 by row 2, not row 1
    assert i[4].tolist() == [0, 3, -1, -1] and u[4].tolist() == [4, 7, -1, -1]
    s, i, u = fref.search_ref(S, tag, mask, 4, subj, 0)
    assert i[4].tolist() == [0, 3, -1, -1] and i[3].tolist() == [2, 7, -1, -1] and u[3].tolist() == [2, 2, -1, -1]
    assert np.all(i[1] == -1) and np.all(u[1] == -1)
    # two copies of a row under different tags: each probe gets the copy it may see, both see the smaller index
    S2 = np.array([[0.3, 0.8, 0.1, 0.8]] * 3, dtype=np.float32)
    s, i, u = fref.search_ref(S2, np.array([7, 1, 7, 2]), np.array([1, 2, 3]), 2)
    assert i.tolist() == [[1, 0], [3, 0], [1, 3]]
    assert s.dtype == np.float32 and i.dtype == np.int64 and u.dtype == np.int32
    # every tag set and a full mask: the unfiltered restatement
    full = np.full(8, 0xFFFFFFFF, dtype=np.int64)
    for distinct in (0, 1):
        assert _same(fref.search_ref(S, full, np.full(5, 0xFFFFFFFF, dtype=np.int64), 5, subj, distinct),
                     sref.search_ref(S, subj, 5, distinct))


def test_merging_shard_lists_equals_one_search_on_the_ref():
    """The shard argument of the header, per probe over its admissible rows: split G at arbitrary points, list every shard,
    merge the lists with the merge of the subject search, which does not know the filter."""
    rng = np.random.default_rng(12)
    for trial in range(30):
        Q, G = 3, int(rng.integers(1, 90))
        S, subj, tag, mask = _random_case(rng, Q, G, int(rng.integers(1, 12)), float(rng.choice([0.0, 0.3])),
                                          int(rng.integers(2, 12)), int(rng.integers(1, 8)))
        k = int(rng.integers(1, 9))
        cuts = sorted(set([0, G] + [int(c) for c in rng.integers(0, G + 1, size=int(rng.integers(0, 5)))]))
        cuts = cuts + [G]                      # and an empty shard at the end
        for subjects, distinct in ((subj, 0), (subj, 1), (None, 0)):
            parts = [fref.search_ref(S[:, lo:hi], tag[lo:hi], mask, k, None if subjects is None else subjects[lo:hi], distinct,
                                     index_base=lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
            if subjects is None:               # the third plane of a shard is shard-local then: no part of the result
                parts = [(p[0], p[1], p[1].astype(np.int32)) for p in parts]
            merged = sref.merge_ref(*[np.stack([p[j] for p in parts]) for j in range(3)], distinct)
            assert _same(merged, fref.search_ref(S, tag, mask, k, subjects, distinct), planes=3 if subjects is not None else 2), (
                trial, distinct, cuts)


def test_python_surface():
    names = {n for n, _, _ in native.SYMBOLS}
    assert 'ffr_search_topk_filtered' in names
    args = dict((n, a) for n, _, a in native.SYMBOLS)['ffr_search_topk_filtered']
    assert len(args) == 17
    assert callable(native.Engine.search_filtered)
    assert list(inspect.signature(native.Engine.search_filtered).parameters) == [
        'self', 'query', 'mask', 'gallery', 'tags', 'k', 'gallery_norms', 'index_base', 'subjects', 'distinct']
    for fn in ('build_tags', 'tags', 'set_tags', 'set_subject_tags'):
        assert hasattr(search.Gallery, fn)
    for fn in (search.Gallery.search, search.Gallery.search_subjects, search.Gallery.add):
        assert 'mask' in inspect.signature(fn).parameters or 'tags' in inspect.signature(fn).parameters
    assert inspect.signature(search.Gallery.search).parameters['mask'].default is None
    assert 'mask' in inspect.signature(search.search_sharded_filtered).parameters


def test_tag_words():
    """The one conversion of tags and masks: int32 carrying the 32-bit pattern"""
    w = native.tag_words
    assert w(2 ** 32 - 1, 'mask').tolist() == [-1] and w(2 ** 32 - 1, 'mask').dtype == torch.int32
    assert w(0, 'mask').tolist() == [0] and w(2 ** 31, 'mask').tolist() == [-2 ** 31] and w(5, 'mask').tolist() == [5]
    t = w(torch.tensor([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], dtype=torch.int64), 'tags')
    assert t.dtype == torch.int32 and t.tolist() == [0, 1, 2 ** 31 - 1, -2 ** 31, -1]
    assert np.array_equal(t.numpy().view(np.uint32), np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32))
    same = torch.tensor([[-1, 3], [0, -2 ** 31]], dtype=torch.int32)
    assert w(same, 'tags').tolist() == [-1, 3, 0, -2 ** 31]                           # int32: the bits as they are, flat
    assert w(torch.empty((0,), dtype=torch.int64), 'tags').shape == (0,)
    for bad in (2 ** 32, -1, torch.tensor([2 ** 32]), torch.tensor([-1]), torch.tensor([1, -5, 3]), torch.tensor([1.0]),
                torch.tensor([1], dtype=torch.int16), torch.tensor([1], dtype=torch.uint8), 1.0, True, None, [1, 2], '1'):
        with pytest.raises(RuntimeError):
            w(bad, 'tags')
