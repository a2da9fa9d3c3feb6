"""CPU checks of the certified bf16 shortlist over a subject-labelled gallery: the shortlist rule ffrnet_amd.search mirrors,
and the method itself through the torch model of tests/search_coarse_subjects_ref.py -- wherever the model certifies, its
answer is the exact one of tests/search_subjects_ref.py, in both modes and under removals; and on planted identities the
shortlist of 4k rows certifies where the one of 2k rows does not."""
import numpy as np
import pytest
import torch

import search_coarse_ref as cref
import search_coarse_subjects_ref as ref
import search_subjects_ref as sref
from ffrnet_amd import native, search


def test_shortlist_rule_for_rows_and_identities():
    for k in range(1, 129):
        rows = 32 if k <= 16 else 2 * k if k <= 64 else None            # None: the exact search alone
        ids = 64 if k <= 16 else 4 * k if k <= 32 else None
        assert search.shortlist_size(k) == rows and search.shortlist_size(k, distinct=False) == rows, k
        assert search.shortlist_size(k, distinct=True) == ids, k
    assert search.shortlist_size(10, True) == 64 and search.shortlist_size(32, True) == 128
    assert search.shortlist_size(33, True) is None and search.shortlist_size(64, True) is None
    assert search.COARSE_MAX_K_DISTINCT == 32 and search.COARSE_MAX_K == 64
    assert 'ffr_search_topk_coarse_subjects' in {n for n, _, _ in native.SYMBOLS}


def gaussian(n, seed):
    return torch.randn((n, 512), generator=torch.Generator().manual_seed(seed))


def families():
    """(name, probes, rows, subject) of the three kinds of rows, small enough for the naive restatement"""
    rows, subject, cent = ref.planted(1500, 8, 0.7, 11)
    probes, _ = ref.planted_probes(cent, 9, 0.7, 12)
    yield 'planted', probes, rows, subject
    base = gaussian(1, 13)
    yield 'correlated', base + 0.05 * gaussian(6, 14), base + 0.05 * gaussian(700, 15), torch.arange(700) % 90
    g = gaussian(900, 16)
    copies = torch.randperm(900, generator=torch.Generator().manual_seed(17))[:40]
    g[copies] = g[450].clone()
    subject = torch.arange(900) % 300
    subject[copies[:20]] = 1000 + torch.arange(20)                          # the copies: 20 subjects of their own, and 20 rows
    subject[copies[20:]] = 2000 + torch.arange(20) % 2                      # of two subjects
    yield 'copies', torch.cat((g[450:451] * 0.5 + 1e-3 * gaussian(1, 18), gaussian(5, 19)), 0), g, subject


@pytest.mark.parametrize('removed', [False, True])
def test_where_the_model_certifies_its_answer_is_exact(removed):
    seen = 0
    for name, q, g, subject in families():
        if removed:
            subject = ref.remove_subjects(subject, 0.1, 21)
            assert 0 < int((subject < 0).sum()) < g.size(0)
        s = cref.exact_scores(q, g)
        c = cref.coarse_scores(q, g)
        for k, distinct in ((1, True), (10, True), (32, True), (10, False), (64, False)):
            got = ref.search(q, g, subject, k, distinct, exact=s, coarse=c)
            want = ref.expected(s, subject, k, distinct)
            for a, b in zip(got[:3], want):
                assert a.dtype == b.dtype and torch.equal(a, b), (name, k, distinct)
            if k <= 10:
                naive = sref.search_naive(s.numpy(), subject.numpy(), k, distinct)
                for a, b in zip(got[:3], naive):
                    assert np.array_equal(a.numpy(), b), (name, k, distinct)
            print('%s removed=%s k=%d distinct=%s: certified %d of %d' % (name, removed, k, distinct, int(got[3].sum()), q.size(0)))
            if name == 'planted' and k == 10:
                assert bool(got[3].all()), (k, distinct)                   # the equality is not that of the fallback alone
            if name == 'correlated':
                assert not bool(got[3].any())                              # a shortlist that cannot separate
            seen += int(got[3].sum())
    assert seen > 0


def test_model_when_the_shortlist_is_the_live_gallery():
    """Fewer live rows than k': certified without a look at the scores, padded exactly; all rows removed: all padding."""
    base = gaussian(1, 31)
    q, g = base + 0.05 * gaussian(4, 32), base + 0.05 * gaussian(500, 33)
    subject = torch.full((500,), -1, dtype=torch.int64)
    subject[::25] = torch.arange(20) % 7                                    # 20 live rows of 7 subjects
    s = cref.exact_scores(q, g)
    for k, distinct in ((10, True), (10, False), (32, False)):
        got = ref.search(q, g, subject, k, distinct, exact=s)
        want = ref.expected(s, subject, k, distinct)
        assert bool(got[3].all()) and all(torch.equal(a, b) for a, b in zip(got[:3], want))
    assert int((got[1] >= 0).sum(1).max()) == 20 and bool((ref.search(q, g, subject, 10, True, exact=s)[2][:, 7:] == -1).all())
    got = ref.search(q, g, torch.full((500,), -1), 10, True, exact=s)
    assert bool(got[3].all()) and bool((got[1] == -1).all()) and bool((got[2] == -1).all()) and bool(torch.isinf(got[0]).all())


def test_one_person_with_more_rows_than_the_shortlist_is_not_certified():
    g = gaussian(3000, 41)
    q = gaussian(2, 42)
    g[:200] = q[0] + 0.01 * gaussian(200, 43)
    subject = torch.arange(3000) + 10
    subject[:200] = 3
    got = ref.search(q, g, subject, 5, True)
    want = ref.expected(cref.exact_scores(q, g), subject, 5, True)
    assert got[3].tolist() == [False, True] and all(torch.equal(a, b) for a, b in zip(got[:3], want))
    assert int(got[2][0, 0]) == 3 and int((got[2][0] == 3).sum()) == 1


PLANTED = [(65537, 8, 1.0), (65537, 8, 0.5), (20000, 4, 0.7)]


def test_identity_shortlist_rule_on_planted_rows():
    """About `per` rows of the probe's own person lead every shortlist.  With eps widened by 3e-4 (what the device's
    accumulation may differ by) the model certifies all 33 probes of every family at (k = 10, k' = 64) and at (k = 32,
    k' = 128), and not all of them at (k = 10, k' = 32): the 2k rule of row lists is too short for identities."""
    eps = search.COARSE_EPS + 3e-4
    short = 0
    for G, per, noise in PLANTED:
        rows, subject, cent = ref.planted(G, per, noise, 5)
        q, _ = ref.planted_probes(cent, 33, noise, 9)
        s, c = cref.exact_scores(q, rows), cref.coarse_scores(q, rows)
        count = {}
        for k, kp in ((10, 64), (32, 128), (10, 32)):
            got = ref.search(q, rows, subject, k, True, eps=eps, exact=s, coarse=c, kp=kp)
            count[(k, kp)] = int(got[3].sum())
            want = ref.expected(s, subject, k, True)
            assert all(torch.equal(a, b) for a, b in zip(got[:3], want))
        print('G = %d, per = %d, noise = %.1f: certified of 33: %s' % (G, per, noise, count))
        assert count[(10, 64)] == 33 and count[(32, 128)] == 33
        short += 33 - count[(10, 32)]
    assert short > 0
