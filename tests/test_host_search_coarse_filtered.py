"""CPU checks of the certified bf16 shortlist under a per-probe filter (include/ffrnet.h: ffr_search_topk_coarse_filtered):
the symbol row against the header; the proof, through the torch model of tests/search_coarse_filtered_ref.py -- wherever the
model certifies a probe, its shortlist answer is the exact one of tests/search_filtered_ref.py, on Gaussian, correlated and
planted rows, with and without subjects, in both modes, under removals, for several tag and mask patterns; and the margin
of the inputs on which tests/test_gpu_search_coarse_filtered.py demands that the device certify every probe."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import search_coarse_filtered_ref as ref
import search_coarse_ref as cref
import search_coarse_subjects_ref as csref
import search_filtered_ref as fref
from ffrnet_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_row_matches_the_header():
    """The prototype of include/ffrnet.h, parameter by parameter, against the argtypes row: pointers as pointers, G and
    index_base as long long, the rest int; and the order the binding relies on."""
    hdr = open(os.path.join(ROOT, 'include', 'ffrnet.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\bint\s+ffr_search_topk_coarse_filtered\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'ffr_search_topk_coarse_filtered is not declared'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    rows = [r for r in native.SYMBOLS if r[0] == 'ffr_search_topk_coarse_filtered']
    assert len(rows) == 1 and rows[0][1] is ctypes.c_int
    argtypes = rows[0][2]
    assert len(argtypes) == len(params) == 20
    for decl, ct in zip(params, argtypes):
        want = ctypes.c_void_p if '*' in decl else ctypes.c_longlong if decl.startswith('long long') else ctypes.c_int
        assert ct is want, (decl, ct)
    names = [p.rsplit(' ', 1)[1].lstrip('*') for p in params]
    assert names == ['h', 'query', 'query_mask', 'Q', 'gallery', 'gallery_norms', 'gallery_plane', 'plane_flag', 'gallery_tag',
                     'gallery_subject', 'G', 'dim', 'k', 'index_base', 'distinct', 'top_score', 'top_index', 'top_subject',
                     'certified', 'stream']
    lib = ctypes.CDLL(native.lib_path())          # loads without a GPU
    assert lib.ffr_search_topk_coarse_filtered is not None


def gaussian(n, seed):
    return torch.randn((n, 512), generator=torch.Generator().manual_seed(seed))


def families():
    """(name, probes, rows, subject) of the three kinds of rows, small enough for the naive restatement"""
    rows, subject, cent = csref.planted(1500, 8, 0.7, 11)
    probes, _ = csref.planted_probes(cent, 9, 0.7, 12)
    yield 'planted', probes, rows, subject
    base = gaussian(1, 13)
    yield 'corr', base + 0.05 * gaussian(6, 14), base + 0.05 * gaussian(700, 15), torch.arange(700) % 90
    yield 'rand', gaussian(7, 16), gaussian(1100, 17), torch.arange(1100) % 140


def masks_for(Q, kind):
    """[Q] masks that go with tag_patterns(kind): different words in one batch, a mask-0 probe among them"""
    if kind == 'all':
        words = [1, 2 ** 31, 0, 0x80000001, 6, 2 ** 32 - 1, 0x10, 3]
    elif kind == 'half':
        words = [1, 2, 3, 0, 1, 4, 2, 0x80000001]
    elif kind == 'one':
        words = [1, 0xFFFF, 2 ** 31, 0, 0xF0F0F0F0, 2, 2 ** 32 - 1, 0x00010001]
    else:
        words = [2 ** 31, 1, 0x80000001, 0, 2 ** 31, 2 ** 32 - 1, 2 ** 31, 0x7FFFFFFF]
    return torch.tensor([words[r % 8] for r in range(Q)], dtype=torch.int64)


@pytest.mark.parametrize('kind', ['all', 'half', 'one', 'bit31'])
def test_where_the_model_certifies_its_answer_is_exact(kind):
    seen = 0
    for name, q, g, subject in families():
        tag = ref.tag_patterns(g.size(0), kind, 23)
        mask = masks_for(q.size(0), kind)
        s = cref.exact_scores(q, g)
        c = cref.coarse_scores(q, g)
        gone = csref.remove_subjects(subject, 0.1, 21)
        for subj in (None, subject, gone):
            for k, distinct in ((1, False), (10, False), (64, False), (1, True), (10, True), (32, True)):
                if distinct and subj is None:
                    continue
                got = ref.search(q, g, tag, mask, k, subj, distinct, exact=s, coarse=c)
                want = fref.search_ref(s.numpy(), tag.numpy(), mask.numpy(), k, None if subj is None else subj.numpy(), int(distinct))
                for a, b in zip(got[:3], want):
                    assert np.array_equal(a.numpy(), b), (name, kind, k, distinct)
                if k == 1:
                    naive = fref.search_naive(s.numpy(), tag.numpy(), mask.numpy(), k, None if subj is None else subj.numpy(), int(distinct))
                    for a, b in zip(got[:3], naive):
                        assert np.array_equal(a.numpy(), b), (name, kind, k, distinct)
                cert = got[3]
                print('%s %s subj=%s k=%d distinct=%s: certified %d of %d' % (name, kind, subj is not None, k, distinct, int(cert.sum()), q.size(0)))
                assert bool(cert[mask == 0].all())                         # an empty shortlist is every admissible row
                if name == 'corr' and kind == 'all':
                    full = torch.tensor([bool(ref.admissible(tag, m, subj).sum() > 128) for m in mask])
                    assert not bool(cert[full].any())                      # a shortlist that cannot separate
                seen += int(cert[mask != 0].sum())
    assert seen > 0


def test_a_short_list_is_every_admissible_row():
    """About 128 admissible rows of 4096 correlated ones: at k = 64 the list of 128 is short for most probes, which are
    certified without a look at the scores; fewer admissible rows than k pads exactly."""
    base = gaussian(1, 31)
    q, g = base + 0.05 * gaussian(8, 32), base + 0.05 * gaussian(4096, 33)
    tag = ref.tag_patterns(4096, 'one', 34)
    mask = torch.tensor([1 << b for b in range(8)], dtype=torch.int64)
    s = cref.exact_scores(q, g)
    got = ref.search(q, g, tag, mask, 64, exact=s)
    n_adm = torch.tensor([int(ref.admissible(tag, m).sum()) for m in mask])
    assert bool((n_adm < 128).any()) and bool((n_adm > 64).all()) and bool(got[3][n_adm < 128].all())
    want = fref.search_ref(s.numpy(), tag.numpy(), mask.numpy(), 64)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(got[:2], want[:2]))
    tag5 = torch.zeros((4096,), dtype=torch.int64)
    tag5[::1000] = 4                                                       # 5 admissible rows under bit 2
    got = ref.search(q, g, tag5, torch.full((8,), 4), 10, exact=s)
    assert bool(got[3].all()) and bool((got[1][:, 5:] == -1).all()) and bool((got[1][:, :5] % 1000 == 0).all())


def test_one_person_with_more_admissible_rows_than_the_shortlist():
    """200 near-copies of probe 0 under one subject: no certificate in identity mode; with all but two of them inadmissible
    for the probe's mask, the same probe certifies."""
    g = gaussian(3000, 41)
    q = gaussian(2, 42)
    g[:200] = q[0] + 0.01 * gaussian(200, 43)
    subject = torch.arange(3000) + 10
    subject[:200] = 3
    mask = torch.tensor([1, 1])
    tag = torch.full((3000,), 1, dtype=torch.int64)
    s = cref.exact_scores(q, g)
    got = ref.search(q, g, tag, mask, 5, subject, True, exact=s)
    want = fref.search_ref(s.numpy(), tag.numpy(), mask.numpy(), 5, subject.numpy(), 1)
    assert got[3].tolist() == [False, True] and all(np.array_equal(a.numpy(), b) for a, b in zip(got[:3], want))
    tag[2:200] = 2
    got = ref.search(q, g, tag, mask, 5, subject, True, exact=s)
    want = fref.search_ref(s.numpy(), tag.numpy(), mask.numpy(), 5, subject.numpy(), 1)
    assert got[3].tolist() == [True, True] and all(np.array_equal(a.numpy(), b) for a, b in zip(got[:3], want))
    assert int(got[2][0, 0]) == 3 and int(got[1][0, 0]) < 2


@pytest.mark.parametrize('kind,seed', ref.CERTIFYING)
def test_margin_of_the_certifying_inputs(kind, seed):
    """The inputs of the device's certification test: the model certifies 33 of 33 at k = 1, 10 and 32, and the smallest
    slack s_k - (c_k' + eps) is above 2^-11.  The model's coarse score differs from the device's only in the accumulation
    order of the matrix core, which the bound allows 2^-13: it cannot flip one of these certificates.  With these seeds the
    smallest slack of the nine cases is 3.1e-3 (all bits set, k = 32) and max |c - s| is 3.3e-4."""
    q, g, tag, mask = ref.certifying_inputs(kind, seed)
    s, c = cref.exact_scores(q, g), cref.coarse_scores(q, g)
    print('%s: max |c - s| = %.3e' % (kind, float((c - s).abs().max())))
    assert float((c - s).abs().max()) < ref.COARSE_EPS
    for k in ref.CERTIFYING_K:
        got = ref.search(q, g, tag, mask, k, exact=s, coarse=c)
        slack = got[4]
        print('%s k = %d: certified %d of 33, smallest slack %.3e' % (kind, k, int(got[3].sum()), float(slack.min())))
        assert bool(got[3].all()) and float(slack.min()) > 2.0 ** -11
        want = fref.search_ref(s.numpy(), tag.numpy(), mask.numpy(), k)
        assert all(np.array_equal(a.numpy(), b) for a, b in zip(got[:2], want[:2]))
