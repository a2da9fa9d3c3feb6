"""CPU checks of the certified bf16 shortlist search: the two rules ffrnet_amd.search mirrors (COARSE_EPS, shortlist_size)
against the header, the method itself through the torch model of tests/search_coarse_ref.py against a float64 ranking, and
the rounding bound on a row built to come close to it."""
import os
import re

import torch

import search_coarse_ref as ref
from ffrnet_amd import native, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eps_and_shortlist_rule():
    assert search.COARSE_EPS == 2.0 ** -8 + 2.0 ** -12
    header = open(os.path.join(ROOT, 'include', 'ffrnet.h')).read()
    m = re.search(r'#define FFR_COARSE_EPS \(([0-9.]+)f \+ ([0-9.]+)f\)', header)
    assert m and float(m.group(1)) + float(m.group(2)) == search.COARSE_EPS      # one value in the kernel and in Python
    for k in range(1, 129):
        want = 32 if k <= 16 else 2 * k if k <= 64 else None                      # None: the exact search alone
        assert search.shortlist_size(k) == want, k
    assert search.shortlist_size(64) == 128
    names = {n for n, _, _ in native.SYMBOLS}
    assert {'ffr_coarse_pack', 'ffr_search_topk_coarse'} <= names


def gaussian(n, seed):
    return torch.randn((n, 512), generator=torch.Generator().manual_seed(seed))


def test_model_reproduces_the_float64_ranking():
    q, g = gaussian(16, 1), gaussian(20000, 2)
    q64, g64 = q.double(), g.double()
    cos = (q64 @ g64.T) / (q64.norm(dim=1)[:, None] * g64.norm(dim=1)[None, :] + 1e-8)
    for k in (1, 10, 64, 65):
        want = torch.stack([ref.topk_total_order(cos[r], torch.arange(g.size(0)), k)[1] for r in range(q.size(0))])
        s, i, cert, slots = ref.search(q, g, k)
        assert torch.equal(i, want), k
        assert (s.double() - cos.gather(1, i)).abs().max().item() <= 1e-6
        if k <= 64:
            assert bool(cert.all()) and int(slots.max()) <= search.shortlist_size(k), (k, slots.tolist())
        else:
            assert not bool(cert.any())
    # the coarse score stays far inside the bound on Gaussian rows
    err = (ref.coarse_scores(q, g).double() - cos).abs().max().item()
    assert err <= 6e-4, err
    # a shortlist that does not separate: the certificate fails, the fallback still gives the ranking
    base = gaussian(1, 3)
    gc = base + 0.05 * gaussian(3000, 4)
    qc = base + 0.05 * gaussian(8, 5)
    s, i, cert, slots = ref.search(qc, gc, 10)
    assert not bool(cert.any()) and int(slots.min()) > 32
    c64 = (qc.double() @ gc.double().T) / (qc.double().norm(dim=1)[:, None] * gc.double().norm(dim=1)[None, :] + 1e-8)
    assert (s.double() - c64.gather(1, i)).abs().max().item() <= 1e-6
    left = c64.clone().scatter_(1, i, float('-inf'))
    assert (left.max(1).values - s[:, -1].double()).max().item() <= 2e-6
    # G <= k': the shortlist is the gallery
    s, i, cert, _ = ref.search(q, g[:20], 10)
    assert bool(cert.all()) and torch.equal(i, torch.stack([ref.topk_total_order(cos[r, :20], torch.arange(20), 10)[1] for r in range(16)]))


def test_midpoint_row_comes_close_to_the_bound_and_keeps_it():
    """Every element of the row rounds up by nearly the full unit round-off, against a probe of one sign: the coarse score
    errs by >= 0.9 * 2^-8, so no smaller eps would do, and by <= COARSE_EPS."""
    g = ref.midpoint_row()[None, :]
    q = torch.ones((1, 512))
    plane = ref.bf16(ref.unit(g, ref.norms32(g)))
    rel = (plane / ref.unit(g, ref.norms32(g)) - 1.0)
    assert rel.min().item() > 0.99 * 2.0 ** -8 / (1 + 2.0 ** -8)                  # all up, all nearly the worst case
    c = ref.coarse_scores(q, g).double()
    cos = (q.double() @ g.double().T) / (q.double().norm() * g.double().norm() + 1e-8)
    s = ref.exact_scores(q, g).double()
    for err in ((c - cos).abs().item(), (c - s).abs().item()):
        print('midpoint row: |coarse - exact| = %.6f = %.3f u' % (err, err * 256))
        assert 0.9 * 2.0 ** -8 <= err <= search.COARSE_EPS, err
    # the probe along the row itself: Cauchy-Schwarz is tight
    err = (ref.coarse_scores(g, g).double() - 1.0).abs().item()
    assert 0.98 * 2.0 ** -8 <= err <= search.COARSE_EPS, err
