"""A torch-CPU model of the certified bf16 shortlist under a per-probe filter (include/ffrnet.h:
ffr_search_topk_coarse_filtered), for the tests.  Composed, per probe, from the models that exist: the coarse score, the
total order and the plane of tests/search_coarse_ref.py, the alive rule of tests/search_coarse_subjects_ref.py, and the
exact filtered search of tests/search_filtered_ref.py for a probe that is not certified.  Each step by its definition:
the admissible set, the k' best of it by coarse score, the re-score, the alive rule, the certificate.  No test in itself."""
import numpy as np
import torch

import search_coarse_ref as cref
import search_coarse_subjects_ref as csref
import search_filtered_ref as fref
from ffrnet_amd.search import COARSE_EPS, shortlist_size


def tag_patterns(G, kind, seed):
    """tag[G] int64 in [0, 2^32): 'all' every bit set, 'half' a coin flip on bit 0 (the other rows carry bit 1 alone),
    'one' one random bit of 32, 'bit31' a coin flip on bit 31 (else 0: a row nobody may see)."""
    gen = torch.Generator().manual_seed(seed)
    if kind == 'all':
        return torch.full((G,), 2 ** 32 - 1, dtype=torch.int64)
    if kind == 'half':
        return torch.where(torch.rand((G,), generator=gen) < 0.5, 1, 2).to(torch.int64)
    if kind == 'one':
        return torch.ones((G,), dtype=torch.int64) << torch.randint(0, 32, (G,), generator=gen)
    assert kind == 'bit31'
    return torch.where(torch.rand((G,), generator=gen) < 0.5, 2 ** 31, 0).to(torch.int64)


def admissible(tag, mask_q, subject=None):
    """bool [G]: the rows probe q may see"""
    ok = (torch.as_tensor(tag).to(torch.int64) & int(mask_q)) != 0
    if subject is not None:
        ok &= torch.as_tensor(subject).to(torch.int64) >= 0
    return ok


def search(q, g, tag, mask, k, subject=None, distinct=False, eps=COARSE_EPS, exact=None, coarse=None):
    """The method on the CPU -> (scores[Q,k] fp32, index[Q,k] int64, subjects[Q,k] int32, certified[Q] bool, slack[Q]).  tag[G]
    and mask[Q] are int64 words in [0, 2^32).  A probe the model does not certify gets the answer of
    tests/search_filtered_ref.py, as on the device.  slack[q] = s_k - (c_k' + eps) where the certificate compares the two (a
    full list at G > k' with k entries to compare), +inf where the list is every admissible row, -inf where it is full and
    holds fewer than k alive entries.  Without `subject` the third plane is the listed rows' own indices and no part of the
    library's result.  `exact` and `coarse`: the [Q,G] score matrices when the caller has them."""
    Q, G = q.size(0), g.size(0)
    tag, mask = torch.as_tensor(tag).to(torch.int64), torch.as_tensor(mask).to(torch.int64)
    s = cref.exact_scores(q, g) if exact is None else exact
    kp = shortlist_size(k, distinct)
    fs, fi, fu = fref.search_ref(s.numpy(), tag.numpy(), mask.numpy(), k, None if subject is None else np.asarray(subject),
                                 int(distinct))
    out_s, out_i, out_u = torch.from_numpy(fs), torch.from_numpy(fi), torch.from_numpy(fu)
    cert = torch.zeros((Q,), dtype=torch.bool)
    slack = torch.full((Q,), float('nan'), dtype=torch.float64)
    if kp is None or G == 0:
        return out_s, out_i, out_u, cert, slack
    c = cref.coarse_scores(q, g) if coarse is None else coarse
    ident = torch.arange(G) if subject is None else torch.as_tensor(subject).to(torch.int64)
    for r in range(Q):
        adm = admissible(tag, mask[r], subject)                       # the admissible set of this probe
        idx = torch.arange(G)[adm]
        cs, ci = cref.topk_total_order(c[r][adm], idx, kp)            # its k' best by coarse score
        ss, si = cref.topk_total_order(s[r][ci], ci, kp)              # re-scored, in the total order
        if distinct:
            alive = csref.first_of_each(ident[si])
            ss, si = ss[alive], si[alive]
        if ci.numel() < kp or G <= kp:                                # the shortlist is every admissible row
            ok, slack[r] = True, float('inf')
        elif ss.numel() < k:
            ok, slack[r] = False, float('-inf')
        else:
            ok = bool(cs[-1] + eps < ss[k - 1])
            slack[r] = float(ss[k - 1].double() - (cs[-1].double() + eps))
        if ok:
            cert[r] = True
            n = min(k, ss.numel())
            out_s[r], out_i[r], out_u[r] = float('-inf'), -1, -1
            out_s[r, :n], out_i[r, :n], out_u[r, :n] = ss[:n], si[:n], ident[si[:n]].to(torch.int32)
    return out_s, out_i, out_u, cert, slack


def certifying_inputs(kind, seed):
    """The inputs on which the device must certify every probe (tests/test_host_search_coarse_filtered.py checks the margin,
    tests/test_gpu_search_coarse_filtered.py the device): Gaussian rows, G = 4096, Q = 33, mask = bit 0, tags of `kind`:
    'all', 'half', or 'one' -> (q[33,512], g[4096,512], tag[4096] int64, mask[33] int64)."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn((4096, 512), generator=gen)
    q = torch.randn((33, 512), generator=gen)
    return q, g, tag_patterns(4096, kind, seed + 1), torch.ones((33,), dtype=torch.int64)


CERTIFYING = [(kind, 500 + 10 * j) for j, kind in enumerate(('all', 'half', 'one'))]      # (tag kind, seed)
CERTIFYING_K = (1, 10, 32)
