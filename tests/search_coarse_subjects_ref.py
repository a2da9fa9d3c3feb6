"""A torch-CPU model of the certified bf16 shortlist over a subject-labelled gallery (include/ffrnet.h:
ffr_search_topk_coarse_subjects), for the tests: the model of tests/search_coarse_ref.py (plane, split probe, coarse score,
shortlist) under the removal mask, plus the alive rule and the certificate, each by its definition; and the planted rows the
tests of the shortlist rule are run on.  No test in itself."""
import numpy as np
import torch

import search_coarse_ref as cref
import search_subjects_ref as sref
from ffrnet_amd.search import COARSE_EPS, shortlist_size


def planted(G, per, noise, seed):
    """G rows of nsub = ceil(G / per) people, a person's rows spread over the gallery (subject[g] = g % nsub): a centre per
    person, rows = centre + noise * randn -> (rows[G,512], subject[G] int64, centres[nsub,512])."""
    gen = torch.Generator().manual_seed(seed)
    nsub = (G + per - 1) // per
    cent = torch.randn((nsub, 512), generator=gen)
    subject = torch.arange(G) % nsub
    rows = cent[subject] + noise * torch.randn((G, 512), generator=gen)
    return rows, subject, cent


def planted_probes(cent, Q, noise, seed):
    """Q probes of Q different people: centre + noise * randn -> (probes[Q,512], pick[Q]: whose)."""
    gen = torch.Generator().manual_seed(seed)
    pick = torch.randperm(cent.size(0), generator=gen)[:Q]
    return cent[pick] + noise * torch.randn((Q, 512), generator=gen), pick


def remove_subjects(subject, frac, seed):
    """subject with a seeded share `frac` of the subjects marked removed (-1)."""
    subject = subject.clone()
    ids = torch.unique(subject[subject >= 0])
    gen = torch.Generator().manual_seed(seed)
    gone = ids[torch.randperm(ids.numel(), generator=gen)[:int(round(frac * ids.numel()))]]
    subject[torch.isin(subject, gone)] = -1
    return subject


def first_of_each(u):
    """positions of the first occurrence of every value of u, ascending"""
    seen, keep = set(), []
    for j, x in enumerate(u.tolist()):
        if x not in seen:
            seen.add(x)
            keep.append(j)
    return torch.tensor(keep, dtype=torch.int64)


def search(q, g, subject, k, distinct, eps=COARSE_EPS, exact=None, coarse=None, kp=None):
    """The method on the CPU -> (scores[Q,k] fp32, index[Q,k] int64, subjects[Q,k] int32, certified[Q] bool).  A probe the
    model does not certify gets the answer of tests/search_subjects_ref.py (the exact search, as on the device).  `exact` and
    `coarse`: the [Q,G] score matrices when the caller has them; kp: a shortlist length other than the rule's."""
    Q, G = q.size(0), g.size(0)
    subject = torch.as_tensor(subject).to(torch.int64)
    s = cref.exact_scores(q, g) if exact is None else exact
    if kp is None:
        kp = shortlist_size(k, distinct)
    fs, fi, fu = sref.search_ref(s.numpy(), subject.numpy(), k, distinct)
    out_s, out_i, out_u = torch.from_numpy(fs), torch.from_numpy(fi), torch.from_numpy(fu)
    cert = torch.zeros((Q,), dtype=torch.bool)
    if kp is None or G == 0:
        return out_s, out_i, out_u, cert
    c = cref.coarse_scores(q, g) if coarse is None else coarse
    live = subject >= 0
    idx = torch.arange(G)[live]
    for r in range(Q):
        cs, ci = cref.topk_total_order(c[r][live], idx, kp)           # the k' best live rows by coarse score
        ss, si = cref.topk_total_order(s[r][ci], ci, kp)              # re-scored, in the total order
        if distinct:
            alive = first_of_each(subject[si])
            ss, si = ss[alive], si[alive]
        if ci.numel() < kp or G <= kp:                                # the shortlist is every live row
            ok = True
        else:
            ok = ss.numel() >= k and bool(cs[-1] + eps < ss[k - 1])
        if ok:
            cert[r] = True
            n = min(k, ss.numel())
            out_s[r], out_i[r], out_u[r] = float('-inf'), -1, -1
            out_s[r, :n], out_i[r, :n], out_u[r, :n] = ss[:n], si[:n], subject[si[:n]].to(torch.int32)
    return out_s, out_i, out_u, cert


def expected(s, subject, k, distinct, index_base=0):
    """The exact answer from a score matrix, as torch tensors (tests/search_subjects_ref.py: search_ref)."""
    return tuple(torch.from_numpy(x) for x in sref.search_ref(np.asarray(s), np.asarray(subject), k, distinct, index_base))
