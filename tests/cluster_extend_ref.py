"""CPU oracle of the incremental clustering (include/ffrnet.h: ffr_cluster_extend): the union-find of tests/cluster_ref.py
over (links i - prior[i]) + (the upper-triangle edges with j >= n_old), on the float64 scores of cluster_ref.cosine64.
Entries of prior outside [0, i] are dropped, as the library reads them as "the row itself"."""
import numpy as np

import cluster_ref


def prior_links(prior):
    """The links (prior[i], i) of the in-contract entries 0 <= prior[i] < i, as an [L,2] array."""
    prior = np.asarray(prior, dtype=np.int64).reshape(-1)
    i = np.arange(prior.size, dtype=np.int64)
    ok = (prior >= 0) & (prior < i)
    return np.stack((prior[ok], i[ok]), 1)


def new_edges(S, threshold, n_old):
    """The pairs i < j with j >= n_old and S[i,j] > threshold (strict): the rectangle and the new rows' triangle."""
    e = cluster_ref.upper_edges(S, threshold)
    return e[e[:, 1] >= n_old]


def extend_from_scores(S, threshold, prior, n_old):
    """rep[N] of the components of the prior's links and the edges of S with a new row."""
    n = np.asarray(S).shape[0]
    edges = np.concatenate((prior_links(prior), new_edges(S, threshold, n_old).reshape(-1, 2)))
    return cluster_ref.union_find(n, edges)


def extend_oracle(emb, threshold, prior, n_old):
    """-> rep[N] from the float64 cosine of emb[N,512]."""
    emb = np.asarray(emb)
    if emb.shape[0] == 0:
        return np.zeros((0,), dtype=np.int64)
    return extend_from_scores(cluster_ref.cosine64(emb), threshold, prior, n_old)


def flat_prior(emb, threshold, n_old):
    """The prior of contract (a): the one-shot oracle clustering of the first n_old rows, then every new row itself."""
    n = np.asarray(emb).shape[0]
    head = cluster_ref.cluster_oracle(emb[:n_old], threshold)[0] if n_old else np.zeros((0,), dtype=np.int64)
    return np.concatenate((head, np.arange(n_old, n, dtype=np.int64)))
