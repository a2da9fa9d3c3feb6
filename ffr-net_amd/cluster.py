"""Grouping unlabelled embeddings into identities (include/ffrnet.h: ffr_cluster_threshold, ffr_cluster_templates).

A photo collection or a dump of video tracks arrives as N unlabelled faces; before the first Gallery.add they have to be
grouped by person and every group fused into one template row:

  c = cluster.cluster(engine, f, threshold)          # f[N,512] e.g. Engine.embed(...)[0]; threshold from lfw.get_avg_accuracy
  t = cluster.templates(engine, f, c)                # [c.n_clusters,512], unit rows
  gallery = Gallery(engine); gallery.add(t)          # template row r is cluster id r

The clustering is single-link at one cosine threshold: rows i < j are joined iff their search score is > threshold, and
a cluster is a connected component of those edges.  It runs on the device; only pairwise_scores() is host logic.
"""
import collections

import torch

Clusters = collections.namedtuple('Clusters', ['rep', 'cluster_id', 'n_clusters', 'sizes'])
Clusters.__doc__ = """rep[N] int64: the smallest row index of each row's cluster; cluster_id[N] int64: dense ids 0 .. C-1 in
order of representative; n_clusters: C (int); sizes[C] int64: rows per cluster."""


def dense_ids(rep):
    """rep[N] (any device) -> Clusters: ids 0 .. C-1 by ascending representative."""
    rep = torch.as_tensor(rep)
    uniq, inv, counts = torch.unique(rep, sorted=True, return_inverse=True, return_counts=True)
    return Clusters(rep, inv.reshape(rep.shape), int(uniq.numel()), counts)


def cluster(engine, emb, threshold, norms=None):
    """Single-link clustering of emb[N,512] (fp32, on the Engine's device) at `threshold` -> Clusters."""
    return dense_ids(engine.cluster(emb, threshold, norms=norms))


def member_order(clusters):
    """-> (order[N], offsets[C+1]) int64: the rows sorted by cluster id then row index, and each cluster's slice of them."""
    cid = clusters.cluster_id
    order = torch.argsort(cid, stable=True)
    offsets = torch.zeros((clusters.n_clusters + 1,), device=cid.device, dtype=torch.int64)
    offsets[1:] = torch.cumsum(clusters.sizes, 0)
    return order, offsets


def templates(engine, emb, clusters, norms=None):
    """One unit template per cluster, row c for cluster id c: the normalised sum of the cluster's normalised rows
    -> [C,512], ready for Gallery.add."""
    order, offsets = member_order(clusters)
    if clusters.cluster_id.numel() != emb.size(0):
        raise RuntimeError('ffrnet_amd: %d cluster ids for %d embeddings' % (clusters.cluster_id.numel(), emb.size(0)))
    return engine.cluster_templates(emb, order, offsets, norms=norms, validate=False)     # in range by construction


def pairwise_scores(pred, truth):
    """Pair-counting agreement of two labelings of the same N rows -> (precision, recall, f): over all N(N-1)/2 row pairs,
    precision = pairs together in both / pairs together in pred, recall = ... / pairs together in truth, f their harmonic
    mean.  From exact integer contingency counts; an empty denominator counts as 1.0.  Host logic: any device, any
    integer labels."""
    pred = torch.as_tensor(pred).reshape(-1).cpu()
    truth = torch.as_tensor(truth).reshape(-1).cpu()
    if pred.numel() != truth.numel():
        raise ValueError('pairwise_scores: %d predicted labels, %d true labels' % (pred.numel(), truth.numel()))

    def pairs(counts):
        return sum(c * (c - 1) // 2 for c in counts.tolist())

    _, p = torch.unique(pred, return_inverse=True)
    _, t = torch.unique(truth, return_inverse=True)
    nt = int(t.max()) + 1 if t.numel() else 1
    together_pred = pairs(torch.unique(p, return_counts=True)[1])
    together_truth = pairs(torch.unique(t, return_counts=True)[1])
    both = pairs(torch.unique(p * nt + t, return_counts=True)[1])
    precision = both / together_pred if together_pred else 1.0
    recall = both / together_truth if together_truth else 1.0
    f = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
    return precision, recall, f
