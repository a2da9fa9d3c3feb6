"""CPU checks of the incremental clustering's host side: the oracle of tests/cluster_extend_ref.py against brute-force
transitive closure, ffrnet_amd.cluster.representatives / changes against hand-written cases, the bookkeeping of
cluster.Incremental and cluster.extend over a stub engine that answers from the oracle.  (The C symbol is held to the header
with every other row of native.SYMBOLS: test_host_logic.py.)"""
import numpy as np
import pytest
import torch

import cluster_extend_ref as xref
import cluster_ref
from ffrnet_amd import cluster as fc

THR = 0.5


def test_oracle_with_prior_matches_bruteforce_closure():
    # hand-made scores on 6 rows: edges (0,4) and (2,5) involve a new row at n_old = 4, (1,3) does not
    S = np.eye(6)
    for i, j in ((0, 4), (2, 5), (1, 3)):
        S[i, j] = 0.9
    S[5, 0] = 0.9                                                        # the lower triangle is never an edge
    assert xref.new_edges(S, THR, 4).tolist() == [[0, 4], [2, 5]]
    assert xref.new_edges(S, THR, 0).tolist() == [[0, 4], [1, 3], [2, 5]]
    assert xref.new_edges(S, THR, 6).tolist() == []
    # prior: 3 belongs with 2; the entries 7 (>= N), -1 and 5 at row 4 (> i) are dropped; 5 with 4
    prior = [0, 1, 2, 2, 5, 4]
    assert xref.prior_links(prior).tolist() == [[2, 3], [4, 5]]
    assert xref.prior_links([0, 7, -1, 2, 5, 4]).tolist() == [[2, 3], [4, 5]]
    # 0-4 (score), 4-5 (link), 2-5 (score), 2-3 (link): everything but row 1, whose edge (1,3) is old x old
    assert xref.extend_from_scores(S, THR, prior, 4).tolist() == [0, 1, 0, 0, 0, 0]
    assert xref.extend_from_scores(S, THR, prior, 6).tolist() == [0, 1, 2, 2, 4, 4]          # nothing scored: the flattened prior
    assert xref.extend_from_scores(S, THR, np.arange(6), 0).tolist() == [0, 1, 2, 1, 0, 2]    # no links: the plain clustering
    # a chain prior flattens to its first row
    assert xref.extend_from_scores(np.eye(5), THR, [0, 0, 1, 2, 3], 5).tolist() == [0] * 5
    # the planted rows: random must-links on top of the scores, against Warshall
    emb, truth, info = cluster_ref.planted(48)
    S = cluster_ref.cosine64(emb)
    rng = np.random.default_rng(5)
    for n_old in (0, 17, 32, 48):
        prior = np.arange(48)
        tie = rng.choice(np.arange(1, 48), 12, replace=False)
        prior[tie] = (rng.random(12) * tie).astype(np.int64)            # prior[i] < i
        edges = xref.prior_links(prior).tolist() + xref.new_edges(S, THR, n_old).tolist()
        want = cluster_ref.closure_bruteforce(48, edges)
        assert xref.extend_oracle(emb, THR, prior, n_old).tolist() == want.tolist()
    # contract (a) on the oracle itself: extending the clustering of the first rows is the clustering of all rows
    full = cluster_ref.cluster_oracle(emb, THR)[0]
    for n_old in (0, 1, 17, 32, 47, 48):
        assert xref.extend_oracle(emb, THR, xref.flat_prior(emb, THR, n_old), n_old).tolist() == full.tolist()


def test_representatives_on_cpu_tensors():
    rep = fc.representatives(torch.tensor([7, 3, 7, 7, 3, -2, 9]))
    assert rep.dtype == torch.int64 and rep.tolist() == [0, 1, 0, 0, 1, 5, 6]
    assert fc.representatives([4, 4, 4]).tolist() == [0, 0, 0]
    assert fc.representatives(torch.arange(5)).tolist() == [0, 1, 2, 3, 4]
    assert fc.representatives(torch.empty(0, dtype=torch.int64)).tolist() == []
    assert fc.representatives(torch.tensor([2, 1, 2, 1], dtype=torch.int32)).tolist() == [0, 1, 0, 1]
    # a rep is its own representatives, and the result is always a legal prior
    r = torch.tensor([0, 1, 0, 3, 1, 0, 6])
    assert torch.equal(fc.representatives(r), r)
    lab = torch.randint(0, 9, (200,), generator=torch.Generator().manual_seed(3))
    rep = fc.representatives(lab)
    assert bool((rep <= torch.arange(200)).all()) and torch.equal(rep[rep], rep)
    assert bool(((lab[:, None] == lab[None, :]) == (rep[:, None] == rep[None, :])).all())


def test_changes_names_the_absorbed_representatives():
    before = torch.tensor([0, 1, 0, 3, 1, 5])
    # two new rows: one bridges the clusters of 1 and 3 (3 goes to 1), one joins cluster 0; 5 stays alone
    after = torch.tensor([0, 1, 0, 1, 1, 5, 1, 0])
    stale, now = fc.changes(before, after)
    assert stale.dtype == torch.int64 and stale.tolist() == [3] and now.tolist() == [1]
    # nothing merged: clusters that only gained rows are not listed
    stale, now = fc.changes(before, torch.tensor([0, 1, 0, 3, 1, 5, 5, 6]))
    assert stale.tolist() == [] and now.tolist() == []
    # a bridge over three clusters
    stale, now = fc.changes(before, torch.tensor([0, 0, 0, 0, 0, 5, 0]))
    assert stale.tolist() == [1, 3] and now.tolist() == [0, 0]
    assert fc.changes([], [0, 0])[0].tolist() == []
    with pytest.raises(ValueError):
        fc.changes(before, before[:3])


class StubEngine(object):
    """Answers row_norms and cluster_extend on the CPU from the oracle, and records what it was asked."""
    device = torch.device('cpu')

    def __init__(self):
        self.norm_calls, self.extend_calls = [], []

    def row_norms(self, x):
        self.norm_calls.append(x.size(0))
        return x.double().norm(dim=1).float()

    def cluster_extend(self, emb, threshold, prior, n_old, norms=None, validate=True, out=None):
        self.extend_calls.append(dict(n=emb.size(0), n_old=n_old, in_place=out is not None and out.data_ptr() == prior.data_ptr(),
                                      norms=None if norms is None else norms.clone(), prior=prior.clone(), validate=validate))
        rep = torch.from_numpy(xref.extend_oracle(emb.numpy(), threshold, prior.numpy(), n_old))
        if out is None:
            return rep
        out.copy_(rep)
        return out


def test_incremental_bookkeeping_on_a_stub_engine():
    emb, truth, info = cluster_ref.planted(168)
    full = torch.from_numpy(cluster_ref.cluster_oracle(emb, THR)[0])
    x = torch.from_numpy(emb)
    eng = StubEngine()
    inc = fc.Incremental(eng, THR, capacity=64)
    assert len(inc) == 0 and inc.embeddings.shape == (0, 512) and inc.clusters.n_clusters == 0
    firsts = [inc.add(x[:50]), inc.add(x[50:100]), inc.add(x[100:100]), inc.add(x[100:])]
    assert firsts == [0, 50, 100, 100] and len(inc) == 168
    # norms for the new rows only; one extend per non-empty add, over everything held, in place, with all the norms
    assert eng.norm_calls == [50, 50, 68]
    assert [(c['n'], c['n_old'], c['in_place'], c['validate']) for c in eng.extend_calls] == [
        (50, 0, True, False), (100, 50, True, False), (168, 100, True, False)]
    want_norms = x.double().norm(dim=1).float()
    for c in eng.extend_calls:
        assert torch.equal(c['norms'], want_norms[:c['n']])
        assert torch.equal(c['prior'][c['n_old']:], torch.arange(c['n_old'], c['n']))           # new rows start alone
    assert torch.equal(eng.extend_calls[1]['prior'][:50], torch.from_numpy(cluster_ref.cluster_oracle(emb[:50], THR)[0]))
    # the buffers grew (64 -> 1024) and kept their rows
    assert inc._emb.size(0) >= 168 and torch.equal(inc.embeddings, x) and torch.equal(inc.norms, want_norms)
    assert torch.equal(inc.rep, full)
    c = inc.clusters
    assert isinstance(c, fc.Clusters) and c.n_clusters == 43 and torch.equal(c.rep, full)
    with pytest.raises(RuntimeError):
        inc.add(x[:, :256])
    with pytest.raises(RuntimeError):
        inc.add(x[:4], must_link=[1, 2, 3])
    assert len(inc) == 168


def test_must_link_priors_of_incremental_and_extend():
    eye = torch.eye(512)[:9].contiguous()                                 # orthogonal rows: no scored edge
    eng = StubEngine()
    inc = fc.Incremental(eng, THR)
    assert inc.add(eye[:4], must_link=[8, 3, 8, 3]) == 0
    assert inc.rep.tolist() == [0, 1, 0, 1]
    assert inc.add(eye[4:9], must_link=torch.tensor([5, 6, 5, 5, 6])) == 4
    assert eng.extend_calls[1]['prior'].tolist() == [0, 1, 0, 1, 4, 5, 4, 4, 5]               # labels tie new rows only
    assert inc.rep.tolist() == [0, 1, 0, 1, 4, 5, 4, 4, 5]
    # extend(): a Clusters or a plain rep as `earlier`, n_old = 0 included
    earlier = fc.dense_ids(torch.tensor([0, 1, 0, 1]))
    for e in (earlier, earlier.rep, [0, 1, 0, 1]):
        c = fc.extend(eng, eye, THR, e, must_link=[5, 6, 5, 5, 6])
        assert isinstance(c, fc.Clusters) and c.rep.tolist() == [0, 1, 0, 1, 4, 5, 4, 4, 5] and c.n_clusters == 4
        assert eng.extend_calls[-1]['n_old'] == 4
    c = fc.extend(eng, eye, THR, torch.empty(0, dtype=torch.int64))
    assert c.rep.tolist() == list(range(9)) and eng.extend_calls[-1]['n_old'] == 0
    with pytest.raises(RuntimeError):
        fc.extend(eng, eye[:3], THR, earlier)
    # planted rows through extend(): contract (a)
    emb, truth, info = cluster_ref.planted(48)
    x = torch.from_numpy(emb)
    head = torch.from_numpy(cluster_ref.cluster_oracle(emb[:20], THR)[0])
    assert fc.extend(eng, x, THR, head).rep.tolist() == cluster_ref.cluster_oracle(emb, THR)[0].tolist()
    import ffrnet_amd
    assert ffrnet_amd.Incremental is fc.Incremental
