"""CPU checks of the removal's host side: the two forms of the oracle of tests/cluster_remove_ref.py against each other and
against brute-force transitive closure; ffrnet_amd.cluster.remove / Incremental.remove / removal_changes over a stub engine
that answers from the oracle (index maps, tie groups renumbered, add after remove, duplicate and empty rows, rows and keep
both or neither refused); and the argument order of the C prototype."""
import os
import re

import numpy as np
import pytest
import torch

import cluster_density_ref as dref
import cluster_extend_ref as xref
import cluster_ref
import cluster_remove_ref as rref
from ffrnet_amd import cluster as fc

THR = 0.5
MARGIN = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DATA = {}


def bridged(N):
    if N not in _DATA:
        emb, truth, info = dref.planted_bridged(N)
        S = cluster_ref.cosine64(emb)
        rep = cluster_ref.union_find(N, cluster_ref.upper_edges(S, THR))
        _DATA[N] = (emb, S, rep, info)
    return _DATA[N]


def patterns(N, rep, info):
    multi = np.unique(rep[np.bincount(rep, minlength=N)[rep] > 1])
    return {'nothing': [], 'everything': list(range(N)), 'bridge': [info['bridge'][0]], 'chain_mid': [info['chain'][2]],
            'chain_end': [info['chain'][0]], 'zero': [info['zero']], 'first': [0], 'last': [N - 1],
            'every_rep': multi.tolist(), 'every_second': list(range(0, N, 2))}


@pytest.mark.parametrize('N', [20, 168, 1000])
def test_the_two_oracle_forms_agree(N):
    emb, S, rep, info = bridged(N)
    assert cluster_ref.margin(S, THR) > MARGIN
    for name, rows in patterns(N, rep, info).items():
        keep = rref.keep_without(N, rows)
        got = rref.remove_from_scores(S, THR, rep, keep)
        assert np.array_equal(got, rref.survivors_only(S, THR, keep)), name
        assert np.all(got[~keep] == -1) and np.all(got[keep] >= 0)
        aff = rref.affected(rep, keep)
        assert np.array_equal(got[keep & ~aff], rep[keep & ~aff])
        if N == 20:                                         # Warshall over the survivors' edges
            e = cluster_ref.upper_edges(S, THR)
            e = e[keep[e[:, 0]] & keep[e[:, 1]]]
            assert np.array_equal(got[keep], cluster_ref.closure_bruteforce(N, e.tolist())[keep]), name


def test_the_planted_patterns_split_as_described():
    for N, m_rep in ((20, None), (168, 126), (1000, 751)):
        emb, S, rep, info = bridged(N)
        chain, bridge = info['chain'], info['bridge']

        def after(rows):
            keep = rref.keep_without(N, rows)
            return rref.remove_from_scores(S, THR, rep, keep), int(rref.affected(rep, keep).sum())

        both = info['ident'][0] + info['ident'][1]
        assert len(set(rep[both + bridge].tolist())) == 1                 # one cluster through the bridge
        got, m = after([bridge[0]])
        assert m == 11 and len(set(got[info['ident'][0]].tolist())) == 1 and len(set(got[both].tolist())) == 2
        got, m = after([chain[2]])
        assert m == 5 and got[chain[0]] == got[chain[1]] != got[chain[3]] == got[chain[4]] == got[chain[5]]
        got, m = after([chain[0]])
        assert m == 5 and len(set(got[chain[1:]].tolist())) == 1
        got, m = after([info['zero']])
        assert m == 0
        if m_rep is not None:
            rows = patterns(N, rep, info)['every_rep']
            got, m = after(rows)
            keep = rref.keep_without(N, rows)
            assert m == m_rep and np.all(got[rref.affected(rep, keep)] > rep[rref.affected(rep, keep)])    # every label rises


def test_oracle_guard_prior_and_hand_made_scores():
    # 0-1-2 a path, 3-4 an edge, 5 alone
    S = np.eye(6)
    for i, j in ((0, 1), (1, 2), (3, 4)):
        S[i, j] = 0.9
    rep = np.array([0, 0, 0, 3, 3, 5])
    keep = rref.keep_without(6, [1])
    assert rref.remove_from_scores(S, THR, rep, keep).tolist() == [0, -1, 2, 3, 3, 5]
    assert rref.remove_from_scores(S, THR, rep, keep, prior=[0, 1, 0, 3, 4, 5]).tolist() == [0, -1, 0, 3, 3, 5]
    # a link to a removed row, to an unaffected row, or forward, is no link
    assert rref.remove_from_scores(S, THR, rep, keep, prior=[0, 1, 1, 2, 4, 7]).tolist() == [0, -1, 2, 3, 3, 5]
    # the guard: a label outside [0, x] reads as x; row 2 then is a cluster of its own, not hit by the removal of row 1
    assert rref.guard([0, 5, -1, 3, 1 << 62, -(1 << 62)]).tolist() == [0, 1, 2, 3, 4, 5]
    assert rref.remove_from_scores(S, THR, [0, 0, 9, 3, 3, 5], keep).tolist() == [0, -1, 2, 3, 3, 5]
    # an unaffected cluster is not re-scored: a wrong label of a whole cluster comes back as it is
    assert rref.remove_from_scores(S, THR, [0, 0, 0, 3, 4, 5], keep).tolist() == [0, -1, 2, 3, 4, 5]
    assert rref.remove_from_scores(S, THR, rep, np.zeros(6, dtype=bool)).tolist() == [-1] * 6
    assert rref.remove_from_scores(S, THR, rep, np.ones(6, dtype=np.uint8) * 7).tolist() == rep.tolist()
    assert rref.compact(np.array([0, -1, 2, 3, 3, 5]), keep).tolist() == [0, 1, 2, 2, 4]
    assert rref.pick_clusters_for(rep, 3).tolist() == [0, 3] and rref.pick_clusters_for(rep, 4) is None


class StubEngine(object):
    """Answers row_norms, cluster_extend and cluster_remove on the CPU from the oracles, and records the removals."""
    device = torch.device('cpu')

    def __init__(self):
        self.remove_calls, self.extend_calls = [], []

    def row_norms(self, x):
        return x.double().norm(dim=1).float()

    def cluster_extend(self, emb, threshold, prior, n_old, norms=None, validate=True, out=None):
        self.extend_calls.append((emb.size(0), n_old))
        rep = torch.from_numpy(xref.extend_oracle(emb.numpy(), threshold, prior.numpy(), n_old))
        if out is None:
            return rep
        out.copy_(rep)
        return out

    def cluster_remove(self, emb, threshold, rep, keep, prior=None, norms=None, validate=True, out=None):
        self.remove_calls.append(dict(n=emb.size(0), keep=keep.clone(), prior=None if prior is None else prior.clone(),
                                      in_place=out is not None and out.data_ptr() == rep.data_ptr(), validate=validate,
                                      norms=None if norms is None else norms.clone()))
        S = cluster_ref.cosine64(emb.numpy())
        res = torch.from_numpy(rref.remove_from_scores(S, threshold, rep.numpy(), keep.numpy(),
                                                       None if prior is None else prior.numpy()))
        if out is None:
            return res
        out.copy_(res)
        return out


def test_remove_returns_compact_clusters_and_index_maps():
    emb, S, rep, info = bridged(168)
    x = torch.from_numpy(emb)
    eng = StubEngine()
    rows = [info['bridge'][0], 5, 5, 167, info['bridge'][0]]                # duplicates
    keep = rref.keep_without(168, rows)
    want = rref.compact(rref.survivors_only(S, THR, keep), keep)
    for earlier in (fc.dense_ids(torch.from_numpy(rep)), torch.from_numpy(rep), rep.tolist()):
        c, old_to_new, kept = fc.remove(eng, x, THR, earlier, rows=rows)
        assert isinstance(c, fc.Clusters) and c.rep.tolist() == want.tolist() and c.n_clusters == np.unique(want).size
        assert old_to_new.dtype == torch.int64 and old_to_new.shape == (168,) and kept.tolist() == np.nonzero(keep)[0].tolist()
        assert torch.equal(old_to_new[kept], torch.arange(165)) and int((old_to_new < 0).sum()) == 3
        assert all(old_to_new[r] == -1 for r in rows)
    # the mask form, bool and uint8, gives the same; the engine got the mask, no prior, and validates
    for mask in (torch.from_numpy(keep), torch.from_numpy(keep.astype(np.uint8) * 3), keep):
        c2, o2, k2 = fc.remove(eng, x, THR, rep, keep=mask)
        assert torch.equal(c2.rep, c.rep) and torch.equal(o2, old_to_new) and torch.equal(k2, kept)
    call = eng.remove_calls[-1]
    assert call['keep'].tolist() == keep.tolist() and call['prior'] is None and call['validate'] and not call['in_place']
    # empty rows: nothing changes; everything: nothing is left
    c, old_to_new, kept = fc.remove(eng, x, THR, rep, rows=[])
    assert c.rep.tolist() == rep.tolist() and torch.equal(old_to_new, torch.arange(168)) and kept.numel() == 168
    c, old_to_new, kept = fc.remove(eng, x, THR, rep, rows=torch.arange(168))
    assert c.n_clusters == 0 and c.rep.numel() == 0 and bool((old_to_new == -1).all()) and kept.numel() == 0
    # refused: both, neither, out of range, a mask of the wrong size or type, labels of the wrong size
    for kw in (dict(), dict(rows=[1], keep=torch.from_numpy(keep))):
        with pytest.raises(ValueError):
            fc.remove(eng, x, THR, rep, **kw)
    for kw in (dict(rows=[168]), dict(rows=[-1]), dict(keep=torch.ones(167, dtype=torch.bool)), dict(keep=torch.ones(168)),
               dict(rows=[1], must_link=[0] * 167)):
        with pytest.raises(RuntimeError):
            fc.remove(eng, x, THR, rep, **kw)
    with pytest.raises(RuntimeError):
        fc.remove(eng, x, THR, rep[:100], rows=[1])


def test_remove_with_must_link_names_the_first_surviving_row():
    eye = torch.eye(512)[:7].contiguous()                   # orthogonal rows: no scored edge
    eng = StubEngine()
    labels = [4, 9, 4, 4, 9, 2, 4]
    rep = fc.representatives(torch.tensor(labels))
    assert rep.tolist() == [0, 1, 0, 0, 1, 5, 0]
    c, old_to_new, kept = fc.remove(eng, eye, THR, rep, rows=[0], must_link=labels)
    assert eng.remove_calls[-1]['prior'].tolist() == [0, 1, 2, 2, 1, 5, 2]
    assert c.rep.tolist() == [0, 1, 1, 0, 4, 1] and kept.tolist() == [1, 2, 3, 4, 5, 6]
    # without the labels the tied rows part
    c, _, _ = fc.remove(eng, eye, THR, rep, rows=[0])
    assert c.rep.tolist() == [0, 1, 2, 0, 4, 5]


def test_removal_changes():
    before = torch.tensor([0, 0, 0, 3, 3, 5, 6, 6])
    # row 1 (the bridge of cluster 0) and row 3 (the representative of cluster 3) leave, and all of cluster 5
    after = torch.tensor([0, -1, 2, -1, 4, -1, 6, 6])
    touched, now = fc.removal_changes(before, after)
    assert touched.dtype == torch.int64 and touched.tolist() == [0, 3, 5] and now.tolist() == [0, 2, 4]
    touched, now = fc.removal_changes(before, before)
    assert touched.tolist() == [] and now.tolist() == []
    touched, now = fc.removal_changes(before, torch.full((8,), -1))
    assert touched.tolist() == [0, 3, 5, 6] and now.tolist() == []
    assert fc.removal_changes([], [])[0].tolist() == []
    with pytest.raises(ValueError):
        fc.removal_changes(before, after[:3])
    assert 'removal_changes' in fc.changes.__doc__


def from_scratch(emb, tie):
    """The clustering of these rows with the rows of equal tie label linked: the reference of every Incremental state."""
    prior = fc.representatives(torch.as_tensor(tie)).numpy()
    return xref.extend_oracle(np.asarray(emb), THR, prior, 0)


def test_incremental_remove_on_a_stub_engine():
    emb, S, rep, info = bridged(168)
    x = torch.from_numpy(emb)
    eng = StubEngine()
    inc = fc.Incremental(eng, THR, capacity=64)
    inc.add(x[:100])
    inc.add(x[100:])
    assert inc.rep.tolist() == rep.tolist() and inc._tie[:168].tolist() == list(range(168))
    # nothing to remove: no call, the identity map
    assert torch.equal(inc.remove([]), torch.arange(168)) and not eng.remove_calls and len(inc) == 168
    rows = [info['bridge'][0], info['chain'][2], 0, 0]
    keep = rref.keep_without(168, rows)
    old_to_new = inc.remove(rows)
    call = eng.remove_calls[-1]
    assert call['n'] == 168 and call['in_place'] and not call['validate'] and call['keep'].tolist() == keep.tolist()
    assert call['prior'].tolist() == list(range(168))                       # no ties: every row its own group
    assert torch.equal(call['norms'], x.double().norm(dim=1).float())
    assert len(inc) == 165 and old_to_new.tolist() == [int(keep[:i].sum()) if k else -1 for i, k in enumerate(keep)]
    kept = np.nonzero(keep)[0]
    assert torch.equal(inc.embeddings, x[kept]) and torch.equal(inc.norms, x[kept].double().norm(dim=1).float())
    want = cluster_ref.cluster_oracle(emb[kept], THR)[0]
    assert inc.rep.tolist() == want.tolist() and inc._tie[:165].tolist() == list(range(165))
    assert inc.clusters.n_clusters == np.unique(want).size
    assert len(set(want[old_to_new[info['ident'][0] + info['ident'][1]].numpy()].tolist())) == 2      # the bridge is gone
    # add after remove: the rows that left come back at the end, and the labels are those of one clustering
    first = inc.add(x[sorted(set(rows))])
    assert first == 165 and len(inc) == 168
    held = np.concatenate((emb[kept], emb[sorted(set(rows))]))
    assert inc.rep.tolist() == cluster_ref.cluster_oracle(held, THR)[0].tolist()
    assert inc.clusters.n_clusters == np.unique(rep).size
    # remove everything, then start again
    assert bool((inc.remove(torch.arange(168)) == -1).all()) and len(inc) == 0 and inc.clusters.n_clusters == 0
    assert inc.add(x[:10]) == 0 and inc.rep.tolist() == cluster_ref.cluster_oracle(emb[:10], THR)[0].tolist()
    with pytest.raises(RuntimeError):
        inc.remove([10])


def test_incremental_renumbers_tie_groups():
    eye = torch.eye(512)[:9].contiguous()                   # orthogonal rows: the labels are the ties
    eng = StubEngine()
    inc = fc.Incremental(eng, THR)
    inc.add(eye[:4], must_link=[8, 3, 8, 3])
    inc.add(eye[4:9], must_link=[5, 6, 5, 5, 6])
    assert inc.rep.tolist() == [0, 1, 0, 1, 4, 5, 4, 4, 5] and inc._tie[:9].tolist() == [0, 1, 0, 1, 4, 5, 4, 4, 5]
    # rows 0 and 4, the first rows of two groups, leave: the groups stay together under their next rows
    old_to_new = inc.remove([4, 0])
    assert old_to_new.tolist() == [-1, 0, 1, 2, -1, 3, 4, 5, 6]
    assert eng.remove_calls[-1]['prior'].tolist() == [0, 1, 2, 1, 4, 5, 6, 6, 5]
    assert inc.rep.tolist() == [0, 1, 0, 3, 4, 4, 3] and inc._tie[:7].tolist() == [0, 1, 0, 3, 4, 4, 3]
    assert inc.rep.tolist() == from_scratch(eye[[1, 2, 3, 5, 6, 7, 8]], [3, 8, 3, 6, 5, 5, 6]).tolist()
    # a second removal works on the renumbered groups; a later add ties its own rows only
    assert inc.remove([0]).tolist() == [-1, 0, 1, 2, 3, 4, 5]
    assert inc.rep.tolist() == [0, 1, 2, 3, 3, 2] and inc._tie[:6].tolist() == [0, 1, 2, 3, 3, 2]
    assert inc.add(eye[:2], must_link=[1, 1]) == 6
    assert inc.rep.tolist() == [0, 1, 2, 3, 3, 2, 6, 6] and inc._tie[:8].tolist() == [0, 1, 2, 3, 3, 2, 6, 6]


def test_incremental_remove_equals_a_clustering_from_scratch_with_the_ties():
    emb, S, rep, info = bridged(168)
    x = torch.from_numpy(emb)
    eng = StubEngine()
    inc = fc.Incremental(eng, THR)
    track = np.arange(168) // 4                             # rows 4k .. 4k + 3 are tied; 4k + 1 and 4k + 3 survive
    inc.add(x, must_link=track)
    old_to_new = inc.remove(list(range(0, 168, 2)))
    assert len(eng.remove_calls) == 1 and old_to_new[1::2].tolist() == list(range(84))
    assert inc.rep.tolist() == from_scratch(emb[1::2], track[1::2]).tolist()
    assert inc._tie[:84].tolist() == fc.representatives(torch.from_numpy(track[1::2])).tolist()


def test_header_prototype_of_the_removal():
    hdr = open(os.path.join(ROOT, 'include', 'ffrnet.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\bint\s+ffr_cluster_remove\s*\(([^;{}]*)\)\s*;', hdr)
    assert m
    params = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert [a.split()[-1].lstrip('*') for a in params] == ['h', 'emb', 'norms', 'N', 'dim', 'threshold', 'rep_in', 'prior', 'keep',
                                                           'rep', 'stream']
    assert len(params) == 11 and params[8] == 'const uint8_t* keep' and params[6] == 'const int64_t* rep_in'
    from ffrnet_amd import native
    row = [r for r in native.SYMBOLS if r[0] == 'ffr_cluster_remove']
    assert len(row) == 1 and len(row[0][2]) == 11
