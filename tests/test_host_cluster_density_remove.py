"""CPU checks of the removal from a density-gated clustering: the two forms of the oracle of
tests/cluster_density_remove_ref.py against each other (the six passes against clustering the survivors from scratch, state
included), the kind transitions the planted data must keep exercising, the constructed cases against their docstrings;
ffrnet_amd.cluster.density_remove / density_removal_changes / IncrementalDensity.remove over a stub engine that answers
from the oracles (key re-encoding, both routes, add after remove, a foreign state refused); the routing rule; and the C
prototype with its binding."""
import os
import re

import numpy as np
import pytest
import torch

import cluster_density_extend_ref as xref
import cluster_density_ref as dref
import cluster_density_remove_ref as rref
import cluster_ref
from ffrnet_amd import cluster as fc

THR = 0.5
MARGIN = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DATA = {}


def bridged(N):
    if N not in _DATA:
        emb, truth, info = dref.planted_bridged(N)
        _DATA[N] = (emb, cluster_ref.cosine64(emb), info)
    return _DATA[N]


@pytest.mark.parametrize('N', [20, 33, 129, 168])
def test_the_two_oracle_forms_agree(N):
    emb, S, info = bridged(N)
    assert cluster_ref.margin(S, THR) > MARGIN
    for min_rows in range(1, 7):
        state = rref.full_state(S, THR, min_rows)
        for name, keep in rref.patterns(S, THR, info, seed=N * 10 + min_rows, n_random=6):
            got = rref.remove_from_scores(S, THR, min_rows, state, keep)
            want = rref.survivors_only(S, THR, min_rows, keep)
            assert rref.same(got, want), (N, min_rows, name)
            assert np.all(got[0][~keep] == -1) and np.all(got[0][keep] >= 0) and not got[1][~keep].any() and not got[2][~keep].any()
            r, m, q = got[4]
            assert r == int((~keep).sum())
            if name == 'nothing':
                assert (m, q) == (0, 0) and np.array_equal(got[0], state[0]) and np.array_equal(got[2], state[1])
            if name == 'everything':
                assert (m, q) == (0, 0)
            if min_rows == 1:                               # every row is core: no row ever chooses
                assert q == 0


def test_removing_a_border_or_noise_row_hits_nothing():
    emb, S, info = bridged(168)
    state = rref.full_state(S, THR, 4)
    kind = dref.density_oracle(S, THR, 4)[1]
    for k in (0, 1):
        for x in np.nonzero(kind == k)[0][:3].tolist():
            got = rref.remove_from_scores(S, THR, 4, state, rref.keep_without(168, [x]))
            assert got[4][1] == 0, (k, x)


def test_every_transition_occurs_at_33_rows_and_min_rows_5():
    emb, S, info = bridged(33)
    state = rref.full_state(S, THR, 5)
    kind = dref.density_oracle(S, THR, 5)[1]
    seen = {}
    for name, keep in rref.patterns(S, THR, info, seed=335, n_random=6):
        got = rref.remove_from_scores(S, THR, 5, state, keep)
        for k, v in xref.transitions(kind[keep], got[1][keep]).items():
            seen[k] = seen.get(k, 0) + v
    assert seen.get((2, 1), 0) > 0 and seen.get((2, 0), 0) > 0 and seen.get((1, 0), 0) > 0, seen
    assert all(a > b for a, b in seen)                      # a removal never raises a kind


def case(which):
    rows, thr, min_rows, remove, named = rref.constructed(which)
    S = cluster_ref.cosine64(rows)
    assert cluster_ref.margin(S, thr) > MARGIN
    keep = rref.keep_without(128, remove)
    state = rref.full_state(S, thr, min_rows)
    before = dref.density_oracle(S, thr, min_rows)
    got = rref.remove_from_scores(S, thr, min_rows, state, keep)
    assert rref.same(got, rref.survivors_only(S, thr, min_rows, keep)), which
    return named, state, before, got


def test_constructed_switch_and_tie():
    for which, to in (('switch', 'B'), ('tie', 'C')):
        named, state, (rep0, kind0, _), (rep, kind, _, (_, brow), counts) = case(which)
        A, x = named['A'], named['x'][0]
        assert x == 0 and kind0[x] == 1 and state[2][1][x] == A[0] and set(rep0[A].tolist()) == {0}
        assert counts == (1, 5, 1)
        assert kind[x] == 1 and brow[x] == named[to][0] and set(rep[named[to]].tolist()) == {0} and rep[x] == 0
        assert set(rep[A[1:]].tolist()) == {A[1]} and rep[A[0]] == -1
        if which == 'tie':
            assert named['C'][0] < named['B'][0] and set(rep[named['B']].tolist()) == {named['B'][0]}


def test_constructed_to_noise():
    named, state, (rep0, kind0, _), (rep, kind, degree, (_, brow), counts) = case('to_noise')
    D, y = named['D'], named['y'][0]
    assert kind0[y] == 1 and set(kind0[D].tolist()) == {2}
    left = [D[0], D[3], D[4]]
    assert counts == (2, 0, 4) and not kind[left + [y]].any() and rep[left + [y]].tolist() == left + [y] and (brow < 0).all()
    assert degree[D[0]] == 3 and degree[y] == 1


def test_constructed_split():
    named, state, (rep0, kind0, _), (rep, kind, _, (_, brow), counts) = case('split')
    E, F, z = named['E'], named['F'], named['z'][0]
    assert kind0[z] == 2 and len(set(rep0[E + F + [z] + named['w']].tolist())) == 1
    assert counts == (1, 10, 1)
    assert set(rep[E].tolist()) == {E[0]} and set(rep[F + [z]].tolist()) == {F[0]} and kind[z] == 1 and brow[z] == F[0]


def test_constructed_no_cascade():
    named, state, (rep0, kind0, deg0), (rep, kind, degree, (_, brow), counts) = case('no_cascade')
    H, v = named['H'], named['v'][0]
    assert kind0[H].tolist() == [2, 2, 2, 1] and kind0[v] == 2 and deg0[H[:3]].tolist() == [4, 4, 4]
    assert counts == (1, 3, 1)
    assert kind[H].tolist() == [2, 2, 2, 1] and degree[H[:3]].tolist() == [4, 4, 4]       # core through v, which still counts
    assert kind[v] == 1 and brow[v] == H[0] and degree[v] == 3 and set(rep[H + [v]].tolist()) == {H[0]}


def test_constructed_rep_rises():
    named, state, (rep0, kind0, _), (rep, kind, _, _, counts) = case('rep_rises')
    members, u = named['I'], named['u'][0]
    assert u == 0 and kind0[u] == 1 and set(rep0[members].tolist()) == {0}
    assert counts == (1, 0, 0) and set(rep[members].tolist()) == {members[0]} and set(kind[members].tolist()) == {2}


def test_a_void_key_is_looked_for_again_and_every_index_stays_in_range():
    emb, S, info = bridged(168)
    rep, degree, (bs, br) = rref.full_state(S, THR, 4)
    kind = dref.density_oracle(S, THR, 4)[1]
    border = int(np.nonzero(kind == 1)[0][0])
    noise = int(np.nonzero(kind == 0)[0][0])
    br = br.copy()
    br[border] = noise                                      # a key that names a row which is not core
    keep = np.ones(168, dtype=bool)
    got = rref.remove_from_scores(S, THR, 4, (rep, degree, (bs, br)), keep)
    assert got[4] == (0, 0, 1) and rref.same(got, rref.survivors_only(S, THR, 4, keep))


# ---- the host side over a stub engine ---------------------------------------------------------------------------------

def unkeys(best):
    """the int64 keys of the binding -> (score[n] float32, row[n]) of the oracle's state"""
    k = np.asarray(best).view(np.uint64)
    has = k != 0
    o = (k >> np.uint64(32)).astype(np.uint32)
    u = np.where(o >> np.uint32(31), o ^ np.uint32(0x80000000), ~o)
    score = np.where(has, u.astype(np.uint32).view(np.float32), -np.inf).astype(np.float32)
    row = np.where(has, np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF)), 0).astype(np.int64)
    return score, np.where(has, row, -1)


def scores32(emb):
    return cluster_ref.cosine64(np.asarray(emb)).astype(np.float32)


class StubEngine(object):
    """Answers row_norms, cluster_density_extend and cluster_density_remove on the CPU from the oracles (fp32 scores, the
    keys in the binding's int64 form), and records the calls."""
    device = torch.device('cpu')

    def __init__(self):
        self.remove_calls, self.extend_calls = [], []

    def _min_rows(self, min_rows, who):
        assert min_rows >= 1

    def row_norms(self, x):
        return x.double().norm(dim=1).float()

    def cluster_density_extend(self, emb, threshold, min_rows, rep, degree, best, n_old, norms=None, validate=True):
        self.extend_calls.append((emb.size(0), n_old))
        state = xref.empty_state(np.float32) if n_old == 0 else (rep[:n_old].numpy(), degree[:n_old].numpy(), unkeys(best[:n_old].numpy()))
        got = xref.extend_from_scores(scores32(emb.numpy()), threshold, min_rows, n_old, state)
        out = [torch.from_numpy(got[0]), torch.from_numpy(got[1]), torch.from_numpy(got[2]), torch.from_numpy(xref.keys(got[3]))]
        for t, o in ((rep, out[0]), (degree, out[2]), (best, out[3])):
            if t is not None and t.numel() == emb.size(0):
                t.copy_(o)
        return tuple(out)

    def cluster_density_remove(self, emb, threshold, min_rows, rep, degree, best, keep, norms=None, validate=True):
        self.remove_calls.append(dict(n=emb.size(0), keep=keep.clone(), validate=validate, state=(rep.data_ptr(), degree.data_ptr(), best.data_ptr())))
        got = rref.remove_from_scores(scores32(emb.numpy()), threshold, min_rows, (rep.numpy().copy(), degree.numpy().copy(), unkeys(best.numpy())),
                                      keep.numpy())
        rep.copy_(torch.from_numpy(got[0]))
        degree.copy_(torch.from_numpy(got[2]))
        best.copy_(torch.from_numpy(xref.keys(got[3])))
        return rep, torch.from_numpy(got[1]), degree, best


def test_unkeys_inverts_keys():
    best = (np.array([0.8, -0.25, 0.0, -np.inf], dtype=np.float32), np.array([3, 7, 0, -1]))
    score, row = unkeys(xref.keys(best))
    assert row.tolist() == [3, 7, 0, -1] and score[:3].tolist() == best[0][:3].tolist()


def scratch_state(eng, x, min_rows=4):
    return fc.density_extend(eng, x, THR, min_rows)


def assert_state_equal(a, b):
    for f in ('rep', 'kind', 'degree', 'best'):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.threshold == b.threshold and a.min_rows == b.min_rows


def test_density_remove_returns_compact_clusters_state_and_maps():
    emb, S, info = bridged(168)
    x = torch.from_numpy(emb)
    eng = StubEngine()
    c0, s0 = scratch_state(eng, x)
    frozen = [t.clone() for t in (s0.rep, s0.kind, s0.degree, s0.best)]
    rows = [info['ident'][0][0], info['bridge'][0], 5, 5, 167]
    keep = rref.keep_without(168, rows)
    c, s, old_to_new, kept = fc.density_remove(eng, x, THR, 4, s0, rows=rows)
    want_c, want_s = scratch_state(eng, x[torch.from_numpy(keep)])
    assert isinstance(c, fc.DensityClusters) and isinstance(s, fc.DensityState)
    assert_state_equal(s, want_s)                                              # the keys name the compact rows
    assert torch.equal(c.rep, want_c.rep) and torch.equal(c.has_core, want_c.has_core) and c.n_clusters == want_c.n_clusters
    assert bool((s.best != 0).any())
    assert kept.tolist() == np.nonzero(keep)[0].tolist() and torch.equal(old_to_new[kept], torch.arange(kept.numel()))
    assert all(old_to_new[r] == -1 for r in rows)
    # earlier is left as it is, the engine got copies and validates
    assert all(torch.equal(a, b) for a, b in zip(frozen, (s0.rep, s0.kind, s0.degree, s0.best)))
    call = eng.remove_calls[-1]
    assert call['validate'] and call['state'][0] != s0.rep.data_ptr() and call['keep'].tolist() == keep.tolist()
    # the mask form
    c2, s2, o2, k2 = fc.density_remove(eng, x, THR, 4, s0, keep=torch.from_numpy(keep))
    assert_state_equal(s2, s) and torch.equal(o2, old_to_new)
    # nothing, everything
    c3, s3, o3, k3 = fc.density_remove(eng, x, THR, 4, s0, rows=[])
    assert_state_equal(s3, s0) and torch.equal(o3, torch.arange(168))
    c4, s4, o4, k4 = fc.density_remove(eng, x, THR, 4, s0, rows=torch.arange(168))
    assert c4.n_clusters == 0 and s4.rep.numel() == 0 and s4.best.numel() == 0 and bool((o4 == -1).all())
    # refused: a foreign state, both or neither of rows and keep, a state of another size
    for thr, m in ((0.4, 4), (THR, 5)):
        with pytest.raises(RuntimeError):
            fc.density_remove(eng, x, thr, m, s0, rows=[1])
    for kw in (dict(), dict(rows=[1], keep=torch.from_numpy(keep))):
        with pytest.raises(ValueError):
            fc.density_remove(eng, x, THR, 4, s0, **kw)
    with pytest.raises(RuntimeError):
        fc.density_remove(eng, x[:100], THR, 4, s0, rows=[1])


def test_rekey_renumbers_the_low_word_only():
    o2n = torch.tensor([-1, 0, 1, -1, 2])
    hi = [0x3F4CCCCD, -0x40000000]                              # the score word, the second with its top bit set
    best = torch.tensor([0, (hi[0] << 32) | (0xFFFFFFFF - 2), (hi[1] << 32) | (0xFFFFFFFF - 4)], dtype=torch.int64)
    got = fc._rekey(best, o2n)
    assert got[0] == 0 and got.dtype == torch.int64
    assert [int(v) >> 32 for v in got[1:]] == hi and [0xFFFFFFFF - (int(v) & 0xFFFFFFFF) for v in got[1:]] == [1, 2]


def test_density_removal_changes():
    # cluster 0 = {0, 1, 2}, cluster 3 = {3, 4}, cluster 5 = {5, 6, 7}, 8 alone
    before = torch.tensor([0, 0, 0, 3, 3, 5, 5, 5, 8])
    # row 4 leaves; the border row 2 moves from cluster 0 to cluster 5, which lost nothing
    after = torch.tensor([0, 0, 2, 3, -1, 2, 2, 2, 8])
    drop, compute = fc.density_removal_changes(before, after)
    assert drop.dtype == torch.int64 and drop.tolist() == [0, 3, 5] and compute.tolist() == [0, 2, 3]
    assert fc.removal_changes(before, after)[0].tolist() == [3]             # the single-link form misses both
    for same in (before, fc.DensityState(before, None, None, None, THR, 4)):
        drop, compute = fc.density_removal_changes(same, before)
        assert drop.tolist() == [] and compute.tolist() == []
    drop, compute = fc.density_removal_changes(before, torch.full((9,), -1))
    assert drop.tolist() == [0, 3, 5, 8] and compute.tolist() == []
    # the representative leaves: the label rises, nothing else changes
    drop, compute = fc.density_removal_changes(before, torch.tensor([-1, 1, 1, 3, 3, 5, 5, 5, 8]))
    assert drop.tolist() == [0] and compute.tolist() == [1]
    with pytest.raises(ValueError):
        fc.density_removal_changes(before, after[:3])
    assert 'density_removal_changes' in fc.changes.__doc__


def test_routing_rule():
    assert fc.density_remove_route(131072, 131072 - 256) == 'remove'
    assert fc.density_remove_route(131072, 65536) == 'recluster'
    assert fc.density_remove_route(16384, 16384 - 256) == 'remove'
    assert fc.density_remove_route(100, 0) == 'recluster'
    n = 1000
    for ns in range(0, n + 1, 37):
        assert fc.density_remove_route(n, ns) == ('remove' if (n - ns) * n <= fc.REMOVE_PAIR_RATIO * ns * (ns - 1) else 'recluster')
    assert 0 < fc.REMOVE_PAIR_RATIO <= 1.0                      # never more removal than the plain pair count allows


@pytest.mark.parametrize('route', ['remove', 'recluster', None])
def test_incremental_density_remove_then_add(route):
    emb, S, info = bridged(168)
    x = torch.from_numpy(emb)
    eng = StubEngine()
    inc = fc.IncrementalDensity(eng, THR, 4, capacity=64)
    inc.add(x[:100])
    inc.add(x[100:])
    assert torch.equal(inc.remove([], route=route), torch.arange(168)) and not eng.remove_calls and len(inc) == 168
    rows = [info['ident'][0][0], info['bridge'][0], 0, 0]
    keep = rref.keep_without(168, rows)
    kept = np.nonzero(keep)[0]
    before = inc.rep.clone()
    n_ext = len(eng.extend_calls)
    old_to_new = inc.remove(rows, route=route)
    if route == 'recluster':
        assert not eng.remove_calls and eng.extend_calls[n_ext:] == [(kept.size, 0)]
    else:                                                       # three rows of 168: the rule takes the removal
        call = eng.remove_calls[-1]
        assert call['n'] == 168 and not call['validate'] and call['keep'].tolist() == keep.tolist() and len(eng.extend_calls) == n_ext
    assert len(inc) == kept.size and old_to_new.tolist() == [int(keep[:i].sum()) if k else -1 for i, k in enumerate(keep)]
    assert torch.equal(inc.embeddings, x[kept]) and torch.equal(inc.norms, x[kept].double().norm(dim=1).float())
    want_c, want_s = scratch_state(StubEngine(), x[kept])
    assert_state_equal(inc.state, want_s)
    assert inc.clusters.n_clusters == want_c.n_clusters and before.numel() == 168
    # add after remove: the rows that left come back at the end; the state is that of one clustering of the rows held
    back = sorted(set(rows))
    assert inc.add(x[back]) == kept.size and len(inc) == 168
    held = torch.cat((x[kept], x[back]))
    assert_state_equal(inc.state, scratch_state(StubEngine(), held)[1])
    # everything leaves, then a new start
    assert bool((inc.remove(torch.arange(168), route=route) == -1).all()) and len(inc) == 0 and inc.clusters.n_clusters == 0
    assert inc.add(x[:40]) == 0
    assert_state_equal(inc.state, scratch_state(StubEngine(), x[:40])[1])
    with pytest.raises(RuntimeError):
        inc.remove([40])
    with pytest.raises(ValueError):
        inc.remove([1], route='other')


def test_both_routes_leave_the_identical_state():
    emb, S, info = bridged(168)
    x = torch.from_numpy(emb)
    states = []
    for route in ('remove', 'recluster'):
        inc = fc.IncrementalDensity(StubEngine(), THR, 5)
        inc.add(x)
        inc.remove(list(range(0, 168, 3)), route=route)
        states.append(inc.state)
    assert_state_equal(*states)


def test_docstrings_no_longer_say_there_is_no_removal():
    from ffrnet_amd import native
    for doc in (fc.__doc__, fc.remove.__doc__, fc.IncrementalDensity.__doc__, native.Engine.cluster_remove.__doc__):
        assert 'there is no removal' not in doc and 'index for ever' not in doc
    hdr = open(os.path.join(ROOT, 'include', 'ffrnet.h')).read()
    assert 'is not offered' not in hdr


def test_header_prototype_and_binding():
    hdr = open(os.path.join(ROOT, 'include', 'ffrnet.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\bint\s+ffr_cluster_density_remove\s*\(([^;{}]*)\)\s*;', hdr)
    assert m
    params = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert [a.split()[-1].lstrip('*') for a in params] == ['h', 'emb', 'norms', 'N', 'dim', 'threshold', 'min_rows', 'keep', 'rep',
                                                           'kind', 'degree', 'best', 'stream']
    assert params[7] == 'const uint8_t* keep' and params[8] == 'int64_t* rep' and params[11] == 'unsigned long long* best'
    from ffrnet_amd import native
    row = [r for r in native.SYMBOLS if r[0] == 'ffr_cluster_density_remove']
    assert len(row) == 1 and len(row[0][2]) == 13
    assert callable(native.Engine.cluster_density_remove)
