"""Removal from a density-gated clustering on the device (include/ffrnet.h: ffr_cluster_density_remove;
Engine.cluster_density_remove, cluster.density_remove, cluster.IncrementalDensity.remove).

The contract under test: after a removal the labels AND the state equal those of clustering the surviving rows alone --
torch.equal with Engine.cluster_density and Engine.cluster_density_extend(n_old = 0) over the compacted rows, the keys
re-encoded through the renumbering -- and equal both forms of the float64 oracle of tests/cluster_density_remove_ref.py
wherever no float64 score lies within 1e-3 of the threshold (the library's fp32 score is within 1e-6 of the float64 cosine;
every such test asserts that margin first).  Where there is no margin (thresholds taken from the scores themselves) the
reference is the device's own clustering of the compacted rows, bit for bit: the walks meet pairs with the roles exchanged
and must compute the bits of the triangle."""
import ctypes as C

import numpy as np
import pytest
import torch

import cluster_density_extend_ref as xref
import cluster_density_ref as dref
import cluster_density_remove_ref as rref
import cluster_ref
import cluster_remove_ref as sref
import ffrnet_amd
from ffrnet_amd import cluster as fc
from ffrnet_amd import native

pytestmark = pytest.mark.gpu

THR = 0.5
MARGIN = 1e-3          # against the documented 1e-6 error of a score
_DATA, _FULL, _OSTATE = {}, {}, {}
PATTERNS = ['member', 'outlier', 'bridge', 'every_second', 'row0', 'nothing', 'everything', 'random0', 'random1']


def bridged(N):
    """(emb float32 numpy, float64 scores, info, the removal patterns) of planted_bridged(N), computed once, read-only."""
    if N not in _DATA:
        emb, truth, info = dref.planted_bridged(N)
        S = cluster_ref.cosine64(emb)
        pats = dict(rref.patterns(S, THR, info, seed=N, n_random=2))
        for a in (emb, S) + tuple(pats.values()):
            a.setflags(write=False)
        _DATA[N] = (emb, S, info, pats, cluster_ref.margin(S, THR))
    return _DATA[N][:4]


def margin(N):
    bridged(N)
    return _DATA[N][4]


@pytest.fixture(scope='module')
def eng():
    return ffrnet_amd.Engine(0)


@pytest.fixture(scope='module')
def synth_rows(state_dicts):
    """f_new of 128 synthetic images: embeddings of the real network, strongly correlated."""
    e = ffrnet_amd.Engine(0)
    e.load_encoder(state_dicts[0])
    e.load_recnet(state_dicts[1])
    f_new, _ = e.embed(ffrnet_amd.synth.synth_images(128, seed=77).cuda(), want_f=False)
    torch.cuda.synchronize()
    e.close()
    return f_new


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the shared arrays are read-only


def arange(lo, hi):
    return torch.arange(lo, hi, device='cuda', dtype=torch.int64)


def from_scratch(eng, emb, thr, m):
    return eng.cluster_density_extend(emb, thr, m, None, None, None, 0)


def full(eng, N, m):
    """the device state (rep, kind, degree, best) of all rows of bridged(N), computed once and left unchanged"""
    if (N, m) not in _FULL:
        _FULL[(N, m)] = from_scratch(eng, dev(bridged(N)[0]), THR, m)
    return _FULL[(N, m)]


def oracle_state(N, m):
    if (N, m) not in _OSTATE:
        _OSTATE[(N, m)] = rref.full_state(bridged(N)[1], THR, m)
    return _OSTATE[(N, m)]


def remove(eng, d, thr, m, state, keep, **kw):
    """Engine.cluster_density_remove on copies of the state -> (rep, kind, degree, best)"""
    return eng.cluster_density_remove(d, thr, m, state[0].clone(), state[2].clone(), state[3].clone(), keep, **kw)


def compacted(got, keep):
    """a device result in the old numbering -> (rep, kind, degree, best) of the survivors in compact numbering"""
    old_to_new = torch.full((keep.numel(),), -1, device='cuda', dtype=torch.int64)
    old_to_new[keep] = arange(0, int(keep.sum()))
    return old_to_new[got[0][keep]], got[1][keep], got[2][keep], fc._rekey(got[3][keep], old_to_new)


def assert_equals_the_rest(eng, d, thr, m, got, keep, what):
    """the removed rows carry -1 / 0 / 0 / 0; the survivors, compacted, are cluster_density and the state from scratch"""
    assert [t.dtype for t in got] == [torch.int64, torch.uint8, torch.int32, torch.int64]
    gone = ~keep
    assert bool((got[0][gone] == -1).all()) and not bool(got[1][gone].any()) and not bool(got[2][gone].any()) and not bool(got[3][gone].any())
    if not bool(keep.any()):
        return
    rest = d[keep].contiguous()
    want = eng.cluster_density(rest, thr, m, return_degree=True)
    state = from_scratch(eng, rest, thr, m)
    c = compacted(got, keep)
    for name, g, w in zip(('rep', 'kind', 'degree'), c, want):
        assert torch.equal(g, w), (name, what, torch.nonzero(g != w).reshape(-1)[:8].tolist())
    assert torch.equal(c[3], state[3]), ('best', what, torch.nonzero(c[3] != state[3]).reshape(-1)[:8].tolist())


def assert_equals_the_oracles(got, S, thr, m, ostate, keep_np, what):
    """rep, kind, degree and the core row of every key against both oracle forms (the score word is fp32 on the device)"""
    a = rref.remove_from_scores(S, thr, m, ostate, keep_np)
    b = rref.survivors_only(S, thr, m, keep_np)
    assert rref.same(a, b), what
    g = [t.cpu().numpy() for t in got]
    assert np.array_equal(g[0], a[0]) and np.array_equal(g[1], a[1]) and np.array_equal(g[2], a[2]), what
    named = np.where(g[3] != 0, 0xFFFFFFFF - (g[3] & 0xFFFFFFFF), -1)
    assert np.array_equal(named, a[3][1]), what
    return a[4]


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('m', [1, 2, 4, 5])
@pytest.mark.parametrize('N', [20, 33, 129, 168, 1000, 4129])
def test_removal_equals_clustering_the_rest(eng, N, m, pattern):
    emb, S, info, pats = bridged(N)
    assert margin(N) > MARGIN
    d, state = dev(emb), full(eng, N, m)
    keep_np = pats[pattern]
    keep = dev(keep_np)
    got = remove(eng, d, THR, m, state, keep)
    counts = assert_equals_the_oracles(got, S, THR, m, oracle_state(N, m), keep_np, (N, m, pattern))
    print('N %d min_rows %d %s: r, m, q = %s' % (N, m, pattern, counts))
    assert_equals_the_rest(eng, d, THR, m, got, keep, (N, m, pattern))
    if pattern == 'nothing':
        assert all(torch.equal(g, w) for g, w in zip(got, state))
    if pattern == 'everything':
        assert bool((got[0] == -1).all())
    if m == 1:                                              # single link: the other removal, bit for bit
        assert torch.equal(got[0], eng.cluster_remove(d, THR, state[0], keep))


def clique_clusters(S, thr, m):
    """the clusters of the oracle in which every member is core and adjacent to every other member -> [members]"""
    rep, kind, degree = dref.density_oracle(S, thr, m)
    out = []
    for r in np.unique(rep[kind == 2]):
        members = np.nonzero(rep == r)[0]
        if np.all(kind[members] == 2) and np.all(degree[members] == members.size - 1):
            out.append(members)
    return out


def rows_for(which, count, N, S):
    """-> (min_rows, rows to remove) so that list `which` gets exactly `count` entries (the oracle confirms it in the test)"""
    if count == 0:
        return 5, []
    if which == 'r':                                        # noise rows have no core neighbour: nothing else is listed
        rep, kind, degree = dref.density_oracle(S, THR, 5)
        return 5, np.nonzero(kind == 0)[0][:count].tolist() if int((kind == 0).sum()) >= count else None
    if which == 'm':                                        # min_rows 1 is single link: the affected survivors are listed
        rep = cluster_ref.union_find(N, cluster_ref.upper_edges(S, THR))
        return 1, sref.pick_clusters_for(rep, count)
    # q at min_rows 5: a clique cut down to 4 - k rows demotes them all, 4 at a time and the remainder last
    rows, left = [], count
    for members in clique_clusters(S, THR, 5):
        take = min(left, 4)
        rows += members[:members.size - take].tolist()
        left -= take
        if left == 0:
            return 5, rows
    return 5, None


@pytest.mark.parametrize('count', [0, 1, 2, 31, 32, 33, 127, 128, 129, 513])
@pytest.mark.parametrize('which', ['r', 'm', 'q'])
def test_list_boundaries(eng, which, count):
    # tile (32), step (128) and multi-step edges of k_list_walk in each of the three lists
    N = 1000 if count <= 129 else 4129
    emb, S, info, pats = bridged(N)
    assert margin(N) > MARGIN
    m, rows = rows_for(which, count, N, S)
    assert rows is not None
    keep_np = sref.keep_without(N, rows)
    d, keep = dev(emb), dev(keep_np)
    got = remove(eng, d, THR, m, full(eng, N, m), keep)
    counts = assert_equals_the_oracles(got, S, THR, m, oracle_state(N, m), keep_np, (which, count))
    assert counts['rmq'.index(which)] == count, counts      # the count the device reaches, from the oracle
    assert_equals_the_rest(eng, d, THR, m, got, keep, (which, count))


def test_no_margin_equals_the_compacted_rows_bitwise(eng, synth_rows):
    emb = synth_rows
    n = emb.size(0)
    s, i = eng.search(emb, emb, n)
    S = torch.full((n, n), float('nan'), device='cuda').scatter_(1, i, s)
    assert not torch.isnan(S).any()
    Sn = S.cpu().numpy()
    ranked = torch.sort(S[torch.triu(torch.ones_like(S, dtype=torch.bool), 1)]).values
    # each threshold IS one of the scores, so the strict > is exercised on equal bits
    picks = [ranked[int(q * (ranked.numel() - 1))].item() for q in (0.5, 0.9, 0.97, 0.99, 0.997)]
    listed, kinds = np.zeros(3, dtype=np.int64), set()
    for thr in picks:
        for m in (3, 6):
            state = from_scratch(eng, emb, thr, m)
            ostate = rref.full_state(Sn, np.float32(thr), m)
            for rows in ([0], [n - 1], list(range(0, n, 5)), list(range(64, 96))):
                keep = torch.ones(n, device='cuda', dtype=torch.bool)
                keep[rows] = False
                got = remove(eng, emb, thr, m, state, keep)
                assert_equals_the_rest(eng, emb, thr, m, got, keep, (thr, m, rows[:4]))
                o = rref.remove_from_scores(Sn, np.float32(thr), m, ostate, keep.cpu().numpy())
                assert np.array_equal(got[3].cpu().numpy(), xref.keys(o[3])), (thr, m, rows[:4])      # fp32 scores: the whole key
                listed += o[4]
                kinds |= set(o[1].tolist())
    assert listed.all() and kinds == {0, 1, 2}              # every list was walked, and not one blob throughout


@pytest.mark.parametrize('which', rref.CONSTRUCTED)
def test_constructed(eng, which):
    rows, thr, m, gone, named = rref.constructed(which)
    d = dev(rows)
    s, i = eng.search(d, d, 128)
    Sn = torch.full((128, 128), float('nan'), device='cuda').scatter_(1, i, s).cpu().numpy()
    keep_np = sref.keep_without(128, gone)
    keep = dev(keep_np)
    state = from_scratch(eng, d, thr, m)
    ostate = rref.full_state(Sn, np.float32(thr), m)
    assert np.array_equal(state[3].cpu().numpy(), xref.keys(ostate[2]))
    got = remove(eng, d, thr, m, state, keep)
    o = rref.remove_from_scores(Sn, np.float32(thr), m, ostate, keep_np)
    assert rref.same(o, rref.survivors_only(Sn, np.float32(thr), m, keep_np))
    for g, w in zip(got[:3], o[:3]):
        assert np.array_equal(g.cpu().numpy(), w), which
    assert np.array_equal(got[3].cpu().numpy(), xref.keys(o[3])), which
    assert_equals_the_rest(eng, d, thr, m, got, keep, which)
    want = dict(switch=(1, 5, 1), tie=(1, 5, 1), to_noise=(2, 0, 4), split=(1, 10, 1), no_cascade=(1, 3, 1), rep_rises=(1, 0, 0))
    assert o[4] == want[which]
    rep, kind = got[0].cpu().numpy(), got[1].cpu().numpy()
    if which in ('switch', 'tie'):
        to = named['B' if which == 'switch' else 'C']
        assert rep[0] == 0 and set(rep[to].tolist()) == {0} and set(rep[named['A'][1:]].tolist()) == {named['A'][1]}
    if which == 'to_noise':
        assert not kind[keep_np].any()
    if which == 'split':
        assert rep[named['z'][0]] == named['F'][0] != rep[named['E'][0]] and kind[named['z'][0]] == 1
    if which == 'no_cascade':
        assert kind[named['H']].tolist() == [2, 2, 2, 1] and kind[named['v'][0]] == 1
    if which == 'rep_rises':
        assert set(rep[named['I']].tolist()) == {named['I'][0]}


@pytest.mark.parametrize('route', ['remove', 'recluster'])
def test_add_remove_add_remove(eng, route):
    emb, S, info, pats = bridged(1000)
    assert margin(1000) > MARGIN
    d = dev(emb)
    inc = fc.IncrementalDensity(eng, THR, 4)
    ids = arange(0, 0)                                      # the side table a caller keeps

    def check():
        held = d[ids].contiguous()
        once, state = fc.density_extend(eng, held, THR, 4)
        whole = fc.density(eng, held, THR, 4)
        assert len(inc) == ids.numel() and torch.equal(inc.embeddings, held) and torch.equal(inc.norms, eng.row_norms(held))
        assert torch.equal(inc.rep, whole.rep) and torch.equal(inc.kind, whole.kind)
        for f in ('rep', 'kind', 'degree', 'best'):
            assert torch.equal(getattr(inc.state, f), getattr(state, f)), f
        sub = ids.cpu().numpy()
        o = dref.density_oracle(S[np.ix_(sub, sub)], THR, 4)
        assert np.array_equal(inc.rep.cpu().numpy(), o[0]) and np.array_equal(inc.kind.cpu().numpy(), o[1])
        return [t.clone() for t in inc.state[:4]]

    def renumber(old_to_new):
        out = torch.empty((int((old_to_new >= 0).sum()),), device='cuda', dtype=torch.int64)
        out[old_to_new[old_to_new >= 0]] = ids[old_to_new >= 0]
        return out

    trail = []
    assert inc.add(d[:600]) == 0
    ids = arange(0, 600)
    trail.append(check())
    ids = renumber(inc.remove(arange(0, 200), route=route))     # the oldest rows expire
    assert torch.equal(ids, arange(200, 600))
    trail.append(check())
    assert inc.add(d[600:]) == 400
    ids = torch.cat((ids, arange(600, 1000)))
    trail.append(check())
    gone = np.random.default_rng(3).choice(800, 100, replace=False)
    ids = renumber(inc.remove(gone, route=route))
    trail.append(check())
    assert torch.equal(inc.templates(), fc.templates(eng, inc.embeddings, inc.clusters)[inc.clusters.has_core])
    _FULL[('trail', route)] = trail
    other = _FULL.get(('trail', 'recluster' if route == 'remove' else 'remove'))
    if other is not None:                                   # both routes leave the identical state at every step
        assert all(torch.equal(a, b) for sa, sb in zip(_FULL[('trail', route)], other) for a, b in zip(sa, sb))


def test_the_functional_form_and_the_changes(eng):
    emb, S, info, pats = bridged(168)
    d = dev(emb)
    c0, s0 = fc.density_extend(eng, d, THR, 4)
    frozen = [t.clone() for t in s0[:4]]
    rows = [info['ident'][0][0], info['bridge'][0], 0]
    c, s, old_to_new, kept = fc.density_remove(eng, d, THR, 4, s0, rows=rows)
    want_c, want_s = fc.density_extend(eng, d[kept].contiguous(), THR, 4)
    for f in ('rep', 'kind', 'degree', 'best'):
        assert torch.equal(getattr(s, f), getattr(want_s, f)), f
    assert torch.equal(c.rep, want_c.rep) and torch.equal(c.has_core, want_c.has_core)
    assert all(torch.equal(a, b) for a, b in zip(frozen, s0[:4]))          # earlier is left as it is
    # the state goes on: an extension after the removal equals clustering everything held
    more = torch.cat((d[kept], d[rows])).contiguous()
    c2, s2 = fc.density_extend(eng, more, THR, 4, earlier=s)
    assert torch.equal(c2.rep, fc.density(eng, more, THR, 4).rep)
    assert torch.equal(s2.best, fc.density_extend(eng, more, THR, 4)[1].best)
    # the changes, on the labels before compaction: every cluster outside drop / compute kept its rows and its label
    keep = old_to_new >= 0
    after = remove(eng, d, THR, 4, s0, keep)[0]
    drop, compute = fc.density_removal_changes(s0, after)
    still = keep & ~torch.isin(s0.rep, drop)
    assert bool((after[still] == s0.rep[still]).all()) and not bool(torch.isin(after[still], compute).any())
    assert bool(torch.isin(s0.rep[~keep], drop).all()) and bool(torch.isin(after[keep & torch.isin(s0.rep, drop)], compute).all())
    with pytest.raises(RuntimeError):
        fc.density_remove(eng, d, THR, 5, s0, rows=rows)


def test_repeatable_and_in_place(eng):
    emb, S, info, pats = bridged(1000)
    d = dev(emb)
    state = full(eng, 1000, 4)
    keep = dev(pats['every_second'])
    a = remove(eng, d, THR, 4, state, keep)
    b = remove(eng, d, THR, 4, state, keep, norms=eng.row_norms(d))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    rep, degree, best = state[0].clone(), state[2].clone(), state[3].clone()
    out = eng.cluster_density_remove(d, THR, 4, rep, degree, best, keep)
    assert out[0].data_ptr() == rep.data_ptr() and out[2].data_ptr() == degree.data_ptr() and out[3].data_ptr() == best.data_ptr()
    assert all(torch.equal(x, y) for x, y in zip(a, out))


def test_wrong_but_in_range_state_returns_consistent_labels(eng):
    N = 1000
    emb, S, info, pats = bridged(N)
    d = dev(emb)
    good = full(eng, N, 4)
    g = torch.Generator(device='cuda')
    g.manual_seed(5)
    row = arange(0, N)
    for trial in range(3):
        rep = (torch.rand((N,), device='cuda', generator=g) * (row + 1)).to(torch.int64).clamp(max=N - 1)     # 0 <= rep[i] <= i
        rep = torch.minimum(rep, row)
        degree = good[2] + torch.randint(0, 6, (N,), device='cuda', generator=g, dtype=torch.int32)           # inflated
        names = torch.randint(0, N, (N,), device='cuda', generator=g)                                         # any row of [0, N)
        best = torch.full((N,), 0x3F000000 << 32, device='cuda', dtype=torch.int64) | (0xFFFFFFFF - names)
        best[::3] = 0
        native.check_density_state(rep, degree, best)                             # in range: validate would not object
        keep = torch.rand((N,), device='cuda', generator=g) < 0.7
        out = eng.cluster_density_remove(d, THR, 4, rep, degree, best, keep, validate=False)
        torch.cuda.synchronize()
        r = out[0]
        assert bool((r[~keep] == -1).all()) and bool(((r[keep] >= 0) & (r[keep] < N)).all())
        assert bool(keep[r[keep]].all()) and torch.equal(r[r[keep]], r[keep])
        named = 0xFFFFFFFF - (out[3] & 0xFFFFFFFF)
        has = out[3] != 0
        assert bool((named[has] < N).all()) and bool(keep[named[has]].all()) and bool((out[2] >= 0).all())
        assert bool((out[1] <= 2).all()) and not bool(out[1][~keep].any())


def test_shares_the_scratch_and_profiles_one_launch():
    e = ffrnet_amd.Engine(0)
    ds, db = dev(bridged(168)[0]), dev(bridged(1000)[0])
    ss, sb = from_scratch(e, ds, THR, 4), from_scratch(e, db, THR, 4)
    ks, kb = dev(bridged(168)[3]['every_second']), dev(bridged(1000)[3]['every_second'])
    r1 = remove(e, ds, THR, 4, ss, ks)
    g1 = e.generation()
    assert all(torch.equal(a, b) for a, b in zip(r1, remove(e, ds, THR, 4, ss, ks))) and e.generation() == g1
    rb = remove(e, db, THR, 4, sb, kb)
    assert e.generation() != g1                             # a larger N grows the arena: captured graphs re-capture
    g2 = e.generation()
    assert torch.equal(e.cluster_density(ds, THR, 4)[0], ss[0])
    assert all(torch.equal(a, b) for a, b in zip(rb, remove(e, db, THR, 4, sb, kb))) and e.generation() == g2
    torch.cuda.synchronize()
    e.profile_enable(True)
    e.profile_read()
    remove(e, ds, THR, 4, ss, ks)
    st = e.profile_read()
    e.profile_enable(False)
    assert st['score']['launches'] == 1 and st['score']['flops'] == 0.0 and st['score']['ms'] > 0
    assert sum(v['launches'] for k, v in st.items() if k != 'score') == 0
    e.close()


def test_binding_errors(eng):
    g = torch.Generator(device='cuda')
    g.manual_seed(51)
    emb = torch.randn((100, 512), device='cuda', generator=g)
    norms = eng.row_norms(emb)
    rep, kind, degree, best = from_scratch(eng, emb, THR, 4)
    keep = torch.ones(100, device='cuda', dtype=torch.uint8)
    keep[::3] = 0
    kind.fill_(9)
    P = native._ptr
    null = C.c_void_p(0)
    ok = (P(emb), P(norms), 100, 512, THR, 4, P(keep), P(rep), P(kind), P(degree), P(best), eng._stream())
    names = ['emb', 'norms', 'N', 'dim', 'thr', 'min_rows', 'keep', 'rep', 'kind', 'degree', 'best', 'st']

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[names.index(key)] = v
        return eng.lib.ffr_cluster_density_remove(eng._h, *a)

    def message():
        return (eng.lib.ffr_last_error(eng._h) or b'').decode()

    assert call(dim=256) == -6 and '512' in message()
    for bad in (dict(N=-1), dict(N=1 << 31), dict(thr=float('nan')), dict(min_rows=0), dict(emb=null), dict(keep=null), dict(rep=null),
                dict(kind=null), dict(degree=null), dict(best=null), dict(emb=C.c_void_p(emb.data_ptr() + 4)),
                dict(rep=C.c_void_p(rep.data_ptr() + 4)), dict(best=C.c_void_p(best.data_ptr() + 4)),
                dict(degree=C.c_void_p(degree.data_ptr() + 2)), dict(norms=C.c_void_p(norms.data_ptr() + 2))):
        assert call(**bad) == -1, bad
        assert 'ffr_cluster_density_remove' in message(), bad
    torch.cuda.synchronize()
    assert bool((kind == 9).all())                          # refused before any launch: nothing was written
    assert call(N=0) == 0 and call(N=0, emb=null, keep=null, rep=null, kind=null, degree=null, best=null) == 0
    torch.cuda.synchronize()
    assert bool((kind == 9).all())
    assert call() == 0 and call(norms=null) == 0
    torch.cuda.synchronize()
    assert bool((rep[::3] == -1).all()) and bool((kind <= 2).all())
    # the binding: wrong device, shape, dtype, length; min_rows and threshold
    rep, kind, degree, best = from_scratch(eng, emb, THR, 4)
    kb = keep != 0
    good = dict(rep=rep, degree=degree, best=best, keep=kb)
    for bad in (dict(rep=rep.cpu()), dict(rep=rep.int()), dict(rep=rep[:99]), dict(degree=degree.to(torch.int64)), dict(degree=degree[:50]),
                dict(best=best.to(torch.float32)), dict(best=best[:50]), dict(keep=kb[:50]), dict(keep=kb.cpu()), dict(keep=kb.float()),
                dict(keep=kb.tolist())):
        a = dict(good, **bad)
        with pytest.raises(RuntimeError):
            eng.cluster_density_remove(emb, THR, 4, a['rep'], a['degree'], a['best'], a['keep'])
    for args in ((emb.cpu(), THR, 4), (emb[:, :256].contiguous(), THR, 4), (emb, THR, 0), (emb, THR, 2.5), (emb, float('nan'), 4)):
        with pytest.raises(RuntimeError):
            eng.cluster_density_remove(*args, rep.clone(), degree.clone(), best.clone(), kb)
    with pytest.raises(RuntimeError):
        eng.cluster_density_remove(emb, THR, 4, rep, degree, best, kb, norms=norms[:50])
    bad = rep.clone()
    bad[2] = 5
    with pytest.raises(RuntimeError):                       # validate: rep[i] > i
        eng.cluster_density_remove(emb, THR, 4, bad, degree, best, kb)
    none = eng.cluster_density_remove(emb[:0], THR, 4, rep[:0], degree[:0], best[:0], kb[:0])
    assert [t.shape for t in none] == [(0,)] * 4
