"""Extending a density-gated clustering on the device (include/ffrnet.h: ffr_cluster_density_extend;
ffrnet_amd.cluster.density_extend, IncrementalDensity).

The reference is always Engine.cluster_density over all N rows, compared with torch.equal: rep, kind and degree, and best
against the state a call from scratch leaves.  Where cluster_ref.margin(S, THR) > 1e-3 is asserted first, the float64
oracles (tests/cluster_density_extend_ref.py, tests/cluster_density_ref.py) are a reference too, and tell what a case
exercises; where there is no margin the oracle runs on the scores ffr_search_topk returns."""
import ctypes as C

import numpy as np
import pytest
import torch

import cluster_density_extend_ref as xref
import cluster_density_ref as dref
import cluster_ref
import ffrnet_amd
from ffrnet_amd import cluster as fc
from ffrnet_amd import native
from ffrnet_amd.search import Gallery

pytestmark = pytest.mark.gpu

THR = 0.5
MARGIN = 1e-3          # against the documented 1e-6 error of a score
MIN_ROWS = (3, 4, 5)
# 4129 = 4096 + 33: the first size where a chunk has several 128-row steps (test_gpu_cluster.py)
SPLITS = ([(20, 0), (20, 1), (33, 32), (129, 128), (129, 96)] + [(168, k) for k in (0, 1, 42, 84, 126, 128, 167, 168)] +
          [(257, 128)] + [(1000, k) for k in (31, 32, 33, 127, 128, 129, 500, 999)] + [(4129, k) for k in (1000, 4096, 4128)])
# (N, n_old, min_rows) -> (promoted rows, {(kind before, kind after): rows}): what the case is there for
COUNTS = {(168, 84, 4): (37, {(1, 2): 2}), (129, 96, 3): (8, {(0, 1): 1, (1, 2): 1}), (168, 167, 5): (3, {(1, 2): 3}),
          (257, 128, 4): (62, {(0, 1): 2}), (1000, 500, 5): (240, {(1, 2): 3})}
_BRIDGED, _FULL = {}, {}


def bridged(N):
    """(emb on the device, float64 scores or None above 1000 rows) of planted_bridged(N), computed once."""
    if N not in _BRIDGED:
        emb = dref.planted_bridged(N)[0]
        S = cluster_ref.cosine64(emb) if N <= 1000 else None
        if S is not None:
            S.setflags(write=False)
        _BRIDGED[N] = (torch.from_numpy(emb).cuda(), S)
    return _BRIDGED[N]


@pytest.fixture(scope='module')
def eng():
    return ffrnet_amd.Engine(0)


@pytest.fixture(scope='module')
def synth_rows(state_dicts):
    """f_new of 128 synthetic images: embeddings of the real network, strongly correlated (the recipe of test_gpu_cluster_density.py)."""
    e = ffrnet_amd.Engine(0)
    e.load_encoder(state_dicts[0])
    e.load_recnet(state_dicts[1])
    f_new, _ = e.embed(ffrnet_amd.synth.synth_images(128, seed=77).cuda(), want_f=False)
    torch.cuda.synchronize()
    e.close()
    return f_new


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def search_matrix(eng, emb):
    """S[i, j] = the score ffr_search_topk gives for probe i and gallery row j (the gallery in slices of 128 rows)."""
    n = emb.size(0)
    S = torch.full((n, n), float('nan'), device='cuda')
    for g0 in range(0, n, 128):
        g1 = min(n, g0 + 128)
        s, i = eng.search(emb, emb[g0:g1].contiguous(), g1 - g0, index_base=g0)
        S.scatter_(1, i, s)
    assert not torch.isnan(S).any()
    return S


def from_scratch(eng, emb, thr, m):
    """The clustering of emb by the extension from nothing: (rep, kind, degree, best), the state included."""
    out = eng.cluster_density_extend(emb, thr, m, None, None, None, 0)
    assert [t.dtype for t in out] == [torch.int64, torch.uint8, torch.int32, torch.int64]
    assert all(t.shape == (emb.size(0),) for t in out)
    return out


def full(eng, N, m):
    """(cluster_density over all rows of bridged(N), the state from scratch), computed once and left unchanged."""
    if (N, m) not in _FULL:
        emb = bridged(N)[0]
        _FULL[(N, m)] = (eng.cluster_density(emb, THR, m, return_degree=True), from_scratch(eng, emb, THR, m))
    return _FULL[(N, m)]


def extend(eng, emb, thr, m, n_old, **kw):
    """The old rows clustered from scratch (their labels held to cluster_density), then the extension to all rows
    -> (before, after), each (rep, kind, degree, best)."""
    head = emb[:n_old].contiguous()
    before = from_scratch(eng, head, thr, m)
    rep0, kind0 = eng.cluster_density(head, thr, m)
    assert torch.equal(before[0], rep0) and torch.equal(before[1], kind0)
    after = eng.cluster_density_extend(emb, thr, m, before[0], before[2], before[3], n_old, **kw)
    return before, after


def promoted(before, after, m):
    n_old = before[2].numel()
    return int(((before[2] < m - 1) & (after[2][:n_old] >= m - 1)).sum())


def assert_same(after, want, state, what):
    for name, g, w in zip(('rep', 'kind', 'degree'), after, want):
        assert torch.equal(g, w), (name, what, torch.nonzero(g != w).reshape(-1)[:8].tolist())
    assert torch.equal(after[3], state[3]), ('best', what, torch.nonzero(after[3] != state[3]).reshape(-1)[:8].tolist())


@pytest.mark.parametrize('N,n_old', SPLITS)
def test_splits_equal_the_full_call(eng, N, n_old):
    emb, S = bridged(N)
    if S is not None:
        assert cluster_ref.margin(S, THR) > MARGIN
    for m in MIN_ROWS:
        want, state = full(eng, N, m)
        assert_same(state, want, state, (N, m, 'scratch'))
        before, after = extend(eng, emb, THR, m, n_old)
        assert_same(after, want, state, (N, n_old, m))
        if S is not None:                                       # the float64 oracle is a reference too, and counts
            o_before, o_after = xref.in_batches(S, THR, m, [n_old, N])
            for g, w in zip(after[:3], o_after[:3]):
                assert np.array_equal(g.cpu().numpy(), w), (N, n_old, m)
            assert promoted(before, after, m) == o_after[4]
            if (N, n_old, m) in COUNTS:
                count, moved = COUNTS[(N, n_old, m)]
                tr = xref.transitions(o_before[1], o_after[1])
                assert o_after[4] == count > 0 and all(tr.get(k) == v for k, v in moved.items()), (o_after[4], tr)
            if n_old == 1:
                assert o_after[4] == int(o_after[1][0] == 2)
    if (N, n_old) == (168, 1):                                  # the single old row is promoted (at min_rows 3 .. 5: where it is core)
        assert any(xref.in_batches(S, THR, m, [1, N])[1][4] == 1 for m in MIN_ROWS)


def test_no_margin_agrees_with_the_full_call_and_the_search_scores(eng, synth_rows):
    emb = synth_rows
    S = search_matrix(eng, emb)
    Sn = S.cpu().numpy()
    ranked = torch.sort(S[torch.triu(torch.ones_like(S, dtype=torch.bool), 1)]).values
    # each threshold IS one of the scores, so the strict > is exercised on equal bits
    picks = [ranked[int(q * (ranked.numel() - 1))].item() for q in (0.5, 0.9, 0.97, 0.99, 0.997, 0.9995)]
    seen, kinds, most = set(), set(), 0
    for thr in picks:
        for m in (3, 6, 12):
            want = eng.cluster_density(emb, thr, m, return_degree=True)
            state = from_scratch(eng, emb, thr, m)
            oracle = dref.density_oracle(Sn, np.float32(thr), m)
            for g, w in zip(want, oracle):
                assert np.array_equal(g.cpu().numpy(), w), (thr, m)
            for n_old in (32, 64, 96, 127):
                before, after = extend(eng, emb, thr, m, n_old)
                assert_same(after, want, state, (thr, m, n_old))
                most = max(most, promoted(before, after, m))
            seen.add(len(np.unique(oracle[0])))
            kinds |= set(oracle[1].tolist())
    assert len(seen) > 1 and kinds == {0, 1, 2}                 # the cases do not all give one blob
    assert most > 0                                             # and promoted rows occur


def run_constructed(eng, which, n_old):
    rows, thr, m, _, at = xref.constructed(which)
    d = dev(rows)
    Sn = search_matrix(eng, d).cpu().numpy()
    o_before, o_after = xref.in_batches(Sn, np.float32(thr), m, [n_old, 128])
    whole = dref.density_oracle(Sn, np.float32(thr), m)
    assert all(np.array_equal(g, w) for g, w in zip(o_after[:3], whole))
    before, after = extend(eng, d, thr, m, n_old)
    assert_same(after, eng.cluster_density(d, thr, m, return_degree=True), from_scratch(eng, d, thr, m), (which, n_old))
    for g, w in zip(after[:3], whole):
        assert np.array_equal(g.cpu().numpy(), w), (which, n_old)
    assert np.array_equal(after[3].cpu().numpy(), xref.keys(o_after[3])), (which, n_old)
    assert np.array_equal(before[3].cpu().numpy(), xref.keys(o_before[3])), (which, n_old)
    return Sn, at, o_before, o_after, [t.cpu().numpy() for t in before], [t.cpu().numpy() for t in after]


def named_row(key):
    """the core row a key names"""
    return int(0xFFFFFFFF - (int(key) & 0xFFFFFFFF))


def test_constructed_switch_through_the_promoted_pass(eng):
    Sn, at, o_before, o_after, before, after = run_constructed(eng, 'switch', 64)
    A, B, x = at['A'], at['B'], at['x']
    assert x == 0 and Sn[x, B[0]] > Sn[x, A[0]] > 0.1
    # from the oracle first ...
    assert o_before[1][x] == 1 and (o_before[0][A] == 0).all() and o_before[3][1][x] == A[0]
    assert o_after[4] == 2 and o_after[1][B[0]] == 2 and o_before[1][B[0]] == 0
    assert o_after[3][1][x] == B[0] and (o_after[0][B] == 0).all() and (o_after[0][A] == A[0]).all()
    # ... then on the device: x is a border row of A, then of B; A's representative rises from 0 to its own smallest row
    assert before[1][x] == 1 and (before[0][A] == 0).all() and named_row(before[3][x]) == A[0]
    assert after[1][x] == 1 and named_row(after[3][x]) == B[0] and (after[0][B] == 0).all() and (after[0][A] == A[0]).all()
    gone, redo = fc.density_changes(torch.from_numpy(before[0]), torch.from_numpy(after[0]))
    assert gone.tolist() == [B[0], B[1]] and set(redo.tolist()) >= {0, A[0]}


@pytest.mark.parametrize('which', ['tie_promoted', 'tie_new'])
def test_constructed_tie_across_passes(eng, which):
    Sn, at, o_before, o_after, before, after = run_constructed(eng, which, 64)
    A, B, x = at['A'], at['B'], at['x']
    assert Sn[min(x, A[0]), max(x, A[0])] == Sn[min(x, B[0]), max(x, B[0])] > 0.1      # bitwise equal scores decide nothing
    assert o_after[4] == (2 if which == 'tie_promoted' else 0)
    assert (B[0] < A[0]) == (which == 'tie_promoted') and (B[0] >= 64) == (which == 'tie_new')
    winner = B if which == 'tie_promoted' else A
    assert named_row(before[3][x]) == A[0] and named_row(after[3][x]) == winner[0] == min(A[0], B[0])
    assert after[1][x] == 1 and after[0][x] == after[0][winner[0]] and after[0][A[0]] != after[0][B[0]]


def test_constructed_noise_pair_at_every_split(eng):
    rows, thr, m, splits, at = xref.constructed('noise_pair')
    for n_old in splits:
        Sn, at, _, _, _, after = run_constructed(eng, 'noise_pair', n_old)
        x, y2 = at['x'], at['y2']
        assert Sn[x, y2] > thr and after[2][x] == 1 and after[2][y2] == 1
        assert after[1][x] == 0 and after[1][y2] == 0 and after[0][x] == x and after[0][y2] == y2
        assert after[3][x] == 0 and after[3][y2] == 0


def test_scores_are_symmetric(eng, synth_rows):
    """The promoted pass scores a pair (y, p), y > p, as probe y against row p: the transpose of what the batch call scores."""
    g = torch.Generator(device='cuda')
    g.manual_seed(9)
    for emb in (synth_rows, torch.randn((257, 512), device='cuda', generator=g) * 3.0):
        S = search_matrix(eng, emb)
        assert torch.equal(S, S.t())


def test_three_batches(eng):
    emb = bridged(168)[0]
    for m in (3, 4):
        store = fc.IncrementalDensity(eng, THR, m)
        states = []
        for lo, hi in ((0, 50), (50, 100), (100, 168)):
            assert store.add(emb[lo:hi]) == lo and len(store) == hi
            want = fc.density(eng, emb[:hi].contiguous(), THR, m)
            c = store.clusters
            for name in ('rep', 'cluster_id', 'sizes', 'kind', 'has_core'):
                assert torch.equal(getattr(c, name), getattr(want, name)), (name, hi, m)
            assert c.n_clusters == want.n_clusters
            assert torch.equal(store.degree, eng.cluster_density(emb[:hi].contiguous(), THR, m, return_degree=True)[2])
            assert torch.equal(store.templates(), fc.templates(eng, emb[:hi].contiguous(), want)[want.has_core])
            states.append(store.rep.clone())
        for before, after in zip(states, states[1:]):
            gone, redo = fc.density_changes(before, after)
            b, a = before.tolist(), after.tolist()
            members = lambda lab, r, n: frozenset(i for i in range(n) if lab[i] == r)
            was = {members(b, r, len(b)) for r in set(b)}
            assert gone.tolist() == sorted(r for r in set(b) if a[r] != r)
            assert redo.tolist() == sorted(r for r in set(a) if members(a, r, len(b)) not in was or members(a, r, len(a)) != members(a, r, len(b)))
            assert len(redo) > 0
    # the functional form; a state made with another min_rows or threshold is refused
    c1, s1 = fc.density_extend(eng, emb[:100].contiguous(), THR, 4)
    c2, s2 = fc.density_extend(eng, emb, THR, 4, earlier=s1)
    want = fc.density(eng, emb, THR, 4)
    assert torch.equal(c2.rep, want.rep) and torch.equal(c2.kind, want.kind) and torch.equal(c2.has_core, want.has_core)
    assert s1.rep.numel() == 100 and s2.min_rows == 4 and s2.threshold == THR
    c3, s3 = fc.density_extend(eng, emb, THR, 4, earlier=s2)                # nothing new: the same labels, s2 untouched
    assert torch.equal(c3.rep, c2.rep) and torch.equal(s3.best, s2.best) and s3.rep.data_ptr() != s2.rep.data_ptr()
    with pytest.raises(RuntimeError):
        fc.density_extend(eng, emb, THR, 5, earlier=s1)
    with pytest.raises(RuntimeError):
        fc.density_extend(eng, emb, 0.6, 4, earlier=s1)
    # enrolment at min_rows 4, where the bridged identities stay apart (test_gpu_cluster_density.py): the templates of the
    # clusters with a core find their own core rows
    assert store.min_rows == 4
    gal = Gallery(eng)
    gal.add(store.templates())
    c = store.clusters
    core = torch.nonzero(c.kind == 2).reshape(-1)
    row_of = torch.cumsum(c.has_core.to(torch.int64), 0) - 1
    assert torch.equal(gal.search(emb[core].contiguous(), 1)[1][:, 0], row_of[c.cluster_id[core]])


def test_min_rows_1_and_2_equal_single_link(eng, synth_rows):
    S = search_matrix(eng, synth_rows)
    ranked = torch.sort(S[torch.triu(torch.ones_like(S, dtype=torch.bool), 1)]).values
    sets = [(bridged(168)[0], THR, (0, 1, 84, 128, 167, 168)), (bridged(1000)[0], THR, (128, 500, 999)),
            (synth_rows, ranked[int(0.97 * (ranked.numel() - 1))].item(), (32, 64, 127))]
    for emb, thr, splits in sets:
        want = eng.cluster(emb, thr)
        for n_old in splits:
            head = emb[:n_old].contiguous()
            prior = torch.cat((eng.cluster(head, thr), torch.arange(n_old, emb.size(0), device='cuda')))
            assert torch.equal(eng.cluster_extend(emb, thr, prior, n_old), want)
            for m in (1, 2):
                before, after = extend(eng, emb, thr, m, n_old)
                assert torch.equal(after[0], want), (n_old, m)
                assert torch.equal(after[1], torch.where(after[2] >= m - 1, 2, 0).to(torch.uint8)) and not bool(after[3].any())
    assert 1 < len(torch.unique(want)) < synth_rows.size(0)


def test_repeatable(eng):
    emb = bridged(1000)[0]
    first = extend(eng, emb, THR, 4, 500)[1]
    again = extend(eng, emb, THR, 4, 500)[1]
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    # in place when the state tensors hold N entries; norms handed in or computed in the call
    before = from_scratch(eng, emb[:500].contiguous(), THR, 4)
    rep, degree, best = [torch.cat((t, torch.full((500,), 7, device='cuda', dtype=t.dtype))) for t in (before[0], before[2], before[3])]
    out = eng.cluster_density_extend(emb, THR, 4, rep, degree, best, 500, norms=eng.row_norms(emb))
    assert out[0].data_ptr() == rep.data_ptr() and out[2].data_ptr() == degree.data_ptr() and out[3].data_ptr() == best.data_ptr()
    assert all(torch.equal(a, b) for a, b in zip(first, out))


def test_wrong_but_in_range_state_returns_consistent_labels(eng):
    emb = bridged(1000)[0]
    n_old, N = 500, 1000
    before = from_scratch(eng, emb[:n_old].contiguous(), THR, 4)
    g = torch.Generator(device='cuda')
    g.manual_seed(17)
    row = torch.arange(n_old, device='cuda')
    rep = (torch.rand((n_old,), device='cuda', generator=g) * (row + 1)).to(torch.int64).clamp_(max=row)     # anything in [0, i]
    degree = before[2] + torch.randint(0, 6, (n_old,), device='cuda', generator=g, dtype=torch.int32)         # inflated
    noncore = torch.nonzero(before[1] != 2).reshape(-1)
    names = noncore[torch.randint(0, noncore.numel(), (n_old,), device='cuda', generator=g)]                  # keys naming non-core old rows
    half = int(xref.keys((np.array([0.5], dtype=np.float32), np.array([0])))[0]) & ~0xFFFFFFFF              # the score word of 0.5
    best = torch.full((n_old,), half, device='cuda', dtype=torch.int64) | (0xFFFFFFFF - names)
    native.check_density_state(rep, degree, best)                             # in range: validate would not object
    out = eng.cluster_density_extend(emb, THR, 4, rep, degree, best, n_old, validate=False)
    torch.cuda.synchronize()
    r = out[0]
    assert bool(((r >= 0) & (r < N)).all()) and torch.equal(r[r], r)
    assert bool((out[1] <= 2).all())


def test_binding_errors(eng):
    emb = bridged(168)[0]
    rep, kind, degree, best = from_scratch(eng, emb[:100].contiguous(), THR, 4)
    ok = lambda **kw: eng.cluster_density_extend(*[kw.get(k, v) for k, v in (('emb', emb), ('thr', THR), ('m', 4), ('rep', rep),
                                                                               ('degree', degree), ('best', best), ('n_old', 100))])
    assert torch.equal(ok()[0], eng.cluster_density(emb, THR, 4)[0])
    for bad in (dict(emb=emb.cpu()), dict(emb=emb[:, :256].contiguous()), dict(rep=rep.cpu()), dict(rep=rep.to(torch.int32)),
                dict(degree=degree.to(torch.int64)), dict(best=best.to(torch.float32)), dict(rep=rep[:99]), dict(best=best[:50]),
                dict(degree=degree.reshape(10, 10)), dict(n_old=-1), dict(n_old=169), dict(m=0), dict(m=2.5), dict(rep=None),
                dict(thr=float('nan'))):
        with pytest.raises((RuntimeError, TypeError)):
            ok(**bad)
    with pytest.raises(RuntimeError):                                         # validate: a state out of range
        ok(rep=torch.full_like(rep, 101))
    with pytest.raises(RuntimeError):
        eng.cluster_density_extend(emb, THR, 4, rep, degree, best, 100, norms=eng.row_norms(emb)[:50])
    none = eng.cluster_density_extend(emb[:0], THR, 4, None, None, None, 0)
    assert all(t.numel() == 0 for t in none)
    one = eng.cluster_density_extend(emb[:1].contiguous(), THR, 1, None, None, None, 0)
    assert [t.tolist() for t in one] == [[0], [2], [0], [0]]

    # the C entry: its own argument checks
    N = 168
    full_rep, full_deg, full_best = [torch.cat((t, torch.zeros((68,), device='cuda', dtype=t.dtype))) for t in (rep, degree, best)]
    kind = torch.empty((N,), device='cuda', dtype=torch.uint8)
    P, null = native._ptr, C.c_void_p(0)
    names = ['emb', 'norms', 'N_old', 'N', 'dim', 'thr', 'min_rows', 'rep', 'kind', 'degree', 'best', 'st']
    good = (P(emb), null, 100, N, 512, THR, 4, P(full_rep), P(kind), P(full_deg), P(full_best), eng._stream())

    def call(**kw):
        a = list(good)
        for key, v in kw.items():
            a[names.index(key)] = v
        return eng.lib.ffr_cluster_density_extend(eng._h, *a)

    assert call() == 0 and torch.equal(full_rep, eng.cluster_density(emb, THR, 4)[0])
    assert call(dim=256) == -6
    for bad in (dict(N=-1), dict(N=1 << 31), dict(N_old=-1), dict(N_old=N + 1), dict(thr=float('nan')), dict(min_rows=0),
                dict(emb=null), dict(rep=null), dict(kind=null), dict(degree=null), dict(best=null),
                dict(emb=C.c_void_p(emb.data_ptr() + 4)), dict(rep=C.c_void_p(full_rep.data_ptr() + 4)),
                dict(best=C.c_void_p(full_best.data_ptr() + 4)), dict(degree=C.c_void_p(full_deg.data_ptr() + 2))):
        assert call(**bad) == -1, bad
        assert 'ffr_cluster_density_extend' in (eng.lib.ffr_last_error(eng._h) or b'').decode(), bad
    assert call(N=0, N_old=0, emb=null, rep=null, kind=null, degree=null, best=null) == 0
