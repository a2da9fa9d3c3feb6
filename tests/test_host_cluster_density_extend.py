"""CPU checks of the extension of a density-gated clustering (include/ffrnet.h: ffr_cluster_density_extend): the pass-by-pass
oracle of tests/cluster_density_extend_ref.py against the batch oracle at every split the GPU test uses, the counts that
make those splits worth running, the constructed cases, the state check of the binding, density_changes, and the C symbol."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cluster_density_extend_ref as xref
import cluster_density_ref as dref
import cluster_ref
from ffrnet_amd import cluster as fc
from ffrnet_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.5
MIN_ROWS = (3, 4, 5)
# (N, n_old) of the GPU test
SPLITS = ([(20, 0), (20, 1), (33, 32), (129, 128), (129, 96)] + [(168, k) for k in (0, 1, 42, 84, 126, 128, 167, 168)] +
          [(257, 128)] + [(1000, k) for k in (31, 32, 33, 127, 128, 129, 500, 999)] + [(4129, k) for k in (1000, 4096, 4128)])
# (N, n_old, min_rows) -> (promoted rows, {(kind before, kind after): rows}) from the committed recipe and its seed
COUNTS = {(168, 84, 4): (37, {(1, 2): 2}), (129, 96, 3): (8, {(0, 1): 1, (1, 2): 1}), (168, 167, 5): (3, {(1, 2): 3}),
          (257, 128, 4): (62, {(0, 1): 2}), (1000, 500, 5): (240, {(1, 2): 3})}
_S = {}


def scores(N):
    if N not in _S:
        _S[N] = cluster_ref.cosine64(dref.planted_bridged(N)[0])
        _S[N].setflags(write=False)
    return _S[N]


def assert_is_batch(got, S, m, what):
    want = dref.density_oracle(S, THR, m)
    for name, g, w in zip(('rep', 'kind', 'degree'), got[:3], want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, what)
    score, row = got[3]
    border = got[1] == 1
    assert (row[border] >= 0).all() and (row[~border] == -1).all() and (got[1][row[border]] == 2).all(), what


@pytest.mark.parametrize('N', sorted({n for n, _ in SPLITS}))
def test_oracle_equals_the_batch_oracle_at_every_split(N):
    S = scores(N)
    for m in MIN_ROWS:
        scratch = xref.extend_from_scores(S, THR, m, 0, xref.empty_state())
        assert scratch[4] == 0
        assert_is_batch(scratch, S, m, (N, m))
        for n_old in [k for n, k in SPLITS if n == N]:
            before, after = xref.in_batches(S, THR, m, [n_old, N])
            assert_is_batch(before, S[:n_old, :n_old], m, (N, n_old, m, 'before'))
            assert_is_batch(after, S, m, (N, n_old, m))
            assert np.array_equal(xref.keys(after[3]), xref.keys(scratch[3])), (N, n_old, m)     # the state, too
            if (N, n_old, m) in COUNTS:
                promoted, moved = COUNTS[(N, n_old, m)]
                tr = xref.transitions(before[1], after[1])
                assert after[4] == promoted and all(tr.get(k) == v for k, v in moved.items()), (N, n_old, m, after[4], tr)
            if n_old == 1:                                      # the single old row is promoted iff it ends up core
                assert after[4] == int(after[1][0] == 2)
            if n_old == N:
                assert after[4] == 0


def test_single_old_row_is_promoted_somewhere():
    assert any(xref.in_batches(scores(N), THR, m, [1, N])[1][4] == 1 for N in (20, 168) for m in MIN_ROWS)


def test_three_batches_hand_the_state_over():
    S = scores(168)
    for m in (1, 2) + MIN_ROWS:
        chain = xref.in_batches(S, THR, m, [50, 100, 168])
        for cut, got in zip((50, 100, 168), chain):
            assert_is_batch(got, S[:cut, :cut], m, (cut, m))
        if m >= 3:
            assert chain[1][4] > 0 and chain[2][4] > 0          # both extensions promote rows
    # random graphs with few distinct scores: ties between offers are common
    rng = np.random.default_rng(11)
    for case in range(40):
        n = int(rng.integers(2, 30))
        R = rng.integers(0, 6, size=(n, n)).astype(np.float32) / 5
        cuts = sorted(set(rng.integers(0, n + 1, size=3).tolist()) | {n})
        for m in (1, 2, 3, 4):
            got = xref.in_batches(R, np.float32(0.4), m, cuts)[-1]
            want = dref.density_oracle(R, np.float32(0.4), m)
            assert all(np.array_equal(g, w) for g, w in zip(got[:3], want)), (case, m, cuts)


def fp32_scores(rows):
    """the exact cosine of integer rows, in the arithmetic of the device (dots and squared norms are exact)"""
    x = rows.astype(np.float32)
    n = np.sqrt((x * x).sum(1, dtype=np.float32))
    return (x @ x.T) / (n[:, None] * n[None, :] + np.float32(1e-8))


def test_constructed_cases_do_what_they_are_named_for():
    rows, thr, m, n_old, at = xref.constructed('switch')
    S = fp32_scores(rows)
    A, B, x = at['A'], at['B'], at['x']
    before, after = xref.in_batches(S, np.float32(thr), m, [n_old, 128])
    assert x == 0 and abs(S[x, A[0]] - 0.4) < 1e-6 and abs(S[x, B[0]] - 0.8) < 1e-6
    assert before[1][x] == 1 and (before[0][A] == 0).all() and before[3][1][x] == A[0]
    assert before[1][B[0]] == 0 and before[1][B[1]] == 0
    assert after[4] == 2 and (after[1][B] == 2).all()
    assert after[1][x] == 1 and after[3][1][x] == B[0] and (after[0][B] == 0).all()
    assert (after[0][A] == A[0]).all() and A[0] > 0            # a representative that ROSE
    assert all(np.array_equal(g, w) for g, w in zip(after[:3], dref.density_oracle(S, np.float32(thr), m)))

    for which, winner in (('tie_promoted', 'B'), ('tie_new', 'A')):
        rows, thr, m, n_old, at = xref.constructed(which)
        S = fp32_scores(rows)
        A, B, x = at['A'], at['B'], at['x']
        assert S[min(x, A[0]), max(x, A[0])] == S[min(x, B[0]), max(x, B[0])] > thr
        before, after = xref.in_batches(S, np.float32(thr), m, [n_old, 128])
        assert before[3][1][x] == A[0] and before[1][x] == 1
        assert after[4] == (2 if which == 'tie_promoted' else 0)
        assert (B[0] < A[0]) == (winner == 'B') and after[3][1][x] == min(A[0], B[0]) and after[0][x] == after[0][at[winner][0]]
        assert all(np.array_equal(g, w) for g, w in zip(after[:3], dref.density_oracle(S, np.float32(thr), m)))

    rows, thr, m, splits, at = xref.constructed('noise_pair')
    S = fp32_scores(rows)
    x, y2 = at['x'], at['y2']
    assert S[x, y2] > thr
    for n_old in splits:
        after = xref.in_batches(S, np.float32(thr), m, [n_old, 128])[-1]
        assert after[1][x] == 0 and after[1][y2] == 0 and after[0][x] == x and after[0][y2] == y2 and after[2][x] == 1
        assert (after[1][at['A'] + at['B']] == 2).all()


def test_keys_order_as_the_scores():
    s = np.array([-1.0, -0.5, -0.0, 0.0, 0.25, 0.8, 1.0], dtype=np.float32)
    bits = xref.ordered_bits(s)
    assert (np.diff(bits.astype(np.int64)) > 0).all()
    k = xref.keys((np.array([0.8, 0.8, 0.25, 0.0], dtype=np.float32), np.array([3, 7, 1, -1])))
    ku = k.view(np.uint64)
    assert ku[0] > ku[1] > ku[2] > ku[3] == 0                   # the score first, then the smaller row
    assert [int(0xFFFFFFFF - (int(v) & 0xFFFFFFFF)) for v in ku[:3]] == [3, 7, 1]


def good_state():
    """the state of planted_bridged(168)[:100] at min_rows 4, as the binding holds it"""
    got = xref.in_batches(scores(168), THR, 4, [100])[0]
    assert set(got[1].tolist()) == {0, 1, 2}
    return torch.from_numpy(got[0]), torch.from_numpy(got[2]), torch.from_numpy(xref.keys(got[3]))


def test_validate_accepts_a_good_state_and_refuses_each_bad_one():
    rep, degree, best = good_state()
    native.check_density_state(rep, degree, best)
    native.check_density_state(rep[:0], degree[:0], best[:0])
    border = int(torch.nonzero(best)[0])

    def broken(**kw):
        s = dict(rep=rep.clone(), degree=degree.clone(), best=best.clone())
        for name, (i, v) in kw.items():
            s[name][i] = v
        return s['rep'], s['degree'], s['best']

    for bad in (dict(rep=(5, -1)), dict(rep=(5, 6)), dict(rep=(99, 100)), dict(degree=(7, -1)),
                dict(best=(border, (1 << 62) | (0xFFFFFFFF - 100))),        # names row 100 of a state of 100 rows
                dict(best=(border, (1 << 62))),                             # low word 0: names row 2^32 - 1
                dict(best=(3, -1 << 32))):                                  # a negative int64: the top bit of the score word
        with pytest.raises(RuntimeError):
            native.check_density_state(*broken(**bad))
    native.check_density_state(*broken(best=(border, (-1 << 63) | (0xFFFFFFFF - 99))))   # row 99 is in range
    with pytest.raises(RuntimeError):
        native.check_density_state(rep, degree[:50], best)


def test_density_changes_on_hand_made_labelings():
    t = lambda *v: torch.tensor(v, dtype=torch.int64)
    # nothing moved, one new row joined cluster 1, one new row is alone
    gone, redo = fc.density_changes(t(0, 1, 0, 1), t(0, 1, 0, 1, 1, 5))
    assert gone.tolist() == [] and redo.tolist() == [1, 5]
    # absorbed: cluster 2 went into cluster 0
    gone, redo = fc.density_changes(t(0, 1, 2, 2), t(0, 1, 0, 0))
    assert gone.tolist() == [2] and redo.tolist() == [0]
    # a border row changes sides: row 0 leaves {0, 2, 3} for {1, 4}; the cluster it left is now named 2, a rep that ROSE
    before, after = t(0, 1, 0, 0, 1), t(0, 0, 2, 2, 0, 0)
    gone, redo = fc.density_changes(before, after)
    assert gone.tolist() == [1] and redo.tolist() == [0, 2]
    stale, now = fc.changes(before, after)                                   # changes() misses cluster 2
    assert stale.tolist() == [1] and now.tolist() == [0]
    # a row changes sides and no representative changes at all: both clusters must be recomputed
    gone, redo = fc.density_changes(t(0, 1, 0, 1, 4), t(0, 1, 1, 1, 4))
    assert gone.tolist() == [] and redo.tolist() == [0, 1]
    assert [x.tolist() for x in fc.changes(t(0, 1, 0, 1, 4), t(0, 1, 1, 1, 4))] == [[], []]
    # objects with a .rep are accepted; fewer labels after than before are not
    c0, c1 = fc.density_ids(t(0, 1, 1), torch.tensor([0, 2, 2], dtype=torch.uint8)), fc.dense_ids(t(0, 1, 1, 1))
    assert [x.tolist() for x in fc.density_changes(c0, c1)] == [[], [1]]
    with pytest.raises(ValueError):
        fc.density_changes(t(0, 1, 2), t(0, 1))


def test_density_state_and_names():
    import ffrnet_amd
    assert fc.DensityState._fields == ('rep', 'kind', 'degree', 'best', 'threshold', 'min_rows')
    assert ffrnet_amd.DensityState is fc.DensityState and ffrnet_amd.IncrementalDensity is fc.IncrementalDensity
    assert callable(fc.density_extend) and callable(fc.density_changes) and hasattr(native.Engine, 'cluster_density_extend')


def test_symbol_arguments_are_spelled_out():
    rows = {name: (res, args) for name, res, args in native.SYMBOLS}
    res, args = rows['ffr_cluster_density_extend']
    L, I, F, P = ctypes.c_longlong, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    assert res is I and list(args) == [P, P, P, L, L, I, F, I, P, P, P, P, P] and len(args) == 13
    hdr = open(os.path.join(ROOT, 'include', 'ffrnet.h')).read()
    proto = re.search(r'^int ffr_cluster_density_extend\(([^;]*)\);', hdr, re.M).group(1)
    assert [a.split()[-1].lstrip('*') for a in proto.split(',')] == [
        'h', 'emb', 'norms', 'N_old', 'N', 'dim', 'threshold', 'min_rows', 'rep', 'kind', 'degree', 'best', 'stream']
    lib = ctypes.CDLL(native.lib_path())                                     # loads without a GPU
    assert lib.ffr_cluster_density_extend is not None
