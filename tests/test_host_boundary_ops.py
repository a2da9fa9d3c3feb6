"""Host side of the boundary-kernel tests (tests/test_gpu_boundary_ops.py): no device needed.

The device fold protocol is held to ffrnet_amd.lfw.get_accuracy_from_predicts.  Here that function is held to the oracle's
plain-loop restatement of the reference (oracle/ffr_oracle.py: kfold, fold_accuracy = lfw/lfw_eval.py's KFold and
get_fold_accuracy) on the very inputs of the device cases: ragged folds, one row per fold, 32 folds, scores on grid thresholds,
duplicates, NaN and infinities, constant labels.  Thresholds and accuracies are equal as Python floats.

With one fold the train set is empty and the reference divides by its length (lfw_eval.py:148): the oracle raises there as the
reference does.  lfw and the device take the LAST threshold instead (every threshold ties), which is what the loop of
find_best_threshold does on equal accuracies; that case is held to this rule and to the oracle's eval_acc on the test fold."""
import numpy as np
import pytest

import boundary_ref as B
from trunk_ref import O

from ffrnet_amd import lfw


@pytest.mark.parametrize('case', B.FOLD_CASES, ids=[B.case_id(c) for c in B.FOLD_CASES])
def test_lfw_protocol_equals_the_oracle_loops(case):
    n, nf = case[:2]
    s, y = B.fold_inputs(case)
    assert s.dtype == np.float32 and len(s) == n == len(y)
    pred = B.predicts(s, y)
    mean, res = B.host_protocol(s, y, nf)
    folds = O.kfold(n, nf)
    assert [sorted(f[1]) for f in folds] == [list(t) for _, t in lfw.KFold(n, nf)]
    assert [f[0] for f in folds] == [list(t) for t, _ in lfw.KFold(n, nf)]
    assert len(res) == nf and all(len(f[1]) >= 1 for f in folds)
    if nf == 1:
        with pytest.raises(ZeroDivisionError):
            O.fold_accuracy(folds[0], pred)
        assert res[0][0] == lfw.THRESHOLDS[-1] and float(res[0][1]) == O.eval_acc(lfw.THRESHOLDS[-1], pred)
        assert mean == float(res[0][1])
        return
    want = [O.fold_accuracy(f, pred) for f in folds]
    assert [float(r[0]) for r in res] == [float(w[0]) for w in want]
    assert [float(r[1]) for r in res] == [float(w[1]) for w in want]
    assert mean == sum(w[1] for w in want) / nf


def test_case_inputs_hold_what_they_claim():
    """every shape class and every kind of score the device cases are there for"""
    shapes = {c[:2] for c in B.FOLD_CASES}
    assert shapes == set(B.FOLD_SHAPES)
    assert any(n == nf for n, nf in shapes) and any(n % nf and n < 256 for n, nf in shapes) and any(n % nf and n > 256 for n, nf in shapes)
    assert any(nf == 32 and n % nf for n, nf in shapes) and any(nf == 1 for n, nf in shapes)
    assert {c[2] for c in B.FOLD_CASES} == {'random', 'zeros', 'ones'} and any(c[3] for c in B.FOLD_CASES)
    grid32 = set(lfw.THRESHOLDS.astype(np.float32).tolist())
    sides = set()
    for c in B.FOLD_CASES:
        s, y = B.fold_inputs(c)
        s2, y2 = B.fold_inputs(c)
        assert np.array_equal(s, s2, equal_nan=True) and np.array_equal(y, y2)          # seeded
        assert all(float(v) in grid32 for v in s[::7])
        fin = s[np.isfinite(s)]
        assert len(np.unique(fin)) < len(fin) or len(s) < 20                             # duplicates
        if len(s) > 100:
            assert (fin > 1.0).any() and (fin < -1.0).any()                              # outside the grid
        assert c[3] == bool(np.isnan(s).any()) and c[3] == bool(np.isposinf(s).any()) and c[3] == bool(np.isneginf(s).any())
        assert set(y.tolist()) <= {0, 1} and (c[2] != 'zeros' or not y.any()) and (c[2] != 'ones' or y.all())
        # a score made from a threshold lies above it or not, as the rounding to fp32 went: both happen
        for v in s[::7]:
            t = lfw.THRESHOLDS[np.argmin(np.abs(lfw.THRESHOLDS - float(v)))]
            sides.add(bool(float(v) > t))
    assert sides == {True, False}


def test_fold_partition_of_the_device_rule():
    """k_fold_counts finds the fold of row r from (r * nf) / n and repairs it against the bounds [f * n / nf, (f + 1) * n / nf);
    k_fold_select divides by the size of that range.  The rule restated here lands every row in the oracle's fold, and no fold
    is empty, for every n it can take up to 200 rows and all of the case shapes."""
    def fold_of(r, n, nf):
        f = (r * nf) // n
        while (f + 1) * n // nf <= r:
            f += 1
        while f * n // nf > r:
            f -= 1
        return f

    shapes = [(n, nf) for nf in range(1, 33) for n in range(nf, 200)] + list(B.FOLD_SHAPES)
    for n, nf in shapes:
        bounds = [(i * n // nf, (i + 1) * n // nf) for i in range(nf)]
        assert all(hi > lo for lo, hi in bounds), (n, nf)
        want = [i for i, (lo, hi) in enumerate(bounds) for _ in range(lo, hi)]
        assert [fold_of(r, n, nf) for r in range(n)] == want, (n, nf)
