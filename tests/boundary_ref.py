"""Test infrastructure of the boundary-kernel tests (tests/test_gpu_boundary_ops.py, tests/test_host_boundary_ops.py): the shapes
and the inputs of the LFW fold protocol cases, built the same way on the host and for the device.

A fold case is (n, n_folds, labels, nonfinite).  Scores are fp32: seeded uniform in [-1.2, 1.2] (part of them outside the
threshold grid [-1, 0.995]), a tenth of the rows copied from other rows (duplicates), every seventh row set to
float32(THRESHOLDS[j]) for a random j -- the protocol compares (double)score > thr, so such a score lies on either side of its own
threshold, whichever way the rounding to fp32 went -- and, with `nonfinite`, rows 1, 2, 3 = NaN, +inf, -inf.
Labels: 'random' 0 / 1, 'zeros', 'ones'."""
import numpy as np

from ffrnet_amd import lfw

# n == n_folds (one row per fold), n % n_folds != 0 below and above the 256 threads of a block, 32 folds (the most the library
# takes), the production shape plus one row, one fold (an empty train set: every threshold ties)
FOLD_SHAPES = ((10, 10), (11, 10), (13, 5), (32, 32), (257, 32), (255, 7), (601, 10), (6001, 10), (600, 1))
FOLD_CASES = tuple((n, nf, 'random', False) for n, nf in FOLD_SHAPES) + \
    ((257, 32, 'zeros', False), (255, 7, 'ones', False), (255, 7, 'random', True), (13, 5, 'random', True))


def case_id(case):
    n, nf, labels, nonfinite = case
    return '%dx%d-%s%s' % (n, nf, labels, '-nonfinite' if nonfinite else '')


def fold_inputs(case):
    """-> (scores fp32 [n], labels int64 [n])"""
    n, nf, labels, nonfinite = case
    g = np.random.Generator(np.random.Philox(key=(n << 16) | (nf << 4) | (2 if nonfinite else 0) | (labels != 'random')))
    s = g.uniform(-1.2, 1.2, n).astype(np.float32)
    k = max(1, n // 10)
    src, dst = g.integers(0, n, k), g.integers(0, n, k)
    s[dst] = s[src]
    j = g.integers(0, len(lfw.THRESHOLDS), n)
    s[::7] = lfw.THRESHOLDS[j[::7]].astype(np.float32)
    if nonfinite:
        s[1:4] = (np.nan, np.inf, -np.inf)
    y = {'random': g.integers(0, 2, n), 'zeros': np.zeros(n, np.int64), 'ones': np.ones(n, np.int64)}[labels]
    return s, y.astype(np.int64)


def predicts(scores, labels):
    """the [n,3] float64 array (score, label, idx) of lfw.calculate_distance, from the fp32-rounded scores"""
    return np.array([scores.astype(np.float64), labels.astype(np.float64), np.arange(len(scores), dtype=np.float64)]).T


def host_protocol(scores, labels, n_folds):
    """lfw.get_accuracy_from_predicts; with one fold the train set is empty and its accuracies are 0 / 0"""
    with np.errstate(invalid='ignore', divide='ignore'):
        return lfw.get_accuracy_from_predicts(predicts(scores, labels), n_folds)
