"""The small kernels at the edge of the C ABI, at other shapes than production's: ffr_cosine_scores (k_cosine) against float64,
ffr_lfw_fold_accuracy (k_fold_counts, k_fold_select) at ragged folds against the host protocol, and the calibration distance
(k_absdiff_max, k_absdiff_fold behind ffr_calibrate) on a forward that is not finite.
Needs a real MI355X: `python -m pytest tests -m gpu`.

Cosine scores.  Reference: sum(a * b) / (|a| * |b| + 1e-8) in torch float64 on the device.  n in {1, 3, 4, 5, 257} (4 rows per
block: a partly empty block, several blocks) x dim in {1, 3, 63, 64, 65, 512, 513, 2048} (lanes without an element, a ragged
last pass).  Bound, absolute (a score is at most 1 in magnitude): each of the three sums is a chain of ceil(dim / 64) adds per
lane and 6 shuffle adds, then two square roots, a product, an add and a divide, and sum |a_i b_i| <= |a| |b|, so
|got - ref| <= (ceil(dim / 64) + 16) * 2^-24.  The bound is not derived from what the kernel gives.
Measured worst |got - ref| per dim on one MI355X, over every n and every kind of row, in units of 2^-24 (bound):
    dim 1: 1.19 (17)   3: 3.35 (17)   63: 2.00 (17)   64: 2.00 (17)   65: 2.00 (18)   512: 2.00 (24)   513: 2.00 (25)   2048: 2.00 (48)
The worst of all is 3.35 * 2^-24 = 1.99e-7, at dim = 3.
The fold protocol's cases and their inputs are tests/boundary_ref.py's; tests/test_host_boundary_ops.py pins the host protocol
they are held to against the oracle's restatement of the reference."""
import ctypes as C

import pytest
import torch

import ffrnet_amd
from ffrnet_amd import native, synth

import boundary_ref as B

pytestmark = pytest.mark.gpu
FFR_ERR_ARG = -1
COSINE_N = (1, 3, 4, 5, 257)
COSINE_DIM = (1, 3, 63, 64, 65, 512, 513, 2048)
WORST = {}               # dim -> largest |got - ref|, printed when the module is done


@pytest.fixture(scope='module')
def eng():
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    e = ffrnet_amd.Engine(0)             # no weights: the scoring entries need none
    yield e
    e.close()
    for dim, w in sorted(WORST.items()):
        print('boundary ops worst  cosine dim %4d  |got - ref| %.3e = %.2f * 2^-24 (bound %d)' % (dim, w, w * 2.0 ** 24, cosine_units(dim)))


def _rc(eng, fn, *args):
    with torch.cuda.device(eng.device):
        return getattr(eng.lib, fn)(eng._h, *args)


def cosine_units(dim):
    return (dim + 63) // 64 + 16


def cosine_ref(a, b):
    a, b = a.double(), b.double()
    return (a * b).sum(1) / (a.square().sum(1).sqrt() * b.square().sum(1).sqrt() + 1e-8)


def cosine_rows(n, dim):
    """-> [(kind, a, b, rows whose score must be exactly 0.0)]"""
    g = torch.Generator().manual_seed(1000 * n + dim)
    a, b = torch.randn(n, dim, generator=g), torch.randn(n, dim, generator=g)
    r = n // 2
    za, zb = a.clone(), b.clone()
    za[r] = 0
    zb[r] = 0
    lo, hi = 2.0 ** -40, 2.0 ** 40
    return [('randn', a, b, []), ('zero row in a', za, b, [r]), ('zero row in b', a, zb, [r]), ('zero rows in both', za, zb, [r]),
            ('b = a', a, a.clone(), []), ('b = -a', a, -a, []),
            ('both * 2^-40', a * lo, b * lo, []), ('both * 2^40', a * hi, b * hi, []), ('a * 2^40, b * 2^-40', a * hi, b * lo, []),
            ('b = a * 2^-40', a, a * lo, []), ('b = -a * 2^40', a, -a * hi, [])]


@pytest.mark.parametrize('dim', COSINE_DIM)
def test_cosine_scores_vs_float64(eng, dim):
    tol = cosine_units(dim) * 2.0 ** -24
    bad = []
    for n in COSINE_N:
        for kind, a, b, zero in cosine_rows(n, dim):
            a, b = a.cuda(), b.cuda()
            assert torch.isfinite(a.square().sum(1)).all() and torch.isfinite(b.square().sum(1)).all()     # squares stay inside fp32
            buf = torch.full((n + 64,), float('nan'), device='cuda')        # the scores, then 64 floats no row may touch
            assert _rc(eng, 'ffr_cosine_scores', native._ptr(a), native._ptr(b), n, dim, native._ptr(buf), eng._stream()) == 0
            ref = cosine_ref(a, b)
            torch.cuda.synchronize()
            got = buf[:n]
            assert torch.isfinite(got).all() and torch.isnan(buf[n:]).all(), (n, dim, kind)
            if kind == 'randn':
                assert torch.equal(eng.cosine_scores(a, b), got)
            e = (got.double() - ref).abs().max().item()
            WORST[dim] = max(WORST.get(dim, 0.0), e)
            for r in zero:
                if got[r].item() != 0.0:
                    bad.append((n, kind, 'row %d is %r, not 0.0' % (r, got[r].item())))
            if not e <= tol:
                bad.append((n, kind, e))
    print('boundary ops  cosine dim %4d  worst |got - ref| %.3e = %.2f * 2^-24, bound %d * 2^-24'
          % (dim, WORST[dim], WORST[dim] * 2.0 ** 24, cosine_units(dim)))
    assert not bad, bad


def test_cosine_scores_refusals(eng):
    a, b = torch.randn(5, 64, device='cuda'), torch.randn(5, 64, device='cuda')
    s = torch.empty(5, device='cuda')
    for x, y in ((a, b[:, :63]), (a, b[:4]), (a[0], b[0]), (a.view(5, 8, 8), b.view(5, 8, 8)), (a, b.double()), (a.cpu(), b)):
        with pytest.raises(RuntimeError):
            eng.cosine_scores(x, y)
    P, st, null = native._ptr, eng._stream(), C.c_void_p(0)
    assert _rc(eng, 'ffr_cosine_scores', P(a), P(b), 5, 64, P(s), st) == 0
    assert _rc(eng, 'ffr_cosine_scores', P(a), P(b), 5, 0, P(s), st) == FFR_ERR_ARG
    assert _rc(eng, 'ffr_cosine_scores', P(a), P(b), 5, -1, P(s), st) == FFR_ERR_ARG
    assert _rc(eng, 'ffr_cosine_scores', P(a), P(b), 0, 64, P(s), st) == FFR_ERR_ARG
    for args in ((null, P(b), 5, 64, P(s)), (P(a), null, 5, 64, P(s)), (P(a), P(b), 5, 64, null)):
        assert _rc(eng, 'ffr_cosine_scores', *args, st) == FFR_ERR_ARG
    torch.cuda.synchronize()
    assert torch.allclose(s.double(), cosine_ref(a, b), rtol=0, atol=17 * 2.0 ** -24)


@pytest.mark.parametrize('case', B.FOLD_CASES, ids=[B.case_id(c) for c in B.FOLD_CASES])
def test_fold_protocol_at_ragged_folds(eng, case):
    """thresholds and accuracies equal as Python floats to lfw.get_accuracy_from_predicts on the fp32-rounded scores as float64"""
    n, nf = case[:2]
    s, y = B.fold_inputs(case)
    mean_h, res_h = B.host_protocol(s, y, nf)
    mean_d, res_d = eng.lfw_fold_accuracy(torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda(), nf)
    assert len(res_d) == nf
    assert [r[0] for r in res_d] == [float(r[0]) for r in res_h]
    assert [r[1] for r in res_d] == [float(r[1]) for r in res_h]
    assert abs(mean_d - mean_h) < 1e-15


def test_fold_protocol_refusals(eng):
    s = torch.linspace(-1, 1, 40, device='cuda')
    y = torch.zeros(40, dtype=torch.int32, device='cuda')
    thr, acc = torch.empty(32, dtype=torch.float64, device='cuda'), torch.empty(32, dtype=torch.float64, device='cuda')
    P, st, null = native._ptr, eng._stream(), C.c_void_p(0)
    assert _rc(eng, 'ffr_lfw_fold_accuracy', P(s), P(y), 40, 32, P(thr), P(acc), st) == 0
    for n, nf in ((40, 0), (40, 33), (40, -1), (9, 10), (31, 32), (0, 1)):
        assert _rc(eng, 'ffr_lfw_fold_accuracy', P(s), P(y), n, nf, P(thr), P(acc), st) == FFR_ERR_ARG, (n, nf)
    for args in ((null, P(y), 40, 10, P(thr), P(acc)), (P(s), null, 40, 10, P(thr), P(acc)), (P(s), P(y), 40, 10, null, P(acc)),
                 (P(s), P(y), 40, 10, P(thr), null)):
        assert _rc(eng, 'ffr_lfw_fold_accuracy', *args, st) == FFR_ERR_ARG
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        eng.lfw_fold_accuracy(s, y, 33)
    with pytest.raises(RuntimeError):
        eng.lfw_fold_accuracy(s[:9], y[:9], 10)


def test_a_non_finite_forward_never_calibrates_as_close(state_dicts):
    """One NaN pixel in image 0 of 2: every output of that image is NaN in every forward of the calibration (the SE squeeze of the
    first bottleneck spreads it over the image), image 1 stays finite.  k_absdiff_max counts a NaN difference as +inf and its
    abs-max of the anchor skips the NaN, so every trial is at distance +inf: the call returns, reports +inf for f and featmap --
    not None, which is what a NaN would turn into -- and leaves every layer it ran on direct arithmetic.  A second call on clean
    images calibrates as test_gpu_arith_plan.py::test_no_needless_pinning_on_a_benign_family expects: all Winograd, every output
    within 5e-5, bit-equal to a fresh handle.

    On the host side ffr_calibrate divides the difference by the anchor's abs-max.  An anchor that holds an infinity gives
    inf / inf = NaN, which std::max would drop; the library counts it as +inf.  No test covers that line: no input was found that
    reaches it.  An image scaled by 2^k, k = 90 .. 127, leaves its all-direct featmap and f either finite in every element or NaN
    in every element (measured on one MI355X): an overflow inside the trunk meets the other sign in the next convolution, and
    the next SE squeeze spreads the NaN over the image before an infinity can reach an output."""
    sd_e, _ = state_dicts
    eng, fresh = ffrnet_amd.Engine(0), ffrnet_amd.Engine(0)
    try:
        eng.load_encoder(sd_e)
        fresh.load_encoder(sd_e)
        clean = synth.synth_images(2, 112, 112, seed=7300).cuda()
        x = clean.clone()
        x[0, 1, 50, 60] = float('nan')
        rep = eng.calibrate(x=x, tol=1e-4)
        assert rep['n'] == 2 and len(rep['layers']) == 44
        assert rep['achieved']['f'] == float('inf') and rep['achieved']['featmap'] == float('inf'), rep['achieved']
        assert rep['achieved']['f_new'] is None and rep['achieved']['feat_new'] is None          # no RecNet in this handle
        assert all(l['arith'] == 'direct' for l in rep['layers']), [l['name'] for l in rep['layers'] if l['arith'] != 'direct']
        assert all(l['sensitivity'] == float('inf') for l in rep['layers']), rep['layers']
        fm, f = eng.encoder_forward(x)
        torch.cuda.synchronize()
        assert torch.isnan(fm[0]).all() and torch.isnan(f[0]).all() and torch.isfinite(fm[1]).all() and torch.isfinite(f[1]).all()
        # the handle is not poisoned
        rep = eng.calibrate(x=clean, tol=1e-4)
        assert all(l['arith'] == 'winograd' for l in rep['layers']), [l['name'] for l in rep['layers'] if l['arith'] == 'direct']
        assert all(rep['achieved'][k] is not None and rep['achieved'][k] <= 5e-5 for k in ('f', 'featmap')), rep['achieved']
        assert all(l['sensitivity'] is not None and l['sensitivity'] < float('inf') for l in rep['layers'])
        got, want = eng.encoder_forward(clean), fresh.encoder_forward(clean)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    finally:
        eng.close()
        fresh.close()
