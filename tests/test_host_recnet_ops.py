"""Host side of the RecNet operator tests (tests/test_gpu_recnet_ops.py): no device needed.

1. The float64 restatements of tests/recnet_ops_ref.py against the taps of oracle/ffr_oracle.py's recnet_forward run in
   float64, to 1e-12 (max-abs over abs-max), on the three weight sets and the edited featmaps the device tests use: a zeroed
   channel, a zeroed position, a channel below the norm clamp, an all-zero image.
2. ffr_plan_channel_rows_host, the choice of k_channel_path's form, swept over N = 1..1100 for 1 / 64 / 256 / 304 CUs against
   an independent restatement (fewest rounds x block time over the three forms, ties to fewer row blocks), with the
   thresholds at 256 CUs spelled out."""
import ctypes
import os
import sys

import pytest
import torch

from ffrnet_amd import native, synth

import recnet_ops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import ffr_oracle as O  # noqa: E402

TOL = 1e-12
BLOCK_US = {1: 181, 2: 140, 4: 101}       # plan.cpp, plan_channel_rows: measured time of one block of each form


@pytest.fixture(scope='module')
def sets(specs, golden_dir):
    return R.weight_sets(specs, golden_dir)


@pytest.mark.parametrize('family', R.FAMILIES)
def test_restatements_match_the_float64_oracle(sets, family):
    sd_e, sd_r = sets[family]
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with torch.no_grad():
        fm, _ = O.encoder_forward(sd_e, synth.synth_images(3, seed=611))
        x = R.edit_featmaps(fm).double()
        sd = R.cast(sd_r, torch.float64)
        taps = {}
        f_new, feat_new = O.recnet_forward(sd, x, taps)
        assert (x[1, 77] == 0).all() and (x[1, :, 3, 5] == 0).all() and (x[2] == 0).all()
        assert 0 < x[0, 301].abs().max() < 1e-15 and (x[0, 301] ** 2).sum().sqrt() < R.EPS
        for t in list(taps.values()) + [f_new, feat_new]:
            assert torch.isfinite(t).all()
        assert 0 <= taps['M_channel'].min() < 0.1 and 0.9 < taps['M_channel'].max() <= 1        # the sigmoid is used over its range
        got = dict(ss_space=R.ss_space(x), ss_channel=R.ss_channel(x), M_channel=R.m_channel(x, sd),
                   feat_channel_raw=R.feat_channel_raw(x, sd), feat_space=R.feat_space(x, taps['M_space']))
        for name, g in got.items():
            assert g.dtype == torch.float64 and g.shape == taps[name].shape, name
            assert R.err(g, taps[name]) <= TOL, (name, R.err(g, taps[name]))
        assert R.err(R.apply_channel(taps['M_channel'], x), taps['feat_channel_raw']) <= TOL
        assert R.err(R.mean7x7(feat_new), f_new) <= TOL
        # the edits reach the taps: clamped norms give zero cosines, never NaN
        assert (taps['ss_space'][2] == 0).all() and (taps['ss_channel'][2] == 0).all()
        assert (taps['ss_channel'][1, 77] == 0).all() and (taps['ss_space'][1, 3 * 7 + 5] == 0).all()
        assert taps['ss_channel'][0, 301, 301] < 1e-12          # below the clamp: not normalised to 1


def plan(lib, N, cus, forced=0):
    rb = ctypes.c_int(-1)
    rc = lib.ffr_plan_channel_rows_host(N, cus, forced, ctypes.byref(rb))
    return rc, rb.value


def restated(N, cus):
    """fewest rounds of one block per CU, weighted with the block time of the form; ties to fewer row blocks"""
    return min((-(-N * rb // cus) * t, rb) for rb, t in BLOCK_US.items())[1]


def test_plan_channel_rows_sweep():
    lib = native.load_library()
    seen = set()
    for cus in (1, 64, 256, 304):
        for N in range(1, 1101):
            rc, rb = plan(lib, N, cus)
            assert rc == 0 and rb == restated(N, cus), (N, cus, rb)
            seen.add((cus, rb))
    assert {rb for cus, rb in seen if cus == 256} == {1, 2, 4}           # every form is reached on the MI355X's 256 CUs
    for N, want in ((64, 4), (65, 2), (128, 2), (129, 1), (257, 1)):
        assert plan(lib, N, 256) == (0, want), N
    for forced in (1, 2, 4):
        for N in (1, 64, 129, 1100):
            assert plan(lib, N, 256, forced) == (0, forced)
    for forced in (3, 5, -1, 8):
        rc, rb = plan(lib, 8, 256, forced)
        assert rc != 0 and rb == -1, forced
    assert plan(lib, 0, 256)[0] != 0 and plan(lib, 8, 0)[0] != 0
    assert lib.ffr_plan_channel_rows_host(8, 256, 0, None) != 0
