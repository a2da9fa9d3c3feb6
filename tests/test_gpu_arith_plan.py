"""Per-layer convolution arithmetic (include/ffrnet.h: ffr_layer_*, ffr_calibrate): enumeration, the
exactness of the all-Winograd / all-direct plans, mixed plans at every junction of the forward, the calibrated guard on the
trained-like family of golden G11, and the module shells.  Needs a real MI355X: `python -m pytest tests -m gpu`."""
import copy
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import ffrnet_amd
from ffrnet_amd import synth
from ffrnet_amd.native import LayerInfo

pytestmark = pytest.mark.gpu
REG_TOL = 5e-5      # the regression gate of tests/test_gpu_parity.py
ROW_TOL = 2e-5      # a row of a batch of 256 vs the same image in a batch of 8 (tests/test_gpu_parity.py)
FFR_ERR_ARG, FFR_ERR_STATE = -1, -2
TENSORS = ('f', 'featmap', 'f_new', 'feat_new')


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def make_engine(sd_e, sd_r, wino=1):
    eng = ffrnet_amd.Engine(0)
    if wino != 1:
        eng.set_option('wino', wino)
    eng.load_encoder(sd_e)
    eng.load_recnet(sd_r)
    return eng


def outputs(eng, x):
    featmap, f = eng.encoder_forward(x)
    f_new, feat_new = eng.recnet_forward(featmap)
    torch.cuda.synchronize()
    return dict(f=f, featmap=featmap, f_new=f_new, feat_new=feat_new)


def wino_launches(eng, x):
    eng.profile_enable(True)
    outputs(eng, x)
    p = eng.profile_read()
    eng.profile_enable(False)
    return p['wino']['launches'] + p['wino_fused']['launches']


def batch256(x8, seed):
    xb = synth.synth_images(256, 112, 112, seed=seed)
    xb[:8] = x8
    return xb.cuda()


ENC_NAMES = ['body.%d.res_layer.%d' % (i, k) for i in range(24) for k in (1, 3) if k == 1 or i not in (0, 3, 7, 21)]
REC_NAMES = [p + '.conv2d' for p in ('Conv4Space.0', 'Conv4Space.1.conv1', 'Conv4Space.1.conv2', 'Conv4Space.2', 'Conv4Space.3.conv1',
                                     'Conv4Space.3.conv2', 'Conv4Space.4', 'Conv4Space.5.conv1', 'Conv4Space.5.conv2', 'ChannelFlipMerge.0',
                                     'ChannelFlipMerge.1.conv1', 'ChannelFlipMerge.1.conv2', 'Conv4Merge.0', 'Conv4Merge.1.conv1',
                                     'Conv4Merge.1.conv2')]


@pytest.fixture(scope='module')
def engines(state_dicts):
    sd_e, sd_r = state_dicts
    e = dict(plan=make_engine(sd_e, sd_r), default=make_engine(sd_e, sd_r), direct=make_engine(sd_e, sd_r, wino=0))
    yield e
    for v in e.values():
        v.close()


def test_enumeration_and_argument_errors(engines, state_dicts):
    eng = engines['plan']
    ls = eng.layers()
    enc = [l['name'] for l in ls if l['net'] == 'encoder']
    rec = [l['name'] for l in ls if l['net'] == 'recnet']
    assert len(enc) == 44 and enc == ENC_NAMES
    assert rec == REC_NAMES                       # every RecNet ConvLayer is packed for Winograd (padded cin >= 64)
    sd_e, sd_r = state_dicts
    for n in enc:
        assert n + '.weight' in sd_e
    for n in rec:
        assert n + '.weight' in sd_r
    assert all(l['arith'] == 'winograd' and l['sensitivity'] is None for l in ls)
    lib, h, n = eng.lib, eng._h, len(ls)
    li = LayerInfo()
    assert lib.ffr_layer_get(h, n, C.byref(li)) == FFR_ERR_ARG
    assert lib.ffr_layer_get(h, -1, C.byref(li)) == FFR_ERR_ARG
    assert lib.ffr_layer_set_arith(h, n, 0) == FFR_ERR_ARG
    assert lib.ffr_layer_set_arith(h, 0, 2) == FFR_ERR_ARG
    assert lib.ffr_layer_set_arith(h, 0, -1) == FFR_ERR_ARG
    # a plan change moves the generation (a captured graph would replay the old plan); setting the same value does not
    g0 = eng.generation()
    eng.set_layer_arith(0, 'winograd')
    assert eng.generation() == g0
    eng.set_layer_arith('body.0.res_layer.1', 'direct')
    assert eng.generation() != g0 and eng.layers()[0]['arith'] == 'direct'
    eng.set_arithmetic_plan({})
    assert all(l['arith'] == 'winograd' for l in eng.layers())
    # a load resets that net's plan only
    eng.set_layer_arith(REC_NAMES[0], 'direct')
    eng.set_layer_arith(ENC_NAMES[5], 'direct')
    eng.load_recnet(sd_r)
    plan = eng.arithmetic_plan()
    assert plan[REC_NAMES[0]] == 'winograd' and plan[ENC_NAMES[5]] == 'direct'
    eng.set_arithmetic_plan({})


@pytest.mark.parametrize('n', [8, 256])
def test_uniform_plans_are_bit_identical(engines, n):
    """All-Winograd = a fresh default handle, all-direct = a wino = 0 handle, bit for bit, on every output tensor."""
    eng = engines['plan']
    x = synth.synth_images(n, 112, 112, seed=3100 + n).cuda()
    ref_w, ref_d = outputs(engines['default'], x), outputs(engines['direct'], x)
    eng.set_arithmetic_plan({})
    got = outputs(eng, x)
    for k in TENSORS:
        assert torch.equal(got[k], ref_w[k]), ('all-winograd', k)
    eng.set_arithmetic_plan({l['name']: 'direct' for l in eng.layers()})
    got = outputs(eng, x)
    for k in TENSORS:
        assert torch.equal(got[k], ref_d[k]), ('all-direct', k)
    assert wino_launches(eng, x) == 0
    eng.set_arithmetic_plan({})


MIXED_PLANS = {
    'conv1': lambda names: [n for n in names if n.endswith('res_layer.1')],
    'conv2': lambda names: [n for n in names if n.endswith('res_layer.3')],
    'alternating': lambda names: names[::2],
    'stage3': lambda names: [n for n in names if n.startswith('body.') and 7 <= int(n.split('.')[1]) <= 20],
    'one_recnet_conv': lambda names: ['Conv4Merge.1.conv1.conv2d'],
}


def test_mixed_plans_at_every_junction(engines, golden_dir):
    """Pinned and Winograd layers side by side: the combine that writes V (k_combine_in_c / k_combine_in_mixed) only for a
    Winograd conv1, the SE squeeze from the tile sums only of a Winograd conv2, the exact tiling, the tail split.  Each plan is held to
    golden G1 at the regression gate (batch 8), every row of batch 256 to its batch-8 run, and to the profile: a pinned layer
    launches no Winograd kernel, so the Winograd launch count drops by exactly the launches the pinned layers make by default."""
    eng = engines['plan']
    names = [l['name'] for l in eng.layers()]
    g = np.load(os.path.join(golden_dir, 'g1_config1.npz'))
    x8 = synth.synth_images(8, 112, 112, seed=123)
    xs = {8: x8.cuda(), 256: batch256(x8, 3300)}
    eng.set_arithmetic_plan({})
    base = {n: wino_launches(eng, xs[n]) for n in xs}
    own = {}                                       # Winograd launches of one layer in the default plan, per batch size

    def own_launches(name, n):
        if (name, n) not in own:
            eng.set_arithmetic_plan({name: 'direct'})
            own[(name, n)] = base[n] - wino_launches(eng, xs[n])
            assert own[(name, n)] >= 1, (name, n)
        return own[(name, n)]

    for tag, pick in MIXED_PLANS.items():
        pinned = pick(names)
        assert pinned
        plan = {p: 'direct' for p in pinned}
        eng.set_arithmetic_plan(plan)
        assert sum(a == 'direct' for a in eng.arithmetic_plan().values()) == len(pinned)
        o8 = outputs(eng, xs[8])
        for k, key in (('f', 'f'), ('f_new', 'f_new')):
            assert rel(o8[k], torch.from_numpy(g[key])) < REG_TOL, (tag, k)
        assert rel(o8['featmap'][0], torch.from_numpy(g['featmap0'])) < REG_TOL, tag
        assert rel(o8['feat_new'][0], torch.from_numpy(g['feat_new0'])) < REG_TOL, tag
        ob = outputs(eng, xs[256])
        xb = xs[256]
        for i in range(0, 256, 8):
            oi = outputs(eng, xb[i:i + 8].contiguous())
            for k in TENSORS:
                assert rel(ob[k][i:i + 8], oi[k]) < ROW_TOL, (tag, k, i)
        for n in (8, 256):
            eng.set_arithmetic_plan(plan)
            got = wino_launches(eng, xs[n])
            want = base[n] - sum(own_launches(p, n) for p in pinned)
            assert got == want, (tag, n, got, want)
    eng.set_arithmetic_plan({})


def _stress_engines(fam, specs, golden_dir):
    sd_e, sd_r = synth.stress_state_dicts(fam, specs['encoder'], specs['recnet'], golden_dir)
    return make_engine(sd_e, sd_r), make_engine(sd_e, sd_r, wino=0)


def test_calibrated_guard_on_the_trained_like_family(specs, golden_dir):
    """G11 'trained' (BatchNorm running_var over 5 decades, saturated SE gates): the tolerance is a quarter of the MEASURED
    default-vs-direct distance on the calibration images; the calibration must pin layers, meet tol / 2 on those images
    and tol on held-out ones (G11's own 8 images as rows 0..7 of another batch of 256)."""
    g = np.load(os.path.join(golden_dir, 'g11_trained.npz'))
    img_seed = synth.STRESS_FAMILIES['trained'][4]
    eng, direct = _stress_engines('trained', specs, golden_dir)
    xc = synth.synth_images(256, 112, 112, seed=img_seed + 1000).cuda()
    o_def, o_dir = outputs(eng, xc), outputs(direct, xc)
    d = max(rel(o_def[k], o_dir[k]) for k in TENSORS)
    assert d > 0
    tol = d / 4.0
    rep = eng.calibrate(x=xc, tol=tol)
    pinned = [l['name'] for l in rep['layers'] if l['arith'] == 'direct']
    assert pinned, rep
    assert all(l['sensitivity'] is not None and l['sensitivity'] >= 0 for l in rep['layers'])
    for k in TENSORS:
        assert rep['achieved'][k] is not None and rep['achieved'][k] <= tol / 2, (k, rep['achieved'], tol)
    o_cal = outputs(eng, xc)
    for k in TENSORS:
        assert rel(o_cal[k], o_dir[k]) <= tol / 2 * 1.0001, k
    # held out
    x8 = synth.synth_images(8, 112, 112, seed=img_seed)
    xh = batch256(x8, img_seed + 2000)
    h_cal, h_dir = outputs(eng, xh), outputs(direct, xh)
    held = {k: rel(h_cal[k], h_dir[k]) for k in TENSORS}
    for k in TENSORS:
        assert held[k] <= tol, (k, held, tol)
    eng.set_arithmetic_plan({})
    h_def = outputs(eng, xh)
    rows = []
    for k, key, sel in (('f', 'f', lambda t: t[:8]), ('f_new', 'f_new', lambda t: t[:8]),
                        ('featmap', 'featmap0', lambda t: t[0]), ('feat_new', 'feat_new0', lambda t: t[0])):
        ref64 = torch.from_numpy(g[key + '_f64'])
        amax = ref64.abs().max().item()
        e = [(sel(o[k]).double().cpu() - ref64).abs().max().item() / amax for o in (h_def, h_dir, h_cal)]
        own = (torch.from_numpy(g[key]).double() - ref64).abs().max().item() / amax
        rows.append((k, e[0], e[1], e[2], own))
    print('\ntol %.3g (d = %.3g), %d of %d layers pinned: %s' % (tol, d, len(pinned), len(rep['layers']), pinned))
    print('%-9s %12s %12s %12s %12s' % ('tensor', 'default', 'direct', 'calibrated', 'ref fp32'))
    for r in rows:
        print('%-9s %12.3e %12.3e %12.3e %12.3e' % r)
    eng.close()
    direct.close()


def test_no_needless_pinning_on_a_benign_family(specs, golden_dir):
    eng, direct = _stress_engines('benign_s1', specs, golden_dir)
    direct.close()
    ref = make_engine(*synth.stress_state_dicts('benign_s1', specs['encoder'], specs['recnet'], golden_dir))
    x = synth.synth_images(256, 112, 112, seed=7100).cuda()
    rep = eng.calibrate(x=x, tol=1e-4)
    assert all(l['arith'] == 'winograd' for l in rep['layers']), [l['name'] for l in rep['layers'] if l['arith'] == 'direct']
    assert all(v is not None and v <= 5e-5 for v in rep['achieved'].values()), rep['achieved']
    a, b = outputs(eng, x), outputs(ref, x)
    for k in TENSORS:
        assert torch.equal(a[k], b[k]), k
    eng.close()
    ref.close()


def test_module_shells_calibrate_and_follow_the_weights(state_dicts):
    sd_e, sd_r = state_dicts
    enc = ffrnet_amd.Backbone(num_layers=50, drop_ratio=0.6, mode='ir_se')
    rec = ffrnet_amd.RecNet(norm_type='bn', relu_type='prelu')
    enc.load_state_dict(sd_e)
    rec.load_state_dict(sd_r)
    enc.to('cuda').eval()
    rec.to('cuda').eval()
    keys_e, keys_r = list(enc.state_dict().keys()), list(rec.state_dict().keys())
    x = synth.synth_images(64, 112, 112, seed=7200).cuda()
    with torch.no_grad():
        fm0, f0 = enc(x)
        fn0, _ = rec(fm0)
    # a tolerance far below the Winograd-vs-direct distance of these weights: layers get pinned
    rep = enc.calibrate_arithmetic(x, tol=1e-7)
    assert len(rep['layers']) == 44 and all(l['net'] == 'encoder' for l in rep['layers'])
    assert any(l['arith'] == 'direct' for l in rep['layers'])
    assert rep['achieved']['f'] <= 5e-8 and rep['achieved']['featmap'] <= 5e-8
    rep_r = rec.calibrate_arithmetic(fm0, tol=1e-7)
    assert len(rep_r['layers']) == 15 and rep_r['achieved']['f_new'] <= 5e-8 and rep_r['achieved']['f'] is None
    with torch.no_grad():
        fm1, f1 = enc(x)
        fn1, _ = rec(fm1)
    assert rel(f1, f0) < 1e-4 and rel(fn1, fn0) < 1e-4
    # set_arithmetic_plan(arithmetic_plan()) changes nothing
    plan = enc.arithmetic_plan()
    assert plan == {l['name']: l['arith'] for l in rep['layers']}
    enc.set_arithmetic_plan(plan)
    rec.set_arithmetic_plan(rec.arithmetic_plan())
    with torch.no_grad():
        fm2, f2 = enc(x)
        fn2, _ = rec(fm2)
    assert torch.equal(f2, f1) and torch.equal(fm2, fm1) and torch.equal(fn2, fn1)
    # deepcopy carries the calibration
    enc_c = copy.deepcopy(enc)
    with torch.no_grad():
        fm3, f3 = enc_c(x)
    assert enc_c.arithmetic_plan() == plan and torch.equal(f3, f1)
    # an in-place weight edit re-packs and recalibrates
    n_cal = enc._arith['calibrations']
    w9 = enc.body[9].res_layer[1].weight.detach().clone()
    with torch.no_grad():
        enc.body[9].res_layer[1].weight.mul_(1.001)
        enc(x)
    assert enc._arith['calibrations'] == n_cal + 1 and enc.calibration_report() is not rep
    assert list(enc.state_dict().keys()) == keys_e and list(rec.state_dict().keys()) == keys_r
    assert len(keys_e) == 402 and len(keys_r) == 121
    # a different plan changes the arithmetic; clear_calibration returns to the default bits
    enc.set_arithmetic_plan({n: 'direct' for n in plan})
    assert all(a == 'direct' for a in enc.arithmetic_plan().values())
    enc.clear_calibration()
    rec.clear_calibration()
    assert all(a == 'winograd' for a in enc.arithmetic_plan().values())
    with torch.no_grad():
        enc.body[9].res_layer[1].weight.copy_(w9)
        fm4, f4 = enc(x)
        fn4, _ = rec(fm4)
    ref = make_engine(sd_e, sd_r)
    o = outputs(ref, x)
    assert torch.equal(f4, o['f']) and torch.equal(fm4, o['featmap']) and torch.equal(fn4, o['f_new'])
    ref.close()


def test_calibration_refusals(state_dicts):
    """Clean errors, nothing crashes: tol 0 / negative / NaN, both or neither input, no net loaded.  (The capture check is the
    first thing ffr_calibrate does, before anything is enqueued; it is held by reading the code, not by a capture.)"""
    sd_e, sd_r = state_dicts
    empty = ffrnet_amd.Engine(0)
    x = synth.synth_images(2, 112, 112, seed=1).cuda()
    fm = torch.zeros((2, 512, 7, 7), device='cuda')
    lib, h = empty.lib, empty._h
    assert lib.ffr_calibrate(h, C.c_void_p(x.data_ptr()), None, 2, 112, 112, 1e-3, None, None) == FFR_ERR_STATE
    assert lib.ffr_calibrate(h, None, C.c_void_p(fm.data_ptr()), 2, 7, 7, 1e-3, None, None) == FFR_ERR_STATE
    with pytest.raises(RuntimeError):
        empty.calibrate(x=x, tol=1e-3)
    n = C.c_int(-1)
    assert lib.ffr_layer_count(h, C.byref(n)) == 0 and n.value == 0
    empty.load_encoder(sd_e)
    lib, h = empty.lib, empty._h
    for tol in (0.0, -1.0, math.nan):
        assert lib.ffr_calibrate(h, C.c_void_p(x.data_ptr()), None, 2, 112, 112, tol, None, None) == FFR_ERR_ARG, tol
        with pytest.raises(RuntimeError):
            empty.calibrate(x=x, tol=tol)
    assert lib.ffr_calibrate(h, C.c_void_p(x.data_ptr()), C.c_void_p(fm.data_ptr()), 2, 112, 112, 1e-3, None, None) == FFR_ERR_ARG
    assert lib.ffr_calibrate(h, None, None, 2, 112, 112, 1e-3, None, None) == FFR_ERR_ARG
    for bad in (dict(), dict(x=x, featmap=fm)):
        with pytest.raises(RuntimeError):
            empty.calibrate(tol=1e-3, **bad)
    # RecNet's layers need RecNet's weights
    assert lib.ffr_calibrate(h, None, C.c_void_p(fm.data_ptr()), 2, 7, 7, 1e-3, None, None) == FFR_ERR_STATE
    assert all(l['arith'] == 'winograd' for l in empty.layers())          # nothing changed on any refusal
    empty.close()
