"""Operator tests for the four kernels of csrc/recnet_ops.hip -- k_selfsim_space, k_channel_path<4|2|1>, k_space_apply,
k_avgpool49 -- each against the float64 restatement of tests/recnet_ops_ref.py, in every form of the channel path (option
channel_rows 1 / 2 / 4 and the automatic choice) at 1, 2 and 3 images, with the plan record (Engine.conv_plan, path 'channel')
proving which instantiation ran.  Inputs: encoder featmaps of three synthetic images, edited on the host (recnet_ops_ref.
edit_featmaps): a channel below the norm clamp, a zero channel, a zero position, an all-zero image.  Weight sets: seed-0
synthetic and the 'trained' / 'kaiming' families of golden G11.

Bound of the isolated checks.  Errors are max-abs over the reference's abs-max, over every element.  e_ref32 is the error of
the same operator evaluated with torch in fp32 on the CPU, e_gpu that of the kernel, both against float64:
    e_gpu <= max(8 * e_ref32, 4 * 2^-24)
8: the kernel sums the same lengths (49 or 512) in another grouping, folds two linears and uses v_rcp_f32 / __expf in the
sigmoid; two correct fp32 orders differ by a small factor, an index or slope error is >= 1e-2; the rigorous worst case
(gamma_512 ~ 3e-5 per dot product) is an order above.  Every case prints its pair; the largest pairs are listed below.

Bitwise: with channel_rows fixed, an image's ss_space, ss_channel, M_channel and feat_channel_raw are the same bits alone and
at any place in a batch of 3, and the same bits in the three forms.  Arena: a call on NaN featmaps leaves nothing that the next
call reads.  Needs a real MI355X: `python -m pytest tests -m gpu`.

Largest e_gpu with its e_ref32 per tap and weight set, over all forms and batch sizes, measured on one MI355X (the module
prints this table when it is done); no margin was raised:
    tap                 seed0  e_ref32 / e_gpu   trained e_ref32 / e_gpu   kaiming e_ref32 / e_gpu
    ss_space            4.17e-7 / 1.89e-7        4.17e-7 / 2.30e-7         3.58e-7 / 2.52e-7
    feat_space          2.89e-7 / 2.89e-7        3.18e-7 / 3.18e-7         2.87e-7 / 2.87e-7
    feat_channel_raw    4.84e-7 / 1.20e-6        5.19e-7 / 1.03e-6         1.04e-6 / 8.81e-7
    ss_channel          3.94e-7 / 5.00e-7        3.72e-7 / 5.60e-7         3.66e-7 / 4.82e-7
    M_channel           4.81e-7 / 1.85e-7        1.94e-6 / 6.72e-7         9.25e-6 / 2.60e-6
    M_channel_gpu@X     5.21e-7 / 1.21e-6        4.25e-7 / 1.03e-6         5.72e-7 / 9.51e-7
    f_new               9.25e-8 / 1.85e-7        3.62e-8 / 7.24e-8         8.95e-8 / 3.08e-7
feat_channel against the float64 oracle (seed0): 8.8e-6 (REG_TOL 5e-5).  The three forms differ by 0 in every tap."""
import os
import sys

import pytest
import torch

import ffrnet_amd
from ffrnet_amd import synth

import recnet_ops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import ffr_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
MARGIN = 8.0
FLOOR = 4 * 2.0 ** -24
REG_TOL = 5e-5           # test_gpu_parity.py: the regression gate of whole-network taps
FORMS = (1, 2, 4, 0)     # option channel_rows; 0 = the automatic choice, 4 row blocks per image at 1..3 images
WORST = {}               # (family, tap) -> (e_ref32, e_gpu) with the largest e_gpu, printed when the module is done


@pytest.fixture(scope='module')
def engine():
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    eng = ffrnet_amd.Engine(0)          # module-owned: the options it changes are its own
    yield eng
    eng.close()
    for (family, tap), (e_ref, e_gpu) in sorted(WORST.items()):
        print('recnet ops worst  %-8s %-22s e_ref32 %.3e  e_gpu %.3e' % (family, tap, e_ref, e_gpu))


@pytest.fixture(scope='module')
def sets(specs, golden_dir):
    return R.weight_sets(specs, golden_dir)


class Case(object):
    pass


@pytest.fixture(scope='module', params=R.FAMILIES)
def case(request, engine, sets):
    """One weight set loaded into the module's engine, the edited featmaps, and the float64 / fp32 CPU references of all three
    images, computed once (images are independent: the references of a shorter batch are a prefix)."""
    c = Case()
    c.family = request.param
    sd_e, c.sd_r = sets[c.family]
    engine.load_encoder(sd_e)
    engine.load_recnet(c.sd_r)
    fm, _ = engine.encoder_forward(synth.synth_images(3, seed=611).cuda(), want_f=False)
    torch.cuda.synchronize()
    c.x = R.edit_featmaps(fm.cpu())
    c.xd = c.x.cuda()
    c.x64 = c.x.double()
    sd64, sd32 = R.cast(c.sd_r, torch.float64), R.cast(c.sd_r, torch.float32)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with torch.no_grad():
        c.ref = {}
        for name, fn in (('ss_space', lambda x, sd: R.ss_space(x)), ('ss_channel', lambda x, sd: R.ss_channel(x)),
                         ('M_channel', R.m_channel)):
            c.ref[name] = (fn(c.x64, sd64), fn(c.x, sd32))
        c.ref['feat_channel_raw'] = (R.apply_channel(c.ref['M_channel'][0], c.x64), R.apply_channel(c.ref['M_channel'][1], c.x))
        c.feat_channel = None
        if c.family == 'seed0':
            taps = {}
            O.recnet_forward(sd64, c.x64, taps)
            c.feat_channel = taps['feat_channel']
    return c


def recorded(engine, fn):
    """fn() with the plan record on -> (result, the launches it made)"""
    engine.conv_plan_record(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        plan = engine.conv_plan()
    finally:
        engine.conv_plan_record(False)
    return out, plan


class Held(object):
    """Collects the isolated checks of one case: every pair is printed, the failures are asserted together at the end."""

    def __init__(self, family, where):
        self.family, self.where, self.bad = family, where, []

    def __call__(self, tap, got, ref64, ref32):
        e_ref, e_gpu = R.err(ref32, ref64), R.err(got, ref64)
        print('recnet ops  %-8s %-18s %-26s e_ref32 %.3e  e_gpu %.3e' % (self.family, self.where, tap, e_ref, e_gpu))
        key = (self.family, tap.split('[')[0])
        if key not in WORST or e_gpu > WORST[key][1]:
            WORST[key] = (e_ref, e_gpu)
        if not e_gpu <= max(MARGIN * e_ref, FLOOR):
            self.bad.append((tap, e_ref, e_gpu))


def channel_entries(plan, N, rows):
    want = dict(path='channel', images=N, nblocks=N * rows, rows=512 // rows)
    got = [r for r in plan if r['path'] == 'channel']
    return len(got) == 1 and all(got[0][k] == v for k, v in want.items())


@pytest.mark.parametrize('N', [1, 2, 3])
@pytest.mark.parametrize('form', FORMS)
def test_operators_vs_float64(engine, case, form, N):
    c = case
    rows = form if form else 4
    xd, x, x64 = c.xd[:N].contiguous(), c.x[:N], c.x64[:N]
    held = Held(c.family, 'rows=%d N=%d' % (form, N))
    keep = engine.get_option('channel_rows')
    engine.set_option('channel_rows', form)
    try:
        dbg = {}
        for image in sorted({0, N - 1}):
            dbg[image], plan = recorded(engine, lambda: engine.recnet_debug(xd, image=image))
            assert channel_entries(plan, N, rows) and plan[0]['path'] == 'channel' and len(plan) >= 16, plan       # + the 15 convolutions
        (f_new, feat_new), plan = recorded(engine, lambda: engine.recnet_forward(xd))
        assert channel_entries(plan, N, rows), plan
    finally:
        engine.set_option('channel_rows', keep)
    d = {k: v.cpu() for k, v in dbg[0].items()}
    with torch.no_grad():
        held('ss_space', d['ss_space'], c.ref['ss_space'][0][:N], c.ref['ss_space'][1][:N])
        # k_space_apply alone: X @ M_space from the M_space the device made
        held('feat_space', d['feat_space'], R.feat_space(x64, d['M_space'].double()), R.feat_space(x, d['M_space']))
        # the whole of k_channel_path, every row block and every image
        held('feat_channel_raw', d['feat_channel_raw'], c.ref['feat_channel_raw'][0][:N], c.ref['feat_channel_raw'][1][:N])
        for image, di in sorted(dbg.items()):
            ssc, M = di['ss_channel0'].cpu(), di['M_channel0'].cpu()
            held('ss_channel[%d]' % image, ssc, c.ref['ss_channel'][0][image], c.ref['ss_channel'][1][image])
            held('M_channel[%d]' % image, M, c.ref['M_channel'][0][image], c.ref['M_channel'][1][image])
            # P5 / P6 alone: the product with X from the M_channel the device made
            held('M_channel_gpu@X[%d]' % image, di['feat_channel_raw'][image].cpu(),
                 R.apply_channel(M.double()[None], x64[image:image + 1])[0], R.apply_channel(M[None], x[image:image + 1])[0])
            # the two debug calls differ in the stored image only
            for k in ('ss_space', 'M_space', 'feat_space', 'feat_channel_raw', 'feat_channel'):
                assert torch.equal(di[k].cpu(), d[k]), (k, image)
        fn = feat_new.cpu()
        held('f_new', f_new.cpu(), R.mean7x7(fn.double()), R.mean7x7(fn))
        if c.feat_channel is not None:      # the only place the W-flipped half of bufF shows
            e = R.err(d['feat_channel'], c.feat_channel[:N])
            print('recnet ops  %-8s %-18s feat_channel vs float64 oracle %.3e' % (c.family, held.where, e))
            assert e < REG_TOL
    for t in list(d.values()) + [f_new, feat_new]:
        assert torch.isfinite(t).all()
    assert not held.bad, held.bad


def test_images_and_forms_are_bitwise_independent(engine, case):
    """channel_rows fixed: an image gives the same bits alone and as image 0, 1, 2 of a batch of 3 -- ss_space, ss_channel,
    M_channel, feat_channel_raw.  The three forms run the same operation sequence per row, so they give the same bits too."""
    c = case
    keep = engine.get_option('channel_rows')
    taps = ('ss_space', 'ss_channel0', 'M_channel0', 'feat_channel_raw')
    per_form = {}
    try:
        for form in (1, 2, 4):
            engine.set_option('channel_rows', form)
            got = []
            for n in range(3):
                (batch, plan_b) = recorded(engine, lambda: engine.recnet_debug(c.xd, image=n))
                (alone, plan_a) = recorded(engine, lambda: engine.recnet_debug(c.xd[n:n + 1].contiguous()))
                assert channel_entries(plan_b, 3, form) and channel_entries(plan_a, 1, form)
                for k in taps:
                    a = alone[k] if k.endswith('0') else alone[k][0]
                    b = batch[k] if k.endswith('0') else batch[k][n]
                    assert torch.equal(a, b), (form, n, k, R.err(b, a))
                got.append({k: alone[k].cpu() for k in taps})
            per_form[form] = got
    finally:
        engine.set_option('channel_rows', keep)
    worst = 0.0
    for form in (2, 4):
        for n in range(3):
            for k in taps:
                worst = max(worst, R.err(per_form[form][n][k], per_form[1][n][k]))
    print('recnet ops  %-8s largest difference between channel_rows 1 / 2 / 4: %.3e' % (c.family, worst))
    assert worst == 0.0


def test_a_call_leaves_nothing_for_the_next(engine, case):
    """N = 3 on featmaps of NaN, then N = 2 on clean data: every output of the second call is finite and the same bits as on a
    fresh Engine (k_selfsim_space's zero fill of bufS channels 561..575 and every other padded or overhanging read)."""
    c = case
    nan = torch.full((3, 512, 7, 7), float('nan'), device='cuda')
    engine.recnet_debug(nan, image=2)
    engine.recnet_forward(nan)
    torch.cuda.synchronize()
    clean = c.xd[:2].contiguous()
    d = engine.recnet_debug(clean, image=1)
    f_new, feat_new = engine.recnet_forward(clean)
    torch.cuda.synchronize()
    fresh = ffrnet_amd.Engine(0)
    try:
        fresh.load_recnet(c.sd_r)
        d2 = fresh.recnet_debug(clean, image=1)
        g_new, geat_new = fresh.recnet_forward(clean)
        torch.cuda.synchronize()
        for k in d:
            assert torch.isfinite(d[k]).all(), k
            assert torch.equal(d[k], d2[k]), (k, R.err(d[k], d2[k]))
        assert torch.isfinite(f_new).all() and torch.isfinite(feat_new).all()
        assert torch.equal(f_new, g_new) and torch.equal(feat_new, geat_new)
    finally:
        fresh.close()


def test_debug_image_outside_the_batch_is_refused(engine, case):
    for image in (-1, 2, 7):
        with pytest.raises(RuntimeError, match='image'):
            engine.recnet_debug(case.xd[:2].contiguous(), image=image)
    d = engine.recnet_debug(case.xd[:2].contiguous())             # the default is image 0
    d0 = engine.recnet_debug(case.xd[:2].contiguous(), image=0)
    assert all(torch.equal(d[k], d0[k]) for k in d)
