"""The split-operand K loop of k_wino_fused (in-kernel input transform, fp32 products as six bf16 x bf16 products on the bf16
matrix cores, option "wf_split") against torch conv2d in float64 on the CPU, beside the fp32-MFMA loop of the same launch.

Errors are max-abs over the tensor's abs-max.  Per case: e32 from use_wino = 1 (fp32 loop), es from use_wino = 5 (split loop);
es < OP_TOL (2e-5, the single-operator bound of test_gpu_parity.py) and es <= 2 * e32: the rounding of the Winograd
transforms is common to both forms and dominates, so es ~ e32 is expected.  Needs a real MI355X: `python -m pytest tests -m gpu`."""
import pytest
import torch
import torch.nn.functional as F

import ffrnet_amd
from ffrnet_amd import synth

pytestmark = pytest.mark.gpu
OP_TOL = 2e-5
REG_TOL = 5e-5


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.fixture(scope='module')
def engine():
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    return ffrnet_amd.Engine(0)


def make_case(case, gen='randn'):
    """Inputs and the float64 reference of one 3x3 / stride 1 / pad 1 launch.  case: N, H, W, cin, cout, mode, prelu, resid."""
    N, H, W, cin, cout, mode, prelu, resid = case
    g = torch.Generator().manual_seed(sum((i + 1) * int(v) for i, v in enumerate(case)) & 0xffff)
    x = torch.randn(N, H, W, cin, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    # PReLU slopes of both signs
    slope = (torch.rand(cout, generator=g) * 0.6 - 0.3) if prelu else None
    r = torch.randn(N, H, W, cout, generator=g) if resid else None
    if gen == 'range':      # input channels scaled by 1e-30 / 1 / 1e30 in turn, the weights of those channels by the inverse square
        # root: products span 1e-15 ... 1e15 and the third bf16 piece of a small channel lies near 1e-36
        sc = torch.tensor([1e-30, 1.0, 1e30])[torch.arange(cin) % 3]
        x = x * sc
        w = w * (1.0 / sc.double().sqrt()).float().view(1, -1, 1, 1)
    xin = x.permute(0, 3, 1, 2).double()
    if mode == 1:
        ref = F.conv2d(F.pad(xin, (1,) * 4, mode='reflect'), w.double(), bias.double())
    else:
        ref = F.conv2d(xin, w.double(), bias.double(), 1, 1)
    if prelu:
        ref = torch.where(ref >= 0, ref, ref * slope.double().view(1, -1, 1, 1))
    if resid:
        ref = ref + r.permute(0, 3, 1, 2).double()
    return dict(x=x.cuda(), w=w, bias=bias, slope=slope, mode=mode, resid=r.cuda() if resid else None), ref


def run(engine, kw, use_wino):
    out = engine.op_conv3x3(kw['x'], kw['w'], kw['bias'], kw['slope'], kw['mode'], use_wino, kw['resid'])
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu()


# N, H, W, cin, cout, pad mode, prelu, resid
CASES = [
    (2, 14, 14, 64, 64, 0, False, False),       # one tile group, two phases
    (3, 13, 11, 64, 128, 0, True, True),        # 36 tiles: a ragged second group, rows beyond T, tiles over both edges, two channel groups
    (2, 7, 7, 96, 64, 1, False, False),         # reflect padding; three phases, an odd count
    (2, 16, 16, 128, 72, 0, False, False),      # four phases; cout no multiple of 64
    # (5 x 8x8, 32 -> 64, a single phase: the hook packs no Winograd weights below cin 64 -- not reachable)
]


@pytest.mark.parametrize('case', CASES)
def test_split_loop_matches_float64(engine, case):
    kw, ref = make_case(case)
    e32 = rel(run(engine, kw, 1), ref)
    es = rel(run(engine, kw, 5), ref)
    print('case %s: e32 %.3e es %.3e' % (case, e32, es))
    assert es < OP_TOL
    assert es <= 2 * e32


def test_extreme_scales(engine):
    """Channels scaled by 1e-30 and 1e30: bf16 has fp32's exponent range, so the pieces neither overflow nor vanish."""
    kw, ref = make_case((2, 14, 14, 96, 128, 0, False, False), gen='range')
    e32 = rel(run(engine, kw, 1), ref)
    got = run(engine, kw, 5)
    es = rel(got, ref)
    print('extreme scales: e32 %.3e es %.3e' % (e32, es))
    assert torch.isfinite(got).all()
    assert es < OP_TOL and es <= 2 * e32


def test_two_runs_are_bitwise_equal(engine):
    kw, ref = make_case(CASES[1])
    assert torch.equal(run(engine, kw, 5), run(engine, kw, 5))


def test_split_form_refuses_wide_layers(engine):
    """cin > wf_phased_maxk: no in-kernel transform, hence no split loop -- an error, not another kernel."""
    kw, ref = make_case((1, 8, 8, 160, 64, 0, False, False))
    with pytest.raises(RuntimeError):
        run(engine, kw, 5)


def test_trunk_runs_the_split_form_and_wf_split_0_is_the_fp32_kernel(state_dicts):
    """Two bottlenecks at 36 images: the 112x112 layer has 882 block tiles and the two 56x56 layers 221, above wf_minblocks = 200,
    so all three transform their own input.  The handle's launch counter tells which form ran."""
    sd_e, _ = state_dicts
    eng = ffrnet_amd.Engine(0)
    assert eng.get_option('wf_split') == 1
    eng.load_encoder(sd_e)
    st = eng.memory_stats()
    assert 0 < st['wf_split_weight_bytes'] < st['encoder_weight_bytes']
    x = synth.synth_images(36, 112, 112, seed=77).cuda()

    def trunk():
        n0 = eng.memory_stats()['wf_split_launches']
        y = eng.encoder_trunk_nhwc(x, 2)
        torch.cuda.synchronize()
        return y, eng.memory_stats()['wf_split_launches'] - n0

    ys, ns = trunk()
    eng.set_option('wf_split', 0)
    y0, n0 = trunk()
    eng.set_option('wf_split', 1)
    ys2, ns2 = trunk()
    eng.set_option('wf_split', 0)
    y1, n1 = trunk()
    print('trunk, 2 blocks, 36 images: split launches %d / %d, |split - fp32| / max %.3e' % (ns, n0, rel(ys, y0)))
    assert ns >= 3 and ns2 == ns and n0 == 0 and n1 == 0
    assert rel(ys, y0) < REG_TOL
    assert torch.equal(y0, y1) and torch.equal(ys, ys2)
