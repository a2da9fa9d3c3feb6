"""The split-operand form of k_igemm (fp32 products as six bf16 x bf16 products on the bf16 matrix cores, option
"igemm_split") against torch conv2d in float64 on the CPU, beside the fp32-MFMA form of the same launch.

Errors are max-abs over the tensor's abs-max.  Per case: e32 of the fp32 form, es of the split form;
es < OP_TOL (2e-5, the single-operator bound of test_gpu_parity.py) and es <= 2 * e32 (the terms the six-product form drops
are bounded by one extra fp32 rounding per product).  Needs a real MI355X: `python -m pytest tests -m gpu`."""
import os

import numpy as np
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


def pack_w(w, cin_pad, cout_pad):
    cout, cin, R, S = w.shape
    p = torch.zeros(cout_pad, R, S, cin_pad, dtype=w.dtype)
    p[:cout, :, :, :cin] = w.permute(0, 2, 3, 1)
    return p.reshape(cout_pad, -1).contiguous()


def border_classes(H, W, R, stride, pad):
    """[Ho, Wo] class 3 * rc + cc of every output pixel: 0 = first tap row / column out of bounds, 2 = last, 1 = neither."""
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    h0 = torch.arange(Ho) * stride - pad
    w0 = torch.arange(Wo) * stride - pad
    rc = torch.where(h0 < 0, 0, torch.where(h0 + R - 1 >= H, 2, 1))
    cc = torch.where(w0 < 0, 0, torch.where(w0 + R - 1 >= W, 2, 1))
    return rc[:, None] * 3 + cc[None, :]


def make_case(case, gen='randn'):
    """Inputs and the float64 reference of one launch.  case: N, H, W, cin, cout, R, stride, pad, mode, prelu, resid, sigmoid,
    tile, border."""
    N, H, W, cin, cout, R, stride, pad, mode, prelu, resid, sig, tile, border = case
    g = torch.Generator().manual_seed(sum((i + 1) * int(v) for i, v in enumerate(case)) & 0xffff)
    cin_pad = (cin + 31) // 32 * 32
    cout_pad = (cout + 63) // 64 * 64
    in_pitch = cin_pad + 32
    ncls = 9 if border else 1
    bias = torch.zeros(ncls, cout_pad)
    slope = torch.zeros(cout_pad)
    if gen == 'int':        # small integers: every product and every partial sum is exact in fp32, in any order
        x = torch.randint(-3, 4, (N, H, W, in_pitch), generator=g).float()
        w = torch.randint(-2, 3, (cout, cin, R, R), generator=g).float()
        bias[:, :cout] = torch.randint(-8, 9, (ncls, cout), generator=g).float()
        slope[:cout] = 0.5
    else:
        x = torch.randn(N, H, W, in_pitch, generator=g)
        w = torch.randn(cout, cin, R, R, generator=g) / (cin * R * R) ** 0.5
        bias[:, :cout] = torch.randn(ncls, cout, generator=g) * 0.1
        slope[:cout] = torch.rand(cout, generator=g) * 0.3 + 0.1
    if gen == 'range':      # input channels scaled by 1e-30 / 1 / 1e30 in turn, the weights of those channels by the inverse square
        # root: products span 1e-15 ... 1e15 and the third bf16 piece of a small channel lies near 1e-36
        sc = torch.tensor([1e-30, 1.0, 1e30])[torch.arange(cin) % 3]
        x[..., :cin] *= sc
        w *= (1.0 / sc.double().sqrt()).float().view(1, -1, 1, 1)
    x[..., cin:cin_pad] = 0
    xin = x[..., :cin].permute(0, 3, 1, 2).double()
    if mode == 1:
        ref = F.conv2d(F.pad(xin, (pad,) * 4, mode='reflect'), w.double(), None, stride)
    else:
        ref = F.conv2d(xin, w.double(), None, stride, pad)
    Ho, Wo = ref.shape[2:]
    if border:
        cls = border_classes(H, W, R, stride, pad)
        ref = ref + bias[:, :cout].double()[cls].permute(2, 0, 1)[None]
    else:
        ref = ref + bias[0, :cout].double().view(1, -1, 1, 1)
    if prelu:
        ref = torch.where(ref >= 0, ref, ref * slope[:cout].double().view(1, -1, 1, 1))
    res_pitch = cout_pad + 64
    r = torch.randn(N, Ho, Wo, res_pitch, generator=g) if gen != 'int' else torch.randint(-5, 6, (N, Ho, Wo, res_pitch), generator=g).float()
    if resid:
        ref = ref + r[..., :cout].permute(0, 3, 1, 2).double()
    if sig:
        ref = torch.sigmoid(ref)
    out_pitch, out_coff = cout_pad + 96, 32
    kw = dict(x=x.cuda(), N=N, H=H, W=W, in_pitch=in_pitch, cin_pad=cin_pad, w=pack_w(w, cin_pad, cout_pad).cuda(),
              bias=bias.cuda(), slope=slope.cuda() if prelu else None, resid=r.cuda() if resid else None, res_pitch=res_pitch,
              out_pitch=out_pitch, out_coff=out_coff, cout_store=cout, cout_pad=cout_pad, R=R, S=R, stride=stride, pad=pad,
              pad_mode=mode, border_bias=1 if border else 0, tile=tile, splitk=0)
    return kw, ref, (N, Ho, Wo, out_pitch, out_coff, cout), sig


def run(engine, kw, shape, sig, split):
    N, Ho, Wo, out_pitch, out_coff, cout = shape
    out = torch.full((N, Ho, Wo, out_pitch), -7.0).cuda()
    engine.op_conv(out=out, flags=(1 if sig else 0) | (2 if split else 0), **kw)
    torch.cuda.synchronize()
    # nothing outside the channel slice was touched
    assert (out[..., :out_coff] == -7.0).all() and (out[..., out_coff + cout:] == -7.0).all()
    return out[..., out_coff:out_coff + cout].permute(0, 3, 1, 2).cpu()


# N, H, W, cin, cout, R, stride, pad, mode, prelu, resid, sigmoid, tile, border
CASES = [
    # the nine CONV_CASES of test_gpu_parity.py: forced tiles 1-4, 3x3 stride 2 with zero padding, 1x1 stride 2, reflect
    # padding, ragged cout, plain-GEMM rows with K = 25088 (a tile cut into segments), the channel-slice store
    (2, 14, 14, 64, 64, 3, 1, 1, 0, True, False, False, 0, 0),
    (3, 14, 14, 64, 128, 3, 2, 1, 0, False, False, False, 1, 0),
    (2, 28, 20, 32, 64, 3, 1, 1, 0, True, True, False, 2, 0),
    (2, 28, 28, 64, 128, 1, 2, 0, 0, False, False, False, 3, 0),
    (5, 7, 7, 96, 49, 3, 1, 1, 1, True, True, True, 0, 0),
    (4, 7, 7, 561, 256, 3, 1, 1, 1, True, False, False, 0, 0),
    (2, 7, 7, 128, 64, 3, 1, 1, 1, True, False, False, 3, 0),
    (2, 16, 16, 64, 64, 3, 1, 1, 0, True, False, False, 4, 0),
    (9, 1, 1, 25088, 512, 1, 1, 0, 0, False, False, False, 0, 0),
    (2, 14, 10, 64, 128, 3, 2, 1, 0, True, True, False, 1, 1),      # the 9 border-class biases, 3x3 stride 2, 128x128 tiles
    (1, 13, 11, 64, 128, 3, 1, 1, 0, True, False, False, 2, 0),     # M = 143: no multiple of BM = 128, rows past M
    (1, 8, 8, 256, 128, 3, 1, 1, 0, False, False, False, 0, 0),     # 2 tiles x 72 K-tiles over 8 blocks: every tile is cut in four
]


@pytest.mark.parametrize('case', CASES)
def test_split_form_matches_float64(engine, case):
    kw, ref, shape, sig = make_case(case)
    e32 = rel(run(engine, kw, shape, sig, False), ref)
    es = rel(run(engine, kw, shape, sig, True), ref)
    print('case %s: e32 %.3e es %.3e' % (case, e32, es))
    assert e32 < OP_TOL
    assert es < OP_TOL
    assert es <= 2 * e32


@pytest.mark.parametrize('case', [(3, 14, 14, 64, 128, 3, 2, 1, 0, True, True, False, 1, 1), (2, 9, 9, 96, 64, 3, 1, 1, 1, True, False, False, 0, 0),
                                  (1, 8, 8, 256, 128, 3, 1, 1, 0, False, False, False, 0, 0)])
def test_small_integers_are_exact(engine, case):
    """Layout, swizzle and plane order: with small-integer data both forms must equal float64 exactly."""
    kw, ref, shape, sig = make_case(case, gen='int')
    for split in (False, True):
        got = run(engine, kw, shape, sig, split)
        assert torch.equal(got.double(), ref), split


def test_extreme_scales(engine):
    """Channels scaled by 1e-30 and 1e30: bf16 has fp32's exponent range, so the pieces neither overflow nor vanish."""
    case = (2, 14, 14, 96, 128, 3, 2, 1, 0, False, False, False, 0, 0)
    kw, ref, shape, sig = make_case(case, gen='range')
    e32 = rel(run(engine, kw, shape, sig, False), ref)
    got = run(engine, kw, shape, sig, True)
    es = rel(got, ref)
    print('extreme scales: e32 %.3e es %.3e' % (e32, es))
    assert torch.isfinite(got).all()
    assert es < OP_TOL and es <= 2 * e32


@pytest.mark.parametrize('case', [CASES[8], CASES[11], CASES[1]])
def test_two_runs_are_bitwise_equal(engine, case):
    """The in-launch fix-up adds the slabs of a cut tile in block order in both forms."""
    kw, ref, shape, sig = make_case(case)
    a = run(engine, kw, shape, sig, True)
    b = run(engine, kw, shape, sig, True)
    assert torch.equal(a, b)


def test_split_flag_needs_the_option(engine):
    kw, ref, shape, sig = make_case(CASES[0])
    engine.set_option('igemm_split', 0)
    try:
        with pytest.raises(RuntimeError):
            run(engine, kw, shape, sig, True)
    finally:
        engine.set_option('igemm_split', 1)


def test_embeddings_default_and_fp32_form(state_dicts, golden_dir):
    """Golden G1 through the default path (split planes made at load time) stays under the regression gate; with
    igemm_split = 0 the same handle runs the fp32 kernels (bit-equal from run to run) and both forms agree far inside the gate."""
    sd_e, sd_r = state_dicts
    eng = ffrnet_amd.Engine(0)
    assert eng.get_option('igemm_split') == 1
    eng.load_encoder(sd_e)
    eng.load_recnet(sd_r)
    st = eng.memory_stats()
    # 4 stride-2 3x3 + 3 shortcuts (1.5 x their fp32 bytes) and the 512 x 25088 output_layer GEMM (77 MB)
    assert 80e6 < st['split_weight_bytes'] < 110e6 and st['split_weight_bytes'] < st['encoder_weight_bytes']
    g = np.load(os.path.join(golden_dir, 'g1_config1.npz'))
    x = synth.synth_images(8, 112, 112, seed=123).cuda()
    f_new, f = eng.embed(x)
    torch.cuda.synchronize()
    es_f, es_fn = rel(f, torch.from_numpy(g['f'])), rel(f_new, torch.from_numpy(g['f_new']))
    eng.set_option('igemm_split', 0)
    f_new0, f0 = eng.embed(x)
    f_new1, f1 = eng.embed(x)
    torch.cuda.synchronize()
    e32_f, e32_fn = rel(f0, torch.from_numpy(g['f'])), rel(f_new0, torch.from_numpy(g['f_new']))
    print('G1: f e32 %.3e es %.3e | f_new e32 %.3e es %.3e' % (e32_f, es_f, e32_fn, es_fn))
    assert es_f < REG_TOL and es_fn < REG_TOL
    assert e32_f < REG_TOL and e32_fn < REG_TOL
    assert torch.equal(f0, f1) and torch.equal(f_new0, f_new1)
    assert rel(f, f0) < REG_TOL and rel(f_new, f_new0) < REG_TOL
