"""Operator tests for every branch of the convolution planners (csrc/plan.cpp) that the product runs at its own batches, each
against a float64 reference of the same operation, with the plan record (Engine.conv_plan) proving which branch ran.

Every branch case names the launch it must reach; the shapes were computed from plan.cpp for 256 CUs.  If a shape lands in
another branch on the device, the shape is what changes, never the assertion.  The record of every Winograd case and of every
direct case without a forced tile is also held, entry by entry, to the answer of ffr_plan_conv_host for the device's CU count
(check_host_plan): the planner that tests/test_host_conv_plan.py sweeps on the host is the one whose entries ran here.

Errors are max-abs over the reference's abs-max.  Bounds: OP_TOL (2e-5, the single-operator bound of test_gpu_parity.py) for the
direct kernel in both forms and for the split-operand Winograd loop, 1e-4 (test_winograd_conv_matches_direct_and_torch) for the
other Winograd forms.  Tile sums: |got - sum| <= 16 * 2^-24 * sum|v| per (tile, channel) against the float64 sum of the values
the same call stored -- a tile has at most 16 values, so at most 15 fp32 additions, each within 2^-24 of a partial sum no larger
than sum|v|.  Needs a real MI355X: `python -m pytest tests -m gpu`."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ffrnet_amd

pytestmark = pytest.mark.gpu
OP_TOL = 2e-5
WINO_TOL = 1e-4
CANARY = -7.0


@pytest.fixture(scope='module')
def engine():
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    return ffrnet_amd.Engine(0)


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def seed_of(*vals):
    return sum((i + 1) * int(v) for i, v in enumerate(vals)) & 0xffff


def recorded(engine, fn):
    """fn() with the plan record on -> (result, the launches it made)."""
    engine.conv_plan_record(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        plan = engine.conv_plan()
    finally:
        engine.conv_plan_record(False)
    return out, plan


HOST_KIND = {'direct': 1, 'unfused-igemm': 1, 'fused': 2, 'unfused-gemm-stream': 3, 'mixed': 4}       # include/ffrnet.h: ffr_plan_conv_host


def check_host_plan(engine, plan, *, cin, cout, N, H, W, in_pitch, out_pitch, out_coff, cout_store, res_pitch, force, R=3, stride=1,
                    pad=1, pad_mode=0, w3=None, mixed=False):
    """The record of one convolution against ffr_plan_conv_host for this device's CU count: what ran is what the host planner
    answers (tests/test_host_conv_plan.py sweeps that answer over the product's table).  Weight sets as pack_conv makes them;
    w3 given: a raw-weight call (op_conv), which has no Winograd weights and the direct split planes its caller asks for."""
    cin_pad = (cin + 31) // 32 * 32
    wino = w3 is None and R == 3 and stride == 1 and pad == 1 and cin_pad >= 64
    w3 = (not wino) if w3 is None else w3
    out = (ctypes.c_longlong * 24)()
    rc = engine.lib.ffr_plan_conv_host(cin, cout, R, stride, pad, pad_mode, int(wino), int(wino and cin_pad <= 128), int(w3), int(mixed), N, H, W,
                                       in_pitch, out_pitch, out_coff, cout_store, res_pitch,
                                       torch.cuda.get_device_properties(0).multi_processor_count, force, out)
    assert rc == 0 and not out[7], list(out)
    sub = ('kind', 'fits', 'tile', 'nblocks', 'granule', 'cut')
    main, rem = dict(zip(sub, out[9:15])), dict(zip(sub, out[15:21]))
    if out[4]:      # a tail split: the header, then the part enqueued first (the remainder when it runs on the second stream)
        assert plan[0]['path'] == 'tail-split' and plan[0]['n_main'] == out[4] and plan[0]['side'] == out[5] and len(plan) == 3, (plan, list(out))
        ran, want = plan[1:], ([rem, main] if out[5] else [main, rem])
    else:
        assert len(plan) == 1 and rem['kind'] == 0, (plan, list(out))
        ran, want = plan, [main]
    for r, w in zip(ran, want):
        assert w['fits'] == 1 and HOST_KIND[r['path']] == w['kind'] and r['tile'] == w['tile'] and r['nblocks'] == w['nblocks'], (r, w)
        if w['kind'] == 1:      # granule and cut are k_igemm's: the host answer leaves them 0 elsewhere, and nothing else cuts a tile
            assert r['granule'] == w['granule'] and r['cut'] == w['cut'], (r, w)
        else:
            assert w['granule'] == 0 and w['cut'] == 0 and r['cut'] == 0, (r, w)


def check_host_plan_wino(engine, plan, kw, cout, use_wino):
    """check_host_plan for a call of run_wino on the inputs of wino_case."""
    N, H, W, in_pitch = kw['x'].shape
    check_host_plan(engine, plan, cin=kw['cin'], cout=cout, N=N, H=H, W=W, in_pitch=in_pitch, out_pitch=kw['out_pitch'],
                    out_coff=kw['out_coff'], cout_store=kw['store'], res_pitch=kw['resid'].shape[3] if kw['resid'] is not None else cout,
                    force=use_wino, pad_mode=kw['pad_mode'], mixed=use_wino == 4)


# ======================================================================================================================
# Direct path (k_igemm through op_conv), both forms
# ======================================================================================================================
def border_classes(H, W, R, stride, pad):
    """[Ho, Wo] class 3 * rc + cc of every output pixel: 0 = first tap row / column out of bounds, 2 = last, 1 = neither."""
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    h0 = torch.arange(Ho) * stride - pad
    w0 = torch.arange(Wo) * stride - pad
    rc = torch.where(h0 < 0, 0, torch.where(h0 + R - 1 >= H, 2, 1))
    cc = torch.where(w0 < 0, 0, torch.where(w0 + R - 1 >= W, 2, 1))
    return rc[:, None] * 3 + cc[None, :]


def pack_w(w, cin_pad, cout_pad):
    cout, cin, R, S = w.shape
    p = torch.zeros(cout_pad, R, S, cin_pad, dtype=w.dtype)
    p[:cout, :, :, :cin] = w.permute(0, 2, 3, 1)
    return p.reshape(cout_pad, -1).contiguous()


def direct_case(c, gen):
    """Inputs (device) and the float64 reference (device, NCHW) of one k_igemm launch."""
    N, H, W, cin, cout, R, stride, pad = c['shape']
    g = torch.Generator().manual_seed(seed_of(*c['shape']))
    dev = torch.device('cuda', 0)
    cin_pad, cout_pad = (cin + 31) // 32 * 32, (cout + 63) // 64 * 64
    in_pitch, res_pitch, out_pitch, out_coff = cin_pad + 32, cout_pad + 64, cout_pad + 96, 32
    ncls = 9 if c['border'] else 1
    bias, slope = torch.zeros(ncls, cout_pad), torch.zeros(cout_pad)
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    if gen == 'int':        # small integers: every product and every partial sum is exact in fp32, in any order
        x = torch.randint(-3, 4, (N, H, W, in_pitch), generator=g).float()
        w = torch.randint(-2, 3, (cout, cin, R, R), generator=g).float()
        bias[:, :cout] = torch.randint(-8, 9, (ncls, cout), generator=g).float()
        slope[:cout] = 0.5
        r = torch.randint(-5, 6, (N, Ho, Wo, res_pitch), generator=g).float()
    else:
        x = torch.randn(N, H, W, in_pitch, generator=g)
        w = torch.randn(cout, cin, R, R, generator=g) / (cin * R * R) ** 0.5
        bias[:, :cout] = torch.randn(ncls, cout, generator=g) * 0.1
        slope[:cout] = torch.rand(cout, generator=g) * 0.6 - 0.3         # both signs
        r = torch.randn(N, Ho, Wo, res_pitch, generator=g)
    x[..., cin:cin_pad] = 0
    xd, rd = x.to(dev), r.to(dev)
    ref = F.conv2d(xd[..., :cin].permute(0, 3, 1, 2).double(), w.to(dev).double(), None, stride, pad)
    if c['border']:
        cls = border_classes(H, W, R, stride, pad).to(dev)
        ref = ref + bias[:, :cout].to(dev).double()[cls].permute(2, 0, 1)[None]
    else:
        ref = ref + bias[0, :cout].to(dev).double().view(1, -1, 1, 1)
    if c['prelu']:
        ref = torch.where(ref >= 0, ref, ref * slope[:cout].to(dev).double().view(1, -1, 1, 1))
    if c['resid']:
        ref = ref + rd[..., :cout].permute(0, 3, 1, 2).double()
    kw = dict(x=xd, N=N, H=H, W=W, in_pitch=in_pitch, cin_pad=cin_pad, w=pack_w(w, cin_pad, cout_pad).to(dev), bias=bias.to(dev),
              slope=slope.to(dev) if c['prelu'] else None, resid=rd if c['resid'] else None, res_pitch=res_pitch, out_pitch=out_pitch,
              out_coff=out_coff, cout_store=cout, cout_pad=cout_pad, R=R, S=R, stride=stride, pad=pad, pad_mode=0,
              border_bias=1 if c['border'] else 0, tile=c['tile'], splitk=0)
    return kw, ref, (N, Ho, Wo, out_pitch, out_coff, cout)


def run_direct(engine, kw, shape, split):
    N, Ho, Wo, out_pitch, out_coff, cout = shape
    out = torch.full((N, Ho, Wo, out_pitch), CANARY, device='cuda')
    engine.op_conv(out=out, flags=2 if split else 0, **kw)
    torch.cuda.synchronize()
    assert (out[..., :out_coff] == CANARY).all() and (out[..., out_coff + cout:] == CANARY).all()     # nothing outside the channel slice
    return out[..., out_coff:out_coff + cout].permute(0, 3, 1, 2)


T128, T128x64, T64, T256 = 1, 2, 3, 4
# shape: N, H, W, cin, cout, R, stride, pad.  fp32 / split: the launch the record must show -- tile, nblocks, tiles, whole (every
# block owns whole tiles: granule == nkt) and cut (the in-launch fix-up runs).
DIRECT_CASES = [
    # `exact`: the tile count is a multiple of the persistent blocks (512 tiles of 128x128 / 1024 of 128x64 on 512 blocks)
    dict(id='1x1s2-exact', shape=(8, 128, 128, 64, 256, 1, 2, 0), prelu=True, resid=False, border=False, tile=0,
         fp32=dict(tile=T128, nblocks=512, tiles=512, whole=True, cut=0), split=dict(tile=T128x64, nblocks=512, tiles=1024, whole=True, cut=0)),
    # whole tiles of a small K (nkt = 2 < 16, tiles >= blocks): 530 / 1060 tiles on 512 blocks, a block owns 1 or 2 / 2 or 3 tiles
    dict(id='1x1s2-whole-small-k', shape=(8, 130, 130, 64, 256, 1, 2, 0), prelu=False, resid=True, border=False, tile=0,
         fp32=dict(tile=T128, nblocks=512, tiles=530, whole=True, cut=0), split=dict(tile=T128x64, nblocks=512, tiles=1060, whole=True, cut=0)),
    dict(id='1x1s2-large-cut', shape=(8, 128, 128, 256, 128, 1, 2, 0), prelu=True, resid=True, border=False, tile=0,
         fp32=dict(tile=T128, nblocks=512, tiles=256, whole=False, cut=1), split=dict(tile=T128x64, nblocks=512, tiles=512, whole=True, cut=0)),
    # M = 8184: rows past M in the last tile; cout 250 of 256: a ragged channel slice at offset 32; the 9 border classes
    dict(id='3x3s2-large-cut', shape=(8, 66, 62, 128, 250, 3, 2, 1), prelu=True, resid=False, border=True, tile=0,
         fp32=dict(tile=T128, nblocks=512, tiles=128, whole=False, cut=1), split=dict(tile=T128, nblocks=256, tiles=128, whole=False, cut=1)),
    dict(id='3x3s2-small-whole', shape=(8, 63, 65, 96, 190, 3, 2, 1), prelu=False, resid=True, border=False, tile=0,
         fp32=dict(tile=T64, nblocks=396, tiles=396, whole=True, cut=0), split=dict(tile=T128x64, nblocks=512, tiles=198, whole=False, cut=1)),
    dict(id='3x3s2-small-whole-392', shape=(16, 56, 56, 64, 128, 3, 2, 1), prelu=True, resid=True, border=True, tile=0,
         fp32=dict(tile=T64, nblocks=392, tiles=392, whole=True, cut=0), split=dict(tile=T128, nblocks=256, tiles=98, whole=False, cut=1)),
    # a forced 256x64 tile on a `large` launch
    dict(id='3x3s2-forced-256x64', shape=(8, 66, 62, 128, 256, 3, 2, 1), prelu=False, resid=False, border=False, tile=T256,
         fp32=dict(tile=T256, nblocks=256, tiles=128, whole=False, cut=1), split=dict(tile=T256, nblocks=256, tiles=128, whole=False, cut=1)),
]


def check_direct_record(plan, want, c, split):
    assert len(plan) == 1, plan
    r = plan[0]
    N, H, W, cin, cout, R, stride, pad = c['shape']
    nkt = R * R * ((cin + 31) // 32 * 32) // 32
    assert r['path'] == 'direct' and r['split'] == int(split) and r['nkt'] == nkt and r['images'] == N, r
    got = dict(tile=r['tile'], nblocks=r['nblocks'], tiles=r['tiles'], whole=r['granule'] == nkt, cut=r['cut'])
    assert got == want, (c['id'], 'split' if split else 'fp32', r)


@pytest.mark.parametrize('c', DIRECT_CASES, ids=[c['id'] for c in DIRECT_CASES])
def test_direct_branch(engine, c):
    # small integers: both forms equal float64 exactly -- the fix-up adds slabs in any order without rounding, so a wrong or
    # missing slab cannot hide
    kw, ref, shape = direct_case(c, 'int')
    for split in (False, True):
        got, plan = recorded(engine, lambda: run_direct(engine, kw, shape, split))
        check_direct_record(plan, c['split' if split else 'fp32'], c, split)
        if not c['tile']:
            check_host_plan(engine, plan, cin=kw['cin_pad'], cout=kw['cout_store'], N=kw['N'], H=kw['H'], W=kw['W'], in_pitch=kw['in_pitch'],
                            out_pitch=kw['out_pitch'], out_coff=kw['out_coff'], cout_store=kw['cout_store'], res_pitch=kw['res_pitch'], force=-1,
                            R=kw['R'], stride=kw['stride'], pad=kw['pad'], w3=split)
        assert torch.equal(got.double(), ref), (c['id'], split)
    kw, ref, shape = direct_case(c, 'randn')
    g32, gs = run_direct(engine, kw, shape, False), run_direct(engine, kw, shape, True)
    e32, es = rel(g32, ref), rel(gs, ref)
    print('direct %s: e32 %.3e es %.3e' % (c['id'], e32, es))
    assert e32 < OP_TOL
    assert es < OP_TOL
    assert es <= 2 * e32
    # the fix-up adds the slabs of a cut tile in block order: two runs are bitwise equal
    if c['fp32']['cut']:
        assert torch.equal(g32, run_direct(engine, kw, shape, False))
    if c['split']['cut']:
        assert torch.equal(gs, run_direct(engine, kw, shape, True))


# ======================================================================================================================
# Winograd path (op_conv3x3_ex)
# ======================================================================================================================
def wino_case(N, H, W, cin, cout, *, in_extra=0, out_extra=0, out_coff=0, res_extra=None, cout_store=0, border=False, prelu=True,
              sigmoid=False, pad_mode=0, sums=True):
    """Inputs (device) and the float64 reference (device, [N, cout_store, H, W]) of one 3x3 / stride 1 / pad 1 convolution with
    the whole epilogue contract.  The reference with `border`: the per-channel affine, then zero padding, then the convolution."""
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(seed_of(N, H, W, cin, cout, in_extra, out_extra, out_coff, cout_store, pad_mode))
    cout_pad = (cout + 63) // 64 * 64
    store = cout_store or cout
    x = torch.randn(N, H, W, cin + in_extra, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    slope = (torch.rand(cout, generator=g) * 0.6 - 0.3) if prelu else None                    # both signs
    in_scale = (torch.rand(cin, generator=g) + 0.5) if border else None
    in_shift = (torch.randn(cin, generator=g) * 0.5) if border else None
    resid = torch.randn(N, H, W, cout_pad + res_extra, generator=g) if res_extra is not None else None
    xin = x[..., :cin].to(dev).double().permute(0, 3, 1, 2)
    if border:
        xin = xin * in_scale.to(dev).double().view(1, -1, 1, 1) + in_shift.to(dev).double().view(1, -1, 1, 1)
    if pad_mode == 1:
        ref = F.conv2d(F.pad(xin, (1,) * 4, mode='reflect'), w.to(dev).double(), bias.to(dev).double())
    else:
        ref = F.conv2d(xin, w.to(dev).double(), bias.to(dev).double(), 1, 1)
    if prelu:
        ref = torch.where(ref >= 0, ref, ref * slope.to(dev).double().view(1, -1, 1, 1))
    if resid is not None:
        ref = ref + resid[..., :cout].to(dev).double().permute(0, 3, 1, 2)
    if sigmoid:
        ref = torch.sigmoid(ref)
    tiles = N * ((H + 3) // 4) * ((W + 3) // 4)
    return dict(x=x.to(dev), w=w, bias=bias, slope=slope, in_scale=in_scale, in_shift=in_shift, resid=resid.to(dev) if resid is not None else None,
                out_pitch=cout_pad + out_extra, out_coff=out_coff, cout_store=cout_store, store=store, cin=cin, cout_pad=cout_pad,
                pad_mode=pad_mode, sigmoid=sigmoid, tiles=tiles, sums=sums), ref[:, :store]


def run_wino(engine, kw, use_wino):
    """-> (stored slice [N, store, H, W], tile sums [T, cout_pad] or None); the canaries around both are checked."""
    x = kw['x']
    N, H, W, _ = x.shape
    out = torch.full((N, H, W, kw['out_pitch']), CANARY, device='cuda')
    want_sums = kw['sums'] and use_wino != 0
    ts = torch.full((kw['tiles'] + 8, kw['cout_pad']), CANARY, device='cuda') if want_sums else None
    engine.op_conv3x3_ex(x, kw['w'], kw['bias'], out, cin=kw['cin'], slope=kw['slope'], in_scale=kw['in_scale'], in_shift=kw['in_shift'],
                         resid=kw['resid'], out_coff=kw['out_coff'], cout_store=kw['cout_store'], pad_mode=kw['pad_mode'],
                         use_wino=use_wino, sigmoid=kw['sigmoid'], tile_sums=ts)
    torch.cuda.synchronize()
    lo, hi = kw['out_coff'], kw['out_coff'] + kw['store']
    assert (out[..., :lo] == CANARY).all() and (out[..., hi:] == CANARY).all()        # nothing outside the channel slice
    if ts is not None:
        assert (ts[kw['tiles']:] == CANARY).all()                                     # nothing behind the last tile
        ts = ts[:kw['tiles']]
    return out[..., lo:hi].permute(0, 3, 1, 2), ts


def tile_slots(H, W, mixed):
    """[(slot within the image, row range, column range)] of the tiles of one map.  F(4x4): raster order.  The exact tiling
    (wino_mixed.hip): the types (4,4), (4,3), (3,4), (3,3) in turn, each in raster order of its own grid."""
    if not mixed:
        tw = (W + 3) // 4
        return [(ty * tw + tx, (4 * ty, min(4 * ty + 4, H)), (4 * tx, min(4 * tx + 4, W))) for ty in range((H + 3) // 4) for tx in range(tw)]
    seg4, seg3 = {14: ([(0, 4), (4, 8)], [(8, 11), (11, 14)]), 7: ([(0, 4)], [(4, 7)])}[H]
    out = []
    for tau in range(4):
        for r in (seg3 if tau >= 2 else seg4):
            for c in (seg3 if tau & 1 else seg4):
                out.append((len(out), r, c))
    return out


def check_tile_sums(got, ts, kw, mixed=False, what=''):
    """ts [T, cout_pad] against the float64 sums of the values the same call stored (got [N, store, H, W])."""
    N, store, H, W = got.shape
    slots = tile_slots(H, W, mixed)
    tpi = len(slots)
    assert ts.shape[0] == N * tpi
    v = got.double()
    want = torch.zeros(N, tpi, kw['cout_pad'], dtype=torch.float64, device=got.device)
    mag = torch.zeros_like(want)
    for k, (r0, r1), (c0, c1) in slots:
        want[:, k, :store] = v[:, :, r0:r1, c0:c1].sum(dim=(2, 3))
        mag[:, k, :store] = v[:, :, r0:r1, c0:c1].abs().sum(dim=(2, 3))
    tsd = ts.double().view(N, tpi, -1)
    bound = 16 * 2.0 ** -24 * mag
    worst = ((tsd - want).abs() - bound).max().item()
    assert worst <= 0, '%s: a tile sum is off by %.3e more than its bound' % (what, worst)        # channels that are not stored: exactly 0
    # per image, the tile sums add up to the plain spatial sum of the stored map
    img = (tsd[..., :store].sum(dim=1) - v.sum(dim=(2, 3))).abs()
    assert (img <= tpi * 16 * 2.0 ** -24 * v.abs().sum(dim=(2, 3))).all(), what


# ---- the Auto choice between Fused, FusedHalf and Unfused, and the tail split ------------------------------------------
# cin, cout, H, W, N, pad mode; the launches the record must show.  form: half_n, phased, split of the k_wino_fused launch.
AUTO_CASES = [
    # 2745 tiles = 86 groups x 3 channel groups = 258 block tiles: 256 fill a round, the images behind the 85 whole groups (302 of
    # 305) run fused with the in-kernel transform and the split-operand loop, the other 3 on the second stream; ragged tiles
    # over both edges of a 9x9 map
    dict(id='fused-phased-split-tail-side', cin=64, cout=192, H=9, W=9, N=305, mode=0, n_main=302, side=1, form=dict(half_n=0, phased=1, split=1), block_tiles=255),
    # n_main a multiple of the 8 images of a tile group
    dict(id='fused-phased-tail-groups', cin=64, cout=256, H=8, W=8, N=516, mode=0, n_main=512, side=1, form=dict(half_n=0, phased=1, split=1), block_tiles=256),
    # V-fed 32 x 32 blocks: 33 groups x 8 = 264 block tiles, the remainder follows on the launch stream
    dict(id='fusedhalf-vfed-tail', cin=256, cout=256, H=7, W=7, N=260, mode=0, n_main=256, side=0, form=dict(half_n=1, phased=0, split=0), block_tiles=256),
    dict(id='fusedhalf-vfed-tail-reflect', cin=256, cout=256, H=7, W=7, N=260, mode=1, n_main=256, side=0, form=dict(half_n=1, phased=0, split=0), block_tiles=256),
    dict(id='fused-vfed-tail', cin=256, cout=256, H=7, W=7, N=520, mode=0, n_main=512, side=0, form=dict(half_n=0, phased=0, split=0), block_tiles=256),
    dict(id='fusedhalf-no-split', cin=256, cout=128, H=7, W=7, N=400, mode=0, n_main=0, side=0, form=dict(half_n=1, phased=0, split=0), block_tiles=200),
    dict(id='unfused-below-minblocks', cin=256, cout=256, H=7, W=7, N=100, mode=0, n_main=0, side=0, form=None, block_tiles=0),
]


@pytest.mark.parametrize('c', AUTO_CASES, ids=[c['id'] for c in AUTO_CASES])
def test_auto_branch(engine, c):
    N, H, W = c['N'], c['H'], c['W']
    kw, ref = wino_case(N, H, W, c['cin'], c['cout'], res_extra=0, pad_mode=c['mode'])
    (got, ts), plan = recorded(engine, lambda: run_wino(engine, kw, -1))
    tiles_img = ((H + 3) // 4) * ((W + 3) // 4)
    paths = [r['path'] for r in plan]
    if c['n_main']:
        assert paths[0] == 'tail-split' and sorted(paths[1:]) == ['fused', 'unfused-gemm-stream'], plan
        assert plan[0]['n_main'] == c['n_main'] and plan[0]['side'] == c['side'] and plan[0]['images'] == N, plan
        # the remainder is enqueued first when it runs on the second stream
        assert paths[1:] == (['unfused-gemm-stream', 'fused'] if c['side'] else ['fused', 'unfused-gemm-stream']), plan
        fused = plan[1 + paths[1:].index('fused')]
        rest = plan[1 + paths[1:].index('unfused-gemm-stream')]
        assert fused['images'] == c['n_main'] and rest['images'] == N - c['n_main'] and rest['rows'] == (N - c['n_main']) * tiles_img, plan
    elif c['form'] is None:
        assert paths == ['unfused-gemm-stream'] and plan[0]['rows'] == N * tiles_img, plan
        fused = None
    else:
        assert paths == ['fused'], plan
        fused = plan[0]
    if fused is not None:
        assert {k: fused[k] for k in c['form']} == c['form'] and fused['block_tiles'] == c['block_tiles'], plan
    check_host_plan_wino(engine, plan, kw, c['cout'], -1)
    direct, _ = run_wino(engine, kw, 0)
    scale = ref.abs().max()
    per_image = (got.double() - ref).abs().amax(dim=(1, 2, 3)) / scale
    e, ed, ew = per_image.max().item(), rel(direct, ref), rel(got, direct)
    print('auto %s: winograd %.3e direct %.3e winograd vs direct %.3e' % (c['id'], e, ed, ew))
    assert e < WINO_TOL and ew < WINO_TOL and ed < OP_TOL
    if c['n_main']:
        # row by row: the images behind n_main are as close to the reference as the ones before it.  Both parts are F(4x4,3x3)
        # in fp32 with the same transforms, and the maximum of the main part runs over 30 to 100 times as many values, so the
        # remainder's maximum has no reason to exceed it, let alone twice; a wrong pointer offset in the split shows here first
        head, tail = per_image[:c['n_main']].max().item(), per_image[c['n_main']:].max().item()
        print('auto %s: images before n_main %.3e, behind %.3e' % (c['id'], head, tail))
        assert tail <= 2 * head
    check_tile_sums(got, ts, kw, what=c['id'])


# ---- the epilogue contract of every form -------------------------------------------------------------------------
# use_wino, cin: k_wino_fused with the in-kernel transform (cin 64) and fed from V (cin 160), 32 x 64 and 32 x 32 blocks, the
# split-operand loop; the transform kernels around k_gemm_stream with k_wino_out; the direct kernel behind the same descriptor
FORMS = [(1, 64), (1, 160), (3, 64), (3, 160), (5, 64), (2, 64), (0, 64)]
# one tile; one tile row with a ragged column; one full tile; ragged both ways; 3x3 tiles with ragged edges; more than one
# block of 32 tiles; whole tiles only
MAPS = [(3, 2, 2), (8, 3, 4), (2, 4, 4), (5, 7, 7), (3, 9, 9), (8, 13, 10), (2, 14, 14)]
VARIANTS = {
    # a channel slice at offset 32 of a wider tensor, a wider input and residual, the 9 border-class biases from a folded affine
    'slice-border': dict(cout=72, in_extra=32, out_extra=96, out_coff=32, res_extra=64, border=True),
    # pitches and an offset that are no multiples of 4 (the scalar-store paths), 49 stored channels, the sigmoid, reflect padding
    'scalar-49': dict(cout=49, out_extra=97, out_coff=33, res_extra=65, sigmoid=True, pad_mode=1),
    # vector stores with a partly stored channel group: 68 of 72 channels
    'ragged-68': dict(cout=72, cout_store=68, out_extra=96, out_coff=32, res_extra=64),
    # scalar stores that end inside a channel quad: 49 of 72 channels, no residual
    'scalar-ragged-49': dict(cout=72, cout_store=49, out_extra=98, out_coff=34, res_extra=None, border=True),
}


@pytest.mark.parametrize('shape', MAPS, ids=['%dx%dx%d' % s for s in MAPS])
@pytest.mark.parametrize('form', FORMS, ids=['wino%d-cin%d' % f for f in FORMS])
def test_epilogue_contract(engine, form, shape):
    use_wino, cin = form
    N, H, W = shape
    tol = OP_TOL if use_wino in (0, 5) else WINO_TOL
    for name, v in VARIANTS.items():
        kw, ref = wino_case(N, H, W, cin, **v)
        (got, ts), plan = recorded(engine, lambda: run_wino(engine, kw, use_wino))
        want = {0: ['direct'], 2: ['unfused-gemm-stream']}.get(use_wino, ['fused'])
        assert [r['path'] for r in plan] == want, plan
        if use_wino in (1, 3, 5):
            assert plan[0]['half_n'] == int(use_wino == 3) and plan[0]['split'] == int(use_wino == 5) and plan[0]['phased'] == int(cin <= 128), plan
        check_host_plan_wino(engine, plan, kw, v['cout'], use_wino)
        e = rel(got, ref)
        print('epilogue wino%d cin %d %dx%dx%d %s: %.3e' % (use_wino, cin, N, H, W, name, e))
        assert e < tol, name
        if ts is not None:
            check_tile_sums(got, ts, kw, what='wino%d %s' % (use_wino, name))


@pytest.mark.parametrize('shape', [(3, 14, 14), (5, 7, 7)], ids=['3x14x14', '5x7x7'])
def test_epilogue_contract_mixed(engine, shape):
    """k_wino_fused_mixed (use_wino = 4) stores whole channel quads from a dense input: it runs the aligned descriptors and
    refuses the others with a reason instead of running another kernel."""
    N, H, W = shape
    runs = {'slice-border': dict(cout=72, out_extra=96, out_coff=32, res_extra=64, border=True),
            'ragged-68': dict(cout=72, cout_store=68, out_extra=96, out_coff=32, res_extra=64)}
    for name, v in runs.items():
        kw, ref = wino_case(N, H, W, 256, **v)
        (got, ts), plan = recorded(engine, lambda: run_wino(engine, kw, 4))
        assert [r['path'] for r in plan] == ['mixed'], plan
        check_host_plan_wino(engine, plan, kw, v['cout'], 4)
        e = rel(got, ref)
        print('epilogue mixed %dx%dx%d %s: %.3e' % (N, H, W, name, e))
        assert e < WINO_TOL, name
        check_tile_sums(got, ts, kw, mixed=True, what='mixed ' + name)
    for name in ('slice-border', 'scalar-49', 'scalar-ragged-49'):      # a wider input; pitches and counts that are no multiples of 4
        kw, ref = wino_case(N, H, W, 256, **VARIANTS[name])
        _, plan = recorded(engine, lambda: pytest.raises(RuntimeError, run_wino, engine, kw, 4))
        assert plan == [], (name, plan)


def test_hook_refuses_what_it_cannot_run(engine):
    """The form that was asked for, or an error with the reason: never another kernel."""
    kw, ref = wino_case(2, 8, 8, 160, 64)
    with pytest.raises(RuntimeError, match='split-operand'):       # cin > wf_phased_maxk: no in-kernel transform, no split loop
        run_wino(engine, kw, 5)
    kw, ref = wino_case(2, 8, 8, 32, 64)
    with pytest.raises(RuntimeError, match='not eligible'):        # cin < wino_mincin: no Winograd weights
        run_wino(engine, kw, -1)
    kw, ref = wino_case(2, 9, 9, 256, 64)
    with pytest.raises(RuntimeError, match='mixed-tile'):          # the exact tiling exists for 14x14 and 7x7 maps
        run_wino(engine, kw, 4)


def test_record_is_off_by_default_and_clears(engine):
    """A fresh handle records nothing; switching the record on clears it, switching it off keeps what it holds."""
    fresh = ffrnet_amd.Engine(0)
    kw, ref = wino_case(2, 8, 8, 64, 64, sums=False)
    run_wino(fresh, kw, 1)
    assert fresh.conv_plan() == []
    _, plan = recorded(fresh, lambda: run_wino(fresh, kw, 1))
    assert [r['path'] for r in plan] == ['fused']
    run_wino(fresh, kw, 2)
    assert fresh.conv_plan() == plan              # off again: nothing is appended
    fresh.conv_plan_record(True)
    assert fresh.conv_plan() == []
    fresh.conv_plan_record(False)
    fresh.close()


def test_record_refuses_a_capturing_stream(engine):
    """A replayed capture would launch without recording: with the record on, a convolution on a capturing stream is an error
    before anything is enqueued; with the record off the same call captures."""
    c = dict(shape=(2, 14, 14, 64, 64, 3, 1, 1), prelu=True, resid=False, border=False, tile=0)
    kw, ref, shape = direct_case(c, 'randn')
    want = run_direct(engine, kw, shape, False)              # outside any capture: the workspace exists from here on
    out = torch.full((shape[0], shape[1], shape[2], shape[3]), CANARY, device='cuda')
    graph = torch.cuda.CUDAGraph()
    engine.conv_plan_record(True)
    try:
        with torch.cuda.graph(graph):
            with pytest.raises(RuntimeError, match='capturing'):
                engine.op_conv(out=out, flags=0, **kw)
    finally:
        engine.conv_plan_record(False)
    torch.cuda.synchronize()
    assert engine.conv_plan() == [] and (out == CANARY).all()
    assert torch.equal(run_direct(engine, kw, shape, False), want)
