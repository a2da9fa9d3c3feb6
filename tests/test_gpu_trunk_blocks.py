"""The encoder trunk block by block at the small input sizes the library accepts: the code between the convolutions -- stem, SE
squeeze from either source, the three forms of the residual combine, the chained conv1 -> conv2 transform, Backbone.bn -- in
every shape-dependent branch of run_trunk (csrc/forward.cpp), each against float64, with the plan record (Engine.conv_plan)
proving which glue launch ran.

Method (test_se_module_isolated's): the activation after `i` bottlenecks is the exact input of bottleneck i, the one after i + 1
its output; both come from Engine.encoder_trunk_nhwc.  b1 = trunk(x, i + 1) is held to block64(i, trunk(x, i)); with count 2,
b2 = trunk(x, i + 2) is held to block64(i + 1, b1): in that run block i makes its combine with a look-ahead to block i + 1's
conv1 (the V-writing combines), and block i + 1 consumes both the NHWC output and V.  The cases, with the launch each must
reach as a literal, are tests/trunk_ref.py's table.  Every output buffer is preset to NaN and must come back finite.
The NCHW featmap of ffr_encoder_forward (k_nhwc_to_nchw moves 64 cells per block) is held to Backbone.bn at maps of 4, 15, 64, 66, 72
and 196 cells, to the uint8 entry bit for bit at 72, and to guard bands around the caller's tensor at 15 and 72.

Bounds.  Errors are max-abs over the reference's abs-max, over every element of a block's output.
  * a block in which a convolution runs Winograd: REG_TOL = 5e-5 (test_se_module_isolated's bound of a whole bottleneck);
  * option wino = 0 (direct arithmetic, __expf in the SE sigmoid), the stem and Backbone.bn: e_ref32 is the error of the same
    piece in torch fp32 on the CPU against float64 on the same input, and e_gpu <= max(8 * e_ref32, 4 * 2^-24) -- the margin
    and floor of test_gpu_recnet_ops.py: two correct fp32 summation orders differ by a small factor, an index, slope or
    scale error is 1e-2 or more.
Every case prints its (e_ref32, e_gpu) pairs; the module prints the largest pair per branch when it is done.
Needs a real MI355X: `python -m pytest tests -m gpu`.

Largest e_gpu with its e_ref32 per branch and weight set (e_ref32 / e_gpu), measured on one MI355X; no margin was raised.  Only
the `wino = 0`, stem and head rows are held to the measured rule (largest ratio 3.0), the others to REG_TOL:
    branch                  seed0                trained              ir (no SEModule)
    plain                   1.63e-7 / 2.71e-6    4.08e-7 / 4.08e-6    3.35e-7 / 9.98e-7
    se-pool                 1.05e-7 / 2.53e-6    4.39e-7 / 4.53e-6
    se-pool, wino = 0       1.06e-7 / 3.14e-7    3.83e-7 / 1.14e-6
    se-tiles                1.11e-7 / 2.04e-6    3.06e-7 / 4.88e-6
    combine-in-c            2.08e-7 / 4.16e-6    4.47e-6 / 1.19e-5    2.72e-7 / 5.27e-6
    combine-in-c-refused    1.33e-7 / 3.64e-6
    combine-v-off           1.90e-7 / 3.57e-6
    wino-out-in             1.63e-7 / 2.71e-6    7.98e-7 / 9.05e-6
    wino-out-in-refused     1.76e-7 / 2.34e-6
    combine-in-mixed        1.66e-7 / 3.72e-6    3.83e-7 / 8.86e-6
    stem                    1.87e-7 / 2.44e-7
    head-bn                 1.02e-7 / 7.80e-8"""
import contextlib
import ctypes as C
import os

import pytest
import torch

import ffrnet_amd
from ffrnet_amd import native, synth

import trunk_ref as T

O = T.O

pytestmark = pytest.mark.gpu
REG_TOL = 5e-5
MARGIN = 8.0
FLOOR = 4 * 2.0 ** -24
WINOGRAD = ('fused', 'unfused-gemm-stream', 'unfused-igemm', 'mixed')
SE_PATHS = (T.POOL, T.TILES)
COMBINES = (T.PLAIN, T.IN_C, T.IN_MIXED)
WORST = {}               # (branch, family) -> (e_ref32, e_gpu) with the largest e_gpu, printed when the module is done
LOADED = {}


@pytest.fixture(scope='module')
def engine():
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    eng = ffrnet_amd.Engine(0)          # module-owned: the options it changes are its own
    yield eng
    eng.close()
    LOADED.clear()
    for (branch, family), (e_ref, e_gpu) in sorted(WORST.items()):
        print('trunk blocks worst  %-22s %-8s e_ref32 %.3e  e_gpu %.3e' % (branch, family, e_ref, e_gpu))


@pytest.fixture(scope='module')
def sets(specs, golden_dir):
    return T.weight_sets(specs, golden_dir)


def use(engine, sets, family):
    """The weight set `family` in the module's engine (loaded when it changes) -> its float64 and float32 state_dicts."""
    if LOADED.get('family') != family:
        engine.load_encoder(sets[family])
        LOADED.update(family=family, sd64=T.cast(sets[family], torch.float64), sd32=T.cast(sets[family], torch.float32))
    return LOADED['sd64'], LOADED['sd32']


@contextlib.contextmanager
def options(engine, opts):
    keep = {k: engine.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            engine.set_option(k, v)
        yield
    finally:
        for k, v in keep.items():
            engine.set_option(k, v)


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


def trunk(engine, x, n_blocks):
    """stem + n_blocks bottlenecks into a buffer preset to NaN -> NCHW view"""
    chans, div = 64, 1
    for cin, depth, stride in O.ir_blocks(50)[:n_blocks]:
        chans, div = depth, div * stride
    out = torch.full((x.size(0), x.size(2) // div, x.size(3) // div, chans), float('nan'), device='cuda')
    engine.encoder_trunk_nhwc(x, n_blocks, out=out)
    return out.permute(0, 3, 1, 2)


def per_block(plan):
    """the record of a trunk run, cut behind every combine entry: one list per bottleneck"""
    groups, cur = [], []
    for r in plan:
        cur.append(r)
        if r['path'] in COMBINES:
            groups.append(cur)
            cur = []
    assert not cur, cur
    return groups


def note(branch, family, e_ref, e_gpu):
    key = (branch, family)
    if key not in WORST or e_gpu > WORST[key][1]:
        WORST[key] = (e_ref, e_gpu)


def measured_ok(e_ref, e_gpu):
    return e_gpu <= max(MARGIN * e_ref, FLOOR)


def check_record(c, plan, n_blocks):
    N, i, w = c['N'], c['i'], c['want']
    groups = per_block(plan)
    assert len(groups) == n_blocks, plan
    g = groups[i]
    cin, depth, stride = O.ir_blocks(50)[i]
    ho, wo = T.stage_maps(c['H'], c['W'])[(64, 128, 256, 512).index(depth)]
    se = [r for r in g if r['path'] in SE_PATHS]
    if w['se'] is None:
        assert not [r for r in plan if r['path'] in SE_PATHS], plan
    else:
        assert len(se) == 1 and (se[0]['path'], se[0]['tiles']) == w['se'] and (se[0]['images'], se[0]['rows']) == (N, ho * wo), g
    comb = g[-1]
    assert (comb['path'], comb['stride'], comb['conv_shortcut'], comb['tiles']) == w['combine'], g
    assert (comb['images'], comb['rows'], comb['se_scale']) == (N, ho * wo, int(w['se'] is not None)), g
    chained = [r for r in g if r['path'] == 'wino-out-in']
    if w['chained']:
        assert len(chained) == 1 and (chained[0]['images'], chained[0]['tiles'], chained[0]['rows']) == \
            (N, w['chained_tiles'], N * w['chained_tiles']), g
    else:
        assert not chained, g
    # which bound applies: under option wino = 0 no convolution of the block runs Winograd, otherwise one does
    wino = [r for r in g if r['path'] in WINOGRAD]
    assert (not wino) if c['opts'].get('wino') == 0 else wino, g


@pytest.mark.parametrize('case', T.CASES, ids=[c['id'] for c in T.CASES])
def test_block_vs_float64(engine, sets, case):
    c = case
    sd64, sd32 = use(engine, sets, c['family'])
    N, H, W, i, count = c['N'], c['H'], c['W'], c['i'], c['count']
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    x = synth.synth_images(N, H, W, seed=700 + i).cuda()
    with options(engine, c['opts']):
        a = trunk(engine, x, i)
        if count == 1:
            b1, plan = recorded(engine, lambda: trunk(engine, x, i + 1))
            outs = [a, b1]
        else:
            b1 = trunk(engine, x, i + 1)
            b2, plan = recorded(engine, lambda: trunk(engine, x, i + 2))
            outs = [a, b1, b2]
    torch.cuda.synchronize()
    check_record(c, plan, i + count)
    for t in outs:
        assert torch.isfinite(t).all()
    sel = list(c['images']) if c['images'] else list(range(N))
    outs = [t[sel].cpu().contiguous() for t in outs]
    bad = []
    with torch.no_grad():
        for k in range(count):
            ref64 = T.block(sd64, i + k, outs[k].double())
            e_ref, e_gpu = T.err(T.block(sd32, i + k, outs[k]), ref64), T.err(outs[k + 1], ref64)
            print('trunk blocks  %-60s block %2d  e_ref32 %.3e  e_gpu %.3e' % (c['id'], i + k, e_ref, e_gpu))
            note(c['branch'] + (', wino = 0' if c['opts'].get('wino') == 0 else ''), c['family'], e_ref, e_gpu)
            if not (measured_ok(e_ref, e_gpu) if c['opts'].get('wino') == 0 else e_gpu < REG_TOL):
                bad.append((i + k, e_ref, e_gpu))
    assert not bad, bad


@pytest.mark.parametrize('shape', T.STEM_SHAPES, ids=['%dx%dx%d' % s for s in T.STEM_SHAPES])
def test_stem_vs_float64(engine, sets, shape):
    """k_stem at other sizes than 112x112: one ragged block, a ragged last block of several, a non-square map"""
    sd64, sd32 = use(engine, sets, 'seed0')
    N, H, W = shape
    x = synth.synth_images(N, H, W, seed=31)
    got = trunk(engine, x.cuda(), 0)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    with torch.no_grad():
        ref64 = T.stem(sd64, x.double())
        e_ref, e_gpu = T.err(T.stem(sd32, x), ref64), T.err(got, ref64)
    print('trunk blocks  stem %dx%dx%d  e_ref32 %.3e  e_gpu %.3e' % (N, H, W, e_ref, e_gpu))
    note('stem', 'seed0', e_ref, e_gpu)
    assert measured_ok(e_ref, e_gpu), (e_ref, e_gpu)


@pytest.mark.parametrize('shape', T.HEAD_SHAPES, ids=['%dx%dx%d' % s for s in T.HEAD_SHAPES])
def test_head_bn_vs_float64(engine, sets, shape):
    """Backbone.bn (k_affine) on the device's own 24-block tap, read as the NCHW featmap: k_nhwc_to_nchw below one chunk of 64
    cells, at exactly one, and over several with a ragged last one; asking for f at these sizes fails as in the reference"""
    sd64, sd32 = use(engine, sets, 'seed0')
    N, H, W = shape
    x = synth.synth_images(N, H, W, seed=32).cuda()
    tap = trunk(engine, x, 24)
    fm, f = engine.encoder_forward(x, want_f=False)
    torch.cuda.synchronize()
    assert f is None and tuple(fm.shape) == (N, 512, H // 16, W // 16) and torch.isfinite(fm).all() and torch.isfinite(tap).all()
    tap = tap.cpu().contiguous()
    with torch.no_grad():
        ref64 = T.head_bn(sd64, tap.double())
        e_ref, e_gpu = T.err(T.head_bn(sd32, tap), ref64), T.err(fm, ref64)
    print('trunk blocks  head bn %dx%dx%d  e_ref32 %.3e  e_gpu %.3e' % (N, H, W, e_ref, e_gpu))
    note('head-bn', 'seed0', e_ref, e_gpu)
    assert measured_ok(e_ref, e_gpu), (e_ref, e_gpu)
    with pytest.raises(RuntimeError, match='25088x512'):
        engine.encoder_forward(x)


def test_u8_stem_is_bit_identical_at_a_small_size(engine, sets):
    """k_stem<U8> with mixed flip flags on a 48x80 map against the float stem fed with the loader's tensors"""
    use(engine, sets, 'seed0')
    img = synth.synth_images_u8(3, 48, 80, seed=33)
    flip = torch.tensor([True, False, True])
    fm_a, _ = engine.encoder_forward(O.preprocess_u8(img, flip).cuda(), want_f=False)
    fm_b, f_b = engine.encoder_forward_u8(img.cuda(), flip.cuda(), want_f=False)
    torch.cuda.synchronize()
    assert f_b is None and tuple(fm_b.shape) == (3, 512, 3, 5) and torch.isfinite(fm_b).all()
    assert torch.equal(fm_a, fm_b)
    with pytest.raises(RuntimeError, match='25088x512'):
        engine.encoder_forward_u8(img.cuda(), flip.cuda())


def test_u8_featmap_is_bit_identical_over_64_cells(engine, sets):
    """the uint8 entry at 128x144, a featmap of 72 cells: the same transpose behind ffr_encoder_forward_u8"""
    use(engine, sets, 'seed0')
    img = synth.synth_images_u8(2, 128, 144, seed=35)
    flip = torch.tensor([False, True])
    fm_a, _ = engine.encoder_forward(O.preprocess_u8(img, flip).cuda(), want_f=False)
    fm_b, f_b = engine.encoder_forward_u8(img.cuda(), flip.cuda(), want_f=False)
    torch.cuda.synchronize()
    assert f_b is None and tuple(fm_b.shape) == (2, 512, 8, 9) and torch.isfinite(fm_b).all()
    assert torch.equal(fm_a, fm_b)


GUARD = 4096                 # floats on either side of the featmap
SENTINEL = -12345.678


@pytest.mark.parametrize('shape', ((2, 128, 144), (3, 48, 80)), ids=['2x128x144', '3x48x80'])
def test_featmap_is_written_whole_and_nowhere_else(engine, sets, shape):
    """ffr_encoder_forward through the C ABI with featmap pointing into a larger tensor: NaN where the featmap goes, a sentinel in
    4096 floats before and after.  Every element of the featmap is written (no NaN is left, and it equals the binding's featmap
    bit for bit) and both guard bands keep their bits: a transpose that walks chunks of 64 cells must stop at P in the last one."""
    use(engine, sets, 'seed0')
    N, H, W = shape
    n = N * 512 * T.cells(H, W)
    x = synth.synth_images(N, H, W, seed=34).cuda()
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, device='cuda')
    buf[GUARD:GUARD + n] = float('nan')
    guard = torch.full((GUARD,), SENTINEL).view(torch.int32)
    with torch.cuda.device(engine.device):
        rc = engine.lib.ffr_encoder_forward(engine._h, native._ptr(x), N, H, W, C.c_void_p(buf.data_ptr() + 4 * GUARD),
                                            C.c_void_p(0), engine._stream())
    assert rc == 0, engine.lib.ffr_last_error(engine._h)
    torch.cuda.synchronize()
    inside = buf[GUARD:GUARD + n]
    assert not torch.isnan(inside).any() and torch.isfinite(inside).all()
    assert torch.equal(buf[:GUARD].view(torch.int32).cpu(), guard) and torch.equal(buf[GUARD + n:].view(torch.int32).cpu(), guard)
    fm, _ = engine.encoder_forward(x, want_f=False)
    assert torch.equal(inside.view(N, 512, H // 16, W // 16), fm)
