"""Test infrastructure of the block-by-block encoder tests (tests/test_gpu_trunk_blocks.py): the encoder trunk in pieces --
stem, one bottleneck, Backbone.bn -- as plain calls into oracle/ffr_oracle.py, evaluated in the dtype of their inputs (float64
is the reference, float32 the yardstick for what fp32 costs), the error measure, and the table of cases.
tests/test_host_trunk_blocks.py pins the pieces to O.encoder_trunk and checks the table's geometry.

A case runs the trunk of one weight set on N images of H x W under `opts` and holds bottleneck `i` (and `i + 1` when count is
2) to float64.  `want` names the glue launches the plan record must show for block `i`, as literals:
    se       None (mode 'ir': no SE entry) | ('se-pool', S slices) | ('se-tiles', S tiles per image)
    combine  (path, stride, conv_shortcut, tiles per image)
    chained  True when 'wino-out-in' must have run between conv1 and conv2, with its tiles per image in `chained_tiles`
The shapes are the smallest that reach each branch on 256 CUs; the record on the device decides.  If a shape lands in another
branch there, the shape is what changes, never the assertion."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import ffr_oracle as O  # noqa: E402

FAMILIES = ('seed0', 'trained', 'ir')      # seed-0 synthetic, golden G11's 'trained' family, the 50_ir key set (no SEModule)


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def stem(sd, x):
    """input_layer: Conv3x3(3 -> 64) + BatchNorm + PReLU (pretrain/model_ir_se50.py:118-120), NCHW"""
    x = F.conv2d(x, sd['input_layer.0.weight'], None, 1, 1)
    return F.prelu(O._bn(x, sd, 'input_layer.1'), sd['input_layer.2.weight'])


def block(sd, i, x):
    """bottleneck i on its own: x NCHW, the output of bottleneck i - 1 (of the stem for i = 0)"""
    cin, depth, stride = O.ir_blocks(O.backbone_config(sd)[0])[i]
    return O.bottleneck_ir_se(x, sd, 'body.%d' % i, cin, depth, stride)


def head_bn(sd, x):
    """Backbone.bn on the output of the last bottleneck (pretrain/model_ir_se50.py:139)"""
    return O._bn(x, sd, 'bn')


def err(a, ref):
    """max-abs error over the reference's abs-max (0 over 0 counts as 0; a NaN counts as inf)"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    d = (a - ref).abs().max().item()
    if d != d:
        return float('inf')
    return 0.0 if d == 0.0 else d / max(ref.abs().max().item(), 1e-300)


def weight_sets(specs, golden_dir):
    """{family: encoder state_dict}"""
    import json
    from ffrnet_amd import synth
    with open(os.path.join(golden_dir, 'g10_backbone_variant_keys.json')) as f:
        ir = json.load(f)['50_ir']
    return {'seed0': synth.synth_state_dict(specs['encoder'], seed=0),
            'trained': synth.stress_state_dicts('trained', specs['encoder'], specs['recnet'], golden_dir)[0],
            'ir': synth.synth_state_dict(ir, seed=0)}


def stage_maps(H, W):
    """the maps of stages 1..4 of an H x W input"""
    return [(H >> s, W >> s) for s in (1, 2, 3, 4)]


def legal_hw(H, W):
    """check_hw of csrc/engine.cpp"""
    return H >= 32 and W >= 32 and H % 16 == 0 and W % 16 == 0


def _case(branch, family, N, H, W, opts, i, count, se, combine, chained=False, chained_tiles=0, images=None):
    return dict(branch=branch, family=family, N=N, H=H, W=W, opts=dict(opts), i=i, count=count,
                want=dict(se=se, combine=combine, chained=chained, chained_tiles=chained_tiles), images=images,
                id='%s-%s-%dx%dx%d-b%d%s%s' % (branch, family, N, H, W, i, '+1' if count == 2 else '',
                                                ''.join('-%s%d' % kv for kv in sorted(opts.items()))))


POOL, TILES = 'se-pool', 'se-tiles'
PLAIN, IN_C, IN_MIXED = 'combine', 'combine-in-c', 'combine-in-mixed'
MIXED_IMAGES = (0, 1, 127, 128, 255, 256)       # the images of the 257-image case that are held to float64


def _cases():
    c = []
    # ---- plain combine, every shortcut kind: default options, the block under test is the last of its run ------------------------
    # 48x80: maps 24x40, 12x20, 6x10, 3x5;  96x32: maps 48x16, 24x8, 12x4, 6x2.  Stride-1 blocks squeeze from tile sums
    # (60, 15, 6, 2 and 48, 12, 3, 2 tiles), stride-2 blocks pool on their own (HW / 16 slices, at most 32)
    c += [_case('plain', 'seed0', 3, 48, 80, {}, 0, 1, (POOL, 32), (PLAIN, 2, 0, 60)),
          _case('plain', 'seed0', 3, 48, 80, {}, 1, 1, (TILES, 60), (PLAIN, 1, 0, 60)),
          _case('plain', 'seed0', 3, 48, 80, {}, 3, 1, (POOL, 15), (PLAIN, 2, 1, 15)),
          _case('plain', 'seed0', 3, 48, 80, {}, 4, 1, (TILES, 15), (PLAIN, 1, 0, 15)),
          _case('plain', 'seed0', 3, 48, 80, {}, 7, 1, (POOL, 3), (PLAIN, 2, 1, 6)),
          _case('plain', 'seed0', 3, 48, 80, {}, 8, 1, (TILES, 6), (PLAIN, 1, 0, 6)),
          _case('plain', 'seed0', 3, 48, 80, {}, 21, 1, (POOL, 1), (PLAIN, 2, 1, 2)),
          _case('plain', 'seed0', 3, 48, 80, {}, 22, 1, (TILES, 2), (PLAIN, 1, 0, 2)),
          _case('plain', 'seed0', 3, 96, 32, {}, 0, 1, (POOL, 32), (PLAIN, 2, 0, 48)),
          _case('plain', 'seed0', 3, 96, 32, {}, 1, 1, (TILES, 48), (PLAIN, 1, 0, 48)),
          _case('plain', 'seed0', 3, 96, 32, {}, 3, 1, (POOL, 12), (PLAIN, 2, 1, 12)),
          _case('plain', 'seed0', 3, 96, 32, {}, 4, 1, (TILES, 12), (PLAIN, 1, 0, 12)),
          _case('plain', 'seed0', 3, 96, 32, {}, 7, 1, (POOL, 3), (PLAIN, 2, 1, 3)),
          _case('plain', 'seed0', 3, 96, 32, {}, 8, 1, (TILES, 3), (PLAIN, 1, 0, 3)),
          _case('plain', 'seed0', 3, 96, 32, {}, 21, 1, (POOL, 1), (PLAIN, 2, 1, 2)),
          _case('plain', 'seed0', 3, 96, 32, {}, 22, 1, (TILES, 2), (PLAIN, 1, 0, 2)),
          _case('plain', 'trained', 3, 48, 80, {}, 0, 1, (POOL, 32), (PLAIN, 2, 0, 60)),
          _case('plain', 'trained', 3, 48, 80, {}, 3, 1, (POOL, 15), (PLAIN, 2, 1, 15)),
          _case('plain', 'trained', 3, 48, 80, {}, 1, 1, (TILES, 60), (PLAIN, 1, 0, 60)),
          _case('plain', 'ir', 3, 48, 80, {}, 0, 1, None, (PLAIN, 2, 0, 60)),
          _case('plain', 'ir', 3, 48, 80, {}, 7, 1, None, (PLAIN, 2, 1, 6))]
    # ---- SE from its own pass ----------------------------------------------------------------------------------------------
    # 32x32: maps 16x16, 8x8, 4x4, 2x2 -> HW 256, 64, 16, 4 -> 16, 4, 1, 1 slices; block 1 at 48x80: HW 960 -> 32 slices of 30
    # rows, no multiple of 2 * rows_par = 32
    for opts in ({'se_maxtiles': 0}, {'wino': 0}):
        for N in (1, 3):
            c += [_case('se-pool', 'seed0', N, 32, 32, opts, 1, 1, (POOL, 16), (PLAIN, 1, 0, 16)),
                  _case('se-pool', 'seed0', N, 32, 32, opts, 4, 1, (POOL, 4), (PLAIN, 1, 0, 4)),
                  _case('se-pool', 'seed0', N, 32, 32, opts, 8, 1, (POOL, 1), (PLAIN, 1, 0, 1)),
                  _case('se-pool', 'seed0', N, 32, 32, opts, 22, 1, (POOL, 1), (PLAIN, 1, 0, 1))]
        c += [_case('se-pool', 'seed0', 3, 48, 80, opts, 1, 1, (POOL, 32), (PLAIN, 1, 0, 60))]
    c += [_case('se-pool', 'trained', 3, 32, 32, {'se_maxtiles': 0}, 4, 1, (POOL, 4), (PLAIN, 1, 0, 4)),
          _case('se-pool', 'trained', 3, 32, 32, {'wino': 0}, 1, 1, (POOL, 16), (PLAIN, 1, 0, 16)),
          # 36x60 map, 135 tiles x 128 channels > 16384: the own pass under default options; 32x64, 128 tiles: still tile sums
          _case('se-pool', 'seed0', 1, 144, 240, {}, 4, 1, (POOL, 32), (PLAIN, 1, 0, 135)),
          _case('se-tiles', 'seed0', 1, 128, 256, {}, 4, 1, (TILES, 128), (PLAIN, 1, 0, 128))]
    # ---- SE from tile sums: 1, 2, 6, 15, 16 tiles (k_se_fc: S < 8, S = 8 + 7, S = 16); 2, 6, 15 are in the plain cases -------------
    c += [_case('se-tiles', 'seed0', 3, 32, 32, {}, 8, 1, (TILES, 1), (PLAIN, 1, 0, 1)),
          _case('se-tiles', 'seed0', 3, 32, 32, {}, 1, 1, (TILES, 16), (PLAIN, 1, 0, 16)),
          _case('se-tiles', 'trained', 3, 48, 80, {}, 4, 1, (TILES, 15), (PLAIN, 1, 0, 15))]
    # ---- launch_combine_in_c, and its refusals beside it ---------------------------------------------------------------------
    f0 = {'wf_minblocks': 0}
    c += [  # 112x96: 7x6 in stage 4, 4 tiles -> 8 images per group; 14x12 in stage 3, 12 tiles: refused
          _case('combine-in-c', 'seed0', 3, 112, 96, f0, 22, 2, (TILES, 4), (IN_C, 1, 0, 4)),
          _case('combine-in-c', 'seed0', 9, 112, 96, f0, 22, 2, (TILES, 4), (IN_C, 1, 0, 4)),
          _case('combine-in-c-refused', 'seed0', 3, 112, 96, f0, 8, 2, (TILES, 12), (PLAIN, 1, 0, 12)),
          # 48x80: 3x5 in stage 4, 2 tiles -> 16 per group; 6x10 in stage 3, 6 tiles: refused
          _case('combine-in-c', 'seed0', 17, 48, 80, f0, 22, 2, (TILES, 2), (IN_C, 1, 0, 2)),
          _case('combine-in-c-refused', 'seed0', 17, 48, 80, f0, 8, 2, (TILES, 6), (PLAIN, 1, 0, 6)),
          # 32x32: 2x2 in stage 4, 1 tile -> 32 per group; 4x4 in stage 3, 1 tile but 32 x 16 pixels > 392: refused
          _case('combine-in-c', 'seed0', 33, 32, 32, f0, 22, 2, (TILES, 1), (IN_C, 1, 0, 1)),
          _case('combine-in-c-refused', 'seed0', 33, 32, 32, f0, 8, 2, (TILES, 1), (PLAIN, 1, 0, 1)),
          # 112x112: 14x14 in stage 3, 16 tiles -> 2 per group; 7x7 in stage 4 -> 8 per group
          _case('combine-in-c', 'seed0', 3, 112, 112, f0, 8, 2, (TILES, 16), (IN_C, 1, 0, 16)),
          _case('combine-in-c', 'seed0', 3, 112, 112, f0, 22, 2, (TILES, 4), (IN_C, 1, 0, 4)),
          _case('combine-in-c', 'trained', 9, 112, 96, f0, 22, 2, (TILES, 4), (IN_C, 1, 0, 4)),
          _case('combine-in-c', 'ir', 3, 112, 112, f0, 8, 2, None, (IN_C, 1, 0, 16))]
    f0v = {'wf_minblocks': 0, 'combine_v': 0}
    c += [_case('combine-v-off', 'seed0', 3, 112, 112, f0v, 8, 2, (TILES, 16), (PLAIN, 1, 0, 16)),
          _case('combine-v-off', 'seed0', 3, 112, 112, f0v, 22, 2, (TILES, 4), (PLAIN, 1, 0, 4)),
          _case('combine-v-off', 'seed0', 3, 112, 96, f0v, 8, 2, (TILES, 12), (PLAIN, 1, 0, 12)),
          _case('combine-v-off', 'seed0', 3, 112, 96, f0v, 22, 2, (TILES, 4), (PLAIN, 1, 0, 4))]
    # ---- launch_wino_out_in: option wino_fused = 0 ---------------------------------------------------------------------------
    u = {'wino_fused': 0}
    for N in (1, 3):
        c += [_case('wino-out-in', 'seed0', N, 32, 32, u, 1, 1, (TILES, 16), (PLAIN, 1, 0, 16), True, 16),   # 16x16x64: 64 KiB of LDS
              _case('wino-out-in', 'seed0', N, 32, 32, u, 8, 1, (TILES, 1), (PLAIN, 1, 0, 1), True, 1),      # 4x4x256: 256-channel blocks
              _case('wino-out-in', 'seed0', N, 48, 80, u, 4, 1, (TILES, 15), (PLAIN, 1, 0, 15), True, 15),   # 12x20: 15 ragged tiles
              _case('wino-out-in', 'seed0', N, 48, 80, u, 22, 1, (TILES, 2), (PLAIN, 1, 0, 2), True, 2),     # 3x5
              _case('wino-out-in-refused', 'seed0', N, 32, 32, u, 4, 1, (TILES, 4), (PLAIN, 1, 0, 4))]       # 8x8x128: 128 % 256
    c += [_case('wino-out-in', 'trained', 3, 32, 32, u, 1, 1, (TILES, 16), (PLAIN, 1, 0, 16), True, 16),
          _case('wino-out-in', 'trained', 3, 48, 80, u, 22, 1, (TILES, 2), (PLAIN, 1, 0, 2), True, 2)]
    # ---- launch_combine_in_mixed: 257 images of 112x112, two blocks per CU; the last combine block holds one image ---------------
    c += [_case('combine-in-mixed', 'seed0', 257, 112, 112, {}, 8, 2, (TILES, 16), (IN_MIXED, 1, 0, 16), images=MIXED_IMAGES),
          _case('combine-in-mixed', 'trained', 257, 112, 112, {}, 8, 2, (TILES, 16), (IN_MIXED, 1, 0, 16), images=MIXED_IMAGES)]
    order = {'ir': 0, 'trained': 1, 'seed0': 2}
    return sorted(c, key=lambda k: order[k['family']])          # one load of each weight set; seed0 stays for the stem and head tests


CASES = _cases()
STEM_SHAPES = ((1, 32, 32), (1, 48, 48), (3, 48, 80))           # 48x48: 2304 pixels, a ragged last block of 512
# the NCHW featmap leaves through a transpose that walks the map in chunks of 64 cells: 15 and 4 cells, 64 (one full chunk),
# 72 (a full chunk and 8), 66 on a non-square 6x11 map, 196 (three full chunks and 4)
HEAD_SHAPES = ((3, 48, 80), (3, 32, 32), (2, 128, 128), (2, 128, 144), (2, 96, 176), (1, 224, 224))


def cells(H, W):
    """positions of the featmap [N,512,H/16,W/16]"""
    return (H // 16) * (W // 16)
