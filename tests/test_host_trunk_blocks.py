"""Host side of the block-by-block encoder tests (tests/test_gpu_trunk_blocks.py): no device needed.

1. Chaining trunk_ref.stem and trunk_ref.block over the bottlenecks reproduces every tap of O.encoder_trunk bit for bit in fp32,
   at a small non-square size, for the IR-SE50 key set and for the 50_ir key set of golden G10 (no SEModule); head_bn is the
   featmap of O.encoder_forward's arithmetic.
2. Every case of the table is one the library accepts (check_hw: multiples of 16, at least 32), has integer stage maps, names a
   block and a count inside the network, and states the tile and slice counts that follow from its geometry.  The head shapes hold a
   featmap of exactly 64 cells (one chunk of the NCHW transpose) and maps above 64."""
import pytest
import torch

from ffrnet_amd import synth

import trunk_ref as T

O = T.O


@pytest.fixture(scope='module')
def sets(specs, golden_dir):
    return T.weight_sets(specs, golden_dir)


@pytest.mark.parametrize('family', ['seed0', 'ir'])
def test_pieces_chain_to_the_oracle_trunk(sets, family):
    sd = sets[family]
    assert O.backbone_config(sd) == (50, family != 'ir')
    x = synth.synth_images(2, 32, 48, seed=77)
    with torch.no_grad():
        taps = {}
        end = O.encoder_trunk(sd, x, None, taps)
        t = T.stem(sd, x)
        assert torch.equal(t, taps['input_layer'])
        for i in range(24):
            t = T.block(sd, i, t)
            assert torch.equal(t, taps['body.%d' % i]), i
        assert torch.equal(t, end) and tuple(t.shape) == (2, 512, 2, 3)
        assert torch.equal(T.head_bn(sd, t), O._bn(end, sd, 'bn'))
        # a piece evaluates in the dtype of its inputs
        sd64 = T.cast(sd, torch.float64)
        b64 = T.block(sd64, 3, taps['body.2'].double())
        assert b64.dtype == torch.float64 and 0 < T.err(taps['body.3'], b64) < 1e-5
    assert T.err(torch.zeros(3), torch.zeros(3)) == 0.0 and T.err(torch.tensor([float('nan')]), torch.ones(1)) == float('inf')


def se_slices(N, HW):
    """csrc/elementwise.hip, se_slices"""
    return max(1, min(2048 // N, HW // 16, 32))


def test_case_table_is_legal_and_consistent():
    blocks = O.ir_blocks(50)
    ids = [c['id'] for c in T.CASES]
    assert len(set(ids)) == len(ids)
    for c in T.CASES:
        H, W, i = c['H'], c['W'], c['i']
        assert T.legal_hw(H, W), c['id']
        maps = T.stage_maps(H, W)
        assert all(h * (2 << s) == H and w * (2 << s) == W and h >= 2 and w >= 2 for s, (h, w) in enumerate(maps)), c['id']
        assert c['count'] in (1, 2) and 0 <= i and i + c['count'] <= 24 and c['family'] in T.FAMILIES, c['id']
        assert c['N'] <= 33 or c['images'] == T.MIXED_IMAGES, c['id']
        cin, depth, stride = blocks[i]
        stage = (64, 128, 256, 512).index(depth)
        ho, wo = maps[stage]
        tiles = ((ho + 3) // 4) * ((wo + 3) // 4)
        w = c['want']
        path, w_stride, conv_sc, w_tiles = w['combine']
        assert (w_stride, conv_sc, w_tiles) == (stride, int(cin != depth), tiles), c['id']
        assert (w['se'] is None) == (c['family'] == 'ir'), c['id']
        if w['se'] is not None:
            assert w['se'][1] == (tiles if w['se'][0] == T.TILES else se_slices(c['N'], ho * wo)), c['id']
            assert stride == 1 or w['se'][0] == T.POOL, c['id']
        assert not w['chained'] or (w['chained_tiles'] == tiles and stride == 1), c['id']
    # every branch the device module must reach has a case that names it
    combines = {(c['want']['combine'][0], c['want']['combine'][1], c['want']['combine'][2]) for c in T.CASES}
    assert {(T.PLAIN, 2, 0), (T.PLAIN, 2, 1), (T.PLAIN, 1, 0), (T.IN_C, 1, 0), (T.IN_MIXED, 1, 0)} <= combines
    per_group = {}
    for c in T.CASES:
        if c['want']['combine'][0] == T.IN_C:
            per_group.setdefault(32 // c['want']['combine'][3], []).append(c['N'])
    assert set(per_group) == {2, 8, 16, 32} and all(n % g for g, ns in per_group.items() for n in ns)     # a partly empty last group
    assert {c['want']['chained_tiles'] > 4 for c in T.CASES if c['want']['chained']} == {True, False}
    assert {c['want']['se'][1] for c in T.CASES if c['want']['se'] and c['want']['se'][0] == T.TILES} >= {1, 2, 6, 15, 16, 128}
    assert {c['want']['se'][1] for c in T.CASES if c['want']['se'] and c['want']['se'][0] == T.POOL} >= {1, 4, 16, 32}
    for fam in ('trained',):
        assert {c['branch'] for c in T.CASES if c['family'] == fam} >= {'plain', 'se-pool', 'se-tiles', 'combine-in-c', 'wino-out-in',
                                                                       'combine-in-mixed'}
    for N, H, W in T.STEM_SHAPES + T.HEAD_SHAPES:
        assert T.legal_hw(H, W)
    assert any(N * H * W % 512 for N, H, W in T.STEM_SHAPES)
    # the featmap transpose moves 64 cells per block: below one chunk, exactly one, a chunk and a ragged rest, several chunks
    head_cells = {T.cells(H, W) for N, H, W in T.HEAD_SHAPES}
    assert 64 in head_cells and min(head_cells) < 64 and {c for c in head_cells if c > 64} >= {66, 72, 196}
    assert any(c > 128 and c % 64 for c in head_cells) and any(H != W and T.cells(H, W) > 64 for N, H, W in T.HEAD_SHAPES)
