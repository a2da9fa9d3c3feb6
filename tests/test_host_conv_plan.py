"""The convolution planners of csrc/plan.cpp on the host, through ffr_plan_igemm_host / ffr_plan_conv_host: no device needed.

plan_igemm is swept over every row count the operator hooks and the product's small launches can reach; plan_conv over the
product's layer table at every batch 1..600 on 256 CUs.  The properties are those the launchers rely on: a launch never has
more blocks than are resident, a cut tile always has its slabs, no launch outgrows the scratch of the workspace, and the tail
split hands whole images to both parts."""
import ctypes
import time

import numpy as np
import pytest

from ffrnet_amd import native

# ffr_kernels.h: IGEMM_TILES and the static_assert on igemm_resident_blocks (fp32 form, split-operand form)
TILE_BM = np.array([0, 128, 128, 64, 256])
TILE_BN = np.array([0, 128, 64, 64, 64])
RESIDENT = {False: np.array([0, 2, 3, 4, 1]), True: np.array([0, 1, 2, 3, 1])}
PARTIAL_CAP = 1024 * 2 * 128 * 128 // 2 + 4096          # forward.cpp, layout(): floats
TICKETS_CAP_8 = 8 * 112 * 112 // 64 + 4096              # forward.cpp, ensure_arena() for 8 images of 112x112
MIN_UNITS = 18                                          # option sk_minunits
M_MAX = 70000
COUT_PADS = (64, 128, 192, 256, 512)
NKTS = (1, 2, 4, 8, 9, 16, 18, 27, 36, 72, 784)


@pytest.fixture(scope='module')
def lib():
    return native.load_library()


def plan_igemm(lib, M0, count, cout_pad, nkt, nbatch, force, split):
    tile, nblocks, granule = (np.zeros(count, dtype=np.int32) for _ in range(3))
    rc = lib.ffr_plan_igemm_host(M0, cout_pad, nkt, nbatch, force, MIN_UNITS, int(split), count, tile.ctypes.data, nblocks.ctypes.data,
                                 granule.ctypes.data)
    assert rc == 0
    return tile.astype(np.int64), nblocks.astype(np.int64), granule.astype(np.int64)


def test_plan_igemm_sweep(lib):
    t0 = time.time()
    M = np.arange(1, M_MAX + 1, dtype=np.int64)
    sample = np.unique(np.concatenate([np.arange(0, 48), np.arange(48, M_MAX, 1009), [M_MAX - 1]]))     # indices of the rows whose block ranges are walked
    bad = []
    configs = 0
    over_tickets = {}
    for cout_pad in COUT_PADS:
        for nkt in NKTS:
            for nbatch in (1, 36):
                for force in range(5):
                    if force and cout_pad % TILE_BN[force]:
                        continue
                    for split in (False, True):
                        configs += 1
                        key = (cout_pad, nkt, nbatch, force, split)
                        tile, P, granule = plan_igemm(lib, 1, M_MAX, cout_pad, nkt, nbatch, force, split)
                        assert ((tile >= 1) & (tile <= 4)).all() and (force == 0 or (tile == force).all()), key
                        bm, bn = TILE_BM[tile], TILE_BN[tile]
                        assert (cout_pad % bn == 0).all(), key
                        pmax = 256 * RESIDENT[split][tile]
                        if not ((P >= 1) & (P <= pmax)).all():
                            bad.append((key, 'nblocks outside 1..256 * resident blocks', int(M[(P < 1) | (P > pmax)][0])))
                        if not ((granule == 1) | (granule == nkt)).all():
                            bad.append((key, 'granule is neither 1 nor nkt', int(M[(granule != 1) & (granule != nkt)][0])))
                        tiles = (M + bm - 1) // bm * (cout_pad // bn) * nbatch
                        units = tiles * nkt
                        cut = (granule == 1) & ((units % P != 0) | ((units // P) % nkt != 0))          # run_gemm's expression
                        if (cut & (granule == nkt) & (nkt > 1)).any():
                            bad.append((key, 'granule == nkt and a tile counted as cut', 0))
                        over = cut & (P * 2 * bm * bn > PARTIAL_CAP)
                        if over.any():
                            bad.append((key, 'cut tiles without room for their slabs', int(M[over][0])))
                        over = tiles > TICKETS_CAP_8
                        if over.any():
                            over_tickets[key] = int(M[over][0])
                        # the block ranges k_igemm derives (igemm.hip: block b owns units [b * G / P, (b + 1) * G / P) * granule,
                        # G = units / granule): with granule == nkt no boundary falls inside a tile, and a boundary inside a
                        # tile is always announced as `cut`, so the slabs and the tickets are there
                        for i in sample:
                            G = int(units[i] // granule[i])
                            b = np.arange(1, int(P[i]), dtype=np.int64)
                            inside = ((b * G // int(P[i]) * int(granule[i])) % nkt != 0).any()
                            if inside and not cut[i]:
                                bad.append((key, 'a block boundary inside a tile that is not announced as cut', int(M[i])))
                                break
    dt = time.time() - t0
    print('plan_igemm sweep: %d configurations x %d row counts in %.1f s; %d flagged' % (configs, M_MAX, dt, len(bad)))
    assert not bad, bad[:10]
    # tiles <= the ticket array of an 8-image arena: holds wherever the planner picks the tile of a single GEMM (what the
    # operator hooks launch at N <= 8).  It cannot hold for a forced small tile or for 36 batched GEMMs at these row counts:
    # the tile count is the problem's, not the planner's.  run_gemm refuses such a launch (FFR_ERR_NOMEM), and the batched
    # launches of the product size their ticket array by their own batch (ensure_arena).
    print('ticket array of an 8-image arena exceeded (first M) in: %s' % sorted(over_tickets.items())[:8])
    assert not [k for k in over_tickets if k[2] == 1 and k[3] == 0], over_tickets


# ---- the product's layer table at 112x112 (pack.cpp: REC_LAYERS, block_table(24); forward.cpp: run_trunk, run_recnet) ----------
def product_layers():
    """(name, cin, cout, R, stride, pad, pad_mode, H, in_pitch, out_pitch, out_coff, res_pitch, tile_sums)"""
    rows = []
    stage_ch = ((64, 64), (64, 128), (128, 256), (256, 512))
    units = (3, 4, 14, 3)
    H = 112
    for s in range(4):
        for u in range(units[s]):
            cin = stage_ch[s][0] if u == 0 else stage_ch[s][1]
            depth = stage_ch[s][1]
            stride = 2 if u == 0 else 1
            name = 'body.%d.%d' % (s, u)
            rows.append((name + '.conv1', cin, depth, 3, 1, 1, 0, H, cin, depth, 0, depth))
            rows.append((name + '.conv2', depth, depth, 3, stride, 1, 0, H, depth, depth, 0, depth))
            if cin != depth:
                rows.append((name + '.shortcut', cin, depth, 1, stride, 0, 0, H, cin, depth, 0, depth))
            H //= stride
    rec = (('Conv4Space.0', 561, 256, 576, 256, 0), ('Conv4Space.1.conv1', 256, 256, 256, 256, 0), ('Conv4Space.1.conv2', 256, 256, 256, 256, 0),
           ('Conv4Space.2', 256, 128, 256, 128, 0), ('Conv4Space.3.conv1', 128, 128, 128, 128, 0), ('Conv4Space.3.conv2', 128, 128, 128, 128, 0),
           ('Conv4Space.4', 128, 49, 128, 64, 0), ('Conv4Space.5.conv1', 49, 49, 64, 64, 0), ('Conv4Space.5.conv2', 49, 49, 64, 64, 0),
           ('ChannelFlipMerge.0', 1024, 512, 1024, 512, 0), ('ChannelFlipMerge.1.conv1', 512, 512, 512, 512, 0),
           ('ChannelFlipMerge.1.conv2', 512, 512, 512, 1536, 512), ('Conv4Merge.0', 1536, 512, 1536, 512, 0),
           ('Conv4Merge.1.conv1', 512, 512, 512, 512, 0), ('Conv4Merge.1.conv2', 512, 512, 512, 512, 0))
    for name, cin, cout, in_pitch, out_pitch, out_coff in rec:
        rows.append((name, cin, cout, 3, 1, 1, 1, 7, in_pitch, out_pitch, out_coff, (cout + 63) // 64 * 64))
    return rows


def plan_conv(lib, row, N, num_cus=256, force=-1, mixed=False):
    name, cin, cout, R, stride, pad, pad_mode, H, in_pitch, out_pitch, out_coff, res_pitch = row
    cin_pad = (cin + 31) // 32 * 32
    wino = R == 3 and stride == 1 and cin_pad >= 64                # pack_conv: option wino_mincin
    out = (ctypes.c_longlong * 24)()
    rc = lib.ffr_plan_conv_host(cin, cout, R, stride, pad, pad_mode, int(wino), int(wino and cin_pad <= 128), int(not wino), int(mixed),
                                N, H, H, in_pitch, out_pitch, out_coff, (cout + 63) // 64 * 64, res_pitch, num_cus, force, out)
    assert rc == 0
    keys = ('path', 'half_n', 'phased', 'split', 'n_main', 'side', 'takes_v', 'refused', 'tiles_img')
    p = dict(zip(keys, out[:9]))
    sub = ('kind', 'fits', 'tile', 'nblocks', 'granule', 'cut')
    p['main'] = dict(zip(sub, out[9:15]))
    p['rem'] = dict(zip(sub, out[15:21]))
    return p


def test_product_layer_table_plans(lib):
    t0 = time.time()
    rows = product_layers()
    assert len(rows) == 15 + 24 * 2 + 3
    bad = []
    seen = set()
    for row in rows:
        name, cin, cout = row[0], row[1], row[2]
        cout_pad = (cout + 63) // 64 * 64
        for mixed in ((False, True) if row[7] == 14 and row[3] == 3 and row[4] == 1 else (False,)):
            for N in range(1, 601):
                p = plan_conv(lib, row, N, mixed=mixed)
                if p['refused']:
                    bad.append((name, N, 'refused'))
                    continue
                if not p['main']['fits'] or p['main']['kind'] == 0:
                    bad.append((name, N, 'the launch does not fit its scratch', p['main']))
                if not 0 <= p['n_main'] < N:
                    bad.append((name, N, 'n_main out of range', p['n_main']))
                seen.add((p['path'], p['half_n'], p['phased'], p['split'], p['n_main'] > 0, p['side']))
                if p['n_main']:
                    # the main part is k_wino_fused on the first n_main images, the remainder the transform kernels + GEMM, and
                    # both fit; the main part's block tiles are whole rounds of the chip and one more image would not fit into
                    # them: the images [0, n_main) are exactly the ones whose 32-tile groups lie inside the whole rounds
                    nbn = cout_pad // (32 if p['half_n'] else 64)
                    full = (N * p['tiles_img'] + 31) // 32 * nbn // 256 * 256
                    groups = full // nbn
                    ok = p['path'] == 2 and p['main']['kind'] == 2 and p['rem']['kind'] == 3 and p['rem']['fits']
                    ok = ok and p['n_main'] * p['tiles_img'] <= groups * 32 < (p['n_main'] + 1) * p['tiles_img']
                    ok = ok and p['side'] == p['phased']
                    if not ok:
                        bad.append((name, N, 'tail split', p))
                else:
                    if p['rem']['kind'] != 0:
                        bad.append((name, N, 'a remainder without a split', p))
    dt = time.time() - t0
    print('plan_conv table: %d layers x 600 batches in %.1f s; %d flagged; forms seen %s' % (len(rows), dt, len(bad), sorted(seen)))
    assert not bad, bad[:10]
    # the branches the GPU branch tests name all occur in the product's table
    paths = {s[0] for s in seen}
    assert paths == {0, 1, 2, 3}
    assert any(s[0] == 2 and s[1] for s in seen) and any(s[0] == 2 and s[3] for s in seen)
    assert any(s[4] and s[5] for s in seen) and any(s[4] and not s[5] for s in seen)


def test_host_planner_entries_reject_bad_arguments(lib):
    z = np.zeros(1, dtype=np.int32)
    assert lib.ffr_plan_igemm_host(0, 64, 1, 1, 0, 18, 0, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data) != 0
    assert lib.ffr_plan_igemm_host(1, 64, 1, 1, 1, 18, 0, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data) != 0       # 128-wide tile, cout_pad 64
    assert lib.ffr_plan_igemm_host(1, 64, 1, 1, 0, 18, 0, 1, None, z.ctypes.data, z.ctypes.data) != 0
    out = (ctypes.c_longlong * 24)()
    assert lib.ffr_plan_conv_host(64, 64, 3, 1, 1, 0, 1, 1, 0, 0, 0, 14, 14, 64, 64, 0, 64, 64, 256, -1, out) != 0    # N = 0
    assert lib.ffr_plan_conv_host(64, 64, 3, 1, 1, 0, 1, 1, 0, 0, 4, 14, 14, 64, 64, 0, 64, 64, 256, 6, out) != 0     # force 6
