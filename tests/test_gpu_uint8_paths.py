"""Decoded uint8 images through every caller: the verification harness (Engine.embed and the Backbone + RecNet shells),
the encoder shell and Engine.encoder_forward_u8, and the training iteration (ffr_train_iteration_u8 /
NativeTrainer.step).  Each path must be bit-identical to the float path fed with the tensors the reference's loader
builds (O.preprocess_u8: BGR swap, per-pair flip, ToTensor, Normalize(0.5, 0.5))."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import ffrnet_amd
from ffrnet_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))
import ffr_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

IMG_U8 = 112 * 112 * 3


@pytest.fixture(scope='module')
def engine(state_dicts):
    sd_e, sd_r = state_dicts
    eng = ffrnet_amd.Engine(0)
    eng.load_encoder(sd_e)
    eng.load_recnet(sd_r)
    return eng


@pytest.fixture(scope='module')
def loaders():
    """Two pair batches of 300 and a ragged one of 37 on the host, as uint8 (+ flip) and as the float tensors the
    reference's loader would yield for the same images and flips."""
    i1, i2, lab, flip = synth.synth_pairs_u8(637, seed=19, block=100)
    assert 0 < int(flip.sum()) < 637
    u8, fp = [], []
    for s in (0, 300, 600):
        e = min(s + 300, 637)
        u8.append(dict(img1=i1[s:e], img2=i2[s:e], label=lab[s:e], idx=torch.arange(s, e), flip=flip[s:e]))
        fp.append(dict(img1=O.preprocess_u8(i1[s:e], flip[s:e]), img2=O.preprocess_u8(i2[s:e], flip[s:e]),
                       label=lab[s:e], idx=torch.arange(s, e)))
    return u8, fp


def _harness(embed, loader, recnet=None):
    pn, p = ffrnet_amd.lfw.calculate_distance(loader, embed, recnet)
    h2d = ffrnet_amd.lfw.last_feed_stats['h2d_bytes']
    acc_new, acc, det = ffrnet_amd.lfw.get_avg_accuracy(embed, recnet, loader, details=True) if recnet is not None \
        else ffrnet_amd.lfw.get_avg_accuracy(embed, loader, details=True)
    return pn, p, h2d, acc_new, acc, np.array(det['folds_new']), np.array(det['folds'])


def _same_harness(a, b):
    for x, y in zip(a[:2] + a[3:], b[:2] + b[3:]):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_harness_uint8_loader_with_engine_embed(engine, loaders):
    u8, fp = loaders
    ref = _harness(engine.embed, fp)
    got = _harness(engine.embed, u8)
    _same_harness(got, ref)
    assert ref[2] == 2 * 637 * IMG_U8 * 4
    assert got[2] == ref[2] // 4 + 637          # uint8 images plus one flip byte per pair


def test_harness_uint8_loader_through_shells(state_dicts, loaders):
    sd_e, sd_r = state_dicts
    enc = ffrnet_amd.Backbone(num_layers=50, drop_ratio=0.6, mode='ir_se')
    rec = ffrnet_amd.RecNet(norm_type='bn', relu_type='prelu')
    enc.load_state_dict(sd_e)
    rec.load_state_dict(sd_r)
    enc.cuda().eval()
    rec.cuda().eval()
    u8, fp = loaders
    with torch.no_grad():
        ref = _harness(enc, fp, rec)
        got = _harness(enc, u8, rec)
    _same_harness(got, ref)
    assert got[2] == ref[2] // 4 + 637


def test_graphed_embed_refuses_uint8(engine, loaders):
    g = ffrnet_amd.GraphedEmbed(engine, 4)
    with pytest.raises(RuntimeError, match='GraphedEmbed'):
        ffrnet_amd.lfw.calculate_distance(loaders[0], g)
    with pytest.raises(RuntimeError, match='GraphedEmbed'):
        g(torch.zeros(4, 112, 112, 3, dtype=torch.uint8, device='cuda'))


def test_backbone_shell_and_encoder_uint8(state_dicts):
    sd_e, _ = state_dicts
    enc = ffrnet_amd.Backbone(num_layers=50, drop_ratio=0.6, mode='ir_se')
    enc.load_state_dict(sd_e)
    enc.cuda().eval()
    img = synth.synth_images_u8(256, seed=41)
    flip = synth.synth_pairs_u8(256, 16, 16, seed=41)[3]
    with torch.no_grad():
        fm_a, f_a = enc(O.preprocess_u8(img, flip).cuda())
        fm_b, f_b = enc(img.cuda(), flip.cuda())
    assert tuple(fm_b.shape) == (256, 512, 7, 7) and tuple(f_b.shape) == (256, 512)
    assert torch.equal(fm_a, fm_b) and torch.equal(f_a, f_b)
    # 112x96: the trunk only
    eng = enc._engine(torch.device('cuda', 0))
    img = synth.synth_images_u8(32, 112, 96, seed=42)
    flip = torch.arange(32) % 3 == 0
    fm_a, _ = eng.encoder_forward(O.preprocess_u8(img, flip).cuda(), want_f=False)
    fm_b, f_b = eng.encoder_forward_u8(img.cuda(), flip.cuda(), want_f=False)
    assert f_b is None and tuple(fm_b.shape) == (32, 512, 7, 6)
    assert torch.equal(fm_a, fm_b)
    with pytest.raises(RuntimeError, match='25088x512'):
        enc(img.cuda())
    with pytest.raises(RuntimeError, match='uint8 images only'):
        enc(O.preprocess_u8(img).cuda(), flip.cuda())


@pytest.mark.parametrize('n', [8, 128])
def test_training_iteration_uint8_is_bit_identical(specs, n):
    sd_e = synth.synth_state_dict(specs['encoder'], seed=0)
    sd_r = synth.synth_state_dict(specs['recnet'], seed=0)
    non, ocl, label, flip = synth.synth_train_batch_u8(n, seed=91)
    assert 0 < int(flip.sum()) < n
    non_f, ocl_f = O.preprocess_u8(non, flip).cuda(), O.preprocess_u8(ocl, flip).cuda()
    non, ocl, flip, label = non.cuda(), ocl.cuda(), flip.cuda(), label.cuda()
    eng = ffrnet_amd.Engine(0)
    eng.load_encoder(sd_e)
    try:
        for mode in (1, 0):
            res = []
            for u8 in (False, True):
                tr = ffrnet_amd.NativeTrainer(eng, sd_r, lr=1e-3)
                eng.train_option('winograd', mode)
                items = tr.step(non, ocl, label, flip) if u8 else tr.step(non_f, ocl_f, label)
                res.append((torch.stack(items + [tr.accuracy]).cpu(), tr.flat_grads.clone(), tr.flat_params.clone()))
            (ia, ga, pa), (ib, gb, pb) = res
            assert torch.isfinite(ia).all()
            assert torch.equal(ia, ib), (mode, ia, ib)
            assert torch.equal(ga, gb), mode
            assert torch.equal(pa, pb), mode
            # the raw entry point: out5 and the gradients of one iteration, no optimiser step
            out_a = eng.train_iteration(non_f, ocl_f, label)
            g_a = tr.flat_grads.clone()
            out_b = eng.train_iteration_u8(non, ocl, label, flip)
            assert torch.equal(out_a, out_b) and torch.equal(g_a, tr.flat_grads)
    finally:
        eng.train_option('winograd', 1)


def test_uint8_refusals(specs, engine):
    dev = engine.device
    img = torch.zeros(4, 112, 112, 3, dtype=torch.uint8, device=dev)
    for bad in (torch.zeros(4, 3, 112, 112, dtype=torch.uint8, device=dev),
                torch.zeros(4, 112, 112, 4, dtype=torch.uint8, device=dev),
                torch.zeros(4, 112, 100, 3, dtype=torch.uint8, device=dev)):
        with pytest.raises(RuntimeError):
            engine.encoder_forward_u8(bad, want_f=False)
    with pytest.raises(RuntimeError, match='uint8'):
        engine.encoder_forward_u8(img.float())
    with pytest.raises(RuntimeError, match='ROCm device'):
        engine.encoder_forward_u8(img.cpu())
    with pytest.raises(RuntimeError, match='4 flags'):
        engine.encoder_forward_u8(img, torch.zeros(3, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match='bool or uint8'):
        engine.encoder_forward_u8(img, torch.zeros(4, dtype=torch.int64, device=dev))
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match='Engine lives on'):
            engine.encoder_forward_u8(img.to('cuda:1'))
        with pytest.raises(RuntimeError, match='Engine lives on'):
            engine.encoder_forward_u8(img, torch.zeros(4, dtype=torch.uint8, device='cuda:1'))
    # a pair batch of mixed dtypes
    loader = [dict(img1=img.cpu(), img2=img.cpu().float(), label=torch.zeros(4), idx=torch.arange(4))]
    with pytest.raises(RuntimeError, match='one image type'):
        ffrnet_amd.lfw.calculate_distance(loader, engine.embed)
    # NULL pointers through the C ABI
    lib = engine.lib
    fm = torch.empty(4, 512, 7, 7, device=dev)
    p = ctypes.c_void_p
    assert lib.ffr_encoder_forward_u8(engine._h, None, None, 4, 112, 112, p(fm.data_ptr()), None, None) == -1
    assert lib.ffr_encoder_forward_u8(engine._h, p(img.data_ptr()), None, 4, 112, 100, p(fm.data_ptr()), None, None) == -1
    assert lib.ffr_encoder_forward_u8(engine._h, p(img.data_ptr()), None, 0, 112, 112, p(fm.data_ptr()), None, None) == -1
    # training: mixed dtypes, flip length, shapes, NULL pointers
    eng = ffrnet_amd.Engine(0)
    eng.load_encoder(synth.synth_state_dict(specs['encoder'], seed=0))
    tr = ffrnet_amd.NativeTrainer(eng, synth.synth_state_dict(specs['recnet'], seed=0), lr=1e-3)
    label = torch.zeros(4, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match='uint8'):
        tr.step(img, img.permute(0, 3, 1, 2).float().contiguous(), label)
    with pytest.raises(RuntimeError, match='4 flags'):
        tr.step(img, img, label, torch.zeros(8, dtype=torch.bool, device=dev))
    with pytest.raises(RuntimeError, match='uint8 images only'):
        tr.step(img.permute(0, 3, 1, 2).float().contiguous(), img.permute(0, 3, 1, 2).float().contiguous(), label,
                torch.zeros(4, dtype=torch.bool, device=dev))
    with pytest.raises(RuntimeError, match='pairs'):
        eng.train_iteration_u8(img, img[:3], label)
    with pytest.raises(RuntimeError):
        eng.train_iteration_u8(img.cpu(), img.cpu(), label)
    lab32 = label.to(torch.int32)
    lw = (ctypes.c_double * 4)(1, 1, 1, 1)
    out = torch.empty(5, device=dev)
    for a, b, lab in ((None, img, lab32), (img, None, lab32), (img, img, None)):
        ptr = [p(t.data_ptr()) if t is not None else None for t in (a, b, lab)]
        assert eng.lib.ffr_train_iteration_u8(eng._h, ptr[0], ptr[1], None, ptr[2], 4, lw, p(out.data_ptr()), None) == -1
    torch.cuda.synchronize()
