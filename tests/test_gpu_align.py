"""Face alignment on the device (include/ffrnet.h: ffr_align_transforms, ffr_align_warp, ffr_embed_aligned).

Transforms are held to the matrices the reference itself returned (golden G13); the warp is held bit for bit to the
integer restatement of tests/align_ref.py and to cases whose answer needs no oracle (a crop pasted into a frame comes back
exactly); embed_aligned is held bit for bit to embed_u8 of the aligned crops."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import align_ref
import ffrnet_amd
from ffrnet_amd import native, synth
from ffrnet_amd.align import TEMPLATE_96x112, TEMPLATE_112x112

pytestmark = pytest.mark.gpu

# An entry error e of A moves a sample by at most e * (112 + 112 + 1) pixels: 1e-6 keeps that under 1/100 of the 1/32-pixel
# sampling quantum, and is four orders above what the float64 closed form shows against the reference on the CPU.
TFM_TOL = 1e-6
# Embeddings are not bitwise independent of the batch they are computed in (other launch shapes, other summation
# orders): the bound of tests/test_gpu_parity.py::test_batch_independence_full_size.
BATCH_TOL = 2e-5


@pytest.fixture(scope='module')
def eng():
    return ffrnet_amd.Engine(0)


@pytest.fixture(scope='module')
def net(state_dicts):
    e = ffrnet_amd.Engine(0)
    e.load_encoder(state_dicts[0])
    e.load_recnet(state_dicts[1])
    yield e
    e.close()


def template_of(out_hw):
    return np.array(TEMPLATE_112x112 if out_hw[1] == 112 else TEMPLATE_96x112, dtype=np.float64)


def scene(F, H, W, N, out_hw, seed, padded=False):
    """F noise frames (optionally cut out of a buffer with wider rows) and N faces spread over them: the template under
    a random similarity (any rotation, scale 0.4-3, a sixth mirrored, 0.7 px point noise), centred anywhere from 30 px
    outside the frame to 30 px outside the other edge, so crops run off every edge."""
    rng = np.random.Generator(np.random.Philox(key=seed))
    Wp = W + 5 if padded else W
    buf = synth.synth_images_u8(F, H, Wp, seed=seed)
    frames = buf[:, :, :W]
    tmpl = template_of(out_hw)
    frame_index = rng.integers(0, F, N) if N != F else rng.permutation(F)
    lm = np.empty((N, 5, 2), np.float32)
    for n in range(N):
        theta = rng.uniform(-np.pi, np.pi) if n % 2 else rng.uniform(-0.3, 0.3)
        sc = rng.uniform(0.4, 3.0)
        L = sc * np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
        if n % 6 == 5:
            L = L @ np.diag([-1.0, 1.0])
        centre = np.array([rng.uniform(-30, W + 30), rng.uniform(-30, H + 30)])
        lm[n] = (tmpl - tmpl.mean(0)) @ L.T + centre + rng.uniform(-0.7, 0.7, (5, 2))
    return buf, frames, frame_index.astype(np.int32), lm, tmpl


def test_transforms_match_reference_matrices(eng, golden_dir):
    g = np.load(os.path.join(golden_dir, 'g13_align_transforms.npz'))
    lm, tmpl, mats = g['landmarks'], g['template'], g['cv2_matrix']
    A, valid = eng.align_transforms(torch.from_numpy(lm).cuda(), torch.from_numpy(tmpl))
    assert A.dtype == torch.float64 and tuple(A.shape) == (lm.shape[0], 6) and valid.dtype == torch.uint8
    A, valid = A.cpu().numpy().reshape(-1, 2, 3), valid.cpu().numpy()
    assert valid.all()
    want = np.stack([align_ref.invert_2x3(M) for M in mats])
    err = np.abs(A - want).max()
    print('max |A - inverse(reference matrix)| = %.3e over %d cases' % (err, lm.shape[0]))
    assert err <= TFM_TOL
    assert np.array_equal(np.linalg.det(A[:, :, :2]) < 0, np.linalg.det(mats[:, :, :2]) < 0)


WARP_CASES = [  # (F, H, W, N, out_hw, padded)
    (1, 250, 250, 1, (112, 112), False),
    (37, 250, 250, 37, (112, 112), False),
    (5, 250, 250, 37, (112, 96), True),
    (4, 1080, 1920, 37, (112, 112), True),
    (8, 1080, 1920, 256, (112, 96), False),
    (256, 250, 250, 256, (112, 112), True),
]


@pytest.mark.parametrize('F,H,W,N,out_hw,padded', WARP_CASES)
def test_warp_bit_exact(eng, F, H, W, N, out_hw, padded):
    buf, frames, fidx, lm, tmpl = scene(F, H, W, N, out_hw, seed=1000 + N + H + out_hw[1], padded=padded)
    dev = buf.cuda()[:, :, :W]                     # the same view on the device: rows keep the buffer's pitch
    assert (dev.stride(1) == 3 * (W + 5)) == padded
    A, valid = eng.align_transforms(torch.from_numpy(lm).cuda(), torch.from_numpy(tmpl))
    crop = eng.align_warp(dev, torch.from_numpy(fidx), A, valid, out_hw)
    assert crop.dtype == torch.uint8 and tuple(crop.shape) == (N,) + tuple(out_hw) + (3,) and crop.is_contiguous()
    assert valid.cpu().numpy().all()
    want = align_ref.warp_batch(frames.numpy(), fidx, A.cpu().numpy(), None, out_hw)
    got = crop.cpu().numpy()
    assert np.array_equal(got, want), 'faces that differ: %s' % np.nonzero((got != want).reshape(N, -1).any(1))[0][:10]
    # the scene exercises the border and the interior: some crops hold zeros from outside the frame, most pixels do not
    assert N == 1 or ((want == 0).all(3).reshape(N, -1).mean(1) > 0.05).any()
    assert (want != 0).mean() > 0.3
    # align_crops is the two calls in one; valid = None warps every face
    assert torch.equal(eng.align_crops(dev, torch.from_numpy(fidx).cuda(), torch.from_numpy(lm).cuda(), tmpl, out_hw), crop)
    assert torch.equal(eng.align_warp(dev, torch.from_numpy(fidx), A, None, out_hw), crop)


def carried(points, k, mirror):
    """where the points of a 112 x 112 image land after an optional mirror and k quarter turns (np.rot90)"""
    p = points.copy()
    if mirror:
        p[:, 0] = 111.0 - p[:, 0]
    for _ in range(k):
        p = np.stack((p[:, 1], 111.0 - p[:, 0]), 1)
    return p


def pasted_scene(n, seed, H=300, W=400):
    """n noise crops, each mirrored or not, turned by 0-3 quarter turns and pasted at an integer offset into its own
    zero frame; the landmarks are the template carried along with the image (mirrored positions, not relabelled)."""
    rng = np.random.Generator(np.random.Philox(key=seed))
    crops = synth.synth_images_u8(n, 112, 112, seed=seed).numpy()
    tmpl = np.array(TEMPLATE_112x112, dtype=np.float64)
    frames = np.zeros((n, H, W, 3), np.uint8)
    lm = np.empty((n, 5, 2), np.float32)
    kinds = []
    for i in range(n):
        k, mirror = i % 4, (i // 4) % 2 == 1
        ox, oy = int(rng.integers(0, W - 112)), int(rng.integers(0, H - 112))
        img = crops[i][:, ::-1] if mirror else crops[i]
        frames[i, oy:oy + 112, ox:ox + 112] = np.rot90(img, k)
        lm[i] = carried(tmpl, k, mirror) + [ox, oy]
        kinds.append((k, mirror))
    return crops, frames, lm, kinds


def test_exact_recoveries(eng):
    crops, frames, lm, kinds = pasted_scene(16, seed=77)
    A, valid = eng.align_transforms(torch.from_numpy(lm).cuda())
    det = np.linalg.det(A.cpu().numpy().reshape(-1, 2, 3)[:, :, :2])
    assert np.array_equal(det < 0, np.array([m for _, m in kinds]))          # the reflective branch wins where mirrored
    assert np.allclose(np.abs(det), 1.0, atol=1e-5)
    got = eng.align_crops(torch.from_numpy(frames).cuda(), torch.arange(16), torch.from_numpy(lm).cuda()).cpu().numpy()
    for i, kind in enumerate(kinds):
        assert np.array_equal(got[i], crops[i]), (i, kind)


def test_degenerate_faces(eng, net):
    _, frames, fidx, _, tmpl = scene(3, 250, 250, 8, (112, 112), seed=5)
    lm = np.tile((tmpl + [60, 70]).astype(np.float32), (8, 1, 1))             # every face well inside its frame
    lm += np.arange(8, dtype=np.float32)[:, None, None]
    clean_lm, clean_fidx = lm.copy(), fidx.copy()
    lm[1] = lm[1, 0]                       # all landmarks equal
    lm[3, 2, 1] = np.nan
    lm[4, 0, 0] = np.inf
    fidx[5], fidx[6] = -1, 3
    dev = frames.cuda()
    A, valid = eng.align_transforms(torch.from_numpy(lm).cuda())
    assert valid.cpu().tolist() == [1, 0, 1, 0, 0, 1, 1, 1]
    assert not A.cpu().numpy()[[1, 3, 4]].any() and torch.isfinite(A).all()
    crop = eng.align_warp(dev, torch.from_numpy(fidx), A, valid).cpu().numpy()
    clean = eng.align_crops(dev, torch.from_numpy(clean_fidx), torch.from_numpy(clean_lm).cuda()).cpu().numpy()
    bad = [1, 3, 4, 5, 6]
    assert not crop[bad].any()
    assert np.array_equal(crop[[0, 2, 7]], clean[[0, 2, 7]]) and clean[[0, 2, 7]].any()
    # transforms that are not finite or far outside, warped without flags: defined (the restatement's) and in bounds
    wild = torch.tensor([[float('nan')] * 6, [1e300, 0, 0, 0, 1e300, 0], [float('inf'), 1, 0, 0, 1, 0], [1, 0, -2e6, 0, 1, 2e6]],
                        dtype=torch.float64)
    got = eng.align_warp(dev, torch.tensor([0, 1, 2, 0]), wild.cuda()).cpu().numpy()
    assert np.array_equal(got, align_ref.warp_batch(frames.numpy(), [0, 1, 2, 0], wild.numpy(), None, (112, 112)))
    # end to end: the flags name the frame index too, invalid faces embed a zero crop, the neighbours are unaffected
    f_new, f, v = net.embed_aligned(dev, torch.from_numpy(fidx), torch.from_numpy(lm).cuda())
    assert v.cpu().tolist() == [1, 0, 1, 0, 0, 0, 0, 1]
    g_new, g = net.embed_u8(torch.from_numpy(crop).cuda())
    assert torch.equal(f_new, g_new) and torch.equal(f, g) and torch.isfinite(f_new).all()


def _rc(eng, fn, *args):
    return getattr(eng.lib, fn)(eng._h, *args)


def test_argument_errors(eng, net):
    P, st, null = native._ptr, eng._stream(), C.c_void_p(0)
    frames = synth.synth_images_u8(2, 64, 80, seed=1).cuda()
    lm = torch.from_numpy((np.array(TEMPLATE_112x112) * 0.4 + 5).astype(np.float32)).cuda().reshape(1, 5, 2).repeat(3, 1, 1)
    tmpl = torch.tensor(TEMPLATE_112x112, dtype=torch.float32).cuda()
    fidx = torch.zeros(3, dtype=torch.int32).cuda()
    A = torch.empty((3, 6), dtype=torch.float64).cuda()
    valid = torch.empty(3, dtype=torch.uint8).cuda()
    crop = torch.empty((3, 256, 256, 3), dtype=torch.uint8).cuda()
    f_new = torch.empty((3, 512)).cuda()

    def tfm(**kw):
        a = dict(lm=P(lm), t=P(tmpl), N=3, K=5, A=P(A), v=P(valid))
        a.update(kw)
        return _rc(eng, 'ffr_align_transforms', a['lm'], a['t'], a['N'], a['K'], a['A'], a['v'], st)

    def warp(e=eng, **kw):
        a = dict(fr=P(frames), F=2, H=64, W=80, pitch=240, fi=P(fidx), A=P(A), v=P(valid), N=3, oh=112, ow=96, c=P(crop))
        a.update(kw)
        return _rc(e, 'ffr_align_warp', a['fr'], a['F'], a['H'], a['W'], a['pitch'], a['fi'], a['A'], a['v'], a['N'], a['oh'],
                   a['ow'], a['c'], st)

    def emb(**kw):
        a = dict(fr=P(frames), F=2, H=64, W=80, pitch=240, fi=P(fidx), lm=P(lm), t=P(tmpl), K=5, fl=null, N=3, fn=P(f_new),
                 f=null, v=null)
        a.update(kw)
        return _rc(net, 'ffr_embed_aligned', a['fr'], a['F'], a['H'], a['W'], a['pitch'], a['fi'], a['lm'], a['t'], a['K'],
                   a['fl'], a['N'], a['fn'], a['f'], a['v'], net._stream())

    assert tfm() == 0 and warp() == 0 and warp(v=null) == 0 and warp(oh=1, ow=4) == 0 and warp(oh=256, ow=256) == 0
    assert emb() == 0
    for bad in (dict(lm=null), dict(t=null), dict(A=null), dict(v=null), dict(N=0), dict(N=-1), dict(K=1), dict(K=17)):
        assert tfm(**bad) == -1, bad
    for bad in (dict(fr=null), dict(fi=null), dict(A=null), dict(c=null), dict(N=0), dict(F=0), dict(H=0), dict(W=0),
                dict(oh=0), dict(oh=257), dict(ow=0), dict(ow=260), dict(ow=98), dict(pitch=239), dict(pitch=1 << 26),
                dict(c=C.c_void_p(crop.data_ptr() + 2))):
        assert warp(**bad) == -1, bad
    for bad in (dict(fr=null), dict(fi=null), dict(lm=null), dict(t=null), dict(fn=null), dict(N=0), dict(K=1), dict(K=17),
                dict(pitch=239), dict(pitch=1 << 26), dict(F=0)):
        assert emb(**bad) == -1, bad
    assert _rc(eng, 'ffr_embed_aligned', P(frames), 2, 64, 80, 240, P(fidx), P(lm), P(tmpl), 5, null, 3, P(f_new), null, null,
               st) == -2                                                         # no weights loaded
    # the binding's own checks
    with pytest.raises(RuntimeError):
        eng.align_transforms(lm.cpu())
    with pytest.raises(RuntimeError):
        eng.align_transforms(lm.double())
    with pytest.raises(RuntimeError):
        eng.align_transforms(lm, [[0.0, 0.0]])
    with pytest.raises(RuntimeError):
        eng.align_warp(frames.float(), fidx, A)
    with pytest.raises(RuntimeError):
        eng.align_warp(frames, fidx[:2], A)
    with pytest.raises(RuntimeError):
        eng.align_warp(frames, fidx, A.float())
    with pytest.raises(RuntimeError):
        eng.align_warp(frames, fidx, A, out_hw=(112, 98))
    with pytest.raises(RuntimeError):
        eng.align_warp(frames.cpu(), fidx, A)


@pytest.mark.parametrize('N', [6, 256])
def test_embed_aligned_equals_embed_u8_of_the_crops(net, N):
    F = 3 if N == 6 else 64
    _, frames, fidx, lm, tmpl = scene(F, 250, 250, N, (112, 112), seed=300 + N)
    dev, dfi, dlm = frames.cuda(), torch.from_numpy(fidx).cuda(), torch.from_numpy(lm).cuda()
    crops = net.align_crops(dev, dfi, dlm)
    for flip in (None, torch.from_numpy(np.arange(N) % 3 == 0)):
        f_new, f, valid = net.embed_aligned(dev, dfi, dlm, flip=flip)
        g_new, g = net.embed_u8(crops, flip)
        assert torch.equal(f_new, g_new) and torch.equal(f, g)
        assert valid.cpu().numpy().all() and torch.isfinite(f_new).all()
    gen = net.generation()
    h_new, h, _ = net.embed_aligned(dev, dfi, dlm, flip=flip)
    assert net.generation() == gen                      # the scratch of this shape is reused
    assert torch.equal(h_new, f_new) and torch.equal(h, f)
    f_only, none, _ = net.embed_aligned(dev, dfi, dlm, flip=flip, want_f=False)
    assert none is None and torch.equal(f_only, f_new)
    if N == 256:
        # faces are independent units: the crop of a face alone is the crop of the batch bit for bit; its embedding in a
        # 1-face call is embed_u8 of that crop bit for bit, and the batch's row within the bound batches hold each other to
        f_new, f, _ = net.embed_aligned(dev, dfi, dlm)
        for q in (0, 101, 255):
            one = (dev, dfi[q:q + 1], dlm[q:q + 1])
            assert torch.equal(net.align_crops(*one), crops[q:q + 1])
            q_new, qf, _ = net.embed_aligned(*one)
            u_new, uf = net.embed_u8(crops[q:q + 1])
            assert torch.equal(q_new, u_new) and torch.equal(qf, uf)
            for a, b in ((q_new, f_new[q:q + 1]), (qf, f[q:q + 1])):
                assert ((a - b).abs().max() / b.abs().max()).item() < BATCH_TOL


def test_frames_to_gallery_search(net):
    """Detector output to identity without the host: the recovered crops enrolled, the transformed frames as probes --
    each face finds its own row first, with the score bits of a search with embed_u8 of the original crops."""
    crops, frames, lm, _ = pasted_scene(16, seed=78)
    dev, dlm, idx = torch.from_numpy(frames).cuda(), torch.from_numpy(lm).cuda(), torch.arange(16)
    recovered = net.align_crops(dev, idx, dlm)
    assert torch.equal(recovered.cpu(), torch.from_numpy(crops))
    gallery = ffrnet_amd.Gallery(net)
    gallery.add(net.embed_u8(recovered)[0])
    probes, _, valid = net.embed_aligned(dev, idx, dlm)
    s1, i1 = gallery.search(probes, k=3)
    s2, i2 = gallery.search(net.embed_u8(torch.from_numpy(crops).cuda())[0], k=3)
    assert valid.cpu().numpy().all()
    assert torch.equal(i1[:, 0].cpu(), idx) and torch.equal(i1, i2) and torch.equal(s1, s2)
    assert (s1[:, 0] > 0.999).all()
