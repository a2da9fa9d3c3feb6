"""CPU checks of the face alignment: the float64 closed form of tests/align_ref.py against the matrices the reference
itself returned (golden G13), the integer warp on cases with a known answer, and the device-free argument checks of
ffrnet_amd.align."""
import os

import numpy as np
import pytest
import torch

import align_ref
from ffrnet_amd import align, synth


@pytest.fixture(scope='module')
def g13(golden_dir):
    return np.load(os.path.join(golden_dir, 'g13_align_transforms.npz'))


def test_closed_form_matches_reference_matrices(g13):
    """The reference's 2x3 matrix (frame -> crop) is the inverse of the closed form's crop -> frame fit: every entry
    within 1e-9 (6e-10 measured on this set, whose translations reach 600 px and scales 4), and the same side of the reflection rule in every case."""
    lm, tmpl, mats = g13['landmarks'], g13['template'], g13['cv2_matrix']
    assert lm.shape[0] >= 200 and lm.shape[1:] == (5, 2) and lm.dtype == np.float32
    worst = 0.0
    for s, M in zip(lm, mats):
        A, valid, _ = align_ref.similarity_dst_to_src(s, tmpl)
        assert valid
        worst = max(worst, np.abs(align_ref.invert_2x3(A) - M).max())
        assert np.sign(np.linalg.det(A[:, :2])) == np.sign(np.linalg.det(M[:, :2]))
    print('max |inverse(closed form) - reference| = %.3e' % worst)
    assert worst < 1e-9
    det = np.linalg.det(mats[:, :, :2])
    assert np.array_equal(det < 0, g13['mirrored'])            # the set holds both branches, decided by the mirroring
    assert 20 <= int((det < 0).sum()) <= lm.shape[0] - 20


def test_templates(g13):
    assert np.array_equal(np.array(align.TEMPLATE_96x112, dtype=np.float64), g13['ref_pts'])
    assert np.array_equal(np.array(align.TEMPLATE_96x112, dtype=np.float32), g13['template'])
    t96, t112 = np.array(align.TEMPLATE_96x112), np.array(align.TEMPLATE_112x112)
    assert np.allclose(t112 - t96, [[8.0, 0.0]] * 5, atol=1e-12)


def test_degenerate_fits_are_invalid_not_errors():
    tmpl = np.array(align.TEMPLATE_112x112)
    for s in (np.full((5, 2), 7.0), np.where(np.eye(5, 2) > 0, np.nan, tmpl), np.where(np.eye(5, 2) > 0, np.inf, tmpl)):
        A, valid, _ = align_ref.similarity_dst_to_src(s, tmpl)
        assert not valid and not A.any()
    A, valid, _ = align_ref.similarity_dst_to_src(tmpl, np.full((5, 2), 3.0))     # den == 0
    assert not valid and not A.any()


def test_ref_warp_identity_translation_quarter_turns():
    img = synth.synth_images_u8(1, 112, 96, seed=5)[0].numpy()
    H, W = img.shape[:2]
    assert np.array_equal(align_ref.warp(img, [1, 0, 0, 0, 1, 0], (H, W)), img)
    # integer translation: crop (x, y) reads frame (x + 5, y - 3); rows that fall outside are the constant-0 border
    out = align_ref.warp(img, [1, 0, 5, 0, 1, -3], (H, W))
    want = np.zeros_like(img)
    want[3:, :W - 5] = img[:H - 3, 5:]
    assert np.array_equal(out, want)
    sq = synth.synth_images_u8(1, 112, 112, seed=6)[0].numpy()
    # quarter turns about the crop: crop (x, y) reads frame (y, 111 - x) etc.
    assert np.array_equal(align_ref.warp(sq, [0, 1, 0, -1, 0, 111], (112, 112)), np.rot90(sq, 3))
    assert np.array_equal(align_ref.warp(sq, [-1, 0, 111, 0, -1, 111], (112, 112)), np.rot90(sq, 2))
    assert np.array_equal(align_ref.warp(sq, [0, -1, 111, 1, 0, 0], (112, 112)), np.rot90(sq, 1))
    assert np.array_equal(align_ref.warp(sq, [-1, 0, 111, 0, 1, 0], (112, 112)), sq[:, ::-1])
    # half a pixel: the mean of two neighbours, rounded half up
    half = align_ref.warp(sq, [1, 0, 0.5, 0, 1, 0], (112, 108))
    assert np.array_equal(half, ((sq[:, :108].astype(np.int64) + sq[:, 1:109] + 1) >> 1).astype(np.uint8))
    # a non-finite or huge transform stays defined
    assert not align_ref.warp(sq, [np.nan] * 6, (8, 8)).any()
    assert not align_ref.warp(sq, [1e300, 0, 0, 0, 1e300, 0], (8, 8))[1:, 1:].any()
    assert not align_ref.warp(sq, np.eye(2, 3).ravel(), (8, 8), valid=False).any()


def test_python_argument_checks_without_a_device():
    t = align.as_template(align.TEMPLATE_112x112)
    assert t.dtype == torch.float32 and tuple(t.shape) == (5, 2) and t.is_contiguous()
    for bad in ([[1.0, 2.0]], [[0.0, 0.0]] * 17, [[1.0, 2.0, 3.0]] * 5, [1.0, 2.0], [[float('nan'), 0.0], [1.0, 1.0]],
                torch.zeros((5, 2), dtype=torch.int32)):
        with pytest.raises(RuntimeError):
            align.as_template(bad)
    assert align.check_out_hw((112, 96)) == (112, 96) and align.check_out_hw([1, 4]) == (1, 4)
    for bad in ((112, 98), (0, 96), (112, 0), (257, 96), (112, 260), (112,), 112):
        with pytest.raises(RuntimeError):
            align.check_out_hw(bad)
    assert align.check_landmarks(torch.zeros((7, 5, 2)), 5) == 7
    for bad in (torch.zeros((7, 4, 2)), torch.zeros((0, 5, 2)), torch.zeros((7, 5, 2), dtype=torch.float64),
                torch.zeros((7, 2, 5)), torch.zeros((7, 10))):
        with pytest.raises(RuntimeError):
            align.check_landmarks(bad, 5)
    with pytest.raises(TypeError):
        align.check_landmarks([[0.0] * 10], 5)
    # the pitch of frames cut out of a wider buffer comes from the row stride; other layouts need a copy
    buf = torch.zeros((3, 20, 40, 3), dtype=torch.uint8)
    assert align.frame_pitch(buf) == 120
    assert align.frame_pitch(buf[:, :, :32]) == 120 and align.frame_pitch(buf[:1, :, 4:36]) == 120
    assert align.frame_pitch(buf[:, :10]) is None              # frames are no longer pitch * H apart
    assert align.frame_pitch(buf[:1, :10]) == 120              # ... which does not matter for a single frame
    assert align.frame_pitch(buf[:, :, ::2]) is None and align.frame_pitch(buf.permute(0, 2, 1, 3)) is None
    align.check_frame_bytes(3 * 1920, 1080)
    with pytest.raises(RuntimeError):
        align.check_frame_bytes(1 << 16, 1 << 15)
