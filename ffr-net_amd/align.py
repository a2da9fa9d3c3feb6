"""Face alignment on the device: the landmark templates and the argument checks of Engine.align_transforms /
align_warp / align_crops / embed_aligned (native.py; include/ffrnet.h, "face alignment").  The arithmetic is in
csrc/align.hip; nothing here computes on tensors.

Replaces the reference's host preprocessing (lfw/gen_lfw112x96.py `align` with lfw/matlab_cp2tform.py): a
MATLAB-cp2tform similarity from five detector landmarks to a fixed template, then a bilinear warp to the crop."""
import torch

# The five published SphereFace points (left eye, right eye, nose tip, left and right mouth corner; x, y) in a crop 96 wide
# and 112 high: `ref_pts` of lfw/gen_lfw112x96.py:8-9 (tests/golden/g13_align_transforms.npz holds the reference's copy).
TEMPLATE_96x112 = ((30.2946, 51.6963), (65.5318, 51.5014), (48.0252, 71.7366), (33.5493, 92.3655), (62.7299, 92.2041))
# The same points in the 112 x 112 crop the encoder reads: x + 8 centres the 96-wide template in 112 columns.  The
# reference defines no square template; this is this project's choice (the usual convention for 112 x 112 face crops).
TEMPLATE_112x112 = tuple((x + 8.0, y) for x, y in TEMPLATE_96x112)

MAX_POINTS = 16
MAX_OUT = 256


def as_template(template):
    """[K,2] points (nested sequence or tensor), 2 <= K <= 16 -> contiguous float32 CPU or device tensor."""
    t = template if isinstance(template, torch.Tensor) else torch.tensor(template, dtype=torch.float64)
    if t.dim() != 2 or t.size(1) != 2 or not 2 <= t.size(0) <= MAX_POINTS:
        raise RuntimeError('ffrnet_amd: template must be [K,2] points with 2 <= K <= %d, got %s' % (MAX_POINTS, list(t.shape)))
    if not (t.is_floating_point() and bool(torch.isfinite(t).all())):
        raise RuntimeError('ffrnet_amd: template must hold finite floating-point coordinates')
    return t.to(torch.float32).contiguous()


def check_out_hw(out_hw):
    """(out_h, out_w) of a crop: 1..256 each, out_w a multiple of 4 (a thread writes 4 pixels)."""
    try:
        oh, ow = (int(v) for v in out_hw)
    except (TypeError, ValueError):
        raise RuntimeError('ffrnet_amd: out_hw must be (height, width), got %r' % (out_hw,))
    if not (1 <= oh <= MAX_OUT and 1 <= ow <= MAX_OUT) or ow % 4:
        raise RuntimeError('ffrnet_amd: out_hw must be within 1..%d with a width that is a multiple of 4, got %s'
                           % (MAX_OUT, (oh, ow)))
    return oh, ow


def check_landmarks(landmarks, K):
    """landmarks: float32 tensor [N,K,2], N >= 1 -> N."""
    if not isinstance(landmarks, torch.Tensor):
        raise TypeError('landmarks must be a torch.Tensor')
    if landmarks.dtype != torch.float32:
        raise RuntimeError('ffrnet_amd: landmarks must be float32, got %s' % landmarks.dtype)
    if landmarks.dim() != 3 or landmarks.size(0) < 1 or tuple(landmarks.shape[1:]) != (K, 2):
        raise RuntimeError('ffrnet_amd: landmarks expected shape [N,%d,2] with N >= 1, got %s' % (K, list(landmarks.shape)))
    return landmarks.size(0)


def frame_pitch(frames):
    """Row pitch in bytes of uint8 frames [F,H,W,3] whose rows may be padded (a view of a wider buffer), or None when
    the layout needs a copy: pixels must be 3 packed bytes and frames pitch * H apart."""
    F, H, W, C = frames.shape
    sf, sh, sw, sc = frames.stride()
    if C != 3 or sc != 1 or sw != 3 or sh < 3 * W or (F > 1 and sf != sh * H):
        return None
    return sh


def check_frame_bytes(pitch, H):
    if pitch * H >= 1 << 31:
        raise RuntimeError('ffrnet_amd: a frame of %d bytes is over the 2 GiB offset limit of the warp' % (pitch * H))
