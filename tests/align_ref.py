"""Test infrastructure: numpy restatements of the two definitions of the face alignment (include/ffrnet.h, "face
alignment"; csrc/align.hip) -- the similarity fit in float64 and the integer bilinear warp in int64 arithmetic.  The
cross-check of the native kernels; never imported by the product package."""
import numpy as np


def _candidate(p, q, den):
    """least squares of q ~ L p, L = [a -b; b a] -> (a, b, norm of the residual of L^-1 q against p)"""
    with np.errstate(all='ignore'):
        a = np.sum(p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) / den
        b = np.sum(p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]) / den
        n = a * a + b * b
        if not n > 0.0:
            return a, b, np.inf
        ex = (a * q[:, 0] + b * q[:, 1]) / n - p[:, 0]
        ey = (a * q[:, 1] - b * q[:, 0]) / n - p[:, 1]
        return a, b, np.sqrt(np.sum(ex * ex + ey * ey))


def similarity_dst_to_src(landmarks, template):
    """landmarks [K,2] (frame), template [K,2] (crop) -> (A [2,3] float64 crop -> frame, valid, (norm1, norm2)).
    findSimilarity of lfw/matlab_cp2tform.py in closed form: the least squares of template -> landmarks IS the matrix the
    warp needs; the reflective candidate is the fit with template.x negated, its first column negated afterwards; the
    non-reflective one wins when its residual norm (landmarks mapped into the crop, against the template) is <=."""
    s = np.asarray(landmarks, dtype=np.float64)
    r = np.asarray(template, dtype=np.float64)
    with np.errstate(all='ignore'):
        ms, mr = s.mean(0), r.mean(0)
        q, p = s - ms, r - mr
        den = np.sum(p * p)
        a1, b1, n1 = _candidate(p, q, den)
        a2, b2, n2 = _candidate(p * np.array([-1.0, 1.0]), q, den)
        if n1 <= n2:
            L = np.array([[a1, -b1], [b1, a1]])
        else:
            L = np.array([[-a2, -b2], [-b2, a2]])
        A = np.concatenate((L, (ms - L @ mr)[:, None]), 1)
    valid = bool(den > 0.0 and (np.isfinite(n1) or np.isfinite(n2)) and np.all(np.isfinite(A)))
    return (A if valid else np.zeros((2, 3))), valid, (n1, n2)


def invert_2x3(M):
    """inverse of an affine map given as [2,3], float64"""
    M = np.asarray(M, dtype=np.float64)
    Li = np.linalg.inv(M[:, :2])
    return np.concatenate((Li, -(Li @ M[:, 2])[:, None]), 1)


def warp(frame, A, out_hw, valid=True):
    """frame [H,W,3] uint8, A [6] or [2,3] float64 (crop -> frame) -> crop [oh,ow,3] uint8 by the integer rule:
    coordinates on a 1/32-pixel grid, 10-bit weights, (sum + 512) >> 10, taps outside the frame contribute 0."""
    oh, ow = out_hw
    if not valid or frame is None:
        return np.zeros((oh, ow, 3), np.uint8)
    H, W = frame.shape[:2]
    a = np.asarray(A, dtype=np.float64).reshape(6)
    y, x = np.meshgrid(np.arange(oh, dtype=np.float64), np.arange(ow, dtype=np.float64), indexing='ij')
    f = frame.astype(np.int64)
    with np.errstate(all='ignore'):
        sx = (a[0] * x + a[1] * y) + a[2]
        sy = (a[3] * x + a[4] * y) + a[5]
        sx = np.fmin(np.fmax(sx, -1048576.0), 1048576.0)        # a NaN goes to the lower bound, as fmin(fmax()) on the device
        sy = np.fmin(np.fmax(sy, -1048576.0), 1048576.0)
    fx = np.floor(sx * 32.0 + 0.5).astype(np.int64)
    fy = np.floor(sy * 32.0 + 0.5).astype(np.int64)
    ix, ax, iy, ay = fx >> 5, fx & 31, fy >> 5, fy & 31
    acc = np.zeros((oh, ow, 3), np.int64)
    for dy, dx, w in ((0, 0, (32 - ax) * (32 - ay)), (0, 1, ax * (32 - ay)), (1, 0, (32 - ax) * ay), (1, 1, ax * ay)):
        xx, yy = ix + dx, iy + dy
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        tap = f[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        acc += np.where(inside, w, 0)[:, :, None] * tap
    return ((acc + 512) >> 10).astype(np.uint8)


def warp_batch(frames, frame_index, A, valid, out_hw):
    """frames [F,H,W,3], frame_index [N], A [N,6], valid [N] or None -> crops [N,oh,ow,3]"""
    out = []
    for n in range(len(frame_index)):
        fi = int(frame_index[n])
        ok = (valid is None or bool(valid[n])) and 0 <= fi < len(frames)
        out.append(warp(frames[fi] if ok else None, A[n], out_hw, ok))
    return np.stack(out)
