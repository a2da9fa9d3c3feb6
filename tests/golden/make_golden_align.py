#!/usr/bin/env python3
"""Generate tests/golden/g13_align_transforms.npz by running THE REFERENCE ITSELF on CPU.

Run in the build container only (needs /root/reference, which never travels):
    python tests/golden/make_golden_align.py

What runs is the reference's own code, imported from its directory:
  lfw/matlab_cp2tform.py:503-537  get_similarity_transform_for_cv2(src_pts, dst_pts)   (findSimilarity, :340-432)
called as lfw/gen_lfw112x96.py:12-15 calls it: float32 landmarks, float32 template.  findSimilarity negates column 0 of
the array it is handed (`xyR = xy` is an alias, :407-408), so every call gets copies.
`ref_pts` is read out of lfw/gen_lfw112x96.py:8-9 as data (the file itself imports cv2 and walks a dataset when imported).

Stored: 256 seeded landmark sets of K = 5 points (upright faces, rotations over the full circle, scales 0.5-4,
translations up to 600 px, point noise up to 1.5 px, a fifth of them mirrored), the template, the 2x3 matrices the
reference returned (frame -> crop, what it hands to cv2.warpAffine) in float64, the mirrored flags and ref_pts.  Cases
whose two residual norms differ by less than 1e-6 relative are near-ties of the reflection rule, which no tolerance
can pin: they are drawn again."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_LFW = '/root/reference/lfw'
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF_LFW)
import align_ref  # noqa: E402
from matlab_cp2tform import get_similarity_transform_for_cv2  # noqa: E402

N_CASES, SEED = 256, 13


def reference_ref_pts():
    tree = ast.parse(open(os.path.join(REF_LFW, 'gen_lfw112x96.py')).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], 'id', None) == 'ref_pts':
            return np.array(ast.literal_eval(node.value), dtype=np.float64)
    raise RuntimeError('ref_pts not found')


def draw(rng, i, r):
    """case i: kind by i % 4 -- 0 upright, 1 rotated over the full circle, 2 rotated + scaled, 3 noisy; every fifth mirrored"""
    kind = i % 4
    theta = rng.uniform(-0.15, 0.15) if kind == 0 else rng.uniform(-np.pi, np.pi)
    scale = rng.uniform(0.9, 1.2) if kind in (0, 1) else rng.uniform(0.5, 4.0)
    noise = 1.5 if kind == 3 else 0.3
    t = rng.uniform(0.0, 600.0, 2)
    L = scale * np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    s = r.astype(np.float64) @ L.T + t + rng.uniform(-noise, noise, r.shape)
    mirrored = i % 5 == 4
    if mirrored:
        s[:, 0] = 2.0 * t[0] - s[:, 0]
    return s.astype(np.float32), mirrored


def main():
    ref_pts = reference_ref_pts()
    r = ref_pts.astype(np.float32)
    rng = np.random.Generator(np.random.Philox(key=SEED))
    lm, mats, mir, redrawn = [], [], [], 0
    i = 0
    while len(lm) < N_CASES:
        s, mirrored = draw(rng, i, r)
        _, valid, (n1, n2) = align_ref.similarity_dst_to_src(s, r)
        if not valid or abs(n1 - n2) < 1e-6 * max(n1, n2):
            redrawn += 1
            continue
        M = get_similarity_transform_for_cv2(s.copy(), r.copy())
        lm.append(s)
        mats.append(np.asarray(M, dtype=np.float64))
        mir.append(mirrored)
        i += 1
    out = os.path.join(HERE, 'g13_align_transforms.npz')
    np.savez_compressed(out, landmarks=np.stack(lm), template=r, cv2_matrix=np.stack(mats), mirrored=np.array(mir),
                        ref_pts=ref_pts)
    det = np.linalg.det(np.stack(mats)[:, :, :2])
    print('wrote %s: %d cases (%d redrawn), %d reflective by determinant, %d mirrored, %d bytes'
          % (out, len(lm), redrawn, int((det < 0).sum()), int(np.sum(mir)), os.path.getsize(out)))


if __name__ == '__main__':
    main()
