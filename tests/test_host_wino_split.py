"""The packer's 3-way bf16 split (pack.cpp: split_bf16x3, behind the weight planes of the split-operand forms of k_igemm and
k_wino_fused) on the host, through ffr_split_planes_host: no device needed."""
import ctypes

import numpy as np
import torch

from ffrnet_amd import native


def split(w):
    lib = ctypes.CDLL(native.lib_path())
    w = np.ascontiguousarray(w, dtype=np.float64).ravel()
    planes = np.zeros((3, w.size), dtype=np.uint16)
    rc = lib.ffr_split_planes_host(ctypes.c_void_p(w.ctypes.data), ctypes.c_longlong(w.size), ctypes.c_void_p(planes.ctypes.data))
    assert rc == 0
    return planes


def as_double(planes):
    return (planes.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def test_planes_reproduce_the_double_precision_winograd_weights():
    """U = G g G^T in double for random 3x3 filters: p1 + p2 + p3 = U to 2^-24 relative, i.e. the planes carry at least what
    the fp32 rounding of U carried."""
    G = np.array([[0.25, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]])
    rng = np.random.default_rng(5)
    g = rng.standard_normal((4096, 3, 3)).astype(np.float32).astype(np.float64) / 24.0
    U = np.einsum('ik,nkl,jl->nij', G, g, G).ravel()
    U = np.concatenate([U, U * 1e-30, U * 1e30, [0.0, 1.0, -1.0, 2.0 ** -126, 3.0 * 2.0 ** -130]])
    p = as_double(split(U))
    err = np.abs(p.sum(axis=0) - U)
    # each piece leaves at most half a unit of its 8-bit significand: 2^-8 of what it rounded; 2^-134 where a piece is a bf16 subnormal
    assert (err <= np.maximum(2.0 ** -24 * np.abs(U), 2.0 ** -134)).all(), (err / np.maximum(np.abs(U), 1e-300)).max()
    assert (np.abs(p[1]) <= 2.0 ** -8 * np.abs(p[0]) + 1e-300).all() and (np.abs(p[2]) <= 2.0 ** -8 * np.abs(p[1]) + 1e-300).all()


def test_first_plane_is_round_to_nearest_even_bf16():
    """Against torch's float32 -> bfloat16 conversion, ties included (values with exactly one bit below the bf16 significand)."""
    rng = np.random.default_rng(6)
    w = rng.standard_normal(8192).astype(np.float32)
    ties = (rng.integers(128, 256, 512).astype(np.float32) + 0.5) * np.float32(2.0) ** rng.integers(-20, 20, 512).astype(np.float32)
    w = np.concatenate([w, ties, -ties])
    want = torch.from_numpy(w).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(split(w.astype(np.float64))[0], want)
