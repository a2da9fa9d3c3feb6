"""Time the on-device face alignment (Engine.align_transforms / align_warp / align_crops: k_align_tfm + k_align_warp) and
embed_aligned against embed_u8 of ready crops, with device events after a warm-up, median of the repeats; and a torch
baseline (affine_grid + grid_sample + rounding to uint8) on the same frames and transforms.

  python tools/bench_align.py [--faces 256] [--reps 20] [--json OUT]

Scenes at --faces faces: LFW-sized frames (250 x 250) with one face each, and 1080p frames with 8 faces each.  The short
calls are timed `inner` at a time between two events (one event pair around a 10 us kernel measures the launch).  The
bytes of the warp: 3 * faces * 112 * 112 written, at most four taps read per byte written."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd  # noqa: E402
from ffrnet_amd import synth  # noqa: E402
from ffrnet_amd.align import TEMPLATE_112x112  # noqa: E402


def timed(fn, reps, inner=1):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    ts.sort()
    return dict(ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1])


def timed_pair(fa, fb, reps):
    """two calls alternated in one loop -> (median of a, median of b, median of the per-repeat difference a - b)"""
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ta, tb = [], []
    for i in range(reps):
        first, second = (fa, fb) if i % 2 == 0 else (fb, fa)       # neither call always runs behind the other
        ev[0].record()
        first()
        ev[1].record()
        second()
        ev[2].record()
        ev[2].synchronize()
        t = (ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]))
        ta.append(t[i % 2])
        tb.append(t[1 - i % 2])
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    return med(ta), med(tb), med([a - b for a, b in zip(ta, tb)])


def landmarks_for(n, H, W, seed):
    """the template under small rotations and scales 0.6-2, centred inside the frame"""
    rng = np.random.Generator(np.random.Philox(key=seed))
    tmpl = np.array(TEMPLATE_112x112)
    lm = np.empty((n, 5, 2), np.float32)
    for i in range(n):
        th, sc = rng.uniform(-0.35, 0.35), rng.uniform(0.6, 2.0)
        L = sc * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        lm[i] = (tmpl - tmpl.mean(0)) @ L.T + [rng.uniform(60, W - 60), rng.uniform(60, H - 60)] + rng.uniform(-1, 1, (5, 2))
    return torch.from_numpy(lm).cuda()


def torch_theta(A, H, W, oh, ow):
    """affine_grid's theta (normalised coordinates, align_corners=False) of the pixel transform A [N,6] (crop -> frame)"""
    A = A.cpu().numpy().reshape(-1, 2, 3)
    to_px = np.array([[ow / 2.0, 0, (ow - 1) / 2.0], [0, oh / 2.0, (oh - 1) / 2.0], [0, 0, 1]])        # crop normalised -> pixel
    to_n = np.array([[2.0 / W, 0, 1.0 / W - 1], [0, 2.0 / H, 1.0 / H - 1]])                          # frame pixel -> normalised
    full = np.concatenate((A, np.tile([[[0.0, 0.0, 1.0]]], (A.shape[0], 1, 1))), 1)
    return torch.from_numpy(np.einsum('ij,njk,kl->nil', to_n, full, to_px)).float().cuda()


def torch_warp(frames_f, per_frame, theta, oh, ow):
    """frames_f [F,3,H,W] float (prepared once, not timed); faces of frame f are rows f*per_frame ... -> uint8 crops"""
    grid = TF.affine_grid(theta, (theta.size(0), 3, oh, ow), align_corners=False)
    if per_frame == 1:
        out = TF.grid_sample(frames_f, grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    else:
        out = torch.cat([TF.grid_sample(frames_f[f:f + 1].expand(per_frame, -1, -1, -1), grid[f * per_frame:(f + 1) * per_frame],
                                        mode='bilinear', padding_mode='zeros', align_corners=False)
                         for f in range(frames_f.size(0))])
    return out.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--faces', type=int, default=256)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', default=None)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    N = args.faces
    eng = ffrnet_amd.Engine(0)
    out = dict(device=torch.cuda.get_device_name(0), faces=N, reps=args.reps, scenes=[])
    for name, H, W, per_frame in (('lfw_250x250_1_face_per_frame', 250, 250, 1), ('1080p_8_faces_per_frame', 1080, 1920, 8)):
        F = N // per_frame
        frames = synth.synth_images_u8(F, H, W, seed=11).cuda()
        fidx = (torch.arange(N, dtype=torch.int32) // per_frame).cuda()
        lm = landmarks_for(N, H, W, seed=12)
        A, valid = eng.align_transforms(lm)
        crop_bytes = 3.0 * N * 112 * 112
        r = dict(scene=name, frames=F, H=H, W=W, crop_mbytes=crop_bytes / 1e6)
        r['align_transforms'] = timed(lambda: eng.align_transforms(lm), args.reps, inner=20)
        r['align_warp'] = timed(lambda: eng.align_warp(frames, fidx, A, valid), args.reps, inner=20)
        r['align_crops'] = timed(lambda: eng.align_crops(frames, fidx, lm), args.reps, inner=20)
        r['align_warp']['written_tb_s'] = crop_bytes / r['align_warp']['ms'] / 1e9
        if not args.no_torch:
            frames_f = frames.permute(0, 3, 1, 2).float().contiguous()
            theta = torch_theta(A, H, W, 112, 112)
            r['torch_affine_grid_sample'] = timed(lambda: torch_warp(frames_f, per_frame, theta, 112, 112), max(5, args.reps // 2))
            r['torch_over_align_crops'] = r['torch_affine_grid_sample']['ms'] / r['align_crops']['ms']
            d = (torch_warp(frames_f, per_frame, theta, 112, 112).int() - eng.align_warp(frames, fidx, A, valid).int()).abs()
            r['torch_vs_native_levels'] = dict(max=int(d.max()), mean=float(d.float().mean()))       # fp32 bilinear vs the 1/32 grid
            del frames_f
        out['scenes'].append(r)
        print(json.dumps(r), flush=True)
        if name.startswith('lfw'):
            keep = (frames, fidx, lm)
    with open(os.path.join(ROOT, 'tests', 'golden', 'g0_state_dict_keys.json')) as f:
        specs = json.load(f)
    eng.load_encoder(synth.synth_state_dict(specs['encoder']))
    eng.load_recnet(synth.synth_state_dict(specs['recnet']))
    frames, fidx, lm = keep
    crops = eng.align_crops(frames, fidx, lm)
    a = eng.embed_aligned(frames, fidx, lm)
    b = eng.embed_u8(crops)
    same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
    ta, tb, diff = timed_pair(lambda: eng.embed_aligned(frames, fidx, lm), lambda: eng.embed_u8(crops), args.reps)
    out['embed'] = dict(scene='lfw_250x250_1_face_per_frame', embed_aligned_ms=ta, embed_u8_ms=tb, difference_ms=diff,
                        difference_over_embed_u8=diff / tb, budget=0.02, within_budget=bool(diff / tb < 0.02), bit_identical=same)
    print(json.dumps(out['embed']), flush=True)
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
    assert out['embed']['bit_identical']


if __name__ == '__main__':
    main()
