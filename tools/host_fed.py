#!/usr/bin/env python3
"""Host-fed input: what feeding decoded uint8 images (plus the pair flip flags) instead of fp32 tensors saves, in one
process on one GPU, the variants alternated with repeats.

  verification  the 6000-pair protocol (lfw.get_avg_accuracy, 20 pair batches of 300) from host memory with an fp32
                loader, the same with a uint8 loader, and with the fp32 images already on the device
  training      host-fed NativeTrainer.step at 128 pairs through ShardFeeder(loader, 0, 1, device), fp32 against uint8

Reported per variant: pairs/s (best and median of the repeats), h2d_bytes (ShardFeeder.stats) and the host staging time
(the copies of one pass of the loader into the pinned staging buffer, timed on their own).

    python3 tools/host_fed.py [--out profiles/host_fed.json] [--reps 3]
    python3 tools/host_fed.py --stem      # a few launches of every k_stem form, for rocprofv3 --kernel-trace --stats"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import ffrnet_amd  # noqa: E402
from ffrnet_amd import synth  # noqa: E402
import ffr_oracle as O  # noqa: E402


def u8_images(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 112, 112, 3), generator=g, dtype=torch.uint8)


def as_float(img, flip, bs=500):
    return torch.cat([O.preprocess_u8(img[s:s + bs], flip[s:s + bs]) for s in range(0, img.size(0), bs)])


def staging_seconds(loader):
    """Host side of ShardFeeder for one pass: both halves of every batch into a pinned block (world 1)."""
    a = loader[0]['img1']
    buf = torch.empty(2 * a.numel() + a.size(0), dtype=a.dtype, pin_memory=True)
    t0 = time.perf_counter()
    for d in loader:
        m, k = d['img1'].size(0), d['img1'][0].numel()
        host = buf[:2 * m * k].view((2 * m,) + tuple(d['img1'].shape[1:]))
        host[:m].copy_(d['img1'])
        host[m:].copy_(d['img2'])
        if 'flip' in d and a.dtype == torch.uint8:
            buf[2 * m * k:2 * m * k + m].copy_(d['flip'].to(torch.uint8))
    return time.perf_counter() - t0


def summary(times, units):
    rates = [units / t for t in times]
    return dict(best_per_s=max(rates), median_per_s=statistics.median(rates), seconds=times)


def stem_launches(eng, sd_r):
    """embed / embed_u8 at batch 256 and one training iteration at 128 pairs, float and uint8 (the two-source stem)."""
    img = u8_images(256, 3).cuda()
    flip = torch.arange(256, device='cuda') % 2 == 0
    x = as_float(img.cpu(), flip.cpu()).cuda()
    label = torch.randint(0, 10575, (128,), generator=torch.Generator().manual_seed(1)).cuda()
    tr = ffrnet_amd.NativeTrainer(eng, sd_r, lr=1e-3)
    for _ in range(6):
        eng.embed(x)
        eng.embed_u8(img, flip)
        tr.step(x[:128], x[128:], label)
        tr.step(img[:128], img[128:], label, flip[:128])
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'host_fed.json'))
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--pairs', type=int, default=6000)
    ap.add_argument('--train-iters', type=int, default=10)
    ap.add_argument('--stem', action='store_true')
    args = ap.parse_args()
    with open(os.path.join(ROOT, 'tests', 'golden', 'g0_state_dict_keys.json')) as f:
        specs = json.load(f)
    sd_e = synth.synth_state_dict(specs['encoder'], seed=0)
    sd_r = synth.synth_state_dict(specs['recnet'], seed=0)
    eng = ffrnet_amd.Engine(0)
    eng.load_encoder(sd_e)
    eng.load_recnet(sd_r)
    if args.stem:
        stem_launches(eng, sd_r)
        return

    # verification loaders: the same images and flips three ways
    P, BS = args.pairs, 300
    i1, i2 = u8_images(P, 11), u8_images(P, 12)
    flip = torch.rand(P, generator=torch.Generator().manual_seed(13)) < 0.5
    lab = (torch.arange(P) % 600 < 300).long()
    f1, f2 = as_float(i1, flip), as_float(i2, flip)
    cut = [(s, min(s + BS, P)) for s in range(0, P, BS)]
    loaders = {
        'fp32_host': [dict(img1=f1[s:e], img2=f2[s:e], label=lab[s:e], idx=torch.arange(s, e)) for s, e in cut],
        'uint8_host': [dict(img1=i1[s:e], img2=i2[s:e], label=lab[s:e], idx=torch.arange(s, e), flip=flip[s:e])
                       for s, e in cut],
        'fp32_device': [dict(img1=f1[s:e].cuda(), img2=f2[s:e].cuda(), label=lab[s:e], idx=torch.arange(s, e))
                        for s, e in cut],
    }
    ver = {k: dict(times=[], h2d_bytes=None, staging_s=[], acc=None) for k in loaders}
    for name, ld in loaders.items():                      # warm-up: arena, mixed-tile weights, pinned buffers
        ffrnet_amd.lfw.get_avg_accuracy(eng.embed, ld)
    for _ in range(args.reps):
        for name, ld in loaders.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc = ffrnet_amd.lfw.get_avg_accuracy(eng.embed, ld)
            torch.cuda.synchronize()
            ver[name]['times'].append(time.perf_counter() - t0)
            ver[name]['h2d_bytes'] = ffrnet_amd.lfw.last_feed_stats['h2d_bytes']
            ver[name]['acc'] = acc
            if name.endswith('host'):
                ver[name]['staging_s'].append(staging_seconds(ld))
    assert ver['fp32_host']['acc'] == ver['uint8_host']['acc'] == ver['fp32_device']['acc']
    for v in ver.values():
        v.update(summary(v.pop('times'), P))

    # training: host-fed 128-pair iterations
    N, IT = 128, args.train_iters
    non, ocl = u8_images(N * IT, 21), u8_images(N * IT, 22)
    tflip = torch.rand(N * IT, generator=torch.Generator().manual_seed(23)) < 0.5
    tlab = torch.randint(0, 10575, (N * IT,), generator=torch.Generator().manual_seed(24))
    tnon, tocl = as_float(non, tflip), as_float(ocl, tflip)
    tcut = [(s, s + N) for s in range(0, N * IT, N)]
    tload = {
        'fp32_host': [dict(img1=tnon[s:e], img2=tocl[s:e], label=tlab[s:e]) for s, e in tcut],
        'uint8_host': [dict(img1=non[s:e], img2=ocl[s:e], label=tlab[s:e], flip=tflip[s:e]) for s, e in tcut],
    }
    trn = {k: dict(times=[], h2d_bytes=None, staging_s=[]) for k in tload}

    def train_pass(ld):
        tr = ffrnet_amd.NativeTrainer(eng, sd_r, lr=1e-3)
        eng.validate_labels = False                       # no per-step device sync for the label range check
        feeder = ffrnet_amd.lfw.ShardFeeder(ld, 0, 1, eng.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for data, both, m, n in feeder:
            tr.step(both[:m], both[m:], data['label'], feeder.pair_flip)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, feeder.stats['h2d_bytes'], float(torch.stack(tr.loss_items).sum())

    for name, ld in tload.items():
        train_pass(ld)
    for _ in range(args.reps):
        losses = {}
        for name, ld in tload.items():
            t, b, losses[name] = train_pass(ld)
            trn[name]['times'].append(t)
            trn[name]['h2d_bytes'] = b
            trn[name]['staging_s'].append(staging_seconds(ld))
        assert losses['fp32_host'] == losses['uint8_host'], losses
    for v in trn.values():
        v.update(summary(v.pop('times'), N * IT))
    eng.validate_labels = True

    out = dict(device=torch.cuda.get_device_name(0), pairs=P, pair_batch=BS, reps=args.reps,
               verification=ver, training=dict(pairs_per_iteration=N, iterations=IT, **trn),
               uint8_vs_device_resident=ver['uint8_host']['best_per_s'] / ver['fp32_device']['best_per_s'],
               uint8_vs_fp32_host=ver['uint8_host']['best_per_s'] / ver['fp32_host']['best_per_s'],
               train_uint8_vs_fp32_host=trn['uint8_host']['best_per_s'] / trn['fp32_host']['best_per_s'])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if not isinstance(v, dict)}))


if __name__ == '__main__':
    main()
