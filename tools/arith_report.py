#!/usr/bin/env python3
"""Per-layer arithmetic on a G11 weight family at batch 256: calibrate, attribute, cost.

    python3 tools/arith_report.py [family] [--tol T] [--out path.json]      (family: trained | kaiming | benign_s1)

  1. calibration images synth_images(256, family seed + 1000); tol = a quarter of the MEASURED default-vs-direct distance
     on them unless --tol is given (tests/test_gpu_arith_plan.py uses the same rule); Engine.calibrate(x, tol)
  2. the per-layer table: sensitivity (end-to-end difference with only that layer on Winograd) and the choice
  3. default / all-direct / calibrated vs the float64 reference of golden G11 for f, f_new, featmap, feat_new (G11's 8 images
     as rows 0..7 of another batch of 256) and the stage taps (image 0 of that batch)
  4. device time: the calibrated batch-256 forward (ffr_embed) against the default one (HIP events, alternating, median),
     and the cost of each pinned layer alone (summed per-launch event time of a profiled forward, minus the default's)
Prints the tables and writes the JSON (default profiles/arith_report_<family>.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd  # noqa: E402
from ffrnet_amd import synth  # noqa: E402

TENSORS = ('f', 'featmap', 'f_new', 'feat_new')
TAPS = [(0, 'input_layer')] + [(i + 1, 'body.%d' % i) for i in (0, 2, 3, 6, 7, 20, 21, 23)]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def outputs(eng, x):
    featmap, f = eng.encoder_forward(x)
    f_new, feat_new = eng.recnet_forward(featmap)
    torch.cuda.synchronize()
    return dict(f=f, featmap=featmap, f_new=f_new, feat_new=feat_new)


def profiled_ms(eng, x, reps=3):
    tot = []
    for _ in range(reps):
        eng.profile_enable(True)
        eng.embed(x)
        p = eng.profile_read()
        eng.profile_enable(False)
        tot.append(sum(v['ms'] for v in p.values()))
    return float(np.median(tot))


def time_embed(engs, x, iters=20, warmup=3):
    """Alternating HIP-event timings of ffr_embed, one list per engine -> medians in ms."""
    for e in engs:
        for _ in range(warmup):
            e.embed(x)
    ts = [[] for _ in engs]
    for _ in range(iters):
        for i, e in enumerate(engs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            e.embed(x)
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('family', nargs='?', default='trained', choices=sorted(synth.STRESS_FAMILIES))
    ap.add_argument('--tol', type=float, default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    gdir = os.path.join(ROOT, 'tests', 'golden')
    with open(os.path.join(gdir, 'g0_state_dict_keys.json')) as fh:
        specs = json.load(fh)
    g = np.load(os.path.join(gdir, 'g11_%s.npz' % a.family))
    sd_e, sd_r = synth.stress_state_dicts(a.family, specs['encoder'], specs['recnet'], gdir)
    img_seed = synth.STRESS_FAMILIES[a.family][4]
    engs = {}
    for k in ('cal', 'default', 'direct'):
        e = ffrnet_amd.Engine(0)
        if k == 'direct':
            e.set_option('wino', 0)
        e.load_encoder(sd_e)
        e.load_recnet(sd_r)
        engs[k] = e
    xc = synth.synth_images(256, 112, 112, seed=img_seed + 1000).cuda()
    oc_def, oc_dir = outputs(engs['default'], xc), outputs(engs['direct'], xc)
    d = {k: rel(oc_def[k], oc_dir[k]) for k in TENSORS}
    tol = a.tol if a.tol is not None else max(d.values()) / 4.0
    rep = engs['cal'].calibrate(x=xc, tol=tol)
    pinned = [l['name'] for l in rep['layers'] if l['arith'] == 'direct']

    x8 = synth.synth_images(8, 112, 112, seed=img_seed)
    xh = synth.synth_images(256, 112, 112, seed=img_seed + 2000)
    xh[:8] = x8
    xh = xh.cuda()
    res = {k: outputs(engs[k], xh) for k in ('default', 'direct', 'cal')}
    held = {k: rel(res['cal'][k], res['direct'][k]) for k in TENSORS}
    vs64 = {}
    for k, key, sel in (('f', 'f', lambda t: t[:8]), ('f_new', 'f_new', lambda t: t[:8]),
                        ('featmap', 'featmap0', lambda t: t[0]), ('feat_new', 'feat_new0', lambda t: t[0])):
        ref64 = torch.from_numpy(g[key + '_f64'])
        amax = ref64.abs().max().item()
        row = {m: (sel(res[m][k]).double().cpu() - ref64).abs().max().item() / amax for m in res}
        row['ref_fp32'] = (torch.from_numpy(g[key]).double() - ref64).abs().max().item() / amax
        vs64[k] = row
    for nb, name in TAPS:
        s64 = torch.from_numpy(g['tap.' + name + '.samples_f64'])
        amax = float(g['tap.' + name + '.absmax'])
        row = {}
        for m in ('default', 'direct', 'cal'):
            got = engs[m].encoder_trunk_nhwc(xh, nb)[0].permute(2, 0, 1).reshape(-1)
            step = max(1, got.numel() // 256)
            row[m] = (got[::step][:256].double().cpu() - s64).abs().max().item() / amax
        row['ref_fp32'] = (torch.from_numpy(g['tap.' + name + '.samples']).double() - s64).abs().max().item() / amax
        vs64['tap ' + name] = row

    ms_def, ms_cal = time_embed([engs['default'], engs['cal']], xh)
    base_ms = profiled_ms(engs['default'], xh)
    cost = {}
    probe = engs['direct']                       # reused: wino back to 1, one layer pinned at a time
    probe.set_option('wino', 1)
    for name in pinned:
        probe.set_arithmetic_plan({name: 'direct'})
        cost[name] = profiled_ms(probe, xh) - base_ms
    probe.set_arithmetic_plan({})
    all_pinned_ms = None
    if pinned:
        probe.set_arithmetic_plan({n: 'direct' for n in pinned})
        all_pinned_ms = profiled_ms(probe, xh) - base_ms

    out = dict(family=a.family, batch=256, tol=tol, tol_rule='given' if a.tol is not None else 'default_vs_direct / 4',
               default_vs_direct_calibration_images=d, achieved=rep['achieved'], held_out_calibrated_vs_direct=held,
               layers=rep['layers'], pinned=pinned, vs_float64=vs64,
               embed_ms_default=ms_def, embed_ms_calibrated=ms_cal,
               device_ms_profiled_default=base_ms, pinned_cost_ms=cost, pinned_all_cost_ms=all_pinned_ms)
    print('family %s, batch 256: default vs direct on the calibration images %s -> tol %.3g' %
          (a.family, ', '.join('%s %.2e' % kv for kv in d.items()), tol))
    print('\n%-28s %-8s %12s %s' % ('layer', 'net', 'sensitivity', 'arith'))
    for l in rep['layers']:
        print('%-28s %-8s %12.3e %s' % (l['name'], l['net'], l['sensitivity'], l['arith']))
    print('\nachieved on the calibration images:', {k: v for k, v in rep['achieved'].items()})
    print('held out (G11 images as rows 0..7 of another 256), calibrated vs direct:', held)
    print('\n%-18s %11s %11s %11s %11s' % ('vs float64', 'default', 'direct', 'calibrated', 'ref fp32'))
    for k, r in vs64.items():
        print('%-18s %11.3e %11.3e %11.3e %11.3e' % (k, r['default'], r['direct'], r['cal'], r['ref_fp32']))
    print('\nffr_embed at 256 (HIP events, median of 20): default %.3f ms, calibrated %.3f ms (%+.1f %%)' %
          (ms_def, ms_cal, 100.0 * (ms_cal / ms_def - 1.0)))
    for n, c in cost.items():
        print('  pinning %-26s alone: %+.3f ms of device time per forward' % (n, c))
    if all_pinned_ms is not None:
        print('  all %d pinned layers together: %+.3f ms' % (len(pinned), all_pinned_ms))
    path = a.out or os.path.join(ROOT, 'profiles', 'arith_report_%s.json' % a.family)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
    for e in engs.values():
        e.close()


if __name__ == '__main__':
    main()
