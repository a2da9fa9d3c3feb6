#!/usr/bin/env python3
"""The weight-gradient launch plan of one training backward, at the G8 test batch (4 pairs) and at the benchmarked batch
(128 pairs), in both arithmetics: every launch_wgrad / launch_wgrad_batched call as the plan record of the handle shows it
(ffr_train_wgrad_plan, include/ffrnet_train.h).  The plan depends on the shapes only, so the inputs are random.

    python3 tools/wgrad_plan.py [--out profiles/wgrad_plan.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd  # noqa: E402
from ffrnet_amd import synth  # noqa: E402


def plan_of(eng, sd_r, n, winograd):
    g = torch.Generator().manual_seed(n)
    fm = torch.randn(2 * n, 512, 7, 7, generator=g).cuda()
    f_enc = torch.randn(2 * n, 512, generator=g).cuda()
    label = torch.randint(0, 10575, (n,), generator=g).cuda()
    eng.train_init(sd_r)
    eng.train_option('winograd', winograd)
    eng.train_forward(fm, torch.cat((label, label)), groups=2, want=())
    eng.train_losses(f_enc)
    eng.train_zero_grad()
    eng.train_backward_losses()
    torch.cuda.synchronize()
    return eng.train_wgrad_plan()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wgrad_plan.txt'))
    args = ap.parse_args()
    with open(os.path.join(ROOT, 'tests', 'golden', 'g0_state_dict_keys.json')) as f:
        import json
        specs = json.load(f)
    sd_r = synth.synth_state_dict(specs['recnet'], seed=0)
    eng = ffrnet_amd.Engine(0)
    lines = []
    cols = ('layer', 'name', 'path', 'rows', 'cout_pad', 'Ng', 'nbatch', 'nkt', 'splits', 'kt_per_split', 'full_tiles',
            'tail_splits', 'tail_kt', 'accumulate')
    for n in (4, 128):
        for wino in (1, 0):
            lines.append('## %d pairs (%d images), winograd=%d' % (n, 2 * n, wino))
            lines.append('%5s %-26s %-11s %6s %8s %5s %6s %4s %6s %12s %10s %11s %7s %10s' % cols)
            for p in plan_of(eng, sd_r, n, wino):
                lines.append('%5d %-26s %-11s %6d %8d %5d %6d %4d %6d %12d %10d %11d %7d %10d' % tuple(p[c] for c in cols))
            lines.append('')
    eng.train_option('winograd', 1)
    text = '\n'.join(lines)
    print(text)
    with open(args.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
