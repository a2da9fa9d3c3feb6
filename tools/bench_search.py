"""Time the exact 1:N search (Engine.search: k_row_norms + k_search_topk + k_topk_merge) with device events after a
warm-up, against torch.mm + torch.topk on the same device and inputs, and check the ranking criterion of
tests/test_gpu_search.py at every shape (float64 oracle on the first probes).

  python tools/bench_search.py [--reps N] [--json OUT]

Per shape: ms, TFLOP/s (2*Q*G*512 / t), its fraction of the 157.3 TFLOP/s fp32-MFMA peak, the gallery read rate
(G*512*4 bytes / t) against 8 TB/s, the torch time and the speed-up."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd  # noqa: E402

PEAK_TFLOPS = 157.3
PEAK_TBS = 8.0
SHAPES = [(1, 1 << 20, 10), (32, 1 << 20, 10), (256, 1 << 20, 10), (1024, 1 << 20, 10), (256, 4 << 20, 10),
          (256, 1 << 20, 100)]
TOL = 1e-6


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def check(q, g, k, s, i, nprobe=16):
    """ranking criterion on the first probes: scores within TOL of float64, distinct indices in the total order, no row
    left out above the k-th + 2 TOL"""
    q, s, i = q[:nprobe], s[:nprobe], i[:nprobe]
    q64 = q.double()
    qn = q64.norm(dim=1)
    got = torch.empty_like(s, dtype=torch.float64)
    best = torch.full((q.size(0),), float('-inf'), device=q.device, dtype=torch.float64)
    step = 1 << 19
    for lo in range(0, g.size(0), step):
        g64 = g[lo:lo + step].double()
        c = (q64 @ g64.T) / (qn[:, None] * g64.norm(dim=1)[None, :] + 1e-8)
        inside = (i >= lo) & (i < lo + g64.size(0))
        got[inside] = c.gather(1, (i - lo).clamp(0, g64.size(0) - 1))[inside]
        c = torch.cat((c, torch.full((c.size(0), 1), float('-inf'), device=c.device, dtype=c.dtype)), 1)
        c.scatter_(1, torch.where(inside, i - lo, g64.size(0)), float('-inf'))     # returned rows leave; others -> spare column
        best = torch.maximum(best, c.max(1).values)
    srt = torch.sort(i, 1).values
    order = bool(torch.all((s[:, :-1] > s[:, 1:]) | ((s[:, :-1] == s[:, 1:]) & (i[:, :-1] < i[:, 1:]))))
    err = (got - s.double()).abs().max().item()
    miss = (best - s[:, -1].double()).max().item()
    return dict(max_err=err, max_left_out_above_kth=miss, distinct=bool(torch.all(srt[:, 1:] != srt[:, :-1])), ordered=order,
                ok=bool(err <= TOL and miss <= 2 * TOL and order))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--json', default=None)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    eng = ffrnet_amd.Engine(0)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    gall = torch.randn((max(G for _, G, _ in SHAPES), 512), device='cuda', generator=gen)
    probes = torch.randn((max(Q for Q, _, _ in SHAPES), 512), device='cuda', generator=gen)
    norms_all = eng.row_norms(gall)
    rows = []
    print('%6s %9s %4s | %8s %7s %6s %8s | %9s %7s | %s' % ('Q', 'G', 'k', 'ms', 'TFLOP/s', 'peak', 'TB/s', 'torch ms',
                                                               'speedup', 'ranking'))
    for Q, G, k in SHAPES:
        q, g, n = probes[:Q], gall[:G], norms_all[:G]
        t = timed(lambda: eng.search(q, g, k, gallery_norms=n), args.reps)
        s, i = eng.search(q, g, k, gallery_norms=n)
        chk = check(q, g, k, s, i)
        flops = 2.0 * Q * G * 512
        r = dict(Q=Q, G=G, k=k, ms=t, tflops=flops / t / 1e9, frac_fp32_mfma_peak=flops / t / 1e9 / PEAK_TFLOPS,
                 gallery_tb_s=G * 512 * 4 / t / 1e9, frac_8tbs=G * 512 * 4 / t / 1e9 / PEAK_TBS, ranking=chk)
        if not args.no_torch:
            def ref():
                sc = torch.mm(q, g.T)
                sc /= q.norm(dim=1)[:, None] * n[None, :] + 1e-8
                return torch.topk(sc, k, dim=1)
            r['torch_ms'] = timed(ref, max(3, args.reps // 2))
            r['speedup'] = r['torch_ms'] / t
        rows.append(r)
        print('%6d %9d %4d | %8.3f %7.1f %6.3f %8.2f | %9s %7s | %s' % (
            Q, G, k, t, r['tflops'], r['frac_fp32_mfma_peak'], r['gallery_tb_s'],
            '%.3f' % r['torch_ms'] if 'torch_ms' in r else '-', '%.2fx' % r['speedup'] if 'speedup' in r else '-',
            'ok' if chk['ok'] else 'FAIL %s' % chk), flush=True)
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), peak_tflops=PEAK_TFLOPS, peak_tb_s=PEAK_TBS, shapes=rows)
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
    assert all(r['ranking']['ok'] for r in rows)


if __name__ == '__main__':
    main()
