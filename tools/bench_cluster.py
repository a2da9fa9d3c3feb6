"""Time the on-device clustering (Engine.cluster: k_row_norms + k_cluster_init + k_cluster_walk + k_cluster_flatten) on
planted identities of about 8 rows each, with device events after a warm-up, against

  (b) Engine.search(emb, emb, k=1) at the same N: the same K loop over the full N x N rectangle, the yardstick;
  (c) torch on the same device: chunked torch.mm + threshold + min-label propagation until nothing changes.

  python tools/bench_cluster.py [--reps N] [--json OUT] [--sizes 16384,131072] [--no-torch]

(a) and (b) are timed alternately in the same process, the median of --reps calls each.  Per size: ms of each, the
pair rate of (a) (N(N-1)/2 pairs / t), its TFLOP/s (N(N-1)*512 / t) and that as a fraction of the 157.3 TFLOP/s fp32-MFMA
peak, the ratios (b)/(a) and (c)/(a), and whether the labels are the planted ones and equal to the torch baseline's.
Writes profiles/cluster_bench.json by default."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd  # noqa: E402
from ffrnet_amd import cluster as fc  # noqa: E402

PEAK_TFLOPS = 157.3
THRESHOLD = 0.5


def planted(N, seed):
    """N rows of N/8 identities (sizes vary around 8): (unit centre + 0.02 randn) * uniform(0.5, 2), shuffled.  Members
    of one identity score about 0.83, different identities below 0.3: far from the threshold on both sides."""
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    ids = torch.sort(torch.randint(0, max(N // 8, 1), (N,), device='cuda', generator=gen)).values
    centres = torch.randn((max(N // 8, 1), 512), device='cuda', generator=gen)
    centres /= centres.norm(dim=1, keepdim=True)
    emb = centres[ids] + 0.02 * torch.randn((N, 512), device='cuda', generator=gen)
    emb *= 0.5 + 1.5 * torch.rand((N, 1), device='cuda', generator=gen)
    perm = torch.randperm(N, device='cuda', generator=gen)
    return emb[perm].contiguous(), ids[perm].contiguous()


def timed_alternating(fns, reps):
    """median ms of each function, the calls interleaved (a b a b ...) after one warm-up call of each"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    return [sorted(t)[len(t) // 2] for t in ts], [(min(t), max(t)) for t in ts]


def torch_cluster(emb, norms, threshold, chunk=4096):
    """min-label propagation: label[i] <- min(label[j] : s(i, j) > threshold) until a fixed point; -> (rep, sweeps)"""
    N = emb.size(0)
    label = torch.arange(N, device=emb.device, dtype=torch.int32)
    big = torch.tensor(N, device=emb.device, dtype=torch.int32)
    sweeps = 0
    while True:
        new = label.clone()
        for lo in range(0, N, chunk):
            sc = torch.mm(emb[lo:lo + chunk], emb.T)
            sc /= norms[lo:lo + chunk, None] * norms[None, :] + 1e-8
            near = torch.where(sc > threshold, label[None, :], big).min(1).values
            new[lo:lo + chunk] = torch.minimum(new[lo:lo + chunk], near)
        sweeps += 1
        if bool(torch.equal(new, label)):
            return label.long(), sweeps
        label = new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sizes', default='16384,131072')
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'cluster_bench.json'))
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    eng = ffrnet_amd.Engine(0)
    rows = []
    print('%8s | %10s %8s %6s | %10s %7s | %10s %7s %6s | %s' % ('N', 'cluster ms', 'TFLOP/s', 'peak', 'search ms', '(b)/(a)',
                                                                  'torch ms', '(c)/(a)', 'sweeps', 'labels'))
    for N in [int(s) for s in args.sizes.split(',')]:
        emb, ids = planted(N, seed=N)
        norms = eng.row_norms(emb)
        (ta, tb), spread = timed_alternating([lambda: eng.cluster(emb, THRESHOLD, norms=norms),
                                              lambda: eng.search(emb, emb, 1, gallery_norms=norms)], args.reps)
        rep = eng.cluster(emb, THRESHOLD, norms=norms)
        c = fc.dense_ids(rep)
        p, r, f = fc.pairwise_scores(c.cluster_id, ids)
        flops = float(N) * (N - 1) * 512
        row = dict(N=N, threshold=THRESHOLD, n_clusters=c.n_clusters, cluster_ms=ta, cluster_ms_min_max=spread[0],
                   search_k1_ms=tb, search_k1_ms_min_max=spread[1], search_over_cluster=tb / ta,
                   pairs_per_s=N * (N - 1) / 2 / (ta * 1e-3), tflops=flops / ta / 1e9,
                   frac_fp32_mfma_peak=flops / ta / 1e9 / PEAK_TFLOPS, pairwise_precision_recall_f=[p, r, f],
                   labels_ok=bool(p == 1.0 and r == 1.0))
        if not args.no_torch:
            want, sweeps = torch_cluster(emb, norms, THRESHOLD)          # also the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ts = []
            for _ in range(max(3, args.reps // 2)):
                e0.record()
                torch_cluster(emb, norms, THRESHOLD)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            row.update(torch_ms=sorted(ts)[len(ts) // 2], torch_sweeps=sweeps, torch_over_cluster=sorted(ts)[len(ts) // 2] / ta,
                       equals_torch=bool(torch.equal(want, rep)))
            row['labels_ok'] = row['labels_ok'] and row['equals_torch']
        rows.append(row)
        print('%8d | %10.3f %8.1f %6.3f | %10.3f %7.2f | %10s %7s %6s | %s' % (
            N, ta, row['tflops'], row['frac_fp32_mfma_peak'], tb, tb / ta,
            '%.3f' % row['torch_ms'] if 'torch_ms' in row else '-',
            '%.2f' % row['torch_over_cluster'] if 'torch_ms' in row else '-', row.get('torch_sweeps', '-'),
            'ok (%d clusters)' % c.n_clusters if row['labels_ok'] else 'FAIL %s' % row), flush=True)
        del emb, ids, norms
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), peak_tflops=PEAK_TFLOPS, reps=args.reps, sizes=rows)
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as fjson:
            json.dump(out, fjson, indent=1)
    assert all(r['labels_ok'] for r in rows)


if __name__ == '__main__':
    main()
