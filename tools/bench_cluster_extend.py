"""Time the incremental clustering (Engine.cluster_extend: k_cluster_seed + k_cluster_walk over the new rows +
k_cluster_flatten) against clustering everything again (Engine.cluster over all N rows), on the planted identities of
tools/bench_cluster.py, with device events after a warm-up, the two calls interleaved in one process.

  python tools/bench_cluster_extend.py [--reps N] [--json OUT] [--sizes 16384,131072]

Per total N the batch sizes N_new = N/32, N/8, N/2 and one small batch of 256 rows: the first N - N_new rows are clustered
once (their rep is the prior, on the device, norms handed in), then per shape: ms of both calls, the pairs scored
(N_old N_new + N_new (N_new - 1) / 2) and their rate, the rate of the full clustering (N (N - 1) / 2 pairs) measured in the
same run -- the yardstick --, TFLOP/s and its fraction of the 157.3 TFLOP/s fp32-MFMA peak, the ratio full / extend next to
the ratio of the pair counts it should approach, and whether the labels are equal.  Writes profiles/cluster_extend_bench.json by default."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ffrnet_amd  # noqa: E402
from bench_cluster import PEAK_TFLOPS, THRESHOLD, planted, timed_alternating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sizes', default='16384,131072')
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'cluster_extend_bench.json'))
    args = ap.parse_args()
    eng = ffrnet_amd.Engine(0)
    rows = []
    print('%8s %8s | %10s %10s | %12s %12s %6s | %8s %6s | %8s %8s | %s' % (
        'N', 'N_new', 'extend ms', 'full ms', 'ext pairs/s', 'full pairs/s', 'ratio', 'TFLOP/s', 'peak', 'full/ext', 'by pairs',
        'labels'))
    for N in [int(s) for s in args.sizes.split(',')]:
        emb, _ = planted(N, seed=N)
        norms = eng.row_norms(emb)
        for n_new in sorted({N // 32, N // 8, N // 2, min(256, N)}):
            n_old = N - n_new
            prior = torch.cat((eng.cluster(emb[:n_old], THRESHOLD, norms=norms[:n_old]),
                               torch.arange(n_old, N, device='cuda', dtype=torch.int64)))
            (te, tf), spread = timed_alternating([lambda: eng.cluster_extend(emb, THRESHOLD, prior, n_old, norms=norms, validate=False),
                                                  lambda: eng.cluster(emb, THRESHOLD, norms=norms)], args.reps)
            equal = bool(torch.equal(eng.cluster_extend(emb, THRESHOLD, prior, n_old, norms=norms), eng.cluster(emb, THRESHOLD, norms=norms)))
            pairs = n_old * n_new + n_new * (n_new - 1) // 2
            full_pairs = N * (N - 1) // 2
            rate, full_rate = pairs / (te * 1e-3), full_pairs / (tf * 1e-3)
            tflops = pairs * 2 * 512 / te / 1e9
            row = dict(N=N, N_new=n_new, N_old=n_old, threshold=THRESHOLD, extend_ms=te, extend_ms_min_max=spread[0], full_ms=tf,
                       full_ms_min_max=spread[1], pairs=pairs, pairs_per_s=rate, full_pairs=full_pairs, full_pairs_per_s=full_rate,
                       rate_over_full_rate=rate / full_rate, tflops=tflops, frac_fp32_mfma_peak=tflops / PEAK_TFLOPS,
                       full_tflops=full_pairs * 2 * 512 / tf / 1e9, full_over_extend=tf / te, pair_count_ratio=full_pairs / pairs,
                       labels_equal=equal)
            rows.append(row)
            print('%8d %8d | %10.3f %10.3f | %12.4g %12.4g %6.3f | %8.1f %6.3f | %8.2f %8.2f | %s' % (
                N, n_new, te, tf, rate, full_rate, rate / full_rate, tflops, tflops / PEAK_TFLOPS, tf / te, full_pairs / pairs,
                'equal' if equal else 'DIFFERENT'), flush=True)
        del emb, norms
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), peak_tflops=PEAK_TFLOPS, reps=args.reps, shapes=rows)
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as fjson:
            json.dump(out, fjson, indent=1)
    assert all(r['labels_equal'] for r in rows)


if __name__ == '__main__':
    main()
