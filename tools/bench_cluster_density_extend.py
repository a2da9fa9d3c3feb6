"""Time the extension of a density-gated clustering (Engine.cluster_density_extend: the seed, k_cluster_walk twice over the
pairs with a new row, the promoted list, k_list_walk over it, root / min / label) against clustering everything again
(Engine.cluster_density over all N rows), on the bridged planted identities of tools/bench_cluster_density.py, with device
events after a warm-up, the two calls interleaved in one process.

  python tools/bench_cluster_density_extend.py [--reps N] [--json OUT] [--sizes 16384,131072] [--min-rows 4]

The shapes of tools/bench_cluster_extend.py: per total N the batch sizes N_new = N/32, N/8, N/2 and one small batch of 256
rows.  The first N - N_new rows are clustered once (the extension from nothing: that is the state), then per shape rep, kind
and degree of the extension are held equal to the full call's BEFORE any time is printed, and: ms of both calls, the ratio
full / extend next to the ratio of the pair counts N (N - 1) / (2 N_old N_new + N_new (N_new - 1) + m N_old) it should
approach, m (the old rows the batch made core) and the share of the scored pairs each of the three passes has (degree walk,
gated walk, promoted pass: shares of the work by count, not separately timed).  Shapes where the extension is slower than
the full call are marked.  Writes profiles/cluster_density_extend_bench.json by default.

For the passes' share of the time, trace the kernels in a run of its own (EXPERIMENTS.md has the figures):

  rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_cluster_density_extend.py --trace-shape 131072,4096"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ffrnet_amd  # noqa: E402
from bench_cluster import THRESHOLD, timed_alternating  # noqa: E402
from bench_cluster_density import planted_bridged  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sizes', default='16384,131072')
    ap.add_argument('--min-rows', type=int, default=4)
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'cluster_density_extend_bench.json'))
    ap.add_argument('--trace-shape', default=None, metavar='N,N_NEW',
                    help='run only the extension of this one shape, 5 times, and print nothing else: for rocprofv3 --kernel-trace --stats')
    args = ap.parse_args()
    eng = ffrnet_amd.Engine(0)
    mr = args.min_rows
    if args.trace_shape:
        N, n_new = [int(s) for s in args.trace_shape.split(',')]
        emb, _, _ = planted_bridged(N, seed=N)
        norms = eng.row_norms(emb)
        state = eng.cluster_density_extend(emb[:N - n_new], THRESHOLD, mr, None, None, None, 0, norms=norms[:N - n_new])
        for _ in range(5):
            eng.cluster_density_extend(emb, THRESHOLD, mr, state[0], state[2], state[3], N - n_new, norms=norms, validate=False)
        torch.cuda.synchronize()
        return
    rows = []
    print('%8s %8s %7s | %10s %10s | %8s %8s | %s' % ('N', 'N_new', 'm', 'extend ms', 'full ms', 'full/ext', 'by pairs',
                                                      'pairs: degree / gated / promoted'))
    for N in [int(s) for s in args.sizes.split(',')]:
        emb, _, _ = planted_bridged(N, seed=N)
        norms = eng.row_norms(emb)
        for n_new in sorted({N // 32, N // 8, N // 2, min(256, N)}):
            n_old = N - n_new
            rep0, _, deg0, best0 = eng.cluster_density_extend(emb[:n_old], THRESHOLD, mr, None, None, None, 0, norms=norms[:n_old])

            def extend():
                return eng.cluster_density_extend(emb, THRESHOLD, mr, rep0, deg0, best0, n_old, norms=norms, validate=False)

            def full():
                return eng.cluster_density(emb, THRESHOLD, mr, norms=norms, return_degree=True)

            got, want = extend(), full()
            for name, g, w in zip(('rep', 'kind', 'degree'), got, want):
                assert torch.equal(g, w), '%s differs at N = %d, N_new = %d' % (name, N, n_new)
            m = int(((deg0 < mr - 1) & (got[2][:n_old] >= mr - 1)).sum())
            (te, tf), spread = timed_alternating([extend, full], args.reps)
            walk = 2 * n_old * n_new + n_new * (n_new - 1)         # both walks together, as pairs scored once each
            pairs = walk + m * n_old
            shares = [walk / 2 / pairs, walk / 2 / pairs, m * n_old / pairs]
            row = dict(N=N, N_new=n_new, N_old=n_old, threshold=THRESHOLD, min_rows=mr, promoted_rows=m, extend_ms=te,
                       extend_ms_min_max=spread[0], full_ms=tf, full_ms_min_max=spread[1], full_over_extend=tf / te,
                       pairs=pairs, full_pairs=N * (N - 1), pair_count_ratio=N * (N - 1) / pairs,
                       pair_share_degree_gated_promoted=shares, labels_equal=True, extension_slower=bool(te > tf))
            rows.append(row)
            print('%8d %8d %7d | %10.3f %10.3f | %8.2f %8.2f | %.3f / %.3f / %.3f%s' % (
                N, n_new, m, te, tf, tf / te, row['pair_count_ratio'], shares[0], shares[1], shares[2],
                '   SLOWER than the full call' if te > tf else ''), flush=True)
        del emb, norms
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, shapes=rows)
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as fjson:
            json.dump(out, fjson, indent=1)


if __name__ == '__main__':
    main()
