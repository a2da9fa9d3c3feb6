"""Time the removal of rows from a single-link clustering (Engine.cluster_remove: mark, list, k_list_walk over the pairs
of the listed rows, flatten) against the only other correct way, compacting the survivors and clustering them again
(Engine.cluster over emb[keep]), on the bridged planted identities of tools/bench_cluster_density.py, with device events
after a warm-up, the two calls interleaved in one process.

  python tools/bench_cluster_remove.py [--reps N] [--json OUT] [--sizes 16384,131072]

Per total N the removal patterns: the oldest n rows for n = 256, 4096, 16384 and N / 2 (a sliding window expires; n = N,
which leaves no survivor and nothing to time, is left out), and 256 random rows (deletions).  The rows are clustered once; per pattern the labels of the removal, compacted, are held equal to
Engine.cluster over the compacted rows BEFORE any time is printed, and: m (the survivors of the clusters that lost a row:
the rows whose pairs the removal scores, computed from the labels and the mask as the header describes), ms of the removal,
of clustering the survivors again and of the compaction copy emb[keep] that the second route also needs (timed apart, not
part of either figure), the ratio again / remove next to the ratio of the pair counts N_s (N_s - 1) / m (m - 1) it should
approach, and the pair rate of both (pairs scored per second, from m read back, since the library's profile records no
flops for the removal).  Shapes where the removal is slower than clustering again are marked.  Writes
profiles/cluster_remove_bench.json by default."""
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


def affected_rows(rep, keep):
    """m: the surviving rows whose cluster lost a row"""
    hit = torch.zeros_like(keep)
    hit[rep[~keep]] = True
    return int((keep & hit[rep]).sum())


def compact_labels(rep, keep):
    old_to_new = torch.full((keep.numel(),), -1, device=keep.device, dtype=torch.int64)
    old_to_new[keep] = torch.arange(int(keep.sum()), device=keep.device, dtype=torch.int64)
    return old_to_new[rep[keep]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sizes', default='16384,131072')
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'cluster_remove_bench.json'))
    args = ap.parse_args()
    eng = ffrnet_amd.Engine(0)
    rows = []
    print('%8s %14s %8s %8s | %10s %10s %8s | %9s %9s | %s' % ('N', 'removed', 'N_s', 'm', 'remove ms', 'again ms', 'copy ms',
                                                               'again/rem', 'by pairs', 'Gpairs/s: remove / again'))
    for N in [int(s) for s in args.sizes.split(',')]:
        emb, _, _ = planted_bridged(N, seed=N)
        norms = eng.row_norms(emb)
        rep = eng.cluster(emb, THRESHOLD, norms=norms)
        gen = torch.Generator(device='cuda')
        gen.manual_seed(N + 1)
        patterns = [('oldest %d' % n, torch.arange(n, device='cuda')) for n in sorted({256, 4096, 16384, N // 2}) if n < N]
        patterns.append(('random 256', torch.randperm(N, device='cuda', generator=gen)[:256]))
        for name, gone in patterns:
            keep = torch.ones(N, device='cuda', dtype=torch.bool)
            keep[gone] = False
            n_s = int(keep.sum())
            survivors, s_norms = emb[keep].contiguous(), norms[keep].contiguous()

            def remove():
                return eng.cluster_remove(emb, THRESHOLD, rep, keep, norms=norms, validate=False)

            def again():
                return eng.cluster(survivors, THRESHOLD, norms=s_norms)

            def copy():
                return emb[keep]

            got, want = remove(), again()
            assert torch.equal(compact_labels(got, keep), want), 'labels differ at N = %d, %s' % (N, name)
            assert bool((got[~keep] == -1).all())
            m = affected_rows(rep, keep)
            (tr, ta, tc), spread = timed_alternating([remove, again, copy], args.reps)
            pairs, full_pairs = m * (m - 1), n_s * (n_s - 1)
            row = dict(N=N, pattern=name, removed=int(gone.numel()), survivors=n_s, threshold=THRESHOLD, affected_rows=m,
                       remove_ms=tr, remove_ms_min_max=spread[0], again_ms=ta, again_ms_min_max=spread[1], copy_ms=tc,
                       copy_ms_min_max=spread[2], again_over_remove=ta / tr, again_plus_copy_over_remove=(ta + tc) / tr,
                       pairs=pairs, again_pairs=full_pairs, pair_count_ratio=full_pairs / pairs if pairs else None,
                       remove_gpairs_per_s=pairs / 2 / tr / 1e6, again_gpairs_per_s=full_pairs / 2 / ta / 1e6,
                       labels_equal=True, removal_slower=bool(tr > ta))
            rows.append(row)
            print('%8d %14s %8d %8d | %10.3f %10.3f %8.3f | %9.2f %9s | %.2f / %.2f%s' % (
                N, name, n_s, m, tr, ta, tc, ta / tr, '%.2f' % row['pair_count_ratio'] if pairs else '-',
                row['remove_gpairs_per_s'], row['again_gpairs_per_s'], '   SLOWER than clustering again' if tr > ta else ''),
                flush=True)
            del survivors, s_norms
        del emb, norms
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, shapes=rows)
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as fjson:
            json.dump(out, fjson, indent=1)


if __name__ == '__main__':
    main()
