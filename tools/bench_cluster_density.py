"""Time the density-gated clustering (Engine.cluster_density: k_row_norms + k_density_init + k_cluster_walk twice, degree
and gated join, + k_density_root / _min / _label) against the single-link clustering (Engine.cluster) over the same rows
in the same run, with device events after a warm-up.

  python tools/bench_cluster_density.py [--reps N] [--json OUT] [--sizes 16384,131072] [--min-rows 4]

Data: the planted identities of tools/bench_cluster.py (about 8 rows each) of which N // 256 pairs are bridged: the two
centres lie at plane angles 0 and 5 theta (theta = arccos 0.8) of a random plane, and four unit rows at theta .. 4 theta
form a chain of consecutive cosine 0.8 between them.  The rows at theta and 4 theta are dense (they score about 0.73 with
every member of the identity next to them), the two in the middle have two neighbours each.  Truth: the chain rows
belong to the nearer identity.  Single link merges each bridged pair; at min_rows = 4 the middle rows are border rows.

Both calls are timed alternately, the median of --reps calls each.  Per size: ms of both, their ratio (two walks of the
triangle predict about 2), the TFLOP/s of both as the library's profile counts them (ffr_profile_read: 2 N (N - 1) 512
FLOP for the density call), the kinds, and pairwise_scores of both clusterings against the planted truth.  Writes
profiles/cluster_density_bench.json by default."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd  # noqa: E402
from ffrnet_amd import cluster as fc  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_cluster import PEAK_TFLOPS, THRESHOLD, timed_alternating  # noqa: E402


def planted_bridged(N, seed):
    """-> (emb[N,512], truth[N], n_bridged_pairs), see the module docstring"""
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    n_id, P = max(N // 8, 2), N // 256
    body = N - 4 * P
    ids = torch.sort(torch.randint(0, n_id, (body,), device='cuda', generator=gen)).values
    centres = torch.randn((n_id, 512), device='cuda', generator=gen)
    centres /= centres.norm(dim=1, keepdim=True)
    theta = math.acos(0.8)
    a = centres[0:2 * P:2].clone()
    v = centres[1:2 * P:2] - (centres[1:2 * P:2] * a).sum(1, keepdim=True) * a
    v /= v.norm(dim=1, keepdim=True)
    centres[1:2 * P:2] = math.cos(5 * theta) * a + math.sin(5 * theta) * v
    emb = centres[ids] + 0.02 * torch.randn((body, 512), device='cuda', generator=gen)
    emb *= 0.5 + 1.5 * torch.rand((body, 1), device='cuda', generator=gen)
    chain = torch.cat([math.cos(k * theta) * a + math.sin(k * theta) * v for k in (1, 2, 3, 4)])
    pair = torch.arange(P, device='cuda')
    chain_ids = torch.cat((2 * pair, 2 * pair, 2 * pair + 1, 2 * pair + 1))
    emb, ids = torch.cat((emb, chain)), torch.cat((ids, chain_ids))
    perm = torch.randperm(N, device='cuda', generator=gen)
    return emb[perm].contiguous(), ids[perm].contiguous(), P


def profiled_tflops(eng, fn):
    """TFLOP/s of one call as the library counts and times it (class 'score')"""
    torch.cuda.synchronize()
    eng.profile_enable(True)
    eng.profile_read()
    fn()
    st = eng.profile_read()['score']
    eng.profile_enable(False)
    return st['flops'] / st['ms'] / 1e9, st['ms']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sizes', default='16384,131072')
    ap.add_argument('--min-rows', type=int, default=4)
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'cluster_density_bench.json'))
    args = ap.parse_args()
    eng = ffrnet_amd.Engine(0)
    m = args.min_rows
    rows = []
    print('%8s | %10s %8s | %10s %8s | %6s | %22s | %s' % ('N', 'density ms', 'TFLOP/s', 'single ms', 'TFLOP/s', 'ratio',
                                                          'core / border / noise', 'pairwise f: density, single link'))
    for N in [int(s) for s in args.sizes.split(',')]:
        emb, ids, P = planted_bridged(N, seed=N)
        norms = eng.row_norms(emb)

        def density():
            return eng.cluster_density(emb, THRESHOLD, m, norms=norms)

        def single():
            return eng.cluster(emb, THRESHOLD, norms=norms)

        (td, ts), spread = timed_alternating([density, single], args.reps)
        tf_d, ms_d = profiled_tflops(eng, density)
        tf_s, ms_s = profiled_tflops(eng, single)
        rep_d, kind = density()
        rep_s = single()
        again = density()
        kinds = torch.bincount(kind.long(), minlength=3).tolist()
        cd, cs = fc.density_ids(rep_d, kind), fc.dense_ids(rep_s)
        row = dict(N=N, threshold=THRESHOLD, min_rows=m, bridged_pairs=P, density_ms=td, density_ms_min_max=spread[0],
                   single_link_ms=ts, single_link_ms_min_max=spread[1], density_over_single_link=td / ts,
                   density_profiled_ms=ms_d, density_tflops=tf_d, density_frac_fp32_mfma_peak=tf_d / PEAK_TFLOPS,
                   single_link_profiled_ms=ms_s, single_link_tflops=tf_s, single_link_frac_fp32_mfma_peak=tf_s / PEAK_TFLOPS,
                   noise_border_core=kinds, density_clusters=cd.n_clusters, density_clusters_with_core=int(cd.has_core.sum()),
                   single_link_clusters=cs.n_clusters,
                   density_pairwise_precision_recall_f=list(fc.pairwise_scores(cd.cluster_id, ids)),
                   single_link_pairwise_precision_recall_f=list(fc.pairwise_scores(cs.cluster_id, ids)),
                   repeatable=bool(torch.equal(again[0], rep_d) and torch.equal(again[1], kind)))
        rows.append(row)
        print('%8d | %10.3f %8.1f | %10.3f %8.1f | %6.2f | %22s | %.4f, %.4f' % (
            N, td, tf_d, ts, tf_s, td / ts, '%d / %d / %d' % (kinds[2], kinds[1], kinds[0]),
            row['density_pairwise_precision_recall_f'][2], row['single_link_pairwise_precision_recall_f'][2]), flush=True)
        del emb, ids, norms
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), peak_tflops=PEAK_TFLOPS, reps=args.reps, sizes=rows)
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as fjson:
            json.dump(out, fjson, indent=1)
    assert all(r['repeatable'] for r in rows)


if __name__ == '__main__':
    main()
