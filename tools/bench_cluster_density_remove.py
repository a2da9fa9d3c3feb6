"""Time the removal of rows from a density-gated clustering (Engine.cluster_density_remove: the removed rows against all
rows, the still-core rows of the hit clusters among themselves, the rows that choose again against all rows, then root,
min, label) against clustering the compacted survivors again, on the bridged planted identities of
tools/bench_cluster_density.py at min_rows = 4, with device events after a warm-up, the calls interleaved in one process.

  python tools/bench_cluster_density_remove.py [--reps N] [--json OUT] [--sizes 16384,131072] [--lib PATH]

Per total N the removal patterns: the oldest n rows for n = 256, 4096, 16384 and N / 2 (a sliding window expires), and 256
random rows (deletions).  The rows are clustered once (Engine.cluster_density_extend from nothing, which leaves the state);
per pattern the removal's labels and state, compacted and the keys re-encoded, are held equal to Engine.cluster_density and
to the state from scratch over the compacted rows BEFORE any time is printed.  Printed per shape: r, m and q (the lengths
of the three device lists, computed here from the states and the mask: the call reads nothing back), ms of the removal, of
Engine.cluster_density over the survivors, of Engine.cluster_density_extend(n_old = 0) over the survivors (the other route
of IncrementalDensity.remove, which must leave the state too) and of the compaction copy emb[keep] (timed apart, in none of
the figures; both routes of the store compact), the ratio again / remove next to the ratio of the pair counts
N_s (N_s - 1) / ((r + q) N + m (m - 1) / 2) it should approach, and the route cluster.density_remove_route takes.  The
removal works on copies of the state (three N-sized clones inside its figure).  Shapes where the removal is slower are
marked.  --lib: another build of the library (the SPAN_STEPS / BLOCKS_PER_CU candidates of EXPERIMENTS.md).  Writes
profiles/cluster_density_remove_bench.json by default."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ffrnet_amd  # noqa: E402
from ffrnet_amd import cluster as fc  # noqa: E402
from ffrnet_amd import native  # noqa: E402
from bench_cluster import THRESHOLD, timed_alternating  # noqa: E402
from bench_cluster_density import planted_bridged  # noqa: E402

MIN_ROWS = 4


def list_lengths(before, after_degree, keep, min_rows):
    """(r, m, q) as include/ffrnet.h defines them, from the state before (rep, kind, degree, best), the degrees after, the mask"""
    rep, _, deg0, best = before
    need = min_rows - 1
    was_core = deg0 >= need
    core = keep & (after_degree >= need)
    hit = torch.zeros_like(keep)
    hit[rep[was_core & ~core]] = True
    named = torch.where(best != 0, 0xFFFFFFFF - (best & 0xFFFFFFFF), torch.zeros_like(best))
    holds = (best != 0) & keep[named] & core[named]
    again = keep & ~core & (was_core | ((best != 0) & ~holds))
    return int((~keep).sum()), int((core & hit[rep]).sum()), int(again.sum())


def compacted(got, keep):
    old_to_new = torch.full((keep.numel(),), -1, device=keep.device, dtype=torch.int64)
    old_to_new[keep] = torch.arange(int(keep.sum()), device=keep.device, dtype=torch.int64)
    return old_to_new[got[0][keep]], got[1][keep], got[2][keep], fc._rekey(got[3][keep], old_to_new)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sizes', default='16384,131072')
    ap.add_argument('--lib', default=None)
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'cluster_density_remove_bench.json'))
    args = ap.parse_args()
    if args.lib:
        native.set_library(args.lib)
    eng = ffrnet_amd.Engine(0)
    rows = []
    print('%8s %14s %8s %8s %8s | %10s %10s %10s %8s | %9s %9s | %s' % (
        'N', 'removed', 'N_s', 'm', 'q', 'remove ms', 'again ms', 'state ms', 'copy ms', 'again/rem', 'by pairs', 'route'))
    for N in [int(s) for s in args.sizes.split(',')]:
        emb, _, _ = planted_bridged(N, seed=N)
        norms = eng.row_norms(emb)
        before = eng.cluster_density_extend(emb, THRESHOLD, MIN_ROWS, None, None, None, 0, norms=norms)
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
                return eng.cluster_density_remove(emb, THRESHOLD, MIN_ROWS, before[0].clone(), before[2].clone(), before[3].clone(),
                                                  keep, norms=norms, validate=False)

            def again():
                return eng.cluster_density(survivors, THRESHOLD, MIN_ROWS, norms=s_norms, return_degree=True)

            def again_state():
                return eng.cluster_density_extend(survivors, THRESHOLD, MIN_ROWS, None, None, None, 0, norms=s_norms, validate=False)

            def copy():
                return emb[keep]

            got, want, state = remove(), again(), again_state()
            c = compacted(got, keep)
            for what, g, w in zip(('rep', 'kind', 'degree', 'best'), c, want + (state[3],)):
                assert torch.equal(g, w), '%s differs at N = %d, %s' % (what, N, name)
            assert bool((got[0][~keep] == -1).all()) and not bool(got[3][~keep].any())
            r, m, q = list_lengths(before, got[2], keep, MIN_ROWS)
            (tr, ta, ts, tc), spread = timed_alternating([remove, again, again_state, copy], args.reps)
            pairs, full_pairs = (r + q) * N + m * (m - 1) // 2, n_s * (n_s - 1)      # the survivors' triangle is walked twice
            route = fc.density_remove_route(N, n_s)
            row = dict(N=N, pattern=name, removed=r, survivors=n_s, threshold=THRESHOLD, min_rows=MIN_ROWS, r=r, m=m, q=q,
                       remove_ms=tr, remove_ms_min_max=spread[0], again_ms=ta, again_ms_min_max=spread[1], again_state_ms=ts,
                       again_state_ms_min_max=spread[2], copy_ms=tc, copy_ms_min_max=spread[3], again_over_remove=ta / tr,
                       again_state_over_remove=ts / tr, pairs=pairs, again_pairs=full_pairs, pair_count_ratio=full_pairs / pairs,
                       remove_gpairs_per_s=pairs / tr / 1e6, again_gpairs_per_s=full_pairs / ta / 1e6, state_equal=True,
                       removal_slower=bool(tr > min(ta, ts)), route=route, host_pair_ratio=r * N / full_pairs)
            rows.append(row)
            print('%8d %14s %8d %8d %8d | %10.3f %10.3f %10.3f %8.3f | %9.2f %9.2f | %s%s' % (
                N, name, n_s, m, q, tr, ta, ts, tc, ta / tr, row['pair_count_ratio'], route,
                '   SLOWER than clustering again' if row['removal_slower'] else ''), flush=True)
            del survivors, s_norms
        del emb, norms, before
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, remove_pair_ratio=fc.REMOVE_PAIR_RATIO, shapes=rows)
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as fjson:
            json.dump(out, fjson, indent=1)


if __name__ == '__main__':
    main()
