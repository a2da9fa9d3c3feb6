"""Time the certified bf16 shortlist over a subject-labelled gallery (Engine.search_coarse_subjects, the call behind
search_subjects() and search() of a Gallery(subjects=True) after build_plane(): k_search_coarse_live + k_search_rescore +
the exact subject pass over uncertified probes) against the exact subject search (Engine.search_subjects) over the same
rows, alternately in one process with device events, medians after a warm-up; torch.equal of scores, indices and subjects is
asserted at every shape.

  python tools/bench_search_coarse_subjects.py [--reps N] [--json OUT] [--small]

Rows: planted identities of 8 rows each, a person's rows spread over the gallery (subject[g] = g % (G / 8)), rows = centre +
0.5 randn; a probe is centre + 0.5 randn of an enrolled person.  Per gallery size: identity lists at k = 10 and 32, and row
lists at k = 10 under a removal mask (a seeded 10 % of the subjects withdrawn), for 256, 32 and 1 probes.  Per shape: ms of
each search, the ratio, the certified share of the probes.  Writes profiles/search_coarse_subjects_bench.json by default."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd  # noqa: E402
from ffrnet_amd.search import Gallery  # noqa: E402

SIZES = [1 << 20, 1 << 22]
MODES = [('identities', 10), ('identities', 32), ('rows under the mask', 10)]
PROBES = [256, 32, 1]
PER, NOISE, REMOVED = 8, 0.5, 0.1
PIECE = 1 << 19


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
    return [sorted(t)[len(t) // 2] for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'search_coarse_subjects_bench.json'))
    ap.add_argument('--small', action='store_true', help='galleries 16 x smaller (a quick check of the tool)')
    args = ap.parse_args()
    sizes = [G >> 4 for G in SIZES] if args.small else SIZES
    eng = ffrnet_amd.Engine(0)
    out = dict(device=torch.cuda.get_device_name(0), rows_per_subject=PER, noise=NOISE, removed_share_of_subjects=REMOVED, shapes=[])
    print('%20s %4s %6s %9s | %9s %9s %7s | %9s' % ('mode', 'k', 'Q', 'G', 'coarse ms', 'exact ms', 'speedup', 'certified'))
    for G in sizes:
        gen = torch.Generator(device='cuda')
        gen.manual_seed(0)
        nsub = G // PER
        cent = torch.randn((nsub, 512), device='cuda', generator=gen)
        gal = Gallery(eng, capacity=G, subjects=True)
        for lo in range(0, G, PIECE):
            ids = torch.arange(lo, min(lo + PIECE, G), device='cuda') % nsub
            gal.add(cent[ids] + NOISE * torch.randn((ids.numel(), 512), device='cuda', generator=gen), ids)
        gal.build_plane()
        pick = torch.randperm(nsub, device='cuda', generator=gen)[:max(PROBES)]
        probes = cent[pick] + NOISE * torch.randn((pick.numel(), 512), device='cuda', generator=gen)
        del cent
        whole = gal.subjects.clone()
        gone = torch.randperm(nsub, device='cuda', generator=gen)[:int(REMOVED * nsub)].to(torch.int32)
        masked = whole.clone()
        masked[torch.isin(whole, gone)] = -1
        emb, nrm, plane = gal.embeddings, gal.norms, gal.plane
        for mode, k in MODES:
            distinct = mode == 'identities'
            subj = whole if distinct else masked
            for Q in PROBES:
                q = probes[:Q]

                def coarse():                        # what the Gallery's searches call
                    return eng.search_coarse_subjects(q, emb, plane, gal.flag, subj, k, gallery_norms=nrm, distinct=distinct,
                                                      return_certified=True)

                def exact():
                    return eng.search_subjects(q, emb, subj, k, gallery_norms=nrm, distinct=distinct)

                tc, te = timed_alternating([coarse, exact], args.reps)
                got, want = coarse(), exact()
                torch.cuda.synchronize()
                assert all(torch.equal(a, b) for a, b in zip(got[:3], want)), (mode, k, Q, G)
                share = float(got[3].float().mean().item())
                r = dict(mode=mode, k=k, Q=Q, G=G, coarse_ms=tc, exact_ms=te, speedup=te / tc, certified_share=share, equal=True)
                out['shapes'].append(r)
                print('%20s %4d %6d %9d | %9.3f %9.3f %6.2fx | %9.3f' % (mode, k, Q, G, tc, te, r['speedup'], share), flush=True)
        del gal, probes, emb, nrm, plane, whole, masked
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
