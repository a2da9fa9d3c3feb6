"""Time the certified bf16 shortlist search (Engine.search_coarse over a Gallery(coarse=True)'s rows and plane, the call
of its search(): k_search_coarse + k_search_rescore + the exact pass over uncertified probes) against the exact search
(Engine.search) over the same rows, alternately in one process with device events, medians after a warm-up; torch.equal
of both outputs is asserted at every shape.

  python tools/bench_search_coarse.py [--reps N] [--json OUT] [--small]

Two data families: Gaussian rows, and planted identities of about 8 rows (the generator of tools/bench_cluster.py).  Per
shape: ms of each search, the ratio, the certified share of the probes, and the plane read rate of the coarse search
(G*512*2 bytes / t).  Also the cost of enrolment per appended row: row_norms and coarse_pack over 2^20 rows.
Writes profiles/search_coarse_bench.json by default."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd  # noqa: E402
from ffrnet_amd.search import Gallery  # noqa: E402

SHAPES = [(1, 1 << 20, 10), (32, 1 << 20, 10), (256, 1 << 20, 10), (1024, 1 << 20, 10), (256, 4 << 20, 10), (256, 1 << 20, 64)]
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


def gaussian_piece(n, gen):
    return torch.randn((n, 512), device='cuda', generator=gen)


def planted_piece(n, gen):
    """n rows of n/8 identities (sizes vary around 8): (unit centre + 0.02 randn) * uniform(0.5, 2), shuffled"""
    ids = torch.randint(0, max(n // 8, 1), (n,), device='cuda', generator=gen)
    centres = torch.randn((max(n // 8, 1), 512), device='cuda', generator=gen)
    centres /= centres.norm(dim=1, keepdim=True)
    emb = centres[ids] + 0.02 * torch.randn((n, 512), device='cuda', generator=gen)
    emb *= 0.5 + 1.5 * torch.rand((n, 1), device='cuda', generator=gen)
    return emb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'search_coarse_bench.json'))
    ap.add_argument('--small', action='store_true', help='galleries 16 x smaller (a quick check of the tool)')
    args = ap.parse_args()
    shapes = [(Q, G >> 4, k) for Q, G, k in SHAPES] if args.small else SHAPES
    eng = ffrnet_amd.Engine(0)
    gmax = max(G for _, G, _ in shapes)
    out = dict(device=torch.cuda.get_device_name(0), families={})
    for family, piece in (('gaussian', gaussian_piece), ('planted', planted_piece)):
        gen = torch.Generator(device='cuda')
        gen.manual_seed(0)
        gal = Gallery(eng, capacity=gmax, coarse=True)
        for lo in range(0, gmax, PIECE):
            gal.add(piece(min(PIECE, gmax - lo), gen))
        # probes: noisy copies of enrolled rows for the planted family (a probe has an identity), fresh rows otherwise
        qmax = max(Q for Q, _, _ in shapes)
        if family == 'planted':
            pick = torch.randint(0, min(G for _, G, _ in shapes), (qmax,), device='cuda', generator=gen)
            probes = gal.embeddings[pick] + 0.02 * torch.randn((qmax, 512), device='cuda', generator=gen)
        else:
            probes = gaussian_piece(qmax, gen)
        rows = []
        print('%s rows' % family)
        print('%6s %9s %4s | %9s %9s %7s | %9s %9s' % ('Q', 'G', 'k', 'coarse ms', 'exact ms', 'speedup', 'certified', 'plane TB/s'))
        for Q, G, k in shapes:
            q = probes[:Q]
            emb, nrm, sub = gal.embeddings[:G], gal.norms[:G], gal.plane[:G]     # the first G rows: views, no copy

            def coarse():                            # what Gallery.search calls, over the view
                return eng.search_coarse(q, emb, sub, gal.flag, k, gallery_norms=nrm, return_certified=True)

            def exact():
                return eng.search(q, emb, k, gallery_norms=nrm)

            tc, te = timed_alternating([coarse, exact], args.reps)
            s, i, cert = coarse()
            es, ei = exact()
            torch.cuda.synchronize()
            assert torch.equal(s, es) and torch.equal(i, ei), (family, Q, G, k)
            share = float(cert.float().mean().item())
            r = dict(Q=Q, G=G, k=k, coarse_ms=tc, exact_ms=te, speedup=te / tc, certified_share=share,
                     plane_tb_s=G * 512 * 2 / tc / 1e9, equal=True)
            rows.append(r)
            print('%6d %9d %4d | %9.3f %9.3f %6.2fx | %9.3f %9.2f' % (Q, G, k, tc, te, r['speedup'], share, r['plane_tb_s']), flush=True)
        out['families'][family] = rows
        if family == 'gaussian':
            n = min(1 << 20, gmax)
            x, nrm = gal.embeddings[:n], gal.norms[:n]
            plane = torch.empty((n, 512), device='cuda', dtype=torch.int16)
            flag = torch.zeros((1,), device='cuda', dtype=torch.int32)
            tn, tp = timed_alternating([lambda: eng.row_norms(x), lambda: eng.coarse_pack(x, nrm, plane, flag)], args.reps)
            out['enrol'] = dict(rows=n, row_norms_ms=tn, coarse_pack_ms=tp, row_norms_ns_per_row=tn * 1e6 / n,
                                coarse_pack_ns_per_row=tp * 1e6 / n)
            print('enrolment of %d rows: row_norms %.3f ms (%.2f ns/row), coarse_pack %.3f ms (%.2f ns/row)'
                  % (n, tn, tn * 1e6 / n, tp, tp * 1e6 / n))
            del plane
        del gal, probes, emb, nrm, sub
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
