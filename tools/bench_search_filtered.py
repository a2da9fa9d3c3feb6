"""Time the filtered search (Engine.search_filtered: k_row_norms + k_search_filtered + the merge) with device events after a
warm-up of every shape, IN THE SAME RUN (machines differ by more than the effect) against

  (a) the unfiltered search of the same gallery, Engine.search / Engine.search_subjects: what the filter costs;
  (b) the workaround that is correct: per distinct mask, boolean-index compaction of the admissible rows (and their norms
      and subjects) and one search of the compacted rows for the probes that carry the mask, the copies timed with it.

  python tools/bench_search_filtered.py [--reps N] [--json OUT]

The gallery is that of tools/bench_search_subjects.py (about 8 rows per person).  A batch carries 8 distinct masks, probe q
bit q % 8 (one mask at Q = 1); a tag gets each of the 8 bits with probability `share`, per row in row mode and per person in
identity mode, so every mask admits about that share of the gallery.  The three routes alternate within every repetition;
medians with p10 / p90.  Before timing, the filtered lists are compared bit for bit with route (b), indices mapped back, for
every probe, and at share 1 with route (a)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd  # noqa: E402
from bench_search_subjects import ROWS_PER_SUBJECT, SPREAD, make_gallery  # noqa: E402

SHAPES = [(256, 1 << 20), (32, 1 << 20), (1, 1 << 20), (256, 1 << 22)]
SHARES = [1.0, 1.0 / 2, 1.0 / 32, 1.0 / 1024]
K = 10
NMASK = 8


def spread(ts):
    ts = sorted(ts)
    n = len(ts)
    return dict(median=ts[n // 2], p10=ts[int(0.1 * (n - 1) + 0.5)], p90=ts[int(0.9 * (n - 1) + 0.5)])


def timed_alternating(fns, reps):
    """every fn once to warm up, then reps rounds that time each fn in turn -> one list of ms per fn"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = [[] for _ in fns]
    for _ in range(reps):
        for j, fn in enumerate(fns):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[j].append(e0.elapsed_time(e1))
    return ts


def make_tags(G, subj, share, per_subject, gen):
    """int32 [G]: each of the bits 0..7 set with probability `share`, per row or per subject"""
    n = int(subj.max().item()) + 1 if per_subject else G
    w = torch.zeros((n,), device='cuda', dtype=torch.int32)
    for b in range(NMASK):
        w |= (torch.rand((n,), device='cuda', generator=gen) < share).to(torch.int32) << b
    return w[subj.long()] if per_subject else w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    eng = ffrnet_amd.Engine(0)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    Gmax, Qmax = max(G for _, G in SHAPES), max(Q for Q, _ in SHAPES)
    gall, subj_all, centres = make_gallery(Gmax, gen)
    who = torch.randint(0, (1 << 20) // ROWS_PER_SUBJECT, (Qmax,), device='cuda', generator=gen)
    probes = centres[who] + SPREAD * torch.randn((Qmax, 512), device='cuda', generator=gen)
    del centres
    norms_all = eng.row_norms(gall)
    rows = []
    print('%5s %8s %5s %7s | %9s | %9s %6s | %9s %6s' % ('Q', 'G', 'mode', 'share', 'plain ms', 'filter ms', 'f / a', 'compact', 'f / b'))
    for Q, G in SHAPES:
        q, g, n, subj = probes[:Q], gall[:G], norms_all[:G], subj_all[:G]
        mask = (1 << (torch.arange(Q, device='cuda') % NMASK)).to(torch.int32)
        groups = [(int(m), (mask == m).nonzero().reshape(-1)) for m in torch.unique(mask).tolist()]
        for ident in (False, True):
            sub = subj if ident else None
            for share in SHARES:
                tag = make_tags(G, subj, share, ident, gen)

                def plain():
                    if ident:
                        return eng.search_subjects(q, g, subj, K, gallery_norms=n, distinct=True)
                    return eng.search(q, g, K, gallery_norms=n)

                def filtered():
                    return eng.search_filtered(q, mask, g, tag, K, gallery_norms=n, subjects=sub, distinct=ident)

                def compact():
                    out = [torch.empty((Q, K), device='cuda'), torch.empty((Q, K), device='cuda', dtype=torch.int64)]
                    if ident:
                        out.append(torch.empty((Q, K), device='cuda', dtype=torch.int32))
                    for m, pq in groups:
                        idx = ((tag & m) != 0).nonzero().reshape(-1)
                        gm, nm = g[idx], n[idx]
                        if ident:
                            got = eng.search_subjects(q[pq], gm, subj[idx], K, gallery_norms=nm, distinct=True)
                        else:
                            got = eng.search(q[pq], gm, K, gallery_norms=nm)
                        got = list(got)
                        got[1] = torch.where(got[1] >= 0, idx[got[1].clamp(min=0)] if idx.numel() else got[1], got[1])
                        for o, x in zip(out, got):
                            o[pq] = x
                    return tuple(out)

                f, b = filtered(), compact()
                eq_b = all(torch.equal(x, y) for x, y in zip(f, b))
                eq_a = all(torch.equal(x, y) for x, y in zip(f, plain())) if share == 1.0 else None
                assert eq_b and eq_a is not False, (Q, G, ident, share, eq_b, eq_a)
                del f, b
                ta, tf, tb = [spread(t) for t in timed_alternating((plain, filtered, compact), args.reps)]
                adm = float(sum(((tag & m) != 0).float().mean().item() for m, _ in groups) / len(groups))
                r = dict(Q=Q, G=G, k=K, mode='identities' if ident else 'rows', share=share, admissible_share=adm,
                         distinct_masks=len(groups), unfiltered_ms=ta, filtered_ms=tf, compact_ms=tb,
                         filtered_over_unfiltered=tf['median'] / ta['median'], filtered_over_compact=tf['median'] / tb['median'],
                         equal_to_compact=bool(eq_b), equal_to_unfiltered=eq_a)
                rows.append(r)
                print('%5d %8d %5s %7.5f | %9.3f | %9.3f %6.3f | %9.3f %6.3f' % (
                    Q, G, 'ident' if ident else 'rows', adm, ta['median'], tf['median'], r['filtered_over_unfiltered'], tb['median'],
                    r['filtered_over_compact']), flush=True)
                torch.cuda.empty_cache()
    slower = [dict(Q=r['Q'], G=r['G'], mode=r['mode'], share=r['share'], filtered_over_compact=r['filtered_over_compact'])
              for r in rows if r['filtered_over_compact'] > 1.0]
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows_per_subject=ROWS_PER_SUBJECT, shapes=rows,
               filtered_slower_than_compact=slower)
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
