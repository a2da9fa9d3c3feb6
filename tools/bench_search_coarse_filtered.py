"""Time the filtered search through the certified bf16 shortlist (Engine.search_coarse_filtered: k_row_norms +
k_search_coarse_filtered + the merge + k_search_rescore + the exact pass over the uncertified probes) with device events
after a warm-up of every shape, IN THE SAME RUN (machines differ by more than the effect) against the exact filtered search,
Engine.search_filtered, of the same gallery, tags and masks.

  python tools/bench_search_coarse_filtered.py [--reps N] [--json OUT]

The grid is that of tools/bench_search_filtered.py: its gallery (about 8 rows per person), k = 10, a batch carries 8 distinct
masks, probe q bit q % 8 (one mask at Q = 1); a tag gets each of the 8 bits with probability `share`, per row in row mode and
per person in identity mode.  The two routes alternate within every repetition; medians with p10 / p90.  Before timing, every
output of the shortlist route is compared bit for bit with the exact route; the certified share of the batch is reported."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd  # noqa: E402
from bench_search_filtered import K, NMASK, SHAPES, SHARES, make_tags, spread, timed_alternating  # noqa: E402
from bench_search_subjects import ROWS_PER_SUBJECT, SPREAD, make_gallery  # noqa: E402


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
    plane_all = torch.empty((Gmax, 512), device='cuda', dtype=torch.int16)
    flag = torch.zeros((1,), device='cuda', dtype=torch.int32)
    eng.coarse_pack(gall, norms_all, plane_all, flag)
    assert int(flag.item()) == 0
    rows = []
    print('%5s %8s %5s %7s | %9s | %9s %9s | %s' % ('Q', 'G', 'mode', 'share', 'exact ms', 'short ms', 'exact / s', 'certified'))
    for Q, G in SHAPES:
        q, g, n, subj, plane = probes[:Q], gall[:G], norms_all[:G], subj_all[:G], plane_all[:G]
        mask = (1 << (torch.arange(Q, device='cuda') % NMASK)).to(torch.int32)
        for ident in (False, True):
            sub = subj if ident else None
            for share in SHARES:
                tag = make_tags(G, subj, share, ident, gen)

                def exact():
                    return eng.search_filtered(q, mask, g, tag, K, gallery_norms=n, subjects=sub, distinct=ident)

                def short():
                    return eng.search_coarse_filtered(q, mask, g, plane, flag, tag, K, gallery_norms=n, subjects=sub, distinct=ident,
                                                      return_certified=True)

                e, s = exact(), short()
                assert len(s) == len(e) + 1 and all(torch.equal(x, y) for x, y in zip(s, e)), (Q, G, ident, share)
                cert = float(s[-1].float().mean().item())
                del e, s
                te, ts = [spread(t) for t in timed_alternating((exact, short), args.reps)]
                adm = float(sum(((tag & int(m)) != 0).float().mean().item() for m in torch.unique(mask).tolist()) / len(torch.unique(mask)))
                r = dict(Q=Q, G=G, k=K, mode='identities' if ident else 'rows', share=share, admissible_share=adm,
                         distinct_masks=int(torch.unique(mask).numel()), certified_share=cert, exact_filtered_ms=te,
                         shortlist_filtered_ms=ts, exact_over_shortlist=te['median'] / ts['median'], equal=True)
                rows.append(r)
                print('%5d %8d %5s %7.5f | %9.3f | %9.3f %9.3f | %.3f' % (
                    Q, G, 'ident' if ident else 'rows', adm, te['median'], ts['median'], r['exact_over_shortlist'], cert), flush=True)
                torch.cuda.empty_cache()
    slower = [dict(Q=r['Q'], G=r['G'], mode=r['mode'], share=r['share'], exact_over_shortlist=r['exact_over_shortlist'])
              for r in rows if r['exact_over_shortlist'] < 1.0]
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows_per_subject=ROWS_PER_SUBJECT, shapes=rows,
               SHORTLIST_SLOWER_THAN_EXACT=slower)
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
