"""Time the subject-labelled search (Engine.search_subjects: k_row_norms + k_search_subjects + k_topk_merge_subjects) with
device events after a warm-up, against Engine.search IN THE SAME RUN on the same inputs (machines differ by more than the
effect), and against today's workaround for an identity list: Engine.search(k=128) followed by a torch de-duplication.

  python tools/bench_search_subjects.py [--reps N] [--json OUT]

The gallery holds about 8 rows per subject, a subject's rows scattered round one centre (enrolments of one person score
alike, so a row list repeats people).  Per shape: ms of the plain row search, of the identity search, of the row search under
a removal mask (5 % of the subjects withdrawn), of the workaround, the ratios to the plain search, and the number of probes
whose workaround list differs from the identity search (128 rows do not always hold k people).  Both searches are checked
against the restatement of tests/search_subjects_ref.py on a few probes."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ffrnet_amd  # noqa: E402
import search_subjects_ref as ref  # noqa: E402

SHAPES = [(256, 1 << 20, 10), (1, 1 << 20, 10), (256, 4 << 20, 10), (256, 1 << 20, 64)]
ROWS_PER_SUBJECT = 8
SPREAD = 0.5


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def make_gallery(G, gen):
    """rows [G,512] = the centre of subject row // 8 + SPREAD * noise, built in blocks; subjects [G] int32"""
    gall = torch.empty((G, 512), device='cuda')
    nsub = (G + ROWS_PER_SUBJECT - 1) // ROWS_PER_SUBJECT
    centres = torch.randn((nsub, 512), device='cuda', generator=gen)
    subj = (torch.arange(G, device='cuda') // ROWS_PER_SUBJECT).to(torch.int32)
    step = 1 << 18
    for lo in range(0, G, step):
        n = min(step, G - lo)
        gall[lo:lo + n] = centres[subj[lo:lo + n].long()] + SPREAD * torch.randn((n, 512), device='cuda', generator=gen)
    return gall, subj, centres


def dedup(s, i, subj, k):
    """The workaround: row lists [Q,128] -> the first k distinct subjects of every list, (-inf, -1, -1) where 128 rows hold
    fewer."""
    Q, n = i.shape
    u = subj[i.clamp(min=0)]
    u = torch.where(i >= 0, u, torch.full_like(u, -1))
    first = ~torch.tril(u[:, :, None] == u[:, None, :], -1).any(2) & (i >= 0)
    rank = first.cumsum(1) - 1
    pos = torch.where(first & (rank < k), rank, torch.full_like(rank, k))
    out_s = torch.full((Q, k + 1), float('-inf'), device=s.device)
    out_i = torch.full((Q, k + 1), -1, device=s.device, dtype=torch.int64)
    out_u = torch.full((Q, k + 1), -1, device=s.device, dtype=torch.int32)
    out_s.scatter_(1, pos, s)
    out_i.scatter_(1, pos, i)
    out_u.scatter_(1, pos, u)
    return out_s[:, :k], out_i[:, :k], out_u[:, :k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    eng = ffrnet_amd.Engine(0)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    Gmax, Qmax = max(G for _, G, _ in SHAPES), max(Q for Q, _, _ in SHAPES)
    gall, subj_all, centres = make_gallery(Gmax, gen)
    who = torch.randint(0, (1 << 20) // ROWS_PER_SUBJECT, (Qmax,), device='cuda', generator=gen)
    probes = centres[who] + SPREAD * torch.randn((Qmax, 512), device='cuda', generator=gen)
    del centres
    norms_all = eng.row_norms(gall)
    rows = []
    print('%5s %8s %3s | %8s | %8s %6s | %8s %6s | %8s %6s %5s' % ('Q', 'G', 'k', 'rows ms', 'ident ms', 'ratio', 'masked', 'ratio',
                                                                      'workard', 'ratio', 'wrong'))
    for Q, G, k in SHAPES:
        q, g, n, subj = probes[:Q], gall[:G], norms_all[:G], subj_all[:G]
        masked = subj.clone()
        masked[(subj % 20) == 7] = -1                         # 5 % of the subjects withdrawn
        t_rows = timed(lambda: eng.search(q, g, k, gallery_norms=n), args.reps)
        t_id = timed(lambda: eng.search_subjects(q, g, subj, k, gallery_norms=n, distinct=True), args.reps)
        t_mask = timed(lambda: eng.search_subjects(q, g, masked, k, gallery_norms=n, distinct=False), args.reps)
        t_rows2 = timed(lambda: eng.search(q, g, k, gallery_norms=n), args.reps)        # again: drift within the run

        def workaround():
            s, i = eng.search(q, g, 128, gallery_norms=n)
            return dedup(s, i, subj, k)
        t_wa = timed(workaround, args.reps)
        s, i, u = eng.search_subjects(q, g, subj, k, gallery_norms=n, distinct=True)
        ws, wi, wu = workaround()
        wrong = int((~((ws == s).all(1) & (wi == i).all(1) & (wu == u).all(1))).sum().item())
        # both modes against the restatement on the first probes, from the scores of the plain search at k = 128 per 128 rows
        np_, Gc = min(Q, 2), min(G, 1 << 16)
        S = torch.empty((np_, Gc), device='cuda')
        for lo in range(0, Gc, 128):
            ps, pi = eng.search(q[:np_], g[lo:lo + 128], 128, gallery_norms=n[lo:lo + 128], index_base=lo)
            S.scatter_(1, pi, ps)
        ok = True
        for distinct, sub in ((True, subj), (False, masked)):
            got = eng.search_subjects(q[:np_], g[:Gc], sub[:Gc], k, gallery_norms=n[:Gc], distinct=distinct)
            want = ref.search_ref(S.cpu().numpy(), sub[:Gc].cpu().numpy(), k, distinct)
            ok = ok and all(torch.equal(a.cpu(), torch.from_numpy(b)) for a, b in zip(got, want))
        base = 0.5 * (t_rows + t_rows2)
        r = dict(Q=Q, G=G, k=k, rows_per_subject=ROWS_PER_SUBJECT, search_ms=t_rows, search_again_ms=t_rows2, identity_ms=t_id,
                 masked_rows_ms=t_mask, workaround_ms=t_wa, identity_over_search=t_id / base, masked_over_search=t_mask / base,
                 workaround_over_search=t_wa / base, identity_over_workaround=t_id / t_wa, workaround_wrong_probes=wrong,
                 exact_on_first_probes=bool(ok))
        rows.append(r)
        print('%5d %8d %3d | %8.3f | %8.3f %6.3f | %8.3f %6.3f | %8.3f %6.3f %5d %s' % (
            Q, G, k, base, t_id, r['identity_over_search'], t_mask, r['masked_over_search'], t_wa, r['workaround_over_search'],
            wrong, 'ok' if ok else 'MISMATCH'), flush=True)
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, shapes=rows)
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
    assert all(r['exact_on_first_probes'] for r in rows)


if __name__ == '__main__':
    main()
