"""A torch-CPU model of the certified bf16 shortlist search (include/ffrnet.h: ffr_search_topk_coarse), for the tests: the
plane, the split probe, the coarse score, the shortlist, the certificate and the fallback, each by its definition.  It shares
the two rules of the method with the product (ffrnet_amd.search.COARSE_EPS, shortlist_size) and nothing else."""
import torch

from ffrnet_amd.search import COARSE_EPS, shortlist_size


def bf16(x):
    """Round to nearest even to 8 significant bits, as fp32."""
    return x.to(torch.bfloat16).to(torch.float32)


def unit(x, norms):
    return torch.where(norms[:, None] > 0, x / norms[:, None].clamp_min(1e-45), torch.zeros_like(x))


def norms32(x):
    return (x * x).sum(1).sqrt()


def exact_scores(q, g):
    """fp32 s = q.g / (|q||g| + 1e-8), [Q,G]."""
    return (q @ g.T) / (norms32(q)[:, None] * norms32(g)[None, :] + 1e-8)


def coarse_scores(q, g):
    """c = (sum (hi + lo) g^) * |q||g| / (|q||g| + 1e-8), [Q,G]: bf16 plane of the normalised rows, two bf16 planes of the
    normalised probe, products accumulated in fp32."""
    qn, gn = norms32(q), norms32(g)
    qh = unit(q, qn)
    hi = bf16(qh)
    lo = bf16(qh - hi)
    plane = bf16(unit(g, gn))
    p = qn[:, None] * gn[None, :]
    return (hi @ plane.T + lo @ plane.T) * (p / (p + 1e-8))


def topk_total_order(scores, index, k):
    """Top k of one probe's (scores[n], index[n]) by descending score, ties by ascending index."""
    by_index = torch.argsort(index, stable=True)
    order = by_index[torch.argsort(-scores[by_index], stable=True)][:k]
    return scores[order], index[order]


def search(q, g, k, eps=COARSE_EPS, exact=None):
    """The method on the CPU -> (scores[Q,k], index[Q,k], certified[Q] bool, slots[Q]): slots = the shortlist length a probe
    needs to certify (rows that cannot be told from the k-th by their coarse score, plus one).  `exact`: the [Q,G] scores to
    rank and re-score with (default: exact_scores in fp32)."""
    Q, G = q.size(0), g.size(0)
    s = exact_scores(q, g) if exact is None else exact
    rows = torch.arange(G)
    kp = shortlist_size(k)
    out_s = torch.full((Q, k), float('-inf'), dtype=s.dtype)
    out_i = torch.full((Q, k), -1, dtype=torch.int64)
    cert = torch.zeros((Q,), dtype=torch.bool)
    slots = torch.zeros((Q,), dtype=torch.int64)
    c = coarse_scores(q, g) if kp is not None else None
    for r in range(Q):
        fs, fi = topk_total_order(s[r], rows, k)              # the exact search: the fallback, and what must come out
        if kp is not None:
            cs, ci = topk_total_order(c[r], rows, kp)
            ss, si = topk_total_order(s[r][ci], ci, k)
            if G <= kp:
                cert[r] = True
            elif bool(cs[-1] + eps < ss[k - 1]):
                cert[r] = True
            if G >= k:
                slots[r] = int((c[r] + eps >= fs[k - 1].to(c.dtype)).sum()) + 1
            if cert[r]:
                fs, fi = ss, si
        n = fs.numel()
        out_s[r, :n], out_i[r, :n] = fs, fi
    return out_s, out_i, cert, slots


def midpoint_row():
    """A unit row whose every element sits just above a bf16 rounding midpoint right after a power of two, where the
    relative rounding error is largest (u / (1 + u), u = 2^-8): 168 elements 2^-4 (1 + u) and 344 elements 2^-5 (1 + u) have a
    norm of 1 - 1.5e-5, so the normalised elements lie 1.5e-5 (relative) above the midpoints and all round UP."""
    u = 2.0 ** -8
    row = torch.cat((torch.full((168,), 2.0 ** -4 * (1 + u)), torch.full((344,), 2.0 ** -5 * (1 + u))))
    return row.to(torch.float32)
