"""numpy restatement of the filtered search (include/ffrnet.h: ffr_search_topk_filtered) from a full score matrix S[Q,G]
(fp32), tag[G], mask[Q] and, when the gallery has them, subject[G]; no test in itself.

Row g is admissible for probe q iff (tag[g] & mask[q]) != 0 and (there are no subjects or subject[g] >= 0).  The result of
probe q is that of the subject search (tests/search_subjects_ref.py) over the gallery in which every row inadmissible for q
is marked removed; without subjects every row is its own subject, arange(G), and the subject plane is not part of the
result."""
import numpy as np

import search_subjects_ref as sref


def words(x):
    """tag or mask words as uint32, from ints, uint32, int64 in [0, 2^32) or int32 bit patterns"""
    x = np.asarray(x)
    if x.dtype == np.int32:
        return x.view(np.uint32)
    assert np.all(x >= 0) and np.all(x < 2 ** 32)
    return x.astype(np.uint32)


def search_ref(S, tag, mask, k, subject=None, distinct=0, index_base=0, order=None):
    """-> (score[Q,k] fp32, index[Q,k] int64, subject[Q,k] int32); without `subject` the third plane is arange(G) of the
    listed rows and no part of the library's result.  `order` = search_subjects_ref.row_order(S) when the caller has it."""
    S = np.asarray(S, dtype=np.float32)
    Q, G = S.shape
    tag, mask = words(tag), words(mask)
    assert tag.shape == (G,) and mask.shape == (Q,)
    assert subject is not None or not distinct
    base = np.arange(G, dtype=np.int64) if subject is None else np.asarray(subject).astype(np.int64)
    out = []
    for q in range(Q):
        sub_q = np.where((tag & mask[q]) != 0, base, -1)
        out.append(sref.search_ref(S[q:q + 1], sub_q, k, distinct, index_base, order=None if order is None else order[q:q + 1]))
    return tuple(np.concatenate([o[j] for o in out], 0) for j in range(3))


def search_naive(S, tag, mask, k, subject=None, distinct=0, index_base=0):
    """The definition once more, without sorting and without the subject restatement: per probe, pick the best remaining
    admissible row k times; in identity mode a subject that was picked is out."""
    S = np.asarray(S, dtype=np.float32)
    Q, G = S.shape
    tag, mask = [int(t) for t in words(tag)], [int(m) for m in words(mask)]
    out_s = np.full((Q, k), -np.inf, dtype=np.float32)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    out_u = np.full((Q, k), -1, dtype=np.int32)
    for q in range(Q):
        taken, seen = set(), set()
        for p in range(k):
            best = -1
            for g in range(G):
                if (tag[g] & mask[q]) == 0 or g in taken:
                    continue
                if subject is not None and (int(subject[g]) < 0 or (distinct and int(subject[g]) in seen)):
                    continue
                if best < 0 or S[q, g] > S[q, best]:         # strict: among equal scores the smallest index stays
                    best = g
            if best < 0:
                break
            taken.add(best)
            out_s[q, p], out_i[q, p] = S[q, best], best + index_base
            out_u[q, p] = best if subject is None else subject[best]
            if subject is not None:
                seen.add(int(subject[best]))
    return out_s, out_i, out_u
