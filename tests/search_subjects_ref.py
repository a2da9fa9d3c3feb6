"""numpy restatement of the subject-labelled search (include/ffrnet.h: ffr_search_topk_subjects, ffr_topk_merge_subjects)
from a full score matrix S[Q,G] (fp32) and subject[G]; no test in itself.

Row g comes before row g' for probe q iff S[q,g] > S[q,g'], or the scores are equal and g < g'.  Rows with subject < 0 are
removed.  Row mode lists the first k live rows; identity mode lists the first k of {best(u)}, best(u) the first row of
subject u.  Slots past the live rows / subjects hold (-inf, -1, -1)."""
import numpy as np


def row_order(S):
    """order[Q,G]: the rows of every probe in the total order (a stable sort of -S: equal scores keep ascending index)."""
    S = np.asarray(S, dtype=np.float32)
    return np.argsort(-S, axis=1, kind='stable')


def _pad(Q, k):
    return (np.full((Q, k), -np.inf, dtype=np.float32), np.full((Q, k), -1, dtype=np.int64),
            np.full((Q, k), -1, dtype=np.int32))


def _first_of_each(subj):
    """positions of the first occurrence of every value of subj, ascending"""
    _, first = np.unique(subj, return_index=True)
    return np.sort(first)


def search_ref(S, subject, k, distinct, index_base=0, order=None):
    """-> (score[Q,k] fp32, index[Q,k] int64, subject[Q,k] int32); `order` = row_order(S) when the caller has it."""
    S = np.asarray(S, dtype=np.float32)
    subject = np.asarray(subject).astype(np.int64)
    Q, G = S.shape
    assert subject.shape == (G,)
    if order is None:
        order = row_order(S)
    out_s, out_i, out_u = _pad(Q, k)
    for q in range(Q):
        o = order[q]
        o = o[subject[o] >= 0]
        if distinct:
            o = o[_first_of_each(subject[o])]
        o = o[:k]
        out_s[q, :len(o)] = S[q, o]
        out_i[q, :len(o)] = o + index_base
        out_u[q, :len(o)] = subject[o]
    return out_s, out_i, out_u


def merge_ref(score, index, subject, distinct):
    """Lists [S,Q,k] (index < 0 = padding) -> one [Q,k] list in the same order; identity mode keeps the first entry of a
    subject."""
    score = np.asarray(score, dtype=np.float32)
    index = np.asarray(index).astype(np.int64)
    subject = np.asarray(subject).astype(np.int64)
    nS, Q, k = score.shape
    out_s, out_i, out_u = _pad(Q, k)
    for q in range(Q):
        s, i, u = score[:, q].reshape(-1), index[:, q].reshape(-1), subject[:, q].reshape(-1)
        real = i >= 0
        s, i, u = s[real], i[real], u[real]
        o = np.lexsort((i, -s))
        if distinct:
            o = o[_first_of_each(u[o])]
        o = o[:k]
        out_s[q, :len(o)] = s[o]
        out_i[q, :len(o)] = i[o]
        out_u[q, :len(o)] = u[o]
    return out_s, out_i, out_u


def search_naive(S, subject, k, distinct, index_base=0):
    """The definition once more, without sorting: per probe, pick the best remaining row k times."""
    S = np.asarray(S, dtype=np.float32)
    Q, G = S.shape
    out_s, out_i, out_u = _pad(Q, k)
    for q in range(Q):
        seen, taken = set(), set()
        for p in range(k):
            best = -1
            for g in range(G):
                u = int(subject[g])
                if u < 0 or g in taken or (distinct and u in seen):
                    continue
                if best < 0 or S[q, g] > S[q, best]:         # strict: among equal scores the smallest index stays
                    best = g
            if best < 0:
                break
            taken.add(best)
            seen.add(int(subject[best]))
            out_s[q, p], out_i[q, p], out_u[q, p] = S[q, best], best + index_base, subject[best]
    return out_s, out_i, out_u


def cmc_naive(subjects, probe_labels, ranks):
    out = {}
    for r in ranks:
        hits = 0
        for row, lab in zip(subjects, probe_labels):
            hits += any(int(u) == int(lab) and int(u) >= 0 for u in list(row)[:r])
        out[r] = hits / float(len(probe_labels)) if len(probe_labels) else 0.0
    return out
