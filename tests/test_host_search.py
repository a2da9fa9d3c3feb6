"""CPU checks of the identification helpers (ffrnet_amd.search) against naive numpy restatements, on hand-made top-k
lists: CMC rank-r rates and the leave-one-out trimming of a top-(k+1) list."""
import numpy as np
import torch

from ffrnet_amd.search import drop_self, identification_rates


def cmc_naive(index, probe_labels, gallery_labels, r):
    hits = 0
    for q in range(index.shape[0]):
        hits += any(index[q, j] >= 0 and gallery_labels[index[q, j]] == probe_labels[q] for j in range(r))
    return hits / index.shape[0]


def drop_naive(scores, index, self_index):
    s_out, i_out = [], []
    for q in range(index.shape[0]):
        row = list(range(index.shape[1]))
        own = [j for j in row if index[q, j] == self_index[q]]
        row.remove(own[0] if own else row[-1])
        s_out.append(scores[q, row])
        i_out.append(index[q, row])
    return np.array(s_out), np.array(i_out)


def test_identification_rates_match_naive_cmc():
    rng = np.random.default_rng(3)
    G, Q, k = 40, 25, 10
    gallery_labels = rng.integers(0, 12, G)
    probe_labels = rng.integers(0, 12, Q)
    index = np.stack([rng.permutation(G)[:k] for _ in range(Q)])
    index[3, 7:] = -1                        # padding of a short gallery
    index[4, :] = -1
    rates = identification_rates(torch.tensor(index), torch.tensor(probe_labels), torch.tensor(gallery_labels),
                                 ranks=(1, 5, 10))
    for r in (1, 5, 10):
        assert abs(rates[r] - cmc_naive(index, probe_labels, gallery_labels, r)) < 1e-12, r
    assert rates[1] <= rates[5] <= rates[10]
    # a hand-made case with known answers
    idx = torch.tensor([[1, 0, 2], [2, 0, 1], [0, -1, -1]])
    r = identification_rates(idx, [7, 9, 5], [9, 7, 8], ranks=(1, 2, 3))
    assert r[1] == 1 / 3 and r[2] == 2 / 3 and r[3] == 2 / 3


def test_leave_one_out_trimming_matches_naive():
    rng = np.random.default_rng(4)
    Q, k1 = 30, 11
    index = np.stack([rng.permutation(100)[:k1] for _ in range(Q)]).astype(np.int64)
    scores = -np.sort(-rng.random((Q, k1)).astype(np.float32), 1)
    self_index = np.array([index[q, q % k1] if q % 3 else 1000 + q for q in range(Q)], dtype=np.int64)
    s, i = drop_self(torch.tensor(scores), torch.tensor(index), torch.tensor(self_index))
    ns, ni = drop_naive(scores, index, self_index)
    assert s.shape == (Q, k1 - 1) and np.array_equal(i.numpy(), ni) and np.array_equal(s.numpy(), ns)
    assert not np.any(i.numpy() == self_index[:, None])
