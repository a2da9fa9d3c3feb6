"""Subject-labelled search on the device (include/ffrnet.h: ffr_search_topk_subjects, ffr_topk_merge_subjects;
ffrnet_amd.search.Gallery with subjects).

Every comparison is bitwise.  The expected score matrix S[Q,G] comes from the existing API: Engine.search over 128-row
shards with k = 128 returns every s(q, g) bit for bit (the sharding contract of ffr_search_topk); the numpy restatement of
tests/search_subjects_ref.py turns S and the subjects into the expected lists."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ffrnet_amd
import search_subjects_ref as ref
from ffrnet_amd import native
from ffrnet_amd.search import Gallery

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {'small': (33, 1000), 'large': (257, 65537), 'one_probe': (1, 300), 'one_row': (31, 1)}


@pytest.fixture(scope='module')
def eng():
    return ffrnet_amd.Engine(0)


def rand_rows(n, seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return torch.randn((n, 512), device='cuda', generator=g)


def score_matrix(eng, q, g, norms):
    """S[Q,G] fp32 from 128-row shards of the existing search, k = 128: every score of the shard, bit for bit."""
    Q, G = q.size(0), g.size(0)
    S = torch.empty((Q, G), device='cuda')
    for lo in range(0, G, 128):
        n = min(128, G - lo)
        s, i = eng.search(q, g[lo:lo + n], 128, gallery_norms=norms[lo:lo + n], index_base=lo)
        S.scatter_(1, i[:, :n], s[:, :n])
    return S


class Data(object):
    def __init__(self, eng, q, g):
        self.q, self.g = q, g
        self.norms = eng.row_norms(g)
        self.S = score_matrix(eng, q, g, self.norms).cpu().numpy()
        self.order = ref.row_order(self.S)


@pytest.fixture(scope='module')
def data(eng):
    """One gallery and one probe set per shape, their score matrix and row order, built once and left unchanged.  Probe 0 of
    the large shape lies between rows 100 and 40000 (the shard test gives them one subject)."""
    out = {}
    for j, (name, (Q, G)) in enumerate(SHAPES.items()):
        q, g = rand_rows(Q, 300 + j), rand_rows(G, 400 + j)
        if name == 'large':
            q[0] = g[100] + g[40000]
        out[name] = Data(eng, q, g)
    return out


def layout(name, G, seed=0):
    """subject[G] int32 (numpy) of a named layout"""
    rng = np.random.default_rng(1000 + seed)
    rows = np.arange(G)
    if name == 'runs':                      # 1..9 consecutive rows per subject, across step and chunk boundaries
        lens = rng.integers(1, 10, size=G)
        subj = np.repeat(np.arange(G), lens)[:G]
    elif name == 'scattered':               # every subject in every chunk, several times per step
        subj = rows % 97
    elif name == 'few':
        subj = rows % 40
    elif name == 'one':
        subj = np.full(G, 7)
    elif name == 'removed':                 # ~30 % of the subjects withdrawn, and a whole run of rows that covers a chunk
        subj = layout('runs', G, seed).astype(np.int64)
        gone = rng.random(G) < 0.3
        subj[gone[subj]] = -1
        subj[128:256 if G <= 1000 else 7000] = -1
    elif name == 'all_removed':
        subj = np.full(G, -1)
    else:
        raise KeyError(name)
    return subj.astype(np.int32)


def run(eng, d, subj, k, distinct, rows=None):
    q = d.q if rows is None else d.q[rows]
    out = eng.search_subjects(q, d.g, torch.from_numpy(subj).cuda(), k, gallery_norms=d.norms, distinct=distinct)
    torch.cuda.synchronize()
    return out


def expect(d, subj, k, distinct):
    return tuple(torch.from_numpy(x).cuda() for x in ref.search_ref(d.S, subj, k, distinct, order=d.order))


def same(got, want):
    return all(a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b) for a, b in zip(got, want))


CASES = [('small', 10, 'runs'), ('small', 10, 'scattered'), ('small', 10, 'one'), ('small', 10, 'removed'),
         ('small', 10, 'all_removed'), ('small', 64, 'few'),
         ('large', 64, 'runs'), ('large', 64, 'scattered'), ('large', 64, 'few'), ('large', 64, 'removed'),
         ('one_probe', 64, 'runs'), ('one_probe', 64, 'few'), ('one_probe', 64, 'removed'), ('one_probe', 64, 'all_removed'),
         ('one_row', 1, 'one'), ('one_row', 1, 'all_removed')]


@pytest.mark.parametrize('shape,k,lay', CASES)
def test_both_modes_equal_the_restatement(eng, data, shape, k, lay):
    d = data[shape]
    subj = layout(lay, d.g.size(0))
    for distinct in (True, False):
        got = run(eng, d, subj, k, distinct)
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[2].dtype == torch.int32
        assert same(got, expect(d, subj, k, distinct)), (shape, k, lay, distinct)
    if lay == 'few':                        # 40 subjects, k = 64: padding
        assert torch.all(got[1][:, :1] >= 0)
        s, i, u = run(eng, d, subj, k, True)
        live = min(40, d.g.size(0))
        assert torch.all(i[:, live:] == -1) and torch.all(u[:, live:] == -1) and torch.all(s[:, live:] == float('-inf'))
        assert torch.all(torch.sort(u[:, :live], 1).values == torch.arange(live, device='cuda', dtype=torch.int32))
    if lay == 'one' and d.g.size(0) > 1:
        s, i, u = run(eng, d, subj, k, True)
        assert torch.all(u[:, 0] == 7) and torch.all(u[:, 1:] == -1) and torch.all(i[:, 1:] == -1)


def test_ties_report_the_smallest_index(eng):
    """Copies of one row under different subjects and under the same subject, in different chunks (G = 1000 is eight chunks
    of 128 rows): a subject speaks with its smallest tied index, and tied subjects order by that index."""
    g = rand_rows(1000, 71)
    for dst in (17, 140, 400, 900):
        g[dst] = g[650]
    q = torch.cat((g[650:651] * 0.5 + rand_rows(1, 72) * 1e-3, rand_rows(32, 73)), 0)
    subj = (100 + np.arange(1000)).astype(np.int32)
    subj[[17, 140]] = 5
    subj[[400, 900]] = 9
    subj[650] = 3
    d = Data(eng, q, g)
    s, i, u = run(eng, d, subj, 10, True)
    assert i[0, :3].tolist() == [17, 400, 650] and u[0, :3].tolist() == [5, 9, 3]
    assert torch.equal(s[0, :3], s[0, :1].expand(3)) and s[0, 3] < s[0, 2]
    assert same((s, i, u), expect(d, subj, 10, True))
    s, i, u = run(eng, d, subj, 10, False)
    assert i[0, :5].tolist() == [17, 140, 400, 650, 900] and u[0, :5].tolist() == [5, 5, 9, 3, 9]
    assert same((s, i, u), expect(d, subj, 10, False))
    # the first copy withdrawn: its subject speaks with the next one
    subj[17] = -1
    s, i, u = run(eng, d, subj, 10, True)
    assert i[0, :3].tolist() == [140, 400, 650] and u[0, :3].tolist() == [5, 9, 3]
    assert same((s, i, u), expect(d, subj, 10, True))


@pytest.mark.parametrize('shape', ['small', 'large'])
def test_row_mode_without_removal_is_the_plain_search(eng, data, shape):
    d = data[shape]
    subj = layout('runs', d.g.size(0))
    st = torch.from_numpy(subj).cuda()
    for k in (10, 128):
        s, i, u = run(eng, d, subj, k, False)
        ws, wi = eng.search(d.q, d.g, k, gallery_norms=d.norms)
        assert torch.equal(s, ws) and torch.equal(i, wi)
        assert torch.equal(u, st[i])


def test_deterministic_and_batch_independent(eng, data):
    d = data['large']
    subj = layout('removed', d.g.size(0))
    for distinct in (True, False):
        a = run(eng, d, subj, 64, distinct)
        b = run(eng, d, subj, 64, distinct)
        assert same(a, b)
        for r in (0, 1, 31, 32, 100, 223, 255, 256):
            one = run(eng, d, subj, 64, distinct, rows=slice(r, r + 1))
            assert all(torch.equal(x[0], y[r]) for x, y in zip(one, a)), (distinct, r)


def test_shard_merge_equals_single_search(eng, data):
    """Three uneven contiguous shards, the first smaller than k, and an empty one.  Rows 100 and 40000 (second and third
    shard) carry one subject, and probe 0 lies between them: that subject leads in two shards."""
    d = data['large']
    G = d.g.size(0)
    subj = layout('scattered', G)
    subj[40000] = subj[100]
    st = torch.from_numpy(subj).cuda()
    for k, distinct in ((10, True), (64, True), (10, False), (128, False)):
        bounds = [0, k // 2, 30000, G, G]
        parts = []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            parts.append(eng.search_subjects(d.q, d.g[lo:hi], st[lo:hi], k, gallery_norms=d.norms[lo:hi], index_base=lo,
                                             distinct=distinct))
        assert torch.all(parts[3][1] == -1) and torch.all(parts[3][2] == -1) and torch.all(torch.isinf(parts[3][0]))
        if distinct:
            assert parts[1][2][0, 0].item() == subj[100] and parts[2][2][0, 0].item() == subj[100]
            assert parts[1][1][0, 0].item() == 100 and parts[2][1][0, 0].item() == 40000
        merged = eng.topk_merge_subjects(*[torch.stack([p[j] for p in parts]) for j in range(3)], distinct=distinct)
        whole = run(eng, d, subj, k, distinct)
        assert same(merged, whole), (k, distinct)
        if k <= 64:
            assert same(whole, expect(d, subj, k, distinct))
        if distinct:
            assert int((whole[2][0] == subj[100]).sum()) == 1


def test_gallery_with_subjects(eng, data):
    d = data['small']
    G = d.g.size(0)
    subj = layout('runs', G)
    st = torch.from_numpy(subj).cuda()
    gal = Gallery(eng, subjects=True)
    assert gal.add(d.g[:600], st[:600]) == 0 and gal.add(d.g[600:], st[600:].to(torch.int64)) == 600 and len(gal) == G
    assert torch.equal(gal.subjects, st) and gal.subjects.dtype == torch.int32 and torch.equal(gal.norms, d.norms)
    s, u, i = gal.search_subjects(d.q, 10)
    es, ei, eu = eng.search_subjects(d.q, d.g, st, 10, gallery_norms=d.norms)
    assert torch.equal(s, es) and torch.equal(i, ei) and torch.equal(u, eu)
    assert same((s, i, u), expect(d, subj, 10, True))
    rs, ri = gal.search(d.q, 10)
    ws, wi = eng.search(d.q, d.g, 10, gallery_norms=d.norms)
    assert torch.equal(rs, ws) and torch.equal(ri, wi)
    # withdraw the subject that leads for probe 0 (and one more): neither search returns them again
    gone = [int(u[0, 0]), int(u[5, 2])]
    n_rows = int(np.isin(subj, gone).sum())
    assert gal.remove(gone) == n_rows and len(gal) == G
    subj2 = subj.copy()
    subj2[np.isin(subj, gone)] = -1
    assert torch.equal(gal.subjects, torch.from_numpy(subj2).cuda())
    s2, u2, i2 = gal.search_subjects(d.q, 10)
    assert not torch.any(torch.isin(u2, torch.tensor(gone, device='cuda', dtype=torch.int32)))
    assert same((s2, i2, u2), expect(d, subj2, 10, True))
    rs2, ri2 = gal.search(d.q, 10)
    assert not torch.any(torch.isin(st[ri2], torch.tensor(gone, device='cuda', dtype=torch.int32)))
    want = expect(d, subj2, 10, False)
    assert torch.equal(rs2, want[0]) and torch.equal(ri2, want[1])
    # leave-one-out still works under the mask
    me = torch.tensor([3, 500, 999], device='cuda')
    me = me[st[me] != gone[0]]
    me = me[torch.from_numpy(subj2).cuda()[me] >= 0]
    ls, li = gal.search(d.g[me], 5, self_index=me)
    assert li.shape == (me.numel(), 5) and not torch.any(li == me[:, None])
    # compact: removed rows leave, scores keep their bits, indices map
    old_to_new = gal.compact()
    assert old_to_new.dtype == torch.int64 and old_to_new.shape == (G,) and len(gal) == G - n_rows
    keep = torch.from_numpy(subj2 >= 0).cuda()
    assert torch.all(old_to_new[~keep] == -1)
    assert torch.equal(old_to_new[keep], torch.arange(G - n_rows, device='cuda'))
    assert torch.equal(gal.embeddings, d.g[keep]) and torch.equal(gal.norms, d.norms[keep])
    assert torch.equal(gal.subjects, st[keep])
    s3, u3, i3 = gal.search_subjects(d.q, 10)
    assert torch.equal(s3, s2) and torch.equal(u3, u2) and torch.equal(i3, old_to_new[i2])
    rs3, ri3 = gal.search(d.q, 10)
    assert torch.equal(rs3, rs2) and torch.equal(ri3, old_to_new[ri2])
    # what the class refuses
    with pytest.raises(RuntimeError, match='shortlist does not know subjects'):
        Gallery(eng, coarse=True, subjects=True)
    with pytest.raises(RuntimeError):
        gal.add(d.g[:4], st[:3])
    with pytest.raises(RuntimeError):
        gal.add(d.g[:2], torch.tensor([1, -1], device='cuda'))
    with pytest.raises(RuntimeError):
        gal.add(d.g[:2], torch.tensor([1, 2 ** 31], device='cuda'))
    with pytest.raises(RuntimeError):
        gal.add(d.g[:2])
    plain = Gallery(eng)
    plain.add(d.g[:10])
    for call in (lambda: plain.search_subjects(d.q, 5), lambda: plain.remove([1]), plain.compact, lambda: plain.subjects,
                 lambda: plain.add(d.g[:2], st[:2])):
        with pytest.raises(RuntimeError):
            call()


def _rc(eng, fn, *args):
    return getattr(eng.lib, fn)(eng._h, *args)


def test_arguments(eng):
    q, g = rand_rows(4, 51), rand_rows(100, 52)
    n = eng.row_norms(g)
    sub = torch.arange(101, device='cuda', dtype=torch.int32)
    s = torch.empty((4, 129), device='cuda')
    i = torch.empty((4, 129), device='cuda', dtype=torch.int64)
    u = torch.empty((4, 129), device='cuda', dtype=torch.int32)
    P = native._ptr
    st = eng._stream()
    ok = (P(q), 4, P(g), P(n), P(sub), 100, 512, 10, 0, 1, P(s), P(i), P(u), st)
    names = ['q', 'Q', 'g', 'n', 'sub', 'G', 'dim', 'k', 'base', 'distinct', 's', 'i', 'u', 'st']

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[names.index(key)] = v
        return _rc(eng, 'ffr_search_topk_subjects', *a)

    null = C.c_void_p(0)
    assert call() == 0 and call(distinct=0) == 0
    assert call(dim=256) == -6
    for bad in (dict(k=0), dict(k=129, distinct=0), dict(Q=0), dict(G=-1), dict(q=null), dict(g=null), dict(n=null), dict(s=null),
                dict(i=null),
                dict(sub=null), dict(sub=C.c_void_p(sub.data_ptr() + 2)), dict(u=null), dict(distinct=2), dict(distinct=-1),
                dict(k=65), dict(k=128)):
        assert call(**bad) == -1, bad
    assert call(k=64) == 0 and call(k=128, distinct=0) == 0 and call(k=65, distinct=0) == 0
    assert call(sub=C.c_void_p(sub.data_ptr() + 4)) == 0            # 4-byte alignment is all the subjects need
    assert call(G=0, g=null, n=null, sub=null) == 0                  # G = 0: all padding, NULL gallery pointers allowed
    torch.cuda.synchronize()
    assert torch.all(i.reshape(-1)[:40] == -1) and torch.all(u.reshape(-1)[:40] == -1)
    assert torch.all(s.reshape(-1)[:40] == float('-inf'))
    mok = (P(s), P(i), P(u), 1, 4, 10, 1, P(s), P(i), P(u), st)
    mnames = ['s', 'i', 'u', 'S', 'Q', 'k', 'distinct', 'os', 'oi', 'ou', 'st']

    def merge(**kw):
        a = list(mok)
        for key, v in kw.items():
            a[mnames.index(key)] = v
        return _rc(eng, 'ffr_topk_merge_subjects', *a)

    assert merge(S=0) == -1 and merge(S=4097) == -1 and merge(k=129, distinct=0) == -1 and merge(k=65) == -1
    assert merge(u=null) == -1 and merge(ou=null) == -1 and merge(distinct=2) == -1 and merge(Q=0) == -1
    # the binding: k, devices and dtypes
    sub = sub[:100]
    es, ei, eu = eng.search_subjects(q, g[:0], sub[:0], 5)
    assert torch.all(ei == -1) and torch.all(eu == -1) and torch.all(es == float('-inf'))
    with pytest.raises(RuntimeError):
        eng.search_subjects(q, g, sub, 65)
    assert eng.search_subjects(q, g, sub, 128, distinct=False)[1].shape == (4, 128)
    with pytest.raises(RuntimeError):
        eng.search_subjects(q, g, sub.cpu(), 10)
    with pytest.raises(RuntimeError):
        eng.search_subjects(q, g, sub.float(), 10)
    with pytest.raises(RuntimeError):
        eng.search_subjects(q, g, sub[:99], 10)
    with pytest.raises(RuntimeError):
        eng.search_subjects(q.cpu(), g, sub, 10)
    a = eng.search_subjects(q, g, sub, 10)
    b = eng.search_subjects(q, g, sub.to(torch.int64), 10)
    assert same(a, b)
    three = [x.unsqueeze(0) for x in a]
    with pytest.raises(RuntimeError):
        eng.topk_merge_subjects(three[0], three[1], three[2].float())
    with pytest.raises(RuntimeError):
        eng.topk_merge_subjects(three[0], three[1], three[2].cpu())
    with pytest.raises(RuntimeError):
        eng.topk_merge_subjects(three[0], three[1], three[2][:, :, :5])
    assert same(eng.topk_merge_subjects(*three), a)
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError):
            eng.search_subjects(q, g, sub.to('cuda:1'), 10)


def test_profile_counts_one_launch_under_score(eng):
    q, g = rand_rows(40, 61), rand_rows(5000, 62)
    n = eng.row_norms(g)
    sub = (torch.arange(5000, device='cuda') // 8).to(torch.int32)
    torch.cuda.synchronize()
    for distinct in (True, False):
        eng.profile_enable(True)
        eng.profile_read()
        eng.search_subjects(q, g, sub, 10, gallery_norms=n, distinct=distinct)
        st = eng.profile_read()
        eng.profile_enable(False)
        assert st['score']['launches'] == 1 and st['score']['flops'] == 2.0 * 40 * 5000 * 512 and st['score']['ms'] > 0
        assert sum(v['launches'] for k, v in st.items() if k != 'score') == 0


def test_sharded_identity_search_two_ranks_on_one_gpu():
    """tools/search_subjects_two_ranks_one_gpu.py: two gloo ranks on cuda:0, each with a contiguous shard; every rank's
    search_sharded(..., distinct=True) equals the single-process identity search bitwise."""
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'search_subjects_two_ranks_one_gpu.py')], cwd=ROOT,
                             capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.fail('two-rank identity search timed out: %s' % ((e.stderr or b'')[-2000:],))
    assert out.returncode == 0 and 'OK' in out.stdout, (out.stdout[-1000:], out.stderr[-2000:])
