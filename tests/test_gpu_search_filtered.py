"""Filtered search on the device (include/ffrnet.h: ffr_search_topk_filtered; Engine.search_filtered; ffrnet_amd.search.Gallery
with tags).

Every comparison is bitwise.  The expected score matrix S[Q,G] is taken as tests/test_gpu_search_subjects.py takes it, from
Engine.search over 128-row shards at k = 128, once per module; the numpy restatement of tests/search_filtered_ref.py turns S,
the tags, the masks and the subjects into the expected lists.  A top-k list is a prefix of every longer one, so the
restatement runs once per case at the largest k and is cut to the others."""
import ctypes as C

import numpy as np
import pytest
import torch

import ffrnet_amd
import search_filtered_ref as fref
import search_subjects_ref as sref
import test_gpu_search_subjects as base
from ffrnet_amd import native
from ffrnet_amd.search import Gallery, drop_self, search_sharded, search_sharded_filtered

pytestmark = pytest.mark.gpu

SHAPES = base.SHAPES            # small (33, 1000): a probe-tile tail, eight 128-row chunks; large (257, 65537): many steps per
#                                 chunk and a ragged last row; one_probe (1, 300); one_row (31, 1)
TAG_LAYOUTS = ('bit', 'blocks', 'sparse', 'zero', 'ones')
SUBJECT_LAYOUTS = (None, 'runs', 'scattered', 'removed')
MASK_SETS = ('single', 'mixed')
FULL, B31 = 0xFFFFFFFF, 0x80000000
K_ROWS, K_IDS = (1, 10, 64, 128), (1, 10, 64)


@pytest.fixture(scope='module')
def eng():
    return ffrnet_amd.Engine(0)


@pytest.fixture(scope='module')
def data(eng):
    """One gallery and one probe set per shape with their score matrix and row order, built once and left unchanged"""
    return {name: base.Data(eng, base.rand_rows(Q, 500 + j), base.rand_rows(G, 600 + j)) for j, (name, (Q, G)) in enumerate(SHAPES.items())}


def tag_layout(name, G):
    """tag[G] as int64 words in [0, 2^32)"""
    g = np.arange(G, dtype=np.int64)
    if name == 'bit':
        return 1 << (g % 32)
    if name == 'blocks':                    # whole steps (128 rows) and, at G = 1000, whole chunks are inadmissible for a probe
        return 1 << ((g // 128) % 4)
    if name == 'sparse':                    # a few bits per word, a fifth of the words zero
        rng = np.random.default_rng(77)
        w = np.zeros(G, dtype=np.int64)
        for b in range(32):
            w |= (rng.random(G) < 0.06).astype(np.int64) << b
        w[rng.random(G) < 0.2] = 0
        return w
    return np.full(G, {'zero': 0, 'ones': FULL}[name], dtype=np.int64)


def mask_set(name, Q):
    """mask[Q] as int64 words: every probe one bit, or the other kinds in turn"""
    q = np.arange(Q, dtype=np.int64)
    if name == 'single':
        return 1 << (q % 32)
    two = (1 << (q % 32)) | (1 << ((q + 7) % 32))
    three = two | (1 << ((3 * q + 1) % 32))
    kinds = np.stack([two, three, np.zeros(Q, dtype=np.int64), np.full(Q, FULL), np.full(Q, B31)])
    return kinds[q % 5, q]


def dev(words):
    """int64 words -> the int32 device tensor the library reads"""
    return native.tag_words(torch.from_numpy(np.asarray(words, dtype=np.int64)), 'words', 'cuda')


def run(eng, d, tag, mask, k, subj=None, distinct=False, rows=None, **kw):
    q = d.q if rows is None else d.q[rows]
    out = eng.search_filtered(q, dev(mask), d.g, dev(tag), k, gallery_norms=d.norms,
                              subjects=None if subj is None else torch.from_numpy(subj).cuda(), distinct=distinct, **kw)
    torch.cuda.synchronize()
    assert len(out) == (2 if subj is None else 3)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int64 and (subj is None or out[2].dtype == torch.int32)
    return out


def expect(d, tag, mask, k, subj=None, distinct=False):
    """the restatement's lists on the device: two planes without subjects, three with"""
    want = fref.search_ref(d.S, tag, mask, k, subj, int(distinct), order=d.order)
    return tuple(torch.from_numpy(x).cuda() for x in want[:2 if subj is None else 3])


def cut(lists, k):
    return tuple(x[:, :k].contiguous() for x in lists)


same = base.same


@pytest.mark.parametrize('subj_lay', SUBJECT_LAYOUTS)
@pytest.mark.parametrize('tag_lay', TAG_LAYOUTS)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_every_layout_equals_the_restatement(eng, data, shape, tag_lay, subj_lay):
    d = data[shape]
    Q, G = SHAPES[shape]
    tag = tag_layout(tag_lay, G)
    subj = None if subj_lay is None else base.layout(subj_lay, G)
    for ms in MASK_SETS:
        mask = mask_set(ms, Q)
        for distinct in ((False,) if subj is None else (False, True)):
            ks = K_IDS if distinct else K_ROWS
            want = expect(d, tag, mask, ks[-1], subj, distinct)
            for k in ks:
                got = run(eng, d, tag, mask, k, subj, distinct)
                assert same(got, cut(want, k)), (shape, tag_lay, subj_lay, ms, distinct, k)
            if tag_lay == 'zero':
                assert torch.all(got[1] == -1) and torch.all(torch.isinf(got[0]))
        if ms == 'mixed' and Q >= 5:            # probe 2 has mask 0: k slots of padding, whatever the tags are
            assert torch.all(got[1][2] == -1) and torch.all(got[0][2] == float('-inf'))


def test_single_bit_masks_fill_k_10_and_pad_k_64(eng, data):
    """tag = 1 << (g % 32) at G = 1000: 32 admissible rows for the bits 0..7 and 31 for the others"""
    d = data['small']
    Q, G = SHAPES['small']
    tag, mask = tag_layout('bit', G), mask_set('single', Q)
    n_adm = torch.tensor([32 if q % 32 < 8 else 31 for q in range(Q)], device='cuda')
    s, i = run(eng, d, tag, mask, 10)
    assert torch.all(i >= 0) and torch.all(i % 32 == torch.arange(Q, device='cuda')[:, None] % 32) and torch.all(torch.isfinite(s))
    s, i = run(eng, d, tag, mask, 64)
    slot = torch.arange(64, device='cuda')[None, :]
    real = slot < n_adm[:, None]
    assert torch.all(i[real] >= 0) and torch.all(i[~real] == -1) and torch.all(s[~real] == float('-inf')) and torch.all(torch.isfinite(s[real]))
    # identities: every row its own subject but pairs (2j, 2j + 1 share one): rows of a pair carry different bits, so the count stays
    subj = (np.arange(G) // 2).astype(np.int32)
    s, i, u = run(eng, d, tag, mask, 64, subj, True)
    assert torch.all(i[real] >= 0) and torch.all(i[~real] == -1) and torch.all(u[~real] == -1) and torch.all(s[~real] == float('-inf'))
    assert torch.equal(u[real], (i[real] // 2).to(torch.int32))


@pytest.mark.parametrize('shape', ['small', 'large'])
def test_all_tags_set_and_a_full_mask_is_the_unfiltered_search(eng, data, shape):
    d = data[shape]
    Q, G = SHAPES[shape]
    tag = tag_layout('sparse', G) | 1 << 13              # no word is zero
    mask = np.full(Q, FULL, dtype=np.int64)
    for k in (10, 128):
        assert same(run(eng, d, tag, mask, k), eng.search(d.q, d.g, k, gallery_norms=d.norms))
    subj = base.layout('removed', G)
    st = torch.from_numpy(subj).cuda()
    for k, distinct in ((10, False), (128, False), (10, True), (64, True)):
        assert same(run(eng, d, tag, mask, k, subj, distinct),
                    eng.search_subjects(d.q, d.g, st, k, gallery_norms=d.norms, distinct=distinct)), (k, distinct)


def test_a_row_of_the_batch_equals_the_one_probe_call(eng, data):
    d = data['large']
    Q, G = SHAPES['large']
    tag, mask = tag_layout('sparse', G), mask_set('mixed', Q)
    subj = base.layout('removed', G)
    for s_, distinct, k in ((None, False, 128), (subj, False, 64), (subj, True, 64)):
        whole = run(eng, d, tag, mask, k, s_, distinct)
        assert same(whole, run(eng, d, tag, mask, k, s_, distinct))
        for r in (0, 1, 2, 31, 32, 100, 223, 255, 256):
            one = run(eng, d, tag, mask[r:r + 1], k, s_, distinct, rows=slice(r, r + 1))
            assert all(torch.equal(x[0], y[r]) for x, y in zip(one, whole)), (distinct, r)
        # an int mask is that word for every probe
        every = eng.search_filtered(d.q, int(mask[1]), d.g, dev(tag), k, gallery_norms=d.norms,
                                    subjects=None if s_ is None else torch.from_numpy(s_).cuda(), distinct=distinct)
        assert all(torch.equal(x[1], y[1]) for x, y in zip(every, whole))


@pytest.mark.parametrize('shape', ['small', 'large'])
def test_shard_merge_equals_one_call(eng, data, shape):
    """Shards of 1, 127 and 128 rows and the rest, each searched with its index_base; the merges do not know the filter"""
    d = data[shape]
    Q, G = SHAPES[shape]
    tag, mask = tag_layout('sparse', G), mask_set('mixed', Q)
    subj = base.layout('scattered', G)
    tt, mt, st = dev(tag), dev(mask), torch.from_numpy(subj).cuda()
    bounds = [0, 1, 128, 256, G]
    for s_, distinct, k in ((None, False, 10), (None, False, 128), (subj, False, 64), (subj, True, 10), (subj, True, 64)):
        parts = [eng.search_filtered(d.q, mt, d.g[lo:hi], tt[lo:hi], k, gallery_norms=d.norms[lo:hi], index_base=lo,
                                     subjects=None if s_ is None else st[lo:hi], distinct=distinct)
                 for lo, hi in zip(bounds[:-1], bounds[1:])]
        stacked = [torch.stack([p[j] for p in parts]) for j in range(len(parts[0]))]
        merged = eng.topk_merge(*stacked) if s_ is None else eng.topk_merge_subjects(*stacked, distinct=distinct)
        whole = run(eng, d, tag, mask, k, s_, distinct)
        assert same(merged, whole), (k, distinct)
        assert same(whole, expect(d, tag, mask, k, s_, distinct))


def test_tied_copies_report_the_smallest_admissible_index(eng):
    """Copies of one row in different chunks (G = 1000 is eight chunks of 128 rows) under different tags; six times the same
    probe under different masks: each gets the smallest index among the tied copies it may see."""
    g = base.rand_rows(1000, 81)
    copies = {17: 1, 140: 2, 400: 1 | 4, 650: 8, 900: 2}
    for dst in copies:
        g[dst] = g[650]
    tag = np.full(1000, FULL & ~31, dtype=np.int64)        # the other rows: bits 5..31
    for dst, w in copies.items():
        tag[dst] = w
    q = (g[650:651] * 0.5 + base.rand_rows(1, 82) * 1e-3).repeat(6, 1)
    mask = np.array([1, 2, 4, 8, 2 | 8, 16 | 32], dtype=np.int64)
    d = base.Data(eng, q, g)
    s, i = run(eng, d, tag, mask, 10)
    assert i[:4, 0].tolist() == [17, 140, 400, 650] and i[4, :3].tolist() == [140, 650, 900] and i[0, :2].tolist() == [17, 400]
    assert torch.equal(s[:5, 0], s[0, :1].expand(5)) and torch.equal(s[4, :3], s[0, :1].expand(3))
    assert s[5, 0] < s[0, 0] and not any(r in copies for r in i[5].tolist())
    assert torch.all(i[:4, 2:] == -1) and torch.all(i[1, 2:] == -1) and i[3, 1].item() == -1
    assert same((s, i), expect(d, tag, mask, 10))
    subj = (100 + np.arange(1000)).astype(np.int32)
    subj[[17, 140]] = 5
    subj[[400, 900]] = 9
    subj[650] = 3
    s, i, u = run(eng, d, tag, mask, 10, subj, True)
    assert i[:5, 0].tolist() == [17, 140, 400, 650, 140] and u[:5, 0].tolist() == [5, 5, 9, 3, 5]
    assert i[4, :3].tolist() == [140, 650, 900] and u[4, :3].tolist() == [5, 3, 9] and i[0, :2].tolist() == [17, 400]
    assert same((s, i, u), expect(d, tag, mask, 10, subj, True))


def _grown(eng, d, n_more, seed):
    """The small gallery and `n_more` copies of its first rows behind it (1100 rows: past the first capacity of 1024), as a
    Data whose score matrix is extended to match"""
    ext = base.Data.__new__(base.Data)
    ext.q, ext.g = d.q, torch.cat((d.g, d.g[:n_more]), 0)
    ext.norms = torch.cat((d.norms, d.norms[:n_more]), 0)
    ext.S = np.concatenate((d.S, d.S[:, :n_more]), 1)
    ext.order = sref.row_order(ext.S)
    rng = np.random.default_rng(seed)
    tag = tag_layout('sparse', ext.g.size(0))
    tag[rng.random(tag.size) < 0.3] |= B31
    return ext, tag


def test_gallery_with_tags(eng, data):
    d, tag = _grown(eng, data['small'], 100, 5)
    Q, G = d.q.size(0), d.g.size(0)
    mask = mask_set('mixed', Q)
    mask[1] = B31
    mt = dev(mask)
    gal = Gallery(eng)
    assert not gal.has_tags
    with pytest.raises(RuntimeError, match='build_tags'):
        gal.search(d.q, 5, mask=1)
    gal.build_tags()
    gal.build_tags()                                             # a second call does nothing
    assert gal.has_tags and gal.tags.shape == (0,)
    assert gal.add(d.g[:600], tags=dev(tag[:600])) == 0                                            # int32 bit patterns
    assert gal.add(d.g[600:1000], tags=torch.from_numpy(tag[600:1000])) == 600                     # int64 words, from the host
    cap = gal._emb.size(0)
    assert gal.add(d.g[1000:], tags=torch.from_numpy(tag[1000:]).cuda()) == 1000 and gal._emb.size(0) > cap      # grows
    assert len(gal) == G and gal.tags.dtype == torch.int32 and torch.equal(gal.tags, dev(tag)) and torch.equal(gal.norms, d.norms)
    for k in (10, 128):
        assert same(gal.search(d.q, k, mask=mt), expect(d, tag, mask, k))
    assert same(gal.search(d.q, 10, mask=torch.from_numpy(mask)), expect(d, tag, mask, 10))       # int64 words
    assert same(gal.search(d.q, 10, mask=B31), expect(d, tag, np.full(Q, B31), 10))                 # an int: every probe
    (bs, bi), (ws, wi) = gal.search(d.q, 10, index_base=1 << 33, mask=mt), expect(d, tag, mask, 10)
    assert torch.equal(bs, ws) and torch.equal(bi, torch.where(wi >= 0, wi + (1 << 33), wi))
    assert same(gal.search(d.q, 10), eng.search(d.q, d.g, 10, gallery_norms=d.norms))              # mask=None: today's path
    assert same(gal.search(d.q, 10, mask=None), eng.search(d.q, d.g, 10, gallery_norms=d.norms))
    # set_tags: an int for all the rows named, then a word each
    tag = tag.copy()
    tag[[3, 700, 1050]] = B31 | 1
    gal.set_tags([3, 700, 1050], B31 | 1)
    rows = np.array([0, 128, 1099, 5])
    tag[rows] = [0, FULL, 2, 1 << 30]
    gal.set_tags(torch.from_numpy(rows).cuda(), torch.tensor([0, FULL, 2, 1 << 30]))
    assert torch.equal(gal.tags, dev(tag))
    assert same(gal.search(d.q, 64, mask=mt), expect(d, tag, mask, 64))
    # leave-one-out under a mask: the k + 1 route
    me = np.array([3, 128, 999, 1050])
    dm = base.Data(eng, d.g[me], d.g)
    mm = np.array([B31, FULL, 1 << 30 | 2, 4], dtype=np.int64)
    ls, li = gal.search(d.g[me], 5, self_index=torch.from_numpy(me).cuda(), mask=dev(mm))
    ws, wi = drop_self(*expect(dm, tag, mm, 6), torch.from_numpy(me).cuda())
    assert li.shape == (4, 5) and not torch.any(li == torch.from_numpy(me).cuda()[:, None]) and same((ls, li), (ws, wi))
    # a plane: with a mask the exact filtered search runs and nothing is certified; without, the shortlist as before
    gal.build_plane()
    gal.search(d.q, 10)
    assert gal.last_certified is not None
    assert same(gal.search(d.q, 10, mask=mt), expect(d, tag, mask, 10)) and gal.last_certified is None
    # what the class refuses
    for bad in (lambda: gal.add(d.g[:2]), lambda: gal.add(d.g[:2], tags=torch.tensor([1, 2, 3])), lambda: gal.add(d.g[:2], tags=-1),
                lambda: gal.add(d.g[:2], tags=1 << 32), lambda: gal.add(d.g[:2], tags=torch.tensor([1.0, 2.0])),
                lambda: gal.set_tags([G], 1), lambda: gal.set_tags([-1], 1), lambda: gal.set_tags([1, 2], torch.tensor([1])),
                lambda: gal.set_subject_tags([1], 1), lambda: gal.search(d.q, 5, mask=torch.tensor([1, 2])),
                lambda: Gallery(eng).add(d.g[:2], tags=1), lambda: Gallery(eng).tags, lambda: Gallery(eng).set_tags([0], 1)):
        with pytest.raises(RuntimeError):
            bad()
    # tags switched on for a gallery that holds rows
    late = Gallery(eng)
    late.add(d.g[:300])
    late.build_tags(6)
    assert torch.equal(late.tags, torch.full((300,), 6, device='cuda', dtype=torch.int32))
    got = late.search(d.q, 5, mask=torch.from_numpy(mask_set('single', Q)))
    assert same(got, tuple(torch.from_numpy(x).cuda() for x in fref.search_ref(d.S[:, :300], np.full(300, 6), mask_set('single', Q), 5)[:2]))


def test_gallery_with_tags_and_subjects(eng, data):
    d, tag = _grown(eng, data['small'], 100, 6)
    Q, G = d.q.size(0), d.g.size(0)
    subj = base.layout('runs', G)
    st = torch.from_numpy(subj).cuda()
    mask = mask_set('mixed', Q)
    mt = dev(mask)
    gal = Gallery(eng, subjects=True)
    gal.build_tags()
    for lo, hi in ((0, 600), (600, 1000), (1000, G)):
        assert gal.add(d.g[lo:hi], st[lo:hi], tags=dev(tag[lo:hi])) == lo
    assert torch.equal(gal.tags, dev(tag)) and torch.equal(gal.subjects, st)

    def check(dd, tg, sj):
        s, u, i = gal.search_subjects(dd.q, 10, mask=mt)
        assert same((s, i, u), expect(dd, tg, mask, 10, sj, True))
        rs, ri = gal.search(dd.q, 64, mask=mt)
        assert same((rs, ri), expect(dd, tg, mask, 64, sj, False)[:2])
    check(d, tag, subj)
    s, u, i = gal.search_subjects(d.q, 10)                       # mask=None: today's path
    assert same((s, i, u), eng.search_subjects(d.q, d.g, st, 10, gallery_norms=d.norms))
    assert same(gal.search(d.q, 10, mask=None), eng.search_subjects(d.q, d.g, st, 10, gallery_norms=d.norms, distinct=False)[:2])
    # set_subject_tags: a word per subject, in any order of the ids, then an int for several
    ids = [int(subj[500]), int(subj[3]), int(subj[1050])]
    wds = [B31, 5, 1 << 20]
    tag = tag.copy()
    for u_, w in zip(ids, wds):
        tag[subj == u_] = w
    assert gal.set_subject_tags(ids, torch.tensor(wds)) == int(np.isin(subj, ids).sum())
    tag[np.isin(subj, [int(subj[7]), int(subj[900])])] = FULL
    gal.set_subject_tags(torch.tensor([int(subj[7]), int(subj[900])]), FULL)
    assert torch.equal(gal.tags, dev(tag))
    check(d, tag, subj)
    # remove, then compact: the tags move with their rows
    gone = [int(subj[10]), int(subj[640]), int(subj[1099])] + list(range(200, 260))
    subj2 = subj.copy()
    subj2[np.isin(subj, gone)] = -1
    assert gal.remove(gone) == int(np.isin(subj, gone).sum())
    check(d, tag, subj2)
    assert gal.set_subject_tags(gone, 1) == 0                    # removed rows belong to nobody
    old_to_new = gal.compact()
    keep = subj2 >= 0
    kt = torch.from_numpy(keep).cuda()
    assert len(gal) == int(keep.sum()) and torch.equal(gal.tags, dev(tag[keep])) and torch.equal(gal.subjects, st[kt])
    assert torch.equal(gal.embeddings, d.g[kt]) and torch.equal(old_to_new[kt], torch.arange(len(gal), device='cuda'))
    dc = base.Data.__new__(base.Data)
    dc.q, dc.g, dc.norms, dc.S = d.q, d.g[kt], d.norms[kt], np.ascontiguousarray(d.S[:, keep])
    dc.order = sref.row_order(dc.S)
    check(dc, tag[keep], subj2[keep])
    # a plane under subjects: the mask takes the exact filtered entry
    gal.build_plane()
    gal.search_subjects(d.q, 10)
    assert gal.last_certified is not None
    check(dc, tag[keep], subj2[keep])
    assert gal.last_certified is None
    with pytest.raises(RuntimeError):
        gal.set_subject_tags([1, 2], torch.tensor([1]))
    with pytest.raises(RuntimeError):
        gal.add(d.g[:2], st[:2])
    # one process is one shard: the sharded form is the gallery's search with the mask
    s, u, i = search_sharded_filtered(gal, d.q, 10, mt, distinct=True)
    assert same((s, i, u), expect(dc, tag[keep], mask, 10, subj2[keep], True))
    assert same(search_sharded_filtered(gal, d.q, 10, mt), expect(dc, tag[keep], mask, 10, subj2[keep], False)[:2])
    assert same(search_sharded(gal, d.q, 10), gal.search(d.q, 10))


def _rc(eng, *args):
    return eng.lib.ffr_search_topk_filtered(eng._h, *args)


def test_arguments(eng):
    q, g = base.rand_rows(4, 51), base.rand_rows(100, 52)
    n = eng.row_norms(g)
    sub = torch.arange(101, device='cuda', dtype=torch.int32)
    tag = torch.full((101,), 3, device='cuda', dtype=torch.int32)
    m = torch.full((5,), 1, device='cuda', dtype=torch.int32)
    s = torch.empty((4, 129), device='cuda')
    i = torch.empty((4, 129), device='cuda', dtype=torch.int64)
    u = torch.empty((4, 129), device='cuda', dtype=torch.int32)
    P = native._ptr
    st = eng._stream()
    null = C.c_void_p(0)
    ok = (P(q), P(m), 4, P(g), P(n), P(tag), P(sub), 100, 512, 10, 0, 1, P(s), P(i), P(u), st)
    names = ['q', 'm', 'Q', 'g', 'n', 'tag', 'sub', 'G', 'dim', 'k', 'base', 'distinct', 's', 'i', 'u', 'st']

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[names.index(key)] = v
        return _rc(eng, *a)

    def off(t, nbytes):
        return C.c_void_p(t.data_ptr() + nbytes)

    assert call() == 0 and call(distinct=0) == 0 and call(sub=null, u=null, distinct=0) == 0
    assert call(dim=256) == -6 and b'ffr_search_topk_filtered' in eng.lib.ffr_last_error(eng._h)
    for bad in (dict(m=null), dict(tag=null), dict(m=off(m, 2)), dict(tag=off(tag, 2)), dict(m=off(m, 1)), dict(sub=null, u=null),
                dict(u=null), dict(sub=null),
                # what ffr_search_topk_subjects rejects
                dict(k=0), dict(k=129, distinct=0), dict(Q=0), dict(G=-1), dict(q=null), dict(g=null), dict(n=null), dict(s=null),
                dict(i=null), dict(sub=off(sub, 2)), dict(distinct=2), dict(distinct=-1), dict(k=65), dict(k=128),
                dict(q=off(q, 4)), dict(g=off(g, 8))):
        assert call(**bad) == -1, bad
        assert b'ffr_search_topk_filtered' in eng.lib.ffr_last_error(eng._h), bad
    assert call(k=64) == 0 and call(k=128, distinct=0) == 0 and call(k=128, distinct=0, sub=null, u=null) == 0
    assert call(m=off(m, 4), tag=off(tag, 4)) == 0                   # 4-byte alignment is all the words need
    torch.cuda.synchronize()
    s.fill_(0), i.fill_(0), u.fill_(0)
    assert call(G=0, g=null, n=null, tag=null, sub=null) == 0        # G = 0: all padding, NULL gallery pointers allowed
    torch.cuda.synchronize()
    assert torch.all(i.reshape(-1)[:40] == -1) and torch.all(u.reshape(-1)[:40] == -1) and torch.all(s.reshape(-1)[:40] == float('-inf'))
    u.fill_(7)
    assert call(G=0, g=null, n=null, tag=null, sub=null, u=null, distinct=0) == 0
    assert call(G=0, g=null, n=null, tag=null, sub=null, u=null, distinct=1) == -1
    assert call(G=0, g=null, n=null, tag=null, sub=null, m=null) == -1
    assert call(sub=null, u=null, distinct=0) == 0                    # without subjects top_subject is not touched
    torch.cuda.synchronize()
    assert torch.all(u == 7)
    # the binding
    tag, sub, m = tag[:100], sub[:100], m[:4]
    es, ei = eng.search_filtered(q, m, g[:0], tag[:0], 5)
    assert torch.all(ei == -1) and torch.all(es == float('-inf'))
    assert len(eng.search_filtered(q, m, g[:0], tag[:0], 5, subjects=sub[:0], distinct=True)) == 3
    assert eng.search_filtered(q, m, g, tag, 128)[1].shape == (4, 128)
    a = eng.search_filtered(q, m, g, tag, 10, subjects=sub, distinct=True)
    assert same(a, eng.search_filtered(q, m.to(torch.int64), g, tag.to(torch.int64), 10, subjects=sub.to(torch.int64), distinct=True))
    assert same(a, eng.search_filtered(q, 1, g, tag, 10, subjects=sub, distinct=True))
    for bad in (lambda: eng.search_filtered(q, m, g, tag, 10, distinct=True), lambda: eng.search_filtered(q, m, g, tag, 65, subjects=sub, distinct=True),
                lambda: eng.search_filtered(q, m, g, tag, 129), lambda: eng.search_filtered(q, m[:3], g, tag, 10),
                lambda: eng.search_filtered(q, m, g, tag[:99], 10), lambda: eng.search_filtered(q, m.float(), g, tag, 10),
                lambda: eng.search_filtered(q, m, g, tag.to(torch.int16), 10), lambda: eng.search_filtered(q, -1, g, tag, 10),
                lambda: eng.search_filtered(q, 1 << 32, g, tag, 10), lambda: eng.search_filtered(q, m, g, tag.to(torch.int64) - 4, 10),
                lambda: eng.search_filtered(q, m, g, tag, 10, subjects=sub[:99]), lambda: eng.search_filtered(q.cpu(), m, g, tag, 10)):
        with pytest.raises(RuntimeError):
            bad()


def test_profile_counts_one_launch_under_score(eng):
    Q, G = 40, 5000
    q, g = base.rand_rows(Q, 61), base.rand_rows(G, 62)
    n = eng.row_norms(g)
    sub = (torch.arange(G, device='cuda') // 8).to(torch.int32)
    tag, m = dev(tag_layout('bit', G)), dev(mask_set('mixed', Q))
    torch.cuda.synchronize()

    def profiled(fn):
        eng.profile_enable(True)
        eng.profile_read()
        fn()
        st = eng.profile_read()
        eng.profile_enable(False)
        assert st['score']['launches'] == 1 and st['score']['flops'] == 2.0 * Q * G * 512 and st['score']['ms'] > 0
        assert sum(v['launches'] for k, v in st.items() if k != 'score') == 0
        return st['score']['bytes']
    for distinct in (True, False):
        got = profiled(lambda: eng.search_filtered(q, m, g, tag, 10, gallery_norms=n, subjects=sub, distinct=distinct))
        assert got == profiled(lambda: eng.search_subjects(q, g, sub, 10, gallery_norms=n, distinct=distinct)) + 4.0 * G + 4.0 * Q
    got = profiled(lambda: eng.search_filtered(q, m, g, tag, 10, gallery_norms=n))
    assert got == profiled(lambda: eng.search(q, g, 10, gallery_norms=n)) + 4.0 * G + 4.0 * Q
