"""What the four search entries (include/ffrnet.h: ffr_search_topk, ffr_search_topk_subjects, ffr_search_topk_coarse,
ffr_search_topk_coarse_subjects) share behind the C ABI, seen from outside: every entry names itself in its own messages, the
coarse entries hand G = 0 and a k above their pass to the exact search as ONE profiled launch with the exact entry's counts,
and a coarse search proper counts one launch of 2 Q G 512 flops.

One shape: Q = 33 (two probe tiles, the second with one probe), G = 300 (three chunks of 128 rows on a 256-CU part, so the
chunk merge runs and the last chunk is partial), k = 10; subjects are row // 3, the rows of subject 7 removed.  Sharding by
hand (topk_merge / topk_merge_subjects with index_base) is left to test_shard_merge_equals_single_search of
test_gpu_search.py and test_gpu_search_subjects.py, which cover its three modes."""
import ctypes as C

import pytest
import torch

import ffrnet_amd
from ffrnet_amd import native
from ffrnet_amd.search import shortlist_size

pytestmark = pytest.mark.gpu

Q, G, K, DIM = 33, 300, 10, 512
ENTRIES = ('ffr_search_topk', 'ffr_search_topk_subjects', 'ffr_search_topk_coarse', 'ffr_search_topk_coarse_subjects')


class Data(object):
    pass


@pytest.fixture(scope='module')
def eng():
    return ffrnet_amd.Engine(0)


@pytest.fixture(scope='module')
def d(eng):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1234)
    d = Data()
    d.q = torch.randn((Q, DIM), device='cuda', generator=gen)
    d.g = torch.randn((G, DIM), device='cuda', generator=gen)
    d.n = eng.row_norms(d.g)
    d.sub = (torch.arange(G, device='cuda') // 3).to(torch.int32)
    d.sub[d.sub == 7] = -1
    d.plane = torch.empty((G, DIM), device='cuda', dtype=torch.int16)
    d.flag = torch.zeros((1,), device='cuda', dtype=torch.int32)
    eng.coarse_pack(d.g, d.n, d.plane, d.flag)
    torch.cuda.synchronize()
    return d


def run(eng, d, entry, k, q=None, G=G, distinct=True, cert=False):
    """One call of `entry` through Engine over the first G rows"""
    q = d.q if q is None else q
    g, n, sub, plane = d.g[:G], d.n[:G], d.sub[:G], d.plane[:G]
    if entry == 'ffr_search_topk':
        return eng.search(q, g, k, gallery_norms=n)
    if entry == 'ffr_search_topk_subjects':
        return eng.search_subjects(q, g, sub, k, gallery_norms=n, distinct=distinct)
    if entry == 'ffr_search_topk_coarse':
        return eng.search_coarse(q, g, plane, d.flag, k, gallery_norms=n, return_certified=cert)
    return eng.search_coarse_subjects(q, g, plane, d.flag, sub, k, gallery_norms=n, distinct=distinct, return_certified=cert)


def message(eng, fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    text = str(e.value)
    print(text)
    return text


def test_each_entry_names_itself(eng, d):
    buf = torch.empty((Q * DIM + 1,), device='cuda')
    qmis = buf[1:].view(Q, DIM)                 # contiguous, and one float past a 16-byte boundary
    qmis.copy_(d.q)
    assert qmis.is_contiguous() and qmis.data_ptr() % 16 == 4
    P = native._ptr
    off2 = C.c_void_p(d.sub.data_ptr() + 2)
    s = torch.empty((Q, K), device='cuda')
    i = torch.empty((Q, K), device='cuda', dtype=torch.int64)
    u = torch.empty((Q, K), device='cuda', dtype=torch.int32)
    raw = {'ffr_search_topk_subjects': (P(d.q), Q, P(d.g), P(d.n), off2, G, DIM, K, 0, 1, P(s), P(i), P(u), eng._stream()),
           'ffr_search_topk_coarse_subjects': (P(d.q), Q, P(d.g), P(d.n), P(d.plane), P(d.flag), off2, G, DIM, K, 0, 1, P(s),
                                               P(i), P(u), C.c_void_p(0), eng._stream())}
    for entry in ENTRIES:
        coarse, subj = 'coarse' in entry, 'subjects' in entry
        pre = 'ffrnet native error -1: ' + entry + ': '
        rows = 'query, gallery and plane rows' if coarse else 'query and gallery rows'
        assert message(eng, lambda: run(eng, d, entry, K, q=qmis)) == pre + rows + ' must be 16-byte aligned'
        assert message(eng, lambda: run(eng, d, entry, 0)) == \
            pre + 'bad arguments (Q >= 1, 1 <= k <= 128, G >= 0, non-null pointers)'
        if subj:
            assert message(eng, lambda: run(eng, d, entry, 65, distinct=True)) == pre + 'identity mode serves k <= 64, got 65'
            assert getattr(eng.lib, entry)(eng._h, *raw[entry]) == -1
            text = eng.lib.ffr_last_error(eng._h).decode()
            print(text)
            assert text == entry + ': gallery_subject must be 4-byte aligned'


def profiled(eng, fn):
    """fn() once to grow the scratch, then once more under the profile -> (its result, the profile)"""
    fn()
    torch.cuda.synchronize()
    eng.profile_enable(True)
    eng.profile_read()
    out = fn()
    st = eng.profile_read()
    eng.profile_enable(False)
    print({k: (v['launches'], v['flops'], v['bytes']) for k, v in st.items() if v['launches']})
    return out, st


def one_score_launch(st, flops):
    return (st['score']['launches'] == 1 and st['score']['flops'] == flops and
            sum(v['launches'] for k, v in st.items() if k != 'score') == 0)


@pytest.mark.parametrize('coarse,exact,rows,k,distinct', [
    ('ffr_search_topk_coarse', 'ffr_search_topk', 0, K, False),
    ('ffr_search_topk_coarse_subjects', 'ffr_search_topk_subjects', 0, K, True),
    ('ffr_search_topk_coarse_subjects', 'ffr_search_topk_subjects', 0, K, False),
    ('ffr_search_topk_coarse', 'ffr_search_topk', G, 65, False),
    ('ffr_search_topk_coarse_subjects', 'ffr_search_topk_subjects', G, 33, True),
    ('ffr_search_topk_coarse_subjects', 'ffr_search_topk_subjects', G, 128, False)])
def test_coarse_entries_delegate_to_the_exact_search(eng, d, coarse, exact, rows, k, distinct):
    """G = 0, or a k above the pass (64 rows, 32 identities): the exact entry's results, profile and counts; nothing certified"""
    assert rows == 0 or shortlist_size(k, distinct) is None
    want, st_e = profiled(eng, lambda: run(eng, d, exact, k, G=rows, distinct=distinct))
    got, st_c = profiled(eng, lambda: run(eng, d, coarse, k, G=rows, distinct=distinct, cert=True))
    assert len(got) == len(want) + 1
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == (Q, k) and torch.equal(a, b)
    assert got[-1].shape == (Q,) and got[-1].dtype == torch.int32 and not bool(got[-1].any())
    assert one_score_launch(st_e, 2.0 * Q * rows * DIM) and one_score_launch(st_c, 2.0 * Q * rows * DIM)
    assert st_c['score']['bytes'] == st_e['score']['bytes'] > 0


@pytest.mark.parametrize('coarse,exact,distinct', [('ffr_search_topk_coarse', 'ffr_search_topk', False),
                                                   ('ffr_search_topk_coarse_subjects', 'ffr_search_topk_subjects', True),
                                                   ('ffr_search_topk_coarse_subjects', 'ffr_search_topk_subjects', False)])
def test_profile_of_the_coarse_pass(eng, d, coarse, exact, distinct):
    """The pass proper at the shape above: one launch under `score`, 2 Q G 512 flops, the bytes of the coarse formula; and the
    exact entry's results"""
    kp = shortlist_size(K, distinct)
    subj = 'subjects' in coarse
    got, st = profiled(eng, lambda: run(eng, d, coarse, K, distinct=distinct, cert=True))
    want = run(eng, d, exact, K, distinct=distinct)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == (Q, K) and torch.equal(a, b)
    assert one_score_launch(st, 2.0 * Q * G * DIM)
    assert st['score']['bytes'] == 2.0 * G * (DIM + 2) + 4.0 * Q * DIM + 12.0 * Q * (K + kp) + (4.0 * G + 4.0 * Q * K if subj else 0.0)
