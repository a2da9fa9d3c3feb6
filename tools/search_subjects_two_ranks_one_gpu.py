"""Sharded identity search with two ranks on ONE GPU over gloo (RCCL refuses two ranks on one device): each rank enrols a
contiguous shard of one subject-labelled gallery (uneven sizes, subjects spread over both shards, some withdrawn) and calls
ffrnet_amd.search_sharded(..., distinct=True); every rank's result must equal the single-process identity search over the
whole gallery, bitwise.  The row search of the same shards (removed rows masked) is checked the same way."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G, Q, SPLIT = 20001, 37, 7003


def rows(n, seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return torch.randn((n, 512), device='cuda', generator=g)


def worker(rank, world, port, q):
    try:
        run(rank, world, port, q)
    except Exception:            # report instead of leaving the parent waiting on the queue
        import traceback
        q.put((rank, ['ERROR ' + traceback.format_exc()]))
        raise


def run(rank, world, port, q):
    import ffrnet_amd
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    eng = ffrnet_amd.Engine(0)
    gal, probes = rows(G, 1), rows(Q, 2)
    subj = (torch.arange(G, device='cuda') * 7919 % 2500).to(torch.int32)       # ~8 rows per subject, in both shards
    lo, hi = (0, SPLIT) if rank == 0 else (SPLIT, G)
    shard = ffrnet_amd.Gallery(eng, subjects=True)
    shard.add(gal[lo:hi], subj[lo:hi])
    gone = list(range(0, 2500, 9))
    shard.remove(gone)
    subj[torch.isin(subj, torch.tensor(gone, device='cuda', dtype=torch.int32))] = -1
    res = []
    for k in (10, 64):
        s, u, i = ffrnet_amd.search_sharded(shard, probes, k, distinct=True)
        ws, wi, wu = eng.search_subjects(probes, gal, subj, k, distinct=True)
        res.append(bool(torch.equal(s, ws) and torch.equal(i, wi) and torch.equal(u, wu)))
    s, i = ffrnet_amd.search_sharded(shard, probes, 128)
    ws, wi, _ = eng.search_subjects(probes, gal, subj, 128, distinct=False)
    res.append(bool(torch.equal(s, ws) and torch.equal(i, wi)))
    torch.cuda.synchronize()
    q.put((rank, res))
    dist.destroy_process_group()


if __name__ == '__main__':
    import socket
    sk = socket.socket()
    sk.bind(('127.0.0.1', 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=240) for _ in procs)
        for p in procs:
            p.join(60)
    finally:
        for p in procs:         # a rank that failed must not leave its peer waiting in a collective
            if p.is_alive():
                p.terminate()
    print('per rank, identity k = 10 / 64 and rows k = 128, equal to the single search:', res)
    assert all(r == [True, True, True] for _, r in res)
    print('OK')
