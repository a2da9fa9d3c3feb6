"""Host side of the uint8 input path (no GPU): ShardFeeder on decoded uint8 images with per-pair flip flags, the
sharded verification harness with a uint8 loader on 2 gloo ranks, and the refusal of embed functions that do not take
uint8 images."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ffrnet_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u8_loader(n_pairs=21, bs=8, h=112, w=112, seed=3):
    i1, i2, lab, flip = ffrnet_amd.synth.synth_pairs_u8(n_pairs, h, w, seed=seed, block=6)
    return [dict(img1=i1[s:s + bs], img2=i2[s:s + bs], label=lab[s:s + bs], idx=torch.arange(s, min(s + bs, n_pairs)),
                 flip=flip[s:s + bs]) for s in range(0, n_pairs, bs)], (i1, i2, lab, flip)


def test_synth_uint8_generators_are_seeded():
    a = ffrnet_amd.synth.synth_pairs_u8(9, 16, 16, seed=4, block=6)
    b = ffrnet_amd.synth.synth_pairs_u8(9, 16, 16, seed=4, block=6)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    i1, i2, lab, flip = a
    assert i1.dtype == torch.uint8 and tuple(i1.shape) == (9, 16, 16, 3) and i2.shape == i1.shape
    assert flip.dtype == torch.bool and flip.numel() == 9 and 0 < int(flip.sum()) < 9
    non, ocl, label, fl = ffrnet_amd.synth.synth_train_batch_u8(6, seed=5)
    assert non.dtype == torch.uint8 and tuple(non.shape) == (6, 112, 112, 3) and ocl.shape == non.shape
    assert label.numel() == 6 and fl.numel() == 6
    img = ffrnet_amd.synth.synth_images_u8(3, 32, 16, seed=1)
    assert img.dtype == torch.uint8 and tuple(img.shape) == (3, 32, 16, 3)
    assert torch.equal(img, ffrnet_amd.synth.synth_images_u8(3, 32, 16, seed=1))


def test_shard_feeder_uint8_shards_images_and_flips():
    """device=None: every rank gets exactly its image and flip shards, as uint8; the byte counts are uint8 bytes."""
    loader, (i1, i2, _, flip) = _u8_loader(21, 8, 8, 8)
    world = 4
    seen = []
    for r in range(world):
        fd = ffrnet_amd.lfw.ShardFeeder(loader, r, world, device=None)
        pairs = 0
        for (data, both, m, n), s0 in zip(fd, (0, 8, 16)):
            lo, hi = ffrnet_amd.lfw.shard_bounds(n, r, world)
            assert m == hi - lo
            if m:
                assert both.dtype == torch.uint8
                assert torch.equal(both[:m], i1[s0 + lo:s0 + hi]) and torch.equal(both[m:], i2[s0 + lo:s0 + hi])
                want = flip[s0 + lo:s0 + hi].to(torch.uint8)
                assert fd.pair_flip.dtype == torch.uint8 and torch.equal(fd.pair_flip, want)
                assert torch.equal(fd.flip, torch.cat((want, want)))
                seen += range(s0 + lo, s0 + hi)
                pairs += m
            else:
                assert both is None and fd.flip is None and fd.pair_flip is None
        st = fd.stats
        assert st['batches'] == 3 and st['h2d_bytes'] == 0
        assert st['shard_bytes'] == 2 * pairs * 8 * 8 * 3
        assert st['full_batch_bytes'] == 2 * 21 * 8 * 8 * 3
    assert sorted(seen) == list(range(21))


def test_shard_feeder_refusals():
    i1, i2, lab, flip = ffrnet_amd.synth.synth_pairs_u8(4, 8, 8, seed=1, block=2)
    mixed = [dict(img1=i1, img2=i2.float(), label=lab, idx=torch.arange(4))]
    with pytest.raises(RuntimeError, match='one image type'):
        list(ffrnet_amd.lfw.ShardFeeder(mixed, 0, 1, None))
    short = [dict(img1=i1, img2=i2, label=lab, idx=torch.arange(4), flip=flip[:3])]
    with pytest.raises(RuntimeError, match='flag per pair'):
        list(ffrnet_amd.lfw.ShardFeeder(short, 0, 1, None))
    # float images arrive preprocessed: a flip entry next to them is not applied again
    f1 = torch.zeros(4, 3, 8, 8)
    fl = ffrnet_amd.lfw.ShardFeeder([dict(img1=f1, img2=f1, label=lab, idx=torch.arange(4), flip=flip)], 0, 1, None)
    for _ in fl:
        assert fl.flip is None


def test_foreign_embed_without_accepts_uint8_is_refused():
    loader, _ = _u8_loader(5, 8, 16, 16)

    def embed(img):
        return img.float().reshape(img.size(0), -1), img.float().reshape(img.size(0), -1)
    with pytest.raises(RuntimeError, match='accepts_uint8'):
        ffrnet_amd.lfw.calculate_distance(loader, embed)
    with pytest.raises(RuntimeError, match='accepts_uint8'):
        ffrnet_amd.lfw.get_avg_accuracy(embed, loader)


_WORKER = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, 'oracle'))
import ffrnet_amd
import ffr_oracle as O
rank, world = int(sys.argv[1]), int(sys.argv[2])
os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = sys.argv[3]
dist.init_process_group('gloo', rank=rank, world_size=world)
P = torch.randn(3 * 16 * 16, 512, generator=torch.Generator().manual_seed(5)) / 10
def embed(img):                      # stand-in embedder on float images (host-logic test, CPU)
    e = img.reshape(img.size(0), -1) @ P
    return e, torch.tanh(e)
calls = []
def embed_u8(img, flip):             # its uint8 twin: the loader's input step, then the same embedder
    calls.append((img.dtype, img.size(0), None if flip is None else flip.tolist()))
    return embed(O.preprocess_u8(img, flip))
embed_u8.accepts_uint8 = True
i1, i2, lab, flip = ffrnet_amd.synth.synth_pairs_u8(21, 16, 16, seed=3, block=6)
u8 = [dict(img1=i1[s:s+8], img2=i2[s:s+8], label=lab[s:s+8], idx=torch.arange(s, min(s+8, 21)), flip=flip[s:s+8])
      for s in (0, 8, 16)]
fp = [dict(img1=O.preprocess_u8(i1[s:s+8], flip[s:s+8]), img2=O.preprocess_u8(i2[s:s+8], flip[s:s+8]), label=lab[s:s+8],
           idx=torch.arange(s, min(s+8, 21))) for s in (0, 8, 16)]
a = np.concatenate(ffrnet_amd.lfw.calculate_distance(u8, embed_u8), 1)
sa = dict(ffrnet_amd.lfw.last_feed_stats)
b = np.concatenate(ffrnet_amd.lfw.calculate_distance(fp, embed), 1)
sb = dict(ffrnet_amd.lfw.last_feed_stats)
np.save(sys.argv[4] + '.%%d.npy' %% rank, np.stack([a, b]))
print('calls', rank, [(str(d), n) for d, n, _ in calls])
lo = [ffrnet_amd.lfw.shard_bounds(n, rank, world) for n in (8, 8, 5)]
want = [f[s + l:s + h].to(torch.uint8).tolist() * 2 for (l, h), s, f in zip(lo, (0, 8, 16), [flip] * 3)]
print('flips', rank, [c[2] for c in calls] == want)
print('bytes', rank, sa['shard_bytes'] * 4 == sb['shard_bytes'], sa['full_batch_bytes'] * 4 == sb['full_batch_bytes'])
dist.destroy_process_group()
'''


def test_uint8_verification_two_ranks_gloo(tmp_path):
    """world_size 2 over gloo: calculate_distance with a uint8 loader (per-pair flips) and an accepts_uint8 embed
    function gives exactly the result of its float twin fed the preprocessed images; each rank's function sees its
    shard as uint8 with the pair flags repeated for both halves."""
    script = tmp_path / 'worker.py'
    script.write_text(_WORKER % {'root': ROOT})
    port = str(31500 + os.getpid() % 2000)
    out = str(tmp_path / 'res')
    procs = [subprocess.Popen([sys.executable, str(script), str(r), '2', port, out],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), logs
    r0, r1 = np.load(out + '.0.npy'), np.load(out + '.1.npy')
    assert np.array_equal(r0, r1)
    assert np.array_equal(r0[0], r0[1])
    assert r0.shape == (2, 21, 6)
    assert "calls 0 [('torch.uint8', 8), ('torch.uint8', 8), ('torch.uint8', 6)]" in logs[0], logs[0]
    assert "calls 1 [('torch.uint8', 8), ('torch.uint8', 8), ('torch.uint8', 4)]" in logs[1], logs[1]
    for r in range(2):
        assert 'flips %d True' % r in logs[r], logs[r]
        assert 'bytes %d True True' % r in logs[r], logs[r]
