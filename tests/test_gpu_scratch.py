"""The search and the clustering scratch of one handle are independent grow-only buffers: growing one neither moves the
other nor changes what either call returns, and generation() moves exactly with the calls that allocate."""
import pytest
import torch

import ffrnet_amd

pytestmark = pytest.mark.gpu
THR = 0.5


def test_search_and_cluster_scratch_grow_independently():
    # 2000 rows around 40 well separated centres: same centre cos ~ 0.83, other centres ~ 0
    g = torch.Generator().manual_seed(11)
    centres = torch.nn.functional.normalize(torch.randn(40, 512, generator=g), dim=1)
    rows = (centres[torch.arange(2000) % 40] + 0.02 * torch.randn(2000, 512, generator=g)).cuda().contiguous()
    query, gallery = rows[:3].contiguous(), rows[100:400].contiguous()
    eng = ffrnet_amd.Engine(0)
    try:
        def search():
            return eng.search(query, gallery, 4)

        def same(a, b):
            return all(torch.equal(x, y) for x, y in zip(a, b))

        gen = [eng.generation()]

        def step(call):
            out = call()
            gen.append(eng.generation())
            return out

        s1 = step(search)                                   # the first search allocates its scratch
        c200 = step(lambda: eng.cluster(rows[:200], THR))   # the first clustering allocates its own
        assert gen[0] != gen[1] != gen[2]
        s2 = step(search)
        assert same(s1, s2) and gen[3] == gen[2]
        c2000 = step(lambda: eng.cluster(rows, THR))        # 2000 rows: the clustering scratch grows
        assert gen[4] != gen[3]
        s3, c200b, c2000b = step(search), step(lambda: eng.cluster(rows[:200], THR)), step(lambda: eng.cluster(rows, THR))
        assert gen[5] == gen[6] == gen[7] == gen[4]
        assert same(s1, s3) and torch.equal(c200, c200b) and torch.equal(c2000, c2000b)
        # and the results are the planted ones
        assert torch.equal(c2000.cpu(), torch.arange(2000) % 40) and torch.equal(c200.cpu(), torch.arange(200) % 40)
        score, index = s1
        assert bool((score > 0.7).all()) and torch.equal((index.cpu() + 100) % 40, torch.arange(3)[:, None].expand(3, 4))
    finally:
        eng.close()
