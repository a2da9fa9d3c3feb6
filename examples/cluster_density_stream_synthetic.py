#!/usr/bin/env python3
"""A collection that arrives in batches, clustered with density gating, on synthetic images (needs an MI355X): per batch
embed -> IncrementalDensity.add; at the end the templates of the clusters with a core -> Gallery.add -> search
(INTEGRATION.md section 9).

    python examples/cluster_density_stream_synthetic.py [--identities 24] [--views 6] [--min-rows 4] [--strays 8]

The collection of examples/cluster_density_synthetic.py (identities seen several times, strays seen once), shuffled and
delivered in three batches.  Every add scores the new faces against everything held and among themselves, and the old
faces that the batch made core against the old ones; the labels after each batch are those of one density() over all faces
held (checked at the end).  An identity whose views are spread over the batches is noise at first and becomes a cluster
when enough of them have arrived; density_changes tells which templates a caller that keeps them would drop and compute.
"""
import argparse, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd
from ffrnet_amd import cluster, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--identities', type=int, default=24)
    ap.add_argument('--views', type=int, default=6)
    ap.add_argument('--strays', type=int, default=8)
    ap.add_argument('--min-rows', type=int, default=4)
    ap.add_argument('--noise', type=float, default=0.25)
    a = ap.parse_args()
    specs = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'g0_state_dict_keys.json')))
    eng = ffrnet_amd.Engine(0)
    eng.load_encoder(synth.synth_state_dict(specs['encoder']))
    eng.load_recnet(synth.synth_state_dict(specs['recnet']))
    n = a.identities * a.views + a.strays
    who = torch.cat((torch.arange(a.identities).repeat_interleave(a.views), a.identities + torch.arange(a.strays)))
    imgs = (synth.synth_images(a.identities + a.strays, seed=11)[who] + a.noise * synth.synth_images(n, seed=12)).clamp(-1, 1)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(13))
    imgs, who = imgs[perm], who[perm]

    # the threshold of this toy collection, picked as in examples/cluster_density_synthetic.py
    f_all, _ = eng.embed(imgs.cuda(), want_f=False)
    s, i = eng.search(f_all, f_all, min(n, 128))
    same = who.cuda()[i] == who.cuda()[:, None]
    own = i == torch.arange(n, device='cuda')[:, None]
    threshold = 0.5 * (s[same & ~own].mean().item() + s[~same].mean().item())

    store = cluster.IncrementalDensity(eng, threshold, a.min_rows)
    for k, batch in enumerate(torch.tensor_split(torch.arange(n), 3)):
        before = store.rep.clone()
        f_new, _ = eng.embed(imgs[batch].cuda(), want_f=False)            # only the new images are embedded
        first = store.add(f_new)
        gone, recompute = cluster.density_changes(before, store.rep)
        c = store.clusters
        kinds = torch.bincount(c.kind.long(), minlength=3).tolist()
        print('batch %d: rows %d..%d -> %d core, %d border, %d noise rows, %d clusters with a core; %d earlier representatives gone'
              % (k, first, len(store) - 1, kinds[2], kinds[1], kinds[0], int(c.has_core.sum()), gone.numel()))
    c = store.clusters
    once = cluster.density(eng, store.embeddings, threshold, a.min_rows)
    p, r, f = cluster.pairwise_scores(c.cluster_id, who)
    print('equal to one density() over all %d faces: %s; pairwise precision %.3f recall %.3f F %.3f'
          % (n, bool(torch.equal(c.rep, once.rep) and torch.equal(c.kind, once.kind)), p, r, f))
    gallery = ffrnet_amd.Gallery(eng)
    gallery.add(store.templates())                                        # the clusters with a core; noise is not enrolled
    row_of = torch.cumsum(c.has_core.long(), 0) - 1                       # cluster id -> gallery row
    member = c.kind > 0
    top_s, top_i = gallery.search(store.embeddings[member], k=1)
    hit = (top_i[:, 0] == row_of[c.cluster_id[member]]).double().mean().item()
    print('searching the %d clustered faces against the %d templates: the own cluster comes first for %.1f %% of them'
          % (int(member.sum()), len(gallery), 100 * hit))


if __name__ == '__main__':
    main()
