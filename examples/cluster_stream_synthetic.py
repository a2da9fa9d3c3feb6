#!/usr/bin/env python3
"""A collection that arrives in batches, on synthetic images (needs an MI355X): per batch embed -> Incremental.add; at the
end templates -> Gallery.add -> search.

    python examples/cluster_stream_synthetic.py [--identities 24] [--views 4]

An "identity" is a random image, a "view" of it the same image under pixel noise; the shuffled views arrive in three
batches.  Every add scores the new faces against everything held and among themselves only, and the labels after the last
batch are those of one clustering of the whole collection (checked at the end).  The threshold is chosen as in
examples/cluster_synthetic.py; with real weights take it from the verification protocol.
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
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--noise', type=float, default=0.25)
    a = ap.parse_args()
    specs = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'g0_state_dict_keys.json')))
    eng = ffrnet_amd.Engine(0)
    eng.load_encoder(synth.synth_state_dict(specs['encoder']))
    eng.load_recnet(synth.synth_state_dict(specs['recnet']))
    n = a.identities * a.views
    who = torch.arange(a.identities).repeat_interleave(a.views)
    imgs = (synth.synth_images(a.identities, seed=11)[who] + a.noise * synth.synth_images(n, seed=12)).clamp(-1, 1)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(13))
    imgs, who = imgs[perm], who[perm]

    # the threshold of this toy collection: midway between its same-identity and different-identity scores
    f_all, _ = eng.embed(imgs.cuda(), want_f=False)
    s, i = eng.search(f_all, f_all, n)
    scores = torch.empty((n, n), device='cuda').scatter_(1, i, s).cpu()
    same = who[:, None] == who[None, :]
    threshold = 0.5 * (scores[same & ~torch.eye(n, dtype=torch.bool)].mean().item() + scores[~same].mean().item())

    store = cluster.Incremental(eng, threshold)
    for k, batch in enumerate(torch.tensor_split(torch.arange(n), 3)):
        before = store.rep.clone()
        f_new, _ = eng.embed(imgs[batch].cuda(), want_f=False)            # only the new images are embedded
        first = store.add(f_new)
        stale, now = cluster.changes(before, store.rep)                   # earlier clusters a new face merged into another
        c = store.clusters
        print('batch %d: rows %d..%d -> %d clusters over %d faces; %d earlier clusters absorbed'
              % (k, first, len(store) - 1, c.n_clusters, len(store), stale.numel()))
    c = store.clusters
    once = cluster.cluster(eng, store.embeddings, threshold)
    p, r, f = cluster.pairwise_scores(c.cluster_id, who)
    print('equal to one clustering of all %d faces: %s; pairwise precision %.3f recall %.3f F %.3f'
          % (n, bool(torch.equal(c.rep, once.rep)), p, r, f))
    gallery = ffrnet_amd.Gallery(eng)
    gallery.add(store.templates())                                        # one row per cluster: row r is cluster id r
    top_s, top_i = gallery.search(store.embeddings, k=1)
    hit = (top_i[:, 0] == c.cluster_id).double().mean().item()
    print('searching every face against the %d templates: its own cluster comes first for %.1f %% of them' % (len(gallery), 100 * hit))


if __name__ == '__main__':
    main()
