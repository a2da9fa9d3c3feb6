#!/usr/bin/env python3
"""From unlabelled faces to an enrolled gallery on synthetic images (needs an MI355X): embed -> cluster -> templates ->
Gallery.add -> search.

    python examples/cluster_synthetic.py [--identities 24] [--views 4]

An "identity" is a random image, a "view" of it the same image under pixel noise.  With real weights and faces, take the
threshold from the verification protocol: ffrnet_amd.lfw.get_avg_accuracy(encoder, recnet, loader, details=True)[2]
['folds_new'] holds (best_threshold, accuracy) per fold; pass the mean threshold.  Here, with random weights, it is the
midpoint between the mean same-identity and the mean different-identity score of the collection itself.
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
    # the collection: views of every identity, shuffled; `who` is the ground truth a real collection does not have
    n = a.identities * a.views
    who = torch.arange(a.identities).repeat_interleave(a.views)
    imgs = (synth.synth_images(a.identities, seed=11)[who] + a.noise * synth.synth_images(n, seed=12)).clamp(-1, 1)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(13))
    imgs, who = imgs[perm], who[perm]
    f_new, _ = eng.embed(imgs.cuda(), want_f=False)                       # [n,512] on the device

    s, i = eng.search(f_new, f_new, n)                                    # every pair's score, to pick a threshold here
    scores = torch.empty((n, n), device='cuda').scatter_(1, i, s).cpu()
    same = who[:, None] == who[None, :]
    off = ~torch.eye(n, dtype=torch.bool)
    threshold = 0.5 * (scores[same & off].mean().item() + scores[~same].mean().item())

    c = cluster.cluster(eng, f_new, threshold)                            # rep, dense ids, sizes
    p, r, f = cluster.pairwise_scores(c.cluster_id, who)
    print('%d faces of %d identities, threshold %.4f -> %d clusters (sizes %d..%d); pairwise precision %.3f recall %.3f F %.3f'
          % (n, a.identities, threshold, c.n_clusters, int(c.sizes.min()), int(c.sizes.max()), p, r, f))
    gallery = ffrnet_amd.Gallery(eng)
    gallery.add(cluster.templates(eng, f_new, c))                         # one row per cluster: row r is cluster id r
    top_s, top_i = gallery.search(f_new, k=1)
    hit = (top_i[:, 0] == c.cluster_id).double().mean().item()
    print('searching every face against the %d templates: its own cluster comes first for %.1f %% of them' % (len(gallery), 100 * hit))


if __name__ == '__main__':
    main()
