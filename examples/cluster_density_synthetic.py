#!/usr/bin/env python3
"""From unlabelled faces to an enrolled gallery with density-gated clustering, on synthetic images (needs an MI355X):
embed -> density -> templates of the clusters with a core -> Gallery.add -> search.

    python examples/cluster_density_synthetic.py [--identities 24] [--views 6] [--min-rows 4] [--strays 8]

An "identity" is a random image, a "view" of it the same image under pixel noise; a "stray" is an image seen once (a
passer-by).  Single link enrols every stray as a one-row identity; density() reports it as noise, and a face between two
identities as a border row that attaches to one of them without merging them.  The threshold is picked as in
examples/cluster_synthetic.py; with real weights it comes from the verification protocol.
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
    # the collection: views of every identity plus the strays, shuffled; `who` is the truth a real collection does not have
    n = a.identities * a.views + a.strays
    who = torch.cat((torch.arange(a.identities).repeat_interleave(a.views), a.identities + torch.arange(a.strays)))
    imgs = (synth.synth_images(a.identities + a.strays, seed=11)[who] + a.noise * synth.synth_images(n, seed=12)).clamp(-1, 1)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(13))
    imgs, who = imgs[perm], who[perm]
    f_new, _ = eng.embed(imgs.cuda(), want_f=False)                       # [n,512] on the device

    s, i = eng.search(f_new, f_new, min(n, 128))                          # the best scores of every face, to pick a threshold here
    same = who.cuda()[i] == who.cuda()[:, None]
    own = i == torch.arange(n, device='cuda')[:, None]
    threshold = 0.5 * (s[same & ~own].mean().item() + s[~same].mean().item())

    c = cluster.density(eng, f_new, threshold, a.min_rows)                # rep, dense ids, sizes, kind, has_core
    kinds = torch.bincount(c.kind.long(), minlength=3).tolist()
    single = cluster.cluster(eng, f_new, threshold)
    print('%d faces (%d identities x %d views, %d strays), threshold %.4f, min_rows %d' % (n, a.identities, a.views, a.strays, threshold, a.min_rows))
    print('density: %d core, %d border, %d noise rows -> %d clusters with a core; single link: %d clusters'
          % (kinds[2], kinds[1], kinds[0], int(c.has_core.sum()), single.n_clusters))
    print('pairwise precision / recall / F against the truth: density %.3f %.3f %.3f, single link %.3f %.3f %.3f'
          % (cluster.pairwise_scores(c.cluster_id, who) + cluster.pairwise_scores(single.cluster_id, who)))
    gallery = ffrnet_amd.Gallery(eng)
    gallery.add(cluster.templates(eng, f_new, c)[c.has_core])             # noise rows are not enrolled
    row_of = torch.cumsum(c.has_core.long(), 0) - 1                       # cluster id -> gallery row
    member = c.kind > 0
    top_s, top_i = gallery.search(f_new[member], k=1)
    hit = (top_i[:, 0] == row_of[c.cluster_id[member]]).double().mean().item()
    print('searching the %d clustered faces against the %d templates: the own cluster comes first for %.1f %% of them'
          % (int(member.sum()), len(gallery), 100 * hit))


if __name__ == '__main__':
    main()
