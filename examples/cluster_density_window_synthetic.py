#!/usr/bin/env python3
"""A sliding window over a stream of faces under the density-gated clustering, on synthetic images (needs an MI355X): per
batch embed -> IncrementalDensity.add, and once the window is full the oldest batch expires -> IncrementalDensity.remove;
at the end the templates of the clusters with a core -> Gallery.add -> search.

    python examples/cluster_density_window_synthetic.py [--identities 24] [--views 5] [--batches 6] [--window 3] [--min-rows 3]

An "identity" is a random image, a "view" of it the same image under pixel noise; the shuffled views arrive in batches and
the store holds the last --window of them.  When faces leave, degrees fall: a core row may be demoted, a border row may
choose another cluster or become noise; the labels and the state after every step are those of one density() over the
faces held (checked at every step).  remove() returns the old-to-new index map; the side table of this example (which
image every row is) is renumbered through it.  The threshold is chosen as in examples/cluster_synthetic.py; with real
weights take it from the verification protocol.
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
    ap.add_argument('--views', type=int, default=5)
    ap.add_argument('--batches', type=int, default=6)
    ap.add_argument('--window', type=int, default=3)
    ap.add_argument('--min-rows', type=int, default=3)
    ap.add_argument('--noise', type=float, default=0.25)
    a = ap.parse_args()
    specs = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'g0_state_dict_keys.json')))
    eng = ffrnet_amd.Engine(0)
    eng.load_encoder(synth.synth_state_dict(specs['encoder']))
    eng.load_recnet(synth.synth_state_dict(specs['recnet']))
    n = a.identities * a.views
    if n > 128:
        ap.error('identities x views must be at most 128: the threshold of this toy is read off one search of k = n')
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

    store = cluster.IncrementalDensity(eng, threshold, a.min_rows)
    image = torch.empty(0, dtype=torch.int64, device='cuda')              # side table: the image each row held shows
    sizes, equal = [], True
    for k, batch in enumerate(torch.tensor_split(torch.arange(n), a.batches)):
        f_new, _ = eng.embed(imgs[batch].cuda(), want_f=False)            # only the new images are embedded
        store.add(f_new)
        image = torch.cat((image, batch.cuda()))
        sizes.append(batch.numel())
        line = 'batch %d: +%d faces' % (k, batch.numel())
        if len(sizes) > a.window:                                         # the oldest batch expires
            before = store.state
            keep = torch.ones(len(store), dtype=torch.bool, device='cuda')
            keep[:sizes[0]] = False
            after = eng.cluster_density_remove(store.embeddings, threshold, a.min_rows, before.rep.clone(), before.degree.clone(),
                                               before.best.clone(), keep, norms=store.norms)            # only to report
            drop, compute = cluster.density_removal_changes(before, after[0])     # templates to drop, templates to compute
            demoted = int(((before.kind == 2) & keep & (after[1] != 2)).sum())
            old_to_new = store.remove(torch.arange(sizes.pop(0)))
            image = image[old_to_new >= 0]                                # survivors keep their order
            line += ', -%d: %d core faces demoted, %d templates to drop, %d to compute' % (
                int((old_to_new < 0).sum()), demoted, drop.numel(), compute.numel())
        c = store.clusters
        once = cluster.density(eng, store.embeddings, threshold, a.min_rows)
        equal &= bool(torch.equal(c.rep, once.rep)) and bool(torch.equal(c.kind, once.kind))
        print('%s -> %d clusters with a core, %d noise faces, over %d faces' % (line, int(c.has_core.sum()), int((c.kind == 0).sum()), len(store)))
    c = store.clusters
    p, r, f = cluster.pairwise_scores(c.cluster_id, who[image.cpu()])
    print('equal to one density() of the faces held after every step: %s; pairwise precision %.3f recall %.3f F %.3f' % (equal, p, r, f))
    if not bool(c.has_core.any()):
        print('no cluster with a core is left in the window: nothing to enrol')
        return
    gallery = ffrnet_amd.Gallery(eng)
    gallery.add(store.templates())                                        # one row per cluster with a core
    enrolled = torch.cumsum(c.has_core.long(), 0) - 1                     # cluster id -> gallery row
    faces = c.has_core[c.cluster_id]                                      # the faces whose cluster was enrolled
    top_s, top_i = gallery.search(store.embeddings, k=1)
    hit = (top_i[faces, 0] == enrolled[c.cluster_id[faces]]).double().mean().item()
    print('searching every enrolled face against the %d templates: its own cluster comes first for %.1f %% of them' % (len(gallery), 100 * hit))


if __name__ == '__main__':
    main()
