#!/usr/bin/env python3
"""Filtered identification on synthetic images (needs an MI355X): people enrolled on overlapping watchlists, probes from
cameras with different subscriptions, searched in ONE call ("Filters").

    python examples/identify_watchlists_synthetic.py [--identities 24] [--views 4] [--coarse]

An "identity" is a random image, a "view" of it the same image under pixel noise; the probes are further views.  Watchlist w
is bit w of a person's tag word; a camera's mask word has the bits of the watchlists it is subscribed to.  A person is
admissible for a camera iff the two words share a bit.
--coarse: the gallery gets its bf16 plane (build_plane()) and shortlist_filtered = True, so every masked search goes through
the certified shortlist -- the same results bit for bit, which the example checks against the exact filtered search.
"""
import argparse, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd
from ffrnet_amd import synth

STAFF, VISITORS, BARRED, VIP = 1 << 0, 1 << 1, 1 << 2, 1 << 31          # bit 31 is a bit like any other
CAMERAS = {'lobby': STAFF | VISITORS | BARRED, 'lab door': STAFF, 'lounge': VIP | STAFF, 'unsubscribed': 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--identities', type=int, default=24)
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--noise', type=float, default=0.25)
    ap.add_argument('--coarse', action='store_true', help='masked searches through the certified bf16 shortlist')
    a = ap.parse_args()
    specs = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'g0_state_dict_keys.json')))
    eng = ffrnet_amd.Engine(0)
    eng.load_encoder(synth.synth_state_dict(specs['encoder']))
    eng.load_recnet(synth.synth_state_dict(specs['recnet']))
    base = synth.synth_images(a.identities, seed=21)
    n = a.identities * a.views
    who = torch.arange(a.identities).repeat_interleave(a.views)
    enrol = (base[who] + a.noise * synth.synth_images(n, seed=22)).clamp(-1, 1)
    probe = (base + a.noise * synth.synth_images(a.identities, seed=23)).clamp(-1, 1)      # one probe per identity
    f_enrol, _ = eng.embed(enrol.cuda(), want_f=False)
    f_probe, _ = eng.embed(probe.cuda(), want_f=False)

    # overlapping watchlists: everybody is staff or a visitor, every third person is barred as well, every eighth a VIP
    person = torch.arange(a.identities)
    lists = torch.where(person % 2 == 0, STAFF, VISITORS) | torch.where(person % 3 == 0, BARRED, 0) | torch.where(person % 8 == 0, VIP, 0)

    gallery = ffrnet_amd.Gallery(eng, subjects=True)
    gallery.build_tags()                                                  # a tag word beside every row from here on
    gallery.add(f_enrol, who.cuda(), tags=lists[who])                     # int64 words in [0, 2^32), or int32 bit patterns
    print('%d rows of %d identities enrolled on %d watchlists' % (len(gallery), a.identities, 4))
    if a.coarse:
        gallery.build_plane()                                             # packs the rows held; add() packs from here on
        gallery.shortlist_filtered = True                                 # masked searches take the shortlist: opt-in

    # every probe is seen by every camera: one batch, one call, one mask word per probe
    names = list(CAMERAS)
    cam = torch.arange(len(names)).repeat(a.identities)
    query = f_probe.repeat_interleave(len(names), 0)
    mask = torch.tensor([CAMERAS[c] for c in names])[cam]
    k = min(3, a.identities)
    scores, subjects, index = gallery.search_subjects(query, k, mask=mask)
    if a.coarse:
        es, ei, eu = eng.search_filtered(query, mask, gallery.embeddings, gallery.tags, k, gallery_norms=gallery.norms,
                                         subjects=gallery.subjects, distinct=True)
        assert torch.equal(scores, es) and torch.equal(index, ei) and torch.equal(subjects, eu)
        print('shortlist: the bits of the exact filtered search; certified for %d of %d probes'
              % (int(gallery.last_certified.sum()), query.size(0)))
    seen = subjects.cpu()
    ok = (seen < 0) | ((lists[seen.clamp(min=0)] & mask[:, None]) != 0)
    assert bool(ok.all())                                                 # nobody outside a camera's watchlists is ever listed
    assert bool((seen[cam == names.index('unsubscribed')] == -1).all())   # mask 0: k slots of padding
    for c, name in enumerate(names):
        hit = seen[cam == c][:, 0] == person
        may = (lists & CAMERAS[name]) != 0
        assert not bool(hit[~may].any())
        print('%-12s sees %2d of %d people; rank-1 among those %.2f; person 1 there: %s'
              % (name, int(may.sum()), a.identities, float(hit[may].float().mean()) if bool(may.any()) else 0.0,
                 seen[cam == c][1].tolist()))

    # the same through one unfiltered search per camera over a gallery compacted to its watchlists: what the call replaces
    for c, name in enumerate(names[:3]):
        rows = ((gallery.tags & ffrnet_amd.native.tag_words(CAMERAS[name], 'mask', 'cuda')) != 0).nonzero().reshape(-1)
        s, i, u = eng.search_subjects(f_probe, gallery.embeddings[rows], gallery.subjects[rows], k, gallery_norms=gallery.norms[rows])
        assert torch.equal(s, scores[cam.cuda() == c]) and torch.equal(u, subjects[cam.cuda() == c])
        assert torch.equal(torch.where(i >= 0, rows[i.clamp(min=0)], i), index[cam.cuda() == c])
    print('one filtered call == one compacted gallery and one search per camera, bit for bit')

    moved = gallery.set_subject_tags([1], BARRED)                          # person 1 is barred now, and nothing else
    scores, subjects, index = gallery.search_subjects(f_probe[1:2].repeat(len(names), 1), k, mask=torch.tensor([CAMERAS[c] for c in names]))
    print('person 1 moved to the barred list (%d rows): now seen by %s'
          % (moved, [name for c, name in enumerate(names) if int(subjects[c, 0]) == 1]))


if __name__ == '__main__':
    main()
