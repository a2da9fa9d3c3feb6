#!/usr/bin/env python3
"""Identification over a subject-labelled gallery on synthetic images (needs an MI355X): several images per identity ->
Gallery(subjects=True).add -> search_subjects -> remove one identity -> search again -> compact.

    python examples/identify_subjects_synthetic.py [--identities 24] [--views 4] [--coarse]

An "identity" is a random image, a "view" of it the same image under pixel noise; the probes are further views.
--coarse: after the first enrolment session the gallery gets its bf16 plane (build_plane()), and every search goes through
the certified shortlist -- the same results bit for bit, which the example checks against the exact subject search.
"""
import argparse, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd
from ffrnet_amd import synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--identities', type=int, default=24)
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--noise', type=float, default=0.25)
    ap.add_argument('--coarse', action='store_true', help='search through the certified bf16 shortlist')
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
    labels = torch.arange(a.identities)

    gallery = ffrnet_amd.Gallery(eng, subjects=True)
    half = n // 2
    gallery.add(f_enrol[:half], who[:half].cuda())                       # enrolment in two sessions
    if a.coarse:
        gallery.build_plane()                                            # packs the rows held; add() packs from here on
    gallery.add(f_enrol[half:], who[half:].cuda())
    k = min(5, a.identities)
    scores, subjects, index = gallery.search_subjects(f_probe, k)         # k people per probe, each once
    rows_s, rows_i = gallery.search(f_probe, k)                           # k rows: mostly views of one person
    print('%d rows of %d identities enrolled' % (len(gallery), a.identities))
    if a.coarse:
        es, ei, eu = eng.search_subjects(f_probe, gallery.embeddings, gallery.subjects, k, gallery_norms=gallery.norms)
        assert torch.equal(scores, es) and torch.equal(index, ei) and torch.equal(subjects, eu)
        print('shortlist: the bits of the exact search; last search certified for %d of %d probes'
              % (int(gallery.last_certified.sum()), a.identities))
    print('probe 0: people %s, rows %s of people %s' % (subjects[0].tolist(), rows_i[0].tolist(),
                                                         who[rows_i[0].cpu()].tolist()))
    print('identity CMC  ', ffrnet_amd.subject_rates(subjects, labels, ranks=(1, k)))
    print('row CMC       ', ffrnet_amd.identification_rates(rows_i, labels, who, ranks=(1, k)))

    gone = int(subjects[0, 0])
    removed = gallery.remove([gone])                                      # withdraw the person probe 0 matched
    scores2, subjects2, index2 = gallery.search_subjects(f_probe, k)
    assert not bool((subjects2 == gone).any()) and not bool((gallery.subjects[gallery.search(f_probe, k)[1]] == gone).any())
    print('removed subject %d (%d rows): probe 0 now matches people %s' % (gone, removed, subjects2[0].tolist()))

    old_to_new = gallery.compact()                                        # drop the rows physically; indices move
    scores3, subjects3, index3 = gallery.search_subjects(f_probe, k)
    assert torch.equal(scores3, scores2) and torch.equal(subjects3, subjects2) and torch.equal(index3, old_to_new[index2])
    print('compacted to %d rows; the results are the same, indices mapped' % len(gallery))


if __name__ == '__main__':
    main()
