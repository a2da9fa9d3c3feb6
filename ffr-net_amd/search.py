"""1:N identification on top of the library's exact cosine top-k (include/ffrnet.h: ffr_search_topk).

FFR-Net matches masked probes against mask-free enrolments with one model; the reference's harness only scores
aligned pairs (lfw/lfw_eval.py).  This module answers "which of my G enrolled people is this?":

  gallery = Gallery(engine); first = gallery.add(f_enrol)        # embeddings [n,512], e.g. Engine.embed(...)[0]
  scores, index = gallery.search(f_probe, k=10)                  # [Q,k] each, descending score, ties by index
  rates = identification_rates(index, probe_labels, gallery_labels)   # CMC rank-1 / 5 / 10

A gallery spread over several processes (one per GPU) searches its shards with search_sharded().

Gallery(engine, coarse=True) keeps a bf16 plane beside the rows (1 KB per row more) and searches through the certified bf16
shortlist (include/ffrnet.h: ffr_search_topk_coarse): the same results bit for bit, the pass over the gallery on the bf16
matrix cores.  Gallery.last_certified says which probes of the last search the shortlist was proven for.

A gallery with subjects gets the shortlist through build_plane() (include/ffrnet.h: ffr_search_topk_coarse_subjects): from
then on search_subjects() and search() rank through the bf16 pass, bit for bit as before, and set last_certified.

Gallery(engine, subjects=True) keeps a subject id beside every row (include/ffrnet.h: ffr_search_topk_subjects): an enrolled
person is several rows, and search_subjects() answers with the top-k PEOPLE, each once, by their best row:

  gallery = Gallery(engine, subjects=True); gallery.add(f_enrol, subject_ids)
  scores, subjects, index = gallery.search_subjects(f_probe, k=10)
  rates = subject_rates(subjects, probe_labels)
  gallery.remove([7, 12])                  # those people never come back, from search() either; rows keep their index
  old_to_new = gallery.compact()           # drop the removed rows physically

Gallery.build_tags() keeps a 32-bit tag word beside every row (include/ffrnet.h: ffr_search_topk_filtered), with or
without subjects.  A search with mask= ranks, for every probe, only the rows whose tag shares a bit with that probe's mask
word -- watchlists a camera is subscribed to, a tenant's enrolments, the people cleared for a door -- in ONE call for a
batch of probes with different masks:

  gallery = Gallery(engine, subjects=True); gallery.build_tags(); gallery.add(f_enrol, subject_ids, tags=watchlist_bits)
  scores, subjects, index = gallery.search_subjects(f_probe, k=10, mask=camera_subscriptions)     # [Q] words, or an int
  gallery.set_subject_tags([7], 0b0101)    # person 7 moves to watchlists 0 and 2

The filtered search is exact and reads every row.  A filter that stays fixed for long and admits a small share of the rows
is served faster by a second Gallery of those rows (INTEGRATION.md section 7 has the measured crossover).  On a gallery
with a plane, gallery.shortlist_filtered = True sends a masked search through the certified bf16 shortlist (include/ffrnet.h:
ffr_search_topk_coarse_filtered): the same results, half the bytes per row; off by default (INTEGRATION.md section 7 says when
it pays).
"""
import functools

import torch

from .native import tag_words

try:
    import torch.distributed as dist
except ImportError:            # pragma: no cover
    dist = None

DIM = 512
COARSE_EPS = 2.0 ** -8 + 2.0 ** -12      # bound on |coarse score - exact score| (FFR_COARSE_EPS of include/ffrnet.h)
COARSE_MAX_K = 64                        # the coarse pass serves k <= 64 rows
COARSE_MAX_K_DISTINCT = 32               # and k <= 32 identities


def shortlist_size(k, distinct=False):
    """Rows the coarse pass lists per probe for a top-k: min(128, max(2k, 32)); None for k > 64, where the exact search
    runs alone.  distinct=True, for a top-k of identities: min(128, max(4k, 64)) -- a person's rows crowd the head of the
    list -- and None for k > 32."""
    k = int(k)
    if distinct:
        return None if k > COARSE_MAX_K_DISTINCT else min(128, max(4 * k, 64))
    if k > COARSE_MAX_K:
        return None
    return min(128, max(2 * k, 32))


class Gallery(object):
    """Enrolled embeddings [n,512] and their norms on the Engine's device, in a grow-only buffer: add() appends, rows
    keep their index for ever (the index search() returns).  coarse=True: a bf16 plane of the normalised rows and its
    unsafe-norm flag grow beside them, add() packs the rows it appends, and search() goes through the certified shortlist
    (the same results; last_certified[Q] int32 tells which probes were certified).  subjects=True: a subject id (int32)
    grows beside every row, add() takes the ids, search_subjects() ranks subjects, remove() withdraws subjects (their rows
    stay in place, marked -1, and search() skips them) and compact() drops the removed rows.  build_plane() switches the
    shortlist on for the rows a gallery holds already, with or without subjects.  build_tags() switches tags on, for an
    empty gallery or one that holds rows: a 32-bit tag word (int32 carrying the pattern) grows beside every row, add() takes
    the words, set_tags() / set_subject_tags() change them, and search(mask=) / search_subjects(mask=) rank per probe the
    rows whose tag shares a bit with the probe's mask word.  Such a search is the exact filtered one, also on a gallery with
    a plane; set the attribute shortlist_filtered = True and a gallery with a plane serves it through the certified
    shortlist (include/ffrnet.h: ffr_search_topk_coarse_filtered): the same results bit for bit, and last_certified is set."""

    def __init__(self, engine, capacity=0, coarse=False, subjects=False):
        if coarse and subjects:
            raise RuntimeError('ffrnet_amd: Gallery(coarse=True, subjects=True): the certified shortlist does not know '
                               'subjects yet at construction; create Gallery(subjects=True) and call build_plane()')
        self.engine = engine
        self._n = 0
        self._side = []                 # the attributes that hold a row per gallery row: they grow and compact together
        self._add_side('_emb', torch.float32, capacity, DIM)
        self._add_side('_norms', torch.float32, capacity)
        self.coarse = bool(coarse)
        self.last_certified = None
        self.shortlist_filtered = False     # True: a search with mask= on a gallery with a plane takes the certified shortlist
        self.has_subjects = bool(subjects)
        if self.has_subjects:
            self._add_side('_subj', torch.int32, capacity)
        self.has_tags = False
        if self.coarse:
            self._add_plane()

    def _add_side(self, name, dtype, capacity, *tail):
        setattr(self, name, torch.empty((int(capacity),) + tail, device=self.engine.device, dtype=dtype))
        self._side.append(name)

    def _add_plane(self):
        self._add_side('_plane', torch.int16, self._emb.size(0), DIM)
        self._flag = torch.zeros((1,), device=self.engine.device, dtype=torch.int32)

    def __len__(self):
        return self._n

    @property
    def embeddings(self):
        return self._emb[:self._n]

    @property
    def norms(self):
        return self._norms[:self._n]

    @property
    def plane(self):
        """bf16 bits [n,512] (int16) of the normalised rows; coarse galleries only."""
        return self._plane[:self._n]

    @property
    def flag(self):
        """int32 [1]: non-zero once a row with an unsafe norm was added; coarse galleries only."""
        return self._flag

    @property
    def subjects(self):
        """int32 [n]: the subject id of every row, -1 where the row was removed; galleries with subjects only."""
        self._need_subjects('subjects')
        return self._subj[:self._n]

    @property
    def tags(self):
        """int32 [n]: the tag word of every row, as a bit pattern (bit 31 shows as a negative value); galleries with tags
        only."""
        self._need_tags('tags')
        return self._tags[:self._n]

    def _need_tags(self, what):
        if not self.has_tags:
            raise RuntimeError('ffrnet_amd: Gallery.%s needs a gallery with tags; call build_tags() first' % what)

    def _tag_words(self, tags, n, what):
        """int32 device tensor [n] of tag words from an int (the same word for all) or n words"""
        words = tag_words(tags, 'Gallery.%s: tags' % what, self._emb.device)
        if isinstance(tags, int):
            words = words.expand(n)
        if words.numel() != n:
            raise RuntimeError('ffrnet_amd: Gallery.%s: %d tag words where %d are needed' % (what, words.numel(), n))
        return words

    def _need_subjects(self, what):
        if not self.has_subjects:
            raise RuntimeError('ffrnet_amd: Gallery.%s needs a gallery created with subjects=True' % what)

    def _subject_ids(self, ids, what):
        """int32 device tensor of subject ids, each in [0, 2^31)."""
        ids = torch.as_tensor(ids)
        if ids.dtype not in (torch.int32, torch.int64):
            raise RuntimeError('ffrnet_amd: Gallery.%s expects int32 or int64 subject ids, got %s' % (what, ids.dtype))
        ids = ids.reshape(-1).to(self._emb.device)
        if ids.numel() and (int(ids.min().item()) < 0 or int(ids.max().item()) >= 2 ** 31):
            raise RuntimeError('ffrnet_amd: Gallery.%s: subject ids must lie in [0, 2^31)' % what)
        return ids.to(torch.int32)

    def add(self, emb, subjects=None, tags=None):
        """Append emb[n,512] (fp32, on the Engine's device) -> the index of its first row.  A gallery with subjects
        takes subjects[n] (int32 or int64, each in [0, 2^31)) as well, a gallery with tags takes tags: an int for all the
        rows or [n] words (int32 bit patterns, or int64 in [0, 2^32))."""
        if not isinstance(emb, torch.Tensor) or emb.dim() != 2 or emb.size(1) != DIM:
            raise RuntimeError('ffrnet_amd: Gallery.add expects [n,%d] embeddings, got %s'
                               % (DIM, list(emb.shape) if isinstance(emb, torch.Tensor) else type(emb)))
        n = emb.size(0)
        if self.has_subjects:
            if subjects is None:
                raise RuntimeError('ffrnet_amd: Gallery.add: this gallery keeps subjects; pass subjects[n]')
            subjects = self._subject_ids(subjects, 'add')
            if subjects.numel() != n:
                raise RuntimeError('ffrnet_amd: Gallery.add: %d rows but %d subject ids' % (n, subjects.numel()))
        elif subjects is not None:
            raise RuntimeError('ffrnet_amd: Gallery.add: subjects given to a gallery created without subjects=True')
        if self.has_tags:
            if tags is None:
                raise RuntimeError('ffrnet_amd: Gallery.add: this gallery keeps tags; pass tags (an int or [n] words)')
            tags = self._tag_words(tags, n, 'add')
        elif tags is not None:
            raise RuntimeError('ffrnet_amd: Gallery.add: tags given to a gallery without tags; call build_tags() first')
        first = self._n
        if first + n > self._emb.size(0):
            cap = max(first + n, 2 * self._emb.size(0), 1024)
            for name in self._side:
                old = getattr(self, name)
                new = torch.empty((cap,) + old.shape[1:], device=old.device, dtype=old.dtype)
                new[:first] = old[:first]
                setattr(self, name, new)
        if n:                           # every side buffer gets its rows from another source: named one by one
            self._emb[first:first + n] = emb
            self._norms[first:first + n] = self.engine.row_norms(self._emb[first:first + n])
            if self.coarse:
                self.engine.coarse_pack(self._emb[first:first + n], self._norms[first:first + n],
                                        self._plane[first:first + n], self._flag)
            if self.has_subjects:
                self._subj[first:first + n] = subjects
            if self.has_tags:
                self._tags[first:first + n] = tags
        self._n = first + n
        return first

    def build_plane(self):
        """Switch the certified shortlist on for this gallery: pack the bf16 plane and the unsafe-norm flag of the rows held
        (one coarse_pack over all of them), set coarse = True; from then on add() packs what it appends.  The way a gallery
        with subjects gets the pass; any gallery can switch it on without enrolling again.  Does nothing on a gallery that
        has a plane."""
        if self.coarse:
            return
        self._add_plane()
        if self._n:
            self.engine.coarse_pack(self.embeddings, self.norms, self._plane[:self._n], self._flag)
        self.coarse = True

    def build_tags(self, tags=0):
        """Switch tags on for this gallery: a tag word beside every row, registered like the other side buffers, so it grows
        and compacts with them.  The rows held get `tags` (an int for all of them, or [n] words; 0 = admissible for nobody
        until set_tags() / set_subject_tags() say otherwise); from then on add() takes tags.  Works on an empty gallery, so
        Gallery(engine); build_tags() is a gallery with tags from the start.  Does nothing on a gallery that has tags."""
        if self.has_tags:
            return
        words = self._tag_words(tags, self._n, 'build_tags')
        self._add_side('_tags', torch.int32, self._emb.size(0))
        self._tags[:self._n] = words
        self.has_tags = True

    def search(self, query, k, self_index=None, index_base=0, mask=None):
        """Top-k enrolled rows of every probe query[Q,512] -> (scores[Q,k], index[Q,k]).  self_index[Q] (gallery
        indices of the probes themselves): leave-one-out search, the probe's own row is never returned.  mask (an int or
        [Q] words; galleries with tags): every probe ranks only the rows whose tag shares a bit with its mask word."""
        if self_index is None:
            return self._search(query, k, index_base, mask)
        s, i = self._search(query, int(k) + 1, index_base, mask)
        return drop_self(s, i, torch.as_tensor(self_index, device=i.device) + int(index_base))

    def search_subjects(self, query, k, index_base=0, mask=None):
        """Top-k enrolled SUBJECTS of every probe query[Q,512], each once, by its best row -> (scores[Q,k],
        subjects[Q,k] int32, index[Q,k]); k <= 64; (-inf, -1, -1) pads when fewer than k subjects are enrolled.  mask: as
        search() takes it; a subject speaks with its best row among those the probe may see."""
        self._need_subjects('search_subjects')
        s, i, u = self._search_subjects(query, k, index_base, True, mask)
        return s, u, i

    def set_tags(self, index, tags):
        """Give the rows index[n] (gallery indices) new tag words: an int for all of them, or [n] words.  On the device."""
        self._need_tags('set_tags')
        idx = torch.as_tensor(index, device=self._emb.device).reshape(-1).to(torch.int64)
        if idx.numel() and (int(idx.min().item()) < 0 or int(idx.max().item()) >= self._n):
            raise RuntimeError('ffrnet_amd: Gallery.set_tags: row indices must lie in [0, %d)' % self._n)
        self.tags[idx] = self._tag_words(tags, idx.numel(), 'set_tags')

    def set_subject_tags(self, subject_ids, tags):
        """Give every live row of the subjects subject_ids[m] (each named once) new tag words: an int for all of them, or
        [m] words, one per subject.  On the device -> the number of rows changed."""
        self._need_tags('set_subject_tags')
        self._need_subjects('set_subject_tags')
        ids = self._subject_ids(subject_ids, 'set_subject_tags')
        words = self._tag_words(tags, ids.numel(), 'set_subject_tags')
        if not ids.numel():
            return 0
        ids, order = torch.sort(ids)
        live = self.subjects
        hit = torch.isin(live, ids)
        self.tags[hit] = words[order[torch.searchsorted(ids, live[hit])]]
        return int(hit.sum().item())

    def _search_subjects(self, query, k, index_base, distinct, mask=None):
        """(scores, index, subjects) of a gallery with subjects, through the shortlist when it has a plane"""
        if mask is not None:
            return self._search_filtered(query, k, index_base, distinct, mask)
        if not self.coarse:
            return self.engine.search_subjects(query, self.embeddings, self.subjects, k, gallery_norms=self.norms,
                                               index_base=index_base, distinct=distinct)
        s, i, u, self.last_certified = self.engine.search_coarse_subjects(
            query, self.embeddings, self.plane, self._flag, self.subjects, k, gallery_norms=self.norms, index_base=index_base,
            distinct=distinct, return_certified=True)
        return s, i, u

    def remove(self, subject_ids):
        """Withdraw subjects: every row of theirs is marked removed (-1) on the device and never returned again; rows keep
        their index and len() does not change -> the number of rows removed."""
        self._need_subjects('remove')
        ids = self._subject_ids(subject_ids, 'remove')
        live = self.subjects
        hit = torch.isin(live, ids)
        live[hit] = -1
        return int(hit.sum().item())

    def compact(self):
        """Drop the removed rows physically: the live rows, their norms, ids and plane rows move up unchanged (no norm is
        computed again, so scores keep their bits; the unsafe-norm flag stays as it is, set or not: conservative)
        -> int64 [old len]: old index -> new index, -1 for a removed row."""
        self._need_subjects('compact')
        keep = self.subjects >= 0
        new_index = torch.cumsum(keep.to(torch.int64), 0) - 1
        new_index[~keep] = -1
        n = int(keep.sum().item())
        for name in self._side:
            buf = getattr(self, name)
            buf[:n] = buf[:self._n][keep]
        self._n = n
        return new_index

    def _search_filtered(self, query, k, index_base, distinct, mask):
        """The filtered search -> (scores, index(, subjects)): the exact one, also on a gallery that has a plane, unless
        shortlist_filtered is set; then a gallery with a plane goes through the certified shortlist, the same results"""
        self._need_tags('search with a mask')
        subjects = self.subjects if self.has_subjects else None
        if self.shortlist_filtered and self.coarse:
            out = self.engine.search_coarse_filtered(query, mask, self.embeddings, self.plane, self._flag, self.tags, k,
                                                     gallery_norms=self.norms, index_base=index_base, subjects=subjects,
                                                     distinct=distinct, return_certified=True)
            self.last_certified = out[-1]
            return out[:-1]
        self.last_certified = None
        return self.engine.search_filtered(query, mask, self.embeddings, self.tags, k, gallery_norms=self.norms,
                                           index_base=index_base, subjects=subjects, distinct=distinct)

    def _search(self, query, k, index_base, mask=None):
        if self.has_subjects:           # row mode under the mask: removed rows never come back
            s, i, _ = self._search_subjects(query, k, index_base, False, mask)
            return s, i
        if mask is not None:
            return self._search_filtered(query, k, index_base, False, mask)
        if not self.coarse:
            return self.engine.search(query, self.embeddings, k, gallery_norms=self.norms, index_base=index_base)
        s, i, self.last_certified = self.engine.search_coarse(query, self.embeddings, self.plane, self._flag, k,
                                                              gallery_norms=self.norms, index_base=index_base,
                                                              return_certified=True)
        return s, i


def drop_self(scores, index, self_index):
    """Leave-one-out trimming of top-(k+1) lists [Q,k+1]: drop the entry whose index is the probe's own self_index[q]
    (or the last entry when the probe's row is not in the list) -> (scores[Q,k], index[Q,k]), order kept."""
    Q, k1 = index.shape
    drop = index == self_index.reshape(-1, 1).to(index.dtype)
    drop[:, -1] |= ~drop.any(1)
    keep = ~drop
    return scores[keep].view(Q, k1 - 1), index[keep].view(Q, k1 - 1)


def search_sharded(gallery_shard, query, k, group=None, distinct=None):
    """Search a gallery split in contiguous shards over the ranks of `group` (rank r holds rows that follow those of
    ranks < r): every rank passes its own Gallery and the SAME probes query[Q,512] and gets the global top-k.
    Index bases come from the gathered shard sizes; the per-rank [Q,k] lists travel in one all_gather_into_tensor and
    every rank merges them (ffr_topk_merge).  Bitwise equal to one search over the concatenated gallery.
    distinct=True, for shards with subjects: the top-k subjects, (scores, subjects, index) as Gallery.search_subjects
    gives them; the exchange carries the subject as a fourth word and the merge is ffr_topk_merge_subjects.  The default
    (None) and False give the row search of the shard: plain, or under the removal mask of a gallery with subjects."""
    return _search_sharded(gallery_shard.search_subjects if distinct else gallery_shard.search, gallery_shard, query, k, group,
                           distinct)


def search_sharded_filtered(gallery_shard, query, k, mask, group=None, distinct=None):
    """search_sharded() under a per-probe filter: mask (an int or [Q] words, the SAME on every rank) goes to the search of
    every shard, a Gallery with tags.  The shard lists hold admissible rows only, so the exchange and the merge are those of
    search_sharded(), and the result is bitwise that of one filtered search over the concatenated gallery."""
    search = gallery_shard.search_subjects if distinct else gallery_shard.search
    return _search_sharded(functools.partial(search, mask=mask), gallery_shard, query, k, group, distinct)


def _search_sharded(search, gallery_shard, query, k, group, distinct):
    """The body of search_sharded() and search_sharded_filtered(): `search` is the shard's search"""
    eng = gallery_shard.engine
    if dist is None or not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return search(query, k)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    sizes = torch.empty((world,), device=query.device, dtype=torch.int64)
    dist.all_gather_into_tensor(sizes, torch.tensor([len(gallery_shard)], device=query.device, dtype=torch.int64),
                                group=group)
    base = int(sizes[:rank].sum().item())
    lists = search(query, k, index_base=base)            # (s, i), with subjects (s, u, i)
    s, i, w = lists[0], lists[-1], 1 + len(lists)
    Q, kk = s.shape
    # one exchange: per slot the score's bits, the two halves of the index and, with subjects, the subject: w int32 words
    mine = torch.cat([s.contiguous().view(torch.int32).view(Q, kk, 1), i.contiguous().view(torch.int32).view(Q, kk, 2)] +
                     [u.view(Q, kk, 1) for u in lists[1:-1]], 2)
    allw = torch.empty((world * Q, kk, w), device=query.device, dtype=torch.int32)      # rank-major along dim 0
    dist.all_gather_into_tensor(allw, mine.contiguous(), group=group)
    allw = allw.view(world, Q, kk, w)
    all_s = allw[..., 0].contiguous().view(torch.float32)
    all_i = allw[..., 1:3].contiguous().view(torch.int64).view(world, Q, kk)
    if not distinct:
        return eng.topk_merge(all_s, all_i)
    out_s, out_i, out_u = eng.topk_merge_subjects(all_s, all_i, allw[..., 3].contiguous(), distinct=True)
    return out_s, out_u, out_i


def subject_rates(subjects, probe_labels, ranks=(1, 5, 10)):
    """CMC over identity lists: the fraction of probes whose label is among their first r listed subjects, for every r in
    ranks.  subjects[Q,k] (Gallery.search_subjects; -1 = padding, which never hits), probe_labels[Q] -> {r: rate}."""
    subjects = torch.as_tensor(subjects)
    pl = torch.as_tensor(probe_labels).to(subjects.device)
    hit = (subjects == pl.reshape(-1, 1).to(subjects.dtype)) & (subjects >= 0)
    out = {}
    for r in ranks:
        out[r] = float(hit[:, :r].any(1).double().mean().item()) if subjects.size(0) else 0.0
    return out


def identification_rates(index, probe_labels, gallery_labels, ranks=(1, 5, 10)):
    """CMC: the fraction of probes whose label appears among their first r results, for every r in ranks.
    index[Q,k] (gallery indices, -1 = padding), probe_labels[Q], gallery_labels[G] -> {r: rate}."""
    index = torch.as_tensor(index)
    gl = torch.as_tensor(gallery_labels).to(index.device)
    pl = torch.as_tensor(probe_labels).to(index.device)
    valid = index >= 0
    lab = gl[index.clamp(min=0)]
    hit = (lab == pl.reshape(-1, 1)) & valid
    out = {}
    for r in ranks:
        out[r] = float(hit[:, :r].any(1).double().mean().item()) if index.size(0) else 0.0
    return out
