"""Grouping unlabelled embeddings into identities (include/ffrnet.h: ffr_cluster_threshold, ffr_cluster_extend,
ffr_cluster_remove, ffr_cluster_density, ffr_cluster_density_extend, ffr_cluster_density_remove, ffr_cluster_templates).

A photo collection or a dump of video tracks arrives as N unlabelled faces; before the first Gallery.add they have to be
grouped by person and every group fused into one template row:

  c = cluster.cluster(engine, f, threshold)          # f[N,512] e.g. Engine.embed(...)[0]; threshold from lfw.get_avg_accuracy
  t = cluster.templates(engine, f, c)                # [c.n_clusters,512], unit rows
  gallery = Gallery(engine); gallery.add(t)          # template row r is cluster id r

The clustering is single-link at one cosine threshold: rows i < j are joined iff their search score is > threshold, and
a cluster is a connected component of those edges.  It runs on the device; only pairwise_scores() is host logic.

Single link lets a few in-between rows (a blurred frame, a half-occluded face, a look-alike) join two people into one
cluster, whose template is then a mixture.  density() gates the same edges by density (DBSCAN): a row with fewer than
min_rows rows within the threshold of it (itself counted) may attach to a cluster but never connects two, and a row with
no dense neighbour is reported as noise instead of being enrolled as a one-row identity:

  c = cluster.density(engine, f, threshold, min_rows=4)
  t = cluster.templates(engine, f, c)[c.has_core]    # the clusters with a core; gallery row r is the r-th of them
  gallery.add(t)

A collection that keeps growing is extended instead of clustered again (include/ffrnet.h: ffr_cluster_extend): only the
pairs that involve a new row are scored, and the result is the clustering of all rows at once, label for label:

  store = cluster.Incremental(engine, threshold)
  store.add(f_batch)                                 # as often as faces arrive; must_link= ties the frames of one track
  t = store.templates()                              # when a gallery is wanted

Rows are taken out again the same way (ffr_cluster_remove): a deleted photo, an expired track, a withdrawn enrolment.  A
cluster that loses no row keeps its label; the survivors of a cluster that loses one are joined again among themselves
(it may fall apart when the row that bridged two people goes), and only their pairs are scored.  The result is the
clustering of the remaining rows, label for label.

  old_to_new = store.remove(rows)                    # compacts; renumber side tables through the map
  c, old_to_new, kept = cluster.remove(engine, f, threshold, c, rows=rows)      # the functional form; f is not touched

The density-gated clustering is extended in the same way (ffr_cluster_density_extend), with the per-row state the
extension needs kept beside the labels; after every add the result is density() over all rows held:

  store = cluster.IncrementalDensity(engine, threshold, min_rows=4)
  store.add(f_batch)
  t = store.templates()                              # one row per cluster with a core: what gets enrolled

and rows leave it again (ffr_cluster_density_remove): degrees fall, core rows may be demoted, border rows choose again, and
afterwards the labels and the state are those of density() over the rows still held, so add() and remove() interleave:

  old_to_new = store.remove(rows)                    # a sliding window: the oldest frames expire
  c, state, old_to_new, kept = cluster.density_remove(engine, f, threshold, 4, state, rows=rows)    # the functional form
"""
import collections

import torch

Clusters = collections.namedtuple('Clusters', ['rep', 'cluster_id', 'n_clusters', 'sizes'])
Clusters.__doc__ = """rep[N] int64: the smallest row index of each row's cluster; cluster_id[N] int64: dense ids 0 .. C-1 in
order of representative; n_clusters: C (int); sizes[C] int64: rows per cluster."""


DensityClusters = collections.namedtuple('DensityClusters', ['rep', 'cluster_id', 'n_clusters', 'sizes', 'kind', 'has_core'])
DensityClusters.__doc__ = """rep, cluster_id, n_clusters, sizes: as Clusters (member_order and templates accept either); kind[N]
uint8: 2 core, 1 border, 0 noise; has_core[C] bool: False exactly for the noise singletons."""


def dense_ids(rep):
    """rep[N] (any device) -> Clusters: ids 0 .. C-1 by ascending representative."""
    rep = torch.as_tensor(rep)
    uniq, inv, counts = torch.unique(rep, sorted=True, return_inverse=True, return_counts=True)
    return Clusters(rep, inv.reshape(rep.shape), int(uniq.numel()), counts)


def cluster(engine, emb, threshold, norms=None):
    """Single-link clustering of emb[N,512] (fp32, on the Engine's device) at `threshold` -> Clusters."""
    return dense_ids(engine.cluster(emb, threshold, norms=norms))


def density_ids(rep, kind):
    """rep[N], kind[N] (any device) -> DensityClusters.  A noise row is alone in its cluster and every other cluster holds
    a core row, so has_core is False exactly where the cluster's rows are noise."""
    c = dense_ids(rep)
    kind = torch.as_tensor(kind)
    has_core = torch.zeros((c.n_clusters,), device=c.cluster_id.device, dtype=torch.bool)
    has_core[c.cluster_id[kind.to(c.cluster_id.device) == 2]] = True
    return DensityClusters(c.rep, c.cluster_id, c.n_clusters, c.sizes, kind, has_core)


def density(engine, emb, threshold, min_rows, norms=None):
    """Density-gated clustering of emb[N,512] (fp32, on the Engine's device) over the edges of cluster() -> DensityClusters:
    rows with at least min_rows rows within `threshold` (themselves counted) are core and link; the others attach to their
    best-scoring core neighbour or are noise.  templates(engine, emb, c)[c.has_core] is what gets enrolled."""
    return density_ids(*engine.cluster_density(emb, threshold, min_rows, norms=norms))


def representatives(labels):
    """Arbitrary integer labels[N] (track ids, person ids; any device) -> rep[N] int64: the first row index that carries
    each row's label.  Plain torch.  This is the `prior` form of Engine.cluster_extend: rows with equal labels are tied."""
    labels = torch.as_tensor(labels).reshape(-1)
    n = labels.numel()
    _, inv = torch.unique(labels, return_inverse=True)
    row = torch.arange(n, device=labels.device, dtype=torch.int64)
    first = torch.full((n,), n, device=labels.device, dtype=torch.int64).scatter_reduce_(0, inv, row, 'amin')
    return first[inv]


def changes(rep_before, rep_after):
    """What an extension did to the clusters that existed: -> (stale, now), both int64.  stale holds the rows that were
    representatives in rep_before and are none in rep_after (their cluster was absorbed by one with a smaller first row),
    now[k] = rep_after[stale[k]], the cluster they went to.  A caller that keeps one template per cluster drops the
    templates of `stale` and recomputes those of `now`; clusters that merely gained rows keep their representative and
    show up in neither.  This is for single link (extend, Incremental) only: it relies on an old row's rep never rising
    and on clusters changing by absorption alone.  A density-gated clustering keeps neither promise (a border row may
    change sides); use density_changes there.  A removal (remove, Incremental.remove) breaks both as well: clusters
    split and representatives rise; use removal_changes there (density_removal_changes for a density-gated one)."""
    rep_before, rep_after = torch.as_tensor(rep_before).reshape(-1), torch.as_tensor(rep_after).reshape(-1)
    n = rep_before.numel()
    if rep_after.numel() < n:
        raise ValueError('changes: %d labels before, %d after' % (n, rep_after.numel()))
    row = torch.arange(n, device=rep_before.device, dtype=torch.int64)
    after = rep_after[:n].to(rep_before.device)
    stale = row[(rep_before == row) & (after != row)]
    return stale, after[stale]


def _new_prior(n_old, n_new, must_link, device):
    """prior of n_new rows appended at n_old: each row itself, or the first new row with its must_link label"""
    if must_link is None:
        return torch.arange(n_old, n_old + n_new, device=device, dtype=torch.int64)
    must_link = torch.as_tensor(must_link).reshape(-1)
    if must_link.numel() != n_new:
        raise RuntimeError('ffrnet_amd: %d must_link labels for %d new rows' % (must_link.numel(), n_new))
    return representatives(must_link).to(device) + n_old


def extend(engine, emb, threshold, earlier, norms=None, must_link=None):
    """Extend a clustering of the first rows of emb[N,512] to all N rows -> Clusters, equal to cluster(engine, emb,
    threshold) when `earlier` is the clustering of emb[:n_old] at this threshold.  earlier: a Clusters or a rep[n_old]
    (n_old = 0: a clustering from scratch).  must_link: integer labels of the N - n_old new rows (track ids); new rows
    with equal labels are in one cluster whatever they score.  Only the pairs with a new row are scored."""
    rep = earlier.rep if isinstance(earlier, Clusters) else torch.as_tensor(earlier)
    rep = rep.reshape(-1).to(device=emb.device, dtype=torch.int64)
    n_old, n = rep.numel(), emb.size(0)
    if n_old > n:
        raise RuntimeError('ffrnet_amd: %d earlier labels for %d embeddings' % (n_old, n))
    prior = torch.cat((rep, _new_prior(n_old, n - n_old, must_link, emb.device)))
    return dense_ids(engine.cluster_extend(emb, threshold, prior, n_old, norms=norms, out=prior))


def _keep_mask(n, rows, keep, device):
    """exactly one of rows (indices to remove; duplicates allowed) and keep (mask of the rows that stay) -> bool[n]"""
    if (rows is None) == (keep is None):
        raise ValueError('ffrnet_amd: give exactly one of rows (the indices to remove) and keep (the mask of rows that stay)')
    if keep is not None:
        keep = torch.as_tensor(keep).reshape(-1).to(device)
        if keep.numel() != n or keep.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError('ffrnet_amd: keep must be a bool or uint8 mask of %d entries' % n)
        return keep != 0
    rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1).to(device)
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
        raise RuntimeError('ffrnet_amd: rows to remove must be in [0, %d)' % n)
    mask = torch.ones((n,), device=device, dtype=torch.bool)
    mask[rows] = False
    return mask


def _index_maps(keep):
    """keep bool[n] -> (old_to_new int64[n], -1 for a removed row; kept int64[n_s], new-to-old, ascending)"""
    kept = torch.nonzero(keep).reshape(-1)
    old_to_new = torch.full((keep.numel(),), -1, device=keep.device, dtype=torch.int64)
    old_to_new[kept] = torch.arange(kept.numel(), device=keep.device, dtype=torch.int64)
    return old_to_new, kept


def _surviving_prior(tie, kept):
    """tie[n]: integer labels of the tie groups (must-links); kept: the surviving rows, ascending -> prior[n] int64: for a
    surviving row the first surviving row of its group, for a removed row the row itself"""
    prior = torch.arange(tie.numel(), device=tie.device, dtype=torch.int64)
    prior[kept] = kept[representatives(tie[kept])]
    return prior


def remove(engine, emb, threshold, earlier, rows=None, keep=None, must_link=None, norms=None):
    """Take rows out of a single-link clustering of emb[N,512] -> (Clusters of the survivors in compact numbering,
    old_to_new int64[N] with -1 for a removed row, kept int64[N_s]: the surviving rows, new-to-old).  The Clusters equal
    cluster(engine, emb[kept], threshold) when `earlier` (a Clusters or a rep[N]) is the clustering of emb at this threshold;
    only the pairs among the survivors of the clusters that lost a row are scored.  Give exactly one of rows (indices to
    remove, duplicates allowed) and keep (mask of the rows that stay).  must_link: integer labels of all N rows (track ids)
    the clustering was made with; surviving rows with equal labels stay in one cluster whatever they score.  emb is not
    touched: compact it with emb[kept].  Single link only; a density-gated clustering has density_remove."""
    rep = earlier.rep if isinstance(earlier, Clusters) else torch.as_tensor(earlier)
    rep = rep.reshape(-1).to(device=emb.device, dtype=torch.int64)
    n = emb.size(0)
    if rep.numel() != n:
        raise RuntimeError('ffrnet_amd: %d earlier labels for %d embeddings' % (rep.numel(), n))
    mask = _keep_mask(n, rows, keep, emb.device)
    old_to_new, kept = _index_maps(mask)
    prior = None
    if must_link is not None:
        must_link = torch.as_tensor(must_link).reshape(-1).to(emb.device)
        if must_link.numel() != n:
            raise RuntimeError('ffrnet_amd: %d must_link labels for %d rows' % (must_link.numel(), n))
        prior = _surviving_prior(must_link, kept)
    after = engine.cluster_remove(emb, threshold, rep, mask, prior=prior, norms=norms)
    return dense_ids(old_to_new[after[kept]]), old_to_new, kept


def removal_changes(rep_before, rep_after):
    """What a removal did to the clusters: -> (touched, now), both int64, ascending, in the numbering BEFORE the removal
    (rep_after as Engine.cluster_remove returns it: same numbering, -1 for a removed row).  touched: the old representatives
    of the clusters that lost a row; now: the representatives of the clusters their survivors form (none where a cluster
    was removed whole; two or more where one fell apart; a row that was no representative before where the old one was
    removed).  A caller that keeps one template per cluster drops those of `touched` and recomputes those of `now`; every
    other cluster kept its rows and its label."""
    before = torch.as_tensor(rep_before).reshape(-1).to(torch.int64)
    after = torch.as_tensor(rep_after).reshape(-1).to(device=before.device, dtype=torch.int64)
    if after.numel() != before.numel():
        raise ValueError('removal_changes: %d labels before, %d after' % (before.numel(), after.numel()))
    gone = after < 0
    touched = torch.unique(before[gone])
    hit = torch.zeros((before.numel(),), device=before.device, dtype=torch.bool)
    hit[touched] = True
    return touched, torch.unique(after[~gone & hit[before]])


def _batch_rows(who, emb):
    """add()'s batch must be emb[n,512] -> n; `who` names the class in the message"""
    if not isinstance(emb, torch.Tensor) or emb.dim() != 2 or emb.size(1) != 512:
        raise RuntimeError('ffrnet_amd: %s.add expects [n,512] embeddings, got %s'
                           % (who, list(emb.shape) if isinstance(emb, torch.Tensor) else type(emb)))
    return emb.size(0)


def _grown(bufs, held, need):
    """The grow-only rule of the stores: bufs, a tuple of buffers that hold `held` rows each -> the same tuple while `need`
    rows fit, else new buffers of at least twice the capacity with the rows held copied over."""
    if need <= bufs[0].size(0):
        return bufs
    cap = max(need, 2 * bufs[0].size(0), 1024)
    grown = []
    for buf in bufs:
        new = torch.empty((cap,) + tuple(buf.shape[1:]), device=buf.device, dtype=buf.dtype)
        new[:held] = buf[:held]
        grown.append(new)
    return tuple(grown)


class Incremental(object):
    """A clustering that keeps being added to: embeddings [n,512], their norms and rep[n] on the Engine's device, in
    grow-only buffers (as search.Gallery).  add() scores the new rows against everything held and among themselves; after
    every add the labels are those of one clustering of all rows held.  Between removals rows keep their index and the rep
    of an old row can only decrease (cluster.changes tells which clusters were absorbed).  remove() takes rows out, compacts
    the buffers and returns the old-to-new index map: the rows behind a removed one move down, and a rep may rise
    (cluster.removal_changes, on the labels before compaction, tells which clusters to recompute).  The tie groups of
    must_link are remembered per row, so that tied rows stay together when the row that connected them leaves.  remove()
    always calls the removal: measured up to half of the rows leaving at once, it was never slower than compacting and
    clustering again (EXPERIMENTS.md, tools/bench_cluster_remove.py), so there is no second route."""

    def __init__(self, engine, threshold, capacity=0):
        self.engine = engine
        self.threshold = float(threshold)
        self._n = 0
        self._emb = torch.empty((int(capacity), 512), device=engine.device, dtype=torch.float32)
        self._norms = torch.empty((int(capacity),), device=engine.device, dtype=torch.float32)
        self._rep = torch.empty((int(capacity),), device=engine.device, dtype=torch.int64)
        self._tie = torch.empty((int(capacity),), device=engine.device, dtype=torch.int64)     # first row of the tie group

    def __len__(self):
        return self._n

    @property
    def embeddings(self):
        return self._emb[:self._n]

    @property
    def norms(self):
        return self._norms[:self._n]

    @property
    def rep(self):
        return self._rep[:self._n]

    @property
    def clusters(self):
        return dense_ids(self.rep)

    def templates(self):
        """One unit template per cluster of the rows held -> [C,512], row c for cluster id c."""
        return templates(self.engine, self.embeddings, self.clusters, norms=self.norms)

    def add(self, emb, must_link=None):
        """Append emb[n,512] (fp32, on the Engine's device) and extend the clustering -> the index of its first row.
        must_link: integer labels of these n rows; equal labels are tied (the frames of one track)."""
        n, first = _batch_rows('Incremental', emb), self._n
        new_prior = _new_prior(first, n, must_link, self._rep.device)
        self._emb, self._norms, self._rep, self._tie = _grown((self._emb, self._norms, self._rep, self._tie), first, first + n)
        if n:
            total = first + n
            self._emb[first:total] = emb
            self._norms[first:total] = self.engine.row_norms(self._emb[first:total])
            self._rep[first:total] = new_prior
            self._tie[first:total] = new_prior
            self.engine.cluster_extend(self._emb[:total], self.threshold, self._rep[:total], first,
                                       norms=self._norms[:total], validate=False, out=self._rep[:total])
            self._n = total
        return first

    def remove(self, rows):
        """Take the rows with these indices out (any integer sequence or tensor; duplicates allowed) and compact the
        buffers in order -> old_to_new int64[n]: the new index of every row held before, -1 for a removed one, so that
        callers can renumber their side tables.  Afterwards the labels are those of one clustering of the rows still held
        (with their must-links), and add() works as before.  Only the pairs among the survivors of the clusters that lost a
        row are scored."""
        n = self._n
        keep = _keep_mask(n, rows, None, self._rep.device)
        old_to_new, kept = _index_maps(keep)
        ns = kept.numel()
        if ns == n:
            return old_to_new
        tie = representatives(self._tie[:n][kept])                 # the first surviving row of each group, new numbering
        prior = torch.arange(n, device=kept.device, dtype=torch.int64)
        prior[kept] = kept[tie]
        rep = self.engine.cluster_remove(self._emb[:n], self.threshold, self._rep[:n], keep, prior=prior,
                                         norms=self._norms[:n], validate=False, out=self._rep[:n])
        self._emb[:ns] = self._emb[:n][kept]
        self._norms[:ns] = self._norms[:n][kept]
        self._rep[:ns] = old_to_new[rep[kept]]
        self._tie[:ns] = tie
        self._n = ns
        return old_to_new


DensityState = collections.namedtuple('DensityState', ['rep', 'kind', 'degree', 'best', 'threshold', 'min_rows'])
DensityState.__doc__ = """What Engine.cluster_density_extend needs of the rows clustered so far: rep[n] int64, kind[n] uint8,
degree[n] int32, best[n] int64 (the key by which a border row chose its core row; 0 for core and noise rows), and the
threshold and min_rows they were made with: a state is valid for no other."""


def density_extend(engine, emb, threshold, min_rows, earlier=None, norms=None):
    """Extend a density-gated clustering of the first rows of emb[N,512] to all N rows -> (DensityClusters, DensityState),
    the clusters equal to density(engine, emb, threshold, min_rows).  earlier: the DensityState an earlier call returned for
    emb[:n_old] (None: a clustering from scratch); it is left as it is.  Only the pairs with a new row, and the pairs of old
    rows of which one was made core by the new rows, are scored.  A state made with another threshold or min_rows is refused."""
    threshold, min_rows = float(threshold), int(min_rows)
    if earlier is None:
        rep = degree = best = None
        n_old = 0
    else:
        if float(earlier.threshold) != threshold or int(earlier.min_rows) != min_rows:
            raise RuntimeError('ffrnet_amd: the state was made with threshold %r and min_rows %d; it cannot be extended with %r '
                               'and %d' % (earlier.threshold, earlier.min_rows, threshold, min_rows))
        n_old = earlier.rep.numel()
        if n_old > emb.size(0):
            raise RuntimeError('ffrnet_amd: a state of %d rows for %d embeddings' % (n_old, emb.size(0)))
        rep, degree, best = earlier.rep, earlier.degree, earlier.best
        if n_old == emb.size(0):                               # [N] tensors are updated in place: work on copies
            rep, degree, best = rep.clone(), degree.clone(), best.clone()
    rep, kind, degree, best = engine.cluster_density_extend(emb, threshold, min_rows, rep, degree, best, n_old, norms=norms)
    return density_ids(rep, kind), DensityState(rep, kind, degree, best, threshold, min_rows)


def density_changes(before, after):
    """What an extension did to the clusters of a density-gated clustering: -> (gone, recompute), both int64 and ascending.
    before, after: rep tensors, or anything with a .rep (DensityClusters, DensityState), of n and N >= n rows.
    gone: the representatives of `before` that are none in `after`.  recompute: the representatives of `after` whose
    members among the first n rows are not exactly the members of one cluster of `before`, or that hold a new row.  A
    caller that keeps one template per cluster drops those of `gone` and computes those of `recompute`.

    changes() is not enough here.  Under single link an old row's rep can only decrease, and a cluster changes only by
    being absorbed or by gaining rows.  Under density gating a border row may move to a better-scoring core row of ANOTHER
    cluster once new rows made that one core: both clusters change though neither was absorbed, and if the row was the
    smallest member of the cluster it left, that cluster's representative RISES to a row that was none before."""
    before = torch.as_tensor(getattr(before, 'rep', before)).reshape(-1)
    after = torch.as_tensor(getattr(after, 'rep', after)).reshape(-1).to(before.device)
    n, total = before.numel(), after.numel()
    if total < n:
        raise ValueError('density_changes: %d labels before, %d after' % (n, total))
    row = torch.arange(n, device=before.device, dtype=torch.int64)
    old = after[:n]
    gone = row[(before == row) & (old != row)]

    def spread(key, value):
        """per row: do all rows with this row's key carry one value?"""
        lo = torch.full((total,), total, device=key.device, dtype=torch.int64).scatter_reduce_(0, key, value, 'amin')
        hi = torch.full((total,), -1, device=key.device, dtype=torch.int64).scatter_reduce_(0, key, value, 'amax')
        return lo[key] == hi[key]

    # a cluster of `after` kept its old members iff they come from one cluster of `before` and that one went nowhere else
    same = spread(old, before) & spread(before, old)
    return gone, torch.unique(torch.cat((old[~same], after[n:])))


def _rekey(best, old_to_new):
    """Keys best[.] int64 whose core rows survive -> the same keys with the core row (0xFFFFFFFF minus the low word)
    renumbered through old_to_new; the score bits in the high word are untouched, 0 stays 0."""
    has = best != 0
    core = torch.where(has, 0xFFFFFFFF - (best & 0xFFFFFFFF), torch.zeros_like(best))
    return torch.where(has, (best & ~0xFFFFFFFF) | (0xFFFFFFFF - old_to_new[core]), best)


def density_remove(engine, emb, threshold, min_rows, earlier, rows=None, keep=None, norms=None):
    """Take rows out of a density-gated clustering of emb[N,512] -> (DensityClusters, DensityState, old_to_new int64[N] with
    -1 for a removed row, kept int64[N_s]: the surviving rows, new-to-old).  Clusters and state are those of the survivors
    in compact numbering, the keys of the state re-encoded: they equal density_extend(engine, emb[kept], threshold, min_rows)
    when `earlier` is the DensityState of all N rows; it is left as it is.  Give exactly one of rows (indices to remove,
    duplicates allowed) and keep (mask of the rows that stay).  emb is not touched: compact it with emb[kept].  A state made
    with another threshold or min_rows is refused."""
    threshold, min_rows = float(threshold), int(min_rows)
    if float(earlier.threshold) != threshold or int(earlier.min_rows) != min_rows:
        raise RuntimeError('ffrnet_amd: the state was made with threshold %r and min_rows %d; rows cannot be removed from it '
                           'with %r and %d' % (earlier.threshold, earlier.min_rows, threshold, min_rows))
    n = emb.size(0)
    if earlier.rep.numel() != n:
        raise RuntimeError('ffrnet_amd: a state of %d rows for %d embeddings' % (earlier.rep.numel(), n))
    mask = _keep_mask(n, rows, keep, emb.device)
    old_to_new, kept = _index_maps(mask)
    rep, kind, degree, best = engine.cluster_density_remove(emb, threshold, min_rows, earlier.rep.clone(), earlier.degree.clone(),
                                                            earlier.best.clone(), mask, norms=norms)
    rep, kind, degree, best = old_to_new[rep[kept]], kind[kept], degree[kept], _rekey(best[kept], old_to_new)
    return density_ids(rep, kind), DensityState(rep, kind, degree, best, threshold, min_rows), old_to_new, kept


def density_removal_changes(before, after):
    """What a removal did to the clusters of a density-gated clustering: -> (drop, compute), both int64, ascending, in the
    numbering BEFORE the removal.  before, after: rep tensors of the same N rows, or anything with a .rep; after as
    Engine.cluster_density_remove returns it (same numbering, -1 for a removed row).  drop: the representatives of `before`
    whose cluster lost a row or whose survivors are not exactly the members of one cluster of `after`.  compute: the
    representatives of `after` whose members are not exactly the members of one cluster of `before`.  A caller that keeps
    one template per cluster drops those of `drop` and computes those of `compute`; every other cluster kept its rows and
    its label.

    removal_changes() is not enough here: it looks at the clusters that lost a row only, but a border row whose core row
    was removed or demoted may move to ANOTHER cluster, which lost nothing and changes all the same."""
    before = torch.as_tensor(getattr(before, 'rep', before)).reshape(-1).to(torch.int64)
    after = torch.as_tensor(getattr(after, 'rep', after)).reshape(-1).to(device=before.device, dtype=torch.int64)
    n = before.numel()
    if after.numel() != n:
        raise ValueError('density_removal_changes: %d labels before, %d after' % (n, after.numel()))
    stay = after >= 0
    b, a = before[stay], after[stay]
    lost = torch.zeros((n,), device=before.device, dtype=torch.bool)
    lost[before[~stay]] = True

    def spread(key, value):
        """per row: do all rows with this row's key carry one value?"""
        lo = torch.full((n,), n, device=key.device, dtype=torch.int64).scatter_reduce_(0, key, value, 'amin')
        hi = torch.full((n,), -1, device=key.device, dtype=torch.int64).scatter_reduce_(0, key, value, 'amax')
        return lo[key] == hi[key]

    # a cluster kept its members iff it lost none, they are in one cluster of `after`, and that one holds nothing else
    changed = lost[b] | ~(spread(a, b) & spread(b, a))
    return torch.unique(torch.cat((before[~stay], b[changed]))), torch.unique(a[changed])


# IncrementalDensity.remove: the removal scores at least r * n pairs (the r removed rows against everything held), clustering
# the ns survivors again scores ns * (ns - 1).  The removal is taken iff r * n <= REMOVE_PAIR_RATIO * ns * (ns - 1).  Measured
# (tools/bench_cluster_density_remove.py, EXPERIMENTS.md): at r * n / (ns * (ns - 1)) <= 0.444 the removal was 1.5 x to 290 x
# faster than clustering again, at 2.0 (half of the rows leave) 1.6 x slower; the plain pair-count rule, 1.0, sends no
# measured shape to the slower route.
REMOVE_PAIR_RATIO = 1.0


def density_remove_route(n, ns):
    """The route IncrementalDensity.remove takes for n rows held of which ns survive -> 'remove' or 'recluster'."""
    return 'remove' if (n - ns) * n <= REMOVE_PAIR_RATIO * ns * (ns - 1) else 'recluster'


class IncrementalDensity(object):
    """A density-gated clustering that keeps being added to: embeddings [n,512], their norms and the state (rep, kind,
    degree, best) on the Engine's device, in grow-only buffers (as Incremental).  After every add() the labels are those of
    density() over all rows held.  Between removals rows keep their index; unlike Incremental, the rep of an old row can
    also rise (density_changes tells which templates to drop and which to compute).  remove() takes rows out, compacts the
    buffers and returns the old-to-new index map; afterwards labels and state are those of density() over the rows still
    held, so add() goes on as before (density_removal_changes, on the labels before compaction, tells which templates to
    drop and compute)."""

    def __init__(self, engine, threshold, min_rows, capacity=0):
        engine._min_rows(min_rows, 'IncrementalDensity')
        self.engine = engine
        self.threshold = float(threshold)
        self.min_rows = int(min_rows)
        self._n = 0
        cap, dev = int(capacity), engine.device
        self._emb = torch.empty((cap, 512), device=dev, dtype=torch.float32)
        self._norms = torch.empty((cap,), device=dev, dtype=torch.float32)
        self._rep = torch.empty((cap,), device=dev, dtype=torch.int64)
        self._kind = torch.empty((cap,), device=dev, dtype=torch.uint8)
        self._degree = torch.empty((cap,), device=dev, dtype=torch.int32)
        self._best = torch.empty((cap,), device=dev, dtype=torch.int64)

    def __len__(self):
        return self._n

    @property
    def embeddings(self):
        return self._emb[:self._n]

    @property
    def norms(self):
        return self._norms[:self._n]

    @property
    def rep(self):
        return self._rep[:self._n]

    @property
    def kind(self):
        return self._kind[:self._n]

    @property
    def degree(self):
        return self._degree[:self._n]

    @property
    def state(self):
        return DensityState(self.rep, self.kind, self.degree, self._best[:self._n], self.threshold, self.min_rows)

    @property
    def clusters(self):
        return density_ids(self.rep, self.kind)

    def templates(self):
        """One unit template per cluster that has a core, in order of representative -> [C',512]: what gets enrolled."""
        c = self.clusters
        return templates(self.engine, self.embeddings, c, norms=self.norms)[c.has_core]

    def add(self, emb):
        """Append emb[n,512] (fp32, on the Engine's device) and extend the clustering -> the index of its first row."""
        n, first = _batch_rows('IncrementalDensity', emb), self._n
        self._emb, self._norms, self._rep, self._kind, self._degree, self._best = _grown(
            (self._emb, self._norms, self._rep, self._kind, self._degree, self._best), first, first + n)
        if n:
            total = first + n
            self._emb[first:total] = emb
            self._norms[first:total] = self.engine.row_norms(self._emb[first:total])
            _, kind, _, _ = self.engine.cluster_density_extend(
                self._emb[:total], self.threshold, self.min_rows, self._rep[:total], self._degree[:total], self._best[:total],
                first, norms=self._norms[:total], validate=False)
            self._kind[:total] = kind
            self._n = total
        return first

    def remove(self, rows, route=None):
        """Take the rows with these indices out (any integer sequence or tensor; duplicates allowed) and compact all six
        buffers in order -> old_to_new int64[n]: the new index of every row held before, -1 for a removed one.  Afterwards
        labels and state are those of density() over the rows still held, and add() works as before.  Two routes leave the
        identical state: the removal (Engine.cluster_density_remove, then compaction with the keys re-encoded), and
        compaction followed by clustering the survivors from scratch.  Unlike single link, the removal can lose: it scores
        the removed rows against everything.  route: None chooses by density_remove_route; 'remove' / 'recluster' force one."""
        n = self._n
        keep = _keep_mask(n, rows, None, self._rep.device)
        old_to_new, kept = _index_maps(keep)
        ns = kept.numel()
        if route is None:
            route = density_remove_route(n, ns)
        if route not in ('remove', 'recluster'):
            raise ValueError("ffrnet_amd: route must be 'remove' or 'recluster', got %r" % (route,))
        if ns == n:
            return old_to_new
        if ns and route == 'remove':
            rep, kind, degree, best = self.engine.cluster_density_remove(
                self._emb[:n], self.threshold, self.min_rows, self._rep[:n], self._degree[:n], self._best[:n], keep,
                norms=self._norms[:n], validate=False)
            rep, kind, degree, best = old_to_new[rep[kept]], kind[kept], degree[kept], _rekey(best[kept], old_to_new)
        self._emb[:ns] = self._emb[:n][kept]
        self._norms[:ns] = self._norms[:n][kept]
        if ns and route == 'recluster':
            rep, kind, degree, best = self.engine.cluster_density_extend(
                self._emb[:ns], self.threshold, self.min_rows, None, None, None, 0, norms=self._norms[:ns], validate=False)
        if ns:
            self._rep[:ns], self._kind[:ns], self._degree[:ns], self._best[:ns] = rep, kind, degree, best
        self._n = ns
        return old_to_new


def member_order(clusters):
    """-> (order[N], offsets[C+1]) int64: the rows sorted by cluster id then row index, and each cluster's slice of them."""
    cid = clusters.cluster_id
    order = torch.argsort(cid, stable=True)
    offsets = torch.zeros((clusters.n_clusters + 1,), device=cid.device, dtype=torch.int64)
    offsets[1:] = torch.cumsum(clusters.sizes, 0)
    return order, offsets


def templates(engine, emb, clusters, norms=None):
    """One unit template per cluster, row c for cluster id c: the normalised sum of the cluster's normalised rows
    -> [C,512], ready for Gallery.add."""
    order, offsets = member_order(clusters)
    if clusters.cluster_id.numel() != emb.size(0):
        raise RuntimeError('ffrnet_amd: %d cluster ids for %d embeddings' % (clusters.cluster_id.numel(), emb.size(0)))
    return engine.cluster_templates(emb, order, offsets, norms=norms, validate=False)     # in range by construction


def pairwise_scores(pred, truth):
    """Pair-counting agreement of two labelings of the same N rows -> (precision, recall, f): over all N(N-1)/2 row pairs,
    precision = pairs together in both / pairs together in pred, recall = ... / pairs together in truth, f their harmonic
    mean.  From exact integer contingency counts; an empty denominator counts as 1.0.  Host logic: any device, any
    integer labels."""
    pred = torch.as_tensor(pred).reshape(-1).cpu()
    truth = torch.as_tensor(truth).reshape(-1).cpu()
    if pred.numel() != truth.numel():
        raise ValueError('pairwise_scores: %d predicted labels, %d true labels' % (pred.numel(), truth.numel()))

    def pairs(counts):
        return sum(c * (c - 1) // 2 for c in counts.tolist())

    _, p = torch.unique(pred, return_inverse=True)
    _, t = torch.unique(truth, return_inverse=True)
    nt = int(t.max()) + 1 if t.numel() else 1
    together_pred = pairs(torch.unique(p, return_counts=True)[1])
    together_truth = pairs(torch.unique(t, return_counts=True)[1])
    both = pairs(torch.unique(p * nt + t, return_counts=True)[1])
    precision = both / together_pred if together_pred else 1.0
    recall = both / together_truth if together_truth else 1.0
    f = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
    return precision, recall, f
