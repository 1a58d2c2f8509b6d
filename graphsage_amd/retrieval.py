"""Approximate top-k partners through an inverted file (IVF) over a k-means partition of the embedding table.

    index = build_ivf(engine, Z, n_clusters=0, n_cand=N)          # clustering.fit_kmeans + IVFIndex.from_labels
    res = index.search(nodes, k=10, nprobe=8, filt=RankFilter.from_full_graph(graph))
    res["ids"], res["scores"], res["count"]                        # what inference.topk_full returns
    res["scanned"]                                                 # int64 [n]: the members of the lists each query probed

The index is the centres (clusters without a member dropped, the rest re-numbered in ascending old id) and, per cluster, its
rows in ascending id (ops.kmeans_members).  A query probes the nprobe centres that come first by (<x_q, c_j> descending, j
ascending) -- <x_q, c_j> is the mean score of list j's members, also for bilinear queries x_q = Z[u] . A -- and gets the first k
of topk_full's candidates among the members of those lists, in topk_full's order (score descending, id ascending), padded with
-1 / -inf.  One library call per 65,536 queries (gs_ivf_search, csrc/gs_ivf.hip); the arithmetic, the order and the merge are
those of gs_topk_select, so a search that probes ALL lists returns topk_full's ids, score bits and counts.
"""
from __future__ import division, print_function

import os

import numpy as np

from . import ops
from ._lib import KMEANS_MAX_K, GraphsageAmdError

MAX_CLUSTERS = 4096          # the largest default (and KMEANS_MAX_K)
LINE_PREFIX = "IVF top-K partners:"
LINE_FILE = "topk_ivf.txt"
CENTERS_FILE, LABELS_FILE = "ivf_centers.npy", "ivf_labels.npy"


def default_clusters(n_cand):
    """min(4096, max(1, round(4 sqrt(n_cand)))), and never more than the rows there are."""
    return int(max(1, min(MAX_CLUSTERS, int(n_cand), int(round(4.0 * np.sqrt(max(int(n_cand), 0)))))))


def renumber(centers, labels):
    """The host half of IVFIndex.from_labels: centers float32 [C, d] and labels int32 [n_cand] with entries in [0, C), checked;
    clusters without a member dropped and the rest re-numbered in ascending old id.  Returns (centers float32 [C', d], labels
    int32 [n_cand] in the new numbering, empty = C - C')."""
    centers = np.asarray(centers, dtype=np.float32)
    labels = np.asarray(labels)
    if centers.ndim != 2 or not 1 <= centers.shape[0] <= KMEANS_MAX_K:
        raise GraphsageAmdError("IVF: centers must be [C, d] with 1 <= C <= %d, got %s" % (KMEANS_MAX_K, centers.shape))
    if labels.ndim != 1 or labels.size == 0 or labels.dtype.kind not in "iu":
        raise GraphsageAmdError("IVF: labels must be a non-empty integer vector, one cluster id per candidate row")
    C = centers.shape[0]
    if labels.min() < 0 or labels.max() >= C:
        raise GraphsageAmdError("IVF: labels must lie in [0, %d) (found %d .. %d)" % (C, labels.min(), labels.max()))
    sizes = np.bincount(labels, minlength=C)
    keep = np.flatnonzero(sizes > 0)
    new_id = np.full(C, -1, np.int64)
    new_id[keep] = np.arange(keep.size)
    return np.ascontiguousarray(centers[keep]), new_id[labels].astype(np.int32), int(C - keep.size)


def recall(ids_approx, ids_exact):
    """The mean, over the queries whose exact row holds an id, of |approx n exact| / |exact ids >= 0| (ids int [n, k]; -1 is
    padding).  Only ids are compared, never scores; nan when no exact row holds an id."""
    a, e = np.asarray(ids_approx), np.asarray(ids_exact)
    if a.ndim != 2 or e.ndim != 2 or a.shape[0] != e.shape[0]:
        raise ValueError("recall: two id matrices with one row per query")
    hit = np.zeros(e.shape[0], np.int64)
    for j in range(a.shape[1]):
        col = a[:, j:j + 1]
        hit += ((col == e) & (col >= 0)).any(axis=1)
    size = (e >= 0).sum(axis=1).astype(np.int64)
    rows = size > 0
    if not rows.any():
        return float("nan")
    return float(np.mean(hit[rows] / size[rows]))


class IVFIndex(object):
    """centers float32 [C', d] and labels int32 [n_cand] (host; the saved form), empty (clusters dropped), sizes int64 [C']; on
    the device the table Z, the centres as a Mat and the lists list_ptr int64 [C' + 1] / list_ids int32 [n_cand]."""

    def __init__(self, engine, Z, centers, labels, empty):
        import torch
        from . import evaluation
        self.engine = engine
        engine.sync()                # Z may have been written on the engine's stream; the grouping below runs on torch's
        self.Z = evaluation.as_table(engine, Z)
        self.centers, self.labels, self.empty = centers, labels, int(empty)
        self.n_cand, self.n_clusters = int(labels.shape[0]), int(centers.shape[0])
        if self.n_cand > self.Z.rows:
            raise GraphsageAmdError("IVF: %d labels for a table of %d rows" % (self.n_cand, self.Z.rows))
        if ops.round_up(centers.shape[1], 4) != self.Z.d:
            raise GraphsageAmdError("IVF: the centres are %d wide, the table %d" % (centers.shape[1], self.Z.d))
        self.sizes = np.bincount(labels, minlength=self.n_clusters).astype(np.int64)
        dev = self.Z.buf.device
        m = ops.Mat.from_numpy(centers, dev)
        self.centers_dev = ops.Mat(m.buf, self.Z.d)
        self.list_ptr, self.list_ids = ops.kmeans_members(torch.from_numpy(labels).to(dev), self.n_clusters)
        torch.cuda.synchronize()

    @classmethod
    def from_labels(cls, engine, Z, centers, labels, n_cand=None):
        """An index from a given partition: labels[i] = the cluster of table row i, i < n_cand (default: every row of Z)."""
        labels = np.asarray(labels)
        if n_cand is not None and labels.shape[0] != int(n_cand):
            raise GraphsageAmdError("IVF: %d labels for n_cand = %d" % (labels.shape[0], int(n_cand)))
        return cls(engine, Z, *renumber(centers, labels))

    def search(self, nodes, k, nprobe, filt=None, exclude_self=True, weights=None, chunk=ops.RANK_CHUNK):
        """inference.topk_full restricted to the members of the nprobe lists every query probes; the same arguments and the same
        result dict plus "scanned" (int64 [n]).  chunk: the queries of one library call (the result does not depend on it)."""
        import torch
        from .inference import _queries
        nodes = np.ascontiguousarray(np.asarray(nodes).reshape(-1), dtype=np.int64)
        Q, k, nprobe, Z = nodes.shape[0], int(k), int(nprobe), self.Z
        if not 1 <= k <= ops.TOPK_MAX:
            raise GraphsageAmdError("IVF search: k = %d must lie in [1, %d]" % (k, ops.TOPK_MAX))
        if not 1 <= nprobe <= min(ops.IVF_MAX_PROBE, self.n_clusters):
            raise GraphsageAmdError("IVF search: nprobe = %d must lie in [1, min(%d, %d clusters)]"
                                    % (nprobe, ops.IVF_MAX_PROBE, self.n_clusters))
        if Q and (nodes.min() < 0 or nodes.max() >= Z.rows):
            raise GraphsageAmdError("IVF search: node ids must lie in [0, %d)" % Z.rows)
        if Q == 0:
            return {"ids": np.zeros((0, k), np.int32), "scores": np.zeros((0, k), np.float32), "count": np.zeros(0, np.int32),
                    "scanned": np.zeros(0, np.int64)}
        e = self.engine
        out = (torch.zeros((Q, k), dtype=torch.int32, device=e.device), torch.zeros((Q, k), dtype=torch.float32, device=e.device),
               torch.zeros(Q, dtype=torch.int32, device=e.device), torch.zeros(Q, dtype=torch.int64, device=e.device))
        src, Xq, f_rowptr, f_col = _queries(e, Z, nodes, filt, weights, "IVF search")
        ops.ivf_search(Xq, Z, self.centers_dev, self.list_ptr, self.list_ids, k, nprobe, n_cand=self.n_cand,
                       src=src if (exclude_self or filt is not None) else None, keep_src=not exclude_self, f_rowptr=f_rowptr,
                       f_col=f_col, ids=out[0], scores=out[1], count=out[2], scanned=out[3], chunk=chunk, stream=e.stream)
        e.sync()
        return {"ids": out[0].cpu().numpy(), "scores": out[1].cpu().numpy(), "count": out[2].cpu().numpy(),
                "scanned": out[3].cpu().numpy()}

    def save(self, out_dir):
        """ivf_centers.npy (float32 [C', d]) and ivf_labels.npy (int32 [n_cand], the re-numbered ids) under out_dir."""
        np.save(os.path.join(out_dir, CENTERS_FILE), self.centers.astype(np.float32))
        np.save(os.path.join(out_dir, LABELS_FILE), self.labels.astype(np.int32))

    @classmethod
    def load(cls, engine, Z, in_dir):
        """The index that save() wrote, over the table Z: it searches bit-equal to the saved one."""
        return cls.from_labels(engine, Z, np.load(os.path.join(in_dir, CENTERS_FILE)), np.load(os.path.join(in_dir, LABELS_FILE)))


def build_ivf(engine, Z, n_clusters=0, n_cand=None, seed=123, max_iter=20, tol=1e-4, init="kmeans++"):
    """clustering.fit_kmeans on the rows 0 .. n_cand - 1 of Z (default: all) followed by IVFIndex.from_labels.  n_clusters in
    [1, 4096], or 0 for default_clusters(n_cand); init as fit_kmeans takes it ("kmeans++", seeded by `seed` on the host, or
    an explicit [n_clusters, d] array).  The fit is kept as index.clustering."""
    from . import clustering, evaluation
    engine.sync()                    # Z may have been written on the engine's stream; the fit runs on torch's
    Z = evaluation.as_table(engine, Z)
    n_cand = Z.rows if n_cand is None else int(n_cand)
    if not 1 <= n_cand <= Z.rows:
        raise GraphsageAmdError("build_ivf: n_cand = %d, the table has %d rows" % (n_cand, Z.rows))
    n_clusters = int(n_clusters)
    if n_clusters == 0:
        n_clusters = default_clusters(n_cand)
    if not 1 <= n_clusters <= KMEANS_MAX_K:
        raise GraphsageAmdError("build_ivf: n_clusters = %d must lie in [1, %d] (0: the default)" % (n_clusters, KMEANS_MAX_K))
    fit = clustering.fit_kmeans(engine, Z, n_clusters, rows=None if n_cand == Z.rows else np.arange(n_cand, dtype=np.int32),
                                init=init, seed=seed, max_iter=max_iter, tol=tol)
    index = IVFIndex.from_labels(engine, Z, fit.centers, fit.labels, n_cand=n_cand)
    index.clustering = fit
    return index


# ------------------------------------------------------------------------------------------------ what the driver prints
def result_line(res):
    return ("%s k= %d nodes= %d clusters= %d empty= %d nprobe= %d list_min= %d list_max= %d scanned= %.5f filled= %.5f "
            "recall@k= %.5f sample= %d build_time= %.5f search_time= %.5f"
            % (LINE_PREFIX, res["k"], res["nodes"], res["clusters"], res["empty"], res["nprobe"], res["list_min"], res["list_max"],
               res["scanned_share"], res["filled"], res["recall"], res["sample"], res["build_time"], res["search_time"]))


def refuse_flags(K, n_clusters, nprobe, sample):
    """What --topk_ivf K cannot do whatever the data, as a SystemExit with the rule in the message."""
    if not 1 <= K <= ops.TOPK_MAX:
        raise SystemExit("--topk_ivf %d: K must lie in [1, %d]" % (K, ops.TOPK_MAX))
    if not 1 <= nprobe <= ops.IVF_MAX_PROBE:
        raise SystemExit("--topk_ivf_nprobe %d: the lists probed per query are 1 to %d" % (nprobe, ops.IVF_MAX_PROBE))
    if not 0 <= n_clusters <= MAX_CLUSTERS:
        raise SystemExit("--topk_ivf_clusters %d: the number of lists is 0 (4 sqrt(N), at most %d) or 1 to %d"
                         % (n_clusters, MAX_CLUSTERS, MAX_CLUSTERS))
    if sample < 0:
        raise SystemExit("--topk_ivf_recall %d: the exact sample has 0 or more nodes" % sample)
