"""Clustering an embedding table: Lloyd's k-means on the device, and the partition scores that embedding papers report next to
F1 (NMI, ARI, purity) on the host.

One iteration is three launches on the table in device memory and a 16-byte read:

    assign   ops.kmeans_assign   labels[i] = argmin_j |x_i - c_j|^2 (a tie to the lowest j), inertia = sum_i |x_i - c_labels[i]|^2
                                 and the number of rows whose label moved -- the fused sweep of csrc/gs_kmeans.hip
    group    ops.kmeans_members  the rows of every cluster, in ascending row order (rowptr, members)
    update   ops.csr_reduce_fwd  c_j = the mean of cluster j's rows: the segmented mean of exact inference (CSR_MEAN), clusters
                                 of more than 512 rows cut and combined in slot order; an empty cluster keeps its centre

No float atomics anywhere and the seeding draws from one RandomState: the same call twice gives the same bits.

The loop: assign to C_t; stop as 'converged' if no label moved, as 'tol' if inertia_(t-1) - inertia_t <= tol * inertia_(t-1),
as 'max_iter' after max_iter assignments; else update to C_(t+1).  The returned labels are therefore the assignment to the
returned centres, and Clustering.predict on the same rows reproduces them bit for bit.
"""
from __future__ import division, print_function

import time

import numpy as np

from ._lib import KMEANS_MAX_K, GraphsageAmdError

MAX_D = 1024             # the sweep's width limit (gs_kmeans_assign)
SPLIT_LEN = 512          # clusters longer than this are cut, as neighbor lists are (inference.SPLIT_LEN)
LINE_PREFIX = "Embedding clusters:"
LINE_FILE = "eval_clusters.txt"


# ------------------------------------------------------------------------------------------------ seeding (host, fp64)
def seed_subsample(n, k, rs):
    """The positions k-means++ runs on: m = min(n, max(4096, 32 k)) of the n rows, drawn without replacement from `rs`
    (np.random.RandomState) and sorted ascending; all of them, without a draw, when m == n."""
    m = min(int(n), max(4096, 32 * int(k)))
    if m == n:
        return np.arange(n, dtype=np.int64)
    return np.sort(rs.choice(n, size=m, replace=False)).astype(np.int64)


def kmeanspp(P, k, rs):
    """Plain k-means++ (Arthur & Vassilvitskii 2007) on the rows of P [m, d] in fp64: the first centre is row rs.randint(m),
    every further one is drawn with probability proportional to the squared distance to the nearest centre so far, by one
    rs.random_sample() against the running sum.  Returns the k chosen row positions, in the order drawn.  A row at distance 0
    is never drawn, so fewer than k distinct rows is refused."""
    P = np.asarray(P, dtype=np.float64)
    m = P.shape[0]
    if k > m:
        raise GraphsageAmdError("k-means++: k=%d centres from %d rows" % (k, m))
    chosen = [int(rs.randint(m))]
    d2 = ((P - P[chosen[0]]) ** 2).sum(axis=1)
    while len(chosen) < k:
        cum = np.cumsum(d2)
        if not cum[-1] > 0.0:
            raise GraphsageAmdError("k-means++: the subsample of %d rows has only %d distinct rows, k=%d" % (m, len(chosen), k))
        j = min(int(np.searchsorted(cum, rs.random_sample() * cum[-1], side="right")), m - 1)
        while d2[j] == 0.0:                      # the rounding of the product put it on a plateau of the running sum
            j -= 1
        chosen.append(j)
        d2 = np.minimum(d2, ((P - P[j]) ** 2).sum(axis=1))
    return np.asarray(chosen, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ metrics (host, fp64)
def contingency(labels_pred, labels_true):
    """The integer table n[i][j] = #{rows with true class i and predicted cluster j} over the classes / clusters that occur."""
    labels_pred, labels_true = np.asarray(labels_pred).ravel(), np.asarray(labels_true).ravel()
    if labels_pred.shape != labels_true.shape or labels_pred.size == 0:
        raise ValueError("cluster_metrics: two label vectors of the same positive length")
    _, ti = np.unique(labels_true, return_inverse=True)
    _, pi = np.unique(labels_pred, return_inverse=True)
    nt, npred = int(ti.max()) + 1, int(pi.max()) + 1
    return np.bincount(ti.astype(np.int64) * npred + pi, minlength=nt * npred).reshape(nt, npred).astype(np.int64)


def cluster_metrics(labels_pred, labels_true):
    """{'nmi', 'ari', 'purity'} of a partition against class labels, in fp64 from the integer contingency table.
    nmi: mutual information over the ARITHMETIC mean of the two entropies; with one class on either side it is 1.0 when both
    sides have one, else 0.0.  ari: the adjusted Rand index (Hubert & Arabie 1985); 1.0 where its denominator vanishes.
    purity: the share of rows that carry the most frequent class of their cluster."""
    tab = contingency(labels_pred, labels_true)
    n = float(tab.sum())
    a, b = tab.sum(axis=1).astype(np.float64), tab.sum(axis=0).astype(np.float64)
    if len(a) == 1 or len(b) == 1:
        nmi = 1.0 if len(a) == 1 and len(b) == 1 else 0.0
    else:
        nz = tab > 0
        nij = tab[nz].astype(np.float64)
        outer = np.outer(a, b)[nz]
        mi = float((nij / n * (np.log(nij) + np.log(n) - np.log(outer))).sum())
        hu = -float((a / n * np.log(a / n)).sum())
        hv = -float((b / n * np.log(b / n)).sum())
        nmi = max(0.0, mi) / (0.5 * (hu + hv))
    comb = lambda x: x * (x - 1.0) / 2.0
    s_ij, s_a, s_b = float(comb(tab.astype(np.float64)).sum()), float(comb(a).sum()), float(comb(b).sum())
    expected = s_a * s_b / comb(n) if n > 1 else 0.0
    den = 0.5 * (s_a + s_b) - expected
    ari = 1.0 if den == 0.0 else (s_ij - expected) / den
    purity = float(tab.max(axis=0).sum()) / n
    return {"nmi": float(nmi), "ari": float(ari), "purity": purity}


# ------------------------------------------------------------------------------------------------ refusals
def refuse(k, width=None, n=None):
    """The cases the kernels do not take, as a ValueError with the rule in the message: k outside [1, 4096], a table wider
    than 1024 columns (after padding to a multiple of 4), more clusters than rows."""
    if k < 1 or k > KMEANS_MAX_K:
        raise ValueError("k=%d clusters: the k-means kernel takes 1 to %d" % (k, KMEANS_MAX_K))
    if width is not None and (width < 1 or -(-width // 4) * 4 > MAX_D):
        raise ValueError("table width %d is over the k-means kernel's limit of %d" % (width, MAX_D))
    if n is not None and k > n:
        raise ValueError("k=%d clusters of %d rows" % (k, n))


# ------------------------------------------------------------------------------------------------ device side
class _Problem(object):
    """A table, its rows and what every assignment of them needs: |x_i|^2, the workspace, the 16-byte result."""

    def __init__(self, engine, Z, rows):
        import torch
        from . import evaluation, ops
        self.width = evaluation._width(Z)
        self.table = evaluation.as_table(engine, Z)
        self.dev = self.table.buf.device
        self.rows, self.n = evaluation._rows(self.table, rows, self.dev)
        self.xsq = ops.kmeans_sqnorm(self.table, rows=self.rows, n=self.n)
        self.ws = torch.empty(max(ops.kmeans_assign_ws_bytes(self.n) // 8, 2), dtype=torch.int64, device=self.dev)
        self.stats = torch.zeros(2, dtype=torch.int64, device=self.dev)

    def centres(self, C):
        """fp32 [k, width] on the host -> Mat [k, padded width] (pad columns zero)."""
        from .ops import Mat
        C = np.ascontiguousarray(C, dtype=np.float32)
        if C.ndim != 2 or C.shape[1] != self.width:
            raise ValueError("the centres are %s, the table is %d wide" % (C.shape, self.width))
        m = Mat.from_numpy(C, self.dev)
        return Mat(m.buf, self.table.d)

    def assign(self, C, prev=None, assign=None, dist=None):
        from . import ops
        csq = ops.kmeans_sqnorm(C)
        ops.kmeans_assign(self.table, C, csq, rows=self.rows, n=self.n, xsq=self.xsq, prev=prev, assign=assign, dist=dist,
                          stats=self.stats, ws=self.ws)
        return ops.kmeans_stats(self.stats)


class Clustering(object):
    """A fitted k-means: centers fp32 [k, d], labels int32 [n] (the assignment of the fitted rows to `centers`), inertia (the
    fp64 sum of their squared distances), iters (assignments made), stop ('converged' | 'tol' | 'max_iter'), sizes int64 [k],
    empty (clusters without a row) and the seeds' row positions (`seeds`: positions among the fitted rows; None for an
    explicit init)."""

    def __init__(self, engine, centers, labels, inertia, iters, stop, seeds=None, history=None):
        self.engine, self.centers, self.labels, self.inertia, self.iters, self.stop = engine, centers, labels, inertia, iters, stop
        self.k = centers.shape[0]
        self.sizes = np.bincount(labels, minlength=self.k).astype(np.int64)
        self.empty = int((self.sizes == 0).sum())
        self.seeds, self.history = seeds, history

    def predict(self, Z, rows=None):
        """int32 [n]: the nearest centre of every row (rows None: all) -- assign only."""
        import torch
        p = _Problem(self.engine, Z, rows)
        out = torch.empty(p.n, dtype=torch.int32, device=p.dev)
        p.assign(p.centres(self.centers), assign=out)
        return out.cpu().numpy()


def _update(p, C, C_next, labels, scratch):
    """C_next = the means of the clusters of `labels`, an empty cluster keeping its row of C; returns the sizes."""
    import torch
    from . import ops
    from ._lib import CSR_MEAN
    from .inference import plan_work_items
    k = C.rows
    rowptr, members = ops.kmeans_members(labels, k, rows=p.rows, rowptr=scratch["rowptr"], members=scratch["members"],
                                         ws=scratch["members_ws"])
    rp = rowptr.cpu().numpy()
    items, _, splits = plan_work_items(rp, SPLIT_LEN)
    n_slots = int(splits[:, 2].sum()) if len(splits) else 0
    ws = None
    if n_slots:
        ws = torch.empty(ops.csr_reduce_ws_bytes(n_slots, C.d) // 4, dtype=torch.float32, device=p.dev)
    ops.csr_reduce_fwd(rowptr, members, torch.from_numpy(items).to(p.dev),
                       torch.from_numpy(splits).to(p.dev) if len(splits) else None, k, SPLIT_LEN, CSR_MEAN, p.table, C_next,
                       0, k, (0, items.shape[0]), (0, splits.shape[0]), (0, n_slots), ws=ws)
    sizes = np.diff(rp)
    if (sizes == 0).any():
        keep = torch.from_numpy(sizes == 0).to(p.dev)
        C_next.buf.copy_(torch.where(keep[:, None], C.buf, C_next.buf))
    return sizes


def fit_kmeans(engine, Z, k, rows=None, init="kmeans++", seed=123, max_iter=100, tol=1e-4, keep_history=False):
    """Lloyd's k-means on rows `rows` (None: all) of the table Z (whatever evaluation.as_table accepts).  init: "kmeans++"
    (seed_subsample + kmeanspp from one np.random.RandomState(seed), the subsample gathered once from the device) or an
    explicit [k, d] array.  keep_history=True keeps the labels of every iteration (Clustering.history).  Returns a Clustering."""
    import torch
    from . import evaluation
    from .ops import Mat
    k = int(k)
    try:
        refuse(k, evaluation._width(Z))
    except ValueError as e:
        raise GraphsageAmdError("fit_kmeans: %s" % e)
    if max_iter < 1:
        raise GraphsageAmdError("fit_kmeans: max_iter=%d must be at least 1" % max_iter)
    p = _Problem(engine, Z, rows)
    if k > p.n or k > p.table.rows:
        raise GraphsageAmdError("fit_kmeans: k=%d clusters of %d rows (a table of %d)" % (k, p.n, p.table.rows))
    seeds = None
    if isinstance(init, str):
        if init != "kmeans++":
            raise GraphsageAmdError("fit_kmeans: init is 'kmeans++' or a [k, d] array, not %r" % init)
        rs = np.random.RandomState(seed)
        sub = seed_subsample(p.n, k, rs)
        sub_dev = torch.from_numpy(sub).to(p.dev)
        pos = p.rows.long()[sub_dev] if p.rows is not None else sub_dev
        P = p.table.buf[pos][:, :p.width].cpu().numpy()               # the one gather
        chosen = kmeanspp(P, k, rs)
        seeds = sub[chosen]
        init = P[chosen]
    init = np.asarray(init, dtype=np.float32)
    if init.shape != (k, p.width):
        raise GraphsageAmdError("fit_kmeans: init is %s, not [k=%d, d=%d]" % (init.shape, k, p.width))
    C = p.centres(init)
    C_next = Mat(torch.zeros_like(C.buf), C.d)
    from . import ops
    cur = torch.empty(p.n, dtype=torch.int32, device=p.dev)
    prev = torch.full((p.n,), -1, dtype=torch.int32, device=p.dev)
    scratch = {"rowptr": torch.empty(k + 1, dtype=torch.int64, device=p.dev),
               "members": torch.empty(p.n, dtype=torch.int32, device=p.dev),
               "members_ws": torch.empty(max(ops.kmeans_members_ws_bytes(p.n, k) // 4, 1), dtype=torch.int32, device=p.dev)}
    history = [] if keep_history else None
    inertia_prev, stop, iters = None, None, 0
    while stop is None:
        inertia, changed = p.assign(C, prev=prev, assign=cur)
        iters += 1
        if history is not None:
            history.append(cur.cpu().numpy())
        if changed == 0:
            stop = "converged"
        elif inertia_prev is not None and inertia_prev - inertia <= tol * inertia_prev:
            stop = "tol"
        elif iters >= max_iter:
            stop = "max_iter"
        else:
            _update(p, C, C_next, cur, scratch)
            C, C_next = C_next, C
            cur, prev = prev, cur
            inertia_prev = inertia
    return Clustering(engine, C.buf[:, :p.width].cpu().numpy().copy(), cur.cpu().numpy(), inertia, iters, stop, seeds=seeds,
                      history=history)


# ------------------------------------------------------------------------------------------------ what the drivers print
def result_line(res):
    return ("%s k= %d nodes= %d inertia= %.6f iters= %d stop= %s empty= %d size_min= %d size_max= %d nmi= %.5f ari= %.5f "
            "purity= %.5f time= %.5f" % (LINE_PREFIX, res["k"], res["nodes"], res["inertia"], res["iters"], res["stop"],
                                         res["empty"], res["size_min"], res["size_max"], res["nmi"], res["ari"], res["purity"],
                                         res["time"]))


def single_label_classes(G):
    """The number of classes of a dataset whose nodes carry ONE class id each; None for multi-label or unlabelled data."""
    labels = getattr(G, "labels", None)
    if labels is None:
        return None
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.size == 0 or labels.dtype.kind not in "iu":
        return None
    return int(labels.max()) + 1


def refuse_flags(flag, K, width=None, save_embeddings=True, G=None, single_label=None):
    """What --eval_clusters / --clusters K cannot do, as a SystemExit with the rule in the message.  single_label: what is
    known of the dataset before it is loaded (False: no single-label classes; None: unknown).  Returns the k to fit (K = -1:
    the dataset's number of classes once G is given, else -1)."""
    K = int(K)
    if K == 0:
        return 0
    if not save_embeddings:
        raise SystemExit("%s clusters the rows of val.npy: it needs --save_embeddings true" % flag)
    if K != -1 and not 1 <= K <= KMEANS_MAX_K:
        raise SystemExit("%s %d: the number of clusters is -1 (the dataset's classes) or 1 to %d" % (flag, K, KMEANS_MAX_K))
    if width is not None:
        try:
            refuse(1, width)
        except ValueError as e:
            raise SystemExit("%s: %s" % (flag, e))
    if K == -1 and single_label is False:
        raise SystemExit("%s -1 takes the number of classes of a single-label dataset; this one has none" % flag)
    if G is None:
        return K
    if K == -1:
        K = single_label_classes(G)
        if K is None:
            raise SystemExit("%s -1 takes the number of classes of a single-label dataset; this one has none" % flag)
        if K > KMEANS_MAX_K:
            raise SystemExit("%s -1: the dataset has %d classes, the k-means kernel takes 1 to %d" % (flag, K, KMEANS_MAX_K))
    n = int(np.asarray(G.present).sum()) if getattr(G, "present", None) is not None else G.n_nodes
    if K > n:
        raise SystemExit("%s %d: more clusters than the graph's %d nodes" % (flag, K, n))
    return K


def evaluate_embedding_dir(engine, G, embed_dir, K, base="val", seed=123, flag="--eval_clusters"):
    """Cluster ALL rows of <embed_dir>/<base>.npy into K groups (K = -1: the dataset's number of classes), score the groups
    against the single-label classes of the nodes that <base>.txt names (nan where the dataset has none), print the
    `Embedding clusters:` line and write eval_clusters.txt, clusters.npy (int32, one label per row of the table, in the order
    of <base>.txt) and cluster_centers.npy (float32 [K, width])."""
    import os
    from . import evaluation
    t0 = time.time()
    emb, index = evaluation.load_table(embed_dir, base)
    k = refuse_flags(flag, K, width=emb.shape[1], G=G)
    if k > emb.shape[0]:
        raise SystemExit("%s %d: more clusters than the table's %d rows" % (flag, k, emb.shape[0]))
    try:
        fit = fit_kmeans(engine, emb, k, seed=seed)
    except GraphsageAmdError as e:
        raise SystemExit("%s: %s" % (flag, e))
    scores = {"nmi": float("nan"), "ari": float("nan"), "purity": float("nan")}
    if single_label_classes(G) is not None:
        ids = getattr(G, "node_ids", None)
        key = (lambda r: str(ids[r])) if ids is not None else (lambda r: str(r))
        nodes = np.array([r for r in range(G.n_nodes) if key(r) in index], dtype=np.int64)
        if len(nodes):
            table_rows = np.array([index[key(r)] for r in nodes], dtype=np.int64)
            scores = cluster_metrics(fit.labels[table_rows], np.asarray(G.labels)[nodes])
    res = {"k": k, "nodes": int(emb.shape[0]), "inertia": fit.inertia, "iters": fit.iters, "stop": fit.stop, "empty": fit.empty,
           "size_min": int(fit.sizes.min()), "size_max": int(fit.sizes.max()), "time": time.time() - t0, "clustering": fit}
    res.update(scores)
    line = result_line(res)
    print(line)
    with open(os.path.join(embed_dir, LINE_FILE), "w") as fp:
        fp.write(line + "\n")
    np.save(os.path.join(embed_dir, "clusters.npy"), fit.labels.astype(np.int32))
    np.save(os.path.join(embed_dir, "cluster_centers.npy"), fit.centers.astype(np.float32))
    return res
