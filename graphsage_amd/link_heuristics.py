"""Graph-only link-ranking baselines: common neighbors, Adamic-Adar, resource allocation and the Jaccard ratio, ranked the way
rank_full ranks the embeddings -- every held-out edge against ALL nodes, known edges filtered, ties lose.

    graph = SimpleGraph.from_csr(rowptr, col, n_nodes)
    res = rank_neighbors(engine, graph, edges, kind="aa", filt=graph.rank_filter())

The scores live on the simple graph of the CSR they are given: rows sorted strictly ascending, duplicates, self loops and pad
ids (>= n_nodes) removed, NOT symmetrised.  N(w) is the stored row of w, deg(w) = |N(w)|, and for a source u and a candidate x
with P(u, x) = {w : w in N(u), x in N(w)}

    cn       s = |P|
    aa       s = sum over P of q(deg w),  q(k) = max(1, floor(2^S / ln k + 0.5)) for k >= 2, 0 below
    ra       s = sum over P of q(deg w),  q(k) = max(1, floor(2^S / k + 0.5)) for k >= 1, 0 at 0
    jaccard  cn / (deg u + deg x - cn), 0 where cn = 0; ratios compare by cross-multiplication in 64-bit unsigned integers

with the fixed-point shift S = min(16, 31 - bit_length(max_degree)), which keeps every sum below 2^32: the scores are integers,
so every result is exact, order-free and the same bits on every run.  q is computed once per graph in fp64 on the host.  On a
directed graph the Jaccard denominator can be 0 while cn > 0 (x has an empty row and lies in every row of N(u)); cross-
multiplication ranks such a ratio above every finite one and level with its like, and scores_float reports it as inf.

One launch (gs_nbr_rank, csrc/gs_nbr_rank.hip) forms a row of A diag(q) A per distinct source in LDS tiles and counts the
candidates above and level with every partner; no score vector exists.  The law is restated in tests/nbr_rank_oracle.py."""
import math

import numpy as np

from . import ops
from ._lib import GraphsageAmdError

KINDS = ("cn", "aa", "ra", "jaccard")
MAX_SCALE_BITS = 16


def parse_kinds(text):
    """'aa,cn' -> ['aa', 'cn']; 'all' -> every kind; '' -> [].  An unknown name raises ValueError."""
    names = [s.strip() for s in str(text or "").split(",") if s.strip()]
    out = []
    for name in names:
        for kind in (KINDS if name == "all" else (name,)):
            if kind not in KINDS:
                raise ValueError("unknown link-ranking baseline %r: choose from %s or all" % (kind, ", ".join(KINDS)))
            if kind not in out:
                out.append(kind)
    return out


def scale_bits(max_degree):
    """S = min(16, 31 - bit_length(max_degree)): max_degree * (2^S / ln 2 + 0.5) stays below 2^32."""
    return min(MAX_SCALE_BITS, 31 - int(max_degree).bit_length())


def neighbor_weights(kind, deg):
    """(q uint32 [N], scale_bits): the weight of a middle node w by its degree, in fp64 on the host.  cn and jaccard: 1, shift 0."""
    if kind not in KINDS:
        raise GraphsageAmdError("neighbor_weights: kind must be one of %s" % ", ".join(KINDS))
    deg = np.asarray(deg, dtype=np.int64).reshape(-1)
    if deg.size and deg.min() < 0:
        raise GraphsageAmdError("neighbor_weights: a degree is negative")
    if kind in ("cn", "jaccard"):
        return np.ones(deg.shape[0], dtype=np.uint32), 0
    S = scale_bits(int(deg.max()) if deg.size else 0)
    if S < 0:
        raise GraphsageAmdError("neighbor_weights: a degree of 2^31 or more")
    # one Python-float (fp64) evaluation per DISTINCT degree: the same arithmetic wherever the table is rebuilt
    ks, inv = np.unique(deg, return_inverse=True)
    if kind == "aa":
        qs = [max(1, int(math.floor(2.0 ** S / math.log(k) + 0.5))) if k >= 2 else 0 for k in ks.tolist()]
    else:
        qs = [max(1, int(math.floor(2.0 ** S / k + 0.5))) if k >= 1 else 0 for k in ks.tolist()]
    q = np.asarray(qs, dtype=np.int64)[inv.reshape(-1)]
    return q.astype(np.uint32), S


class SimpleGraph(object):
    """A CSR as the simple graph the scores are defined on: every row strictly ascending, no duplicate, no self loop, no id
    >= n_nodes; not symmetrised.  Normalised and validated ONCE on the host (an id outside the graph never reaches the kernel),
    uploaded once per device."""

    def __init__(self, rowptr, col, n_nodes):
        self.n_nodes = int(n_nodes)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.deg = np.diff(self.rowptr).astype(np.int64)
        self.max_degree = int(self.deg.max()) if self.deg.size else 0
        self._dev = {}
        self._weights = {}

    @classmethod
    def from_csr(cls, rowptr, col, n_nodes):
        """rowptr [n_nodes + 1], col with entries >= 0 (an entry >= n_nodes is a pad and is dropped); rows in any order."""
        n = int(n_nodes)
        tonp = lambda a: np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
        rp = tonp(rowptr).astype(np.int64)
        col = tonp(col).reshape(-1).astype(np.int64)
        if n < 0 or n >= 2 ** 31 - 1 or rp.ndim != 1 or rp.shape[0] != n + 1:
            raise GraphsageAmdError("SimpleGraph: rowptr must have n_nodes + 1 = %d entries" % (n + 1))
        if rp[0] != 0 or (np.diff(rp) < 0).any() or int(rp[-1]) != col.shape[0]:
            raise GraphsageAmdError("SimpleGraph: rowptr must run from 0 to len(col) without decreasing")
        if col.size and col.min() < 0:
            raise GraphsageAmdError("SimpleGraph: ids must not be negative (found %d)" % col.min())
        row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
        keep = (col < n) & (col != row)
        key = np.unique(row[keep] * max(n, 1) + col[keep])                      # sorts and de-duplicates
        new_rp = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(key // max(n, 1), minlength=n), out=new_rp[1:])
        return cls(new_rp, key % max(n, 1), n)

    def lists(self):
        return [self.col[self.rowptr[r]:self.rowptr[r + 1]] for r in range(self.n_nodes)]

    def rank_filter(self):
        """Every edge of this graph as a RankFilter (rows already are what a filter wants)."""
        from .inference import RankFilter
        return RankFilter(self.rowptr, self.col, self.n_nodes)

    def weights(self, kind):
        if kind not in self._weights:
            self._weights[kind] = neighbor_weights(kind, self.deg)
        return self._weights[kind]

    def two_hop_work(self, sources):
        """int64 [len(sources)]: sum of deg w over w in N(u), the row walks a source costs."""
        sources = np.asarray(sources, dtype=np.int64)
        lens = self.deg[sources]
        starts = self.rowptr[sources]
        if not lens.sum():
            return np.zeros(sources.shape[0], np.int64)
        seg = np.repeat(np.arange(sources.shape[0]), lens)
        idx = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens) + np.repeat(starts, lens)
        return np.bincount(seg, weights=self.deg[self.col[idx]].astype(np.float64), minlength=sources.shape[0]).astype(np.int64)

    def on(self, device):
        """(rowptr int64 [N + 1], col int32, deg int32 [N]) on `device`."""
        key = str(device)
        if key not in self._dev:
            import torch
            col = torch.from_numpy(self.col).to(device) if self.col.size else torch.zeros(1, dtype=torch.int32, device=device)
            self._dev[key] = (torch.from_numpy(self.rowptr).to(device), col,
                              torch.from_numpy(self.deg.astype(np.int32)).to(device))
            torch.cuda.synchronize()
        return self._dev[key]

    def weights_on(self, kind, device):
        """The uint32 weights of `kind` on `device` (their bits in an int32 tensor), or None where every weight is 1."""
        if kind in ("cn", "jaccard"):
            return None
        key = (str(device), kind)
        if key not in self._dev:
            import torch
            self._dev[key] = torch.from_numpy(self.weights(kind)[0].view(np.int32)).to(device)
            torch.cuda.synchronize()
        return self._dev[key]


def group_by_source(src, dst, work=None):
    """(order, group_ptr int64 [G + 1], group_src int32 [G], dst int32 in group order): a stable argsort of src, so that a
    source's partners keep the caller's order; result k of the kernel belongs to the caller's edge order[k].  work (per node,
    optional): the groups are handed out heaviest first (stable among equals), which changes no result."""
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    dst = np.asarray(dst, dtype=np.int64).reshape(-1)
    order = np.argsort(src, kind="stable")
    s = src[order]
    first = np.ones(s.shape[0], dtype=bool)
    first[1:] = s[1:] != s[:-1]
    starts = np.flatnonzero(first)
    sizes = np.diff(np.append(starts, s.shape[0]))
    group_src = s[starts]
    if work is not None and group_src.size:
        by = np.argsort(-np.asarray(work, dtype=np.int64)[group_src], kind="stable")
        lens = sizes[by]
        idx = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens) + np.repeat(starts[by], lens)
        order, group_src, sizes = order[idx], group_src[by], lens
    group_ptr = np.zeros(group_src.shape[0] + 1, np.int64)
    np.cumsum(sizes, out=group_ptr[1:])
    return order, group_ptr, group_src.astype(np.int32), dst[order].astype(np.int32)


def scores_float(graph, kind, edges, t, S):
    """fp64 on the host: t / 2^S, or the Jaccard ratio t / (deg u + deg x - t) (0 where t = 0, inf over a zero denominator)."""
    t = np.asarray(t, dtype=np.float64)
    if kind != "jaccard":
        return t / 2.0 ** S
    den = (graph.deg[edges[:, 0]] + graph.deg[edges[:, 1]]).astype(np.float64) - t
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t > 0, t / den, 0.0)


def rank_neighbors(engine, graph, edges, kind="aa", filt=None, hits=(1, 10, 50, 100), tile=0, max_workgroups=0):
    """Rank the true partner of every edge (src, dst) among ALL nodes of `graph` (SimpleGraph) by the neighbor-overlap score
    `kind`; dst itself, src and the filter row of src (filt: RankFilter, optional) are no candidates.  Returns the dictionary of
    inference.rank_metrics plus scores (uint32 numerators t), scores_float, zero (share of edges with t = 0), scale_bits, sources
    (distinct ones) and paths (sum over them of sum_{w in N(u)} deg w).  tile / max_workgroups: the kernel's LDS tile and grid
    cap (0: its defaults); no result depends on them."""
    import torch
    from .inference import rank_metrics
    if not isinstance(graph, SimpleGraph):
        raise GraphsageAmdError("rank_neighbors needs a SimpleGraph (SimpleGraph.from_csr)")
    if kind not in KINDS:
        raise GraphsageAmdError("rank_neighbors: kind must be one of %s" % ", ".join(KINDS))
    N = graph.n_nodes
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    Q = edges.shape[0]
    if Q and (edges.min() < 0 or edges.max() >= N):
        raise GraphsageAmdError("rank_neighbors: edge ends must lie in [0, %d)" % N)
    if filt is not None and filt.n_nodes != N:
        raise GraphsageAmdError("rank_neighbors: the filter covers %d rows, the graph has %d" % (filt.n_nodes, N))
    if tile and (tile < ops.NBR_MIN_TILE or tile > ops.NBR_MAX_TILE or tile & (tile - 1)):
        raise GraphsageAmdError("rank_neighbors: tile = %d must be a power of two in [%d, %d]" % (tile, ops.NBR_MIN_TILE,
                                                                                                  ops.NBR_MAX_TILE))
    _, S = graph.weights(kind)
    if Q == 0:
        res = rank_metrics(np.zeros(0, np.int64), np.zeros(0, np.int64), hits)
        res.update({"scores": np.zeros(0, np.uint32), "scores_float": np.zeros(0), "zero": 0.0, "scale_bits": S, "sources": 0,
                    "paths": 0})
        return res
    sources = np.unique(edges[:, 0])
    work = np.zeros(N, np.int64)
    work[sources] = graph.two_hop_work(sources)
    order, group_ptr, group_src, dst = group_by_source(edges[:, 0], edges[:, 1], work)
    e = engine
    rowptr, col, deg = graph.on(e.device)
    q = graph.weights_on(kind, e.device)
    f_rowptr, f_col = filt.on(e.device, N) if filt is not None else (None, None)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(e.device)
    group_ptr, group_src, dst = up(group_ptr), up(group_src), up(dst)
    out = [torch.zeros(Q, dtype=torch.int32, device=e.device) for _ in range(3)]
    torch.cuda.synchronize()              # uploads and zero-fills ran on torch's stream; order them before the engine's
    ops.nbr_rank(rowptr, col, N, group_ptr, group_src, dst, q=q, deg=deg if kind == "jaccard" else None, f_rowptr=f_rowptr,
                 f_col=f_col, kind="jaccard" if kind == "jaccard" else "sum", tile=tile, max_workgroups=max_workgroups,
                 max_src_degree=int(graph.deg[sources].max()), t=out[0], n_gt=out[1], n_eq=out[2], stream=e.stream)
    e.sync()
    back = lambda a, dt: _scatter(a.cpu().numpy().view(dt), order)
    t, n_gt, n_eq = back(out[0], np.uint32), back(out[1], np.int32), back(out[2], np.int32)
    res = rank_metrics(n_gt, n_eq, hits)
    res.update({"scores": t, "scores_float": scores_float(graph, kind, edges, t, S), "zero": float(np.mean(t == 0)),
                "scale_bits": S, "sources": int(sources.shape[0]), "paths": int(work[sources].sum())})
    return res


def _scatter(values, order):
    out = np.empty_like(values)
    out[order] = values
    return out


def result_line(kind, res, seconds):
    """The line --rank_baselines prints and writes to rank_baseline_<kind>.txt."""
    return ("Link ranking baseline: kind= %s mrr= %.5f " % (kind, res["mrr"])
            + " ".join("hits@%d= %.5f" % (k, res["hits"][k]) for k in sorted(res["hits"]))
            + " edges= %d zero= %.5f sources= %d paths= %d scale_bits= %d time= %.5f" % (
                len(res["ranks"]), res["zero"], res["sources"], res["paths"], res["scale_bits"], seconds))
