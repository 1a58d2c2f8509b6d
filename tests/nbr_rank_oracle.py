"""The neighbor-overlap link-ranking baselines restated in NumPy int64 / Python integers (no import from the package).

    lists = simple_lists(rowptr, col, n)                  # sorted, no duplicate, no loop, no id >= n; not symmetrised
    t, n_gt, n_eq = rank(lists, n, edges, kind, flists)   # per edge, in the caller's order

s(u, x) = sum of q[w] over the w in N(u) with x in N(w), built per distinct source with np.add.at over the two-hop lists: nothing
is ever N x N.  The candidates of an edge (u, dst) are all x in [0, n) but dst, u and the filter row of u
(test_rank_full_gpu.candidates, one row at a time)."""
import math

import numpy as np

KINDS = ("cn", "aa", "ra", "jaccard")


def simple_lists(rowptr, col, n):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    return [np.array(sorted({int(x) for x in col[rowptr[r]:rowptr[r + 1]] if x < n and x != r}), dtype=np.int64) for r in range(n)]


def scale_bits(max_degree):
    return min(16, 31 - int(max_degree).bit_length())


def weight(kind, k, S):
    """q(k) in Python floats (fp64), one degree at a time."""
    if kind in ("cn", "jaccard"):
        return 1
    if kind == "aa":
        return max(1, int(math.floor(2.0 ** S / math.log(k) + 0.5))) if k >= 2 else 0
    return max(1, int(math.floor(2.0 ** S / k + 0.5))) if k >= 1 else 0


def weights(kind, lists):
    deg = [len(r) for r in lists]
    S = 0 if kind in ("cn", "jaccard") else scale_bits(max(deg) if deg else 0)
    return np.array([weight(kind, k, S) for k in deg], dtype=np.int64), S


def score_row(lists, q, u, n):
    """s(u, .) as int64 [n]."""
    s = np.zeros(n, dtype=np.int64)
    for w in lists[u]:
        np.add.at(s, lists[w], q[w])
    return s


def candidate_row(n, u, dst, flist=None):
    c = np.ones(n, dtype=bool)
    c[dst] = False
    c[u] = False
    if flist is not None:
        f = np.asarray(flist, dtype=np.int64)
        c[f[f < n]] = False
    return c


def rank(lists, n, edges, kind, flists=None):
    """(t, n_gt, n_eq) int64 per edge.  jaccard: t is the numerator cn; ratios compare as Python integers, cross-multiplied."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    q, _ = weights(kind, lists)
    deg = np.array([len(r) for r in lists], dtype=np.int64)
    t, n_gt, n_eq = (np.zeros(len(edges), np.int64) for _ in range(3))
    rows = {}
    for k, (u, x) in enumerate(edges):
        u, x = int(u), int(x)
        if u not in rows:
            rows[u] = score_row(lists, q, u, n)
        s = rows[u]
        c = candidate_row(n, u, x, None if flists is None else flists[u])
        t[k] = s[x]
        if kind == "jaccard":
            # s[y] / den[y] against s[x] / den[x] as s[y] * den[x] against s[x] * den[y], in Python integers where s[y] > 0; a
            # candidate with s[y] = 0 has the product 0 on its side: level where s[x] * den[y] is 0 too, below otherwise
            den = deg[u] + deg - s
            gt, eq = np.zeros(n, dtype=bool), (s == 0) & ((s[x] == 0) | (den == 0))
            for y in np.flatnonzero(s):
                a, b = int(s[y]) * int(den[x]), int(s[x]) * int(den[y])
                gt[y], eq[y] = a > b, a == b
        else:
            gt, eq = s > s[x], s == s[x]
        n_gt[k], n_eq[k] = (gt & c).sum(), (eq & c).sum()
    return t, n_gt, n_eq


def metrics(n_gt, n_eq, hits=(1, 10, 50, 100)):
    ranks = 1 + n_gt + n_eq
    return float(np.mean(1.0 / ranks)), {k: float(np.mean(ranks <= k)) for k in hits}


def brute(lists, n, u, x, kind):
    """s(u, x) on a SYMMETRIC graph by set intersection: the common neighbors of u and x, weighed by their degrees."""
    q, _ = weights(kind, lists)
    return sum(int(q[w]) for w in set(lists[u].tolist()) & set(lists[x].tolist()))
