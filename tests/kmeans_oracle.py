"""NumPy fp64 restatement of graphsage_amd.clustering and csrc/gs_kmeans.hip, with the same rules: assignment by the score
<x, c> - |c|^2 / 2 with an exact tie going to the lowest id, the stable grouping, the mean update in which an empty cluster
keeps its centre, the three stop rules, the seeding stream and the partition scores.  Nothing here imports the package."""
import numpy as np


def scores(X, C):
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    return X.dot(C.T) - 0.5 * (C * C).sum(axis=1)[None, :]


def assign(X, C):
    """(labels int32 [n] -- np.argmax returns the FIRST maximum: the lowest id of a tie --, dist fp64 [n], inertia)."""
    X = np.asarray(X, dtype=np.float64)
    S = scores(X, C)
    labels = np.argmax(S, axis=1).astype(np.int32)
    dist = np.maximum(0.0, (X * X).sum(axis=1) - 2.0 * S[np.arange(len(X)), labels])
    return labels, dist, float(dist.sum())


def margins(X, C):
    """fp64 (best, second-best id, best - second score) per row; k == 1: the margin is +inf."""
    S = scores(X, C)
    order = np.argsort(-S, axis=1, kind="stable")
    best = order[:, 0]
    if S.shape[1] == 1:
        return best, best, np.full(len(S), np.inf)
    second = order[:, 1]
    r = np.arange(len(S))
    return best, second, S[r, best] - S[r, second]


def members(labels, k, rows=None):
    """(rowptr int64 [k + 1], members int32 [n]): cluster j's run holds rows[i] (i) of its members in ascending i."""
    labels = np.asarray(labels)
    order = np.argsort(labels, kind="stable")
    rowptr = np.zeros(k + 1, dtype=np.int64)
    np.cumsum(np.bincount(labels, minlength=k), out=rowptr[1:])
    src = np.arange(len(labels)) if rows is None else np.asarray(rows)
    return rowptr, src[order].astype(np.int32)


def update(X, labels, C):
    """The fp64 means of the clusters; an empty cluster keeps its row of C."""
    X = np.asarray(X, dtype=np.float64)
    out = np.array(C, dtype=np.float64)
    for j in range(out.shape[0]):
        m = labels == j
        if m.any():
            out[j] = X[m].mean(axis=0)
    return out


def fit(X, init, max_iter=100, tol=1e-4):
    """The loop of clustering.fit_kmeans from an explicit init: (centres, labels, inertia, iters, stop, labels per iteration)."""
    C = np.array(init, dtype=np.float64)
    prev = np.full(len(X), -1, dtype=np.int32)
    inertia_prev, stop, iters, history = None, None, 0, []
    while stop is None:
        labels, _, inertia = assign(X, C)
        iters += 1
        history.append(labels)
        changed = int((labels != prev).sum())
        if changed == 0:
            stop = "converged"
        elif inertia_prev is not None and inertia_prev - inertia <= tol * inertia_prev:
            stop = "tol"
        elif iters >= max_iter:
            stop = "max_iter"
        else:
            C = update(X, labels, C)
            prev, inertia_prev = labels, inertia
    return C, labels, inertia, iters, stop, history


def seed_subsample(n, k, rs):
    m = min(n, max(4096, 32 * k))
    if m == n:
        return np.arange(n, dtype=np.int64)
    return np.sort(rs.choice(n, size=m, replace=False)).astype(np.int64)


def kmeanspp(P, k, rs):
    """k-means++ on the rows of P in fp64: the positions drawn, or ValueError with fewer than k distinct rows."""
    P = np.asarray(P, dtype=np.float64)
    m = len(P)
    chosen = [int(rs.randint(m))]
    d2 = ((P - P[chosen[0]]) ** 2).sum(axis=1)
    while len(chosen) < k:
        cum = np.cumsum(d2)
        if not cum[-1] > 0.0:
            raise ValueError("fewer than k distinct rows")
        j = min(int(np.searchsorted(cum, rs.random_sample() * cum[-1], side="right")), m - 1)
        while d2[j] == 0.0:
            j -= 1
        chosen.append(j)
        d2 = np.minimum(d2, ((P - P[j]) ** 2).sum(axis=1))
    return np.asarray(chosen, dtype=np.int64)


def seeds(X, k, seed):
    """Positions (among the rows of X) of the k seeds of fit_kmeans(init='kmeans++', seed=seed)."""
    rs = np.random.RandomState(seed)
    sub = seed_subsample(len(X), k, rs)
    return sub[kmeanspp(np.asarray(X)[sub], k, rs)]


def contingency(pred, true):
    tv, pv = np.unique(true), np.unique(pred)
    return np.array([[int(((true == t) & (pred == p)).sum()) for p in pv] for t in tv], dtype=np.int64)


def metrics(pred, true):
    """{'nmi' (arithmetic mean), 'ari', 'purity'} by their definitions, with loops over the table."""
    pred, true = np.asarray(pred), np.asarray(true)
    tab = contingency(pred, true)
    n = float(tab.sum())
    a, b = tab.sum(axis=1), tab.sum(axis=0)
    if len(a) == 1 or len(b) == 1:
        nmi = 1.0 if len(a) == len(b) == 1 else 0.0
    else:
        mi = 0.0
        for i in range(tab.shape[0]):
            for j in range(tab.shape[1]):
                if tab[i, j]:
                    mi += tab[i, j] / n * np.log(n * tab[i, j] / (float(a[i]) * float(b[j])))
        hu = -sum(x / n * np.log(x / n) for x in a)
        hv = -sum(x / n * np.log(x / n) for x in b)
        nmi = max(mi, 0.0) / ((hu + hv) / 2.0)
    c2 = lambda x: x * (x - 1) / 2.0
    sij = sum(c2(float(x)) for x in tab.ravel())
    sa, sb = sum(c2(float(x)) for x in a), sum(c2(float(x)) for x in b)
    exp = sa * sb / c2(n) if n > 1 else 0.0
    den = (sa + sb) / 2.0 - exp
    ari = 1.0 if den == 0.0 else (sij - exp) / den
    purity = sum(float(tab[:, j].max()) for j in range(tab.shape[1])) / n
    return {"nmi": float(nmi), "ari": float(ari), "purity": float(purity)}
