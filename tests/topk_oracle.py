"""fp64 NumPy oracle of the full-graph top-k retrieval (gs_topk_select): candidate mask, order rule, padding."""
import numpy as np


def candidates(Q, n_cand, src=None, flists=None, keep_src=False):
    """bool [Q, n_cand]: w is a candidate of q (keep_src: src only names the filter row).  There is no dst."""
    C = np.ones((Q, n_cand), dtype=bool)
    if src is not None:
        for q in range(Q):
            if src[q] < n_cand and not keep_src:
                C[q, src[q]] = False
            if flists is not None:
                f = np.asarray(flists[src[q]], dtype=np.int64)
                C[q, f[f < n_cand]] = False
    return C


def select(S, C, k):
    """The first k candidates of every row of S in the total order (score descending, id ascending):
    (ids int32 [Q, k], scores float64 [Q, k], count int32 [Q]); entries at and beyond count are -1 / -inf."""
    Q = S.shape[0]
    ids = np.full((Q, k), -1, np.int32)
    scores = np.full((Q, k), -np.inf, np.float64)
    count = np.zeros(Q, np.int32)
    for q in range(Q):
        w = np.flatnonzero(C[q])
        w = w[np.lexsort((w, -S[q, w]))][:k]
        count[q] = w.size
        ids[q, :w.size] = w
        scores[q, :w.size] = S[q, w]
    return ids, scores, count


def scores64(Xq, Zc, n_cand):
    return Xq.astype(np.float64) @ Zc[:n_cand].astype(np.float64).T
