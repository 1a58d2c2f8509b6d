"""fp64 NumPy oracle of the inverted-file retrieval (gs_ivf_search): the probe rule, the union of the probed lists, and
topk_oracle.select over the candidates inside that union."""
import numpy as np

from topk_oracle import select


def probe(Xq, centers, nprobe):
    """int [Q, nprobe]: the centres that come first by (<x_q, c_j> descending, j ascending)."""
    S = Xq.astype(np.float64) @ centers.astype(np.float64).T
    j = np.arange(S.shape[1])
    return np.stack([j[np.lexsort((j, -S[q]))][:nprobe] for q in range(S.shape[0])])


def union(P, labels, n_cand):
    """bool [Q, n_cand]: row w (labels[w] = its list) lies in one of the lists that query q probes."""
    labels = np.asarray(labels)[:n_cand]
    return np.stack([np.isin(labels, P[q]) for q in range(P.shape[0])])


def scanned(P, labels):
    """int64 [Q]: the members of the probed lists."""
    sizes = np.bincount(labels)
    return sizes[P].sum(axis=1).astype(np.int64)


def search(S, C, Xq, centers, labels, k, nprobe):
    """(ids, scores, count, scanned) of an IVF search: S fp64 scores [Q, n_cand], C the candidate mask of topk_oracle.candidates,
    centers / labels the index in its final numbering."""
    P = probe(Xq, centers, nprobe)
    return select(S, C & union(P, labels, S.shape[1]), k) + (scanned(P, labels),)
