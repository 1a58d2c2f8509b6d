"""NumPy restatement of exact inference for a node SUBSET (TEST INFRASTRUCTURE): the receptive field of a request over the
neighbor lists of FullGraph.lists(), and fullnbr_oracle.forward restricted to it -- layer l computed for the rows of S_l only,
from a compact table over S_{l-1}.  The arithmetic follows the array dtype (the tests run it in float64).

    S_K = the distinct requested ids, sorted;   S_{l-1} = S_l U N(S_l)

`params["agg"][i]` is fullnbr_oracle's per-layer dict; two additions: "bias" (added before the activation) and "mlp", a list of
(weights, bias) pairs for an aggregator with more than one Dense in front of its max (twomaxpool).
"""
import numpy as np

import fullnbr_oracle as fo


def closure(lists, rows):
    """The ascending, duplicate-free list of rows U {lists[r][k] : r in rows}."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    parts = [rows] + [np.asarray(lists[r], dtype=np.int64) for r in rows]
    return np.unique(np.concatenate(parts)) if parts else rows


def position_map(n_rows, S):
    """pos[id] = index of id in S, -1 for every non-member."""
    pos = np.full(n_rows, -1, np.int64)
    pos[np.asarray(S, dtype=np.int64)] = np.arange(len(S))
    return pos


def receptive_field(lists, nodes, K):
    """[S_K, ..., S_0] as ascending int64 arrays, and the edges visited per layer [edges of S_K, ..., edges of S_1]."""
    S = np.unique(np.asarray(nodes, dtype=np.int64).reshape(-1))
    sets, edges = [S], []
    for _ in range(K):
        edges.append(int(sum(len(lists[r]) for r in S)))
        S = closure(lists, S)
        sets.append(S)
    return sets, edges


def layer(sub_lists, H_prev, self_idx, p, agg, concat, last):
    """One aggregator layer for the rows whose neighbor lists (as indices into H_prev) are sub_lists and whose own rows are
    H_prev[self_idx] (fullnbr_oracle.layer on a compact table, + bias, + twomaxpool)."""
    act = (lambda x: x) if last else (lambda x: np.maximum(x, 0))
    bias = p.get("bias", 0)
    self_idx = np.asarray(self_idx, dtype=np.int64)

    def reduce(X, op):
        out = np.zeros((len(sub_lists), X.shape[1]), X.dtype)
        for i, nb in enumerate(sub_lists):
            rows = X[np.asarray(nb, dtype=np.int64)]
            if op == "mean_self":
                out[i] = (rows.sum(axis=0) + X[self_idx[i]]) / X.dtype.type(len(nb) + 1)
            elif len(nb):
                out[i] = rows.sum(axis=0) / X.dtype.type(len(nb)) if op == "mean" else rows.max(axis=0)
        return out

    if agg == "gcn":
        return act(reduce(H_prev, "mean_self") @ p["weights"] + bias)
    if agg == "mean":
        neigh = reduce(H_prev, "mean")
    else:
        hidden = H_prev
        for W, b in (p.get("mlp") or [(p["mlp_weights"], p["mlp_bias"])]):
            hidden = np.maximum(hidden @ W + b, 0)
        neigh = reduce(hidden, "mean" if agg == "meanpool" else "max")
    from_neigh, from_self = neigh @ p["neigh_weights"], H_prev[self_idx] @ p["self_weights"]
    return act((np.concatenate([from_self, from_neigh], axis=1) if concat else from_self + from_neigh) + bias)


def forward(lists, feats, params, agg, concat, nodes):
    """(l2-normalised embeddings of `nodes` in REQUEST order, [S_K, ..., S_0], edges per layer): layer l for S_l only."""
    feats = np.asarray(feats)
    K = len(params["agg"])
    sets, edges = receptive_field(lists, nodes, K)
    H = feats[sets[K]]                                    # compact over S_0
    for l, p in enumerate(params["agg"]):
        S, S_prev = sets[K - 1 - l], sets[K - l]
        pos = position_map(len(lists), S_prev)
        sub = [pos[np.asarray(lists[r], dtype=np.int64)] for r in S]
        assert all((s >= 0).all() for s in sub) and (pos[S] >= 0).all()
        H = layer(sub, H, pos[S], p, agg, concat, last=(l == K - 1))
    emb = fo.l2_normalize(H)
    return emb[np.searchsorted(sets[0], np.asarray(nodes, dtype=np.int64).reshape(-1))], sets, edges
