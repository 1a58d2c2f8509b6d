"""NumPy restatement of the exact layer-wise, full-neighborhood forward pass (TEST INFRASTRUCTURE): every layer for every row
of a multigraph from the row's WHOLE neighbor list, the pad row N computed like any other row (its features are zero, its
neighbors are pad ids; once the pooling MLP's bias is non-zero its hidden state is not zero).

`lists[v]` is row v's neighbor list, v = 0 .. N (duplicates count as often as they occur).  Parameters come in the layout of
ref_fixtures.Fixture.params.  The arithmetic follows the array dtype (float64 twin: 1e-9 pins; float32: the device's class).

When num_samples == max_degree at every layer the reference's sampler returns a permutation of each row of its padded table
and mean / max are symmetric, so `forward(padded_lists(adj), ...)` IS the reference's forward pass at the batch nodes.
"""
import numpy as np


def padded_lists(adj):
    """Row v of the reference's padded table verbatim, the pad row included (FullGraph.from_padded)."""
    return [np.asarray(r) for r in np.asarray(adj)]


def csr_lists(rowptr, col, n_nodes):
    """The true graph with the reference's pad rule: a node without neighbors, and the pad node, have the one neighbor N
    (FullGraph.from_csr)."""
    out = []
    for v in range(n_nodes):
        nb = np.asarray(col[rowptr[v]:rowptr[v + 1]])
        out.append(nb if nb.size else np.asarray([n_nodes]))
    out.append(np.asarray([n_nodes]))
    return out


def reduce_rows(lists, X, op):
    """mean | mean_self | max of X's rows over each list (the kernel's contract: empty list -> 0, X[r] for mean_self)."""
    out = np.zeros((len(lists), X.shape[1]), X.dtype)
    for r, nb in enumerate(lists):
        rows = X[np.asarray(nb, dtype=np.int64)]
        if op == "mean_self":
            out[r] = (rows.sum(axis=0) + X[r]) / X.dtype.type(len(nb) + 1)
        elif len(nb) == 0:
            continue
        elif op == "mean":
            out[r] = rows.sum(axis=0) / X.dtype.type(len(nb))
        else:
            out[r] = rows.max(axis=0)
    return out


def layer(lists, H, p, agg, concat, last):
    """One aggregator layer for all rows (aggregators.py: Mean :46-64, GCN :96-116, MaxPool :176-195, MeanPool :254-273)."""
    act = (lambda x: x) if last else (lambda x: np.maximum(x, 0))
    if agg == "gcn":
        return act(reduce_rows(lists, H, "mean_self") @ p["weights"])
    if agg == "mean":
        neigh = reduce_rows(lists, H, "mean")
    else:
        hidden = np.maximum(H @ p["mlp_weights"] + p["mlp_bias"], 0)
        neigh = reduce_rows(lists, hidden, "max" if agg == "maxpool" else "mean")
    from_neigh, from_self = neigh @ p["neigh_weights"], H @ p["self_weights"]
    return act(np.concatenate([from_self, from_neigh], axis=1) if concat else from_self + from_neigh)


def l2_normalize(x):
    return x / np.sqrt(np.maximum((x * x).sum(axis=1, keepdims=True), 1e-12))


def forward(lists, feats, params, agg, concat):
    """l2-normalised embeddings of every row (models.py:321-330, :368-370)."""
    H = np.asarray(feats)
    K = len(params["agg"])
    for i, p in enumerate(params["agg"]):
        H = layer(lists, H, p, agg, concat, last=(i == K - 1))
    return l2_normalize(H)


def predict(emb, params, sigmoid):
    """(node_preds, preds) of supervised_models.py:86-93, :122-126."""
    z = emb @ params["node_pred"]["weights"] + params["node_pred"]["bias"]
    if sigmoid:
        return z, 1.0 / (1.0 + np.exp(-z))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return z, e / e.sum(axis=1, keepdims=True)
