"""NumPy restatement of the attention-pooling aggregator (graphsage_attn; DESIGN "Attention pooling") with a hand-written backward,
plugged into the oracle's aggregate / model functions (oracle/graphsage_oracle.py) for aggregator_type "attn"; and the same layer
over whole neighbor lists (the full-neighborhood pass of tests/fullnbr_oracle.py).  float64 or float32 by the inputs' dtype.

Parameters of one layer: self_weights [in, out], neigh_weights [hidden, out], (bias), mlp_weights [neigh_in, hidden], mlp_bias
[hidden], attn_a [hidden]; hidden = 512 ("small") or 1024 ("big").

    V_j = relu(x_j . W_mlp + b_mlp);  t_j = <V_j, a>;  alpha = softmax_j(t_j);  pooled = sum_j alpha_j V_j;  the SAGE matmuls.

Backward, dP = d_pooled:  g_j = <dP, V_j>;  G = sum_j alpha_j g_j;  dt_j = alpha_j (g_j - G);
                          dV_j = (alpha_j dP + dt_j a) * (V_j > 0);  da = sum dt_j V_j."""
import contextlib

import numpy as np

from oracle import graphsage_oracle as orc
import fullnbr_oracle as fo

MLP_KEYS = ("mlp_weights", "mlp_bias", "attn_a")


def softmax_rows(t):
    e = np.exp(t - t.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def segment_attn_fwd(V, a):
    """V [n, s, hidden], a [hidden] -> (pooled [n, hidden], alpha [n, s])."""
    alpha = softmax_rows(V @ a)
    return (alpha[:, :, None] * V).sum(axis=1), alpha


def segment_attn_bwd(dP, V, a, alpha):
    """-> (dV [n, s, hidden] through the relu mask V > 0, da [hidden], dt [n, s])."""
    g = np.einsum("nh,nsh->ns", dP, V)
    G = (alpha * g).sum(axis=1, keepdims=True)
    dt = alpha * (g - G)
    dV = (alpha[:, :, None] * dP[:, None, :] + dt[:, :, None] * a[None, None, :]) * (V > 0)
    return dV, np.einsum("ns,nsh->h", dt, V), dt


def attn_aggregator_fwd(self_vecs, neigh_vecs, p, concat, act):
    n, s, d = neigh_vecs.shape
    x = neigh_vecs.reshape(n * s, d)
    V = np.maximum(x @ p["mlp_weights"] + p["mlp_bias"], 0).reshape(n, s, -1)
    pooled, alpha = segment_attn_fwd(V, p["attn_a"])
    from_self = self_vecs @ p["self_weights"]
    from_neigh = pooled @ p["neigh_weights"]
    z = np.concatenate([from_self, from_neigh], axis=1) if concat else from_self + from_neigh
    if "bias" in p:
        z = z + p["bias"]
    y = orc._act(z, act)
    return y, (self_vecs, x, V, alpha, pooled, y)


def attn_aggregator_bwd(dy, cache, p, concat, act):
    self_vecs, x, V, alpha, pooled, y = cache
    n, s, hid = V.shape
    dz = orc._act_bwd(y, dy, act)
    o = p["self_weights"].shape[1]
    dzs, dzn = (dz[:, :o], dz[:, o:]) if concat else (dz, dz)
    g = {"self_weights": self_vecs.T @ dzs, "neigh_weights": pooled.T @ dzn}
    if "bias" in p:
        g["bias"] = dz.sum(axis=0)
    d_self = dzs @ p["self_weights"].T
    dV, g["attn_a"], _ = segment_attn_bwd(dzn @ p["neigh_weights"].T, V, p["attn_a"], alpha)
    dV = dV.reshape(n * s, hid)
    g["mlp_weights"] = x.T @ dV
    g["mlp_bias"] = dV.sum(axis=0)
    d_neigh = (dV @ p["mlp_weights"].T).reshape(n, s, -1)
    return d_self, d_neigh, g


@contextlib.contextmanager
def installed():
    """The oracle's per-aggregator dispatch (orc._agg_fwd / orc._agg_bwd) with "attn" added, for the duration of a block."""
    fwd, bwd = orc._agg_fwd, orc._agg_bwd

    def agg_fwd(aggregator_type, p, self_vecs, neigh_vecs, concat, act):
        if aggregator_type == "attn":
            return attn_aggregator_fwd(self_vecs, neigh_vecs, p, concat, act)
        return fwd(aggregator_type, p, self_vecs, neigh_vecs, concat, act)

    def agg_bwd(aggregator_type, p, dy, cache, concat, act):
        if aggregator_type == "attn":
            return attn_aggregator_bwd(dy, cache, p, concat, act)
        return bwd(aggregator_type, p, dy, cache, concat, act)
    orc._agg_fwd, orc._agg_bwd = agg_fwd, agg_bwd
    try:
        yield
    finally:
        orc._agg_fwd, orc._agg_bwd = fwd, bwd


def make_params(dims, concat, rng, hidden=512, dtype=np.float64, bias=False):
    """One parameter dict per layer (orc.make_aggregator_params for "attn"); small non-zero biases and a spread gate."""
    params = []
    for layer in range(len(dims) - 1):
        din, dout = (2 if (concat and layer) else 1) * dims[layer], dims[layer + 1]
        p = {"mlp_weights": orc.glorot((din, hidden), rng, dtype), "mlp_bias": (0.1 * rng.randn(hidden)).astype(dtype),
             "attn_a": rng.randn(hidden).astype(dtype) / np.sqrt(hidden).astype(dtype),
             "neigh_weights": orc.glorot((hidden, dout), rng, dtype), "self_weights": orc.glorot((din, dout), rng, dtype)}
        if bias:
            p["bias"] = (0.1 * rng.randn((2 if concat else 1) * dout)).astype(dtype)
        params.append(p)
    return params


# ------------------------------------------------------------------------------------------------ full neighborhoods
def softmax_reduce_rows(lists, X, t):
    """out[r] = sum_e softmax_e(t[col[e]]) X[col[e]] over the whole list of every row (a duplicate entry counts as often as it
    occurs); an empty list gives 0: the contract of GS_CSR_SOFTMAX."""
    out = np.zeros((len(lists), X.shape[1]), X.dtype)
    for r, nb in enumerate(lists):
        nb = np.asarray(nb, dtype=np.int64)
        if nb.size:
            out[r] = softmax_rows(t[nb]) @ X[nb]
    return out


def full_layer(lists, H, p, concat, last):
    V = np.maximum(H @ p["mlp_weights"] + p["mlp_bias"], 0)
    neigh = softmax_reduce_rows(lists, V, V @ p["attn_a"])
    from_neigh, from_self = neigh @ p["neigh_weights"], H @ p["self_weights"]
    z = np.concatenate([from_self, from_neigh], axis=1) if concat else from_self + from_neigh
    if "bias" in p:
        z = z + p["bias"]
    return z if last else np.maximum(z, 0)


def full_forward(lists, feats, params, concat):
    """l2-normalised embeddings of every row from its WHOLE neighbor list (fullnbr_oracle.forward for "attn")."""
    H = np.asarray(feats)
    K = len(params["agg"])
    for i, p in enumerate(params["agg"]):
        H = full_layer(lists, H, p, concat, last=(i == K - 1))
    return fo.l2_normalize(H)
