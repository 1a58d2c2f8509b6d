"""NumPy restatement of the two-layer max-pooling aggregator (graphsage/aggregators.py:276-361) with a hand-written backward,
plugged into the oracle's aggregate / model functions (oracle/graphsage_oracle.py) for aggregator_type "twomaxpool"; and the
same layer over whole neighbor lists (the full-neighborhood pass of tests/fullnbr_oracle.py).  float64 or float32 by the
inputs' dtype.

Parameters of one layer: self_weights [in, out], neigh_weights [hid2, out], (bias), mlp_weights [neigh_in, hid1], mlp_bias
[hid1], mlp2_weights [hid1, hid2], mlp2_bias [hid2]; hid1 / hid2 = 512 / 256 ("small") or 1024 / 512 ("big").

    h1 = relu(x . W1 + b1);  h2 = relu(h1 . W2 + b2)  per neighbor row;  pooled = max over the s rows;  then the SAGE matmuls.

Backward: d_pooled lands on the arg-max row of each (group, column) (the first on ties, as the device; DESIGN "MaxPool ties"),
through the second relu, W2, the first relu, W1.

`trace` (inside `tracing()`): one (h2 [n, s, hid2], argmax [n, hid2]) per aggregator call in call order -- layer 0's hops, then
layer 1's ..; `tie_margins` turns one into the lead of every positive maximum over the best row of a DIFFERENT node id."""
import contextlib
import json
import os

import numpy as np

from oracle import graphsage_oracle as orc
import fullnbr_oracle as fo
import ref_fixtures

MLP_KEYS = ("mlp_weights", "mlp_bias", "mlp2_weights", "mlp2_bias")
trace = None


def twomax_aggregator_fwd(self_vecs, neigh_vecs, p, concat, act):
    n, s, d = neigh_vecs.shape
    x = neigh_vecs.reshape(n * s, d)
    h1 = np.maximum(x @ p["mlp_weights"] + p["mlp_bias"], 0)
    h2 = np.maximum(h1 @ p["mlp2_weights"] + p["mlp2_bias"], 0).reshape(n, s, -1)
    arg = h2.argmax(axis=1)
    pooled = np.take_along_axis(h2, arg[:, None, :], axis=1)[:, 0, :]
    if trace is not None:
        trace.append((h2, arg))
    from_self = self_vecs @ p["self_weights"]
    from_neigh = pooled @ p["neigh_weights"]
    z = np.concatenate([from_self, from_neigh], axis=1) if concat else from_self + from_neigh
    if "bias" in p:
        z = z + p["bias"]
    y = orc._act(z, act)
    return y, (self_vecs, x, h1, h2, arg, pooled, y)


def twomax_aggregator_bwd(dy, cache, p, concat, act):
    self_vecs, x, h1, h2, arg, pooled, y = cache
    n, s, hid2 = h2.shape
    dz = orc._act_bwd(y, dy, act)
    o = p["self_weights"].shape[1]
    dzs, dzn = (dz[:, :o], dz[:, o:]) if concat else (dz, dz)
    g = {"self_weights": self_vecs.T @ dzs, "neigh_weights": pooled.T @ dzn}
    if "bias" in p:
        g["bias"] = dz.sum(axis=0)
    d_self = dzs @ p["self_weights"].T
    dpm = (dzn @ p["neigh_weights"].T) * (pooled > 0)            # reduce_max grad, then the second relu's
    dh2 = np.zeros_like(h2)
    np.put_along_axis(dh2, arg[:, None, :], dpm[:, None, :], axis=1)
    dh2 = dh2.reshape(n * s, hid2)
    g["mlp2_weights"] = h1.T @ dh2
    g["mlp2_bias"] = dh2.sum(axis=0)
    dh1 = (dh2 @ p["mlp2_weights"].T) * (h1 > 0)
    g["mlp_weights"] = x.T @ dh1
    g["mlp_bias"] = dh1.sum(axis=0)
    d_neigh = (dh1 @ p["mlp_weights"].T).reshape(n, s, -1)
    return d_self, d_neigh, g


@contextlib.contextmanager
def installed():
    """The oracle's per-aggregator dispatch (orc._agg_fwd / orc._agg_bwd) with "twomaxpool" added, for the duration of a block."""
    fwd, bwd = orc._agg_fwd, orc._agg_bwd

    def agg_fwd(aggregator_type, p, self_vecs, neigh_vecs, concat, act):
        if aggregator_type == "twomaxpool":
            return twomax_aggregator_fwd(self_vecs, neigh_vecs, p, concat, act)
        return fwd(aggregator_type, p, self_vecs, neigh_vecs, concat, act)

    def agg_bwd(aggregator_type, p, dy, cache, concat, act):
        if aggregator_type == "twomaxpool":
            return twomax_aggregator_bwd(dy, cache, p, concat, act)
        return bwd(aggregator_type, p, dy, cache, concat, act)
    orc._agg_fwd, orc._agg_bwd = agg_fwd, agg_bwd
    try:
        yield
    finally:
        orc._agg_fwd, orc._agg_bwd = fwd, bwd


@contextlib.contextmanager
def tracing():
    global trace
    trace = []
    try:
        yield trace
    finally:
        trace = None


def tie_margins(h2, arg, ids):
    """For every (group, column) with a positive maximum: maximum - best activation among the rows of a DIFFERENT node id
    (ids [n, s]: the node each neighbor row belongs to); +inf where the group holds no other id."""
    n, s, hid2 = h2.shape
    mx = np.take_along_axis(h2, arg[:, None, :], axis=1)[:, 0, :]
    win_id = np.take_along_axis(ids, arg, axis=1)                                    # [n, hid2]
    other = ids[:, :, None] != win_id[:, None, :]                                   # [n, s, hid2]
    best_other = np.where(other, h2, -np.inf).max(axis=1)
    return (mx - best_other)[mx > 0]


class _Parts(object):
    """The arrays of ref_<name>.npz, ref_<name>_p1.npz ... as one archive (`files`, `[key]`); `key@@0`, `key@@1` ... are the
    row blocks of one array (tests/golden/make_ref_twomax_fixtures.save_parts)."""

    def __init__(self, name):
        first = np.load(os.path.join(ref_fixtures.GOLDEN, "ref_%s.npz" % name))
        zs = [first] + [np.load(os.path.join(ref_fixtures.GOLDEN, "ref_%s_p%d.npz" % (name, i)))
                        for i in range(1, int(first["n_parts"]))]
        self._where, self._blocks = {}, {}
        for z in zs:
            for k in z.files:
                if "@@" in k:
                    key, j = k.split("@@")
                    self._blocks.setdefault(key, {})[int(j)] = (z, k)
                else:
                    self._where[k] = z
        self.files = sorted(list(self._where) + list(self._blocks))

    def __getitem__(self, k):
        if k in self._blocks:
            b = self._blocks[k]
            return np.concatenate([b[j][0][b[j][1]] for j in range(len(b))], axis=0)
        return self._where[k][k]


class Fixture(ref_fixtures.Fixture):
    """ref_fixtures.Fixture over a fixture written in parts."""

    def __init__(self, name):
        self.name, self.z = name, _Parts(name)
        c = self.cfg = json.loads(str(self.z["cfg"]))
        self.K, self.agg, self.out_dim, self.identity_dim = len(c["num_samples"]), c["aggregator_type"], c["dim"], 0
        self.dims = [self.z["graph/feats"].shape[1]] + [self.out_dim] * self.K
        self.n_steps = int(self.z["n_steps"])
        self.n_nodes = self.z["graph/feats"].shape[0] - 1


def fixture_params(fx, prefix, dtype, supervised=True):
    """Fixture.params plus each layer's second Dense (mlp2_weights / mlp2_bias) and the MLP arrays it does not know; arrays
    the fixture holds only as sketches are left out."""
    params = fx.params(prefix, dtype, supervised)
    for i, p in enumerate(params["agg"]):
        for k in MLP_KEYS + ("bias",):
            key = "%sagg%d/%s" % (prefix, i, k)
            if key in fx.z.files:
                p[k] = fx[key].astype(dtype)
    return params


# ------------------------------------------------------------------------------------------------ full neighborhoods
def full_layer(lists, H, p, concat, last):
    h1 = np.maximum(H @ p["mlp_weights"] + p["mlp_bias"], 0)
    h2 = np.maximum(h1 @ p["mlp2_weights"] + p["mlp2_bias"], 0)
    neigh = fo.reduce_rows(lists, h2, "max")
    from_neigh, from_self = neigh @ p["neigh_weights"], H @ p["self_weights"]
    z = np.concatenate([from_self, from_neigh], axis=1) if concat else from_self + from_neigh
    return z if last else np.maximum(z, 0)


def full_forward(lists, feats, params, concat):
    """l2-normalised embeddings of every row from its WHOLE neighbor list (fullnbr_oracle.forward for "twomaxpool")."""
    H = np.asarray(feats)
    K = len(params["agg"])
    for i, p in enumerate(params["agg"]):
        H = full_layer(lists, H, p, concat, last=(i == K - 1))
    return fo.l2_normalize(H)
