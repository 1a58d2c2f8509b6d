"""NumPy restatement of the LSTM aggregator (graphsage/aggregators.py:363-449 on TF 1.x BasicLSTMCell + dynamic_rnn) with a
hand-written BPTT, plugged into the oracle's aggregate / model functions (oracle/graphsage_oracle.py) for aggregator_type
"seq".  Independent of the TF1 stand-in (tests/tf1_rnn.py restates the same cell with torch autograd).

Parameters of one layer: self_weights [in, out], neigh_weights [H, out], (bias [out]), lstm_kernel [neigh_in + H, 4H],
lstm_bias [4H].  Gate order i, j, f, o; forget_bias 1.0 added at call time; zero initial state; sequence r runs its first
L_r = max(1, #{t : row t of x_r is not all zeros}) steps and its neighborhood vector is h after step L_r - 1.

`sketch` is the compact form in which the fixtures carry the large LSTM kernel arrays (gradients, post-Adam values): row sums,
column sums and the values at 2048 fixed positions."""
import contextlib

import numpy as np

from oracle import graphsage_oracle as orc

SKETCH_PICKS = 2048


def sketch_index(shape):
    rows, cols = shape
    return np.sort(np.random.RandomState(7).choice(rows * cols, min(SKETCH_PICKS, rows * cols), replace=False))


def sketch(a):
    """{"rowsum", "colsum", "pick"} of a 2-D array (summed in float64, returned in a's dtype)."""
    a = np.asarray(a)
    return {"rowsum": a.sum(axis=1, dtype=np.float64).astype(a.dtype), "colsum": a.sum(axis=0, dtype=np.float64).astype(a.dtype),
            "pick": a.reshape(-1)[sketch_index(a.shape)]}


def lengths(neigh_vecs):
    """aggregators.py:411-414: used = sign(max_j |x|), L = max(sum(used), 1)."""
    used = (np.abs(neigh_vecs).max(axis=2) > 0).sum(axis=1)
    return np.maximum(used, 1)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_fwd(x, L, kernel, bias):
    """x [n, T, D] -> (h_last [n, H], cache)."""
    n, T, D = x.shape
    H = kernel.shape[1] // 4
    dt = x.dtype
    Wx, Wh = kernel[:D], kernel[D:]
    c = np.zeros((n, H), dt)
    h = np.zeros((n, H), dt)
    steps = []
    for t in range(T):
        z = x[:, t] @ Wx + h @ Wh + bias
        i, j, f, o = _sig(z[:, :H]), np.tanh(z[:, H:2 * H]), _sig(z[:, 2 * H:3 * H] + dt.type(1.0)), _sig(z[:, 3 * H:])
        nc = c * f + i * j
        nh = np.tanh(nc) * o
        m = (t < L)[:, None]
        steps.append((h, c, i, j, f, o, nc, m))
        c = np.where(m, nc, c)
        h = np.where(m, nh, h)
    return h, (x, L, kernel, steps)


def lstm_bwd(dh_last, cache):
    """-> (dx [n, T, D], d_kernel, d_bias); dG = 0 where t >= L (the state is copied through there)."""
    x, L, kernel, steps = cache
    n, T, D = x.shape
    H = kernel.shape[1] // 4
    Wx, Wh = kernel[:D], kernel[D:]
    dWx, dWh = np.zeros_like(Wx), np.zeros_like(Wh)
    db = np.zeros(4 * H, x.dtype)
    dx = np.zeros_like(x)
    dh, dc = dh_last.copy(), np.zeros_like(dh_last)
    for t in range(T - 1, -1, -1):
        h_prev, c_prev, i, j, f, o, nc, m = steps[t]
        dnh, dnc = np.where(m, dh, 0), np.where(m, dc, 0)
        tc = np.tanh(nc)
        dct = dnc + dnh * o * (1 - tc * tc)
        dz = np.concatenate([dct * j * i * (1 - i), dct * i * (1 - j * j), dct * c_prev * f * (1 - f),
                             dnh * tc * o * (1 - o)], axis=1)
        dWx += x[:, t].T @ dz
        dWh += h_prev.T @ dz
        db += dz.sum(axis=0)
        dx[:, t] = dz @ Wx.T
        dh = dz @ Wh.T + np.where(m, 0, dh)
        dc = dct * f + np.where(m, 0, dc)
    return dx, np.concatenate([dWx, dWh], axis=0), db


def recurrence_fwd(G, L, W_h):
    """The contract of gs_lstm_fwd (include/graphsage_amd.h): gate pre-activations G [n, T, 4H] from the input projection, lengths
    L [n], W_h [H, 4H] -> (A [n, T, 4H] activated gates, C [n, T, H] cell states, H_prev [n, T, H] = h_{t-1}, h_last [n, H],
    ran [n, T] = t < L).  A, C and H_prev are exact zeros where the step does not run (the kernel leaves A and C untouched there
    and zero-fills H_prev); H_prev is exact zero at t = 0."""
    n, T, H4 = G.shape
    H = H4 // 4
    dt = G.dtype
    A, C, Hp = np.zeros((n, T, H4), dt), np.zeros((n, T, H), dt), np.zeros((n, T, H), dt)
    ran = np.arange(T)[None, :] < np.asarray(L)[:, None]
    c, h = np.zeros((n, H), dt), np.zeros((n, H), dt)
    for t in range(T):
        m = ran[:, t]
        z = G[m, t] + h[m] @ W_h
        a = np.concatenate([_sig(z[:, :H]), np.tanh(z[:, H:2 * H]), _sig(z[:, 2 * H:3 * H] + dt.type(1.0)), _sig(z[:, 3 * H:])], axis=1)
        Hp[m, t] = h[m]
        c[m] = c[m] * a[:, 2 * H:3 * H] + a[:, :H] * a[:, H:2 * H]
        h[m] = np.tanh(c[m]) * a[:, 3 * H:]
        A[m, t], C[m, t] = a, c[m]
    return A, C, Hp, h, ran


def recurrence_bwd(dh_last, L, W_h, A, C):
    """The contract of gs_lstm_bwd: BPTT from dh_last [n, H] over the saved A and C of recurrence_fwd -> dG [n, T, 4H], exact zero
    for t >= L.  The gradient enters sequence r at its last step L_r - 1."""
    n, T, H4 = A.shape
    H = H4 // 4
    L = np.asarray(L)
    dG = np.zeros_like(A)
    dh, dc = np.zeros_like(dh_last), np.zeros_like(dh_last)
    for t in range(T - 1, -1, -1):
        m = t < L
        dh[L - 1 == t] += dh_last[L - 1 == t]
        i, j, f, o = A[m, t, :H], A[m, t, H:2 * H], A[m, t, 2 * H:3 * H], A[m, t, 3 * H:]
        cp = C[m, t - 1] if t > 0 else np.zeros_like(dh_last[m])
        tc = np.tanh(C[m, t])
        dct = dc[m] + dh[m] * o * (1 - tc * tc)
        dz = np.concatenate([dct * j * i * (1 - i), dct * i * (1 - j * j), dct * cp * f * (1 - f), dh[m] * tc * o * (1 - o)], axis=1)
        dG[m, t] = dz
        dh[m] = dz @ W_h.T
        dc[m] = dct * f
    return dG


def seq_aggregator_fwd(self_vecs, neigh_vecs, p, concat, act):
    L = lengths(neigh_vecs)
    h_last, lcache = lstm_fwd(neigh_vecs, L, p["lstm_kernel"], p["lstm_bias"])
    from_self = self_vecs @ p["self_weights"]
    from_neigh = h_last @ p["neigh_weights"]
    z = np.concatenate([from_self, from_neigh], axis=1) if concat else from_self + from_neigh
    if "bias" in p:
        z = z + p["bias"]
    y = orc._act(z, act)
    return y, (self_vecs, h_last, lcache, y)


def seq_aggregator_bwd(dy, cache, p, concat, act):
    self_vecs, h_last, lcache, y = cache
    dz = orc._act_bwd(y, dy, act)
    o = p["self_weights"].shape[1]
    dzs, dzn = (dz[:, :o], dz[:, o:]) if concat else (dz, dz)
    g = {"self_weights": self_vecs.T @ dzs, "neigh_weights": h_last.T @ dzn}
    if "bias" in p:
        g["bias"] = dz.sum(axis=0)
    d_self = dzs @ p["self_weights"].T
    dx, g["lstm_kernel"], g["lstm_bias"] = lstm_bwd(dzn @ p["neigh_weights"].T, lcache)
    return d_self, dx, g


@contextlib.contextmanager
def installed():
    """The oracle's per-aggregator dispatch (orc._agg_fwd / orc._agg_bwd) with "seq" added, for the duration of a block."""
    fwd, bwd = orc._agg_fwd, orc._agg_bwd

    def agg_fwd(aggregator_type, p, self_vecs, neigh_vecs, concat, act):
        if aggregator_type == "seq":
            return seq_aggregator_fwd(self_vecs, neigh_vecs, p, concat, act)
        return fwd(aggregator_type, p, self_vecs, neigh_vecs, concat, act)

    def agg_bwd(aggregator_type, p, dy, cache, concat, act):
        if aggregator_type == "seq":
            return seq_aggregator_bwd(dy, cache, p, concat, act)
        return bwd(aggregator_type, p, dy, cache, concat, act)
    orc._agg_fwd, orc._agg_bwd = agg_fwd, agg_bwd
    try:
        yield
    finally:
        orc._agg_fwd, orc._agg_bwd = fwd, bwd


def fixture_params(fx, prefix, dtype, supervised=True):
    """Fixture.params plus each layer's lstm_kernel / lstm_bias (full arrays: init/ only)."""
    params = fx.params(prefix, dtype, supervised)
    for i, p in enumerate(params["agg"]):
        for k in ("lstm_kernel", "lstm_bias", "bias"):
            key = "%sagg%d/%s" % (prefix, i, k)
            if key in fx.z.files:
                p[k] = fx[key].astype(dtype)
    return params
