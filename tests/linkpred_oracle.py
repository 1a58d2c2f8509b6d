"""NumPy restatement of BipartiteEdgePredLayer (graphsage/prediction.py:68-125) + the ranks of models.py:393-405, with
hand-written gradients -- test infrastructure only (the manner of tests/seq_oracle.py).  Computes in the dtype of its inputs
(float64 pins the algebra to 1e-9 against the reference's float64 twin).

    aff_i = <u_i, y2_i>,  neg_aff = u . neg^T,   u = y1 (bilinear_weights=False) or y1 . W (:74-77, :89-91)
    xent      loss_i = xent(1, aff_i) + w sum_j xent(0, neg_aff_ij)                                           (:102-110)
    skipgram  loss_i = aff_i - log sum_j exp(neg_aff_ij)      -- the reference's sign: minimising pushes pairs apart (:112-117)
    hinge     loss_i = sum_j relu(neg_aff_ij - (aff_i - margin)),  relu'(0) = 0                                (:119-125)
neg_sample_weights enters xent only, as in the reference."""
import contextlib

import numpy as np

LOSS_FNS = ("xent", "skipgram", "hinge")


def _sigmoid(x):
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x)))).astype(x.dtype)


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def hinge_terms(aff_all, margin=0.1):
    """t_ij = neg_aff_ij - (aff_i - margin) from an aff_all = [neg_aff | aff] array: the mask is t > 0."""
    aff_all = np.asarray(aff_all)
    return aff_all[:, :-1] - (aff_all[:, -1:] - np.asarray(margin, aff_all.dtype))


def linkpred(y1, y2, neg, loss_fn="xent", W=None, margin=0.1, neg_sample_weights=1.0):
    """Inputs: normalised y1, y2 [B, d], neg [n_neg, d], optional W [d, d].  Returns dict(loss_rows, loss (their sum, not yet
    divided by batch_size), aff_all, ranks, mrr, d_o1, d_o2, d_neg, d_W (None without W)) -- gradients of `loss`."""
    assert loss_fn in LOSS_FNS, loss_fn
    dt = y1.dtype
    u = y1 @ W if W is not None else y1
    aff = (u * y2).sum(axis=1, dtype=dt)
    neg_aff = u @ neg.T
    if loss_fn == "xent":
        w = np.asarray(neg_sample_weights, dt)
        loss_rows = _softplus(-aff) + w * _softplus(neg_aff).sum(axis=1, dtype=dt)
        d_aff = _sigmoid(aff) - 1.0
        d_neg_aff = w * _sigmoid(neg_aff)
    elif loss_fn == "skipgram":
        mx = neg_aff.max(axis=1, keepdims=True)
        ex = np.exp(neg_aff - mx)
        s = ex.sum(axis=1, keepdims=True, dtype=dt)
        loss_rows = aff - (mx[:, 0] + np.log(s[:, 0]))
        d_aff = np.ones_like(aff)
        d_neg_aff = -ex / s
    else:
        t = neg_aff - (aff[:, None] - np.asarray(margin, dt))
        m = t > 0
        loss_rows = np.where(m, t, 0).sum(axis=1, dtype=dt)
        d_neg_aff = m.astype(dt)
        d_aff = -d_neg_aff.sum(axis=1, dtype=dt)
    d_u = d_aff[:, None] * y2 + d_neg_aff @ neg
    d_o2 = d_aff[:, None] * u
    d_neg = d_neg_aff.T @ u
    d_o1, d_W = (d_u @ W.T, y1.T @ d_u) if W is not None else (d_u, None)
    ranks = (neg_aff >= aff[:, None]).sum(axis=1)
    return {"loss_rows": loss_rows.astype(dt), "loss": loss_rows.sum(dtype=dt), "mrr": (1.0 / (ranks + 1)).mean(), "ranks": ranks,
            "aff_all": np.concatenate([neg_aff, aff[:, None]], axis=1), "d_o1": d_o1, "d_o2": d_o2, "d_neg": d_neg, "d_W": d_W}


def l2_normalize(x, eps=1e-12):
    """tf.nn.l2_normalize(x, 1): x * rsqrt(max(sum x^2, eps))."""
    return x / np.sqrt(np.maximum((x * x).sum(axis=1, keepdims=True), np.asarray(eps, x.dtype)))


def l2_normalize_bwd(dy, x, eps=1e-12):
    ss = (x * x).sum(axis=1, keepdims=True)
    inv = 1.0 / np.sqrt(np.maximum(ss, np.asarray(eps, x.dtype)))
    y = x * inv
    return np.where(ss < eps, dy * inv, inv * (dy - y * (dy * y).sum(axis=1, keepdims=True)))


@contextlib.contextmanager
def installed(orc, loss_fn, W=None, margin=0.1):
    """For the duration of the block `orc.linkpred_fwd_bwd` (the xent head of oracle/graphsage_oracle.py, which
    unsupervised_fwd_bwd calls) is this head; the last call's result (d_W among it) is `box["last"]`."""
    box = {}
    orig = orc.linkpred_fwd_bwd

    def head(o1, o2, neg, neg_sample_weights=1.0):
        box["last"] = linkpred(o1, o2, neg, loss_fn, None if W is None else W.astype(o1.dtype), margin, neg_sample_weights)
        return box["last"]
    orc.linkpred_fwd_bwd = head
    try:
        yield box
    finally:
        orc.linkpred_fwd_bwd = orig
