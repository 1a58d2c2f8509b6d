"""NumPy restatement of the in-batch softmax (InfoNCE) link-prediction head (loss_fn='infonce', csrc/gs_infonce.hip) with
hand-written gradients -- test infrastructure only (the manner of tests/linkpred_oracle.py).  Nothing in the reference pins this
loss: tests/test_infonce.py checks these gradients against central finite differences and torch autograd in float64.  Computes
in the dtype of its inputs.

    u = y1 (or y1 . W),  C = [y2 ; neg]  (B + n_neg candidates),  L_ij = <u_i, C_j> / tau
    mask   : j < B, j != i and (ids2[j] == ids2[i] or ids2[j] == ids1[i])    -> candidate j is left out of row i
    loss_i = logsumexp_{j not masked} L_ij - L_ii
    G = softmax over the same set (0 where masked) - I;   d_u = G . C / tau;   d_C = G^T . u / tau
aff_all = [u . neg^T | aff] (raw) and the ranks stay defined over the sampled negatives, as for the other heads."""
import contextlib

import numpy as np


def mask(B, n_neg, ids1=None, ids2=None):
    """bool [B, B + n_neg]: True where candidate j is left out of row i.  A row's own positive (j == i) and the sampled
    negatives (j >= B) are never masked; without ids nothing is."""
    m = np.zeros((B, B + n_neg), bool)
    if ids1 is None and ids2 is None:
        return m
    ids1, ids2 = np.asarray(ids1).reshape(B), np.asarray(ids2).reshape(B)
    m[:, :B] = (ids2[None, :] == ids2[:, None]) | (ids2[None, :] == ids1[:, None])
    m[np.arange(B), np.arange(B)] = False
    return m


def infonce(u_or_y1, y2, neg, tau, ids1=None, ids2=None, W=None):
    """Inputs: normalised y1 (or, with W=None, any left operand u), y2 [B, d], neg [n_neg, d], optional W [d, d].  Returns
    dict(loss_rows, loss (their sum, not yet divided by batch_size), aff_all, ranks, mrr, d_o1, d_o2, d_neg, d_W (None
    without W), stats [B, 2] = (row maximum, log of the rescaled sum)) -- gradients of `loss`."""
    y1 = u_or_y1
    dt = y1.dtype
    B, n_neg = y1.shape[0], neg.shape[0]
    tau = np.asarray(tau, dt)
    u = y1 @ W if W is not None else y1
    C = np.concatenate([y2, neg], axis=0)
    raw = u @ C.T
    L = raw / tau
    m = mask(B, n_neg, ids1, ids2)
    Lm = np.where(m, -np.inf, L)
    mx = Lm.max(axis=1, keepdims=True)
    ex = np.where(m, 0, np.exp(Lm - mx)).astype(dt)
    s = ex.sum(axis=1, keepdims=True, dtype=dt)
    diag = L[np.arange(B), np.arange(B)]
    loss_rows = (mx[:, 0] + np.log(s[:, 0])) - diag
    G = ex / s
    G[np.arange(B), np.arange(B)] -= 1
    d_u = (G @ C) / tau
    d_C = (G.T @ u) / tau
    d_o1, d_W = (d_u @ W.T, y1.T @ d_u) if W is not None else (d_u, None)
    aff = raw[np.arange(B), np.arange(B)]
    neg_aff = raw[:, B:]
    ranks = (neg_aff >= aff[:, None]).sum(axis=1)
    return {"loss_rows": loss_rows.astype(dt), "loss": loss_rows.sum(dtype=dt), "mrr": (1.0 / (ranks + 1)).mean(), "ranks": ranks,
            "aff_all": np.concatenate([neg_aff, aff[:, None]], axis=1), "d_o1": d_o1, "d_o2": d_C[:B], "d_neg": d_C[B:],
            "d_W": d_W, "stats": np.concatenate([mx, np.log(s)], axis=1).astype(dt)}


@contextlib.contextmanager
def installed(orc, tau, ids_box, W=None):
    """For the duration of the block `orc.linkpred_fwd_bwd` (the xent head of oracle/graphsage_oracle.py, which
    unsupervised_fwd_bwd calls) is this head.  ids_box["ids"] = (ids1, ids2) or None is read at every call (the caller sets the
    step's pairs before the step); the last call's result (d_W among it) is `box["last"]`."""
    box = {}
    orig = orc.linkpred_fwd_bwd

    def head(o1, o2, neg, neg_sample_weights=1.0):
        ids = ids_box.get("ids")
        ids1, ids2 = ids if ids is not None else (None, None)
        box["last"] = infonce(o1, o2, neg, tau, ids1, ids2, None if W is None else W.astype(o1.dtype))
        return box["last"]
    orc.linkpred_fwd_bwd = head
    try:
        yield box
    finally:
        orc.linkpred_fwd_bwd = orig
