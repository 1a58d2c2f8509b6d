"""NumPy fp64 oracle of the propagation law (graphsage_amd/propagation.py, csrc/gs_propagate.hip).

A graph is a list of rows (`lists`: row r = the int array of its entries, FullGraph.lists()) over N + 1 rows, pad = N.
"""
import numpy as np


def weights(lists, pad):
    """(deg int64 [n_rows], w float32 [n_rows]): deg[r] = the entries of row r that are not pad (deg[pad] = 0),
    w = np.float32(1 / np.sqrt(np.float64(deg))), 0 where deg = 0."""
    deg = np.array([0 if r == pad else int((np.asarray(row) != pad).sum()) for r, row in enumerate(lists)], dtype=np.int64)
    w = np.zeros(len(lists), np.float32)
    pos = deg > 0
    w[pos] = (1.0 / np.sqrt(deg[pos].astype(np.float64))).astype(np.float32)      # np.float32(1 / np.sqrt(np.float64(deg)))
    return deg, w


def step(lists, pad, w, X, R=None, alpha=1.0, lo=-np.inf, hi=np.inf, with_bound=False):
    """One step in fp64 over X [n_rows, C]: out[r] = clamp(alpha * w[r] * sum_e w[c] X[c] + R[r]), a pad entry contributes exactly
    0, out[pad] = 0.  with_bound: also B[r][j] = sum_e |w_r w_c X[c][j]| + |R[r][j]| and the row lengths."""
    X = np.asarray(X, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    out = np.zeros_like(X)
    bound = np.zeros_like(X)
    for r, row in enumerate(lists):
        if r == pad:
            continue
        row = np.asarray(row, dtype=np.int64)
        real = row[row != pad]
        terms = w[real][:, None] * X[real]
        s = w[r] * terms.sum(axis=0)
        res = R[r].astype(np.float64) if R is not None else 0.0
        out[r] = np.minimum(np.maximum(alpha * s + res, lo), hi)
        bound[r] = np.abs(w[r] * terms).sum(axis=0) + np.abs(res)
    if with_bound:
        return out, bound, np.array([len(row) for row in lists], dtype=np.int64)
    return out


def dense_operator(lists, pad, w):
    """S [N, N] with S[r][c] = w[r] * w[c] * (the multiplicity of c in row r); pad entries left out."""
    N = pad
    S = np.zeros((N, N), np.float64)
    for r in range(N):
        for c in np.asarray(lists[r], dtype=np.int64):
            if c != pad:
                S[r, c] += np.float64(w[r]) * np.float64(w[c])
    return S


def run(lists, pad, X0, alpha, iters, clamp=None, keep_residual=True, dtype=np.float64):
    """X^{t+1} = clamp(alpha S X^t + (1 - alpha) X0) from X^0 = X0 ([N, C]); dtype=np.float32 runs the same algorithm in fp32
    through the dense operator (the input screening of the end-to-end tests)."""
    N = pad
    _, w = weights(lists, pad)
    S = dense_operator(lists, pad, w).astype(dtype)
    X0 = np.asarray(X0).astype(dtype)
    lo, hi = (-np.inf, np.inf) if clamp is None else clamp
    R = (dtype(1.0 - alpha) * X0) if keep_residual else np.zeros_like(X0)
    X = X0.copy()
    for _ in range(int(iters)):
        X = np.minimum(np.maximum(dtype(alpha) * (S @ X) + R, dtype(lo)), dtype(hi)).astype(dtype)
    assert X.shape[0] == N
    return X


def seed_table(labels, known, dtype=np.float64):
    X0 = np.zeros(np.asarray(labels).shape, dtype)
    X0[known] = np.asarray(labels)[known]
    return X0


def label_propagation(lists, pad, labels, known, alpha=0.8, iters=50, dtype=np.float64):
    return run(lists, pad, seed_table(labels, known, dtype), alpha, iters, clamp=(0.0, 1.0), dtype=dtype)


def scale_rule(sigma, E):
    """(scale [n], raw [n]): raw = sigma / l1 of every row (inf at l1 = 0), scale = raw replaced by 1 where it is not finite or
    exceeds 1000."""
    l1 = np.abs(np.asarray(E)).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = np.asarray(sigma, dtype=l1.dtype) / l1
    scale = np.where(np.isfinite(raw) & (raw <= 1000.0), raw, 1.0)
    return scale, raw


def correct(P, E, Y, known_mask, sigma):
    """(G0, raw): G0[i] = known ? Y[i] : P[i] + scale_i E[i]."""
    scale, raw = scale_rule(sigma, E)
    G0 = np.asarray(P) + scale[:, None].astype(np.asarray(E).dtype) * np.asarray(E)
    G0[known_mask] = np.asarray(Y)[known_mask]
    return G0, raw


def correct_and_smooth(lists, pad, preds, labels, known, correct_alpha=0.8, smooth_alpha=0.8, iters=50, dtype=np.float64):
    """The autoscale variant; returns {"preds", "corrected", "sigma", "raw_scale"}."""
    preds = np.asarray(preds).astype(dtype)
    labels = np.asarray(labels).astype(dtype)
    N = pad
    E0 = np.zeros_like(preds)
    E0[known] = labels[known] - preds[known]
    sigma = float(np.abs(E0[known].astype(np.float64)).sum(axis=1).mean())
    E = run(lists, pad, E0, correct_alpha, iters, clamp=(-1.0, 1.0), dtype=dtype)
    mask = np.zeros(N, bool)
    mask[known] = True
    G0, raw = correct(preds, E, seed_table(labels, known, dtype), mask, dtype(sigma))
    G = run(lists, pad, G0, smooth_alpha, iters, clamp=(0.0, 1.0), dtype=dtype)
    return {"preds": G, "corrected": G0, "sigma": sigma, "raw_scale": raw}
