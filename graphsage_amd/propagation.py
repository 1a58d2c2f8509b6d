"""Label propagation and Correct and Smooth (Huang et al., ICLR 2021) over a FullGraph.

What a trained supervised model leaves in device memory -- the test graph, every node's exact predictions (predict_full) and
the train nodes' labels -- used together: the train nodes' residual errors are propagated over the graph and added to the
predictions (correct), then the labels themselves are propagated (smooth).  Plain label propagation is the graph-only baseline.

    res = correct_and_smooth(engine, graph, preds, labels, known)       # {"preds", "corrected", "sigma", "iters"}
    res = sup_model.correct_and_smooth(graph, labels, known)            # predict_full, then the above
    Y = label_propagation(engine, graph, labels, known)

The propagation law (gs_prop_weights / gs_prop_step, csrc/gs_propagate.hip; restated in fp64 by tests/propagate_oracle.py).
With pad = N, the graph's pad id:

    deg[r] = the entries of row r that are not pad (a duplicate counts as often as it occurs), deg[pad] = 0
    w[r]   = fp32(1 / sqrt((double)deg[r])), 0 where deg[r] = 0
    s      = w[r] * sum_e w[col[e]] * X[col[e]][j]              a pad entry contributes exactly 0
    out[r][j] = min(max(fmaf(alpha, s, R[r][j]), lo), hi),      out[pad][:] = 0

Rows may be directed, hold duplicates and pad entries anywhere (FullGraph.from_padded tables are such rows); from_csr gives a
node without neighbors the single neighbor pad: deg = 0 and out = clamp(R[r]).  On a symmetric CSR the operator is
D^-1/2 A D^-1/2.  One iteration is ONE fused launch (two when the graph has rows longer than split_len), bitwise repeatable.

This is the autoscale variant of the paper: the propagated error of a row is scaled to the mean l1 norm sigma of the known
rows' errors (gs_prop_correct).  The fixed-scale variant, which re-imposes the known rows at every step, is not implemented.
"""
import numpy as np

from . import ops
from ._lib import GraphsageAmdError

MAX_ITERS = 1000
LD_MULTIPLE = 32         # floats: every table row starts on a 128-byte line


def check_schedule(alpha, iters, who="propagation"):
    """alpha in (0, 1], iters in [1, MAX_ITERS]."""
    if not (isinstance(alpha, (int, float, np.floating)) and 0.0 < float(alpha) <= 1.0):
        raise GraphsageAmdError("%s: alpha = %r must lie in (0, 1]" % (who, alpha))
    if int(iters) != iters or not 1 <= int(iters) <= MAX_ITERS:
        raise GraphsageAmdError("%s: iters = %r must lie in [1, %d]" % (who, iters, MAX_ITERS))


def check_classes(C, who="propagation"):
    if not 1 <= int(C) <= ops.PROP_MAX_D:
        raise GraphsageAmdError("%s: %d classes; the propagation kernel takes 1 .. %d" % (who, C, ops.PROP_MAX_D))


def check_known(known, n_nodes, who="propagation"):
    """The known rows as an int64 index vector: not empty, every index in [0, N)."""
    known = np.asarray(known)
    if known.dtype == np.bool_:
        if known.shape != (n_nodes,):
            raise GraphsageAmdError("%s: a boolean `known` must have N = %d entries" % (who, n_nodes))
        known = np.flatnonzero(known)
    known = np.ascontiguousarray(known.reshape(-1), dtype=np.int64)
    if known.size == 0:
        raise GraphsageAmdError("%s: no known row" % who)
    if known.min() < 0 or known.max() >= n_nodes:
        raise GraphsageAmdError("%s: known indices must lie in [0, %d) (found %d .. %d)" % (who, n_nodes, known.min(), known.max()))
    return known


def _check_table(name, a, n_nodes, C, who):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[0] != n_nodes or (C is not None and a.shape[1] != C):
        raise GraphsageAmdError("%s: %s has shape %s, wanted [N = %d, C%s]" % (who, name, a.shape, n_nodes,
                                                                                "" if C is None else " = %d" % C))
    return a


class Propagator(object):
    """The propagation state of one graph on one engine: deg and w (computed once), and per table width two ping-pong tables
    and a residual table of N + 1 rows whose leading dimension is a multiple of 32 floats."""

    def __init__(self, engine, graph):
        from .inference import FullGraph
        if not isinstance(graph, FullGraph):
            raise GraphsageAmdError("propagation needs a FullGraph (FullGraph.from_csr / from_padded)")
        self.engine, self.graph = engine, graph
        self.n_nodes, self.n_rows, self.pad = graph.n_nodes, graph.n_rows, graph.n_nodes
        self.n_slots = int(graph.splits[:, 2].sum()) if graph.splits.shape[0] else 0
        rowptr, col, _, _ = graph.on(engine.device)
        engine.sync()
        self.deg, self.w = ops.prop_weights(rowptr, col, self.n_rows, self.pad, stream=engine.stream)
        engine.sync()
        self._tables = {}

    def tables(self, C):
        """(A, B, R): the two ping-pong tables and the residual table of width C."""
        import torch
        check_classes(C, "Propagator")
        if C not in self._tables:
            self._tables[C] = tuple(ops.Mat.zeros(self.n_rows, C, self.engine.device, LD_MULTIPLE) for _ in range(3))
            torch.cuda.synchronize()          # the zero-fills ran on torch's stream; order them before the engine's
        return self._tables[C]

    def _workspace(self, C):
        if not self.n_slots:
            return None
        words = ops.prop_ws_bytes(self.n_slots, C) // 4
        return self.engine.ws_f32(("prop_ws",), max(1 << 16, 1 << (words - 1).bit_length()))

    def step(self, X, out, R=None, alpha=1.0, lo=float("-inf"), hi=float("inf")):
        """One launch of the law above: out = clamp(alpha * S X + R) on the engine's stream (X, out, R: Mats of N + 1 rows)."""
        rowptr, col, items, splits = self.graph.on(self.engine.device)
        return ops.prop_step(rowptr, col, items, splits, self.n_rows, self.graph.split_len, self.pad, self.w, X, out, R=R,
                             alpha=alpha, lo=lo, hi=hi, n_slots=self.n_slots, ws=self._workspace(X.d), stream=self.engine.stream)

    def run(self, X0, alpha, iters, clamp=None, keep_residual=True, device=False):
        """X^{t+1} = clamp(alpha S X^t + (1 - alpha) X0) from X^0 = X0, `iters` times (keep_residual=False: without the X0 term).
        X0: a NumPy [N, C] array or a device Mat of at least N rows; clamp: None or (lo, hi).  Returns a NumPy [N, C] array, or
        with device=True the device Mat [N + 1, C] that holds the result until the next run of this width."""
        import torch
        check_schedule(alpha, iters, "Propagator.run")
        if isinstance(X0, ops.Mat):
            if X0.rows < self.n_nodes:
                raise GraphsageAmdError("Propagator.run: X0 has %d rows, the graph %d nodes" % (X0.rows, self.n_nodes))
            C = X0.d
        else:
            X0 = np.ascontiguousarray(_check_table("X0", X0, self.n_nodes, None, "Propagator.run"), dtype=np.float32)
            C = X0.shape[1]
        lo, hi = (float("-inf"), float("inf")) if clamp is None else (float(clamp[0]), float(clamp[1]))
        if not lo <= hi:
            raise GraphsageAmdError("Propagator.run: clamp = %r is no interval" % (clamp,))
        A, B, R = self.tables(C)
        e, N = self.engine, self.n_nodes
        e.sync()
        src = X0.view()[:N] if isinstance(X0, ops.Mat) else torch.from_numpy(X0).to(e.device)
        A.buf[:N, :C].copy_(src)
        A.buf[N].zero_()
        if keep_residual:
            torch.mul(A.buf, float(np.float32(1.0 - alpha)), out=R.buf)          # (1 - alpha) X0, stored once
        torch.cuda.synchronize()              # the fills ran on torch's stream; order them before the engine's
        for _ in range(int(iters)):
            self.step(A, B, R if keep_residual else None, float(alpha), lo, hi)
            A, B = B, A
        e.sync()
        return A if device else A.numpy()[:N].copy()


def _seed_table(labels, known, dtype=np.float32):
    """`labels` on the known rows, 0 elsewhere."""
    X0 = np.zeros(labels.shape, dtype)
    X0[known] = labels[known]
    return X0


def label_propagation(engine, graph, labels, known, alpha=0.8, iters=50, propagator=None):
    """Plain label propagation: X0 = `labels` ([N, C]) on the rows `known` (indices or a boolean mask) and 0 elsewhere,
    X^{t+1} = clamp(alpha S X^t + (1 - alpha) X0, 0, 1).  Returns the NumPy [N, C] scores."""
    who = "label_propagation"
    check_schedule(alpha, iters, who)
    labels = _check_table("labels", labels, graph.n_nodes, None, who)
    check_classes(labels.shape[1], who)
    known = check_known(known, graph.n_nodes, who)
    prop = propagator if propagator is not None else Propagator(engine, graph)
    return prop.run(_seed_table(labels, known), alpha, iters, clamp=(0.0, 1.0))


def correct_and_smooth(engine, graph, preds, labels, known, correct_alpha=0.8, smooth_alpha=0.8, iters=50, propagator=None):
    """Correct and Smooth, autoscale variant, from the predictions `preds` ([N, C], softmax or sigmoid outputs) and the `labels`
    ([N, C]) of the rows `known`:

      1. E0 = labels - preds on the known rows, 0 elsewhere; sigma = the mean over the known rows of |E0_i|_1 (fp64, host)
      2. E  = run(E0, correct_alpha, iters, clamp=(-1, 1))
      3. G0 = known ? labels : preds + (sigma / |E_i|_1) E, the scale replaced by 1 where not finite or above 1000
      4. G  = run(G0, smooth_alpha, iters, clamp=(0, 1))

    Returns {"preds": G, "corrected": G0, "sigma": sigma, "iters": iters} (NumPy [N, C] arrays)."""
    import torch
    who = "correct_and_smooth"
    check_schedule(correct_alpha, iters, who)
    check_schedule(smooth_alpha, iters, who)
    N = graph.n_nodes
    preds = _check_table("preds", preds, N, None, who)
    C = preds.shape[1]
    check_classes(C, who)
    labels = _check_table("labels", labels, N, C, who)
    known = check_known(known, N, who)
    prop = propagator if propagator is not None else Propagator(engine, graph)
    e = engine
    preds32 = np.ascontiguousarray(preds, dtype=np.float32)
    labels32 = np.ascontiguousarray(labels, dtype=np.float32)
    E0 = np.zeros((N, C), np.float32)
    E0[known] = labels32[known] - preds32[known]
    sigma = float(np.abs(E0[known].astype(np.float64)).sum(axis=1).mean())
    flags = np.zeros(N, np.int32)
    flags[known] = 1
    P = ops.Mat.from_numpy(preds32, e.device, LD_MULTIPLE)
    Y = ops.Mat.from_numpy(_seed_table(labels32, known), e.device, LD_MULTIPLE)
    G0 = ops.Mat.zeros(N, C, e.device, LD_MULTIPLE)
    known_dev = torch.from_numpy(flags).to(e.device)
    torch.cuda.synchronize()                  # the uploads ran on torch's stream; order them before the engine's
    E = prop.run(E0, correct_alpha, iters, clamp=(-1.0, 1.0), device=True)
    ops.prop_correct(P, E, sigma, G0, Y=Y, known=known_dev, n=N, stream=e.stream)
    e.sync()
    corrected = G0.numpy().copy()
    G = prop.run(G0, smooth_alpha, iters, clamp=(0.0, 1.0))
    return {"preds": G, "corrected": corrected, "sigma": sigma, "iters": int(iters)}
