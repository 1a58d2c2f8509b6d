"""Downstream node classification on embeddings: the logistic regression of the reference's eval_scripts/ (reddit_eval.py,
ppi_eval.py, citation_eval.py: one SGDClassifier(loss="log") per class on the train nodes' embeddings, micro-F1 on the val or
test nodes), solved exactly and deterministically on the device.

Objective (scikit-learn's for SGDClassifier(loss="log"), alpha = 1e-4, penalty="l2"), per class k, one-vs-rest:

    J_k(w, b) = 1/n sum_i log(1 + exp(-s_ik (<x_i, w> + b))) + alpha/2 |w|^2          (the intercept is not regularised)

It is convex, so instead of a shuffled SGD it is minimised by L-BFGS in fp64 on the host over all classes jointly; every
loss-and-gradient evaluation is one gs_logreg_eval launch on the embedding table in device memory (ops.logreg_eval) plus one
small copy each way.  No random number is consumed; the same call twice gives the same bits.

One difference from scikit-learn: a multiclass problem with TWO classes is solved here as two one-vs-rest problems (argmax of
two logits), where scikit-learn fits one binary problem.

The scripts' other two inputs are the same classifier on other rows: the feature table (`feat`) and [features | embeddings]
(their n2v branch), both through a StandardScaler fitted on the train rows.  Here the row is never materialised:
gs_logreg_eval_joined (ops.logreg_eval_joined) joins the two tables and applies (x - mean) * (1 / scale) while it stages the tile, and
gs_col_moments (ops.col_moments) fits the scaler on the device; fit_classifier(..., features=, feature_rows=, standardize=True).
"""
from __future__ import division, print_function

import time

import numpy as np

ALPHA = 1e-4             # SGDClassifier's default alpha, which the reference leaves as it is
ARMIJO = 1e-4
MAX_HALVINGS = 30


# ------------------------------------------------------------------------------------------------ solver
def lbfgs(evaluate, n, d, c, alpha=ALPHA, gtol=1e-5, max_evals=1000, memory=10):
    """Minimise sum_k J_k over (W [d, c], b [c]) from zero by L-BFGS (two-loop recursion, `memory` pairs) with an Armijo
    backtracking line search, in fp64.

    evaluate(W, b) -> (loss [c], gW [d, c], gb [c]): the SUMS over the n rows of the log loss and its gradient, without the
    regulariser (what gs_logreg_eval writes; any evaluator with this contract will do, e.g. an fp64 NumPy one).
    Returns (W, b, J [c], evals, stop): stop is 'gtol' (max |gradient| <= gtol), 'noise' (no step along the L-BFGS direction
    nor along the negative gradient decreases the objective any further: the evaluator's rounding is reached) or 'max_evals'."""
    dc = d * c

    def f(x):
        W, b = x[:dc].reshape(d, c), x[dc:]
        loss, gW, gb = evaluate(W, b)
        Jk = np.asarray(loss, dtype=np.float64) / n + 0.5 * alpha * (W * W).sum(axis=0)
        g = np.concatenate([(np.asarray(gW, dtype=np.float64) / n + alpha * W).ravel(), np.asarray(gb, dtype=np.float64) / n])
        return Jk, g

    x = np.zeros(dc + c, dtype=np.float64)
    Jk, g = f(x)
    fx = Jk.sum()
    evals = 1
    S, Y = [], []
    stop = None
    while stop is None:
        if np.abs(g).max() <= gtol:
            stop = 'gtol'
            break
        # two-loop recursion
        q = g.copy()
        al = []
        for s_, y_ in zip(reversed(S), reversed(Y)):
            a = s_.dot(q) / y_.dot(s_)
            al.append(a)
            q -= a * y_
        if S:
            q *= S[-1].dot(Y[-1]) / Y[-1].dot(Y[-1])
        for (s_, y_), a in zip(zip(S, Y), reversed(al)):
            q += (a - y_.dot(q) / y_.dot(s_)) * s_
        p = -q
        gp = g.dot(p)
        if not gp < 0:
            S, Y = [], []
            p, gp = -g, -g.dot(g)
        while True:                 # at most twice: the L-BFGS direction, then the negative gradient
            t = 1.0 if S else 1.0 / max(1.0, np.abs(g).sum())
            found = False
            for _ in range(MAX_HALVINGS):
                if evals >= max_evals:
                    break
                xn = x + t * p
                Jn, gn = f(xn)
                evals += 1
                if Jn.sum() <= fx + ARMIJO * t * gp:
                    found = True
                    break
                t *= 0.5
            if found or evals >= max_evals or not S:
                break
            S, Y = [], []
            p, gp = -g, -g.dot(g)
        if not found:
            stop = 'max_evals' if evals >= max_evals else 'noise'
            break
        s_, y_ = xn - x, gn - g
        if s_.dot(y_) > 1e-12 * np.sqrt(s_.dot(s_) * y_.dot(y_)):
            S.append(s_)
            Y.append(y_)
            if len(S) > memory:
                S.pop(0)
                Y.pop(0)
        x, Jk, fx, g = xn, Jn, Jn.sum(), gn
        if evals >= max_evals and np.abs(g).max() > gtol:
            stop = 'max_evals'
    return x[:dc].reshape(d, c).copy(), x[dc:].copy(), Jk, evals, stop


def numpy_evaluator(X, S):
    """The evaluator contract in fp64 NumPy: X [n, d] rows, S [n, c] targets in {+1, -1}."""
    X = np.asarray(X, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)

    def evaluate(W, b):
        m = S * (X.dot(W) + b)
        loss = (np.maximum(-m, 0.0) + np.log1p(np.exp(-np.abs(m)))).sum(axis=0)
        e = np.exp(-np.abs(m))
        r = -S * np.where(m >= 0, e, 1.0) / (1.0 + e)
        return loss, X.T.dot(r), r.sum(axis=0)

    return evaluate


def objective(X, S, W, b, alpha=ALPHA):
    """J_k in fp64 for every class: X [n, d], S [n, c] in {+1, -1}."""
    X = np.asarray(X, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    m = np.asarray(S, dtype=np.float64) * (X.dot(W) + np.asarray(b, dtype=np.float64))
    return (np.maximum(-m, 0.0) + np.log1p(np.exp(-np.abs(m)))).mean(axis=0) + 0.5 * alpha * (W * W).sum(axis=0)


def targets(labels, n_classes=None):
    """labels (int vector, or 0/1 matrix) -> (S [n, c] in {+1, -1}, multilabel)."""
    labels = np.asarray(labels)
    if labels.ndim == 2:
        return np.where(labels > 0, 1.0, -1.0), True
    c = int(labels.max()) + 1 if n_classes is None else int(n_classes)
    return np.where(labels[:, None] == np.arange(c)[None, :], 1.0, -1.0), False


# ------------------------------------------------------------------------------------------------ refusals
def refuse(width, labels=None, n_classes=None):
    """The cases the device kernel does not take, as a ValueError with the rule in the message (the drivers turn it into a
    SystemExit before any training): no labels, an embedding width over 512, more than 128 classes."""
    from ._lib import LOGREG_MAX_C, LOGREG_MAX_D
    if labels is None and n_classes is None:
        raise ValueError("the dataset has no class labels to fit a classifier on")
    if width is not None and (width < 1 or -(-width // 4) * 4 > LOGREG_MAX_D):
        raise ValueError("embedding width %d is over the classifier kernel's limit of %d" % (width, LOGREG_MAX_D))
    if n_classes is None:
        labels = np.asarray(labels)
        n_classes = labels.shape[1] if labels.ndim == 2 else (int(labels.max()) + 1 if labels.size else 0)
    if n_classes < 1 or n_classes > LOGREG_MAX_C:
        raise ValueError("%d classes: the classifier kernel takes 1 to %d" % (n_classes, LOGREG_MAX_C))
    return n_classes


# ------------------------------------------------------------------------------------------------ device side
def _device(engine):
    import torch
    return engine.device if engine is not None else torch.device("cuda:%d" % torch.cuda.current_device())


def as_table(engine, Z):
    """An embedding table as a device Mat whose width is padded to a multiple of 4 with zero columns (ops.Mat, a torch tensor
    or a NumPy array [N, d]); a Mat is taken as it is."""
    import torch
    from .ops import Mat, round_up
    if isinstance(Z, Mat):
        if Z.d % 4:
            Z = Mat(Z.buf, round_up(Z.d, 4))      # the pad columns of a Mat are zero
        return Z
    if isinstance(Z, torch.Tensor):
        Z = Z.detach().cpu().numpy()
    Z = np.asarray(Z, dtype=np.float32)
    if Z.ndim != 2:
        raise ValueError("an embedding table is a matrix [N, d]")
    m = Mat.from_numpy(Z, _device(engine))
    return Mat(m.buf, round_up(Z.shape[1], 4))


def as_mat(engine, Z):
    """The table on the device at its own width (as_table pads it without another copy); a Mat is taken as it is."""
    import torch
    from .ops import Mat
    if isinstance(Z, Mat):
        return Z
    if isinstance(Z, torch.Tensor):
        Z = Z.detach().cpu().numpy()
    Z = np.asarray(Z, dtype=np.float32)
    if Z.ndim != 2:
        raise ValueError("a table is a matrix [N, d]")
    return Mat.from_numpy(Z, _device(engine))


def _rows(table, rows, dev):
    """Row indices, checked once on the host -> int32 device vector (None: all rows)."""
    import torch
    if rows is None:
        return None, table.rows
    rows = np.asarray(rows)
    if rows.ndim != 1 or rows.size == 0 or rows.dtype.kind not in "iu":
        raise ValueError("rows must be a non-empty integer vector")
    if rows.min() < 0 or rows.max() >= table.rows:
        raise ValueError("rows must lie in [0, %d)" % table.rows)
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev), int(rows.size)


def _labels(labels, n, c, multilabel, dev):
    """(y_class, y_multi) device tensors of n labels."""
    import torch
    labels = np.asarray(labels)
    if labels.shape[0] != n or (labels.ndim == 2) != multilabel or (multilabel and labels.shape[1] != c):
        raise ValueError("labels do not match: %s for %d rows, %d classes" % (labels.shape, n, c))
    if multilabel:
        return None, torch.from_numpy(np.ascontiguousarray(labels > 0, dtype=np.uint8)).to(dev)
    if labels.dtype.kind not in "iu" or labels.min() < 0 or labels.max() >= c:
        raise ValueError("class labels must be integers in [0, %d)" % c)
    return torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev), None


class _Params(object):
    """W [d, c] and b [c] in ONE fp32 device buffer [d + 1, ld] (the last row is b): one copy per evaluation."""

    def __init__(self, d, c, dev):
        import torch
        from .ops import Mat, round_up
        self.d, self.c = d, c
        self.buf = torch.zeros((d + 1, round_up(c, 4)), dtype=torch.float32, device=dev)
        self.host = torch.zeros((d + 1, round_up(c, 4)), dtype=torch.float32)
        self.W = Mat(self.buf[:d], c)
        self.b = self.buf[d, :c]

    def set(self, W, b):
        h = self.host.numpy()
        h[:self.d, :self.c] = W
        h[self.d, :self.c] = b
        self.buf.copy_(self.host)


class DeviceEvaluator(object):
    """The evaluator contract on the device: gs_logreg_eval in FIT mode on `rows` of `table`."""

    def __init__(self, table, rows, n, y_class, y_multi, c):
        import torch
        from . import ops
        dev = table.buf.device
        self.table, self.rows, self.n, self.y_class, self.y_multi = table, rows, n, y_class, y_multi
        self.d, self.c = table.d, c
        self.params = _Params(self.d, c, dev)
        self.out = torch.zeros(2 * c + self.d * c, dtype=torch.float64, device=dev)      # loss, gb, gW: one copy back
        self.ws = torch.empty(max(ops.logreg_ws_bytes(n, self.d, c) // 4, 2), dtype=torch.float32, device=dev)

    def __call__(self, W, b):
        from . import ops
        c, d = self.c, self.d
        self.params.set(W, b)
        ops.logreg_eval(self.table, self.params.W, self.params.b, n=self.n, rows=self.rows, y_class=self.y_class,
                        y_multi=self.y_multi, mode=ops.LOGREG_FIT, loss=self.out[:c], gb=self.out[c:2 * c],
                        gW=self.out[2 * c:].view(d, c), ws=self.ws)
        h = self.out.cpu().numpy()
        return h[:c], h[2 * c:].reshape(d, c), h[c:2 * c]


def _width(Z):
    """The width of a table before it is padded to a multiple of 4."""
    return Z.shape[1] if hasattr(Z, "shape") else Z.d


def refuse_joined(feature_width, embedding_width):
    """The joined input [features | embeddings] (either may be None): each source is padded to a multiple of 4 and the sum
    must not exceed the joined kernel's limit; the embedding's own limit stays refuse()'s.  Returns the padded sum."""
    from ._lib import LOGREG_JOINED_MAX_D
    pad = sum(-(-w // 4) * 4 for w in (feature_width, embedding_width) if w is not None)
    if feature_width is not None and feature_width < 1:
        raise ValueError("the feature table has no columns")
    if pad > LOGREG_JOINED_MAX_D:
        raise ValueError("joined width %d (features %s + embeddings %s, each padded to a multiple of 4) is over the classifier "
                         "kernel's limit of %d" % (pad, feature_width, embedding_width, LOGREG_JOINED_MAX_D))
    return pad


class _Sources(object):
    """A joined problem's rows on the device: source A is the feature table where one is given, else the embedding table;
    source B the embedding table behind a feature table.  widths = the two widths before padding (B's None: absent)."""

    def __init__(self, engine, Z, rows, features, feature_rows):
        if Z is None and features is None:
            raise ValueError("neither an embedding table nor a feature table is given")
        given = [(features, feature_rows)] if features is not None else []
        if Z is not None:
            given.append((Z, rows))
        self.widths = [_width(t) for t, _ in given] + [None] * (2 - len(given))
        tables = [as_table(engine, t) for t, _ in given]
        dev = tables[0].buf.device
        idx = [_rows(t, r, dev) for t, (_, r) in zip(tables, given)]
        with_rows = [n for (r, n) in idx if r is not None]
        self.n = with_rows[0] if with_rows else min(n for _, n in idx)
        if any(n != self.n for _, n in idx):          # without rows a table is taken whole
            raise ValueError("the sources do not give the same number of rows: %s" % [n for _, n in idx])
        self.Xa, self.rows_a = tables[0], idx[0][0]
        self.Xb, self.rows_b = (tables[1], idx[1][0]) if len(tables) == 2 else (None, None)
        self.da, self.db = self.Xa.d, (self.Xb.d if self.Xb is not None else 0)
        self.d = self.da + self.db
        self.dev = dev
        # the columns of the padded joined row that exist before padding
        self.cols = np.concatenate([np.arange(self.widths[0]), self.da + np.arange(self.widths[1] or 0)]).astype(np.int64)

    def kw(self):
        return dict(Xb=self.Xb, n=self.n, rows_a=self.rows_a, rows_b=self.rows_b)


def _affine(src, mean, scale):
    """(mu, inv) fp32 device vectors over the padded joined width from the scaler's fp64 mean and scale (pad columns: 0, 1)."""
    import torch
    mu, inv = np.zeros(src.d, dtype=np.float32), np.ones(src.d, dtype=np.float32)
    mu[src.cols] = mean
    inv[src.cols] = 1.0 / scale
    return torch.from_numpy(mu).to(src.dev), torch.from_numpy(inv).to(src.dev)


def fit_scaler(src):
    """StandardScaler on the joined rows, from gs_col_moments: (mean, scale) in fp64 over the columns before padding, with
    scale = sqrt(population variance) and 1 where the variance is zero."""
    from . import ops
    mean, var = ops.col_moments(src.Xa, **src.kw())
    mean, var = mean.cpu().numpy()[src.cols], var.cpu().numpy()[src.cols]
    scale = np.sqrt(var)
    scale[var == 0.0] = 1.0
    return mean, scale


class JoinedEvaluator(object):
    """The evaluator contract on the device for a joined, standardised input: gs_logreg_eval_joined in FIT mode."""

    def __init__(self, src, mu, inv, y_class, y_multi, c):
        import torch
        from . import ops
        self.src, self.mu, self.inv, self.y_class, self.y_multi = src, mu, inv, y_class, y_multi
        self.n, self.d, self.c = src.n, src.d, c
        self.params = _Params(self.d, c, src.dev)
        self.out = torch.zeros(2 * c + self.d * c, dtype=torch.float64, device=src.dev)
        self.ws = torch.empty(max(ops.logreg_joined_ws_bytes(self.n, self.d, c) // 4, 2), dtype=torch.float32, device=src.dev)

    def __call__(self, W, b):
        from . import ops
        c, d = self.c, self.d
        self.params.set(W, b)
        ops.logreg_eval_joined(self.src.Xa, self.params.W, self.params.b, mu=self.mu, inv=self.inv, y_class=self.y_class,
                               y_multi=self.y_multi, mode=ops.LOGREG_FIT, loss=self.out[:c], gb=self.out[c:2 * c],
                               gW=self.out[2 * c:].view(d, c), ws=self.ws, **self.src.kw())
        h = self.out.cpu().numpy()
        return h[:c], h[2 * c:].reshape(d, c), h[c:2 * c]


class Classifier(object):
    """A fitted one-vs-rest logistic regression: W [d, c] and b [c] in fp32, the per-class objective `loss` in fp64, the
    number of evaluations `evals` and why the solver stopped (`stop`).  Fitted on a joined input, d counts the feature
    columns and then the embedding columns (`widths`), and `mean` / `scale` (fp64 [d], None without standardisation) are the
    scaler fitted on the train rows; predict and score apply it to the tables they are given."""

    def __init__(self, engine, W, b, loss, evals, stop, multilabel, alpha, widths=None, mean=None, scale=None):
        self.engine, self.W, self.b, self.loss, self.evals, self.stop = engine, W, b, loss, evals, stop
        self.multilabel, self.alpha = multilabel, alpha
        self.n_classes = W.shape[1]
        self.widths, self.mean, self.scale = widths, mean, scale

    def _run_joined(self, Z, rows, labels, features, feature_rows):
        import torch
        from . import ops
        src = _Sources(self.engine, Z, rows, features, feature_rows)
        if src.widths != self.widths:
            raise ValueError("the input is %s wide (features, embeddings), the classifier was fitted on %s" % (
                src.widths, self.widths))
        c, n, dev = self.n_classes, src.n, src.dev
        par = _Params(src.d, c, dev)
        Wp = np.zeros((src.d, c), dtype=np.float32)
        Wp[src.cols] = self.W
        par.set(Wp, self.b)
        mu, inv = _affine(src, self.mean, self.scale) if self.mean is not None else (None, None)
        y_class = y_multi = loss = None
        if labels is not None:
            y_class, y_multi = _labels(labels, n, c, self.multilabel, dev)
            loss = torch.zeros(c, dtype=torch.float64, device=dev)
        pred_class = pred_multi = None
        if self.multilabel:
            pred_multi = torch.zeros((n, c), dtype=torch.uint8, device=dev)
        else:
            pred_class = torch.zeros(n, dtype=torch.int32, device=dev)
        ops.logreg_eval_joined(src.Xa, par.W, par.b, mu=mu, inv=inv, y_class=y_class, y_multi=y_multi, mode=ops.LOGREG_PREDICT,
                               loss=loss, pred_class=pred_class, pred_multi=pred_multi, **src.kw())
        pred = (pred_multi if self.multilabel else pred_class).cpu().numpy()
        return pred, (loss.cpu().numpy() / n if loss is not None else None)

    def _run(self, Z, rows, labels=None, features=None, feature_rows=None):
        import torch
        from . import ops
        if self.widths is not None:
            return self._run_joined(Z, rows, labels, features, feature_rows)
        if features is not None:
            raise ValueError("the classifier was fitted on embeddings alone")
        table = as_table(self.engine, Z)
        dev = table.buf.device
        d, c = self.W.shape
        if table.d != -(-d // 4) * 4:
            raise ValueError("the table is %d wide, the classifier was fitted on width %d" % (table.d, d))
        rows_dev, n = _rows(table, rows, dev)
        par = _Params(table.d, c, dev)
        Wp = np.zeros((table.d, c), dtype=np.float32)
        Wp[:d] = self.W
        par.set(Wp, self.b)
        y_class = y_multi = loss = None
        if labels is not None:
            y_class, y_multi = _labels(labels, n, c, self.multilabel, dev)
            loss = torch.zeros(c, dtype=torch.float64, device=dev)
        pred_class = pred_multi = None
        if self.multilabel:
            pred_multi = torch.zeros((n, c), dtype=torch.uint8, device=dev)
        else:
            pred_class = torch.zeros(n, dtype=torch.int32, device=dev)
        ops.logreg_eval(table, par.W, par.b, n=n, rows=rows_dev, y_class=y_class, y_multi=y_multi, mode=ops.LOGREG_PREDICT,
                        loss=loss, pred_class=pred_class, pred_multi=pred_multi)
        pred = (pred_multi if self.multilabel else pred_class).cpu().numpy()
        return pred, (loss.cpu().numpy() / n if loss is not None else None)

    def predict(self, Z, rows=None, features=None, feature_rows=None):
        """Class ids int32 [n] (argmax of the logits, lowest id on a tie), or for multi-label uint8 [n, c] (logit > 0).
        A classifier fitted on a joined input takes the same kinds of table (Z None: features alone)."""
        return self._run(Z, rows, None, features, feature_rows)[0]

    def score(self, Z, rows, labels, features=None, feature_rows=None):
        """{'f1_micro', 'f1_macro'} (sklearn.metrics.f1_score's definitions, from integer counts on the host), 'accuracy'
        (per label for multi-label -- the number ppi_eval.py prints per column -- else one number, which equals f1_micro),
        'loss' (held-out mean log loss per class, fp64, no regulariser) and 'pred'."""
        from .supervised_train import f1_micro_macro
        labels = np.asarray(labels)
        pred, loss = self._run(Z, rows, labels, features, feature_rows)
        mic, mac = f1_micro_macro(labels, pred, self.multilabel)
        if self.multilabel:
            acc = ((labels > 0) == (pred > 0)).mean(axis=0)
        else:
            acc = float((labels == pred).mean())
        return {"f1_micro": mic, "f1_macro": mac, "accuracy": acc, "loss": loss, "pred": pred}


def _fit_joined(engine, Z, rows, labels, n_classes, features, feature_rows, standardize, alpha, gtol, max_evals, memory):
    """fit_classifier on [features | embeddings] (either alone too), standardised on these rows where asked."""
    multilabel = labels.ndim == 2
    ncl = n_classes if not multilabel else None
    if Z is not None:
        refuse(_width(Z), labels, ncl)
    refuse_joined(_width(features) if features is not None else None, _width(Z) if Z is not None else None)
    c = refuse(None, labels, ncl)
    src = _Sources(engine, Z, rows, features, feature_rows)
    y_class, y_multi = _labels(labels, src.n, c, multilabel, src.dev)
    mean = scale = mu = inv = None
    if standardize:
        mean, scale = fit_scaler(src)
        mu, inv = _affine(src, mean, scale)
    ev = JoinedEvaluator(src, mu, inv, y_class, y_multi, c)
    W, b, J, evals, stop = lbfgs(ev, src.n, src.d, c, alpha=alpha, gtol=gtol, max_evals=max_evals, memory=memory)
    return Classifier(engine, W[src.cols].astype(np.float32), b.astype(np.float32), J, evals, stop, multilabel, alpha,
                      widths=src.widths, mean=mean, scale=scale)


def fit_classifier(engine, Z, rows, labels, n_classes=None, alpha=ALPHA, gtol=1e-5, max_evals=1000, memory=10, features=None,
                   feature_rows=None, standardize=False):
    """Fit the one-vs-rest logistic regression on rows `rows` of the embedding table Z (ops.Mat, torch tensor or NumPy array;
    rows None: all) with `labels` an int vector (multiclass) or a 0/1 matrix (multi-label).  Returns a Classifier.
    With `features` (a table of the same kinds) and its `feature_rows` the input rows are [features | embeddings]; Z None
    leaves the features alone.  standardize=True fits a StandardScaler on THESE rows (the train rows) on the device, applies
    it while the rows are staged and keeps it on the Classifier (mean, scale)."""
    labels = np.asarray(labels)
    multilabel = labels.ndim == 2
    if features is not None or standardize or Z is None:
        return _fit_joined(engine, Z, rows, labels, n_classes, features, feature_rows, standardize, alpha, gtol, max_evals, memory)
    d = _width(Z)                                        # the width before padding to a multiple of 4
    refuse(d, labels, n_classes if not multilabel else None)
    table = as_table(engine, Z)
    c = refuse(table.d, labels, n_classes if not multilabel else None)
    dev = table.buf.device
    rows_dev, n = _rows(table, rows, dev)
    y_class, y_multi = _labels(labels, n, c, multilabel, dev)
    ev = DeviceEvaluator(table, rows_dev, n, y_class, y_multi, c)
    W, b, J, evals, stop = lbfgs(ev, n, table.d, c, alpha=alpha, gtol=gtol, max_evals=max_evals, memory=memory)
    return Classifier(engine, W[:d].astype(np.float32), b.astype(np.float32), J, evals, stop, multilabel, alpha)


# ------------------------------------------------------------------------------------------------ what the drivers print
def baseline_f1_micro(train_labels, test_labels):
    """Micro-F1 of predicting the most frequent class of the train part for every test row (multi-label: every label at its
    more frequent value) -- sklearn's DummyClassifier(strategy="prior"), the `Random baseline` of the reference's scripts."""
    from .supervised_train import f1_micro_macro
    train_labels, test_labels = np.asarray(train_labels), np.asarray(test_labels)
    if train_labels.ndim == 2:
        pred = np.tile((2 * (train_labels > 0).sum(axis=0) > train_labels.shape[0]).astype(np.uint8), (test_labels.shape[0], 1))
        return f1_micro_macro(test_labels, pred, True)[0]
    top = int(np.argmax(np.bincount(train_labels.astype(np.int64))))
    return f1_micro_macro(test_labels, np.full(test_labels.shape[0], top, dtype=np.int64), False)[0]


def result_line(setting, res):
    return ("Downstream classifier: setting= %s classes= %d train= %d test= %d f1_micro= %.5f f1_macro= %.5f train_f1_micro= %.5f "
            "baseline_f1_micro= %.5f loss= %.6f evals= %d stop= %s time= %.5f" % (
                setting, res["classes"], res["train"], res["test"], res["f1_micro"], res["f1_macro"], res["train_f1_micro"],
                res["baseline_f1_micro"], res["loss"], res["evals"], res["stop"], res["time"]))


INPUTS = ("embeddings", "features", "both")
LINE_PREFIX = {"embeddings": "Downstream classifier:", "features": "Downstream classifier (features):",
               "both": "Downstream classifier (features+embeddings):"}
LINE_FILE = {"embeddings": "eval_classifier.txt", "features": "eval_classifier_features.txt", "both": "eval_classifier_both.txt"}


def joined_result_line(inputs, setting, res):
    """The line of the `features` and `both` inputs: the fields of result_line with width= (the joined width before padding)
    ahead of time=."""
    line = result_line(setting, res)
    head, tail = line[len(LINE_PREFIX["embeddings"]):].rsplit(" time= ", 1)
    return "%s%s width= %d time= %s" % (LINE_PREFIX[inputs], head, res["width"], tail)


def evaluate_split(engine, train_table, train_rows, train_labels, test_table, test_rows, test_labels, features=None,
                   train_feature_rows=None, test_feature_rows=None, standardize=False, **kw):
    """Fit on (train_table, train_rows), score on (test_table, test_rows): the fields of the `Downstream classifier:` line.
    loss is the held-out mean log loss summed over the classes.  With `features` (one table for both parts, with its train
    and test rows) the input is [features | embeddings], or the features alone where train_table is None."""
    t0 = time.time()
    joined = features is not None or standardize
    up = as_mat if joined else as_table              # one upload per table; the joined path keeps the widths before padding
    if train_table is not None:
        train_table = up(engine, train_table)
        test_table = train_table if test_table is None else up(engine, test_table)
    fkw = {}
    if joined:
        features = as_mat(engine, features) if features is not None else None
        fkw = dict(features=features, feature_rows=train_feature_rows)
        kw = dict(kw, standardize=standardize)
    clf = fit_classifier(engine, train_table, train_rows, train_labels, **dict(kw, **fkw))
    test = clf.score(test_table, test_rows, test_labels, **dict(fkw, feature_rows=test_feature_rows) if fkw else {})
    train = clf.score(train_table, train_rows, train_labels, **fkw)
    res = {"classes": clf.n_classes, "train": len(train_labels), "test": len(test_labels), "f1_micro": test["f1_micro"],
           "f1_macro": test["f1_macro"], "train_f1_micro": train["f1_micro"],
           "baseline_f1_micro": baseline_f1_micro(train_labels, test_labels), "loss": float(np.sum(test["loss"])),
           "evals": clf.evals, "stop": clf.stop, "time": time.time() - t0, "classifier": clf}
    if clf.widths is not None:
        res["width"] = sum(w for w in clf.widths if w is not None)
    return res


# ------------------------------------------------------------------------------------------------ from the drivers' files
def load_table(embed_dir, name):
    """<embed_dir>/<name>.npy and .txt (one ORIGINAL node id per row, as the drivers write them) -> (float32 [M, d], {id: row})."""
    import os
    emb = np.load(os.path.join(embed_dir, name + ".npy")).astype(np.float32, copy=False)
    with open(os.path.join(embed_dir, name + ".txt")) as fp:
        index = {line.strip(): i for i, line in enumerate(fp) if line.strip()}
    if emb.ndim != 2 or len(index) != emb.shape[0]:
        raise SystemExit("%s: %s.npy has %s rows, %s.txt lists %d ids" % (embed_dir, name, emb.shape, name, len(index)))
    return emb, index


def refuse_graph(G):
    """A dataset that the classifier cannot be fitted on is refused (SystemExit) before any training."""
    labels = getattr(G, "labels", None)
    try:
        return refuse(None, labels)
    except ValueError as e:
        raise SystemExit("--eval_classifier: %s" % e)


def refuse_inputs(inputs, feature_width, embedding_width, has_features=True):
    """`features` and `both` need a feature table and a joined width the kernel takes; as a SystemExit with the rule."""
    if inputs not in INPUTS:
        raise SystemExit("the inputs are one of %s, not %s" % (", ".join(INPUTS), inputs))
    if inputs == "embeddings":
        return
    if not has_features:
        raise SystemExit("--eval_classifier inputs %s: the dataset has no feature table (identity features only)" % inputs)
    try:
        refuse_joined(feature_width, embedding_width if inputs == "both" else None)
    except ValueError as e:
        raise SystemExit("--eval_classifier inputs %s: %s" % (inputs, e))


def evaluate_embedding_dir(engine, G, embed_dir, setting, base="val", inputs="embeddings", features=None):
    """The reference's eval_scripts on the files of a log directory: fit on the train nodes (neither val nor test) of
    <base>.npy, score on the `setting` nodes -- from val-test.npy where that table exists (the node2vec baseline,
    reddit_eval.py:61-77), else from <base>.npy.  Prints the `Downstream classifier:` line, writes eval_classifier.txt.
    inputs = "features" fits on the rows of the feature table instead (`feat` of the scripts; no embedding file is read),
    "both" on [features | embeddings] (their n2v branch); both standardise on the train rows, as the scripts do, print
    their own line and write eval_classifier_features.txt / eval_classifier_both.txt.  `features` is the table [N, F]
    indexed by node (a NumPy array or a device Mat with at least N rows); default G.feats."""
    import os
    if setting not in ("val", "test"):
        raise SystemExit("the setting is val or test, not %s" % setting)
    refuse_graph(G)
    if features is None and inputs != "embeddings":
        features = getattr(G, "feats", None)
    refuse_inputs(inputs, _width(features) if features is not None else None, None, features is not None)
    ids = getattr(G, "node_ids", None)
    key = (lambda r: str(ids[r])) if ids is not None else (lambda r: str(r))
    held = G.val_mask | G.test_mask
    train_nodes = np.where(G.present & ~held)[0]
    test_nodes = np.where(G.present & (G.val_mask if setting == "val" else G.test_mask))[0]
    if not len(train_nodes) or not len(test_nodes):
        raise SystemExit("--eval_classifier %s: %d train nodes, %d %s nodes" % (setting, len(train_nodes), len(test_nodes), setting))
    emb = test_emb = train_rows = test_rows = None
    if inputs != "features":
        emb, index = load_table(embed_dir, base)
        try:
            refuse(emb.shape[1], G.labels)
        except ValueError as e:
            raise SystemExit("--eval_classifier: %s" % e)
        refuse_inputs(inputs, _width(features) if features is not None else None, emb.shape[1])
        test_emb, test_index = (emb, index)
        if os.path.exists(os.path.join(embed_dir, "val-test.npy")):
            test_emb, test_index = load_table(embed_dir, "val-test")
        try:
            train_rows = np.array([index[key(r)] for r in train_nodes], dtype=np.int64)
            test_rows = np.array([test_index[key(r)] for r in test_nodes], dtype=np.int64)
        except KeyError as e:
            raise SystemExit("%s: the embedding table has no row for node %s" % (embed_dir, e))
    labels = np.asarray(G.labels)
    labels = (labels > 0).astype(np.uint8) if labels.ndim == 2 else labels.astype(np.int64)
    kw = {} if labels.ndim == 2 else {"n_classes": int(labels.max()) + 1}
    if inputs != "embeddings":
        kw.update(features=features, train_feature_rows=train_nodes, test_feature_rows=test_nodes, standardize=True)
    res = evaluate_split(engine, emb, train_rows, labels[train_nodes], None if test_emb is emb else test_emb, test_rows,
                         labels[test_nodes], **kw)
    line = result_line(setting, res) if inputs == "embeddings" else joined_result_line(inputs, setting, res)
    print(line)
    with open(os.path.join(embed_dir, LINE_FILE[inputs]), "w") as fp:
        fp.write(line + "\n")
    return res
