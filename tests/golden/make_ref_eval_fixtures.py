"""Generate tests/golden/ref_eval_{multiclass,multilabel}.npz by EXECUTING THE REFERENCE'S OWN run_regression.

    GRAPHSAGE_REFERENCE=<reference tree> python tests/golden/make_ref_eval_fixtures.py

`eval_scripts/reddit_eval.py` and `eval_scripts/ppi_eval.py` of the reference are imported UNMODIFIED at run time (nothing of
them is copied into this repository) and their `run_regression(train_embeds, train_labels, test_embeds, test_labels)` is
called on small synthetic unit-norm embeddings.  Two stand-ins make that possible on a current scikit-learn, in the manner of
tests/tf1_shim:
  * the name `sklearn.linear_model.SGDClassifier` is bound to a factory that maps the retired spelling loss="log" to
    "log_loss", and the class's fit records every fitted instance (run_regression keeps its classifiers to itself);
  * the name `sklearn.multioutput.MultiOutputClassifier` is bound to a factory that fits in this process (n_jobs=None): the
    per-label SGD draws from the global NumPy generator that run_regression seeds, which worker processes would not share.
Not part of the suite; needs scikit-learn and scipy, which graphsage_amd/ itself never imports.

Each file holds: X_train / X_test (float32, unit rows), y_train / y_test (int64 [n] or uint8 [n, c]), the reference's
ref_coef [d, c] / ref_intercept [c] and the F1 figures it PRINTED (ref_f1_*), alpha, and the fp64 optimum of the very
objective scikit-learn's SGD descends,

    J_k(w, b) = 1/n sum_i log(1 + exp(-s_ik (<x_i, w> + b))) + alpha/2 |w|^2,

as W_star [d, c], b_star [c], J_star [c] (scipy L-BFGS-B at gtol=1e-11 per class, then Newton steps on the exact Hessian until
the gradient is at rounding level) with J_ref [c], the same objective at the reference's coefficients.  The generator asserts
J_ref >= J_star for every class: a convex objective has no value below its optimum.
"""
import contextlib
import importlib.util
import io
import os
import re
import sys
import types

import numpy as np
import scipy.optimize as so
import sklearn.linear_model
import sklearn.multioutput

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GRAPHSAGE_REFERENCE", os.path.join(HERE, "..", "..", "..", "reference"))
ALPHA = 1e-4                     # SGDClassifier's default, which run_regression leaves as it is

FITTED = []


REAL_SGD = sklearn.linear_model.SGDClassifier
REAL_MULTI = sklearn.multioutput.MultiOutputClassifier
REAL_FIT = REAL_SGD.fit


def sgd_classifier(loss="hinge", **kw):
    return REAL_SGD(loss="log_loss" if loss == "log" else loss, **kw)


def recording_fit(self, X, y, **kw):
    out = REAL_FIT(self, X, y, **kw)
    FITTED.append(self)
    return out


def in_process_multi_output(estimator, n_jobs=None):
    return REAL_MULTI(estimator, n_jobs=None)


def load_reference(name):
    """Import eval_scripts/<name>.py of the reference; its module-level `networkx` import is not needed by run_regression."""
    if "networkx" not in sys.modules:
        try:
            import networkx.readwrite.json_graph  # noqa: F401
        except Exception:
            nx, rw = types.ModuleType("networkx"), types.ModuleType("networkx.readwrite")
            rw.json_graph = types.ModuleType("networkx.readwrite.json_graph")
            nx.readwrite = rw
            sys.modules.update({"networkx": nx, "networkx.readwrite": rw, "networkx.readwrite.json_graph": rw.json_graph})
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "eval_scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(mod, Xtr, ytr, Xte, yte):
    """(fitted SGD instances, printed text) of the reference's run_regression."""
    del FITTED[:]
    sklearn.linear_model.SGDClassifier, sklearn.multioutput.MultiOutputClassifier = sgd_classifier, in_process_multi_output
    REAL_SGD.fit = recording_fit
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            mod.run_regression(Xtr, ytr, Xte, yte)
    finally:
        sklearn.linear_model.SGDClassifier, sklearn.multioutput.MultiOutputClassifier = REAL_SGD, REAL_MULTI
        REAL_SGD.fit = REAL_FIT
    return list(FITTED), buf.getvalue()


def objective(X, s, w, b):
    m = s * (X.dot(w) + b)
    return (np.maximum(-m, 0) + np.log1p(np.exp(-np.abs(m)))).mean() + 0.5 * ALPHA * w.dot(w)


def optimum(X, s):
    """argmin of J_k in fp64 for one class: X [n, d] fp64, s [n] in {+1, -1}."""
    n, d = X.shape

    def grad(t):
        w, b = t[:d], t[d]
        m = s * (X.dot(w) + b)
        e = np.exp(-np.abs(m))
        sg = np.where(m >= 0, e, 1.0) / (1.0 + e)                 # sigma(-m)
        r = -s * sg / n
        return np.concatenate([X.T.dot(r) + ALPHA * w, [r.sum()]]), sg

    def f(t):
        return objective(X, s, t[:d], t[d]), grad(t)[0]

    t = so.minimize(f, np.zeros(d + 1), jac=True, method="L-BFGS-B",
                    options=dict(maxiter=50000, maxfun=100000, ftol=1e-16, gtol=1e-11, maxcor=30)).x
    Xa = np.hstack([X, np.ones((n, 1))])
    reg = np.diag(np.r_[np.full(d, ALPHA), 0.0])
    for _ in range(8):                                            # Newton on the exact Hessian
        g, sg = grad(t)
        H = (Xa * (sg * (1.0 - sg) / n)[:, None]).T.dot(Xa) + reg
        step = np.linalg.solve(H, g)
        if np.abs(grad(t - step)[0]).max() < np.abs(g).max():
            t = t - step
    assert np.abs(grad(t)[0]).max() < 1e-12, np.abs(grad(t)[0]).max()   # J - J* <= |g|^2 / (2 alpha)-ish: far below 1e-16
    return t[:d], t[d], objective(X, s, t[:d], t[d])


def embeddings(rng, n, d, c, multi):
    """Unit-norm rows whose labels come from a noisy linear model (not separable: the optimum is finite and interior)."""
    Wt = rng.randn(d, c) * 3
    X = rng.randn(n, d)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Z = X.dot(Wt) + rng.randn(n, c) * 0.6
    y = (Z > 0.3).astype(np.uint8) if multi else Z.argmax(axis=1).astype(np.int64)
    return X.astype(np.float32), y


def make(name, seed, n_train, n_test, d, c, multi):
    rng = np.random.RandomState(seed)
    X, y = embeddings(rng, n_train + n_test, d, c, multi)
    Xtr, ytr, Xte, yte = X[:n_train], y[:n_train], X[n_train:], y[n_train:]
    S = np.where(ytr > 0, 1.0, -1.0) if multi else np.where(ytr[:, None] == np.arange(c)[None, :], 1.0, -1.0)
    assert (np.abs(S.sum(axis=0)) < n_train).all(), "every class needs both targets in the train part"
    if multi:
        fitted, text = run_reference(load_reference("ppi_eval"), Xtr, ytr, Xte, yte)
        assert len(fitted) == c and all(list(m.classes_) == [0, 1] for m in fitted)
        coef = np.stack([m.coef_[0] for m in fitted], axis=1)
        icpt = np.array([m.intercept_[0] for m in fitted])
        f1 = [float(v) for v in re.findall(r"^F1 score ([0-9.eE+-]+)$", text, flags=re.M)]
        base = [float(v) for v in re.findall(r"^Random baseline F1 score ([0-9.eE+-]+)$", text, flags=re.M)]
        assert len(f1) == c and len(base) == c, text
        printed = {"ref_f1_test": np.array(f1), "ref_f1_baseline": np.array(base)}
    else:
        fitted, text = run_reference(load_reference("reddit_eval"), Xtr, list(ytr), Xte, list(yte))
        assert len(fitted) == 1 and list(fitted[0].classes_) == list(range(c))
        coef, icpt = fitted[0].coef_.T.copy(), fitted[0].intercept_.copy()
        nums = [float(v) for v in re.findall(r"^([0-9.eE+-]+)$", text, flags=re.M)]
        assert len(nums) == 3, text
        printed = {"ref_f1_test": np.array(nums[0]), "ref_f1_train": np.array(nums[1]), "ref_f1_baseline": np.array(nums[2])}
    X64 = Xtr.astype(np.float64)
    coef, icpt = coef.astype(np.float64), icpt.astype(np.float64)      # scikit-learn fits float32 rows in float32
    W_star, b_star, J_star, J_ref = np.zeros((d, c)), np.zeros(c), np.zeros(c), np.zeros(c)
    for k in range(c):
        W_star[:, k], b_star[k], J_star[k] = optimum(X64, S[:, k])
        J_ref[k] = objective(X64, S[:, k], coef[:, k], icpt[k])
    assert (J_ref >= J_star).all(), (J_ref - J_star)
    print(name, "J_ref - J_star per class:", " ".join("%.2e" % v for v in J_ref - J_star),
          "| printed:", {k: np.round(v, 4).tolist() for k, v in printed.items()})
    np.savez_compressed(os.path.join(HERE, name + ".npz"), X_train=Xtr, y_train=ytr, X_test=Xte, y_test=yte,
                        ref_coef=coef, ref_intercept=icpt, W_star=W_star, b_star=b_star, J_star=J_star, J_ref=J_ref,
                        alpha=np.array(ALPHA), **printed)


if __name__ == "__main__":
    make("ref_eval_multiclass", 11, 300, 120, 32, 4, False)
    make("ref_eval_multilabel", 12, 350, 120, 36, 7, True)
