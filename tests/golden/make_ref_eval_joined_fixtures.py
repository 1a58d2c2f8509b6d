"""Generate tests/golden/ref_eval_feat_multiclass.npz and ref_eval_both_multilabel.npz: the raw-feature (`feat`) and the
features + embeddings rows of the reference's eval_scripts, by EXECUTING THE REFERENCE'S OWN run_regression.

    GRAPHSAGE_REFERENCE=<reference tree> python tests/golden/make_ref_eval_joined_fixtures.py

The `__main__` blocks of eval_scripts/reddit_eval.py and ppi_eval.py, where the two inputs are put together, cannot run on a
current interpreter (Python 2 `iteritems`, networkx <= 1.11).  What they do to the rows before the regression is three lines,

    scaler = StandardScaler(); scaler.fit(train_rows); train_rows, test_rows = scaler.transform(train_rows), scaler.transform(test_rows)

on `feats` (reddit_eval.py:54-58, ppi_eval.py:66-70) or on `np.hstack([feats, embeds])` (reddit_eval.py:85-91,
citation_eval.py:83-89).  This generator RESTATES those three lines by calling scikit-learn's StandardScaler directly, on
fp64 copies of the fp32 inputs, and then runs the reference's UNMODIFIED run_regression on the result through the stand-ins
of make_ref_eval_fixtures.py (imported from there; nothing of the reference is copied into this repository).  Not part of the
suite; needs scikit-learn and scipy.

The feature width, 22, is no multiple of 4.  The raw feature columns have unequal scales (std 0.2 .. 30) and non-zero means
(|mean| <= 50); column 0 is count-like (non-negative integers with a long tail) and column 1 score-like with negative values;
the embeddings are unit rows.  Each file holds F_train / F_test (float32 [n, 22]), E_train / E_test (float32 [n, 32], the
`both` fixture only), y_train / y_test, the scaler's scaler_mean / scaler_scale over the joined columns, the reference's
ref_coef / ref_intercept and the F1 it PRINTED (ref_f1_*), alpha, and W_star, b_star, J_star, J_ref: the fp64 optimum of

    J_k(w, b) = 1/n sum_i log(1 + exp(-s_ik (<x_i, w> + b))) + alpha/2 |w|^2

on the STANDARDISED train rows x = (row - scaler_mean) / scaler_scale and the same objective at the reference's
coefficients.  The generator asserts J_ref >= J_star for every class and that no test row has a decision margin <= 1e-4
under (W_star, b_star); it walks the seeds from the given one until both hold.
"""
import os
import re
import sys

import numpy as np
from sklearn.preprocessing import StandardScaler

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_ref_eval_fixtures import ALPHA, load_reference, objective, optimum, run_reference  # noqa: E402

MARGIN = 1e-4
N_FEAT, N_EMB = 22, 32


def inputs(rng, n, c, multi, with_emb):
    """(F [n, 22] raw features, E [n, 32] unit rows or None, labels from a noisy linear model of the standardised columns)."""
    std = np.exp(rng.uniform(np.log(0.2), np.log(30.0), size=N_FEAT))
    mean = rng.uniform(-50.0, 50.0, size=N_FEAT)
    U = rng.randn(n, N_FEAT)                                      # the signal lives in these
    F = mean + std * U
    F[:, 0] = np.floor(np.exp(1.5 + 1.2 * U[:, 0]))               # counts: 0, 1, 2, .. with a long tail
    F[:, 1] = 8.0 * U[:, 1] - 3.0                                 # a score around -3: negative values
    cols = [U]
    E = None
    if with_emb:
        E = rng.randn(n, N_EMB)
        E /= np.linalg.norm(E, axis=1, keepdims=True)
        cols.append(E * np.sqrt(N_EMB))
    X = np.hstack(cols)
    Z = X.dot(rng.randn(X.shape[1], c)) * (3.0 / np.sqrt(X.shape[1])) + rng.randn(n, c) * 0.6
    y = (Z > 0.3).astype(np.uint8) if multi else Z.argmax(axis=1).astype(np.int64)
    return F.astype(np.float32), (E.astype(np.float32) if with_emb else None), y


def attempt(seed, n_train, n_test, c, multi, with_emb):
    rng = np.random.RandomState(seed)
    F, E, y = inputs(rng, n_train + n_test, c, multi, with_emb)
    rows = np.hstack([F, E]) if with_emb else F                   # np.hstack([feats, embeds])
    tr, te = rows[:n_train].astype(np.float64), rows[n_train:].astype(np.float64)
    ytr, yte = y[:n_train], y[n_train:]
    S = np.where(ytr > 0, 1.0, -1.0) if multi else np.where(ytr[:, None] == np.arange(c)[None, :], 1.0, -1.0)
    if not (np.abs(S.sum(axis=0)) < n_train).all():
        return None
    scaler = StandardScaler()                                     # the three lines of the reference's scripts
    scaler.fit(tr)
    Xtr, Xte = scaler.transform(tr), scaler.transform(te)
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
    coef, icpt = coef.astype(np.float64), icpt.astype(np.float64)
    d = Xtr.shape[1]
    W_star, b_star, J_star, J_ref = np.zeros((d, c)), np.zeros(c), np.zeros(c), np.zeros(c)
    for k in range(c):
        W_star[:, k], b_star[k], J_star[k] = optimum(Xtr, S[:, k])
        J_ref[k] = objective(Xtr, S[:, k], coef[:, k], icpt[k])
    z = Xte.dot(W_star) + b_star
    srt = np.sort(z, axis=1)
    margin = np.abs(z).min() if multi else (srt[:, -1] - srt[:, -2]).min()
    if not (J_ref >= J_star).all() or not margin > MARGIN:
        return None
    out = dict(F_train=F[:n_train], F_test=F[n_train:], y_train=ytr, y_test=yte, scaler_mean=scaler.mean_.copy(),
               scaler_scale=scaler.scale_.copy(), ref_coef=coef, ref_intercept=icpt, W_star=W_star, b_star=b_star, J_star=J_star,
               J_ref=J_ref, alpha=np.array(ALPHA), seed=np.array(seed), **printed)
    if with_emb:
        out.update(E_train=E[:n_train], E_test=E[n_train:])
    return out, margin


def make(name, seed, n_train, n_test, c, multi, with_emb):
    for s in range(seed, seed + 50):
        got = attempt(s, n_train, n_test, c, multi, with_emb)
        if got is not None:
            break
    else:
        raise SystemExit("%s: no seed in [%d, %d) gives J_ref >= J_star and a margin above %g" % (name, seed, seed + 50, MARGIN))
    out, margin = got
    assert (out["J_ref"] >= out["J_star"]).all() and margin > MARGIN
    print(name, "seed", s, "smallest test margin %.3e" % margin, "J_ref - J_star per class:",
          " ".join("%.2e" % v for v in out["J_ref"] - out["J_star"]),
          "| printed:", {k: np.round(v, 4).tolist() for k, v in out.items() if k.startswith("ref_f1")})
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)


if __name__ == "__main__":
    make("ref_eval_feat_multiclass", 21, 300, 120, 4, False, False)
    make("ref_eval_both_multilabel", 22, 350, 120, 7, True, True)
