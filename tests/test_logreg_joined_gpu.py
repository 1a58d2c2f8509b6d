"""gs_logreg_eval_joined, gs_col_moments and the classifier inputs built on them, on the device: fp64 parity of FIT and PREDICT
at the width, seam, y-block and row edges with an affine, bit-equality with gs_logreg_eval, repeatability, the column moments,
optimality of the standardised fit on the fixtures made from the reference's own run (tests/golden/ref_eval_feat_multiclass.npz,
ref_eval_both_multilabel.npz), and the --inputs / --eval_classifier_inputs flags of the two tools."""
import json
import os
import re

import numpy as np
import pytest
import torch

from graphsage_amd import evaluation as ev
from graphsage_amd import ops
from graphsage_amd.ops import Mat

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GARBAGE = 7.0e30            # what the pad columns hold: a kernel that reads one shows it
MARGIN = 1e-4


def tol(ref):
    """The project's float tolerance."""
    return 1e-4 * max(1.0, float(np.abs(ref).max()))


def padded(a, pad, dev, fill):
    """a [r, w] in a device buffer [r, round_up(w, 4) + pad] whose other columns hold `fill`."""
    r, w = a.shape
    buf = torch.full((r, ops.round_up(w, 4) + pad), fill, dtype=torch.from_numpy(a).dtype, device=dev)
    buf[:, :w] = torch.from_numpy(a).to(dev)
    return buf


def pick_rows(rng, mode, n, n_rows):
    if mode == "none":
        return None
    if mode == "perm":
        return rng.permutation(n_rows)[:n].astype(np.int32)
    return rng.randint(0, max(1, n_rows // 2), size=n).astype(np.int32)          # repeats, and not every row


class Case(object):
    """One joined problem: two tables with pad columns, two row vectors, an affine; the fp64 restatement of the same fp32
    inputs and the same fp32 mu and inv on the host.  affine: "none" | "rand" | "big" (column 3: mean 4096, std 1, mu = 4096,
    inv = 1 -- a folded scaler loses it) | "const" (column 5 is 2.5 everywhere, mu = 2.5, inv = 1: exact zeros)."""

    def __init__(self, dev, n, da, db, c, multi, rows_a="none", rows_b="none", lda_pad=0, ldb_pad=0, ldw_pad=0, affine="rand", seed=0):
        rng = np.random.RandomState(seed + 1000 * n + 10 * da + 7 * db + c)
        d = da + db
        na = n if rows_a == "none" else n + 9
        nb = n if rows_b == "none" else n + 5
        col_mean, col_std = rng.randn(d) * 0.5, np.exp(rng.uniform(-0.7, 0.7, size=d))
        A = (col_mean[:da] + col_std[:da] * rng.randn(na, da)).astype(np.float32)
        B = (col_mean[da:] + col_std[da:] * rng.randn(nb, db)).astype(np.float32) if db else None
        mu, inv = col_mean.astype(np.float32), (1.0 / col_std).astype(np.float32)
        if affine == "big":
            A[:, 3] = (4096.0 + rng.randn(na)).astype(np.float32)
            mu[3], inv[3] = 4096.0, 1.0
        if affine == "const":
            A[:, 5] = 2.5
            mu[5], inv[5] = 2.5, 1.0
        ia, ib = pick_rows(rng, rows_a, n, na), (pick_rows(rng, rows_b, n, nb) if db else None)
        X = A[ia] if ia is not None else A[:n]
        if db:
            X = np.hstack([X, B[ib] if ib is not None else B[:n]])
        X = X.astype(np.float64)
        if affine != "none":
            X = (X - mu.astype(np.float64)) * inv.astype(np.float64)
        W = (rng.randn(d, c) / np.sqrt(d)).astype(np.float32)
        b = (rng.randn(c) * 0.5).astype(np.float32)
        z = X.dot(W.astype(np.float64)) + b.astype(np.float64)
        noise = z + rng.randn(n, c)
        y = (noise > 0).astype(np.uint8) if multi else noise.argmax(axis=1).astype(np.int32)
        S = ev.targets(y, None if multi else c)[0]
        m = S * z
        e = np.exp(-np.abs(m))
        r = -S * np.where(m >= 0, e, 1.0) / (1.0 + e)
        self.n, self.da, self.db, self.d, self.c, self.multi, self.z, self.X64 = n, da, db, d, c, multi, z, X
        self.loss = (np.maximum(-m, 0.0) + np.log1p(e)).sum(axis=0)
        self.gW, self.gb = X.T.dot(r), r.sum(axis=0)
        self.Xa = Mat(padded(A, lda_pad, dev, GARBAGE), da)
        self.Xb = Mat(padded(B, ldb_pad, dev, GARBAGE), db) if db else None
        self.W = Mat(padded(W, ldw_pad, dev, GARBAGE), c)
        self.b = torch.from_numpy(b).to(dev)
        self.rows_a = torch.from_numpy(ia).to(dev) if ia is not None else None
        self.rows_b = torch.from_numpy(ib).to(dev) if ib is not None else None
        self.mu = torch.from_numpy(mu).to(dev) if affine != "none" else None
        self.inv = torch.from_numpy(inv).to(dev) if affine != "none" else None
        self.y_class = None if multi else torch.from_numpy(y).to(dev)
        self.y_multi = padded(y, 3, dev, 1)[:, :c + 3] if multi else None

    def kw(self):
        return dict(Xb=self.Xb, n=self.n, rows_a=self.rows_a, rows_b=self.rows_b, mu=self.mu, inv=self.inv)

    def labels(self):
        return dict(y_class=self.y_class, y_multi=self.y_multi)

    def fit(self):
        return ops.logreg_eval_joined(self.Xa, self.W, self.b, mode=ops.LOGREG_FIT, **dict(self.kw(), **self.labels()))

    def check(self):
        dev = self.b.device
        n, c = self.n, self.c
        out = [t.cpu().numpy() for t in self.fit()]
        for name, got, ref in (("loss", out[0], self.loss), ("gW", out[1], self.gW), ("gb", out[2], self.gb)):
            err = float(np.abs(got - ref).max())
            print("%s n=%d d=%d+%d c=%d: max err %.3e of tol %.3e" % (name, n, self.da, self.db, c, err, tol(ref)))
            assert got.shape == ref.shape and np.isfinite(got).all() and err <= tol(ref), (name, err, tol(ref))
        # PREDICT into buffers longer than n: n entries are written and no more
        pc_buf = torch.full((n + 40,), -7, dtype=torch.int32, device=dev)
        pm_buf = torch.full((n + 40, c + 3), 9, dtype=torch.uint8, device=dev)
        ploss = torch.zeros(c, dtype=torch.float64, device=dev)
        ops.logreg_eval_joined(self.Xa, self.W, self.b, mode=ops.LOGREG_PREDICT, loss=ploss, pred_class=pc_buf[:n],
                               pred_multi=pm_buf[:n], **dict(self.kw(), **self.labels()))
        assert float(np.abs(ploss.cpu().numpy() - self.loss).max()) <= tol(self.loss)
        pm, pc = pm_buf.cpu().numpy(), pc_buf.cpu().numpy()
        assert (pm[n:] == 9).all() and (pm[:, c:] == 9).all() and (pc[n:] == -7).all()
        sure = np.abs(self.z) > MARGIN
        assert np.array_equal(pm[:n, :c][sure], (self.z > 0).astype(np.uint8)[sure]) and (~sure).mean() <= 0.01
        assert ((pc[:n] >= 0) & (pc[:n] < c)).all()
        srt = np.sort(self.z, axis=1)
        sure = srt[:, -1] - srt[:, -2] > MARGIN
        assert np.array_equal(pc[:n][sure], self.z.argmax(axis=1)[sure]) and (~sure).mean() <= 0.01
        return out


# ------------------------------------------------------------------------------------------------ 1. kernel parity
# one factor at a time around n = 70, da = 36, db = 0, c = 5
MULTI = pytest.mark.parametrize("multi", [False, True], ids=["class", "multi"])


@MULTI
@pytest.mark.parametrize("d", [36, 516, 544, 604, 860, 1020, 1024])
def test_parity_widths(dev, d, multi):
    """516: the first width beyond gs_logreg_eval's; 544: 17 d blocks, the 8-tile template with one y block; 1024: the limit."""
    Case(dev, 70, d, 0, 5, multi).check()


@MULTI
@pytest.mark.parametrize("da,db", [(4, 4), (36, 32), (604, 256), (28, 996), (1020, 4)])
def test_parity_seams(dev, da, db, multi):
    """(36, 32): the seam inside a 32-column block; (604, 256): features + embeddings at the Reddit widths."""
    Case(dev, 70, da, db, 5, multi).check()


@MULTI
@pytest.mark.parametrize("da,db,c", [(1024, 0, 128), (1024, 0, 33), (604, 420, 128)])
def test_parity_y_blocks(dev, da, db, c, multi):
    """ceil(c / 32) * ceil(d / 32) > 32: the d blocks are cut over four (c = 128) and two (c = 33) workgroups along y."""
    Case(dev, 70, da, db, c, multi).check()


@MULTI
@pytest.mark.parametrize("n", [1, 32, 33, 20000])
def test_parity_rows(dev, n, multi):
    Case(dev, n, 36, 32, 5, multi).check()


@MULTI
@pytest.mark.parametrize("kw", [dict(rows_a="perm", rows_b="perm"), dict(rows_a="repeat", rows_b="repeat"),
                                dict(rows_a="none", rows_b="perm"), dict(rows_a="repeat", rows_b="none"),
                                dict(lda_pad=8), dict(ldb_pad=12), dict(lda_pad=4, ldb_pad=8, ldw_pad=4, rows_a="perm", rows_b="repeat")],
                         ids=lambda kw: "-".join("%s=%s" % kv for kv in sorted(kw.items())))
def test_parity_rows_and_layouts(dev, kw, multi):
    """rows_a and rows_b are independent: two different permutations (the seeds differ by draw), repeats, each null."""
    Case(dev, 70, 36, 32, 5, multi, **kw).check()
    Case(dev, 20000, 36, 32, 33, multi, **kw).check()


@MULTI
@pytest.mark.parametrize("db", [0, 32])
def test_parity_affine_columns(dev, db, multi):
    """A column with mean 4096 and std 1: x - mu is exact in fp32, so the staged form keeps every digit; a scaler folded into W
    and b (or an fma with -mu * inv) is off by about 4096 * 2^-24 * |w| * n in gW.  A constant column: exact zeros."""
    Case(dev, 70, 36, db, 5, multi, affine="big").check()
    case = Case(dev, 70, 36, db, 5, multi, affine="const")
    assert np.array_equal(case.X64[:, 5], np.zeros(70))
    loss, gW, gb = case.check()
    assert np.array_equal(gW[5], np.zeros(5))
    Case(dev, 70, 36, db, 5, multi, affine="none").check()


@MULTI
def test_parity_pad_rows(dev, multi):
    """n = 33: the second tile holds one row and 31 pad rows, which are zeros after the affine (mu != 0 here)."""
    case = Case(dev, 33, 36, 32, 5, multi)
    assert float(np.abs(case.mu.cpu().numpy()).min()) > 0
    case.check()


def test_wrapper_refuses_bad_arguments(dev):
    case = Case(dev, 70, 36, 32, 5, False)
    E = ops._lib.GraphsageAmdError
    with pytest.raises(E, match="rows_b"):
        ops.logreg_eval_joined(case.Xa, case.W, case.b, Xb=case.Xb, n=70, rows_b=torch.zeros(70, dtype=torch.int64, device=dev),
                               y_class=case.y_class)
    with pytest.raises(E, match="mu must be"):
        ops.logreg_eval_joined(case.Xa, case.W, case.b, Xb=case.Xb, n=70, mu=case.mu[:8], inv=case.inv, y_class=case.y_class)
    with pytest.raises(E, match="mu and inv"):
        ops.logreg_eval_joined(case.Xa, case.W, case.b, Xb=case.Xb, n=70, mu=case.mu, y_class=case.y_class)
    with pytest.raises(E, match="joined width"):
        ops.logreg_eval_joined(case.Xa, case.W, case.b, n=70, y_class=case.y_class)
    with pytest.raises(E, match="without rows_b"):
        ops.logreg_eval_joined(case.Xa, case.W, case.b, Xb=Mat(case.Xb.buf[:60], 32), n=70, y_class=case.y_class)
    with pytest.raises(ValueError, match=r"rows must lie in \[0, 70\)"):
        ev.fit_classifier(None, None, None, np.array([0, 1]), features=case.Xa, feature_rows=np.array([0, 70]))
    with pytest.raises(ValueError, match="same number of rows"):
        ev.fit_classifier(None, case.Xb, np.array([0, 1, 2]), np.array([0, 1]), features=case.Xa, feature_rows=np.array([0, 1]))


# ------------------------------------------------------------------------------------------------ 2. bit-equality, repeatability
def bits(t):
    a = t.cpu().numpy()
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]).copy()


@pytest.mark.parametrize("multi", [False, True], ids=["class", "multi"])
@pytest.mark.parametrize("n,d,c", [(70, 36, 5), (20000, 36, 33), (150, 512, 128)])
def test_bit_equal_to_logreg_eval(dev, n, d, c, multi):
    """One source, no affine, d <= 512: every output of FIT and PREDICT carries gs_logreg_eval's bits."""
    case = Case(dev, n, d, 0, c, multi, rows_a="repeat", lda_pad=4, affine="none")
    old = ops.logreg_eval(case.Xa, case.W, case.b, n=n, rows=case.rows_a, mode=ops.LOGREG_FIT, **case.labels())
    new = case.fit()
    for a, b in zip(old, new):
        assert np.array_equal(bits(a), bits(b))
    outs = []
    for fn, kw in ((ops.logreg_eval, dict(rows=case.rows_a)), (ops.logreg_eval_joined, dict(rows_a=case.rows_a))):
        pc = torch.full((n,), -7, dtype=torch.int32, device=dev)
        pm = torch.full((n, c), 9, dtype=torch.uint8, device=dev)
        pl = torch.zeros(c, dtype=torch.float64, device=dev)
        fn(case.Xa, case.W, case.b, n=n, mode=ops.LOGREG_PREDICT, loss=pl, pred_class=pc, pred_multi=pm, **dict(kw, **case.labels()))
        outs.append((bits(pc), bits(pm), bits(pl)))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n,da,db,c", [(70, 36, 32, 5), (150, 604, 256, 41)])
def test_same_call_twice_same_bits(dev, n, da, db, c):
    case = Case(dev, n, da, db, c, False, rows_a="repeat", rows_b="perm")
    a = [bits(t) for t in case.fit()]
    b = [bits(t) for t in case.fit()]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------ 3. column moments
@pytest.mark.parametrize("da,db", [(36, 0), (604, 256)])
@pytest.mark.parametrize("n", [1, 33, 20000])
def test_col_moments(dev, n, da, db):
    """Against a two-pass fp64 NumPy restatement.  An fp64 sum of <= 2^15 fp32 terms is off by at most n * 2^-53 = 4e-12
    relative: 1e-9 of max(1, max |x|) for the mean and of its square for the variance leaves more than 100 x."""
    rng = np.random.RandomState(n + da + db)
    d = da + db
    na, nb = n + 11, n + 3
    col_mean, col_std = rng.uniform(-50, 50, size=d), np.exp(rng.uniform(np.log(0.2), np.log(30.0), size=d))
    A = (col_mean[:da] + col_std[:da] * rng.randn(na, da)).astype(np.float32)
    A[:, 7] = np.float32(3.7)                                                    # constant columns: var == 0.0 exactly
    A[:, 0] = np.float32(-1234.5678)
    B = None
    if db:
        B = (col_mean[da:] + col_std[da:] * rng.randn(nb, db)).astype(np.float32)
        B[:, 9] = np.float32(1e-3)
    ia, ib = pick_rows(rng, "repeat", n, na), (pick_rows(rng, "repeat", n, nb) if db else None)
    X = np.hstack([A[ia]] + ([B[ib]] if db else [])).astype(np.float64)
    mean_ref = X.mean(axis=0)
    var_ref = ((X - mean_ref) ** 2).mean(axis=0)
    Xa, Xb = Mat(padded(A, 8, dev, GARBAGE), da), (Mat(padded(B, 4, dev, GARBAGE), db) if db else None)
    kw = dict(Xb=Xb, n=n, rows_a=torch.from_numpy(ia).to(dev), rows_b=torch.from_numpy(ib).to(dev) if db else None)
    mean, var = [t.cpu().numpy().copy() for t in ops.col_moments(Xa, **kw)]
    big = max(1.0, float(np.abs(X).max()))
    print("n=%d d=%d+%d: mean err %.3e of %.3e, var err %.3e of %.3e" % (
        n, da, db, np.abs(mean - mean_ref).max(), 1e-9 * big, np.abs(var - var_ref).max(), 1e-9 * big * big))
    assert mean.dtype == np.float64 and mean.shape == (d,) and var.shape == (d,)
    assert np.abs(mean - mean_ref).max() <= 1e-9 * big and np.abs(var - var_ref).max() <= 1e-9 * big * big
    assert (var >= 0).all()
    const = [0, 7] + ([da + 9] if db else [])
    assert (var[const] == 0.0).all() and mean[7] == np.float64(np.float32(3.7)) and mean[0] == np.float64(np.float32(-1234.5678))
    if n == 1:
        assert (var == 0.0).all() and np.array_equal(mean, X[0])
    mean2, var2 = [t.cpu().numpy() for t in ops.col_moments(Xa, **kw)]
    assert np.array_equal(mean.view(np.int64), mean2.view(np.int64)) and np.array_equal(var.view(np.int64), var2.view(np.int64))


# ------------------------------------------------------------------------------------------------ 4. optimality on the fixtures
FIXTURES = ("ref_eval_feat_multiclass", "ref_eval_both_multilabel")
_FITS = {}


def fit_fixture(fx):
    multi = fx["y_train"].ndim == 2
    return ev.fit_classifier(None, fx.get("E_train"), None, fx["y_train"], n_classes=None if multi else fx["W_star"].shape[1],
                             features=fx["F_train"], standardize=True)


def fitted(dev, name):
    """The fixture, its targets and ONE device fit with the defaults, shared by the tests below."""
    if name not in _FITS:
        fx = dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))
        multi = fx["y_train"].ndim == 2
        _FITS[name] = (fx, ev.targets(fx["y_train"], None if multi else fx["W_star"].shape[1])[0], fit_fixture(fx))
    return _FITS[name]


def standardised(fx, part):
    cols = [fx["F_" + part]] + ([fx["E_" + part]] if "E_" + part in fx else [])
    return (np.hstack(cols).astype(np.float64) - fx["scaler_mean"]) / fx["scaler_scale"]


@pytest.mark.parametrize("name", FIXTURES)
def test_fit_against_reference_and_optimum(dev, name):
    """The scaler is scikit-learn's to 1e-6 relative; per class, with the objective re-evaluated in fp64 on the fixture's
    standardised rows: (a) not above the reference's SGD (convexity: no margin), (b) within 1e-4 relative of the fp64 optimum,
    (c) predictions on the test part equal to the optimum's wherever its fp64 margin exceeds 1e-4 (at most 1 % left out)."""
    fx, S, clf = fitted(dev, name)
    multi = fx["y_train"].ndim == 2
    d = fx["W_star"].shape[0]
    assert clf.mean.dtype == np.float64 and clf.mean.shape == (d,) and clf.scale.shape == (d,) and clf.W.shape == fx["W_star"].shape
    assert clf.widths == [22, 32 if "E_train" in fx else None]
    assert np.allclose(clf.mean, fx["scaler_mean"], rtol=1e-6, atol=0) and np.allclose(clf.scale, fx["scaler_scale"], rtol=1e-6, atol=0)
    assert clf.stop in ("gtol", "noise") and 1 < clf.evals <= 1000
    J = ev.objective(standardised(fx, "train"), S, clf.W, clf.b)
    gap = (J - fx["J_star"]) / fx["J_star"]
    E_test = fx.get("E_test")
    score = clf.score(E_test, None, fx["y_test"], features=fx["F_test"])
    msg = "%s: evals %d stop %s, J - J* rel %s, J_ref - J %s; device f1_micro %.4f | reference printed %s" % (
        name, clf.evals, clf.stop, gap, fx["J_ref"] - J, score["f1_micro"], fx["ref_f1_test"])
    print(msg)
    assert (J <= fx["J_ref"]).all(), msg                                   # (a)
    assert (J - fx["J_star"] <= 1e-4 * fx["J_star"]).all(), msg            # (b)
    z = standardised(fx, "test").dot(fx["W_star"]) + fx["b_star"]          # (c)
    pred = clf.predict(E_test, features=fx["F_test"])
    if multi:
        sure = np.abs(z) > MARGIN
        assert pred.shape == z.shape and np.array_equal(pred[sure], (z > 0).astype(np.uint8)[sure]), msg
    else:
        srt = np.sort(z, axis=1)
        sure = srt[:, -1] - srt[:, -2] > MARGIN
        assert pred.shape == (z.shape[0],) and np.array_equal(pred[sure], z.argmax(axis=1)[sure]), msg
    assert sure.all() and (~sure).mean() <= 0.01, msg                      # the generator's guarantee: none is left out
    assert np.array_equal(score["pred"], pred)


@pytest.mark.parametrize("name", FIXTURES)
def test_fit_twice_same_bits(dev, name):
    fx, S, clf = fitted(dev, name)
    again = fit_fixture(fx)
    assert np.array_equal(clf.W.view(np.int32), again.W.view(np.int32)) and np.array_equal(clf.b.view(np.int32), again.b.view(np.int32))
    assert np.array_equal(clf.mean.view(np.int64), again.mean.view(np.int64))
    assert np.array_equal(clf.scale.view(np.int64), again.scale.view(np.int64))
    assert np.array_equal(clf.loss.view(np.int64), again.loss.view(np.int64)) and (clf.evals, clf.stop) == (again.evals, again.stop)


def test_scaler_is_fitted_on_the_train_rows_and_applied_to_other_tables(dev):
    """fit on rows of two larger tables == fit on the gathered rows, bit for bit; predict takes other tables (the n2v case:
    fit on [feats | val.npy], score on [feats | val-test.npy]) and applies the TRAIN scaler to them."""
    fx, S, clf = fitted(dev, "ref_eval_both_multilabel")
    n = fx["F_train"].shape[0]
    rng = np.random.RandomState(5)
    F = (rng.randn(n + 40, 22) * 100).astype(np.float32)                 # other rows would move every mean
    E = rng.randn(n + 25, 32).astype(np.float32)
    rf, re_ = rng.permutation(n + 40)[:n], rng.permutation(n + 25)[:n]
    F[rf], E[re_] = fx["F_train"], fx["E_train"]
    via = ev.fit_classifier(None, E, re_, fx["y_train"], features=F, feature_rows=rf, standardize=True)
    assert np.array_equal(via.mean.view(np.int64), clf.mean.view(np.int64)) and np.array_equal(via.W.view(np.int32), clf.W.view(np.int32))
    want = clf.predict(fx["E_test"], features=fx["F_test"])
    m = fx["F_test"].shape[0]
    order = rng.permutation(m)
    got = via.predict(fx["E_test"][order], np.argsort(order), features=F_with(F, fx["F_test"]), feature_rows=np.arange(n + 40, n + 40 + m))
    assert np.array_equal(got, want)
    # without standardize nothing is scaled and no scaler is kept; features alone
    raw = ev.fit_classifier(None, None, None, fx["y_train"], features=fx["F_train"], max_evals=30)
    assert raw.mean is None and raw.scale is None and raw.W.shape == (22, 7) and raw.widths == [22, None]
    with pytest.raises(ValueError, match="fitted on"):
        clf.predict(None, features=fx["F_test"])


def F_with(F, extra):
    return np.vstack([F, extra])


# ------------------------------------------------------------------------------------------------ 5. interfaces
def write_toy(tmp_path, rng):
    """A 90-node dataset: 3 classes, 60 / 10 / 20 split, 6 raw feature columns -- 0 count-like, 1 score-like with negative
    values, 2 and 3 carry the class at means 1000 and -500 (no classifier finds it there without the scaler), 4 and 5 noise."""
    n, c = 90, 3
    ids = ["n%d" % i for i in range(n)]
    cls = rng.randint(0, c, size=n)
    split = np.array(["train"] * 60 + ["val"] * 10 + ["test"] * 20)
    nodes = [{"id": ids[i], "val": bool(split[i] == "val"), "test": bool(split[i] == "test")} for i in range(n)]
    links = [{"source": int(a), "target": int(b)} for a, b in rng.randint(0, n, size=(150, 2)) if a != b]
    prefix = str(tmp_path / "toy")
    json.dump({"directed": False, "graph": {}, "nodes": nodes, "links": links, "multigraph": False}, open(prefix + "-G.json", "w"))
    json.dump({ids[i]: i for i in range(n)}, open(prefix + "-id_map.json", "w"))
    json.dump({ids[i]: int(cls[i]) for i in range(n)}, open(prefix + "-class_map.json", "w"))
    centers = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0]])
    feats = np.zeros((n, 6))
    feats[:, 0] = np.floor(np.exp(1.0 + rng.randn(n)))
    feats[:, 1] = rng.uniform(-0.9, 6.0, size=n)
    feats[:, 2] = 1000.0 + centers[cls, 0] + 0.2 * rng.randn(n)
    feats[:, 3] = -500.0 + centers[cls, 1] + 0.2 * rng.randn(n)
    feats[:, 4:] = rng.randn(n, 2) * [0.3, 20.0]
    np.save(prefix + "-feats.npy", feats.astype(np.float32))
    return prefix, ids


def test_eval_embeddings_inputs(dev, tmp_path, capsys):
    from graphsage_amd import eval_embeddings as ee
    rng = np.random.RandomState(3)
    prefix, ids = write_toy(tmp_path, rng)
    empty = tmp_path / "empty"                                            # --inputs features reads no embedding file
    empty.mkdir()
    emb_dir = tmp_path / "emb"
    emb_dir.mkdir()
    order = rng.permutation(90)
    emb = rng.randn(90, 8).astype(np.float32)                             # noise: the score comes from the features
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    np.save(str(emb_dir / "val.npy"), emb[order])
    open(str(emb_dir / "val.txt"), "w").write("\n".join(ids[i] for i in order))
    for inputs, out, width, prefix_word, fname in (("features", empty, 6, "Downstream classifier (features):", "eval_classifier_features.txt"),
                                                   ("both", emb_dir, 14, "Downstream classifier (features+embeddings):",
                                                    "eval_classifier_both.txt")):
        for extra in ([], ["--log_counts"]):
            res = ee.main([prefix, str(out), "test", "--inputs", inputs] + extra)
            lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Downstream classifier")]
            assert len(lines) == 1 and lines[0].startswith(prefix_word + " setting= test classes= 3 train= 60 test= 20 f1_micro= 1.00000 ")
            assert re.search(r" stop= (gtol|noise) width= %d time= \d+\.\d{5}$" % width, lines[0]), lines[0]
            assert open(str(out / fname)).read() == lines[0] + "\n" and sorted(os.listdir(str(empty))) in ([], ["eval_classifier_features.txt"])
            assert res["train_f1_micro"] == 1.0 and res["width"] == width
            clf = res["classifier"]
            assert abs(clf.mean[2] - 1000.0) < 2.0 and abs(clf.mean[3] + 500.0) < 2.0 and clf.mean.shape == (width,)
            if extra:
                assert clf.mean[0] < 3.0 and clf.mean[1] < np.log(7.0)       # the two columns were transformed before the scaler
    # the embeddings alone are noise here: the default inputs score below the features', and write the old file only
    res = ee.main([prefix, str(emb_dir), "test"])
    assert res["f1_micro"] < 1.0 and "width" not in res and os.path.exists(str(emb_dir / "eval_classifier.txt"))
    capsys.readouterr()


def test_unsupervised_driver_eval_classifier_inputs(dev, tmp_path):
    """--eval_classifier test --eval_classifier_inputs all: one line of each of the three kinds, the three files hold them, the
    embeddings line is the one a run without the new flag prints (time= aside), and no other output file appears or goes.
    Two child processes, started together (tests/test_logreg_gpu.py: a second main() in this process is no rerun)."""
    import subprocess
    import sys
    args = ["--synthetic", "small", "--epochs", "1", "--batch_size", "128", "--samples_1", "5", "--samples_2", "3", "--dim_1", "32",
            "--dim_2", "32", "--max_total_steps", "6", "--model", "graphsage_mean", "--learning_rate", "0.001",
            "--max_walk_pairs", "4000", "--validate_iter", "10", "--validate_batch_size", "256", "--eval_classifier", "test"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    extra = {"all": ["--eval_classifier_inputs", "all"], "plain": []}
    procs = {run: subprocess.Popen([sys.executable, "-m", "graphsage_amd.unsupervised_train"] + args + extra[run]
                                   + ["--base_log_dir", str(tmp_path / run)], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                   stderr=subprocess.PIPE, universal_newlines=True) for run in ("all", "plain")}
    outs, files = {}, {}
    for run, proc in procs.items():
        out, err = proc.communicate(timeout=300)
        assert proc.returncode == 0, err[-2000:]
        outs[run] = out
        files[run] = {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path / run)) for f in fs}
    kinds = {"eval_classifier.txt": r"^Downstream classifier: .*$", "eval_classifier_features.txt": r"^Downstream classifier \(features\): .*$",
             "eval_classifier_both.txt": r"^Downstream classifier \(features\+embeddings\): .*$"}
    lines = {}
    for fname, pat in kinds.items():
        found = re.findall(pat, outs["all"], flags=re.M)
        assert len(found) == 1, outs["all"][-2000:]
        lines[fname] = found[0]
        assert open(files["all"][fname]).read() == found[0] + "\n"
    assert len(re.findall(r"^Downstream classifier", outs["all"], flags=re.M)) == 3
    assert outs["all"].index(lines["eval_classifier.txt"]) < outs["all"].index(lines["eval_classifier_features.txt"]) \
        < outs["all"].index(lines["eval_classifier_both.txt"])
    fields = (r" setting= test classes= 7 train= (\d+) test= (\d+) f1_micro= (\d\.\d{5}) f1_macro= (\d\.\d{5}) train_f1_micro= (\d\.\d{5}) "
              r"baseline_f1_micro= (\d\.\d{5}) loss= (\d+\.\d{6}) evals= (\d+) stop= (gtol|noise|max_evals)")
    m = {f: re.match(re.escape(ev.LINE_PREFIX[k]) + fields + (r" width= (\d+)" if k != "embeddings" else "") + r" time= (\d+\.\d{5})$", lines[f])
         for k, f in ev.LINE_FILE.items()}
    assert all(m.values()), lines
    assert int(m["eval_classifier_features.txt"].group(10)) == 50 and int(m["eval_classifier_both.txt"].group(10)) == 50 + 64
    assert len({(x.group(1), x.group(2), x.group(6)) for x in m.values()}) == 1            # the same rows, the same baseline
    plain = re.findall(kinds["eval_classifier.txt"], outs["plain"], flags=re.M)
    assert len(plain) == 1 and len(re.findall(r"^Downstream classifier", outs["plain"], flags=re.M)) == 1
    strip = lambda s: re.sub(r" time= \S+$", "", s)
    assert strip(plain[0]) == strip(lines["eval_classifier.txt"])
    assert set(files["all"]) - {"eval_classifier_features.txt", "eval_classifier_both.txt"} == set(files["plain"])
