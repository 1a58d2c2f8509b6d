"""Host side of the downstream classifier (no GPU): the L-BFGS solver of graphsage_amd/evaluation.py driven by an fp64 NumPy
evaluator against the fp64 optimum stored with the reference's own run (tests/golden/ref_eval_*.npz, made by
make_ref_eval_fixtures.py), its stop reasons, the refusals and flags of the drivers, the C ABI of gs_logreg_eval."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("ref_eval_multiclass", "ref_eval_multilabel")


def load_fixture(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))


def fixture_targets(fx):
    from graphsage_amd import evaluation as ev
    y = fx["y_train"]
    return ev.targets(y, None if y.ndim == 2 else fx["W_star"].shape[1])[0]


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_contents(name):
    """Unit-norm rows, >= 3 classes / >= 7 labels, a train and a test part, the reference's coefficients and printed F1, and an
    optimum that the reference's SGD does not beat in any class (recomputed here, not read)."""
    from graphsage_amd import evaluation as ev
    fx = load_fixture(name)
    X, S = fx["X_train"], fixture_targets(fx)
    assert X.dtype == np.float32 and np.allclose(np.linalg.norm(X.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert fx["X_test"].shape[0] > 0 and fx["X_test"].shape[1] == X.shape[1]
    c = S.shape[1]
    assert c >= (7 if fx["y_train"].ndim == 2 else 3)
    assert fx["ref_coef"].shape == (X.shape[1], c) and fx["ref_intercept"].shape == (c,) and fx["ref_f1_test"].size >= 1
    J_star = ev.objective(X, S, fx["W_star"], fx["b_star"], float(fx["alpha"]))
    J_ref = ev.objective(X, S, fx["ref_coef"], fx["ref_intercept"], float(fx["alpha"]))
    # two orders of summing ~400 fp64 terms differ by at most ~400 * 2^-53 = 5e-14 relative
    assert np.allclose(J_star, fx["J_star"], rtol=1e-12, atol=0) and np.allclose(J_ref, fx["J_ref"], rtol=1e-12, atol=0)
    assert (J_ref >= J_star).all() and float(fx["alpha"]) == ev.ALPHA == 1e-4


# ------------------------------------------------------------------------------------------------ solver
@pytest.mark.parametrize("name", FIXTURES)
def test_solver_reaches_the_fp64_optimum(name):
    """L-BFGS on an fp64 evaluator: every class's objective within 1e-9 relative of J*, from zero, without a random number."""
    from graphsage_amd import evaluation as ev
    fx = load_fixture(name)
    X, S = fx["X_train"], fixture_targets(fx)
    n, d = X.shape
    c = S.shape[1]
    state = np.random.get_state()[1].copy()
    W, b, J, evals, stop = ev.lbfgs(ev.numpy_evaluator(X, S), n, d, c, gtol=1e-9, max_evals=5000)
    assert np.array_equal(np.random.get_state()[1], state)
    assert stop in ("gtol", "noise") and evals < 5000
    J64 = ev.objective(X, S, W, b)
    print(name, "evals", evals, "stop", stop, "max rel gap", ((J64 - fx["J_star"]) / fx["J_star"]).max())
    assert np.allclose(J, J64, rtol=1e-12, atol=0)
    assert (J64 - fx["J_star"] <= 1e-9 * fx["J_star"]).all(), (J64 - fx["J_star"]) / fx["J_star"]
    assert (J64 <= fx["J_ref"]).all()
    W2, b2, J2, evals2, stop2 = ev.lbfgs(ev.numpy_evaluator(X, S), n, d, c, gtol=1e-9, max_evals=5000)
    assert np.array_equal(W, W2) and np.array_equal(b, b2) and (evals, stop) == (evals2, stop2)


def test_stop_semantics():
    from graphsage_amd import evaluation as ev
    fx = load_fixture("ref_eval_multiclass")
    X, S = fx["X_train"], fixture_targets(fx)
    n, d = X.shape
    c = S.shape[1]
    exact = ev.numpy_evaluator(X, S)
    # gtol: the returned point's gradient is below it
    W, b, J, evals, stop = ev.lbfgs(exact, n, d, c, gtol=1e-4)
    loss, gW, gb = exact(W, b)
    assert stop == "gtol" and max(np.abs(gW / n + ev.ALPHA * W).max(), np.abs(gb / n).max()) <= 1e-4
    # already there: a gtol above the gradient at zero costs one evaluation
    assert ev.lbfgs(exact, n, d, c, gtol=10.0)[3:] == (1, "gtol")
    # max_evals: the budget is never exceeded, and what comes back is the best point seen (below the start)
    W3, b3, J3, evals3, stop3 = ev.lbfgs(exact, n, d, c, gtol=1e-12, max_evals=7)
    assert stop3 == "max_evals" and evals3 <= 7 and J3.sum() < c * np.log(2.0)
    # noise: an evaluator rounded to fp32 cannot be driven to gtol = 1e-12; the line search runs dry instead
    calls = [0]

    def rounded(W_, b_):
        calls[0] += 1
        l, gw, gb_ = exact(W_.astype(np.float32), b_.astype(np.float32))
        return l.astype(np.float32), gw.astype(np.float32), gb_.astype(np.float32)

    W4, b4, J4, evals4, stop4 = ev.lbfgs(rounded, n, d, c, gtol=1e-12, max_evals=4000)
    assert stop4 == "noise" and evals4 == calls[0] < 4000
    J64 = ev.objective(X, S, W4, b4)
    assert (J64 - fx["J_star"] <= 1e-4 * fx["J_star"]).all()


# ------------------------------------------------------------------------------------------------ host helpers
def test_targets_baseline_and_line():
    from graphsage_amd import evaluation as ev
    S, multi = ev.targets(np.array([2, 0, 1]), 4)
    assert not multi and np.array_equal(S, [[-1, -1, 1, -1], [1, -1, -1, -1], [-1, 1, -1, -1]])
    S, multi = ev.targets(np.array([[1, 0], [0, 0]], dtype=np.uint8))
    assert multi and np.array_equal(S, [[1, -1], [-1, -1]])
    # most frequent class 1: two of four test rows carry it
    assert ev.baseline_f1_micro(np.array([1, 1, 0, 2]), np.array([1, 0, 1, 2])) == 0.5
    # most frequent value per label: label 0 mostly on, label 1 mostly off -> tp = 1, fp = 1, fn = 1
    tr = np.array([[1, 0], [1, 0], [1, 1]], dtype=np.uint8)
    assert ev.baseline_f1_micro(tr, np.array([[1, 1], [0, 0]], dtype=np.uint8)) == pytest.approx(2.0 / 4.0)
    res = {"classes": 7, "train": 10, "test": 4, "f1_micro": 0.5, "f1_macro": 0.25, "train_f1_micro": 1.0,
           "baseline_f1_micro": 0.125, "loss": 1.5, "evals": 12, "stop": "gtol", "time": 0.25}
    assert ev.result_line("test", res) == (
        "Downstream classifier: setting= test classes= 7 train= 10 test= 4 f1_micro= 0.50000 f1_macro= 0.25000 "
        "train_f1_micro= 1.00000 baseline_f1_micro= 0.12500 loss= 1.500000 evals= 12 stop= gtol time= 0.25000")


def test_module_imports_no_scipy_or_sklearn():
    for mod in ("evaluation.py", "eval_embeddings.py"):
        src = open(os.path.join(ROOT, "graphsage_amd", mod)).read()
        assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn)", src, flags=re.M)


# ------------------------------------------------------------------------------------------------ refusals and flags
def test_refusals():
    from graphsage_amd import evaluation as ev
    assert ev.refuse(512, np.array([0, 127])) == 128 and ev.refuse(510, np.zeros((3, 128))) == 128
    with pytest.raises(ValueError, match="no class labels"):
        ev.refuse(64, None)
    with pytest.raises(ValueError, match="width 516"):
        ev.refuse(516, np.array([0, 1]))
    with pytest.raises(ValueError, match="129 classes"):
        ev.refuse(64, np.array([0, 128]))
    with pytest.raises(ValueError, match="129 classes"):
        ev.refuse(64, np.zeros((3, 129)))


def test_flag_parsing_and_driver_refusals(capsys):
    from graphsage_amd import unsupervised_train as ut
    assert ut.build_flags([]).eval_classifier == ""
    assert ut.build_flags(["--eval_classifier", "test"]).eval_classifier == "test"
    assert ut.build_flags(["--eval_classifier", "val"]).eval_classifier == "val"
    with pytest.raises(SystemExit):
        ut.build_flags(["--eval_classifier", "train"])
    capsys.readouterr()
    f = ut.build_flags(["--model", "n2v", "--dim_1", "300", "--dim_2", "8"])
    assert ut.embedding_width(f) == 600 and ut.embedding_width(ut.build_flags(["--dim_1", "300", "--dim_2", "8"])) == 16
    # an embedding width over 512 and a run that saves no embeddings: refused before the data is loaded
    for argv, word in ((["--dim_2", "260"], "520"), (["--model", "n2v", "--dim_1", "300"], "600"),
                       (["--save_embeddings", "false"], "--save_embeddings")):
        with pytest.raises(SystemExit) as ei:
            ut.main(["--synthetic", "small", "--eval_classifier", "test"] + argv)
        assert "--eval_classifier" in str(ei.value) and word in str(ei.value)
        assert "Loading training data" not in capsys.readouterr().out
    ut.refuse_eval_classifier(ut.build_flags(["--dim_2", "260"]))            # without the flag nothing is refused

    # a dataset without class labels, or with more than 128 classes: refused once the graph is loaded, before training
    class G(object):
        labels = None
    flags = ut.build_flags(["--eval_classifier", "val"])
    with pytest.raises(SystemExit, match="no class labels"):
        ut.refuse_eval_classifier(flags, G())
    G.labels = np.arange(130)
    with pytest.raises(SystemExit, match="130 classes"):
        ut.refuse_eval_classifier(flags, G())
    G.labels = np.zeros((5, 121), dtype=np.float32)
    ut.refuse_eval_classifier(flags, G())

    from graphsage_amd import eval_embeddings as ee
    f = ee.build_flags(["data/ppi", "unsup-ppi/x", "test"])
    assert (f.data_prefix, f.embed_dir, f.setting, f.table) == ("data/ppi", "unsup-ppi/x", "test", "val")
    with pytest.raises(SystemExit):
        ee.build_flags(["data/ppi", "unsup-ppi/x", "train"])
    with pytest.raises(SystemExit, match="feat"):
        ee.main(["data/ppi", "feat", "test"])


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_binding_and_error_reporting():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    for name in ("gs_logreg_eval", "gs_logreg_ws_bytes"):
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"typedef struct gs_logreg_desc \{", header)
    # entry points were added and no struct layout changed: the version stays (the header's own rule)
    version = int(re.search(r"#define GS_ABI_VERSION (\d+)\b", header).group(1))
    lib = _lib.load()
    assert lib.gs_abi_version() == version == _lib.GS_ABI_VERSION
    sizes = (ctypes.c_int32 * 16)()
    assert lib.gs_abi_struct_sizes(sizes, 16) == 8                        # the descriptor goes by pointer
    assert ctypes.sizeof(_lib.LogregDesc) == 168
    for macro, value in (("GS_LOGREG_FIT", _lib.LOGREG_FIT), ("GS_LOGREG_PREDICT", _lib.LOGREG_PREDICT),
                         ("GS_LOGREG_MAX_D", _lib.LOGREG_MAX_D), ("GS_LOGREG_MAX_C", _lib.LOGREG_MAX_C)):
        assert int(re.search(r"#define %s (\d+)\b" % macro, header).group(1)) == value

    # the workspace rule of the header, restated
    cdiv = lambda a, b: -(-a // b)
    out = ctypes.c_int64(0)
    for n, d, c in ((1, 4, 1), (70, 36, 5), (16384, 36, 5), (16385, 36, 5), (153431, 256, 41), (44906, 256, 121)):
        tiles = cdiv(n, 32)
        wgs = cdiv(tiles, cdiv(tiles, 512))
        assert lib.gs_logreg_ws_bytes(n, d, c, ctypes.byref(out)) == 0 and out.value == wgs * (2 * c + d * c) * 4
    for n, d, c, word in ((0, 8, 2, b"n=0"), (5, 6, 2, b"multiple of 4"), (5, 0, 2, b"multiple of 4"), (5, 516, 2, b"multiple of 4"),
                          (5, 8, 0, b"c=0"), (5, 8, 129, b"c=129")):
        assert lib.gs_logreg_ws_bytes(n, d, c, ctypes.byref(out)) == -1 and word in lib.gs_last_error()

    # every bad descriptor is refused before anything is launched or read (the pointers below are host memory)
    assert lib.gs_logreg_eval(None, None) == -1 and b"gs_logreg_eval" in lib.gs_last_error()
    buf = (ctypes.c_int64 * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def desc():
        q = _lib.LogregDesc()
        q.X = q.W = q.b = q.y_class = q.loss = q.gW = q.gb = q.ws = p
        q.n, q.n_rows, q.ldx, q.ldw, q.ldy, q.ldp, q.ws_bytes = 5, 10, 8, 4, 0, 0, 1 << 20
        q.d, q.c, q.mode, q.flags = 8, 3, _lib.LOGREG_FIT, 0
        return q

    def refused(q, word):
        assert lib.gs_logreg_eval(ctypes.addressof(q), None) == -1, word
        assert b"gs_logreg_eval" in lib.gs_last_error() and word in lib.gs_last_error(), lib.gs_last_error()

    cases = [("mode", 2, b"mode"), ("flags", 1, b"flags"), ("n", 0, b"n=0"), ("d", 6, b"multiple of 4"), ("d", 516, b"multiple of 4"),
             ("c", 0, b"c=0"), ("c", 129, b"c=129"), ("ldx", 4, b"ldx"), ("ldx", 9, b"ld"), ("ldw", 2, b"ldw"), ("X", None, b"X"),
             ("X", p + 4, b"aligned"), ("W", None, b"W"), ("b", None, b"W and b"), ("n_rows", 0, b"n_rows"), ("n", 11, b"n_rows"),
             ("y_class", None, b"FIT needs"), ("y_multi", p, b"exclude"), ("loss", None, b"loss, gW and gb"),
             ("gW", None, b"loss, gW and gb"), ("pred_class", p, b"PREDICT mode only"), ("ws", None, b"workspace"),
             ("ws_bytes", 8, b"workspace"), ("ws", p + 4, b"workspace")]
    for field, value, word in cases:
        q = desc()
        setattr(q, field, value)
        refused(q, word)
    q = desc()                                   # multi-label: ldy below c
    q.y_class, q.y_multi, q.ldy = None, p, 2
    refused(q, b"ldy")
    q = desc()                                   # PREDICT: no gradient, something to write, a loss needs labels, ldp >= c
    q.mode = _lib.LOGREG_PREDICT
    refused(q, b"FIT mode only")
    q.gW = q.gb = q.loss = None
    refused(q, b"nothing to write")
    q.loss, q.y_class = p, None
    refused(q, b"needs labels")
    q.loss, q.pred_multi, q.ldp = None, p, 2
    refused(q, b"ldp")
