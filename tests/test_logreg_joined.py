"""Host side of the joined classifier inputs (no GPU): the C ABI of gs_logreg_eval_joined / gs_logreg_joined_ws_bytes /
gs_col_moments and their refusals, the fixtures made from the reference's own run on standardised rows
(tests/golden/ref_eval_feat_multiclass.npz, ref_eval_both_multilabel.npz, made by make_ref_eval_joined_fixtures.py), the
solver on them, the flags and refusals of the drivers."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("ref_eval_feat_multiclass", "ref_eval_both_multilabel")
SHAPES = {"ref_eval_feat_multiclass": (300, 120, 22, 0, 4), "ref_eval_both_multilabel": (350, 120, 22, 32, 7)}


def load_fixture(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))


def joined(fx, part):
    """The raw joined rows [features | embeddings] of a fixture's part, fp32."""
    cols = [fx["F_" + part]] + ([fx["E_" + part]] if "E_" + part in fx else [])
    return np.hstack(cols)


def standardised(fx, part):
    """... standardised in fp64 with the stored scaler."""
    return (joined(fx, part).astype(np.float64) - fx["scaler_mean"]) / fx["scaler_scale"]


def fixture_targets(fx):
    from graphsage_amd import evaluation as ev
    y = fx["y_train"]
    return ev.targets(y, None if y.ndim == 2 else fx["W_star"].shape[1])[0]


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_contents(name):
    """Shapes, the kinds of column the issue asks for, the scaler against a NumPy restatement of StandardScaler, and J_star /
    J_ref recomputed on the standardised rows (not read); no test row within 1e-4 of the optimum's decision boundary."""
    from graphsage_amd import evaluation as ev
    fx = load_fixture(name)
    n_train, n_test, df, de, c = SHAPES[name]
    F = fx["F_train"]
    assert F.dtype == np.float32 and F.shape == (n_train, df) and fx["F_test"].shape == (n_test, df) and df % 4 != 0
    if de:
        E = fx["E_train"]
        assert E.dtype == np.float32 and E.shape == (n_train, de) and fx["E_test"].shape == (n_test, de)
        assert np.allclose(np.linalg.norm(E.astype(np.float64), axis=1), 1.0, atol=1e-6)
    else:
        assert "E_train" not in fx
    std, mean = F.astype(np.float64).std(axis=0), F.astype(np.float64).mean(axis=0)
    assert std.min() >= 0.15 and std.max() <= 40.0 and std.max() / std.min() > 20 and np.abs(mean).max() <= 55.0
    assert np.abs(mean).max() > 10.0
    assert (F[:, 0] >= 0).all() and np.array_equal(F[:, 0], np.floor(F[:, 0])) and (F[:, 1] < 0).any()      # counts, scores
    X = joined(fx, "train").astype(np.float64)
    m = X.mean(axis=0)
    s = np.sqrt(((X - m) ** 2).mean(axis=0))
    s[s == 0] = 1.0
    assert np.allclose(fx["scaler_mean"], m, rtol=1e-12, atol=1e-12) and np.allclose(fx["scaler_scale"], s, rtol=1e-12, atol=0)
    S = fixture_targets(fx)
    assert S.shape == (n_train, c) and fx["W_star"].shape == (df + de, c)
    assert fx["ref_coef"].shape == (df + de, c) and fx["ref_intercept"].shape == (c,) and fx["ref_f1_test"].size >= 1
    Xs = standardised(fx, "train")
    J_star = ev.objective(Xs, S, fx["W_star"], fx["b_star"], float(fx["alpha"]))
    J_ref = ev.objective(Xs, S, fx["ref_coef"], fx["ref_intercept"], float(fx["alpha"]))
    # the generator's rows are scaler.transform's, (x - mean) / scale in fp64 as here: what differs is the order of ~400 sums
    assert np.allclose(J_star, fx["J_star"], rtol=1e-11, atol=0) and np.allclose(J_ref, fx["J_ref"], rtol=1e-11, atol=0)
    assert (J_ref >= J_star).all() and float(fx["alpha"]) == ev.ALPHA == 1e-4
    z = standardised(fx, "test").dot(fx["W_star"]) + fx["b_star"]
    srt = np.sort(z, axis=1)
    assert (np.abs(z).min() if fx["y_train"].ndim == 2 else (srt[:, -1] - srt[:, -2]).min()) > 1e-4


@pytest.mark.parametrize("name", FIXTURES)
def test_solver_reaches_the_fp64_optimum(name):
    from graphsage_amd import evaluation as ev
    fx = load_fixture(name)
    X, S = standardised(fx, "train"), fixture_targets(fx)
    n, d = X.shape
    c = S.shape[1]
    W, b, J, evals, stop = ev.lbfgs(ev.numpy_evaluator(X, S), n, d, c, gtol=1e-9, max_evals=5000)
    assert stop in ("gtol", "noise") and evals < 5000
    J64 = ev.objective(X, S, W, b)
    print(name, "evals", evals, "stop", stop, "max rel gap", ((J64 - fx["J_star"]) / fx["J_star"]).max())
    assert (J64 - fx["J_star"] <= 1e-9 * fx["J_star"]).all(), (J64 - fx["J_star"]) / fx["J_star"]
    assert (J64 <= fx["J_ref"]).all()


# ------------------------------------------------------------------------------------------------ host helpers
def test_joined_line_and_width_refusals():
    from graphsage_amd import evaluation as ev
    res = {"classes": 7, "train": 10, "test": 4, "f1_micro": 0.5, "f1_macro": 0.25, "train_f1_micro": 1.0,
           "baseline_f1_micro": 0.125, "loss": 1.5, "evals": 12, "stop": "gtol", "time": 0.25, "width": 82}
    assert ev.joined_result_line("features", "test", res) == (
        "Downstream classifier (features): setting= test classes= 7 train= 10 test= 4 f1_micro= 0.50000 f1_macro= 0.25000 "
        "train_f1_micro= 1.00000 baseline_f1_micro= 0.12500 loss= 1.500000 evals= 12 stop= gtol width= 82 time= 0.25000")
    assert ev.joined_result_line("both", "val", res).startswith("Downstream classifier (features+embeddings): setting= val ")
    # each source is padded to a multiple of 4: 602 -> 604, + 256 = 860; 602 + 420 = 1024; 602 + 422 -> 1028
    assert ev.refuse_joined(602, None) == 604 and ev.refuse_joined(602, 256) == 860 and ev.refuse_joined(602, 420) == 1024
    assert ev.refuse_joined(1024, None) == 1024
    with pytest.raises(ValueError, match="1028"):
        ev.refuse_joined(602, 422)
    with pytest.raises(ValueError, match="1028"):
        ev.refuse_joined(1025, None)
    with pytest.raises(SystemExit, match="no feature table"):
        ev.refuse_inputs("features", None, 64, has_features=False)
    with pytest.raises(SystemExit, match="1116"):
        ev.refuse_inputs("both", 602, 512)
    ev.refuse_inputs("features", 602, 512)                  # the embeddings take no part in `features`
    ev.refuse_inputs("embeddings", None, 64, has_features=False)
    with pytest.raises(SystemExit, match="inputs"):
        ev.refuse_inputs("feat", 602, 64)


def test_log_counts():
    from graphsage_amd import eval_embeddings as ee
    f = np.array([[0.0, -0.5, 5.0], [9.0, 3.0, 6.0]], dtype=np.float32)
    g = ee.log_counts(f)
    assert np.array_equal(f, np.array([[0.0, -0.5, 5.0], [9.0, 3.0, 6.0]], dtype=np.float32))          # a copy
    assert g.dtype == np.float32 and np.array_equal(g[:, 2], f[:, 2])
    # log(f0 + 1); f1 - min(min f1, -1) = f1 + 1 while min f1 > -1
    assert np.allclose(g[:, 0], np.log([1.0, 10.0])) and np.allclose(g[:, 1], np.log([0.5, 4.0]))
    # a minimum below -1 is the shift: the reference's rule then takes log(0) of that row, which no scaler survives
    with pytest.raises(SystemExit, match="not finite"):
        ee.log_counts(np.array([[1.0, -7.0], [2.0, 2.0]], dtype=np.float32))
    with pytest.raises(SystemExit, match="columns 0 and 1"):
        ee.log_counts(np.zeros((3, 1), dtype=np.float32))


# ------------------------------------------------------------------------------------------------ flags and refusals
def write_toy(prefix, n=12, feats=None):
    ids = ["n%d" % i for i in range(n)]
    nodes = [{"id": ids[i], "val": i % 4 == 2, "test": i % 4 == 3} for i in range(n)]
    links = [{"source": i, "target": (i + 1) % n} for i in range(n)]
    json.dump({"directed": False, "graph": {}, "nodes": nodes, "links": links, "multigraph": False}, open(prefix + "-G.json", "w"))
    json.dump({ids[i]: i for i in range(n)}, open(prefix + "-id_map.json", "w"))
    json.dump({ids[i]: i % 3 for i in range(n)}, open(prefix + "-class_map.json", "w"))
    if feats is not None:
        np.save(prefix + "-feats.npy", feats)


def test_driver_flags_and_refusals(capsys, tmp_path):
    from graphsage_amd import unsupervised_train as ut
    assert ut.build_flags([]).eval_classifier_inputs == "embeddings"
    for kind, kinds in (("embeddings", ()), ("features", ("features",)), ("both", ("both",)), ("all", ("features", "both"))):
        f = ut.build_flags(["--eval_classifier", "test", "--eval_classifier_inputs", kind])
        assert f.eval_classifier_inputs == kind and ut.eval_classifier_kinds(f) == kinds
    with pytest.raises(SystemExit):
        ut.build_flags(["--eval_classifier_inputs", "feat"])
    capsys.readouterr()
    assert ut.feature_width(ut.build_flags(["--synthetic", "small"])) == 50
    assert ut.feature_width(ut.build_flags(["--synthetic", "reddit"])) == 602
    bare, wide = str(tmp_path / "bare"), str(tmp_path / "wide")
    write_toy(bare)
    write_toy(wide, feats=np.zeros((12, 1026), dtype=np.float32))
    assert ut.feature_width(ut.build_flags(["--train_prefix", bare])) is None
    assert ut.feature_width(ut.build_flags(["--train_prefix", wide])) == 1026
    ec = ["--eval_classifier", "test"]
    cases = [(["--synthetic", "small", "--eval_classifier_inputs", "features"], "needs --eval_classifier"),
             (["--synthetic", "small", "--eval_classifier_inputs", "all"], "needs --eval_classifier"),
             (["--train_prefix", bare, "--eval_classifier_inputs", "features"] + ec, "no feature table"),
             (["--train_prefix", bare, "--eval_classifier_inputs", "all"] + ec, "no feature table"),
             (["--train_prefix", wide, "--eval_classifier_inputs", "features"] + ec, "1028"),
             (["--synthetic", "reddit", "--dim_2", "256", "--eval_classifier_inputs", "both"] + ec, "1116"),
             (["--synthetic", "reddit", "--dim_2", "256", "--eval_classifier_inputs", "all"] + ec, "1116"),
             (["--synthetic", "small", "--dim_2", "260", "--eval_classifier_inputs", "both"] + ec, "520")]
    for argv, word in cases:
        with pytest.raises(SystemExit) as ei:
            ut.main(argv)
        assert "--eval_classifier" in str(ei.value) and word in str(ei.value), (argv, str(ei.value))
        assert "Loading training data" not in capsys.readouterr().out
    # what is not refused: 602 -> 604 + 2 * 210 = 1024; features alone beside any embedding width the classifier takes
    ut.refuse_eval_classifier(ut.build_flags(["--synthetic", "reddit", "--dim_2", "210", "--eval_classifier_inputs", "all"] + ec))
    ut.refuse_eval_classifier(ut.build_flags(["--synthetic", "reddit", "--dim_2", "256", "--eval_classifier_inputs", "features"] + ec))

    # once the graph is loaded: its own feature table decides
    class G(object):
        labels = np.arange(5)
        feats = None
    flags = ut.build_flags(["--synthetic", "small", "--eval_classifier_inputs", "both"] + ec)
    with pytest.raises(SystemExit, match="no feature table"):
        ut.refuse_eval_classifier(flags, G())
    G.feats = np.zeros((5, 50), dtype=np.float32)
    ut.refuse_eval_classifier(flags, G())


def test_eval_embeddings_flags_and_refusals(capsys, tmp_path):
    from graphsage_amd import eval_embeddings as ee
    f = ee.build_flags(["data/ppi", "out", "test"])
    assert (f.inputs, f.log_counts) == ("embeddings", False)
    f = ee.build_flags(["data/ppi", "out", "val", "--inputs", "both", "--log_counts"])
    assert (f.data_prefix, f.embed_dir, f.setting, f.inputs, f.log_counts) == ("data/ppi", "out", "val", "both", True)
    with pytest.raises(SystemExit):
        ee.build_flags(["data/ppi", "out", "val", "--inputs", "feat"])
    capsys.readouterr()
    with pytest.raises(SystemExit, match="feat") as ei:
        ee.main(["data/ppi", "feat", "test"])
    assert "--inputs features" in str(ei.value)
    with pytest.raises(SystemExit, match="--log_counts"):
        ee.main(["data/ppi", "out", "test", "--log_counts"])
    assert "Loading data" not in capsys.readouterr().out
    # a dataset without a feature table refuses features and both; one whose table is too wide names the padded width
    bare, wide = str(tmp_path / "bare"), str(tmp_path / "wide")
    write_toy(bare)
    write_toy(wide, feats=np.zeros((12, 1026), dtype=np.float32))
    for inputs in ("features", "both"):
        with pytest.raises(SystemExit, match="no feature table"):
            ee.main([bare, str(tmp_path), "test", "--inputs", inputs])
        assert "Running regression" not in capsys.readouterr().out
    with pytest.raises(SystemExit, match="1028"):
        ee.main([wide, str(tmp_path), "test", "--inputs", "features"])
    assert "Running regression" not in capsys.readouterr().out


def test_existing_signatures_keep_their_defaults():
    import inspect
    from graphsage_amd import evaluation as ev
    sig = inspect.signature(ev.fit_classifier)
    assert list(sig.parameters)[:9] == ["engine", "Z", "rows", "labels", "n_classes", "alpha", "gtol", "max_evals", "memory"]
    assert (sig.parameters["features"].default, sig.parameters["standardize"].default) == (None, False)
    sig = inspect.signature(ev.evaluate_split)
    assert list(sig.parameters)[:7] == ["engine", "train_table", "train_rows", "train_labels", "test_table", "test_rows", "test_labels"]
    sig = inspect.signature(ev.evaluate_embedding_dir)
    assert list(sig.parameters)[:5] == ["engine", "G", "embed_dir", "setting", "base"] and sig.parameters["inputs"].default == "embeddings"
    assert ev.LINE_FILE == {"embeddings": "eval_classifier.txt", "features": "eval_classifier_features.txt",
                            "both": "eval_classifier_both.txt"}
    for mod in ("evaluation.py", "eval_embeddings.py"):
        src = open(os.path.join(ROOT, "graphsage_amd", mod)).read()
        assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn)", src, flags=re.M) and "not provided" not in src
    assert "not provided" not in open(os.path.join(ROOT, "README.md")).read()


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_binding_and_error_reporting():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    for name in ("gs_logreg_eval_joined", "gs_logreg_joined_ws_bytes", "gs_col_moments"):
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"typedef struct gs_logreg_joined_desc \{", header)
    version = int(re.search(r"#define GS_ABI_VERSION (\d+)\b", header).group(1))
    lib = _lib.load()
    for name in ("gs_logreg_eval_joined", "gs_logreg_joined_ws_bytes", "gs_col_moments"):
        assert getattr(lib, name) is not None
    assert lib.gs_abi_version() == version == _lib.GS_ABI_VERSION == 12
    sizes = (ctypes.c_int32 * 16)()
    assert lib.gs_abi_struct_sizes(sizes, 16) == 8
    assert ctypes.sizeof(_lib.LogregDesc) == 168 and ctypes.sizeof(_lib.LogregJoinedDesc) == 224
    for macro, value in (("GS_LOGREG_MAX_D", 512), ("GS_LOGREG_JOINED_MAX_D", _lib.LOGREG_JOINED_MAX_D), ("GS_LOGREG_JOINED_MAX_D", 1024),
                         ("GS_COL_MOMENTS_MAX_CHUNKS", _lib.COL_MOMENTS_MAX_CHUNKS)):
        assert int(re.search(r"#define %s (\d+)\b" % macro, header).group(1)) == value
    assert _lib.LOGREG_MAX_D == 512
    hip = open(os.path.join(ROOT, "graphsage_amd", "csrc", "gs_logreg.hip")).read()
    assert "static_assert(sizeof(gs_logreg_joined_desc) == 224" in hip and '#include "gs_logreg_dev.h"' in hip
    assert "__builtin_amdgcn_mfma" not in hip                 # one copy of the tile loop: the shared header's
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in open(os.path.join(ROOT, "graphsage_amd", "csrc", "gs_logreg_dev.h")).read()

    # the workspace rule: gs_logreg_ws_bytes' formula, d up to 1024; the old entry point keeps its limit
    cdiv = lambda a, b: -(-a // b)
    out = ctypes.c_int64(0)
    for n, d, c in ((1, 4, 1), (70, 36, 5), (70, 516, 5), (16385, 860, 5), (153431, 604, 41), (153431, 1024, 128)):
        tiles = cdiv(n, 32)
        wgs = cdiv(tiles, cdiv(tiles, 512))
        assert lib.gs_logreg_joined_ws_bytes(n, d, c, ctypes.byref(out)) == 0 and out.value == wgs * (2 * c + d * c) * 4
    for n, d, c, word in ((0, 8, 2, b"n=0"), (5, 6, 2, b"multiple of 4"), (5, 1028, 2, b"1024"), (5, 8, 129, b"c=129")):
        assert lib.gs_logreg_joined_ws_bytes(n, d, c, ctypes.byref(out)) == -1 and word in lib.gs_last_error()
        assert b"gs_logreg_joined_ws_bytes" in lib.gs_last_error()
    assert lib.gs_logreg_ws_bytes(5, 516, 2, ctypes.byref(out)) == -1 and b"512" in lib.gs_last_error()

    # every bad descriptor is refused before anything is launched or read (the pointers below are host memory)
    assert lib.gs_logreg_eval_joined(None, None) == -1 and b"gs_logreg_eval_joined" in lib.gs_last_error()
    buf = (ctypes.c_int64 * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def desc(with_b=True, affine=True):
        q = _lib.LogregJoinedDesc()
        q.Xa = q.W = q.b = q.y_class = q.loss = q.gW = q.gb = q.ws = p
        q.n, q.n_rows_a, q.lda, q.ldw, q.ws_bytes = 5, 10, 8, 4, 1 << 20
        q.da, q.c, q.mode = 8, 3, _lib.LOGREG_FIT
        if with_b:
            q.Xb, q.rows_b, q.n_rows_b, q.ldb, q.db = p, p, 7, 12, 12
        if affine:
            q.mu = q.inv = p
        return q

    def refused(q, word):
        assert lib.gs_logreg_eval_joined(ctypes.addressof(q), None) == -1, word
        assert b"gs_logreg_eval_joined" in lib.gs_last_error() and word in lib.gs_last_error(), lib.gs_last_error()

    cases = [("mode", 2, b"mode"), ("flags", 1, b"flags"), ("reserved_", 1, b"flags"), ("n", 0, b"n=0"),
             ("da", 6, b"multiples of 4"), ("da", 0, b"da >= 4"), ("db", 6, b"multiples of 4"), ("da", 1016, b"1028"),
             ("db", 0, b"source B is given"), ("ldb", 8, b"ldb"), ("ldb", 13, b"ld"), ("Xb", None, b"Xb"),
             ("Xb", p + 4, b"aligned"), ("n_rows_b", 0, b"n_rows_b"), ("lda", 4, b"lda"), ("Xa", None, b"Xa"),
             ("n_rows_a", 0, b"n_rows_a"), ("n", 11, b"without rows_a"), ("mu", None, b"mu and inv"), ("inv", None, b"mu and inv"),
             ("mu", p + 4, b"16-byte"), ("c", 0, b"c=0"), ("c", 129, b"c=129"), ("ldw", 2, b"ldw"), ("W", None, b"W"),
             ("y_class", None, b"FIT needs"), ("y_multi", p, b"exclude"), ("loss", None, b"loss, gW and gb"),
             ("pred_class", p, b"PREDICT mode only"), ("ws", None, b"workspace"), ("ws_bytes", 8, b"workspace")]
    for field, value, word in cases:
        q = desc()
        setattr(q, field, value)
        refused(q, word)
    q = desc()                                   # n beyond table B's rows, without rows_b
    q.rows_b, q.n = None, 8
    refused(q, b"without rows_b")
    q = desc(with_b=False)                       # B absent: d = da; a single field of B makes it "given"
    q.da, q.lda = 1028, 1028
    refused(q, b"1028")
    for field, value in (("rows_b", p), ("ldb", 4), ("n_rows_b", 3)):
        q = desc(with_b=False)
        setattr(q, field, value)
        refused(q, b"source B is given")
    q = desc()                                   # PREDICT, as gs_logreg_eval
    q.mode = _lib.LOGREG_PREDICT
    refused(q, b"FIT mode only")
    q.gW = q.gb = q.loss = None
    refused(q, b"nothing to write")

    # gs_col_moments: the same source rules, its outputs and its workspace
    def moments(**kw):
        a = dict(Xa=p, rows_a=None, lda=8, da=8, n_rows_a=10, Xb=p, rows_b=p, ldb=12, db=12, n_rows_b=7, n=5, mean=p, var=p,
                 ws=p, ws_bytes=1 << 20)
        a.update(kw)
        return lib.gs_col_moments(a["Xa"], a["rows_a"], a["lda"], a["da"], a["n_rows_a"], a["Xb"], a["rows_b"], a["ldb"], a["db"],
                                  a["n_rows_b"], a["n"], a["mean"], a["var"], a["ws"], a["ws_bytes"], None)

    for kw, word in ((dict(da=6), b"multiples of 4"), (dict(da=1016), b"1028"), (dict(db=0), b"source B is given"),
                     (dict(ldb=8), b"ldb"), (dict(n=11), b"without rows_a"), (dict(n=0), b"n=0"), (dict(mean=None), b"mean and var"),
                     (dict(var=p + 4), b"mean and var"), (dict(ws=None), b"workspace"), (dict(ws_bytes=256 * 20 * 8 - 8), b"workspace")):
        assert moments(**kw) == -1 and b"gs_col_moments" in lib.gs_last_error() and word in lib.gs_last_error(), (kw, lib.gs_last_error())
