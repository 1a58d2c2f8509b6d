"""gs_logreg_eval and the classifier built on it, on the device: fp64 parity of FIT and PREDICT at the tile, class-block and
width edges, bitwise repeatability, optimality of the fit against the reference's own run and the fp64 optimum
(tests/golden/ref_eval_*.npz), and the --eval_classifier flag of the unsupervised driver."""
import os
import re

import numpy as np
import pytest
import torch

from graphsage_amd import engine as eng
from graphsage_amd import evaluation as ev
from graphsage_amd import ops
from graphsage_amd.ops import Mat

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GARBAGE = 7.0e30            # what the pad columns hold: a kernel that reads one shows it
MARGIN = 1e-4
FIXTURES = ("ref_eval_multiclass", "ref_eval_multilabel")


def tol(ref):
    """The project's float tolerance."""
    return 1e-4 * max(1.0, float(np.abs(ref).max()))


def padded(a, pad, dev, fill):
    """a [r, w] in a device buffer [r, round_up(w, 4) + pad] whose other columns hold `fill`."""
    r, w = a.shape
    buf = torch.full((r, ops.round_up(w, 4) + pad), fill, dtype=torch.from_numpy(a).dtype, device=dev)
    buf[:, :w] = torch.from_numpy(a).to(dev)
    return buf


class Case(object):
    """One problem: inputs on the device with pad columns, the fp64 restatement of the same fp32 inputs on the host."""

    def __init__(self, dev, n, d, c, multi, rows="none", ldx_pad=0, ldw_pad=0, ldy_pad=0, w_scale=1.0, seed=0):
        rng = np.random.RandomState(seed + 1000 * n + 10 * d + c)
        n_rows = n if rows == "none" else n + 9
        X = rng.randn(n_rows, d).astype(np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        W = (rng.randn(d, c) * w_scale).astype(np.float32)                       # unit rows: logits of order w_scale
        b = (rng.randn(c) * 0.5).astype(np.float32)
        if rows == "none":
            idx = None
        elif rows == "perm":
            idx = rng.permutation(n_rows)[:n].astype(np.int32)
        else:                                                                     # repeats, and not every row
            idx = rng.randint(0, max(1, n_rows // 2), size=n).astype(np.int32)
        Xg = X[idx] if idx is not None else X
        z = Xg.astype(np.float64).dot(W.astype(np.float64)) + b.astype(np.float64)
        noise = z + rng.randn(n, c) * w_scale
        y = (noise > 0).astype(np.uint8) if multi else noise.argmax(axis=1).astype(np.int32)
        S = ev.targets(y, None if multi else c)[0]
        m = S * z
        e = np.exp(-np.abs(m))
        r = -S * np.where(m >= 0, e, 1.0) / (1.0 + e)
        self.n, self.d, self.c, self.multi, self.z = n, d, c, multi, z
        self.loss = (np.maximum(-m, 0.0) + np.log1p(e)).sum(axis=0)
        self.gW, self.gb = Xg.astype(np.float64).T.dot(r), r.sum(axis=0)
        self.X = Mat(padded(X, ldx_pad, dev, GARBAGE), d)
        self.W = Mat(padded(W, ldw_pad, dev, GARBAGE), c)
        self.b = torch.from_numpy(b).to(dev)
        self.rows = torch.from_numpy(idx).to(dev) if idx is not None else None
        self.y_class = None if multi else torch.from_numpy(y).to(dev)
        self.y_multi = padded(y, ldy_pad, dev, 1)[:, :c + ldy_pad] if multi else None
        self.ldp_pad = ldy_pad

    def labels(self):
        return dict(y_class=self.y_class, y_multi=self.y_multi)

    def fit(self):
        return ops.logreg_eval(self.X, self.W, self.b, n=self.n, rows=self.rows, mode=ops.LOGREG_FIT, **self.labels())

    def check(self):
        dev = self.b.device
        n, c = self.n, self.c
        loss, gW, gb = [t.cpu().numpy() for t in self.fit()]
        for name, got, ref in (("loss", loss, self.loss), ("gW", gW, self.gW), ("gb", gb, self.gb)):
            err = float(np.abs(got - ref).max())
            print("%s n=%d d=%d c=%d: max err %.3e of tol %.3e" % (name, n, self.d, c, err, tol(ref)))
            assert got.shape == ref.shape and np.isfinite(got).all() and err <= tol(ref), (name, err, tol(ref))
        # PREDICT: both prediction forms and the loss in one call
        pred_class = torch.full((n,), -7, dtype=torch.int32, device=dev)
        pred_multi = torch.full((n, c + self.ldp_pad), 9, dtype=torch.uint8, device=dev)
        ploss = torch.zeros(c, dtype=torch.float64, device=dev)
        ops.logreg_eval(self.X, self.W, self.b, n=n, rows=self.rows, mode=ops.LOGREG_PREDICT, loss=ploss, pred_class=pred_class,
                        pred_multi=pred_multi, **self.labels())
        assert float(np.abs(ploss.cpu().numpy() - self.loss).max()) <= tol(self.loss)
        pm = pred_multi.cpu().numpy()
        assert (pm[:, c:] == 9).all()                                             # pad columns are not written
        sure = np.abs(self.z) > MARGIN
        assert np.array_equal(pm[:, :c][sure], (self.z > 0).astype(np.uint8)[sure])
        assert (~sure).mean() <= 0.01
        pc = pred_class.cpu().numpy()
        assert ((pc >= 0) & (pc < c)).all()
        if c > 1:
            srt = np.sort(self.z, axis=1)
            sure = srt[:, -1] - srt[:, -2] > MARGIN
            assert np.array_equal(pc[sure], self.z.argmax(axis=1)[sure]) and (~sure).mean() <= 0.01
        else:
            assert (pc == 0).all()
        # predictions alone need neither labels nor a workspace
        pc2 = torch.full((n,), -7, dtype=torch.int32, device=dev)
        ops.logreg_eval(self.X, self.W, self.b, n=n, rows=self.rows, mode=ops.LOGREG_PREDICT, pred_class=pc2)
        assert np.array_equal(pc2.cpu().numpy(), pc)


# ------------------------------------------------------------------------------------------------ 1. kernel parity
# one factor at a time around n = 70, d = 36, c = 5.  The kernel's constants are 32 rows per tile and 32 classes per block,
# at most 512 workgroups (n = 16384 is the last shape with one tile each; 20000 gives 313 workgroups of two tiles)
# and at most 32 gradient tiles of 32 x 32 per workgroup: (352, 70) and (512, 128) cut the d blocks over two workgroups.
N_EDGES = [1, 31, 32, 33, 65, 16384, 20000]
C_EDGES = [1, 2, 31, 32, 33, 121, 128]
D_EDGES = [4, 36, 256, 260, 512]
SHAPES = ([(n, 36, 5) for n in N_EDGES] + [(70, 36, c) for c in C_EDGES] + [(70, d, 5) for d in D_EDGES]
          + [(70, 352, 70), (70, 512, 128), (150, 256, 41)])


@pytest.mark.parametrize("multi", [False, True], ids=["class", "multi"])
@pytest.mark.parametrize("n,d,c", SHAPES)
def test_parity_shapes(dev, n, d, c, multi):
    Case(dev, n, d, c, multi).check()


@pytest.mark.parametrize("multi", [False, True], ids=["class", "multi"])
@pytest.mark.parametrize("kw", [dict(ldx_pad=8), dict(ldw_pad=12), dict(ldy_pad=7), dict(ldx_pad=4, ldw_pad=4, ldy_pad=3),
                                dict(rows="perm"), dict(rows="repeat"), dict(rows="repeat", ldx_pad=8, ldw_pad=4, ldy_pad=5)],
                         ids=lambda kw: "-".join("%s=%s" % kv for kv in sorted(kw.items())))
def test_parity_layouts_and_rows(dev, kw, multi):
    Case(dev, 70, 36, 5, multi, **kw).check()
    Case(dev, 20000, 36, 33, multi, **kw).check()


@pytest.mark.parametrize("multi", [False, True], ids=["class", "multi"])
def test_parity_large_logits(dev, multi):
    """Logits beyond +-60 on both sides: exp(60) would overflow nothing in fp32 yet, but the naive log(1 + exp(-m)) loses
    every digit of a loss of 60; the safe form does not, and no residual is NaN."""
    case = Case(dev, 70, 36, 5, multi, w_scale=40.0)
    assert case.z.max() > 60 and case.z.min() < -60
    case.check()


def test_wrapper_refuses_bad_arguments(dev):
    case = Case(dev, 70, 36, 5, False)
    with pytest.raises(ops._lib.GraphsageAmdError, match="y_class"):
        ops.logreg_eval(case.X, case.W, case.b, n=70, y_class=case.y_class.to(torch.int64))
    with pytest.raises(ops._lib.GraphsageAmdError, match="FIT needs"):
        ops.logreg_eval(case.X, case.W, case.b, n=70)
    with pytest.raises(ops._lib.GraphsageAmdError, match="n_rows"):
        ops.logreg_eval(case.X, case.W, case.b, n=71, y_class=torch.zeros(71, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match=r"rows must lie in \[0, 70\)"):
        ev.fit_classifier(None, case.X, np.array([0, 70]), np.array([0, 1]))


# ------------------------------------------------------------------------------------------------ 2. repeatability
@pytest.mark.parametrize("n,d,c", [(70, 36, 5), (20000, 36, 33), (150, 512, 128)])
def test_same_call_twice_same_bits(dev, n, d, c):
    case = Case(dev, n, d, c, False, rows="repeat")
    a = [t.cpu().numpy().copy() for t in case.fit()]
    b = [t.cpu().numpy().copy() for t in case.fit()]
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))


# ------------------------------------------------------------------------------------------------ 3. optimality
_FITS = {}


def fitted(dev, name):
    """The fixture, its targets and ONE device fit with the defaults, shared by the tests below."""
    if name not in _FITS:
        fx = dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))
        c = fx["W_star"].shape[1]
        multi = fx["y_train"].ndim == 2
        clf = ev.fit_classifier(None, fx["X_train"], None, fx["y_train"], n_classes=None if multi else c)
        _FITS[name] = (fx, ev.targets(fx["y_train"], None if multi else c)[0], clf)
    return _FITS[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_fit_twice_same_bits(dev, name):
    fx, S, clf = fitted(dev, name)
    again = ev.fit_classifier(None, fx["X_train"], None, fx["y_train"], n_classes=clf.n_classes)
    assert np.array_equal(clf.W.view(np.int32), again.W.view(np.int32)) and np.array_equal(clf.b.view(np.int32), again.b.view(np.int32))
    assert np.array_equal(clf.loss.view(np.int64), again.loss.view(np.int64)) and (clf.evals, clf.stop) == (again.evals, again.stop)


@pytest.mark.parametrize("name", FIXTURES)
def test_fit_against_reference_and_optimum(dev, name):
    """Per class, with the objective re-evaluated in fp64: (a) not above the reference's SGD (convexity: no margin), (b) within
    1e-4 relative of the fp64 optimum, (c) predictions on the test part equal to the optimum's wherever its fp64 margin
    exceeds 1e-4 (at most 1 % left out).  The reference's printed F1 goes into the message; SGD stops short of the optimum, so
    it is not asserted equal."""
    fx, S, clf = fitted(dev, name)
    multi = fx["y_train"].ndim == 2
    assert clf.W.dtype == np.float32 and clf.b.dtype == np.float32 and clf.loss.dtype == np.float64
    assert clf.stop in ("gtol", "noise") and 1 < clf.evals <= 1000
    J = ev.objective(fx["X_train"], S, clf.W, clf.b)
    gap = (J - fx["J_star"]) / fx["J_star"]
    score = clf.score(fx["X_test"], None, fx["y_test"])
    msg = "%s: evals %d stop %s, J - J* rel %s, J_ref - J %s; device f1_micro %.4f accuracy %s | reference printed %s" % (
        name, clf.evals, clf.stop, gap, fx["J_ref"] - J, score["f1_micro"], score["accuracy"], fx["ref_f1_test"])
    print(msg)
    assert np.allclose(clf.loss, J, rtol=1e-4, atol=0), msg               # what the solver reports is the objective
    assert (J <= fx["J_ref"]).all(), msg                                   # (a)
    assert (J - fx["J_star"] <= 1e-4 * fx["J_star"]).all(), msg            # (b)
    z = fx["X_test"].astype(np.float64).dot(fx["W_star"]) + fx["b_star"]   # (c)
    pred = clf.predict(fx["X_test"])
    if multi:
        sure = np.abs(z) > MARGIN
        assert pred.shape == z.shape and np.array_equal(pred[sure], (z > 0).astype(np.uint8)[sure]), msg
    else:
        srt = np.sort(z, axis=1)
        sure = srt[:, -1] - srt[:, -2] > MARGIN
        assert pred.shape == (z.shape[0],) and np.array_equal(pred[sure], z.argmax(axis=1)[sure]), msg
    assert (~sure).mean() <= 0.01, msg
    assert np.array_equal(score["pred"], pred)
    # the scores are the host's integer counts on those predictions
    from graphsage_amd.supervised_train import f1_micro_macro
    assert (score["f1_micro"], score["f1_macro"]) == f1_micro_macro(fx["y_test"], pred, multi)
    held = ev.objective(fx["X_test"], ev.targets(fx["y_test"], None if multi else clf.n_classes)[0], clf.W, clf.b, alpha=0.0)
    assert np.abs(score["loss"] - held).max() <= 1e-4 * max(1.0, held.max()), msg


def test_rows_subset_and_unpadded_width(dev):
    """fit / predict through `rows` of a larger table equals the fit on the gathered rows, bit for bit; a width that is no
    multiple of 4 is padded with zero columns."""
    fx, S, clf = fitted(dev, "ref_eval_multiclass")
    n, d = fx["X_train"].shape
    rng = np.random.RandomState(5)
    table = rng.randn(n + 40, d).astype(np.float32)
    rows = rng.permutation(n + 40)[:n]
    table[rows] = fx["X_train"]
    via = ev.fit_classifier(None, table, rows, fx["y_train"], n_classes=clf.n_classes)
    assert np.array_equal(via.W.view(np.int32), clf.W.view(np.int32)) and via.evals == clf.evals
    odd = ev.fit_classifier(None, fx["X_train"][:, :30], None, fx["y_train"], n_classes=clf.n_classes, max_evals=40)
    assert odd.W.shape == (30, clf.n_classes) and odd.stop == "max_evals" and odd.evals <= 40
    assert odd.predict(fx["X_test"][:, :30]).shape == (fx["X_test"].shape[0],)


# ------------------------------------------------------------------------------------------------ 4. driver
def test_unsupervised_driver_eval_classifier(dev, tmp_path, capsys):
    """--eval_classifier test prints the line and writes the file; rerunning the command gives the same line bit for bit (its
    time= field, a wall clock, aside); without the flag the other output files are the same set and the line does not appear;
    scoring the written files again gives the line once more.
    The two runs of the command are two child processes, started together: a second ut.main() in THIS process is no rerun
    (the layer-name counters and NumPy's global generator carry over from whatever ran before)."""
    import subprocess
    import sys
    from graphsage_amd import unsupervised_train as ut
    args = ["--synthetic", "small", "--epochs", "1", "--batch_size", "128", "--samples_1", "5", "--samples_2", "3", "--dim_1", "32",
            "--dim_2", "32", "--max_total_steps", "6", "--model", "graphsage_mean", "--learning_rate", "0.001",
            "--max_walk_pairs", "4000", "--validate_iter", "10", "--validate_batch_size", "256"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    procs = {run: subprocess.Popen([sys.executable, "-m", "graphsage_amd.unsupervised_train"] + args
                                   + ["--base_log_dir", str(tmp_path / run), "--eval_classifier", "test"], cwd=ROOT, env=env,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
             for run in ("on", "again")}
    eng.reset_engine()
    ut.main(args + ["--base_log_dir", str(tmp_path / "off")])
    assert "Downstream classifier" not in capsys.readouterr().out
    lines, files = {}, {}
    for run, proc in procs.items():
        out, err = proc.communicate(timeout=300)
        assert proc.returncode == 0, err[-2000:]
        found = re.findall(r"^Downstream classifier: .*$", out, flags=re.M)
        assert len(found) == 1, out[-2000:]
        lines[run] = found[0]
    for run in ("on", "again", "off"):
        files[run] = {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path / run)) for f in fs}
    assert open(files["on"]["eval_classifier.txt"]).read() == lines["on"] + "\n"
    m = re.match(r"Downstream classifier: setting= test classes= (\d+) train= (\d+) test= (\d+) f1_micro= (\d\.\d{5}) "
                 r"f1_macro= (\d\.\d{5}) train_f1_micro= (\d\.\d{5}) baseline_f1_micro= (\d\.\d{5}) loss= (\d+\.\d{6}) "
                 r"evals= (\d+) stop= (gtol|noise|max_evals) time= (\d+\.\d{5})$", lines["on"])
    assert m, lines["on"]
    assert int(m.group(1)) == 7 and int(m.group(2)) + int(m.group(3)) < 3000 and int(m.group(3)) > 0
    assert 0.0 < float(m.group(7)) < 1.0 and 0.0 <= float(m.group(4)) <= 1.0
    strip = lambda s: re.sub(r" time= \S+$", "", s)
    assert strip(lines["on"]) == strip(lines["again"])
    assert set(files["on"]) - {"eval_classifier.txt"} == set(files["off"]) and "val.npy" in files["off"]
    # the same files scored once more, in this process
    from graphsage_amd import supervised_train as st
    import argparse
    st.FLAGS = argparse.Namespace(synthetic="small", train_prefix="", sigmoid=False)
    G = st.load_graph()
    res = ev.evaluate_embedding_dir(None, G, os.path.dirname(files["on"]["val.npy"]), "test")
    assert strip(ev.result_line("test", res)) == strip(lines["on"])
    capsys.readouterr()


def test_eval_embeddings_from_files(dev, tmp_path, capsys):
    """python -m graphsage_amd.eval_embeddings DATA_PREFIX EMBED_DIR test: the dataset through utils.load_data, the train rows
    from val.npy / val.txt (any row order, ORIGINAL ids), the scored rows from val-test.npy where it exists."""
    import json
    from graphsage_amd import eval_embeddings as ee
    rng = np.random.RandomState(3)
    n, c, d = 90, 3, 8
    ids = ["n%d" % i for i in range(n)]
    cls = rng.randint(0, c, size=n)
    split = np.array(["train"] * 60 + ["val"] * 10 + ["test"] * 20)
    nodes = [{"id": ids[i], "val": bool(split[i] == "val"), "test": bool(split[i] == "test")} for i in range(n)]
    links = [{"source": int(a), "target": int(b)} for a, b in rng.randint(0, n, size=(150, 2)) if a != b]
    prefix = str(tmp_path / "toy")
    json.dump({"directed": False, "graph": {}, "nodes": nodes, "links": links, "multigraph": False}, open(prefix + "-G.json", "w"))
    json.dump({ids[i]: i for i in range(n)}, open(prefix + "-id_map.json", "w"))
    json.dump({ids[i]: int(cls[i]) for i in range(n)}, open(prefix + "-class_map.json", "w"))
    centers = rng.randn(c, d) * 4
    emb = (centers[cls] + 0.3 * rng.randn(n, d)).astype(np.float32)              # separable: the fit scores 1.0 on its rows
    out = tmp_path / "emb"
    out.mkdir()
    order = rng.permutation(n)
    np.save(str(out / "val.npy"), emb[order])
    open(str(out / "val.txt"), "w").write("\n".join(ids[i] for i in order))
    res = ee.main([prefix, str(out), "test"])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Downstream classifier:")]
    assert len(line) == 1 and open(str(out / "eval_classifier.txt")).read() == line[0] + "\n"
    assert " setting= test classes= 3 train= 60 test= 20 f1_micro= 1.00000 " in line[0] and res["train_f1_micro"] == 1.0
    assert ee.main([prefix, str(out), "val"])["test"] == 10
    # a val-test table (the node2vec baseline's) takes over the scored rows: here its rows are noise, and the score shows it
    held = np.where(split != "train")[0][::-1]
    np.save(str(out / "val-test.npy"), rng.randn(len(held), d).astype(np.float32))
    open(str(out / "val-test.txt"), "w").write("\n".join(ids[i] for i in held))
    noisy = ee.main([prefix, str(out), "test"])
    assert noisy["test"] == 20 and noisy["f1_micro"] < 1.0 and noisy["train_f1_micro"] == 1.0
    capsys.readouterr()
    # a table that lacks a node is refused with its id
    open(str(out / "val-test.txt"), "w").write("\n".join(["zz"] + [ids[i] for i in held[1:]]))
    with pytest.raises(SystemExit, match=ids[held[0]]):
        ee.main([prefix, str(out), "test"])
