"""k-means on the device against tests/kmeans_oracle.py: the fused assignment (exact on integer-valued inputs, ties included;
within the project's float tolerance on floats), the stable grouping, the centroid update through gs_csr_reduce_fwd, the Lloyd
loop of clustering.fit_kmeans, and the two drivers."""
import os
import re

import numpy as np
import pytest

import kmeans_oracle as ko

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mat(a, dev, pad=8, fill=99.0):
    """A Mat of width a.shape[1] in a buffer `pad` columns wider (ld > d); the pad columns hold `fill`: nothing may read them."""
    import torch
    from graphsage_amd.ops import Mat
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.float32, device=dev)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(dev)
    return Mat(buf, a.shape[1])


def i32(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def run_assign(dev, T, C, rows=None, prev=None):
    """kmeans_sqnorm + kmeans_assign on table T -> (assign, dist, inertia, changed, xsq, csq) on the host."""
    import torch
    from graphsage_amd import ops
    X, Cm = mat(T, dev), mat(C, dev, pad=4)
    rows_dev = i32(rows, dev) if rows is not None else None
    n = len(rows) if rows is not None else len(T)
    xsq = ops.kmeans_sqnorm(X, rows=rows_dev)
    csq = ops.kmeans_sqnorm(Cm)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    assign, _, stats = ops.kmeans_assign(X, Cm, csq, rows=rows_dev, xsq=xsq, prev=i32(prev, dev) if prev is not None else None,
                                         dist=dist)
    inertia, changed = ops.kmeans_stats(stats)
    return assign.cpu().numpy(), dist.cpu().numpy(), inertia, changed, xsq.cpu().numpy(), csq.cpu().numpy()


def integer_case(rng, n, k, d, with_rows):
    """Entries in {-3..3}, centroid entries even (|c|^2 / 2 is an integer): every fp32 sum is exact.  Duplicated centroid rows
    are planted, and rows that sit exactly between two centroids."""
    C = 2.0 * rng.randint(-1, 2, size=(k, d))
    if k >= 2:
        for _ in range(max(1, k // 8)):
            a, b = rng.randint(0, k, size=2)
            C[a] = C[b]
    n_rows = n + 5 if with_rows else n
    T = rng.randint(-3, 4, size=(n_rows, d)).astype(np.float64)
    T[rng.randint(0, n_rows, size=max(1, n_rows // 4))] = C[rng.randint(0, k, size=max(1, n_rows // 4))]      # on a centroid
    rows = None
    if with_rows:
        rows = rng.randint(0, n_rows, size=n)
        if n >= 2:
            rows[-1] = rows[0]                                                                                  # a repeated id
    return T, C, rows


@pytest.mark.parametrize("d", [4, 28, 32, 36, 256])
def test_assign_exact_on_integers(dev, d):
    rng = np.random.RandomState(100 + d)
    case = ties = 0
    for n in (1, 127, 128, 129, 300):
        for k in (1, 2, 127, 128, 129, 300):
            with_rows = bool(case % 2)
            case += 1
            T, C, rows = integer_case(rng, n, k, d, with_rows)
            X = T[rows] if rows is not None else T
            prev = rng.randint(0, k, size=n)
            want, dist64, inertia64 = ko.assign(X, C)
            got, dist, inertia, changed, xsq, csq = run_assign(dev, T, C, rows, prev)
            tag = (n, k, d, with_rows)
            assert np.array_equal(xsq, (X * X).sum(axis=1)) and np.array_equal(csq, (C * C).sum(axis=1)), tag
            assert np.array_equal(got, want), (tag, np.flatnonzero(got != want)[:5])
            assert np.array_equal(dist.astype(np.float64), dist64), tag
            assert inertia == inertia64 and changed == int((want != prev).sum()), (tag, inertia, inertia64, changed)
            # said once more without argmax: the reported id attains the maximum and no lower id does
            S = ko.scores(X, C)
            top = S == S.max(axis=1, keepdims=True)
            assert np.all(top[np.arange(n), got]) and np.array_equal(got, np.argmax(top, axis=1)), tag
            ties += int((top.sum(axis=1) > 1).sum())
    assert ties > 100                                                    # the planted duplicates do tie at the maximum


def test_assign_exact_at_the_largest_k(dev):
    rng = np.random.RandomState(7)
    n, k, d = 130, 4096, 8
    T, C, _ = integer_case(rng, n, k, d, False)
    want, dist64, inertia64 = ko.assign(T, C)
    got, dist, inertia, changed, _, _ = run_assign(dev, T, C)
    assert np.array_equal(got, want) and np.array_equal(dist.astype(np.float64), dist64) and inertia == inertia64 and changed == 0
    assert len(np.unique(C, axis=0)) < k                                 # 3^8 > 4096 but rows repeat: ties all over the sweep


def test_assign_without_xsq_prev_and_dist(dev):
    from graphsage_amd import ops
    rng = np.random.RandomState(8)
    T, C, _ = integer_case(rng, 200, 5, 12, False)
    X, Cm = mat(T, dev), mat(C, dev)
    assign, dist, stats = ops.kmeans_assign(X, Cm, ops.kmeans_sqnorm(Cm))
    want, _, _ = ko.assign(T, C)
    S = ko.scores(T, C)
    assert dist is None and np.array_equal(assign.cpu().numpy(), want)
    inertia, changed = ops.kmeans_stats(stats)
    assert changed == 0 and inertia == float(np.maximum(0.0, -2.0 * S.max(axis=1)).sum())      # xsq taken as 0


FLOAT_SHAPES = [(300, 300, 4), (129, 129, 36), (257, 127, 256), (300, 2, 512), (4099, 1030, 64)]


@pytest.mark.parametrize("n,k,d", FLOAT_SHAPES)
def test_assign_floats(dev, n, k, d):
    rng = np.random.RandomState(n + k + d)
    C = rng.randn(k, d).astype(np.float32)
    label = rng.randint(0, k, size=n)
    X = (C[label] + 0.05 * rng.randn(n, d)).astype(np.float32)
    best, second, margin = ko.margins(X, C)
    xsq64, csq64 = (X.astype(np.float64) ** 2).sum(axis=1), (C.astype(np.float64) ** 2).sum(axis=1)
    clear = margin > 1e-4 * (xsq64 + csq64.max())
    print("rows under the margin: %d of %d (%.2f %%)" % ((~clear).sum(), n, 100.0 * (~clear).mean()))
    assert (~clear).mean() <= 0.01                                        # on the oracle alone
    got, dist, inertia, changed, xsq, _ = run_assign(dev, X, C)
    assert np.array_equal(got[clear], best[clear])
    assert np.all((got == best) | (got == second))
    assert got.min() >= 0 and got.max() < k
    dist64 = ((X.astype(np.float64) - C.astype(np.float64)[got]) ** 2).sum(axis=1)
    err = np.abs(dist - dist64)
    tol = 1e-4 * (xsq64 + csq64[got])
    print("max |dist - dist64| / tol = %.3g" % (err / tol).max())
    assert np.all(err <= tol)
    own = dist.astype(np.float64).sum()
    print("inertia %.9g, fp64 sum of the kernel's dist %.9g" % (inertia, own))
    assert abs(inertia - own) <= 1e-5 * own and changed == 0
    assert np.allclose(xsq, xsq64, rtol=1e-5)


def test_assign_is_bitwise_repeatable_and_duplicates_score_equal(dev):
    rng = np.random.RandomState(11)
    C = rng.randn(200, 40).astype(np.float32)
    C[150] = C[3]                                                        # bit-identical rows in different tiles and lanes
    C[77] = C[140]
    X = np.concatenate([C[[3, 140, 150, 77]], rng.randn(296, 40).astype(np.float32)])
    a = run_assign(dev, X, C)
    b = run_assign(dev, X, C)
    assert a[0][:4].tolist() == [3, 77, 3, 77]                            # an exact tie between two tiles: the lowest id
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


# ------------------------------------------------------------------------------------------------ members
@pytest.mark.parametrize("k", [1, 3, 4096])
def test_members(dev, k):
    from graphsage_amd import ops
    rng = np.random.RandomState(k)
    for n in (1, 63, 64, 65, 5000):
        cases = [rng.randint(0, k, size=n), np.full(n, k - 1), np.full(n, 0)]
        if k >= 3:
            cases.append(rng.choice([0, k - 1], size=n))                  # every other cluster is empty
        for ci, labels in enumerate(cases):
            rows = rng.randint(0, 10 ** 6, size=n) if ci % 2 else None
            want_ptr, want_mem = ko.members(labels, k, rows)
            assert np.array_equal(np.diff(want_ptr), np.bincount(labels, minlength=k))
            outs = []
            for chunk in (0, 64, 128):
                rowptr, members = ops.kmeans_members(i32(labels, dev), k, rows=i32(rows, dev) if rows is not None else None,
                                                     chunk=chunk)
                outs.append((rowptr.cpu().numpy(), members.cpu().numpy()))
                assert np.array_equal(outs[-1][0], want_ptr) and np.array_equal(outs[-1][1], want_mem), (n, k, ci, chunk)
            if rows is None:
                assert np.array_equal(outs[0][1], np.argsort(labels, kind="stable"))


# ------------------------------------------------------------------------------------------------ update
def test_update_through_csr_reduce(dev):
    import torch
    from graphsage_amd import clustering as cl
    from graphsage_amd import ops
    rng = np.random.RandomState(21)
    n, k, d = 1500, 5, 20
    X = rng.randn(n, d).astype(np.float32)
    labels = np.concatenate([np.zeros(700), rng.choice([1, 3, 4], size=n - 700)]).astype(np.int32)      # 0: cut at 512; 2: empty
    rng.shuffle(labels)
    C = rng.randn(k, d).astype(np.float32)
    p = cl._Problem(None, X, None)
    Cm = p.centres(C)
    C_next = ops.Mat(torch.zeros_like(Cm.buf), Cm.d)
    scratch = {"rowptr": None, "members": None, "members_ws": None}
    sizes = cl._update(p, Cm, C_next, i32(labels, dev), scratch)
    assert sizes.tolist() == np.bincount(labels, minlength=k).tolist() and sizes[0] == 700 and sizes[2] == 0
    got = C_next.buf[:, :d].cpu().numpy()
    want = ko.update(X, labels, C)
    err = np.abs(got - want).max()
    print("max |mean - mean64| = %.3g (bound %.3g)" % (err, 1e-5 * np.abs(X).max()))
    assert err <= 1e-5 * np.abs(X).max()
    assert got[2].tobytes() == C[2].tobytes()                            # the empty cluster keeps its centre bit for bit


# ------------------------------------------------------------------------------------------------ fit
def blobs(rng, n, k, d, spread=0.3):
    centres = 4.0 * rng.randn(k, d)
    label = rng.randint(0, k, size=n)
    return (centres[label] + spread * rng.randn(n, d)).astype(np.float32), label, centres


def test_fit_follows_the_oracle(dev):
    from graphsage_amd import clustering as cl
    rng = np.random.RandomState(31)
    X, label, _ = blobs(rng, 1000, 7, 32)
    init = X[rng.choice(1000, size=7, replace=False)]                     # data points: blobs may share a seed or have none
    C64, lab64, inertia64, iters64, stop64, hist64 = ko.fit(X, init)
    fit = cl.fit_kmeans(None, X, 7, init=init, keep_history=True)
    print("iters %d stop %s inertia %.6f (oracle %.6f)" % (fit.iters, fit.stop, fit.inertia, inertia64))
    assert fit.iters == iters64 and fit.stop == stop64 and iters64 >= 2
    assert len(fit.history) == len(hist64) and all(np.array_equal(a, b) for a, b in zip(fit.history, hist64))
    assert np.array_equal(fit.labels, lab64) and fit.labels.dtype == np.int32
    assert fit.centers.dtype == np.float32 and fit.centers.shape == (7, 32)
    assert np.abs(fit.centers - C64).max() <= 1e-5 * max(1.0, np.abs(C64).max())
    assert abs(fit.inertia - inertia64) <= 1e-4 * inertia64
    assert np.array_equal(fit.sizes, np.bincount(lab64, minlength=7)) and fit.empty == int((fit.sizes == 0).sum())
    assert np.array_equal(fit.predict(X), fit.labels)                     # bit for bit: the labels ARE the assignment to centers
    sub = np.array([5, 5, 999, 0, 17])
    assert np.array_equal(fit.predict(X, rows=sub), fit.labels[sub])
    again = cl.fit_kmeans(None, X, 7, init=init)
    assert again.centers.tobytes() == fit.centers.tobytes() and again.labels.tobytes() == fit.labels.tobytes()
    assert again.inertia == fit.inertia and again.iters == fit.iters
    one = cl.fit_kmeans(None, X, 7, init=init, max_iter=1)
    assert (one.iters, one.stop) == (1, "max_iter") and np.array_equal(one.labels, hist64[0])
    assert np.array_equal(one.centers, init)
    # rows: a fit on a subset is the fit on the gathered table
    rows = rng.choice(1000, size=400, replace=False)
    a, b = cl.fit_kmeans(None, X, 7, rows=rows, init=init), cl.fit_kmeans(None, X[rows], 7, init=init)
    assert a.centers.tobytes() == b.centers.tobytes() and np.array_equal(a.labels, b.labels)


def test_fit_one_cluster_and_refusals(dev):
    from graphsage_amd import clustering as cl
    from graphsage_amd._lib import GraphsageAmdError
    rng = np.random.RandomState(32)
    X = rng.randn(333, 10).astype(np.float32)                             # width 10: padded to 12 on the device
    fit = cl.fit_kmeans(None, X, 1, init=X[:1])
    assert (fit.iters, fit.stop) == (2, "converged") and not fit.labels.any() and fit.sizes.tolist() == [333]
    assert fit.centers.shape == (1, 10) and np.abs(fit.centers[0] - X.astype(np.float64).mean(axis=0)).max() <= 1e-5
    want = ((X.astype(np.float64) - X.astype(np.float64).mean(axis=0)) ** 2).sum()
    assert abs(fit.inertia - want) <= 1e-4 * want
    for k, kw, word in ((334, {}, "k=334"), (0, {}, "k=0"), (3, {"init": "random"}, "init"), (3, {"init": X[:2]}, "init"),
                        (3, {"max_iter": 0}, "max_iter")):
        with pytest.raises(GraphsageAmdError, match=word):
            cl.fit_kmeans(None, X, k, **kw)
    with pytest.raises(GraphsageAmdError, match="distinct"):
        cl.fit_kmeans(None, np.repeat(X[:2], 10, axis=0), 3)


def test_fit_kmeanspp_reproduces_the_oracles_seeds(dev):
    from graphsage_amd import clustering as cl
    rng = np.random.RandomState(33)
    X, label, _ = blobs(rng, 5000, 5, 16)                                 # 5000 > 4096: the subsample is drawn
    for seed in (123, 7):
        fit = cl.fit_kmeans(None, X, 5, seed=seed, max_iter=1)
        want = ko.seeds(X, 5, seed)
        assert np.array_equal(fit.seeds, want) and np.array_equal(fit.centers, X[want])
    rows = rng.permutation(5000)[:4500]
    fit = cl.fit_kmeans(None, X, 5, rows=rows, seed=5, max_iter=1)
    assert np.array_equal(fit.seeds, ko.seeds(X[rows], 5, 5))
    full = cl.fit_kmeans(None, X, 5, seed=123)
    got = cl.cluster_metrics(full.labels, label)
    assert got == ko.metrics(full.labels, label) or all(abs(got[m] - ko.metrics(full.labels, label)[m]) < 1e-12 for m in got)
    assert full.stop in ("converged", "tol") and got["purity"] > 0.5


# ------------------------------------------------------------------------------------------------ drivers
LINE = (r"^Embedding clusters: k= (\d+) nodes= (\d+) inertia= (\d+\.\d{6}) iters= (\d+) stop= (converged|tol|max_iter) empty= (\d+) "
        r"size_min= (\d+) size_max= (\d+) nmi= (\d\.\d{5}) ari= (-?\d\.\d{5}) purity= (\d\.\d{5}) time= (\d+\.\d{5})$")


def write_synthetic_prefix(prefix):
    """The dataset of --synthetic small in the reference's on-disk format (what eval_embeddings reads)."""
    import json
    from graphsage_amd import utils
    G = utils.synthetic_graph(n_nodes=3000, feat_dim=50, num_classes=7, avg_degree=8, seed=123, multilabel=False)
    nodes = [{"id": i, "val": bool(G.val_mask[i]), "test": bool(G.test_mask[i])} for i in range(G.n_nodes)]
    json.dump({"directed": False, "graph": {}, "nodes": nodes, "links": [], "multigraph": False}, open(prefix + "-G.json", "w"))
    json.dump({str(i): i for i in range(G.n_nodes)}, open(prefix + "-id_map.json", "w"))
    json.dump({str(i): int(G.labels[i]) for i in range(G.n_nodes)}, open(prefix + "-class_map.json", "w"))
    return G


def test_drivers_eval_clusters(dev, tmp_path, capsys):
    """--eval_clusters -1 next to --eval_classifier test: the line, its file, clusters.npy and cluster_centers.npy appear and
    every other output is what a run without the flag writes (time= aside).  Two child processes, started together; then
    eval_embeddings --clusters on the first run's directory prints the same line."""
    import subprocess
    import sys
    args = ["--synthetic", "small", "--epochs", "1", "--batch_size", "128", "--samples_1", "5", "--samples_2", "3", "--dim_1", "32",
            "--dim_2", "32", "--max_total_steps", "6", "--model", "graphsage_mean", "--learning_rate", "0.001",
            "--max_walk_pairs", "4000", "--validate_iter", "10", "--validate_batch_size", "256", "--eval_classifier", "test"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    extra = {"clusters": ["--eval_clusters", "-1"], "plain": []}
    procs = {run: subprocess.Popen([sys.executable, "-m", "graphsage_amd.unsupervised_train"] + args + extra[run]
                                   + ["--base_log_dir", str(tmp_path / run)], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                   stderr=subprocess.PIPE, universal_newlines=True) for run in ("clusters", "plain")}
    outs, files = {}, {}
    for run, proc in procs.items():
        out, err = proc.communicate(timeout=300)
        assert proc.returncode == 0, err[-2000:]
        outs[run] = out
        files[run] = {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path / run)) for f in fs}
    found = re.findall(r"^Embedding clusters: .*$", outs["clusters"], flags=re.M)
    assert len(found) == 1 and not re.findall(r"^Embedding clusters", outs["plain"], flags=re.M), outs["clusters"][-2000:]
    m = re.match(LINE, found[0])
    assert m, found[0]
    assert outs["clusters"].index("Downstream classifier:") < outs["clusters"].index(found[0])
    new = {"eval_clusters.txt", "clusters.npy", "cluster_centers.npy"}
    assert set(files["clusters"]) - new == set(files["plain"]) and new <= set(files["clusters"])
    assert open(files["clusters"]["eval_clusters.txt"]).read() == found[0] + "\n"
    val = np.load(files["clusters"]["val.npy"])
    labels, centres = np.load(files["clusters"]["clusters.npy"]), np.load(files["clusters"]["cluster_centers.npy"])
    k = int(m.group(1))
    assert k == 7 and int(m.group(2)) == val.shape[0]
    assert labels.dtype == np.int32 and labels.shape == (val.shape[0],) and labels.min() >= 0 and labels.max() < k
    assert centres.dtype == np.float32 and centres.shape == (k, val.shape[1]) and val.shape[1] == 64
    sizes = np.bincount(labels, minlength=k)
    assert (int(m.group(6)), int(m.group(7)), int(m.group(8))) == (int((sizes == 0).sum()), sizes.min(), sizes.max())
    # every other output of the two runs is byte-identical, time= fields aside
    strip = lambda b: re.sub(br" time= \S+", b"", b)
    for f, path in files["plain"].items():
        a, b = open(path, "rb").read(), open(files["clusters"][f], "rb").read()
        assert (a == b) if f.endswith(".npy") else (strip(a) == strip(b)), f
    # the scores are the ones of the labels in the file, against the classes of the nodes val.txt names
    G = write_synthetic_prefix(str(tmp_path / "small"))
    order = np.array([int(s) for s in open(files["clusters"]["val.txt"]).read().split()])
    want = ko.metrics(labels, G.labels[order])
    assert abs(float(m.group(9)) - want["nmi"]) < 1e-5 and abs(float(m.group(10)) - want["ari"]) < 1e-5
    assert abs(float(m.group(11)) - want["purity"]) < 1e-5
    # ... and the labels are the assignment to the centres in the file: no centre is nearer than the one named, in fp64
    d2 = ((val.astype(np.float64)[:, None, :] - centres.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    slack = 1e-4 * ((val.astype(np.float64) ** 2).sum(axis=1) + (centres.astype(np.float64) ** 2).sum(axis=1).max())
    assert np.all(d2[np.arange(len(val)), labels] <= d2.min(axis=1) + slack)

    from graphsage_amd import eval_embeddings as ee
    capsys.readouterr()
    res = ee.main([str(tmp_path / "small"), os.path.dirname(files["clusters"]["val.npy"]), "val", "--clusters", "-1"])
    again = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Embedding clusters:")]
    cut = lambda s: re.sub(r" time= \S+$", "", s)
    assert len(again) == 1 and cut(again[0]) == cut(found[0])
    assert np.array_equal(np.load(files["clusters"]["clusters.npy"]), labels) and res["k"] == 7
