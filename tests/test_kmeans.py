"""k-means and the partition scores without a GPU: the NumPy oracle against brute force, the metrics on hand-computed tables,
the seeding stream, the drivers' flags and refusals, the C ABI of csrc/gs_kmeans.hip against the binding's mirrors."""
import ctypes
import os
import re

import numpy as np
import pytest

import kmeans_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("n,k,d,seed", [(1, 1, 4, 0), (7, 3, 4, 1), (40, 5, 8, 2), (33, 33, 3, 3)])
def test_oracle_assign_is_the_nearest_centre(n, k, d, seed):
    rng = np.random.RandomState(seed)
    X, C = rng.randn(n, d), rng.randn(k, d)
    brute = ((X[:, None, :] - C[None, :, :]) ** 2).sum(axis=2)
    labels, dist, inertia = ko.assign(X, C)
    assert np.array_equal(labels, np.argmin(brute, axis=1))
    assert np.allclose(dist, brute.min(axis=1), rtol=1e-12, atol=1e-12) and abs(inertia - brute.min(axis=1).sum()) < 1e-9


def test_oracle_ties_members_update_and_stops():
    X = np.array([[1.0, 0.0], [0.0, 1.0], [3.0, 3.0], [1.0, 0.0]])
    C = np.array([[3.0, 3.0], [0.0, 0.0], [0.0, 0.0], [3.0, 3.0]])       # 0 == 3 and 1 == 2: a tie goes to the lowest id
    labels, dist, _ = ko.assign(X, C)
    assert labels.tolist() == [1, 1, 0, 1] and dist.tolist() == [1.0, 1.0, 0.0, 1.0]
    rowptr, mem = ko.members(labels, 4)
    assert rowptr.tolist() == [0, 1, 4, 4, 4] and mem.tolist() == [2, 0, 1, 3]
    rowptr, mem = ko.members(labels, 4, rows=np.array([9, 8, 7, 9]))
    assert mem.tolist() == [7, 9, 8, 9]
    C1 = ko.update(X, labels, C)
    assert np.array_equal(C1[0], [3.0, 3.0]) and np.allclose(C1[1], [2.0 / 3, 1.0 / 3])
    assert np.array_equal(C1[2], C[2]) and np.array_equal(C1[3], C[3])   # empty clusters keep their centres
    # stops: nothing moves on the second assignment; one assignment allowed; a loose tolerance
    blobs = np.concatenate([np.random.RandomState(0).randn(30, 2) * 0.1 + c for c in ([0, 0], [5, 5], [0, 5])])
    init = blobs[[0, 30, 60]]
    C2, lab, inertia, iters, stop, hist = ko.fit(blobs, init)
    assert stop == "converged" and iters == 2 and len(hist) == 2 and np.array_equal(hist[0], hist[1])
    assert np.array_equal(lab, np.repeat([0, 1, 2], 30)) and np.allclose(C2, [blobs[:30].mean(0), blobs[30:60].mean(0), blobs[60:].mean(0)])
    assert ko.fit(blobs, init, max_iter=1)[3:5] == (1, "max_iter")
    rng = np.random.RandomState(1)
    cloud = rng.randn(400, 2)
    assert ko.fit(cloud, cloud[:6], tol=0.9)[3:5] == (2, "tol")          # no step from data points gains nine tenths
    assert ko.fit(blobs[:1], blobs[:1])[3:5] == (2, "converged")


def test_library_host_functions_follow_the_oracle():
    from graphsage_amd import clustering as cl
    rng = np.random.RandomState(5)
    for n, k in ((50, 5), (5000, 3), (5000, 200)):
        a, b = cl.seed_subsample(n, k, np.random.RandomState(9)), ko.seed_subsample(n, k, np.random.RandomState(9))
        assert np.array_equal(a, b) and len(a) == min(n, max(4096, 32 * k)) and np.all(np.diff(a) > 0)
    P = rng.randn(300, 6)
    for seed in (0, 1, 123):
        assert np.array_equal(cl.kmeanspp(P, 12, np.random.RandomState(seed)), ko.kmeanspp(P, 12, np.random.RandomState(seed)))
    for _ in range(5):
        pred, true = rng.randint(0, 6, size=200), rng.randint(0, 4, size=200)
        got, want = cl.cluster_metrics(pred, true), ko.metrics(pred, true)
        assert all(abs(got[m] - want[m]) < 1e-12 for m in ("nmi", "ari", "purity"))


# ------------------------------------------------------------------------------------------------ metrics
def test_metrics_on_hand_computed_tables():
    from graphsage_amd.clustering import cluster_metrics, contingency
    true = np.array([0, 0, 1, 1, 2, 2, 2])
    same = cluster_metrics(true, true)
    assert same == {"nmi": 1.0, "ari": 1.0, "purity": 1.0} or all(abs(v - 1.0) < 1e-12 for v in same.values())
    relabelled = cluster_metrics(np.array([5, 5, 9, 9, 1, 1, 1]), true)
    assert all(abs(v - 1.0) < 1e-12 for v in relabelled.values())
    # independent partitions: every cell of the table holds the product of its margins -> MI = 0 exactly, ARI ~ 0
    t = np.repeat(np.arange(4), 300)
    p = np.tile(np.arange(3), 400)
    ind = cluster_metrics(p, t)
    # ARI: sum C(100, 2) = 59,400 against the expected 179,400 * 239,400 / 719,400 = 59,700.25 -> -300.25 / 149,699.75
    assert abs(ind["nmi"]) < 1e-12 and abs(ind["ari"] + 300.25 / 149699.75) < 1e-6 and abs(ind["purity"] - 0.25) < 1e-12
    # one class on a side
    assert cluster_metrics(np.zeros(5, int), np.zeros(5, int))["nmi"] == 1.0
    assert cluster_metrics(np.zeros(5, int), np.arange(5))["nmi"] == 0.0
    assert cluster_metrics(np.arange(5), np.zeros(5, int))["nmi"] == 0.0
    # a fixed 3 x 3 table (rows: classes, columns: clusters), the values written out:
    #   [[5, 1, 0], [1, 4, 1], [0, 2, 6]]   n = 20, class margins 6, 6, 8, cluster margins 6, 7, 7
    tab = np.array([[5, 1, 0], [1, 4, 1], [0, 2, 6]])
    true3 = np.concatenate([np.full(tab[i].sum(), i) for i in range(3)])
    pred3 = np.concatenate([np.repeat(np.arange(3), tab[i]) for i in range(3)])
    assert np.array_equal(contingency(pred3, true3), tab)
    got = cluster_metrics(pred3, true3)
    # purity = (5 + 4 + 6) / 20
    assert abs(got["purity"] - 0.75) < 1e-15
    # ARI: sum C(nij, 2) = 10 + 6 + 1 + 15 = 32; classes 15 + 15 + 28 = 58; clusters 15 + 21 + 21 = 57; C(20, 2) = 190
    #      expected = 58 * 57 / 190 = 17.4; (32 - 17.4) / (57.5 - 17.4) = 14.6 / 40.1
    assert abs(got["ari"] - 14.6 / 40.1) < 1e-12
    # NMI: MI = sum nij / n * ln(n nij / (a_i b_j)), H over the margins, arithmetic mean
    mi = sum(x / 20.0 * np.log(20.0 * x / (a * b)) for x, a, b in ((5, 6, 6), (1, 6, 7), (1, 6, 6), (4, 6, 7), (1, 6, 7), (2, 8, 7), (6, 8, 7)))
    h = lambda m: -sum(x / 20.0 * np.log(x / 20.0) for x in m)
    assert abs(got["nmi"] - mi / (0.5 * (h((6, 6, 8)) + h((6, 7, 7))))) < 1e-12
    assert abs(got["nmi"] - 0.4354) < 1e-4                                # the hand formula's value: 0.43543
    with pytest.raises(ValueError):
        cluster_metrics(np.arange(3), np.arange(4))


def test_module_imports_no_scipy_or_sklearn():
    src = open(os.path.join(ROOT, "graphsage_amd", "clustering.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn)", src, flags=re.M)


# ------------------------------------------------------------------------------------------------ seeding
def test_seeding_stream():
    from graphsage_amd import clustering as cl
    from graphsage_amd._lib import GraphsageAmdError
    X = np.random.RandomState(0).randn(6000, 5)
    a, b, c = ko.seeds(X, 10, 123), ko.seeds(X, 10, 123), ko.seeds(X, 10, 124)
    assert np.array_equal(a, b) and not np.array_equal(a, c) and len(set(a.tolist())) == 10
    assert a.min() >= 0 and a.max() < 6000
    sub = cl.seed_subsample(6000, 10, np.random.RandomState(123))
    assert len(sub) == 4096 and set(a.tolist()) <= set(sub.tolist())
    # fewer than k distinct rows in the subsample: refused
    dup = np.repeat(np.arange(3.0)[:, None], 20, axis=0).repeat(4, axis=1)
    assert len(np.unique(dup, axis=0)) == 3
    assert len(cl.kmeanspp(dup, 3, np.random.RandomState(0))) == 3
    with pytest.raises(GraphsageAmdError, match="distinct"):
        cl.kmeanspp(dup, 4, np.random.RandomState(0))
    with pytest.raises(ValueError):
        ko.kmeanspp(dup, 4, np.random.RandomState(0))
    with pytest.raises(GraphsageAmdError):
        cl.kmeanspp(dup[:2], 3, np.random.RandomState(0))


# ------------------------------------------------------------------------------------------------ flags and refusals
def write_toy(prefix, n=12, multilabel=False):
    import json
    ids = ["n%d" % i for i in range(n)]
    nodes = [{"id": ids[i], "val": i % 4 == 2, "test": i % 4 == 3} for i in range(n)]
    links = [{"source": i, "target": (i + 1) % n} for i in range(n)]
    json.dump({"directed": False, "graph": {}, "nodes": nodes, "links": links, "multigraph": False}, open(prefix + "-G.json", "w"))
    json.dump({ids[i]: i for i in range(n)}, open(prefix + "-id_map.json", "w"))
    json.dump({ids[i]: ([i % 2, 1] if multilabel else i % 3) for i in range(n)}, open(prefix + "-class_map.json", "w"))


def test_flag_parsing_and_driver_refusals(capsys, tmp_path):
    from graphsage_amd import clustering as cl
    from graphsage_amd import unsupervised_train as ut
    f = ut.build_flags([])
    assert f.eval_clusters == 0 and f.eval_clusters_seed == 123
    f = ut.build_flags(["--eval_clusters", "-1", "--eval_clusters_seed", "7"])
    assert f.eval_clusters == -1 and f.eval_clusters_seed == 7
    assert ut.build_flags(["--eval_clusters", "41"]).eval_clusters == 41
    with pytest.raises(SystemExit):
        ut.build_flags(["--eval_clusters", "many"])
    capsys.readouterr()
    assert ut.refuse_eval_clusters(ut.build_flags(["--save_embeddings", "false", "--dim_2", "600"])) == 0   # flag off: nothing refused

    # refused before the data is loaded
    for argv, word in ((["--eval_clusters", "5", "--save_embeddings", "false"], "--save_embeddings"),
                       (["--eval_clusters", "4097"], "4096"), (["--eval_clusters", "-2"], "4096"),
                       (["--eval_clusters", "5", "--dim_2", "516"], "1032"),
                       (["--eval_clusters", "5", "--model", "n2v", "--dim_1", "514"], "1028")):
        with pytest.raises(SystemExit) as ei:
            ut.main(["--synthetic", "small"] + argv)
        assert "--eval_clusters" in str(ei.value) and word in str(ei.value), str(ei.value)
        assert "Loading training data" not in capsys.readouterr().out
    with pytest.raises(SystemExit) as ei:
        ut.main(["--synthetic", "ppi", "--eval_clusters", "-1"])
    assert "single-label" in str(ei.value) and "Loading training data" not in capsys.readouterr().out
    ut.refuse_eval_clusters(ut.build_flags(["--synthetic", "ppi", "--eval_clusters", "5"]))
    ut.refuse_eval_clusters(ut.build_flags(["--synthetic", "small", "--eval_clusters", "-1", "--dim_2", "512"]))

    # refused once the graph is loaded: -1 without single-label classes, more clusters than nodes
    class G(object):
        labels = None
        n_nodes = 10
        present = np.ones(10, dtype=bool)
    minus1, five, eleven = (ut.build_flags(["--eval_clusters", k]) for k in ("-1", "5", "11"))
    with pytest.raises(SystemExit, match="single-label"):
        ut.refuse_eval_clusters(minus1, G())
    assert ut.refuse_eval_clusters(five, G()) == 5                        # a given K needs no labels
    G.labels = np.zeros((10, 121), dtype=np.float32)
    with pytest.raises(SystemExit, match="single-label"):
        ut.refuse_eval_clusters(minus1, G())
    G.labels = np.array([0, 1, 2, 6, 1, 1, 0, 0, 3, 3])
    assert ut.refuse_eval_clusters(minus1, G()) == 7
    with pytest.raises(SystemExit, match="more clusters than the graph's 10 nodes"):
        ut.refuse_eval_clusters(eleven, G())
    G.present = np.arange(10) < 4
    with pytest.raises(SystemExit, match="4 nodes"):
        ut.refuse_eval_clusters(five, G())
    assert cl.single_label_classes(G()) == 7

    with pytest.raises(ValueError, match="k=0"):
        cl.refuse(0)
    with pytest.raises(ValueError, match="k=4097"):
        cl.refuse(4097)
    with pytest.raises(ValueError, match="width 1026"):
        cl.refuse(3, 1026)
    with pytest.raises(ValueError, match="of 2 rows"):
        cl.refuse(3, 8, 2)
    cl.refuse(4096, 1024, 4096)
    cl.refuse(1, 1021)

    from graphsage_amd import eval_embeddings as ee
    f = ee.build_flags(["data/ppi", "unsup-ppi/x", "test"])
    assert f.clusters == 0 and f.clusters_seed == 123
    f = ee.build_flags(["data/ppi", "unsup-ppi/x", "val", "--clusters", "-1", "--clusters_seed", "5", "--table", "val_full"])
    assert (f.clusters, f.clusters_seed, f.table) == (-1, 5, "val_full")
    with pytest.raises(SystemExit, match="4096"):
        ee.main(["data/none", str(tmp_path), "test", "--clusters", "5000"])
    assert "Loading data" not in capsys.readouterr().out
    multi = str(tmp_path / "multi")
    write_toy(multi, multilabel=True)
    with pytest.raises(SystemExit, match="single-label"):
        ee.main([multi, str(tmp_path), "test", "--clusters", "-1"])
    single = str(tmp_path / "single")
    write_toy(single)
    with pytest.raises(SystemExit, match="12 nodes"):
        ee.main([single, str(tmp_path), "test", "--clusters", "13"])
    capsys.readouterr()

    line = cl.result_line({"k": 7, "nodes": 3000, "inertia": 12.5, "iters": 9, "stop": "converged", "empty": 0, "size_min": 3,
                           "size_max": 900, "nmi": float("nan"), "ari": float("nan"), "purity": float("nan"), "time": 0.25})
    assert line == ("Embedding clusters: k= 7 nodes= 3000 inertia= 12.500000 iters= 9 stop= converged empty= 0 size_min= 3 "
                    "size_max= 900 nmi= nan ari= nan purity= nan time= 0.25000")


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_binding_and_error_reporting():
    from graphsage_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    names = ("gs_kmeans_sqnorm", "gs_kmeans_assign_ws_bytes", "gs_kmeans_assign", "gs_kmeans_members_ws_bytes", "gs_kmeans_members")
    for name in names:
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"typedef struct gs_kmeans_desc \{", header) and re.search(r"typedef struct gs_kmeans_members_desc \{", header)
    version = int(re.search(r"#define GS_ABI_VERSION (\d+)\b", header).group(1))
    lib = _lib.load()
    assert lib.gs_abi_version() == version == _lib.GS_ABI_VERSION == 12   # entry points were added, no layout changed
    sizes = (ctypes.c_int32 * 16)()
    assert lib.gs_abi_struct_sizes(sizes, 16) == 8                        # the descriptors go by pointer
    assert ctypes.sizeof(_lib.KmeansDesc) == 128 and ctypes.sizeof(_lib.KmeansMembersDesc) == 72
    for macro, value in (("GS_KMEANS_MAX_K", _lib.KMEANS_MAX_K), ("GS_KMEANS_CHUNK", _lib.KMEANS_CHUNK)):
        assert int(re.search(r"#define %s (\d+)\b" % macro, header).group(1)) == value
    assert ops.KMEANS_MAX_K == 4096
    src = open(os.path.join(ROOT, "graphsage_amd", "csrc", "gs_kmeans.hip")).read()
    assert "sizeof(gs_kmeans_desc) == 128" in src and "sizeof(gs_kmeans_members_desc) == 72" in src
    # the K loop is the shared sweep, called and not restated
    assert '#include "gs_rank_dev.h"' in src and "__builtin_amdgcn_mfma" not in src
    for fn in ("rank_first_loads(", "rank_k_loop("):
        assert fn in src
    for own in ("rank_load_tiles(", "rank_store_tiles(", "rank_compute(", "k0"):      # the pipeline's pieces: gs_rank_dev.h alone
        assert own not in src

    out = ctypes.c_int64(0)
    for n in (0, 1, 128, 129, 232965):
        assert lib.gs_kmeans_assign_ws_bytes(n, ctypes.byref(out)) == 0 and out.value == 16 * (-(-n // 128))
    assert lib.gs_kmeans_assign_ws_bytes(1 << 31, ctypes.byref(out)) == -1
    for n, k, chunk, want in ((1, 1, 0, 4), (2048, 3, 0, 12), (2049, 3, 0, 24), (5000, 4096, 64, 79 * 4096 * 4), (100, 7, 128, 28)):
        assert lib.gs_kmeans_members_ws_bytes(n, k, chunk, ctypes.byref(out)) == 0 and out.value == want
    for n, k, chunk in ((5, 0, 0), (5, 4097, 0), (5, 3, 100), (5, 3, -64)):
        assert lib.gs_kmeans_members_ws_bytes(n, k, chunk, ctypes.byref(out)) == -1 and b"gs_kmeans_members_ws_bytes" in lib.gs_last_error()

    # every bad descriptor is refused before anything is launched or read (the pointers below are host memory)
    assert lib.gs_kmeans_assign(None, None) == -1 and b"gs_kmeans_assign" in lib.gs_last_error()
    assert lib.gs_kmeans_members(None, None) == -1 and b"gs_kmeans_members" in lib.gs_last_error()
    buf = (ctypes.c_int64 * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def desc():
        q = _lib.KmeansDesc()
        q.X = q.C = q.csq = q.assign = q.stats = q.ws = p
        q.n, q.n_rows, q.ld, q.ldc, q.ws_bytes, q.k, q.d = 5, 10, 8, 8, 1 << 20, 3, 8
        return q
    for field, value, word in (("n", 0, b"n=0"), ("k", 0, b"k=0"), ("k", 4097, b"k=4097"), ("d", 6, b"multiple of 4"),
                               ("d", 1028, b"multiple of 4"), ("ld", 4, b"ld must be >= d"), ("ldc", 6, b"ld %"),
                               ("n", 11, b"11 rows asked of a table of 10"), ("csq", None, b"non-null"),
                               ("stats", None, b"non-null"), ("ws_bytes", 8, b"workspace"), ("ws", p + 4, b"workspace"),
                               ("X", p + 4, b"16-byte aligned")):
        q = desc()
        setattr(q, field, value)
        assert lib.gs_kmeans_assign(ctypes.addressof(q), None) == -1 and word in lib.gs_last_error(), (field, lib.gs_last_error())

    def mdesc():
        q = _lib.KmeansMembersDesc()
        q.assign = q.rowptr = q.members = q.ws = p
        q.n, q.ws_bytes, q.k, q.chunk, q.reserved_ = 5, 1 << 20, 3, 0, 0
        return q
    for field, value, word in (("n", 0, b"n=0"), ("k", 0, b"k=0"), ("k", 4097, b"k=4097"), ("chunk", 65, b"chunk=65"),
                               ("reserved_", 1, b"reserved_"), ("members", None, b"non-null"), ("ws_bytes", 8, b"workspace")):
        q = mdesc()
        setattr(q, field, value)
        assert lib.gs_kmeans_members(ctypes.addressof(q), None) == -1 and word in lib.gs_last_error(), (field, lib.gs_last_error())
    assert lib.gs_kmeans_sqnorm(p, 8, 10, None, 5, 6, p, None) == -1 and b"multiple of 4" in lib.gs_last_error()
    assert lib.gs_kmeans_sqnorm(p, 8, 10, None, 11, 8, p, None) == -1 and b"11 rows asked" in lib.gs_last_error()
    assert lib.gs_kmeans_sqnorm(p, 8, 10, None, 0, 8, p, None) == 0      # nothing to do, nothing launched
