"""Host side of the inverted-file retrieval (no GPU): the C ABI of gs_ivf_search / gs_ivf_ws_bytes, the oracle, recall, the
re-numbering of IVFIndex.from_labels, the --topk_ivf flags of the unsupervised driver."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import ivf_oracle
from topk_oracle import candidates, scores64, select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_descriptor_size_and_symbols():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    source = open(os.path.join(ROOT, "graphsage_amd", "csrc", "gs_ivf.hip")).read()
    asserted = re.search(r"static_assert\(sizeof\(gs_ivf_desc\) == (\d+)", source)
    assert asserted and ctypes.sizeof(_lib.IvfDesc) == int(asserted.group(1)) == 200
    assert re.search(r"typedef struct gs_ivf_desc \{", header) and "gs_ivf_desc is 200 bytes" in header
    assert re.search(r"#define GS_IVF_MAX_PROBE %d\b" % _lib.IVF_MAX_PROBE, header) and _lib.IVF_MAX_PROBE == 128
    assert re.search(r"#define GS_ABI_VERSION %d\b" % _lib.GS_ABI_VERSION, header)       # added entry points alone: unchanged
    # the fields of the header's struct, in order, are the mirror's
    body = re.search(r"typedef struct gs_ivf_desc \{(.*?)\} gs_ivf_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [f[0] for f in _lib.IvfDesc._fields_]
    lib = _lib.load()
    for name in ("gs_ivf_search", "gs_ivf_ws_bytes"):
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    # the shared header: both files include it, neither restates what it holds
    topk = open(os.path.join(ROOT, "graphsage_amd", "csrc", "gs_topk.hip")).read()
    shared = open(os.path.join(ROOT, "graphsage_amd", "csrc", "gs_topk_dev.h")).read()
    for text in (topk, source):
        assert '#include "gs_topk_dev.h"' in text
        assert not re.search(r"^__device__ .*\btopk_(key|score|compact|push)\(", text, re.M) and "void topk_merge_kernel" not in text
    for fn in ("topk_key", "topk_score", "topk_uniform", "topk_compact", "topk_push", "topk_merge_kernel", "topk_merge_launch"):
        assert re.search(r"\b%s\(" % fn, shared), fn


def test_error_reporting_and_workspace_rule():
    from graphsage_amd import _lib
    lib = _lib.load()
    assert lib.gs_ivf_search(None, None) == -1 and b"gs_ivf_search" in lib.gs_last_error()
    q = _lib.IvfDesc()                       # every pointer null: each call below is refused before anything is launched or read
    q.Q, q.ldq, q.n_rows, q.n_cand, q.ldz, q.ldc, q.n_list, q.d, q.k, q.nprobe, q.n_clusters = 5, 8, 10, 10, 8, 8, 10, 8, 3, 2, 4
    good = dict(k=3, nprobe=2, d=8, n_clusters=4)
    for field, bad, word in (("k", (0, 129, -1), b"k="), ("nprobe", (0, 129, 5, -1), b"nprobe="), ("d", (0, 6, 1028), b"multiple of 4"),
                             ("n_clusters", (0, 4097), b"n_clusters=")):
        for v in bad:
            setattr(q, field, v)
            assert lib.gs_ivf_search(ctypes.addressof(q), None) == -1 and word in lib.gs_last_error(), (field, v)
        setattr(q, field, good[field])
    q.n_cand = 11
    assert lib.gs_ivf_search(ctypes.addressof(q), None) == -1 and b"n_cand" in lib.gs_last_error()
    q.n_cand, q.flags = 10, 6
    assert lib.gs_ivf_search(ctypes.addressof(q), None) == -1 and b"flags" in lib.gs_last_error()
    q.flags, q.stop_after = 0, 6
    assert lib.gs_ivf_search(ctypes.addressof(q), None) == -1 and b"stop_after" in lib.gs_last_error()
    q.stop_after = 0
    assert lib.gs_ivf_search(ctypes.addressof(q), None) == -1 and b"Xq" in lib.gs_last_error()      # null matrices
    buf = (ctypes.c_int64 * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    q.Xq = q.Zc = q.centers = q.list_ptr = q.list_ids = q.ids = q.scores = q.count = p
    q.f_rowptr = q.f_col = p                                                                          # a filter without src
    assert lib.gs_ivf_search(ctypes.addressof(q), None) == -1 and b"src" in lib.gs_last_error()
    q.f_rowptr = q.f_col = None
    assert lib.gs_ivf_search(ctypes.addressof(q), None) == -1 and b"workspace" in lib.gs_last_error()
    q.Q = 0                                                                                           # no queries: returns at once
    assert lib.gs_ivf_search(ctypes.addressof(q), None) == 0

    out = ctypes.c_int64(-1)
    assert lib.gs_ivf_ws_bytes(5, 4, 3, 2, None) == -1 and b"gs_ivf_ws_bytes" in lib.gs_last_error()
    for bad in ((5, 4, 0, 2), (5, 4, 129, 2), (5, 4, 3, 0), (5, 4, 3, 5), (5, 0, 3, 1), (1 << 24, 4, 3, 2)):
        assert lib.gs_ivf_ws_bytes(*bad, ctypes.byref(out)) == -1, bad
    # the documented parts: the lists alone are Q * nprobe * (8 * cap + 4) bytes, and the whole is not much more
    for Q, C, k, P in ((1, 1, 1, 1), (129, 7, 65, 7), (65536, 1931, 10, 16)):
        assert lib.gs_ivf_ws_bytes(Q, C, k, P, ctypes.byref(out)) == 0
        lists = Q * P * (8 * 64 * (1 + -(-k // 64)) + 4)
        probe = ctypes.c_int64(0)
        assert lib.gs_topk_ws_bytes(Q, C, P, ctypes.byref(probe)) == 0
        small = 4 * Q * P * 4 + 4 * Q + 12 * (C + 1) + 4 * C * -(-Q * P // 2048)
        assert lists + probe.value + small <= out.value <= lists + probe.value + small + 16 * 12 and out.value % 16 == 0


def test_oracle_with_every_list_probed_is_the_exhaustive_oracle():
    rng = np.random.RandomState(0)
    Q, n_cand, n_rows, d, C, k = 9, 60, 64, 8, 5, 7
    Z, Xq = rng.randint(-3, 4, size=(n_rows, d)).astype(np.float32), rng.randint(-3, 4, size=(Q, d)).astype(np.float32)
    centers, labels = rng.randint(-3, 4, size=(C, d)).astype(np.float32), rng.randint(0, C, size=n_cand)
    labels[:C] = np.arange(C)
    src = rng.randint(0, n_rows, size=Q)
    flists = [np.sort(rng.choice(n_rows, size=rng.randint(0, 6), replace=False)) for _ in range(n_rows)]
    S, Cm = scores64(Xq, Z, n_cand), candidates(Q, n_cand, src, flists)
    full = ivf_oracle.search(S, Cm, Xq, centers, labels, k, C)
    want = select(S, Cm, k)
    assert all(np.array_equal(a, b) for a, b in zip(full[:3], want)) and (full[3] == n_cand).all()
    # fewer probes: a subset of the candidates, only rows of the probed lists, never a better score than the exhaustive one
    P = ivf_oracle.probe(Xq, centers, 2)
    assert P.shape == (Q, 2) and all(len(set(r)) == 2 for r in P.tolist())
    some = ivf_oracle.search(S, Cm, Xq, centers, labels, k, 2)
    for q in range(Q):
        got = some[0][q][some[0][q] >= 0]
        assert np.isin(labels[got], P[q]).all() and Cm[q, got].all()
        assert (some[1][q] <= want[1][q]).all() and some[2][q] <= want[2][q]
        assert some[3][q] == np.isin(labels, P[q]).sum()
    # the probe order: score descending, then centre id ascending
    tie = ivf_oracle.probe(np.ones((1, 4), np.float32), np.asarray([[1, 0, 0, 0], [2, 0, 0, 0], [0, 1, 0, 0], [0, 0, 2, 0]], np.float32), 4)
    assert tie.tolist() == [[1, 3, 0, 2]]


def test_recall_on_hand_made_cases():
    from graphsage_amd.retrieval import recall
    exact = np.asarray([[1, 2, 3, 4], [5, 6, -1, -1], [-1, -1, -1, -1], [7, 8, 9, 10]], np.int32)
    assert recall(exact, exact) == 1.0
    approx = np.asarray([[4, 3, 2, 1], [6, 9, 9, -1], [3, 3, 3, 3], [-1, -1, -1, -1]], np.int32)
    assert recall(approx, exact) == pytest.approx((4 / 4 + 1 / 2 + 0 / 4) / 3, abs=0, rel=1e-15)      # the empty exact row is left out
    assert recall(np.full((2, 3), -1), np.asarray([[0, 1, 2], [3, -1, -1]])) == 0.0                    # -1 never matches the padding
    assert math.isnan(recall(approx[2:3], exact[2:3]))
    assert recall(np.asarray([[1, 2]]), np.asarray([[2, 5, 6, 1]])) == 0.5                             # k of the two may differ
    with pytest.raises(ValueError):
        recall(approx[:2], exact)


def test_from_labels_renumbers_past_empty_clusters():
    from graphsage_amd._lib import GraphsageAmdError
    from graphsage_amd.retrieval import default_clusters, renumber
    centers = np.arange(6 * 4, dtype=np.float32).reshape(6, 4)
    labels = np.asarray([5, 1, 1, 3, 5, 5, 1], np.int64)                         # 0, 2 and 4 have no member
    c2, l2, empty = renumber(centers, labels)
    assert empty == 3 and c2.dtype == np.float32 and l2.dtype == np.int32
    assert np.array_equal(c2, centers[[1, 3, 5]]) and l2.tolist() == [2, 0, 0, 1, 2, 2, 0]
    c3, l3, empty3 = renumber(c2, l2)                                            # already compact: unchanged
    assert empty3 == 0 and np.array_equal(c3, c2) and np.array_equal(l3, l2)
    for bad in (np.asarray([0, 6]), np.asarray([-1, 0]), np.zeros(0, np.int64), np.asarray([0.5, 1.0])):
        with pytest.raises(GraphsageAmdError):
            renumber(centers, bad)
    with pytest.raises(GraphsageAmdError):
        renumber(np.zeros((4097, 4), np.float32), labels)
    assert default_clusters(232965) == round(4 * math.sqrt(232965)) == 1931 and default_clusters(10 ** 7) == 4096
    assert default_clusters(1) == 1 and default_clusters(9) == 9 and default_clusters(100) == 40


def test_flags_parse_and_the_line():
    from graphsage_amd import retrieval
    from graphsage_amd import unsupervised_train as ut
    f = ut.build_flags([])
    assert (f.topk_ivf, f.topk_ivf_clusters, f.topk_ivf_nprobe, f.topk_ivf_recall, f.topk_ivf_seed) == (0, 0, 8, 0, 123)
    f = ut.build_flags(["--topk_ivf", "10", "--topk_ivf_clusters", "64", "--topk_ivf_nprobe", "4", "--topk_ivf_recall", "100"])
    assert (f.topk_ivf, f.topk_ivf_clusters, f.topk_ivf_nprobe, f.topk_ivf_recall) == (10, 64, 4, 100)
    res = {"k": 10, "nodes": 500, "clusters": 63, "empty": 1, "nprobe": 4, "list_min": 2, "list_max": 40, "scanned_share": 0.0625,
           "filled": 1.0, "recall": float("nan"), "sample": 0, "build_time": 0.5, "search_time": 0.25}
    assert retrieval.result_line(res) == ("IVF top-K partners: k= 10 nodes= 500 clusters= 63 empty= 1 nprobe= 4 list_min= 2 "
                                          "list_max= 40 scanned= 0.06250 filled= 1.00000 recall@k= nan sample= 0 "
                                          "build_time= 0.50000 search_time= 0.25000")


@pytest.mark.parametrize("extra,word", [
    (["--model", "graphsage_seq", "--topk_ivf", "5"], "graphsage_seq"),
    (["--model", "n2v", "--topk_ivf", "5"], "n2v"),
    (["--topk_ivf", "5", "--importance_neighbors", "8"], "--importance_neighbors"),
    (["--topk_ivf", "129"], "[1, 128]"),
    (["--topk_ivf", "-1"], "[1, 128]"),
    (["--topk_ivf", "5", "--topk_ivf_nprobe", "0"], "--topk_ivf_nprobe"),
    (["--topk_ivf", "5", "--topk_ivf_nprobe", "129"], "--topk_ivf_nprobe"),
    (["--topk_ivf", "5", "--topk_ivf_clusters", "4097"], "--topk_ivf_clusters"),
    (["--topk_ivf", "5", "--topk_ivf_clusters", "-2"], "--topk_ivf_clusters"),
    (["--topk_ivf", "5", "--topk_ivf_recall", "-1"], "--topk_ivf_recall"),
])
def test_flag_refusals_fire_before_training(extra, word, capsys):
    from graphsage_amd import unsupervised_train as ut
    with pytest.raises(SystemExit) as ei:
        ut.main(["--synthetic", "small"] + extra)
    assert "topk_ivf" in str(ei.value) and word in str(ei.value)
    assert "Loading training data" not in capsys.readouterr().out
