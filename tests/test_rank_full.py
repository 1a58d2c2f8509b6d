"""Host side of the full-graph link ranking (no GPU): the C ABI of gs_rank_count / gs_rank_ws_bytes, RankFilter, the metrics
from hand-made counts, the --rank_full flag of the unsupervised driver."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ws_bytes_documented(Q, n_cand):
    """The rule of include/graphsage_amd.h, restated."""
    cdiv = lambda a, b: -(-a // b)
    tiles, q_tiles = cdiv(n_cand, 128), max(1, cdiv(Q, 128))
    tps = min(16384, max(4, cdiv(tiles, max(1, cdiv(2048, q_tiles)))))
    return max(1, cdiv(tiles, tps)) * Q * 2 * 4


# ------------------------------------------------------------------------------------------------ binding
def test_header_binding_and_error_reporting():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    for name in ("gs_rank_count", "gs_rank_ws_bytes"):
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"typedef struct gs_rank_desc \{", header)
    assert _lib.GS_ABI_VERSION == 12 and re.search(r"#define GS_ABI_VERSION 12\b", header)
    lib = _lib.load()
    assert lib.gs_abi_version() == 12
    for name in ("gs_rank_count", "gs_rank_ws_bytes"):
        assert hasattr(lib, name)
    # the descriptor goes by pointer: it is not one of the structs gs_abi_struct_sizes reports
    sizes = (ctypes.c_int32 * 16)()
    assert lib.gs_abi_struct_sizes(sizes, 16) == 8
    assert ctypes.sizeof(_lib.RankDesc) == 144

    assert lib.gs_rank_count(None, None) == -1 and b"gs_rank_count" in lib.gs_last_error()
    q = _lib.RankDesc()                      # every pointer null
    q.Q, q.ldq, q.n_rows, q.n_cand, q.ldz, q.d = 5, 8, 10, 10, 8, 8
    assert lib.gs_rank_count(ctypes.addressof(q), None) == -1 and b"gs_rank_count" in lib.gs_last_error()
    # from here on the pointers are non-null and aligned; every call is refused before anything is launched or read
    buf = (ctypes.c_int64 * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    q.Xq = q.Zc = q.dst = q.t = q.n_gt = q.n_eq = p
    for bad_d in (0, 2, 6, 1028, -4):
        q.d = bad_d
        assert lib.gs_rank_count(ctypes.addressof(q), None) == -1
        assert b"gs_rank_count" in lib.gs_last_error() and b"multiple of 4" in lib.gs_last_error()
    q.d, q.n_cand = 8, 11
    assert lib.gs_rank_count(ctypes.addressof(q), None) == -1
    assert b"gs_rank_count" in lib.gs_last_error() and b"n_cand" in lib.gs_last_error()
    q.n_cand, q.f_rowptr = 10, p               # half a filter; then a filter without src
    assert lib.gs_rank_count(ctypes.addressof(q), None) == -1 and b"gs_rank_count" in lib.gs_last_error()
    q.f_col = p
    assert lib.gs_rank_count(ctypes.addressof(q), None) == -1 and b"src" in lib.gs_last_error()
    q.f_rowptr = q.f_col = None
    q.flags = 6                                # unknown flag bits
    assert lib.gs_rank_count(ctypes.addressof(q), None) == -1 and b"flags" in lib.gs_last_error()
    q.flags = _lib.RANK_KEEP_SRC               # no workspace
    assert re.search(r"#define GS_RANK_KEEP_SRC %d\b" % _lib.RANK_KEEP_SRC, header)
    assert lib.gs_rank_count(ctypes.addressof(q), None) == -1 and b"workspace" in lib.gs_last_error()

    assert lib.gs_rank_ws_bytes(5, 10, None) == -1 and b"gs_rank_ws_bytes" in lib.gs_last_error()
    out = ctypes.c_int64(-1)
    assert lib.gs_rank_ws_bytes(-1, 10, ctypes.byref(out)) == -1 and b"gs_rank_ws_bytes" in lib.gs_last_error()
    for Q, n_cand in ((1, 1), (5, 10), (129, 1031), (300, 128 * 40 + 1), (65536, 232965), (38400, 232965), (1, 128 * 5000)):
        assert lib.gs_rank_ws_bytes(Q, n_cand, ctypes.byref(out)) == 0
        assert out.value == ws_bytes_documented(Q, n_cand), (Q, n_cand)
    assert ws_bytes_documented(65536, 232965) == 4 * 65536 * 8          # four slices at the Reddit shape: a 2 MB slab
    assert ws_bytes_documented(1, 1031) == 3 * 8                        # 9 tiles in slices of 4, 4, 1


# ------------------------------------------------------------------------------------------------ RankFilter
def test_rank_filter_sorts_dedups_and_keeps_empty_rows():
    from graphsage_amd.inference import RankFilter
    rowptr = np.asarray([0, 4, 4, 7, 7, 8], np.int64)
    col = np.asarray([3, 1, 3, 0, 4, 2, 4, 0], np.int64)
    f = RankFilter.from_csr(rowptr, col, 5)
    assert f.rowptr.dtype == np.int64 and f.col.dtype == np.int32 and f.n_nodes == 5
    assert [r.tolist() for r in f.lists()] == [[0, 1, 3], [], [2, 4], [], [0]]
    assert f.rowptr.tolist() == [0, 3, 3, 5, 5, 6]
    for r in f.lists():
        assert (np.diff(r) > 0).all()
    g = RankFilter.from_csr(np.zeros(4, np.int64), np.zeros(0, np.int64), 3)       # nothing but empty rows
    assert g.rowptr.tolist() == [0, 0, 0, 0] and g.col.size == 0


def test_rank_filter_takes_ascending_rows_as_they_are():
    from graphsage_amd.inference import RankFilter
    col = np.asarray([5, 9, 2, 3, 0], np.int32)                # every row ascending; the steps between rows go down
    g = RankFilter.from_csr(np.asarray([0, 2, 2, 4, 5] + [5] * 6, np.int64), col, 10)
    assert g.rowptr.tolist() == [0, 2, 2, 4, 5] + [5] * 6 and g.col.tolist() == col.tolist() and g.col.dtype == np.int32
    h = RankFilter.from_csr(np.asarray([0, 2, 2, 4, 5] + [5] * 6, np.int64), np.asarray([5, 9, 3, 3, 0]), 10)    # a duplicate
    assert [r.tolist() for r in h.lists()][:4] == [[5, 9], [], [3], [0]]


def test_rank_filter_refuses_ids_outside_the_table():
    from graphsage_amd._lib import GraphsageAmdError
    from graphsage_amd.inference import RankFilter
    rowptr = np.asarray([0, 2, 3], np.int64)
    with pytest.raises(GraphsageAmdError, match="ids must lie"):
        RankFilter.from_csr(rowptr, np.asarray([0, 2, 1]), 2)
    with pytest.raises(GraphsageAmdError, match="ids must lie"):
        RankFilter.from_csr(rowptr, np.asarray([0, -1, 1]), 2)
    with pytest.raises(GraphsageAmdError, match="rowptr"):
        RankFilter.from_csr(rowptr, np.asarray([0, 1]), 2)
    with pytest.raises(GraphsageAmdError, match="rowptr"):
        RankFilter.from_csr(rowptr[:2], np.asarray([0, 1]), 2)


def test_rank_filter_from_full_graph_covers_the_pad_row():
    from graphsage_amd.inference import FullGraph, RankFilter
    g = FullGraph.from_csr(np.asarray([0, 3, 3, 5], np.int64), np.asarray([2, 1, 2, 1, 0]), 3)
    f = RankFilter.from_full_graph(g)
    assert f.n_nodes == 4
    assert [r.tolist() for r in f.lists()] == [[1, 2], [3], [0, 1], [3]]
    assert g.rank_filter() is g.rank_filter() and g.rank_filter().col.tolist() == f.col.tolist()


# ------------------------------------------------------------------------------------------------ metrics
def test_metrics_from_hand_made_counts():
    from graphsage_amd.inference import rank_metrics
    n_gt = np.asarray([0, 0, 3, 9, 48, 120], np.int32)
    n_eq = np.asarray([0, 2, 0, 1, 2, 0], np.int32)
    res = rank_metrics(n_gt, n_eq)
    assert res["ranks"].tolist() == [1, 3, 4, 11, 51, 121]
    assert res["ranks_optimistic"].tolist() == [1, 1, 4, 10, 49, 121]
    assert res["n_gt"].tolist() == n_gt.tolist() and res["n_eq"].tolist() == n_eq.tolist()
    assert res["mrr"] == pytest.approx((1 + 1 / 3 + 1 / 4 + 1 / 11 + 1 / 51 + 1 / 121) / 6, rel=1e-12)
    assert res["hits"] == {1: 1 / 6, 10: 3 / 6, 50: 4 / 6, 100: 5 / 6}
    assert rank_metrics(n_gt, n_eq, hits=(3, 4))["hits"] == {3: 2 / 6, 4: 3 / 6}


# ------------------------------------------------------------------------------------------------ flag
def test_flag_parses():
    from graphsage_amd import unsupervised_train as ut
    assert ut.build_flags([]).rank_full is False
    assert ut.build_flags(["--rank_full"]).rank_full is True
    assert ut.build_flags(["--rank_full", "true"]).rank_full is True
    assert ut.build_flags(["--rank_full", "false"]).rank_full is False


@pytest.mark.parametrize("model", ["graphsage_seq", "n2v"])
def test_models_without_embed_full_are_refused_before_training(model, capsys):
    from graphsage_amd import unsupervised_train as ut
    with pytest.raises(SystemExit) as ei:
        ut.main(["--synthetic", "small", "--model", model, "--rank_full"])
    assert "--rank_full" in str(ei.value) and model in str(ei.value)
    assert "Loading training data" not in capsys.readouterr().out


def test_report_line():
    from graphsage_amd import unsupervised_train as ut
    from graphsage_amd.inference import rank_metrics
    line = ut.rank_full_line(rank_metrics(np.asarray([0, 11]), np.asarray([0, 0])))
    assert line == ("Full-graph link ranking: mrr= 0.54167 hits@1= 0.50000 hits@10= 0.50000 hits@50= 1.00000 "
                    "hits@100= 1.00000 edges= 2")
