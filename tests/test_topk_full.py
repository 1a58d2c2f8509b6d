"""Host side of the full-graph top-k retrieval (no GPU): the C ABI of gs_topk_select / gs_topk_ws_bytes, the oracle's order
rule, the --topk_full flag of the unsupervised driver."""
import ctypes
import os
import re

import numpy as np
import pytest

from topk_oracle import candidates, select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ws_bytes_documented(Q, n_cand, k):
    """The rule of include/graphsage_amd.h, restated."""
    cdiv = lambda a, b: -(-a // b)
    tiles, q_tiles = cdiv(n_cand, 128), max(1, cdiv(Q, 128))
    tps = min(16384, max(4, cdiv(tiles, max(1, cdiv(2048, q_tiles)))))
    return max(1, cdiv(tiles, tps)) * Q * (8 * 64 * (1 + cdiv(k, 64)) + 4)


def test_descriptor_size_and_symbols():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    source = open(os.path.join(ROOT, "graphsage_amd", "csrc", "gs_topk.hip")).read()
    asserted = re.search(r"static_assert\(sizeof\(gs_topk_desc\) == (\d+)", source)
    assert asserted and ctypes.sizeof(_lib.TopkDesc) == int(asserted.group(1)) == 144
    assert re.search(r"typedef struct gs_topk_desc \{", header)
    assert re.search(r"#define GS_TOPK_MAX %d\b" % _lib.TOPK_MAX, header) and _lib.TOPK_MAX == 128
    lib = _lib.load()
    for name in ("gs_topk_select", "gs_topk_ws_bytes"):
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)


def test_error_reporting_and_workspace_rule():
    from graphsage_amd import _lib
    lib = _lib.load()
    assert lib.gs_topk_select(None, None) == -1 and b"gs_topk_select" in lib.gs_last_error()
    q = _lib.TopkDesc()                      # every pointer null
    q.Q, q.ldq, q.n_rows, q.n_cand, q.ldz, q.d, q.k = 5, 8, 10, 10, 8, 8, 3
    assert lib.gs_topk_select(ctypes.addressof(q), None) == -1 and b"gs_topk_select" in lib.gs_last_error()
    # from here on the pointers are non-null and aligned; every call is refused before anything is launched or read
    buf = (ctypes.c_int64 * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    q.Xq = q.Zc = q.ids = q.scores = q.count = p
    for bad_k in (0, 129, -1):
        q.k = bad_k
        assert lib.gs_topk_select(ctypes.addressof(q), None) == -1 and b"k=" in lib.gs_last_error()
    q.k = 3
    for bad_d in (0, 6, 1028):
        q.d = bad_d
        assert lib.gs_topk_select(ctypes.addressof(q), None) == -1 and b"multiple of 4" in lib.gs_last_error()
    q.d, q.n_cand = 8, 11
    assert lib.gs_topk_select(ctypes.addressof(q), None) == -1 and b"n_cand" in lib.gs_last_error()
    q.n_cand, q.f_rowptr, q.f_col = 10, p, p   # a filter without src
    assert lib.gs_topk_select(ctypes.addressof(q), None) == -1 and b"src" in lib.gs_last_error()
    q.f_rowptr = q.f_col = None
    q.flags = 6                                # unknown flag bits
    assert lib.gs_topk_select(ctypes.addressof(q), None) == -1 and b"flags" in lib.gs_last_error()
    q.flags = _lib.RANK_KEEP_SRC               # no workspace
    assert lib.gs_topk_select(ctypes.addressof(q), None) == -1 and b"workspace" in lib.gs_last_error()
    q.Q = 0                                    # no queries: returns at once
    assert lib.gs_topk_select(ctypes.addressof(q), None) == 0

    out = ctypes.c_int64(-1)
    assert lib.gs_topk_ws_bytes(5, 10, 3, None) == -1 and b"gs_topk_ws_bytes" in lib.gs_last_error()
    assert lib.gs_topk_ws_bytes(5, 10, 0, ctypes.byref(out)) == -1 and lib.gs_topk_ws_bytes(5, 10, 129, ctypes.byref(out)) == -1
    for Q, n_cand, k in ((1, 1, 1), (5, 10, 64), (129, 1031, 65), (300, 128 * 40 + 1, 128), (65536, 232965, 10), (1, 128 * 5000, 100)):
        assert lib.gs_topk_ws_bytes(Q, n_cand, k, ctypes.byref(out)) == 0
        assert out.value == ws_bytes_documented(Q, n_cand, k), (Q, n_cand, k)
    assert ws_bytes_documented(65536, 232965, 10) == 4 * 65536 * (128 * 8 + 4)      # four slices at the Reddit shape


def test_order_rule_of_the_oracle():
    """3 queries x 6 candidates with ties: score descending, then id ascending; exclusions; padding."""
    S = np.asarray([[1., 3., 3., 0., 3., -2.],
                    [5., 5., 5., 5., 5., 5.],
                    [0., -1., 0., 2., -1., 2.]])
    ids, scores, count = select(S, np.ones((3, 6), bool), 4)
    assert ids.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3], [3, 5, 0, 2]] and ids.dtype == np.int32
    assert scores.tolist() == [[3., 3., 3., 1.], [5., 5., 5., 5.], [2., 2., 0., 0.]] and count.tolist() == [4, 4, 4]
    flists = [[1, 4], [], [0, 1, 2, 3, 4, 5, 7]]
    C = candidates(3, 6, src=np.asarray([2, 0, 2]), flists=flists)
    assert C.astype(int).tolist() == [[0, 0, 0, 0, 0, 0], [0, 0, 1, 1, 0, 1], [0, 0, 0, 0, 0, 0]]
    ids, scores, count = select(S, C, 4)
    assert ids.tolist() == [[-1] * 4, [2, 3, 5, -1], [-1] * 4] and count.tolist() == [0, 3, 0]
    assert scores[1].tolist() == [5., 5., 5., -np.inf] and np.isneginf(scores[0]).all()
    kept = candidates(3, 6, src=np.asarray([2, 0, 5]), flists=[[], [], [], [], [], [0]], keep_src=True)
    assert kept.astype(int).tolist() == [[1] * 6, [1] * 6, [0, 1, 1, 1, 1, 1]]
    assert select(S, kept, 2)[0].tolist() == [[1, 2], [0, 1], [3, 5]]


def test_flag_parses():
    from graphsage_amd import unsupervised_train as ut
    assert ut.build_flags([]).topk_full == 0
    assert ut.build_flags(["--topk_full", "10"]).topk_full == 10


@pytest.mark.parametrize("model", ["graphsage_seq", "n2v"])
def test_models_without_embed_full_are_refused_before_training(model, capsys):
    from graphsage_amd import unsupervised_train as ut
    with pytest.raises(SystemExit) as ei:
        ut.main(["--synthetic", "small", "--model", model, "--topk_full", "5"])
    assert "--topk_full" in str(ei.value) and model in str(ei.value)
    assert "Loading training data" not in capsys.readouterr().out


def test_report_line():
    from graphsage_amd import unsupervised_train as ut
    ids = np.asarray([[3, 1, -1], [-1, -1, -1]], np.int32)
    assert ut.topk_full_line({"ids": ids}) == "Full-graph top-K partners: k= 3 nodes= 2 filled= 0.33333"
