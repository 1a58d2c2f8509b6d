"""Correct and Smooth / label propagation without a GPU: the fp64 oracle against closed forms, the C ABI, the drivers' refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import propagate_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def symmetric_lists(n, extra, seed):
    """A connected symmetric simple graph on n nodes (a ring plus `extra` random chords) as rows over n + 1 rows, pad = n."""
    rng = np.random.RandomState(seed)
    adj = [set() for _ in range(n)]
    for u in range(n):
        adj[u].add((u + 1) % n)
        adj[(u + 1) % n].add(u)
    for _ in range(extra):
        u, v = rng.randint(0, n, 2)
        if u != v:
            adj[u].add(int(v))
            adj[v].add(int(u))
    return [np.array(sorted(a), dtype=np.int64) for a in adj] + [np.array([n], dtype=np.int64)]


# ------------------------------------------------------------------------------------------------ the law
def test_run_reaches_the_closed_form():
    n = 30
    lists = symmetric_lists(n, 40, 0)
    _, w = po.weights(lists, n)
    S = po.dense_operator(lists, n, w)
    assert np.array_equal(S, S.T)                                    # symmetric on a symmetric graph
    X0 = np.random.RandomState(1).randn(n, 5)
    want = np.linalg.solve(np.eye(n) - 0.5 * S, 0.5 * X0)
    got = po.run(lists, n, X0, 0.5, 60)
    assert np.abs(got - want).max() <= 1e-10
    # one step of the row form equals one step of the dense form
    Xp = np.vstack([X0, np.zeros((1, 5))])
    one = po.step(lists, n, w, Xp, R=0.5 * Xp, alpha=0.5)
    assert np.abs(one[:n] - (0.5 * S @ X0 + 0.5 * X0)).max() <= 1e-14 and not one[n].any()


def test_duplicates_pads_and_empty_rows():
    pad = 4
    lists = [np.array([1, 1, 2]), np.array([pad, 0, pad]), np.array([pad, pad]), np.array([], dtype=np.int64), np.array([pad])]
    deg, w = po.weights(lists, pad)
    assert deg.tolist() == [3, 1, 0, 0, 0]                           # a duplicate counts twice, a pad entry not at all
    assert w.dtype == np.float32 and w[0] == np.float32(1 / np.sqrt(3.0)) and w[1] == 1.0 and not w[2:].any()
    X = np.array([[1.0, 2.0], [3.0, 5.0], [7.0, 11.0], [13.0, 17.0], [1e30, -1e30]])     # the pad row's values must not leak
    R = np.array([[0.5, -0.5], [0.25, 4.0], [2.0, -3.0], [0.125, 9.0], [1.0, 1.0]])
    out = po.step(lists, pad, w, X, R=R, alpha=1.0, lo=-1.0, hi=2.5)
    w0 = np.float64(w[0])
    s0 = w0 * (2 * 1.0 * X[1] + 0.0 * X[2])                          # row 2 has deg 0: its weight is 0
    assert np.allclose(out[0], np.clip(s0 + R[0], -1.0, 2.5), rtol=0, atol=1e-15)
    assert np.array_equal(out[1], np.clip(1.0 * w0 * X[0] + R[1], -1.0, 2.5))
    assert np.array_equal(out[2], np.clip(R[2], -1.0, 2.5))          # a row of pads only: clamp(R[r])
    assert np.array_equal(out[3], np.clip(R[3], -1.0, 2.5))
    assert not out[pad].any()
    assert np.array_equal(po.step(lists, pad, w, X, alpha=1.0)[2], [0.0, 0.0])      # R NULL


def test_scale_rule_edges():
    E = np.array([[0.0, 0.0], [1e-4, -1e-4], [0.5, -0.5], [2e-3, 0.0]])
    scale, raw = po.scale_rule(1.0, E)
    assert np.isinf(raw[0]) and scale[0] == 1.0                      # l1 = 0
    assert raw[1] == pytest.approx(5000.0) and scale[1] == 1.0       # beyond the cap
    assert scale[2] == raw[2] == 1.0 and scale[3] == raw[3] == pytest.approx(500.0)
    P = np.ones_like(E)
    Y = np.full_like(E, 9.0)
    G0, _ = po.correct(P, E, Y, np.array([False, False, False, True]), 1.0)
    assert np.array_equal(G0[0], [1.0, 1.0]) and np.allclose(G0[1], [1.0001, 0.9999]) and np.array_equal(G0[3], [9.0, 9.0])


def test_label_propagation_isolated_known_node():
    n = 6
    lists = symmetric_lists(5, 2, 3)[:5] + [np.array([n])] + [np.array([n])]      # node 5 has no neighbor: the single entry pad
    labels = np.zeros((n, 3))
    labels[5, 1] = 1.0
    labels[0, 0] = 1.0
    got = po.label_propagation(lists, n, labels, np.array([0, 5]), alpha=0.8, iters=7)
    # X^t[5] = (1 - alpha) * label from the first step on (S has no entry in row 5; the geometric sum has one term)
    assert np.allclose(got[5], [0.0, 1.0 - 0.8, 0.0], rtol=0, atol=1e-15)
    # a node with a self loop keeps feeding itself: sum_k alpha^k (1 - alpha) -> 1
    loop = [np.array([0]), np.array([1])]
    got = po.label_propagation(loop, 1, np.array([[1.0]]), np.array([0]), alpha=0.8, iters=9)
    assert got[0, 0] == pytest.approx(0.8 ** 9 + (1 - 0.8) * sum(0.8 ** k for k in range(9)))


def test_correct_and_smooth_oracle_shapes_and_fp32_run():
    n = 40
    lists = symmetric_lists(n, 60, 5)
    rng = np.random.RandomState(6)
    labels = np.eye(4)[rng.randint(0, 4, n)]
    logits = rng.randn(n, 4) + 2.0 * labels
    preds = np.exp(logits) / np.exp(logits).sum(axis=1, keepdims=True)
    known = np.arange(0, n, 2)
    a = po.correct_and_smooth(lists, n, preds, labels, known, iters=20)
    b = po.correct_and_smooth(lists, n, preds, labels, known, iters=20, dtype=np.float32)
    assert a["preds"].shape == (n, 4) and a["preds"].min() >= 0.0 and a["preds"].max() <= 1.0
    assert np.array_equal(a["corrected"][known], labels[known])
    assert np.abs(a["preds"] - b["preds"]).max() <= 2.5e-5


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_binding_and_library_agree():
    from graphsage_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    for name in ("gs_prop_weights", "gs_prop_ws_bytes", "gs_prop_step", "gs_prop_correct"):
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"typedef struct gs_prop_desc \{", header)
    version = int(re.search(r"#define GS_ABI_VERSION (\d+)\b", header).group(1))
    lib = _lib.load()                                                     # binds every name of _PROTOS: the library exports them
    assert lib.gs_abi_version() == version == _lib.GS_ABI_VERSION == 12   # entry points were added, no layout changed
    sizes = (ctypes.c_int32 * 16)()
    assert lib.gs_abi_struct_sizes(sizes, 16) == 8                        # the descriptor goes by pointer
    assert ctypes.sizeof(_lib.PropDesc) == 176
    assert int(re.search(r"#define GS_PROP_MAX_D (\d+)\b", header).group(1)) == _lib.PROP_MAX_D == ops.PROP_MAX_D == 256
    src = open(os.path.join(ROOT, "graphsage_amd", "csrc", "gs_propagate.hip")).read()
    assert "sizeof(gs_prop_desc) == 176" in src and "atomic" not in src.lower().replace("no float atomics", "")

    out = ctypes.c_int64(0)
    for slots, d, want in ((0, 41, 0), (3, 1, 48), (3, 41, 3 * 44 * 4), (2, 256, 2048)):
        assert lib.gs_prop_ws_bytes(slots, d, ctypes.byref(out)) == 0 and out.value == want
    assert lib.gs_prop_ws_bytes(1, 0, ctypes.byref(out)) == -1 and b"gs_prop_ws_bytes" in lib.gs_last_error()

    # every bad call is refused before anything is launched or read (the pointers below are host memory)
    assert lib.gs_prop_step(None, None) == -1 and b"gs_prop_step" in lib.gs_last_error()
    buf = (ctypes.c_int64 * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def desc():
        q = _lib.PropDesc()
        q.rowptr = q.col = q.items = q.X = q.R = q.w = p
        q.out = p + 64
        q.n_rows, q.nnz, q.n_items, q.pad, q.ldx, q.ldr, q.ldo = 5, 9, 5, 4, 44, 44, 44
        q.alpha, q.lo, q.hi, q.d, q.split_len = 0.5, 0.0, 0.5, 41, 512
        return q
    for field, value, rc, word in (("d", 0, -3, b"1 <= d <= 256"), ("d", 257, -3, b"1 <= d <= 256"), ("out", p, -1, b"out must not be X"),
                                   ("ldx", 40, -1, b"round_up(d,4) = 44"), ("ldo", 40, -1, b"round_up(d,4)"),
                                   ("ldr", 40, -1, b"round_up(d,4)"), ("ldx", 46, -1, b"ld %"), ("X", p + 4, -1, b"16-byte aligned"),
                                   ("w", None, -1, b"non-null"), ("pad", 6, -1, b"pad=6"), ("n_items", 4, -1, b"4 items for 5 rows"),
                                   ("n_split", 1, -1, b"workspace"), ("lo", 1.0, -1, b"lo <= hi"), ("hi", -1.0, -1, b"lo <= hi"),
                                   ("alpha", float("nan"), -1, b"numbers")):
        q = desc()
        setattr(q, field, value)
        assert lib.gs_prop_step(ctypes.addressof(q), None) == rc and word in lib.gs_last_error(), (field, lib.gs_last_error())
    q = desc()
    q.n_items = q.n_rows = q.pad = 0
    assert lib.gs_prop_step(ctypes.addressof(q), None) == 0              # nothing to do, nothing launched

    assert lib.gs_prop_weights(p, p, 5, 6, p, p, None) == -1 and b"pad=6" in lib.gs_last_error()
    assert lib.gs_prop_weights(p, p, 5, 4, None, p, None) == -1 and b"non-null" in lib.gs_last_error()
    assert lib.gs_prop_weights(p, p, 0, 0, p, p, None) == 0
    for d, rc in ((0, -3), (257, -3)):
        assert lib.gs_prop_correct(p, 44, p, 44, None, 0, None, 5, d, 1.0, p, 44, None) == rc
    assert lib.gs_prop_correct(p, 40, p, 44, None, 0, None, 5, 41, 1.0, p, 44, None) == -1 and b"round_up(d,4)" in lib.gs_last_error()
    assert lib.gs_prop_correct(p, 44, p, 44, p, 44, None, 5, 41, 1.0, p, 44, None) == -1 and b"known" in lib.gs_last_error()
    assert lib.gs_prop_correct(p, 44, p, 44, None, 0, None, 0, 41, 1.0, p, 44, None) == 0


# ------------------------------------------------------------------------------------------------ drivers and module
def test_flags_and_driver_refusals(capsys):
    from graphsage_amd import supervised_train as st
    f = st.build_flags([])
    assert (f.correct_smooth, f.label_propagation, f.cs_correct_alpha, f.cs_smooth_alpha, f.cs_iters) == (False, False, 0.8, 0.8, 50)
    f = st.build_flags(["--correct_smooth", "--label_propagation", "--cs_correct_alpha", "0.5", "--cs_smooth_alpha", "1",
                        "--cs_iters", "7"])
    assert (f.correct_smooth, f.label_propagation, f.cs_correct_alpha, f.cs_smooth_alpha, f.cs_iters) == (True, True, 0.5, 1.0, 7)
    st.refuse_propagation(f)
    st.refuse_propagation(st.build_flags(["--cs_iters", "0"]))            # flags off: nothing refused
    capsys.readouterr()
    for argv, word in ((["--correct_smooth", "--model", "graphsage_seq"], "--correct_smooth is not available"),
                       (["--label_propagation", "--model", "graphsage_seq"], "--label_propagation is not available"),
                       (["--correct_smooth", "--cs_correct_alpha", "0"], "(0, 1]"),
                       (["--correct_smooth", "--cs_correct_alpha", "1.5"], "(0, 1]"),
                       (["--correct_smooth", "--cs_smooth_alpha", "-0.1"], "(0, 1]"),
                       (["--label_propagation", "--cs_smooth_alpha", "nan"], "(0, 1]"),
                       (["--label_propagation", "--cs_iters", "0"], "[1, 1000]"),
                       (["--correct_smooth", "--cs_iters", "1001"], "[1, 1000]")):
        with pytest.raises(SystemExit) as ei:
            st.main(["--synthetic", "small"] + argv)
        assert word in str(ei.value), str(ei.value)
        assert "Loading training data" not in capsys.readouterr().out
    # --label_propagation alone does not look at --cs_correct_alpha
    st.refuse_propagation(st.build_flags(["--label_propagation", "--cs_correct_alpha", "7"]))
    # more than 256 classes: refused once the data is loaded
    with pytest.raises(SystemExit, match="257 classes"):
        st.refuse_propagation_classes(st.build_flags(["--correct_smooth"]), 257)
    st.refuse_propagation_classes(st.build_flags(["--correct_smooth"]), 256)
    st.refuse_propagation_classes(st.build_flags([]), 1000)


def test_module_refusals_come_before_any_launch():
    """Bad arguments never reach the device: the engine below has none."""
    from graphsage_amd import propagation as pr
    from graphsage_amd._lib import GraphsageAmdError
    from graphsage_amd.inference import FullGraph

    lists = symmetric_lists(10, 5, 2)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in lists[:10]])])
    graph = FullGraph.from_csr(rowptr, np.concatenate(lists[:10]), 10)
    labels = np.eye(3)[np.arange(10) % 3]
    preds = np.full((10, 3), 1.0 / 3)
    known = np.array([0, 2, 4])
    bad = (dict(correct_alpha=0.0), dict(smooth_alpha=1.01), dict(iters=0), dict(iters=1001), dict(correct_alpha=float("nan")),
           dict(preds=preds[:9]), dict(labels=labels[:, :2]), dict(preds=np.zeros((10, 257)), labels=np.zeros((10, 257))),
           dict(known=np.array([0, 10])), dict(known=np.array([-1])), dict(known=np.array([], dtype=np.int64)))
    for change in bad:
        kw = dict(preds=preds, labels=labels, known=known)
        kw.update(change)
        with pytest.raises(GraphsageAmdError):
            pr.correct_and_smooth(None, graph, kw.pop("preds"), kw.pop("labels"), kw.pop("known"), **kw)
    for change in (dict(alpha=0.0), dict(alpha=2.0), dict(iters=0), dict(labels=labels[:9]), dict(labels=np.zeros((10, 300))),
                   dict(known=np.array([10])), dict(known=np.zeros(10, dtype=bool))):
        kw = dict(labels=labels, known=known)
        kw.update(change)
        with pytest.raises(GraphsageAmdError):
            pr.label_propagation(None, graph, kw.pop("labels"), kw.pop("known"), **kw)
    with pytest.raises(GraphsageAmdError, match="FullGraph"):
        pr.Propagator(None, object())
