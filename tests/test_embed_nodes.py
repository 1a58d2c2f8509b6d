"""CPU suite of receptive-field inference (embed_nodes): the C ABI surface of gs_frontier_expand / gs_csr_reduce_rows and their
host-side refusals (every one happens before a launch: this suite runs without a device), FullGraph.plan_rows against a
brute-force plan on the edge graph of tests/test_csr_reduce_gpu.py's design, the subset oracle's closure against a set-based
restatement, and the --embed_nodes refusals of both drivers."""
import ctypes
import os
import re

import numpy as np
import pytest

import subset_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
L = 512


# ------------------------------------------------------------------------------------------------ binding
def test_abi_version_struct_count_and_descriptor_sizes():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    assert _lib.GS_ABI_VERSION == 12 and re.search(r"#define GS_ABI_VERSION 12\b", header)
    lib = _lib.load()
    assert lib.gs_abi_version() == 12
    sizes = (ctypes.c_int32 * 16)()
    assert lib.gs_abi_struct_sizes(sizes, 16) == 8            # the new descriptors go by pointer: not part of this list
    for src, struct, mirror, size in (("gs_frontier.hip", "gs_frontier_desc", _lib.FrontierDesc, 96),
                                      ("gs_csr_reduce.hip", "gs_csr_rows_desc", _lib.CsrRowsDesc, 168),
                                      ("gs_csr_reduce.hip", "gs_csr_reduce_desc", _lib.CsrReduceDesc, 200)):
        text = open(os.path.join(ROOT, "graphsage_amd", "csrc", src)).read()
        m = re.search(r"static_assert\(sizeof\(%s\) == (\d+)" % struct, text)
        assert m and int(m.group(1)) == size == ctypes.sizeof(mirror), struct
        assert re.search(r"typedef struct %s \{" % struct, header)


def test_symbols_are_declared_bound_and_exported():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    lib = _lib.load()
    for name in ("gs_frontier_expand", "gs_frontier_ws_bytes", "gs_csr_reduce_rows"):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert _lib._PROTOS["gs_frontier_expand"] == _lib._PROTOS["gs_csr_reduce_rows"] == _lib._PROTOS["gs_csr_reduce_fwd"]
    out = ctypes.c_int64(-1)
    assert lib.gs_frontier_ws_bytes(1000, ctypes.byref(out)) == 0 and out.value == (1000 + 256) * 4
    assert lib.gs_frontier_ws_bytes(1000, None) == -1 and b"gs_frontier_ws_bytes" in lib.gs_last_error()


FAKE = 0x10000          # a non-null, 16-byte aligned address that is never dereferenced: every refusal precedes the launch


def frontier_desc():
    from graphsage_amd import _lib
    q = _lib.FrontierDesc()
    q.rowptr = q.col = q.rows_in = q.rows_out = q.pos = q.count = q.ws = FAKE
    q.n_rows, q.nnz, q.m, q.rows_out_cap, q.ws_bytes = 100, 400, 10, 100, (100 + 256) * 4
    return q


def test_frontier_expand_refuses_bad_calls_before_any_launch():
    from graphsage_amd import _lib
    lib = _lib.load()

    def refused(q, word):
        assert lib.gs_frontier_expand(ctypes.addressof(q) if q is not None else None, None) == -1
        msg = lib.gs_last_error()
        assert b"gs_frontier_expand" in msg and word in msg, msg

    refused(None, b"null descriptor")
    for field in ("rowptr", "col", "rows_in", "rows_out", "pos", "count"):
        q = frontier_desc()
        setattr(q, field, None)
        refused(q, b"non-null")
    for field, value in (("m", -1), ("m", 101), ("n_rows", 0), ("n_rows", 1 << 31), ("nnz", -1), ("rows_out_cap", -1)):
        q = frontier_desc()
        setattr(q, field, value)
        refused(q, b"bad sizes")
    q = frontier_desc()
    q.ws = None
    refused(q, b"workspace")
    q = frontier_desc()
    q.ws = FAKE + 4
    refused(q, b"16-byte aligned")
    q = frontier_desc()
    q.ws_bytes -= 4
    refused(q, b"too small")


def rows_desc():
    from graphsage_amd import _lib
    q = _lib.CsrRowsDesc()
    q.rowptr = q.col = q.items = q.splits = q.x_pos = q.out_pos = q.X = q.out = q.ws = FAKE
    q.n_rows, q.nnz, q.n_items, q.n_split, q.n_slots = 100, 400, 12, 1, 3
    q.ldx, q.x_rows, q.ldo, q.out_rows, q.ws_bytes = 52, 60, 52, 10, 3 * 256 * 4
    q.d, q.op, q.act, q.split_len = 50, _lib.CSR_MEAN, _lib.ACT_IDENTITY, L
    return q


def test_csr_reduce_rows_refuses_bad_calls_before_any_launch():
    from graphsage_amd import _lib
    lib = _lib.load()

    def refused(q, word):
        assert lib.gs_csr_reduce_rows(ctypes.addressof(q) if q is not None else None, None) == -1
        msg = lib.gs_last_error()
        assert b"gs_csr_reduce_rows" in msg and word in msg, msg

    refused(None, b"null descriptor")
    for field in ("rowptr", "col", "items", "out_pos"):
        q = rows_desc()
        setattr(q, field, None)
        refused(q, b"non-null")
    for field in ("X", "out"):
        q = rows_desc()
        setattr(q, field, None)
        refused(q, b"matrix must be non-null")
    for field, value in (("n_items", -1), ("n_rows", -1), ("nnz", -1), ("d", 0), ("split_len", 0), ("n_slots", -1),
                         ("n_split", -1), ("x_rows", -1), ("out_rows", -1)):
        q = rows_desc()
        setattr(q, field, value)
        refused(q, b"bad sizes")
    q = rows_desc()
    q.op = 7
    refused(q, b"unknown op")
    q = rows_desc()
    q.act = 5
    refused(q, b"unknown act")
    q = rows_desc()
    q.ldo = 48
    refused(q, b"ld must be")
    q = rows_desc()
    q.x_pos = None                 # no map: the table is indexed by node id and must hold every row of the graph
    refused(q, b"no x_pos")
    for field in ("splits", "ws"):
        q = rows_desc()
        setattr(q, field, None)
        refused(q, b"long rows need")
    q = rows_desc()
    q.ws = FAKE + 8
    refused(q, b"16-byte aligned")
    q = rows_desc()
    q.ws_bytes -= 4
    refused(q, b"too small")
    q = rows_desc()
    q.n_items = 0                  # nothing to do is no error, and launches nothing
    assert lib.gs_csr_reduce_rows(ctypes.addressof(q), None) == 0


# ------------------------------------------------------------------------------------------------ plan_rows
DEGS = [0, 1, 2, 63, 64, 65, L - 1, L, L + 1, 3 * L + 7, 0, 5, 2 * L + 1, 3]       # the last row is the pad row
CUT = [8, 9, 12]


def edge_graph():
    from graphsage_amd.inference import FullGraph
    rng = np.random.RandomState(3)
    n = len(DEGS) - 1
    rowptr = np.concatenate([[0], np.cumsum(DEGS)]).astype(np.int64)
    col = rng.randint(0, n + 1, size=int(rowptr[-1])).astype(np.int32)
    col[rowptr[n]:] = n                                                               # the pad row lists itself
    return FullGraph(rowptr, col, n)


def brute_force_plan(rowptr, rows, split_len):
    items, splits, slot = [], [], 0
    for r in rows:
        e0, deg = int(rowptr[r]), int(rowptr[r + 1] - rowptr[r])
        if deg <= split_len:
            items.append((r, e0, deg, -1))
            continue
        parts = -(-deg // split_len)
        splits.append((r, slot, parts))
        for k in range(parts):
            items.append((r, e0 + k * split_len, min(split_len, deg - k * split_len), slot))
            slot += 1
    return np.asarray(items, np.int64).reshape(-1, 4), np.asarray(splits, np.int64).reshape(-1, 3)


SUBSETS = {"every row": list(range(len(DEGS))), "one uncut row": [5], "one cut row": [9], "only cut rows": CUT,
           "the empty rows": [0, 10], "the pad row": [len(DEGS) - 1], "mixed": [0, 3, 8, 11, 12, 13], "none": []}


@pytest.mark.parametrize("which", sorted(SUBSETS))
def test_plan_rows_equals_a_brute_force_plan(which):
    g = edge_graph()
    rows = SUBSETS[which]
    items, splits = g.plan_rows(rows)
    want_items, want_splits = brute_force_plan(g.rowptr, rows, L)
    assert items.dtype == np.int64 and splits.dtype == np.int64 and items.shape[1] == 4 and splits.shape[1] == 3
    assert np.array_equal(items, want_items) and np.array_equal(splits, want_splits)
    # slots consecutive from 0, in item order; the items are the graph plan's own, in its order
    cut = items[:, 3] >= 0
    assert np.array_equal(items[cut, 3], np.arange(cut.sum()))
    assert int(splits[:, 2].sum()) == int(cut.sum())
    keep = np.isin(g.items[:, 0], rows)
    assert np.array_equal(items[:, :3], g.items[keep, :3])
    if which == "every row":
        assert np.array_equal(items, g.items) and np.array_equal(splits, g.splits)
    if which == "one cut row":
        assert g.items[g.item_ptr[9], 3] > 0 and items[0, 3] == 0                     # re-based, not copied


def test_plan_rows_refuses_lists_that_are_not_ascending_and_in_range():
    from graphsage_amd._lib import GraphsageAmdError
    g = edge_graph()
    for rows in ([3, 2], [2, 2], [-1, 2], [2, len(DEGS)]):
        with pytest.raises(GraphsageAmdError, match="plan_rows"):
            g.plan_rows(rows)
    before = g.items.copy()
    g.plan_rows(CUT)
    assert np.array_equal(g.items, before), "plan_rows must not write into the graph's plan"


# ------------------------------------------------------------------------------------------------ oracle
def test_oracle_closure_equals_a_set_based_restatement():
    g = edge_graph()
    lists = g.lists()
    n_rows = len(lists)
    for rows in SUBSETS.values():
        want = set(rows)
        for r in rows:
            want |= set(int(c) for c in lists[r])
        got = so.closure(lists, rows)
        assert got.tolist() == sorted(want)
        pos = so.position_map(n_rows, got)
        assert [int(i) for i in np.flatnonzero(pos >= 0)] == sorted(want) and np.array_equal(pos[got], np.arange(len(got)))
    sets, edges = so.receptive_field(lists, [5, 1, 5], 2)
    assert sets[0].tolist() == [1, 5] and sets[1].tolist() == so.closure(lists, [1, 5]).tolist()
    assert sets[2].tolist() == so.closure(lists, sets[1]).tolist()
    assert edges == [DEGS[1] + DEGS[5], sum(DEGS[r] for r in sets[1])]


def test_oracle_subset_pass_equals_the_full_pass():
    """subset_oracle.forward == fullnbr_oracle.forward at the requested rows (float64, 1e-12: the same sums in the same order
    up to the position of the rows), for every aggregator fullnbr_oracle knows."""
    import fullnbr_oracle as fo
    rng = np.random.RandomState(11)
    n, F, D, hid = 40, 6, 4, 5
    lists = [rng.randint(0, n + 1, size=rng.randint(0, 4)) for _ in range(n)] + [np.asarray([n])]
    lists = [nb if len(nb) else np.asarray([n]) for nb in lists]
    feats = rng.randn(n + 1, F)
    nodes = [7, 3, 3, 21]
    for agg in ("mean", "gcn", "maxpool", "meanpool"):
        for concat in (True, False):
            d1 = D * (2 if concat and agg != "gcn" else 1)
            params = {"agg": []}
            for d_in in (F, d1):
                p = {"weights": rng.randn(d_in, D)} if agg == "gcn" else {
                    "neigh_weights": rng.randn(hid if "pool" in agg else d_in, D), "self_weights": rng.randn(d_in, D),
                    "mlp_weights": rng.randn(d_in, hid), "mlp_bias": rng.randn(hid)}
                params["agg"].append(p)
            want = fo.forward(lists, feats, params, agg, concat)[nodes]
            got, sets, _ = so.forward(lists, feats, params, agg, concat, nodes)
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
            assert len(sets[2]) < n + 1


# ------------------------------------------------------------------------------------------------ flags
@pytest.mark.parametrize("driver", ["supervised_train", "unsupervised_train"])
def test_both_drivers_parse_the_flag(driver):
    import importlib
    mod = importlib.import_module("graphsage_amd." + driver)
    assert mod.build_flags([]).embed_nodes == ""
    assert mod.build_flags(["--embed_nodes", "ids.txt"]).embed_nodes == "ids.txt"


@pytest.mark.parametrize("driver", ["supervised_train", "unsupervised_train"])
@pytest.mark.parametrize("model", ["graphsage_seq", "n2v"])
def test_models_without_layers_to_restrict_are_refused_before_training(driver, model, tmp_path, capsys):
    import importlib
    mod = importlib.import_module("graphsage_amd." + driver)
    ids = tmp_path / "ids.txt"
    ids.write_text("1\n2\n")
    with pytest.raises(SystemExit) as ei:
        mod.main(["--synthetic", "small", "--model", model, "--embed_nodes", str(ids)])
    assert "--embed_nodes" in str(ei.value) and model in str(ei.value)
    assert "Loading training data" not in capsys.readouterr().out


@pytest.mark.parametrize("driver", ["supervised_train", "unsupervised_train"])
def test_a_missing_file_is_refused_before_training(driver, tmp_path, capsys):
    import importlib
    mod = importlib.import_module("graphsage_amd." + driver)
    with pytest.raises(SystemExit) as ei:
        mod.main(["--synthetic", "small", "--embed_nodes", str(tmp_path / "nothing.txt")])
    assert "--embed_nodes" in str(ei.value) and "no such file" in str(ei.value)
    assert "Loading training data" not in capsys.readouterr().out


@pytest.mark.parametrize("driver", ["supervised_train", "unsupervised_train"])
@pytest.mark.parametrize("bad", ["99999999", "-1", "seven"])
def test_an_id_the_graph_does_not_have_is_refused_before_training(driver, bad, tmp_path, capsys, monkeypatch):
    import importlib
    mod = importlib.import_module("graphsage_amd." + driver)
    ids = tmp_path / "ids.txt"
    ids.write_text("0\n%s\n3\n" % bad)
    monkeypatch.setattr(mod, "train", lambda *a, **k: pytest.fail("training started"))
    with pytest.raises(SystemExit) as ei:
        mod.main(["--synthetic", "small", "--max_walk_pairs", "100", "--embed_nodes", str(ids)]
                 if driver == "unsupervised_train" else ["--synthetic", "small", "--embed_nodes", str(ids)])
    assert "--embed_nodes" in str(ei.value) and "no node %s" % bad in str(ei.value)
    assert "Done loading training data" in capsys.readouterr().out


def test_embed_nodes_rows_go_through_the_id_map_and_keep_file_order():
    from graphsage_amd import supervised_train as st

    class G(object):
        n_nodes = 5
        id_map = {"a": 3, "b": 0, "7": 4}

    assert st.embed_nodes_rows(G, ["7", "a", "a", "b"], "f").tolist() == [4, 3, 3, 0]
    with pytest.raises(SystemExit, match="no node 3"):
        st.embed_nodes_rows(G, ["a", "3"], "f")                      # 3 is a row, not an ORIGINAL id
    G.id_map = None
    assert st.embed_nodes_rows(G, ["4", "0"], "f").tolist() == [4, 0]
    with pytest.raises(SystemExit, match="no node 5"):
        st.embed_nodes_rows(G, ["5"], "f")                           # the pad row is no node
    with pytest.raises(SystemExit, match="lists no node"):
        st.embed_nodes_rows(G, [], "f")
    line = st.embed_nodes_line(17, {"rows": [16, 40, 90], "edges": [50, 130], "n_rows": 301}, 0.25)
    assert line == "Receptive-field inference: nodes= 17 rows= 16 / 40 / 90 of 301 edges= 180 time= 0.25000"
