"""CPU suite of full-neighborhood inference.

  * tests/fullnbr_oracle.py (the NumPy layer-wise pass) == the REFERENCE'S OWN RUN wherever the reference computes a
    full-neighborhood pass itself: num_samples == max_degree at every layer (its sampler then returns a permutation of each
    padded row).  Five fixtures, float64 twin at 1e-9 (tests/test_ref_pin.py's tolerance); step 1 runs under the reference's
    own post-Adam weights (non-zero MLP bias: the pad row's hidden state is not zero).
  * the generator reproduces the four committed fixtures;
  * the work-item plan, FullGraph.from_csr / from_padded, graph validation, the C ABI surface, the driver flags.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fullnbr_oracle as fo
from ref_fixtures import Fixture

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("GRAPHSAGE_REFERENCE", "/root/reference")
NEW = ["full_gcn", "full_maxpool", "full_meanpool_sigmoid", "full_unsup_mean"]
FIXTURES = ["sup_mean_full_degree"] + NEW
TOL64 = dict(rtol=1e-9, atol=1e-9)


def weights_prefix(s, prec):
    return "init/" if s == 0 else "s%d/%s/after/" % (s - 1, prec)


def pinned_steps(fx):
    """Steps whose weights the fixture holds: step 0 (init) and every step after one whose post-Adam weights were kept."""
    return [s for s in range(fx.n_steps) if s == 0 or fx.has("s%d/64/after/agg0/%s" % (s - 1, "weights" if fx.agg == "gcn"
                                                                                         else "neigh_weights"))]


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_the_reference_run_at_full_degree(name):
    fx = Fixture(name)
    c = fx.cfg
    assert c["num_samples"] == [c["max_degree"]] * fx.K and fx["graph/adj_train"].shape[1] == c["max_degree"]
    sup = c["kind"] == "supervised"
    lists = fo.padded_lists(fx["graph/adj_train"])
    feats = fx["graph/feats"].astype(np.float64)
    steps = pinned_steps(fx)
    assert steps[0] == 0 and (name == "sup_mean_full_degree" or len(steps) >= 2)
    for s in steps:
        p = "s%d/" % s
        params = fx.params(weights_prefix(s, "64"), np.float64, supervised=sup)
        emb = fo.forward(lists, feats, params, fx.agg, c["concat"])
        if sup:
            b = fx[p + "batch"]
            np.testing.assert_allclose(emb[b], fx[p + "64/outputs1"], err_msg="outputs1 step %d" % s, **TOL64)
            node_preds, preds = fo.predict(emb[b], params, c["sigmoid"])
            np.testing.assert_allclose(node_preds, fx[p + "64/node_preds"], err_msg="node_preds step %d" % s, **TOL64)
            np.testing.assert_allclose(preds, fx[p + "64/preds"], err_msg="preds step %d" % s, **TOL64)
        else:
            for key, ids in (("outputs1", "batch1"), ("outputs2", "batch2"), ("neg_outputs", "neg_samples")):
                np.testing.assert_allclose(emb[fx[p + ids]], fx[p + "64/" + key], err_msg="%s step %d" % (key, s), **TOL64)


def test_trained_pad_row_is_part_of_the_pin():
    """The trap of this feature: after one Adam step the pooling MLP's bias is +-0.01, the pad row's hidden state
    relu(0 . W + b) is not zero, and zeroing it instead of computing it moves the reference's own outputs."""
    fx = Fixture("full_maxpool")
    params = fx.params(weights_prefix(1, "64"), np.float64)
    assert np.abs(params["agg"][0]["mlp_bias"]).max() > 5e-3
    lists = fo.padded_lists(fx["graph/adj_train"])
    feats = fx["graph/feats"].astype(np.float64)
    N = fx.n_nodes
    assert np.array_equal(lists[N], np.full(fx.cfg["max_degree"], N))
    H1 = fo.layer(lists, feats, params["agg"][0], "maxpool", True, last=False)
    assert np.abs(H1[N]).max() > 0


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "graphsage")), reason="the reference's sources are not on this machine")
def test_generator_reproduces_the_committed_fixtures(tmp_path):
    env = dict(os.environ, REF_FIXTURE_DIR=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(HERE, "golden", "make_ref_fullnbr_fixtures.py")], env=env,
                          stdout=subprocess.DEVNULL)
    for name in NEW:
        a = np.load(os.path.join(HERE, "golden", "ref_%s.npz" % name))
        b = np.load(os.path.join(str(tmp_path), "ref_%s.npz" % name))
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)


def test_committed_fixtures_stay_small():
    for name in NEW:
        assert os.path.getsize(os.path.join(HERE, "golden", "ref_%s.npz" % name)) < (1 << 20), name


# ------------------------------------------------------------------------------------------------ work-item plan
@pytest.mark.parametrize("L", [512, 8])
def test_work_item_plan_covers_every_edge_once_and_in_order(L):
    from graphsage_amd.inference import plan_work_items
    degs = [0, 1, L - 1, L, L + 1, 2 * L, 3 * L + 7, 0, 5, 2 * L + 1, 0]
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    items, item_ptr, splits = plan_work_items(rowptr, L)
    assert items.dtype == np.int64 and items.shape[1] == 4 and splits.shape[1] == 3
    assert item_ptr[0] == 0 and item_ptr[-1] == len(items) and len(item_ptr) == len(degs) + 1
    assert np.all(np.diff(items[:, 0]) >= 0)
    next_slot = 0
    split_rows = {int(r): (int(s0), int(n)) for r, s0, n in splits}
    for r, deg in enumerate(degs):
        mine = items[item_ptr[r]:item_ptr[r + 1]]
        assert len(mine) >= 1 and np.all(mine[:, 0] == r)
        assert mine[:, 2].max() <= L and mine[:, 2].min() >= 0
        # every edge exactly once, in order
        covered = np.concatenate([np.arange(e0, e0 + cnt) for _, e0, cnt, _ in mine]) if deg else np.zeros(0, np.int64)
        assert np.array_equal(covered, np.arange(rowptr[r], rowptr[r + 1]))
        if deg <= L:
            assert len(mine) == 1 and mine[0, 3] == -1 and r not in split_rows            # no partials
        else:
            assert len(mine) == -(-deg // L)
            assert np.array_equal(mine[:, 3], next_slot + np.arange(len(mine)))           # contiguous per row
            assert split_rows[r] == (next_slot, len(mine))
            next_slot += len(mine)
    assert len(split_rows) == sum(d > L for d in degs)
    assert np.all(np.diff(splits[:, 0]) > 0)


def test_row_windows_select_their_items_splits_and_slots():
    from graphsage_amd.inference import FullGraph
    L = 4
    degs = [1, 9, 0, 4, 5, 13, 2]
    n = len(degs) - 1                     # the last row is the pad row
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    col = (np.arange(rowptr[-1]) % (n + 1)).astype(np.int32)
    g = FullGraph(rowptr, col, n, split_len=L)
    assert g.window(0, g.n_rows) == ((0, len(g.items)), (0, 3), (0, 3 + 2 + 4))
    (i0, i1), (s0, s1), (t0, t1) = g.window(2, 3)             # rows 2, 3, 4: one split row (4) of two partials
    assert np.array_equal(np.unique(g.items[i0:i1, 0]), [2, 3, 4]) and (s0, s1) == (1, 2) and (t0, t1) == (3, 5)
    assert g.window(2, 2) == ((i0, i0 + 2), (1, 1), (0, 0))   # no split row: no slots
    assert [w for w in g.windows(3)] == [(0, 3), (3, 3), (6, 1)]


# ------------------------------------------------------------------------------------------------ graph constructors
def test_from_csr_points_isolated_nodes_and_the_pad_row_at_the_pad_node():
    from graphsage_amd.inference import FullGraph
    fx = Fixture("sup_mean_full_degree")
    rp, col, N = fx["graph/full_rowptr"], fx["graph/full_col"], fx.n_nodes
    deg = np.diff(rp)
    assert (deg == 0).sum() >= 3                          # the fixture graph has degree-0 nodes
    g = FullGraph.from_csr(rp, col, N)
    assert g.n_rows == N + 1 and g.col.dtype == np.int32 and g.rowptr.dtype == np.int64
    lists, want = g.lists(), fx.lists("full")
    for v in range(N):
        assert np.array_equal(lists[v], want[v] if deg[v] else [N]), v
    assert np.array_equal(lists[N], [N])
    assert [list(x) for x in lists] == [list(x) for x in fo.csr_lists(rp, col, N)]


def test_from_padded_round_trips_the_table():
    from graphsage_amd.inference import FullGraph
    adj = Fixture("full_gcn")["graph/adj_train"]
    g = FullGraph.from_padded(adj)
    assert g.n_nodes == adj.shape[0] - 1 and g.nnz == adj.size
    assert np.array_equal(np.stack(g.lists()), adj)
    assert np.array_equal(g.lists()[-1], np.full(adj.shape[1], adj.shape[0] - 1))


def test_bad_graphs_are_refused_at_construction():
    from graphsage_amd._lib import GraphsageAmdError
    from graphsage_amd.inference import FullGraph
    N = 4
    rp = np.asarray([0, 2, 2, 3, 5, 6], np.int64)          # N + 1 rows
    col = np.asarray([1, 2, 0, 4, 1, 4], np.int32)
    FullGraph(rp, col, N)
    bad_col = col.copy(); bad_col[3] = N + 1
    with pytest.raises(GraphsageAmdError, match="column ids"):
        FullGraph(rp, bad_col, N)
    neg_col = col.copy(); neg_col[0] = -1
    with pytest.raises(GraphsageAmdError, match="column ids"):
        FullGraph(rp, neg_col, N)
    with pytest.raises(GraphsageAmdError, match="non-decreasing"):
        FullGraph(np.asarray([0, 2, 1, 3, 5, 6], np.int64), col, N)
    with pytest.raises(GraphsageAmdError, match=r"rowptr\[-1\]"):
        FullGraph(np.asarray([0, 2, 2, 3, 5, 7], np.int64), col, N)
    with pytest.raises(GraphsageAmdError):
        FullGraph(rp[:-1], col, N)
    # the same through the constructors
    with pytest.raises(GraphsageAmdError, match="column ids"):
        FullGraph.from_csr(rp[:-1], bad_col[:5], N)
    with pytest.raises(GraphsageAmdError):
        FullGraph.from_csr(np.asarray([0, 2, 1, 3, 5], np.int64), col[:5], N)
    with pytest.raises(GraphsageAmdError):
        FullGraph.from_csr(np.asarray([0, 2, 2, 3, 6], np.int64), col[:5], N)
    with pytest.raises(GraphsageAmdError, match="column ids"):
        FullGraph.from_padded(np.asarray([[1, 5], [0, 4], [4, 4], [4, 4], [4, 4]]))


# ------------------------------------------------------------------------------------------------ binding
def test_header_binding_and_error_reporting():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    for name in ("gs_csr_reduce_fwd", "gs_csr_reduce_ws_bytes"):
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib._PROTOS
    for name, code in (("GS_CSR_MEAN", _lib.CSR_MEAN), ("GS_CSR_MEAN_SELF", _lib.CSR_MEAN_SELF), ("GS_CSR_MAX", _lib.CSR_MAX)):
        assert re.search(r"#define %s %d\b" % (name, code), header)
    assert len({_lib.CSR_MEAN, _lib.CSR_MEAN_SELF, _lib.CSR_MAX}) == 3
    assert _lib.GS_ABI_VERSION == 12 and re.search(r"#define GS_ABI_VERSION 12\b", header)
    lib = _lib.load()
    assert lib.gs_abi_version() == 12
    assert lib.gs_csr_reduce_fwd(None, None) == -1 and b"gs_csr_reduce_fwd" in lib.gs_last_error()
    q = _lib.CsrReduceDesc()               # every pointer null
    q.n_rows, q.n, q.d, q.split_len, q.n_items, q.item1 = 4, 4, 8, 512, 4, 4
    assert lib.gs_csr_reduce_fwd(ctypes.addressof(q), None) == -1 and b"gs_csr_reduce_fwd" in lib.gs_last_error()
    q.op = 7
    assert lib.gs_csr_reduce_fwd(ctypes.addressof(q), None) == -1 and b"unknown op" in lib.gs_last_error()
    assert lib.gs_csr_reduce_ws_bytes(3, 602, None) == -1 and b"gs_csr_reduce_ws_bytes" in lib.gs_last_error()
    out = ctypes.c_int64(-1)
    assert lib.gs_csr_reduce_ws_bytes(3, 602, ctypes.byref(out)) == 0 and out.value == 3 * 3 * 256 * 4
    # the descriptor goes by pointer: it is not one of the structs gs_abi_struct_sizes reports
    sizes = (ctypes.c_int32 * 16)()
    assert lib.gs_abi_struct_sizes(sizes, 16) == 8


# ------------------------------------------------------------------------------------------------ flags
def test_both_drivers_parse_the_flag():
    from graphsage_amd import supervised_train as st
    from graphsage_amd import unsupervised_train as ut
    for mod in (st, ut):
        assert mod.build_flags([]).full_inference is False
        assert mod.build_flags(["--full_inference"]).full_inference is True
        assert mod.build_flags(["--full_inference", "true"]).full_inference is True
        assert mod.build_flags(["--full_inference", "false"]).full_inference is False


@pytest.mark.parametrize("driver,model", [("supervised_train", "graphsage_seq"), ("supervised_train", "n2v"),
                                          ("unsupervised_train", "graphsage_seq"), ("unsupervised_train", "n2v")])
def test_models_without_a_full_neighborhood_form_are_refused_before_training(driver, model, capsys):
    import importlib
    mod = importlib.import_module("graphsage_amd." + driver)
    with pytest.raises(SystemExit) as ei:
        mod.main(["--synthetic", "small", "--model", model, "--full_inference"])
    assert "--full_inference" in str(ei.value) and model in str(ei.value)
    assert "Loading training data" not in capsys.readouterr().out


def test_seq_aggregator_has_no_full_neighborhood_form():
    from graphsage_amd._lib import GraphsageAmdError
    from graphsage_amd.aggregators import SeqAggregator
    with pytest.raises(GraphsageAmdError, match="full-neighborhood"):
        SeqAggregator.infer_full(object.__new__(SeqAggregator), None, None)
