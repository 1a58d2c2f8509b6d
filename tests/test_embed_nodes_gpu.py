"""-m gpu: embed_nodes / predict_nodes (exact inference for a node subset from its receptive field: gs_frontier_expand,
gs_csr_reduce_rows and the existing dense kernels) == tests/subset_oracle.py in float64, == embed_full / predict_full on the
same model and graph, == the reference's own numbers through the pins tests/golden/ref_full_*.npz, and the two drivers'
--embed_nodes outputs.

The graph: 300 nodes + the pad row, sparse (mean degree about 3), one hub of 2 L + 77 edges (a cut row: three partials), one
isolated node (from_csr points it at the pad node); built with FullGraph.from_csr, and as a padded table (every row re-sampled
to width 6, no cut row) with FullGraph.from_padded.

Tolerance: rtol = atol = 1e-4 everywhere, the project's float tolerance for unit-norm embeddings and probabilities.  The
comparison with embed_full is NOT bitwise although the reduce gives the same bits: the contractions around it run over |S_l| rows
here and over N + 1 rows there and may take another tile form (another order of the k-sum) at another row count.  Two runs of
embed_nodes itself agree bit for bit."""
import re

import numpy as np
import pytest

from graphsage_amd import engine as eng
from graphsage_amd.inference import FullGraph
from infer_cases import HUB, ISOLATED, MODELS, N, build, many_request, world
from ref_fixtures import Fixture
from test_full_inference_gpu import COMMON, SUP, build_unsupervised, files_under, legs
from test_ref_pin_gpu import build_supervised, load_weights
import fullnbr_oracle as fo
import subset_oracle as so

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)
_cache = {}


def requests(lists):
    """The five requests; the one-node request is picked with the oracle so that the partial path is really the one under test."""
    key = ("req", id(lists))
    if key not in _cache:
        one = None
        for v in range(N):
            sets, _ = so.receptive_field(lists, [v], 2)
            if len(sets[2]) < N // 4 and HUB not in sets[2] and len(sets[2]) > len(sets[1]) > 1:
                one = v
                break
        assert one is not None
        _cache[key] = {"one": [one], "isolated": [ISOLATED], "hub": [HUB], "many": many_request(), "all": list(range(N))}
    return _cache[key]


def ask(model, graph, nodes):
    if hasattr(model, "predict_nodes"):
        return model.predict_nodes(graph, nodes)
    emb, stats = model.embed_nodes(graph, nodes)
    return emb, None, stats


@pytest.mark.parametrize("name", sorted(MODELS))
def test_embed_nodes_equals_the_oracle_and_the_full_pass(dev, name):
    agg, dim, K, idim, sup, sigmoid = MODELS[name]
    model, params, feats = build(name)
    concat = agg != "gcn"
    graph, lists = world()["graphs"]["csr"]
    full = model.predict_full(graph) if sup else (model.embed_full(graph), None)
    if agg != "twomaxpool":                                    # embed_full itself against fullnbr_oracle, on this graph
        np.testing.assert_allclose(full[0], fo.forward(lists, feats, params, agg, concat)[:N], **TOL)
    for what, nodes in sorted(requests(lists).items()):
        want, sets, edges = so.forward(lists, feats, params, agg, concat, nodes)
        if what == "one" and K == 2:
            # the partial path is the one under test: a small field, and no cut row anywhere in it
            assert len(sets[-1]) < N // 4 and HUB not in sets[-1]
        if what == "hub":
            assert HUB in sets[0] and (K != 2 or len(sets[-1]) < N // 2)
        emb, preds, stats = ask(model, graph, nodes)
        assert emb.shape == (len(nodes), dim * (2 if concat else 1)) and emb.dtype == np.float32, what
        assert stats == {"rows": [len(S) for S in sets], "edges": edges, "n_rows": N + 1}, what
        np.testing.assert_allclose(emb, want, err_msg=what, **TOL)
        np.testing.assert_allclose(emb, full[0][nodes], err_msg=what, **TOL)
        np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1.0, rtol=1e-5)
        if sup:
            np.testing.assert_allclose(preds, fo.predict(want, params, sigmoid)[1], err_msg=what, **TOL)
            np.testing.assert_allclose(preds, full[1][nodes], err_msg=what, **TOL)
        if what == "many":
            assert np.array_equal(emb[5], emb[12])             # the duplicate request is answered twice, in request order
            again = ask(model, graph, nodes)
            assert np.array_equal(again[0], emb) and (not sup or np.array_equal(again[1], preds)), "two runs must agree bit for bit"
        if what == "all":
            assert stats["rows"][0] == N and stats["rows"][-1] == N + 1          # the isolated node pulls the pad row in


@pytest.mark.parametrize("name", ["mean_narrow", "maxpool", "gcn_plain"])
def test_padded_graph_and_device_resident_csr(dev, name):
    """FullGraph.from_padded (the reference's multigraph: no cut row, the pad row [N, N, ...]) and from_csr on device tensors
    (the graph only exists in HBM: the receptive field is found there)."""
    import torch
    agg, dim, K, idim, sup, sigmoid = MODELS[name]
    model, params, feats = build(name)
    graph, lists = world()["graphs"]["padded"]
    nodes = requests(world()["graphs"]["csr"][1])["many"] + [ISOLATED]
    want, sets, edges = so.forward(lists, feats, params, agg, agg != "gcn", nodes)
    emb, preds, stats = ask(model, graph, nodes)
    assert stats["rows"] == [len(S) for S in sets] and stats["edges"] == edges and N in sets[1]
    np.testing.assert_allclose(emb, want, **TOL)
    np.testing.assert_allclose(preds, fo.predict(want, params, sigmoid)[1], **TOL)
    host, host_lists = world()["graphs"]["csr"]
    devg = FullGraph(torch.from_numpy(host.rowptr).to(dev), torch.from_numpy(host.col).to(dev), N)
    a = ask(model, host, nodes)
    b = ask(model, devg, nodes)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_requests_are_checked_and_the_seq_model_refuses(dev):
    from graphsage_amd._lib import GraphsageAmdError
    model, params, feats = build("mean_narrow")
    graph, lists = world()["graphs"]["csr"]
    with pytest.raises(GraphsageAmdError, match="node ids"):
        model.embed_nodes(graph, [3, N + 1])
    with pytest.raises(GraphsageAmdError, match="node ids"):
        model.embed_nodes(graph, [-1])
    with pytest.raises(GraphsageAmdError, match="at least one node"):
        model.embed_nodes(graph, [])
    with pytest.raises(GraphsageAmdError, match="FullGraph"):
        model.embed_nodes(None, [3])
    emb, stats = model.embed_nodes(graph, [N])                 # the pad row is a row like any other
    assert emb.shape == (1, 16) and stats["rows"] == [1, 1, 1]
    fx = Fixture("sup_seq")
    e, ph, adj_info, sampler, seq = build_supervised(fx)
    with pytest.raises(GraphsageAmdError, match="full-neighborhood"):
        seq.predict_nodes(FullGraph.from_padded(fx["graph/adj_train"]), [1, 2])


# ------------------------------------------------------------------------------------------------ reference pins
@pytest.mark.parametrize("name", SUP)
def test_predict_nodes_holds_the_reference_pins(dev, name):
    fx = Fixture(name)
    e, ph, adj_info, sampler, model = build_supervised(fx)
    graph = FullGraph.from_padded(fx["graph/adj_train"])
    for s, prefix in legs(fx):
        load_weights(model, fx, prefix)
        p = "s%d/" % s
        emb, preds, stats = model.predict_nodes(graph, fx[p + "batch"])
        np.testing.assert_allclose(emb, fx[p + "32/outputs1"], err_msg="outputs1 step %d" % s, **TOL)
        np.testing.assert_allclose(preds, fx[p + "32/preds"], err_msg="preds step %d" % s, **TOL)
        assert stats["rows"][0] == len(np.unique(fx[p + "batch"])) and stats["n_rows"] == fx.n_nodes + 1


def test_embed_nodes_holds_the_unsupervised_reference_pin(dev):
    fx = Fixture("full_unsup_mean")
    e, model = build_unsupervised(fx)
    graph = FullGraph.from_padded(fx["graph/adj_train"])
    for s, prefix in legs(fx):
        load_weights(model, fx, prefix, supervised=False)
        p = "s%d/" % s
        for key, ids in (("outputs1", "batch1"), ("outputs2", "batch2"), ("neg_outputs", "neg_samples")):
            emb, stats = model.embed_nodes(graph, fx[p + ids])
            np.testing.assert_allclose(emb, fx[p + "32/" + key], err_msg="%s step %d" % (key, s), **TOL)


# ------------------------------------------------------------------------------------------------ drivers
LINE = r"Receptive-field inference: nodes= 5 rows= 4 / \d+ / \d+ of \d+ edges= \d+ time= \d+\.\d{5}"


def test_supervised_driver_embed_nodes(dev, tmp_path, capsys):
    from graphsage_amd import supervised_train as st
    ids = tmp_path / "ids.txt"
    ids.write_text("12\n3\n12\n250\n\n7\n")
    eng.reset_engine()
    st.main(COMMON + ["--model", "graphsage_mean", "--validate_iter", "10", "--print_every", "5", "--base_log_dir",
                      str(tmp_path / "on"), "--embed_nodes", str(ids)])
    out = capsys.readouterr().out
    assert re.search(LINE, out)
    files = files_under(tmp_path / "on")
    emb, preds = np.load(files["embed_nodes.npy"]), np.load(files["embed_nodes_preds.npy"])
    assert emb.shape == (5, 64) and emb.dtype == np.float32 and preds.shape[0] == 5
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1.0, rtol=1e-5)
    assert np.array_equal(emb[0], emb[2]) and not np.array_equal(emb[0], emb[1])
    assert open(files["embed_nodes.txt"]).read().split("\n") == ["12", "3", "12", "250", "7"]
    assert "val_stats.txt" in files and "val_stats_full.txt" not in files
    eng.reset_engine()
    st.main(COMMON + ["--model", "graphsage_mean", "--validate_iter", "10", "--print_every", "5", "--base_log_dir",
                      str(tmp_path / "off")])
    assert "Receptive-field" not in capsys.readouterr().out
    off = files_under(tmp_path / "off")
    assert "val_stats.txt" in off and not any(f.startswith("embed_nodes") for f in off)


def test_unsupervised_driver_embed_nodes(dev, tmp_path, capsys, monkeypatch):
    from graphsage_amd import supervised_train as st
    from graphsage_amd import unsupervised_train as ut
    kept = {}
    real = st.save_embed_nodes

    def spy(model, minibatch, n_nodes, rows, out_dir, supervised):
        real(model, minibatch, n_nodes, rows, out_dir, supervised)
        kept["full"] = model.embed_full(st.full_graph(minibatch, n_nodes), nodes=rows)

    monkeypatch.setattr(st, "save_embed_nodes", spy)
    ids = tmp_path / "ids.txt"
    ids.write_text("12\n3\n12\n250\n7")
    eng.reset_engine()
    ut.main(COMMON + ["--model", "graphsage_mean", "--learning_rate", "0.001", "--max_walk_pairs", "4000", "--validate_iter",
                      "10", "--validate_batch_size", "256", "--base_log_dir", str(tmp_path / "on"), "--embed_nodes", str(ids)])
    assert re.search(LINE, capsys.readouterr().out)
    files = files_under(tmp_path / "on")
    emb = np.load(files["embed_nodes.npy"])
    assert emb.shape == (5, 64) and "embed_nodes_preds.npy" not in files
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1.0, rtol=1e-5)
    np.testing.assert_allclose(emb, kept["full"], **TOL)       # the rows of embed_full on the driver's own test graph
    assert open(files["embed_nodes.txt"]).read().split("\n") == ["12", "3", "12", "250", "7"]
    assert "val.npy" in files and "val_full.npy" not in files
