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
from graphsage_amd import inits
from graphsage_amd.inference import SPLIT_LEN, FullGraph
from ref_fixtures import Fixture
from test_full_inference_gpu import COMMON, SUP, build_unsupervised, files_under, legs
from test_ref_pin_gpu import build_supervised, load_weights
import fullnbr_oracle as fo
import subset_oracle as so

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)
N, F, C, L = 300, 20, 5, SPLIT_LEN
HUB, ISOLATED = 40, 77
_cache = {}


def world():
    """rowptr / col of the true graph, its padded twin, features (pad row zero), and both FullGraphs with their lists."""
    if "w" in _cache:
        return _cache["w"]
    rng = np.random.RandomState(2)
    degs = rng.poisson(3.0, size=N)
    degs[HUB], degs[ISOLATED] = 2 * L + 77, 0
    lists = [rng.randint(0, N, size=d) for d in degs]
    lists[HUB] = rng.randint(100, 120, size=degs[HUB])          # the hub lists 20 ids over and over: its field stays small
    for v in range(N):                                          # nobody but node 41 lists the hub or the isolated node
        lists[v][np.isin(lists[v], [HUB, ISOLATED])] = (v + 1) % 30
    lists[41] = np.asarray([HUB, 41, 7])                        # ... with a self-loop
    degs = np.asarray([len(x) for x in lists])
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    col = np.concatenate(lists).astype(np.int32)
    adj = np.full((N + 1, 6), N, np.int64)
    for v in range(N):
        if degs[v]:
            adj[v] = lists[v][rng.randint(0, degs[v], size=6)]
    feats = np.concatenate([rng.randn(N, F).astype(np.float32), np.zeros((1, F), np.float32)])
    g_csr = FullGraph.from_csr(rowptr, col, N)
    g_pad = FullGraph.from_padded(adj)
    assert g_csr.splits.shape[0] == 1 and g_csr.splits[0, 0] == HUB and g_csr.splits[0, 2] == 3 and g_pad.splits.shape[0] == 0
    assert np.array_equal(g_csr.lists()[ISOLATED], [N])
    _cache["w"] = dict(adj=adj, feats=feats, deg=degs, graphs={"csr": (g_csr, g_csr.lists()), "padded": (g_pad, g_pad.lists())})
    return _cache["w"]


MODELS = {
    # name: (aggregator, dim, layers, identity_dim, supervised, sigmoid); concat everywhere but gcn, as the reference runs them
    "mean_narrow": ("mean", 8, 2, 0, True, False),              # dim < F: the reduce runs over H . W_neigh
    "mean_plain": ("mean", 24, 2, 0, True, True),               # dim >= F at layer 0: the plain form; sigmoid head
    "gcn_narrow": ("gcn", 8, 2, 0, True, False),
    "gcn_plain": ("gcn", 24, 2, 0, True, False),
    "maxpool": ("maxpool", 8, 2, 0, True, False),
    "meanpool": ("meanpool", 8, 2, 0, True, True),
    "twomaxpool": ("twomaxpool", 8, 2, 0, True, False),
    "mean_3layer": ("mean", 8, 3, 0, True, False),
    "mean_identity": ("mean", 8, 2, 4, True, False),
    "unsup_mean": ("mean", 8, 2, 0, False, False),
}


def build(name):
    """(model, oracle params in float64, feature table as the device holds it): random weights in EVERY variable, the Dense biases
    included, so that the pad row's hidden state is not zero."""
    from graphsage_amd.models import Placeholder, SAGEInfo, SampleAndAggregate
    from graphsage_amd.neigh_samplers import AdjInfo, PaddedAdjacency, UniformNeighborSampler
    from graphsage_amd.supervised_models import SupervisedGraphsage
    agg, dim, K, idim, sup, sigmoid = MODELS[name]
    w = world()
    eng.reset_engine()
    inits.set_seed(1)
    e = eng.get_engine()
    ph = {'labels': Placeholder('labels'), 'batch': Placeholder('batch1'), 'batch1': Placeholder('batch1'),
          'batch2': Placeholder('batch2'), 'neg_samples': Placeholder('neg'), 'dropout': Placeholder('dropout', 0.),
          'batch_size': Placeholder('batch_size')}
    adj_info = AdjInfo(PaddedAdjacency(w["adj"], e.device))
    sampler = UniformNeighborSampler(adj_info)
    layer_infos = [SAGEInfo("node", sampler, 3, dim) for _ in range(K)]
    if sup:
        model = SupervisedGraphsage(C, ph, w["feats"], adj_info, w["deg"], layer_infos, concat=(agg != "gcn"),
                                    aggregator_type=agg, sigmoid_loss=sigmoid, identity_dim=idim)
    else:
        model = SampleAndAggregate(ph, w["feats"], adj_info, w["deg"], layer_infos, concat=(agg != "gcn"), aggregator_type=agg,
                                   identity_dim=idim)
    rng = np.random.RandomState(len(name))

    def fill(v, scale):
        a = (rng.randn(*v.numpy().shape) * scale).astype(np.float32)
        v.assign(a)
        return a.astype(np.float64)

    params = {"agg": []}
    for a in model.aggregators:
        p = {k: fill(v, 0.3) for k, v in sorted(a.vars.items())}
        mlp = [(fill(l.vars['weights'], 0.2), fill(l.vars['bias'], 0.2).reshape(-1)) for l in getattr(a, "mlp_layers", [])]
        if len(mlp) == 1:
            p["mlp_weights"], p["mlp_bias"] = mlp[0]                # fullnbr_oracle's names for the one-Dense aggregators
        elif mlp:
            p["mlp"] = mlp
        if "bias" in p:
            p["bias"] = p["bias"].reshape(-1)
        params["agg"].append(p)
    if sup:
        params["node_pred"] = {"weights": fill(model.node_pred.vars['weights'], 0.5),
                               "bias": fill(model.node_pred.vars['bias'], 0.5).reshape(-1)}
    if model.embeds is not None:
        fill(model.embeds, 0.5)
        model._refresh_embeds()
    e.sync()
    feats = model.features.numpy().astype(np.float64)
    assert feats.shape == (N + 1, F + idim) and len(model.aggregators) == K
    return model, params, feats


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
        rng = np.random.RandomState(9)
        many = rng.permutation(N)[:16].tolist()
        many.insert(5, many[11])                               # 17 unsorted ids, one of them twice
        assert len(many) == 17 and len(set(many)) == 16 and many != sorted(many)
        _cache[key] = {"one": [one], "isolated": [ISOLATED], "hub": [HUB], "many": many, "all": list(range(N))}
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
