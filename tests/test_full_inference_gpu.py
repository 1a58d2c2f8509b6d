"""-m gpu: embed_full / predict_full (exact layer-wise inference over whole neighbor lists, gs_csr_reduce_fwd + the existing
dense kernels) == the REFERENCE'S OWN RUN where the reference computes that pass itself (num_samples == max_degree: five
fixtures, four aggregators, both heads, init weights and the reference's post-Adam weights with a non-zero pad-row hidden
state), == tests/fullnbr_oracle.py on the true graph (degree-0 nodes -> the pad node) and for a 3-layer model, and the two
drivers' --full_inference outputs.  rtol = atol = 1e-4, the tolerance of every reference pin."""
import os
import re

import numpy as np
import pytest

from graphsage_amd import engine as eng
from graphsage_amd.inference import FullGraph
from ref_fixtures import Fixture
from test_ref_pin_gpu import build_supervised, load_weights
import fullnbr_oracle as fo

pytestmark = pytest.mark.gpu
SUP = ["sup_mean_full_degree", "full_gcn", "full_maxpool", "full_meanpool_sigmoid"]
TOL = dict(rtol=1e-4, atol=1e-4)


def build_unsupervised(fx):
    from graphsage_amd import inits
    from graphsage_amd.models import Placeholder, SAGEInfo, SampleAndAggregate
    from graphsage_amd.neigh_samplers import AdjInfo, PaddedAdjacency, UniformNeighborSampler
    c = fx.cfg
    eng.reset_engine()
    inits.set_seed(1)
    e = eng.get_engine()
    ph = {'batch1': Placeholder('batch1'), 'batch2': Placeholder('batch2'), 'neg_samples': Placeholder('neg'),
          'dropout': Placeholder('dropout', 0.), 'batch_size': Placeholder('batch_size')}
    adj_info = AdjInfo(PaddedAdjacency(fx["graph/adj_train"], e.device))
    sampler = UniformNeighborSampler(adj_info)
    layer_infos = [SAGEInfo("node", sampler, s, fx.out_dim) for s in c["num_samples"]]
    model = SampleAndAggregate(ph, fx["graph/feats"], adj_info, fx["graph/deg"], layer_infos, concat=c["concat"],
                               aggregator_type=fx.agg, learning_rate=c["learning_rate"], weight_decay=c["weight_decay"],
                               neg_sample_size=c["neg_sample_size"])
    return e, model


def legs(fx):
    """(step, weight prefix): the initial weights, then the reference's own weights after its first Adam step."""
    return [(0, "init/"), (1, "s0/32/after/")] if fx.n_steps >= 2 else [(0, "init/")]


@pytest.mark.parametrize("name", SUP)
def test_predict_full_equals_the_reference_run(dev, name):
    fx = Fixture(name)
    e, ph, adj_info, sampler, model = build_supervised(fx)
    graph = FullGraph.from_padded(fx["graph/adj_train"])
    assert len(legs(fx)) == (1 if name == "sup_mean_full_degree" else 2)
    for s, prefix in legs(fx):
        load_weights(model, fx, prefix)
        p = "s%d/" % s
        emb, preds = model.predict_full(graph, nodes=fx[p + "batch"])
        np.testing.assert_allclose(emb, fx[p + "32/outputs1"], err_msg="outputs1 step %d" % s, **TOL)
        np.testing.assert_allclose(preds, fx[p + "32/preds"], err_msg="preds step %d" % s, **TOL)
        np.testing.assert_allclose(model.embed_full(graph, nodes=fx[p + "batch"]), emb, rtol=0, atol=0)


def test_embed_full_equals_the_reference_run_unsupervised(dev):
    fx = Fixture("full_unsup_mean")
    e, model = build_unsupervised(fx)
    graph = FullGraph.from_padded(fx["graph/adj_train"])
    for s, prefix in legs(fx):
        load_weights(model, fx, prefix, supervised=False)
        p = "s%d/" % s
        for key, ids in (("outputs1", "batch1"), ("outputs2", "batch2"), ("neg_outputs", "neg_samples")):
            np.testing.assert_allclose(model.embed_full(graph, nodes=fx[p + ids]), fx[p + "32/" + key],
                                       err_msg="%s step %d" % (key, s), **TOL)


@pytest.mark.parametrize("name", SUP + ["sup_mean_3layer"])
def test_true_graph_equals_the_oracle(dev, name):
    """FullGraph.from_csr on the fixture's whole graph (it has degree-0 nodes), every node at once, trained weights; the
    3-layer mean model (--samples_3) against the oracle only."""
    fx = Fixture(name)
    c = fx.cfg
    e, ph, adj_info, sampler, model = build_supervised(fx)
    prefix = "s0/32/after/" if fx.has("s0/32/after/node_pred/bias") else "init/"
    load_weights(model, fx, prefix)
    rp, col, N = fx["graph/full_rowptr"], fx["graph/full_col"], fx.n_nodes
    assert (np.diff(rp) == 0).any()
    emb, preds = model.predict_full(FullGraph.from_csr(rp, col, N))
    assert emb.shape[0] == N and preds.shape == (N, fx["graph/labels"].shape[1])
    params = fx.params(prefix, np.float64)
    want = fo.forward(fo.csr_lists(rp, col, N), fx["graph/feats"].astype(np.float64), params, fx.agg, c["concat"])[:N]
    np.testing.assert_allclose(emb, want, **TOL)
    np.testing.assert_allclose(preds, fo.predict(want, params, c["sigmoid"])[1], **TOL)
    assert len(model.aggregators) == (3 if name == "sup_mean_3layer" else 2)


def test_device_resident_csr_and_small_windows(dev, monkeypatch):
    """from_csr on device tensors (the RMAT path) builds the same graph, and row windows of 16 give the same bits as one window."""
    import torch
    from graphsage_amd import inference as inf
    fx = Fixture("full_maxpool")
    e, ph, adj_info, sampler, model = build_supervised(fx)
    load_weights(model, fx, "s0/32/after/")
    rp, col, N = fx["graph/full_rowptr"], fx["graph/full_col"], fx.n_nodes
    host = FullGraph.from_csr(rp, col, N)
    devg = FullGraph.from_csr(torch.from_numpy(rp.astype(np.int64)).to(dev), torch.from_numpy(col.astype(np.int32)).to(dev), N)
    assert [list(x) for x in devg.lists()] == [list(x) for x in host.lists()]
    one = model.predict_full(host)
    monkeypatch.setattr(inf, "WINDOW_ROWS", 16)
    many = model.predict_full(devg)
    assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1])


def test_seq_model_refuses(dev):
    from graphsage_amd._lib import GraphsageAmdError
    fx = Fixture("sup_seq")
    e, ph, adj_info, sampler, model = build_supervised(fx)
    with pytest.raises(GraphsageAmdError, match="full-neighborhood"):
        model.predict_full(FullGraph.from_padded(fx["graph/adj_train"]))


# ------------------------------------------------------------------------------------------------ drivers
COMMON = ["--synthetic", "small", "--epochs", "1", "--batch_size", "128", "--samples_1", "5", "--samples_2", "3", "--dim_1", "32",
          "--dim_2", "32", "--max_total_steps", "6"]


def files_under(path):
    return {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(path)) for f in fs}


@pytest.mark.parametrize("extra", [["--model", "graphsage_mean"], ["--model", "graphsage_maxpool", "--sampler", "padded",
                                                                   "--max_degree", "16"]])
def test_supervised_driver_full_inference(dev, tmp_path, capsys, extra):
    from graphsage_amd import supervised_train as st
    eng.reset_engine()
    st.main(COMMON + ["--validate_iter", "10", "--print_every", "5", "--base_log_dir", str(tmp_path / "on"),
                      "--full_inference"] + extra)
    out = capsys.readouterr().out
    assert re.search(r"Full-neighborhood validation stats: f1_micro= \d\.\d{5} f1_macro= \d\.\d{5} time= \d+\.\d{5}", out)
    files = files_under(tmp_path / "on")
    assert re.match(r"f1_micro=\d\.\d{5} f1_macro=\d\.\d{5} time=\d+\.\d{5}$", open(files["val_stats_full.txt"]).read())
    assert re.match(r"f1_micro=\d\.\d{5} f1_macro=\d\.\d{5}$", open(files["test_stats_full.txt"]).read())
    assert "val_stats.txt" in files and "test_stats.txt" in files


def test_supervised_driver_without_the_flag_writes_none_of_it(dev, tmp_path, capsys):
    from graphsage_amd import supervised_train as st
    eng.reset_engine()
    st.main(COMMON + ["--validate_iter", "10", "--print_every", "5", "--base_log_dir", str(tmp_path)])
    assert "Full-neighborhood" not in capsys.readouterr().out
    files = files_under(tmp_path)
    assert "val_stats.txt" in files and not any(f.endswith("_full.txt") or f.endswith("_full.npy") for f in files)


def test_unsupervised_driver_full_inference(dev, tmp_path, capsys, monkeypatch):
    from graphsage_amd import unsupervised_train as ut
    kept = {}
    real = ut.save_full_embeddings

    def spy(model, minibatch, out_dir):
        real(model, minibatch, out_dir)
        from graphsage_amd.supervised_train import full_graph
        kept["direct"] = model.embed_full(full_graph(minibatch, minibatch.G.n_nodes))
        kept["n"] = minibatch.G.n_nodes

    monkeypatch.setattr(ut, "save_full_embeddings", spy)
    eng.reset_engine()
    args = COMMON + ["--model", "graphsage_mean", "--learning_rate", "0.001", "--max_walk_pairs", "4000", "--validate_iter", "10",
                     "--validate_batch_size", "256"]
    ut.main(args + ["--base_log_dir", str(tmp_path / "on"), "--full_inference"])
    files = files_under(tmp_path / "on")
    emb = np.load(files["val_full.npy"])
    N = kept["n"]
    assert emb.shape == (N, 64) and emb.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1.0, rtol=1e-5)
    assert np.array_equal(emb, kept["direct"])                         # the rows of a direct embed_full call
    assert open(files["val_full.txt"]).read().split("\n") == [str(i) for i in range(N)]
    assert "val.npy" in files and "val.txt" in files
    monkeypatch.setattr(ut, "save_full_embeddings", real)
    eng.reset_engine()
    ut.main(args + ["--base_log_dir", str(tmp_path / "off")])
    off = files_under(tmp_path / "off")
    assert "val.npy" in off and "val_full.npy" not in off and "val_full.txt" not in off
