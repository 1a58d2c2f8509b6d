"""-m gpu: the two-layer max-pooling aggregator (graphsage_twomaxpool) on the device.

  * every step of the reference's own runs (tests/golden/ref_{sup_twomaxpool,sup_twomaxpool_big_sigmoid,unsup_twomaxpool}*.npz)
    within the tolerances of test_ref_pin_gpu: sampled ids bit-exact; loss, predictions, embeddings, every gradient and the
    parameters after clip + Adam (its Adam-knee selection) by its `close` rule, sketched arrays as sketches.  Each supervised
    fixture runs with dH1 from gs_pool2_dgrad, from the three-launch composition, and with layer 0 on the step's distinct ids
    (both split-MFMA forms; the h_idx form of the kernel);
  * evaluation on the test adjacency, forward only;
  * ref_full_twomaxpool: embed_full / predict_full over FullGraph.from_padded == the reference's numbers, under the initial
    weights and under the reference's own trained ones;
  * a fan-out above 64 (the unfused forward, the composed backward, the dense W2 weight gradient) == tests/twomax_oracle.py;
  * identity features: one step at identity_dim = 8 on the fixture graph == tests/twomax_oracle.py on the device's own sampled
    ids, the node_embeddings gradient included;
  * both training drivers run --model graphsage_twomaxpool as fresh child processes; --dropout is refused before any step;
  * both forms of the backward give the same bits across two identical runs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import seq_oracle as so
import twomax_oracle as tmo
from graphsage_amd import engine as eng
from graphsage_amd.neigh_samplers import PaddedAdjacency
from oracle import graphsage_oracle as orc
from twomax_oracle import Fixture
from test_full_inference_gpu import TOL, build_unsupervised, files_under
from test_ref_pin_gpu import ADAM_KNEE, RTOL, build_supervised, close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUP = ["sup_twomaxpool", "sup_twomaxpool_big_sigmoid"]


class Vars(object):
    """name (fixture naming) -> engine Variable, both Dense layers of every aggregator included."""

    def __init__(self, model, supervised=True):
        self.v = {}
        for i, a in enumerate(model.aggregators):
            for k, v in a.vars.items():
                self.v["agg%d/%s" % (i, k)] = v
            for tag, layer in zip(("mlp", "mlp2"), a.mlp_layers):
                self.v["agg%d/%s_weights" % (i, tag)] = layer.vars['weights']
                self.v["agg%d/%s_bias" % (i, tag)] = layer.vars['bias']
        if supervised:
            self.v["node_pred/weights"] = model.node_pred.vars['weights']
            self.v["node_pred/bias"] = model.node_pred.vars['bias']
        self.embeds = model.embeds

    def load(self, params):
        """From the oracle's layout (twomax_oracle.fixture_params); names it does not hold keep the device's values."""
        items = [("agg%d/%s" % (i, k), a) for i, p in enumerate(params["agg"]) for k, a in p.items()]
        items += [("node_pred/" + k, a) for k, a in params.get("node_pred", {}).items()]
        for k, a in items:
            v = self.v[k]
            v.assign(np.asarray(a, np.float32).reshape(v.numpy().shape))
        eng.get_engine().sync()

    def params(self):
        out = {"agg": []}
        for k, v in self.v.items():
            head, name = k.split("/")
            a = v.numpy().copy()
            a = a.reshape(-1) if name.endswith("bias") else a
            if head == "node_pred":
                out.setdefault("node_pred", {})[name] = a
            else:
                i = int(head[3:])
                while len(out["agg"]) <= i:
                    out["agg"].append({})
                out["agg"][i][name] = a
        return out


def check_step(fx, p, vs):
    """Gradients and post-Adam parameters of one step against the reference's float32 run (full arrays or their sketches)."""
    for k, v in vs.v.items():
        gkey, akey = p + "32/grad/" + k, p + "32/after/" + k
        got_g, got_w = v.grad.numpy(), v.numpy()
        if fx.has(gkey):
            g = fx[gkey]
            close(got_g, g, "grad/" + k)
            g_pick = None
        else:
            for part, a in so.sketch(got_g).items():
                close(a, fx["%s#%s" % (gkey, part)], "grad/%s#%s" % (k, part))
            g_pick = fx[gkey + "#pick"]
        # parameters after clip + Adam, outside Adam's knee (test_ref_pin_gpu.ADAM_KNEE)
        if fx.has(akey):
            want = fx[akey]
            solid = np.abs(g) > max(1e-6 * max(1e-2, np.abs(g).max()), ADAM_KNEE)
            np.testing.assert_allclose(got_w.reshape(want.shape)[solid], want[solid], rtol=RTOL, atol=2e-5, err_msg="after/" + k)
        else:
            idx = so.sketch_index(got_w.shape)
            want = fx[akey + "#pick"]
            gp = g_pick if g_pick is not None else g.reshape(-1)[idx]
            gmax = np.abs(gp).max() if g_pick is not None else np.abs(g).max()
            solid = np.abs(gp) > max(1e-6 * max(1e-2, gmax), ADAM_KNEE)
            np.testing.assert_allclose(got_w.reshape(-1)[idx][solid], want[solid], rtol=RTOL, atol=2e-5, err_msg="after/" + k)


def continue_from_reference(fx, p, vs, supervised=True):
    """Each step is pinned by itself: the next one starts from the reference's parameters (the big case's mlp2_weights, held as
    sketches, stay the device's own)."""
    vs.load(tmo.fixture_params(fx, p + "32/after/", np.float32, supervised))


MODES = ["pool2_dgrad", "composed", "distinct_f16x2", "distinct_bf16x3"]


def prepare(e, model, mode):
    for a in model.aggregators:
        a.fuse_dgrad = mode != "composed"
    if mode.startswith("distinct"):
        # layer 0 through the step's DISTINCT sampled ids although the fixture gathers far fewer rows than the default threshold
        e.pool_f16 = mode == "distinct_f16x2"
        assert e.split_pool
        model.aggregators[0].dedup_min_rows = 0


def check_paths(model, mode):
    a0 = model.aggregators[0]
    for a in model.aggregators:
        assert a.last_dgrad_kernel == ("composed" if mode == "composed" else "pool2_dgrad"), (mode, a.last_dgrad_kernel)
    if mode.startswith("distinct"):
        assert a0.last_pool_kernel == {"distinct_f16x2": "split16", "distinct_bf16x3": "split_bf16x3"}[mode], a0.last_pool_kernel
        cnt, rows_total = a0.last_unique
        assert 0 < int(cnt.item()) <= rows_total
        assert a0.last_dgrad_indexed is True and model.aggregators[1].last_dgrad_indexed is False
    else:
        assert a0.last_unique is None and a0.last_dgrad_indexed is False


def run_supervised(name, mode, check=True):
    fx = Fixture(name)
    e, ph, adj_info, sampler, model = build_supervised(fx)
    big = fx.cfg.get("model_size") == "big"
    a0 = model.aggregators[0]
    assert (a0.hidden_dim_1, a0.hidden_dim_2) == ((1024, 512) if big else (512, 256))
    assert not any(v.decay for layer in a0.mlp_layers for v in layer.vars.values()) and a0.vars['neigh_weights'].decay
    assert a0.vars['neigh_weights'].rows == a0.hidden_dim_2
    prepare(e, model, mode)
    vs = Vars(model)
    assert all(v in e.variables for v in vs.v.values())              # ... all in the flat gradient buffer
    vs.load(tmo.fixture_params(fx, "init/", np.float32))
    for s in range(fx.n_steps):
        p = "s%d/" % s
        batch, labels = fx[p + "batch"], fx[p + "labels"]
        sampler.inject_perms(fx.perms(p, fx.K))
        loss, preds = model.train_step({ph['batch']: batch, ph['labels']: labels, ph['batch_size']: len(batch)})
        check_paths(model, mode)
        if check:
            for k in range(fx.K):
                assert np.array_equal(model.samples1[k + 1].cpu().numpy(), fx[p + "sampled%d" % k].reshape(-1)), (s, k)
            close(loss, fx[p + "32/loss"], "loss step %d" % s)
            close(preds, fx[p + "32/preds"], "preds step %d" % s)
            close(model.outputs1.numpy(), fx[p + "32/outputs1"], "outputs1 step %d" % s)
            check_step(fx, p, vs)
            continue_from_reference(fx, p, vs)
    return fx, e, ph, adj_info, sampler, model


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SUP)
def test_supervised_steps_equal_reference_run(dev, name, mode):
    fx, e, ph, adj_info, sampler, model = run_supervised(name, mode)
    if fx.has("eval/batch") and mode == "pool2_dgrad":
        # supervised_train.py:280-285: evaluation on the test adjacency after the run (tf.assign(adj_info, test_adj)); forward only
        adj_info.assign(PaddedAdjacency(fx["graph/adj_test"], e.device))
        sampler.inject_perms(fx.perms("eval/", fx.K))
        batch, labels = fx["eval/batch"], fx["eval/labels"]
        loss, preds = model.eval_step({ph['batch']: batch, ph['labels']: labels, ph['batch_size']: len(batch)})
        for k in range(fx.K):
            assert np.array_equal(model.samples1[k + 1].cpu().numpy(), fx["eval/sampled%d" % k].reshape(-1))
        close(loss, fx["eval/32/loss"], "eval loss")
        close(preds, fx["eval/32/preds"], "eval preds")


@pytest.mark.parametrize("mode", ["pool2_dgrad", "composed"])
def test_two_identical_runs_give_the_same_bits(dev, mode):
    outs = []
    for _ in range(2):
        fx, e, ph, adj_info, sampler, model = run_supervised("sup_twomaxpool", mode, check=False)
        e.sync()
        outs.append((e.params.cpu().numpy().tobytes(), e.grads.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


@pytest.mark.parametrize("fuse_dgrad", [True, False])
def test_unsupervised_steps_equal_reference_run(dev, fuse_dgrad):
    fx = Fixture("unsup_twomaxpool")
    c = fx.cfg
    K, n_neg = fx.K, c["neg_sample_size"]
    e, model = build_unsupervised(fx)
    model.use_graphs = False
    ph, sampler = model.placeholders, model.layer_infos[0].neigh_sampler
    for a in model.aggregators:
        a.fuse_dgrad = fuse_dgrad
    vs = Vars(model, supervised=False)
    vs.load(tmo.fixture_params(fx, "init/", np.float32, supervised=False))
    for s in range(fx.n_steps):
        p = "s%d/" % s
        b1, b2, neg = fx[p + "batch1"], fx[p + "batch2"], fx[p + "neg_samples"]
        B = len(b1)
        sampler.inject_perms(fx.perms(p, 3 * K))
        model.inject_negatives(neg)
        loss, ranks, aff_all, mrr, outputs1 = model.train_step({ph['batch1']: b1, ph['batch2']: b2, ph['batch_size']: B})
        assert all(a.last_dgrad_kernel == ("pool2_dgrad" if fuse_dgrad else "composed") for a in model.aggregators)
        for k in range(K):
            want = np.concatenate([fx[p + "sampled%d" % (g * K + k)].reshape(-1) for g in range(3)])
            assert np.array_equal(model.samples1[k + 1].cpu().numpy(), want), (s, k)
        close(loss, fx[p + "32/loss"], "loss step %d" % s)
        close(mrr, fx[p + "32/mrr"], "mrr step %d" % s)
        close(aff_all, fx[p + "32/aff_all"], "aff_all")
        close(outputs1, fx[p + "32/outputs1"], "outputs1")
        full = model.outputs_all.numpy()
        close(full[B:2 * B], fx[p + "32/outputs2"], "outputs2")
        close(full[2 * B:2 * B + n_neg], fx[p + "32/neg_outputs"], "neg_outputs")
        check_step(fx, p, vs)
        continue_from_reference(fx, p, vs, supervised=False)


def test_full_inference_equals_the_reference_run(dev):
    """num_samples == [max_degree] * 2: the reference's forward pass IS the full-neighborhood pass over its padded table.  Step 0
    under the initial weights, step 1 under the reference's own weights after its first Adam step (the Dense biases are no
    longer zero: the pad row's hidden state is not zero)."""
    from graphsage_amd.inference import FullGraph
    fx = Fixture("full_twomaxpool")
    e, ph, adj_info, sampler, model = build_supervised(fx)
    graph = FullGraph.from_padded(fx["graph/adj_train"])
    vs = Vars(model)
    assert fx.n_steps >= 2
    for s, prefix in ((0, "init/"), (1, "s0/32/after/")):
        params = tmo.fixture_params(fx, prefix, np.float32)
        assert all(set(tmo.MLP_KEYS) <= set(q) for q in params["agg"])
        vs.load(params)
        p = "s%d/" % s
        emb, preds = model.predict_full(graph, nodes=fx[p + "batch"])
        np.testing.assert_allclose(emb, fx[p + "32/outputs1"], err_msg="outputs1 step %d" % s, **TOL)
        np.testing.assert_allclose(preds, fx[p + "32/preds"], err_msg="preds step %d" % s, **TOL)
        np.testing.assert_allclose(model.embed_full(graph, nodes=fx[p + "batch"]), emb, rtol=0, atol=0)


@pytest.mark.parametrize("mode", ["pool2_dgrad", "distinct_bf16x3"])
def test_identity_features_match_oracle(dev, mode):
    """identity_dim = 8 on the fixture graph: trainable node_embeddings in front of the features; their gradient is the per-id
    sum of layer 0's input gradients, which for this aggregator go back through both Dense layers."""
    fx = Fixture("sup_twomaxpool")
    c, idim = fx.cfg, 8
    fx.identity_dim = idim
    fx.dims = [fx.dims[0] + idim] + fx.dims[1:]
    e, ph, adj_info, sampler, model = build_supervised(fx)
    prepare(e, model, mode)
    vs = Vars(model)
    params = vs.params()
    emb0 = model.embeds.numpy().copy()
    assert emb0.shape == (fx.n_nodes + 1, idim)
    feats = np.concatenate([emb0, fx["graph/feats"]], axis=1)
    batch, labels = fx["s0/batch"], fx["s0/labels"]
    perms = fx.perms("s0/", fx.K)
    sampler.inject_perms(perms)
    loss, preds = model.train_step({ph['batch']: batch, ph['labels']: labels, ph['batch_size']: len(batch)})
    check_paths(model, mode)
    if mode.startswith("distinct"):
        assert model.aggregators[0].last_pool_kernel == "split_bf16x3"        # the table has trainable columns: never cut once
    samples = [t.cpu().numpy() for t in model.samples1]
    want_samples, support = orc.sample(fx["graph/adj_train"], batch, c["num_samples"], perms)
    for a, b in zip(samples, want_samples):
        assert np.array_equal(a, b)
    with tmo.installed():
        res = orc.supervised_fwd_bwd(params, feats, samples, support, labels, fx.dims, c["num_samples"], len(batch), "twomaxpool",
                                     c["concat"], c["sigmoid"], weight_decay=c["weight_decay"], identity_dim=idim)
    close(loss, res["loss"], "loss")
    close(preds, res["preds"], "preds")
    for k, v in vs.v.items():
        head, name = k.split("/")
        want = res["grads"]["node_pred"][name] if head == "node_pred" else res["grads"]["agg"][int(head[3:])][name]
        close(v.grad.numpy(), want, "grad/" + k)
    w = res["grads"]["embeds"]
    assert np.count_nonzero(w) > 0
    close(model.embeds.grad.numpy(), w, "grad/node_embeddings")


@pytest.mark.parametrize("fuse_dgrad", [True, False])
def test_fan_out_above_64_matches_oracle(dev, fuse_dgrad):
    """num_samples = [65, 2]: layer 0 holds a hop of 65 samples per node, beyond what gs_dense_pool_max_fwd, gs_pool2_dgrad and
    gs_maxpool_sparse_wgrad take, so BOTH its hops run the second Dense as its own GEMM + gs_segment_max_fwd, the composed
    backward and the dense W2 weight gradient whatever fuse_dgrad says; layer 1 (s = 2) keeps the fused forms.  One step on a
    small synthetic graph against the oracle on the device's own sampled ids."""
    from graphsage_amd import inits
    from graphsage_amd.minibatch import NodeMinibatchIterator
    from graphsage_amd.models import Placeholder, SAGEInfo
    from graphsage_amd.neigh_samplers import AdjInfo, UniformNeighborSampler
    from graphsage_amd.supervised_models import SupervisedGraphsage
    from graphsage_amd.utils import synthetic_graph
    eng.reset_engine()
    inits.set_seed(7)
    G = synthetic_graph(n_nodes=300, feat_dim=20, num_classes=5, avg_degree=8, seed=5, multilabel=False)
    ph = {'labels': Placeholder('labels'), 'batch': Placeholder('batch1'), 'dropout': Placeholder('dropout', 0.),
          'batch_size': Placeholder('batch_size')}
    it = NodeMinibatchIterator(G, None, ph, None, G.num_classes, batch_size=8, max_degree=66)
    e = eng.get_engine()
    sampler = UniformNeighborSampler(AdjInfo(PaddedAdjacency(it.adj, e.device)))
    ns, wd = [65, 2], 0.01
    model = SupervisedGraphsage(G.num_classes, ph, G.padded_features(), sampler.adj_info, it.deg,
                                [SAGEInfo("node", sampler, n, 16) for n in ns], concat=True, aggregator_type="twomaxpool",
                                sigmoid_loss=False, learning_rate=0.01, weight_decay=wd)
    model.use_graphs = False
    for a in model.aggregators:
        a.fuse_dgrad = fuse_dgrad
    vs = Vars(model)
    params = vs.params()
    rng = np.random.RandomState(3)
    batch = rng.choice(it.train_nodes, size=7, replace=False).astype(np.int32)
    perms = [rng.permutation(it.max_degree) for _ in ns]
    labels = it.label_matrix[batch]
    sampler.inject_perms(perms)
    loss, preds = model.train_step({ph['batch']: batch, ph['labels']: labels, ph['batch_size']: len(batch)})
    a0, a1 = model.aggregators
    assert a0.last_dgrad_kernel == "composed" and a1.last_dgrad_kernel == ("pool2_dgrad" if fuse_dgrad else "composed")
    samples, support = orc.sample(it.adj, batch, ns, perms)
    for got, want in zip(model.samples1, samples):
        assert np.array_equal(got.cpu().numpy(), want)
    with tmo.installed():
        res = orc.supervised_fwd_bwd(params, G.padded_features(), samples, support, labels, model.dims, ns, len(batch),
                                     "twomaxpool", True, False, weight_decay=wd)
    close(loss, res["loss"], "loss")
    close(preds, res["preds"], "preds")
    close(model.outputs1.numpy(), res["outputs1"], "outputs1")
    for k, v in vs.v.items():
        head, name = k.split("/")
        want = res["grads"]["node_pred"][name] if head == "node_pred" else res["grads"]["agg"][int(head[3:])][name]
        close(v.grad.numpy(), want, "grad/" + k)


# ---------------------------------------------------------------------------------------------------------------
# drivers: fresh child processes, one epoch
# ---------------------------------------------------------------------------------------------------------------
COMMON = ["--synthetic", "small", "--epochs", "1", "--batch_size", "128", "--samples_1", "5", "--samples_2", "3", "--dim_1", "32",
          "--dim_2", "32", "--max_total_steps", "6", "--model", "graphsage_twomaxpool"]


def child(module, args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "graphsage_amd." + module] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, universal_newlines=True, timeout=600)


def test_supervised_train_driver(dev, tmp_path):
    r = child("supervised_train", COMMON + ["--validate_iter", "10", "--print_every", "2", "--base_log_dir", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    assert "Epoch: 0001" in out and "Optimization Finished!" in out and "Full validation stats:" in out
    assert re.search(r"Iter: \d{4} train_loss= \d+\.\d{5} train_f1_mic= \d\.\d{5} .* val_f1_mic= \d\.\d{5} .* time= \d+\.\d{5}", out)
    files = files_under(tmp_path)
    assert "val_stats.txt" in files and "test_stats.txt" in files
    assert "graphsage_twomaxpool_small" in files["val_stats.txt"]
    assert re.match(r"loss=\d+\.\d{5} f1_micro=\d\.\d{5} f1_macro=\d\.\d{5} time=\d+\.\d{5}", open(files["val_stats.txt"]).read())


def test_unsupervised_train_driver_with_full_inference(dev, tmp_path):
    r = child("unsupervised_train", COMMON + ["--learning_rate", "0.001", "--max_walk_pairs", "4000", "--validate_iter", "10",
                                              "--print_every", "2", "--validate_batch_size", "256", "--base_log_dir", str(tmp_path),
                                              "--full_inference"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Optimization Finished!" in r.stdout
    assert re.search(r"Iter: \d{4} train_loss= \d+\.\d{5} train_mrr= \d\.\d{5}", r.stdout)
    files = files_under(tmp_path)
    assert "val.npy" in files and "val.txt" in files and "val_full.npy" in files and "val_full.txt" in files
    assert "graphsage_twomaxpool_small" in files["val.npy"]
    emb = np.load(files["val_full.npy"])
    assert emb.shape[1] == 64 and emb.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1.0, rtol=1e-5)
    assert np.isfinite(np.load(files["val.npy"])).all()


@pytest.mark.parametrize("module", ["supervised_train", "unsupervised_train"])
def test_dropout_is_refused_before_any_step(dev, tmp_path, module):
    r = child(module, COMMON + ["--dropout", "0.1", "--base_log_dir", str(tmp_path)])
    assert r.returncode != 0
    assert "GraphsageAmdError" in r.stderr and "--dropout > 0 is not supported with --model graphsage_twomaxpool" in r.stderr
    assert "Epoch:" not in r.stdout and "Loading training data" not in r.stdout
    assert not files_under(tmp_path)


def test_model_refuses_dropout_at_the_first_step(dev):
    from graphsage_amd._lib import GraphsageAmdError
    fx = Fixture("sup_twomaxpool")
    e, ph, adj_info, sampler, model = build_supervised(fx)
    sampler.inject_perms(fx.perms("s0/", fx.K))
    batch, labels = fx["s0/batch"], fx["s0/labels"]
    with pytest.raises(GraphsageAmdError, match="dropout > 0 is not supported"):
        model.train_step({ph['batch']: batch, ph['labels']: labels, ph['batch_size']: len(batch), ph['dropout']: 0.1})
