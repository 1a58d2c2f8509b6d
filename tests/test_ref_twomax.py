"""CPU suite of the two-layer max-pooling aggregator (graphsage_twomaxpool): the reference's own TwoMaxLayerPoolingAggregator
(tests/golden/ref_*twomaxpool*.npz, made by tests/golden/make_ref_twomax_fixtures.py on the TF1 stand-in) == the independent
NumPy restatement with a hand-written backward (tests/twomax_oracle.py): float64 twin at 1e-9, float32 at 1e-4 -- loss,
predictions, embeddings, every gradient (the large ones as sketches: row sums, column sums, fixed entries), parameters after
clip + Adam, evaluation on the test adjacency, the unsupervised objective, and full-neighborhood inference.

The mlp2_weights arrays the fixture holds after a step only as sketches (the float64 twin's, the big case's) are carried forward
by the oracle's own clip + Adam on the gradients just checked (`carry`), which is compared with the sketch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fullnbr_oracle as fo
import twomax_oracle as tmo
from oracle import graphsage_oracle as orc
from twomax_oracle import Fixture
from test_ref_seq import DT, _items, _set, close, close_var

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GRAPHSAGE_REFERENCE", "/root/reference")
SUP = ["sup_twomaxpool", "sup_twomaxpool_big_sigmoid"]
UNSUP = ["unsup_twomaxpool"]
FULL = ["full_twomaxpool"]
AGG = "twomaxpool"
TIE_WIDTH = 1e-5          # the near-tie width of orc.argmax_ties_from


def zeros_like_params(params):
    return {k: np.zeros_like(a) for k, a in _items(params)}


def carry(fx, p, prec, params, grads, m, v, t, supervised=True):
    """Parameters of the next step: the reference's post-Adam values where the fixture holds them in full, the oracle's clip +
    TF Adam on this step's (checked) gradients for the rest."""
    gd = dict(_items(grads if supervised else {"agg": grads}))
    nxt = {"agg": [dict() for _ in params["agg"]]}
    if supervised:
        nxt["node_pred"] = {}
    for k, w in _items(params):
        w = w.copy()
        orc.adam_tf_update(w, orc.clip_by_value(gd[k]).reshape(w.shape), m[k], v[k], t, fx.cfg["learning_rate"])
        key = p + prec + "/after/" + k
        if prec == "64" and fx.has(key + "#pick"):      # (float32: Adam's knee amplifies rounding differences of tiny gradients)
            close_var(fx, key, w, prec, "after/" + k)
        _set(nxt, k, fx[key].astype(DT[prec]).reshape(w.shape) if fx.has(key) else w)
    return nxt


def sup_steps(fx, prec, weight_decay=None):
    """(step prefix, parameters before the step, oracle result, samples, parameters after) for every training step."""
    dt, c = DT[prec], fx.cfg
    ns, K = c["num_samples"], fx.K
    feats, adj = fx["graph/feats"].astype(dt), fx["graph/adj_train"]
    params = tmo.fixture_params(fx, "init/", dt)
    m, v = zeros_like_params(params), zeros_like_params(params)
    for s in range(fx.n_steps):
        p = "s%d/" % s
        batch, labels = fx[p + "batch"], fx[p + "labels"].astype(dt)
        samples, support = orc.sample(adj, batch, ns, fx.perms(p, K))
        for k in range(K):
            assert np.array_equal(samples[k + 1], fx[p + "sampled%d" % k].reshape(-1)), (s, k)
        with tmo.installed(), tmo.tracing() as tr:
            res = orc.supervised_fwd_bwd(params, feats, samples, support, labels, fx.dims, ns, len(batch), AGG, c["concat"],
                                         c["sigmoid"], weight_decay=c["weight_decay"] if weight_decay is None else weight_decay)
        res["trace"] = list(tr)
        nxt = carry(fx, p, prec, params, res["grads"], m, v, s + 1)
        yield p, params, res, samples, nxt
        params = nxt


def unsup_steps(fx, prec):
    dt, c = DT[prec], fx.cfg
    ns, K, n_neg = c["num_samples"], fx.K, c["neg_sample_size"]
    feats, adj = fx["graph/feats"].astype(dt), fx["graph/adj_train"]
    params = tmo.fixture_params(fx, "init/", dt, supervised=False)
    m, v = zeros_like_params(params), zeros_like_params(params)
    for s in range(fx.n_steps):
        p = "s%d/" % s
        roots = [fx[p + "batch1"], fx[p + "batch2"], fx[p + "neg_samples"]]
        B = len(roots[0])
        per_group = []
        for gi, r in enumerate(roots):
            smp, support = orc.sample(adj, r, ns, [fx[p + "perm%d" % (gi * K + k)] for k in range(K)])
            for k in range(K):
                assert np.array_equal(smp[k + 1], fx[p + "sampled%d" % (gi * K + k)].reshape(-1)), (s, gi, k)
            per_group.append(smp)
        samples = [np.concatenate([g[h] for g in per_group]) for h in range(K + 1)]
        with tmo.installed(), tmo.tracing() as tr:
            res = orc.unsupervised_fwd_bwd(params["agg"], feats, samples, support, fx.dims, ns, B, n_neg, AGG, c["concat"],
                                           weight_decay=c["weight_decay"])
        res["trace"] = list(tr)
        nxt = carry(fx, p, prec, params, res["grads"], m, v, s + 1, supervised=False)
        yield p, params, res, samples, nxt
        params = nxt


def margins(trace, samples, K):
    """tie_margins of every aggregator call of one forward pass (call order: layer 0's hops 0 .. K-1, layer 1's hops ..)."""
    out, t = [], 0
    for layer in range(K):
        for hop in range(K - layer):
            h2, arg = trace[t]
            t += 1
            out.append(tmo.tie_margins(h2, arg, np.asarray(samples[hop + 1]).reshape(h2.shape[0], h2.shape[1])))
    assert t == len(trace)
    return np.concatenate(out)


@pytest.mark.parametrize("prec", ["32", "64"])
@pytest.mark.parametrize("name", SUP + FULL)
def test_supervised_steps_equal_reference_run(name, prec):
    fx = Fixture(name)
    assert fx.agg == AGG
    c = fx.cfg
    for s, (p, params, res, samples, nxt) in enumerate(sup_steps(fx, prec)):
        for key in ("loss", "preds", "outputs1", "node_preds"):
            close(res[key], fx[p + prec + "/" + key], prec, key)
        if name in FULL and not any("/grad/" in k for k in fx.z.files if k.startswith(p)):
            continue                                      # the inference fixture keeps no gradients
        names = []
        for k, g in _items(res["grads"]):
            close_var(fx, p + prec + "/grad/" + k, g, prec, "grad/" + k)
            names.append(k)
        assert {"agg%d/%s" % (i, k) for i in range(fx.K) for k in tmo.MLP_KEYS} <= set(names)
        m, v = zeros_like_params(params), zeros_like_params(params)
        for k, w in _items(params):                      # clip + Adam on the reference's own gradients (where held in full)
            if fx.has(p + prec + "/grad/" + k) and s == 0:
                w = w.copy()
                orc.adam_tf_update(w, orc.clip_by_value(fx[p + prec + "/grad/" + k].astype(DT[prec])).reshape(w.shape), m[k],
                                   v[k], 1, c["learning_rate"])
                if fx.has(p + prec + "/after/" + k) or fx.has(p + prec + "/after/" + k + "#pick"):
                    close_var(fx, p + prec + "/after/" + k, w, prec, "after/" + k)
    assert fx.n_steps >= 1


def test_widths_and_the_full_float32_gradients():
    fx = Fixture("sup_twomaxpool")
    p = tmo.fixture_params(fx, "init/", np.float32)["agg"]
    assert p[0]["mlp_weights"].shape == (fx.dims[0], 512) and p[0]["mlp2_weights"].shape == (512, 256)
    assert p[1]["mlp_weights"].shape == (2 * fx.dims[1], 512) and p[0]["neigh_weights"].shape == (256, fx.dims[1])
    assert fx["s0/32/grad/agg0/mlp2_weights"].shape == (512, 256) and fx["s0/32/grad/agg0/mlp2_weights"].dtype == np.float32
    big = Fixture("sup_twomaxpool_big_sigmoid")
    assert big.cfg["model_size"] == "big"
    q = tmo.fixture_params(big, "init/", np.float32)["agg"]
    assert q[0]["mlp_weights"].shape == (big.dims[0], 1024) and q[1]["mlp2_weights"].shape == (1024, 512)
    assert q[0]["neigh_weights"].shape == (512, big.dims[1])


@pytest.mark.parametrize("name", SUP + UNSUP + FULL)
def test_no_near_tie_between_different_nodes(name):
    """TF's reduce_max gradient splits among tied maxima, the device gives it to the first; duplicated neighbor ids give the
    same weight gradients either way, a near tie between DIFFERENT ids decided by rounding would not.  In the float64 run of
    every step and both layers, every positive maximum leads the best row of a different node id by more than 1e-5."""
    fx = Fixture(name)
    steps = unsup_steps(fx, "64") if name in UNSUP else sup_steps(fx, "64")
    n_checked = 0
    for p, params, res, samples, nxt in steps:
        mg = margins(res["trace"], samples, fx.K)
        n_checked += mg.size
        assert mg.min() > TIE_WIDTH, (name, p, float(mg.min()))
    assert n_checked > 1000


def test_mlp_layers_take_no_weight_decay():
    """weight_decay > 0: the gradients of the reference's loss w.r.t. both Dense layers' variables carry no decay term, those
    of aggregator.vars do (aggregators.py:303-325; supervised_models.py:104-106)."""
    for name in SUP:
        fx = Fixture(name)
        wd = fx.cfg["weight_decay"]
        assert wd > 0
        p, params, res, samples, nxt = next(sup_steps(fx, "64", weight_decay=0.0))
        for i in range(fx.K):
            g, w = res["grads"]["agg"][i], params["agg"][i]
            for k in ("self_weights", "neigh_weights"):
                assert np.abs(w[k]).max() > 0
                close_var(fx, "s0/64/grad/agg%d/%s" % (i, k), g[k] + wd * w[k], "64", k + " with decay")
            for k in tmo.MLP_KEYS:
                close_var(fx, "s0/64/grad/agg%d/%s" % (i, k), g[k], "64", k + " without decay")
            assert np.abs(w["mlp_weights"]).max() > 0 and np.abs(w["mlp2_weights"]).max() > 0


def test_evaluation_on_the_test_adjacency_equals_reference():
    fx, dt = Fixture("sup_twomaxpool"), np.float64
    c = fx.cfg
    for p, params, res, samples, nxt in sup_steps(fx, "64"):
        pass
    batch, labels = fx["eval/batch"], fx["eval/labels"].astype(dt)
    samples, support = orc.sample(fx["graph/adj_test"], batch, c["num_samples"], fx.perms("eval/", fx.K))
    for k in range(fx.K):
        assert np.array_equal(samples[k + 1], fx["eval/sampled%d" % k].reshape(-1))
    with tmo.installed():
        res = orc.supervised_fwd_bwd(nxt, fx["graph/feats"].astype(dt), samples, support, labels, fx.dims, c["num_samples"],
                                     len(batch), AGG, c["concat"], c["sigmoid"], weight_decay=c["weight_decay"], want_grads=False)
    close(res["loss"], fx["eval/64/loss"], "64")
    close(res["preds"], fx["eval/64/preds"], "64")


@pytest.mark.parametrize("prec", ["32", "64"])
@pytest.mark.parametrize("name", UNSUP)
def test_unsupervised_steps_equal_reference_run(name, prec):
    fx = Fixture(name)
    for p, params, res, samples, nxt in unsup_steps(fx, prec):
        B = len(fx[p + "batch1"])
        close(res["loss"], fx[p + prec + "/loss"], prec, "loss")
        close(res["mrr"], fx[p + prec + "/mrr"], prec, "mrr")
        close(res["aff_all"], fx[p + prec + "/aff_all"], prec, "aff_all")
        close(res["outputs_all"][:B], fx[p + prec + "/outputs1"], prec)
        close(res["outputs_all"][B:2 * B], fx[p + prec + "/outputs2"], prec)
        close(res["outputs_all"][2 * B:], fx[p + prec + "/neg_outputs"], prec)
        for k, g in _items({"agg": res["grads"]}):
            close_var(fx, p + prec + "/grad/" + k, g, prec, "grad/" + k)
    assert fx.n_steps >= 2


@pytest.mark.parametrize("prec", ["32", "64"])
def test_full_neighborhood_pass_equals_reference_under_trained_weights(prec):
    """num_samples == [max_degree] * 2: the reference's forward pass IS the full-neighborhood pass over its padded table; step 1
    runs under the weights step 0 trained (the Dense biases are no longer zero: the pad row's hidden state is not zero)."""
    fx = Fixture("full_twomaxpool")
    c = fx.cfg
    assert c["num_samples"] == [c["max_degree"]] * fx.K and fx.n_steps >= 2
    lists = fo.padded_lists(fx["graph/adj_train"])
    feats = fx["graph/feats"].astype(DT[prec])
    for p, params, res, samples, nxt in sup_steps(fx, prec):
        emb = tmo.full_forward(lists, feats, params, c["concat"])
        batch = fx[p + "batch"]
        close(emb[batch], fx[p + prec + "/outputs1"], prec, p + "outputs1")
        node_preds, preds = fo.predict(emb[batch], params, c["sigmoid"])
        close(node_preds, fx[p + prec + "/node_preds"], prec, p + "node_preds")
        close(preds, fx[p + prec + "/preds"], prec, p + "preds")
        if p == "s1/":
            assert all(np.abs(q["mlp_bias"]).max() > 0 and np.abs(q["mlp2_bias"]).max() > 0 for q in params["agg"])


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "graphsage")), reason="the reference's sources are not on this machine")
def test_generator_reproduces_the_committed_fixtures(tmp_path):
    env = dict(os.environ, REF_FIXTURE_DIR=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(HERE, "golden", "make_ref_twomax_fixtures.py")], env=env,
                          stdout=subprocess.DEVNULL)
    import glob
    for name in SUP + UNSUP + FULL:
        parts = sorted(os.path.basename(f) for f in glob.glob(os.path.join(HERE, "golden", "ref_%s*.npz" % name))
                       if re.match(r"ref_%s(_p\d+)?\.npz$" % name, os.path.basename(f)))
        made = sorted(f for f in os.listdir(str(tmp_path)) if re.match(r"ref_%s(_p\d+)?\.npz$" % name, f))
        assert parts == made and len(parts) == int(np.load(os.path.join(HERE, "golden", "ref_%s.npz" % name))["n_parts"])
        for f in parts:
            assert os.path.getsize(os.path.join(HERE, "golden", f)) <= 1 << 20, f          # the limit for a committed file
            a, b = np.load(os.path.join(HERE, "golden", f)), np.load(os.path.join(str(tmp_path), f))
            assert sorted(a.files) == sorted(b.files), f
            for k in a.files:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (f, k)
