"""CPU suite of the LSTM aggregator (graphsage_seq): the reference's own SeqAggregator (tests/golden/ref_*seq*.npz, made by
tests/golden/make_ref_seq_fixtures.py on the TF1 stand-in + tests/tf1_rnn.py) == the independent NumPy restatement with a
hand-written BPTT (tests/seq_oracle.py): float64 twin at 1e-9 -- loss, predictions, embeddings, every gradient (the LSTM
kernel's as sketches: row sums, column sums, fixed entries), parameters after clip + Adam."""
import os
import subprocess
import sys

import numpy as np
import pytest

import seq_oracle as so
from oracle import graphsage_oracle as orc
from ref_fixtures import Fixture, flat_items

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GRAPHSAGE_REFERENCE", "/root/reference")
SEQ_SUP = ["sup_seq", "sup_seq_big_sigmoid"]
SEQ_UNSUP = ["unsup_seq"]
TOL = {"32": dict(rtol=1e-4, atol=2e-6), "64": dict(rtol=1e-9, atol=1e-12)}
DT = {"32": np.float32, "64": np.float64}


def close(got, want, prec, msg=""):
    want = np.asarray(want)
    scale = max(1.0, float(np.abs(want).max())) if want.size else 1.0
    np.testing.assert_allclose(np.asarray(got).reshape(want.shape), want, rtol=TOL[prec]["rtol"],
                               atol=TOL[prec]["atol"] * scale, err_msg=msg)


def close_var(fx, key, got, prec, msg):
    """A full array, or the sketch the fixture holds in its place."""
    if fx.has(key):
        close(got, fx[key], prec, msg)
        return
    for part, v in so.sketch(np.asarray(got)).items():
        want = fx["%s#%s" % (key, part)]
        if prec == "32" and part != "pick":
            # a float32 sum of a few hundred gradient entries cancels: its rounding scales with the largest sum, not with 1
            np.testing.assert_allclose(v, want, rtol=1e-4, atol=1e-4 * max(1e-2, float(np.abs(want).max())),
                                       err_msg="%s#%s" % (msg, part))
        else:
            close(v, want, prec, "%s#%s" % (msg, part))


def _items(params):
    items = []
    for i, p in enumerate(params["agg"]):
        for k in sorted(p):
            items.append(("agg%d/%s" % (i, k), p[k]))
    if "node_pred" in params:
        items += [("node_pred/weights", params["node_pred"]["weights"]), ("node_pred/bias", params["node_pred"]["bias"])]
    return items


def _set(params, name, value):
    if name.startswith("agg"):
        i, k = name.split("/", 1)
        params["agg"][int(i[3:])][k] = value
    else:
        params["node_pred"][name.split("/", 1)[1]] = value


def _step_params(fx, p, prec, params, grads, m, v, t, supervised=True):
    """Parameters of the next step: the reference's post-Adam values where the fixture holds them in full; for the LSTM kernels
    (sketched in the fixture) clip + TF Adam on this step's gradients, checked against the sketch of the reference's values."""
    dt = DT[prec]
    nxt = so.fixture_params(fx, p + prec + "/after/", dt, supervised)
    gd = dict(_items(grads if supervised else {"agg": grads}))
    for k, w in _items(params):
        if not k.endswith("lstm_kernel"):
            continue
        w = w.copy()
        orc.adam_tf_update(w, orc.clip_by_value(gd[k]), m[k], v[k], t, fx.cfg["learning_rate"])
        if prec == "64":         # (float32: Adam's knee amplifies rounding differences of tiny gradients, see test_ref_pin_gpu)
            close_var(fx, p + prec + "/after/" + k, w, prec, "after/" + k)
        _set(nxt, k, w)
    return nxt


@pytest.mark.parametrize("prec", ["32", "64"])
@pytest.mark.parametrize("name", SEQ_SUP)
def test_supervised_seq_steps_equal_reference_run(name, prec):
    fx, dt = Fixture(name), DT[prec]
    c = fx.cfg
    ns, K = c["num_samples"], fx.K
    feats, adj = fx["graph/feats"].astype(dt), fx["graph/adj_train"]
    params = so.fixture_params(fx, "init/", dt)
    m = {k: np.zeros_like(a) for k, a in _items(params)}
    v = {k: np.zeros_like(a) for k, a in _items(params)}
    for s in range(fx.n_steps):
        p = "s%d/" % s
        batch, labels = fx[p + "batch"], fx[p + "labels"].astype(dt)
        samples, support = orc.sample(adj, batch, ns, fx.perms(p, K))
        for k in range(K):
            assert np.array_equal(samples[k + 1], fx[p + "sampled%d" % k].reshape(-1)), (s, k)
        with so.installed():
            res = orc.supervised_fwd_bwd(params, feats, samples, support, labels, fx.dims, ns, len(batch), "seq", c["concat"],
                                         c["sigmoid"], weight_decay=c["weight_decay"])
        for key in ("loss", "preds", "outputs1", "node_preds"):
            close(res[key], fx[p + prec + "/" + key], prec, key)
        names = []
        for k, g in _items(res["grads"]):
            close_var(fx, p + prec + "/grad/" + k, g, prec, "grad/" + k)
            names.append(k)
        assert {"agg0/lstm_kernel", "agg0/lstm_bias", "agg1/lstm_kernel", "agg1/lstm_bias"} <= set(names)
        for k, w in _items(params):                      # clip + Adam on the reference's gradients (full arrays)
            if fx.has(p + prec + "/grad/" + k):
                w = w.copy()
                orc.adam_tf_update(w, orc.clip_by_value(fx[p + prec + "/grad/" + k].astype(dt)).reshape(w.shape), m[k], v[k],
                                   s + 1, c["learning_rate"])
                close(w, fx[p + prec + "/after/" + k], prec, "after/" + k)
        params = _step_params(fx, p, prec, params, res["grads"], m, v, s + 1)
    assert fx.n_steps >= 1


def test_lstm_variables_take_no_weight_decay():
    """sup_seq_big_sigmoid has weight_decay > 0: the gradient of the reference's loss w.r.t. the LSTM bias (zero-initialised)
    has no decay term, those of aggregator.vars have one (aggregators.py:386-399; supervised_models.py:104-106)."""
    fx = Fixture("sup_seq_big_sigmoid")
    assert fx.cfg["weight_decay"] > 0 and fx.cfg["model_size"] == "big"
    params = so.fixture_params(fx, "init/", np.float64)
    assert params["agg"][0]["lstm_kernel"].shape == (fx.dims[0] + 256, 1024)
    c = fx.cfg
    samples, support = orc.sample(fx["graph/adj_train"], fx["s0/batch"], c["num_samples"], fx.perms("s0/", fx.K))
    with so.installed():
        res = orc.supervised_fwd_bwd(params, fx["graph/feats"].astype(np.float64), samples, support,
                                     fx["s0/labels"].astype(np.float64), fx.dims, c["num_samples"], len(fx["s0/batch"]), "seq",
                                     c["concat"], c["sigmoid"], weight_decay=0.0)
    g0 = res["grads"]["agg"][0]
    wd = c["weight_decay"]
    close(g0["self_weights"] + wd * params["agg"][0]["self_weights"], fx["s0/64/grad/agg0/self_weights"], "64")
    close_var(fx, "s0/64/grad/agg0/lstm_kernel", g0["lstm_kernel"], "64", "lstm_kernel without decay")


def test_evaluation_on_the_test_adjacency_equals_reference():
    fx, dt = Fixture("sup_seq"), np.float64
    c = fx.cfg
    last = fx.n_steps - 1
    params = so.fixture_params(fx, "s%d/64/after/" % last, dt)
    # the LSTM kernels after the last step: replay the run's Adam on the oracle's gradients
    p0 = so.fixture_params(fx, "init/", dt)
    m = {k: np.zeros_like(a) for k, a in _items(p0)}
    v = {k: np.zeros_like(a) for k, a in _items(p0)}
    for s in range(fx.n_steps):
        p = "s%d/" % s
        samples, support = orc.sample(fx["graph/adj_train"], fx[p + "batch"], c["num_samples"], fx.perms(p, fx.K))
        with so.installed():
            res = orc.supervised_fwd_bwd(p0, fx["graph/feats"].astype(dt), samples, support, fx[p + "labels"].astype(dt),
                                         fx.dims, c["num_samples"], len(fx[p + "batch"]), "seq", c["concat"], c["sigmoid"],
                                         weight_decay=c["weight_decay"])
        p0 = _step_params(fx, p, "64", p0, res["grads"], m, v, s + 1)
    for i in range(fx.K):
        params["agg"][i]["lstm_kernel"] = p0["agg"][i]["lstm_kernel"]
    batch, labels = fx["eval/batch"], fx["eval/labels"].astype(dt)
    samples, support = orc.sample(fx["graph/adj_test"], batch, c["num_samples"], fx.perms("eval/", fx.K))
    with so.installed():
        res = orc.supervised_fwd_bwd(params, fx["graph/feats"].astype(dt), samples, support, labels, fx.dims,
                                     c["num_samples"], len(batch), "seq", c["concat"], c["sigmoid"],
                                     weight_decay=c["weight_decay"], want_grads=False)
    close(res["loss"], fx["eval/64/loss"], "64")
    close(res["preds"], fx["eval/64/preds"], "64")


@pytest.mark.parametrize("prec", ["32", "64"])
@pytest.mark.parametrize("name", SEQ_UNSUP)
def test_unsupervised_seq_steps_equal_reference_run(name, prec):
    fx, dt = Fixture(name), DT[prec]
    c = fx.cfg
    ns, K, n_neg = c["num_samples"], fx.K, c["neg_sample_size"]
    feats, adj = fx["graph/feats"].astype(dt), fx["graph/adj_train"]
    params = so.fixture_params(fx, "init/", dt, supervised=False)
    m = {k: np.zeros_like(a) for k, a in _items(params)}
    v = {k: np.zeros_like(a) for k, a in _items(params)}
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
        with so.installed():
            res = orc.unsupervised_fwd_bwd(params["agg"], feats, samples, support, fx.dims, ns, B, n_neg, "seq", c["concat"],
                                           weight_decay=c["weight_decay"])
        close(res["loss"], fx[p + prec + "/loss"], prec, "loss")
        close(res["mrr"], fx[p + prec + "/mrr"], prec, "mrr")
        close(res["aff_all"], fx[p + prec + "/aff_all"], prec, "aff_all")
        close(res["outputs_all"][:B], fx[p + prec + "/outputs1"], prec)
        close(res["outputs_all"][B:2 * B], fx[p + prec + "/outputs2"], prec)
        close(res["outputs_all"][2 * B:], fx[p + prec + "/neg_outputs"], prec)
        for k, g in _items({"agg": res["grads"]}):
            close_var(fx, p + prec + "/grad/" + k, g, prec, "grad/" + k)
        params = _step_params(fx, p, prec, params, res["grads"], m, v, s + 1, supervised=False)
    assert fx.n_steps >= 2


def test_length_rule_interior_zero_row():
    """L = max(1, number of non-zero rows): a zero row INSIDE the first L steps still runs, and the steps dropped are the
    LAST ones (aggregators.py:411-414 with dynamic_rnn's sequence_length); an all-zero sequence runs one step."""
    rng = np.random.RandomState(3)
    D, H, T = 5, 128, 4
    x = rng.randn(3, T, D)
    x[0, 1] = 0.0                # interior zero row: L = 3, steps 0, 1 (zero input), 2 run; step 3 (non-zero) is dropped
    x[1] = 0.0                   # degree-0 node (pad rows only): L = 1
    assert so.lengths(x).tolist() == [3, 1, 4]
    kernel = rng.uniform(-0.1, 0.1, (D + H, 4 * H))
    bias = rng.uniform(-0.1, 0.1, 4 * H)

    def plain(seq):              # the cell over exactly these rows, no masking
        h, c = np.zeros(H), np.zeros(H)
        for xt in seq:
            z = xt @ kernel[:D] + h @ kernel[D:] + bias
            s = lambda a: 1 / (1 + np.exp(-a))
            c = c * s(z[2 * H:3 * H] + 1.0) + s(z[:H]) * np.tanh(z[H:2 * H])
            h = np.tanh(c) * s(z[3 * H:])
        return h
    h_last, _ = so.lstm_fwd(x, so.lengths(x), kernel, bias)
    np.testing.assert_allclose(h_last[0], plain(x[0, :3]), rtol=1e-12, atol=1e-14)
    assert not np.allclose(h_last[0], plain(x[0, [0, 2, 3]]))          # not "skip the zero row"
    np.testing.assert_allclose(h_last[1], plain(x[1, :1]), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(h_last[2], plain(x[2]), rtol=1e-12, atol=1e-14)


def test_fixtures_hold_interior_zero_rows_and_degree_zero_nodes():
    """The fixture graph's two zeroed feature rows appear inside the first L steps of sampled sequences, and degree-0 nodes
    sample only the pad row (L = 1)."""
    fx = Fixture("sup_seq")
    feats = fx["graph/feats"]
    zero = ~np.abs(feats).max(axis=1).astype(bool)
    assert zero[-1] and zero[:-1].sum() == 2
    ns = fx.cfg["num_samples"]
    x = zero[fx["s0/sampled0"].reshape(-1, ns[1])]            # hop-0 neighbor sequences of layer 0 (T = num_samples[1])
    y = zero[fx["s0/sampled1"].reshape(-1, ns[0])]            # hop-1 neighbor sequences (T = num_samples[0])
    interior = False
    for seqs in (x, y):
        L = np.maximum((~seqs).sum(axis=1), 1)
        interior |= any(seqs[r, :L[r]].any() and not seqs[r].all() for r in range(len(seqs)))
    assert interior
    assert any(seqs.all() for seqs in y)                     # an all-pad sequence (degree-0 or val/test node)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "graphsage")), reason="the reference's sources are not on this machine")
def test_generator_reproduces_the_committed_fixtures(tmp_path):
    env = dict(os.environ, REF_FIXTURE_DIR=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(HERE, "golden", "make_ref_seq_fixtures.py")], env=env,
                          stdout=subprocess.DEVNULL)
    for name in SEQ_SUP + SEQ_UNSUP:
        a = np.load(os.path.join(HERE, "golden", "ref_%s.npz" % name))
        b = np.load(os.path.join(str(tmp_path), "ref_%s.npz" % name))
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)
