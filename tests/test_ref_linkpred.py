"""CPU suite of the link-prediction heads (hinge / skipgram losses, bilinear affinity): the reference's own
BipartiteEdgePredLayer (tests/golden/ref_unsup_{hinge,skipgram,hinge_bilinear,xent_bilinear}.npz, made by
tests/golden/make_ref_linkpred_fixtures.py on the TF1 stand-in) == the NumPy restatement of tests/linkpred_oracle.py inside
the oracle's unsupervised step: float64 twin at 1e-9, float32 leg at 1e-4 -- loss, aff_all, ranks, embeddings, every gradient
(the bilinear matrix's among them).  Plus the host-only surface: constructor, flags, log directory, ABI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import linkpred_oracle as lo
from oracle import graphsage_oracle as orc
from ref_fixtures import Fixture, flat_items

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("GRAPHSAGE_REFERENCE", "/root/reference")
CASES = ["unsup_hinge", "unsup_skipgram", "unsup_hinge_bilinear", "unsup_xent_bilinear"]
RTOL = 1e-4
TOL = {"32": dict(rtol=RTOL, atol=2e-6), "64": dict(rtol=1e-9, atol=1e-12)}
DT = {"32": np.float32, "64": np.float64}


def close(got, want, prec, msg=""):
    want = np.asarray(want)
    scale = max(1.0, float(np.abs(want).max())) if want.size else 1.0
    np.testing.assert_allclose(np.asarray(got).reshape(want.shape), want, rtol=TOL[prec]["rtol"],
                               atol=TOL[prec]["atol"] * scale, err_msg=msg)


def step_inputs(fx, s, prec):
    """(aggregator parameters, W or None) the reference used in step s: its initial values, then its own post-Adam values."""
    prefix = "init/" if s == 0 else "s%d/%s/after/" % (s - 1, prec)
    params = fx.params(prefix, DT[prec], supervised=False)
    W = fx[prefix + "edge_predict/weights"].astype(DT[prec]) if fx.cfg["bilinear_weights"] else None
    return params, W


@pytest.mark.parametrize("prec", ["32", "64"])
@pytest.mark.parametrize("name", CASES)
def test_unsupervised_steps_equal_reference_run(name, prec):
    fx, dt = Fixture(name), DT[prec]
    c = fx.cfg
    ns, K, n_neg = c["num_samples"], fx.K, c["neg_sample_size"]
    feats, adj = fx["graph/feats"].astype(dt), fx["graph/adj_train"]
    assert fx.has("init/edge_predict/weights") == c["bilinear_weights"]
    for s in range(fx.n_steps):
        p = "s%d/" % s
        params, W = step_inputs(fx, s, prec)
        roots = [fx[p + "batch1"], fx[p + "batch2"], fx[p + "neg_samples"]]
        B = len(roots[0])
        per_group = []
        for gi, r in enumerate(roots):
            smp, support = orc.sample(adj, r, ns, [fx[p + "perm%d" % (gi * K + k)] for k in range(K)])
            for k in range(K):
                assert np.array_equal(smp[k + 1], fx[p + "sampled%d" % (gi * K + k)].reshape(-1)), (s, gi, k)
            per_group.append(smp)
        samples = [np.concatenate([g[h] for g in per_group]) for h in range(K + 1)]
        with lo.installed(orc, c["loss_fn"], W) as box:
            res = orc.unsupervised_fwd_bwd(params["agg"], feats, samples, support, fx.dims, ns, B, n_neg, "mean", c["concat"],
                                           weight_decay=c["weight_decay"])
        q = p + prec + "/"
        close(res["loss"], fx[q + "loss"], prec, "loss")
        close(res["aff_all"], fx[q + "aff_all"], prec, "aff_all")
        close(res["outputs_all"][:B], fx[q + "outputs1"], prec)
        close(res["outputs_all"][B:2 * B], fx[q + "outputs2"], prec)
        close(res["outputs_all"][2 * B:], fx[q + "neg_outputs"], prec)
        ref_aff = fx[q + "aff_all"]
        solid = np.abs(ref_aff[:, :-1] - ref_aff[:, -1:]).min(axis=1) > 1e-4            # float near-ties aside
        assert np.array_equal(np.asarray(res["ranks"])[solid], fx[q + "ranks"][:, -1][solid])
        if solid.all():
            close(res["mrr"], fx[q + "mrr"], prec, "mrr")
        # the head's gradients carried back to every aggregator variable, and the bilinear matrix's own
        for k, g in flat_items({"agg": res["grads"]}):
            close(g, fx[q + "grad/" + k], prec, "grad/" + k)
        if W is not None:
            # no weight-decay term although weight_decay > 0: _loss decays aggregator variables only (models.py:386-388)
            assert c["weight_decay"] > 0
            close(box["last"]["d_W"] / dt(B), fx[q + "grad/edge_predict/weights"], prec, "grad/edge_predict/weights")
        # the head alone on the reference's stored (normalised) outputs
        head = lo.linkpred(fx[q + "outputs1"].astype(dt), fx[q + "outputs2"].astype(dt), fx[q + "neg_outputs"].astype(dt),
                           c["loss_fn"], W)
        close(head["aff_all"], ref_aff, prec, "aff_all from stored outputs")
        if c["weight_decay"] == 0:
            close(head["loss"] / dt(B), fx[q + "loss"], prec, "loss from stored outputs")
    assert fx.n_steps >= 2


@pytest.mark.parametrize("name", ["unsup_hinge", "unsup_hinge_bilinear"])
def test_hinge_fixtures_stay_off_the_kink_and_use_both_branches(name):
    """What the generator asserts, on the committed files: no entry of n_ij - a_i + margin within 1e-3 of 0 (a 1e-4 float
    difference cannot flip a mask), at least 20 % of the entries active and 20 % inactive -- both legs, every step."""
    fx = Fixture(name)
    for s in range(fx.n_steps):
        for prec in ("32", "64"):
            t = lo.hinge_terms(fx["s%d/%s/aff_all" % (s, prec)], 0.1)
            assert np.abs(t).min() >= 1e-3
            assert 0.2 <= (t > 0).mean() <= 0.8


@pytest.mark.parametrize("bilinear", [False, True])
@pytest.mark.parametrize("loss_fn", ["xent", "skipgram", "hinge"])
def test_oracle_gradients_equal_finite_differences(loss_fn, bilinear):
    rng = np.random.RandomState(5)
    B, n_neg, d = 3, 4, 6
    y1, y2, neg = [lo.l2_normalize(rng.randn(n, d)) for n in (B, B, n_neg)]
    W = rng.uniform(-0.5, 0.5, (d, d)) if bilinear else None
    res = lo.linkpred(y1, y2, neg, loss_fn, W)
    if loss_fn == "hinge":
        assert np.abs(lo.hinge_terms(res["aff_all"])).min() > 1e-4          # off the kink: the loss is smooth around here
    h = 1e-6
    for key, x in (("d_o1", y1), ("d_o2", y2), ("d_neg", neg), ("d_W", W)):
        if x is None:
            continue
        num = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            old = x[idx]
            x[idx] = old + h
            up = lo.linkpred(y1, y2, neg, loss_fn, W)["loss"]
            x[idx] = old - h
            dn = lo.linkpred(y1, y2, neg, loss_fn, W)["loss"]
            x[idx] = old
            num[idx] = (up - dn) / (2 * h)
        np.testing.assert_allclose(res[key], num, rtol=1e-6, atol=1e-8, err_msg=key)


def test_skipgram_keeps_the_reference_sign_and_a_stable_log_sum_exp():
    """prediction.py:115-116 is `aff - log sum exp(neg_aff)`: the loss GROWS with the true pair's affinity.  Rows far from 0
    must not overflow (row maximum subtracted)."""
    y1 = np.asarray([[1.0, 0.0]])
    neg = np.asarray([[0.0, 1.0], [0.6, 0.8]])
    lo_aff = lo.linkpred(y1, np.asarray([[0.0, 1.0]]), neg, "skipgram")["loss"]
    hi_aff = lo.linkpred(y1, np.asarray([[1.0, 0.0]]), neg, "skipgram")["loss"]
    assert hi_aff - lo_aff == pytest.approx(1.0)
    big = lo.linkpred(y1, y1, neg, "skipgram", W=np.eye(2) * 1000.0)
    assert np.isfinite(big["loss"]) and big["loss"] == pytest.approx(1000.0 - 600.0, rel=1e-12)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "graphsage")), reason="the reference's sources are not on this machine")
def test_generator_reproduces_the_committed_fixtures(tmp_path):
    env = dict(os.environ, REF_FIXTURE_DIR=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(HERE, "golden", "make_ref_linkpred_fixtures.py")], env=env,
                          stdout=subprocess.DEVNULL)
    for name in CASES:
        a = np.load(os.path.join(HERE, "golden", "ref_%s.npz" % name))
        b = np.load(os.path.join(str(tmp_path), "ref_%s.npz" % name))
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)


# ------------------------------------------------------------------------------------------------ host-only surface
class _HostEngine(object):
    """What a Layer constructor asks of the engine (no device needed): dropout site ids and variable registration."""

    def __init__(self):
        self.added = []

    def new_site(self):
        return 16

    def add_variable(self, name, init, decay=False, scatter=False):
        self.added.append((name, np.asarray(init), decay))
        return self.added[-1]


@pytest.fixture
def host_engine():
    from graphsage_amd import engine as eng
    e = _HostEngine()
    eng.set_engine(e)
    try:
        yield e
    finally:
        eng.reset_engine()


@pytest.mark.parametrize("loss_fn", ["xent", "skipgram", "hinge"])
@pytest.mark.parametrize("bilinear", [False, True])
@pytest.mark.parametrize("bias", [False, True])
def test_constructor_accepts_the_reference_surface(host_engine, loss_fn, bilinear, bias):
    """prediction.py:13-15: every loss, bilinear_weights and bias construct (the parent raised NotImplementedError)."""
    from graphsage_amd.prediction import BipartiteEdgePredLayer
    layer = BipartiteEdgePredLayer(64, 64, {}, act="sigmoid", loss_fn=loss_fn, bias=bias, bilinear_weights=bilinear,
                                   name="edge_predict")
    assert (layer.loss_fn, layer.bilinear_weights, layer.bias, layer.margin, layer.output_dim) == (loss_fn, bilinear, bias, 0.1, 1)
    assert sorted(layer.vars) == sorted((["weights"] if bilinear else []) + (["bias"] if bias else []))
    assert layer.default_head == (loss_fn == "xent" and not bilinear)
    by_name = {n: (a, dec) for n, a, dec in host_engine.added}
    if bilinear:
        w, decay = by_name["edge_predict/weights"]
        r = np.sqrt(6.0 / 128)
        assert w.shape == (64, 64) and decay is False and np.abs(w).max() <= r and np.abs(w).max() > 0.5 * r    # Glorot-uniform
    if bias:
        b, decay = by_name["edge_predict/bias"]
        assert b.shape == (1,) and not b.any() and decay is False
    assert len(by_name) == int(bilinear) + int(bias)


def test_constructor_refuses_what_it_cannot_run(host_engine):
    from graphsage_amd._lib import GraphsageAmdError
    from graphsage_amd.prediction import BipartiteEdgePredLayer
    with pytest.raises(ValueError):
        BipartiteEdgePredLayer(64, 64, {}, loss_fn="margin")
    for d1, d2 in ((64, 128), (96, 96)):                    # a square matrix at a width the kernel takes
        with pytest.raises(GraphsageAmdError):
            BipartiteEdgePredLayer(d1, d2, {}, bilinear_weights=True)
    assert host_engine.added == []


def test_driver_flags_and_log_directory(tmp_path):
    from graphsage_amd import unsupervised_train as ut
    base = ["--base_log_dir", str(tmp_path)]
    f = ut.build_flags(base)
    assert f.loss_fn == "xent" and f.bilinear_weights is False
    f = ut.build_flags(base + ["--loss_fn", "hinge", "--bilinear_weights"])
    assert f.loss_fn == "hinge" and f.bilinear_weights is True
    with pytest.raises(SystemExit):
        ut.build_flags(["--loss_fn", "margin"])
    old = ut.FLAGS
    try:
        want = str(tmp_path) + "/unsup-data/graphsage_small_0.000010"
        for argv, suffix in (([], ""), (["--loss_fn", "hinge"], "_hinge"), (["--loss_fn", "skipgram"], "_skipgram"),
                             (["--bilinear_weights"], "_bilinear"), (["--loss_fn", "hinge", "--bilinear_weights"], "_hinge_bilinear"),
                             (["--model", "n2v", "--loss_fn", "hinge", "--bilinear_weights"], None)):
            ut.FLAGS = ut.build_flags(base + argv)
            got = ut.log_dir()
            assert got == (want + suffix + "/" if suffix is not None else str(tmp_path) + "/unsup-data/n2v_small_0.000010/")
            assert os.path.isdir(got)
    finally:
        ut.FLAGS = old


def test_model_passes_the_head_arguments_and_leaves_the_fused_tail_to_xent():
    """Source-level: the keyword arguments exist with the reference's defaults (no device needed to read a signature)."""
    import inspect
    from graphsage_amd.models import SampleAndAggregate
    sig = inspect.signature(SampleAndAggregate.__init__).parameters
    assert (sig["loss_fn"].default, sig["bilinear_weights"].default, sig["pred_bias"].default) == ("xent", False, False)

    class Probe(object):
        fuse_tail, layer_infos, aggregator_type = True, [0, 1], "mean"
    for loss_fn, bilinear in (("hinge", False), ("skipgram", False), ("xent", True)):
        m = Probe()
        m.loss_fn, m.bilinear_weights = loss_fn, bilinear
        assert SampleAndAggregate._lp_tail_ok(m) is False         # decided before anything else of the model is read


def test_header_and_binding_declare_the_new_entry_points():
    from graphsage_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    version = int(re.search(r"#define GS_ABI_VERSION (\d+)\b", header).group(1))
    assert version == _lib.GS_ABI_VERSION          # added entry points only: no struct layout changed
    declared = sorted(set(re.findall(r"\b(gs_linkpred_loss_[a-z0-9_]+)\s*\(", header)))
    assert declared == ["gs_linkpred_loss_fwd_bwd", "gs_linkpred_loss_fwd_bwd_step"]
    for name in declared:
        assert name in _lib.EXPORTED_SYMBOLS
    for kind, code in ops.LP_LOSS_KINDS.items():
        assert re.search(r"#define GS_LP_LOSS_%s %d\b" % (kind.upper(), code), header)
    lib = _lib.load()
    assert lib.gs_abi_version() == version and all(hasattr(lib, n) for n in declared)
