"""CPU suite of the in-batch softmax (InfoNCE) head, loss_fn='infonce'.  Nothing in the reference pins this loss, so the NumPy
oracle (tests/infonce_oracle.py) is checked against central finite differences and against torch autograd, both in float64;
the GPU suite (tests/test_infonce_gpu.py) then holds the kernel to the oracle.  Plus the host-only surface: constructor,
flags, log directory, signatures, the ABI."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import infonce_oracle as io
import linkpred_oracle as lo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def draw(B, n_neg, d, seed, bilinear=False, masked=False):
    rng = np.random.RandomState(seed)
    y1, y2, neg = [lo.l2_normalize(rng.randn(n, d)) for n in (B, B, n_neg)]
    W = rng.uniform(-0.5, 0.5, (d, d)) if bilinear else None
    ids1 = ids2 = None
    if masked:
        ids1, ids2 = np.arange(B, dtype=np.int32), np.arange(100, 100 + B, dtype=np.int32)
        ids2[B - 1] = ids2[0]                 # the same context in two pairs: each leaves the other out
        ids1[1] = ids2[2]                     # the query of pair 1 is the context of pair 2: row 1 leaves candidate 2 out
    return y1, y2, neg, W, ids1, ids2


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("bilinear", [False, True])
def test_oracle_gradients_equal_finite_differences(bilinear, masked):
    B, n_neg, d, tau = 4, 3, 6, 0.3
    y1, y2, neg, W, ids1, ids2 = draw(B, n_neg, d, 5, bilinear, masked)
    res = io.infonce(y1, y2, neg, tau, ids1, ids2, W)
    assert io.mask(B, n_neg, ids1, ids2).sum() == (3 if masked else 0)
    h = 1e-6
    for key, x in (("d_o1", y1), ("d_o2", y2), ("d_neg", neg), ("d_W", W)):
        if x is None:
            assert res[key] is None
            continue
        num = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            old = x[idx]
            x[idx] = old + h
            up = io.infonce(y1, y2, neg, tau, ids1, ids2, W)["loss"]
            x[idx] = old - h
            dn = io.infonce(y1, y2, neg, tau, ids1, ids2, W)["loss"]
            x[idx] = old
            num[idx] = (up - dn) / (2 * h)
        np.testing.assert_allclose(res[key], num, rtol=1e-6, atol=1e-8, err_msg=key)


@pytest.mark.parametrize("tau", [0.01, 0.1, 10.0])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("bilinear", [False, True])
def test_oracle_equals_torch_autograd(bilinear, masked, tau):
    B, n_neg, d = 7, 5, 8
    y1, y2, neg, W, ids1, ids2 = draw(B, n_neg, d, 11, bilinear, masked)
    res = io.infonce(y1, y2, neg, tau, ids1, ids2, W)
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in (("y1", y1), ("y2", y2), ("neg", neg), ("W", W))
         if v is not None}
    u = t["y1"] @ t["W"] if bilinear else t["y1"]
    L = u @ torch.cat([t["y2"], t["neg"]], dim=0).T / tau
    Lm = L.masked_fill(torch.from_numpy(io.mask(B, n_neg, ids1, ids2)), float("-inf"))
    rows = torch.logsumexp(Lm, dim=1) - torch.diagonal(L[:, :B])
    rows.sum().backward()
    np.testing.assert_allclose(res["loss_rows"], rows.detach().numpy(), rtol=1e-12, atol=1e-12)
    for key, name in (("d_o1", "y1"), ("d_o2", "y2"), ("d_neg", "neg"), ("d_W", "W")):
        if name in t:
            np.testing.assert_allclose(res[key], t[name].grad.numpy(), rtol=1e-10, atol=1e-12, err_msg=key)
    assert np.isfinite(res["loss_rows"]).all() and (res["loss_rows"] >= 0).all()


def test_one_pair_reduces_to_the_plain_softmax():
    """B = 1, n_neg = 3: loss = -log softmax([pos | negs] / tau)[0], the ranks and aff_all those of the sampled negatives."""
    y1, y2, neg, _, _, _ = draw(1, 3, 6, 3)
    tau = 0.2
    for ids in ((None, None), (np.asarray([4], np.int32), np.asarray([9], np.int32))):
        res = io.infonce(y1, y2, neg, tau, *ids)
        z = np.concatenate([y1 @ y2.T, y1 @ neg.T], axis=1)[0] / tau
        p = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
        assert res["loss_rows"][0] == pytest.approx(-np.log(p[0]), rel=1e-12)
        np.testing.assert_allclose(res["aff_all"][0], np.concatenate([(y1 @ neg.T)[0], (y1 @ y2.T)[0]]), rtol=1e-12)
        assert res["ranks"][0] == ((y1 @ neg.T)[0] >= (y1 @ y2.T)[0, 0]).sum()
        np.testing.assert_allclose(res["d_o2"][0], (p[0] - 1) * y1[0] / tau, rtol=1e-12)
        np.testing.assert_allclose(res["d_neg"], p[1:, None] * y1 / tau, rtol=1e-12)


def test_mask_leaves_out_false_negatives_only():
    ids1 = np.asarray([0, 7, 2, 3], np.int32)
    ids2 = np.asarray([5, 6, 7, 5], np.int32)
    m = io.mask(4, 2, ids1, ids2)
    want = np.zeros((4, 6), bool)
    want[0, 3] = want[3, 0] = True            # ids2[0] == ids2[3]
    want[1, 2] = True                         # ids2[2] == ids1[1]
    assert np.array_equal(m, want)
    y1, y2, neg, _, _, _ = draw(4, 2, 6, 9)
    a, b = io.infonce(y1, y2, neg, 0.1), io.infonce(y1, y2, neg, 0.1, ids1, ids2)
    assert (b["loss_rows"][[0, 1, 3]] < a["loss_rows"][[0, 1, 3]]).all() and b["loss_rows"][2] == a["loss_rows"][2]
    assert b["d_o2"][3] @ y1[0] != a["d_o2"][3] @ y1[0]
    assert np.array_equal(a["aff_all"], b["aff_all"]) and np.array_equal(a["ranks"], b["ranks"])      # sampled negatives only


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


@pytest.mark.parametrize("bilinear", [False, True])
def test_constructor_accepts_infonce(host_engine, bilinear):
    from graphsage_amd.prediction import LOSS_FNS, BipartiteEdgePredLayer
    assert LOSS_FNS == ("xent", "skipgram", "hinge", "infonce")
    layer = BipartiteEdgePredLayer(64, 64, {}, loss_fn="infonce", bilinear_weights=bilinear, name="edge_predict")
    assert (layer.loss_fn, layer.temperature, layer.default_head) == ("infonce", 0.1, False)
    assert sorted(layer.vars) == (["weights"] if bilinear else [])
    assert BipartiteEdgePredLayer(64, 64, {}, loss_fn="infonce", temperature=2.0, name="e2").temperature == 2.0
    assert inspect.signature(BipartiteEdgePredLayer.__init__).parameters["temperature"].default == 0.1
    sig = inspect.signature(BipartiteEdgePredLayer.loss_and_grads_fused).parameters
    assert sig["ids"].default is None and sig["epilogue"].default is None


def test_constructor_refuses_what_the_head_cannot_run(host_engine):
    from graphsage_amd._lib import GraphsageAmdError
    from graphsage_amd.prediction import BipartiteEdgePredLayer
    for tau in (0.001, 0.0, -1.0, 10.5, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            BipartiteEdgePredLayer(64, 64, {}, loss_fn="infonce", temperature=tau)
    for d1, d2 in ((64, 128), (96, 96)):
        with pytest.raises(GraphsageAmdError, match="infonce"):
            BipartiteEdgePredLayer(d1, d2, {}, loss_fn="infonce")
    assert host_engine.added == []
    # the temperature belongs to this loss alone: the others do not look at it
    assert BipartiteEdgePredLayer(96, 96, {}, loss_fn="hinge", temperature=0.001, name="h").temperature == 0.001


def test_model_takes_the_temperature_and_keeps_the_per_operator_schedule():
    from graphsage_amd.models import SampleAndAggregate
    sig = inspect.signature(SampleAndAggregate.__init__).parameters
    assert sig["loss_temperature"].default == 0.1 and sig["loss_fn"].default == "xent"

    class Probe(object):
        fuse_tail, layer_infos, aggregator_type = True, [0, 1], "mean"
    for bilinear in (False, True):
        m = Probe()
        m.loss_fn, m.bilinear_weights = "infonce", bilinear
        assert SampleAndAggregate._lp_tail_ok(m) is False         # decided before anything else of the model is read


def test_driver_flags_and_log_directory(tmp_path):
    from graphsage_amd import unsupervised_train as ut
    base = ["--base_log_dir", str(tmp_path)]
    f = ut.build_flags(base)
    assert f.loss_fn == "xent" and f.loss_temperature == 0.1
    ut.refuse_loss_flags(f)
    f = ut.build_flags(base + ["--loss_fn", "infonce", "--loss_temperature", "0.5"])
    assert f.loss_fn == "infonce" and f.loss_temperature == 0.5
    ut.refuse_loss_flags(f)
    for bad in ("0.001", "0", "11", "nan"):
        with pytest.raises(SystemExit, match="loss_temperature"):
            ut.refuse_loss_flags(ut.build_flags(base + ["--loss_fn", "infonce", "--loss_temperature", bad]))
    ut.refuse_loss_flags(ut.build_flags(base + ["--loss_fn", "hinge", "--loss_temperature", "0.001"]))      # ignored by the others
    with pytest.raises(SystemExit, match="n2v"):
        ut.refuse_loss_flags(ut.build_flags(base + ["--model", "n2v", "--loss_fn", "infonce"]))
    ut.refuse_loss_flags(ut.build_flags(base + ["--model", "n2v", "--loss_temperature", "0.001"]))
    old = ut.FLAGS
    try:
        want = str(tmp_path) + "/unsup-data/graphsage_small_0.000010"
        for argv, suffix in ((["--loss_fn", "infonce"], "_infonce"), (["--loss_fn", "infonce", "--bilinear_weights"], "_infonce_bilinear"),
                             (["--loss_temperature", "0.5"], "")):
            ut.FLAGS = ut.build_flags(base + argv)
            got = ut.log_dir()
            assert got == want + suffix + "/" and os.path.isdir(got)
    finally:
        ut.FLAGS = old


def test_main_refuses_a_temperature_out_of_range_before_any_work(tmp_path, capsys):
    from graphsage_amd import unsupervised_train as ut
    old = ut.FLAGS
    try:
        with pytest.raises(SystemExit, match="loss_temperature"):
            ut.main(["--synthetic", "small", "--base_log_dir", str(tmp_path), "--loss_fn", "infonce", "--loss_temperature", "0.001"])
    finally:
        ut.FLAGS = old
    assert "Loading training data" not in capsys.readouterr().out


def test_header_and_binding_declare_the_new_entry_points():
    from graphsage_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    version = int(re.search(r"#define GS_ABI_VERSION (\d+)\b", header).group(1))
    assert version == _lib.GS_ABI_VERSION == 12          # added entry points only: no struct layout changed
    declared = sorted(set(re.findall(r"\bint (gs_linkpred_infonce_[a-z0-9_]+)\s*\(", header)))
    assert declared == ["gs_linkpred_infonce_fwd_bwd", "gs_linkpred_infonce_fwd_bwd_step", "gs_linkpred_infonce_ws_floats"]
    for name in declared:
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._PROTOS
    assert len(_lib._PROTOS["gs_linkpred_infonce_fwd_bwd_step"]) == len(_lib._PROTOS["gs_linkpred_infonce_fwd_bwd"]) + 9
    assert ops.INFONCE_TAU_RANGE == (0.01, 10.0) and "infonce" not in ops.LP_LOSS_KINDS
    lib = _lib.load()
    assert lib.gs_abi_version() == version and all(hasattr(lib, n) for n in declared)
