"""-m gpu: the link-prediction head generalised over the loss kind and the left operand (csrc/gs_linkpred_loss.hip).

  * the kernel through the C ABI against tests/linkpred_oracle.py (float64) on rows of a 1/64 grid: a partial last
    workgroup and a single live wave (B = 1, 5, 9), n_neg = 1, 3, 20, d = 64, 256 (+ 512 with 3 negatives), every loss, with
    and without the separate left operand U, a clamped (all-zero) raw row;
  * unsupported shapes return the library's error and launch nothing;
  * the reference's own runs (tests/golden/ref_unsup_{hinge,skipgram,hinge_bilinear,xent_bilinear}.npz) step by step, in the
    manner of test_ref_pin_gpu._unsupervised_steps;
  * the default configuration is untouched (bit-identical to a model built without the new arguments, fused tail in use);
  * hipGraph replay of the device epoch == single eager launches, bit for bit.
Tolerances: the close() rule of tests/test_ref_pin_gpu.py (RTOL = 1e-4); ranks compared off near-ties (1e-4)."""
import os
import re

import numpy as np
import pytest
import torch

import linkpred_oracle as lo
from graphsage_amd import _lib, ops
from graphsage_amd import engine as eng
from graphsage_amd import inits
from graphsage_amd.models import Placeholder, SAGEInfo, SampleAndAggregate
from graphsage_amd.neigh_samplers import AdjInfo, PaddedAdjacency, UniformNeighborSampler
from graphsage_amd.ops import Mat
from ref_fixtures import Fixture
from test_ref_pin_gpu import ADAM_KNEE, RTOL, close, model_variables

pytestmark = pytest.mark.gpu
MARGIN = 0.1
SENTINEL = -77.0

SHAPES = [(B, nn, d) for d in (64, 256) for nn in (1, 3, 20) for B in (1, 5, 9)] + [(B, 3, 512) for B in (1, 5, 9)]
# the second block of 64 negatives: lane 63 of block 0, lane 0 of block 1, the LDS bound n_neg * d = 8192
SECOND_BLOCK = [(5, 64, 64), (5, 65, 64), (5, 128, 64)]


def _sync():
    torch.cuda.synchronize()


def _grid(rng, rows, d, scale):
    return np.round(rng.normal(size=(rows, d)) * scale * 64) / 64


def draw(kind, with_u, B, nn, d, seed):
    """Rows on a 1/64 grid (exact in fp32).  Without U they are RAW aggregator outputs (one of them all zero: the clamped
    normalisation); with U they stand for normalised rows (norm ~ 1) and U for l2_normalize(outputs1) . W.  Hinge inputs are
    drawn again until no n_ij - a_i + margin lies within 1e-3 of 0 (the subgradient jumps there)."""
    rng = np.random.RandomState(seed)
    n_rows = 2 * B + nn
    for _ in range(200):
        if with_u:
            X = _grid(rng, n_rows, d, 1.0 / np.sqrt(d))
            U = _grid(rng, B, d, 1.5 / np.sqrt(d))
            U[:] = np.round((U + 0.1 * X[B:2 * B]) * 64) / 64               # true pairs correlate a little: both hinge branches occur
            zero_row = None
            res = lo.linkpred(U, X[B:2 * B], X[2 * B:], kind, None, MARGIN)
        else:
            X = _grid(rng, n_rows, d, 1.0)
            X[:B] += 0.15 * X[B:2 * B]
            X = np.round(X * rng.uniform(0.3, 3.0, size=(n_rows, 1)) * 64) / 64
            U = None
            zero_row = (B + nn + d // 64) % n_rows
            X[zero_row] = 0.0
            y = lo.l2_normalize(X)
            res = lo.linkpred(y[:B], y[B:2 * B], y[2 * B:], kind, None, MARGIN)
        if kind != "hinge" or np.abs(lo.hinge_terms(res["aff_all"], MARGIN)).min() >= 1e-3:
            return X, U, zero_row, res
    raise AssertionError("no hinge draw off the kink")


def run_kernel(dev, kind, X, U, B, nn, d, scale, epilogue=None):
    n_rows = 2 * B + nn
    Xd = Mat.from_numpy(X.astype(np.float32), dev)
    out = dict(Y=Mat.zeros(n_rows, d, dev), dX=Mat.zeros(n_rows, d, dev), aff=Mat.zeros(B, nn + 1, dev),
               loss_rows=torch.zeros(B, device=dev), rr=torch.zeros(B, device=dev),
               slabs=torch.zeros(((B + 3) // 4) * nn * d, device=dev))
    out["dX"].buf.fill_(SENTINEL)
    out["loss_rows"].fill_(SENTINEL)
    Ud = dU = None
    if U is not None:
        Ud, dU = Mat.from_numpy(U.astype(np.float32), dev), Mat.zeros(B, d, dev)
        out["dU"] = dU
    _sync()
    ops.linkpred_loss_fwd_bwd(kind, Xd, B, nn, 1.0, MARGIN, scale, out["loss_rows"], out["rr"], out["aff"], out["dX"],
                              out["slabs"], Y=out["Y"] if U is None else None, U=Ud, dU=dU, epilogue=epilogue,
                              stream=ops.current_stream())
    _sync()
    return out


@pytest.mark.parametrize("with_u", [False, True])
@pytest.mark.parametrize("kind", ["hinge", "skipgram", "xent"])
@pytest.mark.parametrize("B,nn,d", SHAPES + SECOND_BLOCK)
def test_loss_kernel_equals_oracle(dev, B, nn, d, kind, with_u):
    scale = 1.0 / B
    X, U, zero_row, want = draw(kind, with_u, B, nn, d, seed=1000 * B + 10 * nn + d + len(kind))
    out = run_kernel(dev, kind, X, U, B, nn, d, scale)
    close(out["loss_rows"].cpu().numpy(), want["loss_rows"], "loss_rows")
    close(out["aff"].numpy(), want["aff_all"], "aff_all")
    solid = np.abs(want["aff_all"][:, :-1] - want["aff_all"][:, -1:]).min(axis=1) > 1e-4          # float near-ties aside
    if (B, nn, d) in SECOND_BLOCK:
        assert solid.mean() >= 0.8                              # the near-tie filter hides no wrong rank
    got_rank = np.round(1.0 / out["rr"].cpu().numpy() - 1).astype(np.int64)
    assert np.array_equal(got_rank[solid], want["ranks"][solid])
    got = out["dX"].numpy().astype(np.float64)
    if with_u:
        close(out["dU"].numpy(), want["d_o1"] * scale, "dU")
        close(got[B:2 * B], want["d_o2"] * scale, "d outputs2")
        close(got[2 * B:], want["d_neg"] * scale, "d negatives")
        assert (got[:B] == SENTINEL).all()                      # the caller's rows (dU . W^T goes there)
        return
    y = lo.l2_normalize(X)
    close(out["Y"].numpy(), y, "normalised rows")
    d_y = np.concatenate([want["d_o1"], want["d_o2"], want["d_neg"]], axis=0) * scale
    d_z = lo.l2_normalize_bwd(d_y, X)
    live = np.ones(2 * B + nn, bool)
    live[zero_row] = False                                      # the clamped row is 1e6-scaled: compared by itself
    close(got[live], d_z[live], "dZ")
    close(got[~live], d_z[~live], "dZ of the clamped row")


def test_hinge_draws_use_both_branches():
    """The hinge cases above are no vacuous gradient check: at every shape with several pairs and >= 15 entries both branches
    of the relu occur (a single pair's entries share one a_i and may all fall on one side)."""
    for with_u in (False, True):
        for B, nn, d in [s for s in SHAPES if s[0] >= 5 and s[0] * s[1] >= 15]:
            t = lo.hinge_terms(draw("hinge", with_u, B, nn, d, seed=1000 * B + 10 * nn + d + 5)[3]["aff_all"], MARGIN)
            assert 0 < (t > 0).sum() < t.size, (with_u, B, nn, d)


@pytest.mark.parametrize("with_u", [False, True])
def test_step_epilogue_rides_in_the_second_launch(dev, with_u):
    B, nn, d = 9, 3, 64
    X, U, _, want = draw("hinge", with_u, B, nn, d, seed=3)
    loss_out, mrr_out = torch.full((1,), 5.0, device=dev), torch.zeros(1, device=dev)
    c0, c1 = torch.full((1,), 7, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    out = run_kernel(dev, "hinge", X, U, B, nn, d, 1.0 / B, epilogue=(loss_out, True, mrr_out, [(c0, 1), (c1, 3), (None, 0)]))
    close(loss_out.item(), 5.0 + want["loss"] / B, "accumulated mean loss")
    close(mrr_out.item(), (1.0 / (np.round(1.0 / out["rr"].cpu().numpy() - 1) + 1)).mean(), "mrr")
    assert (int(c0.item()), int(c1.item())) == (8, 3)


def _epilogue(dev):
    loss_out, mrr_out = torch.full((1,), 5.0, device=dev), torch.zeros(1, device=dev)
    c0, c1 = torch.full((1,), 7, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    return (loss_out, True, mrr_out, [(c0, 1), (c1, 3), (None, 0)])


def _same(a, b):
    return np.array_equal(a.cpu().numpy() if torch.is_tensor(a) else a.numpy(), b.cpu().numpy() if torch.is_tensor(b) else b.numpy())


@pytest.mark.parametrize("B,d,nn", [(9, 64, 3), (5, 64, 65)])
def test_norm_entry_points_are_the_general_kernel(dev, B, d, nn):
    """gs_linkpred_norm_fwd_bwd_step == gs_linkpred_loss_fwd_bwd_step(xent, U = NULL): every buffer, the means and the counters,
    bit for bit, from the same inputs into sentinel-filled outputs."""
    X = draw("xent", False, B, nn, d, seed=7)[0]
    epi_a, epi_b = _epilogue(dev), _epilogue(dev)
    a = run_kernel(dev, "xent", X, None, B, nn, d, 1.0 / B, epilogue=epi_a)
    n_rows = 2 * B + nn
    Xd = Mat.from_numpy(X.astype(np.float32), dev)
    b = dict(Y=Mat.zeros(n_rows, d, dev), dX=Mat.zeros(n_rows, d, dev), aff=Mat.zeros(B, nn + 1, dev),
             loss_rows=torch.full((B,), SENTINEL, device=dev), rr=torch.zeros(B, device=dev),
             slabs=torch.zeros(((B + 3) // 4) * nn * d, device=dev))
    b["dX"].buf.fill_(SENTINEL)
    loss_out, _, mrr_out, ((c0, d0), (c1, d1), _) = epi_b
    _sync()
    ops.call("gs_linkpred_norm_fwd_bwd_step", Xd.ptr, Xd.ld, B, d, nn, 1.0, 1.0 / B, b["Y"].ptr, b["Y"].ld, ops.ptr(b["loss_rows"]),
             ops.ptr(b["rr"]), b["aff"].ptr, b["aff"].ld, b["dX"].ptr, b["dX"].ld, ops.ptr(b["slabs"]), ops.ptr(loss_out), 1,
             ops.ptr(mrr_out), ops.ptr(c0), d0, ops.ptr(c1), d1, None, 0, ops.current_stream())
    _sync()
    for k in b:
        assert _same(a[k], b[k]), k
    assert not (b["dX"].numpy() == SENTINEL).any() and not (b["loss_rows"] == SENTINEL).any()
    assert _same(epi_a[0], loss_out) and _same(epi_a[2], mrr_out) and loss_out.item() != 5.0
    assert [int(c.item()) for c, _ in epi_a[3][:2]] == [int(c0.item()), int(c1.item())] == [8, 3]


@pytest.mark.parametrize("B,d,nn", [(9, 64, 3), (5, 64, 65)])
def test_normalised_rows_entry_point_is_the_general_kernel(dev, B, d, nn):
    """gs_linkpred_fwd_bwd + gs_reduce_slabs == gs_linkpred_loss_fwd_bwd(xent, U = rows [0, B) of X): the pair rows, loss_rows,
    rr_rows and aff_all bit for bit; the negatives' rows to rounding (the two slab reductions sum in different orders)."""
    import ctypes
    X = draw("xent", True, B, nn, d, seed=11)[0]
    a = run_kernel(dev, "xent", X, X[:B], B, nn, d, 1.0 / B)
    n_rows, n_slabs = 2 * B + nn, (B + 3) // 4
    Yd, dY, aff = Mat.from_numpy(X.astype(np.float32), dev), Mat.zeros(n_rows, d, dev), Mat.zeros(B, nn + 1, dev)
    dY.buf.fill_(SENTINEL)
    loss_rows, rr = torch.full((B,), SENTINEL, device=dev), torch.zeros(B, device=dev)
    slabs, ns = torch.zeros(n_slabs * nn * d, device=dev), ctypes.c_int32()
    _sync()
    ops.call("gs_linkpred_fwd_bwd", Yd.ptr, Yd.ld, B, d, nn, 1.0, 1.0 / B, ops.ptr(loss_rows), ops.ptr(rr), aff.ptr, aff.ld,
             dY.ptr, dY.ld, ops.ptr(slabs), ctypes.byref(ns), ops.current_stream())
    assert ns.value == n_slabs
    dneg = dY.rows_slice(2 * B, n_rows)
    ops.call("gs_reduce_slabs", ops.ptr(slabs), n_slabs, nn * d, nn, d, d, 0.0, None, 0, dneg.ptr, dneg.ld, 0, ops.current_stream())
    _sync()
    got, want = dY.numpy(), a["dX"].numpy()
    assert np.array_equal(got[:B], a["dU"].numpy()) and np.array_equal(got[B:2 * B], want[B:2 * B])
    assert _same(loss_rows, a["loss_rows"]) and _same(rr, a["rr"]) and _same(aff, a["aff"]) and _same(slabs, a["slabs"])
    assert not (got == SENTINEL).any()
    close(got[2 * B:], want[2 * B:].astype(np.float64), "d negatives")


@pytest.mark.parametrize("nn,d,what", [(3, 96, "d must be"), (20, 512, "do not fit LDS")])
def test_unsupported_shapes_are_refused_before_any_launch(dev, nn, d, what):
    B = 5
    rng = np.random.RandomState(0)
    X = _grid(rng, 2 * B + nn, d, 1.0)
    for kind in ("hinge", "skipgram"):
        for U in (None, _grid(rng, B, d, 1.0)):
            with pytest.raises(_lib.GraphsageAmdError, match=what):
                run_kernel(dev, kind, X, U, B, nn, d, 1.0)
    # nothing ran: a fresh set of outputs keeps its fill
    n_rows = 2 * B + nn
    Xd, dX = Mat.from_numpy(X.astype(np.float32), dev), Mat.zeros(n_rows, d, dev)
    Y, loss_rows, rr = Mat.zeros(n_rows, d, dev), torch.full((B,), SENTINEL, device=dev), torch.zeros(B, device=dev)
    dX.buf.fill_(SENTINEL)
    slabs = torch.full((2 * nn * d,), SENTINEL, device=dev)
    _sync()
    with pytest.raises(_lib.GraphsageAmdError):
        ops.linkpred_loss_fwd_bwd("hinge", Xd, B, nn, 1.0, MARGIN, 1.0, loss_rows, rr, None, dX, slabs, Y=Y,
                                  stream=ops.current_stream())
    _sync()
    assert (dX.buf == SENTINEL).all() and (loss_rows == SENTINEL).all() and (slabs == SENTINEL).all()
    with pytest.raises(_lib.GraphsageAmdError, match="unknown loss kind"):
        ops.linkpred_loss_fwd_bwd(7, Mat.zeros(2 * B + 3, 64, dev), B, 3, 1.0, MARGIN, 1.0, loss_rows, rr, None,
                                  Mat.zeros(2 * B + 3, 64, dev), slabs, Y=Mat.zeros(2 * B + 3, 64, dev), stream=ops.current_stream())


# ------------------------------------------------------------------------------------------------ the reference's own runs
def _build_fixture_model(fx, **head):
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
                               neg_sample_size=c["neg_sample_size"], **head)
    model.use_graphs = False                      # the padded sampler takes a host permutation per call
    return e, ph, sampler, model


def _variables(model):
    mv = model_variables(model, supervised=False)
    if model.bilinear_weights:
        mv["edge_predict/weights"] = model.link_pred_layer.vars['weights']
    return mv


def _load(mv, fx, prefix):
    assert sorted(mv) == sorted(k[len(prefix):] for k in fx.z.files if k.startswith(prefix))
    for k, v in mv.items():
        v.assign(fx[prefix + k].astype(np.float32).reshape(v.numpy().shape))
    eng.get_engine().sync()


@pytest.mark.parametrize("name", ["unsup_hinge", "unsup_skipgram", "unsup_hinge_bilinear", "unsup_xent_bilinear"])
def test_unsupervised_steps_equal_reference_run(dev, name):
    """The reference's BipartiteEdgePredLayer with the case's loss_fn / bilinear_weights, every step: sampled ids bit-exact;
    loss, aff_all, the three embedding groups, every gradient (edge_predict/weights among them) and the parameters after
    clip + Adam within 1e-4 (same ADAM_KNEE exclusion as test_ref_pin_gpu)."""
    fx = Fixture(name)
    c = fx.cfg
    K, n_neg = fx.K, c["neg_sample_size"]
    e, ph, sampler, model = _build_fixture_model(fx, loss_fn=c["loss_fn"], bilinear_weights=c["bilinear_weights"])
    mv = _variables(model)
    assert ("edge_predict/weights" in mv) == c["bilinear_weights"]
    _load(mv, fx, "init/")
    for s in range(fx.n_steps):
        p = "s%d/" % s
        b1, b2, neg = fx[p + "batch1"], fx[p + "batch2"], fx[p + "neg_samples"]
        B = len(b1)
        sampler.inject_perms(fx.perms(p, 3 * K))
        model.inject_negatives(neg)
        loss, ranks, aff_all, mrr, outputs1 = model.train_step({ph['batch1']: b1, ph['batch2']: b2, ph['batch_size']: B})
        assert model._lp_tail_used is False                                   # the per-operator schedule
        assert np.array_equal(model.samples1[0].cpu().numpy(), np.concatenate([b1, b2, neg]))
        for k in range(K):
            want = np.concatenate([fx[p + "sampled%d" % (g * K + k)].reshape(-1) for g in range(3)])
            assert np.array_equal(model.samples1[k + 1].cpu().numpy(), want), (s, k)
        close(loss, fx[p + "32/loss"], "loss step %d" % s)
        close(aff_all, fx[p + "32/aff_all"], "aff_all")
        close(outputs1, fx[p + "32/outputs1"], "outputs1")
        full = model.outputs_all.numpy()
        close(full[B:2 * B], fx[p + "32/outputs2"], "outputs2")
        close(full[2 * B:2 * B + n_neg], fx[p + "32/neg_outputs"], "neg_outputs")
        ref_aff = fx[p + "32/aff_all"]
        margin = np.abs(ref_aff[:, :-1] - ref_aff[:, -1:]).min(axis=1) > 1e-4           # float near-ties aside
        assert np.array_equal(np.asarray(ranks)[margin], fx[p + "32/ranks"][:, -1][margin])
        if margin.all():
            close(mrr, fx[p + "32/mrr"], "mrr")
        for k, v in mv.items():
            close(v.grad.numpy(), fx[p + "32/grad/" + k], "grad/%s step %d" % (k, s))
        for k, v in mv.items():
            want, g = fx[p + "32/after/" + k], fx[p + "32/grad/" + k]
            solid = np.abs(g) > max(1e-6 * max(1e-2, np.abs(g).max()), ADAM_KNEE)
            np.testing.assert_allclose(v.numpy().reshape(want.shape)[solid], want[solid], rtol=RTOL, atol=2e-5,
                                       err_msg="after/%s step %d" % (k, s))
        for k, v in mv.items():
            v.assign(fx[p + "32/after/" + k].astype(np.float32).reshape(v.numpy().shape))
        e.sync()
    assert fx.n_steps >= 2


def test_prediction_bias_is_created_and_never_updated(dev):
    """bias=True: vars['bias'] is [1] zeros in the flat buffer; the reference never reads it (prediction.py:55-56), so it gets
    no gradient and clip + Adam leave it at 0."""
    fx = Fixture("unsup_hinge")
    e, ph, sampler, model = _build_fixture_model(fx, loss_fn="hinge", pred_bias=True)
    bias = model.link_pred_layer.vars['bias']
    _load(model_variables(model, supervised=False), fx, "init/")
    sampler.inject_perms(fx.perms("s0/", 3 * fx.K))
    model.inject_negatives(fx["s0/neg_samples"])
    b1, b2 = fx["s0/batch1"], fx["s0/batch2"]
    loss = model.train_step({ph['batch1']: b1, ph['batch2']: b2, ph['batch_size']: len(b1)})[0]
    close(loss, fx["s0/32/loss"], "loss")
    assert bias.numpy().shape == (1, 1) and bias.decay is False
    assert not bias.numpy().any() and not bias.grad.numpy().any()


def test_default_arguments_leave_the_fused_tail_path_bit_identical(dev):
    """loss_fn='xent', bilinear_weights=False == a model built without the new arguments: two steps of ref_unsup_mean_tail,
    same loss and parameter bits, and the fused two-launch tail is still what runs."""
    fx = Fixture("unsup_mean_tail")
    runs = []
    for head in ({}, dict(loss_fn='xent', bilinear_weights=False, pred_bias=False)):
        e, ph, sampler, model = _build_fixture_model(fx, **head)
        _load(model_variables(model, supervised=False), fx, "init/")
        losses = []
        for s in range(2):
            p = "s%d/" % s
            b1, b2 = fx[p + "batch1"], fx[p + "batch2"]
            sampler.inject_perms(fx.perms(p, 3 * fx.K))
            model.inject_negatives(fx[p + "neg_samples"])
            losses.append(model.train_step({ph['batch1']: b1, ph['batch2']: b2, ph['batch_size']: len(b1)})[0])
            assert model._lp_tail_used is True
        e.sync()
        runs.append((np.asarray(losses, np.float32), e.params.cpu().numpy().copy()))
    assert fx.n_steps >= 2
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()


# ------------------------------------------------------------------------------------------------ device epoch / replay
def _build_synthetic(**head):
    """The small synthetic graph of tests/test_unsup_gpu.py (its build(csr=True)) with the head's arguments."""
    from graphsage_amd.minibatch import EdgeMinibatchIterator
    from graphsage_amd.neigh_samplers import CSRAdjacency
    from graphsage_amd.utils import synthetic_graph
    from test_unsup_gpu import placeholders
    eng.reset_engine()
    inits.set_seed(11)
    np.random.seed(7)
    G = synthetic_graph(n_nodes=400, feat_dim=50, num_classes=5, avg_degree=6, seed=5)
    ph = placeholders()
    it = EdgeMinibatchIterator(G, None, ph, context_pairs=None, batch_size=32, max_degree=10)
    e = eng.get_engine()
    adj_info = AdjInfo(CSRAdjacency(it.train_csr[0], it.train_csr[1], G.n_nodes, e.device))
    sampler = UniformNeighborSampler(adj_info)
    layer_infos = [SAGEInfo("node", sampler, 5, 32), SAGEInfo("node", sampler, 3, 32)]
    model = SampleAndAggregate(ph, G.padded_features(), adj_info, it.deg, layer_infos, concat=True, aggregator_type="mean",
                               learning_rate=0.01, weight_decay=0.0, neg_sample_size=6, **head)
    return it, ph, model


def test_graph_replay_of_the_device_epoch_is_bit_identical(dev):
    """8 steps of train_step_device with loss_fn='hinge', bilinear_weights=True: eager | captured | replayed launches give the
    loss and parameter bits of 8 single eager launches (no in-kernel hand-over on this path, the epilogue folded into the
    head's second launch)."""
    runs = []
    for graphs in (True, False):
        it, ph, model = _build_synthetic(loss_fn="hinge", bilinear_weights=True)
        model.use_graphs = graphs
        model.attach_device_pairs(it.train_edges[:256])
        losses = [model.train_step_device(32, fetch=True)[0] for _ in range(8)]
        assert model._lp_tail_used is False and model._epilogue_folded is True
        assert bool(model._graphs) == graphs
        e = eng.get_engine()
        e.sync()
        runs.append((np.asarray(losses, np.float32), e.params.cpu().numpy().copy()))
    assert np.isfinite(runs[0][0]).all() and len(set(runs[0][0].tolist())) > 1
    assert runs[0][0].tobytes() == runs[1][0].tobytes(), (runs[0][0], runs[1][0])
    assert runs[0][1].tobytes() == runs[1][1].tobytes()


def test_eval_step_and_feed_path_agree_with_the_device_epoch(dev):
    """train_step (host-fed) == train_step_device on the same pairs, and eval_step reports the loss of the head in use."""
    outs = []
    for mode in ("feed", "device"):
        it, ph, model = _build_synthetic(loss_fn="skipgram", bilinear_weights=False)
        pairs = it.train_edges[:96]
        if mode == "feed":
            model.use_graphs = False
            for i in range(3):
                ed = pairs[i * 32:(i + 1) * 32]
                model.train_step({ph['batch1']: ed[:, 0], ph['batch2']: ed[:, 1], ph['batch_size']: 32})
        else:
            model.attach_device_pairs(pairs)
            for i in range(3):
                model.train_step_device(32)
        eng.get_engine().sync()
        outs.append(eng.get_engine().params.cpu().numpy().copy())
    assert np.array_equal(outs[0], outs[1])
    ed = pairs[:32]
    loss, ranks, mrr, outputs1 = model.eval_step({ph['batch1']: ed[:, 0], ph['batch2']: ed[:, 1], ph['batch_size']: 32})
    aff = model.aff_all.numpy().astype(np.float64)
    mx = aff[:, :-1].max(axis=1)
    want = (aff[:, -1] - (mx + np.log(np.exp(aff[:, :-1] - mx[:, None]).sum(axis=1)))).mean()
    close(loss, want, "skipgram loss of eval_step")
    assert np.isfinite(mrr) and 0 < mrr <= 1 and np.allclose(np.linalg.norm(outputs1, axis=1), 1.0, atol=1e-4)


def test_driver_trains_with_hinge_and_bilinear_weights(dev, tmp_path, capsys):
    from graphsage_amd import unsupervised_train as ut
    eng.reset_engine()
    ut.main(["--synthetic", "small", "--model", "graphsage_mean", "--epochs", "1", "--batch_size", "128", "--samples_1", "5",
             "--samples_2", "3", "--dim_1", "32", "--dim_2", "32", "--max_total_steps", "50", "--print_every", "10",
             "--validate_iter", "25", "--learning_rate", "0.001", "--max_walk_pairs", "20000", "--base_log_dir", str(tmp_path),
             "--loss_fn", "hinge", "--bilinear_weights"])
    out = capsys.readouterr().out
    assert "Optimization Finished!" in out
    lines = re.findall(r"train_loss= (\d+\.\d{5}) train_mrr= (\d\.\d{5})", out)
    assert len(lines) >= 4 and all(np.isfinite(float(a)) and 0 < float(b) <= 1 for a, b in lines)
    npy = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs if f == "val.npy"]
    assert len(npy) == 1 and "/graphsage_mean_small_0.001000_hinge_bilinear/" in npy[0]
    emb = np.load(npy[0])
    assert emb.shape == (3000, 64) and np.allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-4)
