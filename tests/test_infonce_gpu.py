"""-m gpu: the in-batch softmax (InfoNCE) head, csrc/gs_infonce.hip, through the C ABI against the float64 oracle of
tests/infonce_oracle.py evaluated on the same (float32-valued) rows.

  * tile edges of the 128 x 128 sweep (B and B + n_neg at 1, tile - 1, tile, tile + 1, several tiles), every width, ld = d + 4,
    without and with mask ids; sweeps long enough that a gradient workgroup walks several tiles and the last cut is short,
    more than 64 candidate tiles in the finish launch; phantom (padded) columns; the mask across tiles; exactly representable scores; the temperature
    range; forward only; repeatability; refused arguments; the bilinear schedule of the layer;
  * whole steps of the model on the graph of tests/golden/ref_unsup_mean_tail.npz (its inputs only: the reference has no such
    loss), eager | captured | replayed steps, evaluation, the driver.
Tolerances: loss_rows, aff_all and the whole-step quantities take close() of tests/test_ref_pin_gpu.py (1e-4); the head's raw
gradients carry the factor scale / tau and take 1e-4 * scale / tau absolute."""
import os
import re

import numpy as np
import pytest
import torch

import infonce_oracle as io
import linkpred_oracle as lo
from graphsage_amd import _lib, ops
from graphsage_amd import engine as eng
from graphsage_amd.ops import Mat
from oracle import graphsage_oracle as orc
from oracle import sampler_hash
from ref_fixtures import Fixture
from test_ref_pin_gpu import ADAM_KNEE, RTOL, close, model_variables

pytestmark = pytest.mark.gpu
TILE = 128                      # RK_BM = RK_BN of csrc/gs_rank_dev.h
SENTINEL = -77.0

TILE_EDGES = [(1, 0, 64), (1, 1, 64), (5, 20, 64), (TILE - 1, 1, 64), (TILE, 0, 64), (TILE + 1, TILE + 2, 64), (200, 20, 64)] + \
             [(TILE + 1, 20, d) for d in (64, 128, 256, 512)]


def _sync():
    torch.cuda.synchronize()


def padded(a, dev, pad=4, fill=None):
    """Mat of a [rows, d] array with ld = d + pad (d rounded up to whole float4 first)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.zeros((a.shape[0], ops.round_up(a.shape[1], 4) + pad), dtype=torch.float32, device=dev)
    if fill is not None:
        buf.fill_(fill)
    else:
        buf[:, :a.shape[1]].copy_(torch.from_numpy(a))
    return Mat(buf, a.shape[1])


def unit_rows(rng, n, d):
    """float32 rows of norm 1 (to rounding), as float64: what the device gets and what the oracle computes on."""
    x = rng.randn(n, d)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)


def draw_ids(rng, B):
    """Node ids with collisions of both kinds at every B > 1 (drawn from 2B values)."""
    return rng.randint(0, 2 * B, size=B).astype(np.int32), rng.randint(0, 2 * B, size=B).astype(np.int32)


def run_head(dev, u, y2, neg, tau, scale, ids=None, left=None, grads=True, epilogue=None):
    """left: a separate left operand [B, d] (else rows [0, B) of X, as the layer passes them without bilinear weights)."""
    B, d, nn = u.shape[0], u.shape[1], neg.shape[0]
    X = padded(np.concatenate([u, y2, neg], axis=0), dev)
    U = padded(left, dev) if left is not None else X.rows_slice(0, B)
    out = dict(loss_rows=torch.full((B,), SENTINEL, device=dev), rr=torch.full((B,), SENTINEL, device=dev),
               aff=padded(np.zeros((B, nn + 1)), dev, fill=SENTINEL),
               stats=torch.zeros(ops.linkpred_infonce_ws_floats(B, d, nn, grads), device=dev))
    if grads:
        out["dX"] = padded(np.zeros((2 * B + nn, d)), dev, fill=SENTINEL)
        out["dU"] = padded(np.zeros((B, d)), dev, fill=SENTINEL)
    dev_ids = None
    if ids is not None:
        dev_ids = tuple(torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).to(dev) for t in ids)
    _sync()
    ops.linkpred_infonce_fwd_bwd(X, U, B, nn, tau, scale, out["loss_rows"], out["rr"], out["aff"], out["stats"],
                                 dX=out.get("dX"), dU=out.get("dU"), ids=dev_ids, epilogue=epilogue, stream=ops.current_stream())
    _sync()
    return out


def check(out, want, B, nn, tau, scale, tag, exact_scores=False):
    """exact_scores: every score is exactly representable, so every rank is compared, ties included."""
    loss = out["loss_rows"].cpu().numpy()
    print("%s: max |loss_rows - oracle| = %.3g" % (tag, np.abs(loss - want["loss_rows"]).max()))
    close(loss, want["loss_rows"], tag + " loss_rows")
    close(out["aff"].numpy(), want["aff_all"], tag + " aff_all")
    assert (out["aff"].buf[:, nn + 1:] == SENTINEL).all()
    if nn:
        solid = np.abs(want["aff_all"][:, :-1] - want["aff_all"][:, -1:]).min(axis=1) > 1e-4          # float near-ties aside
        if exact_scores:
            solid[:] = True
        assert solid.mean() >= 0.8, tag                         # the near-tie filter hides no wrong rank
        got_rank = np.round(1.0 / out["rr"].cpu().numpy() - 1).astype(np.int64)
        assert np.array_equal(got_rank[solid], want["ranks"][solid]), tag
    else:
        assert (out["rr"].cpu().numpy() == 1.0).all()
    if "dX" not in out:
        return
    atol = 1e-4 * scale / tau
    dX, dU = out["dX"].numpy().astype(np.float64), out["dU"].numpy().astype(np.float64)
    d = dU.shape[1]
    for name, got, ref in (("dU", dU, want["d_o1"]), ("d outputs2", dX[B:2 * B], want["d_o2"]), ("d negatives", dX[2 * B:], want["d_neg"])):
        if ref.size:
            print("%s: max |%s - oracle| = %.3g (bound %.3g)" % (tag, name, np.abs(got - ref * scale).max(), atol))
        np.testing.assert_allclose(got, ref * scale, rtol=0, atol=atol, err_msg="%s %s" % (tag, name))
    assert (dX[:B] == SENTINEL).all()                               # the caller's rows
    assert (out["dX"].buf[:, d:] == SENTINEL).all() and (out["dU"].buf[:, d:] == SENTINEL).all()      # the pad columns


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("B,nn,d", TILE_EDGES)
def test_head_equals_oracle_at_the_tile_edges(dev, B, nn, d, with_ids):
    rng = np.random.RandomState(1000 * B + 10 * nn + d)
    u, y2, neg = unit_rows(rng, B, d), unit_rows(rng, B, d), unit_rows(rng, nn, d)
    y2 = lo.l2_normalize(y2 + 0.5 * u).astype(np.float32).astype(np.float64)       # pairs correlate, as trained ones do
    ids = draw_ids(rng, B) if with_ids else None
    tau, scale = 0.1, 1.0 / B
    want = io.infonce(u, y2, neg, tau, *(ids or (None, None)))
    if with_ids and B >= 5:
        assert io.mask(B, nn, *ids).any()
    out = run_head(dev, u, y2, neg, tau, scale, ids=ids, left=u)
    check(out, want, B, nn, tau, scale, "B=%d nn=%d d=%d ids=%s" % (B, nn, d, with_ids))
    # the left operand as rows [0, B) of X (no bilinear weights): the same bits
    again = run_head(dev, u, y2, neg, tau, scale, ids=ids)
    for k in ("loss_rows", "rr", "aff", "dU"):
        assert _same(out[k], again[k]), k
    assert np.array_equal(out["dX"].numpy()[B:], again["dX"].numpy()[B:])


# The gradient sweeps are cut over at most NCE_MAX_CUT = 8 workgroups: beyond 8 swept tiles a workgroup walks `per` > 1 tiles (its
# accumulators, the tile buffer and the stage buffers pass from one tile to the next) and the last cut may be short.
#   (1100, 20): 9 query tiles and 9 candidate tiles -> per = 2, five cuts, the last of one tile, on both sides
#   (5, 1300):  11 candidate tiles for one query tile -> the row owners walk two tiles each, the column owners' sweep is not cut
CUT_SWEEPS = [(1100, 20, 64), (5, 1300, 64)]


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("B,nn,d", CUT_SWEEPS)
def test_head_equals_oracle_where_a_workgroup_walks_several_tiles(dev, B, nn, d, with_ids):
    assert -(-(B + nn) // TILE) > 8
    rng = np.random.RandomState(B + nn)
    u, y2, neg = unit_rows(rng, B, d), unit_rows(rng, B, d), unit_rows(rng, nn, d)
    y2 = lo.l2_normalize(y2 + 0.5 * u).astype(np.float32).astype(np.float64)
    ids = draw_ids(rng, B) if with_ids else None
    tau, scale = 0.1, 1.0 / B
    want = io.infonce(u, y2, neg, tau, *(ids or (None, None)))
    if with_ids:
        assert io.mask(B, nn, *ids).any()
    out = run_head(dev, u, y2, neg, tau, scale, ids=ids, left=u)
    check(out, want, B, nn, tau, scale, "B=%d nn=%d d=%d ids=%s" % (B, nn, d, with_ids))
    again = run_head(dev, u, y2, neg, tau, scale, ids=ids, left=u)
    for k in ("loss_rows", "rr", "aff", "dU", "dX"):
        assert _same(out[k], again[k]), k


def test_forward_only_with_more_than_64_candidate_tiles(dev):
    """65 candidate tiles: the lanes of the finish launch take a second tile each."""
    rng = np.random.RandomState(65)
    B, nn, d, tau = 5, 64 * TILE + 10, 64, 0.1
    u, y2, neg = unit_rows(rng, B, d), unit_rows(rng, B, d), unit_rows(rng, nn, d)
    y2 = lo.l2_normalize(y2 + u).astype(np.float32).astype(np.float64)      # the positives stand clear of 8,202 negatives' scores
    neg[-3:] = u[:3]                                            # the last tile holds the first rows' largest logits
    out = run_head(dev, u, y2, neg, tau, 1.0 / B, left=u, grads=False)
    check(out, io.infonce(u, y2, neg, tau), B, nn, tau, 1.0 / B, "65 tiles")


def _same(a, b):
    return np.array_equal(a.cpu().numpy() if torch.is_tensor(a) else a.numpy(), b.cpu().numpy() if torch.is_tensor(b) else b.numpy())


def test_padded_columns_do_not_enter_the_sum(dev):
    """y2_i = -u_i and every negative anti-aligned with every u_i at tau = 0.05: every real logit is at most -10, so one padded
    zero column (logit 0) in the sum would change loss_rows by an order of magnitude."""
    rng = np.random.RandomState(3)
    B, nn, d, tau = 5, 3, 64, 0.05
    e = rng.randn(1, d)
    u = lo.l2_normalize(e + 0.1 * rng.randn(B, d)).astype(np.float32).astype(np.float64)
    y2 = -u
    neg = -lo.l2_normalize(e + 0.1 * rng.randn(nn, d)).astype(np.float32).astype(np.float64)
    assert (u @ np.concatenate([y2, neg]).T / tau).max() <= -10.0
    want = io.infonce(u, y2, neg, tau)
    leaked = np.log(np.exp(want["stats"][:, 0] + want["stats"][:, 1]) + 1.0) - (want["stats"][:, 0] + want["stats"][:, 1])
    assert leaked.min() > 9.0                                   # what one phantom column would add to every row
    for ids in (None, (np.arange(B), 100 + np.arange(B))):
        out = run_head(dev, u, y2, neg, tau, 1.0 / B, ids=ids, left=u)
        check(out, want, B, nn, tau, 1.0 / B, "phantom columns")


def test_mask_across_tiles(dev):
    """B = 130: ids2 holds one id three times across the two tiles and ids1[5] == ids2[128]; the masked candidates are copies
    of the query row, so they are the largest logits of their rows.  The head equals the masked oracle and is far from the
    unmasked one."""
    rng = np.random.RandomState(9)
    B, nn, d, tau = TILE + 2, 20, 64, 0.1
    scale = 1.0 / B
    u, y2, neg = unit_rows(rng, B, d), unit_rows(rng, B, d), unit_rows(rng, nn, d)
    ids1, ids2 = (1000 + np.arange(B)).astype(np.int32), (5000 + np.arange(B)).astype(np.int32)
    trio = [3, 60, TILE + 1]
    for i in trio:
        ids2[i] = 7777
        u[i] = u[trio[0]]
        y2[i] = u[trio[0]]
    ids1[5] = ids2[TILE]
    y2[TILE] = u[5]
    # a sampled negative close to u_5 takes the mass the masked copy leaves: the negatives' gradient moves with the mask too
    neg[0] = lo.l2_normalize(u[5:6] + 0.3 * unit_rows(rng, 1, d))[0].astype(np.float32)
    m = io.mask(B, nn, ids1, ids2)
    assert m.sum() == 7 and m[5, TILE] and m[3, TILE + 1] and m[TILE + 1, 3] and m[60, 3]
    want, plain = io.infonce(u, y2, neg, tau, ids1, ids2), io.infonce(u, y2, neg, tau)
    rows = trio + [5]
    atol = 1e-4 * scale / tau
    assert np.abs(want["loss_rows"] - plain["loss_rows"])[rows].min() > 0.3               # ... against 1e-4 * |loss|
    for k in ("d_o1", "d_o2", "d_neg"):
        assert np.abs(want[k] - plain[k]).max() * scale > 100 * atol, k
    out = run_head(dev, u, y2, neg, tau, scale, ids=(ids1, ids2), left=u)
    check(out, want, B, nn, tau, scale, "mask")
    got = out["loss_rows"].cpu().numpy()
    assert np.abs(got - plain["loss_rows"])[rows].min() > 0.3
    assert np.abs(out["dU"].numpy() - plain["d_o1"] * scale).max() > 100 * atol
    assert np.abs(out["dX"].numpy()[B:2 * B] - plain["d_o2"] * scale).max() > 100 * atol
    assert np.abs(out["dX"].numpy()[2 * B:] - plain["d_neg"] * scale).max() > 100 * atol
    # without ids the same inputs give the unmasked oracle
    check(run_head(dev, u, y2, neg, tau, scale, left=u), plain, B, nn, tau, scale, "no ids")


def test_exactly_representable_scores_are_bit_equal(dev):
    """Entries in {0, +-2^-4}: every product and every partial sum is exact in fp32, whatever the order."""
    rng = np.random.RandomState(4)
    B, nn, d = TILE + 1, 20, 64
    u, y2, neg = [rng.randint(-1, 2, size=(n, d)).astype(np.float32) / 16 for n in (B, B, nn)]
    want = np.concatenate([u @ neg.T, (u * y2).sum(axis=1, keepdims=True)], axis=1)
    assert want.dtype == np.float32
    out = run_head(dev, u, y2, neg, 0.1, 1.0 / B, left=u)
    assert np.array_equal(out["aff"].numpy(), want)
    check(out, io.infonce(*[a.astype(np.float64) for a in (u, y2, neg)], 0.1), B, nn, 0.1, 1.0 / B, "grid", exact_scores=True)


@pytest.mark.parametrize("tau", [0.01, 1.0, 10.0])
def test_temperature_range(dev, tau):
    rng = np.random.RandomState(6)
    B, nn, d = TILE + 1, 20, 128
    u, y2, neg = unit_rows(rng, B, d), unit_rows(rng, B, d), unit_rows(rng, nn, d)
    y2[:40] = u[:40]                                            # logits reach 1 / tau
    ids = draw_ids(rng, B)
    out = run_head(dev, u, y2, neg, tau, 1.0 / B, ids=ids, left=u)
    for k in ("loss_rows", "rr", "aff", "dX", "dU", "stats"):
        a = out[k].cpu().numpy() if torch.is_tensor(out[k]) else out[k].numpy()
        assert np.isfinite(a[:2 * B] if k == "stats" else a).all(), k       # (stats: the rows' (maximum, log sum) lead the workspace)
    check(out, io.infonce(u, y2, neg, tau, *ids), B, nn, tau, 1.0 / B, "tau=%g" % tau)


def test_forward_only_and_repeatability(dev):
    rng = np.random.RandomState(8)
    B, nn, d, tau = 200, 20, 256, 0.1
    u, y2, neg = unit_rows(rng, B, d), unit_rows(rng, B, d), unit_rows(rng, nn, d)
    ids = draw_ids(rng, B)
    a = run_head(dev, u, y2, neg, tau, 1.0 / B, ids=ids, left=u)
    b = run_head(dev, u, y2, neg, tau, 1.0 / B, ids=ids, left=u)
    for k in a:
        assert _same(a[k], b[k]), k                             # two runs: the same bits in every output
    f = run_head(dev, u, y2, neg, tau, 1.0 / B, ids=ids, left=u, grads=False)
    for k in ("loss_rows", "rr", "aff"):
        assert _same(a[k], f[k]), k
    assert _same(a["stats"][:2 * B], f["stats"][:2 * B]) and f["stats"].numel() < a["stats"].numel()
    assert not (f["loss_rows"] == SENTINEL).any()


@pytest.mark.parametrize("B", [9, TILE + 1])                   # one tile: the gradient launch carries it; a cut sweep: the reduce launch
@pytest.mark.parametrize("grads", [True, False])
def test_step_epilogue_runs_exactly_once(dev, grads, B):
    rng = np.random.RandomState(2)
    nn, d = 3, 64
    u, y2, neg = unit_rows(rng, B, d), unit_rows(rng, B, d), unit_rows(rng, nn, d)
    loss_out, mrr_out = torch.full((1,), 5.0, device=dev), torch.zeros(1, device=dev)
    c0, c1 = torch.full((1,), 7, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    out = run_head(dev, u, y2, neg, 0.1, 1.0 / B, left=u, grads=grads, epilogue=(loss_out, True, mrr_out, [(c0, 1), (c1, 3), (None, 0)]))
    want = io.infonce(u, y2, neg, 0.1)
    close(loss_out.item(), 5.0 + want["loss"] / B, "accumulated mean loss")
    close(mrr_out.item(), out["rr"].cpu().numpy().astype(np.float64).mean(), "mrr")
    assert (int(c0.item()), int(c1.item())) == (8, 3)
    check(out, want, B, nn, 0.1, 1.0 / B, "with the epilogue")


def test_unsupported_arguments_are_refused_before_any_launch(dev):
    rng = np.random.RandomState(0)
    B, nn = 5, 3
    for d, tau, what in ((96, 0.1, "d must be"), (64, 0.001, "temperature"), (64, 11.0, "temperature")):
        u, y2, neg = unit_rows(rng, B, d), unit_rows(rng, B, d), unit_rows(rng, nn, d)
        with pytest.raises(_lib.GraphsageAmdError, match=what):
            run_head(dev, u, y2, neg, tau, 1.0, left=u)
    u, y2, neg = unit_rows(rng, B, 64), unit_rows(rng, B, 64), unit_rows(rng, nn, 64)
    X = padded(np.concatenate([u, y2, neg]), dev)
    loss_rows, rr = torch.full((B,), SENTINEL, device=dev), torch.zeros(B, device=dev)
    stats, aff = torch.zeros(ops.linkpred_infonce_ws_floats(B, 64, nn), device=dev), padded(np.zeros((B, nn + 1)), dev)
    dX, dU = padded(np.zeros((2 * B + nn, 64)), dev, fill=SENTINEL), padded(np.zeros((B, 64)), dev, fill=SENTINEL)
    ids1 = torch.zeros(B, dtype=torch.int32, device=dev)
    _sync()
    with pytest.raises(_lib.GraphsageAmdError, match="both"):
        ops.linkpred_infonce_fwd_bwd(X, X.rows_slice(0, B), B, nn, 0.1, 1.0, loss_rows, rr, aff, stats, dX=dX, dU=None)
    with pytest.raises(_lib.GraphsageAmdError, match="together"):
        ops.linkpred_infonce_fwd_bwd(X, X.rows_slice(0, B), B, nn, 0.1, 1.0, loss_rows, rr, aff, stats, dX=dX, dU=dU, ids=(ids1, None))
    with pytest.raises(_lib.GraphsageAmdError, match="width"):
        ops.linkpred_infonce_fwd_bwd(X, padded(np.zeros((B, 128)), dev), B, nn, 0.1, 1.0, loss_rows, rr, aff, stats, dX=dX, dU=dU)
    with pytest.raises(_lib.GraphsageAmdError, match="aff_all"):
        ops.linkpred_infonce_fwd_bwd(X, X.rows_slice(0, B), B, nn, 0.1, 1.0, loss_rows, rr, None, stats, dX=dX, dU=dU)
    with pytest.raises(_lib.GraphsageAmdError, match="workspace"):
        ops.linkpred_infonce_fwd_bwd(X, X.rows_slice(0, B), B, nn, 0.1, 1.0, loss_rows, rr, aff, stats[:8], dX=dX, dU=dU)
    _sync()
    assert (dX.buf == SENTINEL).all() and (dU.buf == SENTINEL).all() and (loss_rows == SENTINEL).all()


def test_bilinear_schedule_of_the_layer(dev):
    """U = Y1 . W at (129, 20, 128): the layer's five launches against the oracle on the raw rows, d_W through bilinear_wgrad()."""
    from graphsage_amd import inits
    from graphsage_amd.prediction import BipartiteEdgePredLayer
    eng.reset_engine()
    inits.set_seed(3)
    e = eng.get_engine()
    B, nn, d, tau = TILE + 1, 20, 128, 0.1
    layer = BipartiteEdgePredLayer(d, d, {}, loss_fn="infonce", bilinear_weights=True, temperature=tau, name="edge_predict")
    e.finalize()
    rng = np.random.RandomState(12)
    z = (rng.randn(2 * B + nn, d) * rng.uniform(0.3, 3.0, size=(2 * B + nn, 1))).astype(np.float32).astype(np.float64)
    z[:B] += 0.5 * z[B:2 * B]
    z = z.astype(np.float32).astype(np.float64)
    ids = draw_ids(rng, B)
    W = layer.vars['weights'].numpy().astype(np.float64)
    y = lo.l2_normalize(z)
    want = io.infonce(y[:B], y[B:2 * B], y[2 * B:], tau, ids[0], ids[1], W)
    Z, Y, dZ = Mat.from_numpy(z, dev), Mat.zeros(2 * B + nn, d, dev), Mat.zeros(2 * B + nn, d, dev)
    loss_rows, rr, aff = torch.zeros(B, device=dev), torch.zeros(B, device=dev), Mat.zeros(B, nn + 1, dev)
    dev_ids = tuple(torch.from_numpy(t).to(dev) for t in ids)
    _sync()
    scale = 1.0 / B
    layer.loss_and_grads_fused(Z, Y, B, nn, scale, loss_rows, rr, aff, dZ, ids=dev_ids)
    e.begin_backward()
    layer.bilinear_wgrad()
    e.finish_backward(0.0)
    e.sync()
    close(loss_rows.cpu().numpy(), want["loss_rows"], "loss_rows")
    close(aff.numpy(), want["aff_all"], "aff_all")
    close(Y.numpy(), y, "normalised rows")
    d_y = np.concatenate([want["d_o1"], want["d_o2"], want["d_neg"]], axis=0) * scale
    close(dZ.numpy(), lo.l2_normalize_bwd(d_y, z), "dZ")
    close(layer.vars['weights'].grad.numpy(), want["d_W"] * scale, "d_W")
    # forward only (validation): the same loss bits, no gradient written
    loss2, dZ_before = torch.zeros(B, device=dev), dZ.numpy().copy()
    _sync()
    layer.loss_and_grads_fused(Z, Y, B, nn, scale, loss2, rr, aff, None, ids=dev_ids)
    e.sync()
    assert _same(loss_rows, loss2) and np.array_equal(dZ.numpy(), dZ_before)


# ------------------------------------------------------------------------------------------------ whole steps
class _Adam(object):
    """The oracle's clip + TF Adam per variable, with the knee exclusion of tests/test_ref_pin_gpu.py."""

    def __init__(self, lr):
        self.m, self.v, self.t, self.lr = {}, {}, 0, lr

    def step(self, params, grads):
        self.t += 1
        out = {}
        for k, p in params.items():
            g = np.asarray(grads[k], np.float64).reshape(p.shape)
            if k not in self.m:
                self.m[k], self.v[k] = np.zeros_like(p), np.zeros_like(p)
            q = p.copy()
            orc.adam_tf_update(q, orc.clip_by_value(g), self.m[k], self.v[k], self.t, self.lr)
            out[k] = (q, np.abs(g) > max(1e-6 * max(1e-2, np.abs(g).max()), ADAM_KNEE))
        return out


def test_device_steps_equal_the_oracle_on_the_reference_graph(dev):
    """Three train_step_device steps with loss_fn='infonce' on the graph and features of ref_unsup_mean_tail: the staged pairs,
    the negatives and every sampled id bit-exact; loss, mrr, aff_all, every gradient and the parameters after clip + Adam
    against the oracle with the head installed; then evaluation in the forward-only form."""
    from graphsage_amd import inits
    from graphsage_amd.models import Placeholder, SAGEInfo, SampleAndAggregate
    from graphsage_amd.neigh_samplers import AdjInfo, PaddedAdjacency, UniformNeighborSampler
    from test_unsup_gpu import sample_three_calls
    fx = Fixture("unsup_mean_tail")
    c = fx.cfg
    K, ns, nn, tau, B = fx.K, c["num_samples"], c["neg_sample_size"], 0.2, 12
    adj, deg = fx["graph/adj_train"], fx["graph/deg"]
    eng.reset_engine()
    inits.set_seed(1)
    e = eng.get_engine()
    ph = {'batch1': Placeholder('batch1'), 'batch2': Placeholder('batch2'), 'neg_samples': Placeholder('neg'),
          'dropout': Placeholder('dropout', 0.), 'batch_size': Placeholder('batch_size')}
    adj_info = AdjInfo(PaddedAdjacency(adj, e.device))
    sampler = UniformNeighborSampler(adj_info)
    model = SampleAndAggregate(ph, fx["graph/feats"], adj_info, deg, [SAGEInfo("node", sampler, s, fx.out_dim) for s in ns],
                               concat=c["concat"], aggregator_type="mean", learning_rate=c["learning_rate"],
                               weight_decay=c["weight_decay"], neg_sample_size=nn, loss_fn="infonce", loss_temperature=tau)
    model.use_graphs = False                      # the padded sampler takes a host permutation per call
    assert model.link_pred_layer.temperature == tau and model._lp_tail_ok() is False
    rng = np.random.RandomState(21)
    N = fx.n_nodes
    src = rng.choice(np.where(adj[:N, 0] != N)[0], size=3 * B, replace=False).astype(np.int32)
    pairs = np.stack([src, adj[src, 0].astype(np.int32)], axis=1)
    pairs[1, 1] = pairs[0, 1]                     # the same context in two pairs of step 0
    pairs[B + 2, 0] = pairs[B + 3, 1]             # a query that is another pair's context in step 1
    model.attach_device_pairs(pairs)
    mv = model_variables(model, supervised=False)
    feats = fx["graph/feats"].astype(np.float64)
    cdf = sampler_hash.unigram_cdf_u32(deg)
    perms = [[rng.permutation(adj.shape[1]) for _ in range(3 * K)] for _ in range(4)]
    adam = _Adam(c["learning_rate"])
    sampler.inject_perms(perms[0])
    model._prime(B)
    masked = 0
    for s in range(3):
        b1, b2 = pairs[s * B:(s + 1) * B, 0], pairs[s * B:(s + 1) * B, 1]
        params = {k: v.numpy().astype(np.float64) for k, v in mv.items()}
        sampler.inject_perms(perms[s + 1])        # this call samples the NEXT step's neighbors
        loss, ranks, aff_all, mrr, outputs1 = model.train_step_device(B, fetch=True)
        assert model._lp_tail_used is False
        neg = sampler_hash.sample_unigram(cdf, nn, 123, s)
        assert np.array_equal(model.samples1[0].cpu().numpy(), np.concatenate([b1, b2, neg]))
        samples, support = sample_three_calls(adj, b1, b2, neg, ns, perms[s])
        for got, want in zip(model.samples1, samples):
            assert np.array_equal(got.cpu().numpy(), want)
        masked += int(io.mask(B, nn, b1, b2).sum())
        agg = [{k.split("/")[1]: params[k] for k in params if k.startswith("agg%d/" % i)} for i in range(K)]
        with io.installed(orc, tau, {"ids": (b1, b2)}) as box:
            res = orc.unsupervised_fwd_bwd(agg, feats, samples, support, fx.dims, ns, B, nn, "mean", c["concat"],
                                           weight_decay=c["weight_decay"])
        assert box["last"]["d_W"] is None
        close(loss, res["loss"], "loss step %d" % s)
        close(aff_all, res["aff_all"], "aff_all")
        close(outputs1, res["outputs1"], "outputs1")
        solid = np.abs(res["aff_all"][:, :-1] - res["aff_all"][:, -1:]).min(axis=1) > 1e-4
        assert solid.mean() >= 0.8
        assert np.array_equal(np.asarray(ranks)[solid], res["ranks"][solid])
        if solid.all():
            close(mrr, res["mrr"], "mrr")
        grads = {k: res["grads"][int(k[3])][k.split("/")[1]] for k in mv}
        for k, v in mv.items():
            close(v.grad.numpy(), grads[k], "grad/%s step %d" % (k, s))
        for k, (want, ok) in adam.step(params, grads).items():
            np.testing.assert_allclose(mv[k].numpy().reshape(want.shape)[ok], want[ok], rtol=RTOL, atol=2e-5,
                                       err_msg="after/%s step %d" % (k, s))
    assert masked >= 3                             # the mask was in play
    # evaluation: forward only, the loss of the head in use from the embeddings it wrote
    b1, b2 = pairs[:B, 0], pairs[:B, 1]
    sampler.inject_perms(perms[0])
    d_before = model._d_agg_out.numpy().copy()
    loss, ranks, mrr, outputs1 = model.eval_step({ph['batch1']: b1, ph['batch2']: b2, ph['batch_size']: B})
    y = model.outputs_all.numpy().astype(np.float64)
    reg = 0.5 * c["weight_decay"] * sum((v.numpy().astype(np.float64) ** 2).sum() for v in mv.values())     # models.py:386-388
    close(loss, (reg + io.infonce(y[:B], y[B:2 * B], y[2 * B:], tau, b1, b2)["loss"]) / B, "eval loss")
    assert np.array_equal(model._d_agg_out.numpy(), d_before) and 0 < mrr <= 1


@pytest.mark.parametrize("bilinear", [False, True])
def test_graph_replay_of_the_device_epoch_is_bit_identical(dev, bilinear):
    """8 steps of train_step_device with loss_fn='infonce': eager | captured | replayed launches give the loss and parameter
    bits of 8 single eager launches (the check of tests/test_linkpred_gpu.py for this head)."""
    from test_linkpred_gpu import _build_synthetic
    runs = []
    for graphs in (True, False):
        it, ph, model = _build_synthetic(loss_fn="infonce", bilinear_weights=bilinear)
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


def test_driver_trains_with_infonce_and_ranks(dev, tmp_path, capsys):
    from graphsage_amd import unsupervised_train as ut
    eng.reset_engine()
    ut.main(["--synthetic", "small", "--model", "graphsage_mean", "--epochs", "1", "--batch_size", "128", "--samples_1", "5",
             "--samples_2", "3", "--dim_1", "32", "--dim_2", "32", "--max_total_steps", "30", "--print_every", "10",
             "--validate_iter", "15", "--learning_rate", "0.001", "--max_walk_pairs", "8000", "--base_log_dir", str(tmp_path),
             "--loss_fn", "infonce", "--rank_full"])
    out = capsys.readouterr().out
    assert "Optimization Finished!" in out
    lines = re.findall(r"train_loss= (\d+\.\d{5}) train_mrr= (\d\.\d{5})", out)
    assert len(lines) >= 3 and all(np.isfinite(float(a)) and 0 < float(b) <= 1 for a, b in lines)
    assert re.search(r"Full-graph link ranking: mrr= (\d\.\d{5}) hits@1= ", out), out[-2000:]
    npy = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs if f == "val.npy"]
    assert len(npy) == 1 and "/graphsage_mean_small_0.001000_infonce/" in npy[0]
