"""-m gpu: the fused-tail launches with the layer-1 neighbor means as an INPUT (gs_sage_tail_fwd_bwd_means, gs_sage_tail_z_means,
gs_linkpred_tail_means: graphsage_amd/csrc/gs_tail_dev.h, TailArgs.means_ready).  The neighbor-term helper workgroups load 16 rows
of `means` instead of summing 16 x s rows of h0; with means = the float32 expression the helpers use (zero start, j = 0..s-1, one
multiply by 1.f / s -- what gs_sage_dense_fwd_tiled3_means writes) EVERY output has the bits of the plain entry's, the hand-over
error word stays 0 and `means` is not written.  h0 is about half zeros, so the relu bits of the input gradients matter."""
import numpy as np
import pytest
import torch

from graphsage_amd import ops
from graphsage_amd._lib import GraphsageAmdError
from graphsage_amd.ops import Mat

pytestmark = pytest.mark.gpu

SHAPES = [(16, 10, 256, 128),     # one full group
          (20, 11, 256, 128),     # ragged group
          (48, 1, 128, 64)]       # D = 128 and O = 64 instantiation, s = 1
C = 41


def np_means(h0, n, s):
    v = np.zeros((n, h0.shape[1]), dtype=np.float32)
    hop = h0[n:].reshape(n, s, h0.shape[1])
    for j in range(s):
        v = v + hop[:, j]
    return v * (np.float32(1) / np.float32(s))


def _operands(rng, rows, D, O, dev):
    h0n = np.maximum(rng.normal(size=(rows, D)), 0).astype(np.float32)
    assert 0.4 < (h0n == 0).mean() < 0.6
    Ws = Mat.from_numpy((rng.normal(size=(D, O)) * 0.2).astype(np.float32), dev)
    Wn = Mat.from_numpy((rng.normal(size=(D, O)) * 0.2).astype(np.float32), dev)
    return h0n, Mat.from_numpy(h0n, dev), Ws, Wn


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("n,s,D,O", SHAPES)
def test_tail_fwd_bwd_means(dev, n, s, D, O):
    rng = np.random.default_rng(n + s + D)
    rows, Z = n + n * s, 2 * O
    h0n, h0, Ws, Wn = _operands(rng, rows, D, O, dev)
    Wh = Mat.from_numpy((rng.normal(size=(Z, C)) * 0.3).astype(np.float32), dev)
    bh = torch.from_numpy((rng.normal(size=(C,)) * 0.1).astype(np.float32)).to(dev)
    lab = Mat.from_numpy(np.eye(C, dtype=np.float32)[rng.integers(0, C, n)], dev)
    want_means = np_means(h0n, n, s)
    outs = []
    for ready in (False, True):
        means = Mat.from_numpy(want_means, dev) if ready else Mat.zeros(n, D, dev)
        z, y = Mat.zeros(n, Z, dev), Mat.zeros(n, Z, dev)
        lo, pr, dl = Mat.zeros(n, C, dev), Mat.zeros(n, C, dev), Mat.zeros(n, C, dev)
        lr, dz, dh0 = torch.zeros(n, device=dev), Mat.zeros(n, Z, dev), Mat.zeros(rows, D, dev)
        sync = torch.zeros(ops.tail_sync_words(n, O), dtype=torch.int32, device=dev)       # fresh hand-over state of its own
        torch.cuda.synchronize()
        ops.sage_tail_fwd_bwd(h0, n, s, Ws, Wn, O, Wh, bh, lab, C, False, means, z, y, lo, pr, dl, lr, dz=dz, d_h0=dh0, sync=sync,
                              means_ready=ready)
        torch.cuda.synchronize()
        assert ops.tail_sync_error(sync, n) == 0
        outs.append([m.numpy() for m in (means, z, y, lo, pr, dl, dz, dh0)] + [lr.cpu().numpy()])
    assert np.array_equal(outs[0][0], want_means)            # the plain entry's means ARE the float32 formula
    assert _same(outs[0], outs[1])
    assert np.abs(outs[1][7]).max() > 0 and (outs[1][7] == 0).mean() > 0.3       # d_h0: written, and masked by the relu bits


@pytest.mark.parametrize("n,s,D,O", SHAPES)
def test_tail_z_means(dev, n, s, D, O):
    rng = np.random.default_rng(n + s + D + 1)
    rows, Z = n + n * s, 2 * O
    h0n, h0, Ws, Wn = _operands(rng, rows, D, O, dev)
    want_means = np_means(h0n, n, s)
    outs = []
    for ready in (False, True):
        means = Mat.from_numpy(want_means, dev) if ready else Mat.zeros(n, D, dev)
        z = Mat.zeros(n, Z, dev)
        ops.sage_tail_z(h0, n, s, Ws, Wn, O, means, z, means_ready=ready)
        torch.cuda.synchronize()
        outs.append([means.numpy(), z.numpy()])
    assert np.array_equal(outs[0][0], want_means)
    assert _same(outs[0], outs[1]) and np.abs(outs[1][1]).max() > 0


@pytest.mark.parametrize("n,s,D,O", SHAPES)
def test_linkpred_tail_means(dev, n, s, D, O):
    """B = 12 pairs (a partial pair group), 20 negatives (ragged negative groups): n = 44 roots whatever the shape's n."""
    B, nn = 12, 20
    n = 2 * B + nn
    rng = np.random.default_rng(s + D + O)
    rows, Z = n + n * s, 2 * O
    h0n, h0, Ws, Wn = _operands(rng, rows, D, O, dev)
    want_means = np_means(h0n, n, s)
    assert ops.linkpred_tail_supported(D, O, nn)
    outs = []
    for ready in (False, True):
        means = Mat.from_numpy(want_means, dev) if ready else Mat.zeros(n, D, dev)
        z, y, dz, dh0 = Mat.zeros(n, Z, dev), Mat.zeros(n, Z, dev), Mat.zeros(n, Z, dev), Mat.zeros(rows, D, dev)
        lr, rr, aff = torch.zeros(B, device=dev), torch.zeros(B, device=dev), Mat.zeros(B, nn + 1, dev)
        slabs = torch.zeros(((B + 7) // 8) * nn * Z, device=dev)
        loss, mrr = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        sync = torch.zeros(ops.lp_tail_sync_words(B, nn), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        desc = ops.linkpred_tail_desc(h0, B, nn, s, Ws, Wn, O, means, z, y, lr, rr, aff, 1.0, 1.0 / B, sync, dz=dz, d_h0=dh0,
                                      neg_slabs=slabs)
        ops.linkpred_tail(desc, means_ready=ready)
        ops.linkpred_tail_neg(desc, loss_out=loss, accumulate=False, mrr_out=mrr)
        torch.cuda.synchronize()
        assert ops.lp_tail_sync_error(sync, B, nn) == 0
        outs.append([m.numpy() for m in (means, z, y, dz, dh0, aff)] + [t.cpu().numpy() for t in (lr, rr, slabs, loss, mrr)])
    assert np.array_equal(outs[0][0], want_means)
    assert _same(outs[0], outs[1])
    assert np.abs(outs[1][4]).max() > 0 and np.isfinite(outs[1][9]).all()


def test_means_entries_refuse_the_gcn_form(dev):
    """The GCN mean includes the self row: the *_means entries answer GS_ENOTSUP (-3) and launch nothing."""
    n, s, D, O = 16, 10, 256, 128
    rng = np.random.default_rng(5)
    rows, Z = n + n * s, 2 * O
    h0 = Mat.from_numpy(np.maximum(rng.normal(size=(rows, D)), 0).astype(np.float32), dev)
    W = Mat.from_numpy((rng.normal(size=(D, Z)) * 0.2).astype(np.float32), dev)          # ONE matrix, its two column halves
    Ws, Wn = W.cols_slice(0, O), W.cols_slice(O, Z)
    Wh, bh = Mat.zeros(Z, C, dev), torch.zeros(C, device=dev)
    lab = Mat.from_numpy(np.eye(C, dtype=np.float32)[rng.integers(0, C, n)], dev)
    means, z, y = Mat.zeros(n, D, dev), Mat.zeros(n, Z, dev), Mat.zeros(n, Z, dev)
    lo, pr, dl = Mat.zeros(n, C, dev), Mat.zeros(n, C, dev), Mat.zeros(n, C, dev)
    lr, dz, dh0 = torch.zeros(n, device=dev), Mat.zeros(n, Z, dev), Mat.zeros(rows, D, dev)
    with pytest.raises(GraphsageAmdError, match=r"rc=-3"):
        ops.sage_tail_fwd_bwd(h0, n, s, Ws, Wn, O, Wh, bh, lab, C, False, means, z, y, lo, pr, dl, lr, dz=dz, d_h0=dh0, gcn=True,
                              means_ready=True)
    with pytest.raises(GraphsageAmdError, match=r"rc=-3"):
        ops.sage_tail_z(h0, n, s, Ws, Wn, O, means, z, means_ready=True, gcn=True)
    torch.cuda.synchronize()
    assert float(z.buf.abs().max().item()) == 0.0
