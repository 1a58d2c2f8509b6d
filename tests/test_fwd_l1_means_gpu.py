"""-m gpu: gs_sage_dense_fwd_tiled3_means (graphsage_amd/csrc/gs_split.hip) -- the tiled layer-0 forward over the rows
[roots | hop 1] that also writes the NEXT layer's neighbor means from its finished tiles.  Claims checked here, all bit for bit:
  * h0 is what gs_sage_dense_fwd_tiled3 of the same library writes (the hop rows are tiled (64 / s) * s to a workgroup instead of
    64, and an element's K reduction does not depend on the tile map);
  * l1_means[i, c] = (((0 + h0[n + i s, c]) + h0[n + i s + 1, c]) + ...) * (1.f / s) in float32 -- the expression of the fused
    tail's z helpers (gs_tail_dev.h), so the tail can load the means instead of forming them;
  * nothing but rows [0, n_roots) x columns [0, 2 out_dim) of l1_means is touched.
Shapes: the smallest that hit every branch of the row tiling (partial / several root tiles, RB = 60 / 55 / 63 / 64, ragged last hop
tile), K with a masked last stage and not a multiple of 4, out_dim with masked columns inside a wave's 32."""
import numpy as np
import pytest
import torch

from graphsage_amd import ops
from graphsage_amd.ops import Mat

pytestmark = pytest.mark.gpu

SHAPES = [(20, 10),     # partial root tile, 60-row hop tiles, last hop tile 20 rows
          (64, 11),     # RB = 55
          (70, 7),      # RB = 63, two root tiles
          (130, 1),     # RB = 64, mean = the row
          (33, 3)]      # ragged root and hop tiles
N_TABLE = 500


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _nan_mat(rows, d, ld, dev):
    m = Mat(torch.full((rows, ld), float("nan"), dtype=torch.float32, device=dev), d)
    return m


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def np_l1_means(h0, n_roots, s):
    """float32, sequential adds from 0 in the order j = 0..s-1, then ONE multiply by the float32 reciprocal."""
    v = np.zeros((n_roots, h0.shape[1]), dtype=np.float32)
    hop = h0[n_roots:].reshape(n_roots, s, h0.shape[1])
    for j in range(s):
        v = v + hop[:, j]
    return v * (np.float32(1) / np.float32(s))


def _check(dev, n_roots, s, K, out, act, gathered=False, riders=False):
    rng = np.random.default_rng(1000 * n_roots + 10 * s + K + out)
    n = n_roots * (1 + s)
    X = rng.normal(size=(N_TABLE, K)).astype(np.float32)
    self_ids = rng.integers(0, N_TABLE, size=n).astype(np.int32)
    self_m = X[self_ids] if gathered else rng.normal(size=(n, K)).astype(np.float32)
    mean = rng.normal(size=(n, K)).astype(np.float32)
    Ws, Wn = (rng.normal(size=(K, out)) * 0.1).astype(np.float32), (rng.normal(size=(K, out)) * 0.1).astype(np.float32)
    b = (rng.normal(size=(2 * out,)) * 0.1).astype(np.float32)
    Xd, sd, md = Mat.from_numpy(X, dev, 32), Mat.from_numpy(self_m, dev, 32), Mat.from_numpy(mean, dev, 4)
    Wsd, Wnd, bd = Mat.from_numpy(Ws, dev), Mat.from_numpy(Wn, dev), torch.from_numpy(b).to(dev)
    sid_d = _i32(self_ids, dev)
    idx = rng.integers(0, N_TABLE, size=(300, 25)).astype(np.int32)
    idx_d = _i32(idx.reshape(-1), dev)
    a_self, a_idx = (Xd, sid_d) if gathered else (sd, None)
    got = []
    for with_means in (False, True):
        h0 = _nan_mat(n, 2 * out, 2 * out + 4, dev)
        g_out = Mat.zeros(300, K, dev)
        jobs = [ops.gather_job(Xd, idx_d, 300, 25, g_out)] if riders else []
        if with_means:
            lm = _nan_mat(n_roots + 3, 2 * out, 2 * out + 8, dev)
            ops.sage_dense_fwd_tiled3_means(a_self, a_idx, md, n, Wsd, Wnd, out, act, bd, h0, n_roots, s, lm, jobs)
        else:
            ops.sage_dense_fwd_tiled3(a_self, a_idx, md, n, Wsd, Wnd, out, act, bd, h0, jobs)
        torch.cuda.synchronize()
        got.append(h0.buf.cpu().numpy())
        if riders:
            np.testing.assert_allclose(g_out.numpy(), X[idx].mean(axis=1), rtol=1e-4, atol=1e-4)
    # h0: the bits of the plain entry, pad columns untouched (NaN bit patterns compared as words)
    assert np.array_equal(_bits(got[0]), _bits(got[1]))
    h0n = got[1][:, :2 * out]
    assert np.isfinite(h0n).all()
    if act == ops.ACT_RELU:
        assert (h0n == 0).mean() > 0.2                      # (the relu really cut: zeros among the summands)
    lmn = lm.buf.cpu().numpy()
    want = np_l1_means(h0n, n_roots, s)
    assert np.array_equal(_bits(lmn[:n_roots, :2 * out]), _bits(want))
    assert np.isnan(lmn[n_roots:]).all() and np.isnan(lmn[:, 2 * out:]).all()


@pytest.mark.parametrize("act", [ops.ACT_RELU, ops.ACT_IDENTITY])
@pytest.mark.parametrize("out", [64, 100, 128])
@pytest.mark.parametrize("K", [50, 602])
@pytest.mark.parametrize("n_roots,s", SHAPES)
def test_fwd_tiled3_means(dev, n_roots, s, K, out, act):
    _check(dev, n_roots, s, K, out, act)


def test_fwd_tiled3_means_gathered_self(dev):
    """The self term gathered through self_idx inside the A loads (how layer 0 reads the feature table)."""
    _check(dev, 70, 7, 602, 128, ops.ACT_RELU, gathered=True)


def test_fwd_tiled3_means_with_riders(dev):
    """One gather+mean job of the next step riding in the launch: rider workgroups start behind the NEW tile count."""
    _check(dev, 20, 10, 602, 100, ops.ACT_RELU, gathered=True, riders=True)


def test_fwd_tiled3_means_rejects_bad_shapes(dev):
    from graphsage_amd._lib import GraphsageAmdError
    K, out = 50, 64
    z = lambda r, d: Mat.zeros(r, d, dev)
    for n, n_roots, s in [(221, 20, 10), (66 * 66, 66, 65), (20, 20, 0)]:
        with pytest.raises(GraphsageAmdError):
            ops.sage_dense_fwd_tiled3_means(z(n, K), None, z(n, K), n, z(K, out), z(K, out), out, ops.ACT_RELU, None, z(n, 2 * out),
                                            n_roots, s, z(n_roots, 2 * out), [])
    torch.cuda.synchronize()
