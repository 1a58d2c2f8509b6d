"""-m gpu: gs_pool2_dgrad through the C ABI -- the input gradient of the first dense layer of the two-layer max-pool,

    dH1[i*s + j, k] = H1[h(i*s + j), k] > 0 ?  sum over { c : argmax[i, c] == j } of dpm[i, c] * W2[k, c]  :  0

against a float64 evaluation of that formula from the same fp32 inputs, next to the three-launch composition it replaces
(gs_segment_max_bwd + gs_dense_dgrad + gs_act_bwd).

Bound, for both sides: |err| <= hid2 * 2^-23 * sum_c |dpm[i, c] * W2[k, c]| over the row's own columns -- a sequential fp32 sum
of at most hid2 products has relative error (hid2 - 1 + 1) u on the sum of magnitudes with u = 2^-24 (each product rounds
once, each of the <= hid2 - 1 additions once); the factor 2 covers the two sides contracting products and additions into FMAs
differently.  Where H1 <= 0, and in rows that won no column, the output is exactly 0; two launches of the new kernel give the
same bits.  The output buffer starts as NaN, so a row or a column the kernel skipped shows."""
import numpy as np
import pytest
import torch

from graphsage_amd import _lib, ops

pytestmark = pytest.mark.gpu
ENOTSUP = -3          # GS_ENOTSUP of include/graphsage_amd.h

# (n, s, hid1, hid2, variant): the smallest shapes that exercise each edge
CASES = [
    (1, 1, 512, 256, "plain"),           # one group of one row: it wins everything
    (3, 25, 512, 256, "plain"),          # the headline fan-out; most rows win ~5 live columns, some none
    (5, 10, 1024, 512, "plain"),         # model_size = "big": two column passes per thread, four float4s of k per lane
    (2, 64, 512, 256, "plain"),          # the largest s: every lane of the offset scan holds a row
    (7, 3, 44, 36, "wide_ld"),           # partial wave of columns, partial wave of float4s; every ld larger than its width
    (4, 5, 512, 256, "h_idx"),           # H1 holds distinct rows, picked through repeated and out-of-order indices
    (3, 4, 512, 256, "one_winner"),      # one row of each group wins every column
    (3, 4, 512, 256, "zero_dpm"),        # nothing to route: exact zeros everywhere
]


def _inputs(n, s, hid1, hid2, variant, seed):
    rng = np.random.RandomState(seed)
    arg = rng.randint(0, s, size=(n, hid2)).astype(np.int32)
    if variant == "one_winner":
        arg[:] = (np.arange(n) % s)[:, None]
    dpm = rng.standard_normal((n, hid2)).astype(np.float32)
    dpm[rng.rand(n, hid2) < 0.5] = 0.0                                # the second relu's mask: about half exactly 0
    if variant == "zero_dpm":
        dpm[:] = 0.0
    W2 = (rng.standard_normal((hid1, hid2)) / np.sqrt(hid2)).astype(np.float32)
    if variant == "h_idx":
        rows_h = 7                                                    # a shorter H1: rows repeat and come out of order
        h_idx = rng.randint(0, rows_h, size=n * s).astype(np.int32)
        h_idx[:4] = [5, 5, 0, 5]
    else:
        rows_h, h_idx = n * s, None
    H1 = rng.standard_normal((rows_h, hid1)).astype(np.float32)       # zero-mean: about half of the mask is closed
    return arg, dpm, W2, H1, h_idx


def _reference(arg, dpm, W2, H1, h_idx, n, s):
    """(dH1, magnitude sums) in float64 from the fp32 inputs; winners[r]: whether row r won a live column."""
    hid1, hid2 = W2.shape
    want = np.zeros((n * s, hid1))
    mag = np.zeros((n * s, hid1))
    for i in range(n):
        for j in range(s):
            cols = np.flatnonzero(arg[i] == j)
            v = dpm[i, cols].astype(np.float64)
            w = W2[:, cols].astype(np.float64)
            want[i * s + j] = w @ v
            mag[i * s + j] = np.abs(w) @ np.abs(v)
    rows = h_idx if h_idx is not None else np.arange(n * s)
    open_ = H1[rows] > 0
    return np.where(open_, want, 0.0), mag, open_


def _padded(a, ld, dev, fill):
    buf = np.full((a.shape[0], ld), fill, a.dtype)
    buf[:, :a.shape[1]] = a
    return torch.from_numpy(buf).to(dev)


def _run(case, dev):
    n, s, hid1, hid2, variant = case
    arg, dpm, W2, H1, h_idx = _inputs(n, s, hid1, hid2, variant, seed=1000 * n + 10 * s + len(variant))
    extra = 8 if variant == "wide_ld" else 0
    ldd, lda, ldw, ldh, ldo = hid2 + extra, hid2 + extra + 4 * bool(extra), hid2 + extra, hid1 + extra, hid1 + 2 * extra
    d_dpm, d_W2, d_H1 = _padded(dpm, ldd, dev, np.nan), _padded(W2, ldw, dev, np.nan), _padded(H1, ldh, dev, np.nan)
    d_arg = _padded(arg, lda, dev, -7)
    d_idx = torch.from_numpy(h_idx).to(dev) if h_idx is not None else None
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    def fused():
        out = torch.full((n * s, ldo), float("nan"), dtype=torch.float32, device=dev)
        rc = lib.gs_pool2_dgrad(d_dpm.data_ptr(), ldd, d_arg.data_ptr(), lda, d_W2.data_ptr(), ldw, d_H1.data_ptr(), ldh,
                                d_idx.data_ptr() if d_idx is not None else None, n, s, hid1, hid2, out.data_ptr(), ldo, stream)
        assert rc == 0, lib.gs_last_error()
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def composed():
        Mat = ops.Mat
        pooled = torch.ones((n, hid2), dtype=torch.float32, device=dev)          # dpm is already masked: pooled > 0 everywhere
        dH2 = torch.full((n * s, hid2), float("nan"), dtype=torch.float32, device=dev)
        out = torch.full((n * s, ldo), float("nan"), dtype=torch.float32, device=dev)
        ops.segment_max_bwd(Mat(d_dpm, hid2), Mat(pooled, hid2), d_arg, n, s, Mat(dH2, hid2))
        ops.dense_dgrad(Mat(dH2, hid2), 0, hid2, n * s, Mat(d_W2, hid2), Mat(out, hid1))
        Hx = Mat(d_H1, hid1) if d_idx is None else ops.gather_rows(Mat(d_H1, hid1), d_idx)
        ops.act_bwd(Mat(out, hid1), Hx, n * s, hid1, ops.ACT_RELU, Mat(out, hid1))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    want, mag, open_ = _reference(arg, dpm, W2, H1, h_idx, n, s)
    return fused, composed, want, mag, open_, (n, s, hid1, hid2, arg, dpm)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%d_%d_%s" % c)
def test_pool2_dgrad_equals_the_formula_and_the_composition(case, dev):
    fused, composed, want, mag, open_, (n, s, hid1, hid2, arg, dpm) = _run(case, dev)
    a, b = fused(), fused()
    assert a.tobytes() == b.tobytes()                                  # one fixed summation order
    bound = hid2 * 2.0 ** -23 * mag
    live = np.zeros((n, s), bool)                                      # rows that won a column with a non-zero gradient
    for i in range(n):
        live[i, np.unique(arg[i][dpm[i] != 0])] = True
    live = live.reshape(-1)
    for name, got in (("pool2_dgrad", a), ("composed", composed())):
        body, pad = got[:, :hid1], got[:, hid1:]
        assert np.isfinite(body).all(), name                           # every row and column written
        assert np.isnan(pad).all(), name                               # nothing beyond the width
        err = np.abs(body.astype(np.float64) - want)
        print("%s %s: max |err| %.3e, max err / bound %.3f" % (case, name, err.max(), (err / np.maximum(bound, 1e-300)).max()
                                                                 if bound.max() > 0 else 0.0))
        assert (err <= bound).all(), name
        assert (body[~open_] == 0).all(), name                         # exactly 0 where H1 <= 0
        assert (body[~live] == 0).all(), name                          # ... and in rows that won no column
    if case[4] == "zero_dpm":
        assert not a[:, :hid1].any()
    if case[4] == "one_winner":
        assert live.sum() == n


@pytest.mark.parametrize("case", [(3, 25, 512, 256, "h_idx"), (7, 3, 44, 36, "wide_ld")], ids=lambda c: "%dx%d_%d_%d_%s" % c)
def test_transpose_and_dgrad_t_with_a_padded_copy(dev, case):
    """What a training step launches: gs_pool2_transpose into a workspace, then gs_pool2_dgrad_t -- here with ldt > hid1 (the
    copy's pad columns stay NaN: neither kernel touches them).  The copy is W2^T bit for bit, and the result has the bits of
    gs_pool2_dgrad on the same inputs (same kernel, same order) and meets the same bound."""
    n, s, hid1, hid2, variant = case
    arg, dpm, W2, H1, h_idx = _inputs(n, s, hid1, hid2, variant, seed=77 + n)
    ldd, lda, ldw, ldh, ldo, ldt = hid2 + 4, hid2 + 8, hid2 + 12, hid1 + 4, hid1 + 8, hid1 + 12
    d_dpm, d_W2, d_H1 = _padded(dpm, ldd, dev, np.nan), _padded(W2, ldw, dev, np.nan), _padded(H1, ldh, dev, np.nan)
    d_arg = _padded(arg, lda, dev, -7)
    d_idx = torch.from_numpy(h_idx).to(dev) if h_idx is not None else None
    idx_ptr = d_idx.data_ptr() if d_idx is not None else None
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    W2T = torch.full((hid2, ldt), float("nan"), dtype=torch.float32, device=dev)
    assert lib.gs_pool2_transpose(d_W2.data_ptr(), ldw, hid1, hid2, W2T.data_ptr(), ldt, stream) == 0, lib.gs_last_error()
    out_t = torch.full((n * s, ldo), float("nan"), dtype=torch.float32, device=dev)
    rc = lib.gs_pool2_dgrad_t(d_dpm.data_ptr(), ldd, d_arg.data_ptr(), lda, W2T.data_ptr(), ldt, d_H1.data_ptr(), ldh, idx_ptr, n, s,
                              hid1, hid2, out_t.data_ptr(), ldo, stream)
    assert rc == 0, lib.gs_last_error()
    out = torch.full((n * s, ldo), float("nan"), dtype=torch.float32, device=dev)
    rc = lib.gs_pool2_dgrad(d_dpm.data_ptr(), ldd, d_arg.data_ptr(), lda, d_W2.data_ptr(), ldw, d_H1.data_ptr(), ldh, idx_ptr, n, s,
                            hid1, hid2, out.data_ptr(), ldo, stream)
    assert rc == 0, lib.gs_last_error()
    torch.cuda.synchronize()
    wt = W2T.cpu().numpy()
    assert np.array_equal(wt[:, :hid1], W2.T) and np.isnan(wt[:, hid1:]).all()
    got = out_t.cpu().numpy()
    assert got.tobytes() == out.cpu().numpy().tobytes()
    want, mag, open_ = _reference(arg, dpm, W2, H1, h_idx, n, s)
    assert np.isnan(got[:, hid1:]).all()
    assert (np.abs(got[:, :hid1].astype(np.float64) - want) <= hid2 * 2.0 ** -23 * mag).all()
    assert (got[:, :hid1][~open_] == 0).all()
    rc = lib.gs_pool2_dgrad_t(d_dpm.data_ptr(), ldd, d_arg.data_ptr(), lda, W2T.data_ptr(), hid1 - 4, d_H1.data_ptr(), ldh, idx_ptr,
                              n, s, hid1, hid2, out_t.data_ptr(), ldo, stream)
    assert rc == -1 and b"gs_pool2_dgrad_t" in lib.gs_last_error()          # ldt < hid1: refused before any launch


def test_iota(dev):
    lib = _lib.load()
    out = torch.full((1000 + 8,), -5, dtype=torch.int32, device=dev)
    assert lib.gs_pool2_iota(out.data_ptr(), 1000, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:1000], np.arange(1000)) and (got[1000:] == -5).all()
    assert lib.gs_pool2_iota(None, 0, None) == 0 and lib.gs_pool2_iota(None, 5, None) == -1


def test_argument_checks_return_before_any_launch(dev):
    lib = _lib.load()
    # s = 65 is outside the kernel's range, n = 0 is empty: neither reads a pointer (all null here)
    rc = lib.gs_pool2_dgrad(None, 256, None, 256, None, 256, None, 512, None, 3, 65, 512, 256, None, 512, None)
    assert rc == ENOTSUP
    assert b"gs_pool2_dgrad" in lib.gs_last_error()
    assert lib.gs_pool2_dgrad(None, 256, None, 256, None, 256, None, 512, None, 0, 25, 512, 256, None, 512, None) == 0
    assert lib.gs_pool2_dgrad_t(None, 256, None, 256, None, 512, None, 512, None, 0, 25, 512, 256, None, 512, None) == 0
    assert "gs_pool2_dgrad" in _lib.EXPORTED_SYMBOLS and "gs_pool2_dgrad_t" in _lib.EXPORTED_SYMBOLS
