"""-m gpu: the K loops of the two tiled three-piece contractions at the shapes where their stage kinds change.

sage_tiled3_fwd_kernel (gs_sage_dense_fwd_tiled3 / _means) runs STEADY rings of four 16-k stages -- no select, no clamp, requests
by pointer increments -- while every request of a ring lies wholly inside K (the first ring: K >= 160), then CAREFUL stages with
selects and clamped addresses, and it ends behind its last real stage instead of padding the loop to whole rings with stages of
zeros.  K here covers 1 .. 13 stages, every ring remainder, last stages with 16 valid k and with one, and K = 160 / 176 / 208 with
a steady ring in front of 6 / 7 / 9 careful stages.  wgrad_tiled3_acut_kernel (gs_dense_wgrad_grouped_tiled3, form 1) against the
first form on reduction lengths around its stage and ring edges.

Every operand lies in a buffer with NaN in its pad columns and a NaN guard row immediately behind its last row: a request
beyond K or beyond the last row shows up as a non-finite output."""
import ctypes

import numpy as np
import pytest
import torch

from graphsage_amd import _lib, ops
from graphsage_amd.ops import Mat, round_up
import gemm_oracle as go
from test_gemm_edges_gpu import Slabs, _wgrad_problem

pytestmark = pytest.mark.gpu

KS = [7, 16, 17, 48, 64, 65, 96, 100, 112, 113, 128, 160, 176, 208]
N_TABLE, N_MAX, OUT_MAX = 200, 130, 128


def _guarded(a, dev, ld_multiple):
    """Mat over the rows of `a` in a buffer of one more row: NaN in every pad column and in the guard row."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    rows, d = a.shape
    ld = round_up(d, ld_multiple)
    buf = torch.full((rows + 1, ld), float("nan"), dtype=torch.float32, device=dev)
    buf[:rows, :d].copy_(torch.from_numpy(a))
    return Mat(buf[:rows], d)


_OPERANDS = {}


def _operands(K):
    """Per K, once: table, ids (the table's last row among them), neighbor means, both weights, bias, all at the largest n / out."""
    if K not in _OPERANDS:
        rng = np.random.default_rng(1000 + K)
        X = rng.normal(size=(N_TABLE, K)).astype(np.float32)
        ids = rng.integers(0, N_TABLE, size=1000).astype(np.int32)
        ids[::7] = N_TABLE - 1
        ids[0] = N_TABLE - 1
        mean = rng.normal(size=(1000, K)).astype(np.float32)
        Ws = (rng.normal(size=(K, OUT_MAX)) * 0.1).astype(np.float32)
        Wn = (rng.normal(size=(K, OUT_MAX)) * 0.1).astype(np.float32)
        b = (rng.normal(size=(2 * OUT_MAX,)) * 0.1).astype(np.float32)
        _OPERANDS.clear()                                   # (one K at a time: the cases of a K run back to back)
        _OPERANDS[K] = (X, ids, mean, Ws, Wn, b)
    return _OPERANDS[K]


def _check_fwd(got, self_m, mean, Ws, Wn, b, two, relu, tag):
    """The bound of test_split_gemm_gpu.test_sage_dense_fwd_tiled3: against fp64, relative to the rms of the pre-activation, at most
    4 x the error of a float32 NumPy product (or 4e-7), and below 4e-6."""
    assert np.isfinite(got).all(), tag
    want_n = mean.astype(np.float64) @ Wn.astype(np.float64)
    want = np.concatenate([self_m.astype(np.float64) @ Ws.astype(np.float64), want_n], axis=1) if two else want_n
    want = want + b
    pre = want.copy()
    f32 = np.concatenate([self_m @ Ws, mean @ Wn], axis=1) if two else mean @ Wn
    f32 = f32 + b
    if relu:
        want, f32 = np.maximum(want, 0), np.maximum(f32, 0)
    rms = np.sqrt((pre * pre).mean())
    err = np.abs(got.astype(np.float64) - want).max() / rms
    err32 = np.abs(f32.astype(np.float64) - want).max() / rms
    print("%s: err %.3g err32 %.3g" % (tag, err, err32))
    assert err <= max(4 * err32, 4e-7), (tag, err, err32)
    assert err < 4e-6, (tag, err)


@pytest.mark.parametrize("K", KS)
def test_fwd_tiled3_stage_kinds(dev, K):
    """gs_sage_dense_fwd_tiled3 at n = 1 / 65 / 130, out = 8 / 128, one and two terms, gathered self rows."""
    X, ids, mean, Ws, Wn, b = _operands(K)
    Xd = _guarded(X, dev, 32)                               # the table: ld a multiple of 32
    for n in (1, 65, N_MAX):
        md = _guarded(mean[:n], dev, 4)                     # the means: ld = round_up(K, 4) only
        sid = ids[:n].copy()
        sid[n // 2] = N_TABLE - 1
        sid_d = torch.from_numpy(sid).to(dev)
        for out in (8, OUT_MAX):
            Wsd, Wnd = _guarded(Ws[:, :out], dev, 4), _guarded(Wn[:, :out], dev, 4)
            for two in (False, True):
                bias = np.concatenate([b[:out], b[OUT_MAX:OUT_MAX + out]]) if two else b[:out]
                bd = torch.from_numpy(np.ascontiguousarray(bias)).to(dev)
                relu = out == OUT_MAX
                act = ops.ACT_RELU if relu else ops.ACT_IDENTITY
                outs = []
                for rep in range(2):
                    o = Mat.zeros(n, (2 if two else 1) * out, dev)
                    o.buf.fill_(float("nan"))
                    if two:
                        ops.sage_dense_fwd_tiled3(Xd, sid_d, md, n, Wsd, Wnd, out, act, bd, o, [])
                    else:
                        ops.sage_dense_fwd_tiled3(None, None, md, n, None, Wnd, out, act, bd, o, [])
                    torch.cuda.synchronize()
                    outs.append(o.numpy())
                tag = "K=%d n=%d out=%d terms=%d" % (K, n, out, 2 if two else 1)
                assert np.array_equal(outs[0], outs[1]), tag           # bit-identical reruns
                _check_fwd(outs[0], X[sid], mean[:n], Ws[:, :out], Wn[:, :out], bias, two, relu, tag)


@pytest.mark.parametrize("K", KS)
def test_fwd_tiled3_means_stage_kinds(dev, K):
    """gs_sage_dense_fwd_tiled3_means at (n_roots, s) = (7, 10), (70, 10), (13, 3): the output under the same bound; the layer-1
    means are, bit for bit, the float32 expression of the kernel's epilogue on that output (zero start, rows j = 0 .. s - 1 added in
    order, one multiply by 1 / s)."""
    X, ids, mean, Ws, Wn, b = _operands(K)
    Xd = _guarded(X, dev, 32)
    out = OUT_MAX
    Wsd, Wnd = _guarded(Ws, dev, 4), _guarded(Wn, dev, 4)
    bd = torch.from_numpy(b).to(dev)
    for n_roots, s in ((7, 10), (70, 10), (13, 3)):
        n = n_roots * (1 + s)
        md = _guarded(mean[:n], dev, 4)
        sid = ids[:n].copy()
        sid[n - 1] = N_TABLE - 1
        sid_d = torch.from_numpy(sid).to(dev)
        res = []
        for rep in range(2):
            o, l1 = Mat.zeros(n, 2 * out, dev), Mat.zeros(n_roots, 2 * out, dev)
            o.buf.fill_(float("nan"))
            l1.buf.fill_(float("nan"))
            ops.sage_dense_fwd_tiled3_means(Xd, sid_d, md, n, Wsd, Wnd, out, ops.ACT_RELU, bd, o, n_roots, s, l1, [])
            torch.cuda.synchronize()
            res.append((o.numpy(), l1.numpy()))
        tag = "means K=%d roots=%d s=%d" % (K, n_roots, s)
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]), tag
        got, got_means = res[0]
        _check_fwd(got, X[sid], mean[:n], Ws, Wn, b, True, True, tag)
        assert np.isfinite(got_means).all(), tag
        hop = got[n_roots:].reshape(n_roots, s, 2 * out)
        v = np.zeros((n_roots, 2 * out), np.float32)
        for j in range(s):
            v = v + hop[:, j]
        v = v * (np.float32(1.0) / np.float32(s))
        assert np.array_equal(got_means, v), tag


@pytest.fixture
def _library_default_afterwards():
    yield
    _lib.set_wgrad_tiled3_form(_lib.WGRAD_TILED3_FORM_DEFAULT)


def _wgrad_launch(dev, prob, shape, form):
    """The problem through gs_dense_wgrad_grouped_tiled3 in the given form into fresh slabs -> [n_slabs, d, out] (guards checked)."""
    n, d, out, col0, n_slabs = shape
    A, idx_d, Z, _, _, _ = prob
    sl = Slabs(dev, n_slabs, d, out)
    arr = (_lib.WgradDesc * 1)()
    q = arr[0]
    q.A, q.a_idx, q.dZ, q.slabs = A.ptr, ops.ptr(idx_d), Z.ptr, sl.ptr
    q.lda, q.ldz, q.ld_slab, q.n, q.d, q.col0, q.out_dim, q.n_slabs = A.ld, Z.ld, sl.ld, n, d, col0, out, n_slabs
    q.a_rows = A.t.shape[0] - 1
    jn = (_lib.GatherDesc * 1)()
    _lib.set_wgrad_tiled3_form(form)
    ops.call("gs_dense_wgrad_grouped_tiled3", ctypes.addressof(arr), 1, ctypes.addressof(jn), 0, ops.current_stream())
    torch.cuda.synchronize()
    raw = sl.t.cpu().numpy()
    assert np.all(raw[:sl.guard] == go.SENTINEL) and np.all(raw[-sl.guard:] == go.SENTINEL), "wrote outside the slabs"
    body = raw[sl.guard:-sl.guard].reshape(n_slabs, d, sl.ld)
    assert np.all(body[:, :, out:] == go.SENTINEL), "wrote beyond the logical columns of a slab row"
    return body[:, :, :out]


@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("n", [16, 17, 100, 512, 513, 1040])
def test_wgrad_tiled3_forms_stage_kinds(dev, _library_default_afterwards, n, gathered):
    """Reduction lengths of one whole stage, one stage + one row, 6 stages + 4 rows, whole rings (512), whole rings + one row, and
    more than one 1024-row slice can hold (1040: two and three slices); d = 7 / 64 / 70 (a nearly empty, a whole, two m tiles), out =
    8 / 128, col0 = 0 / 128, one to three slabs.  Form 1 must equal form 0 element for element; both within 1e-5 of the rms of
    the fp64 product (the bound of test_dense_wgrad_grouped_tiled3_shapes)."""
    rng = np.random.default_rng(7 * n + gathered)
    combo = 0
    for d in (7, 64, 70):
        for out in (8, 128):
            for col0 in (0, 128):
                n_slabs = combo % 3 + 1
                if n > 1024:
                    n_slabs = 2 + combo % 2                  # (a slice holds at most 1024 rows)
                combo += 1
                shape = (n, d, out, col0, n_slabs)
                prob = _wgrad_problem(dev, rng, n, d, out, col0, n_slabs, gathered)
                if gathered:                                  # the ids reach the table's last row too
                    A, idx_d, _, _, A_rows, _ = prob
                    last = A.t.shape[0] - 2                   # (In appends one NaN row)
                    if not bool((idx_d == last).any()):       # no id drew it: a live row there with the values of the one it
                        A.t[last, :d] = A.t[int(idx_d[n // 2]), :d].clone()       # replaces, so A_rows stays the logical operand
                        idx_d[n // 2] = last
                first = _wgrad_launch(dev, prob, shape, 0)
                second = _wgrad_launch(dev, prob, shape, 1)
                tag = "n=%d d=%d out=%d col0=%d slabs=%d gathered=%d" % (shape + (gathered,))
                assert np.isfinite(first).all() and np.isfinite(second).all(), tag
                assert np.array_equal(second, first), tag
                want = prob[4].astype(np.float64).T @ prob[5].astype(np.float64)
                rms = np.sqrt((want * want).mean()) + 1e-30
                for name, got in (("first", first), ("second", second)):
                    err = np.abs(got.astype(np.float64).sum(axis=0) - want).max() / rms
                    assert err < 1e-5, (tag, name, err)
