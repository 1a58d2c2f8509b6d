"""-m gpu: the small float4 / row-per-wave kernels that run in every backward pass (gs_mean_bwd, gs_act_bwd,
gs_input_grad_pull, gs_segment_max_fwd / _bwd, gs_l2norm_fwd / _bwd, gs_class_loss) at ragged shapes, one sweep per kernel.

Widths d in {1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 602} (one lane, a partial float4, exactly / just over one wave of columns or
float4, Reddit's 602), ld in {round_up(d, 4), round_up(d, 4) + 8}; rows n in {1, 3, 4, 5, 257} (the row-per-wave kernels pack
4 rows per workgroup); group sizes s in {1, 2, 25, 70}.  In every case
  * each output lives in a larger sentinel-filled buffer, two rows down, and the kernel gets a row-sliced Mat: rows outside the
    view and columns >= round_up(d, 4) keep the sentinel, columns [d, round_up(d, 4)) are exact zeros;
  * every input holds NaN in its columns [d, ld): the kernels' masks are selects, nothing may leak.
Copies, selects and maxima are bit-equal to NumPy in fp32; the summing / transcendental kernels are held to the bounds derived
in tests/optim_oracle.py from the operations as written (the numbers are in each docstring).  One past-the-cap case per
grid-capped kernel at d = 5 (two float4 per row), compared on the whole output."""
import numpy as np
import pytest
import torch

from graphsage_amd import _lib, ops
from graphsage_amd.ops import Mat
import optim_oracle as oo

pytestmark = pytest.mark.gpu
S = oo.SENTINEL
MAX_ROWS = max(oo.ROWS) * max(oo.GROUPS)
_base = {}


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sync():
    torch.cuda.synchronize()


def rand(seed, rows, d):
    """[rows, d] fp32 standard normals: the first rows of one stream per (seed, d), whatever `rows` is (a sweep first asks for
    its largest shape, so the stream is drawn once per width)."""
    key = (seed, d)
    if any(k[1] != d for k in _base):
        _base.clear()                                            # one width at a time
    if key not in _base or _base[key].shape[0] < rows:
        _base[key] = np.random.RandomState(1000 * seed + d).standard_normal((rows, d)).astype(np.float32)
    return _base[key][:rows]


def inp(a, ld, dev, pad=np.nan):
    """[n, d] -> Mat with leading dimension ld, the pad columns NaN."""
    a = np.asarray(a, np.float32)
    buf = np.full((a.shape[0], ld), pad, np.float32)
    buf[:, :a.shape[1]] = a
    return Mat(_dev(buf, dev), a.shape[1])


class Out(object):
    """[n, d] output two rows down a sentinel-filled [n + 4, ld] buffer."""

    def __init__(self, dev, n, d, ld, prefill=None, dtype=np.float32, sentinel=S):
        a = np.full((n + 4, ld), sentinel, dtype)
        if prefill is not None:
            a[2:2 + n, :d] = prefill
        self.big, self.n, self.d, self.sentinel = _dev(a, dev), n, d, sentinel
        self.view = self.big[2:2 + n]
        self.mat = Mat(self.view, d) if dtype == np.float32 else None

    def read(self, tag, d4=None):
        _sync()
        n, d = self.n, self.d
        d4 = (d + 3) // 4 * 4 if d4 is None else d4
        got = self.big.cpu().numpy()
        assert np.all(got[:2] == self.sentinel) and np.all(got[2 + n:] == self.sentinel), "%s: rows outside the view were written" % (tag,)
        assert np.all(got[:, d4:] == self.sentinel), "%s: columns beyond round_up(d, 4) were written" % (tag,)
        assert np.all(got[2:2 + n, d:d4] == 0), "%s: the pad columns of the last float4 must be exact zeros" % (tag,)
        return got[2:2 + n, :d]


# ----------------------------------------------------------------------------------------------- gs_mean_bwd
def _mean_bwd_case(dev, n, s, d, ld, use_mask, accumulate, tag):
    scale = 0.37                                                                  # not 1 / s
    dm, y = rand(1, n, d), rand(2, n * s, d)
    prev = rand(3, n * s, d) if accumulate else None
    out = Out(dev, n * s, d, ld, prefill=prev)
    ops.mean_bwd(inp(dm, ld, dev), n, s, scale, out.mat, mask_y=inp(y, ld, dev) if use_mask else None, accumulate=bool(accumulate))
    got = out.read(tag)
    want = oo.mean_bwd(dm, s, scale, y if use_mask else None)
    if not accumulate:
        assert np.array_equal(got, want), tag
    else:
        a = prev + want                                           # fp32: product, then add; the kernel may contract them into an fma,
        ulp = np.spacing(np.maximum(np.abs(prev), np.abs(want)))  # which skips the product's rounding: 1 ulp of the larger operand
        assert np.all(np.abs(got.astype(np.float64) - a) <= ulp), tag


@pytest.mark.parametrize("d", oo.WIDTHS)
def test_mean_bwd_sweep(dev, d):
    """gs_mean_bwd == repeat(dm * fp32(scale)) under the relu mask, scale = 0.37: bit-equal without accumulate; with it, within
    1 ulp (of the larger operand: where the two cancel, the product's own rounding is many ulps of the small sum) of the fp32
    prev + that (fma contraction of scale * x + prev, as test_input_grad_pull notes); with and without mask_y."""
    for seed in (1, 2, 3):
        rand(seed, MAX_ROWS, d)
    for ld in oo.lds(d):
        for n in oo.ROWS:
            for s in oo.GROUPS:
                for use_mask in (0, 1):
                    for acc in (0, 1):
                        _mean_bwd_case(dev, n, s, d, ld, use_mask, acc, "mean_bwd d=%d ld=%d n=%d s=%d mask=%d acc=%d" % (d, ld, n, s, use_mask, acc))


@pytest.mark.parametrize("accumulate", [0, 1])
def test_mean_bwd_past_the_grid_cap(dev, accumulate):
    cap = 2048 * 256                     # gs_gather.hip gs_mean_bwd: at most 2048 blocks of 256 threads, one float4 each
    n, s = oo.CAP_MEAN_BWD
    assert n * s * 2 > cap
    _mean_bwd_case(dev, n, s, oo.CAP_D, 8, 1, accumulate, "mean_bwd past the cap acc=%d" % accumulate)


# ----------------------------------------------------------------------------------------------- gs_act_bwd
def _act_bwd_case(dev, n, d, ld, tag):
    dY, Y = rand(4, n, d), rand(5, n, d)
    for act, Ym, want in ((ops.ACT_RELU, inp(Y, ld, dev), np.where(Y > 0, dY, np.float32(0))), (ops.ACT_IDENTITY, None, dY)):
        out = Out(dev, n, d, ld)
        ops.act_bwd(inp(dY, ld, dev), Ym, n, d, act, out.mat)
        assert np.array_equal(out.read(tag), want), (tag, act)


@pytest.mark.parametrize("d", oo.WIDTHS)
def test_act_bwd_sweep(dev, d):
    """gs_act_bwd: relu (dY where Y > 0) and identity with Y = None (a copy), bit-equal."""
    for ld in oo.lds(d):
        for n in oo.ROWS:
            _act_bwd_case(dev, n, d, ld, "act_bwd d=%d ld=%d n=%d" % (d, ld, n))


def test_act_bwd_past_the_grid_cap(dev):
    cap = 2048 * 256                     # gs_gemm.hip gs_act_bwd: at most 2048 blocks of 256 threads, one float4 each
    assert oo.CAP_ACT_BWD * 2 > cap
    _act_bwd_case(dev, oo.CAP_ACT_BWD, oo.CAP_D, 8, "act_bwd past the cap")


# ----------------------------------------------------------------------------------------------- gs_input_grad_pull
def _pull(dev, rows, d, ld, d_self, n_self, segments, y, tag):
    out = Out(dev, rows, d, ld)
    segs = [(inp(src, ld, dev), row0, n, s, scale) for src, row0, n, s, scale in segments]
    ops.input_grad_pull(out.mat, rows, d, d_self=inp(d_self, ld, dev) if d_self is not None else None, n_self=n_self,
                        segments=segs, mask_y=inp(y, ld, dev) if y is not None else None)
    got = out.read(tag)
    want, bound = oo.input_grad_pull(rows, d, d_self, n_self, segments, y)
    oo.check("input_grad_pull", "out", got, want, bound)
    return got, want


def _pull_cases(dev, B, d, ld):
    s2, s1 = 3, 5
    n_self = B + B * s2
    rows = n_self + B * s2 * s1
    d_self, dm, y = rand(6, n_self, d), rand(7, n_self, d), rand(8, rows + 5, d)
    tag = "input_grad_pull d=%d ld=%d B=%d " % (d, ld, B)
    # the three-layer shape: the rows of the middle hop are self rows AND neighbor rows
    three = [(dm[:B], B, B, s2, 1.0 / s2), (dm[B:], n_self, B * s2, s1, 1.0 / s1)]
    _pull(dev, rows, d, ld, d_self, n_self, three, y[:rows], tag + "three-layer")
    _pull(dev, rows, d, ld, d_self, n_self, three, None, tag + "three-layer, no mask")
    # no d_self, a segment from row 0, two rows covered by nothing between the segments and three behind them: exact zeros
    gap = [(dm[:B], 0, B, s2, 0.37), (dm[B:], B * s2 + 2, B * s2, s1, 1.0 / s1)]
    rows_g = B * s2 + 2 + B * s2 * s1 + 3
    got, _ = _pull(dev, rows_g, d, ld, None, 0, gap, None, tag + "no d_self, gaps")
    assert np.all(got[B * s2:B * s2 + 2] == 0) and np.all(got[rows_g - 3:] == 0), tag + "rows covered by nothing must be zero"
    _pull(dev, rows_g, d, ld, None, 0, gap, y[:rows_g], tag + "no d_self, gaps, mask")
    # GS_PULL_MAX segments, neighbours overlapping by half, over self rows
    assert _lib.GS_PULL_MAX == 6
    six = [(dm[k * B:(k + 1) * B] if (k + 1) * B <= n_self else dm[:B], k * B, B, 2, 0.1 * (k + 1)) for k in range(6)]
    _pull(dev, 7 * B + 1, d, ld, d_self[:B], B, six, y[:7 * B + 1], tag + "n_seg = GS_PULL_MAX")


@pytest.mark.parametrize("d", oo.WIDTHS)
def test_input_grad_pull_sweep(dev, d):
    """gs_input_grad_pull against oo.input_grad_pull: the three-layer shape of test_input_grad_pull at ragged d (B in the row
    counts), without d_self, a segment that starts at row 0, rows covered by nothing (exact zeros), n_seg = GS_PULL_MAX with
    overlapping segments.  Bound per element: one rounding per product scale * src and one per add after the first term, times
    the terms' magnitudes: 0 for a copied self row (bit-equal), 1 u for a single segment, at most 4 u = 2.4e-7 (a self row under two segments)."""
    for ld in oo.lds(d):
        for B in oo.ROWS:
            _pull_cases(dev, B, d, ld)


def test_input_grad_pull_past_the_grid_cap(dev):
    cap = 4096 * 256                     # gs_gather.hip gs_input_grad_pull: at most 4096 blocks of 256 threads, one float4 each
    rows, d = oo.CAP_PULL_ROWS, oo.CAP_D
    assert rows * 2 > cap
    n = (rows - 1) // 2
    src, d_self, y = rand(9, n, d), rand(10, 1000, d), rand(11, rows, d)
    got, want = _pull(dev, rows, d, 8, d_self, 1000, [(src, 1, n, 2, 0.5)], y, "input_grad_pull past the cap")
    assert np.array_equal(got[0], np.where(y[0] > 0, d_self[0], np.float32(0)))


# ----------------------------------------------------------------------------------------------- gs_segment_max_fwd / _bwd
def _segmax_inputs(n, s, d):
    """Half-integer values (exact ties: the first index must win), relu'd groups, all-equal groups, groups whose maximum is
    <= 0 (no gradient), plain groups with negative values."""
    H = (np.round(rand(12, n * s, d) * 2) / 2).reshape(n, s, d).copy()
    g = np.arange(n)
    H[g % 3 == 1] = np.maximum(H[g % 3 == 1], 0)
    H[g % 4 == 2] = H[g % 4 == 2][:, :1]
    H[g % 5 == 3] = -np.abs(H[g % 5 == 3])
    return H.reshape(n * s, d).astype(np.float32)


def _segmax_fwd_case(dev, n, s, d, ld, tag):
    H = _segmax_inputs(n, s, d)
    pooled = Out(dev, n, d, ld)
    lda = d + 3
    arg = Out(dev, n, d, lda, dtype=np.int32, sentinel=-99)
    ops.segment_max_fwd(inp(H, ld, dev), n, s, pooled.mat, arg.view)
    want_p, want_a = oo.segment_max_fwd(H, n, s)
    assert np.array_equal(pooled.read(tag), want_p), tag
    assert np.array_equal(arg.read(tag, d4=d), want_a), tag                      # the arg-max has no pad columns: [d, lda) untouched


@pytest.mark.parametrize("d", oo.WIDTHS)
def test_segment_max_fwd_sweep(dev, d):
    """gs_segment_max_fwd: pooled bit-equal to NumPy's fp32 max, arg-max equal to np.argmax (first index on ties); negative
    inputs, relu'd groups, exact ties, all-equal groups, s = 1."""
    rand(12, MAX_ROWS, d)
    for ld in oo.lds(d):
        for n in oo.ROWS:
            for s in oo.GROUPS:
                _segmax_fwd_case(dev, n, s, d, ld, "segment_max_fwd d=%d ld=%d n=%d s=%d" % (d, ld, n, s))


def test_segment_max_fwd_past_the_grid_cap(dev):
    cap = 4096 * 256                     # gs_head.hip gs_segment_max_fwd: at most 4096 blocks of 256 threads, one float4 each
    n, s = oo.CAP_SEGMAX_FWD
    assert n * 2 > cap
    _segmax_fwd_case(dev, n, s, oo.CAP_D, 8, "segment_max_fwd past the cap")


def _segmax_bwd_case(dev, n, s, d, ld, tag):
    H = _segmax_inputs(n, s, d)
    pooled, arg = oo.segment_max_fwd(H, n, s)
    dP = rand(13, n, d)
    lda = d + 3
    arg_pad = np.full((n, lda), -99, np.int32)
    arg_pad[:, :d] = arg
    dH = Out(dev, n * s, d, ld)
    ops.segment_max_bwd(inp(dP, ld, dev), inp(pooled, ld, dev), _dev(arg_pad, dev), n, s, dH.mat)
    want = oo.segment_max_bwd(dP, pooled, arg, n, s)
    assert np.array_equal(dH.read(tag), want), tag
    return pooled, want


@pytest.mark.parametrize("d", oo.WIDTHS)
def test_segment_max_bwd_sweep(dev, d):
    """gs_segment_max_bwd: dP lands on the arg-max row where pooled > 0, zero elsewhere, bit-equal; groups whose maximum is <= 0
    get no gradient."""
    rand(12, MAX_ROWS, d)
    seen_gated = False
    for ld in oo.lds(d):
        for n in oo.ROWS:
            for s in oo.GROUPS:
                pooled, want = _segmax_bwd_case(dev, n, s, d, ld, "segment_max_bwd d=%d ld=%d n=%d s=%d" % (d, ld, n, s))
                seen_gated = seen_gated or bool((pooled <= 0).any())
    assert seen_gated


def test_segment_max_bwd_past_the_grid_cap(dev):
    cap = 8192 * 256                     # gs_head.hip gs_segment_max_bwd: at most 8192 blocks of 256 threads, one float4 each
    n, s = oo.CAP_SEGMAX_BWD
    assert n * s * 2 > cap
    _segmax_bwd_case(dev, n, s, oo.CAP_D, 8, "segment_max_bwd past the cap")


# ----------------------------------------------------------------------------------------------- gs_l2norm_fwd / _bwd
def _l2_fwd(dev, x, n, d, ld, tag):
    y = Out(dev, n, d, ld)
    inv = torch.full((n + 2,), S, dtype=torch.float32, device=dev)
    ops.l2norm_fwd(inp(x, ld, dev), n, y.mat, inv[1:1 + n])
    got_y = y.read(tag)
    got_inv = inv.cpu().numpy()
    assert got_inv[0] == S and got_inv[-1] == S, tag
    return got_y, got_inv[1:1 + n]


@pytest.mark.parametrize("d", oo.WIDTHS)
def test_l2norm_fwd_sweep(dev, d):
    """gs_l2norm_fwd on oo.l2_rows: unit-scale rows, an all-zero row (y = 0, inv = 1e6), sum(x^2) = 1e-12 (1 -+ 2^-10) (just
    clamped / just not) and a row of norm 1e18.  Bounds (x 4, LIB): inv (R_ss / 2 + 2.5) u with R_ss = ceil(d / 64) + 7: 6.5 u at
    d <= 64, 11 u at d = 602, so 4 * 11 u = 2.6e-6 relative; y one rounding more: 2.9e-6 |y|."""
    for ld in oo.lds(d):
        for n in oo.ROWS:
            tag = "l2norm_fwd d=%d ld=%d n=%d" % (d, ld, n)
            x = oo.l2_rows(n, d, d)
            got_y, got_inv = _l2_fwd(dev, x, n, d, ld, tag)
            want_y, want_inv, _, by, binv = oo.l2norm_fwd(x)
            oo.check("l2norm_fwd", "y", got_y, want_y, by)
            oo.check("l2norm_fwd", "inv_norm", got_inv, want_inv, binv)
            assert np.all(got_y[n - 1] == 0), tag + ": the all-zero row"


@pytest.mark.parametrize("d", oo.WIDTHS)
def test_l2norm_bwd_sweep(dev, d):
    """gs_l2norm_bwd on EVERY row, the clamped ones included (dx = dy * inv there, no normalisation term), twice: on the oracle's
    y and inv rounded to fp32, and on the y and inv that gs_l2norm_fwd itself produced (the pair the training step feeds it; a
    forward whose 1 / sqrtf(1e-12f) fell below 1e6 would un-clamp the backward).  The oracle gets the same y and inv and the
    exact sum of squares.  Bound (x 4): (ceil(d / 64) + 10) u inv (|dy| + |y| sum|dy y|): 11 u at d <= 64, 20 u = 1.2e-6 at 602
    (4.8e-6 with LIB); one rounding on a clamped row."""
    for ld in oo.lds(d):
        for n in oo.ROWS:
            tag = "l2norm_bwd d=%d ld=%d n=%d" % (d, ld, n)
            x = oo.l2_rows(n, d, d)
            dy = rand(14, n, d)
            y64, inv64, cache, _, _ = oo.l2norm_fwd(x)
            ss = cache[2][:, 0]
            pairs = {"oracle": (y64.astype(np.float32), inv64.astype(np.float32)), "gpu_fwd": _l2_fwd(dev, x, n, d, ld, tag)}
            for src, (y, inv) in sorted(pairs.items()):
                dx = Out(dev, n, d, ld)
                ops.l2norm_bwd(inp(dy, ld, dev), inp(y, ld, dev), _dev(inv, dev), n, dx.mat)
                got = dx.read(tag + " " + src)
                want, bound = oo.l2norm_bwd(dy, y, inv, ss)
                oo.check("l2norm_bwd", "dx (%s y, inv)" % src, got, want, bound)
            if n >= 2:
                assert ss[n - 2] < 1e-12 and np.array_equal(got[n - 2], dy[n - 2] * inv[n - 2]), tag + ": the just-clamped row"


# ----------------------------------------------------------------------------------------------- gs_class_loss
@pytest.mark.parametrize("sigmoid_loss", [0, 1], ids=["softmax", "sigmoid"])
@pytest.mark.parametrize("C", oo.CLASSES)
def test_class_loss_sweep(dev, C, sigmoid_loss):
    """gs_class_loss row by row: loss_rows (not only their mean), preds, dlogits; logits at scale 3 with planted +-30, +-88, +-200;
    softmax with one-hot, multi-hot (zs != 1) and all-zero label rows, sigmoid with 0/1 labels; with preds = None and with
    dlogits = None.  Everything finite.  Bounds (oo.class_loss, x 4): sigmoid loss (ceil(C / 64) + 11) u mean(|max(x, 0)| + |x z| +
    softplus): 14 u, 3.3e-6 of the terms; p (4 * 3 + |x| (1 - p)) u: 42 u = 2.5e-6 p at x = -30, where expf's argument-proportional error
    (oo.class_loss) was seen at 14.7 u; softmax p_c (|x_c - m| + ceil(C / 64) + 10 + ...) u p_c: the rounding
    of x_c - m enters the exponent, ~ 110 u = 2.6e-5 p_c at x_c - m = -88 (p_c ~ 1e-38) and 13 u at the row's maximum; softmax
    loss ~ (zs (E_se + |log se| + 2 |lse|) + R |z x| + ...) u: 1.2e-5 * 4 at |x| = 200, where zs * lse - zx cancels; all + 2^-149."""
    sig = bool(sigmoid_loss)
    for ld in oo.lds(C):
        for n in oo.ROWS:
            tag = "class_loss C=%d ld=%d n=%d sigmoid=%d" % (C, ld, n, sigmoid_loss)
            x, z = oo.class_inputs(n, C, sig, C)
            r = oo.class_loss(x, z, sig)
            for want_p, want_d in ((1, 1), (0, 1), (1, 0)):
                lr = torch.full((n + 2,), S, dtype=torch.float32, device=dev)
                pr, dl = Out(dev, n, C, ld), Out(dev, n, C, ld)
                ops.class_loss(inp(x, ld, dev), inp(z, ld, dev), n, C, sig, lr[1:1 + n], pr.mat if want_p else None,
                               dl.mat if want_d else None)
                _sync()
                got_l = lr.cpu().numpy()
                assert got_l[0] == S and got_l[-1] == S, tag
                oo.check("class_loss", "loss_rows (%s)" % ("sigmoid" if sig else "softmax"), got_l[1:1 + n], r["loss"], r["b_loss"])
                if want_p:
                    oo.check("class_loss", "preds (%s)" % ("sigmoid" if sig else "softmax"), pr.read(tag), r["preds"], r["b_preds"])
                else:
                    assert np.all(pr.big.cpu().numpy() == S), tag + ": preds = None must write nothing"
                if want_d:
                    oo.check("class_loss", "dlogits (%s)" % ("sigmoid" if sig else "softmax"), dl.read(tag), r["dlogits"], r["b_dlogits"])
                else:
                    assert np.all(dl.big.cpu().numpy() == S), tag + ": dlogits = None must write nothing"
