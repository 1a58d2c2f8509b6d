"""-m gpu: the fp32 MFMA contractions of csrc/gs_gemm.hip against float64, per tile variant, at the edges of each variant.

Every case
  * reads its operands from buffers with a leading dimension beyond round_up(width, 4) (one tight case per entry point), in which
    EVERYTHING outside the logical operand is NaN: pad columns, the columns outside [col0, col0 + out_dim), table rows that no
    index points at, the row after the last one (the K tail of a transposed operand);
  * writes into a sentinel-filled buffer with two spare rows above, three below and spare columns: afterwards the logical block
    is inside gemm_oracle's derived bound (the only tolerance here), columns [N, round_up(N, 4)) are exact zeros where the kernel
    promises that (every non-split-K form), and every other word still holds the sentinel.
tests/test_gemm_oracle.py shows on the CPU that this bound passes the kernels' arithmetic and fails each planted fault.

Instantiation -> cases (variants are forced by shape only; `variant()` below restates dispatch_gemm):
  gemm_small_kernel<NN>, <NT>              test_gemm_small_sweep (M 1..2048, N {1,4,33,36}, K 1..389), test_gemm_row_gather_kc,
                                           test_sage_dense_fwd (n <= 2048: two terms, concat / add), test_dense_dgrad /
                                           test_sage_dense_dgrad (n <= 2048: NT, accumulate, col0)
  gemm_f32_mfma_kernel<64,64,NN>, <..,NT>  test_gemm_t64_sweep (tA = 0, M {2049, 2113}), test_sage_dense_fwd (n > 2048),
                                           test_dense_fwd_rows_dev (device-side row count), test_dense_dgrad /
                                           test_sage_dense_dgrad (n > 2048), test_dense_pool_max_fwd_t64 (pool epilogue)
  gemm_f32_mfma_kernel<64,64,TN>, <..,TT>  test_gemm_t64_sweep (tA = 1, M {1,63,65,100}), test_gemm_tn_gather_refill (index cache across
                                           1024 k without split-K), test_dense_wgrad (split-K slabs, gathered / contiguous)
  gemm_f32_mfma_kernel<128,128,*>          test_gemm_t128 (all four layouts: M 65409, N {129,132}, K {37,97}, A_KC row gather),
                                           test_dense_wgrad (TN split-K: (16385,130,132,0,3), (16384,128,128,4,1)),
                                           test_dense_pool_max_fwd_t128 (NN, pool epilogue), test_dense_fwd_rows_dev_t128
  gemm_grouped_tn_kernel, .._cogather_..   test_dense_wgrad_grouped (13 problems: two launches; gather jobs on the last)
  sage_dense_cogather_kernel               test_sage_dense_fwd_cogather (n > 2048; n <= 2048 takes the separate launches)
Each of them meets an M tail, an N tail with N % 4 == 0 (the float4 LDS epilogue's row / column guard: 68, 132) and one with
N % 4 != 0 (the per-element epilogue and its pad-column zeroing), and a K tail.

Long reductions (gs_dense_wgrad from 4096 rows: the 128x128 split-K cases) take a row-sparse dZ whose live rows include every slab's
first and last rows, the rows around each refill of the index cache and the last row (gemm_oracle.wgrad_dz): with dense unit operands
the bound at n = 16384 is about 10 per element and would hide a lost or foreign product; sparse, it is about 0.2 and each slab is held
to its own slice.  What stays unseen there: a fault confined to rows whose dZ is zero (63 of 64 away from the edges).

Every test prints the largest err / bound it met per variant (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

from graphsage_amd import _lib, ops
from graphsage_amd.ops import round_up
import gemm_oracle as go

pytestmark = pytest.mark.gpu
S, IS = go.SENTINEL, go.ISENTINEL
NAN = np.float32("nan")
ID, RELU = ops.ACT_IDENTITY, ops.ACT_RELU
WORST = {}


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _st():
    return ops.current_stream()


def _note(variant, r):
    WORST[variant] = max(WORST.get(variant, 0.0), r)


@pytest.fixture(autouse=True)
def _print_worst():
    """Prints the largest err / bound per variant that the test met (pytest -s); a figure, not a check."""
    WORST.clear()
    yield
    for k in sorted(WORST):
        print("\nworst err/bound %-24s %.4f" % (k, WORST[k]), end="")


def cdiv(a, b):
    return -(-a // b)


def variant(a_kc, b_kc, M, N, halves=1, nz=1, split=False):
    """dispatch_gemm (gs_gemm.hip) restated: which kernel a shape runs."""
    lay = ("N" if a_kc else "T") + ("T" if b_kc else "N")
    if a_kc and not split and M <= 2048:
        return "small_" + lay
    return ("t128_" if cdiv(M, 128) * cdiv(N, 128) * halves * nz >= 1024 else "t64_") + lay


class In(object):
    """A logical [rows, w] operand at columns [col0, col0 + w) of a [rows + 1, ld] buffer; everything else is `fill` (NaN, or an
    array of live finite data for the cases that model a cols_slice of a wider matrix).  tight: ld = round_up(col0 + w, 4)."""

    def __init__(self, a, dev, col0=0, tight=False, fill=NAN, ld=None):
        a = np.asarray(a, np.float32)
        if a.ndim == 1:
            a = a[None, :]
        rows, w = a.shape
        self.ld = ld if ld is not None else round_up(col0 + w, 4) + (0 if tight else 12)
        buf = np.empty((rows + 1, self.ld), np.float32)
        buf[...] = fill
        buf[:rows, col0:col0 + w] = a
        self.t = _dev(buf, dev)
        self.ptr = self.t.data_ptr()


class Out(object):
    """A [rows, n] output two rows down a sentinel-filled [rows + 5, ld] buffer (ld = round_up(n, 4) + 12; tight: + 0)."""

    def __init__(self, dev, rows, n, prefill=None, tight=False, dtype=np.float32, ld=None):
        self.rows, self.n, self.sent = rows, n, (S if dtype == np.float32 else IS)
        self.ld = ld if ld is not None else round_up(n, 4) + (0 if tight else 12)
        a = np.full((rows + 5, self.ld), self.sent, dtype)
        if prefill is not None:
            a[2:2 + rows, :n] = prefill
        self.t = _dev(a, dev)
        self.ptr = self.t.data_ptr() + 2 * self.ld * 4

    def read(self, tag, rows_written=None, pad_zero=True):
        """The written block [rows_written, n] after checking that nothing else changed."""
        torch.cuda.synchronize()
        rw = self.rows if rows_written is None else rows_written
        got = self.t.cpu().numpy()
        n4 = round_up(self.n, 4) if pad_zero else self.n
        for part in (got[:2], got[2 + rw:], got[2:2 + rw, n4:]):
            assert np.all(part == self.sent), "%s: %d words outside the output block were written" % (
                tag, int((part != self.sent).sum()))
        assert np.all(got[2:2 + rw, self.n:n4] == 0), "%s: pad columns [N, round_up(N, 4)) must be exact zeros" % tag
        return got[2:2 + rw, :self.n]

    def untouched(self, tag):
        torch.cuda.synchronize()
        assert np.all(self.t.cpu().numpy() == self.sent), "%s: a refused / empty call wrote its output" % tag


def _bias(b, dev):
    """bias with NaN on both sides -> (tensor keeping it alive, pointer) or (None, None)."""
    if b is None:
        return None, None
    t = _dev(np.concatenate([np.full(4, NAN, np.float32), np.asarray(b, np.float32), np.full(4, NAN, np.float32)]), dev)
    return t, t.data_ptr() + 16


def _table(rng, rows_logical, width, n_table):
    """(table with NaN in every row that no index points at, idx [rows_logical] with repeats and out of order, the gathered rows)."""
    tab = go.asym(rng, (n_table, width))
    idx = rng.integers(0, n_table, size=rows_logical).astype(np.int32)
    if rows_logical >= 3:
        idx[-1] = idx[1]                      # a repeat even where the draw had none ...
        if idx[0] == idx[1]:
            idx[0] = (idx[1] + 1) % n_table   # ... that differs from the first id (K = 1025: the one index of the second cache fill)
    dead = np.ones(n_table, bool)
    dead[idx] = False
    poisoned = tab.copy()
    poisoned[dead] = NAN
    return poisoned, idx, tab[idx]


COMBOS = [(False, ID), (True, ID), (False, RELU), (True, RELU)]


# ============================================================================================================ gs_gemm_f32
def _gemm_launches(dev, tA, tB, M, N, K, Ain, a_idx, B, zmk, bias, tight=False):
    Bin = In(B.T if tB else B, dev, tight=tight)
    kind = variant(not tA, bool(tB), M, N)
    for use_bias, act in COMBOS:
        bt, bp = _bias(bias if use_bias else None, dev)
        C = Out(dev, M, N, tight=tight)
        ops.call("gs_gemm_f32", tA, tB, M, N, K, Ain.ptr, Ain.ld, ops.ptr(a_idx), Bin.ptr, Bin.ld, bp, act, C.ptr, C.ld, _st())
        t = "%s gemm tA=%d tB=%d M=%d N=%d K=%d bias=%d act=%d" % (kind, tA, tB, M, N, K, use_bias, act)
        want, bound = go.product([zmk], bias=bias if use_bias else None, relu=(act == RELU))
        _note(kind, go.assert_within(C.read(t), want, bound, t))


def _gemm_shape(dev, tAs, M, N, K, tight=False):
    rng = np.random.default_rng(M * 1000003 + N * 1009 + K)
    A, B, bias = go.asym(rng, (M, K)), go.asym(rng, (K, N)), go.asym(rng, (N,))
    zmk = go.contract(A, B)
    for tA in tAs:
        Ain = In(A.T if tA else A, dev, tight=tight)
        for tB in (0, 1):
            _gemm_launches(dev, tA, tB, M, N, K, Ain, None, B, zmk, bias, tight)


@pytest.mark.parametrize("N", [1, 4, 33, 36])
@pytest.mark.parametrize("M", [1, 31, 33, 2048])
def test_gemm_small_sweep(dev, M, N):
    """gemm_small_kernel<NN / NT>: K in {1, 3, 32, 33, 127, 129, 300, 389} gives a wave 0, 1, 2 and >= 3 of the 32-k stages."""
    for K in (1, 3, 32, 33, 127, 129, 300, 389):
        assert variant(True, False, M, N) == "small_NN"
        _gemm_shape(dev, (0,), M, N, K, tight=(N == 36 and K == 33))


@pytest.mark.parametrize("N", [1, 7, 60, 64, 68, 130])
@pytest.mark.parametrize("tA,M", [(1, 1), (1, 63), (1, 65), (1, 100), (0, 2049), (0, 2113)])
def test_gemm_t64_sweep(dev, tA, M, N):
    """gemm_f32_mfma_kernel<64,64,*>: K in {1..161} takes every branch of the two-stage pipeline (one stage, two, the prefetch of a
    third and fourth, a second trip round the loop, with and without a k tail); N in {60, 68} x an M tail is the float4 LDS
    epilogue's row / column guard, N in {1, 7, 130} the per-element epilogue."""
    for K in (1, 31, 32, 33, 64, 65, 96, 97, 129, 161):
        assert variant(not tA, False, M, N).startswith("t64_")
        _gemm_shape(dev, (tA,), M, N, K, tight=(N == 68 and K == 33))


@pytest.mark.parametrize("tA", [0, 1])
@pytest.mark.parametrize("N,K", [(129, 37), (129, 97), (132, 37), (132, 97)])
def test_gemm_t128(dev, N, K, tA):
    """gemm_f32_mfma_kernel<128,128,*>, all four layouts: M = 511 * 128 + 1 is the smallest row count that reaches 1024 big tiles
    with two column tiles, and leaves one row in the last tile."""
    M = 65409
    assert variant(True, False, M, N) == "t128_NN" and variant(False, True, M, N) == "t128_TT"
    _gemm_shape(dev, (tA,), M, N, K)


@pytest.mark.parametrize("M,N,K,n_table", [(33, 36, 129, 50), (2048, 33, 33, 700), (2049, 7, 33, 700), (2113, 68, 97, 4000),
                                           (65409, 132, 37, 3000)])
def test_gemm_row_gather_kc(dev, M, N, K, n_table):
    """A_KC with a_row_idx (repeated and out-of-order ids; unreferenced table rows are NaN), in all three kernels."""
    rng = np.random.default_rng(M + N + K)
    tab, idx, A = _table(rng, M, K, n_table)
    B, bias = go.asym(rng, (K, N)), go.asym(rng, (N,))
    zmk = go.contract(A, B)
    Ain = In(tab, dev)
    for tB in (0, 1):
        _gemm_launches(dev, 0, tB, M, N, K, Ain, _dev(idx, dev), B, zmk, bias)


@pytest.mark.parametrize("K", [1023, 1024, 1025, 2049, 2080])
def test_gemm_tn_gather_refill(dev, K):
    """The row-gathered TN operand without split-K: its LDS index cache holds GS_IDXCAP = 1024 k and is refilled inside one slice at
    K > 1024 (twice at K >= 2049); a stale or shifted index after a refill is a wrong row of the table."""
    rng = np.random.default_rng(K)
    for M, N in ((65, 68), (100, 7)):
        tab, idx, At = _table(rng, K, M, K + 300)          # stored [K, M]: row k of A^T is table row idx[k]
        B, bias = go.asym(rng, (K, N)), go.asym(rng, (N,))
        zmk = go.contract(At.T, B)
        Ain = In(tab, dev)
        for tB in (0, 1):
            _gemm_launches(dev, 1, tB, M, N, K, Ain, _dev(idx, dev), B, zmk, bias)


def test_gemm_empty(dev):
    """M = 0 (n = 0 for the layer entry points) returns OK and touches nothing."""
    rng = np.random.default_rng(0)
    A, B, C = In(go.asym(rng, (4, 8)), dev), In(go.asym(rng, (8, 8)), dev), Out(dev, 4, 8)
    ops.call("gs_gemm_f32", 0, 0, 0, 8, 8, A.ptr, A.ld, None, B.ptr, B.ld, None, ID, C.ptr, C.ld, _st())
    ops.call("gs_sage_dense_fwd", None, 0, None, 0, A.ptr, A.ld, None, 8, 0, None, 0, B.ptr, B.ld, 8, 0, ID, None, C.ptr, C.ld, _st())
    ops.call("gs_dense_dgrad", A.ptr, A.ld, 0, 8, 0, B.ptr, B.ld, 8, C.ptr, C.ld, 0, _st())
    ops.call("gs_sage_dense_dgrad", A.ptr, A.ld, 0, 8, 0, B.ptr, B.ld, B.ptr, B.ld, 4, C.ptr, C.ld, _st())
    ops.call("gs_dense_fwd_rows_dev", A.ptr, A.ld, None, 8, 0, None, B.ptr, B.ld, 8, ID, None, C.ptr, C.ld, _st())
    C.untouched("empty calls")


# ====================================================================================== gs_sage_dense_fwd (+ _cogather)
class GatherJob(object):
    """One gather+mean job: its descriptor, the device buffers the descriptor points into, and the float64 mean."""

    def __init__(self, dev, rng, n, s, d, gcn):
        tab, idx, rows = _table(rng, n * s, d, 90)
        self.X, self.out, self.idx = In(tab, dev), Out(dev, n, d), _dev(idx, dev)
        j = self.desc = _lib.GatherDesc()
        j.X, j.idx, j.out, j.ldx, j.ldo, j.n, j.s, j.d = self.X.ptr, self.idx.data_ptr(), self.out.ptr, self.X.ld, self.out.ld, n, s, d
        self_rows = None
        if gcn:
            stab, sidx, self_rows = _table(rng, n, d, 40)
            self.S, self.sidx = In(stab, dev), _dev(sidx, dev)
            j.self_src, j.self_idx, j.ld_self = self.S.ptr, self.sidx.data_ptr(), self.S.ld
        self.want, self.bound = go.gather_mean(rows, np.arange(n * s), n, s, self_rows)
        self.tag = "gather job n=%d s=%d d=%d gcn=%d" % (n, s, d, gcn)

    def check(self):
        got = self.out.read(self.tag)
        _note("gather_job", go.assert_within(got, self.want, self.bound, self.tag))
        # ... and the rider has the BITS of the stand-alone launch of the same descriptor (the summation order is fixed)
        j = self.desc
        alone = Out(self.out.t.device, j.n, j.d)
        ops.call("gs_gather_mean_fwd", j.X, j.ldx, j.idx, j.n, j.s, j.d, j.self_src, j.ld_self, j.self_idx, alone.ptr, alone.ld, _st())
        want = alone.read(self.tag + " (stand-alone)")
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), \
            "%s: the rider's bits differ from gs_gather_mean_fwd's" % self.tag


def _gather_jobs(dev, rng, n_jobs):
    """Up to four gather+mean jobs: s = 1, s >= 8 (the two wave bodies), a GCN self term, more than one 64-float4 chunk."""
    specs = [(5, 1, 7, False), (33, 9, 50, False), (17, 3, 130, True), (6, 25, 260, False)][:n_jobs]
    return [GatherJob(dev, rng, *spec) for spec in specs]


def _sage_case(dev, rng, n, ds, da, out, concat, use_self, self_gather, agg_gather, use_bias, act, jobs=None, tight=False):
    n_table = 300
    terms, bufs = [], []                     # per term that is present: (rows, W) and its device operands (X, idx, W)
    for use, d, gather in ((use_self, ds, self_gather), (True, da, agg_gather)):
        if not use:
            continue
        tab, idx, rows = _table(rng, n, d, n_table)
        W = go.asym(rng, (d, out), 0.1)
        terms.append((rows, W))
        bufs.append((In(tab if gather else rows, dev, tight=tight), _dev(idx, dev) if gather else None, In(W, dev, tight=tight), d))
    args = [(None, 0, None, 0, None, 0)] * (2 - len(bufs)) + [(X.ptr, X.ld, ops.ptr(i), d, W.ptr, W.ld) for X, i, W, d in bufs]
    halves = 2 if (use_self and concat) else 1
    bias = go.asym(rng, (out * halves,)) if use_bias else None
    bt, bp = _bias(bias, dev)
    o = Out(dev, n, out * halves, tight=tight)
    (sp, sld, sip, sd, wsp, wsld), (ap, ald, aip, ad, wnp, wnld) = args
    head = (sp, sld, sip, sd, ap, ald, aip, ad, n, wsp, wsld, wnp, wnld, out, 1 if concat else 0, act, bp, o.ptr, o.ld)
    if jobs is None:
        ops.call("gs_sage_dense_fwd", *(head + (_st(),)))
        kind = variant(True, False, n, out, halves)
    else:
        arr = (_lib.GatherDesc * max(len(jobs), 1))(*[j.desc for j in jobs])
        ops.call("gs_sage_dense_fwd_cogather", *(head + (ctypes.addressof(arr), len(jobs), _st())))
        kind = "cogather_t64_NN" if n > 2048 else variant(True, False, n, out, halves)
    t = "%s sage n=%d d=(%d,%d) out=%d concat=%d self=%d gather=(%d,%d) bias=%d act=%d jobs=%s" % (
        kind, n, ds, da, out, concat, use_self, self_gather, agg_gather, use_bias, act, None if jobs is None else len(jobs))
    want, bound = go.product(terms, concat=bool(concat and use_self), bias=bias, relu=(act == RELU))
    _note(kind, go.assert_within(o.read(t), want, bound, t))


GATHERS = [(True, False), (False, True), (True, True), (False, False)]


@pytest.mark.parametrize("ds,da", [(50, 37), (602, 130)])
@pytest.mark.parametrize("n", [1, 33, 2048, 2049, 2113])
def test_sage_dense_fwd(dev, n, ds, da):
    """Two terms of different lengths, concat (out % 4 == 0) and add (also out 7 and 41); self_idx / agg_idx each present and absent
    (rotating through the four combinations along the sweep); bias over the full concat width, present and absent; self = None."""
    rng = np.random.default_rng(n * 7 + ds)
    i = 0
    for concat in (1, 0):
        for out in (4, 12, 68, 132) + (() if concat else (7, 41)):
            for rep in range(2 if out in (12, 68) else 1):      # the middle widths meet all four gather combinations
                sg, ag = GATHERS[i % 4]
                _sage_case(dev, rng, n, ds, da, out, concat, True, sg, ag, i % 3 != 2, RELU if i % 2 else ID,
                           tight=(out == 12 and rep == 0))
                i += 1
    for out, ag in ((68, True), (7, False), (132, True)):
        _sage_case(dev, rng, n, ds, da, out, 0, False, False, ag, True, RELU)


@pytest.mark.parametrize("n", [33, 2049, 2113])
@pytest.mark.parametrize("n_jobs", [0, 4])
def test_sage_dense_fwd_cogather(dev, n, n_jobs):
    """The horizontally fused launch (n > 2048: sage_dense_cogather_kernel; n <= 2048: the separate launches) with 0 and 4 gather
    jobs; the job outputs against the float64 mean."""
    rng = np.random.default_rng(n + n_jobs)
    i = 0
    for ds, da in ((50, 37), (602, 130)):
        for concat, out in ((1, 12), (1, 68), (0, 41), (0, 132)):
            jobs = _gather_jobs(dev, rng, n_jobs)
            sg, ag = GATHERS[i % 4]
            _sage_case(dev, rng, n, ds, da, out, concat, True, sg, ag, True, RELU if i % 2 else ID, jobs=jobs)
            for j in jobs:
                j.check()
            i += 1
    jobs = _gather_jobs(dev, rng, n_jobs)
    _sage_case(dev, rng, n, 50, 37, 68, 0, False, False, True, True, RELU, jobs=jobs)
    for j in jobs:
        j.check()


# ================================================================================================= gs_dense_fwd_rows_dev
def _rows_dev_case(dev, rng, n_max, n_dev, out, d, act):
    n_table = 500
    live = max(min(n_max, n_dev), 0)
    tab, idx, _ = _table(rng, n_max, d, n_table)
    idx[idx == n_table - 1] = 0
    idx[live:] = n_table - 1                                            # rows that do not exist point at a NaN row
    dead = np.ones(n_table, bool)
    dead[idx[:live]] = False
    tab = np.where(np.isnan(tab), np.float32(0.5), tab)
    tab[dead] = NAN
    W, bias = go.asym(rng, (d, out), 0.2), go.asym(rng, (out,))
    X, Wd, idx_d = In(tab, dev), In(W, dev), _dev(idx, dev)
    cnt = _dev(np.array([n_dev], np.int32), dev)
    bt, bp = _bias(bias, dev)
    o = Out(dev, n_max, out)
    ops.call("gs_dense_fwd_rows_dev", X.ptr, X.ld, idx_d.data_ptr(), d, n_max, cnt.data_ptr(), Wd.ptr, Wd.ld, out, act, bp,
             o.ptr, o.ld, _st())
    kind = variant(True, False, n_max, out, split=True) + "_mdev"
    t = "%s rows_dev n_max=%d n_dev=%d out=%d d=%d" % (kind, n_max, n_dev, out, d)
    got = o.read(t, rows_written=live)                                  # rows >= min(n_max, *n_dev) keep the sentinel
    assert not np.isnan(tab[idx[:live]]).any()
    want, bound = go.product([(tab[idx[:live]], W)], bias=bias, relu=(act == RELU))
    _note(kind, go.assert_within(got, want, bound, t))


@pytest.mark.parametrize("n_max", [2049, 4100])
def test_dense_fwd_rows_dev(dev, n_max):
    rng = np.random.default_rng(n_max)
    for i, n_dev in enumerate((0, 1, 63, 65, n_max, n_max + 7)):
        for out in (64, 68, 130):
            _rows_dev_case(dev, rng, n_max, n_dev, out, 37, RELU if i % 2 else ID)


def test_dense_fwd_rows_dev_t128(dev):
    """The device-side row count in the 128-row tiles: the XCD swizzle runs over the tiles that exist."""
    rng = np.random.default_rng(9)
    for n_dev in (65409, 40001):
        _rows_dev_case(dev, rng, 65409, n_dev, 130, 37, RELU)


# ================================================================================================= gs_dense_pool_max_fwd
def _pool_case(dev, rng, n, s, d, hid, gathered, big):
    rows = n * s
    tab, idx, Xr = _table(rng, rows, d, 300)
    p1, p2 = 0, 0
    if s >= 2:                                   # an exact tie in every group: position p2 repeats the id at p1 < p2
        p1, p2 = (s // 3, s - 1) if s > 2 else (0, 1)
        idx2 = idx.reshape(n, s)
        idx2[:, p2] = idx2[:, p1]
        dead = np.ones(tab.shape[0], bool); dead[idx] = False
        tab[dead] = NAN                          # (rows that lost their last reference)
        Xr = tab[idx]
        assert not np.isnan(Xr).any()
    W, bias = go.asym(rng, (d, hid), 0.2), go.asym(rng, (hid,), 0.1)
    neg = np.arange(hid) % 7 == 3
    bias[neg] = -100.0                           # all-negative columns: relu gives 0 in every row of every group
    X = In(tab, dev) if gathered else In(Xr, dev)
    idx_d = _dev(idx, dev) if gathered else None
    Wd = In(W, dev)
    bt, bp = _bias(bias, dev)
    pooled, arg = Out(dev, n, hid), Out(dev, n, hid, dtype=np.int32)
    ops.call("gs_dense_pool_max_fwd", X.ptr, X.ld, ops.ptr(idx_d), d, n, s, Wd.ptr, Wd.ld, hid, bp, pooled.ptr, pooled.ld,
             arg.ptr, arg.ld, _st())
    tiles128 = cdiv(rows, (128 // s) * s) * cdiv(hid, 128)
    assert (tiles128 >= 512) == big
    kind = ("t128" if big else "t64") + "_NN_pool"
    t = "%s pool n=%d s=%d d=%d hid=%d gathered=%d" % (kind, n, s, d, hid, gathered)
    h, hb = go.product([(Xr, W)], bias=bias, relu=True)
    want, wb, h3, hb3 = go.pool_max(h, hb, s)
    _note(kind, go.assert_within(pooled.read(t, pad_zero=False), want, wb, t))
    a = arg.read(t, pad_zero=False)
    assert go.argmax_acceptable(h3, hb3, a).all(), "%s: an arg-max outside the slack" % t
    if s >= 2:
        assert (a != p2).all(), "%s: the later of two identical rows was reported" % t
    assert (a[:, neg] == 0).all() and (want[:, neg] == 0).all(), "%s: an all-zero group must report index 0" % t


@pytest.mark.parametrize("s", [1, 2, 25, 33, 64])
def test_dense_pool_max_fwd_t64(dev, s):
    """64-row tiles hold g = 64 // s whole groups; n = 2 g + ceil(g / 2) leaves a partial set in the last tile (g = 1: n = 3)."""
    rng = np.random.default_rng(s)
    g = 64 // s
    n = 2 * g + (g + 1) // 2 if g > 1 else 3
    for hid in (5, 64, 68, 130):
        for gathered in (True, False):
            _pool_case(dev, rng, n, s, 37, hid, gathered, False)


@pytest.mark.parametrize("s", [1, 2, 25, 33, 64])
def test_dense_pool_max_fwd_t128(dev, s):
    """128-row tiles from 512 of them: the smallest n with one more group than fills 255 (hidden 130: two column tiles) or 511
    (hidden <= 128) row tiles, so the last tile holds a single group."""
    rng = np.random.default_rng(100 + s)
    g = 128 // s
    for hid, gathered in ((130, True), (130, False), (68, True), (64, False), (5, True)):
        n = (255 if hid > 128 else 511) * g + 1
        _pool_case(dev, rng, n, s, 37 if hid == 130 else 9, hid, gathered, True)


# ========================================================================= gs_dense_wgrad (+ _grouped, _grouped_cogather)
class Slabs(object):
    """[n_slabs, d, ld_slab] split-K slabs inside a flat buffer with guard words on both sides, pre-filled with the sentinel."""

    def __init__(self, dev, n_slabs, d, out, tight=False):
        self.n_slabs, self.d, self.out = n_slabs, d, out
        self.ld = round_up(out, 4) + (0 if tight else 12)
        self.guard = 64
        self.t = _dev(np.full(2 * self.guard + n_slabs * d * self.ld, S, np.float32), dev)
        self.ptr = self.t.data_ptr() + 4 * self.guard

    def check(self, A_rows, dZ_cols, n, tag):
        """Split-K promises the logical block of every slab (zeros for an empty slice) and nothing else: the pad columns keep the
        sentinel.  Each slab is compared with its own row slice, and the float64 sum of the slabs with the whole product."""
        torch.cuda.synchronize()
        got = self.t.cpu().numpy()
        assert np.all(got[:self.guard] == S) and np.all(got[-self.guard:] == S), "%s: wrote outside the slabs" % tag
        sl = got[self.guard:-self.guard].reshape(self.n_slabs, self.d, self.ld)
        assert np.all(sl[:, :, self.out:] == S), "%s: split-K wrote beyond the logical columns" % tag
        r = 0.0
        for z, (a, b) in enumerate(go.slab_rows(n, self.n_slabs)):
            if a == b:
                assert np.all(sl[z, :, :self.out] == 0), "%s: the empty slab %d must be zeros" % (tag, z)
            else:                                 # every slab against its own row slice, K_total = the slice's length
                want, bound = go.wgrad(A_rows[a:b], dZ_cols[a:b])
                r = max(r, go.assert_within(sl[z, :, :self.out], want, bound, "%s slab %d rows [%d, %d)" % (tag, z, a, b)))
        want, bound = go.wgrad(A_rows, dZ_cols)
        return max(r, go.assert_within(sl[:, :, :self.out].astype(np.float64).sum(axis=0), want, bound, tag + " slab sum"))


def _wgrad_problem(dev, rng, n, d, out, col0, slabs, gathered, tight=False, live=False):
    tab, idx, A_rows = _table(rng, n, d, n + 200 if gathered else n)
    A = In(tab, dev, tight=tight) if gathered else In(A_rows, dev, tight=tight)
    idx_d = _dev(idx, dev) if gathered else None
    dZ = go.wgrad_dz(rng, n, out, slabs)          # row-sparse from go.LONG_N rows, so that the bound stays sensitive
    ldz = col0 + round_up(out, 4) + (0 if tight else 12)
    fill = go.asym(rng, (n + 1, ldz)) if live else NAN       # live: a cols_slice of a wider matrix, the K tail is its next columns
    Z = In(dZ, dev, col0=col0, fill=fill, ld=ldz)
    return A, idx_d, Z, Slabs(dev, slabs, d, out, tight), A_rows, dZ


WGRAD = [(1, 5, 7, 0, 1), (33, 65, 68, 4, 2), (100, 50, 41, 0, 7), (2080, 130, 132, 128, 1), (130, 64, 64, 0, 3),
         (16385, 130, 132, 0, 3), (16384, 128, 128, 4, 1)]


@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("n,d,out,col0,slabs", WGRAD)
def test_dense_wgrad(dev, n, d, out, col0, slabs, gathered):
    """(100, 50, 41, 0, 7): slices of 32 rows, the last three slabs are empty and must be written as zeros; (2080, 130, 132, 128, 1): one
    slab, the index cache refills twice inside it; n >= 16384 with d, out >= 128: the 128x128 TN tiles."""
    rng = np.random.default_rng(n + d + out + col0)
    big = n >= 16384 and d >= 128 and out >= 128
    kind = ("t128" if big else "t64") + "_TN_splitk"
    for live in ((False, True) if col0 == 4 else (False,)):
        A, idx_d, Z, sl, A_rows, dZ = _wgrad_problem(dev, rng, n, d, out, col0, slabs, gathered, tight=(n == 33), live=live)
        ops.call("gs_dense_wgrad", A.ptr, A.ld, ops.ptr(idx_d), d, Z.ptr, Z.ld, col0, out, n, slabs, sl.ptr, sl.ld, _st())
        t = "%s wgrad n=%d d=%d out=%d col0=%d slabs=%d gathered=%d live=%d" % (kind, n, d, out, col0, slabs, gathered, live)
        _note(kind, sl.check(A_rows, dZ, n, t))


@pytest.mark.parametrize("with_jobs", [False, True])
def test_dense_wgrad_grouped(dev, with_jobs):
    """13 problems of mixed shapes: GS_MAX_GROUP = 12 in the first launch, one in the second, where the gather jobs ride."""
    rng = np.random.default_rng(13 + with_jobs)
    shapes = [(1, 5, 7, 0, 1), (33, 65, 68, 4, 2), (100, 50, 41, 0, 7), (2080, 130, 132, 128, 1), (65, 1, 12, 0, 2),
              (130, 64, 64, 0, 3), (97, 3, 130, 8, 4), (1025, 9, 5, 4, 1), (64, 128, 4, 0, 2), (31, 66, 1, 0, 1),
              (300, 37, 36, 12, 5), (1, 1, 1, 0, 3), (161, 70, 129, 4, 2)]
    assert len(shapes) == 13
    probs = [_wgrad_problem(dev, rng, n, d, out, col0, slabs, gathered=(i % 2 == 1), live=(i % 5 == 1))
             for i, (n, d, out, col0, slabs) in enumerate(shapes)]
    arr = (_lib.WgradDesc * 13)()
    for q, (A, idx_d, Z, sl, _, _), (n, d, out, col0, slabs) in zip(arr, probs, shapes):
        q.A, q.a_idx, q.dZ, q.slabs = A.ptr, ops.ptr(idx_d), Z.ptr, sl.ptr
        q.lda, q.ldz, q.ld_slab, q.n, q.d, q.col0, q.out_dim, q.n_slabs = A.ld, Z.ld, sl.ld, n, d, col0, out, slabs
        q.a_rows = A.t.shape[0] - 1
    if with_jobs:
        jobs = _gather_jobs(dev, rng, 4)
        jarr = (_lib.GatherDesc * 4)(*[j.desc for j in jobs])
        ops.call("gs_dense_wgrad_grouped_cogather", ctypes.addressof(arr), 13, ctypes.addressof(jarr), 4, _st())
        for j in jobs:
            j.check()
    else:
        ops.call("gs_dense_wgrad_grouped", ctypes.addressof(arr), 13, _st())
    kind = "grouped_cogather_TN" if with_jobs else "grouped_TN"
    for (A, idx_d, Z, sl, A_rows, dZ), shape in zip(probs, shapes):
        _note(kind, sl.check(A_rows, dZ, shape[0], "%s problem %r" % (kind, shape)))


# ==================================================================================== gs_dense_dgrad, gs_sage_dense_dgrad
@pytest.mark.parametrize("n", [1, 33, 2048, 2049, 2113])
def test_dense_dgrad(dev, n):
    """dX (+)= dZ[:, col0 : col0 + out] . W^T: the NT form (small kernel to n = 2048, 64x64 beyond).  col0 = 4 puts live finite data on
    both sides of the slice (the K tail reads the neighbour's columns: only the kernels' masking keeps them out), col0 in {0, 128}
    NaN; accumulate over a random pre-fill and plain over the sentinel."""
    rng = np.random.default_rng(n)
    for out in (1, 7, 41, 128):
        for col0 in (0, 4, 128):
            dZ = go.asym(rng, (n, out))
            ldz = col0 + round_up(out, 4) + 12
            Z = In(dZ, dev, col0=col0, ld=ldz, fill=(go.asym(rng, (n + 1, ldz)) if col0 == 4 else NAN))
            for d in (4, 7, 36, 41, 68, 256):
                W = go.asym(rng, (d, out))
                Wd = In(W, dev, tight=(d == 36))
                for acc in (0, 1):
                    prev = go.asym(rng, (n, d)) if acc else None
                    o = Out(dev, n, d, prefill=prev, tight=(d == 36))
                    ops.call("gs_dense_dgrad", Z.ptr, Z.ld, col0, out, n, Wd.ptr, Wd.ld, d, o.ptr, o.ld, acc, _st())
                    kind = variant(True, True, n, d)
                    t = "%s dgrad n=%d d=%d out=%d col0=%d acc=%d" % (kind, n, d, out, col0, acc)
                    want, bound = go.product([(dZ, W.T)], c_in=prev)
                    _note(kind, go.assert_within(o.read(t), want, bound, t))


@pytest.mark.parametrize("n", [1, 33, 2048, 2049, 2113])
def test_sage_dense_dgrad(dev, n):
    """Both input gradients in one two-term NT launch with a concatenated output [n, 2 d_in]; the forward was a concat (the neighbour
    half reads dZ + out_dim: its K tail is the end of the row, the self half's K tail is the neighbour half's live data) or an add."""
    rng = np.random.default_rng(50 + n)
    for concat, outs in ((1, (4, 12, 128)), (0, (7, 41))):
        for out in outs:
            w = out * (2 if concat else 1)
            dZ = go.asym(rng, (n, w))
            Z = In(dZ, dev, tight=(out == 12))
            for d_in in (4, 36, 68, 256):
                Ws, Wn = go.asym(rng, (d_in, out)), go.asym(rng, (d_in, out))
                Wsd, Wnd = In(Ws, dev), In(Wn, dev)
                o = Out(dev, n, 2 * d_in, tight=(d_in == 36))
                ops.call("gs_sage_dense_dgrad", Z.ptr, Z.ld, n, out, concat, Wsd.ptr, Wsd.ld, Wnd.ptr, Wnd.ld, d_in, o.ptr, o.ld, _st())
                kind = variant(True, True, n, d_in, halves=2)
                t = "%s sage_dgrad n=%d d_in=%d out=%d concat=%d" % (kind, n, d_in, out, concat)
                dZn = dZ[:, out:] if concat else dZ
                want, bound = go.product([(dZ[:, :out], Ws.T), (dZn, Wn.T)], concat=True)
                _note(kind, go.assert_within(o.read(t), want, bound, t))


# ==================================================================================================== argument refusals
def test_argument_refusals(dev):
    """Bad arguments come back as an error through ops.call (nothing is launched) and the outputs keep their sentinels."""
    rng = np.random.default_rng(77)
    n, d, out = 40, 16, 8
    X, W, Z = In(go.asym(rng, (n, d)), dev), In(go.asym(rng, (d, 2 * out)), dev), In(go.asym(rng, (n, 2 * out)), dev)
    idx = _dev(np.arange(n, dtype=np.int32), dev)
    cnt = _dev(np.array([n], np.int32), dev)
    o = Out(dev, 4100, 2 * d + 2 * out)
    oi = Out(dev, n, 2 * out, dtype=np.int32)
    sl = Slabs(dev, 2, d, out)
    st = _st()
    wd = _lib.WgradDesc()
    wd.A, wd.dZ, wd.slabs, wd.lda, wd.ldz, wd.ld_slab, wd.n, wd.d, wd.col0, wd.out_dim, wd.n_slabs = (
        X.ptr, Z.ptr, sl.ptr, X.ld, Z.ld, sl.ld, n, d, 2, out, 2)
    wd_ld = _lib.WgradDesc()
    wd_ld.A, wd_ld.dZ, wd_ld.slabs, wd_ld.lda, wd_ld.ldz, wd_ld.ld_slab, wd_ld.n, wd_ld.d, wd_ld.col0, wd_ld.out_dim, wd_ld.n_slabs = (
        X.ptr, Z.ptr, sl.ptr, X.ld, Z.ld, out - 4, n, d, 0, out, 2)
    no_jobs = (_lib.GatherDesc * 1)()
    bad = [
        # ld too small
        ("gs_gemm_f32", (0, 0, n, out, d, X.ptr, d - 4, None, W.ptr, W.ld, None, ID, o.ptr, o.ld, st)),
        ("gs_gemm_f32", (0, 0, n, out, d, X.ptr, X.ld, None, W.ptr, out - 4, None, ID, o.ptr, o.ld, st)),
        ("gs_gemm_f32", (1, 0, d, out, n, X.ptr, X.ld, None, Z.ptr, Z.ld, None, ID, o.ptr, out - 4, st)),
        ("gs_sage_dense_fwd", (X.ptr, X.ld, None, d, X.ptr, X.ld, None, d, n, W.ptr, W.ld, W.ptr, W.ld, out, 1, ID, None, o.ptr, 2 * out - 4, st)),
        ("gs_sage_dense_fwd", (X.ptr, d - 4, None, d, X.ptr, X.ld, None, d, n, W.ptr, W.ld, W.ptr, W.ld, out, 1, ID, None, o.ptr, o.ld, st)),
        ("gs_sage_dense_fwd_cogather", (X.ptr, X.ld, None, d, X.ptr, X.ld, None, d, n, W.ptr, W.ld, W.ptr, W.ld, out, 1, ID, None, o.ptr,
                                        2 * out - 4, ctypes.addressof(no_jobs), 0, st)),
        ("gs_dense_fwd_rows_dev", (X.ptr, X.ld, idx.data_ptr(), d, 4100, cnt.data_ptr(), W.ptr, W.ld, out, ID, None, o.ptr, out - 4, st)),
        ("gs_dense_fwd_rows_dev", (X.ptr, X.ld, idx.data_ptr(), d, 4100, cnt.data_ptr(), W.ptr, out - 4, out, ID, None, o.ptr, o.ld, st)),
        ("gs_dense_pool_max_fwd", (X.ptr, X.ld, None, d, 10, 4, W.ptr, W.ld, out, None, o.ptr, out - 4, oi.ptr, oi.ld, st)),
        ("gs_dense_pool_max_fwd", (X.ptr, X.ld, None, d, 10, 4, W.ptr, W.ld, out, None, o.ptr, o.ld, oi.ptr, out - 4, st)),
        ("gs_dense_wgrad", (X.ptr, X.ld, None, d, Z.ptr, Z.ld, 0, out, n, 2, sl.ptr, out - 4, st)),
        ("gs_dense_wgrad", (X.ptr, X.ld, None, d, Z.ptr, out + 4, 8, out, n, 2, sl.ptr, sl.ld, st)),
        ("gs_dense_wgrad_grouped", (ctypes.addressof(wd_ld), 1, st)),
        ("gs_dense_dgrad", (Z.ptr, Z.ld, 0, out, n, W.ptr, W.ld, d, o.ptr, d - 4, 0, st)),
        ("gs_sage_dense_dgrad", (Z.ptr, Z.ld, n, out, 1, W.ptr, W.ld, W.ptr, W.ld, d, o.ptr, 2 * d - 4, st)),
        # concat with out % 4 != 0
        ("gs_sage_dense_fwd", (X.ptr, X.ld, None, d, X.ptr, X.ld, None, d, n, W.ptr, W.ld, W.ptr, W.ld, 7, 1, ID, None, o.ptr, o.ld, st)),
        ("gs_sage_dense_fwd_cogather", (X.ptr, X.ld, None, d, X.ptr, X.ld, None, d, n, W.ptr, W.ld, W.ptr, W.ld, 7, 1, ID, None, o.ptr,
                                        o.ld, ctypes.addressof(no_jobs), 0, st)),
        ("gs_sage_dense_dgrad", (Z.ptr, Z.ld, n, 7, 1, W.ptr, W.ld, W.ptr, W.ld, d, o.ptr, o.ld, st)),
        # col0 % 4 != 0
        ("gs_dense_wgrad", (X.ptr, X.ld, None, d, Z.ptr, Z.ld, 2, out, n, 2, sl.ptr, sl.ld, st)),
        ("gs_dense_wgrad_grouped", (ctypes.addressof(wd), 1, st)),
        ("gs_dense_wgrad_grouped_cogather", (ctypes.addressof(wd), 1, ctypes.addressof(no_jobs), 0, st)),
        ("gs_dense_dgrad", (Z.ptr, Z.ld, 6, out, n, W.ptr, W.ld, d, o.ptr, o.ld, 0, st)),
        # the device-side row count is for the tiled kernels only
        ("gs_dense_fwd_rows_dev", (X.ptr, X.ld, idx.data_ptr(), d, 2048, cnt.data_ptr(), W.ptr, W.ld, out, ID, None, o.ptr, o.ld, st)),
        # pool groups beyond a tile
        ("gs_dense_pool_max_fwd", (X.ptr, X.ld, None, d, 1, 65, W.ptr, W.ld, out, None, o.ptr, o.ld, oi.ptr, oi.ld, st)),
        # d_in % 4 != 0
        ("gs_sage_dense_dgrad", (Z.ptr, Z.ld, n, out, 1, W.ptr, W.ld, W.ptr, W.ld, 6, o.ptr, o.ld, st)),
    ]
    for name, args in bad:
        with pytest.raises(_lib.GraphsageAmdError):
            ops.call(name, *args)
    torch.cuda.synchronize()
    o.untouched("refusals")
    oi.untouched("refusals (arg-max)")
    assert np.all(sl.t.cpu().numpy() == S)
