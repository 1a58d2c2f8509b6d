"""CPU: the evidence that tests/test_gemm_edges_gpu.py is sensitive.  The kernels' arithmetic is emulated in np.float32 (a k-ordered
fmaf chain; the four-partial K split of gemm_small_kernel) on the input distribution and the shape classes of the GPU tests:
  * the emulation stays inside gemm_oracle's derived bound (so a correct kernel passes), and
  * each planted fault -- a dropped last k, a dropped last row, output columns shifted by one, a bias indexed without the concat
    offset, one pad element (a finite value of about 1) leaking into the K tail, a stale gather index after a 1024 boundary --
    lands outside it for the same inputs (so a wrong kernel fails)."""
import numpy as np
import pytest

import gemm_oracle as go

# (name, small form?, M, N, K): one per kernel variant / pipeline class of the GPU sweeps of the forward / input-gradient forms, at the
# largest K of each; the long weight-gradient reductions (K_total = n up to 16385) have test_long_reduction_faults below
SHAPES = [("small_1stage", True, 33, 36, 33), ("small_3stages", True, 31, 33, 389), ("small_k1", True, 1, 4, 1),
          ("t64_pipeline", False, 65, 68, 161), ("t64_tail", False, 63, 7, 97), ("t128", False, 130, 132, 97),
          ("tn_gather_refill", False, 65, 68, 2080)]


def _ops(name, M, N, K):
    rng = np.random.default_rng(sum(name.encode()) + M + N + K)
    return go.asym(rng, (M, K)), go.asym(rng, (K, N)), go.asym(rng, (N,))


def _emulate(small, terms):
    if small:
        return go.chain_small(terms)
    acc = None
    for A, B in terms:
        acc = go.chain(A, B, acc)
    return acc


@pytest.mark.parametrize("name,small,M,N,K", SHAPES)
def test_emulation_inside_bound(name, small, M, N, K):
    A, B, bias = _ops(name, M, N, K)
    for b in (None, bias):
        for relu in (False, True):
            want, bound = go.product([(A, B)], bias=b, relu=relu)
            r = go.assert_within(go.epilogue(_emulate(small, [(A, B)]), b, relu), want, bound, name)
            print("%s bias=%d relu=%d: err / bound %.3f" % (name, b is not None, relu, r))


@pytest.mark.parametrize("name,small,M,N,K", SHAPES)
def test_planted_faults_outside_bound(name, small, M, N, K):
    A, B, bias = _ops(name, M, N, K)
    want, bound = go.product([(A, B)], bias=bias)
    good = go.epilogue(_emulate(small, [(A, B)]), bias)
    assert go.within(good, want, bound)
    # last k element dropped
    A_drop = A.copy(); A_drop[:, K - 1] = 0
    assert not go.within(go.epilogue(_emulate(small, [(A_drop, B)]), bias), want, bound)
    # last row dropped: the output keeps its pre-fill
    for prefill in (go.SENTINEL, np.float32(0)):
        bad = good.copy(); bad[M - 1] = prefill
        assert not go.within(bad, want, bound)
    # output columns shifted by one (either way), the vacated column zero
    if N > 1:
        for sh in (1, -1):
            bad = np.roll(good, sh, axis=1); bad[:, 0 if sh == 1 else N - 1] = 0
            assert not go.within(bad, want, bound)
    # one pad element leaking into the K tail: A's pad holds 1.0 and B's row K is the next operand's live data
    leak = go.asym(np.random.default_rng(K), (N,))
    bad = good.copy(); bad[M // 2] = (bad[M // 2].astype(np.float64) + 1.0 * leak).astype(np.float32)
    assert not go.within(bad, want, bound)
    # ... and NaN pads (what the GPU tests plant) can never pass
    bad = good.copy(); bad[0, 0] = np.nan
    assert not go.within(bad, want, bound)
    with pytest.raises(AssertionError):
        go.assert_within(bad, want, bound, name)


@pytest.mark.parametrize("small,M,K0,K1,N", [(True, 33, 50, 37, 12), (False, 65, 602, 130, 68)])
def test_two_terms_concat_add_and_bias_offset(small, M, K0, K1, N):
    rng = np.random.default_rng(M + K0)
    A0, B0, A1, B1 = go.asym(rng, (M, K0)), go.asym(rng, (K0, N)), go.asym(rng, (M, K1)), go.asym(rng, (K1, N))
    # add: one chain over both terms
    bias = go.asym(rng, (N,))
    want, bound = go.product([(A0, B0), (A1, B1)], bias=bias, relu=True)
    assert go.within(go.epilogue(_emulate(small, [(A0, B0), (A1, B1)]), bias, True), want, bound)
    assert not go.within(go.epilogue(_emulate(small, [(A0, B0)]), bias, True), want, bound)          # second term lost
    # concat: two chains side by side, bias over the full width
    bias2 = go.asym(rng, (2 * N,))
    want, bound = go.product([(A0, B0), (A1, B1)], concat=True, bias=bias2)
    halves = [_emulate(small, [(A0, B0)]), _emulate(small, [(A1, B1)])]
    assert go.within(go.epilogue(np.concatenate(halves, axis=1), bias2), want, bound)
    # bias indexed without the concat offset: the neighbour half gets the self half's bias
    bad = np.concatenate([go.epilogue(halves[0], bias2[:N]), go.epilogue(halves[1], bias2[:N])], axis=1)
    assert not go.within(bad, want, bound)
    # halves swapped
    assert not go.within(go.epilogue(np.concatenate(halves[::-1], axis=1), bias2), want, bound)


def test_stale_index_after_1024_boundary():
    """Row-gathered TN operand (dW = A[idx]^T . dZ): the index cache is refilled every 1024 k; one index left over from the previous
    fill (idx[1024] read as idx[0]) must be caught at K = 1025 and 2080."""
    for K in (1025, 2080):
        rng = np.random.default_rng(K)
        d, out, rows = 9, 7, 300
        X, dZ = go.asym(rng, (rows, d)), go.asym(rng, (K, out))
        idx = rng.integers(0, rows, size=K)
        idx[1024] = (idx[0] + 1) % rows
        want, bound = go.wgrad(X[idx], dZ)
        assert go.within(go.chain(X[idx].T, dZ), want, bound)
        stale = idx.copy(); stale[1024] = idx[0]
        assert not go.within(go.chain(X[stale].T, dZ), want, bound)


@pytest.mark.parametrize("n,d,out,n_slabs", [(16385, 130, 132, 3), (16384, 128, 128, 1)])
def test_long_reduction_faults(n, d, out, n_slabs):
    """The 128x128 split-K weight-gradient shapes of the GPU test, with its inputs (dense A rows, gemm_oracle.wgrad_dz): with dense unit
    operands the bound is about 10 per element there and a single lost product passes; with the row-sparse dZ the emulated chain is
    inside the bound and each fault is outside it, per slab and in the slab sum.  (A row whose dZ is zero adds exactly nothing to an
    fmaf chain, so the emulation walks the live rows only.)"""
    rng = np.random.default_rng(n)
    rows = 300
    X, idx = go.asym(rng, (rows, d)), rng.integers(0, rows, size=n)
    dZ = go.wgrad_dz(rng, n, out, n_slabs)
    live = np.flatnonzero(np.abs(dZ).sum(axis=1))
    assert len(live) < n // 32 and set(go.edge_rows(n, n_slabs)) <= set(live.tolist())
    slices = [(a, b) for a, b in go.slab_rows(n, n_slabs) if b > a]

    def slabs_of(idx_used, dZ_used, slices_used=slices, extra=None):
        out_ = []
        for a, b in slices_used:
            ks = [k for k in live if a <= k < b]
            acc = go.chain(X[idx_used].T, dZ_used, None, ks)
            if extra is not None and (a, b) == slices_used[-1]:
                acc = (acc.astype(np.float64) + extra).astype(np.float32)
            out_.append(acc)
        return out_

    def inside(slabs):
        per_slab = all(go.within(s_, *go.wgrad(X[idx[a:b]], dZ[a:b])) for s_, (a, b) in zip(slabs, slices))
        total = go.within(np.sum([s_.astype(np.float64) for s_ in slabs], axis=0), *go.wgrad(X[idx], dZ))
        return per_slab, total

    assert inside(slabs_of(idx, dZ)) == (True, True)
    # the last k dropped; the last k of the first slab dropped
    for k in (n - 1, slices[0][1] - 1):
        cut = dZ.copy(); cut[k] = 0
        assert inside(slabs_of(idx, cut)) == (False, False), k
    # a stale gather index after a refill of the 1024-entry cache (first slab, and the last slab counted from its own first row)
    for k in (1024, slices[-1][0] + 1024):
        stale = idx.copy(); stale[k] = (idx[k - 1024] + 1) % rows if idx[k - 1024] == idx[k] else idx[k - 1024]
        assert inside(slabs_of(stale, dZ)) == (False, False), k
    # one pad element (1.0) leaking into the K tail: A's row n holds 1.0 and dZ's row n is live data
    leak = 1.0 * go.f64(go.asym(rng, (out,)))[None, :] * np.ones((d, 1))
    assert inside(slabs_of(idx, dZ, extra=leak)) == (False, False)
    # a slab that runs one row into its neighbour (wrong k_end): the slab is wrong; so is the sum, which counts that row twice
    if len(slices) > 1:
        (a0, b0), rest = slices[0], slices[1:]
        assert inside(slabs_of(idx, dZ, [(a0, b0 + 1)] + rest)) == (False, False)
    # ... and what the sparse inputs are for: dense unit operands hide the dropped last k at this length
    dense = go.asym(rng, (n, out))
    want, bound = go.wgrad(X[idx], dense)
    err = np.abs(np.outer(go.f64(X[idx[n - 1]]), go.f64(dense[n - 1])))
    print("dense operands, n = %d: a dropped last k is at most %.2f of the bound" % (n, float((err / bound).max())))


def test_accumulate_slabs_and_slab_rows():
    rng = np.random.default_rng(5)
    n, d, out = 100, 50, 41
    A, dZ, prev = go.asym(rng, (n, d)), go.asym(rng, (n, out)), go.asym(rng, (d, out))
    want, bound = go.product([(A.T, dZ)], c_in=prev)
    assert go.within(go.epilogue(go.chain(A.T, dZ), c_in=prev), want, bound)
    assert not go.within(go.chain(A.T, dZ), want, bound)                       # accumulate ignored
    sl = go.slab_rows(n, 7)
    assert sl == [(0, 32), (32, 64), (64, 96), (96, 100), (100, 100), (100, 100), (100, 100)]
    slabs = [go.chain(A[a:b].T, dZ[a:b]) for a, b in sl]
    assert all(not s.any() for s in slabs[4:])
    want, bound = go.wgrad(A, dZ)
    assert go.within(np.sum([s.astype(np.float64) for s in slabs], axis=0), want, bound)
    assert not go.within(np.sum([s.astype(np.float64) for s in slabs[:-4]], axis=0), want, bound)   # the short slab lost
    assert go.slab_rows(16385, 3) == [(0, 5472), (5472, 10944), (10944, 16385)]


def test_pool_max_and_argmax_slack():
    rng = np.random.default_rng(6)
    n, s, d, hid = 5, 25, 37, 12
    X, W, b = go.asym(rng, (n * s, d)), go.asym(rng, (d, hid), 0.2), go.asym(rng, (hid,), 0.1)
    b[3] = -100.0                                                 # an all-negative column: relu gives 0 everywhere
    X[2::s] = X[1::s]                                             # an exact tie at positions 1 and 2 of every group
    h, hb = go.product([(X, W)], bias=b, relu=True)
    want, wb, h3, hb3 = go.pool_max(h, hb, s)
    got = go.epilogue(go.chain(X, W), b, True).reshape(n, s, hid)
    assert go.within(got.max(axis=1), want, wb)
    arg = got.argmax(axis=1)                                      # NumPy: the first maximum, as the kernel
    assert go.argmax_acceptable(h3, hb3, arg).all()
    assert (arg != 2).all() and (arg[:, 3] == 0).all() and (want[:, 3] == 0).all()
    assert not go.argmax_acceptable(h3, hb3, h3.argmin(axis=1))[:, np.arange(hid) != 3].all()
    assert not go.argmax_acceptable(h3, hb3, np.full_like(arg, s)).any()
    # a pooled value taken over s - 1 rows (last row of the group dropped) is caught wherever that row wins
    short = got[:, :s - 1].max(axis=1)
    assert go.within(short, want, wb) == bool((h3.argmax(axis=1) != s - 1).all())


def test_gather_mean_bound():
    rng = np.random.default_rng(7)
    X = go.asym(rng, (40, 9))
    for s in (1, 9, 25):
        idx = rng.integers(0, 40, size=6 * s)
        want, bound = go.gather_mean(X, idx, 6, s)
        acc = np.zeros((6, 9), np.float32)
        for j in range(s):
            acc = acc + X[idx].reshape(6, s, 9)[:, j]
        assert go.within(acc * np.float32(1.0 / s), want, bound)
        assert not go.within(acc * np.float32(1.0 / (s + 1)), want, bound)
