"""NumPy float64 references and a DERIVED elementwise error bound for the fp32 MFMA contractions of csrc/gs_gemm.hip
(gs_gemm_f32, gs_sage_dense_fwd[_cogather], gs_dense_fwd_rows_dev, gs_dense_pool_max_fwd, gs_dense_wgrad[_grouped[_cogather]],
gs_dense_dgrad, gs_sage_dense_dgrad).  No GPU, no torch.

The bound.  Every output element of these kernels is a k-ordered fp32 fmaf chain over the K_total products that land in it
(v_mfma_f32_32x32x2_f32 accumulates in k order; the 8-wide k group is permuted, which re-orders but does not lengthen the
chain), followed by at most a handful of further fp32 additions: the small kernel adds four partial chains, a two-term add
continues the chain, then bias, then the accumulate read-modify-write; a slab sum adds the slabs.  With u = 2^-24 the unit
roundoff, the standard forward bound of a length-n recursive sum of exact products is gamma_n * sum|a_k b_k| with
gamma_n = n u / (1 - n u); every addend passes through at most K_total + 8 roundings here, so

    |got - exact| <= (K_total + 8) * u * (|A| @ |B| + |bias| + |C_in|)  +  u * |want|

where the last term is the rounding of the value that is finally stored (relu is 1-Lipschitz and exact).  This is the first-order
form: the second-order factor 1 / (1 - n u) is <= 1 + 2^-10 at the longest chain of the suite (n = 16392) and is left out -- a worst
case needs every rounding to err the same way by a full u, and the fmaf chain's roundings number K_total + 5 at most, three short
of the count used.  It is evaluated in float64 and it is the ONLY tolerance of tests/test_gemm_edges_gpu.py: no rtol / atol
constants.
"""
import numpy as np

U = 2.0 ** -24
SENTINEL = np.float32(-24680.5)          # what outputs are pre-filled with (never produced by the standard-normal inputs)
ISENTINEL = np.int32(-77)


def asym(rng, shape, scale=1.0):
    """fp32 standard normals (scaled): no symmetry, so a transposed or shifted operand cannot pass."""
    return (rng.standard_normal(size=shape) * scale).astype(np.float32)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def contract(A, B):
    """(z = A @ B, |A| @ |B|, K) in float64: a term that several cases share is contracted once and passed to product()."""
    A, B = f64(A), f64(B)
    return A @ B, np.abs(A) @ np.abs(B), A.shape[1]


def product(terms, concat=False, bias=None, relu=False, c_in=None):
    """terms: [(A [M, K_i], B [K_i, N])], the LOGICAL operands (already gathered / transposed / column-sliced), or the triples
    that contract() made of them.  concat: term i fills columns [i*N, (i+1)*N); otherwise the terms are summed.  bias spans
    the full output width.  c_in: accumulate (C += result, identity activation only).
    Returns (want, bound), float64 [M, N_total]."""
    done = [t if len(t) == 3 else contract(*t) for t in terms]
    zs, mags, ks = [t[0] for t in done], [t[1] for t in done], [t[2] for t in done]
    if concat:
        z = np.concatenate(zs, axis=1)
        mag = np.concatenate(mags, axis=1)
        k = np.concatenate([np.full(zz.shape[1], kk, np.float64) for zz, kk in zip(zs, ks)])[None, :]
    else:
        z, mag, k = sum(zs), sum(mags), float(sum(ks))
    if bias is not None:
        z = z + f64(bias)[None, :]
        mag = mag + np.abs(f64(bias))[None, :]
    if c_in is not None:
        assert not relu
        z = z + f64(c_in)
        mag = mag + np.abs(f64(c_in))
    want = np.maximum(z, 0.0) if relu else z
    return want, (k + 8.0) * U * mag + U * np.abs(want)


def wgrad(A_rows, dZ_cols):
    """gs_dense_wgrad over the given rows: A_rows [n, d] (gathered), dZ_cols [n, out] -> (want [d, out], bound).  Given one slab's
    row slice: that slab (K_total = its length).  Given all rows: the float64 sum of the slabs, which are fmaf chains over
    disjoint row slices, so K_total = n."""
    return product([(f64(A_rows).T, dZ_cols)])


def slab_rows(n, n_slabs):
    """Row slices of gs_dense_wgrad's split-K: slab z covers rows [z * kchunk, min(n, (z + 1) * kchunk)), kchunk =
    round_up(ceil(n / n_slabs), 32); trailing slabs may be empty (written as zeros)."""
    kchunk = (-(-n // n_slabs) + 31) // 32 * 32
    return [(min(z * kchunk, n), min((z + 1) * kchunk, n)) for z in range(n_slabs)]


LONG_N = 4096          # reductions from this length get the sparse dZ below


def edge_rows(n, n_slabs):
    """The rows of a split-K reduction where an off-by-one shows: the first two and last two rows of every slab, and the rows
    around every refill of the 1024-entry gather index cache (counted from the slab's first row)."""
    rows = set()
    for a, b in slab_rows(n, n_slabs):
        for r in (a, a + 1, b - 2, b - 1) + tuple(k + e for k in range(a + 1024, b, 1024) for e in (-1, 0, 1)):
            if a <= r < b:
                rows.add(r)
    return sorted(rows)


def wgrad_dz(rng, n, out, n_slabs):
    """dZ [n, out] of a weight-gradient case.  Standard normals below LONG_N rows.  From there the bound's (n + 8) u |A|^T |dZ| of
    dense unit operands (about +-10 per element at n = 16384) would hide a lost or foreign product (about 1), so dZ is
    ROW-SPARSE: zero except in one row of 64 drawn at random and in edge_rows(), the latter at 4 x the scale.  |A|^T |dZ| is then
    the sum over ~ n / 64 rows, the bound ~ 0.2, and any single product of an edge row that is lost, doubled, taken from the
    neighbouring slab or gathered through a wrong index is several times that.  The bound itself is not touched."""
    dZ = asym(rng, (n, out))
    if n >= LONG_N:
        live = rng.random(n) < 1.0 / 64
        edges = edge_rows(n, n_slabs)
        live[edges] = True
        dZ[~live] = 0
        dZ[edges] *= np.float32(4)
    return dZ


def gather_mean(X, idx, n, s, self_rows=None):
    """gs_gather_mean_fwd: (want [n, d], bound).  s (+1) fp32 additions, one multiplication by fp32(1 / s) (itself rounded:
    one more u), one stored rounding."""
    g = f64(X)[idx].reshape(n, s, -1)
    tot, mag, cnt = g.sum(axis=1), np.abs(g).sum(axis=1), s
    if self_rows is not None:
        tot, mag, cnt = tot + f64(self_rows), mag + np.abs(f64(self_rows)), s + 1
    want = tot / cnt
    return want, (cnt + 3.0) * U * mag / cnt + U * np.abs(want)


def pool_max(h, hb, s):
    """h, hb: relu'd activations [n * s, hid] and their bound -> (pooled want [n, hid], its bound, h3 [n, s, hid], hb3).
    |max_j a_j - max_j b_j| <= max_j |a_j - b_j|: the pooled bound is the group's largest elementwise bound."""
    h3, hb3 = h.reshape(-1, s, h.shape[1]), hb.reshape(-1, s, h.shape[1])
    return h3.max(axis=1), hb3.max(axis=1), h3, hb3


def argmax_acceptable(h3, hb3, arg):
    """The slack the pool arg-max needs: the kernel's activations differ from the reference's by <= bound each, so the kernel's
    winner j can be any index with ref[j] >= ref.max() - 2 * bound (bound: the larger of the two elements' bounds, taken here
    as the group's largest).  Returns the boolean [n, hid] mask of acceptable reports."""
    n, s, hid = h3.shape
    ok_range = (arg >= 0) & (arg < s)
    a = np.clip(arg, 0, s - 1)
    picked = np.take_along_axis(h3, a[:, None, :], axis=1)[:, 0, :]
    return ok_range & (picked >= h3.max(axis=1) - 2.0 * hb3.max(axis=1))


def worst(got, want, bound):
    """(largest err / bound, its index).  A NaN or infinity in `got` counts as infinitely wrong."""
    got, want, bound = f64(got), f64(want), f64(bound)
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    if got.size == 0:
        return 0.0, ()
    with np.errstate(invalid="ignore", over="ignore"):
        ratio = np.abs(got - want) / np.maximum(bound, np.finfo(np.float64).tiny)
    ratio[~(ratio >= 0)] = np.inf                      # NaN
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[i]), i


def within(got, want, bound):
    return worst(got, want, bound)[0] <= 1.0


def assert_within(got, want, bound, tag=""):
    """Every element inside its bound; reports the worst err / bound and its index.  Returns that ratio."""
    r, i = worst(got, want, bound)
    assert r <= 1.0, "%s: err / bound = %.4g at %s (got %r, want %r, bound %.3g)" % (
        tag, r, i, float(np.asarray(got)[i]), float(np.asarray(want)[i]), float(np.asarray(bound)[i]))
    return r


# ------------------------------------------------------------------------------------------------ fp32 emulation (CPU tests)
def chain(A, B, acc=None, ks=None):
    """The kernels' arithmetic in np.float32: acc = fmaf(A[:, k], B[k, :], acc) for k in order (the product is exact in float64,
    the sum is rounded once to fp32).  ks: the k indices this chain owns (default all)."""
    A64, B64 = f64(A), f64(B)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32) if acc is None else acc
    for k in (range(A.shape[1]) if ks is None else ks):
        acc = (acc.astype(np.float64) + A64[:, k, None] * B64[None, k, :]).astype(np.float32)
    return acc


def chain_small(terms):
    """gemm_small_kernel: wave w owns the 32-k stages w, w + 4, ... of every term; the four partial tiles are then summed in
    the fixed order ((p0 + p1) + p2) + p3."""
    parts = []
    for w in range(4):
        acc = None
        for A, B in terms:
            ks = [k for k in range(A.shape[1]) if (k // 32) % 4 == w]
            acc = chain(A, B, acc, ks)
        parts.append(acc)
    return ((parts[0] + parts[1]) + parts[2]) + parts[3]


def epilogue(acc, bias=None, relu=False, c_in=None):
    v = acc.astype(np.float32)
    if bias is not None:
        v = v + np.asarray(bias, np.float32)[None, :]
    if c_in is not None:
        v = v + np.asarray(c_in, np.float32)
    return np.maximum(v, np.float32(0)) if relu else v
