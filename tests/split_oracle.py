"""NumPy restatement of what the split contractions on gathered rows promise (csrc/gs_split.hip: gs_dense_fwd_rows_split[_ws];
csrc/gs_split16.hip: gs_dense_fwd_rows_split16): which kernel a call runs, how its tail round is cut, a float64 reference, ONE derived
elementwise bound, the inputs that make a small fault visible, a sentinel frame and an fp32 emulation of the kernels' summation order
with planted faults (tests/test_split_oracle.py shows that the bound passes the emulation and fails every fault).  No GPU, no torch.

Reference.  want = act(pieces(X[idx], W) + bias) in float64, where `pieces` is oracle/split_pieces.py's exact sum of the KEPT piece
products (six of nine for three bf16 pieces, three of four for two fp16 pieces under row / column scales): what the arithmetic gives
up by design -- the dropped products, the last operand bit of the fp16 cut -- is in the reference, not in the tolerance.

Bound (the only tolerance of tests/test_split_edges_gpu.py), in float64, u = 2^-24:

    |got - want| <= 2 (n_live + 8) u mag + u |want|,     mag = |X[idx]| @ |W| + |bias|,     n_live = (X[idx] != 0) @ (W != 0)

  * a zero operand has zero pieces and every product with it is exactly zero: it adds exactly nothing to an accumulator, so only the
    n_live products of an output element can cost a rounding;
  * the piece products of a live product are exact (8 x 8 or 11 x 11 bits) and each enters an fp32 accumulator once (the h-h one or
    the small-terms one), so the chain that an addend passes through has at most n_live additions that are not additions of zero;
  * how v_mfma_f32_32x32x16_{bf16,f16} rounds the sum of its 16 products into the accumulator is not documented in our guides.
    Whether each addition rounds to nearest (u of the running sum) or truncates (one ulp = 2u), it loses at most 2u of a running sum
    that is itself bounded by mag: hence the factor 2;
  * + 8, i.e. 16 u mag: what follows the MFMAs is plain fp32 addition, round to nearest, u each -- acc + sml (once per part, each
    relative to its own part of mag: one u mag in all), up to nine additions of the ten part sums, the bias: at most 11 u mag; and
    u |want| for the stored value (relu is exact and 1-Lipschitz; the scale-back by 2^-(e_row + e_col) is exact in the normal range).
The bound is NOT tuned to what the device gives; profiles/split_edges.md records the largest err / bound per variant as a figure.

Inputs.
  lattice   X one-hot per row at kappa(row) = (K - 1 - row) mod K (walks every k < K from the last one down), value with exactly 24
            (bf16) / 22 (f16) significant bits; W dense, +-2^p with |p| <= 4.  Every output is ONE product whose pieces sum to it
            exactly: the device must return float32(x * w) bit for bit, through acc + sml, every split-K part and the scale-back.
            mirror=True swaps the roles: X one-hot with +-2^p, W dense with full-width mantissas in [1, 8).
  sparse_k  two live k per X row, drawn from the first and last k of every 32-k stage and K - 1; full 24-bit mantissas on both
            sides, so m m' and both cross terms are live and n_live <= 2: the bound is ~2^-19.7 of two products.
  dense     asymmetric normals; wild=True: row scales 2^+-40 (neighbouring rows differ), column scales 2^+-30 (neighbouring
            columns differ), an all-zero row and an all-zero column."""
import numpy as np

import gemm_oracle as go
from oracle import split_pieces as sp

U = go.U
SENTINEL = go.SENTINEL
FORMS = ("bf16", "f16", "f16r")            # three bf16 pieces | two fp16 pieces, LDS-DMA form | ... register-staged form (GS_SPLIT16_DMA=0)
KINDS = ("lattice", "mirror", "sparse_k", "dense", "wild")
BF16_SMALL = ("hl", "lh", "mm", "hm", "mh")          # the small-terms accumulator's products, in the kernels' order
F16_SMALL = ("hm", "mh")


def cdiv(a, b):
    return -(-a // b)


def round_up(x, m):
    return cdiv(x, m) * m


# ------------------------------------------------------------------------------------------------ dispatch and schedule
def variant(form, N, ws):
    """The kernel a call runs (dense_fwd_rows_split_impl / gs_dense_fwd_rows_split16): a name per instantiation and tail-round use.
    `ws`: the call passes a workspace that is large enough."""
    if form == "bf16":
        if N < 256:
            return "bf16_narrow"                       # split_tiled_fwd_kernel: never a tail round
        return "bf16_wide_tail" if ws else "bf16_wide"
    assert form in ("f16", "f16r")
    return ("f16_dma" if form == "f16" else "f16_staged") + ("_tail" if ws else "")


def units(form, K):
    """What a tail-round tile is cut into: stage pairs for the bf16 forms and the register-staged f16 form, stages for the DMA form."""
    stages = cdiv(K, 32)
    return stages if form == "f16" else ((stages + 1) & ~1) // 2


def tiles(form, count, N):
    """Workgroup tiles of a call: 128 x 128 in the narrow bf16 form, 128 x 256 everywhere else."""
    return cdiv(count, 128) * cdiv(N, 128 if (form == "bf16" and N < 256) else 256)


def schedule(nwg, units_, n_cu, have_ws):
    """wide_schedule / split16_schedule restated: (full, rem, S) -- tiles [0, full) whole, the rem tiles behind them in S parts."""
    if have_ws and n_cu > 0:
        r = nwg % n_cu
        if r > 0 and 2 * r <= n_cu:
            sp_ = min(units_, n_cu // r, 10)
            if sp_ >= 2:
                return nwg - r, r, sp_
    return nwg, 0, 1


def part_units(units_, S):
    """Part p covers the units [units p / S, units (p + 1) / S)."""
    return [(units_ * p // S, units_ * (p + 1) // S) for p in range(S)]


def part_k(form, K, S):
    """The k ranges of the S parts of a tail-round tile (clipped to K)."""
    per = 32 if form == "f16" else 64
    return [(min(K, per * a), min(K, per * b)) for a, b in part_units(units(form, K), S)]


# ------------------------------------------------------------------------------------------------ reference and bound
def pieces(form):
    return sp.matmul_three_pieces if form == "bf16" else sp.matmul_two_pieces


def reference(form, Xg, W, bias=None, relu=False):
    """(want, bound, mag) float64 [rows, N] for the logical operands Xg = X[idx] [rows, K] and W [K, N]."""
    Xg, W = np.asarray(Xg, np.float32), np.asarray(W, np.float32)
    z = pieces(form)(Xg, W)
    mag = np.abs(go.f64(Xg)) @ np.abs(go.f64(W))
    n_live = (Xg != 0).astype(np.float64) @ (W != 0).astype(np.float64)
    if bias is not None:
        z = z + go.f64(bias)[None, :]
        mag = mag + np.abs(go.f64(bias))[None, :]
    want = np.maximum(z, 0.0) if relu else z
    return want, 2.0 * (n_live + 8.0) * U * mag + U * np.abs(want), mag


def same_bits(a, b):
    """Bit equality of two float32 arrays (-0 counts as +0: relu and an empty accumulator give +0)."""
    a, b = np.asarray(a, np.float32) + np.float32(0), np.asarray(b, np.float32) + np.float32(0)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ inputs
def _signs(rng, shape):
    return np.where(rng.integers(0, 2, size=shape) == 1, 1.0, -1.0)


def _mantissas(rng, shape, bits):
    """Values in [1, 2) with exactly `bits` significant bits (the last one set)."""
    return (rng.integers(2 ** (bits - 1), 2 ** bits, size=shape) | 1) * 2.0 ** -(bits - 1)


def kappa(rows, K):
    return (K - 1 - np.arange(rows)) % K


def lattice(form, rng, rows, K, N, mirror=False):
    """(X [rows, K], W [K, N]) float32, see the module docstring."""
    bits = 24 if form == "bf16" else 22
    X = np.zeros((rows, K), np.float64)
    if not mirror:
        val = _signs(rng, rows) * _mantissas(rng, rows, bits) * 2.0 ** rng.integers(-3, 4, size=rows)
        W = _signs(rng, (K, N)) * 2.0 ** rng.integers(-4, 5, size=(K, N))
    else:
        val = _signs(rng, rows) * 2.0 ** rng.integers(-4, 5, size=rows)
        W = _signs(rng, (K, N)) * _mantissas(rng, (K, N), bits) * 2.0 ** rng.integers(0, 3, size=(K, N))
    X[np.arange(rows), kappa(rows, K)] = val
    X32, W32 = X.astype(np.float32), W.astype(np.float32)
    assert np.array_equal(X32, X) and np.array_equal(W32, W)
    return X32, W32


def stage_edges(K):
    """The first and last k of every 32-k stage, and K - 1."""
    ks = set([K - 1])
    for s in range(cdiv(K, 32)):
        ks.add(32 * s)
        ks.add(min(32 * s + 31, K - 1))
    return sorted(ks)


def sparse_k(rng, rows, K, N):
    """(X, W): row r of X is live at two consecutive members of stage_edges(K) (one if there is only one)."""
    P = stage_edges(K)
    X = np.zeros((rows, K), np.float64)
    r = np.arange(rows)
    for off in (0, 1):
        k = np.asarray(P)[(r + off) % len(P)]
        X[r, k] = _signs(rng, rows) * _mantissas(rng, rows, 24) * 2.0 ** rng.integers(-2, 3, size=rows)
    W = _signs(rng, (K, N)) * _mantissas(rng, (K, N), 24) * 2.0 ** rng.integers(-2, 3, size=(K, N))
    return X.astype(np.float32), W.astype(np.float32)


def dense(rng, rows, K, N, wild=False):
    X, W = go.asym(rng, (rows, K)), go.asym(rng, (K, N), 0.1)
    if wild:
        # neighbours differ by 4 mod 8 / 3 mod 6: more than the largest elements of two rows / columns of normals differ by
        re = 8 * rng.integers(-5, 6, size=rows) + 4 * (np.arange(rows) & 1)
        ce = 6 * rng.integers(-5, 6, size=N) + 3 * (np.arange(N) & 1)
        X = np.ldexp(X, re[:, None].astype(np.int32)).astype(np.float32)
        W = np.ldexp(W, ce[None, :].astype(np.int32)).astype(np.float32)
        X[rows // 2] = 0
        W[:, N // 3] = 0
    return X, W


def inputs(kind, form, rng, rows, K, N):
    if kind in ("lattice", "mirror"):
        return lattice(form, rng, rows, K, N, mirror=(kind == "mirror"))
    if kind == "sparse_k":
        return sparse_k(rng, rows, K, N)
    return dense(rng, rows, K, N, wild=(kind == "wild"))


def gather_plan(rng, n_rows, gathered):
    """(table rows, idx or None): idx [n_rows] with repeats, out of order, pointing at the last table row and leaving some rows
    of the table unreferenced; None: the table's first n_rows rows are the operand."""
    if not gathered:
        return n_rows, None
    n_table = n_rows + 7
    idx = rng.permutation(n_table)[:n_rows].astype(np.int32)
    if n_rows >= 3:
        idx[n_rows // 2] = idx[0]                      # a repeat
    idx[-1] = n_table - 1                              # the last table row
    return n_table, idx


# ------------------------------------------------------------------------------------------------ the sentinel frame
def frame(n_rows, N, tight=False):
    """A [n_rows, N] output two rows down a sentinel-filled [n_rows + 5, ldo] buffer, ldo = round_up(N, 4) + 12 (tight: + 0)."""
    return np.full((n_rows + 5, round_up(N, 4) + (0 if tight else 12)), SENTINEL, np.float32)


def read_frame(buf, count, N, tag=""):
    """The written block [count, N] after checking that every other word -- rows >= count, columns [N, ldo), the rows above and
    below -- still holds the sentinel."""
    for name, part in (("above", buf[:2]), ("rows >= count", buf[2 + count:]), ("columns [N, ldo)", buf[2:2 + count, N:])):
        assert np.all(part == SENTINEL), "%s: %d words written %s" % (tag, int((part != SENTINEL).sum()), name)
    return buf[2:2 + count, :N]


# ------------------------------------------------------------------------------------------------ fp32 emulation (CPU tests)
def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def emulate(form, Xg, W, bias=None, relu=False, kparts=None, fault=None):
    """The kernels' summation order in fp32: per part, k ascending, the h-h products into one accumulator and the small terms into
    another, acc + sml per part, the parts summed in part order, (scale-back,) bias, activation.  One rounding per k and accumulator
    -- the device rounds once per MFMA (16 k), so this is the longer chain.
    fault (planted, one key): drop=(product, k) | skip_last_group | shift_stage=s (A's stage s meets B's stage s + 1) |
    lose_part=p | dup_part=p | row_exp (the neighbouring row's exponent) | col_exp (column N - 1's exponent for column N - 2)."""
    fault = fault or {}
    Xg, W = np.asarray(Xg, np.float32), np.asarray(W, np.float32)
    M, K = Xg.shape
    N = W.shape[1]
    re = ce = None
    if form == "bf16":
        xp = dict(zip("hml", (a.astype(np.float64) for a in sp.cut_bf16x3(Xg))))
        wp = dict(zip("hml", (a.astype(np.float64) for a in sp.cut_bf16x3(W))))
        small = BF16_SMALL
    else:
        hx, mx, re = sp.cut_rows_f16(Xg)
        hw, mw, ce = sp.cut_cols_f16(W)
        xp = {"h": hx.astype(np.float64), "m": mx.astype(np.float64)}
        wp = {"h": hw.astype(np.float64), "m": mw.astype(np.float64)}
        small = F16_SMALL
    zero_row = np.zeros(N)

    def prod(name, k, kb):
        if fault.get("drop") == (name, k):
            return 0.0
        return np.outer(xp[name[0]][:, k], wp[name[1]][kb] if kb < K else zero_row)

    total = None
    for p, (k0, k1) in enumerate(kparts or [(0, K)]):
        acc, sml = np.zeros((M, N), np.float32), np.zeros((M, N), np.float32)
        for k in range(k0, min(k1, K)):
            if fault.get("skip_last_group") and k >= 8 * ((K - 1) // 8):
                continue
            kb = k + 32 if fault.get("shift_stage") == k // 32 else k
            acc = _f32(acc.astype(np.float64) + prod("hh", k, kb))
            sml = _f32(sml.astype(np.float64) + sum(prod(nm, k, kb) for nm in small))
        v = _f32(acc.astype(np.float64) + sml)
        for _ in range(0 if fault.get("lose_part") == p else 2 if fault.get("dup_part") == p else 1):
            total = v if total is None else _f32(total.astype(np.float64) + v)
    if total is None:
        total = np.zeros((M, N), np.float32)
    if re is not None:
        if fault.get("row_exp"):
            re = np.roll(re, -1)
        if fault.get("col_exp"):
            ce = ce.copy()
            ce[N - 2] = ce[N - 1]
        total = _f32(np.ldexp(total.astype(np.float64), -(re[:, None].astype(np.int64) + ce[None, :])))
    if bias is not None:
        total = _f32(total.astype(np.float64) + go.f64(bias)[None, :])
    return np.maximum(total, np.float32(0)) if relu else total
