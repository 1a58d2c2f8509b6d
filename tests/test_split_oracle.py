"""CPU: the reference, the bound and the inputs of tests/split_oracle.py are fit for purpose -- the lattice inputs are exact, the
bound passes an fp32 emulation of the kernels' summation order on every input kind, and every planted fault fails on the input kind
that is there to catch it (the case named beside each fault is the one tests/test_split_edges_gpu.py runs on the device)."""
import numpy as np
import pytest

import gemm_oracle as go
import split_oracle as so
from oracle import split_pieces as sp

COUNT, K = 129, 65                                   # the star sweep's base case
N_OF = {"bf16": 100, "f16": 257}
_CACHE = {}


def _case(form, kind, N=None, K_=K, count=COUNT):
    """(Xg, W, bias, want, bound, mag), computed once per (form, kind, shape) and shared (read-only)."""
    N = N or N_OF[form]
    key = (form, kind, N, K_, count)
    if key not in _CACHE:
        rng = np.random.default_rng(len(_CACHE) + 11)
        Xg, W = so.inputs(kind, form, rng, count, K_, N)
        bias = go.asym(rng, (N,), 0.1) if kind in ("dense", "wild") else None
        want, bound, mag = so.reference(form, Xg, W, bias, relu=False)
        for a in (Xg, W, want, bound, mag):
            a.setflags(write=False)
        _CACHE[key] = (Xg, W, bias, want, bound, mag)
    return _CACHE[key]


def test_variant_and_schedule_restate_the_dispatch():
    assert so.variant("bf16", 255, False) == "bf16_narrow" and so.variant("bf16", 255, True) == "bf16_narrow"
    assert so.variant("bf16", 256, False) == "bf16_wide" and so.variant("bf16", 256, True) == "bf16_wide_tail"
    assert so.variant("f16", 1, False) == "f16_dma" and so.variant("f16", 1, True) == "f16_dma_tail"
    assert so.variant("f16r", 1, True) == "f16_staged_tail"
    assert [so.units("bf16", k) for k in (1, 32, 33, 64, 65, 128, 129, 602)] == [1, 1, 1, 1, 2, 2, 3, 10]
    assert [so.units("f16", k) for k in (1, 32, 33, 64, 65, 96, 97, 602)] == [1, 1, 2, 2, 3, 3, 4, 19]
    assert so.units("f16r", 602) == 10
    assert so.tiles("bf16", 129, 255) == 4 and so.tiles("bf16", 129, 257) == 4 and so.tiles("f16", 129, 100) == 2
    assert so.schedule(1300, 10, 256, True) == (1280, 20, 10)            # the pooling MLP: 20 tail tiles in 10 parts
    assert so.schedule(1300, 10, 256, False) == (1300, 0, 1)
    assert so.schedule(2, 1, 256, True) == (2, 0, 1)                      # one unit: nothing to cut
    assert so.schedule(2, 2, 256, True) == (0, 2, 2)
    assert so.schedule(26, 10, 256, True) == (0, 26, 9)                   # capped by n_cu / rem
    assert so.schedule(129, 10, 256, True) == (129, 0, 1)                 # 2 rem > n_cu
    assert so.schedule(512, 10, 256, True) == (512, 0, 1)                 # no incomplete round
    assert so.part_units(19, 10) == [(0, 1), (1, 3), (3, 5), (5, 7), (7, 9), (9, 11), (11, 13), (13, 15), (15, 17), (17, 19)]
    assert so.part_k("f16", 65, 3) == [(0, 32), (32, 64), (64, 65)] and so.part_k("bf16", 65, 2) == [(0, 64), (64, 65)]
    for u in range(1, 23):
        for S in range(1, min(u, 10) + 1):
            pu = so.part_units(u, S)
            assert pu[0][0] == 0 and pu[-1][1] == u and all(a < b for a, b in pu)
            assert all(pu[i][1] == pu[i + 1][0] for i in range(S - 1))


@pytest.mark.parametrize("form", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["lattice", "mirror"])
@pytest.mark.parametrize("K_", [1, 31, 65, 130])
def test_lattice_reference_is_exact(form, kind, K_):
    """The piece reference of a lattice input equals the float64 product exactly, and the product is an fp32 number: NO element is
    excluded from the bit comparison.  The one-hot column walks every k."""
    Xg, W, _, want, _, _ = _case(form, kind, K_=K_, count=131)
    exact = go.f64(Xg) @ go.f64(W)
    ok = (want == exact) & (exact.astype(np.float32).astype(np.float64) == exact) & (exact != 0)
    assert 1.0 - ok.mean() == 0.0
    assert set(np.nonzero(Xg)[1]) == set(range(K_)) and np.all((Xg != 0).sum(axis=1) == 1)
    # significant bits of the one-hot values / the dense side: 24 (bf16) or 22 (f16), or one (a power of two)
    full = Xg[Xg != 0] if kind == "lattice" else W
    m, _ = np.frexp(np.abs(full.astype(np.float64)))
    bits = 24 if form == "bf16" else 22
    assert np.all(m * 2.0 ** bits % 2 == 1)
    pow2 = W if kind == "lattice" else Xg[Xg != 0]
    assert np.all(np.frexp(np.abs(pow2))[0] == 0.5) and np.abs(np.log2(np.abs(pow2))).max() <= 4


@pytest.mark.parametrize("form", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["sparse_k", "dense", "wild"])
def test_pieces_stay_close_to_the_plain_product(form, kind):
    """What the arithmetic gives up by design is below 2^-22 of |x| . |w| on the dense kinds.  sparse_k is built to have ONE or TWO
    full-mantissa products per output, where the per-product worst case applies instead: m l' + l m' + l l' with |m| < 2^-7 |h|,
    |l| < 2^-15 |h| (bf16: 2 * 2^-22 + 2^-30), or m m' with |m| <= 2^-11 |h| plus the last bit of either operand, 2^-23 each
    (f16: 2^-22 + 2 * 2^-23), i.e. 2^-21 of the product up to second-order terms (1 + 2^-7)."""
    Xg, W, bias, want, _, mag = _case(form, kind)             # mag = |x| . |w| + |bias|
    plain = go.f64(Xg) @ go.f64(W) + (0 if bias is None else go.f64(bias))
    lim = 2.0 ** -21 * (1 + 2.0 ** -7) if kind == "sparse_k" else 2.0 ** -22
    print("\ndesign loss / mag %-5s %-9s 2^%.2f" % (form, kind, np.log2((np.abs(want - plain) / np.maximum(mag, 1e-300)).max())), end="")
    assert np.all(np.abs(want - plain) <= lim * mag)
    if kind == "sparse_k":
        assert ((Xg != 0).sum(axis=1) <= 2).all() and set(np.nonzero(Xg)[1]) == set(so.stage_edges(K))
        assert so.stage_edges(65) == [0, 31, 32, 63, 64] and so.stage_edges(1) == [0]
    if kind == "wild":
        e = sp.cut_rows_f16(Xg)[2]
        c = sp.cut_cols_f16(W)[2]
        live_r, live_c = np.abs(Xg).max(axis=1) > 0, np.abs(W).max(axis=0) > 0
        assert (~live_r).sum() == 1 and (~live_c).sum() == 1 and e[~live_r][0] == 0 and c[~live_c][0] == 0
        assert np.all(e[:-1] != e[1:]) and np.all(c[:-1] != c[1:])               # neighbours never share an exponent
        assert e[live_r].max() - e[live_r].min() > 60 and c[live_c].max() - c[live_c].min() > 40


def _parts(form, S):
    return so.part_k(form, K, S) if S > 1 else None


@pytest.mark.parametrize("form,S", [("bf16", 1), ("bf16", 2), ("f16", 1), ("f16", 3), ("f16r", 2)])
@pytest.mark.parametrize("kind", so.KINDS)
def test_emulation_passes_the_bound(form, S, kind):
    """fp32 accumulation in the kernels' order (separate h-h and small-term accumulators, k ascending, parts in part order) is
    inside the bound on every input kind, and bit-exact on the lattice."""
    f = "f16" if form == "f16r" else form
    Xg, W, bias, want, bound, _ = _case(f, kind)
    for relu in (False, True):
        got = so.emulate(f, Xg, W, bias, relu, _parts(form, S))
        w = np.maximum(want, 0) if relu else want
        r = go.assert_within(got, w, bound, "%s S=%d %s" % (form, S, kind))
        if kind in ("lattice", "mirror"):
            assert so.same_bits(got, w.astype(np.float32))
    print("\nemulation err/bound %-6s S=%d %-9s %.4f" % (form, S, kind, r), end="")


def _caught(form, kind, fault, S=1, exact=False):
    f = "f16" if form == "f16r" else form
    Xg, W, bias, want, bound, _ = _case(f, kind)
    got = so.emulate(f, Xg, W, bias, False, _parts(form, S), fault)
    assert go.within(so.emulate(f, Xg, W, bias, False, _parts(form, S)), want, bound)
    return (not so.same_bits(got, want.astype(np.float32))) if exact else (not go.within(got, want, bound))


# fault -> the input kind whose check must catch it (bound; "exact": the lattice's bit comparison)
@pytest.mark.parametrize("form,name", [("bf16", n) for n in ("hh",) + so.BF16_SMALL] + [("f16", n) for n in ("hh",) + so.F16_SMALL])
def test_a_dropped_piece_product_is_caught(form, name):
    """One kept piece product dropped at one k (the last k of the first stage: live in sparse_k).  sparse_k's bound catches every
    one of them; the lattice's bit comparison catches those that are live there (one side is a power of two: no m m')."""
    k = 31
    assert _caught(form, "sparse_k", {"drop": (name, k)})
    if name[1] == "h":                                   # X carries the mantissa in `lattice`
        assert _caught(form, "lattice", {"drop": (name, k)}, exact=True)
    if name[0] == "h":                                   # W carries it in `mirror`
        assert _caught(form, "mirror", {"drop": (name, k)}, exact=True)
    if name in ("hl", "lh", "mm"):                       # ... and the dense kinds do NOT see 2^-16 of one product: why sparse_k exists
        assert not _caught(form, "dense", {"drop": (name, k)})


@pytest.mark.parametrize("form", ["bf16", "f16"])
def test_schedule_and_staging_faults_are_caught(form):
    for kind in ("lattice", "sparse_k"):
        assert _caught(form, kind, {"skip_last_group": True}, exact=(kind == "lattice"))
        assert _caught(form, kind, {"shift_stage": 0}, exact=(kind == "lattice"))
        assert _caught(form, kind, {"shift_stage": 1}, exact=(kind == "lattice"))
    S = 3 if form == "f16" else 2
    for p in range(S):
        for kind in ("lattice", "mirror", "sparse_k", "dense"):
            assert _caught(form, kind, {"lose_part": p}, S, exact=kind in ("lattice", "mirror")), (kind, p)
            assert _caught(form, kind, {"dup_part": p}, S, exact=kind in ("lattice", "mirror")), (kind, p)


def test_a_foreign_scale_exponent_is_caught():
    """The neighbouring row's exponent, or column N - 1's for the column beside it (the epilogue clamps the exponent index of pad
    columns to N - 1): `wild` gives neighbours different exponents."""
    assert _caught("f16", "wild", {"row_exp": True})
    assert _caught("f16", "wild", {"col_exp": True})


def test_a_write_outside_the_block_is_caught():
    count, n_rows, N = 129, 300, 257
    buf = so.frame(n_rows, N)
    assert buf.shape == (n_rows + 5, 260 + 12)
    buf[2:2 + count, :N] = 1.0
    assert so.read_frame(buf, count, N).shape == (count, N)
    for r, c in ((2 + count, 0), (2 + n_rows, 5), (1, 0), (2, N), (2 + count - 1, buf.shape[1] - 1), (2 + 17, 259)):
        bad = buf.copy()
        bad[r, c] = 0.0                                  # a row >= count | the row behind the buffer's rows | above | a column in [N, ldo)
        with pytest.raises(AssertionError):
            so.read_frame(bad, count, N)
    assert so.frame(4, 257, tight=True).shape == (9, 260)
