"""-m gpu: the split contractions on gathered rows (csrc/gs_split.hip: gs_dense_fwd_rows_split[_ws]; csrc/gs_split16.hip:
gs_dense_fwd_rows_split16) and their cut kernels against tests/split_oracle.py, element by element, at the edges of every kernel.

Every contraction case
  * reads X from a table with ldx = round_up(K, 4) + 12 in which EVERYTHING outside the logical operand is NaN: pad columns, the
    table rows that no index points at, the row after the last one (split16: that table goes through gs_split_table_f16 first);
    W has ldw = N + 5 with NaN pads and a NaN row behind it; the bias has NaN on both sides;
  * writes two rows down a sentinel-filled [n_max + 5, round_up(N, 4) + 12] buffer (one tight case per entry point): afterwards
    the block [count, N] is inside split_oracle's derived bound -- the only tolerance here -- or BIT-equal to float32(x * w) for the
    lattice inputs, and every other word, columns [N, ldo) and rows >= count included, still holds the sentinel;
  * runs twice and gives the same bits.
tests/test_split_oracle.py shows on the CPU that these checks pass the kernels' arithmetic and fail each planted fault.

Instantiation -> cases (`so.variant` restates the dispatch; the tail round is reached by shape, see test_tail_cases_reach_*):
  split_tiled_fwd_kernel (bf16, N < 256)     test_star[narrow-*]: count {1..257}, (n_max, n_dev), K {1..130}, N {1..255}
  split_tiled_fwd_wide_kernel (N >= 256)     test_star[wide-*]: the same rows / K, N {256..513}, each with and without a workspace;
                                             test_tail_round[bf16-*]
  split_tiled_fixup_kernel                   test_star[wide-*] (workspace: S = 2 from K = 65), test_tail_round[bf16-s2|s10|s10u|cap]
  split16_dma_fwd_kernel                     test_star[f16-*] (N {1..513}), test_tail_round[f16-*], test_split16_tail_round_mixes_*
  split16_fixup_kernel                       test_star[f16-*] (workspace), test_tail_round[f16-s2|s3|s3b|s10|cap], ..._mixes_*
  split16_tiled_fwd_kernel (GS_SPLIT16_DMA=0) test_register_staged_split16_form (one child process, bit equality with the DMA form)
  split_rows_kernel, split16_rows_kernel     test_cut_rows: K {1..130} x N {1..257}, bit-equal to oracle/split_pieces.py
  split16_table_kernel                       test_cut_table: d {1..130} x rows {1..9}

Every test prints the largest err / bound it met per variant (pytest -s); profiles/split_edges.md keeps those figures."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from graphsage_amd import ops
from graphsage_amd.ops import round_up
import gemm_oracle as go
import split_oracle as so
from oracle import split_pieces as sp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAN = np.float32("nan")
ISENT = np.int32(-1234567)
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


def n_cu_of():
    return ops.split_tiled_ws_words() // (128 * 256)


_WS = {}


def workspace(dev):
    """The tail round's workspace (one partial tile per CU), NaN-filled before every use."""
    if dev not in _WS:
        _WS[dev] = torch.empty(ops.split_tiled_ws_words(), dtype=torch.float32, device=dev)
    _WS[dev].fill_(float("nan"))
    return _WS[dev]


# ------------------------------------------------------------------------------------------------ operands on the device
def cut_w(form, W, dev, tail_words=64):
    """W [K, N] in a NaN-padded [K + 1, N + 5] buffer -> (cut weights as an int32 tensor with `tail_words` sentinel words behind
    the entry point's own byte count, that count in words)."""
    K, N = W.shape
    buf = np.full((K + 1, N + 5), NAN, np.float32)
    buf[:K, :N] = W
    t = _dev(buf, dev)
    words = ops.split_rows_words(K, N) if form == "bf16" else ops.split_rows_f16_words(K, N)
    out = torch.full((words + tail_words,), int(ISENT), dtype=torch.int32, device=dev)
    ops.call("gs_split_rows" if form == "bf16" else "gs_split_rows_f16", t.data_ptr(), N + 5, K, N, out.data_ptr(), _st())
    return out, words


def cut_table(buf, d, ldx, dev, tail_words=64):
    """A [rows, ldx] fp32 device table of logical width d -> (X2, rexp, table words, exponent words) with sentinel tails."""
    rows = buf.shape[0]
    tb, eb = ctypes.c_int64(), ctypes.c_int64()
    ops.call("gs_split_table_f16_bytes", rows, d, ctypes.byref(tb), ctypes.byref(eb))
    tw, ew = int(tb.value) // 4, int(eb.value) // 4
    X2 = torch.full((tw + tail_words,), int(ISENT), dtype=torch.int32, device=dev)
    rexp = torch.full((ew + tail_words,), int(ISENT), dtype=torch.int32, device=dev)
    ops.call("gs_split_table_f16", buf.data_ptr(), ldx, rows, d, X2.data_ptr(), rexp.data_ptr(), _st())
    return X2, rexp, tw, ew


class Problem(object):
    """One contraction's operands on the host (logical) and on the device (padded, NaN everywhere else)."""

    def __init__(self, form, kind, dev, n_max, K, N, gathered, bias, seed):
        f = "f16" if form == "f16r" else form
        rng = np.random.default_rng(seed)
        n_table, idx = so.gather_plan(rng, n_max, gathered)
        T, W = so.inputs(kind, f, rng, n_table, K, N)
        self.form, self.f, self.kind, self.K, self.N, self.n_max = form, f, kind, K, N, n_max
        self.Xg = T[idx] if gathered else T                    # [n_max, K]
        self.W = W
        self.b = go.asym(rng, (N,), 0.1) if bias else None
        ldx = round_up(K, 4) + 12
        buf = np.full((n_table + 1, ldx), NAN, np.float32)
        live = np.unique(idx) if gathered else np.arange(n_table)
        buf[live, :K] = T[live]
        self.xt = _dev(buf, dev)
        self.idx_t = _dev(idx, dev) if gathered else None
        self.keep = [self.xt, self.idx_t]
        if f == "bf16":
            self.w, _ = cut_w("bf16", W, dev)
            self.x_args = (self.xt.data_ptr(), ldx)
        else:
            self.w, _ = cut_w("f16", W, dev)
            X2, rexp, _, _ = cut_table(self.xt, K, ldx, dev)
            self.keep += [X2, rexp]
            self.x_args = (X2.data_ptr(), rexp.data_ptr())
        self.bias_t = None
        if bias:
            self.bias_t = _dev(np.concatenate([np.full(4, NAN, np.float32), self.b, np.full(4, NAN, np.float32)]), dev)
        self.dev = dev
        self.refs = {}                                         # (count, relu) -> (want, bound): computed once, read-only

    def run(self, count_dev, relu, tight=False, ws=None, ws_bytes=None):
        """One call into a fresh sentinel frame -> the frame as a NumPy array.  count_dev: None (n_dev = NULL) or the device count."""
        dev = self.dev
        fr = _dev(so.frame(self.n_max, self.N, tight), dev)
        ldo = fr.shape[1]
        out_ptr = fr.data_ptr() + 2 * ldo * 4
        cnt = _dev(np.asarray([count_dev], np.int32), dev) if count_dev is not None else None
        bptr = self.bias_t.data_ptr() + 16 if self.bias_t is not None else None
        act = RELU if relu else ID
        wsp = ws.data_ptr() if ws is not None else None
        wsb = (4 * ws.numel() if ws_bytes is None else ws_bytes) if ws is not None else 0
        common = (ops.ptr(self.idx_t), self.K, self.n_max, ops.ptr(cnt), self.w.data_ptr(), self.N, act, bptr, out_ptr, ldo)
        if self.f == "bf16":
            if ws is not None:
                ops.call("gs_dense_fwd_rows_split_ws", *(self.x_args + common + (wsp, wsb, _st())))
            else:
                ops.call("gs_dense_fwd_rows_split", *(self.x_args + common + (_st(),)))
        else:
            ops.call("gs_dense_fwd_rows_split16", *(self.x_args + common + (wsp, wsb, _st())))
        torch.cuda.synchronize()
        return fr.cpu().numpy()

    def check(self, count_dev, relu, tight=False, ws=None, ws_bytes=None, tag=""):
        """Runs twice, checks the frame and the block (bound, or bits for the lattice kinds) -> the block."""
        count = self.n_max if count_dev is None else min(self.n_max, count_dev)
        tag = "%s %s %s count=%d n_max=%d K=%d N=%d ws=%s" % (tag, self.form, self.kind, count, self.n_max, self.K, self.N,
                                                               ws is not None)
        a = self.run(count_dev, relu, tight, ws, ws_bytes)
        b = self.run(count_dev, relu, tight, ws, ws_bytes)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), tag + ": two runs differ"
        got = so.read_frame(a, count, self.N, tag)
        if (count, relu) not in self.refs:
            self.refs[(count, relu)] = so.reference(self.f, self.Xg[:count], self.W, self.b, relu)[:2]
        want, bound = self.refs[(count, relu)]
        splits = ws is not None and (ws_bytes is None or ws_bytes >= 4 * ws.numel())
        r = go.assert_within(got, want, bound, tag)
        _note(so.variant(self.form, self.N, splits), r)
        if self.kind in ("lattice", "mirror"):
            assert self.b is None
            assert so.same_bits(got, want.astype(np.float32)), "%s: %d outputs are not float32(x * w)" % (
                tag, int((got != want.astype(np.float32)).sum()))
        return got


# ------------------------------------------------------------------------------------------------ the star sweep
BASE = {"narrow": ("bf16", 100), "wide": ("bf16", 257), "f16": ("f16", 257)}
ROWS = [1, 127, 128, 129, 257]
NDEV = [(129, None), (300, 129), (300, 0), (128, 500)]
KS = [1, 3, 4, 8, 31, 32, 33, 63, 64, 65, 96, 97, 130]
NS = {"narrow": [1, 3, 4, 64, 100, 127, 128, 129, 252, 255], "wide": [256, 257, 260, 511, 513],
      "f16": [1, 3, 4, 63, 65, 100, 255, 256, 257, 513]}
STAR = [(arm, fac, v) for arm in ("narrow", "wide", "f16")
        for fac, vals in (("rows", ROWS), ("ndev", NDEV), ("K", KS), ("N", NS[arm])) for v in vals]


def _star_id(c):
    v = c[2]
    return "%s-%s-%s" % (c[0], c[1], "x".join(str(x) for x in v) if isinstance(v, tuple) else v)


@pytest.mark.parametrize("case", list(enumerate(STAR)), ids=[_star_id(c) for c in STAR])
def test_star(dev, case):
    """One factor away from (count 129, K 65, N 100 | 257) per case; every input kind; the rows arm alternates n_dev = NULL
    with a device-side count below n_max; gathered idx (repeats, out of order, the
    last table row) alternates with idx = NULL, bias with none, relu with identity; the first case of each arm is the tight one;
    the wide and f16 arms run with and without a workspace (a tail round of S = min(units, 10) parts on every tile)."""
    i, (arm, fac, v) = case
    form, N = BASE[arm]
    n_max, n_dev, K = 129, None, 65
    if fac == "rows":
        n_max, n_dev = (v + 43, v) if i & 1 else (v, None)         # the count from the device, or n_max itself
    elif fac == "ndev":
        n_max, n_dev = v
    elif fac == "K":
        K = v
    else:
        N = v
    for j, kind in enumerate(so.KINDS):
        lat = kind in ("lattice", "mirror")
        p = Problem(form, kind, dev, n_max, K, N, gathered=((i + j) & 1) == 0, bias=(not lat) and ((i >> 1) + j) & 1 == 0,
                    seed=1000 * i + j)
        relu = ((i + j // 2) & 1) == 1
        tight = (fac, v) == ("rows", 1)
        plain = p.check(n_dev, relu, tight, tag="star")
        if arm != "narrow":
            split = p.check(n_dev, relu, tight, ws=workspace(dev), tag="star")
            n_cu = n_cu_of()
            count = n_max if n_dev is None else min(n_max, n_dev)
            S = so.schedule(so.tiles(form, count, N), so.units(form, K), n_cu, True)[2]
            if S == 1 or lat:
                assert so.same_bits(plain, split)


# ------------------------------------------------------------------------------------------------ the tail round
def tail_cases(n_cu):
    """name -> (form, count, K, N, how the workspace is passed).  Shapes by the chip's CU count; the expectations are asserted from
    so.schedule in test_tail_cases_reach_every_schedule."""
    cap_tiles = 26 if n_cu == 256 else max(1, n_cu // 9)
    big = 128 * (n_cu // 2 + 1) - 37
    return {
        "bf16-s1": ("bf16", 129, 64, 257, "ws"), "f16-s1": ("f16", 129, 32, 257, "ws"),
        "bf16-s2": ("bf16", 129, 65, 257, "ws"), "f16-s2": ("f16", 129, 64, 257, "ws"),
        "f16-s3": ("f16", 129, 65, 257, "ws"), "f16-s3b": ("f16", 100, 96, 200, "ws"),
        "bf16-s10": ("bf16", 100, 602, 256, "ws"), "f16-s10": ("f16", 100, 602, 200, "ws"),
        "bf16-s10u": ("bf16", 100, 700, 300, "ws"),
        "bf16-cap": ("bf16", 128 * cap_tiles - 37, 602, 256, "ws"), "f16-cap": ("f16", 128 * cap_tiles - 37, 602, 200, "ws"),
        "bf16-nosplit": ("bf16", big, 65, 256, "ws"), "f16-nosplit": ("f16", big, 65, 200, "ws"),
        "bf16-short": ("bf16", 129, 65, 257, "short"), "f16-short": ("f16", 129, 65, 257, "short"),
    }


TAIL_NAMES = sorted(tail_cases(256))


def _tail_schedule(form, count, K, N, n_cu):
    return so.schedule(so.tiles(form, count, N), so.units(form, K), n_cu, True)


def test_tail_cases_reach_every_schedule(dev):
    """From so.schedule and the chip's CU count: the tail cases below reach S = 1 with a workspace, S = 2, S = 3 with one-stage
    parts, S = 10 with unequal parts, S capped by n_cu / rem, and 2 rem > n_cu (no split)."""
    n_cu = n_cu_of()
    assert n_cu >= 64
    tc = tail_cases(n_cu)
    sch = {name: _tail_schedule(c[0], c[1], c[2], c[3], n_cu) for name, c in tc.items()}
    for f in ("bf16", "f16"):
        assert sch[f + "-s1"] == (4, 0, 1) and so.units(f, tc[f + "-s1"][2]) == 1
        assert sch[f + "-s2"] == (0, 4, 2)
        full, rem, S = sch[f + "-cap"]
        assert full == 0 and rem > 0 and S == n_cu // rem and 2 <= S < min(so.units(f, 602), 10)
        full, rem, S = sch[f + "-nosplit"]
        assert (rem, S) == (0, 1) and 2 * (full % n_cu) > n_cu
        assert sch[f + "-short"][2] >= 2                                           # ... it WOULD split with the whole workspace
    assert sch["f16-s3"] == (0, 4, 3) and so.part_units(3, 3) == [(0, 1), (1, 2), (2, 3)]
    assert sch["f16-s3b"] == (0, 1, 3)
    assert sch["bf16-s10"] == (0, 1, 10) and sch["f16-s10"] == (0, 1, 10) and sch["bf16-s10u"] == (0, 2, 10)
    for f, K in (("f16", 602), ("bf16", 700)):
        assert len(set(b - a for a, b in so.part_units(so.units(f, K), 10))) > 1      # unequal parts
    print("\nn_cu = %d: " % n_cu + ", ".join("%s %s" % (k, sch[k]) for k in sorted(sch)), end="")


@pytest.mark.parametrize("name", TAIL_NAMES)
def test_tail_round(dev, name):
    """The tail round at every schedule (see above): ragged rows and columns in the tail tiles, lattice bits and the bound on the
    other kinds; where the schedule does not split (S = 1, 2 rem > n_cu, a workspace one byte short) the bits equal the call
    without a workspace and the workspace is not written."""
    n_cu = n_cu_of()
    form, count, K, N, mode = tail_cases(n_cu)[name]
    S = _tail_schedule(form, count, K, N, n_cu)[2]
    big = count > 1000
    for j, kind in enumerate(("lattice", "dense") if big else ("lattice", "mirror", "sparse_k", "dense", "wild")):
        lat = kind in ("lattice", "mirror")
        p = Problem(form, kind, dev, count + (0 if big else 40), K, N, gathered=(j & 1) == 0, bias=not lat, seed=7000 + j)
        ws = workspace(dev)
        ws_bytes = 4 * ws.numel() - 1 if mode == "short" else None
        split = p.check(count, relu=(j & 1) == 1, ws=ws, ws_bytes=ws_bytes, tag=name)
        if S == 1 or mode == "short":
            assert bool(torch.isnan(ws).all()), name + ": a call that does not split wrote its workspace"
        if S == 1 or mode == "short" or lat:
            plain = so.read_frame(p.run(count, relu=(j & 1) == 1), count, N, name)
            assert so.same_bits(plain, split), name


def test_split16_tail_round_mixes_whole_and_split_tiles(dev):
    """split16's counterpart of test_dense_fwd_rows_split_tail_round_mixes_whole_and_split_tiles: one full round of whole tiles
    and 18 tail tiles in parts, d = 96, N = 512.  Against the bound, and on the rows of whole tiles bit-equal to the call without
    a workspace."""
    n_cu = n_cu_of()
    d, N = 96, 512
    count = 128 * (n_cu // 2 + 9) - 37
    full, rem, S = _tail_schedule("f16", count, d, N, n_cu)
    assert (full, rem) == (n_cu, 18) and S == 3
    for j, kind in enumerate(("lattice", "dense")):
        p = Problem("f16", kind, dev, count + 40, d, N, gathered=True, bias=kind == "dense", seed=8000 + j)
        split = p.check(count, relu=True, ws=workspace(dev), tag="mix")
        plain = p.check(count, relu=True, tag="mix")
        whole = 128 * (n_cu // 2)
        assert so.same_bits(plain[:whole], split[:whole])
        if kind == "lattice":
            assert so.same_bits(plain, split)


# ------------------------------------------------------------------------------------------------ the cut kernels
CUT_K = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]
CUT_N = [1, 63, 64, 65, 100, 257]
CUT_ROWS = [1, 3, 4, 5, 9]


def _cut_input(rng, rows, cols, by_row):
    """fp32 [rows, cols] over a wide exponent range with edge values, an all-zero line and a line whose maximum is denormal
    (line = row if by_row else column; only where there are at least three lines)."""
    A = np.ldexp(rng.standard_normal(size=(rows, cols)), rng.integers(-20, 20, size=(rows, cols))).astype(np.float32)
    scale = np.ldexp(1.0, rng.integers(-40, 40, size=rows if by_row else cols)).astype(np.float32)
    A = (A * (scale[:, None] if by_row else scale[None, :])).astype(np.float32)
    edge = np.asarray([0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 3.0e38, 2.0 ** -100], np.float32)
    flat = A.reshape(-1)
    flat[:min(flat.size, 8)] = edge[:min(flat.size, 8)]
    lines = rows if by_row else cols
    if lines >= 3:
        den = (rng.integers(1, 2 ** 20, size=cols if by_row else rows) * 2.0 ** -149).astype(np.float32)
        if by_row:
            A[1], A[2] = 0, den
        else:
            A[:, 1], A[:, 2] = 0, den
    return A


def _bf16_bits(a):
    return (np.asarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


@pytest.mark.parametrize("K", CUT_K)
def test_cut_rows(dev, K):
    """gs_split_rows and gs_split_rows_f16 at every N: pieces and exponents bit-equal to oracle/split_pieces.py in the layout the
    contractions read, zeros beyond K up to the padded length, exponent 0 for an all-zero column, a column with a denormal
    maximum, NaN pads beyond N, nothing written behind *_bytes."""
    KP = 32 * ((so.cdiv(K, 32) + 1) & ~1)
    for N in CUT_N:
        rng = np.random.default_rng(100 * K + N)
        W = _cut_input(rng, K, N, by_row=False)
        tag = "K=%d N=%d" % (K, N)
        # three bf16 pieces: [KP / 8][3][N][8]
        w3, words = cut_w("bf16", W, dev)
        torch.cuda.synchronize()
        raw = w3.cpu().numpy()
        assert words == KP // 8 * 3 * N * 4 and np.all(raw[words:] == ISENT), tag
        got = raw[:words].view(np.uint16).reshape(KP // 8, 3, N, 8)
        want = np.zeros((3, KP, N), np.uint16)
        for pi, piece in enumerate(sp.cut_bf16x3(W)):
            want[pi, :K] = _bf16_bits(piece)
        assert np.array_equal(got, want.reshape(3, KP // 8, 8, N).transpose(1, 0, 3, 2)), tag
        # two fp16 pieces: [KP / 8][2][N][8] + N exponents
        w2, words = cut_w("f16", W, dev)
        torch.cuda.synchronize()
        raw = w2.cpu().numpy()
        body = KP // 8 * 2 * N * 4
        assert words == body + N and np.all(raw[words:] == ISENT), tag
        h, m, e = sp.cut_cols_f16(W)
        assert np.array_equal(raw[body:words], e), tag
        if N >= 3:
            assert e[1] == 0 and e[2] == 140
        want = np.zeros((2, KP, N), np.uint16)
        want[0, :K], want[1, :K] = h.view(np.uint16), m.view(np.uint16)
        got = raw[:body].view(np.uint16).reshape(KP // 8, 2, N, 8)
        assert np.array_equal(got, want.reshape(2, KP // 8, 8, N).transpose(1, 0, 3, 2)), tag


@pytest.mark.parametrize("d", CUT_K)
def test_cut_table(dev, d):
    """gs_split_table_f16 at every row count (one wave per row, four rows per workgroup): [rows][2][KP] pieces and the row
    exponents bit-equal to oracle/split_pieces.py; zeros in [d, KP); NaN pads beyond d; nothing written behind either byte count."""
    KP = 32 * ((so.cdiv(d, 32) + 1) & ~1)
    for rows in CUT_ROWS:
        rng = np.random.default_rng(100 * d + rows)
        X = _cut_input(rng, rows, d, by_row=True)
        ldx = round_up(d, 4) + 12
        buf = np.full((rows, ldx), NAN, np.float32)
        buf[:, :d] = X
        X2, rexp, tw, ew = cut_table(_dev(buf, dev), d, ldx, dev)
        torch.cuda.synchronize()
        tag = "d=%d rows=%d" % (d, rows)
        raw, ex = X2.cpu().numpy(), rexp.cpu().numpy()
        assert tw == rows * KP and ew == rows and np.all(raw[tw:] == ISENT) and np.all(ex[ew:] == ISENT), tag
        h, m, e = sp.cut_rows_f16(X)
        assert np.array_equal(ex[:ew], e), tag
        if rows >= 3:
            assert e[1] == 0 and e[2] == 140
        want = np.zeros((rows, 2, KP), np.uint16)
        want[:, 0, :d], want[:, 1, :d] = h.view(np.uint16), m.view(np.uint16)
        assert np.array_equal(raw[:tw].view(np.uint16).reshape(rows, 2, KP), want), tag


# ------------------------------------------------------------------------------------------------ the register-staged split16 form
def staged_cases(n_cu):
    """(name, kind, count, K, N, workspace?) of the cases both processes run: the lattice at the star's base and at the K edges,
    and the tail-round shapes (lattice: exact in any part order; dense without a workspace: the two forms sum in the same order)."""
    out = []
    for K in (1, 31, 32, 33, 64, 65, 96, 97, 130):
        out += [("lat-K%d" % K, "lattice", 129, K, 257, False), ("mir-K%d" % K, "mirror", 129, K, 257, True)]
    tc = tail_cases(n_cu)
    for name in ("f16-s1", "f16-s2", "f16-s3", "f16-s3b", "f16-s10", "f16-cap"):
        _, count, K, N, _ = tc[name]
        out += [(name + "-lat", "lattice", count, K, N, True), (name + "-dense", "dense", count, K, N, False),
                (name + "-dense-ws", "dense", count, K, N, True)]
    return out


def staged_outputs(dev, form):
    """name -> block of every staged case, each checked against the oracle as usual (form: "f16" here, "f16r" in the child)."""
    res = {}
    for j, (name, kind, count, K, N, use_ws) in enumerate(staged_cases(n_cu_of())):
        p = Problem(form, kind, dev, count + 9, K, N, gathered=(j & 1) == 0, bias=kind == "dense", seed=9000 + j)
        res[name] = p.check(count, relu=(j & 2) == 2, ws=workspace(dev) if use_ws else None, tag=name)
    return res


def test_register_staged_split16_form(dev, tmp_path):
    """split16_tiled_fwd_kernel (GS_SPLIT16_DMA=0, read once per process): ONE fresh child process, started after this process's
    own GPU work is done, runs tests/split_edges_child.py -- the staged cases through the same checks -- and writes its blocks;
    they must be bit-equal to the DMA form's wherever the two sum in the same order: the lattice (exact), every call without a
    workspace, and those with one whose schedule is the same for stages and stage pairs."""
    n_cu = n_cu_of()
    mine = staged_outputs(dev, "f16")
    torch.cuda.synchronize()
    path = str(tmp_path / "staged.npz")
    root = os.path.dirname(HERE)
    env = dict(os.environ, GS_SPLIT16_DMA="0", PYTHONPATH=os.pathsep.join([root, HERE, os.environ.get("PYTHONPATH", "")]))
    proc = subprocess.run([sys.executable, os.path.join(HERE, "split_edges_child.py"), path], cwd=root, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-3000:]
    print(proc.stdout[-1500:], end="")
    theirs = np.load(path)
    compared = 0
    for name, kind, count, K, N, use_ws in staged_cases(n_cu):
        same_order = (not use_ws) or kind in ("lattice", "mirror")
        if use_ws and not same_order:
            a = _tail_schedule("f16", count, K, N, n_cu)
            b = _tail_schedule("f16r", count, K, N, n_cu)
            same_order = a[2] == 1 and b[2] == 1
        if same_order:
            assert so.same_bits(mine[name], theirs[name]), name
            compared += 1
    assert compared >= 30
