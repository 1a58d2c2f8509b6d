"""-m gpu: the LSTM recurrence kernels (gs_lstm_lengths, gs_lstm_fwd, gs_lstm_bwd with its W_h transpose; csrc/gs_lstm.hip) against
the float64 oracle of tests/seq_oracle.py (recurrence_fwd / recurrence_bwd) at their tile, length and layout edges.  The cases are
those of tests/lstm_cases.py (checked on the CPU by tests/test_seq_oracle.py): n in {0, 1, 3, 15, 16, 17, 33}, T in 1 .. 25, empty
segments first / in the middle / last, GS_LSTM_MAX_SEG segments, the planted length cases (all-zero rows, interior / trailing /
leading zero row, only the last row non-zero, a subnormal, -0.0), L = 1 next to L = T in one tile, a tile with tmax < T.

Buffers (the convention of test_elementwise_edges_gpu.py): every output is a row-sliced Mat two rows down a buffer filled with
optim_oracle.SENTINEL, at the exact leading dimension and at ld + 8; every input's pad columns hold NaN (W_h at ldw = 4H + 8
included); W_hT_ws is exactly 4H * H floats and `lengths` exactly its rows inside sentinel-bracketed buffers; step rows lie
contiguously or with three rows nobody owns before every segment.  ONE rule covers what must stay: every element that the contract
of include/graphsage_amd.h does not name as written keeps its bits (rows t >= L of A and C -- of G when A aliases G --, gap rows,
rows outside the view, columns >= 4H or >= H, every input).  H_prev at t = 0 and for t >= L and dG for t >= L are exact zeros.

Values: A, C, H_prev, h_last and dG element by element on the rows t < L within max(8 e32, 8 * 2^-24 * max(1, max |want|)) of the
float64 oracle, e32 = the largest |fp32 oracle - fp64 oracle| of that output in that case (the device sums h . W_h as one serial FMA
chain where NumPy uses blocked BLAS, and its expf / tanhf may be a couple of ulp off).  Bit-identical, with no tolerance: in place
(A is G, dG is A) == separate buffers; ld + 8 and gapped rows == exact and contiguous; one launch == one launch per segment; a
permuted segment == the permuted rows; the first and last sequence alone as n = 1; the backward with rows t >= L of A and C
overwritten by NaN (what they hold in production: the engine reuses its workspaces).

Worst observed device error / e32 per output on an MI355X over all cases (bound: 8; pytest -s prints every figure):
  A 1.22    C 1.05    H_prev 1.00    h_last 1.12    dG 1.36
The device is as close to float64 as NumPy's fp32 is.  Planted sequence 5 of lstm_cases (the subnormal) counts as a non-zero row on the device too:
its fp32 compare does not flush.
"""
import ctypes

import numpy as np
import pytest
import torch

import lstm_cases as lc
import optim_oracle as oo
import seq_oracle as so
from graphsage_amd import _lib, ops
from graphsage_amd._lib import GraphsageAmdError
from graphsage_amd.ops import Mat

pytestmark = pytest.mark.gpu
S = oo.SENTINEL
LS = -777                                # the sentinel of the int32 buffer around `lengths`
ALL = [(i, 128) for i in range(len(lc.CASES))] + [(i, 256) for i in lc.CASES_256]
IDS = ["H%d-%s" % (H, lc.case_id(i)) for i, H in ALL]
WORST = {}
_baseline = {}


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Buf(object):
    """A [rows, w] fp32 matrix two rows down a [rows + 4, ld] buffer filled with `fill`; `parts` (per segment [n, T, w]) or `whole`
    ([rows', w]) are planted first.  `before` keeps the bits it started with."""

    def __init__(self, dev, rows, w, ld, fill, lay=None, parts=None, whole=None):
        a = np.full((rows + 4, ld), fill, np.float32)
        if parts is not None:
            lay.scatter(parts, a[2:2 + rows])
        if whole is not None:
            a[2:2 + len(whole), :w] = whole
        self.before, self.big, self.rows, self.w = a, _dev(a, dev), rows, w
        self.mat = Mat(self.big[2:2 + rows], w)

    def read(self):
        torch.cuda.synchronize()
        return self.big.cpu().numpy()

    def only_written(self, allowed, tag, since=None):
        """Every element outside `allowed` ([rows, ld] bool, within the view) keeps its bits; -> the view."""
        got = self.read()
        keep = np.ones(got.shape, bool)
        keep[2:2 + self.rows] = ~allowed
        ref = self.before if since is None else since
        bad = keep & (_bits(got) != _bits(ref))
        assert not bad.any(), "%s: %d elements written that the contract leaves alone, first at (row, column) %s" % (
            tag, bad.sum(), tuple(np.argwhere(bad)[0] - (2, 0)))
        return got[2:2 + self.rows]

    def poke(self, view):
        self.big[2:2 + self.rows].copy_(_dev(view, self.big.device))


def _segs(lay, only=None):
    """ops segment tuples (the recurrence reads neither X nor ids); only = k: segment k alone."""
    ks = range(len(lay.segs)) if only is None else [only]
    return [(None, None, lay.segs[k][0], lay.segs[k][1], lay.row0[k]) for k in ks]


def run(dev, c, tag, pad=0, gap=0, inplace=False, per_segment=False, poison=False):
    """gs_lstm_fwd then gs_lstm_bwd on case c, with every contract check that needs no oracle; -> {A, C, Hp, dG: per segment
    [n, T, w]; hl [n_total, H]}."""
    H, lay = c.H, lc.Layout(c.segs, gap)
    rows, nt = lay.rows, lay.n_total
    ld4, ld1 = 4 * H + pad, H + pad
    ran = [np.arange(T)[None, :] < L[:, None] for (n, T), L in zip(c.segs, c.L)]
    owned = [np.ones((n, T), bool) for n, T in c.segs]
    Wh = Buf(dev, H, 4 * H, ld4, np.nan, whole=c.W_h)
    G = Buf(dev, rows, 4 * H, ld4, S if inplace else np.nan, lay, c.G)
    A = G if inplace else Buf(dev, rows, 4 * H, ld4, S)
    C, Hp = Buf(dev, rows, H, ld1, S), Buf(dev, rows, H, ld1, S)
    hl = Buf(dev, nt + 1, H, ld1, S)
    dh = Buf(dev, nt + 1, H, ld1, np.nan, whole=np.concatenate(c.dh))
    Lh = np.full(nt + 17, LS, np.int32)
    Lh[8:8 + nt] = np.concatenate(c.L)
    Lbuf = _dev(Lh, dev)
    Lv = Lbuf[8:8 + nt + 1]
    wt_h = np.full(4 * H * H + 128, S, np.float32)
    wt = _dev(wt_h, dev)
    launches = [(_segs(lay, k), lay.seq0[k]) for k in range(len(c.segs))] if per_segment else [(_segs(lay), 0)]
    for segs, s0 in launches:
        ops.lstm_fwd(segs, H, Wh.mat, Lv[s0:], G.mat, A.mat, C.mat, Hp.mat, hl.mat.rows_slice(s0, nt + 1))
    a = A.only_written(lay.step_mask(ran, 4 * H, ld4), tag + " A").copy()
    cc = C.only_written(lay.step_mask(ran, H, ld1), tag + " C").copy()
    hp = Hp.only_written(lay.step_mask(owned, H, ld1), tag + " H_prev")
    seq_rows = np.zeros((nt + 1, ld1), bool)
    seq_rows[:nt, :H] = True
    h = hl.only_written(seq_rows, tag + " h_last")[:nt, :H]
    if not inplace:
        G.only_written(np.zeros((rows, ld4), bool), tag + " G (input of the forward)")
    out = {"A": lay.gather(a, 4 * H), "C": lay.gather(cc, H), "Hp": lay.gather(hp, H), "hl": h, "ran": ran}
    for p, r in zip(out["Hp"], ran):
        assert not _bits(p[~r]).any() and not _bits(p[:, :1]).any(), tag + ": H_prev must be +0 at t = 0 and for t >= L"
    if poison:                       # what the rows past a length hold in production is not the kernels' business
        for buf, view, w in ((A, a, 4 * H), (C, cc, H)):
            view[lay.step_mask([~r for r in ran], w, view.shape[1])] = np.nan
            buf.poke(view)
    a_in = A.read()
    c_in = C.read()
    dG = A if inplace else Buf(dev, rows, 4 * H, ld4, S)
    for segs, s0 in launches:
        ops.lstm_bwd(segs, H, Wh.mat, wt[64:64 + 4 * H * H], Lv[s0:], A.mat, C.mat, dh.mat.rows_slice(s0, nt + 1), dG.mat)
    g = dG.only_written(lay.step_mask(owned, 4 * H, ld4), tag + " dG", since=a_in if inplace else None)
    out["dG"] = lay.gather(g, 4 * H)
    for p, r in zip(out["dG"], ran):
        assert not _bits(p[~r]).any(), tag + ": dG must be +0 for t >= L"
    # the backward's inputs, and the transpose scratch
    for buf, ref, name in ((Wh, None, "W_h"), (dh, None, "dh_last"), (C, c_in, "C")) + (() if inplace else ((A, a_in, "A"), (G, None, "G"))):
        buf.only_written(np.zeros((buf.rows, buf.before.shape[1]), bool), "%s %s (input of the backward)" % (tag, name), since=ref)
    assert np.array_equal(Lbuf.cpu().numpy(), Lh), tag + ": lengths changed"
    wt_got = wt.cpu().numpy()
    assert (wt_got[:64] == S).all() and (wt_got[64 + 4 * H * H:] == S).all(), tag + ": written outside W_hT_ws[0 : 4H*H]"
    if nt:
        assert np.array_equal(_bits(wt_got[64:64 + 4 * H * H].reshape(4 * H, H)), _bits(c.W_h.T)), tag + ": W_hT_ws != W_h^T"
    else:
        assert (wt_got == S).all(), tag + ": nothing to do, yet W_hT_ws was written"
    return out


def same_bits(got, want, tag, picks=None):
    """Every output of two runs, bit for bit: H_prev and dG whole, A and C on the rows t < L (what the others hold is the buffer's,
    and run() has checked that it stayed).  picks = [(segment, indices)]: got's segments are those sequences of want's."""
    s0 = np.cumsum([0] + [len(p) for p in want["C"]])
    for k in ("ran", "A", "C", "Hp", "dG"):
        sel = want[k] if picks is None else [want[k][s][idx] for s, idx in picks]
        assert len(got[k]) == len(sel)
        for j, (a, b) in enumerate(zip(got[k], sel)):
            if k == "ran":
                assert np.array_equal(a, b), tag
                continue
            if k in ("A", "C"):
                a, b = a[got["ran"][j]], b[got["ran"][j]]
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), "%s: %s of segment %d differs" % (tag, k, j)
    hl = want["hl"] if picks is None else np.concatenate([want["hl"][s0[s] + np.asarray(idx, np.int64)] for s, idx in picks] or [want["hl"][:0]])
    assert np.array_equal(_bits(got["hl"]), _bits(hl)), tag + ": h_last differs"


def against_oracle(c, out, tag):
    """Element by element on the rows that ran; records the worst error / e32 per output."""
    tol, e32, o64 = c.tolerance(), c.e32(), c.oracle(np.float64)
    s0 = 0
    for k, o in enumerate(o64):
        n = c.segs[k][0]
        for name in lc.OUTPUTS:
            got = out["hl"][s0:s0 + n] if name == "hl" else out[name][k][o["ran"]]
            want = o["hl"] if name == "hl" else o[name][o["ran"]]
            if not want.size:
                continue
            assert np.isfinite(got).all(), "%s: non-finite %s" % (tag, name)
            err = float(np.abs(got.astype(np.float64) - want).max())
            ratio = err / e32[name] if e32[name] else 0.0
            WORST[name] = max(WORST.get(name, 0.0), ratio)
            print("%s segment %d %s: err %.3g, e32 %.3g (ratio %.2f), bound %.3g" % (tag, k, name, err, e32[name], ratio, tol[name]))
            assert err <= tol[name], "%s: %s is %.3g from the fp64 oracle, bound %.3g (e32 %.3g)" % (tag, name, err, tol[name], e32[name])
        s0 += n


def baseline(dev, i, H):
    if (i, H) not in _baseline:
        _baseline[(i, H)] = run(dev, lc.case(i, H), "H=%d %s" % (H, lc.case_id(i)))
    return _baseline[(i, H)]


# ----------------------------------------------------------------------------------------------- the recurrence
@pytest.mark.parametrize("i,H", ALL, ids=IDS)
def test_recurrence_equals_float64_oracle(dev, i, H):
    """Separate buffers, exact leading dimensions, contiguous rows: A, C, H_prev, h_last, dG on the rows t < L."""
    against_oracle(lc.case(i, H), baseline(dev, i, H), "H=%d %s" % (H, lc.case_id(i)))
    print("worst err / e32 so far: " + ", ".join("%s %.2f" % kv for kv in sorted(WORST.items())))


@pytest.mark.parametrize("i,H", ALL, ids=IDS)
def test_layouts_and_aliasing_have_the_bits_of_the_plain_launch(dev, i, H):
    """ld + 8 (NaN / sentinel pad columns), three unowned rows before every segment, in place (A is G, then dG is A): all eight
    combinations; each run checks its own buffers for stray writes."""
    c, base = lc.case(i, H), baseline(dev, i, H)
    for pad in (0, 8):
        for gap in (0, 3):
            for inplace in (False, True):
                if pad or gap or inplace:
                    tag = "H=%d %s pad=%d gap=%d inplace=%d" % (H, lc.case_id(i), pad, gap, inplace)
                    same_bits(run(dev, c, tag, pad=pad, gap=gap, inplace=inplace), base, tag)


@pytest.mark.parametrize("i,H", ALL, ids=IDS)
def test_launch_forms_have_the_bits_of_the_plain_launch(dev, i, H):
    """One launch per segment; every segment permuted; the first and the last sequence alone (n = 1); the backward over A and C
    whose rows t >= L hold NaN -- a sequence's result depends on nothing but its own rows."""
    c, base = lc.case(i, H), baseline(dev, i, H)
    tag = "H=%d %s " % (H, lc.case_id(i))
    same_bits(run(dev, c, tag + "per segment", per_segment=True, gap=3, inplace=True), base, tag + "per segment")
    for inplace in (False, True):
        same_bits(run(dev, c, tag + "poisoned", poison=True, inplace=inplace), base, tag + "poisoned")
    picks = [(k, lc.permutation(n)) for k, (n, T) in enumerate(c.segs)]
    same_bits(run(dev, c.select(picks), tag + "permuted", inplace=True), base, tag + "permuted", picks)
    full = [k for k, (n, T) in enumerate(c.segs) if n]
    for k, r in ([(full[0], 0), (full[-1], c.segs[full[-1]][0] - 1)] if full else []):
        picks = [(k, [r])]
        same_bits(run(dev, c.select(picks), tag + "alone"), base, tag + "sequence %d of segment %d alone" % (r, k), picks)


def test_saturated_gates(dev):
    """+-100 planted in eight units of each gate at every step (H = 128, 5 sequences of 3 steps): everything finite and within the
    bound, and dG exactly zero wherever the float64 oracle's is (sigma(100) = 1, tanh(+-100) = +-1 in either precision)."""
    c = lc.saturated_case()
    out = run(dev, c, "saturated")
    against_oracle(c, out, "saturated")
    o = c.oracle(np.float64)[0]
    zero = (o["dG"] == 0) & o["ran"][:, :, None]
    planted = np.zeros(4 * 128, bool)
    for g in range(4):
        planted[g * 128 + 8 * g:g * 128 + 8 * g + 8] = True
    assert zero[:, :, planted].sum() >= 5 * 8 * 2                  # the oracle does have exact zeros at the planted gates
    assert not out["dG"][0][zero].any()
    same_bits(run(dev, c, "saturated in place", inplace=True, pad=8), out, "saturated in place")


# ----------------------------------------------------------------------------------------------- gs_lstm_lengths
def _lengths_case(dev, segs, short, d, ldx, use_ids, last, tag):
    xs, Ls = lc.inputs(segs, d, last_col_only=last, short=short, seed=d)
    nt = sum(n for n, _ in segs)
    want = np.concatenate([so.lengths(x) for x in xs]).astype(np.int32)
    assert np.array_equal(want, np.concatenate(Ls))
    pad = lambda a: _dev(np.concatenate([a, np.full((len(a), ldx - d), np.nan, np.float32)], axis=1), dev)   # noqa: E731
    if use_ids:
        table, ids, gathered = lc.id_table(xs, np.random.RandomState(d))
        assert np.array_equal(want, np.concatenate([so.lengths(g) for g in gathered]).astype(np.int32))
        X = Mat(pad(table), d)
        ids_dev = [_dev(i, dev) if len(i) else None for i in ids]
        seg_args = [(X, i, n, T, 0) for i, (n, T) in zip(ids_dev, segs)]
    else:
        flat = np.concatenate([x.reshape(-1, d) for x in xs] + [np.ones((1, d), np.float32)])
        X = Mat(pad(flat), d)
        seg_args, r = [], 0
        for n, T in segs:
            seg_args.append((X.rows_slice(r, r + max(n * T, 1)), None, n, T, 0))
            r += n * T
    Lh = np.full(nt + 17, LS, np.int32)
    Lbuf = _dev(Lh, dev)
    ops.lstm_lengths(seg_args, d, Lbuf[8:8 + nt + 1])
    torch.cuda.synchronize()
    got = Lbuf.cpu().numpy()
    assert (got[:8] == LS).all() and (got[8 + nt:] == LS).all(), tag + ": written outside lengths[0 : n_total]"
    assert np.array_equal(got[8:8 + nt], want), "%s: got %s, want %s" % (tag, got[8:8 + nt].tolist(), want.tolist())


@pytest.mark.parametrize("d", lc.WIDTHS)
def test_lengths_sweep(dev, d):
    """lengths == seq_oracle.lengths on every segment list, at ldx = round_up(d, 4) and + 8 (NaN beyond column d), from the rows
    themselves and through ids into a larger table (repeated rows, one zero pad row), with the only non-zero of every planted
    non-zero row in column d - 1 for half of the cases."""
    d4 = ops.round_up(d, 4)
    for ldx in (d4, d4 + 8):
        for use_ids in (0, 1):
            for last in (0, 1):
                for i, (segs, short) in enumerate(lc.CASES):
                    _lengths_case(dev, segs, short, d, ldx, use_ids, last, "lengths d=%d ldx=%d ids=%d last=%d %s" % (d, ldx, use_ids, last, lc.case_id(i)))


# ----------------------------------------------------------------------------------------------- refused calls
def test_bad_calls_are_refused_before_any_launch(dev):
    H, n, T, d = 128, 5, 3, 12
    rows = n * T
    outs = {k: Buf(dev, rows, w, w + 8, S) for k, w in (("G", 4 * H), ("A", 4 * H), ("C", H), ("Hp", H), ("dG", 4 * H))}
    outs["hl"] = Buf(dev, n, H, H + 8, S)
    Wh, dh, X = Buf(dev, H, 4 * H, 4 * H, 0.25), Buf(dev, n, H, H, 0.5), Buf(dev, rows, d, d, 1.0)
    wt = _dev(np.full(4 * H * H, S, np.float32), dev)
    Lbuf = _dev(np.full(n, LS, np.int32), dev)

    def seg_array(specs):
        arr = (_lib.LstmSeg * max(len(specs), 1))()
        for k, (x, ldx, nn, tt, row0, seq0) in enumerate(specs):
            arr[k].X, arr[k].ids, arr[k].ldx, arr[k].n, arr[k].row0, arr[k].seq0, arr[k].T = x, None, ldx, nn, row0, seq0, tt
        return arr

    good = [(X.mat.ptr, d, n, T, 0, 0)]
    two_bad = [(X.mat.ptr, d, 2, T, 0, 0), (X.mat.ptr, d, 3, T, 2 * T, 3)]           # the second starts at sequence 3, not 2
    five = [(X.mat.ptr, d, 1, T, k * T, k) for k in range(5)]

    def fwd(specs=good, n_seg=None, h=H, w=Wh.mat.ptr, ldw=4 * H, g=outs["G"], ldg=None, a=outs["A"], lda=None, ldc=H + 8):
        arr = seg_array(specs)
        ops.call("gs_lstm_fwd", ctypes.addressof(arr), len(specs) if n_seg is None else n_seg, h, w, ldw, ops.ptr(Lbuf),
                 g.mat.ptr, g.mat.ld if ldg is None else ldg, a.mat.ptr, a.mat.ld if lda is None else lda, outs["C"].mat.ptr, ldc,
                 outs["Hp"].mat.ptr, H + 8, outs["hl"].mat.ptr, H + 8, ops.current_stream())

    def bwd(specs=good, n_seg=None, h=H, w=Wh.mat.ptr, ws=ops.ptr(wt), a=outs["A"], lda=None, g=outs["dG"], lddg=None):
        arr = seg_array(specs)
        ops.call("gs_lstm_bwd", ctypes.addressof(arr), len(specs) if n_seg is None else n_seg, h, w, 4 * H, ws,
                 ops.ptr(Lbuf), a.mat.ptr, a.mat.ld if lda is None else lda, outs["C"].mat.ptr, H + 8, dh.mat.ptr, H,
                 g.mat.ptr, g.mat.ld if lddg is None else lddg, ops.current_stream())

    def lengths(specs=good, n_seg=None, dd=d, out=ops.ptr(Lbuf)):
        arr = seg_array(specs)
        ops.call("gs_lstm_lengths", ctypes.addressof(arr), len(specs) if n_seg is None else n_seg, dd, out, ops.current_stream())

    bad = [
        ("H = 64", lambda: fwd(h=64)), ("H = 64", lambda: bwd(h=64)),
        ("n_seg = 0", lambda: fwd(n_seg=0)), ("n_seg = 0", lambda: bwd(n_seg=0)), ("n_seg = 0", lambda: lengths(n_seg=0)),
        ("n_seg = 5", lambda: fwd(five)), ("n_seg = 5", lambda: bwd(five)), ("n_seg = 5", lambda: lengths(five)),
        ("T = 0", lambda: fwd([(X.mat.ptr, d, n, 0, 0, 0)])), ("T = 0", lambda: bwd([(X.mat.ptr, d, n, 0, 0, 0)])),
        ("T = 0", lambda: lengths([(X.mat.ptr, d, n, 0, 0, 0)])),
        ("seq0", lambda: fwd(two_bad)), ("seq0", lambda: bwd(two_bad)), ("seq0", lambda: lengths(two_bad)),
        ("ldg < 4H", lambda: fwd(ldg=4 * H - 4)), ("lda < 4H", lambda: fwd(lda=4 * H - 4)), ("ldc < H", lambda: fwd(ldc=H - 4)),
        ("ldw < 4H", lambda: fwd(ldw=4 * H - 4)), ("lddg < 4H", lambda: bwd(lddg=4 * H - 4)), ("lda < 4H", lambda: bwd(lda=4 * H - 4)),
        ("G is A, ldg != lda", lambda: fwd(a=outs["G"], lda=4 * H + 16)), ("A is dG, lda != lddg", lambda: bwd(g=outs["A"], lddg=4 * H + 16)),
        ("W_h = NULL", lambda: fwd(w=None)), ("W_h = NULL", lambda: bwd(w=None)), ("W_hT_ws = NULL", lambda: bwd(ws=None)),
        ("X = NULL", lambda: lengths([(None, d, n, T, 0, 0)])), ("ldx < d", lambda: lengths([(X.mat.ptr, d - 1, n, T, 0, 0)])),
        ("lengths = NULL", lambda: lengths(out=None)), ("d = 0", lambda: lengths(dd=0)),
    ]
    for what, f in bad:
        with pytest.raises(GraphsageAmdError):
            f()
            pytest.fail("accepted: " + what)
    torch.cuda.synchronize()
    for k, b in outs.items():
        b.only_written(np.zeros((b.rows, b.before.shape[1]), bool), "refused calls: " + k)
    assert (wt.cpu().numpy() == S).all() and (Lbuf.cpu().numpy() == LS).all()
    # ... and the same buffers do go through when nothing is wrong (so the refusals above were about what they name)
    outs["G"].poke(np.zeros((rows, 4 * H + 8), np.float32))
    lengths()
    fwd()
    bwd()
    torch.cuda.synchronize()
    assert (Lbuf.cpu().numpy() == T).all() and np.isfinite(outs["dG"].read()[2:2 + rows, :4 * H]).all()
