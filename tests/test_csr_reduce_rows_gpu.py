"""-m gpu: gs_csr_reduce_rows (csrc/gs_csr_reduce.hip) over a row SUBSET of tests/test_csr_reduce_gpu.py's graph (degrees 0, 1,
2, 63, 64, 65, L - 1, L, L + 1, 3 L + 7; duplicated ids, self-loops; cut rows in front of, inside and behind the old window),
at that file's widths (4, 12, 50 / ld 52, 256, 260, 602 / ld 608), the three ops, with relu and without, read

  * with x_pos null from the id-indexed table, and
  * through x_pos from a compact, PERMUTED copy that holds only the rows the subset reads (every other row of it is 1e30),

and written through out_pos into a permuted, taller and wider output pre-filled with a sentinel.

Expected values: the float64 oracle at rtol = atol = 1e-4 for the two means (the bound is derived in
tests/test_csr_reduce_gpu.py's docstring: the longest row sums 1543 unit-scale terms), max bit-equal to NumPy's fp32 max -- and,
on every row, BIT-EQUAL to gs_csr_reduce_fwd over the whole graph: the item loop and the combine are one device function for
both kernels, so the order of additions is the same and nothing weaker is acceptable."""
import numpy as np
import pytest
import torch

from graphsage_amd import engine as eng
from graphsage_amd import ops
from graphsage_amd.ops import Mat
from test_csr_reduce_gpu import N_TABLE, N_WIN, OPS, ROW0, SENTINEL, WIDTHS, graph, table
import fullnbr_oracle as fo
import subset_oracle as so

pytestmark = pytest.mark.gpu
# the empty row 1 and the cut row 2 in front of the old window, its fifteen special rows, every second of its other rows, the cut
# row behind it and the last row of the table
ROWS = sorted({1, 2} | {ROW0 + i for i in range(15)} | {ROW0 + i for i in range(15, N_WIN, 2)} | {ROW0 + N_WIN, N_TABLE - 1})
N_OUT = len(ROWS) + 3                   # three rows of the output table that no out_pos names
_cache = {}


def maps(dev):
    """(out_pos host, out_pos device, x_pos host, x_pos device, rows of the compact table): both maps permute."""
    if "maps" not in _cache:
        g, lists = graph()
        rng = np.random.RandomState(17)
        out_pos = np.full(N_TABLE, -1, np.int32)
        out_pos[ROWS] = rng.permutation(N_OUT)[:len(ROWS)]
        S = so.closure(lists, ROWS)
        assert set(ROWS) <= set(S.tolist())  # (the 3 L + 7 hub reads most of the table: the copy is permuted, hardly smaller)
        x_pos = np.full(N_TABLE, -1, np.int32)
        x_pos[S] = rng.permutation(len(S) + 2)[:len(S)]
        _cache["maps"] = (out_pos, torch.from_numpy(out_pos).to(dev), x_pos, torch.from_numpy(x_pos).to(dev), len(S) + 2)
        torch.cuda.synchronize()
    return _cache["maps"]


def compact_table(dev, d, ld):
    key = ("xc", d)
    if key not in _cache:
        x, _ = table(dev, d, ld)
        _, _, x_pos, _, n_c = maps(dev)
        xc = np.full((n_c, d), 1e30, np.float32)
        member = np.flatnonzero(x_pos >= 0)
        xc[x_pos[member]] = x[member]
        big = torch.zeros((n_c + 2, ld), dtype=torch.float32, device=dev)       # the table sits inside a larger allocation
        m = Mat(big[1:1 + n_c], d)
        m.buf[:, :d].copy_(torch.from_numpy(xc))
        torch.cuda.synchronize()
        _cache[key] = m
    return _cache[key]


def run_rows(e, g, op, X, d, out_pos_dev, x_pos_dev, act, rows=ROWS):
    d4 = (d + 3) // 4 * 4
    big = torch.full((N_OUT + 4, d4 + 8), SENTINEL, dtype=torch.float32, device=e.device)
    torch.cuda.synchronize()
    out = Mat(big[2:2 + N_OUT], d)
    g.reduce_rows(e, op, X, out, rows, out_pos_dev, x_pos=x_pos_dev, act=act)
    e.sync()
    return big.cpu().numpy(), d4


def check_strays(got, d, d4, named):
    body = got[2:2 + N_OUT]
    assert np.all(got[:2] == SENTINEL) and np.all(got[2 + N_OUT:] == SENTINEL), "rows outside the table were written"
    unnamed = np.setdiff1d(np.arange(N_OUT), named)
    assert np.all(body[unnamed] == SENTINEL), "rows that no out_pos names were written"
    assert np.all(got[:, d4:] == SENTINEL), "columns beyond round_up(d, 4) were written"
    assert not np.any(body[named, :d] == SENTINEL), "a named row was not written"
    if d4 > d:
        assert np.all(body[named, d:d4] == 0), "the pad columns of the last float4 must be zero"


def window_reference(e, g, op, X, d, act):
    out = Mat.zeros(N_TABLE, d, e.device)
    torch.cuda.synchronize()
    g.reduce(e, op, X, out, 0, N_TABLE, act=act)
    e.sync()
    return out.numpy()


@pytest.mark.parametrize("d,ld", WIDTHS)
@pytest.mark.parametrize("op", sorted(OPS))
def test_row_list_reduce_equals_the_oracle_and_the_window_kernel(dev, op, d, ld):
    eng.reset_engine()
    e = eng.get_engine()
    g, lists = graph()
    x, X = table(dev, d, ld)
    Xc = compact_table(dev, d, ld)
    out_pos, out_pos_dev, x_pos, x_pos_dev, _ = maps(dev)
    named = out_pos[ROWS]
    want = fo.reduce_rows(lists, x if op == "max" else x.astype(np.float64), op)[ROWS]
    for act in (ops.ACT_IDENTITY, ops.ACT_RELU):
        ref = window_reference(e, g, OPS[op], X, d, act)[ROWS]
        w = np.maximum(want, 0) if act == ops.ACT_RELU else want
        for table_, map_ in ((X, None), (Xc, x_pos_dev)):
            got, d4 = run_rows(e, g, OPS[op], table_, d, out_pos_dev, map_, act)
            check_strays(got, d, d4, named)
            res = got[2:2 + N_OUT][named, :d]
            if op == "max":
                assert w.dtype == np.float32 and np.array_equal(res, w)
            else:
                np.testing.assert_allclose(res, w, rtol=1e-4, atol=1e-4)
            assert np.array_equal(res, ref), "the row-list reduce must give the window kernel's bits (x_pos %s, act %d)" % (
                "null" if map_ is None else "set", act)
    # empty rows: 0 for mean and max, X[r] for mean-with-self (through the map)
    for r in (1, ROW0, ROW0 + 10):
        assert len(lists[r]) == 0 and r in ROWS
        assert np.array_equal(res[ROWS.index(r)], np.maximum(x[r], 0) if op == "mean_self" else np.zeros(d, np.float32))


@pytest.mark.parametrize("op", sorted(OPS))
def test_smaller_lists_and_every_row_give_the_same_bits(dev, op):
    """One uncut row, one cut row, only cut rows, every row: each row's value does not depend on the list it is part of."""
    eng.reset_engine()
    e = eng.get_engine()
    g, lists = graph()
    d, ld = 50, 52
    x, X = table(dev, d, ld)
    ref = window_reference(e, g, OPS[op], X, d, ops.ACT_IDENTITY)
    cut = [int(r) for r in g.splits[:, 0]]
    assert len(cut) == 4
    for rows in ([ROW0 + 5], [cut[1]], cut, list(range(N_TABLE))):
        ident = torch.arange(N_TABLE, dtype=torch.int32, device=dev)
        out = Mat.zeros(N_TABLE, d, dev)
        out.buf.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.reduce_rows(e, OPS[op], X, out, rows, ident, x_pos=ident)            # identity maps: a map that changes nothing
        e.sync()
        got = out.buf.cpu().numpy()
        assert np.array_equal(got[rows, :d], ref[rows])
        assert np.all(got[np.setdiff1d(np.arange(N_TABLE), rows)] == SENTINEL)


def test_positions_outside_the_tables_are_skipped_not_followed(dev):
    """A row whose out_pos is -1 or one past the table, and an uncut row that reads an id whose x_pos is -1 (a non-member), are
    left unwritten; every row that reads no such id keeps its bits.  (A CUT row that reads one loses that segment's partial and
    combines whatever the workspace held: its value is not checked, only that nothing outside the table is touched.)  All
    tables sit inside larger allocations."""
    eng.reset_engine()
    e = eng.get_engine()
    g, lists = graph()
    d, ld = 50, 52
    _, X = table(dev, d, ld)
    Xc = compact_table(dev, d, ld)
    out_pos, out_pos_dev, x_pos, x_pos_dev, _ = maps(dev)
    good, _ = run_rows(e, g, OPS["mean"], Xc, d, out_pos_dev, x_pos_dev, ops.ACT_IDENTITY)
    bad_out = out_pos.copy()
    r_neg, r_past, r_read = ROW0 + 3, ROW0 + 9, ROW0 + 5          # an uncut row, the 3 L + 7 hub (its combine), a reader
    bad_out[r_neg], bad_out[r_past] = -1, N_OUT
    bad_x = x_pos.copy()
    bad_x[int(lists[r_read][64])] = -1                            # an id of the reader's second 64-id batch
    hit = [r for r in ROWS if int(lists[r_read][64]) in lists[r] or r in (r_neg, r_past)]
    assert r_read in hit
    got, d4 = run_rows(e, g, OPS["mean"], Xc, d, torch.from_numpy(bad_out).to(dev), torch.from_numpy(bad_x).to(dev),
                       ops.ACT_IDENTITY)
    body, ref = got[2:2 + N_OUT], good[2:2 + N_OUT]
    keep = [r for r in ROWS if r not in hit]
    cut = [int(r) for r in g.splits[:, 0]]
    unwritten = [r for r in hit if r not in cut and r != r_neg] + [r_past]
    assert len(keep) > 10 and r_read in unwritten
    assert np.array_equal(body[out_pos[keep]], ref[out_pos[keep]])
    named = np.asarray([bad_out[r] for r in unwritten if 0 <= bad_out[r] < N_OUT], dtype=np.int64)
    assert np.all(body[named] == SENTINEL)
    claimed = set(int(p) for p in bad_out[ROWS] if 0 <= p < N_OUT)
    assert np.all(body[[p for p in range(N_OUT) if p not in claimed]] == SENTINEL)
    assert np.all(got[:2] == SENTINEL) and np.all(got[2 + N_OUT:] == SENTINEL) and np.all(got[:, d4:] == SENTINEL)


def test_bad_calls_are_refused_on_the_host(dev):
    from graphsage_amd._lib import GraphsageAmdError
    eng.reset_engine()
    e = eng.get_engine()
    g, _ = graph()
    _, X = table(dev, 12, 12)
    out_pos, out_pos_dev, _, _, _ = maps(dev)
    out = Mat.zeros(N_OUT, 12, dev)
    short = Mat(X.buf[:N_TABLE - 1], 12)
    with pytest.raises(GraphsageAmdError, match="rows"):
        g.reduce_rows(e, OPS["mean"], short, out, ROWS, out_pos_dev)          # no map: an id could point past the table
    with pytest.raises(GraphsageAmdError, match="unknown op"):
        g.reduce_rows(e, 9, X, out, ROWS, out_pos_dev)
    with pytest.raises(GraphsageAmdError, match="ld"):
        g.reduce_rows(e, OPS["mean"], X, Mat.zeros(N_OUT, 8, dev), ROWS, out_pos_dev)
    with pytest.raises(GraphsageAmdError, match="int32"):
        g.reduce_rows(e, OPS["mean"], X, out, ROWS, out_pos_dev.long())
    with pytest.raises(GraphsageAmdError, match="n_rows"):
        g.reduce_rows(e, OPS["mean"], X, out, ROWS, out_pos_dev[:-1])
    with pytest.raises(GraphsageAmdError, match="plan_rows"):
        g.reduce_rows(e, OPS["mean"], X, out, ROWS[::-1], out_pos_dev)
    e.sync()
