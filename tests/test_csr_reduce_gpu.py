"""-m gpu: gs_csr_reduce_fwd (csrc/gs_csr_reduce.hip) == a float64 NumPy oracle, for the three ops, on one synthetic CSR whose
rows sit on every edge of the kernel's paths: degree 0, 1, 2, around the 64-id broadcast batch (63, 64, 65), around the split
length L = 512 (L - 1, L, L + 1: the last whole row, the first cut one) and a hub of 3 L + 7 (four partials, a ragged last
one); duplicated ids, self-loops.  Widths: one float4 (4), a few (12), not a multiple of 4 (50, ld 52), exactly one 64-float4
column chunk (256), a ragged second chunk (260), Reddit's 602 (ld 608, three chunks).  The output buffer is wider and taller
than what the call may write and pre-filled with a sentinel: a stray store shows without provoking anything.

Tolerances: mean / mean-with-self rtol = atol = 1e-4 against the float64 oracle (the project's float tolerance; the longest row
sums 1543 unit-scale terms in fp32: error ~ 1543 * 6e-8 * |x| ~ 1e-4 of ONE term's scale before the division by 1543, far
inside); max is bit-equal to NumPy's fp32 max."""
import numpy as np
import pytest
import torch

from graphsage_amd import engine as eng
from graphsage_amd import ops
from graphsage_amd.inference import CSR_MAX, CSR_MEAN, CSR_MEAN_SELF, SPLIT_LEN, FullGraph
from graphsage_amd.ops import Mat
import fullnbr_oracle as fo

pytestmark = pytest.mark.gpu
L = SPLIT_LEN
N_TABLE = 300                     # rows of the table (the graph's rows: N_TABLE - 1 nodes + the pad row)
ROW0, N_WIN = 7, 40               # the window under test
SENTINEL = -12345.5
WIDTHS = [(4, 4), (12, 12), (50, 52), (256, 256), (260, 260), (602, 608)]
OPS = {"mean": CSR_MEAN, "mean_self": CSR_MEAN_SELF, "max": CSR_MAX}
_cache = {}


def graph():
    if "g" in _cache:
        return _cache["g"]
    assert L == 512
    rng = np.random.RandomState(5)
    special = [0, 1, 2, 63, 64, 65, L - 1, L, L + 1, 3 * L + 7, 0, 130, 1, 3, 17]
    degs = np.asarray([1] * N_TABLE)
    degs[:ROW0] = [3, 0, 600, 1, 2, 0, 70]                    # rows before the window (a cut row among them: slot0 > 0)
    win = np.asarray(special + list(rng.randint(0, 9, size=N_WIN - len(special))))
    degs[ROW0:ROW0 + N_WIN] = win
    degs[ROW0 + N_WIN:ROW0 + N_WIN + 3] = [2 * L + 1, 0, 5]      # ... and behind it
    lists = [rng.randint(0, N_TABLE, size=d) for d in degs]
    lists[ROW0 + 2][:] = lists[ROW0 + 2][0]                      # duplicated ids
    lists[ROW0 + 11][:40] = 123
    lists[ROW0 + 3][5] = ROW0 + 3                                # self-loops
    lists[ROW0 + 9][700] = ROW0 + 9
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    col = np.concatenate(lists).astype(np.int32)
    g = FullGraph(rowptr, col, N_TABLE - 1)
    (i0, i1), (s0, s1), (t0, t1) = g.window(ROW0, N_WIN)
    assert i1 - i0 == N_WIN + 1 + 3 and s1 - s0 == 2 and t0 == 2 and t1 == 2 + 2 + 4      # L + 1 -> 2 partials, 3 L + 7 -> 4
    _cache["g"] = (g, lists)
    return _cache["g"]


def table(dev, d, ld):
    key = ("x", d)
    if key not in _cache:
        x = np.random.RandomState(d).randn(N_TABLE, d).astype(np.float32)
        m = Mat(torch.zeros((N_TABLE, ld), dtype=torch.float32, device=dev), d)
        m.buf[:, :d].copy_(torch.from_numpy(x))
        torch.cuda.synchronize()
        _cache[key] = (x, m)
    return _cache[key]


def run(e, g, op, X, d, row0, n, act=ops.ACT_IDENTITY):
    d4 = (d + 3) // 4 * 4
    big = torch.full((n + 5, d4 + 8), SENTINEL, dtype=torch.float32, device=e.device)
    torch.cuda.synchronize()
    out = Mat(big[2:2 + n], d)
    g.reduce(e, op, X, out, row0, n, act=act)
    e.sync()
    got = big.cpu().numpy()
    assert np.all(got[:2] == SENTINEL) and np.all(got[2 + n:] == SENTINEL), "rows outside the window were written"
    assert np.all(got[:, d4:] == SENTINEL), "columns beyond round_up(d, 4) were written"
    if d4 > d:
        assert np.all(got[2:2 + n, d:d4] == 0), "the pad columns of the last float4 must be zero"
    return got[2:2 + n, :d]


@pytest.mark.parametrize("d,ld", WIDTHS)
@pytest.mark.parametrize("op", sorted(OPS))
def test_csr_reduce_equals_the_oracle(dev, op, d, ld):
    eng.reset_engine()
    e = eng.get_engine()
    g, lists = graph()
    x, X = table(dev, d, ld)
    assert X.ld == ld
    got = run(e, g, OPS[op], X, d, ROW0, N_WIN)
    if op == "max":
        want = fo.reduce_rows(lists, x, "max")[ROW0:ROW0 + N_WIN]
        assert want.dtype == np.float32 and np.array_equal(got, want)
    else:
        want = fo.reduce_rows(lists, x.astype(np.float64), op)[ROW0:ROW0 + N_WIN]
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)
    # empty rows: 0 for mean and max, X[r] for mean-with-self
    for r in (ROW0, ROW0 + 10):
        assert len(lists[r]) == 0
        assert np.array_equal(got[r - ROW0], x[r] if op == "mean_self" else np.zeros(d, np.float32))
    again = run(e, g, OPS[op], X, d, ROW0, N_WIN)
    assert np.array_equal(got, again), "two launches on the same inputs must agree bit for bit (split rows included)"


@pytest.mark.parametrize("op", sorted(OPS))
def test_whole_graph_other_windows_and_relu(dev, op):
    """All rows in one call == the rows window by window (bit for bit: a row's order of additions does not depend on the
    window), cut rows in front of and behind the tested window included; act = relu clamps the result."""
    eng.reset_engine()
    e = eng.get_engine()
    g, lists = graph()
    d, ld = 50, 52
    x, X = table(dev, d, ld)
    whole = run(e, g, OPS[op], X, d, 0, N_TABLE)
    ref = fo.reduce_rows(lists, x.astype(np.float64) if op != "max" else x, op)
    np.testing.assert_allclose(whole, ref, rtol=1e-4, atol=1e-4)
    parts = [run(e, g, OPS[op], X, d, r0, n) for r0, n in ((0, ROW0), (ROW0, N_WIN), (ROW0 + N_WIN, N_TABLE - ROW0 - N_WIN))]
    assert np.array_equal(np.concatenate(parts), whole)
    relu = run(e, g, OPS[op], X, d, 0, N_TABLE, act=ops.ACT_RELU)
    assert np.array_equal(relu, np.maximum(whole, 0))


def test_bad_calls_are_refused_on_the_host(dev):
    from graphsage_amd._lib import GraphsageAmdError
    eng.reset_engine()
    e = eng.get_engine()
    g, _ = graph()
    _, X = table(dev, 12, 12)
    out = Mat.zeros(N_WIN, 12, dev)
    short = Mat(X.buf[:N_TABLE - 1], 12)
    with pytest.raises(GraphsageAmdError, match="rows"):
        g.reduce(e, CSR_MEAN, short, out, ROW0, N_WIN)                # an id could point past the table
    with pytest.raises(GraphsageAmdError):
        g.reduce(e, CSR_MEAN, X, out, N_TABLE - 3, N_WIN)             # window past the graph
    with pytest.raises(GraphsageAmdError, match="unknown op"):
        g.reduce(e, 9, X, out, ROW0, N_WIN)
    narrow = Mat.zeros(N_WIN, 8, dev)
    with pytest.raises(GraphsageAmdError, match="ld"):
        g.reduce(e, CSR_MEAN, X, narrow, ROW0, N_WIN)
    e.sync()
