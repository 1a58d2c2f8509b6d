"""-m gpu: gs_frontier_expand (csrc/gs_frontier.hip) == tests/subset_oracle.py's closure, EXACTLY: rows_out, pos (-1 for every
non-member) and the count word.  Integers only, so there is no tolerance.

Row counts 2 (one node plus the pad row), 255, 256, 257, 300 and 65,537: the count / rank pass cuts the id range into 256
blocks of ceil(n_rows / 256) ids and every block into 256 threads, so these sit on both sides of one id per block, and 65,537
on both sides of 256 ids per block (one id per thread).  Every graph has an empty row, a hub of 3 L + 7 edges (seven rounds of
one wave's 256-edge stride, a ragged last one), a row of one duplicated id, self-loops and the pad row listing itself.  The
flag workspace is read back after every call: it must be all zero again."""
import numpy as np
import pytest
import torch

from graphsage_amd import engine as eng
from graphsage_amd import ops
from graphsage_amd.inference import SPLIT_LEN, FullGraph
import subset_oracle as so

pytestmark = pytest.mark.gpu
L = SPLIT_LEN
ROW_COUNTS = [2, 255, 256, 257, 300, 65537]
_cache = {}


def graph(n_rows):
    """(FullGraph, lists, named row lists).  Row 0: the hub; row 1 (n_rows > 2): empty; row 2: one id 9 times; row 3: self-loops."""
    if n_rows in _cache:
        return _cache[n_rows]
    rng = np.random.RandomState(n_rows)
    n = n_rows - 1
    degs = rng.randint(0, 7, size=n_rows)
    degs[0] = 3 * L + 7
    degs[n] = 4
    if n_rows > 4:
        degs[1:4] = [0, 9, 5]
    # the hub reaches a quarter of the ids at most, so that "the hub" and "all rows" are different answers
    lists = [rng.randint(0, n_rows, size=d) for d in degs]
    lists[0] = rng.randint(0, max(1, n_rows // 4), size=degs[0])
    lists[n] = np.full(4, n)
    if n_rows > 4:
        lists[2][:] = n_rows // 2
        lists[3][:] = [3, 3, 7 % n_rows, 3, n]
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    g = FullGraph(rowptr, np.concatenate(lists).astype(np.int32), n)
    named = {"one row": [n_rows // 3], "all rows": list(range(n_rows)), "with the pad row": sorted({0, n // 2, n}),
             "the hub": [0]}
    if n_rows > 4:
        named.update({"an empty row": [1], "duplicates and self-loops": [2, 3],
                      "scattered": sorted(set(rng.randint(0, n_rows, size=17).tolist()))})
    _cache[n_rows] = (g, g.lists(), named)
    return _cache[n_rows]


class Runner(object):
    def __init__(self, dev, g):
        eng.reset_engine()
        self.e = eng.get_engine()
        self.g = g
        self.rowptr, self.col, _, _ = g.on(self.e.device)
        self.ws = torch.zeros(ops.frontier_ws_bytes(g.n_rows) // 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

    def __call__(self, rows):
        g, e = self.g, self.e
        rows = np.asarray(rows, dtype=np.int32)
        rows_dev = torch.from_numpy(rows).to(e.device) if rows.size else None
        rows_out = torch.full((g.n_rows + 3,), -7, dtype=torch.int32, device=e.device)
        pos = torch.full((g.n_rows + 3,), -7, dtype=torch.int32, device=e.device)
        count = torch.full((3,), -7, dtype=torch.int32, device=e.device)
        torch.cuda.synchronize()
        ops.frontier_expand(self.rowptr, self.col, g.n_rows, rows_dev, rows.size, rows_out[:g.n_rows], pos[:g.n_rows],
                            count[1:2], self.ws, stream=e.stream)
        e.sync()
        c = count.cpu().numpy()
        assert c[0] == -7 and c[2] == -7
        n = int(c[1])
        out, p = rows_out.cpu().numpy(), pos.cpu().numpy()
        assert np.all(out[n:] == -7), "rows_out was written beyond the count"
        assert np.all(p[g.n_rows:] == -7), "pos was written beyond n_rows"
        assert not self.ws[:g.n_rows].any().item(), "the flag workspace must be left zero"
        return out[:n], p[:g.n_rows], n


def check(got, lists, rows):
    out, pos, n = got
    want = so.closure(lists, rows)
    assert n == len(want)
    assert out.dtype == np.int32 and np.array_equal(out, want)
    assert np.array_equal(pos, so.position_map(len(lists), want))
    assert np.all(pos[np.setdiff1d(np.arange(len(lists)), want)] == -1)


@pytest.mark.parametrize("n_rows", ROW_COUNTS)
def test_frontier_equals_the_oracle(dev, n_rows):
    g, lists, named = graph(n_rows)
    run = Runner(dev, g)
    sizes = {}
    for name in sorted(named):                  # every call after the first runs on the workspace the one before left behind
        got = run(named[name])
        check(got, lists, named[name])
        sizes[name] = got[2]
    assert sizes["all rows"] == n_rows
    if n_rows > 4:
        assert sizes["an empty row"] == 1 and sizes["duplicates and self-loops"] == len({2, 3, n_rows // 2, 7, n_rows - 1})
        assert sizes["the hub"] < sizes["all rows"]
    check(run([]), lists, [])                   # nothing in, nothing out: pos all -1, count 0


@pytest.mark.parametrize("n_rows", [300, 65537])
def test_chained_expansions_equal_the_two_hop_closure_and_repeat_bit_for_bit(dev, n_rows):
    g, lists, named = graph(n_rows)
    run = Runner(dev, g)
    start = named["scattered"]
    one = run(start)
    two = run(one[0])
    sets, edges = so.receptive_field(lists, start, 2)
    assert np.array_equal(one[0], sets[1]) and np.array_equal(two[0], sets[2])
    assert np.array_equal(two[1], so.position_map(n_rows, sets[2]))
    assert len(sets[2]) > len(sets[1]) > len(sets[0])
    again = run(one[0])
    assert np.array_equal(again[0], two[0]) and np.array_equal(again[1], two[1]) and again[2] == two[2]


def test_receptive_field_returns_the_oracles_sets_maps_and_edges(dev):
    from graphsage_amd.inference import receptive_field
    g, lists, named = graph(300)
    eng.reset_engine()
    e = eng.get_engine()
    nodes = [41, 7, 41, 299, 130]
    sets, maps, edges = receptive_field(e, g, nodes, 2)
    want, want_edges = so.receptive_field(lists, nodes, 2)
    assert edges == want_edges and len(sets) == len(maps) == 3
    for S, pos, w in zip(sets, maps, want):
        assert S.dtype == np.int32 and np.array_equal(S, w)
        assert pos.dtype == torch.int32 and np.array_equal(pos.cpu().numpy(), so.position_map(300, w))
    again = receptive_field(e, g, nodes, 2)     # the engine's flag workspace was left zero
    assert all(np.array_equal(a, b) for a, b in zip(again[0], sets))


def test_a_short_rows_out_is_not_overrun(dev):
    """rows_out_cap below the member count: the count is still the truth, the list is cut, nothing beyond it is written."""
    g, lists, named = graph(300)
    run = Runner(dev, g)
    e = run.e
    rows = np.asarray(named["the hub"], np.int32)
    want = so.closure(lists, rows)
    buf = torch.full((len(want),), -7, dtype=torch.int32, device=dev)
    pos = torch.empty(g.n_rows, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    rows_dev = torch.from_numpy(rows).to(dev)
    torch.cuda.synchronize()
    ops.frontier_expand(run.rowptr, run.col, g.n_rows, rows_dev, 1, buf[:5], pos, count, run.ws, stream=e.stream)
    e.sync()
    got = buf.cpu().numpy()
    assert int(count.item()) == len(want) and np.array_equal(got[:5], want[:5]) and np.all(got[5:] == -7)
