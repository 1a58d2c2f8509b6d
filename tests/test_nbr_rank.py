"""Neighbor-overlap link-ranking baselines without a GPU: the oracle against a set-intersection restatement, the host-side
normalisation, weights, grouping and refusals, the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import nbr_rank_oracle as no

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def symmetric_csr(n, m, seed):
    """A random symmetric simple graph on n nodes from m drawn pairs, as (rowptr, col)."""
    rng = np.random.RandomState(seed)
    a, b = rng.randint(0, n, m), rng.randint(0, n, m)
    keep = a != b
    a, b = np.concatenate([a[keep], b[keep]]), np.concatenate([b[keep], a[keep]])
    key = np.unique(a.astype(np.int64) * n + b)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=rowptr[1:])
    return rowptr, key % n


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("n,m,seed", [(30, 60, 0), (47, 200, 1), (60, 90, 2)])
def test_oracle_equals_set_intersection_on_symmetric_graphs(n, m, seed):
    rowptr, col = symmetric_csr(n, m, seed)
    lists = no.simple_lists(rowptr, col, n)
    rng = np.random.RandomState(seed + 10)
    edges = np.stack([rng.randint(0, n, 12), rng.randint(0, n, 12)], axis=1)
    edges[0] = [edges[0, 0], edges[0, 0]]                                       # src == dst
    edges[1] = edges[2]                                                         # a repeated edge
    deg = np.array([len(r) for r in lists])
    for kind in no.KINDS:
        t, n_gt, n_eq = no.rank(lists, n, edges, kind, flists=lists)
        for k, (u, x) in enumerate(edges):
            s = np.array([no.brute(lists, n, u, y, kind) for y in range(n)], dtype=object)
            assert t[k] == s[x]
            valid = [y for y in range(n) if y != x and y != u and y not in set(lists[u].tolist())]
            if kind == "jaccard":
                key = lambda y: (int(s[y]), int(deg[u] + deg[y] - s[y]))
                cmp = lambda y: key(y)[0] * key(x)[1] - key(x)[0] * key(y)[1]
            else:
                cmp = lambda y: int(s[y]) - int(s[x])
            assert n_gt[k] == sum(1 for y in valid if cmp(y) > 0)
            assert n_eq[k] == sum(1 for y in valid if cmp(y) == 0)
        assert (t[1], n_gt[1], n_eq[1]) == (t[2], n_gt[2], n_eq[2])
        mrr, hits = no.metrics(n_gt, n_eq)
        assert 0 < mrr <= 1 and hits[1] <= hits[10] <= hits[50] <= hits[100] <= 1


def test_oracle_follows_paths_on_a_directed_graph():
    """P(u, x) = {w in N(u) : x in N(w)}: rows are followed as stored, not symmetrised."""
    #       0 -> 1, 2     1 -> 3     2 -> 3, 4     3 -> (none)     4 -> 0
    lists = [np.array(r, dtype=np.int64) for r in ([1, 2], [3], [3, 4], [], [0])]
    q = np.ones(5, np.int64)
    assert no.score_row(lists, q, 0, 5).tolist() == [0, 0, 0, 2, 1]
    assert no.score_row(lists, q, 3, 5).tolist() == [0] * 5                    # 3 is reached, but leads nowhere
    assert no.score_row(lists, q, 4, 5).tolist() == [0, 1, 1, 0, 0]
    t, n_gt, n_eq = no.rank(lists, 5, [[0, 3], [0, 4], [3, 0], [0, 0]], "cn")
    assert t.tolist() == [2, 1, 0, 0]
    assert (n_gt.tolist(), n_eq.tolist()) == ([0, 1, 0, 2], [0, 0, 3, 2])
    # jaccard: node 3 has an empty row and lies in both rows of N(0): 2 / (2 + 0 - 2), above every finite ratio
    t, n_gt, n_eq = no.rank(lists, 5, [[0, 3], [0, 4]], "jaccard")
    assert t.tolist() == [2, 1] and n_gt.tolist() == [0, 1] and n_eq.tolist() == [0, 0]
    # ra weighs the middle node by its out-degree: s(0, 3) = q(1) + q(2), s(0, 4) = q(2)
    qr, S = no.weights("ra", lists)
    assert S == 16 and qr.tolist() == [1 << 15, 1 << 16, 1 << 15, 0, 1 << 16]
    assert no.score_row(lists, qr, 0, 5).tolist() == [0, 0, 0, 3 << 15, 1 << 15]
    # aa: q(1) = 0, so a middle node of degree 1 carries nothing
    qa, _ = no.weights("aa", lists)
    assert qa[1] == 0 and qa[0] == qa[2] == int(np.floor(2.0 ** 16 / np.log(2.0) + 0.5))


# ------------------------------------------------------------------------------------------------ SimpleGraph
def test_simple_graph_normalises_rows():
    from graphsage_amd._lib import GraphsageAmdError
    from graphsage_amd.link_heuristics import SimpleGraph
    n = 5
    rows = [[3, 1, 1, 0, 5, 9], [], [4, 3, 2, 2], [0], [4, 4]]                  # duplicates, loops (0, 2, 4), pads (5, 9), descending
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    col = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows])
    g = SimpleGraph.from_csr(rowptr, col, n)
    assert [r.tolist() for r in g.lists()] == [[1, 3], [], [3, 4], [0], []]
    assert g.rowptr.dtype == np.int64 and g.col.dtype == np.int32 and g.deg.tolist() == [2, 0, 2, 1, 0] and g.max_degree == 2
    assert [r.tolist() for r in no.simple_lists(rowptr, col, n)] == [r.tolist() for r in g.lists()]
    assert g.two_hop_work([0, 1, 2, 3]).tolist() == [1, 0, 1, 2]
    f = g.rank_filter()
    assert f.n_nodes == n and np.array_equal(f.rowptr, g.rowptr) and np.array_equal(f.col, g.col)
    empty = SimpleGraph.from_csr(np.zeros(4, np.int64), np.zeros(0, np.int32), 3)
    assert empty.max_degree == 0 and empty.col.size == 0
    for rp, c in (([0, 2, 1, 3, 3, 3, 3], [0, 1, 2]), ([0, 1, 2], [0, 1]), ([1, 1, 1, 1, 1, 1], [0]), ([0, 0, 0, 0, 0, 2], [0]),
                  ([0, 1, 1, 1, 1, 1], [-1])):
        with pytest.raises(GraphsageAmdError):
            SimpleGraph.from_csr(np.asarray(rp), np.asarray(c), n)


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("bits", range(1, 32))
def test_weight_sums_stay_below_2_32_for_every_bit_length(bits):
    """The worst case of a bit length: max_degree = 2^bits - 1 middle nodes of the heaviest weight (aa: degree 2, ra: degree 1)."""
    from graphsage_amd import link_heuristics as lh
    max_degree = (1 << bits) - 1
    S = lh.scale_bits(max_degree)
    assert S == no.scale_bits(max_degree) == min(16, 31 - bits) and S >= 0
    for kind, k in (("aa", 2), ("ra", 1)):
        q, got = lh.neighbor_weights(kind, np.array([max_degree, k]))
        assert got == S
        assert max_degree * int(q.max()) < 1 << 32 and int(q[1]) == q.max()
        assert max_degree * (1.4427 * 2.0 ** S + 0.5) < 2.0 ** 31.53 + 2.0 ** 30 < 2.0 ** 32


def test_weights_are_positive_monotone_and_match_the_oracle():
    from graphsage_amd import link_heuristics as lh
    deg = np.concatenate([np.arange(0, 3000), [2 ** 15, 2 ** 15 + 1, 2 ** 20, 2 ** 26]])
    for top in (len(deg), 3000):                                               # S = 4 and S = 16 - 12 + ... whatever the top gives
        d = deg[:top]
        for kind in ("aa", "ra"):
            q, S = lh.neighbor_weights(kind, d)
            assert q.dtype == np.uint32 and S == lh.scale_bits(int(d.max()))
            lo = 2 if kind == "aa" else 1
            assert (q[d >= lo] >= 1).all() and not q[d < lo].any()
            assert (np.diff(q[d >= lo].astype(np.int64)) <= 0).all()           # non-increasing in k (d ascends)
            assert q.tolist() == [no.weight(kind, int(k), S) for k in d]
    for kind in ("cn", "jaccard"):
        q, S = lh.neighbor_weights(kind, deg)
        assert S == 0 and q.dtype == np.uint32 and (q == 1).all()
    assert lh.scale_bits(0) == 16 and lh.scale_bits(2 ** 15 - 1) == 16 and lh.scale_bits(2 ** 15) == 15
    with pytest.raises(lh.GraphsageAmdError):
        lh.neighbor_weights("katz", deg)


# ------------------------------------------------------------------------------------------------ grouping
def test_grouping_by_source_keeps_the_callers_order():
    from graphsage_amd import link_heuristics as lh
    rng = np.random.RandomState(4)
    src, dst = rng.randint(0, 9, 50), rng.randint(0, 9, 50)
    src[10], dst[10] = src[3], dst[3]                                           # a repeated edge
    for work in (None, rng.randint(0, 5, 9)):
        order, gp, gs, d = lh.group_by_source(src, dst, work)
        assert sorted(order.tolist()) == list(range(50)) and gp[0] == 0 and gp[-1] == 50 and len(set(gs.tolist())) == len(gs)
        for g in range(len(gs)):
            mine = order[gp[g]:gp[g + 1]]
            assert (src[mine] == gs[g]).all() and (np.diff(mine) > 0).all()    # stable: a source's partners in the caller's order
            assert np.array_equal(d[gp[g]:gp[g + 1]], dst[mine])
        if work is None:
            assert (np.diff(gs) > 0).all()
        else:
            assert (np.diff(work[gs]) <= 0).all()                              # heaviest first
        per_group_value = 100 * src[order] + dst[order]                         # what a kernel would answer, in group order
        assert np.array_equal(lh._scatter(per_group_value, order), 100 * src + dst)


# ------------------------------------------------------------------------------------------------ refusals
def test_module_refusals_come_before_any_launch():
    """Bad arguments never reach the device: the engine below has none."""
    from graphsage_amd import link_heuristics as lh
    from graphsage_amd.inference import RankFilter
    rowptr, col = symmetric_csr(12, 30, 3)
    g = lh.SimpleGraph.from_csr(rowptr, col, 12)
    for kw in (dict(edges=[[0, 12]]), dict(edges=[[-1, 3]]), dict(kind="pa"), dict(tile=100), dict(tile=32),
               dict(tile=2 * lh.ops.NBR_MAX_TILE), dict(filt=RankFilter.from_csr(np.zeros(14, np.int64), np.zeros(0, np.int32), 13))):
        args = dict(edges=[[0, 1]])
        args.update(kw)
        with pytest.raises(lh.GraphsageAmdError):
            lh.rank_neighbors(None, g, **args)
    with pytest.raises(lh.GraphsageAmdError, match="SimpleGraph"):
        lh.rank_neighbors(None, object(), [[0, 1]])
    res = lh.rank_neighbors(None, g, np.zeros((0, 2), np.int64), kind="ra")
    assert res["mrr"] == 0.0 and res["scores"].dtype == np.uint32 and res["paths"] == 0 and res["scale_bits"] == 16


def test_driver_flag_default_and_refusal(capsys):
    from graphsage_amd import link_heuristics as lh
    from graphsage_amd import unsupervised_train as ut
    f = ut.build_flags([])
    assert f.rank_baselines == "" and ut.rank_baseline_kinds(f) == []          # the default: nothing runs, nothing is printed
    assert ut.rank_baseline_kinds(ut.build_flags(["--rank_baselines", "ra,cn"])) == ["ra", "cn"]
    assert ut.rank_baseline_kinds(ut.build_flags(["--rank_baselines", "all"])) == ["cn", "aa", "ra", "jaccard"]
    assert lh.parse_kinds("jaccard, all") == ["jaccard", "cn", "aa", "ra"]
    capsys.readouterr()
    for model in ("graphsage_mean", "n2v"):
        with pytest.raises(SystemExit) as ei:
            ut.main(["--synthetic", "small", "--model", model, "--rank_baselines", "cn,katz"])
        assert "--rank_baselines" in str(ei.value) and "katz" in str(ei.value)
        assert "Loading training data" not in capsys.readouterr().out
    line = lh.result_line("aa", {"mrr": 0.25, "hits": {1: 0.0, 10: 0.5, 50: 1.0, 100: 1.0}, "ranks": np.arange(4), "zero": 0.75,
                                 "sources": 3, "paths": 123456789012, "scale_bits": 16}, 0.5)
    assert line == ("Link ranking baseline: kind= aa mrr= 0.25000 hits@1= 0.00000 hits@10= 0.50000 hits@50= 1.00000 "
                    "hits@100= 1.00000 edges= 4 zero= 0.75000 sources= 3 paths= 123456789012 scale_bits= 16 time= 0.50000")


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_binding_and_library_agree():
    from graphsage_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    for name in ("gs_nbr_rank_grid", "gs_nbr_rank_ws_bytes", "gs_nbr_rank"):
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"typedef struct gs_nbr_rank_desc \{", header)
    version = int(re.search(r"#define GS_ABI_VERSION (\d+)\b", header).group(1))
    lib = _lib.load()                                                     # binds every name of _PROTOS: the library exports them
    assert lib.gs_abi_version() == version == _lib.GS_ABI_VERSION         # entry points were added, no layout changed
    sizes = (ctypes.c_int32 * 16)()
    assert lib.gs_abi_struct_sizes(sizes, 16) == 8                        # the descriptor goes by pointer
    assert ctypes.sizeof(_lib.NbrRankDesc) == 160
    const = lambda n: int(re.search(r"#define %s (\d+)\b" % n, header).group(1))
    assert const("GS_NBR_TILE") == ops.NBR_TILE and const("GS_NBR_PARTNER_CHUNK") == ops.NBR_PARTNER_CHUNK
    assert (const("GS_NBR_MIN_TILE"), const("GS_NBR_MAX_TILE"), const("GS_NBR_CURSORS")) == (ops.NBR_MIN_TILE, ops.NBR_MAX_TILE,
                                                                                             ops.NBR_CURSORS)
    assert ops.NBR_TILE & (ops.NBR_TILE - 1) == 0 and ops.NBR_MIN_TILE <= 256 <= ops.NBR_TILE <= ops.NBR_MAX_TILE
    assert (const("GS_NBR_SUM"), const("GS_NBR_JACCARD")) == (ops.NBR_KINDS["sum"], ops.NBR_KINDS["jaccard"])
    src = open(os.path.join(ROOT, "graphsage_amd", "csrc", "gs_nbr_rank.hip")).read()
    assert "sizeof(gs_nbr_rank_desc) == 160" in src
    assert not re.search(r"\b(float|double)\b", re.sub(r"//[^\n]*", "", src))           # integers only

    out = ctypes.c_int64(-1)
    for wgs, deg, want in ((8, ops.NBR_CURSORS, 0), (8, ops.NBR_CURSORS + 1, 8 * (ops.NBR_CURSORS + 1) * 4), (0, 10 ** 6, 0)):
        assert lib.gs_nbr_rank_ws_bytes(wgs, deg, ctypes.byref(out)) == 0 and out.value == want
    assert lib.gs_nbr_rank_ws_bytes(-1, 5, ctypes.byref(out)) == -1 and b"gs_nbr_rank_ws_bytes" in lib.gs_last_error()

    # every bad call is refused before anything is launched or read (the pointers below are host memory)
    assert lib.gs_nbr_rank(None, None) == -1 and b"gs_nbr_rank" in lib.gs_last_error()
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)

    def desc(**kw):
        q = _lib.NbrRankDesc()
        for name in ("rowptr", "col", "group_ptr", "group_src", "dst", "t", "n_gt", "n_eq"):
            setattr(q, name, p)
        q.n_nodes, q.n_groups, q.n_queries, q.kind = 5, 1, 1, ops.NBR_KINDS["sum"]
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    for kw, word in ((dict(n_nodes=-1), b"bad sizes"), (dict(n_nodes=1 << 31), b"bad sizes"), (dict(n_queries=0), b"bad sizes"),
                     (dict(kind=2), b"kind"), (dict(tile=100), b"power of two"), (dict(tile=32), b"power of two"),
                     (dict(tile=2 * ops.NBR_MAX_TILE), b"power of two"), (dict(max_workgroups=-1), b"negative"),
                     (dict(dst=None), b"non-null"), (dict(kind=1), b"Jaccard"), (dict(kind=1, deg=p, q=p), b"Jaccard"),
                     (dict(f_rowptr=p), b"filter")):
        q = desc(**kw)
        assert lib.gs_nbr_rank(ctypes.addressof(q), None) == -1 and word in lib.gs_last_error(), kw
    q = desc(n_groups=0, n_queries=0)
    assert lib.gs_nbr_rank(ctypes.addressof(q), None) == 0                # nothing to do, nothing launched
