"""-m gpu: the fused neighbor-overlap ranking kernel (gs_nbr_rank), rank_neighbors and --rank_baselines against the integer
oracle of tests/nbr_rank_oracle.py.  Every comparison is bit for bit in t, n_gt and n_eq, for all four kinds."""
import functools
import os
import re

import numpy as np
import pytest

import nbr_rank_oracle as no
from graphsage_amd import engine as eng
from graphsage_amd import link_heuristics as lh
from graphsage_amd import ops
from graphsage_amd.inference import RankFilter

pytestmark = pytest.mark.gpu
TILE = 256
CHUNK = ops.NBR_PARTNER_CHUNK


# ------------------------------------------------------------------------------------------------ helpers
def csr_of(lists):
    rowptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(r) for r in lists], out=rowptr[1:])
    col = np.concatenate([np.asarray(r, dtype=np.int64) for r in lists]) if rowptr[-1] else np.zeros(0, np.int64)
    return rowptr, col


def graph_of(lists):
    """(SimpleGraph, oracle lists) of rows given as Python lists."""
    n = len(lists)
    rowptr, col = csr_of(lists)
    g = lh.SimpleGraph.from_csr(rowptr, col, n)
    mine = no.simple_lists(rowptr, col, n)
    assert all(np.array_equal(a, b) for a, b in zip(g.lists(), mine))
    return g, mine


def symmetric_lists(n, m, seed):
    rng = np.random.RandomState(seed)
    adj = [set() for _ in range(n)]
    for a, b in zip(rng.randint(0, n, m), rng.randint(0, n, m)):
        if a != b:
            adj[a].add(int(b))
            adj[b].add(int(a))
    return [sorted(a) for a in adj]


def from_edges(n, pairs, symmetric=True):
    adj = [set() for _ in range(n)]
    for a, b in pairs:
        adj[a].add(b)
        if symmetric:
            adj[b].add(a)
    return [sorted(a) for a in adj]


def filter_of(flists, n):
    rowptr, col = csr_of(flists)
    return RankFilter.from_csr(rowptr, col, n)


def check(dev, g, lists, edges, flists=None, tile=TILE, max_workgroups=0, kinds=no.KINDS):
    """rank_neighbors == the oracle, bit for bit, for every kind; returns {kind: result}."""
    e = eng.get_engine()
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    n = g.n_nodes
    filt = filter_of(flists, n) if flists is not None else None
    out = {}
    for kind in kinds:
        want_t, want_gt, want_eq = no.rank(lists, n, edges, kind, flists)
        res = lh.rank_neighbors(e, g, edges, kind=kind, filt=filt, tile=tile, max_workgroups=max_workgroups)
        tag = "%s n=%d tile=%d wgs=%d" % (kind, n, tile, max_workgroups)
        assert res["scores"].dtype == np.uint32 and np.array_equal(res["scores"].astype(np.int64), want_t), tag
        assert np.array_equal(res["n_gt"], want_gt), tag
        assert np.array_equal(res["n_eq"], want_eq), tag
        assert np.array_equal(res["ranks"], 1 + want_gt + want_eq)
        assert res["scale_bits"] == no.weights(kind, lists)[1]
        out[kind] = res
    return out


# ------------------------------------------------------------------------------------------------ 1. tile edges
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 515])
def test_small_tile_on_random_graphs_at_every_tile_edge(dev, n):
    lists = symmetric_lists(n, 3 * n, n)
    g, mine = graph_of(lists)
    rng = np.random.RandomState(n + 1)
    ends = sorted({x for x in (0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, n - 1) if x < n})     # first / last id of every tile
    src = rng.randint(0, n, size=4 * len(ends))
    edges = np.stack([src, np.tile(ends, 4)], axis=1)
    edges = np.concatenate([edges, edges[:, ::-1]])                             # ... as dst and as src
    check(dev, g, mine, edges, flists=mine)
    check(dev, g, mine, edges)


def test_the_only_positive_candidate_sits_at_a_tile_edge(dev):
    n = 515
    spots = [0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, n - 1]
    pairs = []
    for i, x in enumerate(spots):                                              # directed: 10+i -> 30+i -> x, nothing else
        pairs += [(10 + i, 30 + i), (30 + i, x)]
    g, mine = graph_of(from_edges(n, pairs, symmetric=False))
    edges = [(10 + i, x) for i, x in enumerate(spots)] + [(10 + i, 100) for i in range(len(spots))]
    res = check(dev, g, mine, edges)
    k = len(spots)
    assert (res["cn"]["scores"][:k] == 1).all() and not res["cn"]["n_gt"][:k].any() and not res["cn"]["n_eq"][:k].any()
    assert (res["cn"]["n_gt"][k:] == 1).all() and (res["cn"]["n_eq"][k:] == n - 3).all()      # all but src, dst and the one above


def test_default_tile_on_a_sparse_graph_of_two_tiles_and_three(dev):
    n = 2 * ops.NBR_TILE + 3
    lists = symmetric_lists(n, 3 * n, 7)
    g, mine = graph_of(lists)
    rng = np.random.RandomState(8)
    ends = [0, ops.NBR_TILE - 1, ops.NBR_TILE, 2 * ops.NBR_TILE - 1, 2 * ops.NBR_TILE, n - 1]
    edges = np.stack([rng.randint(0, n, 12), np.tile(ends, 2)], axis=1)
    edges = np.concatenate([edges, edges[:6, ::-1]])
    check(dev, g, mine, edges, flists=mine, tile=0)


# ------------------------------------------------------------------------------------------------ 2. row lengths
LENS = (0, 1, 63, 64, 65, 300)          # 300: longer than a workgroup (256 lanes)


def test_row_lengths_around_the_wave_and_the_workgroup(dev):
    """Directed rows of length LENS[v % 6]: N(u) and every N(w) take each length, short and long runs inside a tile included."""
    n = 700
    rng = np.random.RandomState(2)
    lists = [sorted(rng.choice(np.setdiff1d(np.arange(n), [v]), size=LENS[v % 6], replace=False).tolist()) for v in range(n)]
    g, mine = graph_of(lists)
    assert sorted(set(g.deg.tolist())) == list(LENS)
    src = np.arange(12)                                                         # two sources of every length
    edges = np.stack([src, rng.randint(0, n, 12)], axis=1)
    for v in range(1, 6):
        edges[v, 1] = mine[mine[v][0]][0]                                       # a partner that is reached
    check(dev, g, mine, edges, flists=mine)
    check(dev, g, mine, edges, tile=0)


# ------------------------------------------------------------------------------------------------ 3. partner chunks
def test_partners_per_source_around_the_chunk(dev):
    n = 200
    lists = symmetric_lists(n, 500, 3)
    g, mine = graph_of(lists)
    rng = np.random.RandomState(4)
    edges = []
    for u, count in ((5, CHUNK - 1), (6, CHUNK), (7, CHUNK + 1), (8, 2 * CHUNK + 2), (9, 1)):
        edges += [(u, int(x)) for x in rng.randint(0, n, count)]
    edges = np.asarray(edges)[rng.permutation(len(edges))]                     # the caller's order is no group order
    res = check(dev, g, mine, edges, flists=mine)
    t7 = res["cn"]["scores"][edges[:, 0] == 7]
    assert len(t7) == CHUNK + 1 and len(set(t7.tolist())) < len(t7)            # equal t among a source's partners


# ------------------------------------------------------------------------------------------------ 4. structure
def test_star(dev):
    n = 300
    g, mine = graph_of(from_edges(n, [(0, v) for v in range(1, n)]))
    edges = [(1, 2), (299, 1), (0, 5), (5, 0), (0, 0), (7, 7)]
    res = check(dev, g, mine, edges, flists=mine)
    cn = res["cn"]
    assert cn["scores"].tolist() == [1, 1, 0, 0, n - 1, 1]                      # every leaf pair shares the hub
    assert cn["n_gt"][0] == 0 and cn["n_eq"][0] == n - 3                        # the other leaves tie
    assert cn["n_gt"][2] == 0 and cn["n_eq"][2] == 0                            # the hub: every node is filtered or itself
    unfiltered = check(dev, g, mine, edges)["cn"]
    assert unfiltered["n_gt"][2] == 0 and unfiltered["n_eq"][2] == n - 2       # no valid positive: all others tie at 0


def test_complete_bipartite_clique_and_path(dev):
    a, b = 7, 270
    kab = from_edges(a + b, [(i, a + j) for i in range(a) for j in range(b)])
    g, mine = graph_of(kab)
    res = check(dev, g, mine, [(0, 1), (a, a + 1), (a + b - 1, a), (0, a), (a, 0)])
    assert res["cn"]["scores"].tolist() == [b, a, a, 0, 0]
    assert res["cn"]["n_eq"][:3].tolist() == [a - 2, b - 2, b - 2]              # all same-side pairs tie
    n = 70
    g, mine = graph_of(from_edges(n, [(i, j) for i in range(n) for j in range(i)]))
    res = check(dev, g, mine, [(0, 1), (n - 1, 0), (3, 3)], flists=mine)
    assert res["cn"]["scores"].tolist() == [n - 2, n - 2, n - 1]
    n = 600
    g, mine = graph_of(from_edges(n, [(i, i + 1) for i in range(n - 1)]))
    res = check(dev, g, mine, [(0, 2), (2, 0), (255, 257), (257, 255), (0, 1), (599, 597), (300, 10)])
    assert res["cn"]["scores"].tolist() == [1, 1, 1, 1, 0, 1, 0]


def test_isolated_ends_and_an_untouched_tile_between_two_touched(dev):
    """Edges only among the ids of tiles 0 and 2 (tile 1 and the tail hold isolated nodes): tile 1 is never visited, and its
    ids are counted as candidates that score 0."""
    n = 3 * TILE + 40
    rng = np.random.RandomState(5)
    ids = np.concatenate([np.arange(0, TILE - 6), np.arange(2 * TILE, 3 * TILE)])
    pairs = [(int(a), int(b)) for a, b in zip(rng.choice(ids, 1500), rng.choice(ids, 1500)) if a != b]
    g, mine = graph_of(from_edges(n, pairs))
    assert not g.deg[TILE - 6:2 * TILE].any() and not g.deg[3 * TILE:].any()
    iso_a, iso_b = TILE + 3, 3 * TILE + 1
    edges = [(3, 2 * TILE + 5), (2 * TILE + 5, 3), (iso_a, 3), (3, iso_a), (iso_a, iso_b), (iso_a, iso_a), (TILE - 1, 2 * TILE)]
    res = check(dev, g, mine, edges, flists=mine)
    assert res["cn"]["scores"][2:].tolist() == [0] * 5
    assert res["cn"]["n_gt"][2] == 0 and res["cn"]["n_eq"][2] == n - 2          # a source of degree 0: everyone else ties
    assert res["cn"]["n_gt"][3] > 0 and res["cn"]["n_gt"][3] + res["cn"]["n_eq"][3] == n - 2 - g.deg[3]
    check(dev, g, mine, edges)


# ------------------------------------------------------------------------------------------------ 5. the filter
def test_filter_rows(dev):
    n = 520
    lists = symmetric_lists(n, 2500, 6)
    g, mine = graph_of(lists)
    rng = np.random.RandomState(7)
    flists = [np.sort(rng.choice(n, size=rng.randint(0, 30), replace=False)) for _ in range(n)]
    flists[0] = np.zeros(0, np.int64)                                          # an empty row
    flists[1] = np.asarray([7, 300, 519])                                      # holds its query's dst (300)
    flists[2] = np.asarray([2, 9, TILE - 1, TILE, 2 * TILE])                   # holds its own src, and tile edges
    flists[3] = np.arange(n)                                                   # every node
    flists[4] = np.setdiff1d(np.arange(n), [4, 11])                            # everything but src and dst
    edges = [(0, 17), (1, 300), (2, 40), (3, 50), (3, 3), (4, 11), (5, 5), (6, 90), (6, 90), (1, 8), (2, 2), (0, 17)]
    res = check(dev, g, mine, edges, flists=flists)
    for kind in no.KINDS:
        r = res[kind]
        assert r["n_gt"][3] == r["n_eq"][3] == r["n_gt"][4] == r["n_eq"][4] == r["n_gt"][5] == r["n_eq"][5] == 0
        assert (r["n_gt"][7], r["n_eq"][7], r["scores"][7]) == (r["n_gt"][8], r["n_eq"][8], r["scores"][8])     # a repeated edge
    plain = check(dev, g, mine, edges)
    assert (plain["cn"]["n_gt"] + plain["cn"]["n_eq"] >= res["cn"]["n_gt"] + res["cn"]["n_eq"]).all()

# ------------------------------------------------------------------------------------------------ 6. grids, tiles, runs
def test_more_groups_than_workgroups_and_no_state_left_behind(dev):
    """Sources of very different kinds follow one another in one workgroup: long rows, degree 0, many partners, none reached."""
    n = 900
    rng = np.random.RandomState(9)
    lists = symmetric_lists(n, 4000, 9)
    lists[0] = sorted(set(lists[0]) | set(range(300, 700)))                    # a long directed row
    lists += [[] for _ in range(30)]                                           # isolated nodes at the end
    n += 30
    g, mine = graph_of(lists)
    src = np.concatenate([rng.randint(0, n, 150), [0] * 5, [n - 1] * 3, [17] * (CHUNK + 3)])
    edges = np.stack([src, rng.randint(0, n, len(src))], axis=1)[rng.permutation(len(src))]
    assert len(np.unique(src)) > 100
    base = check(dev, g, mine, edges, flists=mine, tile=TILE, max_workgroups=1)
    for tile, wgs in ((TILE, 2), (TILE, 0), (1024, 1), (1024, 2), (0, 0), (TILE, 1)):
        e = eng.get_engine()
        for kind in no.KINDS:
            res = lh.rank_neighbors(e, g, edges, kind=kind, filt=g.rank_filter(), tile=tile, max_workgroups=wgs)
            for key in ("scores", "n_gt", "n_eq"):
                assert np.array_equal(res[key], base[kind][key]), (kind, tile, wgs, key)
            assert res["paths"] == base[kind]["paths"] and res["sources"] == len(np.unique(src))


# ------------------------------------------------------------------------------------------------ 7. a hub
def test_hub_that_forces_fewer_scale_bits(dev):
    """A hub of degree 2^15 over leaves and a few isolated nodes: scale_bits = 15, a source with more neighbors than cursors fit
    in LDS (with and without the cursor workspace), one row that fills whole tiles."""
    import torch
    leaves = 1 << 15
    n = leaves + 1 + 4
    g, mine = graph_of(from_edges(n, [(0, v) for v in range(1, leaves + 1)]))
    assert g.max_degree == leaves > ops.NBR_CURSORS and lh.scale_bits(g.max_degree) == 15
    edges = [(0, 1), (1, 0), (1, 2), (leaves, 1), (0, n - 1), (n - 1, 0), (5, n - 2), (0, 0)]
    res = check(dev, g, mine, edges, flists=mine, tile=0)
    assert res["ra"]["scale_bits"] == res["aa"]["scale_bits"] == 15 and res["cn"]["scale_bits"] == 0
    assert res["ra"]["scores"][2] == 1 and res["aa"]["scores"][2] == int(np.floor(2.0 ** 15 / np.log(leaves) + 0.5))
    assert res["cn"]["n_eq"][2] == leaves - 2 and res["cn"]["scores"][7] == leaves
    # the same launch without the workspace: the hub's cursors are searched again per tile
    e = eng.get_engine()
    order, gp, gs, d = lh.group_by_source(np.asarray(edges)[:, 0], np.asarray(edges)[:, 1])
    rowptr, col, deg = g.on(e.device)
    f_rowptr, f_col = g.rank_filter().on(e.device, n)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(e.device)
    torch.cuda.synchronize()
    t, n_gt, n_eq = ops.nbr_rank(rowptr, col, n, up(gp), up(gs), up(d), f_rowptr=f_rowptr, f_col=f_col, kind="sum",
                                 max_src_degree=0, stream=e.stream)
    e.sync()
    assert np.array_equal(lh._scatter(t.cpu().numpy().view(np.uint32), order), res["cn"]["scores"])
    assert np.array_equal(lh._scatter(n_gt.cpu().numpy(), order), res["cn"]["n_gt"])
    assert np.array_equal(lh._scatter(n_eq.cpu().numpy(), order), res["cn"]["n_eq"])


# ------------------------------------------------------------------------------------------------ 8. the small synthetic graph
@functools.lru_cache(maxsize=None)
def small_reference():
    """The test graph and the held-out edges (both directions) of --synthetic small, and the oracle's answer for every kind."""
    import argparse
    from graphsage_amd import supervised_train as st
    from graphsage_amd import utils
    st.FLAGS = argparse.Namespace(synthetic="small", train_prefix="", sigmoid=False)
    G = st.load_graph()
    rowptr, col = utils.build_csr(G.n_nodes, G.src, G.dst)
    val = np.stack([G.src, G.dst], axis=1)[G.train_removed].astype(np.int64)
    edges = np.concatenate([val, val[:, ::-1]], axis=0)
    lists = no.simple_lists(rowptr, col, G.n_nodes)
    want = {kind: no.rank(lists, G.n_nodes, edges, kind, lists) for kind in no.KINDS}
    return G.n_nodes, rowptr, col, edges, lists, want


def test_rank_neighbors_on_the_small_synthetic_test_graph(dev):
    n, rowptr, col, edges, lists, want = small_reference()
    g = lh.SimpleGraph.from_csr(rowptr, col, n)
    e = eng.get_engine()
    for kind in no.KINDS:
        res = lh.rank_neighbors(e, g, edges, kind=kind, filt=g.rank_filter())
        t, n_gt, n_eq = want[kind]
        assert np.array_equal(res["scores"].astype(np.int64), t) and np.array_equal(res["n_gt"], n_gt)
        assert np.array_equal(res["n_eq"], n_eq)
        mrr, hits = no.metrics(n_gt, n_eq)
        assert res["mrr"] == pytest.approx(mrr, abs=1e-12) and res["hits"] == pytest.approx(hits, abs=1e-12)
        assert res["zero"] == pytest.approx(np.mean(t == 0)) and 0 < res["zero"] < 1
        assert res["sources"] == len(np.unique(edges[:, 0]))
        assert res["paths"] == sum(sum(len(lists[w]) for w in lists[u]) for u in np.unique(edges[:, 0]))
        sf = res["scores_float"]
        if kind == "jaccard":
            deg = np.array([len(r) for r in lists])
            den = deg[edges[:, 0]] + deg[edges[:, 1]] - t
            assert np.array_equal(sf[t > 0], t[t > 0] / den[t > 0]) and not sf[t == 0].any()
        else:
            assert np.array_equal(sf, t / 2.0 ** res["scale_bits"])
        again = lh.rank_neighbors(e, g, edges, kind=kind, filt=g.rank_filter())
        for key in ("scores", "n_gt", "n_eq"):
            assert np.array_equal(res[key], again[key])                       # two runs, bit for bit


# ------------------------------------------------------------------------------------------------ 9. driver
PAT = (r"Link ranking baseline: kind= (\w+) mrr= (\d\.\d{5}) hits@1= (\d\.\d{5}) hits@10= (\d\.\d{5}) hits@50= (\d\.\d{5}) "
       r"hits@100= (\d\.\d{5}) edges= (\d+) zero= (\d\.\d{5}) sources= (\d+) paths= (\d+) scale_bits= (\d+) time= (\d+\.\d{5})")


def test_unsupervised_driver_rank_baselines(dev, tmp_path, capsys, monkeypatch):
    """--rank_baselines prints and writes one line per kind whose numbers are the oracle's on minibatch.test_csr; --model n2v
    prints them too; without the flag nothing of it appears."""
    from graphsage_amd import unsupervised_train as ut
    n, rowptr, col, edges, lists, want = small_reference()
    kept = {}
    real = ut.save_rank_baselines

    def spy(minibatch, out_dir, kinds):
        kept["csr"], kept["val"] = minibatch.test_csr, np.asarray(minibatch.val_edges)
        return real(minibatch, out_dir, kinds)

    monkeypatch.setattr(ut, "save_rank_baselines", spy)
    eng.reset_engine()
    args = ["--synthetic", "small", "--epochs", "1", "--batch_size", "128", "--samples_1", "5", "--samples_2", "3", "--dim_1", "32",
            "--dim_2", "32", "--max_total_steps", "3", "--learning_rate", "0.001", "--max_walk_pairs", "4000",
            "--validate_iter", "10", "--validate_batch_size", "256"]
    ut.main(args + ["--model", "graphsage_mean", "--base_log_dir", str(tmp_path / "on"), "--rank_baselines", "all"])
    out = capsys.readouterr().out
    found = list(re.finditer(PAT, out))
    assert [m.group(1) for m in found] == ["cn", "aa", "ra", "jaccard"], out[-3000:]
    assert np.array_equal(kept["csr"][0], rowptr) and np.array_equal(kept["csr"][1], col)
    assert np.array_equal(np.concatenate([kept["val"], kept["val"][:, ::-1]]), edges)
    files = {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path / "on")) for f in fs}
    for m in found:
        kind = m.group(1)
        assert open(files["rank_baseline_%s.txt" % kind]).read() == m.group(0) + "\n"
        t, n_gt, n_eq = want[kind]
        mrr, hits = no.metrics(n_gt, n_eq)
        assert float(m.group(2)) == pytest.approx(mrr, abs=1e-5)
        assert [float(m.group(i)) for i in (3, 4, 5, 6)] == [pytest.approx(hits[k], abs=1e-5) for k in (1, 10, 50, 100)]
        assert int(m.group(7)) == len(edges) and float(m.group(8)) == pytest.approx(np.mean(t == 0), abs=1e-5)
        assert int(m.group(9)) == len(np.unique(edges[:, 0])) and int(m.group(11)) == no.weights(kind, lists)[1]
    assert "val.npy" in files and "rank_full.txt" not in files
    eng.reset_engine()
    ut.main(args + ["--model", "n2v", "--learning_rate", "0.1", "--base_log_dir", str(tmp_path / "n2v"), "--rank_baselines", "ra"])
    m = re.search(PAT, capsys.readouterr().out)
    mrr, _ = no.metrics(want["ra"][1], want["ra"][2])
    assert m and m.group(1) == "ra" and float(m.group(2)) == pytest.approx(mrr, abs=1e-5)
    assert any(f == "rank_baseline_ra.txt" for _, _, fs in os.walk(str(tmp_path / "n2v")) for f in fs)
    eng.reset_engine()
    ut.main(args + ["--model", "graphsage_mean", "--base_log_dir", str(tmp_path / "off")])
    assert "Link ranking baseline" not in capsys.readouterr().out
    assert not any(f.startswith("rank_baseline_") for _, _, fs in os.walk(str(tmp_path / "off")) for f in fs)
