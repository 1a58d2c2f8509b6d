"""Host side of the importance neighborhoods (no GPU): the NumPy restatement of tests/importance_oracle.py held to the properties
the rule promises, the C ABI of gs_importance_table, the driver flags and their refusals, CSRAdjacency.from_table, and the
reference sampling law on the CSR made from a table."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest

import importance_oracle as io
import walk_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 77


def graph200():
    """200 nodes, 500 random undirected edges among 0 .. 189, rows ascending, one entry per pair; 190 .. 199 have no edges"""
    rng = np.random.RandomState(5)
    rows = [set() for _ in range(200)]
    for a, b in rng.randint(0, 190, size=(500, 2)):
        if a != b:
            rows[a].add(int(b))
            rows[b].add(int(a))
    return wo.csr_from_rows([sorted(r) for r in rows])


_runs = {}


def oracle_run(name, pq=(1.0, 1.0), num_walks=10, walk_len=3):
    """(paths, n_nodes) of num_walks walks from every node of the graph, computed once and never written to."""
    key = (name, pq, num_walks, walk_len)
    if key not in _runs:
        rowptr, col = wo.hand_graph() if name == "hand" else graph200()
        n = len(rowptr) - 1
        paths, _ = wo.walk_paths(rowptr, col, np.arange(n), num_walks, walk_len, wo.thresholds(*pq), SEED)
        paths.setflags(write=False)
        _runs[key] = (paths, n)
    return _runs[key]


def check_rows(paths, num_walks, walk_len, n_nodes, top, slots, pad_id, table, stats):
    """Every property rule 1 - 6 promises of a row, from the paths alone."""
    assert table.shape == (paths.shape[0] // num_walks, slots) and stats.shape == (table.shape[0], 2)
    for i, row in enumerate(table):
        walks = paths[i * num_walks:(i + 1) * num_walks, :walk_len]
        u = int(walks[0, 0])
        c = collections.Counter(int(x) for x in walks[:, 1:].reshape(-1) if 0 <= x < n_nodes and x != u) \
            if 0 <= u < n_nodes else collections.Counter()
        if not c:
            assert np.all(row == pad_id) and tuple(stats[i]) == (0, 0)
            continue
        assert np.all(row != pad_id) and np.all(row != u) and np.all(np.diff(row) >= 0)       # slots non-pad entries, ascending
        n = collections.Counter(int(x) for x in row)
        assert sum(n.values()) == slots and set(n) <= set(c) and len(n) <= top
        assert tuple(stats[i]) == (len(c), len(n))
        for a in c:
            for b in c:
                assert not (c[a] > c[b] and n.get(a, 0) < n.get(b, 0)), (i, a, b)


@pytest.mark.parametrize("name", ["hand", "graph200"])
@pytest.mark.parametrize("top,slots", [(1, 1), (2, 5), (3, 16), (8, 16), (50, 7), (4096, 128)])
def test_the_oracle_keeps_what_the_rule_promises(name, top, slots):
    paths, n = oracle_run(name)
    table, stats = io.importance_rows(paths, 10, 3, n, top, slots, n)
    check_rows(paths, 10, 3, n, top, slots, n, table, stats)
    if name == "graph200":                                           # a node without edges stays put: all pad; no other row is
        deg = np.diff(graph200()[0])
        assert np.all(deg[190:] == 0) and np.array_equal(stats[:, 0] == 0, deg == 0) and np.all(table[deg == 0] == n)


def test_the_oracle_on_rows_worked_by_hand():
    P = 9                                                            # pad id = n_nodes
    # start 0; visits 1 1 1 2 2 3 and the start, the pad id, -1 and an id past the graph, none of which count
    walks = np.array([[0, 1, 1], [0, 1, 2], [0, 2, 3], [0, 0, P], [0, -1, P + 5]], dtype=np.int32)
    row, st = io.importance_row(walks, P, 2, 4, P)                  # top 2: {1: 3, 2: 2}, C = 5: q = (2, 1), r = (2, 3): rest 1 -> node 2
    assert (row, st) == ([1, 1, 2, 2], (3, 2))
    row, st = io.importance_row(walks, P, 3, 6, P)                  # C = 6: exact shares
    assert (row, st) == ([1, 1, 1, 2, 2, 3], (3, 3))
    row, st = io.importance_row(walks, P, 3, 1, P)                  # one slot: q = 0 everywhere, the largest remainder takes it
    assert (row, st) == ([1], (3, 1))
    ties = np.array([[5, 1, 2], [5, 3, 4]], dtype=np.int32)        # four nodes, one visit each
    assert io.importance_row(ties, P, 2, 3, P) == ([1, 1, 2], (4, 2))       # the top boundary and the remainder tie: lowest id
    assert io.importance_row(ties, P, 4, 2, P) == ([1, 2], (4, 2))          # fewer slots than selected nodes
    assert io.importance_row(np.array([[5, 5, 5]]), P, 2, 3, P) == ([P] * 3, (0, 0))
    assert io.importance_row(np.array([[-1, -1, -1]]), P, 2, 3, P) == ([P] * 3, (0, 0))
    assert io.importance_row(np.array([[P, 1, 2]]), P, 2, 3, P) == ([P] * 3, (0, 0))


def test_descriptor_size_symbol_and_abi_version():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    source = open(os.path.join(ROOT, "graphsage_amd", "csrc", "gs_importance.hip")).read()
    asserted = re.search(r"static_assert\(sizeof\(gs_importance_desc\) == (\d+)", source)
    assert asserted and ctypes.sizeof(_lib.ImportanceDesc) == int(asserted.group(1)) == 72
    assert re.search(r"typedef struct gs_importance_desc \{", header)
    assert re.search(r"\bint gs_importance_table\s*\(const gs_importance_desc\*", header)
    for name, value in (("VISITS", _lib.IMPORTANCE_MAX_VISITS), ("TOP", _lib.IMPORTANCE_MAX_TOP), ("SLOTS", _lib.IMPORTANCE_MAX_SLOTS)):
        assert re.search(r"#define GS_IMPORTANCE_MAX_%s %d\b" % (name, value), header)
    assert (_lib.IMPORTANCE_MAX_VISITS, _lib.IMPORTANCE_MAX_TOP, _lib.IMPORTANCE_MAX_SLOTS) == (4096, 4096, 1024)
    lib = _lib.load()
    assert "gs_importance_table" in _lib._PROTOS and "gs_importance_table" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "gs_importance_table")
    assert lib.gs_abi_version() == _lib.GS_ABI_VERSION == 12
    sizes = (ctypes.c_int32 * 16)()
    assert lib.gs_abi_struct_sizes(sizes, 16) == 8


def test_the_entry_point_refuses_before_it_launches():
    from graphsage_amd import _lib
    lib = _lib.load()
    assert lib.gs_importance_table(None, None) == -1 and b"gs_importance_table" in lib.gs_last_error()

    def desc(**kw):
        d = _lib.ImportanceDesc()                                    # every pointer null
        d.n_starts, d.n_nodes, d.ld_paths, d.num_walks, d.walk_len, d.top, d.slots, d.pad_id = 3, 10, 3, 50, 3, 8, 16, 10
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw, word in ((dict(num_walks=0), b"num_walks"), (dict(walk_len=1), b"walk_len"), (dict(num_walks=2049), b"visits"),
                     (dict(num_walks=1, walk_len=4098, ld_paths=4098), b"visits"), (dict(top=0), b"top"), (dict(top=4097), b"top"),
                     (dict(slots=0), b"slots"), (dict(slots=1025), b"slots"), (dict(ld_paths=2), b"ld_paths"),
                     (dict(n_starts=-1), b"n_starts"), (dict(n_nodes=1 << 31), b"n_nodes"), (dict(reserved_=1), b"reserved_"),
                     (dict(), b"non-null")):
        d = desc(**kw)
        assert lib.gs_importance_table(ctypes.addressof(d), None) == -1 and word in lib.gs_last_error(), kw
    d = desc(n_starts=0)                                             # nothing to do: returns at once
    assert lib.gs_importance_table(ctypes.addressof(d), None) == 0
    d = desc(num_walks=2048, n_starts=0)                             # 4096 visits: the largest job
    assert lib.gs_importance_table(ctypes.addressof(d), None) == 0


def test_driver_flags_and_refusals():
    from graphsage_amd import supervised_train as st
    from graphsage_amd import unsupervised_train as ut
    for mod in (st, ut):
        f = mod.build_flags([])
        assert (f.importance_neighbors, f.importance_walks, f.importance_walk_len, f.importance_p, f.importance_q) == (0, 50, 3, 1.0, 1.0)
        st.refuse_importance(f)
        f = mod.build_flags(["--importance_neighbors", "8", "--importance_walks", "200", "--importance_walk_len", "4",
                             "--importance_p", "0.5", "--importance_q", "2", "--max_degree", "16", "--model", "graphsage_seq"])
        assert (f.importance_neighbors, f.importance_walks, f.importance_walk_len, f.importance_p, f.importance_q) == (8, 200, 4, 0.5, 2.0)
        st.refuse_importance(f)
    # off: nothing is checked, whatever the other flags say
    st.refuse_importance(ut.build_flags(["--model", "n2v", "--rank_full", "--importance_walks", "0"]))
    on = ["--importance_neighbors", "8"]
    for argv, word in ((["--importance_walks", "2049"], "4098 visits"), (["--importance_walks", "50", "--importance_walk_len", "84"],
                                                                           "at most 4096"),
                       (["--importance_walks", "0"], "at least 1"), (["--importance_walk_len", "1"], "at least 2"),
                       (["--max_degree", "1025"], "max_degree"), (["--max_degree", "0"], "max_degree"),
                       (["--importance_p", "0.25", "--importance_q", "8"], "1/16"), (["--importance_p", "0"], "positive")):
        for mod in (st, ut):
            with pytest.raises(SystemExit, match=word):
                st.refuse_importance(mod.build_flags(on + argv))
    for bad in ("4097", "-1"):
        with pytest.raises(SystemExit, match="1 .. 4096"):
            st.refuse_importance(st.build_flags(["--importance_neighbors", bad]))
    for argv, word in ((["--model", "n2v"], "n2v"), (["--rank_full"], "rank_full"), (["--topk_full", "5"], "topk_full")):
        with pytest.raises(SystemExit, match="--importance_neighbors.*" + word):
            st.refuse_importance(ut.build_flags(on + argv))
    old = ut.FLAGS, st.FLAGS
    try:                                     # refused before any data is loaded or anything is trained
        with pytest.raises(SystemExit, match="not available with --model n2v"):
            ut.main(["--synthetic", "small", "--model", "n2v"] + on)
        with pytest.raises(SystemExit, match="cannot be combined with --rank_full"):
            ut.main(["--synthetic", "small", "--model", "graphsage_mean", "--rank_full"] + on)
        with pytest.raises(SystemExit, match="cannot be combined with --topk_full"):
            ut.main(["--synthetic", "small", "--model", "graphsage_mean", "--topk_full", "3"] + on)
        with pytest.raises(SystemExit, match="visits per node"):
            st.main(["--synthetic", "small", "--importance_walks", "5000"] + on)
        with pytest.raises(SystemExit, match="max_degree"):
            st.main(["--synthetic", "small", "--max_degree", "2000"] + on)
    finally:
        ut.FLAGS, st.FLAGS = old


def test_the_printed_line():
    from graphsage_amd import supervised_train as st
    f = st.build_flags(["--importance_neighbors", "8", "--max_degree", "16", "--importance_walks", "10"])
    line = st.importance_line(f, "train", 4, np.array([[3, 2], [0, 0], [5, 4], [4, 2]]), 0.25)
    assert line == ("Importance neighborhoods: graph= train top= 8 slots= 16 walks= 10 len= 3 p= 1 q= 1 rows= 4 distinct_mean= 3.00000 "
                    "kept_mean= 2.00000 empty= 1 time= 0.25000")


def table200(top=8, slots=16):
    paths, n = oracle_run("graph200")
    table, _ = io.importance_rows(paths, 10, 3, n, top, slots, n)
    return np.concatenate([table, np.full((1, slots), n, np.int32)]), n


def test_csr_from_a_host_table():
    import torch
    from graphsage_amd._lib import GraphsageAmdError
    from graphsage_amd.neigh_samplers import CSRAdjacency
    table, n = table200()
    adj = CSRAdjacency.from_table(torch.from_numpy(table))
    assert adj.n_nodes == n and adj.rowptr.dtype == torch.int64 and adj.col.dtype == torch.int32
    rowptr, col = adj.rowptr.numpy(), adj.col.numpy()
    empty = np.all(table[:n] == n, axis=1)
    assert empty[190:].all() and 10 <= empty.sum() < n
    assert np.array_equal(np.diff(rowptr), np.where(empty, 0, 16)) and rowptr[0] == 0 and rowptr[-1] == col.size
    for v in range(n):
        assert np.array_equal(col[rowptr[v]:rowptr[v + 1]], table[v] if not empty[v] else table[v][:0])
    none = CSRAdjacency.from_table(torch.full((4, 3), 3, dtype=torch.int32))           # every row pad
    assert none.n_nodes == 3 and none.rowptr.tolist() == [0, 0, 0, 0] and none.col.numel() == 1
    for bad in (table, torch.from_numpy(table).to(torch.int64), torch.zeros(5, dtype=torch.int32)):
        with pytest.raises(GraphsageAmdError, match="from_table"):
            CSRAdjacency.from_table(bad)


def test_the_reference_law_draws_each_row_as_it_stands():
    """num_samples == max_degree == slots: the law takes the list itself, so a call returns a permutation of each non-empty
    row -- every entry as often as it is stored -- and the pad id for an empty one."""
    import torch
    from graphsage_amd.neigh_samplers import CSRAdjacency
    from oracle import sampler_hash as sh
    table, n = table200()
    adj = CSRAdjacency.from_table(torch.from_numpy(table))
    rowptr, col = adj.rowptr.numpy(), adj.col.numpy()
    ids = np.arange(n)
    for step, hop in ((0, 0), (3, 1)):
        got = sh.sample_uniform_csr(rowptr, col, n, n, ids, 16, 123, step, hop, law=sh.LAW_REFERENCE, max_degree=16)
        assert got.shape == (n, 16)
        assert np.array_equal(np.sort(got, axis=1), table[:n])       # rows ascending; an empty row is all pad, which is n
        assert not np.array_equal(got, table[:n])                    # (a permutation, not the identity)
