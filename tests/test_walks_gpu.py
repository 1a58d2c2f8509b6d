"""-m gpu: the second-order (p, q) random-walk kernels (gs_walk_paths, gs_walk_pairs) and device_walk_pairs against the NumPy
uint64 restatement of walk_oracle.py, bit for bit, at the smallest shapes that can go wrong; the walk law on the device's own
output; the unsupervised driver with --walk_p / --walk_q.

A walk's stream depends on (seed, global walk index) only, so the first n walks of a job are the job of n walks: the oracle
runs once per (graph, p, q, walk_len) for 257 walks and serves every n_walks."""
import os
import re

import numpy as np
import pytest
import torch

import walk_oracle as wo
from test_walks import LAW_PQ, LAW_SEED, LAW_WALKS, check_law

pytestmark = pytest.mark.gpu

PQS = [(1.0, 1.0), (0.5, 2.0), (4.0, 0.25), (4.0, 4.0)]
N_WALKS = (1, 63, 65, 257)           # below / above one wave, above one workgroup
WALK_LENS = (1, 2, 5, 80)
SEED = 20240


def _syn300():
    from graphsage_amd import utils
    G = utils.synthetic_graph(n_nodes=300, feat_dim=4, num_classes=3, avg_degree=6, seed=7)
    rowptr, col = utils.build_csr_numpy(G.n_nodes, G.src, G.dst)               # symmetric, rows ascending, one entry per pair
    return rowptr, col, np.arange(0, 300, 2), 2


def _hub():
    """node 0 next to 1 .. 1500 (a search of 11 probes), the spokes chained in pairs so that common neighbors exist"""
    rows = [list(range(1, 1501))]
    for i in range(1, 1501):
        mate = i + 1 if i % 2 else i - 1
        rows.append(sorted([0, mate]))
    rowptr, col = wo.csr_from_rows(rows)
    return rowptr, col, [0, 1, 2, 1500, 0], 52


def _graphs():
    hand = wo.hand_graph()
    return {
        "hand": hand + (list(range(6)), 43),
        "syn300": _syn300(),
        # 0 is a leaf: from it the only candidate is the way back, accepted at 1/16 per attempt under p = 4, q = 0.25
        "degree1": wo.csr_from_rows([[1], [0, 2, 3], [1], [1]]) + ([0, 2, 3, 1], 65),
        "hub": _hub(),
        "duplicates": wo.csr_from_rows([[1, 1, 2], [0, 0, 2, 2, 2], [0, 1, 1, 3, 3], [2, 2]]) + ([0, 1, 2, 3], 65),
        "directed": wo.csr_from_rows([[1, 2], [2], [], [0, 4], [3, 3, 5], [5]]) + ([0, 1, 2, 3, 4, 5], 43),
        # node 6 has no edges; -1, 7 = n_nodes, 100 and the extremes are no nodes; 3 and 0 repeat
        "bad_starts": wo.csr_from_rows([[1, 2], [0, 2, 3, 5], [0, 1], [1, 4], [3], [1], []])
        + ([0, 6, -1, 7, 3, 3, 100, 0, -2 ** 31, 2 ** 31 - 1, 5], 24),
        # 4 = n_nodes, the pad id of the padded tables: walked to, never from
        "pad_entry": wo.csr_from_rows([[1, 4], [0, 2, 4], [1, 3, 4], [2, 4]]) + ([0, 1, 2, 3], 65),
    }


GRAPHS = _graphs()
_oracle = {}


def oracle(name, pq, walk_len):
    """257 walks, computed once and never written to."""
    k = (name, pq, walk_len)
    if k not in _oracle:
        rowptr, col, starts, num_walks = GRAPHS[name]
        paths, counts = wo.walk_paths(rowptr, col, starts, num_walks, walk_len, wo.thresholds(*pq), SEED, n_walks=257)
        paths.setflags(write=False)
        counts.setflags(write=False)
        _oracle[k] = (paths, counts)
    return _oracle[k]


def on_device(name, dev):
    rowptr, col, starts, num_walks = GRAPHS[name]
    return (torch.from_numpy(np.asarray(rowptr, dtype=np.int64)).to(dev), torch.from_numpy(np.asarray(col, dtype=np.int32)).to(dev),
            torch.from_numpy(np.asarray(starts, dtype=np.int32)).to(dev), num_walks)


def device_run(rowptr, col, starts, num_walks, walk_len, pq, n_walks, walk0=0, seed=SEED):
    from graphsage_amd import ops
    paths, counts = ops.walk_paths(rowptr, col, starts, num_walks, walk_len, ops.walk_thresholds(*pq), seed, walk0=walk0,
                                   n_walks=n_walks)
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    pairs = ops.walk_pairs(paths, ends - counts, int(ends[-1]))
    torch.cuda.synchronize()
    return paths.cpu().numpy(), counts.cpu().numpy(), pairs.cpu().numpy()


@pytest.mark.parametrize("pq", PQS, ids=lambda pq: "p%g_q%g" % pq)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_paths_counts_and_pairs_are_bit_equal_to_the_oracle(dev, name, pq):
    rowptr, col, starts, num_walks = on_device(name, dev)
    assert starts.numel() * num_walks >= 257
    for walk_len in WALK_LENS:
        want_paths, want_counts = oracle(name, pq, walk_len)
        for n in N_WALKS:
            paths, counts, pairs = device_run(rowptr, col, starts, num_walks, walk_len, pq, n)
            where = (name, pq, walk_len, n)
            assert paths.shape == (n, walk_len) and paths.dtype == np.int32 and np.array_equal(paths, want_paths[:n]), where
            assert np.array_equal(counts, want_counts[:n]), where
            assert np.array_equal(pairs, wo.walk_pairs(want_paths[:n], want_counts[:n])), where


def test_the_cases_reach_what_they_are_there_for():
    """The oracle's runs do take the paths the graphs were built for (else the parity above would show less than it says)."""
    stats = {}
    rowptr, col, starts, num_walks = GRAPHS["degree1"]
    wo.walk_paths(rowptr, col, starts, num_walks, 80, wo.thresholds(4, 0.25), SEED, n_walks=257, stats=stats)
    assert stats["attempts"] > 20 * 257 * 79 / 4 and stats["capped"] == 0      # a leaf's only way out is accepted at 1/16
    paths, counts = oracle("bad_starts", (0.5, 2.0), 5)                        # 24 walks per start id
    assert np.all(paths[:24, 0] == 0) and counts[:24].min() > 0
    assert np.all(paths[24:48] == 6) and np.all(counts[24:48] == 0)            # a node without edges: the walk stays
    for lo, hi in ((48, 96), (144, 168), (192, 240)):                          # -1 and 7; 100; the extremes
        assert np.all(paths[lo:hi] == -1) and np.all(counts[lo:hi] == 0)
    assert np.all(paths[96:144, 0] == 3) and not np.array_equal(paths[96:120], paths[120:144])      # a repeated id: new walks
    paths, counts = oracle("pad_entry", (0.5, 2.0), 5)
    assert np.any(paths == 4) and counts.max() == 4
    for row in paths:                                                          # once at the pad id, always there
        k = np.nonzero(row == 4)[0]
        assert k.size == 0 or np.all(row[k[0]:] == 4)
    paths, _ = oracle("directed", (1.0, 1.0), 80)
    assert np.all(paths[paths[:, 0] == 2] == 2)                                # a dead end
    assert np.all(paths[np.isin(paths[:, 0], (0, 1)), -1] == 2)                # and where the walks from 0 and 1 end up
    paths, _ = oracle("hub", (4.0, 0.25), 5)
    assert np.any(paths[:, 1:] == 0) and len(np.unique(paths)) > 100
    paths, _ = oracle("duplicates", (1.0, 1.0), 2)                             # an entry stored three times of five
    first = paths[paths[:, 0] == 1, 1]
    assert 0.4 < np.mean(first == 2) < 0.8


def test_chunks_through_walk0_give_the_walks_of_one_call(dev):
    rowptr, col, starts, num_walks = on_device("syn300", dev)
    for pq in ((0.5, 2.0), (1.0, 1.0)):
        whole = device_run(rowptr, col, starts, num_walks, 5, pq, 257)
        parts = [device_run(rowptr, col, starts, num_walks, 5, pq, min(64, 257 - w0), walk0=w0) for w0 in range(0, 257, 64)]
        assert len(parts) == 5 and parts[-1][0].shape[0] == 1
        for k in range(3):
            assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), (pq, k)
    # a chunk that does not begin at 0, against the oracle run with the same walk0
    want_paths, want_counts = wo.walk_paths(*GRAPHS["syn300"][:2], GRAPHS["syn300"][2], num_walks, 5, wo.thresholds(0.5, 2.0), SEED,
                                            walk0=130, n_walks=65)
    paths, counts, pairs = device_run(rowptr, col, starts, num_walks, 5, (0.5, 2.0), 65, walk0=130)
    assert np.array_equal(paths, want_paths) and np.array_equal(counts, want_counts)
    assert np.array_equal(pairs, wo.walk_pairs(want_paths, want_counts))


def test_two_launches_give_the_same_bytes(dev):
    rowptr, col, starts, num_walks = on_device("hub", dev)
    for pq in ((4.0, 0.25), (1.0, 1.0)):
        a = device_run(rowptr, col, starts, num_walks, 80, pq, 257)
        b = device_run(rowptr, col, starts, num_walks, 80, pq, 257)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        c = device_run(rowptr, col, starts, num_walks, 80, pq, 257, seed=SEED + 1)       # another seed is another stream
        assert not np.array_equal(a[0], c[0])


def test_device_walk_pairs(dev):
    from graphsage_amd import utils
    rowptr_h, col_h, _, _ = GRAPHS["bad_starts"]
    rowptr, col = torch.from_numpy(rowptr_h).to(dev), torch.from_numpy(col_h).to(dev)
    nodes = np.array([0, 6, 3, 3, 5, 2])                                       # 6 has no edges: dropped (utils.py:80-81)
    kept = nodes[nodes != 6]
    for pq in ((0.5, 2.0), (1.0, 1.0)):
        want_paths, want_counts = wo.walk_paths(rowptr_h, col_h, kept, 7, 6, wo.thresholds(*pq), 99)
        pairs, paths = utils.device_walk_pairs(rowptr, col, nodes, num_walks=7, walk_len=6, p=pq[0], q=pq[1], seed=99,
                                               return_paths=True)
        assert pairs.dtype == torch.int32 and pairs.is_cuda and np.array_equal(paths.cpu().numpy(), want_paths)
        want_pairs = wo.walk_pairs(want_paths, want_counts)
        assert np.array_equal(pairs.cpu().numpy(), want_pairs)
        chunked = utils.device_walk_pairs(rowptr, col, nodes, num_walks=7, walk_len=6, p=pq[0], q=pq[1], seed=99, chunk_walks=4)
        assert np.array_equal(chunked.cpu().numpy(), want_pairs)
        # max_pairs: fewer start nodes, then a seeded truncation; the same call gives the same pairs
        capped = utils.device_walk_pairs(rowptr, col, nodes, num_walks=7, walk_len=6, p=pq[0], q=pq[1], seed=99, max_pairs=40)
        again = utils.device_walk_pairs(rowptr, col, nodes, num_walks=7, walk_len=6, p=pq[0], q=pq[1], seed=99, max_pairs=40)
        assert 0 < capped.shape[0] <= 40 and torch.equal(capped, again)
        assert len(set(capped[:, 0].tolist())) <= int(np.ceil(40 / 35.0))
    with pytest.raises(ValueError, match=r"\[0, 7\)"):
        utils.device_walk_pairs(rowptr, col, [0, 7], p=0.5, q=2.0)
    with pytest.raises(ValueError, match="1/16"):
        utils.device_walk_pairs(rowptr, col, [0], p=0.25, q=8.0)
    empty = utils.device_walk_pairs(rowptr, col, [6], p=0.5, q=2.0)
    assert tuple(empty.shape) == (0, 2) and empty.dtype == torch.int32


def test_device_walk_pairs_wants_sorted_rows_only_where_it_searches(dev):
    from graphsage_amd import utils
    rowptr_h, col_h = wo.csr_from_rows([[2, 1], [0, 2, 5, 3], [1, 0], [1, 4], [3], [1]])      # the hand graph, rows 0 to 2 shuffled
    rowptr, col = torch.from_numpy(rowptr_h).to(dev), torch.from_numpy(col_h).to(dev)
    for p, q in ((0.5, 2.0), (1.0, 0.5), (4.0, 4.0)):
        with pytest.raises(ValueError, match="row 0 of the adjacency is not ascending"):
            utils.device_walk_pairs(rowptr, col, [0, 1], num_walks=3, p=p, q=q)
    pairs, paths = utils.device_walk_pairs(rowptr, col, [0, 1], num_walks=40, walk_len=4, p=1.0, q=1.0, seed=5, return_paths=True)
    want_paths, want_counts = wo.walk_paths(rowptr_h, col_h, [0, 1], 40, 4, wo.thresholds(1, 1), 5)
    assert np.array_equal(paths.cpu().numpy(), want_paths) and np.array_equal(pairs.cpu().numpy(), wo.walk_pairs(want_paths))
    # a sorted graph passes, and the verdict of one graph is not carried over to the next
    good = wo.hand_graph()
    utils.device_walk_pairs(torch.from_numpy(good[0]).to(dev), torch.from_numpy(good[1]).to(dev), [0, 1], num_walks=3, p=0.5, q=2.0)
    with pytest.raises(ValueError, match="not ascending"):
        utils.device_walk_pairs(rowptr, col, [0, 1], num_walks=3, p=0.5, q=2.0)


def test_the_device_obeys_the_law(dev):
    """The law test of test_walks.py on the kernel's own output (which is also the oracle's, bit for bit)."""
    from graphsage_amd import ops
    rowptr_h, col_h = wo.hand_graph()
    rowptr, col = torch.from_numpy(rowptr_h).to(dev), torch.from_numpy(col_h).to(dev)
    starts = torch.zeros(1, dtype=torch.int32, device=dev)
    paths, counts = ops.walk_paths(rowptr, col, starts, LAW_WALKS, 3, ops.walk_thresholds(*LAW_PQ), LAW_SEED)
    paths = paths.cpu().numpy()
    check_law(rowptr_h, col_h, paths, *LAW_PQ)
    want_paths, want_counts = wo.walk_paths(rowptr_h, col_h, [0], LAW_WALKS, 3, wo.thresholds(*LAW_PQ), LAW_SEED)
    assert np.array_equal(paths, want_paths) and np.array_equal(counts.cpu().numpy(), want_counts)


def test_unsupervised_train_driver_with_pq_walks(dev, tmp_path, capsys):
    from graphsage_amd import engine as eng
    from graphsage_amd import unsupervised_train as ut
    eng.reset_engine()
    old = ut.FLAGS
    try:
        ut.main(["--model", "n2v", "--synthetic", "small", "--learning_rate", "0.5", "--batch_size", "128", "--dim_1", "32",
                 "--walk_p", "0.5", "--walk_q", "2", "--walk_len", "4", "--num_walks", "10", "--max_walk_pairs", "20000",
                 "--max_total_steps", "12", "--print_every", "4", "--validate_iter", "100", "--n2v_test_epochs", "0",
                 "--base_log_dir", str(tmp_path)])
    finally:
        ut.FLAGS = old
    out = capsys.readouterr().out
    lines = re.findall(r"^Random walks: law= node2vec p= 0\.5 q= 2 len= 4 walks= 10 pairs= (\d+) time= \d+\.\d{5}$", out, re.M)
    assert len(lines) == 2 and 0 < int(lines[0]) <= 20000 and int(lines[1]) > 0  # the training walks, then n2v's retrain walks
    assert "Optimization Finished!" in out
    files = {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs}
    assert {"val.npy", "val.txt"} <= set(files)
    val = np.load(files["val.npy"])
    assert val.shape == (3000, 64) and np.isfinite(val).all()
