"""-m gpu: gs_importance_table against the NumPy restatement of importance_oracle.py, bit for bit, on crafted paths at every edge
the kernel has (the wave width, the sort sizes, both ends of every limit); utils.importance_neighbors against the oracle on
walk_oracle's paths under every chunking; the table as the sampler's adjacency and as the exact-inference graph; the two drivers
with --importance_neighbors.

The kernel has ONE form for every V = num_walks * (walk_len - 1) from 1 to 4096 (no switch point): what changes with V is the
power of two its first sort runs over (64 up to V = 64, then the power of two at or above V), so V sits on both sides of 64, 128
and 1024 and at the two ends."""
import os
import re

import numpy as np
import pytest
import torch

import importance_oracle as io
from test_importance import SEED, graph200, oracle_run

pytestmark = pytest.mark.gpu

N_NODES = 10000
PAD = N_NODES
# V -> (num_walks, walk_len, n_starts): every V the issue lists, every n_starts it lists among them
SHAPES = {1: (1, 2, 1), 2: (1, 3, 3), 63: (21, 4, 4), 64: (64, 2, 5), 65: (13, 6, 257), 127: (127, 2, 3), 128: (64, 3, 4),
          129: (43, 4, 5), 1023: (341, 4, 3), 1024: (512, 3, 4), 1025: (205, 6, 3), 4096: (1024, 5, 5)}


def random_paths(V, seed, extra_cols=0):
    """Visits from a pool whose size differs from start to start (1 node up to more than V), a tenth of them the pad id, -1 or an
    id past the graph; the second start (where there is one) a row of -1, as the walker writes for a start that is no node."""
    num_walks, walk_len, n_starts = SHAPES[V]
    rng = np.random.RandomState(seed)
    paths = np.empty((n_starts * num_walks, walk_len + extra_cols), dtype=np.int32)
    for i in range(n_starts):
        pool = rng.choice(N_NODES, size=int(rng.choice([1, 2, 5, 40, V, 2 * V + 3])), replace=False)
        blk = pool[rng.randint(0, len(pool), size=(num_walks, walk_len + extra_cols))]
        junk = rng.rand(*blk.shape)
        blk = np.where(junk < 0.03, PAD, np.where(junk < 0.06, -1, np.where(junk < 0.1, N_NODES + 5, blk)))
        blk[:, 0] = pool[0]
        paths[i * num_walks:(i + 1) * num_walks] = blk
    if n_starts > 1:
        paths[num_walks:2 * num_walks] = -1
    return paths, num_walks, walk_len


def on_device(dev, paths, num_walks, walk_len, n_nodes, top, slots, pad_id):
    from graphsage_amd import ops
    buf = torch.from_numpy(np.ascontiguousarray(paths)).to(dev)
    table, stats = ops.importance_table(buf, num_walks, walk_len, n_nodes, top, slots, pad_id)
    torch.cuda.synchronize()
    return table.cpu().numpy(), stats.cpu().numpy()


def check(dev, paths, num_walks, walk_len, n_nodes, top, slots, pad_id):
    want = io.importance_rows(paths, num_walks, walk_len, n_nodes, top, slots, pad_id)
    got = on_device(dev, paths, num_walks, walk_len, n_nodes, top, slots, pad_id)
    bad = np.nonzero(np.any(got[0] != want[0], axis=1) | np.any(got[1] != want[1], axis=1))[0]
    assert bad.size == 0, "start %d: got %s %s, want %s %s" % (bad[0], got[0][bad[0]], got[1][bad[0]], want[0][bad[0]], want[1][bad[0]])
    return got


@pytest.mark.parametrize("V", sorted(SHAPES))
def test_table_equals_the_oracle_at_every_size(dev, V):
    paths, num_walks, walk_len = random_paths(V, 100 + V)
    assert num_walks * (walk_len - 1) == V
    first = check(dev, paths, num_walks, walk_len, N_NODES, 8, 16, PAD)
    again = on_device(dev, paths, num_walks, walk_len, N_NODES, 8, 16, PAD)           # two launches give equal bits
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    check(dev, paths, num_walks, walk_len, N_NODES, 4096, 1024, PAD)                  # top > m, the widest row
    check(dev, paths, num_walks, walk_len, N_NODES, 1, 1, PAD)                        # the narrowest of both
    check(dev, paths, num_walks, walk_len, N_NODES, 50, 7, -7)                        # fewer slots than selected nodes; another pad id


@pytest.mark.parametrize("V", [65, 1025])
def test_rows_wider_than_the_walks(dev, V):
    """ld_paths > walk_len: the columns past walk_len hold ids that would change every row if they were read."""
    paths, num_walks, walk_len = random_paths(V, 7, extra_cols=3)
    assert paths.shape[1] == walk_len + 3
    check(dev, paths, num_walks, walk_len, N_NODES, 8, 16, PAD)


def test_more_starts_than_workgroups(dev):
    """The grid holds at most 65,536 one-wave workgroups; the starts beyond that are reached by grid stride."""
    rng = np.random.RandomState(3)
    n_starts = 65536 + 67
    paths = rng.randint(-1, 12, size=(2 * n_starts, 3)).astype(np.int32)
    got, stats = check(dev, paths, 2, 3, 10, 2, 4, 10)
    assert got.shape == (n_starts, 4) and np.any(stats[65536:, 0] > 0) and np.any(got[65536:] != 10)


def crafted():
    """name -> (paths, num_walks, walk_len, n_nodes, top, slots)"""
    A = lambda rows: np.asarray(rows, dtype=np.int32)
    every = np.arange(1, 4097, dtype=np.int32).reshape(1024, 4)
    return {
        "all visits the start": (A([[4, 4, 4]] * 50), 50, 3, 9, 3, 8),
        "all visits one node": (A([[4, 6, 6]] * 50), 50, 3, 9, 3, 8),
        "one node, slots 1024": (A([[4, 6, 6]] * 50), 50, 3, 9, 5, 1024),
        "4096 distinct": (np.concatenate([np.zeros((1024, 1), np.int32), every], axis=1), 1024, 5, 5000, 4096, 1024),
        "4096 distinct, top 100, slots 33": (np.concatenate([np.zeros((1024, 1), np.int32), every], axis=1), 1024, 5, 5000, 100, 33),
        "4096 distinct, descending": (np.concatenate([np.zeros((1024, 1), np.int32), every[::-1, ::-1]], axis=1), 1024, 5, 5000, 4096, 1000),
        "no visit kept": (A([[0, 9, -1, 14], [0, 0, 9, 9]]), 2, 4, 9, 3, 8),
        "a start of -1": (A([[-1, -1, -1]] * 3 + [[2, 1, 3]] * 3), 3, 3, 9, 3, 8),
        "a start past the graph": (A([[9, 1, 2]] * 2 + [[14, 1, 2]] * 2), 2, 3, 9, 3, 8),
        "count ties across top": (A([[0, 1, 1], [0, 2, 2], [0, 3, 3], [0, 4, 4]]), 4, 3, 9, 2, 8),
        "count ties across top, ids descending": (A([[0, 8, 8], [0, 6, 6], [0, 3, 3], [0, 1, 1]]), 4, 3, 9, 3, 8),
        "top 1": (A([[0, 1, 2], [0, 2, 3]]), 2, 3, 9, 1, 8),
        "top above m": (A([[0, 1, 2], [0, 2, 3]]), 2, 3, 9, 4096, 8),
        "slots 1": (A([[0, 1, 2], [0, 2, 3]]), 2, 3, 9, 3, 1),
        "fewer slots than selected": (A([[0, 1, 2, 3, 4, 5, 6, 7, 8]]), 1, 9, 9, 8, 3),
        "remainder ties": (A([[0, 1, 2, 3]]), 1, 4, 9, 3, 4),
        "remainder ties, two rests": (A([[0, 1, 2, 3, 4, 5]]), 1, 6, 9, 5, 7),
        "exact shares": (A([[0, 1, 1], [0, 1, 2], [0, 2, 3]]), 3, 3, 9, 3, 6),
        "the largest id": (A([[0, 2 ** 31 - 2, 2 ** 31 - 2], [0, 5, 2 ** 31 - 1]]), 2, 3, 2 ** 31 - 1, 3, 4),
    }


CRAFTED = crafted()


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_rows(dev, name):
    paths, num_walks, walk_len, n_nodes, top, slots = CRAFTED[name]
    got, stats = check(dev, paths, num_walks, walk_len, n_nodes, top, slots, n_nodes)
    if name == "count ties across top":
        assert got.tolist() == [[1] * 4 + [2] * 4] and stats.tolist() == [[4, 2]]
    if name == "remainder ties":                                     # q = 1 each, r = 1 each, one slot left: the lowest id
        assert got.tolist() == [[1, 1, 2, 3]]
    if name == "all visits the start" or name == "no visit kept":
        assert np.all(got == n_nodes) and np.all(stats == 0)
    if name == "a start of -1":
        assert np.all(got[0] == n_nodes) and got[1].tolist() == [1, 1, 1, 1, 3, 3, 3, 3]


def test_limit_violations_launch_nothing(dev):
    from graphsage_amd import ops
    from graphsage_amd._lib import GraphsageAmdError

    def refused(word, num_walks=2, walk_len=3, top=3, slots=8, n_nodes=9, cols=None, n_starts=2):
        paths = torch.ones((n_starts * max(num_walks, 1), walk_len if cols is None else cols), dtype=torch.int32, device=dev)
        table = torch.full((n_starts, slots), 77, dtype=torch.int32, device=dev)
        stats = torch.full((n_starts, 2), 77, dtype=torch.int32, device=dev)
        with pytest.raises(GraphsageAmdError, match=word):
            ops.importance_table(paths, num_walks, walk_len, n_nodes, top, slots, n_nodes, table=table, stats=stats)
        torch.cuda.synchronize()
        assert bool((table == 77).all()) and bool((stats == 77).all())

    refused("walk_len", walk_len=1)
    refused("visits", num_walks=2049)
    refused("visits", num_walks=1, walk_len=4098)
    refused("top", top=0)
    refused("top", top=4097)
    refused("slots", slots=1025)
    refused("ld_paths", cols=2)
    refused("ld_paths", cols=2, n_starts=1, num_walks=1)
    refused("n_nodes", n_nodes=2 ** 31)
    with pytest.raises(GraphsageAmdError, match="num_walks"):
        ops.importance_table(torch.ones((4, 3), dtype=torch.int32, device=dev), 0, 3, 9, 3, 8, 9)
    with pytest.raises(GraphsageAmdError, match="slots"):
        ops.importance_table(torch.ones((4, 3), dtype=torch.int32, device=dev), 2, 3, 9, 3, 0, 9)
    with pytest.raises(GraphsageAmdError, match="device of paths"):                  # outputs that live elsewhere than the paths
        ops.importance_table(torch.ones((4, 3), dtype=torch.int32, device=dev), 2, 3, 9, 3, 8, 9, table=torch.zeros((2, 8), dtype=torch.int32))
    with pytest.raises(GraphsageAmdError, match="device of paths"):
        ops.importance_table(torch.ones((4, 3), dtype=torch.int32, device=dev), 2, 3, 9, 3, 8, 9, stats=torch.zeros((2, 2), dtype=torch.int32))
    table, stats = ops.importance_table(torch.ones((0, 3), dtype=torch.int32, device=dev), 2, 3, 9, 3, 8, 9)      # no start: a no-op
    assert table.shape == (0, 8) and stats.shape == (0, 2)


# ------------------------------------------------------------------------------------------------ walks -> table
def graph200_device(dev):
    rowptr, col = graph200()
    return torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev)


@pytest.mark.parametrize("pq", [(1.0, 1.0), (0.5, 2.0)])
def test_importance_neighbors_equals_the_oracle_under_every_chunking(dev, pq):
    from graphsage_amd import utils
    paths, n = oracle_run("graph200", pq)
    want_table, want_stats = io.importance_rows(paths, 10, 3, n, 8, 16, n)
    rowptr, col = graph200_device(dev)
    for chunk in (1, 7, None):
        table, stats = utils.importance_neighbors(rowptr, col, n, 8, 16, num_walks=10, walk_len=3, p=pq[0], q=pq[1], seed=SEED,
                                                  chunk_starts=chunk)
        assert table.shape == (n + 1, 16) and table.dtype == torch.int32 and table.device.type == "cuda"
        assert np.array_equal(table.cpu().numpy()[:n], want_table), chunk
        assert np.all(table.cpu().numpy()[n] == n) and np.array_equal(stats.cpu().numpy(), want_stats)
    assert np.all(want_table[190:] == n) and np.any(want_table[:190] != n)             # degree-0 starts are kept, as pad rows


def test_the_sampler_draws_each_row_as_it_stands(dev):
    """law reference on the CSR made from the table, num_samples == max_degree == slots: the multiset of each row."""
    from graphsage_amd import engine as eng
    from graphsage_amd import utils
    from graphsage_amd.neigh_samplers import AdjInfo, CSRAdjacency, UniformNeighborSampler
    rowptr, col = graph200_device(dev)
    table, _ = utils.importance_neighbors(rowptr, col, 200, 8, 16, num_walks=10, walk_len=3, seed=SEED)
    eng.reset_engine()
    e = eng.get_engine()
    sampler = UniformNeighborSampler(AdjInfo(CSRAdjacency.from_table(table)), seed=123, law="reference", max_degree=16)
    ids = torch.arange(201, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sampler.new_step()
    got = sampler((ids, 16))
    e.sync()
    got, want = got.cpu().numpy(), table.cpu().numpy()
    assert np.array_equal(np.sort(got, axis=1), want)                # rows ascending; the pad row and the empty rows all pad
    assert not np.array_equal(got, want)


def test_embed_full_over_the_table_equals_the_oracle(dev):
    """Mean aggregator, trained weights: exact inference over the table's multigraph -- an id stored n times weighs n / slots."""
    from graphsage_amd import utils
    from graphsage_amd.inference import FullGraph
    from ref_fixtures import Fixture
    from test_ref_pin_gpu import build_supervised, load_weights
    import fullnbr_oracle as fo
    fx = Fixture("sup_mean_full_degree")
    e, ph, adj_info, sampler, model = build_supervised(fx)
    prefix = "s0/32/after/" if fx.has("s0/32/after/node_pred/bias") else "init/"
    load_weights(model, fx, prefix)
    rp, col, N = fx["graph/full_rowptr"], fx["graph/full_col"], fx.n_nodes
    table, stats = utils.importance_neighbors(torch.from_numpy(rp.astype(np.int64)).to(dev), torch.from_numpy(col.astype(np.int32)).to(dev),
                                              N, 5, 12, num_walks=10, walk_len=3, seed=SEED)
    host = table.cpu().numpy()
    assert np.any(np.diff(host[:N], axis=1) == 0) and np.any(stats.cpu().numpy()[:, 0] == 0)     # repeats, and an empty row
    emb = model.embed_full(FullGraph.from_padded(table))
    want = fo.forward(fo.padded_lists(host), fx["graph/feats"].astype(np.float64), fx.params(prefix, np.float64), fx.agg,
                      fx.cfg["concat"])[:N]
    assert emb.shape == want.shape
    np.testing.assert_allclose(emb, want, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ drivers
# the issue's command; --samples_1 / --samples_2 are added because the defaults (25, 10) exceed --max_degree 16, which the sampler
# refuses under every adjacency, and the small batch and widths keep the run short
ON = ["--synthetic", "small", "--importance_neighbors", "8", "--max_degree", "16", "--importance_walks", "10", "--epochs", "1",
      "--max_total_steps", "5"]
SMALL = ["--samples_1", "5", "--samples_2", "3", "--batch_size", "128", "--dim_1", "32", "--dim_2", "32", "--validate_iter", "10"]
LINE = (r"Importance neighborhoods: graph= %s top= 8 slots= 16 walks= 10 len= 3 p= 1 q= 1 rows= 3000 distinct_mean= \d+\.\d{5} "
        r"kept_mean= \d+\.\d{5} empty= \d+ time= \d+\.\d{5}")


def files_under(path):
    return {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(path)) for f in fs}


@pytest.mark.parametrize("extra", [[], ["--sampler", "padded"]])
def test_supervised_driver(dev, tmp_path, capsys, extra):
    from graphsage_amd import engine as eng
    from graphsage_amd import supervised_train as st
    eng.reset_engine()
    st.main(ON + SMALL + ["--print_every", "1", "--full_inference", "--base_log_dir", str(tmp_path)] + extra)
    out = capsys.readouterr().out
    assert re.search(LINE % "train", out) and re.search(LINE % "test", out)
    assert out.index("graph= train") < out.index("graph= test") < out.index("Epoch: 0001")
    losses = [float(x) for x in re.findall(r"train_loss= (\S+)", out)]
    assert len(losses) >= 5 and np.all(np.isfinite(losses))
    assert re.search(r"Full-neighborhood validation stats: f1_micro= \d\.\d{5} f1_macro= \d\.\d{5}", out)
    files = files_under(tmp_path)
    assert re.match(r"f1_micro=\d\.\d{5} f1_macro=\d\.\d{5} time=\d+\.\d{5}$", open(files["val_stats_full.txt"]).read())
    assert re.match(r"f1_micro=\d\.\d{5} f1_macro=\d\.\d{5}$", open(files["test_stats_full.txt"]).read())


def test_supervised_driver_seq_trains_normally(dev, tmp_path, capsys):
    """graphsage_seq has no full-neighborhood form, but it samples like every other model: it trains over the importance tables."""
    from graphsage_amd import engine as eng
    from graphsage_amd import supervised_train as st
    eng.reset_engine()
    st.main(ON + SMALL + ["--model", "graphsage_seq", "--print_every", "1", "--base_log_dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert re.search(LINE % "train", out) and re.search(LINE % "test", out)
    losses = [float(x) for x in re.findall(r"train_loss= (\S+)", out)]
    assert len(losses) >= 5 and np.all(np.isfinite(losses))
    assert re.search(r"Full validation stats: loss= \d+\.\d{5} f1_micro= \d\.\d{5}", out)


def test_unsupervised_driver(dev, tmp_path, capsys, monkeypatch):
    """The supervised command (--full_inference included) with --eval_classifier val: val_full.npy is exact inference over the
    importance table of the test graph, and the classifier line comes from that file."""
    from graphsage_amd import engine as eng
    from graphsage_amd import evaluation
    from graphsage_amd import unsupervised_train as ut
    from graphsage_amd.inference import FullGraph
    kept = {}
    real_save, real_eval = ut.save_full_embeddings, evaluation.evaluate_embedding_dir

    def spy_save(model, minibatch, out_dir):
        real_save(model, minibatch, out_dir)
        kept["table"] = minibatch.importance_test.cpu().numpy()
        kept["direct"] = model.embed_full(FullGraph.from_padded(minibatch.importance_test))
        kept["true_deg"] = np.diff(minibatch.test_csr[0])

    def spy_eval(*args, **kw):
        kept["base"] = kw.get("base")
        return real_eval(*args, **kw)

    monkeypatch.setattr(ut, "save_full_embeddings", spy_save)
    monkeypatch.setattr(evaluation, "evaluate_embedding_dir", spy_eval)
    eng.reset_engine()
    ut.main(ON + SMALL + ["--model", "graphsage_mean", "--learning_rate", "0.001", "--max_walk_pairs", "4000", "--print_every", "1",
                          "--validate_batch_size", "256", "--full_inference", "--eval_classifier", "val",
                          "--base_log_dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert re.search(LINE % "train", out) and re.search(LINE % "test", out)
    losses = [float(x) for x in re.findall(r"train_loss= (\S+)", out)]
    assert len(losses) >= 5 and np.all(np.isfinite(losses))
    files = files_under(tmp_path)
    assert "val.npy" in files and np.all(np.isfinite(np.load(files["val.npy"])))
    # the exact embeddings: over the importance table (16 slots a row, repeats and all), not over the adjacency rows
    emb = np.load(files["val_full.npy"])
    assert emb.shape == (3000, 64) and emb.dtype == np.float32 and np.all(np.isfinite(emb))
    assert kept["table"].shape == (3001, 16) and np.any(np.diff(kept["table"][:3000], axis=1) == 0)
    assert np.any(kept["true_deg"] != 16)
    assert np.array_equal(emb, kept["direct"])
    assert open(files["val_full.txt"]).read().split("\n") == [str(i) for i in range(3000)]
    # ... and the classifier was fitted on that file
    assert kept["base"] == "val_full"
    found = re.findall(r"^Downstream classifier: .*$", out, flags=re.M)
    assert len(found) == 1 and open(files["eval_classifier.txt"]).read() == found[0] + "\n"


def test_the_flag_at_zero_changes_nothing(dev, tmp_path):
    """--importance_neighbors 0 prints what a run without the flag prints, bit for bit (the time= fields, wall clocks, aside) and
    writes the same stats.  The two runs are two child processes, one after the other: a second main() in one process is no rerun
    (the layer-name counters and NumPy's global generator carry over).  subprocess.run kills a child that outlives its limit."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    args = ["--synthetic", "small", "--epochs", "1", "--max_total_steps", "5", "--max_degree", "16", "--print_every", "1"] + SMALL
    outs, stats = {}, {}
    for tag, extra in (("off", []), ("zero", ["--importance_neighbors", "0"])):
        proc = subprocess.run([sys.executable, "-m", "graphsage_amd.supervised_train"] + args + extra
                              + ["--base_log_dir", str(tmp_path / tag)], cwd=root, env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-2000:]
        out = proc.stdout
        assert "Importance neighborhoods" not in out and len(re.findall(r"train_loss= \d", out)) >= 5
        outs[tag] = re.sub(r"time= \S+", "time=", out)
        stats[tag] = re.sub(r"time=\S+", "time=", open(files_under(tmp_path / tag)["val_stats.txt"]).read())
    assert outs["off"] == outs["zero"] and stats["off"] == stats["zero"] and "f1_micro=" in stats["off"]
