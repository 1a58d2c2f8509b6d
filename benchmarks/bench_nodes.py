"""Receptive-field inference (embed_nodes) against the whole-graph pass (embed_full) on an RMAT graph generated in HBM
(utils.rmat_csr_device, the generator of bench.py --workload rmat; mean degree 20), supervised graphsage_mean, F = 256, dim 128.

    python benchmarks/bench_nodes.py [--nodes 10000000] [--edges 200000000] [--out profiles/embed_nodes.json]

Prints one JSON line (and writes it to --out):
  * "runs": per request size (random distinct nodes) the set sizes [|S_2|, |S_1|, |S_0|], the edges visited per layer, the time of
    embed_nodes, the time of the expansion alone (inference.receptive_field) and its share, the time of embed_full(graph, nodes)
    on the same model and graph, and their ratio.  Host clock around calls that end in a device synchronise (uploads, table
    allocation and the copy of the answer included), best of 3 after a warm-up call -- bench_infer.py's layer-table method.
  * "crossover": the closure fraction |S_0| / N between the last request size at which embed_nodes is faster and the first at
    which it is not (log-linear interpolation of the time ratio), or that no measured size crosses.
  * "reduce": gathered bytes per second (edges * 512 B / time, HIP events on the engine stream, median of 5 regions) of
    gs_csr_reduce_rows over the rows S_1 of the 4,096-node request -- with x_pos null and with an identity map -- and of
    gs_csr_reduce_fwd over every row of the graph, width 128.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FEAT, DIM, CLASSES = 256, 128, 64


def build(args):
    from graphsage_amd import engine as eng
    from graphsage_amd import inits
    from graphsage_amd.inference import FullGraph
    from graphsage_amd.models import Placeholder, SAGEInfo
    from graphsage_amd.neigh_samplers import AdjInfo, CSRAdjacency, UniformNeighborSampler
    from graphsage_amd.ops import Mat
    from graphsage_amd.supervised_models import SupervisedGraphsage
    from graphsage_amd.utils import rmat_csr_device
    eng.reset_engine()
    inits.set_seed(1)
    e = eng.get_engine()
    N = args.nodes
    rowptr, col = rmat_csr_device(N, args.edges, e.device, seed=123)
    g = torch.Generator(device=e.device)
    g.manual_seed(123)
    feats = Mat.zeros(N + 1, FEAT, e.device, ld_multiple=32)
    feats.buf[:N, :FEAT].uniform_(-1.0, 1.0, generator=g)
    torch.cuda.synchronize()
    ph = {'labels': Placeholder('labels'), 'batch': Placeholder('batch1'), 'dropout': Placeholder('dropout', 0.),
          'batch_size': Placeholder('batch_size')}
    adj_info = AdjInfo(CSRAdjacency.from_device(rowptr, col, N))
    sampler = UniformNeighborSampler(adj_info)
    layer_infos = [SAGEInfo("node", sampler, 15, DIM), SAGEInfo("node", sampler, 10, DIM)]
    model = SupervisedGraphsage(CLASSES, ph, feats, adj_info, None, layer_infos, concat=True, aggregator_type="mean")
    graph = FullGraph.from_csr(rowptr, col, N)
    return e, model, graph


def best_of(fn, reps=3):
    fn()                                   # warm-up: every shape's workspaces and uploads exist
    best, res = 1e30, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.time()
        res = fn()
        best = min(best, time.time() - t0)
    return best, res


def reduce_rates(e, graph, rows):
    """Gathered TB/s of the row-list reduce over `rows` (x_pos null / identity map) and of the window reduce over every row."""
    from graphsage_amd import inference as inf
    from graphsage_amd import ops
    from graphsage_amd.ops import Mat
    X = Mat.zeros(graph.n_rows, DIM, e.device, ld_multiple=32)
    X.buf[:, :DIM].normal_()
    ident = torch.arange(graph.n_rows, dtype=torch.int32, device=e.device)
    out_pos = torch.full((graph.n_rows,), -1, dtype=torch.int32, device=e.device)
    out_pos[torch.from_numpy(rows).to(e.device).long()] = torch.arange(rows.shape[0], dtype=torch.int32, device=e.device)
    out = Mat.zeros(rows.shape[0], DIM, e.device, ld_multiple=32)
    win = e.ws_mat(("bench_out",), inf.WINDOW_ROWS, DIM)
    plan = graph.upload_plan(e, rows)
    torch.cuda.synchronize()
    edges = int(np.diff(graph.rowptr_host)[rows].sum())

    def timed(fn, reps):
        fn()
        e.sync()
        ms = []
        for _ in range(5):
            a, b = ops.Event(), ops.Event()
            a.record(e.stream)
            for _ in range(reps):
                fn()
            b.record(e.stream)
            e.sync()
            ms.append(a.elapsed_ms(b) / reps)
        return float(np.median(ms))

    def window_pass():
        for r0, n in graph.windows(inf.WINDOW_ROWS):
            graph.reduce(e, inf.CSR_MEAN, X, win, r0, n)

    res = {"rows": int(rows.shape[0]), "edges": edges, "d": DIM}
    for tag, x_pos in (("rows_x_pos_null", None), ("rows_identity_map", ident)):
        ms = timed(lambda: graph.reduce_rows(e, inf.CSR_MEAN, X, out, rows, out_pos, x_pos=x_pos, plan=plan), 4)
        res[tag] = {"ms": ms, "gathered_TB_per_s": edges * DIM * 4 / (ms * 1e-3) / 1e12}
    ms = timed(window_pass, 1)
    res["window_all_rows"] = {"ms": ms, "edges": graph.nnz, "gathered_TB_per_s": graph.nnz * DIM * 4 / (ms * 1e-3) / 1e12}
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000000)
    ap.add_argument("--edges", type=int, default=200000000)
    ap.add_argument("--requests", default="1,64,4096,262144")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_nodes.py needs the GPU"
    from graphsage_amd import inference as inf
    t0 = time.time()
    e, model, graph = build(args)
    N = graph.n_nodes
    deg = np.diff(graph.rowptr_host)
    res = {"metric": "receptive-field inference (embed_nodes) vs the whole-graph pass (embed_full), RMAT graph in HBM",
           "basis": "host clock around synchronising calls, best of 3 after a warm-up call; reduce: hipEventElapsedTime, median of 5",
           "graph": {"n_nodes": N, "edges": graph.nnz, "degree_max": int(deg.max()), "degree_p99": float(np.percentile(deg, 99)),
                     "rows_cut": int(graph.splits.shape[0]), "setup_s": time.time() - t0},
           "model": "supervised graphsage_mean, F=%d, dim %d, concat, 2 layers" % (FEAT, DIM), "runs": []}
    sys.stderr.write("graph ready: %s\n" % json.dumps(res["graph"]))
    rng = np.random.RandomState(7)
    s1_rows = None
    for n_req in [int(x) for x in args.requests.split(",")]:
        nodes = rng.choice(N, size=min(n_req, N), replace=False)
        t_nodes, (emb, stats) = best_of(lambda: model.embed_nodes(graph, nodes))
        t_rf, sets = best_of(lambda: inf.receptive_field(e, graph, nodes, 2)[0])
        t_full, full = best_of(lambda: model.embed_full(graph, nodes=nodes))
        run = {"nodes": int(nodes.shape[0]), "rows": stats["rows"], "edges": stats["edges"], "closure_fraction": stats["rows"][-1] / N,
               "embed_nodes_ms": t_nodes * 1e3, "expansion_ms": t_rf * 1e3, "expansion_share": t_rf / t_nodes,
               "embed_full_ms": t_full * 1e3, "speedup": t_full / t_nodes,
               "max_abs_diff_vs_embed_full": float(np.abs(emb - full).max())}
        res["runs"].append(run)
        sys.stderr.write(json.dumps(run) + "\n")
        if n_req == 4096:
            s1_rows = sets[1]
        del emb, full
    runs = res["runs"]
    cross = None
    for a, b in zip(runs[:-1], runs[1:]):
        if a["speedup"] > 1.0 >= b["speedup"]:
            w = np.log(a["speedup"]) / (np.log(a["speedup"]) - np.log(b["speedup"]))
            cross = float(np.exp(np.log(a["closure_fraction"]) + w * (np.log(b["closure_fraction"]) - np.log(a["closure_fraction"]))))
    res["crossover"] = {"closure_fraction": cross,
                        "note": "log-linear interpolation between the two bracketing request sizes" if cross is not None else
                        ("embed_nodes is faster at every measured size" if runs[-1]["speedup"] > 1.0 else
                         "embed_nodes is not faster at the smallest measured size")}
    if s1_rows is not None:
        res["reduce"] = reduce_rates(e, graph, np.ascontiguousarray(s1_rows, dtype=np.int64))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
