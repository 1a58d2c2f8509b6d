"""Full-neighborhood inference on a Reddit-shaped synthetic graph (N = 232,965 nodes, F = 602 features, mean degree ~492,
log-normal degrees: median ~300, hubs of thousands): the CSR reduce kernel (csrc/gs_csr_reduce.hip) and the layer-wise pass
built on it (graphsage_amd/inference.py), mean and maxpool models, dim 128.

    python benchmarks/bench_infer.py [--avg_degree 492] [--out profiles/full_inference.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o infer -- python benchmarks/bench_infer.py --hip_only

Prints one JSON line (and writes it to --out):
  * "reduce": per (op, width) the time of ONE reduce over every row of the graph (all row windows; HIP events on the engine
    stream around --reps passes, median of 5 regions) and the gathered bytes per second = nnz * round_up(d, 4) * 4 / time --
    to be read against the 5.5-5.8 TB/s of register gathers of whole rows from a table beyond the Infinity Cache.  Both on
    the SKEWED graph and on an EVENLY LOADED one with the same number of edges (every row the mean degree): their ratio is
    what the split rule (rows longer than 512 edges cut into separately reduced segments) has to keep near 1.
  * the same reduce restated in torch on the same device and graph, as a user without the kernel would write it: mean =
    torch.sparse CSR (values 1 / deg) @ dense; max = torch.segment_reduce over the gathered rows X[col], in row windows so
    that the gathered tensor stays under --torch_gather_gb (the [nnz, d] tensor itself would be tens of GB).  torch events,
    median of 5.  `hip_not_slower` records the comparison; a torch form that fails on this build is recorded as such.
  * "layers": wall time (host clock around calls that end in a device synchronise, table allocation included; best of 3 after a
    warm-up pass) of each aggregator's infer_full for the two-layer mean and maxpool models.
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

N_NODES, FEAT = 232965, 602


def synthetic_csr(n, avg_degree, skewed, seed, device):
    """(rowptr int64 [n + 1], col int32 [nnz]) on the device: log-normal degrees (sigma 1) scaled to the mean, or every row
    the mean degree; uniformly random neighbors."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    if skewed:
        w = torch.exp(torch.randn(n, device=device, generator=g, dtype=torch.float64))
        deg = torch.clamp((w * (avg_degree / float(w.mean()))).round(), 1, 21000).to(torch.int64)
    else:
        deg = torch.full((n,), int(avg_degree), dtype=torch.int64, device=device)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, n, (int(rowptr[-1]),), device=device, generator=g, dtype=torch.int32)
    return rowptr, col


def median_ms(fn, record, elapsed, regions=5):
    ms = []
    for _ in range(regions):
        a = record()
        fn()
        b = record()
        ms.append(elapsed(a, b))
    return float(np.median(ms)), float(np.min(ms))


def time_reduce(e, graph, op, X, reps):
    from graphsage_amd import inference as inf
    from graphsage_amd import ops
    out = e.ws_mat(("bench_out",), inf.WINDOW_ROWS, X.d)

    def one_pass():
        for r0, n in graph.windows(inf.WINDOW_ROWS):
            graph.reduce(e, op, X, out, r0, n)

    one_pass()
    e.sync()

    def region():
        for _ in range(reps):
            one_pass()

    def record():
        ev = ops.Event()
        ev.record(e.stream)
        return ev

    def elapsed(a, b):
        e.sync()
        return a.elapsed_ms(b) / reps

    return median_ms(region, record, elapsed)


def time_torch(fn, reps):
    fn()
    torch.cuda.synchronize()

    def region():
        for _ in range(reps):
            fn()

    def record():
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def elapsed(a, b):
        b.synchronize()
        return a.elapsed_time(b) / reps

    return median_ms(region, record, elapsed)


def torch_forms(graph, X, gather_gb):
    """(mean, max) restated in torch over the graph's device CSR and the logical [rows, d] view of X."""
    rowptr, col, _, _ = graph.on(X.buf.device)
    x = X.view().contiguous()
    deg = (rowptr[1:] - rowptr[:-1])
    col64 = col.to(torch.int64)
    vals = torch.repeat_interleave(1.0 / deg.clamp(min=1).to(torch.float32), deg)
    A = torch.sparse_csr_tensor(rowptr, col64, vals, size=(graph.n_rows, graph.n_rows))
    # row windows whose gathered rows stay under the budget
    budget = int(gather_gb * (1 << 30) / (4 * x.shape[1]))
    rp = rowptr.cpu().numpy()
    cuts, r = [0], 0
    while r < graph.n_rows:
        r2 = int(np.searchsorted(rp, rp[r] + budget, side="right")) - 1
        r = max(r + 1, min(r2, graph.n_rows))
        cuts.append(r)

    def mean():
        return A @ x

    def amax():
        outs = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            rows = x.index_select(0, col64[rp[a]:rp[b]])
            outs.append(torch.segment_reduce(rows, "max", offsets=rowptr[a:b + 1] - rowptr[a]))   # (from_csr leaves no empty row)
        return torch.cat(outs)

    return mean, amax


def bench_reduce(e, graphs, args):
    from graphsage_amd import inference as inf
    from graphsage_amd.ops import Mat
    res = {}
    g = torch.Generator(device=e.device)
    g.manual_seed(7)
    for op_name, op, d in (("mean", inf.CSR_MEAN, FEAT), ("mean", inf.CSR_MEAN, 128), ("max", inf.CSR_MAX, 512)):
        X = Mat.zeros(N_NODES + 1, d, e.device, ld_multiple=32)
        X.buf[:, :d].copy_(torch.randn(N_NODES + 1, d, device=e.device, generator=g))
        torch.cuda.synchronize()
        entry = {"d": d, "ld": X.ld}
        for tag, graph in graphs.items():
            med, best = time_reduce(e, graph, op, X, args.reps)
            gathered = graph.nnz * ((d + 3) // 4 * 4) * 4
            entry[tag] = {"ms": med, "ms_min": best, "gathered_TB_per_s": gathered / (med * 1e-3) / 1e12, "nnz": graph.nnz}
        entry["skewed_over_even_time_at_equal_bytes"] = (entry["skewed"]["ms"] / entry["skewed"]["nnz"]) / \
            (entry["even"]["ms"] / entry["even"]["nnz"])
        if not args.hip_only:
            try:
                mean, amax = torch_forms(graphs["skewed"], X, args.torch_gather_gb)
                med, best = time_torch(mean if op_name == "mean" else amax, max(1, args.reps // 2))
                entry["torch"] = {"ms": med, "ms_min": best,
                                  "form": "sparse_csr @ dense" if op_name == "mean" else "segment_reduce(X[col]) in row windows"}
                entry["hip_not_slower"] = bool(entry["skewed"]["ms"] <= med)
                entry["speedup_vs_torch"] = med / entry["skewed"]["ms"]
            except Exception as ex:             # recorded, not hidden: the torch form is the yardstick, not the product
                entry["torch"] = {"failed": "%s: %s" % (type(ex).__name__, str(ex)[:300])}
            torch.cuda.synchronize()
        res["%s_d%d" % (op_name, d)] = entry
        del X
        torch.cuda.empty_cache()
    return res


def bench_layers(graph, agg_type):
    from graphsage_amd import engine as eng
    from graphsage_amd import inits
    from graphsage_amd.models import Placeholder, SAGEInfo
    from graphsage_amd.neigh_samplers import AdjInfo, CSRAdjacency, UniformNeighborSampler
    from graphsage_amd.ops import Mat
    from graphsage_amd.supervised_models import SupervisedGraphsage
    eng.reset_engine()
    inits.set_seed(1)
    e = eng.get_engine()
    rowptr, col, _, _ = graph.on(e.device)
    g = torch.Generator(device=e.device)
    g.manual_seed(11)
    feats = Mat.zeros(N_NODES + 1, FEAT, e.device, ld_multiple=32)
    feats.buf[:N_NODES, :FEAT].copy_(torch.randn(N_NODES, FEAT, device=e.device, generator=g))
    torch.cuda.synchronize()
    ph = {'labels': Placeholder('labels'), 'batch': Placeholder('batch1'), 'dropout': Placeholder('dropout', 0.),
          'batch_size': Placeholder('batch_size')}
    adj_info = AdjInfo(CSRAdjacency.from_device(rowptr[:N_NODES + 1], col, N_NODES))
    sampler = UniformNeighborSampler(adj_info)
    layer_infos = [SAGEInfo("node", sampler, 25, 128), SAGEInfo("node", sampler, 10, 128)]
    model = SupervisedGraphsage(41, ph, feats, adj_info, np.ones(N_NODES, np.int64), layer_infos, aggregator_type=agg_type)
    out = {}
    for rep in range(4):                           # the first pass warms every shape
        H, times = model.features, []
        for agg in model.aggregators:
            e.sync()
            t0 = time.time()
            H = agg.infer_full(graph, H)
            times.append((time.time() - t0) * 1e3)
        if rep:
            for i, t in enumerate(times):
                out["layer%d_ms" % i] = min(out.get("layer%d_ms" % i, 1e30), t)
        del H
    t0 = time.time()
    emb, preds = model.predict_full(graph)
    out["predict_full_all_nodes_s"] = time.time() - t0
    out["embedding_shape"] = list(emb.shape)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--avg_degree", type=int, default=492)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--torch_gather_gb", type=float, default=4.0)
    ap.add_argument("--hip_only", action="store_true", help="skip the torch restatement (kernel-trace runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_infer.py needs the GPU"
    from graphsage_amd import engine as eng
    from graphsage_amd.inference import FullGraph
    eng.reset_engine()
    e = eng.get_engine()
    graphs = {}
    for tag, skewed in (("skewed", True), ("even", False)):
        rowptr, col = synthetic_csr(N_NODES, args.avg_degree, skewed, 123, e.device)
        graphs[tag] = FullGraph.from_csr(rowptr, col, N_NODES)
        del rowptr, col
    deg = np.diff(graphs["skewed"].rowptr.cpu().numpy())
    res = {"metric": "full-neighborhood inference, Reddit-shaped synthetic graph",
           "basis": "reduce: hipEventElapsedTime on the engine stream around %d passes over all rows, median of 5; torch: torch "
                    "events, median of 5; layers: host clock around synchronising calls, best of 3" % args.reps,
           "graph": {"n_nodes": N_NODES, "nnz": graphs["skewed"].nnz, "degree_median": float(np.median(deg)),
                     "degree_p99": float(np.percentile(deg, 99)), "degree_max": int(deg.max()),
                     "rows_cut": int(graphs["skewed"].splits.shape[0]), "split_len": graphs["skewed"].split_len,
                     "even_degree": args.avg_degree},
           "reduce": bench_reduce(e, graphs, args)}
    del graphs["even"]
    torch.cuda.empty_cache()
    res["layers"] = {agg: bench_layers(graphs["skewed"], agg) for agg in ("mean", "maxpool")}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
