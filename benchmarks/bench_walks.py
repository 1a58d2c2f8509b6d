"""Random-walk generation at the Reddit shape: 50 walks of 5 nodes from every train node of reddit_shaped_device's train view,
by the walk kernels (csrc/gs_walk.hip, through utils.device_walk_pairs) at (p, q) = (1, 1) and (0.5, 2), next to the eager
torch walker (utils.random_walk_pairs_device, uniform only) and the NumPy walker on the host (utils.run_random_walks, at a
subsample of the start nodes), all in one process.

    python benchmarks/bench_walks.py [--avg_degree 492] [--num_walks 50] [--walk_len 5] [--out profiles/random_walks.json]

Prints one JSON line (and writes it to --out).  Device work: torch events on the current stream around one call, median (min ..
max) of --regions regions after a warm-up call of the same shape (--reps calls per region for the paths launch alone).  Host
walker: a host clock, 3 runs.
  * "paths": gs_walk_paths alone over all walks (one launch per chunk of utils.WALK_CHUNK walks).
  * "pairs": device_walk_pairs end to end: paths, the prefix sum of the counts (torch.cumsum and one read-back of the total
    per chunk), gs_walk_pairs, the concatenation of the chunks.
  * "torch": random_walk_pairs_device end to end.
  * "host": run_random_walks on --host_nodes start nodes; steps per second from its own number of steps.
A step is one transition of one walk: n_walks * (walk_len - 1) per call.
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


def regions(fn, n_regions, reps=1):
    ms = []
    for _ in range(n_regions):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return {"ms": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_nodes", type=int, default=232965)
    ap.add_argument("--avg_degree", type=int, default=492)
    ap.add_argument("--num_walks", type=int, default=50)
    ap.add_argument("--walk_len", type=int, default=5)
    ap.add_argument("--pqs", default="1:1,0.5:2")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="calls per timed region of the paths launch alone")
    ap.add_argument("--host_nodes", type=int, default=4096)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_walks.py needs the GPU"
    from graphsage_amd import ops, utils
    dev = torch.device("cuda:0")
    G = utils.reddit_shaped_device(dev, n_nodes=args.n_nodes, avg_degree=args.avg_degree)
    rowptr, col = G.train_csr
    nodes = torch.from_numpy(np.asarray(G.train_nodes)).to(dev)
    starts = nodes.to(torch.int32).contiguous()
    n_walks = int(starts.numel()) * args.num_walks
    steps = n_walks * (args.walk_len - 1)
    deg = (rowptr[1:] - rowptr[:-1])[nodes.long()].double()
    res = {"metric": "random-walk generation, train view of the Reddit-shaped graph", "n_nodes": G.n_nodes,
           "train_nodes": int(starts.numel()), "nnz": int(col.numel()), "mean_degree_of_starts": float(deg.mean()),
           "max_degree_of_starts": int(deg.max()), "num_walks": args.num_walks, "walk_len": args.walk_len, "n_walks": n_walks,
           "steps": steps, "chunk_walks": utils.WALK_CHUNK,
           "basis": "torch events around one call, median / min / max of %d regions after a warm-up call; host: time.time(), "
                    "3 runs" % args.regions,
           "paths": {}, "pairs": {}}
    utils.check_rows_ascending(rowptr, col)                  # once per graph; not part of any timed region
    paths = torch.empty((min(n_walks, utils.WALK_CHUNK), args.walk_len), dtype=torch.int32, device=dev)
    counts = torch.empty(paths.shape[0], dtype=torch.int32, device=dev)
    for pq in args.pqs.split(","):
        p, q = (float(x) for x in pq.split(":"))
        thr = ops.walk_thresholds(p, q)

        def paths_call():
            for w0 in range(0, n_walks, utils.WALK_CHUNK):
                n = min(utils.WALK_CHUNK, n_walks - w0)
                ops.walk_paths(rowptr, col, starts, args.num_walks, args.walk_len, thr, 123, walk0=w0, n_walks=n, paths=paths[:n],
                               counts=counts[:n])

        def pairs_call():
            return utils.device_walk_pairs(rowptr, col, nodes, num_walks=args.num_walks, walk_len=args.walk_len, p=p, q=q, seed=123)

        paths_call()
        n_pairs = int(pairs_call().shape[0])
        torch.cuda.synchronize()
        r = regions(paths_call, args.regions, reps=args.reps)
        r["steps_per_s"] = steps / (r["ms"] * 1e-3)
        res["paths"][pq] = r
        r = regions(pairs_call, args.regions)
        r["steps_per_s"] = steps / (r["ms"] * 1e-3)
        r["n_pairs"] = n_pairs
        res["pairs"][pq] = r
    first = args.pqs.split(",")[0]
    for pq in args.pqs.split(",")[1:]:
        res["paths"][pq]["over_" + first] = res["paths"][pq]["ms"] / res["paths"][first]["ms"]
        res["pairs"][pq]["over_" + first] = res["pairs"][pq]["ms"] / res["pairs"][first]["ms"]

    def torch_call():
        return utils.random_walk_pairs_device(rowptr, col, nodes, num_walks=args.num_walks, walk_len=args.walk_len, seed=123)

    torch_pairs = int(torch_call().shape[0])
    torch.cuda.synchronize()
    # the torch walker also takes the step after the last recorded position (walk_len draws per walk)
    r = regions(torch_call, min(args.regions, 5))
    r["steps_per_s"] = steps / (r["ms"] * 1e-3)
    r["n_pairs"] = torch_pairs
    res["torch"] = r
    if "1:1" in res["pairs"]:
        res["torch"]["over_device_walk_pairs_1:1"] = r["ms"] / res["pairs"]["1:1"]["ms"]

    rp_h, col_h = rowptr.cpu().numpy(), col.cpu().numpy()
    sub = np.asarray(G.train_nodes)[:: max(1, len(G.train_nodes) // max(1, args.host_nodes))][:args.host_nodes]
    ts = []
    for _ in range(3):
        t0 = time.time()
        utils.run_random_walks(rp_h, col_h, sub, num_walks=args.num_walks, walk_len=args.walk_len)
        ts.append(time.time() - t0)
    host_steps = len(sub) * args.num_walks * (args.walk_len - 1)
    res["host"] = {"nodes": int(len(sub)), "steps": host_steps, "ms": float(np.median(ts)) * 1e3, "ms_min": float(np.min(ts)) * 1e3,
                   "ms_max": float(np.max(ts)) * 1e3, "steps_per_s": host_steps / float(np.median(ts))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
