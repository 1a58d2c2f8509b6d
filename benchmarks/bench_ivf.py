"""Approximate top-k retrieval through an inverted file (csrc/gs_ivf.hip, through ops.ivf_search) next to the exhaustive kernel
(ops.topk_select) on the same queries and table, in one process, the two alternating.

    python benchmarks/bench_ivf.py [--q 65536] [--n 232965] [--d 256] [--k 10] [--clusters 0,1024,4096] [--nprobes 1,4,16,64]
                                   [--components 1024] [--sigma 0.05] [--out profiles/topk_ivf_reddit.json]

Rows: an l2-normalised Gaussian MIXTURE generated on the device from a seed -- --components unit-norm means, every row a mean
plus --sigma * N(0, I), normalised (pure Gaussian rows have no cluster structure; recall would mean nothing).  Queries: the
rows of --q random nodes, the node itself no candidate.  Filter: the 492-per-row random CSR of bench_topk.py; with
--sparse_filter only the rows that a query names carry entries (the same work for the kernels, which read no other row; at
N = 10^7 the full CSR would take 20 GB and most of the run to generate).

Index: k-means from --kmeans_iters Lloyd iterations at most, started from C random rows (NOT k-means++: its host-side seeding
walks C times over a 32 C-row subsample in fp64, minutes at C = 4096).  Build time is the fit plus the grouping.

Protocol of bench_topk.py: HIP events on the engine stream, median (min .. max) of 5 regions of --reps calls after a warm-up
call; between two IVF regions the exhaustive kernel runs on the same queries (on the first --alternate_queries of them where
one full call takes seconds; the ratio then uses the full call's own median).  Per setting the search is also timed cut short
after its probe, plan and scan steps (gs_ivf_desc.stop_after; 3 regions of one call): probe = t1, group + plan = t3 - t1,
scan = t4 - t3, merge = total - t4.  recall@k: retrieval.recall against ops.topk_select on the first --recall_queries queries.
Prints one JSON line (and writes it to --out).
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

from benchmarks.bench_rank import random_filter, regions  # noqa: E402


def mixture(N, d, components, sigma, dev, seed, rows_per_pass=1 << 20):
    """Mat [N + 1, d]: rows 0 .. N-1 the mixture, row N the zero pad row."""
    from graphsage_amd import ops
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    means = torch.nn.functional.normalize(torch.randn(components, d, device=dev, generator=g), dim=1)
    Z = ops.Mat.zeros(N + 1, d, dev)
    for r0 in range(0, N, rows_per_pass):
        r1 = min(N, r0 + rows_per_pass)
        comp = torch.randint(0, components, (r1 - r0,), device=dev, generator=g)
        x = means[comp] + sigma * torch.randn(r1 - r0, d, device=dev, generator=g)
        Z.buf[r0:r1, :d].copy_(torch.nn.functional.normalize(x, dim=1))
    return Z


def sparse_filter(n_rows, src, avg_degree, seed, dev):
    """random_filter's rows for the nodes in `src` only; every other row is empty."""
    nodes = torch.unique(src.to(torch.int64))
    rp, col = random_filter(int(nodes.numel()), avg_degree, seed, dev)        # ids in [0, len(nodes)): spread them over the table
    scale = max(1, (n_rows - 1) // max(int(nodes.numel()), 1))
    deg = torch.zeros(n_rows, dtype=torch.int64, device=dev)
    deg[nodes] = rp[1:] - rp[:-1]
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(deg, 0)
    return rowptr, (col.to(torch.int64) * scale).to(torch.int32)              # ascending rows stay ascending


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, default=65536)
    ap.add_argument("--n", type=int, default=232965)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--clusters", default="0,1024,4096")
    ap.add_argument("--nprobes", default="1,4,16,64")
    ap.add_argument("--components", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--avg_degree", type=int, default=492)
    ap.add_argument("--sparse_filter", action="store_true")
    ap.add_argument("--kmeans_iters", type=int, default=10)
    ap.add_argument("--recall_queries", type=int, default=4096)
    ap.add_argument("--alternate_queries", type=int, default=0,
                    help="queries of the exhaustive call between two IVF regions (0: all; fewer where one such call takes seconds)")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_ivf.py needs the GPU"
    from graphsage_amd import engine as eng
    from graphsage_amd import ops, retrieval
    eng.reset_engine()
    e = eng.get_engine()
    dev = e.device
    Q, N, d, k = args.q, args.n, args.d, args.k
    Z = mixture(N, d, args.components, args.sigma, dev, 3)
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    src = torch.randint(0, N, (Q,), device=dev, generator=g, dtype=torch.int32)
    f_rowptr, f_col = (sparse_filter(N + 1, src, args.avg_degree, 5, dev) if args.sparse_filter
                       else random_filter(N + 1, args.avg_degree, 5, dev))
    Xq = ops.Mat.zeros(Q, d, dev)
    ids = torch.zeros((Q, k), dtype=torch.int32, device=dev)
    scores = torch.zeros((Q, k), dtype=torch.float32, device=dev)
    count = torch.zeros(Q, dtype=torch.int32, device=dev)
    scanned = torch.zeros(Q, dtype=torch.int64, device=dev)
    chunk = min(Q, ops.RANK_CHUNK)
    topk_ws = torch.zeros(ops.topk_ws_bytes(chunk, N, k) // 8 + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ops.gather_rows(Z, src, out=Xq, stream=e.stream)
    e.sync()

    def record():
        ev = ops.Event()
        ev.record(e.stream)
        return ev

    def elapsed(a, b):
        e.sync()
        return a.elapsed_ms(b)

    filters = (("unfiltered", (None, None)), ("filtered", (f_rowptr, f_col)))
    Rq = min(Q, args.recall_queries)
    Aq = min(Q, args.alternate_queries) if args.alternate_queries > 0 else Q

    def exact_call(filt, n=Q):
        ops.topk_select(ops.Mat(Xq.buf[:n], d), Z, k, n_cand=N, src=src[:n], f_rowptr=filt[0], f_col=filt[1], ids=ids[:n],
                        scores=scores[:n], count=count[:n], ws=topk_ws, stream=e.stream)

    res = {"metric": "approximate top-k retrieval through an inverted file, next to the exhaustive kernel", "Q": Q, "n_cand": N,
           "d": d, "k": k, "rows": {"law": "l2-normalised Gaussian mixture", "components": args.components, "sigma": args.sigma},
           "filter": {"avg_degree_of_query_rows": float(f_col.numel()) / float(torch.unique(src).numel() if args.sparse_filter
                                                                                else N + 1),
                      "nnz": int(f_col.numel()), "rows_with_entries": "query nodes only" if args.sparse_filter else "all"},
           "basis": "hipEventElapsedTime on the engine stream around %d call(s), median / min / max of 5 regions after a warm-up "
                    "call, exact and IVF alternating; steps: 3 regions of one call cut short by stop_after" % args.reps,
           "recall_queries": Rq, "kmeans": {"init": "random rows", "max_iter": args.kmeans_iters}, "exact": {}, "index": {},
           "ivf": {}}
    exact_ids = {}
    for tag, filt in filters:
        exact_call(filt)
        e.sync()
        exact_ids[tag] = ids[:Rq].cpu().numpy().copy()
        res["exact"][tag] = regions(lambda: exact_call(filt), record, elapsed, args.reps)

    rs = np.random.RandomState(7)
    for C in sorted({retrieval.default_clusters(N) if int(c) == 0 else int(c) for c in args.clusters.split(",")}):
        t0 = time.time()
        init = Z.buf[torch.from_numpy(np.sort(rs.choice(N, size=C, replace=False))).to(dev), :d].cpu().numpy()
        index = retrieval.build_ivf(e, Z, C, n_cand=N, init=init, max_iter=args.kmeans_iters)
        build_s = time.time() - t0
        C2 = index.n_clusters
        res["index"][str(C)] = {"clusters": C2, "empty": index.empty, "build_s": build_s, "kmeans_iters": index.clustering.iters,
                                "kmeans_stop": index.clustering.stop, "list_min": int(index.sizes.min()),
                                "list_max": int(index.sizes.max()), "list_mean": float(index.sizes.mean()),
                                "list_max_over_mean": float(index.sizes.max() / index.sizes.mean())}
        res["ivf"][str(C)] = {}
        for P in [int(p) for p in args.nprobes.split(",")]:
            if P > C2:
                continue
            ws = torch.zeros(ops.ivf_ws_bytes(chunk, C2, k, P) // 8 + 2, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            res["ivf"][str(C)][str(P)] = {"workspace_bytes": ops.ivf_ws_bytes(chunk, C2, k, P)}
            for tag, filt in filters:
                def ivf_call(stop_after=0):
                    ops.ivf_search(Xq, Z, index.centers_dev, index.list_ptr, index.list_ids, k, P, n_cand=N, src=src, f_rowptr=filt[0],
                                   f_col=filt[1], ids=ids, scores=scores, count=count, scanned=scanned, ws=ws, stop_after=stop_after,
                                   stream=e.stream)
                ivf_call()
                e.sync()
                r = {"recall": retrieval.recall(ids[:Rq].cpu().numpy(), exact_ids[tag]),
                     "scanned_share": float(scanned.double().mean()) / N, "filled_share": float((ids >= 0).float().mean())}
                ms_ivf, ms_exact = [], []
                for _ in range(5):                           # alternating regions
                    a = record()
                    for _ in range(args.reps):
                        ivf_call()
                    b = record()
                    ms_ivf.append(elapsed(a, b) / args.reps)
                    a = record()
                    exact_call(filt, Aq)                     # the yardstick between the regions (all queries unless --alternate_queries)
                    b = record()
                    ms_exact.append(elapsed(a, b))
                r.update({"ms": float(np.median(ms_ivf)), "ms_min": float(np.min(ms_ivf)), "ms_max": float(np.max(ms_ivf)),
                          "exact_ms_alternating": float(np.median(ms_exact)), "exact_queries_alternating": Aq})
                cut = {s: regions(lambda: ivf_call(s), record, elapsed, 1, n_regions=3)["ms"] for s in (1, 3, 4)}
                r["steps_ms"] = {"probe": cut[1], "group_plan": cut[3] - cut[1], "scan": cut[4] - cut[3], "merge": r["ms"] - cut[4]}
                r["over_exact"] = r["ms"] / (r["exact_ms_alternating"] if Aq == Q else res["exact"][tag]["ms"])
                res["ivf"][str(C)][str(P)][tag] = r
            del ws
        del index
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
