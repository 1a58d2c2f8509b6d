"""Link-ranking baselines (gs_nbr_rank, csrc/gs_nbr_rank.hip): time per kind and per 10^6 paths at two shapes, next to the same
ranking composed from eager torch.

    python benchmarks/bench_nbr_rank.py [--shapes reddit,rmat] [--rmat_nodes 10000000 --rmat_edges 200000000]
                                        [--rmat_queries 65536] [--torch_queries 16384] [--tiles 0] [--out FILE]

Prints one JSON line.  Per shape:
  * "reddit": the graph of --synthetic reddit (utils.reddit_shaped: N = 232,965, average degree 50), its test graph, every
    held-out edge in both directions, the graph's edges as the filter -- what --rank_baselines ranks.
  * "rmat": the R-MAT graph of bench.py --workload rmat (utils.rmat_csr_device, made simple on the device), --rmat_queries
    random edges (a random source, one of its two-hop nodes or a random node), the graph's edges as the filter.
  * per kind "kernel_ms": HIP events on the engine's stream around ONE gs_nbr_rank launch over all queries (inputs grouped and
    uploaded before), median of 3 after a warm-up; "ms_per_Mpaths" = kernel_ms / (paths / 10^6), paths = sum over distinct
    sources of sum_{w in N(u)} deg w; "wall_s": host clock around link_heuristics.rank_neighbors (grouping, uploads, launch,
    downloads, metrics).  --tiles lists LDS tile sizes to time besides the default.
  * "torch": the first --torch_queries queries in group order ranked by eager torch, in batches of sources: S^T = A^T @ X with X
    [N, B] dense, X[w, b] = q[w] for w in N(u_b) (torch.sparse.mm, fp32), invalid candidates set to 0, then per edge compare
    and sum; "kernel_ms_same_queries" is gs_nbr_rank over the same queries.  fp32 sums are exact for cn only: "cn_equal" says
    whether the counts agree there.
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


def launch_ms(e, fn, regions=3):
    from graphsage_amd import ops
    fn()
    e.sync()
    ms = []
    for _ in range(regions):
        a, b = ops.Event(), ops.Event()
        a.record(e.stream)
        fn()
        b.record(e.stream)
        e.sync()
        ms.append(a.elapsed_ms(b))
    return float(np.median(ms)), float(np.min(ms))


def prepared(e, graph, filt, edges, kind, tile):
    """A closure that launches gs_nbr_rank over `edges`, and what it needs to read the answer back."""
    from graphsage_amd import link_heuristics as lh
    from graphsage_amd import ops
    N = graph.n_nodes
    sources = np.unique(edges[:, 0])
    work = np.zeros(N, np.int64)
    work[sources] = graph.two_hop_work(sources)
    order, gp, gs, dst = lh.group_by_source(edges[:, 0], edges[:, 1], work)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(e.device)
    gp, gs, dst = up(gp), up(gs), up(dst)
    rowptr, col, deg = graph.on(e.device)
    q = graph.weights_on(kind, e.device)
    f_rowptr, f_col = filt.on(e.device, N)
    out = [torch.zeros(len(edges), dtype=torch.int32, device=e.device) for _ in range(3)]
    max_deg = int(graph.deg[sources].max())
    grid = ops.nbr_rank_grid(len(sources))
    ws = torch.empty(max(1, ops.nbr_rank_ws_bytes(grid, max_deg) // 4), dtype=torch.int32, device=e.device)
    torch.cuda.synchronize()

    def fn():
        ops.nbr_rank(rowptr, col, N, gp, gs, dst, q=q, deg=deg if kind == "jaccard" else None, f_rowptr=f_rowptr, f_col=f_col,
                     kind="jaccard" if kind == "jaccard" else "sum", tile=tile, max_src_degree=max_deg, t=out[0], n_gt=out[1],
                     n_eq=out[2], ws=ws, stream=e.stream)

    return fn, out, order, int(work[sources].sum()), len(sources)


def torch_rank(e, graph, edges, kind, batch):
    """The same ranking from eager torch for `edges` (sorted by source).  Returns (n_gt, n_eq) int64 on the host, seconds."""
    N = graph.n_nodes
    dev = e.device
    rowptr, col, deg = graph.on(dev)
    q = torch.from_numpy(graph.weights(kind)[0].astype(np.float32)).to(dev)
    rows = torch.repeat_interleave(torch.arange(N, device=dev), rowptr[1:] - rowptr[:-1])
    col64 = col[:rows.numel()].to(torch.int64)
    At = torch.sparse_coo_tensor(torch.stack([col64, rows]), torch.ones(rows.numel(), device=dev), (N, N)).coalesce().to_sparse_csr()
    keys = rows * N + col64                                             # ascending: rows ascend and are sorted inside
    degf = deg.to(torch.float32)
    src = torch.from_numpy(edges[:, 0]).to(dev)
    dst = torch.from_numpy(edges[:, 1]).to(dev)
    n_gt = torch.zeros(len(edges), dtype=torch.int64, device=dev)
    n_eq = torch.zeros(len(edges), dtype=torch.int64, device=dev)
    us, inv = torch.unique(src, return_inverse=True)
    torch.cuda.synchronize()
    t0 = time.time()
    for b0 in range(0, us.numel(), batch):
        u = us[b0:b0 + batch]
        B = u.numel()
        lens = rowptr[u + 1] - rowptr[u]
        which = torch.repeat_interleave(torch.arange(B, device=dev), lens)
        pos = torch.arange(int(lens.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens) \
            + torch.repeat_interleave(rowptr[u], lens)
        nb = col[pos].to(torch.int64)                                  # the neighbors w of every source of the batch
        X = torch.zeros(N, B, device=dev)
        X[nb, which] = q[nb]
        S = torch.sparse.mm(At, X)                                      # [N, B]: S[x, b] = s(u_b, x)
        S[nb, which] = 0                                                # the filter: the graph's own edges
        S[u, torch.arange(B, device=dev)] = 0
        sel = torch.nonzero((inv >= b0) & (inv < b0 + B)).reshape(-1)
        for k0 in range(0, sel.numel(), 64):                            # edges of these sources, 64 columns at a time
            k = sel[k0:k0 + 64]
            b = inv[k] - b0
            Sk = S[:, b]                                                # [N, E_k]
            x = dst[k]
            cols = torch.arange(k.numel(), device=dev)
            t = _true_scores(keys, rowptr, col, q, src[k], x, N, dev)   # from the unfiltered rows: the filter may hold dst
            Sk[x, cols] = 0                                             # dst is no candidate of its own edge
            if kind == "jaccard":
                den_t = degf[src[k]] + degf[x] - t
                den = degf[src[k]][None, :] + degf[:, None] - Sk
                a, c = Sk * den_t[None, :], t[None, :] * den
                pos_mask = Sk > 0
                gt, eq = (a > c) & pos_mask, (a == c) & pos_mask
            else:
                gt, eq = (Sk > t[None, :]) & (Sk > 0), (Sk == t[None, :]) & (Sk > 0)
            g, q_ = gt.sum(0), eq.sum(0)
            valid = N - lens[b] - 1 - ((x != src[k]) & ~_in_rows(keys, N, src[k], x)).to(torch.int64)
            q_ = torch.where(t == 0, valid - g, q_)
            n_gt[k], n_eq[k] = g, q_
    torch.cuda.synchronize()
    return n_gt.cpu().numpy(), n_eq.cpu().numpy(), time.time() - t0


def _in_rows(keys, N, u, x):
    """bool per pair: x in N(u), by a search in the ascending list of row * N + col."""
    want = u * N + x
    at = torch.searchsorted(keys, want).clamp(max=keys.numel() - 1)
    return keys[at] == want


def _true_scores(keys, rowptr, col, q, u, x, N, dev):
    """t = s(u, x) per pair: sum of q[w] over w in N(u) with x in N(w)."""
    lens = rowptr[u + 1] - rowptr[u]
    which = torch.repeat_interleave(torch.arange(u.numel(), device=dev), lens)
    pos = torch.arange(int(lens.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens) \
        + torch.repeat_interleave(rowptr[u], lens)
    w = col[pos].to(torch.int64)
    hit = _in_rows(keys, N, w, x[which])
    return torch.zeros(u.numel(), device=dev).index_add_(0, which, q[w] * hit)


def bench_shape(e, name, graph, edges, args):
    from graphsage_amd import link_heuristics as lh
    filt = graph.rank_filter()
    res = {"nodes": graph.n_nodes, "entries": int(graph.col.size), "max_degree": graph.max_degree, "queries": int(len(edges)),
           "kinds": {}}
    tiles = [0] + [int(t) for t in args.tiles.split(",") if t and int(t)]
    for kind in lh.KINDS:
        r = {}
        for tile in tiles:
            fn, out, order, paths, sources = prepared(e, graph, filt, edges, kind, tile)
            med, best = launch_ms(e, fn)
            key = "kernel_ms" if tile == 0 else "kernel_ms_tile_%d" % tile
            r[key], r[key + "_min"] = med, best
            if tile == 0:
                r["paths"], r["sources"], r["ms_per_Mpaths"] = paths, sources, med / max(paths / 1e6, 1e-9)
        t0 = time.time()
        full = lh.rank_neighbors(e, graph, edges, kind=kind, filt=filt)
        r["wall_s"], r["mrr"], r["zero"], r["scale_bits"] = time.time() - t0, full["mrr"], full["zero"], full["scale_bits"]
        res["kinds"][kind] = r
        print("# %s %s %s" % (name, kind, json.dumps(r)), file=sys.stderr, flush=True)
    # the composed form on a prefix of the queries, in group order
    nq = min(args.torch_queries, len(edges))
    if nq:
        sub = edges[np.argsort(edges[:, 0], kind="stable")[:nq]]
        res["torch"] = {"queries": int(nq), "batch_sources": args.torch_batch}
        for kind in lh.KINDS:
            fn, out, order, paths, sources = prepared(e, graph, filt, sub, kind, 0)
            med, _ = launch_ms(e, fn)
            r = {"kernel_ms_same_queries": med, "paths": paths}
            try:
                g, q_, secs = torch_rank(e, graph, sub, kind, args.torch_batch)
                r["torch_ms"] = secs * 1e3
                r["torch_over_kernel"] = r["torch_ms"] / med
                if kind == "cn":
                    got_gt = lh._scatter(out[1].cpu().numpy(), order)
                    got_eq = lh._scatter(out[2].cpu().numpy(), order)
                    r["cn_equal"] = bool(np.array_equal(got_gt, g) and np.array_equal(got_eq, q_))
            except Exception as ex:                                     # torch.sparse.mm or the memory it needs
                r["torch_error"] = repr(ex)[:300]
            res["torch"][kind] = r
            print("# %s torch %s %s" % (name, kind, json.dumps(r)), file=sys.stderr, flush=True)
    return res


def reddit_shape():
    from graphsage_amd import link_heuristics as lh
    from graphsage_amd import utils
    G = utils.reddit_shaped(seed=123)
    rowptr, col = utils.build_csr(G.n_nodes, G.src, G.dst)
    val = np.stack([G.src, G.dst], axis=1)[G.train_removed].astype(np.int64)
    return lh.SimpleGraph.from_csr(rowptr, col, G.n_nodes), np.concatenate([val, val[:, ::-1]], axis=0)


def rmat_shape(e, n_nodes, n_edges, n_queries):
    from graphsage_amd import link_heuristics as lh
    from graphsage_amd import utils
    rowptr, col = utils.rmat_csr_device(n_nodes, n_edges, e.device, seed=123)
    rows = torch.repeat_interleave(torch.arange(n_nodes, device=e.device), rowptr[1:] - rowptr[:-1])
    c = col.to(torch.int64)
    key = torch.unique((rows * n_nodes + c)[rows != c])                 # sorted, no duplicate, no loop
    del rows, c, rowptr, col
    new_rp = torch.zeros(n_nodes + 1, dtype=torch.int64, device=e.device)
    new_rp[1:] = torch.cumsum(torch.bincount(key // n_nodes, minlength=n_nodes), 0)
    graph = lh.SimpleGraph(new_rp.cpu().numpy(), (key % n_nodes).to(torch.int32).cpu().numpy(), n_nodes)
    del key, new_rp
    torch.cuda.empty_cache()
    rng = np.random.RandomState(5)
    src = rng.randint(0, n_nodes, n_queries).astype(np.int64)
    dst = rng.randint(0, n_nodes, n_queries).astype(np.int64)
    for k in range(0, n_queries, 2):                                    # every other partner is a two-hop node of its source
        row = graph.col[graph.rowptr[src[k]]:graph.rowptr[src[k] + 1]]
        if row.size:
            w = int(row[rng.randint(row.size)])
            row2 = graph.col[graph.rowptr[w]:graph.rowptr[w + 1]]
            if row2.size:
                dst[k] = int(row2[rng.randint(row2.size)])
    return graph, np.stack([src, dst], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="reddit,rmat")
    ap.add_argument("--rmat_nodes", type=int, default=10000000)
    ap.add_argument("--rmat_edges", type=int, default=200000000)
    ap.add_argument("--rmat_queries", type=int, default=65536)
    ap.add_argument("--torch_queries", type=int, default=16384)
    ap.add_argument("--torch_batch", type=int, default=64)
    ap.add_argument("--tiles", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from graphsage_amd import engine as eng
    e = eng.get_engine()
    res = {"bench": "nbr_rank", "device": torch.cuda.get_device_name(0)}
    for name in args.shapes.split(","):
        t0 = time.time()
        graph, edges = reddit_shape() if name == "reddit" else rmat_shape(e, args.rmat_nodes, args.rmat_edges, args.rmat_queries)
        print("# %s: graph ready in %.1f s" % (name, time.time() - t0), file=sys.stderr, flush=True)
        res[name] = bench_shape(e, name, graph, edges, args)
        del graph
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
