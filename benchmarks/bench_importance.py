"""Importance neighborhoods at the Reddit shape: num_walks walks of walk_len nodes from EVERY node of reddit_shaped_device's train
view (gs_walk_paths), then the [N, slots] table from those paths (gs_importance_table, one launch over all starts), timed
separately, next to a torch restatement of the table rule on the same device (per-row sort, run lengths by scatter-add, two
more per-row sorts for the selection and the remainders, a batched search for the slots), whose table is compared with the
kernel's bit for bit at the size that is timed.

    python benchmarks/bench_importance.py [--shapes 50:3,200:3] [--top 25] [--slots 128] [--out profiles/importance_neighbors.json]

Prints one JSON line (and writes it to --out).  Torch events on the current stream around one call, median (min .. max) of
--regions regions after a warm-up call of the same shape; --reps calls per region for the two kernels, one for the torch rows.
"walks" is every gs_walk_paths launch of the job (chunks of utils.WALK_CHUNK walks) into one paths tensor; "table" is the one
gs_importance_table launch that reads it; "torch" is torch_table() on the same paths.
"""
import argparse
import json
import os
import sys

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


def torch_table(paths, num_walks, walk_len, n_nodes, top, slots, pad_id):
    """The rule of include/graphsage_amd.h, section IMPORTANCE, in batched torch ops -> (table int32 [n_starts, slots], stats int32
    [n_starts, 2]).  int64 keys; every row is sorted whole, whatever it holds."""
    n = paths.shape[0] // num_walks
    dev = paths.device
    p = paths[:, :walk_len].reshape(n, num_walks, walk_len).long()
    u = p[:, 0, 0]
    vis = p[:, :, 1:].reshape(n, -1)
    V = vis.shape[1]
    BIG = 1 << 40
    keep = (vis >= 0) & (vis < n_nodes) & (vis != u[:, None]) & ((u >= 0) & (u < n_nodes))[:, None]
    key = torch.where(keep, vis, torch.full_like(vis, BIG)).sort(dim=1).values
    valid = key < BIG
    head = valid.clone()
    head[:, 1:] &= key[:, 1:] != key[:, :-1]
    run = (torch.cumsum(head, 1) - 1).clamp(min=0)                  # run index of every kept position
    cnt = torch.zeros((n, V), dtype=torch.int64, device=dev).scatter_add_(1, run, valid.long())
    ids = torch.full((n, V), BIG, dtype=torch.int64, device=dev).scatter_reduce_(1, run, key, "amin", include_self=True)
    m = head.sum(1)
    col = torch.arange(V, device=dev)[None, :]
    is_run = col < m[:, None]
    key2 = torch.where(is_run, ((4096 - cnt) << 32) | ids.clamp(max=(1 << 31) - 1), torch.full_like(cnt, 1 << 62)).sort(dim=1).values
    sel = col < torch.minimum(m, torch.full_like(m, top))[:, None]
    c = torch.where(sel, 4096 - (key2 >> 32), torch.zeros_like(key2))
    sid = key2 & 0xFFFFFFFF
    C = c.sum(1, keepdim=True)
    q = c * slots // C.clamp(min=1)
    r = c * slots - q * C
    rest = slots - q.sum(1, keepdim=True)
    order3 = torch.where(sel, ((C - r) << 32) | sid, torch.full_like(sid, 1 << 62)).argsort(dim=1, stable=True)
    extra = torch.zeros_like(q).scatter_(1, order3, (col < rest).long().expand(n, V).contiguous())
    nk = torch.where(sel, q + extra, torch.zeros_like(q))
    order4 = torch.where(sel, sid, torch.full_like(sid, 1 << 62)).argsort(dim=1, stable=True)      # ascending id
    nk4, id4 = nk.gather(1, order4), sid.gather(1, order4)
    cum = torch.cumsum(nk4, 1)
    slot = torch.arange(slots, device=dev)[None, :].expand(n, slots).contiguous()
    which = torch.searchsorted(cum, slot, right=True).clamp(max=V - 1)
    table = torch.where((m > 0)[:, None], id4.gather(1, which), torch.full_like(which, pad_id)).to(torch.int32)
    stats = torch.stack([m, (nk > 0).sum(1)], dim=1).to(torch.int32)
    return table, stats


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_nodes", type=int, default=232965)
    ap.add_argument("--avg_degree", type=int, default=492)
    ap.add_argument("--shapes", default="50:3,200:3", help="num_walks:walk_len, comma separated")
    ap.add_argument("--top", type=int, default=25)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=64,
                    help="calls per timed region of the two kernels (a region of tens of milliseconds at the default shapes)")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_importance.py needs the GPU"
    from graphsage_amd import ops, utils
    dev = torch.device("cuda:0")
    G = utils.reddit_shaped_device(dev, n_nodes=args.n_nodes, avg_degree=args.avg_degree)
    rowptr, col = G.train_csr
    N = G.n_nodes
    starts = torch.arange(N, dtype=torch.int32, device=dev)
    thr = ops.walk_thresholds(1.0, 1.0)
    res = {"metric": "importance neighborhoods of every node, train view of the Reddit-shaped graph", "n_nodes": N,
           "nnz": int(col.numel()), "top": args.top, "slots": args.slots, "chunk_walks": utils.WALK_CHUNK,
           "basis": "torch events around one call, median / min / max of %d regions after a warm-up call; %d calls per region for "
                    "the kernels, 1 for torch" % (args.regions, args.reps), "shapes": {}}
    for shape in args.shapes.split(","):
        R, L = (int(x) for x in shape.split(":"))
        n_walks = N * R
        paths = torch.empty((n_walks, L), dtype=torch.int32, device=dev)
        counts = torch.empty(min(n_walks, utils.WALK_CHUNK), dtype=torch.int32, device=dev)
        table = torch.empty((N, args.slots), dtype=torch.int32, device=dev)
        stats = torch.empty((N, 2), dtype=torch.int32, device=dev)

        def walks_call():
            for w0 in range(0, n_walks, utils.WALK_CHUNK):
                n = min(utils.WALK_CHUNK, n_walks - w0)
                ops.walk_paths(rowptr, col, starts, R, L, thr, 123, walk0=w0, n_walks=n, paths=paths[w0:w0 + n], counts=counts[:n])

        def table_call():
            ops.importance_table(paths, R, L, N, args.top, args.slots, N, table=table, stats=stats)

        def torch_call():
            return torch_table(paths, R, L, N, args.top, args.slots, N)

        walks_call()
        table_call()
        t_table, t_stats = torch_call()
        torch.cuda.synchronize()
        st = stats.cpu().numpy()
        one = {"num_walks": R, "walk_len": L, "visits_per_start": R * (L - 1), "n_walks": n_walks,
               "paths_mb": paths.numel() * 4 / 1e6, "table_mb": table.numel() * 4 / 1e6,
               "distinct_mean": float(st[:, 0].mean()), "kept_mean": float(st[:, 1].mean()), "empty": int((st[:, 0] == 0).sum()),
               "torch_table_equal": bool(torch.equal(t_table, table)), "torch_stats_equal": bool(torch.equal(t_stats, stats))}
        del t_table, t_stats
        one["walks"] = regions(walks_call, args.regions, reps=args.reps)
        one["table"] = regions(table_call, args.regions, reps=args.reps)
        one["table"]["starts_per_s"] = N / (one["table"]["ms"] * 1e-3)
        one["table"]["nonempty_starts"] = int((st[:, 0] > 0).sum())      # an empty row leaves before the first sort
        # the least the table launch moves: every path entry read once, every table and stats entry written once
        one["table"]["bytes"] = paths.numel() * 4 + table.numel() * 4 + stats.numel() * 4
        one["table"]["gb_per_s"] = one["table"]["bytes"] / (one["table"]["ms"] * 1e-3) / 1e9
        one["torch"] = regions(torch_call, min(args.regions, 3))
        one["torch"]["over_table"] = one["torch"]["ms"] / one["table"]["ms"]
        res["shapes"][shape] = one
        del paths, counts, table, stats
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
