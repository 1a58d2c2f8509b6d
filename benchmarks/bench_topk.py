"""Full-graph top-k retrieval at the Reddit shape: Q = 65,536 queries against N = 232,965 candidates of width d = 256 with the
fused score-and-select kernel (csrc/gs_topk.hip, through ops.topk_select) at k = 10 and k = 100, unfiltered and with a filter of
Reddit's average degree (492 sorted ids per row), next to the score-and-count kernel (ops.rank_count: the same contraction with
a cheaper epilogue, the floor) and an eager torch restatement, all in one process.

    python benchmarks/bench_topk.py [--q 65536] [--n 232965] [--d 256] [--ks 10,100] [--out profiles/topk_full.json]

Prints one JSON line (and writes it to --out).  Protocol of bench_rank.py: HIP events on the engine stream around --reps
calls, median (min .. max) of 5 regions after a warm-up call; torch events for the restatement, 3 regions of 1 pass.
  * "select": time of one ops.topk_select over all queries per k, its ratio to "count" and to "torch".
  * "count": time of one ops.rank_count over all queries.
  * "torch": per chunk of --torch_chunk queries S = Xq @ Zc.T, the excluded cells set to -inf, torch.topk(S, k).
  * "agreement": on the first torch chunk, the share of queries whose id lists are identical in both (they may differ at
    near-ties: the two contractions sum in different orders).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmarks.bench_rank import random_filter, regions  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, default=65536)
    ap.add_argument("--n", type=int, default=232965)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--avg_degree", type=int, default=492)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--torch_chunk", type=int, default=4096)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_topk.py needs the GPU"
    from graphsage_amd import engine as eng
    from graphsage_amd import ops
    eng.reset_engine()
    e = eng.get_engine()
    dev = e.device
    Q, N, d = args.q, args.n, args.d
    ks = [int(k) for k in args.ks.split(",")]
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    Z = ops.Mat.zeros(N + 1, d, dev)                       # row N: the pad row, never a candidate
    Z.buf[:N, :d].copy_(torch.nn.functional.normalize(torch.randn(N, d, device=dev, generator=g), dim=1))
    src = torch.randint(0, N, (Q,), device=dev, generator=g, dtype=torch.int32)
    dst = torch.randint(0, N, (Q,), device=dev, generator=g, dtype=torch.int32)
    f_rowptr, f_col = random_filter(N + 1, args.avg_degree, 5, dev)
    Xq = ops.Mat.zeros(Q, d, dev)
    t = torch.zeros(Q, dtype=torch.float32, device=dev)
    n_gt = torch.zeros(Q, dtype=torch.int32, device=dev)
    n_eq = torch.zeros(Q, dtype=torch.int32, device=dev)
    chunk = min(Q, ops.RANK_CHUNK)
    rank_ws = torch.zeros(ops.rank_ws_bytes(chunk, N) // 4 + 2, dtype=torch.int32, device=dev)
    topk_ws = torch.zeros(max(ops.topk_ws_bytes(chunk, N, k) for k in ks) // 8 + 1, dtype=torch.int64, device=dev)
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
    res = {"metric": "full-graph top-k retrieval, fused score-and-select", "Q": Q, "n_cand": N, "d": d, "ks": ks,
           "filter": {"avg_degree": float(f_col.numel()) / (N + 1), "nnz": int(f_col.numel())},
           "basis": "fused: hipEventElapsedTime on the engine stream around %d calls, median / min / max of 5 regions after a "
                    "warm-up call; torch: torch events, 3 regions of 1 pass" % args.reps,
           "workspace_bytes": {str(k): ops.topk_ws_bytes(chunk, N, k) for k in ks},
           "count": {}, "select": {}}
    for tag, filt in filters:
        def count_call():
            ops.rank_count(Xq, Z, dst, n_cand=N, src=src, f_rowptr=filt[0], f_col=filt[1], t=t, n_gt=n_gt, n_eq=n_eq, ws=rank_ws,
                           stream=e.stream)
        count_call()
        e.sync()
        res["count"][tag] = regions(count_call, record, elapsed, args.reps)
    got = {}
    for k in ks:
        ids = torch.zeros((Q, k), dtype=torch.int32, device=dev)
        scores = torch.zeros((Q, k), dtype=torch.float32, device=dev)
        count = torch.zeros(Q, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        res["select"][str(k)] = {}
        for tag, filt in filters:
            def select_call():
                ops.topk_select(Xq, Z, k, n_cand=N, src=src, f_rowptr=filt[0], f_col=filt[1], ids=ids, scores=scores, count=count,
                                ws=topk_ws, stream=e.stream)
            select_call()
            e.sync()
            r = regions(select_call, record, elapsed, args.reps)
            r["select_over_count"] = r["ms"] / res["count"][tag]["ms"]
            r["filled_share"] = float((ids >= 0).float().mean())
            res["select"][str(k)][tag] = r
            got[(k, tag)] = ids[:args.torch_chunk].cpu().numpy()

    z = Z.view()[:N]
    x = Xq.view()
    src64 = src.to(torch.int64)
    ninf = float("-inf")

    def torch_topk(k, filtered, only_first=False):
        out = []
        for q0 in range(0, Q, args.torch_chunk):
            q1 = min(Q, q0 + args.torch_chunk)
            S = x[q0:q1] @ z.T
            rows = torch.arange(q1 - q0, device=dev)
            S[rows, src64[q0:q1]] = ninf
            if filtered:
                a, b = f_rowptr[src64[q0:q1]], f_rowptr[src64[q0:q1] + 1]
                deg = b - a
                r = torch.repeat_interleave(rows, deg)
                off = torch.arange(int(deg.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(deg, 0) - deg, deg)
                c = f_col[torch.repeat_interleave(a, deg) + off].to(torch.int64)
                ok = c < N
                S[r[ok], c[ok]] = ninf
            out.append(torch.topk(S, k, dim=1))
            if only_first:
                break
        return torch.cat([o.indices for o in out]), torch.cat([o.values for o in out])

    def tev():
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def tel(a, b):
        b.synchronize()
        return a.elapsed_time(b)

    res["torch"], res["agreement"] = {}, {}
    for k in ks:
        res["torch"][str(k)], res["agreement"][str(k)] = {}, {}
        for tag, filtered in (("unfiltered", False), ("filtered", True)):
            t_ids, _ = torch_topk(k, filtered, only_first=True)
            torch.cuda.synchronize()
            t_ids = t_ids.cpu().numpy()
            mine = got[(k, tag)][:t_ids.shape[0]]
            res["agreement"][str(k)][tag] = {
                "queries": int(t_ids.shape[0]), "identical_lists_share": float((t_ids == mine).all(1).mean()),
                "identical_sets_share": float(np.mean([set(a) == set(b) for a, b in zip(t_ids.tolist(), mine.tolist())]))}
            r = regions(lambda: torch_topk(k, filtered), tev, tel, 1, n_regions=3)
            r["chunk"] = args.torch_chunk
            res["torch"][str(k)][tag] = r
            sel = res["select"][str(k)][tag]
            sel["select_over_torch"] = sel["ms"] / r["ms"]
            sel["not_slower_than_torch"] = bool(sel["ms"] <= r["ms"])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
