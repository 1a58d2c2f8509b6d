"""Correct and Smooth / label propagation: one propagation step (gs_prop_step, csrc/gs_propagate.hip) and a whole
correct_and_smooth (50 + 50 steps) on the Reddit-shaped graph (utils.reddit_shaped_device: N = 232,965, average degree 492) at
C = 41 and, for the step, C = 121, and on the R-MAT graph at C = 41.

    python benchmarks/bench_propagate.py [--reps 10] [--rmat_nodes 10000000 --rmat_edges 200000000] [--out FILE]

Prints one JSON line.  Per (graph, C):
  * "step": ONE fused step out = clamp(alpha S X + R) over every row; HIP events on the engine's stream around --reps steps
    (ping-pong tables), median of 5 regions after a warm-up.  "gathered_TB_per_s" = nnz * round_up(C, 4) * 4 bytes / time: the
    table rows the step gathers; "bytes" also counts the ids and weights (8 bytes per entry) and the R and out rows.
  * "composed": the same step from the kernels that were there before, put together here only: X * w (torch), gs_csr_reduce_fwd
    GS_CSR_MEAN in row windows, * deg w, axpy with R, clamp (torch), all on the engine's stream; "max_abs_diff" against the
    fused step.
  * "torch_sparse": clamp(alpha * (CSR tensor with values w_r w_c) @ X + R) where torch.sparse.mm runs on this build.
  * "correct_and_smooth": host clock around propagation.correct_and_smooth (uploads, 50 + 50 steps, downloads), best of 2, with
    micro-F1 before / after on the val and test nodes -- from SYNTHETIC predictions (the labels blurred by noise), since no
    model is trained here; for information only.
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


def median_ms(e, fn, reps, regions=5):
    from graphsage_amd import ops
    fn()
    e.sync()
    ms = []
    for _ in range(regions):
        a, b = ops.Event(), ops.Event()
        a.record(e.stream)
        for _ in range(reps):
            fn()
        b.record(e.stream)
        e.sync()
        ms.append(a.elapsed_ms(b) / reps)
    return float(np.median(ms)), float(np.min(ms))


def bench_step(e, prop, C, alpha, reps, with_torch):
    from graphsage_amd import inference as inf
    from graphsage_amd.ops import Mat
    graph = prop.graph
    n_rows, N = graph.n_rows, graph.n_nodes
    g = torch.Generator(device=e.device)
    g.manual_seed(C)
    A, B, R = prop.tables(C)
    A.buf[:N, :C].copy_(torch.rand(N, C, device=e.device, generator=g))
    R.buf[:N, :C].copy_(torch.rand(N, C, device=e.device, generator=g) * (1.0 - alpha))
    torch.cuda.synchronize()
    lo, hi = 0.0, 1.0
    state = {"x": A, "y": B}

    def fused():
        prop.step(state["x"], state["y"], R, alpha, lo, hi)
        state["x"], state["y"] = state["y"], state["x"]

    cpad = (C + 3) // 4 * 4
    med, best = median_ms(e, fused, reps)
    gathered = graph.nnz * cpad * 4
    total = gathered + graph.nnz * 8 + 2 * n_rows * cpad * 4
    res = {"C": C, "ld": A.ld, "step": {"ms": med, "ms_min": best, "gathered_TB_per_s": gathered / (med * 1e-3) / 1e12,
                                       "bytes": total, "TB_per_s": total / (med * 1e-3) / 1e12}}

    # the same step from A into B, once, as the yardstick of the two comparators
    prop.step(A, B, R, alpha, lo, hi)
    e.sync()
    want = B.buf.clone()

    # composed from the kernels that were there before (torch's elementwise launches ride on the engine's stream)
    ext = torch.cuda.ExternalStream(e.stream)
    Xs = Mat.zeros(n_rows, C, e.device, 32)
    M = Mat.zeros(n_rows, C, e.device, 32)
    w_col = prop.w[:, None]
    dw_col = (prop.deg.to(torch.float32) * prop.w)[:, None]
    torch.cuda.synchronize()

    def composed():
        with torch.cuda.stream(ext):
            torch.mul(A.buf, w_col, out=Xs.buf)
        for r0, n in graph.windows(inf.WINDOW_ROWS):
            graph.reduce(e, inf.CSR_MEAN, Xs, M.rows_slice(r0, r0 + n), r0, n)
        with torch.cuda.stream(ext):
            torch.mul(M.buf, dw_col, out=M.buf)
            torch.add(R.buf, M.buf, alpha=alpha, out=M.buf)
            torch.clamp(M.buf, lo, hi, out=M.buf)

    med, best = median_ms(e, composed, reps)
    res["composed"] = {"ms": med, "ms_min": best, "max_abs_diff": float((M.buf[:N] - want[:N]).abs().max())}
    res["fused_speedup_vs_composed"] = res["composed"]["ms"] / res["step"]["ms"]

    if with_torch:
        try:
            rowptr, col, _, _ = graph.on(e.device)
            deg_all = rowptr[1:] - rowptr[:-1]
            rows = torch.repeat_interleave(torch.arange(n_rows, device=e.device), deg_all)
            vals = prop.w[rows] * prop.w[col.long()]
            del rows
            S = torch.sparse_csr_tensor(rowptr, col.to(torch.int64), vals, size=(n_rows, n_rows))
            x, r = A.buf[:, :C].contiguous(), R.buf[:, :C].contiguous()
            torch.cuda.synchronize()

            def sparse():
                with torch.cuda.stream(ext):
                    return torch.clamp(torch.add(r, torch.sparse.mm(S, x), alpha=alpha), lo, hi)

            med, best = median_ms(e, sparse, max(1, reps // 2))
            got = sparse()
            e.sync()                              # it ran on the engine's stream; the comparison below runs on torch's
            res["torch_sparse"] = {"ms": med, "ms_min": best, "max_abs_diff": float((got[:N] - want[:N, :C]).abs().max())}
            del got
            res["fused_speedup_vs_torch_sparse"] = med / res["step"]["ms"]
            del S, vals
        except Exception as ex:                  # recorded, not hidden: the torch form is a yardstick, not the product
            res["torch_sparse"] = {"failed": "%s: %s" % (type(ex).__name__, str(ex)[:300])}
        torch.cuda.synchronize()
    del Xs, M, want
    torch.cuda.empty_cache()
    return res


def micro_f1(labels, scores, nodes):
    return float((labels[nodes].argmax(axis=1) == scores[nodes].argmax(axis=1)).mean())      # single-label: micro-F1 = accuracy


def bench_cs(e, prop, labels, known, val, test, seed):
    from graphsage_amd import propagation as pr
    rng = np.random.RandomState(seed)
    logits = rng.randn(*labels.shape).astype(np.float32) * 1.5 + 2.0 * labels
    preds = np.exp(logits - logits.max(axis=1, keepdims=True))
    preds /= preds.sum(axis=1, keepdims=True)
    times = []
    for _ in range(2):
        t0 = time.time()
        res = pr.correct_and_smooth(e, prop.graph, preds, labels, known, iters=50, propagator=prop)
        times.append(time.time() - t0)
    t0 = time.time()
    lp = pr.label_propagation(e, prop.graph, labels, known, iters=50, propagator=prop)
    t_lp = time.time() - t0
    return {"seconds": min(times), "iters": "50 + 50", "sigma": res["sigma"], "known": int(len(known)),
            "predictions": "synthetic: softmax(2 * onehot + 1.5 * N(0, 1))",
            "val_f1_micro": {"base": micro_f1(labels, preds, val), "correct_smooth": micro_f1(labels, res["preds"], val),
                             "label_propagation": micro_f1(labels, lp, val)},
            "test_f1_micro": {"base": micro_f1(labels, preds, test), "correct_smooth": micro_f1(labels, res["preds"], test),
                              "label_propagation": micro_f1(labels, lp, test)},
            "label_propagation_seconds": t_lp}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.8)
    ap.add_argument("--avg_degree", type=int, default=492)
    ap.add_argument("--rmat_nodes", type=int, default=10000000)
    ap.add_argument("--rmat_edges", type=int, default=200000000)
    ap.add_argument("--no_rmat", action="store_true")
    ap.add_argument("--no_torch", action="store_true", help="skip the torch.sparse.mm restatement")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_propagate.py needs the GPU"
    from graphsage_amd import engine as eng
    from graphsage_amd import propagation as pr
    from graphsage_amd import utils
    from graphsage_amd.inference import FullGraph
    eng.reset_engine()
    e = eng.get_engine()
    res = {"metric": "Correct and Smooth: one propagation step and 50 + 50 steps",
           "basis": "step: hipEventElapsedTime on the engine stream around %d steps, median of 5 regions; correct_and_smooth: "
                    "host clock, best of 2" % args.reps, "alpha": args.alpha, "graphs": {}}

    dg = utils.reddit_shaped_device(e.device, feat_dim=8, avg_degree=args.avg_degree)
    graph = FullGraph.from_csr(dg.test_csr[0], dg.test_csr[1], dg.n_nodes)
    deg = np.diff(graph.rowptr_host)
    prop = pr.Propagator(e, graph)
    entry = {"n_nodes": graph.n_nodes, "nnz": graph.nnz, "degree_median": float(np.median(deg)), "degree_max": int(deg.max()),
             "rows_cut": int(graph.splits.shape[0]), "steps": [bench_step(e, prop, C, args.alpha, args.reps, not args.no_torch)
                                                               for C in (41, 121)]}
    labels = dg.label_table.numpy()[:dg.n_nodes]
    val = np.flatnonzero(dg.val_mask.cpu().numpy())
    test = np.flatnonzero(dg.test_mask.cpu().numpy())
    known = np.setdiff1d(np.arange(dg.n_nodes), np.concatenate([val, test]))
    entry["correct_and_smooth"] = bench_cs(e, prop, labels, known, val, test, 5)
    res["graphs"]["reddit_shaped"] = entry
    del prop, graph, dg
    torch.cuda.empty_cache()

    if not args.no_rmat:
        rowptr, col = utils.rmat_csr_device(args.rmat_nodes, args.rmat_edges, e.device, seed=123)
        graph = FullGraph.from_csr(rowptr, col, args.rmat_nodes)
        del rowptr, col
        deg = np.diff(graph.rowptr_host)
        prop = pr.Propagator(e, graph)
        res["graphs"]["rmat"] = {"n_nodes": graph.n_nodes, "nnz": graph.nnz, "degree_median": float(np.median(deg)),
                                 "degree_max": int(deg.max()), "rows_cut": int(graph.splits.shape[0]),
                                 "steps": [bench_step(e, prop, 41, args.alpha, args.reps, not args.no_torch)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
