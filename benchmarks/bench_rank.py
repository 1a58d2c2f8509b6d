"""Full-graph link ranking at the Reddit shape: Q = 65,536 queries against N = 232,965 candidates of width d = 256 with the fused
score-and-count kernel (csrc/gs_rank.hip, through ops.rank_count), unfiltered and with a filter of Reddit's average degree
(492 sorted ids per row), next to an eager torch restatement on the same device.

    python benchmarks/bench_rank.py [--q 65536] [--n 232965] [--d 256] [--out profiles/rank_full.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o rank -- python benchmarks/bench_rank.py --hip_only

Prints one JSON line (and writes it to --out):
  * "fused": time of one ops.rank_count over all queries (HIP events on the engine stream around --reps calls, median and
    minimum of 5 regions, after a warm-up call), the rate of useful FLOP 2 * Q * n_cand * d / time (the t tile of every
    slice is not counted) and that rate's share of the fp32 matrix peak (157.3 TFLOP/s).
  * "torch": the same counts as a user without the kernel would write them: per chunk of --torch_chunk queries
    S = Xq @ Zc.T, the excluded cells set to -inf, (S > t).sum(1) and (S == t).sum(1).  torch events, same regions.
  * "agreement": on the first torch chunk, the share of queries whose (n_gt, n_eq) are identical in both (they may differ
    at near-ties: the two contractions sum in different orders).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MATRIX_PEAK = 157.3e12


def random_filter(n, avg_degree, seed, device):
    """(rowptr int64 [n + 1], col int32) on the device: every row strictly ascending ids in [0, n), about avg_degree of them
    (cumulated positive gaps, cut at n)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    width = int(avg_degree * 1.25)
    gaps = torch.randint(1, max(2, 2 * n // avg_degree), (n, width), device=device, generator=g, dtype=torch.int64)
    ids = torch.cumsum(gaps, 1) - 1
    keep = ids < n
    deg = keep.sum(1)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
    rowptr[1:] = torch.cumsum(deg, 0)
    return rowptr, ids[keep].to(torch.int32)


def regions(fn, record, elapsed, reps, n_regions=5):
    ms = []
    for _ in range(n_regions):
        a = record()
        for _ in range(reps):
            fn()
        b = record()
        ms.append(elapsed(a, b) / reps)
    return {"ms": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, default=65536)
    ap.add_argument("--n", type=int, default=232965)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--avg_degree", type=int, default=492)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--torch_chunk", type=int, default=4096)
    ap.add_argument("--hip_only", action="store_true", help="skip the torch restatement (kernel-trace runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_rank.py needs the GPU"
    from graphsage_amd import engine as eng
    from graphsage_amd import ops
    eng.reset_engine()
    e = eng.get_engine()
    dev = e.device
    Q, N, d = args.q, args.n, args.d
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
    ws = torch.zeros(ops.rank_ws_bytes(min(Q, ops.RANK_CHUNK), N) // 4 + 2, dtype=torch.int32, device=dev)
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

    flop = 2.0 * Q * N * d
    res = {"metric": "full-graph link ranking, fused score-and-count", "Q": Q, "n_cand": N, "d": d,
           "filter": {"avg_degree": float(f_col.numel()) / (N + 1), "nnz": int(f_col.numel())},
           "basis": "fused: hipEventElapsedTime on the engine stream around %d calls, median / min / max of 5 regions after a "
                    "warm-up call; torch: torch events, same regions; FLOP = 2 Q n_cand d" % args.reps,
           "slab_bytes": ops.rank_ws_bytes(min(Q, ops.RANK_CHUNK), N)}
    fused = {}
    for tag, filt in (("unfiltered", (None, None)), ("filtered", (f_rowptr, f_col))):
        def call():
            ops.rank_count(Xq, Z, dst, n_cand=N, src=src, f_rowptr=filt[0], f_col=filt[1], t=t, n_gt=n_gt, n_eq=n_eq, ws=ws,
                           stream=e.stream)
        call()
        e.sync()
        r = regions(call, record, elapsed, args.reps)
        r["TFLOP_per_s"] = flop / (r["ms"] * 1e-3) / 1e12
        r["share_of_fp32_matrix_peak"] = flop / (r["ms"] * 1e-3) / FP32_MATRIX_PEAK
        r["counts"] = (n_gt.cpu().numpy().astype(np.int64), n_eq.cpu().numpy().astype(np.int64))
        fused[tag] = r

    if not args.hip_only:
        z = Z.view()[:N]
        x = Xq.view()
        src64, dst64 = src.to(torch.int64), dst.to(torch.int64)
        ninf = float("-inf")

        def torch_counts(filtered, only_first=False):
            gts, eqs = [], []
            for q0 in range(0, Q, args.torch_chunk):
                q1 = min(Q, q0 + args.torch_chunk)
                S = x[q0:q1] @ z.T
                tt = (x[q0:q1] * Z.view()[dst64[q0:q1]]).sum(1)
                rows = torch.arange(q1 - q0, device=dev)
                S[rows, dst64[q0:q1]] = ninf
                S[rows, src64[q0:q1]] = ninf
                if filtered:
                    a, b = f_rowptr[src64[q0:q1]], f_rowptr[src64[q0:q1] + 1]
                    deg = b - a
                    r = torch.repeat_interleave(rows, deg)
                    off = torch.arange(int(deg.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(deg, 0) - deg, deg)
                    c = f_col[torch.repeat_interleave(a, deg) + off].to(torch.int64)
                    ok = c < N
                    S[r[ok], c[ok]] = ninf
                gts.append((S > tt[:, None]).sum(1))
                eqs.append((S == tt[:, None]).sum(1))
                if only_first:
                    break
            return torch.cat(gts), torch.cat(eqs)

        def tev():
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            return ev

        def tel(a, b):
            b.synchronize()
            return a.elapsed_time(b)

        res["torch"], res["agreement"] = {}, {}
        for tag, filtered in (("unfiltered", False), ("filtered", True)):
            gt, eq = torch_counts(filtered, only_first=True)
            torch.cuda.synchronize()
            n = gt.numel()
            fg, fe = fused[tag]["counts"]
            same = (gt.cpu().numpy() == fg[:n]) & (eq.cpu().numpy() == fe[:n])
            res["agreement"][tag] = {"queries": int(n), "identical_share": float(same.mean()),
                                     "max_abs_rank_difference": int(np.abs((gt + eq).cpu().numpy() - (fg[:n] + fe[:n])).max())}
            r = regions(lambda: torch_counts(filtered), tev, tel, 1, n_regions=3)
            r["chunk"] = args.torch_chunk
            res["torch"][tag] = r
            res.setdefault("fused_over_torch_time", {})[tag] = fused[tag]["ms"] / r["ms"]
            res.setdefault("fused_not_slower", {})[tag] = bool(fused[tag]["ms"] <= r["ms"])
    for r in fused.values():
        gt, eq = r.pop("counts")
        r["mean_rank"] = float(np.mean(1 + gt + eq))
        r["ties_total"] = int(eq.sum())
    res["fused"] = fused
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
