"""Downstream classifier at the Reddit and PPI shapes: one loss-and-gradient evaluation of the fused kernel (csrc/gs_logreg.hip,
through ops.logreg_eval) next to an eager torch restatement on the same device, and the whole fit next to scikit-learn's
SGDClassifier on the CPU where scikit-learn imports.

    python benchmarks/bench_eval.py [--shapes reddit,ppi] [--fit_rows 20000] [--out profiles/eval_classifier.json]

Shapes (train rows n of a table of N rows, width d, classes c): reddit = 153,431 of 232,965 x 256, 41 classes (multiclass);
ppi = 44,906 of 56,944 x 256, 121 labels (multi-label).  Embeddings are synthetic unit rows with labels from a noisy
linear model.  Prints one JSON line (and writes it to --out):
  * "fused": time of one ops.logreg_eval in FIT mode (torch events around --reps calls on the current stream, median / min /
    max of 5 regions, after a warm-up call), both launches included; the rate of the 4 n d c FLOP of the two contractions and
    the bytes of gathered rows per second.
  * "torch": the same evaluation as a user without the kernel would write it: Xg = X[rows]; Z = Xg @ W + b;
    loss = softplus(-S * Z).sum(0); R = -S * sigmoid(-S * Z); gW = Xg.T @ R; gb = R.sum(0)   (fp32, S = +-1 made once).
  * "fit": evaluation.fit_classifier on the whole shape: evaluations, stop reason, seconds.
  * "sklearn": SGDClassifier(loss="log_loss") (one-vs-rest; MultiOutputClassifier for multi-label) on the first --fit_rows
    train rows on the CPU, and fit_classifier on the same rows, when scikit-learn imports; else null.

    python benchmarks/bench_eval.py --joined all [--chunked_lib benchmarks/variants/_lib/libgs_logreg_chunked.so]

measures the joined inputs instead (gs_logreg_eval_joined, profiles/eval_classifier_features.md), all at the Reddit shape:
d256 = the embeddings alone through gs_logreg_eval and gs_logreg_eval_joined in one process (alternating regions),
features = 604 standardised feature columns, both = 604 + 256, d1024 = 604 + 420; each next to the eager restatement
(materialised hstack, standardise, two matmuls), gs_col_moments, and with --chunked_lib the column-chunked form of the kernel.
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

SHAPES = {"reddit": dict(N=232965, n=153431, d=256, c=41, multi=False),
          "ppi": dict(N=56944, n=44906, d=256, c=121, multi=True)}


def regions(fn, reps, n_regions=5):
    ms = []
    for _ in range(n_regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return {"ms": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}


def problem(shape, dev, seed=0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    N, n, d, c = shape["N"], shape["n"], shape["d"], shape["c"]
    X = torch.randn(N, d, device=dev, generator=g)
    X /= X.norm(dim=1, keepdim=True)
    Wt = torch.randn(d, c, device=dev, generator=g) * 3
    rows = torch.randperm(N, device=dev, generator=g)[:n].to(torch.int32)
    Z = X[rows.long()] @ Wt + torch.randn(n, c, device=dev, generator=g) * 0.6
    y = (Z > 0.3).to(torch.uint8) if shape["multi"] else Z.argmax(1).to(torch.int32)
    return X, rows, y


def bench_shape(name, shape, args, dev):
    from graphsage_amd import evaluation as ev
    from graphsage_amd import ops
    X, rows, y = problem(shape, dev)
    n, d, c, multi = shape["n"], shape["d"], shape["c"], shape["multi"]
    table = ops.Mat(X, d)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    W = ops.Mat(torch.randn(d, ops.round_up(c, 4), device=dev, generator=g) * 0.5, c)
    b = torch.zeros(c, device=dev)
    loss = torch.zeros(c, dtype=torch.float64, device=dev)
    gW = torch.zeros((d, c), dtype=torch.float64, device=dev)
    gb = torch.zeros(c, dtype=torch.float64, device=dev)
    ws = torch.empty(ops.logreg_ws_bytes(n, d, c) // 4, dtype=torch.float32, device=dev)
    labels = dict(y_multi=y) if multi else dict(y_class=y)

    def fused():
        ops.logreg_eval(table, W, b, n=n, rows=rows, loss=loss, gW=gW, gb=gb, ws=ws, **labels)

    S = (y.float() * 2 - 1) if multi else (torch.nn.functional.one_hot(y.long(), c).float() * 2 - 1)
    rows64, Wv = rows.long(), W.view()
    out = {}

    def eager():
        Xg = X[rows64]
        M = S * (Xg @ Wv + b)
        out["loss"] = torch.nn.functional.softplus(-M).sum(0)
        R = -S * torch.sigmoid(-M)
        out["gW"], out["gb"] = Xg.t() @ R, R.sum(0)

    fused()
    eager()
    torch.cuda.synchronize()
    agree = float((gW.float() - out["gW"]).abs().max() / max(1.0, float(gW.abs().max())))
    res = {"n": n, "d": d, "c": c, "multi": multi, "fused": regions(fused, args.reps), "torch": regions(eager, args.reps),
           "max_rel_diff_gW": agree}
    res["fused"]["tflops"] = 4.0 * n * d * c / (res["fused"]["ms"] * 1e-3) / 1e12
    res["fused"]["row_gbytes_per_s"] = 4.0 * n * d / (res["fused"]["ms"] * 1e-3) / 1e9
    res["speedup_vs_torch"] = res["torch"]["ms"] / res["fused"]["ms"]

    y_host, rows_host = y.cpu().numpy(), rows.cpu().numpy()
    kw = {} if multi else {"n_classes": c}
    t0 = time.time()
    clf = ev.fit_classifier(None, table, rows_host, y_host, **kw)
    res["fit"] = {"evals": clf.evals, "stop": clf.stop, "seconds": time.time() - t0}

    res["sklearn"] = None
    try:
        from sklearn.linear_model import SGDClassifier
        from sklearn.multioutput import MultiOutputClassifier
    except ImportError:
        return res
    m = min(args.fit_rows, n)
    Xs, ys = X[rows64[:m]].cpu().numpy(), y_host[:m]
    np.random.seed(1)
    sgd = MultiOutputClassifier(SGDClassifier(loss="log_loss")) if multi else SGDClassifier(loss="log_loss")
    t0 = time.time()
    sgd.fit(Xs, ys)
    t_sk = time.time() - t0
    t0 = time.time()
    sub = ev.fit_classifier(None, table, rows_host[:m], ys, **kw)
    t_dev = time.time() - t0
    Sm = ev.targets(ys, None if multi else c)[0]
    if multi:
        coef = np.stack([e.coef_[0] for e in sgd.estimators_], axis=1)
        icpt = np.array([e.intercept_[0] for e in sgd.estimators_])
    else:
        coef, icpt = sgd.coef_.T, sgd.intercept_
    res["sklearn"] = {"rows": m, "sgd_seconds": t_sk, "device_seconds": t_dev, "device_evals": sub.evals, "device_stop": sub.stop,
                      "objective_sgd_sum": float(ev.objective(Xs, Sm, coef, icpt).sum()),
                      "objective_device_sum": float(ev.objective(Xs, Sm, sub.W, sub.b).sum())}
    return res


# (da, db) of the joined inputs at the Reddit shape: the embeddings alone through both entry points, the 602 feature columns
# (604 padded), features + embeddings, and the widest row the kernel takes
JOINED = {"d256": (256, 0), "features": (604, 0), "both": (604, 256), "d1024": (604, 420)}


def bench_joined(name, da, db, args, dev, chunked=None):
    """One FIT evaluation of gs_logreg_eval_joined on standardised [A | B] rows at the Reddit shape (153,431 of 232,965 rows,
    41 classes), next to gs_logreg_eval where the shape allows it (d256: one table, no scaler -- the same arithmetic), the
    column-chunked build (--chunked_lib) and an eager restatement (materialised hstack, standardise, two matmuls)."""
    import ctypes
    from graphsage_amd import _lib, ops
    shape = SHAPES["reddit"]
    N, n, c = shape["N"], shape["n"], shape["c"]
    d = da + db
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    A = torch.randn(N, da, device=dev, generator=g)
    plain = db == 0 and d <= ops.LOGREG_MAX_D
    if plain:
        A /= A.norm(dim=1, keepdim=True)                        # an embedding table: unit rows, no scaler
    else:
        A = A * torch.exp(torch.rand(da, device=dev, generator=g) * 5.0 - 1.6) + (torch.rand(da, device=dev, generator=g) - 0.5) * 100
    B = None
    if db:
        B = torch.randn(N, db, device=dev, generator=g)
        B /= B.norm(dim=1, keepdim=True)
    Xa, Xb = ops.Mat(A, da), (ops.Mat(B, db) if db else None)
    rows_a = torch.randperm(N, device=dev, generator=g)[:n].to(torch.int32)
    rows_b = torch.randperm(N, device=dev, generator=g)[:n].to(torch.int32) if db else None
    y = torch.randint(0, c, (n,), device=dev, generator=g).to(torch.int32)
    W = ops.Mat(torch.randn(d, ops.round_up(c, 4), device=dev, generator=g) / d ** 0.5, c)
    b = torch.zeros(c, device=dev)
    mu = inv = None
    res = {"n": n, "da": da, "db": db, "c": c}
    if not plain:
        t0 = time.time()
        mean, var = ops.col_moments(Xa, Xb=Xb, n=n, rows_a=rows_a, rows_b=rows_b)
        torch.cuda.synchronize()
        res["col_moments_first_call_s"] = time.time() - t0
        res["col_moments"] = regions(lambda: ops.col_moments(Xa, Xb=Xb, n=n, rows_a=rows_a, rows_b=rows_b, mean=mean, var=var), 2)
        scale = torch.where(var == 0, torch.ones_like(var), var.sqrt())
        mu, inv = mean.float().contiguous(), (1.0 / scale).float().contiguous()
    loss = torch.zeros(c, dtype=torch.float64, device=dev)
    gW = torch.zeros((d, c), dtype=torch.float64, device=dev)
    gb = torch.zeros(c, dtype=torch.float64, device=dev)
    ws = torch.empty(ops.logreg_joined_ws_bytes(n, d, c) // 4, dtype=torch.float32, device=dev)

    def joined():
        ops.logreg_eval_joined(Xa, W, b, Xb=Xb, n=n, rows_a=rows_a, rows_b=rows_b, mu=mu, inv=inv, y_class=y, loss=loss, gW=gW,
                               gb=gb, ws=ws)

    joined()
    torch.cuda.synchronize()
    want = [t.clone() for t in (loss, gW, gb)]
    res["joined"] = regions(joined, args.reps)
    res["joined"]["tflops"] = 4.0 * n * d * c / (res["joined"]["ms"] * 1e-3) / 1e12
    res["joined"]["row_gbytes_per_s"] = 4.0 * n * d / (res["joined"]["ms"] * 1e-3) / 1e9
    if plain:
        def single():
            ops.logreg_eval(Xa, W, b, n=n, rows=rows_a, y_class=y, loss=loss, gW=gW, gb=gb, ws=ws)
        single()
        torch.cuda.synchronize()
        res["bit_equal_to_logreg_eval"] = all(torch.equal(a, b_) for a, b_ in zip(want, (loss, gW, gb)))
        # alternate the two entry points: the run-to-run spread of each is visible next to their difference
        res["logreg_eval"], res["joined_again"] = regions(single, args.reps), regions(joined, args.reps)
        res["logreg_eval_again"] = regions(single, args.reps)
    if chunked is not None:
        q = _lib.LogregJoinedDesc()
        q.Xa, q.rows_a, q.lda, q.n_rows_a, q.da = Xa.ptr, rows_a.data_ptr(), Xa.ld, Xa.rows, da
        if db:
            q.Xb, q.rows_b, q.ldb, q.n_rows_b, q.db = Xb.ptr, rows_b.data_ptr(), Xb.ld, Xb.rows, db
        if mu is not None:
            q.mu, q.inv = mu.data_ptr(), inv.data_ptr()
        q.W, q.b, q.y_class, q.loss, q.gW, q.gb, q.ws = W.ptr, b.data_ptr(), y.data_ptr(), loss.data_ptr(), gW.data_ptr(), \
            gb.data_ptr(), ws.data_ptr()
        q.n, q.ldw, q.ws_bytes, q.c, q.mode = n, W.ld, 4 * ws.numel(), c, ops.LOGREG_FIT
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def chunk():
            rc = chunked.gs_logreg_eval_joined_chunked(ctypes.addressof(q), stream)
            assert rc == 0, rc

        for t in (loss, gW, gb):
            t.zero_()
        chunk()
        torch.cuda.synchronize()
        res["chunked_bit_equal"] = all(torch.equal(a, b_) for a, b_ in zip(want, (loss, gW, gb)))
        res["chunked"], res["joined_after_chunked"] = regions(chunk, args.reps), regions(joined, args.reps)
    S = torch.nn.functional.one_hot(y.long(), c).float() * 2 - 1
    ra, rb, Wv = rows_a.long(), (rows_b.long() if db else None), W.view()
    out = {}

    def eager():
        Xg = torch.hstack([A[ra], B[rb]]) if db else A[ra]
        if mu is not None:
            Xg = (Xg - mu) * inv
        M = S * (Xg @ Wv + b)
        out["loss"] = torch.nn.functional.softplus(-M).sum(0)
        R = -S * torch.sigmoid(-M)
        out["gW"], out["gb"] = Xg.t() @ R, R.sum(0)

    eager()
    torch.cuda.synchronize()
    res["max_rel_diff_gW"] = float((want[1].float() - out["gW"]).abs().max() / max(1.0, float(want[1].abs().max())))
    res["torch"] = regions(eager, max(2, args.reps // 2))
    res["speedup_vs_torch"] = res["torch"]["ms"] / res["joined"]["ms"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="reddit,ppi")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fit_rows", type=int, default=20000)
    ap.add_argument("--out", default="")
    ap.add_argument("--joined", default="", help="comma list of %s (or 'all'): the joined-input measurements instead of --shapes"
                    % ",".join(JOINED))
    ap.add_argument("--chunked_lib", default="", help="library built by benchmarks/variants/build_logreg_chunked.sh: the "
                    "column-chunked form of the joined kernel is timed next to the library's")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_eval.py needs the GPU"
    dev = torch.device("cuda:0")
    if args.joined:
        import ctypes
        from graphsage_amd import _lib
        _lib.load()                                  # torch's HIP runtime first, then the product library, then the variant
        chunked = ctypes.CDLL(args.chunked_lib) if args.chunked_lib else None
        if chunked is not None:                      # without argtypes ctypes passes a Python int as a C int: half an address
            chunked.gs_logreg_eval_joined_chunked.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            chunked.gs_logreg_eval_joined_chunked.restype = ctypes.c_int
        names = list(JOINED) if args.joined == "all" else args.joined.split(",")
        res = {name: bench_joined(name, JOINED[name][0], JOINED[name][1], args, dev, chunked) for name in names}
    else:
        res = {name: bench_shape(name, SHAPES[name], args, dev) for name in args.shapes.split(",")}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
