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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="reddit,ppi")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fit_rows", type=int, default=20000)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_eval.py needs the GPU"
    dev = torch.device("cuda:0")
    res = {name: bench_shape(name, SHAPES[name], args, dev) for name in args.shapes.split(",")}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
