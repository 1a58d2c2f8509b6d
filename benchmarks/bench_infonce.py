"""The in-batch softmax (InfoNCE) head alone -- the launches of gs_linkpred_infonce_fwd_bwd (csrc/gs_infonce.hip) -- against an
eager torch restatement (matmul + logsumexp + autograd) on the same device and the same normalised rows, at the unsupervised
benchmark shape (B = 512, n_neg = 20, d = 256) unless told otherwise.

    python benchmarks/bench_infonce.py [--B 512] [--n_neg 20] [--d 256] [--iters 2000] [--rounds 7]

Both sides are timed with device events around `iters` back-to-back calls on one stream (the head through its C entry point,
torch through its Python front end: its launch overhead is part of what a user of that path pays), the two alternated round
by round; the first round of each is warm-up.  Also prints the largest difference between the two sides' outputs.  One JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_head(U, Y2, NEG, ids1, ids2, tau, scale):
    """loss rows and the three gradients, eager: what the kernel replaces."""
    u, y2, neg = U.detach().requires_grad_(True), Y2.detach().requires_grad_(True), NEG.detach().requires_grad_(True)
    B = u.shape[0]
    L = (u @ torch.cat([y2, neg], dim=0).T) / tau
    m = (ids2[None, :] == ids2[:, None]) | (ids2[None, :] == ids1[:, None])
    m.fill_diagonal_(False)
    Lm = torch.cat([L[:, :B].masked_fill(m, float("-inf")), L[:, B:]], dim=1)
    rows = torch.logsumexp(Lm, dim=1) - torch.diagonal(L[:, :B])
    (rows.sum() * scale).backward()
    return rows.detach(), u.grad, y2.grad, neg.grad


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--n_neg", type=int, default=20)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--tau", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args(argv)
    from graphsage_amd import ops
    from graphsage_amd.ops import Mat
    dev = torch.device("cuda:0")
    B, nn, d, tau = args.B, args.n_neg, args.d, args.tau
    scale = 1.0 / B
    rng = np.random.RandomState(1)
    x = rng.randn(2 * B + nn, d)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    X = Mat.from_numpy(x, dev)
    ids1 = torch.from_numpy(rng.randint(0, 4 * B, size=B).astype(np.int32)).to(dev)
    ids2 = torch.from_numpy(rng.randint(0, 4 * B, size=B).astype(np.int32)).to(dev)
    U = X.rows_slice(0, B)
    dX = Mat.zeros(2 * B + nn, d, dev)
    loss_rows, rr = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    stats = torch.zeros(ops.linkpred_infonce_ws_floats(B, d, nn), device=dev)
    aff = Mat.zeros(B, nn + 1, dev)
    stream = ops.current_stream()

    def ours(train=True):
        ops.linkpred_infonce_fwd_bwd(X, U, B, nn, tau, scale, loss_rows, rr, aff, stats, dX=dX if train else None,
                                     dU=dX.rows_slice(0, B) if train else None, ids=(ids1, ids2), stream=stream)

    Xt = X.view()
    tU, tY2, tNEG = Xt[:B].contiguous(), Xt[B:2 * B].contiguous(), Xt[2 * B:].contiguous()

    def theirs():
        return torch_head(tU, tY2, tNEG, ids1, ids2, tau, scale)

    ours()
    rows_t, gu, gy2, gneg = theirs()
    torch.cuda.synchronize()
    diff = {"loss_rows": float((loss_rows - rows_t).abs().max()),
            "grads_over_scale_tau": float(max((dX.view()[:B] - gu).abs().max(), (dX.view()[B:2 * B] - gy2).abs().max(),
                                              (dX.view()[2 * B:] - gneg).abs().max()) * tau / scale)}

    def region(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters

    sides = [("hip_fwd_bwd", ours), ("hip_fwd_only", lambda: ours(False)), ("torch_eager_fwd_bwd", theirs)]
    us = {k: [] for k, _ in sides}
    for r in range(args.rounds + 1):
        for k, fn in sides:
            t = region(fn)
            if r:
                us[k].append(t)
    res = {k: {"us": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in us.items()}
    flops = 2.0 * B * (B + nn) * d * 3            # the score matrix and its two gradient contractions, once each
    print(json.dumps({"metric": "in-batch softmax head alone, B=%d n_neg=%d d=%d tau=%g, us per call" % (B, nn, d, tau),
                      "calls": res, "max_abs_diff_vs_torch": diff, "useful_flop": flops, "iters": args.iters, "rounds": args.rounds,
                      "basis": "device events around %d back-to-back calls on one stream, sides alternated, median of %d rounds "
                               "after one warm-up round" % (args.iters, args.rounds)}))


if __name__ == "__main__":
    main()
