"""Step time of the node2vec baseline (models.Node2VecModel, csrc/gs_n2v.hip): d = 256, B = 512, 20 distinct negatives, on a
Reddit-shaped table (N = 232,965 rows) and an RMAT-sized one (10^7 rows), device-resident pairs, steps replayed as
multi-step captured graphs.

    python benchmarks/bench_n2v.py [--steps 400] [--steps_per_launch 8] [--out profiles/n2v_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o n2v -- python benchmarks/bench_n2v.py --hip_only --configs reddit

Prints one JSON line (and writes it to --out): per configuration us per step and pairs per second of the three-launch HIP step
(HIP events on the engine stream around each region of --steps steps, median of 5 regions), and -- as the yardstick -- a
plain eager torch restatement of the same step (index_select, matmul, index_add_) on the same device and the same id batches
(torch events on torch's stream, same number of steps, median of 5).  The step moves about 1 MB each way and is launch- and
latency-bound, so the bar is only that the HIP step is not slower than the eager one; `hip_not_slower` records it.
The degrees are heavy-tailed (Zipf-like) and the pairs are drawn degree-weighted, like random-walk co-occurrences: hubs
repeat within a batch and meet the negatives.
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

CONFIGS = {"reddit": 232965, "rmat": 10 ** 7}


def synthetic_degrees(n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    u = torch.rand(n, device="cuda", generator=g, dtype=torch.float64)
    return torch.clamp((u ** -0.8).floor(), max=20000.0)             # Pareto tail, minimum 1


def synthetic_pairs(deg, n_pairs, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed + 1)
    cdf = torch.cumsum(deg, 0)
    r = torch.rand(2 * n_pairs, device="cuda", generator=g, dtype=torch.float64) * cdf[-1]
    ids = torch.searchsorted(cdf, r).clamp(max=deg.numel() - 1)
    return ids.view(n_pairs, 2).to(torch.int32)


def torch_step(T, C, bias, ids, B, n_neg, lr):
    """The same step in eager torch: what a user without the kernels would write."""
    b1, b2, neg = ids[:B].long(), ids[B:2 * B].long(), ids[2 * B:].long()
    o1, o2, no = T.index_select(0, b1), C.index_select(0, b2), C.index_select(0, neg)
    aff = (o1 * o2).sum(1)
    nav = o1 @ no.t()
    affb, navb = aff + bias[b2], nav + bias[neg]
    loss = (torch.nn.functional.softplus(-affb).sum() + torch.nn.functional.softplus(navb).sum()) / B
    aff_all = torch.cat([nav, aff[:, None]], 1)
    mrr = (1.0 / (1.0 + (nav >= aff[:, None]).sum(1))).mean()
    da = (torch.sigmoid(affb) - 1.0) / B
    gq = torch.sigmoid(navb) / B
    g_t = da[:, None] * o2 + gq @ no
    g_c = da[:, None] * o1
    g_n = gq.t() @ o1
    T.index_add_(0, b1, g_t, alpha=-lr)
    C.index_add_(0, b2, g_c, alpha=-lr)
    C.index_add_(0, neg, g_n, alpha=-lr)
    bias.index_add_(0, b2, da, alpha=-lr)
    bias.index_add_(0, neg, gq.sum(0), alpha=-lr)
    return loss, mrr, aff_all, o1


def run_config(name, n_rows, args):
    from graphsage_amd import engine as eng
    from graphsage_amd import ops
    from graphsage_amd.models import Node2VecModel, Placeholder
    B, d, n_neg, lr = 512, 256, 20, 0.025
    eng.reset_engine()
    e = eng.get_engine()
    t0 = time.time()
    deg = synthetic_degrees(n_rows, 123)
    pairs = synthetic_pairs(deg, args.pairs, 123)
    ph = {k: Placeholder(k) for k in ("batch1", "batch2", "batch_size", "dropout")}
    model = Node2VecModel(ph, n_rows + 1, deg.cpu().numpy(), nodevec_dim=d, lr=lr, neg_sample_size=n_neg, device_init=True)
    model.attach_device_pairs(pairs.cpu().numpy())
    setup_s = time.time() - t0
    spl, steps = args.steps_per_launch, args.steps
    out = {"rows": n_rows, "d": d, "B": B, "n_neg": n_neg, "steps": steps, "steps_per_launch": spl, "setup_s": round(setup_s, 1)}
    if not args.hip_only:
        # the yardstick first, on copies of the initial tables and the id batches the HIP path will stage (cursor s * B,
        # clock s): staged here by the same kernel
        T, C, bias = model.target_embeds.clone(), model.context_embeds.clone(), model.context_bias.clone()
        batches = []
        cur = torch.zeros(1, dtype=torch.int64, device=e.device)
        clk = torch.zeros(1, dtype=torch.int64, device=e.device)
        for s in range(steps):
            ids = torch.zeros(2 * B + n_neg, dtype=torch.int32, device=e.device)
            cur.fill_(s * B)
            clk.fill_(s)
            torch.cuda.synchronize()
            ops.call("gs_n2v_stage", ops.ptr(model._pairs), model._pairs.shape[0], ops.ptr(cur), B, ops.ptr(model._neg_cdf),
                     model._n_cdf, n_neg, model.neg_seed, ops.ptr(clk), 0, ops.ptr(model._neg_guide), model._guide_bits,
                     ops.ptr(ids), None, e.stream)
            e.sync()
            batches.append(ids)
        for ids in batches[:10]:
            torch_step(T, C, bias, ids, B, n_neg, lr)
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for ids in batches:
                torch_step(T, C, bias, ids, B, n_neg, lr)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / steps)
        out["torch_eager_us_per_step"] = float(np.median(ms)) * 1e3
        out["torch_eager_us_per_step_min"] = float(np.min(ms)) * 1e3
        del T, C, bias
    model.train_steps_device(B, 2 * spl, steps_per_launch=spl)       # eager, then captured
    rem = steps % spl
    if rem:
        model.train_steps_device(B, 2 * rem, steps_per_launch=rem)
    e.sync()
    ms = []
    for _ in range(5):
        a, b = ops.Event(), ops.Event()
        a.record(e.stream)
        model.train_steps_device(B, steps, steps_per_launch=spl)
        b.record(e.stream)
        e.sync()
        ms.append(a.elapsed_ms(b) / steps)
    loss, _, _, mrr, _ = model.train_steps_device(B, 0, fetch=True)
    us = float(np.median(ms)) * 1e3
    out.update(hip_us_per_step=us, hip_us_per_step_min=float(np.min(ms)) * 1e3, hip_pairs_per_s=B / (us * 1e-6),
               loss=loss, mrr=mrr)
    if "torch_eager_us_per_step" in out:
        out["hip_not_slower"] = bool(us <= out["torch_eager_us_per_step"])
        out["speedup_vs_torch_eager"] = out["torch_eager_us_per_step"] / us
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--steps_per_launch", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=2000000)
    ap.add_argument("--configs", default="reddit,rmat")
    ap.add_argument("--hip_only", action="store_true", help="skip the torch yardstick (kernel-trace runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_n2v.py needs the GPU"
    res = {"metric": "node2vec baseline training step (stage | forward + gradient rows | sparse SGD apply), d 256, batch 512, "
                     "20 distinct negatives",
           "basis": "hipEventElapsedTime on the engine stream around each %d-step region of %d-step graph replays, median "
                    "of 5; torch eager: torch events around the same number of steps, median of 5" % (args.steps, args.steps_per_launch)}
    for name in args.configs.split(","):
        res[name] = run_config(name, CONFIGS[name], args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
