"""graphsage_twomaxpool (the two-layer max-pooling aggregator): the new backward kernel against the launches it replaces, and
the whole training step next to graphsage_maxpool.  bench.py's model table does not list the model, so this script times it.

    python benchmarks/bench_twomax.py [--steps 20] [--warmup 10] [--nodes 232965] [--skip_step] [--skip_kernel] [--models a,b]

(a) kernel level, the layer-0 shapes of the headline fan-out (512 groups of 10 and 5120 groups of 25, hid1 / hid2 = 512 / 256),
    H1 one row per sampled row and H1 one row per distinct id read through an index (63 % distinct, Reddit's share):
      pool2_dgrad  gs_pool2_transpose (W2 -> W2^T, once per backward pass) + gs_pool2_dgrad_t
      composed     gs_segment_max_bwd + gs_dense_dgrad + gs_act_bwd (+ gs_gather_rows of H1 in the indexed form)
    medians over 30 launches between HIP events after 5 warm-up launches, one process; the bytes the fused form must move (the
    [n s, hid1] store and the H1 read) over its time is printed as a rate.
(b) step level: Reddit-shaped supervised step (B = 512, 25 x 10, F = 602, dims 128 / 128), device-resident epoch, captured graphs:
    us per step of graphsage_twomaxpool with fuse_dgrad on and off, and of graphsage_maxpool, from the same process.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_us(fn, stream, reps=30, warmup=5):
    from graphsage_amd import ops
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(ops.Event(), ops.Event()) for _ in range(reps)]
    for a, b in evs:
        a.record(stream)
        fn()
        b.record(stream)
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_ms(b) * 1e3 for a, b in evs)
    return float(np.median(ts)), float(ts[0])


def kernel_level(dev):
    from graphsage_amd import ops
    from graphsage_amd.ops import Mat
    st = ops.Stream()
    s_ = st.handle
    g = torch.Generator(device="cpu").manual_seed(0)
    hid1, hid2 = 512, 256
    out = {}
    W2 = Mat((torch.randn((hid1, hid2), generator=g) / 16).to(dev), hid2)
    W2T = Mat.zeros(hid2, hid1, dev)
    for n, s in ((512, 10), (5120, 25)):
        rows = n * s
        arg = torch.randint(0, s, (n, hid2), generator=g, dtype=torch.int32).to(dev)
        dpm = torch.randn((n, hid2), generator=g)
        dpm[torch.rand((n, hid2), generator=g) < 0.5] = 0.0
        dpm = Mat(dpm.to(dev), hid2)
        pooled = Mat(torch.ones((n, hid2), device=dev), hid2)
        dH1, dH2 = Mat.zeros(rows, hid1, dev), Mat.zeros(rows, hid2, dev)
        for form in ("rows", "indexed"):
            n_h = rows if form == "rows" else int(0.63 * rows)
            H1 = Mat(torch.randn((n_h, hid1), generator=g).to(dev), hid1)
            idx = None if form == "rows" else torch.randint(0, n_h, (rows,), generator=g, dtype=torch.int32).to(dev)
            H1x = Mat.zeros(rows, hid1, dev) if idx is not None else H1

            def fused():
                ops.pool2_transpose(W2, W2T, stream=s_)
                ops.pool2_dgrad(dpm, arg, H1, idx, n, s, dH1, W2T=W2T, stream=s_)

            def fused_kernel_only():
                ops.pool2_dgrad(dpm, arg, H1, idx, n, s, dH1, W2T=W2T, stream=s_)

            def composed():
                ops.segment_max_bwd(dpm, pooled, arg, n, s, dH2, stream=s_)
                ops.dense_dgrad(dH2, 0, hid2, rows, W2, dH1, stream=s_)
                if idx is not None:
                    ops.gather_rows(H1, idx, out=H1x, stream=s_)
                ops.act_bwd(dH1, H1x, rows, hid1, ops.ACT_RELU, dH1, stream=s_)

            composed()
            torch.cuda.synchronize()
            want = dH1.numpy().copy()
            fused()
            torch.cuda.synchronize()
            got = dH1.numpy()
            err = float(np.abs(got - want).max())
            f_med, f_min = _median_us(fused, s_)
            k_med, _ = _median_us(fused_kernel_only, s_)
            c_med, c_min = _median_us(composed, s_)
            moved = rows * hid1 * 4 * 2                      # the dH1 store + the H1 read (one row per stored row)
            out["%dx%d_%s" % (n, s, form)] = {
                "pool2_dgrad_us": f_med, "pool2_dgrad_min_us": f_min, "pool2_dgrad_kernel_only_us": k_med,
                "composed_us": c_med, "composed_min_us": c_min, "speedup": c_med / f_med,
                "store_plus_mask_read_GBps": moved / (k_med * 1e-6) / 1e9, "max_abs_diff_vs_composed": err,
                "flops_fused": 2.0 * n * hid2 * hid1 * 0.5, "flops_composed": 2.0 * rows * hid2 * hid1}
    return out


def step_level(args, dev):
    from graphsage_amd import engine as eng
    from graphsage_amd import ops
    from graphsage_amd.models import Placeholder, SAGEInfo
    from graphsage_amd.neigh_samplers import AdjInfo, CSRAdjacency, UniformNeighborSampler
    from graphsage_amd.supervised_models import SupervisedGraphsage
    from graphsage_amd.utils import reddit_shaped_device
    B, S1, S2, DIM, F, C = 512, 25, 10, 128, 602, 41
    DG = reddit_shaped_device(dev, n_nodes=args.nodes, feat_dim=F, num_classes=C, avg_degree=args.avg_degree, seed=123)
    out = {}
    for tag, agg, fuse in (("twomaxpool_pool2_dgrad", "twomaxpool", True), ("twomaxpool_composed", "twomaxpool", False),
                           ("maxpool", "maxpool", None)):
        if args.models and tag not in args.models.split(","):
            continue
        eng.reset_engine()
        e = eng.get_engine()
        adj_info = AdjInfo(CSRAdjacency.from_device(DG.train_csr[0], DG.train_csr[1], DG.n_nodes))
        sampler = UniformNeighborSampler(adj_info, seed=123, law="reference", max_degree=128)
        ph = {'labels': Placeholder('labels'), 'batch': Placeholder('batch1'), 'dropout': Placeholder('dropout', 0.),
              'batch_size': Placeholder('batch_size')}
        layer_infos = [SAGEInfo("node", sampler, S1, DIM), SAGEInfo("node", sampler, S2, DIM)]
        model = SupervisedGraphsage(DG.num_classes, ph, DG.feats, adj_info, DG.deg, layer_infos, concat=True,
                                    aggregator_type=agg, model_size="small", learning_rate=0.01, weight_decay=0.0)
        if fuse is not None:
            for a in model.aggregators:
                a.fuse_dgrad = fuse
        model.attach_device_epoch(np.random.RandomState(123).permutation(DG.train_nodes), DG.label_table)
        spl = args.steps_per_launch

        def run():
            model.train_steps_device(B, args.steps, steps_per_launch=spl)
        model.train_steps_device(B, max(args.warmup, 2 * spl + 2), steps_per_launch=spl)
        run()
        run()                                  # eager + capture of every graph length the timed call uses
        e.sync()
        evs = [(ops.Event(), ops.Event()) for _ in range(5)]
        for a, b in evs:
            a.record(e.stream)
            run()
            b.record(e.stream)
        torch.cuda.synchronize()
        us = np.asarray([a.elapsed_ms(b) for a, b in evs]) * 1e3 / args.steps
        loss, _ = model._fetch(B)
        a0 = model.aggregators[0]
        out[tag] = {"us_per_step": float(np.median(us)), "us_per_step_min": float(us.min()), "loss": float(loss),
                    "dgrad": getattr(a0, "last_dgrad_kernel", None), "pool_kernel": getattr(a0, "last_pool_kernel", None)}
        del model
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--avg_degree", type=int, default=492)
    ap.add_argument("--steps_per_launch", type=int, default=8)
    ap.add_argument("--skip_step", action="store_true")
    ap.add_argument("--skip_kernel", action="store_true")
    ap.add_argument("--models", default="", help="comma-separated subset of twomaxpool_pool2_dgrad,twomaxpool_composed,maxpool "
                                                 "(e.g. one model under rocprofv3 --kernel-trace)")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    t0 = time.time()
    res = {} if args.skip_kernel else {"kernel": kernel_level(dev)}
    if not args.skip_step:
        res["step"] = step_level(args, dev)
    res["basis"] = ("kernel: hipEventElapsedTime around each launch sequence, median of 30 after 5 warm-up launches; step: "
                    "around each %d-step region of captured graphs, median of 5, per step" % args.steps)
    res["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
