"""graphsage_attn (the attention-pooling aggregator): its two segment launches alone, and the whole training step next to
graphsage_maxpool and graphsage_meanpool.  bench.py's model table does not list the model, so this script times it.

    python benchmarks/bench_attn.py [--steps 20] [--warmup 10] [--nodes 232965] [--skip_step] [--skip_kernel] [--models a,b]

(a) kernel level, the layer-0 shapes of the headline fan-out (512 groups of 10 and 5120 groups of 25, hidden = 512), H one row
    per sampled row and H one row per distinct id read through an index (63 % distinct, Reddit's share):
      gs_segment_attn_fwd                  must move the H rows it reads (one read of every row) + pooled + alpha
      gs_segment_attn_bwd                  at the slab counts the aggregator gives the two hops (11 / 52 of the gate's 64);
                                           must move the H rows + the dV store (its second pass re-reads rows it has just read)
    medians over 30 launches between HIP events after 5 warm-up launches, one process; those bytes over the time as a rate.
(b) step level: Reddit-shaped supervised step (B = 512, 25 x 10, F = 602, dims 128 / 128), device-resident epoch, captured graphs:
    us per step of graphsage_attn, graphsage_maxpool and graphsage_meanpool (whose unfused Dense + reduce path is the one the
    attention model shares), from the same process.

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


def layer0_slabs(shapes, free=64):
    """The aggregator's split of the gate's slabs among the hops of a layer (AttentionPoolingAggregator.backward_hops)."""
    roots = [(n * s) ** 0.5 for n, s in shapes]
    return [int(max(1, min(1 + int((free - len(shapes)) * r / sum(roots)), (n + 15) // 16))) for (n, s), r in zip(shapes, roots)]


def kernel_level(dev, slabs=0):
    from graphsage_amd import ops
    from graphsage_amd.ops import Mat
    st = ops.Stream()
    s_ = st.handle
    g = torch.Generator(device="cpu").manual_seed(0)
    hidden = 512
    out = {}
    a = (torch.randn(hidden, generator=g) / hidden ** 0.5).to(dev)
    shapes = ((512, 10), (5120, 25))
    counts = [slabs] * len(shapes) if slabs else layer0_slabs(shapes)
    slab_buf = torch.zeros(64 * hidden, device=dev)
    for (n, s), n_slabs in zip(shapes, counts):
        rows = n * s
        dP = Mat(torch.randn((n, hidden), generator=g).to(dev), hidden)
        pooled, dV = Mat.zeros(n, hidden, dev), Mat.zeros(rows, hidden, dev)
        alpha = torch.zeros(rows, device=dev)
        for form in ("rows", "indexed"):
            n_h = rows if form == "rows" else int(0.63 * rows)
            H = Mat(torch.relu(torch.randn((n_h, hidden), generator=g)).to(dev), hidden)
            idx = None if form == "rows" else torch.randint(0, n_h, (rows,), generator=g, dtype=torch.int32).to(dev)

            def fwd():
                ops.segment_attn_fwd(H, idx, a, n, s, pooled, alpha, stream=s_)

            def bwd():
                ops.segment_attn_bwd(dP, H, idx, a, alpha, n, s, dV, n_slabs, slab_buf.data_ptr(), stream=s_)

            f_med, f_min = _median_us(fwd, s_)
            b_med, b_min = _median_us(bwd, s_)
            h_bytes = n_h * hidden * 4 + (rows * 4 if idx is not None else 0)
            f_bytes = h_bytes + n * hidden * 4 + rows * 4
            b_bytes = h_bytes + rows * hidden * 4 + rows * 4 + n * hidden * 4
            out["%dx%d_%s" % (n, s, form)] = {
                "fwd_us": f_med, "fwd_min_us": f_min, "fwd_bytes": f_bytes, "fwd_GBps": f_bytes / (f_med * 1e-6) / 1e9,
                "bwd_us": b_med, "bwd_min_us": b_min, "bwd_bytes": b_bytes, "bwd_GBps": b_bytes / (b_med * 1e-6) / 1e9,
                "bwd_slabs": n_slabs}
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
    for agg in ("attn", "maxpool", "meanpool"):
        if args.models and agg not in args.models.split(","):
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
        out[agg] = {"us_per_step": float(np.median(us)), "us_per_step_min": float(us.min()), "loss": float(loss),
                    "pool_kernel": getattr(a0, "last_pool_kernel", None),
                    "distinct_ids": a0.last_unique is not None and int(a0.last_unique[0].item())}
        del model
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--avg_degree", type=int, default=492)
    ap.add_argument("--steps_per_launch", type=int, default=8)
    ap.add_argument("--bwd_slabs", type=int, default=0, help="slabs (= workgroups, at most 64) of gs_segment_attn_bwd at the kernel "
                                                             "level; 0 = what the aggregator gives each hop of the layer (11 / 52)")
    ap.add_argument("--skip_step", action="store_true")
    ap.add_argument("--skip_kernel", action="store_true")
    ap.add_argument("--models", default="", help="comma-separated subset of attn,maxpool,meanpool")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    t0 = time.time()
    res = {} if args.skip_kernel else {"kernel": kernel_level(dev, args.bwd_slabs)}
    if not args.skip_step:
        res["step"] = step_level(args, dev)
    res["basis"] = ("kernel: hipEventElapsedTime around each launch, median of 30 after 5 warm-up launches; step: around each "
                    "%d-step region of captured graphs, median of 5, per step" % args.steps)
    res["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
