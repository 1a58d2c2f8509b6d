"""Reddit-shaped unsupervised graphsage_mean step time per link-prediction head: BASELINE configs[3] shapes (N = 232,965,
F = 602, fan-out 25 x 10, batch 512, dims 128 / 128 -> embedding width 256, 20 negatives), device-resident pairs, full
training steps replayed as captured graphs.  bench.py times the default head only (xent on the fused tail); this script times

    xent_fused_tail   the default (gs_linkpred_tail / gs_linkpred_tail_neg)
    xent_per_op       the same loss on the per-operator schedule (model.fuse_tail = False): the comparison point
    hinge, skipgram   gs_linkpred_loss_fwd_bwd on the per-operator schedule
    hinge_bilinear, xent_bilinear   + U = Y1 . W, dY1 = dU . W^T, dW = Y1^T . dU (three 512 x 256 x 256 products)
    infonce, infonce_bilinear       the in-batch softmax, gs_linkpred_infonce_fwd_bwd (normalise | [U = Y1 . W] | the head's
                      launches | [dY1 = dU . W^T] | normalisation backward); `hinge` is its yardstick: same schedule, the old head

in ONE process, alternating the configurations round by round (other work shares the machine: the spread of a
configuration over the rounds is printed next to its median).

    python benchmarks/bench_linkpred.py [--steps 200] [--rounds 7] [--heads hinge,infonce] [--md profiles/linkpred_losses.md]

Prints one JSON line; --md also writes the table.
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

CONFIGS = [
    ("xent_fused_tail", dict(), True),
    ("xent_per_op", dict(), False),
    ("hinge", dict(loss_fn="hinge"), True),
    ("skipgram", dict(loss_fn="skipgram"), True),
    ("hinge_bilinear", dict(loss_fn="hinge", bilinear_weights=True), True),
    ("xent_bilinear", dict(loss_fn="xent", bilinear_weights=True), True),
    ("infonce", dict(loss_fn="infonce"), True),
    ("infonce_bilinear", dict(loss_fn="infonce", bilinear_weights=True), True),
]


def build(DG, pairs, head, fuse_tail, args):
    from graphsage_amd import engine as eng
    from graphsage_amd.models import Placeholder, SAGEInfo, SampleAndAggregate
    from graphsage_amd.neigh_samplers import AdjInfo, CSRAdjacency, UniformNeighborSampler
    eng.reset_engine()                  # every model keeps the engine (stream, parameters, workspaces) it was built on
    e = eng.get_engine()
    adj_info = AdjInfo(CSRAdjacency.from_device(DG.train_csr[0], DG.train_csr[1], DG.n_nodes))
    sampler = UniformNeighborSampler(adj_info, seed=123, law="reference", max_degree=128)
    ph = {'batch1': Placeholder('batch1'), 'batch2': Placeholder('batch2'), 'neg_samples': Placeholder('neg'),
          'dropout': Placeholder('dropout', 0.), 'batch_size': Placeholder('batch_size')}
    layer_infos = [SAGEInfo("node", sampler, 25, 128), SAGEInfo("node", sampler, 10, 128)]
    model = SampleAndAggregate(ph, DG.feats, adj_info, DG.deg, layer_infos, concat=True, aggregator_type="mean",
                               learning_rate=0.00001, weight_decay=0.0, neg_sample_size=20, **head)
    model.fuse_tail = fuse_tail
    model.attach_device_pairs(pairs)
    return e, model


def region_ms(e, model, B, steps, spl):
    from graphsage_amd import ops
    a, b = ops.Event(), ops.Event()
    a.record(e.stream)
    model.train_steps_device(B, steps, steps_per_launch=spl)
    b.record(e.stream)
    e.sync()
    return a.elapsed_ms(b)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--avg_degree", type=int, default=492)
    ap.add_argument("--steps_per_launch", type=int, default=8)
    ap.add_argument("--md", default="", help="also write the table as markdown to this path")
    ap.add_argument("--heads", default="", help="comma-separated subset of the configurations (default: all; xent_per_op, the "
                                                "table's comparison point, is always among them)")
    args = ap.parse_args(argv)
    want = set(args.heads.split(",")) | {"xent_per_op"} if args.heads else None
    unknown = (want or set()) - {name for name, _, _ in CONFIGS}
    if unknown:
        ap.error("unknown heads: %s" % ", ".join(sorted(unknown)))
    configs = [c for c in CONFIGS if want is None or c[0] in want]
    from graphsage_amd.utils import random_walk_pairs_device, reddit_shaped_device
    B, spl = 512, args.steps_per_launch
    t0 = time.time()
    dev = torch.device("cuda:0")
    DG = reddit_shaped_device(dev, n_nodes=args.nodes, feat_dim=602, num_classes=41, avg_degree=args.avg_degree, seed=123)
    pairs = random_walk_pairs_device(DG.train_csr[0], DG.train_csr[1], DG.train_nodes, max_pairs=1000000, seed=123).cpu().numpy()
    models = []
    for name, head, fuse_tail in configs:
        e, model = build(DG, pairs, head, fuse_tail, args)
        # eager + capture of every graph length the timed call uses, then one untimed region
        model.train_steps_device(B, 2 * spl + 2, steps_per_launch=spl)
        for _ in range(2):
            model.train_steps_device(B, args.steps, steps_per_launch=spl)
        e.sync()
        assert bool(model._lp_tail_used) == (name == "xent_fused_tail"), name
        models.append((name, e, model))
    setup_s = time.time() - t0
    us = {name: [] for name, _, _ in models}
    for _ in range(args.rounds):                       # alternate: a drift of the machine hits every configuration alike
        for name, e, model in models:
            us[name].append(region_ms(e, model, B, args.steps, spl) * 1e3 / args.steps)
    res = {}
    for name, e, model in models:
        loss, _, _, mrr, _ = model._fetch_unsup(B, with_outputs=False)
        v = np.asarray(us[name])
        res[name] = {"us_per_step": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "loss": loss, "mrr": mrr}
    base = res["xent_per_op"]["us_per_step"]
    lines = ["| head | us/step (median of %d rounds x %d steps) | min .. max | vs xent per-operator |" % (args.rounds, args.steps),
             "|---|---|---|---|"]
    for name, _, _ in models:
        r = res[name]
        lines.append("| %s | %.1f | %.1f .. %.1f | %+.1f |" % (name, r["us_per_step"], r["min"], r["max"], r["us_per_step"] - base))
    table = "\n".join(lines)
    if args.md:
        with open(args.md, "w") as f:
            f.write(table + "\n")
    print(table, file=sys.stderr)
    print(json.dumps({
        "metric": "Reddit-shaped unsupervised graphsage_mean training step per link-prediction head, fan-out 25x10, batch 512, "
                  "dims 128/128, 20 negatives",
        "heads": res, "steps": args.steps, "rounds": args.rounds, "steps_per_launch": spl, "setup_s": round(setup_s, 1),
        "bilinear_cost_us": {k: res[k + "_bilinear"]["us_per_step"] - res["xent_per_op" if k == "xent" else k]["us_per_step"]
                             for k in ("hinge", "xent", "infonce")
                             if k + "_bilinear" in res and ("xent_per_op" if k == "xent" else k) in res},
        "basis": "hipEventElapsedTime on each model's engine stream around %d-step regions, configurations alternated, "
                 "median over %d rounds" % (args.steps, args.rounds)}))


if __name__ == "__main__":
    main()
