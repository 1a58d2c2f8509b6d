"""Reddit-shaped supervised graphsage_seq (the LSTM aggregator) step time: BASELINE configs[1] shapes (N = 232,965, F = 602,
C = 41, fan-out 25 x 10, batch 512, dims 128 / 128, model_size "small": LSTM hidden 128), device-resident epoch, full training
step replayed as captured graphs.  bench.py's model table does not list graphsage_seq, so this script times it.

    python benchmarks/bench_seq.py [--steps 20] [--warmup 10] [--nodes 232965]

Prints one JSON line: ms/step (HIP events on the engine stream around the timed region), sampled edges/s, and -- as a
yardstick -- torch.nn.LSTM (MIOpen) forward + backward on the same three sequence batches as the step's two recurrence
launches (layer 0: 512 x 10 and 5120 x 25 sequences of 602-wide rows; layer 1: 512 x 10 of 256-wide rows).
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


def _events_ms(fn, reps, stream):
    from graphsage_amd import ops
    evs = [(ops.Event(), ops.Event()) for _ in range(reps)]
    for a, b in evs:
        a.record(stream)
        fn()
        b.record(stream)
    torch.cuda.synchronize()
    return [a.elapsed_ms(b) for a, b in evs]


def miopen_lstm_ms(batches, H, reps):
    """torch.nn.LSTM (cuDNN/MIOpen path on ROCm) forward + backward over each (n, T, D) batch, median ms per batch."""
    out = {}
    for n, T, D in batches:
        lstm = torch.nn.LSTM(D, H, batch_first=True).cuda()
        x = torch.randn(n, T, D, device="cuda", requires_grad=True)

        def fb():
            y, (h, c) = lstm(x)
            h.sum().backward()
        for _ in range(3):
            fb()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fb()
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e))
        out["%dx%dx%d" % (n, T, D)] = float(np.median(ts))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--avg_degree", type=int, default=492)
    ap.add_argument("--steps_per_launch", type=int, default=8)
    args = ap.parse_args(argv)
    from graphsage_amd import engine as eng
    from graphsage_amd.models import Placeholder, SAGEInfo
    from graphsage_amd.neigh_samplers import AdjInfo, CSRAdjacency, UniformNeighborSampler
    from graphsage_amd.supervised_models import SupervisedGraphsage
    from graphsage_amd.utils import reddit_shaped_device
    B, S1, S2, DIM, F, C = 512, 25, 10, 128, 602, 41
    t0 = time.time()
    dev = torch.device("cuda:0")
    DG = reddit_shaped_device(dev, n_nodes=args.nodes, feat_dim=F, num_classes=C, avg_degree=args.avg_degree, seed=123)
    eng.reset_engine()
    e = eng.get_engine()
    adj_info = AdjInfo(CSRAdjacency.from_device(DG.train_csr[0], DG.train_csr[1], DG.n_nodes))
    sampler = UniformNeighborSampler(adj_info, seed=123, law="reference", max_degree=128)
    ph = {'labels': Placeholder('labels'), 'batch': Placeholder('batch1'), 'dropout': Placeholder('dropout', 0.),
          'batch_size': Placeholder('batch_size')}
    layer_infos = [SAGEInfo("node", sampler, S1, DIM), SAGEInfo("node", sampler, S2, DIM)]
    model = SupervisedGraphsage(DG.num_classes, ph, DG.feats, adj_info, DG.deg, layer_infos, concat=True,
                                aggregator_type="seq", model_size="small", learning_rate=0.01, weight_decay=0.0)
    model.attach_device_epoch(np.random.RandomState(123).permutation(DG.train_nodes), DG.label_table)
    setup_s = time.time() - t0
    spl = args.steps_per_launch

    def run():
        model.train_steps_device(B, args.steps, steps_per_launch=spl)
    model.train_steps_device(B, max(args.warmup, 2 * spl + 2), steps_per_launch=spl)
    run()
    run()                                  # eager + capture of every graph length the timed call uses
    e.sync()
    ms = np.asarray(_events_ms(run, 5, e.stream)) / args.steps
    loss, _ = model._fetch(B)
    edges = B * (S2 + S2 * S1)
    H = model.aggregators[0].hidden_dim
    yard = miopen_lstm_ms([(B, S2, F), (B * S2, S1, F), (B, S2, 2 * DIM)], H, 10)
    print(json.dumps({
        "metric": "Reddit-shaped supervised graphsage_seq training step, fan-out %dx%d, batch %d, dims %d/%d, LSTM hidden %d"
                  % (S1, S2, B, DIM, DIM, H),
        "ms_per_step": float(np.median(ms)), "ms_per_step_min": float(ms.min()),
        "sampled_edges_per_s": edges / (float(np.median(ms)) * 1e-3), "edges_per_step": edges,
        "steps": args.steps, "steps_per_launch": spl, "loss": float(loss), "setup_s": round(setup_s, 1),
        "miopen_lstm_fwd_bwd_ms": yard, "miopen_lstm_fwd_bwd_ms_total": float(sum(yard.values())),
        "basis": "hipEventElapsedTime on the engine stream around each %d-step region, median of 5" % args.steps}))


if __name__ == "__main__":
    main()
