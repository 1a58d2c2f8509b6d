"""Recorder of the step schedule: which entry points of the library a model calls, in which order, through the eager pass, the
capture pass and the replays of every step form (host-fed step, device step, multi-step graphs, epoch reset).

    python tests/golden/make_step_traces.py          # on the GPU; writes tests/golden/step_schedule_traces.json

tests/test_step_schedule_gpu.py replays the same scenarios and compares.  The traces hold NAMES only (plus the row split of every
gather share), so they pin launch order, graph lengths and the shares per launch -- not the arithmetic, which the parity tests
pin.  Regenerate only when a schedule change is intended, and say so in the commit.

What is logged:  every graphsage_amd.ops.call / _lib.call by entry-point name (the *_destroy calls come from finalizers and are
dropped; so are the *_bytes size queries, which launch nothing and of which ops caches one per process, so that it would appear
only in the first scenario a process runs), "graph.launch" for every ops.Graph.launch, "hook" for every call of the model's grad_hook, and
"split:<rows of the largest job>:<frac>:<head rows>:<tail rows>" for every ops.split_gather_jobs.

Shapes: the smallest that still take the default kernels -- a reddit_shaped graph of 6,000 nodes, F = 64, dims 128 / 128,
fan-out 25 x 10, C = 41; supervised B = 256 (2,816 layer-0 rows), unsupervised B = 128 with 20 negatives (3,036 rows): both above
the tiled path's 2,048-row threshold.  One supervised scenario runs B = 64 (704 rows: the stream path)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TRACE_FILE = os.path.join(HERE, "step_schedule_traces.json")
DROPPED = ("gs_stream_destroy", "gs_graph_destroy", "gs_event_destroy")

F, DIM, C, FANOUT, N_NODES = 64, 128, 41, (25, 10), 6000
B_SUP, B_UNSUP, N_NEG = 256, 128, 20


# ---------------------------------------------------------------------------------------------------- the recorder
class Recorder(object):
    """Context manager: patches the four logging points, restores them on exit; `.events` is the trace."""

    def __init__(self):
        self.events = []

    def __enter__(self):
        from graphsage_amd import _lib, ops
        self._saved = (_lib.call, ops.call, ops.Graph.launch, ops.split_gather_jobs)
        raw_call, _, raw_launch, raw_split = self._saved
        ev = self.events

        def call(name, *args):
            if name not in DROPPED and not name.endswith("_bytes"):
                ev.append(name)
            return raw_call(name, *args)

        def launch(graph, *a, **kw):
            ev.append("graph.launch")
            return raw_launch(graph, *a, **kw)

        def split(jobs, frac):
            head, tail = raw_split(jobs, frac)
            big = max(jobs, key=lambda j: j.n * j.s).n if jobs else 0
            ev.append("split:%d:%s:%d:%d" % (big, repr(round(float(frac), 6)), sum(j.n for j in head), sum(j.n for j in tail)))
            return head, tail

        _lib.call = ops.call = call
        ops.Graph.launch = launch
        ops.split_gather_jobs = split
        return self

    def __exit__(self, *exc):
        from graphsage_amd import _lib, ops
        _lib.call, ops.call, ops.Graph.launch, ops.split_gather_jobs = self._saved
        return False

    def hook(self, capturable):
        ev = self.events

        class Hook(object):
            def __call__(self, model):
                ev.append("hook")
        Hook.capturable = capturable
        return Hook()


# ---------------------------------------------------------------------------------------------------- run-length coding
def encode(seq, max_period=96):
    """[symbol | [count, [block]]]: greedy; at every position the (period, repeats) pair that saves the most symbols."""
    out, i, n = [], 0, len(seq)
    while i < n:
        best = (0, 1, 1)
        for L in range(1, min(max_period, (n - i) // 2) + 1):
            reps = 1
            while seq[i + reps * L: i + (reps + 1) * L] == seq[i: i + L]:
                reps += 1
            if L * (reps - 1) > best[0]:
                best = (L * (reps - 1), L, reps)
        saved, L, reps = best
        if saved >= 2:
            out.append([reps, encode(seq[i: i + L], max_period)])
            i += L * reps
        else:
            out.append(seq[i])
            i += 1
    return out


def decode(code):
    out = []
    for item in code:
        if isinstance(item, list):
            out.extend(decode(item[1]) * item[0])
        else:
            out.append(item)
    return out


def pack(traces):
    symbols = sorted({s for t in traces.values() for s in t})
    index = {s: i for i, s in enumerate(symbols)}
    return {"symbols": symbols, "scenarios": {k: encode([index[s] for s in t]) for k, t in traces.items()}}


def unpack(doc):
    return {k: [doc["symbols"][i] for i in decode(code)] for k, code in doc["scenarios"].items()}


# ---------------------------------------------------------------------------------------------------- models
_GRAPH = {}


def graph():
    """The graph and its two iterators, built once per process."""
    if not _GRAPH:
        from graphsage_amd.minibatch import EdgeMinibatchIterator, NodeMinibatchIterator
        from graphsage_amd.utils import reddit_shaped
        G = reddit_shaped(avg_degree=10, seed=5, n_nodes=N_NODES, feat_dim=F, num_classes=C)
        np.random.seed(7)            # EdgeMinibatchIterator permutes edges with the global NumPy RNG
        _GRAPH["G"] = G
        _GRAPH["nodes"] = NodeMinibatchIterator(G, None, placeholders(False), None, G.num_classes, batch_size=B_SUP, max_degree=25)
        _GRAPH["edges"] = EdgeMinibatchIterator(G, None, placeholders(True), context_pairs=None, batch_size=B_UNSUP, max_degree=25)
    return _GRAPH["G"], _GRAPH["nodes"], _GRAPH["edges"]


def placeholders(unsup):
    from graphsage_amd.models import Placeholder
    names = ("batch1", "batch2", "neg_samples") if unsup else ("labels", "batch")
    ph = {k: Placeholder(k) for k in names + ("batch_size",)}
    ph["dropout"] = Placeholder("dropout", 0.)
    return ph


def make_model(unsup, agg="mean", identity_dim=0, loss_fn="xent", weight_decay=0.0):
    from graphsage_amd import engine as eng
    from graphsage_amd import inits
    from graphsage_amd.models import SAGEInfo, SampleAndAggregate
    from graphsage_amd.neigh_samplers import AdjInfo, CSRAdjacency, UniformNeighborSampler
    from graphsage_amd.supervised_models import SupervisedGraphsage
    G, nodes, edges = graph()
    eng.reset_engine()
    inits.set_seed(7)
    e = eng.get_engine()
    it = edges if unsup else nodes
    adj_info = AdjInfo(CSRAdjacency(it.train_csr[0], it.train_csr[1], G.n_nodes, e.device))
    sampler = UniformNeighborSampler(adj_info)
    mult = 2 if agg == "gcn" else 1                   # the drivers double the GCN widths (supervised_train.py:175-176)
    layer_infos = [SAGEInfo("node", sampler, FANOUT[i], mult * DIM) for i in range(2)]
    ph = placeholders(unsup)
    if unsup:
        model = SampleAndAggregate(ph, G.padded_features(), adj_info, it.deg, layer_infos, concat=(agg != "gcn"),
                                   aggregator_type=agg, learning_rate=0.01, weight_decay=weight_decay, neg_sample_size=N_NEG,
                                   loss_fn=loss_fn)
    else:
        model = SupervisedGraphsage(G.num_classes, ph, G.padded_features(), adj_info, it.deg, layer_infos, concat=(agg != "gcn"),
                                    aggregator_type=agg, sigmoid_loss=False, learning_rate=0.01, weight_decay=weight_decay,
                                    identity_dim=identity_dim)
    return model, ph, it


def _loss(out):
    return float(out[0])


def run_supervised(rec, agg="mean", B=B_SUP, B_change=None, dropout=0.0, hook=None, attrs=(), **model_kw):
    """The base sequence on a SupervisedGraphsage; returns (fetched losses, parameters)."""
    model, ph, it = make_model(False, agg, **model_kw)
    for k, v in attrs:
        setattr(model, k, v)
    if hook is not None:
        model.grad_hook = rec.hook(hook == "capturable")
    rng = np.random.RandomState(3)
    order = it.train_nodes.astype(np.int32)

    def feed(train):
        b = rng.choice(it.train_nodes, size=B, replace=False).astype(np.int32)
        fd = {ph['batch']: b, ph['labels']: it.label_matrix[b], ph['batch_size']: B}
        if train and dropout:
            fd[ph['dropout']] = dropout
        return fd

    losses = [_loss(model.train_step(feed(True))), _loss(model.eval_step(feed(False)))]
    ph['dropout'].value = dropout                       # (the validation feed left it at 0)
    model.attach_device_epoch(order, it.label_matrix)
    sizes = (B, B, B) if B_change is None else (B, B_change, B)
    for n in sizes:
        losses.append(_loss(model.train_step_device(n, fetch=True)))
    model.train_steps_device(B, 7, steps_per_launch=4)          # lengths 4, 2 and a single step
    losses.append(_loss(model._fetch(B)))
    model.set_epoch_order(order[::-1].copy())
    model.train_steps_device(B, 4, steps_per_launch=4)
    losses.append(_loss(model._fetch(B)))
    return losses, [model.engine.params.cpu().numpy().copy()]


def run_unsupervised(rec, agg="mean", B=B_UNSUP, B_change=None, hook=None, **model_kw):
    model, ph, it = make_model(True, agg, **model_kw)
    if hook is not None:
        model.grad_hook = rec.hook(hook == "capturable")
    rng = np.random.RandomState(3)
    pairs = np.ascontiguousarray(it.train_edges, dtype=np.int32)

    def feed():
        e = pairs[rng.choice(len(pairs), size=B, replace=False)]
        return {ph['batch1']: e[:, 0], ph['batch2']: e[:, 1], ph['batch_size']: B}

    losses = [_loss(model.train_step(feed())), _loss(model.eval_step(feed()))]
    model.attach_device_pairs(pairs)
    sizes = (B, B, B) if B_change is None else (B, B_change, B)
    for n in sizes:
        losses.append(_loss(model.train_step_device(n, fetch=True)))
    model.train_steps_device(B, 7, steps_per_launch=4)
    losses.append(_loss(model._fetch_unsup(B, with_outputs=False)))
    model.set_epoch_pairs(pairs[::-1].copy())
    model.train_steps_device(B, 4, steps_per_launch=4)
    losses.append(_loss(model._fetch_unsup(B, with_outputs=False)))
    return losses, [model.engine.params.cpu().numpy().copy()]


def run_node2vec(rec):
    from graphsage_amd import engine as eng
    from graphsage_amd.models import Node2VecModel
    G, nodes, edges = graph()
    eng.reset_engine()
    ph = placeholders(True)
    model = Node2VecModel(ph, G.n_nodes + 1, edges.deg, nodevec_dim=2 * DIM, lr=0.1, neg_sample_size=N_NEG)
    model.attach_device_pairs(np.ascontiguousarray(edges.train_edges, dtype=np.int32))
    out = model.train_steps_device(128, 5, steps_per_launch=2, fetch=True)
    return [_loss(out)], list(model.tables())


SCENARIOS = {
    "sup_mean": (run_supervised, {}),
    "sup_gcn": (run_supervised, dict(agg="gcn", weight_decay=1e-4)),
    "sup_maxpool": (run_supervised, dict(agg="maxpool")),
    "sup_mean_dropout": (run_supervised, dict(dropout=0.1)),
    "sup_mean_no_pipeline": (run_supervised, dict(attrs=(("pipeline", False),))),
    "sup_mean_identity8": (run_supervised, dict(identity_dim=8)),
    "sup_mean_tail_split": (run_supervised, dict(attrs=(("tail_split", True),))),
    "sup_mean_no_rides": (run_supervised, dict(attrs=(("sampler_rides", False),))),
    "sup_mean_sampler_in_wgrad": (run_supervised, dict(attrs=(("sampler_in_wgrad", True),))),
    "sup_mean_batch_change": (run_supervised, dict(B_change=128)),
    "sup_mean_b64": (run_supervised, dict(B=64)),
    "unsup_mean_xent": (run_unsupervised, {}),
    "unsup_mean_hinge": (run_unsupervised, dict(loss_fn="hinge")),
    "unsup_gcn": (run_unsupervised, dict(agg="gcn", weight_decay=1e-4)),
    "unsup_maxpool": (run_unsupervised, dict(agg="maxpool")),
    "unsup_mean_batch_change": (run_unsupervised, dict(B_change=64)),
    "sup_mean_hook": (run_supervised, dict(hook="eager")),
    "sup_mean_hook_capturable": (run_supervised, dict(hook="capturable")),
    "unsup_mean_hook": (run_unsupervised, dict(hook="eager")),
    "unsup_mean_hook_capturable": (run_unsupervised, dict(hook="capturable")),
    "node2vec": (run_node2vec, {}),
}


def record(name):
    """(trace, fetched losses, [parameter arrays]) of one scenario."""
    fn, kw = SCENARIOS[name]
    graph()                      # (built outside the recorder: its CSR construction calls the library too)
    with Recorder() as rec:
        losses, params = fn(rec, **kw)
    return rec.events, losses, params


def main():
    sys.path.append(os.path.dirname(os.path.dirname(HERE)))
    traces = {}
    for name in SCENARIOS:
        traces[name] = record(name)[0]
        print("%-28s %5d events" % (name, len(traces[name])), flush=True)
    doc = pack(traces)
    assert unpack(doc) == traces
    with open(TRACE_FILE, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (TRACE_FILE, os.path.getsize(TRACE_FILE)))


if __name__ == "__main__":
    main()
