"""Generate tests/golden/ref_{sup_seq,sup_seq_big_sigmoid,unsup_seq}.npz by EXECUTING THE REFERENCE'S OWN SeqAggregator.

    python tests/golden/make_ref_seq_fixtures.py          # needs /root/reference (or $GRAPHSAGE_REFERENCE)

Same machinery as make_ref_fixtures.py (imported as a module, its cases untouched), with three additions:
  * tests/tf1_rnn.py installs BasicLSTMCell / dynamic_rnn on the TF1 stand-in (the LSTM of aggregators.py:363-449);
  * named_variables also names each layer's LSTM kernel and bias (agg%d/lstm_kernel, agg%d/lstm_bias): they are trainable
    but live in neither aggregator.vars nor the MLP layers, so they are added to the name table for the duration of the
    call (the reference's loss graph was built before and is not affected);
  * the LSTM kernels start on a 1/64 grid, and their gradients / post-Adam values are stored as sketches (row sums, column
    sums, 2048 fixed entries; tests/seq_oracle.py) -- the full arrays would exceed the size of a committed file;
  * make_graph zeroes the feature rows of two nodes that other nodes have as neighbors, so sampled sequences hold all-zero
    rows: each one lowers the sequence's length by one (aggregators.py:411-414) -- the zero row still runs if it lies within
    the first L steps, and the LAST steps are the ones dropped.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import make_ref_fixtures as mrf  # noqa: E402
import tf1_rnn  # noqa: E402
from seq_oracle import sketch  # noqa: E402

tf = tf1_rnn.install(mrf.tf)

_named_variables = mrf.named_variables
_make_graph = mrf.make_graph


def named_variables(model, supervised):
    added = []
    for a in model.aggregators:
        cell = getattr(a, "cell", None)
        if cell is not None and cell.kernel is not None:
            with torch.no_grad():       # initial kernel on a 1/64 grid (exact in fp32; keeps the fixture small)
                cell.kernel.value.copy_(torch.round(cell.kernel.value * 64) / 64)
            a.vars["lstm_kernel"], a.vars["lstm_bias"] = cell.kernel, cell.bias
            added.append(a)
    try:
        return _named_variables(model, supervised)
    finally:
        for a in added:
            del a.vars["lstm_kernel"], a.vars["lstm_bias"]


def zeroed_nodes(G):
    """The two train nodes that the most other nodes have as (train) neighbors, lower id first on ties."""
    n = len(G.node)
    train = [i for i in range(n) if not (G.node[i]['val'] or G.node[i]['test'])]
    count = {i: sum(1 for v in G.neighbors(i) if not G[i][v]['train_removed']) for i in train}
    return sorted(train, key=lambda i: (-count[i], i))[:2]


def make_graph(*args, **kw):
    G, feats, single, multi = _make_graph(*args, **kw)
    feats = feats.copy()
    feats[zeroed_nodes(G)] = 0.0
    return G, feats, single, multi


_save = mrf.save


def save(name, out):
    """The LSTM kernels' gradients and post-Adam values ([neigh_in + H, 4H] per layer, step and precision: far beyond the size
    of a committed file) are stored as seq_oracle.sketch(): row sums, column sums, 2048 fixed entries."""
    for k in [k for k in out if k.endswith("/lstm_kernel") and ("/grad/" in k or "/after/" in k)]:
        for part, v in sketch(out.pop(k)).items():
            out["%s#%s" % (k, part)] = v
    _save(name, out)


mrf.named_variables = named_variables
mrf.make_graph = make_graph
mrf.save = save

SUP_CASES = {
    "sup_seq": dict(aggregator_type="seq", concat=True, sigmoid=False, num_samples=[4, 3], dim=16, max_degree=8,
                    batch_size=16, batches=[list(range(8, 22)), list(range(40, 51))], weight_decay=0.0,
                    learning_rate=0.01, seed=21, np_seed=121, eval_nodes=[0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 71]),
    # FLAGS.model_size = "big": the cell is 256 wide; weight decay > 0 pins that the LSTM variables take none
    "sup_seq_big_sigmoid": dict(aggregator_type="seq", concat=True, sigmoid=True, num_samples=[3, 2], dim=16, max_degree=6,
                                batch_size=16, batches=[list(range(25, 37))], weight_decay=0.01, learning_rate=0.01,
                                seed=22, np_seed=122, model_size="big"),
}
UNSUP_CASES = {
    # embedding width 2 * 32 = 64: the device's link-prediction launch takes d in {64, 128, 256, 512}
    "unsup_seq": dict(aggregator_type="seq", concat=True, num_samples=[3, 2], dim=32, max_degree=6, batch_size=8,
                      n_pairs=16, neg_sample_size=4, weight_decay=0.005, learning_rate=0.01, seed=23, np_seed=123),
}


def main():
    import json
    torch.set_num_threads(1)           # one summation order: a re-run reproduces every array bit for bit
    only = set(sys.argv[1:])
    for name, cfg in SUP_CASES.items():
        if only and name not in only:
            continue
        out = {"cfg": np.asarray(json.dumps(dict(cfg, kind="supervised")))}
        for real in ("float32", "float64"):
            mrf.run_supervised(cfg, real, out)
        mrf.save(name, out)
    for name, cfg in UNSUP_CASES.items():
        if only and name not in only:
            continue
        out = {"cfg": np.asarray(json.dumps(dict(cfg, kind="unsupervised")))}
        for real in ("float32", "float64"):
            mrf.run_unsupervised(cfg, real, out)
        mrf.save(name, out)


if __name__ == "__main__":
    main()
