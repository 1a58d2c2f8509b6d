"""Generate tests/golden/ref_full_{gcn,maxpool,meanpool_sigmoid,unsup_mean}.npz by EXECUTING THE REFERENCE'S OWN SOURCE with
`num_samples == [max_degree] * 2`.

    python tests/golden/make_ref_fullnbr_fixtures.py          # needs the reference's sources (see make_ref_fixtures.py)

Same machinery as make_ref_fixtures.py (imported as a module, its cases untouched).  With num_samples == max_degree at every
layer the reference's sampler (neigh_samplers.py:24-29) returns a PERMUTATION of each row of the padded adjacency table, and
mean / max / the GCN mean are symmetric in their arguments: the reference's forward pass then IS the full-neighborhood pass
over the multigraph whose row v is adj[v] -- pad row N included, whose neighbors are [N] * max_degree.  These runs pin
graphsage_amd.inference (FullGraph.from_padded, infer_full, embed_full, predict_full) against the reference's own numbers.

The supervised cases run two batches, so that step 1 is a pin under TRAINED weights: after one Adam step the pooling MLP's
bias is +-0.01 and the pad row's hidden state relu(0 . W + b) is no longer zero.

Only what an inference pin reads is kept: the per-variable gradients and the parameters after the last step are dropped
before saving (the pooling MLPs make them most of the bytes).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]

import make_ref_fixtures as mrf  # noqa: E402

SUP_CASES = {
    "full_gcn": dict(aggregator_type="gcn", concat=False, sigmoid=False, num_samples=[5, 5], dim=8, max_degree=5,
                     batch_size=16, batches=[list(range(18, 31)), list(range(41, 49))], weight_decay=0.005,
                     learning_rate=0.01, seed=41, np_seed=141),
    "full_maxpool": dict(aggregator_type="maxpool", concat=True, sigmoid=False, num_samples=[3, 3], dim=16, max_degree=3,
                         batch_size=16, batches=[list(range(10, 22)), list(range(50, 59))], weight_decay=0.01,
                         learning_rate=0.01, seed=42, np_seed=142),
    "full_meanpool_sigmoid": dict(aggregator_type="meanpool", concat=True, sigmoid=True, num_samples=[6, 6], dim=16,
                                  max_degree=6, batch_size=16, batches=[list(range(0, 10)), list(range(60, 72))],
                                  weight_decay=0.0, learning_rate=0.01, seed=43, np_seed=143),
}
UNSUP_CASES = {
    # embedding width 2 * 32 = 64; 30 pairs in batches of 12: three steps
    "full_unsup_mean": dict(aggregator_type="mean", concat=True, num_samples=[4, 4], dim=32, max_degree=4, batch_size=12,
                            n_pairs=30, neg_sample_size=6, weight_decay=0.01, learning_rate=0.01, seed=44, np_seed=144),
}
NAMES = list(SUP_CASES) + list(UNSUP_CASES)


def trim(out):
    last = int(out["n_steps"]) - 1
    for k in list(out):
        if "/grad/" in k or k.startswith("s%d/32/after/" % last) or k.startswith("s%d/64/after/" % last):
            del out[k]
    return out


def run_case(name):
    sup = name in SUP_CASES
    cfg = (SUP_CASES if sup else UNSUP_CASES)[name]
    assert cfg["num_samples"] == [cfg["max_degree"]] * len(cfg["num_samples"])
    out = {"cfg": np.asarray(json.dumps(dict(cfg, kind="supervised" if sup else "unsupervised")))}
    for real in ("float32", "float64"):
        (mrf.run_supervised if sup else mrf.run_unsupervised)(cfg, real, out)
    assert int(out["n_steps"]) >= 2
    return trim(out)


def main():
    torch.set_num_threads(1)           # one summation order: a re-run reproduces every array bit for bit
    only = set(sys.argv[1:])
    for name in NAMES:
        if only and name not in only:
            continue
        mrf.save(name, run_case(name))


if __name__ == "__main__":
    main()
