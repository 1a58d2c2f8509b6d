"""Generate tests/golden/ref_unsup_{hinge,skipgram,hinge_bilinear,xent_bilinear}.npz by EXECUTING THE REFERENCE'S OWN
BipartiteEdgePredLayer with loss_fn / bilinear_weights other than what models.py:363-366 hard-codes.

    python tests/golden/make_ref_linkpred_fixtures.py          # needs /root/reference (or $GRAPHSAGE_REFERENCE)

Same machinery as make_ref_fixtures.py (imported as a module, its cases untouched), with two additions:
  * for the duration of a case the NAME BipartiteEdgePredLayer in the reference's `models` module is bound to a
    functools.partial that forces the case's loss_fn / bilinear_weights over the hard-coded arguments (the class itself, and
    every line of the reference, run unmodified; nothing of it is stored);
  * named_variables also names the bilinear matrix (edge_predict/weights): it is trainable but lives in no aggregator.
The hinge cases must keep every entry of n_ij - a_i + margin at least 1e-3 away from 0 (the subgradient jumps there: a 1e-4
float difference must not flip a mask) with at least 20 % of the entries active and 20 % inactive, on both legs and every
step -- asserted below; the seeds were chosen so that the reference's run satisfies it.
"""
import functools
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import make_ref_fixtures as mrf  # noqa: E402
import graphsage.models as ref_models  # noqa: E402
from linkpred_oracle import hinge_terms  # noqa: E402

_named_variables = mrf.named_variables
_RefLayer = ref_models.BipartiteEdgePredLayer
MARGIN = 0.1             # prediction.py:32


def named_variables(model, supervised):
    layer = getattr(model, "link_pred_layer", None)
    w = layer.vars.get("weights") if layer is not None else None
    if w is None:
        return _named_variables(model, supervised)
    trainable = mrf.tf.trainable_variables
    mrf.tf.trainable_variables = lambda: [v for v in trainable() if v is not w]
    try:
        out = _named_variables(model, supervised)
    finally:
        mrf.tf.trainable_variables = trainable
    out["edge_predict/weights"] = w
    assert set(map(id, out.values())) == set(map(id, trainable())), "unnamed trainable variable"
    return out


mrf.named_variables = named_variables


def _forced(cls, forced, *args, **kwargs):
    kwargs.update(forced)
    return cls(*args, **kwargs)


def check_hinge(name, out, n_steps):
    for s in range(n_steps):
        for pre in ("32", "64"):
            t = hinge_terms(out["s%d/%s/aff_all" % (s, pre)], MARGIN)
            active = float((t > 0).mean())
            assert np.abs(t).min() >= 1e-3, (name, s, pre, float(np.abs(t).min()))
            assert 0.2 <= active <= 0.8, (name, s, pre, active)


_BASE = dict(aggregator_type="mean", concat=True, num_samples=[3, 2], dim=32, max_degree=6, batch_size=8, n_pairs=16,
             neg_sample_size=4, learning_rate=0.01)
CASES = {
    # embedding width 2 * 32 = 64; two steps of 8 pairs; weight_decay > 0 in the bilinear cases pins that W takes none
    "unsup_hinge": dict(_BASE, loss_fn="hinge", bilinear_weights=False, weight_decay=0.0, seed=33, np_seed=133),
    "unsup_skipgram": dict(_BASE, loss_fn="skipgram", bilinear_weights=False, weight_decay=0.0, seed=32, np_seed=132),
    "unsup_hinge_bilinear": dict(_BASE, loss_fn="hinge", bilinear_weights=True, weight_decay=0.005, seed=35, np_seed=135),
    "unsup_xent_bilinear": dict(_BASE, loss_fn="xent", bilinear_weights=True, weight_decay=0.005, seed=34, np_seed=134),
}


def run_case(name, cfg):
    out = {"cfg": np.asarray(json.dumps(dict(cfg, kind="unsupervised")))}
    forced = dict(loss_fn=cfg["loss_fn"], bilinear_weights=cfg["bilinear_weights"])
    ref_models.BipartiteEdgePredLayer = functools.partial(_forced, _RefLayer, forced)
    try:
        for real in ("float32", "float64"):
            mrf.run_unsupervised(cfg, real, out)
    finally:
        ref_models.BipartiteEdgePredLayer = _RefLayer
    assert ("init/edge_predict/weights" in out) == cfg["bilinear_weights"]
    if cfg["loss_fn"] == "hinge":
        check_hinge(name, out, int(out["n_steps"]))
    return out


def main():
    torch.set_num_threads(1)           # one summation order: a re-run reproduces every array bit for bit
    only = set(sys.argv[1:])
    for name, cfg in CASES.items():
        if only and name not in only:
            continue
        mrf.save(name, run_case(name, cfg))


if __name__ == "__main__":
    main()
