"""Generate tests/golden/ref_{sup_twomaxpool,sup_twomaxpool_big_sigmoid,unsup_twomaxpool,full_twomaxpool}[_pN].npz by EXECUTING THE
REFERENCE'S OWN TwoMaxLayerPoolingAggregator (aggregators.py:276-361).

    python tests/golden/make_ref_twomax_fixtures.py          # needs the reference's sources (see make_ref_fixtures.py)

Same machinery as make_ref_fixtures.py (imported as a module, its cases untouched).  The reference's dispatch
(models.py:211-222, supervised_models.py:34-45) never selects this class, so for the duration of a case it is bound in
place of MaxPoolingAggregator in those two modules, at run time, and the case runs with aggregator_type "maxpool"; the
fixture's cfg says "twomaxpool".  Further:
  * named_variables names both Dense layers of the aggregator (agg%d/mlp_weights, mlp_bias, mlp2_weights, mlp2_bias);
  * the [hid1, hid2] arrays (mlp2_weights: gradients, post-Adam values) of the float64 twin, and of the "big" case in both
    precisions, are stored as seq_oracle.sketch() parts (row sums, column sums, 2048 fixed entries).  Everything else is kept
    in full: ref_sup_twomaxpool holds the float32 gradient of both layers' mlp2_weights;
  * no committed file may exceed 1 MiB, and one step's arrays are several: a fixture is written as ref_<name>.npz plus
    ref_<name>_p1.npz, _p2 ... (arrays in sorted order, a new part whenever the next array would not fit; an array larger than
    a part is cut along its rows into `key@@0`, `key@@1` ...).  twomax_oracle.Fixture reads the parts back as one fixture;
  * full_twomaxpool (num_samples == [max_degree] * 2, two batches) is trimmed like make_ref_fullnbr_fixtures.trim.
The seeds are chosen so that in the float64 run every positive maximum of the pooled second layer leads the best row of a
different node id by more than 1e-5 (tests/test_ref_twomax.py asserts it).
"""
import contextlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import make_ref_fixtures as mrf  # noqa: E402
from seq_oracle import sketch  # noqa: E402

import graphsage.models as ref_models  # noqa: E402
import graphsage.supervised_models as ref_supervised_models  # noqa: E402
from graphsage.aggregators import TwoMaxLayerPoolingAggregator  # noqa: E402

tf = mrf.tf


@contextlib.contextmanager
def twomax_bound():
    saved = ref_models.MaxPoolingAggregator, ref_supervised_models.MaxPoolingAggregator
    ref_models.MaxPoolingAggregator = ref_supervised_models.MaxPoolingAggregator = TwoMaxLayerPoolingAggregator
    try:
        yield
    finally:
        ref_models.MaxPoolingAggregator, ref_supervised_models.MaxPoolingAggregator = saved


def named_variables(model, supervised):
    out = {}
    for i, a in enumerate(model.aggregators):
        for k, v in a.vars.items():
            out["agg%d/%s" % (i, k)] = v
        mlp = getattr(a, "mlp_layers", [])
        assert len(mlp) == 2
        for tag, layer in (("mlp", mlp[0]), ("mlp2", mlp[1])):
            out["agg%d/%s_weights" % (i, tag)] = layer.vars['weights']
            out["agg%d/%s_bias" % (i, tag)] = layer.vars['bias']
    if supervised:
        out["node_pred/weights"] = model.node_pred.vars['weights']
        out["node_pred/bias"] = model.node_pred.vars['bias']
    assert model.embeds is None
    assert set(map(id, out.values())) == set(map(id, tf.trainable_variables())), "unnamed trainable variable"
    return out


mrf.named_variables = named_variables

SUP_CASES = {
    # weight_decay > 0 pins that neither Dense layer takes any
    "sup_twomaxpool": dict(aggregator_type="twomaxpool", concat=True, sigmoid=False, num_samples=[4, 3], dim=16, max_degree=8,
                           batch_size=16, batches=[list(range(10, 22))], weight_decay=0.01, learning_rate=0.01, seed=41,
                           np_seed=141, eval_nodes=[0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 71]),
    # FLAGS.model_size = "big": 1024 / 512
    "sup_twomaxpool_big_sigmoid": dict(aggregator_type="twomaxpool", concat=True, sigmoid=True, num_samples=[3, 2], dim=16,
                                       max_degree=6, batch_size=16, batches=[list(range(25, 36))], weight_decay=0.01,
                                       learning_rate=0.01, seed=102, np_seed=202, model_size="big"),
}
UNSUP_CASES = {
    # embedding width 2 * 32 = 64: the device's link-prediction launch takes d in {64, 128, 256, 512}; 16 pairs = two steps
    "unsup_twomaxpool": dict(aggregator_type="twomaxpool", concat=True, num_samples=[3, 2], dim=32, max_degree=6, batch_size=8,
                             n_pairs=16, neg_sample_size=4, weight_decay=0.005, learning_rate=0.01, seed=104, np_seed=204),
}
FULL_CASES = {
    "full_twomaxpool": dict(aggregator_type="twomaxpool", concat=True, sigmoid=False, num_samples=[3, 3], dim=16, max_degree=3,
                            batch_size=16, batches=[list(range(10, 22)), list(range(50, 59))], weight_decay=0.01,
                            learning_rate=0.01, seed=45, np_seed=145),
}
NAMES = list(SUP_CASES) + list(UNSUP_CASES) + list(FULL_CASES)

PART_BYTES = 900 * 1024        # raw bytes of the arrays of one file (compressed: less; the limit for a committed file is 1 MiB)


def compact(name, out):
    """The mlp2_weights-shaped gradients and post-Adam values of the float64 twin -- and of the big case in both precisions --
    become sketches."""
    big = "big" in name
    for k in list(out):
        parts = k.split("/")
        if len(parts) == 5 and parts[2] in ("grad", "after") and parts[4] == "mlp2_weights" and (parts[1] == "64" or big):
            for part, v in sketch(out.pop(k)).items():
                out["%s#%s" % (k, part)] = v
    return out


def save_parts(name, out):
    """ref_<name>.npz, ref_<name>_p1.npz ...: see the module docstring."""
    items = []
    for k in sorted(out):
        a = np.asarray(out[k])
        if a.nbytes > PART_BYTES:
            rows = max(1, PART_BYTES // (a.nbytes // a.shape[0]))
            for j, r0 in enumerate(range(0, a.shape[0], rows)):
                items.append(("%s@@%d" % (k, j), a[r0:r0 + rows]))
        else:
            items.append((k, a))
    files, used = [{}], 0
    for k, a in items:
        if used + a.nbytes > PART_BYTES and files[-1]:
            files.append({})
            used = 0
        files[-1][k] = a
        used += a.nbytes
    files[0]["n_parts"] = np.asarray(len(files))
    for i, f in enumerate(files):
        mrf.save(name if i == 0 else "%s_p%d" % (name, i), f)


def trim_full(out):
    """make_ref_fullnbr_fixtures.trim: an inference pin reads no gradient and no parameter after the last step."""
    last = int(out["n_steps"]) - 1
    for k in list(out):
        if "/grad/" in k or k.startswith("s%d/32/after/" % last) or k.startswith("s%d/64/after/" % last):
            del out[k]
    return out


def run_case(name):
    sup = name in SUP_CASES or name in FULL_CASES
    cfg = SUP_CASES.get(name) or UNSUP_CASES.get(name) or FULL_CASES[name]
    out = {"cfg": np.asarray(json.dumps(dict(cfg, kind="supervised" if sup else "unsupervised")))}
    ref_cfg = dict(cfg, aggregator_type="maxpool")            # what the reference's dispatch is asked for
    with twomax_bound():
        for real in ("float32", "float64"):
            (mrf.run_supervised if sup else mrf.run_unsupervised)(ref_cfg, real, out)
    if name in FULL_CASES:
        assert cfg["num_samples"] == [cfg["max_degree"]] * len(cfg["num_samples"]) and int(out["n_steps"]) >= 2
        out = trim_full(out)
    return compact(name, out)


def main():
    torch.set_num_threads(1)           # one summation order: a re-run reproduces every array bit for bit
    only = set(sys.argv[1:])
    for name in NAMES:
        if only and name not in only:
            continue
        save_parts(name, run_case(name))


if __name__ == "__main__":
    main()
