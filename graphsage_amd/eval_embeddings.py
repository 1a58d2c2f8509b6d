"""Downstream node classification on saved embeddings, with the three arguments of the reference's eval_scripts/
(reddit_eval.py, ppi_eval.py, citation_eval.py):

    python -m graphsage_amd.eval_embeddings DATA_PREFIX EMBED_DIR {val,test} [--inputs {embeddings,features,both}] [--log_counts]

DATA_PREFIX names the dataset as --train_prefix does (<prefix>-G.json for the val / test flags, -id_map.json,
-class_map.json, -feats.npy); EMBED_DIR is a log directory of unsupervised_train (val.npy / val.txt, and val-test.npy /
val-test.txt where the node2vec baseline wrote them: the test rows then come from that table).  A logistic regression is
fitted on the train nodes' rows on the device (graphsage_amd.evaluation) and scored on the val or test nodes.

--inputs embeddings (the default): the rows are the embeddings as they are; the `Downstream classifier:` line is printed and
    written to EMBED_DIR/eval_classifier.txt.
--inputs features: the reference's raw-feature baseline (`feat`): the rows of <prefix>-feats.npy, standardised on the train
    rows.  EMBED_DIR need not hold val.npy; it receives eval_classifier_features.txt.
--inputs both: [features | embeddings] standardised on the train rows (the scripts' n2v branch) -> eval_classifier_both.txt.
--log_counts: the scripts' transform of feature columns 0 and 1 before anything else, log(f0 + 1) and
    log(f1 - min(min f1, -1)); needs --inputs features or both.
"""
from __future__ import print_function

import argparse


def build_flags(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("data_prefix", help="prefix of the dataset files, as --train_prefix")
    p.add_argument("embed_dir", help="directory holding val.npy / val.txt; receives the output file")
    p.add_argument("setting", choices=["val", "test"], help="the split to score on")
    p.add_argument("--table", default="val", help="name of the table to fit on (val, or val_full from --full_inference)")
    p.add_argument("--inputs", default="embeddings", choices=["embeddings", "features", "both"],
                   help="what a row is made of: the embeddings, the dataset's feature table, or [features | embeddings]")
    p.add_argument("--log_counts", action="store_true",
                   help="log(f0 + 1) and log(f1 - min(min f1, -1)) on feature columns 0 and 1 first (reddit_eval.py:46-47)")
    p.add_argument("--clusters", type=int, default=0,
                   help="K: instead of the regression, k-means of ALL rows of --table into K clusters on the device (-1: the "
                        "dataset's number of classes), scored against the class labels -> eval_clusters.txt, clusters.npy, "
                        "cluster_centers.npy; the setting is not used")
    p.add_argument("--clusters_seed", type=int, default=123, help="seed of the k-means++ seeding of --clusters")
    return p.parse_args(argv)


def log_counts(feats):
    """The reference's transform of the raw feature columns 0 and 1 (reddit_eval.py:46-47, ppi_eval.py:58-59), on a copy."""
    import numpy as np
    if feats.shape[1] < 2:
        raise SystemExit("--log_counts transforms feature columns 0 and 1; the table has %d" % feats.shape[1])
    feats = np.array(feats, dtype=np.float32)
    f0, f1 = feats[:, 0].astype(np.float64), feats[:, 1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        feats[:, 0] = np.log(f0 + 1.0)
        feats[:, 1] = np.log(f1 - min(float(f1.min()), -1.0))
    if not np.isfinite(feats[:, :2]).all():
        raise SystemExit("--log_counts: log(f0 + 1) or log(f1 - min(min f1, -1)) is not finite on this table (column 0 below "
                         "-1, or the minimum of column 1 below -1: the rule takes log(0) of that row)")
    return feats


def main(argv=None):
    flags = build_flags(argv)
    if flags.embed_dir == "feat":
        raise SystemExit("the raw-feature baseline (feat) is --inputs features with a directory for the output file")
    if flags.log_counts and flags.inputs == "embeddings":
        raise SystemExit("--log_counts transforms the feature table: it needs --inputs features or both")
    from . import evaluation, utils
    if flags.clusters:
        from . import clustering
        clustering.refuse_flags("--clusters", flags.clusters)
        print("Loading data...")
        G = utils.load_data(flags.data_prefix, normalize=False)
        clustering.refuse_flags("--clusters", flags.clusters, G=G)
        print("Running k-means..")
        return clustering.evaluate_embedding_dir(None, G, flags.embed_dir, flags.clusters, base=flags.table,
                                                 seed=flags.clusters_seed, flag="--clusters")
    print("Loading data...")
    G = utils.load_data(flags.data_prefix, normalize=False)
    evaluation.refuse_graph(G)
    features = None
    if flags.inputs != "embeddings":
        evaluation.refuse_inputs(flags.inputs, G.feats.shape[1] if G.feats is not None else None, None, G.feats is not None)
        features = log_counts(G.feats) if flags.log_counts else G.feats
    print("Running regression..")
    return evaluation.evaluate_embedding_dir(None, G, flags.embed_dir, flags.setting, base=flags.table, inputs=flags.inputs,
                                             features=features)


if __name__ == "__main__":
    main()
