"""Downstream node classification on saved embeddings, with the three arguments of the reference's eval_scripts/
(reddit_eval.py, ppi_eval.py, citation_eval.py):

    python -m graphsage_amd.eval_embeddings DATA_PREFIX EMBED_DIR {val,test}

DATA_PREFIX names the dataset as --train_prefix does (<prefix>-G.json for the val / test flags, -id_map.json,
-class_map.json); EMBED_DIR is a log directory of unsupervised_train (val.npy / val.txt, and val-test.npy / val-test.txt where
the node2vec baseline wrote them: the test rows then come from that table).  A logistic regression is fitted on the train
nodes' embeddings on the device (graphsage_amd.evaluation) and scored on the val or test nodes; the `Downstream classifier:`
line is printed and written to EMBED_DIR/eval_classifier.txt.  The reference's raw-feature baseline (`feat`) is not provided.
"""
from __future__ import print_function

import argparse


def build_flags(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("data_prefix", help="prefix of the dataset files, as --train_prefix")
    p.add_argument("embed_dir", help="directory holding val.npy / val.txt")
    p.add_argument("setting", choices=["val", "test"], help="the split to score on")
    p.add_argument("--table", default="val", help="name of the table to fit on (val, or val_full from --full_inference)")
    return p.parse_args(argv)


def main(argv=None):
    flags = build_flags(argv)
    if flags.embed_dir == "feat":
        raise SystemExit("the raw-feature baseline (feat) of the reference's scripts is not provided")
    from . import evaluation, utils
    print("Loading data...")
    G = utils.load_data(flags.data_prefix, normalize=False)
    evaluation.refuse_graph(G)
    print("Running regression..")
    return evaluation.evaluate_embedding_dir(None, G, flags.embed_dir, flags.setting, base=flags.table)


if __name__ == "__main__":
    main()
