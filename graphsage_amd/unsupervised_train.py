"""Unsupervised training driver with the flags, loop structure, log-line format and output files of
graphsage/unsupervised_train.py (flags :25-55, loop :246-316, save_val_embeddings :94-117), driving the MI355X engine.

    python -m graphsage_amd.unsupervised_train --train_prefix ./example_data/toy-ppi --model graphsage_mean --max_total_steps 1000
    python -m graphsage_amd.unsupervised_train --synthetic small --model graphsage_mean --epochs 1
    python -m graphsage_amd.unsupervised_train --synthetic small --model n2v --learning_rate 0.1

Models: graphsage_mean | gcn | graphsage_seq | graphsage_maxpool | graphsage_meanpool | graphsage_twomaxpool | graphsage_attn | n2v.  n2v is
the DeepWalk /
node2vec baseline (:227-232): after val.npy it retrains on random walks from the val / test nodes for --n2v_test_epochs
epochs and writes val-test.npy / val-test.txt (:322-372).
"""
from __future__ import division, print_function

import argparse
import os
import time

import numpy as np

seed = 123
np.random.seed(seed)
FLAGS = None


def build_flags(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    b = lambda v: str(v).lower() in ("1", "true", "yes")
    p.add_argument('--log_device_placement', type=b, default=False)
    p.add_argument('--model', default='graphsage', help='model names. See README for possible values.')
    p.add_argument('--learning_rate', type=float, default=0.00001, help='initial learning rate.')
    p.add_argument('--model_size', default='small', help="Can be big or small; model specific def'ns")
    p.add_argument('--train_prefix', default='', help='name of the object file that stores the training data.')
    p.add_argument('--epochs', type=int, default=1, help='number of epochs to train.')
    p.add_argument('--dropout', type=float, default=0.0, help='dropout rate (1 - keep probability).')
    p.add_argument('--weight_decay', type=float, default=0.0, help='weight for l2 loss on embedding matrix.')
    p.add_argument('--max_degree', type=int, default=100, help='maximum node degree.')
    p.add_argument('--samples_1', type=int, default=25, help='number of samples in layer 1')
    p.add_argument('--samples_2', type=int, default=10, help='number of users samples in layer 2')
    p.add_argument('--dim_1', type=int, default=128, help='Size of output dim (final is 2x this, if using concat)')
    p.add_argument('--dim_2', type=int, default=128, help='Size of output dim (final is 2x this, if using concat)')
    p.add_argument('--random_context', type=b, default=True, help='Whether to use random context or direct edges')
    p.add_argument('--neg_sample_size', type=int, default=20, help='number of negative samples')
    p.add_argument('--batch_size', type=int, default=512, help='minibatch size.')
    p.add_argument('--n2v_test_epochs', type=int, default=1, help='Number of new SGD epochs for n2v.')
    p.add_argument('--identity_dim', type=int, default=0)
    p.add_argument('--save_embeddings', type=b, default=True, help='whether to save embeddings for all nodes after training')
    p.add_argument('--base_log_dir', default='.', help='base directory for logging and saving embeddings')
    p.add_argument('--validate_iter', type=int, default=5000, help='how often to run a validation minibatch.')
    p.add_argument('--validate_batch_size', type=int, default=256, help='how many nodes per validation sample.')
    p.add_argument('--gpu', type=int, default=1, help='ignored: one process per GPU (LOCAL_RANK)')
    p.add_argument('--print_every', type=int, default=50, help='How often to print training info.')
    p.add_argument('--max_total_steps', type=int, default=10 ** 10, help='Maximum total number of iterations')
    p.add_argument('--synthetic', default='', help='ppi | reddit | small: generate a graph of that shape')
    p.add_argument('--sampler', default='csr', help='csr (MI355X-native) | padded (reference table semantics)')
    p.add_argument('--sampler_law', default='reference',
                   help='sampling law of the CSR sampler: reference (the reference\'s joint law on a virtual padded '
                        '[N+1, max_degree] table, minibatch.py:227-245 + neigh_samplers.py:24-29) | iid (independent '
                        'draws with replacement from the full neighbor list) | distinct (per-row without replacement)')
    p.add_argument('--loss_fn', default='xent', choices=['xent', 'skipgram', 'hinge', 'infonce'],
                   help='loss of the link-prediction layer (prediction.py:58-63); skipgram keeps the reference\'s sign; '
                        'infonce (not in the reference): softmax over the other contexts of the batch and the sampled '
                        'negatives; ignored by --model n2v (infonce is refused there)')
    p.add_argument('--loss_temperature', type=float, default=0.1,
                   help='temperature of --loss_fn infonce, in [0.01, 10]; ignored by the other losses')
    p.add_argument('--bilinear_weights', action='store_true',
                   help='affinity u^T A v with a trainable A (prediction.py:68-92); ignored by --model n2v')
    p.add_argument('--full_inference', type=b, nargs='?', const=True, default=False,
                   help='after val.npy: exact layer-wise embeddings of ALL nodes from their whole neighbor lists on the test '
                        'graph (embed_full) -> val_full.npy / val_full.txt; not for n2v / graphsage_seq')
    p.add_argument('--rank_full', type=b, nargs='?', const=True, default=False,
                   help='after val.npy: rank every held-out edge (both directions) against ALL nodes with the exact embeddings '
                        'on the test graph, known edges filtered (rank_full) -> rank_full.txt; not for n2v / graphsage_seq')
    p.add_argument('--rank_baselines', default='',
                   help='comma list of cn | aa | ra | jaccard, or all: after val.npy (and --rank_full), rank the same held-out '
                        'edges by these neighbor-overlap scores of the TRUE test graph, known edges filtered '
                        '(link_heuristics.rank_neighbors) -> rank_baseline_<kind>.txt; reads the graph only: every --model')
    p.add_argument('--topk_full', type=int, default=0,
                   help='K > 0: after val.npy, the K best-scoring partners of every node among ALL nodes with the exact '
                        'embeddings on the test graph, known edges filtered (topk_full) -> topk_full.npy / '
                        'topk_full_scores.npy; not for n2v / graphsage_seq')
    p.add_argument('--topk_ivf', type=int, default=0,
                   help='K > 0: after val.npy (and --topk_full), the K best-scoring partners of every node through an inverted '
                        'file over a k-means partition of the exact embeddings (topk_ivf: every query scans only the lists it '
                        'probes) -> topk_ivf.npy / topk_ivf_scores.npy / ivf_centers.npy / ivf_labels.npy / topk_ivf.txt; not '
                        'for n2v / graphsage_seq')
    p.add_argument('--topk_ivf_clusters', type=int, default=0, help='lists of --topk_ivf: 1 to 4096 (0: 4 sqrt(N), at most 4096)')
    p.add_argument('--topk_ivf_nprobe', type=int, default=8, help='lists every query of --topk_ivf probes: 1 to 128')
    p.add_argument('--topk_ivf_recall', type=int, default=0,
                   help='S > 0: S nodes are also searched exactly (topk_full) and the line of --topk_ivf carries their recall@K')
    p.add_argument('--topk_ivf_seed', type=int, default=123,
                   help='seed of the k-means++ seeding of --topk_ivf and of its recall sample')
    from .supervised_train import add_embed_nodes_flag, add_importance_flags
    add_embed_nodes_flag(p)
    add_importance_flags(p)
    p.add_argument('--eval_classifier', default='', choices=['', 'val', 'test'],
                   help='val | test: after val.npy, fit a logistic regression on the train nodes\' embeddings on the device and '
                        'score it on that split (the reference\'s eval_scripts; with --full_inference on val_full.npy, with '
                        '--model n2v the scored rows come from val-test.npy) -> eval_classifier.txt')
    p.add_argument('--eval_classifier_inputs', default='embeddings', choices=['embeddings', 'features', 'both', 'all'],
                   help='with --eval_classifier: besides the embeddings line, the same classifier on the feature table the model '
                        'trained on (features -> eval_classifier_features.txt), on [features | embeddings] (both -> '
                        'eval_classifier_both.txt), or the two of them (all); these rows are standardised on the train nodes')
    p.add_argument('--eval_clusters', type=int, default=0,
                   help='K: after val.npy (and --eval_classifier), k-means of ALL rows of the embedding table on the device into '
                        'K clusters (-1: the dataset\'s number of classes), scored against the class labels (NMI, ARI, purity) '
                        '-> eval_clusters.txt, clusters.npy, cluster_centers.npy; with --full_inference on val_full.npy')
    p.add_argument('--eval_clusters_seed', type=int, default=123, help='seed of the k-means++ seeding of --eval_clusters')
    p.add_argument('--max_walk_pairs', type=int, default=2000000, help='cap on generated random-walk pairs (synthetic data)')
    p.add_argument('--walk_p', type=float, default=1.0,
                   help='return parameter p of node2vec\'s second-order walk (a step back to the previous node weighs 1/p)')
    p.add_argument('--walk_q', type=float, default=1.0,
                   help='in-out parameter q of node2vec\'s second-order walk (a step away from the previous node\'s '
                        'neighborhood weighs 1/q); p = q = 1 is the uniform walk of DeepWalk')
    p.add_argument('--walk_len', type=int, default=5, help='nodes per generated random walk, the start included')
    p.add_argument('--num_walks', type=int, default=50, help='generated random walks per start node')
    p.add_argument('--device_walks', type=b, nargs='?', const=True, default=False,
                   help='generate the random walks on the device (gs_walk_paths / gs_walk_pairs); implied by --walk_p / '
                        '--walk_q other than 1')
    return p.parse_args(argv)


def use_device_walks(flags):
    return bool(getattr(flags, "device_walks", False)) or getattr(flags, "walk_p", 1.0) != 1.0 \
        or getattr(flags, "walk_q", 1.0) != 1.0


def refuse_walk_flags(flags):
    """Out-of-range walk parameters are refused before any work is done, with the rule in the message."""
    if flags.walk_len < 1 or flags.num_walks < 1:
        raise SystemExit("--walk_len and --num_walks must be at least 1")
    if not use_device_walks(flags):
        return
    from .ops import walk_thresholds
    try:
        walk_thresholds(flags.walk_p, flags.walk_q)
    except ValueError as e:
        raise SystemExit("--walk_p / --walk_q: %s" % e)


def refuse_loss_flags(flags):
    """--loss_fn infonce: the temperature must lie in the head's range and the model must have a link-prediction layer; refused
    before any work is done, with the rule in the message."""
    if getattr(flags, "loss_fn", "xent") != "infonce":
        return
    if flags.model == 'n2v':
        raise SystemExit("--loss_fn infonce: --model n2v has no link-prediction layer")
    from .ops import INFONCE_TAU_RANGE
    lo, hi = INFONCE_TAU_RANGE
    if not lo <= flags.loss_temperature <= hi:
        raise SystemExit("--loss_temperature %g: must lie in [%g, %g]" % (flags.loss_temperature, lo, hi))


def embedding_width(flags):
    """Columns of val.npy: 2 * dim_2 (concat; gcn doubles its dims instead), 2 * dim_1 for the node2vec table."""
    return 2 * (flags.dim_1 if flags.model == 'n2v' else flags.dim_2)


def refuse_eval_classifier(flags, G=None):
    """--eval_classifier needs the saved embeddings, a width the classifier kernel takes and (once the graph is loaded) class
    labels in its range: anything else is refused before training, with the rule in the message."""
    kinds = eval_classifier_kinds(flags)
    if not getattr(flags, "eval_classifier", ""):
        if kinds:
            raise SystemExit("--eval_classifier_inputs %s needs --eval_classifier val or test" % flags.eval_classifier_inputs)
        return
    from . import evaluation
    if not flags.save_embeddings:
        raise SystemExit("--eval_classifier reads val.npy: it needs --save_embeddings true")
    try:
        evaluation.refuse(embedding_width(flags), n_classes=1)
    except ValueError as e:
        raise SystemExit("--eval_classifier: %s" % e)
    if kinds:
        width = G.feats.shape[1] if G is not None and G.feats is not None else (None if G is not None else feature_width(flags))
        for kind in kinds:
            evaluation.refuse_inputs(kind, width, embedding_width(flags), width is not None)
    if G is not None:
        evaluation.refuse_graph(G)


def refuse_eval_clusters(flags, G=None):
    """--eval_clusters needs the saved embeddings, K in {-1} U [1, 4096], a width the k-means kernel takes, for K = -1 a
    single-label dataset and (once the graph is loaded) no more clusters than nodes: anything else is refused before training,
    with the rule in the message."""
    K = getattr(flags, "eval_clusters", 0)
    if not K:
        return 0
    from . import clustering
    single = False if flags.synthetic == 'ppi' else (True if flags.synthetic else None)
    return clustering.refuse_flags("--eval_clusters", K, width=embedding_width(flags), save_embeddings=flags.save_embeddings,
                                   G=G, single_label=single)


def save_eval_clusters(G, out_dir):
    """eval_clusters.txt, clusters.npy, cluster_centers.npy: k-means of every row of the table that was just written."""
    from . import clustering
    from . import engine as eng
    base = "val_full" if FLAGS.full_inference else "val"
    return clustering.evaluate_embedding_dir(eng.get_engine(), G, out_dir, FLAGS.eval_clusters, base=base,
                                             seed=FLAGS.eval_clusters_seed)


def eval_classifier_kinds(flags):
    """The inputs --eval_classifier_inputs adds to the embeddings line."""
    return {"embeddings": (), "features": ("features",), "both": ("both",),
            "all": ("features", "both")}[getattr(flags, "eval_classifier_inputs", "embeddings")]


def feature_width(flags):
    """Columns of the feature table the run will load, read without loading it; None: the dataset has none."""
    if flags.synthetic:
        return 602 if flags.synthetic == 'reddit' else 50          # supervised_train.load_graph
    path = flags.train_prefix + "-feats.npy"
    if not os.path.exists(path):
        return None
    shape = np.load(path, mmap_mode="r").shape
    return int(shape[1]) if len(shape) == 2 else None


def save_eval_classifier(G, out_dir):
    """eval_classifier.txt: the `Downstream classifier:` line for the table that was just written; then the lines and files
    of --eval_classifier_inputs, on the feature table the model trained on (one upload)."""
    from . import engine as eng
    from . import evaluation
    base = "val_full" if FLAGS.full_inference else "val"
    res = evaluation.evaluate_embedding_dir(eng.get_engine(), G, out_dir, FLAGS.eval_classifier, base=base)
    kinds = eval_classifier_kinds(FLAGS)
    if kinds:
        features = evaluation.as_mat(eng.get_engine(), G.feats)
        for kind in kinds:
            evaluation.evaluate_embedding_dir(eng.get_engine(), G, out_dir, FLAGS.eval_classifier, base=base, inputs=kind,
                                              features=features)
    return res


def device_walks(rowptr, col, nodes, max_pairs=None):
    """(start, current) pairs of (p, q) walks over a host CSR, generated on the device; prints the `Random walks:` line."""
    import torch
    from . import utils
    dev = torch.device("cuda")
    t0 = time.time()
    pairs = utils.device_walk_pairs(torch.from_numpy(np.ascontiguousarray(rowptr, dtype=np.int64)).to(dev),
                                    torch.from_numpy(np.ascontiguousarray(col, dtype=np.int32)).to(dev), nodes,
                                    num_walks=FLAGS.num_walks, walk_len=FLAGS.walk_len, p=FLAGS.walk_p, q=FLAGS.walk_q,
                                    seed=seed, max_pairs=max_pairs).cpu().numpy()
    print("Random walks:", "law=", "node2vec", "p=", "{:g}".format(FLAGS.walk_p), "q=", "{:g}".format(FLAGS.walk_q),
          "len=", FLAGS.walk_len, "walks=", FLAGS.num_walks, "pairs=", len(pairs), "time=", "{:.5f}".format(time.time() - t0))
    return pairs


def log_dir():
    """unsupervised_train.py:61-69"""
    parts = FLAGS.train_prefix.split("/")
    tag = parts[-2] if len(parts) >= 2 else (FLAGS.synthetic or "data")
    d = FLAGS.base_log_dir + "/unsup-" + tag
    d += "/{model:s}_{model_size:s}_{lr:0.6f}".format(model=FLAGS.model, model_size=FLAGS.model_size, lr=FLAGS.learning_rate)
    if FLAGS.model != 'n2v':            # non-default heads get their own directory (the defaults keep the reference's name)
        loss_fn = getattr(FLAGS, "loss_fn", "xent")
        d += ("_" + loss_fn if loss_fn != "xent" else "") + ("_bilinear" if getattr(FLAGS, "bilinear_weights", False) else "")
    d += "/"
    if not os.path.exists(d):
        os.makedirs(d)
    return d


def evaluate(model, minibatch_iter, size=None):
    """unsupervised_train.py:72-77"""
    t_test = time.time()
    feed_dict_val = minibatch_iter.val_feed_dict(size)
    loss, ranks, mrr, _ = model.eval_step(feed_dict_val)
    return loss, ranks, mrr, (time.time() - t_test)


def incremental_evaluate(model, minibatch_iter, size):
    """unsupervised_train.py:79-92"""
    t_test = time.time()
    finished = False
    val_losses, val_mrrs = [], []
    iter_num = 0
    while not finished:
        feed_dict_val, finished, edges = minibatch_iter.incremental_val_feed_dict(size, iter_num)
        iter_num += 1
        if len(edges) == 0:
            continue
        loss, ranks, mrr, _ = model.eval_step(feed_dict_val)
        val_losses.append(loss)
        val_mrrs.append(mrr)
    return np.mean(val_losses), np.mean(val_mrrs), (time.time() - t_test)


def save_val_embeddings(model, minibatch_iter, size, out_dir, mod=""):
    """unsupervised_train.py:94-117: embeddings of every node via (n, n) pairs -> val.npy + val.txt"""
    val_embeddings, nodes = [], []
    seen = set()
    finished = False
    iter_num = 0
    name = "val"
    while not finished:
        feed_dict_val, finished, edges = minibatch_iter.incremental_embed_feed_dict(size, iter_num)
        iter_num += 1
        if len(edges) == 0:
            continue
        _, _, _, outputs1 = model.eval_step(feed_dict_val)
        # ONLY SAVE FOR embeds1 because of planetoid
        for i, edge in enumerate(edges):
            if not edge[0] in seen:
                val_embeddings.append(outputs1[i, :])
                ids = getattr(minibatch_iter.G, "node_ids", None)     # val.txt lists ORIGINAL node ids (:106-110)
                nodes.append(ids[edge[0]] if ids is not None else edge[0])
                seen.add(edge[0])
    if not os.path.exists(out_dir):
        os.makedirs(out_dir)
    val_embeddings = np.vstack(val_embeddings)
    np.save(out_dir + name + mod + ".npy", val_embeddings)
    with open(out_dir + name + mod + ".txt", "w") as fp:
        fp.write("\n".join(map(str, nodes)))


def save_full_embeddings(model, minibatch, out_dir):
    """val_full.npy: the exact (full-neighborhood, layer-wise) embeddings of all N nodes in id order; val_full.txt: their
    ORIGINAL ids, as val.txt lists them."""
    from .supervised_train import full_graph
    G = minibatch.G
    emb = model.embed_full(full_graph(minibatch, G.n_nodes))
    if not os.path.exists(out_dir):
        os.makedirs(out_dir)
    np.save(out_dir + "val_full.npy", emb)
    ids = getattr(G, "node_ids", None)
    with open(out_dir + "val_full.txt", "w") as fp:
        fp.write("\n".join(str(ids[i] if ids is not None else i) for i in range(G.n_nodes)))


def rank_full_line(res):
    """The line --rank_full prints and writes to rank_full.txt."""
    return ("Full-graph link ranking: mrr= {:.5f} ".format(res["mrr"])
            + " ".join("hits@%d= %.5f" % (k, res["hits"][k]) for k in sorted(res["hits"]))
            + " edges= %d" % len(res["ranks"]))


def save_full_ranking(model, minibatch, out_dir):
    """rank_full.txt: every held-out edge, in both directions, ranked against all N nodes with the exact embeddings of the
    test graph; the query node and every edge of the test graph are filtered out of the candidates."""
    from .supervised_train import full_graph
    edges = np.asarray(minibatch.val_edges, dtype=np.int64).reshape(-1, 2)
    res = model.rank_full(full_graph(minibatch, minibatch.G.n_nodes), np.concatenate([edges, edges[:, ::-1]], axis=0))
    line = rank_full_line(res)
    print(line)
    if not os.path.exists(out_dir):
        os.makedirs(out_dir)
    with open(out_dir + "rank_full.txt", "w") as fp:
        fp.write(line + "\n")
    return res


def rank_baseline_kinds(flags):
    """The kinds --rank_baselines lists, in its order; an unknown name is refused before any work is done."""
    from .link_heuristics import parse_kinds
    try:
        return parse_kinds(getattr(flags, "rank_baselines", ""))
    except ValueError as e:
        raise SystemExit("--rank_baselines: %s" % e)


def save_rank_baselines(minibatch, out_dir, kinds):
    """rank_baseline_<kind>.txt: the edges of --rank_full (every held-out edge, both directions) ranked against all N nodes by the
    neighbor-overlap scores of the TRUE test graph (minibatch.test_csr, whatever the sampler reads), its edges filtered."""
    from . import engine as eng
    from . import link_heuristics as lh
    graph = lh.SimpleGraph.from_csr(minibatch.test_csr[0], minibatch.test_csr[1], minibatch.G.n_nodes)
    filt = graph.rank_filter()
    edges = np.asarray(minibatch.val_edges, dtype=np.int64).reshape(-1, 2)
    edges = np.concatenate([edges, edges[:, ::-1]], axis=0)
    if not os.path.exists(out_dir):
        os.makedirs(out_dir)
    out = {}
    for kind in kinds:
        t0 = time.time()
        res = lh.rank_neighbors(eng.get_engine(), graph, edges, kind=kind, filt=filt)
        line = lh.result_line(kind, res, time.time() - t0)
        print(line)
        with open(out_dir + "rank_baseline_%s.txt" % kind, "w") as fp:
            fp.write(line + "\n")
        out[kind] = res
    return out


def topk_full_line(res):
    """The line --topk_full prints."""
    ids = res["ids"]
    return "Full-graph top-K partners: k= %d nodes= %d filled= %.5f" % (
        ids.shape[1], ids.shape[0], float(np.mean(ids >= 0)) if ids.size else 0.0)


def save_full_topk(model, minibatch, out_dir, k):
    """topk_full.npy (int32 [N, K]) / topk_full_scores.npy (float32 [N, K]): for every node in id order its K best-scoring
    partners among all N nodes with the exact embeddings of the test graph, best first (-1 / -inf where a node has fewer
    candidates); the node itself and every edge of the test graph are filtered out of the candidates."""
    from .supervised_train import full_graph
    res = model.topk_full(full_graph(minibatch, minibatch.G.n_nodes), k=k)
    print(topk_full_line(res))
    if not os.path.exists(out_dir):
        os.makedirs(out_dir)
    np.save(out_dir + "topk_full.npy", res["ids"])
    np.save(out_dir + "topk_full_scores.npy", res["scores"])
    return res


def refuse_topk_ivf(flags):
    """--topk_ivf with K, lists, probes or a sample outside their ranges is refused before any work is done."""
    if getattr(flags, "topk_ivf", 0):
        from . import retrieval
        retrieval.refuse_flags(flags.topk_ivf, flags.topk_ivf_clusters, flags.topk_ivf_nprobe, flags.topk_ivf_recall)


def save_ivf_topk(model, minibatch, out_dir, flags):
    """topk_ivf.npy (int32 [N, K]) / topk_ivf_scores.npy (float32 [N, K]): save_full_topk through an inverted file, with the
    index (ivf_centers.npy, ivf_labels.npy) and the line of topk_ivf.txt.  With --topk_ivf_recall S the line carries the
    recall@K of S nodes drawn from RandomState(--topk_ivf_seed) against their exact lists (topk_full)."""
    from . import retrieval
    from ._lib import GraphsageAmdError
    from .supervised_train import full_graph
    N, k, nprobe = minibatch.G.n_nodes, flags.topk_ivf, flags.topk_ivf_nprobe
    graph = full_graph(minibatch, N)
    t0 = time.time()
    try:
        index = retrieval.build_ivf(model.engine, model._exact_table(graph), flags.topk_ivf_clusters, n_cand=N,
                                    seed=flags.topk_ivf_seed)
    except GraphsageAmdError as e:
        raise SystemExit("--topk_ivf: %s" % e)
    build_time = time.time() - t0
    if nprobe > index.n_clusters:
        raise SystemExit("--topk_ivf_nprobe %d: the index has %d lists" % (nprobe, index.n_clusters))
    t0 = time.time()
    res = model.topk_ivf(graph, k=k, nprobe=nprobe, index=index)
    search_time = time.time() - t0
    sample, rec = min(flags.topk_ivf_recall, N), float("nan")
    if sample > 0:
        nodes = np.sort(np.random.RandomState(flags.topk_ivf_seed).choice(N, size=sample, replace=False))
        rec = retrieval.recall(res["ids"][nodes], model.topk_full(graph, nodes=nodes, k=k)["ids"])
    ids = res["ids"]
    res.update({"k": k, "nodes": N, "clusters": index.n_clusters, "empty": index.empty, "nprobe": nprobe,
                "list_min": int(index.sizes.min()), "list_max": int(index.sizes.max()),
                "scanned_share": float(np.mean(res["scanned"]) / max(N, 1)) if ids.size else 0.0,
                "filled": float(np.mean(ids >= 0)) if ids.size else 0.0, "recall": rec, "sample": sample,
                "build_time": build_time, "search_time": search_time})
    line = retrieval.result_line(res)
    print(line)
    if not os.path.exists(out_dir):
        os.makedirs(out_dir)
    with open(out_dir + retrieval.LINE_FILE, "w") as fp:
        fp.write(line + "\n")
    np.save(out_dir + "topk_ivf.npy", ids)
    np.save(out_dir + "topk_ivf_scores.npy", res["scores"])
    index.save(out_dir)
    return res


def construct_placeholders():
    """unsupervised_train.py:119-130"""
    from .models import Placeholder
    return {'batch1': Placeholder('batch1'), 'batch2': Placeholder('batch2'), 'neg_samples': Placeholder('neg_sample_size'),
            'dropout': Placeholder('dropout', 0.), 'batch_size': Placeholder('batch_size')}


def train(G, context_pairs, embed_rows=None):
    from . import engine as eng
    from .minibatch import EdgeMinibatchIterator
    from .models import Node2VecModel, SAGEInfo, SampleAndAggregate
    from .neigh_samplers import AdjInfo, CSRAdjacency, PaddedAdjacency, UniformNeighborSampler

    features = G.padded_features()
    placeholders = construct_placeholders()
    minibatch = EdgeMinibatchIterator(G, None, placeholders, batch_size=FLAGS.batch_size, max_degree=FLAGS.max_degree,
                                      context_pairs=context_pairs if FLAGS.random_context else None,
                                      build_padded=(FLAGS.sampler == 'padded'))
    e = eng.get_engine()
    if getattr(FLAGS, "importance_neighbors", 0):
        from .supervised_train import importance_adjacencies
        train_adj, test_adj = importance_adjacencies(FLAGS, minibatch, G.n_nodes, e.device)
    elif FLAGS.sampler == 'padded':
        train_adj, test_adj = PaddedAdjacency(minibatch.adj, e.device), PaddedAdjacency(minibatch.test_adj, e.device)
    else:
        train_adj = CSRAdjacency(minibatch.train_csr[0], minibatch.train_csr[1], G.n_nodes, e.device)
        test_adj = CSRAdjacency(minibatch.test_csr[0], minibatch.test_csr[1], G.n_nodes, e.device)
    adj_info = AdjInfo(train_adj)
    sampler = UniformNeighborSampler(adj_info, law=FLAGS.sampler_law, max_degree=FLAGS.max_degree)
    kw = dict(model_size=FLAGS.model_size, identity_dim=FLAGS.identity_dim, learning_rate=FLAGS.learning_rate,
              weight_decay=FLAGS.weight_decay, neg_sample_size=FLAGS.neg_sample_size, logging=True,
              loss_fn=FLAGS.loss_fn, bilinear_weights=FLAGS.bilinear_weights, loss_temperature=FLAGS.loss_temperature)
    if FLAGS.model in ('graphsage_mean', 'graphsage'):          # unsupervised_train.py:160-172
        layer_infos = [SAGEInfo("node", sampler, FLAGS.samples_1, FLAGS.dim_1),
                       SAGEInfo("node", sampler, FLAGS.samples_2, FLAGS.dim_2)]
        model = SampleAndAggregate(placeholders, features, adj_info, minibatch.deg, layer_infos=layer_infos, **kw)
    elif FLAGS.model == 'gcn':                                   # :173-187
        layer_infos = [SAGEInfo("node", sampler, FLAGS.samples_1, 2 * FLAGS.dim_1),
                       SAGEInfo("node", sampler, FLAGS.samples_2, 2 * FLAGS.dim_2)]
        model = SampleAndAggregate(placeholders, features, adj_info, minibatch.deg, layer_infos=layer_infos,
                                   aggregator_type="gcn", concat=False, **kw)
    elif FLAGS.model == 'graphsage_seq':                         # :183-198
        layer_infos = [SAGEInfo("node", sampler, FLAGS.samples_1, FLAGS.dim_1),
                       SAGEInfo("node", sampler, FLAGS.samples_2, FLAGS.dim_2)]
        model = SampleAndAggregate(placeholders, features, adj_info, minibatch.deg, layer_infos=layer_infos,
                                   aggregator_type="seq", **kw)
    elif FLAGS.model in ('graphsage_maxpool', 'graphsage_meanpool', 'graphsage_twomaxpool', 'graphsage_attn'):   # :203-230
        layer_infos = [SAGEInfo("node", sampler, FLAGS.samples_1, FLAGS.dim_1),
                       SAGEInfo("node", sampler, FLAGS.samples_2, FLAGS.dim_2)]
        model = SampleAndAggregate(placeholders, features, adj_info, minibatch.deg, layer_infos=layer_infos,
                                   aggregator_type=FLAGS.model.split('_')[1], **kw)
    elif FLAGS.model == 'n2v':                                   # :227-232
        model = Node2VecModel(placeholders, G.n_nodes + 1, minibatch.deg,
                              nodevec_dim=2 * FLAGS.dim_1,      # 2x because graphsage uses concat
                              lr=FLAGS.learning_rate, neg_sample_size=FLAGS.neg_sample_size)
    else:
        raise Exception('Error: model name unrecognized.')

    train_shadow_mrr = None
    shadow_mrr = None
    total_steps = 0
    avg_time = 0.0
    epoch_val_costs = []
    val_cost = val_mrr = 0.0
    for epoch in range(FLAGS.epochs):
        minibatch.shuffle()
        it = 0
        print('Epoch: %04d' % (epoch + 1))
        epoch_val_costs.append(0)
        while not minibatch.end():
            feed_dict = minibatch.next_minibatch_feed_dict()
            feed_dict.update({placeholders['dropout']: FLAGS.dropout})
            t = time.time()
            train_cost, ranks, aff_all, train_mrr, outputs1 = model.train_step(feed_dict)     # :273-274
            if train_shadow_mrr is None:
                train_shadow_mrr = train_mrr
            else:
                train_shadow_mrr -= (1 - 0.99) * (train_shadow_mrr - train_mrr)
            if it % FLAGS.validate_iter == 0:
                adj_info.assign(test_adj)
                val_cost, ranks, val_mrr, duration = evaluate(model, minibatch, size=FLAGS.validate_batch_size)
                adj_info.assign(train_adj)
                epoch_val_costs[-1] += val_cost
            if shadow_mrr is None:
                shadow_mrr = val_mrr
            else:
                shadow_mrr -= (1 - 0.99) * (shadow_mrr - val_mrr)
            avg_time = (avg_time * total_steps + time.time() - t) / (total_steps + 1)
            if total_steps % FLAGS.print_every == 0:
                print("Iter:", '%04d' % it,
                      "train_loss=", "{:.5f}".format(train_cost),
                      "train_mrr=", "{:.5f}".format(train_mrr),
                      "train_mrr_ema=", "{:.5f}".format(train_shadow_mrr),
                      "val_loss=", "{:.5f}".format(val_cost),
                      "val_mrr=", "{:.5f}".format(val_mrr),
                      "val_mrr_ema=", "{:.5f}".format(shadow_mrr),
                      "time=", "{:.5f}".format(avg_time))
            it += 1
            total_steps += 1
            if total_steps > FLAGS.max_total_steps:
                break
        if total_steps > FLAGS.max_total_steps:
            break
    print("Optimization Finished!")
    if FLAGS.save_embeddings:
        adj_info.assign(test_adj)
        save_val_embeddings(model, minibatch, FLAGS.validate_batch_size, log_dir())
        if FLAGS.full_inference:
            save_full_embeddings(model, minibatch, log_dir())
        if FLAGS.rank_full:
            save_full_ranking(model, minibatch, log_dir())
        if rank_baseline_kinds(FLAGS):
            save_rank_baselines(minibatch, log_dir(), rank_baseline_kinds(FLAGS))
        if FLAGS.topk_full:
            save_full_topk(model, minibatch, log_dir(), FLAGS.topk_full)
        if FLAGS.topk_ivf:
            save_ivf_topk(model, minibatch, log_dir(), FLAGS)
        if FLAGS.model == "n2v":
            n2v_retrain(G, model, minibatch, placeholders)
        if FLAGS.eval_classifier:
            save_eval_classifier(G, log_dir())
        if FLAGS.eval_clusters:
            save_eval_clusters(G, log_dir())
    elif rank_baseline_kinds(FLAGS):                 # the baselines read the graph alone: no embeddings needed
        save_rank_baselines(minibatch, log_dir(), rank_baseline_kinds(FLAGS))
    if embed_rows is not None:
        from .supervised_train import save_embed_nodes
        save_embed_nodes(model, minibatch, G.n_nodes, embed_rows, log_dir(), supervised=False)
    return shadow_mrr


def n2v_retrain(G, model, minibatch, placeholders):
    """unsupervised_train.py:322-372: embeddings for the val / test nodes of the node2vec baseline -- random walks from
    them over the whole graph, n2v_test_epochs more SGD epochs on the walk pairs whose context is a train node, then
    val-test.npy / val-test.txt.
    The reference first re-binds the Python attribute model.context_embeds to a stop-gradient mix (:324-333), AFTER opt_op
    was built: the optimizer keeps updating the variable itself, so that block changes no gradient.  What restricts this
    phase is the iterator's _n2v_prune alone (every first node is a val / test node, every second a train node), and that
    is what runs here."""
    from . import utils
    from .minibatch import EdgeMinibatchIterator
    nodes = np.where((G.val_mask | G.test_mask) & G.present)[0]
    start_time = time.time()
    rowptr, col = minibatch.test_csr                              # the walks see every edge (:335-338 walks on G)
    if use_device_walks(FLAGS):
        pairs = device_walks(rowptr, col, nodes)
    else:
        pairs = utils.run_random_walks(rowptr, col, nodes, num_walks=FLAGS.num_walks, walk_len=FLAGS.walk_len)
    walk_time = time.time() - start_time
    test_minibatch = EdgeMinibatchIterator(G, None, placeholders, batch_size=FLAGS.batch_size, max_degree=FLAGS.max_degree,
                                           num_neg_samples=FLAGS.neg_sample_size, context_pairs=pairs, n2v_retrain=True,
                                           fixed_n2v=True, build_padded=False)
    start_time = time.time()
    print("Doing test training for n2v.")
    test_steps = 0
    for epoch in range(FLAGS.n2v_test_epochs):
        test_minibatch.shuffle()
        while not test_minibatch.end():
            feed_dict = test_minibatch.next_minibatch_feed_dict()
            feed_dict.update({placeholders['dropout']: FLAGS.dropout})
            train_cost, ranks, aff_all, train_mrr, outputs1 = model.train_step(feed_dict)
            if test_steps % FLAGS.print_every == 0:
                print("Iter:", '%04d' % test_steps,
                      "train_loss=", "{:.5f}".format(train_cost),
                      "train_mrr=", "{:.5f}".format(train_mrr))
            test_steps += 1
    train_time = time.time() - start_time
    save_val_embeddings(model, minibatch, FLAGS.validate_batch_size, log_dir(), mod="-test")
    print("Total time: ", train_time + walk_time)
    print("Walk time: ", walk_time)
    print("Train time: ", train_time)


def main(argv=None):
    global FLAGS
    FLAGS = build_flags(argv)
    from . import utils
    from . import supervised_train as st
    st.refuse_full_inference(FLAGS)
    st.refuse_dropout(FLAGS)
    st.refuse_samples(FLAGS)
    st.refuse_importance(FLAGS)
    refuse_walk_flags(FLAGS)
    refuse_loss_flags(FLAGS)
    refuse_eval_classifier(FLAGS)
    refuse_eval_clusters(FLAGS)
    refuse_topk_ivf(FLAGS)
    rank_baseline_kinds(FLAGS)
    tokens = st.read_embed_nodes(FLAGS)
    print("Loading training data..")
    st.FLAGS = argparse.Namespace(synthetic=FLAGS.synthetic, train_prefix=FLAGS.train_prefix, sigmoid=False)
    G = st.load_graph()
    refuse_eval_classifier(FLAGS, G)
    refuse_eval_clusters(FLAGS, G)
    pairs = None
    if FLAGS.random_context:
        walks = FLAGS.train_prefix + "-walks.txt"
        if FLAGS.train_prefix and os.path.exists(walks):          # utils.py:70-74
            pairs = utils.load_walk_pairs(walks, G)                # original ids -> rows via id_map
        else:
            rp, col = utils.build_csr(G.n_nodes, G.src, G.dst, keep=~G.train_removed)
            train_nodes = np.where(~(G.val_mask | G.test_mask))[0]
            if use_device_walks(FLAGS):
                pairs = device_walks(rp, col, train_nodes, max_pairs=FLAGS.max_walk_pairs)
            else:
                pairs = utils.run_random_walks(rp, col, train_nodes, num_walks=FLAGS.num_walks, walk_len=FLAGS.walk_len,
                                               max_pairs=FLAGS.max_walk_pairs)
    print("Done loading training data..")
    return train(G, pairs, st.embed_nodes_rows(G, tokens, FLAGS.embed_nodes) if tokens is not None else None)


if __name__ == '__main__':
    main()
