"""Supervised training driver with the flags, loop structure, log-line format and output files of
graphsage/supervised_train.py (flags :28-57, loop :262-312, stats files :314-330), driving the MI355X
engine.  `sess.run(...)` becomes `model.train_step(feed_dict)` / `model.eval_step(feed_dict)`.

    python -m graphsage_amd.supervised_train --train_prefix ./example_data/toy-ppi --model graphsage_mean --sigmoid
    python -m graphsage_amd.supervised_train --synthetic ppi --model graphsage_mean --sigmoid --epochs 2

`--synthetic {ppi,reddit,small}` generates a graph of the reference dataset's shape (the datasets themselves
are not shipped with the reference: example_data/.MISSING_LARGE_BLOBS).  `--sampler {csr,padded}` selects the
MI355X-native CSR sampler (default) or the reference's padded-table sampler.
"""
from __future__ import division, print_function

import argparse
import os
import time

import numpy as np

# Set random seed (supervised_train.py:20-22)
seed = 123
np.random.seed(seed)


def build_flags(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    b = lambda v: str(v).lower() in ("1", "true", "yes")
    p.add_argument('--log_device_placement', type=b, default=False)
    # core params..
    p.add_argument('--model', default='graphsage_mean', help='model names. See README for possible values.')
    p.add_argument('--learning_rate', type=float, default=0.01, help='initial learning rate.')
    p.add_argument('--model_size', default='small', help="Can be big or small; model specific def'ns")
    p.add_argument('--train_prefix', default='', help='prefix identifying training data. must be specified.')
    # left to default values in main experiments
    p.add_argument('--epochs', type=int, default=10, help='number of epochs to train.')
    p.add_argument('--dropout', type=float, default=0.0, help='dropout rate (1 - keep probability).')
    p.add_argument('--weight_decay', type=float, default=0.0, help='weight for l2 loss on embedding matrix.')
    p.add_argument('--max_degree', type=int, default=128, help='maximum node degree.')
    p.add_argument('--samples_1', type=int, default=25, help='number of samples in layer 1')
    p.add_argument('--samples_2', type=int, default=10, help='number of samples in layer 2')
    p.add_argument('--samples_3', type=int, default=0, help='number of users samples in layer 3. (Only for mean model)')
    p.add_argument('--dim_1', type=int, default=128, help='Size of output dim (final is 2x this, if using concat)')
    p.add_argument('--dim_2', type=int, default=128, help='Size of output dim (final is 2x this, if using concat)')
    p.add_argument('--random_context', type=b, default=True, help='Whether to use random context or direct edges')
    p.add_argument('--batch_size', type=int, default=512, help='minibatch size.')
    p.add_argument('--sigmoid', action='store_true', default=False, help='whether to use sigmoid loss')
    p.add_argument('--identity_dim', type=int, default=0, help='identity embedding features dimension. Default 0.')
    # logging, saving, validation settings etc.
    p.add_argument('--base_log_dir', default='.', help='base directory for logging and saving embeddings')
    p.add_argument('--validate_iter', type=int, default=5000, help='how often to run a validation minibatch.')
    p.add_argument('--validate_batch_size', type=int, default=256, help='how many nodes per validation sample.')
    p.add_argument('--gpu', type=int, default=1, help='which gpu to use (ignored: one process per GPU, LOCAL_RANK).')
    p.add_argument('--print_every', type=int, default=5, help='How often to print training info.')
    p.add_argument('--max_total_steps', type=int, default=10 ** 10, help='Maximum total number of iterations')
    # additions of this engine
    p.add_argument('--synthetic', default='', help='ppi | reddit | small: generate a graph of that shape')
    p.add_argument('--sampler', default='csr', help='csr (MI355X-native) | padded (reference table semantics)')
    p.add_argument('--sampler_law', default='reference',
                   help='sampling law of the CSR sampler: reference (the reference\'s joint law on a virtual padded '
                        '[N+1, max_degree] table, minibatch.py:227-245 + neigh_samplers.py:24-29) | iid (independent '
                        'draws with replacement from the full neighbor list) | distinct (per-row without replacement)')
    p.add_argument('--feed_path', default='device',
                   help='device: epoch order + labels resident in HBM, host fetches only printed steps (CSR sampler); '
                        'host: the reference feed_dict path, one host round trip per step')
    p.add_argument('--full_inference', type=b, nargs='?', const=True, default=False,
                   help='after training: exact layer-wise inference over every node\'s WHOLE neighbor list on the test graph '
                        '(predict_full) -> val_stats_full.txt / test_stats_full.txt; not for graphsage_seq')
    add_embed_nodes_flag(p)
    add_importance_flags(p)
    add_propagation_flags(p)
    return p.parse_args(argv)


def add_propagation_flags(p):
    b = lambda v: str(v).lower() in ("1", "true", "yes")
    p.add_argument('--correct_smooth', type=b, nargs='?', const=True, default=False,
                   help='after training: Correct and Smooth (autoscale) over the TRUE test graph from the predict_full predictions '
                        'and the labels of every node that is neither val nor test -> val_stats_cs.txt / test_stats_cs.txt; not '
                        'for graphsage_seq')
    p.add_argument('--label_propagation', type=b, nargs='?', const=True, default=False,
                   help='after training: plain label propagation of the same labels over the same graph (the graph-only '
                        'baseline; --cs_smooth_alpha, --cs_iters) -> val_stats_lp.txt / test_stats_lp.txt; not for graphsage_seq')
    p.add_argument('--cs_correct_alpha', type=float, default=0.8, help='alpha of the error propagation of --correct_smooth')
    p.add_argument('--cs_smooth_alpha', type=float, default=0.8,
                   help='alpha of the label propagation of --correct_smooth and --label_propagation')
    p.add_argument('--cs_iters', type=int, default=50, help='propagation steps of --correct_smooth (each phase) and '
                                                           '--label_propagation')


def add_embed_nodes_flag(p):
    p.add_argument('--embed_nodes', default='',
                   help='FILE with one ORIGINAL node id per line (the ids val.txt lists): after training, their exact embeddings '
                        'from their receptive field alone on the test graph (embed_nodes) -> embed_nodes.npy / embed_nodes.txt '
                        '(supervised: + embed_nodes_preds.npy); not for n2v / graphsage_seq')


def add_importance_flags(p):
    p.add_argument('--importance_neighbors', type=int, default=0,
                   help='T > 0: importance neighborhoods (PinSage) in place of adjacency rows: a node\'s neighbors are the T '
                        'nodes that short random walks from it visit most often, stored in the --max_degree slots of its table '
                        'row in proportion to their visits (gs_importance_table); sampling, validation, --full_inference, '
                        '--embed_nodes and --eval_classifier then run over that graph; 0: off')
    p.add_argument('--importance_walks', type=int, default=50, help='random walks per node for --importance_neighbors')
    p.add_argument('--importance_walk_len', type=int, default=3,
                   help='nodes per walk for --importance_neighbors, the start included')
    p.add_argument('--importance_p', type=float, default=1.0, help='return parameter p of the walks for --importance_neighbors')
    p.add_argument('--importance_q', type=float, default=1.0, help='in-out parameter q of the walks for --importance_neighbors')


FLAGS = None


def refuse_importance(flags):
    """--importance_neighbors with a model, a follow-up flag or sizes it does not cover is refused before any work is done, with
    the rule in the message."""
    top = getattr(flags, "importance_neighbors", 0)
    if not top:
        return
    from . import _lib
    if flags.model == 'n2v':
        raise SystemExit("--importance_neighbors is not available with --model n2v: node2vec has no aggregation layers (it "
                         "samples no neighborhoods)")
    for flag in ("rank_full", "topk_full", "topk_ivf"):
        if getattr(flags, flag, False):
            raise SystemExit("--importance_neighbors cannot be combined with --%s: its filter is the known edges of the graph it "
                             "is given, and that must stay the true graph, not the importance neighborhoods" % flag)
    walks, length, slots = flags.importance_walks, flags.importance_walk_len, flags.max_degree
    if not 1 <= top <= _lib.IMPORTANCE_MAX_TOP:
        raise SystemExit("--importance_neighbors %d: must lie in 1 .. %d" % (top, _lib.IMPORTANCE_MAX_TOP))
    if walks < 1 or length < 2:
        raise SystemExit("--importance_walks must be at least 1 and --importance_walk_len at least 2")
    if walks * (length - 1) > _lib.IMPORTANCE_MAX_VISITS:
        raise SystemExit("--importance_walks %d x (--importance_walk_len %d - 1) = %d visits per node; at most %d"
                         % (walks, length, walks * (length - 1), _lib.IMPORTANCE_MAX_VISITS))
    if not 1 <= slots <= _lib.IMPORTANCE_MAX_SLOTS:
        raise SystemExit("--importance_neighbors fills --max_degree %d slots per node; it must lie in 1 .. %d"
                         % (slots, _lib.IMPORTANCE_MAX_SLOTS))
    from .ops import walk_thresholds
    try:
        walk_thresholds(flags.importance_p, flags.importance_q)
    except ValueError as e:
        raise SystemExit("--importance_p / --importance_q: %s" % e)


def importance_line(flags, graph, n_rows, stats, duration):
    """The line --importance_neighbors prints per graph; stats: int [n_rows, 2] = (distinct nodes visited, nodes with a slot)."""
    stats = np.asarray(stats).reshape(-1, 2)
    return ("Importance neighborhoods: graph= %s top= %d slots= %d walks= %d len= %d p= %g q= %g rows= %d distinct_mean= %.5f "
            "kept_mean= %.5f empty= %d time= %.5f" % (
                graph, flags.importance_neighbors, flags.max_degree, flags.importance_walks, flags.importance_walk_len,
                flags.importance_p, flags.importance_q, n_rows, stats[:, 0].mean() if n_rows else 0.0,
                stats[:, 1].mean() if n_rows else 0.0, int((stats[:, 0] == 0).sum()), duration))


def importance_adjacencies(flags, minibatch, n_nodes, device):
    """The importance tables of the train and the test graph (utils.importance_neighbors over minibatch.train_csr / .test_csr),
    one printed line each, as the adjacencies the sampler sees: padded tables under --sampler padded, else their CSR.  The test
    table is kept on the iterator for full_graph().  The true graph stays what it was everywhere else (minibatch.deg, the
    negative-sampling law, the context pairs, val_edges)."""
    import torch
    from . import utils
    from .neigh_samplers import CSRAdjacency, PaddedAdjacency
    out = []
    for graph, (rowptr, col) in (("train", minibatch.train_csr), ("test", minibatch.test_csr)):
        t0 = time.time()
        table, stats = utils.importance_neighbors(
            torch.from_numpy(np.ascontiguousarray(rowptr, dtype=np.int64)).to(device),
            torch.from_numpy(np.ascontiguousarray(col, dtype=np.int32)).to(device), n_nodes, flags.importance_neighbors,
            flags.max_degree, num_walks=flags.importance_walks, walk_len=flags.importance_walk_len, p=flags.importance_p,
            q=flags.importance_q, seed=seed)
        stats = stats.cpu().numpy()                          # (the copy ends the timed work)
        print(importance_line(flags, graph, n_nodes, stats, time.time() - t0))
        out.append(PaddedAdjacency(table, device) if flags.sampler == 'padded' else CSRAdjacency.from_table(table))
        if graph == "test":
            minibatch.importance_test = table
    # the tables and their CSRs were made on torch's current stream; the engine's stream does not wait for it by itself
    torch.cuda.current_stream().synchronize()
    return out


def refuse_full_inference(flags):
    """--full_inference (and --rank_full / --topk_full / --topk_ivf, which rank the embed_full embeddings) has no meaning for the models
    without a full-neighborhood form: say so before any work is done."""
    for flag in ("full_inference", "rank_full", "topk_full", "topk_ivf", "embed_nodes", "correct_smooth", "label_propagation"):
        if getattr(flags, flag, False) and flags.model in ('n2v', 'graphsage_seq'):
            raise SystemExit("--%s is not available with --model %s: %s" % (
                flag, flags.model, "node2vec has no aggregation layers (its embeddings are table rows)" if flags.model == 'n2v'
                else "an LSTM over a random permutation of a neighbor sample has no full-neighborhood form"))


def read_embed_nodes(flags):
    """The tokens of --embed_nodes FILE, one per non-empty line (None without the flag); a missing file is refused here, before
    any work is done."""
    path = getattr(flags, "embed_nodes", "")
    if not path:
        return None
    if not os.path.isfile(path):
        raise SystemExit("--embed_nodes %s: no such file" % path)
    with open(path) as fp:
        return [line.strip() for line in fp if line.strip()]


def embed_nodes_rows(G, tokens, path):
    """Rows of the ORIGINAL node ids `tokens` in G (through the id map, where the graph has one); an id that the graph does not
    have is refused, before training."""
    id_map = getattr(G, "id_map", None)
    rows = []
    for tok in tokens:
        if id_map is not None:
            row = id_map.get(tok)
        else:
            row = int(tok) if tok.lstrip("-").isdigit() and 0 <= int(tok) < G.n_nodes else None
        if row is None:
            raise SystemExit("--embed_nodes %s: the graph has no node %s" % (path, tok))
        rows.append(row)
    if not rows:
        raise SystemExit("--embed_nodes %s: the file lists no node" % path)
    return np.asarray(rows, dtype=np.int64)


def embed_nodes_line(n, stats, duration):
    """The line --embed_nodes prints."""
    return "Receptive-field inference: nodes= %d rows= %s of %d edges= %d time= %.5f" % (
        n, " / ".join(str(r) for r in stats["rows"]), stats["n_rows"], sum(stats["edges"]), duration)


def save_embed_nodes(model, minibatch, n_nodes, rows, out_dir, supervised):
    """embed_nodes.npy (+ embed_nodes_preds.npy): the exact embeddings of the rows `rows` from their receptive field on the test
    graph, in the order of the file; embed_nodes.txt: their ORIGINAL ids, as val.txt lists them."""
    graph = full_graph(minibatch, n_nodes)
    t0 = time.time()
    res = model.predict_nodes(graph, rows) if supervised else model.embed_nodes(graph, rows)
    duration = time.time() - t0
    print(embed_nodes_line(len(rows), res[-1], duration))
    if not os.path.exists(out_dir):
        os.makedirs(out_dir)
    np.save(out_dir + "embed_nodes.npy", res[0])
    if supervised:
        np.save(out_dir + "embed_nodes_preds.npy", res[1])
    ids = getattr(minibatch.G, "node_ids", None)
    with open(out_dir + "embed_nodes.txt", "w") as fp:
        fp.write("\n".join(str(ids[i] if ids is not None else i) for i in rows))
    return res


def refuse_dropout(flags):
    """The two-layer max-pooling aggregator runs without dropout (its second Dense has no mask site): say so before any work."""
    if flags.model == 'graphsage_twomaxpool' and getattr(flags, "dropout", 0.0) > 0:
        from ._lib import GraphsageAmdError
        raise GraphsageAmdError("--dropout > 0 is not supported with --model graphsage_twomaxpool (the reference drops the "
                                "input of both Dense layers of the aggregator; only --dropout 0 is implemented)")


def refuse_samples(flags):
    """The attention-pooling kernels take 1 <= s <= 128 sampled neighbors per node: refuse a wider --samples_* before any work."""
    if flags.model == 'graphsage_attn':
        from .aggregators import AttentionPoolingAggregator
        AttentionPoolingAggregator.check_samples([s for s in (flags.samples_1, flags.samples_2, getattr(flags, "samples_3", 0))
                                                  if s != 0])


def full_graph(minibatch, n_nodes):
    """The test graph for full-neighborhood inference: the padded test table verbatim under --sampler padded, else the CSR."""
    from .inference import FullGraph
    if getattr(minibatch, "importance_test", None) is not None:      # --importance_neighbors: that table verbatim
        return FullGraph.from_padded(minibatch.importance_test)
    if minibatch.test_adj is not None:
        return FullGraph.from_padded(minibatch.test_adj)
    return FullGraph.from_csr(minibatch.test_csr[0], minibatch.test_csr[1], n_nodes)


def refuse_propagation(flags):
    """--correct_smooth / --label_propagation with an alpha or a step count outside the kernel's schedule are refused before any
    work is done."""
    if not (getattr(flags, "correct_smooth", False) or getattr(flags, "label_propagation", False)):
        return
    from . import propagation
    from ._lib import GraphsageAmdError
    try:
        if flags.correct_smooth:
            propagation.check_schedule(flags.cs_correct_alpha, flags.cs_iters, "--cs_correct_alpha / --cs_iters")
        propagation.check_schedule(flags.cs_smooth_alpha, flags.cs_iters, "--cs_smooth_alpha / --cs_iters")
    except GraphsageAmdError as e:
        raise SystemExit(str(e))


def refuse_propagation_classes(flags, num_classes):
    """... and a label table wider than the propagation kernel takes, once the data is loaded."""
    if getattr(flags, "correct_smooth", False) or getattr(flags, "label_propagation", False):
        from . import propagation
        from ._lib import GraphsageAmdError
        try:
            propagation.check_classes(num_classes, "--correct_smooth / --label_propagation")
        except GraphsageAmdError as e:
            raise SystemExit(str(e))


def _write_f1_files(tag, stats, duration):
    """val_stats_<tag>.txt / test_stats_<tag>.txt in the layout of val_stats_full.txt."""
    with open(log_dir() + "val_stats_%s.txt" % tag, "w") as fp:
        fp.write("f1_micro={:.5f} f1_macro={:.5f} time={:.5f}".format(stats[0][0], stats[0][1], duration))
    with open(log_dir() + "test_stats_%s.txt" % tag, "w") as fp:
        fp.write("f1_micro={:.5f} f1_macro={:.5f}".format(stats[1][0], stats[1][1]))


def _val_test_f1(minibatch, scores):
    return [calc_f1(minibatch.label_matrix[nodes], scores[nodes]) if len(nodes) else (0.0, 0.0)
            for nodes in (minibatch.val_nodes, minibatch.test_nodes)]


def propagation_stats(model, minibatch, n_nodes, preds=None):
    """--correct_smooth and --label_propagation: over the TRUE test graph (the real edges, also under --sampler padded and
    --importance_neighbors), from the labels of every node that is neither val nor test.  preds: the predict_full predictions
    of every node when --full_inference has computed them already."""
    from . import propagation
    from .inference import FullGraph
    graph = FullGraph.from_csr(minibatch.test_csr[0], minibatch.test_csr[1], n_nodes)
    known = np.ones(n_nodes, dtype=bool)
    known[minibatch.val_nodes] = False
    known[minibatch.test_nodes] = False
    known = np.flatnonzero(known)
    labels = np.asarray(minibatch.label_matrix, dtype=np.float32)[:n_nodes]          # (the table also has the pad node's row)
    e = model.engine
    prop = propagation.Propagator(e, graph)
    out = {}
    if FLAGS.correct_smooth:
        if preds is None:
            _, preds = model.predict_full(full_graph(minibatch, n_nodes))
        t0 = time.time()
        res = propagation.correct_and_smooth(e, graph, preds, labels, known, correct_alpha=FLAGS.cs_correct_alpha,
                                             smooth_alpha=FLAGS.cs_smooth_alpha, iters=FLAGS.cs_iters, propagator=prop)
        duration = time.time() - t0
        base, stats = _val_test_f1(minibatch, preds), _val_test_f1(minibatch, res["preds"])
        print("Correct and smooth: nodes= %d known= %d classes= %d correct_alpha= %g smooth_alpha= %g iters= %d sigma= %.5f "
              "base_val_f1_micro= %.5f val_f1_micro= %.5f val_f1_macro= %.5f base_test_f1_micro= %.5f test_f1_micro= %.5f "
              "test_f1_macro= %.5f time= %.5f" % (
                  n_nodes, len(known), labels.shape[1], FLAGS.cs_correct_alpha, FLAGS.cs_smooth_alpha, FLAGS.cs_iters,
                  res["sigma"], base[0][0], stats[0][0], stats[0][1], base[1][0], stats[1][0], stats[1][1], duration))
        _write_f1_files("cs", stats, duration)
        out["correct_smooth"] = stats
    if FLAGS.label_propagation:
        t0 = time.time()
        scores = propagation.label_propagation(e, graph, labels, known, alpha=FLAGS.cs_smooth_alpha, iters=FLAGS.cs_iters,
                                               propagator=prop)
        duration = time.time() - t0
        stats = _val_test_f1(minibatch, scores)
        print("Label propagation: nodes= %d known= %d classes= %d alpha= %g iters= %d val_f1_micro= %.5f val_f1_macro= %.5f "
              "test_f1_micro= %.5f test_f1_macro= %.5f time= %.5f" % (
                  n_nodes, len(known), labels.shape[1], FLAGS.cs_smooth_alpha, FLAGS.cs_iters, stats[0][0], stats[0][1],
                  stats[1][0], stats[1][1], duration))
        _write_f1_files("lp", stats, duration)
        out["label_propagation"] = stats
    return out


def full_inference_stats(model, minibatch, n_nodes, keep=None):
    """Exact inference for every node at once (model.predict_full), scored on the validation and the test nodes.  keep: a dict
    that receives the predictions under "preds", for what follows."""
    t_test = time.time()
    _, preds = model.predict_full(full_graph(minibatch, n_nodes))
    duration = time.time() - t_test
    if keep is not None:
        keep["preds"] = preds
    stats = []
    for nodes in (minibatch.val_nodes, minibatch.test_nodes):
        stats.append(calc_f1(minibatch.label_matrix[nodes], preds[nodes]) if len(nodes) else (0.0, 0.0))
    print("Full-neighborhood validation stats:",
          "f1_micro=", "{:.5f}".format(stats[0][0]),
          "f1_macro=", "{:.5f}".format(stats[0][1]),
          "time=", "{:.5f}".format(duration))
    with open(log_dir() + "val_stats_full.txt", "w") as fp:
        fp.write("f1_micro={:.5f} f1_macro={:.5f} time={:.5f}".format(stats[0][0], stats[0][1], duration))
    with open(log_dir() + "test_stats_full.txt", "w") as fp:
        fp.write("f1_micro={:.5f} f1_macro={:.5f}".format(stats[1][0], stats[1][1]))
    return stats


def f1_micro_macro(y_true, y_pred, multilabel):
    """sklearn.metrics.f1_score(average="micro") and (average="macro") in NumPy (same definitions: per-class
    tp/fp/fn; macro averages the per-class F1 over the classes that occur in y_true or y_pred -- every column for
    multilabel indicator input -- with F1 = 0 where tp + fp + fn == 0 ... == 0 only for absent columns, which sklearn
    scores 0 as well).  The reference calls sklearn every print_every steps (supervised_train.py:63-70); at ~0.15 ms per
    training step that call would dominate the loop."""
    if multilabel:
        t = np.asarray(y_true) > 0.5
        p = np.asarray(y_pred) > 0.5
        tp = (t & p).sum(axis=0).astype(np.float64)
        fp = (~t & p).sum(axis=0).astype(np.float64)
        fn = (t & ~p).sum(axis=0).astype(np.float64)
    else:
        t = np.asarray(y_true).astype(np.int64)
        p = np.asarray(y_pred).astype(np.int64)
        classes = np.union1d(t, p)
        C = int(classes.max()) + 1 if classes.size else 1
        hit = t == p
        tp_all = np.bincount(t[hit], minlength=C).astype(np.float64)
        fp_all = np.bincount(p[~hit], minlength=C).astype(np.float64)
        fn_all = np.bincount(t[~hit], minlength=C).astype(np.float64)
        tp, fp, fn = tp_all[classes], fp_all[classes], fn_all[classes]
    den = 2 * tp + fp + fn
    per_class = np.where(den > 0, 2 * tp / np.where(den > 0, den, 1), 0.0)
    D = 2 * tp.sum() + fp.sum() + fn.sum()
    micro = float(2 * tp.sum() / D) if D > 0 else 0.0
    macro = float(per_class.mean()) if per_class.size else 0.0
    return micro, macro


def calc_f1(y_true, y_pred):
    """supervised_train.py:63-70"""
    y_pred = np.array(y_pred, copy=True)
    if not FLAGS.sigmoid:
        return f1_micro_macro(np.argmax(y_true, axis=1), np.argmax(y_pred, axis=1), False)
    return f1_micro_macro(y_true, y_pred > 0.5, True)


def evaluate(model, minibatch_iter, placeholders, size=None):
    """supervised_train.py:73-79"""
    t_test = time.time()
    feed_dict_val, labels = minibatch_iter.node_val_feed_dict(size)
    loss, preds = model.eval_step(feed_dict_val)
    mic, mac = calc_f1(labels, preds)
    return loss, mic, mac, (time.time() - t_test)


def log_dir():
    """supervised_train.py:81-89"""
    parts = FLAGS.train_prefix.split("/")
    tag = parts[-2] if len(parts) >= 2 else (FLAGS.synthetic or "data")
    d = FLAGS.base_log_dir + "/sup-" + tag
    d += "/{model:s}_{model_size:s}_{lr:0.4f}/".format(model=FLAGS.model, model_size=FLAGS.model_size,
                                                      lr=FLAGS.learning_rate)
    if not os.path.exists(d):
        os.makedirs(d)
    return d


def incremental_evaluate(model, minibatch_iter, size, test=False):
    """supervised_train.py:91-110"""
    t_test = time.time()
    val_losses, val_preds, labels = [], [], []
    iter_num = 0
    finished = False
    while not finished:
        feed_dict_val, batch_labels, finished, _ = minibatch_iter.incremental_node_val_feed_dict(size, iter_num, test=test)
        if len(batch_labels) > 0:
            loss, preds = model.eval_step(feed_dict_val)
            val_preds.append(preds)
            labels.append(batch_labels)
            val_losses.append(loss)
        iter_num += 1
    val_preds = np.vstack(val_preds)
    labels = np.vstack(labels)
    f1_scores = calc_f1(labels, val_preds)
    return np.mean(val_losses), f1_scores[0], f1_scores[1], (time.time() - t_test)


def construct_placeholders(num_classes):
    """supervised_train.py:112-120"""
    from .models import Placeholder
    return {'labels': Placeholder('labels'), 'batch': Placeholder('batch1'),
            'dropout': Placeholder('dropout', 0.), 'batch_size': Placeholder('batch_size')}


def load_graph():
    from . import utils
    if FLAGS.synthetic == 'ppi':       # toy-PPI shape: N=14,755, F=50, C=121 multi-label
        return utils.synthetic_graph(n_nodes=14755, feat_dim=50, num_classes=121, avg_degree=28, seed=seed,
                                     multilabel=True, val_frac=0.1, test_frac=0.1)
    if FLAGS.synthetic == 'reddit':
        return utils.reddit_shaped(seed=seed)
    if FLAGS.synthetic == 'small':
        return utils.synthetic_graph(n_nodes=3000, feat_dim=50, num_classes=7, avg_degree=8, seed=seed,
                                     multilabel=FLAGS.sigmoid)
    if not FLAGS.train_prefix:
        raise SystemExit("--train_prefix (or --synthetic) must be specified")
    return utils.load_data(FLAGS.train_prefix)


def train(G, embed_rows=None):
    from . import engine as eng
    from .minibatch import NodeMinibatchIterator
    from .models import SAGEInfo
    from .neigh_samplers import AdjInfo, CSRAdjacency, PaddedAdjacency, UniformNeighborSampler
    from .supervised_models import SupervisedGraphsage

    num_classes = G.num_classes
    features = G.padded_features()            # pad with dummy zero vector (:133-135)
    placeholders = construct_placeholders(num_classes)
    minibatch = NodeMinibatchIterator(G, None, placeholders, None, num_classes, batch_size=FLAGS.batch_size,
                                      max_degree=FLAGS.max_degree, build_padded=(FLAGS.sampler == 'padded'))
    e = eng.get_engine()
    if getattr(FLAGS, "importance_neighbors", 0):
        train_adj, test_adj = importance_adjacencies(FLAGS, minibatch, G.n_nodes, e.device)
    elif FLAGS.sampler == 'padded':
        train_adj = PaddedAdjacency(minibatch.adj, e.device)
        test_adj = PaddedAdjacency(minibatch.test_adj, e.device)
    else:
        train_adj = CSRAdjacency(minibatch.train_csr[0], minibatch.train_csr[1], G.n_nodes, e.device)
        test_adj = CSRAdjacency(minibatch.test_csr[0], minibatch.test_csr[1], G.n_nodes, e.device)
    adj_info = AdjInfo(train_adj)
    sampler = UniformNeighborSampler(adj_info, law=FLAGS.sampler_law, max_degree=FLAGS.max_degree)

    kw = dict(model_size=FLAGS.model_size, sigmoid_loss=FLAGS.sigmoid, identity_dim=FLAGS.identity_dim,
              learning_rate=FLAGS.learning_rate, weight_decay=FLAGS.weight_decay, logging=True)
    if FLAGS.model == 'graphsage_mean':       # :150-171
        if FLAGS.samples_3 != 0:
            layer_infos = [SAGEInfo("node", sampler, FLAGS.samples_1, FLAGS.dim_1),
                           SAGEInfo("node", sampler, FLAGS.samples_2, FLAGS.dim_2),
                           SAGEInfo("node", sampler, FLAGS.samples_3, FLAGS.dim_2)]
        elif FLAGS.samples_2 != 0:
            layer_infos = [SAGEInfo("node", sampler, FLAGS.samples_1, FLAGS.dim_1),
                           SAGEInfo("node", sampler, FLAGS.samples_2, FLAGS.dim_2)]
        else:
            layer_infos = [SAGEInfo("node", sampler, FLAGS.samples_1, FLAGS.dim_1)]
        model = SupervisedGraphsage(num_classes, placeholders, features, adj_info, minibatch.deg, layer_infos, **kw)
    elif FLAGS.model == 'gcn':                # :172-188
        layer_infos = [SAGEInfo("node", sampler, FLAGS.samples_1, 2 * FLAGS.dim_1),
                       SAGEInfo("node", sampler, FLAGS.samples_2, 2 * FLAGS.dim_2)]
        model = SupervisedGraphsage(num_classes, placeholders, features, adj_info, minibatch.deg,
                                    layer_infos=layer_infos, aggregator_type="gcn", concat=False, **kw)
    elif FLAGS.model in ('graphsage_maxpool', 'graphsage_meanpool', 'graphsage_seq', 'graphsage_twomaxpool',
                         'graphsage_attn'):   # :190-236
        layer_infos = [SAGEInfo("node", sampler, FLAGS.samples_1, FLAGS.dim_1),
                       SAGEInfo("node", sampler, FLAGS.samples_2, FLAGS.dim_2)]
        model = SupervisedGraphsage(num_classes, placeholders, features, adj_info, minibatch.deg,
                                    layer_infos=layer_infos, aggregator_type=FLAGS.model.split('_')[1], **kw)
    else:
        raise Exception('Error: model name unrecognized.')

    # Train model (:254-312).  Same loop, log line and validation cadence as the reference; the difference is WHERE the
    # batches come from: with the CSR sampler the shuffled epoch order and the label table live in HBM
    # (attach_device_epoch), and the steps between two host-visible events (a printed line, a validation, the end of
    # the epoch) are replayed as hipGraphs with no host round trip -- loss / preds are fetched only for the step whose
    # statistics are printed (`--feed_path host` keeps the reference's per-step feed_dict path).
    device_path = (FLAGS.sampler == 'csr' and FLAGS.feed_path == 'device')
    total_steps = 0
    avg_time = 0.0
    epoch_val_costs = []
    val_cost = val_f1_mic = val_f1_mac = 0.0
    B = FLAGS.batch_size
    if device_path:
        model.attach_device_epoch(minibatch.train_nodes, minibatch.label_matrix)

    def validate():
        adj_info.assign(test_adj)                             # sess.run(val_adj_info.op) (:280)
        if FLAGS.validate_batch_size == -1:
            res = incremental_evaluate(model, minibatch, FLAGS.batch_size)
        else:
            res = evaluate(model, minibatch, placeholders, FLAGS.validate_batch_size)
        adj_info.assign(train_adj)                            # sess.run(train_adj_info.op) (:285)
        return res

    for epoch in range(FLAGS.epochs):
        minibatch.shuffle()
        it = 0
        print('Epoch: %04d' % (epoch + 1))
        epoch_val_costs.append(0)
        if device_path:
            placeholders['dropout'].value = FLAGS.dropout
            model.set_epoch_order(minibatch.train_nodes)
            n_train = len(minibatch.train_nodes)
            n_iters = (n_train + B - 1) // B
            while it < n_iters:
                # the next iteration whose results the host looks at: a validation (it % validate_iter == 0), a printed
                # line (total_steps % print_every == 0) or the last, possibly short, batch of the epoch
                quiet = 0
                while (it + quiet < n_iters - 1 and (it + quiet) % FLAGS.validate_iter != 0
                       and (total_steps + quiet) % FLAGS.print_every != 0
                       and total_steps + quiet + 1 <= FLAGS.max_total_steps):
                    quiet += 1
                t = time.time()
                if quiet:
                    model.train_steps_device(B, quiet)                  # no host round trip
                it += quiet
                total_steps += quiet
                n = min(B, n_train - it * B)
                train_cost, preds = model.train_step_device(n, fetch=True)      # Training step (:275)
                batch_nodes = minibatch.train_nodes[it * B: it * B + n]
                labels = minibatch.label_matrix[batch_nodes]
                if it % FLAGS.validate_iter == 0:
                    val_cost, val_f1_mic, val_f1_mac, duration = validate()
                    epoch_val_costs[-1] += val_cost
                dt = (time.time() - t) / (quiet + 1)
                avg_time = (avg_time * (total_steps - quiet) + dt * (quiet + 1)) / (total_steps + 1)
                if total_steps % FLAGS.print_every == 0:
                    train_f1_mic, train_f1_mac = calc_f1(labels, preds)
                    print("Iter:", '%04d' % it,
                          "train_loss=", "{:.5f}".format(train_cost),
                          "train_f1_mic=", "{:.5f}".format(train_f1_mic),
                          "train_f1_mac=", "{:.5f}".format(train_f1_mac),
                          "val_loss=", "{:.5f}".format(val_cost),
                          "val_f1_mic=", "{:.5f}".format(val_f1_mic),
                          "val_f1_mac=", "{:.5f}".format(val_f1_mac),
                          "time=", "{:.5f}".format(avg_time))
                it += 1
                total_steps += 1
                if total_steps > FLAGS.max_total_steps:
                    break
            if total_steps > FLAGS.max_total_steps:
                break
            continue
        while not minibatch.end():
            feed_dict, labels = minibatch.next_minibatch_feed_dict()
            feed_dict.update({placeholders['dropout']: FLAGS.dropout})
            t = time.time()
            train_cost, preds = model.train_step(feed_dict)          # Training step (:275)
            if it % FLAGS.validate_iter == 0:
                val_cost, val_f1_mic, val_f1_mac, duration = validate()
                epoch_val_costs[-1] += val_cost
            avg_time = (avg_time * total_steps + time.time() - t) / (total_steps + 1)
            if total_steps % FLAGS.print_every == 0:
                train_f1_mic, train_f1_mac = calc_f1(labels, preds)
                print("Iter:", '%04d' % it,
                      "train_loss=", "{:.5f}".format(train_cost),
                      "train_f1_mic=", "{:.5f}".format(train_f1_mic),
                      "train_f1_mac=", "{:.5f}".format(train_f1_mac),
                      "val_loss=", "{:.5f}".format(val_cost),
                      "val_f1_mic=", "{:.5f}".format(val_f1_mic),
                      "val_f1_mac=", "{:.5f}".format(val_f1_mac),
                      "time=", "{:.5f}".format(avg_time))
            it += 1
            total_steps += 1
            if total_steps > FLAGS.max_total_steps:
                break
        if total_steps > FLAGS.max_total_steps:
            break

    print("Optimization Finished!")
    adj_info.assign(test_adj)
    val_cost, val_f1_mic, val_f1_mac, duration = incremental_evaluate(model, minibatch, FLAGS.batch_size)
    print("Full validation stats:",
          "loss=", "{:.5f}".format(val_cost),
          "f1_micro=", "{:.5f}".format(val_f1_mic),
          "f1_macro=", "{:.5f}".format(val_f1_mac),
          "time=", "{:.5f}".format(duration))
    with open(log_dir() + "val_stats.txt", "w") as fp:
        fp.write("loss={:.5f} f1_micro={:.5f} f1_macro={:.5f} time={:.5f}".format(val_cost, val_f1_mic, val_f1_mac, duration))
    print("Writing test set stats to file (don't peak!)")
    val_cost, val_f1_mic, val_f1_mac, duration = incremental_evaluate(model, minibatch, FLAGS.batch_size, test=True)
    with open(log_dir() + "test_stats.txt", "w") as fp:
        fp.write("loss={:.5f} f1_micro={:.5f} f1_macro={:.5f}".format(val_cost, val_f1_mic, val_f1_mac))
    kept = {}
    if FLAGS.full_inference:
        full_inference_stats(model, minibatch, G.n_nodes, keep=kept)
    if getattr(FLAGS, "correct_smooth", False) or getattr(FLAGS, "label_propagation", False):
        propagation_stats(model, minibatch, G.n_nodes, preds=kept.get("preds"))
    if embed_rows is not None:
        save_embed_nodes(model, minibatch, G.n_nodes, embed_rows, log_dir(), supervised=True)
    return val_f1_mic


def main(argv=None):
    global FLAGS
    FLAGS = build_flags(argv)
    refuse_full_inference(FLAGS)
    refuse_dropout(FLAGS)
    refuse_samples(FLAGS)
    refuse_importance(FLAGS)
    refuse_propagation(FLAGS)
    tokens = read_embed_nodes(FLAGS)
    print("Loading training data..")
    G = load_graph()
    print("Done loading training data..")
    refuse_propagation_classes(FLAGS, G.num_classes)
    return train(G, embed_nodes_rows(G, tokens, FLAGS.embed_nodes) if tokens is not None else None)


if __name__ == '__main__':
    main()
