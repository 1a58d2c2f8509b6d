"""Generate tests/golden/ref_n2v_{a,b}.npz by EXECUTING THE REFERENCE'S OWN Node2VecModel, EdgeMinibatchIterator and
run_random_walks (models.py:408-504, minibatch.py:8-176, utils.py:77-92).

    python tests/golden/make_ref_n2v_fixtures.py          # needs the reference's sources (see make_ref_fixtures.py: $GRAPHSAGE_REFERENCE)

Same machinery as make_ref_fixtures.py (imported as a module, its cases untouched); tests/tf1_n2v.py installs
tf.truncated_normal, the unique form of the candidate sampler and a version-string stand-in for networkx 1.x onto the TF1
stand-in.  Each case follows the n2v path of unsupervised_train.py:227-232 and :318-372 on the graph of make_graph():

  * Node2VecModel(placeholders, N + 1, minibatch.deg, nodevec_dim = 2 * dim_1, lr) and one training epoch over
    EdgeMinibatchIterator(context_pairs = pairs) -- steps "s0/", "s1/", ...;
  * the rows save_val_embeddings would write to val.npy: outputs1 of the (n, n) pairs of incremental_embed_feed_dict;
  * run_random_walks(G, val / test nodes, num_walks) and EdgeMinibatchIterator(context_pairs = walks, n2v_retrain = True,
    fixed_n2v = True): the walk pairs and the pruned list are stored;
  * one retrain epoch over that iterator -- further steps -- and the rows of val-test.npy.

unsupervised_train.py:324-333 re-binds the Python attribute model.context_embeds to a sum of two scatter_nd tensors after
opt_op was built; the optimizer's gradients were taken w.r.t. the Variable, so the block changes nothing that runs and is
not executed here.  What restricts the retrain phase is _n2v_prune alone.

Stored per step: batch1, batch2, neg_samples; per precision (float32 / float64 twin) loss, mrr, ranks, aff_all, outputs1 and
the touched rows of target_embeds, context_embeds and context_bias after the step (row ids under rows_target /
rows_context).  The generator asserts that some stored step has a node twice in batch1, a node twice in batch2 and a
batch2 node among the negatives, and that more nodes have non-zero train degree than the largest neg_sample_size.
"""
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import make_ref_fixtures as mrf  # noqa: E402
import tf1_n2v  # noqa: E402

tf = tf1_n2v.install(mrf.tf)
tf1_n2v.networkx_stub()
FLAGS = mrf.FLAGS

from graphsage.minibatch import EdgeMinibatchIterator  # noqa: E402
from graphsage.models import Node2VecModel  # noqa: E402
from graphsage.utils import run_random_walks  # noqa: E402

CASES = {
    # d = 2 * dim_1 = 64: the narrowest width the device kernels take
    "n2v_a": dict(dim_1=32, neg_sample_size=4, learning_rate=0.5, batch_size=16, n_pairs=40, num_walks=1, max_degree=8,
                  seed=31, np_seed=131, embed_batch=32),
    "n2v_b": dict(dim_1=32, neg_sample_size=6, learning_rate=0.05, batch_size=12, n_pairs=30, num_walks=1, max_degree=8,
                  seed=32, np_seed=132, embed_batch=25),
}


class WalkGraph(mrf.RefGraph):
    """RefGraph plus the one more accessor run_random_walks uses (utils.py:80)."""

    def degree(self, n):
        return len(self.adj[n])


def make_graph():
    G, feats, single, multi = mrf.make_graph()
    W = WalkGraph.__new__(WalkGraph)
    W.__dict__.update(G.__dict__)
    return W, feats


def make_pairs(G, cfg):
    """'Random-walk co-occurrences' among train nodes, first nodes from a pool of 10 and second nodes that favour the
    best-connected train nodes, so that a batch repeats nodes on both sides and meets the degree-weighted negatives."""
    n = len(G.node)
    prng = np.random.RandomState(cfg["np_seed"] + 1)
    train_ok = [i for i in range(n) if not (G.node[i]['val'] or G.node[i]['test'])]
    tdeg = {i: sum(1 for v in G.neighbors(i) if not G[i][v]['train_removed']) for i in train_ok}
    pool = [int(i) for i in prng.choice([i for i in train_ok if tdeg[i] > 0], 10, replace=False)]
    hubs = sorted(train_ok, key=lambda i: (-tdeg[i], i))[:6]
    pairs = []
    for _ in range(cfg["n_pairs"]):
        u = int(prng.choice(pool))
        if prng.rand() < 0.5:
            v = int(prng.choice(hubs))
        else:
            v = int(prng.choice([w for w in G.neighbors(u) if not G[u][w]['train_removed']]))
        pairs.append((u, v))
    return pairs


def run_case(cfg, real, out):
    G, feats = make_graph()
    n = len(G.node)
    id_map = {i: i for i in range(n)}
    mrf.fresh(cfg["seed"], real)
    FLAGS.learning_rate = cfg["learning_rate"]
    FLAGS.neg_sample_size = cfg["neg_sample_size"]
    placeholders = {
        'batch1': tf.placeholder(tf.int32, shape=(None), name='batch1'),
        'batch2': tf.placeholder(tf.int32, shape=(None), name='batch2'),
        'neg_samples': tf.placeholder(tf.int32, shape=(None,), name='neg_sample_size'),
        'dropout': tf.placeholder_with_default(0., shape=(), name='dropout'),
        'batch_size': tf.placeholder(tf.int32, name='batch_size'),
    }
    pairs = make_pairs(G, cfg)
    np.random.seed(cfg["np_seed"])
    random.seed(cfg["np_seed"])
    it = EdgeMinibatchIterator(G, id_map, placeholders, batch_size=cfg["batch_size"], max_degree=cfg["max_degree"],
                               num_neg_samples=cfg["neg_sample_size"], context_pairs=pairs)
    assert int((it.deg > 0).sum()) > max(c["neg_sample_size"] for c in CASES.values()), "unique negatives would never end"
    features = np.vstack([feats, np.zeros((feats.shape[1],))])
    # unsupervised_train.py:227-232
    model = Node2VecModel(placeholders, features.shape[0], it.deg, nodevec_dim=2 * cfg["dim_1"], lr=FLAGS.learning_rate)
    variables = {"target": model.target_embeds, "context": model.context_embeds, "bias": model.context_bias}
    assert set(map(id, variables.values())) == set(map(id, tf.trainable_variables()))
    sess = tf.Session()
    sess.run(tf.global_variables_initializer())
    pre = real[-2:]
    if real == "float32":
        out["graph/val"] = np.asarray([G.node[i]['val'] for i in range(n)])
        out["graph/test"] = np.asarray([G.node[i]['test'] for i in range(n)])
        out["graph/deg"] = it.deg.astype(np.int64)
        out["graph/pairs"] = np.asarray(pairs, np.int32)
        out["graph/train_edges"] = np.asarray(it.train_edges, np.int32)
        full = [G.neighbors(i) for i in range(n)]
        out["graph/full_rowptr"], out["graph/full_col"] = mrf.csr_of(full)
        for k, v in variables.items():
            out["init/" + k] = sess.run(v).astype(np.float32)
    else:
        for k, v in variables.items():
            assert np.array_equal(out["init/" + k], sess.run(v).astype(np.float32)), "the twin run starts elsewhere"

    state = {"step": 0, "dups": False}

    def train_epoch(iterator):
        iterator.shuffle()
        while not iterator.end():
            feed = iterator.next_minibatch_feed_dict()
            feed.update({placeholders['dropout']: 0.0})
            # unsupervised_train.py:273-274 / :356-357
            res = sess.run([model.opt_op, model.loss, model.ranks, model.aff_all, model.mrr, model.outputs1,
                            model.neg_samples], feed_dict=feed)
            p = "s%d/" % state["step"]
            b1 = np.asarray(feed[placeholders['batch1']], np.int32)
            b2 = np.asarray(feed[placeholders['batch2']], np.int32)
            neg = res[6].astype(np.int32)
            assert len(set(neg.tolist())) == len(neg) and (it.deg[neg] > 0).all()
            if real == "float32":
                out[p + "batch1"], out[p + "batch2"], out[p + "neg_samples"] = b1, b2, neg
                out[p + "rows_target"] = np.unique(b1).astype(np.int32)
                out[p + "rows_context"] = np.unique(np.concatenate([b2, neg])).astype(np.int32)
            else:
                assert np.array_equal(out[p + "neg_samples"], neg) and np.array_equal(out[p + "batch1"], b1)
            if (len(set(b1.tolist())) < len(b1) and len(set(b2.tolist())) < len(b2) and set(b2.tolist()) & set(neg.tolist())):
                state["dups"] = True
            out[p + pre + "/loss"] = np.asarray(res[1])
            out[p + pre + "/ranks"] = res[2]
            out[p + pre + "/aff_all"] = res[3]
            out[p + pre + "/mrr"] = np.asarray(res[4])
            out[p + pre + "/outputs1"] = res[5]
            out[p + pre + "/after/target"] = sess.run(model.target_embeds)[out[p + "rows_target"]]
            out[p + pre + "/after/context"] = sess.run(model.context_embeds)[out[p + "rows_context"]]
            out[p + pre + "/after/bias"] = sess.run(model.context_bias)[out[p + "rows_context"]]
            state["step"] += 1

    def embeddings(tag):
        """The loop of save_val_embeddings (unsupervised_train.py:94-117) over the FIRST iterator: rows of val<mod>.npy"""
        rows, nodes, seen = [], [], set()
        finished, iter_num = False, 0
        while not finished:
            feed, finished, edges = it.incremental_embed_feed_dict(cfg["embed_batch"], iter_num)
            iter_num += 1
            o1 = sess.run([model.loss, model.mrr, model.outputs1], feed_dict=feed)[-1]
            for i, edge in enumerate(edges):
                if edge[0] not in seen:
                    rows.append(o1[i, :])
                    nodes.append(edge[0])
                    seen.add(edge[0])
        if real == "float32":
            out[tag + "/nodes"] = np.asarray(nodes, np.int32)
        out[tag + "/" + pre + "/emb"] = np.vstack(rows)

    train_epoch(it)
    out["n_train_steps"] = np.asarray(state["step"])
    embeddings("val")
    # unsupervised_train.py:335-349
    nodes = [v for v in G.nodes() if G.node[v]["val"] or G.node[v]["test"]]
    walks = run_random_walks(G, nodes, num_walks=cfg["num_walks"])
    test_it = EdgeMinibatchIterator(G, id_map, placeholders, batch_size=cfg["batch_size"], max_degree=cfg["max_degree"],
                                    num_neg_samples=cfg["neg_sample_size"], context_pairs=walks, n2v_retrain=True,
                                    fixed_n2v=True)
    if real == "float32":
        out["retrain/walk_pairs"] = np.asarray(walks, np.int32)
        out["retrain/train_edges"] = np.asarray(test_it.train_edges, np.int32)
        out["retrain/val_set_size"] = np.asarray(test_it.val_set_size)
    else:
        assert np.array_equal(out["retrain/train_edges"], np.asarray(test_it.train_edges, np.int32))
    assert 0 < len(test_it.train_edges) < len(walks), "the prune must drop some pairs and keep some"
    train_epoch(test_it)
    embeddings("val-test")
    out["n_steps"] = np.asarray(state["step"])
    assert state["dups"], "no stored step repeats a node in batch1, one in batch2 and has a batch2 node among the negatives"


def main():
    torch.set_num_threads(1)           # one summation order: a re-run reproduces every array bit for bit
    only = set(sys.argv[1:])
    for name, cfg in CASES.items():
        if only and name not in only:
            continue
        out = {"cfg": np.asarray(json.dumps(dict(cfg, kind="n2v")))}
        for real in ("float32", "float64"):
            run_case(cfg, real, out)
        mrf.save(name, out)


if __name__ == "__main__":
    main()
