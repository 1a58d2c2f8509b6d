"""CPU suite of the node2vec baseline: the NumPy restatement (tests/n2v_oracle.py) == the REFERENCE'S OWN Node2VecModel.

tests/golden/ref_n2v_*.npz hold what graphsage/models.py:408-504, minibatch.py and utils.py:77-92 computed when executed
unmodified on the TF1 stand-in (tests/golden/make_ref_n2v_fixtures.py).  Tolerances are those of tests/test_ref_pin.py:
the float64 twin at 1e-9, float32 at 1e-4.  Also here: the host restatement of the distinct-negatives sampler against the
with-replacement law already pinned (oracle/sampler_hash.py), the iterator's retrain forms, and the C ABI at version 12.
"""
import os
import re

import numpy as np
import pytest

import n2v_oracle
from n2v_oracle import N2V, Fixture
from oracle import sampler_hash
from test_ref_pin import DT, close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables_before(fx, s, prec):
    return fx.tables_before(s, DT[prec])


@pytest.mark.parametrize("name", N2V)
def test_fixture_holds_the_duplicate_cases_and_large_steps(name):
    fx = Fixture(name)
    n_steps, n_neg, lr = fx.n_steps, fx.cfg["neg_sample_size"], fx.cfg["learning_rate"]
    assert int((fx["graph/deg"] > 0).sum()) > n_neg
    found = False
    for s in range(n_steps):
        p = "s%d/" % s
        b1, b2, neg = fx[p + "batch1"], fx[p + "batch2"], fx[p + "neg_samples"]
        assert len(neg) == n_neg and len(np.unique(neg)) == n_neg, "unique=True"
        assert (fx["graph/deg"][neg] > 0).all()
        found |= len(np.unique(b1)) < len(b1) and len(np.unique(b2)) < len(b2) and len(np.intersect1d(b2, neg)) > 0
        # one step moves the touched rows far above the comparison tolerance
        t, _, _ = tables_before(fx, s, "32")
        moved = np.abs(fx[p + "32/after/target"] - t[fx[p + "rows_target"]]).max()
        assert moved > 100 * 1e-4 * lr
    assert found


@pytest.mark.parametrize("prec", ["64", "32"])
@pytest.mark.parametrize("name", N2V)
def test_restatement_equals_the_reference_every_step(name, prec):
    fx = Fixture(name)
    lr = fx.cfg["learning_rate"]
    for s in range(fx.n_steps):
        p = "s%d/" % s
        t, c, b = tables_before(fx, s, prec)
        b1, b2, neg = fx[p + "batch1"], fx[p + "batch2"], fx[p + "neg_samples"]
        res = n2v_oracle.step(t, c, b, b1, b2, neg, lr=lr)
        q = p + prec + "/"
        close(res["loss"], fx[q + "loss"], prec, "loss step %d" % s)
        close(res["aff_all"], fx[q + "aff_all"], prec, "aff_all")
        close(res["outputs1"], fx[q + "outputs1"], prec, "outputs1")
        ref_aff = fx[q + "aff_all"]
        margin = np.abs(ref_aff[:, :-1] - ref_aff[:, -1:]).min(axis=1) > 1e-4           # float near-ties aside
        # models.py:500-502: ranks[:, -1] is the rank of the true pair
        assert np.array_equal(res["rank_true"][margin], fx[q + "ranks"][:, -1][margin])
        if margin.all():
            close(res["mrr"], fx[q + "mrr"], prec, "mrr")
        close(res["target"][fx[p + "rows_target"]], fx[q + "after/target"], prec, "target rows after step %d" % s)
        close(res["context"][fx[p + "rows_context"]], fx[q + "after/context"], prec, "context rows after step %d" % s)
        close(res["bias"][fx[p + "rows_context"]], fx[q + "after/bias"], prec, "bias after step %d" % s)
        # nothing else moves
        rest_t = np.setdiff1d(np.arange(len(t)), fx[p + "rows_target"])
        rest_c = np.setdiff1d(np.arange(len(c)), fx[p + "rows_context"])
        assert np.array_equal(res["target"][rest_t], t[rest_t]) and np.array_equal(res["context"][rest_c], c[rest_c])
        assert np.array_equal(res["bias"][rest_c], b[rest_c])


@pytest.mark.parametrize("name", N2V)
def test_saved_embeddings_are_the_target_rows(name):
    """save_val_embeddings (unsupervised_train.py:94-117) stores outputs1 = target_embeds[batch1] of the (n, n) pairs."""
    fx = Fixture(name)
    t_train, _, _ = tables_before(fx, fx.n_train_steps, "64")
    t_end, _, _ = tables_before(fx, fx.n_steps, "64")
    assert len(np.unique(fx["val/nodes"])) == len(fx["val/nodes"])
    close(t_train[fx["val/nodes"]], fx["val/64/emb"], "64")
    close(t_end[fx["val-test/nodes"]], fx["val-test/64/emb"], "64")


def graph_of(fx):
    from graphsage_amd.utils import GraphData
    rp, col = fx["graph/full_rowptr"], fx["graph/full_col"]
    n = len(rp) - 1
    src = np.repeat(np.arange(n), np.diff(rp))
    keep = src < col                                                   # one entry per undirected edge
    return GraphData(n, src[keep], col[keep], None, np.zeros(n, np.int64), fx["graph/val"], fx["graph/test"])


def pair_multiset(a):
    a = np.asarray(a).reshape(-1, 2)
    return sorted(map(tuple, a.tolist()))


@pytest.mark.parametrize("name", N2V)
def test_iterator_retrain_forms_match_the_reference(name):
    """minibatch.py:39-58.  The order differs (the reference's iterator also draws its padded tables from the global NumPy
    stream); the pair SETS, with multiplicity, must be equal."""
    from graphsage_amd.minibatch import EdgeMinibatchIterator
    fx = Fixture(name)
    G = graph_of(fx)
    ph = {k: k for k in ("batch1", "batch2", "batch_size", "dropout")}
    walks = fx["retrain/walk_pairs"]
    it = EdgeMinibatchIterator(G, None, ph, context_pairs=walks, batch_size=fx.cfg["batch_size"], max_degree=fx.cfg["max_degree"],
                               n2v_retrain=True, fixed_n2v=True, build_padded=False)
    assert pair_multiset(it.train_edges) == pair_multiset(fx["retrain/train_edges"])
    assert it.val_edges is it.train_edges and it.val_set_size == int(fx["retrain/val_set_size"])
    no_train = fx["graph/val"] | fx["graph/test"]
    assert not no_train[it.train_edges[:, 1]].any() and len(it.train_edges) < len(walks)
    # n2v_retrain without fixed_n2v keeps every pair, isolated endpoints included
    it2 = EdgeMinibatchIterator(G, None, ph, context_pairs=walks, n2v_retrain=True, build_padded=False)
    assert pair_multiset(it2.train_edges) == pair_multiset(walks) and it2.val_edges is it2.train_edges
    # the ordinary iterator is unchanged
    it3 = EdgeMinibatchIterator(G, None, ph, context_pairs=fx["graph/pairs"], batch_size=fx.cfg["batch_size"],
                                max_degree=fx.cfg["max_degree"], build_padded=False)
    assert pair_multiset(it3.train_edges) == pair_multiset(fx["graph/train_edges"])
    assert np.array_equal(it3.deg, fx["graph/deg"])
    assert len(it3.val_edges) == int(G.train_removed.sum())
    feed = it.next_minibatch_feed_dict()
    assert len(feed["batch1"]) == min(fx.cfg["batch_size"], len(it.train_edges))


@pytest.mark.parametrize("n_neg,seed,clock,slot_offset", [(1, 123, 0, 0), (6, 123, 1, 0), (20, 7, 5, 1024), (40, 99, 2 ** 33, 3)])
def test_unique_sampler_is_the_first_distinct_of_the_pinned_stream(n_neg, seed, clock, slot_offset):
    """The identity that carries the pinned with-replacement law over: no new statistical test."""
    rng = np.random.RandomState(n_neg)
    deg = rng.randint(0, 30, size=300)
    deg[rng.choice(300, 120, replace=False)] = 0                       # val / test nodes: weight 0
    deg[:3] = 400                                                      # hubs: the stream repeats them often
    deg[-1] = 0
    cdf = sampler_hash.unigram_cdf_u32(deg)
    assert n2v_oracle.reachable_nodes(cdf) == int((deg > 0).sum())
    got = n2v_oracle.sample_unigram_unique(cdf, n_neg, seed, clock, slot_offset)
    assert got.dtype == np.int32 and len(got) == n_neg and len(np.unique(got)) == n_neg
    assert (deg[got] > 0).all(), "a node of weight zero was drawn"
    stream = sampler_hash.sample_unigram(cdf, 4096, seed, clock, slot_offset)
    _, first = np.unique(stream, return_index=True)
    want = stream[np.sort(first)][:n_neg]
    assert np.array_equal(got, want)


def test_unique_sampler_refuses_what_cannot_end():
    deg = np.zeros(50, np.int64)
    deg[[3, 7, 9]] = 5
    cdf = sampler_hash.unigram_cdf_u32(deg)
    assert n2v_oracle.reachable_nodes(cdf) == 3
    assert sorted(n2v_oracle.sample_unigram_unique(cdf, 3, 1, 0).tolist()) == [3, 7, 9]
    with pytest.raises(ValueError):
        n2v_oracle.sample_unigram_unique(cdf, 4, 1, 0, max_draws=64 * 64)


def test_library_exports_the_n2v_entry_points_at_abi_12():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    assert re.search(r"#define GS_ABI_VERSION 12\b", header) and _lib.GS_ABI_VERSION == 12
    declared = sorted(set(re.findall(r"\b(gs_n2v_[a-z0-9_]+)\s*\(", header)))
    assert declared == ["gs_n2v_apply", "gs_n2v_fwd_bwd", "gs_n2v_slabs", "gs_n2v_stage", "gs_n2v_supported"]
    lib = _lib.load()
    assert lib.gs_abi_version() == 12
    for name in declared:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
    # shapes: every width of the link-prediction kernel takes the default 20 negatives; anything else is refused
    for d in (64, 128, 256, 512):
        assert lib.gs_n2v_supported(d, 20) == 1 and lib.gs_n2v_supported(d, 1) == 1
        assert lib.gs_n2v_slabs(512, d, 20) in (128, 256, 512)
    assert lib.gs_n2v_supported(100, 20) == 0 and lib.gs_n2v_supported(512, 0) == 0 and lib.gs_n2v_supported(512, 1000) == 0


def test_stand_in_additions_behave_as_documented():
    """tests/tf1_n2v.py: truncated_normal stays within two standard deviations and has the normal's shape inside them;
    the unique candidate sampler returns distinct classes of non-zero weight and leaves the with-replacement form alone."""
    import sys
    shim_dir = os.path.join(ROOT, "tests", "tf1_shim")
    sys.path.insert(0, shim_dir)
    try:
        import tensorflow as tf
        import tf1_n2v
        tf1_n2v.install(tf)
        tf.reset_default_graph()
        tf.set_random_seed(5)
        sess = tf.Session()
        x = sess.run(tf.truncated_normal([4000, 8], stddev=0.125))
        assert x.dtype == np.float32 and np.abs(x).max() <= 0.25 and abs(x.mean()) < 0.01
        assert abs(x.std() - 0.125 * 0.8796) < 0.005            # std of a normal truncated at two sigma: 0.8796 sigma
        unigrams = [0, 5, 0, 1, 9, 0, 2, 7]
        labels = tf.constant(np.zeros((3, 1), np.int64))
        s, _, _ = tf.nn.fixed_unigram_candidate_sampler(true_classes=labels, num_true=1, num_sampled=5, unique=True,
                                                        range_max=8, distortion=0.75, unigrams=unigrams)
        for _ in range(20):
            got = sess.run(s)
            assert sorted(got.tolist()) == [1, 3, 4, 6, 7]
        r, _, _ = tf.nn.fixed_unigram_candidate_sampler(true_classes=labels, num_true=1, num_sampled=50, unique=False,
                                                        range_max=8, distortion=0.75, unigrams=unigrams)
        got = sess.run(r)
        assert len(got) == 50 and set(got.tolist()) <= {1, 3, 4, 6, 7}
    finally:
        sys.path.remove(shim_dir)
