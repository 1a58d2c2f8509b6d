"""What the reference's Node2VecModel (models.py:408-504) and run_random_walks (utils.py:77-92) need beyond the TF1 stand-in
of tests/tf1_shim -- TEST INFRASTRUCTURE ONLY, installed at run time by tests/golden/make_ref_n2v_fixtures.py (as tests/tf1_rnn.py
is for the LSTM cell); the stand-in's own module is not changed.  Semantics follow TF 1.x's published documentation:

  tf.truncated_normal(shape, mean, stddev): normal draws, values further than 2 stddev from the mean are dropped and
      re-drawn.  Drawn from the stand-in's NumPy stream and rounded to float32 also in the float64 twin run (as its
      random_uniform), so both runs start from identical tables.
  tf.nn.fixed_unigram_candidate_sampler(unique=True): draws from P(class) ~ unigrams[class]**distortion are repeated until
      num_sampled DISTINCT classes were seen (rejection); kept in the order of first occurrence, logged like the
      with-replacement form (tf.shim.log["unigram"]).  unique=False goes to the stand-in's own function.
  networkx: graphsage/utils.py asserts networkx <= 1.11 at import and touches it nowhere else on the way to
      run_random_walks, which needs only G.degree(n) and G.neighbors(n); `networkx_stub()` is a module object that carries
      the version string and the one submodule utils.py imports.
"""
import sys
import types

import numpy as np
import torch


def install(tf):
    shim = tf.shim
    with_replacement = tf.nn.fixed_unigram_candidate_sampler

    def truncated_normal(shape, mean=0.0, stddev=1.0, dtype=tf.float32, seed=None, name=None):
        def draw(s):
            shape_ = tf._shape_list(s)
            n = int(np.prod(shape_))
            out = np.empty(0, np.float64)
            while out.size < n:
                z = shim.rng.standard_normal(n - out.size)
                out = np.concatenate([out, z[np.abs(z) <= 2.0]])
            v = (mean + stddev * out.reshape(shape_)).astype(np.float32)
            return tf._as_torch(v, dtype.torch())
        return tf.Tensor(draw, (shape,))

    def fixed_unigram_candidate_sampler(true_classes, num_true, num_sampled, unique, range_max, vocab_file="",
                                        distortion=1.0, num_reserved_ids=0, num_shards=1, shard=0, unigrams=(), seed=None,
                                        name=None):
        if not unique:
            return with_replacement(true_classes, num_true, num_sampled, unique, range_max, vocab_file, distortion,
                                    num_reserved_ids, num_shards, shard, unigrams, seed, name)
        assert num_true == 1 and len(unigrams) == range_max
        w = np.asarray(unigrams, dtype=np.float64) ** distortion
        p = w / w.sum()
        assert int((p > 0).sum()) >= num_sampled, "unique=True with fewer than num_sampled classes of non-zero weight never ends"

        def run(_true):
            kept = []
            while len(kept) < num_sampled:
                c = int(shim.rng.choice(range_max, p=p))
                if c not in kept:
                    kept.append(c)
            s = np.asarray(kept, dtype=np.int64)
            shim.log["unigram"].append((id(sampled), s.copy()))
            return torch.as_tensor(s, dtype=torch.int64)
        sampled = tf.Tensor(run, (true_classes,))
        # expected counts of the unique form: 1 - (1 - p)^num_tries; the reference discards them (models.py:449)
        true_exp = tf._op(lambda t: tf._as_torch(p[t.numpy()] * num_sampled), true_classes)
        samp_exp = tf._op(lambda s: tf._as_torch(p[s.numpy()] * num_sampled), sampled)
        return sampled, true_exp, samp_exp

    tf.truncated_normal = truncated_normal
    tf.nn.fixed_unigram_candidate_sampler = fixed_unigram_candidate_sampler
    return tf


def networkx_stub():
    """Put a module named networkx with __version__ 1.11 into sys.modules (unless a real 1.x is importable)."""
    try:
        import networkx as nx
        major, minor = [int(x) for x in nx.__version__.split('.')[:2]]
        if major <= 1 and minor <= 11:
            return nx
    except Exception:
        pass
    nx = types.ModuleType("networkx")
    nx.__version__ = "1.11"
    rw = types.ModuleType("networkx.readwrite")
    jg = types.ModuleType("networkx.readwrite.json_graph")
    rw.json_graph = jg
    nx.readwrite = rw
    sys.modules["networkx"] = nx
    sys.modules["networkx.readwrite"] = rw
    sys.modules["networkx.readwrite.json_graph"] = jg
    return nx
