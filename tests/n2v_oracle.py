"""NumPy restatement of the node2vec baseline (graphsage/models.py:408-504, Node2VecModel) and of the device's
distinct-negatives sampler -- TEST INFRASTRUCTURE ONLY (precedent: tests/seq_oracle.py).

  step(target, context, bias, batch1, batch2, neg, lr, train)   one sess.run of [opt_op, loss, ranks, aff_all, mrr, outputs1]
  sample_unigram_unique(cdf, n_neg, seed, clock, slot_offset)   gs_n2v_stage's negatives, bit for bit
  reachable_nodes(cdf)                                          how many nodes the cdf can draw at all
  Fixture(name)                                                 loader of tests/golden/ref_n2v_*.npz

Written from the reference's formulas, in whatever precision the arrays come in (float64 pins the algebra to the
reference's float64 run; float32 is what the HIP path is compared with).
"""
import json
import os

import numpy as np

from oracle import sampler_hash

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N2V = ["n2v_a", "n2v_b"]


class Fixture(object):
    """tests/golden/ref_<name>.npz of make_ref_n2v_fixtures.py: arrays by key, the case's settings under .cfg"""

    def __init__(self, name):
        self.name = name
        self.z = np.load(os.path.join(GOLDEN, "ref_%s.npz" % name))
        self.cfg = json.loads(str(self.z["cfg"]))
        self.d = 2 * self.cfg["dim_1"]
        self.n_neg = self.cfg["neg_sample_size"]
        self.lr = self.cfg["learning_rate"]
        self.n_steps = int(self.z["n_steps"])
        self.n_train_steps = int(self.z["n_train_steps"])

    def __getitem__(self, k):
        return self.z[k]

    def tables_before(self, s, dtype):
        """The three variables as the reference held them before step s: the initial values with every stored touched row
        of the earlier steps written over them."""
        prec = "64" if np.dtype(dtype) == np.float64 else "32"
        t, c, b = (self.z["init/" + k].astype(dtype) for k in ("target", "context", "bias"))
        for k in range(s):
            p = "s%d/" % k
            t[self.z[p + "rows_target"]] = self.z[p + prec + "/after/target"]
            c[self.z[p + "rows_context"]] = self.z[p + prec + "/after/context"]
            b[self.z[p + "rows_context"]] = self.z[p + prec + "/after/bias"]
        return t, c, b


def _xent(logits, label):
    """tf.nn.sigmoid_cross_entropy_with_logits: max(x, 0) - x z + log(1 + exp(-|x|))"""
    return np.maximum(logits, 0) - logits * label + np.log1p(np.exp(-np.abs(logits)))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def step(target, context, bias, batch1, batch2, neg, lr=0.0, train=True):
    """Returns a dict: loss, aff_all [B, n_neg + 1] (negatives first, WITHOUT the bias: models.py:489-500 goes through
    BipartiteEdgePredLayer.affinity / neg_cost), ranks (of the true pair among its row, ties to the lower column as
    tf.nn.top_k), mrr, outputs1, and when train: the gradients per SLOT and the three arrays after
    GradientDescentOptimizer(lr): gradients of repeated rows are summed, then subtracted once (indexed slices).
    The inputs are not modified."""
    batch1, batch2, neg = (np.asarray(a, dtype=np.int64) for a in (batch1, batch2, neg))
    B = len(batch1)
    dt = target.dtype
    o1, o2, no = target[batch1], context[batch2], context[neg]
    aff = (o1 * o2).sum(axis=1)
    nav = o1 @ no.T
    affb = aff + bias[batch2]
    navb = nav + bias[neg][None, :]
    loss = (_xent(affb, 1.0).sum() + _xent(navb, 0.0).sum()) / dt.type(B)
    aff_all = np.concatenate([nav, aff[:, None]], axis=1)
    ranks_true = (nav >= aff[:, None]).sum(axis=1)
    out = {"loss": loss, "aff_all": aff_all, "rank_true": ranks_true, "mrr": (1.0 / (ranks_true + 1.0)).astype(dt).mean(),
           "outputs1": o1.copy()}
    if not train:
        return out
    da = (_sigmoid(affb) - 1.0) / dt.type(B)                 # d loss / d (aff + bias)
    gq = _sigmoid(navb) / dt.type(B)                         # [B, n_neg]
    g_target = da[:, None] * o2 + gq @ no
    g_ctx = da[:, None] * o1
    g_neg = gq.T @ o1
    gb_neg = gq.sum(axis=0)
    t2, c2, b2 = target.copy(), context.copy(), bias.copy()
    dT, dC, dB = np.zeros_like(target), np.zeros_like(context), np.zeros_like(bias)
    np.add.at(dT, batch1, g_target)
    np.add.at(dC, neg, g_neg)
    np.add.at(dC, batch2, g_ctx)
    np.add.at(dB, neg, gb_neg)
    np.add.at(dB, batch2, da)
    lr = dt.type(lr)
    rows_t = np.unique(batch1)
    rows_c = np.unique(np.concatenate([batch2, neg]))
    t2[rows_t] -= lr * dT[rows_t]
    c2[rows_c] -= lr * dC[rows_c]
    b2[rows_c] -= lr * dB[rows_c]
    out.update(g_target=g_target, g_ctx=g_ctx, g_bias=da, g_neg=g_neg, gb_neg=gb_neg, target=t2, context=c2, bias=b2,
               rows_target=rows_t, rows_context=rows_c)
    return out


def reachable_nodes(cdf):
    """Number of nodes some 32-bit draw below 2^32 - 1 maps to: i is drawn iff cdf[i] > cdf[i - 1]."""
    c = np.concatenate([[0], np.asarray(cdf, dtype=np.uint64)])
    return int((c[1:] > c[:-1]).sum())


def sample_unigram_unique(cdf, n_neg, seed, clock, slot_offset=0, chunk=64, max_draws=64 * 4096):
    """The first n_neg DISTINCT nodes of the with-replacement stream oracle.sampler_hash.sample_unigram(cdf, ., seed, clock,
    slot_offset) -- draw t is keyed by slot_offset + t -- in stream order (gs_n2v_stage walks it 64 draws at a time)."""
    kept, seen = [], set()
    t0 = 0
    while len(kept) < n_neg and t0 < max_draws:
        draws = sampler_hash.sample_unigram(cdf, chunk, seed, clock, slot_offset + t0)
        for v in draws.tolist():
            if v not in seen:
                seen.add(v)
                kept.append(v)
                if len(kept) == n_neg:
                    break
        t0 += chunk
    if len(kept) < n_neg:
        raise ValueError("fewer than %d distinct nodes in %d draws" % (n_neg, max_draws))
    return np.asarray(kept, dtype=np.int32)
