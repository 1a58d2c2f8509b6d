"""-m gpu: the attention-pooling aggregator (graphsage_attn) on the device.

  * gs_segment_attn_fwd / _bwd against the float64 oracle (tests/attn_oracle.py) at the edges of their range, with and without
    the distinct-id index, inside NaN canaries, scores spread over +-80, equal scores, s = 1, an all-zero group, several slab
    counts, refused shapes, two runs bit-equal;
  * GS_CSR_SOFTMAX in the window and the row-list form on a graph with an empty row, rows at the split length, a hub of three
    partials whose scores differ by 160 between partials, duplicate entries;
  * supervised and unsupervised model steps against the oracle on the oracle's sampled neighbor sets: loss, predictions, every
    gradient (the gate's included) and the parameters after three Adam steps;
  * embed_full / predict_full / embed_nodes / rank_full / topk_full; both training drivers as fresh child processes.

Every float comparison is `close` of tests/test_ref_pin_gpu.py (rtol 1e-4, atol 1e-4 of the largest expected magnitude), the
criterion of tests/test_twomax_gpu.py; ids and integers are exact.  Parameters after Adam are compared outside Adam's knee
(test_ref_pin_gpu.ADAM_KNEE: below it a gradient difference far inside the gradient tolerance moves the parameter by the whole
step), over the elements whose gradient was outside it in EVERY step so far."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_oracle as ao
import fullnbr_oracle as fo
from graphsage_amd import engine as eng
from graphsage_amd import inits, ops
from graphsage_amd._lib import CSR_SOFTMAX, GraphsageAmdError
from graphsage_amd.inference import SPLIT_LEN, FullGraph
from graphsage_amd.ops import Mat
from oracle import graphsage_oracle as orc
from test_full_inference_gpu import files_under
from test_ref_pin_gpu import ADAM_KNEE, RTOL, close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _sync():
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# the two segment launches
# ---------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 4), (5, 2, 36), (33, 3, 512), (5, 10, 1024), (33, 25, 512), (5, 64, 36), (1, 128, 1024), (33, 128, 1024),
          (33, 1, 1024), (1, 128, 4)]


def canaried(dev, a, pad_cols=8, pad_rows=2):
    """`a` [rows, d] inside a NaN-filled [rows + pad_rows, d + pad_cols] buffer: (Mat over the rows, the whole buffer)."""
    rows, d = a.shape
    big = torch.full((rows + pad_rows, d + pad_cols), NAN, dtype=torch.float32, device=dev)
    big[:rows, :d] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return Mat(big[:rows], d), big


def untouched(big, rows, d):
    g = big.cpu().numpy()
    return np.isnan(g[rows:]).all() and np.isnan(g[:, d:]).all()


def segment_case(n, s, hidden, indexed, seed, spread=80.0):
    """(V rows table [m, hidden] >= 0, inv or None, a, dP).

    spread > 10: the scores span [-spread, spread], chosen per sample and reached by scaling the sample's row.  Two things keep
    such a case inside what float32 can hold to 1e-4, so that the comparison measures the kernel and not the data:
      * a score of magnitude 80 must be exact to 1e-4 ABSOLUTE for its softmax weight to be exact to 1e-4 relative, about ten
        float32 ulps of it: every row lives on the columns where the gate has ONE sign (relu zeros in between), so its dot
        product has no cancellation;
      * da = sum dt_j V_j with dt_j = alpha_j (g_j - G) vanishes where one row takes all the weight (g_j - G is then the
        rounding error of g_j): the two best rows of a group score within 0.7 of each other, so dt is of the size of its terms.
    With an index the first two thirds of the samples own their row and the last third re-use random ones.
    spread <= 10: relu(randn) rows, scaled to scores in [-spread, spread] (0: left as they are)."""
    rng = np.random.RandomState(seed)
    rows = n * s
    m = max(1, (rows * 2) // 3) if indexed else rows
    a = rng.randn(hidden).astype(np.float32)
    a[0], a[1] = abs(a[0]) + 0.5, -abs(a[1]) - 0.5
    dP = rng.randn(n, hidden).astype(np.float32)
    if spread > 10:
        top = rng.uniform(20.0, spread, size=n)
        top[0] = spread
        target = rng.uniform(-spread, top[:, None] - 3.0, size=(n, s))
        target[:, 0] = top
        if s > 1:
            target[:, 1] = top - 0.7
        if s > 2:
            target[0, 2] = -spread
        elif n > 1:
            target[1] = -spread + 0.7 * np.arange(s)[::-1]
        target = target.reshape(-1)[:m]
        side = (target > 0)[:, None] == (a > 0)[None, :]
        table = np.where(side, np.maximum(rng.randn(m, hidden) + 0.5, 0), 0)
        table[:, :2] = np.where(side[:, :2], 0.7, 0)                         # no row without a score
        table = (table * (target / (table @ a.astype(np.float64)))[:, None]).astype(np.float32)
    else:
        table = np.maximum(rng.randn(m, hidden), 0).astype(np.float32)
        if spread:
            raw = table.astype(np.float64) @ a.astype(np.float64)
            target = np.sign(raw) * rng.uniform(0.0, spread, size=m)
            scale = np.where(np.abs(raw) > 0.1, target / np.where(raw == 0, 1.0, raw), 1.0)
            table = (table * scale[:, None]).astype(np.float32)
    inv = None
    if indexed:
        inv = np.concatenate([np.arange(m), rng.randint(0, m, size=rows - m)]).astype(np.int32)
        if n > 1 and s >= 3:
            inv[s + 2] = inv[s]                                               # a repeated id inside one group
        elif n == 1 and s >= 4:
            inv[3] = inv[0]
    return table, inv, a, dP


def run_segment(dev, table, inv, a, dP, n, s, n_slabs=3):
    hidden = table.shape[1]
    H, H_big = canaried(dev, table)
    inv_d = torch.from_numpy(inv).to(dev) if inv is not None else None
    a_d = torch.from_numpy(a).to(dev)
    pooled, pooled_big = canaried(dev, np.zeros((n, hidden), np.float32))
    pooled_big.fill_(NAN)
    alpha = torch.full((n * s + 5,), NAN, dtype=torch.float32, device=dev)
    dPm, _ = canaried(dev, dP)
    dV, dV_big = canaried(dev, np.zeros((n * s, hidden), np.float32))
    dV_big.fill_(NAN)
    slabs = torch.full(((n_slabs + 1) * hidden,), NAN, dtype=torch.float32, device=dev)
    _sync()
    ops.segment_attn_fwd(H, inv_d, a_d, n, s, pooled, alpha)
    ops.segment_attn_bwd(dPm, H, inv_d, a_d, alpha, n, s, dV, n_slabs, slabs.data_ptr())
    _sync()
    assert untouched(pooled_big, n, hidden) and untouched(dV_big, n * s, hidden), "a canary around pooled / dV was written"
    assert np.isnan(alpha[n * s:].cpu().numpy()).all() and np.isnan(slabs[n_slabs * hidden:].cpu().numpy()).all()
    assert np.array_equal(np.isnan(H_big.cpu().numpy()), np.isnan(canaried(dev, table)[1].cpu().numpy()))
    return (pooled.numpy(), alpha[:n * s].cpu().numpy().reshape(n, s), dV.numpy(),
            slabs[:n_slabs * hidden].cpu().numpy().reshape(n_slabs, hidden))


def oracle_segment(table, inv, a, dP, n, s):
    V = table.astype(np.float64)[inv if inv is not None else np.arange(n * s)].reshape(n, s, -1)
    pooled, alpha = ao.segment_attn_fwd(V, a.astype(np.float64))
    dV, da, dt = ao.segment_attn_bwd(dP.astype(np.float64), V, a.astype(np.float64), alpha)
    return pooled, alpha, dV.reshape(n * s, -1), da, dt


@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("n,s,hidden", SHAPES)
def test_segment_kernels_equal_the_oracle(dev, n, s, hidden, indexed):
    table, inv, a, dP = segment_case(n, s, hidden, indexed, seed=n + 7 * s + hidden)
    pooled, alpha, dV, slabs = run_segment(dev, table, inv, a, dP, n, s)
    w_pooled, w_alpha, w_dV, w_da, w_dt = oracle_segment(table, inv, a, dP, n, s)
    t = table.astype(np.float64)[inv if inv is not None else np.arange(n * s)] @ a.astype(np.float64)
    if n * s > 2:
        assert t.max() > 79.0 and t.min() < -79.0, "the scores must spread over +-80"
    assert np.isfinite(pooled).all() and np.isfinite(alpha).all() and np.isfinite(dV).all() and np.isfinite(slabs).all()
    close(alpha, w_alpha, "alpha")
    close(pooled, w_pooled, "pooled")
    close(dV, w_dV, "dV")
    close(slabs.astype(np.float64).sum(axis=0), w_da, "da")
    np.testing.assert_allclose(alpha.sum(axis=1), 1.0, rtol=1e-5)
    if s == 1:
        assert np.all(alpha == 1.0) and np.all(slabs == 0.0)                  # alpha == 1 exactly, dt == 0
        assert np.array_equal(dV, np.where(table[inv if inv is not None else np.arange(n)] > 0, dP, 0).astype(np.float32))
    again = run_segment(dev, table, inv, a, dP, n, s)
    for x, y in zip((pooled, alpha, dV, slabs), again):
        assert np.array_equal(x, y), "two runs on the same inputs must agree bit for bit"


@pytest.mark.parametrize("n,s,hidden", [(5, 10, 36), (33, 25, 512)])
def test_equal_scores_give_the_mean_and_a_zero_group_gives_zero(dev, n, s, hidden):
    table, inv, a, dP = segment_case(n, s, hidden, False, seed=3, spread=0)
    table[s:2 * s] = 0.0 if n > 1 else table[s:2 * s]                         # group 1: every row zero after the relu
    zero_a = np.zeros(hidden, np.float32)
    pooled, alpha, dV, slabs = run_segment(dev, table, None, zero_a, dP, n, s)
    close(pooled, table.astype(np.float64).reshape(n, s, hidden).mean(axis=1), "pooled == row mean")
    close(alpha, np.full((n, s), 1.0 / s), "alpha == 1 / s")
    # ... and with a real gate (scaled to scores of a few units: a smooth softmax, da well above its rounding) the zero group still
    # has equal scores (all 0), a zero pooled row and no gradient through the relu
    a = (a / np.sqrt(hidden)).astype(np.float32)
    pooled, alpha, dV, slabs = run_segment(dev, table, None, a, dP, n, s)
    w_pooled, w_alpha, w_dV, w_da, _ = oracle_segment(table, None, a, dP, n, s)
    close(pooled, w_pooled, "pooled")
    close(dV, w_dV, "dV")
    close(slabs.astype(np.float64).sum(axis=0), w_da, "da")
    assert np.all(pooled[1] == 0.0) and np.all(dV[s:2 * s] == 0.0) and np.all(alpha[1] == np.float32(1.0) / np.float32(s))


@pytest.mark.parametrize("n_slabs", [1, 2, 7, 40])
def test_gate_gradient_from_several_slab_counts(dev, n_slabs):
    n, s, hidden = 33, 10, 36
    table, inv, a, dP = segment_case(n, s, hidden, True, seed=11, spread=4.0)
    _, _, dV, slabs = run_segment(dev, table, inv, a, dP, n, s, n_slabs=n_slabs)
    _, _, w_dV, w_da, _ = oracle_segment(table, inv, a, dP, n, s)
    assert slabs.shape == (n_slabs, hidden)
    close(slabs.astype(np.float64).sum(axis=0), w_da, "da from %d slabs" % n_slabs)
    close(dV, w_dV, "dV")
    if n_slabs == 40:
        assert np.all(slabs[3:] == 0.0)           # 33 groups, 16 per workgroup: workgroups 3 .. 39 have none and write zeros


def test_shapes_outside_the_range_are_refused(dev):
    z = Mat.zeros(8, 1028, dev)
    v = torch.zeros(2048, device=dev)
    _sync()
    for s, H in ((129, Mat.zeros(129, 8, dev)), (0, Mat.zeros(4, 8, dev)), (2, z), (2, Mat.zeros(4, 6, dev))):
        with pytest.raises(GraphsageAmdError, match="rc=-3"):
            ops.segment_attn_fwd(H, None, v, 1, s, Mat.zeros(1, H.d, dev), v)
        with pytest.raises(GraphsageAmdError, match="rc=-3"):
            ops.segment_attn_bwd(Mat.zeros(1, H.d, dev), H, None, v, v, 1, s, Mat.zeros(max(s, 1), H.d, dev), 1, v.data_ptr())
    with pytest.raises(GraphsageAmdError, match="rc=-3"):
        ops.attn_scores(z, v)
    with pytest.raises(GraphsageAmdError, match="score column"):
        ops.attn_scores(Mat.zeros(4, 8, dev), v)                              # no spare column behind the table's own
    _sync()


# ---------------------------------------------------------------------------------------------------------------
# GS_CSR_SOFTMAX
# ---------------------------------------------------------------------------------------------------------------
N_ROWS = 1300
HUB, HUB_DEG = 6, 1100
_csr = {}


def csr_graph():
    if "g" not in _csr:
        assert SPLIT_LEN == 512
        rng = np.random.RandomState(9)
        degs = rng.randint(0, 9, size=N_ROWS)
        degs[:7] = [0, 1, 2, 511, 512, 513, HUB_DEG]
        lists = [rng.randint(0, N_ROWS, size=d) for d in degs]
        lists[HUB] = 100 + rng.permutation(HUB_DEG)                          # 1,100 distinct rows: three partials (512, 512, 76)
        lists[2][:] = lists[2][0]                                            # duplicate entries
        lists[5][:200] = 77
        lists[10] = np.asarray([3, 3, 3, 9, 9], dtype=np.int64)
        rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        g = FullGraph(rowptr, np.concatenate(lists).astype(np.int32), N_ROWS - 1)
        assert g.splits.shape[0] == 2 and list(g.splits[:, 2]) == [2, 3]     # 513 -> two partials, the hub -> three
        _csr["g"] = (g, lists)
    return _csr["g"]


def csr_table(dev, d):
    """x [N_ROWS, d], logits t [N_ROWS] and the device table: the logit in column d, NaN behind it.  The hub's partials hold
    logits of -80 (first), +80 (second) and about 0 (third): a combine that did not rescale to the common maximum would fail."""
    if ("x", d) not in _csr:
        g, lists = csr_graph()
        rng = np.random.RandomState(d)
        x = rng.randn(N_ROWS, d).astype(np.float32)
        t = (3.0 * rng.randn(N_ROWS)).astype(np.float32)
        hub = lists[HUB]
        t[hub[:512]] = np.float32(-80.0) + t[hub[:512]] / 3
        t[hub[512:1024]] = np.float32(80.0) + t[hub[512:1024]] / 3
        big = torch.full((N_ROWS, d + 8), NAN, dtype=torch.float32, device=dev)
        big[:, :d] = torch.from_numpy(x).to(dev)
        big[:, d] = torch.from_numpy(t).to(dev)
        _sync()
        want = ao.softmax_reduce_rows(lists, x.astype(np.float64), t.astype(np.float64))
        _csr[("x", d)] = (x, t, Mat(big, d), want)
    return _csr[("x", d)]


def out_table(dev, rows, d):
    big = torch.full((rows + 2, d + 8), NAN, dtype=torch.float32, device=dev)
    _sync()
    return Mat(big[:rows], d), big


@pytest.mark.parametrize("d", [4, 36, 512])
def test_csr_softmax_window_and_row_list_forms(dev, d):
    eng.reset_engine()
    e = eng.get_engine()
    g, lists = csr_graph()
    x, t, X, want = csr_table(dev, d)
    assert X.ld == d + 8

    def windows():
        out, big = out_table(dev, N_ROWS, d)
        for r0, n in ((0, 700), (700, N_ROWS - 700)):
            g.reduce(e, CSR_SOFTMAX, X, out.rows_slice(r0, r0 + n), r0, n)
        e.sync()
        assert untouched(big, N_ROWS, d), "a canary around the output was written"
        return out.numpy()

    rows = sorted({0, 1, 2, 3, 4, 5, HUB, 10} | set(range(40, N_ROWS, 7)))
    out_pos = np.full(N_ROWS, -1, np.int32)
    out_pos[rows] = np.random.RandomState(1).permutation(len(rows))
    out_pos_dev = torch.from_numpy(out_pos).to(dev)

    def row_list():
        out, big = out_table(dev, len(rows), d)
        g.reduce_rows(e, CSR_SOFTMAX, X, out, rows, out_pos_dev)
        e.sync()
        assert untouched(big, len(rows), d)
        return out.numpy()[out_pos[rows]]

    got = windows()
    assert np.isfinite(got).all()
    close(got, want, "window form")
    assert len(lists[0]) == 0 and np.all(got[0] == 0.0)                       # an empty row gives 0
    close(got[1], x[lists[1][0]], "degree 1: the neighbor's row")
    close(got[HUB], want[HUB], "the hub")
    close(got[10], (3 * np.exp(t[3] - t[[3, 9]].max()) * x[3] + 2 * np.exp(t[9] - t[[3, 9]].max()) * x[9])
          / (3 * np.exp(t[3] - t[[3, 9]].max()) + 2 * np.exp(t[9] - t[[3, 9]].max())), "duplicates count as often as they occur")
    sub = row_list()
    close(sub, want[rows], "row-list form")
    assert np.array_equal(sub, got[rows]), "a row must come out bit-equal from both forms"
    assert np.array_equal(windows(), got) and np.array_equal(row_list(), sub), "a second run must give the same bits"


def test_csr_softmax_needs_the_logit_column_and_the_wider_workspace(dev):
    eng.reset_engine()
    e = eng.get_engine()
    g, _ = csr_graph()
    X = Mat.zeros(N_ROWS, 12, dev)                                            # ld 12: no column behind the 12 values
    out = Mat.zeros(N_ROWS, 12, dev)
    _sync()
    with pytest.raises(GraphsageAmdError, match="logit"):
        g.reduce(e, CSR_SOFTMAX, X, out, 0, N_ROWS)
    assert ops.csr_reduce_ws_bytes(5, 252 + 4) == 5 * 256 * 4 and ops.csr_reduce_ws_bytes(5, 256 + 4) == 5 * 512 * 4
    rowptr, col, items, splits = g.on(e.device)
    X = Mat(torch.zeros((N_ROWS, 260), device=dev), 256)
    out = Mat.zeros(N_ROWS, 256, dev)
    small = torch.zeros(5 * 256, device=dev)                                  # what the other ops need at d = 256
    _sync()
    with pytest.raises(GraphsageAmdError, match="workspace"):
        ops.csr_reduce_fwd(rowptr, col, items, splits, g.n_rows, g.split_len, CSR_SOFTMAX, X, out, 0, N_ROWS,
                           (0, items.shape[0]), (0, 2), (0, 5), ws=small, stream=e.stream)
    e.sync()


# ---------------------------------------------------------------------------------------------------------------
# model steps against the oracle
# ---------------------------------------------------------------------------------------------------------------
NS, DIM, FEAT, N_NODES, BATCH, WD, LR = [4, 3], 16, 12, 60, 8, 0.01, 0.01


class Vars(object):
    """name (oracle naming) -> engine Variable of an attention model, the Dense and the gate of every aggregator included."""

    def __init__(self, model, supervised):
        self.v = {}
        for i, a in enumerate(model.aggregators):
            assert set(a.vars) == {"self_weights", "neigh_weights"} and all(v.decay for v in a.vars.values())
            assert not a.attn_a.decay and not any(v.decay for v in a.mlp_layers[0].vars.values())
            for k, v in a.vars.items():
                self.v["agg%d/%s" % (i, k)] = v
            self.v["agg%d/mlp_weights" % i] = a.mlp_layers[0].vars['weights']
            self.v["agg%d/mlp_bias" % i] = a.mlp_layers[0].vars['bias']
            self.v["agg%d/attn_a" % i] = a.attn_a
        if supervised:
            self.v["node_pred/weights"] = model.node_pred.vars['weights']
            self.v["node_pred/bias"] = model.node_pred.vars['bias']
        assert all(v in model.engine.variables for v in self.v.values())      # ... all in the flat gradient buffer

    def randomize(self, rng):
        """Non-zero Dense biases (the pad row's hidden state is then not zero) and a gate wide enough to matter."""
        for k, v in self.v.items():
            if k.endswith("mlp_bias"):
                v.assign(0.1 * rng.randn(*v.numpy().shape))
            if k.endswith("attn_a"):
                v.assign(0.5 * rng.randn(*v.numpy().shape))
        eng.get_engine().sync()

    def params(self, dtype=np.float64):
        out = {"agg": []}
        for k, v in self.v.items():
            head, name = k.split("/")
            a = v.numpy().astype(dtype)
            a = a.reshape(-1) if (name.endswith("bias") or name == "attn_a") else a
            if head == "node_pred":
                out.setdefault("node_pred", {})[name] = a
            else:
                while len(out["agg"]) <= int(head[3:]):
                    out["agg"].append({})
                out["agg"][int(head[3:])][name] = a
        return out

    @staticmethod
    def pick(tree, k):
        head, name = k.split("/")
        return tree["node_pred"][name] if head == "node_pred" else tree["agg"][int(head[3:])][name]


class Adam(object):
    """The oracle's clip + TF Adam per variable, and the knee bookkeeping of the module docstring."""

    def __init__(self):
        self.m, self.v, self.solid, self.t = {}, {}, {}, 0

    def step(self, named_params, named_grads):
        self.t += 1
        out = {}
        for k, p in named_params.items():
            g = np.asarray(named_grads[k], np.float64).reshape(p.shape)
            if k not in self.m:
                self.m[k], self.v[k], self.solid[k] = np.zeros_like(p), np.zeros_like(p), np.ones(p.shape, bool)
            self.solid[k] &= np.abs(g) > max(1e-6 * max(1e-2, np.abs(g).max()), ADAM_KNEE)
            q = p.copy()
            orc.adam_tf_update(q, orc.clip_by_value(g), self.m[k], self.v[k], self.t, LR)
            out[k] = q
        return out

    def check(self, k, got, want):
        s = self.solid[k]
        assert s.any() or k.endswith("attn_a") or k.endswith("bias"), k
        np.testing.assert_allclose(got.reshape(want.shape)[s], want[s], rtol=RTOL, atol=2e-5, err_msg="after/" + k)


def graph_and_iterator(kind):
    from graphsage_amd.minibatch import EdgeMinibatchIterator, NodeMinibatchIterator
    from graphsage_amd.models import Placeholder
    from graphsage_amd.utils import synthetic_graph
    eng.reset_engine()
    inits.set_seed(7)
    np.random.seed(7)
    G = synthetic_graph(n_nodes=N_NODES, feat_dim=FEAT, num_classes=5, avg_degree=5, seed=5, multilabel=False)
    if kind == "sup":
        ph = {'labels': Placeholder('labels'), 'batch': Placeholder('batch1'), 'dropout': Placeholder('dropout', 0.),
              'batch_size': Placeholder('batch_size')}
        it = NodeMinibatchIterator(G, None, ph, None, G.num_classes, batch_size=BATCH, max_degree=6)
    else:
        ph = {'batch1': Placeholder('batch1'), 'batch2': Placeholder('batch2'), 'neg_samples': Placeholder('neg'),
              'dropout': Placeholder('dropout', 0.), 'batch_size': Placeholder('batch_size')}
        it = EdgeMinibatchIterator(G, None, ph, context_pairs=None, batch_size=BATCH, max_degree=6)
    return G, ph, it


def build_supervised(concat=True, identity_dim=0, model_size="small"):
    from graphsage_amd.models import SAGEInfo
    from graphsage_amd.neigh_samplers import AdjInfo, PaddedAdjacency, UniformNeighborSampler
    from graphsage_amd.supervised_models import SupervisedGraphsage
    G, ph, it = graph_and_iterator("sup")
    e = eng.get_engine()
    sampler = UniformNeighborSampler(AdjInfo(PaddedAdjacency(it.adj, e.device)))
    model = SupervisedGraphsage(G.num_classes, ph, G.padded_features(), sampler.adj_info, it.deg,
                                [SAGEInfo("node", sampler, n, DIM) for n in NS], concat=concat, aggregator_type="attn",
                                model_size=model_size, sigmoid_loss=False, learning_rate=LR, weight_decay=WD,
                                identity_dim=identity_dim)
    model.use_graphs = False
    return G, it, ph, sampler, model


def build_unsupervised(concat=True, n_neg=5):
    from graphsage_amd.models import SAGEInfo, SampleAndAggregate
    from graphsage_amd.neigh_samplers import AdjInfo, PaddedAdjacency, UniformNeighborSampler
    G, ph, it = graph_and_iterator("unsup")
    e = eng.get_engine()
    sampler = UniformNeighborSampler(AdjInfo(PaddedAdjacency(it.adj, e.device)))
    dim = 32 if concat else 64          # the link-prediction loss kernel takes embeddings of 64 / 128 / 256 / 512 columns, not 2 * 16
    model = SampleAndAggregate(ph, G.padded_features(), sampler.adj_info, it.deg, [SAGEInfo("node", sampler, n, dim) for n in NS],
                               concat=concat, aggregator_type="attn", learning_rate=LR, weight_decay=WD, neg_sample_size=n_neg)
    model.use_graphs = False
    return G, it, ph, sampler, model


SUP_CASES = {
    "concat": dict(),
    "add": dict(concat=False),
    "distinct_ids": dict(dedup_min_rows=0),
    "no_dedup": dict(dedup_pool=False, dedup_min_rows=0),
    "dropout": dict(dropout=0.5),
    "identity": dict(identity_dim=4),
    "identity_distinct_ids": dict(identity_dim=4, dedup_min_rows=0),
    "big": dict(model_size="big"),
}


@pytest.mark.parametrize("case", sorted(SUP_CASES))
def test_supervised_steps_match_oracle(dev, case):
    from test_model_gpu import _device_masks
    c = dict(dict(concat=True, identity_dim=0, model_size="small", dedup_min_rows=None, dedup_pool=True, dropout=0.0), **SUP_CASES[case])
    G, it, ph, sampler, model = build_supervised(c["concat"], c["identity_dim"], c["model_size"])
    for a in model.aggregators:
        assert a.hidden_dim == (1024 if c["model_size"] == "big" else 512) and a.attn_a.numpy().shape == (1, a.hidden_dim)
        a.dedup_min_rows, a.dedup_pool = c["dedup_min_rows"], c["dedup_pool"]
    vs = Vars(model, supervised=True)
    rng = np.random.RandomState(3)
    vs.randomize(rng)
    adam, adam_emb = Adam(), Adam()
    idim, rate = c["identity_dim"], c["dropout"]
    for step in range(3):
        batch = rng.choice(it.train_nodes, size=BATCH - (step == 1), replace=False).astype(np.int32)      # one ragged batch
        labels = it.label_matrix[batch]
        perms = [rng.permutation(it.max_degree) for _ in NS]
        sampler.inject_perms(perms)
        params = vs.params()
        feats = G.padded_features().astype(np.float64)
        if idim:
            emb0 = model.embeds.numpy().astype(np.float64)
            feats = np.concatenate([emb0, feats], axis=1)
        clock = int(model.engine.sample_clock_dev.item())
        feed = {ph['batch']: batch, ph['labels']: labels, ph['batch_size']: len(batch)}
        if rate:
            feed[ph['dropout']] = rate
        loss, preds = model.train_step(feed)
        a0 = model.aggregators[0]
        if c["dedup_min_rows"] == 0 and c["dedup_pool"]:
            cnt, rows_total = a0.last_unique
            assert 0 < int(cnt.item()) <= rows_total and a0.last_pool_kernel in ("split16", "split_bf16x3", "fp32_mfma")
            if idim:
                assert a0.last_pool_kernel == "split_bf16x3"                  # a table with trainable columns is never cut once
            assert model.aggregators[1].last_unique is None                   # layer 1 reads hidden rows, not table ids
        else:
            assert a0.last_unique is None and a0.last_pool_kernel is None
        samples, support = orc.sample(it.adj, batch, NS, perms)
        for got, want in zip(model.samples1, samples):
            assert np.array_equal(got.cpu().numpy(), want)
        masks = head_mask = None
        if rate:
            masks, hm = _device_masks(model, "meanpool", rate, clock, NS, len(batch))      # the pooling aggregators' mask sites
            head_mask = hm(len(batch), model.agg_out.d)
        with ao.installed():
            res = orc.supervised_fwd_bwd(params, feats, samples, support, labels.astype(np.float64), model.dims, NS, len(batch),
                                         "attn", c["concat"], False, weight_decay=WD, identity_dim=idim, masks=masks,
                                         head_mask=head_mask)
        close(loss, res["loss"], "loss step %d" % step)
        close(preds, res["preds"], "preds step %d" % step)
        close(model.outputs1.numpy(), res["outputs1"], "outputs1 step %d" % step)
        grads = {k: Vars.pick(res["grads"], k) for k in vs.v}
        for k, v in vs.v.items():
            close(v.grad.numpy(), grads[k], "step %d grad/%s" % (step, k))
        assert np.abs(grads["agg0/attn_a"]).max() > 0 and np.abs(grads["agg1/attn_a"]).max() > 0
        after = adam.step({k: Vars.pick(params, k) for k in vs.v}, grads)
        for k, v in vs.v.items():
            adam.check(k, v.numpy().astype(np.float64), after[k])
        if idim:
            w = res["grads"]["embeds"]
            assert np.count_nonzero(w) > 0
            close(model.embeds.grad.numpy(), w, "step %d grad/node_embeddings" % step)
            want = adam_emb.step({"e": emb0}, {"e": w})["e"]
            adam_emb.check("e", model.embeds.numpy().astype(np.float64), want)


@pytest.mark.parametrize("concat", [True, False])
def test_unsupervised_steps_match_oracle(dev, concat):
    from test_unsup_gpu import sample_three_calls
    n_neg = 5
    G, it, ph, sampler, model = build_unsupervised(concat, n_neg)
    vs = Vars(model, supervised=False)
    rng = np.random.RandomState(5)
    vs.randomize(rng)
    adam = Adam()
    feats = G.padded_features().astype(np.float64)
    for step in range(3):
        edges = it.train_edges[step * BATCH:(step + 1) * BATCH - (step == 1)]
        B = len(edges)
        perms = [rng.permutation(it.max_degree) for _ in range(3 * len(NS))]
        sampler.inject_perms(perms)
        params = vs.params()
        loss, ranks, aff_all, mrr, outputs1 = model.train_step({ph['batch1']: edges[:, 0], ph['batch2']: edges[:, 1],
                                                                ph['batch_size']: B})
        roots = model.samples1[0].cpu().numpy()
        assert np.array_equal(roots[:2 * B], np.concatenate([edges[:, 0], edges[:, 1]]))
        neg = roots[2 * B:]
        assert neg.shape == (n_neg,)
        samples, support = sample_three_calls(it.adj, edges[:, 0], edges[:, 1], neg, NS, perms)
        for got, want in zip(model.samples1, samples):
            assert np.array_equal(got.cpu().numpy(), want)
        with ao.installed():
            res = orc.unsupervised_fwd_bwd(params["agg"], feats, samples, support, model.dims, NS, B, n_neg, "attn", concat,
                                           weight_decay=WD)
        close(loss, res["loss"], "loss step %d" % step)
        close(outputs1, res["outputs1"], "outputs1 step %d" % step)
        close(aff_all, res["aff_all"], "aff_all step %d" % step)
        grads = {k: Vars.pick({"agg": res["grads"]}, k) for k in vs.v}
        for k, v in vs.v.items():
            close(v.grad.numpy(), grads[k], "step %d grad/%s" % (step, k))
        after = adam.step({k: Vars.pick(params, k) for k in vs.v}, grads)
        for k, v in vs.v.items():
            adam.check(k, v.numpy().astype(np.float64), after[k])


@pytest.mark.parametrize("dedup_min_rows", [None, 0])
def test_a_step_repeated_from_the_same_state_gives_the_same_bits(dev, dedup_min_rows):
    outs = []
    for _ in range(2):
        G, it, ph, sampler, model = build_supervised()
        model.aggregators[0].dedup_min_rows = dedup_min_rows
        e = eng.get_engine()
        rng = np.random.RandomState(2)
        Vars(model, True).randomize(rng)
        for step in range(2):
            batch = rng.choice(it.train_nodes, size=BATCH, replace=False).astype(np.int32)
            sampler.inject_perms([rng.permutation(it.max_degree) for _ in NS])
            loss, preds = model.train_step({ph['batch']: batch, ph['labels']: it.label_matrix[batch], ph['batch_size']: BATCH})
        e.sync()
        outs.append((loss, preds.tobytes(), e.params.cpu().numpy().tobytes(), e.grads.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


def test_a_fan_out_beyond_the_range_is_refused_at_the_first_step(dev):
    from graphsage_amd.models import SAGEInfo
    from graphsage_amd.neigh_samplers import AdjInfo, PaddedAdjacency, UniformNeighborSampler
    from graphsage_amd.supervised_models import SupervisedGraphsage
    from graphsage_amd.minibatch import NodeMinibatchIterator
    from graphsage_amd.models import Placeholder
    from graphsage_amd.utils import synthetic_graph
    eng.reset_engine()
    inits.set_seed(7)
    G = synthetic_graph(n_nodes=N_NODES, feat_dim=FEAT, num_classes=5, avg_degree=5, seed=5, multilabel=False)
    ph = {'labels': Placeholder('labels'), 'batch': Placeholder('batch1'), 'dropout': Placeholder('dropout', 0.),
          'batch_size': Placeholder('batch_size')}
    it = NodeMinibatchIterator(G, None, ph, None, G.num_classes, batch_size=2, max_degree=130)
    sampler = UniformNeighborSampler(AdjInfo(PaddedAdjacency(it.adj, eng.get_engine().device)))
    model = SupervisedGraphsage(G.num_classes, ph, G.padded_features(), sampler.adj_info, it.deg,
                                [SAGEInfo("node", sampler, 2, DIM), SAGEInfo("node", sampler, 129, DIM)], concat=True,
                                aggregator_type="attn", sigmoid_loss=False, learning_rate=LR)
    model.use_graphs = False
    batch = it.train_nodes[:2].astype(np.int32)
    with pytest.raises(GraphsageAmdError, match="1 <= samples <= 128"):
        model.train_step({ph['batch']: batch, ph['labels']: it.label_matrix[batch], ph['batch_size']: 2})


# ---------------------------------------------------------------------------------------------------------------
# exact inference
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("concat", [True, False])
def test_full_and_subset_inference_match_the_whole_list_oracle(dev, concat):
    G, it, ph, sampler, model = build_supervised(concat)
    vs = Vars(model, True)
    vs.randomize(np.random.RandomState(4))
    params = vs.params()
    feats = G.padded_features().astype(np.float64)
    N = G.n_nodes
    for graph, lists in ((FullGraph.from_padded(it.adj), fo.padded_lists(it.adj)),          # duplicates: the padded rows repeat ids
                         (FullGraph.from_csr(it.train_csr[0], it.train_csr[1], N), fo.csr_lists(it.train_csr[0], it.train_csr[1], N))):
        want = ao.full_forward(lists, feats, params, concat)
        emb = model.embed_full(graph)
        close(emb, want[:N], "embed_full")
        emb2, preds = model.predict_full(graph)
        assert np.array_equal(emb2, emb)
        close(preds, fo.predict(want[:N], params, False)[1], "predict_full")
        nodes = [7, 3, 7, N - 1, 20]
        sub, stats = model.embed_nodes(graph, nodes)                          # RowsLayer: the row-list reduce, compact tables
        close(sub, emb[nodes], "embed_nodes == embed_full")
        close(sub, want[nodes], "embed_nodes == oracle")
        assert stats["rows"][0] == 4 and stats["n_rows"] == N + 1
        again, _ = model.embed_nodes(graph, nodes)
        assert np.array_equal(sub, again) and np.array_equal(model.embed_full(graph), emb)
        pad, _ = model.embed_nodes(graph, [N])                                # the pad row is a row like any other
        close(pad, want[[N]], "the pad row")


def test_rank_full_and_topk_full_run_on_the_new_model(dev):
    G, it, ph, sampler, model = build_unsupervised()
    Vars(model, False).randomize(np.random.RandomState(6))
    N = G.n_nodes
    graph = FullGraph.from_csr(it.train_csr[0], it.train_csr[1], N)
    top = model.topk_full(graph, nodes=np.arange(10), k=3)
    assert top["ids"].shape == (10, 3) and np.all(top["count"] == 3) and np.all((top["ids"] >= 0) & (top["ids"] < N))
    assert np.all(np.diff(top["scores"], axis=1) <= 0)
    edges = np.stack([np.arange(10), top["ids"][:, 0]], axis=1)
    res = model.rank_full(graph, edges)
    assert np.array_equal(res["scores"], top["scores"][:, 0]), "the scores of a pair: the same bits from both sweeps"
    assert np.all(res["ranks_optimistic"] == 1) and np.all(res["ranks"] >= 1)                # the best candidate ranks first
    assert np.array_equal(model.topk_full(graph, nodes=np.arange(10), k=3)["ids"], top["ids"])


# ---------------------------------------------------------------------------------------------------------------
# drivers: fresh child processes
# ---------------------------------------------------------------------------------------------------------------
COMMON = ["--synthetic", "small", "--epochs", "1", "--batch_size", "128", "--samples_1", "5", "--samples_2", "3", "--dim_1", "32",
          "--dim_2", "32", "--max_total_steps", "6", "--model", "graphsage_attn"]
EMBED_LINE = r"Receptive-field inference: nodes= 4 rows= 3 / \d+ / \d+ of \d+ edges= \d+ time= \d+\.\d{5}"


def child(module, args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "graphsage_amd." + module] + args, cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=400)


def test_supervised_train_driver(dev, tmp_path):
    ids = tmp_path / "ids.txt"
    ids.write_text("12\n3\n12\n250")
    r = child("supervised_train", COMMON + ["--validate_iter", "10", "--print_every", "2", "--base_log_dir", str(tmp_path / "log"),
                                            "--full_inference", "--embed_nodes", str(ids)])
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    assert "Optimization Finished!" in out and "Full validation stats:" in out
    losses = [float(x) for x in re.findall(r"train_loss= (\S+)", out)]
    assert losses and np.isfinite(losses).all()
    assert re.search(r"Full-neighborhood validation stats: f1_micro= \d\.\d{5}", out) and re.search(EMBED_LINE, out)
    files = files_under(tmp_path / "log")
    assert {"val_stats.txt", "test_stats.txt", "val_stats_full.txt", "embed_nodes.npy", "embed_nodes_preds.npy"} <= set(files)
    assert "graphsage_attn_small" in files["val_stats.txt"]
    emb = np.load(files["embed_nodes.npy"])
    assert emb.shape == (4, 64) and np.isfinite(emb).all() and np.array_equal(emb[0], emb[2])
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1.0, rtol=1e-5)


def test_unsupervised_train_driver(dev, tmp_path):
    ids = tmp_path / "ids.txt"
    ids.write_text("12\n3\n12\n250")
    r = child("unsupervised_train", COMMON + ["--learning_rate", "0.001", "--max_walk_pairs", "4000", "--validate_iter", "10",
                                              "--print_every", "2", "--validate_batch_size", "256", "--base_log_dir",
                                              str(tmp_path / "log"), "--full_inference", "--embed_nodes", str(ids)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Optimization Finished!" in r.stdout and re.search(EMBED_LINE, r.stdout)
    losses = [float(x) for x in re.findall(r"train_loss= (\S+)", r.stdout)]
    assert losses and np.isfinite(losses).all()
    files = files_under(tmp_path / "log")
    assert {"val.npy", "val.txt", "val_full.npy", "val_full.txt", "embed_nodes.npy"} <= set(files)
    assert "graphsage_attn_small" in files["val.npy"]
    full = np.load(files["val_full.npy"])
    assert full.shape[1] == 64 and np.isfinite(full).all() and np.isfinite(np.load(files["val.npy"])).all()
    np.testing.assert_allclose(np.linalg.norm(full, axis=1), 1.0, rtol=1e-5)
    row_of = {tok: i for i, tok in enumerate(open(files["val_full.txt"]).read().split("\n"))}
    close(np.load(files["embed_nodes.npy"]), full[[row_of[t] for t in ("12", "3", "12", "250")]], "embed_nodes rows == val_full rows")


@pytest.mark.parametrize("module", ["supervised_train", "unsupervised_train"])
def test_a_samples_flag_beyond_the_range_is_refused_before_the_first_step(dev, tmp_path, module):
    args = [a for a in COMMON]
    args[args.index("--samples_1") + 1] = "129"
    r = child(module, args + ["--base_log_dir", str(tmp_path)])
    assert r.returncode != 0
    assert "GraphsageAmdError" in r.stderr and "1 <= samples <= 128" in r.stderr
    assert "Epoch:" not in r.stdout and "Loading training data" not in r.stdout
    assert not files_under(tmp_path)
