"""-m gpu: the node2vec baseline on the device (csrc/gs_n2v.hip, models.Node2VecModel, the n2v branch of the driver).

  kernels alone == the NumPy restatement (tests/n2v_oracle.py) over the supported widths, batch sizes and negative counts,
      with planted duplicates, an all-same-pair batch and rows beyond byte offset 2^32 of a table;
  device distinct-negatives sampler == its host restatement, bit for bit;
  every step of tests/golden/ref_n2v_*.npz (the reference's own Node2VecModel run) on identical pairs and negatives;
  captured multi-step graphs == single launches and run-to-run reproducibility, bit for bit;
  the unsupervised_train driver with --model n2v end to end.
Floats are compared with RTOL and close() of tests/test_ref_pin_gpu.py; ids bit-exact.
"""
import os
import re

import numpy as np
import pytest
import torch

import n2v_oracle
from n2v_oracle import N2V, Fixture
from oracle import sampler_hash
from test_ref_pin_gpu import RTOL, close

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------
# the three launches, bare
# ---------------------------------------------------------------------------------------------------------------
class Bare(object):
    """target / context / bias on the device and one step's buffers, driven through ops.call."""

    def __init__(self, dev, target, context, bias, B, n_neg):
        from graphsage_amd import ops
        self.ops, self.dev = ops, dev
        self.t = target if isinstance(target, torch.Tensor) else torch.from_numpy(target).to(dev)
        self.c = context if isinstance(context, torch.Tensor) else torch.from_numpy(context).to(dev)
        self.b = bias if isinstance(bias, torch.Tensor) else torch.from_numpy(bias).to(dev)
        self.rows, self.d = self.t.shape
        self.B, self.n_neg = B, n_neg
        self.n_slabs = int(ops._lib.load().gs_n2v_slabs(B, self.d, n_neg))
        assert self.n_slabs > 0
        f = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
        self.ids = torch.zeros(2 * B + n_neg, dtype=torch.int32, device=dev)
        self.loss_rows, self.rr_rows, self.aff_all, self.outputs1 = f(B), f(B), f(B, n_neg + 1), f(B, self.d)
        self.g_target, self.g_ctx, self.g_bias = f(B, self.d), f(B, self.d), f(B)
        self.neg_slabs, self.bias_slabs = f(self.n_slabs, n_neg, self.d), f(self.n_slabs, n_neg)
        self.loss, self.mrr = f(1), f(1)
        torch.cuda.synchronize()

    def step(self, b1, b2, neg, lr, train=True):
        ops, P = self.ops, self.ops.ptr
        ids = np.concatenate([b1, b2, neg]).astype(np.int32)
        assert ids.min() >= 0 and ids.max() < self.rows
        self.ids.copy_(torch.from_numpy(ids))
        torch.cuda.synchronize()
        d, B, n_neg = self.d, self.B, self.n_neg
        grads = [self.g_target, self.g_ctx, self.g_bias, self.neg_slabs, self.bias_slabs] if train else [None] * 5
        ops.call("gs_n2v_fwd_bwd", P(self.t), d, P(self.c), d, P(self.b), self.rows, P(self.ids), B, d, n_neg, 1 if train else 0,
                 P(self.loss_rows), P(self.rr_rows), P(self.aff_all), n_neg + 1, P(self.outputs1), d,
                 *([P(g) for g in grads] + [None]))
        if train:
            ops.call("gs_n2v_apply", P(self.t), d, P(self.c), d, P(self.b), self.rows, P(self.ids), B, d, n_neg, lr,
                     P(self.g_target), P(self.g_ctx), P(self.g_bias), P(self.neg_slabs), P(self.bias_slabs), self.n_slabs,
                     P(self.loss_rows), P(self.rr_rows), P(self.loss), P(self.mrr), None, 0, None, 0, None)
        torch.cuda.synchronize()


def check_against_oracle(bare, t0, c0, b0, b1, b2, neg, lr):
    """t0 / c0 / b0: float32 NumPy tables before the step (only rows the step touches need to be real)."""
    want = n2v_oracle.step(t0.astype(np.float64), c0.astype(np.float64), b0.astype(np.float64), b1, b2, neg, lr=lr)
    B = len(b1)
    close(bare.loss_rows.cpu().numpy().sum() / B, want["loss"], "loss")
    close(bare.loss.item(), want["loss"], "loss (epilogue)")
    close(bare.aff_all.cpu().numpy(), want["aff_all"], "aff_all")
    assert np.array_equal(bare.outputs1.cpu().numpy(), t0[b1]), "outputs1 is a gather: bit-exact"
    aff = want["aff_all"]
    margin = np.abs(aff[:, :-1] - aff[:, -1:]).min(axis=1) > 1e-4
    rr = bare.rr_rows.cpu().numpy()
    assert np.array_equal(rr[margin], (np.float32(1.0) / (want["rank_true"] + 1).astype(np.float32))[margin])
    if margin.all():
        close(bare.mrr.item(), want["mrr"], "mrr")
    close(bare.g_target.cpu().numpy(), want["g_target"], "g_target")
    close(bare.g_ctx.cpu().numpy(), want["g_ctx"], "g_ctx")
    close(bare.g_bias.cpu().numpy(), want["g_bias"], "g_bias")
    close(bare.neg_slabs.cpu().numpy().sum(axis=0), want["g_neg"], "sum of the negatives' slabs")
    close(bare.bias_slabs.cpu().numpy().sum(axis=0), want["gb_neg"], "sum of the bias slabs")
    return want


def planted_batch(rng, n_rows, B, n_neg, pool):
    """Pairs from a small pool (repeats on both sides), distinct negatives of which some are batch2 nodes."""
    ids = rng.choice(n_rows - 1, size=min(pool, n_rows - 1), replace=False)
    b1 = rng.choice(ids, size=B)
    b2 = rng.choice(ids, size=B)
    if B >= 3:
        b1[-1] = b1[0]
        b2[-2] = b2[0]
    others = np.setdiff1d(np.arange(n_rows - 1), ids)
    k = min(n_neg, max(1, n_neg // 2), len(np.unique(b2)))
    neg = np.concatenate([rng.choice(np.unique(b2), size=k, replace=False), rng.choice(others, size=n_neg - k, replace=False)])
    return b1.astype(np.int32), b2.astype(np.int32), rng.permutation(neg).astype(np.int32)


@pytest.mark.parametrize("n_neg", [1, 20])
@pytest.mark.parametrize("B", [1, 37, 512])
@pytest.mark.parametrize("d", [64, 128, 256, 512])
def test_kernels_equal_numpy(dev, d, B, n_neg):
    rng = np.random.RandomState(1000 * d + 10 * B + n_neg)
    n_rows = 400
    t0 = rng.uniform(-1, 1, (n_rows, d)).astype(np.float32)
    c0 = (rng.standard_normal((n_rows, d)) / np.sqrt(d)).astype(np.float32) * 3
    b0 = rng.uniform(-0.5, 0.5, n_rows).astype(np.float32)
    b1, b2, neg = planted_batch(rng, n_rows, B, n_neg, pool=40)
    lr = 0.3
    bare = Bare(dev, t0.copy(), c0.copy(), b0.copy(), B, n_neg)
    bare.step(b1, b2, neg, lr)
    want = check_against_oracle(bare, t0, c0, b0, b1, b2, neg, lr)
    t1, c1, bb1 = bare.t.cpu().numpy(), bare.c.cpu().numpy(), bare.b.cpu().numpy()
    rt, rc = want["rows_target"], want["rows_context"]
    close(t1[rt], want["target"][rt], "target rows")
    close(c1[rc], want["context"][rc], "context rows")
    close(bb1[rc], want["bias"][rc], "bias")
    assert np.abs(t1[rt] - t0[rt]).max() > 100 * RTOL * lr / B, "the step must move rows far above the tolerance"
    rest_t, rest_c = np.setdiff1d(np.arange(n_rows), rt), np.setdiff1d(np.arange(n_rows), rc)
    assert np.array_equal(t1[rest_t], t0[rest_t]) and np.array_equal(c1[rest_c], c0[rest_c]) and np.array_equal(bb1[rest_c], b0[rest_c])
    # the evaluation form: same loss / affinities, nothing written to the tables or the gradient buffers
    ev = Bare(dev, t0.copy(), c0.copy(), b0.copy(), B, n_neg)
    ev.step(b1, b2, neg, lr, train=False)
    assert np.array_equal(ev.loss_rows.cpu().numpy(), bare.loss_rows.cpu().numpy())
    assert np.array_equal(ev.aff_all.cpu().numpy(), bare.aff_all.cpu().numpy())
    assert np.array_equal(ev.t.cpu().numpy(), t0) and np.array_equal(ev.c.cpu().numpy(), c0)
    assert torch.isnan(ev.g_target).all() and torch.isnan(ev.neg_slabs).all()


@pytest.mark.parametrize("d,B,n_neg", [(64, 512, 20), (256, 37, 5), (512, 512, 20)])
def test_every_pair_the_same_pair(dev, d, B, n_neg):
    """One target row and one context row take the sum of B gradient rows; the context row is a negative as well."""
    rng = np.random.RandomState(d + B)
    n_rows = 64
    t0 = rng.uniform(-1, 1, (n_rows, d)).astype(np.float32)
    c0 = (rng.standard_normal((n_rows, d)) / np.sqrt(d)).astype(np.float32)
    b0 = rng.uniform(-0.5, 0.5, n_rows).astype(np.float32)
    b1, b2 = np.full(B, 7, np.int32), np.full(B, 9, np.int32)
    neg = np.concatenate([[9], rng.choice(np.setdiff1d(np.arange(n_rows), [9]), n_neg - 1, replace=False)]).astype(np.int32)
    bare = Bare(dev, t0.copy(), c0.copy(), b0.copy(), B, n_neg)
    bare.step(b1, b2, neg, 0.25)
    want = check_against_oracle(bare, t0, c0, b0, b1, b2, neg, 0.25)
    close(bare.t.cpu().numpy(), want["target"], "target")
    close(bare.c.cpu().numpy(), want["context"], "context")
    close(bare.b.cpu().numpy(), want["bias"], "bias")


def test_rows_beyond_byte_offset_2_to_32(dev):
    d, B, n_neg = 512, 37, 20
    n_rows = (1 << 32) // (4 * d) + 4096                     # the last 4096 rows start beyond byte 2^32
    need = 4 * n_rows * d * 4 + (2 << 30)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %.1f GiB of free device memory, the card has %.1f" % (need / 2.0 ** 30, free / 2.0 ** 30))
    rng = np.random.RandomState(5)
    far = np.arange(n_rows - 4096, n_rows - 1)
    assert far.min() * d * 4 >= 1 << 32
    ids = np.concatenate([rng.choice(far, 30, replace=False), [3, 100]])
    b1, b2 = rng.choice(ids, B).astype(np.int32), rng.choice(ids, B).astype(np.int32)
    neg = np.concatenate([[b2[0]], rng.choice(np.setdiff1d(far, ids), n_neg - 1, replace=False)]).astype(np.int32)
    used = np.unique(np.concatenate([b1, b2, neg]))
    t = torch.zeros((n_rows, d), dtype=torch.float32, device=dev)
    c = torch.zeros((n_rows, d), dtype=torch.float32, device=dev)
    b = torch.zeros(n_rows, dtype=torch.float32, device=dev)
    tu = rng.uniform(-1, 1, (len(used), d)).astype(np.float32)
    cu = (rng.standard_normal((len(used), d)) / np.sqrt(d)).astype(np.float32)
    ui = torch.from_numpy(used).to(dev).long()
    t[ui] = torch.from_numpy(tu).to(dev)
    c[ui] = torch.from_numpy(cu).to(dev)
    t_before, c_before = t.clone(), c.clone()
    bare = Bare(dev, t, c, b, B, n_neg)
    bare.step(b1, b2, neg, 0.5)
    # the oracle on the used rows only, ids renumbered
    renum = {int(v): k for k, v in enumerate(used)}
    m = lambda a: np.asarray([renum[int(v)] for v in a])
    want = check_against_oracle_small(bare, tu, cu, np.zeros(len(used), np.float32), m(b1), m(b2), m(neg), 0.5)
    close(t[ui].cpu().numpy(), want["target"], "target rows")
    close(c[ui].cpu().numpy(), want["context"], "context rows")
    close(b[ui].cpu().numpy(), want["bias"], "bias")
    changed_t = torch.nonzero((t != t_before).any(dim=1)).flatten().cpu().numpy()
    changed_c = torch.nonzero((c != c_before).any(dim=1)).flatten().cpu().numpy()
    assert np.array_equal(changed_t, np.unique(b1)) and np.array_equal(changed_c, np.unique(np.concatenate([b2, neg])))
    assert int(torch.count_nonzero(b)) <= len(used)


def check_against_oracle_small(bare, tu, cu, bu, b1, b2, neg, lr):
    want = n2v_oracle.step(tu.astype(np.float64), cu.astype(np.float64), bu.astype(np.float64), b1, b2, neg, lr=lr)
    close(bare.loss.item(), want["loss"], "loss")
    close(bare.aff_all.cpu().numpy(), want["aff_all"], "aff_all")
    assert np.array_equal(bare.outputs1.cpu().numpy(), tu[b1])
    return want


# ---------------------------------------------------------------------------------------------------------------
# staging
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_neg,seed,clock,slot_offset", [(1, 123, 0, 0), (6, 123, 1, 0), (20, 7, 5, 1024), (200, 99, 2 ** 33, 3)])
def test_device_unique_sampler_equals_host_restatement(dev, n_neg, seed, clock, slot_offset):
    from graphsage_amd import ops
    rng = np.random.RandomState(n_neg)
    deg = rng.randint(0, 30, size=700)
    deg[rng.choice(700, 300, replace=False)] = 0
    deg[:3] = 400                                                      # hubs: the stream repeats them often
    deg[-1] = 0
    cdf = sampler_hash.unigram_cdf_u32(deg)
    want = n2v_oracle.sample_unigram_unique(cdf, n_neg, seed, clock, slot_offset)
    B = 300
    pairs = rng.randint(0, 700, size=(1000, 2)).astype(np.int32)
    cursor = 850                                                       # wraps round the end of the list
    cdf_d = torch.from_numpy(cdf.view(np.int32).copy()).to(dev)
    pairs_d = torch.from_numpy(pairs).to(dev)
    cur_d = torch.tensor([cursor], dtype=torch.int64, device=dev)
    clk_d = torch.tensor([clock], dtype=torch.int64, device=dev)
    ids = torch.full((2 * B + n_neg,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    bits = 7                                                           # buckets that hold several nodes, and empty ones
    thr = np.arange((1 << bits) + 1, dtype=np.uint64) << np.uint64(32 - bits)
    guide = np.minimum(np.searchsorted(cdf.astype(np.uint64), thr, side="right"), len(cdf) - 1).astype(np.int32)
    guide_d = torch.from_numpy(guide).to(dev)
    torch.cuda.synchronize()
    for g, gb in ((None, 0), (guide_d, bits)):                         # the plain search and the guided one: same draws
        ids.fill_(-1)
        torch.cuda.synchronize()
        ops.call("gs_n2v_stage", ops.ptr(pairs_d), len(pairs), ops.ptr(cur_d), B, ops.ptr(cdf_d), len(cdf), n_neg, seed,
                 ops.ptr(clk_d), slot_offset, ops.ptr(g), gb, ops.ptr(ids), ops.ptr(status), None)
        torch.cuda.synchronize()
        got = ids.cpu().numpy()
        e = (cursor + np.arange(B)) % len(pairs)
        assert np.array_equal(got[:B], pairs[e, 0]) and np.array_equal(got[B:2 * B], pairs[e, 1])
        assert np.array_equal(got[2 * B:], want) and int(status.item()) == 0
        assert len(np.unique(got[2 * B:])) == n_neg and (deg[got[2 * B:]] > 0).all()


def test_too_few_weighted_nodes_are_refused_on_the_host(dev):
    from graphsage_amd import engine as eng
    from graphsage_amd.models import Node2VecModel, Placeholder
    eng.reset_engine()
    deg = np.zeros(100, np.int64)
    deg[:5] = 3
    ph = {k: Placeholder(k) for k in ("batch1", "batch2", "batch_size", "dropout")}
    with pytest.raises(ValueError, match="non-zero"):
        Node2VecModel(ph, 101, deg, nodevec_dim=64, lr=0.1, neg_sample_size=6)
    with pytest.raises(Exception, match="64 / 128 / 256 / 512"):
        Node2VecModel(ph, 101, deg, nodevec_dim=50, lr=0.1, neg_sample_size=4)
    with pytest.raises(NotImplementedError):
        Node2VecModel(ph, 101, deg, nodevec_dim=64, lr=0.1, neg_sample_size=4, world_size=2)
    Node2VecModel(ph, 101, deg, nodevec_dim=64, lr=0.1, neg_sample_size=5)


# ---------------------------------------------------------------------------------------------------------------
# the reference's own run
# ---------------------------------------------------------------------------------------------------------------
def build_model(fx):
    from graphsage_amd import engine as eng
    from graphsage_amd.models import Node2VecModel, Placeholder
    eng.reset_engine()
    ph = {k: Placeholder(k) for k in ("batch1", "batch2", "batch_size", "dropout")}
    n = len(fx["graph/deg"])
    model = Node2VecModel(ph, n + 1, fx["graph/deg"], nodevec_dim=fx.d, lr=fx.lr, neg_sample_size=fx.n_neg)
    return ph, model


@pytest.mark.parametrize("name", N2V)
def test_every_step_of_the_reference_run(dev, name):
    fx = Fixture(name)
    ph, model = build_model(fx)
    assert tuple(model.target_embeds.shape) == fx["init/target"].shape
    for s in range(fx.n_steps):
        p = "s%d/" % s
        t0, c0, b0 = fx.tables_before(s, np.float32)
        model.assign_tables(t0, c0, b0)
        b1, b2, neg = fx[p + "batch1"], fx[p + "batch2"], fx[p + "neg_samples"]
        model.inject_negatives(neg)
        loss, ranks, aff_all, mrr, outputs1 = model.train_step({ph['batch1']: b1, ph['batch2']: b2, ph['batch_size']: len(b1)})
        assert np.array_equal(model.neg_samples.cpu().numpy(), neg)
        close(loss, fx[p + "32/loss"], "loss step %d" % s)
        close(aff_all, fx[p + "32/aff_all"], "aff_all")
        close(outputs1, fx[p + "32/outputs1"], "outputs1")
        ref_aff = fx[p + "32/aff_all"]
        margin = np.abs(ref_aff[:, :-1] - ref_aff[:, -1:]).min(axis=1) > 1e-4           # float near-ties aside
        assert np.array_equal(np.asarray(ranks)[margin], fx[p + "32/ranks"][:, -1][margin])
        if margin.all():
            close(mrr, fx[p + "32/mrr"], "mrr")
        t1, c1, bb1 = model.tables()
        rt, rc = fx[p + "rows_target"], fx[p + "rows_context"]
        close(t1[rt], fx[p + "32/after/target"], "target rows after step %d" % s)
        close(c1[rc], fx[p + "32/after/context"], "context rows after step %d" % s)
        close(bb1[rc], fx[p + "32/after/bias"], "bias after step %d" % s)
        rest_t, rest_c = np.setdiff1d(np.arange(len(t0)), rt), np.setdiff1d(np.arange(len(c0)), rc)
        assert np.array_equal(t1[rest_t], t0[rest_t]) and np.array_equal(c1[rest_c], c0[rest_c])
        assert np.array_equal(bb1[rest_c], b0[rest_c])


@pytest.mark.parametrize("name", N2V)
def test_val_and_val_test_rows_of_the_reference_run(dev, name):
    """The whole short run without re-loading anything in between: train epoch, the rows of val.npy, retrain epoch on the
    pruned walk pairs, the rows of val-test.npy (outputs1 of the (n, n) pairs through the evaluation form)."""
    fx = Fixture(name)
    ph, model = build_model(fx)
    model.assign_tables(fx["init/target"], fx["init/context"], fx["init/bias"])

    def run(s0, s1):
        for s in range(s0, s1):
            p = "s%d/" % s
            b1, b2 = fx[p + "batch1"], fx[p + "batch2"]
            model.inject_negatives(fx[p + "neg_samples"])
            model.train_step({ph['batch1']: b1, ph['batch2']: b2, ph['batch_size']: len(b1)})

    def embed(nodes):
        rows = []
        for i in range(0, len(nodes), fx.cfg["embed_batch"]):
            part = nodes[i:i + fx.cfg["embed_batch"]]
            before = model.tables()
            _, _, _, o1 = model.eval_step({ph['batch1']: part, ph['batch2']: part, ph['batch_size']: len(part)})
            assert all(np.array_equal(a, b) for a, b in zip(before, model.tables())), "evaluation must not train"
            rows.append(o1)
        return np.vstack(rows)

    run(0, fx.n_train_steps)
    close(embed(fx["val/nodes"]), fx["val/32/emb"], "val.npy rows")
    run(fx.n_train_steps, fx.n_steps)
    close(embed(fx["val-test/nodes"]), fx["val-test/32/emb"], "val-test.npy rows")
    t_init = fx["init/target"]
    touched = np.unique(np.concatenate([fx["s%d/rows_target" % s] for s in range(fx.n_steps)]))
    rest = np.setdiff1d(np.arange(len(t_init)), touched)
    assert np.array_equal(model.tables()[0][rest], t_init[rest])


# ---------------------------------------------------------------------------------------------------------------
# graphs, reproducibility
# ---------------------------------------------------------------------------------------------------------------
def dense_model(use_graphs, d=128, n_nodes=64, B=512, lr=0.2):
    """A 64-node graph at B = 512: every batch repeats every node several times on both sides, and the 20 negatives are
    a third of all nodes."""
    from graphsage_amd import engine as eng
    from graphsage_amd.models import Node2VecModel, Placeholder
    eng.reset_engine()
    rng = np.random.RandomState(77)
    deg = rng.randint(1, 12, size=n_nodes)
    ph = {k: Placeholder(k) for k in ("batch1", "batch2", "batch_size", "dropout")}
    model = Node2VecModel(ph, n_nodes + 1, deg, nodevec_dim=d, lr=lr, neg_sample_size=20)
    model.use_graphs = use_graphs
    pairs = rng.randint(0, n_nodes, size=(3000, 2)).astype(np.int32)
    model.attach_device_pairs(pairs)
    return model


def test_eight_steps_in_one_graph_equal_eight_single_launches(dev):
    B = 512
    g = dense_model(True)
    g.train_steps_device(B, 8, steps_per_launch=8)                   # first use of the length: eager
    out_g = g.train_steps_device(B, 8, steps_per_launch=8, fetch=True)   # captured and replayed
    assert (B, 8) in g._graphs
    tg = g.tables()
    s = dense_model(False)
    for _ in range(15):
        s.train_step_device(B)
    out_s = s.train_step_device(B, fetch=True)
    ts = s.tables()
    assert int(g._cursor.item()) == int(s._cursor.item()) == 16 * B and int(g.clock_dev.item()) == 16
    for a, b in zip(tg, ts):
        assert np.array_equal(a, b)
    assert out_g[0] == out_s[0] and out_g[3] == out_s[3] and np.array_equal(out_g[2], out_s[2])
    assert np.array_equal(out_g[4], out_s[4])
    assert not np.array_equal(tg[0], dense_model(True).tables()[0])


def test_the_same_200_step_run_twice(dev):
    B = 512
    runs = []
    for _ in range(2):
        m = dense_model(True)
        m.train_steps_device(B, 200, steps_per_launch=8)
        loss = m.train_steps_device(B, 0, fetch=True)[0]
        runs.append((m.tables(), loss))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a, b)
    assert runs[0][1] == runs[1][1] and np.isfinite(runs[0][1])
    assert all(np.isfinite(a).all() for a in runs[0][0])


# ---------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------
def test_unsupervised_train_driver_n2v(dev, tmp_path, capsys):
    """--model n2v --synthetic small end to end.  The learning rate is given (the driver's default, 1e-5, is the reference's
    default for its Adam models: plain SGD on a loss averaged over the batch does not move in one epoch at that rate)."""
    from graphsage_amd import engine as eng
    from graphsage_amd import unsupervised_train as ut
    eng.reset_engine()
    ut.main(["--model", "n2v", "--synthetic", "small", "--learning_rate", "0.5", "--batch_size", "128", "--dim_1", "32",
             "--max_walk_pairs", "60000", "--print_every", "10", "--validate_iter", "100", "--n2v_test_epochs", "1",
             "--base_log_dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert "Epoch: 0001" in out and "Optimization Finished!" in out and "Doing test training for n2v." in out
    pat = (r"Iter: \d{4} train_loss= (\d+\.\d{5}) train_mrr= \d\.\d{5} train_mrr_ema= \d\.\d{5} val_loss= \d+\.\d{5} "
           r"val_mrr= \d\.\d{5} val_mrr_ema= \d\.\d{5} time= \d+\.\d{5}")
    first, retrain = out.split("Doing test training for n2v.")
    losses = [float(x) for x in re.findall(pat, first)]
    assert len(losses) > 20
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), (losses[:5], losses[-5:])
    assert re.search(r"^Iter: \d{4} train_loss= \d+\.\d{5} train_mrr= \d\.\d{5}$", retrain, re.M)
    for line in ("Total time: ", "Walk time: ", "Train time: "):
        assert re.search("^" + line + r" \d+\.\d+", retrain, re.M), line
    files = {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs}
    assert {"val.npy", "val.txt", "val-test.npy", "val-test.txt"} <= set(files)
    assert "/unsup-small/n2v_small_0.500000/" in files["val.npy"]
    ids = open(files["val.txt"]).read().split("\n")
    val, val_test = np.load(files["val.npy"]), np.load(files["val-test.npy"])
    assert len(ids) == len(set(ids)) == val.shape[0] == 3000 and val.shape == val_test.shape == (3000, 64)
    assert open(files["val-test.txt"]).read().split("\n") == ids
    assert np.isfinite(val).all() and np.isfinite(val_test).all()
    # the retrain phase moves the rows of val / test nodes only (every first node of a walk pair is one)
    moved = np.abs(val_test - val).max(axis=1) > 0
    from graphsage_amd import utils
    G = utils.synthetic_graph(n_nodes=3000, feat_dim=50, num_classes=7, avg_degree=8, seed=123, multilabel=False)
    order = np.asarray([int(i) for i in ids])
    assert moved.any() and not moved[~(G.val_mask | G.test_mask)[order]].any()
