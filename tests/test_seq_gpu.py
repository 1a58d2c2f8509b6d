"""-m gpu: the LSTM aggregator (graphsage_seq) on the gfx950 kernels of csrc/gs_lstm.hip.

  * the recurrence kernels alone == NumPy (tests/seq_oracle.py) for H in {128, 256}, L = 1, L = T, an interior zero row and
    a sequence count that is not a multiple of the 16-sequence tile;
  * every step of the reference's own runs (tests/golden/ref_{sup_seq,sup_seq_big_sigmoid,unsup_seq}.npz) within the
    tolerances of test_ref_pin_gpu: sampled ids bit-exact, loss, predictions, embeddings, every gradient, post-Adam parameters
    (the LSTM kernel's gradient and post-Adam values through the fixtures' sketches), evaluation on the test adjacency;
  * eight steps replayed as one captured graph == eight single steps, bit for bit;
  * both training drivers run --model graphsage_seq."""
import os
import re

import numpy as np
import pytest
import torch

import seq_oracle as so
from graphsage_amd import engine as eng
from graphsage_amd import inits, ops
from graphsage_amd.neigh_samplers import PaddedAdjacency
from ref_fixtures import Fixture
from test_ref_pin_gpu import ADAM_KNEE, RTOL, build_supervised, close

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------
# the kernels alone
# ---------------------------------------------------------------------------------------------------------------
def _kernel_case(H, seg_shapes, seed):
    """Segments (n, T) of random inputs with the length cases planted; returns the device results and NumPy's."""
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(seed)
    D = 12
    xs = [rng.randn(n, T, D).astype(np.float32) for n, T in seg_shapes]
    for x in xs:
        T = x.shape[1]
        x[0] = 0.0                              # L = 1 (a degree-0 node: pad rows only)
        if len(x) > 1 and T > 2:
            x[1, 1] = 0.0                        # interior zero row: L = T - 1, step 1 runs, the last step is dropped
        if len(x) > 2:
            x[2, T - 1] = 0.0                    # trailing zero row
        # the rest: L = T
    kernel = rng.uniform(-0.15, 0.15, (D + H, 4 * H)).astype(np.float32)
    bias = rng.uniform(-0.1, 0.1, 4 * H).astype(np.float32)
    rows = sum(n * T for n, T in seg_shapes)
    n_total = sum(n for n, _ in seg_shapes)
    X = ops.Mat.from_numpy(np.concatenate([x.reshape(-1, D) for x in xs]), dev)
    segs, r = [], 0
    for n, T in seg_shapes:
        segs.append((X.rows_slice(r, r + n * T), None, n, T, r))
        r += n * T
    G = ops.Mat.from_numpy(X.numpy().astype(np.float64) @ kernel[:D].astype(np.float64) + bias, dev)
    Wh = ops.Mat.from_numpy(kernel[D:], dev)
    L = torch.zeros(n_total, dtype=torch.int32, device=dev)
    C, Hp, hl = ops.Mat.zeros(rows, H, dev), ops.Mat.zeros(rows, H, dev), ops.Mat.zeros(n_total, H, dev)
    ops.lstm_lengths(segs, D, L)
    ops.lstm_fwd(segs, H, Wh, L, G, G, C, Hp, hl)
    dh = rng.randn(n_total, H).astype(np.float32)
    dG = ops.Mat.zeros(rows, 4 * H, dev)
    wt = torch.zeros(4 * H * H, dtype=torch.float32, device=dev)
    ops.lstm_bwd(segs, H, Wh, wt, L, G, C, ops.Mat.from_numpy(dh, dev), dG)
    torch.cuda.synchronize()
    return xs, kernel, bias, dh, L.cpu().numpy(), hl.numpy(), dG.numpy(), Hp.numpy()


@pytest.mark.parametrize("H,seg_shapes", [(128, [(37, 5), (3, 1), (21, 9)]), (256, [(19, 7), (16, 3)]),
                                          (128, [(16, 25)])])
def test_lstm_kernels_equal_numpy(dev, H, seg_shapes):
    xs, kernel, bias, dh, L, hl, dG, Hp = _kernel_case(H, seg_shapes, seed=H + len(seg_shapes))
    D = xs[0].shape[2]
    k64, b64 = kernel.astype(np.float64), bias.astype(np.float64)
    s0 = r0 = 0
    for x, (n, T) in zip(xs, seg_shapes):
        x64 = x.astype(np.float64)
        Lr = so.lengths(x64)
        assert np.array_equal(L[s0:s0 + n], Lr)
        assert Lr[0] == 1 and (T <= 2 or n < 2 or Lr[1] == T - 1) and (n < 4 or Lr[3] == T)
        h_ref, cache = so.lstm_fwd(x64, Lr, k64, b64)
        close(hl[s0:s0 + n], h_ref, "h_last (H=%d, T=%d)" % (H, T))
        dx, dk, db = so.lstm_bwd(dh[s0:s0 + n].astype(np.float64), cache)
        g = dG[r0:r0 + n * T].astype(np.float64)
        steps = np.arange(n * T) % T
        assert not g[steps >= np.repeat(Lr, T)].any()                       # no gradient past a sequence's length
        hp = Hp[r0:r0 + n * T].astype(np.float64)
        close(g.sum(axis=0), db, "bias grad")
        close(x64.reshape(-1, D).T @ g, dk[:D], "W_x grad")
        close(hp.T @ g, dk[D:], "W_h grad")
        close((g @ k64[:D].T).reshape(n, T, D), dx, "input grad")
        s0 += n
        r0 += n * T


# ---------------------------------------------------------------------------------------------------------------
# the reference's own runs
# ---------------------------------------------------------------------------------------------------------------
class SeqVars(object):
    """name (fixture naming) -> getter / setter over the engine's variables; agg%d/lstm_kernel is [lstm_wx ; lstm_wh]."""

    def __init__(self, model, supervised=True):
        self.full = {}
        self.aggs = model.aggregators
        for i, a in enumerate(model.aggregators):
            for k, v in a.vars.items():
                self.full["agg%d/%s" % (i, k)] = v
            self.full["agg%d/lstm_bias" % i] = a.lstm_b
        if supervised:
            self.full["node_pred/weights"] = model.node_pred.vars['weights']
            self.full["node_pred/bias"] = model.node_pred.vars['bias']

    def kernel(self, i, grad=False):
        a = self.aggs[i]
        f = (lambda v: v.grad.numpy()) if grad else (lambda v: v.numpy())
        return np.concatenate([f(a.lstm_wx), f(a.lstm_wh)], axis=0)

    def load(self, fx, prefix, with_kernels=True):
        for k, v in self.full.items():
            v.assign(fx[prefix + k].astype(np.float32).reshape(v.numpy().shape))
        if with_kernels:
            for i, a in enumerate(self.aggs):
                w = fx["%sagg%d/lstm_kernel" % (prefix, i)].astype(np.float32)
                a.lstm_wx.assign(w[:a.lstm_wx.rows])
                a.lstm_wh.assign(w[a.lstm_wx.rows:])
        eng.get_engine().sync()


def _check_sketch(got, fx, key, msg):
    for part, v in so.sketch(got).items():
        close(v, fx["%s#%s" % (key, part)], "%s#%s" % (msg, part))


def _check_step(fx, p, sv, n_layers):
    for k, v in sv.full.items():
        close(v.grad.numpy(), fx[p + "32/grad/" + k], "grad/" + k)
        want, g = fx[p + "32/after/" + k], fx[p + "32/grad/" + k]
        solid = np.abs(g) > max(1e-6 * max(1e-2, np.abs(g).max()), ADAM_KNEE)
        np.testing.assert_allclose(v.numpy().reshape(want.shape)[solid], want[solid], rtol=RTOL, atol=2e-5, err_msg="after/" + k)
    for i in range(n_layers):
        key = "agg%d/lstm_kernel" % i
        _check_sketch(sv.kernel(i, grad=True), fx, p + "32/grad/" + key, "grad/" + key)
        idx = so.sketch_index(sv.kernel(i).shape)
        g, want = fx[p + "32/grad/%s#pick" % key], fx[p + "32/after/%s#pick" % key]
        solid = np.abs(g) > max(1e-6 * max(1e-2, np.abs(g).max()), ADAM_KNEE)
        np.testing.assert_allclose(sv.kernel(i).reshape(-1)[idx][solid], want[solid], rtol=RTOL, atol=2e-5, err_msg="after/" + key)


@pytest.mark.parametrize("name", ["sup_seq", "sup_seq_big_sigmoid"])
def test_supervised_seq_steps_equal_reference_run(dev, name):
    fx = Fixture(name)
    e, ph, adj_info, sampler, model = build_supervised(fx)
    assert model.aggregators[0].hidden_dim == (256 if fx.cfg.get("model_size") == "big" else 128)
    sv = SeqVars(model)
    sv.load(fx, "init/")
    for s in range(fx.n_steps):
        p = "s%d/" % s
        batch, labels = fx[p + "batch"], fx[p + "labels"]
        sampler.inject_perms(fx.perms(p, fx.K))
        loss, preds = model.train_step({ph['batch']: batch, ph['labels']: labels, ph['batch_size']: len(batch)})
        for k in range(fx.K):
            assert np.array_equal(model.samples1[k + 1].cpu().numpy(), fx[p + "sampled%d" % k].reshape(-1)), (s, k)
        close(loss, fx[p + "32/loss"], "loss step %d" % s)
        close(preds, fx[p + "32/preds"], "preds step %d" % s)
        close(model.outputs1.numpy(), fx[p + "32/outputs1"], "outputs1 step %d" % s)
        _check_step(fx, p, sv, fx.K)
        sv.load(fx, p + "32/after/", with_kernels=False)       # continue from the reference's parameters (kernels: the device's)
    if fx.has("eval/batch"):
        # supervised_train.py:280-285: evaluation on the test adjacency after the run (tf.assign(adj_info, test_adj))
        adj_info.assign(PaddedAdjacency(fx["graph/adj_test"], e.device))
        sampler.inject_perms(fx.perms("eval/", fx.K))
        batch, labels = fx["eval/batch"], fx["eval/labels"]
        loss, preds = model.eval_step({ph['batch']: batch, ph['labels']: labels, ph['batch_size']: len(batch)})
        for k in range(fx.K):
            assert np.array_equal(model.samples1[k + 1].cpu().numpy(), fx["eval/sampled%d" % k].reshape(-1))
        close(loss, fx["eval/32/loss"], "eval loss")
        close(preds, fx["eval/32/preds"], "eval preds")


def test_unsupervised_seq_steps_equal_reference_run(dev):
    from graphsage_amd.models import Placeholder, SAGEInfo, SampleAndAggregate
    from graphsage_amd.neigh_samplers import AdjInfo, UniformNeighborSampler
    fx = Fixture("unsup_seq")
    c = fx.cfg
    K, n_neg = fx.K, c["neg_sample_size"]
    eng.reset_engine()
    inits.set_seed(1)
    e = eng.get_engine()
    ph = {'batch1': Placeholder('batch1'), 'batch2': Placeholder('batch2'), 'neg_samples': Placeholder('neg'),
          'dropout': Placeholder('dropout', 0.), 'batch_size': Placeholder('batch_size')}
    adj_info = AdjInfo(PaddedAdjacency(fx["graph/adj_train"], e.device))
    sampler = UniformNeighborSampler(adj_info)
    layer_infos = [SAGEInfo("node", sampler, s, fx.out_dim) for s in c["num_samples"]]
    model = SampleAndAggregate(ph, fx["graph/feats"], adj_info, fx["graph/deg"], layer_infos, concat=c["concat"],
                               aggregator_type="seq", learning_rate=c["learning_rate"], weight_decay=c["weight_decay"],
                               neg_sample_size=n_neg)
    model.use_graphs = False
    sv = SeqVars(model, supervised=False)
    sv.load(fx, "init/")
    for s in range(fx.n_steps):
        p = "s%d/" % s
        b1, b2, neg = fx[p + "batch1"], fx[p + "batch2"], fx[p + "neg_samples"]
        B = len(b1)
        sampler.inject_perms(fx.perms(p, 3 * K))
        model.inject_negatives(neg)
        loss, ranks, aff_all, mrr, outputs1 = model.train_step({ph['batch1']: b1, ph['batch2']: b2, ph['batch_size']: B})
        for k in range(K):
            want = np.concatenate([fx[p + "sampled%d" % (g * K + k)].reshape(-1) for g in range(3)])
            assert np.array_equal(model.samples1[k + 1].cpu().numpy(), want), (s, k)
        close(loss, fx[p + "32/loss"], "loss step %d" % s)
        close(aff_all, fx[p + "32/aff_all"], "aff_all")
        close(outputs1, fx[p + "32/outputs1"], "outputs1")
        full = model.outputs_all.numpy()
        close(full[B:2 * B], fx[p + "32/outputs2"], "outputs2")
        close(full[2 * B:2 * B + n_neg], fx[p + "32/neg_outputs"], "neg_outputs")
        _check_step(fx, p, sv, K)
        sv.load(fx, p + "32/after/", with_kernels=False)


def test_identity_features_are_refused_with_seq(dev):
    from graphsage_amd._lib import GraphsageAmdError
    fx = Fixture("sup_seq")
    fx.identity_dim = 4
    with pytest.raises(GraphsageAmdError, match="identity_dim"):
        build_supervised(fx)


# ---------------------------------------------------------------------------------------------------------------
# graph replay, drivers
# ---------------------------------------------------------------------------------------------------------------
def test_seq_multistep_graph_equals_single_steps(dev):
    """Eight steps per captured graph == one step per launch == the eager schedule, bit for bit (Reddit-shaped step)."""
    from test_bench_parity_gpu import B, build
    outs = []
    for mode in ("multi", "single", "eager"):
        G, it, model, order = build("seq")
        if mode == "multi":
            model.train_steps_device(B, 17, steps_per_launch=8)
        elif mode == "single":
            for _ in range(17):
                model.train_step_device(B)
        else:
            model.use_graphs = False
            for _ in range(17):
                model.train_step_device(B)
        loss, preds = model._fetch(B)
        outs.append((loss, preds.copy(), model.engine.params.cpu().numpy().copy()))
    for other in outs[1:]:
        assert outs[0][0] == other[0]
        assert np.array_equal(outs[0][1], other[1])
        assert np.array_equal(outs[0][2], other[2])
    assert np.isfinite(outs[0][0])


def test_supervised_train_driver_seq(dev, tmp_path, capsys):
    from graphsage_amd import supervised_train as st
    eng.reset_engine()
    f1 = st.main(["--synthetic", "small", "--epochs", "2", "--batch_size", "128", "--samples_1", "5", "--samples_2", "3",
                  "--dim_1", "32", "--dim_2", "32", "--validate_iter", "10", "--print_every", "5",
                  "--base_log_dir", str(tmp_path), "--model", "graphsage_seq"])
    out = capsys.readouterr().out
    assert "Epoch: 0001" in out and "Optimization Finished!" in out and "Full validation stats:" in out
    assert re.search(r"Iter: \d{4} train_loss= \d+\.\d{5} train_f1_mic= \d\.\d{5} .* val_f1_mic= \d\.\d{5} .* time= \d+\.\d{5}", out)
    stats = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs]
    assert any(p.endswith("val_stats.txt") for p in stats) and any(p.endswith("test_stats.txt") for p in stats)
    txt = open([p for p in stats if p.endswith("val_stats.txt")][0]).read()
    assert re.match(r"loss=\d+\.\d{5} f1_micro=\d\.\d{5} f1_macro=\d\.\d{5} time=\d+\.\d{5}", txt)
    assert f1 > 0.6, f1


def test_unsupervised_train_driver_seq(dev, tmp_path, capsys):
    from graphsage_amd import unsupervised_train as ut
    eng.reset_engine()
    ut.main(["--synthetic", "small", "--model", "graphsage_seq", "--epochs", "1", "--batch_size", "128", "--samples_1", "5",
             "--samples_2", "3", "--dim_1", "32", "--dim_2", "32", "--max_total_steps", "20", "--print_every", "10",
             "--validate_iter", "10", "--max_walk_pairs", "20000", "--base_log_dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert "Optimization Finished!" in out
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path)) for f in fs]
    emb = [p for p in files if p.endswith("val.npy")]
    assert emb and any(p.endswith("val.txt") for p in files)
    assert np.isfinite(np.load(emb[0])).all()
