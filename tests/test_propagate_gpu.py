"""-m gpu: gs_prop_weights / gs_prop_step / gs_prop_correct and graphsage_amd.propagation against the fp64 oracle."""
import os
import re

import numpy as np
import pytest

import propagate_oracle as po
from graphsage_amd import engine as eng
from graphsage_amd import ops
from graphsage_amd import propagation as pr
from graphsage_amd._lib import GraphsageAmdError
from graphsage_amd.inference import FullGraph

pytestmark = pytest.mark.gpu
SENTINEL = -77.25


def graph_of(lists, n_nodes):
    """FullGraph over the rows `lists` (n_nodes + 1 of them, the pad row last) exactly as they are."""
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    col = np.concatenate([np.asarray(r, dtype=np.int64) for r in lists]) if rowptr[-1] else np.zeros(0, np.int64)
    return FullGraph(rowptr, col, n_nodes)


def table(dev, values, ld):
    """A Mat whose buffer is [rows, ld], SENTINEL everywhere but in the columns of `values`."""
    import torch
    buf = torch.full((values.shape[0], ld), SENTINEL, dtype=torch.float32, device=dev)
    buf[:, :values.shape[1]] = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(dev)
    return ops.Mat(buf, values.shape[1])


def device_step(e, graph, X, out, R, alpha, lo, hi, w=None, d=None):
    import torch
    rowptr, col, items, splits = graph.on(e.device)
    n_slots = int(graph.splits[:, 2].sum()) if graph.splits.shape[0] else 0
    if w is None:
        _, w = ops.prop_weights(rowptr, col, graph.n_rows, graph.n_nodes, stream=e.stream)
    ws = torch.zeros(max(1, ops.prop_ws_bytes(n_slots, X.d if d is None else max(d, 1)) // 4), dtype=torch.float32,
                     device=e.device) if n_slots else None
    torch.cuda.synchronize()
    ops.prop_step(rowptr, col, items, splits, graph.n_rows, graph.split_len, graph.n_nodes, w, X, out, R=R, alpha=alpha, lo=lo,
                  hi=hi, n_slots=n_slots, ws=ws, d=d, stream=e.stream)
    e.sync()
    return w


# ------------------------------------------------------------------------------------------------ exact
EXACT_DEGS = (0, 1, 4, 16, 64, 256, 1024, 4096)
_exact = {}


def exact_graph():
    """Directed rows with duplicates whose real degrees are powers of four (every w a power of two), pad entries at the start,
    in the middle and at the end; an uncut 1024 and 4096 row are 2 and 8 partials, padded ones more; the last row is cut."""
    if not _exact:
        rng = np.random.RandomState(11)
        N = 61
        degs = [EXACT_DEGS[i % 6] for i in range(N)]                 # 0 .. 256 in turn
        degs[7], degs[20], degs[33], degs[N - 1] = 1024, 4096, 1024, 1024
        lists = []
        for r, k in enumerate(degs):
            real = rng.randint(0, N, k)
            real[: k // 4] = real[k // 2: k // 2 + k // 4]           # duplicates
            a, b, c = (0, 0, 0) if r in (7, 20) else rng.randint(0, 4, 3)
            if k == 0:
                a = r % 3                                             # rows of pads only, and empty rows
            h = k // 2
            lists.append(np.concatenate([[N] * a, real[:h], [N] * b, real[h:], [N] * c]).astype(np.int64))
        lists.append(np.array([N], dtype=np.int64))
        _exact["lists"], _exact["N"], _exact["degs"] = lists, N, degs
    return _exact["lists"], _exact["N"], _exact["degs"]


@pytest.mark.parametrize("C", [41, 121, 200])
def test_one_step_is_bit_exact_on_exact_inputs(dev, C):
    lists, N, degs = exact_graph()
    e = eng.get_engine()
    graph = graph_of(lists, N)
    parts = {int(r): int(p) for r, _, p in graph.splits}
    assert parts[7] == 2 and parts[20] == 8 and parts[33] >= 2 and parts[N - 1] >= 2
    rng = np.random.RandomState(C)
    X = rng.randint(-8, 9, (N + 1, C)) * 0.5                          # small integers and halves; the pad row is not 0 here
    R = rng.randint(-8, 9, (N + 1, C)) * 0.5
    deg, w = po.weights(lists, N)
    assert deg[:N].tolist() == degs and set(np.unique(w)) <= {0.0, 1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625}
    Xd, Rd = table(dev, X, 256), table(dev, R, 224)
    rowptr, col, _, _ = graph.on(e.device)
    deg_dev, w_dev = ops.prop_weights(rowptr, col, N + 1, N, stream=e.stream)
    e.sync()
    assert np.array_equal(deg_dev.cpu().numpy(), deg) and np.array_equal(w_dev.cpu().numpy(), w)
    for alpha in (1.0, 0.5):
        for lo, hi in ((-np.inf, np.inf), (-1.5, 2.0)):
            for res in (Rd, None):
                want = po.step(lists, N, w, X, R=R if res is not None else None, alpha=alpha, lo=lo, hi=hi)
                assert np.array_equal(want, want.astype(np.float32).astype(np.float64))      # exact in fp32
                out = table(dev, np.full((N + 1, C), 5.0), 256)
                device_step(e, graph, Xd, out, res, alpha, float(lo), float(hi), w=w_dev)
                got = out.numpy()
                assert np.array_equal(got, want.astype(np.float32)), (alpha, lo, res is not None,
                                                                      np.argwhere(got != want.astype(np.float32))[:5])
                assert not got[N].any()


# ------------------------------------------------------------------------------------------------ edges
EDGE_LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 511, 512, 513, 1025)         # {0, 1, G - 1, G, G + 1, ...} for G = 1, 2, 4
_edge = {}


def edge_graph():
    if not _edge:
        rng = np.random.RandomState(5)
        lengths = list(EDGE_LENGTHS) * 2 + [7, 130, 1025]              # 29 rows + the pad row: 30 rows, the last real row cut
        N = len(lengths)
        lists = [rng.randint(0, N + 1, k).astype(np.int64) for k in lengths]       # directed, duplicates, pad entries anywhere
        lists.append(np.array([N], dtype=np.int64))
        _edge["lists"], _edge["N"] = lists, N
    return _edge["lists"], _edge["N"]


@pytest.mark.parametrize("C", [1, 3, 4, 41, 64, 65, 121, 128, 129, 256])
def test_step_edges_stay_inside_the_fmaf_chain_bound(dev, C):
    lists, N = edge_graph()
    e = eng.get_engine()
    graph = graph_of(lists, N)
    assert (N + 1) % 4 != 0 and graph.items.shape[0] % 4 != 0 and int(graph.splits[-1, 0]) == N - 1
    cpad = (C + 3) // 4 * 4
    rng = np.random.RandomState(100 + C)
    X = rng.randn(N + 1, C).astype(np.float32)
    R = rng.randn(N + 1, C).astype(np.float32)
    Xd, Rd, out = table(dev, X, cpad + 8), table(dev, R, cpad + 4), table(dev, np.full((N + 1, C), 3.0), cpad + 12)
    x_before, r_before = Xd.buf.clone(), Rd.buf.clone()
    deg, w = po.weights(lists, N)
    for alpha, lo, hi, res in ((0.8, -np.inf, np.inf, Rd), (1.0, -0.75, 0.5, Rd), (0.5, -np.inf, np.inf, None)):
        w_dev = device_step(e, graph, Xd, out, res, alpha, float(lo), float(hi))
        assert np.array_equal(w_dev.cpu().numpy(), w)                 # fp64 sqrt and division, rounded once
        want, bound, length = po.step(lists, N, w, X, R=R if res is not None else None, alpha=alpha, lo=lo, hi=hi, with_bound=True)
        got = out.numpy().astype(np.float64)
        err = np.abs(got - want)
        tol = 2.0 ** -24 * (length[:, None] + 8) * bound
        print("C=%d alpha=%g: worst err/tol %.3f" % (C, alpha, float((err / np.maximum(tol, 1e-300)).max())))
        assert (err <= tol).all(), np.argwhere(err > tol)[:5]
        full = out.buf.cpu().numpy()
        assert not full[:, C:cpad].any() and (full[:, cpad:] == SENTINEL).all()      # beyond cpad: untouched
    import torch
    assert torch.equal(Xd.buf, x_before) and torch.equal(Rd.buf, r_before)


def test_refusals_come_before_any_launch(dev):
    import torch
    lists, N = edge_graph()
    e = eng.get_engine()
    graph = graph_of(lists, N)
    X = table(dev, np.zeros((N + 1, 41)), 44)
    out = table(dev, np.zeros((N + 1, 41)), 44)
    narrow = ops.Mat(torch.zeros((N + 1, 40), dtype=torch.float32, device=dev), 40)
    wide = ops.Mat(torch.zeros((N + 1, 260), dtype=torch.float32, device=dev), 260)
    for args, rc in ((dict(X=X, out=out, d=0), -3), (dict(X=wide, out=wide.cols_slice(0, 260), d=257), -3),
                     (dict(X=X, out=X), -1), (dict(X=narrow, out=out, d=41), -1), (dict(X=X, out=narrow, d=41), -1)):
        with pytest.raises(GraphsageAmdError, match=r"rc=%d" % rc):
            device_step(e, graph, args["X"], args["out"], None, 0.5, -1.0, 1.0, d=args.get("d"))
    assert (out.buf[:, :41] == 0).all() and (out.buf[:, 41:] == SENTINEL).all()      # nothing ran


# ------------------------------------------------------------------------------------------------ end to end
_e2e = {}


def e2e_inputs():
    """A connected symmetric graph of 2,000 nodes (a ring, random chords, one hub of more than split_len neighbors) with
    softmax-like and sigmoid-like predictions; every second node known."""
    if "lists" not in _e2e:
        n = 2000
        rng = np.random.RandomState(21)
        adj = [set() for _ in range(n)]

        def link(u, v):
            if u != v:
                adj[u].add(int(v))
                adj[v].add(int(u))
        for u in range(n):
            link(u, (u + 1) % n)
        for u, v in rng.randint(0, n, (6000, 2)):
            link(u, v)
        for v in rng.choice(n, 600, replace=False):
            link(0, v)
        lists = [np.array(sorted(a), dtype=np.int64) for a in adj] + [np.array([n], dtype=np.int64)]
        cls = rng.randint(0, 41, n)
        onehot = np.eye(41)[cls]
        logits = rng.randn(n, 41) + 2.5 * onehot
        soft = np.exp(logits) / np.exp(logits).sum(axis=1, keepdims=True)
        multi = (rng.rand(n, 121) < 0.3).astype(np.float64)
        sig = 1.0 / (1.0 + np.exp(-(rng.randn(n, 121) + 2.0 * (2 * multi - 1))))
        _e2e.update(lists=lists, n=n, known=np.arange(0, n, 2),
                    softmax=(soft.astype(np.float32), onehot.astype(np.float32)),
                    sigmoid=(sig.astype(np.float32), multi.astype(np.float32)))
    return _e2e


def e2e_oracle(kind, alpha, what):
    """The fp64 oracle of one end-to-end case, computed once; the fp32 CPU run of the same algorithm screens the input."""
    key = (kind, alpha, what)
    if key not in _e2e.setdefault("oracle", {}):
        d = e2e_inputs()
        preds, labels = d[kind]
        if what == "lp":
            a = {"preds": po.label_propagation(d["lists"], d["n"], labels, d["known"], alpha=alpha, iters=20)}
            b = {"preds": po.label_propagation(d["lists"], d["n"], labels, d["known"], alpha=alpha, iters=20, dtype=np.float32)}
        else:
            a = po.correct_and_smooth(d["lists"], d["n"], preds, labels, d["known"], alpha, alpha, 20)
            b = po.correct_and_smooth(d["lists"], d["n"], preds, labels, d["known"], alpha, alpha, 20, dtype=np.float32)
        keep = np.ones(d["n"], bool)
        if what == "cs":
            keep = ~(np.abs(a["raw_scale"] - 1000.0) <= 10.0)            # sigma / l1 within 1 % of the cap: either side is right
            assert (~keep).mean() <= 0.01
        assert np.abs(a["preds"][keep] - b["preds"][keep]).max() <= 2.5e-5      # the input is mild enough for fp32
        _e2e["oracle"][key] = (a, keep)
    return _e2e["oracle"][key]


@pytest.mark.parametrize("alpha", [0.8, 0.5])
@pytest.mark.parametrize("kind", ["softmax", "sigmoid"])
def test_correct_and_smooth_equals_the_oracle(dev, kind, alpha):
    d = e2e_inputs()
    want, keep = e2e_oracle(kind, alpha, "cs")
    preds, labels = d[kind]
    e = eng.get_engine()
    graph = graph_of(d["lists"], d["n"])
    assert graph.splits.shape[0] == 1                                  # the hub is a cut row
    got = pr.correct_and_smooth(e, graph, preds, labels, d["known"], correct_alpha=alpha, smooth_alpha=alpha, iters=20)
    assert got["iters"] == 20 and got["sigma"] == pytest.approx(want["sigma"], rel=1e-6)      # E0 is formed in fp32
    for key in ("corrected", "preds"):
        err = np.abs(got[key].astype(np.float64) - want[key])[keep].max()
        print("%s alpha=%g %s: max err %.3g" % (kind, alpha, key, err))
        assert err <= 1e-4
    assert np.array_equal(got["corrected"][d["known"]], labels[d["known"]])
    assert got["preds"].min() >= 0.0 and got["preds"].max() <= 1.0


@pytest.mark.parametrize("alpha", [0.8, 0.5])
def test_label_propagation_equals_the_oracle(dev, alpha):
    d = e2e_inputs()
    want, _ = e2e_oracle("softmax", alpha, "lp")
    got = pr.label_propagation(eng.get_engine(), graph_of(d["lists"], d["n"]), d["softmax"][1], d["known"], alpha=alpha, iters=20)
    err = np.abs(got.astype(np.float64) - want["preds"]).max()
    print("label propagation alpha=%g: max err %.3g" % (alpha, err))
    assert got.shape == (d["n"], 41) and err <= 1e-4


def test_two_runs_give_the_same_bits(dev):
    d = e2e_inputs()
    preds, labels = d["softmax"]
    e = eng.get_engine()
    graph = graph_of(d["lists"], d["n"])
    a = pr.correct_and_smooth(e, graph, preds, labels, d["known"], iters=10)
    b = pr.correct_and_smooth(e, graph, preds, labels, d["known"], iters=10, propagator=pr.Propagator(e, graph))
    assert np.array_equal(a["preds"], b["preds"]) and np.array_equal(a["corrected"], b["corrected"]) and a["sigma"] == b["sigma"]


def test_run_without_the_residual_and_device_result(dev):
    """keep_residual=False is the bare operator; device=True hands the table back without a copy to the host."""
    lists, N = edge_graph()
    e = eng.get_engine()
    prop = pr.Propagator(e, graph_of(lists, N))
    X0 = np.random.RandomState(3).randn(N, 5).astype(np.float32)
    want = po.run(lists, N, X0, 0.9, 3, keep_residual=False)
    M = prop.run(X0, 0.9, 3, keep_residual=False, device=True)
    assert isinstance(M, ops.Mat) and M.rows == N + 1 and M.ld % 32 == 0 and M.d == 5
    host = M.numpy()[:N].copy()                                        # M lives in a ping-pong table: the next run reuses it
    assert np.abs(host - want).max() <= 1e-4 and not M.numpy()[N].any()
    from_device = prop.run(M, 1.0, 1, keep_residual=False)
    assert np.array_equal(from_device, prop.run(host, 1.0, 1, keep_residual=False))


# ------------------------------------------------------------------------------------------------ model and driver
def test_model_method_is_predict_full_then_correct_and_smooth(dev):
    from ref_fixtures import Fixture
    from test_ref_pin_gpu import build_supervised, load_weights
    fx = Fixture("sup_mean_full_degree")
    e, ph, adj_info, sampler, model = build_supervised(fx)
    load_weights(model, fx, "init/")
    N = fx.n_nodes
    graph = FullGraph.from_csr(fx["graph/full_rowptr"], fx["graph/full_col"], N)
    labels = fx["graph/labels"].astype(np.float32)
    known = np.arange(0, N, 3)
    res = model.correct_and_smooth(graph, labels, known, iters=5, correct_alpha=0.7)
    _, preds = model.predict_full(graph)
    want = pr.correct_and_smooth(e, graph, preds, labels, known, iters=5, correct_alpha=0.7)
    assert res["preds"].shape == labels.shape and res["sigma"] == want["sigma"]
    assert np.array_equal(res["preds"], want["preds"]) and np.array_equal(res["corrected"], want["corrected"])
    some = model.correct_and_smooth(graph, labels, known, nodes=[5, 1, 5], iters=5, correct_alpha=0.7)
    assert np.array_equal(some["preds"], want["preds"][[5, 1, 5]])
    with pytest.raises(GraphsageAmdError):
        model.correct_and_smooth(graph, labels, known, nodes=[N])


COMMON = ["--synthetic", "small", "--epochs", "1", "--batch_size", "128", "--samples_1", "5", "--samples_2", "3", "--dim_1", "32",
          "--dim_2", "32", "--max_total_steps", "6", "--validate_iter", "10", "--print_every", "5"]
F1 = r"\d\.\d{5}"


def files_under(path):
    return {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(path)) for f in fs}


def run_driver(argv):
    from graphsage_amd import inits
    from graphsage_amd import supervised_train as st
    eng.reset_engine()
    np.random.seed(st.seed)
    inits.set_seed(123)
    st.main(argv)


def test_supervised_driver_with_and_without_the_flags(dev, tmp_path, capsys):
    run_driver(COMMON + ["--base_log_dir", str(tmp_path / "on"), "--correct_smooth", "--label_propagation", "--cs_iters", "10",
                         "--cs_correct_alpha", "0.7"])
    on = capsys.readouterr().out
    line = [l for l in on.splitlines() if l.startswith("Correct and smooth:")]
    assert len(line) == 1 and re.match(
        r"Correct and smooth: nodes= 3000 known= \d+ classes= 7 correct_alpha= 0.7 smooth_alpha= 0.8 iters= 10 sigma= \d+\.\d{5} "
        r"base_val_f1_micro= %s val_f1_micro= %s val_f1_macro= %s base_test_f1_micro= %s test_f1_micro= %s test_f1_macro= %s "
        r"time= \d+\.\d{5}$" % ((F1,) * 6), line[0]), line
    line = [l for l in on.splitlines() if l.startswith("Label propagation:")]
    assert len(line) == 1 and re.match(
        r"Label propagation: nodes= 3000 known= \d+ classes= 7 alpha= 0.8 iters= 10 val_f1_micro= %s val_f1_macro= %s "
        r"test_f1_micro= %s test_f1_macro= %s time= \d+\.\d{5}$" % ((F1,) * 4), line[0]), line
    files = files_under(tmp_path / "on")
    for tag in ("cs", "lp"):
        assert re.match(r"f1_micro=%s f1_macro=%s time=\d+\.\d{5}$" % (F1, F1), open(files["val_stats_%s.txt" % tag]).read())
        assert re.match(r"f1_micro=%s f1_macro=%s$" % (F1, F1), open(files["test_stats_%s.txt" % tag]).read())

    run_driver(COMMON + ["--base_log_dir", str(tmp_path / "off")])
    off = capsys.readouterr().out
    assert "Correct and smooth" not in off and "Label propagation" not in off
    plain = files_under(tmp_path / "off")
    assert sorted(plain) == sorted(f for f in files if not re.search(r"_(cs|lp)\.txt$", f))
    # the other outputs are what they were: the same log but for the two lines and the wall-clock figures
    strip = lambda text: [re.sub(r"time= ?\d+\.\d+", "time=", l) for l in text.splitlines()
                          if not l.startswith(("Correct and smooth:", "Label propagation:"))]
    assert strip(on) == strip(off)
    for name in ("val_stats.txt", "test_stats.txt"):
        assert re.sub(r"time=\S+", "", open(files[name]).read()) == re.sub(r"time=\S+", "", open(plain[name]).read())
