"""-m gpu: the fused score-and-count kernel (gs_rank_count) and rank_full against an fp64 NumPy oracle written here.

1. exact on a lattice (integer entries in [-3, 3]: every dot product is exact in fp32 in any order) at every edge of the
   128 x 128 tiling and of the slices of 4 tiles, with bit-duplicate copies of the target row;
2. the filter's edge cases on the same lattice, exact;
3. real-valued rows inside the derived fp32 dot-product band;
4. the reference's own runs: n_gt + n_eq == the rank the reference computed in the batch;
5. model.rank_full == the oracle applied to model.embed_full."""
import numpy as np
import pytest

from graphsage_amd import engine as eng
from graphsage_amd import ops
from graphsage_amd.inference import FullGraph, RankFilter
from ref_fixtures import Fixture

pytestmark = pytest.mark.gpu
BM = BN = 128            # the kernel's tile (csrc/gs_rank.hip)
SLICE = 4 * BN           # candidates per slice while the query tiles are few (4 tiles per slice)


# ------------------------------------------------------------------------------------------------ oracle
def candidates(Q, n_cand, dst, src=None, flists=None, keep_src=False):
    """bool [Q, n_cand]: w is a candidate of q (keep_src: src only names the filter row)."""
    C = np.ones((Q, n_cand), dtype=bool)
    for q in range(Q):
        if dst[q] < n_cand:
            C[q, dst[q]] = False
        if src is not None:
            if src[q] < n_cand and not keep_src:
                C[q, src[q]] = False
            if flists is not None:
                f = np.asarray(flists[src[q]], dtype=np.int64)
                C[q, f[f < n_cand]] = False
    return C


def oracle(Xq, Zc, dst, n_cand, src=None, flists=None, keep_src=False):
    """(S [Q, n_cand], t [Q], candidate mask) in fp64."""
    X64, Z64 = Xq.astype(np.float64), Zc.astype(np.float64)
    S = X64 @ Z64[:n_cand].T
    t = np.einsum("qd,qd->q", X64, Z64[dst])
    return S, t, candidates(Xq.shape[0], n_cand, dst, src, flists, keep_src)


def exact_counts(S, t, C):
    return ((S > t[:, None]) & C).sum(1), ((S == t[:, None]) & C).sum(1)


def run(dev, Xq, Zc, dst, n_cand, src=None, filt=None, keep_src=False):
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    f_rowptr, f_col = filt.on(dev, Zc.shape[0]) if filt is not None else (None, None)
    t, n_gt, n_eq = ops.rank_count(ops.Mat.from_numpy(Xq, dev), ops.Mat.from_numpy(Zc, dev), up(dst), n_cand=n_cand,
                                   src=None if src is None else up(src), f_rowptr=f_rowptr, f_col=f_col,
                                   keep_src=keep_src)
    torch.cuda.synchronize()
    return t.cpu().numpy(), n_gt.cpu().numpy().astype(np.int64), n_eq.cpu().numpy().astype(np.int64)


def lattice(rng, rows, d):
    return rng.randint(-3, 4, size=(rows, d)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. exact, on a lattice
@pytest.mark.parametrize("d", [4, 36, 64, 256, 512])
def test_lattice_exact_at_every_tile_and_slice_edge(dev, d):
    rng = np.random.RandomState(d)
    # 1031 candidates = 9 tiles = slices of 4, 4, 1 tiles (ragged last slice, three slices); 700 = a ragged second slice
    for Q in (1, BM - 1, BM, BM + 1):
        for n_cand in (1, BN - 1, BN, BN + 1, 700, 1031):
            for dst_inside in (True, False):
                n_rows = n_cand if dst_inside else n_cand + 37
                Zc = lattice(rng, n_rows, d)
                Xq = lattice(rng, Q, d)
                dst = rng.randint(0, n_cand, size=Q) if dst_inside else rng.randint(n_cand, n_rows, size=Q)
                # bit-duplicate copies of the first queries' target rows, at both ends and in the middle of the candidates
                dups = {}
                if n_cand >= BN - 1:
                    spots = [w for w in (0, 5, n_cand // 2, n_cand - 2, n_cand - 1) if w not in set(dst[:3])]
                    for i, w in enumerate(spots):
                        q = i % min(Q, 3)
                        Zc[w] = Zc[dst[q]]
                        dups.setdefault(q, []).append(w)
                S, t, C = oracle(Xq, Zc, dst, n_cand)
                assert np.abs(S).max() <= 9 * d and np.array_equal(S, S.astype(np.float32))        # exact in fp32
                want_gt, want_eq = exact_counts(S, t, C)
                got_t, got_gt, got_eq = run(dev, Xq, Zc, dst, n_cand)
                tag = "Q=%d n_cand=%d n_rows=%d d=%d" % (Q, n_cand, n_rows, d)
                assert np.array_equal(got_t.astype(np.float64), t), tag
                assert np.array_equal(got_gt, want_gt), tag
                assert np.array_equal(got_eq, want_eq), tag
                for q, ws in dups.items():
                    # (a later copy may have overwritten an earlier one's source row: count what still is a copy)
                    n = sum(1 for w in set(ws) if w != dst[q] and np.array_equal(Zc[w], Zc[dst[q]]))
                    assert got_eq[q] >= n, tag


def test_lattice_exact_with_several_query_tiles_and_self_exclusion(dev):
    """Three query tiles against seven slices, src given (excluded), src == dst for some queries."""
    rng = np.random.RandomState(11)
    Q, n_cand, n_rows, d = 2 * BM + 3, 7 * SLICE - 77, 7 * SLICE, 36
    Zc, Xq = lattice(rng, n_rows, d), lattice(rng, Q, d)
    src, dst = rng.randint(0, n_rows, size=Q), rng.randint(0, n_rows, size=Q)
    dst[:5] = src[:5]
    S, t, C = oracle(Xq, Zc, dst, n_cand, src)
    want_gt, want_eq = exact_counts(S, t, C)
    got_t, got_gt, got_eq = run(dev, Xq, Zc, dst, n_cand, src)
    assert np.array_equal(got_t.astype(np.float64), t)
    assert np.array_equal(got_gt, want_gt) and np.array_equal(got_eq, want_eq)
    assert (want_eq > 0).any() and (want_gt > 0).any()


def test_lattice_exact_across_the_query_chunk_of_the_binding(dev):
    """More queries than one gs_rank_count call takes (ops.RANK_CHUNK): the second call's rows, targets and outputs are offset."""
    rng = np.random.RandomState(13)
    Q, n_cand, n_rows, d = ops.RANK_CHUNK + BM + 2, 5, 9, 4
    Zc, Xq = lattice(rng, n_rows, d), lattice(rng, Q, d)
    src, dst = rng.randint(0, n_rows, size=Q), rng.randint(0, n_rows, size=Q)
    S, t, C = oracle(Xq, Zc, dst, n_cand, src)
    want_gt, want_eq = exact_counts(S, t, C)
    got_t, got_gt, got_eq = run(dev, Xq, Zc, dst, n_cand, src)
    assert np.array_equal(got_t.astype(np.float64), t)
    assert np.array_equal(got_gt, want_gt) and np.array_equal(got_eq, want_eq)
    assert want_gt[ops.RANK_CHUNK:].any() and want_eq[ops.RANK_CHUNK:].any()


# ------------------------------------------------------------------------------------------------ 2. filter edges
def test_filter_edges_on_the_lattice(dev):
    rng = np.random.RandomState(5)
    n_rows, n_cand, d, Q = 1100, 1031, 36, BM + 2
    Zc, Xq = lattice(rng, n_rows, d), lattice(rng, Q, d)
    flists = [np.sort(rng.choice(n_rows, size=rng.randint(0, 40), replace=False)) for _ in range(n_rows)]
    flists[0] = np.zeros(0, np.int64)                                          # an empty row
    flists[1] = np.arange(n_cand)                                              # a hub: every candidate
    flists[2] = np.concatenate([np.arange(BN - 8, BN + 8), np.arange(SLICE - 7, SLICE + 9)])     # runs over a tile / slice edge
    flists[3] = np.asarray([0, SLICE - 1, SLICE, 2 * SLICE - 1, 2 * SLICE, n_cand - 1])         # first / last of every slice
    flists[4] = np.asarray([7, 300, 900, 1050])                                # holds its query's own dst (300)
    flists[5] = np.asarray([5, 6, BN, n_cand, n_rows - 1])                     # src == dst == 5, entries beyond n_cand
    flists[6] = np.arange(0, n_rows, 2)                                        # two queries share it
    flists[8] = np.arange(n_rows)                                              # a hub beyond n_cand too
    src = rng.randint(9, n_rows, size=Q)
    dst = rng.randint(0, n_rows, size=Q)
    src[:10] = [0, 1, 2, 3, 4, 5, 6, 6, 8, 1]
    dst[4], dst[5], dst[6], dst[7] = 300, 5, 10, 1040
    src[Q - 1], src[BM - 1], src[BM] = 3, 2, 1                                 # the same rows in the second query tile
    rowptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum([len(f) for f in flists], out=rowptr[1:])
    order = [rng.permutation(len(f)) for f in flists]                          # handed over unsorted, with duplicates
    col = np.concatenate([np.concatenate([f[o], f[o][:3]]) for f, o in zip(flists, order)])
    rowptr2 = np.zeros(n_rows + 1, np.int64)
    np.cumsum([len(f) + min(3, len(f)) for f in flists], out=rowptr2[1:])
    filt = RankFilter.from_csr(rowptr2, col, n_rows)
    assert np.array_equal(filt.rowptr, rowptr) and all(np.array_equal(a, b) for a, b in zip(filt.lists(), flists))
    S, t, C = oracle(Xq, Zc, dst, n_cand, src, flists)
    want_gt, want_eq = exact_counts(S, t, C)
    got_t, got_gt, got_eq = run(dev, Xq, Zc, dst, n_cand, src, filt)
    assert np.array_equal(got_t.astype(np.float64), t)
    assert np.array_equal(got_gt, want_gt) and np.array_equal(got_eq, want_eq)
    for q in (1, 8, 9, BM):
        assert got_gt[q] == 0 and got_eq[q] == 0                               # hubs: nothing left to count
    # dst inside its own filter row is left out once: the same counts as with that entry removed from the row
    flists4 = list(flists)
    flists4[4] = np.asarray([7, 900, 1050])
    g4, e4 = exact_counts(*oracle(Xq[4:5], Zc, dst[4:5], n_cand, src[4:5], flists4))
    assert (got_gt[4], got_eq[4]) == (g4[0], e4[0])
    # the query node kept as a candidate (it then only names its filter row), unless its own row lists it
    S, t, C = oracle(Xq, Zc, dst, n_cand, src, flists, keep_src=True)
    k_t, k_gt, k_eq = run(dev, Xq, Zc, dst, n_cand, src, filt, keep_src=True)
    assert np.array_equal(k_t, got_t) and [np.array_equal(a, b) for a, b in zip((k_gt, k_eq), exact_counts(S, t, C))] == [True] * 2
    assert (k_gt + k_eq >= got_gt + got_eq).all() and (k_gt + k_eq > got_gt + got_eq).any()
    # the same through inference.rank_full(exclude_self=False, filt=...): the two options are independent
    from graphsage_amd import inference as inf
    eng.reset_engine()
    res = inf.rank_full(eng.get_engine(), ops.Mat.from_numpy(Zc, dev), np.stack([src, dst], axis=1), n_cand=n_cand, filt=filt,
                        exclude_self=False)
    r_gt, r_eq = exact_counts(*oracle(Zc[src], Zc, dst, n_cand, src, flists, keep_src=True))
    assert np.array_equal(res["n_gt"], r_gt) and np.array_equal(res["n_eq"], r_eq)
    # and the unfiltered counts of the same queries are no smaller
    _, gt0, eq0 = run(dev, Xq, Zc, dst, n_cand, src)
    assert (gt0 >= got_gt).all() and (eq0 >= got_eq).all() and (gt0 + eq0 > got_gt + got_eq).any()


# ------------------------------------------------------------------------------------------------ 3. real-valued rows
def band_check(S, t, C, tau, got_gt, got_eq, cap=None):
    """Rule 3: exact counts for the unambiguous queries, the two-sided bound for the others.  Returns the ambiguous share."""
    amb = ((np.abs(S - t[:, None]) <= tau) & C).any(1)
    share = amb.mean()
    print("ambiguous share: %.4f (%d of %d queries)" % (share, amb.sum(), amb.size))
    if cap is not None:
        assert share <= cap, share                                             # from the oracle alone
    want_gt, want_eq = exact_counts(S, t, C)
    ok = ~amb
    assert np.array_equal(got_gt[ok], want_gt[ok]) and np.array_equal(got_eq[ok], want_eq[ok])
    lo = ((S > t[:, None] + tau) & C).sum(1)
    hi = ((S >= t[:, None] - tau) & C).sum(1)
    assert (lo <= got_gt).all() and (got_gt + got_eq <= hi).all()
    return share


def fp32_band(Xq, Zc, dst, n_cand):
    """tau(q, w) = gamma_d |x_q| (|z_w| + |z_dst|), gamma_d = d u / (1 - d u), u = 2^-24, norms in fp64."""
    d = Xq.shape[1]
    gamma = d * 2.0 ** -24 / (1 - d * 2.0 ** -24)
    nx = np.linalg.norm(Xq.astype(np.float64), axis=1)
    nz = np.linalg.norm(Zc.astype(np.float64), axis=1)
    return gamma * nx[:, None] * (nz[None, :n_cand] + nz[dst][:, None])


@pytest.mark.parametrize("N,d,Q", [(777, 96, 200), (389, 256, 257), (300, 36, 129), (2049, 64, 130)])
def test_real_valued_rows_inside_the_fp32_band(dev, N, d, Q):
    rng = np.random.RandomState(0)
    Z = rng.randn(N, d)
    Z = (Z / np.linalg.norm(Z, axis=1, keepdims=True)).astype(np.float32)
    src = rng.randint(0, N, size=Q)
    dst = rng.randint(0, N, size=Q)
    Xq = Z[src]
    S, t, C = oracle(Xq, Z, dst, N, src)
    tau = fp32_band(Xq, Z, dst, N)
    got_t, got_gt, got_eq = run(dev, Xq, Z, dst, N, src)
    band_check(S, t, C, tau, got_gt, got_eq, cap=0.15)
    assert (np.abs(got_t - t) <= tau.max(1)).all()


# ------------------------------------------------------------------------------------------------ 4. the reference's own runs
REF = ["unsup_mean", "unsup_gcn", "unsup_mean_tail", "unsup_maxpool", "unsup_skipgram", "unsup_xent_bilinear",
       "unsup_hinge_bilinear"]


@pytest.mark.parametrize("step", [0, 1])
@pytest.mark.parametrize("name", REF)
def test_counts_equal_the_reference_ranks(dev, name, step):
    fx = Fixture(name)
    p = "s%d/32/" % step
    out1, out2, neg = (fx[p + k].astype(np.float32) for k in ("outputs1", "outputs2", "neg_outputs"))
    B, n_neg = out1.shape[0], neg.shape[0]
    Xq = out1
    assert fx.cfg.get("bilinear_weights", False) == name.endswith("_bilinear")
    if name.endswith("_bilinear"):
        W = fx[("init/" if step == 0 else "s0/32/after/") + "edge_predict/weights"].astype(np.float32)
        Xq = (out1.astype(np.float64) @ W.astype(np.float64)).astype(np.float32)
    else:
        assert not fx.has("init/edge_predict/weights")
    Zc = np.concatenate([neg, out2], axis=0)
    dst = n_neg + np.arange(B)
    if Zc.shape[1] % 4:
        pytest.fail("the fixture's embedding width %d is no multiple of 4" % Zc.shape[1])
    got_t, got_gt, got_eq = run(dev, Xq, Zc, dst, n_neg)
    assert np.array_equal(got_gt + got_eq, fx[p + "ranks"][:, -1].astype(np.int64))
    S, t, C = oracle(Xq, Zc, dst, n_neg)
    assert np.abs(S - t[:, None]).min() > 10 * fp32_band(Xq, Zc, dst, n_neg).max()        # no case is ambiguous
    assert C.all()


# ------------------------------------------------------------------------------------------------ 5. model level
def synthetic_model(dev, aggregator_type, bilinear):
    from graphsage_amd import inits
    from graphsage_amd.models import Placeholder, SAGEInfo, SampleAndAggregate
    from graphsage_amd.neigh_samplers import AdjInfo, PaddedAdjacency, UniformNeighborSampler
    rng = np.random.RandomState(3)
    N, F, max_degree = 300, 50, 10
    feats = np.concatenate([rng.randn(N, F), np.zeros((1, F))]).astype(np.float32)
    a, b = rng.randint(0, N, size=1500), rng.randint(0, N, size=1500)
    a, b = np.concatenate([a, b]), np.concatenate([b, a])
    a[:40], b[:40] = 7, np.arange(40)                                            # a denser row; nodes 290.. stay isolated
    keep = (a < 290) & (b < 290)
    a, b = a[keep], b[keep]
    order = np.argsort(a, kind="stable")
    rowptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(a, minlength=N), out=rowptr[1:])
    graph = FullGraph.from_csr(rowptr, b[order], N)
    adj = np.full((N + 1, max_degree), N, dtype=np.int32)
    for v, nb in enumerate(graph.lists()[:N]):
        adj[v] = rng.choice(nb, size=max_degree, replace=True)
    eng.reset_engine()
    inits.set_seed(1)
    e = eng.get_engine()
    ph = {'batch1': Placeholder('batch1'), 'batch2': Placeholder('batch2'), 'neg_samples': Placeholder('neg'),
          'dropout': Placeholder('dropout', 0.), 'batch_size': Placeholder('batch_size')}
    adj_info = AdjInfo(PaddedAdjacency(adj, e.device))
    sampler = UniformNeighborSampler(adj_info)
    layer_infos = [SAGEInfo("node", sampler, 5, 32), SAGEInfo("node", sampler, 4, 32)]
    deg = np.diff(rowptr)
    model = SampleAndAggregate(ph, feats, adj_info, deg, layer_infos, concat=True, aggregator_type=aggregator_type,
                               learning_rate=0.01, weight_decay=0.0, neg_sample_size=5, bilinear_weights=bilinear)
    edges = np.stack([rng.randint(0, N, size=150), rng.randint(0, N, size=150)], axis=1)
    edges[:3] = [[7, 8], [7, 7], [295, 7]]
    return model, graph, edges


@pytest.mark.parametrize("bilinear", [False, True])
def test_model_rank_full_equals_the_oracle_on_embed_full(dev, bilinear):
    """Rule 3 with its cap of 15 % ambiguous queries, filtered and unfiltered.  Measured ambiguous shares on this graph: mean
    1.3 % (2 of 150 queries) both ways; bilinear, whose band also covers the fp32 query rows Z[src] . A, 4.7 % (7 of 150)."""
    model, graph, edges = synthetic_model(dev, "mean", bilinear)
    N = graph.n_nodes
    emb = model.embed_full(graph)
    assert emb.shape == (N, 64) and emb.dtype == np.float32
    src, dst = edges[:, 0], edges[:, 1]
    X64 = emb.astype(np.float64)[src]
    extra = 0.0
    if bilinear:
        W = model.link_pred_layer.vars['weights'].value.numpy().astype(np.float64)
        # the device forms the query rows Z[src] . A in fp32: |dx| <= (gamma_d + u) |z_src|^T |A| per entry, hence a score error
        # of at most that vector against |z_w| (and |z_dst| for t) on top of the dot product's own band
        d = emb.shape[1]
        gamma = d * 2.0 ** -24 / (1 - d * 2.0 ** -24)
        dx = (gamma + 2.0 ** -24) * (np.abs(X64) @ np.abs(W))
        az = np.abs(emb.astype(np.float64))
        extra = dx @ az.T + np.einsum("qd,qd->q", dx, az[dst])[:, None]
        X64 = X64 @ W
    Z64 = emb.astype(np.float64)
    S = X64 @ Z64.T
    t = np.einsum("qd,qd->q", X64, Z64[dst])
    gamma = 64 * 2.0 ** -24 / (1 - 64 * 2.0 ** -24)
    nz = np.linalg.norm(Z64, axis=1)
    tau = gamma * np.linalg.norm(X64, axis=1)[:, None] * (nz[None, :] + nz[dst][:, None]) + extra
    flists = [np.unique(f) for f in graph.lists()]
    res = model.rank_full(graph, edges)
    band_check(S, t, candidates(len(edges), N, dst, src, flists), tau, res["n_gt"], res["n_eq"], cap=0.15)
    assert np.array_equal(res["ranks"], 1 + res["n_gt"] + res["n_eq"])
    assert np.array_equal(res["ranks_optimistic"], 1 + res["n_gt"])
    assert res["mrr"] == pytest.approx(np.mean(1.0 / res["ranks"])) and sorted(res["hits"]) == [1, 10, 50, 100]
    assert (np.abs(res["scores"] - t) <= tau.max(1)).all()
    plain = model.rank_full(graph, edges, filtered=False)
    band_check(S, t, candidates(len(edges), N, dst, src), tau, plain["n_gt"], plain["n_eq"], cap=0.15)
    assert (plain["n_gt"] >= res["n_gt"]).all() and (plain["n_eq"] >= res["n_eq"]).all()
    assert (plain["n_gt"] + plain["n_eq"] > res["n_gt"] + res["n_eq"]).any()
    again = model.rank_full(graph, edges)
    for k in ("n_gt", "n_eq", "ranks", "scores"):
        assert np.array_equal(res[k], again[k]), k


# ------------------------------------------------------------------------------------------------ driver
def test_unsupervised_driver_rank_full(dev, tmp_path, capsys, monkeypatch):
    """--rank_full prints and writes the ranking of every held-out edge in both directions; the numbers are those of a direct
    model.rank_full call, and without the flag nothing of it appears."""
    import os
    import re
    from graphsage_amd import unsupervised_train as ut
    kept = {}
    real = ut.save_full_ranking

    def spy(model, minibatch, out_dir):
        kept["res"] = real(model, minibatch, out_dir)
        kept["n_val"] = len(minibatch.val_edges)

    monkeypatch.setattr(ut, "save_full_ranking", spy)
    eng.reset_engine()
    args = ["--synthetic", "small", "--epochs", "1", "--batch_size", "128", "--samples_1", "5", "--samples_2", "3", "--dim_1", "32",
            "--dim_2", "32", "--max_total_steps", "6", "--model", "graphsage_mean", "--learning_rate", "0.001",
            "--max_walk_pairs", "4000", "--validate_iter", "10", "--validate_batch_size", "256"]
    ut.main(args + ["--base_log_dir", str(tmp_path / "on"), "--rank_full"])
    out = capsys.readouterr().out
    pat = (r"Full-graph link ranking: mrr= (\d\.\d{5}) hits@1= (\d\.\d{5}) hits@10= (\d\.\d{5}) hits@50= (\d\.\d{5}) "
           r"hits@100= (\d\.\d{5}) edges= (\d+)")
    m = re.search(pat, out)
    assert m, out[-2000:]
    files = {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path / "on")) for f in fs}
    assert open(files["rank_full.txt"]).read() == m.group(0) + "\n" and "val.npy" in files
    res = kept["res"]
    assert int(m.group(6)) == 2 * kept["n_val"] == len(res["ranks"]) and kept["n_val"] > 0
    assert float(m.group(1)) == pytest.approx(res["mrr"], abs=1e-5) and 0 < res["mrr"] <= 1
    assert [float(m.group(i)) for i in (2, 3, 4, 5)] == [pytest.approx(res["hits"][k], abs=1e-5) for k in (1, 10, 50, 100)]
    assert res["hits"][1] <= res["hits"][10] <= res["hits"][50] <= res["hits"][100]
    monkeypatch.setattr(ut, "save_full_ranking", real)
    eng.reset_engine()
    ut.main(args + ["--base_log_dir", str(tmp_path / "off")])
    assert "Full-graph link ranking" not in capsys.readouterr().out
    assert not any(f == "rank_full.txt" for _, _, fs in os.walk(str(tmp_path / "off")) for f in fs)
