"""-m gpu: the fused score-and-select kernel (gs_topk_select) and topk_full against the fp64 NumPy oracle of topk_oracle.py.

1. exact on a lattice (integer entries in [-3, 3]: every dot product is exact in fp32 in any order, ties are plentiful) at every
   edge of the 128 x 128 tiling, of the slices of 4 tiles and of k against the candidate count, with bit-duplicate rows;
2. several query tiles and slices; 3. the filter's edge cases; 4. the binding's query chunks -- all exact;
5. bit-equality with the count kernel: t, n_gt of gs_rank_count for every returned (query, id);
6. real-valued rows against fp64 inside the derived fp32 dot-product band;
7. model.topk_full; 8. the driver's --topk_full; 9. argument checks."""
import numpy as np
import pytest

from graphsage_amd import engine as eng
from graphsage_amd import ops
from graphsage_amd._lib import GraphsageAmdError
from graphsage_amd.inference import RankFilter
from topk_oracle import candidates, scores64, select

pytestmark = pytest.mark.gpu
BM = BN = 128            # the kernel's tile (csrc/gs_rank_dev.h)
SLICE = 4 * BN           # candidates per slice while the query tiles are few (4 tiles per slice)


def up(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def run(dev, Xq, Zc, k, n_cand, src=None, filt=None, keep_src=False):
    """ops.topk_select on host arrays (or Mats already on the device) -> NumPy (ids, scores, count)."""
    import torch
    Xm = Xq if isinstance(Xq, ops.Mat) else ops.Mat.from_numpy(Xq, dev)
    Zm = Zc if isinstance(Zc, ops.Mat) else ops.Mat.from_numpy(Zc, dev)
    f_rowptr, f_col = filt.on(dev, Zm.rows) if filt is not None else (None, None)
    ids, scores, count = ops.topk_select(Xm, Zm, k, n_cand=n_cand, src=None if src is None else up(dev, src),
                                         f_rowptr=f_rowptr, f_col=f_col, keep_src=keep_src)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy()


def assert_exact(got, want, tag=""):
    """ids, scores and count equal the oracle's exactly, padding included (the scores are exact in fp32 on the lattice)."""
    (ids, scores, count), (w_ids, w_scores, w_count) = got, want
    assert ids.dtype == np.int32 and scores.dtype == np.float32 and count.dtype == np.int32, tag
    assert np.array_equal(count, w_count), tag
    assert np.array_equal(ids, w_ids), tag
    assert np.array_equal(scores.astype(np.float64), w_scores), tag


def lattice(rng, rows, d):
    return rng.randint(-3, 4, size=(rows, d)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. exact, on a lattice
@pytest.mark.parametrize("d", [4, 36, 256])
def test_lattice_exact_at_every_tile_slice_and_k_edge(dev, d):
    rng = np.random.RandomState(d)
    seen_empty = seen_short = False
    # 1031 candidates = 9 tiles = slices of 4, 4, 1 tiles (ragged last slice, three slices); 700 = a ragged second slice
    for Q in (1, BM - 1, BM, BM + 1):
        for n_cand in (1, BN - 1, BN, BN + 1, 700, 1031):
            for with_src in (False, True):
                n_rows = n_cand + 37 if with_src else n_cand                  # (the variant with src also has n_rows > n_cand)
                Zc, Xq = lattice(rng, n_rows, d), lattice(rng, Q, d)
                dups = [w for w in (0, 5, n_cand // 2, n_cand - 1) if w < n_cand]
                for w in dups:
                    Zc[w] = Zc[0]                                              # bit-duplicate candidate rows
                src = None
                if with_src:
                    src = rng.randint(0, n_rows, size=Q)
                    src[0] = 0                                                 # n_cand == 1: nothing is left for this query
                S = scores64(Xq, Zc, n_cand)
                assert np.abs(S).max() <= 9 * d and np.array_equal(S, S.astype(np.float32))        # exact in fp32
                C = candidates(Q, n_cand, src)
                Xm, Zm = ops.Mat.from_numpy(Xq, dev), ops.Mat.from_numpy(Zc, dev)
                for k in (1, 10, 128):
                    tag = "Q=%d n_cand=%d n_rows=%d d=%d k=%d" % (Q, n_cand, n_rows, d, k)
                    want = select(S, C, k)
                    got = run(dev, Xm, Zm, k, n_cand, src)
                    assert_exact(got, want, tag)
                    ids, scores, count = got
                    seen_empty |= bool((count == 0).any())
                    seen_short |= bool(((count > 0) & (count < k)).any())
                    for q in range(min(Q, 3)):                                 # the duplicates: ascending ids, equal scores
                        pos = [int(np.flatnonzero(ids[q] == w)[0]) for w in sorted(set(dups)) if (ids[q] == w).any()]
                        assert pos == sorted(pos) and len(set(scores[q, pos].tolist())) <= 1, tag
                        if k == 128 and n_cand <= 128 and src is None:
                            assert len(pos) == len(set(dups)), tag
    assert seen_empty and seen_short           # count == 0 (n_cand = 1, src == 0) and k beyond the candidate count were covered


# ------------------------------------------------------------------------------------------------ 2. several tiles and slices
def test_lattice_exact_with_several_query_tiles_and_slices(dev):
    """Three query tiles against seven slices, src given (excluded)."""
    rng = np.random.RandomState(11)
    Q, n_cand, n_rows, d, k = 2 * BM + 3, 7 * SLICE - 77, 7 * SLICE, 36, 50
    Zc, Xq = lattice(rng, n_rows, d), lattice(rng, Q, d)
    src = rng.randint(0, n_rows, size=Q)
    want = select(scores64(Xq, Zc, n_cand), candidates(Q, n_cand, src), k)
    assert_exact(run(dev, Xq, Zc, k, n_cand, src), want)
    w_scores = want[1]
    assert (w_scores[:, :-1] == w_scores[:, 1:]).any()                         # ties inside the lists: the id rule decides


# ------------------------------------------------------------------------------------------------ 3. filter edges
def test_filter_edges_on_the_lattice(dev):
    """The filter rows of test_rank_full_gpu.test_filter_edges_on_the_lattice, without a dst."""
    rng = np.random.RandomState(5)
    n_rows, n_cand, d, Q, k = 1100, 1031, 36, BM + 2, 40
    Zc, Xq = lattice(rng, n_rows, d), lattice(rng, Q, d)
    flists = [np.sort(rng.choice(n_rows, size=rng.randint(0, 40), replace=False)) for _ in range(n_rows)]
    flists[0] = np.zeros(0, np.int64)                                          # an empty row
    flists[1] = np.arange(n_cand)                                              # a hub: every candidate
    flists[2] = np.concatenate([np.arange(BN - 8, BN + 8), np.arange(SLICE - 7, SLICE + 9)])     # runs over a tile / slice edge
    flists[3] = np.asarray([0, SLICE - 1, SLICE, 2 * SLICE - 1, 2 * SLICE, n_cand - 1])         # first / last of every slice
    flists[4] = np.asarray([7, 300, 900, 1050])
    flists[5] = np.asarray([5, 6, BN, n_cand, n_rows - 1])                     # lists its own query node, entries beyond n_cand
    flists[6] = np.arange(0, n_rows, 2)                                        # two queries share it
    flists[8] = np.arange(n_rows)                                              # a hub beyond n_cand too
    src = rng.randint(9, n_rows, size=Q)
    src[:10] = [0, 1, 2, 3, 4, 5, 6, 6, 8, 1]
    src[Q - 1], src[BM - 1], src[BM] = 3, 2, 1                                 # the same rows in the second query tile
    order = [rng.permutation(len(f)) for f in flists]                          # handed over unsorted, with duplicates
    col = np.concatenate([np.concatenate([f[o], f[o][:3]]) for f, o in zip(flists, order)])
    rowptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum([len(f) + min(3, len(f)) for f in flists], out=rowptr[1:])
    filt = RankFilter.from_csr(rowptr, col, n_rows)
    assert all(np.array_equal(a, b) for a, b in zip(filt.lists(), flists))
    S = scores64(Xq, Zc, n_cand)
    got = run(dev, Xq, Zc, k, n_cand, src, filt)
    assert_exact(got, select(S, candidates(Q, n_cand, src, flists), k))
    for q in (1, 8, 9, BM):
        assert got[2][q] == 0 and (got[0][q] == -1).all() and np.isneginf(got[1][q]).all()       # hubs: nothing left
    # the query node kept as a candidate (it then only names its filter row), unless its own row lists it
    kept = run(dev, Xq, Zc, k, n_cand, src, filt, keep_src=True)
    assert_exact(kept, select(S, candidates(Q, n_cand, src, flists, keep_src=True), k))
    assert not np.array_equal(kept[0], got[0])
    # the same through inference.topk_full(exclude_self=False, filt=...): the two options are independent
    from graphsage_amd import inference as inf
    eng.reset_engine()
    res = inf.topk_full(eng.get_engine(), ops.Mat.from_numpy(Zc, dev), src, k, n_cand=n_cand, filt=filt, exclude_self=False)
    want = select(scores64(Zc[src], Zc, n_cand), candidates(Q, n_cand, src, flists, keep_src=True), k)
    assert_exact((res["ids"], res["scores"], res["count"]), want)
    own = [(res["ids"][q] == src[q]).any() for q in range(Q) if src[q] < n_cand and src[q] not in flists[src[q]]]
    assert any(own)                                                            # |z|^2 is a row's best score more often than not


# ------------------------------------------------------------------------------------------------ 4. query chunking
def test_lattice_exact_across_the_query_chunk_of_the_binding(dev):
    """More queries than one gs_topk_select call takes (ops.RANK_CHUNK): the second call's rows, src and outputs are offset."""
    rng = np.random.RandomState(13)
    Q, n_cand, n_rows, d, k = ops.RANK_CHUNK + BM + 2, 5, 9, 4, 3
    Zc, Xq = lattice(rng, n_rows, d), lattice(rng, Q, d)
    src = rng.randint(0, n_rows, size=Q)
    want = select(scores64(Xq, Zc, n_cand), candidates(Q, n_cand, src), k)
    got = run(dev, Xq, Zc, k, n_cand, src)
    assert_exact(got, want)
    tail = slice(ops.RANK_CHUNK, Q)
    assert np.array_equal(got[0][tail], want[0][tail]) and (want[0][tail] >= 0).all() and len(set(map(tuple, want[0][tail]))) > 10


# ------------------------------------------------------------------------------------------------ 5. / 6. real-valued rows
REAL = [(777, 96, 200), (389, 256, 257), (2049, 64, 130)]
_real = {}


def real_case(dev, N, d, Q, filtered):
    """Rows, queries, filter, the fp64 scores and the device result at k = 20: computed once, shared by tests 5 and 6."""
    key = (N, d, Q, filtered)
    if key not in _real:
        rng = np.random.RandomState(N + d)
        Z = rng.randn(N, d)
        Z = (Z / np.linalg.norm(Z, axis=1, keepdims=True)).astype(np.float32)
        src = rng.randint(0, N, size=Q)
        flists = filt = None
        if filtered:
            flists = [np.sort(rng.choice(N, size=rng.randint(0, 30), replace=False)) for _ in range(N)]
            rowptr = np.zeros(N + 1, np.int64)
            np.cumsum([len(f) for f in flists], out=rowptr[1:])
            filt = RankFilter.from_csr(rowptr, np.concatenate(flists), N)
        got = run(dev, Z[src], Z, 20, N, src, filt)
        _real[key] = dict(Z=Z, src=src, flists=flists, filt=filt, S=scores64(Z[src], Z, N),
                          C=candidates(Q, N, src, flists), got=tuple(a.copy() for a in got))
        for a in _real[key]["got"]:
            a.setflags(write=False)
    return _real[key]


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("N,d,Q", REAL)
def test_agreement_with_the_count_kernel(dev, N, d, Q, filtered):
    """No tolerance: for every returned (q, j), gs_rank_count with dst = ids[q, j] gives t bit-equal to scores[q, j] and n_gt
    equal to the number of strictly better entries before j."""
    import torch
    c = real_case(dev, N, d, Q, filtered)
    ids, scores, count = c["got"]
    k = ids.shape[1]
    assert (count == k).all() and (ids >= 0).all()
    # non-increasing along j, ids ascending inside runs of equal score
    assert (scores[:, :-1] >= scores[:, 1:]).all()
    assert (ids[:, :-1] < ids[:, 1:])[scores[:, :-1] == scores[:, 1:]].all()
    Xm, Zm, src_dev = ops.Mat.from_numpy(c["Z"][c["src"]], dev), ops.Mat.from_numpy(c["Z"], dev), up(dev, c["src"])
    f_rowptr, f_col = c["filt"].on(dev, N) if filtered else (None, None)
    for j in range(k):
        t, n_gt, n_eq = ops.rank_count(Xm, Zm, up(dev, ids[:, j]), n_cand=N, src=src_dev, f_rowptr=f_rowptr, f_col=f_col)
        torch.cuda.synchronize()
        t, n_gt = t.cpu().numpy(), n_gt.cpu().numpy()
        assert np.array_equal(t.view(np.uint32), scores[:, j].view(np.uint32)), j
        assert np.array_equal(n_gt, (scores[:, :j] > scores[:, j:j + 1]).sum(1)), j
        assert (n_gt <= j).all()


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("N,d,Q", REAL)
def test_real_valued_rows_against_fp64(dev, N, d, Q, filtered):
    """tau = gamma_d |x| |z| (gamma_d = d u / (1 - d u), u = 2^-24) bounds the error of ONE fp32 dot product; two scores are
    compared, hence 2 tau (the two-sided form of test_rank_full_gpu.fp32_band).  The bounds hold for every query."""
    c = real_case(dev, N, d, Q, filtered)
    ids, scores, count = c["got"]
    S, C = c["S"], c["C"]
    k = ids.shape[1]
    gamma = d * 2.0 ** -24 / (1 - d * 2.0 ** -24)
    nz = np.linalg.norm(c["Z"].astype(np.float64), axis=1)
    tau = gamma * nz[c["src"]] * nz.max()                                      # [Q]
    rows = np.arange(Q)[:, None]
    assert (np.abs(scores.astype(np.float64) - S[rows, ids]) <= tau[:, None]).all()
    assert C[rows, ids].all()                                                  # only candidates are returned
    kth = -np.sort(-np.where(C, S, -np.inf), axis=1)[:, k - 1]                 # the fp64 k-th best
    assert (S[rows, ids] >= (kth - 2 * tau)[:, None]).all()
    must = C & (S > (kth + 2 * tau)[:, None])
    got = np.zeros_like(C)
    got[rows, ids] = True
    assert (got | ~must).all() and must.any()


# ------------------------------------------------------------------------------------------------ 7. model level
@pytest.mark.parametrize("bilinear", [False, True])
def test_model_topk_full(dev, bilinear):
    from test_rank_full_gpu import synthetic_model
    model, graph, edges = synthetic_model(dev, "mean", bilinear)
    N, k = graph.n_nodes, 10
    res = model.topk_full(graph, k=k)
    ids, scores, count = res["ids"], res["scores"], res["count"]
    assert ids.shape == (N, k) and ids.dtype == np.int32 and scores.shape == (N, k) and scores.dtype == np.float32
    assert (count == k).all() and (count[290:] == k).all()                     # isolated nodes 290.. get lists too
    assert (ids >= 0).all() and (ids < N).all()                                # never the pad row
    assert (ids != np.arange(N)[:, None]).all()                                # never the query itself
    lists = graph.lists()
    assert not any(np.isin(ids[u], lists[u]).any() for u in range(N))          # never a graph neighbor
    plain = model.topk_full(graph, k=k, filtered=False)
    assert any(np.isin(plain["ids"][u], lists[u]).any() for u in range(N))
    # against rank_full on the same edges, unfiltered on both sides: exact, because the scores are bit-equal.  (An edge
    # (u, u) is left out: rank_full scores the query node as dst, topk_full never returns it.)
    rk = model.rank_full(graph, edges, filtered=False)
    checked = 0
    for (u, v), r, r_opt in zip(edges, rk["ranks"], rk["ranks_optimistic"]):
        if u == v:
            continue
        inside = bool((plain["ids"][u] == v).any())
        assert not (r <= k) or inside
        assert not inside or r_opt <= k
        checked += inside
    assert checked > 0
    some = model.topk_full(graph, nodes=[7, 295, 7], k=k)
    assert np.array_equal(some["ids"], ids[[7, 295, 7]]) and np.array_equal(some["scores"], scores[[7, 295, 7]])
    again = model.topk_full(graph, k=k)
    for key in ("ids", "scores", "count"):
        assert np.array_equal(res[key].view(np.int32), again[key].view(np.int32)), key


# ------------------------------------------------------------------------------------------------ 8. driver
def test_unsupervised_driver_topk_full(dev, tmp_path, capsys, monkeypatch):
    """--topk_full K prints one line and writes both arrays, equal to a direct model.topk_full call; without the flag nothing of
    it appears; the models without a full-neighborhood form are refused before training."""
    import os
    import re
    from graphsage_amd import unsupervised_train as ut
    kept = {}
    real = ut.save_full_topk

    def spy(model, minibatch, out_dir, k):
        real(model, minibatch, out_dir, k)
        from graphsage_amd.supervised_train import full_graph
        kept["res"] = model.topk_full(full_graph(minibatch, minibatch.G.n_nodes), k=k)
        kept["N"] = minibatch.G.n_nodes

    monkeypatch.setattr(ut, "save_full_topk", spy)
    eng.reset_engine()
    args = ["--synthetic", "small", "--epochs", "1", "--batch_size", "128", "--samples_1", "5", "--samples_2", "3", "--dim_1", "32",
            "--dim_2", "32", "--max_total_steps", "6", "--model", "graphsage_mean", "--learning_rate", "0.001",
            "--max_walk_pairs", "4000", "--validate_iter", "10", "--validate_batch_size", "256"]
    ut.main(args + ["--base_log_dir", str(tmp_path / "on"), "--topk_full", "5"])
    out = capsys.readouterr().out
    m = re.search(r"Full-graph top-K partners: k= (\d+) nodes= (\d+) filled= (\d\.\d{5})", out)
    assert m, out[-2000:]
    files = {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path / "on")) for f in fs}
    assert "val.npy" in files
    ids, scores = np.load(files["topk_full.npy"]), np.load(files["topk_full_scores.npy"])
    N = kept["N"]
    assert ids.shape == (N, 5) and ids.dtype == np.int32 and scores.shape == (N, 5) and scores.dtype == np.float32
    assert np.array_equal(ids, kept["res"]["ids"]) and np.array_equal(scores.view(np.int32), kept["res"]["scores"].view(np.int32))
    assert (int(m.group(1)), int(m.group(2))) == (5, N)
    assert float(m.group(3)) == pytest.approx(np.mean(ids >= 0), abs=1e-5) and float(m.group(3)) > 0
    monkeypatch.setattr(ut, "save_full_topk", real)
    eng.reset_engine()
    ut.main(args + ["--base_log_dir", str(tmp_path / "off")])
    assert "Full-graph top-K partners" not in capsys.readouterr().out
    assert not any(f.startswith("topk_full") for _, _, fs in os.walk(str(tmp_path / "off")) for f in fs)
    for model in ("n2v", "graphsage_seq"):
        with pytest.raises(SystemExit) as ei:
            ut.main(["--synthetic", "small", "--model", model, "--topk_full", "5"])
        assert "--topk_full" in str(ei.value) and model in str(ei.value)
        assert "Loading training data" not in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------ 9. argument checks
def test_bad_arguments_are_refused_before_any_launch(dev):
    import torch
    rng = np.random.RandomState(1)
    Zc, Xq = lattice(rng, 12, 8), lattice(rng, 5, 8)
    Xm, Zm = ops.Mat.from_numpy(Xq, dev), ops.Mat.from_numpy(Zc, dev)
    src = up(dev, np.arange(5))
    rowptr = torch.zeros(13, dtype=torch.int64, device=dev)
    col = torch.zeros(1, dtype=torch.int32, device=dev)
    out = dict(ids=torch.full((5, 3), 7, dtype=torch.int32, device=dev), scores=torch.full((5, 3), 7.0, device=dev),
               count=torch.full((5,), 7, dtype=torch.int32, device=dev))
    with pytest.raises(GraphsageAmdError, match="k="):
        ops.topk_select(Xm, Zm, 0)
    with pytest.raises(GraphsageAmdError, match="k="):
        ops.topk_select(Xm, Zm, ops.TOPK_MAX + 1)
    assert ops.TOPK_MAX == 128
    with pytest.raises(GraphsageAmdError, match="multiple of 4"):
        ops.topk_select(ops.Mat.from_numpy(Xq[:, :6], dev), ops.Mat.from_numpy(Zc[:, :6], dev), 3, **out)
    with pytest.raises(GraphsageAmdError, match="n_cand"):
        ops.topk_select(Xm, Zm, 3, n_cand=13, **out)
    with pytest.raises(GraphsageAmdError, match="src"):
        ops.topk_select(Xm, Zm, 3, f_rowptr=rowptr, f_col=col, **out)
    with pytest.raises(GraphsageAmdError, match="workspace"):
        ops.topk_select(Xm, Zm, 3, src=src, ws=torch.zeros(1, dtype=torch.int64, device=dev), **out)
    torch.cuda.synchronize()
    assert (out["ids"] == 7).all() and (out["scores"] == 7.0).all() and (out["count"] == 7).all()      # nothing was launched
    ids, scores, count = ops.topk_select(Xm, Zm, 3, src=src, **out)                                    # ... and the good call
    torch.cuda.synchronize()
    assert_exact((ids.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy()),
                 select(scores64(Xq, Zc, 12), candidates(5, 12, np.arange(5)), 3))
