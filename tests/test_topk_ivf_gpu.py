"""-m gpu: the inverted-file scan (gs_ivf_search), retrieval.IVFIndex / build_ivf, model.topk_ivf and the driver's --topk_ivf.

1. exact against the fp64 oracle of ivf_oracle.py on a lattice (integer entries in [-3, 3], centres too: every dot product is
   exact in fp32 in any order, ties are plentiful) at every edge of the 128-row tiling of the lists AND of the pairs;
2. all lists probed == gs_topk_select by bits, on real-valued rows; 3. the filter's edge cases; 4. separated blobs: nprobe = 1
   is exact; 5. the binding's query chunks and repeatability; 6. build_ivf, save / load; 7. model.topk_ivf and the driver."""
import numpy as np
import pytest

import ivf_oracle
from graphsage_amd import engine as eng
from graphsage_amd import ops
from graphsage_amd.inference import RankFilter
from topk_oracle import candidates, scores64

pytestmark = pytest.mark.gpu
BM = BN = 128            # the kernel's tile (csrc/gs_rank_dev.h): 128 pairs x 128 list members


def up(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def lattice(rng, rows, d):
    return rng.randint(-3, 4, size=(rows, d)).astype(np.float32)


def make_index(Z, centers, labels, n_cand=None):
    from graphsage_amd.retrieval import IVFIndex
    eng.reset_engine()
    return IVFIndex.from_labels(eng.get_engine(), Z, centers, labels, n_cand=n_cand)


def run(dev, index, Xq, k, nprobe, src=None, filt=None, keep_src=False, chunk=ops.RANK_CHUNK):
    """ops.ivf_search on host queries (or a Mat already on the device) -> NumPy (ids, scores, count, scanned)."""
    import torch
    Xm = Xq if isinstance(Xq, ops.Mat) else ops.Mat.from_numpy(Xq, dev)
    f_rowptr, f_col = filt.on(dev, index.Z.rows) if filt is not None else (None, None)
    out = ops.ivf_search(Xm, index.Z, index.centers_dev, index.list_ptr, index.list_ids, k, nprobe, n_cand=index.n_cand,
                         src=None if src is None else up(dev, src), f_rowptr=f_rowptr, f_col=f_col, keep_src=keep_src, chunk=chunk)
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in out)


def assert_exact(got, want, tag=""):
    """ids, scores, count (and scanned, where the oracle gives it) equal the oracle's exactly, padding included."""
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].dtype == np.int32 and got[3].dtype == np.int64, tag
    assert np.array_equal(got[2], want[2]), tag
    assert np.array_equal(got[0], want[0]), tag
    assert np.array_equal(got[1].astype(np.float64), want[1]), tag
    if len(want) > 3:
        assert np.array_equal(got[3], want[3]), tag


# ------------------------------------------------------------------------------------------------ 1. exact, on a lattice
LENGTHS = {0: 1, 1: BN - 1, 2: 0, 3: BN, 4: BN + 1, 5: 300}        # old cluster id -> members; 2 is dropped


@pytest.mark.parametrize("d", [4, 36, 256])
def test_lattice_exact_at_every_list_pair_and_k_edge(dev, d):
    rng = np.random.RandomState(d)
    n_cand = sum(LENGTHS.values())
    n_rows = n_cand + 37
    labels = rng.permutation(np.repeat(list(LENGTHS), list(LENGTHS.values())))          # every list spans the id space
    Z, centers = lattice(rng, n_rows, d), lattice(rng, len(LENGTHS), d)
    lone = int(np.flatnonzero(labels == 0)[0])                                           # the one member of list 0
    dups = [int(np.flatnonzero(labels == c)[0]) for c in (1, 3, 4, 5)]
    Z[dups] = Z[dups[0]]                                                                 # bit-duplicate rows in four different lists
    x0 = lattice(rng, 1, d)[0]
    centers[0] = np.where(x0 >= 0, 3, -3)                  # <x0, c_0> = 3 |x0|_1 is the largest a centre can reach: x0 probes list 0 first
    index = make_index(Z, centers, labels, n_cand)
    assert index.n_clusters == 5 and index.empty == 1 and sorted(index.sizes.tolist()) == sorted(v for v in LENGTHS.values() if v)
    lp, li = index.list_ptr.cpu().numpy(), index.list_ids.cpu().numpy()
    assert lp.dtype == np.int64 and li.dtype == np.int32 and np.array_equal(np.diff(lp), index.sizes)
    for j in range(index.n_clusters):
        assert np.array_equal(li[lp[j]:lp[j + 1]], np.flatnonzero(index.labels == j))                 # ascending row id
    seen_empty = seen_short = False
    pairs_seen = set()
    for Q in (1, BM - 1, BM, BM + 1):
        for with_src in (False, True):
            # without src: random query rows.  with src: EVERY query row is x0, so each probed list is probed by exactly Q pairs
            # (1, 127, 128, 129: one tile of pairs, a full one, a full one and one more), and only src tells the queries apart
            Xq = np.repeat(x0[None], Q, axis=0) if with_src else lattice(rng, Q, d)
            src = None
            if with_src:
                src = rng.randint(0, n_rows, size=Q)
                src[0] = lone                                                  # nprobe = 1: nothing is left for this query
            S = scores64(Xq, Z, n_cand)
            assert np.abs(S).max() <= 9 * d and np.array_equal(S, S.astype(np.float32))            # exact in fp32
            Sc = Xq.astype(np.float64) @ index.centers.astype(np.float64).T
            assert np.array_equal(Sc, Sc.astype(np.float32))
            C = candidates(Q, n_cand, src)
            Xm = ops.Mat.from_numpy(Xq, dev)
            for nprobe in (1, 3, index.n_clusters):
                P = ivf_oracle.probe(Xq, index.centers, nprobe)
                if with_src:
                    assert (P == P[0]).all() and P[0, 0] == 0
                    pairs_seen.add(Q)
                for k in (1, 10, 128):
                    tag = "Q=%d d=%d k=%d nprobe=%d src=%s" % (Q, d, k, nprobe, with_src)
                    want = ivf_oracle.search(S, C, Xq, index.centers, index.labels, k, nprobe)
                    got = run(dev, index, Xm, k, nprobe, src)
                    assert_exact(got, want, tag)
                    ids, scores, count, _ = got
                    seen_empty |= bool((count == 0).any())
                    seen_short |= bool(((count > 0) & (count < k)).any())
                    if nprobe == index.n_clusters:
                        for q in range(min(Q, 3)):                             # the duplicates: ascending ids, equal scores
                            pos = [int(np.flatnonzero(ids[q] == w)[0]) for w in sorted(dups) if (ids[q] == w).any()]
                            assert pos == sorted(pos) and len(set(scores[q, pos].tolist())) <= 1, tag
    assert seen_empty and seen_short and pairs_seen == {1, BM - 1, BM, BM + 1}


# ------------------------------------------------------------------------------------------------ 2. all lists == exhaustive
@pytest.mark.parametrize("d", [36, 256])
def test_all_lists_probed_equals_the_exhaustive_kernel_by_bits(dev, d):
    """No tolerance: the same fmaf chain per (query, row), the same key, the same merge."""
    import torch
    rng = np.random.RandomState(100 + d)
    N, n_cand, Cn, Q, k = 1100, 1093, 7, 300, 20
    Z = rng.randn(N, d)
    Z = (Z / np.linalg.norm(Z, axis=1, keepdims=True)).astype(np.float32)
    labels = rng.randint(0, Cn, size=n_cand)
    index = make_index(Z, rng.randn(Cn, d).astype(np.float32), labels, n_cand)
    assert index.n_clusters == Cn
    flists = [np.sort(rng.choice(N, size=rng.randint(0, 30), replace=False)) for _ in range(N)]
    rowptr = np.zeros(N + 1, np.int64)
    np.cumsum([len(f) for f in flists], out=rowptr[1:])
    filt = RankFilter.from_csr(rowptr, np.concatenate(flists), N)
    src = rng.randint(0, N, size=Q)
    Xm = ops.Mat.from_numpy(Z[src], dev)
    f_rowptr, f_col = filt.on(dev, N)
    for kw in (dict(), dict(src=src), dict(src=src, filt=filt), dict(src=src, filt=filt, keep_src=True)):
        got = run(dev, index, Xm, k, Cn, **kw)
        has_f = "filt" in kw
        ids, scores, count = ops.topk_select(Xm, index.Z, k, n_cand=n_cand, src=up(dev, src) if "src" in kw else None,
                                             f_rowptr=f_rowptr if has_f else None, f_col=f_col if has_f else None,
                                             keep_src=kw.get("keep_src", False))
        torch.cuda.synchronize()
        assert np.array_equal(got[0], ids.cpu().numpy()), kw.keys()
        assert np.array_equal(got[1].view(np.int32), scores.cpu().numpy().view(np.int32)), kw.keys()
        assert np.array_equal(got[2], count.cpu().numpy()) and (got[2] == k).all() and (got[3] == n_cand).all()
    # the filter took something out, so the comparison above saw it work
    plain, filtered = run(dev, index, Xm, k, Cn, src=src), run(dev, index, Xm, k, Cn, src=src, filt=filt)
    assert not np.array_equal(plain[0], filtered[0])


# ------------------------------------------------------------------------------------------------ 3. filter edges
def test_filter_edges_on_the_lattice(dev):
    """The filter rows of test_topk_full_gpu.test_filter_edges_on_the_lattice; lists of about 200 rows spread over the ids."""
    rng = np.random.RandomState(5)
    n_rows, n_cand, d, Q, k, Cn = 1100, 1031, 36, BM + 2, 40, 5
    SLICE = 4 * BN
    Zc, Xq = lattice(rng, n_rows, d), lattice(rng, Q, d)
    flists = [np.sort(rng.choice(n_rows, size=rng.randint(0, 40), replace=False)) for _ in range(n_rows)]
    flists[0] = np.zeros(0, np.int64)                                          # an empty row
    flists[1] = np.arange(n_cand)                                              # a hub: every candidate
    flists[2] = np.concatenate([np.arange(BN - 8, BN + 8), np.arange(SLICE - 7, SLICE + 9)])
    flists[3] = np.asarray([0, SLICE - 1, SLICE, 2 * SLICE - 1, 2 * SLICE, n_cand - 1])
    flists[4] = np.asarray([7, 300, 900, 1050])
    flists[5] = np.asarray([5, 6, BN, n_cand, n_rows - 1])                     # lists its own query node, entries at and beyond n_cand
    flists[6] = np.arange(0, n_rows, 2)                                        # two queries share it
    flists[8] = np.arange(n_rows)                                              # a hub beyond n_cand too
    src = rng.randint(9, n_rows, size=Q)
    src[:10] = [0, 1, 2, 3, 4, 5, 6, 6, 8, 1]
    src[Q - 1], src[BM - 1], src[BM] = 3, 2, 1                                 # the same rows in the second tile of pairs
    rowptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum([len(f) for f in flists], out=rowptr[1:])
    filt = RankFilter.from_csr(rowptr, np.concatenate(flists), n_rows)
    index = make_index(Zc, lattice(rng, Cn, d), rng.randint(0, Cn, size=n_cand), n_cand)
    S = scores64(Xq, Zc, n_cand)
    for nprobe in (2, Cn):
        got = run(dev, index, Xq, k, nprobe, src, filt)
        assert_exact(got, ivf_oracle.search(S, candidates(Q, n_cand, src, flists), Xq, index.centers, index.labels, k, nprobe), nprobe)
        for q in (1, 8, 9, BM):
            assert got[2][q] == 0 and (got[0][q] == -1).all() and np.isneginf(got[1][q]).all()   # hubs: nothing left
        kept = run(dev, index, Xq, k, nprobe, src, filt, keep_src=True)
        assert_exact(kept, ivf_oracle.search(S, candidates(Q, n_cand, src, flists, keep_src=True), Xq, index.centers, index.labels,
                                             k, nprobe), nprobe)
    assert not np.array_equal(kept[0], got[0])


# ------------------------------------------------------------------------------------------------ 4. separated blobs
def test_separated_blobs_are_exact_with_one_probe(dev):
    """Rows 32 e_b + noise in {-1, 0, 1}^36, 5 blobs of 150: a same-blob score is at least 31^2 - 35 = 926, a cross-blob score at
    most 33 + 33 + 34 = 100, the own centre scores at least 992 against at most 32 -- one probe finds every true partner."""
    from graphsage_amd import inference as inf
    from graphsage_amd.retrieval import recall
    rng = np.random.RandomState(4)
    B, per, d, k = 5, 150, 36, 20
    blob = np.repeat(np.arange(B), per)
    Z = rng.randint(-1, 2, size=(B * per, d)).astype(np.float32)
    Z[np.arange(B * per), blob] += 32
    perm = rng.permutation(B * per)
    Z, blob = Z[perm], blob[perm]
    centers = 32 * np.eye(B, d, dtype=np.float32)
    index = make_index(Z, centers, blob)
    nodes = np.arange(B * per)
    res = index.search(nodes, k, 1)
    exact = inf.topk_full(eng.get_engine(), index.Z, nodes, k)
    assert np.array_equal(res["ids"], exact["ids"]) and np.array_equal(res["count"], exact["count"]) and (res["count"] == k).all()
    assert np.array_equal(res["scores"].view(np.int32), exact["scores"].view(np.int32))
    assert (res["scores"] >= 926).all() and (blob[res["ids"]] == blob[:, None]).all()
    assert recall(res["ids"], exact["ids"]) == 1.0
    assert res["scanned"].dtype == np.int64 and (res["scanned"] == per).all()


# ------------------------------------------------------------------------------------------------ 5. chunks, repeatability
def test_binding_chunks_and_repeatability(dev):
    rng = np.random.RandomState(13)
    n_cand, d, Q, k, Cn = 700, 36, 3 * 64 + 9, 10, 6
    Z = rng.randn(n_cand + 1, d).astype(np.float32)
    index = make_index(Z, rng.randn(Cn, d).astype(np.float32), rng.randint(0, Cn, size=n_cand), n_cand)
    src = rng.randint(0, n_cand, size=Q)
    Xm = ops.Mat.from_numpy(Z[src], dev)
    whole = run(dev, index, Xm, k, 3, src)
    for chunk in (64, 200):                                                    # 4 calls (the last of 9 queries); 2 calls
        parts = run(dev, index, Xm, k, 3, src, chunk=chunk)
        for a, b in zip(whole, parts):
            assert a.tobytes() == b.tobytes(), chunk
    again = run(dev, index, Xm, k, 3, src)
    for a, b in zip(whole, again):
        assert a.tobytes() == b.tobytes()
    assert (whole[2] == k).all() and len(set(map(tuple, whole[0]))) > 10


# ------------------------------------------------------------------------------------------------ 6. build_ivf, save / load
def test_build_ivf_and_save_load(dev, tmp_path):
    from graphsage_amd import inference as inf
    from graphsage_amd.retrieval import IVFIndex, build_ivf
    rng = np.random.RandomState(6)
    N, d, k, Cn = 1100, 36, 10, 9
    means = rng.randn(Cn, d)
    Z = means[rng.randint(0, Cn, size=N + 1)] + 0.3 * rng.randn(N + 1, d)
    Z = (Z / np.linalg.norm(Z, axis=1, keepdims=True)).astype(np.float32)
    eng.reset_engine()
    e = eng.get_engine()
    Zm = ops.Mat.from_numpy(Z, dev)
    index = build_ivf(e, Zm, Cn, n_cand=N, seed=7)                             # the last row of Z plays the pad row
    C2 = index.n_clusters
    assert C2 + index.empty == Cn and index.n_cand == N
    lp, li = index.list_ptr.cpu().numpy(), index.list_ids.cpu().numpy()
    assert np.array_equal(np.sort(li), np.arange(N)) and lp[0] == 0 and lp[-1] == N and (np.diff(lp) > 0).all()
    fit = index.clustering
    kept = np.flatnonzero(np.bincount(fit.labels, minlength=Cn) > 0)
    assert len(kept) == C2 and np.array_equal(kept[index.labels], fit.labels) and np.array_equal(index.centers, fit.centers[kept])
    for j in range(C2):
        assert np.array_equal(li[lp[j]:lp[j + 1]], np.flatnonzero(fit.labels == kept[j]))
    nodes = rng.randint(0, N, size=260)
    flists = [np.sort(rng.choice(N, size=rng.randint(0, 20), replace=False)) for _ in range(N + 1)]
    rowptr = np.zeros(N + 2, np.int64)
    np.cumsum([len(f) for f in flists], out=rowptr[1:])
    filt = RankFilter.from_csr(rowptr, np.concatenate(flists), N + 1)
    full = index.search(nodes, k, C2, filt=filt)
    exact = inf.topk_full(e, Zm, nodes, k, n_cand=N, filt=filt)
    for key in ("ids", "scores", "count"):
        assert full[key].tobytes() == exact[key].tobytes(), key
    assert (full["scanned"] == N).all() and (full["ids"] < N).all()            # never the pad row
    from graphsage_amd._lib import GraphsageAmdError
    with pytest.raises(GraphsageAmdError, match="nprobe"):
        index.search(nodes, k, C2 + 1)
    few = index.search(nodes, k, 2, filt=filt)
    assert (few["scanned"] < N).all() and (few["scores"] <= exact["scores"]).all()
    index.save(str(tmp_path))
    c, l = np.load(str(tmp_path / "ivf_centers.npy")), np.load(str(tmp_path / "ivf_labels.npy"))
    assert c.dtype == np.float32 and c.shape == (C2, d) and l.dtype == np.int32 and l.shape == (N,)
    loaded = IVFIndex.load(e, Zm, str(tmp_path))
    assert loaded.empty == 0 and np.array_equal(loaded.list_ids.cpu().numpy(), li) and np.array_equal(loaded.list_ptr.cpu().numpy(), lp)
    again = loaded.search(nodes, k, 2, filt=filt)
    for key in ("ids", "scores", "count", "scanned"):
        assert few[key].tobytes() == again[key].tobytes(), key


# ------------------------------------------------------------------------------------------------ 7. model and driver
@pytest.mark.parametrize("bilinear", [False, True])
def test_model_topk_ivf(dev, bilinear):
    from test_rank_full_gpu import synthetic_model
    model, graph, edges = synthetic_model(dev, "mean", bilinear)
    N, k = graph.n_nodes, 10
    first = model.topk_ivf(graph, k=k, nprobe=1, n_clusters=6)
    index = first["index"]
    assert index.n_cand == N and index.Z.rows == N + 1 and first["ids"].shape == (N, k)
    res = model.topk_ivf(graph, k=k, nprobe=index.n_clusters, index=index)
    exact = model.topk_full(graph, k=k)
    for key in ("ids", "scores", "count"):
        assert res[key].tobytes() == exact[key].tobytes(), key
    assert (res["scanned"] == N).all() and (first["scanned"] < N).all() and (first["ids"] < N).all()
    lists = graph.lists()
    assert not any(np.isin(first["ids"][u], lists[u]).any() for u in range(N))                    # never a graph neighbor
    assert (first["ids"] != np.arange(N)[:, None]).all()                                          # never the query itself
    plain = model.topk_ivf(graph, nodes=[7, 295, 7], k=k, nprobe=index.n_clusters, filtered=False, index=index)
    want = model.topk_full(graph, nodes=[7, 295, 7], k=k, filtered=False)
    assert np.array_equal(plain["ids"], want["ids"]) and np.array_equal(plain["ids"][0], plain["ids"][2])


def test_unsupervised_driver_topk_ivf(dev, tmp_path, capsys):
    """--topk_ivf K writes the four files and one line that parses; with every list probed the recall of the sample is 1 and
    the arrays are those of --topk_full."""
    import os
    import re
    from graphsage_amd import unsupervised_train as ut
    eng.reset_engine()
    args = ["--synthetic", "small", "--epochs", "1", "--batch_size", "128", "--samples_1", "5", "--samples_2", "3", "--dim_1", "32",
            "--dim_2", "32", "--max_total_steps", "6", "--model", "graphsage_mean", "--learning_rate", "0.001",
            "--max_walk_pairs", "4000", "--validate_iter", "10", "--validate_batch_size", "256"]
    ut.main(args + ["--base_log_dir", str(tmp_path / "on"), "--topk_ivf", "5", "--topk_ivf_clusters", "4", "--topk_ivf_nprobe", "1"])
    out = capsys.readouterr().out
    pat = (r"IVF top-K partners: k= (\d+) nodes= (\d+) clusters= (\d+) empty= (\d+) nprobe= (\d+) list_min= (\d+) list_max= (\d+) "
           r"scanned= (\d\.\d{5}) filled= (\d\.\d{5}) recall@k= (nan|\d\.\d{5}) sample= (\d+) build_time= (\d+\.\d{5}) "
           r"search_time= (\d+\.\d{5})")
    m = re.search(pat, out)
    assert m, out[-2000:]
    files = {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path / "on")) for f in fs}
    ids, scores = np.load(files["topk_ivf.npy"]), np.load(files["topk_ivf_scores.npy"])
    centers, labels = np.load(files["ivf_centers.npy"]), np.load(files["ivf_labels.npy"])
    N = ids.shape[0]
    assert ids.shape == (N, 5) and ids.dtype == np.int32 and scores.shape == (N, 5) and scores.dtype == np.float32
    C2 = int(m.group(3))
    assert centers.shape == (C2, 64) and centers.dtype == np.float32 and labels.shape == (N,) and labels.dtype == np.int32
    assert (int(m.group(1)), int(m.group(2)), int(m.group(5))) == (5, N, 1) and C2 + int(m.group(4)) == 4
    sizes = np.bincount(labels, minlength=C2)
    assert (int(m.group(6)), int(m.group(7))) == (sizes.min(), sizes.max()) and sizes.min() > 0
    assert 0 < float(m.group(8)) < 1 and (m.group(10), m.group(11)) == ("nan", "0")
    assert float(m.group(9)) == pytest.approx(np.mean(ids >= 0), abs=1e-5) and float(m.group(9)) > 0
    assert open(files["topk_ivf.txt"]).read().strip() == m.group(0)
    eng.reset_engine()
    ut.main(args + ["--base_log_dir", str(tmp_path / "all"), "--topk_ivf", "5", "--topk_ivf_clusters", "4", "--topk_ivf_nprobe",
                    str(C2), "--topk_ivf_recall", "50", "--topk_full", "5"])
    out = capsys.readouterr().out
    m = re.search(pat, out)
    assert m and (m.group(10), m.group(11)) == ("1.00000", "50") and float(m.group(8)) == 1.0, out[-2000:]
    assert out.index("Full-graph top-K partners") < out.index("IVF top-K partners")
    files = {f: os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path / "all")) for f in fs}
    assert np.array_equal(np.load(files["topk_ivf.npy"]), np.load(files["topk_full.npy"]))
    assert np.load(files["topk_ivf_scores.npy"]).tobytes() == np.load(files["topk_full_scores.npy"]).tobytes()
