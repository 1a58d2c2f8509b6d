"""Recorder of the five 128 x 128 fp32-MFMA score sweeps (gs_rank_count, gs_topk_select, gs_ivf_search, gs_kmeans_assign,
gs_linkpred_infonce_fwd_bwd) at small seeded shapes with REAL-VALUED inputs.

    GS_LIB=<library of the commit to pin> python tests/golden/make_sweep_parent_outputs.py     # on the GPU

writes tests/golden/sweep_parent_outputs.npz.  The inputs are not stored: `run(name, dev)` rebuilds them from the case's seed and
returns every buffer the case's launches write.  tests/test_sweep_golden_gpu.py recomputes every case with the in-tree library and
compares with no tolerance.  The lattice inputs of the kernels' own suites are exact under any order of additions; these are not,
so a changed k order of the tile pipeline (csrc/gs_rank_dev.h) moves bits here.

The file in the tree was recorded with the library of commit 54ac9ec ("Add the in-batch softmax (InfoNCE) link-prediction loss")
-- the last commit in which the five kernel files each carried their own copy of the K loop.  Regenerate it only when the
kernels' arithmetic is meant to change, and say so in the commit.

Stored per output `<case>.<output>` (`index`, JSON): the array itself when it has at most 8 KB (a slice of the byte buffer
`whole`); else the SHA-256 of its bytes, floats with -0 folded to +0 (a row of `sha256`).

Cases (every d reaches another branch of the K loop: 4 one partial stage, 36 a second, partial stage, 64 exactly two stages, 96
an odd stage count -- the next tile starts on the other buffer --, 256 four passes):
  rank_* / topk_*   Q = 129 (a second query tile with one row) against 300 candidates (a ragged last tile), or against 520 (five
                    candidate tiles: rank_plan gives two slices, the second with one tile -- asserted from the workspace size);
                    with and without src, a filter and GS_RANK_KEEP_SRC; candidate rows 7 and 200 bit-identical; k = 1, 64, 65, 128
  ivf_*             Q = 130, five lists of 0, 1, 128, 129 and 300 members over a 558-row table, nprobe 1 and 5 (every cluster then
                    has 130 pairs: two work items), with and without a filter
  km_*              n = 130 through a `rows` gather, k = 1, 129 and 300, with and without xsq, prev and dist
  nce_*             training at (B, n_neg, d) = (130, 5, 64), (1030, 3, 64) (nine row and nine candidate tiles: by nce_plan both
                    gradient sweeps are cut in five and their slabs summed -- asserted from the workspace size) and (9, 0, 128);
                    forward only at (130, 5, 256)"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, "sweep_parent_outputs.npz")
WHOLE_BYTES = 8 * 1024
TWIN = (7, 200)                                           # candidate rows with the same bits

# name: (seed, Q, n_cand, d, src, filter, keep_src)
RANK = {
    "rank_d4": (101, 129, 300, 4, False, False, False),
    "rank_d36": (102, 129, 300, 36, True, True, False),
    "rank_d64": (103, 129, 300, 64, True, True, True),
    "rank_d96": (104, 129, 520, 96, True, True, False),
    "rank_d256": (105, 129, 300, 256, True, False, False),
}
# name: (seed, Q, n_cand, d, k, src, filter, keep_src)
TOPK = {
    "topk_d4_k1": (111, 129, 300, 4, 1, False, False, False),
    "topk_d36_k64": (112, 129, 300, 36, 64, True, True, False),
    "topk_d64_k65": (113, 129, 300, 64, 65, True, True, True),
    "topk_d96_k128": (114, 129, 520, 96, 128, True, False, False),
    "topk_d256_k64": (115, 129, 520, 256, 64, True, True, False),
}
IVF_LISTS = (0, 1, 128, 129, 300)
# name: (seed, d, k, nprobe, filter)
IVF = {
    "ivf_d36_p1": (121, 36, 10, 1, False),
    "ivf_d64_p1_f": (122, 64, 65, 1, True),
    "ivf_d4_p5": (123, 4, 10, 5, False),
    "ivf_d96_p5_f": (124, 96, 65, 5, True),
    "ivf_d256_p5": (125, 256, 128, 5, False),
}
# name: (seed, d, k, xsq, prev, dist)
KM = {
    "km_d4_k1": (131, 4, 1, False, False, False),
    "km_d36_k129": (132, 36, 129, True, True, True),
    "km_d64_k129": (133, 64, 129, True, False, True),
    "km_d96_k300": (134, 96, 300, True, True, True),
    "km_d256_k300": (135, 256, 300, False, False, False),
}
# name: (seed, B, n_neg, d, train, ids)
NCE = {
    "nce_b130": (141, 130, 5, 64, True, True),
    "nce_b1030": (142, 1030, 3, 64, True, False),
    "nce_b9": (143, 9, 0, 128, True, False),
    "nce_b130_fwd": (144, 130, 5, 256, False, True),
}
CASES = tuple(RANK) + tuple(TOPK) + tuple(IVF) + tuple(KM) + tuple(NCE)


def _root():
    root = os.path.dirname(os.path.dirname(HERE))
    if root not in sys.path:
        sys.path.insert(0, root)


def _table(rng, n, d):
    z = rng.standard_normal((n, d)).astype(np.float32)
    z[TWIN[1] % n] = z[TWIN[0] % n]
    return z


def _filter(rng, n_rows, dev):
    """A CSR filter over the table's rows: sorted, distinct columns; row 0 empty, row 1 long."""
    import torch
    lens = rng.integers(0, 9, n_rows)
    lens[0], lens[1] = 0, min(n_rows, 140)
    cols = [np.sort(rng.choice(n_rows, int(m), replace=False)) for m in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = (np.concatenate(cols) if rowptr[-1] else np.zeros(0)).astype(np.int32)
    return torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev)


def _query(rng, Q, n, d, src, filt, dev):
    import torch
    from graphsage_amd.ops import Mat
    Xq, Zc = Mat.from_numpy(rng.standard_normal((Q, d)), dev), Mat.from_numpy(_table(rng, n, d), dev)
    s = rng.integers(0, n, Q).astype(np.int32)
    s[:2] = (0, 1)                                        # the empty and the long filter row
    s = torch.from_numpy(s).to(dev) if src else None
    fr, fc = _filter(rng, n, dev) if filt else (None, None)
    return Xq, Zc, s, fr, fc


def _run_rank(name, dev):
    import torch
    from graphsage_amd import ops
    seed, Q, n, d, src, filt, keep = RANK[name]
    rng = np.random.default_rng(seed)
    Xq, Zc, s, fr, fc = _query(rng, Q, n, d, src, filt, dev)
    dst = rng.integers(0, n, Q).astype(np.int32)
    dst[:4] = (TWIN[0], TWIN[1], TWIN[0], n - 1)          # the twin rows tie with their own targets
    if n == 520:
        assert ops.rank_ws_bytes(Q, n) == 2 * Q * 2 * 4   # two slices (four tiles and one)
    t, n_gt, n_eq = ops.rank_count(Xq, Zc, torch.from_numpy(dst).to(dev), src=s, f_rowptr=fr, f_col=fc, keep_src=keep,
                                   stream=ops.current_stream())
    torch.cuda.synchronize()
    return {"t": t.cpu().numpy(), "n_gt": n_gt.cpu().numpy(), "n_eq": n_eq.cpu().numpy()}


def _run_topk(name, dev):
    import torch
    from graphsage_amd import ops
    seed, Q, n, d, k, src, filt, keep = TOPK[name]
    rng = np.random.default_rng(seed)
    Xq, Zc, s, fr, fc = _query(rng, Q, n, d, src, filt, dev)
    if n == 520:
        assert ops.topk_ws_bytes(Q, n, k) == 2 * Q * (64 * (1 + -(-k // 64)) * 8 + 4)      # two slices
    ids, scores, count = ops.topk_select(Xq, Zc, k, src=s, f_rowptr=fr, f_col=fc, keep_src=keep, stream=ops.current_stream())
    torch.cuda.synchronize()
    return {"ids": ids.cpu().numpy(), "scores": scores.cpu().numpy(), "count": count.cpu().numpy()}


def _run_ivf(name, dev):
    import torch
    from graphsage_amd import ops
    from graphsage_amd.ops import Mat
    seed, d, k, nprobe, filt = IVF[name]
    rng = np.random.default_rng(seed)
    Q, n = 130, sum(IVF_LISTS)
    Xq, Zc, s, fr, fc = _query(rng, Q, n, d, True, filt, dev)
    centers = Mat.from_numpy(rng.standard_normal((len(IVF_LISTS), d)), dev)
    perm = rng.permutation(n)
    ptr = np.concatenate([[0], np.cumsum(IVF_LISTS)]).astype(np.int64)
    lists = np.concatenate([np.sort(perm[ptr[j]:ptr[j + 1]]) for j in range(len(IVF_LISTS))]).astype(np.int32)
    ids, scores, count, scanned = ops.ivf_search(Xq, Zc, centers, torch.from_numpy(ptr).to(dev), torch.from_numpy(lists).to(dev), k, nprobe,
                                                 src=s, f_rowptr=fr, f_col=fc, stream=ops.current_stream())
    torch.cuda.synchronize()
    return {"ids": ids.cpu().numpy(), "scores": scores.cpu().numpy(), "count": count.cpu().numpy(), "scanned": scanned.cpu().numpy()}


def _run_km(name, dev):
    import torch
    from graphsage_amd import ops
    from graphsage_amd.ops import Mat
    seed, d, k, with_xsq, with_prev, with_dist = KM[name]
    rng = np.random.default_rng(seed)
    n, n_rows = 130, 211
    X, C = Mat.from_numpy(rng.standard_normal((n_rows, d)), dev), Mat.from_numpy(_table(rng, k, d), dev)
    rows = torch.from_numpy(rng.integers(0, n_rows, n).astype(np.int32)).to(dev)
    st = ops.current_stream()
    csq = ops.kmeans_sqnorm(C, stream=st)
    xsq = ops.kmeans_sqnorm(X, rows=rows, stream=st) if with_xsq else None
    prev = torch.from_numpy(rng.integers(0, k, n).astype(np.int32)).to(dev) if with_prev else None
    dist = torch.zeros(n, dtype=torch.float32, device=dev) if with_dist else None
    assign, dist, stats = ops.kmeans_assign(X, C, csq, rows=rows, xsq=xsq, prev=prev, dist=dist, stream=st)
    torch.cuda.synchronize()
    res = {"assign": assign.cpu().numpy(), "stats": stats.cpu().numpy()}
    if with_dist:
        res["dist"] = dist.cpu().numpy()
    return res


def _run_nce(name, dev):
    import torch
    from graphsage_amd import ops
    from graphsage_amd.ops import Mat
    seed, B, nn, d, train, with_ids = NCE[name]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2 * B + nn, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    X = Mat.from_numpy(x, dev)
    U = X.rows_slice(0, B)
    ids = None
    if with_ids:                                          # few distinct nodes: some candidates are masked
        ids = tuple(torch.from_numpy(rng.integers(0, 40, B).astype(np.int32)).to(dev) for _ in range(2))
    floats = ops.linkpred_infonce_ws_floats(B, d, nn, train)
    if B == 1030:                                         # nine tiles either way: five cuts of two tiles, slabs of dU and dC
        assert floats - ops.linkpred_infonce_ws_floats(B, d, nn, False) == 5 * B * d + 5 * (B + nn) * d
    ws = torch.zeros(floats, device=dev)
    loss_rows, rr, aff = torch.zeros(B, device=dev), torch.zeros(B, device=dev), Mat.zeros(B, nn + 1, dev)
    dX, dU = (Mat.zeros(2 * B + nn, d, dev), Mat.zeros(B, d, dev)) if train else (None, None)
    torch.cuda.synchronize()
    ops.linkpred_infonce_fwd_bwd(X, U, B, nn, 0.2, 1.0 / B, loss_rows, rr, aff, ws, dX=dX, dU=dU, ids=ids, stream=ops.current_stream())
    torch.cuda.synchronize()
    res = {"loss_rows": loss_rows.cpu().numpy(), "rr_rows": rr.cpu().numpy(), "aff_all": aff.buf.cpu().numpy(),
           "stats": ws[:2 * B].cpu().numpy()}
    if train:
        res.update({"dX": dX.buf.cpu().numpy(), "dU": dU.buf.cpu().numpy()})
    return res


def run(name, dev):
    """The case through the loaded library -> {output name: array}: every buffer its launches write."""
    _root()
    for table, fn in ((RANK, _run_rank), (TOPK, _run_topk), (IVF, _run_ivf), (KM, _run_km), (NCE, _run_nce)):
        if name in table:
            return fn(name, dev)
    raise KeyError(name)


def fold(a):
    """The array's bytes, a float array's -0 folded to +0."""
    a = np.ascontiguousarray(a)
    return (np.where(a == 0, np.zeros((), a.dtype), a) if a.dtype.kind == "f" else a).tobytes()


def digest(a):
    return np.frombuffer(hashlib.sha256(fold(a)).digest(), dtype=np.uint8)


def load(path=GOLDEN_FILE):
    """{`<case>.<output>`: ("whole", array) | ("sha256", 32 bytes)}."""
    with np.load(path) as z:
        index, whole, sha = json.loads(str(z["index"])), z["whole"], z["sha256"]
    doc = {}
    for key, e in index.items():
        if e[0] == "whole":
            dt = np.dtype(e[3])
            n = int(np.prod(e[2])) * dt.itemsize
            doc[key] = ("whole", np.frombuffer(whole[e[1]:e[1] + n].tobytes(), dtype=dt).reshape(e[2]))
        else:
            doc[key] = ("sha256", sha[e[1]])
    return doc


def main():
    import torch
    dev = torch.device("cuda")
    index, whole, sha, at = {}, [], [], 0
    for name in CASES:
        for key, a in run(name, dev).items():
            a = np.ascontiguousarray(a)
            assert a.dtype.kind in "fi" and not np.isnan(a).any(), (name, key)
            full = "%s.%s" % (name, key)
            if a.nbytes <= WHOLE_BYTES:
                index[full] = ["whole", at, list(a.shape), a.dtype.str]
                whole.append(np.frombuffer(fold(a), dtype=np.uint8))
                at += a.nbytes
            else:
                index[full] = ["sha256", len(sha)]
                sha.append(digest(a))
        print("%-16s recorded" % name, flush=True)
    target = os.environ.get("SWEEP_GOLDEN_OUT", GOLDEN_FILE)
    np.savez_compressed(target, index=np.array(json.dumps(index)), whole=np.concatenate(whole), sha256=np.stack(sha))
    print("wrote %s (%d bytes, %d outputs)" % (target, os.path.getsize(target), len(index)))


if __name__ == "__main__":
    main()
