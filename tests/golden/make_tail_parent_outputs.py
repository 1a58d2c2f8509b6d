"""Recorder of the fused tail launches (gs_tail.hip, gs_unsup_tail.hip: gs_sage_tail_fwd_bwd, gs_sage_tail_z, gs_sage_tail_dh0,
gs_linkpred_tail, gs_linkpred_tail_neg) at small seeded shapes.

    GS_LIB=<library of the commit to pin> python tests/golden/make_tail_parent_outputs.py     # on the GPU

writes tests/golden/tail_parent_outputs.npz.  The inputs are not stored: `run(name, dev)` rebuilds them from the case's seed and
returns every buffer the case's launches write.  tests/test_tail_golden_gpu.py recomputes every case with the in-tree library and
compares as float values, with no tolerance.

The file in the tree was recorded with the library of commit fc44b47 ("Gather+mean: edge-shape parity stand-alone and riding in
every launch") -- the last commit in which the five tail kernels each carried their own copy of the relu-mask, input-gradient,
d_h0-store, l2-normalise and z-helper bodies.  Regenerate it only when the kernels' arithmetic is meant to change, and say so in
the commit.

Stored per output `<case>.<output>` (`index`, JSON): the array itself when it has at most 8 KB (a slice of `whole`); else the
SHA-256 of its bytes with -0 folded to +0, so that equal float VALUES hash alike (a row of `sha256`).  means, z and d_h0 also
carry their float64 column sums (a slice of `colsum`), read only for the failure message: they name the columns that moved.  The
other large outputs (y, dz, neg_slabs, 128-class logits / preds / dlogits) carry the hash alone: with their sums the file does not
fit the 113 KB it is held to (130 KB; an .npz entry of its own per value, 195 KB).  An output whose bytes equal those of an output
stored earlier is a `same_as` entry naming that one (the split form, the means_ready form and the stand-alone z launch give the
bits of the fused launch).

Cases:
  the thirteen tail hosts of tests/test_gather_edges_gpu.py (HOSTS, imported), launched with no jobs: n = 20 (a ragged second
  group), two main workgroups per group and one, two class groups, eval, split, means_ready, both link-prediction launches;
  sup_*: gs_sage_tail_fwd_bwd (train), gs_sage_tail_z and gs_sage_tail_dh0 on the same operands, one case per (d_in, out_dim):
    sup_s11   n 17, s 11 = TAIL_NB, 128 -> 128, 128 sigmoid classes (two class groups)
    sup_s1    n 5, s 1, 256 -> 64, one softmax class
    sup_gcn   n 17, s 3, 256 -> 128, 41 classes, the gcn form (W_neigh = W_self + out_dim), fused and split (gs_sage_tail_z gcn);
              gs_sage_tail_dh0 has no gcn form and takes the two column halves as W_self / W_neigh
    sup_zero  n 17, s 2, 128 -> 64, 7 classes, the self and neighbor rows of batch rows 3 and 16 all zero: z = 0 there, the
              clamped branch of l2-normalise forward and backward
  lp_*: gs_linkpred_tail + gs_linkpred_tail_neg, training (lp_b9 also forward only):
    lp_b9     B 9, 17 negatives, s 2, 128 -> 64: second pair group and second negative group ragged; pair row 2 and negative 1 zero
    lp_b3     B 3, 3 negatives, s 1, 256 -> 128: only the scalar remainder loop of the affinities
    lp_b8     B 8, 32 negatives = LP_MAX_NEG, s 11, 128 -> 128
    lp_b16    B 16, 6 negatives, s 3, 256 -> 64: one four-wide pass and two remainders
After every case the hand-over error word (tail_sync_error / lp_tail_sync_error) is 0."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, "tail_parent_outputs.npz")
WHOLE_BYTES = 8 * 1024
COLSUM_OUTPUTS = ("means", "z", "d_h0")                   # of the sup_* / lp_* cases; the edge hosts return unnamed buffers:
COLSUM_EDGE = tuple("%s.out%d" % (h, i) for h, ids in (("tail_train_D256", (0, 1, 7)), ("tail_train_D128", (0, 1, 7)), ("tail_train_C65", (0, 1, 7)),
                                                       ("tail_z", (0, 1)), ("tail_dh0", (0,)), ("lp_tail", (0, 1, 4))) for i in ids)

EDGE_HOSTS = ("tail_train_D256", "tail_train_D128", "tail_eval", "tail_train_C65", "tail_split", "tail_means", "tail_z", "tail_z_means",
              "tail_dh0", "lp_tail", "lp_tail_means", "lp_neg_train", "lp_neg_eval")
# name: (seed, n, s, d_in, out_dim, C, sigmoid, gcn, batch rows that are zero)
SUP = {
    "sup_s11": (31, 17, 11, 128, 128, 128, True, False, ()),
    "sup_s1": (32, 5, 1, 256, 64, 1, False, False, ()),
    "sup_gcn": (33, 17, 3, 256, 128, 41, False, True, ()),
    "sup_zero": (34, 17, 2, 128, 64, 7, False, False, (3, 16)),
}
# name: (seed, B, n_neg, s, d_in, out_dim, rows that are zero, also forward only)
LP = {
    "lp_b9": (51, 9, 17, 2, 128, 64, (2, 2 * 9 + 1), True),
    "lp_b3": (52, 3, 3, 1, 256, 128, (), False),
    "lp_b8": (53, 8, 32, 11, 128, 128, (), False),
    "lp_b16": (54, 16, 6, 3, 256, 64, (), False),
}
CASES = EDGE_HOSTS + tuple(SUP) + tuple(LP)


def _edges():
    tests = os.path.dirname(HERE)
    for p in (tests, os.path.dirname(tests)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import test_gather_edges_gpu as edges
    return edges


def _h0(E, rng, n, s, D, zero_rows):
    h0n = E._relu_h0(rng, n + n * s, D)
    for r in zero_rows:
        h0n[r] = 0
        h0n[n + r * s:n + (r + 1) * s] = 0
    return h0n


def _run_edge(name, dev):
    import torch
    outs, launch, after = _edges().HOSTS[name][0](dev)()
    launch([])
    torch.cuda.synchronize()
    if after is not None:
        after()                                           # (the error word is 0, z and d_h0 are not all zero)
    return {"out%d" % i: t.cpu().numpy() for i, t in enumerate(outs)}


def _run_sup(name, dev):
    import torch
    E = _edges()
    from graphsage_amd import ops
    from graphsage_amd.ops import Mat
    seed, n, s, D, O, C, sig, gcn, zero_rows = SUP[name]
    rng = np.random.default_rng(seed)
    rows, Z = n + n * s, 2 * O
    h0 = Mat.from_numpy(_h0(E, rng, n, s, D, zero_rows), dev)
    if gcn:
        W = Mat.from_numpy(E._asym(rng, (D, Z), 0.2), dev)
        Ws, Wn = W.cols_slice(0, O), W.cols_slice(O, Z)
    else:
        Ws, Wn = Mat.from_numpy(E._asym(rng, (D, O), 0.2), dev), Mat.from_numpy(E._asym(rng, (D, O), 0.2), dev)
    Wh, bh = Mat.from_numpy(E._asym(rng, (Z, C), 0.3), dev), E._dev(E._asym(rng, (C,), 0.1), dev)
    labn = (rng.random((n, C)) > 0.5).astype(np.float32) if sig else np.eye(C, dtype=np.float32)[rng.integers(0, C, n)]
    lab = Mat.from_numpy(labn, dev)
    dz_in = Mat.from_numpy(E._asym(rng, (n, Z)), dev)
    assert ops.sage_tail_supported(D, O, C)
    res = {}
    for form in ("fused", "split") if gcn else ("fused",):
        means, z, y = Mat.zeros(n, D, dev), Mat.zeros(n, Z, dev), Mat.zeros(n, Z, dev)
        lo, pr, dl = Mat.zeros(n, C, dev), Mat.zeros(n, C, dev), Mat.zeros(n, C, dev)
        lr, dz, dh0 = torch.zeros(n, device=dev), Mat.zeros(n, Z, dev), Mat.zeros(rows, D, dev)
        sync = torch.zeros(ops.tail_sync_words(n, O), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ops.sage_tail_fwd_bwd(h0, n, s, Ws, Wn, O, Wh, bh, lab, C, sig, means, z, y, lo, pr, dl, lr, dz=dz, d_h0=dh0,
                              split=form == "split", sync=sync, gcn=gcn)
        torch.cuda.synchronize()
        assert form == "split" or ops.tail_sync_error(sync, n) == 0
        for k, m in (("means", means), ("z", z), ("y", y), ("logits", lo), ("preds", pr), ("dlogits", dl), ("dz", dz), ("d_h0", dh0)):
            res["%s.%s" % (form, k)] = m.buf.cpu().numpy()
        res["%s.loss_rows" % form] = lr.cpu().numpy()
    means, z, dh0 = Mat.zeros(n, D, dev), Mat.zeros(n, Z, dev), Mat.zeros(rows, D, dev)
    ops.sage_tail_z(h0, n, s, Ws, Wn, O, means, z, gcn=gcn)
    ops.sage_tail_dh0(h0, n, s, Ws, Wn, O, dz_in, dh0)
    torch.cuda.synchronize()
    res.update({"tail_z.means": means.buf.cpu().numpy(), "tail_z.z": z.buf.cpu().numpy(), "tail_dh0.d_h0": dh0.buf.cpu().numpy()})
    return res


def _run_lp(name, dev):
    import torch
    E = _edges()
    from graphsage_amd import ops
    from graphsage_amd.ops import Mat
    seed, B, nn, s, D, O, zero_rows, also_eval = LP[name]
    rng = np.random.default_rng(seed)
    n = 2 * B + nn
    rows, Z = n + n * s, 2 * O
    h0 = Mat.from_numpy(_h0(E, rng, n, s, D, zero_rows), dev)
    Ws, Wn = Mat.from_numpy(E._asym(rng, (D, O), 0.2), dev), Mat.from_numpy(E._asym(rng, (D, O), 0.2), dev)
    assert ops.linkpred_tail_supported(D, O, nn)
    res = {}
    for train in (True, False) if also_eval else (True,):
        means, z, y, dz, dh0 = Mat.zeros(n, D, dev), Mat.zeros(n, Z, dev), Mat.zeros(n, Z, dev), Mat.zeros(n, Z, dev), Mat.zeros(rows, D, dev)
        lr, rr, aff = torch.zeros(B, device=dev), torch.zeros(B, device=dev), Mat.zeros(B, nn + 1, dev)
        slabs = torch.zeros(((B + 7) // 8) * nn, Z, device=dev)
        loss, mrr = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        sync = torch.zeros(ops.lp_tail_sync_words(B, nn), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        desc = ops.linkpred_tail_desc(h0, B, nn, s, Ws, Wn, O, means, z, y, lr, rr, aff, 1.0, 1.0 / B, sync, dz=dz if train else None,
                                      d_h0=dh0 if train else None, neg_slabs=slabs if train else None)
        ops.linkpred_tail(desc)
        ops.linkpred_tail_neg(desc, loss_out=loss, accumulate=False, mrr_out=mrr)
        torch.cuda.synchronize()
        assert ops.lp_tail_sync_error(sync, B, nn) == 0
        form = "train" if train else "eval"
        outs = [("means", means.buf), ("z", z.buf), ("y", y.buf), ("aff", aff.buf), ("loss_rows", lr), ("rr_rows", rr), ("loss", loss), ("mrr", mrr)]
        if train:
            outs += [("dz", dz.buf), ("d_h0", dh0.buf), ("neg_slabs", slabs)]
        for k, t in outs:
            res["%s.%s" % (form, k)] = t.cpu().numpy()
    return res


def run(name, dev):
    """The case through the loaded library -> {output name: array}: every buffer its launches write, pad columns included."""
    return (_run_sup if name in SUP else _run_lp if name in LP else _run_edge)(name, dev)


def fold(a):
    """The array's bytes with -0 folded to +0."""
    return np.where(a == 0, np.zeros((), a.dtype), a).tobytes()


def digest(a):
    return np.frombuffer(hashlib.sha256(fold(a)).digest(), dtype=np.uint8)


def colsum(a):
    return np.atleast_1d(a.astype(np.float64).sum(axis=0))


def has_colsum(key):
    return key.rsplit(".", 1)[-1] in COLSUM_OUTPUTS or key in COLSUM_EDGE


def load(path=GOLDEN_FILE):
    """{`<case>.<output>`: ("whole", array) | ("sha256", 32 bytes, column sums or None)}, `same_as` entries resolved."""
    with np.load(path) as z:
        index, whole, sha, sums = json.loads(str(z["index"])), z["whole"], z["sha256"], z["colsum"]
    doc = {}
    for key, e in index.items():
        if e[0] == "whole":
            doc[key] = ("whole", whole[e[1]:e[1] + int(np.prod(e[2]))].reshape(e[2]))
        elif e[0] == "sha256":
            doc[key] = ("sha256", sha[e[1]], sums[e[2]:e[2] + e[3]] if e[3] else None)
    for key, e in index.items():
        if e[0] == "same_as":
            doc[key] = doc[e[1]]
    return doc


def main():
    import torch
    dev = torch.device("cuda")
    index, seen, whole, sha, sums = {}, {}, [], [], []
    for name in CASES:
        for key, a in run(name, dev).items():
            a = np.ascontiguousarray(a)
            assert a.dtype == np.float32 and np.isfinite(a).all(), (name, key)
            full = "%s.%s" % (name, key)
            ident = (a.shape, fold(a))
            if ident in seen:
                index[full] = ["same_as", seen[ident]]
            elif a.nbytes <= WHOLE_BYTES:
                index[full] = ["whole", sum(w.size for w in whole), list(a.shape)]
                whole.append(a.reshape(-1))
            else:
                cs = colsum(a) if has_colsum(full) else np.zeros(0)
                index[full] = ["sha256", len(sha), sum(c.size for c in sums), int(cs.size)]
                sha.append(digest(a))
                sums.append(cs)
            seen.setdefault(ident, full)
        print("%-16s recorded" % name, flush=True)
    target = os.environ.get("TAIL_GOLDEN_OUT", GOLDEN_FILE)
    np.savez_compressed(target, index=np.array(json.dumps(index)), whole=np.concatenate(whole), sha256=np.stack(sha),
                        colsum=np.concatenate(sums))
    print("wrote %s (%d bytes, %d outputs)" % (target, os.path.getsize(target), len(index)))


if __name__ == "__main__":
    main()
