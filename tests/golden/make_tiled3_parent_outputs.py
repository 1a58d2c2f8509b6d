"""Recorder of the layer-0 tiled forward's outputs (gs_sage_dense_fwd_tiled3 / _means) at small seeded shapes.

    GS_LIB=<library of the commit to pin> python tests/golden/make_tiled3_parent_outputs.py     # on the GPU

writes tests/golden/tiled3_parent_outputs.npz: per case the output matrix (and the layer-1 means of the _means case).  The inputs
are not stored: `inputs(case)` rebuilds them from the case's seed.  tests/test_tiled3_lean_golden_gpu.py recomputes every case with
the in-tree library and compares as float values.  The file in the tree was recorded with the library of the commit BEFORE the K
loop of sage_tiled3_fwd_kernel was split into a steady ring and careful stages (which also stopped running the all-zero stages
that padded the loop to whole rings of four: K = 17, 100, 160 and 208 had two, one, two and three of them); regenerate it only
when the kernel's arithmetic is meant to change, and say so in the commit.

Shapes: K = 17 (two stages, one valid k in the last), 64 (four whole stages), 100 (7 stages), 113 (8 stages, one valid k in the
last), 160 (10 whole stages: the smallest ring remainder 2 behind a steady ring), 208 (13 stages); one and two terms, gathered and
dense self rows, out = 8 and 128, one to three row tiles."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, "tiled3_parent_outputs.npz")
N_TABLE = 300

# name: (seed, K, n, out, two terms, gathered self rows, bias, relu, (n_roots, s) of the _means entry or None)
CASES = {
    "k17_n1": (1, 17, 1, 8, True, True, True, False, None),
    "k64_n130": (2, 64, 130, 8, True, True, False, True, None),
    "k100_n65": (3, 100, 65, 128, True, True, True, True, None),
    "k113_n65": (4, 113, 65, 8, False, False, True, False, None),
    "k160_n130": (5, 160, 130, 8, True, False, False, True, None),
    "k208_n65": (6, 208, 65, 128, False, False, True, True, None),
    "k100_means": (7, 100, 77, 128, True, True, False, True, (7, 10)),
}


def inputs(name):
    """The operands of a case as NumPy arrays: table X [N_TABLE, K], self ids [n] (the last table row among them), dense self rows
    / neighbor means [n, K], weights [K, out] x 2, bias [terms * out] or None."""
    seed, K, n, out, two, gathered, bias, relu, means = CASES[name]
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N_TABLE, K)).astype(np.float32)
    ids = rng.integers(0, N_TABLE, size=n).astype(np.int32)
    ids[n // 2] = N_TABLE - 1
    self_m = X[ids] if gathered else rng.normal(size=(n, K)).astype(np.float32)
    mean = rng.normal(size=(n, K)).astype(np.float32)
    Ws = (rng.normal(size=(K, out)) * 0.1).astype(np.float32)
    Wn = (rng.normal(size=(K, out)) * 0.1).astype(np.float32)
    b = (rng.normal(size=((2 if two else 1) * out,)) * 0.1).astype(np.float32) if bias else None
    return X, ids, self_m, mean, Ws, Wn, b


def run(name, dev):
    """The case through the loaded library -> {"out": [n, terms * out]} (+ {"means": [n_roots, 2 out]})."""
    import torch
    from graphsage_amd import ops
    from graphsage_amd.ops import Mat
    seed, K, n, out, two, gathered, bias, relu, means = CASES[name]
    X, ids, self_m, mean, Ws, Wn, b = inputs(name)
    Xd, sd, md = Mat.from_numpy(X, dev, 32), Mat.from_numpy(self_m, dev, 32), Mat.from_numpy(mean, dev, 4)
    for mat in (Xd, sd, md):
        if mat.ld > K:
            mat.buf[:, K:] = float("nan")
    Wsd, Wnd = Mat.from_numpy(Ws, dev), Mat.from_numpy(Wn, dev)
    bd = torch.from_numpy(b).to(dev) if bias else None
    ids_d = torch.from_numpy(ids).to(dev)
    act = ops.ACT_RELU if relu else ops.ACT_IDENTITY
    outm = Mat.zeros(n, (2 if two else 1) * out, dev)
    outm.buf.fill_(float("nan"))
    res = {}
    if means:
        n_roots, s = means
        assert n == n_roots * (1 + s) and two
        l1 = Mat.zeros(n_roots, 2 * out, dev)
        l1.buf.fill_(float("nan"))
        ops.sage_dense_fwd_tiled3_means(Xd if gathered else sd, ids_d if gathered else None, md, n, Wsd, Wnd, out, act, bd, outm,
                                        n_roots, s, l1, [])
        torch.cuda.synchronize()
        res["means"] = l1.numpy()
    elif two:
        ops.sage_dense_fwd_tiled3(Xd if gathered else sd, ids_d if gathered else None, md, n, Wsd, Wnd, out, act, bd, outm, [])
    else:
        ops.sage_dense_fwd_tiled3(None, None, md, n, None, Wnd, out, act, bd, outm, [])
    torch.cuda.synchronize()
    res["out"] = outm.numpy()
    return res


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import torch
    dev = torch.device("cuda")
    doc = {}
    for name in CASES:
        for key, a in run(name, dev).items():
            assert np.isfinite(a).all(), (name, key)
            doc["%s.%s" % (name, key)] = a
        print("%-12s recorded" % name, flush=True)
    target = os.environ.get("TILED3_GOLDEN_OUT", GOLDEN_FILE)
    np.savez_compressed(target, **doc)
    print("wrote %s (%d bytes)" % (target, os.path.getsize(target)))


if __name__ == "__main__":
    main()
