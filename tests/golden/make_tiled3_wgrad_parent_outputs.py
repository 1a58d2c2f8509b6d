"""Recorder of the tiled weight gradients' slabs (gs_dense_wgrad_grouped_tiled3) at small seeded shapes.

    GS_LIB=<library of the commit to pin> python tests/golden/make_tiled3_wgrad_parent_outputs.py     # on the GPU

writes tests/golden/tiled3_wgrad_parent_outputs.npz: per case and problem the logical block [n_slabs, d, out] of the slabs (and
the rows of the riding gather job of the grouped case).  The inputs are not stored: `problems(case, dev)` rebuilds them from the
case's seed, as tests/test_gemm_edges_gpu.py builds its weight-gradient operands (NaN in every pad column and unreferenced table
row, slabs inside sentinel-guarded buffers, the table's last row among the ids of a gathered problem).
tests/test_tiled3_wgrad_golden_gpu.py recomputes every case with the in-tree library in BOTH forms (gs_set_wgrad_tiled3_form) and
compares as float values.  The two forms vouch for each other in tests/test_wgrad_acut_gpu.py; they share their item decode, riders
and epilogue (gs_split.hip, "shared by the tiled3 kernels"), so this file is what a mistake in a shared piece would fail.

The file in the tree was recorded with the library of commit 55f4f81 ("Tiled contractions: steady stages without bookkeeping, no
zero stages"), form 1 -- the last commit in which the three tiled kernels each carried their own copy of those pieces; form 0 of
that library gave the same bits.  Regenerate it only when the kernels' arithmetic is meant to change, and say so in the commit.

Cases (n, d, out, col0, slabs, gathered): one partial stage | 16 * 5 + 3 rows: the register ring and both piece buffers wrap,
masked tail, two m and two n tiles, col0 > 0 | kchunk 32 with three empty slices | 512 + 1 rows: steady rings, the unmasked loop
copy and its seam | two slices, rb > 0 in the hand-advanced dZ base | two problems and a gather job in one launch (item decode
across problems, rider dispatch)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, "tiled3_wgrad_parent_outputs.npz")

# name: (seed, [(n, d, out, col0, slabs, gathered) per problem], gather job (n, s, d) or None)
CASES = {
    "n8": (11, [(8, 6, 41, 0, 1, True)], None),
    "n83": (12, [(83, 70, 136, 128, 1, True)], None),
    "n100_s7": (13, [(100, 6, 136, 0, 7, False)], None),
    "n513": (14, [(513, 7, 8, 0, 1, True)], None),
    "n1040_s2": (15, [(1040, 7, 8, 128, 2, False)], None),
    "grouped": (77, [(200, 70, 41, 0, 3, True), (83, 6, 136, 128, 2, False)], (33, 9, 50)),
}


def _edges():
    tests = os.path.dirname(HERE)
    for p in (tests, os.path.dirname(tests)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import test_gemm_edges_gpu as edges
    return edges


def problems(name, dev):
    """The case's operands on the device: ([_wgrad_problem tuple per problem], GatherJob or None)."""
    edges = _edges()
    seed, shapes, job = CASES[name]
    rng = np.random.default_rng(seed)
    probs = []
    for n, d, out, col0, slabs, gathered in shapes:
        prob = edges._wgrad_problem(dev, rng, n, d, out, col0, slabs, gathered)
        if gathered:                                      # the ids reach the LAST row of the table too
            A, idx_d = prob[0], prob[1]
            last = A.t.shape[0] - 2                       # (In appends one NaN row)
            if not bool((idx_d == last).any()):           # no id drew it: a live row there with the values of the one it replaces
                A.t[last, :d] = A.t[int(idx_d[n // 2]), :d].clone()
                idx_d[n // 2] = last
        probs.append(prob)
    return probs, (edges.GatherJob(dev, rng, job[0], job[1], job[2], False) if job else None)


def run(name, dev, form, check=False):
    """The case through the loaded library in `form` -> {"slabs<i>": [n_slabs, d, out]} (+ {"job": [n, d]}).  check: the slabs (guard
    words, pad columns, float64 bound) and the job's rows are also held to tests/test_gemm_edges_gpu.py's own checks."""
    import torch
    shapes, (probs, job) = CASES[name][1], problems(name, dev)         # (first: it puts the repository on sys.path)
    from graphsage_amd import _lib, ops
    arr = (_lib.WgradDesc * len(probs))()
    for q, (A, idx_d, Z, sl, _, _), (n, d, out, col0, slabs, _) in zip(arr, probs, shapes):
        q.A, q.a_idx, q.dZ, q.slabs = A.ptr, ops.ptr(idx_d), Z.ptr, sl.ptr
        q.lda, q.ldz, q.ld_slab, q.n, q.d, q.col0, q.out_dim, q.n_slabs = A.ld, Z.ld, sl.ld, n, d, col0, out, slabs
        q.a_rows = A.t.shape[0] - 1
    jarr = (_lib.GatherDesc * 1)(*([job.desc] if job else []))
    _lib.set_wgrad_tiled3_form(form)
    try:
        ops.call("gs_dense_wgrad_grouped_tiled3", ctypes.addressof(arr), len(probs), ctypes.addressof(jarr), 1 if job else 0,
                 ops.current_stream())
        torch.cuda.synchronize()
    finally:
        _lib.set_wgrad_tiled3_form(_lib.WGRAD_TILED3_FORM_DEFAULT)
    res = {}
    for i, ((A, idx_d, Z, sl, A_rows, dZ), shape) in enumerate(zip(probs, shapes)):
        if check:
            sl.check(A_rows, dZ, shape[0], "%s problem %d form %d" % (name, i, form))
        got = sl.t.cpu().numpy()[sl.guard:-sl.guard].reshape(sl.n_slabs, sl.d, sl.ld)
        res["slabs%d" % i] = np.ascontiguousarray(got[:, :, :sl.out])
    if job:
        if check:
            job.check()
        res["job"] = np.ascontiguousarray(job.out.read(job.tag))
    return res


def main():
    import torch
    dev = torch.device("cuda")
    doc = {}
    for name in CASES:
        first = run(name, dev, 1, check=True)
        other = run(name, dev, 0, check=True)
        for key, a in first.items():
            assert np.isfinite(a).all(), (name, key)
            assert np.array_equal(a.view(np.uint32), other[key].view(np.uint32)), (name, key, "the two forms differ")
            doc["%s.%s" % (name, key)] = a
        print("%-10s recorded" % name, flush=True)
    target = os.environ.get("TILED3_WGRAD_GOLDEN_OUT", GOLDEN_FILE)
    np.savez_compressed(target, **doc)
    print("wrote %s (%d bytes)" % (target, os.path.getsize(target)))


if __name__ == "__main__":
    main()
