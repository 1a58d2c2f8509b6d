"""gs_dense_wgrad_grouped_tiled3 in its two forms (gs_set_wgrad_tiled3_form): wgrad_tiled3_acut_kernel, which cuts the A rows once
per workgroup, against wgrad_tiled3_kernel on the same operands.  The slab buffers must be BITWISE equal (same pieces, same
MFMA sequence per accumulator), and the new form must meet gemm_oracle's float64 bound on its own.  Operands as in
test_gemm_edges_gpu.py: NaN in every pad column / unreferenced table row, outputs inside sentinel-filled buffers."""
import ctypes

import numpy as np
import pytest
import torch

from graphsage_amd import _lib, ops
import gemm_oracle as go
from test_gemm_edges_gpu import GatherJob, Slabs, _wgrad_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _library_default_afterwards():
    yield
    _lib.set_wgrad_tiled3_form(_lib.WGRAD_TILED3_FORM_DEFAULT)


def _descs(probs, shapes):
    arr = (_lib.WgradDesc * len(probs))()
    for q, (A, idx_d, Z, sl, _, _), (n, d, out, col0, slabs) in zip(arr, probs, shapes):
        q.A, q.a_idx, q.dZ, q.slabs = A.ptr, ops.ptr(idx_d), Z.ptr, sl.ptr
        q.lda, q.ldz, q.ld_slab, q.n, q.d, q.col0, q.out_dim, q.n_slabs = A.ld, Z.ld, sl.ld, n, d, col0, out, slabs
        q.a_rows = A.t.shape[0] - 1
    return arr


def _both_forms(dev, probs, shapes, jobs=()):
    """Launches the problems in form 0 into their own slabs and in form 1 into a second set; returns the second set."""
    jarr = (_lib.GatherDesc * max(len(jobs), 1))(*[j.desc for j in jobs])
    new = [Slabs(dev, sl.n_slabs, sl.d, sl.out) for (_, _, _, sl, _, _) in probs]
    for form, slabs in ((0, [p[3] for p in probs]), (1, new)):
        _lib.set_wgrad_tiled3_form(form)
        arr = _descs([p[:3] + (sl,) + p[4:] for p, sl in zip(probs, slabs)], shapes)
        ops.call("gs_dense_wgrad_grouped_tiled3", ctypes.addressof(arr), len(probs), ctypes.addressof(jarr), len(jobs),
                 ops.current_stream())
    torch.cuda.synchronize()
    for p, sl, shape in zip(probs, new, shapes):
        a, b = p[3].t.cpu().numpy().view(np.uint32), sl.t.cpu().numpy().view(np.uint32)
        assert np.array_equal(a, b), "problem %r: %d words of the two forms' slab buffers differ" % (shape, int((a != b).sum()))
    return new


# (n, d, out, col0, slabs): one partial stage, shorter than the rings | 16 * 5 + 3 rows in one slab: the register ring and both
# piece buffers wrap, masked tail | 3 slabs of kchunk 96, the last slice 8 rows | kchunk 32: three EMPTY slices of 7 |
# d = 6 / 70 / 130: one nearly empty, two and three m tiles; out = 41 / 136: one and two n tiles; col0 = 0 / 128
CASES = [(8, 6, 41, 0, 1), (83, 70, 136, 128, 1), (200, 130, 41, 128, 3), (100, 6, 136, 0, 7), (83, 130, 136, 0, 2)]


@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("n,d,out,col0,slabs", CASES)
def test_acut_form_is_bitwise_the_first_form(dev, n, d, out, col0, slabs, gathered):
    rng = np.random.default_rng(1000 * n + d + out + col0 + gathered)
    prob = _wgrad_problem(dev, rng, n, d, out, col0, slabs, gathered)
    if gathered:                                      # the ids reach the LAST row of the table too (and repeat: _table)
        A, idx_d, Z, sl, A_rows, dZ = prob
        last = A.t.shape[0] - 2                       # (In appends one NaN row)
        if not bool((idx_d == last).any()):           # no id drew it: a live row there with the values of the one it replaces,
            A.t[last, :d] = A.t[int(idx_d[n // 2]), :d].clone()                   # so A_rows stays the logical operand
            idx_d[n // 2] = last
    new = _both_forms(dev, [prob], [(n, d, out, col0, slabs)])
    tag = "acut n=%d d=%d out=%d col0=%d slabs=%d gathered=%d" % (n, d, out, col0, slabs, gathered)
    new[0].check(prob[4], prob[5], n, tag)
    if slabs == 7:
        assert [b - a for a, b in go.slab_rows(n, slabs)].count(0) == 3


def test_acut_form_grouped_with_a_gather_rider(dev):
    """Two problems in one launch (one gathered), one gather+mean job riding behind them: both forms, and the job's rows."""
    rng = np.random.default_rng(77)
    shapes = [(200, 70, 41, 0, 3), (83, 6, 136, 128, 2)]
    probs = [_wgrad_problem(dev, rng, n, d, out, col0, slabs, gathered=(i == 0))
             for i, (n, d, out, col0, slabs) in enumerate(shapes)]
    job = GatherJob(dev, rng, 33, 9, 50, False)
    new = _both_forms(dev, probs, shapes, jobs=[job])
    for p, sl, shape in zip(probs, new, shapes):
        sl.check(p[4], p[5], shape[0], "acut grouped %r" % (shape,))
    job.check()


def test_form_setter_refuses_unknown_forms(dev):
    with pytest.raises(_lib.GraphsageAmdError):
        _lib.set_wgrad_tiled3_form(2)
