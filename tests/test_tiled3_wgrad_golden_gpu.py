"""-m gpu: gs_dense_wgrad_grouped_tiled3 in both forms against slabs recorded with the library of an earlier commit
(tests/golden/tiled3_wgrad_parent_outputs.npz, tests/golden/make_tiled3_wgrad_parent_outputs.py: the kernels that each carried
their own item decode, rider dispatch and slab epilogue).  tests/test_wgrad_acut_gpu.py holds the two forms to each other; they
share those pieces now, so a mistake in one of them would pass there and fails here.  Every slab value (and every row of the riding
gather job) must compare equal AS A FLOAT VALUE (`==`) -- no tolerance -- and be finite; guard words, pad columns and the float64
bound are checked as in tests/test_gemm_edges_gpu.py."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_tiled3_wgrad_parent_outputs",
    os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_tiled3_wgrad_parent_outputs.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with np.load(rec.GOLDEN_FILE) as z:
        return {k: z[k] for k in z.files}


def test_golden_file_covers_every_case(golden):
    want = {"%s.slabs%d" % (n, i) for n, c in rec.CASES.items() for i in range(len(c[1]))}
    want |= {"%s.job" % n for n, c in rec.CASES.items() if c[2]}
    assert set(golden) == want
    assert os.path.getsize(rec.GOLDEN_FILE) <= 113 * 1024


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", sorted(rec.CASES))
def test_wgrad_tiled3_equals_the_recorded_slabs(dev, golden, name, form):
    got = rec.run(name, dev, form, check=True)
    for key, a in got.items():
        want = golden["%s.%s" % (name, key)]
        assert a.shape == want.shape and a.dtype == want.dtype
        assert np.isfinite(a).all()
        diff = int((a != want).sum())
        assert diff == 0, "%s.%s form %d: %d of %d values differ from the recorded ones (max |diff| %g)" % (
            name, key, form, diff, a.size, float(np.abs(a.astype(np.float64) - want).max()))
