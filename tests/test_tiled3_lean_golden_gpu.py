"""-m gpu: gs_sage_dense_fwd_tiled3 / _means against outputs recorded with the library of an earlier commit
(tests/golden/tiled3_parent_outputs.npz, tests/golden/make_tiled3_parent_outputs.py: the kernel that still padded its K loop to
whole rings with stages of zeros and ran every stage with selects and clamps).  The stage kinds of the current kernel and the
dropped stages of zeros change no term of any sum but `+ 0`: every output must compare equal AS A FLOAT VALUE (`==`: -0 equals
+0) -- no tolerance."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_tiled3_parent_outputs", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_tiled3_parent_outputs.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with np.load(rec.GOLDEN_FILE) as z:
        return {k: z[k] for k in z.files}


def test_golden_file_covers_every_case(golden):
    want = {"%s.out" % n for n in rec.CASES} | {"%s.means" % n for n, c in rec.CASES.items() if c[8]}
    assert set(golden) == want


@pytest.mark.parametrize("name", sorted(rec.CASES))
def test_fwd_tiled3_equals_the_recorded_outputs(dev, golden, name):
    got = rec.run(name, dev)
    for key, a in got.items():
        want = golden["%s.%s" % (name, key)]
        assert a.shape == want.shape and a.dtype == want.dtype
        assert np.isfinite(a).all()
        diff = int((a != want).sum())
        assert diff == 0, "%s.%s: %d of %d values differ from the recorded ones (max |diff| %g)" % (
            name, key, diff, a.size, float(np.abs(a.astype(np.float64) - want).max()))
