"""-m gpu: the five tail kernels (gs_sage_tail_fwd_bwd, gs_sage_tail_z, gs_sage_tail_dh0, gs_linkpred_tail, gs_linkpred_tail_neg)
against outputs recorded with the library of an earlier commit (tests/golden/tail_parent_outputs.npz,
tests/golden/make_tail_parent_outputs.py: the kernels that each carried their own copy of the relu-mask, input-gradient, d_h0-store,
l2-normalise and z-helper bodies).  They share those bodies now (csrc/gs_tail_dev.h), so the tests that hold one launch to another
(split to fused, means_ready to computed means) would pass a mistake in a shared piece; it fails here.  Every value of every output
must be finite and compare equal AS A FLOAT VALUE to the recorded one -- no tolerance; outputs above 8 KB are compared through the
SHA-256 of their bytes with -0 folded to +0.  The hand-over error word is 0 after every case (asserted by `run`)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_tail_parent_outputs", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_tail_parent_outputs.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    return rec.load()


def test_golden_file_covers_every_case(golden):
    assert {k.split(".", 1)[0] for k in golden} == set(rec.CASES) and len(set(rec.CASES)) == 13 + 4 + 4
    assert os.path.getsize(rec.GOLDEN_FILE) <= 113 * 1024


@pytest.mark.parametrize("name", rec.CASES)
def test_tail_equals_the_recorded_outputs(dev, golden, name):
    got = rec.run(name, dev)
    assert {"%s.%s" % (name, k) for k in got} == {k for k in golden if k.split(".", 1)[0] == name}
    for key, a in got.items():
        a = np.ascontiguousarray(a)
        want = golden["%s.%s" % (name, key)]
        assert a.dtype == np.float32 and np.isfinite(a).all(), "%s.%s is not finite" % (name, key)
        if want[0] == "whole":
            assert a.shape == want[1].shape
            diff = int((a != want[1]).sum())
            assert diff == 0, "%s.%s: %d of %d values differ from the recorded ones (max |diff| %g)" % (
                name, key, diff, a.size, float(np.abs(a.astype(np.float64) - want[1]).max()))
        else:
            assert a.nbytes > rec.WHOLE_BYTES
            if not np.array_equal(rec.digest(a), want[1]):
                moved = "no column sums recorded"
                if want[2] is not None:
                    d = rec.colsum(a) - want[2]
                    moved = "float64 column sums differ in columns %s (largest difference %g)" % (np.flatnonzero(d)[:16].tolist(), float(np.abs(d).max()))
                pytest.fail("%s.%s: the SHA-256 of its values differs from the recorded one; %s" % (name, key, moved))
